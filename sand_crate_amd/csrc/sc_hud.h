// The HUD overlay (sc_set_hud): the text of Playback.draw_debug_text (playback.py:215-219) written in white over a
// frame that resolve has finished -- H x W x 3 RGB (k_render_resolve) or H x W palette indices (k_render_resolve_index,
// where white is index 255) -- before an encoder reads it.  The pixel rule is specified in NumPy by tests/text_spec.py;
// this kernel reproduces it bit for bit.  Included once by sandcrate_hip.hip.
//
// The grid covers the text's bounding box clipped to the frame, one thread per pixel, a wave along 64 pixels of a
// row.  A thread finds its line (start and length, a table built on the host), its character and the glyph's row,
// and stores only where the glyph has a bit set: byte stores into its own pixel, nothing read from the frame, so the
// frame may start at any address and no thread touches a neighbour's pixel.
#pragma once
#include "sc_device.h"
#include "sc_font.h"

namespace sc {

constexpr int kHudPitch = 18;       // rows of cell pixels from one line to the next: 16 of glyph, 2 of leading
constexpr int kHudMaxBytes = 65536;
constexpr int kHudMaxScale = 64;
constexpr int kHudTileW = 64, kHudTileH = kBlock / kHudTileW;  // a workgroup's pixels: a wave per row

struct HudFont {
  unsigned char rows[(kFontLast - kFontFirst + 1) * kFontRows];
};

constexpr HudFont make_hud_font() {
  HudFont f{};
  for (int k = 0; k < (int)sizeof f.rows; ++k) f.rows[k] = kFontTable[k];
  return f;
}

__constant__ HudFont kHudFont = make_hud_font();

struct HudLine {
  int start, length;  // in bytes of the text
};

struct HudBox {
  int width;    // of the frame, pixels
  int x0, y0;   // the text's origin
  int bw, bh;   // the bounding box clipped to the frame: x0 + bw <= width, y0 + bh <= height, bh <= lines * pitch * scale
  int scale;
};

// INDEX: the frame is one palette index per pixel, else three bytes r, g, b.
template <bool INDEX>
__global__ void __launch_bounds__(kBlock) k_hud_overlay(HudBox b, const unsigned char* __restrict__ text,
                                                        const HudLine* __restrict__ lines, unsigned char* __restrict__ frame) {
  const int bx = (int)blockIdx.x * kHudTileW + (int)(threadIdx.x & 63u);
  const int by = (int)blockIdx.y * kHudTileH + (int)(threadIdx.x >> 6);
  if (bx >= b.bw || by >= b.bh) return;
  const int cy = by / b.scale, cx = bx / b.scale;  // in cell pixels
  const int line = cy / kHudPitch, row = cy - line * kHudPitch;
  if (row >= kFontRows) return;  // leading
  const HudLine ln = lines[line];
  const int k = cx / kFontCols;
  if (k >= ln.length) return;  // past the end of a short line
  unsigned ch = text[ln.start + k];
  if (ch < (unsigned)kFontFirst || ch > (unsigned)kFontLast) ch = '?';
  const unsigned bits = kHudFont.rows[(ch - kFontFirst) * kFontRows + row];
  if (!(bits & (0x80u >> (cx - k * kFontCols)))) return;
  const size_t p = (size_t)(b.y0 + by) * (size_t)b.width + (size_t)(b.x0 + bx);
  if (INDEX) {
    frame[p] = 255;
  } else {
    frame[3 * p] = 255;
    frame[3 * p + 1] = 255;
    frame[3 * p + 2] = 255;
  }
}

}  // namespace sc
