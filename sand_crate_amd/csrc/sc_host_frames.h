// Host side of the frames: rendering with its HUD and arrows, and the JPEG and GIF encoders.
#pragma once
#include "sc_host.h"
#include "sc_arrows.h"
#include "sc_gif.h"
#include "sc_hud.h"
#include "sc_jpeg.h"
#include "sc_render.h"

extern "C" {

// ---- rendering (sc_render.h) ------------------------------------------------------------------

constexpr int kRenderMaxSide = 16384;
constexpr long long kRenderMaxRadius = 1LL << 24;  // keeps the squared pixel distances of a disc exact in 64 bits

// A workspace's parts start at multiples of 256 bytes.
constexpr int64_t carve_up(int64_t n) { return (n + 255) & ~(int64_t)255; }

// The frame sizes every call here takes (`ok`: what the call checks in the same breath).
static int check_frame(int width, int height, bool ok = true) {
  if (width < 1 || width > kRenderMaxSide || height < 1 || height > kRenderMaxSide || !ok)
    return fail(SC_ERR_ARG, "frame of %d x %d pixels; each side 1..%d", width, height, kRenderMaxSide);
  return SC_OK;
}

// Checks the call, turns the view and the walls into the kernels' argument and selects the context's device.
static int render_prepare(sc_ctx* c, const sc_view* view, const double* segments, int32_t ns, bool has_frame, RenderView& v) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "rendering happens between ticks");
  if (!view || !has_frame) return fail(SC_ERR_ARG, "null view or frame");
  const sc_view& q = *view;
  if (const int rc = check_frame(q.width, q.height)) return rc;
  if (!(std::isfinite(q.zoom) && q.zoom > 0)) return fail(SC_ERR_ARG, "zoom must be finite and positive");
  if (!std::isfinite(q.center_x) || !std::isfinite(q.center_y)) return fail(SC_ERR_ARG, "the view center must be finite");
  if (!(std::isfinite(q.particle_radius) && q.particle_radius >= 0))
    return fail(SC_ERR_ARG, "particle_radius must be finite and not negative");
  if (q.segment_width < 0) return fail(SC_ERR_ARG, "segment_width must not be negative");
  if (ns < 0 || ns > kMaxSeg) return fail(SC_ERR_ARG, "%d segments, at most %d", ns, kMaxSeg);
  if (ns > 0 && !segments) return fail(SC_ERR_ARG, "null segments");
  v = RenderView{};
  v.width = q.width;
  v.height = q.height;
  v.center_x = q.center_x;
  v.center_y = q.center_y;
  v.zoom = q.zoom;
  v.half_w = q.width / 2.0;
  v.half_h = q.height / 2.0;
  v.sx = q.width - 1.0;
  v.sy = q.height - 1.0;
  // playback.py:195: int(screen_x * particle_radius) * zoom_factor, floored to whole pixels
  const double R = std::floor(std::trunc(q.width * q.particle_radius) * q.zoom);
  if (!(R <= (double)kRenderMaxRadius)) return fail(SC_ERR_ARG, "disc radius of %g pixels, at most %lld", R, kRenderMaxRadius);
  v.radius = (long long)R;
  v.radius_d = R;
  v.w2 = (double)q.segment_width * q.segment_width;
  const double margin = q.segment_width + 1.0;
  for (int k = 0; k < ns; ++k) {
    const double* e = segments + 4 * k;
    // the same view as the particles', not floored (playback.py:180-186 hands these to pygame.draw.line)
    const double ax = (std::trunc(e[0] * v.sx) - v.center_x) * v.zoom + v.half_w;
    const double ay = (std::trunc(e[1] * v.sy) - v.center_y) * v.zoom + v.half_h;
    const double bx = (std::trunc(e[2] * v.sx) - v.center_x) * v.zoom + v.half_w;
    const double by = (std::trunc(e[3] * v.sy) - v.center_y) * v.zoom + v.half_h;
    if (!std::isfinite(ax) || !std::isfinite(ay) || !std::isfinite(bx) || !std::isfinite(by)) continue;  // covers nothing
    RenderSeg& r = v.seg[v.nseg++];
    r.ax = ax;
    r.ay = ay;
    r.dx = bx - ax;
    r.dy = by - ay;
    r.len2 = r.dx * r.dx + r.dy * r.dy;
    // the closest point a + t (b - a), t in [0, 1], lies between a and the ROUNDED a + (b - a)
    const double ex = ax + r.dx, ey = ay + r.dy;
    r.lox = std::min({ax, bx, ex}) - margin;
    r.hix = std::max({ax, bx, ex}) + margin;
    r.loy = std::min({ay, by, ey}) - margin;
    r.hiy = std::max({ay, by, ey}) + margin;
  }
  HIPCHK(hipSetDevice(c->device));
  return SC_OK;
}

// Enqueues the HUD overlay over a resolved frame: over the text's bounding box clipped to the frame, or not at all
// when there is no HUD or the box is empty.
static void hud_launch(sc_ctx* c, const RenderView& v, unsigned char* frame, bool as_index) {
  if (c->frame.hud_lines == 0) return;
  const long long bw = std::min<long long>(v.width - c->frame.hud_x, (long long)c->frame.hud_longest * kFontCols * c->frame.hud_scale);
  const long long bh = std::min<long long>(v.height - c->frame.hud_y, (long long)c->frame.hud_lines * kHudPitch * c->frame.hud_scale);
  if (bw <= 0 || bh <= 0) return;
  const HudBox b{v.width, c->frame.hud_x, c->frame.hud_y, (int)bw, (int)bh, c->frame.hud_scale};
  const dim3 grid((unsigned)((bw + kHudTileW - 1) / kHudTileW), (unsigned)((bh + kHudTileH - 1) / kHudTileH));
  if (as_index)
    hipLaunchKernelGGL(k_hud_overlay<true>, grid, dim3(kBlock), 0, c->stream, b, c->frame.hudText, c->frame.hudLines, frame);
  else
    hipLaunchKernelGGL(k_hud_overlay<false>, grid, dim3(kBlock), 0, c->stream, b, c->frame.hudText, c->frame.hudLines, frame);
}

// Enqueues the arrow pass over a resolved frame: a wave per kArrowListPerWave arrows of the list, or a thread per slot
// under the host's bound of the live count, or nothing at all when no arrows are set.
static void arrows_launch(sc_ctx* c, const RenderView& v, unsigned char* frame, bool as_index) {
  if (c->frame.arrow_mode == SC_ARROWS_OFF) return;
  const bool from_list = c->frame.arrow_mode == SC_ARROWS_LIST;
  const int64_t count = from_list ? c->frame.arrow_n : slot_bound(c);
  if (count <= 0) return;
  const ArrowView a{v.width, v.height, v.center_x, v.center_y, v.zoom, v.half_w, v.half_h, v.sx, v.sy};
  const sc_arrow* list = from_list ? c->frame.arrowList.get() : nullptr;
  const int64_t threads = from_list ? (count + kArrowListPerWave - 1) / kArrowListPerWave * 64 : count;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(threads)), dim3(kBlock), 0, c->stream, a, list, (int)count, c->counters, c->x,
                       c->y, c->vx, c->vy, c->id[0], c->frame.arrow_scale, (long long)c->frame.arrow_every, frame);
  };
  as_index ? launch(k_arrows<true>) : launch(k_arrows<false>);
}

// Grows the key buffer and enqueues splat, resolve, the arrows and the HUD overlay into `rgb` (device memory), or with
// `as_index` the resolve that writes one palette index per pixel into it (4-byte aligned).
static int render_launch(sc_ctx* c, const RenderView& v, unsigned char* rgb, bool as_index = false) {
  const int64_t pixels = (int64_t)v.width * v.height;
  if (pixels > c->frame.keys.size()) {
    HIPCHK(c->frame.keys.grow(pixels, c->stream));
    // zero once: every resolve clears the keys it reads, which are all that the splat before it may have set
    HIPCHK(hipMemsetAsync(c->frame.keys, 0, c->frame.keys.bytes(), c->stream));
  }
  const int64_t bound = slot_bound(c);
  if (bound > 0) {
    if (v.radius > kRenderWaveRadius)
      hipLaunchKernelGGL(k_render_splat<true>, dim3((unsigned)((bound * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                         v, c->counters, c->x, c->y, c->id[0], c->P, c->normals_valid ? 1 : 0, (int)bound, c->frame.keys);
    else
      hipLaunchKernelGGL(k_render_splat<false>, dim3(grid_for(bound)), dim3(kBlock), 0, c->stream, v, c->counters, c->x,
                         c->y, c->id[0], c->P, c->normals_valid ? 1 : 0, (int)bound, c->frame.keys);
  }
  if (as_index)
    hipLaunchKernelGGL(k_render_resolve_index, dim3(grid_for((pixels + 3) / 4)), dim3(kBlock), 0, c->stream, v, c->frame.keys,
                       rgb, c->frame.arrow_mode == SC_ARROWS_OFF ? 1u : 2u);  // (entry 1 is the arrows' when there are any)
  else
    hipLaunchKernelGGL(k_render_resolve, dim3(grid_for((pixels + 3) / 4)), dim3(kBlock), 0, c->stream, v, c->frame.keys, rgb,
                       ((uintptr_t)rgb & 3) == 0 ? 1 : 0);
  arrows_launch(c, v, rgb, as_index);
  hud_launch(c, v, rgb, as_index);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

int sc_set_hud(sc_ctx* c, const char* text, int32_t n_bytes, int32_t x, int32_t y, int32_t scale) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (n_bytes < 0 || n_bytes > kHudMaxBytes) return fail(SC_ERR_ARG, "HUD text of %d bytes; 0..%d", n_bytes, kHudMaxBytes);
  if (n_bytes > 0 && !text) return fail(SC_ERR_ARG, "null HUD text");
  if (x < 0 || x > kRenderMaxSide || y < 0 || y > kRenderMaxSide)
    return fail(SC_ERR_ARG, "HUD origin (%d, %d); each coordinate 0..%d", x, y, kRenderMaxSide);
  if (scale < 1 || scale > kHudMaxScale) return fail(SC_ERR_ARG, "HUD scale %d; 1..%d", scale, kHudMaxScale);
  HIPCHK(hipSetDevice(c->device));
  c->frame.hud_lines = 0;  // (a call that fails below leaves no HUD)
  if (n_bytes > 0) {
    // the lines as str.split("\n") cuts them: a trailing newline yields an empty last line
    std::vector<HudLine> lines;
    int start = 0, longest = 0;
    for (int k = 0; k <= n_bytes; ++k) {
      if (k < n_bytes && text[k] != '\n') continue;
      lines.push_back(HudLine{start, k - start});
      longest = std::max(longest, k - start);
      start = k + 1;
    }
    HIPCHK(c->frame.hudText.grow(n_bytes, c->stream));
    HIPCHK(c->frame.hudLines.grow((int64_t)lines.size(), c->stream));
    HIPCHK(hipMemcpyAsync(c->frame.hudText, text, (size_t)n_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->frame.hudLines, lines.data(), lines.size() * sizeof(HudLine), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // `text` and `lines` are the caller's and ours: read before we return
    c->frame.hud_longest = longest;
    c->frame.hud_x = x;
    c->frame.hud_y = y;
    c->frame.hud_scale = scale;
    c->frame.hud_lines = (int)lines.size();
    return SC_OK;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return SC_OK;
}

int sc_set_arrows(sc_ctx* c, int32_t mode, const sc_arrow* arrows, int64_t n, double scale, int64_t every) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "the arrows are set between ticks");
  if (mode != SC_ARROWS_OFF && mode != SC_ARROWS_LIST && mode != SC_ARROWS_VELOCITY)
    return fail(SC_ERR_ARG, "arrow mode %d; SC_ARROWS_OFF, _LIST or _VELOCITY", mode);
  // (every argument is checked in every mode: a caller's mistake shows at once, not when the mode changes)
  if (n < 0 || n > kArrowMaxList) return fail(SC_ERR_ARG, "%lld arrows; 0..%lld", (long long)n, kArrowMaxList);
  if (n > 0 && !arrows) return fail(SC_ERR_ARG, "null arrow list");
  if (every < 1) return fail(SC_ERR_ARG, "an arrow for every %lld-th particle; at least 1", (long long)every);
  if (!std::isfinite(scale)) return fail(SC_ERR_ARG, "the arrows' scale must be finite");
  HIPCHK(hipSetDevice(c->device));
  c->frame.arrow_mode = SC_ARROWS_OFF;  // (a call that fails below leaves no arrows)
  if (mode == SC_ARROWS_LIST && n > 0) {
    HIPCHK(c->frame.arrowList.grow(n, c->stream));
    HIPCHK(hipMemcpyAsync(c->frame.arrowList, arrows, (size_t)n * sizeof(sc_arrow), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));  // `arrows` is the caller's: read before we return
  if (mode == SC_ARROWS_LIST && n > 0) {
    c->frame.arrow_n = n;
    c->frame.arrow_mode = SC_ARROWS_LIST;
  } else if (mode == SC_ARROWS_VELOCITY) {
    c->frame.arrow_scale = scale;
    c->frame.arrow_every = every;
    c->frame.arrow_mode = SC_ARROWS_VELOCITY;
  }
  return SC_OK;
}

int sc_render_device(sc_ctx* c, const sc_view* view, const double* segments, int32_t n_segments, uint8_t* dev_rgb) {
  RenderView v;
  if (const int rc = render_prepare(c, view, segments, n_segments, dev_rgb != nullptr, v)) return rc;
  return render_launch(c, v, dev_rgb);
}

int sc_render(sc_ctx* c, const sc_view* view, const double* segments, int32_t n_segments, uint8_t* rgb) {
  RenderView v;
  int rc = render_prepare(c, view, segments, n_segments, rgb != nullptr, v);
  if (rc) return rc;
  const int64_t bytes = 3 * (int64_t)v.width * v.height;
  HIPCHK(c->frame.rgb.grow(bytes, c->stream));
  if ((rc = render_launch(c, v, c->frame.rgb))) return rc;
  return read_back(c, rgb, c->frame.rgb, (size_t)bytes);
}

// ---- JPEG encoding (sc_jpeg.h) -------------------------------------------------------------------

constexpr int kJpegHeaderBytes = 613;  // SOI, APP0, DQT, SOF0, DHT, DRI, SOS as jpeg_header writes them

static void jpeg_quant(int quality, int q[2][64]) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int k = 0; k < 64; ++k) {
    q[0][k] = std::min(255, std::max(1, (kJpegLumaQ[k] * s + 50) / 100));
    q[1][k] = std::min(255, std::max(1, (kJpegChromaQ[k] * s + 50) / 100));
  }
}

// SOI through SOS (tests/jpeg_spec.py: header).
static std::vector<unsigned char> jpeg_header(int width, int height, const int q[2][64]) {
  std::vector<unsigned char> h;
  auto u8 = [&](int v) { h.push_back((unsigned char)v); };
  auto u16 = [&](int v) { u8(v >> 8); u8(v & 0xFF); };
  u16(0xFFD8);
  u16(0xFFE0); u16(16);
  for (char ch : {'J', 'F', 'I', 'F', '\0'}) u8(ch);
  u8(1); u8(1); u8(0); u16(1); u16(1); u8(0); u8(0);
  u16(0xFFDB); u16(2 + 2 * 65);
  for (int t = 0; t < 2; ++t) {
    unsigned char zz[64];
    for (int k = 0; k < 64; ++k) zz[kJpegZigzag.of[k]] = (unsigned char)q[t][k];
    u8(t);
    for (int k = 0; k < 64; ++k) u8(zz[k]);
  }
  u16(0xFFC0); u16(17); u8(8); u16(height); u16(width); u8(3);
  for (int id = 1; id <= 3; ++id) { u8(id); u8(0x11); u8(id == 1 ? 0 : 1); }
  u16(0xFFC4); u16(2 + 2 * (17 + 12) + 2 * (17 + 162));
  for (int t = 0; t < 2; ++t) {
    u8(t);
    for (int k = 0; k < 16; ++k) u8(kJpegDcBits[t][k]);
    for (int k = 0; k < 12; ++k) u8(kJpegDcVals[k]);
    u8(0x10 | t);
    for (int k = 0; k < 16; ++k) u8(kJpegAcBits[t][k]);
    for (int k = 0; k < 162; ++k) u8(kJpegAcVals[t][k]);
  }
  u16(0xFFDD); u16(4); u16((width + 7) / 8);
  u16(0xFFDA); u16(12); u8(3);
  for (int id = 1; id <= 3; ++id) { u8(id); u8(id == 1 ? 0x00 : 0x11); }
  u8(0); u8(63); u8(0);
  return h;
}

int sc_jpeg_bound(int32_t width, int32_t height, int64_t* bound) {
  if (const int rc = check_frame(width, height, bound != nullptr)) return rc;
  const int64_t mcus = (width + 7) / 8, rows = (height + 7) / 8;
  const int64_t row_bytes = (3 * mcus * kJpegBlockBits + 7) / 8;
  *bound = kJpegHeaderBytes + rows * (2 * row_bytes + 2) + 2;  // every byte 0xFF, a marker after each row, EOI
  return SC_OK;
}

// Encodes the W x H x 3 RGB frame at `rgb` (device memory, checked by the caller) into `out` (host memory).
// Enqueued on the context's stream; synchronises twice: for the total length, then for the bytes.
static int jpeg_encode(sc_ctx* c, const unsigned char* rgb, int width, int height, int quality, uint8_t* out,
                       int64_t capacity, int64_t* n_out) {
  JpegDims d;
  d.width = width;
  d.height = height;
  d.mcus = (width + 7) / 8;
  d.rows = (height + 7) / 8;
  jpeg_quant(quality, d.quant);
  const int64_t nblocks = (int64_t)d.rows * d.mcus * 3;
  const long long row_words = (3LL * d.mcus * kJpegBlockBits + 7) / 32 + 1;  // a row's bits, padded
  // the workspace: coef | masks | acbits | rows' bit buffers | row bytes, row lengths | row offsets + total
  const int64_t o_mask = carve_up(nblocks * 64 * (int64_t)sizeof(short));
  const int64_t o_ac = o_mask + carve_up(nblocks * (int64_t)sizeof(unsigned long long));
  const int64_t o_rows = o_ac + carve_up(nblocks * (int64_t)sizeof(int));
  const int64_t o_len = o_rows + carve_up((int64_t)d.rows * row_words * (int64_t)sizeof(unsigned));
  const int64_t o_off = o_len + carve_up(2 * (int64_t)d.rows * (int64_t)sizeof(int));
  const int64_t bytes = o_off + carve_up(((int64_t)d.rows + 1) * (int64_t)sizeof(long long));
  HIPCHK(c->jpeg.work.grow(bytes, c->stream));
  unsigned char* w = c->jpeg.work;
  short* coef = (short*)w;
  unsigned long long* masks = (unsigned long long*)(w + o_mask);
  int* acbits = (int*)(w + o_ac);
  unsigned* rowbuf = (unsigned*)(w + o_rows);
  int* row_bytes = (int*)(w + o_len);
  int* row_len = row_bytes + d.rows;
  long long* row_off = (long long*)(w + o_off);

  hipLaunchKernelGGL(k_jpeg_dct, dim3((unsigned)((nblocks * 8 + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, d, rgb,
                     coef, masks, acbits);
  hipLaunchKernelGGL(k_jpeg_rows, dim3((unsigned)d.rows), dim3(64), 0, c->stream, d, coef, masks, acbits, rowbuf, row_words,
                     row_bytes, row_len);
  hipLaunchKernelGGL(k_jpeg_scan, dim3(1), dim3(64), 0, c->stream, d.rows, row_len, row_off);
  HIPCHK(hipGetLastError());
  long long total = 0;
  int rc = read_back(c, &total, row_off + d.rows, sizeof total);
  if (rc) return rc;
  const std::vector<unsigned char> hdr = jpeg_header(width, height, d.quant);
  const int64_t need = (int64_t)hdr.size() + total + 2;
  if ((rc = refuse_room(need, capacity, n_out, "the JPEG takes %lld bytes, the buffer holds %lld"))) return rc;
  HIPCHK(c->jpeg.out.grow(total, c->stream));
  hipLaunchKernelGGL(k_jpeg_stuff, dim3((unsigned)d.rows), dim3(64), 0, c->stream, d.rows, rowbuf, row_words, row_bytes,
                     row_off, c->jpeg.out);
  HIPCHK(hipGetLastError());
  std::memcpy(out, hdr.data(), hdr.size());
  if ((rc = read_back(c, out + hdr.size(), c->jpeg.out, (size_t)total))) return rc;
  out[need - 2] = 0xFF;
  out[need - 1] = 0xD9;
  return SC_OK;
}

static int jpeg_check(sc_ctx* c, int quality, const uint8_t* out, int64_t capacity, const int64_t* n_out) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "encoding happens between ticks");
  if (quality < 1 || quality > 100) return fail(SC_ERR_ARG, "quality %d, expected 1..100", quality);
  if (!n_out || capacity < 0 || (!out && capacity > 0)) return fail(SC_ERR_ARG, "null n_out, or a negative capacity, or a null buffer");
  return SC_OK;
}

int sc_jpeg_encode_device(sc_ctx* c, const uint8_t* dev_rgb, int32_t width, int32_t height, int32_t quality, uint8_t* out,
                          int64_t capacity, int64_t* n_out) {
  int rc = jpeg_check(c, quality, out, capacity, n_out);
  if (rc) return rc;
  if (!dev_rgb) return fail(SC_ERR_ARG, "null frame");
  if ((rc = check_frame(width, height))) return rc;
  HIPCHK(hipSetDevice(c->device));
  return jpeg_encode(c, dev_rgb, width, height, quality, out, capacity, n_out);
}

int sc_render_jpeg(sc_ctx* c, const sc_view* view, const double* segments, int32_t n_segments, int32_t quality, uint8_t* out,
                   int64_t capacity, int64_t* n_out) {
  int rc = jpeg_check(c, quality, out, capacity, n_out);
  if (rc) return rc;
  RenderView v;
  if ((rc = render_prepare(c, view, segments, n_segments, true, v))) return rc;
  HIPCHK(c->frame.rgb.grow(3 * (int64_t)v.width * v.height, c->stream));
  if ((rc = render_launch(c, v, c->frame.rgb))) return rc;
  return jpeg_encode(c, c->frame.rgb, v.width, v.height, quality, out, capacity, n_out);
}

// ---- GIF encoding (sc_gif.h) ---------------------------------------------------------------------

int sc_gif_bound(int32_t width, int32_t height, int64_t* bound) {
  if (const int rc = check_frame(width, height, bound != nullptr)) return rc;
  const int64_t pixels = (int64_t)width * height, chunks = (pixels + kGifChunk - 1) / kGifChunk;
  const int64_t bytes = (11 * (pixels + chunks + 1) + 7) / 8;  // a code per pixel, a clear per chunk, the end code
  *bound = 2 + bytes + (bytes + 254) / 255;                    // minimum code size, sub-block lengths, terminator
  return SC_OK;
}

// Encodes the W x H palette indices at `index` (device memory, checked by the caller) into `out` (host memory).
// Enqueued on the context's stream; synchronises twice: for the total length, then for the bytes.
static int gif_encode(sc_ctx* c, const unsigned char* index, int width, int height, uint8_t* out, int64_t capacity,
                      int64_t* n_out) {
  const int64_t pixels = (int64_t)width * height, chunks = (pixels + kGifChunk - 1) / kGifChunk;
  // the workspace: codes | code counts | bit offsets + the end code's, the two totals
  const int64_t o_count = carve_up(chunks * kGifChunk * (int64_t)sizeof(unsigned short));
  const int64_t o_off = o_count + carve_up(chunks * (int64_t)sizeof(int));
  HIPCHK(c->gif.work.grow(o_off + carve_up((chunks + 3) * (int64_t)sizeof(long long)), c->stream));
  unsigned char* w = c->gif.work;
  unsigned short* codes = (unsigned short*)w;
  int* ncodes = (int*)(w + o_count);
  long long* bit_off = (long long*)(w + o_off);
  long long* totals = bit_off + chunks + 1;

  hipLaunchKernelGGL(k_gif_lzw, dim3((unsigned)chunks), dim3(64), 0, c->stream, index, (long long)pixels, codes, ncodes);
  hipLaunchKernelGGL(k_gif_scan, dim3(1), dim3(64), 0, c->stream, (int)chunks, ncodes, bit_off, totals);
  HIPCHK(hipGetLastError());
  long long total = 0;
  int rc = read_back(c, &total, totals, sizeof total);
  if (rc) return rc;
  if ((rc = refuse_room(total, capacity, n_out, "the GIF image data takes %lld bytes, the buffer holds %lld"))) return rc;
  const int64_t words = (total + 3) / 4;
  HIPCHK(c->gif.out.grow(words, c->stream));
  HIPCHK(hipMemsetAsync(c->gif.out, 0, (size_t)words * sizeof(unsigned), c->stream));
  hipLaunchKernelGGL(k_gif_merge, dim3((unsigned)chunks), dim3(64), 0, c->stream, (int)chunks, codes, ncodes, bit_off, totals,
                     c->gif.out);
  HIPCHK(hipGetLastError());
  return read_back(c, out, c->gif.out, (size_t)total);
}

// (*n_out is set whatever follows: 0 until the size is known)
static int gif_check(sc_ctx* c, const uint8_t* out, int64_t capacity, int64_t* n_out) {
  if (n_out) *n_out = 0;
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "encoding happens between ticks");
  if (!n_out || capacity < 0 || (!out && capacity > 0)) return fail(SC_ERR_ARG, "null n_out, or a negative capacity, or a null buffer");
  return SC_OK;
}

int sc_gif_encode_device(sc_ctx* c, const uint8_t* dev_index, int32_t width, int32_t height, uint8_t* out, int64_t capacity,
                         int64_t* n_out) {
  int rc = gif_check(c, out, capacity, n_out);
  if (rc) return rc;
  if (!dev_index) return fail(SC_ERR_ARG, "null frame");
  if ((rc = check_frame(width, height))) return rc;
  HIPCHK(hipSetDevice(c->device));
  return gif_encode(c, dev_index, width, height, out, capacity, n_out);
}

int sc_render_gif(sc_ctx* c, const sc_view* view, const double* segments, int32_t n_segments, uint8_t* out, int64_t capacity,
                  int64_t* n_out) {
  int rc = gif_check(c, out, capacity, n_out);
  if (rc) return rc;
  RenderView v;
  if ((rc = render_prepare(c, view, segments, n_segments, true, v))) return rc;
  HIPCHK(c->gif.index.grow((int64_t)v.width * v.height, c->stream));
  if ((rc = render_launch(c, v, c->gif.index, true))) return rc;
  return gif_encode(c, c->gif.index, v.width, v.height, out, capacity, n_out);
}

}  // extern "C"
