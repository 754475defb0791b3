// Frame rendering (sc_render / sc_render_device): the particles as discs coloured by pressure and the walls on top,
// as Playback.draw_scene draws them (playback.py:75-85, :191-206), into an H x W x 3 uint8 RGB image.  The raster rule
// is specified in NumPy by tests/render_spec.py; these kernels reproduce it bit for bit.  Included once by
// sandcrate_hip.hip.  Rendering only reads the state: no counter, flag or particle array is written.
//
//   splat    per covered pixel, a no-return atomicMax of key = (id + 1) << 8 | c: the largest key is the highest id, so
//            "the particle drawn last wins" (the reference draws in array = id order) holds in any execution order
//   resolve  per pixel: white if a wall covers it, else background (key 0) or (c, c, 255) from the key's low byte;
//            it also clears the key it read, which leaves the W x H 64-bit key buffer zero for the next frame.
//            k_render_resolve_index writes the same pixel as one palette index instead (the GIF path, sc_gif.h)
#pragma once
#include "sc_device.h"

namespace sc {

constexpr int kRenderWaveRadius = 4;  // discs with a larger radius get a whole wave each (k_render_splat<true>)

// One wall segment in screen coordinates (playback.py:208-213, not floored) with what the exact test needs, and a box
// that holds every pixel the test can accept (the segment's hull widened by segment_width + 1: a covered pixel is
// within segment_width / 2 of it).  Filled on the host.
struct RenderSeg {
  double ax, ay, dx, dy, len2;
  double lox, hix, loy, hiy;
};

struct RenderView {
  int width, height;
  double center_x, center_y, zoom;
  double half_w, half_h;  // W / 2, H / 2
  double sx, sy;          // W - 1, H - 1
  long long radius;     // R = floor(trunc(W * particle_radius) * zoom)
  double radius_d;
  double w2;            // segment_width^2
  int nseg;
  RenderSeg seg[kMaxSeg];
};

// The covered pixels of the disc of radius R around (px, py), clipped to the frame, visited from `first` in steps of
// `step` over the clipped bounding box flattened row by row.
__device__ __forceinline__ void splat_disc(unsigned long long* __restrict__ keys, unsigned long long key, long long px,
                                           long long py, long long R, int W, int H, int first, int step) {
  const int x0 = (int)max(px - R, 0LL), x1 = (int)min(px + R, (long long)W - 1);
  const int y0 = (int)max(py - R, 0LL), y1 = (int)min(py + R, (long long)H - 1);
  if (x0 > x1 || y0 > y1) return;
  const unsigned bw = (unsigned)(x1 - x0 + 1), n = bw * (unsigned)(y1 - y0 + 1);  // at most 16384^2
  const long long r2 = R * R;
  for (unsigned k = first; k < n; k += step) {
    const unsigned row = k / bw;
    const int i = x0 + (int)(k - row * bw), j = y0 + (int)row;
    const long long ex = i - px, ey = j - py;
    if (ex * ex + ey * ey <= r2) atomicMax(keys + (size_t)j * W + i, key);
  }
}

// WAVE = false: one thread per stored slot.  WAVE = true: one wave per slot, its lanes share the disc's pixels.
// The live count is read on the device, so nothing waits for the host; launched over the host's bound of it.
template <bool WAVE>
__global__ void __launch_bounds__(kBlock) k_render_splat(RenderView v, const int* __restrict__ counters,
                                                         const double* __restrict__ x, const double* __restrict__ y,
                                                         const int* __restrict__ id, const double* __restrict__ P,
                                                         int pressure_valid, int bound, unsigned long long* __restrict__ keys) {
  const int slot = WAVE ? (int)(blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u) : (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int ns = counters[C_NS];
  if (slot >= bound || slot >= ns) return;
  const double px_w = x[slot], py_w = y[slot];
  if (!isfinite(px_w) || !isfinite(py_w)) return;  // (also the dead ghost copies of slab mode, x = +inf)
  // playback.py:208-213: int(x * (W - 1)), then (. - center) * zoom + W / 2 in float64, then the pixel it falls in
  const double X = floor((trunc(px_w * v.sx) - v.center_x) * v.zoom + v.half_w);
  const double Y = floor((trunc(py_w * v.sy) - v.center_y) * v.zoom + v.half_h);
  const double Rd = v.radius_d;
  if (!(X + Rd >= 0.0 && X - Rd <= v.sx && Y + Rd >= 0.0 && Y - Rd <= v.sy)) return;  // the disc misses the frame
  // sc_download_state's pairing: the pressure of the last finished tick belongs to the slots it left live
  const int np = pressure_valid ? pressure_slots(counters, ns) : 0;
  const double p = slot < np ? P[slot] : 0.0;
  // playback.py:197-200: 255 - int(p * 255), clipped to [0, 255]; NaN and +inf -> 0, -inf -> 255
  const double cc = 255.0 - trunc(p * 255.0);
  const unsigned c = cc >= 255.0 ? 255u : (cc > 0.0 ? (unsigned)cc : 0u);
  const unsigned long long key = ((unsigned long long)(unsigned)(id[slot] + 1) << 8) | c;
  if (WAVE)
    splat_disc(keys, key, (long long)X, (long long)Y, v.radius, v.width, v.height, (int)(threadIdx.x & 63u), 64);
  else
    splat_disc(keys, key, (long long)X, (long long)Y, v.radius, v.width, v.height, 0, 1);
}

// Squared distance test of one pixel against one wall, in render_spec.py's order of operations.
__device__ __forceinline__ bool wall_covers(const RenderSeg& s, double fi, double fj, double w2) {
  if (fi < s.lox || fi > s.hix || fj < s.loy || fj > s.hiy) return false;
  double t = 0.0;
  if (s.len2 != 0.0) {
    t = ((fi - s.ax) * s.dx + (fj - s.ay) * s.dy) / s.len2;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  }
  const double qx = s.ax + t * s.dx, qy = s.ay + t * s.dy;
  const double e = (fi - qx) * (fi - qx) + (fj - qy) * (fj - qy);
  return 4.0 * e <= w2;
}

// What resolve knows of a thread's four pixels p0 .. p0 + 3 (the first m of them inside the frame): the key of each,
// cleared once read -- the buffer is all zero between frames (zeroed once when allocated), so no separate clear has
// to run before the next splat -- and whether a wall covers it.
struct ResolvedQuad {
  unsigned long long key[4];
  bool wall[4];
};

__device__ __forceinline__ ResolvedQuad resolve_quad(const RenderView& v, unsigned long long* __restrict__ keys,
                                                     unsigned p0, int m) {
  ResolvedQuad r = {{0ull, 0ull, 0ull, 0ull}, {false, false, false, false}};
  double fi[4], fj[4];
  int i = (int)(p0 % (unsigned)v.width), j = (int)(p0 / (unsigned)v.width);
  for (int q = 0; q < 4; ++q) {
    if (q < m) {
      r.key[q] = keys[p0 + q];
      keys[p0 + q] = 0ull;
    }
    fi[q] = (double)i;
    fj[q] = (double)j;
    if (++i == v.width) {
      i = 0;
      ++j;
    }
  }
  for (int s = 0; s < v.nseg; ++s) {
    const RenderSeg g = v.seg[s];
    for (int q = 0; q < 4; ++q) r.wall[q] = r.wall[q] || wall_covers(g, fi[q], fj[q], v.w2);
  }
  return r;
}

// Four pixels per thread, written as three dwords (or byte by byte when `rgb` is not 4-byte aligned, and for the
// last pixels of a frame whose size is not a multiple of four).
__global__ void __launch_bounds__(kBlock) k_render_resolve(RenderView v, unsigned long long* __restrict__ keys,
                                                           unsigned char* __restrict__ rgb, int aligned) {
  const unsigned total = (unsigned)v.width * (unsigned)v.height;  // at most 16384^2
  const unsigned p0 = 4u * (blockIdx.x * blockDim.x + threadIdx.x);
  if (p0 >= total) return;
  const int m = (int)min(4u, total - p0);
  const ResolvedQuad r = resolve_quad(v, keys, p0, m);
  unsigned c[4];
  for (int q = 0; q < 4; ++q) {
    const unsigned k = (unsigned)(r.key[q] & 0xFF);
    c[q] = r.wall[q] ? 0xFFFFFFu : (r.key[q] == 0 ? 0u : (k | (k << 8) | (255u << 16)));  // bytes r, g, b
  }
  unsigned char* out = rgb + 3 * (size_t)p0;
  if (m == 4 && aligned) {
    unsigned* o = (unsigned*)out;
    o[0] = c[0] | (c[1] << 24);
    o[1] = (c[1] >> 8) | (c[2] << 16);
    o[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
    for (int q = 0; q < m; ++q) {
      out[3 * q] = (unsigned char)c[q];
      out[3 * q + 1] = (unsigned char)(c[q] >> 8);
      out[3 * q + 2] = (unsigned char)(c[q] >> 16);
    }
  }
}

// The same frame as one palette index per pixel (sc_gif.h; tests/gif_spec.py: indices): 0 for the background, 255 for
// a wall, max(c, lowest) for a disc of colour byte c -- lowest = 1, or 2 when entry 1 belongs to the arrows
// (sc_arrows.h).  `index` is 4-byte aligned: four pixels are one dword.
__global__ void __launch_bounds__(kBlock) k_render_resolve_index(RenderView v, unsigned long long* __restrict__ keys,
                                                                 unsigned char* __restrict__ index, unsigned lowest) {
  const unsigned total = (unsigned)v.width * (unsigned)v.height;
  const unsigned p0 = 4u * (blockIdx.x * blockDim.x + threadIdx.x);
  if (p0 >= total) return;
  const int m = (int)min(4u, total - p0);
  const ResolvedQuad r = resolve_quad(v, keys, p0, m);
  unsigned c[4];
  for (int q = 0; q < 4; ++q) c[q] = r.wall[q] ? 255u : (r.key[q] == 0 ? 0u : max((unsigned)(r.key[q] & 0xFF), lowest));
  if (m == 4) {
    *(unsigned*)(index + p0) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
  } else {
    for (int q = 0; q < m; ++q) index[p0 + q] = (unsigned char)c[q];
  }
}

}  // namespace sc
