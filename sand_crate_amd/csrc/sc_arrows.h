// The debug arrows (sc_set_arrows): the layer Playback.draw_debug_arrows puts between the walls and the HUD text
// (playback.py:95-107), written in green over a frame that resolve has finished -- H x W x 3 RGB (k_render_resolve) or
// H x W palette indices (k_render_resolve_index, where an arrow is index 1) -- before the HUD overlay and the encoders.
// The pixel rule is specified in NumPy by tests/arrow_spec.py; this kernel reproduces it bit for bit (the file is
// compiled with -ffp-contract=off: every product and sum below is rounded on its own, in the spec's order).
// Included once by sandcrate_hip.hip.
//
// One thread per arrow, the rest of its wave at hand.  The arrows come from a list of (start, end) in world units, or from the particles: one arrow
// per stored live particle whose id is a multiple of `every`, from its position along velocity * scale compressed as
// playback.py:99 compresses a direction; the live count is read on the device.  A thread maps its arrow to the screen
// and clips the hull of its two ends, widened by kArrowMargin pixels, to the frame -- in float64, before anything
// becomes an integer, so that coordinates of 1e300 neither overflow nor loop.  A box of at most kArrowWaveBox pixels
// the thread walks alone; the larger ones the wave then takes one after the other, the arrow handed from its lane to
// all 64, which stride the box.  A list's arrows sit kArrowListPerWave to a wave, the other lanes only helping: a wave
// full of large boxes would walk 64 of them in turn while most of the GPU idles (a list is at most 2^20 arrows, so the
// wider grid stays small; the particles' arrows are thinned by `every` and mostly short).  Stores only: bytes into
// covered pixels, nothing read from the frame, so the frame may start at any address; all arrows have one colour, so
// arrows that overlap race harmlessly.
#pragma once
#include "sandcrate_hip.h"
#include "sc_device.h"

namespace sc {

constexpr int kArrowMargin = 3;      // pixels around the hull of S and E: the head reaches 2 from the axis
constexpr unsigned kArrowWaveBox = 256;  // a clipped box of more pixels than this gets the whole wave
constexpr long long kArrowMaxList = 1 << 20;
constexpr int kArrowListPerWave = 4;  // arrows of a list held by one wave, in its first lanes

struct ArrowView {
  int width, height;
  double center_x, center_y, zoom;
  double half_w, half_h;  // W / 2, H / 2
  double sx, sy;          // W - 1, H - 1
};

// An arrow on the screen, and its clipped box flattened row by row: n pixels, bw of them in a row, from (x0, y0).
struct ArrowJob {
  double Sx, Sy, ax, ay, L2, L;
  int x0, y0;
  unsigned bw, n;  // n == 0: nothing to draw
};

// playback.py:99: d / (|d| + 0.001) ^ 0.3
__device__ __forceinline__ void arrow_compress(double& dx, double& dy) {
  const double f = pow(sqrt(dx * dx + dy * dy) + 0.001, 0.3);
  dx = dx / f;
  dy = dy / f;
}

__device__ __forceinline__ ArrowJob arrow_job(const ArrowView& v, double s_x, double s_y, double e_x, double e_y) {
  ArrowJob j = {};
  if (!isfinite(s_x) || !isfinite(s_y) || !isfinite(e_x) || !isfinite(e_y)) return j;
  // crate_to_screen_coord (playback.py:208-213), not floored: tests/render_spec.py, screen
  const double Sx = (trunc(s_x * v.sx) - v.center_x) * v.zoom + v.half_w;
  const double Sy = (trunc(s_y * v.sy) - v.center_y) * v.zoom + v.half_h;
  const double Ex = (trunc(e_x * v.sx) - v.center_x) * v.zoom + v.half_w;
  const double Ey = (trunc(e_y * v.sy) - v.center_y) * v.zoom + v.half_h;
  if (!isfinite(Sx) || !isfinite(Sy) || !isfinite(Ex) || !isfinite(Ey)) return j;
  const double ax = Ex - Sx, ay = Ey - Sy;
  const double L2 = ax * ax + ay * ay;
  if (L2 == 0.0) return j;
  // the box, clipped while still float64: each bound ends inside [0, side - 1] or the box is empty
  const double lox = fmax(ceil(fmin(Sx, Ex) - kArrowMargin), 0.0), hix = fmin(floor(fmax(Sx, Ex) + kArrowMargin), v.sx);
  const double loy = fmax(ceil(fmin(Sy, Ey) - kArrowMargin), 0.0), hiy = fmin(floor(fmax(Sy, Ey) + kArrowMargin), v.sy);
  if (!(lox <= hix && loy <= hiy)) return j;
  j.Sx = Sx;
  j.Sy = Sy;
  j.ax = ax;
  j.ay = ay;
  j.L2 = L2;
  j.L = sqrt(L2);
  j.x0 = (int)lox;
  j.y0 = (int)loy;
  j.bw = (unsigned)((int)hix - j.x0 + 1);
  j.n = j.bw * (unsigned)((int)hiy - j.y0 + 1);  // at most 16384^2
  return j;
}

// tests/arrow_spec.py, covered: the body, a rectangle of half-width 1 from S to 2 pixels before E (only when the arrow
// is at least as long as the head), and the head, a triangle of half-width 2 there with its tip on E; closed
// point-in-shape tests multiplied through by L.
__device__ __forceinline__ bool arrow_covers(const ArrowJob& j, int i, int jj) {
  const double px = (double)i - j.Sx, py = (double)jj - j.Sy;
  const double nx = -j.ay, ny = j.ax;
  const double t = px * j.ax + py * j.ay;
  const double w = px * nx + py * ny;
  const double neck = j.L2 - 2.0 * j.L;
  const bool body = j.L2 >= 4.0 && 0.0 <= t && t <= neck && w * w <= j.L2;
  const bool head = neck <= t && t <= j.L2 && fabs(w) <= j.L2 - t;
  return body || head;
}

// The box's pixels from `first` in steps of `step`.
template <bool INDEX>
__device__ __forceinline__ void arrow_draw(const ArrowJob& j, int W, unsigned char* __restrict__ frame, unsigned first,
                                           unsigned step) {
  for (unsigned k = first; k < j.n; k += step) {
    const unsigned row = k / j.bw;
    const int x = j.x0 + (int)(k - row * j.bw), y = j.y0 + (int)row;
    if (!arrow_covers(j, x, y)) continue;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    if (INDEX) {
      frame[p] = 1;
    } else {
      frame[3 * p] = 0;
      frame[3 * p + 1] = 255;
      frame[3 * p + 2] = 0;
    }
  }
}

// INDEX: the frame is one palette index per pixel, else three bytes r, g, b.  `list` != null: arrow k of `count` is
// list[k], kArrowListPerWave of them to a wave.  `list` == null: slot k of the particle arrays, the first
// min(count, counters[C_NS]) of them, `count` being the host's bound of the live count.
template <bool INDEX>
__global__ void __launch_bounds__(kBlock) k_arrows(ArrowView v, const sc_arrow* __restrict__ list, int count,
                                                   const int* __restrict__ counters, const double* __restrict__ x,
                                                   const double* __restrict__ y, const double* __restrict__ vx,
                                                   const double* __restrict__ vy, const int* __restrict__ id,
                                                   double scale, long long every, unsigned char* __restrict__ frame) {
  const unsigned lane = threadIdx.x & 63u;
  const long long thread = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long k = !list ? thread : (lane < (unsigned)kArrowListPerWave ? (thread >> 6) * kArrowListPerWave + lane : count);
  ArrowJob j = {};
  if (list) {
    if (k < count) {
      const sc_arrow a = list[k];
      j = arrow_job(v, a.start_x, a.start_y, a.end_x, a.end_y);
    }
  } else if (k < count && k < counters[C_NS] && (long long)id[k] % every == 0) {
    const double s_x = x[k], s_y = y[k];  // (not finite: also the dead ghost copies of slab mode, x = +inf)
    double dx = vx[k] * scale, dy = vy[k] * scale;
    arrow_compress(dx, dy);
    j = arrow_job(v, s_x, s_y, s_x + dx, s_y + dy);
  }
  const bool big = j.n > kArrowWaveBox;
  if (!big) arrow_draw<INDEX>(j, v.width, frame, 0u, 1u);
  // the wave's large boxes, one after the other (every lane of the wave gets here)
  for (unsigned long long todo = __ballot(big); todo; todo &= todo - 1) {
    const int src = __ffsll((long long)todo) - 1;
    ArrowJob b;
    b.Sx = __shfl(j.Sx, src);
    b.Sy = __shfl(j.Sy, src);
    b.ax = __shfl(j.ax, src);
    b.ay = __shfl(j.ay, src);
    b.L2 = __shfl(j.L2, src);
    b.L = __shfl(j.L, src);
    b.x0 = __shfl(j.x0, src);
    b.y0 = __shfl(j.y0, src);
    b.bw = __shfl(j.bw, src);
    b.n = __shfl(j.n, src);
    arrow_draw<INDEX>(b, v.width, frame, lane, 64u);
  }
}

}  // namespace sc
