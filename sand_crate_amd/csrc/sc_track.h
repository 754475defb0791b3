// Tracking (sc_track_capture / sc_track_enable / sc_track_read / sc_track_load): the stored state as a packed frame of
// 9 bytes per particle -- id, two 16-bit coordinates, the colour byte the renderer would give it -- behind a 64-byte header
// and the tick's walls, and such a frame back into the state arrays.  The format is specified in NumPy by
// tests/track_spec.py; these kernels reproduce it byte for byte.  Included once by sandcrate_hip.hip.  Packing only reads
// the state: no counter of the tick, flag or particle array is written.
//
//   reserve  one workgroup of one wave: reads the stored count on the device, sizes the frame, and takes its place --
//            one atomic add on the log's byte cursor if the frame fits, else the counter of dropped frames goes up and
//            nothing of the frame is written -- then writes the header and the walls.  Where the frame starts (or that
//            there is none) and its particle count are left in the track words for the pack that follows on the stream.
//   pack     four particles per thread: their ids leave as two 8-byte stores, each coordinate plane as one, the
//            colours as one dword, so a wave writes 1024 / 512 / 512 / 256 contiguous bytes per plane.  Every plane
//            starts on a multiple of 8 bytes of a frame that starts on one; the groups that hold the end of a plane
//            write element by element, and the zero padding with it.
//   unpack   one thread per particle of a frame already in device memory; sets the counters so that all of them are live
//            with a valid pressure.
#pragma once
#include "sc_device.h"

namespace sc {

constexpr unsigned kTrackMagic = 0x4B544353u;  // "SCTK", little-endian
constexpr unsigned kTrackVersion = 1u;
constexpr int kTrackHeaderBytes = 64;
constexpr double kTrackLo = -0.25, kTrackSpan = 1.5;
constexpr double kTrackCodes = 65534.0;  // codes 0..65534 span [lo, lo + span]; 65535: not finite
constexpr int kTrackPerThread = 4;

// the track words: 64 bit each
enum TrackWord { TW_CURSOR = 0, TW_FRAMES = 1, TW_DROPPED = 2, TW_AT = 3, TW_N = 4, TW_COUNT = 8 };

__host__ __device__ __forceinline__ long long track_pad8(long long b) { return (b + 7) & ~7LL; }

struct TrackPlanes {
  long long id, qx, qy, c, end;  // byte offsets into the frame
};

__host__ __device__ __forceinline__ TrackPlanes track_planes(long long n, int nseg) {
  TrackPlanes p;
  p.id = kTrackHeaderBytes + 32LL * nseg;
  p.qx = p.id + track_pad8(4 * n);
  p.qy = p.qx + track_pad8(2 * n);
  p.c = p.qy + track_pad8(2 * n);
  p.end = p.c + track_pad8(n);
  return p;
}

struct TrackArgs {
  long long tick;        // ticks finished by the context
  long long log_bytes;   // the log's capacity; negative: on demand, the frame goes to the start of the buffer given
  long long room;        // on demand: the bytes of that buffer
  double scale;          // 65534 / span, taken once on the host
  int pressure_valid;    // k_render_splat's rule: P belongs to the slots the last finished tick left live
  int cap;               // capacity of the storage arrays
  int nseg;
  Seg seg[kMaxSeg];      // the walls the tick ran with
};

// q = floor((v - lo) * (65534 / span) + 0.5) clamped to 0..65534, each operation rounded on its own; 65535 for a
// coordinate that is not finite
__device__ __forceinline__ unsigned track_quantise(double v, double scale) {
#pragma clang fp contract(off)
  if (!isfinite(v)) return 65535u;
  const double t = (v - kTrackLo) * scale;
  const double q = floor(t + 0.5);
  return q >= kTrackCodes ? 65534u : (q > 0.0 ? (unsigned)q : 0u);
}

// k_render_splat's colour byte: 255 - trunc(p * 255), clipped; NaN and +inf -> 0, -inf -> 255
__device__ __forceinline__ unsigned track_colour(double p) {
#pragma clang fp contract(off)
  const double cc = 255.0 - trunc(p * 255.0);
  return cc >= 255.0 ? 255u : (cc > 0.0 ? (unsigned)cc : 0u);
}

__global__ void __launch_bounds__(64) k_track_reserve(TrackArgs a, const int* __restrict__ counters,
                                                      unsigned long long* words, unsigned char* base) {
  __shared__ long long s_at, s_n;
  const int tid = (int)threadIdx.x;
  if (tid == 0) {
    const long long n = max(0, min(counters[C_NS], a.cap));
    const long long bytes = track_planes(n, a.nseg).end;
    long long at = -1;
    if (a.log_bytes < 0) {
      if (bytes <= a.room) at = 0;
    } else if (tick_abandoned(counters)) {
      // the log holds a frame per tick that happened: an abandoned one leaves none, and none is counted as dropped
    } else if ((long long)words[TW_CURSOR] + bytes <= a.log_bytes) {
      at = (long long)atomicAdd(&words[TW_CURSOR], (unsigned long long)bytes);
      words[TW_FRAMES] += 1;
    } else {  // the frame does not fit: it is absent, and counted
      words[TW_DROPPED] += 1;
    }
    words[TW_AT] = (unsigned long long)at;
    words[TW_N] = (unsigned long long)n;
    s_at = at;
    s_n = n;
  }
  __syncthreads();
  if (s_at < 0) return;
  unsigned long long* out = (unsigned long long*)(base + s_at);  // (frames start on multiples of 8 bytes)
  const int qwords = kTrackHeaderBytes / 8 + 4 * a.nseg;
  for (int k = tid; k < qwords; k += 64) {
    unsigned long long v = 0ull;
    if (k == 0) v = (unsigned long long)kTrackMagic | ((unsigned long long)kTrackVersion << 32);
    else if (k == 1) v = (unsigned long long)a.tick;
    else if (k == 2) v = (unsigned long long)s_n;
    else if (k == 3) v = (unsigned long long)(unsigned)a.nseg | ((unsigned long long)(a.pressure_valid ? 1u : 0u) << 32);
    else if (k == 4) v = (unsigned long long)__double_as_longlong(kTrackLo);
    else if (k == 5) v = (unsigned long long)__double_as_longlong(kTrackSpan);
    else if (k >= 8) {
      const Seg s = a.seg[(k - 8) >> 2];
      const int f = (k - 8) & 3;
      v = (unsigned long long)__double_as_longlong(f == 0 ? s.ax : f == 1 ? s.ay : f == 2 ? s.bx : s.by);
    }
    out[k] = v;
  }
}

__global__ void __launch_bounds__(kBlock) k_track_pack(TrackArgs a, const int* __restrict__ counters,
                                                       const unsigned long long* __restrict__ words,
                                                       const double* __restrict__ x, const double* __restrict__ y,
                                                       const int* __restrict__ id, const double* __restrict__ P,
                                                       unsigned char* base) {
  const long long at = (long long)words[TW_AT];
  if (at < 0) return;  // dropped
  const int n = (int)words[TW_N];
  const int np = a.pressure_valid ? pressure_slots(counters, n) : 0;
  const TrackPlanes pl = track_planes(n, a.nseg);
  unsigned char* frame = base + at;
  unsigned* pid = (unsigned*)(frame + pl.id);
  unsigned short* pqx = (unsigned short*)(frame + pl.qx);
  unsigned short* pqy = (unsigned short*)(frame + pl.qy);
  unsigned char* pc = frame + pl.c;
  const int n_id = (int)(track_pad8(4LL * n) / 4), n_q = (int)(track_pad8(2LL * n) / 2), n_c = (int)track_pad8(n);
  const int groups = n_c / kTrackPerThread;
  for (int g = (int)(blockIdx.x * blockDim.x + threadIdx.x); g < groups; g += (int)(gridDim.x * blockDim.x)) {
    const int s0 = g * kTrackPerThread;
    if (s0 + kTrackPerThread <= n) {
      const double2 xa = *(const double2*)(x + s0), xb = *(const double2*)(x + s0 + 2);
      const double2 ya = *(const double2*)(y + s0), yb = *(const double2*)(y + s0 + 2);
      const int4 ids = *(const int4*)(id + s0);
      double p[4];
      for (int j = 0; j < 4; ++j) p[j] = s0 + j < np ? P[s0 + j] : 0.0;
      const unsigned qx0 = track_quantise(xa.x, a.scale), qx1 = track_quantise(xa.y, a.scale);
      const unsigned qx2 = track_quantise(xb.x, a.scale), qx3 = track_quantise(xb.y, a.scale);
      const unsigned qy0 = track_quantise(ya.x, a.scale), qy1 = track_quantise(ya.y, a.scale);
      const unsigned qy2 = track_quantise(yb.x, a.scale), qy3 = track_quantise(yb.y, a.scale);
      *(uint2*)(pid + s0) = make_uint2((unsigned)ids.x, (unsigned)ids.y);
      *(uint2*)(pid + s0 + 2) = make_uint2((unsigned)ids.z, (unsigned)ids.w);
      *(uint2*)(pqx + s0) = make_uint2(qx0 | (qx1 << 16), qx2 | (qx3 << 16));
      *(uint2*)(pqy + s0) = make_uint2(qy0 | (qy1 << 16), qy2 | (qy3 << 16));
      *(unsigned*)(pc + s0) =
          track_colour(p[0]) | (track_colour(p[1]) << 8) | (track_colour(p[2]) << 16) | (track_colour(p[3]) << 24);
    } else {  // the end of the planes: element by element, and the zero padding
      for (int j = 0; j < kTrackPerThread; ++j) {
        const int s = s0 + j;
        if (s < n) {
          pid[s] = (unsigned)id[s];
          pqx[s] = (unsigned short)track_quantise(x[s], a.scale);
          pqy[s] = (unsigned short)track_quantise(y[s], a.scale);
          pc[s] = (unsigned char)track_colour(s < np ? P[s] : 0.0);
        } else {
          if (s < n_id) pid[s] = 0u;
          if (s < n_q) {
            pqx[s] = 0;
            pqy[s] = 0;
          }
          if (s < n_c) pc[s] = 0;
        }
      }
    }
  }
}

struct TrackLoad {
  int n, nseg;
  int plain;        // every particle gets the reference's playback colour, byte 100
  int next_id;      // the largest id of the frame plus one
  double lo, step;  // x = lo + q * step, step = span / 65534 taken once on the host
};

__global__ void __launch_bounds__(kBlock) k_track_unpack(TrackLoad a, const unsigned char* __restrict__ frame, int* counters,
                                                         double* __restrict__ x, double* __restrict__ y,
                                                         double* __restrict__ vx, double* __restrict__ vy,
                                                         int* __restrict__ id, double* __restrict__ P) {
#pragma clang fp contract(off)
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i == 0) {
    counters[C_NS] = a.n;
    counters[C_NT] = a.n;
    counters[C_NT_DONE] = a.n;
    counters[C_NEXT_ID] = a.next_id;
  }
  if (i >= a.n) return;
  const TrackPlanes pl = track_planes(a.n, a.nseg);
  const unsigned qx = ((const unsigned short*)(frame + pl.qx))[i], qy = ((const unsigned short*)(frame + pl.qy))[i];
  const unsigned c = a.plain ? 100u : (unsigned)frame[pl.c + i];
  const double inf = __builtin_inf();
  x[i] = qx == 65535u ? inf : a.lo + (double)qx * a.step;
  y[i] = qy == 65535u ? inf : a.lo + (double)qy * a.step;
  vx[i] = 0.0;
  vy[i] = 0.0;
  id[i] = (int)((const unsigned*)(frame + pl.id))[i];
  P[i] = (255.0 - (double)c + 0.5) / 255.0;
}

}  // namespace sc
