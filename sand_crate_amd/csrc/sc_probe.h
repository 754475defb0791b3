// The probe (sc_probe_now / sc_probe_enable / sc_probe_read): sixteen observables of the stored state and a per-column
// profile of the free surface, reduced on the device in one pass over x, y, vx, vy, P (40 bytes per particle).  The rule
// is specified in NumPy by tests/probe_spec.py.  Included once by sandcrate_hip.hip.  The probe only reads the state: no
// counter of the tick, flag or particle array is written.
//
// The row is a pure function of the stored state: no floating-point atomics anywhere.
//   sums     a thread adds its slots (slot = thread, thread + kProbeThreads, ...), then the wave (an xor butterfly), then
//            the workgroup's waves in order; the workgroup writes one partial record, and the last workgroup to finish (a
//            ticket, as k_halo_unpack takes one, on the probe's own word) adds the partials in index order.  The launch
//            is kProbeBlocks workgroups whatever the particle count; those whose first slot lies beyond the stored count
//            leave at once, so the partition depends on the stored count alone.
//   profile  count and top of a workgroup live in LDS (int and 64-bit words, integer atomics); top is held as an
//            order-preserving 64-bit key of the double under atomicMin, all ones standing for an empty bin.  The
//            workgroup then adds / mins its non-empty bins into the row's arrays in global memory with the same atomics.
// Counts, minima and maxima do not depend on any order; vx vx + vy vy is evaluated without contraction, so max_speed2 and
// the terms of sum_ke are NumPy's bit for bit.  A NaN in a velocity, a pressure or y propagates into the sums, minima
// and maxima it takes part in (NumPy's min / max); a NaN y takes no part in `top`.
#pragma once
#include "sc_device.h"

namespace sc {

constexpr int kProbeBlock = 1024;   // 16 wave64 per workgroup, one workgroup per CU
constexpr int kProbeBlocks = 256;   // the launch: fixed, so that a row never depends on the host's bound of the count
constexpr int kProbeThreads = kProbeBlock * kProbeBlocks;
constexpr int kProbeFields = SC_PROBE_FIELDS;
constexpr int kProbeMaxBins = SC_PROBE_MAX_BINS;
constexpr unsigned long long kProbeEmptyTop = ~0ull;  // (the key of no double that takes part: NaNs do not)

enum ProbeField { PF_TICK = 0, PF_N, PF_SUM_X, PF_SUM_Y, PF_SUM_VX, PF_SUM_VY, PF_SUM_KE, PF_SUM_P, PF_MIN_X, PF_MAX_X,
                  PF_MIN_Y, PF_MAX_Y, PF_MAX_SPEED2, PF_MAX_P, PF_N_PRESSED, PF_N_BINNED };
// the probe's own words, next to its partial records
enum ProbeWord { PW_TICKET = 0, PW_HEAD = 1, PW_DROPPED = 2, PW_COUNT = 4 };

struct ProbeArgs {
  int nbins;             // 0: no profile
  double x0, w;          // bin k holds floor((x - x0) / w) == k; w = (x1 - x0) / nbins, taken once on the host
  double tick;           // ticks finished by the context
  int pressure_valid;    // k_render_splat's rule: P belongs to the slots the last finished tick left live
  int cap;               // capacity of the storage arrays
  long long log_rows;    // the log's capacity in rows; negative: on demand, the row is row 0 of the arrays given
};

// The double as a 64-bit key whose unsigned order is the doubles' order (-inf lowest, -0 below +0, +inf highest).
__device__ __host__ __forceinline__ unsigned long long probe_key(double v) {
  unsigned long long b;
  __builtin_memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// min / max as NumPy's: a NaN on either side is the result
__device__ __forceinline__ double probe_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double probe_max(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double probe_combine(int f, double a, double b) {
  if (f == PF_MIN_X || f == PF_MIN_Y) return probe_min(a, b);
  if (f == PF_MAX_X || f == PF_MAX_Y || f == PF_MAX_SPEED2 || f == PF_MAX_P) return probe_max(a, b);
  return a + b;
}

template <int J>
__device__ __forceinline__ void probe_wave_step(double (&acc)[kProbeFields]) {
#pragma unroll
  for (int f = 1; f < kProbeFields; ++f) acc[f] = probe_combine(f, acc[f], xor_lane<J>(acc[f]));
}

__global__ void __launch_bounds__(kProbeBlock)
    k_probe(ProbeArgs a, const int* __restrict__ counters, const double* __restrict__ x, const double* __restrict__ y,
            const double* __restrict__ vx, const double* __restrict__ vy, const double* __restrict__ P, double* partials,
            int* words, double* rows, int* counts, unsigned long long* tops) {
#pragma clang fp contract(off)
  __shared__ int s_count[kProbeMaxBins];
  __shared__ unsigned long long s_top[kProbeMaxBins];
  __shared__ double s_wave[kProbeBlock / 64][kProbeFields];
  __shared__ double s_part[kProbeBlocks][kProbeFields];
  __shared__ int s_last;
  const int tid = (int)threadIdx.x;
  const int ns = min(counters[C_NS], a.cap);
  const int nb = max(1, min(kProbeBlocks, (int)(((long long)ns + kProbeBlock - 1) / kProbeBlock)));
  if ((int)blockIdx.x >= nb) return;  // no slot of this workgroup is stored
  long long row = 0;
  if (a.log_rows >= 0) {
    if (tick_abandoned(counters)) return;  // the log holds a row per tick that happened: an abandoned one leaves none
    row =__hip_atomic_load(&words[PW_HEAD], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (row >= a.log_rows) {  // the log is full: the tick is not recorded, only counted
      if (blockIdx.x == 0 && tid == 0) words[PW_DROPPED] += 1;
      return;
    }
  }
  for (int k = tid; k < a.nbins; k += kProbeBlock) {
    s_count[k] = 0;
    s_top[k] = kProbeEmptyTop;
  }
  __syncthreads();

  const int np = a.pressure_valid ? pressure_slots(counters, ns) : 0;
  const double inf = __builtin_inf();
  double acc[kProbeFields];
#pragma unroll
  for (int f = 0; f < kProbeFields; ++f) acc[f] = 0.0;
  acc[PF_MIN_X] = acc[PF_MIN_Y] = inf;
  acc[PF_MAX_X] = acc[PF_MAX_Y] = -inf;
  const double nbins_d = (double)a.nbins;
  for (int i = (int)blockIdx.x * kProbeBlock + tid; i < ns; i += kProbeThreads) {
    const double px = x[i];
    if (!(fabs(px) < 1e300)) continue;  // k_owned_count's rule: a dead ghost copy, a particle that is not finite
    const double py = y[i], ux = vx[i], uy = vy[i];
    const double p = i < np ? P[i] : 0.0;
    const double s2 = ux * ux + uy * uy;  // (not contracted: the pragma above, and the library's -ffp-contract=off)
    acc[PF_N] += 1.0;
    acc[PF_SUM_X] += px;
    acc[PF_SUM_Y] += py;
    acc[PF_SUM_VX] += ux;
    acc[PF_SUM_VY] += uy;
    acc[PF_SUM_KE] += 0.5 * s2;
    acc[PF_SUM_P] += p;
    acc[PF_MIN_X] = probe_min(acc[PF_MIN_X], px);
    acc[PF_MAX_X] = probe_max(acc[PF_MAX_X], px);
    acc[PF_MIN_Y] = probe_min(acc[PF_MIN_Y], py);
    acc[PF_MAX_Y] = probe_max(acc[PF_MAX_Y], py);
    acc[PF_MAX_SPEED2] = probe_max(acc[PF_MAX_SPEED2], s2);
    acc[PF_MAX_P] = probe_max(acc[PF_MAX_P], p);
    if (p > 0.0) acc[PF_N_PRESSED] += 1.0;
    if (a.nbins > 0) {
      const double q = floor((px - a.x0) / a.w);
      if (q >= 0.0 && q < nbins_d) {
        const int k = (int)q;
        acc[PF_N_BINNED] += 1.0;
        atomicAdd(&s_count[k], 1);
        if (py == py) {
          const unsigned long long key = probe_key(py);
          // (the word only ever decreases: a key that is not below what it holds now is not below what it ends with)
          if (key < *(volatile unsigned long long*)&s_top[k]) atomicMin(&s_top[k], key);
        }
      }
    }
  }

  // the wave: an xor butterfly, after which every lane holds the wave's record; then the waves in order
  probe_wave_step<1>(acc);
  probe_wave_step<2>(acc);
  probe_wave_step<4>(acc);
  probe_wave_step<8>(acc);
  probe_wave_step<16>(acc);
  probe_wave_step<32>(acc);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int f = 0; f < kProbeFields; ++f) s_wave[tid >> 6][f] = acc[f];
  }
  __syncthreads();
  if (tid < kProbeFields) {
    double v = s_wave[0][tid];
    for (int wv = 1; wv < kProbeBlock / 64; ++wv) v = probe_combine(tid, v, s_wave[wv][tid]);
    // (8-byte agent-scope stores and, in the last workgroup, loads: written through, never served from a stale line)
    __hip_atomic_store((unsigned long long*)&partials[(size_t)blockIdx.x * kProbeFields + tid],
                       (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the workgroup's bins into the row's: integer atomics, exact in any order
  if (a.nbins > 0) {
    int* gc = counts + (size_t)row * a.nbins;
    unsigned long long* gt = tops + (size_t)row * a.nbins;
    for (int k = tid; k < a.nbins; k += kProbeBlock) {
      const int cnt = s_count[k];
      if (cnt > 0) {
        atomicAdd(&gc[k], cnt);
        if (s_top[k] != kProbeEmptyTop) atomicMin(&gt[k], s_top[k]);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // every store and atomic of this workgroup has been issued and has left
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int ticket = __hip_atomic_fetch_add(&words[PW_TICKET], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = ticket == nb - 1;
    if (s_last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!s_last) return;

  // the last workgroup: the partial records in index order
  for (int k = tid; k < nb * kProbeFields; k += kProbeBlock)
    s_part[k / kProbeFields][k % kProbeFields] = __longlong_as_double((long long)__hip_atomic_load(
        (unsigned long long*)&partials[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  __syncthreads();
  if (tid < kProbeFields) {
    double v = s_part[0][tid];
    for (int b = 1; b < nb; ++b) v = probe_combine(tid, v, s_part[b][tid]);
    rows[(size_t)row * kProbeFields + tid] = tid == PF_TICK ? a.tick : v;
  }
  if (tid == 0) {
    __hip_atomic_store(&words[PW_TICKET], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.log_rows >= 0) __hip_atomic_store(&words[PW_HEAD], (int)row + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace sc
