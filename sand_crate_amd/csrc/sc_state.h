// The state to and from the caller's DEVICE memory in particle-index order (sc_export_state_device /
// sc_import_state_device).  The rule of the export is specified in NumPy by tests/state_spec.py: exactly what
// sc_download_state delivers to the host.  Included once by sandcrate_hip.hip.  The export only reads the state: no
// counter of the tick, flag or particle array is written.
//
// The storage arrays are in cell-sorted order; the caller's order is ascending id.  The ranking is an LSD radix sort of
// (id, slot) pairs, hand-written: kStatePasses passes over kStateDigitBits bits each, and per pass
//   k_state_hist     a workgroup counts the digits of its kStateTile keys in LDS (integer atomics) and writes its 256
//                    counts digit-major: hist[digit * tiles + tile].  The first pass also MAKES the pairs: the key of a
//                    stored slot whose x is finite is its id, every other slot of the launch gets kStateDead, which is
//                    above every id (ids stay below 2^31 - 1) and so sorts behind all of them;
//   k_scan_local / k_scan_fix (sc_kernels.h)  the exclusive scan of those counts: in digit-major order it is, for every
//                    (digit, tile), the place of the tile's first key with that digit;
//   k_state_scatter  a key goes to that place plus its rank among the tile's keys of the same digit: the lanes of a wave
//                    that hold the same digit find each other with eight ballots, the waves' counts meet in LDS.  Keys of
//                    equal digit keep their order (the sort is stable), so four passes order by the whole key.
// No workgroup waits for another, no floating-point or order-dependent atomics: the result is a pure function of the
// stored state.  k_state_gather then moves slot slots[k] to row k: (x, y) and (vx, vy) as 16-byte records, the pressure,
// the id, and -- the one thread that sits on the border between ids and kStateDead -- the count.
// Cost: linear in the launch bound (the stored count; in slab mode the capacity), whatever the ids are.
#pragma once
#include "sc_device.h"

namespace sc {

constexpr int kStateTile = 256;       // keys (= threads) per workgroup of a sorting pass
constexpr int kStateDigitBits = 8;
constexpr int kStateBins = 1 << kStateDigitBits;
constexpr int kStatePasses = 4;       // 32 bits: ids below 2^31 - 1 and kStateDead above them (an even number: the
                                      // pairs end in the set they started in)
constexpr unsigned kStateDead = 0xFFFFFFFFu;
static_assert(kStateBins == kStateTile, "thread t writes the tile's count of digit t");
static_assert(kStatePasses * kStateDigitBits == 32 && kStatePasses % 2 == 0, "the passes cover the key");

// what the export writes; any of the four arrays may be null
struct StateOut {
  double* xy;
  double* vxy;
  double* pressure;
  long long* ids;
  long long* n;
};

// `x` given: the first pass, which makes the pairs of the m slots of the launch from the stored state.
__global__ void __launch_bounds__(kStateTile)
    k_state_hist(const int* __restrict__ counters, const double* __restrict__ x, const int* __restrict__ id, int cap,
                 unsigned* __restrict__ keys, int* __restrict__ slots, int m, int shift, int tiles, int* __restrict__ hist) {
  __shared__ int s_h[kStateBins];
  const int tid = (int)threadIdx.x;
  s_h[tid] = 0;
  __syncthreads();
  const int i = (int)blockIdx.x * kStateTile + tid;
  if (i < m) {
    unsigned key;
    if (x) {
      const int ns = min(counters[C_NS], cap);
      key = (i < ns && fabs(x[i]) < __builtin_inf()) ? (unsigned)id[i] : kStateDead;  // (NaN compares false: dead)
      keys[i] = key;
      slots[i] = i;
    } else {
      key = keys[i];
    }
    atomicAdd(&s_h[(key >> shift) & (kStateBins - 1)], 1);
  }
  __syncthreads();
  hist[(size_t)tid * tiles + blockIdx.x] = s_h[tid];
}

__global__ void __launch_bounds__(kStateTile)
    k_state_scatter(const unsigned* __restrict__ keys_in, const int* __restrict__ slots_in, unsigned* __restrict__ keys_out,
                    int* __restrict__ slots_out, int m, int shift, int tiles, const int* __restrict__ offs) {
  __shared__ int s_cnt[kStateTile / 64][kStateBins];
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int w = 0; w < kStateTile / 64; ++w) s_cnt[w][tid] = 0;
  __syncthreads();
  const int i = (int)blockIdx.x * kStateTile + tid;
  const bool on = i < m;
  const unsigned key = on ? keys_in[i] : 0u;
  const int slot = on ? slots_in[i] : 0;
  const int digit = (int)((key >> shift) & (kStateBins - 1));
  // the lanes of this wave that hold a key with the same digit (every lane of the wave takes part in the ballots)
  unsigned long long peers = __ballot(on);
#pragma unroll
  for (int b = 0; b < kStateDigitBits; ++b) {
    const bool bit = (digit >> b) & 1;
    const unsigned long long set = __ballot(on && bit);
    peers &= bit ? set : ~set;
  }
  const int rank = __popcll(peers & ((1ull << lane) - 1ull));
  if (on && rank == 0) s_cnt[wv][digit] = __popcll(peers);
  __syncthreads();
  if (on) {
    int before = 0;
    for (int w = 0; w < wv; ++w) before += s_cnt[w][digit];
    const int dest = offs[(size_t)digit * tiles + blockIdx.x] + before + rank;
    if ((unsigned)dest < (unsigned)m) {  // (always, when the counts are this launch's)
      keys_out[dest] = key;
      slots_out[dest] = slot;
    }
  }
}

// Row k of the caller's arrays is the slot with the k-th smallest id.  The pressure follows sc_download_state's rule:
// P belongs to the slots the last finished tick left live.
__global__ void __launch_bounds__(kBlock)
    k_state_gather(const int* __restrict__ counters, StateOut o, const unsigned* __restrict__ keys,
                   const int* __restrict__ slots, int m, int cap, int pressure_valid, const double* __restrict__ x,
                   const double* __restrict__ y, const double* __restrict__ vx, const double* __restrict__ vy,
                   const double* __restrict__ P) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k == 0 && (m == 0 || keys[0] == kStateDead)) *o.n = 0;
  if (k >= m) return;
  const unsigned key = keys[k];
  if (key == kStateDead) return;
  if (k == m - 1 || keys[k + 1] == kStateDead) *o.n = (long long)k + 1;
  const int s = slots[k];
  if (o.xy) ((XY*)o.xy)[k] = XY{x[s], y[s]};
  if (o.vxy) ((XY*)o.vxy)[k] = XY{vx[s], vy[s]};
  if (o.pressure) {
    const int ns = min(counters[C_NS], cap);
    const int np = pressure_valid ? pressure_slots(counters, ns) : 0;
    o.pressure[k] = s < np ? P[s] : 0.0;
  }
  if (o.ids) o.ids[k] = (long long)key;
}

// The import's ids: 64-bit in the caller's memory, 32-bit in the library's.  words[0] becomes the largest id plus one
// (0: none), words[1] nonzero when an id lies outside 0..2^31 - 2; both are cleared before the launch.  One atomic of
// each kind per wave.
__global__ void __launch_bounds__(kBlock)
    k_state_check_ids(const long long* __restrict__ ids, int n, int* __restrict__ ids32, int* __restrict__ words) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const long long v = k < n ? ids[k] : 0;
  const bool bad = v < 0 || v > (long long)INT_MAX - 1;
  if (k < n) ids32[k] = (int)v;
  const int top = wave_max_all((k < n && !bad) ? (int)v + 1 : 0);
  const bool any_bad = __ballot(bad) != 0ull;
  if ((threadIdx.x & 63) == 0) {
    if (top > 0) atomicMax(&words[0], top);
    if (any_bad) atomicOr(&words[1], 1);
  }
}

}  // namespace sc
