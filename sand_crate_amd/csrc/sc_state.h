// The state to and from the caller's DEVICE memory in particle-index order (sc_export_state_device /
// sc_import_state_device).  The rule of the export is specified in NumPy by tests/state_spec.py: exactly what
// sc_download_state delivers to the host.  Included once by sandcrate_hip.hip.  The export only reads the state: no
// counter of the tick, flag or particle array is written.
//
// The storage arrays are in cell-sorted order; the caller's order is ascending id.  The ranking is the radix sort of
// sc_radix.h over (id, slot) pairs, kStatePasses passes.  Its first pass makes the pairs from the stored state (StateKey):
// the key of a stored slot whose x is finite is its id, every other slot of the launch gets kStateDead, which is above
// every id (ids stay below 2^31 - 1) and so sorts behind all of them.  The index-order rule on the device is then
// state_row_live: row k is live while its key is an id, and n is where the ids end.  k_state_gather moves slot slots[k]
// to row k: (x, y) and (vx, vy) as 16-byte records, the pressure and the id.
// Cost: linear in the launch bound (the stored count; in slab mode the capacity), whatever the ids are.
#pragma once
#include "sc_device.h"
#include "sc_radix.h"

namespace sc {

constexpr int kStatePasses = 4;  // 32 bits: ids below 2^31 - 1 and kStateDead above them
constexpr unsigned kStateDead = 0xFFFFFFFFu;
static_assert(kStatePasses * kRadixDigitBits == 32, "the passes cover the key");

// what the export writes; any of the four arrays may be null
struct StateOut {
  double* xy;
  double* vxy;
  double* pressure;
  long long* ids;
  long long* n;
};

// The key of slot i, for the first pass of the ranking (k_radix_hist).
struct StateKey {
  const int* counters;
  const double* x;
  const int* id;
  int cap;
  __device__ unsigned operator()(int i) const {
    const int ns = min(counters[C_NS], cap);
    return (i < ns && fabs(x[i]) < __builtin_inf()) ? (unsigned)id[i] : kStateDead;  // (NaN compares false: dead)
  }
};

// Is k a live row of the m ranked keys?  The one thread that sits on the border between ids and kStateDead writes the
// count to *n.  Every thread of a launch over at least max(m, 1) rows calls this.
__device__ __forceinline__ bool state_row_live(const unsigned* __restrict__ keys, int k, int m, long long* __restrict__ n) {
  if (k == 0 && (m == 0 || keys[0] == kStateDead)) *n = 0;
  if (k >= m || keys[k] == kStateDead) return false;
  if (k == m - 1 || keys[k + 1] == kStateDead) *n = (long long)k + 1;
  return true;
}

// Row k of the caller's arrays is the slot with the k-th smallest id.  The pressure follows sc_download_state's rule:
// P belongs to the slots the last finished tick left live.
__global__ void __launch_bounds__(kBlock)
    k_state_gather(const int* __restrict__ counters, StateOut o, const unsigned* __restrict__ keys,
                   const int* __restrict__ slots, int m, int cap, int pressure_valid, const double* __restrict__ x,
                   const double* __restrict__ y, const double* __restrict__ vx, const double* __restrict__ vy,
                   const double* __restrict__ P) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (!state_row_live(keys, k, m, o.n)) return;
  const int s = slots[k];
  if (o.xy) ((XY*)o.xy)[k] = XY{x[s], y[s]};
  if (o.vxy) ((XY*)o.vxy)[k] = XY{vx[s], vy[s]};
  if (o.pressure) {
    const int ns = min(counters[C_NS], cap);
    const int np = pressure_valid ? pressure_slots(counters, ns) : 0;
    o.pressure[k] = s < np ? P[s] : 0.0;
  }
  if (o.ids) o.ids[k] = (long long)keys[k];
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
