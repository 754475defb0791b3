// The clusters of the fixed-radius graph on the device (sc_pairs_label_device): the connected components of the graph
// that sc_pairs_count_device defines, over the points whose coordinates are all finite -- labels (the cluster of every
// point, -1 for a point in none), and per cluster its size and its root, the smallest member index; clusters are numbered
// 0 .. C-1 ascending in their roots.  The rule is specified in NumPy by tests/cluster_spec.py; the result is a pure function
// of the points.  Included once by sandcrate_hip.hip, after sc_pairs.h.
//
// Everything is read from the workspace the last count left (sc_pairs.h): the points in index order, the hashed cell table,
// the members in bucket order with their positions and cells, n and the domain flag.  The caller's points are not read
// again.  Then
//   k_cluster_init   parent[i] = i: every point a set of its own;
//   k_cluster_union  a thread per row walks the buckets of its point's nine cells as k_pairs_count does -- the own-cell
//                    test, pairs_accept's arithmetic, `half` off -- and unites its set with that of every partner j < i:
//                    both roots are found (with path halving), the LARGER root is hooked under the smaller by a
//                    compare-and-swap on its parent word, and a failed swap finds again from the value it returned;
//   k_cluster_jump   parent[i] = parent[parent[i]], ceil(log2(max(m, 2))) launches whatever the data: afterwards every
//                    parent is its root.  The kernel boundaries are the synchronisation;
//   k_cluster_mark / k_scan_local / k_scan_fix (sc_kernels.h) / k_cluster_write / k_cluster_finish
//                    the roots get the numbers 0 .. C-1 in index order by an exclusive scan of "is a root", every point
//                    its root's number, every cluster its root and -- integer atomics into an int workspace, one per
//                    run of equal numbers in a wave, then widened -- its size.
// The invariant: parent[x] <= x, always.  A hook lowers a root's parent, a halving or a jump replaces a parent by an
// ancestor further up, so a set's root is its smallest member whatever order the atomics take: the result does not depend
// on timing, and neither on which of a pair's threads did the uniting (a thread unites with j < i only: every edge once).
//
// Memory.  In k_cluster_union `parent` is written and read by different CUs inside one launch, and a CU's L1 is never
// refreshed by another CU's stores: every read of it there is a relaxed agent-scope atomic load (served past the L1), every
// write an agent-scope atomic (the swap; atomicMin for the halving, which can only lower a word).  A stale value would
// still be an ancestor -- the swap is the only judge of who is a root -- but there is none to reason about.
// Nothing waits: a failed swap means that another hook has succeeded (at most n - 1 do), and the root it is retried on is
// smaller than the last one, so a thread's retries are bounded too.  No workgroup polls for another; no spin, flag or
// ticket.  The depth of the trees the union kernel leaves is not bounded by it: the jump launches bound it afterwards, so
// the finds need no depth guarantee to be correct, and no later thread walks a chain.
//
// With the domain flag up every kernel returns at once, except that counts[1] = -1 is written.
//
// The batched form (sc_pairs_label_batch_device, on the grid of a count after sc_pairs_set_batch_device): an edge never
// crosses clouds.  k_cluster_union<true> reads its row's record once (pairs_row, sc_pairs.h), hashes with the row's
// cloud and skips a candidate below the cloud's first row; everything after the union is the unbatched label -- labels
// and roots are global, and because a cloud is a range of rows and clusters are numbered by their smallest member, cloud
// b's clusters are a contiguous range: k_cluster_ptr reads its ends out of the scan the label makes anyway.  Bad batch
// offsets were found by the count: counts[1] = -3 and nothing else.  The label is left valid, so
// sc_pairs_cluster_sums_device reads it as it reads any other.
#pragma once
#include "sc_pairs.h"

namespace sc {

__device__ __forceinline__ bool cluster_finite(XY p) { return fabs(p.x) < __builtin_inf() && fabs(p.y) < __builtin_inf(); }

__device__ __forceinline__ int cluster_parent(const int* parent, int x) {
  return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's set.  Path halving: every other node on the way is handed to its grandparent (atomicMin: another thread
// may have lowered the word further meanwhile).  Ends: parent[x] < x until the root.
__device__ __forceinline__ int cluster_find(int* parent, int x) {
  for (;;) {
    const int p = cluster_parent(parent, x);
    if (p == x) return x;
    const int g = cluster_parent(parent, p);
    if (g == p) return p;
    __hip_atomic_fetch_min(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
}

// Unites the sets of a and b and yields the root of the union as far as this thread knows it (an ancestor of both).
__device__ __forceinline__ int cluster_unite(int* parent, int a, int b) {
  a = cluster_find(parent, a);
  b = cluster_find(parent, b);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(&parent[hi], hi, lo);
    if (old == hi) return lo;
    a = cluster_find(parent, old);  // hi was hooked by another thread meanwhile: old < hi is its parent
    b = cluster_find(parent, lo);
  }
  return a;
}

__global__ void __launch_bounds__(kBlock)
    k_cluster_init(const long long* __restrict__ words, const int* __restrict__ flag, int m, int* __restrict__ parent) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= m || *flag || i >= words[PW_N]) return;
  parent[i] = i;
}

// `v.g.half` is off (the view's): the graph is the full one, and each edge is united from its larger end.  A bucket's
// members ascend in index (the binning sort is stable), so a run is left at the first j >= i, before its cell is even read:
// that early exit is this reader's alone, one more reason why it keeps its own loop over the view (sc_pairs.h).
// Batched: the row's record (lo, hi, cloud) comes from pairs_row, the buckets hash with the row's cloud, and of pairs_in
// only j >= lo is left to test -- j < i < hi already.  The unbatched instantiation carries no record.
template <bool batched>
__global__ void __launch_bounds__(kBlock) k_cluster_union(PairsView v, int m, int* parent) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= m || *v.flag || i >= v.words[PW_N]) return;
  const XY p = v.xy[i];
  if (!cluster_finite(p)) return;
  const PairsRow row = pairs_row<batched>(v.bt, i);
  const unsigned cx0 = pairs_cell(p.x, v.g.h), cy0 = pairs_cell(p.y, v.g.h);
  int root = i;  // an ancestor of i: where the next find starts
  for (int c = 0; c < 9; ++c) {
    const unsigned cx = cx0 + (unsigned)(c % 3 - 1), cy = cy0 + (unsigned)(c / 3 - 1);
    const unsigned b = pairs_bucket(cx, cy, row.cloud, v.g.mask);
    const int end = v.start[b + 1];
    for (int k = v.start[b]; k < end; ++k) {
      const int j = v.sidx[k];
      if (j >= i) break;
      if (batched && j < row.lo) continue;  // (another cloud's member, met by collision)
      const uint2 cell = v.scell[k];
      double d2;
      if (cell.x == cx && cell.y == cy && pairs_accept(v.g, i, j, p, v.sxy[k], d2)) root = cluster_unite(parent, root, j);
    }
  }
}

// One round of pointer jumping, in place.  The race is benign: a thread reads another's parent before or after that thread
// has replaced it, and either value is an ancestor -- values only decrease towards the root --, so a round at least halves
// every depth, as the synchronous round would.  A thread whose parent is a root does nothing.
__global__ void __launch_bounds__(kBlock)
    k_cluster_jump(const long long* __restrict__ words, const int* __restrict__ flag, int m, int* parent) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= m || *flag || i >= words[PW_N]) return;
  const int p = cluster_parent(parent, i);
  const int g = cluster_parent(parent, p);
  if (g != p) __hip_atomic_store(&parent[i], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// isRoot over the whole bound (0 from n on: the scan runs over m), and the clusters' counters cleared.
__global__ void __launch_bounds__(kBlock)
    k_cluster_mark(const long long* __restrict__ words, const int* __restrict__ flag, int m, const XY* __restrict__ xy,
                   const int* __restrict__ parent, int* __restrict__ isRoot, int* __restrict__ sizeW) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= m || *flag) return;
  isRoot[i] = i < words[PW_N] && cluster_finite(xy[i]) && parent[i] == i;
  sizeW[i] = 0;
}

// dense[r] is the number of root r (the exclusive scan of isRoot).  Sizes: integer adds, a count does not depend on their
// order -- one add per run of equal numbers among the lanes of a wave (lane_run, sc_device.h), not one per point: a body
// of water is one cluster, and a million adds to one word take their turns, 12 ms of them.  A lane without a cluster
// carries a key of its own.  Every lane of the wave reaches lane_run: no early return.
__global__ void __launch_bounds__(kBlock)
    k_cluster_write(const long long* __restrict__ words, const int* __restrict__ flag, int m, const XY* __restrict__ xy,
                    const int* __restrict__ parent, const int* __restrict__ dense, int* __restrict__ sizeW,
                    long long* __restrict__ labels, long long* __restrict__ roots, long long room_clusters) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  int d = -1 - (int)(threadIdx.x & 63);
  if (i < m && !*flag && i < words[PW_N]) {
    if (cluster_finite(xy[i])) {
      const int r = parent[i];
      d = dense[r];
      labels[i] = d;
      if (r == i && roots && d < room_clusters) roots[d] = i;
    } else {
      labels[i] = -1;
    }
  }
  const LaneRun run = lane_run(d);
  if (d >= 0 && run.is_head) atomicAdd(&sizeW[d], run.len);
}

// ... the sizes widened into the caller's array, below the room, and the two words.  With the count's flag up:
// counts[1] = -1 (the domain) or -3 (the offsets of a batched count), nothing else.
__global__ void __launch_bounds__(kBlock)
    k_cluster_finish(const long long* __restrict__ words, const int* __restrict__ flag, int m, const int* __restrict__ dense,
                     const int* __restrict__ sizeW, long long* __restrict__ sizes, long long room_clusters,
                     long long* __restrict__ counts) {
  const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (const int up = *flag) {
    if (c == 0) counts[1] = pairs_status(up);
    return;
  }
  const int total = dense[m];
  if (c == 0) {
    counts[0] = words[PW_N];
    counts[1] = total;
  }
  if (sizes && c < total && c < room_clusters) sizes[c] = sizeW[c];
}

// The batched label's offset table, a thread per entry: cluster_ptr[b] is the number of roots below ptr[b], which is
// dense[ptr[b]] -- clusters are numbered by their smallest member and a cloud is a range of rows, so cloud b's clusters
// are cluster_ptr[b] .. cluster_ptr[b + 1].  ptr[b] <= n <= m, and the scan has written dense[0 .. m]: isRoot is 0 from n
// on, so the last entry, dense[n], is C even when n = m.  With the flag up nothing is written.
__global__ void __launch_bounds__(kBlock)
    k_cluster_ptr(const int* __restrict__ flag, const long long* __restrict__ ptr, int clouds, const int* __restrict__ dense,
                  long long* __restrict__ cluster_ptr) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b > clouds || *flag) return;
  cluster_ptr[b] = dense[ptr[b]];
}

}  // namespace sc
