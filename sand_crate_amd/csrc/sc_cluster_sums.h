// Per-cluster sums and extents on the device (sc_pairs_cluster_sums_device): for every cluster of the last label the sum,
// and optionally the minimum and the maximum, of up to kClusterSumsMaxChannels float64 channels over the cluster's members.
// The rule is specified in NumPy by tests/cluster_sums_spec.py: the sum of a cluster is `tree` of its members' values in
// ascending index -- pairwise summation in groups of 64, and groups of groups, padded with +0.0 --, so the result is a pure
// function of the cluster's own members: the same bits on every call, whatever the other clusters, the capacity, the
// bucket count or the launch bound are.  Included once by sandcrate_hip.hip, after sc_clusters.h.
//
// A reader of what sc_pairs_label_device left (sc_clusters.h): parent and the root marks with their scan (dense[parent[i]]
// is the label of a point whose parent is a marked root; any other row is dead), the clusters' sizes, and n and the flag
// of the pairs workspace.  Of the caller's it reads `values` and nothing else.  Nothing of those workspaces is written.
//   k_reader_check   (sc_pairs.h) prepares counts[1] and raises the flag OF THIS CALL when `values` has fewer rows than
//                    the count has points (n is known on the device only); the count's flag stays as the count left it;
//   radix_sort       (sc_radix.h) with CsumKey, a stable sort of (label, index) in a RadixSpace of its own, a dead row's
//                    key behind every cluster: the members of a cluster end up contiguous and ascending in index.  The
//                    number of passes comes from the launch bound m alone;
//   k_csum_count / k_scan_local / k_scan_fix (sc_kernels.h)
//                    the exclusive scans that say where things start: of the sizes (a cluster's members in the sorted
//                    order), of ceil(size / 64) (its chunks: the work items of level 0), and per upper level of the
//                    number of items a cluster still has there.  All of them are functions of the size (csum_elems);
//   k_csum_items     a thread per sorted position: the first of every 64 members of a cluster, counted from the cluster's
//                    start and not from the array's, enters its chunk in the item list (cluster, chunk);
//   k_csum_reduce    level 0 .. L - 1, L = ceil(log64(m)) launches whatever the data.  A GROUP OF LANES per item: a lane
//                    takes element 64 * chunk + l of the cluster -- at level 0 values[index] of a member, a row of 8
//                    channels is one 64-byte read; above, the partials of the level below -- or +0.0 beyond the cluster's
//                    end, and the xor butterfly, xor_lane<1> .. xor_lane<32>, is the group of 64 of the rule: a
//                    commutative add gives every lane the same bits.  A wave walks its share of the items: its lanes
//                    fetch the next 64, and the narrowest power of two W whose first 64 / W items have at most W elements
//                    is the width of a group, so the wave reduces 64 / W items at once with the first log2(W) steps of the
//                    butterfly (the remaining steps only add the padding: one + 0.0).  A full chunk has the whole wave,
//                    64 singletons are one pass of a thread each.  A cluster with one item at a level gets its result
//                    written there; one with more gets a partial per item, and every 64th item enters the next level's
//                    list.  The items are dealt to the waves in equal contiguous shares (their number is read from the
//                    scan's last entry): no workgroup waits for another, no spin, ticket or poll, no atomics of any kind.
//                    MEASURED (profiles/cluster_sums_time.txt, 1,048,576 points, 8 channels with extrema, the whole
//                    reduction on the device): with the whole wave on every item, all singletons took 2.28 ms -- one
//                    live lane per wave -- and one giant cluster 0.27 ms; with 64 items per wave taken in turn, 0.38 ms
//                    and 0.87 ms -- few waves, each waiting for its loads 64 times; with the shares, 0.38 and 0.27 ms;
//   k_csum_finish    counts[0] = n and counts[1] = C, or the status.
// Minima and maxima take the same path with probe_min / probe_max (sc_probe.h: a NaN on either side is the result), the
// padding is +inf / -inf.  They do not depend on order.
//
// Registers.  The channels live in register arrays indexed by unrolled loops only -- the kernel is instantiated for 1, 2, 4
// and 8 channels as k_fields_sum is, and once per group width --, so nothing is indexed dynamically and no kernel here uses
// scratch (DESIGN.md has the table).
//
// With the count's flag or the call's own up every kernel returns at once; only counts[1] is written.
#pragma once
#include "sc_clusters.h"
#include "sc_probe.h"
#include "sc_radix.h"

namespace sc {

constexpr int kClusterSumsMaxChannels = 8;
constexpr int kCsumGroup = 64;  // the rule's group: a wave

// The flags every kernel here looks at first, and n.
struct CsumGuard {
  const long long* words;
  const int* flag;  // the count's
  const int* own;   // the call's
};

__device__ __forceinline__ bool csum_off(const CsumGuard& g) { return *g.flag || *g.own; }

// The elements a cluster of s members has at `level`: its members at level 0; above, the items it had one level below
// if they were more than one (a cluster with one item is finished there).  Its items at a level: ceil(elements / 64).
__host__ __device__ __forceinline__ int csum_elems(int s, int level) {
  int e = s;
  for (int k = 0; k < level; ++k) {
    const int items = (e + kCsumGroup - 1) / kCsumGroup;
    e = items > 1 ? items : 0;
  }
  return e;
}

// The sort's key: the label, or m -- behind every cluster, C <= n <= m -- for a row in none.
struct CsumKey {
  const long long* words;
  const int* flag;
  const int* own;
  const int* parent;
  const int* isRoot;
  const int* dense;
  int m;
  __device__ __forceinline__ unsigned operator()(int i) const {
    // (the label is loaded before it is chosen: written as `root ? dense[r] : m` the compiler selects between the two
    // ADDRESSES, and m, a kernel argument, goes to scratch to have one)
    const unsigned dead = (unsigned)m;
    unsigned key = dead;
    if (!(*flag | *own) && i < words[PW_N]) {
      const int r = parent[i];
      const unsigned d = (unsigned)dense[r];
      key = isRoot[r] ? d : dead;  // (a point that is not finite is its own parent and no root)
    }
    return key;
  }
};

// out[c] = the elements (`as_elems`) or the items of cluster c at `level`, over the whole bound: sizes from C on are 0.
__global__ void __launch_bounds__(kBlock)
    k_csum_count(CsumGuard g, int m, const int* __restrict__ size, int level, int as_elems, int* __restrict__ out) {
  const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (c >= m) return;
  int v = 0;
  if (!csum_off(g)) {
    v = csum_elems(size[c], level);
    if (!as_elems) v = (v + kCsumGroup - 1) / kCsumGroup;
  }
  out[c] = v;
}

// The items of level 0.  `keys` are the sorted labels, `member_start` and `chunk_start` the scans of the sizes and of the
// chunk counts: position p is member p - member_start[c] of its cluster.
__global__ void __launch_bounds__(kBlock)
    k_csum_items(CsumGuard g, int m, const unsigned* __restrict__ keys, const int* __restrict__ member_start,
                 const int* __restrict__ chunk_start, int2* __restrict__ items) {
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= m || csum_off(g)) return;
  const unsigned c = keys[p];
  if (c >= (unsigned)m) return;  // dead
  const int o = p - member_start[c];
  if (o & (kCsumGroup - 1)) return;
  items[chunk_start[c] + o / kCsumGroup] = int2{(int)c, o / kCsumGroup};
}

// A level as its kernel sees it.
struct CsumLevel {
  int level;
  const int2* items;      // (cluster, item within the cluster)
  const int* total;       // how many items there are: the last entry of their scan
  const int* in_start;    // per cluster: where its elements start -- in the sorted order (level 0), in part_in (above)
  const int* out_start;   // per cluster: where its partials go in part_out
  const int* next_start;  // per cluster: where its items of the next level go in next_items; null at the last level
  int2* next_items;
};

// ... and what it reads and writes.  The partials: three arrays of `cap` rows, sums, minima, maxima.
struct CsumIo {
  const double* values;
  const int* sidx;  // the members in sorted order
  const double* part_in;
  double* part_out;
  long long cap;
  double *sums, *mins, *maxs;  // (room, channels); mins and maxs may be null
  long long room;
  int channels;
};

// One step of the butterfly, for the groups of W lanes that are wider than J.
template <int J, int W, int C>
__device__ __forceinline__ void csum_stage(double (&s)[C], double (&lo)[C], double (&hi)[C], bool extrema) {
  if constexpr (W > J) {
#pragma unroll
    for (int f = 0; f < C; ++f) s[f] = s[f] + xor_lane<J>(s[f]);
    if (extrema) {
#pragma unroll
      for (int f = 0; f < C; ++f) {
        lo[f] = probe_min(lo[f], xor_lane<J>(lo[f]));
        hi[f] = probe_max(hi[f], xor_lane<J>(hi[f]));
      }
    }
  }
}

// What a lane knows of the item it fetched for its wave: the cluster, the item within it, the elements the cluster has at
// this level, and where this item's begin and how many they are (0: no item).
struct CsumItem {
  int c, j, elems, start, len;
};

// 64 / W items at once: each group of W lanes reduces one item of at most W elements, group g the item lane g fetched.
// The first log2(W) steps of the butterfly are the tree over the item's first W places; the places from W on hold the
// padding, and all that the tree's remaining steps do is add +0.0, once said, said for all.  Every lane of the wave
// comes in here.
template <int W, int C, bool first>
__device__ __forceinline__ void csum_block(const CsumLevel& lv, const CsumIo& io, const CsumItem& mine, bool extrema) {
  const int lane = (int)threadIdx.x & 63;
  const int channels = io.channels;
  const int q = lane / W, r = lane & (W - 1);
  const int c = __shfl(mine.c, q, 64), j = __shfl(mine.j, q, 64), elems = __shfl(mine.elems, q, 64);
  const int start = __shfl(mine.start, q, 64), len = __shfl(mine.len, q, 64);
  double s[C], lo[C], hi[C];
#pragma unroll
  for (int f = 0; f < C; ++f) {
    s[f] = 0.0;
    lo[f] = __builtin_inf();
    hi[f] = -__builtin_inf();
  }
  if (r < len) {
    const long long pos = (long long)start + r;
    if (first) {
      const double* src = io.values + (long long)io.sidx[pos] * channels;
#pragma unroll
      for (int f = 0; f < C; ++f)
        if (f < channels) s[f] = lo[f] = hi[f] = src[f];
    } else {
      const double* src = io.part_in + pos * channels;
#pragma unroll
      for (int f = 0; f < C; ++f)
        if (f < channels) s[f] = src[f];
      if (extrema) {
#pragma unroll
        for (int f = 0; f < C; ++f)
          if (f < channels) {
            lo[f] = src[io.cap * channels + f];
            hi[f] = src[2 * io.cap * channels + f];
          }
      }
    }
  }
  csum_stage<1, W>(s, lo, hi, extrema);
  csum_stage<2, W>(s, lo, hi, extrema);
  csum_stage<4, W>(s, lo, hi, extrema);
  csum_stage<8, W>(s, lo, hi, extrema);
  csum_stage<16, W>(s, lo, hi, extrema);
  csum_stage<32, W>(s, lo, hi, extrema);
  if constexpr (W < kCsumGroup) {
#pragma unroll
    for (int f = 0; f < C; ++f) s[f] = s[f] + 0.0;
  }
  if (r != 0 || len == 0) return;  // (nothing below needs the wave)
  if (elems <= kCsumGroup) {       // the cluster's only item here: its result
    if (c < io.room) {
      const long long o = (long long)c * channels;
#pragma unroll
      for (int f = 0; f < C; ++f)
        if (f < channels) {
          io.sums[o + f] = s[f];
          if (io.mins) io.mins[o + f] = lo[f];
          if (io.maxs) io.maxs[o + f] = hi[f];
        }
    }
  } else {
    const long long o = ((long long)lv.out_start[c] + j) * channels;
#pragma unroll
    for (int f = 0; f < C; ++f)
      if (f < channels) {
        io.part_out[o + f] = s[f];
        if (extrema) {
          io.part_out[io.cap * channels + o + f] = lo[f];
          io.part_out[2 * io.cap * channels + o + f] = hi[f];
        }
      }
    if ((j & (kCsumGroup - 1)) == 0) lv.next_items[lv.next_start[c] + j / kCsumGroup] = int2{c, j / kCsumGroup};
  }
}

// Do the first 64 / W of the items the lanes fetched have at most W elements each?  (The same answer in every lane.)
template <int W>
__device__ __forceinline__ bool csum_fits(int len) {
  constexpr int G = kCsumGroup / W;
  const unsigned long long over = __ballot(len > W);
  return (over & (G == 64 ? ~0ull : (1ull << G) - 1ull)) == 0ull;
}

// `first`: level 0, the elements are the caller's values.  The items are dealt to the waves in equal contiguous shares
// -- a function of their number and of the launch, not of the data.  A wave walks its share: the lanes fetch the next (up
// to) 64 items, the narrowest width W whose first 64 / W items all fit is taken, those are reduced at once, and the walk
// goes on behind them.  With few items, or long ones, a share is an item or two and the whole wave is on each.
template <int C, bool first>
__global__ void __launch_bounds__(kBlock) k_csum_reduce(CsumGuard g, CsumLevel lv, CsumIo io, const int* __restrict__ size) {
  if (csum_off(g)) return;
  const int lane = (int)threadIdx.x & 63;
  const int waves = (int)gridDim.x * (kBlock / 64);
  const int total = *lv.total;
  const bool extrema = io.mins != nullptr || io.maxs != nullptr;
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kBlock + threadIdx.x) >> 6);
  const int share = (total + waves - 1) / waves;
  const long long begin = (long long)wave * share;
  if (begin >= total) return;  // (the wave's own: every lane leaves)
  const int end = (int)min((long long)total, begin + share);
  for (int cur = (int)begin; cur < end;) {
    CsumItem mine{0, 0, 0, 0, 0};
    if (cur + lane < end) {
      const int2 it = lv.items[cur + lane];
      mine.c = it.x;
      mine.j = it.y;
      mine.elems = csum_elems(size[it.x], lv.level);
      mine.start = lv.in_start[it.x] + it.y * kCsumGroup;
      mine.len = min(kCsumGroup, mine.elems - it.y * kCsumGroup);
    }
    if (csum_fits<1>(mine.len)) {
      csum_block<1, C, first>(lv, io, mine, extrema);
      cur += 64;
    } else if (csum_fits<2>(mine.len)) {
      csum_block<2, C, first>(lv, io, mine, extrema);
      cur += 32;
    } else if (csum_fits<4>(mine.len)) {
      csum_block<4, C, first>(lv, io, mine, extrema);
      cur += 16;
    } else if (csum_fits<8>(mine.len)) {
      csum_block<8, C, first>(lv, io, mine, extrema);
      cur += 8;
    } else if (csum_fits<16>(mine.len)) {
      csum_block<16, C, first>(lv, io, mine, extrema);
      cur += 4;
    } else if (csum_fits<32>(mine.len)) {
      csum_block<32, C, first>(lv, io, mine, extrema);
      cur += 2;
    } else {
      csum_block<64, C, first>(lv, io, mine, extrema);
      cur += 1;
    }
  }
}

// With a flag up: counts[1] = the status, nothing else.
__global__ void k_csum_finish(CsumGuard g, const int* __restrict__ dense, int m, long long* __restrict__ counts) {
  if (threadIdx.x || blockIdx.x) return;
  if (csum_off(g)) {
    counts[1] = reader_status(*g.flag, *g.own);
    return;
  }
  counts[0] = g.words[PW_N];
  counts[1] = dense[m];
}

}  // namespace sc
