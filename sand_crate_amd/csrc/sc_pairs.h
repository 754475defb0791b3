// Fixed-radius pair lists on the device (sc_pairs_count_device / sc_pairs_fill_device): for n points and a radius, the
// CSR list of all (i, j), i != j, whose rounded squared distance is at most the rounded radius * radius -- offsets (the
// exclusive scan of the row lengths, 64 bit) and partners, row by row and ascending in j.  The rule is specified in NumPy
// by tests/pairs_spec.py; the result is a pure function of the points.  Included once by sandcrate_hip.hip.
//
// The points are the caller's array, or the state in particle-index order: the export's ranking and its rule of the
// live rows (sc_state.h), and k_pairs_gather.  Either way they are copied into the context's workspace, so the fill does not read the caller's memory
// again.  Then
//   k_pairs_key     the cell of every point, (floor(x / h), floor(y / h)), its bucket in a hashed table of kPairsLoad * n
//                   buckets (a power of two; pairs_bucket below) and the bucket's count (integer atomics: a count does not
//                   depend on their order).  The key of a point is its bucket; a point with a coordinate that is not
//                   finite gets the key `buckets`, which sorts behind all of them: it is in no bucket, so it is
//                   nobody's partner.  The same kernel raises the domain flag (below);
//   the stable radix sort of sc_radix.h over those (bucket, index) pairs, as many passes of eight bits as the bucket index
//                   has: every bucket's members end up contiguous and ascending in index;
//   k_scan_* over the buckets' counts: where every bucket starts;
//   k_pairs_place   the members' positions and cells in that order (a candidate is then one 16-byte and one 8-byte read);
//   k_pairs_count   a thread per row walks the buckets of its point's nine cells and counts the partners;
//   k_scan64_local / k_scan64_fix  the exclusive scan of the row lengths in 64 bits -- the two levels of k_scan_local /
//                   k_scan_fix (sc_kernels.h), no workgroup waits for another -- into the workspace and the caller's
//                   offsets, and E;
//   k_pairs_fill    a thread per row merges its nine runs (each ascending in j) by always taking the smallest head; the
//                   cursors live in LDS (a dynamically indexed register array would go to scratch).
// A hashed table: the bounding box is known on the device only, and a loaded state may be arbitrarily sparse.  Several of
// one point's nine cells may share a bucket, so a candidate is accepted only when its OWN cell is the cell looked for:
// every candidate is then seen exactly once.  No floating-point atomics, nothing that decides the output depends on the
// order of an atomic.
//
// The cell rule.  The decision is d2 = fl(fl(dx dx) + fl(dy dy)) <= fl(radius radius) with dx = fl(x_i - x_j), never the
// cells: the 3 x 3 search must only never lose such a pair.  With radius^2 a normal finite number (checked on the host),
// a pair has |x_i - x_j| <= radius (1 + 2^-50): three roundings on the way to d2, one in radius^2.  The computed cell is
// floor(fl(x / h)); fl(x / h) is off by at most 2^-53 |x / h| <= 2^-22 cells inside the domain |x| / radius < 2^31 (so
// 0.03 / 0.01 may well floor to 3 where 0.03 < 3 * 0.01).  With h = fl(radius (1 + 2^-20)) the computed quotients of a
// pair differ by at most (1 + 2^-50) / ((1 + 2^-20)(1 - 2^-53)) + 2^-21 < 1, and two numbers that differ by at most 1
// have floors that differ by at most 1.  The same for y.  So the cell is a little larger than the radius, by a factor the
// rounding of the division cannot use up at the largest cell index there is.
// The domain: every finite coordinate needs fl(|c| / radius) < 2^31, so that its cell is an int (h > radius: its quotient
// is no larger).  k_pairs_key raises a flag otherwise; every later kernel of the count and of the fill returns at once when
// it is up, except that E = -1 is written: no host round trip.  Inside the domain |cell| <= 2^31 / (1 + 2^-20), 2047
// short of the ends of int, so cx +- 1 does not overflow (the cells are kept as unsigned words all the same).
//
// The batched form (sc_pairs_set_batch_device before the count): the points are B disjoint clouds, cloud b the rows
// ptr[b] .. ptr[b + 1] of B + 1 ascending 64-bit offsets, and j is a partner of row i only when both lie in one cloud.
// Frames of one scene overlap completely in space, and shifting them apart would round dx differently, so the clouds
// share the one grid.  k_pairs_batch_check copies ptr into the workspace and tests it (first entry 0, no descent, last
// entry n: otherwise the flag's second bit goes up, and E = -3); k_pairs_key finds every point's cloud by binary search,
// keeps it as one int per point and mixes it into the bucket hash -- cloud 0 hashes exactly as an unbatched point does --,
// so that clouds which share a cell land in different buckets, except by collision.  Exactness does not rest on the hash:
// besides the own-cell test a candidate j must lie in the row's [lo, hi) = [ptr[b], ptr[b + 1]), two compares on the
// sidx[k] that pairs_accept needs anyway.  A row reads its record (lo, hi, cloud) once, before its nine cells -- a point
// from the workspace, a query by binary search over query_ptr --, nothing is read per candidate.  The sort, the scans,
// k_pairs_place and scell are as they are.  Every kernel that walks is a template on `batched`: the unbatched
// instantiation carries no record at all.  The clusters, the histograms, the rays and the ray paths (sc_clusters.h,
// sc_hist.h, sc_rays.h) read a batched grid through entry points of their own (sc_pairs_label_batch_device,
// sc_pairs_hist_batch_device, sc_pairs_rays_batch_device, sc_pairs_ray_paths_batch_device): their outputs have other
// shapes -- a cluster offset table, totals per cloud -- and the unbatched calls keep refusing a batched grid.  Each pair
// shares one host body and one kernel template.
//
// The readers.  The workspace a count leaves is read by the fill and by the clusters, the nearest-k tables, the weighted
// sums, their position gradient and the distance histograms (sc_clusters.h, sc_nearest.h, sc_fields.h, sc_fields_grad.h,
// sc_hist.h).  What they share is here, once: PairsView, the workspace as a reader sees it; pairs_merge, a row's partners
// ascending in j, for the fill and the sums (the gradient writes the same merge out, sc_fields_grad.h says on what
// measurement); k_reader_check with the readers' flag bits and reader_status.
// None of it knows who calls: what a reader does with a partner is the callable it hands in.
// The plain walk -- the nine cells in raster order, the own-cell test, pairs_in, pairs_accept -- stays written out in
// k_pairs_count, k_nearest, k_hist and k_cluster_union.  As one function with a callable it was built and MEASURED: the
// compiler orders the three loads of a candidate (cell, index, position) differently per kernel today -- k_hist issues
// index and position together, k_pairs_count one after the other -- and gave the shared loop one order for all: k_hist
// 9 to 15 % and k_nearest 2 to 10 % slower, k_pairs_count 1 % either way (profiles/readers_refactor.txt).
#pragma once
#include "sc_device.h"
#include "sc_kernels.h"
#include "sc_state.h"

namespace sc {

constexpr int kPairsLoad = 2;               // buckets per point, at least (then rounded up to a power of two)
constexpr unsigned kPairsMinBuckets = 256;
constexpr unsigned kPairsHashX = 0x9E3779B1u, kPairsHashY = 0x85EBCA77u, kPairsHashMix = 0x2C1B3C6Du;
constexpr unsigned kPairsHashCloud = 0xC2B2AE3Du;  // the batched form's third factor
constexpr int kPairsFlagDomain = 1, kPairsFlagBatch = 2;  // the bits of the count's flag
// the bits of a reader's own flag: a query outside the domain, an array of the caller's with too few rows, bad query offsets
constexpr int kReaderFlagDomain = 1, kReaderFlagRows = 2, kReaderFlagBatch = 4;
constexpr long long kPairsStatusDomain = -1, kPairsStatusRows = -2, kPairsStatusBatch = -3;
constexpr double kPairsCellFactor = 1.0 + 1.0 / 1048576.0;  // h = radius * (1 + 2^-20)
constexpr double kPairsDomain = 2147483648.0;                // |c| / radius must stay below 2^31

// the workspace's 64-bit words
enum PairsWord { PW_N = 0, PW_E = 1, PW_WORDS = 2 };

struct PairsGrid {
  double h, radius, r2;
  unsigned mask;  // buckets - 1
  int half;       // keep j > i only
};

// The batched grid as the kernels see it: the workspace's copy of ptr, the points' clouds, and -- query form -- the
// caller's query_ptr.  All null and 0 in the unbatched instantiations, which never look.
struct PairsBatch {
  const long long* ptr;   // clouds + 1 offsets into the points (the workspace's copy)
  const long long* qptr;  // clouds + 1 offsets into the queries, or null: the self form
  const int* cloud;       // the cloud of every point
  int clouds;
};

// What a row carries through its walk: its partners are the indices lo <= j < hi, and its cells hash with `cloud`.
struct PairsRow {
  int lo, hi;
  unsigned cloud;
};

__device__ __forceinline__ unsigned pairs_bucket(unsigned cx, unsigned cy, unsigned cloud, unsigned mask) {
  unsigned v = (cx * kPairsHashX) ^ (cy * kPairsHashY) ^ (cloud * kPairsHashCloud);  // (cloud 0: the unbatched hash)
  v ^= v >> 15;
  v *= kPairsHashMix;
  v ^= v >> 13;
  return v & mask;
}

// The workspace as a reader sees it, by value in every kernel that reads the grid (k_nearest and k_fields_grad take it
// unpacked: sc_nearest.h, sc_fields_grad.h): the grid, n and E, the count's flag,
// the points in index order, where every bucket starts, and the members in bucket order -- positions, cells, indices.
struct PairsView {
  PairsGrid g;
  const long long* words;
  const int* flag;
  const XY* xy;
  const int* start;
  const XY* sxy;
  const uint2* scell;
  const int* sidx;
  PairsBatch bt;
};

// The cloud of row i: the last b < clouds with ptr[b] <= i (empty clouds before it are skipped).  Reads entries
// 0 .. clouds - 1 only, whatever they hold.
__device__ __forceinline__ int pairs_cloud_of(const long long* __restrict__ ptr, int clouds, long long i) {
  int lo = 0, hi = clouds;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <bool batched>
__device__ __forceinline__ PairsRow pairs_row(const PairsBatch& bt, long long i) {
  PairsRow r{0, INT_MAX, 0u};
  if (batched) {
    const int b = bt.qptr ? pairs_cloud_of(bt.qptr, bt.clouds, i) : bt.cloud[i];
    r.lo = (int)bt.ptr[b];
    r.hi = (int)bt.ptr[b + 1];
    r.cloud = (unsigned)b;
  }
  return r;
}

template <bool batched>
__device__ __forceinline__ bool pairs_in(const PairsRow& r, int j) {
  return !batched || (j >= r.lo && j < r.hi);
}

__device__ __forceinline__ long long pairs_status(int flag) {
  return (flag & kPairsFlagBatch) ? kPairsStatusBatch : kPairsStatusDomain;
}

// counts[1] of a reader with a flag up: `flag` the count's, `own` the call's.  Bad offsets first, then the domain, then the
// rows.  A reader that never raises a bit never gets its status: the nearest and the histogram hand k_reader_check no row
// counts, so -2 is the sums' and the gradient's alone; the unbatched histogram refuses a batched grid, so neither the
// count's batch bit nor its own is ever up and -1 is all it reports (the batched one reports -3 too); and on an unbatched
// grid no reader has query offsets to be wrong.
__device__ __forceinline__ long long reader_status(int flag, int own) {
  if ((flag & kPairsFlagBatch) || (own & kReaderFlagBatch)) return kPairsStatusBatch;
  return flag || (own & kReaderFlagDomain) ? kPairsStatusDomain : kPairsStatusRows;
}

// The domain rule, for the absolute value of one coordinate: finite, and fl(|c| / radius) not below 2^31.
__device__ __forceinline__ bool pairs_outside(double c_abs, double radius) {
  return c_abs < __builtin_inf() && !(c_abs / radius < kPairsDomain);  // (NaN compares false: not outside, just dead)
}

__device__ __forceinline__ unsigned pairs_cell(double c, double h) { return (unsigned)(int)floor(c / h); }

// The state form: row k is the slot with the k-th smallest id, as in k_state_gather.
__global__ void __launch_bounds__(kBlock)
    k_pairs_gather(const unsigned* __restrict__ keys, const int* __restrict__ slots, int m, const double* __restrict__ x,
                   const double* __restrict__ y, XY* __restrict__ xy, long long* __restrict__ words) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (!state_row_live(keys, k, m, &words[PW_N])) return;
  const int s = slots[k];
  xy[k] = XY{x[s], y[s]};
}

// The batched form's offsets: entry k of the caller's `src` goes to `dst`, the workspace, and `bit` of the flag goes up
// unless src[0] = 0, no entry is below the one before, and src[clouds] = n.  `dst` null: nothing is copied (a query_ptr,
// which a reader's own check tests against the number of queries, with its own flag).
__device__ __forceinline__ void pairs_ptr_check(const long long* __restrict__ src, long long* __restrict__ dst, int clouds,
                                                long long n, long long k, int* __restrict__ flag, int bit) {
  if (k > clouds) return;
  const long long v = src[k];
  if (dst) dst[k] = v;
  const bool bad = k == 0 ? v != 0 : v < src[k - 1];
  if (bad || (k == clouds && v != n)) atomicOr(flag, bit);
}

__global__ void __launch_bounds__(kBlock)
    k_pairs_batch_check(const long long* __restrict__ src, long long* __restrict__ dst, int clouds, long long n,
                        int* __restrict__ flag) {
  pairs_ptr_check(src, dst, clouds, n, (long long)blockIdx.x * blockDim.x + threadIdx.x, flag, kPairsFlagBatch);
}

// `n_host` >= 0: the caller's points, n is known (and written to words); -1: xy is the workspace, n is words[PW_N].
// Batched: `ptr` is the workspace's copy (which k_pairs_batch_check has written), the clouds go to `cloud`.
template <bool batched>
__global__ void __launch_bounds__(kBlock)
    k_pairs_key(PairsGrid g, const XY* __restrict__ src, XY* __restrict__ xy, long long n_host, long long* __restrict__ words,
                int m, unsigned* __restrict__ keys, int* __restrict__ index, int* __restrict__ bucketCount,
                int* __restrict__ flag, const long long* __restrict__ ptr, int clouds, int* __restrict__ cloud) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const long long n = n_host >= 0 ? n_host : words[PW_N];
  if (i == 0 && n_host >= 0) words[PW_N] = n_host;
  if (i >= m) return;
  unsigned key = g.mask + 1u;  // dead: behind every bucket
  if (i < n) {
    const XY p = src[i];
    if (src != xy) xy[i] = p;
    unsigned b = 0u;
    if (batched) {
      b = (unsigned)pairs_cloud_of(ptr, clouds, i);
      cloud[i] = (int)b;
    }
    const double ax = fabs(p.x), ay = fabs(p.y);
    if (pairs_outside(ax, g.radius) || pairs_outside(ay, g.radius)) atomicOr(flag, kPairsFlagDomain);
    else if (ax < __builtin_inf() && ay < __builtin_inf()) {
      key = pairs_bucket(pairs_cell(p.x, g.h), pairs_cell(p.y, g.h), b, g.mask);
      atomicAdd(&bucketCount[key], 1);
    }
  }
  keys[i] = key;
  index[i] = i;
}

// Sorted place k holds point index[k]: its position and cell go there too.
__global__ void __launch_bounds__(kBlock)
    k_pairs_place(PairsGrid g, const unsigned* __restrict__ keys, const int* __restrict__ index, int m,
                  const XY* __restrict__ xy, const int* __restrict__ flag, XY* __restrict__ sxy, uint2* __restrict__ scell) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= m || *flag) return;
  if (keys[k] > g.mask) return;
  const XY p = xy[index[k]];
  sxy[k] = p;
  scell[k] = make_uint2(pairs_cell(p.x, g.h), pairs_cell(p.y, g.h));
}

// Is (i, j) a pair, with p the point i and q the point j; d2 is the number that was compared.
__device__ __forceinline__ bool pairs_accept(const PairsGrid& g, int i, int j, XY p, XY q, double& d2) {
  const double dx = p.x - q.x, dy = p.y - q.y;
  d2 = dx * dx + dy * dy;
  return j != i && (!g.half || j > i) && d2 <= g.r2;
}

// The first place from k on, below `end`, whose point lies in cell (cx, cy) -- and, batched, in the row's cloud -- and is
// a partner of i; `end` when none.
template <bool batched>
__device__ __forceinline__ int pairs_advance(const PairsView& v, const PairsRow& row, int i, XY p, unsigned cx, unsigned cy,
                                             int k, int end) {
  for (; k < end; ++k) {
    const uint2 cell = v.scell[k];
    const int j = v.sidx[k];
    double d2;
    if (cell.x == cx && cell.y == cy && pairs_in<batched>(row, j) && pairs_accept(v.g, i, j, p, v.sxy[k], d2)) break;
  }
  return k;
}

// The merge: a row's partners ascending in j.  The nine runs are each ascending (the sort is stable), the smallest head
// goes out next: f(j, q) with q the partner's position, until f returns false or every run is at its end.  The cursors
// live in the kernel's LDS, a column per thread (a dynamically indexed register array would go to scratch); no barrier:
// every thread is on its own.
template <bool batched, class F>
__device__ __forceinline__ void pairs_merge(const PairsView& v, const PairsRow& row, int me, XY p, int (&s_cur)[9][kBlock],
                                            int (&s_end)[9][kBlock], int (&s_head)[9][kBlock], int tid, F&& f) {
  const unsigned cx0 = pairs_cell(p.x, v.g.h), cy0 = pairs_cell(p.y, v.g.h);
  for (int c = 0; c < 9; ++c) {
    const unsigned cx = cx0 + (unsigned)(c % 3 - 1), cy = cy0 + (unsigned)(c / 3 - 1);
    const unsigned b = pairs_bucket(cx, cy, row.cloud, v.g.mask);
    const int end = v.start[b + 1];
    const int k = pairs_advance<batched>(v, row, me, p, cx, cy, v.start[b], end);
    s_cur[c][tid] = k;
    s_end[c][tid] = end;
    s_head[c][tid] = k < end ? v.sidx[k] : INT_MAX;
  }
  for (;;) {
    int best = INT_MAX, bc = 0;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const int h = s_head[c][tid];
      if (h < best) {
        best = h;
        bc = c;
      }
    }
    if (best == INT_MAX) break;  // every run is at its end
    const int k = s_cur[bc][tid];
    if (!f(best, v.sxy[k])) break;
    const unsigned cx = cx0 + (unsigned)(bc % 3 - 1), cy = cy0 + (unsigned)(bc / 3 - 1);
    const int end = s_end[bc][tid];
    const int next = pairs_advance<batched>(v, row, me, p, cx, cy, k + 1, end);
    s_cur[bc][tid] = next;
    s_head[bc][tid] = next < end ? v.sidx[next] : INT_MAX;
  }
}

// `v.g.half` is the count's.
template <bool batched>
__global__ void __launch_bounds__(kBlock) k_pairs_count(PairsView v, int m, int* __restrict__ rowLen) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= m || *v.flag) return;
  int count = 0;
  if (i < v.words[PW_N]) {
    const XY p = v.xy[i];
    if (fabs(p.x) < __builtin_inf() && fabs(p.y) < __builtin_inf()) {
      const PairsRow row = pairs_row<batched>(v.bt, i);
      const unsigned cx0 = pairs_cell(p.x, v.g.h), cy0 = pairs_cell(p.y, v.g.h);
      for (int c = 0; c < 9; ++c) {
        const unsigned cx = cx0 + (unsigned)(c % 3 - 1), cy = cy0 + (unsigned)(c / 3 - 1);
        const unsigned b = pairs_bucket(cx, cy, row.cloud, v.g.mask);
        const int end = v.start[b + 1];
        for (int k = v.start[b]; k < end; ++k) {
          const uint2 cell = v.scell[k];
          const int j = v.sidx[k];
          double d2;
          if (cell.x == cx && cell.y == cy && pairs_in<batched>(row, j) && pairs_accept(v.g, i, j, p, v.sxy[k], d2)) ++count;
        }
      }
    }
  }
  rowLen[i] = count;
}

// The exclusive scan of in[0 .. n) in 64 bits into out[0 .. n] (out[n] is the total), n = words[PW_N] <= the launch's
// bound: k_scan_local / k_scan_fix with wider sums.  Entries of `in` from n on are not read.
__global__ void __launch_bounds__(kBlock)
    k_scan64_local(const int* __restrict__ in, long long* __restrict__ out, const long long* __restrict__ words,
                   const int* __restrict__ flag, long long* __restrict__ blockSums) {
  if (*flag) return;
  const long long n = words[PW_N];
  const long long base = (long long)blockIdx.x * kScanPerBlock + (long long)threadIdx.x * kScanPerThread;
  long long v[kScanPerThread];
  long long sum = 0;
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) {
    const long long e = base + k < n ? in[base + k] : 0;
    v[k] = sum;
    sum += e;
  }
  const long long excl = scan_block_excl(sum);
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k)
    if (base + k <= n) out[base + k] = excl + v[k];
  if (threadIdx.x == kBlock - 1) blockSums[blockIdx.x] = excl + sum;
}

// ... adds the totals of the workgroups before, writes the caller's copy, and -- the thread that holds entry n -- E and
// the caller's two words.  With the flag up: E = -1 (the domain) or -3 (the batch offsets) and the caller's words, nothing
// else.
__global__ void __launch_bounds__(kBlock)
    k_scan64_fix(long long* __restrict__ out, long long* __restrict__ out_caller, long long* __restrict__ words,
                 const int* __restrict__ flag, const long long* __restrict__ blockSums, long long* __restrict__ counts) {
  const long long n = words[PW_N];
  if (const int up = *flag) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      words[PW_E] = pairs_status(up);
      counts[0] = n;
      counts[1] = pairs_status(up);
    }
    return;
  }
  const long long off = scan_blocks_before(blockSums);
  const long long base = (long long)blockIdx.x * kScanPerBlock + (long long)threadIdx.x * kScanPerThread;
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) {
    if (base + k <= n) {
      const long long v = out[base + k] + off;
      out[base + k] = v;
      out_caller[base + k] = v;
      if (base + k == n) {
        words[PW_E] = v;
        counts[0] = n;
        counts[1] = v;
      }
    }
  }
}

// Row i's partners at offs[i], ascending in j (pairs_merge).  Entry e is written only when e < room.  `v.g.half` is the
// count's.
template <bool batched>
__global__ void __launch_bounds__(kBlock)
    k_pairs_fill(PairsView v, int m, const long long* __restrict__ offs, long long* __restrict__ partners,
                 double* __restrict__ d2_out, long long room) {
  __shared__ int s_cur[9][kBlock], s_end[9][kBlock], s_head[9][kBlock];
  const int tid = (int)threadIdx.x;
  const int i = (int)(blockIdx.x * blockDim.x + tid);
  if (i >= m || *v.flag || i >= v.words[PW_N]) return;  // (no barrier below: every thread is on its own)
  long long e = offs[i];
  const long long row_end = offs[i + 1];
  if (e >= room || e == row_end) return;
  const XY p = v.xy[i];
  pairs_merge<batched>(v, pairs_row<batched>(v.bt, i), i, p, s_cur, s_end, s_head, tid, [&](int j, XY q) {
    double d2;
    (void)pairs_accept(v.g, i, j, p, q, d2);
    partners[e] = j;
    if (d2_out) d2_out[e] = d2;
    ++e;
    return e < room && e < row_end;  // (the runs hold exactly row_end - offs[i] partners)
  });
}

// The check every reader but the fill and the clusters launches first, on the same stream, after its own flag was zeroed:
// thread 0 prepares counts[1] (0, or the count's status) and compares the caller's row counts with what only the device
// knows -- `row_rows` the rows of the arrays that go by row (at least n_queries, or n in the self form), `part_rows` of
// those that go by partner (at least n), -1: no such array --; a thread per query tests it against the domain
// (`queries` null: the self form, nothing to test); and on a batched grid a thread per entry tests `qptr`, the query
// offsets, as the count tested ptr (null: none; the launch covers its clouds + 1 entries).  What it finds goes up in
// `own_flag`: the count's flag stays as the count left it, a fill or a label afterwards still reads it.
__global__ void __launch_bounds__(kBlock)
    k_reader_check(double radius, const XY* __restrict__ queries, long long n_queries, long long row_rows, long long part_rows,
                   const long long* __restrict__ words, const int* __restrict__ flag, int* __restrict__ own_flag,
                   long long* __restrict__ counts, const long long* __restrict__ qptr, int clouds) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (qptr) pairs_ptr_check(qptr, nullptr, clouds, n_queries, i, own_flag, kReaderFlagBatch);
  if (i == 0) {
    counts[1] = *flag ? pairs_status(*flag) : 0;
    if (row_rows >= 0 || part_rows >= 0) {  // (no array of the caller's: n is not even read)
      const long long n = words[PW_N];
      if ((row_rows >= 0 && row_rows < (queries ? n_queries : n)) || (part_rows >= 0 && part_rows < n))
        atomicOr(own_flag, kReaderFlagRows);
    }
  }
  if (!queries || i >= n_queries) return;
  const XY q = queries[i];
  if (pairs_outside(fabs(q.x), radius) || pairs_outside(fabs(q.y), radius)) atomicOr(own_flag, kReaderFlagDomain);
}

}  // namespace sc
