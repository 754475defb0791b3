// Distance histograms on the device (sc_pairs_hist_device): for every row -- a point of the last count, or a query given
// beside it -- how many partners lie in each of B distance bands, and the same counts summed over the rows: the table of
// shell counts a learned simulator reads next to the neighbour table, and the numerator of the radial distribution
// function g(r).  The rule is specified in NumPy by tests/hist_spec.py; the result is a pure function of the points, the
// queries and the edges.  Included once by sandcrate_hip.hip, after sc_fields_grad.h.
//
// The rule.  e2[0 .. B] are the SQUARED edges, strictly ascending, squared once on the host; no square root is taken
// anywhere.  j is a partner of row r iff pairs_accept says so with `half` off and r2 = e2[B] -- the arithmetic of the pair
// list, d2 = fl(fl(dx dx) + fl(dy dy)) -- and j != r in the self form.  A partner is in bin b iff e2[b] <= d2 < e2[b + 1],
// the last bin closed on top (d2 <= e2[B] is the acceptance itself); one with d2 < e2[0] is in no bin.
//
// Why the walk and not the merge.  The readers that add floating-point numbers (sc_fields.h) or store a list
// (k_pairs_fill) merge a row's nine runs into ascending j, because the walk's own order depends on the table's size.  A
// histogram is integer counts: the order in which a row's partners are met cannot reach it.  So the walk is that of
// k_pairs_count -- the nine cells in raster order, the own-cell test, pairs_accept -- with no cursors, written out here
// (sc_pairs.h says why it is not one function).
//
// Everything about the points is read from the workspace the last count left (sc_pairs.h), and nothing of it is written:
// a fill, a label, a table, a sum or another histogram may follow.
//   k_reader_check (sc_pairs.h) prepares counts[1] and raises the flag OF THE HISTOGRAM for a query outside the domain (the
//                  count's stays as the count left it).  The flag and the accumulator of the totals were zeroed on the
//                  stream before, by one memset: the flag is the word behind the accumulator, not the other readers';
//   k_hist<NB>     a thread per row walks, places every accepted d2 by a binary search over e2 in LDS and adds one to
//                  its own counter; then the workgroup writes its block of rows of the table together and adds its
//                  column sums to the accumulator;
//   k_hist_finish  copies the accumulator to the caller's totals -- unless a flag is up: with a status below 0 only
//                  counts[1] is written, so the totals cannot be accumulated in the caller's array, which would have to
//                  be zeroed before the flag is known.
// The LDS.  The search array: s_e2[0] = e2[0], s_e2[k] = e2[k] for k < B and +inf from B on (the top edge is the
// acceptance's r2 and takes no part), NB entries, so the search is log2(NB) steps of "is the edge `step` further still
// at most d2", each an exact compare, without a branch.  The counters: int32, slot-major, s_bins[b][lane] -- each lane
// owns its column, so no LDS atomics; a dynamically indexed register array would go to scratch (k_pairs_fill).  A line is
// one entry longer than the workgroup (kHistPad): in the write-out and in the column sums consecutive lanes read
// consecutive BINS of one row, which without the pad would all lie in one bank.  A workgroup is one wave of 64 rows, as
// k_nearest's.  The search is made for B in three steps -- NB = 16, 32 or 64: four, five or six compares per partner --
// but the counters take kHistLines = 64 lines, 16.8 KiB, in all three: sized by NB (4.2 and 8.4 KiB, 32 and 19 waves on a
// CU instead of 9) the walk of 1,048,576 rows in random index order was MEASURED 1.9 and 2.2 x slower for 16 bins (1,777
// against 947 us at the diameter, 6,460 against 2,975 us at twice the diameter), and 128 lines (4 waves) 1.5 x slower:
// every lane of a wave reads its own cache lines, and more rows in flight than about nine waves a CU evict each
// other's (profiles/hist_time.txt).  The LDS is what holds the occupancy there; the lines beyond B are not touched.
// The table.  rows x B contiguous int32; the workgroup writes its block -- 64 B consecutive entries -- together: entry e
// is bin e % B of row e / B.  That needs a barrier, so NO thread returns before it: a row past the row count, a dead row
// and a raised flag only skip the walk.  (Both flags are uniform over the launch.)
// The totals.  Lane b adds up bin b over the workgroup's 64 rows in 64 bits (64 rows of up to 2^28 partners do not fit
// 32) and issues one 64-bit integer atomicAdd when the sum is not zero.  Integer adds commute: no atomic's order reaches
// the output.  No floating-point atomics, no workgroup waits for another, no workspace beyond the flag and the 64 words.
//
// The batched form (sc_pairs_hist_batch_device, on the grid of a count after sc_pairs_set_batch_device; the rule is
// tests/batch_readers_spec.py): k_hist<NB, true>.  The row reads its record (lo, hi, cloud) once -- pairs_row,
// sc_pairs.h: a point's from the workspace, a query's by binary search over query_ptr --, hashes its nine cells with its
// cloud and counts a candidate only when pairs_in says its index lies in the cloud.  The table is as before.  The totals
// are per cloud, clouds x bins words in the context's accumulator: a workgroup's 64 rows may hold several clouds, but rows
// ascend, so clouds ascend -- every row leaves its cloud in LDS (64 ints more, in this instantiation only), and lane b
// sums bin b over each run of equal cloud and issues one 64-bit integer atomicAdd per non-zero (run, bin).  The counters
// still take kHistLines lines whatever the clouds: the occupancy argument above is the walk's and has not changed.
// k_hist_finish copies clouds x bins words, and only with no flag up.  The unbatched instantiation carries no record and
// no s_cloud.
#pragma once
#include "sc_pairs.h"

namespace sc {

constexpr int kHistMaxBins = 64;
constexpr int kHistPad = 1;
constexpr int kHistBlock = 64;  // rows per workgroup: one wave
// the bins a kernel's search is made for: the smallest of these that is at least B, then kHistMaxBins
// (sc_pairs_hist_device chooses; mirrored by sand_crate_amd/_native.py: HIST_BLOCK, HIST_SLOTS)
constexpr int kHistFewBins = 16, kHistMidBins = 32;
constexpr int kHistLines = kHistMaxBins;  // lines of counters in every workgroup's LDS (measured: see above)

struct HistEdges {
  double e2[kHistMaxBins + 1];  // e2[0 .. bins]
};

struct HistOut {
  int* table;         // rows x bins, or null
  long long* total;   // bins -- batched: clouds x bins --, or null
  long long* counts;  // [2]: rows, status
};

// `queries` null: row i is point i of the count (n rows, n = words[PW_N]); otherwise row i is queries[i] (n_queries rows).
// v.g.r2 is e2[bins], at most the count's; v.g.h and v.g.mask are the count's.  `batched`: `acc` holds clouds x bins words.
template <int NB, bool batched>
__global__ void __launch_bounds__(kHistBlock)
    k_hist(PairsView v, HistEdges edges, int bins, const int* __restrict__ own_flag, const XY* __restrict__ queries,
           long long n_queries, long long* __restrict__ acc, HistOut out) {
  constexpr int W = kHistBlock;
  static_assert(NB <= W, "lane b loads edge b and sums bin b");
  __shared__ double s_e2[NB];
  static_assert(NB <= kHistLines, "a line of counters per bin");
  __shared__ int s_bins[kHistLines][W + kHistPad];
  __shared__ int s_cloud[batched ? W : 1];  // the cloud of every row of the workgroup (batched only)
  const int tid = (int)threadIdx.x;
  const long long base = (long long)blockIdx.x * W;
  const long long i = base + tid;
  const bool up = *v.flag || *own_flag;
  const long long rows = queries ? n_queries : v.words[PW_N];
  if (blockIdx.x == 0 && tid == 0) {
    if (up) out.counts[1] = reader_status(*v.flag, *own_flag);
    else out.counts[0] = rows;
  }
  if (up) return;  // (uniform over the launch: nobody is left at the barriers below)
  if (tid < NB) s_e2[tid] = tid < bins ? edges.e2[tid] : __builtin_inf();
  for (int b = 0; b < bins; ++b) s_bins[b][tid] = 0;
  __syncthreads();
  if (i < rows) {
    const XY p = queries ? queries[i] : v.xy[i];
    const PairsRow row = pairs_row<batched>(v.bt, i);  // (a dead row has a cloud too: its zeros are credited there)
    if (batched) s_cloud[tid] = (int)row.cloud;
    if (fabs(p.x) < __builtin_inf() && fabs(p.y) < __builtin_inf()) {
      const int me = queries ? -1 : (int)i;  // (no j is -1)
      const double first = s_e2[0];
      const unsigned cx0 = pairs_cell(p.x, v.g.h), cy0 = pairs_cell(p.y, v.g.h);
      for (int c = 0; c < 9; ++c) {
        const unsigned cx = cx0 + (unsigned)(c % 3 - 1), cy = cy0 + (unsigned)(c / 3 - 1);
        const unsigned bk = pairs_bucket(cx, cy, row.cloud, v.g.mask);
        const int end = v.start[bk + 1];
        for (int k = v.start[bk]; k < end; ++k) {
          const uint2 cell = v.scell[k];
          double d2;
          if (!(cell.x == cx && cell.y == cy && pairs_in<batched>(row, v.sidx[k]) &&
                pairs_accept(v.g, me, v.sidx[k], p, v.sxy[k], d2)))
            continue;
          if (d2 < first) continue;  // below the first edge: in no bin
          int b = 0;                 // the last edge among 1 .. bins - 1 that is at most d2
#pragma unroll
          for (int step = NB / 2; step >= 1; step /= 2)
            if (s_e2[b + step] <= d2) b += step;
          s_bins[b][tid] += 1;
        }
      }
    }
  }
  __syncthreads();
  const long long left = rows - base;  // the block's rows: min(W, left), none when left <= 0
  const int mine = left >= W ? W : left > 0 ? (int)left : 0;
  if (out.table) {
    const int entries = mine * bins;
    int* tb = out.table + base * bins;
    for (int e = tid; e < entries; e += W) {
      const int t = e / bins, b = e - t * bins;
      tb[e] = s_bins[b][t];
    }
  }
  if (out.total && tid < bins) {
    long long sum = 0;
    if (batched) {
      // the rows ascend, so their clouds ascend: one add per run of equal cloud, into that cloud's line
      int cur = mine > 0 ? s_cloud[0] : 0;
      for (int t = 0; t < mine; ++t) {
        const int cl = s_cloud[t];
        if (cl != cur) {
          if (sum) atomicAdd((unsigned long long*)&acc[(long long)cur * bins + tid], (unsigned long long)sum);
          sum = 0;
          cur = cl;
        }
        sum += s_bins[tid][t];
      }
      if (sum) atomicAdd((unsigned long long*)&acc[(long long)cur * bins + tid], (unsigned long long)sum);
    } else {
      for (int t = 0; t < mine; ++t) sum += s_bins[tid][t];
      if (sum) atomicAdd((unsigned long long*)&acc[tid], (unsigned long long)sum);
    }
  }
}

// After k_hist on the same stream: the `cells` totals -- bins, batched clouds x bins -- go to the caller unless a flag is up.
__global__ void __launch_bounds__(kHistBlock)
    k_hist_finish(long long cells, const int* __restrict__ flag, const int* __restrict__ own_flag,
                  const long long* __restrict__ acc, long long* __restrict__ total) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (*flag || *own_flag || b >= cells) return;
  total[b] = acc[b];
}

}  // namespace sc
