// Nearest-k neighbour tables on the device (sc_pairs_nearest_device): for every row -- a point of the last count, or a
// query given beside it -- the k nearest partners within the radius as a table of fixed shape, rows x k, padded with -1
// (and +inf in the squared distances), and the uncapped number of partners per row.  The rule is specified in NumPy by
// tests/nearest_spec.py; the result is a pure function of the points and the queries.  Included once by
// sandcrate_hip.hip, after sc_pairs.h.
//
// Everything about the points is read from the workspace the last count left (sc_pairs.h): the points in index order, the
// hashed cell table, the members in bucket order with their positions and cells, n and the domain flag.  The caller's
// points are not read again, and nothing of the workspace is written: a fill, a label or another table may follow.
//   k_reader_check    (sc_pairs.h) clears the caller's cut counter (or writes the count's status there when its flag is
//                     up) and, query form, tests every query against the domain: one outside raises the flag OF THE
//                     READER -- the count's stays as the count left it, the fill and the label read it;
//   k_nearest<K>      a thread per row walks the buckets of its row's nine cells as k_pairs_count does -- the own-cell
//                     test, pairs_accept's arithmetic, `half` off, and j != i in the self form only (the walk is written
//                     out here: sc_pairs.h says why) -- and keeps its k best so far, ascending in the key (d2, j), then
//                     the workgroup writes its block of rows.
// The key.  d2 alone does not order a row: a lattice has four partners at bit-equal d2, a pile any number at 0.  The
// smaller j breaks the tie, so the table is the row of the full pair list, stably sorted by d2 and cut at k: a total order
// on the candidates, nothing left to the order in which they arrive.  Candidates arrive in bucket order -- the nine cells in
// raster order, several cells may share a bucket, a bucket ascends in j -- which has nothing to do with the key: the insert
// is a real insertion, from the end of the list towards its place.
//
// The list lives in LDS, slot-major: s_d2[slot][thread] and s_j[slot][thread], 12 bytes per place (a dynamically indexed
// register array would go to scratch, as k_pairs_fill notes).  The key of the list's last place is kept in registers: once
// the list is full a candidate that does not beat it costs one compare and no LDS access.  A workgroup is one wave of 64
// rows, and its LDS is sized by k in three steps -- 16, 32 or 64 places per row: 12, 24 and 49 KiB, so 12, 6 and 3 waves
// on a CU's 160 KiB.  (Wider workgroups at the same LDS per row -- 256 threads up to k = 16, 128 up to 32 -- hold as many
// waves on a CU and measured 2 % slower: profiles/nearest_time.txt.)  A slot's line is one entry longer than the workgroup
// (kNearestPad): in the write-out below consecutive lanes read consecutive SLOTS of one thread, which without the pad would
// all lie in one bank.
//
// The write-out.  The table is rows x k contiguous; a thread storing its own row would stride by 8 k bytes, 64 lines per
// wave store.  Instead the workgroup writes its block of rows -- 64 k consecutive entries -- together: entry e of the block
// is slot e % k of thread e / k.  That needs a barrier, so NO thread returns before it: a row past the row count, a dead
// row and a raised flag only skip the walk.  (Both flags are uniform over the launch.)
//
// counts[1], the number of rows with more partners than k: one integer add per such row, a count does not depend on their
// order.  With either flag up the kernel writes counts[1] = -1 and nothing else.
//
// On a batched grid (sc_pairs.h) the kernels are the `batched` instantiations: a row carries its record (lo, hi, cloud), a
// query finds its cloud by binary search over query_ptr, which k_reader_check tests as the count tested ptr; bad offsets
// give counts[1] = -3.  Rows of several clouds share a workgroup: the write-out does not care whose rows they are.
#pragma once
#include "sc_pairs.h"

namespace sc {

constexpr int kNearestMaxK = 64;
constexpr int kNearestPad = 1;
constexpr int kNearestBlock = 64;  // rows per workgroup: one wave
// the places per row a workgroup's LDS holds: the smallest of these that is at least k, then kNearestMaxK
// (sc_pairs_nearest_device chooses; mirrored by sand_crate_amd/_native.py: NEAREST_BLOCK, NEAREST_SLOTS)
constexpr int kNearestFewK = 16, kNearestMidK = 32;

struct NearestOut {
  long long* neighbors;  // rows x k
  double* d2;            // rows x k, or null
  long long* partners;   // rows, or null
  long long* counts;     // [2]: rows, cut
};

__device__ __forceinline__ bool nearest_before(double d2a, int ja, double d2b, int jb) {
  return d2a < d2b || (d2a == d2b && ja < jb);
}

// `queries` null: row i is point i of the count (n rows, n = words[PW_N]); otherwise row i is queries[i] (n_queries rows).
// The one reader whose kernel takes the PairsView unpacked: with the view by value its loops compiled to the same
// instructions and the table was still MEASURED 1.3 to 5.8 % slower in all seven cases of scripts/nearest_time.py; with
// the loose arguments it is inside the spread of the parent build (profiles/readers_refactor.txt; only the argument
// loads of the prologue differ, why that costs time was not found).
template <int K, bool batched>
__global__ void __launch_bounds__(kNearestBlock)
    k_nearest(PairsGrid g, const long long* __restrict__ words, const int* __restrict__ flag,
              const int* __restrict__ own_flag, const XY* __restrict__ xy, const XY* __restrict__ queries,
              long long n_queries, int k, const int* __restrict__ start, const XY* __restrict__ sxy,
              const uint2* __restrict__ scell, const int* __restrict__ sidx, NearestOut out, PairsBatch bt) {
  constexpr int W = kNearestBlock;
  __shared__ double s_d2[K][W + kNearestPad];
  __shared__ int s_j[K][W + kNearestPad];
  const int tid = (int)threadIdx.x;
  const long long base = (long long)blockIdx.x * W;
  const long long i = base + tid;
  const bool up = *flag || *own_flag;
  const long long rows = queries ? n_queries : words[PW_N];
  if (blockIdx.x == 0 && tid == 0) {
    if (up) out.counts[1] = reader_status(*flag, *own_flag);
    else out.counts[0] = rows;
  }
  int len = 0;  // places of the list in use
  if (!up && i < rows) {
    const XY p = queries ? queries[i] : xy[i];
    const int self = queries ? -1 : (int)i;  // (no j is -1)
    long long count = 0;
    if (fabs(p.x) < __builtin_inf() && fabs(p.y) < __builtin_inf()) {
      double worst_d2 = 0;
      int worst_j = 0;
      const PairsRow row = pairs_row<batched>(bt, i);
      const unsigned cx0 = pairs_cell(p.x, g.h), cy0 = pairs_cell(p.y, g.h);
      for (int c = 0; c < 9; ++c) {
        const unsigned cx = cx0 + (unsigned)(c % 3 - 1), cy = cy0 + (unsigned)(c / 3 - 1);
        const unsigned b = pairs_bucket(cx, cy, row.cloud, g.mask);
        const int end = start[b + 1];
        for (int s = start[b]; s < end; ++s) {
          const uint2 cell = scell[s];
          const int j = sidx[s];
          double d2;
          if (!(cell.x == cx && cell.y == cy && pairs_in<batched>(row, j) && pairs_accept(g, self, j, p, sxy[s], d2))) continue;
          ++count;
          int pos;
          if (len == k) {
            if (!nearest_before(d2, j, worst_d2, worst_j)) continue;
            pos = k - 1;  // the last place falls out
          } else {
            pos = len++;
          }
          for (; pos > 0; --pos) {
            const double pd = s_d2[pos - 1][tid];
            const int pj = s_j[pos - 1][tid];
            if (!nearest_before(d2, j, pd, pj)) break;
            s_d2[pos][tid] = pd;
            s_j[pos][tid] = pj;
          }
          s_d2[pos][tid] = d2;
          s_j[pos][tid] = j;
          if (len == k) {
            worst_d2 = s_d2[k - 1][tid];
            worst_j = s_j[k - 1][tid];
          }
        }
      }
    }
    if (out.partners) out.partners[i] = count;
    if (count > k) atomicAdd((unsigned long long*)&out.counts[1], 1ull);
  }
  for (int s = len; s < k; ++s) {
    s_d2[s][tid] = __builtin_inf();
    s_j[s][tid] = -1;
  }
  __syncthreads();
  if (up) return;
  const long long left = rows - base;  // the block's rows: min(W, left), none when left <= 0
  const int entries = (left >= W ? W : left > 0 ? (int)left : 0) * k;
  long long* nb = out.neighbors + base * k;
  double* db = out.d2 ? out.d2 + base * k : nullptr;
  for (int e = tid; e < entries; e += W) {
    const int t = e / k, s = e - t * k;
    nb[e] = s_j[s][t];
    if (db) db[e] = s_d2[s][t];
  }
}

}  // namespace sc
