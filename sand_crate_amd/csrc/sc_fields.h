// Weighted neighbourhood sums on the device (sc_pairs_sum_device): for every row -- a point of the last count, or a query
// given beside it -- the sum over its partners within the radius of w(d2) * values[j, :], and the sum of the weights: an
// SPH interpolation, the density at a particle or a probe, the "sum over neighbours" of a message-passing layer.  The
// rule is specified in NumPy by tests/field_spec.py; the result is a pure function of the points, the queries and the
// values, bit for bit.  Included once by sandcrate_hip.hip, after sc_nearest.h.
//
// The rule.  j is a partner of row r iff pairs_accept says so with `half` off -- and j != r in the self form without
// SC_FIELDS_SELF.  t = 1 - d2 / r2 (one division, one subtraction), w = 1, t, t t or (t t) t for power 0 .. 3, and
//     wsum[r] = ((0 + w_j1) + w_j2) + ...     out[r, c] = ((0 + w_j1 v[j1, c]) + w_j2 v[j2, c]) + ...
// over the partners in ASCENDING j, every product and every sum rounded on its own (-ffp-contract=off).  Why ascending j
// and not the order of the walk: the walk meets a row's partners in bucket order -- the nine cells in raster order, a cell's
// bucket by the hash -- which depends on the table's size and so on the BOUND the count was sized by, not on the points
// alone; a float64 sum in that order would change in its last bits with the crate's capacity.  Ascending j is the order
// of the pair list's row, which NumPy restates with a loop.
//
// Everything about the points is read from the workspace the last count left (sc_pairs.h), as sc_nearest.h does, and
// nothing of it is written: a fill, a label, a table or another sum may follow.
//   k_reader_check  (sc_pairs.h) prepares counts[1] and raises the flag OF THE READER (the count's stays as the count left
//                   it): the domain bit for a query outside, the rows bit when the caller's values have fewer rows than
//                   the count has points (n is known on the device only);
//   k_fields_sum<C> a thread per row takes its partners from pairs_merge (sc_pairs.h), the merge k_pairs_fill stores its
//                   list from -- the cursors in the kernel's LDS (s_cur / s_end / s_head) -- and instead of storing the
//                   partner adds to wsum and to C channel sums in registers; the loops over the channels are unrolled.
//                   C is 1, 2, 4 or 8: a call with 3 channels runs C = 4, the loads and the stores guarded.
// The values are gathered by j from the caller's array as they are: values[j, 0 .. channels) is one run of at most 64
// bytes.  Copying them into bucket order first, next to the sxy[s] the walk reads (16-byte loads at a fixed stride), was
// built and measured and is 2 to 4 % SLOWER at 1,048,576 points in random index order and 10 % slower for 65,536 probes:
// the copy costs more than the gather saves (profiles/fields_time.txt).  No j at or beyond values_rows is ever read:
// the walk yields j < n only, and with values_rows < n the flag is up and no thread walks.
// A thread stores its own row: channels * 8 contiguous bytes, at most 64, rows x channels in all -- small beside what the
// walk reads; a write-out through LDS as in k_nearest was not built.  No barrier, so a thread with nothing to do returns.
// No floating-point atomics, no atomic's order reaches the output (the flag is an OR), no workgroup waits for another.
// With either flag up only counts[1] is written: -1 for the domain (the count's flag or a query), else -2 for the values.
//
// On a batched grid (sc_pairs.h) the kernels are the `batched` instantiations: a row carries its record (lo, hi, cloud), a
// query finds its cloud by binary search over query_ptr, which k_reader_check tests as the count tested ptr (the batch bit
// of the reader's flag); bad offsets, the count's or the queries', give counts[1] = -3 before anything else.  No LDS is
// added.
#pragma once
#include "sc_pairs.h"

namespace sc {

constexpr int kFieldsMaxChannels = 8;

struct FieldsOut {
  double* sums;       // rows x channels, or null (channels 0)
  double* wsum;       // rows, or null
  long long* counts;  // [2]: rows, status
};

// 1 - d2 / r2 to the power: 1, t, t t, (t t) t.  Power 0 computes no division.
__device__ __forceinline__ double fields_weight(int power, double d2, double r2) {
  if (power == 0) return 1.0;
  const double t = 1.0 - d2 / r2;
  if (power == 1) return t;
  const double tt = t * t;
  return power == 2 ? tt : tt * t;
}

// `queries` null: row i is point i of the count (n rows, n = words[PW_N]); otherwise row i is queries[i] (n_queries rows).
// `self`: 1 when a point is a partner of its own row (always so for a query that lies on a point).  `values` null: the
// weight sums only.
template <int C, bool batched>
__global__ void __launch_bounds__(kBlock)
    k_fields_sum(PairsView v, const int* __restrict__ own_flag, const XY* __restrict__ queries, long long n_queries, int self,
                 int power, int channels, const double* __restrict__ values, FieldsOut out) {
  __shared__ int s_cur[9][kBlock], s_end[9][kBlock], s_head[9][kBlock];
  const int tid = (int)threadIdx.x;
  const long long i = (long long)blockIdx.x * blockDim.x + tid;
  const int own = *own_flag;
  const bool up = *v.flag || own;
  const long long rows = queries ? n_queries : v.words[PW_N];
  if (i == 0) {
    if (up) out.counts[1] = reader_status(*v.flag, own);
    else out.counts[0] = rows;
  }
  if (up || i >= rows) return;  // (no barrier below: every thread is on its own)
  double wsum = 0.0;
  double acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0;
  const XY p = queries ? queries[i] : v.xy[i];
  if (fabs(p.x) < __builtin_inf() && fabs(p.y) < __builtin_inf()) {
    const int me = queries || self ? -1 : (int)i;  // (no j is -1)
    pairs_merge<batched>(v, pairs_row<batched>(v.bt, i), me, p, s_cur, s_end, s_head, tid, [&](int j, XY q) {
      double d2;
      (void)pairs_accept(v.g, me, j, p, q, d2);
      const double w = fields_weight(power, d2, v.g.r2);
      wsum += w;
      if (values) {
        const double* src = values + (long long)j * channels;
        double val[C];  // (all loads first, then the sums: a load guarded next to its use waits for the one before)
#pragma unroll
        for (int c = 0; c < C; ++c) val[c] = c < channels ? src[c] : 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += w * val[c];
      }
      return true;
    });
  }
  if (out.wsum) out.wsum[i] = wsum;
  if (out.sums) {
    double* row = out.sums + i * channels;
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (c < channels) row[c] = acc[c];
  }
}

}  // namespace sc
