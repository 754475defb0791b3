// The position gradient of the weighted neighbourhood sums on the device (sc_pairs_sum_grad_device): what torch's autograd
// needs to differentiate sc_pairs_sum_device through the coordinates of the points or of the queries.  The rule is
// specified in NumPy by tests/field_grad_spec.py (`position_grad`); the result is a pure function of its inputs, bit for
// bit.  Included once by sandcrate_hip.hip, after sc_fields.h.
//
// The other half of the gradient -- with respect to the values -- needs no kernel: w depends on d2 only and d2 is bitwise
// symmetric in its two points, so it is k_fields_sum with rows and partners swapped.
//
// The rule.  j is a partner of row r iff pairs_accept says so with `half` off, and in the self form j != r always
// (d2_rr is identically 0: its derivative is 0 whatever SC_FIELDS_SELF said in the forward).  With dx = qx - x[j],
// dy = qy - y[j] (pairs_accept's), t = 1 - d2 / r2 and m = 1, t, t t for power 1, 2, 3,
//     s  = ((((0 + row_s[r]) + part_s[j]) + row_a[r, 0] part_b[j, 0]) + row_a[r, 1] part_b[j, 1]) + ...
//     ax = ((0 + (s m) dx_j1) + (s m) dx_j2) + ...        ay likewise
//     grad[r] = (k ax, k ay),  k = -(2 power) / r2
// over the partners in ASCENDING j, every product and every sum rounded on its own (-ffp-contract=off); an absent
// row_s or part_s adds nothing.  Power 0 has no gradient: every row gets +0.0 and nothing walks.  A row whose own point
// is not finite walks nothing either and gets k * 0.
//
//   k_reader_check       (sc_pairs.h) prepares counts[1] and raises the readers' flag (which every reader zeroes before
//                        its own use, on the same stream): the domain bit for a query outside, the rows bit when the
//                        row arrays (row_a, row_s) have fewer rows than there are rows, or the partner arrays (part_b,
//                        part_s) fewer than the count has points (n is known on the device only);
//   k_fields_grad<C>     a thread per row, the nine-run merge of pairs_merge (sc_pairs.h) written out -- cursors in LDS,
//                        27 KiB at 256 rows, pairs_advance as the inner step --, its arguments loose and the PairsView
//                        put together inside.  Both on measurement: through pairs_merge with the view by value, and
//                        again with its own loop and the view by value (loops then instruction for instruction the
//                        old ones, only the argument loads of the prologue differ), the 1,248-row state at 8 channels
//                        and twice the diameter was MEASURED 2 to 5 % slower in three runs of three; this form compiles
//                        to the instructions it had before (profiles/readers_refactor.txt; why the prologue costs time
//                        where five workgroups hide no latency was not found).  The row's own row_a[r, 0 .. C) and row_s[r] are
//                        loaded once into registers, per partner part_b[j, 0 .. channels) is gathered where it lies
//                        (one run of at most 64 bytes) and
//                        part_s[j] likewise; two accumulators, one 16-byte store per row.  C is 1, 2, 4 or 8; a call
//                        with 3 channels runs C = 4, the loads guarded (a missing channel adds 0 * 0 = +0.0 to an s
//                        that is never -0.0: nothing changes).  Channels 0 runs C = 1 with nothing to load.
// No barrier, no scratch, no floating-point atomics, no atomic's order reaches the output (the flag is an OR), nothing of
// the workspace is written.  No j at or beyond part_rows and no row at or beyond row_rows is ever read: with fewer the
// flag is up and no thread walks.  With either flag up only counts[1] is written: -1 for the domain, else -2.
// On a batched grid the kernels are the `batched` instantiations, as in sc_fields.h: the row's record, query_ptr tested by
// the check, -3 for bad offsets, the same 27 KiB of LDS.
#pragma once
#include "sc_fields.h"

namespace sc {

struct FieldsGradIn {
  const double* row_a;   // rows x channels, or null (channels 0)
  const double* part_b;  // points x channels, or null (channels 0)
  const double* row_s;   // rows, or null
  const double* part_s;  // points, or null
};

// `queries` null: row i is point i of the count (n rows, n = words[PW_N]) and never its own partner; otherwise row i is
// queries[i] (n_queries rows).  `grad`: rows x 2, aligned to 16 bytes.
template <int C, bool batched>
__global__ void __launch_bounds__(kBlock)
    k_fields_grad(PairsGrid g, const long long* __restrict__ words, const int* __restrict__ flag,
                  const int* __restrict__ own_flag, const XY* __restrict__ xy, const XY* __restrict__ queries,
                  long long n_queries, int power, int channels, const int* __restrict__ start,
                  const XY* __restrict__ sxy, const uint2* __restrict__ scell, const int* __restrict__ sidx, FieldsGradIn in,
                  XY* __restrict__ grad, long long* __restrict__ counts, PairsBatch bt) {
  const PairsView v{g, words, flag, xy, start, sxy, scell, sidx, bt};  // (the view arrives unpacked: see above)
  __shared__ int s_cur[9][kBlock], s_end[9][kBlock], s_head[9][kBlock];
  const int tid = (int)threadIdx.x;
  const long long i = (long long)blockIdx.x * blockDim.x + tid;
  const int own = *own_flag;
  const bool up = *v.flag || own;
  const long long rows = queries ? n_queries : v.words[PW_N];
  if (i == 0) {
    if (up) counts[1] = reader_status(*v.flag, own);
    else counts[0] = rows;
  }
  if (up || i >= rows) return;  // (no barrier below: every thread is on its own)
  if (power == 0) {
    grad[i] = XY{0.0, 0.0};
    return;
  }
  double ax = 0.0, ay = 0.0;
  const XY p = queries ? queries[i] : v.xy[i];
  if (fabs(p.x) < __builtin_inf() && fabs(p.y) < __builtin_inf()) {
    double a[C];
#pragma unroll
    for (int c = 0; c < C; ++c) a[c] = c < channels ? in.row_a[i * channels + c] : 0.0;
    double s_row = 0.0;
    if (in.row_s) s_row += in.row_s[i];
    const int me = queries ? -1 : (int)i;  // (no j is -1)
    const PairsRow row = pairs_row<batched>(v.bt, i);
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
      const XY q = v.sxy[k];
      const double* src = in.part_b + (long long)best * channels;
      double val[C];  // (all loads first, then the sums: a load guarded next to its use waits for the one before)
#pragma unroll
      for (int c = 0; c < C; ++c) val[c] = c < channels ? src[c] : 0.0;
      double s = s_row;
      if (in.part_s) s += in.part_s[best];
      const double dx = p.x - q.x, dy = p.y - q.y;  // (pairs_accept's, which has said yes to this partner)
      const double d2 = dx * dx + dy * dy;
#pragma unroll
      for (int c = 0; c < C; ++c) s += a[c] * val[c];
      double sm = s;
      if (power > 1) {
        const double t = 1.0 - d2 / v.g.r2;
        sm = s * (power == 2 ? t : t * t);
      }
      ax += sm * dx;
      ay += sm * dy;
      const unsigned cx = cx0 + (unsigned)(bc % 3 - 1), cy = cy0 + (unsigned)(bc / 3 - 1);
      const int end = s_end[bc][tid];
      const int next = pairs_advance<batched>(v, row, me, p, cx, cy, k + 1, end);
      s_cur[bc][tid] = next;
      s_head[bc][tid] = next < end ? v.sidx[next] : INT_MAX;
    }
  }
  const double scale = -(2.0 * (double)power) / v.g.r2;
  grad[i] = XY{scale * ax, scale * ay};
}

}  // namespace sc
