// Host side of the state in the caller's device memory: export and import, pair lists, clusters, nearest-k tables,
// weighted neighbourhood sums with their position gradient, distance histograms, and ray sensors.
#pragma once
#include "sc_host.h"
#include "sc_state.h"
#include "sc_pairs.h"
#include "sc_clusters.h"
#include "sc_cluster_sums.h"
#include "sc_nearest.h"
#include "sc_fields.h"
#include "sc_fields_grad.h"
#include "sc_hist.h"
#include "sc_rays.h"

extern "C" {

// ---- the state in the caller's device memory (sc_state.h) ---------------------------------------

// Ranks the m slots of the launch by id into set *set of state.sort: slots that are not stored, or whose x is not finite,
// carry kStateDead and come last.
static int state_rank(sc_ctx* c, int64_t m, int* set) {
  if (const int rc = c->state.sort.ensure(m, c->stream)) return rc;
  return radix_sort(c, c->state.sort, StateKey{c->counters, c->x, c->id[0], (int)c->cap}, m, kStatePasses, set);
}

int sc_export_state_device(sc_ctx* c, double* dev_xy, double* dev_vxy, double* dev_pressure, int64_t* dev_ids, int64_t room,
                           int64_t* dev_n) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_n) return fail(SC_ERR_ARG, "null count pointer");
  if (room < 0) return fail(SC_ERR_ARG, "negative room");
  if (((uintptr_t)dev_xy | (uintptr_t)dev_vxy) & 15) return fail(SC_ERR_ARG, "xy and vxy must be aligned to 16 bytes");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_export_state_device inside a tick");
  const int64_t m = slot_bound(c);
  if (room < m)
    return fail(SC_ERR_CAPACITY, "device arrays hold %lld, up to %lld particles stored", (long long)room, (long long)m);
  HIPCHK(hipSetDevice(c->device));
  int set;
  if (const int rc = state_rank(c, m, &set)) return rc;
  const StateOut o{dev_xy, dev_vxy, dev_pressure, (long long*)dev_ids, (long long*)dev_n};
  hipLaunchKernelGGL(k_state_gather, dim3(grid_for(m)), dim3(kBlock), 0, c->stream, c->counters, o,
                     c->state.sort.keys[set].get(), c->state.sort.vals[set].get(), (int)m, (int)c->cap,
                     c->normals_valid ? 1 : 0, c->x.get(), c->y.get(), c->vx.get(), c->vy.get(), c->P.get());
  HIPCHK(hipGetLastError());
  return SC_OK;
}

int sc_import_state_device(sc_ctx* c, const double* dev_xy, const double* dev_vxy, const int64_t* dev_ids, int64_t n) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  int rc = put_check(c, dev_xy, dev_vxy, n, true);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  int* ids32 = nullptr;
  int64_t max_id = -1;
  if (dev_ids && n > 0) {
    HIPCHK(c->state.words.grow(2, c->stream));
    HIPCHK(c->state.ids.grow(n, c->stream));
    HIPCHK(hipMemsetAsync(c->state.words, 0, 2 * sizeof(int), c->stream));
    hipLaunchKernelGGL(k_state_check_ids, dim3(grid_for(n)), dim3(kBlock), 0, c->stream, (const long long*)dev_ids, (int)n,
                       c->state.ids.get(), c->state.words.get());
    HIPCHK(hipGetLastError());
    int words[2] = {0, 0};
    if ((rc = read_back(c, words, c->state.words, sizeof words))) return rc;
    if (words[1]) return fail(SC_ERR_ARG, "particle id out of range");
    ids32 = c->state.ids;
    max_id = (int64_t)words[0] - 1;
  }
  return put_from_device(c, dev_xy, dev_vxy, ids32, max_id, n, true);
}

// ---- pair lists (sc_pairs.h) --------------------------------------------------------------------

constexpr int64_t kPairsMaxPoints = (int64_t)1 << 28;

static unsigned pairs_buckets(int64_t m) {
  unsigned t = kPairsMinBuckets;
  while ((int64_t)t < kPairsLoad * m) t <<= 1;
  return t;
}

int sc_pairs_set_batch_device(sc_ctx* c, const int64_t* dev_ptr, int64_t clouds) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (clouds < 0) return fail(SC_ERR_ARG, "negative number of clouds");
  if (clouds > kPairsMaxPoints) return fail(SC_ERR_CAPACITY, "%lld clouds, at most %lld", (long long)clouds, (long long)kPairsMaxPoints);
  const bool set = dev_ptr && clouds > 0;
  c->pairs.next_ptr = set ? dev_ptr : nullptr;
  c->pairs.next_clouds = set ? clouds : 0;
  return SC_OK;
}

int sc_pairs_set_query_batch_device(sc_ctx* c, const int64_t* dev_query_ptr) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!c->pairs.valid || !c->pairs.clouds)
    return fail(SC_ERR_ARG, "query offsets without a batched grid: sc_pairs_set_batch_device and sc_pairs_count_device come first");
  c->pairs.next_qptr = dev_query_ptr;  // (null clears)
  return SC_OK;
}

// The clusters, the histograms, the rays and the ray paths come in two calls each, `who` and `twin`, which share a host
// body: the unbatched one refuses a batched grid and the batched one an unbatched grid, each naming the other.
static int pairs_grid_is(sc_ctx* c, bool batched, const char* who, const char* twin) {
  if ((c->pairs.clouds != 0) == batched) return SC_OK;
  if (batched)
    return fail(SC_ERR_ARG, "%s reads a batched grid only: sc_pairs_set_batch_device and a count come first, or call %s", who, twin);
  return fail(SC_ERR_ARG, "%s does not read a batched grid: call %s, or count without sc_pairs_set_batch_device first", who, twin);
}

int sc_pairs_count_device(sc_ctx* c, const double* dev_xy, int64_t n, double radius, int32_t flags, int64_t* dev_offsets,
                          int64_t room_rows, int64_t* dev_counts) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  const int64_t* batch_ptr = c->pairs.next_ptr;  // consumed here, whatever becomes of the call
  const int64_t clouds = c->pairs.next_clouds;
  c->pairs.next_ptr = nullptr;
  c->pairs.next_clouds = 0;
  c->pairs.next_qptr = nullptr;
  if (clouds && !dev_xy) return fail(SC_ERR_ARG, "a batch needs the caller's points: the state is one cloud");
  if (!dev_offsets || !dev_counts) return fail(SC_ERR_ARG, "null offsets or counts pointer");
  if (room_rows < 0) return fail(SC_ERR_ARG, "negative room");
  if (flags & ~SC_PAIRS_HALF) return fail(SC_ERR_ARG, "unknown flags %d", flags);
  const double r2 = radius * radius;
  if (!(radius > 0) || !std::isfinite(radius) || !std::isfinite(r2) || r2 < std::numeric_limits<double>::min())
    return fail(SC_ERR_ARG, "the radius must be finite and positive, and so must its square (about 1.5e-154 .. 1.3e154)");
  if (dev_xy && n < 0) return fail(SC_ERR_ARG, "negative point count");
  if ((uintptr_t)dev_xy & 15) return fail(SC_ERR_ARG, "the points must be aligned to 16 bytes");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_pairs_count_device inside a tick");
  if (!dev_xy && c->slab)
    return fail(SC_ERR_STATE, "the pairs of the state are not available in slab mode: partners across a cut live on another rank");
  const int64_t m = dev_xy ? n : slot_bound(c);
  if (m > kPairsMaxPoints) return fail(SC_ERR_CAPACITY, "%lld points, at most %lld", (long long)m, (long long)kPairsMaxPoints);
  if (room_rows < m)
    return fail(SC_ERR_CAPACITY, "offsets hold %lld rows, up to %lld points", (long long)room_rows, (long long)m);
  HIPCHK(hipSetDevice(c->device));
  c->pairs.valid = false;
  c->pairs.clouds = 0;
  c->clusters.valid = false;  // (a label belongs to the count it was made from)
  const unsigned buckets = pairs_buckets(m);
  int rc = c->pairs.ensure(m, buckets, c->stream);
  if (rc) return rc;
  if (clouds) {
    HIPCHK(c->pairs.ptr.grow(clouds + 1, c->stream));
    HIPCHK(c->pairs.cloud.grow(m, c->stream));
  }
  PairsGrid g{};
  g.radius = radius;
  g.h = radius * kPairsCellFactor;
  g.r2 = r2;
  g.mask = buckets - 1;
  g.half = (flags & SC_PAIRS_HALF) ? 1 : 0;
  const int grid = grid_for(m);
  if (!dev_xy) {
    int set;
    if ((rc = state_rank(c, m, &set))) return rc;
    hipLaunchKernelGGL(k_pairs_gather, dim3(grid), dim3(kBlock), 0, c->stream, c->state.sort.keys[set].get(),
                       c->state.sort.vals[set].get(), (int)m, c->x.get(), c->y.get(), c->pairs.xy.get(), c->pairs.words.get());
  }
  HIPCHK(hipMemsetAsync(c->pairs.flag, 0, sizeof(int), c->stream));
  HIPCHK(hipMemsetAsync(c->pairs.bucketCount, 0, (size_t)buckets * sizeof(int), c->stream));
  RadixSpace& w = c->pairs.sort;
  c->pairs.clouds = clouds;
  c->pairs.grid = g;
  if (clouds)
    hipLaunchKernelGGL(k_pairs_batch_check, dim3(grid_for(clouds + 1)), dim3(kBlock), 0, c->stream, (const long long*)batch_ptr,
                       c->pairs.ptr.get(), (int)clouds, (long long)n, c->pairs.flag.get());
  hipLaunchKernelGGL(clouds ? k_pairs_key<true> : k_pairs_key<false>, dim3(grid), dim3(kBlock), 0, c->stream, g,
                     dev_xy ? (const XY*)dev_xy : c->pairs.xy.get(), c->pairs.xy.get(), dev_xy ? (long long)n : -1LL,
                     c->pairs.words.get(), (int)m, w.keys[0].get(), w.vals[0].get(), c->pairs.bucketCount.get(),
                     c->pairs.flag.get(), c->pairs.ptr.get(), (int)clouds, c->pairs.cloud.get());
  // the binning sort: the keys are 0 .. buckets (a dead point's), so as many digits as `buckets` has
  int bits = 1;
  while ((buckets >> bits) != 0) ++bits;
  int in;
  if ((rc = radix_sort(c, w, RadixStored{}, m, (bits + kRadixDigitBits - 1) / kRadixDigitBits, &in))) return rc;
  c->pairs.set = in;
  if ((rc = launch_scan(c, c->pairs.bucketCount, c->pairs.bucketStart, buckets, c->pairs.bucketSums, nullptr))) return rc;
  hipLaunchKernelGGL(k_pairs_place, dim3(grid), dim3(kBlock), 0, c->stream, g, w.keys[in].get(), w.vals[in].get(), (int)m,
                     c->pairs.xy.get(), c->pairs.flag.get(), c->pairs.sxy.get(), c->pairs.cell.get());
  hipLaunchKernelGGL(clouds ? k_pairs_count<true> : k_pairs_count<false>, dim3(grid), dim3(kBlock), 0, c->stream,
                     c->pairs.view_of_count(), (int)m, c->pairs.rowLen.get());
  const int nb = (int)(m / kScanPerBlock + 1);  // entry n <= m lies in one of them
  hipLaunchKernelGGL(k_scan64_local, dim3(nb), dim3(kBlock), 0, c->stream, c->pairs.rowLen.get(), c->pairs.offs.get(),
                     c->pairs.words.get(), c->pairs.flag.get(), c->pairs.sums.get());
  hipLaunchKernelGGL(k_scan64_fix, dim3(nb), dim3(kBlock), 0, c->stream, c->pairs.offs.get(), (long long*)dev_offsets,
                     c->pairs.words.get(), c->pairs.flag.get(), c->pairs.sums.get(), (long long*)dev_counts);
  HIPCHK(hipGetLastError());
  c->pairs.valid = true;
  c->pairs.m = m;
  return SC_OK;
}

int sc_pairs_fill_device(sc_ctx* c, int64_t* dev_partners, double* dev_d2, int64_t room_pairs) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (room_pairs < 0) return fail(SC_ERR_ARG, "negative room");
  if (!dev_partners && room_pairs > 0) return fail(SC_ERR_ARG, "null partners pointer");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_pairs_fill_device inside a tick");
  if (!c->pairs.valid)
    return fail(SC_ERR_STATE, "no pair count to fill from: sc_pairs_count_device comes first, and the state must not change in between");
  HIPCHK(hipSetDevice(c->device));
  const int64_t m = c->pairs.m;
  if (room_pairs == 0) return SC_OK;
  hipLaunchKernelGGL(c->pairs.clouds ? k_pairs_fill<true> : k_pairs_fill<false>, dim3(grid_for(m)), dim3(kBlock), 0, c->stream,
                     c->pairs.view_of_count(), (int)m, c->pairs.offs.get(), (long long*)dev_partners, dev_d2,
                     (long long)room_pairs);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

// ---- clusters (sc_clusters.h) --------------------------------------------------------------------

// sc_pairs_label_device and sc_pairs_label_batch_device: `batched` says which, and `dev_cluster_ptr` is the second one's.
static int pairs_label(sc_ctx* c, bool batched, int64_t* dev_labels, int64_t room_rows, int64_t* dev_sizes, int64_t* dev_roots,
                       int64_t room_clusters, int64_t* dev_cluster_ptr, int64_t* dev_counts) {
  const char* who = batched ? "sc_pairs_label_batch_device" : "sc_pairs_label_device";
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_labels || !dev_counts) return fail(SC_ERR_ARG, "null labels or counts pointer");
  if (batched && !dev_cluster_ptr) return fail(SC_ERR_ARG, "null cluster_ptr pointer");
  if (room_rows < 0 || room_clusters < 0) return fail(SC_ERR_ARG, "negative room");
  if (c->in_step) return fail(SC_ERR_STATE, "%s inside a tick", who);
  if (!c->pairs.valid)
    return fail(SC_ERR_STATE, "no pair count to label from: sc_pairs_count_device comes first, and the state must not change in between");
  if (const int rc = pairs_grid_is(c, batched, who, batched ? "sc_pairs_label_device" : "sc_pairs_label_batch_device")) return rc;
  const int64_t m = c->pairs.m;
  if (room_rows < m)
    return fail(SC_ERR_CAPACITY, "labels hold %lld rows, up to %lld points", (long long)room_rows, (long long)m);
  HIPCHK(hipSetDevice(c->device));
  int rc = c->clusters.ensure(m, c->stream);
  if (rc) return rc;
  const int grid = grid_for(m);
  const long long* words = c->pairs.words.get();
  const int* flag = c->pairs.flag.get();
  int* parent = c->clusters.parent.get();
  hipLaunchKernelGGL(k_cluster_init, dim3(grid), dim3(kBlock), 0, c->stream, words, flag, (int)m, parent);
  // (the view's `half` is off: the components are those of the full graph, whichever form the count had)
  hipLaunchKernelGGL(batched ? k_cluster_union<true> : k_cluster_union<false>, dim3(grid), dim3(kBlock), 0, c->stream,
                     c->pairs.view(nullptr), (int)m, parent);
  // a tree of at most m nodes is at most m - 1 deep, and a round halves (rounding up) every depth
  int rounds = 1;
  while (((int64_t)1 << rounds) < m) ++rounds;
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(k_cluster_jump, dim3(grid), dim3(kBlock), 0, c->stream, words, flag, (int)m, parent);
  hipLaunchKernelGGL(k_cluster_mark, dim3(grid), dim3(kBlock), 0, c->stream, words, flag, (int)m, c->pairs.xy.get(), parent,
                     c->clusters.isRoot.get(), c->clusters.size.get());
  if ((rc = launch_scan(c, c->clusters.isRoot, c->clusters.dense, m, c->clusters.sums, nullptr))) return rc;
  hipLaunchKernelGGL(k_cluster_write, dim3(grid), dim3(kBlock), 0, c->stream, words, flag, (int)m, c->pairs.xy.get(), parent,
                     c->clusters.dense.get(), c->clusters.size.get(), (long long*)dev_labels, (long long*)dev_roots,
                     (long long)room_clusters);
  hipLaunchKernelGGL(k_cluster_finish, dim3(grid), dim3(kBlock), 0, c->stream, words, flag, (int)m, c->clusters.dense.get(),
                     c->clusters.size.get(), (long long*)dev_sizes, (long long)room_clusters, (long long*)dev_counts);
  if (batched)
    hipLaunchKernelGGL(k_cluster_ptr, dim3(grid_for(c->pairs.clouds + 1)), dim3(kBlock), 0, c->stream, flag, c->pairs.ptr.get(),
                       (int)c->pairs.clouds, c->clusters.dense.get(), (long long*)dev_cluster_ptr);
  HIPCHK(hipGetLastError());
  c->clusters.valid = true;
  c->clusters.m = m;
  return SC_OK;
}

int sc_pairs_label_device(sc_ctx* c, int64_t* dev_labels, int64_t room_rows, int64_t* dev_sizes, int64_t* dev_roots,
                          int64_t room_clusters, int64_t* dev_counts) {
  return pairs_label(c, false, dev_labels, room_rows, dev_sizes, dev_roots, room_clusters, nullptr, dev_counts);
}

int sc_pairs_label_batch_device(sc_ctx* c, int64_t* dev_labels, int64_t room_rows, int64_t* dev_sizes, int64_t* dev_roots,
                                int64_t room_clusters, int64_t* dev_cluster_ptr, int64_t* dev_counts) {
  return pairs_label(c, true, dev_labels, room_rows, dev_sizes, dev_roots, room_clusters, dev_cluster_ptr, dev_counts);
}

}  // extern "C"

// ---- per-cluster sums and extents (sc_cluster_sums.h) ----------------------------------------------

template <int C>
static void csum_launch(sc_ctx* c, bool first, int grid, const CsumGuard& g, const CsumLevel& lv, const CsumIo& io) {
  hipLaunchKernelGGL((first ? k_csum_reduce<C, true> : k_csum_reduce<C, false>), dim3(grid), dim3(kBlock), 0, c->stream, g, lv, io,
                     c->clusters.size.get());
}

extern "C" {

int sc_pairs_cluster_sums_device(sc_ctx* c, const double* dev_values, int64_t values_rows, int32_t channels, double* dev_sums,
                                 double* dev_mins, double* dev_maxs, int64_t room_clusters, int64_t* dev_counts) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_counts) return fail(SC_ERR_ARG, "null counts pointer");
  if (channels < 1 || channels > SC_CLUSTER_SUMS_MAX_CHANNELS)
    return fail(SC_ERR_ARG, "%d channels, it must be 1 .. %d", (int)channels, (int)SC_CLUSTER_SUMS_MAX_CHANNELS);
  static_assert(kClusterSumsMaxChannels == SC_CLUSTER_SUMS_MAX_CHANNELS, "the header's bound is the kernel's");
  if (room_clusters < 0 || values_rows < 0) return fail(SC_ERR_ARG, "negative room or number of value rows");
  if (!dev_values || (!dev_sums && room_clusters > 0)) return fail(SC_ERR_ARG, "null values or sums pointer");
  if ((uintptr_t)dev_values & 15) return fail(SC_ERR_ARG, "the values must be aligned to 16 bytes");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_pairs_cluster_sums_device inside a tick");
  if (!c->pairs.valid || !c->clusters.valid)
    return fail(SC_ERR_STATE, "no label to sum over: sc_pairs_count_device and sc_pairs_label_device come first, with no "
                              "count and no change of the state in between");
  HIPCHK(hipSetDevice(c->device));
  const int64_t m = c->clusters.m;
  ClusterSumSpace& w = c->csums;
  int rc = w.ensure(m, c->stream);
  if (rc) return rc;
  const CsumGuard g{c->pairs.words.get(), c->pairs.flag.get(), w.flag.get()};
  HIPCHK(hipMemsetAsync(w.flag, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(k_reader_check, dim3(1), dim3(kBlock), 0, c->stream, c->pairs.grid.radius, (const XY*)nullptr, 0LL, -1LL,
                     (long long)values_rows, g.words, g.flag, w.flag.get(), (long long*)dev_counts, (const long long*)nullptr, 0);
  if (m > 0) {
    const int grid = grid_for(m);
    const int* size = c->clusters.size.get();
    // the sort: the keys are 0 .. m (a dead row's), so as many digits as m has
    int bits = 1;
    while ((m >> bits) != 0) ++bits;
    int set;
    const CsumKey key{g.words, g.flag, g.own, c->clusters.parent.get(), c->clusters.isRoot.get(), c->clusters.dense.get(), (int)m};
    if ((rc = radix_sort(c, w.sort, key, m, (bits + kRadixDigitBits - 1) / kRadixDigitBits, &set))) return rc;
    int levels = 1;  // 64^levels >= m: the last level leaves every cluster one value
    for (int64_t reach = kCsumGroup; reach < m; reach *= kCsumGroup) ++levels;
    // Which of the four scans holds what: the member starts, the partial starts of level 0 (a level above numbers its
    // partials as its items), and the item starts of level k.  One is overwritten only after its last reader is queued.
    int* const member_start = w.st[0];
    int* const part_start = w.st[2];
    const auto item_start = [&](int k) { return w.st[k == 0 ? 1 : (k + 2) % 4].get(); };
    const auto count_scan = [&](int level, int as_elems, int* out) {
      hipLaunchKernelGGL(k_csum_count, dim3(grid), dim3(kBlock), 0, c->stream, g, (int)m, size, level, as_elems, w.cnt.get());
      return launch_scan(c, w.cnt, out, m, w.sums, nullptr);
    };
    if ((rc = launch_scan(c, size, member_start, m, w.sums, nullptr))) return rc;
    if ((rc = count_scan(0, 0, item_start(0)))) return rc;
    hipLaunchKernelGGL(k_csum_items, dim3(grid), dim3(kBlock), 0, c->stream, g, (int)m, w.sort.keys[set].get(), member_start,
                       item_start(0), w.items0.get());
    if (levels > 1) {
      if ((rc = count_scan(1, 1, part_start))) return rc;
      if ((rc = count_scan(1, 0, item_start(1)))) return rc;
    }
    const int64_t cap = ClusterSumSpace::partials(m);
    for (int k = 0; k < levels; ++k) {
      const bool last = k + 1 == levels;
      if (k >= 1 && !last)
        if ((rc = count_scan(k + 1, 0, item_start(k + 1)))) return rc;
      CsumLevel lv{};
      lv.level = k;
      lv.items = k == 0 ? w.items0.get() : w.items[(k - 1) & 1].get();
      lv.total = item_start(k) + m;
      lv.in_start = k == 0 ? member_start : k == 1 ? part_start : item_start(k - 1);
      lv.out_start = k == 0 ? part_start : item_start(k);
      lv.next_start = last ? nullptr : item_start(k + 1);
      lv.next_items = w.items[k & 1].get();
      const CsumIo io{dev_values, w.sort.vals[set].get(), w.part[(k + 1) & 1].get(), w.part[k & 1].get(), (long long)cap,
                      dev_sums, dev_mins, dev_maxs, (long long)room_clusters, (int)channels};
      // the items -- at most m at level 0, `cap` above -- in equal shares: a wave each while they last
      const int64_t bound = k == 0 ? m : cap;
      const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((bound + kBlock / 64 - 1) / (kBlock / 64), (int64_t)c->num_cus * 8));
      if (channels <= 1) csum_launch<1>(c, k == 0, blocks, g, lv, io);
      else if (channels <= 2) csum_launch<2>(c, k == 0, blocks, g, lv, io);
      else if (channels <= 4) csum_launch<4>(c, k == 0, blocks, g, lv, io);
      else csum_launch<8>(c, k == 0, blocks, g, lv, io);
    }
  }
  hipLaunchKernelGGL(k_csum_finish, dim3(1), dim3(64), 0, c->stream, g, c->clusters.dense.get(), (int)m, (long long*)dev_counts);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

}  // extern "C"

// ---- what the readers with rows of their own share: tables, sums, gradients, histograms -------------------------

// A reader's call as its messages name it.
struct ReaderCall {
  const char* who;     // the function
  const char* verb;    // "no pair count to <verb>"
  const char* holder;  // "<holder> <room> rows": the caller's array with a row per row, and its verb
  bool batched_ok;     // reads a batched grid
  bool holds_rows;     // the caller gave such an array: its room is tested against the rows
  const char* twin = nullptr;  // with `batched_ok` off: the call that reads a batched grid; on: the one `who` is the
                               // batched form of, which makes `who` refuse an unbatched grid
};

// ... and what it launches with.
struct Reader {
  int64_t rows;
  const XY* queries;  // null: the self form
  PairsView view;
};

// The checks and the preparation every reader begins with, after the checks of its own arguments.
static int reader_begin(sc_ctx* c, const ReaderCall& call, const double* dev_queries, int64_t n_queries, int64_t room_rows,
                        Reader* r) {
  if (room_rows < 0) return fail(SC_ERR_ARG, "negative room");
  if (dev_queries && n_queries < 0) return fail(SC_ERR_ARG, "negative query count");
  if ((uintptr_t)dev_queries & 15) return fail(SC_ERR_ARG, "the queries must be aligned to 16 bytes");
  if (c->in_step) return fail(SC_ERR_STATE, "%s inside a tick", call.who);
  if (!c->pairs.valid)
    return fail(SC_ERR_STATE, "no pair count to %s: sc_pairs_count_device comes first, and the state must not change in between",
                call.verb);
  if (!call.batched_ok || call.twin)
    if (const int rc = pairs_grid_is(c, call.batched_ok, call.who, call.twin)) return rc;
  if (dev_queries && n_queries > kPairsMaxPoints)
    return fail(SC_ERR_CAPACITY, "%lld queries, at most %lld", (long long)n_queries, (long long)kPairsMaxPoints);
  r->rows = dev_queries ? n_queries : c->pairs.m;
  if (call.holds_rows && room_rows < r->rows)
    return fail(SC_ERR_CAPACITY, "%s %lld rows, up to %lld %s", call.holder, (long long)room_rows, (long long)r->rows,
                dev_queries ? "queries" : "points");
  const int64_t* qptr;
  if (!c->pairs.take_query_batch(dev_queries != nullptr, &qptr))
    return fail(SC_ERR_ARG, "queries on a batched grid need sc_pairs_set_query_batch_device first");
  HIPCHK(hipSetDevice(c->device));
  r->queries = (const XY*)dev_queries;
  r->view = c->pairs.view(qptr);
  return SC_OK;
}

// The reader's own flag zeroed -- the `zero_bytes` from `zero` on, which hold it --, then k_reader_check: a thread per
// query, and on a batched grid per entry of query_ptr.  `row_rows` / `part_rows`: the rows of the caller's arrays that go
// by row / by partner, -1 for none.  The radius is the count's.
static int reader_check(sc_ctx* c, const Reader& r, int* own_flag, void* zero, size_t zero_bytes, int64_t row_rows,
                        int64_t part_rows, int64_t* dev_counts) {
  HIPCHK(hipMemsetAsync(zero, 0, zero_bytes, c->stream));
  const PairsBatch& bt = r.view.bt;
  const int grid = !r.queries ? 1 : grid_for(bt.qptr ? std::max<int64_t>(r.rows, (int64_t)bt.clouds + 1) : r.rows);
  hipLaunchKernelGGL(k_reader_check, dim3(grid), dim3(kBlock), 0, c->stream, c->pairs.grid.radius, r.queries,
                     (long long)r.rows, (long long)row_rows, (long long)part_rows, r.view.words, r.view.flag, own_flag,
                     (long long*)dev_counts, bt.qptr, bt.clouds);
  return SC_OK;
}

// ... for the readers whose flag is the pairs workspace's.
static int reader_check(sc_ctx* c, const Reader& r, int64_t row_rows, int64_t part_rows, int64_t* dev_counts) {
  int* own = c->pairs.readerFlag.get();
  return reader_check(c, r, own, own, sizeof(int), row_rows, part_rows, dev_counts);
}

// ---- nearest-k tables (sc_nearest.h) -------------------------------------------------------------

template <int K>
static void nearest_launch(sc_ctx* c, const Reader& r, int k, const NearestOut& out) {
  const int64_t grid = std::max<int64_t>(1, (r.rows + kNearestBlock - 1) / kNearestBlock);  // (one at least: it writes the counts)
  const PairsView& v = r.view;  // (unpacked: k_nearest alone keeps loose arguments, sc_nearest.h says why)
  hipLaunchKernelGGL((v.bt.clouds ? k_nearest<K, true> : k_nearest<K, false>), dim3((unsigned)grid), dim3(kNearestBlock), 0,
                     c->stream, v.g, v.words, v.flag, c->pairs.readerFlag.get(), v.xy, r.queries, (long long)r.rows, k, v.start,
                     v.sxy, v.scell, v.sidx, out, v.bt);
}

extern "C" {

int sc_pairs_nearest_device(sc_ctx* c, const double* dev_queries, int64_t n_queries, int32_t k, int64_t* dev_neighbors,
                            double* dev_d2, int64_t* dev_partners, int64_t room_rows, int64_t* dev_counts) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_neighbors || !dev_counts) return fail(SC_ERR_ARG, "null neighbors or counts pointer");
  if (k < 1 || k > SC_NEAREST_MAX_K) return fail(SC_ERR_ARG, "k is %d, it must be 1 .. %d", (int)k, (int)SC_NEAREST_MAX_K);
  static_assert(kNearestMaxK == SC_NEAREST_MAX_K, "the header's bound is the kernel's");
  Reader r;
  if (const int rc = reader_begin(c, {"sc_pairs_nearest_device", "search in", "the table holds", true, true}, dev_queries,
                                  n_queries, room_rows, &r))
    return rc;
  const NearestOut out{(long long*)dev_neighbors, dev_d2, (long long*)dev_partners, (long long*)dev_counts};
  if (const int rc = reader_check(c, r, -1, -1, dev_counts)) return rc;
  if (k <= kNearestFewK) nearest_launch<kNearestFewK>(c, r, k, out);
  else if (k <= kNearestMidK) nearest_launch<kNearestMidK>(c, r, k, out);
  else nearest_launch<kNearestMaxK>(c, r, k, out);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

}  // extern "C"

// ---- weighted neighbourhood sums (sc_fields.h) ---------------------------------------------------

template <int C>
static void fields_launch(sc_ctx* c, const Reader& r, int self, int power, int channels, const double* values,
                          const FieldsOut& out) {
  hipLaunchKernelGGL((r.view.bt.clouds ? k_fields_sum<C, true> : k_fields_sum<C, false>), dim3(grid_for(r.rows)), dim3(kBlock), 0,
                     c->stream, r.view, c->pairs.readerFlag.get(), r.queries, (long long)r.rows, self, power, channels, values,
                     out);
}

extern "C" {

int sc_pairs_sum_device(sc_ctx* c, const double* dev_queries, int64_t n_queries, const double* dev_values, int64_t values_rows,
                        int32_t channels, int32_t power, int32_t flags, double* dev_sums, double* dev_wsum, int64_t room_rows,
                        int64_t* dev_counts) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_counts) return fail(SC_ERR_ARG, "null counts pointer");
  if (!dev_sums && !dev_wsum) return fail(SC_ERR_ARG, "neither sums nor weight sums to write");
  if (channels < 0 || channels > SC_FIELDS_MAX_CHANNELS)
    return fail(SC_ERR_ARG, "%d channels, it must be 0 .. %d", (int)channels, (int)SC_FIELDS_MAX_CHANNELS);
  if (channels > 0 && (!dev_values || !dev_sums)) return fail(SC_ERR_ARG, "null values or sums pointer with %d channels", (int)channels);
  if (power < 0 || power > 3) return fail(SC_ERR_ARG, "power is %d, it must be 0 .. 3", (int)power);
  if (flags & ~SC_FIELDS_SELF) return fail(SC_ERR_ARG, "unknown flags %d", flags);
  if (room_rows < 0 || values_rows < 0) return fail(SC_ERR_ARG, "negative room or number of value rows");
  static_assert(kFieldsMaxChannels == SC_FIELDS_MAX_CHANNELS, "the header's bound is the kernel's");
  Reader r;
  if (const int rc = reader_begin(c, {"sc_pairs_sum_device", "sum over", "the sums hold", true, true}, dev_queries, n_queries,
                                  room_rows, &r))
    return rc;
  const double* values = channels ? dev_values : nullptr;
  const FieldsOut out{channels ? dev_sums : nullptr, dev_wsum, (long long*)dev_counts};
  const int self = (flags & SC_FIELDS_SELF) ? 1 : 0;
  if (const int rc = reader_check(c, r, -1, values ? values_rows : -1, dev_counts)) return rc;
  if (channels <= 1) fields_launch<1>(c, r, self, power, channels, values, out);
  else if (channels <= 2) fields_launch<2>(c, r, self, power, channels, values, out);
  else if (channels <= 4) fields_launch<4>(c, r, self, power, channels, values, out);
  else fields_launch<8>(c, r, self, power, channels, values, out);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

}  // extern "C"

// ---- the position gradient of the sums (sc_fields_grad.h) -----------------------------------------

template <int C>
static void fields_grad_launch(sc_ctx* c, const Reader& r, int power, int channels, const FieldsGradIn& in, double* grad,
                               long long* counts) {
  const PairsView& v = r.view;  // (unpacked, as for k_nearest: sc_fields_grad.h says why)
  hipLaunchKernelGGL((v.bt.clouds ? k_fields_grad<C, true> : k_fields_grad<C, false>), dim3(grid_for(r.rows)), dim3(kBlock), 0,
                     c->stream, v.g, v.words, v.flag, c->pairs.readerFlag.get(), v.xy, r.queries, (long long)r.rows, power,
                     channels, v.start, v.sxy, v.scell, v.sidx, in, (XY*)grad, counts, v.bt);
}

extern "C" {

int sc_pairs_sum_grad_device(sc_ctx* c, const double* dev_queries, int64_t n_queries, const double* dev_row_a,
                             int64_t row_a_rows, const double* dev_part_b, int64_t part_b_rows, int32_t channels,
                             const double* dev_row_s, const double* dev_part_s, int32_t power, double* dev_grad,
                             int64_t room_rows, int64_t* dev_counts) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_counts) return fail(SC_ERR_ARG, "null counts pointer");
  if (!dev_grad) return fail(SC_ERR_ARG, "null gradient pointer");
  if (channels < 0 || channels > SC_FIELDS_MAX_CHANNELS)
    return fail(SC_ERR_ARG, "%d channels, it must be 0 .. %d", (int)channels, (int)SC_FIELDS_MAX_CHANNELS);
  if (channels > 0 && (!dev_row_a || !dev_part_b)) return fail(SC_ERR_ARG, "null row_a or part_b pointer with %d channels", (int)channels);
  if (power < 0 || power > 3) return fail(SC_ERR_ARG, "power is %d, it must be 0 .. 3", (int)power);
  if (room_rows < 0 || row_a_rows < 0 || part_b_rows < 0) return fail(SC_ERR_ARG, "negative room or number of rows");
  // (reader_begin's check, here as well: it goes before the gradient's alignment, which is tested with the queries')
  if (dev_queries && n_queries < 0) return fail(SC_ERR_ARG, "negative query count");
  if (((uintptr_t)dev_queries | (uintptr_t)dev_grad) & 15) return fail(SC_ERR_ARG, "the queries and the gradient must be aligned to 16 bytes");
  Reader r;
  if (const int rc = reader_begin(c, {"sc_pairs_sum_grad_device", "sum over", "the gradient holds", true, true}, dev_queries,
                                  n_queries, room_rows, &r))
    return rc;
  const FieldsGradIn in{channels ? dev_row_a : nullptr, channels ? dev_part_b : nullptr, dev_row_s, dev_part_s};
  long long* counts = (long long*)dev_counts;
  if (const int rc = reader_check(c, r, in.row_a || in.row_s ? row_a_rows : -1, in.part_b || in.part_s ? part_b_rows : -1, dev_counts))
    return rc;
  if (channels <= 1) fields_grad_launch<1>(c, r, power, channels, in, dev_grad, counts);
  else if (channels <= 2) fields_grad_launch<2>(c, r, power, channels, in, dev_grad, counts);
  else if (channels <= 4) fields_grad_launch<4>(c, r, power, channels, in, dev_grad, counts);
  else fields_grad_launch<8>(c, r, power, channels, in, dev_grad, counts);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

}  // extern "C"

// ---- distance histograms (sc_hist.h) --------------------------------------------------------------

template <int NB>
static void hist_launch(sc_ctx* c, const Reader& r, const HistEdges& edges, int bins, long long* acc, const HistOut& out) {
  const int64_t grid = std::max<int64_t>(1, (r.rows + kHistBlock - 1) / kHistBlock);  // (one at least: it writes the counts)
  hipLaunchKernelGGL((r.view.bt.clouds ? k_hist<NB, true> : k_hist<NB, false>), dim3((unsigned)grid), dim3(kHistBlock), 0,
                     c->stream, r.view, edges, bins, c->hist.flag(), r.queries, (long long)r.rows, acc, out);
}

// sc_pairs_hist_device and sc_pairs_hist_batch_device: `batched` says which; `dev_total` holds bins words, or -- batched --
// `room_clouds` x bins.
static int pairs_hist(sc_ctx* c, bool batched, const double* dev_queries, int64_t n_queries, const double* edges2, int32_t bins,
                      int32_t* dev_table, int64_t* dev_total, int64_t room_rows, int64_t room_clouds, int64_t* dev_counts) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_counts) return fail(SC_ERR_ARG, "null counts pointer");
  if (!dev_table && !dev_total) return fail(SC_ERR_ARG, "neither a table nor totals to write");
  if (bins < 1 || bins > SC_HIST_MAX_BINS) return fail(SC_ERR_ARG, "%d bins, it must be 1 .. %d", (int)bins, (int)SC_HIST_MAX_BINS);
  if (!edges2) return fail(SC_ERR_ARG, "null edges pointer");
  if (!(edges2[0] >= 0) || !std::isfinite(edges2[0])) return fail(SC_ERR_ARG, "the first squared edge must be finite and not negative");
  for (int k = 0; k < bins; ++k)
    if (!(edges2[k] < edges2[k + 1])) return fail(SC_ERR_ARG, "the squared edges must be strictly ascending (edge %d is not)", k + 1);
  static_assert(kHistMaxBins == SC_HIST_MAX_BINS, "the header's bound is the kernel's");
  if (batched && room_clouds < 0) return fail(SC_ERR_ARG, "negative room");
  Reader r;
  const ReaderCall call = batched ? ReaderCall{"sc_pairs_hist_batch_device", "take a histogram of", "the table holds", true,
                                               dev_table != nullptr, "sc_pairs_hist_device"}
                                  : ReaderCall{"sc_pairs_hist_device", "take a histogram of", "the table holds", false,
                                               dev_table != nullptr, "sc_pairs_hist_batch_device"};
  if (const int rc = reader_begin(c, call, dev_queries, n_queries, room_rows, &r)) return rc;
  if (!(edges2[bins] <= c->pairs.grid.r2))
    return fail(SC_ERR_ARG, "the last squared edge %.17g lies beyond the count's squared radius %.17g", edges2[bins], c->pairs.grid.r2);
  const int64_t cells = batched ? c->pairs.clouds * bins : 0;  // the batched accumulator: a line of bins per cloud
  if (cells > SC_HIST_BATCH_MAX_CELLS)
    return fail(SC_ERR_CAPACITY, "%lld clouds x %d bins, at most %lld words of totals", (long long)c->pairs.clouds, (int)bins,
                (long long)SC_HIST_BATCH_MAX_CELLS);
  if (batched && dev_total && room_clouds < c->pairs.clouds)
    return fail(SC_ERR_CAPACITY, "the totals hold %lld clouds, the grid has %lld", (long long)room_clouds, (long long)c->pairs.clouds);
  if (const int rc = c->hist.ensure(c->stream, cells)) return rc;
  r.view.g.r2 = edges2[bins];  // the full list up to the histogram's own last edge: the cells are the count's, which are no smaller
  HistEdges edges{};
  std::copy(edges2, edges2 + bins + 1, edges.e2);
  const HistOut out{(int*)dev_table, (long long*)dev_total, (long long*)dev_counts};
  // (one memset: the accumulator and, behind it, the flag -- batched: the flag and, behind it, the clouds' accumulator)
  long long* acc = batched ? c->hist.batch_acc() : c->hist.acc();
  void* zero = batched ? (void*)c->hist.flag() : (void*)c->hist.words.get();
  const size_t zero_words = batched ? (size_t)cells + 1 : (size_t)kHistMaxBins + 1;
  if (const int rc = reader_check(c, r, c->hist.flag(), zero, zero_words * sizeof(long long), -1, -1, dev_counts)) return rc;
  if (bins <= kHistFewBins) hist_launch<kHistFewBins>(c, r, edges, bins, acc, out);
  else if (bins <= kHistMidBins) hist_launch<kHistMidBins>(c, r, edges, bins, acc, out);
  else hist_launch<kHistMaxBins>(c, r, edges, bins, acc, out);
  if (dev_total) {
    const long long words = batched ? (long long)cells : (long long)bins;
    hipLaunchKernelGGL(k_hist_finish, dim3((unsigned)((words + kHistBlock - 1) / kHistBlock)), dim3(kHistBlock), 0, c->stream,
                       words, r.view.flag, c->hist.flag(), acc, out.total);
  }
  HIPCHK(hipGetLastError());
  return SC_OK;
}

extern "C" {

int sc_pairs_hist_device(sc_ctx* c, const double* dev_queries, int64_t n_queries, const double* edges2, int32_t bins,
                         int32_t* dev_table, int64_t* dev_total, int64_t room_rows, int64_t* dev_counts) {
  return pairs_hist(c, false, dev_queries, n_queries, edges2, bins, dev_table, dev_total, room_rows, 0, dev_counts);
}

int sc_pairs_hist_batch_device(sc_ctx* c, const double* dev_queries, int64_t n_queries, const double* edges2, int32_t bins,
                               int32_t* dev_table, int64_t* dev_cloud_total, int64_t room_rows, int64_t room_clouds,
                               int64_t* dev_counts) {
  return pairs_hist(c, true, dev_queries, n_queries, edges2, bins, dev_table, dev_cloud_total, room_rows, room_clouds, dev_counts);
}

}  // extern "C"

// ---- ray sensors (sc_rays.h) ----------------------------------------------------------------------

// What a rays call launches with: the reader, the directions, the walls by value, a wave per ray.
struct RaysCall {
  Reader r;
  const XY* dirs;
  RayWalls walls;
  unsigned grid;  // (one at least: it writes the counts)
};

// What the rays and the ray paths share, after the checks of their own arguments: the checks of the common ones, the
// reader's, the disc radius against the count's, and the check passes over leg 0.  `one`, `many`: the call and its
// batched form, `batched` says which this is.
static int rays_begin(sc_ctx* c, bool batched, const char* one, const char* many, const char* holder, const double* dev_origins,
                      const double* dev_directions, int64_t n_rays, double disc_radius, double max_t, const double* segments,
                      int32_t n_segments, int64_t room_rows, int64_t* dev_counts, RaysCall* call) {
  if (n_rays < 0) return fail(SC_ERR_ARG, "negative ray count");
  if ((uintptr_t)dev_directions & 15) return fail(SC_ERR_ARG, "the directions must be aligned to 16 bytes");
  if (!(max_t >= 0) || !std::isfinite(max_t)) return fail(SC_ERR_ARG, "max_t must be finite and not negative");
  if (!(disc_radius >= 0) || !std::isfinite(disc_radius)) return fail(SC_ERR_ARG, "the disc radius must be finite and not negative");
  if (n_segments < 0 || n_segments > kMaxSeg) return fail(SC_ERR_CAPACITY, "%d segments, at most %d", (int)n_segments, kMaxSeg);
  if (n_segments > 0 && !segments) return fail(SC_ERR_ARG, "null segment array");
  const ReaderCall names = batched ? ReaderCall{many, "send rays through", holder, true, true, one}
                                   : ReaderCall{one, "send rays through", holder, false, true, many};
  Reader& r = call->r;
  if (const int rc = reader_begin(c, names, dev_origins, n_rays, room_rows, &r)) return rc;
  if (!(disc_radius <= c->pairs.grid.radius / 2))
    return fail(SC_ERR_ARG, "the disc radius %.17g is more than half the count's radius %.17g: count at twice the disc radius",
                disc_radius, c->pairs.grid.radius);
  call->dirs = (const XY*)dev_directions;
  call->walls = RayWalls{};
  call->walls.n = n_segments;
  if (n_segments) std::memcpy(call->walls.s, segments, sizeof(double) * 4 * (size_t)n_segments);
  call->grid = (unsigned)std::max<int64_t>(1, r.rows);
  if (const int rc = reader_check(c, r, -1, -1, dev_counts)) return rc;
  if (disc_radius > 0)
    hipLaunchKernelGGL(k_rays_check, dim3(grid_for(r.rows)), dim3(kBlock), 0, c->stream, c->pairs.grid.radius, call->walls, max_t,
                       r.queries, call->dirs, (long long)r.rows, c->pairs.readerFlag.get());
  return SC_OK;
}

// sc_pairs_rays_device and sc_pairs_rays_batch_device: `batched` says which.
static int pairs_rays(sc_ctx* c, bool batched, const double* dev_origins, const double* dev_directions, int64_t n_rays,
                      double disc_radius, double max_t, const double* segments, int32_t n_segments, double* dev_t,
                      int64_t* dev_hit, int64_t room_rows, int64_t* dev_counts) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_origins || !dev_directions || !dev_t || !dev_hit || !dev_counts)
    return fail(SC_ERR_ARG, "null origins, directions, t, hit or counts pointer");
  RaysCall k;
  if (const int rc = rays_begin(c, batched, "sc_pairs_rays_device", "sc_pairs_rays_batch_device", "t and hit hold", dev_origins,
                                dev_directions, n_rays, disc_radius, max_t, segments, n_segments, room_rows, dev_counts, &k))
    return rc;
  const RayOut out{dev_t, (long long*)dev_hit, (long long*)dev_counts};
  hipLaunchKernelGGL(batched ? k_rays<true> : k_rays<false>, dim3(k.grid), dim3(kRayBlock), 0, c->stream, k.r.view, k.walls,
                     (int)(disc_radius > 0), disc_radius * disc_radius, max_t, c->pairs.readerFlag.get(), k.r.queries, k.dirs,
                     (long long)k.r.rows, out);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

// sc_pairs_ray_paths_device and sc_pairs_ray_paths_batch_device: `batched` says which.
static int pairs_ray_paths(sc_ctx* c, bool batched, const double* dev_origins, const double* dev_directions, int64_t n_rays,
                           int32_t bounces, double disc_radius, double max_t, const double* segments, int32_t n_segments,
                           double* dev_t, int64_t* dev_hit, double* dev_points, double* dev_normals, int64_t* dev_end,
                           int64_t room_rows, int64_t* dev_counts) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_origins || !dev_directions || !dev_t || !dev_hit || !dev_points || !dev_normals || !dev_end || !dev_counts)
    return fail(SC_ERR_ARG, "null origins, directions, t, hit, points, normals, end or counts pointer");
  if (bounces < 0 || bounces > SC_RAY_MAX_BOUNCES)
    return fail(SC_ERR_ARG, "%d bounces, it must be 0 .. %d", (int)bounces, (int)SC_RAY_MAX_BOUNCES);
  static_assert(kRayMaxLegs == SC_RAY_MAX_BOUNCES + 1, "the header's bound is the kernel's");
  if (((uintptr_t)dev_points | (uintptr_t)dev_normals) & 15) return fail(SC_ERR_ARG, "the points and the normals must be aligned to 16 bytes");
  RaysCall k;
  if (const int rc = rays_begin(c, batched, "sc_pairs_ray_paths_device", "sc_pairs_ray_paths_batch_device", "the paths hold",
                                dev_origins, dev_directions, n_rays, disc_radius, max_t, segments, n_segments, room_rows,
                                dev_counts, &k))
    return rc;
  const RayPathOut out{dev_t, (long long*)dev_hit, (XY*)dev_points, (XY*)dev_normals, (long long*)dev_end, (long long*)dev_counts};
  hipLaunchKernelGGL(batched ? k_ray_paths<true> : k_ray_paths<false>, dim3(k.grid), dim3(kRayBlock), 0, c->stream, k.r.view,
                     k.walls, (int)(disc_radius > 0), disc_radius * disc_radius, max_t, (int)bounces + 1,
                     c->pairs.readerFlag.get(), k.r.queries, k.dirs, (long long)k.r.rows, out);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

extern "C" {

int sc_pairs_rays_device(sc_ctx* c, const double* dev_origins, const double* dev_directions, int64_t n_rays, double disc_radius,
                         double max_t, const double* segments, int32_t n_segments, double* dev_t, int64_t* dev_hit,
                         int64_t room_rows, int64_t* dev_counts) {
  return pairs_rays(c, false, dev_origins, dev_directions, n_rays, disc_radius, max_t, segments, n_segments, dev_t, dev_hit,
                    room_rows, dev_counts);
}

int sc_pairs_rays_batch_device(sc_ctx* c, const double* dev_origins, const double* dev_directions, int64_t n_rays,
                               double disc_radius, double max_t, const double* segments, int32_t n_segments, double* dev_t,
                               int64_t* dev_hit, int64_t room_rows, int64_t* dev_counts) {
  return pairs_rays(c, true, dev_origins, dev_directions, n_rays, disc_radius, max_t, segments, n_segments, dev_t, dev_hit,
                    room_rows, dev_counts);
}

int sc_pairs_ray_paths_device(sc_ctx* c, const double* dev_origins, const double* dev_directions, int64_t n_rays, int32_t bounces,
                              double disc_radius, double max_t, const double* segments, int32_t n_segments, double* dev_t,
                              int64_t* dev_hit, double* dev_points, double* dev_normals, int64_t* dev_end, int64_t room_rows,
                              int64_t* dev_counts) {
  return pairs_ray_paths(c, false, dev_origins, dev_directions, n_rays, bounces, disc_radius, max_t, segments, n_segments, dev_t,
                         dev_hit, dev_points, dev_normals, dev_end, room_rows, dev_counts);
}

int sc_pairs_ray_paths_batch_device(sc_ctx* c, const double* dev_origins, const double* dev_directions, int64_t n_rays,
                                    int32_t bounces, double disc_radius, double max_t, const double* segments,
                                    int32_t n_segments, double* dev_t, int64_t* dev_hit, double* dev_points, double* dev_normals,
                                    int64_t* dev_end, int64_t room_rows, int64_t* dev_counts) {
  return pairs_ray_paths(c, true, dev_origins, dev_directions, n_rays, bounces, disc_radius, max_t, segments, n_segments, dev_t,
                         dev_hit, dev_points, dev_normals, dev_end, room_rows, dev_counts);
}

}  // extern "C"
