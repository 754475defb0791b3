// What the host files of libsandcrate_hip.so share: the error string, the owned buffers, the sort's and the scan's
// launchers, every add-on's state, the context, and the short list of the tick's internals an add-on may use.
// Included by sandcrate_hip.hip -- the single translation unit -- after the kernel headers, whose types and constants it
// names; the sc_host_*.h files, one per feature family, are included at that file's end.
#pragma once
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "sc_kernels.h"
#include "sc_radix.h"

using namespace sc;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return fail(SC_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e_)); \
  } while (0)

enum KernelId { K_APPEND = 0, K_WALL_BIN, K_SCAN, K_SCATTER, K_REORDER, K_NEIGHBORS, K_NOISE_OFFSETS, K_DENSITY, K_FORCE, K_HALO_PACK, K_HALO_UNPACK, K_PASS_A };

struct DeviceMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};

template <unsigned Flags>
struct PinnedMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
  static void release(void* p) { (void)hipHostFree(p); }
};

// `size()` elements of T that the owner frees.  grow(n, stream) makes room for n elements and does not keep the
// contents: it waits for `stream` (the last user of the old memory), frees, and records the new size only once the
// allocation has succeeded -- a failed growth leaves the buffer empty, never dangling or larger than it is.
template <class T, class Mem>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  Owned& operator=(Owned o) noexcept {
    std::swap(p_, o.p_);
    std::swap(n_, o.n_);
    return *this;
  }
  ~Owned() { reset(); }

  hipError_t grow(int64_t n, hipStream_t stream) {
    if (n <= n_) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    reset();
    void* p = nullptr;
    const hipError_t a = Mem::alloc(&p, std::max<int64_t>(n, 1) * sizeof(T));
    if (a != hipSuccess) return a;
    p_ = (T*)p;
    n_ = n;
    return hipSuccess;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  int64_t size() const { return n_; }
  size_t bytes() const { return (size_t)n_ * sizeof(T); }

 private:
  void reset() {
    if (p_) Mem::release(p_);
    p_ = nullptr;
    n_ = 0;
  }
  T* p_ = nullptr;
  int64_t n_ = 0;
};

template <class T>
using DevBuf = Owned<T, DeviceMem>;
template <class T>
using HostBuf = Owned<T, PinnedMem<hipHostMallocDefault>>;  // pinned host memory

// The workspace of a radix sort (sc_radix.h; radix_sort below): the (key, value) pairs -- two sets that take turns --,
// the tiles' digit counts, their scan and its block sums.
struct RadixSpace {
  DevBuf<unsigned> keys[2];
  DevBuf<int> vals[2], hist, offs, sums;
  // Room for a sort of m pairs: sized by the last member, which grows last.
  int ensure(int64_t m, hipStream_t stream) {
    if (m <= vals[1].size()) return SC_OK;
    const int64_t cells = (m + kRadixTile - 1) / kRadixTile * kRadixBins;  // a count per tile and digit
    HIPCHK(hist.grow(cells, stream));
    HIPCHK(offs.grow(cells + 1, stream));
    HIPCHK(sums.grow(cells / kScanPerBlock + 2, stream));
    for (int k = 0; k < 2; ++k) {
      HIPCHK(keys[k].grow(m, stream));
      HIPCHK(vals[k].grow(m, stream));
    }
    return SC_OK;
  }
};

// What a tick takes from the caller: coefficients, walls (the segments and their padded twins) and rigid bodies.
struct TickInputs {
  sc_params params{};
  int nseg = 0, nbody = 0;
  Seg seg[kMaxSeg]{};
  Seg pad[2 * kMaxSeg]{};
  BodyK body[kMaxBody]{};
};

// ---- the add-ons' state: one struct per feature, one member of sc_ctx each --------------------------------------------
// Where a group of buffers is sized by its last member, which grows last (once it has grown, so have the others), the
// rule is the struct's ensure(), as RadixSpace::ensure is.

// The probe (sc_probe.h; sc_host_logs.h): the workgroups' partial records, its own words (ticket, log head, dropped ticks),
// the row and profile of sc_probe_now, and the log of sc_probe_enable -- rows, bin counts and the bins' tops as 64-bit keys.
struct ProbeState {
  DevBuf<double> partials, nowRow, rows;
  DevBuf<int> words, nowCounts, counts;
  DevBuf<unsigned long long> nowTops, tops;
  bool on = false;
  int64_t cap = 0, tail = 0;  // ... its capacity in rows, and the first row not yet delivered
  int bins = 0;
  double x0 = 0.0, x1 = 1.0;
  int ensure(hipStream_t stream) {
    if (words.size() >= PW_COUNT) return SC_OK;
    HIPCHK(partials.grow((int64_t)kProbeBlocks * kProbeFields, stream));
    HIPCHK(nowRow.grow(kProbeFields, stream));
    HIPCHK(nowCounts.grow(kProbeMaxBins, stream));
    HIPCHK(nowTops.grow(kProbeMaxBins, stream));
    HIPCHK(words.grow(PW_COUNT, stream));
    HIPCHK(hipMemsetAsync(words, 0, words.bytes(), stream));
    return SC_OK;
  }
};

// Tracking (sc_track.h; sc_host_logs.h): the frame of sc_track_capture, the log of sc_track_enable with its words (byte
// cursor, frames, dropped frames, and where the frame being packed starts), and the frame sc_track_load unpacks.
struct TrackState {
  DevBuf<unsigned char> now, log, load;
  DevBuf<unsigned long long> words;
  bool on = false;
  int64_t every = 1, cap = 0;  // ... every how many ticks a frame is logged, and the log's capacity in bytes
  int ensure(hipStream_t stream) {
    if (words.size() >= TW_COUNT) return SC_OK;
    HIPCHK(words.grow(TW_COUNT, stream));
    HIPCHK(hipMemsetAsync(words, 0, words.bytes(), stream));
    return SC_OK;
  }
};

// Trajectories (sc_traj.h; sc_host_logs.h): the log of sc_traj_enable_device -- the caller's device memory, not owned:
// states, pressure (or null), the frames' ticks, counts and outsiders, and the words (cursor, dropped frames, the frame
// the last reserve chose) -- with its capacity in frames, the window of ids and every how many ticks a frame is taken.
struct TrajState {
  TrajLog log{};
  bool on = false;
  int64_t frames = 0, id0 = 0, rows = 0, every = 1;
};

// What every rendered frame is made of and carries (sc_render.h, sc_hud.h, sc_arrows.h; sc_host_frames.h).
struct FrameState {
  // sc_render: the per-pixel key buffer and (host path) the device frame, grown to the largest frame asked for
  DevBuf<unsigned long long> keys;
  DevBuf<unsigned char> rgb;
  // sc_set_hud: the text and its lines' (start, length); hud_lines == 0: no HUD
  DevBuf<unsigned char> hudText;
  DevBuf<HudLine> hudLines;
  int hud_lines = 0, hud_longest = 0;  // ... how many lines, and the bytes of the longest
  int hud_x = 0, hud_y = 0, hud_scale = 1;
  // sc_set_arrows: the arrows; SC_ARROWS_OFF: none
  DevBuf<sc_arrow> arrowList;
  int arrow_mode = SC_ARROWS_OFF;
  int64_t arrow_n = 0, arrow_every = 1;  // ... the list's length; velocity mode: ids that are multiples of this
  double arrow_scale = 1.0;
};

// sc_jpeg_encode_device: the encoder's workspace (coefficients, per-block masks and code lengths, the rows' bit buffers,
// lengths and offsets; sc_jpeg.h) and the entropy-coded data, each grown to the largest frame asked for.
struct JpegSpace {
  DevBuf<unsigned char> work, out;
};

// sc_gif_encode_device: the encoder's workspace (the chunks' codes, counts and bit offsets; sc_gif.h) and the image data,
// and sc_render_gif's frame of palette indices, each grown to the largest frame asked for.
struct GifSpace {
  DevBuf<unsigned char> work, index;
  DevBuf<unsigned> out;
};

// sc_export_state_device (sc_state.h; sc_host_state.h): the sort of the (id, slot) pairs, grown to the launch bound asked
// for; sc_import_state_device: the ids as 32-bit values and its two words (largest id plus one, out-of-range flag).
struct StateIo {
  RadixSpace sort;
  DevBuf<int> ids, words;
};

// sc_pairs_count_device / sc_pairs_fill_device (sc_pairs.h; sc_host_state.h): the points in index order, the binning sort
// of the (bucket, index) pairs -- a workspace of its own: the fill reads its result, and an export may come in between --,
// the buckets' counts and starts, the members' positions and cells in bucket order, the row lengths, their 64-bit scan
// with its block sums, the domain flag and the two words (n, E); each grown to the largest bound asked for.
// `valid`: the workspace holds the grid of a count, and nothing has changed the state since.
// The batched form (sc_pairs_set_batch_device): `ptr`, the count's copy of the offsets, and `cloud`, every point's cloud;
// `clouds` > 0 says that the grid is batched.  `next_ptr` / `next_clouds` wait for the next count, `next_qptr` for the
// next query-form reader: the caller's device memory, read by that call's launches only.
// `readerFlag`: the flag of the reader that runs (sc_nearest.h, sc_fields.h, sc_fields_grad.h, sc_rays.h) -- a query outside the
// domain, an array of the caller's with too few rows, bad query offsets.  A flag apart from the count's, which stays as
// the count left it: a fill or a label after a reader still reads it.  One word for all of them: every reader zeroes it
// before its check, on the one stream, so no call's verdict reaches the next.
struct PairsSpace {
  DevBuf<XY> xy, sxy;
  DevBuf<uint2> cell;
  RadixSpace sort;
  DevBuf<int> bucketCount, bucketStart, bucketSums, rowLen, flag, readerFlag, cloud;
  DevBuf<long long> offs, sums, words, ptr;
  bool valid = false;
  int64_t m = 0;  // ... the bound its launches were sized by
  int set = 0;    // ... which of the sort's two sets holds the sorted pairs
  PairsGrid grid{};
  int64_t clouds = 0;
  const int64_t* next_ptr = nullptr;
  int64_t next_clouds = 0;
  const int64_t* next_qptr = nullptr;
  // The workspace as a reader's kernels see it: the full list (`half` off), whichever form the count had.  `qptr`: the
  // query offsets of a batched grid, null in the self form.
  PairsView view(const int64_t* qptr) const {
    PairsView v{grid, words.get(), flag.get(), xy.get(), bucketStart.get(), sxy.get(), cell.get(), sort.vals[set].get(),
                PairsBatch{ptr.get(), (const long long*)qptr, cloud.get(), (int)clouds}};
    v.g.half = 0;
    return v;
  }
  // ... and as the count and the fill see it: with the count's `half`.
  PairsView view_of_count() const {
    PairsView v = view(nullptr);
    v.g.half = grid.half;
    return v;
  }
  // The offsets a query-form reader of a batched grid was given (consumed); false when there are none.
  bool take_query_batch(bool query_form, const int64_t** qptr) {
    *qptr = nullptr;
    if (!clouds || !query_form) return true;
    *qptr = next_qptr;
    next_qptr = nullptr;
    return *qptr != nullptr;
  }
  // Room for a search over n points in `buckets` buckets.
  int ensure(int64_t n, int64_t buckets, hipStream_t stream) {
    HIPCHK(flag.grow(1, stream));
    HIPCHK(readerFlag.grow(1, stream));
    HIPCHK(words.grow(PW_WORDS, stream));
    if (buckets + 1 > bucketStart.size()) {
      HIPCHK(bucketCount.grow(buckets, stream));
      HIPCHK(bucketSums.grow(buckets / kScanPerBlock + 2, stream));
      HIPCHK(bucketStart.grow(buckets + 1, stream));
    }
    const int rc = sort.ensure(n, stream);
    if (rc) return rc;
    if (n + 1 > offs.size()) {
      HIPCHK(xy.grow(n, stream));
      HIPCHK(sxy.grow(n, stream));
      HIPCHK(cell.grow(n, stream));
      HIPCHK(rowLen.grow(n, stream));
      HIPCHK(sums.grow(n / kScanPerBlock + 2, stream));
      HIPCHK(offs.grow(n + 1, stream));
    }
    return SC_OK;
  }
};

// sc_pairs_label_device (sc_clusters.h; sc_host_state.h): the parents, the root marks, their scan (the dense numbers) with
// its block sums and the clusters' sizes -- apart from the pairs workspace, which a fill after the labelling still reads;
// each grown to the largest bound asked for.
// `valid`: they hold the label of the pairs workspace as it is -- every count clears it --, over the bound `m`.
struct ClusterSpace {
  DevBuf<int> parent, isRoot, size, sums, dense;
  bool valid = false;
  int64_t m = 0;
  int ensure(int64_t m, hipStream_t stream) {
    if (m + 1 <= dense.size()) return SC_OK;
    HIPCHK(parent.grow(m, stream));
    HIPCHK(isRoot.grow(m, stream));
    HIPCHK(size.grow(m, stream));
    HIPCHK(sums.grow(m / kScanPerBlock + 2, stream));
    HIPCHK(dense.grow(m + 1, stream));
    return SC_OK;
  }
};

// sc_pairs_cluster_sums_device (sc_cluster_sums.h; sc_host_state.h): the sort of the (label, index) pairs -- a workspace of
// its own: a fill or a table after the sums still reads the count's --, the per-cluster counts of a level, four scans of
// them that take turns (member starts, chunk starts, partial starts, and the upper levels' item starts), the scans' block
// sums, the call's flag, the item lists -- level 0 has up to m items, a level above at most partials(m) -- and the
// partials of two levels that take turns: sums, minima, maxima.  Each grown to the largest bound asked for.
struct ClusterSumSpace {
  RadixSpace sort;
  DevBuf<int> cnt, st[4], sums, flag;
  DevBuf<int2> items0, items[2];
  DevBuf<double> part[2];
  // A cluster has partials only with more than 64 elements: ceil(s / 64) <= s / 64 + s / 65 < s / 32 of them.
  static int64_t partials(int64_t m) { return m / 32 + 2; }
  int ensure(int64_t m, hipStream_t stream) {
    HIPCHK(flag.grow(1, stream));
    if (const int rc = sort.ensure(m, stream)) return rc;
    if (m + 1 <= st[3].size()) return SC_OK;
    HIPCHK(cnt.grow(m, stream));
    HIPCHK(sums.grow(m / kScanPerBlock + 2, stream));
    HIPCHK(items0.grow(m, stream));
    for (int k = 0; k < 2; ++k) {
      HIPCHK(items[k].grow(partials(m), stream));
      HIPCHK(part[k].grow(3 * partials(m) * kClusterSumsMaxChannels, stream));
    }
    for (int k = 0; k < 4; ++k) HIPCHK(st[k].grow(m + 1, stream));
    return SC_OK;
  }
};

// sc_pairs_hist_device (sc_hist.h; sc_host_state.h): the accumulator of the totals, kHistMaxBins 64-bit words, and behind
// it the word that holds the flag of the call's own -- a query outside the domain: the count's flag stays as the count
// left it.  One buffer, so that one memset prepares both; the readers' check gets the flag's address and nothing else.
// sc_pairs_hist_batch_device: its accumulator, `cells` = clouds x bins words, lies BEHIND the flag -- again one memset,
// from the flag on -- and the buffer is grown to the largest one asked for.
struct HistSpace {
  DevBuf<long long> words;
  int ensure(hipStream_t stream, int64_t cells = 0) {
    HIPCHK(words.grow(kHistMaxBins + 1 + cells, stream));
    return SC_OK;
  }
  long long* acc() const { return words.get(); }
  int* flag() const { return (int*)(words.get() + kHistMaxBins); }
  long long* batch_acc() const { return words.get() + kHistMaxBins + 1; }
};

// The checkpoint (sc_checkpoint_begin / _finish; sc_host_snapshot.h): device-side snapshot, pinned host copy, and the
// events that order them on the context's stream and the side stream.
struct Snapshot {
  DevBuf<double> d[4];
  DevBuf<int> id_d;
  DevBuf<RngState> rng_d;
  HostBuf<double> h[4];
  HostBuf<int> id_h, counters_h;  // (the C_COUNT counters)
  HostBuf<RngState> rng_h;
  int64_t n_bound = 0, tick = -1;
  bool has_rng = false, pending = false;
  hipEvent_t ready = nullptr, done = nullptr;
};

// A slab's link to its neighbors (sc_host_slab.h): the cut, the halo buffers and counters, the RCCL communicator and the
// overlap of the exchange with pass B.  The tick reads the cut (build_world) and the rest where it launches pass B.
struct SlabLink {
  long long own_lo = 0, own_hi = 0;
  int slab_axis = 0;  // 0: slabs of columns (x), 1: of rows (y)
  int halo = 0, has_left = 0, has_right = 0;
  double *haloL = nullptr, *haloR = nullptr;  // send buffers of the last sc_halo_pack (caller-owned device memory)
  int haloCap = 0;
  int64_t halo_ring_from = 0;  // first tick whose halo counts in the progress block belong to the current state
  // halo overlap (sc_set_halo_overlap): the exchange runs on the side stream between the two launches of pass B
  bool overlap = false, band_pending = false;
  bool band_by_flag = false;  // slabs of rows: the split force kernel is ONE launch + a polling kernel on the side stream (sc_set_band_flag)
  bool band_flagged = false;  // the pending band is announced by the flag (k_wait_band), not by ev_band
  int band_epoch = 0;
  hipEvent_t ev_band = nullptr, ev_xchg = nullptr;
  RcclComm comm = nullptr;  // RCCL communicator of the slab chain (sc_comm_init), or null
  int comm_world = 0;
  DevBuf<int> owned_out, colHist;  // sc_owned_count, sc_column_histogram
};

}  // namespace

// ---- the context ------------------------------------------------------------------------------------------------------
// The fields directly in sc_ctx are the tick's own; every add-on has one member.
// (hidden: its destructor, which frees the buffers, is not part of the library's exported symbols)
struct __attribute__((visibility("hidden"))) sc_ctx {
  int device = 0;
  int num_cus = 256;
  int tile_choice = 0;  // 0 = by grid size, 1 = always the narrow pass A tile, 2 = always the wide one (SANDCRATE_TILE, for tests)
  hipStream_t own_stream = nullptr, stream = nullptr, side_stream = nullptr;  // (the side stream: halo overlap, checkpoint)
  int64_t cap = 0;
  // the storage set (input of a tick, output of pass B); of the cell-sorted set only the ids are an array of their
  // own (id[1]) -- positions and velocities are the pairs sxy / svv
  DevBuf<double> x, y, vx, vy;
  DevBuf<int> id[2];
  DevBuf<int> cellS, wslotS, cellT, wslotT;
  DevBuf<SortKey> keys;  // a bucket slot's (x, id, storage index): k_scatter writes, k_sort_big sorts, k_reorder ranks
  DevBuf<int> keyCell;  // the packed cell of the particle in a bucket slot (k_scatter writes it next to the key)
  DevBuf<int> tileBounds;   // per block of kTileW sorted particles: its three candidate ranges (k_reorder)
  DevBuf<int> tileBoundsT;  // ... the three ranges its neighbor-table slots refer to (the search; sc_tiled.h)
  DevBuf<int> tileBand;  // per block of pass A / B: holds a particle that may be packed into a halo message
  DevBuf<int> cellCount, cellStart, sortedStamp;
  DevBuf<unsigned long long> scanDesc;  // the bucket scan's look-back descriptors, one per 2048 cells (k_scan_cells)
  unsigned scanStamp = 0;               // ... and the stamp of its last launch
  int scan_max_polls = kScanMaxPolls;   // ... and how often a workgroup asks for a predecessor's total before it gives up (sc_set_scan_patience)
  DevBuf<int2> sortTasks;  // k_sort_big's task list (cell, chunk | length): the scan writes it
  bool piles_now = false;  // the hint "big buckets exist", latched once per tick (sc_step_begin)
  int64_t live_hint_from = 0;  // the live count the device publishes is usable once a tick >= this one has finished
  DevBuf<RngState> rng;        // NumPy's MT19937 stream on the device (sc_rng_set_state), or empty
  DevBuf<double> monitor;      // force monitor: sum of |dv| per phase and the particle count (sc_enable_force_monitor)
  bool monitor_on = false;
  int64_t emit_most = 0;  // the largest per-call bound of emitted particles so far (sc_emit_particles)
  // the progress block (kProgress* in sc_kernels.h): written by the GPU, read by the host without synchronisation
  Owned<int, PinnedMem<hipHostMallocMapped>> progress;
  int* progress_dev = nullptr;  // ... its address on the device
  bool force_rank_big = false;
  DevBuf<double> wrec[2];  // wall records of even / odd ticks
  DevBuf<int> nbr;         // neighbor table of tiles beyond 65535 entries: -(sorted index + 1), 32 bit
  DevBuf<NbrRow> rows;     // neighbor table: a 32-byte row per sorted particle (twenty 12-bit tile slots and the count)
  DevBuf<double> P;
  DevBuf<XY> sxy, svv, snn;  // the sorted positions and velocities, the surface normals: 16-byte pairs
  DevBuf<int> counters;
  // SC_NOISE_HOST
  DevBuf<int> cntById, offById, idBlockSums;
  DevBuf<double> eta;  // pairs of uniforms
  int64_t etaPairs = 0;
  bool offsets_pending = false;  // the offsets of this tick are left to the launch that draws the noise (k_rng_noise_small)
  // staging for uploads
  DevBuf<double> stage_xy, stage_vxy;
  DevBuf<int> stage_ids;

  TickInputs now;
  bool have_params = false;
  int noise_mode = SC_NOISE_NONE;
  uint64_t seed = 0;
  int64_t tick = 0;
  int64_t upper = 0;    // host-side upper bound of the stored particle count
  int64_t next_id = 0;
  bool ids_bounded = false;  // the device has handed out ids since (sc_emit_particles): next_id is an upper bound, C_NEXT_ID the counter
  bool in_step = false;
  int64_t normals_valid = 0;
  bool custom_grid = false;  // sc_neighbor_search: grid from the data, no walls, no removal
  long long grid_row0 = 0, grid_col0 = 0;
  int grid_nrows = 0, grid_ncols = 0;
  double custom_d = 0;
  bool slab = false;  // slab mode (sc_set_slab); `link` has the rest
  std::vector<int> ids_host;
  int64_t stats_live = -1;  // live count read by sc_step_stats inside the current tick, or -1
  World w{};
  // sc_set_next_inputs: the promised inputs of the tick after the current one.  Its pads are never read: only the
  // WallInputs of that tick are used (sc_step_finish), and they hold no pads.
  bool have_next = false;
  TickInputs next;
  bool prebinned = false;     // the last sc_step_finish already ran K1 of the coming tick ...
  WallInputs promised{};      // ... with these inputs

  bool timing = false;
  struct Ev {
    hipEvent_t a, b;
    int k;
  };
  std::vector<Ev> ev_used, ev_free;
  double ms[SC_NUM_KERNELS] = {};
  int64_t launches[SC_NUM_KERNELS] = {};

  ProbeState probe;
  TrackState track;
  TrajState traj;
  FrameState frame;
  JpegSpace jpeg;
  GifSpace gif;
  StateIo state;
  PairsSpace pairs;
  ClusterSpace clusters;
  ClusterSumSpace csums;
  HistSpace hist;
  Snapshot snap;
  SlabLink link;
};

namespace {

// ---- what a feature file may use of the tick ----------------------------------------------------------------------------
// The sc_host_*.h files are included at the end of sandcrate_hip.hip and could name anything in it.  They keep to
//   the storage arrays x, y, vx, vy, id[0], P and counters;  cap, stream, device, tick;
//   in_step, prebinned, slab;  normals_valid, now.seg and now.nseg;
//   launch_bound and slot_bound, and abandon_promise, put_check and put_from_device, declared below;
//   and what this header defines,
// and to their own member of sc_ctx.  Some need more, and say so here:
//   sc_host_logs.h      the force monitor's monitor and monitor_on, which pass B reads; sc_track_load writes what an
//                       upload writes: upper, next_id, live_hint_from
//   sc_host_state.h     nothing more
//   sc_host_frames.h    nothing more
//   sc_host_slab.h      halo pack and unpack are the tick's first and last step on another rank: make_world and w,
//                       wall_inputs_of and promised, cellS, wslotS, cellCount and wrec (K1 of the arrivals), the progress
//                       block (progress_read, wait_ticks_finished, progress_dev); sc_column_histogram reads have_params,
//                       custom_grid and custom_d; side_stream
//   sc_host_snapshot.h  the whole stored state: rng, upper, next_id, live_hint_from, progress, index_order and
//                       write_pairs; side_stream (ensure_side_stream of sc_host_slab.h) and link.halo_ring_from
// The other way round the tick reads probe.on, track.on and traj.on (a logged tick is not fused) and launches probe_launch,
// track_launch and traj_launch after pass B, clears pairs.valid where the state changes, and reads `link` as said there.

// In slab mode the stored count changes on the device every tick (halo records arrive without the
// host knowing how many), so launches cover the capacity; surplus workgroups exit on their first load.
int64_t launch_bound(const sc_ctx* c) { return c->slab ? c->cap : c->upper; }
// ... and never more slots than there are.
int64_t slot_bound(const sc_ctx* c) { return std::min<int64_t>(launch_bound(c), c->cap); }
int abandon_promise(sc_ctx* c);
int put_check(sc_ctx* c, const void* xy, const void* vxy, int64_t n, bool reset);
int put_from_device(sc_ctx* c, const double* dev_xy, const double* dev_vxy, const int* dev_ids, int64_t max_id, int64_t n, bool reset);

struct Bracket {  // two HIP events around a launch when timing is on
  sc_ctx* c;
  sc_ctx::Ev ev{};
  bool on;
  Bracket(sc_ctx* ctx, int k) : c(ctx), on(ctx->timing) {
    if (!on) return;
    if (!c->ev_free.empty()) {
      ev = c->ev_free.back();
      c->ev_free.pop_back();
    } else if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) {
      on = false;
      return;
    }
    ev.k = k;
    (void)hipEventRecord(ev.a, c->stream);
  }
  ~Bracket() {
    if (!on) return;
    (void)hipEventRecord(ev.b, c->stream);
    c->ev_used.push_back(ev);
  }
};

int grid_for(int64_t n) { return (int)std::max<int64_t>(1, (n + kBlock - 1) / kBlock); }

// What a call does that hands the host as many bytes as the device decides (a JPEG, a GIF, a track frame or log):
// read_back brings the size, and later the bytes, to the host -- a copy on the context's stream and the synchronisation
// that makes it readable; refuse_room reports the size in *n_out whatever follows, and refuses a buffer that is too small
// (`fmt` takes the size and the room, in this order).
int read_back(sc_ctx* c, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return SC_OK;
}
int refuse_room(int64_t bytes, int64_t room, int64_t* n_out, const char* fmt) {
  *n_out = bytes;
  return bytes > room ? fail(SC_ERR_CAPACITY, fmt, (long long)bytes, (long long)room) : SC_OK;
}

// exclusive scan of in[0..n) into out[0..n], out[n] = total (also to *total_out if given)
int launch_scan(sc_ctx* c, const int* in, int* out, int64_t n, int* blockSums, int* total_out) {
  int nb = (int)((n + kScanPerBlock - 1) / kScanPerBlock);
  if (nb < 1) nb = 1;
  hipLaunchKernelGGL(k_scan_local, dim3(nb), dim3(kBlock), 0, c->stream, in, out, (int)n, blockSums);
  hipLaunchKernelGGL(k_scan_fix, dim3(nb), dim3(kBlock), 0, c->stream, out, (int)n, blockSums, nb, total_out);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

// Sorts the m pairs of `w` by the lowest `passes` digits of their keys (sc_radix.h) and yields in *set which of the two
// sets holds the result.  The pairs are those of set 0, or -- `first` is not RadixStored -- made by the first pass:
// (first(i), i).
template <class Key>
int radix_sort(sc_ctx* c, RadixSpace& w, Key first, int64_t m, int passes, int* set) {
  const int tiles = (int)((m + kRadixTile - 1) / kRadixTile);
  int in = 0, rc;
  for (int pass = 0; pass < passes && m > 0; ++pass, in ^= 1) {
    const int shift = pass * kRadixDigitBits;
    if (pass == 0)
      hipLaunchKernelGGL(k_radix_hist<Key>, dim3(tiles), dim3(kRadixTile), 0, c->stream, first, w.keys[in].get(),
                         w.vals[in].get(), (int)m, shift, tiles, w.hist.get());
    else
      hipLaunchKernelGGL(k_radix_hist<RadixStored>, dim3(tiles), dim3(kRadixTile), 0, c->stream, RadixStored{},
                         w.keys[in].get(), w.vals[in].get(), (int)m, shift, tiles, w.hist.get());
    if ((rc = launch_scan(c, w.hist, w.offs, (int64_t)tiles * kRadixBins, w.sums, nullptr))) return rc;
    hipLaunchKernelGGL(k_radix_scatter, dim3(tiles), dim3(kRadixTile), 0, c->stream, w.keys[in].get(), w.vals[in].get(),
                       w.keys[in ^ 1].get(), w.vals[in ^ 1].get(), (int)m, shift, tiles, w.offs.get());
  }
  *set = in;
  return SC_OK;
}

}  // namespace
