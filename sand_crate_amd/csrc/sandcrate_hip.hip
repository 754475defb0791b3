// libsandcrate_hip.so -- host side of the C ABI declared in include/sandcrate_hip.h.
// Owns the device memory (float64 SoA particle arrays, cell buckets, neighbor table), builds the
// per-tick kernel argument block and enqueues the kernels of sc_kernels.h on one HIP stream.
// gfx950 (MI355X) only; there is no CPU path in this library.
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
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "sandcrate_hip.h"
#include "sc_arrows.h"
#include "sc_gif.h"
#include "sc_hud.h"
#include "sc_jpeg.h"
#include "sc_kernels.h"
#include "sc_probe.h"
#include "sc_radix.h"
#include "sc_state.h"
#include "sc_pairs.h"
#include "sc_clusters.h"
#include "sc_track.h"
#include "sc_rccl.h"
#include "sc_render.h"
#include "sc_rng.h"
#include "sc_tiled.h"

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
const char* kKernelNames[SC_NUM_KERNELS] = {"append",    "wall_bin",      "cell_scan", "scatter", "reorder",
                                            "neighbors", "noise_offsets", "density",   "force_integrate",
                                            "halo_pack", "halo_unpack", "neighbors_density"};

// Largest s with sqrt(s) <= R.  sqrt is correctly rounded and monotone, so for s >= 0
// (sqrt(s) <= R) == (s <= threshold): the kernels compare squared distances and skip the sqrt
// while taking exactly the reference's decision (collision_detector.py:78-79, crate.py:229).
double sq_threshold(double R) {
  if (!(R >= 0)) return -1.0;
  if (std::isinf(R)) return R;
  double t = R * R;
  const double inf = std::numeric_limits<double>::infinity();
  while (std::sqrt(t) > R) t = std::nextafter(t, -inf);
  while (std::sqrt(std::nextafter(t, inf)) <= R) t = std::nextafter(t, inf);
  return t;
}

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

}  // namespace

// (hidden: its destructor, which frees the buffers, is not part of the library's exported symbols)
struct __attribute__((visibility("hidden"))) sc_ctx {
  int device = 0;
  int num_cus = 256;
  int tile_choice = 0;  // 0 = by grid size, 1 = always the narrow pass A tile, 2 = always the wide one (SANDCRATE_TILE, for tests)
  hipStream_t own_stream = nullptr, stream = nullptr;
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
  // halo overlap (sc_set_halo_overlap): the exchange runs on the side stream between the two launches of pass B
  bool overlap = false, band_pending = false;
  bool band_by_flag = false;  // slabs of rows: the split force kernel is ONE launch + a polling kernel on the side stream (sc_set_band_flag)
  bool band_flagged = false;  // the pending band is announced by the flag (k_wait_band), not by ev_band
  int band_epoch = 0;
  hipEvent_t ev_band = nullptr, ev_xchg = nullptr;
  DevBuf<int> cellCount, cellStart, sortedStamp;
  DevBuf<unsigned long long> scanDesc;  // the bucket scan's look-back descriptors, one per 2048 cells (k_scan_cells)
  unsigned scanStamp = 0;               // ... and the stamp of its last launch
  int scan_max_polls = kScanMaxPolls;   // ... and how often a workgroup asks for a predecessor's total before it gives up (sc_set_scan_patience)
  DevBuf<int2> sortTasks;  // k_sort_big's task list (cell, chunk | length): the scan writes it
  bool piles_now = false;  // the hint "big buckets exist", latched once per tick (sc_step_begin)
  RcclComm comm = nullptr;  // RCCL communicator of the slab chain (sc_comm_init), or null
  int comm_rank = -1, comm_world = 0;
  double *haloL = nullptr, *haloR = nullptr;  // send buffers of the last sc_halo_pack (caller-owned device memory)
  int haloCap = 0;
  int64_t halo_ring_from = 0;  // first tick whose halo counts in the progress block belong to the current state
  int64_t live_hint_from = 0;  // the live count the device publishes is usable once a tick >= this one has finished
  DevBuf<RngState> rng;        // NumPy's MT19937 stream on the device (sc_rng_set_state), or empty
  DevBuf<double> monitor;      // force monitor: sum of |dv| per phase and the particle count (sc_enable_force_monitor)
  bool monitor_on = false;
  // the probe (sc_probe.h): the workgroups' partial records, its own words (ticket, log head, dropped ticks), the row and
  // profile of sc_probe_now, and the log of sc_probe_enable -- rows, bin counts and the bins' tops as 64-bit keys
  DevBuf<double> probePartials, probeNowRow, probeRows;
  DevBuf<int> probeWords, probeNowCounts, probeCounts;
  DevBuf<unsigned long long> probeNowTops, probeTops;
  bool probe_on = false;
  int64_t probe_cap = 0, probe_tail = 0;  // ... its capacity in rows, and the first row not yet delivered
  int probe_bins = 0;
  double probe_x0 = 0.0, probe_x1 = 1.0;
  // tracking (sc_track.h): the frame of sc_track_capture, the log of sc_track_enable with its words (byte cursor, frames,
  // dropped frames, and where the frame being packed starts), and the frame sc_track_load unpacks
  DevBuf<unsigned char> trackNow, trackLog, trackLoad;
  DevBuf<unsigned long long> trackWords;
  bool track_on = false;
  int64_t track_every = 1, track_cap = 0;  // ... every how many ticks a frame is logged, and the log's capacity in bytes
  // checkpoint (sc_checkpoint_begin / _finish): device-side snapshot, pinned host copy, side stream
  DevBuf<double> snap_d[4];
  DevBuf<int> snap_id_d;
  DevBuf<RngState> snap_rng_d;
  HostBuf<double> snap_h[4];
  HostBuf<int> snap_id_h;
  HostBuf<int> snap_counters_h;  // C_COUNT counters
  HostBuf<RngState> snap_rng_h;
  int64_t snap_n_bound = 0, snap_tick = -1;
  bool snap_has_rng = false, snap_pending = false;
  hipStream_t side_stream = nullptr;
  hipEvent_t snap_ready = nullptr, snap_done = nullptr;
  DevBuf<int> colHist;  // sc_column_histogram
  // sc_render: the per-pixel key buffer and (host path) the device frame, grown to the largest frame asked for
  DevBuf<unsigned long long> renderKeys;
  DevBuf<unsigned char> renderRgb;
  // sc_jpeg_encode_device: the encoder's workspace (coefficients, per-block masks and code lengths, the rows' bit
  // buffers, lengths and offsets; sc_jpeg.h) and the entropy-coded data, each grown to the largest frame asked for
  DevBuf<unsigned char> jpegWork, jpegOut;
  // sc_gif_encode_device: the encoder's workspace (the chunks' codes, counts and bit offsets; sc_gif.h) and the image
  // data, and sc_render_gif's frame of palette indices, each grown to the largest frame asked for
  DevBuf<unsigned char> gifWork, gifIndex;
  DevBuf<unsigned> gifOut;
  // sc_set_hud: the text every rendered frame carries and its lines' (start, length); hud_lines == 0: no HUD
  DevBuf<unsigned char> hudText;
  DevBuf<HudLine> hudLines;
  int hud_lines = 0, hud_longest = 0;  // ... how many lines, and the bytes of the longest
  int hud_x = 0, hud_y = 0, hud_scale = 1;
  // sc_set_arrows: the arrows every rendered frame carries; SC_ARROWS_OFF: none
  DevBuf<sc_arrow> arrowList;
  int arrow_mode = SC_ARROWS_OFF;
  int64_t arrow_n = 0, arrow_every = 1;  // ... the list's length; velocity mode: ids that are multiples of this
  double arrow_scale = 1.0;
  // sc_export_state_device (sc_state.h): the sort of the (id, slot) pairs, grown to the launch bound asked for;
  // sc_import_state_device: the ids as 32-bit values and its two words (largest id plus one, out-of-range flag)
  RadixSpace stateSort;
  DevBuf<int> stateIds, stateWords;
  // sc_pairs_count_device / sc_pairs_fill_device (sc_pairs.h): the points in index order, the binning sort of the
  // (bucket, index) pairs -- a workspace of its own: the fill reads its result, and an export may come in between --,
  // the buckets' counts and starts, the members' positions and cells in bucket order, the row lengths, their 64-bit scan
  // with its block sums, the domain flag and the two words (n, E); each grown to the largest bound asked for.
  // `pairs_valid`: the workspace holds the grid of a count, and nothing has changed the state since.
  DevBuf<XY> pairsXY, pairsSXY;
  DevBuf<uint2> pairsCell;
  RadixSpace pairsSort;
  DevBuf<int> pairsBucketCount, pairsBucketStart, pairsBucketSums;
  DevBuf<int> pairsRowLen, pairsFlag;
  DevBuf<long long> pairsOffs, pairsSums, pairsWords;
  bool pairs_valid = false;
  int64_t pairs_m = 0;   // ... the bound its launches were sized by
  int pairs_set = 0;     // ... which of pairsSort's two sets holds the sorted pairs
  PairsGrid pairs_grid{};
  // sc_pairs_label_device (sc_clusters.h): the parents, the root marks, their scan (the dense numbers) with its block sums
  // and the clusters' sizes -- apart from the pairs workspace, which a fill after the labelling still reads; each grown to
  // the largest bound asked for
  DevBuf<int> clusterParent, clusterIsRoot, clusterSize, clusterSums, clusterDense;
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
  bool in_step = false;
  int64_t normals_valid = 0;
  bool custom_grid = false;  // sc_neighbor_search: grid from the data, no walls, no removal
  long long grid_row0 = 0, grid_col0 = 0;
  int grid_nrows = 0, grid_ncols = 0;
  double custom_d = 0;
  bool slab = false;
  long long own_lo = 0, own_hi = 0;
  int slab_axis = 0;  // 0: slabs of columns (x), 1: of rows (y)
  int halo = 0, has_left = 0, has_right = 0;
  std::vector<int> ids_host;
  int64_t stats_live = -1;  // live count read by sc_step_stats inside the current tick, or -1
  DevBuf<int> owned_out;
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
};

namespace {

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

// In slab mode the stored count changes on the device every tick (halo records arrive without the
// host knowing how many), so launches cover the capacity; surplus workgroups exit on their first load.
int64_t launch_bound(const sc_ctx* c);
int probe_launch(sc_ctx* c, bool to_log);
int track_launch(sc_ctx* c, bool to_log);

// A slot of the progress block as the device last wrote it (no synchronisation: possibly stale).
int progress_read(const sc_ctx* c, int slot) { return ((const volatile int*)c->progress.get())[slot]; }

// Waits until the device has published `ticks` finished ticks, or until nothing is queued on the stream any more (the
// counter is then simply behind: a re-upload or a restore).
int wait_ticks_finished(sc_ctx* c, int64_t ticks, const char* what) {
  int spins = 0;
  while (progress_read(c, kProgressTicks) < ticks) {
    if (++spins > 64) {
      const hipError_t q = hipStreamQuery(c->stream);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) return fail(SC_ERR_HIP, "stream error while waiting for %s: %s", what, hipGetErrorString(q));
      spins = 0;
    }
    sched_yield();
  }
  return SC_OK;
}

// Checks and converts a tick's walls and bodies.  `with_pads`: the padded twins come too (sc_set_segments); a promised
// tick has none (sc_set_next_inputs).
int load_walls(TickInputs& in, const double* segments, const double* padded, bool with_pads, int ns, const sc_body* bodies,
               int nb) {
  if (ns < 0 || ns > kMaxSeg) return fail(SC_ERR_CAPACITY, "%d segments, at most %d", ns, kMaxSeg);
  if (nb < 0 || nb > kMaxBody) return fail(SC_ERR_CAPACITY, "%d bodies, at most %d", nb, kMaxBody);
  if (ns > 0 && (!segments || (with_pads && !padded)))
    return fail(SC_ERR_ARG, with_pads ? "null segment arrays" : "null segment array");
  int total = 0;
  for (int b = 0; b < nb; ++b) total += bodies[b].n_segments;
  if (nb > 0 && total != ns) return fail(SC_ERR_ARG, "bodies own %d segments, %d given", total, ns);
  in.nseg = ns;
  in.nbody = nb;
  std::memset(in.seg, 0, sizeof in.seg);
  std::memset(in.pad, 0, sizeof in.pad);
  std::memset(in.body, 0, sizeof in.body);
  for (int k = 0; k < ns; ++k) in.seg[k] = Seg{segments[4 * k], segments[4 * k + 1], segments[4 * k + 2], segments[4 * k + 3]};
  for (int k = 0; k < 2 * ns && with_pads; ++k)
    in.pad[k] = Seg{padded[4 * k], padded[4 * k + 1], padded[4 * k + 2], padded[4 * k + 3]};
  for (int b = 0; b < nb; ++b)
    in.body[b] = BodyK{bodies[b].position_x,        bodies[b].position_y, bodies[b].center_velocity_x,
                       bodies[b].center_velocity_y, bodies[b].angular_clockwise_velocity, bodies[b].n_segments, 0};
  return SC_OK;
}

// The promised tick will not run as promised: forget the bucket counts its K1 left, the next tick bins afresh.
int abandon_promise(sc_ctx* c) {
  HIPCHK(hipMemsetAsync(c->cellCount, 0, c->cellCount.bytes(), c->stream));
  c->prebinned = false;
  return SC_OK;
}

// Each group of buffers below is sized by its last member, which grows last: once it has grown, so have the others.

int ensure_cells(sc_ctx* c, int64_t ncells) {
  if (ncells + 1 <= c->cellCount.size()) return SC_OK;
  if (ncells > (int64_t)1 << 28) return fail(SC_ERR_CAPACITY, "cell grid of %lld cells is too large", (long long)ncells);
  const int64_t n = ncells + 1 + ncells / 4;
  HIPCHK(c->cellStart.grow(n + 1, c->stream));
  HIPCHK(c->scanDesc.grow(n / kScanPerBlock + 4, c->stream));
  HIPCHK(hipMemsetAsync(c->scanDesc, 0, c->scanDesc.bytes(), c->stream));  // stamp 0: never launched
  HIPCHK(c->sortedStamp.grow(n, c->stream));
  HIPCHK(hipMemsetAsync(c->sortedStamp, 0, c->sortedStamp.bytes(), c->stream));
  HIPCHK(c->cellCount.grow(n, c->stream));
  HIPCHK(hipMemsetAsync(c->cellCount, 0, c->cellCount.bytes(), c->stream));
  return SC_OK;
}

int ensure_ids(sc_ctx* c, int64_t n) {
  if (n <= c->cntById.size()) return SC_OK;
  const int64_t m = n + n / 2 + 1024;
  HIPCHK(c->offById.grow(m + 1, c->stream));
  HIPCHK(c->idBlockSums.grow(m / kScanPerBlock + 2, c->stream));
  HIPCHK(c->cntById.grow(m, c->stream));
  return SC_OK;
}

int ensure_stage(sc_ctx* c, int64_t n) {
  if (n <= c->stage_ids.size()) return SC_OK;
  const int64_t m = n + n / 2 + 256;
  HIPCHK(c->stage_xy.grow(2 * m, c->stream));
  HIPCHK(c->stage_vxy.grow(2 * m, c->stream));
  HIPCHK(c->stage_ids.grow(m, c->stream));
  return SC_OK;
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

// Kernel-argument block of this tick.  The cell grid covers [-r, 1+r]^2 -- where
// remove_particles (crate.py:152) leaves particles -- plus three cells of margin for the hard wall
// fix, plus a ring of always-empty cells so that c-1 / c+1 / c+-ncols never leave the arrays.
int build_world(sc_ctx* c, World& w, const TickInputs& in, int64_t tick) {
  const sc_params& p = in.params;
  std::memset(&w, 0, sizeof w);
  const double inf = std::numeric_limits<double>::infinity();
  if (c->custom_grid) {
    w.d = c->custom_d;
    w.r = w.d / 2;
    w.lo = -inf;
    w.hi = inf;
    w.row0 = c->grid_row0;
    w.col0 = c->grid_col0;
    w.nrows = c->grid_nrows;
    w.ncols = c->grid_ncols;
    w.t_nbr = sq_threshold(w.d);
    w.t_wall = -1.0;
    w.far_box = w.touch_box = -1.0;
    w.ccd_skip2 = inf;
  } else {
    if (!(p.particle_radius > 0) || !std::isfinite(p.particle_radius))
      return fail(SC_ERR_ARG, "particle_radius must be positive and finite");
    w.dt = p.dt;
    w.r = p.particle_radius;
    w.d = p.particle_radius * 2;  // crate.py:65-67
    w.decay = p.wall_collision_decay;
    w.pamp = p.pressure_amplifier;
    w.ignored = p.ignored_pressure;
    w.level = p.collider_noise_level;
    w.visc = p.viscosity;
    w.ss = p.surface_smoothing;
    w.tp = p.target_pressure;
    w.gx = p.gravity_x;
    w.gy = p.gravity_y;
    w.lo = -w.r;    // crate.py:152
    w.hi = 1 + w.r;
    w.t_nbr = sq_threshold(w.d);
    double r12 = w.r * 1.2;  // crate.py:229
    w.t_wall = sq_threshold(r12);
    w.touch_box = r12 * (1 + 1e-6) + 1e-12;
    w.far_box = (w.r + 2 * w.d) * (1 + 1e-6) + 1e-12;
    w.ccd_skip2 = (2 * w.d) * (2 * w.d) * (1 - 1e-6);
    long long cmin = (long long)std::floor(w.lo / w.d) - 3;
    long long cmax = (long long)std::floor(w.hi / w.d) + 3;
    // slabs keep a local grid: the slab, its ghost band, one column / row of slack for the wall fix
    long long ccmin = cmin, ccmax = cmax, rrmin = cmin, rrmax = cmax;
    if (c->slab) {
      long long& lo = c->slab_axis ? rrmin : ccmin;
      long long& hi = c->slab_axis ? rrmax : ccmax;
      lo = std::max(cmin, c->own_lo - c->halo - 1);
      hi = std::min(cmax, c->own_hi + c->halo);
      if (hi < lo) hi = lo;
    }
    w.row0 = rrmin - 1;
    w.nrows = (int)(rrmax - rrmin + 1) + 2;
    w.col0 = ccmin - 1;
    w.ncols = (int)(ccmax - ccmin + 1) + 2;
  }
  w.inv_d = 1.0 / w.d;
  // With dx = fl(x_j - x_i), |dx| < d (1 - 2^-20) puts the true difference below d (1 - 2^-21); fl(x +- d) is off by at most
  // |x +- d| 2^-53 <= d 2^-21 as long as |x| / d < 2^32: then x_j is inside [fl(x_i - d), fl(x_i + d)] and x_i inside
  // [fl(x_j - d), fl(x_j + d)] -- both forms of the reference's window (collision_detector.py:106-119, :85-88) hold.
  {
    const long long far = std::max(std::llabs(w.col0), std::llabs(w.col0 + w.ncols)) + 2;
    const long long far_r = std::max(std::llabs(w.row0), std::llabs(w.row0 + w.nrows)) + 2;
    w.dsafe = std::max(far, far_r) < (1LL << 30) ? w.d * (1.0 - 0x1p-20) : 0.0;
  }
  w.row0d = (double)w.row0;
  w.col0d = (double)w.col0;
  w.eta_scale = (w.d * w.level) * (1.0 / 4294967296.0);
  w.eta_half = (w.d * w.level) * 0.5;
  w.k_ss = w.dt * w.ss;
  w.k_pp = w.dt * (1 + w.pamp);
  w.k_0 = -2 * w.tp * w.dt;
  w.dt_gx = w.dt * w.gx;
  w.dt_gy = w.dt * w.gy;
  w.dt_visc = w.dt * w.visc;
  w.dt_pamp = w.dt * w.pamp;
  w.nseg = in.nseg;
  w.nbody = in.nbody;
  std::memcpy(w.seg, in.seg, sizeof w.seg);
  std::memcpy(w.pad, in.pad, sizeof w.pad);
  std::memcpy(w.body, in.body, sizeof w.body);
  w.noise_mode = c->noise_mode;
  w.tick = (int)tick;
  w.noise_key = mix64(c->seed + (uint64_t)(tick + 1) * kGold);
  w.slab = c->slab ? 1 : 0;
  w.slab_axis = c->slab ? c->slab_axis : 0;
  w.band_margin = w.slab_axis ? kBandMarginRows : kBandMarginColumns;
  w.own_lo = c->slab ? c->own_lo : std::numeric_limits<long long>::min();
  w.own_hi = c->slab ? c->own_hi : std::numeric_limits<long long>::max();
  w.halo = c->halo;
  {  // where the particles are expected to end: for slabs a recent tick's live count (blocks beyond it are placed one by one)
    const int64_t done = progress_read(c, kProgressTicks), published = progress_read(c, kProgressLive);
    const int64_t bound = launch_bound(c);
    w.live_hint = (int)(c->slab && published > 0 && done > c->live_hint_from
                            ? std::min<int64_t>(bound, (int64_t)published + 2048)
                            : bound);
  }
  w.has_left = c->has_left;
  w.has_right = c->has_right;
  return SC_OK;
}

int make_world(sc_ctx* c) {
  if (!c->custom_grid && !c->have_params) return fail(SC_ERR_STATE, "sc_set_params has not been called");
  int rc = build_world(c, c->w, c->now, c->tick);
  if (rc) return rc;
  return ensure_cells(c, (int64_t)c->w.nrows * c->w.ncols);
}

// the part of a tick's inputs that K1 reads (see WallInputs)
WallInputs wall_inputs_of(const World& w) {
  WallInputs k;
  std::memset(&k, 0, sizeof k);
  k.r = w.r; k.d = w.d; k.inv_d = w.inv_d; k.lo = w.lo; k.hi = w.hi; k.t_wall = w.t_wall; k.touch_box = w.touch_box; k.far_box = w.far_box;
  k.row0 = w.row0; k.col0 = w.col0; k.row0d = w.row0d; k.col0d = w.col0d; k.own_lo = w.own_lo; k.own_hi = w.own_hi;
  k.nrows = w.nrows; k.ncols = w.ncols; k.nseg = w.nseg; k.nbody = w.nbody; k.slab = w.slab; k.slab_axis = w.slab_axis;
  k.halo = w.halo; k.has_left = w.has_left; k.has_right = w.has_right;
  std::memcpy(k.seg, w.seg, sizeof k.seg);
  std::memcpy(k.body, w.body, sizeof k.body);
  return k;
}


int read_counters(sc_ctx* c, int* out) {
  HIPCHK(hipMemcpyAsync(out, c->counters, C_COUNT * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return SC_OK;
}

int check_flags(int flags) {
  if (flags & F_NAN)
    return fail(SC_ERR_DOMAIN, "a particle position became NaN (zero distance to a wall, crate.py:206); it was dropped");
  if (flags & F_OUT_OF_GRID) return fail(SC_ERR_DOMAIN, "a particle left the cell grid; it was dropped");
  if (flags & F_HALO_OVERFLOW) return fail(SC_ERR_CAPACITY, "a halo buffer was too small; ghost particles were lost");
  if (flags & F_CAPACITY) return fail(SC_ERR_CAPACITY, "received halo particles exceed the context capacity");
  if (flags & F_BAND_TIMEOUT)
    return fail(SC_ERR_HIP, "the halo exchange waited 50 ms for the band blocks of the force kernel and gave up");
  if (flags & F_SCAN_TIMEOUT)
    return fail(SC_ERR_HIP, "the bucket scan waited for a workgroup that never published its total and gave up; the tick was "
                "skipped (the particles are as the tick found them)");
  if (flags & F_HALO_LATE)
    return fail(SC_ERR_DOMAIN, "a particle moved more than the band margin (%d columns / %d rows) in one tick and missed the "
                "overlapped halo message: run without halo overlap", kBandMarginColumns, kBandMarginRows);
  if (flags & F_HALO_CROSSED)
    return fail(SC_ERR_DOMAIN, "a particle crossed a whole slab in one tick: the slab it is in now never received it; it was "
                "dropped (use fewer, wider slabs or a shorter dt)");
  if (flags & F_HALO_REACH)
    return fail(SC_ERR_DOMAIN, "the hard wall fix moved a particle next to a slab cut by more than one radius along the slab "
                "axis (several wall contacts at once, as at a joint of two segments): the ghost band of three columns / rows "
                "may not have reached all it needs; place the cuts away from such joints");
  return SC_OK;
}

// What every reader of the error bits does with them (sc_synchronize, sc_download_state; `h`: the counters as read):
// they are cleared on the stream and reported, once.  A tick abandoned behind its scan (F_SCAN_TIMEOUT) -- and every tick
// queued behind it, which the flag abandoned too -- has left more than the flag, and all of it is put right here, so that
// the next tick starts from the storage arrays whichever call came first:
//   cellCount   holds the counts of the abandoned tick's K1, which no scatter took back; a look-ahead may have promised
//               a K1 that pass B never ran (abandon_promise)
//   C_NBIG / C_NTASKS   pass B zeroes them, and returned before it did: every abandoned scan added its buckets and
//               appended its tasks, which k_sort_big would run beside the next tick's
//   C_NT        is the partial sum of a workgroup that gave up; between ticks it says which slots have a pressure, and
//               goes back to what the last finished tick left (C_NT_DONE: C_NS, unless particles were appended since;
//               0 after an upload, whatever normals_valid says -- sc_step_finish sets it for an abandoned tick too)
// Inside a tick (sc_synchronize between sc_step_begin and sc_step_finish) the bit stays up: the rest of the tick must
// not run on what the scan left, so it is reported now and again -- with the repair -- by the first reader after the tick.
int recover_flags(sc_ctx* c, const int* h) {
  const int flags = h[C_FLAGS];
  if (!flags) return SC_OK;
  const bool abandoned = (flags & F_SCAN_TIMEOUT) != 0;
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(c->counters + C_FLAGS), abandoned && c->in_step ? F_SCAN_TIMEOUT : 0, 1, c->stream));
  if (abandoned && !c->in_step) {
    const int rc = abandon_promise(c);
    if (rc) return rc;
    static_assert(C_NTASKS == C_NBIG + 1, "one memset for the two");
    HIPCHK(hipMemsetAsync(c->counters + C_NBIG, 0, 2 * sizeof(int), c->stream));
    HIPCHK(hipMemcpyAsync(c->counters + C_NT, c->counters + C_NT_DONE, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  }
  return check_flags(flags);
}

// What every upload and append starts with: the call is allowed and the particles fit; a reset gives up a promised tick.
int put_check(sc_ctx* c, const void* xy, const void* vxy, int64_t n, bool reset) {
  if (n < 0 || (n > 0 && (!xy || !vxy))) return fail(SC_ERR_ARG, "bad particle arrays");
  if (c->in_step) return fail(SC_ERR_STATE, "particles cannot change between sc_step_begin and sc_step_finish");
  if (c->prebinned && !reset)
    return fail(SC_ERR_STATE, "particles cannot be appended after sc_set_next_inputs promised the next tick");
  const int64_t base = reset ? 0 : c->upper;
  if (base + n > c->cap)
    return fail(SC_ERR_CAPACITY, "%lld particles exceed the context capacity %lld", (long long)(base + n), (long long)c->cap);
  if ((reset ? 0 : c->next_id) + n > std::numeric_limits<int>::max()) return fail(SC_ERR_CAPACITY, "particle ids exhausted");
  return SC_OK;
}

// ... and ends with: n particles in DEVICE memory (P x 2 interleaved; ids 32-bit with their largest, or null: the next
// ids) go behind the stored ones, or replace them.  After put_check.
int put_from_device(sc_ctx* c, const double* dev_xy, const double* dev_vxy, const int* dev_ids, int64_t max_id, int64_t n,
                    bool reset) {
  if (c->prebinned && reset) {
    const int rc = abandon_promise(c);
    if (rc) return rc;
  }
  const int64_t base = reset ? 0 : c->upper;
  c->pairs_valid = false;
  if (reset) {
    c->next_id = 0;
    c->normals_valid = 0;
    c->halo_ring_from = c->tick;  // counts published before this belong to another state
  }
  if (n > 0) {
    if (dev_ids) c->next_id = std::max<int64_t>(c->next_id, max_id + 1 - n);
    Bracket br(c, K_APPEND);
    hipLaunchKernelGGL(k_append, dim3(grid_for(n)), dim3(kBlock), 0, c->stream, dev_xy, dev_vxy, (int)n, (int)c->next_id,
                       dev_ids, c->counters, c->x, c->y, c->vx, c->vy, c->id[0], reset ? 1 : 0, (int)c->cap);
  }
  c->upper = base + n;
  c->next_id += n;
  c->live_hint_from = c->tick;  // counts published by earlier ticks do not include these particles
  hipLaunchKernelGGL(k_bump, dim3(1), dim3(1), 0, c->stream, c->counters, (int)n, reset ? 1 : 0, (int)c->next_id, (int)c->cap);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

int put_particles(sc_ctx* c, const double* xy, const double* vxy, int64_t n, bool reset, const int64_t* ids = nullptr) {
  int rc = put_check(c, xy, vxy, n, reset);
  if (rc) return rc;
  int* dev_ids = nullptr;
  int64_t max_id = -1;
  if (n > 0) {
    if ((rc = ensure_stage(c, n))) return rc;
    std::vector<int>& ids32 = c->ids_host;  // outlives the asynchronous copy below
    if (ids) {
      HIPCHK(hipStreamSynchronize(c->stream));  // an earlier copy out of ids_host has finished
      ids32.resize(n);
      for (int64_t k = 0; k < n; ++k) {
        if (ids[k] < 0 || ids[k] > std::numeric_limits<int>::max() - 1) return fail(SC_ERR_ARG, "particle id out of range");
        ids32[k] = (int)ids[k];
        max_id = std::max<int64_t>(max_id, ids[k]);
      }
      dev_ids = c->stage_ids;  // room for n ids (ensure_stage)
      HIPCHK(hipMemcpyAsync(dev_ids, ids32.data(), n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipMemcpyAsync(c->stage_xy, xy, 2 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->stage_vxy, vxy, 2 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  return put_from_device(c, c->stage_xy, c->stage_vxy, dev_ids, max_id, n, reset);
}

int64_t launch_bound(const sc_ctx* c) { return c->slab ? c->cap : c->upper; }

int tile_grid(const sc_ctx* c) { return (int)std::max<int64_t>(1, (launch_bound(c) + kTileW - 1) / kTileW); }

// neighbor search (+ pass A unless the host's noise block has to be indexed first)
bool piles_expected(const sc_ctx* c);

template <int NOISE, bool ENUM, bool DENS, int CAP>
void launch_pass_a_cap(sc_ctx* c) {
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(tile_grid(c)), dim3(kTileW), 0, c->stream, c->w, c->counters,
                       c->sxy, c->id[1], c->cellT, Buckets{c->cellStart}, c->nbr, c->rows, (int)c->cap, c->eta, c->offById,
                       c->P, c->snn, ENUM ? c->tileBounds : c->tileBoundsT, c->tileBand, c->tileBoundsT);
  };
  if (ENUM && DENS && piles_expected(c))  // dense tiles ahead: the instantiation that stages their lists' reach
    launch(k_pass_a<NOISE, ENUM, DENS, CAP, ENUM && DENS>);
  else
    launch(k_pass_a<NOISE, ENUM, DENS, CAP, false>);
}

template <int NOISE, bool ENUM, bool DENS>
void launch_pass_a(sc_ctx* c, int kernel_id) {
  Bracket br(c, kernel_id);
  // up to 16 waves per CU: all resident with the wide tile too; beyond that the narrow tile's higher
  // occupancy wins (measured with 128-wide tiles: 262,144 particles 35.9 -> 32.2 us wide; 1,048,576: 78 us
  // narrow, 82 us wide)
  // (slabs size their grids by capacity; the live count a recent tick published is the better estimate of the work)
  const int published = progress_read(c, kProgressLive);
  const int tiles = c->slab && published > 0 ? (published + kTileW - 1) / kTileW + 64 : tile_grid(c);
  if (c->tile_choice ? c->tile_choice == 2 : tiles <= (8 * 128 / kTileW) * c->num_cus)
    launch_pass_a_cap<NOISE, ENUM, DENS, kTileCapAWide>(c);
  else
    launch_pass_a_cap<NOISE, ENUM, DENS, kTileCapA>(c);
}

// Big buckets were seen by the last scan the host knows about (an unsynchronised, possibly stale hint in host-mapped
// memory): the tick sorts its big buckets before ranking them and its cell counts group scrambled waves by cell.
// Both only cost time when they are wrong; results do not depend on the choice.
// (latched by sc_step_begin: every launch of a tick sees the same answer -- the sort of the big buckets and the grouping
// variants of scatter, search and force kernel go together)
bool piles_expected(const sc_ctx* c) { return c->piles_now; }

template <int NOISE, bool FUSED, bool MON = false>
void launch_pass_b(sc_ctx* c, const WallInputs& wn, int part = 0) {
  const int cur = (int)(c->tick & 1), nxt = cur ^ 1;
  // slabs of rows: the band blocks lie within (ghost rows + halo + margin) rows of either end of the sorted order; the
  // window takes twice the blocks those rows hold on average (a band block outside it is handled by part 2 and, should
  // it have anything to pack, reported like a particle that was too fast)
  int bandw = 0;
  if (part && c->slab_axis == 1) {
    const int64_t rows = std::max<int64_t>(1, std::min<int64_t>(c->own_hi, c->w.row0 + c->w.nrows) - std::max<int64_t>(c->own_lo, c->w.row0));
    const int64_t band_rows = 2 * c->halo + kBandMarginRows + 2;
    bandw = (int)std::min<int64_t>(tile_grid(c), 2 * band_rows * (c->w.live_hint / rows + 1) / kTileW + 16);
  }
  const int grid = part == 1 && bandw ? 2 * bandw : part == 3 ? tile_grid(c) + 2 * bandw : tile_grid(c);
  hipStream_t stream = c->stream;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kTileW), 0, stream, c->w, c->counters, c->sxy, c->svv,
                       c->id[1], c->wslotT, c->cellT, c->nbr, c->rows, (int)c->cap, c->eta, c->offById, c->P,
                       c->snn, c->wrec[cur], c->x, c->y, c->vx, c->vy, c->id[0], c->tileBoundsT,
                       c->progress_dev, wn, c->cellS, c->wslotS, c->cellCount, c->wrec[nxt], c->haloL, c->haloR, c->haloCap,
                       c->monitor, c->tileBand, part, bandw, c->band_epoch);
  };
  auto pick = [&]() {
    const bool group = FUSED && piles_expected(c);
    if (FUSED && bandw > 0) {  // the instantiation with the band window (slabs of rows, halo overlap)
      if (group)
        launch(k_pass_b<NOISE, FUSED, MON, FUSED, FUSED>);
      else
        launch(k_pass_b<NOISE, FUSED, MON, false, FUSED>);
    } else if (group) {
      launch(k_pass_b<NOISE, FUSED, MON, FUSED>);
    } else {
      launch(k_pass_b<NOISE, FUSED, MON, false>);
    }
  };
  Bracket br(c, K_FORCE);
  pick();
}

template <int NOISE>
void launch_pass_b_any(sc_ctx* c, bool fused, const WallInputs& wn) {
  if (c->monitor_on) {
    launch_pass_b<NOISE, false, true>(c, wn);
  } else if (fused && c->slab && c->overlap && c->haloL && (c->has_left || c->has_right)) {
    // halo overlap: the blocks that may pack halo records first; once they are done (ev_band) the exchange of the
    // coming tick may start on the side stream while the interior blocks run
    if (c->slab_axis == 1 && c->band_by_flag) {
      // slabs of rows: one launch, the window blocks first; the side stream polls for their completion (k_wait_band)
      c->band_epoch += 1;
      launch_pass_b<NOISE, true>(c, wn, 3);
      c->band_flagged = true;
    } else {
      launch_pass_b<NOISE, true>(c, wn, 1);
      (void)hipEventRecord(c->ev_band, c->stream);
      launch_pass_b<NOISE, true>(c, wn, 2);
      c->band_flagged = false;
    }
    c->band_pending = true;
  } else if (fused)
    launch_pass_b<NOISE, true>(c, wn);
  else
    launch_pass_b<NOISE, false>(c, wn);
}

// ---- the probe (sc_probe.h) ---------------------------------------------------------------------

int probe_check_bins(int32_t n_bins, double x0, double x1) {
  if (n_bins < 0 || n_bins > kProbeMaxBins) return fail(SC_ERR_ARG, "%d bins; 0..%d", n_bins, kProbeMaxBins);
  if (n_bins > 0 && !(std::isfinite(x0) && std::isfinite(x1) && x1 > x0))
    return fail(SC_ERR_ARG, "the profile's range must be finite with x1 > x0");
  return SC_OK;
}

int probe_ensure(sc_ctx* c) {
  if (c->probeWords.size() >= PW_COUNT) return SC_OK;
  HIPCHK(c->probePartials.grow((int64_t)kProbeBlocks * kProbeFields, c->stream));
  HIPCHK(c->probeNowRow.grow(kProbeFields, c->stream));
  HIPCHK(c->probeNowCounts.grow(kProbeMaxBins, c->stream));
  HIPCHK(c->probeNowTops.grow(kProbeMaxBins, c->stream));
  HIPCHK(c->probeWords.grow(PW_COUNT, c->stream));
  HIPCHK(hipMemsetAsync(c->probeWords, 0, c->probeWords.bytes(), c->stream));
  return SC_OK;
}

// Enqueues one measurement: into the log's next row (`to_log`; the device decides which, or that the log is full), or
// into the row and profile of sc_probe_now with the bins given.
int probe_launch(sc_ctx* c, bool to_log, int n_bins, double x0, double x1) {
  ProbeArgs a{};
  a.nbins = n_bins;
  a.x0 = x0;
  a.w = n_bins > 0 ? (x1 - x0) / n_bins : 1.0;
  a.tick = (double)c->tick;
  a.pressure_valid = c->normals_valid ? 1 : 0;
  a.cap = (int)c->cap;
  a.log_rows = to_log ? c->probe_cap : -1;
  hipLaunchKernelGGL(k_probe, dim3(kProbeBlocks), dim3(kProbeBlock), 0, c->stream, a, c->counters, c->x, c->y, c->vx, c->vy,
                     c->P, c->probePartials, c->probeWords, to_log ? c->probeRows : c->probeNowRow,
                     to_log ? c->probeCounts : c->probeNowCounts, to_log ? c->probeTops : c->probeNowTops);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

int probe_launch(sc_ctx* c, bool to_log) { return probe_launch(c, to_log, c->probe_bins, c->probe_x0, c->probe_x1); }

// the bins' tops as the kernel keeps them (probe_key; all ones: an empty bin) back to float64
void probe_decode_tops(const unsigned long long* keys, double* tops, int64_t n) {
  for (int64_t k = 0; k < n; ++k) {
    const unsigned long long key = keys[k];
    if (key == kProbeEmptyTop) {
      tops[k] = std::numeric_limits<double>::infinity();
    } else {
      const unsigned long long b = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
      std::memcpy(&tops[k], &b, 8);
    }
  }
}

// ---- tracking (sc_track.h) ----------------------------------------------------------------------

int track_ensure(sc_ctx* c) {
  if (c->trackWords.size() >= TW_COUNT) return SC_OK;
  HIPCHK(c->trackWords.grow(TW_COUNT, c->stream));
  HIPCHK(hipMemsetAsync(c->trackWords, 0, c->trackWords.bytes(), c->stream));
  return SC_OK;
}

// Enqueues one frame of the state as it stands, with the walls the last tick ran with: appended to the log (`to_log`;
// the device decides where, or that it does not fit), or at the start of trackNow, which holds `trackNow.size()` bytes.
int track_launch(sc_ctx* c, bool to_log) {
  TrackArgs a{};
  a.tick = c->tick;
  a.log_bytes = to_log ? c->track_cap : -1;
  a.room = c->trackNow.size();
  a.scale = kTrackCodes / kTrackSpan;
  a.pressure_valid = c->normals_valid ? 1 : 0;
  a.cap = (int)c->cap;
  a.nseg = c->now.nseg;
  std::memcpy(a.seg, c->now.seg, sizeof a.seg);
  unsigned char* base = to_log ? c->trackLog.get() : c->trackNow.get();
  hipLaunchKernelGGL(k_track_reserve, dim3(1), dim3(64), 0, c->stream, a, c->counters, c->trackWords, base);
  const int64_t bound = std::min<int64_t>(launch_bound(c), c->cap);
  const int64_t groups = track_pad8(bound) / kTrackPerThread;
  if (groups > 0)
    hipLaunchKernelGGL(k_track_pack, dim3(grid_for(groups)), dim3(kBlock), 0, c->stream, a, c->counters, c->trackWords, c->x,
                       c->y, c->id[0], c->P, base);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

int track_refuse(const sc_ctx* c, bool switching) {
  if (c->slab) return fail(SC_ERR_STATE, "tracking is not available in slab mode");
  if (c->in_step) return fail(SC_ERR_STATE, switching ? "the track log cannot change inside a tick" : "tracking happens between ticks");
  if (switching && c->prebinned)
    return fail(SC_ERR_STATE, "the track log cannot change after sc_set_next_inputs promised the next tick");
  return SC_OK;
}

}  // namespace

extern "C" {

const char* sc_last_error(void) { return g_err.c_str(); }
int sc_abi_version(void) { return SC_ABI_VERSION; }
const char* sc_kernel_name(int i) { return (i >= 0 && i < SC_NUM_KERNELS) ? kKernelNames[i] : ""; }

int sc_create(int device, int64_t capacity, sc_ctx** out) {
  if (!out || capacity < 1 || capacity > (int64_t)100000000) return fail(SC_ERR_ARG, "bad capacity");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(SC_ERR_ARG, "device %d of %d", device, ndev);
  HIPCHK(hipSetDevice(device));
  sc_ctx* c = new sc_ctx();
  c->device = device;
  c->cap = capacity;
  if (hipDeviceGetAttribute(&c->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->num_cus < 1)
    c->num_cus = 256;
  if (const char* tile = std::getenv("SANDCRATE_TILE"))
    c->tile_choice = !std::strcmp(tile, "narrow") ? 1 : !std::strcmp(tile, "wide") ? 2 : 0;
  const int64_t n = capacity;
  hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
  c->stream = c->own_stream;
  if (e == hipSuccess) e = c->x.grow(n, c->stream);
  if (e == hipSuccess) e = c->y.grow(n, c->stream);
  if (e == hipSuccess) e = c->vx.grow(n, c->stream);
  if (e == hipSuccess) e = c->vy.grow(n, c->stream);
  if (e == hipSuccess) e = c->id[0].grow(n, c->stream);
  if (e == hipSuccess) e = c->id[1].grow(n, c->stream);
  if (e == hipSuccess) e = c->cellS.grow(n, c->stream);
  if (e == hipSuccess) e = c->wslotS.grow(n, c->stream);
  if (e == hipSuccess) e = c->cellT.grow(n, c->stream);
  if (e == hipSuccess) e = c->wslotT.grow(n, c->stream);
  if (e == hipSuccess) e = c->keys.grow(n, c->stream);
  if (e == hipSuccess) e = c->keyCell.grow(n, c->stream);
  if (e == hipSuccess) e = c->tileBounds.grow(6 * (n / kTileW + 2), c->stream);
  if (e == hipSuccess) e = c->tileBoundsT.grow(6 * (n / kTileW + 2), c->stream);
  if (e == hipSuccess) e = c->tileBand.grow(n / kTileW + 2, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->tileBand, 0, c->tileBand.bytes(), c->stream);
  if (e == hipSuccess) e = c->sortTasks.grow(kMaxSortTasks, c->stream);
  if (e == hipSuccess) e = c->progress.grow(kProgressInts, c->stream);
  if (e == hipSuccess) {
    std::fill_n(c->progress.get(), kProgressInts, 0);
    e = hipHostGetDevicePointer((void**)&c->progress_dev, c->progress, 0);
  }
  if (e == hipSuccess) e = c->wrec[0].grow(5 * n, c->stream);
  if (e == hipSuccess) e = c->wrec[1].grow(5 * n, c->stream);
  if (e == hipSuccess) e = c->nbr.grow(kMaxNbr * n, c->stream);
  if (e == hipSuccess) e = c->rows.grow(n, c->stream);
  if (e == hipSuccess) e = c->P.grow(n, c->stream);
  if (e == hipSuccess) e = c->snn.grow(n, c->stream);
  if (e == hipSuccess) e = c->sxy.grow(n, c->stream);
  if (e == hipSuccess) e = c->svv.grow(n, c->stream);
  if (e == hipSuccess) e = c->counters.grow(C_ALLOC, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->counters, 0, c->counters.bytes(), c->stream);
  if (e != hipSuccess) {
    int rc = fail(SC_ERR_HIP, "sc_create: %s", hipGetErrorString(e));
    sc_destroy(c);
    return rc;
  }
  *out = c;
  return SC_OK;
}

int sc_destroy(sc_ctx* c) {
  if (!c) return SC_OK;
  (void)hipSetDevice(c->device);
  if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
  if (c->comm) (void)sc_comm_destroy(c);
  if (c->ev_band) (void)hipEventDestroy(c->ev_band);
  if (c->ev_xchg) (void)hipEventDestroy(c->ev_xchg);
  for (auto& v : {c->ev_used, c->ev_free})
    for (auto& e : v) {
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
  if (c->snap_ready) (void)hipEventDestroy(c->snap_ready);
  if (c->snap_done) (void)hipEventDestroy(c->snap_done);
  if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;  // frees the buffers
  return SC_OK;
}

int sc_set_stream(sc_ctx* c, void* s) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  HIPCHK(hipStreamSynchronize(c->stream));
  c->stream = (hipStream_t)s;
  return SC_OK;
}

int sc_use_own_stream(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  HIPCHK(hipStreamSynchronize(c->stream));
  c->stream = c->own_stream;
  return SC_OK;
}

int sc_upload_state(sc_ctx* c, const double* xy, const double* vxy, int64_t n) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  HIPCHK(hipSetDevice(c->device));
  return put_particles(c, xy, vxy, n, true);
}

int sc_append_particles(sc_ctx* c, const double* xy, const double* vxy, int64_t n) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  HIPCHK(hipSetDevice(c->device));
  return put_particles(c, xy, vxy, n, false);
}

int sc_synchronize(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  int h[C_COUNT];
  int rc = read_counters(c, h);
  if (rc) return rc;
  if (!c->in_step) c->upper = h[C_NS];
  return recover_flags(c, h);
}

int sc_set_scan_patience(sc_ctx* c, int64_t polls) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  c->scan_max_polls = polls < 0 ? -1 : (int)std::min<int64_t>(polls, kScanMaxPolls);
  return SC_OK;
}

int sc_count(sc_ctx* c, int64_t* n) {
  if (!c || !n) return fail(SC_ERR_ARG, "null argument");
  int h[C_COUNT];
  int rc = read_counters(c, h);
  if (rc) return rc;
  *n = c->in_step ? h[C_NT] : h[C_NS];
  if (!c->in_step) c->upper = h[C_NS];
  return SC_OK;
}

int sc_set_params(sc_ctx* c, const sc_params* p) {
  if (!c || !p) return fail(SC_ERR_ARG, "null argument");
  if (c->in_step) return fail(SC_ERR_STATE, "coefficients cannot change inside a tick");
  c->now.params = *p;
  c->have_params = true;
  return SC_OK;
}

int sc_set_segments(sc_ctx* c, const double* segments, const double* padded, int32_t ns, const sc_body* bodies,
                    int32_t nb) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "segments cannot change inside a tick");
  return load_walls(c->now, segments, padded, true, ns, bodies, nb);
}

int sc_set_noise_mode(sc_ctx* c, int mode, uint64_t seed) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (mode < SC_NOISE_NONE || mode > SC_NOISE_COUNTER) return fail(SC_ERR_ARG, "noise mode %d", mode);
  if (c->in_step) return fail(SC_ERR_STATE, "noise mode cannot change inside a tick");
  c->noise_mode = mode;
  c->seed = seed;
  return SC_OK;
}

// host-noise mode: every particle's offset into the tick's rand(sum C_i, 2) block (crate.py:165-170 draws in id order)
static int launch_noise_offsets(sc_ctx* c) {
  Bracket br(c, K_NOISE_OFFSETS);
  HIPCHK(hipMemsetAsync(c->cntById, 0, c->next_id * sizeof(int), c->stream));
  hipLaunchKernelGGL(k_count_by_id, dim3(grid_for(launch_bound(c))), dim3(kBlock), 0, c->stream, c->counters, c->id[1],
                     (const unsigned int*)c->rows.get(), c->cntById);
  return launch_scan(c, c->cntById, c->offById, c->next_id, c->idBlockSums, nullptr);
}

int sc_step_begin(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_step_begin called twice");
  if (c->slab && c->noise_mode == SC_NOISE_HOST) return fail(SC_ERR_STATE, "SC_NOISE_HOST is not available in slab mode");
  HIPCHK(hipSetDevice(c->device));
  // Keep at most kMaxTicksQueued ticks of launches in flight.  The GPU publishes the number of
  // finished ticks in host-mapped memory (pass B); nothing else is needed to know how far ahead the
  // host is, and a bounded queue keeps per-tick hints (big buckets) at most that many ticks stale.
  constexpr int64_t kMaxTicksQueued = 4;
  if (!c->custom_grid) {
    const int rc = wait_ticks_finished(c, c->tick - kMaxTicksQueued, "queued ticks");
    if (rc) return rc;
  }
  int rc = make_world(c);
  if (rc) return rc;
  c->pairs_valid = false;
  const World& w = c->w;
  int grid = grid_for(launch_bound(c));
  int cap = (int)c->cap;
  // big buckets were seen by the last scan the host knows about (an unsynchronised, possibly stale hint in host-mapped
  // memory), read ONCE per tick
  c->piles_now = c->force_rank_big || progress_read(c, kProgressBigBuckets) > 0;
  if (c->prebinned) {
    // the previous sc_step_finish ran K1 of this tick with the promised inputs: they must be the inputs
    const WallInputs now = wall_inputs_of(w);
    if (std::memcmp(&now, &c->promised, sizeof now) != 0)
      return fail(SC_ERR_STATE, "this tick's coefficients / segments differ from what sc_set_next_inputs promised");
    c->prebinned = false;
  } else {
    Bracket br(c, K_WALL_BIN);
    hipLaunchKernelGGL(k_wall_bin, dim3(grid), dim3(kBlock), 0, c->stream, w, c->counters, c->x, c->y, c->cellS,
                       c->wslotS, c->cellCount, c->wrec[c->tick & 1], cap);
  }
  {
    Bracket br(c, K_SCAN);
    const int64_t ncells = (int64_t)w.nrows * w.ncols;
    const int nb = (int)((ncells + 1 + kScanPerBlock - 1) / kScanPerBlock);  // covers the one-past-the-end entry
    c->scanStamp = c->scanStamp % 0x3FFFFFFFu + 1;  // 1 .. 2^30 - 1: never the cleared descriptors' 0
    hipLaunchKernelGGL(k_scan_cells, dim3(nb), dim3(kBlock), 0, c->stream, c->cellCount, c->cellStart, (int)ncells,
                       c->scanDesc, c->scanStamp, c->counters, c->sortTasks, c->scan_max_polls);
  }
  {
    Bracket br(c, K_SCATTER);
    if (piles_expected(c))
      hipLaunchKernelGGL(k_scatter<true>, dim3(grid), dim3(kBlock), 0, c->stream, c->counters, c->cellS, c->x,
                         c->id[0], Buckets{c->cellStart}, c->cellCount, c->keys, c->keyCell, cap, w.live_hint);
    else
      hipLaunchKernelGGL(k_scatter<false>, dim3(grid), dim3(kBlock), 0, c->stream, c->counters, c->cellS, c->x,
                         c->id[0], Buckets{c->cellStart}, c->cellCount, c->keys, c->keyCell, cap, w.live_hint);
  }
  const int stamp = (int)((c->tick + 1) & 0x3FFFFFFF);
  // big buckets were seen by the last scan the host knows about (an unsynchronised, possibly stale
  // hint in host-mapped memory): rank this tick's big buckets over the whole GPU first
  if (piles_expected(c)) {
    Bracket br(c, K_SCAN);
    hipLaunchKernelGGL(k_sort_big, dim3(kSortGridPerCu * c->num_cus), dim3(kSortBlock), 0, c->stream, c->counters, c->sortTasks,
                       Buckets{c->cellStart}, c->keys, c->sortedStamp, stamp);
  }
  {
    Bracket br(c, K_REORDER);
    hipLaunchKernelGGL(k_reorder, dim3((int)std::max<int64_t>(1, (launch_bound(c) + kReorderBlock - 1) / kReorderBlock)),
                       dim3(kReorderBlock), 0, c->stream, c->counters, c->keys, c->keyCell,
                       c->cellS, Buckets{c->cellStart}, c->wslotS, c->y, c->vx, c->vy, c->sxy, c->svv,
                       c->id[1], c->cellT, c->wslotT, c->sortedStamp, stamp, w.ncols, c->tileBounds, w.live_hint, c->progress_dev);
  }
  // SC_NOISE_HOST (and the stand-alone search) stop after the lists: the host's rand block can only be
  // indexed once every count is known.  Otherwise the search and pass A are one launch.
  if (c->noise_mode == SC_NOISE_HOST || c->custom_grid)
    launch_pass_a<SC_NOISE_NONE, true, false>(c, K_NEIGHBORS);
  else if (c->noise_mode == SC_NOISE_COUNTER)
    launch_pass_a<SC_NOISE_COUNTER, true, true>(c, K_PASS_A);
  else
    launch_pass_a<SC_NOISE_NONE, true, true>(c, K_PASS_A);
  c->offsets_pending = false;
  if (c->noise_mode == SC_NOISE_HOST && c->next_id > 0) {
    rc = ensure_ids(c, c->next_id);
    if (rc) return rc;
    // a small world whose stream the device holds: the offsets are taken by the same launch that draws the noise
    // (sc_step_finish: k_rng_noise_small) -- unless the host brings its own block after all (sc_set_noise_host)
    if (c->rng && c->next_id <= kSmallIds)
      c->offsets_pending = true;
    else if ((rc = launch_noise_offsets(c)))
      return rc;
  }
  HIPCHK(hipGetLastError());
  c->in_step = true;
  c->etaPairs = -1;
  c->stats_live = -1;
  return SC_OK;
}

int sc_step_stats(sc_ctx* c, sc_stats* out) {
  if (!c || !out) return fail(SC_ERR_ARG, "null argument");
  if (!c->in_step) return fail(SC_ERR_STATE, "sc_step_stats needs sc_step_begin first");
  hipLaunchKernelGGL(k_count_stats, dim3(1), dim3(kBlock), 0, c->stream, c->counters, (const unsigned int*)c->rows.get(), c->wslotT);
  int h[C_COUNT];
  int rc = read_counters(c, h);
  if (rc) return rc;
  out->flags = h[C_FLAGS];
  out->reserved = 0;
  if (h[C_FLAGS] & F_SCAN_TIMEOUT) {
    // the tick is abandoned: C_NT is a partial sum and the rows counted are an earlier tick's.  The particles are the
    // stored ones, there are no lists, and the host's bound of the stored count is not taken from this tick
    out->particles = h[C_NS];
    out->neighbor_slots = out->max_neighbors = out->wall_particles = 0;
    return SC_OK;
  }
  c->stats_live = h[C_NT];
  out->particles = h[C_NT];
  out->neighbor_slots = (int64_t)(uint32_t)h[C_SUMC] + ((int64_t)h[C_SUMC_HI] << 32);
  out->max_neighbors = h[C_MAXC];
  out->wall_particles = h[C_WREC];
  return SC_OK;
}

int sc_set_noise_host(sc_ctx* c, const double* u01, int64_t n_pairs) {
  if (!c || n_pairs < 0 || (n_pairs > 0 && !u01)) return fail(SC_ERR_ARG, "bad noise array");
  if (!c->in_step) return fail(SC_ERR_STATE, "sc_set_noise_host needs sc_step_begin first");
  if (c->offsets_pending) {  // (the host draws this tick's block itself: the offsets into it are needed after all)
    c->offsets_pending = false;
    int rc = launch_noise_offsets(c);
    if (rc) return rc;
  }
  if (2 * n_pairs > c->eta.size()) HIPCHK(c->eta.grow(2 * (n_pairs + n_pairs / 2 + 1024), c->stream));
  if (n_pairs > 0)
    HIPCHK(hipMemcpyAsync(c->eta, u01, 2 * n_pairs * sizeof(double), hipMemcpyHostToDevice, c->stream));
  c->etaPairs = n_pairs;
  return SC_OK;
}

int sc_step_finish(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!c->in_step) return fail(SC_ERR_STATE, "sc_step_finish needs sc_step_begin first");
  if (c->noise_mode == SC_NOISE_HOST && c->etaPairs < 0) {
    if (!c->rng) return fail(SC_ERR_STATE, "SC_NOISE_HOST: sc_set_noise_host must be called every tick (or sc_rng_set_state once)");
    // the device holds the stream: draw the tick's rand(sum C_i, 2) there; sum C_i is the last entry of the
    // offsets sc_step_begin scanned, so the host never learns it
    HIPCHK(c->eta.grow(2 * kMaxNbr * c->cap, c->stream));
    const long long eta_pairs = c->eta.size() / 2;
    if (c->next_id > 0) {
      Bracket br(c, K_NOISE_OFFSETS);
      if (c->offsets_pending)
        hipLaunchKernelGGL(k_rng_noise_small, dim3(1), dim3(kSmallBlock), 0, c->stream, c->rng, c->id[1], (const unsigned int*)c->rows.get(),
                           (int)c->next_id, c->cntById, c->offById, c->eta, eta_pairs, c->counters);
      else
        hipLaunchKernelGGL(k_rng_noise, dim3(1), dim3(kRngBlock), 0, c->stream, c->rng, c->offById + c->next_id, c->eta,
                           eta_pairs, c->counters);
      c->offsets_pending = false;
    }
    c->etaPairs = 0;
  }
  // look-ahead: run K1 of the next tick in pass B's epilogue.  Slabs: pass B also packs the next halo
  // message into the buffers of the last sc_halo_pack, and sc_halo_unpack does K1 for what it appends.
  WallInputs wn;
  std::memset(&wn, 0, sizeof wn);
  const bool slab_ready = !c->slab || c->haloL || !(c->has_left || c->has_right);
  // (the monitor runs with the plain kernel; the probe's log and the track log record the state sc_download_state
  // stands for, which a fused tick does not leave in the storage arrays)
  const bool fused = c->have_next && slab_ready && !c->custom_grid && !c->monitor_on && !c->probe_on && !c->track_on;
  if (fused) {
    World next;
    int rc = build_world(c, next, c->next, c->tick + 1);
    if (rc) return rc;
    if (next.nrows != c->w.nrows || next.ncols != c->w.ncols) {
      rc = ensure_cells(c, (int64_t)next.nrows * next.ncols);  // the radius changed: the grid may have grown
      if (rc) return rc;
    }
    wn = wall_inputs_of(next);
  }
  c->have_next = false;
  switch (c->noise_mode) {
    case SC_NOISE_HOST:
      launch_pass_a<SC_NOISE_HOST, false, true>(c, K_DENSITY);
      launch_pass_b_any<SC_NOISE_HOST>(c, fused, wn);
      break;
    case SC_NOISE_COUNTER: launch_pass_b_any<SC_NOISE_COUNTER>(c, fused, wn); break;
    default:
      if (c->custom_grid) launch_pass_a<SC_NOISE_NONE, false, true>(c, K_DENSITY);
      launch_pass_b_any<SC_NOISE_NONE>(c, fused, wn);
      break;
  }
  if (fused) {
    c->prebinned = true;
    c->promised = wn;
  }
  HIPCHK(hipGetLastError());
  c->in_step = false;
  c->tick += 1;
  c->normals_valid = 1;
  // pass B stores exactly the live particles of this tick: a count the host has read inside the tick
  // (sc_step_stats) brings the host-side bound back down, so that a long run of emit / remove / emit
  // without downloads does not accumulate `upper` as everything ever emitted
  if (c->stats_live >= 0 && !c->slab) c->upper = c->stats_live;
  c->stats_live = -1;
  if (c->probe_on && !c->slab && !c->custom_grid) {
    const int rc = probe_launch(c, true);
    if (rc) return rc;
  }
  if (c->track_on && !c->slab && !c->custom_grid && c->tick % c->track_every == 0) return track_launch(c, true);
  return SC_OK;
}

int sc_step(sc_ctx* c, int32_t n_ticks) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->noise_mode == SC_NOISE_HOST) return fail(SC_ERR_STATE, "sc_step is not available in SC_NOISE_HOST mode");
  if (c->slab && n_ticks > 1) return fail(SC_ERR_STATE, "slab mode: one tick per halo exchange");
  for (int t = 0; t < n_ticks; ++t) {
    int rc = sc_step_begin(c);
    if (rc) return rc;
    if (t + 1 < n_ticks) {  // the next tick of this call has the same inputs: promise them
      c->next = c->now;
      c->have_next = true;
    }
    rc = sc_step_finish(c);
    if (rc) return rc;
  }
  return SC_OK;
}

int sc_tick(sc_ctx* c, const sc_tick_inputs* now, const sc_tick_inputs* next) {
  if (!c || !now) return fail(SC_ERR_ARG, "null argument");
  // (SC_NOISE_HOST needs the host's noise block between the two halves of a tick -- unless the device holds the stream)
  if (c->noise_mode == SC_NOISE_HOST && !c->rng)
    return fail(SC_ERR_STATE, "sc_tick is not available in SC_NOISE_HOST mode unless the device holds the stream (sc_rng_set_state)");
  int rc = sc_set_params(c, &now->params);
  if (rc) return rc;
  rc = sc_set_segments(c, now->segments, now->padded, now->n_segments, now->bodies, now->n_bodies);
  if (rc) return rc;
  rc = sc_step_begin(c);
  if (rc) return rc;
  if (next) {
    rc = sc_set_next_inputs(c, &next->params, next->segments, next->n_segments, next->bodies, next->n_bodies);
    if (rc) {
      c->have_next = false;
      (void)sc_step_finish(c);  // leave the context between ticks; the error of the promise is what is reported
      return rc;
    }
  }
  return sc_step_finish(c);
}

int sc_set_next_inputs(sc_ctx* c, const sc_params* p, const double* segments, int32_t ns, const sc_body* bodies,
                       int32_t nb) {
  if (!c || !p) return fail(SC_ERR_ARG, "null argument");
  if (!c->in_step) return fail(SC_ERR_STATE, "sc_set_next_inputs belongs between sc_step_begin and sc_step_finish");
  const int rc = load_walls(c->next, segments, nullptr, false, ns, bodies, nb);
  if (rc) return rc;
  c->next.params = *p;
  c->have_next = true;
  return SC_OK;
}

// ---- downloads -----------------------------------------------------------------------------

static int fetch(sc_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return SC_OK;
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  return SC_OK;
}

// The index order on the host: the slots 0 .. n -- with `x`, only those whose x is finite: slab mode leaves dead ghost
// copies (x = +inf) behind -- ascending by id.  (On the device: state_row_live in sc_state.h.)
static std::vector<int> index_order(const int* id, const double* x, int64_t n) {
  std::vector<int> order;
  order.reserve(n);
  for (int64_t k = 0; k < n; ++k)
    if (!x || std::isfinite(x[k])) order.push_back((int)k);
  std::sort(order.begin(), order.end(), [&](int p, int q) { return id[p] < id[q]; });
  return order;
}

// Row k of `out` (may be null) is the pair (a[stride s], b[stride s]) of slot s = order[k].
static void write_pairs(double* out, const std::vector<int>& order, const double* a, const double* b, int stride = 1) {
  for (size_t k = 0; k < order.size() && out; ++k) {
    out[2 * k] = a[(size_t)stride * order[k]];
    out[2 * k + 1] = b[(size_t)stride * order[k]];
  }
}

int sc_download_state(sc_ctx* c, double* xy, double* vxy, double* pressure, int64_t* ids, int64_t room, int64_t* n_out) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_download_state inside a tick");
  int h[C_COUNT];
  int rc = read_counters(c, h);
  if (rc) return rc;
  int64_t n = h[C_NS];
  c->upper = n;
  if (n_out) *n_out = n;
  if (n > room) return fail(SC_ERR_CAPACITY, "host arrays hold %lld, %lld particles live", (long long)room, (long long)n);
  // the error bits are this call's to report, once the state is out; what an abandoned tick left is repaired first, so that
  // the pressures are cut where the last finished tick left them
  const int flagged = recover_flags(c, h);
  if (h[C_FLAGS] & F_SCAN_TIMEOUT) h[C_NT] = h[C_NT_DONE];
  std::vector<double> hx(n), hy(n), hvx(n), hvy(n), hp(n, 0.0);
  std::vector<int> hid(n);
  size_t b = n * sizeof(double);
  if ((rc = fetch(c, hx.data(), c->x, b)) || (rc = fetch(c, hy.data(), c->y, b)) ||
      (rc = fetch(c, hvx.data(), c->vx, b)) || (rc = fetch(c, hvy.data(), c->vy, b)) ||
      (rc = fetch(c, hid.data(), c->id[0], n * sizeof(int))))
    return rc;
  // pressure is valid for the particles of the last finished tick, which are exactly the stored
  // ones unless particles were uploaded/appended since
  int64_t np = c->normals_valid ? std::min<int64_t>(n, h[C_NT]) : 0;
  if (pressure && np > 0 && (rc = fetch(c, hp.data(), c->P, np * sizeof(double)))) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  const std::vector<int> order = index_order(hid.data(), hx.data(), n);
  n = (int64_t)order.size();
  if (n_out) *n_out = n;
  write_pairs(xy, order, hx.data(), hy.data());
  write_pairs(vxy, order, hvx.data(), hvy.data());
  for (int64_t k = 0; k < n; ++k) {
    const int s = order[k];
    if (pressure) pressure[k] = s < np ? hp[s] : 0.0;
    if (ids) ids[k] = hid[s];
  }
  return flagged;
}

// ---- the state in the caller's device memory (sc_state.h) ---------------------------------------

// Ranks the m slots of the launch by id into set *set of stateSort: slots that are not stored, or whose x is not finite,
// carry kStateDead and come last.
static int state_rank(sc_ctx* c, int64_t m, int* set) {
  const int rc = c->stateSort.ensure(m, c->stream);
  if (rc) return rc;
  return radix_sort(c, c->stateSort, StateKey{c->counters, c->x, c->id[0], (int)c->cap}, m, kStatePasses, set);
}

int sc_export_state_device(sc_ctx* c, double* dev_xy, double* dev_vxy, double* dev_pressure, int64_t* dev_ids, int64_t room,
                           int64_t* dev_n) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_n) return fail(SC_ERR_ARG, "null count pointer");
  if (room < 0) return fail(SC_ERR_ARG, "negative room");
  if (((uintptr_t)dev_xy | (uintptr_t)dev_vxy) & 15) return fail(SC_ERR_ARG, "xy and vxy must be aligned to 16 bytes");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_export_state_device inside a tick");
  const int64_t m = std::min<int64_t>(launch_bound(c), c->cap);
  if (room < m)
    return fail(SC_ERR_CAPACITY, "device arrays hold %lld, up to %lld particles stored", (long long)room, (long long)m);
  HIPCHK(hipSetDevice(c->device));
  int set;
  const int rc = state_rank(c, m, &set);
  if (rc) return rc;
  const StateOut o{dev_xy, dev_vxy, dev_pressure, (long long*)dev_ids, (long long*)dev_n};
  hipLaunchKernelGGL(k_state_gather, dim3(grid_for(m)), dim3(kBlock), 0, c->stream, c->counters, o,
                     c->stateSort.keys[set].get(), c->stateSort.vals[set].get(), (int)m, (int)c->cap,
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
    HIPCHK(c->stateWords.grow(2, c->stream));
    HIPCHK(c->stateIds.grow(n, c->stream));
    HIPCHK(hipMemsetAsync(c->stateWords, 0, 2 * sizeof(int), c->stream));
    hipLaunchKernelGGL(k_state_check_ids, dim3(grid_for(n)), dim3(kBlock), 0, c->stream, (const long long*)dev_ids, (int)n,
                       c->stateIds.get(), c->stateWords.get());
    HIPCHK(hipGetLastError());
    int words[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(words, c->stateWords, sizeof words, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (words[1]) return fail(SC_ERR_ARG, "particle id out of range");
    ids32 = c->stateIds;
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

// Room for a search over m points in `buckets` buckets: each group is sized by its last member, which grows last.
static int pairs_ensure(sc_ctx* c, int64_t m, int64_t buckets) {
  HIPCHK(c->pairsFlag.grow(1, c->stream));
  HIPCHK(c->pairsWords.grow(PW_WORDS, c->stream));
  if (buckets + 1 > c->pairsBucketStart.size()) {
    HIPCHK(c->pairsBucketCount.grow(buckets, c->stream));
    HIPCHK(c->pairsBucketSums.grow(buckets / kScanPerBlock + 2, c->stream));
    HIPCHK(c->pairsBucketStart.grow(buckets + 1, c->stream));
  }
  const int rc = c->pairsSort.ensure(m, c->stream);
  if (rc) return rc;
  if (m + 1 > c->pairsOffs.size()) {
    HIPCHK(c->pairsXY.grow(m, c->stream));
    HIPCHK(c->pairsSXY.grow(m, c->stream));
    HIPCHK(c->pairsCell.grow(m, c->stream));
    HIPCHK(c->pairsRowLen.grow(m, c->stream));
    HIPCHK(c->pairsSums.grow(m / kScanPerBlock + 2, c->stream));
    HIPCHK(c->pairsOffs.grow(m + 1, c->stream));
  }
  return SC_OK;
}

int sc_pairs_count_device(sc_ctx* c, const double* dev_xy, int64_t n, double radius, int32_t flags, int64_t* dev_offsets,
                          int64_t room_rows, int64_t* dev_counts) {
  if (!c) return fail(SC_ERR_ARG, "null context");
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
  const int64_t m = dev_xy ? n : std::min<int64_t>(launch_bound(c), c->cap);
  if (m > kPairsMaxPoints) return fail(SC_ERR_CAPACITY, "%lld points, at most %lld", (long long)m, (long long)kPairsMaxPoints);
  if (room_rows < m)
    return fail(SC_ERR_CAPACITY, "offsets hold %lld rows, up to %lld points", (long long)room_rows, (long long)m);
  HIPCHK(hipSetDevice(c->device));
  c->pairs_valid = false;
  const unsigned buckets = pairs_buckets(m);
  int rc = pairs_ensure(c, m, buckets);
  if (rc) return rc;
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
    hipLaunchKernelGGL(k_pairs_gather, dim3(grid), dim3(kBlock), 0, c->stream, c->stateSort.keys[set].get(),
                       c->stateSort.vals[set].get(), (int)m, c->x.get(), c->y.get(), c->pairsXY.get(), c->pairsWords.get());
  }
  HIPCHK(hipMemsetAsync(c->pairsFlag, 0, sizeof(int), c->stream));
  HIPCHK(hipMemsetAsync(c->pairsBucketCount, 0, (size_t)buckets * sizeof(int), c->stream));
  RadixSpace& w = c->pairsSort;
  hipLaunchKernelGGL(k_pairs_key, dim3(grid), dim3(kBlock), 0, c->stream, g, dev_xy ? (const XY*)dev_xy : c->pairsXY.get(),
                     c->pairsXY.get(), dev_xy ? (long long)n : -1LL, c->pairsWords.get(), (int)m, w.keys[0].get(),
                     w.vals[0].get(), c->pairsBucketCount.get(), c->pairsFlag.get());
  // the binning sort: the keys are 0 .. buckets (a dead point's), so as many digits as `buckets` has
  int bits = 1;
  while ((buckets >> bits) != 0) ++bits;
  int in;
  if ((rc = radix_sort(c, w, RadixStored{}, m, (bits + kRadixDigitBits - 1) / kRadixDigitBits, &in))) return rc;
  if ((rc = launch_scan(c, c->pairsBucketCount, c->pairsBucketStart, buckets, c->pairsBucketSums, nullptr))) return rc;
  hipLaunchKernelGGL(k_pairs_place, dim3(grid), dim3(kBlock), 0, c->stream, g, w.keys[in].get(), w.vals[in].get(), (int)m,
                     c->pairsXY.get(), c->pairsFlag.get(), c->pairsSXY.get(), c->pairsCell.get());
  hipLaunchKernelGGL(k_pairs_count, dim3(grid), dim3(kBlock), 0, c->stream, g, c->pairsWords.get(), c->pairsFlag.get(), (int)m,
                     c->pairsXY.get(), c->pairsBucketStart.get(), c->pairsSXY.get(), c->pairsCell.get(), w.vals[in].get(),
                     c->pairsRowLen.get());
  const int nb = (int)(m / kScanPerBlock + 1);  // entry n <= m lies in one of them
  hipLaunchKernelGGL(k_scan64_local, dim3(nb), dim3(kBlock), 0, c->stream, c->pairsRowLen.get(), c->pairsOffs.get(),
                     c->pairsWords.get(), c->pairsFlag.get(), c->pairsSums.get());
  hipLaunchKernelGGL(k_scan64_fix, dim3(nb), dim3(kBlock), 0, c->stream, c->pairsOffs.get(), (long long*)dev_offsets,
                     c->pairsWords.get(), c->pairsFlag.get(), c->pairsSums.get(), (long long*)dev_counts);
  HIPCHK(hipGetLastError());
  c->pairs_valid = true;
  c->pairs_m = m;
  c->pairs_set = in;
  c->pairs_grid = g;
  return SC_OK;
}

int sc_pairs_fill_device(sc_ctx* c, int64_t* dev_partners, double* dev_d2, int64_t room_pairs) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (room_pairs < 0) return fail(SC_ERR_ARG, "negative room");
  if (!dev_partners && room_pairs > 0) return fail(SC_ERR_ARG, "null partners pointer");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_pairs_fill_device inside a tick");
  if (!c->pairs_valid)
    return fail(SC_ERR_STATE, "no pair count to fill from: sc_pairs_count_device comes first, and the state must not change in between");
  HIPCHK(hipSetDevice(c->device));
  const int64_t m = c->pairs_m;
  if (room_pairs == 0) return SC_OK;
  hipLaunchKernelGGL(k_pairs_fill, dim3(grid_for(m)), dim3(kBlock), 0, c->stream, c->pairs_grid, c->pairsWords.get(),
                     c->pairsFlag.get(), (int)m, c->pairsXY.get(), c->pairsOffs.get(), c->pairsBucketStart.get(),
                     c->pairsSXY.get(), c->pairsCell.get(), c->pairsSort.vals[c->pairs_set].get(), (long long*)dev_partners, dev_d2,
                     (long long)room_pairs);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

// ---- clusters (sc_clusters.h) --------------------------------------------------------------------

int sc_pairs_label_device(sc_ctx* c, int64_t* dev_labels, int64_t room_rows, int64_t* dev_sizes, int64_t* dev_roots,
                          int64_t room_clusters, int64_t* dev_counts) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_labels || !dev_counts) return fail(SC_ERR_ARG, "null labels or counts pointer");
  if (room_rows < 0 || room_clusters < 0) return fail(SC_ERR_ARG, "negative room");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_pairs_label_device inside a tick");
  if (!c->pairs_valid)
    return fail(SC_ERR_STATE, "no pair count to label from: sc_pairs_count_device comes first, and the state must not change in between");
  const int64_t m = c->pairs_m;
  if (room_rows < m)
    return fail(SC_ERR_CAPACITY, "labels hold %lld rows, up to %lld points", (long long)room_rows, (long long)m);
  HIPCHK(hipSetDevice(c->device));
  if (m + 1 > c->clusterDense.size()) {  // (sized by the last member, which grows last)
    HIPCHK(c->clusterParent.grow(m, c->stream));
    HIPCHK(c->clusterIsRoot.grow(m, c->stream));
    HIPCHK(c->clusterSize.grow(m, c->stream));
    HIPCHK(c->clusterSums.grow(m / kScanPerBlock + 2, c->stream));
    HIPCHK(c->clusterDense.grow(m + 1, c->stream));
  }
  PairsGrid g = c->pairs_grid;
  g.half = 0;  // the components are those of the full graph, whichever form the count had
  const int grid = grid_for(m);
  const long long* words = c->pairsWords.get();
  const int* flag = c->pairsFlag.get();
  int* parent = c->clusterParent.get();
  hipLaunchKernelGGL(k_cluster_init, dim3(grid), dim3(kBlock), 0, c->stream, words, flag, (int)m, parent);
  hipLaunchKernelGGL(k_cluster_union, dim3(grid), dim3(kBlock), 0, c->stream, g, words, flag, (int)m, c->pairsXY.get(),
                     c->pairsBucketStart.get(), c->pairsSXY.get(), c->pairsCell.get(),
                     c->pairsSort.vals[c->pairs_set].get(), parent);
  // a tree of at most m nodes is at most m - 1 deep, and a round halves (rounding up) every depth
  int rounds = 1;
  while (((int64_t)1 << rounds) < m) ++rounds;
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(k_cluster_jump, dim3(grid), dim3(kBlock), 0, c->stream, words, flag, (int)m, parent);
  hipLaunchKernelGGL(k_cluster_mark, dim3(grid), dim3(kBlock), 0, c->stream, words, flag, (int)m, c->pairsXY.get(), parent,
                     c->clusterIsRoot.get(), c->clusterSize.get());
  const int rc = launch_scan(c, c->clusterIsRoot, c->clusterDense, m, c->clusterSums, nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(k_cluster_write, dim3(grid), dim3(kBlock), 0, c->stream, words, flag, (int)m, c->pairsXY.get(), parent,
                     c->clusterDense.get(), c->clusterSize.get(), (long long*)dev_labels, (long long*)dev_roots,
                     (long long)room_clusters);
  hipLaunchKernelGGL(k_cluster_finish, dim3(grid), dim3(kBlock), 0, c->stream, words, flag, (int)m, c->clusterDense.get(),
                     c->clusterSize.get(), (long long*)dev_sizes, (long long)room_clusters, (long long*)dev_counts);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

// ---- rendering (sc_render.h) ------------------------------------------------------------------

constexpr int kRenderMaxSide = 16384;
constexpr long long kRenderMaxRadius = 1LL << 24;  // keeps the squared pixel distances of a disc exact in 64 bits

// Checks the call and turns the view and the walls into the kernels' argument.
static int render_prepare(sc_ctx* c, const sc_view* view, const double* segments, int32_t ns, bool has_frame, RenderView& v) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "rendering happens between ticks");
  if (!view || !has_frame) return fail(SC_ERR_ARG, "null view or frame");
  const sc_view& q = *view;
  if (q.width < 1 || q.width > kRenderMaxSide || q.height < 1 || q.height > kRenderMaxSide)
    return fail(SC_ERR_ARG, "frame of %d x %d pixels; each side 1..%d", q.width, q.height, kRenderMaxSide);
  if (!(std::isfinite(q.zoom) && q.zoom > 0)) return fail(SC_ERR_ARG, "zoom must be finite and positive");
  if (!std::isfinite(q.center_x) || !std::isfinite(q.center_y)) return fail(SC_ERR_ARG, "the view center must be finite");
  if (!(std::isfinite(q.particle_radius) && q.particle_radius >= 0))
    return fail(SC_ERR_ARG, "particle_radius must be finite and not negative");
  if (q.segment_width < 0) return fail(SC_ERR_ARG, "segment_width must not be negative");
  if (ns < 0 || ns > kMaxSeg) return fail(SC_ERR_ARG, "%d segments, at most %d", ns, kMaxSeg);
  if (ns > 0 && !segments) return fail(SC_ERR_ARG, "null segments");
  v = RenderView{};
  v.width = q.width;
  v.height = q.height;
  v.center_x = q.center_x;
  v.center_y = q.center_y;
  v.zoom = q.zoom;
  v.half_w = q.width / 2.0;
  v.half_h = q.height / 2.0;
  v.sx = q.width - 1.0;
  v.sy = q.height - 1.0;
  // playback.py:195: int(screen_x * particle_radius) * zoom_factor, floored to whole pixels
  const double R = std::floor(std::trunc(q.width * q.particle_radius) * q.zoom);
  if (!(R <= (double)kRenderMaxRadius)) return fail(SC_ERR_ARG, "disc radius of %g pixels, at most %lld", R, kRenderMaxRadius);
  v.radius = (long long)R;
  v.radius_d = R;
  v.w2 = (double)q.segment_width * q.segment_width;
  const double margin = q.segment_width + 1.0;
  for (int k = 0; k < ns; ++k) {
    const double* e = segments + 4 * k;
    // the same view as the particles', not floored (playback.py:180-186 hands these to pygame.draw.line)
    const double ax = (std::trunc(e[0] * v.sx) - v.center_x) * v.zoom + v.half_w;
    const double ay = (std::trunc(e[1] * v.sy) - v.center_y) * v.zoom + v.half_h;
    const double bx = (std::trunc(e[2] * v.sx) - v.center_x) * v.zoom + v.half_w;
    const double by = (std::trunc(e[3] * v.sy) - v.center_y) * v.zoom + v.half_h;
    if (!std::isfinite(ax) || !std::isfinite(ay) || !std::isfinite(bx) || !std::isfinite(by)) continue;  // covers nothing
    RenderSeg& r = v.seg[v.nseg++];
    r.ax = ax;
    r.ay = ay;
    r.dx = bx - ax;
    r.dy = by - ay;
    r.len2 = r.dx * r.dx + r.dy * r.dy;
    // the closest point a + t (b - a), t in [0, 1], lies between a and the ROUNDED a + (b - a)
    const double ex = ax + r.dx, ey = ay + r.dy;
    r.lox = std::min({ax, bx, ex}) - margin;
    r.hix = std::max({ax, bx, ex}) + margin;
    r.loy = std::min({ay, by, ey}) - margin;
    r.hiy = std::max({ay, by, ey}) + margin;
  }
  return SC_OK;
}

// Enqueues the HUD overlay over a resolved frame: over the text's bounding box clipped to the frame, or not at all
// when there is no HUD or the box is empty.
static void hud_launch(sc_ctx* c, const RenderView& v, unsigned char* frame, bool as_index) {
  if (c->hud_lines == 0) return;
  const long long bw = std::min<long long>(v.width - c->hud_x, (long long)c->hud_longest * kFontCols * c->hud_scale);
  const long long bh = std::min<long long>(v.height - c->hud_y, (long long)c->hud_lines * kHudPitch * c->hud_scale);
  if (bw <= 0 || bh <= 0) return;
  const HudBox b{v.width, c->hud_x, c->hud_y, (int)bw, (int)bh, c->hud_scale};
  const dim3 grid((unsigned)((bw + kHudTileW - 1) / kHudTileW), (unsigned)((bh + kHudTileH - 1) / kHudTileH));
  if (as_index)
    hipLaunchKernelGGL(k_hud_overlay<true>, grid, dim3(kBlock), 0, c->stream, b, c->hudText, c->hudLines, frame);
  else
    hipLaunchKernelGGL(k_hud_overlay<false>, grid, dim3(kBlock), 0, c->stream, b, c->hudText, c->hudLines, frame);
}

// Enqueues the arrow pass over a resolved frame: a wave per kArrowListPerWave arrows of the list, or a thread per slot
// under the host's bound of the live count, or nothing at all when no arrows are set.
static void arrows_launch(sc_ctx* c, const RenderView& v, unsigned char* frame, bool as_index) {
  if (c->arrow_mode == SC_ARROWS_OFF) return;
  const bool from_list = c->arrow_mode == SC_ARROWS_LIST;
  const int64_t count = from_list ? c->arrow_n : std::min<int64_t>(launch_bound(c), c->cap);
  if (count <= 0) return;
  const ArrowView a{v.width, v.height, v.center_x, v.center_y, v.zoom, v.half_w, v.half_h, v.sx, v.sy};
  const sc_arrow* list = from_list ? c->arrowList.get() : nullptr;
  const int64_t threads = from_list ? (count + kArrowListPerWave - 1) / kArrowListPerWave * 64 : count;
  if (as_index)
    hipLaunchKernelGGL(k_arrows<true>, dim3(grid_for(threads)), dim3(kBlock), 0, c->stream, a, list, (int)count, c->counters,
                       c->x, c->y, c->vx, c->vy, c->id[0], c->arrow_scale, (long long)c->arrow_every, frame);
  else
    hipLaunchKernelGGL(k_arrows<false>, dim3(grid_for(threads)), dim3(kBlock), 0, c->stream, a, list, (int)count, c->counters,
                       c->x, c->y, c->vx, c->vy, c->id[0], c->arrow_scale, (long long)c->arrow_every, frame);
}

// Grows the key buffer and enqueues splat, resolve, the arrows and the HUD overlay into `rgb` (device memory), or with
// `as_index` the resolve that writes one palette index per pixel into it (4-byte aligned).
static int render_launch(sc_ctx* c, const RenderView& v, unsigned char* rgb, bool as_index = false) {
  const int64_t pixels = (int64_t)v.width * v.height;
  if (pixels > c->renderKeys.size()) {
    HIPCHK(c->renderKeys.grow(pixels, c->stream));
    // zero once: every resolve clears the keys it reads, which are all that the splat before it may have set
    HIPCHK(hipMemsetAsync(c->renderKeys, 0, c->renderKeys.bytes(), c->stream));
  }
  const int64_t bound = std::min<int64_t>(launch_bound(c), c->cap);
  if (bound > 0) {
    if (v.radius > kRenderWaveRadius)
      hipLaunchKernelGGL(k_render_splat<true>, dim3((unsigned)((bound * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                         v, c->counters, c->x, c->y, c->id[0], c->P, c->normals_valid ? 1 : 0, (int)bound, c->renderKeys);
    else
      hipLaunchKernelGGL(k_render_splat<false>, dim3(grid_for(bound)), dim3(kBlock), 0, c->stream, v, c->counters, c->x,
                         c->y, c->id[0], c->P, c->normals_valid ? 1 : 0, (int)bound, c->renderKeys);
  }
  if (as_index)
    hipLaunchKernelGGL(k_render_resolve_index, dim3(grid_for((pixels + 3) / 4)), dim3(kBlock), 0, c->stream, v, c->renderKeys,
                       rgb, c->arrow_mode == SC_ARROWS_OFF ? 1u : 2u);  // (entry 1 is the arrows' when there are any)
  else
    hipLaunchKernelGGL(k_render_resolve, dim3(grid_for((pixels + 3) / 4)), dim3(kBlock), 0, c->stream, v, c->renderKeys, rgb,
                       ((uintptr_t)rgb & 3) == 0 ? 1 : 0);
  arrows_launch(c, v, rgb, as_index);
  hud_launch(c, v, rgb, as_index);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

int sc_set_hud(sc_ctx* c, const char* text, int32_t n_bytes, int32_t x, int32_t y, int32_t scale) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (n_bytes < 0 || n_bytes > kHudMaxBytes) return fail(SC_ERR_ARG, "HUD text of %d bytes; 0..%d", n_bytes, kHudMaxBytes);
  if (n_bytes > 0 && !text) return fail(SC_ERR_ARG, "null HUD text");
  if (x < 0 || x > kRenderMaxSide || y < 0 || y > kRenderMaxSide)
    return fail(SC_ERR_ARG, "HUD origin (%d, %d); each coordinate 0..%d", x, y, kRenderMaxSide);
  if (scale < 1 || scale > kHudMaxScale) return fail(SC_ERR_ARG, "HUD scale %d; 1..%d", scale, kHudMaxScale);
  HIPCHK(hipSetDevice(c->device));
  c->hud_lines = 0;  // (a call that fails below leaves no HUD)
  if (n_bytes > 0) {
    // the lines as str.split("\n") cuts them: a trailing newline yields an empty last line
    std::vector<HudLine> lines;
    int start = 0, longest = 0;
    for (int k = 0; k <= n_bytes; ++k) {
      if (k < n_bytes && text[k] != '\n') continue;
      lines.push_back(HudLine{start, k - start});
      longest = std::max(longest, k - start);
      start = k + 1;
    }
    HIPCHK(c->hudText.grow(n_bytes, c->stream));
    HIPCHK(c->hudLines.grow((int64_t)lines.size(), c->stream));
    HIPCHK(hipMemcpyAsync(c->hudText, text, (size_t)n_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->hudLines, lines.data(), lines.size() * sizeof(HudLine), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // `text` and `lines` are the caller's and ours: read before we return
    c->hud_longest = longest;
    c->hud_x = x;
    c->hud_y = y;
    c->hud_scale = scale;
    c->hud_lines = (int)lines.size();
    return SC_OK;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return SC_OK;
}

int sc_set_arrows(sc_ctx* c, int32_t mode, const sc_arrow* arrows, int64_t n, double scale, int64_t every) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "the arrows are set between ticks");
  if (mode != SC_ARROWS_OFF && mode != SC_ARROWS_LIST && mode != SC_ARROWS_VELOCITY)
    return fail(SC_ERR_ARG, "arrow mode %d; SC_ARROWS_OFF, _LIST or _VELOCITY", mode);
  // (every argument is checked in every mode: a caller's mistake shows at once, not when the mode changes)
  if (n < 0 || n > kArrowMaxList) return fail(SC_ERR_ARG, "%lld arrows; 0..%lld", (long long)n, kArrowMaxList);
  if (n > 0 && !arrows) return fail(SC_ERR_ARG, "null arrow list");
  if (every < 1) return fail(SC_ERR_ARG, "an arrow for every %lld-th particle; at least 1", (long long)every);
  if (!std::isfinite(scale)) return fail(SC_ERR_ARG, "the arrows' scale must be finite");
  HIPCHK(hipSetDevice(c->device));
  c->arrow_mode = SC_ARROWS_OFF;  // (a call that fails below leaves no arrows)
  if (mode == SC_ARROWS_LIST && n > 0) {
    HIPCHK(c->arrowList.grow(n, c->stream));
    HIPCHK(hipMemcpyAsync(c->arrowList, arrows, (size_t)n * sizeof(sc_arrow), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));  // `arrows` is the caller's: read before we return
  if (mode == SC_ARROWS_LIST && n > 0) {
    c->arrow_n = n;
    c->arrow_mode = SC_ARROWS_LIST;
  } else if (mode == SC_ARROWS_VELOCITY) {
    c->arrow_scale = scale;
    c->arrow_every = every;
    c->arrow_mode = SC_ARROWS_VELOCITY;
  }
  return SC_OK;
}

int sc_render_device(sc_ctx* c, const sc_view* view, const double* segments, int32_t n_segments, uint8_t* dev_rgb) {
  RenderView v;
  int rc = render_prepare(c, view, segments, n_segments, dev_rgb != nullptr, v);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  return render_launch(c, v, dev_rgb);
}

int sc_render(sc_ctx* c, const sc_view* view, const double* segments, int32_t n_segments, uint8_t* rgb) {
  RenderView v;
  int rc = render_prepare(c, view, segments, n_segments, rgb != nullptr, v);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  const int64_t bytes = 3 * (int64_t)v.width * v.height;
  HIPCHK(c->renderRgb.grow(bytes, c->stream));
  if ((rc = render_launch(c, v, c->renderRgb))) return rc;
  HIPCHK(hipMemcpyAsync(rgb, c->renderRgb, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return SC_OK;
}

// ---- JPEG encoding (sc_jpeg.h) -------------------------------------------------------------------

constexpr int kJpegHeaderBytes = 613;  // SOI, APP0, DQT, SOF0, DHT, DRI, SOS as jpeg_header writes them

static void jpeg_quant(int quality, int q[2][64]) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int k = 0; k < 64; ++k) {
    q[0][k] = std::min(255, std::max(1, (kJpegLumaQ[k] * s + 50) / 100));
    q[1][k] = std::min(255, std::max(1, (kJpegChromaQ[k] * s + 50) / 100));
  }
}

// SOI through SOS (tests/jpeg_spec.py: header).
static std::vector<unsigned char> jpeg_header(int width, int height, const int q[2][64]) {
  std::vector<unsigned char> h;
  auto u8 = [&](int v) { h.push_back((unsigned char)v); };
  auto u16 = [&](int v) { u8(v >> 8); u8(v & 0xFF); };
  u16(0xFFD8);
  u16(0xFFE0); u16(16);
  for (char ch : {'J', 'F', 'I', 'F', '\0'}) u8(ch);
  u8(1); u8(1); u8(0); u16(1); u16(1); u8(0); u8(0);
  u16(0xFFDB); u16(2 + 2 * 65);
  for (int t = 0; t < 2; ++t) {
    unsigned char zz[64];
    for (int k = 0; k < 64; ++k) zz[kJpegZigzag.of[k]] = (unsigned char)q[t][k];
    u8(t);
    for (int k = 0; k < 64; ++k) u8(zz[k]);
  }
  u16(0xFFC0); u16(17); u8(8); u16(height); u16(width); u8(3);
  for (int id = 1; id <= 3; ++id) { u8(id); u8(0x11); u8(id == 1 ? 0 : 1); }
  u16(0xFFC4); u16(2 + 2 * (17 + 12) + 2 * (17 + 162));
  for (int t = 0; t < 2; ++t) {
    u8(t);
    for (int k = 0; k < 16; ++k) u8(kJpegDcBits[t][k]);
    for (int k = 0; k < 12; ++k) u8(kJpegDcVals[k]);
    u8(0x10 | t);
    for (int k = 0; k < 16; ++k) u8(kJpegAcBits[t][k]);
    for (int k = 0; k < 162; ++k) u8(kJpegAcVals[t][k]);
  }
  u16(0xFFDD); u16(4); u16((width + 7) / 8);
  u16(0xFFDA); u16(12); u8(3);
  for (int id = 1; id <= 3; ++id) { u8(id); u8(id == 1 ? 0x00 : 0x11); }
  u8(0); u8(63); u8(0);
  return h;
}

int sc_jpeg_bound(int32_t width, int32_t height, int64_t* bound) {
  if (width < 1 || width > kRenderMaxSide || height < 1 || height > kRenderMaxSide || !bound)
    return fail(SC_ERR_ARG, "frame of %d x %d pixels; each side 1..%d", width, height, kRenderMaxSide);
  const int64_t mcus = (width + 7) / 8, rows = (height + 7) / 8;
  const int64_t row_bytes = (3 * mcus * kJpegBlockBits + 7) / 8;
  *bound = kJpegHeaderBytes + rows * (2 * row_bytes + 2) + 2;  // every byte 0xFF, a marker after each row, EOI
  return SC_OK;
}

// Encodes the W x H x 3 RGB frame at `rgb` (device memory, checked by the caller) into `out` (host memory).
// Enqueued on the context's stream; synchronises twice: for the total length, then for the bytes.
static int jpeg_encode(sc_ctx* c, const unsigned char* rgb, int width, int height, int quality, uint8_t* out,
                       int64_t capacity, int64_t* n_out) {
  JpegDims d;
  d.width = width;
  d.height = height;
  d.mcus = (width + 7) / 8;
  d.rows = (height + 7) / 8;
  jpeg_quant(quality, d.quant);
  const int64_t nblocks = (int64_t)d.rows * d.mcus * 3;
  const long long row_words = (3LL * d.mcus * kJpegBlockBits + 7) / 32 + 1;  // a row's bits, padded
  // the workspace: coef | masks | acbits | rows' bit buffers | row bytes, row lengths | row offsets + total
  auto up = [](int64_t n) { return (n + 255) & ~(int64_t)255; };
  const int64_t o_mask = up(nblocks * 64 * (int64_t)sizeof(short));
  const int64_t o_ac = o_mask + up(nblocks * (int64_t)sizeof(unsigned long long));
  const int64_t o_rows = o_ac + up(nblocks * (int64_t)sizeof(int));
  const int64_t o_len = o_rows + up((int64_t)d.rows * row_words * (int64_t)sizeof(unsigned));
  const int64_t o_off = o_len + up(2 * (int64_t)d.rows * (int64_t)sizeof(int));
  const int64_t bytes = o_off + up(((int64_t)d.rows + 1) * (int64_t)sizeof(long long));
  HIPCHK(c->jpegWork.grow(bytes, c->stream));
  unsigned char* w = c->jpegWork;
  short* coef = (short*)w;
  unsigned long long* masks = (unsigned long long*)(w + o_mask);
  int* acbits = (int*)(w + o_ac);
  unsigned* rowbuf = (unsigned*)(w + o_rows);
  int* row_bytes = (int*)(w + o_len);
  int* row_len = row_bytes + d.rows;
  long long* row_off = (long long*)(w + o_off);

  hipLaunchKernelGGL(k_jpeg_dct, dim3((unsigned)((nblocks * 8 + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, d, rgb,
                     coef, masks, acbits);
  hipLaunchKernelGGL(k_jpeg_rows, dim3((unsigned)d.rows), dim3(64), 0, c->stream, d, coef, masks, acbits, rowbuf, row_words,
                     row_bytes, row_len);
  hipLaunchKernelGGL(k_jpeg_scan, dim3(1), dim3(64), 0, c->stream, d.rows, row_len, row_off);
  HIPCHK(hipGetLastError());
  long long total = 0;
  HIPCHK(hipMemcpyAsync(&total, row_off + d.rows, sizeof total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const std::vector<unsigned char> hdr = jpeg_header(width, height, d.quant);
  const int64_t need = (int64_t)hdr.size() + total + 2;
  *n_out = need;
  if (need > capacity) return fail(SC_ERR_CAPACITY, "the JPEG takes %lld bytes, the buffer holds %lld", (long long)need,
                                   (long long)capacity);
  HIPCHK(c->jpegOut.grow(total, c->stream));
  hipLaunchKernelGGL(k_jpeg_stuff, dim3((unsigned)d.rows), dim3(64), 0, c->stream, d.rows, rowbuf, row_words, row_bytes,
                     row_off, c->jpegOut);
  HIPCHK(hipGetLastError());
  std::memcpy(out, hdr.data(), hdr.size());
  HIPCHK(hipMemcpyAsync(out + hdr.size(), c->jpegOut, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  out[need - 2] = 0xFF;
  out[need - 1] = 0xD9;
  return SC_OK;
}

static int jpeg_check(sc_ctx* c, int quality, const uint8_t* out, int64_t capacity, const int64_t* n_out) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "encoding happens between ticks");
  if (quality < 1 || quality > 100) return fail(SC_ERR_ARG, "quality %d, expected 1..100", quality);
  if (!n_out || capacity < 0 || (!out && capacity > 0)) return fail(SC_ERR_ARG, "null n_out, or a negative capacity, or a null buffer");
  return SC_OK;
}

int sc_jpeg_encode_device(sc_ctx* c, const uint8_t* dev_rgb, int32_t width, int32_t height, int32_t quality, uint8_t* out,
                          int64_t capacity, int64_t* n_out) {
  int rc = jpeg_check(c, quality, out, capacity, n_out);
  if (rc) return rc;
  if (!dev_rgb) return fail(SC_ERR_ARG, "null frame");
  if (width < 1 || width > kRenderMaxSide || height < 1 || height > kRenderMaxSide)
    return fail(SC_ERR_ARG, "frame of %d x %d pixels; each side 1..%d", width, height, kRenderMaxSide);
  HIPCHK(hipSetDevice(c->device));
  return jpeg_encode(c, dev_rgb, width, height, quality, out, capacity, n_out);
}

int sc_render_jpeg(sc_ctx* c, const sc_view* view, const double* segments, int32_t n_segments, int32_t quality, uint8_t* out,
                   int64_t capacity, int64_t* n_out) {
  int rc = jpeg_check(c, quality, out, capacity, n_out);
  if (rc) return rc;
  RenderView v;
  if ((rc = render_prepare(c, view, segments, n_segments, true, v))) return rc;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(c->renderRgb.grow(3 * (int64_t)v.width * v.height, c->stream));
  if ((rc = render_launch(c, v, c->renderRgb))) return rc;
  return jpeg_encode(c, c->renderRgb, v.width, v.height, quality, out, capacity, n_out);
}

// ---- GIF encoding (sc_gif.h) ---------------------------------------------------------------------

int sc_gif_bound(int32_t width, int32_t height, int64_t* bound) {
  if (width < 1 || width > kRenderMaxSide || height < 1 || height > kRenderMaxSide || !bound)
    return fail(SC_ERR_ARG, "frame of %d x %d pixels; each side 1..%d", width, height, kRenderMaxSide);
  const int64_t pixels = (int64_t)width * height, chunks = (pixels + kGifChunk - 1) / kGifChunk;
  const int64_t bytes = (11 * (pixels + chunks + 1) + 7) / 8;  // a code per pixel, a clear per chunk, the end code
  *bound = 2 + bytes + (bytes + 254) / 255;                    // minimum code size, sub-block lengths, terminator
  return SC_OK;
}

// Encodes the W x H palette indices at `index` (device memory, checked by the caller) into `out` (host memory).
// Enqueued on the context's stream; synchronises twice: for the total length, then for the bytes.
static int gif_encode(sc_ctx* c, const unsigned char* index, int width, int height, uint8_t* out, int64_t capacity,
                      int64_t* n_out) {
  const int64_t pixels = (int64_t)width * height, chunks = (pixels + kGifChunk - 1) / kGifChunk;
  // the workspace: codes | code counts | bit offsets + the end code's, the two totals
  auto up = [](int64_t n) { return (n + 255) & ~(int64_t)255; };
  const int64_t o_count = up(chunks * kGifChunk * (int64_t)sizeof(unsigned short));
  const int64_t o_off = o_count + up(chunks * (int64_t)sizeof(int));
  HIPCHK(c->gifWork.grow(o_off + up((chunks + 3) * (int64_t)sizeof(long long)), c->stream));
  unsigned char* w = c->gifWork;
  unsigned short* codes = (unsigned short*)w;
  int* ncodes = (int*)(w + o_count);
  long long* bit_off = (long long*)(w + o_off);
  long long* totals = bit_off + chunks + 1;

  hipLaunchKernelGGL(k_gif_lzw, dim3((unsigned)chunks), dim3(64), 0, c->stream, index, (long long)pixels, codes, ncodes);
  hipLaunchKernelGGL(k_gif_scan, dim3(1), dim3(64), 0, c->stream, (int)chunks, ncodes, bit_off, totals);
  HIPCHK(hipGetLastError());
  long long total = 0;
  HIPCHK(hipMemcpyAsync(&total, totals, sizeof total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *n_out = total;
  if (total > capacity) return fail(SC_ERR_CAPACITY, "the GIF image data takes %lld bytes, the buffer holds %lld", total,
                                    (long long)capacity);
  const int64_t words = (total + 3) / 4;
  HIPCHK(c->gifOut.grow(words, c->stream));
  HIPCHK(hipMemsetAsync(c->gifOut, 0, (size_t)words * sizeof(unsigned), c->stream));
  hipLaunchKernelGGL(k_gif_merge, dim3((unsigned)chunks), dim3(64), 0, c->stream, (int)chunks, codes, ncodes, bit_off, totals,
                     c->gifOut);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, c->gifOut, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return SC_OK;
}

// (*n_out is set whatever follows: 0 until the size is known)
static int gif_check(sc_ctx* c, const uint8_t* out, int64_t capacity, int64_t* n_out) {
  if (n_out) *n_out = 0;
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "encoding happens between ticks");
  if (!n_out || capacity < 0 || (!out && capacity > 0)) return fail(SC_ERR_ARG, "null n_out, or a negative capacity, or a null buffer");
  return SC_OK;
}

int sc_gif_encode_device(sc_ctx* c, const uint8_t* dev_index, int32_t width, int32_t height, uint8_t* out, int64_t capacity,
                         int64_t* n_out) {
  int rc = gif_check(c, out, capacity, n_out);
  if (rc) return rc;
  if (!dev_index) return fail(SC_ERR_ARG, "null frame");
  if (width < 1 || width > kRenderMaxSide || height < 1 || height > kRenderMaxSide)
    return fail(SC_ERR_ARG, "frame of %d x %d pixels; each side 1..%d", width, height, kRenderMaxSide);
  HIPCHK(hipSetDevice(c->device));
  return gif_encode(c, dev_index, width, height, out, capacity, n_out);
}

int sc_render_gif(sc_ctx* c, const sc_view* view, const double* segments, int32_t n_segments, uint8_t* out, int64_t capacity,
                  int64_t* n_out) {
  int rc = gif_check(c, out, capacity, n_out);
  if (rc) return rc;
  RenderView v;
  if ((rc = render_prepare(c, view, segments, n_segments, true, v))) return rc;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(c->gifIndex.grow((int64_t)v.width * v.height, c->stream));
  if ((rc = render_launch(c, v, c->gifIndex, true))) return rc;
  return gif_encode(c, c->gifIndex, v.width, v.height, out, capacity, n_out);
}

int sc_download_sort(sc_ctx* c, int64_t* y_floored, int64_t* ids, int64_t room, int64_t* n_out) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!c->in_step) return fail(SC_ERR_STATE, "sc_download_sort is valid between sc_step_begin and sc_step_finish");
  int h[C_COUNT];
  int rc = read_counters(c, h);
  if (rc) return rc;
  int64_t n = h[C_NT];
  if (n_out) *n_out = n;
  if (n > room) return fail(SC_ERR_CAPACITY, "host arrays too small");
  std::vector<int> cell(n), id(n);
  if ((rc = fetch(c, cell.data(), c->cellT, n * sizeof(int))) || (rc = fetch(c, id.data(), c->id[1], n * sizeof(int))))
    return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int64_t k = 0; k < n; ++k) {
    if (y_floored) y_floored[k] = (int64_t)(cell[k] / c->w.ncols) + c->w.row0;
    if (ids) ids[k] = id[k];
  }
  return SC_OK;
}

int sc_download_neighbors(sc_ctx* c, int64_t* ids, int32_t* counts, int64_t* neighbors, double* fixed_xy, int64_t room,
                          int64_t* n_out) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!c->in_step) return fail(SC_ERR_STATE, "sc_download_neighbors is valid between sc_step_begin and sc_step_finish");
  int h[C_COUNT];
  int rc = read_counters(c, h);
  if (rc) return rc;
  int64_t n = h[C_NT];
  if (n_out) *n_out = n;
  if (n > room) return fail(SC_ERR_CAPACITY, "host arrays too small");
  std::vector<int> id(n);
  std::vector<NbrRow> rows(n);
  std::vector<double> hxy(2 * n);
  std::vector<int> slot(n);
  const int64_t nblocks = (n + kTileW - 1) / kTileW;
  std::vector<int> tb(6 * std::max<int64_t>(nblocks, 1));
  if ((rc = fetch(c, tb.data(), c->tileBoundsT, 6 * nblocks * sizeof(int)))) return rc;
  if ((rc = fetch(c, id.data(), c->id[1], n * sizeof(int))) || (rc = fetch(c, rows.data(), c->rows, n * sizeof(NbrRow))) ||
      (rc = fetch(c, hxy.data(), c->sxy, 2 * n * sizeof(double))))
    return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (neighbors)
    for (int64_t k = 0; k < n * kMaxNbr; ++k) neighbors[k] = -1;
  auto tile_of = [&](int64_t k) {  // the table holds tile slots of the particle's block
    const int* b = tb.data() + 6 * (k / kTileW);
    return Tile{b[0], b[1] - b[0], b[2], b[3] - b[2], b[4], b[5] - b[4]};
  };
  bool any_big = false;  // a block whose tile exceeds 16-bit slots: the 32-bit table holds -(index + 1)
  for (int64_t b = 0; b < nblocks; ++b) {
    const Tile tl = tile_of(b * kTileW);
    any_big |= tl.n0 + tl.n1 + tl.n2 > kRowSlotMax;
  }
  for (int s = 0; s < kMaxNbr && neighbors; ++s) {
    if (any_big) {
      if ((rc = fetch(c, slot.data(), c->nbr + (size_t)s * c->cap, n * sizeof(int)))) return rc;
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    for (int64_t k = 0; k < n; ++k) {
      if (s >= row_count(rows[k])) continue;
      const Tile tl = tile_of(k);
      const bool big = tl.n0 + tl.n1 + tl.n2 > kRowSlotMax;
      neighbors[k * kMaxNbr + s] = id[entry_index(tl, big ? slot[k] : row_entry(rows[k], s))];
    }
  }
  for (int64_t k = 0; k < n; ++k) {
    if (ids) ids[k] = id[k];
    if (counts) counts[k] = (int32_t)row_count(rows[k]);
    if (fixed_xy) {
      fixed_xy[2 * k] = hxy[2 * k];
      fixed_xy[2 * k + 1] = hxy[2 * k + 1];
    }
  }
  return SC_OK;
}

int sc_download_normals(sc_ctx* c, double* sxy, int64_t room, int64_t* n_out) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step || !c->normals_valid) return fail(SC_ERR_STATE, "sc_download_normals needs a finished tick");
  int h[C_COUNT];
  int rc = read_counters(c, h);
  if (rc) return rc;
  int64_t n = h[C_NT];
  if (n_out) *n_out = n;
  if (n > room) return fail(SC_ERR_CAPACITY, "host arrays too small");
  std::vector<double> ab(2 * n);
  std::vector<int> id(n);
  if ((rc = fetch(c, ab.data(), c->snn, 2 * n * sizeof(double))) || (rc = fetch(c, id.data(), c->id[1], n * sizeof(int))))
    return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  write_pairs(sxy, index_order(id.data(), nullptr, n), ab.data(), ab.data() + 1, 2);
  return SC_OK;
}

// ---- stand-alone reference functions ----------------------------------------------------------

int sc_neighbor_search(int device, const double* xy, int64_t n, double diameter, int64_t* y_floored,
                       int64_t* sorted_indices, int32_t* counts, int64_t* table) {
  if (n < 0 || (n > 0 && !xy) || !(diameter > 0)) return fail(SC_ERR_ARG, "bad arguments");
  if (n == 0) return SC_OK;
  // the grid comes from the data's bounding box; the search itself runs on the device
  double xmin = xy[0], xmax = xy[0], ymin = xy[1], ymax = xy[1];
  for (int64_t i = 0; i < n; ++i) {
    double px = xy[2 * i], py = xy[2 * i + 1];
    if (!std::isfinite(px) || !std::isfinite(py)) return fail(SC_ERR_DOMAIN, "non-finite coordinate at %lld", (long long)i);
    xmin = std::min(xmin, px);
    xmax = std::max(xmax, px);
    ymin = std::min(ymin, py);
    ymax = std::max(ymax, py);
  }
  double c0 = std::floor(xmin / diameter), c1 = std::floor(xmax / diameter);
  double r0 = std::floor(ymin / diameter), r1 = std::floor(ymax / diameter);
  if (!(std::fabs(c0) < 4e15 && std::fabs(c1) < 4e15 && std::fabs(r0) < 4e15 && std::fabs(r1) < 4e15))
    return fail(SC_ERR_DOMAIN, "coordinates too large for the diameter");
  double ncols = c1 - c0 + 3, nrows = r1 - r0 + 3;
  if (ncols * nrows > (double)((int64_t)1 << 27))
    return fail(SC_ERR_CAPACITY, "bounding box of %.0f x %.0f cells is too sparse for a uniform grid", nrows, ncols);
  sc_ctx* c = nullptr;
  int rc = sc_create(device, n, &c);
  if (rc) return rc;
  c->custom_grid = true;
  c->force_rank_big = true;  // no previous tick to take the hint from
  c->custom_d = diameter;
  c->grid_row0 = (long long)r0 - 1;
  c->grid_col0 = (long long)c0 - 1;
  c->grid_nrows = (int)nrows;
  c->grid_ncols = (int)ncols;
  std::vector<double> zero(2 * n, 0.0);
  std::vector<int64_t> ids(n), nb((size_t)n * kMaxNbr);
  std::vector<int32_t> cn(n);
  int64_t got = 0;
  if ((rc = sc_upload_state(c, xy, zero.data(), n)) == SC_OK && (rc = sc_step_begin(c)) == SC_OK &&
      (rc = sc_download_sort(c, y_floored, sorted_indices, n, &got)) == SC_OK &&
      (rc = sc_download_neighbors(c, ids.data(), cn.data(), nb.data(), nullptr, n, &got)) == SC_OK) {
    if (got != n) {
      rc = fail(SC_ERR_DOMAIN, "%lld of %lld particles were binned", (long long)got, (long long)n);
    } else {
      for (int64_t k = 0; k < n; ++k) {
        int64_t i = ids[k];
        if (counts) counts[i] = cn[k];
        if (table) std::memcpy(table + i * kMaxNbr, nb.data() + k * kMaxNbr, kMaxNbr * sizeof(int64_t));
      }
    }
  }
  std::string keep = g_err;
  sc_destroy(c);
  g_err = keep;
  return rc;
}

// geometry_utils.py:146-172 (pad_segments) on the host, operation for operation: o = cw90(b - a) * pad / |b - a| with the
// norm as np.linalg.norm takes it for two components (sqrt of the sum of the squares, separately rounded -- this file is
// compiled with -ffp-contract=off); first every (a + o, b + o), then every (b - o, a - o).  In the library because the
// padded twins of a moving wall are needed every tick and the NumPy form of these thirty operations costs the host 15-25 us.
int sc_pad_segments(const double* segments, int32_t ns, double pad_distance, double* padded) {
  if (ns < 0 || (ns > 0 && (!segments || !padded))) return fail(SC_ERR_ARG, "bad arguments");
  for (int k = 0; k < ns; ++k) {
    const double ax = segments[4 * k], ay = segments[4 * k + 1], bx = segments[4 * k + 2], by = segments[4 * k + 3];
    const double alx = bx - ax, aly = by - ay;
    const double nx = aly, ny = -alx;  // clockwise quarter turn of (end - start)
    const double norm = std::sqrt(nx * nx + ny * ny);
    const double ox = nx * pad_distance / norm, oy = ny * pad_distance / norm;
    double* plus = padded + 4 * k;
    double* minus = padded + 4 * (ns + k);
    plus[0] = ax + ox; plus[1] = ay + oy; plus[2] = bx + ox; plus[3] = by + oy;
    minus[0] = bx - ox; minus[1] = by - oy; minus[2] = ax - ox; minus[3] = ay - oy;
  }
  return SC_OK;
}

int sc_points_to_segments(int device, const double* xy, int64_t n, const double* segments, int32_t ns, double* nearest,
                          double* distances) {
  if (n < 0 || ns < 0 || (n > 0 && !xy) || (ns > 0 && !segments)) return fail(SC_ERR_ARG, "bad arguments");
  if (n == 0 || ns == 0) return SC_OK;
  HIPCHK(hipSetDevice(device));
  DevBuf<double> dxy, dseg, dnear, ddist;
  const int64_t t = n * ns;
  hipError_t e = dxy.grow(2 * n, nullptr);
  if (e == hipSuccess) e = dseg.grow(4 * ns, nullptr);
  if (e == hipSuccess) e = dnear.grow(2 * t, nullptr);
  if (e == hipSuccess) e = ddist.grow(t, nullptr);
  if (e == hipSuccess) e = hipMemcpy(dxy, xy, 2 * n * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dseg, segments, 4 * ns * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_points_to_segments, dim3((unsigned)((t + kBlock - 1) / kBlock)), dim3(kBlock), 0, 0, dxy, (int)n,
                       dseg, (int)ns, dnear, ddist);
    e = hipGetLastError();
  }
  if (e == hipSuccess && nearest) e = hipMemcpy(nearest, dnear, 2 * t * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && distances) e = hipMemcpy(distances, ddist, t * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(SC_ERR_HIP, "sc_points_to_segments: %s", hipGetErrorString(e));
  return SC_OK;
}


// ---- multi-GPU slabs ---------------------------------------------------------------------------

int sc_set_slab_axis(sc_ctx* c, int32_t axis) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "slab cannot change inside a tick");
  if (axis != 0 && axis != 1) return fail(SC_ERR_ARG, "slab axis: 0 (columns of x) or 1 (rows of y)");
  c->slab_axis = axis;
  c->halo_ring_from = c->tick;
  return SC_OK;
}

int sc_set_slab(sc_ctx* c, int64_t col_lo, int64_t col_hi, int32_t halo, int32_t has_left, int32_t has_right) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "slab cannot change inside a tick");
  if (col_hi <= col_lo || halo < 3) return fail(SC_ERR_ARG, "slab needs col_lo < col_hi and a halo of at least 3 columns");
  c->slab = true;
  c->own_lo = col_lo;
  c->own_hi = col_hi;
  c->halo = halo;
  c->has_left = has_left ? 1 : 0;
  c->has_right = has_right ? 1 : 0;
  c->halo_ring_from = c->tick;  // new cuts: the halo counts of earlier ticks say nothing about the coming ones
  HIPCHK(c->owned_out.grow(1, c->stream));
  return SC_OK;
}

// Records a halo message of tick `tick` carries, from the count the same direction had `kHaloLag` ticks earlier
// (+50 % and 1024 records of headroom, in steps of 256).  Sender and receiver evaluate this on the same number:
// the sender published what it packed, the receiver what the header it received said.
static int64_t halo_message_records(int64_t count, int64_t cap) {
  const int64_t want = count + count / 2 + 1024;
  return std::min<int64_t>(cap, (want + 255) / 256 * 256);
}

int sc_halo_sizes(sc_ctx* c, int64_t cap_records, int64_t* send_left, int64_t* recv_left, int64_t* send_right,
                  int64_t* recv_right) {
  if (!c || !send_left || !recv_left || !send_right || !recv_right || cap_records < 1) return fail(SC_ERR_ARG, "bad arguments");
  if (!c->slab) return fail(SC_ERR_STATE, "sc_set_slab first");
  constexpr int64_t kHaloLag = 6;  // more than the ticks the host may run ahead of the device (sc_step_begin)
  static_assert(kHaloLag < kHaloRing, "the ring must still hold the tick the sizes come from");
  *send_left = *recv_left = *send_right = *recv_right = cap_records;
  const int64_t src = c->tick - kHaloLag;
  if (src < c->halo_ring_from) return SC_OK;  // no history yet: whole buffers
  // tick `src` has finished on the device (at most a few ticks are ever queued), so its counts are published
  const int rc = wait_ticks_finished(c, src + 1, "halo counts");
  if (rc) return rc;
  if (progress_read(c, kProgressTicks) <= src) return SC_OK;  // counter behind (fresh upload): whole buffers
  const int ring = kProgressHaloRing + 4 * (int)(src % kHaloRing);
  *send_left = halo_message_records(progress_read(c, ring), cap_records);
  *send_right = halo_message_records(progress_read(c, ring + 1), cap_records);
  *recv_left = halo_message_records(progress_read(c, ring + 2), cap_records);
  *recv_right = halo_message_records(progress_read(c, ring + 3), cap_records);
  return SC_OK;
}

int sc_column_histogram(sc_ctx* c, int64_t col0, int32_t ncols, int64_t* hist) {
  if (!c || !hist || ncols < 1) return fail(SC_ERR_ARG, "bad arguments");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_column_histogram inside a tick");
  if (!c->have_params && !c->custom_grid) return fail(SC_ERR_STATE, "sc_set_params has not been called");
  HIPCHK(hipSetDevice(c->device));
  if (ncols > c->colHist.size()) HIPCHK(c->colHist.grow(ncols + 256, c->stream));
  HIPCHK(hipMemsetAsync(c->colHist, 0, ncols * sizeof(int), c->stream));
  const double d = c->custom_grid ? c->custom_d : c->now.params.particle_radius * 2;
  hipLaunchKernelGGL(k_column_histogram, dim3(grid_for(launch_bound(c))), dim3(kBlock), 0, c->stream, c->counters, c->x,
                     c->slab_axis ? c->y : c->x, d, (long long)col0, (int)ncols, c->colHist);
  std::vector<int> h(ncols);
  HIPCHK(hipMemcpyAsync(h.data(), c->colHist, ncols * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < ncols; ++k) hist[k] = h[k];
  return SC_OK;
}

int sc_upload_state_ids(sc_ctx* c, const double* xy, const double* vxy, const int64_t* ids, int64_t n) {
  if (!c || (n > 0 && !ids)) return fail(SC_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(c->device));
  return put_particles(c, xy, vxy, n, true, ids);
}

int sc_append_particles_ids(sc_ctx* c, const double* xy, const double* vxy, const int64_t* ids, int64_t n) {
  if (!c || (n > 0 && !ids)) return fail(SC_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(c->device));
  return put_particles(c, xy, vxy, n, false, ids);
}

int sc_halo_pack(sc_ctx* c, double* dev_left, double* dev_right, int64_t cap_records) {
  if (!c || !dev_left || !dev_right || cap_records < 1) return fail(SC_ERR_ARG, "bad halo buffers");
  if (!c->slab) return fail(SC_ERR_STATE, "sc_set_slab first");
  if (c->in_step) return fail(SC_ERR_STATE, "halo exchange happens between ticks");
  int rc = make_world(c);
  if (rc) return rc;
  if (c->prebinned) return fail(SC_ERR_STATE, "the halo message of the promised tick was packed by sc_step_finish");
  c->band_pending = false;  // this message depends on the kernel below, not on a split force kernel
  c->haloL = dev_left;  // stay bound: with sc_set_next_inputs, sc_step_finish packs the next message itself
  c->haloR = dev_right;
  c->haloCap = (int)cap_records;
  Bracket br(c, K_HALO_PACK);
  hipLaunchKernelGGL(k_halo_pack, dim3(grid_for(launch_bound(c))), dim3(kBlock), 0, c->stream, c->w, c->counters, c->x,
                     c->y, c->vx, c->vy, c->id[0], dev_left, dev_right, (int)cap_records, (int)c->cap);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

int sc_halo_unpack(sc_ctx* c, const double* from_left, int64_t left_records, const double* from_right,
                   int64_t right_records) {
  if (!c || (!from_left && !from_right) || (from_left && left_records < 1) || (from_right && right_records < 1))
    return fail(SC_ERR_ARG, "bad halo buffers");
  if (!c->slab) return fail(SC_ERR_STATE, "sc_set_slab first");
  if (c->in_step) return fail(SC_ERR_STATE, "halo exchange happens between ticks");
  Bracket br(c, K_HALO_UNPACK);
  const int capL = from_left ? (int)left_records : 0, capR = from_right ? (int)right_records : 0;
  const dim3 grid(grid_for(capL + capR)), block(kBlock);
  int* ring = c->progress_dev + kProgressHaloRing + 4 * (int)(c->tick % kHaloRing);
  if (c->prebinned) {  // the stored particles went through K1 of the coming tick in pass B: same for the arrivals
    hipLaunchKernelGGL(k_halo_unpack<true>, grid, block, 0, c->stream, from_left, from_right, capL, capR,
                       c->counters, c->x, c->y, c->vx, c->vy, c->id[0], (int)c->cap, c->haloL, c->haloR,
                       c->promised, c->cellS, c->wslotS, c->cellCount, c->wrec[c->tick & 1], ring);
  } else {
    const int rc = make_world(c);  // (the slab and the diameter the records are judged by)
    if (rc) return rc;
    const WallInputs none = wall_inputs_of(c->w);
    hipLaunchKernelGGL(k_halo_unpack<false>, grid, block, 0, c->stream, from_left, from_right, capL, capR,
                       c->counters, c->x, c->y, c->vx, c->vy, c->id[0], (int)c->cap, c->haloL, c->haloR, none,
                       c->cellS, c->wslotS, c->cellCount, c->wrec[c->tick & 1], ring);
  }
  HIPCHK(hipGetLastError());
  return SC_OK;
}

#define RCCLCHK(expr)                                                                       \
  do {                                                                                      \
    int rc_ = (expr);                                                                       \
    if (rc_ != 0) return fail(SC_ERR_HIP, "RCCL: %s failed: %s", #expr, rccl_error(rc_)); \
  } while (0)

static int ensure_side_stream(sc_ctx* c) {
  if (!c->side_stream) HIPCHK(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
  // (device-side ordering only: without the system-scope fence an event between two kernels costs ~1 us instead of ~10)
  if (!c->ev_band) HIPCHK(hipEventCreateWithFlags(&c->ev_band, hipEventDisableTiming | hipEventDisableSystemFence));
  // (ev_xchg orders halo buffers that a peer GPU wrote: it keeps the system-scope fence)
  if (!c->ev_xchg) HIPCHK(hipEventCreateWithFlags(&c->ev_xchg, hipEventDisableTiming));
  return SC_OK;
}

int sc_set_halo_overlap(sc_ctx* c, int on) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "halo overlap cannot change inside a tick");
  if (on && !c->slab) return fail(SC_ERR_STATE, "sc_set_slab first");
  HIPCHK(hipSetDevice(c->device));
  if (on) {
    int rc = ensure_side_stream(c);
    if (rc) return rc;
  }
  c->overlap = on != 0;
  return SC_OK;
}

int sc_set_band_flag(sc_ctx* c, int on) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "the band mode cannot change inside a tick");
  c->band_by_flag = on != 0;  // (a band that is pending keeps the announcement it was launched with: band_flagged)
  return SC_OK;
}

int sc_side_stream(sc_ctx* c, void** stream) {
  if (!c || !stream) return fail(SC_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(c->device));
  int rc = ensure_side_stream(c);
  if (rc) return rc;
  *stream = (void*)c->side_stream;
  return SC_OK;
}

// side stream <- everything the halo message of the coming tick depends on (the band blocks of pass B when the last
// tick packed it, else all work queued so far); `peer`: also what that context's message depends on
int sc_halo_overlap_begin(sc_ctx* c, sc_ctx* peer) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  HIPCHK(hipSetDevice(c->device));
  int rc = ensure_side_stream(c);
  if (rc) return rc;
  for (sc_ctx* q : {c, peer}) {
    if (!q) continue;
    if (q != c && (rc = ensure_side_stream(q))) return rc;
    if (q->band_pending && q->band_flagged) {  // the window blocks of q's one-launch force kernel
      hipLaunchKernelGGL(k_wait_band, dim3(1), dim3(1), 0, c->side_stream, q->counters, q->band_epoch);
      continue;
    }
    if (!q->band_pending) HIPCHK(hipEventRecord(q->ev_band, q->stream));  // no split pass B before: wait for all of it
    HIPCHK(hipStreamWaitEvent(c->side_stream, q->ev_band, 0));
  }
  return SC_OK;
}

// context's stream <- what was enqueued on the side stream since sc_halo_overlap_begin (the received buffers)
int sc_halo_overlap_end(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!c->side_stream || !c->ev_xchg) return fail(SC_ERR_STATE, "sc_halo_overlap_begin first");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventRecord(c->ev_xchg, c->side_stream));
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_xchg, 0));
  c->band_pending = false;
  return SC_OK;
}

int sc_comm_available(const char* rccl_path) {
  if (rccl_load(rccl_path)) return fail(SC_ERR_HIP, "%s", rccl_api().error.c_str());
  return SC_OK;
}

int sc_comm_unique_id(const char* rccl_path, void* id) {
  if (!id) return fail(SC_ERR_ARG, "null argument");
  if (rccl_load(rccl_path)) return fail(SC_ERR_HIP, "%s", rccl_api().error.c_str());
  RcclUniqueId u;
  RCCLCHK(rccl_api().GetUniqueId(&u));
  std::memcpy(id, &u, sizeof u);
  return SC_OK;
}

int sc_comm_init(sc_ctx* c, const char* rccl_path, const void* id, int32_t rank, int32_t world) {
  if (!c || !id) return fail(SC_ERR_ARG, "null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail(SC_ERR_ARG, "rank %d of %d", rank, world);
  if (c->comm) return fail(SC_ERR_STATE, "sc_comm_init called twice");
  if (rccl_load(rccl_path)) return fail(SC_ERR_HIP, "%s", rccl_api().error.c_str());
  HIPCHK(hipSetDevice(c->device));
  RcclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  RCCLCHK(rccl_api().CommInitRank(&c->comm, world, u, rank));
  c->comm_rank = rank;
  c->comm_world = world;
  return SC_OK;
}

int sc_comm_destroy(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!c->comm) return SC_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  RcclComm comm = c->comm;
  c->comm = nullptr;
  RCCLCHK(rccl_api().CommDestroy(comm));
  return SC_OK;
}

int sc_halo_exchange(sc_ctx* c, const double* send_left, int64_t send_left_records, double* recv_left,
                     int64_t recv_left_records, int32_t left_rank, const double* send_right, int64_t send_right_records,
                     double* recv_right, int64_t recv_right_records, int32_t right_rank) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!c->comm) return fail(SC_ERR_STATE, "sc_comm_init first");
  if (c->in_step) return fail(SC_ERR_STATE, "halo exchange happens between ticks");
  if ((left_rank >= 0 && (!send_left || !recv_left || left_rank >= c->comm_world || send_left_records < 1 || recv_left_records < 1)) ||
      (right_rank >= 0 && (!send_right || !recv_right || right_rank >= c->comm_world || send_right_records < 1 || recv_right_records < 1)))
    return fail(SC_ERR_ARG, "neighbor ranks %d / %d need their buffers and record counts and must be below %d", left_rank,
                right_rank, c->comm_world);
  auto doubles = [](int64_t records) { return (size_t)(records + 1) * kHaloFields; };  // + the header record
  const RcclApi& r = rccl_api();
  HIPCHK(hipSetDevice(c->device));
  hipStream_t xs = c->stream;
  if (c->overlap) {  // on the side stream, next to the interior blocks of the last pass B
    int rc0 = sc_halo_overlap_begin(c, nullptr);
    if (rc0) return rc0;
    xs = c->side_stream;
  }
  RCCLCHK(r.GroupStart());
  int rc = 0;
  // posting order is the same on every rank (left pair, then right pair): rank k's right pair meets rank k+1's left pair
  if (left_rank >= 0) {
    if (!rc) rc = r.Send(send_left, doubles(send_left_records), kRcclDouble, left_rank, c->comm, xs);
    if (!rc) rc = r.Recv(recv_left, doubles(recv_left_records), kRcclDouble, left_rank, c->comm, xs);
  }
  if (right_rank >= 0) {
    if (!rc) rc = r.Send(send_right, doubles(send_right_records), kRcclDouble, right_rank, c->comm, xs);
    if (!rc) rc = r.Recv(recv_right, doubles(recv_right_records), kRcclDouble, right_rank, c->comm, xs);
  }
  const int rc_end = r.GroupEnd();
  if (rc) return fail(SC_ERR_HIP, "RCCL: send/recv failed: %s", rccl_error(rc));
  if (rc_end) return fail(SC_ERR_HIP, "RCCL: ncclGroupEnd failed: %s", rccl_error(rc_end));
  if (c->overlap) return sc_halo_overlap_end(c);
  return SC_OK;
}

int sc_owned_count(sc_ctx* c, int64_t* n) {
  if (!c || !n) return fail(SC_ERR_ARG, "null argument");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_owned_count inside a tick");
  int rc = c->slab ? make_world(c) : SC_OK;
  if (rc) return rc;
  HIPCHK(c->owned_out.grow(1, c->stream));
  HIPCHK(hipMemsetAsync(c->owned_out, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(k_owned_count, dim3(grid_for(launch_bound(c))), dim3(kBlock), 0, c->stream, c->counters, c->x,
                     c->owned_out);
  int h = 0;
  HIPCHK(hipMemcpyAsync(&h, c->owned_out, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *n = h;
  return SC_OK;
}

// ---- tracking -------------------------------------------------------------------------------------

int sc_track_bound(int64_t n, int32_t n_segments, int64_t* bytes) {
  if (!bytes) return fail(SC_ERR_ARG, "null argument");
  if (n < 0 || n > (int64_t)100000000) return fail(SC_ERR_ARG, "%lld particles", (long long)n);
  if (n_segments < 0 || n_segments > kMaxSeg) return fail(SC_ERR_ARG, "%d segments; 0..%d", n_segments, kMaxSeg);
  *bytes = track_planes(n, n_segments).end;
  return SC_OK;
}

int sc_track_capture(sc_ctx* c, uint8_t* out, int64_t room, int64_t* n_bytes) {
  if (!c || !n_bytes || room < 0 || (room > 0 && !out)) return fail(SC_ERR_ARG, "null argument or negative room");
  *n_bytes = 0;
  int rc = track_refuse(c, false);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  if ((rc = track_ensure(c))) return rc;
  HIPCHK(c->trackNow.grow(track_planes(std::min<int64_t>(launch_bound(c), c->cap), c->now.nseg).end, c->stream));
  if ((rc = track_launch(c, false))) return rc;
  unsigned long long words[TW_COUNT];
  HIPCHK(hipMemcpyAsync(words, c->trackWords, sizeof words, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int64_t bytes = track_planes((int64_t)words[TW_N], c->now.nseg).end;
  if ((long long)words[TW_AT] < 0)
    return fail(SC_ERR_HIP, "the device stores %lld particles, more than the host's bound", (long long)words[TW_N]);
  *n_bytes = bytes;
  if (bytes > room) return fail(SC_ERR_CAPACITY, "a frame of %lld bytes, room for %lld", (long long)bytes, (long long)room);
  HIPCHK(hipMemcpyAsync(out, c->trackNow, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return SC_OK;
}

int sc_track_enable(sc_ctx* c, int64_t every, int64_t capacity_bytes) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (every < 1) return fail(SC_ERR_ARG, "every %lld; at least 1", (long long)every);
  if (capacity_bytes < 1 || capacity_bytes > ((int64_t)1 << 40))
    return fail(SC_ERR_ARG, "a log of %lld bytes; 1..2^40", (long long)capacity_bytes);
  int rc = track_refuse(c, true);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  if ((rc = track_ensure(c))) return rc;
  c->track_on = false;  // (a call that fails below leaves no log)
  HIPCHK(c->trackLog.grow(track_pad8(capacity_bytes), c->stream));
  HIPCHK(hipMemsetAsync(c->trackWords, 0, c->trackWords.bytes(), c->stream));
  c->track_every = every;
  c->track_cap = capacity_bytes;
  c->track_on = true;
  return SC_OK;
}

int sc_track_disable(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  const int rc = track_refuse(c, true);
  if (rc) return rc;
  c->track_on = false;
  return SC_OK;
}

int sc_track_read(sc_ctx* c, uint8_t* out, int64_t room, int64_t* n_bytes, int64_t* n_frames, int64_t* dropped) {
  if (!c || !n_bytes || !n_frames || !dropped || room < 0 || (room > 0 && !out))
    return fail(SC_ERR_ARG, "null argument or negative room");
  *n_bytes = *n_frames = *dropped = 0;
  const int rc = track_refuse(c, false);
  if (rc) return rc;
  if (!c->track_on) return fail(SC_ERR_STATE, "sc_track_enable first");
  unsigned long long words[TW_COUNT];
  HIPCHK(hipMemcpyAsync(words, c->trackWords, sizeof words, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int64_t bytes = std::min<int64_t>((int64_t)words[TW_CURSOR], c->track_cap);
  *n_bytes = bytes;
  if (bytes > room)  // nothing is delivered and nothing forgotten
    return fail(SC_ERR_CAPACITY, "%lld bytes logged, room for %lld", (long long)bytes, (long long)room);
  if (bytes > 0) {
    HIPCHK(hipMemcpyAsync(out, c->trackLog, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  *n_frames = (int64_t)words[TW_FRAMES];
  *dropped = (int64_t)words[TW_DROPPED];
  HIPCHK(hipMemsetAsync(c->trackWords, 0, c->trackWords.bytes(), c->stream));  // the log starts over
  return SC_OK;
}

int sc_track_load(sc_ctx* c, const uint8_t* frame, int64_t n_bytes, int32_t plain) {
  if (!c || !frame) return fail(SC_ERR_ARG, "null argument");
  if (c->slab) return fail(SC_ERR_STATE, "tracking is not available in slab mode");
  if (c->in_step) return fail(SC_ERR_STATE, "particles cannot change between sc_step_begin and sc_step_finish");
  if (n_bytes < kTrackHeaderBytes) return fail(SC_ERR_ARG, "%lld bytes are no frame", (long long)n_bytes);
  uint32_t magic, version;
  int64_t n;
  int32_t nseg;
  double lo, span;
  std::memcpy(&magic, frame, 4);
  std::memcpy(&version, frame + 4, 4);
  std::memcpy(&n, frame + 16, 8);
  std::memcpy(&nseg, frame + 24, 4);
  std::memcpy(&lo, frame + 32, 8);
  std::memcpy(&span, frame + 40, 8);
  if (magic != kTrackMagic) return fail(SC_ERR_ARG, "not a track frame (magic %08x)", magic);
  if (version != kTrackVersion) return fail(SC_ERR_ARG, "track frame of version %u; this library reads %u", version, kTrackVersion);
  if (n < 0) return fail(SC_ERR_ARG, "a frame of %lld particles", (long long)n);
  if (nseg < 0 || nseg > kMaxSeg) return fail(SC_ERR_ARG, "a frame of %d segments; 0..%d", nseg, kMaxSeg);
  if (n > c->cap)
    return fail(SC_ERR_CAPACITY, "%lld particles exceed the context capacity %lld", (long long)n, (long long)c->cap);
  const TrackPlanes pl = track_planes(n, nseg);
  if (n_bytes != pl.end) return fail(SC_ERR_ARG, "%lld bytes; a frame of %lld particles and %d segments has %lld",
                                     (long long)n_bytes, (long long)n, nseg, (long long)pl.end);
  if (!(std::isfinite(lo) && std::isfinite(span) && span > 0)) return fail(SC_ERR_ARG, "the frame's coordinate range is not finite");
  int64_t max_id = -1;
  for (int64_t k = 0; k < n; ++k) {
    uint32_t v;
    std::memcpy(&v, frame + pl.id + 4 * k, 4);
    if (v > (uint32_t)std::numeric_limits<int>::max() - 1) return fail(SC_ERR_ARG, "particle id out of range");
    max_id = std::max<int64_t>(max_id, v);
  }
  HIPCHK(hipSetDevice(c->device));
  if (c->prebinned) {
    const int rc = abandon_promise(c);
    if (rc) return rc;
  }
  c->pairs_valid = false;
  HIPCHK(c->trackLoad.grow(n_bytes, c->stream));
  HIPCHK(hipMemcpyAsync(c->trackLoad, frame, (size_t)n_bytes, hipMemcpyHostToDevice, c->stream));
  TrackLoad a{};
  a.n = (int)n;
  a.nseg = nseg;
  a.plain = plain ? 1 : 0;
  a.next_id = (int)(max_id + 1);
  a.lo = lo;
  a.step = span / kTrackCodes;
  hipLaunchKernelGGL(k_track_unpack, dim3(grid_for(n)), dim3(kBlock), 0, c->stream, a, c->trackLoad, c->counters, c->x, c->y,
                     c->vx, c->vy, c->id[0], c->P);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));  // `frame` is the caller's: read before we return
  c->upper = n;
  c->next_id = max_id + 1;
  c->normals_valid = 1;  // every slot carries the pressure its colour stands for
  c->halo_ring_from = c->tick;
  c->live_hint_from = c->tick;
  return SC_OK;
}

// ---- the probe ----------------------------------------------------------------------------------

int sc_probe_now(sc_ctx* c, int32_t n_bins, double x0, double x1, double* row16, int32_t* counts, double* tops) {
  if (!c || !row16) return fail(SC_ERR_ARG, "null argument");
  int rc = probe_check_bins(n_bins, x0, x1);
  if (rc) return rc;
  if (n_bins > 0 && (!counts || !tops)) return fail(SC_ERR_ARG, "null profile arrays");
  if (c->slab) return fail(SC_ERR_STATE, "the probe is not available in slab mode");
  if (c->in_step) return fail(SC_ERR_STATE, "measuring happens between ticks");
  HIPCHK(hipSetDevice(c->device));
  if ((rc = probe_ensure(c))) return rc;
  std::vector<unsigned long long> keys((size_t)n_bins);
  if (n_bins > 0) {
    HIPCHK(hipMemsetAsync(c->probeNowCounts, 0, (size_t)n_bins * sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(c->probeNowTops, 0xFF, (size_t)n_bins * sizeof(unsigned long long), c->stream));
  }
  if ((rc = probe_launch(c, false, n_bins, x0, x1))) return rc;
  HIPCHK(hipMemcpyAsync(row16, c->probeNowRow, kProbeFields * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (n_bins > 0) {
    HIPCHK(hipMemcpyAsync(counts, c->probeNowCounts, (size_t)n_bins * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(keys.data(), c->probeNowTops, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  probe_decode_tops(keys.data(), tops, n_bins);
  return SC_OK;
}

int sc_probe_enable(sc_ctx* c, int64_t capacity_rows, int32_t n_bins, double x0, double x1) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (capacity_rows < 1 || capacity_rows > (int64_t)1 << 20)
    return fail(SC_ERR_ARG, "a log of %lld rows; 1..1048576", (long long)capacity_rows);
  int rc = probe_check_bins(n_bins, x0, x1);
  if (rc) return rc;
  if (c->slab) return fail(SC_ERR_STATE, "the probe is not available in slab mode");
  if (c->in_step) return fail(SC_ERR_STATE, "the probe's log cannot change inside a tick");
  if (c->prebinned) return fail(SC_ERR_STATE, "the probe's log cannot change after sc_set_next_inputs promised the next tick");
  HIPCHK(hipSetDevice(c->device));
  if ((rc = probe_ensure(c))) return rc;
  c->probe_on = false;  // (a call that fails below leaves no log)
  HIPCHK(c->probeRows.grow(capacity_rows * kProbeFields, c->stream));
  HIPCHK(c->probeCounts.grow(capacity_rows * n_bins, c->stream));
  HIPCHK(c->probeTops.grow(capacity_rows * n_bins, c->stream));
  if (n_bins > 0) {
    HIPCHK(hipMemsetAsync(c->probeCounts, 0, (size_t)capacity_rows * n_bins * sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(c->probeTops, 0xFF, (size_t)capacity_rows * n_bins * sizeof(unsigned long long), c->stream));
  }
  HIPCHK(hipMemsetAsync(c->probeWords, 0, c->probeWords.bytes(), c->stream));
  c->probe_cap = capacity_rows;
  c->probe_tail = 0;
  c->probe_bins = n_bins;
  c->probe_x0 = x0;
  c->probe_x1 = x1;
  c->probe_on = true;
  return SC_OK;
}

int sc_probe_disable(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->slab) return fail(SC_ERR_STATE, "the probe is not available in slab mode");
  if (c->in_step) return fail(SC_ERR_STATE, "the probe's log cannot change inside a tick");
  if (c->prebinned) return fail(SC_ERR_STATE, "the probe's log cannot change after sc_set_next_inputs promised the next tick");
  c->probe_on = false;
  return SC_OK;
}

int sc_probe_read(sc_ctx* c, double* rows, int32_t* counts, double* tops, int64_t room, int64_t* n_out, int64_t* n_dropped) {
  if (!c || !n_out || !n_dropped) return fail(SC_ERR_ARG, "null argument");
  if (room < 0) return fail(SC_ERR_ARG, "room for %lld rows", (long long)room);
  if (room > 0 && (!rows || (c->probe_on && c->probe_bins > 0 && (!counts || !tops)))) return fail(SC_ERR_ARG, "null arrays");
  if (c->slab) return fail(SC_ERR_STATE, "the probe is not available in slab mode");
  if (c->in_step) return fail(SC_ERR_STATE, "the log is read between ticks");
  if (!c->probe_on) return fail(SC_ERR_STATE, "sc_probe_enable first");
  HIPCHK(hipSetDevice(c->device));
  int words[PW_COUNT];
  HIPCHK(hipMemcpyAsync(words, c->probeWords, sizeof words, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int64_t head = std::min<int64_t>(words[PW_HEAD], c->probe_cap), tail = std::min(c->probe_tail, head);
  const int64_t m = std::min(head - tail, room);
  const size_t nb = (size_t)c->probe_bins;
  if (m > 0) {
    HIPCHK(hipMemcpyAsync(rows, c->probeRows + tail * kProbeFields, (size_t)m * kProbeFields * sizeof(double),
                          hipMemcpyDeviceToHost, c->stream));
    std::vector<unsigned long long> keys((size_t)m * nb);
    if (nb > 0) {
      HIPCHK(hipMemcpyAsync(counts, c->probeCounts + tail * nb, (size_t)m * nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(keys.data(), c->probeTops + tail * nb, keys.size() * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    probe_decode_tops(keys.data(), tops, (int64_t)keys.size());
  }
  c->probe_tail = tail + m;
  if (c->probe_tail == head) {  // all of it has been read: the log starts over, its bins empty
    if (nb > 0 && head > 0) {
      HIPCHK(hipMemsetAsync(c->probeCounts, 0, (size_t)head * nb * sizeof(int), c->stream));
      HIPCHK(hipMemsetAsync(c->probeTops, 0xFF, (size_t)head * nb * sizeof(unsigned long long), c->stream));
    }
    HIPCHK(hipMemsetAsync(c->probeWords + PW_HEAD, 0, sizeof(int), c->stream));
    c->probe_tail = 0;
  }
  if (words[PW_DROPPED]) HIPCHK(hipMemsetAsync(c->probeWords + PW_DROPPED, 0, sizeof(int), c->stream));
  *n_out = m;
  *n_dropped = words[PW_DROPPED];
  return SC_OK;
}

// ---- force monitor ------------------------------------------------------------------------------

int sc_enable_force_monitor(sc_ctx* c, int on) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "the force monitor cannot change inside a tick");
  if (c->prebinned) return fail(SC_ERR_STATE, "the force monitor cannot change after sc_set_next_inputs promised the next tick");
  HIPCHK(hipSetDevice(c->device));
  if (on) HIPCHK(c->monitor.grow(kMonPhases + 1, c->stream));
  if (on) HIPCHK(hipMemsetAsync(c->monitor, 0, (kMonPhases + 1) * sizeof(double), c->stream));
  c->monitor_on = on != 0;
  return SC_OK;
}

int sc_get_force_monitor(sc_ctx* c, double* sums, int64_t* particles) {
  if (!c || !sums || !particles) return fail(SC_ERR_ARG, "null argument");
  if (!c->monitor_on) return fail(SC_ERR_STATE, "sc_enable_force_monitor first");
  double h[kMonPhases + 1];
  HIPCHK(hipMemcpyAsync(h, c->monitor, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemsetAsync(c->monitor, 0, sizeof h, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < kMonPhases; ++k) sums[k] = h[k];
  *particles = (int64_t)h[kMonPhases];
  return SC_OK;
}

// ---- checkpoint ---------------------------------------------------------------------------------
// The stored state is copied device-to-device on the context's stream (a few microseconds), the copy travels to
// pinned host memory on a side stream, and the ticks that follow run meanwhile; sc_checkpoint_finish waits for the
// side stream only.

int sc_checkpoint_begin(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_checkpoint_begin inside a tick");
  if (c->snap_pending) return fail(SC_ERR_STATE, "a checkpoint is already under way: sc_checkpoint_finish first");
  HIPCHK(hipSetDevice(c->device));
  // After a promised tick the storage arrays already hold the coming tick's removal and wall fix while its cell
  // indices and bucket counts live in buffers a snapshot does not take: a restore would run that wall pass a second
  // time, on fixed positions.  (Crate.run / physics_tick never leave a promise pending between calls.)
  if (c->prebinned)
    return fail(SC_ERR_STATE, "sc_checkpoint_begin after sc_set_next_inputs promised the next tick: run that tick first");
  // the side stream may exist already (halo overlap creates it): every snapshot resource is created on its own
  {
    const int rc = ensure_side_stream(c);
    if (rc) return rc;
  }
  if (!c->snap_ready) HIPCHK(hipEventCreateWithFlags(&c->snap_ready, hipEventDisableTiming));
  if (!c->snap_done) HIPCHK(hipEventCreateWithFlags(&c->snap_done, hipEventDisableTiming));
  HIPCHK(c->snap_counters_h.grow(C_COUNT, c->side_stream));
  HIPCHK(c->snap_rng_h.grow(1, c->side_stream));
  HIPCHK(c->snap_rng_d.grow(1, c->side_stream));
  const int64_t n = launch_bound(c);  // a host-side bound of the stored count; the exact count travels with the copy
  if (n > c->snap_id_h.size()) {  // (snap_id_h grows last: once it has grown, so have the others)
    const int64_t m = std::min<int64_t>(c->cap, n + n / 2 + 1024);
    for (int k = 0; k < 4; ++k) {
      HIPCHK(c->snap_d[k].grow(m, c->side_stream));
      HIPCHK(c->snap_h[k].grow(m, c->side_stream));
    }
    HIPCHK(c->snap_id_d.grow(m, c->side_stream));
    HIPCHK(c->snap_id_h.grow(m, c->side_stream));
  }
  const double* src[4] = {c->x, c->y, c->vx, c->vy};
  // on the context's stream: after the last tick, before the next one changes the storage arrays
  for (int k = 0; k < 4 && n > 0; ++k)
    HIPCHK(hipMemcpyAsync(c->snap_d[k], src[k], n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  if (n > 0) HIPCHK(hipMemcpyAsync(c->snap_id_d, c->id[0], n * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  c->snap_has_rng = c->rng != nullptr;
  if (c->rng) HIPCHK(hipMemcpyAsync(c->snap_rng_d, c->rng, sizeof(RngState), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->snap_counters_h, c->counters, C_COUNT * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipEventRecord(c->snap_ready, c->stream));
  // on the side stream: the snapshot goes to pinned host memory while the context's stream runs on
  HIPCHK(hipStreamWaitEvent(c->side_stream, c->snap_ready, 0));
  for (int k = 0; k < 4 && n > 0; ++k)
    HIPCHK(hipMemcpyAsync(c->snap_h[k], c->snap_d[k], n * sizeof(double), hipMemcpyDeviceToHost, c->side_stream));
  if (n > 0) HIPCHK(hipMemcpyAsync(c->snap_id_h, c->snap_id_d, n * sizeof(int), hipMemcpyDeviceToHost, c->side_stream));
  if (c->rng) HIPCHK(hipMemcpyAsync(c->snap_rng_h, c->snap_rng_d, sizeof(RngState), hipMemcpyDeviceToHost, c->side_stream));
  HIPCHK(hipEventRecord(c->snap_done, c->side_stream));
  c->snap_n_bound = n;
  c->snap_tick = c->tick;
  c->snap_pending = true;
  return SC_OK;
}

int sc_checkpoint_finish(sc_ctx* c, double* xy, double* vxy, int64_t* ids, int64_t room, int64_t* n_out, int64_t* tick,
                         int64_t* next_id, uint32_t* rng_key, int32_t* rng_pos) {
  if (!c || !n_out) return fail(SC_ERR_ARG, "null argument");
  if (!c->snap_pending) return fail(SC_ERR_STATE, "sc_checkpoint_begin first");
  HIPCHK(hipEventSynchronize(c->snap_ready));  // the counters' copy rode on the context's stream up to here
  HIPCHK(hipEventSynchronize(c->snap_done));
  c->snap_pending = false;
  const int64_t stored = std::min<int64_t>(c->snap_counters_h[C_NS], c->snap_n_bound);
  const std::vector<int> order = index_order(c->snap_id_h, c->snap_h[0], stored);
  const int64_t n = (int64_t)order.size();
  *n_out = n;
  if (tick) *tick = c->snap_tick;
  if (next_id) *next_id = c->snap_counters_h[C_NEXT_ID];
  const RngState& rs = *c->snap_rng_h;
  if (rng_pos) *rng_pos = c->snap_has_rng ? rs.pos : -1;
  if (rng_key && c->snap_has_rng) std::memcpy(rng_key, rs.mt, sizeof rs.mt);
  if (n > room) return fail(SC_ERR_CAPACITY, "host arrays hold %lld, the checkpoint has %lld particles", (long long)room, (long long)n);
  write_pairs(xy, order, c->snap_h[0], c->snap_h[1]);
  write_pairs(vxy, order, c->snap_h[2], c->snap_h[3]);
  for (int64_t k = 0; k < n && ids; ++k) ids[k] = c->snap_id_h[order[k]];
  return SC_OK;
}

int sc_restore_counters(sc_ctx* c, int64_t tick, int64_t next_id) {
  if (!c || tick < 0 || next_id < 0 || next_id > std::numeric_limits<int>::max()) return fail(SC_ERR_ARG, "bad tick / next id");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_restore_counters inside a tick");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->prebinned) {
    const int rc = abandon_promise(c);
    if (rc) return rc;
  }
  c->tick = tick;
  c->halo_ring_from = tick;
  c->live_hint_from = tick;
  c->progress[kProgressTicks] = (int)tick;  // nothing of the new numbering is queued
  c->next_id = std::max<int64_t>(c->next_id, next_id);
  const int nid = (int)c->next_id;
  HIPCHK(hipMemcpyAsync(c->counters + C_NEXT_ID, &nid, sizeof nid, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return SC_OK;
}

// ---- NumPy's global MT19937 stream on the device (sc_rng.h) -------------------------------------

int sc_rng_set_state(sc_ctx* c, const uint32_t* key, int32_t pos) {
  if (!c || !key || pos < 0 || pos > kMtN) return fail(SC_ERR_ARG, "an MT19937 state is 624 words and a position in [0, 624]");
  if (c->in_step) return fail(SC_ERR_STATE, "the generator cannot change inside a tick");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(c->rng.grow(1, c->stream));
  RngState h;
  std::memcpy(h.mt, key, sizeof h.mt);
  h.pos = pos;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(c->rng, &h, sizeof h, hipMemcpyHostToDevice));
  return SC_OK;
}

int sc_rng_get_state(sc_ctx* c, uint32_t* key, int32_t* pos) {
  if (!c || !key || !pos) return fail(SC_ERR_ARG, "null argument");
  if (!c->rng) return fail(SC_ERR_STATE, "sc_rng_set_state has not been called");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_rng_get_state inside a tick");
  RngState h;
  HIPCHK(hipMemcpyAsync(&h, c->rng, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::memcpy(key, h.mt, sizeof h.mt);
  *pos = h.pos;
  return SC_OK;
}

int sc_emit_particles(sc_ctx* c, const sc_source* sources, int32_t n_sources, double dt, int64_t max_particles) {
  if (!c || n_sources < 0 || (n_sources > 0 && !sources)) return fail(SC_ERR_ARG, "bad sources");
  if (!c->rng) return fail(SC_ERR_STATE, "sc_rng_set_state has not been called");
  if (c->in_step) return fail(SC_ERR_STATE, "particles cannot change between sc_step_begin and sc_step_finish");
  if (c->prebinned) return fail(SC_ERR_STATE, "particles cannot be emitted after sc_set_next_inputs promised the next tick");
  if (n_sources == 0) return SC_OK;
  c->pairs_valid = false;
  // the sources go to the device in groups of kMaxSources, one k_rng_emit launch per group in source order on the
  // stream: each launch continues the stream and reads the stored count the previous one left, as one launch would
  std::vector<SourcesK> groups((n_sources + kMaxSources - 1) / kMaxSources);
  std::memset(groups.data(), 0, groups.size() * sizeof(SourcesK));
  int64_t most = 0;  // (over ALL sources: the bounds below are per call)
  for (int i = 0; i < n_sources; ++i) {
    const sc_source& s = sources[i];
    const double p = dt;
    // the legacy binomial for p <= 0.5: inversion up to n p = 30 (both YAML scenes: n p = 4 and 14), BTPE beyond;
    // p > 0.5 (a time step above one half) is not on the device
    if (!(p > 0.0 && p <= 0.5) || s.flow < 1)
      return fail(SC_ERR_DOMAIN, "binomial(%lld, %g): the device draws NumPy's legacy binomial for 0 < p <= 0.5 only",
                  (long long)s.flow, p);
    SourcesK& g = groups[i / kMaxSources];
    SourceK& d = g.src[g.n++];
    d.radius = s.radius; d.px = s.position_x; d.py = s.position_y; d.vx = s.velocity_x; d.vy = s.velocity_y;
    d.noise = s.noise; d.flow = s.flow; d.p = p;
    d.q = 1.0 - p;
    d.qn = std::exp((double)s.flow * std::log(d.q));
    const double np_ = (double)s.flow * p;
    d.bound = (long long)std::min((double)s.flow, np_ + 10.0 * std::sqrt(np_ * d.q + 1));
    d.btpe = np_ > 30.0 ? 1 : 0;
    if (d.btpe) {  // randomkit's rk_binomial_btpe set-up, in its operation order (r = p, q = 1 - p here)
      const double n = (double)s.flow, r = p, q = d.q, fm = n * r + r;
      d.m = (long long)std::floor(fm);
      d.p1 = std::floor(2.195 * std::sqrt(n * r * q) - 4.6 * q) + 0.5;
      d.xm = (double)d.m + 0.5;
      d.xl = d.xm - d.p1;
      d.xr = d.xm + d.p1;
      d.c = 0.134 + 20.5 / (15.3 + (double)d.m);
      double a = (fm - d.xl) / (fm - d.xl * r);
      d.laml = a * (1.0 + a / 2.0);
      a = (d.xr - fm) / (d.xr * q);
      d.lamr = a * (1.0 + a / 2.0);
      d.p2 = d.p1 * (1.0 + 2.0 * d.c);
      d.p3 = d.p2 + d.c / d.laml;
      d.p4 = d.p3 + d.c / d.lamr;
      d.nrq = n * r * q;
    }
    most += d.bound;
  }
  // host-side bounds of the stored count and of the ids: at most `bound` particles per source; the live count a
  // recent tick published (progress block) keeps the bound from drifting away without any synchronisation
  // (the device writes the tick number last: the three words belong together when it reads the same before and after)
  int64_t done = progress_read(c, kProgressTicks);
  const int64_t live = progress_read(c, kProgressLive), published_ids = progress_read(c, kProgressNextId);
  std::atomic_thread_fence(std::memory_order_acquire);
  if (progress_read(c, kProgressTicks) != done) done = -1;  // a tick finished in between: no hint this time
  int64_t upper = c->upper + most;
  if (done > c->live_hint_from && c->tick >= done && c->tick - done <= 8)
    upper = std::min(upper, live + (c->tick - done + 1) * most);
  upper = std::min<int64_t>(upper, std::max<int64_t>(max_particles, c->upper));
  if (upper > c->cap) {
    int h[C_COUNT];
    int rc = read_counters(c, h);  // rare: the bound reached the capacity, look at the real count
    if (rc) return rc;
    upper = std::min<int64_t>(h[C_NS] + most, std::max<int64_t>(max_particles, h[C_NS]));
    if (upper > c->cap) return fail(SC_ERR_CAPACITY, "%lld particles may exceed the context capacity %lld", (long long)upper, (long long)c->cap);
  }
  // The host's id counter is a bound too (the device hands out the real ids): every call adds the binomial's restart
  // bound, several times the particles actually emitted, and the id tables of SC_NOISE_HOST are sized and scanned by
  // it every tick.  The count the device published with a recent tick pulls it back, like `upper` above.
  c->emit_most = std::max(c->emit_most, most);
  if (done > c->live_hint_from && c->tick >= done && c->tick - done <= 8) {
    if (published_ids > 0) c->next_id = std::min(c->next_id, published_ids + (c->tick - done + 1) * c->emit_most);
  }
  if (c->next_id + most > std::numeric_limits<int>::max()) return fail(SC_ERR_CAPACITY, "particle ids exhausted");
  HIPCHK(hipSetDevice(c->device));
  for (const SourcesK& g : groups) {
    Bracket br(c, K_APPEND);
    hipLaunchKernelGGL(k_rng_emit, dim3(1), dim3(64), 0, c->stream, g, (long long)max_particles, c->rng, c->counters, c->x,
                       c->y, c->vx, c->vy, c->id[0], (int)c->cap);
  }
  HIPCHK(hipGetLastError());
  c->upper = upper;
  c->next_id += most;  // an upper bound from here on: the device counts the ids it hands out (C_NEXT_ID)
  return SC_OK;
}

#ifdef SC_STAMPS
// diagnostic build: copies the stamp buffer (kStampKernels x 65536 waves x kStampSlots slots, int64) to the host
int sc_debug_stamps(sc_ctx* c, long long* out) {
  if (!c || !out) return fail(SC_ERR_ARG, "null argument");
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(sc::g_stamps), sizeof(long long) * sc::kStampKernels * sc::kStampWaves * sc::kStampSlots));
  return SC_OK;
}
#endif

#ifdef SC_TIMELINE
// diagnostic build: [kTlKernels][65536][4] = (start, end) on the 100 MHz clock, HW_ID, XCC_ID of every wave of the last pass A / pass B
int sc_debug_timeline(sc_ctx* c, long long* out) {
  if (!c || !out) return fail(SC_ERR_ARG, "null argument");
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(sc::g_timeline), sizeof(long long) * sc::kTlKernels * sc::kTlWaves * 4));
  return SC_OK;
}
#endif

// ---- timing -----------------------------------------------------------------------------------

static int harvest(sc_ctx* c) {
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto& e : c->ev_used) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      c->ms[e.k] += ms;
      c->launches[e.k] += 1;
    }
    c->ev_free.push_back(e);
  }
  c->ev_used.clear();
  return SC_OK;
}

int sc_enable_timing(sc_ctx* c, int on) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!on && c->timing) harvest(c);
  c->timing = on != 0;
  return SC_OK;
}

int sc_reset_timing(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  int rc = harvest(c);
  for (int k = 0; k < SC_NUM_KERNELS; ++k) {
    c->ms[k] = 0;
    c->launches[k] = 0;
  }
  return rc;
}

int sc_get_timing(sc_ctx* c, double* ms, int64_t* launches) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  int rc = harvest(c);
  for (int k = 0; k < SC_NUM_KERNELS; ++k) {
    if (ms) ms[k] = c->ms[k];
    if (launches) launches[k] = c->launches[k];
  }
  return rc;
}

}  // extern "C"
