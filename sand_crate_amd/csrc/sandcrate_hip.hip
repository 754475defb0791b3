// libsandcrate_hip.so -- host side of the C ABI declared in include/sandcrate_hip.h.
// Owns the device memory (float64 SoA particle arrays, cell buckets, neighbor table), builds the
// per-tick kernel argument block and enqueues the kernels of sc_kernels.h on one HIP stream.
// gfx950 (MI355X) only; there is no CPU path in this library.
// The single translation unit: the kernel headers, sc_host.h (what all host code shares: buffers, the context, every
// add-on's state), the tick below, and at the end one sc_host_*.h per family of add-ons.
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
#include "sc_cluster_sums.h"
#include "sc_nearest.h"
#include "sc_fields.h"
#include "sc_fields_grad.h"
#include "sc_hist.h"
#include "sc_rays.h"
#include "sc_track.h"
#include "sc_traj.h"
#include "sc_rccl.h"
#include "sc_render.h"
#include "sc_rng.h"
#include "sc_tiled.h"
#include "sc_host.h"

namespace {

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
      long long& lo = c->link.slab_axis ? rrmin : ccmin;
      long long& hi = c->link.slab_axis ? rrmax : ccmax;
      lo = std::max(cmin, c->link.own_lo - c->link.halo - 1);
      hi = std::min(cmax, c->link.own_hi + c->link.halo);
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
  w.slab_axis = c->slab ? c->link.slab_axis : 0;
  w.band_margin = w.slab_axis ? kBandMarginRows : kBandMarginColumns;
  w.own_lo = c->slab ? c->link.own_lo : std::numeric_limits<long long>::min();
  w.own_hi = c->slab ? c->link.own_hi : std::numeric_limits<long long>::max();
  w.halo = c->link.halo;
  {  // where the particles are expected to end: for slabs a recent tick's live count (blocks beyond it are placed one by one)
    const int64_t done = progress_read(c, kProgressTicks), published = progress_read(c, kProgressLive);
    const int64_t bound = launch_bound(c);
    w.live_hint = (int)(c->slab && published > 0 && done > c->live_hint_from
                            ? std::min<int64_t>(bound, (int64_t)published + 2048)
                            : bound);
  }
  w.has_left = c->link.has_left;
  w.has_right = c->link.has_right;
  return SC_OK;
}

int make_world(sc_ctx* c) {
  if (!c->custom_grid && !c->have_params) return fail(SC_ERR_STATE, "sc_set_params has not been called");
  if (const int rc = build_world(c, c->w, c->now, c->tick)) return rc;
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


int read_counters(sc_ctx* c, int* out) { return read_back(c, out, c->counters, C_COUNT * sizeof(int)); }

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
    if (const int rc = abandon_promise(c)) return rc;
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
  if (c->prebinned && reset)
    if (const int rc = abandon_promise(c)) return rc;
  if (!reset && c->ids_bounded) {
    // the device has handed out ids since the host last knew the counter: what the host holds is a bound, and ids taken
    // from it would leave a gap that a host that emitted everything itself does not have.  Ask the device -- one
    // synchronisation, on the rare path of a host append behind a device emission (a crate whose dt passed one half)
    int h[C_COUNT];
    if (const int rc = read_counters(c, h)) return rc;
    c->next_id = h[C_NEXT_ID];
  }
  c->ids_bounded = false;
  const int64_t base = reset ? 0 : c->upper;
  c->pairs.valid = false;
  if (reset) {
    c->next_id = 0;
    c->normals_valid = 0;
    c->link.halo_ring_from = c->tick;  // counts published before this belong to another state
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
  if (part && c->link.slab_axis == 1) {
    const int64_t rows = std::max<int64_t>(1, std::min<int64_t>(c->link.own_hi, c->w.row0 + c->w.nrows) - std::max<int64_t>(c->link.own_lo, c->w.row0));
    const int64_t band_rows = 2 * c->link.halo + kBandMarginRows + 2;
    bandw = (int)std::min<int64_t>(tile_grid(c), 2 * band_rows * (c->w.live_hint / rows + 1) / kTileW + 16);
  }
  const int grid = part == 1 && bandw ? 2 * bandw : part == 3 ? tile_grid(c) + 2 * bandw : tile_grid(c);
  hipStream_t stream = c->stream;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kTileW), 0, stream, c->w, c->counters, c->sxy, c->svv,
                       c->id[1], c->wslotT, c->cellT, c->nbr, c->rows, (int)c->cap, c->eta, c->offById, c->P,
                       c->snn, c->wrec[cur], c->x, c->y, c->vx, c->vy, c->id[0], c->tileBoundsT,
                       c->progress_dev, wn, c->cellS, c->wslotS, c->cellCount, c->wrec[nxt], c->link.haloL, c->link.haloR, c->link.haloCap,
                       c->monitor, c->tileBand, part, bandw, c->link.band_epoch);
  };
  Bracket br(c, K_FORCE);
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
}

template <int NOISE>
void launch_pass_b_any(sc_ctx* c, bool fused, const WallInputs& wn) {
  if (c->monitor_on) {
    launch_pass_b<NOISE, false, true>(c, wn);
  } else if (fused && c->slab && c->link.overlap && c->link.haloL && (c->link.has_left || c->link.has_right)) {
    // halo overlap: the blocks that may pack halo records first; once they are done (ev_band) the exchange of the
    // coming tick may start on the side stream while the interior blocks run
    if (c->link.slab_axis == 1 && c->link.band_by_flag) {
      // slabs of rows: one launch, the window blocks first; the side stream polls for their completion (k_wait_band)
      c->link.band_epoch += 1;
      launch_pass_b<NOISE, true>(c, wn, 3);
      c->link.band_flagged = true;
    } else {
      launch_pass_b<NOISE, true>(c, wn, 1);
      (void)hipEventRecord(c->link.ev_band, c->stream);
      launch_pass_b<NOISE, true>(c, wn, 2);
      c->link.band_flagged = false;
    }
    c->link.band_pending = true;
  } else if (fused)
    launch_pass_b<NOISE, true>(c, wn);
  else
    launch_pass_b<NOISE, false>(c, wn);
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
  // room for m elements in each of `bufs`, in this order, as long as nothing has failed
  auto grow = [&](int64_t m, auto&... bufs) { ((e = e == hipSuccess ? bufs.grow(m, c->stream) : e), ...); };
  grow(n, c->x, c->y, c->vx, c->vy, c->id[0], c->id[1], c->cellS, c->wslotS, c->cellT, c->wslotT, c->keys, c->keyCell);
  grow(6 * (n / kTileW + 2), c->tileBounds, c->tileBoundsT);
  grow(n / kTileW + 2, c->tileBand);
  if (e == hipSuccess) e = hipMemsetAsync(c->tileBand, 0, c->tileBand.bytes(), c->stream);
  grow(kMaxSortTasks, c->sortTasks);
  grow(kProgressInts, c->progress);
  if (e == hipSuccess) {
    std::fill_n(c->progress.get(), kProgressInts, 0);
    e = hipHostGetDevicePointer((void**)&c->progress_dev, c->progress, 0);
  }
  grow(5 * n, c->wrec[0], c->wrec[1]);
  grow(kMaxNbr * n, c->nbr);
  grow(n, c->rows, c->P, c->snn, c->sxy, c->svv);
  grow(C_ALLOC, c->counters);
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
  if (c->link.comm) (void)sc_comm_destroy(c);
  if (c->link.ev_band) (void)hipEventDestroy(c->link.ev_band);
  if (c->link.ev_xchg) (void)hipEventDestroy(c->link.ev_xchg);
  for (auto& v : {c->ev_used, c->ev_free})
    for (auto& e : v) {
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
  if (c->snap.ready) (void)hipEventDestroy(c->snap.ready);
  if (c->snap.done) (void)hipEventDestroy(c->snap.done);
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
  if (const int rc = read_counters(c, h)) return rc;
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
  if (const int rc = read_counters(c, h)) return rc;
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
  if (!c->custom_grid)
    if (const int rc = wait_ticks_finished(c, c->tick - kMaxTicksQueued, "queued ticks")) return rc;
  int rc = make_world(c);
  if (rc) return rc;
  c->pairs.valid = false;
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
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, c->stream, c->counters, c->cellS, c->x, c->id[0],
                         Buckets{c->cellStart}, c->cellCount, c->keys, c->keyCell, cap, w.live_hint);
    };
    piles_expected(c) ? launch(k_scatter<true>) : launch(k_scatter<false>);
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
  if (const int rc = read_counters(c, h)) return rc;
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
    if (const int rc = launch_noise_offsets(c)) return rc;
  }
  if (2 * n_pairs > c->eta.size()) HIPCHK(c->eta.grow(2 * (n_pairs + n_pairs / 2 + 1024), c->stream));
  if (n_pairs > 0)
    HIPCHK(hipMemcpyAsync(c->eta, u01, 2 * n_pairs * sizeof(double), hipMemcpyHostToDevice, c->stream));
  c->etaPairs = n_pairs;
  return SC_OK;
}

// what a finished tick appends to the logs that are on (sc_host_logs.h)
static int probe_launch(sc_ctx* c, bool to_log);
static int track_launch(sc_ctx* c, bool to_log);
static int traj_launch(sc_ctx* c, bool on_demand);

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
  const bool slab_ready = !c->slab || c->link.haloL || !(c->link.has_left || c->link.has_right);
  // (the monitor runs with the plain kernel; the probe's log, the track log and the trajectory log record the state
  // sc_download_state stands for, which a fused tick does not leave in the storage arrays)
  const bool fused =
      c->have_next && slab_ready && !c->custom_grid && !c->monitor_on && !c->probe.on && !c->track.on && !c->traj.on;
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
  if (c->probe.on && !c->slab && !c->custom_grid)
    if (const int rc = probe_launch(c, true)) return rc;
  if (c->track.on && !c->slab && !c->custom_grid && c->tick % c->track.every == 0)
    if (const int rc = track_launch(c, true)) return rc;
  if (c->traj.on && !c->slab && !c->custom_grid && c->tick % c->traj.every == 0) return traj_launch(c, false);
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
  if (const int rc = load_walls(c->next, segments, nullptr, false, ns, bodies, nb)) return rc;
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

int sc_download_pressure(sc_ctx* c, double* pressure, int64_t room, int64_t* n_out) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step || !c->normals_valid) return fail(SC_ERR_STATE, "sc_download_pressure needs a finished tick");
  int h[C_COUNT];
  int rc = read_counters(c, h);
  if (rc) return rc;
  int64_t n = h[C_NT];
  if (n_out) *n_out = n;
  if (n > room) return fail(SC_ERR_CAPACITY, "host arrays too small");
  std::vector<double> hp(n);
  std::vector<int> id(n);
  if ((rc = fetch(c, hp.data(), c->P, n * sizeof(double))) || (rc = fetch(c, id.data(), c->id[1], n * sizeof(int))))
    return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  const std::vector<int> order = index_order(id.data(), nullptr, n);
  for (size_t k = 0; k < order.size() && pressure; ++k) pressure[k] = hp[order[k]];
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
  if (const int rc = read_back(c, &h, c->rng, sizeof h)) return rc;
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
  c->pairs.valid = false;
  // the sources go to the device in groups of kMaxSources, one k_rng_emit launch per group in source order on the
  // stream: each launch continues the stream and reads the stored count the previous one left, as one launch would
  std::vector<SourcesK> groups((n_sources + kMaxSources - 1) / kMaxSources);
  std::memset(groups.data(), 0, groups.size() * sizeof(SourcesK));
  int64_t most = 0;  // (over ALL sources: the bounds below are per call)
  for (int i = 0; i < n_sources; ++i) {
    const sc_source& s = sources[i];
    const double p = dt;
    // the legacy binomial for p <= 0.5: inversion up to n p = 30 (both YAML scenes: n p = 4 and 14), BTPE beyond;
    // p > 0.5 (a time step above one half) is not on the device.  flow = 0 (a flow slider at its stop) is: NumPy spends
    // one double on binomial(0, p) and returns 0, and so does the inversion loop -- qn = exp(0) = 1, bound = 0, no U
    // exceeds it.  Only a negative flow, which NumPy refuses, is refused here
    if (!(p > 0.0 && p <= 0.5) || s.flow < 0)
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
  c->ids_bounded = true;
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

// ---- the add-ons: each family's host code in a file of its own (sc_host.h says what they may use of the above) ----
#include "sc_host_frames.h"
#include "sc_host_logs.h"
#include "sc_host_state.h"
#include "sc_host_slab.h"
#include "sc_host_snapshot.h"
