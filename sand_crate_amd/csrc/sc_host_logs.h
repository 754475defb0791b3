// Host side of what a run records about itself: the probe, tracking, trajectories and the force monitor.
#pragma once
#include "sc_host.h"
#include "sc_probe.h"
#include "sc_track.h"
#include "sc_traj.h"

extern "C" {

// ---- the probe (sc_probe.h) ---------------------------------------------------------------------

static int probe_check_bins(int32_t n_bins, double x0, double x1) {
  if (n_bins < 0 || n_bins > kProbeMaxBins) return fail(SC_ERR_ARG, "%d bins; 0..%d", n_bins, kProbeMaxBins);
  if (n_bins > 0 && !(std::isfinite(x0) && std::isfinite(x1) && x1 > x0))
    return fail(SC_ERR_ARG, "the profile's range must be finite with x1 > x0");
  return SC_OK;
}

// What every call of the probe starts with once its arguments are checked; `switching`: the log is turned on or off.
static int probe_refuse(const sc_ctx* c, bool switching) {
  if (c->slab) return fail(SC_ERR_STATE, "the probe is not available in slab mode");
  if (switching && c->in_step) return fail(SC_ERR_STATE, "the probe's log cannot change inside a tick");
  if (switching && c->prebinned)
    return fail(SC_ERR_STATE, "the probe's log cannot change after sc_set_next_inputs promised the next tick");
  return SC_OK;
}

// Empties n bins: no members, and the top of none (all ones).
static int probe_clear(sc_ctx* c, int* counts, unsigned long long* tops, size_t n) {
  HIPCHK(hipMemsetAsync(counts, 0, n * sizeof(int), c->stream));
  HIPCHK(hipMemsetAsync(tops, 0xFF, n * sizeof(unsigned long long), c->stream));
  return SC_OK;
}

// Enqueues one measurement: into the log's next row (`to_log`; the device decides which, or that the log is full), or
// into the row and profile of sc_probe_now with the bins given.
static int probe_launch(sc_ctx* c, bool to_log, int n_bins, double x0, double x1) {
  ProbeArgs a{};
  a.nbins = n_bins;
  a.x0 = x0;
  a.w = n_bins > 0 ? (x1 - x0) / n_bins : 1.0;
  a.tick = (double)c->tick;
  a.pressure_valid = c->normals_valid ? 1 : 0;
  a.cap = (int)c->cap;
  a.log_rows = to_log ? c->probe.cap : -1;
  hipLaunchKernelGGL(k_probe, dim3(kProbeBlocks), dim3(kProbeBlock), 0, c->stream, a, c->counters, c->x, c->y, c->vx, c->vy,
                     c->P, c->probe.partials, c->probe.words, to_log ? c->probe.rows : c->probe.nowRow,
                     to_log ? c->probe.counts : c->probe.nowCounts, to_log ? c->probe.tops : c->probe.nowTops);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

static int probe_launch(sc_ctx* c, bool to_log) { return probe_launch(c, to_log, c->probe.bins, c->probe.x0, c->probe.x1); }

// the bins' tops as the kernel keeps them (probe_key; all ones: an empty bin) back to float64
static void probe_decode_tops(const unsigned long long* keys, double* tops, int64_t n) {
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

// Enqueues one frame of the state as it stands, with the walls the last tick ran with: appended to the log (`to_log`;
// the device decides where, or that it does not fit), or at the start of track.now, which holds `track.now.size()` bytes.
static int track_launch(sc_ctx* c, bool to_log) {
  TrackArgs a{};
  a.tick = c->tick;
  a.log_bytes = to_log ? c->track.cap : -1;
  a.room = c->track.now.size();
  a.scale = kTrackCodes / kTrackSpan;
  a.pressure_valid = c->normals_valid ? 1 : 0;
  a.cap = (int)c->cap;
  a.nseg = c->now.nseg;
  std::memcpy(a.seg, c->now.seg, sizeof a.seg);
  unsigned char* base = to_log ? c->track.log.get() : c->track.now.get();
  hipLaunchKernelGGL(k_track_reserve, dim3(1), dim3(64), 0, c->stream, a, c->counters, c->track.words, base);
  const int64_t bound = slot_bound(c);
  const int64_t groups = track_pad8(bound) / kTrackPerThread;
  if (groups > 0)
    hipLaunchKernelGGL(k_track_pack, dim3(grid_for(groups)), dim3(kBlock), 0, c->stream, a, c->counters, c->track.words, c->x,
                       c->y, c->id[0], c->P, base);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

static int track_refuse(const sc_ctx* c, bool switching) {
  if (c->slab) return fail(SC_ERR_STATE, "tracking is not available in slab mode");
  if (c->in_step) return fail(SC_ERR_STATE, switching ? "the track log cannot change inside a tick" : "tracking happens between ticks");
  if (switching && c->prebinned)
    return fail(SC_ERR_STATE, "the track log cannot change after sc_set_next_inputs promised the next tick");
  return SC_OK;
}

// ---- trajectories (sc_traj.h) -------------------------------------------------------------------

// Enqueues one frame of the state as it stands into the log's next place: the device decides which, or that the log is
// full.  `on_demand`: sc_traj_capture, between ticks.
static int traj_launch(sc_ctx* c, bool on_demand) {
  TrajArgs a{};
  a.tick = c->tick;
  a.frames = c->traj.frames;
  a.id0 = c->traj.id0;
  a.rows = c->traj.rows;
  a.on_demand = on_demand ? 1 : 0;
  a.pressure_valid = c->normals_valid ? 1 : 0;
  a.cap = (int)c->cap;
  hipLaunchKernelGGL(k_traj_reserve, dim3(1), dim3(64), 0, c->stream, a, c->counters, c->traj.log);
  hipLaunchKernelGGL(k_traj_clear, dim3(grid_for(a.rows)), dim3(kBlock), 0, c->stream, a, c->traj.log);
  const int64_t bound = slot_bound(c);
  if (bound > 0)
    hipLaunchKernelGGL(k_traj_scatter, dim3(grid_for(bound)), dim3(kBlock), 0, c->stream, a, c->counters, c->traj.log, c->x,
                       c->y, c->vx, c->vy, c->id[0], c->P);
  HIPCHK(hipGetLastError());
  return SC_OK;
}

static int traj_refuse(const sc_ctx* c, bool switching) {
  if (c->slab) return fail(SC_ERR_STATE, "trajectories are not available in slab mode");
  if (c->in_step)
    return fail(SC_ERR_STATE, switching ? "the trajectory log cannot change inside a tick" : "a frame is captured between ticks");
  if (switching && c->prebinned)
    return fail(SC_ERR_STATE, "the trajectory log cannot change after sc_set_next_inputs promised the next tick");
  return SC_OK;
}

int sc_traj_enable_device(sc_ctx* c, double* dev_states, double* dev_pressure, int64_t* dev_ticks, int64_t* dev_counts,
                          int64_t* dev_outside, int64_t* dev_words, int64_t frames, int64_t id0, int64_t rows, int64_t every,
                          int32_t reset) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!dev_states || !dev_ticks || !dev_counts || !dev_outside || !dev_words) return fail(SC_ERR_ARG, "null argument");
  if ((uintptr_t)dev_states % 16) return fail(SC_ERR_ARG, "the states must be aligned to 16 bytes");
  if (frames < 1) return fail(SC_ERR_ARG, "a log of %lld frames; at least 1", (long long)frames);
  if (rows < 1 || id0 < 0 || id0 > (int64_t)std::numeric_limits<int>::max() - rows)
    return fail(SC_ERR_ARG, "a window of %lld ids from %lld; at least one, within 0..2^31 - 2", (long long)rows, (long long)id0);
  if (every < 1) return fail(SC_ERR_ARG, "every %lld; at least 1", (long long)every);
  if (const int rc = traj_refuse(c, true)) return rc;
  HIPCHK(hipSetDevice(c->device));
  if (reset) HIPCHK(hipMemsetAsync(dev_words, 0, JW_COUNT * sizeof(int64_t), c->stream));  // (a failure leaves what was)
  c->traj.log = TrajLog{dev_states, dev_pressure, (long long*)dev_ticks, (long long*)dev_counts, (long long*)dev_outside,
                        (long long*)dev_words};
  c->traj.frames = frames;
  c->traj.id0 = id0;
  c->traj.rows = rows;
  c->traj.every = every;
  c->traj.on = true;
  return SC_OK;
}

int sc_traj_capture(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (const int rc = traj_refuse(c, false)) return rc;
  if (!c->traj.on) return fail(SC_ERR_STATE, "sc_traj_enable_device first");
  HIPCHK(hipSetDevice(c->device));
  return traj_launch(c, true);
}

int sc_traj_disable(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (const int rc = traj_refuse(c, true)) return rc;
  c->traj.on = false;
  c->traj.log = TrajLog{};
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
  if ((rc = c->track.ensure(c->stream))) return rc;
  HIPCHK(c->track.now.grow(track_planes(slot_bound(c), c->now.nseg).end, c->stream));
  if ((rc = track_launch(c, false))) return rc;
  unsigned long long words[TW_COUNT];
  if ((rc = read_back(c, words, c->track.words, sizeof words))) return rc;
  const int64_t bytes = track_planes((int64_t)words[TW_N], c->now.nseg).end;
  if ((long long)words[TW_AT] < 0)
    return fail(SC_ERR_HIP, "the device stores %lld particles, more than the host's bound", (long long)words[TW_N]);
  if ((rc = refuse_room(bytes, room, n_bytes, "a frame of %lld bytes, room for %lld"))) return rc;
  return read_back(c, out, c->track.now, (size_t)bytes);
}

int sc_track_enable(sc_ctx* c, int64_t every, int64_t capacity_bytes) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (every < 1) return fail(SC_ERR_ARG, "every %lld; at least 1", (long long)every);
  if (capacity_bytes < 1 || capacity_bytes > ((int64_t)1 << 40))
    return fail(SC_ERR_ARG, "a log of %lld bytes; 1..2^40", (long long)capacity_bytes);
  int rc = track_refuse(c, true);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  if ((rc = c->track.ensure(c->stream))) return rc;
  c->track.on = false;  // (a call that fails below leaves no log)
  HIPCHK(c->track.log.grow(track_pad8(capacity_bytes), c->stream));
  HIPCHK(hipMemsetAsync(c->track.words, 0, c->track.words.bytes(), c->stream));
  c->track.every = every;
  c->track.cap = capacity_bytes;
  c->track.on = true;
  return SC_OK;
}

int sc_track_disable(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (const int rc = track_refuse(c, true)) return rc;
  c->track.on = false;
  return SC_OK;
}

int sc_track_read(sc_ctx* c, uint8_t* out, int64_t room, int64_t* n_bytes, int64_t* n_frames, int64_t* dropped) {
  if (!c || !n_bytes || !n_frames || !dropped || room < 0 || (room > 0 && !out))
    return fail(SC_ERR_ARG, "null argument or negative room");
  *n_bytes = *n_frames = *dropped = 0;
  int rc = track_refuse(c, false);
  if (rc) return rc;
  if (!c->track.on) return fail(SC_ERR_STATE, "sc_track_enable first");
  unsigned long long words[TW_COUNT];
  if ((rc = read_back(c, words, c->track.words, sizeof words))) return rc;
  const int64_t bytes = std::min<int64_t>((int64_t)words[TW_CURSOR], c->track.cap);
  // (a log larger than the room: nothing is delivered and nothing forgotten)
  if ((rc = refuse_room(bytes, room, n_bytes, "%lld bytes logged, room for %lld"))) return rc;
  if (bytes > 0 && (rc = read_back(c, out, c->track.log, (size_t)bytes))) return rc;
  *n_frames = (int64_t)words[TW_FRAMES];
  *dropped = (int64_t)words[TW_DROPPED];
  HIPCHK(hipMemsetAsync(c->track.words, 0, c->track.words.bytes(), c->stream));  // the log starts over
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
  if (c->prebinned)
    if (const int rc = abandon_promise(c)) return rc;
  c->pairs.valid = false;
  HIPCHK(c->track.load.grow(n_bytes, c->stream));
  HIPCHK(hipMemcpyAsync(c->track.load, frame, (size_t)n_bytes, hipMemcpyHostToDevice, c->stream));
  TrackLoad a{};
  a.n = (int)n;
  a.nseg = nseg;
  a.plain = plain ? 1 : 0;
  a.next_id = (int)(max_id + 1);
  a.lo = lo;
  a.step = span / kTrackCodes;
  hipLaunchKernelGGL(k_track_unpack, dim3(grid_for(n)), dim3(kBlock), 0, c->stream, a, c->track.load, c->counters, c->x, c->y,
                     c->vx, c->vy, c->id[0], c->P);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));  // `frame` is the caller's: read before we return
  c->upper = n;
  c->next_id = max_id + 1;
  c->normals_valid = 1;  // every slot carries the pressure its colour stands for
  c->link.halo_ring_from = c->tick;
  c->live_hint_from = c->tick;
  return SC_OK;
}

// ---- the probe ----------------------------------------------------------------------------------

int sc_probe_now(sc_ctx* c, int32_t n_bins, double x0, double x1, double* row16, int32_t* counts, double* tops) {
  if (!c || !row16) return fail(SC_ERR_ARG, "null argument");
  int rc = probe_check_bins(n_bins, x0, x1);
  if (rc) return rc;
  if (n_bins > 0 && (!counts || !tops)) return fail(SC_ERR_ARG, "null profile arrays");
  if ((rc = probe_refuse(c, false))) return rc;
  if (c->in_step) return fail(SC_ERR_STATE, "measuring happens between ticks");
  HIPCHK(hipSetDevice(c->device));
  if ((rc = c->probe.ensure(c->stream))) return rc;
  std::vector<unsigned long long> keys((size_t)n_bins);
  if (n_bins > 0 && (rc = probe_clear(c, c->probe.nowCounts, c->probe.nowTops, (size_t)n_bins))) return rc;
  if ((rc = probe_launch(c, false, n_bins, x0, x1))) return rc;
  HIPCHK(hipMemcpyAsync(row16, c->probe.nowRow, kProbeFields * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (n_bins > 0) {
    HIPCHK(hipMemcpyAsync(counts, c->probe.nowCounts, (size_t)n_bins * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(keys.data(), c->probe.nowTops, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
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
  if ((rc = probe_refuse(c, true))) return rc;
  HIPCHK(hipSetDevice(c->device));
  if ((rc = c->probe.ensure(c->stream))) return rc;
  c->probe.on = false;  // (a call that fails below leaves no log)
  HIPCHK(c->probe.rows.grow(capacity_rows * kProbeFields, c->stream));
  HIPCHK(c->probe.counts.grow(capacity_rows * n_bins, c->stream));
  HIPCHK(c->probe.tops.grow(capacity_rows * n_bins, c->stream));
  if (n_bins > 0 && (rc = probe_clear(c, c->probe.counts, c->probe.tops, (size_t)capacity_rows * n_bins))) return rc;
  HIPCHK(hipMemsetAsync(c->probe.words, 0, c->probe.words.bytes(), c->stream));
  c->probe.cap = capacity_rows;
  c->probe.tail = 0;
  c->probe.bins = n_bins;
  c->probe.x0 = x0;
  c->probe.x1 = x1;
  c->probe.on = true;
  return SC_OK;
}

int sc_probe_disable(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (const int rc = probe_refuse(c, true)) return rc;
  c->probe.on = false;
  return SC_OK;
}

int sc_probe_read(sc_ctx* c, double* rows, int32_t* counts, double* tops, int64_t room, int64_t* n_out, int64_t* n_dropped) {
  if (!c || !n_out || !n_dropped) return fail(SC_ERR_ARG, "null argument");
  if (room < 0) return fail(SC_ERR_ARG, "room for %lld rows", (long long)room);
  if (room > 0 && (!rows || (c->probe.on && c->probe.bins > 0 && (!counts || !tops)))) return fail(SC_ERR_ARG, "null arrays");
  int rc = probe_refuse(c, false);
  if (rc) return rc;
  if (c->in_step) return fail(SC_ERR_STATE, "the log is read between ticks");
  if (!c->probe.on) return fail(SC_ERR_STATE, "sc_probe_enable first");
  HIPCHK(hipSetDevice(c->device));
  int words[PW_COUNT];
  if ((rc = read_back(c, words, c->probe.words, sizeof words))) return rc;
  const int64_t head = std::min<int64_t>(words[PW_HEAD], c->probe.cap), tail = std::min(c->probe.tail, head);
  const int64_t m = std::min(head - tail, room);
  const size_t nb = (size_t)c->probe.bins;
  if (m > 0) {
    HIPCHK(hipMemcpyAsync(rows, c->probe.rows + tail * kProbeFields, (size_t)m * kProbeFields * sizeof(double),
                          hipMemcpyDeviceToHost, c->stream));
    std::vector<unsigned long long> keys((size_t)m * nb);
    if (nb > 0) {
      HIPCHK(hipMemcpyAsync(counts, c->probe.counts + tail * nb, (size_t)m * nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(keys.data(), c->probe.tops + tail * nb, keys.size() * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    probe_decode_tops(keys.data(), tops, (int64_t)keys.size());
  }
  c->probe.tail = tail + m;
  if (c->probe.tail == head) {  // all of it has been read: the log starts over, its bins empty
    if (nb > 0 && head > 0 && (rc = probe_clear(c, c->probe.counts, c->probe.tops, (size_t)head * nb))) return rc;
    HIPCHK(hipMemsetAsync(c->probe.words + PW_HEAD, 0, sizeof(int), c->stream));
    c->probe.tail = 0;
  }
  if (words[PW_DROPPED]) HIPCHK(hipMemsetAsync(c->probe.words + PW_DROPPED, 0, sizeof(int), c->stream));
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

}  // extern "C"
