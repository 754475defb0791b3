/*
 * sandcrate_hip.h -- C ABI of libsandcrate_hip.so: the MI355X (gfx950) implementation of
 * SandCrate's per-timestep particle update.
 *
 * The reference has no FFI (it is pure Python/NumPy); this header is the boundary a
 * maintainer binds with ctypes (INTEGRATION.md shows the stub).  Each entry point names the
 * reference code it replaces as  file:line  relative to the reference repository.
 *
 * Conventions
 *   - every function returns 0 on success, a negative SC_ERR_* otherwise; the message of the
 *     last failure on the calling thread is sc_last_error().  Nothing throws across the ABI and
 *     nothing calls back into the host language.
 *   - host arrays are caller-allocated, C-contiguous, float64 / int64 / int32 exactly as NumPy
 *     holds them (particles are P x 2 interleaved x,y like crate.py:24-25); the library owns all
 *     device memory.  Device state is float64 SoA (x, y, vx, vy) in cell-sorted order plus a
 *     per-particle id that remembers the reference's particle index order.
 *   - one context per GPU, one calling thread per context.  Calls are enqueued on the context's
 *     HIP stream and return before the GPU finishes unless the description says "synchronises".
 */
#ifndef SANDCRATE_HIP_H
#define SANDCRATE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_ABI_VERSION 5
#define SC_MAX_NEIGHBORS 20 /* collision_detector.py:6  MAX_ALLOWED_NEIGHBORS */
#define SC_MAX_SEGMENTS 16  /* wall segments of all rigid bodies together (scenes use 6 and 8) */
#define SC_MAX_BODIES 8

enum {
  SC_OK = 0,
  SC_ERR_ARG = -1,      /* bad argument */
  SC_ERR_HIP = -2,      /* HIP runtime failure, see sc_last_error() */
  SC_ERR_CAPACITY = -3, /* more particles / cells than the context was created for */
  SC_ERR_STATE = -4,    /* call order violated (e.g. sc_step_finish without sc_step_begin) */
  SC_ERR_DOMAIN = -5    /* a particle fell outside the cell grid (NaN or runaway position) */
};

/* Collider noise of crate.py:169 ((rand(C_i,2) - 0.5) * diameter * collider_noise_level). */
enum {
  SC_NOISE_NONE = 0,    /* eta = 0 (what collider_noise_level = 0 gives) */
  SC_NOISE_HOST = 1,    /* uniforms supplied per tick by sc_set_noise_host: the host's MT19937 stream */
  SC_NOISE_COUNTER = 2  /* counter-based hash of (seed, tick, particle id, slot); no host traffic */
};

/* Live-editable coefficients: the YAML keys of config/ *.yaml:10-22 that the tick reads
 * (crate.py:55-57).  spring_* are inert in the reference (crate.py:117-118) and absent here. */
typedef struct sc_params {
  double dt;
  double particle_radius;
  double wall_collision_decay;
  double pressure_amplifier;
  double ignored_pressure;
  double collider_noise_level;
  double viscosity;
  double surface_smoothing;
  double target_pressure;
  double gravity_x;
  double gravity_y;
} sc_params;

/* One rigid body after RigidBody.apply_velocity (rigid_body.py:42-46, :64-68): what
 * calc_body_points_velocities (rigid_body.py:28-34) needs, and how many of the stacked
 * segments (crate.py:69-71) belong to it. */
typedef struct sc_body {
  double position_x, position_y;
  double center_velocity_x, center_velocity_y;
  double angular_clockwise_velocity;
  int32_t n_segments;
  int32_t reserved;
} sc_body;

typedef struct sc_stats {
  int64_t particles;      /* P after remove_particles (crate.py:149-159) */
  int64_t neighbor_slots; /* sum of C_i: how many (rand, rand) pairs crate.py:169 draws this tick */
  int32_t max_neighbors;  /* max C_i */
  int32_t wall_particles; /* particles with at least one wall contact (crate.py:229) */
  int32_t flags;          /* nonzero: an error condition seen on the device (reported by the next synchronising call).
                           * With SC_FLAG_SCAN_TIMEOUT the tick is abandoned (sc_set_scan_patience): `particles` is the
                           * stored count, the other numbers are 0 -- the host draws no noise for such a tick */
  int32_t reserved;
} sc_stats;
#define SC_FLAG_SCAN_TIMEOUT 64

typedef struct sc_ctx sc_ctx;

const char* sc_last_error(void);
int sc_abi_version(void);

/* Lifetime.  capacity = most particles the context will ever hold (Crate: max_particles). */
int sc_create(int device, int64_t capacity, sc_ctx** out);
int sc_destroy(sc_ctx* ctx);
/* Run on this hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) instead of the context's
 * own stream; NULL is HIP's default stream, as everywhere in HIP.  sc_use_own_stream goes back to
 * the private non-blocking stream the context was created with.  Both synchronise the old stream. */
int sc_set_stream(sc_ctx* ctx, void* hip_stream);
int sc_use_own_stream(sc_ctx* ctx);

/* State in/out.  Replaces direct assignment of Crate.particles / particle_velocities
 * (crate.py:24-25).  Particle i gets id i; ids order ties exactly like the reference's
 * array index does (collision_detector.py:127 lexsort is stable). */
int sc_upload_state(sc_ctx* ctx, const double* xy, const double* vxy, int64_t n);
/* crate.py:138-147 create_new_particles: appended particles get the next ids. */
int sc_append_particles(sc_ctx* ctx, const double* xy, const double* vxy, int64_t n);
/* Synchronises.  Number of live particles. */
int sc_count(sc_ctx* ctx, int64_t* n);
/* Synchronises.  Writes live particles in id order (= the reference's array order): xy, vxy are
 * n x 2, pressure (crate.py:275 particles_pressure) and ids are n.  Any pointer may be NULL.
 * n_capacity is the room in the host arrays; *n_out is what was written. */
int sc_download_state(sc_ctx* ctx, double* xy, double* vxy, double* pressure, int64_t* ids,
                      int64_t n_capacity, int64_t* n_out);

/* Per-tick inputs.  Coefficients are re-sent every tick because the viewer edits them live
 * (playback.py:221-226); segments because bodies move (crate.py:363-365). */
int sc_set_params(sc_ctx* ctx, const sc_params* p);
/* segments: n_segments x 2 x 2 (crate.py:69-71); padded: 2*n_segments x 2 x 2 from pad_segments
 * (geometry_utils.py:146-172), computed on the host because it is O(S). */
int sc_set_segments(sc_ctx* ctx, const double* segments, const double* padded, int32_t n_segments,
                    const sc_body* bodies, int32_t n_bodies);
int sc_set_noise_mode(sc_ctx* ctx, int mode, uint64_t seed);

/* The tick: crate.py:91-129 from remove_particles on.
 *   sc_step_begin  : remove_particles (:149-159), calc_virtual_colliders + hard wall fix (:97-99,
 *                    :202-243), strip sort + neighbor lists (collision_detector.py:9-49)
 *   sc_step_stats  : synchronises; P and sum C_i, so the host can draw rand(sum C_i, 2)
 *   sc_set_noise_host: those uniforms, (n_pairs x 2) in particle-index order, slot-minor (:169)
 *   sc_step_finish : populate_colliders ... apply_particles_velocity (:103-125)
 * sc_step(ctx, k) = k x (begin, finish) with no synchronisation; not valid in SC_NOISE_HOST mode. */
/* Look-ahead for back-to-back ticks (optional; between sc_step_begin and sc_step_finish).  Declares the
 * coefficients and walls of the tick AFTER the one being finished.  sc_step_finish then also performs
 * that next tick's remove_particles / calc_virtual_colliders / apply_hard_wall_fix and the bucket counts
 * (crate.py:93, :97-99) in the epilogue of the force kernel, while the new position is still in
 * registers, and the next sc_step_begin skips them: one launch and one pass over the positions less per
 * tick.  The promise is binding: the next tick must be started with exactly these inputs and without
 * appending particles in between, otherwise sc_step_begin / sc_append_particles return SC_ERR_STATE.
 * (Crate.physics_tick() never promises -- the viewer may edit coefficients between ticks; Crate.run()
 * and sc_step(ctx, k > 1) do.)  Not used with slabs. */
int sc_set_next_inputs(sc_ctx* ctx, const sc_params* p, const double* segments, int32_t n_segments,
                       const sc_body* bodies, int32_t n_bodies);
int sc_step_begin(sc_ctx* ctx);
int sc_step_stats(sc_ctx* ctx, sc_stats* out);
int sc_set_noise_host(sc_ctx* ctx, const double* u01, int64_t n_pairs);
int sc_step_finish(sc_ctx* ctx);
int sc_step(sc_ctx* ctx, int32_t n_ticks);
/* One whole tick in ONE call, for drivers whose per-call overhead matters (ctypes: ~4 us per call):
 *   sc_set_params(now) + sc_set_segments(now) + sc_step_begin + [sc_set_next_inputs(next)] + sc_step_finish.
 * `next` may be NULL (no look-ahead).  Same errors as the calls it stands for; in SC_NOISE_HOST mode
 * valid only when the device holds the stream (sc_rng_set_state) -- otherwise the host has to draw the noise
 * between begin and finish (crate.py:169). */
typedef struct sc_tick_inputs {
  sc_params params;
  const double* segments; /* n_segments x 2 x 2 (crate.py:69-71) */
  const double* padded;   /* 2 n_segments x 2 x 2 (geometry_utils.py:146-172) */
  const sc_body* bodies;
  int32_t n_segments, n_bodies;
} sc_tick_inputs;
int sc_tick(sc_ctx* ctx, const sc_tick_inputs* now, const sc_tick_inputs* next);
int sc_synchronize(sc_ctx* ctx);

/* The bucket scan is one pass with decoupled look-back: a workgroup waits for the totals of the workgroups before it,
 * which the dispatcher starts first.  The wait is bounded -- `polls` attempts per predecessor (default 2^22; negative:
 * give up at once, for tests) -- and a workgroup that gives up abandons the TICK: its later kernels do nothing, the particles
 * stay as the tick found them, and the next synchronising call returns SC_ERR_HIP.  (A knob for tests of that path.)
 *
 * What an abandoned tick leaves, and what the caller may do after it:
 *   - The state is the one the tick found, but for the hard wall fix of the tick's first kernel, which runs ahead of the
 *     scan and in place (crate.py:202-211, applied once): velocities, ids and the count are exact, the pressures are those
 *     of the last finished tick.  The tick counter has advanced (SC_NOISE_COUNTER keys the noise by it); the stream of
 *     SC_NOISE_HOST has not moved, whether the device holds it or the host draws it (sc_step_stats says so: no noise).
 *   - Every tick started before the error is read is abandoned whole -- it does not even apply a wall fix.
 *   - The error is read, cleared and repaired by sc_synchronize and sc_download_state, whichever is called first, exactly
 *     once; the run then goes on from the stored state (a tick, an upload, an append) as if the abandoned ticks had not
 *     been asked for.  sc_synchronize BETWEEN sc_step_begin and sc_step_finish reports it too but leaves the rest of the
 *     tick abandoned: the first of the two calls after sc_step_finish reports it again and repairs.  sc_count does not
 *     read errors.
 *   - Before that reader, calls that only read the state on the device -- sc_export_state_device, sc_render*,
 *     sc_probe_now, sc_track_capture -- deliver it as described above: positions, velocities, ids and count exact,
 *     pressures those of the last finished tick, exactly what sc_download_state then returns.
 *   - The logs (sc_probe_enable, sc_track_enable) hold NO row / frame for an abandoned tick, and count none as dropped:
 *     every row is the state after a tick that happened. */
int sc_set_scan_patience(sc_ctx* ctx, int64_t polls);

/* Parity taps, valid between sc_step_begin and sc_step_finish.  Synchronise.  All arrays have one
 * entry per sorted slot k = 0..P-1 (the order of collision_detector.py:127):
 *   y_floored[k]  row index floor(y/d) (collision_detector.py:126)
 *   ids[k]        particle id in that slot (= sorted_indices when ids are array indices)
 *   counts[k]     C of that particle, neighbors[k*20 + s] the id of its s-th neighbor or -1
 *   fixed_xy[k*2] position after apply_hard_wall_fix (crate.py:202-211) */
int sc_download_sort(sc_ctx* ctx, int64_t* y_floored, int64_t* ids, int64_t n_capacity, int64_t* n_out);
int sc_download_neighbors(sc_ctx* ctx, int64_t* ids, int32_t* counts, int64_t* neighbors, double* fixed_xy,
                          int64_t n_capacity, int64_t* n_out);
/* After sc_step_finish: surface normals s_i of apply_tension pass 1 (crate.py:337-342) in id order. */
int sc_download_normals(sc_ctx* ctx, double* sxy, int64_t n_capacity, int64_t* n_out);
/* After sc_step_finish: the pressures of apply_pressure pass 1 (crate.py:261-275) in id order, one per particle of the
 * finished tick -- those whose position the tick left NaN included, which sc_download_state no longer lists. */
int sc_download_pressure(sc_ctx* ctx, double* pressure, int64_t n_capacity, int64_t* n_out);

/* Stand-alone forms of two reference functions (its tests/test_distance.py pins both).
 * sc_neighbor_search = detect_particle_collisions (collision_detector.py:9-49) on arbitrary
 * coordinates: y_floored/sorted_indices per sorted slot, counts[i] and table[i*20+s] per ORIGINAL
 * index i, -1 padded.  sc_points_to_segments = points_to_segments_distance
 * (geometry_utils.py:7-39): nearest is n x s x 2, distances n x s. */
int sc_neighbor_search(int device, const double* xy, int64_t n, double diameter, int64_t* y_floored,
                       int64_t* sorted_indices, int32_t* counts, int64_t* table);
int sc_points_to_segments(int device, const double* xy, int64_t n, const double* segments, int32_t n_segments,
                          double* nearest, double* distances);
/* pad_segments (geometry_utils.py:146-172) on the host, the reference's operations in its order: `padded` receives
 * 2 * n_segments segments, first every (a + o, b + o), then every (b - o, a - o), o = cw90(b - a) * pad_distance / |b - a|.
 * No GPU involved: the padded twins of a moving wall are a kernel argument of every tick (sc_set_segments). */
int sc_pad_segments(const double* segments, int32_t n_segments, double pad_distance, double* padded);

/* Kernel timing with HIP events on the context's stream.  While enabled every kernel launch is
 * bracketed by two events; sc_get_timing synchronises and returns, per kernel, the summed
 * milliseconds and the number of launches since sc_reset_timing.  Names: sc_kernel_name(i). */
#define SC_NUM_KERNELS 12
int sc_enable_timing(sc_ctx* ctx, int on);
int sc_reset_timing(sc_ctx* ctx);
int sc_get_timing(sc_ctx* ctx, double* ms /*[SC_NUM_KERNELS]*/, int64_t* launches /*[SC_NUM_KERNELS]*/);
const char* sc_kernel_name(int index);

/* Multi-GPU slabs (of columns, or of rows: sc_set_slab_axis) (no reference counterpart).  One context per GPU owns the
 * grid columns [col_lo, col_hi), column = floor(x / diameter) of the position a particle has when
 * the tick starts.  Particles within `halo` columns outside the slab are ghosts: they take part in
 * the wall fix, the neighbor search and pass A exactly like owned particles, are never integrated,
 * and are dropped at the end of the tick.  Three columns reach all an owned particle needs as long as no hard wall
 * fix exceeds one radius along the slab axis (one contact never does; a joint of two segments can).  A fix that does,
 * on an owned particle that is put at least half a column beyond the slab's edge, or comes from beyond the band to
 * less than 2.5 columns from the edge, is reported: SC_ERR_DOMAIN at the next synchronising call.
 * A particle that crosses a whole slab in one tick -- sc_halo_unpack finds a record from the left beyond the slab's
 * right edge, or the mirror image -- belongs to a slab that never receives it: reported the same way.
 * Ids are global (sc_upload_state_ids), so tie-breaks and
 * the counter-based noise are the same as on one GPU.  Not available with SC_NOISE_HOST.
 *
 * Per tick:  sc_halo_pack -> exchange the two buffers with the neighbors (RCCL send/recv on
 * the stream given to sc_set_stream, or any transport) -> sc_halo_unpack of the two received buffers
 * (either pointer may be NULL at a domain edge) -> the tick.  Buffers are DEVICE memory of
 * (capacity_records + 1) * 5 doubles, caller-owned (e.g. torch tensors) and zero-initialised: record 0 is
 * a header whose first 32-bit word is the record count, records 1.. are (x, y, vx, vy, id).
 * sc_halo_pack writes every stored particle within `halo` columns of the left / right edge, including
 * particles that have already moved out of the slab on that side (migrants: the receiver owns them from
 * this tick on).  sc_halo_unpack also re-arms the headers of the send buffers, which must therefore have
 * been sent (in stream order) by then.  Nothing here synchronises.
 *
 * Look-ahead: the buffers given to the last sc_halo_pack stay bound to the context.  A tick whose successor
 * was promised (sc_set_next_inputs / sc_tick with `next`) packs the successor's halo message in the epilogue
 * of its force kernel, and the following sc_halo_unpack runs the removal / wall pass for what it appends; the
 * steady-state slab tick is then:  exchange -> sc_halo_unpack -> sc_tick(now, next).  Calling sc_halo_pack
 * for a tick that was packed this way is refused (SC_ERR_STATE). */
int sc_set_slab(sc_ctx* ctx, int64_t col_lo, int64_t col_hi, int32_t halo, int32_t has_left, int32_t has_right);
/* Which way the domain is cut: axis 0 (the default) -- slabs are ranges of COLUMNS floor(x / d), "left" / "right"
 * are the neighbors towards smaller / larger x; axis 1 -- ranges of ROWS floor(y / d), neighbors towards smaller /
 * larger y (sc_set_slab's col_lo / col_hi, the histogram of sc_column_histogram and `halo` then count rows).  The
 * sorted order is row-major, so with rows the halo bands are the first and last few blocks of it: the blocks
 * that may pack halo records (sc_set_halo_overlap) are a percent of all instead of a third.  Call before
 * sc_set_slab; results do not depend on the axis. */
int sc_set_slab_axis(sc_ctx* ctx, int32_t axis);
int sc_upload_state_ids(sc_ctx* ctx, const double* xy, const double* vxy, const int64_t* ids, int64_t n);
/* crate.py:138-147 under slabs: every rank draws the same new particles (same host stream) and appends the ones whose
 * column / row it owns, under their global ids. */
int sc_append_particles_ids(sc_ctx* ctx, const double* xy, const double* vxy, const int64_t* ids, int64_t n);
int sc_halo_pack(sc_ctx* ctx, double* dev_left, double* dev_right, int64_t capacity_records);
/* Message sizes.  A message need not carry the whole buffer: sc_halo_sizes gives, for the exchange of the coming
 * tick, the number of records (after the header record) to send to / receive from each side -- the count the same
 * direction had six ticks earlier plus 50 % and 1024 records, in steps of 256, at most capacity_records.  Sender
 * and receiver of a message derive it from the same number (what was packed = what the received header said;
 * sc_halo_unpack publishes both in host-mapped memory), so the two ends agree without talking; the lag exceeds
 * the number of ticks the host may run ahead of the device, so nothing synchronises.  Whole buffers for the
 * first ticks after an upload or sc_set_slab.  sc_halo_unpack is told how many records each message carried; a
 * header that announces more sets the halo-overflow condition (SC_ERR_CAPACITY at the next synchronising call). */
int sc_halo_sizes(sc_ctx* ctx, int64_t capacity_records, int64_t* send_left_records, int64_t* recv_left_records,
                  int64_t* send_right_records, int64_t* recv_right_records);
int sc_halo_unpack(sc_ctx* ctx, const double* dev_from_left, int64_t left_records, const double* dev_from_right,
                   int64_t right_records);
/* Slab re-balancing: stored live particles per grid column floor(x / diameter), columns clamped into
 * [col0, col0 + n_columns).  Every particle is stored live on exactly one rank, so the ranks' histograms add up
 * to the global one, from which all ranks derive the same new cuts (sc_set_slab; the next halo exchange moves
 * the particles that changed owner).  Synchronises. */
int sc_column_histogram(sc_ctx* ctx, int64_t col0, int32_t n_columns, int64_t* histogram);
/* RCCL transport for the exchange step (optional: any transport that moves the buffers between the
 * calls above will do; sand_crate_amd.slab falls back to torch.distributed P2P ops).  librccl is dlopen()ed
 * on first use -- the copy already loaded in the process if any, else `rccl_path`, else the default search
 * path -- so the library itself has no link-time dependency on it.
 *   sc_comm_available  0 when librccl can be loaded in this process: every rank checks (and the ranks agree on
 *                      the answer) BEFORE any of them enters the collective sc_comm_init
 *   sc_comm_unique_id  rank 0: 128 bytes to hand to every rank (ncclGetUniqueId)
 *   sc_comm_init       collective over the `world` contexts of the slab chain (ncclCommInitRank); rank = slab index
 *   sc_halo_exchange   on the context's stream, one group: send `send_left` to / receive `recv_left` from
 *                      rank `left_rank`, the same on the right; a negative rank means no neighbor on that side.
 *                      Each message is (records + 1) * 5 doubles from the start of its buffer (sc_halo_sizes).
 * A failing RCCL call returns SC_ERR_HIP with RCCL's message in sc_last_error(). */
int sc_comm_available(const char* rccl_path);
int sc_comm_unique_id(const char* rccl_path, void* id_128_bytes);
int sc_comm_init(sc_ctx* ctx, const char* rccl_path, const void* id_128_bytes, int32_t rank, int32_t world);
int sc_comm_destroy(sc_ctx* ctx);
int sc_halo_exchange(sc_ctx* ctx, const double* send_left, int64_t send_left_records, double* recv_left,
                     int64_t recv_left_records, int32_t left_rank, const double* send_right, int64_t send_right_records,
                     double* recv_right, int64_t recv_right_records, int32_t right_rank);

/* Force monitor: the reference's HUD shows the mean |dv| of each force phase (force_monitor.py:13-37 around
 * crate.py:110-123).  While enabled, the force kernel also sums |dv| per particle and phase -- tension, gravity,
 * pressure, viscosity, wall_bounce, continuous_collision, in this order -- without changing any result (ticks are
 * then never fused with their successor's wall pass).  sc_get_force_monitor returns the six sums and the number
 * of particles summed since the last call and clears them; it synchronises. */
int sc_enable_force_monitor(sc_ctx* ctx, int on);
int sc_get_force_monitor(sc_ctx* ctx, double* sums_6, int64_t* particles);

/* Checkpoint.  sc_checkpoint_begin copies the stored state (positions, velocities, ids, counters, the MT19937
 * stream if the device holds it) device-to-device on the context's stream and sends the copy to pinned host memory
 * on a side stream; it returns at once and later ticks overlap the transfer.  sc_checkpoint_finish waits for that
 * transfer only and delivers the particles in particle-index order with the tick they belong to, the id the next
 * emitted particle gets, and the generator state (rng_position = -1: the host holds the stream).  One checkpoint
 * at a time.  sc_restore_counters, after sc_upload_state_ids on a fresh context, puts tick and next id back. */
int sc_checkpoint_begin(sc_ctx* ctx);
int sc_checkpoint_finish(sc_ctx* ctx, double* xy, double* vxy, int64_t* ids, int64_t room, int64_t* n_out, int64_t* tick,
                         int64_t* next_id, uint32_t* rng_key_624, int32_t* rng_position);
int sc_restore_counters(sc_ctx* ctx, int64_t tick, int64_t next_id);

/* NumPy's legacy global generator on the device (the reference draws particle sources and collider noise from
 * `np.random`, seeded in Crate.__init__, crate.py:22).  sc_rng_set_state hands the stream to the context -- the
 * 624-word key and the position of `np.random.get_state()` -- and from then on
 *   sc_emit_particles  runs ParticleSource.generate_particles (particle_source.py:17-24) for the given sources,
 *                      any number of them, in order on the device: binomial(flow, dt) new particles each (the legacy
 *                      inversion branch up to flow * dt = 30, BTPE beyond; a flow of 0 draws its one double and emits
 *                      nothing; SC_ERR_DOMAIN if flow < 0, dt <= 0 or dt > 0.5), rand(n, 2) position jitter, rand(n, 2) velocity noise, capped at max_particles minus
 *                      the count the previous sources left (a source capped at 0 or less draws its binomial only),
 *                      appended with the next ids;
 *   sc_step_finish     in SC_NOISE_HOST mode without a sc_set_noise_host call draws the tick's rand(sum C_i, 2)
 *                      block on the device,
 * bit for bit the numbers NumPy would have produced, with no count readback and no upload.  sc_rng_get_state
 * (synchronises) returns the stream to the host, e.g. for `np.random.set_state`. */
typedef struct sc_source {
  double radius, position_x, position_y, velocity_x, velocity_y, noise;
  int64_t flow;
} sc_source;
int sc_rng_set_state(sc_ctx* ctx, const uint32_t* key_624, int32_t position);
int sc_rng_get_state(sc_ctx* ctx, uint32_t* key_624, int32_t* position);
int sc_emit_particles(sc_ctx* ctx, const sc_source* sources, int32_t n_sources, double dt, int64_t max_particles);

/* Halo overlap (BASELINE.json configs[4]: "halo overlap on side HIP stream").  With it on, a tick whose successor
 * was promised runs its force kernel in two launches: first the blocks that hold a particle within the halo band
 * plus two columns of a cut -- the only ones that can pack halo records -- then the interior blocks; the exchange
 * of the coming tick waits for the first launch only and runs on the context's side stream next to the second.
 *   sc_halo_exchange        does both waits itself (RCCL calls go to the side stream);
 *   sc_halo_overlap_begin   for other transports: the side stream waits for what the coming message depends on
 *                           (`peer`, optional: and for what that context's message depends on -- in-process chains);
 *                           the caller then enqueues its copies / sends on sc_side_stream;
 *   sc_halo_overlap_end     the context's stream waits for the side stream; sc_halo_unpack follows as usual.
 * A particle of an interior block that ends the tick inside a band after all (it moved more than the margin: two
 * columns / eight rows) is not silently lost: SC_ERR_DOMAIN at the next synchronising call.
 *
 * sc_set_band_flag (slabs of rows only): instead of two launches the force kernel runs as ONE whose first workgroups
 * take the blocks at both ends of the sorted order (where the band blocks are); the last of them to finish publishes
 * a flag, and the side stream waits for it with a one-thread polling kernel (hipStreamWaitValue32 is not usable
 * here).  Costs ~4 us per tick instead of ~24 -- PROVIDED the side stream has a hardware queue of its own: a process
 * with more streams than hardware queues may put the polling kernel in front of the very kernel it waits for, which
 * then costs the poll's time-out (50 ms, reported as SC_ERR_HIP).  Off by default; bench.py tries it and keeps it when
 * it is faster. */
int sc_set_halo_overlap(sc_ctx* ctx, int on);
int sc_set_band_flag(sc_ctx* ctx, int on);
int sc_side_stream(sc_ctx* ctx, void** hip_stream);
int sc_halo_overlap_begin(sc_ctx* ctx, sc_ctx* peer);
int sc_halo_overlap_end(sc_ctx* ctx);

/* Frames: what Playback.draw_scene draws (playback.py:75-85) -- every particle as a disc coloured by its pressure
 * (playback.py:191-206), the walls on top in white (:180-186), black elsewhere -- rendered next to the state into an
 * RGB image of height x width x 3 bytes, row 0 at the top (the layout of pygame.image.tostring(..., 'RGB')).  The
 * particles and pressures drawn are exactly what sc_download_state would return; among discs that cover a pixel the
 * highest id wins (the reference draws in array order).  tests/render_spec.py is the raster rule, bit for bit.
 * Rendering reads the state only: no counter, look-ahead promise, RNG position or pending error flag changes.
 * SC_ERR_STATE between sc_step_begin and sc_step_finish; SC_ERR_ARG for a bad view, a null buffer, or n_segments
 * outside 0..SC_MAX_SEGMENTS.  The device buffers it needs grow to the largest frame asked for. */
typedef struct sc_view {
  int32_t width, height;      /* 1..16384 */
  double zoom;                /* finite, > 0 */
  double center_x, center_y;  /* screen pixels; reference default width/2, height/2 */
  double particle_radius;     /* world units */
  int32_t segment_width;      /* pixels, >= 0 */
  int32_t reserved;
} sc_view;
/* Synchronises; rgb is host memory of height*width*3 bytes. */
int sc_render(sc_ctx* ctx, const sc_view* view, const double* segments, int32_t n_segments, uint8_t* rgb);
/* Enqueued on the context's stream only; dev_rgb is device memory (e.g. a torch uint8 tensor). */
int sc_render_device(sc_ctx* ctx, const sc_view* view, const double* segments, int32_t n_segments, uint8_t* dev_rgb);

/* JPEG frames: baseline sequential JPEG (JFIF, SOF0), 8-bit Y Cb Cr sampled 4:4:4, the Annex K quantisation tables scaled
 * by the IJG quality rule (quality 1..100) and the Annex K Huffman tables, a restart interval of one MCU row.  The image
 * is encoded on the device; only the compressed bytes reach `out` (host memory).  tests/jpeg_spec.py is the bitstream,
 * byte for byte.  Both calls synchronise.  *n_out is set to the file's size; if that exceeds `capacity`, nothing is
 * written and SC_ERR_CAPACITY is returned (out may be null with capacity 0 to ask for the size).  sc_jpeg_bound gives a
 * capacity that always suffices.  SC_ERR_STATE between sc_step_begin and sc_step_finish; SC_ERR_ARG for a bad size,
 * quality or pointer.  The device workspace grows to the largest frame asked for (about 16 bytes per pixel). */
int sc_jpeg_bound(int32_t width, int32_t height, int64_t* bound);
/* dev_rgb: device memory of height*width*3 bytes, row 0 at the top (e.g. written by sc_render_device).  The context's
 * stream does not wait for other streams: the frame must be ready when this is called. */
int sc_jpeg_encode_device(sc_ctx* ctx, const uint8_t* dev_rgb, int32_t width, int32_t height, int32_t quality, uint8_t* out,
                          int64_t capacity, int64_t* n_out);
/* sc_render into a frame owned by the context, then that frame encoded as sc_jpeg_encode_device does. */
int sc_render_jpeg(sc_ctx* ctx, const sc_view* view, const double* segments, int32_t n_segments, int32_t quality,
                   uint8_t* out, int64_t capacity, int64_t* n_out);

/* GIF frames: the image data of one frame of an animated GIF (the LZW minimum code size 8, the data sub-blocks, the
 * block terminator) over a fixed palette of 256 colours: entry 0 is black, entry k is (k, k, 255).  A frame of sc_render
 * is a palette image by construction: the background is index 0, a wall 255, a disc of colour byte c max(c, 1) -- the
 * one loss is that (0, 0, 255), a pressure of 1 and above, is stored as (1, 1, 255).  The LZW dictionary is restarted
 * with a clear code every 1024 pixels, so the frame is compressed on the device in independent chunks; only the
 * compressed bytes reach `out` (host memory).  tests/gif_spec.py is the bitstream, byte for byte, and
 * sand_crate_amd/gif.py (GifWriter) puts such frames into a file.  Both calls synchronise.  *n_out is always set, to the
 * size of the image data once the arguments are valid; if that exceeds `capacity`, nothing is written and
 * SC_ERR_CAPACITY is returned (out may be null with capacity 0 to ask for the size).  sc_gif_bound gives a capacity that
 * always suffices.  SC_ERR_STATE between sc_step_begin and sc_step_finish; SC_ERR_ARG for a bad size (each side
 * 1..16384) or pointer.  The device workspace grows to the largest frame asked for (about 5 bytes per pixel). */
int sc_gif_bound(int32_t width, int32_t height, int64_t* bound);
/* dev_index: device memory of height*width palette indices, row 0 at the top.  The context's stream does not wait for
 * other streams: the frame must be ready when this is called. */
int sc_gif_encode_device(sc_ctx* ctx, const uint8_t* dev_index, int32_t width, int32_t height, uint8_t* out,
                         int64_t capacity, int64_t* n_out);
/* sc_render's frame, resolved to palette indices in a buffer owned by the context, then encoded as
 * sc_gif_encode_device does. */
int sc_render_gif(sc_ctx* ctx, const sc_view* view, const double* segments, int32_t n_segments, uint8_t* out,
                  int64_t capacity, int64_t* n_out);

/* HUD: the text the reference's viewer draws at the top left of every frame (Playback.draw_debug_text, playback.py:215-219;
 * Crate.debug_prints is that text).  From this call on every frame made by sc_render, sc_render_device, sc_render_jpeg and
 * sc_render_gif carries `text` in white -- (255, 255, 255), palette index 255 -- drawn over the discs and walls before an
 * encoder reads the frame, in a built-in bitmap font, not antialiased: ASCII 0x20..0x7E in cells of 8 x 16 pixels, any
 * other byte drawn as '?'.  The text is split into lines at '\n'; line l starts at pixel row y + l * 18 * scale,
 * character k of a line at pixel column x + k * 8 * scale, a glyph bit covers scale x scale pixels, pixels outside the
 * frame are dropped.  tests/text_spec.py is the pixel rule, bit for bit.  The text is copied (it need not end in a zero
 * byte); n_bytes == 0 clears the HUD (text may then be null), and a new context has none.  Synchronises the context's
 * stream: frames enqueued before the call keep the text they were enqueued with.  Like rendering it leaves the simulation
 * alone.  SC_ERR_ARG for n_bytes outside 0..65536, a null text with n_bytes > 0, x or y outside 0..16384 or scale
 * outside 1..64; the HUD is then what it was. */
int sc_set_hud(sc_ctx* ctx, const char* text, int32_t n_bytes, int32_t x, int32_t y, int32_t scale);

/* Debug arrows: the layer the reference's viewer draws between the walls and the HUD text (Playback.draw_debug_arrows,
 * playback.py:95-107).  From this call on every frame made by sc_render, sc_render_device, sc_render_jpeg and
 * sc_render_gif carries the arrows in green -- (0, 255, 0), palette index 1 -- drawn over the discs and walls after
 * resolve, before the HUD text and before an encoder reads the frame.  An arrow runs from `start` to `end`, both in world
 * units and mapped to the screen as the walls' ends are (not floored): a body two pixels wide that stops two pixels
 * before `end` and a head four pixels wide with its tip on `end`, pygame_utils.draw_arrow with the viewer's sizes;
 * shorter than two pixels it is the head alone.  An arrow with a number that is not finite, or whose ends fall on the
 * same screen point, draws nothing; pixels outside the frame are dropped.  tests/arrow_spec.py is the pixel rule, bit
 * for bit.
 *   SC_ARROWS_OFF       none.  A new context has none.
 *   SC_ARROWS_LIST      the `n` arrows at `arrows`, 0..1,048,576 of them; n == 0 is SC_ARROWS_OFF.  The list is copied.
 *   SC_ARROWS_VELOCITY  nothing is uploaded: one arrow for every stored live particle whose id is a multiple of `every`
 *                       (>= 1), as of the frame's own time: from its position p to p + d / (|d| + 0.001)^0.3 with
 *                       d = velocity * scale (`scale` finite), the compression of playback.py:99, computed on the device
 *                       (its pow may differ from the host's in the last bits).  Positions and velocities are those
 *                       sc_download_state returns; particles that are not finite (the dead ghost copies of slab mode
 *                       among them) are skipped.
 * While arrows are set, sc_render_gif stores a disc of colour byte c as palette index max(c, 2) instead of max(c, 1):
 * index 1 is the arrows', and a GIF's colour table needs (0, 255, 0) there (gif.py: palette(arrows=True)).
 * Synchronises the context's stream: frames enqueued before the call keep the arrows they were enqueued with.  Like
 * rendering it leaves the simulation alone.  SC_ERR_ARG for an unknown mode, n outside 0..1,048,576, a null list with n > 0,
 * every < 1 or a scale that is not finite -- each checked in every mode, so SC_ARROWS_OFF is (ctx, SC_ARROWS_OFF, NULL, 0,
 * 1.0, 1); the arrows are then what they were.
 * SC_ERR_STATE between sc_step_begin and sc_step_finish. */
typedef struct sc_arrow { double start_x, start_y, end_x, end_y; } sc_arrow;   /* world units */
enum { SC_ARROWS_OFF = 0, SC_ARROWS_LIST = 1, SC_ARROWS_VELOCITY = 2 };
int sc_set_arrows(sc_ctx* ctx, int32_t mode, const sc_arrow* arrows, int64_t n, double scale, int64_t every);

/* Synchronises.  Live particles stored in this context (dead ghost copies excluded); summed over
 * the ranks this is the global particle count. */
int sc_owned_count(sc_ctx* ctx, int64_t* n);

/* The probe: numbers instead of pictures.  One pass over the stored state (40 bytes per particle) reduces it on the
 * device to a row of SC_PROBE_FIELDS float64 values and, with n_bins > 0, a profile of the free surface; the particles and
 * pressures measured are exactly what sc_download_state would return (particles whose x is not finite, |x| < 1e300 as in
 * sc_owned_count, are skipped).  tests/probe_spec.py is the rule.  The row:
 *    0 tick          ticks finished by the context when the state was measured
 *    1 n             live particles
 *    2..5            sum_x, sum_y, sum_vx, sum_vy
 *    6 sum_ke        sum of 0.5 (vx vx + vy vy)
 *    7 sum_p         sum of the pressures
 *    8..11           min_x, max_x, min_y, max_y (+inf / -inf for an empty crate)
 *   12 max_speed2    max of vx vx + vy vy and 0        13 max_p   max of the pressures and 0
 *   14 n_pressed     particles with pressure > 0       15 n_binned  particles that fell into a bin of the profile
 * The profile: bin k of n_bins (0..SC_PROBE_MAX_BINS) over [x0, x1) holds the particles with floor((x - x0) / w) == k,
 * w = (x1 - x0) / n_bins in float64; counts[k] is how many, tops[k] the smallest y among them -- gravity points to +y, so
 * that is the free surface -- or +inf for an empty bin.
 * Counts, minima, maxima, max_speed2 (vx vx + vy vy is not contracted) and the profile are exact.  The six sums are added
 * in an order that depends on the stored particle count alone and with no floating-point atomics: the same state measured
 * twice, or once by the log and once on demand, gives the same 128 bytes; against another order of summation they differ
 * by rounding (probe_spec.py states the bound).  A NaN velocity or pressure at a finite position counts and propagates.
 *
 * sc_probe_now     one measurement of the state as it stands; synchronises.  counts / tops may be NULL when n_bins == 0.
 * sc_probe_enable  from now on every finished tick (sc_step_finish, so also sc_tick and every tick of sc_step) appends
 *                  one row and one profile to a log of capacity_rows (1..1,048,576) rows in device memory, on the
 *                  context's stream after the force kernel: no synchronisation, no host traffic, the row index is a
 *                  device counter.  A tick that finds the log full is not recorded and a device counter of dropped ticks
 *                  goes up; memory is never overrun.  Enabling again starts an empty log with the new settings.  While
 *                  enabled, results are bit for bit what they are without it (ticks are then never fused with their
 *                  successor's wall pass: a fused tick leaves the NEXT tick's removal and wall fix in the storage arrays,
 *                  which is not the state sc_download_state stands for).
 * sc_probe_disable stops logging and discards what was not read.
 * sc_probe_read    synchronises; delivers and clears what was logged since the last read, oldest first: rows is
 *                  room x SC_PROBE_FIELDS, counts and tops room x n_bins (not touched, and may be NULL, when n_bins == 0).
 *                  *n_out rows were delivered; with less room than rows logged the rest stay for the next read (the
 *                  log's space is reused once all of it has been read).  *n_dropped is the counter of dropped ticks,
 *                  which is cleared.
 * SC_ERR_ARG for null pointers, n_bins outside 0..SC_PROBE_MAX_BINS, n_bins > 0 with bounds that are not finite or
 * x1 <= x0, capacity_rows outside 1..1,048,576, room < 0.  SC_ERR_STATE for sc_probe_now / sc_probe_read between
 * sc_step_begin and sc_step_finish, for sc_probe_read without sc_probe_enable, for sc_probe_enable / sc_probe_disable
 * inside a tick or after sc_set_next_inputs promised the next tick, and for all four on a context in slab mode
 * (sc_set_slab).  Like rendering the probe reads the state only: no counter, look-ahead promise, RNG position or pending
 * error flag changes, and its launches are not bracketed by the timing events. */
#define SC_PROBE_FIELDS 16
#define SC_PROBE_MAX_BINS 1024
int sc_probe_now(sc_ctx* ctx, int32_t n_bins, double x0, double x1, double* row16, int32_t* counts, double* tops);
int sc_probe_enable(sc_ctx* ctx, int64_t capacity_rows, int32_t n_bins, double x0, double x1);
int sc_probe_disable(sc_ctx* ctx);
int sc_probe_read(sc_ctx* ctx, double* rows, int32_t* counts, double* tops, int64_t room, int64_t* n_out,
                  int64_t* n_dropped);

/* Tracking: the state as small packed frames, and such a frame back into a context.  A frame (format 1, little-endian;
 * tests/track_spec.py is the rule, byte for byte) is
 *   a 64-byte header   "SCTK", u32 version = 1, i64 tick (ticks finished by the context, as in the probe's rows), i64 n,
 *                      i32 n_segments, i32 flags (bit 0: the pressure was valid), f64 lo = -0.25, f64 span = 1.5, zeros;
 *   n_segments x 4 f64 the walls the tick ran with (the unpadded segments of sc_set_segments / sc_tick);
 *   four planes, each zero-padded to a multiple of 8 bytes: u32 id[n], u16 qx[n], u16 qy[n], u8 c[n].
 * n counts the stored slots, as sc_count does.  A coordinate is q = floor((x - lo) * (65534 / span) + 0.5) clamped to
 * 0..65534, each operation rounded on its own in float64, and 65535 when it is not finite; back: lo + q * (span / 65534),
 * +inf for 65535 -- within half a step, 1.14445e-5, of what was stored.  c is the colour byte sc_render gives the slot
 * (255 - trunc(P * 255) clipped, 255 without a valid pressure); back: P = (255 - c + 0.5) / 255, which renders as c again.
 * Records stand in the storage order of the moment; ids are unique, and the renderer orders by id.
 *
 * sc_track_bound    the size of a frame of n particles and n_segments walls.
 * sc_track_capture  packs the state as it stands on the device and downloads the one frame; synchronises.  *n_bytes is
 *                   the frame's size; if that exceeds `room` nothing is written and SC_ERR_CAPACITY is returned (out may
 *                   be null with room 0 to ask for the size).
 * sc_track_enable   from now on every finished tick (sc_step_finish, so also sc_tick and every tick of sc_step) whose
 *                   count of finished ticks is a multiple of `every` (>= 1) appends one frame to a log of capacity_bytes
 *                   (1..2^40) in device memory, on the context's stream after the force kernel: no synchronisation, no
 *                   host traffic.  The frame's size is known on the device only; its place is taken with one atomic add
 *                   on a byte cursor that lives there.  A frame that does not fit is not written, not even in part, and a
 *                   device counter of dropped frames goes up.  Enabling again starts an empty log.  While enabled,
 *                   results are bit for bit what they are without it (ticks are then never fused with their successor's
 *                   wall pass, for the probe's reason).
 * sc_track_disable  stops logging and discards what was not read.
 * sc_track_read     synchronises; delivers what was logged since the last read, oldest first and back to back (every
 *                   frame's header gives its length), and rewinds the cursor: *n_bytes, *n_frames, and *dropped, the
 *                   counter of dropped frames, which is cleared.  With less room than bytes logged nothing is delivered
 *                   or forgotten: *n_bytes is what is needed, SC_ERR_CAPACITY is returned.
 * sc_track_load     `frame` (host memory, n_bytes) becomes the context's state: dequantised positions, zero velocities,
 *                   the ids, P from c -- with `plain` from c = 100 for every particle, the reference's colour for particles
 *                   that come without a pressure, (100, 100, 255) -- all n slots live with a valid pressure, the next
 *                   appended particle's id above the frame's largest.  The frame is checked on the host first: the magic,
 *                   the version, n >= 0, 0 <= n_segments <= SC_MAX_SEGMENTS, n_bytes equal to the size such a frame has,
 *                   a finite range, ids below 2^31 - 1 (SC_ERR_ARG), n within the context's capacity (SC_ERR_CAPACITY); a
 *                   frame that fails launches nothing and leaves the context as it was.  Synchronises.  The tick counter
 *                   and the walls of the context stay as they are: the frame's own are for the caller to read
 *                   (sand_crate_amd/track.py: parse).  The surface normals of sc_download_normals are not the frame's.
 * SC_ERR_ARG for null pointers, a negative room, every < 1 or a capacity outside 1..2^40.  SC_ERR_STATE between
 * sc_step_begin and sc_step_finish, for sc_track_read without sc_track_enable, for sc_track_enable / sc_track_disable
 * after sc_set_next_inputs promised the next tick, and for all of them but sc_track_bound on a context in slab mode
 * (sc_set_slab).  Packing reads the state only: no counter, look-ahead promise, RNG position or pending error flag
 * changes, and its launches are not bracketed by the timing events. */
int sc_track_bound(int64_t n, int32_t n_segments, int64_t* bytes);
int sc_track_capture(sc_ctx* ctx, uint8_t* out, int64_t room, int64_t* n_bytes);
int sc_track_enable(sc_ctx* ctx, int64_t every, int64_t capacity_bytes);
int sc_track_disable(sc_ctx* ctx);
int sc_track_read(sc_ctx* ctx, uint8_t* out, int64_t room, int64_t* n_bytes, int64_t* n_frames, int64_t* dropped);
int sc_track_load(sc_ctx* ctx, const uint8_t* frame, int64_t n_bytes, int32_t plain);

/* Trajectories: the state at full precision as frames in DEVICE memory of the caller (e.g. torch CUDA tensors), one row
 * per particle id: row r of a frame is the live particle whose id is id0 + r, whatever slot it is stored in, so the
 * frames of a run line up by particle without a sort (tests/trajectory_spec.py is the rule, byte for byte, on top of
 * tests/state_spec.py).  The log is
 *   dev_states    float64 frames x rows x 4, aligned to 16 bytes: (x, y, vx, vy), the very bits sc_export_state_device
 *                 delivers for that particle; the row of an id that is not live holds four quiet NaNs, each
 *                 0x7FF8000000000000.  "Live" is the export's rule -- a stored slot whose x is finite -- so a row is
 *                 present exactly when its x is finite; -0.0, infinities and NaN in y or the velocity pass unchanged.
 *   dev_pressure  float64 frames x rows, or NULL: the export's pressure (0 where the last finished tick did not leave
 *                 the slot live), the same NaN where the row is absent.
 *   dev_ticks, dev_counts, dev_outside   int64 x frames: the frame's tick (ticks finished by the context), its live
 *                 particles, and how many of them have an id outside [id0, id0 + rows): counted, not recorded.
 *   dev_words     int64 x 4: the cursor (frames written), the frames dropped because the log was full, the frame the last
 *                 reserve chose (-1: none), one spare.
 * Ids are unique in a state; nothing is said about a state where they are not.
 *
 * sc_traj_enable_device  from now on every finished tick (sc_step_finish, so also sc_tick and every tick of sc_step) whose
 *     count of finished ticks is a multiple of `every` (>= 1) writes one frame at the cursor, on the context's stream after
 *     the force kernel: three launches, no synchronisation, no host traffic, no allocation.  A tick that finds the log
 *     full (`frames` frames) writes nothing and the dropped word goes up; an abandoned tick leaves no frame and is not
 *     counted as dropped.  `reset` != 0 zeroes the words on the stream, a fresh recording; 0 continues where they stand --
 *     a log may outlive a context and go on in its successor.  The arrays stay the caller's: they must live, and not be
 *     written elsewhere, until sc_traj_disable and a synchronisation.  Enabling again replaces the log.  While enabled,
 *     results are bit for bit what they are without it (ticks are then never fused with their successor's wall pass, for
 *     the probe's reason).
 * sc_traj_capture        writes one frame of the state as it stands, between ticks: the initial state, or one just loaded.
 *     Enqueued only.  It takes its place in the log like any frame, or is dropped and counted.
 * sc_traj_disable        stops recording; the log is left as it is.
 * SC_ERR_ARG for null pointers (dev_pressure apart), misaligned states, frames < 1, rows < 1, id0 < 0,
 * id0 + rows > 2^31 - 1 or every < 1.  SC_ERR_STATE between sc_step_begin and sc_step_finish, for sc_traj_capture without
 * sc_traj_enable_device, for enabling / disabling after sc_set_next_inputs promised the next tick, and for all of them
 * on a context in slab mode (sc_set_slab); a refused call leaves the log and a recording already running as they were.
 * Recording reads the state only: no counter, look-ahead promise, RNG position or pending error flag changes, and its
 * launches are not bracketed by the timing events. */
int sc_traj_enable_device(sc_ctx* ctx, double* dev_states, double* dev_pressure /* may be NULL */, int64_t* dev_ticks,
                          int64_t* dev_counts, int64_t* dev_outside, int64_t* dev_words, int64_t frames, int64_t id0,
                          int64_t rows, int64_t every, int32_t reset);
int sc_traj_capture(sc_ctx* ctx);
int sc_traj_disable(sc_ctx* ctx);

/* The state to and from DEVICE memory of the caller (e.g. torch CUDA tensors), in particle-index order: what
 * sc_download_state / sc_upload_state move through the host, without the host.
 *
 * sc_export_state_device  writes exactly what sc_download_state would write into host memory at the same point of the
 *     stream: xy and vxy n x 2 interleaved, pressure and ids of length n, in ascending id order; slots whose x is not
 *     finite (the dead ghost copies of slab mode) are skipped; the pressure is that of the last finished tick for the slots
 *     it left live and 0 for every other (tests/state_spec.py is the rule).  *dev_n (device memory, required) receives n.
 *     Any of the four arrays may be NULL; xy and vxy are written as 16-byte records and must be aligned to 16 bytes.
 *     `room` is the room of the arrays in particles; elements past n are left as they were.  Enqueued on the context's
 *     stream only: nothing synchronises, nothing reaches the host, and the context's stream does not wait for other
 *     streams -- the arrays must not be in use elsewhere when this is called.  Like rendering it reads the state only: no
 *     counter, look-ahead promise, RNG position or pending error flag changes, and like the probe's its launches are not
 *     bracketed by the timing events.  Works in slab mode, as sc_download_state does.
 *     The ranking is a radix sort of (id, slot) pairs on the device -- least significant digit first, four passes of
 *     eight bits, each a count per tile of 256 keys, a two-level scan of the counts and a stable scatter (csrc/sc_radix.h)
 *     -- so the result is exact, does not depend on timing, no workgroup waits for another, and the cost is linear in
 *     the stored count whatever the ids are (a bitmap over the ids would cost 2^31 bits for one large id, and a slab does
 *     not know the largest id of the ghosts it was sent).  The workspace belongs to the context: 24 bytes per particle of
 *     the host's bound of the stored count (in slab mode: of the capacity), grown -- which synchronises once -- to the
 *     largest bound asked for.
 *     SC_ERR_STATE between sc_step_begin and sc_step_finish; SC_ERR_ARG for a null dev_n, a negative room or a misaligned
 *     array; SC_ERR_CAPACITY when room is below the host's bound of the stored count -- checked before anything is
 *     launched, the arrays are then untouched.
 * sc_import_state_device  sc_upload_state (dev_ids NULL: particle i gets id i) or sc_upload_state_ids with the arrays in
 *     device memory: the n particles become the context's state, pressures and normals are no longer valid, a pending
 *     promise (sc_set_next_inputs) is abandoned; the same SC_ERR_STATE and SC_ERR_CAPACITY rules.  No particle data
 *     passes through the host.  The arrays are read on the context's stream, which does not wait for other streams: they
 *     must be ready when this is called and stay untouched until the stream has passed the call.  With ids the call
 *     synchronises once, to bring back two words: the largest id and whether one lies outside 0..2^31 - 2 -- then
 *     SC_ERR_ARG, and the context is as it was.  Duplicate ids are the caller's responsibility, as in sc_upload_state_ids. */
int sc_export_state_device(sc_ctx* ctx, double* dev_xy, double* dev_vxy, double* dev_pressure, int64_t* dev_ids, int64_t room,
                           int64_t* dev_n);
int sc_import_state_device(sc_ctx* ctx, const double* dev_xy, const double* dev_vxy, const int64_t* dev_ids /* may be NULL */,
                           int64_t n);

/* Fixed-radius pair lists in DEVICE memory of the caller (e.g. torch CUDA tensors), as a CSR edge list in index order:
 * which points lie within `radius` of which.  tests/pairs_spec.py is the rule: with all arithmetic in separately rounded
 * float64, (i, j) is a pair iff i != j and fl(fl(dx dx) + fl(dy dy)) <= fl(radius radius), dx = fl(x_i - x_j); with
 * SC_PAIRS_HALF in `flags` only j > i is kept.  A point with a coordinate that is not finite has no partners and is
 * nobody's; coincident points are each other's.  No cap on a row's length, any radius whose square is a normal finite
 * float64 (about 1.5e-154 .. 1.3e154).  The result is a pure function of the points.
 *
 * sc_pairs_count_device  the points are the n rows of dev_xy (n x 2 interleaved float64, aligned to 16 bytes), or with
 *     dev_xy NULL the state: the particles exactly as sc_export_state_device would write them at the same point of the
 *     stream -- ascending id, slots whose x is not finite skipped -- so index i is the row of that export, not the id, and
 *     n is known on the device only (`n` is then ignored).  Writes dev_offsets[0 .. n], int64: the exclusive scan of the
 *     row lengths, so dev_offsets[n] = E, the number of pairs, which may exceed 2^32; entries past n are left as they
 *     were.  dev_counts[0] = n, dev_counts[1] = E.  `room_rows` is the room of dev_offsets in rows (it holds room_rows + 1
 *     entries) and must be at least the host's bound of the point count: n, or for the state the bound
 *     sc_export_state_device uses.  The domain: every finite coordinate c needs fl(|c| / radius) < 2^31.  A point outside
 *     is found on the device: dev_counts[1] = -1 then, dev_counts[0] = n, and nothing else is written, here or by the fill
 *     -- no host round trip.  The grid of the search stays in the context's workspace for sc_pairs_fill_device.
 * sc_pairs_fill_device   row i's partners go to dev_partners[dev_offsets[i] ...], int64 and ascending in j, and -- unless
 *     dev_d2 is NULL -- each pair's squared distance next to it: the very number that was compared, no square root.  An
 *     entry e is written only when e < room_pairs: a list longer than the room is clipped there, nothing is written past
 *     the room.  Reads the workspace of the last count of this context, not the caller's points or offsets.
 *     SC_ERR_STATE when there is no such count, or when a tick, an upload, an append, an emission, an import or a track
 *     load has touched the state since (whichever form the count had).
 * Both enqueue on the context's stream only: nothing synchronises, nothing reaches the host, and the context's stream does
 * not wait for other streams -- the arrays must be ready, and not in use elsewhere, when the calls are made.  Like the
 * export they read the state only: no counter, look-ahead promise, RNG position, pending error flag or particle array
 * changes, and their launches are not bracketed by the timing events.
 *     The search bins the points into cells a little larger than the radius -- h = radius (1 + 2^-20), so that the
 * rounding of x / h cannot separate a pair by more than one cell (csrc/sc_pairs.h has the argument) -- in a hashed table of
 * at least two buckets per point, with a stable radix sort of (bucket, index) pairs, counts each row's partners in the
 * nine cells around its point, scans the counts in 64 bits on two levels, and fills each row by merging its nine runs.
 * No workgroup waits for another, no floating-point atomics, and no atomic's order reaches the output.  The workspace
 * belongs to the context: about 100 bytes per point of the host's bound, grown -- which synchronises once -- to the largest
 * bound asked for.
 *     SC_ERR_STATE between sc_step_begin and sc_step_finish, and for the state form on a context in slab mode
 * (sc_set_slab: partners across a cut live on another rank).  SC_ERR_ARG for a null context, null dev_offsets, dev_counts
 * or (with room) dev_partners, a misaligned dev_xy, a negative n or room, unknown flags, or a radius outside the range
 * above.  SC_ERR_CAPACITY when room_rows is below the host's bound, or for more than 2^28 points -- checked before
 * anything is launched, the arrays are then untouched. */
enum { SC_PAIRS_HALF = 1 };
int sc_pairs_count_device(sc_ctx* ctx, const double* dev_xy /* NULL: the state */, int64_t n, double radius, int32_t flags,
                          int64_t* dev_offsets, int64_t room_rows, int64_t* dev_counts /* [2]: n, E */);
int sc_pairs_fill_device(sc_ctx* ctx, int64_t* dev_partners, double* dev_d2 /* may be NULL */, int64_t room_pairs);

/* Batched point clouds: many disjoint clouds -- the frames of a minibatch -- in one count, one grid and one launch of every
 * reader.  dev_ptr holds clouds + 1 ascending int64 offsets in DEVICE memory, ptr[0] = 0 and ptr[clouds] = n; cloud b is the
 * rows ptr[b] .. ptr[b + 1] of the points and may be empty.  j is a partner of row i iff both lie in one cloud and the
 * rule of the call accepts them: indices stay global, the orders are the orders of the unbatched calls, and every result
 * equals, bit for bit, the per-cloud results concatenated with the partner indices shifted by ptr[b] (tests/batch_spec.py).
 * The clouds may overlap in space completely: they share the one grid, the cloud is mixed into the bucket hash, and a
 * candidate counts only when its index lies in the row's [ptr[b], ptr[b + 1]) -- the hash is for speed, the range for
 * exactness (csrc/sc_pairs.h).
 *
 * sc_pairs_set_batch_device  applies to the NEXT sc_pairs_count_device of this context and is consumed by it, whatever
 *     that call returns; the count must have the caller's points (dev_xy NULL with a batch pending: SC_ERR_ARG).  The
 *     count copies dev_ptr into the workspace on the context's stream -- it must be ready then, as the points must --
 *     and the readers never read it again.  clouds = 0 or dev_ptr NULL clears a pending batch.  The grid the count
 *     leaves is batched, which the context knows on the host: sc_pairs_fill_device, sc_pairs_nearest_device,
 *     sc_pairs_sum_device and sc_pairs_sum_grad_device read it as such.  sc_pairs_label_device, sc_pairs_hist_device,
 *     sc_pairs_rays_device and sc_pairs_ray_paths_device do NOT read a batched grid: on one they return SC_ERR_ARG and
 *     write nothing.  Their batched forms have outputs of other shapes and are calls of their own, at the end of this
 *     header: sc_pairs_label_batch_device, sc_pairs_hist_batch_device, sc_pairs_rays_batch_device and
 *     sc_pairs_ray_paths_batch_device, which in turn return SC_ERR_ARG on an unbatched grid.
 * sc_pairs_set_query_batch_device  with queries a second array, dev_query_ptr, also clouds + 1 entries ending at
 *     n_queries: query rows query_ptr[b] .. query_ptr[b + 1] see the points of cloud b only; a cloud may have points and
 *     no queries, or queries and no points (rows without partners).  Applies to the next query-form reader of the batched
 *     grid and is consumed by it; it is read by that reader's launches only.  SC_ERR_ARG when the last count left no
 *     batched grid; a query-form reader on a batched grid without it returns SC_ERR_ARG; NULL clears.
 * Offsets that do not start at 0, that descend, or that do not end at n (n_queries) are found on the device, no host
 * round trip: dev_counts[1] = -3 -- next to -1, the domain, and -2, short arrays -- and nothing else is written, by the
 * count, the fill or any reader.  SC_ERR_ARG for a null context or negative clouds, SC_ERR_CAPACITY for more than 2^28. */
int sc_pairs_set_batch_device(sc_ctx* ctx, const int64_t* dev_ptr, int64_t clouds);
int sc_pairs_set_query_batch_device(sc_ctx* ctx, const int64_t* dev_query_ptr);

/* The clusters of that graph in DEVICE memory of the caller: what hangs together.  tests/cluster_spec.py is the rule: a
 * cluster is a connected component of the graph above -- i ~ j iff (i, j) is a pair of the full list, whether or not the
 * count had SC_PAIRS_HALF -- over the points whose coordinates are all finite; a point with a coordinate that is not finite
 * is in no cluster and bridges none.  Clusters are numbered 0 .. C-1 in ascending order of their smallest member index:
 * dev_roots[c] is that member, dev_sizes[c] the member count, dev_labels[i] the cluster of point i, or -1 for a point in
 * none.  The result is a pure function of the points.
 *
 * sc_pairs_label_device  labels the points of the last sc_pairs_count_device of this context, in either form and with any
 *     flags: it reads the grid that count left in the workspace, not the caller's points.  Writes dev_labels[0 .. n-1]
 *     (int64), always whole; dev_sizes[c] and dev_roots[c] (int64, either may be NULL) for c < min(C, room_clusters) only:
 *     entries from the room on are left as they were; dev_counts[0] = n, dev_counts[1] = C.  `room_rows`, the room of
 *     dev_labels, must be at least the bound the count was sized by.  After a count that found a point outside the domain
 *     dev_counts[1] = -1 is written and nothing else.  The workspace of the count is left as it is: sc_pairs_fill_device
 *     may follow, and the labelling may be repeated.
 * It enqueues on the context's stream only, with the rules of the two calls above: nothing synchronises, nothing reaches
 * the host, no counter, look-ahead promise, RNG position, pending error flag or particle array changes, and the launches
 * are not bracketed by the timing events.
 *     The algorithm: every point starts as a set of its own (parent[i] = i); a thread per row walks its nine cells as the
 * count does and unites its set with that of every partner j < i -- finds with path halving, the larger root hooked under
 * the smaller by a compare-and-swap, so parent[x] <= x throughout and a set's root is its smallest member in whatever order
 * the atomics land; ceil(log2(max(m, 2))) launches of pointer jumping, m the bound, then leave every parent at its root;
 * an exclusive scan of "is a root" numbers the clusters; one more pass writes labels, roots and (integer atomics) sizes.
 * No workgroup waits for another and no atomic's order reaches the output (csrc/sc_clusters.h).  The workspace belongs to
 * the context: about 16 bytes per point of the bound, grown -- which synchronises once -- to the largest bound asked for.
 *     SC_ERR_ARG for a null context, null dev_labels or dev_counts, or a negative room.  SC_ERR_STATE between
 * sc_step_begin and sc_step_finish, when there is no count, and when a tick, an upload, an append, an emission, an import
 * or a track load has touched the state since (the fill's rule).  SC_ERR_CAPACITY when room_rows is below the count's
 * bound.  All checked before anything is launched: the arrays are then untouched. */
int sc_pairs_label_device(sc_ctx* ctx, int64_t* dev_labels, int64_t room_rows, int64_t* dev_sizes /* may be NULL */,
                          int64_t* dev_roots /* may be NULL */, int64_t room_clusters, int64_t* dev_counts /* [2]: n, C */);

/* What each cluster carries, in DEVICE memory of the caller: per cluster of the last label the sum, and optionally the
 * minimum and the maximum, of up to SC_CLUSTER_SUMS_MAX_CHANNELS float64 channels over the cluster's members.
 * tests/cluster_sums_spec.py is the rule: the members of cluster c are the rows i with label c in ascending i; the sum of a
 * channel is `tree` of their values in that order -- pairwise summation in groups of 64, and groups of groups, each add
 * rounded on its own, the padding +0.0, a single member still through one group (so a cluster of -0.0 sums to +0.0);
 * minima and maxima are NumPy's: a NaN on either side is the result.  A row with label -1 is never read into any result,
 * whatever its values hold.  The result of a cluster is a pure function of its own members' values: the same bits on every
 * call, whatever the other clusters, the capacity, the bucket count or the count's flags are.
 *
 * sc_pairs_cluster_sums_device  reads what the last sc_pairs_label_device of this context left in its workspace, and n and
 *     the domain flag of the count it labelled; of the caller's it reads dev_values (values_rows x channels contiguous
 *     float64, aligned to 16 bytes; row i belongs to point i of the count), nothing else.  Writes dev_sums[c, :] and -- unless
 *     NULL -- dev_mins[c, :] and dev_maxs[c, :] (float64, room_clusters x channels contiguous) for c < min(C,
 *     room_clusters) only: rows from the room on are left as they were; dev_counts[0] = n, dev_counts[1] = C.  After a
 *     count that found a point outside the domain dev_counts[1] = -1 is written and nothing else; with values_rows < n --
 *     only the device knows n in the state form -- dev_counts[1] = -2 and nothing else: a flag of this call's own, the
 *     count's verdict stays as the count left it.  Nothing of the count's or the label's workspace is written: a fill, a
 *     table, a sum, a histogram or another label may follow, and the call may be repeated.
 * It enqueues on the context's stream only, with the rules of the calls above: nothing synchronises, nothing reaches the
 * host, no counter, look-ahead promise, RNG position, pending error flag or particle array changes, and the launches are
 * not bracketed by the timing events.
 *     The algorithm: a stable radix sort of (label, index), a dead row's key behind every cluster, brings every cluster's
 * members together in ascending index; exclusive scans of the sizes and of ceil(size / 64) give the member and chunk
 * starts; level 0 takes a wave per chunk of 64 consecutive members of ONE cluster, counted from the cluster's start, gathers
 * values[index] rows and reduces them by the wave's xor butterfly, which is the rule's group of 64; a cluster of one chunk
 * has its result, larger ones leave a partial per chunk, and ceil(log64(m)) - 1 more levels reduce those the same way, m
 * the bound.  The number of launches depends on m alone.  No workgroup waits for another and there are no atomics at all
 * (csrc/sc_cluster_sums.h).  The workspace belongs to the context: under 60 bytes per point of the bound, grown -- which
 * synchronises once -- to the largest bound asked for.
 *     SC_ERR_ARG for a null context, null dev_counts or dev_values, null dev_sums with room, channels outside 1 ..
 * SC_CLUSTER_SUMS_MAX_CHANNELS, values that are not aligned to 16 bytes, or a negative room or number of rows.  SC_ERR_STATE
 * between sc_step_begin and sc_step_finish, when there is no label, when an sc_pairs_count_device has run since the label
 * (in either form, batched or not: a batched grid has no label), and when anything has touched the state since (the fill's
 * rule).  All checked before anything is launched: the arrays are then untouched. */
enum { SC_CLUSTER_SUMS_MAX_CHANNELS = 8 };
int sc_pairs_cluster_sums_device(sc_ctx* ctx, const double* dev_values, int64_t values_rows,
                                 int32_t channels /* 1 .. SC_CLUSTER_SUMS_MAX_CHANNELS */, double* dev_sums,
                                 double* dev_mins /* may be NULL */, double* dev_maxs /* may be NULL */, int64_t room_clusters,
                                 int64_t* dev_counts /* [2]: n, C or a status */);

/* Nearest-k neighbour tables of that graph in DEVICE memory of the caller: a table of fixed shape, rows x k, for code that
 * wants neighbors[i, 0 .. k) rather than a CSR list of data-dependent length.  tests/nearest_spec.py is the rule: j is a
 * partner of row r iff fl(fl(dx dx) + fl(dy dy)) <= fl(radius radius), dx = fl(x_r - x_j) -- the arithmetic of the pair list
 * -- and, in the self form only, j != r; row r of the table holds its partners in ascending order of the key (d2, j) -- d2
 * the float64 that was compared, bit-equal d2 ordered by the smaller j --, the first min(k, partners) of them; the places
 * behind hold -1, and +inf in dev_d2.  A point with a coordinate that is not finite is nobody's partner, a row whose own
 * point or query is not finite is empty.  The result is a pure function of the points and the queries.
 *
 * sc_pairs_nearest_device  searches the grid of the last sc_pairs_count_device of this context, in either form and with any
 *     flags (SC_PAIRS_HALF is ignored: the table is cut from the full list): it reads the workspace that count left, never
 *     the count's caller's points, and leaves it as it is -- sc_pairs_fill_device, sc_pairs_label_device and further tables
 *     may follow.  The rows: with dev_queries NULL the count's n points themselves (the self form; n is known on the
 *     device only for the state form), else the n_queries rows of dev_queries (n_queries x 2 interleaved float64, aligned
 *     to 16 bytes), which need not be points: a query that coincides with a point has it as a partner at d2 = 0.  Writes,
 *     for every row below the row count, all k places of dev_neighbors (int64, rows x k contiguous) and -- unless NULL --
 *     of dev_d2 (float64, the same shape) and dev_partners[row] (int64), the number of partners without the cap: in the
 *     self form the row length of the full pair list.  Rows from the row count on are left as they were.  `room_rows`,
 *     the room of the three arrays in rows, must be at least the bound the count was sized by (self form) or n_queries.
 *     dev_counts[0] = the row count, dev_counts[1] = the number of rows with more partners than k: 0 means that the table
 *     is the whole pair list.  The domain of the queries is that of the points, fl(|c| / radius) < 2^31 for every finite
 *     coordinate; after a count that found a point outside it, or with a query outside it, dev_counts[1] = -1 is written
 *     and nothing else.  A query outside raises a flag of this call's own: the count's verdict, which the fill and the
 *     label read, stays as the count left it.
 * It enqueues on the context's stream only, with the rules of the calls above: nothing synchronises, nothing reaches the
 * host, no counter, look-ahead promise, RNG position, pending error flag or particle array changes, and the launches are
 * not bracketed by the timing events.
 *     The algorithm: a thread per row walks the buckets of its nine cells as the count does and keeps its k best so far as
 * a sorted list in LDS, slot-major, inserting by (d2, j) -- candidates arrive in bucket order, which is not the key's --,
 * with the key of the last place in registers, so that a full list rejects most candidates with one compare.  A
 * workgroup is one wave of 64 rows with LDS for 16, 32 or 64 places per row, whichever holds k (12, 24, 49 KiB).  It writes
 * its block of rows together, consecutive lanes to consecutive entries (csrc/sc_nearest.h).  One integer atomic per cut row: no
 * atomic's order reaches the output, and no workgroup waits for another.
 *     SC_ERR_ARG for a null context, null dev_neighbors or dev_counts, k outside 1 .. SC_NEAREST_MAX_K, a negative
 * n_queries or room, or misaligned queries.  SC_ERR_STATE between sc_step_begin and sc_step_finish, when there is no
 * count, and when a tick, an upload, an append, an emission, an import or a track load has touched the state since (the
 * fill's rule).  SC_ERR_CAPACITY when room_rows is too small, or for more than 2^28 queries.  All checked before anything
 * is launched: the arrays are then untouched. */
enum { SC_NEAREST_MAX_K = 64 };
int sc_pairs_nearest_device(sc_ctx* ctx, const double* dev_queries /* NULL: the points themselves */, int64_t n_queries,
                            int32_t k, int64_t* dev_neighbors /* rows x k */, double* dev_d2 /* rows x k, may be NULL */,
                            int64_t* dev_partners /* rows, may be NULL */, int64_t room_rows,
                            int64_t* dev_counts /* [2]: rows, cut */);

/* Weighted neighbourhood sums over that graph in DEVICE memory of the caller: what is there, not who -- the density at a
 * particle or a probe, a smoothed velocity, a raster of a field, the "sum over neighbours" of a message-passing layer.
 * tests/field_spec.py is the rule: j is a partner of row r iff fl(fl(dx dx) + fl(dy dy)) <= fl(radius radius), dx =
 * fl(x_r - x_j) -- the arithmetic of the pair list -- and, in the self form without SC_FIELDS_SELF only, j != r; with
 * t = fl(1 - fl(d2 / r2)), r2 = fl(radius radius), the weight w is 1, t, fl(t t) or fl(fl(t t) t) for `power` 0, 1, 2, 3
 * (3 is the poly6 shape; 0 <= t <= 1 for a partner), and
 *     dev_wsum[r]    = ((0 + w_j1) + w_j2) + ...
 *     dev_sums[r, c] = ((0 + fl(w_j1 v[j1, c])) + fl(w_j2 v[j2, c])) + ...
 * over the partners in ASCENDING j, from +0.0, every product and every sum rounded on its own.  A point with a coordinate
 * that is not finite is nobody's partner; a row whose own point or query is not finite gets 0 everywhere.  The values are
 * taken as they are: a NaN or an infinity propagates by IEEE rules, 0 * inf at d2 == r2 is NaN.  The result is a pure
 * function of the points, the queries and the values: two calls give the same bits.
 *
 * sc_pairs_sum_device  sums over the grid of the last sc_pairs_count_device of this context, in either form and with any
 *     flags (SC_PAIRS_HALF is ignored: the sums run over the full list): it reads the workspace that count left, never the
 *     count's caller's points, and leaves it as it is -- fills, labels, tables and further sums may follow.  The rows: with
 *     dev_queries NULL the count's n points themselves (the self form; with SC_FIELDS_SELF point r is its own partner at
 *     d2 = 0, in its place in index order), else the n_queries rows of dev_queries (n_queries x 2 interleaved float64,
 *     aligned to 16 bytes; SC_FIELDS_SELF has no meaning and is ignored), which need not be points.  dev_values is
 *     values_rows x channels contiguous float64, row j the values of point j of the count; channels is 0 ..
 *     SC_FIELDS_MAX_CHANNELS, with 0 dev_values, values_rows and dev_sums are not looked at and only dev_wsum is written.
 *     Writes dev_sums (rows x channels contiguous) and -- unless NULL -- dev_wsum for every row below the row count; rows
 *     from the row count on are left as they were.  `room_rows`, the room of the two arrays in rows, must be at least
 *     the bound the count was sized by (self form) or n_queries.  dev_counts[0] = the row count, dev_counts[1] = the
 *     status: 0 when all is well; -1 after a count that found a point outside the domain fl(|c| / radius) < 2^31, or with
 *     a query outside it; -2 when values_rows is below the count's n, which for the state form is known on the device
 *     only.  With a status below 0 only dev_counts[1] is written, and no row of dev_values at or beyond values_rows is ever
 *     read.  The status comes from a flag of this call's own: the count's verdict, which the fill and the label read, stays
 *     as the count left it.
 * It enqueues on the context's stream only, with the rules of the calls above: nothing synchronises, nothing reaches the
 * host, no counter, look-ahead promise, RNG position, pending error flag or particle array changes, and the launches are
 * not bracketed by the timing events.
 *     The algorithm: a check pass over the queries and the values' rows, then a thread per row merges the nine runs of its
 * nine cells, each ascending in j, by always taking the smallest head -- the merge of sc_pairs_fill_device, cursors in LDS
 * -- and instead of storing the partner adds to the weight sum and to the channel sums in registers, reading values[j, :]
 * where it lies.  Four kernels, for 1, 2, 4 and 8 channels; a call with 3 runs the one for 4.  Nothing of the list's size
 * is written and there is no workspace beyond the flag.  No floating-point atomics, no atomic's order reaches the output,
 * no workgroup waits for another (csrc/sc_fields.h).  scripts/fields_time.py measures it on an MI355X against the list
 * route -- sc_pairs_fill_device with distances, then torch's gather, multiply and index_add_ --:
 * profiles/fields_time.txt has the times.
 *     SC_ERR_ARG for a null context, null dev_counts, dev_sums and dev_wsum both NULL, channels outside 0 ..
 * SC_FIELDS_MAX_CHANNELS, channels > 0 with dev_values or dev_sums NULL, power outside 0 .. 3, unknown flags, a negative
 * n_queries, values_rows or room, or misaligned queries.  SC_ERR_STATE between sc_step_begin and sc_step_finish, when
 * there is no count, and when a tick, an upload, an append, an emission, an import or a track load has touched the state
 * since (the fill's rule).  SC_ERR_CAPACITY when room_rows is too small, or for more than 2^28 queries.  All checked
 * before anything is launched: the arrays are then untouched. */
enum { SC_FIELDS_MAX_CHANNELS = 8, SC_FIELDS_SELF = 1 };
int sc_pairs_sum_device(sc_ctx* ctx, const double* dev_queries /* NULL: the points themselves */, int64_t n_queries,
                        const double* dev_values /* points x channels, may be NULL with channels 0 */, int64_t values_rows,
                        int32_t channels, int32_t power, int32_t flags, double* dev_sums /* rows x channels */,
                        double* dev_wsum /* rows, may be NULL */, int64_t room_rows,
                        int64_t* dev_counts /* [2]: rows, status */);

/* The gradient of those sums with respect to POSITIONS, in DEVICE memory of the caller: what torch's autograd needs to
 * differentiate sc_pairs_sum_device through the coordinates of the points or of the queries (`Crate.field_function`).
 * The gradient with respect to the values needs no call of its own: the weight depends on d2 only and d2 is bitwise
 * symmetric, so it is sc_pairs_sum_device with rows and partners swapped.  tests/field_grad_spec.py (`position_grad`) is
 * the rule: j is a partner of row r iff fl(fl(dx dx) + fl(dy dy)) <= fl(radius radius), dx = fl(x_r - x_j), and in the
 * self form j != r always (d2_rr is identically 0; SC_FIELDS_SELF plays no part); with t = fl(1 - fl(d2 / r2)) and
 * m = 1, t, fl(t t) for `power` 1, 2, 3,
 *     s           = ((((0 + row_s[r]) + part_s[j]) + fl(row_a[r, 0] part_b[j, 0])) + fl(row_a[r, 1] part_b[j, 1])) + ...
 *     ax          = ((0 + fl(fl(s m) dx_j1)) + fl(fl(s m) dx_j2)) + ...          ay likewise with dy
 *     dev_grad[r] = (fl(k ax), fl(k ay)),  k = fl(-(2 power) / r2)
 * over the partners in ASCENDING j, from +0.0, every product and every sum rounded on its own; an absent row_s or part_s
 * adds nothing.  With `power` 0 the weights are constant: every row gets +0.0.  A point with a coordinate that is not
 * finite is nobody's partner; a row whose own point or query is not finite gets fl(k 0).  The arrays are taken as they
 * are: a NaN or an infinity propagates by IEEE rules.  A pure function of its inputs: two calls give the same bits.
 *     The three uses, with G and gw the upstream gradients of dev_sums and dev_wsum and V the values: the self form with
 * respect to the points has row_a = [G | V], part_b = [V | G] (twice the channels: s = G_r V_j + V_r G_j) and row_s =
 * part_s = gw; the query form with respect to the queries has row_a = G, part_b = V, row_s = gw over a count of the
 * points; the query form with respect to the points has the POINTS as dev_queries over a count of the queries, row_a = V,
 * part_b = G, part_s = gw.  More than SC_FIELDS_MAX_CHANNELS channels go in groups, the scalars with the first, and the
 * results are added in ascending group order.
 *
 * sc_pairs_sum_grad_device  runs over the grid of the last sc_pairs_count_device of this context, as sc_pairs_sum_device
 *     does, and leaves the workspace as it is.  The rows: with dev_queries NULL the count's n points themselves, else
 *     the n_queries rows of dev_queries (n_queries x 2 interleaved float64, aligned to 16 bytes).  dev_row_a is row_a_rows
 *     x channels and dev_part_b part_b_rows x channels contiguous float64; channels is 0 .. SC_FIELDS_MAX_CHANNELS, with 0
 *     neither is looked at.  dev_row_s (row_a_rows entries) and dev_part_s (part_b_rows entries) may each be NULL.
 *     Writes dev_grad (rows x 2 interleaved, aligned to 16 bytes) for every row below the row count; rows from the row
 *     count on are left as they were.  `room_rows`, the room of dev_grad in rows, must be at least the bound the count was
 *     sized by (self form) or n_queries.  dev_counts[0] = the row count, dev_counts[1] = the status: 0 when all is well;
 *     -1 after a count that found a point outside the domain, or with a query outside it; -2 when row_a_rows is below the
 *     row count and dev_row_a (with channels > 0) or dev_row_s is given, or part_b_rows is below the count's n and
 *     dev_part_b (with channels > 0) or dev_part_s is given.  With a status below 0 only dev_counts[1] is written, and no
 *     row of an array at or beyond its stated length is ever read.  The status comes from a flag of this call's own.
 * It enqueues on the context's stream only, with the rules of sc_pairs_sum_device.
 *     The algorithm: a check pass, then a thread per row walks the merge of sc_pairs_sum_device with its own row_a[r, :]
 * and row_s[r] in registers, gathers part_b[j, :] and part_s[j] where they lie, keeps two sums and writes one 16-byte
 * record.  Four kernels, for 1, 2, 4 and 8 channels.  No floating-point atomics, no atomic's order reaches the output,
 * no workgroup waits for another, nothing of the list's size is written (csrc/sc_fields_grad.h).
 * scripts/field_grad_time.py measures it on an MI355X against torch's autograd of the list route:
 * profiles/field_grad_time.txt has the times.
 *     SC_ERR_ARG for a null context, null dev_counts or dev_grad, channels outside 0 .. SC_FIELDS_MAX_CHANNELS, channels
 * > 0 with dev_row_a or dev_part_b NULL, power outside 0 .. 3, a negative n_queries, row count or room, or misaligned
 * queries or gradient.  SC_ERR_STATE and SC_ERR_CAPACITY as for sc_pairs_sum_device.  All checked before anything is
 * launched: the arrays are then untouched. */
int sc_pairs_sum_grad_device(sc_ctx* ctx, const double* dev_queries /* NULL: the points themselves */, int64_t n_queries,
                             const double* dev_row_a /* rows x channels */, int64_t row_a_rows,
                             const double* dev_part_b /* points x channels */, int64_t part_b_rows,
                             int32_t channels /* 0 .. SC_FIELDS_MAX_CHANNELS */,
                             const double* dev_row_s /* rows, may be NULL */,
                             const double* dev_part_s /* points, may be NULL */, int32_t power,
                             double* dev_grad /* rows x 2 */, int64_t room_rows,
                             int64_t* dev_counts /* [2]: rows, status */);

/* Distance histograms over that graph in DEVICE memory of the caller: how far apart -- per row a table of shell counts,
 * how many partners lie in each distance band (the radial descriptors of a learned simulator), and the same counts summed
 * over the rows (the numerator of the radial distribution function g(r)).  tests/hist_spec.py is the rule: edges2[0 ..
 * bins] are the SQUARED edges, e2[k] = fl(edge_k edge_k), computed once by the caller in float64, strictly ascending,
 * e2[0] >= 0; j is a partner of row r iff d2 = fl(fl(dx dx) + fl(dy dy)) <= e2[bins], dx = fl(x_r - x_j) -- the
 * arithmetic of the pair list -- and, in the self form, j != r (there is no flag for the point itself: its distance to
 * itself is not a distance); a partner is in bin b iff e2[b] <= d2 < e2[b + 1], the last bin closed on top, d2 <=
 * e2[bins]; a partner with d2 < e2[0] is in no bin; coincident distinct points have d2 = 0 and are in bin 0 iff e2[0] is
 * 0.  A point with a coordinate that is not finite is nobody's partner; a row whose own point or query is not finite is
 * all zero.  table[r, b] is the number of partners of row r in bin b, total[b] the sum of table[r, b] over the rows below
 * the row count: in the self form it counts ordered pairs, each unordered pair twice.  No square root is taken anywhere,
 * and the result is a pure function of the points, the queries and the edges.
 *
 * sc_pairs_hist_device  counts over the grid of the last sc_pairs_count_device of this context, in either form and with
 *     any flags (SC_PAIRS_HALF is ignored): it reads the workspace that count left, never the count's caller's points,
 *     and leaves it as it is -- fills, labels, tables, sums and further histograms may follow.  edges2 is HOST memory,
 *     bins + 1 entries, read before the call returns; edges2[bins] may be at most the count's fl(radius radius), so that
 *     one count serves several histograms: partners beyond the last edge are in no bin.  The rows: with dev_queries NULL
 *     the count's n points themselves, else the n_queries rows of dev_queries (n_queries x 2 interleaved float64,
 *     aligned to 16 bytes), which need not be points.  Writes -- unless NULL -- dev_table (int32, rows x bins contiguous)
 *     for every row below the row count, rows from the row count on are left as they were, and dev_total (int64, bins
 *     entries).  `room_rows`, the room of dev_table in rows, must be at least the bound the count was sized by (self form)
 *     or n_queries; without a table it is not looked at beyond its sign.  dev_counts[0] = the row count, dev_counts[1] =
 *     the status: 0 when all is well; -1 after a count that found a point outside the domain fl(|c| / radius) < 2^31 (the
 *     count's radius), or with a query outside it.  With a status below 0 only dev_counts[1] is written -- neither the
 *     table nor the totals.  The status comes from a flag of this call's own: the count's verdict, which the fill and the
 *     label read, stays as the count left it.
 * It enqueues on the context's stream only, with the rules of sc_pairs_sum_device: nothing synchronises, nothing reaches
 * the host, no counter, look-ahead promise, RNG position, pending error flag or particle array changes, and the launches
 * are not bracketed by the timing events.
 *     The algorithm: a check pass over the queries, then a thread per row walks the buckets of its nine cells as the
 * count does -- a histogram is integer counts, the order in which a row's partners are met cannot reach it, so there is
 * no merge --, places every accepted d2 by a binary search over the squared edges in LDS (exact compares) and adds one
 * to its own int32 counter in LDS, slot-major.  A workgroup is one wave of 64 rows; three kernels, with a search of 4, 5 or 6
 * steps for up to 16, 32 or 64 bins, each with 64 lines of counters in LDS (17 KiB: the LDS holds the occupancy at nine
 * waves on a CU, where the walk was measured fastest).  It writes its block of rows of the table together, consecutive lanes to consecutive
 * entries, sums its columns over its rows in 64 bits and adds them with one 64-bit integer atomic per non-zero bin to a
 * context-owned accumulator, which a last small launch copies to dev_total when the status is 0 (csrc/sc_hist.h).  Only
 * integer atomics: no atomic's order reaches the output, and no workgroup waits for another.  Nothing of the list's size
 * is written.  scripts/hist_time.py measures it on an MI355X against the list route -- sc_pairs_fill_device with
 * distances, then torch's bucketize and bincount --: profiles/hist_time.txt has the times.
 *     SC_ERR_ARG for a null context, null dev_counts, dev_table and dev_total both NULL, bins outside 1 ..
 * SC_HIST_MAX_BINS, a null or not strictly ascending edges2, a negative or non-finite edges2[0], edges2[bins] above the
 * count's squared radius, a negative n_queries or room, or misaligned queries.  SC_ERR_STATE and SC_ERR_CAPACITY as for
 * sc_pairs_sum_device.  All checked before anything is launched: the arrays are then untouched. */
enum { SC_HIST_MAX_BINS = 64 };
int sc_pairs_hist_device(sc_ctx* ctx, const double* dev_queries /* NULL: the points themselves */, int64_t n_queries,
                         const double* edges2 /* HOST, bins + 1 */, int32_t bins,
                         int32_t* dev_table /* rows x bins, may be NULL */, int64_t* dev_total /* bins, may be NULL */,
                         int64_t room_rows, int64_t* dev_counts /* [2]: rows, status */);

/* Ray sensors over the points of that grid and a list of wall segments, in DEVICE memory of the caller: what a sensor
 * sees along a line -- a range finder on a stirring body, the height of the free surface under a probe, the particle
 * under the cursor.  tests/ray_spec.py is the rule, by brute force: ray r has the origin o = dev_origins[r] and the
 * direction d = dev_directions[r], which nobody normalises -- the parameter t is in units of |d|, the distance for a unit
 * direction.  Every point with finite coordinates carries a disc of radius disc_radius, rho2 = fl(rho rho).  With
 * f = o - c: a = fl(fl(dx dx) + fl(dy dy)), b = fl(fl(fx dx) + fl(fy dy)), cc = fl(fl(fl(fx fx) + fl(fy fy)) - rho2);
 * cc <= 0 (the origin inside or on the disc): t = +0; else b >= 0: no hit; else disc = fl(fl(b b) - fl(a cc)) < 0: no
 * hit; else t = fl(cc / fl(-b + sqrt(disc))), a form without cancellation; a hit iff t <= max_t.  Wall s from A to B,
 * e = B - A, g = A - o: den = fl(fl(dx ey) - fl(dy ex)), 0: no hit (parallel and collinear rays miss);
 * t = fl(fl(fl(gx ey) - fl(gy ex)) / den), u = fl(fl(fl(gx dy) - fl(gy dx)) / den); a hit iff 0 <= t <= max_t and
 * 0 <= u <= 1, from either face -- a sensor, not the physics' one-sided crossing test --, a t of -0 reported as +0.
 * The result of a ray is the hit with the smallest key (t, kind, index), walls before discs: dev_hit[r] = j >= 0 for
 * the disc of point j of the count, -2 - s for wall s, -1 for none, with dev_t[r] = +inf.  A ray whose origin or
 * direction is not finite, or whose a is 0, is dead: t = NaN, hit = -1.  The result is a pure function of the points,
 * the walls, the rays, disc_radius and max_t: the same on every call and for every capacity.
 *
 * sc_pairs_rays_device  sends n_rays rays through the grid of the last sc_pairs_count_device of this context, unbatched,
 *     with any flags: it reads the workspace that count left and leaves it as it is -- fills, labels, tables, sums,
 *     histograms and further rays may follow.  dev_origins and dev_directions are n_rays x 2 interleaved float64,
 *     aligned to 16 bytes.  disc_radius must be at most HALF the count's radius (count at twice the disc radius: the
 *     cell is then one disc diameter wide and a ray that advances a cell width per step meets, in the 3 x 3 cells round
 *     the step's midpoint, every disc it can touch); 0 skips the discs: walls only.  max_t is finite and not negative.
 *     `segments` is HOST memory, n_segments x 2 x 2 (A.x, A.y, B.x, B.y), read before the call returns, at most
 *     SC_MAX_SEGMENTS; NULL with 0.  Writes dev_t (float64) and dev_hit (int64) for every ray, rows from n_rays on are
 *     left as they were; `room_rows`, their room in rows, must be at least n_rays.  dev_counts[0] = n_rays,
 *     dev_counts[1] = the status: 0 when all is well; -1 after a count that found a point outside the domain
 *     fl(|c| / radius) < 2^31 (the count's radius), or with an origin outside it, or -- when discs are looked for -- a
 *     live ray's end point fl(o + fl(max_t d)) outside it or not finite; -4 when a live ray would have to walk more
 *     than 8192 cells: with dt = fl(radius / sqrt(a)) and t_end = min(max_t, the ray's nearest wall hit) it needs
 *     fl(8192 dt) > t_end -- in a closed crate every ray ends at a wall, in an open scene shorten max_t.  With a status
 *     below 0 only dev_counts[1] is written.
 * It enqueues on the context's stream only, with the rules of sc_pairs_sum_device: nothing synchronises, nothing reaches
 * the host, no counter, look-ahead promise, RNG position, pending error flag or particle array changes, and the launches
 * are not bracketed by the timing events.
 *     The algorithm: the readers' check pass over the origins, a pass over the rays for the end points and the range,
 *     then the walls -- passed by value -- and the walk: step k covers t in [fl(k dt), fl((k + 1) dt)] and tests the
 *     members of the nine cells round its midpoint by the rule above, keeping the smallest key, so the order in which
 *     candidates are met cannot reach the output; the nearest wall caps the walk, which ends after the first step with
 *     best t < fl((k + 1) dt) (csrc/sc_rays.h has the argument and its rounding margin).  A wave per ray: the lanes
 *     take the (step, cell) pairs of seven steps at a time and the wave the minimum key; a thread per ray was measured
 *     slower at every size (scripts/rays_time.py, profiles/rays_time.txt).  No atomics beyond the flag's.
 *     SC_ERR_ARG for a null context or a null origins, directions, t, hit or counts pointer, a negative n_rays or room,
 *     misaligned origins or directions, a max_t or disc_radius that is negative or not finite, a disc_radius above half
 *     the count's radius, a null `segments` with n_segments > 0, and on a batched grid; SC_ERR_CAPACITY for more than
 *     SC_MAX_SEGMENTS segments (or fewer than 0), more than 2^28 rays and too few rows; SC_ERR_STATE as for
 *     sc_pairs_sum_device.  All checked before anything is launched: the arrays are then untouched. */
int sc_pairs_rays_device(sc_ctx* ctx, const double* dev_origins, const double* dev_directions, int64_t n_rays,
                         double disc_radius /* 0: walls only */, double max_t,
                         const double* segments /* HOST, may be NULL */, int32_t n_segments,
                         double* dev_t, int64_t* dev_hit, int64_t room_rows,
                         int64_t* dev_counts /* [2]: rays, status */);

/* ---- Ray paths: hit points, normals and specular bounces ----------------------------------------------------------
 * The rays above, followed through `bounces` specular reflections: L = bounces + 1 legs per ray, each with its t, what
 * it hit, the hit point and the surface normal there.  Sonar and light multipath in a closed crate, the facet a range
 * finder sees, the slope of the free surface under a probe.  The rule is specified in NumPy in tests/ray_path_spec.py;
 * every operation is a float64 operation rounded on its own, and the directions are never normalised.
 *
 * Leg k has an origin o, a direction d, a budget m and an excluded object.  Leg 0 has the caller's origin and direction,
 * m = max_t and nothing excluded: its t and hit are sc_pairs_rays_device's, bit for bit.  A leg k >= 1 is hit by the same
 * rule, 0 <= t <= m, the smallest key (t, kind, index), with two changes: the object the leg before it hit -- disc j or
 * wall s -- takes no part, and a disc with cc <= 0 (the origin inside or on it) is hit at t = +0 only if b < 0, the ray
 * heading inward; otherwise the ray is leaving it and it is not hit.  A leg starts ON what it has just left, and that is
 * named, not nudged away from: the continuation needs no epsilon and its bits depend on none.
 * A leg that hit has P = (fl(ox + fl(t dx)), fl(oy + fl(t dy))) and the normal n: for a disc with centre c,
 * g = (fl(Px - cx), fl(Py - cy)), len = sqrt(fl(fl(gx gx) + fl(gy gy))), n = (fl(gx / len), fl(gy / len)); for a wall
 * A -> B, e = B - A, len = sqrt(fl(fl(ex ex) + fl(ey ey))), n0 = (fl(ey / len), fl(-ex / len)),
 * q = fl(fl(dx n0x) + fl(dy n0y)), n = -n0 if q > 0, else n0: the normal faces the side the ray came from.
 * The next leg: dn = fl(fl(dx nx) + fl(dy ny)); dn < 0: k2 = fl(2 dn), d' = (fl(dx - fl(k2 nx)), fl(dy - fl(k2 ny)));
 * otherwise d' = d (the ray leaves already: a leg 0 that began inside a disc, pointing outward).  o' = P, m' = fl(m - t).
 * dev_end[r] says how the path of ray r ended: 0, all L legs hit something; 1, a leg met nothing within its budget --
 * that leg has t = +inf, hit = -1, P = n = NaN; 2, leg 0 is dead (t = NaN, hit = -1), or a normal has a component that is
 * not finite (len = 0, a hit from the disc's own centre: the leg is written as computed), or the next leg would be dead
 * (a number of o' or d' not finite, a' = 0); and, only when discs are looked for, the two tests of the call's status
 * made on (o', d', m'): -1, a coordinate c of o' or of the end point fl(o' + fl(m' d')) fails fl(|c| / radius) < 2^31 or
 * that end point is not finite -- tested first --, -4, fl(8192 dt) <= t_end with dt = fl(radius / sqrt(a')) and
 * t_end = min(m', the next leg's nearest wall hit, the excluded wall left out).  The tests of a next leg are made only
 * when there is one.  Every leg after the last one written is t = NaN, hit = -1, P = n = NaN: the call writes all L rows
 * of every ray itself, the caller's arrays need no clear.
 *
 * sc_pairs_ray_paths_device  is sc_pairs_rays_device in its arguments, rules of the stream, refusals and statuses, with
 *     `bounces`, 0 .. SC_RAY_MAX_BOUNCES, and the wider outputs: dev_t and dev_hit n_rays x L, dev_points and dev_normals
 *     n_rays x L x 2 float64, aligned to 16 bytes, dev_end n_rays int64; `room_rows` is their room in rays.  The statuses
 *     in dev_counts[1] are about leg 0, the caller's input, and refuse the whole call: -1 and -4 as above, nothing else
 *     written.  Later legs are data: their failures end that ray alone, in dev_end.
 *     The algorithm: the two check passes of the rays on leg 0, then a wave per ray that keeps the ray, leg after leg:
 *     the walls with the excluded one skipped, the walk of sc_pairs_rays_device from step 0 with the leg's own dt, the
 *     place of the best candidate in the sorted arrays carried through the wave's minimum so that its centre is read,
 *     not searched again; every lane computes the normal, the reflection and the next leg's tests, so the wave stays
 *     uniform (csrc/sc_rays.h extends the walk's argument to later legs).  No LDS, no atomics beyond the flag's.
 *     SC_ERR_ARG, SC_ERR_CAPACITY and SC_ERR_STATE as for sc_pairs_rays_device, and SC_ERR_ARG for `bounces` outside
 *     0 .. SC_RAY_MAX_BOUNCES, a null points, normals or end pointer and misaligned points or normals.  All checked before
 *     anything is launched. */
#define SC_RAY_MAX_BOUNCES 15
int sc_pairs_ray_paths_device(sc_ctx* ctx, const double* dev_origins, const double* dev_directions, int64_t n_rays,
                              int32_t bounces, double disc_radius /* 0: walls only */, double max_t,
                              const double* segments /* HOST, may be NULL */, int32_t n_segments,
                              double* dev_t /* n_rays x L */, int64_t* dev_hit /* n_rays x L */,
                              double* dev_points /* n_rays x L x 2 */, double* dev_normals /* n_rays x L x 2 */,
                              int64_t* dev_end /* n_rays */, int64_t room_rows, int64_t* dev_counts /* [2] */);

/* ---- The batched forms of the four calls above: clusters, histograms, rays and ray paths of a minibatch -------------
 * Each reads the grid that a count after sc_pairs_set_batch_device has left -- B clouds, cloud b the rows
 * ptr[b] .. ptr[b + 1] -- and returns SC_ERR_ARG on an unbatched grid, as its unbatched twin does on a batched one.  Each
 * obeys the count-then-read protocol of its twin, with the same arguments, alignment rules, dev_counts[2], rules of the
 * stream, refusals and status codes, and one more status: dev_counts[1] = -3 when the count's offsets, or the call's own
 * query offsets, were not in order -- found on the device, nothing else is written.  tests/batch_readers_spec.py is the
 * rule: there is no new arithmetic, every result is the twin's rule cloud by cloud, concatenated in cloud order, indices
 * global.  The kernels are the twins' with the row's record (its cloud and index range) read once per row: the cloud
 * goes into the bucket hash, the range decides (csrc/sc_pairs.h).
 *
 * sc_pairs_label_batch_device  sc_pairs_label_device plus dev_cluster_ptr, int64, clouds + 1 entries, always written
 *     whole.  A cluster never crosses clouds.  Labels and roots are global; clusters are numbered by their smallest
 *     member, so cloud b's clusters are the contiguous range dev_cluster_ptr[b] .. dev_cluster_ptr[b + 1], and
 *     dev_cluster_ptr[clouds] = C.  A cloud without a finite point has no cluster: its two entries are equal.  The label
 *     it leaves is an ordinary one: sc_pairs_cluster_sums_device reads it unchanged.  SC_ERR_ARG also for a null
 *     dev_cluster_ptr.
 * sc_pairs_hist_batch_device  sc_pairs_hist_device with totals per cloud: dev_table as before, rows x bins int32;
 *     dev_cloud_total int64, clouds x bins contiguous, row b the column sums of the table over the rows of cloud b (all
 *     zero for a cloud without rows); `room_clouds`, its room in clouds, must be at least the grid's clouds.  With
 *     dev_queries, sc_pairs_set_query_batch_device comes first, as for every query-form reader of a batched grid.  The
 *     context's accumulator grows with clouds x bins: SC_ERR_CAPACITY beyond SC_HIST_BATCH_MAX_CELLS words, and for too
 *     small a room_clouds.
 * sc_pairs_rays_batch_device, sc_pairs_ray_paths_batch_device  the unbatched argument lists.  Rays are always the query
 *     form, so sc_pairs_set_query_batch_device comes first with the rays' offsets: ray r of ray-cloud b meets the discs
 *     of cloud b only, a ray-cloud over an empty cloud sees the walls alone.  The walls go in by value and are shared by
 *     all clouds.  dev_hit is the global row, and so is the disc a path's next leg leaves out. */
enum { SC_HIST_BATCH_MAX_CELLS = 1 << 24 };
int sc_pairs_label_batch_device(sc_ctx* ctx, int64_t* dev_labels, int64_t room_rows, int64_t* dev_sizes /* may be NULL */,
                                int64_t* dev_roots /* may be NULL */, int64_t room_clusters,
                                int64_t* dev_cluster_ptr /* clouds + 1 */, int64_t* dev_counts /* [2]: n, C */);
int sc_pairs_hist_batch_device(sc_ctx* ctx, const double* dev_queries /* NULL: the points themselves */, int64_t n_queries,
                               const double* edges2 /* HOST, bins + 1 */, int32_t bins,
                               int32_t* dev_table /* rows x bins, may be NULL */,
                               int64_t* dev_cloud_total /* clouds x bins, may be NULL */, int64_t room_rows,
                               int64_t room_clouds, int64_t* dev_counts /* [2]: rows, status */);
int sc_pairs_rays_batch_device(sc_ctx* ctx, const double* dev_origins, const double* dev_directions, int64_t n_rays,
                               double disc_radius /* 0: walls only */, double max_t,
                               const double* segments /* HOST, may be NULL */, int32_t n_segments,
                               double* dev_t, int64_t* dev_hit, int64_t room_rows,
                               int64_t* dev_counts /* [2]: rays, status */);
int sc_pairs_ray_paths_batch_device(sc_ctx* ctx, const double* dev_origins, const double* dev_directions, int64_t n_rays,
                                    int32_t bounces, double disc_radius /* 0: walls only */, double max_t,
                                    const double* segments /* HOST, may be NULL */, int32_t n_segments,
                                    double* dev_t /* n_rays x L */, int64_t* dev_hit /* n_rays x L */,
                                    double* dev_points /* n_rays x L x 2 */, double* dev_normals /* n_rays x L x 2 */,
                                    int64_t* dev_end /* n_rays */, int64_t room_rows, int64_t* dev_counts /* [2] */);

#ifdef __cplusplus
}
#endif
#endif /* SANDCRATE_HIP_H */
