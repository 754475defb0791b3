// Host side of the checkpoint: snapshot on the stream, copy to the host on the side stream, restore.
#pragma once
#include "sc_host.h"

extern "C" {

// ---- checkpoint ---------------------------------------------------------------------------------
// The stored state is copied device-to-device on the context's stream (a few microseconds), the copy travels to
// pinned host memory on a side stream, and the ticks that follow run meanwhile; sc_checkpoint_finish waits for the
// side stream only.

int sc_checkpoint_begin(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_checkpoint_begin inside a tick");
  if (c->snap.pending) return fail(SC_ERR_STATE, "a checkpoint is already under way: sc_checkpoint_finish first");
  HIPCHK(hipSetDevice(c->device));
  // After a promised tick the storage arrays already hold the coming tick's removal and wall fix while its cell
  // indices and bucket counts live in buffers a snapshot does not take: a restore would run that wall pass a second
  // time, on fixed positions.  (Crate.run / physics_tick never leave a promise pending between calls.)
  if (c->prebinned)
    return fail(SC_ERR_STATE, "sc_checkpoint_begin after sc_set_next_inputs promised the next tick: run that tick first");
  // the side stream may exist already (halo overlap creates it): every snapshot resource is created on its own
  if (const int rc = ensure_side_stream(c)) return rc;
  if (!c->snap.ready) HIPCHK(hipEventCreateWithFlags(&c->snap.ready, hipEventDisableTiming));
  if (!c->snap.done) HIPCHK(hipEventCreateWithFlags(&c->snap.done, hipEventDisableTiming));
  HIPCHK(c->snap.counters_h.grow(C_COUNT, c->side_stream));
  HIPCHK(c->snap.rng_h.grow(1, c->side_stream));
  HIPCHK(c->snap.rng_d.grow(1, c->side_stream));
  const int64_t n = launch_bound(c);  // a host-side bound of the stored count; the exact count travels with the copy
  if (n > c->snap.id_h.size()) {  // (id_h grows last: once it has grown, so have the others)
    const int64_t m = std::min<int64_t>(c->cap, n + n / 2 + 1024);
    for (int k = 0; k < 4; ++k) {
      HIPCHK(c->snap.d[k].grow(m, c->side_stream));
      HIPCHK(c->snap.h[k].grow(m, c->side_stream));
    }
    HIPCHK(c->snap.id_d.grow(m, c->side_stream));
    HIPCHK(c->snap.id_h.grow(m, c->side_stream));
  }
  const double* src[4] = {c->x, c->y, c->vx, c->vy};
  // on the context's stream: after the last tick, before the next one changes the storage arrays
  for (int k = 0; k < 4 && n > 0; ++k)
    HIPCHK(hipMemcpyAsync(c->snap.d[k], src[k], n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  if (n > 0) HIPCHK(hipMemcpyAsync(c->snap.id_d, c->id[0], n * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  c->snap.has_rng = c->rng != nullptr;
  if (c->rng) HIPCHK(hipMemcpyAsync(c->snap.rng_d, c->rng, sizeof(RngState), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->snap.counters_h, c->counters, C_COUNT * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipEventRecord(c->snap.ready, c->stream));
  // on the side stream: the snapshot goes to pinned host memory while the context's stream runs on
  HIPCHK(hipStreamWaitEvent(c->side_stream, c->snap.ready, 0));
  for (int k = 0; k < 4 && n > 0; ++k)
    HIPCHK(hipMemcpyAsync(c->snap.h[k], c->snap.d[k], n * sizeof(double), hipMemcpyDeviceToHost, c->side_stream));
  if (n > 0) HIPCHK(hipMemcpyAsync(c->snap.id_h, c->snap.id_d, n * sizeof(int), hipMemcpyDeviceToHost, c->side_stream));
  if (c->rng) HIPCHK(hipMemcpyAsync(c->snap.rng_h, c->snap.rng_d, sizeof(RngState), hipMemcpyDeviceToHost, c->side_stream));
  HIPCHK(hipEventRecord(c->snap.done, c->side_stream));
  c->snap.n_bound = n;
  c->snap.tick = c->tick;
  c->snap.pending = true;
  return SC_OK;
}

int sc_checkpoint_finish(sc_ctx* c, double* xy, double* vxy, int64_t* ids, int64_t room, int64_t* n_out, int64_t* tick,
                         int64_t* next_id, uint32_t* rng_key, int32_t* rng_pos) {
  if (!c || !n_out) return fail(SC_ERR_ARG, "null argument");
  if (!c->snap.pending) return fail(SC_ERR_STATE, "sc_checkpoint_begin first");
  HIPCHK(hipEventSynchronize(c->snap.ready));  // the counters' copy rode on the context's stream up to here
  HIPCHK(hipEventSynchronize(c->snap.done));
  c->snap.pending = false;
  const int64_t stored = std::min<int64_t>(c->snap.counters_h[C_NS], c->snap.n_bound);
  const std::vector<int> order = index_order(c->snap.id_h, c->snap.h[0], stored);
  const int64_t n = (int64_t)order.size();
  *n_out = n;
  if (tick) *tick = c->snap.tick;
  if (next_id) *next_id = c->snap.counters_h[C_NEXT_ID];
  const RngState& rs = *c->snap.rng_h;
  if (rng_pos) *rng_pos = c->snap.has_rng ? rs.pos : -1;
  if (rng_key && c->snap.has_rng) std::memcpy(rng_key, rs.mt, sizeof rs.mt);
  if (n > room) return fail(SC_ERR_CAPACITY, "host arrays hold %lld, the checkpoint has %lld particles", (long long)room, (long long)n);
  write_pairs(xy, order, c->snap.h[0], c->snap.h[1]);
  write_pairs(vxy, order, c->snap.h[2], c->snap.h[3]);
  for (int64_t k = 0; k < n && ids; ++k) ids[k] = c->snap.id_h[order[k]];
  return SC_OK;
}

int sc_restore_counters(sc_ctx* c, int64_t tick, int64_t next_id) {
  if (!c || tick < 0 || next_id < 0 || next_id > std::numeric_limits<int>::max()) return fail(SC_ERR_ARG, "bad tick / next id");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_restore_counters inside a tick");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->prebinned)
    if (const int rc = abandon_promise(c)) return rc;
  c->tick = tick;
  c->link.halo_ring_from = tick;
  c->live_hint_from = tick;
  c->progress[kProgressTicks] = (int)tick;  // nothing of the new numbering is queued
  c->next_id = std::max<int64_t>(c->next_id, next_id);
  const int nid = (int)c->next_id;
  HIPCHK(hipMemcpyAsync(c->counters + C_NEXT_ID, &nid, sizeof nid, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return SC_OK;
}

}  // extern "C"
