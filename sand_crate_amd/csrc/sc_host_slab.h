// Host side of multi-GPU slabs: the cut, halo pack and unpack, the overlap of the exchange with pass B, and RCCL.
#pragma once
#include "sc_host.h"
#include "sc_rccl.h"

extern "C" {

// ---- multi-GPU slabs ---------------------------------------------------------------------------

int sc_set_slab_axis(sc_ctx* c, int32_t axis) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "slab cannot change inside a tick");
  if (axis != 0 && axis != 1) return fail(SC_ERR_ARG, "slab axis: 0 (columns of x) or 1 (rows of y)");
  c->link.slab_axis = axis;
  c->link.halo_ring_from = c->tick;
  return SC_OK;
}

int sc_set_slab(sc_ctx* c, int64_t col_lo, int64_t col_hi, int32_t halo, int32_t has_left, int32_t has_right) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "slab cannot change inside a tick");
  if (col_hi <= col_lo || halo < 3) return fail(SC_ERR_ARG, "slab needs col_lo < col_hi and a halo of at least 3 columns");
  c->slab = true;
  c->link.own_lo = col_lo;
  c->link.own_hi = col_hi;
  c->link.halo = halo;
  c->link.has_left = has_left ? 1 : 0;
  c->link.has_right = has_right ? 1 : 0;
  c->link.halo_ring_from = c->tick;  // new cuts: the halo counts of earlier ticks say nothing about the coming ones
  HIPCHK(c->link.owned_out.grow(1, c->stream));
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
  if (src < c->link.halo_ring_from) return SC_OK;  // no history yet: whole buffers
  // tick `src` has finished on the device (at most a few ticks are ever queued), so its counts are published
  if (const int rc = wait_ticks_finished(c, src + 1, "halo counts")) return rc;
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
  if (ncols > c->link.colHist.size()) HIPCHK(c->link.colHist.grow(ncols + 256, c->stream));
  HIPCHK(hipMemsetAsync(c->link.colHist, 0, ncols * sizeof(int), c->stream));
  const double d = c->custom_grid ? c->custom_d : c->now.params.particle_radius * 2;
  hipLaunchKernelGGL(k_column_histogram, dim3(grid_for(launch_bound(c))), dim3(kBlock), 0, c->stream, c->counters, c->x,
                     c->link.slab_axis ? c->y : c->x, d, (long long)col0, (int)ncols, c->link.colHist);
  std::vector<int> h(ncols);
  if (const int rc = read_back(c, h.data(), c->link.colHist, ncols * sizeof(int))) return rc;
  for (int k = 0; k < ncols; ++k) hist[k] = h[k];
  return SC_OK;
}

int sc_halo_pack(sc_ctx* c, double* dev_left, double* dev_right, int64_t cap_records) {
  if (!c || !dev_left || !dev_right || cap_records < 1) return fail(SC_ERR_ARG, "bad halo buffers");
  if (!c->slab) return fail(SC_ERR_STATE, "sc_set_slab first");
  if (c->in_step) return fail(SC_ERR_STATE, "halo exchange happens between ticks");
  if (const int rc = make_world(c)) return rc;
  if (c->prebinned) return fail(SC_ERR_STATE, "the halo message of the promised tick was packed by sc_step_finish");
  c->link.band_pending = false;  // this message depends on the kernel below, not on a split force kernel
  c->link.haloL = dev_left;  // stay bound: with sc_set_next_inputs, sc_step_finish packs the next message itself
  c->link.haloR = dev_right;
  c->link.haloCap = (int)cap_records;
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
  auto launch = [&](auto kernel, const WallInputs& walls) {
    hipLaunchKernelGGL(kernel, grid, block, 0, c->stream, from_left, from_right, capL, capR, c->counters, c->x, c->y, c->vx,
                       c->vy, c->id[0], (int)c->cap, c->link.haloL, c->link.haloR, walls, c->cellS, c->wslotS, c->cellCount,
                       c->wrec[c->tick & 1], ring);
  };
  if (c->prebinned) {  // the stored particles went through K1 of the coming tick in pass B: same for the arrivals
    launch(k_halo_unpack<true>, c->promised);
  } else {
    if (const int rc = make_world(c)) return rc;  // (the slab and the diameter the records are judged by)
    launch(k_halo_unpack<false>, wall_inputs_of(c->w));
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
  if (!c->link.ev_band) HIPCHK(hipEventCreateWithFlags(&c->link.ev_band, hipEventDisableTiming | hipEventDisableSystemFence));
  // (ev_xchg orders halo buffers that a peer GPU wrote: it keeps the system-scope fence)
  if (!c->link.ev_xchg) HIPCHK(hipEventCreateWithFlags(&c->link.ev_xchg, hipEventDisableTiming));
  return SC_OK;
}

int sc_set_halo_overlap(sc_ctx* c, int on) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "halo overlap cannot change inside a tick");
  if (on && !c->slab) return fail(SC_ERR_STATE, "sc_set_slab first");
  HIPCHK(hipSetDevice(c->device));
  if (on) {
    if (const int rc = ensure_side_stream(c)) return rc;
  }
  c->link.overlap = on != 0;
  return SC_OK;
}

int sc_set_band_flag(sc_ctx* c, int on) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (c->in_step) return fail(SC_ERR_STATE, "the band mode cannot change inside a tick");
  c->link.band_by_flag = on != 0;  // (a band that is pending keeps the announcement it was launched with: band_flagged)
  return SC_OK;
}

int sc_side_stream(sc_ctx* c, void** stream) {
  if (!c || !stream) return fail(SC_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(c->device));
  if (const int rc = ensure_side_stream(c)) return rc;
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
    if (q->link.band_pending && q->link.band_flagged) {  // the window blocks of q's one-launch force kernel
      hipLaunchKernelGGL(k_wait_band, dim3(1), dim3(1), 0, c->side_stream, q->counters, q->link.band_epoch);
      continue;
    }
    if (!q->link.band_pending) HIPCHK(hipEventRecord(q->link.ev_band, q->stream));  // no split pass B before: wait for all of it
    HIPCHK(hipStreamWaitEvent(c->side_stream, q->link.ev_band, 0));
  }
  return SC_OK;
}

// context's stream <- what was enqueued on the side stream since sc_halo_overlap_begin (the received buffers)
int sc_halo_overlap_end(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!c->side_stream || !c->link.ev_xchg) return fail(SC_ERR_STATE, "sc_halo_overlap_begin first");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventRecord(c->link.ev_xchg, c->side_stream));
  HIPCHK(hipStreamWaitEvent(c->stream, c->link.ev_xchg, 0));
  c->link.band_pending = false;
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
  if (c->link.comm) return fail(SC_ERR_STATE, "sc_comm_init called twice");
  if (rccl_load(rccl_path)) return fail(SC_ERR_HIP, "%s", rccl_api().error.c_str());
  HIPCHK(hipSetDevice(c->device));
  RcclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  RCCLCHK(rccl_api().CommInitRank(&c->link.comm, world, u, rank));
  c->link.comm_world = world;
  return SC_OK;
}

int sc_comm_destroy(sc_ctx* c) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!c->link.comm) return SC_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  RcclComm comm = c->link.comm;
  c->link.comm = nullptr;
  RCCLCHK(rccl_api().CommDestroy(comm));
  return SC_OK;
}

int sc_halo_exchange(sc_ctx* c, const double* send_left, int64_t send_left_records, double* recv_left,
                     int64_t recv_left_records, int32_t left_rank, const double* send_right, int64_t send_right_records,
                     double* recv_right, int64_t recv_right_records, int32_t right_rank) {
  if (!c) return fail(SC_ERR_ARG, "null context");
  if (!c->link.comm) return fail(SC_ERR_STATE, "sc_comm_init first");
  if (c->in_step) return fail(SC_ERR_STATE, "halo exchange happens between ticks");
  if ((left_rank >= 0 && (!send_left || !recv_left || left_rank >= c->link.comm_world || send_left_records < 1 || recv_left_records < 1)) ||
      (right_rank >= 0 && (!send_right || !recv_right || right_rank >= c->link.comm_world || send_right_records < 1 || recv_right_records < 1)))
    return fail(SC_ERR_ARG, "neighbor ranks %d / %d need their buffers and record counts and must be below %d", left_rank,
                right_rank, c->link.comm_world);
  auto doubles = [](int64_t records) { return (size_t)(records + 1) * kHaloFields; };  // + the header record
  const RcclApi& r = rccl_api();
  HIPCHK(hipSetDevice(c->device));
  hipStream_t xs = c->stream;
  if (c->link.overlap) {  // on the side stream, next to the interior blocks of the last pass B
    if (const int rc0 = sc_halo_overlap_begin(c, nullptr)) return rc0;
    xs = c->side_stream;
  }
  RCCLCHK(r.GroupStart());
  int rc = 0;
  // posting order is the same on every rank (left pair, then right pair): rank k's right pair meets rank k+1's left pair
  if (left_rank >= 0) {
    if (!rc) rc = r.Send(send_left, doubles(send_left_records), kRcclDouble, left_rank, c->link.comm, xs);
    if (!rc) rc = r.Recv(recv_left, doubles(recv_left_records), kRcclDouble, left_rank, c->link.comm, xs);
  }
  if (right_rank >= 0) {
    if (!rc) rc = r.Send(send_right, doubles(send_right_records), kRcclDouble, right_rank, c->link.comm, xs);
    if (!rc) rc = r.Recv(recv_right, doubles(recv_right_records), kRcclDouble, right_rank, c->link.comm, xs);
  }
  const int rc_end = r.GroupEnd();
  if (rc) return fail(SC_ERR_HIP, "RCCL: send/recv failed: %s", rccl_error(rc));
  if (rc_end) return fail(SC_ERR_HIP, "RCCL: ncclGroupEnd failed: %s", rccl_error(rc_end));
  if (c->link.overlap) return sc_halo_overlap_end(c);
  return SC_OK;
}

int sc_owned_count(sc_ctx* c, int64_t* n) {
  if (!c || !n) return fail(SC_ERR_ARG, "null argument");
  if (c->in_step) return fail(SC_ERR_STATE, "sc_owned_count inside a tick");
  int rc = c->slab ? make_world(c) : SC_OK;
  if (rc) return rc;
  HIPCHK(c->link.owned_out.grow(1, c->stream));
  HIPCHK(hipMemsetAsync(c->link.owned_out, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(k_owned_count, dim3(grid_for(launch_bound(c))), dim3(kBlock), 0, c->stream, c->counters, c->x,
                     c->link.owned_out);
  int h = 0;
  if ((rc = read_back(c, &h, c->link.owned_out, sizeof(int)))) return rc;
  *n = h;
  return SC_OK;
}

}  // extern "C"
