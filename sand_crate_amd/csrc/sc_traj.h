// Trajectories (sc_traj_enable_device / sc_traj_capture / sc_traj_disable): the state at full precision as frames of one
// 32-byte record (x, y, vx, vy) per particle id, in the CALLER's device memory -- row r of a frame is the particle whose
// id is id0 + r, whatever slot it sits in, so frames line up by particle without a sort.  The rule is specified in NumPy
// by tests/trajectory_spec.py on top of tests/state_spec.py: a present row holds the bits sc_export_state_device delivers
// for that particle, an absent one four NaNs of one fixed pattern (kTrajFillBits).  Included once by sandcrate_hip.hip.
// Recording only reads the state: no counter of the tick, flag or particle array is written.
//
//   reserve  one workgroup of one wave: reads the stored count on the device and takes the frame's index from the cursor
//            word -- or, the log being full, raises the counter of dropped frames; an abandoned tick leaves neither --,
//            writes the frame's tick and count, zeroes its outsiders, and leaves the index (or -1) in the words for the
//            two kernels behind it on the stream.  One thread: the stream orders the frames, nothing here races.
//   clear    a thread per row of the frame: the NaN record as two 16-byte stores (and the pressure), fully coalesced.
//   scatter  a thread per stored slot: a live slot (the export's rule: below the stored count, x finite) whose id lies in
//            the window writes its record as two 16-byte stores -- position and velocity share a record, so a scattered
//            row touches one cache line, not two -- and its pressure.  Slots are cell-sorted and ids are not: the stores
//            are uncoalesced by nature, the price of skipping the sort (profiles/trajectory_time.txt).  A live slot
//            outside the window is counted, a stored slot that is not live is taken off the frame's count: one integer
//            add per wave that has any (ballot, popcount), and every lane reaches the ballots.
// No floating-point atomics, no workgroup waits for another, no LDS.
#pragma once
#include "sc_device.h"

namespace sc {

constexpr unsigned long long kTrajFillBits = 0x7FF8000000000000ull;  // the quiet NaN of an absent row (NumPy's np.nan)

// the trajectory words: int64 each, in the caller's memory next to the log
enum TrajWord { JW_CURSOR = 0, JW_DROPPED = 1, JW_AT = 2, JW_SPARE = 3, JW_COUNT = 4 };

struct TrajArgs {
  long long tick;      // ticks finished by the context
  long long frames;    // the log's capacity in frames
  long long id0, rows; // the window of ids [id0, id0 + rows)
  int on_demand;       // sc_traj_capture: the state as it stands, whatever became of the last tick
  int pressure_valid;  // the export's rule: P belongs to the slots the last finished tick left live
  int cap;             // capacity of the storage arrays
};

// the log: the caller's arrays (pressure may be null)
struct TrajLog {
  double* states;      // frames x rows x 4
  double* pressure;    // frames x rows
  long long* ticks;    // frames
  long long* counts;   // frames
  long long* outside;  // frames
  long long* words;    // JW_COUNT
};

__global__ void __launch_bounds__(64) k_traj_reserve(TrajArgs a, const int* __restrict__ counters, TrajLog o) {
  if (threadIdx.x != 0) return;
  const long long n = max(0, min(counters[C_NS], a.cap));
  long long f = -1;
  if (!a.on_demand && tick_abandoned(counters)) {
    // the log holds a frame per tick that happened: an abandoned one leaves none, and none is counted as dropped
  } else if (o.words[JW_CURSOR] >= 0 && o.words[JW_CURSOR] < a.frames) {
    f = o.words[JW_CURSOR];
    o.words[JW_CURSOR] = f + 1;
    o.ticks[f] = a.tick;
    o.counts[f] = n;  // (the stored slots; the scatter takes off those that are not live)
    o.outside[f] = 0;
  } else {  // the log is full: the frame is absent, and counted
    o.words[JW_DROPPED] += 1;
  }
  o.words[JW_AT] = f;
}

__global__ void __launch_bounds__(kBlock) k_traj_clear(TrajArgs a, TrajLog o) {
  const long long f = o.words[JW_AT];
  if (f < 0) return;  // no frame (uniform over the launch)
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.rows) return;
  const double fill = __longlong_as_double((long long)kTrajFillBits);
  double2* rec = (double2*)(o.states + (f * a.rows + r) * 4);
  rec[0] = make_double2(fill, fill);
  rec[1] = make_double2(fill, fill);
  if (o.pressure) o.pressure[f * a.rows + r] = fill;
}

__global__ void __launch_bounds__(kBlock)
    k_traj_scatter(TrajArgs a, const int* __restrict__ counters, TrajLog o, const double* __restrict__ x,
                   const double* __restrict__ y, const double* __restrict__ vx, const double* __restrict__ vy,
                   const int* __restrict__ id, const double* __restrict__ P) {
  const long long f = o.words[JW_AT];
  if (f < 0) return;  // no frame (uniform over the launch)
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int ns = max(0, min(counters[C_NS], a.cap));
  const bool stored = s < ns;
  const double xs = stored ? x[s] : 0.0;
  const bool live = stored && fabs(xs) < __builtin_inf();  // (NaN compares false: absent, as in the export)
  const long long r = live ? (long long)id[s] - a.id0 : -1;  // 64 bits: id0 + rows may pass INT_MAX
  const bool inside = live && r >= 0 && r < a.rows;
  if (inside) {
    double2* rec = (double2*)(o.states + (f * a.rows + r) * 4);
    rec[0] = make_double2(xs, y[s]);
    rec[1] = make_double2(vx[s], vy[s]);
    if (o.pressure) {
      const int np = a.pressure_valid ? pressure_slots(counters, ns) : 0;
      o.pressure[f * a.rows + r] = s < np ? P[s] : 0.0;
    }
  }
  const unsigned long long out = __ballot(live && !inside), dead = __ballot(stored && !live);
  if ((threadIdx.x & 63) == 0) {
    if (out) atomicAdd((unsigned long long*)&o.outside[f], (unsigned long long)__popcll(out));
    if (dead) atomicAdd((unsigned long long*)&o.counts[f], (unsigned long long)(-(long long)__popcll(dead)));
  }
}

}  // namespace sc
