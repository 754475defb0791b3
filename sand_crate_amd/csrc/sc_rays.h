// Ray sensors on the device (sc_pairs_rays_device): for every ray -- an origin and a direction -- the first thing it
// meets among the discs of radius rho round the points of the last count and up to SC_MAX_SEGMENTS wall segments: the
// ray's parameter t and what was hit.  A range finder, the height of the free surface under a probe, the particle under
// the cursor.  The rule is specified in NumPy, by brute force, in tests/ray_spec.py; the result is a pure function of
// the points, the walls, the rays, rho and max_t.  Included once by sandcrate_hip.hip, after sc_hist.h.
//
// The rule (ray_disc, ray_walls below: every operation rounded on its own, -ffp-contract=off).  Disc with centre c:
// f = o - c, a = fl(fl(dx dx) + fl(dy dy)), b = fl(fl(fx dx) + fl(fy dy)), cc = fl(fl(fl(fx fx) + fl(fy fy)) - rho2);
// cc <= 0: t = +0; else b >= 0: none; else disc = fl(fl(b b) - fl(a cc)) < 0: none; else t = fl(cc / fl(-b + sqrt(disc)));
// a hit iff t <= max_t.  Wall A -> B, e = B - A, g = A - o: den = fl(fl(dx ey) - fl(dy ex)), 0: none;
// t = fl(fl(fl(gx ey) - fl(gy ex)) / den), u = fl(fl(fl(gx dy) - fl(gy dx)) / den); a hit iff 0 <= t <= max_t and
// 0 <= u <= 1, from either face, -0 reported as +0.  The result is the smallest key (t, kind, index), walls before
// discs: hit = j for disc j, -2 - s for wall s, -1 and t = +inf for none; a ray with an origin or a direction that is
// not finite, or with a = 0, is dead: t = NaN, hit = -1.  sqrt and / are correctly rounded here, as the host's are.
//
// Everything about the points is read from the workspace the last count left (sc_pairs.h), through PairsView, and
// nothing of it is written: any other reader may follow.
//   k_reader_check (sc_pairs.h) prepares counts[1] and raises the domain bit of the readers' flag for an origin outside
//                  the domain: the origins are the queries;
//   k_rays_check   a thread per ray: the domain bit for a live ray's end point fl(o + fl(max_t d)) that fails
//                  pairs_outside's rule or is not finite (ray_end_outside), and kRayFlagRange for a live ray whose walk
//                  would take more than kRayMaxSteps steps (ray_too_long).  Not launched for walls alone;
//   k_rays         a wave per ray: the walls, the walk, the result -- unless a flag is up: then counts[1] = -1 (the
//                  domain) or -4 (the range) is all that is written (ray_begin).  A ray is one leg;
//   k_ray_paths    (sc_pairs_ray_paths_device) the same wave, kept for bounces + 1 legs in a loop: "Paths" below.
//
// A leg is what is walked: an origin o, a direction d, a budget max_t -- and, in a path, the object the leg before it hit,
// which takes no part in it.  There is one walk, ray_walk, with one scan, ray_scan, for the legs of both kernels; what
// follows is about that one loop.
//
// The walk.  s is the count's radius and the host requires rho <= s / 2; the cells are h = fl(s (1 + 2^-20)) wide.  With
// dt = fl(s / sqrt(a)), step k covers t in [fl(k dt), fl((k + 1) dt)] -- consecutive steps share their border, so the
// steps tile t >= 0 -- and looks at the 3 x 3 cells round the cell of its midpoint M = fl(o + fl(tm d)),
// tm = fl((k + 0.5) dt).  A candidate is a member of a bucket of those nine whose stored cell is the cell looked for,
// the own-cell test of every reader: it is tested by the rule, and the smallest key (t, j) is kept, so the order in
// which candidates are met does not reach the output.  The walls are tested first; t_end = min(max_t, the nearest wall's
// t) caps the walk: step k is walked iff fl(k dt) <= t_end.  The walk ends after the first step k with
// best t < fl((k + 1) dt).  A disc that would win has t* <= best t; its own step k* (the one whose piece holds t*) is
// then at most k, and -- the claim below -- the disc was a candidate of step k*.  ray_walk takes kRayWaveSteps steps
// at a time, lane L the cell L % 9 of step k0 + L / 9, takes the minimum key over the wave, and ends after the first
// batch with best t < fl((k0 + kRayWaveSteps) dt): the same argument with the batch's last step for k.
//
// What the walk asks of a leg, and who has seen to it before the leg is walked:
//   * the domain: o and the end point fl(o + fl(max_t d)) are finite and have |c| / s < 2^31;
//   * the range: fl(kRayMaxSteps dt) > t_end, with the leg's own dt and its own walls ("The cap" below).
// Leg 0 -- a ray of k_rays, the first leg of a path -- is tested by the two check kernels (the origins are the queries of
// k_reader_check) and refuses the call.  A later leg of a path is data: every lane of k_ray_paths tests (o', d', m') with
// the same ray_end_outside and ray_too_long, and the origin as well, and a leg that fails ends its ray alone.
//
// The claim: the disc hit at t* in step k has its centre c in the 3 x 3 block of M's cell, in computed cells.  With
// u = 2^-53 and |f| the distance from the origin to c:
//   * the point P = o + t* d (exact, at the COMPUTED t*) is at most sqrt(rho^2 + 18 u |f|^2) from c.  The computed a, b,
//     cc are those of an exact problem whose coefficients are off by 2u a, 2u |f| |d| and 3u |f|^2; t* solves that
//     problem up to the roundings of disc (3u b^2, seen through t / q <= t / |b|), of sqrt, the sum and the quotient
//     (3u t), and t* |d| <= |f| for a hit on the near side: put into |P - c|^2 - rho^2 = a t^2 + 2 b t + cc the terms add
//     up to at most 18 u |f|^2.  A walk has at most kRayMaxSteps = 2^13 steps, so |f| <= (2^13 + 1.5) s and, at
//     rho = s / 2 where it is worst, |P - c| <= s / 2 + 2^-22.8 s.  Nothing here assumes an exact origin: a, b and cc
//     are computed from a later leg's (o', d') exactly as from (o, d), whatever roundings made o' and d', and the walk
//     starts again at step 0;
//   * |P - M'| <= s / 2 (1 + 2^-35) for the exact midpoint M' = o + tm d: dt |d| = s (1 + 3u), and fl(k dt), tm and
//     fl((k + 1) dt) are each off by at most u 2^13 dt;
//   * the computed M is off M' by at most u (|M| + |tm d|) <= 2^-22 s (1 + 2^-17) per axis inside the domain
//     |c| / s < 2^31, which holds the origin and the end point and so every M between.
//     The last step walked has fl(k dt) <= t_end <= max_t, so its midpoint may lie up to half a cell BEYOND the end
//     point: |M| / s < 2^31 + 1/2 then, and M / h still below 2^31 by some 2^11 cells, because h > s (sc_pairs.h: 2047
//     cells short of the ends of int) -- the (int) conversion in pairs_cell is defined, and cx +- 1 does not overflow;
//   * the two divisions by h are each off by at most 2^-22 cells there (sc_pairs.h).
// So per axis the computed quotients of c and M differ by at most
//   (1 + 2^-22.8 + 2^-22 + 2^-34) / (1 + 2^-20) + 2^-21 < 1 - 2^-20 (1 - 0.15 - 0.25 - 0.5) < 1,
// and two numbers less than 1 apart have floors at most 1 apart.  The margin of 2^-20 is thus used up to nine tenths at
// the far corner of the domain, at the last step, for a grazed disc of the largest radius; 2^14 steps would not fit:
// the cap is the largest power of two the margin of sc_pairs.h carries.  An origin inside a disc (cc <= 0, t = 0) has c
// within rho (1 + 2u) of o, which lies in step 0's piece: the same bound with room to spare.
//
// The cap.  A live leg needs fl(kRayMaxSteps dt) > t_end: for leg 0 kRayFlagRange goes up otherwise and the call ends as
// status -4 -- a max_t of 1e12 in an open scene is a status, not a kernel that walks for minutes --, a later leg ends its
// ray with `end` -4.  (An a that overflowed gives dt = 0 and the same.)  A leg that passed ends its walk by step
// kRayMaxSteps: fl(k dt) is monotone in k.
//
// Paths (sc_pairs_ray_paths_device, k_ray_paths; the rule is tests/ray_path_spec.py).  The ray stays in its wave for
// L = bounces + 1 legs, each with its budget m.  A disc with cc <= 0 is hit (at t = +0) by a later leg only if b < 0 --
// the ray heads inward --, else the ray is leaving it.  A leg therefore starts ON the surface it has left and names it: no epsilon moves the origin, and no bit depends on
// one.  A leg that hit has P = fl(o + fl(t d)) and the normal n -- g = P - c, n = g / sqrt(fl(fl(gx gx) + fl(gy gy)))
// for a disc; n0 = (ey, -ex) / sqrt(fl(fl(ex ex) + fl(ey ey))) for a wall, negated if fl(fl(dx n0x) + fl(dy n0y)) > 0 --;
// the next leg has o' = P, m' = fl(m - t) and, with dn = fl(fl(dx nx) + fl(dy ny)) < 0, d' = fl(d - fl(fl(2 dn) n)),
// else d' = d.  How a path ends is `end`: 0 all legs hit, 1 a leg met nothing, 2 dead (leg 0, a normal that is not
// finite, the next leg), -1 and -4 the next leg fails the two tests above.
// The excluded disc is skipped by its index before the rule is asked, so it cannot win; skipping a candidate removes a
// key from a minimum and leaves the walk's argument for the others as it was.  A disc with cc <= 0 that is hit (b < 0)
// has its centre within rho (1 + 2u) of o', which lies in step 0's piece: the bound of the last sentence of the claim.  A
// disc with cc <= 0 that is NOT hit (b >= 0) is not a candidate at all, in the rule as in the walk.  The excluded wall is
// left out of t_end as out of the result.  The path is finite because every leg, a t = 0 leg included, uses up one of L.
//
// The form (profiles/rays_time.txt).  What every other reader does, a thread per row in workgroups of one wave, was
// built too -- the same ray_scan, the eighteen `start` loads of a step's nine buckets issued together -- and MEASURED
// slower at every size: a lane walks its steps one after the other, each a chain of dependent loads (6.8 us a step where
// the cells are mostly empty), and the lanes of a wave wait for its longest ray.  Over 1,048,576 particles the wave per
// ray took 25 us against 42 us for a fan of 256 rays and 0.79 ms against 2.52 ms for 262,144 rays looking down; over
// every 256th of those particles, where a ray walks some sixty cells, 74 against 758 us and 1.04 against 1.79 ms.
//
// The batched form (sc_pairs_rays_batch_device, sc_pairs_ray_paths_batch_device, on the grid of a count after
// sc_pairs_set_batch_device; the rule is tests/batch_readers_spec.py).  Rays are always the query form, so their clouds
// come as query offsets (sc_pairs_set_query_batch_device): ray r of ray-cloud b meets the discs of cloud b only.  The
// wave reads its ray's record (lo, hi, cloud) once -- pairs_row over query_ptr, uniform and so scalar --, hashes every
// step's cells with the cloud and drops a candidate whose index is outside [lo, hi) (pairs_in): the hash is for speed,
// the range for exactness, as in sc_pairs.h.  The walls go in by value and are shared by all clouds; `hit`, and a path's
// excluded disc, are global indices.  Nothing in the walk's claim changes: it speaks of the candidates that are met, and
// a cloud's discs lie in the buckets of its own hash.  k_rays_check is unchanged.  Offsets out of order -- the
// count's or the rays' -- are status -3.  The unbatched instantiations carry no record.
#pragma once
#include "sc_pairs.h"

namespace sc {

constexpr int kRayMaxSteps = 8192;      // 2^13: see "the claim" (mirrored by sand_crate_amd/_native.py: RAY_MAX_STEPS)
constexpr int kRayBlock = 64;           // a workgroup: the one wave of a ray
constexpr int kRayWaveSteps = 7;        // steps per batch: 63 (step, cell) pairs, one lane idle
constexpr int kRayFlagRange = 8;        // a bit of the readers' flag, beside kReaderFlag* (sc_pairs.h)
constexpr long long kRayStatusRange = -4;
constexpr int kRayNoDisc = INT_MAX;     // the index of "no disc yet": behind every j

struct RayWalls {
  double s[kMaxSeg][4];  // A.x, A.y, B.x, B.y: the caller's (S, 2, 2)
  int n;
};

struct RayOut {
  double* t;
  long long* hit;
  long long* counts;  // [2]: rays, status
};

// counts[1] with a flag up: batched, offsets out of order -- the count's or the rays' own -- come first (-3).
template <bool batched>
__device__ __forceinline__ long long ray_status(int flag, int own) {
  if (batched && ((flag & kPairsFlagBatch) || (own & kReaderFlagBatch))) return kPairsStatusBatch;
  return flag || (own & kReaderFlagDomain) ? kPairsStatusDomain : kRayStatusRange;
}

// Is the ray alive; a = fl(fl(dx dx) + fl(dy dy)).
__device__ __forceinline__ bool ray_live(XY o, XY d, double& a) {
  a = d.x * d.x + d.y * d.y;
  const double inf = __builtin_inf();
  return fabs(o.x) < inf && fabs(o.y) < inf && fabs(d.x) < inf && fabs(d.y) < inf && a != 0;
}

// The nearest wall hit: (t, s), the lowest s among equals; (+inf, -1) for none.  kPath: wall `skip` takes no part.
template <bool kPath = false>
__device__ __forceinline__ void ray_walls(const RayWalls& w, XY o, XY d, double max_t, double& best, int& who, int skip = -1) {
  best = __builtin_inf();
  who = -1;
  for (int s = 0; s < w.n; ++s) {
    if (kPath && s == skip) continue;
    const double ax = w.s[s][0], ay = w.s[s][1];
    const double ex = w.s[s][2] - ax, ey = w.s[s][3] - ay;
    const double gx = ax - o.x, gy = ay - o.y;
    const double den = d.x * ey - d.y * ex;
    const double t = (gx * ey - gy * ex) / den, u = (gx * d.y - gy * d.x) / den;
    if (den != 0 && t >= 0 && t <= max_t && u >= 0 && u <= 1 && t < best) {
      best = t == 0 ? 0.0 : t;  // (-0 is +0)
      who = s;
    }
  }
}

// The disc round c: is it hit, and at which t.  kPath and `later`, a leg >= 1 of a path: a disc the origin lies in or
// on is hit only by a ray that heads inward.
template <bool kPath = false>
__device__ __forceinline__ bool ray_disc(XY o, XY d, double a, XY c, double rho2, double max_t, double& t, bool later = false) {
  const double fx = o.x - c.x, fy = o.y - c.y;
  const double b = fx * d.x + fy * d.y;
  const double cc = (fx * fx + fy * fy) - rho2;
  if (cc <= 0) {
    if (kPath && later && !(b < 0)) return false;
    t = 0.0;
  } else {
    if (!(b < 0)) return false;
    const double disc = b * b - a * cc;
    if (!(disc >= 0)) return false;
    t = cc / (-b + sqrt(disc));
  }
  return t <= max_t;
}

// The candidates of one bucket, places lo .. hi - 1: those whose own cell is (cx, cy) -- and, batched, whose index lies
// in the ray's cloud --, by the rule, into the best key.  kPath, a leg of a path: disc `skip` takes no part (a global
// index, as j is, batched or not), `later` is ray_disc's, and the place in the sorted arrays of the best candidate rides
// along with its key, for the normal.  (`row` by value: by reference the compiler scheduled the unbatched k_rays
// differently from a kernel without a record.)
template <bool batched, bool kPath>
__device__ __forceinline__ void ray_scan(const PairsView& v, const PairsRow row, XY o, XY d, double a, double rho2,
                                         double max_t, bool later, int skip, unsigned cx, unsigned cy, int lo, int hi,
                                         double& best, int& who, int& place) {
  for (int k = lo; k < hi; ++k) {
    const uint2 cell = v.scell[k];
    if (cell.x != cx || cell.y != cy) continue;
    const int j = v.sidx[k];
    double t;
    if (kPath && j == skip) continue;
    if (!pairs_in<batched>(row, j) || !ray_disc<kPath>(o, d, a, v.sxy[k], rho2, max_t, t, later)) continue;
    if (t < best || (t == best && j < who)) {
      best = t;
      who = j;
      if (kPath) place = k;
    }
  }
}

// The walk of a leg (o, d, a) with the budget max_t and the nearest wall at tw, in steps of dt: the smallest key (best, who) among
// its discs, in every lane, and under kPath its place.  The caller sets (+inf, kRayNoDisc, any place).  Lane L < 63 takes
// cell L % 9 of step k0 + L / 9 of the batch (the lane is read here, where its range shows); everything else is uniform
// over the wave.  v.g.h is the count's; batched, the cells hash with the ray's cloud and ray_scan tests pairs_in.
template <bool batched, bool kPath>
__device__ __forceinline__ void ray_walk(const PairsView& v, const PairsRow row, XY o, XY d, double a, double rho2,
                                         double max_t, double tw, double dt, bool later, int skip, double& best, int& who,
                                         int& place) {
  const double t_end = fmin(max_t, tw);
  static_assert(9 * kRayWaveSteps <= kRayBlock && kRayBlock == 64, "a lane per (step, cell) pair of a batch, one wave");
  const int lane = (int)threadIdx.x, step = lane / 9, c = lane % 9;
  for (int k0 = 0; k0 < kRayMaxSteps && (double)k0 * dt <= t_end; k0 += kRayWaveSteps) {  // (uniform over the wave)
    const int k = k0 + step;
    if (step < kRayWaveSteps && (double)k * dt <= t_end) {
      const double tm = ((double)k + 0.5) * dt;
      const unsigned cx = pairs_cell(o.x + tm * d.x, v.g.h) + (unsigned)(c % 3 - 1);
      const unsigned cy = pairs_cell(o.y + tm * d.y, v.g.h) + (unsigned)(c / 3 - 1);
      const unsigned bk = pairs_bucket(cx, cy, row.cloud, v.g.mask);
      ray_scan<batched, kPath>(v, row, o, d, a, rho2, max_t, later, skip, cx, cy, v.start[bk], v.start[bk + 1], best, who, place);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {  // the smallest key of the wave, in every lane
      const double t2 = __shfl_xor(best, off, 64);
      const int j2 = __shfl_xor(who, off, 64);
      const int p2 = kPath ? __shfl_xor(place, off, 64) : 0;
      if (t2 < best || (t2 == best && j2 < who)) {
        best = t2;
        who = j2;
        if (kPath) place = p2;
      }
    }
    if (best < (double)(k0 + kRayWaveSteps) * dt) break;
  }
}

// The two tests a leg passes before it is walked (k_rays_check for leg 0, k_ray_paths for a later one).  The domain: the
// end point fl(o + fl(max_t d)) fails pairs_outside's rule with s, the count's radius, or is not finite ...
__device__ __forceinline__ bool ray_end_outside(XY o, XY d, double max_t, double s) {
  const double ex = fabs(o.x + max_t * d.x), ey = fabs(o.y + max_t * d.y);
  return !(ex / s < kPairsDomain) | !(ey / s < kPairsDomain);  // (inf too; no branch between the axes)
}

// ... and the range: up to t_end = min(max_t, the nearest wall's tw) the walk would take more than kRayMaxSteps steps.
__device__ __forceinline__ bool ray_too_long(double dt, double max_t, double tw) {
  return (double)kRayMaxSteps * dt <= fmin(max_t, tw);
}

// What a ray's wave begins with: lane 0 of ray 0 writes the ray count -- or, with a flag up, the status, which is then all
// that is written.  Is ray r to be done?
template <bool batched>
__device__ __forceinline__ bool ray_begin(const PairsView& v, const int* own_flag, long long r, int lane, long long n_rays,
                                          long long* counts) {
  const bool up = *v.flag || *own_flag;
  if (r == 0 && lane == 0) {
    if (up) counts[1] = ray_status<batched>(*v.flag, *own_flag);
    else counts[0] = n_rays;
  }
  return !up && r < n_rays;
}

// The result of a live ray from its nearest wall (tw, sw) and its nearest disc (td, jd): a wall wins a tie.
__device__ __forceinline__ void ray_write(const RayOut& out, long long r, double tw, int sw, double td, int jd) {
  const bool disc = td < tw;
  out.t[r] = disc ? td : tw;
  out.hit[r] = disc ? (long long)jd : sw >= 0 ? -2LL - sw : -1LL;
}

// After k_reader_check on the same stream, when discs are looked for: what only the rays can say.
__global__ void __launch_bounds__(kBlock)
    k_rays_check(double radius, RayWalls walls, double max_t, const XY* __restrict__ origins, const XY* __restrict__ dirs,
                 long long n_rays, int* __restrict__ own_flag) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const XY o = origins[r], d = dirs[r];
  double a;
  if (!ray_live(o, d, a)) return;
  if (ray_end_outside(o, d, max_t, radius)) atomicOr(own_flag, kReaderFlagDomain);
  double tw;
  int sw;
  ray_walls(walls, o, d, max_t, tw, sw);
  const double dt = radius / sqrt(a);
  if (ray_too_long(dt, max_t, tw)) atomicOr(own_flag, kRayFlagRange);
}

// A wave per ray: workgroup r is ray r, and a ray is one leg.  Every lane computes the ray and its walls (uniform: scalar
// work).  `discs` 0: walls alone.  v.g.radius is the count's.  Batched: the ray's record (lo, hi, cloud) comes from
// pairs_row over query_ptr -- the rays are queries --, uniform over the wave and so scalar work.  `who` stays global.
template <bool batched>
__global__ void __launch_bounds__(kRayBlock)
    k_rays(PairsView v, RayWalls walls, int discs, double rho2, double max_t, const int* __restrict__ own_flag,
           const XY* __restrict__ origins, const XY* __restrict__ dirs, long long n_rays, RayOut out) {
  const long long r = blockIdx.x;
  const int lane = (int)threadIdx.x;
  if (!ray_begin<batched>(v, own_flag, r, lane, n_rays, out.counts)) return;
  const XY o = origins[r], d = dirs[r];
  double a;
  if (!ray_live(o, d, a)) {
    if (lane == 0) {
      out.t[r] = __builtin_nan("");
      out.hit[r] = -1;
    }
    return;
  }
  double tw, best = __builtin_inf();
  int sw, who = kRayNoDisc, place = 0;  // (the place is a path's)
  ray_walls(walls, o, d, max_t, tw, sw);
  if (discs)
    ray_walk<batched, false>(v, pairs_row<batched>(v.bt, r), o, d, a, rho2, max_t, tw, v.g.radius / sqrt(a), false,
                             -1, best, who, place);
  if (lane == 0) ray_write(out, r, tw, sw, best, who);
}

// ---- ray paths (sc_pairs_ray_paths_device): the ray stays in its wave, leg after leg ---------------

constexpr int kRayMaxLegs = 16;  // bounces 0 .. 15 (include/sandcrate_hip.h: SC_RAY_MAX_BOUNCES + 1)
constexpr long long kRayEndNothing = 1, kRayEndDead = 2;  // `end`; 0: every leg hit; kPairsStatusDomain, kRayStatusRange

struct RayPathOut {
  double* t;       // n_rays x legs
  long long* hit;  // n_rays x legs
  XY* points;      // n_rays x legs
  XY* normals;     // n_rays x legs
  long long* end;  // n_rays
  long long* counts;  // [2]: rays, status
};

__device__ __forceinline__ void ray_path_write(const RayPathOut& out, long long at, double t, long long hit, XY p, XY n) {
  out.t[at] = t;
  out.hit[at] = hit;
  out.points[at] = p;
  out.normals[at] = n;
}

// A wave per ray, as k_rays: workgroup r is ray r, and the leg loop runs here.  Every lane holds the leg -- o, d, a, the
// budget m and the excluded wall and disc -- and computes the walls, the normal, the reflection and the tests of the next
// leg: all uniform over the wave.  Every leg is walked by ray_walk, from step 0 with the leg's own dt.  Lane 0 writes the
// legs; the lanes share the rows the path never reached.  Leg 0's own domain and range are the call's (the flags); a
// later leg's end the ray only.  Batched: the ray's record once, before leg 0, as in k_rays; every leg stays in the
// ray's cloud.
template <bool batched>
__global__ void __launch_bounds__(kRayBlock)
    k_ray_paths(PairsView v, RayWalls walls, int discs, double rho2, double max_t, int legs, const int* __restrict__ own_flag,
                const XY* __restrict__ origins, const XY* __restrict__ dirs, long long n_rays, RayPathOut out) {
  const long long r = blockIdx.x;
  const int lane = (int)threadIdx.x;
  if (!ray_begin<batched>(v, own_flag, r, lane, n_rays, out.counts)) return;
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  const XY none{nan, nan};
  const long long row = r * legs;
  XY o = origins[r], d = dirs[r];
  double a, m = max_t;
  int skip_wall = -1, skip_disc = -1;  // (no wall and no disc has these indices)
  long long end = 0;
  int leg = 0;
  const PairsRow rec = pairs_row<batched>(v.bt, r);  // the ray's cloud
  if (!ray_live(o, d, a)) end = kRayEndDead;
  while (end == 0 && leg < legs) {
    double tw, best = inf;
    int sw, who = kRayNoDisc, place = 0;
    ray_walls<true>(walls, o, d, m, tw, sw, skip_wall);
    if (discs) {
      const double dt = v.g.radius / sqrt(a);
      if (ray_too_long(dt, m, tw)) {  // (never leg 0: k_rays_check has raised the flag for it)
        end = kRayStatusRange;
        break;
      }
      ray_walk<batched, true>(v, rec, o, d, a, rho2, m, tw, dt, leg > 0, skip_disc, best, who, place);
    }
    const bool disc = best < tw;  // (a wall wins a tie)
    if (!disc && sw < 0) {
      if (lane == 0) ray_path_write(out, row + leg, inf, -1, none, none);
      ++leg;
      end = kRayEndNothing;
      break;
    }
    const double t = disc ? best : tw;
    const XY p{o.x + t * d.x, o.y + t * d.y};
    XY n;
    if (disc) {
      const XY c = v.sxy[place];
      const double gx = p.x - c.x, gy = p.y - c.y;
      const double len = sqrt(gx * gx + gy * gy);
      n = XY{gx / len, gy / len};
    } else {
      const double ex = walls.s[sw][2] - walls.s[sw][0], ey = walls.s[sw][3] - walls.s[sw][1];
      const double len = sqrt(ex * ex + ey * ey);
      n = XY{ey / len, -ex / len};
      if (d.x * n.x + d.y * n.y > 0) n = -n;  // the side the ray came from
    }
    if (lane == 0) ray_path_write(out, row + leg, t, disc ? (long long)who : -2LL - sw, p, n);
    ++leg;
    if (!(fabs(n.x) < inf && fabs(n.y) < inf)) {
      end = kRayEndDead;
      break;
    }
    if (leg == legs) break;
    // the next leg, and whether it may be walked
    const double dn = d.x * n.x + d.y * n.y;
    if (dn < 0) {
      const double k2 = 2.0 * dn;
      d = XY{d.x - k2 * n.x, d.y - k2 * n.y};
    }
    o = p;
    m = m - t;
    skip_wall = disc ? -1 : sw;
    skip_disc = disc ? who : -1;
    if (!ray_live(o, d, a)) {
      end = kRayEndDead;
    } else if (discs) {
      const double s = v.g.radius;
      if (!(fabs(o.x) / s < kPairsDomain) || !(fabs(o.y) / s < kPairsDomain) || ray_end_outside(o, d, m, s))
        end = kPairsStatusDomain;
    }
  }
  // the legs the path never reached -- for a dead ray all of them: its leg 0 is t = NaN, hit = -1 as well
  for (int k = leg + lane; k < legs; k += kRayBlock) ray_path_write(out, row + k, nan, -1, none, none);
  if (lane == 0) out.end[r] = end;
}

}  // namespace sc
