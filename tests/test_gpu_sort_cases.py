"""The sort chain (k_scan_cells, k_scatter, k_sort_big, k_reorder) on the worlds of tests/sort_cases.py, on both of its
routes, tapped between step_begin and step_finish.  What each world is for, and that a tick with dt = 0 changes nothing:
tests/test_sort_cases_cpu.py.

  plain     a fresh context: the first tick sees the state -- k_scatter<false>, no k_sort_big, K4 ranks every bucket itself
  sorting   the hint is up (one tick of sort_cases.prime, then the world is uploaded): k_scatter<true>, k_sort_big, K4 ranks
            from the sorted chunks
  promised  sorting, and the tick was promised by its predecessor (Engine.tick(now, now)): its bucket counts come from
            pass B's epilogue

The route is asserted: k_sort_big shares the scan's timing bracket, so "cell_scan" counts 1 launch on the plain route and 2
on the other two.  Rows, sorted ids and wall-fixed positions are compared exactly; the velocities K4 moved come back byte
for byte (dt = 0); wall_pile's tick is compared with the oracle's within test_ticks_match_oracle's tolerances.
(A promised tick's wall pass has run before the tap: there the wall-fixed positions are the ones downloaded before it.)"""
import copy
import time

import numpy as np
import pytest

import gpu_support as U
import recovery_cases as rc
import sort_cases as cases

pytestmark = pytest.mark.gpu

ORACLE = rc.oracle(rc.PILE_COEF)  # (built before any crate, as in test_gpu_recovery)
ROUTES = {"plain": 1, "sorting": 2, "promised": 2}  # -> launches in the "cell_scan" bracket of the tapped tick


@pytest.fixture(scope="module")
def lib():
    import torch
    torch.cuda.init()  # torch's HIP runtime must come up before the library's in a process that uses both
    import sand_crate_amd
    return sand_crate_amd


def make_crate(lib, name):
    from sand_crate_amd.load_config import WorldConfig
    (p, _, _), d = cases.world(name)
    wc = WorldConfig([copy.deepcopy(rc.BOX)], [], copy.deepcopy(cases.coef_of(name)))
    crate = lib.Crate(wc, noise="none", capacity=len(p) + 64)
    assert crate.particle_radius == d / 2
    crate.engine.enable_timing(True)
    return crate


def wall_fixed(p, r):
    from oracle.tick import hard_wall_fix, wall_contacts
    V, u, _ = wall_contacts(p, ORACLE.segments, ORACLE.body_states(), r)
    return hard_wall_fix(p, V, u, r)


def bring_to_route(crate, name, route):
    """-> the state (p, v, ids) the tapped tick starts from, and whether its positions are what the wall fix leaves."""
    (p, v, ids), d = cases.world(name)
    eng = crate.engine
    if route != "plain":
        eng.upload_with_ids(*cases.prime(d))
        eng.tick(crate._pack_tick_inputs())
        eng.synchronize()  # the hint is written by that tick's K4
    eng.upload_with_ids(p, v, ids)
    if route != "promised":
        crate._send_tick_inputs()
        return (p, v, ids), name != "wall_pile"  # (elsewhere nobody is within 1.2 r of a wall: the fix has nothing to move)
    now = crate._pack_tick_inputs()
    eng.tick(now, now)  # ... whose pass B has run the wall pass and the bucket counts of the tick that is tapped
    gp, gv, _, gids = eng.download()
    if name != "wall_pile":  # no time has passed
        order = np.argsort(ids)
        U.same_bytes(gp, p[order])
        U.same_bytes(gv, v[order])
    return (gp, gv, gids), True


def tap(crate, state, fixed_already, route, neighbors=True):
    """One tick, tapped.  -> what the engine downloads after it (None without `neighbors`: the sort tap alone)."""
    p, v, ids = state
    d = crate.particle_radius * 2
    eng = crate.engine
    q = p if fixed_already else wall_fixed(p, d / 2)
    order = cases.reference_order(q, ids, d)
    eng.reset_timing()
    eng.step_begin()
    rows, sorted_ids = eng.download_sort()
    fixed_xy = eng.download_neighbors()[3] if neighbors else None
    eng.step_finish()
    got = eng.download() if neighbors else eng.synchronize()
    launches = eng.timing()["cell_scan"][1]
    assert launches == ROUTES[route], f"the tick ran the other route: {launches} launches in the scan's bracket"
    assert np.array_equal(rows, np.floor(q[order, 1] / d).astype(np.int64))
    assert np.array_equal(sorted_ids, ids[order])
    if neighbors:
        U.same_bytes(fixed_xy, q[order])
    return got


def check_world(lib, name, route):
    crate = make_crate(lib, name)
    state, fixed_already = bring_to_route(crate, name, route)
    got = tap(crate, state, fixed_already, route)
    p, v, ids = state
    by_id = np.argsort(ids)
    assert np.array_equal(got[3], ids[by_id])
    if name == "wall_pile":
        from oracle.tick import tick_core
        from test_gpu_recovery import assert_tick
        # the oracle breaks ties in x by the index, as the reference does, and the kernels by the id, which is the index there:
        # it is given the state in id order (hundreds of the pile's particles stand on x = r exactly, and which twenty
        # neighbours a list keeps hangs on their order)
        with np.errstate(all="ignore"):
            out = tick_core(p[by_id], v[by_id], ORACLE.segments, ORACLE.body_states(), ORACLE.coef)
        assert out["wall_count"].sum() > 1500 and out["pressure"].max() > 1.0  # wall slots and a pile's pressures
        assert_tick(got, out, ids[by_id])
    else:  # no forces, no time: what K4 moved to the sorted arrays is what comes back
        U.same_bytes(got[0], p[by_id])
        U.same_bytes(got[1], v[by_id])
    crate.engine.close()


@pytest.mark.parametrize("route", ["plain", "sorting"])
@pytest.mark.parametrize("name", ["ladder", "ends", "scan_neighbours", "table_collisions", "wall_pile"])
def test_sort_chain_on_both_routes(lib, name, route):
    check_world(lib, name, route)


@pytest.mark.parametrize("name", ["ladder", "table_collisions", "wall_pile"])
def test_sort_chain_of_a_promised_tick(lib, name):
    check_world(lib, name, "promised")


def test_more_tasks_than_the_list_holds(lib):
    """overflow: 16,390 tasks for a list of kMaxSortTasks = 16,384.  The buckets the list's end falls on get no-op tasks and
    no stamp, and K4 ranks them by counting -- whichever they are: the order of the scan's atomics decides.  The sorting
    route and the sort tap only."""
    t0 = time.perf_counter()
    crate = make_crate(lib, "overflow")
    state, _ = bring_to_route(crate, "overflow", "sorting")
    t1 = time.perf_counter()
    tap(crate, state, True, "sorting", neighbors=False)
    t2 = time.perf_counter()
    ms = crate.engine.timing()
    print(f"overflow: world, context and upload {t1 - t0:.2f} s, tapped tick with its reference order {t2 - t1:.2f} s; "
          f"scan + k_sort_big {ms['cell_scan'][0]:.3f} ms, K4 {ms['reorder'][0]:.3f} ms")
    crate.engine.close()
