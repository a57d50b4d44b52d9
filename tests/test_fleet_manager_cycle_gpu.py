"""replan.manager_cycle on a small scene: a resident map of 128 x 128 cells at 0.1 m, max_replan_time 0.5, replan_time 1.0, four robots,
13 periods 0.25 s apart with alore_nmpc_refs_promote between them.  Nothing is read back during the run: every period's slabs are
copied into device-side histories in stream order and compared afterwards.
  A  a free run of 3 m: a FRESH plan delivered with start time now, REPLAN deliveries with exactly now + 0.5
  B  its goal walled in by painted cells: no path, EMERGENCY_STOP, nothing delivered, its store slots invalid (stop_on_no_path = 1)
  C  0.95 m from its goal: FRESH, GOINGTOGOAL at the first cycle after replan_time, IDLE once its duration has passed
  D  no request: all of its words stay as they were
The state sequence of every robot is the oracle's (tests/fleet_manager_cases.py) fed with the statuses the device produced."""
import numpy as np
import pytest

from tests import fleet_manager_cases as cases

pytestmark = pytest.mark.gpu

NB, K, T0, DTICK = 4, 13, 10.0, 0.25
A, Bw, Cn, D = 0, 1, 2, 3
NX, LO, RES = 128, -6.4, 0.1
PARAMS = dict(replan_time=1.0, max_replan_time=0.5, replan_on_collision_only=0, stop_inside_obstacle=0, stop_on_no_path=1)
START = np.array([[-1.5, -2.5, 0.0], [-1.5, 2.5, 0.0], [-0.5, 0.0, 0.0], [3.0, 4.5, 0.0]])
GOAL = np.array([[1.5, -2.5, 0.0], [1.5, 2.5, 0.0], [0.45, 0.0, 0.0], [0.0, 0.0, 0.0]])


def scene_grid():
    c = (np.arange(NX) + 0.5) * RES + LO
    d = np.maximum(np.abs(c[:, None] - GOAL[Bw, 0]), np.abs(c[None, :] - GOAL[Bw, 1]))
    g = np.ones((NX, NX), np.uint8)
    g[(d > 0.75) & (d < 1.05)] = 2                         # a square wall three cells thick round B's goal
    return g


def view(address, shape, typestr):
    import torch
    from alore_legged_manipulator_amd.backend import _DeviceArray
    return torch.as_tensor(_DeviceArray(address, shape, typestr), device="cuda")


@pytest.fixture(scope="module")
def run():
    import torch
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    from alore_legged_manipulator_amd.nmpc import BatchedNmpc
    from alore_legged_manipulator_amd.replan import ManagerWork, manager_cycle
    pl = BatchedMSPlanner(NB, 16)
    pl.map_create(NX, NX, LO, LO, RES, detection_range=7.0, perspective=0)
    pl.map_set_grid(scene_grid())
    pl.map_update_esdf((0.0, 0.0))
    pl.manager_create(**PARAMS)
    eng = BatchedNmpc(NB, 20, 0.01)
    eng.refs_init(max_pieces=16, max_checkpoints=128)
    req = np.array([1, 1, 1, 0], np.int32)
    pl.manager_request(START, GOAL, req)
    first = pl.get_manager(NB)
    poses = torch.as_tensor(START).cuda()
    w = ManagerWork(pl, NB)
    mv, dv, pv = pl.manager_view(), pl.device_view(), eng.refs_pending_view()
    P = pl.P
    src = dict(ints=view(mv.state, (11 * NB + 8,), "<i4"), doubles=view(mv.goal, (14 * NB,), "<f8"), search=w.search_status, build=w.build_status,
               ok=view(dv.ok, (NB,), "<i4"), n_pieces=view(dv.n_pieces, (NB,), "<i4"), T=view(dv.T, (NB, P), "<f8"), xytheta=w.xytheta,
               promotions=view(pv.promotions, (NB,), "<i4"), pending_status=view(pv.status, (NB,), "<i4"),
               pending_meta=view(pv.pending_meta, (NB, 8), "<f8"), active_meta=view(pv.active_meta, (NB, 8), "<f8"))
    hist = {k: torch.zeros((K,) + tuple(v.shape), dtype=v.dtype, device="cuda") for k, v in src.items()}
    promoted_before = torch.zeros((K, NB), dtype=torch.int32, device="cuda")
    for k in range(K):
        now = T0 + DTICK * k
        eng.refs_promote(now)
        promoted_before[k].copy_(src["promotions"])
        manager_cycle(pl, eng, now, poses, work=w, nmpc_plant=False)
        for name, v in src.items():
            hist[name][k].copy_(v)
    torch.cuda.synchronize()                                # the only wait: after the run
    out = {k: v.cpu().numpy() for k, v in hist.items()}
    out.update(first=first, promoted_before=promoted_before.cpu().numpy(), now=np.array([T0 + DTICK * k for k in range(K)]), req=req)
    return out


def test_the_state_sequences_are_the_oracles(run):
    fleet = cases.Fleet(NB, PARAMS)
    fleet.request(START, GOAL, run["req"])
    same0 = (run["first"]["ints"], run["first"]["doubles"], np.zeros(8, np.int32))
    cases.same(same0, fleet.snapshot(), "after the request")
    poses = START
    for k in range(K):
        fleet.begin(run["now"][k], poses)
        fleet.starts(run["xytheta"][k], np.zeros((NB, 3)), np.zeros((NB, 3)))
        fleet.end(run["search"][k], run["build"][k], run["ok"][k], run["T"][k], run["n_pieces"][k])
        got = (run["ints"][k][:11 * NB].reshape(11, NB), run["doubles"][k].reshape(14, NB), run["ints"][k][11 * NB:])
        cases.same(got, fleet.snapshot(), ("period", k))
    states = run["ints"][:, :NB]
    print("states", states.T.tolist(), "durations", run["doubles"][:, 12 * NB:13 * NB].max(0))
    assert states[0].tolist() == [cases.PLANNING, cases.EMERGENCY_STOP, cases.PLANNING, cases.IDLE]
    # C: FRESH, GOINGTOGOAL at the first cycle after replan_time (period 5: 1.25 s > 1.0 s), IDLE once its duration has passed
    assert (states[:5, Cn] == cases.PLANNING).all() and states[5, Cn] == cases.GOINGTOGOAL and states[-1, Cn] == cases.IDLE
    total = run["doubles"][0].reshape(14, NB)[12, Cn]
    gone = int(np.argmax(states[:, Cn] == cases.IDLE))
    assert gone >= 6 and run["now"][gone] - T0 >= total                    # period 5 returns before the finish rule: 6 at the earliest
    assert gone == 6 or run["now"][gone - 1] - T0 < total
    # A replans at period 5 (and, while it still has a goal, every 1.25 s after)
    assert run["ints"][5][4 * NB + A] == cases.REPLAN_ACTION and states[5, A] == cases.REPLAN
    assert {"fresh", "replan", "going_by_distance", "no_path_with_stop", "going_to_idle"} <= fleet.events


def test_deliveries_carry_the_start_times_of_the_reference(run):
    fresh, replan = run["ints"][:, 7 * NB:8 * NB], run["ints"][:, 8 * NB:9 * NB]
    assert fresh[0].tolist() == [1, 0, 1, 0] and not fresh[1:].any()
    assert replan[5, A] == 1 and not replan[:, [Bw, Cn, D]].any()
    for k in range(K):
        for b in range(NB):
            if fresh[k, b] or replan[k, b]:
                meta = run["pending_meta"][k, b]
                assert meta[6] == 1.0 and meta[0] == (run["now"][k] if fresh[k, b] else run["now"][k] + 0.5), (k, b, meta[0])
                assert run["pending_status"][k, b] == 0
    # every promotion happens in front of the first period whose time exceeds the start time
    expect = np.zeros(NB, int)
    waiting = {}
    for k in range(K):
        for b in list(waiting):
            if run["now"][k] > waiting[b]:
                expect[b] += 1
                del waiting[b]
        assert run["promoted_before"][k].tolist() == expect.tolist(), k
        for b in range(NB):
            if fresh[k, b] or replan[k, b]:
                assert b not in waiting
                waiting[b] = run["pending_meta"][k, b, 0]
    assert expect[A] >= 2 and expect[Cn] == 1 and expect[Bw] == 0 and expect[D] == 0


def test_the_walled_in_robot_stops_and_the_idle_one_is_untouched(run):
    assert (run["search"][0][[A, Cn]] == 0).all() and run["search"][0][Bw] == -4
    stop = run["ints"][:, 9 * NB:10 * NB]
    assert stop[0].tolist() == [0, 1, 0, 0] and not stop[1:].any()
    assert not run["pending_meta"][:, Bw, 6].any() and not run["active_meta"][:, Bw, 6].any() and (run["pending_status"][:, Bw] == 1).all()
    assert not run["promotions"][:, [Bw, D]].any()
    first_i, first_d = run["first"]["ints"], run["first"]["doubles"]
    for k in range(K):
        ints, dbl = run["ints"][k][:11 * NB].reshape(11, NB), run["doubles"][k].reshape(14, NB)
        assert np.array_equal(ints[:, D], first_i[:, D])
        assert dbl[:, D].tobytes() == first_d[:, D].tobytes()
    assert not run["pending_meta"][:, D].any() and not run["active_meta"][:, D].any() and (run["pending_status"][:, D] == 1).all()
