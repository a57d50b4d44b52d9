"""The ICR EKF kernels (csrc/icr_ekf.hip, through BatchedNmpc.ekf_step) against the sequential oracle, tests/icr_ekf_cases.py.

Every robot of a batch runs one group of the oracle's cases.  A call of ekf_step has ONE dt and either a pose for everybody or
for nobody, so step s of the groups is issued as one call per distinct (dt, pose given) among them, the robots of the other
groups masked out (which is also what tests the mask).  After every call status, x, P and conv_step of every robot are read back:
  * groups whose held wheel speeds are zero never multiply anything by sin or cos (update only): the bits of the oracle;
  * the others differ by what the device's sincos differs from libm: FORECAST_TOL, relative to max(1, |oracle|);
  * status and conv_step equal the oracle's; a robot whose step failed or was masked keeps the bits it had before the call."""
import numpy as np
import pytest

from tests import icr_ekf_cases as cases

pytestmark = pytest.mark.gpu

# Largest |device - oracle| / max(1, |oracle|) over all groups, measured on an MI355X (profiles/icr_ekf.txt): 3.941e-15.
# The bound is 16 times that (6.3e-14), rounded up to a power of ten; it may not exceed 1e-10 (a wrong term of J is orders above that).
MEASURED_FORECAST_ERR = 3.941e-15
FORECAST_TOL = 1e-13
assert 16 * MEASURED_FORECAST_ERR <= FORECAST_TOL <= 1e-10

SPECIAL = ("fail_singular_zero", "flags_standard_zero")                 # groups with parameters of their own
MAIN = [n for n in cases.NAMES if n not in SPECIAL]


def trig_free(name):
    g = cases.group(name)
    return g["init"].u == [0.0, 0.0] and all(s["wheel"] == [0.0, 0.0] for s in g["steps"][:-1])


def engine(B, prm):
    from alore_legged_manipulator_amd.nmpc import BatchedNmpc
    e = BatchedNmpc(B, 20, 0.01)
    e.refs_init(max_pieces=2, max_checkpoints=4)
    e.ekf_init(q=prm["q"], r=prm["r"], standard=prm["standard"])
    return e


def run_groups(names, B):
    """robot b runs group names[b % len(names)]; returns the largest relative error of the groups that are not trig-free"""
    import torch
    prm = cases.group(names[0])["prm"]
    assert all(cases.group(n)["prm"] == prm for n in names)
    eng = engine(B, prm)
    mine = [names[b % len(names)] for b in range(B)]
    groups = [cases.group(n) for n in mine]
    eng.ekf_reset(pose=np.zeros((B, 3)))
    eng.ekf_set_state(x=[g["init"].x for g in groups], P=[g["init"].P for g in groups], u=[g["init"].u for g in groups])
    state = eng.ekf_get()
    worst = 0.0
    for s in range(max(len(g["steps"]) for g in groups)):
        live = [b for b in range(B) if s < len(groups[b]["steps"])]
        keys = sorted({(groups[b]["steps"][s]["dt"], groups[b]["steps"][s]["z"] is not None) for b in live})
        for dt, has_z in keys:
            sel = [b for b in live if (groups[b]["steps"][s]["dt"], groups[b]["steps"][s]["z"] is not None) == (dt, has_z)]
            on = [b for b in sel if groups[b]["steps"][s]["mask"] in (None, 1)]
            wheel, meas, mask = np.zeros((B, 2)), np.zeros((B, 3)), np.zeros(B, np.uint8)
            mask[on] = 1
            for b in sel:
                wheel[b] = groups[b]["steps"][s]["wheel"]
                if has_z:
                    meas[b] = groups[b]["steps"][s]["z"]
            eng.ekf_step(torch.from_numpy(wheel).cuda(), dt, torch.from_numpy(meas).cuda() if has_z else None, torch.from_numpy(mask).cuda())
            got = eng.ekf_get()
            for b in range(B):
                if b not in on:
                    assert got["status"][b] == cases.MASKED, (mine[b], s)
                else:
                    st, f = cases.expected(mine[b])[s]
                    assert got["status"][b] == st, (mine[b], s, got["status"][b], st)
                    assert got["conv_step"][b].tolist() == f.conv_step, (mine[b], s)
                    if st == cases.OK:
                        want = np.array(f.x + f.P)
                        have = np.concatenate([got["x"][b], got["P"][b].reshape(-1)])
                        if trig_free(mine[b]):
                            assert have.tobytes() == want.tobytes(), (mine[b], s, np.max(np.abs(have - want)))
                        else:
                            worst = max(worst, float(np.max(np.abs(have - want) / np.maximum(1.0, np.abs(want)))))
                if got["status"][b] != cases.OK:        # failed or masked: the bits it had
                    assert got["x"][b].tobytes() == state["x"][b].tobytes() and got["P"][b].tobytes() == state["P"][b].tobytes(), (mine[b], s)
            state = got
    eng.close()
    return worst


def test_b70_every_group_against_the_oracle():
    worst = run_groups(MAIN, 70)
    print("forecast: largest |device - oracle| / max(1, |oracle|) = %.3e (bound %.0e)" % (worst, FORECAST_TOL))
    assert worst < FORECAST_TOL, worst


@pytest.mark.parametrize("name", ["random0", "update_only1", "turns-3", "fail_D", "masks", "flags_run12", "fail_singular_zero", "flags_standard_zero"])
def test_b1_one_group_against_the_oracle(name):
    worst = run_groups([name], 1)
    assert worst < FORECAST_TOL, worst


def test_the_update_only_groups_are_compared_for_bits():
    free = [n for n in cases.NAMES if trig_free(n)]
    assert all(n in free for n in cases.NAMES if n.startswith(("update_only", "turns", "flags", "fail_meas_far")))
    assert not any(n in free for n in cases.NAMES if n.startswith("random"))


@pytest.mark.parametrize("odom_every", [1, 10])
def test_open_loop_rollouts_on_the_device(odom_every):
    """the 3000-step rollouts of tests/test_icr_ekf_cpu.py through ekf_step, three robots (one per true ICR): the final x within
    1e-6 of the oracle's (the project's figure for device-against-host routes), and every ICR error below half of its start"""
    import torch
    K = len(cases.TRUE_ICRS)
    eng = engine(K, cases.DEFAULT)
    eng.ekf_reset(pose=np.zeros((K, 3)))
    ins = [cases.rollout_inputs(k) for k in range(K)]
    wheels = torch.from_numpy(np.array([[ins[k][0][t] for k in range(K)] for t in range(cases.ROLLOUT_STEPS)])).cuda()
    poses = torch.from_numpy(np.array([[ins[k][1][t] for k in range(K)] for t in range(cases.ROLLOUT_STEPS)])).cuda()
    for t in range(cases.ROLLOUT_STEPS):
        eng.ekf_step(wheels[t], cases.ROLLOUT_DT, poses[t] if (t + 1) % odom_every == 0 else None)
    got = eng.ekf_get()
    assert (got["status"] == 0).all()
    for k in range(K):
        f = cases.rollout(k, odom_every)
        assert np.max(np.abs(got["x"][k] - np.array(f.x))) < 1e-6, (k, got["x"][k], f.x)
        f.x = got["x"][k].tolist()
        ratios = cases.icr_error_ratios(f, k)
        assert all(r < 0.5 for r in ratios), (k, ratios)
    eng.close()
