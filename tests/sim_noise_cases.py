"""The oracle of csrc/sim_noise.h (counter-based normal draws) and of ltv_plant::step_noisy (the simulator's noisy PoseSub),
in plain Python: integers for Philox4x32-10, float64 scalars for the uniforms, Box-Muller and the plant.

A draw is a pure function of (seed, robot, event, stream): counter = (event lo, event hi, robot, stream), key = (seed lo, seed hi).
Uniforms: u = ((w_a >> 6) 2^26 + (w_b >> 6) + 0.5) 2^-52 from the word pairs (0, 1) and (2, 3) -- every term exact, u strictly
inside (0, 1).  (53 bits plus the half do not fit a double: with w_a >> 5 the all-one words round to u = 1.0, see
uniform_53bit below and the test that shows it.)"""
import math
from dataclasses import dataclass, field

import numpy as np

from tests import ltv_plant_cases as plant

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM_VEL, STREAM_MEAS_XY, STREAM_MEAS_TH = 0, 1, 2

# counter / key -> output (Random123's known answers for Philox4x32-10)
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox4x32(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return (c0, c1, c2, c3)


def words(seed, robot, event, stream):
    return philox4x32((event & MASK, (event >> 32) & MASK, robot & MASK, stream & MASK), (seed & MASK, (seed >> 32) & MASK))


def uniform(wa, wb):
    return (float(wa >> 6) * 67108864.0 + float(wb >> 6) + 0.5) * 2.0 ** -52


def uniform_53bit(wa, wb):
    """the 53-bit variant, as float64 evaluates it: NOT what the header does (it reaches 1.0)"""
    return (float(wa >> 5) * 67108864.0 + float(wb >> 6) + 0.5) * 2.0 ** -53


def box_muller(u1, u2):
    r = math.sqrt(-2.0 * math.log(u1))
    a = 6.28318530717958647692 * u2
    return r * math.cos(a), r * math.sin(a)


def normal2(seed, robot, event, stream):
    w = words(seed, robot, event, stream)
    return box_muller(uniform(w[0], w[1]), uniform(w[2], w[3]))


def random_keys(n=64, seed=11):
    """(seed, robot, event, stream) with every word exercised: 64-bit seeds and events, robots beyond 16 bits"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        out.append((int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 20)),
                    int(rng.integers(0, 2 ** 64, dtype=np.uint64)) if i % 2 else int(rng.integers(0, 1000)), int(rng.integers(0, 3))))
    return out


# ---- the noisy PoseSub: tests/ltv_plant_cases.plant_step with the noise of simulator.h:222-229
def plant_step_noisy(p, has_traj, at_goal, cmd, state, stddev, seed, robot, event):
    """one control period; state = [x, y, th, v, w, dv, dw] -> the new state.  v <- cmd.v, omega <- cmd.omega, then
    v += (v stddev) z0, omega += (omega stddev) z1; desired (follow = 1) takes the un-noised command."""
    x, y, th, v, w, dv, dw = (float(s) for s in state)
    if has_traj:
        cv, cw = (0.0, 0.0) if at_goal else (float(cmd[0]), float(cmd[1]))
        v, w = cv, cw
        if stddev > 0.0:
            z0, z1 = normal2(seed, robot, event, STREAM_VEL)
            v += (v * stddev) * z0
            w += (w * stddev) * z1
        if p.follow:
            dv, dw = cv, cw
    # the propagation steps are the un-noised plant's: a robot without a trajectory and the current velocities as the command
    q = plant.PlantParams(**dict(p.kw(), follow=0))
    return plant.plant_step(q, True, False, (v, w), [x, y, th, v, w, dv, dw])


@dataclass
class Scene:
    name: str
    params: plant.PlantParams
    has_traj: bool
    at_goal: bool
    cmd: tuple
    state: list
    stddev: float
    seed: int
    robot: int
    event: int
    ticks: int = 1                                 # event advances by one per tick
    want: list = field(default_factory=list)


def _scenes():
    out = []
    pose = [1.25, -0.75, 0.6]
    rest = pose + [0.0, 0.0, 0.0, 0.0]
    S = 0x1234567890ABCDEF
    for follow in (0, 1):
        # follow = 1 holds `desired` at the un-noised command, and a perturbation below the launch file's clamps (0.02, 0.04 per
        # substep) is gone after the first substep: those scenes take clamps a hundred times smaller, so that the noise shows
        p = plant.PlantParams(follow=1, max_acc=0.02, max_domega=0.04) if follow else plant.PlantParams()
        tag = f"follow{follow}"
        out.append(Scene(tag + "_sigma0", p, True, False, (0.5, 0.3), list(rest), 0.0, S, 3, 7))
        out.append(Scene(tag + "_sigma0_three_ticks", p, True, False, (1.1, 0.8), [-2.0, 3.0, -2.9, 0.4, 0.1, 0.0, 0.0], 0.0, S, 3, 7, ticks=3))
        out.append(Scene(tag + "_launch_noise", p, True, False, (0.5, 0.3), list(rest), 0.01, S, 3, 7))
        out.append(Scene(tag + "_launch_noise_three_ticks", p, True, False, (1.1, 0.8), [-2.0, 3.0, -2.9, 0.4, 0.1, 0.0, 0.0], 0.01, S, 3, 7, ticks=3))
        out.append(Scene(tag + "_large_noise", p, True, False, (0.9, -1.2), pose + [0.3, 0.2, 0.0, 0.0], 0.2, S, 0, 0))
        out.append(Scene(tag + "_at_goal", p, True, True, (0.9, 0.7), pose + [0.6, 0.5, 0.3, 0.1], 0.01, S, 5, 2))
        out.append(Scene(tag + "_no_trajectory", p, False, False, (0.9, 0.7), pose + [0.6, 0.5, 0.3, 0.1], 0.01, S, 5, 2))
        out.append(Scene(tag + "_v_negative", p, True, False, (-0.6, 0.4), list(rest), 0.05, S, 9, 4))
        out.append(Scene(tag + "_event_a", p, True, False, (0.8, 0.5), list(rest), 0.05, S, 12, 100))
        out.append(Scene(tag + "_event_b", p, True, False, (0.8, 0.5), list(rest), 0.05, S, 12, 101))
        out.append(Scene(tag + "_robot_a", p, True, False, (0.8, 0.5), list(rest), 0.05, S, 40, 2 ** 33 + 5))
        out.append(Scene(tag + "_robot_b", p, True, False, (0.8, 0.5), list(rest), 0.05, S, 41, 2 ** 33 + 5))
    out.append(Scene("euler_unicycle_noise", plant.PlantParams(state_propa_period=0.01, substeps=1, follow=1), True, False, (1.7, -0.9),
                     [9.5, -9.5, 3.0, 0.0, 0.0, 0.0, 0.0], 0.01, 1, 0, 0, ticks=2))
    for s in out:
        st = list(s.state)
        for t in range(s.ticks):
            st = plant_step_noisy(s.params, s.has_traj, s.at_goal, s.cmd, st, s.stddev, s.seed, s.robot, s.event + t)
        s.want = st
    return out


SCENES = _scenes()
TOL = plant.TOL     # 1e-12: the plant's bound; the noise adds two products of a value <= 3, stddev <= 0.2 and |z| < 8.6 known to 1e-13
TOL_NORMAL = 1e-13  # |z| <= sqrt(-2 ln 2^-53) < 8.6; the argument 2 pi u2 <= 6.3 carries one rounding of 9e-16, cos and sin are within
#                     about 1e-16, r within a few ulp: |dz| < 1e-14, with a tenfold margin
