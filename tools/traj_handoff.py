"""What the hand-over to a replanned trajectory costs (include/alore_nmpc.h: alore_nmpc_refs_set_pending_from_backend,
alore_nmpc_refs_promote; csrc/traj_handoff.hip).  python tools/traj_handoff.py [out.txt]

(a) the promotion kernel at 64 / 512 / 4096 robots with none, a quarter and all of the pending entries due (Monte-Carlo plans of
    tools' other rows: monte_carlo_goals(seed 44), 16-piece handle), device time between two events, median of 30;
(b) refs_set_pending_from_backend against refs_set_from_backend for the same plans: time until the host returns and device time;
(c) alore_nmpc_closed_loop_run over 100 ticks at 4096 robots, alternating in one process: no pending entry / one hand-over of every
    robot in the middle of the run (the pending entries are written before the timed region; the run is cut once); store, plant
    and iterate are put back before every timed run, so that all runs do the same work;
(d) replan_cycle (alore_legged_manipulator_amd/replan.py) on the scene of tools/path_search.py: 8192 Monte-Carlo plans tracked from
    t = 0, discs appear in the start area, one cycle at now = 0.3 with max_replan_time = 0.2: time until the host returns and
    device time per step (an event after every step), on fresh handles after a warm-up cycle on other handles.
The comparison of the no-pending run with the parent commit is not in this tool: it needs a second build (profiles/traj_handoff.txt
says how it was made)."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alore_legged_manipulator_amd.backend import BatchedMSPlanner
from alore_legged_manipulator_amd.flat_traj import monte_carlo_goals
from alore_legged_manipulator_amd.nmpc import BatchedNmpc

N, DT, REPS = 20, 0.01, 30


def timed(fn, before=None):
    """(host microseconds until fn returns, device microseconds), medians of REPS after 3 warm-up rounds"""
    host, dev = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(REPS + 3):
        if before:
            before()
        torch.cuda.synchronize()
        e0.record()
        t = time.perf_counter()
        fn()
        h = time.perf_counter() - t
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            host.append(h * 1e6)
            dev.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(host), statistics.median(dev)


def fleet(B):
    fts = monte_carlo_goals(B, seed=44)
    pl = BatchedMSPlanner(B, 16)
    pl.set_free_map(half=20.0)
    pl.set_problems(fts)
    pl.plan()
    res = pl.results()
    eng = BatchedNmpc(B, N, DT, diagnostics=False)
    eng.load({"W": np.tile(np.diag([10, 10, 0.5, 0.1, 0.1]).astype(np.float32), (B, N, 1, 1)),
              "WN": np.tile(np.diag([10, 10, 0.5]).astype(np.float32), (B, 1, 1))})
    eng.refs_init(max_pieces=16, max_checkpoints=128)
    eng.refs_set_from_backend(pl)
    pieces = np.asarray(res["T"] > 0).sum(1)
    return pl, eng, fts, (int(res["ok"].sum()), float(pieces.mean()))


def cycle(say):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from flat_traj_build import goals_as_paths
    from path_search import LO, NX, NY, RES, disc_map
    from alore_legged_manipulator_amd.replan import ReplanWork, replan_cycle
    B = 8192
    xy, sy, ey = goals_as_paths(B)
    d_n = torch.full((B,), 2, dtype=torch.int32, device="cuda")
    d_xy, d_sy, d_ey = torch.from_numpy(xy).cuda(), torch.from_numpy(sy).cuda(), torch.from_numpy(ey).cuda()
    d_goal = torch.from_numpy(np.ascontiguousarray(xy[:, 1])).cuda()
    dist = disc_map()

    def setup():
        pl = BatchedMSPlanner(B, 16)
        pl.set_map(np.full((NX, NY), 100.0), LO, LO, RES)
        pl.set_paths_device(B, 3, d_n, d_xy, d_sy, d_ey)
        pl.plan()
        eng = BatchedNmpc(B, N, DT, diagnostics=False)
        eng.refs_init(max_pieces=16, max_checkpoints=160)
        eng.refs_set_from_backend(pl)
        eng.refs_pending_view()                               # allocates the pending store: not part of a cycle
        pl.set_map(dist, LO, LO, RES)
        return pl, eng, ReplanWork(B)

    names, rows = [], []
    for timed_round in (False, True, True, True):              # the first round loads the kernels
        pl, eng, work = setup()
        ev = [torch.cuda.Event(enable_timing=True)]
        names = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)
            names.append(name)
        torch.cuda.synchronize()
        ev[0].record()
        t = time.perf_counter()
        replan_cycle(pl, eng, 0.3, 0.2, d_goal, d_ey, start_times=0.0, work=work, mark=mark)
        host = (time.perf_counter() - t) * 1e6
        torch.cuda.synchronize()
        if timed_round:
            rows.append([host] + [ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(len(names))])
        mask = work.mask.cpu().numpy()
        st = eng.refs_pending_status()
        eng.close()
    r = np.median(np.array(rows), 0)
    say("  (d) replan_cycle, %d plans, %d delivered (pending entries valid: %d; status words below 0: %d), medians of %d fresh rounds:"
        % (B, int(mask.sum()), int(st["valid"].sum()), int((st["status"] < 0).sum()), len(rows)))
    say("      host returns after %8.1f us (rounds: %s)" % (r[0], " ".join("%.0f" % x[0] for x in rows)))
    for k, name in enumerate(names):
        say("      device, %-16s %9.1f us" % (name, r[1 + k]))
    say("      device, whole cycle      %9.1f us" % float(r[1:].sum()))


def main(out):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("hand-over to a replanned trajectory: medians of %d, microseconds" % REPS)
    for B in (64, 512, 4096):
        pl, eng, fts, (n_ok, mean_pieces) = fleet(B)
        say("B = %d (%d plans ok, %.1f pieces on average)" % (B, n_ok, mean_pieces))
        for name, due in (("none", 0), ("a quarter", B // 4), ("all", B)):
            mask = torch.zeros(B, dtype=torch.int32, device="cuda")
            mask[:due] = 1
            # entries of the first `due` robots start at 1.0, the others at 3.0; promoted at 2.0
            def fill():
                eng.refs_promote(10.0)
                eng.refs_set_pending_from_backend(pl, mask=1 - mask, traj_start_time=3.0)
                eng.refs_set_pending_from_backend(pl, mask=mask, traj_start_time=1.0)
            _, d = timed(lambda: eng.refs_promote(2.0), before=fill)
            say("  (a) promotion, %-9s due: device %7.1f" % (name, d))
        h0, d0 = timed(lambda: eng.refs_set_from_backend(pl))
        h1, d1 = timed(lambda: eng.refs_set_pending_from_backend(pl, traj_start_time=1.0), before=lambda: eng.refs_promote(10.0))
        say("  (b) refs_set_from_backend          host %7.1f  device %7.1f" % (h0, d0))
        say("      refs_set_pending_from_backend  host %7.1f  device %7.1f   (forced-promotion launch included, nothing pending)" % (h1, d1))
        if B == 4096:
            pose0 = np.array([ft.start_xytheta for ft in fts])
            icr = np.tile([0.1, -0.3, 0.3], (B, 1))
            eng.plant_init()
            t0 = 0.06

            def reset():                                        # every timed run does the same work: same store, same start
                eng.refs_promote(1e9)
                eng.refs_set_from_backend(pl)
                eng.plant_set_state(pose0, icr)
                eng.closed_loop_reset()
                eng.closed_loop_tick(0.05, delay_num=1)

            def reset_and_pend():
                reset()
                eng.refs_set_pending_from_backend(pl, traj_start_time=t0 + 49.5 * DT)

            def run():
                eng.closed_loop_run(t0, DT, 100, delay_num=1)

            plain, handed = [], []
            for _ in range(6):                                  # alternating in one process
                plain.append(timed(run, before=reset)[1])
                handed.append(timed(run, before=reset_and_pend)[1])
            say("  (c) closed_loop_run, 100 ticks: no pending entry %8.1f per run (rounds: %s)" % (statistics.median(plain), " ".join("%.0f" % x for x in plain)))
            say("      one hand-over of all robots at tick 50      %8.1f per run (rounds: %s)" % (statistics.median(handed), " ".join("%.0f" % x for x in handed)))
            say("      difference %+.1f us per run: the promotion (a), the end of the first part (plant step, copy back of y / yN), the whole sampling"
                % (statistics.median(handed) - statistics.median(plain)))
            say("      of the second part's first tick -- and other work for the solver, which tracks the new plans from their start after tick 50")
        eng.close()
    cycle(say)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
