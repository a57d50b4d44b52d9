"""Oracle and scenarios of the fleet's plan_manager state machine (csrc/fleet_manager.h, alore_backend_manager_*).

The oracle is a sequential restatement, robot by robot, of the reference's start_callback / goal_callback
(plan_manager.hpp:434-468) and PlanManager::MainThread (:556-712) with the collision stop of PlanTester::MainThread
(plan_tester.hpp:529-541) in front.  Python floats are IEEE doubles and every operation below is one correctly rounded double
operation in the reference's order, so the header (built without contraction) and the kernels must give the same BITS.

The scenario generator scripts B robots x K ticks.  Robot b plays ROLES[b % len(ROLES)]; the seed chooses the manager's parameters
(SEED_PARAMS) and jitters everything that decides no branch.  Tick times are T0 + DT * k with T0, DT and the parameters exact in
binary, so that `now - loop_start_time == replan_time` and `now - traj_start_time == traj_total_time` happen EXACTLY.

"GOINGTOGOAL by the yaw term" -- the yaw term of :579 only adds to the squared distance, so alone it can never take a robot to
GOINGTOGOAL.  What it can do is decide: role `yaw_wraps` has |dyaw| = 4 pi + 0.5, where the fmod makes the sum fall below 1.0
(without the fmod it would not), and role `yaw_blocks` has a squared distance below 1.0 that the yaw term lifts to 1.0 or more, so
the robot replans.  Both are in the coverage list (test_fleet_manager_cpu.py).

"A first plan that fails and the GOINGTOGOAL -> IDLE it leads to" needs a manager whose replan_time is shorter than a tick
(seed 1): with traj_start_time = traj_total_time = 0 at the start, the finish rule takes a robot whose first plan failed to IDLE
on the first tick that starts no cycle, which with a longer replan_time is the very next one (seeds 0 and 2 pin that)."""
import math

import numpy as np

INIT, IDLE, PLANNING, REPLAN, GOINGTOGOAL, EMERGENCY_STOP = range(6)
NONE, FRESH, REPLAN_ACTION = 0, 1, 2
SEARCH_OK, SEARCH_E_NO_PATH, BUILD_OK, BUILD_E_POINTS = 0, -4, 0, -1
INT_ROWS = ("state", "have_goal", "have_start", "leg", "action", "returned", "plan_mask", "fresh_mask", "replan_mask", "stop_mask",
            "after_plan_mask")
DOUBLE_ROWS = ("goal_x", "goal_y", "goal_yaw", "start_x", "start_y", "start_yaw", "plan_start_x", "plan_start_y", "plan_start_yaw",
               "loop_start_time", "plan_start_time", "traj_start_time", "traj_total_time", "time")
COUNTERS = ("fresh", "replan", "going_to_goal", "stopped", "delivered", "arrived", "refused", "pad")
MAX_LEGS = 20
P = 16                      # pieces per row of T: max_pieces as a handle of 16 pieces rounds it
T0, DT = 100.0, 0.25
SEEDS = (0, 1, 2)
SEED_PARAMS = {
    0: dict(replan_time=1.0, max_replan_time=0.5, replan_on_collision_only=0, stop_inside_obstacle=0, stop_on_no_path=0),
    1: dict(replan_time=0.125, max_replan_time=0.5, replan_on_collision_only=0, stop_inside_obstacle=1, stop_on_no_path=1),
    2: dict(replan_time=1.0, max_replan_time=0.5, replan_on_collision_only=1, stop_inside_obstacle=0, stop_on_no_path=0),
}
DEFAULT_PARAMS = dict(replan_time=5000.0, max_replan_time=0.05, replan_on_collision_only=0, stop_inside_obstacle=0, stop_on_no_path=0)

# the small map of the collision stop: free but for a 5 x 5 block of occupied cells, whose inner 3 x 3 cells have a negative distance
NX = NY = 16
X_LO = Y_LO = -4.0
RES = 0.5
BLOCK = (10, 15, 5, 10)     # occupied cells x in [10, 15), y in [5, 10)


def finite3(v):
    return all(math.isfinite(float(x)) for x in v)


def inside_obstacle(dist, x, y, nx=NX, ny=NY, x_lo=X_LO, y_lo=Y_LO, res=RES):
    """getDistanceReal(pose) < 0: the nearest cell, nothing outside the map (fleet::inside_obstacle)"""
    if dist is None or not (math.isfinite(x) and math.isfinite(y)):
        return False
    x_hi, y_hi = x_lo + nx * res, y_lo + ny * res
    if x < x_lo or y < y_lo or x > x_hi or y > y_hi:
        return False
    inv = 1.0 / res
    ix, iy = int((x - x_lo) * inv), int((y - y_lo) * inv)
    ix, iy = min(max(ix, 0), nx - 1), min(max(iy, 0), ny - 1)
    return bool(dist[ix, iy] < 0.0)


def grid_of_map():
    """cell states of the small map: 1 unoccupied, 2 occupied"""
    g = np.ones((NX, NY), np.uint8)
    g[BLOCK[0]:BLOCK[1], BLOCK[2]:BLOCK[3]] = 2
    return g


def stand_in_dist():
    """a distance field with the signs of the map's ESDF: negative in the inner 3 x 3 cells of the block, 0 on its rim, positive
    elsewhere (the CPU tests run on it; the GPU test reads the field the device built and checks these signs)"""
    d = np.full((NX, NY), 1.0)
    d[BLOCK[0]:BLOCK[1], BLOCK[2]:BLOCK[3]] = 0.0
    d[BLOCK[0] + 1:BLOCK[1] - 1, BLOCK[2] + 1:BLOCK[3] - 1] = -RES
    return d


class Robot:
    def __init__(self):
        self.state, self.have_goal, self.have_start, self.leg, self.action, self.returned = IDLE, 0, 0, 0, NONE, 1
        self.goal, self.start, self.plan_start = [0.0] * 3, [0.0] * 3, [0.0] * 3
        self.loop_start_time, self.plan_start_time, self.traj_start_time, self.traj_total_time, self.time = 0.0, -1.0, 0.0, 0.0, -1.0
        self.flags = [0, 0, 0, 0, 0]        # plan, fresh, replan, stop, after_plan


class Fleet:
    """the manager of B robots; `events` collects what the coverage test looks for"""

    def __init__(self, B, params=None):
        self.B, self.p = B, dict(DEFAULT_PARAMS, **(params or {}))
        self.robots = [Robot() for _ in range(B)]
        self.counters = dict.fromkeys(COUNTERS, 0)
        self.events = set()
        self.now = None

    # start_callback / goal_callback
    def request(self, starts=None, goals=None, mask=None):
        """one alore_backend_manager_request: starts / goals [n][3] or None, mask [n] or None; `refused` counts THIS call"""
        self.counters["refused"] = 0
        for b, r in enumerate(self.robots[:len(starts if starts is not None else goals)]):
            if mask is not None and not mask[b]:
                continue
            for given, flag, dst in ((starts, "have_start", r.start), (goals, "have_goal", r.goal)):
                if given is None:
                    continue
                if r.state != IDLE or not finite3(given[b]):
                    self.counters["refused"] += 1
                    self.events.add("refused_busy" if r.state != IDLE else "refused_not_finite")
                else:
                    setattr(r, flag, 1)
                    dst[:] = [float(v) for v in given[b][:3]]

    def begin(self, now, poses, inside=None, collision=None, count=None):
        p, self.now = self.p, float(now)
        for b, r in enumerate(self.robots[:count or self.B]):
            r.flags, r.action, r.returned = [0, 0, 0, 0, 0], NONE, 1
            if p["stop_inside_obstacle"] and r.have_goal and inside is not None and inside[b]:
                r.state, r.flags[3] = EMERGENCY_STOP, 1
                self.counters["stopped"] += 1
                self.events.add("stop_inside_obstacle")
                continue
            if not (r.have_goal and r.have_start):
                if r.have_goal or r.have_start:
                    self.events.add("goal_or_start_alone_does_nothing")
                continue
            r.returned = 0
            waited = now - r.loop_start_time
            if r.state in (PLANNING, REPLAN) and waited == p["replan_time"]:
                self.events.add("replan_time_exactly")
            if not (r.state == IDLE or (r.state in (PLANNING, REPLAN) and waited > p["replan_time"])):
                continue
            r.loop_start_time = float(now)
            if r.state == IDLE:
                r.state, r.plan_start_time, r.time, r.plan_start = PLANNING, -1.0, -1.0, list(r.start)
                r.action, r.flags[0] = FRESH, 1
                self.counters["fresh"] += 1
                self.events.add("fresh")
                continue
            dx, dy = float(poses[b][0]) - r.goal[0], float(poses[b][1]) - r.goal[1]
            d2, dyaw = dx * dx + dy * dy, abs(r.plan_start[2] - r.goal[2])
            near = d2 + math.fmod(dyaw, 2.0 * math.pi) * 0.02 < 1.0
            if near or r.traj_total_time < p["max_replan_time"]:
                if near and dyaw == 0.0:
                    self.events.add("going_by_distance")
                if near and not d2 + dyaw * 0.02 < 1.0:
                    self.events.add("going_yaw_wraps")
                if not near:
                    self.events.add("going_by_short_trajectory")
                    if r.plan_start_time < 0.0:
                        self.events.add("going_after_failed_first_plan")
                r.state, r.returned = GOINGTOGOAL, 1
                self.counters["going_to_goal"] += 1
                continue
            if d2 < 1.0:
                self.events.add("yaw_blocks")
            if p["replan_on_collision_only"]:
                hit = collision is not None and bool(collision[b])
                self.events.add("collision_only_set" if hit else "collision_only_clear")
                if not hit:
                    continue
            r.state, r.time = REPLAN, now + p["max_replan_time"] - r.plan_start_time
            r.action, r.flags[0] = REPLAN_ACTION, 1
            self.counters["replan"] += 1
            self.events.add("replan")

    def starts(self, xytheta, vaj, oaj, count=None):
        """manager_starts on copies: (xytheta, vaj, oaj, start_yaw, end_yaw)"""
        x, v, o = np.array(xytheta, np.float64), np.array(vaj, np.float64), np.array(oaj, np.float64)
        n = count or self.B
        for b, r in enumerate(self.robots[:n]):
            if r.action == FRESH:
                x[b], v[b], o[b] = r.start, 0.0, 0.0
            elif r.action == REPLAN_ACTION:
                r.plan_start = [float(c) for c in x[b]]
        return x, v, o, np.array([r.plan_start[2] for r in self.robots[:n]]), np.array([r.goal[2] for r in self.robots[:n]])

    def end(self, search, build, ok, T, n_pieces, count=None):
        p, now = self.p, self.now
        for b, r in enumerate(self.robots[:count or self.B]):
            if r.returned:
                continue
            if r.action != NONE:
                if search[b] != SEARCH_OK:
                    r.state = EMERGENCY_STOP
                    if p["stop_on_no_path"]:
                        r.flags[3] = 1
                    self.counters["stopped"] += 1
                    self.events.add("no_path_with_stop" if p["stop_on_no_path"] else "no_path_without_stop")
                    continue
                if build[b] != BUILD_OK or not ok[b]:
                    self.events.add("build_failure" if build[b] != BUILD_OK else "plan_failure")
                    if r.action == FRESH:
                        self.events.add("first_plan_fails")
                    continue
                r.plan_start_time = now if r.plan_start_time < 0.0 else now + p["max_replan_time"]
                r.traj_start_time = r.plan_start_time
                duration = 0.0
                for i in range(min(max(int(n_pieces[b]), 0), len(T[b]))):
                    duration += float(T[b][i])
                r.traj_total_time = duration
                r.flags[1 if r.action == FRESH else 2] = 1
                r.flags[4] = 1
                self.counters["delivered"] += 1
            if now - r.traj_start_time >= r.traj_total_time:
                if now - r.traj_start_time == r.traj_total_time and r.traj_total_time > 0.0:
                    self.events.add("arrival_exactly")
                if r.state == GOINGTOGOAL:
                    self.events.add("going_to_idle")
                    if r.plan_start_time < 0.0:
                        self.events.add("failed_first_plan_going_to_idle")
                if r.have_goal:
                    self.events.add("arrival")
                r.state, r.have_goal, r.have_start = IDLE, 0, 0
                self.counters["arrived"] += 1

    def next_legs(self, poses, task_status, n_order, leg_goal_xy, leg_yaw, reset_legs=False, count=None):
        for b, r in enumerate(self.robots[:count or self.B]):
            if r.state != IDLE or r.have_goal:
                continue
            if reset_legs:
                r.leg = 0
            if task_status[b] < 0 or not 0 <= r.leg < min(int(n_order[b]), MAX_LEGS):
                continue
            r.goal = [float(leg_goal_xy[b][r.leg][0]), float(leg_goal_xy[b][r.leg][1]), float(leg_yaw[b][r.leg])]
            r.start = [float(v) for v in poses[b][:3]]
            r.have_goal = r.have_start = 1
            r.leg += 1

    def snapshot(self, count=None):
        """ints [11][n] int32, doubles [14][n] float64, counters [8] int32: what alore_backend_get_manager returns"""
        rs = self.robots[:count or self.B]
        ints = np.array([[r.state, r.have_goal, r.have_start, r.leg, r.action, r.returned] + r.flags for r in rs], np.int32).T
        dbl = np.array([r.goal + r.start + r.plan_start + [r.loop_start_time, r.plan_start_time, r.traj_start_time, r.traj_total_time, r.time]
                        for r in rs], np.float64).T
        return np.ascontiguousarray(ints), np.ascontiguousarray(dbl), np.array([self.counters[k] for k in COUNTERS], np.int32)


def same(got, exp, what):
    """two snapshots (ints, doubles, counters) are equal, the doubles by their bit patterns"""
    for k, name in enumerate(INT_ROWS):
        assert np.array_equal(got[0][k], exp[0][k]), (what, name, np.argwhere(got[0][k] != exp[0][k])[:8].ravel(), got[0][k], exp[0][k])
    for k, name in enumerate(DOUBLE_ROWS):
        g, e = got[1][k].view(np.uint64), exp[1][k].view(np.uint64)
        assert np.array_equal(g, e), (what, name, np.argwhere(g != e)[:8].ravel(), got[1][k][g != e][:4], exp[1][k][g != e][:4])
    assert np.array_equal(got[2], exp[2]), (what, "counters", got[2], exp[2])


# ---- scenarios -------------------------------------------------------------------------------------------------------------------
ROLES = ("free_run", "near_goal", "yaw_wraps", "yaw_blocks", "first_plan_fails", "no_path", "build_then_plan_failure", "second_request",
         "goal_alone", "into_obstacle", "exact_arrival", "collides")
LONG, FAR = 100.0, (40.0, 30.0)     # a duration no run reaches; an offset of the pose from the goal far beyond 1 m


def tick_time(k):
    return T0 + DT * k


def scenario(seed, B=70, K=12):
    """B robots x K ticks of scripted inputs.  Per tick k a dict: now; req_mask [B] (all 0: no request call), req_start / req_goal
    [B][3] with has_start / has_goal [B]; poses [B][3]; collision [B]; predicted xytheta / vaj / oaj [B][3] (what the predicted
    state would be); search / build / ok [B]; T [B][P] and n_pieces [B]."""
    rng = np.random.default_rng(1000 + seed)
    params = SEED_PARAMS[seed]
    every_tick = params["replan_time"] < DT
    role = [ROLES[b % len(ROLES)] for b in range(B)]
    goal = np.stack([rng.uniform(-3.5, -0.5, B), rng.uniform(-3.5, 3.5, B), rng.uniform(-3.0, 3.0, B)], 1)
    start = np.stack([rng.uniform(-3.5, -0.5, B), rng.uniform(-3.5, 3.5, B), rng.uniform(-3.0, 3.0, B)], 1)
    offset = np.tile(np.array(FAR), (B, 1)) + rng.uniform(0.0, 5.0, (B, 2))     # far from the goal, outside the map
    first = np.zeros(B, int)                                                     # the tick of the first request
    for b, r in enumerate(role):
        if r == "near_goal":
            offset[b], start[b, 2] = rng.uniform(-0.5, 0.5, 2), goal[b, 2]
        elif r == "yaw_wraps":
            offset[b], start[b, 2] = (0.75, 0.5), goal[b, 2] + (4.0 * math.pi + 0.5)
        elif r == "yaw_blocks":
            offset[b], start[b, 2] = (0.9, 0.4), goal[b, 2] + 3.0
        elif r == "exact_arrival":
            first[b] = 1
    ticks = []
    for k in range(K):
        t = dict(now=tick_time(k), req_mask=np.zeros(B, np.int32), has_start=np.zeros(B, np.int32), has_goal=np.zeros(B, np.int32),
                 req_start=start.copy(), req_goal=goal.copy(), poses=np.concatenate([goal[:, :2] + offset, rng.uniform(-3, 3, (B, 1))], 1),
                 collision=np.zeros(B, np.int32), xytheta=rng.uniform(-3.0, 3.0, (B, 3)), vaj=rng.uniform(-1.0, 1.0, (B, 3)),
                 oaj=rng.uniform(-1.0, 1.0, (B, 3)), search=rng.choice([SEARCH_OK, 1, SEARCH_E_NO_PATH], B).astype(np.int32),
                 build=rng.choice([BUILD_OK, 1, BUILD_E_POINTS], B).astype(np.int32), ok=rng.integers(0, 2, B).astype(np.int32),
                 T=np.full((B, P), np.nan), n_pieces=rng.integers(1, 6, B).astype(np.int32))
        for b, r in enumerate(role):
            n = int(t["n_pieces"][b])
            t["T"][b, :n] = rng.dirichlet(np.ones(n)) * LONG * rng.uniform(0.9, 1.1)
            plans_first = k == first[b]
            if k == first[b] and r != "goal_alone":
                t["req_mask"][b] = t["has_start"][b] = t["has_goal"][b] = 1
            # the statuses of a tick are read only for a robot that plans in it: make every robot's plan succeed, then script the failures
            t["search"][b], t["build"][b], t["ok"][b] = SEARCH_OK, BUILD_OK, 1
            if k in (2, 3, 7, 8) and r in ("free_run", "collides") and not every_tick:
                t["search"][b], t["build"][b], t["ok"][b] = SEARCH_E_NO_PATH, BUILD_E_POINTS, 0    # never read: no cycle on these ticks
            if r == "near_goal":
                t["T"][b, :2], t["n_pieces"][b] = (1.25, 0.75), 2
            elif r == "yaw_wraps":
                t["T"][b, :3], t["n_pieces"][b] = (0.5, 0.5, 0.75), 3
            elif r == "first_plan_fails" and plans_first:
                t["ok"][b] = 0
            elif r == "no_path" and plans_first:
                t["search"][b] = SEARCH_E_NO_PATH
            elif r == "build_then_plan_failure":
                cycle = k if every_tick else k // 5
                if not plans_first and cycle == 1:
                    t["build"][b] = BUILD_E_POINTS
                elif not plans_first and cycle == 2:
                    t["ok"][b] = 0
            elif r == "second_request" and k == 2:
                t["req_mask"][b] = t["has_start"][b] = t["has_goal"][b] = 1
                t["req_start"][b], t["req_goal"][b] = start[b] + 1.0, goal[b] + 1.0
            elif r == "goal_alone":
                if k == 0:
                    t["req_mask"][b] = t["has_goal"][b] = 1
                elif k == 6:
                    t["req_mask"][b] = t["has_start"][b] = 1
            elif r == "into_obstacle" and k >= 3:
                cx, cy = rng.integers(BLOCK[0] + 1, BLOCK[1] - 1), rng.integers(BLOCK[2] + 1, BLOCK[3] - 1)
                t["poses"][b, :2] = (X_LO + (cx + rng.uniform(0.05, 0.95)) * RES, Y_LO + (cy + rng.uniform(0.05, 0.95)) * RES)
            elif r == "exact_arrival":
                t["T"][b, :2], t["n_pieces"][b] = (0.25, 0.5), 2
                if k == 5:                                          # a goal that is not finite: refused and counted
                    t["req_mask"][b] = t["has_goal"][b] = 1
                    t["req_goal"][b, 1] = np.nan
                elif k == 6:                                        # the next mission of a robot that has arrived
                    t["req_mask"][b] = t["has_start"][b] = t["has_goal"][b] = 1
            elif r == "collides":
                t["collision"][b] = 1
        ticks.append(t)
    return dict(seed=seed, B=B, K=K, params=dict(params), ticks=ticks, roles=role, dist=stand_in_dist())


def request_calls(t, n):
    """the request calls of a tick for robots 0..n-1, as (starts or None, goals or None, mask): one call with both arrays when every
    addressed robot is given both, else one call for the starts and one for the goals"""
    hs, hg = t["req_mask"][:n] * t["has_start"][:n], t["req_mask"][:n] * t["has_goal"][:n]
    if not (hs.any() or hg.any()):
        return []
    if np.array_equal(hs, hg):
        return [(t["req_start"][:n], t["req_goal"][:n], hs)]
    return [c for c in ((t["req_start"][:n], None, hs), (None, t["req_goal"][:n], hg)) if c[2].any()]


def steps_of(sc, count=None):
    """a scenario as the list of calls it makes: ("Q", starts, goals, mask), ("T", tick) and ("L", reset_legs, poses)"""
    n = count or sc["B"]
    if "steps" in sc:
        return sc["steps"]
    out = []
    for t in sc["ticks"]:
        out += [("Q",) + c for c in request_calls(t, n)] + [("T", t)]
    return out


def run_oracle(sc, count=None, dist=None):
    """the oracle through a scenario: (fleet, snapshots after every T and L step, the predicted-state arrays after `starts` of every
    T step)"""
    n = count or sc["B"]
    fleet, snaps, started = Fleet(n, sc["params"]), [], []
    d = sc["dist"] if dist is None else dist
    for step in steps_of(sc, n):
        if step[0] == "Q":
            fleet.request(*step[1:])
            continue
        if step[0] == "L":
            task = sc["task"]
            fleet.next_legs(step[2], task["status"], task["n_order"], task["leg_goal_xy"], task["leg_yaw"], step[1])
        else:
            t = step[1]
            inside = [inside_obstacle(d, t["poses"][b, 0], t["poses"][b, 1]) for b in range(n)]
            fleet.begin(t["now"], t["poses"], inside, t["collision"])
            started.append(fleet.starts(t["xytheta"][:n], t["vaj"][:n], t["oaj"][:n]))
            fleet.end(t["search"], t["build"], t["ok"], t["T"], t["n_pieces"])
        snaps.append(fleet.snapshot())
    return fleet, snaps, started


LEG_TASKS = (1, 3, 2, 2, 3, 1)      # tasks per mission: n_order = 2 n legs; mission 3 has a failed status, robot 5 is busy throughout


def plain_tick(k, B, rng, duration):
    """a tick in which every plan succeeds with the given duration (two pieces)"""
    t = dict(now=tick_time(k), poses=rng.uniform(-3.5, -0.5, (B, 3)), collision=np.zeros(B, np.int32), xytheta=rng.uniform(-3.0, 3.0, (B, 3)),
             vaj=rng.uniform(-1.0, 1.0, (B, 3)), oaj=rng.uniform(-1.0, 1.0, (B, 3)), search=np.zeros(B, np.int32), build=np.zeros(B, np.int32),
             ok=np.ones(B, np.int32), T=np.full((B, P), np.nan), n_pieces=np.full(B, 2, np.int32))
    t["T"][:, :2] = np.asarray(duration)[:, None] / 2
    return t


def legs_scenario(task=None):
    """next_legs on a task slab of 6 missions, stepped until every mission is through its legs: a robot takes a leg, plans it FRESH
    with a duration of one tick, arrives on the next tick and takes the next leg.  task: status, n_order [6], leg_goal_xy [6][20][2]
    as alore_backend_get_task returns them (None: a stand-in with the same shape); leg_yaw is scripted here."""
    B, rng = len(LEG_TASKS), np.random.default_rng(77)
    if task is None:
        task = dict(status=np.array([0, 0, 0, -1, 0, 0], np.int32), n_order=np.array([2 * n for n in LEG_TASKS], np.int32),
                    leg_goal_xy=rng.uniform(-3.5, -0.5, (B, MAX_LEGS, 2)))
        task["n_order"][3] = 0
    task = dict(task, leg_yaw=rng.uniform(-3.0, 3.0, (B, MAX_LEGS)))
    duration = np.full(B, DT)
    duration[5] = LONG
    busy = np.zeros(B, np.int32)
    busy[5] = 1
    far = rng.uniform(-3.5, -0.5, (B, 3))
    far[:, :2] += 50.0
    steps = [("Q", rng.uniform(-3.5, -0.5, (B, 3)), far, busy)]
    for i in range(max(LEG_TASKS) * 2 + 1):
        steps += [("L", int(i == 0), rng.uniform(-3.5, -0.5, (B, 3))), ("T", plain_tick(2 * i, B, rng, duration)),
                  ("T", plain_tick(2 * i + 1, B, rng, duration))]
    steps += [("L", 1, rng.uniform(-3.5, -0.5, (B, 3)))]        # reset_legs: every free robot with a mission starts again at leg 0
    return dict(B=B, params=dict(SEED_PARAMS[0]), steps=steps, task=task, dist=stand_in_dist())


# what the committed seeds must reach between them (test_fleet_manager_cpu.py::test_the_seeds_reach_every_branch)
COVERAGE = ("fresh", "replan", "going_by_distance", "going_yaw_wraps", "yaw_blocks", "going_by_short_trajectory", "first_plan_fails",
            "going_after_failed_first_plan", "failed_first_plan_going_to_idle", "no_path_with_stop", "no_path_without_stop",
            "stop_inside_obstacle", "build_failure", "plan_failure", "arrival", "arrival_exactly", "refused_busy", "refused_not_finite",
            "goal_or_start_alone_does_nothing", "replan_time_exactly", "collision_only_set", "collision_only_clear", "going_to_idle")
