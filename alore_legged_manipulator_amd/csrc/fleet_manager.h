// fleet_manager.h -- the state machine of plan_manager for one robot of a fleet, the arithmetic once (internal).
// Plain C++17, float64: __host__ __device__ under hipcc, no HIP dependency otherwise.  Restates what decides in the reference
// (planning_ddr_opt/plan_manager/include/plan_manager/plan_manager.hpp): start_callback / goal_callback (:434-468), MainThread
// (:556-712), with the collision stop of PlanTester::MainThread (plan_tester/include/plan_tester/plan_tester.hpp:529-541) in front
// of it.  The functions are what one lane of the kernels of fleet_manager.hip computes for its robot;
// tests/harness/fleet_manager_check.cpp runs them robot by robot on the CPU.
//
// A manager period is begin() ... the planning of the robots whose action is not NONE ... end().  begin() decides who plans
// (FRESH: a first plan from the requested start; REPLAN: from the state predicted at `time` along the stored plan), end() reads
// what the search, the problem build and the optimiser made of it and applies the finish rule.
//
// THE REFERENCE'S RETURNS.  MainThread leaves early in four places, and the finish rule at its end (:707-711) runs only on a
// path that did not: (a) without a goal AND a start (:558), (b) on the tick that goes to GOINGTOGOAL (:581-582), (c) after a
// search without a path (:662-666), (d) after a plan that failed (:670-673); the collision stop returns as well.  Robot::returned
// carries (a), (b) and the collision stop from begin() to end().  Two ticks therefore differ from one: a robot goes to
// GOINGTOGOAL on one tick and can be IDLE on the next at the earliest.
// A robot in GOINGTOGOAL or EMERGENCY_STOP starts no cycle, and LEAVES THAT STATE ONLY THROUGH THE FINISH RULE
// (now - traj_start_time >= traj_total_time): then it is IDLE without goal and start, as in the reference.  An EMERGENCY_STOP
// by the collision stop repeats on every tick while the robot has a goal and stands in an obstacle, and on those ticks the
// finish rule does not run.
//
// CONTRACTION is off (the pragma below; g++ does not contract in ISO mode and the harness is built with -ffp-contract=off):
// every double operation is correctly rounded, in the reference's order: (dx * dx + dy * dy) + fmod(|dyaw|, 2 pi) * 0.02 < 1.0
// (:579) and (now + max_replan_time) - plan_start_time (:587).
//
// DEVIATIONS from the reference:
//   traj_total_time  starts at 0 and so does traj_start_time; the reference leaves Traj_total_time_ uninitialised;
//   duration         the rule of :580 reads final_traj_.getTotalDuration(); here it reads traj_total_time, the duration of the
//                    last plan that was DELIVERED.  The two are equal whenever the slot's last plan succeeded;
//   first plan       plan_start_time = traj_start_time = the cycle's `now`; the reference takes ros::Time::now() after planning;
//   build failure    a problem that does not build (ALORE_BE_BUILD_*) is treated like a plan that failed: the reference has no
//                    build step of its own that can fail;
//   no path          goes to EMERGENCY_STOP as the reference does, which publishes nothing there: the stop flag is raised only
//                    with stop_on_no_path;
//   requests         a start or goal with a value that is not finite is refused and counted;
//   collision only   replan_on_collision_only (off by default: the reference replans periodically) is ours.
#ifndef ALORE_FLEET_MANAGER_H
#define ALORE_FLEET_MANAGER_H

#include <cmath>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define FLEET_HD __host__ __device__ inline
#else
#define FLEET_HD inline
#endif

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

namespace fleet {

// StateMachine of plan_manager.hpp
constexpr int INIT = 0, IDLE = 1, PLANNING = 2, REPLAN = 3, GOINGTOGOAL = 4, EMERGENCY_STOP = 5;
constexpr int ACT_NONE = 0, ACT_FRESH = 1, ACT_REPLAN = 2;
constexpr int SEARCH_OK = 0, BUILD_OK = 0; // ALORE_BE_SEARCH_OK, ALORE_BE_BUILD_OK
// what a call did to a robot, for the counters
constexpr int EV_FRESH = 1, EV_REPLAN = 2, EV_GOING = 4, EV_STOPPED = 8, EV_DELIVERED = 16, EV_ARRIVED = 32, EV_REFUSED = 64;
constexpr int N_COUNTERS = 8; // fresh, replan, going_to_goal, stopped, delivered, arrived, refused, (pad)
constexpr int MAX_LEGS = 20;  // ALORE_BE_TASK_MAX_LEGS

// alore_backend_manager_params, field for field
struct Params {
    double replan_time, max_replan_time;
    int replan_on_collision_only, stop_inside_obstacle, stop_on_no_path, reserved;
};
inline void default_params(Params* p)
{
    p->replan_time = 5000.0;    // planner_sim.launch:63
    p->max_replan_time = 0.05;  // planner_sim.launch:65
    p->replan_on_collision_only = 0;
    p->stop_inside_obstacle = 0;
    p->stop_on_no_path = 0;
    p->reserved = 0;
}

struct Robot {
    int state, have_goal, have_start, leg;
    int action, returned; // of the last begin(): what end() goes on from
    double goal[3], start[3], plan_start_xytheta[3];
    double loop_start_time, plan_start_time, traj_start_time, traj_total_time;
    double time; // predicted_traj_start_time_ of the last begin(): -1 for FRESH, the time along the stored plan for REPLAN
};
// as after the constructor (:158), with the two times the reference leaves open at 0; returned = 1: no begin() yet, an end() does nothing
FLEET_HD Robot initial()
{
    Robot r{};
    r.state = IDLE;
    r.returned = 1;
    r.plan_start_time = -1.0;
    r.time = -1.0;
    return r;
}

// the five words a period leaves per robot
struct Flags {
    int plan, fresh, replan, stop, after_plan;
};

FLEET_HD bool finite3(const double* v) { return v[0] - v[0] == 0.0 && v[1] - v[1] == 0.0 && v[2] - v[2] == 0.0; }

// start_callback and goal_callback; either pointer may be null.  Returns the number of refusals (0 .. 2)
FLEET_HD int request(Robot& r, const double* start, const double* goal)
{
    int refused = 0;
    if (start) {
        if (r.state != IDLE || !finite3(start)) ++refused;
        else {
            r.have_start = 1;
            r.start[0] = start[0]; r.start[1] = start[1]; r.start[2] = start[2];
        }
    }
    if (goal) {
        if (r.state != IDLE || !finite3(goal)) ++refused;
        else {
            r.have_goal = 1;
            r.goal[0] = goal[0]; r.goal[1] = goal[1]; r.goal[2] = goal[2];
        }
    }
    return refused;
}

// getDistanceReal(pose) < 0 (sdf_map.cpp:865-871: the nearest cell; 10000 outside the map, which does not fire)
FLEET_HD bool inside_obstacle(const double* dist, int nx, int ny, double x_lo, double y_lo, double x_hi, double y_hi, double res, double x,
                              double y)
{
    if (!dist || !(x - x == 0.0 && y - y == 0.0)) return false;
    if (x < x_lo || y < y_lo || x > x_hi || y > y_hi) return false;
    const double inv = 1.0 / res;
    int ix = (int)((x - x_lo) * inv), iy = (int)((y - y_lo) * inv);
    ix = ix < 0 ? 0 : (ix > nx - 1 ? nx - 1 : ix);
    iy = iy < 0 ? 0 : (iy > ny - 1 ? ny - 1 : iy);
    return dist[(long)ix * ny + iy] < 0.0;
}

// the head of MainThread, :558-590.  inside: inside_obstacle() of the pose; collision: the robot's word of the collision mask.
// Writes r.action, r.returned and r.time, resets the five flags; returns the EV_* bits
FLEET_HD int begin(Robot& r, const Params& P, double now, const double* pose, bool inside, bool collision, Flags& f)
{
    f = Flags{0, 0, 0, 0, 0};
    r.action = ACT_NONE;
    r.returned = 1;
    if (P.stop_inside_obstacle && r.have_goal && inside) { // plan_tester.hpp:529-541
        r.state = EMERGENCY_STOP;
        f.stop = 1;
        return EV_STOPPED;
    }
    if (!(r.have_goal && r.have_start)) return 0; // :558
    r.returned = 0;
    const bool cycle = r.state == IDLE || ((r.state == PLANNING || r.state == REPLAN) && now - r.loop_start_time > P.replan_time);
    if (!cycle) return 0;
    r.loop_start_time = now;
    if (r.state == IDLE) {
        r.state = PLANNING;
        r.plan_start_time = -1.0;
        r.time = -1.0;
        r.plan_start_xytheta[0] = r.start[0]; r.plan_start_xytheta[1] = r.start[1]; r.plan_start_xytheta[2] = r.start[2];
        r.action = ACT_FRESH;
        f.plan = 1;
        return EV_FRESH;
    }
    const double dx = pose[0] - r.goal[0], dy = pose[1] - r.goal[1];
    const double near = (dx * dx + dy * dy) + std::fmod(std::fabs(r.plan_start_xytheta[2] - r.goal[2]), 2.0 * M_PI) * 0.02;
    if (near < 1.0 || r.traj_total_time < P.max_replan_time) { // :579-583
        r.state = GOINGTOGOAL;
        r.returned = 1;
        return EV_GOING;
    }
    if (P.replan_on_collision_only && !collision) return 0; // loop_start_time has moved; the state stays
    r.state = REPLAN;
    r.time = now + P.max_replan_time - r.plan_start_time; // :587, left to right
    r.action = ACT_REPLAN;
    f.plan = 1;
    return EV_REPLAN;
}

// the sum of the plan's piece durations in piece order: final_traj_.getTotalDuration()
FLEET_HD double total_duration(const double* T, int n_pieces)
{
    double s = 0.0;
    for (int i = 0; i < n_pieces; ++i) s += T[i];
    return s;
}

// the rest of MainThread, :660-711, with the `now` of the matching begin().  ORs into the flags; returns the EV_* bits
FLEET_HD int end(Robot& r, const Params& P, double now, int search_status, int build_status, int plan_ok, double duration, Flags& f)
{
    if (r.returned) return 0;
    int ev = 0;
    if (r.action != ACT_NONE) {
        if (search_status != SEARCH_OK) { // :662-666
            r.state = EMERGENCY_STOP;
            if (P.stop_on_no_path) f.stop = 1;
            return EV_STOPPED;
        }
        if (build_status != BUILD_OK || plan_ok == 0) return 0; // :670-673
        if (r.plan_start_time < 0.0) r.plan_start_time = now;   // :682-689
        else r.plan_start_time = now + P.max_replan_time;
        r.traj_start_time = r.plan_start_time;
        r.traj_total_time = duration; // :693
        if (r.action == ACT_FRESH) f.fresh = 1; else f.replan = 1;
        f.after_plan = 1;
        ev |= EV_DELIVERED;
    }
    if (now - r.traj_start_time >= r.traj_total_time) { // :707-711
        r.state = IDLE;
        r.have_goal = 0;
        r.have_start = 0;
        ev |= EV_ARRIVED;
    }
    return ev;
}

// The part of the ALORE FSM that sends /planner_start_pose and /planner_goal_pose once per entry of /task_plan/results: a robot
// that is IDLE without a goal and has legs left takes the next one.  leg_goal_xy: the mission's row [MAX_LEGS][2] of the task
// slab; leg_yaw: [MAX_LEGS].  Returns true when a leg was taken
FLEET_HD bool next_leg(Robot& r, int task_status, int n_order, const double* leg_goal_xy, const double* leg_yaw, const double* pose, bool reset_legs)
{
    if (r.state != IDLE || r.have_goal) return false;
    if (reset_legs) r.leg = 0;
    if (task_status < 0 || r.leg < 0 || r.leg >= n_order || r.leg >= MAX_LEGS) return false;
    r.goal[0] = leg_goal_xy[2 * r.leg]; r.goal[1] = leg_goal_xy[2 * r.leg + 1]; r.goal[2] = leg_yaw[r.leg];
    r.start[0] = pose[0]; r.start[1] = pose[1]; r.start[2] = pose[2];
    r.have_goal = r.have_start = 1;
    r.leg += 1;
    return true;
}

// ---- the slab: structure of arrays, one entry per robot; vectors as [3][B] so that a wavefront reads whole lines -----------------
struct Slab {
    int B;
    int *state, *have_goal, *have_start, *leg, *action, *returned;
    int *plan_mask, *fresh_mask, *replan_mask, *stop_mask, *after_plan_mask;
    double *goal, *start, *plan_start_xytheta; // [3][B]
    double *loop_start_time, *plan_start_time, *traj_start_time, *traj_total_time, *time;
    int* counters; // [N_COUNTERS]
};
constexpr int SLAB_INT_ROWS = 11, SLAB_DOUBLE_ROWS = 14;

FLEET_HD Robot load(const Slab& s, int b)
{
    Robot r;
    r.state = s.state[b]; r.have_goal = s.have_goal[b]; r.have_start = s.have_start[b]; r.leg = s.leg[b];
    r.action = s.action[b]; r.returned = s.returned[b];
    for (int k = 0; k < 3; ++k) {
        r.goal[k] = s.goal[(long)k * s.B + b];
        r.start[k] = s.start[(long)k * s.B + b];
        r.plan_start_xytheta[k] = s.plan_start_xytheta[(long)k * s.B + b];
    }
    r.loop_start_time = s.loop_start_time[b]; r.plan_start_time = s.plan_start_time[b];
    r.traj_start_time = s.traj_start_time[b]; r.traj_total_time = s.traj_total_time[b];
    r.time = s.time[b];
    return r;
}
FLEET_HD void store(const Slab& s, int b, const Robot& r)
{
    s.state[b] = r.state; s.have_goal[b] = r.have_goal; s.have_start[b] = r.have_start; s.leg[b] = r.leg;
    s.action[b] = r.action; s.returned[b] = r.returned;
    for (int k = 0; k < 3; ++k) {
        s.goal[(long)k * s.B + b] = r.goal[k];
        s.start[(long)k * s.B + b] = r.start[k];
        s.plan_start_xytheta[(long)k * s.B + b] = r.plan_start_xytheta[k];
    }
    s.loop_start_time[b] = r.loop_start_time; s.plan_start_time[b] = r.plan_start_time;
    s.traj_start_time[b] = r.traj_start_time; s.traj_total_time[b] = r.traj_total_time;
    s.time[b] = r.time;
}
FLEET_HD Flags load_flags(const Slab& s, int b) { return Flags{s.plan_mask[b], s.fresh_mask[b], s.replan_mask[b], s.stop_mask[b], s.after_plan_mask[b]}; }
FLEET_HD void store_flags(const Slab& s, int b, const Flags& f)
{
    s.plan_mask[b] = f.plan; s.fresh_mask[b] = f.fresh; s.replan_mask[b] = f.replan; s.stop_mask[b] = f.stop; s.after_plan_mask[b] = f.after_plan;
}

} // namespace fleet

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace fleet {
// the handle's map as inside_obstacle() reads it; dist NULL: no map, nothing fires
struct Map {
    const double* dist;
    int nx, ny;
    double x_lo, y_lo, x_hi, y_hi, res;
};
// The launches of fleet_manager.hip, one lane per robot, all on the given stream.  Masks are read as every mask of alore_backend.h
// (the int at (char *)mask + b * stride; NULL: every robot, for the collision mask: no robot).
hipError_t request_enqueue(const Slab& s, int count, const double* start, const double* goal, int stride, const int* mask, int mask_stride,
                           hipStream_t st);
hipError_t begin_enqueue(const Slab& s, const Params& P, const Map& m, int count, double now, const double* poses, int pose_stride,
                         const int* collision, int collision_stride, hipStream_t st);
hipError_t starts_enqueue(const Slab& s, int count, double* xytheta, double* vaj, double* oaj, double* start_yaw, double* end_yaw, hipStream_t st);
// T: [count][T_stride]
hipError_t end_enqueue(const Slab& s, const Params& P, int count, double now, const int* search_status, const int* build_status, const int* plan_ok,
                       const double* T, int T_stride, const int* n_pieces, hipStream_t st);
hipError_t next_legs_enqueue(const Slab& s, int count, const double* poses, int pose_stride, const int* task_status, const int* n_order,
                             const double* leg_goal_xy, const double* leg_yaw, int reset_legs, hipStream_t st);
} // namespace fleet
#endif
#endif
