// task_fsm.h -- the ALORE task FSM for one robot, the rules once (internal).
// Plain C++17, float64: __host__ __device__ under hipcc, no HIP dependency otherwise.  Restates the rest of the reference's FSM
// next to object_grasp (Simulation/isaac_b2_controller/b2z1/b2z1_object_fsm.py: FSM :511-572, path_callback :484-508,
// robot_tracking_controller :575-640, object_tracking_controller :752-821, object_release :824-837, object_com_cal :876-897, the
// start and goal publishers :301-363, the /env_control_data row :366-375, task_state_callback :156-167;
// Deployment/object_arrangement_fsm.py holds the same code).  GRASPING is z1::grasp_step of z1_kinematics.h.  The functions are
// what one lane of the kernels of task_fsm.hip computes for its robot; tests/harness/task_fsm_check.cpp runs them one robot at a
// time on the CPU, and tests/task_fsm_cases.py is their oracle.
//
// ONE TICK (tick_head, then tick_grasp for a robot that tick_head found in GRASPING), in this order:
//   1. request <- 0.  A robot with dwell > 0 counts it down and is done: nothing else of it changes.
//   2. A robot with back_off != 0 clears it, and zeroes robot_vel_cmd when its stop_after_back_off != 0.
//   3. One call of FSM() on task_state:
//      WAIT_TASK_PLANNING  with is_task_plan: state <- WAIT_ROBOT_PATH, task_num <- 0, the call occupies ticks_plan ticks;
//                          without: ticks_no_plan.
//      WAIT_ROBOT_PATH     object_type, target_type <- the sequences at task_num; request <- 1, start <- the robot's (x, y, yaw),
//                          goal <- get_grasp_pose(object_pose[object_type], plan_cfg) as (x_g, y_g, yaw): the rows
//                          alore_arm_grasp_poses(ALORE_ARM_POSE_PLAN) writes.  ticks_wait_path.
//      ROBOT_TRACKING      track() on the robot's pose and robot_path with 0.6 rad/s, 5 degrees and 0.15, the final heading towards
//                          the object; writes robot_vel_cmd.  Done: state <- GRASPING, ticks_robot_reached.
//      GRASPING            z1::grasp_step on robot_pose[0:2], object_pose[object_type], arm_base_pose, joint_positions.  Done:
//                          state <- WAIT_OBJECT_PATH, ticks_grasp_done.
//      WAIT_OBJECT_PATH    request <- 1, start <- the object's (x, y, yaw), goal <- target_poses[target_type] (x, y, yaw).
//                          ticks_wait_path.
//      OBJECT_TRACKING     track() on the object's pose and object_path with 0.5 rad/s, 10 degrees and 0.2, the final heading along
//                          the last two path points, current_yaw wrapped first (:782; the final turn reads the raw yaw, :761);
//                          writes object_vel_cmd.  Done: state <- RELEASING, ticks_object_reached.
//      RELEASING           object_release: joint_cmd <- arm_default_pose with the gripper at -1.5, k <- max(k - d_gripper, -0.15),
//                          joint_cmd[1] += k, robot_vel_cmd <- 0; ticks_release.  Done when k <= -0.15: k <- d_gripper <- 0,
//                          task_num += 1, robot_vel_cmd <- (-0.5, 0, 0), back_off <- 1, ticks_release_done; then task_num >=
//                          n_tasks: finished <- 1, robot_vel_cmd <- 0, back_off <- 0 (the state STAYS RELEASING); else state <-
//                          WAIT_ROBOT_PATH.
//   4. dwell <- (the ticks the call occupies) - 1; a call without a sleep occupies one tick.
//   The object's pose is object_com_cal of the raw pose of object_type with the class's com_offset:
//   (x + dx cos yaw - dy sin yaw, y + dx sin yaw + dy cos yaw, z, yaw), evaluated after step WAIT_ROBOT_PATH has chosen object_type;
//   object_pose_used keeps it (the row a second arm handle needs to repeat the grasp step).
//   wrap(e) = (e + pi) % (2 pi) - pi with Python's float %: fmod, then + 2 pi when the remainder is non-zero and negative.
//   track(): index >= n: with n > 1 and |wrap(final_yaw - yaw)| > tolerance, cmd <- (0, 0, clamp(2 e)), not done; else cmd <- 0, done.
//            index < n: dist = hypot to the point; at the LAST point reach_threshold <- the final threshold; dist < reach_threshold:
//            index += 1 and NOTHING else (no command is written); else vx = 0 beyond 15 degrees of |e| and 0.5 otherwise, cmd <-
//            (vx, 0, clamp(2 e)).
//   SLEEPS ARE SKIPPED TICKS.  A call of FSM() that sleeps s seconds occupies max(1, round(s * rate)) ticks; the defaults are the
//   reference's sleeps at its 100 Hz loop (:905): 10, 310, 10, 100, 200, 100, 10, 410.
//   path_callback is asynchronous in the reference: deliver_path changes state and index whatever dwell is, and leaves dwell alone.
//
// THE QUIRKS, kept:
//   reach_threshold  is sticky: 0.25 until the first final robot point, then 0.15 until the first final object point, then 0.2 into
//                    the next robot leg (and 0.15 again from its final point on);
//   doubled points   the last point of every piece of the marker is there twice: the second copy costs one more index tick;
//   back-off         robot_vel_cmd stays (-0.5, 0, 0) after the release until a tracking tick writes a command
//                    (stop_after_back_off == 0, the reference); any other value zeroes it at the robot's first call after the
//                    back-off dwell;
//   the last task    leaves the state RELEASING as the reference reports it, finished = 1; later calls do what object_release does
//                    from k = 0, d_gripper = 0: they rewrite joint_cmd and robot_vel_cmd and are never done;
//   one point        a path of one point skips the final turn (len > 1);
//   k at the release grasp_step leaves k = 0 and d_gripper = 0.01 when it is done (:739-740): a release takes 15 calls.
// DEVIATIONS: obj_num is per robot (n_tasks, 1..10), not 4; the control row is doubles where the reference's message is float32;
//   sim_2_rviz_offset is the caller's business, poses arrive in the planner's frame; a path with 0 points or more than
//   max_path_points is ignored (the reference empties its path for the former); object_type starts as 0 and the sequences as the
//   identity; what the reference prints is not kept.
//
// CONTRACTION is off (z1_kinematics.h's pragma; g++ does not contract in ISO mode and the harness is built with -ffp-contract=off).
#ifndef ALORE_TASK_FSM_H
#define ALORE_TASK_FSM_H

#include "z1_kinematics.h"

namespace fsm {

constexpr int WAIT_TASK_PLANNING = 0, WAIT_ROBOT_PATH = 1, ROBOT_TRACKING = 2, GRASPING = 3, WAIT_OBJECT_PATH = 4, OBJECT_TRACKING = 5,
              RELEASING = 6; // task_state_mapping, :31-39
constexpr int MAX_TASKS = 10;
constexpr double REACH_INITIAL = 0.25, REACH_ROBOT = 0.15, REACH_OBJECT = 0.2;
constexpr double ROBOT_WZ = 0.6, OBJECT_WZ = 0.5, MAX_VX = 0.5, KP_YAW = 2.0;
constexpr double DEG = M_PI / 180.0; // math.radians(x) = x * (pi / 180)
constexpr double ROBOT_FINAL_TOL = 5.0 * DEG, OBJECT_FINAL_TOL = 10.0 * DEG, TURN_ONLY = 15.0 * DEG;
constexpr double RELEASE_K = -0.15, RELEASE_GRIPPER = -1.5, BACK_OFF_VX = -0.5;

// alore_fsm_params, field for field
struct Params {
    int ticks_no_plan, ticks_plan, ticks_wait_path, ticks_robot_reached, ticks_grasp_done, ticks_object_reached, ticks_release,
        ticks_release_done;
    int stop_after_back_off, reserved;
};
inline void default_params(Params* p)
{
    p->ticks_no_plan = 10;         // :522
    p->ticks_plan = 310;           // :521-522
    p->ticks_wait_path = 10;       // :530, :552
    p->ticks_robot_reached = 100;  // :538
    p->ticks_grasp_done = 200;     // :544
    p->ticks_object_reached = 100; // :558
    p->ticks_release = 10;         // :831
    p->ticks_release_done = 410;   // :831 and :566
    p->stop_after_back_off = 0;
    p->reserved = 0;
}

// one robot's words next to its z1::Grasp; the paths, the sequences and the targets are arrays of the caller
struct Robot {
    int task_state, task_num, n_tasks, object_type, target_type, robot_path_index, object_path_index, n_robot_path, n_object_path, dwell,
        finished, is_task_plan, back_off, stop_after_back_off, request;
    double reach_threshold, object_vel_cmd[3], start_xytheta[3], goal_xytheta[3], object_pose_used[4];
};
constexpr int ROBOT_INTS = 15, ROBOT_DOUBLES = 14;

// a fresh FSM (:29-82, :147); sequences[2 * MAX_TASKS]: object_sequence, then target_sequence
Z1_HD void reset(const Params& F, Robot& r, int* sequences)
{
    r.task_state = WAIT_TASK_PLANNING;
    r.task_num = 0;
    r.n_tasks = 1;
    r.object_type = r.target_type = 0;
    r.robot_path_index = r.object_path_index = 0;
    r.n_robot_path = r.n_object_path = 0;
    r.dwell = 0;
    r.finished = 0;
    r.is_task_plan = 0;
    r.back_off = 0;
    r.stop_after_back_off = F.stop_after_back_off;
    r.request = 0;
    r.reach_threshold = REACH_INITIAL;
    for (int i = 0; i < 3; ++i) r.object_vel_cmd[i] = r.start_xytheta[i] = r.goal_xytheta[i] = 0.0;
    for (int i = 0; i < 4; ++i) r.object_pose_used[i] = 0.0;
    for (int i = 0; i < MAX_TASKS; ++i) sequences[i] = sequences[MAX_TASKS + i] = i;
}

// Python's (e + pi) % (2 pi) - pi
Z1_HD double wrap(double e)
{
    const double two_pi = 2.0 * M_PI;
    double r = std::fmod(e + M_PI, two_pi);
    if (r != 0.0 && r < 0.0) r += two_pi;
    return r - M_PI;
}
Z1_HD double clamp(double v, double m)
{
    const double lo = v < m ? v : m; // min(v, m)
    return lo > -m ? lo : -m;        // max(., -m)
}

// task_state_callback: order[n_order] alternates item and target.  false (and nothing changes) for a row that is refused
Z1_HD bool set_sequence(Robot& r, int* sequences, const int* order, int n_order, int max_tasks, int max_objects)
{
    if (n_order < 2 || n_order > 2 * max_tasks || (n_order & 1)) return false;
    for (int i = 0; i < n_order; i += 2)
        if (order[i] < 0 || order[i] >= max_objects || order[i + 1] < 0 || order[i + 1] >= max_tasks) return false;
    for (int i = 0; i < n_order / 2; ++i) {
        sequences[i] = order[2 * i];
        sequences[MAX_TASKS + i] = order[2 * i + 1];
    }
    r.n_tasks = n_order / 2;
    r.is_task_plan = 1;
    return true;
}

// path_callback: 0 ignored (the state, or no points), 1 the robot's path, 2 the object's, -1 too many points (ignored, counted).
// The caller copies the n points into the path the return value names
Z1_HD int deliver_path(Robot& r, int n_points, int max_path_points)
{
    if (r.task_state != WAIT_ROBOT_PATH && r.task_state != WAIT_OBJECT_PATH) return 0;
    if (n_points <= 0) return 0;
    if (n_points > max_path_points) return -1;
    if (r.task_state == WAIT_ROBOT_PATH) {
        r.n_robot_path = n_points;
        r.robot_path_index = 0;
        r.task_state = ROBOT_TRACKING;
        return 1;
    }
    r.n_object_path = n_points;
    r.object_path_index = 0;
    r.task_state = OBJECT_TRACKING;
    return 2;
}

// both tracking controllers.  path[n][2]; final_dx, final_dy: the direction of the final heading; yaw_raw is what the final turn
// reads, yaw what the points are steered by
Z1_HD int track(const double* path, int n, int& index, double x, double y, double yaw, double yaw_raw, double final_dx, double final_dy,
                double max_wz, double final_tol, double final_threshold, double& reach_threshold, double* cmd)
{
    if (index >= n) {
        if (n > 1) {
            const double e = wrap(std::atan2(final_dy, final_dx) - yaw_raw);
            if (std::fabs(e) > final_tol) {
                cmd[0] = 0.0; cmd[1] = 0.0; cmd[2] = clamp(KP_YAW * e, max_wz);
                return 0;
            }
        }
        cmd[0] = cmd[1] = cmd[2] = 0.0;
        return 1;
    }
    const double dx = path[2 * index] - x, dy = path[2 * index + 1] - y;
    const double dist = std::hypot(dx, dy);
    if (index == n - 1) reach_threshold = final_threshold;
    const double e = wrap(std::atan2(dy, dx) - yaw);
    if (dist < reach_threshold) {
        index += 1;
        return 0;
    }
    cmd[0] = std::fabs(e) > TURN_ONLY ? 0.0 : MAX_VX;
    cmd[1] = 0.0;
    cmd[2] = clamp(KP_YAW * e, max_wz);
    return 0;
}

// object_release, :824-837
Z1_HD int release(const z1::Class& c, z1::Grasp& g)
{
    for (int i = 0; i < 7; ++i) g.joint_cmd[i] = c.arm_default_pose[i];
    g.joint_cmd[6] = RELEASE_GRIPPER;
    g.k = g.k - g.d_gripper;
    g.k = g.k > RELEASE_K ? g.k : RELEASE_K;
    g.joint_cmd[1] = g.joint_cmd[1] + g.k;
    z1::set_vel(g, 0.0);
    if (g.k <= RELEASE_K) {
        g.k = 0.0;
        g.d_gripper = 0.0;
        return 1;
    }
    return 0;
}

// object_com_cal for one object: raw[4] -> out[4]
Z1_HD void com_pose(const double* raw, const double* com_offset, double* out)
{
    const double c = std::cos(raw[3]), s = std::sin(raw[3]);
    out[0] = raw[0] + com_offset[0] * c - com_offset[1] * s;
    out[1] = raw[1] + com_offset[0] * s + com_offset[1] * c;
    out[2] = raw[2];
    out[3] = raw[3];
}

// Steps 1 to 4 but for the grasp step.  sequences[2 * MAX_TASKS], robot_path and object_path [.][2], target_poses [max_tasks][4],
// robot_pose[4], object_poses [max_objects][4] raw.  Returns 1 when the robot is to run tick_grasp on this tick
Z1_HD int tick_head(const Params& F, const z1::Class& c, const double* com_offset, Robot& r, z1::Grasp& g, const int* sequences,
                    const double* robot_path, const double* object_path, const double* target_poses, const double* robot_pose,
                    const double* object_poses)
{
    r.request = 0;
    if (r.dwell > 0) { // 1
        r.dwell -= 1;
        return 0;
    }
    if (r.back_off) { // 2
        r.back_off = 0;
        if (r.stop_after_back_off) z1::set_vel(g, 0.0);
    }
    int ticks = 1;
    if (r.task_state == WAIT_TASK_PLANNING) { // 3
        ticks = F.ticks_no_plan;
        if (r.is_task_plan) {
            r.task_state = WAIT_ROBOT_PATH;
            r.task_num = 0;
            ticks = F.ticks_plan;
        }
        r.dwell = ticks - 1;
        return 0;
    }
    if (r.task_state == WAIT_ROBOT_PATH) {
        r.object_type = sequences[r.task_num];
        r.target_type = sequences[MAX_TASKS + r.task_num];
    }
    com_pose(object_poses + 4 * r.object_type, com_offset, r.object_pose_used);
    const double* obj = r.object_pose_used;
    if (r.task_state == GRASPING) return 1;
    if (r.task_state == WAIT_ROBOT_PATH) {
        const double cfg[3] = {c.plan_cfg[0], c.plan_cfg[1], c.plan_cfg[2]};
        double pose[7];
        z1::grasp_pose(obj, cfg, pose);
        r.request = 1;
        r.start_xytheta[0] = robot_pose[0]; r.start_xytheta[1] = robot_pose[1]; r.start_xytheta[2] = robot_pose[3];
        r.goal_xytheta[0] = pose[0]; r.goal_xytheta[1] = pose[1]; r.goal_xytheta[2] = obj[3];
        ticks = F.ticks_wait_path;
    } else if (r.task_state == ROBOT_TRACKING) {
        if (track(robot_path, r.n_robot_path, r.robot_path_index, robot_pose[0], robot_pose[1], robot_pose[3], robot_pose[3],
                  obj[0] - robot_pose[0], obj[1] - robot_pose[1], ROBOT_WZ, ROBOT_FINAL_TOL, REACH_ROBOT, r.reach_threshold, g.robot_vel_cmd)) {
            r.task_state = GRASPING;
            ticks = F.ticks_robot_reached;
        }
    } else if (r.task_state == WAIT_OBJECT_PATH) {
        const double* t = target_poses + 4 * r.target_type;
        r.request = 1;
        r.start_xytheta[0] = obj[0]; r.start_xytheta[1] = obj[1]; r.start_xytheta[2] = obj[3];
        r.goal_xytheta[0] = t[0]; r.goal_xytheta[1] = t[1]; r.goal_xytheta[2] = t[3];
        ticks = F.ticks_wait_path;
    } else if (r.task_state == OBJECT_TRACKING) {
        const int n = r.n_object_path;
        const double fdx = n > 1 ? object_path[2 * (n - 1)] - object_path[2 * (n - 2)] : 0.0;
        const double fdy = n > 1 ? object_path[2 * (n - 1) + 1] - object_path[2 * (n - 2) + 1] : 0.0;
        if (track(object_path, n, r.object_path_index, obj[0], obj[1], wrap(obj[3]), obj[3], fdx, fdy, OBJECT_WZ, OBJECT_FINAL_TOL,
                  REACH_OBJECT, r.reach_threshold, r.object_vel_cmd)) {
            r.task_state = RELEASING;
            ticks = F.ticks_object_reached;
        }
    } else { // RELEASING
        ticks = F.ticks_release;
        if (release(c, g)) {
            r.task_num += 1;
            z1::set_vel(g, BACK_OFF_VX);
            r.back_off = 1;
            ticks = F.ticks_release_done;
            if (r.task_num >= r.n_tasks) {
                r.finished = 1;
                z1::set_vel(g, 0.0);
                r.back_off = 0;
            } else
                r.task_state = WAIT_ROBOT_PATH;
        }
    }
    r.dwell = ticks - 1; // 4
    return 0;
}

// GRASPING: the grasp step on the pose tick_head left in object_pose_used
Z1_HD void tick_grasp(const Params& F, const z1::Params& P, const z1::Class& c, Robot& r, z1::Grasp& g, const double* robot_pose,
                      const double* arm_base_pose, const double* joint_positions)
{
    int ticks = 1;
    if (z1::grasp_step(P, c, g, robot_pose, r.object_pose_used, arm_base_pose, joint_positions)) {
        r.task_state = WAIT_OBJECT_PATH;
        ticks = F.ticks_grasp_done;
    }
    r.dwell = ticks - 1;
}

// the /env_control_data row, :366-375
Z1_HD void control_row(const Robot& r, const z1::Grasp& g, double* row)
{
    for (int i = 0; i < 3; ++i) row[i] = g.robot_vel_cmd[i];
    for (int i = 0; i < 3; ++i) row[3 + i] = r.object_vel_cmd[i];
    for (int i = 0; i < 7; ++i) row[6 + i] = g.joint_cmd[i];
    row[13] = (double)r.task_state;
    row[14] = (double)r.object_type;
}

} // namespace fsm
#endif
