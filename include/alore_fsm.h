/* alore_fsm.h -- C ABI of the batched ALORE task FSM (libalore_nmpc.so): the whole state machine of
 * Simulation/isaac_b2_controller/b2z1/b2z1_object_fsm.py (FSM, path_callback, the two tracking controllers, object_grasp,
 * object_release, the start and goal publishers, the /env_control_data row) for B robots on state that lives on the device.  It lives
 * on an alore_arm_handle (alore_arm.h): the grasp state, the class table and the class of every robot are the arm's, and a robot in
 * GRASPING gets the bits alore_arm_grasp_step gives it.  HIP kernels for gfx950 in float64, one lane per robot; there is no CPU
 * path.  The rules, the order of a tick, the quirks kept and the deviations are stated once, in
 * alore_legged_manipulator_amd/csrc/task_fsm.h.
 *
 * CONVENTIONS (those of alore_arm.h).  Every call returns ALORE_ARM_OK or a negative ALORE_ARM_E_* code; alore_arm_last_error has the
 * text.  Rows are addressed by BYTE strides (a multiple of 8 for doubles, of 4 for ints, at least the row).  device_pointers != 0:
 * every array of the call is DEVICE memory, read and written in stream order; nothing is allocated, nothing crosses the bus but the
 * argument block and nothing waits.  device_pointers == 0: HOST memory, uploaded, and the stream is synchronised before the call
 * returns.  Masks and n_points / n_order are packed ints [count]; a mask may be NULL (every robot).  A call is REFUSED, with
 * ALORE_ARM_E_INVALID and before anything is enqueued, for a handle without an FSM, count < 0 or count > max_problems, a bad stride,
 * or a NULL array that is not optional.  Successive calls on one handle must be ordered on the device.
 *
 * THE CHAIN without the host, on one stream:
 *   alore_backend_task_plan -> alore_fsm_set_sequences (the order slab as it lies) -> alore_fsm_tick -> request_mask, start_xytheta,
 *   goal_xytheta -> alore_backend_manager_request (device_pointers = 1) -> ... plan ... -> alore_backend_path_points_device ->
 *   alore_fsm_set_paths -> alore_fsm_tick -> the control rows. */
#ifndef ALORE_FSM_H
#define ALORE_FSM_H

#include "alore_arm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* task_state, the reference's task_state_mapping */
#define ALORE_FSM_WAIT_TASK_PLANNING 0
#define ALORE_FSM_WAIT_ROBOT_PATH 1
#define ALORE_FSM_ROBOT_TRACKING 2
#define ALORE_FSM_GRASPING 3
#define ALORE_FSM_WAIT_OBJECT_PATH 4
#define ALORE_FSM_OBJECT_TRACKING 5
#define ALORE_FSM_RELEASING 6

#define ALORE_FSM_MAX_TASKS 10
#define ALORE_FSM_CONTROL_ROW 15

/* The reference's sleeps as skipped ticks: a call of FSM() that sleeps s seconds occupies max(1, round(s * rate)) ticks.  The
 * defaults are the sleeps at the reference's 100 Hz loop.  Every count is at least 1. */
typedef struct alore_fsm_params {
    int ticks_no_plan;        /* 10: WAIT_TASK_PLANNING without a plan */
    int ticks_plan;           /* 310: the call that sees the task plan */
    int ticks_wait_path;      /* 10: each WAIT_ROBOT_PATH / WAIT_OBJECT_PATH call */
    int ticks_robot_reached;  /* 100 */
    int ticks_grasp_done;     /* 200 */
    int ticks_object_reached; /* 100 */
    int ticks_release;        /* 10: each object_release call */
    int ticks_release_done;   /* 410 */
    int stop_after_back_off;  /* 0: robot_vel_cmd stays (-0.5, 0, 0) after the back-off until a tracking tick writes a command (the
                                 reference); otherwise it is zeroed at the robot's first call after the back-off dwell.  The initial
                                 value of every robot's own word (alore_fsm_reset), which the device view exposes */
    int reserved;             /* 0 */
} alore_fsm_params;
void alore_fsm_default_params(alore_fsm_params *p);

/* Attaches an FSM for the arm's max_problems robots and allocates its slab, once: max_tasks 1..10 (rows of targets, the longest
 * sequence), max_objects >= 1 (objects a robot sees), max_path_points >= 1.  params NULL: the defaults.  Every robot starts as
 * alore_fsm_reset leaves it.  ALORE_ARM_E_INVALID for a handle that has an FSM already.  alore_arm_destroy destroys an FSM that is still
 * attached. */
int alore_fsm_create(alore_arm_handle arm, const alore_fsm_params *params, int max_tasks, int max_objects, int max_path_points);
int alore_fsm_destroy(alore_arm_handle arm);

/* com_offset [n_classes][2] (HOST, copied synchronously), parallel to the arm's class table; classes beyond n_classes and the default:
 * zeros.  1 <= n_classes <= ALORE_ARM_MAX_CLASSES; finite numbers. */
int alore_fsm_set_class_offsets(alore_arm_handle arm, int n_classes, const double *com_offset);

/* Robots 0..count-1 (mask NULL: all; otherwise HOST ints [count], robot b when mask[b] != 0) become a fresh FSM: WAIT_TASK_PLANNING,
 * no task plan, identity sequences (clamped into max_objects and max_tasks), n_tasks 1, no paths, reach_threshold 0.25, dwell 0, and the arm's grasp state as
 * alore_arm_grasp_reset leaves it.  Targets stay.  Synchronous. */
int alore_fsm_reset(alore_arm_handle arm, int count, const int *mask);

/* target_poses of robot b: [max_tasks][4] doubles (x, y, z, yaw) at (char *)target_poses + b * row_stride_bytes. */
int alore_fsm_set_targets(alore_arm_handle arm, int count, const double *target_poses, int row_stride_bytes, int device_pointers,
                          void *stream);

/* task_state_callback: the order of robot b, n_order[b] ints at (char *)order + b * order_stride_bytes, item and target alternately
 * (n_order = 2 n_tasks): the `order` and `n_order` slabs of alore_backend_device_task serve as they lie, with stride 80.  Sets
 * is_task_plan.  A row whose n_order is odd, < 2 or > 2 max_tasks, or with an item outside 0..max_objects-1 or a target outside
 * 0..max_tasks-1, leaves its robot untouched and adds one to the `refused_sequences` counter. */
int alore_fsm_set_sequences(alore_arm_handle arm, int count, const int *order, int order_stride_bytes, const int *n_order, const int *mask,
                            int device_pointers, void *stream);

/* path_callback: the marker points of robot b, n_points[b] (x, y) pairs at (char *)xy + b * xy_row_stride_bytes: the layout of
 * alore_backend_path_points[_device].  A robot in WAIT_ROBOT_PATH or WAIT_OBJECT_PATH with 0 < n_points <= max_path_points copies
 * its row, starts at index 0 and goes to ROBOT_TRACKING / OBJECT_TRACKING whatever its dwell is (the callback is asynchronous in
 * the reference), the dwell stays; n_points == 0 and every other state ignore the row; n_points > max_path_points is ignored and adds
 * one to the `refused_paths` counter. */
int alore_fsm_set_paths(alore_arm_handle arm, int count, const double *xy, int xy_row_stride_bytes, const int *n_points, const int *mask,
                        int device_pointers, void *stream);

/* One tick of robots 0..count-1: robot_pose [count][4] (x, y, z, yaw), object_poses [count][max_objects][4] raw (object_com_cal
 * is applied here), arm_base_pose [count][7], joint_positions [count][7] (as alore_arm_grasp_step).  The joint_cmd slab of
 * alore_arm_device_grasp may be joint_positions (stride 56).  One launch; a wavefront without a robot in GRASPING leaves without
 * entering the IK. */
int alore_fsm_tick(alore_arm_handle arm, int count, const double *robot_pose, int pose_stride_bytes, const double *object_poses,
                   int objects_stride_bytes, const double *arm_base_pose, int base_stride_bytes, const double *joint_positions,
                   int joint_stride_bytes, int device_pointers, void *stream);

/* The device slabs [max_problems]; valid until the FSM is destroyed.  joint_cmd, robot_vel_cmd, k, d_gripper and the rest of the grasp
 * state are in alore_arm_device_grasp. */
typedef struct alore_fsm_view {
    int *task_state, *task_num, *n_tasks, *object_type, *target_type, *robot_path_index, *object_path_index, *n_robot_path,
        *n_object_path, *dwell, *finished, *is_task_plan, *back_off, *stop_after_back_off; /* [.] */
    int *request_mask;           /* [.]: 1 on a tick whose call was WAIT_ROBOT_PATH or WAIT_OBJECT_PATH, else 0 */
    int *object_sequence, *target_sequence; /* [.][ALORE_FSM_MAX_TASKS] */
    double *reach_threshold;     /* [.] */
    double *object_vel_cmd;      /* [.][3] */
    double *start_xytheta, *goal_xytheta; /* [.][3], stride 24: alore_backend_manager_request reads them as they lie */
    double *object_pose_used;    /* [.][4]: object_com_cal of the object of object_type on the robot's last call */
    double *control;             /* [.][15]: robot_vel_cmd, object_vel_cmd, joint_cmd, task_state, object_type */
    double *robot_path, *object_path; /* [.][max_path_points][2] */
    double *target_poses;        /* [.][max_tasks][4] */
    int *counters;               /* [2]: refused_sequences, refused_paths since alore_fsm_create */
    int max_tasks, max_objects, max_path_points, reserved;
} alore_fsm_view;
int alore_fsm_device_view(alore_arm_handle arm, alore_fsm_view *out);
/* The same copied to HOST arrays with [count] rows (any pointer may be NULL; the four ints at the end are filled in); waits for the
 * device. */
int alore_fsm_get(alore_arm_handle arm, int count, alore_fsm_view *out);

#ifdef __cplusplus
}
#endif
#endif
