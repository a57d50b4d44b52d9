/* alore_arm.h -- C ABI of the batched Z1 grasp kinematics (libalore_nmpc.so): closed-loop IK for B independent problems and the
 * grasp step of the ALORE FSM (Simulation/isaac_b2_controller/b2z1/b2z1_object_fsm.py: object_grasp, :643-749) for B robots on
 * state that lives on the device.  HIP kernels for gfx950 in float64; there is no CPU path behind it (alore_arm_create fails
 * without a GPU).  The arithmetic, its small-angle branch, the quirks kept and the deviations are stated once, in
 * alore_legged_manipulator_amd/csrc/z1_kinematics.h.
 *
 * CONVENTIONS (those of alore_backend.h).  Every call returns ALORE_ARM_OK or a negative code; alore_arm_last_error has the text.
 * Rows are addressed by BYTE strides: row b of an array is at (char *)array + b * stride_bytes; a stride is a multiple of 8 and at
 * least the row.  device_pointers != 0: every array of the call is DEVICE memory, read and written in stream order; nothing is
 * allocated, nothing crosses the bus but the argument block and nothing waits.  device_pointers == 0: they are HOST memory; inputs
 * are uploaded, outputs are copied back, and the stream is synchronised before the call returns.  `stream` is a hipStream_t (NULL:
 * the default stream).  Successive calls on one handle must be ordered on the device (one stream, or events).
 * A call is REFUSED, with ALORE_ARM_E_INVALID and before anything is enqueued, for count < 0 or count > max_problems, a stride that is
 * smaller than its row or not a multiple of 8, a NULL array that is not optional, and a class index out of range in HOST input.
 * Poses are [12] doubles (R row-major, then p) in the arm's base frame link00, or [7] doubles (x, y, z, then the quaternion x, y, z,
 * w) in the world; joint vectors are [7] doubles, entry 6 the gripper, which the IK passes through. */
#ifndef ALORE_ARM_H
#define ALORE_ARM_H

#ifdef __cplusplus
extern "C" {
#endif

#define ALORE_ARM_OK 0
#define ALORE_ARM_E_INVALID (-1)
#define ALORE_ARM_E_NO_DEVICE (-2)
#define ALORE_ARM_E_HIP (-3)
#define ALORE_ARM_E_NOMEM (-4)

/* status of a problem */
#define ALORE_ARM_IK_OK 0          /* |err| < eps */
#define ALORE_ARM_IK_LIMIT 1       /* max_iter steps were taken */
#define ALORE_ARM_IK_PIVOT 2       /* a pivot of the 6 x 6 factorisation was not positive and finite: q as it stood */
#define ALORE_ARM_IK_NOT_RUN 3     /* grasp state only: the tick ran no IK */
#define ALORE_ARM_IK_NOT_FINITE (-1) /* an input was not finite: q = q_init, err_norm NaN */

#define ALORE_ARM_CATEGORY_OTHER 0 /* x += k, z += 0.03 (the chair) */
#define ALORE_ARM_CATEGORY_TABLE 1 /* x += k / 1.5, z -= 0.01; the arm goes to arm_default_pose while the gripper closes */
#define ALORE_ARM_CATEGORY_BOX 2   /* z -= k / 2.2 */

#define ALORE_ARM_POSE_GRASP 0 /* get_grasp_pose with grasp_cfg */
#define ALORE_ARM_POSE_PLAN 1  /* get_grasp_pose with plan_cfg: the planner's goal */

#define ALORE_ARM_MAX_CLASSES 64

typedef struct alore_arm *alore_arm_handle;

typedef struct alore_arm_params {
    double eps, damp, dt; /* 1e-3, 1e-12, 3e-3: finite and positive */
    int max_iter;         /* 200; at least 1 */
    int reserved;         /* 0 */
    double joint1_xyz[3]; /* joint1 in link00: 0, 0, 0.0585 */
    double tool_xyz[3];   /* gripperStator in link06: 0.051, 0, 0 */
    double joint_default[7]; /* the command of the approach: 0, 1.48, -0.63, -0.84, 0, 1.57, 0 */
} alore_arm_params;
void alore_arm_default_params(alore_arm_params *p);

/* one object class: config.yaml `objects` */
typedef struct alore_arm_class {
    int category; /* ALORE_ARM_CATEGORY_* */
    int reserved; /* 0 */
    double grasp_cfg[3]; /* dx, dz, pitch in degrees */
    double plan_cfg[3];  /* the same for the planner's goal; [0] is also the grasp distance of the base */
    double arm_default_pose[7];
} alore_arm_class;

/* params NULL: the defaults.  ALORE_ARM_E_INVALID for max_problems < 1, max_iter < 1, an eps, damp or dt that is not finite and
 * positive, or any other number that is not finite; ALORE_ARM_E_NO_DEVICE without a GPU.  The class table starts as the three classes
 * of the reference's config.yaml (0 chair, 1 table, 2 box) until alore_arm_set_classes replaces it; every robot starts in class 0
 * and in the reset grasp state. */
int alore_arm_create(const alore_arm_params *params, int device, int max_problems, alore_arm_handle *out);
int alore_arm_destroy(alore_arm_handle h);
const char *alore_arm_last_error(alore_arm_handle h);

/* For inspection: q [count][7] -> pose [count][12] and the LOCAL frame Jacobian [count][6][6] (row-major, linear rows first);
 * either output may be NULL. */
int alore_arm_fk(alore_arm_handle h, int count, const double *q, int q_stride_bytes, double *pose, int pose_stride_bytes, double *jac,
                 int jac_stride_bytes, int device_pointers, void *stream);

/* Solves problems 0..count-1 from q_init [count][7] towards target [count][12]; the results stay on the device.  A problem that has
 * finished is frozen; iteration counts are per problem.  With device_pointers != 0 the q slab of alore_arm_device_ik may be q_init
 * (stride 56): a servo sequence runs in stream order without the host. */
int alore_arm_ik(alore_arm_handle h, int count, const double *q_init, int q_stride_bytes, const double *target, int target_stride_bytes,
                 int device_pointers, void *stream);
typedef struct alore_arm_ik_view {
    double *q;              /* [.][7] */
    const double *err_norm; /* [.]: the last norm that was evaluated (not evaluated again after the last step) */
    const int *iterations;  /* [.] */
    const int *status;      /* [.]: ALORE_ARM_IK_* */
} alore_arm_ik_view;
/* the device slabs [max_problems]; valid until the handle is destroyed */
int alore_arm_device_ik(alore_arm_handle h, alore_arm_ik_view *out);
/* the same copied to HOST arrays (any may be NULL); waits for the device */
int alore_arm_get_ik(alore_arm_handle h, int count, double *q, double *err_norm, int *iterations, int *status);

/* The class table (1 .. ALORE_ARM_MAX_CLASSES rows, HOST memory; copied synchronously).  ALORE_ARM_E_INVALID for a category that is
 * none of ALORE_ARM_CATEGORY_* or a number that is not finite. */
int alore_arm_set_classes(alore_arm_handle h, int n_classes, const alore_arm_class *classes);
/* class_of [count] ints: the class of each robot / object slot.  HOST input (device_pointer == 0) is checked against the table and
 * refused as a whole; DEVICE input is clamped into the table where it is read. */
int alore_arm_set_robot_classes(alore_arm_handle h, int count, const int *class_of, int device_pointer, void *stream);

/* get_grasp_pose for slots 0..count-1 with the cfg of each slot's class: object_pose [count][4] (x, y, z, yaw) ->
 * out_pose [count][7] (may be NULL) and out_goal_xytheta [count][3] = (x_g, y_g, yaw) (may be NULL).  `which`: ALORE_ARM_POSE_*.
 * With ALORE_ARM_POSE_PLAN and stride 24 the goal rows are what alore_backend_manager_request reads as goal_xytheta. */
int alore_arm_grasp_poses(alore_arm_handle h, int count, const double *object_pose, int object_stride_bytes, int which, double *out_pose,
                          int pose_stride_bytes, double *out_goal_xytheta, int goal_stride_bytes, int device_pointers, void *stream);

/* Puts robots 0..count-1 (mask NULL: all; otherwise HOST ints [count], robot b when mask[b] != 0) into the state of a fresh FSM:
 * k 0, d_gripper 0, gripper_ang -1.5, err_norm 1000, grasp_time 0, flag 0, stable 0, done 0, joint_cmd = joint_default,
 * robot_vel_cmd 0.  Synchronous. */
int alore_arm_grasp_reset(alore_arm_handle h, int count, const int *mask);
/* One call of object_grasp for robots 0..count-1, the IK inside it: robot_xy [count][2], object_pose [count][4],
 * arm_base_pose [count][7] (world), joint_positions [count][7] (the measured arm joints: entries 8 and 13..18 of the reference's
 * joint vector).  The joint_cmd slab of alore_arm_device_grasp may be joint_positions (stride 56). */
int alore_arm_grasp_step(alore_arm_handle h, int count, const double *robot_xy, int xy_stride_bytes, const double *object_pose,
                         int object_stride_bytes, const double *arm_base_pose, int base_stride_bytes, const double *joint_positions,
                         int joint_stride_bytes, int device_pointers, void *stream);
typedef struct alore_arm_grasp_view {
    double *joint_cmd;           /* [.][7] */
    const double *robot_vel_cmd; /* [.][3] */
    const int *done;             /* [.]: 1 on the tick that finished a grasp */
    const double *k, *d_gripper, *gripper_ang, *err_norm; /* [.] */
    const int *grasp_time, *flag, *stable;                /* [.] */
    const int *ik_iterations, *ik_status;                 /* [.]: of the last tick; ALORE_ARM_IK_NOT_RUN when it ran no IK */
} alore_arm_grasp_view;
int alore_arm_device_grasp(alore_arm_handle h, alore_arm_grasp_view *out);
/* HOST arrays of the same shapes (any may be NULL); alore_arm_get_grasp waits for the device */
typedef struct alore_arm_grasp_host {
    double *joint_cmd, *robot_vel_cmd;
    int *done;
    double *k, *d_gripper, *gripper_ang, *err_norm;
    int *grasp_time, *flag, *stable, *ik_iterations, *ik_status;
} alore_arm_grasp_host;
int alore_arm_get_grasp(alore_arm_handle h, int count, const alore_arm_grasp_host *out);

#ifdef __cplusplus
}
#endif
#endif
