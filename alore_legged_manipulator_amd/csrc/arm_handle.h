// arm_handle.h -- what stands behind an alore_arm_handle (internal): shared by arm_ik.hip (include/alore_arm.h) and task_fsm.hip
// (include/alore_fsm.h), which keeps the task FSM of the same robots on the same handle.
#ifndef ALORE_ARM_HANDLE_H
#define ALORE_ARM_HANDLE_H

#include "../../include/alore_arm.h"
#include "z1_kinematics.h"

namespace arm {

constexpr int LANES = 64;

// the grasp state of the handle, structure of arrays
struct GraspSlab {
    double *joint_cmd, *robot_vel_cmd, *k, *d_gripper, *gripper_ang, *err_norm; // [.][7], [.][3], [.] ...
    int *done, *grasp_time, *flag, *stable, *ik_iterations, *ik_status;
};

} // namespace arm

struct alore_fsm_slab; // task_fsm.hip

struct alore_arm {
    int device, max_problems, n_classes;
    z1::Params P;
    z1::Class* d_classes; // [ALORE_ARM_MAX_CLASSES]
    int* d_class_of;      // [max]
    double *d_q, *d_err;  // [max][7], [max]
    int *d_iterations, *d_status;
    arm::GraspSlab g;
    double* d_stage; // [max][STAGE_ROW] doubles: host inputs and outputs of a call with device_pointers == 0
    int* d_stage_int; // [max]
    char err[256];
    alore_fsm_slab* fsm;              // NULL until alore_fsm_create
    void (*fsm_free)(alore_arm* h);   // set with it: alore_arm_destroy frees an FSM that is still attached
};

#endif
