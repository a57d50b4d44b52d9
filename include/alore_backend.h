/*
 * alore_backend.h -- C ABI of the MI355X-native batched back_end trajectory optimiser.
 *
 * Drop-in boundary for `bool MSPlanner::minco_plan(const FlatTrajData&)`
 * (reference: planning_ddr_opt/back_end/include/back_end/optimizer.h:207, src/optimizer.cpp:169-220; input
 * struct planning_ddr_opt/front_end/include/front_end/traj_representation.h:46-58; results read back through
 * get_current_iniState / finState / Innerpoints / finalpieceTime / iniStateXYTheta, optimizer.h:253-268, the
 * fields plan_manager serialises into carstatemsgs/Polynome, plan_manager.hpp:784-831).
 * One call plans `count` independent FlatTrajData problems -- Monte-Carlo start poses x object classes --
 * in one kernel launch, one wavefront per problem: differential-flat (yaw, arc length) minimum-jerk
 * spline, Simpson-integrated pose, smoothed-L1 penalties, ESDF clearance, L-BFGS with the Lewis-Overton
 * line search, augmented-Lagrangian terminal constraint, final collision check and retry, all in float64
 * like the reference.  Plain pointers and sizes only; nothing throws across this boundary; there is no CPU
 * path behind it (alore_backend_create fails without a GPU).
 *
 * Functions return 0 or a negative ALORE_BE_E_* code.  A handle is bound to one GPU and is not
 * thread-safe; `stream` is a hipStream_t passed as void* (NULL = default stream).
 */
#ifndef ALORE_BACKEND_H
#define ALORE_BACKEND_H

#ifdef __cplusplus
extern "C" {
#endif

#define ALORE_BE_OK 0
#define ALORE_BE_E_INVALID (-1)
#define ALORE_BE_E_NO_DEVICE (-2)
#define ALORE_BE_E_HIP (-3)
#define ALORE_BE_E_NOMEM (-4)
#define ALORE_BE_E_UNSUPPORTED (-5) /* more pieces than the handle was created for, or than any handle takes (64) */

typedef struct alore_backend_planner *alore_backend_handle;

/* lbfgs::lbfgs_parameter_t (planning_ddr_opt/back_end/include/gcopter/lbfgs.hpp:14-129) */
typedef struct alore_lbfgs_param {
    int mem_size, past, max_iterations, max_linesearch;
    double g_epsilon, delta, min_step, max_step, f_dec_coeff, s_curv_coeff, cautious_factor, machine_prec;
} alore_lbfgs_param;

/* What MSPlanner reads from the parameter server (optimizer.cpp:17-166: back_end/config/global_planning3ms.yaml,
 * planner_sim.launch:41-46) and from plan_manager's Config (plan_manager/config/car3ms.yaml).
 * alore_backend_default_config fills the values of those files. */
typedef struct alore_backend_config {
    double max_vel, min_vel, max_acc, max_omega, max_domega, max_cen_acc;
    int direct_v_omega;                                                            /* if_directly_constrain_v_omega */
    double w_time, w_acc, w_domega, w_collision, w_moment, w_mean_time, w_cen_acc; /* penaltyWeights */
    double p_time, p_bigpath, p_moment, p_mean_time, p_acc, p_domega;              /* PathpenaltyWeights */
    double energy_w[2];                                                            /* energyWeights (yaw, s) */
    double smooth_eps, safe_dis, final_min_safe_dis;
    int final_check_num, safe_replan_max;
    double mean_lo, mean_hi;
    int sparse_res;  /* sparseResolution; this build supports 8 (17 Simpson nodes per piece) */
    int n_check;     /* body check points (<= 8) */
    double check_pts[8][2];
    double icr_xv;
    int standard_diff;
    double lam0[2], rho0[2], rho_max[2], gamma[2], tol;
    double cut_lam0[2], cut_rho0[2], cut_rho_max[2], cut_gamma[2], cut_tol;
    alore_lbfgs_param path_lbfgs;
    int shot_path_past;
    double shot_path_horizon;
    alore_lbfgs_param lbfgs;
    int max_alm_rounds; /* cap on the reference's unbounded `while (ros::ok())` ALM loop (optimizer.cpp:376) */
} alore_backend_config;

/* FlatTrajData, host pointers; M = n_pieces = len(UnOccupied_traj_pts) + 1 */
typedef struct alore_flat_traj {
    int n_pieces;
    const double *traj_pts;  /* (M-1) x 3: yaw, s, t (t unused by the optimiser) */
    double init_T;           /* UnOccupied_initT */
    const double *positions; /* (M-1) x 3: x, y, yaw of UnOccupied_positions */
    double start_state[2][3], final_state[2][3]; /* [yaw | s][p v a] */
    double start_xytheta[3], final_xytheta[3];
    int if_cut;
} alore_flat_traj;

/* per-problem outcome; `ok` is minco_plan's return value */
typedef struct alore_backend_status {
    int ok;         /* 1: planned and collision-free */
    int attempts;   /* optimiser passes (collision retries with 0.75 x time weight, optimizer.cpp:179-200) */
    int alm_rounds; /* of the last pass */
    int evals;      /* cost-callback evaluations, all passes */
    int lbfgs_ret;  /* lbfgs return code of the last stage-2 call (lbfgs.hpp:135-184) */
    int path_ret;   /* of the pre-processing stage */
    int collision;  /* final check of the last pass */
    int n_pieces;
    double cost, xy_err[2], min_dist, tail_s;
} alore_backend_status;

void alore_backend_default_config(alore_backend_config *c);
/* max_pieces: the longest trajectory a slot holds, 1 .. 64; the handle rounds it up to the piece capacity P of one of the three
 * builds of the optimiser -- 16, 32 or 64 (alore_backend_slots: max_pieces) -- and every slab below is sized by P.  64 pieces are
 * a route of about 50 m at the default front-end parameters.  More than 64: ALORE_BE_E_UNSUPPORTED.
 * Device memory per problem slot is dominated by the L-BFGS history [256][2][3 P] doubles: 192 KiB at P = 16, 384 KiB at 32 and
 * 768 KiB at 64; with the cross products (36 KiB), the evaluation workspace (28.25 KiB at P <= 32, 60.5 KiB at 64) and the problem
 * and result slabs that is about 260, 455 and 880 KiB per slot.  A handle that cannot be allocated fails with ALORE_BE_E_NOMEM and
 * leaves nothing allocated. */
int alore_backend_create(const alore_backend_config *cfg, int device, int max_pieces, int max_problems,
                         alore_backend_handle *out);
int alore_backend_destroy(alore_backend_handle h);
const char *alore_backend_last_error(alore_backend_handle h);

/* plan_env::SDFmap as the optimiser queries it (sdf_map.cpp:760-863): double grid, dist[ix * ny + iy], cell
 * centres at ((i + 0.5) res + lo); copied to the device and kept until replaced */
int alore_backend_set_map(alore_backend_handle h, const double *dist, int nx, int ny, double x_lo, double y_lo, double res);
/* The same map built on the device from the occupancy grid: SDFmap::updateESDF2d (sdf_map.cpp:618-681, fillESDF
 * :683-714).  grid [nx][ny] holds the reference's cell states (0 unknown, 1 unoccupied, 2 occupied; sdf_map.h:98); the
 * field is recomputed inside the window (odom_x, odom_y) +- detection_range, cells outside it keep their values
 * (DBL_MAX after the first call with a new geometry, as in sdf_map.h:160).  dist_out (HOST, [nx][ny]) may be NULL. */
int alore_backend_build_esdf(alore_backend_handle h, const unsigned char *grid, int nx, int ny, double x_lo, double y_lo, double res,
                             double odom_x, double odom_y, double detection_range, double *dist_out);

/* upload `count` problems (<= max_problems) into the handle's device slots 0..count-1 */
int alore_backend_set_problems(alore_backend_handle h, int count, const alore_flat_traj *problems, void *stream);
/* MSPlanner::minco_plan for every uploaded problem, one launch; results stay on the device */
int alore_backend_plan(alore_backend_handle h, int count, void *stream);
/* results of the last plan: status[count]; inner [count][(P-1)*2] (yaw, s), T [count][P],
 * coef [count][P*12] (coefficient of t^q of piece i, dimension d at ((6 i + q) * 2 + d)); any pointer may be NULL;
 * P = max_pieces.  Synchronises the stream. */
int alore_backend_results(alore_backend_handle h, int count, alore_backend_status *status, double *inner, double *T,
                          double *coef, void *stream);

/* device pointers of the result slabs (for consumers on the same GPU, e.g. alore_nmpc_refs_set_from_backend):
 * same layouts as alore_backend_results; valid until the handle is destroyed */
typedef struct alore_backend_device_view {
    int max_pieces;
    const int *n_pieces;        /* [B] */
    const double *inner;        /* [B][(P-1)*2] */
    const double *T;            /* [B][P] */
    const double *coef;         /* [B][P*12] */
    const double *head;         /* [B][6]  start_state as uploaded: [d][p v a] */
    const double *tail;         /* [B][6]  final_state with the optimised arc length */
    const double *start_xytheta; /* [B][3] */
    const int *ok;              /* [B] */
} alore_backend_device_view;
int alore_backend_device_results(alore_backend_handle h, alore_backend_device_view *out);

/* ---- pieces of the optimiser, exposed for parity tests against the CPU oracle ------------------------ */
/* one cost-callback evaluation per problem: stage 1 = costFunctionCallbackPath (optimizer.cpp:1272-1317),
 * 2 = costFunctionCallback (:631-692).  x, grad: [count][3P-1 stride = 3 * max_pieces]; lam, rho: [count][2] or
 * NULL (config values); cost [count]; xy_err [count][2].  Host pointers; synchronises.  safe_dis, time_weight: the value for
 * every slot, or NaN for the configured one (config.safe_dis, config.w_time: with a class table the slot's class's). */
int alore_backend_eval(alore_backend_handle h, int count, int stage, const double *x, const double *lam, const double *rho,
                       double safe_dis, double time_weight, double *cost, double *grad, double *xy_err, void *stream);
/* lbfgs_optimize on one stage from x (in/out), at most max_iter iterations (0 = the configured limit);
 * ret/iters/evals [count] */
int alore_backend_lbfgs(alore_backend_handle h, int count, int stage, double *x, const double *lam, const double *rho,
                        double safe_dis, double time_weight, int max_iter, double *cost, int *ret, int *iters, int *evals,
                        double *xy_err, void *stream);

/* duration of the last alore_backend_plan launch in ms (HIP events on its stream; synchronises) */
int alore_backend_last_plan_ms(alore_backend_handle h, float *ms);

/* MSPlanner::get_the_predicted_state (optimizer.cpp:1108-1188) and get_the_predicted_state_and_path (:1190-1262) on the
 * plans of the last alore_backend_plan: the pose reached at time[b] by Simpson integration in steps of `resolution`
 * (trajPredictResolution) from start_time[b] (NULL: 0) and start_xytheta[b] (NULL: the plan's start pose), the flat
 * derivatives there (vaj = v, a, j of the arc length; oaj = omega, alpha, jerk of the yaw) and the reference's
 * if_forward flag.  HOST pointers, [count] / [count][3]; outputs may be NULL. */
int alore_backend_predicted_state(alore_backend_handle h, int count, double resolution, const double *start_time, const double *time,
                                  const double *start_xytheta, double *xytheta, double *vaj, double *oaj, int *forward);

/* MSPlanner::mincoPointPub (optimizer.cpp:1714-1826) on the plans of the last alore_backend_plan: the optimised path as the
 * marker points the reference publishes for the ALORE FSM to follow -- per piece `panels_per_piece` Simpson panels of the
 * planar velocity ((int)(sparseResolution * 0.4) in the reference), accumulated from the plan's start position, the last
 * point of every piece twice.  HOST pointers: xy [count][max_pieces (panels_per_piece + 1)][2] (z = 0.15 in the marker),
 * yaw [count][max_pieces panels_per_piece] or NULL (the heading at the end of every panel: the reference computes it and
 * does not publish it), n_points [count] (n_pieces (panels_per_piece + 1); 0 for a slot whose plan the optimiser rejected).
 * Synchronises. */
int alore_backend_path_points(alore_backend_handle h, int count, int panels_per_piece, double *xy, double *yaw, int *n_points);
/* The same kernel on the caller's DEVICE slabs of the same shapes, in stream order: nothing is allocated, nothing is copied and
 * nothing waits.  A row is written up to its n_points only (alore_backend_path_points zeroes its slabs first: on zeroed slabs the
 * two leave the same bits).  d_xy with row stride max_pieces (panels_per_piece + 1) 16 bytes and d_n_points are what
 * alore_fsm_set_paths (alore_fsm.h) reads; max_pieces is the handle's rounded value (alore_backend_status). */
int alore_backend_path_points_device(alore_backend_handle h, int count, int panels_per_piece, double *d_xy, double *d_yaw_or_null,
                                     int *d_n_points, void *stream);

/* ---- stored plans against the map of now ------------------------------------------------------------- */
/* MSPlanner::check_final_collision (optimizer.cpp:474-571) again, on the plans of the last alore_backend_plan and the handle's
 * CURRENT map (alore_backend_set_map / alore_backend_build_esdf since then), one wavefront per plan, nothing but the records below
 * crosses the bus: what a replanner asks every cycle (plan_manager.hpp:714-727).  The path is integrated from the plan's start
 * position in final_check_num Simpson panels per piece; panel p = i R + q ends at tau_p = sum_{k<i} T_k + (q + 1) T_i / R and
 * COUNTS for robot b when its interval (tau_p - T_i / R, tau_p] overlaps the open window (t_from[b], t_to[b]) -- the part of the
 * plan the robot has not driven yet.  The distance of a panel is the ESDF at the reference point at its end and, with body != 0,
 * the minimum over that point and the n_check body points placed like the optimiser's clearance penalty places them. */
typedef struct alore_backend_check {
    int collision;    /* 1: a counted panel is closer than the threshold */
    int first_panel;  /* the first such panel, or -1 */
    int n_checked;    /* counted panels up to and including the first hit (all counted panels without one) */
    int pad;
    double first_time;  /* tau of first_panel, or -1 */
    double first_xy[2]; /* reference point at the end of first_panel, or zeros */
    double min_dist;    /* over the n_checked panels (the reference stops at its first hit); DBL_MAX when nothing counts */
} alore_backend_check;
/* t_from, t_to: HOST arrays [count] or NULL (0 and +infinity); min_safe_dis <= 0: the configured final_min_safe_dis.  The launch
 * goes on `stream`; with out (HOST, [count]) the records are copied down and the stream is synchronised, with out == NULL nothing
 * waits and a consumer on the same GPU reads the slab of alore_backend_device_check in stream order.  A slot whose plan the
 * optimiser rejected is checked like any other (what is stored is its last pass).  A check on another stream than the one before it
 * starts after that one has ended (the handle keeps one argument block and one slab of records); a consumer of the slab on another
 * stream, and a map update or a new plan while a check is in flight on another stream, are the caller's to order. */
int alore_backend_check_plans(alore_backend_handle h, int count, const double *t_from, const double *t_to, double min_safe_dis, int body,
                              alore_backend_check *out, void *stream);
/* device slab [max_problems] of the records of the last check; valid until the handle is destroyed */
int alore_backend_device_check(alore_backend_handle h, const alore_backend_check **out);

/* ---- problems from way-point paths, on the device ----------------------------------------------------- */
/* What turns the front end's pruned polyline into FlatTrajData: getSampleTraj and getTrajsWithTime (front_end/src/jps_planner/
 * jps_planner.cpp:212-366) with the trapezoid of :378-441, one wavefront per path (csrc/flat_traj_build.h holds the arithmetic,
 * csrc/flat_traj_build.hip the kernel).  alore_front_end_default_params fills the values of jps3ms.yaml, global_planning3ms.yaml
 * and car3ms.yaml. */
typedef struct alore_front_end_params {
    double distance_weight, yaw_weight; /* jps_distance_weight, jps_yaw_weight */
    double traj_cut_length;             /* trajCutLength */
    double sample_time;                 /* timeResolution */
    int min_traj_num;                   /* mintrajNum */
    double max_vel, max_acc;
} alore_front_end_params;
void alore_front_end_default_params(alore_front_end_params *p);

/* `count` paths of up to max_points (<= 31) way-points each; arrays of HOST or DEVICE memory (alore_backend_set_paths says which) */
typedef struct alore_backend_paths {
    int max_points;          /* K: row length of xy */
    const int *n_points;     /* [count], 2 .. K */
    const double *xy;        /* [count][K][2]; rows are read up to n_points */
    const double *start_yaw; /* [count] */
    const double *end_yaw;   /* [count] */
    const double *start_vaj; /* [count][3] or NULL (zeros): v, a, j of the arc length at the start (v starts the trapezoid) */
    const double *start_oaj; /* [count][3] or NULL (zeros): omega, alpha, jerk of the yaw at the start */
} alore_backend_paths;

/* build status of a slot */
#define ALORE_BE_BUILD_OK 0
#define ALORE_BE_BUILD_MASKED 1         /* the mask left the slot out: nothing of it was touched */
#define ALORE_BE_BUILD_E_POINTS (-1)    /* fewer than 2 or more than K way-points: slot untouched */
#define ALORE_BE_BUILD_E_PIECES (-2)    /* more pieces than the handle was created for: slot untouched */

/* Builds the problems of slots 0..count-1 from the paths, in the layout alore_backend_set_problems uploads, and the launch order
 * (most pieces first, stable in the slot index), and sets the number of uploaded problems to count like alore_backend_set_problems.
 * fe NULL: the defaults.  mask NULL: every slot; otherwise slot b is rebuilt when the int at (char *)mask + b * mask_stride_bytes is
 * not 0 and left untouched when it is 0 -- with mask_stride_bytes = sizeof(alore_backend_check) the `collision` words of the slab of
 * alore_backend_device_check are a mask as they lie.  A path that does not build leaves its slot untouched; the outcome per slot
 * is in the build-status slab.
 * device_pointers == 0: the arrays of `p` and the mask are HOST memory; they are uploaded, the stream is synchronised, and the call
 * returns ALORE_BE_E_INVALID / ALORE_BE_E_UNSUPPORTED for the first slot that did not build (bad point count / too many pieces).
 * device_pointers != 0: they are DEVICE memory, read in stream order; nothing crosses the bus but the argument block, nothing is
 * allocated and nothing waits (a second call waits for the first one's argument block to have left the host, not for its kernel).
 * ORDERING.  Between this call and the next plan launch a rebuilt slot holds its new n_pieces and start pose next to the results of
 * its old plan: alore_backend_check_plans, alore_backend_predicted_state[_device], alore_backend_path_points and
 * alore_backend_results on such a slot in that window are the caller's to avoid (alore_backend_set_problems has the same window).
 * In a replan cycle, check and predict first, then set the paths, then plan.  With object classes (alore_backend_set_classes) a
 * handle's stored plans are checked and predicted with the table and the class indices of NOW: changing either between a plan and
 * its check is the caller's to avoid. */
int alore_backend_set_paths(alore_backend_handle h, int count, const alore_backend_paths *p, const alore_front_end_params *fe,
                            int device_pointers, const int *mask, int mask_stride_bytes, void *stream);
/* device slab [max_problems] of the build status of the last alore_backend_set_paths; valid until the handle is destroyed */
int alore_backend_device_build_status(alore_backend_handle h, const int **out);
/* the same copied to HOST memory out[count]; waits for the device */
int alore_backend_build_status(alore_backend_handle h, int count, int *out);
/* the launch order that alore_backend_set_problems / alore_backend_set_paths left on the device, copied to HOST memory out[count]
 * (count = the slots of that call): workgroup w of alore_backend_plan works on slot out[w] -- most pieces first, stable in the slot
 * index; waits for the device */
int alore_backend_launch_order(alore_backend_handle h, int count, int *out);
/* The problem slots as they lie on the device, copied to HOST arrays (any pointer may be NULL; P = max_pieces as rounded by the
 * handle, 16, 32 or 64): n_pieces [count], inner [count][(P-1)*2] (yaw, s), init_T [count], positions [count][P*2] (way-point xy,
 * then final xy), head / tail [count][6] ([yaw | s][p v a]), start_xytheta [count][3], final_xy [count][2], if_cut [count].
 * Waits for the device. */
int alore_backend_get_problems(alore_backend_handle h, int count, int *n_pieces, double *inner, double *init_T, double *positions,
                               double *head, double *tail, double *start_xytheta, double *final_xy, int *if_cut);

/* alore_backend_predicted_state with DEVICE inputs and outputs, on `stream`: no allocation, no copy, no synchronisation.
 * d_start_time and d_start_xytheta may be NULL (0 / the plan's start pose), as may any output but d_xytheta, d_vaj and d_oaj.
 * Its d_xytheta, d_vaj and d_oaj are the start pose and start_vaj / start_oaj of a replan from the predicted state
 * (plan_manager.hpp:587-588): alore_backend_set_paths reads them in stream order. */
int alore_backend_predicted_state_device(alore_backend_handle h, int count, double resolution, const double *d_start_time,
                                         const double *d_time, const double *d_start_xytheta, double *d_xytheta, double *d_vaj,
                                         double *d_oaj, int *d_forward, void *stream);

/* alore_backend_plan for the slots a DEVICE mask names (read like the mask of alore_backend_set_paths; NULL: every slot): the
 * workgroup of a slot whose mask word is 0 returns at entry, and the stored plan, status record and history of that slot stay
 * bit for bit.  Nothing waits: the argument block goes up from pinned memory (a second call waits for the first one's block to
 * have left the host). */
int alore_backend_plan_masked(alore_backend_handle h, int count, const int *mask, int mask_stride_bytes, void *stream);

/* The delivery mask of a replan cycle (check -> predict -> search -> set paths -> plan_masked), on DEVICE memory in stream order:
 * out_mask[b] = 1 where the last alore_backend_check_plans flags a collision AND the search status of slot b is
 * ALORE_BE_SEARCH_OK AND its build status is ALORE_BE_BUILD_OK AND its plan has ok != 0; else 0.  A flagged slot whose search or
 * build failed is planned again by alore_backend_plan_masked from its OLD problem: without this mask that plan would be delivered
 * to the controllers under a new start time (alore_nmpc_refs_set_pending_from_backend takes the mask as it lies).
 * A robot whose replan failed keeps its colliding trajectory: the reference goes to EMERGENCY_STOP there
 * (plan_manager.hpp:662-666); stopping it stays with the caller, who reads the collision words and this mask. */
int alore_backend_replan_mask(alore_backend_handle h, int count, int *out_mask, void *stream);

/* ---- object classes: one robot model per problem slot, mixed in one launch ---------------------------------------------- */
/* A batch of Monte-Carlo poses x object classes plans robots that differ in their model: the ICR offset, the speed and
 * acceleration limits, the footprint (check_pts), the clearance.  A handle carries a TABLE of whole configs and a CLASS INDEX per
 * problem slot, and every call that reads robot-model parameters reads them from the slot's class: alore_backend_plan,
 * _plan_masked, _eval and _lbfgs (an argument of _eval / _lbfgs -- safe_dis, time_weight, lam, rho, max_iter -- overrides the config
 * for every slot as before; the argument that stands for the configured value -- NULL for lam and rho, 0 for max_iter, NaN for
 * safe_dis and time_weight -- takes the class's), alore_backend_check_plans (xv,
 * n_check, check_pts, final_check_num, and final_min_safe_dis when min_safe_dis <= 0; with a table body != 0 is accepted even if
 * a class has no check points: such a slot checks the reference point alone), alore_backend_predicted_state[_device] and
 * alore_backend_path_points (icr_xv, standard_diff), and alore_backend_set_paths (the class's front-end parameters, below).
 * Everything slot b leaves behind equals bit for bit what a handle created with classes[class_of[b]] leaves for the same problem
 * on the same map, whatever the classes of its batch mates; a table of one class equal to the handle's config equals no table; a
 * handle without a table enqueues what it enqueued before there were classes.  csrc/backend_classes.h holds the arithmetic.
 * OUT OF SCOPE, on purpose: alore_backend_search_paths and alore_backend_task_plan keep their per-call safe_dis; the fleet
 * manager, the mission and the map calls read no robot model. */
#define ALORE_BE_MAX_CLASSES 256
/* Uploads the table (HOST pointers; the call synchronises the device).  A class is a complete alore_backend_config: limits, weights,
 * safe_dis, final_min_safe_dis, n_check / check_pts, icr_xv / standard_diff, ALM and L-BFGS parameters.  Every entry must pass the
 * checks of alore_backend_create, and the fields that size a device buffer or a launch must equal the handle's: sparse_res (the
 * L-BFGS history is sized for 256 slots whatever mem_size says, so mem_size may differ).  A class that fails gets
 * ALORE_BE_E_INVALID with an error text naming the class and the field, and the table of before stays.  fe: the front-end
 * parameters per class, [n_classes], or NULL: with them alore_backend_set_paths(fe == NULL) builds slot b with its class's (max_vel
 * and max_acc start the trapezoid, so a heavier class gets a longer init_T); a non-NULL fe argument there applies to every slot as
 * before.  n_classes: 1 .. ALORE_BE_MAX_CLASSES; 0 removes the table and the handle behaves as without one.  A slot whose index lies
 * outside the new table becomes class 0.  The first call allocates for ALORE_BE_MAX_CLASSES classes; no later call allocates. */
int alore_backend_set_classes(alore_backend_handle h, int n_classes, const alore_backend_config *classes,
                              const alore_front_end_params *fe);
/* The class of slots 0..count-1: an attribute of the slot (the robot) that survives alore_backend_set_problems, _set_paths and
 * plans; slots never set are class 0.  device_pointer == 0: class_of is HOST memory; an index outside [0, n_classes) (outside
 * [0, 1) without a table) is ALORE_BE_E_INVALID and nothing is changed; the call synchronises the stream.  device_pointer != 0:
 * DEVICE memory read in stream order by a small kernel, nothing waits; the kernel clamps an index into the table (below 0: class 0,
 * beyond it: the last class) and adds the number it clamped to the counter of the view below. */
int alore_backend_set_problem_classes(alore_backend_handle h, int count, const int *class_of, int device_pointer, void *stream);
/* per class, the outcome of the slots 0..count-1 as their status records lie (the last plan launch; slots a masked launch left out
 * keep the record of their last plan).  Integer sums, minima and maxima only: the result does not depend on the order. */
typedef struct alore_backend_class_stat {
    int n;                /* slots of the class */
    int n_ok;             /* ok != 0 */
    int n_collision;      /* collision != 0 */
    int sum_attempts;
    long long sum_evals;
    int max_evals;
    int pad;
    double min_dist;      /* minimum of min_dist over the slots with ok != 0; DBL_MAX without one */
    double max_duration;  /* maximum over the same slots of the plan's duration, the sum of its piece times in piece order; 0 without one */
} alore_backend_class_stat; /* 48 bytes */
/* device addresses, valid until the handle is destroyed (the first of the four calls of this section allocates them) */
typedef struct alore_backend_class_view {
    int n_classes;                            /* 0 without a table */
    int pad;
    const int *class_of;                      /* [max_problems] */
    const double *xv;                         /* [max_problems] the effective ICR offset of every slot: 0 for a standard_diff class,
                                                 else icr_xv; kept up to date by the two calls above; what the store hand-over reads
                                                 (alore_nmpc_refs_set_from_backend_xv) */
    const int *clamped;                       /* one int: indices the device route had to clamp, summed over its calls */
    const alore_backend_config *classes;      /* [n_classes]; NULL without a table */
    const alore_backend_class_stat *stats;    /* [max(n_classes, 1)] the records of the last alore_backend_class_stats */
} alore_backend_class_view;
int alore_backend_device_classes(alore_backend_handle h, alore_backend_class_view *out);
/* One kernel on `stream`, one workgroup per class.  out (HOST, [max(n_classes, 1)]) NULL: nothing waits and the records stay in the
 * slab of the view; otherwise they are copied down and the stream is synchronised.  Without a table: one class, every slot. */
int alore_backend_class_stats(alore_backend_handle h, int count, alore_backend_class_stat *out, void *stream);

/* ---- the resident occupancy map: point clouds in, ESDF out, on the device ------------------------------------- */
/* The half of plan_env::SDFmap that runs before updateESDF2d (sdf_map.cpp: updateOccupancyCallback :35-130, raycastProcess
 * :132-175, updateOccupancyMap :281-314, RemoveOutliers :316-350), then updateESDF2d itself, on a map that stays on the device:
 * occupancy log-odds, the cell-state grid (0 unknown, 1 unoccupied, 2 occupied) and the distance field are updated in place, and
 * the distance field is the map that alore_backend_plan, alore_backend_plan_masked and alore_backend_check_plans read.  Grids are
 * [nx][ny], cell (ix, iy) at ix * ny + iy, x_hi = x_lo + nx * res.  csrc/occupancy_update.h holds the arithmetic and lists the
 * deviations from the reference (int counts, non-finite points skipped, a sensor outside the map refused, no access outside the
 * map at its edge).  Out of scope: cirSupRaycastProcess (off in both launch files), TF lookups and PCL conversion (the caller hands
 * over points in the world frame).  The laser simulator that makes the clouds is the alore_backend_laser_* section below, the front
 * end's search on this map alore_backend_search_paths after it. */
typedef struct alore_backend_map_params {
    double p_hit, p_miss, p_min, p_max, p_occ; /* probabilities in (0, 1); their logits are the log-odds of the update */
    double detection_range;
    int perspective;                           /* if_perspective: 0 raycast and log-odds, 1 window free and points occupied */
} alore_backend_map_params;
/* 0.99, 0.35, 0.12, 0.90, 0.80 (plan_env/config/mapsim.yaml), 27.0 and 1 (planner_sim.launch) */
void alore_backend_map_default_params(alore_backend_map_params *p);
/* Allocates, once: the state grid (all unknown), the log-odds (clamp_min - 0.01, sdf_map.h:179-180), two count arrays, the
 * distance field (DBL_MAX) as the handle's map, the ESDF workspace for the largest window of this geometry and detection range,
 * and a pinned argument block.  params NULL: the defaults.  Replaces a map set before.
 * A later alore_backend_set_map or alore_backend_build_esdf behaves exactly as without a resident map and ENDS it: the
 * alore_backend_map_* calls below return ALORE_BE_E_INVALID until the next alore_backend_map_create. */
int alore_backend_map_create(alore_backend_handle h, int nx, int ny, double x_lo, double y_lo, double res,
                             const alore_backend_map_params *params);
/* the log-odds as computed on the host, log(p / (1 - p)): hit, miss, min, max, occ */
int alore_backend_map_logodds(alore_backend_handle h, double out[5]);
/* seeds the state grid from a prior map: grid is HOST memory [nx][ny]; synchronises */
int alore_backend_map_set_grid(alore_backend_handle h, const unsigned char *grid);
/* one cloud with the pose it was taken at */
typedef struct alore_backend_scan {
    const float *points;    /* x, y of point i at (char *)points + i * point_stride_bytes: HOST or DEVICE memory (the call says) */
    int n_points;           /* may be 0: a cycle without rays */
    int point_stride_bytes; /* a multiple of 4, at least 8: 8 for x, y pairs, 12 for x, y, z, 16 for a PCL PointXYZ array */
    double odom[3];         /* x, y, yaw of the sensor in the world frame (HOST values: the pose arrives with the cloud) */
} alore_backend_scan;
/* The scans in order, each a full cycle of updateOccupancyCallback: in raycast mode the rays' counts, the log-odds update,
 * RemoveOutliers on the state grid of the previous cycle, the state update; in perspective mode the window and the points.  With
 * update_esdf != 0 every scan is followed by updateESDF2d in that scan's window, odom +- detection_range, as in the reference
 * (its distances depend on the window); a window of less than two cells a side is left out.  A scan whose sensor position is not
 * strictly inside the map makes the call return ALORE_BE_E_INVALID before anything is enqueued.  With fewer than 32768 rays
 * through one cell per scan the result is the reference's, which counts in shorts; beyond that (the sensor's cell of a cloud of
 * 32768 valid points or more) the reference's total wraps negative and the cell takes a hit update, here the count stays exact
 * and the cell is a miss.
 * device_points != 0: the points are DEVICE memory, read in stream order; nothing is allocated, nothing crosses the bus but the
 * argument block and nothing waits (a second call waits for the first one's block to have left the host, and so does every eighth
 * scan of one call).  The next alore_backend_check_plans or plan launch on the same stream sees the new map.
 * device_points == 0: the points are HOST memory; they are uploaded through a staging buffer that grows when needed, and the
 * stream is synchronised before the call returns. */
int alore_backend_map_integrate(alore_backend_handle h, int n_scans, const alore_backend_scan *scans, int device_points, int update_esdf,
                                void *stream);
/* updateESDF2d alone in a window of the caller's choice, odom +- detection_range (no larger than the map's own detection range:
 * the workspace is sized for that); asynchronous.  map_integrate and map_update_esdf share one ESDF workspace and one argument
 * block: each call waits on `stream` (a device-side wait, the host does not block) for the map_integrate or map_update_esdf
 * call before it, on whatever stream that ran, so the calls may use different streams.  They are not safe to issue from two host
 * threads at once, like every call on one handle.  Readers of the map on ANOTHER stream (check_plans, plan) must be ordered
 * after the update by the caller; map_set_grid and map_get synchronise the device. */
int alore_backend_map_update_esdf(alore_backend_handle h, double odom_x, double odom_y, double detection_range, void *stream);
/* copies to HOST arrays [nx][ny]; any pointer may be NULL; waits for the device */
int alore_backend_map_get(alore_backend_handle h, unsigned char *grid, double *log_odds, double *dist);
/* device pointers of the resident map and its geometry; valid until the map ends */
typedef struct alore_backend_map_view {
    unsigned char *grid;
    double *log_odds;
    double *dist;
    const int *count_hit, *count_all; /* the rays' counts of a scan in flight; zero between scans */
    int nx, ny;
    double x_lo, y_lo, res;
} alore_backend_map_view;
int alore_backend_map_device(alore_backend_handle h, alore_backend_map_view *out);

/* ---- laser scans of a resident world cloud, on the device ----------------------------------------------------- */
/* What produces the clouds that alore_backend_map_integrate reads: the reference's laser simulator
 * (utils/laser_simulator/src/laser_sim_node.cpp) holds the world as a point cloud and publishes, at every sensing tick, what a robot
 * at the current pose sees -- renderSensedPoints (:423-533), a range image over hrz x vtc laser lines with occlusion and the optional
 * resolution filter, or perspectivePoints (:343-421, what planner_sim.launch runs), every world point within the horizon.  Here the
 * world cloud stays on the device and one call renders the scans of a batch of poses, one workgroup per scan (csrc/laser_scan.hip).
 * The contract -- the order of every operation, the per-line sine and cosine tables computed once on the host, the deviations from
 * the reference (in range on the double sum; non-finite points and, in range mode, a point at the sensor skipped; the filter's
 * spread clamped in double and to one turn of the ring) -- is stated in csrc/laser_scan.h.  The fields are the node's parameters
 * (:540-581).  The voxel filter of rcvGlobalPointCloudCallBack is the caller's, as PCL conversion is elsewhere. */
typedef struct alore_backend_laser_params {
    double sensing_horizon, pc_resolution;
    int hrz_laser_line_num, vtc_laser_line_num;
    double vtc_laser_range_dgr;
    int hrz_limited;
    double hrz_laser_range_dgr;
    int use_resolution_filter;
    int if_perspective; /* 0 renderSensedPoints, 1 perspectivePoints */
} alore_backend_laser_params;
/* 27.0, 0.1, 360, 16, 30.0, 0, 90.0, 0, 1 (planner_sim.launch, config/perspective_laser.yaml); config/normal_laser.yaml, the
 * occluding sensor, has horizon 10.0, 360 x 2 lines over 10 degrees and the filter on */
void alore_backend_laser_default_params(alore_backend_laser_params *p);

#define ALORE_BE_LASER_MAX_BINS 8192
/* status of a scan */
#define ALORE_BE_LASER_OK 0
#define ALORE_BE_LASER_E_POSE (-1)     /* x, y or yaw is not finite: count 0, an empty image, NaN slots */
#define ALORE_BE_LASER_E_CAPACITY (-2) /* perspective mode: more points within the horizon than slots; n_points is the true count */

/* Allocates, once: the slabs of max_scans scans, the line tables and a pinned argument block.  A scan has hrz x vtc slots in range
 * mode and max_points_per_scan slots in perspective mode (where max_points_per_scan must be at least 1; range mode ignores it).
 * params NULL: the defaults.  ALORE_BE_E_INVALID before anything is allocated for vtc_laser_line_num < 2 (the reference divides by
 * zero), hrz_laser_line_num < 1, more than ALORE_BE_LASER_MAX_BINS bins, a horizon or resolution that is not positive and finite,
 * vtc_laser_range_dgr outside (0, 180), or hrz_limited with a horizontal range that is not positive.  Replaces a sensor created
 * before, cloud included. */
int alore_backend_laser_create(alore_backend_handle h, const alore_backend_laser_params *params, int max_scans, int max_points_per_scan);
/* The world cloud: x, y, z of point i are the three floats at (char *)points + i * stride_bytes (a multiple of 4, at least 12: 12
 * for triples, 16 for a PCL PointXYZ array).  n == 0 is legal (points may be NULL then); at most 2^30 points (the kernels index
 * them with an int).  device_points == 0: HOST memory, packed,
 * uploaded, and the stream is synchronised.  device_points != 0: DEVICE memory, copied in stream order; the device buffer grows
 * (with a device synchronisation) only when n exceeds every cloud set before. */
int alore_backend_laser_set_cloud(alore_backend_handle h, const float *points, int n, int stride_bytes, int device_points, void *stream);
/* Renders scans 0..count-1 (count <= max_scans): x, y, yaw of scan i are the three doubles at (char *)poses + i *
 * pose_stride_bytes (a multiple of 8, at least 24), so the d_xytheta [count][3] of alore_backend_predicted_state_device serves as
 * the poses as it lies.  Every scan gets a status (above) and a count; a scan that fails leaves the others as they are.
 * device_poses != 0: DEVICE memory read in stream order; nothing is allocated, nothing crosses the bus but the argument block and
 * nothing waits (a second call waits for the first one's block to have left the host).  device_poses == 0: HOST memory; the poses
 * go up with the argument block and the stream is synchronised before the call returns.  The return value speaks of the call,
 * not of the scans: read their status.  Without alore_backend_laser_create or alore_backend_laser_set_cloud: ALORE_BE_E_INVALID.
 * The argument block on the device and the slabs are the handle's: successive calls must be ordered on the device (one stream, or
 * events), as for alore_backend_search_paths. */
int alore_backend_laser_scan(alore_backend_handle h, int count, const double *poses, int pose_stride_bytes, int device_poses, void *stream);
/* The device slabs, scan i at row i; valid until the next alore_backend_laser_create or the end of the handle.
 * Range mode: range_image [max_scans][bins] (bins = hrz x vtc, bin (x, y) at x * vtc + y, 9999.0 where nothing was hit);
 * laser_points and world_points [max_scans][slots][3], slot = bin, three NaN where the bin was not hit; n_points the number of hit
 * bins; index [max_scans][slots] the hit bins in x-major order (the reference's message), -1 from n_points on; compact_points
 * [max_scans][slots][3] their laser-frame points in that order, NaN from n_points on.
 * Perspective mode: laser_points (rot^T (p - t)) and world_points (the source point) [max_scans][slots][3] and index (the source
 * index) for the n_points points within the horizon in no particular order, NaN and -1 beyond; range_image is NULL and
 * compact_points is laser_points.
 * Scan i goes into alore_backend_map_integrate(device_points = 1) as alore_backend_scan{points = world_points + i * slots * 3,
 * n_points = slots, point_stride_bytes = 12}: non-finite points are skipped there. */
typedef struct alore_backend_laser_view {
    double *range_image;
    float *laser_points, *world_points;
    int *index;
    float *compact_points;
    int *n_points, *status;
    int slots, bins, max_scans;
} alore_backend_laser_view;
int alore_backend_device_laser(alore_backend_handle h, alore_backend_laser_view *out);
/* The slabs of scans 0..count-1 copied to HOST arrays of the shapes above with count for max_scans (any pointer may be NULL;
 * range_image is not written in perspective mode).  Waits for the device. */
int alore_backend_get_laser(alore_backend_handle h, int count, double *range_image, float *laser_points, float *world_points, int *index,
                            float *compact_points, int *n_points, int *status);

/* ---- way-point paths by grid search on the handle's map, on the device ---------------------------------------- */
/* What produces the paths that alore_backend_set_paths reads: per problem a shortest 8-connected path from a start to a goal over
 * the cells whose distance is at least a safe distance, pruned by line of sight -- JPSPlanner::plan and removeCornerPts
 * (front_end/src/jps_planner/jps_planner.cpp:31-68, 97-177, graph_search.cpp:92-243).  The reference's JPS returns one of several
 * equal-cost paths, which one depends on its heap; here the path is fixed by a contract with exactly one answer, stated in
 * csrc/path_search.h: the cost is optimal on the reference's graph (eight moves, only the destination must be free, 1 or sqrt 2),
 * kept as an exact pair (a, b) = a + b sqrt 2; among equal-cost paths the walk from the start keeps its direction when it can and
 * otherwise takes the first of (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1); the pruning is removeCornerPts' arithmetic.
 * The safe distance is the reference's (safe_dis capped by 0.8 times the distance at either end cell, not below 0).  The search
 * stays in a window: the bounding box of the two cells grown by ceil(window_margin / res) cells a side, clipped to the map, at most
 * ALORE_BE_SEARCH_MAX_CELLS cells.  Deviations: an end point outside the map or not finite is refused (the reference clamps), equal
 * end cells are refused (the reference hands on a one-point path).  One workgroup per problem, the field of the window in LDS
 * (csrc/path_search.hip).
 * LARGER WINDOWS are opt-in: after alore_backend_search_reserve(h, max_cells, slots) a slot whose window has more than
 * ALORE_BE_SEARCH_MAX_CELLS and at most max_cells cells is searched by a second kernel behind the first on the same stream, which
 * keeps the field in one of the reservation's `slots` slabs in device memory and relaxes it tile by tile in LDS
 * (csrc/path_search_wide.h, csrc/path_search_wide.hip).  The contract is the same and so is the answer, bit for bit; slots of at
 * most ALORE_BE_SEARCH_MAX_CELLS cells take the first kernel as before.  One more status exists on that route only,
 * ALORE_BE_SEARCH_E_RANGE: a cost is the pair (a, b) in 16 bits each, ordered exactly while both stay below 32768, which a window
 * of 32768 cells guarantees and one of 4 M cells does not; a slot in whose window the goal reaches a cell whose least cost has
 * a >= 32767 or b >= 32767 (a route of more than 3 km at 0.1 m) fails with it, whatever its own path.  alore_backend_task_plan
 * takes no part in the reservation and keeps ALORE_BE_TASK_E_WINDOW at ALORE_BE_SEARCH_MAX_CELLS.
 * alore_backend_task_plan has a reservation of its own, alore_backend_task_reserve (below): with it a mission whose window has more
 * than ALORE_BE_SEARCH_MAX_CELLS cells has its cost fields on that reservation's slabs, by the same tiles.  The legs of such a
 * mission are searched afterwards only on a handle that also has a search reservation large enough for them. */
typedef struct alore_backend_search_params {
    double safe_dis;      /* jps_safe_dis */
    double window_margin; /* metres round the bounding box of start and goal */
} alore_backend_search_params;
/* 0.3 (front_end/config/jps3ms.yaml) and 3.0 */
void alore_backend_search_default_params(alore_backend_search_params *p);

#define ALORE_BE_SEARCH_MAX_CELLS 32768
/* search status of a slot */
#define ALORE_BE_SEARCH_OK 0
#define ALORE_BE_SEARCH_MASKED 1          /* the mask left the slot out: nothing of it was touched, n_points included */
#define ALORE_BE_SEARCH_E_ENDPOINT (-1)   /* a coordinate is not finite or outside [lo, hi] of the map */
#define ALORE_BE_SEARCH_E_SAME_CELL (-2)  /* start and goal lie in one cell */
#define ALORE_BE_SEARCH_E_WINDOW (-3)     /* the window has more than ALORE_BE_SEARCH_MAX_CELLS cells, or more than the reservation */
#define ALORE_BE_SEARCH_E_NO_PATH (-4)    /* an end cell is not free, or the goal cannot be reached inside the window */
#define ALORE_BE_SEARCH_E_POINTS (-5)     /* more than 1024 raw nodes, or more than 31 way-points after pruning */
#define ALORE_BE_SEARCH_E_RANGE (-6)      /* wide route only: a cost in the window has a component of 32767 or more; decided after the
                                             field, before the walk (so before its E_NO_PATH and E_POINTS) */

/* Reserves device memory for searches on windows of more than ALORE_BE_SEARCH_MAX_CELLS cells: `slots` slabs of max_cells words.
 * max_cells in (32768, 1 << 22], slots in [1, 1024], slots * max_cells * 4 <= 1 GiB, else ALORE_BE_E_INVALID; a second call
 * replaces the first (waits for the stream of the last search); max_cells = 0 releases it.  No map is needed yet.  `slots` is
 * the number of wide slots searched at a time (one workgroup each); a call with more of them takes them in turn. */
int alore_backend_search_reserve(alore_backend_handle h, int max_cells, int slots);
int alore_backend_search_reserved(alore_backend_handle h, int *max_cells, int *slots);   /* 0, 0 without one */

/* Searches slots 0..count-1 on the handle's current map (resident, or set by alore_backend_set_map / alore_backend_build_esdf;
 * without one: ALORE_BE_E_INVALID).  x, y of slot b are the two doubles at (char *)start_xy + b * start_stride_bytes, likewise the
 * goal (strides: multiples of 8, at least 16): the d_xytheta [count][3] of alore_backend_predicted_state_device serves as the
 * starts as it lies, with stride 24.  params NULL: the defaults.  The mask is read as alore_backend_set_paths reads its mask.
 * A slot that succeeds has 2 .. 31 way-points in the slab of alore_backend_device_paths, the first the given start and the last
 * the given goal, and status 0; a slot that fails has n_points = 0, its xy row untouched and a negative status, so
 * alore_backend_set_paths on the slab refuses it with ALORE_BE_BUILD_E_POINTS and its stored plan stays as it is.
 * device_pointers != 0: start_xy, goal_xy and mask are DEVICE memory read in stream order; nothing is allocated, nothing crosses
 * the bus but the argument block and nothing waits (a second call waits for the first one's block to have left the host).
 * device_pointers == 0: they are HOST memory; they are uploaded, the stream is synchronised, and the call returns, for the first
 * slot that failed, ALORE_BE_E_INVALID (end point, same cell, no path) or ALORE_BE_E_UNSUPPORTED (window, points, range).
 * With a reservation (alore_backend_search_reserve) both forms enqueue the second kernel too: a slot whose window has more than
 * ALORE_BE_SEARCH_MAX_CELLS and at most the reserved number of cells gets a searched path or one of the negative statuses above
 * instead of ALORE_BE_SEARCH_E_WINDOW, a larger window stays ALORE_BE_SEARCH_E_WINDOW; the device-pointer form still allocates
 * nothing, waits for nothing and moves only the argument block, and the host form's return code is taken after both kernels. */
int alore_backend_search_paths(alore_backend_handle h, int count, const double *start_xy, int start_stride_bytes, const double *goal_xy,
                               int goal_stride_bytes, const alore_backend_search_params *params, int device_pointers, const int *mask,
                               int mask_stride_bytes, void *stream);
/* The handle's device slab of searched paths [max_problems]: max_points = 31, n_points and xy are set; start_yaw, end_yaw,
 * start_vaj and start_oaj are NULL for the caller to fill, then the struct goes into alore_backend_set_paths with
 * device_pointers = 1.  Valid until the handle is destroyed. */
int alore_backend_device_paths(alore_backend_handle h, alore_backend_paths *out);
/* device slab [max_problems] of the search status of the last alore_backend_search_paths */
int alore_backend_device_search_status(alore_backend_handle h, const int **out);
/* the same copied to HOST memory out[count]; waits for the device */
int alore_backend_search_status(alore_backend_handle h, int count, int *out);
/* The searched paths copied to HOST arrays (any pointer may be NULL): n_points [count], xy [count][31][2], cost_ab [count][2] (the
 * cost a + b sqrt 2 of the unpruned path; written by slots that succeeded).  Waits for the device. */
int alore_backend_get_paths(alore_backend_handle h, int count, int *n_points, double *xy, int *cost_ab);
/* diagnostic: sweeps over the window until the field stood still, per slot of the last search; for a slot searched on the wide
 * route the number of visits of tiles instead; HOST out[count]; waits */
int alore_backend_search_sweeps(alore_backend_handle h, int count, int *out);
/* diagnostic, with a reservation only: HOST out[count][2], ticks of the device's 100 MHz clock that a slot took on the wide route
 * and the part of them in its walk and pruning; a slot that did not take the wide route keeps what it had (0 at first); waits */
int alore_backend_search_wide_ticks(alore_backend_handle h, int count, long long *out);

/* ---- the visit order of rearrangement missions from path costs on the handle's map, on the device --------------------- */
/* What plan_manager does before any trajectory is planned (plan_manager.hpp:210-250): the grid-path length between the robot, n
 * items and n targets, then the order of the visits -- solvePathWithGreedy (:347-432, the reference's live call) or the
 * fixed-assignment routing of BranchAndBoundCombined::solve (:252-345, branch_and_bound.hpp).  The contract, with exactly one answer
 * for the cost matrix and for both orders, is stated in csrc/task_plan.h.  A mission has P = 1 + 2 n points: 0 the robot, 1..n the
 * items, n+1..2n the targets.  d(i, j) is the least cost a + b sqrt 2 on the search's graph between the cells of points i and j
 * inside the MISSION's window (the bounding box of all P cells grown by ceil(window_margin / res) cells a side, clipped, at most
 * ALORE_BE_SEARCH_MAX_CELLS cells) with the pair's safe distance, as the exact pair (a, b); (0, 0) for equal cells, (-1, -1) where
 * there is no path.  Costs are added and ordered exactly, in integers.  Deviations from the reference: the window (the reference
 * searches the whole map); a point outside the map is refused, not clamped; the optimal mode returns, among optimal orders, the
 * lexicographically smallest item sequence (the reference's best-first search returns an optimum); a leg searched afterwards by
 * alore_backend_search_paths uses that pair's own smaller window, so its cost_ab can exceed the matrix entry.  Two kernels
 * (csrc/task_plan.hip): one workgroup per (mission, source point) fills the matrices, one cost-to-source field serving every
 * other point of the mission; one workgroup per mission then finds the order.
 * Two further modes choose the item-to-target assignment on the device, which the optimal mode takes from the caller (the
 * reference ships hungarian.hpp for it and a fixed_assignment argument, plan_manager.hpp:273-306, and calls neither).
 * ALORE_BE_TASK_ASSIGNED: the bijection of items to targets with the least sum of carry legs d(item i, target sigma(i)), among
 * those the lexicographically smallest vector (sigma(0), sigma(1), ...), then exactly the optimal mode's routing for it.  The
 * assignment is decided on the carry legs ALONE: if its routing has no finite order the mission is ALORE_BE_TASK_E_NO_ORDER, even
 * where another bijection could be routed.  ALORE_BE_TASK_JOINT: assignment and order together, the least cost of the whole route
 * over all item orders and all bijections, for at most ALORE_BE_TASK_JOINT_MAX_TASKS tasks per mission (max_tasks of the launch
 * may still be 10); among optimal routes the lexicographically smallest published order (item, target, item, target, ...).
 * Neither mode reads assignment_or_null.  Both write everything the optimal mode writes, in the same way, and the two rows of
 * alore_backend_task_assign_view. */
#define ALORE_BE_TASK_MAX_TASKS 10
#define ALORE_BE_TASK_MAX_POINTS 21 /* 1 + 2 * ALORE_BE_TASK_MAX_TASKS */
#define ALORE_BE_TASK_MAX_LEGS 20
#define ALORE_BE_TASK_GREEDY 0
#define ALORE_BE_TASK_OPTIMAL 1
#define ALORE_BE_TASK_ASSIGNED 2        /* least carrying distance, then the optimal order for that assignment */
#define ALORE_BE_TASK_JOINT 3           /* assignment and order together; n <= ALORE_BE_TASK_JOINT_MAX_TASKS */
#define ALORE_BE_TASK_JOINT_MAX_TASKS 5
/* task status of a mission */
#define ALORE_BE_TASK_OK 0
#define ALORE_BE_TASK_MASKED 1          /* the mask left the mission out: only its status was written */
#define ALORE_BE_TASK_E_ENDPOINT (-1)   /* a point of the mission is not finite or outside [lo, hi] of the map */
#define ALORE_BE_TASK_E_WINDOW (-3)     /* the mission's window has more than ALORE_BE_SEARCH_MAX_CELLS cells, or more than the reservation */
#define ALORE_BE_TASK_E_TASKS (-6)      /* n outside 1..max_tasks, (optimal mode) an assignment that is no permutation, (joint mode) n > 5 */
#define ALORE_BE_TASK_E_NO_ORDER (-7)   /* optimal and joint mode: no order has a finite cost; assigned mode: no assignment has a finite
                                           sum of carry legs, or the one chosen has no finite order (the matrix is written) */
#define ALORE_BE_TASK_E_RANGE (-8)      /* wide missions only (alore_backend_task_reserve): a cost field of the mission has a reached
                                           cell whose cost has a component of 32767 or more; decided after the matrix and before
                                           any ordering, so before ALORE_BE_TASK_E_NO_ORDER (-6 is ALORE_BE_TASK_E_TASKS here) */
typedef struct alore_backend_task_params {
    double safe_dis;      /* jps_safe_dis */
    double window_margin; /* metres round the bounding box of the mission's points */
    int mode;             /* ALORE_BE_TASK_GREEDY, _OPTIMAL, _ASSIGNED or _JOINT */
} alore_backend_task_params;
/* 0.3, 3.0 and ALORE_BE_TASK_GREEDY */
void alore_backend_task_default_params(alore_backend_task_params *p);
/* Plans missions 0..count-1 (count <= max_problems) on the handle's current map.  Mission m has n_tasks[m] tasks, 1..max_tasks
 * (max_tasks <= ALORE_BE_TASK_MAX_TASKS); its points are packed at the beginning of a row of 1 + 2 max_tasks (x, y) pairs at
 * (char *)points + m * point_row_stride_bytes (a multiple of 8, at least 16 (1 + 2 max_tasks)).  assignment_or_null:
 * [count][max_tasks] ints, item i of mission m goes to target assignment[m * max_tasks + i]; read in the optimal mode only (the
 * assigned and joint modes choose their own and read it neither for values nor for validity); NULL: the identity.  params NULL: the defaults.  The mask is read as alore_backend_search_paths reads its mask.
 * A failed mission has a negative status and n_order = 0, nothing else of it is written (ALORE_BE_TASK_E_NO_ORDER: its matrix and
 * diagnostics are).  device_pointers != 0: n_tasks, points, assignment and mask are DEVICE memory read in stream order; nothing
 * crosses the bus but the argument block and nothing waits.  device_pointers == 0: they are HOST memory; they are uploaded, the
 * stream is synchronised, and the call returns, for the first mission that failed, ALORE_BE_E_INVALID (tasks, end point, no order)
 * or ALORE_BE_E_UNSUPPORTED (window, range); the error text of such a return begins with "task_plan: mission failed", every other error means
 * that nothing was launched and the slab is as it was.
 * Successive calls on one handle must be ordered on the device, on one stream or by events: the argument block on the device is the
 * handle's, and a call overwrites it while the kernels of an earlier call on an unordered stream may still read it.
 * MISSIONS ON LARGER WINDOWS are opt-in: after alore_backend_task_reserve(h, max_cells, slots) a mission whose window has more than
 * ALORE_BE_SEARCH_MAX_CELLS and at most max_cells cells is planned like any other, a larger one stays ALORE_BE_TASK_E_WINDOW.  A
 * third kernel (csrc/task_plan.hip: task_costs_wide_kernel, `slots` workgroups) runs between the two and computes the fields of such
 * missions in the reservation's slabs, tile by tile as the wide search does (csrc/path_search_wide.h); the matrix, the orders of
 * all four modes, the tie rules, legs, `fields`, masked and failed missions are as above, bit for bit what the contract says.
 * `sweeps` of such a mission is the most visits of tiles any of its fields needed.  One status exists on that route only,
 * ALORE_BE_TASK_E_RANGE: a field is rooted at the cell of the LOWER-indexed point of a pair (source k, for the targets j > k, one
 * field per distinct safe distance); if any field of the mission reaches a cell whose least cost has a >= 32767 or b >= 32767 the
 * mission fails with it after the matrix and before any ordering, in every mode: status, n_order = 0, fields and sweeps are
 * written, its matrix rows are unspecified, order, total, legs and the assignment rows untouched.  Without that status every
 * entry has both components below 32767, so sums of twenty legs stay exact as stated above.  Missions of at most
 * ALORE_BE_SEARCH_MAX_CELLS cells take the first kernel as before and keep their bits.  The device-pointer form still allocates
 * nothing, waits for nothing and moves only the argument block; the host form's return code is taken after all kernels. */
int alore_backend_task_plan(alore_backend_handle h, int count, int max_tasks, const int *n_tasks, const double *points,
                            int point_row_stride_bytes, const int *assignment_or_null, const alore_backend_task_params *params,
                            int device_pointers, const int *mask, int mask_stride_bytes, void *stream);
/* Diagnostic: launches the order phase of the last alore_backend_task_plan call of this handle again, alone, on the matrices that
 * lie in the slab, with that call's arguments (for device_pointers != 0 its inputs must still be as they were); it writes what that
 * call wrote.  Nothing waits.  What tools/task_assign.py times the order kernels with. */
int alore_backend_task_reorder(alore_backend_handle h, void *stream);
/* Reserves device memory for missions on windows of more than ALORE_BE_SEARCH_MAX_CELLS cells: `slots` slabs of max_cells words,
 * this call's own (alore_backend_search_reserve's slabs stay the search's).  max_cells in (32768, 1 << 22], slots in [1, 1024],
 * slots * max_cells * 4 <= 1 GiB, else ALORE_BE_E_INVALID; a second call replaces the first (waits for the stream of the last
 * alore_backend_task_plan); max_cells = 0 releases it.  No map is needed yet.  `slots` is the number of (mission, source point)
 * pairs whose fields are computed at a time (one workgroup each); a call with more of them takes them in turn. */
int alore_backend_task_reserve(alore_backend_handle h, int max_cells, int slots);
int alore_backend_task_reserved(alore_backend_handle h, int *max_cells, int *slots);   /* 0, 0 without one */
/* diagnostic, with a task reservation only: HOST out[count][ALORE_BE_TASK_MAX_LEGS], per mission and source point the ticks of the
 * device's 100 MHz clock that its fields took on the wide route; a source that did not take it keeps what it had (0 at first); waits */
int alore_backend_task_wide_ticks(alore_backend_handle h, int count, long long *out);
/* The handle's device slab of the missions [max_problems].  Leg l of every mission goes into alore_backend_search_paths
 * (device_pointers = 1) as it lies: start_xy = leg_start_xy + 2 l, goal_xy = leg_goal_xy + 2 l, both strides
 * ALORE_BE_TASK_MAX_LEGS * 16 bytes.  Rows of order and of the legs beyond n_order are left untouched. */
typedef struct alore_backend_task_view {
    int max_points, max_legs; /* 21, 20 */
    const int *status;        /* [.] */
    const int *matrix;        /* [.][21][21][2]: (a, b) of d(i, j) for i, j < P */
    const int *order;         /* [.][20]: item index, target index, alternately, each 0-based in its own group */
    const int *n_order;       /* [.] */
    const int *total;         /* [.][2]: the cost of the whole route */
    const double *leg_start_xy, *leg_goal_xy; /* [.][20][2] */
    const int *fields;        /* [.] diagnostic: cost fields computed for the mission */
    const int *sweeps;        /* [.] diagnostic: the most sweeps any of them needed */
} alore_backend_task_view;
int alore_backend_device_task(alore_backend_handle h, alore_backend_task_view *out);
/* The slab copied to HOST arrays with the shapes above and [count] rows (any pointer may be NULL).  Waits for the device. */
int alore_backend_get_task(alore_backend_handle h, int count, int *status, int *matrix, int *order, int *n_order, int *total,
                           double *leg_start_xy, double *leg_goal_xy, int *fields, int *sweeps);
/* The assignment that ALORE_BE_TASK_ASSIGNED or ALORE_BE_TASK_JOINT chose, a slab of its own beside the one above.  A mission with
 * status ALORE_BE_TASK_OK in one of these modes writes both rows; so does, in the assigned mode, a mission whose assignment is
 * finite and whose routing is not (ALORE_BE_TASK_E_NO_ORDER).  Every other failure, a masked mission and every launch in the greedy
 * or optimal mode leave them untouched. */
typedef struct alore_backend_task_assign_view {
    const int *assignment;   /* [.][10]: the target of item i, i < n; entries beyond n are untouched */
    const int *assign_total; /* [.][2]: (a, b) of the sum of the carry legs d(item i, target assignment[i]) */
} alore_backend_task_assign_view;
int alore_backend_device_task_assign(alore_backend_handle h, alore_backend_task_assign_view *out);
/* Both rows copied to HOST arrays [count][10] and [count][2] (either pointer may be NULL).  Waits for the device. */
int alore_backend_get_task_assign(alore_backend_handle h, int count, int *assignment, int *assign_total);

/* ---- the edits a mission makes to the resident map: item and target footprints, on the device -------------------------- */
/* What plan_manager does to its map while a mission runs (plan_manager.hpp: paintSquare / paintBox / paintTable / paintChair
 * :470-496, MapUpdateThread :498-554, MainThread :618-658 and :695-704; sdf_map.cpp setObs / setFree :485-509): the items are
 * painted into the occupancy grid as obstacles, an item's square is freed when the robot comes near, a target's square is locked
 * when the robot delivers there, a target just left is locked after the next plan.  csrc/mission_map.h holds the arithmetic,
 * csrc/mission_map.hip the kernels.  An edit is the reference's double loop
 *     for (x = cx - hx; x <= cx + hx; x += res) for (y = cy - hy; y <= cy + hy; y += res) setObs / setFree (x, y)
 * and three details of it decide cells: the lattice is ACCUMULATED in double (x += res, not cx - hx + i * res); setObs / setFree
 * NARROW the coordinate to float, compare the float with the double bounds (< lo or >= hi: the point is skipped) and index with
 * (int)((coord - lo) * inv), so the cells of an edit are neither a contiguous range nor one per lattice point; ONLY THE STATE GRID
 * is written (2 occupied for make_obs != 0, else 1 unoccupied), log-odds and counts stay.  Deviations: an index that rounding
 * takes to n is clamped to n - 1 (the reference writes out of bounds), and the validity rule below. */
typedef struct alore_backend_map_edit {
    double cx, cy, hx, hy;
    int make_obs;
    int reserved; /* 0 */
} alore_backend_map_edit; /* 40 bytes */
/* Applies the edits to the state grid of the resident map AS IF ONE AFTER THE OTHER IN LIST ORDER: where a free and a lock overlap
 * the later one wins.  The call also leaves, in six device ints of the handle (alore_backend_device_paint_counters): n_changed, the
 * number of cells whose state after the call differs from before it; min_x, min_y, max_x, max_y, the box of those cells (nx, ny,
 * -1, -1 without one); n_skipped.  A DEVICE edit is skipped and counted when a field is not finite, a half size is negative, or it
 * has more than 64 lattice points on an axis ((int)(2 h / res) + 2 > 64).
 * device_edits == 0: `edits` is HOST memory of n_or_capacity edits and d_count is ignored; a list with an edit that would be
 * skipped is refused with ALORE_BE_E_INVALID before anything is enqueued; the list is uploaded (the staging buffer grows when
 * needed) and the stream is synchronised.
 * device_edits != 0: `edits` is DEVICE memory of n_or_capacity entries and so is the length, *d_count: entries at and beyond
 * min(*d_count, n_or_capacity) are never read into the map.  Nothing waits and nothing but the arguments crosses the bus; nothing
 * is allocated after the handle's first paint call or alore_backend_mission_create (8192 descriptors and the counters).
 * A list of more than 8192 edits is cut into launches in list order; later-wins holds across them, the counters then add up per
 * launch (a cell one launch changes and a later one changes back counts twice, and is in the box).
 * The ESDF is NOT part of the call: enqueue alore_backend_map_update_esdf behind it on the same stream in the window you want (the
 * reference calls updateESDF2d after each group of edits).  Calls on one handle must be ordered on the device, as for
 * alore_backend_search_paths; so must a map_integrate or map_update_esdf on another stream.  Without a resident map:
 * ALORE_BE_E_INVALID. */
int alore_backend_map_paint(alore_backend_handle h, const alore_backend_map_edit *edits, int n_or_capacity, const int *d_count,
                            int device_edits, void *stream);
/* the six device ints above; valid until the handle is destroyed.  ALORE_BE_E_INVALID before the first paint call */
int alore_backend_device_paint_counters(alore_backend_handle h, const int **out);
/* the same copied to HOST memory; waits for the device */
int alore_backend_map_paint_counters(alore_backend_handle h, int out[6]);

/* Mission state: one mission slot per problem slot of the handle (max_problems), up to ALORE_BE_TASK_MAX_TASKS tasks each.  ALL
 * missions edit the handle's ONE map: the fleet form of the reference's one robot with its own map -- a robot sees the items of
 * every other robot as obstacles, and the edits of a call are applied in slot order. */
typedef struct alore_backend_mission_params {
    double item_half;        /* 0.5  items -> OBS, plan_manager.hpp:518 */
    double free_half;        /* 0.5  :533 */
    double item_free_dist;   /* 2.0  :531 */
    double target_lock_half; /* 0.3  :547 */
    double target_lock_dist; /* 0.5  :545 */
    double left_target_half; /* 0.2  :700 */
    double left_target_dist; /* 0.3  :699 */
} alore_backend_mission_params;
void alore_backend_mission_default_params(alore_backend_mission_params *p);
/* status of a mission */
#define ALORE_BE_MISSION_OK 0
#define ALORE_BE_MISSION_MASKED 1      /* the slot was never set: a mask that leaves a slot out leaves ALL of it, this word included */
#define ALORE_BE_MISSION_E_POINT (-1)  /* a coordinate of an item or target is not finite */
#define ALORE_BE_MISSION_E_TASKS (-6)  /* n outside 1..max_tasks, or a kind outside 0..3 */
/* phase of a mission, and the status of its last goal */
#define ALORE_BE_MISSION_PHASE_NONE 0
#define ALORE_BE_MISSION_PHASE_ITEM 1
#define ALORE_BE_MISSION_PHASE_TARGET 2
#define ALORE_BE_MISSION_GOAL_OK 0
#define ALORE_BE_MISSION_GOAL_E_POINT (-1) /* the goal is not finite: the phase is NONE */
/* footprints of an item (the reference's if_mix_task shapes) */
#define ALORE_BE_ITEM_SQUARE 0 /* item_half x item_half */
#define ALORE_BE_ITEM_BOX 1    /* 0.25 x 0.15 */
#define ALORE_BE_ITEM_TABLE 2  /* 0.5 x 0.25 */
#define ALORE_BE_ITEM_CHAIR 3  /* 0.2 x 0.2 */
/* Allocates, once: the slab of max_problems missions, an edit list of ALORE_BE_TASK_MAX_TASKS * max_problems entries (mission_set
 * appends one edit per item, mission_step at most two per mission) with its length, and the staging of the host routes.  params
 * NULL: the defaults; a second call only replaces the parameters.  Needs the resident map. */
int alore_backend_mission_create(alore_backend_handle h, const alore_backend_mission_params *params);
/* Stores items and targets of missions 0..count-1 from rows of the layout alore_backend_task_plan reads (point 0, the robot, is
 * ignored; the same buffer serves both calls), then paints "items -> OBS" (:507-522): for missions in slot order and items in index
 * order one edit per item, through the kernels of alore_backend_map_paint on the same stream.  kinds: [count][max_tasks] ints, one
 * ALORE_BE_ITEM_* per item, NULL: all squares.  A mission that is set starts with phase NONE.  A mission with a negative status
 * paints nothing and takes no part in later calls.  The mask is read as alore_backend_search_paths reads its mask.
 * device_pointers as for alore_backend_task_plan: != 0, everything is DEVICE memory read in stream order and nothing waits; == 0,
 * HOST memory, uploaded, and the stream is synchronised (the return value speaks of the call: read the status words). */
int alore_backend_mission_set(alore_backend_handle h, int count, int max_tasks, const int *n_tasks, const double *points,
                              int point_row_stride_bytes, const int *kinds_or_null, int device_pointers, const int *mask,
                              int mask_stride_bytes, void *stream);
/* The classification MainThread makes at every plan start (:618-658) for the goal of mission m, the two doubles at (char *)goal_xy
 * + m * goal_stride_bytes (a multiple of 8, at least 16): goal_item is the FIRST item at the least distance from the goal
 * (nearest_point starts from DBL_MAX and compares with <), goal_target likewise, the phase ITEM if dist_item < dist_target, else
 * TARGET.  A goal that is not finite leaves the phase NONE and the goal status ALORE_BE_MISSION_GOAL_E_POINT.  leg_goal_xy + 2 l
 * of alore_backend_device_task with stride ALORE_BE_TASK_MAX_LEGS * 16 serves as the goals as it lies. */
int alore_backend_mission_set_goals(alore_backend_handle h, int count, const double *goal_xy, int goal_stride_bytes, int device_pointers,
                                    const int *mask, int mask_stride_bytes, void *stream);
/* One tick of MapUpdateThread plus the post-plan rule, for missions 0..count-1 in slot order, each with status OK and a phase; x, y
 * of robot m are the two doubles at (char *)poses + m * pose_stride_bytes (a multiple of 8, at least 16: d_xytheta of
 * alore_backend_predicted_state_device and the closed loops' pose slabs serve as they lie).  Each rule that fires appends one edit:
 *   1. phase ITEM and |pose - goal_item| < item_free_dist: free goal_item with free_half (:526-537);
 *   2. phase TARGET and |pose - goal_target| < target_lock_dist: lock goal_target with target_lock_half (:539-552);
 *   3. after_plan_mask selects the mission (NULL: none; the word alore_backend_replan_mask writes serves as it lies) and the phase
 *      is ITEM: the nearest target to the POSE, if closer than left_target_dist, is locked with left_target_half (:695-704).
 * Distances are sqrt(dx * dx + dy * dy) in double without contraction, comparisons are strict (a pose exactly 2.0 away frees
 * nothing), a pose that is not finite fails every comparison.  As in the reference an edit repeats on every tick while its
 * condition holds: n_changed says whether anything moved.  The list is compacted in slot order with its length on the device and
 * painted by the kernels of alore_backend_map_paint in the same call on the same stream; with device_pointers != 0 nothing waits
 * and nothing is copied to the host. */
int alore_backend_mission_step(alore_backend_handle h, int count, const double *poses, int pose_stride_bytes, int device_pointers,
                               const int *after_plan_mask, int mask_stride_bytes, void *stream);
/* the device slab of the missions [max_problems]; valid until the handle is destroyed */
typedef struct alore_backend_mission_view {
    int max_tasks, edit_capacity; /* 10, 10 * max_problems */
    const int *status, *phase, *goal_item, *goal_target, *goal_status, *n_tasks; /* [.]; goal_item / goal_target: indices, -1 before a goal */
    const int *kinds;                                                            /* [.][10] */
    const double *items, *targets;                                               /* [.][10][2] */
    const alore_backend_map_edit *edits; /* the list of the last mission_set or mission_step */
    const int *n_edits;                  /* its length */
    const int *counters;                 /* n_changed, min_x, min_y, max_x, max_y, n_skipped of the last paint */
} alore_backend_mission_view;
int alore_backend_device_mission(alore_backend_handle h, alore_backend_mission_view *out);
/* The same copied to HOST arrays [count] (any pointer may be NULL); edits needs room for edit_capacity entries and receives
 * *n_edits.  Waits for the device. */
int alore_backend_get_mission(alore_backend_handle h, int count, int *status, int *phase, int *goal_item, int *goal_target,
                              int *goal_status, alore_backend_map_edit *edits, int *n_edits, int counters[6]);

/* ---- plan_manager's state machine for the fleet, on the device -------------------------------------------------------- */
/* What decides in plan_manager: start_callback / goal_callback (plan_manager.hpp:434-468) and PlanManager::MainThread (:556-712),
 * with the collision stop of PlanTester::MainThread (plan_tester.hpp:529-541), as per-robot device state, one robot per problem slot
 * of the handle.  csrc/fleet_manager.h holds the rules, states their order of operations and lists the deviations from the
 * reference; csrc/fleet_manager.hip holds the kernels (one lane per robot).  A manager period is
 *     manager_begin -> predicted_state_device -> manager_starts -> search_paths / set_paths / plan_masked under plan_mask ->
 *     manager_end -> refs_set_pending_from_backend under fresh_mask (start time now) and replan_mask (now + max_replan_time) ->
 *     alore_nmpc_refs_stop / alore_*_plant_stop under stop_mask -> mission_step with after_plan_mask,
 * all device memory in stream order: nothing waits, and there is no per-robot state on the host.  Calls on one handle must be
 * ordered on one stream, as for alore_backend_search_paths.
 * A robot in GOINGTOGOAL or EMERGENCY_STOP leaves that state only through the finish rule (now - traj_start_time >=
 * traj_total_time), as in the reference. */
#define ALORE_BE_STATE_INIT 0
#define ALORE_BE_STATE_IDLE 1
#define ALORE_BE_STATE_PLANNING 2
#define ALORE_BE_STATE_REPLAN 3
#define ALORE_BE_STATE_GOINGTOGOAL 4
#define ALORE_BE_STATE_EMERGENCY_STOP 5
#define ALORE_BE_ACTION_NONE 0
#define ALORE_BE_ACTION_FRESH 1  /* a first plan from the requested start, with zero derivatives */
#define ALORE_BE_ACTION_REPLAN 2 /* a plan from the state predicted at `time` along the stored plan */
typedef struct alore_backend_manager_params {
    double replan_time;           /* 5000 (planner_sim.launch:63) */
    double max_replan_time;       /* 0.05 (planner_sim.launch:65) */
    int replan_on_collision_only; /* 0: the reference replans periodically */
    int stop_inside_obstacle;     /* 0; not 0: the collision stop of plan_tester.hpp:529-541 in front of every begin */
    int stop_on_no_path;          /* 0: a robot without a path goes to EMERGENCY_STOP and no stop flag is raised (the reference
                                     publishes nothing there); not 0: the flag is raised */
    int reserved;                 /* 0 */
} alore_backend_manager_params;
void alore_backend_manager_default_params(alore_backend_manager_params *p);
/* Allocates, once: the slab of max_problems robots (every robot IDLE without goal and start, `returned` 1, all times 0 but plan_start_time
 * and time, which are -1), the masks and the counters (0).  params NULL: the defaults.  A second call only replaces the parameters.
 * ALORE_BE_E_INVALID for times that are not finite or a max_replan_time that is negative. */
int alore_backend_manager_create(alore_backend_handle h, const alore_backend_manager_params *params);
/* start_callback and goal_callback for robots 0..count-1: x, y, yaw of robot b are the three doubles at (char *)start_xytheta + b *
 * stride_bytes (a multiple of 8, at least 24), likewise the goal.  Either array may be NULL (not both).  A robot that is not IDLE
 * refuses both, a value that is not finite is refused; the `refused` counter holds the refusals of THIS call (a start and a goal
 * count one each).  mask (NULL: every robot) is read as alore_backend_search_paths reads its mask; it is DEVICE memory when
 * device_pointers != 0.  device_pointers == 0: the arrays are HOST memory, uploaded, and the stream is synchronised. */
int alore_backend_manager_request(alore_backend_handle h, int count, const double *start_xytheta, const double *goal_xytheta, int stride_bytes,
                                  int device_pointers, const int *mask, int mask_stride_bytes, void *stream);
/* The head of MainThread for robots 0..count-1 at time `now`: x, y of robot b are the two doubles at (char *)poses + b *
 * pose_stride_bytes (a multiple of 8, at least 16).  Writes the action (ALORE_BE_ACTION_*), the predicted time and the five masks
 * (plan_mask = the action is not NONE; the others 0 but stop_mask of a robot the collision stop fires for).
 * collision_mask_or_null: the robots that may replan under replan_on_collision_only, read with mask_stride_bytes; the
 * `collision` words of alore_backend_device_check serve as they lie.  The collision stop reads the handle's map of now.
 * device_pointers as for alore_backend_manager_request. */
int alore_backend_manager_begin(alore_backend_handle h, int count, double now, const double *poses, int pose_stride_bytes,
                                const int *collision_mask_or_null, int mask_stride_bytes, int device_pointers, void *stream);
/* Behind alore_backend_predicted_state_device, on its outputs (DEVICE, [count][3]): the rows of FRESH robots become the requested
 * start with zero d_vaj and d_oaj, the predicted pose of REPLAN robots becomes their plan_start_xytheta (:588), rows of other robots
 * stay bit for bit.  d_start_yaw and d_end_yaw (DEVICE, [count], may be NULL) receive plan_start_xytheta[2] and goal[2] of every
 * robot: the arrays alore_backend_set_paths reads. */
int alore_backend_manager_starts(alore_backend_handle h, int count, double *d_xytheta, double *d_vaj, double *d_oaj, double *d_start_yaw,
                                 double *d_end_yaw, void *stream);
/* The rest of MainThread with the `now` of the matching begin (without one: ALORE_BE_E_INVALID): the outcome of the robots that
 * planned, the delivery masks (fresh_mask: deliver with start time now; replan_mask: with now + max_replan_time), after_plan_mask,
 * stop_mask, then the finish rule.  Each pointer may be NULL, which means the handle's own slab (search status, build status, the
 * plans' ok words, their durations T [.][max_pieces as rounded by the handle] and piece counts); a pointer that is not NULL is
 * DEVICE memory of the same layout.  The duration of a plan is the sum of T[0 .. n_pieces - 1] in piece order. */
int alore_backend_manager_end(alore_backend_handle h, int count, const int *search_status, const int *build_status, const int *plan_ok,
                              const double *T, const int *n_pieces, void *stream);
/* Sequencing of a mission's legs (the ALORE FSM sends /planner_start_pose and /planner_goal_pose once per entry of
 * /task_plan/results): a robot that is IDLE without a goal, whose mission in the slab of alore_backend_task_plan has status >= 0 and
 * whose `leg` is below n_order takes goal = (leg_goal_xy[leg], leg_yaw[leg]), start = its pose (x, y, yaw at (char *)poses + b *
 * pose_stride_bytes, a multiple of 8, at least 24), both flags, leg += 1.  Every other robot is untouched.  reset_legs != 0: such a
 * robot starts again at leg 0 (alore_backend_manager_request never changes `leg`).  All pointers are DEVICE memory; leg_yaw is
 * [count][ALORE_BE_TASK_MAX_LEGS]. */
int alore_backend_manager_next_legs(alore_backend_handle h, int count, const double *poses, int pose_stride_bytes, const double *leg_yaw,
                                    int reset_legs, void *stream);
/* the device slab [max_problems]; vectors are [3][max_problems] (component-major); valid until the handle is destroyed */
typedef struct alore_backend_manager_view {
    int max_problems, n_counters; /* n_counters = 8 */
    const int *state, *have_goal, *have_start, *leg;
    const int *action;   /* of the last begin */
    const int *returned; /* the last begin left MainThread early for this robot: its end does nothing */
    const int *plan_mask, *fresh_mask, *replan_mask, *stop_mask, *after_plan_mask; /* stride sizeof(int) */
    const double *goal, *start, *plan_start_xytheta;                               /* [3][max_problems] */
    const double *loop_start_time, *plan_start_time, *traj_start_time, *traj_total_time;
    const double *time;  /* the predicted time of the last begin: the d_time of alore_backend_predicted_state_device; -1 for FRESH */
    const int *counters; /* fresh, replan, going_to_goal, stopped, delivered, arrived (since manager_create), refused (last request), 0 */
} alore_backend_manager_view;
int alore_backend_device_manager(alore_backend_handle h, alore_backend_manager_view *out);
/* The slab of robots 0..count-1 copied to HOST memory: ints [11][count] in the order of the view (state .. after_plan_mask), doubles
 * [14][count] (goal x, y, yaw, start x, y, yaw, plan_start x, y, yaw, loop_start_time, plan_start_time, traj_start_time,
 * traj_total_time, time), counters [8].  Any pointer may be NULL.  Waits for the device. */
int alore_backend_get_manager(alore_backend_handle h, int count, int *ints, double *doubles, int *counters);

#ifdef __cplusplus
}
#endif
#endif /* ALORE_BACKEND_H */
