// task_fsm_check.cpp -- csrc/task_fsm.h on the CPU (tests/test_task_fsm_cpu.py): replays a recorded scene through the header one
// robot at a time and prints the state after every tick, every double with 17 digits.
//   usage: task_fsm_check <command file>
//   commands:
//     P eps damp dt max_iter                     the IK parameters of the scenes that follow
//     T t[8]                                     the tick counts (fsm::Params in order)
//     X k d_gripper arm_default_pose[7]          object_release until it is done -> per call: done k d_gripper joint_cmd[7]
//     R robots ticks max_tasks max_objects max_path_points
//        then per robot "category grasp_cfg[3] plan_cfg[3] arm_default_pose[7] com_offset[2] stop_after_back_off targets[max_tasks][4]"
//        then per tick and robot "n_events", the events "S n order[n]" (the sequences) / "L n xy[n][2]" (a path), and the inputs
//        robot_pose[4] object_poses[max_objects][4] arm_base_pose[7] joint_positions[7]
//        -> per tick and robot: the 15 words of fsm::Robot, grasp_time flag stable done ik_iterations ik_status,
//           reach_threshold object_vel_cmd[3] start[3] goal[3] object_pose_used[4], k d_gripper gripper_ang err_norm, joint_cmd[7],
//           robot_vel_cmd[3], the control row[15], then the counters refused_sequences refused_paths
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "task_fsm.h"

namespace {
bool read(std::FILE* f, double* v, int n)
{
    for (int i = 0; i < n; ++i) {
        char word[64];
        if (std::fscanf(f, "%63s", word) != 1) return false;
        v[i] = std::strtod(word, nullptr);
    }
    return true;
}
bool read_int(std::FILE* f, int* v, int n)
{
    for (int i = 0; i < n; ++i)
        if (std::fscanf(f, "%d", v + i) != 1) return false;
    return true;
}
void print(const double* v, int n)
{
    for (int i = 0; i < n; ++i) std::printf("%.17g ", v[i]);
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    z1::Params P;
    z1::default_params(&P);
    fsm::Params F;
    fsm::default_params(&F);
    char cmd[8];
    while (std::fscanf(f, "%7s", cmd) == 1) {
        if (cmd[0] == 'P') {
            double v[3];
            if (!read(f, v, 3) || std::fscanf(f, "%d", &P.max_iter) != 1) return 3;
            P.eps = v[0]; P.damp = v[1]; P.dt = v[2];
        } else if (cmd[0] == 'T') {
            if (!read_int(f, &F.ticks_no_plan, 1) || !read_int(f, &F.ticks_plan, 1) || !read_int(f, &F.ticks_wait_path, 1) ||
                !read_int(f, &F.ticks_robot_reached, 1) || !read_int(f, &F.ticks_grasp_done, 1) || !read_int(f, &F.ticks_object_reached, 1) ||
                !read_int(f, &F.ticks_release, 1) || !read_int(f, &F.ticks_release_done, 1))
                return 3;
        } else if (cmd[0] == 'X') {
            z1::Class* c = new z1::Class();
            z1::Grasp* g = new z1::Grasp();
            z1::grasp_initial(P, *g);
            if (!read(f, &g->k, 1) || !read(f, &g->d_gripper, 1) || !read(f, c->arm_default_pose, 7)) return 3;
            for (int call = 0; call < 100; ++call) {
                const int done = fsm::release(*c, *g);
                std::printf("%d ", done);
                print(&g->k, 1); print(&g->d_gripper, 1); print(g->joint_cmd, 7);
                std::printf("\n");
                if (done) break;
            }
            delete c; delete g;
        } else if (cmd[0] == 'R') {
            int R, ticks, mt, mo, mp;
            if (std::fscanf(f, "%d %d %d %d %d", &R, &ticks, &mt, &mo, &mp) != 5 || R < 1 || ticks < 1 || mt < 1 || mt > fsm::MAX_TASKS || mo < 1 || mp < 1)
                return 3;
            // every array on the heap with its exact size: the address sanitizer sees an overrun
            z1::Class* cls = new z1::Class[R]();
            z1::Grasp* g = new z1::Grasp[R];
            fsm::Robot* rb = new fsm::Robot[R];
            int* seq = new int[R * 2 * fsm::MAX_TASKS];
            double *com = new double[2 * R], *targets = new double[R * mt * 4], *rpath = new double[R * mp * 2], *opath = new double[R * mp * 2];
            double *pose = new double[4], *objs = new double[mo * 4], *base = new double[7], *jp = new double[7], *ctl = new double[15];
            int counters[2] = {0, 0};
            for (int r = 0; r < R; ++r) {
                int stop;
                if (std::fscanf(f, "%d", &cls[r].category) != 1) return 3;
                if (!read(f, cls[r].grasp_cfg, 3) || !read(f, cls[r].plan_cfg, 3) || !read(f, cls[r].arm_default_pose, 7) || !read(f, com + 2 * r, 2) ||
                    !read_int(f, &stop, 1) || !read(f, targets + r * mt * 4, mt * 4))
                    return 3;
                fsm::reset(F, rb[r], seq + r * 2 * fsm::MAX_TASKS);
                rb[r].stop_after_back_off = stop;
                z1::grasp_initial(P, g[r]);
                for (int i = 0; i < mp * 2; ++i) rpath[r * mp * 2 + i] = opath[r * mp * 2 + i] = 0.0;
            }
            for (int t = 0; t < ticks; ++t)
                for (int r = 0; r < R; ++r) {
                    int n_events;
                    if (!read_int(f, &n_events, 1)) return 3;
                    for (int e = 0; e < n_events; ++e) {
                        char kind[8];
                        int n;
                        if (std::fscanf(f, "%7s %d", kind, &n) != 2 || n < 0) return 3;
                        if (kind[0] == 'S') {
                            int* order = new int[n > 0 ? n : 1];
                            if (!read_int(f, order, n)) return 3;
                            if (!fsm::set_sequence(rb[r], seq + r * 2 * fsm::MAX_TASKS, order, n, mt, mo)) counters[0] += 1;
                            delete[] order;
                        } else if (kind[0] == 'L') {
                            double* xy = new double[n > 0 ? 2 * n : 1];
                            if (!read(f, xy, 2 * n)) return 3;
                            const int which = fsm::deliver_path(rb[r], n, mp);
                            if (which < 0) counters[1] += 1;
                            if (which > 0) std::memcpy((which == 1 ? rpath : opath) + r * mp * 2, xy, sizeof(double) * 2 * n);
                            delete[] xy;
                        } else
                            return 3;
                    }
                    if (!read(f, pose, 4) || !read(f, objs, mo * 4) || !read(f, base, 7) || !read(f, jp, 7)) return 3;
                    if (fsm::tick_head(F, cls[r], com + 2 * r, rb[r], g[r], seq + r * 2 * fsm::MAX_TASKS, rpath + r * mp * 2, opath + r * mp * 2,
                                       targets + r * mt * 4, pose, objs))
                        fsm::tick_grasp(F, P, cls[r], rb[r], g[r], pose, base, jp);
                    const int* w = &rb[r].task_state;
                    for (int i = 0; i < fsm::ROBOT_INTS; ++i) std::printf("%d ", w[i]);
                    std::printf("%d %d %d %d %d %d ", g[r].grasp_time, g[r].flag, g[r].stable, g[r].done, g[r].ik_iterations, g[r].ik_status);
                    print(&rb[r].reach_threshold, 1); print(rb[r].object_vel_cmd, 3); print(rb[r].start_xytheta, 3); print(rb[r].goal_xytheta, 3);
                    print(rb[r].object_pose_used, 4);
                    print(&g[r].k, 1); print(&g[r].d_gripper, 1); print(&g[r].gripper_ang, 1); print(&g[r].err_norm, 1);
                    print(g[r].joint_cmd, 7); print(g[r].robot_vel_cmd, 3);
                    fsm::control_row(rb[r], g[r], ctl);
                    print(ctl, 15);
                    std::printf("%d %d\n", counters[0], counters[1]);
                }
            delete[] cls; delete[] g; delete[] rb; delete[] seq; delete[] com; delete[] targets; delete[] rpath; delete[] opath;
            delete[] pose; delete[] objs; delete[] base; delete[] jp; delete[] ctl;
        } else
            return 3;
    }
    std::fclose(f);
    return 0;
}
