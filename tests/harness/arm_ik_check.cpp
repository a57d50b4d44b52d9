// arm_ik_check.cpp -- csrc/z1_kinematics.h on the CPU (tests/test_arm_ik_cpu.py, tools/arm_ik.py): runs the commands of a file
// through the header one problem and one robot at a time and prints every result, every double with 17 digits.
//   usage: arm_ik_check <command file> [repeat]      (repeat: runs the I commands that many times, for timing; prints once)
//   commands, one per line:
//     P eps damp dt max_iter                    the parameters of the commands that follow (the rest stays at its default)
//     F q[7]                                    -> pose[12] J[36]
//     L R[9] p[3]                               -> log6[6] jlog6[36]
//     I q_init[7] target[12]                    -> q[7] err_norm iterations status
//     G object[4] cfg[3]                        -> pose[7]
//     B base_pose[7] target_pose[7] category k  -> target[12]
//     S robots ticks                            a grasp sequence with the plant joint_positions <- joint_cmd; then per robot a line
//                                               "category grasp_cfg[3] plan_cfg[3] arm_default_pose[7] object[4] arm_base_pose[7]"
//                                               and per tick and robot a line "x y" (robot_xy)
//                                               -> per tick and robot: grasp_time flag stable done ik_iterations ik_status,
//                                                  k d_gripper gripper_ang err_norm, joint_cmd[7], robot_vel_cmd[3]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "z1_kinematics.h"

namespace {
bool read(std::FILE* f, double* v, int n)
{
    for (int i = 0; i < n; ++i) {
        char word[64];
        if (std::fscanf(f, "%63s", word) != 1) return false;
        v[i] = std::strtod(word, nullptr); // nan and inf included
    }
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
    const int repeat = argc > 2 ? std::atoi(argv[2]) : 1;
    z1::Params P;
    z1::default_params(&P);
    char cmd[8];
    while (std::fscanf(f, "%7s", cmd) == 1) {
        // every array on the heap with its exact size: the address sanitizer sees an overrun
        if (cmd[0] == 'P') {
            double v[3];
            if (!read(f, v, 3) || std::fscanf(f, "%d", &P.max_iter) != 1) return 3;
            P.eps = v[0]; P.damp = v[1]; P.dt = v[2];
            continue; // prints nothing
        } else if (cmd[0] == 'F') {
            double *q = new double[7], *pose = new double[12], *J = new double[36];
            if (!read(f, q, 7)) return 3;
            z1::fk(P, q, pose, pose + 9);
            z1::jac_local(P, q, J);
            print(pose, 12); print(J, 36);
            delete[] q; delete[] pose; delete[] J;
        } else if (cmd[0] == 'L') {
            double *T = new double[12], *l = new double[6], *Jl = new double[36];
            if (!read(f, T, 12)) return 3;
            z1::log6(T, T + 9, l);
            z1::jlog6(T, T + 9, Jl);
            print(l, 6); print(Jl, 36);
            delete[] T; delete[] l; delete[] Jl;
        } else if (cmd[0] == 'I') {
            double *qi = new double[7], *T = new double[12], *q = new double[7];
            if (!read(f, qi, 7) || !read(f, T, 12)) return 3;
            z1::IkResult r{};
            for (int k = 0; k < repeat; ++k) r = z1::ik_solve(P, qi, T, q);
            print(q, 7);
            std::printf("%.17g %d %d", r.err_norm, r.iterations, r.status);
            delete[] qi; delete[] T; delete[] q;
        } else if (cmd[0] == 'G') {
            double *in = new double[7], *pose = new double[7];
            if (!read(f, in, 7)) return 3;
            z1::grasp_pose(in, in + 4, pose);
            print(pose, 7);
            delete[] in; delete[] pose;
        } else if (cmd[0] == 'B') {
            double *in = new double[14], *T = new double[12], k;
            int category;
            if (!read(f, in, 14) || std::fscanf(f, "%d", &category) != 1 || !read(f, &k, 1)) return 3;
            z1::base_target(in, in + 7, category, k, T);
            print(T, 12);
            delete[] in; delete[] T;
        } else if (cmd[0] == 'S') {
            int R, ticks;
            if (std::fscanf(f, "%d %d", &R, &ticks) != 2 || R < 1 || ticks < 1) return 3;
            z1::Class* cls = new z1::Class[R]();
            z1::Grasp* g = new z1::Grasp[R];
            double *obj = new double[4 * R], *base = new double[7 * R], *jp = new double[7 * R], *xy = new double[2];
            for (int r = 0; r < R; ++r) {
                if (std::fscanf(f, "%d", &cls[r].category) != 1) return 3;
                if (!read(f, cls[r].grasp_cfg, 3) || !read(f, cls[r].plan_cfg, 3) || !read(f, cls[r].arm_default_pose, 7)) return 3;
                if (!read(f, obj + 4 * r, 4) || !read(f, base + 7 * r, 7)) return 3;
                z1::grasp_initial(P, g[r]);
                for (int i = 0; i < 7; ++i) jp[7 * r + i] = P.joint_default[i];
            }
            for (int t = 0; t < ticks; ++t)
                for (int r = 0; r < R; ++r) {
                    if (!read(f, xy, 2)) return 3;
                    z1::grasp_step(P, cls[r], g[r], xy, obj + 4 * r, base + 7 * r, jp + 7 * r);
                    for (int i = 0; i < 7; ++i) jp[7 * r + i] = g[r].joint_cmd[i];
                    std::printf("%d %d %d %d %d %d ", g[r].grasp_time, g[r].flag, g[r].stable, g[r].done, g[r].ik_iterations, g[r].ik_status);
                    print(&g[r].k, 1); print(&g[r].d_gripper, 1); print(&g[r].gripper_ang, 1); print(&g[r].err_norm, 1);
                    print(g[r].joint_cmd, 7); print(g[r].robot_vel_cmd, 3);
                    if (t + 1 < ticks || r + 1 < R) std::printf("\n");
                }
            delete[] cls; delete[] g; delete[] obj; delete[] base; delete[] jp; delete[] xy;
        } else
            return 3;
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
