// mission_map_check.cpp -- csrc/mission_map.h on the CPU (tests/test_mission_map_cpu.py): runs the calls of a text file through the
// header's serial drivers and prints the state after every call.  Doubles are read with strtod (hex floats, nan, inf) and printed
// with %a.
//   usage: mission_map_check <calls file>
//   file:  nx ny x_lo y_lo res slots  item_half free_half item_free_dist target_lock_half target_lock_dist left_target_half left_target_dist
//          then calls:  V n  {cx cy hx hy make_obs} x n                      host validation only: prints "invalid <index or -1>"
//                       P n  {cx cy hx hy make_obs} x n                      paint_list
//                       S count T  {mask n_tasks  (1 + 2 T) x, y pairs  T kinds} x count
//                       G count  {mask gx gy} x count
//                       T count  {px py after_plan} x count
//   out:   per P / S / G / T call: "counters n_changed min_x min_y max_x max_y n_skipped", "edits n" and n lines
//          "cx cy hx hy make_obs reserved", five lines of `slots` ints (status, phase, goal_item, goal_target, goal_status), nx lines of
//          ny states
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mission_map.h"

static bool read_double(std::FILE* f, double* v)
{
    char tok[64];
    if (std::fscanf(f, "%63s", tok) != 1) return false;
    char* end = nullptr;
    *v = std::strtod(tok, &end);
    return end != tok && *end == 0;
}
static bool read_int(std::FILE* f, int* v) { return std::fscanf(f, "%d", v) == 1; }
static bool read_edits(std::FILE* f, int n, mission::Edit* e)
{
    for (int k = 0; k < n; ++k) {
        int obs;
        if (!read_double(f, &e[k].cx) || !read_double(f, &e[k].cy) || !read_double(f, &e[k].hx) || !read_double(f, &e[k].hy) || !read_int(f, &obs)) return false;
        e[k].make_obs = obs;
        e[k].reserved = 0;
    }
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx, ny, slots;
    double x_lo, y_lo, res, pv[7];
    if (!read_int(f, &nx) || !read_int(f, &ny) || !read_double(f, &x_lo) || !read_double(f, &y_lo) || !read_double(f, &res) || !read_int(f, &slots)) return 3;
    for (double& v : pv)
        if (!read_double(f, &v)) return 3;
    if (nx < 2 || ny < 2 || slots < 1) return 3;
    const mission::Params P{pv[0], pv[1], pv[2], pv[3], pv[4], pv[5], pv[6]};
    const occ::Geom g = occ::make_geom(nx, ny, x_lo, y_lo, res);
    const size_t cells = (size_t)nx * ny, T = mission::MAX_TASKS;
    // every array on the heap with its exact size: the address sanitizer sees an overrun
    unsigned char *grid = new unsigned char[cells](), *before = new unsigned char[cells];
    int* ints = new int[(size_t)slots * 6]();
    int* kinds = new int[(size_t)slots * T]();
    double *items = new double[(size_t)slots * T * 2](), *targets = new double[(size_t)slots * T * 2]();
    const mission::Slab s{ints, ints + slots, ints + 2 * slots, ints + 3 * slots, ints + 4 * slots, ints + 5 * slots, kinds, items, targets};
    for (int b = 0; b < slots; ++b) {
        s.status[b] = mission::MASKED;
        s.goal_item[b] = s.goal_target[b] = -1;
    }
    char call;
    mission::Counters c = mission::no_change(nx, ny); // of the last paint: a G call leaves them and the list as they are
    std::vector<mission::Edit> list;
    while (std::fscanf(f, " %c", &call) == 1) {
        int n;
        if (!read_int(f, &n) || n < 0 || (call != 'V' && call != 'P' && n > slots)) return 3;
        if (call == 'V' || call == 'P') {
            mission::Edit* e = new mission::Edit[n];
            if (!read_edits(f, n, e)) return 3;
            if (call == 'V') {
                std::printf("invalid %ld\n", mission::first_invalid(e, n, res));
                delete[] e;
                continue;
            }
            c = mission::paint_list(g, grid, e, n, before);
            list.clear();
            delete[] e;
        } else if (call == 'S') {
            int max_tasks;
            if (!read_int(f, &max_tasks) || max_tasks < 1 || max_tasks > (int)T) return 3;
            int* set = new int[n];
            double* row = new double[2 * (1 + 2 * max_tasks)];
            int* k = new int[max_tasks];
            for (int b = 0; b < n; ++b) {
                int n_tasks;
                if (!read_int(f, &set[b]) || !read_int(f, &n_tasks)) return 3;
                for (int i = 0; i < 2 * (1 + 2 * max_tasks); ++i)
                    if (!read_double(f, &row[i])) return 3;
                for (int i = 0; i < max_tasks; ++i)
                    if (!read_int(f, &k[i])) return 3;
                if (set[b]) mission::set_one(s, b, max_tasks, n_tasks, row, k);
            }
            mission::Edit* e = new mission::Edit[(size_t)n * T];
            const long ne = mission::item_edits_all(s, P, n, set, e);
            list.assign(e, e + ne);
            c = mission::paint_list(g, grid, e, ne, before);
            delete[] e; delete[] set; delete[] row; delete[] k;
        } else if (call == 'G') {
            for (int b = 0; b < n; ++b) {
                int sel;
                double gx, gy;
                if (!read_int(f, &sel) || !read_double(f, &gx) || !read_double(f, &gy)) return 3;
                if (sel) mission::goals_one(s, b, gx, gy);
            }
        } else if (call == 'T') {
            double* poses = new double[2 * (size_t)n];
            int* after = new int[n];
            for (int b = 0; b < n; ++b)
                if (!read_double(f, &poses[2 * b]) || !read_double(f, &poses[2 * b + 1]) || !read_int(f, &after[b])) return 3;
            mission::Edit* e = new mission::Edit[2 * (size_t)n];
            const long ne = mission::step_all(s, P, n, poses, after, e);
            list.assign(e, e + ne);
            c = mission::paint_list(g, grid, e, ne, before);
            delete[] e; delete[] poses; delete[] after;
        } else
            return 3;
        std::printf("counters %d %d %d %d %d %d\n", c.n_changed, c.min_x, c.min_y, c.max_x, c.max_y, c.n_skipped);
        std::printf("edits %zu\n", list.size());
        for (const mission::Edit& e : list) std::printf("%a %a %a %a %d %d\n", e.cx, e.cy, e.hx, e.hy, e.make_obs, e.reserved);
        for (int a = 0; a < 5; ++a) {
            for (int b = 0; b < slots; ++b) std::printf("%d ", ints[(size_t)a * slots + b]);
            std::printf("\n");
        }
        for (int x = 0; x < nx; ++x) {
            for (int y = 0; y < ny; ++y) std::printf("%d ", (int)grid[(size_t)x * ny + y]);
            std::printf("\n");
        }
    }
    std::fclose(f);
    delete[] grid; delete[] before; delete[] ints; delete[] kinds; delete[] items; delete[] targets;
    return 0;
}
