// task_plan.h -- the visit order of a rearrangement mission from path costs on the distance field, the arithmetic once (internal).
// Plain C++17: __host__ __device__ under hipcc, no HIP dependency otherwise.  What the reference's plan_manager does before any
// trajectory is planned (planning_ddr_opt/plan_manager/include/plan_manager/plan_manager.hpp:210-250): the grid-path length between
// the robot, the items and the targets (jps_planner_->plan + getPathLength, :287-300 and :370-413), then the order of the visits,
// solvePathWithGreedy (:347-432, the live call) or BranchAndBoundCombined::solve with a fixed assignment (:252-345,
// branch_and_bound.hpp).  Stated so that the matrix and both orders have exactly one answer each.  The small functions are what the
// kernels of task_plan.hip run; plan_one() strings them together serially and is what tests/harness/task_plan_check.cpp and
// tools/task_plan.py (one host core) run; plan_one_assigned() does the same for the modes that choose the assignment
// (tests/harness/task_assign_check.cpp).  The oracles are tests/task_plan_cases.py and tests/task_assign_cases.py; harness and device
// equal them bit for bit.
//
// THE CONTRACT
//   mission  n tasks, 1 <= n <= max_tasks <= MAX_TASKS = 10, and P = 1 + 2 n points (x, y): index 0 the robot, 1..n the items,
//            n+1..2n the targets (plan_manager.hpp:279).  Missions are batched: mission m has its points packed at the beginning of
//            a row of 1 + 2 max_tasks points, (char*)points + m * row stride, its n at n_tasks[m], its assignment (optimal mode, may
//            be absent) at assign[m * max_tasks + i].
//   status   OK 0, MASKED 1, E_ENDPOINT -1 and E_WINDOW -3 as in path_search.h; E_TASKS -6: n outside 1..max_tasks, or (optimal
//            mode) a given assignment that is no permutation of 0..n-1, or (joint mode) n > 5; E_NO_ORDER -7 (every mode but
//            greedy): no order has a finite cost.
//            A point of the mission that is not finite or outside [lo, hi] is E_ENDPOINT.  The checks come in the order tasks,
//            end point, window.  A mission that fails a check writes its status and n_order = 0 and nothing else; a masked-out
//            mission writes status 1 and nothing else.  E_NO_ORDER is found after the matrix: status, n_order = 0, the matrix and
//            the diagnostics are written, order, total and legs are not.
//   window   the bounding box of the cells of all P points grown by ceil(window_margin / res) cells a side, clipped to the map;
//            more than psearch::MAX_CELLS cells is E_WINDOW.  One window per mission: every pair is searched in it.
//   d(i, j)  the least cost over the reference's graph (eight moves, only the destination must be free, 1 or sqrt 2,
//            graph_search.cpp:225-243) between the cells of points i and j inside the window, as the exact pair (a, b) for
//            a + b sqrt 2.  A cell is free when !(dist < safe_ij); safe_ij is the reference's rule for the pair
//            (jps_planner.cpp:39-42), max(min(max(min(safe_dis, 0.8 dist_i), 0), 0.8 dist_j), 0) with i < j, symmetric for
//            safe_dis >= 0.  Equal cells give (0, 0), whatever their distance.  Otherwise an end cell that is not free, or no path
//            in the window, gives INF = (-1, -1) (the reference: DBL_MAX).  d(i, j) = d(j, i).
//   sums     a route's cost is the component-wise sum of pairs, INF absorbs.  Two sums are ordered exactly: the sign of
//            da + db sqrt 2 from the signs of da and db, and where they differ from da^2 against 2 db^2 in 64-bit integers (twenty
//            legs of fewer than 32768 steps: below 2^41).  A finite sum is less than INF, INF is not less than INF.  No
//            floating-point sum anywhere.
//   GREEDY   solvePathWithGreedy as written: from point 0 the unvisited item of least d, strict <, so the lowest index wins a tie
//            and an INF is never chosen; from that item the unvisited target of least d (any target: no assignment in this mode);
//            from that target again.  It stops where nothing is reachable: n_order may be odd.
//   OPTIMAL  the fixed-assignment routing of BranchAndBoundCombined::solve: item i goes to target assign[i] (the identity without an
//            assignment); minimise sum d(previous, item) + d(item, its target) over all item orders, by dynamic programming over
//            subsets: togo[S][last], the least cost still to pay when the items of S are served and the robot stands at the target
//            of `last`.  Among optimal orders the one whose item sequence is lexicographically smallest: going forward, always the
//            lowest item index that still attains the optimum.  The reference's best-first search returns AN optimum; its cost is
//            the contract, the tie rule is ours.
//   outputs  status; the matrix [P_MAX][P_MAX][2] (entry (i, j) at (i * P_MAX + j) * 2, i, j < P); order[2 MAX_TASKS] as the
//            reference publishes it, item index, target index, alternately, each 0-based in its own group; n_order; total[2];
//            leg_start_xy, leg_goal_xy [2 MAX_TASKS][2], the end points of the legs in visit order, rows beyond n_order untouched;
//            fields, the number of cost fields computed for the mission (per source k < P - 1 the number of distinct safe_kj over
//            j > k), and sweeps, the most any of them needed.
//   ASSIGNED the item-to-target assignment, then the OPTIMAL routing for it.  The assignment is the bijection sigma of items to
//            targets of least carrying distance, sum_i d(1 + i, n + 1 + sigma(i)), by the sums and the order above; among optimal
//            bijections the one whose vector (sigma(0), sigma(1), ...) is lexicographically smallest.  It is what the reference's
//            hungarian.hpp (included by plan_manager.hpp, never called) would feed the fixed_assignment of
//            solvePathWithBranchAndBound (:273-306) with, up to ties; the tie rule is ours.  Dynamic programming over target
//            subsets: rest[T], the least cost of giving the items popcount(T) .. n-1 the targets outside T; going forward, item k
//            takes the lowest target that still attains rest.  No bijection with a finite sum: E_NO_ORDER, the matrix and the
//            diagnostics written as in the optimal mode.  THE ASSIGNMENT IS DECIDED ON THE CARRY LEGS ALONE: the legs from the
//            robot and between a target and the next item play no part in it, so the routing of sigma (exactly OPTIMAL with
//            assign = sigma) can be without a finite order where another bijection has one; that mission is E_NO_ORDER too, with
//            its assignment rows written.  A given assignment is not read in this mode, neither for values nor for validity.
//   JOINT    the assignment and the order together: minimise sum_k d(prev_k, item pi_k) + d(item pi_k, target sigma(pi_k)), prev_1
//            the robot, prev_k+1 the target just served, over all item orders pi and all bijections sigma -- the problem the
//            greedy mode is a heuristic for.  Dynamic programming over (served items Si, used targets St, last target), |Si| =
//            |St|: togo[Si][St][last], indexed (Si * 32 + St) * 5 + last.  n <= JOINT_MAX_TASKS = 5 (5120 states, 40 KiB); a
//            mission with more tasks in this mode is E_TASKS, whatever max_tasks the launch has (task_limit).  Among optimal routes the one
//            whose published order (item, target, item, target, ...) is lexicographically smallest: going forward, the lowest
//            item, then the lowest target, that still attains the optimum.  No finite route: E_NO_ORDER.  A given assignment is
//            not read.
//   outputs of ASSIGNED and JOINT: all of the above exactly as OPTIMAL writes them (total: the cost of the route), and
//            assignment[MAX_TASKS], the target of item i for i < n, entries beyond n untouched, with assign_total[2], the sum of
//            its carry legs.  Both rows are written by a mission with status OK, and in the ASSIGNED mode by a mission whose
//            assignment is finite and whose routing is not (E_NO_ORDER); by no other mission, and never in the other two modes.
//   WIDE     missions on windows beyond LDS (alore_backend_task_reserve; task_plan_wide.h has the serial form, task_costs_wide_kernel
//            the device's).  check_mission takes the cap on the window as a parameter; the form without it keeps
//            psearch::MAX_CELLS, and the order of the checks does not change.  A mission whose window has more cells than LDS
//            holds and at most the cap has its fields in a slab of device memory, relaxed tile by tile by the machinery of
//            path_search_wide.h as it stands (relax_tile_cell: a word with a component of 32767 or more is never extended); a
//            field starts with the root's tile and the tiles of the root's eight neighbours dirty (task_plan_wide.h).
//            Everything above holds unchanged -- matrix, the four orders, tie rules, legs, fields, masked and failed missions,
//            E_NO_ORDER with its matrix written -- with two differences.  sweeps is the most VISITS OF TILES any field of the
//            mission needed.  And THE RANGE RULE: E_RANGE -8 (not psearch::E_RANGE's -6, which is E_TASKS here) if any field the
//            mission computes has a reached word with a >= 32767 or b >= 32767.  A field is ROOTED AT THE CELL OF THE LOWER
//            INDEX: source k with safe_kj for the targets j > k, one field per distinct safe_kj in order of first appearance,
//            computed whether or not a target shares the source's cell.  The flag is a property of the map, the window, the
//            safe distance and the root (path_search_wide.h), so an oracle decides it from its own fields if it roots them the
//            same way.  E_RANGE is decided after the matrix and before any ordering, so before E_NO_ORDER, in all four modes:
//            status, n_order = 0, fields and sweeps are written, the matrix rows of the mission are unspecified, order, total,
//            legs and the assignment rows untouched.  The exactness of sums holds as stated: without the flag every component
//            of every entry is below 32767, twenty legs stay below 2^41 in the squared comparison.
// DEVIATIONS FROM THE REFERENCE
//   the window: the reference searches the whole map;  an end point outside the map is refused, the reference clamps it;  the tie
//   rules of the optimal, assigned and joint modes;  the assigned and joint modes themselves: the reference has the pieces
//   (hungarian.hpp, fixed_assignment) and calls neither;  a leg searched later by psearch uses that pair's own, smaller window, so
//   its cost can exceed d(i, j).
#ifndef ALORE_TASK_PLAN_H
#define ALORE_TASK_PLAN_H

#include "path_search.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace tplan {

constexpr int MAX_TASKS = 10, P_MAX = 1 + 2 * MAX_TASKS, MAX_LEGS = 2 * MAX_TASKS;
constexpr int OK = 0, MASKED = 1, E_ENDPOINT = -1, E_WINDOW = -3, E_TASKS = -6, E_NO_ORDER = -7;
constexpr int E_RANGE = -8; // wide missions only: a field of the mission has a reached word with a component of 32767 or more
constexpr int GREEDY = 0, OPTIMAL = 1, ASSIGNED = 2, JOINT = 3;
constexpr int STATES = (1 << MAX_TASKS) * MAX_TASKS; // togo[S * MAX_TASKS + last]: 80 KiB
constexpr int REST_STATES = 1 << MAX_TASKS;          // rest[T]: 8 KiB
constexpr int ASSIGNED_STATES = STATES + REST_STATES; // the assigned mode: togo, then rest
constexpr int JOINT_MAX_TASKS = 5, JOINT_SETS = 1 << JOINT_MAX_TASKS;
constexpr int JOINT_STATES = JOINT_SETS * JOINT_SETS * JOINT_MAX_TASKS; // togo[(Si * 32 + St) * 5 + last]: 40 KiB

struct Params {
    double safe_dis, window_margin;
    int mode;
};
inline void default_params(Params* p) { p->safe_dis = 0.3; p->window_margin = 3.0; p->mode = GREEDY; } // the reference's live call

struct Cost {
    int a, b;
};
PS_HD Cost inf_cost() { return Cost{-1, -1}; }
PS_HD bool is_inf(Cost c) { return c.a < 0; }
PS_HD bool same(Cost p, Cost q) { return p.a == q.a && p.b == q.b; }
PS_HD Cost add(Cost p, Cost q) { return (is_inf(p) || is_inf(q)) ? inf_cost() : Cost{p.a + q.a, p.b + q.b}; }
// p < q, exactly
PS_HD bool less(Cost p, Cost q)
{
    if (is_inf(p)) return false;
    if (is_inf(q)) return true;
    const long long da = (long long)p.a - q.a, db = (long long)p.b - q.b;
    if (da >= 0 && db >= 0) return false;
    if (da <= 0 && db <= 0) return true;             // not both zero here
    if (da > 0) return da * da < 2 * db * db;        // da - |db| sqrt 2 < 0
    return da * da > 2 * db * db;                    // -|da| + db sqrt 2 < 0
}
PS_HD Cost entry(const int* mat, int i, int j) { return Cost{mat[(i * P_MAX + j) * 2], mat[(i * P_MAX + j) * 2 + 1]}; }
PS_HD Cost word_cost(unsigned w) { return w >= psearch::UNREACHED ? inf_cost() : Cost{(int)(w >> 16), (int)(w & 0xFFFFu)}; }

struct Mission {
    int status, P;
    int x0, y0, wx, wy; // the window: origin in the map and size in cells
};

// the most tasks a mission may have in a launch for rows of max_tasks: what the joint mode hands check_mission as max_tasks, so
// that n > JOINT_MAX_TASKS is E_TASKS there by the check of n that every mode has
PS_HD int task_limit(int mode, int max_tasks) { return (mode == JOINT && max_tasks > JOINT_MAX_TASKS) ? JOINT_MAX_TASKS : max_tasks; }
// the checks of a mission, in the order tasks, end point, window; pts: the mission's row of points; max_cells: the cap on the window
PS_HD Mission check_mission(const psearch::Grid& g, int n, int max_tasks, const double* pts, const int* assign, int mode, double window_margin,
                            long long max_cells)
{
    Mission m{};
    m.status = E_TASKS;
    if (max_tasks < 1 || max_tasks > MAX_TASKS || n < 1 || n > max_tasks) return m;
    if (mode == OPTIMAL && assign) {
        unsigned seen = 0;
        for (int i = 0; i < n; ++i) {
            const int t = assign[i];
            if (t < 0 || t >= n || ((seen >> t) & 1u)) return m;
            seen |= 1u << t;
        }
    }
    m.P = 1 + 2 * n;
    m.status = E_ENDPOINT;
    int cxa = g.nx, cxb = -1, cya = g.ny, cyb = -1;
    for (int p = 0; p < m.P; ++p) {
        const double x = pts[2 * p], y = pts[2 * p + 1];
        if (!occ::finite_point(x, y)) return m;
        if (x < g.x_lo || x > g.x_hi || y < g.y_lo || y > g.y_hi) return m;
        const int cx = occ::cell_1d(x, g.x_lo, g.inv, g.nx), cy = occ::cell_1d(y, g.y_lo, g.inv, g.ny);
        cxa = cx < cxa ? cx : cxa; cxb = cx > cxb ? cx : cxb;
        cya = cy < cya ? cy : cya; cyb = cy > cyb ? cy : cyb;
    }
    double md = std::ceil(window_margin / g.res);
    if (!(md > 0.0)) md = 0.0;
    if (md > 1.0e9) md = 1.0e9;
    const long long mg = (long long)md;
    const long long xa = cxa - mg, xb = cxb + mg, ya = cya - mg, yb = cyb + mg;
    const int x0 = xa < 0 ? 0 : (int)xa, x1 = xb > g.nx - 1 ? g.nx - 1 : (int)xb;
    const int y0 = ya < 0 ? 0 : (int)ya, y1 = yb > g.ny - 1 ? g.ny - 1 : (int)yb;
    m.x0 = x0; m.y0 = y0; m.wx = x1 - x0 + 1; m.wy = y1 - y0 + 1;
    m.status = ((long long)m.wx * m.wy > max_cells) ? E_WINDOW : OK;
    return m;
}
// the cap of a window that lies in LDS
PS_HD Mission check_mission(const psearch::Grid& g, int n, int max_tasks, const double* pts, const int* assign, int mode, double window_margin)
{
    return check_mission(g, n, max_tasks, pts, assign, mode, window_margin, (long long)psearch::MAX_CELLS);
}

// the cell of point p in window coordinates, x * wy + y, and the map's distance there (a checked mission: the point is inside)
PS_HD int point_cell(const psearch::Grid& g, const Mission& m, const double* pts, int p, double* dist)
{
    const int cx = occ::cell_1d(pts[2 * p], g.x_lo, g.inv, g.nx), cy = occ::cell_1d(pts[2 * p + 1], g.y_lo, g.inv, g.ny);
    *dist = g.dist[(long)cx * g.ny + cy];
    return (cx - m.x0) * m.wy + (cy - m.y0);
}
// the safe distance of the pair (i, j), i < j, from the distances at their cells (jps_planner.cpp:39-42)
PS_HD double pair_safe(double safe_dis, double dist_i, double dist_j)
{
    const double s = psearch::max_of(psearch::min_of(safe_dis, 0.8 * dist_i), 0.0);
    return psearch::max_of(psearch::min_of(s, 0.8 * dist_j), 0.0);
}
// the window of the mission as the search's, its goal the cell of the source: what first_word and relax_cell take
PS_HD psearch::Window field_window(const Mission& m, int source_cell, double safe)
{
    psearch::Window w{};
    w.status = psearch::OK;
    w.x0 = m.x0; w.y0 = m.y0; w.wx = m.wx; w.wy = m.wy;
    w.gx = source_cell / m.wy; w.gy = source_cell - w.gx * m.wy;
    w.sx = w.gx; w.sy = w.gy;
    w.safe = safe;
    return w;
}
// d(k, j) from the field of source k at its fixed point
PS_HD Cost read_cost(const unsigned* words, int cell_k, int cell_j) { return cell_k == cell_j ? Cost{0, 0} : word_cost(words[cell_j]); }
PS_HD void put_entry(int* mat, int i, int j, Cost c)
{
    mat[(i * P_MAX + j) * 2] = c.a;
    mat[(i * P_MAX + j) * 2 + 1] = c.b;
}

// the global index of a point of the published order: entry e of order[] is an item (e even) or a target (e odd)
PS_HD int order_point(int n, const int* order, int e) { return (e & 1) ? n + 1 + order[e] : 1 + order[e]; }

// solvePathWithGreedy on the matrix
PS_HD void greedy_order(const int* mat, int n, int* order, int* n_order, int* total)
{
    unsigned items = 0, targets = 0;
    int at = 0, cur = 0;
    Cost sum{0, 0};
    for (int step = 0; step < n; ++step) {
        Cost best = inf_cost();
        int pick = -1;
        for (int i = 0; i < n; ++i) {
            if ((items >> i) & 1u) continue;
            const Cost c = entry(mat, cur, 1 + i);
            if (less(c, best)) { best = c; pick = i; }
        }
        if (pick < 0) break;
        items |= 1u << pick;
        cur = 1 + pick;
        order[at++] = pick;
        sum = add(sum, best);
        best = inf_cost();
        pick = -1;
        for (int i = 0; i < n; ++i) {
            if ((targets >> i) & 1u) continue;
            const Cost c = entry(mat, cur, n + 1 + i);
            if (less(c, best)) { best = c; pick = i; }
        }
        if (pick < 0) break;
        targets |= 1u << pick;
        cur = n + 1 + pick;
        order[at++] = pick;
        sum = add(sum, best);
    }
    *n_order = at;
    total[0] = sum.a;
    total[1] = sum.b;
}

// the optimal mode.  step_cost: serve item i next, standing at point `from`, the items of S served: the two legs and what is left
PS_HD Cost step_cost(const int* mat, int n, const int* assign, const Cost* togo, int from, unsigned S, int i)
{
    const int t = n + 1 + (assign ? assign[i] : i);
    const Cost legs = add(entry(mat, from, 1 + i), entry(mat, 1 + i, t));
    return add(legs, togo[(S | (1u << i)) * MAX_TASKS + i]);
}
// togo[S][last] from the states with one more item served; S holds `last`
PS_HD Cost togo_state(const int* mat, int n, const int* assign, const Cost* togo, unsigned S, int last)
{
    if (S == (1u << n) - 1u) return Cost{0, 0};
    const int from = n + 1 + (assign ? assign[last] : last);
    Cost best = inf_cost();
    for (int i = 0; i < n; ++i) {
        if ((S >> i) & 1u) continue;
        const Cost c = step_cost(mat, n, assign, togo, from, S, i);
        if (less(c, best)) best = c;
    }
    return best;
}
PS_HD int popcount(unsigned v)
{
    int c = 0;
    for (; v; v &= v - 1) ++c;
    return c;
}
// forward through the filled table: the lexicographically smallest optimal item sequence.  E_NO_ORDER writes nothing but *n_order
PS_HD int optimal_order(const int* mat, int n, const int* assign, const Cost* togo, int* order, int* n_order, int* total)
{
    *n_order = 0;
    Cost want = inf_cost();
    for (int i = 0; i < n; ++i) {
        const Cost c = step_cost(mat, n, assign, togo, 0, 0u, i);
        if (less(c, want)) want = c;
    }
    if (is_inf(want)) return E_NO_ORDER;
    total[0] = want.a;
    total[1] = want.b;
    unsigned S = 0;
    int from = 0;
    for (int step = 0; step < n; ++step) {
        int pick = -1;
        for (int i = 0; i < n && pick < 0; ++i)
            if (!((S >> i) & 1u) && same(step_cost(mat, n, assign, togo, from, S, i), want)) pick = i;
        if (pick < 0) return E_NO_ORDER; // never: the optimum of a state is attained by one of its steps
        const int t = assign ? assign[pick] : pick;
        order[2 * step] = pick;
        order[2 * step + 1] = t;
        S |= 1u << pick;
        from = n + 1 + t;
        want = togo[S * MAX_TASKS + pick];
    }
    *n_order = 2 * n;
    return OK;
}
// ---- the assigned mode: the matching by dynamic programming over target subsets ------------------------------------------------
// rest[T] from the sets with one more target: item popcount(T) takes a target outside T
PS_HD Cost rest_state(const int* mat, int n, const Cost* rest, unsigned T)
{
    const int k = popcount(T);
    if (k == n) return Cost{0, 0};
    Cost best = inf_cost();
    for (int t = 0; t < n; ++t) {
        if ((T >> t) & 1u) continue;
        const Cost c = add(entry(mat, 1 + k, n + 1 + t), rest[T | (1u << t)]);
        if (less(c, best)) best = c;
    }
    return best;
}
// forward through the filled table: the lexicographically smallest optimal bijection.  E_NO_ORDER writes nothing
PS_HD int matching(const int* mat, int n, const Cost* rest, int* assign, int* assign_total)
{
    Cost want = rest[0];
    if (is_inf(want)) return E_NO_ORDER;
    assign_total[0] = want.a;
    assign_total[1] = want.b;
    unsigned T = 0;
    for (int k = 0; k < n; ++k) {
        int pick = -1;
        for (int t = 0; t < n && pick < 0; ++t)
            if (!((T >> t) & 1u) && same(add(entry(mat, 1 + k, n + 1 + t), rest[T | (1u << t)]), want)) pick = t;
        if (pick < 0) return E_NO_ORDER; // never: the optimum of a state is attained by one of its steps
        assign[k] = pick;
        T |= 1u << pick;
        want = rest[T];
    }
    return OK;
}

// ---- the joint mode: togo[(Si * JOINT_SETS + St) * JOINT_MAX_TASKS + last], Si the served items, St the used targets --------------
PS_HD unsigned joint_index(unsigned Si, unsigned St, int last) { return (Si * JOINT_SETS + St) * JOINT_MAX_TASKS + (unsigned)last; }
// the indices below joint_span(n) hold every state of a mission of n tasks
PS_HD unsigned joint_span(int n) { return joint_index((1u << n) - 1u, (1u << n) - 1u, JOINT_MAX_TASKS - 1) + 1u; }
// index e is a state of the level: as many items served as targets used, `level` of them, the last target among the used
PS_HD bool joint_on_level(int n, unsigned e, int level)
{
    const unsigned sets = e / JOINT_MAX_TASKS, last = e - sets * JOINT_MAX_TASKS, Si = sets / JOINT_SETS, St = sets - Si * JOINT_SETS;
    return (int)last < n && St < (1u << n) && popcount(Si) == level && popcount(St) == level && ((St >> last) & 1u);
}
// serve item i next and carry it to target t, standing at point `from`: the two legs and what is left
PS_HD Cost joint_step(const int* mat, int n, const Cost* togo, int from, unsigned Si, unsigned St, int i, int t)
{
    const Cost legs = add(entry(mat, from, 1 + i), entry(mat, 1 + i, n + 1 + t));
    return add(legs, togo[joint_index(Si | (1u << i), St | (1u << t), t)]);
}
// the least over the free items and targets
PS_HD Cost joint_best(const int* mat, int n, const Cost* togo, int from, unsigned Si, unsigned St)
{
    Cost best = inf_cost();
    for (int i = 0; i < n; ++i) {
        if ((Si >> i) & 1u) continue;
        for (int t = 0; t < n; ++t) {
            if ((St >> t) & 1u) continue;
            const Cost c = joint_step(mat, n, togo, from, Si, St, i, t);
            if (less(c, best)) best = c;
        }
    }
    return best;
}
// the state at index e (joint_on_level) from the states with one more task done
PS_HD Cost joint_state(const int* mat, int n, const Cost* togo, unsigned e)
{
    const unsigned sets = e / JOINT_MAX_TASKS, last = e - sets * JOINT_MAX_TASKS, Si = sets / JOINT_SETS, St = sets - Si * JOINT_SETS;
    if (Si == (1u << n) - 1u) return Cost{0, 0};
    return joint_best(mat, n, togo, n + 1 + (int)last, Si, St);
}
// forward through the filled table: the lexicographically smallest optimal published order, its assignment and the sum of its
// carry legs.  E_NO_ORDER writes nothing but *n_order
PS_HD int joint_order(const int* mat, int n, const Cost* togo, int* order, int* n_order, int* total, int* assign, int* assign_total)
{
    *n_order = 0;
    Cost want = joint_best(mat, n, togo, 0, 0u, 0u);
    if (is_inf(want)) return E_NO_ORDER;
    total[0] = want.a;
    total[1] = want.b;
    unsigned Si = 0, St = 0;
    int from = 0;
    Cost carry{0, 0};
    for (int step = 0; step < n; ++step) {
        int pi = -1, pt = -1;
        for (int i = 0; i < n && pi < 0; ++i) {
            if ((Si >> i) & 1u) continue;
            for (int t = 0; t < n && pi < 0; ++t)
                if (!((St >> t) & 1u) && same(joint_step(mat, n, togo, from, Si, St, i, t), want)) { pi = i; pt = t; }
        }
        if (pi < 0) return E_NO_ORDER; // never: the optimum of a state is attained by one of its steps
        order[2 * step] = pi;
        order[2 * step + 1] = pt;
        assign[pi] = pt;
        carry = add(carry, entry(mat, 1 + pi, n + 1 + pt));
        Si |= 1u << pi;
        St |= 1u << pt;
        from = n + 1 + pt;
        want = togo[joint_index(Si, St, pt)];
    }
    *n_order = 2 * n;
    assign_total[0] = carry.a;
    assign_total[1] = carry.b;
    return OK;
}
// the end points of the legs in visit order
PS_HD void write_legs(const double* pts, int n, const int* order, int n_order, double* leg_start_xy, double* leg_goal_xy)
{
    int prev = 0;
    for (int e = 0; e < n_order; ++e) {
        const int p = order_point(n, order, e);
        leg_start_xy[2 * e] = pts[2 * prev]; leg_start_xy[2 * e + 1] = pts[2 * prev + 1];
        leg_goal_xy[2 * e] = pts[2 * p]; leg_goal_xy[2 * e + 1] = pts[2 * p + 1];
        prev = p;
    }
}

// ---- one mission, serially: words[] holds the window (<= psearch::MAX_CELLS), togo[] STATES pairs (optimal mode) ------------------
struct Out {
    int* matrix;          // [P_MAX][P_MAX][2]
    int* order;           // [MAX_LEGS]
    int* n_order;
    int* total;           // [2]
    double* leg_start_xy; // [MAX_LEGS][2]
    double* leg_goal_xy;
    int *fields, *sweeps;
};
// the matrix and the diagnostics of a checked mission
inline void fill_matrix(const psearch::Grid& g, const Mission& m, const double* pts, const Params& p, unsigned* words, const Out& o)
{
    int cell[P_MAX];
    double dist[P_MAX], safe[P_MAX];
    for (int j = 0; j < m.P; ++j) cell[j] = point_cell(g, m, pts, j, &dist[j]);
    int fields = 0, most = 0;
    for (int k = 0; k < m.P; ++k) put_entry(o.matrix, k, k, Cost{0, 0});
    for (int k = 0; k < m.P - 1; ++k) {
        for (int j = k + 1; j < m.P; ++j) safe[j] = pair_safe(p.safe_dis, dist[k], dist[j]);
        for (int j = k + 1; j < m.P; ++j) {
            bool first = true;
            for (int e = k + 1; e < j; ++e) first = first && !(safe[e] == safe[j]);
            if (!first) continue;
            const psearch::Window w = field_window(m, cell[k], safe[j]);
            for (int x = 0; x < w.wx; ++x)
                for (int y = 0; y < w.wy; ++y) words[x * w.wy + y] = psearch::first_word(g, w, x, y);
            int sweeps = 0;
            for (bool changed = true; changed;) {
                changed = false;
                if (sweeps & 1) {
                    for (int x = w.wx - 1; x >= 0; --x)
                        for (int y = w.wy - 1; y >= 0; --y) changed |= psearch::relax_cell(words, w.wx, w.wy, x, y);
                } else {
                    for (int x = 0; x < w.wx; ++x)
                        for (int y = 0; y < w.wy; ++y) changed |= psearch::relax_cell(words, w.wx, w.wy, x, y);
                }
                ++sweeps;
            }
            ++fields;
            most = sweeps > most ? sweeps : most;
            for (int e = j; e < m.P; ++e) {
                if (!(safe[e] == safe[j])) continue;
                const Cost c = read_cost(words, cell[k], cell[e]);
                put_entry(o.matrix, k, e, c);
                put_entry(o.matrix, e, k, c);
            }
        }
    }
    *o.fields = fields;
    *o.sweeps = most;
}
// togo[] of the optimal routing for `assign`, level by level, then the order
inline int route_one(const int* mat, int n, const int* assign, Cost* togo, const Out& o)
{
    for (int level = n; level >= 1; --level)
        for (unsigned S = 1; S < (1u << n); ++S) {
            if (popcount(S) != level) continue;
            for (int last = 0; last < n; ++last)
                if ((S >> last) & 1u) togo[S * MAX_TASKS + last] = togo_state(mat, n, assign, togo, S, last);
        }
    return optimal_order(mat, n, assign, togo, o.order, o.n_order, o.total);
}
// the order of a mission whose matrix is filled, modes GREEDY and OPTIMAL
inline int order_given(int n, const double* pts, const int* assign, const Params& p, Cost* togo, const Out& o)
{
    int status = OK;
    if (p.mode == OPTIMAL) status = route_one(o.matrix, n, assign, togo, o);
    else greedy_order(o.matrix, n, o.order, o.n_order, o.total);
    if (status == OK) write_legs(pts, n, o.order, *o.n_order, o.leg_start_xy, o.leg_goal_xy);
    return status;
}
inline int plan_one(const psearch::Grid& g, int n, int max_tasks, const double* pts, const int* assign, const Params& p, unsigned* words,
                    Cost* togo, const Out& o)
{
    const Mission m = check_mission(g, n, max_tasks, pts, assign, p.mode, p.window_margin);
    if (m.status != OK) { *o.n_order = 0; return m.status; }
    fill_matrix(g, m, pts, p, words, o);
    return order_given(n, pts, assign, p, togo, o);
}
inline int order_chosen(int n, const double* pts, const Params& p, Cost* table, const Out& o, int* assignment, int* assign_total);
// the modes that choose the assignment (p.mode ASSIGNED or JOINT).  table[]: ASSIGNED_STATES pairs, togo then rest (ASSIGNED), or
// JOINT_STATES pairs (JOINT).  assignment[MAX_TASKS] and assign_total[2] are written as the contract says
inline int plan_one_assigned(const psearch::Grid& g, int n, int max_tasks, const double* pts, const Params& p, unsigned* words, Cost* table,
                             const Out& o, int* assignment, int* assign_total)
{
    const Mission m = check_mission(g, n, task_limit(p.mode, max_tasks), pts, nullptr, p.mode, p.window_margin);
    if (m.status != OK) { *o.n_order = 0; return m.status; }
    fill_matrix(g, m, pts, p, words, o);
    return order_chosen(n, pts, p, table, o, assignment, assign_total);
}
// the order of a mission whose matrix is filled, modes ASSIGNED and JOINT
inline int order_chosen(int n, const double* pts, const Params& p, Cost* table, const Out& o, int* assignment, int* assign_total)
{
    int status;
    if (p.mode == JOINT) {
        for (int level = n; level >= 1; --level)
            for (unsigned e = 0; e < joint_span(n); ++e)
                if (joint_on_level(n, e, level)) table[e] = joint_state(o.matrix, n, table, e);
        int asg[JOINT_MAX_TASKS], sum[2];
        status = joint_order(o.matrix, n, table, o.order, o.n_order, o.total, asg, sum);
        if (status == OK) {
            for (int i = 0; i < n; ++i) assignment[i] = asg[i];
            assign_total[0] = sum[0]; assign_total[1] = sum[1];
        }
    } else {
        Cost* rest = table + STATES;
        for (int level = n; level >= 0; --level)
            for (unsigned T = 0; T < (1u << n); ++T)
                if (popcount(T) == level) rest[T] = rest_state(o.matrix, n, rest, T);
        *o.n_order = 0;
        status = matching(o.matrix, n, rest, assignment, assign_total);
        if (status == OK) status = route_one(o.matrix, n, assignment, table, o);
    }
    if (status == OK) write_legs(pts, n, o.order, *o.n_order, o.leg_start_xy, o.leg_goal_xy);
    return status;
}

} // namespace tplan

#endif
