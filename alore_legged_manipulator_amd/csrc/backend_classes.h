// backend_classes.h -- object classes of the back_end: one robot model (a whole alore_backend_config) per problem slot, the
// arithmetic once (internal).  Plain C++17: __host__ __device__ under hipcc, no HIP dependency otherwise.
// What is stated here and nowhere else:
//   invalid_field     what alore_backend_create refuses in a config, as the name of the first offending field;
//   sizing_mismatch   the fields of a class that size a device buffer or a launch and so must equal the handle's;
//   effective_xv      the ICR offset a config integrates its paths with: 0 for the standard differential model;
//   Stat / stat_*     the per-class outcome of a plan launch (alore_backend_class_stat) as order-independent reductions --
//                     integer sums, minima and maxima -- so that any grouping of the slots gives the same bits;
//   plan_duration     the sum of the piece times in piece order, as fleet::end forms it.
// class_stats_kernel (backend_capi.hip) folds with stat_add / stat_merge; tests/harness/backend_classes_check.cpp runs reduce()
// and the validation on the CPU.
#ifndef ALORE_BACKEND_CLASSES_H
#define ALORE_BACKEND_CLASSES_H

#include "../../include/alore_backend.h"

#if defined(__HIPCC__)
#define BCLASS_HD __host__ __device__ inline
#else
#define BCLASS_HD inline
#endif

namespace bclass {

constexpr int MAX_CLASSES = 256;
constexpr int MEM_MAX = 256;  // backend::MEM_MAX: history slots per problem
constexpr double BIG = 1.79769313486231570815e+308; // DBL_MAX

using Config = alore_backend_config;
using Status = alore_backend_status;
using Stat = alore_backend_class_stat;

// the checks of alore_backend_create on a config: null, or the first field that fails them
BCLASS_HD const char* invalid_field(const Config& c)
{
    if (c.sparse_res != 8) return "sparse_res";
    if (c.n_check < 0 || c.n_check > 8) return "n_check";
    if (c.lbfgs.mem_size < 1 || c.lbfgs.mem_size > MEM_MAX) return "lbfgs.mem_size";
    if (c.path_lbfgs.mem_size < 1 || c.path_lbfgs.mem_size > MEM_MAX) return "path_lbfgs.mem_size";
    if (c.lbfgs.past > 16) return "lbfgs.past";
    if (c.path_lbfgs.past > 16) return "path_lbfgs.past";
    if (c.shot_path_past > 16) return "shot_path_past";
    if (c.final_check_num < 1 || c.final_check_num > 64) return "final_check_num";
    return nullptr;
}

// Fields that size a device buffer or a launch: sparse_res (the Simpson nodes per piece fix the LDS layout of the optimiser).
// Everything else -- limits, weights, clearances, check points, the ICR, ALM and L-BFGS parameters (the history is sized for
// MEM_MAX slots whatever mem_size says), final_check_num -- is read per slot.
BCLASS_HD const char* sizing_mismatch(const Config& c, const Config& handle)
{
    if (c.sparse_res != handle.sparse_res) return "sparse_res";
    return nullptr;
}

// null, or the field that keeps `c` from being a class of a handle created with `handle`
BCLASS_HD const char* class_error(const Config& c, const Config& handle)
{
    if (const char* f = sizing_mismatch(c, handle)) return f;
    return invalid_field(c);
}

BCLASS_HD double effective_xv(const Config& c) { return c.standard_diff ? 0.0 : c.icr_xv; }

// the index a device route reads, brought into [0, n): below 0 is class 0, beyond the table its last class
BCLASS_HD int clamp_class(int k, int n) { return k < 0 ? 0 : (k >= n ? n - 1 : k); }

BCLASS_HD double plan_duration(const double* T, int n_pieces)
{
    double total = 0.0;
    for (int i = 0; i < n_pieces; ++i) total += T[i];
    return total;
}

BCLASS_HD void stat_init(Stat& s)
{
    s.n = s.n_ok = s.n_collision = s.sum_attempts = 0;
    s.sum_evals = 0;
    s.max_evals = 0;
    s.pad = 0;
    s.min_dist = BIG;
    s.max_duration = 0.0;
}

// one slot's status record and the duration of its plan
BCLASS_HD void stat_add(Stat& s, const Status& st, double duration)
{
    s.n += 1;
    s.n_ok += st.ok != 0 ? 1 : 0;
    s.n_collision += st.collision != 0 ? 1 : 0;
    s.sum_attempts += st.attempts;
    s.sum_evals += (long long)st.evals;
    s.max_evals = st.evals > s.max_evals ? st.evals : s.max_evals;
    if (st.ok != 0) {
        s.min_dist = st.min_dist < s.min_dist ? st.min_dist : s.min_dist;
        s.max_duration = duration > s.max_duration ? duration : s.max_duration;
    }
}

BCLASS_HD void stat_merge(Stat& s, const Stat& o)
{
    s.n += o.n;
    s.n_ok += o.n_ok;
    s.n_collision += o.n_collision;
    s.sum_attempts += o.sum_attempts;
    s.sum_evals += o.sum_evals;
    s.max_evals = o.max_evals > s.max_evals ? o.max_evals : s.max_evals;
    s.min_dist = o.min_dist < s.min_dist ? o.min_dist : s.min_dist;
    s.max_duration = o.max_duration > s.max_duration ? o.max_duration : s.max_duration;
}

// the pieces of slot b that the duration sums: the record's n_pieces inside the slab's row
BCLASS_HD int pieces_of(const Status& st, int P) { return st.n_pieces < 0 ? 0 : (st.n_pieces > P ? P : st.n_pieces); }

// out[k], k < n_classes: the slots 0..count-1 of class k (class_of null: every slot is class 0; an index outside the table is
// counted nowhere).  T: [count][P] piece times.
BCLASS_HD void reduce(const int* class_of, const Status* status, const double* T, int P, int count, int n_classes, Stat* out)
{
    for (int k = 0; k < n_classes; ++k) stat_init(out[k]);
    for (int b = 0; b < count; ++b) {
        const int k = class_of ? class_of[b] : 0;
        if (k < 0 || k >= n_classes) continue;
        stat_add(out[k], status[b], plan_duration(T + (long long)b * P, pieces_of(status[b], P)));
    }
}

} // namespace bclass

#endif
