"""The scene of the object-class tests (tests/test_backend_classes_*.py): four robot models, three problems, one map."""
import ctypes as C

import numpy as np

N_CLASSES = 4


def class_configs():
    """k0 the default; k1 the ICR model with xv 0.2; k2 a heavy, wide object: xv 0.3, slower, more clearance, a third check point;
    k3 xv 0.1, no check points, a slower turn"""
    from alore_legged_manipulator_amd.backend import default_config
    k = [default_config() for _ in range(N_CLASSES)]
    k[1].standard_diff, k[1].icr_xv = 0, 0.2
    k[2].standard_diff, k[2].icr_xv, k[2].max_vel, k[2].max_acc, k[2].safe_dis, k[2].n_check = 0, 0.3, 2.0, 1.0, 0.8, 3
    k[2].check_pts[2][0], k[2].check_pts[2][1] = 0.0, 0.35
    k[3].standard_diff, k[3].icr_xv, k[3].n_check, k[3].max_omega = 0, 0.1, 0, 1.0
    return k


def effective_xv(cfg) -> float:
    return 0.0 if cfg.standard_diff else float(cfg.icr_xv)


def copy_config(cfg):
    out = type(cfg)()
    C.memmove(C.byref(out), C.byref(cfg), C.sizeof(cfg))
    return out


def problems():
    from alore_legged_manipulator_amd.flat_traj import monte_carlo_goals
    return monte_carlo_goals(3, seed=44)


def disc_centres(fts, shift=(0.2, -0.2)):
    return [(0.5 * (ft.start_xytheta[0] + ft.final_xytheta[0]) + shift[0], 0.5 * (ft.start_xytheta[1] + ft.final_xytheta[1]) + shift[1])
            for ft in fts]


def disc_grid(centres, radius=0.4, half=20.0):
    """three discs, one per problem, as an exact distance field"""
    from oracle.backend_driver import EsdfGrid

    def field(X, Y):
        d = None
        for cx, cy in centres:
            q = np.hypot(X - cx, Y - cy) - radius
            d = q if d is None else np.minimum(d, q)
        return d
    return EsdfGrid.from_field(field, half=half)


def stats_numpy(class_of, status, T, n_classes):
    """alore_backend_class_stat per class from status records (a dict of arrays, or a STATUS structured array) and the piece times:
    integer sums, minima and maxima; the duration is the sum of the piece times in piece order"""
    from alore_legged_manipulator_amd.backend import CLASS_STAT_DTYPE
    out = np.zeros(n_classes, CLASS_STAT_DTYPE)
    out["min_dist"] = np.finfo(np.float64).max
    class_of = np.asarray(class_of)
    for k in range(n_classes):
        idx = np.nonzero(class_of == k)[0]
        if not len(idx):
            continue
        ok = status["ok"][idx] != 0
        out["n"][k] = len(idx)
        out["n_ok"][k] = int(ok.sum())
        out["n_collision"][k] = int((status["collision"][idx] != 0).sum())
        out["sum_attempts"][k] = int(status["attempts"][idx].astype(np.int64).sum())
        out["sum_evals"][k] = int(status["evals"][idx].astype(np.int64).sum())
        out["max_evals"][k] = max(0, int(status["evals"][idx].max()))
        if ok.any():
            out["min_dist"][k] = status["min_dist"][idx][ok].min()
            dur = []
            for b in idx[ok]:
                d = 0.0
                for i in range(min(max(int(status["n_pieces"][b]), 0), T.shape[1])):
                    d += float(T[b, i])
                dur.append(d)
            out["max_duration"][k] = max(0.0, max(dur))
    return out
