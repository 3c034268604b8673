"""Host mirror of the gradient guard's record (include/pdgn_hip.h, pdgn_guard_record; csrc/adam.hip, gradnorm_final_kernel): numpy
only, the expressions the header fixes.

    total   = sum of g^2 over the whole list                 float64 (every square and every addition)
    norm    = float32(sqrt(total))                           the float64 root, rounded once
    coef    = float32(min(1, max_norm / (sqrt(total) + 1e-6)))   in float64, for a finite total and a finite max_norm > 0;
              exactly 1 for max_norm <= 0 or infinite ("no clipping") and for a non-finite total (nothing is applied then)
    applied = 1 if total is finite else 0;   found_inf = 1 - applied
"""
import numpy as np


def total_of(arrays):
    """The float64 sum of squares of a list of float32 arrays (numpy's pairwise order: the order of the additions is not part of
    the contract, their precision is)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float64(sum(np.sum(np.square(np.asarray(a, dtype=np.float64))) for a in arrays))


def record(total, max_norm):
    """{norm, coef, applied, found_inf} from the float64 total."""
    total, max_norm = np.float64(total), np.float64(max_norm)
    finite = bool(np.isfinite(total))
    with np.errstate(invalid="ignore"):
        norm64 = np.sqrt(total)
    coef = np.float32(1.0)
    if finite and max_norm > 0 and np.isfinite(max_norm):
        coef = np.float32(min(np.float64(1.0), max_norm / (norm64 + np.float64(1e-6))))
    return {"norm": np.float32(norm64), "coef": coef, "applied": np.float32(1.0 if finite else 0.0),
            "found_inf": np.float32(0.0 if finite else 1.0)}


def ulps(a, b):
    """Distance of two finite float32 values of one sign in units in the last place."""
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))
