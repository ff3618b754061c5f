// The reference's pivot rules, each stated once.  Functions of scalars only: no memory, no DevState, no side effects.  Every
// kernel that prices or tests ratios calls these; it keeps its own loads, stores and NaN flag (s_nan in the LU-per-iteration
// loops, st->nan_flag in the explicit-inverse kernels).  The dual leaving-row rule is dual_violation (ellp_engine.hip): its
// one body loads a bound only on the branch that needs it, so it takes the arrays; dual_violation_v calls it on values.

// Primal entering key of a nonbasic column with reduced cost rj and label nb (primal…:253-270): -inf where the column is
// not a candidate (|rj| < EPS, the wrong sign for its bound, or rj NaN: the caller raises its flag on rj != rj).
__device__ __forceinline__ double primal_key(double rj, int nb, double eps) {
    double key = -INFINITY;
    if (rj == rj && !(fabs(rj) < eps)) {
        const bool pos = rj > 0.0;
        if (pos && nb == ELLP_NB_UPPER) key = rj;
        else if (!pos && nb == ELLP_NB_LOWER) key = -rj;
        else if (nb == ELLP_NB_FREE) key = fabs(rj);
    }
    return key;
}

// Dual ratio test: does the column with (sign-adjusted) row entry al and label nb take part (dual…:263-278)?  The caller
// forms d_j / al and tests it for NaN.
__device__ __forceinline__ bool dual_keep(double al, int nb, double eps) {
    if (nb == ELLP_NB_LOWER) return al > eps;
    if (nb == ELLP_NB_UPPER) return al < -eps;
    return true;
}

// Primal bounded ratio lambda_i of a basic row (primal…:320-367): d_i the (signed) FTRAN entry, x_i / lb_i / ub_i / kind of
// the row's variable.  +inf where the row does not bound the step; NaN only from the division (the caller raises its flag on
// li != li).
__device__ __forceinline__ double primal_lambda(double di, double xi, double lbi, double ubi, int kind, double eps) {
    double li = INFINITY;
    if (!(fabs(di) < eps)) {
        if (kind == ELLP_BOUND_FREE) li = INFINITY;
        else if (kind == ELLP_BOUND_LOWER) {
            if (di > 0.0) li = INFINITY;
            else if (xi > lbi) li = (lbi - xi) / di;
            else li = 0.0;
        } else if (kind == ELLP_BOUND_UPPER) {
            if (di > 0.0) li = (xi < ubi) ? (ubi - xi) / di : 0.0;
            else li = INFINITY;
        } else if (kind == ELLP_BOUND_TWOSIDED) {
            if (di > 0.0) li = (xi < ubi) ? (ubi - xi) / di : 0.0;
            else if (xi < lbi) li = (lbi - xi) / di;  // quirk Q1 (primal…:359)
            else li = 0.0;
        } else li = 0.0;  // Fixed
    }
    return li;
}
