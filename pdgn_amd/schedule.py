"""Learning-rate schedules as the Adam launches read them (include/pdgn_hip.h, "learning-rate schedule").

A schedule is a list of knots (t_i, f_i): a piecewise-linear factor f(t) of Adam's step count t, constant before the first and
after the last knot.  At most MAX_KNOTS = 16 knots, t finite, non-negative and strictly increasing, f finite and non-negative.  On
the device it is a table of TABLE_DOUBLES = 33 fp64 words -- tab[0] = n, tab[1 + 2i] = t_i, tab[2 + 2i] = f_i -- that the kernels of
csrc/adam.hip evaluate from their own step counter: rate = lr * f(t), with t the count of the update being made (1 for the first).

`knots` compiles the named kinds, `validate` checks a list, `table` makes the device tensor, `factor` is the host evaluation: the
header's expressions in Python floats (IEEE fp64, every operation rounded on its own), the same bits as the device's."""
import math

MAX_KNOTS = 16                  # PDGN_LR_MAX_KNOTS
TABLE_DOUBLES = 33              # PDGN_LR_TABLE_DOUBLES
KINDS = ("constant", "linear", "cosine", "step")


def knots(kind, total_iters, warmup_iters=0, final_factor=0.0, step_iters=None, gamma=0.1):
    """The knot list [(t, f), ...] of a named schedule over `total_iters` updates (T), after `warmup_iters` (W) of linear warm-up.

    constant  [(0, 1)]; every kind with W > 0 starts [(0, 0), (W, 1)] instead: update t <= W runs at t / W of the rate.
    linear    ... + (T, final_factor): a straight line from 1 at W to final_factor at T.
    cosine    final + (1 - final) (1 + cos(pi u)) / 2 with u = (t - W) / (T - W), on all the knots that are left (16, or 15 behind a
              warm-up), equally spaced in t over [W, T]; the first is exactly 1, the last exactly final_factor.  Between knots the
              factor is the chord: for a knot spacing h in u * pi (h = pi / 15, or pi / 14 behind a warm-up) it is off the
              cosine by at most h^2 / 16 of the range 1 - final (the chord error h^2 / 8 * max|g''| of g = (1 + cos x) / 2, whose
              second derivative is at most 1 / 2): 0.27 %, or 0.31 %, of the range.
    step      a drop by `gamma` every `step_iters` (s) updates, as torch's StepLR counts them: updates 1 .. s at 1, s + 1 .. 2s at
              gamma, ...: for every k >= 1 with k s < T the pair (k s, gamma^(k-1)), (k s + 1, gamma^k).  Raises ValueError if
              the drops do not fit into 16 knots (7 drops) or the first drop is not behind the warm-up."""
    T, W = float(total_iters), float(warmup_iters)
    if kind not in KINDS:
        raise ValueError("lr schedule %r: one of %s" % (kind, ", ".join(KINDS)))
    if not (math.isfinite(T) and T >= 1):
        raise ValueError("total_iters must be at least one, got %r" % (total_iters,))
    if not (math.isfinite(W) and W >= 0):
        raise ValueError("warmup_iters must not be negative, got %r" % (warmup_iters,))
    final = float(final_factor)
    if not (math.isfinite(final) and final >= 0):
        raise ValueError("final_factor must be finite and not negative, got %r" % (final_factor,))
    ks = [(0.0, 0.0), (W, 1.0)] if W > 0 else [(0.0, 1.0)]
    if kind in ("linear", "cosine") and not W < T:
        raise ValueError("the warm-up (%g updates) leaves nothing of the %g updates to decay over" % (W, T))
    if kind == "linear":
        ks.append((T, final))
    elif kind == "cosine":
        left = MAX_KNOTS - len(ks) + 1                           # (the knot at W is the cosine's first)
        ks.pop()
        for j in range(left):
            u = j / (left - 1)
            f = 1.0 if j == 0 else final if j == left - 1 else final + (1.0 - final) * (1.0 + math.cos(math.pi * u)) / 2.0
            ks.append((W + (T - W) * j / (left - 1) if j < left - 1 else T, f))
    elif kind == "step":
        if step_iters is None or not (math.isfinite(float(step_iters)) and float(step_iters) >= 1):
            raise ValueError("a step schedule needs step_iters >= 1, got %r" % (step_iters,))
        s, g = float(step_iters), float(gamma)
        if not (math.isfinite(g) and g > 0):
            raise ValueError("gamma must be positive, got %r" % (gamma,))
        if not W < s:
            raise ValueError("the first drop (update %g) must come behind the warm-up (%g updates)" % (s, W))
        k = 1
        while k * s < T:
            if len(ks) + 2 > MAX_KNOTS:
                raise ValueError("a step schedule with a drop every %g of %g updates has more drops than fit into %d knots"
                                 % (s, T, MAX_KNOTS))
            ks += [(k * s, g ** (k - 1)), (k * s + 1.0, g ** k)]
            k += 1
    validate(ks)
    return ks


def validate(knots):
    """Raises ValueError unless `knots` is 1 .. 16 pairs (t, f) with t finite, >= 0 and strictly increasing and f finite and >= 0.
    Returns the list as pairs of floats."""
    try:
        ks = [(float(t), float(f)) for t, f in knots]
    except (TypeError, ValueError):
        raise ValueError("an lr schedule is a list of (t, factor) pairs, got %r" % (knots,)) from None
    if not 1 <= len(ks) <= MAX_KNOTS:
        raise ValueError("an lr schedule has 1 .. %d knots, got %d" % (MAX_KNOTS, len(ks)))
    for i, (t, f) in enumerate(ks):
        if not (math.isfinite(t) and t >= 0):
            raise ValueError("knot %d: t must be finite and not negative, got %r" % (i, t))
        if not (math.isfinite(f) and f >= 0):
            raise ValueError("knot %d: the factor must be finite and not negative, got %r" % (i, f))
        if i and not t > ks[i - 1][0]:
            raise ValueError("knot %d: t must increase strictly (%r after %r)" % (i, t, ks[i - 1][0]))
    return ks


def words(knots):
    """The 33 table words of a validated knot list, as Python floats."""
    ks = validate(knots)
    out = [float(len(ks))]
    for t, f in ks:
        out += [t, f]
    return out + [0.0] * (TABLE_DOUBLES - len(out))


def table(knots, device=None):
    """The schedule as the kernels read it: one torch.float64 tensor of TABLE_DOUBLES words on `device` (validated first)."""
    import torch
    return torch.tensor(words(knots), dtype=torch.float64, device=device)


def _table_words(knots_or_table):
    if hasattr(knots_or_table, "detach"):                        # a torch tensor
        w = [float(x) for x in knots_or_table.detach().cpu().reshape(-1).tolist()]
    elif hasattr(knots_or_table, "dtype") and hasattr(knots_or_table, "ravel"):   # a numpy array
        w = [float(x) for x in knots_or_table.ravel().tolist()]
    else:
        return words(knots_or_table)
    if len(w) != TABLE_DOUBLES:
        raise ValueError("an lr table has %d words, got %d" % (TABLE_DOUBLES, len(w)))
    return w


def factor(knots_or_table, t):
    """f(t) of a knot list or of a 33-word table (torch tensor or numpy array), on the host, by the header's expressions: f_0 up to
    the first knot, f_{n-1} from the last, else f_i + (f_{i+1} - f_i) * ((t - t_i) / (t_{i+1} - t_i)) on the first segment (scanned
    from 0) with t < t_{i+1}, every operation an fp64 one rounded on its own.  A malformed TABLE (n no integer in 1 .. 16, t not
    increasing) gives f_0, as on the device; a malformed knot list raises."""
    w, t = _table_words(knots_or_table), float(t)
    nd, f0 = w[0], w[2]
    if not 1.0 <= nd <= float(MAX_KNOTS) or nd != int(nd):
        return f0
    n, seg = int(nd), -1
    for i in range(n - 1):
        if not w[3 + 2 * i] > w[1 + 2 * i]:
            return f0
        if seg < 0 and t < w[3 + 2 * i]:
            seg = i
    if t <= w[1]:
        return f0
    if seg < 0:
        return w[2 * n]
    ti, fi, tj, fj = w[1 + 2 * seg], w[2 + 2 * seg], w[3 + 2 * seg], w[4 + 2 * seg]
    return fi + (fj - fi) * ((t - ti) / (tj - ti))


def lr_eff(lr, knots_or_table, t):
    """The rate of update t: lr * f(t) in fp64."""
    return float(lr) * factor(knots_or_table, t)
