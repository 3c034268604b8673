"""Host mirror of the learning-rate schedule (csrc/adam.hip: lr_factor; include/pdgn_hip.h, "learning-rate schedule"): numpy only,
the arithmetic the header fixes, so that tests can demand equal bits.  A restatement, not an import of pdgn_amd/schedule.py.

    tab[0] = n (1 .. 16 knots), tab[1 + 2i] = t_i, tab[2 + 2i] = f_i            33 float64 words
    f(t) = f_0 for t <= t_0;  f_{n-1} for t >= t_{n-1};  else, for the first i (from 0) with t < t_{i+1},
    f(t) = f_i + (f_{i+1} - f_i) * ((t - t_i) / (t_{i+1} - t_i))                four float64 operations, each rounded on its own
    lr_eff = lr * f(t)                                                          one more
    a malformed table (n no integer in 1 .. 16, some t_{i+1} > t_i false) gives f_0
"""
import numpy as np

MAX_KNOTS, TABLE_DOUBLES = 16, 33


def table(knots):
    """The 33 words of a knot list [(t, f), ...] (no validation: the tests write malformed ones on purpose)."""
    tab = np.zeros(TABLE_DOUBLES, dtype=np.float64)
    tab[0] = len(knots)
    for i, (t, f) in enumerate(knots[:MAX_KNOTS]):
        tab[1 + 2 * i], tab[2 + 2 * i] = t, f
    return tab


def factor(tab, t):
    tab = np.asarray(tab, dtype=np.float64)
    assert tab.shape == (TABLE_DOUBLES,)
    t = np.float64(t)
    n, f0 = tab[0], tab[2]
    if not (n >= 1 and n <= MAX_KNOTS) or n != np.floor(n):
        return f0
    n = int(n)
    ts, fs = tab[1:1 + 2 * n:2], tab[2:2 + 2 * n:2]
    if not np.all(ts[1:] > ts[:-1]):
        return f0
    if t <= ts[0]:
        return f0
    if not t < ts[-1]:
        return fs[-1]
    i = int(np.nonzero(t < ts[1:])[0][0])
    num = np.subtract(t, ts[i], dtype=np.float64)
    den = np.subtract(ts[i + 1], ts[i], dtype=np.float64)
    rise = np.subtract(fs[i + 1], fs[i], dtype=np.float64)
    return np.add(fs[i], np.multiply(rise, np.divide(num, den, dtype=np.float64), dtype=np.float64), dtype=np.float64)


def lr_eff(lr, tab, t):
    return np.multiply(np.float64(lr), factor(tab, t), dtype=np.float64)


def lr32(lr, tab, t):
    """What the routes through torch's kernel run at: lr_eff rounded to float32."""
    return np.float32(lr_eff(lr, tab, t))
