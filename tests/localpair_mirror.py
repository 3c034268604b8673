"""Host mirror of the local-pair loss kernels (csrc/localpair.hip): numpy only, float64, written from the formulas the kernels and
pdgn_amd/losses.py quote, so that tests can demand equal bits on inputs whose arithmetic is exact in float32.

    Chamfer      P[i,j] = (|x_i|^2 + |y_j|^2) - 2 <x_i, y_j>;  minx[i] = min_j P, argx[i] = the LOWEST j attaining it (numpy's argmin
                 returns the first occurrence, as torch.min and the kernel's strict '<' ascending scan do);  miny / argy over i
    its adjoint  d/dq P[q, c*] = 2 (q - c*), d/dc* = -2 (q - c*):  gx[i] += 2 gminx[i] (x_i - y_argx[i]),  gy[argx[i]] -= the same;
                 gy[j] += 2 gminy[j] (y_j - x_argy[j]),  gx[argy[j]] -= the same
    statistics   mu = (1/K) sum_s p_s,  cov = (1/K) sum_s t_s t_s^T,  t_s = p_s - mu      (compute_mean_covariance)
    its adjoint  dxyz[idx[q,s]] += dmu_q / K + (G + G^T) t_s / K,  G = dcov_q as 3x3      (sum_s t_s = 0 removes the path through mu)

Exactness.  With coordinates on a dyadic grid (hashweights.lattice_points) and upstream gradients that are multiples of 1/4, every
product above is a multiple of a known power of two (the `quantum`) and every sum of them stays below 2^24 quanta: each
intermediate value is then a float32, whatever the order of the additions, whether a product and an addition are contracted into
one fma, and in whatever order atomics arrive.  `assert_exact` checks exactly that on the host, BEFORE a device result is compared,
so a failing bit comparison is the kernel's fault and not the case's."""
import numpy as np

F64 = np.float64


# ---------------------------------------------------------------------------- the exactness guard
def assert_exact(result, quantum, abs_sum=None):
    """`result` (float64): every value finite, a multiple of `quantum` and equal to its own float32 rounding.  `abs_sum`: for every
    destination the sum of the ABSOLUTE values of the terms added into it (the *_abs functions below; default |result|, a single
    term each): multiples of `quantum` too, and below 2^24 quanta -- every partial sum in every order is then a float32."""
    r = np.asarray(result, dtype=F64)
    s = np.abs(r) if abs_sum is None else np.asarray(abs_sum, dtype=F64)
    for name, a in (("result", r), ("abs_sum", s)):
        if not np.isfinite(a).all():
            raise AssertionError("%s is not finite" % name)
        k = a / quantum
        if not np.array_equal(k, np.rint(k)):
            raise AssertionError("%s is not a multiple of the quantum %g (worst remainder %g quanta)"
                                 % (name, quantum, float(np.abs(k - np.rint(k)).max())))
    if s.size and float(s.max()) >= 2.0 ** 24 * quantum:
        raise AssertionError("sum of |terms| reaches %.4g quanta at one destination: not below 2^24" % (float(s.max()) / quantum))
    if not np.array_equal(r, r.astype(np.float32).astype(F64)):
        raise AssertionError("the float64 result is not a float32")


# ---------------------------------------------------------------------------- Chamfer (Gram form)
def gram(x, y):
    """P (b, m, n) for x (b, m, d), y (b, n, d)."""
    x, y = np.asarray(x, dtype=F64), np.asarray(y, dtype=F64)
    rx, ry = (x * x).sum(2), (y * y).sum(2)
    return (rx[:, :, None] + ry[:, None, :]) - 2.0 * np.einsum("bmd,bnd->bmn", x, y)


def gram_abs(x, y):
    """max over (i, j) of |x_i|^2 + |y_j|^2 + 2 sum_c |x_ic| |y_jc|: the sum of |terms| behind the worst entry of P, per sample."""
    x, y = np.abs(np.asarray(x, dtype=F64)), np.abs(np.asarray(y, dtype=F64))
    rx, ry = (x * x).sum(2), (y * y).sum(2)
    return ((rx[:, :, None] + ry[:, None, :]) + 2.0 * np.einsum("bmd,bnd->bmn", x, y)).max(axis=(1, 2))


def chamfer(x, y):
    """-> minx (b, m) float64, argx (b, m) int32, miny (b, n), argy (b, n): both directions' minima of P, first index on ties."""
    x, y = np.asarray(x, dtype=F64), np.asarray(y, dtype=F64)
    b, m, n = x.shape[0], x.shape[1], y.shape[1]
    minx, miny = np.empty((b, m), F64), np.empty((b, n), F64)
    argx, argy = np.empty((b, m), np.int32), np.empty((b, n), np.int32)
    for s in range(b):
        P = gram(x[s:s + 1], y[s:s + 1])[0]
        argx[s], argy[s] = P.argmin(1), P.argmin(0)
        minx[s], miny[s] = P[np.arange(m), argx[s]], P[argy[s], np.arange(n)]
    return minx, argx, miny, argy


def _chamfer_scatter(x, y, argx, argy, gminx, gminy, absolute):
    x, y = np.asarray(x, dtype=F64), np.asarray(y, dtype=F64)
    gminx, gminy = np.asarray(gminx, dtype=F64), np.asarray(gminy, dtype=F64)
    gx, gy = np.zeros_like(x), np.zeros_like(y)
    for s in range(x.shape[0]):
        for own, oth, arg, g, g_own, g_oth in ((x[s], y[s], argx[s], gminx[s], gx[s], gy[s]), (y[s], x[s], argy[s], gminy[s], gy[s], gx[s])):
            arg = np.asarray(arg, dtype=np.int64)
            t = 2.0 * g[:, None] * (own - oth[arg])
            if absolute:
                t = np.abs(t)
            g_own += t
            np.add.at(g_oth, arg, t if absolute else -t)
    return gx, gy


def chamfer_grad(x, y, argx, argy, gminx, gminy):
    """-> gx (b, m, d), gy (b, n, d): the adjoint of `chamfer`'s minima for upstream gradients gminx (b, m), gminy (b, n)."""
    return _chamfer_scatter(x, y, argx, argy, gminx, gminy, False)


def chamfer_grad_abs(x, y, argx, argy, gminx, gminy):
    """The same scatter over the terms' absolute values: per destination, the sum `assert_exact` bounds."""
    return _chamfer_scatter(x, y, argx, argy, gminx, gminy, True)


def _uniform(x, y, g, scale):
    u = F64(np.float32(g)) * F64(np.float32(scale))
    return np.full(np.shape(x)[:2], u, F64), np.full(np.shape(y)[:2], u, F64)


def chamfer_grad_uniform(x, y, argx, argy, g, scale):
    """The adjoint of scale * (sum minx + sum miny) for the upstream scalar g: every minimum's gradient is g * scale."""
    return _chamfer_scatter(x, y, argx, argy, *_uniform(x, y, g, scale), False)


def chamfer_grad_uniform_abs(x, y, argx, argy, g, scale):
    return _chamfer_scatter(x, y, argx, argy, *_uniform(x, y, g, scale), True)


# ---------------------------------------------------------------------------- neighbourhood mean and covariance
def _gathered(xyz, idx):
    xyz, idx = np.asarray(xyz, dtype=F64), np.asarray(idx, dtype=np.int64)
    return xyz[np.arange(xyz.shape[0])[:, None, None], idx]        # (b, m, K, 3)


def local_stats(xyz, idx):
    """xyz (b, n, 3), idx (b, m, K) -> mu (b, m, 3), cov (b, m, 9)."""
    p = _gathered(xyz, idx)
    K = p.shape[2]
    mu = p.sum(2) / K
    t = p - mu[:, :, None, :]
    cov = np.einsum("bmka,bmkc->bmac", t, t) / K
    return mu, cov.reshape(cov.shape[0], cov.shape[1], 9)


def local_stats_abs(xyz, idx):
    """Sums of |terms| behind mu and cov."""
    p = _gathered(xyz, idx)
    K = p.shape[2]
    t = np.abs(p - (p.sum(2) / K)[:, :, None, :])
    cov = np.einsum("bmka,bmkc->bmac", t, t) / K
    return np.abs(p).sum(2) / K, cov.reshape(cov.shape[0], cov.shape[1], 9)


def _stats_scatter(xyz, idx, dmu, dcov, absolute):
    xyz, idx = np.asarray(xyz, dtype=F64), np.asarray(idx, dtype=np.int64)
    p = _gathered(xyz, idx)
    b, m, K = idx.shape
    t = p - (p.sum(2) / K)[:, :, None, :]
    G = np.asarray(dcov, dtype=F64).reshape(b, m, 3, 3)
    S = G + G.transpose(0, 1, 3, 2)
    base = np.asarray(dmu, dtype=F64)[:, :, None, :] / K
    if absolute:                                                   # |dmu| / K + sum_c |S_ac| |t_c| / K bounds every term the kernel adds
        term = np.abs(base) + np.einsum("bmac,bmkc->bmka", np.abs(S), np.abs(t)) / K
    else:
        term = base + np.einsum("bmac,bmkc->bmka", S, t) / K
    out = np.zeros_like(xyz)
    for s in range(b):
        np.add.at(out[s], idx[s].reshape(-1), term[s].reshape(-1, 3))
    return out


def local_stats_grad(xyz, idx, dmu, dcov):
    """-> dxyz (b, n, 3): the adjoint of `local_stats` for upstream gradients dmu (b, m, 3), dcov (b, m, 9)."""
    return _stats_scatter(xyz, idx, dmu, dcov, False)


def local_stats_grad_abs(xyz, idx, dmu, dcov):
    return _stats_scatter(xyz, idx, dmu, dcov, True)
