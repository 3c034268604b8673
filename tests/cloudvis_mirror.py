"""numpy restatement of csrc/cloudvis.hip (include/pdgn_hip.h: pdgn_cloud_normal_votes and pdgn_orient_pool): the
rules of the kernel file's header block, the snap and the vote's weight in fp32 with every operation rounded on its own, everything else
on integers, so that the kernels and this file agree bit for bit.  Used by tests/test_cloudvis_host.py and tests/test_gpu_cloudvis.py;
imports nothing of pdgn_amd."""
import numpy as np

from normals_mirror import dot3, same_bits  # noqa: F401  (same_bits: for the tests that import this module)
from visible_mirror import snap

F = np.float32
EMPTY = 0xFFFFFFFF
SIGN = np.uint32(0x80000000)
MAX_ROUNDS = 4
DEFAULTS = dict(views=26, resolution=64, radius_factor=2.0, bias_factor=0.25, rounds=1, k=16)      # pointops.orient_normals_visible's


def live_points(x, g):
    """All three coordinates and all three normal components finite."""
    return np.isfinite(x).all(axis=1) & np.isfinite(g).all(axis=1)


def depth_buffer(X, Y, Z, R, splat):
    """Pass 1 for one (cloud, view): the snapped live points (int64 arrays) -> (R,R) int64 buffer, indexed [py, px]."""
    buf = np.full((R, R), EMPTY, dtype=np.int64)
    if X.size == 0:
        return buf
    splat = int(splat)
    np.minimum.at(buf, (np.minimum(Y >> 8, R - 1), np.minimum(X >> 8, R - 1)), Z)
    px0, px1 = np.maximum((X - splat - 128 + 255) >> 8, 0), np.minimum((X + splat - 128) >> 8, R - 1)
    py0, py1 = np.maximum((Y - splat - 128 + 255) >> 8, 0), np.minimum((Y + splat - 128) >> 8, R - 1)
    for oy in range(int(max((py1 - py0).max() + 1, 0))):
        py = py0 + oy
        for ox in range(int(max((px1 - px0).max() + 1, 0))):
            px = px0 + ox
            ok = (py <= py1) & (px <= px1)
            ok &= (256 * px + 128 - X) ** 2 + (256 * py + 128 - Y) ** 2 <= splat * splat
            np.minimum.at(buf, (py[ok], px[ok]), Z[ok])
    return buf


def votes_cloud(x, g, frame, views, R, splat, bias, return_passes=False):
    """One cloud: x, g (n,3), frame (4), views (NV,3,3), integers R, splat (sub-pixel units), bias (depth quanta) -> votes (n,2) uint32
    [, passes (NV,n) bool]."""
    x, g = np.ascontiguousarray(x, dtype=F), np.ascontiguousarray(g, dtype=F)
    views = np.asarray(views, dtype=F).reshape(-1, 3, 3)
    n = x.shape[0]
    live = live_points(x, g)
    votes = np.zeros((n, 2), dtype=np.uint32)
    seen = np.zeros((views.shape[0], n), dtype=bool)
    at = np.flatnonzero(live)
    for v, view in enumerate(views):
        P = snap(x[at], frame, view, R)
        X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
        buf = depth_buffer(X, Y, Z, R, splat)
        passes = Z <= buf[np.minimum(Y >> 8, R - 1), np.minimum(X >> 8, R - 1)] + int(bias)
        seen[v, at] = passes
        s = dot3(g[at], np.broadcast_to(view[2], (at.size, 3))).astype(F)
        with np.errstate(all="ignore"):
            w = (np.minimum(np.abs(s), F(1.0)) * F(256.0)).astype(F)
        w = np.where(np.isnan(s), F(0.0), w).astype(np.uint32)
        votes[at, 0] += np.where(passes & (s < 0), w, 0).astype(np.uint32)
        votes[at, 1] += np.where(passes & (s > 0), w, 0).astype(np.uint32)
    return (votes, seen) if return_passes else votes


def votes(x, g, frame, views, R, splat, bias):
    """x, g (b,n,3), frame (b,4) -> votes (b,n,2) uint32."""
    return np.stack([votes_cloud(xc, gc, fc, views, R, splat, bias) for xc, gc, fc in zip(x, g, np.asarray(frame, dtype=F))])


def coefficients(x, g, idx):
    """The surviving slots of one cloud as (i, j, c) arrays, c in {-1, 0, 1} int64; a repeated slot appears as often as it occurs."""
    n, k = idx.shape
    live = live_points(x, g)
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = np.asarray(idx).astype(np.int64).reshape(-1)
    ok = (j >= 0) & (j < n)
    js = np.where(ok, j, 0)                                         # (never dereferenced where outside)
    ok &= (js != i) & live[i] & live[js]
    i, j = i[ok], js[ok]
    with np.errstate(all="ignore"):
        d = (x[j] - x[i]).astype(F)
        lim = (F(0.25) * dot3(d, d)).astype(F)
        a, a2, t = dot3(d, g[i]).astype(F), dot3(d, g[j]).astype(F), dot3(g[i], g[j]).astype(F)
        keep = ((a * a).astype(F) <= lim) & ((a2 * a2).astype(F) <= lim) & (np.abs(t) > F(0.5))
    return i, j, np.where(keep, np.where(t > 0, 1, -1), 0).astype(np.int64)


def pool_cloud(x, g, idx, vote, rounds):
    """One cloud: x, g (n,3), idx (n,k), vote (n,2) uint32 -> (o (n,3) fp32, pooled (n,) int64, (flipped, undecided, unseen, dead))."""
    x, g = np.ascontiguousarray(x, dtype=F), np.ascontiguousarray(g, dtype=F)
    idx, vote = np.asarray(idx), np.asarray(vote).astype(np.int64)
    assert 0 <= int(rounds) <= MAX_ROUNDS
    live = live_points(x, g)
    v = np.where(live, vote[:, 0] - vote[:, 1], 0).astype(np.int64)
    i, j, c = coefficients(x, g, idx)
    for _ in range(int(rounds)):
        nxt = 2 * v
        np.add.at(nxt, i, c * v[j])
        v = np.where(live, nxt, 0)
    flip = v < 0
    o = g.copy()
    o.view(np.uint32)[flip] ^= SIGN
    stats = (int(flip.sum()), int((live & (v == 0)).sum()), int((live & (vote.sum(axis=1) == 0)).sum()), int((~live).sum()))
    return o, v, stats


def pool(x, g, idx, vote, rounds):
    """x, g (b,n,3), idx (b,n,k), vote (b,n,2) -> (o (b,n,3), pooled (b,n) int64, stats (b,4) int32)."""
    out = [pool_cloud(xc, gc, ic, vc, rounds) for xc, gc, ic, vc in zip(np.asarray(x, dtype=F), np.asarray(g, dtype=F), np.asarray(idx), np.asarray(vote))]
    return np.stack([r[0] for r in out]), np.stack([r[1] for r in out]), np.array([r[2] for r in out], dtype=np.int32).reshape(-1, 4)


# ---------------------------------------------------------------------------- the host side of pointops.normal_votes, in numpy
def cloud_frame(x):
    """pointops.cloud_frames for one cloud: the box centre of the finite points and the largest distance from it times (1 + 2^-10), fp64,
    rounded once; (0, 0, 0, 1) for a cloud without a finite point."""
    p = np.asarray(x, dtype=F).astype(np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    if p.shape[0] == 0:
        return np.array([0, 0, 0, 1], dtype=F)
    ctr = (p.min(axis=0) + p.max(axis=0)) / 2.0
    rho = np.sqrt(((p - ctr) ** 2).sum(axis=1).max()) * (1.0 + 2.0 ** -10)
    return np.concatenate([ctr, [rho if rho > 0 else 1.0]]).astype(F)


def mean_spacing(x):
    """The mean distance to the nearest other point, fp64, all pairs of the points with finite coordinates."""
    p = np.asarray(x, dtype=np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    return float(np.sqrt(d2.min(axis=1)).mean())


def quanta(radius, bias, rho, R):
    """World lengths to the kernel's integers: splat = rint(radius / rho * R 2^7) sub-pixel units, bias = rint(bias / rho * 2^20) depth
    quanta (fp64, rounded once)."""
    return int(np.rint(float(radius) / float(rho) * R * 128.0)), int(np.rint(float(bias) / float(rho) * 1048576.0))


# ---------------------------------------------------------------------------- test shapes
def slab(n, t, seed):
    """n points uniform by area on the surface of the box 1 x 1 x t centred at the origin -> (points (n,3) fp32, outward normals (n,3))."""
    rng = np.random.default_rng(seed)
    half = np.array([0.5, 0.5, t / 2.0])
    area = np.array([t, t, t, t, 1.0, 1.0])                         # faces -x, +x, -y, +y, -z, +z
    face = rng.choice(6, size=n, p=area / area.sum())
    p = rng.uniform(-1.0, 1.0, size=(n, 3)) * half
    axis, side = face // 2, (face % 2) * 2.0 - 1.0
    p[np.arange(n), axis] = side * half[axis]
    nrm = np.zeros((n, 3))
    nrm[np.arange(n), axis] = side
    return p.astype(F), nrm


def wrong_and_undecided(o, pooled, analytic, estimate=None):
    """Among the SURE points (|g . analytic| > 0.8, g the unoriented estimate, `o` where none is given): (sure, wrong: o . analytic < 0
    and decided, undecided: pooled == 0; pooled None: no point counts as undecided)."""
    g = np.asarray(o if estimate is None else estimate, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        sure = np.abs((g * analytic).sum(axis=1)) > 0.8
        side = (np.asarray(o, dtype=np.float64) * analytic).sum(axis=1)
    undecided = np.zeros_like(sure) if pooled is None else np.asarray(pooled) == 0
    return int(sure.sum()), int((sure & ~undecided & (side < 0)).sum()), int((sure & undecided).sum())
