"""numpy restatement of csrc/normals.hip (include/pdgn_hip.h: pdgn_estimate_normals) and of the lit shade of
csrc/render.hip (pdgn_render_sheet_lit), on top of tests/render_mirror.py: the operation order of the kernel file's header block, looped
over the neighbour slots and vectorised over the points.  numpy's float32 ufuncs round every operation on its own, as the kernel's
__fadd_rn / __fsub_rn / __fmul_rn / __fdiv_rn and sqrtf do, so the two agree bit for bit.  Used by tests/test_normals_host.py and
tests/test_gpu_normals.py; imports nothing of pdgn_amd."""
import numpy as np

import render_mirror as rm

F = np.float32
MAX_K = 64
SWEEPS = 5
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))                          # (p, q, the remaining index r), in the order of a sweep
ORIENT = {None: 0, "direction": 1, "towards": 2, "away": 3}


def covariance(x, idx):
    """One cloud x (n, 3) fp32, idx (n, k) with every index inside [0, n) -> (a {(i, j): (n,) fp32, i <= j}, the means (n, 3))."""
    n, k = idx.shape
    invk = F(1.0) / F(k)
    zero = np.zeros(n, F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = [zero, zero, zero]
        for slot in range(k):
            p = x[idx[:, slot]]
            s = [s[c] + p[:, c] for c in range(3)]
        mu = [s[c] * invk for c in range(3)]
        a = {(i, j): zero for i in range(3) for j in range(i, 3)}
        for slot in range(k):
            p = x[idx[:, slot]]
            d = [p[:, c] - mu[c] for c in range(3)]
            for i, j in a:
                a[(i, j)] = a[(i, j)] + d[i] * d[j]
        a = {ij: v * invk for ij, v in a.items()}
    return a, np.stack(mu, axis=1)


def _get(a, i, j):
    return a[(i, j) if i <= j else (j, i)]


def _set(a, i, j, v):
    a[(i, j) if i <= j else (j, i)] = v


def jacobi(a, sweeps=SWEEPS):
    """The cyclic Jacobi iteration of the header block: a {(i, j): (n,)} -> (diagonal [3 x (n,)], V [[3 x (n,)] x 3] as V[row][column]).
    A pair whose off-diagonal element is 0 is skipped, point by point (np.where keeps the old values there)."""
    a = dict(a)
    n = a[(0, 0)].shape[0]
    one, two, zero = F(1.0), F(2.0), np.zeros(n, F)
    V = [[(np.ones(n, F) if r == c else zero) for c in range(3)] for r in range(3)]
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q, r in PAIRS:
                apq, app, aqq = _get(a, p, q), _get(a, p, p), _get(a, q, q)
                on = ~(apq == 0)
                theta = (aqq - app) / (two * apq)
                t = one / (np.abs(theta) + np.sqrt(theta * theta + one))
                t = np.where(theta < 0, -t, t)
                c = one / np.sqrt(t * t + one)
                s = t * c
                tap = t * apq
                arp, arq = _get(a, r, p), _get(a, r, q)
                _set(a, p, p, np.where(on, app - tap, app))
                _set(a, q, q, np.where(on, aqq + tap, aqq))
                _set(a, p, q, np.where(on, zero, apq))
                _set(a, r, p, np.where(on, c * arp - s * arq, arp))
                _set(a, r, q, np.where(on, s * arp + c * arq, arq))
                for row in range(3):
                    vp, vq = V[row][p], V[row][q]
                    V[row][p] = np.where(on, c * vp - s * vq, vp)
                    V[row][q] = np.where(on, s * vp + c * vq, vq)
    return [a[(0, 0)], a[(1, 1)], a[(2, 2)]], V


def select(lam, V):
    """Ascending order of the three diagonal values by a stable three-element bubble sort on `<` (equal values: the lower column first)
    -> (eig (n, 3), normal (n, 3): V's column of the smallest value)."""
    n = lam[0].shape[0]
    l = [v.copy() for v in lam]
    col = [np.full(n, c, dtype=np.int64) for c in range(3)]
    with np.errstate(invalid="ignore"):
        for i, j in ((0, 1), (1, 2), (0, 1)):
            sw = l[j] < l[i]
            l[i], l[j] = np.where(sw, l[j], l[i]), np.where(sw, l[i], l[j])
            col[i], col[j] = np.where(sw, col[j], col[i]), np.where(sw, col[i], col[j])
    normal = np.stack([np.where(col[0] == 0, V[r][0], np.where(col[0] == 1, V[r][1], V[r][2])) for r in range(3)], axis=1)
    return np.stack(l, axis=1), normal


def dot3(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z, every operation rounded on its own."""
    with np.errstate(all="ignore"):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def sign(normal, x, orient, o):
    """Step 5: orient 0 .. 3 as include/pdgn_hip.h numbers them."""
    normal = normal.copy()
    with np.errstate(all="ignore"):
        if orient == 0:
            mag = np.abs(normal)
            m = np.zeros(normal.shape[0], dtype=np.int64)
            m = np.where(mag[:, 1] > mag[:, 0], 1, m)
            m = np.where(mag[:, 2] > np.take_along_axis(mag, m[:, None], axis=1)[:, 0], 2, m)
            flip = np.take_along_axis(normal, m[:, None], axis=1)[:, 0] < 0
        else:
            o = np.asarray(o, dtype=F).reshape(1, 3)
            w = np.broadcast_to(o, x.shape) if orient == 1 else (o - x) if orient == 2 else (x - o)
            flip = dot3(normal, w) < 0
    normal[flip] = -normal[flip]
    return normal


def estimate_cloud(x, idx, orient=0, o=(0.0, 0.0, 0.0)):
    """One cloud: x (n, 3), idx (n, k) -> (normals (n, 3), eig (n, 3)) as pdgn_estimate_normals stores them."""
    x = np.ascontiguousarray(x, dtype=F)
    idx = np.asarray(idx).astype(np.int64)
    n, k = idx.shape
    assert x.shape == (n, 3) and 1 <= k <= MAX_K and orient in (0, 1, 2, 3)
    outside = ((idx < 0) | (idx >= n)).any(axis=1)
    safe = np.where(outside[:, None], 0, idx)                       # (never dereferenced by the kernel; poisoned below)
    a, _ = covariance(x, safe)
    lam, V = jacobi(a)
    eig, normal = select(lam, V)
    normal = sign(normal, x, orient, o)
    poison = outside | ~np.isfinite(eig).all(axis=1)
    normal[poison] = np.nan
    eig[poison] = np.nan
    return normal, eig


def estimate(x, idx, orient=0, o=(0.0, 0.0, 0.0)):
    """x (b, n, 3), idx (b, n, k) -> (normals (b, n, 3), eig (b, n, 3))."""
    out = [estimate_cloud(xc, ic, orient, o) for xc, ic in zip(np.asarray(x, dtype=F), np.asarray(idx))]
    return np.stack([o_[0] for o_ in out]), np.stack([o_[1] for o_ in out])


def knn_indices(x, k):
    """Ascending (squared distance, index) neighbours of every point among its own cloud, in fp64: what a test on the host uses in place
    of pdgn_knnquery.  x (n, 3) -> (n, k) int32."""
    x64 = np.asarray(x, dtype=np.float64)
    d2 = ((x64[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
    return np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int32)


def same_bits(got, want):
    """Equal bit for bit where `want` is a number, NaN exactly where `want` is NaN."""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---------------------------------------------------------------------------- the lit sheet
def lit_shade(normals, light):
    """c = |n . l| in dot3's order, 0 where !(c >= 0), 1 where c > 1; shade = 48 + (uint32)(207 c), truncating."""
    l = np.broadcast_to(np.asarray(light, dtype=F).reshape(3), np.asarray(normals).shape)
    with np.errstate(all="ignore"):
        c = np.abs(dot3(np.asarray(normals, dtype=F), l))
        c = np.where(c >= 0, c, F(0.0)).astype(F)
        c = np.where(c > 1, F(1.0), c).astype(F)
        return np.uint32(48) + (F(207.0) * c).astype(np.uint32)


def sheet_keys_lit(clouds, normals, view, light, cell, radius):
    """render_mirror.sheet_keys with the key's low byte taken from `lit_shade` in the columns that have normals (a None entry: the
    depth shade, as it was)."""
    B = clouds[0].shape[0]
    keys = np.full((B * cell, len(clouds) * cell), rm.EMPTY, dtype=np.uint32)
    for c, pts in enumerate(clouds):
        iu, iv, key, valid = rm.point_keys(pts, view)
        if normals[c] is not None:
            key = (key & np.uint32(0xFFFFFF00)) | lit_shade(normals[c], light)
        row0 = (np.arange(B, dtype=np.int64) * cell).reshape(B, 1)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if dx * dx + dy * dy > radius * radius:
                    continue
                px, py = iu + dx, iv + dy
                ok = valid & (px >= 0) & (px < cell) & (py >= 0) & (py < cell)
                np.minimum.at(keys, ((row0 + py)[ok], (c * cell + px)[ok]), key[ok])
    return keys


def render_lit(clouds, normals, view, light, cell, radius):
    return rm.resolve(sheet_keys_lit(clouds, normals, view, light, cell, radius))


# ---------------------------------------------------------------------------- the clouds of the accuracy check
def accuracy_clouds(seed=0):
    """The five seeded clouds of the comparison with float64 eigh: name -> (n, 3) fp32."""
    rng = np.random.default_rng(seed)

    def sphere(n):
        v = rng.standard_normal((n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    cube = rng.uniform(-1.0, 1.0, size=(512, 3))
    face = rng.integers(0, 6, size=512)
    cube[np.arange(512), face % 3] = np.where(face < 3, -1.0, 1.0)
    noisy = sphere(512) * (1.0 + 0.05 * rng.standard_normal((512, 1)))
    out = {"sphere512": sphere(512), "cube512": cube, "noisy512": noisy, "sphere64": sphere(64), "blob256": rng.standard_normal((256, 3))}
    return {k: np.ascontiguousarray(v, dtype=F) for k, v in out.items()}


def against_eigh(x, idx):
    """The mirror on one cloud against float64 numpy.linalg.eigh of the float64 covariance of the same neighbourhoods ->
    (max over ALL points of angle [degrees] * (lambda1 - lambda0) / lambda2, max of |eig - eig64| / lambda2)."""
    normal, eig = estimate_cloud(x, idx)
    x64 = np.asarray(x, dtype=np.float64)
    nb = x64[np.asarray(idx, dtype=np.int64)]                       # (n, k, 3)
    d = nb - nb.mean(axis=1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", d, d) / idx.shape[1]
    w, v = np.linalg.eigh(cov)
    ref = v[:, :, 0]
    cosang = np.abs((normal.astype(np.float64) * ref).sum(-1)) / np.linalg.norm(normal.astype(np.float64), axis=1)
    angle = np.degrees(np.arccos(np.clip(cosang, 0.0, 1.0)))
    # arccos loses everything below 1e-8 rad near 1: use the sine (the cross product) for small angles
    cross = np.linalg.norm(np.cross(normal.astype(np.float64), ref), axis=1) / np.linalg.norm(normal.astype(np.float64), axis=1)
    angle = np.where(cosang > 0.5, np.degrees(np.arcsin(np.clip(cross, 0.0, 1.0))), angle)
    gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    return float((angle * gap).max()), float((np.abs(eig.astype(np.float64) - w) / w[:, 2:3]).max())
