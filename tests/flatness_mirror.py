"""numpy restatement of csrc/flatness.hip (include/pdgn_hip.h: pdgn_flatness): the definition of that file's
header block on top of tests/normals_mirror.py's steps 1 to 4 (imported, not copied) and tests/repulsion_mirror.py's reduction.  numpy's
float32 ufuncs round every operation on its own, as the kernel's __fadd_rn / __fsub_rn / __fmul_rn / __fdiv_rn do, so the two agree bit
for bit.  The gather runs in ascending edge order.  Also the same function in fp64 (numpy.linalg.eigh), for the accuracy and finite-difference
checks.  Used by tests/test_flatness_host.py and tests/test_gpu_flatness.py; imports nothing of pdgn_amd."""
import numpy as np

import normals_mirror as nm
import repulsion_mirror as rpm

F = np.float32
H_KEYS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))         # the six entries of a record, in its order


def coef_of(b, n):
    """1 / (b n), computed in fp64 and rounded once."""
    return F(1.0 / (float(b) * float(n)))


def points(x, idx, eps):
    """The per-point launch on one cloud: x (n, 3), idx (n, k) -> {sigma (n), mu (n, 3), h (n, 6), bad (n), degenerate (n), eig (n, 3)}."""
    x = np.ascontiguousarray(x, dtype=F)
    idx = np.asarray(idx).astype(np.int64)
    n, k = idx.shape
    assert x.shape == (n, 3) and 1 <= k <= nm.MAX_K
    eps = F(eps)
    outside = ((idx < 0) | (idx >= n)).any(axis=1)
    safe = np.where((idx < 0) | (idx >= n), 0, idx)                 # (the kernel reads point 0 in place of an index outside the cloud)
    a, mu = nm.covariance(x, safe)
    lam, V = nm.jacobi(a)
    eig, v = nm.select(lam, V)
    inv = F(1.0) / F(k)
    with np.errstate(all="ignore"):
        l0 = eig[:, 0]
        q = ((l0 + eig[:, 1]) + eig[:, 2]) + eps
        bad = outside | ~np.isfinite(eig).all(axis=1)
        deg = ~bad & (~(l0 > 0) | ~(q > 0))
        sigma = l0 / q
        w = (F(2.0) * inv) / q
        h = np.stack([w * ((v[:, a_] * v[:, b_] - sigma) if a_ == b_ else (v[:, a_] * v[:, b_])) for a_, b_ in H_KEYS], axis=1)
    sigma = np.where(deg, F(0.0), np.where(bad, F(np.nan), sigma)).astype(F)
    h = np.where(deg[:, None], F(0.0), np.where(bad[:, None], F(np.nan), h)).astype(F)
    return {"sigma": sigma, "mu": mu.astype(F), "h": h, "bad": bad, "degenerate": deg, "eig": eig}


def gather(x, idx, mu, h, coef):
    """The gather launch on one cloud: for every target j its in-edges e = i k + s in ASCENDING e, from acc = 0; grad = coef * acc.  An
    index outside [0, n) is in no row.  Vectorised over the targets, looped over the position inside the rows."""
    x = np.ascontiguousarray(x, dtype=F)
    idx = np.asarray(idx).astype(np.int64)
    n, k = idx.shape
    tgt = idx.reshape(-1)
    e = np.flatnonzero((tgt >= 0) & (tgt < n))                      # ascending edge ids
    order = np.argsort(tgt[e], kind="stable")                       # rows of the transpose, every row in ascending e
    e, t = e[order], tgt[e][order]
    start = np.searchsorted(t, np.arange(n), side="left")
    rank = np.arange(e.shape[0]) - start[t]
    acc = np.zeros((n, 3), F)
    rows = ((0, 1, 2), (1, 3, 4), (2, 4, 5))                        # (h00 h01 h02), (h01 h11 h12), (h02 h12 h22)
    with np.errstate(all="ignore"):
        for r in range(int(rank.max()) + 1 if rank.size else 0):
            sel = rank == r
            j, i = t[sel], e[sel] // k
            d = x[j] - mu[i]
            hh = h[i]
            for c, (p0, p1, p2) in enumerate(rows):
                acc[j, c] = acc[j, c] + ((hh[:, p0] * d[:, 0] + hh[:, p1] * d[:, 1]) + hh[:, p2] * d[:, 2])
        return (F(coef) * acc).astype(F)


def flatness(x, idx, eps=0.0, coef=None, grad=True):
    """x (b, n, 3), idx (b, n, k) -> {loss, per_cloud (b), sigma (b, n), degenerate (b) int32, grad (b, n, 3) | None, eig (b, n, 3)}: what
    pdgn_flatness stores (coef: 1 / (b n) by default)."""
    x = np.ascontiguousarray(x, dtype=F)
    idx = np.asarray(idx)
    b, n, _ = x.shape
    coef = coef_of(b, n) if coef is None else F(coef)
    per = [points(x[c], idx[c], eps) for c in range(b)]
    sigma = np.stack([p["sigma"] for p in per])
    loss, per_cloud = rpm.reduce(sigma)
    out = {"loss": loss, "per_cloud": per_cloud, "sigma": sigma, "eig": np.stack([p["eig"] for p in per]),
           "degenerate": np.array([p["degenerate"].sum() for p in per], dtype=np.int32), "grad": None}
    if grad:
        out["grad"] = np.stack([gather(x[c], idx[c], per[c]["mu"], per[c]["h"], coef) for c in range(b)])
    return out


# ---------------------------------------------------------------------------- the definition in fp64
def define64(x, idx, eps=0.0):
    """The definition in fp64 on one batch: numpy.linalg.eigh of the fp64 covariance, sigma = l0 / (l0 + l1 + l2 + eps), H = (2 / (k q)) (v v^T -
    sigma I), grad_j = (1 / (b n)) sum over the in-edges of H_i (x_j - mu_i) (np.add.at: no order to speak of) -> {loss, sigma (b, n),
    h (b, n, 6), grad (b, n, 3), eig (b, n, 3)}.  Every index inside [0, n)."""
    x = np.asarray(x, dtype=np.float64)
    idx = np.asarray(idx).astype(np.int64)
    b, n, k = idx.shape
    sigma, h6, grad, eigs = np.empty((b, n)), np.empty((b, n, 6)), np.zeros((b, n, 3)), np.empty((b, n, 3))
    for c in range(b):
        nb = x[c][idx[c]]                                           # (n, k, 3)
        mu = nb.mean(axis=1, keepdims=True)
        d = nb - mu
        cov = np.einsum("nki,nkj->nij", d, d) / k
        w, vec = np.linalg.eigh(cov)
        v = vec[:, :, 0]
        q = w.sum(axis=1) + eps
        live = (w[:, 0] > 0) & (q > 0)
        qs = np.where(live, q, 1.0)
        sg = np.where(live, w[:, 0] / qs, 0.0)
        H = (2.0 / (k * qs))[:, None, None] * (v[:, :, None] * v[:, None, :] - sg[:, None, None] * np.eye(3)) * live[:, None, None]
        sigma[c], eigs[c] = sg, w
        h6[c] = np.stack([H[:, a_, b_] for a_, b_ in H_KEYS], axis=1)
        contrib = np.einsum("nij,nkj->nki", H, d)                   # H_i (x_j - mu_i) for every slot
        np.add.at(grad[c], idx[c].reshape(-1), contrib.reshape(-1, 3))
    return {"loss": float(sigma.mean()), "sigma": sigma, "h": h6, "grad": grad / float(b * n), "eig": eigs}


def against_define64(x, idx, eps):
    """The mirror on one cloud against `define64` -> (max over the points of the relative error of the six h x the relative gap (l1 - l0) / l2,
    the relative L2 error of the whole gradient, the relative error of the loss).  The eigenvector, and so H, is not defined where the two
    smallest eigenvalues meet: the gap weights that away, as tests/test_normals_host.py weights the angle.  H is compared at the points
    that are live on both sides: on an exactly flat neighbourhood (the cube's faces) the definition sets H = 0, where fp64 rounding leaves an
    l0 of the order of 1e-17 and so (2 / (k q)) v v^T -- but there v . (x_j - mu) = 0, the point's contribution H (x_j - mu) to the gradient is
    zero either way, and the gradient's error, taken over ALL points, covers it."""
    got = flatness(x[None], idx[None], eps)
    ref = define64(x[None], idx[None], eps)
    pts = points(x, idx, eps)
    w = ref["eig"][0]
    gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    hn = np.linalg.norm(ref["h"][0], axis=1)
    both = ~pts["degenerate"] & ~pts["bad"] & (hn > 0)
    assert both.any()
    h_err = np.linalg.norm(pts["h"].astype(np.float64) - ref["h"][0], axis=1)[both] / hn[both]
    g_err = np.linalg.norm(got["grad"].astype(np.float64) - ref["grad"]) / np.linalg.norm(ref["grad"])
    l_err = abs(float(got["loss"]) - ref["loss"]) / ref["loss"]
    return float((h_err * gap[both]).max()), float(g_err), float(l_err)


def random_lists(rng, b, n, k, repeats=True):
    """(b, n, k) int32 lists drawn uniformly, with forced repeats (slot 1 repeats slot 0 in every second list) where k > 1."""
    idx = rng.integers(0, n, size=(b, n, k)).astype(np.int32)
    if repeats and k > 1:
        idx[:, ::2, 1] = idx[:, ::2, 0]
    return idx
