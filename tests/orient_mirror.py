"""numpy restatement of csrc/orient.hip (include/pdgn_hip.h: pdgn_orient_normals): the rules of the kernel file's
header block, one Prim round per loop turn, every fp32 operation rounded on its own and every comparison on integers, so that the kernel
and this file agree bit for bit.  Used by tests/test_orient_host.py and tests/test_gpu_orient.py; imports nothing of pdgn_amd."""
import numpy as np

from normals_mirror import dot3, same_bits  # noqa: F401  (same_bits: for the tests that import this module)

F = np.float32
MAX_N = 4096
MAX_K = 64
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
HI = np.uint64(0xFFFFFFFF00000000)
UNTOUCHED = 0xFFFFFFFF
HALF_BITS = int(np.array(0.5, dtype=F).view(np.uint32))
SIGN = np.uint32(0x80000000)


def live_points(x, g):
    """Rule 1: all three coordinates and all three normal components finite."""
    return np.isfinite(x).all(axis=1) & np.isfinite(g).all(axis=1)


def edges(x, g, idx):
    """Rules 2 and 3: the directed slots that survive, as (u, v, wbits) arrays (an undirected edge may appear many times, from either end)."""
    n, k = idx.shape
    live = live_points(x, g)
    u = np.repeat(np.arange(n, dtype=np.int64), k)
    v = np.asarray(idx).astype(np.int64).reshape(-1)
    ok = (v >= 0) & (v < n)
    vs = np.where(ok, v, 0)                                         # (never dereferenced where outside)
    ok &= (vs != u) & live[u] & live[vs]
    u, v = u[ok], vs[ok]
    with np.errstate(all="ignore"):
        w = (F(1.0) - np.abs(dot3(g[u], g[v]))).astype(F)
        w = np.where(w > 0, w, F(0.0)).astype(F)
    return u, v, np.ascontiguousarray(w).view(np.uint32).astype(np.uint64)


def orient_cloud(x, g, idx):
    """One cloud: x (n,3), g (n,3), idx (n,k) -> (o (n,3) fp32, parent (n,) int32, (components, flipped, weak, dead))."""
    x = np.ascontiguousarray(x, dtype=F)
    g = np.ascontiguousarray(g, dtype=F)
    idx = np.asarray(idx)
    n, k = idx.shape
    assert x.shape == (n, 3) and g.shape == (n, 3) and 1 <= n <= MAX_N and 1 <= k <= MAX_K
    live = live_points(x, g)
    eu, ev, ew = edges(x, g, idx)
    # both directions, grouped by the end that joins the tree
    su, sv, sw = np.concatenate([eu, ev]), np.concatenate([ev, eu]), np.concatenate([ew, ew])
    order = np.argsort(su, kind="stable")
    su, sv, sw = su[order], sv[order], sw[order]
    start = np.searchsorted(su, np.arange(n + 1))
    best = np.full(n, NONE, dtype=np.uint64)
    outside = live.copy()
    flip = np.zeros(n, dtype=bool)
    parent = np.full(n, -2, dtype=np.int32)
    ar = np.arange(n, dtype=np.uint64)
    z = x[:, 2]
    components = weak = 0
    for _ in range(int(live.sum())):
        key = np.where(outside, (best & HI) | ar, NONE)
        u = int(np.argmin(key))
        hi = int(best[u] >> np.uint64(32))
        if hi == UNTOUCHED:
            with np.errstate(invalid="ignore"):
                u = int(np.argmax(np.where(outside, z, F(-np.inf))))   # (first of the largest: ties to the lowest index)
            parent[u] = -1
            components += 1
            flip[u] = bool(g[u, 2] < 0)
        else:
            p = int(best[u] & np.uint64(0xFFFFFFFF))
            parent[u] = p
            op = -g[p] if flip[p] else g[p]
            flip[u] = bool(dot3(g[u], op) < 0)
            weak += int(hi > HALF_BITS)
        outside[u] = False
        t, wb = sv[start[u]:start[u + 1]], sw[start[u]:start[u + 1]]
        keep = outside[t]
        np.minimum.at(best, t[keep], (wb[keep] << np.uint64(32)) | np.uint64(u))
    o = g.copy()
    ob = o.view(np.uint32)
    ob[flip] ^= SIGN
    return o, parent, (components, int(flip.sum()), weak, int(n - live.sum()))


def orient(x, g, idx):
    """x (b,n,3), g (b,n,3), idx (b,n,k) -> (o (b,n,3), parent (b,n) int32, stats (b,4) int32)."""
    out = [orient_cloud(xc, gc, ic) for xc, gc, ic in zip(np.asarray(x, dtype=F), np.asarray(g, dtype=F), np.asarray(idx))]
    return (np.stack([r[0] for r in out]), np.stack([r[1] for r in out]), np.array([r[2] for r in out], dtype=np.int32).reshape(-1, 4))


def torus(n, seed, R=1.0, r=0.4):
    """n points uniform by area on the torus of radii R, r, by rejection -> (points (n,3) fp32, analytic outward normals (n,3) fp64)."""
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    while len(pts) < n:
        u = rng.uniform(0.0, 2.0 * np.pi)
        v = rng.uniform(0.0, 2.0 * np.pi)
        w = rng.uniform(0.0, 1.0)
        if w <= (R + r * np.cos(v)) / (R + r):
            pts.append(((R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)))
            nrm.append((np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)))
    return np.asarray(pts, dtype=F), np.asarray(nrm, dtype=np.float64)
