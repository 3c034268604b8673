"""The exact cases of tests/test_gpu_localpair.py, built once: inputs from hashweights (dyadic lattices, no RNG), expected results from
tests/localpair_mirror.py, every one passed through the mirror's `assert_exact` before it is handed out.  Shared by the host test
(tests/test_localpair_mirror_host.py: the guard accepts every case, wherever the suite runs), the GPU module and its child process."""
import functools

import numpy as np

import localpair_mirror as lm
from hashweights import lattice_points, unit_hash

# ---------------------------------------------------------------------------- Chamfer
# (kind, bits, b, m, n, d).  kinds: "lattice" both clouds from lattice_points; "shift40" the same translated by +40 in every coordinate;
# "same_y" every point of y identical; "x_is_y" the two clouds are one; "tie5_1030" / "tie1023_1024" one candidate outside the cube
# planted at those two indices of y and queries 64..127 of x on it or one lattice step further out.
CHAMFER_FORWARD = [
    ("lattice", 3, 2, 300, 1500, 3),        # far more candidates than queries one way, blocks that exit early the other way
    ("lattice", 3, 2, 1366, 1400, 9),       # two candidate tiles both ways, D = 9
    ("lattice", 2, 1, 769, 40, 16),         # generic instance at CH_MAXD
    ("lattice", 4, 1, 40, 33, 1),           # generic instance at d = 1
    ("lattice", 3, 1, 257, 1025, 2),        # one past the block, one past the tile
    ("lattice", 3, 2, 255, 1023, 3),        # one short of both
    ("lattice", 2, 1, 256, 1024, 9),        # exactly both
    ("lattice", 4, 1, 1, 2049, 3),          # m = 1, three tiles
    ("lattice", 4, 1, 2049, 1, 3),          # n = 1
    ("lattice", 3, 3, 1, 1, 9),
    ("tie5_1030", 3, 1, 300, 1100, 3),      # a tie across two CH_TILE tiles
    ("tie1023_1024", 3, 1, 300, 1100, 3),   # ... across the tile's very edge
    ("same_y", 2, 1, 300, 70, 3),
    ("x_is_y", 3, 2, 700, 700, 3),
    ("shift40", 3, 1, 300, 1500, 3),
]
# shapes on both sides of CHL_MAXF = 12288 floats of one cloud's gradient: the LDS kernel / memset + the global-atomic kernel
CHAMFER_GRAD = [
    ("lattice", 4, 2, 4096, 300, 3), ("lattice", 4, 2, 4097, 300, 3),
    ("lattice", 3, 1, 1365, 1365, 9), ("lattice", 3, 2, 1366, 1400, 9),
    ("lattice", 2, 1, 768, 40, 16), ("lattice", 2, 1, 769, 40, 16),
    ("lattice", 4, 1, 200, 4097, 3),        # only the second cloud over the limit
    # one hot target: every x chooses y[0], every y the same x -- thousands of atomics onto one row, through both kernels
    ("same_y", 2, 1, 4096, 300, 3), ("same_y", 2, 1, 4097, 300, 3),
    ("lattice", 2, 1, 4096, 1, 3), ("lattice", 2, 1, 4097, 1, 3),
]
CHAMFER_OVER_LIMIT = [c for c in CHAMFER_GRAD if max(c[3], c[4]) * c[5] > 12288]
WORKER_CASE = ("lattice", 3, 2, 256, 128, 9)
UNIFORM_G, UNIFORM_SCALE = 3.0, 0.25
# pair lists over clouds of unequal point counts: repeats, a reversed run, clouds nobody names (4 of the first set; 2 and 5 of the second)
PAIR_SHAPES = [(300, 100), (100, 250)]
PAIR_SETS = (5, 6)
PAIR_IA = [3, 3, 2, 1, 0, 0, 3, 1]
PAIR_IB = [0, 4, 4, 3, 1, 0, 0, 3]
PAIR_BITS = 3


def quarter_steps(key, shape):
    """Multiples of 1/4 in [-2, 2], a function of the key alone."""
    return (np.rint(unit_hash(key, int(np.prod(shape))).astype(np.float64) * 8.0) / 4.0).astype(np.float32).reshape(shape)


def chamfer_inputs(kind, bits, b, m, n, d):
    key = "localpair/%s/%d/%d/%d/%d/%d" % (kind, bits, b, m, n, d)
    x = lattice_points(key + "/x", (b, m, d), bits)
    y = lattice_points(key + "/y", (b, n, d), bits)
    if kind == "shift40":
        x, y = x + np.float32(40.0), y + np.float32(40.0)
    elif kind == "same_y":
        y = np.ascontiguousarray(np.broadcast_to(y[:, :1], y.shape))
    elif kind == "x_is_y":
        assert m == n
        y = x.copy()
    elif kind.startswith("tie"):
        i0, i1 = (int(v) for v in kind[3:].split("_"))
        p = np.array([1.25, -1.5, 1.0][:d], np.float32)                  # outside [-1, 1)^d: no other candidate is as near
        step = np.zeros(d, np.float32)
        step[0] = 2.0 ** -bits
        y[:, i0], y[:, i1] = p, p
        x[:, 64:96], x[:, 96:128] = p, p + step
    else:
        assert kind == "lattice", kind
    return x, y


@functools.lru_cache(maxsize=None)
def chamfer_reference(case):
    """Inputs (float32), upstream gradients and the mirror's results (float64; argmins int32) of one case, every result guarded."""
    kind, bits, b, m, n, d = case
    x, y = chamfer_inputs(*case)
    q = 2.0 ** -bits
    lm.assert_exact(x, q)
    lm.assert_exact(y, q)
    minx, argx, miny, argy = lm.chamfer(x, y)
    bound = lm.gram_abs(x, y)                                            # covers every entry of P, not the minima alone
    lm.assert_exact(minx, q * q, bound)
    lm.assert_exact(miny, q * q, bound)
    key = "localpair/g/%s/%d/%d/%d/%d/%d" % case
    gminx, gminy = quarter_steps(key + "/x", (b, m)), quarter_steps(key + "/y", (b, n))
    gx, gy = lm.chamfer_grad(x, y, argx, argy, gminx, gminy)
    ux, uy = lm.chamfer_grad_uniform(x, y, argx, argy, UNIFORM_G, UNIFORM_SCALE)
    qg = 2.0 ** -(bits + 2)
    for got, bnd in (((gx, gy), lm.chamfer_grad_abs(x, y, argx, argy, gminx, gminy)),
                     ((ux, uy), lm.chamfer_grad_uniform_abs(x, y, argx, argy, UNIFORM_G, UNIFORM_SCALE))):
        lm.assert_exact(got[0], qg, bnd[0])
        lm.assert_exact(got[1], qg, bnd[1])
    out = dict(x=x, y=y, minx=minx, argx=argx, miny=miny, argy=argy, gminx=gminx, gminy=gminy, gx=gx, gy=gy, ux=ux, uy=uy)
    for v in out.values():
        v.setflags(write=False)
    return out


def tied_rows(x, y):
    """Fraction of x's points whose minimum of P is attained at two or more DISTINCT candidate indices."""
    P = lm.gram(x, y)
    return float(((P == P.min(2, keepdims=True)).sum(2) > 1).mean())


@functools.lru_cache(maxsize=None)
def pair_inputs(which):
    n, m = PAIR_SHAPES[which]
    a = lattice_points("localpair/pairs/%d/a" % which, (PAIR_SETS[0], n, 3), PAIR_BITS)
    b = lattice_points("localpair/pairs/%d/b" % which, (PAIR_SETS[1], m, 3), PAIR_BITS)
    return a, b, np.array(PAIR_IA, np.int32), np.array(PAIR_IB, np.int32)


# ---------------------------------------------------------------------------- local statistics
STATS_BITS = 3
# (b, n, m, K), K a power of two so that 1 / K is dyadic.  n * 3 <= 6144: points and slab in LDS; <= 8192: the slab alone; else global atomics
STATS_EXACT = [
    (2, 2048, 300, 16), (2, 2049, 300, 16),      # LP_PTS_FLOATS: the last n with staged points, the first without
    (1, 2730, 600, 8), (1, 2731, 600, 8),        # LP_LDS_FLOATS: the last n with the slab, the first on global atomics
    (1, 5000, 64, 4),
    (1025, 8, 5, 2),                             # 1024 / b == 0: qsplit clamped up to 1
    (1, 700, 601, 4),                            # qsplit = 3, per = 201 does not divide m
    (3, 40, 1, 1),                               # K = 1: cov == 0, the gradient is dmu alone
]
SAME_POINT = 5                                   # query 1 (where there is one) names this point K times


def stats_inputs(b, n, m, K):
    key = "localpair/stats/%d/%d/%d/%d" % (b, n, m, K)
    xyz = lattice_points(key + "/xyz", (b, n, 3), STATS_BITS)
    u = (unit_hash(key + "/idx", b * m * K).astype(np.float64) + 1.0) / 2.0
    idx = np.minimum(np.floor(u * n), n - 1).astype(np.int32).reshape(b, m, K)
    if m > 1:
        idx[:, 1, :] = SAME_POINT                # duplicate neighbours inside one query
    idx[:, ::2, 0] = 0                           # a hot destination: point 0 in every 2nd query
    idx[idx == n - 1] = n - 2                    # a point no query references
    return xyz, idx, quarter_steps(key + "/dmu", (b, m, 3)), quarter_steps(key + "/dcov", (b, m, 9))


@functools.lru_cache(maxsize=None)
def stats_reference(case):
    b, n, m, K = case
    xyz, idx, dmu, dcov = stats_inputs(*case)
    lg = int(np.log2(K))
    assert 2 ** lg == K and idx.min() >= 0 and idx.max() < n - 1
    lm.assert_exact(xyz, 2.0 ** -STATS_BITS)
    mu, cov = lm.local_stats(xyz, idx)
    amu, acov = lm.local_stats_abs(xyz, idx)
    lm.assert_exact(mu, 2.0 ** -(STATS_BITS + lg), amu)
    lm.assert_exact(cov, 2.0 ** -(2 * STATS_BITS + 3 * lg), acov)
    dxyz = lm.local_stats_grad(xyz, idx, dmu, dcov)
    lm.assert_exact(dxyz, 2.0 ** -(STATS_BITS + 2 + 2 * lg), lm.local_stats_grad_abs(xyz, idx, dmu, dcov))
    out = dict(xyz=xyz, idx=idx, dmu=dmu, dcov=dcov, mu=mu, cov=cov, dxyz=dxyz)
    for v in out.values():
        v.setflags(write=False)
    return out
