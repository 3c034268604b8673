"""The cases of tests/test_gpu_bn.py, built once: inputs from hashweights (dyadic lattices, no RNG), expected results from
tests/bn_mirror.py, every exact one passed through the mirror's `assert_exact` before it is handed out.  Shared by the host test
(tests/test_bn_mirror_host.py) and the GPU module (through tests/bn_worker.py).

Every case names the regime it is meant to reach; `check_table` asserts that through the mirror's launch rules.  The shapes are the
smallest that reach a regime (csrc/bn_geom.h, fb_slices and mp_geometry in csrc/bnact.hip).

The apply and backward entry points take `stats` as an argument: their cases pass HAND-MADE statistics (`hand_stats`: powers of two
and small multiples of them, negative scales, a scale of exactly zero), so that xhat is dyadic and every sum exact.  Every such case
holds z == +0 (recipe 0 at x = 0.5) and z == -0 (recipe 1 at x = 0) in its first and last row.

LeakyReLU's slope 0.01f is no dyadic number: a float32 sum that mixes dy*0.01f with other terms depends on its order.  The LeakyReLU
backward cases therefore carry dy == 0 wherever z <= 0, except in the channels of recipes 0 (z == 0) and 5 (every z < 0), whose only
non-zero dy are the 2.0 of the first and the last row: one addition of two equal terms."""
import collections
import functools

import numpy as np

import bn_mirror as bm
from hashweights import lattice_points, unit_hash
from localpair_cases import quarter_steps

F32, F64 = np.float32, np.float64
EPS, MOMENTUM = 1e-5, 0.1
BITS = 3                                                            # x on a 1/8 lattice in [-1, 1)

# (scale, shift, mean, invstd) by (channel + rot) % 8
RECIPES = ((2.0, -1.0, 0.25, 2.0),          # 0: z == +0 at x = 0.5
           (-2.0, -0.0, 0.0, 1.0),          # 1: negative scale; z == -0 at x = +0
           (1.0, 0.25, -0.5, 0.5),
           (-0.5, 0.5, 0.125, 4.0),
           (0.0, -1.0, 0.0, 1.0),           # 4: scale exactly 0: every z == -1
           (1.0, -8.0, 0.0, 1.0),           # 5: every z < 0 (ReLU's plateau)
           (2.0 ** -30, 1.0, 0.25, 1.0),    # 6: different x, the same activated bits (z == 1 for every x of the lattice)
           (-1.0, -0.25, 0.0, 2.0))
# gamma, beta by channel % 8 for the statistics that a device computes itself: the same plants for the one-pass max-pool
GAMMAS = (1.0, -1.0, 0.5, -2.0, 0.0, 1.0, 2.0 ** -30, -0.75)
BETAS = (0.25, 0.0, -0.5, 0.125, -1.0, -100.0, 1.0, 0.5)

Geo = collections.namedtuple("Geo", "name R C act mul training inter rot reach")
Blk = collections.namedtuple("Blk", "name C nparts block_rows last spare want")
Raw = collections.namedtuple("Raw", "name R C")
Ev = collections.namedtuple("Ev", "name C full")
MP = collections.namedtuple("MP", "name b n c act rot")


def _reach(**kw):
    return tuple(sorted(kw.items()))


GEOMETRY = [
    Geo("one_row", 1, 4, 2, False, True, 0, 0, _reach(cgb=1, gy=1)),                 # 255 idle row lanes, the R == 1 variance branch
    Geo("last_block_one_row", 4097, 4, 1, False, True, 0, 0, _reach(cgb=1, gy=2, last=1)),
    Geo("two_blocks", 1025, 16, 0, True, False, 0, 0, _reach(cgb=4, gy=2)),
    Geo("idle_columns_6_of_8", 777, 24, 2, False, True, 111, 0, _reach(cgb=8, gy=2, idle=2)),
    Geo("idle_columns_10_of_16", 300, 40, 1, True, True, 0, 0, _reach(cgb=16, gy=2, idle=6)),
    Geo("rl1_three_blocks", 33, 1024, 2, False, True, 0, 0, _reach(cgb=256, gy=3, rl=1)),
    Geo("four_blocks_of_16", 64, 1024, 1, False, False, 16, 0, _reach(cgb=256, gy=4, last=16)),
    Geo("gx2", 100, 1028, 0, False, True, 0, 0, _reach(cgb=256, gx=2, idle=255)),
    Geo("gx3", 70, 2052, 1, True, True, 0, 0, _reach(cgb=256, gx=3)),
    Geo("gy257", 4097, 1024, 2, False, True, 0, 0, _reach(cgb=256, gy=257)),
]
# per cgb (every power of two from 1 to 256; C = 24 is cgb = 8 with two idle column lanes), single blocks of 1, rl, 3 rl + 1, 4 rl and
# 4 rl + 1 rows: the four-row unrolled loops and their remainders
SWEEP = ((4, 256), (8, 128), (16, 64), (24, 32), (64, 16), (128, 8), (256, 4), (512, 2), (1024, 1))


def sweep_rows(rl):
    return sorted({1, rl, 3 * rl + 1, 4 * rl, 4 * rl + 1})


for _C, _rl in SWEEP:
    for _i, _R in enumerate(sweep_rows(_rl)):
        _act = (_i + _C // 8) % 3
        GEOMETRY.append(Geo("c%d_rows%d" % (_C, _R), _R, _C, _act, _C == 24 and _R % 2 == 1 and _act != 2, _R % 2 == 1,
                            _R // 4 if (_C == 256 and _R % 4 == 0) else 0, (0, 6, 7, 0, 6)[_i] if _C == 4 else _i + 3,
                            _reach(gy=1, rl=_rl)))                               # (four channels: a rotation that keeps recipes 0 and 1)
# (rows, c, interleave_n, with mul): refused by pdgn_bn_act_forward and pdgn_bn_act_backward
APPLY_REFUSED = [(10, 8, 3, False), (12, 8, 3, True), (12, 8, -1, False), (12, 6, 0, False), (0, 8, 0, False), (12, 8, 0, "act3")]

BLOCKS = [
    Blk("one_block", 16, 1, 32, 32, 0, "one_launch"),
    Blk("n63_rows_of_one", 16, 63, 1, 1, 0, "one_launch"),
    Blk("n64", 16, 64, 32, 1, 0, "one_launch"),
    Blk("n65", 16, 65, 32, 31, 0, "one_launch"),
    Blk("n65_spare", 16, 65, 32, 32, 25, "one_launch"),                            # 25 NaN rows behind the 40 that hold rows
    Blk("n257", 16, 257, 128, 127, 0, "one_launch"),
    Blk("n511", 16, 511, 256, 255, 0, "one_launch"),
    Blk("c64_n1400", 64, 1400, 32, 32, 0, "one_launch"),
    Blk("c1028_n512", 1028, 512, 1, 1, 0, "one_launch"),                           # C / 4 >= 512: no slice count >= 2
    Blk("slice4_4x128", 16, 512, 128, 1, 0, "slice4"),
    Blk("slice4_spare", 16, 512, 32, 31, 212, "slice4"),                           # slice 2 holds 44 rows, slice 3 only spare ones
    Blk("slice4_8", 24, 1024, 32, 31, 0, "slice4"),
    Blk("slice4_4x150", 40, 600, 32, 32, 0, "slice4"),
    Blk("slice4_32", 8, 8192, 32, 1, 0, "slice4"),
    Blk("slice64_21", 64, 1401, 32, 32, 0, "slice64"),                             # 21 slices of 67, the last holds 61
    Blk("slice64_clamped", 128, 8193, 1, 1, 0, "slice64"),                         # 128 slices of 65, the last holds none
    Blk("slice64_spare", 128, 8193, 1, 1, 4193, "slice64"),                        # slices 62.. hold only spare rows
    Blk("slice64_br256", 64, 1401, 256, 255, 1301, "slice64"),                     # 100 blocks of 256 rows, 1301 spare
]
# the rounded tier: sums that no lattice makes order-independent (block_rows, or the last block, not a power of two)
ROUNDED = [
    Blk("br160_left13", 16, 64, 160, 13, 0, "one_launch"),
    Blk("br250_left13", 24, 1024, 250, 13, 0, "slice4"),
    Blk("br160_slice64", 64, 1401, 160, 13, 1337, "slice64"),
]
# (rows, c, nparts, block_rows)
BLOCKS_REFUSED = [(101, 16, 10, 10), (100, 18, 10, 10), (100, 0, 10, 10), (100, 16, 0, 10), (100, 16, 10, 0), (0, 16, 10, 10)]

RAW = [Raw("gy2", 1025, 16), Raw("gy3", 33, 1024), Raw("gy257", 4097, 1024)]
EVAL = [Ev("c%d_%s" % (c, "full" if full else "bare"), c, full) for c in (1, 5, 256, 257) for full in (True, False)]

MAXPOOL = [
    MP("n1", 1, 1, 4, 2, 0), MP("n1_b17", 17, 1, 24, 1, 3),
    MP("n15", 17, 15, 24, 2, 0), MP("n16", 33, 16, 256, 1, 0), MP("n17_gx2", 1, 17, 260, 2, 0), MP("n33", 17, 33, 4, 1, 4),
    MP("n300_idle", 33, 300, 24, 2, 0), MP("n300_cgb64", 1, 300, 256, 0, 0), MP("n16_gx2", 17, 16, 260, 1, 0),
    MP("n33_c4_rot", 33, 33, 4, 2, 1), MP("n300_c4", 1, 300, 4, 1, 5),
]
MAXPOOL_REFUSED = [(0, 8, 8, 2), (2, 0, 8, 2), (2, 8, 6, 2), (2, 8, 0, 2), (2, 8, 8, 3), (65536, 1, 4, 2)]


def by_name(table, name):
    (case,) = [c for c in table if c.name == name]
    return case


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---------------------------------------------------------------------------- inputs
def hand_stats(C, rot=0):
    r = np.array([RECIPES[(c + rot) % 8] for c in range(C)], F32)
    return np.concatenate([r[:, 0], r[:, 1], r[:, 2], r[:, 3]]).astype(F32)


def params(key, C, full=True):
    """gamma, beta (the plants of GAMMAS / BETAS), pre_bias, running_mean, running_var."""
    if not full:
        return dict(gamma=None, beta=None, pre_bias=None)
    return dict(gamma=np.array([GAMMAS[c % 8] for c in range(C)], F32), beta=np.array([BETAS[c % 8] for c in range(C)], F32),
                pre_bias=lattice_points(key + "/pre_bias", (C,), 4))


def running(key, C):
    return dict(rm=lattice_points(key + "/rm", (C,), 4), rv=(1.0 + lattice_points(key + "/rv", (C,), 4) / 2).astype(F32))


def matrix(key, R, C, rot=0):
    """x (R, C) on the 1/8 lattice, with the activation kinks planted in the first and the last row."""
    X = lattice_points(key + "/x", (R, C), BITS) + F32(0.0)
    for c in range(C):
        r = (c + rot) % 8
        if r in (0, 5):
            X[0, c] = X[R - 1, c] = 0.5
        elif r == 1:
            X[0, c] = X[R - 1, c] = 0.0
    return X


def block_matrix(case, key, exact=True):
    """The host matrix behind a block-partial case (it never goes to a device).  A short last block whose row count is no power of
    two holds pv + last/8 * {-1, 0, 1}: its sums divide by `last` exactly."""
    used = case.nparts - case.spare
    R = (used - 1) * case.block_rows + case.last
    if not exact:
        u = unit_hash(key + "/x", R * case.C).reshape(R, case.C).astype(F64)
        return (u + 3.0 * unit_hash(key + "/mean", case.C).astype(F64)).astype(F32), R        # |mean| <= 3, std = 0.577: |mean| <= 8 std
    X = lattice_points(key + "/x", (R, case.C), BITS)
    if case.last & (case.last - 1):
        start = (used - 1) * case.block_rows
        k = np.rint(X[start:].astype(F64) * 1.4)                                   # -1, 0, 1
        k[0] = 0
        X[start:] = (X[start].astype(F64) + k * case.last / 8.0).astype(F32)
    return X, R


# ---------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def geometry_reference(case):
    """x, the own-pass statistics (exact), hand-made stats, y, dy, mul and the backward's results."""
    key = "bn/geo/" + case.name
    R, C = case.R, case.C
    g = bm.Guard()
    X = matrix(key, R, C, case.rot)
    p, run = params(key, C), running(key, C)
    part = bm.partials_own_pivot(X, g)
    fin = bm.finalize_sums(part, R, X[0], EPS, MOMENTUM, guard=g, **p, **run)
    stats = hand_stats(C, case.rot)
    mul = (np.rint(unit_hash(key + "/mul", R * C).astype(F64) * 4.0) / 2.0).astype(F32).reshape(R, C) + F32(0.0) if case.mul else None
    y, z = bm.apply(X, stats, case.act, mul, case.inter)
    dy = quarter_steps(key + "/dy", (R, C)) + F32(0.0)
    if case.act == bm.ACT_LEAKY:
        dy[z <= 0] = 0.0
        for c in range(C):
            if (c + case.rot) % 8 in (0, 5):
                dy[:, c] = 0.0
                dy[0, c] = dy[R - 1, c] = 2.0
    dy_dev = bm.interleave(dy, case.inter) if case.inter else dy
    bwd = bm.backward(X, dy_dev, stats, case.act, case.training, mul, case.inter, guard=g)
    bm.assert_exact(g)
    return _freeze(dict(X=X, part=part, fin=fin["stats"], rm=fin["running_mean"], rv=fin["running_var"], p=p, run=run, stats=stats,
                        mul=mul, y=y, z=z, dy=dy_dev, bsums=bwd["bsums"], dx=bwd["dx"], dmul=bwd["dmul"], coef=bwd["coef"]))


@functools.lru_cache(maxsize=None)
def blocks_reference(case):
    key = "bn/blk/" + case.name
    g = bm.Guard()
    X, R = block_matrix(case, key)
    part = bm.partials_blocks(X, case.block_rows, case.nparts, guard=g)
    p, run = params(key, case.C), running(key, case.C)
    slices = bm.fb_slices(case.C, case.nparts)
    fin = bm.finalize_blocks(part, R, case.block_rows, slices, EPS, MOMENTUM, guard=g, **p, **run)
    bm.assert_exact(g)
    return _freeze(dict(R=R, part=part, stats=fin["stats"], rm=fin["running_mean"], rv=fin["running_var"], p=p, run=run, slices=slices,
                        mean64=fin["mean64"], var64=fin["var64"], X=X))


@functools.lru_cache(maxsize=None)
def rounded_reference(case):
    """float32 partials of a matrix that is on no lattice, and the exact (rational) statistics of those partials."""
    key = "bn/rounded/" + case.name
    X, R = block_matrix(case, key, exact=False)
    part = bm.partials_blocks(X, case.block_rows, case.nparts)
    means, vars_, unb, inv = bm.rational_blocks(part, R, case.block_rows, EPS)
    std = np.sqrt(np.array([float(v) for v in vars_]))
    assert (np.abs(np.array([float(m) for m in means])) <= 8 * std).all()
    p = params(key, case.C)
    p["pre_bias"] = None
    return dict(R=R, part=part, mean=means, var=vars_, unbiased=unb, invstd=inv, p=p)


@functools.lru_cache(maxsize=None)
def raw_reference(case):
    key = "bn/raw/" + case.name
    g = bm.Guard()
    X = matrix(key, case.R, case.C)
    part = bm.partials_own_pivot(X, g, raw=True)
    p, run = params(key, case.C), running(key, case.C)
    fin = bm.finalize_sums(part, case.R, None, EPS, MOMENTUM, guard=g, **p, **run)
    bm.assert_exact(g)
    return _freeze(dict(X=X, part=part.astype(F32), stats=fin["stats"], rm=fin["running_mean"], rv=fin["running_var"], p=p, run=run,
                        mean64=fin["mean64"], var64=fin["var64"]))


@functools.lru_cache(maxsize=None)
def eval_reference(case):
    key = "bn/eval/" + case.name
    return _freeze(dict(p=params(key, case.C, case.full), run=running(key, case.C)))


def maxpool_matrix(case, key):
    """x (b*n, c) on the lattice (16 values: ties in every channel once n > 16), with +-1.5 planted twice per sample and channel:
    in two row lanes of the first split, in two different splits, or in the first and the last row."""
    b, n, c = case.b, case.n, case.c
    X = (lattice_points(key + "/x", (b, n, c), BITS) + F32(0.0))
    if n >= 6:
        pairs = ((0, n - 1), (1, 2), (n // 3, 2 * n // 3))
        for ch in range(c):
            i, j = pairs[ch % 3]
            X[:, i, ch] = X[:, j, ch] = 1.5
            X[:, (i + 2) % n, ch] = X[:, (j + 2) % n, ch] = -1.5
    return X.reshape(b * n, c)


@functools.lru_cache(maxsize=None)
def maxpool_reference(case):
    """Both forms and the adjoint: the one-pass form's own statistics (exact), the apply form with those and with hand-made ones."""
    key = "bn/mp/" + case.name
    b, n, c = case.b, case.n, case.c
    g = bm.Guard()
    X = maxpool_matrix(case, key)
    p, run = params(key, c), running(key, c)
    fin = bm.maxpool_stats(X, b, n, guard=g, eps=EPS, momentum=MOMENTUM, **p, **run)
    own = fin["stats"]
    pick_max, pick_arg = bm.maxpool_pick(X, own, case.act, b, n)
    own_max, own_arg, own_unique = bm.maxpool_apply(X, own, case.act, b, n)
    hand = hand_stats(c, case.rot)
    hand_max, hand_arg, hand_unique = bm.maxpool_apply(X, hand, case.act, b, n)
    hand_pick_max, hand_pick_arg = bm.maxpool_pick(X, hand, case.act, b, n)
    dout = quarter_steps(key + "/dout", (b, c)) + F32(0.0)
    # the adjoint takes either form's yarg: both are run
    bwd = {(t, which): bm.maxpool_backward(X, dout, arg, hand, case.act, t, b, n, guard=g)
           for t in (0, 1) for which, arg in (("apply", hand_arg), ("pick", hand_pick_arg))}
    bm.assert_exact(g)

    def z_at(stats, arg):                                         # z of the row a form names: ReLU's zero is sign-free only where it is -0
        sc, sh, _, _ = bm.split_stats(stats)
        return bm.fma32(np.take_along_axis(X.reshape(b, n, c), arg.astype(np.int64)[:, None, :], 1)[:, 0], sc, sh)

    return _freeze(dict(X=X, p=p, run=run, own=own, rm=fin["running_mean"], rv=fin["running_var"], pick_max=pick_max, pick_arg=pick_arg,
                        pick_z=z_at(own, pick_arg), own_z=z_at(own, own_arg), hand_z=z_at(hand, hand_arg),
                        own_max=own_max, own_arg=own_arg, own_unique=own_unique, hand=hand, hand_max=hand_max, hand_arg=hand_arg,
                        hand_unique=hand_unique, hand_pick_max=hand_pick_max, hand_pick_arg=hand_pick_arg, dout=dout, bwd=bwd))


# ---------------------------------------------------------------------------- end to end: statistics from a producer's epilogue
THIN = dict(m=5 * 256 + 64, n=8, k=3, act=1)                       # rows no multiple of the block; the last block a power of two
GATHER = "geom6_small"                                             # the case of tests/wgs_cases.py whose epilogue writes raw partial rows


def thin_block_rows():
    return int(bm.wm._one(bm.wm._read("thin.hip"), r"#define THIN_ROWS (\d+) ", "rows per partial row of pdgn_thin_nt"))


@functools.lru_cache(maxsize=None)
def thin_reference():
    """x (m, 3) and W (n, 3) on a 1/4 lattice: y = x W^T, its block-shifted partials as pdgn_thin_nt's epilogue leaves them, the
    statistics pdgn_bn_stats_from_gemm_partials makes of them and the activated output."""
    key, t = "bn/e2e/thin", THIN
    g = bm.Guard()
    x, w = lattice_points(key + "/x", (t["m"], t["k"]), 2), lattice_points(key + "/w", (t["n"], t["k"]), 2)
    y = x.astype(F64) @ w.astype(F64).T
    br = thin_block_rows()
    nparts = bm.cdiv(t["m"], br)
    part = bm.partials_blocks(y, br, nparts, guard=g)
    p, run = params(key, t["n"]), running(key, t["n"])
    p["pre_bias"] = None
    fin = bm.finalize_blocks(part, t["m"], br, bm.fb_slices(t["n"], nparts), EPS, MOMENTUM, guard=g, **p, **run)
    bm.assert_exact(g)
    out, z = bm.apply(y.astype(F32), fin["stats"], t["act"])
    return dict(x=x, w=w, y=y, part=part, block_rows=br, p=p, run=run, rm=fin["running_mean"], rv=fin["running_var"], out=out, z=z)


@functools.lru_cache(maxsize=None)
def gather_reference():
    """The gather-sum case's exact output as (b*n*P, C) rows, the raw partial rows of its epilogue finalised, and the activated output."""
    import wgs_cases as wc
    case = wc.by_name(wc.STATS, GATHER)
    ref = wc.forward_reference(case)
    C = case.spec[2]
    rows = ref["out"].reshape(-1, C)
    g = bm.Guard()
    part = bm.partials_own_pivot(rows, g, raw=True)
    p, run = params("bn/e2e/gather", C), running("bn/e2e/gather", C)
    p["pre_bias"] = None
    fin = bm.finalize_sums(part, rows.shape[0], None, EPS, MOMENTUM, guard=g, **p, **run)
    bm.assert_exact(g)
    out, z = bm.apply(rows.astype(F32), fin["stats"], bm.ACT_LEAKY)
    return dict(case=case, wgs=ref, p=p, run=run, rm=fin["running_mean"], rv=fin["running_var"], out=out, z=z)


# ---------------------------------------------------------------------------- the table against the launchers' rules
def check_table():
    """Every case reaches what its line names."""
    for c in GEOMETRY:
        cgb, gx, gy, rpb = bm.cl_geometry(c.R, c.C)
        cg = c.C // 4
        got = dict(cgb=cgb, gx=gx, gy=gy, rl=256 // cgb, last=c.R - (gy - 1) * rpb, idle=gx * cgb - cg)
        assert all(got[k] == v for k, v in c.reach), (c.name, got)
        assert not c.inter or (c.R % c.inter == 0 and not c.mul), c.name
    single = {}                                                   # cgb -> the row counts of its single-block cases
    for c in GEOMETRY:
        cgb, gx, gy, rpb = bm.cl_geometry(c.R, c.C)
        if gx == 1 and gy == 1:
            single.setdefault(cgb, set()).add(c.R)
    assert sorted(single) == [1 << i for i in range(9)], sorted(single)
    for cgb, rows in single.items():
        assert rows >= set(sweep_rows(256 // cgb)), (cgb, sorted(rows))
    assert {c.act for c in GEOMETRY} == {0, 1, 2} and {c.mul for c in GEOMETRY} == {True, False}
    assert {c.training for c in GEOMETRY} == {True, False} and any(c.inter for c in GEOMETRY)
    assert {(c.act, c.training) for c in GEOMETRY} >= {(a, t) for a in (0, 1, 2) for t in (True, False)}
    for rows, c, inter, mul in APPLY_REFUSED:
        assert rows < 1 or c < 4 or c % 4 or inter < 0 or (inter > 0 and (rows % inter or mul)) or mul == "act3"
    for c in BLOCKS + ROUNDED:
        used = c.nparts - c.spare
        R = (used - 1) * c.block_rows + c.last
        assert 1 <= c.last <= c.block_rows and bm.cdiv(R, c.block_rows) == used
        assert bm.regime(R, c.C, c.nparts, c.block_rows) == c.want, c
        assert bm.regime(R, c.C, c.nparts, c.block_rows, scratch=False) == "one_launch"
    counts = {c.name: bm.slice_counts(c.nparts, bm.fb_slices(c.C, c.nparts), c.nparts - c.spare) for c in BLOCKS if c.want != "one_launch"}
    assert counts["slice4_4x128"] == [128] * 4 and counts["slice4_4x150"] == [150] * 4 and len(counts["slice4_8"]) == 8
    assert len(counts["slice4_32"]) == 32 and counts["slice4_spare"] == [128, 128, 44, 0]
    assert counts["slice64_21"] == [67] * 20 + [61] and counts["slice64_clamped"] == [65] * 126 + [3, 0]
    assert counts["slice64_spare"][61:63] == [35, 0] and not any(counts["slice64_spare"][62:])
    assert {c.nparts for c in BLOCKS if c.C == 16 and c.want == "one_launch"} >= {1, 63, 64, 65, 257, 511}
    assert {c.block_rows for c in BLOCKS} == {1, 32, 128, 256}
    assert {(c.last == 1, c.last == c.block_rows - 1, c.last == c.block_rows) for c in BLOCKS if c.block_rows > 2} == \
        {(True, False, False), (False, True, False), (False, False, True)}
    for rows, c, nparts, br in BLOCKS_REFUSED:
        assert bm.regime(rows, c, nparts, br) == "invalid"
    assert [bm.cl_geometry(c.R, c.C)[2] for c in RAW] == [2, 3, 257]
    for c in MAXPOOL:
        assert c.n in (1, 15, 16, 17, 33, 300) and c.c in (4, 24, 256, 260) and c.b in (1, 17, 33)
    assert {c.n for c in MAXPOOL} == {1, 15, 16, 17, 33, 300} and {c.c for c in MAXPOOL} == {4, 24, 256, 260}
    assert {c.b for c in MAXPOOL} == {1, 17, 33} and {c.act for c in MAXPOOL} == {0, 1, 2}
    assert [bm.mp_geometry(c) for c in (4, 24, 256, 260)] == [(1, 1, 256), (8, 1, 32), (64, 1, 4), (64, 2, 4)]
    for table in (GEOMETRY, BLOCKS, ROUNDED, RAW, EVAL, MAXPOOL):
        assert len({c.name for c in table}) == len(table)


check_table()
