"""The reference of tests/test_gpu_bn.py checked on the host: tests/bn_mirror.py against torch.nn.BatchNorm1d in float64 (forward,
autograd, running buffers, eval mode) and the torch stand-ins, its exactness guard on every case the GPU module compares bit for bit,
the case table of tests/bn_cases.py against the launch rules as csrc/bnact.hip and csrc/bn_geom.h state them today, and the table's
sharpness: every mutant of the mirror (bn_mirror.MUTANTS) differs from the mirror in at least one output bit on at least one case.

Tolerances.  The mirror's float64 mean and variance are sums of R terms and a handful of operations: (R + 8) * 2^-53 relative to the
data's scale.  Everything behind them is rounded to float32 where the kernels round (invstd, scale, shift, z, dz, the coefficients):
a chain of at most 8 such roundings per output element and one more per summed row in bsums, each 2^-24 relative -- outputs are held
to 16 * 2^-24, batch sums to (R + 16) * 2^-24, of the largest magnitude in the tensor."""
import numpy as np
import pytest
import torch

import bn_cases as bc
import bn_mirror as bm
import wgs_mirror as wm
from torch_standins import bn_act_maxpool_torch, bn_act_torch

U32, U64 = 2.0 ** -24, 2.0 ** -53
ACTS = ("none", "relu", "leaky_relu")


def _name(case):
    return case.name if hasattr(case, "name") else "-".join(map(str, case))


def _b(*arrays):
    return np.concatenate([np.ascontiguousarray(a).view(np.uint32).reshape(-1) if a.dtype == np.float32 else np.asarray(a, np.uint32).reshape(-1)
                           for a in arrays])


# ---------------------------------------------------------------------------- launch rules
def test_launch_rules_are_read_from_the_sources():
    assert bm.source_constants() == {"MP_SPLIT": 16, "MP_CGB": 64, "FB_MIN": 512, "FB64_MIN": 1400, "FB64_MAX": 128, "FB_WG": 512,
                                     "FB_MAX": 32, "FB_PER": 128}
    for R in (1, 2, 15, 16, 17, 255, 256, 257, 1024, 1025, 4096, 4097, 65536, 65537, 358400, 1 << 27):
        for C in (4, 8, 12, 16, 24, 40, 64, 100, 256, 260, 1020, 1024, 1028, 2048, 2052, 16384):
            assert bm.cl_geometry(R, C) == wm.cl_geometry(R, C), (R, C)
    assert [bm.fb_slices(16, n) for n in (511, 512)] == [0, 4] and [bm.fb_slices(64, n) for n in (1400, 1401)] == [0, 21]
    assert bm.fb_slices(128, 8192) == 128 and bm.fb_slices(128, 8193) == 128 and bm.fb_slices(128, 1 << 20) == 128
    assert bm.fb_slices(1028, 512) == 0 and bm.fb_slices(8, 8192) == 32 and bm.fb_slices(4, 1 << 20) == 32
    assert bm.blocks_scratch_doubles(64, 1401) == 21 * 2 * 64 and bm.blocks_scratch_doubles(16, 511) == 0
    assert bm.mp_splits(1)[:2] == [(0, 1), (1, 1)] and bm.mp_splits(17)[7:10] == [(14, 16), (16, 17), (17, 17)]
    assert bm.mp_splits(300)[-1] == (285, 300)


def test_every_regime_is_reached_and_named_by_its_case():
    bc.check_table()
    assert {c.want for c in bc.BLOCKS} == {c.want for c in bc.ROUNDED} == {"one_launch", "slice4", "slice64"}
    assert {bm.cl_geometry(c.R, c.C)[1] for c in bc.GEOMETRY} == {1, 2, 3}
    # every power-of-two cgb, each with single blocks of 1, rl, 3 rl + 1, 4 rl and 4 rl + 1 rows (check_table asserts the same)
    for cgb in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        rows = {c.R for c in bc.GEOMETRY if bm.cl_geometry(c.R, c.C)[:3] == (cgb, 1, 1)}
        rl = 256 // cgb
        assert rows >= {1, rl, 3 * rl + 1, 4 * rl, 4 * rl + 1}, (cgb, sorted(rows))
    assert max(c.R * c.C for c in bc.GEOMETRY) * 4 <= 17 << 20                    # the largest allocation


# ---------------------------------------------------------------------------- the guard on every case
@pytest.mark.parametrize("case", bc.GEOMETRY, ids=_name)
def test_guard_accepts_every_geometry_case_and_the_kinks_are_in_it(case):
    ref = bc.geometry_reference(case)                             # (runs assert_exact)
    z = ref["z"]
    assert (z == 0).any() and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    assert ref["y"].shape == ((2 * case.R, case.C // 2) if case.inter else (case.R, case.C))
    assert (ref["stats"][:case.C] < 0).any() and np.isfinite(ref["dx"]).all()


@pytest.mark.parametrize("case", bc.BLOCKS, ids=_name)
def test_guard_accepts_every_block_case(case):
    ref = bc.blocks_reference(case)
    assert ref["part"].shape == (case.nparts, 3 * case.C) and np.isnan(ref["part"][case.nparts - case.spare:]).all()
    assert np.isfinite(ref["part"][:case.nparts - case.spare]).all() and np.isfinite(ref["stats"]).all()


@pytest.mark.parametrize("case", bc.RAW, ids=_name)
def test_guard_accepts_every_raw_partial_case(case):
    assert bc.raw_reference(case)["part"].shape == (bm.cl_geometry(case.R, case.C)[2], 2 * case.C)


@pytest.mark.parametrize("case", bc.MAXPOOL, ids=_name)
def test_guard_accepts_every_maxpool_case_and_the_ties_are_in_it(case):
    ref = bc.maxpool_reference(case)
    assert np.array_equal(ref["own_max"].view(np.uint32), ref["pick_max"].view(np.uint32))        # one ymax, two tie rules
    assert np.array_equal(ref["hand_max"].view(np.uint32), ref["hand_pick_max"].view(np.uint32))
    u = ref["own_unique"]
    assert np.array_equal(ref["own_arg"][u], ref["pick_arg"][u])
    if case.n >= 15:
        assert not u.all() and not ref["hand_unique"].all()
    if case.n >= 15 and case.c >= 24:                             # scale 0, the plateau, equal activated bits: the rules part
        assert (ref["own_arg"] != ref["pick_arg"]).any() and (ref["hand_arg"] != ref["hand_pick_arg"]).any()


def test_end_to_end_references_pass_the_guard():
    t = bc.thin_reference()
    assert t["part"].shape == (6, 24) and t["block_rows"] == 256
    g = bc.gather_reference()
    assert g["out"].shape == (960, 64)


def test_guard_rejects_what_is_not_exact():
    g = bm.Guard()
    g.sum32("thirds", np.full((3, 2), 1.0 / 3.0, np.float32))
    with pytest.raises(AssertionError, match="quanta"):
        bm.assert_exact(g)
    g = bm.Guard()
    g.sum32("large", np.full((5, 1), 2.0 ** 21 + 0.25))           # five terms of 2^23 + 1 quarters: past 2^24 of them
    with pytest.raises(AssertionError, match="quanta"):
        bm.assert_exact(g)
    g = bm.Guard()
    g.sum32("wide", np.array([[1.0 + 2.0 ** -30]]))
    with pytest.raises(AssertionError, match="not a float32"):
        bm.assert_exact(g)
    g = bm.Guard()
    g.round32("midpoint", np.array([1.0 + 2.0 ** -24 + 2.0 ** -52]))
    with pytest.raises(AssertionError, match="midpoint"):
        bm.assert_exact(g)
    g = bm.Guard()
    g.sum32("two equal terms", np.array([[bm.SLOPE * 2], [0.0], [bm.SLOPE * 2]]))
    g.round32("far from a midpoint", np.array([1.0 + 2.0 ** -30]))
    bm.assert_exact(g)


def test_fma32_is_single_rounded():
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -60)
    # a*b = 1 + 2^-11 + 2^-24: a float32 midpoint; the tiny addend decides, which the float64 sum alone cannot see
    assert bm.fma32(a, b, c) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23) and bm.fma32(a, b, -c) == np.float32(1 + 2.0 ** -11)
    assert np.signbit(bm.fma32(np.float32(0), np.float32(-2), np.float32(-0.0))) and not np.signbit(bm.fma32(np.float32(0.5), np.float32(2), np.float32(-1)))


# ---------------------------------------------------------------------------- the three partial layouts
@pytest.mark.parametrize("case", bc.BLOCKS, ids=_name)
def test_three_partial_layouts_finalise_to_the_same_statistics(case):
    """Every block case's matrix through the own-pivot and the raw layout, and through numpy's mean and var: the block finaliser's
    float64 mean and variance agree with all three.  |x| < 1 on the lattice (up to 5 in a planted last block): x^2 and the blocks'
    squares stay below 32, R + 8 float64 operations each."""
    ref = bc.blocks_reference(case)
    X, R = ref["X"], ref["R"]
    own = bm.finalize_sums(bm.partials_own_pivot(X), R, X[0], bc.EPS)
    raw = bm.finalize_sums(bm.partials_own_pivot(X, raw=True), R, None, bc.EPS)
    x64 = X.astype(np.float64)
    tol = (R + 8) * U64 * 32.0
    for mean, var in ((own["mean64"], own["var64"]), (raw["mean64"], raw["var64"]), (x64.mean(0), x64.var(0))):
        np.testing.assert_allclose(ref["mean64"], mean, rtol=0, atol=tol)
        np.testing.assert_allclose(ref["var64"], var, rtol=0, atol=tol)


@pytest.mark.parametrize("case", bc.RAW, ids=_name)
def test_raw_partial_cases_against_numpy(case):
    ref = bc.raw_reference(case)
    x64 = ref["X"].astype(np.float64)
    np.testing.assert_allclose(ref["mean64"], x64.mean(0), rtol=0, atol=(case.R + 8) * U64)
    np.testing.assert_allclose(ref["var64"], x64.var(0), rtol=0, atol=(case.R + 8) * U64 * 2)
    np.testing.assert_allclose(ref["stats"][2 * case.C:3 * case.C], x64.mean(0), rtol=0, atol=U32)
    np.testing.assert_allclose(ref["stats"][3 * case.C:], 1 / np.sqrt(x64.var(0) + bc.EPS), rtol=2 * U32, atol=0)


# ---------------------------------------------------------------------------- the mirror against torch
def _torch_bn(C, p, run):
    bn = torch.nn.BatchNorm1d(C, eps=bc.EPS, momentum=bc.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(p["gamma"].astype(np.float64)))
        bn.bias.copy_(torch.from_numpy(p["beta"].astype(np.float64)))
        bn.running_mean.copy_(torch.from_numpy(run["rm"].astype(np.float64)))
        bn.running_var.copy_(torch.from_numpy(run["rv"].astype(np.float64)))
    return bn


@pytest.mark.parametrize("act", (0, 1, 2))
@pytest.mark.parametrize("R,C,inter,with_mul,training", [(50, 8, 0, True, True), (50, 8, 0, True, False), (36, 12, 9, False, True),
                                                          (36, 12, 9, False, False), (1, 4, 0, False, False), (300, 40, 0, False, True)])
def test_mirror_equals_batchnorm1d_in_float64(R, C, inter, with_mul, training, act):
    rng = np.random.default_rng(R * C + act)
    X = (rng.standard_normal((R, C)) * 1.5 + rng.standard_normal(C)).astype(np.float32)
    p = dict(gamma=rng.standard_normal(C).astype(np.float32), beta=rng.standard_normal(C).astype(np.float32), pre_bias=None)
    run = dict(rm=rng.standard_normal(C).astype(np.float32), rv=(0.5 + rng.random(C)).astype(np.float32))
    mul = rng.standard_normal((R, C)).astype(np.float32) if with_mul else None
    dy = rng.standard_normal((2 * R, C // 2) if inter else (R, C)).astype(np.float32)
    if training:
        fin = bm.finalize_sums(bm.partials_own_pivot(X), R, X[0], bc.EPS, bc.MOMENTUM, **p, **run)
        stats = fin["stats"]
    else:
        stats = bm.eval_stats(C, bc.EPS, rm=run["rm"], rv=run["rv"], **p)
    y, z = bm.apply(X, stats, act, mul, inter)
    bwd = bm.backward(X, dy, stats, act, training, mul, inter)
    bn = _torch_bn(C, p, run)
    xt = torch.from_numpy(X.astype(np.float64)).requires_grad_(True)
    mt = torch.from_numpy(mul.astype(np.float64)).requires_grad_(True) if with_mul else None
    yt = bn_act_torch(xt, bn, training, ACTS[act], mul=mt, interleave_n=inter)
    yt.backward(torch.from_numpy(dy.astype(np.float64)))
    scale = lambda a: max(1.0, float(np.abs(a).max()))
    if training:
        # on data that is on no lattice the kernel's float32 x - pivot rounds (half an ulp of |d| each): the mean carries U32 max|d|, the
        # variance 2 max|d| times that in the squares and again in ms^2
        d = scale(X.astype(np.float64) - X[0])
        np.testing.assert_allclose(fin["mean64"], X.astype(np.float64).mean(0), rtol=0, atol=U32 * d + (R + 8) * U64 * d)
        np.testing.assert_allclose(fin["var64"], X.astype(np.float64).var(0), rtol=0, atol=4 * U32 * d * d + (R + 8) * U64 * d * d)
        np.testing.assert_allclose(fin["running_mean"], bn.running_mean.numpy(), rtol=0, atol=4 * U32 * scale(bn.running_mean.numpy()))
        np.testing.assert_allclose(fin["running_var"], bn.running_var.numpy(), rtol=0, atol=4 * U32 * scale(bn.running_var.numpy()))
    want = yt.detach().numpy()
    np.testing.assert_allclose(y, want, rtol=0, atol=16 * U32 * scale(want))
    # the gradients amplify the rounding of xhat by |dgamma| <= R max|dz*xhat|: the batch-sum bound carries over to dx
    np.testing.assert_allclose(bwd["dx"], xt.grad.numpy(), rtol=0, atol=(R + 16) * U32 * scale(xt.grad.numpy()) * scale(1 / np.sqrt(X.var(0) + bc.EPS) if training else 1.0))
    np.testing.assert_allclose(bwd["bsums"][:C], bn.bias.grad.numpy(), rtol=0, atol=(R + 16) * U32 * scale(dy) * scale(mul if with_mul else 1.0))
    np.testing.assert_allclose(bwd["bsums"][C:], bn.weight.grad.numpy(), rtol=0, atol=(R + 16) * U32 * scale(bn.weight.grad.numpy()))
    if with_mul:
        np.testing.assert_allclose(bwd["dmul"], mt.grad.numpy(), rtol=0, atol=16 * U32 * scale(mt.grad.numpy()))


def _act64(z, act):
    return z if act == 0 else (np.maximum(z, 0.0) if act == 1 else np.where(z > 0, z, 0.01 * z))


def _reference64(X, p, run, act, mul, inter, dy):
    """What float64 makes of a training-mode BatchNorm + activation on X + pre_bias and of its gradients for dy (None: forward only):
    BatchNorm1d and the stand-in through autograd.  torch refuses a training batch of ONE row; there the closed form stands in:
    mean = x, var = 0, so z = beta whatever x is, dx = 0, dgamma = 0, dbeta = dz, and -- the kernels' choice, include/pdgn_hip.h -- the
    running variance is blended with the biased variance 0."""
    R, C = X.shape
    x64, pb = X.astype(np.float64), p["pre_bias"].astype(np.float64)
    if R > 1:
        bn = _torch_bn(C, p, run)
        xt = torch.from_numpy(x64).requires_grad_(True)
        mt = torch.from_numpy(mul.astype(np.float64)) if mul is not None else None
        z = bn_act_torch(torch.from_numpy(x64), _torch_bn(C, p, run), True, "none", pre_bias=torch.from_numpy(pb)).detach().numpy()
        yt = bn_act_torch(xt, bn, True, ACTS[act], mul=mt, pre_bias=torch.from_numpy(pb), interleave_n=inter)
        out = dict(y=yt.detach().numpy(), z=z, rm=bn.running_mean.numpy().copy(), rv=bn.running_var.numpy().copy())
        if dy is not None:
            yt.backward(torch.from_numpy(dy.astype(np.float64)))
            out.update(dx=xt.grad.numpy(), dbeta=bn.bias.grad.numpy(), dgamma=bn.weight.grad.numpy())
        return out
    z = np.broadcast_to(p["beta"].astype(np.float64), (1, C)).copy()
    y = _act64(z, act) * (mul.astype(np.float64) if mul is not None else 1.0)
    out = dict(y=bm.interleave(y, inter) if inter else y, z=z, rm=(1 - bc.MOMENTUM) * run["rm"] + bc.MOMENTUM * (x64[0] + pb),
               rv=(1 - bc.MOMENTUM) * run["rv"].astype(np.float64))
    if dy is not None:
        g = (bm.deinterleave(dy, inter) if inter else dy).astype(np.float64) * (mul.astype(np.float64) if mul is not None else 1.0)
        slope = np.ones_like(z) if act == 0 else np.where(z > 0, 1.0, 0.0 if act == 1 else 0.01)
        out.update(dx=np.zeros((1, C)), dbeta=(g * slope)[0], dgamma=np.zeros(C))
    return out


@pytest.mark.parametrize("case", bc.GEOMETRY, ids=_name)
def test_mirror_equals_torch_on_every_geometry_case(case):
    """The case's own x, parameters, mul and dy: the statistics the mirror finalises from x, applied and differentiated by the
    mirror, against `_reference64`.  z = fma(x, scale, shift) rounds relative to |x*scale| and |shift|, not to |z|: the output's
    bound is 16 * 2^-24 of the largest of them."""
    R, C = case.R, case.C
    ref = bc.geometry_reference(case)
    p, run, X = ref["p"], ref["run"], ref["X"]
    s = lambda a: max(1.0, float(np.abs(a).max()))
    inv = s(1 / np.sqrt(X.astype(np.float64).var(0) + bc.EPS))
    # act' jumps at z == 0: where float64 puts z within the float32 rounding of it (a channel of equal values: x - mean is pure
    # rounding, times 1/sqrt(eps)), the two sides may differ -- no gradient is sent there
    zt = _reference64(X, p, run, 0, None, 0, None)["z"]
    near = (np.abs(zt) <= 256 * U32 * s(zt) * inv) & (case.act != 0)
    dy = ref["dy"].copy()
    dy[bm.interleave(near, case.inter) if case.inter else near] = 0.0
    y, _ = bm.apply(X, ref["fin"], case.act, ref["mul"], case.inter)
    bwd = bm.backward(X, dy, ref["fin"], case.act, True, ref["mul"], case.inter)
    want = _reference64(X, p, run, case.act, ref["mul"], case.inter, dy)
    mag = max(s(want["y"]), s(X * ref["fin"][:C]), s(ref["fin"][C:2 * C])) * s(ref["mul"] if case.mul else 1.0)
    np.testing.assert_allclose(y, want["y"], rtol=0, atol=16 * U32 * mag)
    np.testing.assert_allclose(ref["rm"], want["rm"], rtol=0, atol=4 * U32 * s(want["rm"]))
    np.testing.assert_allclose(ref["rv"], want["rv"], rtol=0, atol=4 * U32 * s(want["rv"]))
    np.testing.assert_allclose(bwd["dx"], want["dx"], rtol=0, atol=(R + 16) * U32 * s(want["dx"]) * inv)
    np.testing.assert_allclose(bwd["bsums"][:C], want["dbeta"], rtol=0, atol=(R + 16) * U32 * s(ref["dy"]) * s(ref["mul"] if case.mul else 1.0))
    np.testing.assert_allclose(bwd["bsums"][C:], want["dgamma"], rtol=0, atol=(R + 16) * U32 * s(want["dgamma"]) * inv)


@pytest.mark.parametrize("case", bc.MAXPOOL, ids=_name)
def test_mirror_equals_the_torch_standin_on_every_maxpool_case(case):
    ref = bc.maxpool_reference(case)
    C = case.c
    want64 = _reference64(ref["X"], ref["p"], ref["run"], case.act, None, 0, None)
    full = torch.from_numpy(want64["y"]).view(case.b, case.n, C)
    want, idx = full.max(dim=1)
    mag = max(1.0, float(want.abs().max()), float(np.abs(ref["X"] * ref["own"][:C]).max()), float(np.abs(ref["own"][C:2 * C]).max()))
    np.testing.assert_allclose(ref["pick_max"], want.numpy(), rtol=0, atol=16 * U32 * mag)
    np.testing.assert_allclose(ref["rm"], want64["rm"], rtol=0, atol=4 * U32 * max(1.0, float(np.abs(want64["rm"]).max())))
    np.testing.assert_allclose(ref["rv"], want64["rv"], rtol=0, atol=4 * U32 * max(1.0, float(np.abs(want64["rv"]).max())))
    # where ONE row attains the maximum -- in float64 too, by more than the float32 roundings could bridge -- the indices are exact
    top2 = full.topk(min(2, case.n), dim=1)[0]
    clear = (top2[:, 0] - top2[:, -1]).numpy() > 64 * U32 * mag if case.n > 1 else np.ones((case.b, C), bool)
    np.testing.assert_array_equal(ref["own_arg"][clear], idx.numpy()[clear])      # (few: these cases are made of ties)
    np.testing.assert_array_equal(ref["pick_arg"][clear], idx.numpy()[clear])
    if case.b * case.n > 1:                                       # (the stand-in is torch's training mode: not for a batch of one row)
        pooled = bn_act_maxpool_torch(torch.from_numpy(ref["X"].astype(np.float64)), _torch_bn(C, ref["p"], ref["run"]), True, case.b, case.n,
                                      ACTS[case.act], pre_bias=torch.from_numpy(ref["p"]["pre_bias"].astype(np.float64)))
        assert torch.equal(pooled.detach(), want)


def test_pre_bias_enters_the_running_mean_and_the_eval_mean_only():
    rng = np.random.default_rng(5)
    R, C = 40, 8
    X = rng.standard_normal((R, C)).astype(np.float32)
    pb = rng.standard_normal(C).astype(np.float32)
    p = dict(gamma=rng.standard_normal(C).astype(np.float32), beta=rng.standard_normal(C).astype(np.float32))
    run = dict(rm=rng.standard_normal(C).astype(np.float32), rv=(0.5 + rng.random(C)).astype(np.float32))
    fin = bm.finalize_sums(bm.partials_own_pivot(X), R, X[0], bc.EPS, bc.MOMENTUM, pre_bias=pb, **p, **run)
    bare = bm.finalize_sums(bm.partials_own_pivot(X), R, X[0], bc.EPS, bc.MOMENTUM, pre_bias=None, **p, **run)
    assert np.array_equal(fin["stats"], bare["stats"]) and np.array_equal(fin["running_var"], bare["running_var"])
    bn = _torch_bn(C, dict(p, pre_bias=None), run)
    xt, pbt = torch.from_numpy(X.astype(np.float64)), torch.from_numpy(pb.astype(np.float64))
    want = bn_act_torch(xt, bn, True, "none", pre_bias=pbt).detach().numpy()
    np.testing.assert_allclose(bm.apply(X, fin["stats"], 0)[0], want, rtol=0, atol=16 * U32 * np.abs(want).max())
    np.testing.assert_allclose(fin["running_mean"], bn.running_mean.numpy(), rtol=0, atol=4 * U32 * 4)
    ev = bm.eval_stats(C, bc.EPS, rm=fin["running_mean"], rv=fin["running_var"], pre_bias=pb, **p)
    bn.eval()
    want = bn_act_torch(xt, bn, False, "relu", pre_bias=pbt).detach().numpy()
    np.testing.assert_allclose(bm.apply(X, ev, 1)[0], want, rtol=0, atol=16 * U32 * max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("act", (0, 1, 2))
@pytest.mark.parametrize("B,N,C", [(3, 17, 8), (1, 1, 4), (5, 40, 12)])
def test_mirror_maxpool_equals_the_torch_standin_and_its_autograd(B, N, C, act):
    rng = np.random.default_rng(B * N + C + act)
    X = rng.standard_normal((B * N, C)).astype(np.float32)
    p = dict(gamma=rng.standard_normal(C).astype(np.float32), beta=rng.standard_normal(C).astype(np.float32), pre_bias=None)
    run = dict(rm=np.zeros(C, np.float32), rv=np.ones(C, np.float32))
    training = B * N > 1
    stats = bm.maxpool_stats(X, B, N, eps=bc.EPS, momentum=bc.MOMENTUM, **p, **run)["stats"] if training else \
        bm.eval_stats(C, bc.EPS, rm=run["rm"], rv=run["rv"], **p)
    ymax, yarg, unique = bm.maxpool_apply(X, stats, act, B, N)
    pmax, parg = bm.maxpool_pick(X, stats, act, B, N)
    assert (unique.all() or act == 1) and np.array_equal(yarg[unique], parg[unique]) and np.array_equal(ymax.view(np.uint32), pmax.view(np.uint32))
    dout = rng.standard_normal((B, C)).astype(np.float32)
    bwd = bm.maxpool_backward(X, dout, yarg, stats, act, training, B, N)
    bn = _torch_bn(C, p, run)
    xt = torch.from_numpy(X.astype(np.float64)).requires_grad_(True)
    full = bn_act_torch(xt, bn, training, ACTS[act]).view(B, N, C)
    bn2 = _torch_bn(C, p, run)
    pooled = bn_act_maxpool_torch(xt, bn2, training, B, N, ACTS[act])
    # Gaussian data: the maxima are unique (but on ReLU's plateau) and the indices exact; on the plateau the lowest row, as torch's
    np.testing.assert_array_equal(full.max(dim=1)[1].numpy()[unique], yarg[unique])
    assert (yarg[~unique] == 0).all()
    np.testing.assert_allclose(ymax, pooled.detach().numpy(), rtol=0, atol=16 * U32 * max(1.0, float(pooled.detach().abs().max())))
    pooled.backward(torch.from_numpy(dout.astype(np.float64)))
    s = lambda a: max(1.0, float(np.abs(a).max()))
    inv = s(1 / np.sqrt(X.var(0) + bc.EPS)) if training else 1.0
    np.testing.assert_allclose(bwd["dx"], xt.grad.numpy(), rtol=0, atol=(B + 16) * U32 * s(xt.grad.numpy()) * inv)
    np.testing.assert_allclose(bwd["bsums"][:C], bn2.bias.grad.numpy(), rtol=0, atol=(B + 16) * U32 * s(dout))
    np.testing.assert_allclose(bwd["bsums"][C:], bn2.weight.grad.numpy(), rtol=0, atol=(B + 16) * U32 * s(bn2.weight.grad.numpy()) * inv)


def test_interleave_is_the_products_regrouping():
    from pdgn_amd.fused import interleave_rows
    y = np.arange(6 * 8, dtype=np.float32).reshape(6, 8)
    want = interleave_rows(torch.from_numpy(y), 3).numpy()
    assert np.array_equal(bm.interleave(y, 3), want) and np.array_equal(bm.deinterleave(want, 3), y)
    assert not np.array_equal(bm.interleave(y, 3, {"interleave_2n"}), want)


# ---------------------------------------------------------------------------- sharpness: every mutant is told from the mirror
def _geo(name, mut):
    case = bc.by_name(bc.GEOMETRY, name)
    ref = bc.geometry_reference(case)
    fin = bm.finalize_sums(ref["part"], case.R, ref["X"][0], bc.EPS, bc.MOMENTUM, mut=mut, **ref["p"], **ref["run"])
    y, _ = bm.apply(ref["X"], ref["stats"], case.act, ref["mul"], case.inter, mut=mut)
    bwd = bm.backward(ref["X"], ref["dy"], ref["stats"], case.act, case.training, ref["mul"], case.inter, mut=mut)
    return _b(fin["stats"], fin["running_mean"], fin["running_var"], y, bwd["bsums"], bwd["dx"], bwd["dmul"], bwd["coef"])


def _blk(name, mut):
    case = bc.by_name(bc.BLOCKS, name)
    ref = bc.blocks_reference(case)
    fin = bm.finalize_blocks(ref["part"], ref["R"], case.block_rows, ref["slices"], bc.EPS, bc.MOMENTUM, mut=mut, **ref["p"], **ref["run"])
    return _b(fin["stats"], fin["running_mean"], fin["running_var"])


def _mp(name, mut):
    case = bc.by_name(bc.MAXPOOL, name)
    ref = bc.maxpool_reference(case)
    a = bm.maxpool_apply(ref["X"], ref["hand"], case.act, case.b, case.n, mut=mut)
    o = bm.maxpool_pick(ref["X"], ref["own"], case.act, case.b, case.n, mut=mut)
    bwd = bm.maxpool_backward(ref["X"], ref["dout"], ref["hand_arg"], ref["hand"], case.act, 1, case.b, case.n, mut=mut)
    return _b(a[0], a[1], o[0], o[1], bwd["bsums"], bwd["dx"], bwd["coef"])


SHARP = {"last_block_full": (_blk, ["n65", "n257", "slice4_8"]), "spare_rows": (_blk, ["n65_spare", "slice4_spare", "slice64_spare"]),
         "no_pivot": (_geo, ["c24_rows32", "two_blocks"]), "biased_running_var": (_geo, ["c24_rows32", "idle_columns_10_of_16"]),
         "pre_bias_in_mean": (_geo, ["c24_rows32", "one_row"]), "drop_last_slice": (_blk, ["slice4_4x128", "slice64_21", "slice64_br256"]),
         "ties_highest": (_mp, ["n33", "n300_idle"]), "no_min_branch": (_mp, ["n15", "n33_c4_rot"]),
         "kink_grad_one": (_geo, ["c24_rows32", "one_row", "two_blocks"]), "interleave_2n": (_geo, ["c256_rows16", "idle_columns_6_of_8"]),
         "ca_without_mean": (_geo, ["c24_rows97", "idle_columns_10_of_16"])}


@pytest.mark.parametrize("mutant", bm.MUTANTS)
def test_every_mutant_differs_from_the_mirror_in_some_output_bit(mutant):
    run, names = SHARP[mutant]
    told = [name for name in names if not np.array_equal(run(name, frozenset()), run(name, frozenset({mutant})))]
    assert told, "no case of the table tells the mutant %s from the mirror: the table lacks a case" % mutant
    assert np.array_equal(run(names[0], frozenset()), run(names[0], frozenset()))      # (the mirror itself is deterministic)
    assert set(SHARP) == set(bm.MUTANTS) and len(bm.MUTANTS) == 11


def test_the_clamped_slice_case_has_an_empty_last_slice():
    """Dropping the last slice of (128, 8193) changes nothing -- it holds no partial row -- which is why the table also has (64, 1401)."""
    assert np.array_equal(_blk("slice64_clamped", frozenset()), _blk("slice64_clamped", frozenset({"drop_last_slice"})))
