"""csrc/bnact.hip in every geometry and finalisation regime: the statistics pass, the four finalisers (own pivot, raw partials,
block-shifted partials in their one-launch, four-channel-slice and 64-channel-slice forms, eval), the apply pass, the three-launch
backward and both max-pool tails with their adjoint -- against tests/bn_mirror.py on the cases of tests/bn_cases.py, whose every sum
is exact in whatever order it is taken (the mirror's guard ran on each case before anything is compared; tests/test_bn_mirror_host.py
checks mirror, guard and case table on the host).  Every output and scratch buffer is a slice of a sentinel-filled allocation
(tests/bn_worker.py).  In the exact tier every comparison is an equality of bit patterns and every call runs twice.

One freedom is left open: C's fmaxf(-0, +0) may return either zero, so the SIGN of a zero that ReLU makes of z == -0 is not compared
(nor that of its products with mul and dy).

The rounded tier (block finaliser, block_rows or last block not a power of two) bounds mean, invstd and the running statistics by one
float32 ulp around the correctly rounded exact value of the given float32 partials: with |mean| <= 8 std the cancellation in
b/R - mean^2 amplifies the float64 error by at most 2^7, and at most nparts float64 additions stay far below a float32 ulp; the
float64 -> float32 rounding then lands on the correctly rounded value or its neighbour.  The running buffers start at zero with
momentum 1/8, so that the blend adds no rounding of its own.  pdgn_bn_eval_stats' rsqrtf is the hardware approximation (HIP documents
1 ulp): invstd is bounded by one ulp and the other three rows are restated bit for bit from the device's own invstd."""
import numpy as np
import pytest
import torch

import bn_cases as bc
import bn_mirror as bm
import bn_worker as bw
from bn_worker import bits, twice

pytestmark = pytest.mark.gpu
SIGN = np.uint32(0x80000000)


def _name(case):
    return case.name if hasattr(case, "name") else "-".join(map(str, case))


def same_bits(got, want, sign_free=None, what=""):
    got, want = np.asarray(got), bits(want).reshape(np.shape(got))
    if sign_free is not None and sign_free.any():
        free = sign_free.reshape(got.shape) & ((got & ~SIGN) == 0)
        got, want = np.where(free, got & ~SIGN, got), np.where(free, want & ~SIGN, want)
    np.testing.assert_array_equal(got, want, err_msg=what)


def ulps_apart(got_bits, want):
    """Distance in float32 steps between a device's bit patterns and float32 values."""
    def key(u):
        u = u.astype(np.int64)
        return np.where(u & 0x80000000, 0x80000000 - u, u)
    return np.abs(key(np.asarray(got_bits, np.uint32)) - key(bits(want)))


def round32(values):
    """Fractions / floats correctly rounded to float32."""
    return np.array([bm._round_fraction32(v) if not isinstance(v, float) else bm.F32(v) for v in values], bm.F32)


# ---------------------------------------------------------------------------- A. row-by-channel geometry
@pytest.mark.parametrize("case", bc.GEOMETRY, ids=_name)
def test_statistics_pass_and_own_pivot_finaliser(case):
    ref = bc.geometry_reference(case)
    stats, rm, rv, part = twice(bw.device_stats, ref["X"], ref["p"], ref["run"], bc.EPS, bc.MOMENTUM)
    assert np.isfinite(part).all(), "a partial row is not finite"
    np.testing.assert_array_equal(part.astype(np.float64).sum(0), ref["part"].sum(0))
    same_bits(stats, ref["fin"], what="stats")
    same_bits(rm, ref["rm"], what="running_mean")
    same_bits(rv, ref["rv"], what="running_var")


@pytest.mark.parametrize("case", bc.GEOMETRY, ids=_name)
def test_apply_pass(case):
    ref = bc.geometry_reference(case)
    (y,) = twice(bw.device_forward, ref["X"], ref["stats"], case.act, ref["mul"], case.inter)
    free = bm.relu_zero_sign_free(ref["z"], case.act)
    same_bits(y, ref["y"], bm.interleave(free, case.inter) if case.inter else free)
    z = ref["z"]
    assert (z == 0).any() and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()      # both zeros are in the case


@pytest.mark.parametrize("case", bc.GEOMETRY, ids=_name)
def test_backward_sums_coefficients_and_gradients(case):
    ref = bc.geometry_reference(case)
    bs, dx, coef, dmul = twice(bw.device_backward, ref["X"], ref["dy"], ref["stats"], case.act, case.training, ref["mul"], case.inter)
    same_bits(bs, ref["bsums"], what="bsums")
    same_bits(coef, ref["coef"], what="coef")
    same_bits(dx, ref["dx"], what="dx")
    same_bits(dmul, ref["dmul"], bm.relu_zero_sign_free(ref["z"], case.act), what="dmul")
    bs2, dx2, coef2 = bw.device_backward(ref["X"], ref["dy"], ref["stats"], case.act, case.training, ref["mul"], case.inter, want_dmul=False)
    assert np.array_equal(bs2, bs) and np.array_equal(dx2, dx) and np.array_equal(coef2, coef)


@pytest.mark.parametrize("args", bc.APPLY_REFUSED, ids=_name)
def test_apply_and_backward_refuse_what_they_document(args):
    rc1, rc2, untouched = bw.device_apply_refused(*args)
    assert rc1 == bw.INVALID and rc2 == bw.INVALID and untouched


# ---------------------------------------------------------------------------- B. the block finaliser
@pytest.mark.parametrize("case", bc.BLOCKS, ids=_name)
def test_block_finaliser_in_every_form(case):
    """Spare partial rows hold NaN and must not be read; the sliced forms and the scratch == NULL form give the same bytes."""
    ref = bc.blocks_reference(case)
    got = twice(bw.device_from_blocks, ref["part"], ref["R"], case.C, case.block_rows, ref["p"], ref["run"], bc.EPS, bc.MOMENTUM)
    for g, name in zip(got, ("stats", "rm", "rv")):
        same_bits(g, ref[name], what=name)
    if case.want != "one_launch":
        plain = bw.device_from_blocks(ref["part"], ref["R"], case.C, case.block_rows, ref["p"], ref["run"], bc.EPS, bc.MOMENTUM, with_scratch=False)
        for g, p_ in zip(got, plain):
            assert np.array_equal(g, p_), "the one-launch form gives other bytes than the sliced one"
    bare = bw.device_from_blocks(ref["part"], ref["R"], case.C, case.block_rows, dict(gamma=None, beta=None, pre_bias=None), None, bc.EPS, bc.MOMENTUM)
    want = bm.finalize_blocks(ref["part"], ref["R"], case.block_rows, ref["slices"], bc.EPS, bc.MOMENTUM)["stats"]
    same_bits(bare[0], want, what="stats without gamma, beta and running buffers")


@pytest.mark.parametrize("case", bc.ROUNDED, ids=_name)
def test_block_finaliser_rounded_tier(case):
    ref = bc.rounded_reference(case)
    C = case.C
    run = dict(rm=np.zeros(C, np.float32), rv=np.zeros(C, np.float32))
    for with_scratch in (True, False):
        stats, rm, rv = bw.device_from_blocks(ref["part"], ref["R"], C, case.block_rows, ref["p"], run, bc.EPS, 0.125, with_scratch=with_scratch)
        got = stats.view(np.float32)
        scale, shift, mean, invstd = got[:C], got[C:2 * C], got[2 * C:3 * C], got[3 * C:]
        assert ulps_apart(stats[2 * C:3 * C], round32(ref["mean"])).max() <= 1
        assert ulps_apart(stats[3 * C:], round32([float(v) for v in ref["invstd"]])).max() <= 1
        assert ulps_apart(rm, round32([m / 8 for m in ref["mean"]])).max() <= 1
        assert ulps_apart(rv, round32([v / 8 for v in ref["unbiased"]])).max() <= 1
        want_scale = ref["p"]["gamma"] * invstd
        same_bits(stats[:C], want_scale, what="scale = fl(gamma*invstd)")
        same_bits(stats[C:2 * C], ref["p"]["beta"] - mean * want_scale, what="shift = fl(beta - fl(mean*scale))")


@pytest.mark.parametrize("args", bc.BLOCKS_REFUSED, ids=_name)
def test_block_finaliser_refuses_what_it_documents(args):
    rc, untouched = bw.device_blocks_refused(*args)
    assert rc == bw.INVALID and untouched


# ---------------------------------------------------------------------------- C. raw partials, eval
@pytest.mark.parametrize("case", bc.RAW, ids=_name)
def test_raw_partials_finaliser(case):
    ref = bc.raw_reference(case)
    got = twice(bw.device_from_partials, ref["part"], case.R, case.C, ref["p"], ref["run"], bc.EPS, bc.MOMENTUM)
    for g, name in zip(got, ("stats", "rm", "rv")):
        same_bits(g, ref[name], what=name)


@pytest.mark.parametrize("case", bc.EVAL, ids=_name)
def test_eval_finaliser(case):
    ref = bc.eval_reference(case)
    C = case.C
    (stats,) = twice(bw.device_eval, C, ref["p"], ref["run"], bc.EPS)
    exact = bm.eval_stats(C, bc.EPS, rm=ref["run"]["rm"], rv=ref["run"]["rv"], **ref["p"])
    assert ulps_apart(stats[3 * C:], exact[3 * C:]).max() <= 1
    same_bits(stats, bm.eval_stats(C, bc.EPS, rm=ref["run"]["rm"], rv=ref["run"]["rv"], invstd=stats[3 * C:].view(np.float32), **ref["p"]))


# ---------------------------------------------------------------------------- D. max-pool tails
def _zero_free(act, z):
    """z of the row a form names: the pooled zero's sign is open only where that z is -0 (on the plateau, z < 0, it is +0)."""
    return bm.relu_zero_sign_free(z, act)


@pytest.mark.parametrize("case", bc.MAXPOOL, ids=_name)
def test_maxpool_forms_and_their_tie_rules(case):
    """The contract of include/pdgn_hip.h: both forms return the same ymax bits for the same statistics; the apply form's yarg is the
    lowest row attaining ymax; the one-pass form's is the lowest row attaining the largest x (scale >= 0) or the smallest x
    (scale < 0), and that row's activated value has ymax's bits; where the maximum is unique both name it."""
    ref = bc.maxpool_reference(case)
    b, n, c = case.b, case.n, case.c
    stats, rm, rv, ymax, yarg = twice(bw.device_maxpool_onepass, ref["X"], ref["p"], ref["run"], case.act, b, n, bc.EPS, bc.MOMENTUM)
    same_bits(stats, ref["own"], what="stats")
    same_bits(rm, ref["rm"], what="running_mean")
    same_bits(rv, ref["rv"], what="running_var")
    same_bits(ymax, ref["pick_max"], _zero_free(case.act, ref["pick_z"]), what="one-pass ymax")
    np.testing.assert_array_equal(yarg, ref["pick_arg"])
    amax, aarg = twice(bw.device_maxpool_apply, ref["X"], ref["own"], case.act, b, n)
    same_bits(amax, ref["own_max"], _zero_free(case.act, ref["own_z"]), what="apply-form ymax")
    np.testing.assert_array_equal(aarg, ref["own_arg"])
    free = _zero_free(case.act, ref["own_z"]) | _zero_free(case.act, ref["pick_z"])      # (the forms may name different rows)
    assert np.array_equal(np.where(free, amax & ~SIGN, amax), np.where(free, ymax & ~SIGN, ymax)), "the two forms disagree on ymax"
    u = ref["own_unique"]
    assert np.array_equal(aarg[u], yarg[u])
    hmax, harg = twice(bw.device_maxpool_apply, ref["X"], ref["hand"], case.act, b, n)
    same_bits(hmax, ref["hand_max"], _zero_free(case.act, ref["hand_z"]), what="apply-form ymax, hand-made statistics")
    np.testing.assert_array_equal(harg, ref["hand_arg"])


@pytest.mark.parametrize("case", bc.MAXPOOL, ids=_name)
@pytest.mark.parametrize("training", (1, 0))
@pytest.mark.parametrize("which", ("apply", "pick"))
def test_maxpool_adjoint(case, training, which):
    """With the yarg of either form (they differ at scale == 0, on the plateau and on rounding ties): the gradient goes to the row named."""
    ref = bc.maxpool_reference(case)
    want = ref["bwd"][(training, which)]
    yarg = ref["hand_arg"] if which == "apply" else ref["hand_pick_arg"]
    bs, dx, scr = twice(bw.device_maxpool_backward, ref["X"], ref["dout"], yarg, ref["hand"], case.act, training, case.b, case.n)
    same_bits(bs, want["bsums"], what="bsums")
    same_bits(scr, np.concatenate([want["dz"].reshape(-1), want["coef"]]), what="dz | ca | cb")
    same_bits(dx, want["dx"], what="dx")


@pytest.mark.parametrize("args", bc.MAXPOOL_REFUSED, ids=_name)
def test_maxpool_entry_points_refuse_what_they_document(args):
    rcs, untouched = bw.device_maxpool_refused(*args)
    assert rcs == (bw.INVALID,) * 3 and untouched


# ---------------------------------------------------------------------------- E. end to end
def _module(C, p, run):
    bn = torch.nn.BatchNorm1d(C, eps=bc.EPS, momentum=bc.MOMENTUM).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(p["gamma"]))
        bn.bias.copy_(torch.from_numpy(p["beta"]))
        bn.running_mean.copy_(torch.from_numpy(run["rm"]))
        bn.running_var.copy_(torch.from_numpy(run["rv"]))
    return bn


@pytest.mark.parametrize("name", ["idle_columns_10_of_16", "gx2"])
def test_bn_act_end_to_end_own_statistics_pass(name):
    """pdgn_amd.fused.bn_act hands pdgn_bn_stats and pdgn_bn_act_forward the rows it was given: output and running buffers bit for bit."""
    from pdgn_amd import fused
    case = bc.by_name(bc.GEOMETRY, name)
    ref = bc.geometry_reference(case)
    bn = _module(case.C, ref["p"], ref["run"])
    act = ("none", "relu", "leaky_relu")[case.act]
    y = fused.bn_act(bw.dev(ref["X"]), bn, True, act=act, pre_bias=bw.dev(ref["p"]["pre_bias"]))
    want, z = bm.apply(ref["X"], ref["fin"], case.act)
    same_bits(bits(y.detach().cpu().numpy()), want, bm.relu_zero_sign_free(z, case.act))
    same_bits(bits(bn.running_mean.cpu().numpy()), ref["rm"])
    same_bits(bits(bn.running_var.cpu().numpy()), ref["rv"])


def test_bn_act_end_to_end_block_partials_from_the_thin_layer():
    """linear_cl's thin path hands bn_act the partial rows of pdgn_thin_nt's epilogue together with their block size; bn_act hands
    pdgn_bn_stats_from_gemm_partials the rows, nparts and block_rows the producer used."""
    from pdgn_amd import _lib, fused
    ref = bc.thin_reference()
    t = bc.THIN
    assert _lib.lib().pdgn_thin_stat_block_rows() == ref["block_rows"]
    bn = _module(t["n"], ref["p"], ref["run"])
    y, partials = fused.linear_cl(bw.dev(ref["x"]), bw.dev(ref["w"]), want_stats=True)
    part, block_rows = partials
    assert block_rows == ref["block_rows"] and tuple(part.shape) == ref["part"].shape
    same_bits(bits(y.cpu().numpy()), ref["y"], what="y = x W^T")
    same_bits(bits(part.cpu().numpy()), ref["part"], what="the epilogue's partial rows")
    out = fused.bn_act(y, bn, True, act="relu", partials=partials)
    same_bits(bits(out.detach().cpu().numpy()), ref["out"], bm.relu_zero_sign_free(ref["z"], t["act"]))
    same_bits(bits(bn.running_mean.cpu().numpy()), ref["rm"])
    same_bits(bits(bn.running_var.cpu().numpy()), ref["rv"])


def test_bn_act_end_to_end_raw_partials_from_the_gather_sum():
    from pdgn_amd import fused
    from pdgn_amd.deconv import EdgeGatherSum
    ref = bc.gather_reference()
    case, wgs = ref["case"], ref["wgs"]
    T, P, C, off, offc = case.spec
    bn = _module(C, ref["p"], ref["run"])
    bias = bw.dev(wgs["bias"]) if wgs["bias"] is not None else None
    out, part = EdgeGatherSum.apply(bw.dev(wgs["Y"]), bw.dev(wgs["idx"]), (case.spec + (True,),), bias)
    same_bits(bits(out.cpu().numpy()), wgs["out"], what="the gather-sum's output")
    y = fused.bn_act(out.view(-1, C), bn, True, act="leaky_relu", partials=part)
    same_bits(bits(y.detach().cpu().numpy()), ref["out"])
    same_bits(bits(bn.running_mean.cpu().numpy()), ref["rm"])
    same_bits(bits(bn.running_var.cpu().numpy()), ref["rv"])


@pytest.mark.parametrize("name", ["n300_idle", "n17_gx2"])
def test_bn_act_maxpool_end_to_end_one_pass(name):
    """Both routes of fused.bn_act_maxpool return the same ymax bits, by the contract above; the yarg it saves for the backward tells
    them apart: the one-pass form's rule, which differs from the apply form's at the planted ties."""
    from pdgn_amd import fused
    case = bc.by_name(bc.MAXPOOL, name)
    ref = bc.maxpool_reference(case)
    bn = _module(case.c, ref["p"], ref["run"])
    act = ("none", "relu", "leaky_relu")[case.act]
    y = fused.bn_act_maxpool(bw.dev(ref["X"]), bn, True, case.b, case.n, act=act, pre_bias=bw.dev(ref["p"]["pre_bias"]))
    same_bits(bits(y.detach().cpu().numpy()), ref["pick_max"], _zero_free(case.act, ref["pick_z"]))
    saved = [t for t in y.grad_fn.saved_tensors if t.dtype == torch.int32]
    assert len(saved) == 1 and (ref["pick_arg"] != ref["own_arg"]).any()
    np.testing.assert_array_equal(saved[0].cpu().numpy(), ref["pick_arg"])
    same_bits(bits(bn.running_mean.cpu().numpy()), ref["rm"])
    same_bits(bits(bn.running_var.cpu().numpy()), ref["rv"])
