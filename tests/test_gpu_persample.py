"""The per-sample layer kernels -- csrc/skinny.hip (nt / nt_act / nn / nn_masked / tn) and csrc/small_mlp.hip (forward / backward) -- in
every launch regime (tests/persample_cases.py; tests/test_persample_host.py checks table, guards and regime coverage on the host),
straight through the C ABI (tests/persample_worker.py: pitched, sentinel-banded outputs; every call twice, same bytes), and the
Python routes in front of them (pdgn_amd.fused).

Tier 1, bit patterns: small-integer operands, every sum exact in any order.  LeakyReLU is one float32 multiply of the exact value.
    One freedom: a column of dpre that holds only -0 (ReLU's dy * 0.f for dy < 0) sums to -0, an int64 reference says +0: the sign
    of a zero dbias is not compared.
Tier 2, bounded against float64 of the same float32 inputs:
    products   |got - ref| <= (K + 4) 2^-23 (|A| @ |B|) per element, K the reduction length: twice the any-order, fused-or-not bound
               gamma_{K+1} of a float32 sum of K products, plus the mask's (or the slope's) own rounding.  A dropped or doubled term
               is about sum|ab| / K: above the bound at every K here (orders at the short reductions, about twice at K = 4100, where
               tier 1 on the same shapes is exact).  Where a bias joins the sum it joins |A| @ |B| and K.
    BatchNorm  the bounds tests/test_gpu_deconv.py::test_small_sequential_vs_torch holds: y rtol 2e-4 / atol 2e-5; gradients within
               2e-3 of their scale + 1e-6; running buffers (and the saved mean | invstd) rtol 1e-5 / atol 1e-6.  dbias in bn_mode 1
               is analytically zero: it is held, as there, below 1e-4 of the weight gradient's scale.
Tier 3, routes: a recording proxy around _lib.lib() says which entry point a wrapper called (or that it called none), and the result
    equals the direct ABI call bit for bit, or torch's own expression where the route is torch.  Products on this tier use integer
    operands, so that pdgn_skinny_nn's atomics cannot make two runs differ."""
import copy

import numpy as np
import pytest
import torch

import persample_cases as pc
import persample_worker as pw
from persample_worker import bits, twice

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def _id(case):
    return case.name if hasattr(case, "name") else "-".join(map(str, case))


def same_bits(got, want, what=""):
    np.testing.assert_array_equal(np.asarray(got), bits(want).reshape(np.shape(got)), err_msg=what)


def f32(b):
    return np.asarray(b).view(F32)


def within(got_bits, ref, bound, what):
    """|got - ref| <= bound per element; prints the largest ratio."""
    err = np.abs(f32(got_bits).astype(F64).reshape(np.shape(ref)) - ref)
    assert np.isfinite(err).all(), what
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("%s: largest |got - ref| / bound = %.3f" % (what, ratio))
    assert (err <= bound).all(), "%s: %.3f of the bound" % (what, ratio)


def close(got_bits, ref, rtol, atol, what):
    got = f32(got_bits).astype(F64).reshape(np.shape(ref))
    err = np.abs(got - ref)
    print("%s: max |got - ref| = %.3e (largest |ref| %.3e)" % (what, err.max() if err.size else 0.0, np.abs(ref).max() if err.size else 0.0))
    assert np.isfinite(got).all() and (err <= atol + rtol * np.abs(ref)).all(), what


def of_scale(got_bits, ref, what):
    """Gradients: within 2e-3 of their scale + 1e-6."""
    got = f32(got_bits).astype(F64).reshape(np.shape(ref))
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print("%s: max |got - ref| = %.3e, scale %.3e" % (what, err, scale))
    assert np.isfinite(got).all() and err <= 2e-3 * scale + 1e-6, what


# ---------------------------------------------------------------------------- tiers 1 and 2: csrc/skinny.hip
@pytest.mark.parametrize("case", pc.NT_CASES, ids=_id)
def test_persample_nt(case):
    o = pc.nt_operands(case)
    got = twice(pw.call_nt, o["A"], o["B"], o["bias"], case.pads, case.act, case.entry)["C"]
    if case.data == "int":
        same_bits(got, o["want"])
    else:
        within(got, o["ref"], (case.K + 4 + int(case.bias)) * pc.U * o["mag"], "nt " + case.name)


@pytest.mark.parametrize("case", pc.NN_CASES, ids=_id)
def test_persample_nn_and_nn_masked(case):
    o = pc.nn_operands(case)
    repeatable = case.data == "int" or pc.nn_launch(case.R, case.N, case.K)["single"]
    run = twice if repeatable else (lambda fn, *a: fn(*a))           # several K slices of random data: fp32 atomics, any order
    got = run(pw.call_nn, o["A"], o["B"], o["P"], case.pads, case.act)["C"]
    if case.data == "int":
        same_bits(got, o["want"])
    else:
        within(got, o["ref"], (case.K + 4) * pc.U * o["mag"], "nn " + case.name)


@pytest.mark.parametrize("case", pc.TN_CASES, ids=_id)
def test_persample_tn(case):
    o = pc.tn_operands(case)
    got = twice(pw.call_tn, o["A"], o["B"], case.pads)["C"]
    if case.data == "int":
        same_bits(got, o["want"])
    else:
        within(got, o["ref"], (case.R + 4) * pc.U * o["mag"], "tn " + case.name)


def test_persample_row_padding_changes_no_row():
    """Rows 0 .. 34 of an nt call with R = 35 equal those of the call with R = 64; a tn call with R = 35 equals the call with R = 64
    whose extra rows are zero.  Random data, bit for bit."""
    rng = np.random.default_rng(35)
    A, B, bias = (rng.standard_normal(s).astype(F32) for s in ((64, 68), (20, 68), (20,)))
    short = pw.call_nt(A[:35], B, bias, (4, 4, 1), 2, "act")["C"]
    full = pw.call_nt(A, B, bias, (4, 4, 1), 2, "act")["C"]
    np.testing.assert_array_equal(short, full[:35])
    G, X = rng.standard_normal((64, 65)).astype(F32), rng.standard_normal((64, 40)).astype(F32)
    G[35:], X[35:] = 0.0, 0.0
    np.testing.assert_array_equal(pw.call_tn(G[:35], X[:35], (1, 2, 3))["C"], pw.call_tn(G, X, (1, 2, 3))["C"])


# ---------------------------------------------------------------------------- tiers 1 and 2: csrc/small_mlp.hip
MODE0 = [c for c in pc.SM_CASES if c.bn == 0]
BN = [c for c in pc.SM_CASES if c.bn]
FOUR = ("dgamma", "dbeta", "dbias", "dW")


@pytest.mark.parametrize("case", MODE0, ids=_id)
def test_persample_small_mlp_forward_without_batchnorm(case):
    o = pc.sm_operands(case)
    args = (case.act, 0, pc.EPS, pc.MOMENTUM, o["x"], o["W"], o["bias"], None, None, None, None)
    got = twice(pw.call_sm_forward, *args)
    if case.data == "int":
        same_bits(got["pre"], o["want_pre"], "pre")
        same_bits(got["y"], o["want_y"], "y")
    else:
        bound = (case.K + 4 + int(case.bias)) * pc.U * o["mag_pre"]
        within(got["pre"], o["ref"]["pre"], bound, "pre " + case.name)
        within(got["y"], o["ref"]["y"], bound, "y " + case.name)
    bare = pw.call_sm_forward(*args, saved=False)                     # pre = stat = NULL
    assert bare["pre"] is None and np.array_equal(bare["y"], got["y"])


@pytest.mark.parametrize("case", MODE0, ids=_id)
def test_persample_small_mlp_backward_without_batchnorm(case):
    """pre handed as y, as SkinnyLinearAct does (the activation's derivative is read off the sign)."""
    o = pc.sm_operands(case)
    y = o["want_y"] if case.data == "int" else pc.act_f32(o["ref"]["pre"].astype(F32), case.act)
    got = twice(pw.call_sm_backward, case.act, 0, o["x"], o["dy"], y, None, None, None)
    assert got["dgamma"] is None and got["dbeta"] is None
    if case.data == "int":
        same_bits(got["dpre"], o["want_dpre"], "dpre")
        if o["exact_sums"]:
            same_bits(bits(f32(got["dbias"]) + F32(0)), o["want_dbias"], "dbias")      # (-0 + 0 = +0: the zero's sign is open)
            same_bits(got["dW"], o["want_dW"], "dW")
        else:                                                        # LeakyReLU: dpre = dy * 0.01f is rounded, its sums are bounded
            within(got["dbias"], o["ref_dbias"], (case.R + 4) * pc.U * o["mag_dbias"], "dbias " + case.name)
            within(got["dW"], o["ref_dW"], (case.R + 4) * pc.U * o["mag_dW"], "dW " + case.name)
    else:
        within(got["dpre"], o["ref"]["dpre"], pc.U * np.abs(o["ref"]["dpre"]), "dpre " + case.name)
        within(got["dbias"], o["ref"]["dbias"], (case.R + 4) * pc.U * o["mag_dbias"], "dbias " + case.name)
        within(got["dW"], o["ref"]["dW"], (case.R + 4) * pc.U * o["mag_dW"], "dW " + case.name)
    for nulls in (("dW",), ("dbias",), ("dW", "dbias")):
        part = pw.call_sm_backward(case.act, 0, o["x"], o["dy"], y, None, None, None, nulls=nulls)
        for k in ("dpre", "dbias", "dW"):
            assert (part[k] is None) if k in nulls else np.array_equal(part[k], got[k]), (nulls, k)


@pytest.mark.parametrize("case", BN, ids=_id)
def test_persample_small_mlp_forward_with_batchnorm(case):
    """R == 1 in bn_mode 1: variance 0, and running_var takes the biased variance (include/pdgn_hip.h)."""
    o = pc.sm_operands(case)
    ref = o["ref"]
    args = (case.act, case.bn, pc.EPS, pc.MOMENTUM, o["x"], o["W"], o["bias"], o["gamma"], o["beta"], o["rm"], o["rv"])
    got = twice(pw.call_sm_forward, *args)
    same_bits(got["pre"], ref["pre"], "pre (an exact integer)")
    close(got["y"], ref["y"], 2e-4, 2e-5, "y " + case.name)
    close(got["stat"], ref["stat"], 1e-5, 1e-6, "mean | invstd " + case.name)
    if case.bn == 1 and case.running:
        close(got["rm"], ref["rm"], 1e-5, 1e-6, "running_mean " + case.name)
        close(got["rv"], ref["rv"], 1e-5, 1e-6, "running_var " + case.name)
    elif case.running:                                               # bn_mode 2 reads them
        same_bits(got["rm"], o["rm"])
        same_bits(got["rv"], o["rv"])
    bare = pw.call_sm_forward(*args, saved=False)
    assert bare["pre"] is None and bare["stat"] is None
    for k in ("y", "rm", "rv"):
        assert (bare[k] is None and got[k] is None) or np.array_equal(bare[k], got[k]), k


@pytest.mark.parametrize("case", BN, ids=_id)
def test_persample_small_mlp_backward_with_batchnorm(case):
    o = pc.sm_operands(case)
    ref = o["ref"]
    args = (case.act, case.bn, o["x"], o["dy"], ref["pre"].astype(F32), ref["stat"].astype(F32), o["gamma"], o["beta"])
    got = twice(pw.call_sm_backward, *args)
    for k in ("dpre", "dgamma", "dbeta", "dW"):
        of_scale(got[k], ref[k], "%s %s" % (k, case.name))
    if case.bn == 1:                                                 # analytically zero
        worst = float(np.abs(f32(got["dbias"])).max())
        print("dbias %s: max |got| = %.3e, weight gradient's scale %.3e" % (case.name, worst, np.abs(ref["dW"]).max()))
        assert worst <= 1e-4 * np.abs(ref["dW"]).max()
    else:
        of_scale(got["dbias"], ref["dbias"], "dbias " + case.name)
    for nulls in [(n,) for n in FOUR] + [FOUR]:
        part = pw.call_sm_backward(*args, nulls=nulls)
        for k in ("dpre",) + FOUR:
            assert (part[k] is None) if k in nulls else np.array_equal(part[k], got[k]), (nulls, k)


@pytest.mark.parametrize("bn,act", [(0, 0), (0, 2), (1, 2), (1, 1), (2, 2)])
def test_persample_small_mlp_scalar_form_equals_vector_form(bn, act):
    """K = 20 (float4 loads) against K = 21 whose extra x column is zero and whose extra W column is arbitrary: the same FMA chain
    plus one fma(0, w, acc) -- pre, y, stat, dpre, dbias, dgamma, dbeta and dW[:, :20] bit for bit, on random data."""
    rng = np.random.default_rng(2021 + 3 * bn + act)
    R, N = 35, 9
    x, W = rng.standard_normal((R, 21)).astype(F32), rng.standard_normal((N, 21)).astype(F32)
    x[:, 20] = 0.0
    bias, gamma, beta, dy = (rng.standard_normal(s).astype(F32) for s in ((N,), (N,), (N,), (R, N)))
    rm, rv = (rng.uniform(-0.3, 0.3, N).astype(F32), rng.uniform(0.5, 2.0, N).astype(F32)) if bn else (None, None)
    g, b = (gamma, beta) if bn else (None, None)
    fwd = [pw.call_sm_forward(act, bn, pc.EPS, pc.MOMENTUM, np.ascontiguousarray(x[:, :k]), np.ascontiguousarray(W[:, :k]), bias, g, b, rm, rv)
           for k in (20, 21)]
    for k in ("pre", "y", "stat", "rm", "rv"):
        assert (fwd[0][k] is None and fwd[1][k] is None) or np.array_equal(fwd[0][k], fwd[1][k]), k
    pre, stat = f32(fwd[0]["pre"]), (f32(fwd[0]["stat"]) if bn else None)
    bwd = [pw.call_sm_backward(act, bn, np.ascontiguousarray(x[:, :k]), dy, pre, stat, g, b) for k in (20, 21)]
    for k in ("dpre", "dbias", "dgamma", "dbeta"):
        assert (bwd[0][k] is None and bwd[1][k] is None) or np.array_equal(bwd[0][k], bwd[1][k]), k
    np.testing.assert_array_equal(bwd[0]["dW"], bwd[1]["dW"][:, :20])
    assert (f32(bwd[1]["dW"][:, 20]) == 0).all()


@pytest.mark.parametrize("args", pc.REFUSED, ids=_id)
def test_persample_entry_points_refuse_what_they_document(args):
    entry, kind, want = args
    rc, untouched = pw.call_refused(entry, kind)
    assert rc == want and untouched


# ---------------------------------------------------------------------------- tier 3: the Python routes
OURS = ("pdgn_skinny_nt", "pdgn_skinny_nt_act", "pdgn_skinny_nn", "pdgn_skinny_nn_masked", "pdgn_skinny_tn", "pdgn_small_mlp_forward",
        "pdgn_small_mlp_backward")


@pytest.fixture
def calls(monkeypatch):
    """[(entry point, its scalar arguments)] of every call a wrapper makes into the per-sample kernels."""
    from pdgn_amd import _lib
    real, seen = _lib.lib(), []

    class Recording:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in OURS:
                return fn

            def recorded(*a):
                seen.append((name, tuple(v for v in a if isinstance(v, (int, float)))))
                return fn(*a)
            return recorded
    monkeypatch.setattr(_lib, "lib", lambda: Recording())
    return seen


def names(calls):
    return [c[0] for c in calls]


def ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-7, 8, shape, generator=g).float().cuda()


def direct(entry, *args):
    from pdgn_amd import _lib
    L = _lib._lib or _lib.lib()                                      # (the loaded handle itself: never the recording proxy)
    rc = getattr(L, entry)(*[_lib.ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args], _lib.stream_of(torch.empty(1, device="cuda")))
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()


def direct_nt(a, w, bias=None):
    out = torch.empty(a.shape[0], w.shape[0], device="cuda")
    direct("pdgn_skinny_nt", a.shape[0], w.shape[0], a.shape[1], a, a.stride(0), w, w.stride(0), bias, out, out.stride(0))
    return out


def direct_nn(a, w, pre=None, act=0):
    out = torch.zeros(a.shape[0], w.shape[1], device="cuda")
    R, K, N = a.shape[0], a.shape[1], w.shape[1]
    if pre is None:
        direct("pdgn_skinny_nn", R, N, K, a, a.stride(0), w, w.stride(0), out, N)
    else:
        direct("pdgn_skinny_nn_masked", R, N, K, a, a.stride(0), pre, pre.stride(0), act, w, w.stride(0), out, N)
    return out


def direct_tn(a, b):
    out = torch.empty(a.shape[1], b.shape[1], device="cuda")
    direct("pdgn_skinny_tn", a.shape[0], a.shape[1], b.shape[1], a, a.stride(0), b, b.stride(0), out, out.stride(0))
    return out


@pytest.mark.parametrize("R", [64, 65])
def test_persample_route_rows(R, calls):
    """R <= 64 for every product wrapper: 64 rows on the kernel, 65 on torch."""
    from pdgn_amd import fused
    a, w, b = ints((R, 8), 1), ints((16, 8), 2), ints((16,), 3)
    dy, wl = ints((R, 2048), 4), ints((2048, 8), 5)
    pre = ints((R, 16), 6)
    got = [fused.skinny_nt(a, w, b), fused.skinny_nn(dy, wl), fused.skinny_nn_masked(pre, pre, 2, w), fused.skinny_tn(pre, a)]
    if R == 64:
        assert names(calls) == ["pdgn_skinny_nt", "pdgn_skinny_nn", "pdgn_skinny_nn_masked", "pdgn_skinny_tn"]
        want = [direct_nt(a, w, b), direct_nn(dy, wl), direct_nn(pre, w, pre, 2), direct_tn(pre, a)]
    else:
        assert names(calls) == []
        want = [torch.addmm(b, a, w.t()), dy.matmul(wl), (pre * torch.where(pre > 0, 1.0, 0.01)).matmul(w), pre.t().matmul(a)]
    for g_, w_ in zip(got, want):
        assert torch.equal(g_, w_)


@pytest.mark.parametrize("K", [2047, 2048])
def test_persample_route_nn_reduction_length(K, calls):
    from pdgn_amd import fused
    assert fused._SK_NN_MIN_K == 2048
    a, w = ints((35, K), K), ints((K, 64), K + 1)
    got = fused.skinny_nn(a, w)
    if K == 2048:
        assert names(calls) == ["pdgn_skinny_nn"] and torch.equal(got, direct_nn(a, w))
    else:
        assert names(calls) == [] and torch.equal(got, a.matmul(w))
    np.testing.assert_array_equal(got.cpu().numpy(), (a.cpu().double() @ w.cpu().double()).float().numpy())


def test_persample_route_multiples_of_four_and_alignment(calls):
    """K % 4 (nt, nn_masked), N % 4 (nn, nn_masked), a weight slice that starts one column in (pointer 4 bytes off 16) and a pitch
    not divisible by 4: every one goes to torch, and says what torch says."""
    from pdgn_amd import fused
    a6, w6 = ints((35, 6), 1), ints((16, 6), 2)
    assert torch.equal(fused.skinny_nt(a6, w6), a6.matmul(w6.t()))
    dy, w_n6 = ints((35, 2048), 3), ints((2048, 6), 4)
    assert torch.equal(fused.skinny_nn(dy, w_n6), dy.matmul(w_n6))
    pre6, pre16 = ints((35, 6), 5), ints((35, 16), 6)
    mask = lambda p, s: torch.where(p > 0, 1.0, s)                   # noqa: E731
    assert torch.equal(fused.skinny_nn_masked(pre6, pre6, 1, ints((6, 16), 7)), (pre6 * mask(pre6, 0.0)).matmul(ints((6, 16), 7)))
    assert torch.equal(fused.skinny_nn_masked(pre16, pre16, 2, w6), (pre16 * mask(pre16, 0.01)).matmul(w6))
    a8 = ints((35, 8), 8)
    wide = ints((16, 12), 9)
    off = wide[:, 1:9]                                               # pitch 12, pointer 4 bytes in
    assert off.data_ptr() % 16 == 4 and torch.equal(fused.skinny_nt(a8, off), a8.matmul(off.t()))
    odd = ints((16, 9), 10)[:, :8]                                   # pitch 9
    assert odd.stride(0) == 9 and torch.equal(fused.skinny_nt(a8, odd), a8.matmul(odd.t()))
    assert names(calls) == []
    ok = wide[:, 4:12]                                               # the aligned slice of the same weight: the kernel
    assert torch.equal(fused.skinny_nt(a8, ok), direct_nt(a8, ok)) and names(calls) == ["pdgn_skinny_nt"]


def test_persample_route_tn_into_a_column_slice(calls):
    from pdgn_amd import fused
    dy, x = ints((35, 17), 1), ints((35, 8), 2)
    target = torch.full((17, 13), float("nan"), device="cuda")
    out = fused.skinny_tn(dy, x, out=target[:, :8])
    assert names(calls) == ["pdgn_skinny_tn"] and calls[0][1][-1] == 13
    assert torch.equal(out, direct_tn(dy, x)) and torch.isnan(target[:, 8:]).all()


@pytest.mark.parametrize("N", [16, 2048])
def test_persample_route_skinny_linear(N, calls):
    """skinny_linear: forward on pdgn_skinny_nt, dW on pdgn_skinny_tn.  Its dx = dy W reduces over the N outputs and goes to torch
    below _SK_NN_MIN_K = 2048: at N = 16 that dx is no kernel coverage."""
    from pdgn_amd import fused
    x, w, dy = ints((35, 8), 1).requires_grad_(True), ints((N, 8), 2).requires_grad_(True), ints((35, N), 3)
    y = fused.skinny_linear(x, w)
    y.backward(dy)
    assert names(calls) == ["pdgn_skinny_nt"] + (["pdgn_skinny_nn"] if N >= 2048 else []) + ["pdgn_skinny_tn"]
    xd, wd = x.detach(), w.detach()
    assert torch.equal(y.detach(), direct_nt(xd, wd)) and torch.equal(w.grad, direct_tn(dy, xd))
    assert torch.equal(x.grad, direct_nn(dy, wd) if N >= 2048 else dy.matmul(wd))
    calls.clear()
    x65 = ints((65, 8), 4)
    assert torch.equal(fused.skinny_linear(x65, wd), torch.nn.functional.linear(x65, wd)) and names(calls) == []


def _sequential(dims, bn=None, act="leaky", seed=0):
    import torch.nn as nn
    torch.manual_seed(seed)
    layers = []
    for a, b in zip(dims[:-1], dims[1:]):
        layers.append(nn.Linear(a, b))
        if bn is not None:
            layers.append(nn.BatchNorm1d(b, **bn))
        if act is not None:
            layers.append({"leaky": nn.LeakyReLU(inplace=True), "relu": nn.ReLU(inplace=True), "leaky02": nn.LeakyReLU(0.2)}[act])
    seq = nn.Sequential(*layers).cuda()
    with torch.no_grad():
        for m in seq:
            if isinstance(m, nn.BatchNorm1d):
                if m.affine:
                    m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.5, 0.5)
                if m.track_running_stats:
                    m.running_mean.uniform_(-0.3, 0.3); m.running_var.uniform_(0.5, 2.0)
    return seq


def _both(seq, R, training=True, frozen=False, seed=1):
    """small_sequential on a copy of `seq` and torch on `seq` itself, forward and backward -> (mine, ya, xa, yb, xb)."""
    from pdgn_amd import fused
    mine = copy.deepcopy(seq)
    seq.train(training); mine.train(training)
    for m in (seq, mine):
        for p in m.parameters():
            p.requires_grad_(not frozen)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(R, seq[0].in_features, device="cuda", generator=g)
    t = torch.randn(R, [m for m in seq if hasattr(m, "out_features")][-1].out_features, device="cuda", generator=g)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = fused.small_sequential(mine, xa, training)
    fused.flush_bn_counters()
    yb = seq(xb)
    (ya * t).sum().backward()
    (yb * t).sum().backward()
    return mine, ya.detach(), xa, yb.detach(), xb


def _agree(mine, ya, xa, seq, yb, xb, frozen=False):
    """test_small_sequential_vs_torch's bounds."""
    torch.testing.assert_close(ya, yb, rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=2e-3, atol=2e-5)
    if not frozen:
        BatchNorm = torch.nn.BatchNorm1d
        wscale = max(p.grad.abs().max().item() for n, p in seq.named_parameters() if n.endswith("weight"))
        for (n1, p1), (n2, p2) in zip(mine.named_parameters(), seq.named_parameters()):
            i = int(n1.split(".")[0])
            j = i + 2 if isinstance(seq[i], BatchNorm) and i + 1 < len(seq) and isinstance(seq[i + 1], torch.nn.Linear) else i + 1
            nxt = seq[j] if j < len(seq) else None
            if n1.endswith(".bias") and isinstance(nxt, BatchNorm) and (nxt.training or not nxt.track_running_stats):
                # a per-channel constant in front of batch statistics (a Linear's bias; a BatchNorm's beta with nothing but a Linear
                # behind it): analytically zero, both sides hold rounding residue
                assert p1.grad.abs().max().item() <= 1e-4 * wscale and p2.grad.abs().max().item() <= 1e-4 * wscale, n1
                continue
            scale = max(p2.grad.abs().max().item(), 1e-6)
            assert (p1.grad - p2.grad).abs().max().item() <= 2e-3 * scale + 1e-6, n1
    for (n1, b1), (n2, b2) in zip(mine.named_buffers(), seq.named_buffers()):
        torch.testing.assert_close(b1.float(), b2.float(), rtol=1e-5, atol=1e-6, msg=n1)


@pytest.mark.parametrize("R,K,fused_", [(64, 632, True), (64, 636, False), (35, 1024, True), (35, 1028, False), (65, 20, False)])
def test_persample_route_small_sequential_size_limits(R, K, fused_, calls):
    """The LDS condition (R (K + 4) 4 + 1024 <= 160 KiB) and in_features <= 1024, on both sides; 65 rows."""
    seq = _sequential((K, 16), bn={})
    mine, ya, xa, yb, xb = _both(seq, R)
    if fused_:
        assert names(calls) == ["pdgn_small_mlp_forward", "pdgn_small_mlp_backward"]
        assert calls[0][1][:5] == (R, K, 16, 2, 1)
        _agree(mine, ya, xa, seq, yb, xb)
    else:
        assert names(calls) == [] and torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    assert int(mine[1].num_batches_tracked) == 1 == int(seq[1].num_batches_tracked)


@pytest.mark.parametrize("act,code", [("relu", 1), ("leaky", 2), (None, 0), ("leaky02", None)])
@pytest.mark.parametrize("training", [True, False])
def test_persample_route_small_sequential_activations(act, code, training, calls):
    """ReLU, LeakyReLU(0.01) and no activation are fused; LeakyReLU(0.2) is torch's.  Eval mode: bn_mode 2, counter untouched."""
    seq = _sequential((20, 12, 8), bn={}, act=act)
    mine, ya, xa, yb, xb = _both(seq, 35, training=training)
    if code is None:
        assert names(calls) == [] and torch.equal(ya, yb)
    else:
        assert names(calls) == ["pdgn_small_mlp_forward"] * 2 + ["pdgn_small_mlp_backward"] * 2
        assert [c[1][3:5] for c in calls] == [(code, 1 if training else 2)] * 4
        _agree(mine, ya, xa, seq, yb, xb)
    assert int(mine[1].num_batches_tracked) == int(seq[1].num_batches_tracked) == int(training)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("K,N", [(6, 8), (8, 12)])
def test_persample_route_linear_without_batchnorm(K, N, frozen, calls):
    """in_features % 4 != 0: SmallLinearBNAct with bn_mode 0 (the scalar form of small_mlp.hip); % 4 == 0: SkinnyLinearAct
    (pdgn_skinny_nt_act).  Frozen parameters: the input gradient alone, pdgn_skinny_nn_masked where its shape allows
    (in_features % 4 == 0 and out_features % 4 == 0), torch's expression of the same product elsewhere."""
    seq = _sequential((K, N), bn=None)
    mine, ya, xa, yb, xb = _both(seq, 35, frozen=frozen)
    fwd = "pdgn_small_mlp_forward" if K % 4 else "pdgn_skinny_nt_act"
    if frozen:
        assert names(calls) == [fwd] + ([] if K % 4 else ["pdgn_skinny_nn_masked"])
    else:
        assert names(calls) == [fwd, "pdgn_small_mlp_backward"]
    if K % 4:
        assert calls[0][1][:5] == (35, K, N, 2, 0)
    _agree(mine, ya, xa, seq, yb, xb, frozen)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("bn", [dict(track_running_stats=False), dict(affine=False), dict(affine=False, track_running_stats=False)], ids=str)
def test_persample_route_small_sequential_batchnorm_variants(bn, frozen, calls):
    """track_running_stats=False (batch statistics, no buffers, in either mode) and affine=False (gamma / beta NULL).  Frozen Linear
    parameters with affine=False: the backward still goes through the normalisation (pdgn_small_mlp_backward), and the input
    gradient matches a float64 run of the same modules."""
    seq = _sequential((20, 9), bn=bn, act="relu")
    ref64 = copy.deepcopy(seq).double()
    mine, ya, xa, yb, xb = _both(seq, 35, frozen=frozen)
    g = torch.Generator(device="cuda").manual_seed(1)                # (_both's draw)
    x = torch.randn(35, 20, device="cuda", generator=g)
    t = torch.randn(35, 9, device="cuda", generator=g)
    x64 = x.double().requires_grad_(True)
    ref64.train()
    (ref64(x64) * t.double()).sum().backward()
    err, scale = (xa.grad.double() - x64.grad).abs().max().item(), x64.grad.abs().max().item()
    print("dx against float64: max |difference| %.3e, scale %.3e" % (err, scale))
    assert err <= 2e-3 * scale + 1e-6
    _agree(mine, ya, xa, seq, yb, xb, frozen)
    assert names(calls) == ["pdgn_small_mlp_forward", "pdgn_small_mlp_backward"]
    assert calls[0][1][:5] == (35, 20, 9, 1, 1)


def test_persample_route_momentum_none_is_left_to_torch(calls):
    """BatchNorm1d(momentum=None) is a cumulative average: no fused launch takes a fixed factor for it; the running buffers are
    torch's after two steps."""
    from pdgn_amd import fused
    seq = _sequential((20, 9), bn=dict(momentum=None))
    mine = copy.deepcopy(seq)
    for step in range(2):
        x = torch.randn(35, 20, device="cuda", generator=torch.Generator(device="cuda").manual_seed(step))
        ya, yb = fused.small_sequential(mine, x, True), seq(x)
        fused.flush_bn_counters()
        assert torch.equal(ya, yb)
    assert names(calls) == []
    for (n1, b1), (n2, b2) in zip(mine.named_buffers(), seq.named_buffers()):
        assert torch.equal(b1, b2), n1
    assert int(mine[1].num_batches_tracked) == 2


def test_persample_route_small_sequential_equals_its_entry_point(calls):
    """One fused group against the direct call of pdgn_small_mlp_forward on the same operands: y and the running buffers bit for bit."""
    from pdgn_amd import fused
    seq = _sequential((21, 9), bn={})
    lin, bn = seq[0], seq[1]
    x = torch.randn(35, 21, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    y = torch.empty(35, 9, device="cuda")
    direct("pdgn_small_mlp_forward", 35, 21, 9, 2, 1, bn.eps, bn.momentum, x, lin.weight.detach(), lin.bias.detach(), bn.weight.detach(),
           bn.bias.detach(), rm, rv, y, None, None)
    with torch.no_grad():
        got = fused.small_sequential(seq, x, True)
    fused.flush_bn_counters()
    assert names(calls) == ["pdgn_small_mlp_forward"]
    assert torch.equal(got, y) and torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv)
    assert int(bn.num_batches_tracked) == 1


def test_persample_route_head_mlp(calls):
    """HeadMLP at B = 3, M = 16, nc = 8, Fo = 4: the per-sample row on pdgn_skinny_nt (W0[:, :nc]: a column slice, pitch nc + Fo),
    dW0[:, :nc] on pdgn_skinny_tn into its column slice; dg = drb W0[:, :nc] reduces over 256 < _SK_NN_MIN_K and is torch's.  Each
    against the direct call on the operands the function handed over."""
    from pdgn_amd import fused
    B, M, nc, Fo = 3, 16, 8, 4
    x, g = ints((B * M, Fo), 1).requires_grad_(True), ints((B, nc), 2).requires_grad_(True)
    W0 = (ints((256, nc + Fo), 3) / 8).requires_grad_(True)
    b0, W2, b2 = ints((256,), 4).requires_grad_(True), (ints((64, 256), 5) / 64).requires_grad_(True), ints((64,), 6).requires_grad_(True)
    W3, b3 = (ints((3, 64), 7) / 8).requires_grad_(True), ints((3,), 8).requires_grad_(True)
    seen = {}
    real_nt, real_tn = fused.skinny_nt, fused.skinny_tn

    def nt(a, w, bias=None):
        seen["nt"] = (a, w, bias, real_nt(a, w, bias))
        return seen["nt"][3]

    def tn(a, b, out=None):
        res = real_tn(a, b, out=out)
        seen["tn"] = (a, b, res.clone())
        return res
    fused.skinny_nt, fused.skinny_tn = nt, tn
    try:
        p = fused.HeadMLP.apply(x, g, W0, b0, W2, b2, W3, b3, B)
        p.backward(ints((B * M, 3), 9))
    finally:
        fused.skinny_nt, fused.skinny_tn = real_nt, real_tn
    assert names(calls) == ["pdgn_skinny_nt", "pdgn_skinny_tn"]
    assert calls[0][1] == (B, 256, nc, nc, nc + Fo, 256) and calls[1][1] == (B, 256, nc, 256, nc, nc + Fo)
    a, w, bias, rb = seen["nt"]
    assert w.data_ptr() == W0.data_ptr() and torch.equal(rb, direct_nt(a, w.detach(), bias.detach()))
    drb, gg, dw = seen["tn"]
    assert torch.equal(dw, direct_tn(drb, gg)) and torch.equal(W0.grad[:, :nc], dw)
    assert torch.equal(g.grad, drb.matmul(W0.detach()[:, :nc]))
