"""The BatchNorm op layer of pdgn_amd.fused (bn_act, bn_softmax_slots_permute, bilateral_weighting, bn_act_maxpool, small_sequential) at the
smallest shapes that reach each of its branches.  Per wrapper and branch:
  (a) the ordered C-ABI entry points of the forward and of the backward, against a literal list (a recording proxy around _lib.lib(), as
      tests/test_gpu_persample.py uses for its routes; size queries are entry points too);
  (b) num_batches_tracked after flush_bn_counters(): one per BatchNorm per training forward, none in eval;
  (c) the gradients: finite, and equal to torch's composed ops within the bounds tests/test_gpu_deconv.py holds for the same op
      (bn_act / bn_act_maxpool: rtol 1e-4, atol 1e-4 max(1, |ref|); the softmax ops: dx / du rtol 2e-3, atol 2e-6, parameters rtol 2e-3,
      atol 1e-4; small_sequential: dx rtol 2e-3, atol 2e-5, parameters 2e-3 of their scale + 1e-6, the zero bias gradient 1e-4 of the
      weight gradient's scale)."""
import copy

import numpy as np
import pytest
import torch

from hashweights import fill_module
from torch_standins import bilateral_weighting_torch, bn_act_maxpool_torch, bn_act_torch, bn_softmax_slots_permute_torch

gpu = pytest.mark.gpu
STATS = ["pdgn_bn_scratch_floats", "pdgn_bn_stats"]                  # _bn_stats in training without partials
ADJOINT = ["pdgn_bn_scratch_floats", "pdgn_bn_act_backward"]         # the streaming adjoint


@pytest.fixture
def calls(monkeypatch):
    """The names of the entry points called since the last clear()."""
    from pdgn_amd import _lib
    real, seen = _lib.lib(), []

    class Recording:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def recorded(*a):
                seen.append(name)
                return fn(*a)
            return recorded
    monkeypatch.setattr(_lib, "lib", lambda: Recording())
    return seen


def taken(calls):
    got = list(calls)
    calls.clear()
    return got


def drive(calls, make_bn, x, run, grads_out, training, n_bn=1):
    """run(side, to, bns, x leaf) -> (y, other leaves) on the device (float32) and in torch (float64), then y.backward(grads_out).
    -> the device side's forward calls, its backward calls, per side [y, dx, the other leaves' gradients, (dgamma, dbeta) per BatchNorm],
    and the device side's modules."""
    rows = []
    for side, to in (("dev", lambda t: t.cuda()), ("ref", lambda t: t.double())):
        bns = [to(make_bn(i)).train(training) for i in range(n_bn)]
        xi = to(x).requires_grad_(True)
        taken(calls)
        y, leaves = run(side, to, bns, xi)
        first = taken(calls)
        y.backward(to(grads_out))
        second = taken(calls)
        if side == "dev":
            fwd, bwd, dev_bns = first, second, bns
        row = [y.detach(), xi.grad] + [t.grad for t in leaves] + [g for bn in bns for g in (bn.weight.grad, bn.bias.grad)]
        rows.append([t.detach().cpu().double().numpy() for t in row])
    return fwd, bwd, rows[0], rows[1], dev_bns


def counters(bns, training):
    from pdgn_amd.fused import flush_bn_counters
    flush_bn_counters()
    assert [int(bn.num_batches_tracked) for bn in bns] == [1 if training else 0] * len(bns)


def close_as_bn_act(got, ref, names):
    """tests/test_gpu_deconv.py::test_fused_bn_act_vs_torch's bound."""
    assert len(got) == len(ref) == len(names)
    for name, a, b in zip(names, got, ref):
        assert np.isfinite(a).all(), name
        print("%s: max |got - ref| = %.3e" % (name, np.abs(a - b).max()))
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(b).max()), err_msg=name)


def close_as_softmax_ops(got, ref, names):
    """tests/test_gpu_deconv.py::test_bn_softmax_slots_permute / test_bilateral_weighting's bounds: y, then inputs, then parameters."""
    assert len(got) == len(ref) == len(names)
    for name, a, b in zip(names, got, ref):
        assert np.isfinite(a).all(), name
        print("%s: max |got - ref| = %.3e" % (name, np.abs(a - b).max()))
        rtol, atol = (1e-4, 1e-6) if name == "y" else ((2e-3, 2e-6) if name in ("dx", "du") else (2e-3, 1e-4))
        np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=name)


def bn1d(C, salt):
    def make(i):
        bn = torch.nn.BatchNorm1d(C[i] if isinstance(C, (tuple, list)) else C)
        fill_module(bn, salt=salt + i)
        return bn
    return make


def normal(shape, seed, scale=1.0, shift=0.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale + shift).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- bn_act
@gpu
@pytest.mark.parametrize("training,mul,pre_bias", [(True, False, False), (False, False, False), (True, True, False), (True, False, True)],
                         ids=["train", "eval", "mul", "pre_bias"])
def test_bn_act(calls, training, mul, pre_bias):
    from pdgn_amd.fused import bn_act
    x, g = normal((32, 4), 1, 2.0, 0.7), normal((32, 4), 2)
    m, pb = normal((32, 4), 3), normal((4,), 4)

    def run(side, to, bns, xi):
        leaves = [to(t).requires_grad_(True) for t, on in ((m, mul), (pb, pre_bias)) if on]
        kw = dict(zip([n for n, on in (("mul", mul), ("pre_bias", pre_bias)) if on], leaves))
        return (bn_act if side == "dev" else bn_act_torch)(xi, bns[0], training, **kw), leaves
    fwd, bwd, got, ref, bns = drive(calls, bn1d(4, 2), x, run, g, training)
    assert fwd == (STATS if training else ["pdgn_bn_eval_stats"]) + ["pdgn_bn_act_forward"]
    assert bwd == ADJOINT
    counters(bns, training)
    close_as_bn_act(got, ref, ["y", "dx"] + ["dmul"] * mul + ["dpre_bias"] * pre_bias + ["dgamma", "dbeta"])


@gpu
@pytest.mark.parametrize("C,mul", [(8, False), (8, True), (6, False)], ids=["fused_store", "mul_delegates", "torch_path"])
def test_bn_act_interleaved(calls, C, mul):
    """B = 2, n = 8: the interleaving store of the apply pass itself (C = 8); with a product the wrapper hands the whole call to itself
    without the interleave and permutes behind it -- one forward, ONE tick; C = 6: torch's own ops, no entry point at all."""
    from pdgn_amd.fused import bn_act
    x, g, m = normal((16, C), 5, 1.5, -0.3), normal((32, C // 2), 6), normal((16, C), 7)

    def run(side, to, bns, xi):
        leaves = [to(m).requires_grad_(True)] if mul else []
        return (bn_act if side == "dev" else bn_act_torch)(xi, bns[0], True, act="relu", mul=leaves[0] if mul else None, interleave_n=8), leaves
    fwd, bwd, got, ref, bns = drive(calls, bn1d(C, 4), x, run, g, True)
    assert got[0].shape == (32, C // 2)
    assert fwd == ([] if C == 6 else STATS + ["pdgn_bn_act_forward"])
    assert bwd == ([] if C == 6 else ADJOINT)
    counters(bns, True)
    close_as_bn_act(got, ref, ["y", "dx"] + ["dmul"] * mul + ["dgamma", "dbeta"])


# ------------------------------------------------------------------------------------------------ the slot-softmax ops
def bn2d(C, seed):
    def make(i):
        ch = C[i] if isinstance(C, (tuple, list)) else C
        rng = np.random.default_rng(seed + i)
        bn = torch.nn.BatchNorm2d(ch)
        with torch.no_grad():
            bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, ch).astype(np.float32)))
            bn.bias.copy_(torch.from_numpy(rng.uniform(-0.5, 0.5, ch).astype(np.float32)))
            bn.running_mean.copy_(torch.from_numpy(rng.uniform(-0.2, 0.8, ch).astype(np.float32)))
            bn.running_var.copy_(torch.from_numpy(rng.uniform(2.0, 5.0, ch).astype(np.float32)))
        return bn
    return make


@gpu
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_bn_softmax_slots_permute(calls, training):
    from pdgn_amd.fused import bn_softmax_slots_permute
    M, k, C = 8, 4, 4
    x, g = normal((M * k, C), 8, 2.0, 0.5), normal((M, k // 2, 2 * C), 9)

    def run(side, to, bns, xi):
        return (bn_softmax_slots_permute if side == "dev" else bn_softmax_slots_permute_torch)(xi, bns[0], training, k), []
    fwd, bwd, got, ref, bns = drive(calls, bn2d(C, 10), x, run, g, training)
    assert fwd == (STATS if training else ["pdgn_bn_eval_stats"]) + ["pdgn_bn_softmax_slots_permute"]
    assert bwd == ["pdgn_softmax_slots_permute_backward"] + ADJOINT
    counters(bns, training)
    close_as_softmax_ops(got, ref, ["y", "dx", "dgamma", "dbeta"])


@gpu
@pytest.mark.parametrize("k,C,training", [(4, 4, True), (4, 4, False), (6, 4, True), (4, 6, True)],
                         ids=["fused_adjoint", "fused_adjoint_eval", "generic_chain", "delegates"])
def test_bilateral_weighting(calls, k, C, training):
    """k = 4: both adjoints in pdgn_bilateral_weighting_backward; k = 6: the chain adjoint(u, with the product) -> softmax adjoint ->
    adjoint(x); C = 6: the wrapper hands x to bn_softmax_slots_permute (torch's BatchNorm, then the softmax kernel) and u, 12 channels,
    to bn_act with the weights as its product -- each of the two ticks its own BatchNorm."""
    from pdgn_amd.fused import bilateral_weighting
    M = 8
    x, u = normal((M * k, C), 11, 2.0, 0.5), normal((M * k // 2, 2 * C), 12, 1.5, -0.2)
    g, pb = normal((M * k // 2, 2 * C), 13), normal((C,), 14)

    def run(side, to, bns, xi):
        ui = to(u).requires_grad_(True)
        fn = bilateral_weighting if side == "dev" else bilateral_weighting_torch
        return fn(xi, bns[0], ui, bns[1], training, k, pre_bias_x=to(pb) if training else None), [ui]
    fwd, bwd, got, ref, bns = drive(calls, bn2d((C, 2 * C), 15), x, run, g, training, n_bn=2)
    stats = STATS if training else ["pdgn_bn_eval_stats"]
    if C == 6:
        assert fwd == ["pdgn_softmax_slots_permute"] + stats + ["pdgn_bn_act_forward"]
        assert bwd == ADJOINT + ["pdgn_softmax_slots_permute_backward"]
    else:
        assert fwd == stats + stats + ["pdgn_bn_softmax_slots_permute_mul"]
        assert bwd == (["pdgn_bilateral_scratch_floats", "pdgn_bilateral_weighting_backward"] if k == 4 else
                       ADJOINT + ["pdgn_softmax_slots_permute_backward"] + ADJOINT)
    counters(bns, training)
    close_as_softmax_ops(got, ref, ["y", "dx", "du", "dgamma_x", "dbeta_x", "dgamma_u", "dbeta_u"])


# ---------------------------------------------------------------------------------------------------------- bn_act_maxpool
@gpu
@pytest.mark.parametrize("one_pass,training", [(True, True), (False, True), (True, False)], ids=["one_pass", "stats_then_max", "eval"])
def test_bn_act_maxpool(calls, monkeypatch, one_pass, training):
    from pdgn_amd import fused
    monkeypatch.setattr(fused, "_STATS_MAX", one_pass)
    B, N, C = 2, 16, 4
    x, g = normal((B * N, C), 16, 1.5, 0.3), normal((B, C), 17)

    def run(side, to, bns, xi):
        return (fused.bn_act_maxpool if side == "dev" else bn_act_maxpool_torch)(xi, bns[0], training, B, N), []
    fwd, bwd, got, ref, bns = drive(calls, bn1d(C, 5), x, run, g, training)
    if one_pass and training:
        assert fwd == ["pdgn_bn_stats_maxpool_scratch_floats", "pdgn_bn_stats_act_maxpool"]
    else:
        assert fwd == (STATS if training else ["pdgn_bn_eval_stats"]) + ["pdgn_bn_maxpool_scratch_floats", "pdgn_bn_act_maxpool"]
    assert bwd == ["pdgn_bn_act_maxpool_backward"]
    counters(bns, training)
    close_as_bn_act(got, ref, ["y", "dx", "dgamma", "dbeta"])


# -------------------------------------------------------------------------------------------------------- small_sequential
@gpu
@pytest.mark.parametrize("tracked,training", [(True, True), (True, False), (False, True), (False, False)],
                         ids=["tracked_train", "tracked_eval", "untracked_train", "untracked_eval"])
def test_small_sequential(calls, tracked, training):
    """R = 2, K = 4, N = 4: Linear + BatchNorm1d + LeakyReLU in one launch each way against the same nn.Sequential in torch, with the
    bounds of tests/test_gpu_deconv.py::test_small_sequential_vs_torch.  Without running statistics the layer normalises with
    the batch's in eval too, has no buffers to update and no counter."""
    import torch.nn as nn
    from pdgn_amd import fused
    torch.manual_seed(3)
    ref = nn.Sequential(nn.Linear(4, 4), nn.BatchNorm1d(4, track_running_stats=tracked), nn.LeakyReLU(inplace=True)).cuda()
    with torch.no_grad():
        ref[1].weight.uniform_(0.5, 1.5); ref[1].bias.uniform_(-0.5, 0.5)
        if tracked:
            ref[1].running_mean.uniform_(-0.3, 0.3); ref[1].running_var.uniform_(0.5, 2.0)
    mine = copy.deepcopy(ref)
    ref.train(training); mine.train(training)
    x = torch.randn(2, 4, device="cuda")
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    t = torch.randn(2, 4, device="cuda")
    taken(calls)
    ya = fused.small_sequential(mine, xa, training)
    assert taken(calls) == ["pdgn_small_mlp_forward"]
    yb = ref(xb)
    torch.testing.assert_close(ya, yb, rtol=2e-4, atol=2e-5)
    (ya * t).sum().backward()
    assert taken(calls) == ["pdgn_small_mlp_backward"]
    (yb * t).sum().backward()
    fused.flush_bn_counters()
    if tracked:
        assert int(mine[1].num_batches_tracked) == (1 if training else 0)
    else:
        assert mine[1].num_batches_tracked is None and mine[1].running_mean is None
    assert torch.isfinite(xa.grad).all()
    torch.testing.assert_close(xa.grad, xb.grad, rtol=2e-3, atol=2e-5)
    batch_stats = training or not tracked
    wscale = max(p.grad.abs().max().item() for n, p in ref.named_parameters() if n.endswith("weight"))
    for (n1, p1), (n2, p2) in zip(mine.named_parameters(), ref.named_parameters()):
        assert torch.isfinite(p1.grad).all(), n1
        if batch_stats and n1 == "0.bias":                        # in front of a BatchNorm on batch statistics: analytically zero
            assert p1.grad.abs().max().item() <= 1e-4 * wscale and p2.grad.abs().max().item() <= 1e-4 * wscale, n1
            continue
        scale = max(p2.grad.abs().max().item(), 1e-6)
        assert (p1.grad - p2.grad).abs().max().item() <= 2e-3 * scale + 1e-6, n1
    for (n1, b1), (n2, b2) in zip(mine.named_buffers(), ref.named_buffers()):
        torch.testing.assert_close(b1.float(), b2.float(), rtol=1e-5, atol=1e-6, msg=n1)


# ------------------------------------------------------------------------------------------------------- the record (host)
def test_bn_state_record():
    """bn_state: the module's buffers and the caller's flag; without running statistics null buffers and batch statistics, eval included."""
    from pdgn_amd.fused import BNState, bn_state
    bn = torch.nn.BatchNorm1d(4, momentum=0.25, eps=1e-3)
    for training in (True, False):
        st = bn_state(bn, training)
        assert isinstance(st, BNState) and st.running_mean is bn.running_mean and st.running_var is bn.running_var
        assert st.training is training and (st.momentum, st.eps) == (0.25, 1e-3)
    bn = torch.nn.BatchNorm2d(4, momentum=0.5, track_running_stats=False)
    for training in (True, False):
        assert bn_state(bn, training) == BNState(None, None, True, 0.5, bn.eps)
