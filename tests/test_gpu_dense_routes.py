"""fused.linear_cl against the C ABI it dispatches to, in every cell of its route decision (fused.dense_route): planes on three
parts, two-part planes on the big tile and on the row-panel kernel, the thin kernels (k <= 4, n <= 4), the own NT kernel with and
without partials, torch below _OWN_MIN_ROWS -- each crossed with want_stats None / False / True and bias / addend where the cell has
them.  Every case first asks the read-only route which cell it is in; then

  forward    y, the BatchNorm partials and the block size handed on with them equal, bit for bit, the same product made by a direct
             call of the cell's entry point with the documented arguments (tail workspace set for the call: fixed-order sums);
  block size bn_act on the returned (partials, block rows) equals bn_act's own statistics pass over y;
  backward   dx equals, bit for bit, the direct call of the entry point the route names; dW and db an fp64 product within
             test_linear_cl_autograd's bound (the weight-gradient kernels sum with atomics: not repeatable bit for bit).

The shapes are the smallest that existing tests are known to drive down each route (test_gpu_deconv.py: test_linear_cl_autograd,
test_thin_layers, test_linear_cl_with_planes_equals_without, test_two_part_planes_on_the_big_tile_for_mid_size_products,
test_row_panel_kernel_of_the_short_reductions).

bn_act with against without partials: tests/test_gpu_bn.py compares that pair bit for bit on inputs whose sums are exact in any
order; on the random inputs here the two passes add in different orders, so the bound is the one the partials tests of
test_gpu_deconv.py hold against fp64 -- 1e-4 of the normalised (unit-variance) output -- which a wrong block size (every block's
row count, hence mean and variance, off by the ratio) misses by orders of magnitude."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

#        cell              M      N     K    planes  bias / addend allowed   partials when asked
CELLS = {"planes3":       (6000,  384,  256,  True,   True,  True,            True),
         "planes2_tile":  (17920, 256,  2560, True,   True,  True,            True),      # (the smallest of them whose partials' tile is 256 x 128)
         "planes2_panel": (4099,  4100, 128,  True,   False, False,           True),      # (the row-panel kernel: plain epilogue only)
         "thin_k":        (2049,  32,   3,    False,  True,  False,           True),      # (an addend sends a thin shape to the own kernel)
         "thin_n":        (5001,  3,    32,   False,  True,  False,           False),
         "own":           (5000,  20,   12,   False,  True,  True,            True),
         "own_padded":    (2048,  6,    3,    False,  True,  True,            False),     # n % 4 != 0: padded launch, no partials
         "torch":         (300,   64,   64,   False,  True,  True,            False)}
CASES = [(cell, stats, bias, addend) for cell, c in CELLS.items() for stats in (None, False, True)
         for bias in ((False, True) if c[4] else (False,)) for addend in ((False, True) if c[5] else (False,))]
IDS = ["%s-stats_%s%s%s" % (cell, stats, "-bias" if bias else "", "-addend" if addend else "") for cell, stats, bias, addend in CASES]


@functools.lru_cache(maxsize=None)
def _cell(cell):
    """The cell's operands and the fp64 gradients every one of its cases shares (dW = dy^T x and db = dy's column sums depend on
    neither bias, addend nor want_stats); made once, never written."""
    from pdgn_amd import fused
    M, N, K, with_planes = CELLS[cell][:4]
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    t = {"x": torch.randn(M, K, device="cuda", generator=g), "w": torch.randn(N, K, device="cuda", generator=g),
         "b": torch.randn(N, device="cuda", generator=g), "add": torch.randn(M, N, device="cuda", generator=g),
         "dy": torch.randn(M, N, device="cuda", generator=g)}
    t["planes"] = fused.split_planes(t["w"], True, rows=None if cell == "planes3" else M, dy_maxima_free=True, x_maxima_free=True) \
        if with_planes else None
    t["dw64"] = t["dy"].double().t() @ t["x"].double()
    t["db64"] = t["dy"].double().sum(0)
    return t


def _assert_in_cell(cell, route, planes, N, K, stats):
    from pdgn_amd import fused
    parts = planes.parts_p if planes is not None else 0
    want = {"planes3": ("planes", 3, False), "planes2_tile": ("planes", 2, True), "planes2_panel": ("planes", 2, False),
            "thin_k": ("thin", 0, False), "thin_n": ("thin", 0, False), "own": ("own", 0, False), "own_padded": ("own", 0, False),
            "torch": ("torch", 0, False)}[cell]
    assert (route.route, parts, route.x_maxima) == want, (cell, route, parts)
    assert {"thin_k": K <= 4, "thin_n": N <= 4, "own": N % 4 == 0, "own_padded": N % 4 != 0}.get(cell, True)
    assert route.stats is bool(stats and CELLS[cell][6]) and (route.block_rows > 0) == route.stats
    assert cell != "torch" or CELLS[cell][0] < fused._OWN_MIN_ROWS


def _pad4(c):
    return (c + 3) // 4 * 4


def _direct_planes(L, a, P, n, k, bias, addend, stats, hand_maxima):
    """pdgn_gemm_nt_ps as include/pdgn_hip.h documents it: the tail workspace and (two-part planes off the row-panel kernel) a's
    row maxima handed over for this one call."""
    from pdgn_amd import fused
    from pdgn_amd._lib import ptr, stream_of
    m, parts, plain = a.shape[0], P.shape[0], int(bias is None and addend is None)
    out = torch.empty(m, n, device="cuda")
    part = torch.empty(L.pdgn_gemm_nt_ps_stat_rows(m, n, k, parts, plain), 3 * n, device="cuda") if stats else None
    maxima = fused.operand_maxima(a) if hand_maxima else None
    ws = fused._tail_workspace(L, m, n, k, stats, a.device, parts=parts)
    if maxima is not None:
        assert L.pdgn_gemm_set_operand_scales(ptr(maxima), None) == 0
    assert L.pdgn_gemm_nt_ps(m, n, k, ptr(a), a.stride(0), ptr(P), P.shape[2], P.shape[1] * P.shape[2], parts, ptr(bias), ptr(addend),
                             addend.stride(0) if addend is not None else 0, ptr(out), n, ptr(part), None, 0, 1, 0, None, 0, stream_of(a)) == 0
    torch.cuda.synchronize()
    del ws
    return out, part, (L.pdgn_gemm_nt_ps_stat_block_rows(m, n, k, parts, plain) if stats else None)


def _direct_own(L, a, w, bias, addend, stats, transposed=False):
    """pdgn_gemm_nt (transposed: pdgn_gemm_nn, w as (k, n)) on operands zero-padded to multiples of 4 channels."""
    from pdgn_amd import fused
    from pdgn_amd._lib import ptr, stream_of
    pad = torch.nn.functional.pad
    m, k = a.shape
    n = w.shape[1] if transposed else w.shape[0]
    kp, np_ = _pad4(k), _pad4(n)
    ap = pad(a, (0, kp - k)).contiguous()
    wp = (pad(w, (0, np_ - n, 0, kp - k)) if transposed else pad(w, (0, kp - k, 0, np_ - n))).contiguous()
    b = pad(bias, (0, np_ - n)).contiguous() if bias is not None else None
    add = pad(addend, (0, np_ - n)).contiguous() if addend is not None else None
    out = torch.empty(m, np_, device="cuda")
    part = torch.empty(L.pdgn_gemm_nt_stat_rows(m, np_, kp), 3 * np_, device="cuda") if stats else None
    ws = fused._tail_workspace(L, m, np_, kp, stats, a.device)
    fn = L.pdgn_gemm_nn if transposed else L.pdgn_gemm_nt
    assert fn(m, np_, kp, ptr(ap), kp, ptr(wp), wp.stride(0), ptr(b), ptr(add), np_ if add is not None else 0, ptr(out), np_, ptr(part),
              stream_of(a)) == 0
    torch.cuda.synchronize()
    del ws
    return out[:, :n].contiguous(), part, (L.pdgn_gemm_nt_stat_block_rows(m, np_, kp) if stats else None)


def _direct_thin(L, a, w, wrs, wcs, n, bias, stats):
    from pdgn_amd._lib import ptr, stream_of
    m, k = a.shape
    out = torch.empty(m, n, device="cuda")
    part = torch.empty(L.pdgn_thin_stat_rows(m), 3 * n, device="cuda") if stats else None
    assert L.pdgn_thin_nt(m, n, k, ptr(a), a.stride(0), ptr(w), wrs, wcs, ptr(bias), ptr(out), n, ptr(part), stream_of(a)) == 0
    return out, part, (L.pdgn_thin_stat_block_rows() if stats else None)


def _direct_forward(L, cell, t, bias, addend, stats):
    N, K = t["w"].shape
    if cell.startswith("planes"):
        return _direct_planes(L, t["x"], t["planes"].p, N, K, bias, addend, stats, hand_maxima=cell == "planes2_tile")
    if cell.startswith("thin"):
        return _direct_thin(L, t["x"], t["w"], K, 1, N, bias, stats)
    if cell.startswith("own"):
        return _direct_own(L, t["x"], t["w"], bias, addend, stats)
    y = torch.nn.functional.linear(t["x"], t["w"], bias)
    return (y + addend if addend is not None else y), None, None


def _direct_input_gradient(L, cell, t):
    N, K = t["w"].shape
    if cell.startswith("planes"):                                # dX = dY (W^T)^T against the transposed planes
        return _direct_planes(L, t["dy"], t["planes"].t, K, N, None, None, False, hand_maxima=t["planes"].parts_t == 2)[0]
    if cell.startswith("thin"):                                  # W'[j, kk] = w[kk, j]
        return _direct_thin(L, t["dy"], t["w"], 1, K, K, None, False)[0]
    if cell.startswith("own"):
        return _direct_own(L, t["dy"], t["w"], None, None, False, transposed=True)[0]
    return t["dy"].matmul(t["w"])


def test_the_read_only_route_exists():
    """(The cases below ask it where it exists; a revision from before it -- where this file's bit-for-bit comparisons hold
    unchanged -- goes on unasked.)"""
    from pdgn_amd import fused
    assert callable(fused.dense_route)


@pytest.mark.parametrize("cell,stats,bias,addend", CASES, ids=IDS)
def test_every_cell_equals_its_entry_point_bit_for_bit(cell, stats, bias, addend):
    import torch.nn as nn
    from pdgn_amd import _lib, fused
    L = _lib.lib()
    _lib.set_gemm_mode("x2")                                     # (the default; the cells' planes belong to it)
    t = _cell(cell)
    M, N, K = CELLS[cell][:3]
    b, add = (t["b"] if bias else None), (t["add"] if addend else None)
    if hasattr(fused, "dense_route"):
        _assert_in_cell(cell, fused.dense_route(t["x"], t["w"], b, add, t["planes"], bool(stats)), t["planes"], N, K, stats)
    emits = bool(stats) and CELLS[cell][6]
    # forward
    leaves = [t["x"].clone().requires_grad_(True), t["w"].clone().requires_grad_(True), b.clone().requires_grad_(True) if bias else None,
              add.clone().requires_grad_(True) if addend else None]
    got = fused.linear_cl(leaves[0], leaves[1], leaves[2], leaves[3], want_stats=stats, planes=t["planes"])
    y, pair = (got, None) if stats is None else got
    assert stats is None or (isinstance(got, tuple) and len(got) == 2)
    want_y, want_part, want_block = _direct_forward(L, cell, t, b, add, emits)
    assert torch.equal(y.detach(), want_y)
    if emits:
        assert pair is not None and pair[1] == want_block and pair[0].shape == want_part.shape and torch.equal(pair[0], want_part)
        assert not pair[0].requires_grad
        # the block size, consumed: the partials' statistics are those of a pass over y
        bn_a, bn_b = nn.BatchNorm1d(N).cuda().train(), nn.BatchNorm1d(N).cuda().train()
        with torch.no_grad():
            out_a = fused.bn_act(y.detach(), bn_a, True, act="none", partials=pair)
            out_b = fused.bn_act(y.detach(), bn_b, True, act="none")
        err = (out_a - out_b).abs().max().item()
        print("bn_act with - without partials: max |difference| %.3e" % err)
        assert err <= 1e-4 * max(1.0, out_b.abs().max().item())
        np.testing.assert_allclose(bn_a.running_mean.cpu().numpy(), bn_b.running_mean.cpu().numpy(), rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(bn_a.running_var.cpu().numpy(), bn_b.running_var.cpu().numpy(), rtol=1e-4)
    else:
        assert pair is None
    # backward
    y.backward(t["dy"])
    assert torch.equal(leaves[0].grad, _direct_input_gradient(L, cell, t))
    sc = float(M) ** 0.5
    np.testing.assert_allclose(leaves[1].grad.cpu().numpy(), t["dw64"].cpu().numpy(), rtol=1e-4, atol=2e-4 * sc + 1e-6, err_msg="dw")
    if bias:
        np.testing.assert_allclose(leaves[2].grad.cpu().numpy(), t["db64"].cpu().numpy(), rtol=1e-4, atol=2e-4 * sc + 1e-6, err_msg="db")
    if addend:
        assert torch.equal(leaves[3].grad, t["dy"])


QUERIES = ("pdgn_gemm_nt_config", "pdgn_gemm_nt_ps_row_panel", "pdgn_gemm_nt_stat_block_rows", "pdgn_gemm_nt_ps_stat_block_rows",
           "pdgn_thin_stat_block_rows")


@pytest.mark.parametrize("cell,bias", [(c, b) for c in CELLS if c != "torch" for b in (False, True) if CELLS[c][4] or not b])
def test_the_launch_model_is_asked_each_question_once(cell, bias, monkeypatch):
    """One linear_cl(..., want_stats=True): no predicate of the library's launch model is called twice (host time on the step's
    critical path, ~300 dense calls per step) -- and the route comes from those answers alone."""
    from pdgn_amd import _lib, fused
    real = _lib.lib()
    _lib.set_gemm_mode("x2")
    t = _cell(cell)
    calls = {}

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in QUERIES:
                return fn

            def counted(*args):
                calls[name] = calls.get(name, 0) + 1
                return fn(*args)
            return counted
    monkeypatch.setattr(_lib, "lib", lambda: Counting())
    y, pair = fused.linear_cl(t["x"], t["w"], t["b"] if bias else None, None, want_stats=True, planes=t["planes"])
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert (pair is not None) == CELLS[cell][6]
    assert all(n == 1 for n in calls.values()), calls
    assert (len(calls) > 0) == CELLS[cell][6], calls
