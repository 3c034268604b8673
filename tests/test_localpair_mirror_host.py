"""The reference of tests/test_gpu_localpair.py checked on the host: tests/localpair_mirror.py against the float64 torch stand-ins
(tests/torch_standins.py) and their autograd, and its exactness guard on every lattice case the GPU module compares bit for bit."""
import os

import numpy as np
import pytest
import torch

import localpair_cases as lc
import localpair_mirror as lm
from torch_standins import chamfer_min_torch, local_stats_torch


@pytest.mark.parametrize("b,m,n,d", [(2, 70, 90, 3), (1, 33, 20, 9), (2, 5, 64, 16), (1, 1, 7, 1)])
def test_chamfer_mirror_equals_the_torch_standin_and_its_autograd(b, m, n, d):
    rng = np.random.default_rng(m * n + d)
    x, y = rng.standard_normal((b, m, d)), rng.standard_normal((b, n, d))
    gminx, gminy = rng.standard_normal((b, m)), rng.standard_normal((b, n))
    minx, argx, miny, argy = lm.chamfer(x, y)
    xt, yt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(y).requires_grad_(True)
    rx, ry = chamfer_min_torch(xt, yt)
    np.testing.assert_allclose(minx, rx.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(miny, ry.detach().numpy(), rtol=1e-12, atol=1e-12)
    P = lm.gram(x, y)
    assert np.array_equal(argx, torch.from_numpy(P).min(2)[1].numpy()) and np.array_equal(argy, torch.from_numpy(P).min(1)[1].numpy())
    ((rx * torch.from_numpy(gminx)).sum() + (ry * torch.from_numpy(gminy)).sum()).backward()
    gx, gy = lm.chamfer_grad(x, y, argx, argy, gminx, gminy)
    np.testing.assert_allclose(gx, xt.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gy, yt.grad.numpy(), rtol=1e-12, atol=1e-12)
    xt.grad, yt.grad = None, None
    rx, ry = chamfer_min_torch(xt, yt)
    ((rx.sum() + ry.sum()) * 0.25 * 3.0).backward()
    ux, uy = lm.chamfer_grad_uniform(x, y, argx, argy, 3.0, 0.25)
    np.testing.assert_allclose(ux, xt.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(uy, yt.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_chamfer_mirror_takes_the_first_index_on_ties_like_torch_min():
    x = np.zeros((1, 3, 2))
    y = np.array([[[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, -1.0]]])
    minx, argx, miny, argy = lm.chamfer(x, y)
    assert np.array_equal(argx, [[0, 0, 0]]) and np.array_equal(argy, [[0, 0, 0, 0]]) and np.array_equal(minx, [[1.0, 1.0, 1.0]])
    P = torch.from_numpy(lm.gram(x, y))
    assert np.array_equal(argx, P.min(2)[1].numpy()) and np.array_equal(argy, P.min(1)[1].numpy())
    # the adjoint follows those indices: all three queries pull on y[0] alone
    gx, gy = lm.chamfer_grad(x, y, argx, argy, np.ones((1, 3)), np.zeros((1, 4)))
    assert np.array_equal(gy, [[[6.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]]) and np.array_equal(gx, np.broadcast_to([-2.0, 0.0], (1, 3, 2)))


@pytest.mark.parametrize("b,n,m,K", [(2, 50, 30, 20), (1, 9, 40, 7), (3, 16, 1, 1), (1, 200, 17, 16)])
def test_local_stats_mirror_equals_the_torch_standin_and_its_autograd(b, n, m, K):
    rng = np.random.default_rng(n + m + K)
    xyz = rng.standard_normal((b, n, 3))
    idx = rng.integers(0, n, (b, m, K)).astype(np.int32)
    idx[:, 0, :] = idx[:, 0, :1]                                  # duplicate neighbours inside a query
    dmu, dcov = rng.standard_normal((b, m, 3)), rng.standard_normal((b, m, 9))
    xt = torch.from_numpy(xyz).requires_grad_(True)
    rmu, rcov = local_stats_torch(xt, torch.from_numpy(idx))
    mu, cov = lm.local_stats(xyz, idx)
    np.testing.assert_allclose(mu, rmu.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(cov, rcov.detach().numpy(), rtol=1e-12, atol=1e-12)
    ((rmu * torch.from_numpy(dmu)).sum() + (rcov * torch.from_numpy(dcov)).sum()).backward()
    np.testing.assert_allclose(lm.local_stats_grad(xyz, idx, dmu, dcov), xt.grad.numpy(), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("case", sorted(set(lc.CHAMFER_FORWARD + lc.CHAMFER_GRAD + [lc.WORKER_CASE])), ids=lambda c: "-".join(map(str, c)))
def test_guard_accepts_every_exact_chamfer_case(case):
    """chamfer_reference() runs assert_exact on the inputs, on P (through its worst sum of |terms|), and on both adjoints with the sum
    of |terms| at every destination; what it returns is what the GPU is compared with."""
    kind, bits, b, m, n, d = case
    ref = lc.chamfer_reference(case)
    assert ref["minx"].shape == (b, m) and ref["argy"].shape == (b, n) and ref["gx"].shape == (b, m, d) and ref["uy"].shape == (b, n, d)
    assert np.abs(ref["gminx"]).max() <= 2.0 and np.array_equal(ref["gminy"] * 4, np.rint(ref["gminy"] * 4))
    P = lm.gram(ref["x"], ref["y"])
    assert np.array_equal(P, P.astype(np.float32).astype(np.float64))     # the whole Gram matrix is float32, not its minima alone
    if kind == "same_y":
        assert not ref["argx"].any() and len(np.unique(ref["argy"])) == 1    # one hot row in either cloud
    if kind == "x_is_y":
        assert not ref["minx"].any() and not ref["miny"].any() and (ref["argx"] <= np.arange(m)).all() and (ref["argx"] < np.arange(m)).any()
    if kind.startswith("tie"):
        i0, i1 = (int(v) for v in kind[3:].split("_"))
        assert i0 // 1024 != i1 // 1024 and (ref["argx"][:, 64:128] == i0).all() and np.array_equal(ref["y"][:, i0], ref["y"][:, i1])
        assert not ref["minx"][:, 64:96].any() and (ref["minx"][:, 96:128] == 4.0 ** -bits).all()


def test_the_adjoint_shapes_straddle_the_lds_limit():
    """CHL_MAXF = 12288 floats of one cloud's gradient (csrc/localpair.hip): the adjoint's shapes come in pairs around it."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pdgn_amd", "csrc", "localpair.hip")) as f:
        src = f.read()
    assert "#define CHL_MAXF 12288 " in src and "#define CH_TILE 1024\n" in src and "#define CH_MAXD 16\n" in src
    assert "#define LP_LDS_FLOATS 8192 " in src and "#define LP_PTS_FLOATS 6144 " in src       # 2730 and 2048 points
    over = {c[2:] for c in lc.CHAMFER_OVER_LIMIT}
    assert over == {(2, 4097, 300, 3), (2, 1366, 1400, 9), (1, 769, 40, 16), (1, 200, 4097, 3), (1, 4097, 300, 3), (1, 4097, 1, 3)}
    under = [c for c in lc.CHAMFER_GRAD if c not in lc.CHAMFER_OVER_LIMIT]
    assert {max(c[3], c[4]) * c[5] for c in under} == {12288, 12285}                           # 4096 x 3, 768 x 16; 1365 x 9
    assert {max(c[3], c[4]) * c[5] for c in lc.CHAMFER_OVER_LIMIT} == {12291, 12304, 12600}


def test_the_lattice_cases_are_full_of_ties():
    """What makes the argmin comparison bite: minima attained at several distinct candidates."""
    for case, least in ((lc.CHAMFER_FORWARD[0], 0.3), (lc.CHAMFER_FORWARD[1], 0.01), (lc.CHAMFER_FORWARD[2], 0.01)):
        ref = lc.chamfer_reference(case)
        assert lc.tied_rows(ref["x"], ref["y"]) > least, case


@pytest.mark.parametrize("case", lc.STATS_EXACT, ids=lambda c: "-".join(map(str, c)))
def test_guard_accepts_every_exact_local_stats_case(case):
    b, n, m, K = case
    ref = lc.stats_reference(case)
    idx = ref["idx"]
    assert not (idx == n - 1).any() and not ref["dxyz"][:, n - 1].any()   # the unreferenced point
    assert (idx[:, ::2, 0] == 0).all()
    if m > 1:
        assert (idx[:, 1] == lc.SAME_POINT).all() and not ref["cov"][:, 1].any()
        assert np.array_equal(ref["mu"][:, 1], ref["xyz"][:, lc.SAME_POINT])
    if K == 1:
        assert not ref["cov"].any()
        want = np.zeros((b, n, 3))
        for s in range(b):
            np.add.at(want[s], idx[s].reshape(-1), ref["dmu"][s].astype(np.float64))
        assert np.array_equal(ref["dxyz"], want)


@pytest.mark.parametrize("which", [0, 1])
def test_guard_accepts_the_pair_list_clouds(which):
    a, b, ia, ib = lc.pair_inputs(which)
    assert len(set(ia.tolist())) < len(ia) and set(range(len(a))) - set(ia.tolist()) and set(range(len(b))) - set(ib.tolist())
    q = 2.0 ** -lc.PAIR_BITS
    minx, argx, miny, argy = lm.chamfer(a[ia], b[ib])
    bound = lm.gram_abs(a[ia], b[ib])
    lm.assert_exact(minx, q * q, bound)
    lm.assert_exact(miny, q * q, bound)


def test_guard_rejects_what_is_not_exact():
    x, y = lc.chamfer_inputs("lattice", 3, 1, 40, 50, 3)
    lm.assert_exact(x, 2.0 ** -3)
    bad = x.copy()
    bad[0, 7, 1] = np.float32(0.3)                                # not dyadic
    with pytest.raises(AssertionError, match="multiple"):
        lm.assert_exact(bad, 2.0 ** -3)
    with pytest.raises(AssertionError, match="multiple"):
        lm.assert_exact(lm.chamfer(bad, y)[0], 4.0 ** -3, lm.gram_abs(bad, y))
    with pytest.raises(AssertionError, match="multiple"):         # a gradient that is no multiple of 1/4
        lm.assert_exact(lm.chamfer_grad_uniform(x, y, *lm.chamfer(x, y)[1::2], 0.3, 1.0)[0], 2.0 ** -5)
    with pytest.raises(AssertionError, match="2\\^24"):           # a destination that collects too much
        lm.assert_exact(np.array([1.0]), 2.0 ** -10, np.array([2.0 ** 14]))
    with pytest.raises(AssertionError, match="2\\^24"):           # a translation the lattice cannot carry
        big = x + np.float32(1024.0)
        lm.assert_exact(lm.chamfer(big, y + np.float32(1024.0))[0], 4.0 ** -3, lm.gram_abs(big, y + np.float32(1024.0)))
    with pytest.raises(AssertionError, match="float32"):          # (below 2^24 quanta, yet under float32's range)
        lm.assert_exact(np.array([3.0 * 2.0 ** -160]), 2.0 ** -160)
    with pytest.raises(AssertionError, match="finite"):
        lm.assert_exact(np.array([np.nan]), 1.0)
