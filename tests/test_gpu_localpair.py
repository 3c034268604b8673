"""csrc/localpair.hip in every dispatch regime, bit for bit: the Gram-form Chamfer minima WITH their argmins, the Chamfer adjoint
through the LDS kernel and through the zero-fill + global-atomic kernel (both fill branches), the pair-list entry points, and the
neighbourhood statistics with their adjoint in all three staging regimes -- against tests/localpair_mirror.py (float64 numpy) on
dyadic-lattice inputs whose every intermediate value is a float32 (tests/localpair_cases.py runs the mirror's exactness guard on each
case before anything is compared; tests/test_localpair_mirror_host.py checks mirror and guard on the host).  The argmins are read
through the C ABI (localpair_worker.device_chamfer*); the Python wrappers are used where values and gradients are all that matters."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import localpair_cases as lc
import localpair_mirror as lm
import localpair_worker as lw
from localpair_worker import dev, f32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _id(case):
    return "-".join(map(str, case))


# ---------------------------------------------------------------------------- A. Chamfer forward, exact, with ties
@pytest.mark.parametrize("case", lc.CHAMFER_FORWARD, ids=_id)
def test_chamfer_forward_minima_and_argmins_exact(case):
    kind, bits, b, m, n, d = case
    ref = lc.chamfer_reference(case)
    minx, argx, miny, argy = (t.cpu().numpy() for t in lw.device_chamfer(dev(ref["x"]), dev(ref["y"])))
    np.testing.assert_array_equal(argx, ref["argx"])
    np.testing.assert_array_equal(argy, ref["argy"])
    np.testing.assert_array_equal(minx, f32(ref["minx"]))
    np.testing.assert_array_equal(miny, f32(ref["miny"]))
    if kind.startswith("tie"):                                    # the copy in the earlier candidate tile wins
        assert (argx[:, 64:128] == int(kind[3:].split("_")[0])).all()
    if kind == "same_y":
        assert not argx.any()
    if kind == "x_is_y":                                          # exactly zero, not a small negative number
        assert not minx.any() and not miny.any() and (argx <= np.arange(m)).all() and (argy <= np.arange(n)).all()
    from pdgn_amd.losses import chamfer_min
    wx, wy = chamfer_min(dev(ref["x"]), dev(ref["y"]))
    np.testing.assert_array_equal(wx.cpu().numpy(), minx)
    np.testing.assert_array_equal(wy.cpu().numpy(), miny)


def test_a_nan_coordinate_makes_the_chamfer_sum_non_finite():
    """What the gradient guard (trainer.GradGuard) relies on: a poisoned cloud cannot come out as a finite loss."""
    from pdgn_amd import losses
    x, y = lc.chamfer_inputs("lattice", 3, 2, 300, 200, 3)
    x = x.copy()
    x[1, 17, 2] = np.nan
    assert not torch.isfinite(losses.chamfer_sum(dev(x), dev(y))).item()
    assert not torch.isfinite(losses.chamfer_sum(dev(y), dev(x))).item()


# ---------------------------------------------------------------------------- B. Chamfer adjoint, exact, every launch path
@pytest.mark.parametrize("layout", ["one", "two"])
@pytest.mark.parametrize("case", lc.CHAMFER_GRAD, ids=_id)
def test_chamfer_adjoint_exact_from_sentinel_filled_buffers(case, layout):
    """Both C entry points (per-minimum gradients; the uniform g = 3, scale = 0.25) at shapes on either side of CHL_MAXF, into one
    buffer (the fallback's single fill) and into two (its two fills): whatever the buffers held is gone, nothing beside them is
    written, and the sums are the mirror's scatter through the mirror's argmins."""
    lw.run_case(case, layouts=(layout,))


@pytest.mark.parametrize("case", lc.CHAMFER_GRAD, ids=_id)
def test_chamfer_wrappers_adjoints_exact(case):
    """losses.chamfer_min (ChamferGram: gx and gy from two empty_like allocations) and losses.chamfer_sum (ChamferSum: one buffer)
    through autograd: what reaches .grad is the mirror's, bit for bit -- the fallback's fills are all that clears those buffers."""
    from pdgn_amd import losses
    ref = lc.chamfer_reference(case)
    x, y = dev(ref["x"]).requires_grad_(True), dev(ref["y"]).requires_grad_(True)
    torch.empty(x.numel() + y.numel() + 4096, device="cuda").fill_(lw.SENTINEL)     # leave the allocator's free blocks dirty
    minx, miny = losses.chamfer_min(x, y)
    ((minx * dev(ref["gminx"])).sum() + (miny * dev(ref["gminy"])).sum()).backward()
    np.testing.assert_array_equal(x.grad.cpu().numpy(), f32(ref["gx"]))
    np.testing.assert_array_equal(y.grad.cpu().numpy(), f32(ref["gy"]))
    x.grad, y.grad = None, None
    torch.empty(x.numel() + y.numel() + 4096, device="cuda").fill_(lw.SENTINEL)
    total = losses.chamfer_sum(x, y, lc.UNIFORM_SCALE)
    (total * lc.UNIFORM_G).backward()
    np.testing.assert_array_equal(x.grad.cpu().numpy(), f32(ref["ux"]))
    np.testing.assert_array_equal(y.grad.cpu().numpy(), f32(ref["uy"]))
    mins = np.concatenate([ref["minx"].reshape(-1), ref["miny"].reshape(-1)])
    lm.assert_exact(lc.UNIFORM_SCALE * mins.sum(), 4.0 ** -case[1] * lc.UNIFORM_SCALE, lc.UNIFORM_SCALE * np.abs(mins).sum())
    assert total.item() == lc.UNIFORM_SCALE * mins.sum()


def test_global_atomic_adjoint_in_a_child_process_with_the_lds_kernel_switched_off(tmp_path):
    """PDGN_CHAMFER_LDS=0 is read once per process: a fresh child runs (2, 256, 128, 9) -- an LDS shape -- through the fills and the
    global-atomic kernel, checks it against the mirror itself, and hands its bits back; this process runs the LDS kernel."""
    mine = lw.run_case(lc.WORKER_CASE)
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, PDGN_CHAMFER_LDS="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "localpair_worker.py"), out], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0 and "localpair worker ok: PDGN_CHAMFER_LDS=0" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
    theirs = np.load(out)
    assert sorted(theirs.files) == sorted(mine)
    for k in mine:
        np.testing.assert_array_equal(theirs[k], mine[k], err_msg=k)


def test_local_pair_at_a_fallback_shape_vs_oracle():
    """LocalPairLoss(20) with 1400 query points: the 9-D covariance pair (1400 x 9 = 12600 floats > CHL_MAXF) takes the fills and the
    global-atomic adjoint, the 3-D mean pair the LDS kernel; against the oracle's restatement of get_local_pair."""
    from oracle import pdgnet_ref
    from pdgn_amd.losses import LocalPairLoss
    rng = np.random.default_rng(11)
    p1 = torch.from_numpy(rng.standard_normal((1, 3, 1400)).astype(np.float32))
    p2 = torch.from_numpy(rng.standard_normal((1, 3, 1500)).astype(np.float32))
    a, b = p1.cuda().requires_grad_(True), p2.cuda().requires_grad_(True)
    mu, cov = LocalPairLoss(20)(a, b)
    (mu + cov).backward()
    ar, br = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    rmu, rcov = pdgnet_ref.local_pair(ar, br)
    (rmu + rcov).backward()
    print("mu %.8g / %.8g, cov %.8g / %.8g, max |grad diff| %.3e, %.3e" % (mu.item(), rmu.item(), cov.item(), rcov.item(),
          (a.grad.cpu() - ar.grad).abs().max().item(), (b.grad.cpu() - br.grad).abs().max().item()))
    # the tolerances of test_gpu_losses.py::test_local_pair_vs_oracle
    np.testing.assert_allclose(mu.item(), rmu.item(), rtol=1e-4)
    np.testing.assert_allclose(cov.item(), rcov.item(), rtol=1e-4)
    np.testing.assert_allclose(a.grad.cpu().numpy(), ar.grad.numpy(), rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(b.grad.cpu().numpy(), br.grad.numpy(), rtol=1e-3, atol=1e-4)


# ---------------------------------------------------------------------------- C. pair lists
def _emd(a, b, ia=None, ib=None):
    from pdgn_amd import _lib
    L, ptr = _lib.lib(), _lib.ptr
    n, m = a.shape[1], b.shape[1]
    pairs = a.shape[0] if ia is None else ia.numel()
    temp = torch.empty(L.pdgn_emd_cost_temp_floats(pairs, n, m), device=a.device)
    out = torch.full((pairs,), lw.SENTINEL, device=a.device)
    if ia is None:
        rc = L.pdgn_emd_cost(pairs, n, m, ptr(a), ptr(b), ptr(temp), ptr(out), _lib.stream_of(a))
    else:
        rc = L.pdgn_emd_cost_indexed(pairs, n, m, ptr(a), ptr(ia), ptr(b), ptr(ib), ptr(temp), ptr(out), _lib.stream_of(a))
    _lib.check(rc, "pdgn_emd_cost")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("which", [0, 1])
def test_pair_lists_with_repeats_and_gaps_equal_the_plain_calls_on_gathered_clouds(which):
    a, b, ia, ib = lc.pair_inputs(which)
    ad, bd, iad, ibd = dev(a), dev(b), dev(ia), dev(ib)
    ga, gb = dev(a[ia]), dev(b[ib])
    listed = lw.device_chamfer(ad, bd, iad, ibd)
    plain = lw.device_chamfer(ga, gb)
    for got, want in zip(listed, plain):
        assert torch.equal(got, want)
    minx, argx, miny, argy = lm.chamfer(a[ia], b[ib])             # (guarded in tests/test_localpair_mirror_host.py)
    np.testing.assert_array_equal(listed[0].cpu().numpy(), f32(minx))
    np.testing.assert_array_equal(listed[1].cpu().numpy(), argx)
    np.testing.assert_array_equal(listed[2].cpu().numpy(), f32(miny))
    np.testing.assert_array_equal(listed[3].cpu().numpy(), argy)
    e_listed, e_plain = _emd(ad, bd, iad, ibd), _emd(ga, gb)
    assert torch.equal(e_listed, e_plain) and bool(torch.isfinite(e_listed).all()) and bool((e_listed > 0).all())
    pairs = list(zip(ia.tolist(), ib.tolist()))
    assert pairs[0] == pairs[6] and pairs[3] == pairs[7] and e_listed[0] == e_listed[6] and e_listed[3] == e_listed[7]
    assert len(set(e_listed.tolist())) == len(set(pairs))        # the same pair twice: the same cost; another pair: another cost
    assert torch.equal(ad, dev(a)) and torch.equal(bd, dev(b))   # read-only


def test_pairwise_emd_cd_with_unequal_point_counts_equals_expanded_calls():
    from pdgn_amd import evaluation as ev
    from pdgn_amd.losses import chamfer_min
    from pdgn_amd.structural_losses import emd_cost
    S, R, N, M = 3, 4, 96, 160
    smp = dev(lc.lattice_points("localpair/pairwise/smp", (S, N, 3), 4))
    ref = dev(lc.lattice_points("localpair/pairwise/ref", (R, M, 3), 4))
    cd, emd = ev.pairwise_emd_cd(smp, ref)
    assert cd.shape == (S, R) and emd.shape == (S, R)
    for i in range(S):
        a = smp[i:i + 1].expand(R, -1, -1).contiguous()
        minx, miny = chamfer_min(a, ref)
        assert torch.equal(cd[i], miny.mean(1) + minx.mean(1))
        assert torch.equal(emd[i], emd_cost(a, ref) / float(N))
    assert torch.equal(ev.pairwise_cd(smp, ref), cd)


def test_pair_list_arguments_are_refused_before_any_launch():
    from pdgn_amd import _lib
    L, ptr = _lib.lib(), _lib.ptr
    x = torch.zeros(2, 8, 3, device="cuda")
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.full((64,), lw.SENTINEL, device="cuda")
    arg = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    stream = _lib.stream_of(x)

    def listed(npairs=4, m=8, n=8, d=3):
        return L.pdgn_chamfer_gram_indexed(npairs, m, n, d, ptr(x), ptr(idx), ptr(x), ptr(idx), ptr(out), ptr(arg), ptr(out), ptr(arg), stream)

    INVALID = -1
    assert listed(npairs=65536) == INVALID and listed(d=17) == INVALID and listed(m=0) == INVALID
    assert listed(n=0) == INVALID and listed(d=0) == INVALID and listed(npairs=-1) == INVALID
    assert L.pdgn_chamfer_gram(2, 0, 8, 3, ptr(x), ptr(x), ptr(out), ptr(arg), ptr(out), ptr(arg), stream) == INVALID
    assert L.pdgn_chamfer_gram(2, 8, 8, 17, ptr(x), ptr(x), ptr(out), ptr(arg), ptr(out), ptr(arg), stream) == INVALID
    assert L.pdgn_emd_cost_indexed(4, 0, 8, ptr(x), ptr(idx), ptr(x), ptr(idx), ptr(out), ptr(out), stream) == INVALID
    assert L.pdgn_emd_cost_indexed(-1, 8, 8, ptr(x), ptr(idx), ptr(x), ptr(idx), ptr(out), ptr(out), stream) == INVALID
    assert listed(npairs=0) == 0                                  # nothing to do is not an error, and launches nothing either
    torch.cuda.synchronize()
    assert bool((out == lw.SENTINEL).all()) and bool((arg == -7).all())


# ---------------------------------------------------------------------------- D. local statistics
@pytest.mark.parametrize("case", lc.STATS_EXACT, ids=_id)
def test_local_stats_and_adjoint_exact_in_every_staging_regime(case):
    """n <= 2048 (points and slab in LDS), <= 2730 (the slab alone), beyond (global atomics), both clamps of qsplit, K = 1; a query
    naming one point K times, point 0 in every 2nd query, a point nobody names."""
    from pdgn_amd.losses import local_stats
    b, n, m, K = case
    ref = lc.stats_reference(case)
    xyz = dev(ref["xyz"]).requires_grad_(True)
    mu, cov = local_stats(xyz, dev(ref["idx"]))
    np.testing.assert_array_equal(mu.detach().cpu().numpy(), f32(ref["mu"]))
    np.testing.assert_array_equal(cov.detach().cpu().numpy(), f32(ref["cov"]))
    ((mu * dev(ref["dmu"])).sum() + (cov * dev(ref["dcov"])).sum()).backward()
    got = xyz.grad.cpu().numpy()
    np.testing.assert_array_equal(got, f32(ref["dxyz"]))
    assert not got[:, n - 1].any() and got[:, 0].any()           # the unreferenced point stays exactly 0.0; the hot one does not


def test_local_stats_adjoint_adds_into_what_the_caller_zeroed():
    """The C entry point accumulates (the wrapper hands it zeros): called on a buffer holding 1.0 it returns the mirror's sums + 1,
    in the slab regime (flushed with atomics) as in the global one."""
    from pdgn_amd import _lib
    for case in (lc.STATS_EXACT[2], lc.STATS_EXACT[3]):
        b, n, m, K = case
        ref = lc.stats_reference(case)
        xyz, idx, dmu, dcov = dev(ref["xyz"]), dev(ref["idx"]), dev(ref["dmu"]), dev(ref["dcov"])
        dxyz = torch.ones(b, n, 3, device="cuda")
        _lib.check(_lib.lib().pdgn_local_stats_backward(b, n, m, K, _lib.ptr(xyz), _lib.ptr(idx), _lib.ptr(dmu), _lib.ptr(dcov),
                                                        _lib.ptr(dxyz), _lib.stream_of(xyz)), "pdgn_local_stats_backward")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dxyz.cpu().numpy(), f32(ref["dxyz"] + 1.0))


@pytest.mark.parametrize("K", [20, 7])
@pytest.mark.parametrize("n", [2048, 2500, 3000])
def test_local_stats_at_the_workloads_k_in_every_staging_regime(n, K):
    """1 / 20 and 1 / 7 are not dyadic: Gaussian clouds against the mirror with the tolerances of
    test_gpu_losses.py::test_local_stats_forward_backward."""
    from pdgn_amd.losses import local_stats
    B, M = 2, 300
    rng = np.random.default_rng(n + K)
    xyz = rng.standard_normal((B, n, 3)).astype(np.float32)
    idx = rng.integers(0, n, (B, M, K)).astype(np.int32)
    dmu = rng.standard_normal((B, M, 3)).astype(np.float32)
    dcov = rng.standard_normal((B, M, 9)).astype(np.float32)
    xd = dev(xyz).requires_grad_(True)
    mu, cov = local_stats(xd, dev(idx))
    ((mu * dev(dmu)).sum() + (cov * dev(dcov)).sum()).backward()
    rmu, rcov = lm.local_stats(xyz, idx)
    np.testing.assert_allclose(mu.detach().cpu().numpy(), rmu, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(cov.detach().cpu().numpy(), rcov, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(xd.grad.cpu().numpy(), lm.local_stats_grad(xyz, idx, dmu, dcov), rtol=1e-3, atol=1e-4)
