"""GPU: the exact EMD (csrc/auction.hip) -- pdgn_auction_assign against scipy's Hungarian optimum and against the host mirror
(tests/auction_mirror.py) element for element; termination and status on degenerate and tie-heavy inputs; the gradient; the
evaluation's emd="auction" path, the test phase's log.txt and the full report's metrics.csv under --emd auction; the indexed
entry point against the batched one.  Raw outputs sit inside sentinel-filled guard
bands.  tests/golden holds no mesh, so the inputs of the optimum test are Gaussian and anisotropic clouds only."""
import os

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import auction_mirror as am

pytestmark = pytest.mark.gpu
GUARD = 64
SENTINEL = -12345
F32, I32 = torch.float32, torch.int32


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _guarded(shape, dev, dtype):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    return whole[GUARD:GUARD + n].view(shape), whole


def _raw(a, b):
    """pdgn_auction_assign itself, every output inside guard bands -> numpy (assign, cost, status, bids)."""
    from pdgn_amd import _lib
    dev = _dev()
    ta, tb = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(b, np.float32)).to(dev)
    p, n, _ = ta.shape
    outs = [_guarded((p, n), dev, I32), _guarded((p,), dev, F32), _guarded((p,), dev, I32), _guarded((p,), dev, torch.int64)]
    rc = _lib.lib().pdgn_auction_assign(p, n, _lib.ptr(ta), _lib.ptr(tb), *[_lib.ptr(v) for v, _ in outs], _lib.stream_of(ta))
    torch.cuda.synchronize()
    assert rc == 0
    for _, whole in outs:
        assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())
    return tuple(v.cpu().numpy() for v, _ in outs)


def _hungarian(a, b):
    d = np.sqrt(((a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]) ** 2).sum(-1))
    r, c = linear_sum_assignment(d)
    return float(d[r, c].sum())


def _check_optimum(a, b, assign, what):
    """The issue's two-sided check: the fp64 cost of `assign` is no less than the Hungarian optimum (1e-6 relative for the fp64
    sums) and at most n quanta above it."""
    n = a.shape[0]
    q = float(am.quantum_of(am.cmax_of(a, b)))
    opt, got = _hungarian(a, b), am.cost_of(a, b, assign)
    print("%s: optimum %.9g auction %.9g excess %.3g n q %.3g" % (what, opt, got, got - opt, n * q))
    assert got >= opt - 1e-6 * opt, what
    assert got <= opt + n * q, what


def _clouds(n, seed):
    """Four pairs: two of Gaussian clouds, two anisotropic ones (axes 1 : 0.1 : 0.01, the second cloud shifted)."""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((4, n, 3)), rng.standard_normal((4, n, 3))
    a[2:] *= (1.0, 0.1, 0.01)
    b[2:] = b[2:] * (1.0, 0.1, 0.01) + 0.25
    return a.astype(np.float32), b.astype(np.float32)


# ---------------------------------------------------------------------------- 1. the optimum
# n = 1 and 2: the smallest problems; 63 / 64 / 65: a partial wave, a full one, one object past it; 256: the last size of the
# 256-thread instance; 512: the 512-thread instance, several objects per lane; 1160: the 1024-thread instance where the dynamic
# LDS alone (64 960 bytes) is under 64 KB and dynamic plus static is over it
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 256, 512, 1160])
def test_assignment_is_the_hungarian_optimum_within_n_quanta(n):
    from pdgn_amd import _lib
    a, b = _clouds(n, 1000 + n)
    assign, cost, status, bids = _raw(a, b)
    cap = _lib.lib().pdgn_auction_max_bids(n)
    for p in range(a.shape[0]):
        assert am.is_permutation(assign[p]), (n, p)
        assert status[p] == 0, (n, p, status[p])
        assert 0 <= bids[p] < cap, (n, p, bids[p], cap)         # not the capped path in disguise
        assert (bids[p] > 0) == (n > 1)
        _check_optimum(a[p], b[p], assign[p], "n %d pair %d (%d bids of %d)" % (n, p, bids[p], cap))
        host = am.cost_of(a[p], b[p], assign[p])
        assert abs(float(cost[p]) - host) <= 1e-5 * host + 1e-30, (n, p, cost[p], host)       # the kernel's own fp32 sum of n terms


# ---------------------------------------------------------------------------- 2. the mirror, element for element
@pytest.mark.parametrize("n", [64, 256])
def test_assignment_and_bid_count_equal_the_mirror_and_repeat(n):
    a, b = _clouds(n, 2000 + n)
    side = round(n ** (1 / 3) + 0.5)
    ax = np.arange(side, dtype=np.float32)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(n)
    a[1], b[1] = g[rng.integers(0, len(g), n)], g[rng.integers(0, len(g), n)]                # lattice draws: exact cost ties, repeated points
    first, second = _raw(a, b), _raw(a, b)
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()
    assign, cost, status, bids = first
    for p in range(a.shape[0]):
        m_assign, m_bids, m_status, _ = am.auction(a[p], b[p])
        assert status[p] == m_status, (n, p)
        assert bids[p] == m_bids, (n, p, bids[p], m_bids)
        assert np.array_equal(assign[p], m_assign), (n, p)


# ---------------------------------------------------------------------------- 3. the workload's size, the LDS limit
def test_one_pair_of_2048_points():
    from pdgn_amd import _lib
    from pdgn_amd.structural_losses import emd_cost
    rng = np.random.default_rng(2048)
    a = rng.standard_normal((1, 2048, 3)).astype(np.float32)
    b = rng.standard_normal((1, 2048, 3)).astype(np.float32)
    assign, cost, status, bids = _raw(a, b)
    assert am.is_permutation(assign[0]) and status[0] == 0
    assert 0 < bids[0] < _lib.lib().pdgn_auction_max_bids(2048)
    dev = _dev()
    approx = float(emd_cost(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))[0])
    print("n 2048: exact %.9g approximate %.9g bids %d" % (float(cost[0]), approx, bids[0]))
    assert float(cost[0]) <= approx * (1 + 1e-3)                 # a sanity bound, not a theorem: the approximate matching is not exactly feasible
    host = am.cost_of(a[0], b[0], assign[0])
    assert abs(float(cost[0]) - host) <= 1e-5 * host


# ---------------------------------------------------------------------------- 4. termination
def _termination_cases():
    rng = np.random.default_rng(4)
    cases = {}
    cases["all-equal"] = (np.full((64, 3), 0.75, np.float32), np.full((64, 3), 0.75, np.float32))
    nan = rng.standard_normal((64, 3)).astype(np.float32)
    nan[17, 1] = np.nan
    cases["nan"] = (nan, rng.standard_normal((64, 3)).astype(np.float32))
    a = rng.standard_normal((256, 3)).astype(np.float32)
    cases["permuted-copy"] = (a, a[rng.permutation(256)])
    ax = np.arange(8, dtype=np.float32)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    cases["lattice-shifted"] = (g, g[rng.permutation(512)] + np.float32([1, 0, 0]))
    cases["lattice-draws"] = (g[rng.integers(0, 512, 512)], g[rng.integers(0, 512, 512)])
    c, d = rng.standard_normal((256, 3)).astype(np.float32), rng.standard_normal((256, 3)).astype(np.float32)
    c[128:] += np.float32(2.0 ** 20)
    d[100:] += np.float32(2.0 ** 20)                             # 28 points have to cross
    cases["two-clusters"] = (c, d)
    # every bidder the same point: identical rows, one price war per object -- about n^2 / 2 bids per phase, the cap's case
    cases["coincident-bidders"] = (np.full((256, 3), 0.5, np.float32), rng.standard_normal((256, 3)).astype(np.float32))
    return cases


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", ["all-equal", "nan", "permuted-copy", "lattice-shifted", "lattice-draws", "two-clusters", "coincident-bidders"])
def test_every_input_terminates_with_a_permutation_and_a_status(name):
    from pdgn_amd import _lib
    a, b = _termination_cases()[name]
    n = a.shape[0]
    assign, cost, status, bids = _raw(a[None], b[None])
    print("%s: status %d bids %d of %d cost %r" % (name, status[0], bids[0], _lib.lib().pdgn_auction_max_bids(n), float(cost[0])))
    assert am.is_permutation(assign[0])
    assert status[0] in (0, 1, 2)
    assert 0 <= bids[0] <= _lib.lib().pdgn_auction_max_bids(n)
    if name in ("all-equal", "nan"):
        assert status[0] == 2 and bids[0] == 0 and np.array_equal(assign[0], np.arange(n))
        assert np.isnan(cost[0]) if name == "nan" else cost[0] == 0.0
    if status[0] == 0:
        _check_optimum(a, b, assign[0], name)
    m_assign, m_bids, m_status, _ = am.auction(a, b)             # capped or not, the mirror says the same
    assert (status[0], bids[0]) == (m_status, m_bids) and np.array_equal(assign[0], m_assign)


# ---------------------------------------------------------------------------- 5. the gradient
def _separated_pair(rng, b=2):
    """A 4 x 4 x 4 grid of spacing 4 and, shuffled, a copy displaced by 0.5 .. 1.5 per point: every point's twin is its nearest
    object by more than 1, so the optimum is the twin matching and stays it under perturbations far larger than the step."""
    ax = np.arange(4, dtype=np.float64) * 4.0
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    a = np.stack([g] * b)
    u = rng.standard_normal((b, 64, 3))
    u *= rng.uniform(0.5, 1.5, (b, 64, 1)) / np.linalg.norm(u, axis=2, keepdims=True)
    perms = [rng.permutation(64) for _ in range(b)]
    bb = np.stack([(a[p] + u[p])[perms[p]] for p in range(b)])
    return a.astype(np.float32), bb.astype(np.float32)


def test_cost_grad_is_the_closed_form_and_grad2_its_negative_scatter():
    from pdgn_amd import _lib
    from pdgn_amd.structural_losses import auction_match
    dev = _dev()
    rng = np.random.default_rng(5)
    a, b = _clouds(64, 5)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    assign, _, status = auction_match(ta, tb)
    assert bool((status == 0).all())
    g = torch.from_numpy(rng.uniform(0.5, 2.0, a.shape[0]).astype(np.float32)).to(dev)
    (g1, w1), (g2, w2) = _guarded(a.shape, dev, F32), _guarded(b.shape, dev, F32)
    rc = _lib.lib().pdgn_auction_cost_grad(a.shape[0], 64, _lib.ptr(ta), _lib.ptr(tb), _lib.ptr(assign), _lib.ptr(g), _lib.ptr(g1),
                                           _lib.ptr(g2), _lib.stream_of(ta))
    torch.cuda.synchronize()
    assert rc == 0
    for whole in (w1, w2):
        assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())
    idx = assign.long()
    matched = torch.gather(tb, 1, idx[:, :, None].expand(-1, -1, 3))
    diff = ta - matched
    want = g[:, None, None] * diff / (diff * diff).sum(2, keepdim=True).clamp_min(1e-20).sqrt()
    assert torch.allclose(g1, want, rtol=1e-6, atol=1e-30), float((g1 - want).abs().max())
    scattered = torch.zeros_like(g2).scatter_(1, idx[:, :, None].expand(-1, -1, 3), -g1)
    assert torch.equal(g2, scattered)


def test_exact_emd_cost_backward_agrees_with_finite_differences():
    """Central differences of the fp32 cost against the backward, on pairs whose optimum is separated from the runner-up by more
    than 1 (the perturbed assignments are checked to be the base one).

    Along the gradient, v = grad / |grad| over both clouds (|v| = 1, h = 1/2: a point moves 0.044): a_i and its match move apart
    along their own difference, so the cost is LINEAR in the step -- no truncation term -- and the derivative is |grad| =
    sqrt(64 + 64) = 11.3 (a unit vector per point of either cloud).  What is left is fp32: a cost below 100 carries at most 10 * 2^-24 relative
    from its terms and its sum (6e-5) and at most 64 * 2 * sqrt(3) * 2^-21 (1.1e-4) from rounding the perturbed coordinates, which are
    below 16: 1.7e-4 per evaluation, 3.4e-4 over 2 h = 1 for the difference, 3e-5 of the derivative.  Asserted: the issue's 1e-4
    relative, nothing added.

    Along random directions (a unit vector per point, one trial on each cloud alone and two on both, h = 2^-7) the cost is curved:
    the central difference of |u + t w| is off by at most h^2 / 6 * 3 |w|^3 / (|u| - h |w|)^2, summed here over the pairs from
    the inputs; the fp32 term above becomes 3.4e-4 / (2 h).  Asserted: 1e-4 relative plus that explicit absolute term (printed; about
    3e-2 on derivatives of about 5, so these trials catch a wrong or missing point's gradient -- a change of order 1 -- and the
    gradient direction carries the tight bound)."""
    from pdgn_amd.structural_losses import auction_match, exact_emd_cost
    dev = _dev()
    rng = np.random.default_rng(55)
    a, b = _separated_pair(rng)
    ta = torch.from_numpy(a).to(dev).requires_grad_(True)
    tb = torch.from_numpy(b).to(dev).requires_grad_(True)
    cost = exact_emd_cost(ta, tb)
    assert cost.requires_grad and cost.shape == (2,)
    cost.sum().backward()
    base = auction_match(ta.detach(), tb.detach())[0]
    assert torch.equal(exact_emd_cost(ta.detach(), tb.detach()), cost.detach())          # the plain launch: the same bits
    assert float(cost.detach().max()) < 100.0 and float(torch.maximum(ta.detach().abs().max(), tb.detach().abs().max())) < 15.0      # what the fp32 term assumes
    fp32_term = 100.0 * 10 * 2.0 ** -24 + 64 * 2 * 3 ** 0.5 * 2.0 ** -21                 # per evaluation

    def central(va, vb, h):
        with torch.no_grad():
            plus, minus = ((ta + h * va).contiguous(), (tb + h * vb).contiguous()), ((ta - h * va).contiguous(), (tb - h * vb).contiguous())
            for pa, pb in (plus, minus):
                assert torch.equal(auction_match(pa, pb)[0], base)
            fd = (exact_emd_cost(*plus).double() - exact_emd_cost(*minus).double()) / (2 * h)
        return fd, ((ta.grad * va).sum((1, 2)) + (tb.grad * vb).sum((1, 2))).double()

    # ---- along the gradient: 1e-4 relative
    norm = (ta.grad.double().pow(2).sum((1, 2)) + tb.grad.double().pow(2).sum((1, 2))).sqrt().float().view(-1, 1, 1)
    fd, analytic = central(ta.grad / norm, tb.grad / norm, 0.5)
    print("gradient direction: fd %s analytic %s relative error %s" % (fd.tolist(), analytic.tolist(), ((fd - analytic).abs() / analytic.abs()).tolist()))
    assert bool((analytic > 11.0).all())
    assert bool(((fd - analytic).abs() <= 1e-4 * analytic.abs()).all())
    # ---- random directions: 1e-4 relative plus the truncation and fp32 terms
    h = 2.0 ** -7
    idx = base.long()[:, :, None].expand(-1, -1, 3)
    for trial in range(4):
        va = torch.from_numpy(rng.standard_normal(a.shape).astype(np.float32)).to(dev)
        vb = torch.from_numpy(rng.standard_normal(b.shape).astype(np.float32)).to(dev)
        va, vb = va / va.norm(dim=2, keepdim=True), vb / vb.norm(dim=2, keepdim=True)
        if trial == 0:
            vb = torch.zeros_like(vb)
        if trial == 1:
            va = torch.zeros_like(va)
        fd, analytic = central(va, vb, h)
        with torch.no_grad():
            u = (ta - torch.gather(tb, 1, idx)).double().norm(dim=2)
            w = (va - torch.gather(vb, 1, idx)).double().norm(dim=2)
            truncation = (h * h / 2 * w.pow(3) / (u - h * w).pow(2)).sum(1)
        atol = truncation + 2 * fp32_term / (2 * h)
        print("trial %d: fd %s analytic %s error %s atol %s" % (trial, fd.tolist(), analytic.tolist(), (fd - analytic).abs().tolist(), atol.tolist()))
        assert bool(((fd - analytic).abs() <= 1e-4 * analytic.abs() + atol).all())


def test_unequal_sizes_raise():
    from pdgn_amd.structural_losses import auction_match, exact_emd_cost
    dev = _dev()
    with pytest.raises(ValueError):
        auction_match(torch.zeros(1, 8, 3, device=dev), torch.zeros(1, 9, 3, device=dev))
    with pytest.raises(ValueError):
        exact_emd_cost(torch.zeros(1, 8, 3, device=dev), torch.zeros(1, 9, 3, device=dev))


# ---------------------------------------------------------------------------- 6. the evaluation
def test_evaluation_with_the_exact_emd():
    from pdgn_amd import evaluation as ev
    from pdgn_amd.structural_losses import auction_match
    dev = _dev()
    S = R = 6
    n = 256
    gen = torch.Generator(device="cpu").manual_seed(6)
    smp = (torch.randn(S, n, 3, generator=gen) * 0.2).to(dev)
    ref = (torch.randn(R, n, 3, generator=gen) * 0.2).to(dev)
    cd_x, emd_x = ev.pairwise_emd_cd(smp, ref, emd="auction")
    cd_a, emd_a = ev.pairwise_emd_cd(smp, ref, emd="approx")
    _, cost, status = auction_match(smp.repeat_interleave(R, 0).contiguous(), ref.repeat(S, 1, 1).contiguous())
    assert torch.equal(emd_x, (cost / float(n)).view(S, R))
    assert bool((status == 0).all())
    assert cd_x.cpu().numpy().tobytes() == cd_a.cpu().numpy().tobytes()
    assert bool((emd_x <= emd_a * (1 + 1e-3)).all())             # (the sanity bound of the 2048-point test, on 36 pairs)
    default, approx = ev.compute_all_metrics(smp, ref), ev.compute_all_metrics(smp, ref, emd="approx")
    assert list(default) == list(approx)
    for k in default:
        assert default[k].cpu().numpy().tobytes() == approx[k].cpu().numpy().tobytes(), k
    exact = ev.compute_all_metrics(smp, ref, emd="auction")
    assert list(exact) == list(default) + ["emd-capped"]
    assert float(exact["emd-capped"]) == 0.0
    for k in default:
        if "EMD" not in k:
            assert exact[k].cpu().numpy().tobytes() == default[k].cpu().numpy().tobytes(), k
    assert float(exact["lgan_mmd-EMD"]) <= float(default["lgan_mmd-EMD"]) * (1 + 1e-3)
    paired = ev.emd_cd(smp, ref, reduced=False, emd="auction")
    assert torch.equal(paired["MMD-EMD"], torch.diagonal(emd_x))
    with pytest.raises(ValueError):
        ev.pairwise_emd_cd(smp, ref[:, :128].contiguous(), emd="auction")


def test_launches_of_the_evaluation_are_split_and_the_result_is_not(monkeypatch):
    """The exact EMD goes out in launches of at most _MAX_AUCTION_PAIRS pairs; with the limit at 5 (36 pairs: eight launches, the
    last of one pair) the matrix and the capped count are those of one launch."""
    from pdgn_amd import evaluation as ev
    dev = _dev()
    gen = torch.Generator(device="cpu").manual_seed(66)
    smp, ref = (torch.randn(6, 65, 3, generator=gen) * 0.2).to(dev), (torch.randn(6, 65, 3, generator=gen) * 0.2).to(dev)
    smp[2] = 0.1                                                 # a cloud collapsed to one point: against itself degenerate
    whole = ev.compute_all_metrics(smp, ref, emd="auction")
    emd_whole = ev.pairwise_emd_cd(smp, smp, emd="auction")[1]
    monkeypatch.setattr(ev, "_MAX_AUCTION_PAIRS", 5)
    split = ev.compute_all_metrics(smp, ref, emd="auction")
    assert torch.equal(ev.pairwise_emd_cd(smp, smp, emd="auction")[1], emd_whole)
    assert list(split) == list(whole)
    for k in whole:
        assert whole[k].cpu().numpy().tobytes() == split[k].cpu().numpy().tobytes(), k
    assert float(whole["emd-capped"]) >= 1.0                     # (smp[2], smp[2]) at the least


def test_test_phase_log_names_the_exact_emd(tmp_path):
    """--phase test --emd auction on a toy data set (initial weights: no checkpoint is given): log.txt opens with the line that
    names the EMD and the pairs not at an optimum, the rest are the metric lines, emd-capped among them with that count."""
    from pdgn_amd import train
    from pdgn_amd.data import cate_to_synsetid
    rng = np.random.default_rng(8)
    sid = cate_to_synsetid["chair"]
    for sp, count in (("train", 4), ("val", 2), ("test", 5)):
        (tmp_path / "pc" / sid / sp).mkdir(parents=True)
        for j in range(count):
            np.save(tmp_path / "pc" / sid / sp / ("shape%02d.npy" % j), rng.standard_normal((64, 3)).astype(np.float32))
    common = ["--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root", str(tmp_path / "pc"), "--choice", "chair",
              "--batch_size", "4", "--seed", "1", "--num_point", "64", "--num_k", "4", "--phase", "test"]
    out = train.main(common + ["--save_dir", str(tmp_path / "exact"), "--emd", "auction"])
    lines = open(os.path.join(out, "log.txt")).read().splitlines()
    assert lines[0].startswith("# EMD: auction") and "pdgn_auction_assign_indexed" in lines[0]
    metrics = dict(l.split(": ") for l in lines[1:])
    assert "lgan_mmd-EMD" in metrics and "1-NN-EMD-acc" in metrics and "jsd" in metrics
    capped = float(metrics["emd-capped"])
    assert capped == int(capped) and 0 <= capped <= 75 and lines[0].endswith("pairs not at an optimum: %d" % capped)
    out = train.main(common + ["--save_dir", str(tmp_path / "approx")])       # the default: metric lines only, as before
    lines = open(os.path.join(out, "log.txt")).read().splitlines()
    assert all(len(l.split(": ")) == 2 and np.isfinite(float(l.split(": ")[1])) for l in lines) and not any("capped" in l or "#" in l for l in lines)


def test_full_report_with_the_exact_emd_has_the_capped_column(tmp_path):
    from pdgn_amd.report import FULL_KEYS, SnapshotReporter
    from pdgn_amd.trainer import PDGNTrainer
    dev = _dev()
    gen = torch.Generator(device="cpu").manual_seed(9)
    val = (torch.randn(4, 2048, 3, generator=gen) * 0.2).to(dev)
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    reporter = SnapshotReporter(tr, val, tmp_path / "report", every=1, batch_size=4, normalize="shape_bbox", seed=9, rows=2, cell=32, full=True,
                                emd="auction")
    epoch, results, _ = reporter(1)
    rows = open(tmp_path / "report" / "metrics.csv").read().splitlines()
    header = rows[0].split(",")
    assert header == ["epoch"] + list(FULL_KEYS) + ["emd-capped", "seconds"] and len(rows) == 2
    row = dict(zip(header, rows[1].split(",")))
    assert float(row["emd-capped"]) == results["emd-capped"] and 0 <= results["emd-capped"] <= 48
    with pytest.raises(ValueError):
        SnapshotReporter(tr, val, tmp_path / "report", every=1, batch_size=4, normalize="shape_bbox", seed=9, emd="exact")


# ---------------------------------------------------------------------------- 7. indexed against batched
@pytest.mark.parametrize("n", [65, 256])
def test_indexed_and_batched_entry_points_agree_bit_for_bit(n):
    from pdgn_amd import _lib
    from pdgn_amd.structural_losses import auction_match
    dev = _dev()
    a, b = _clouds(n, 7000 + n)
    a[3] = 0.5                                                   # a degenerate pair where it meets b[3] = the same point
    b[3] = 0.5
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    ia = torch.tensor([0, 1, 2, 3, 3, 0, 2, 1], dtype=I32, device=dev)
    ib = torch.tensor([0, 1, 2, 3, 0, 3, 2, 0], dtype=I32, device=dev)
    (cost, wc), (status, ws) = _guarded((8,), dev, F32), _guarded((8,), dev, I32)
    rc = _lib.lib().pdgn_auction_assign_indexed(8, n, _lib.ptr(ta), _lib.ptr(ia), _lib.ptr(tb), _lib.ptr(ib), _lib.ptr(cost), _lib.ptr(status),
                                                _lib.stream_of(ta))
    torch.cuda.synchronize()
    assert rc == 0
    for whole in (wc, ws):
        assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())
    _, cost_b, status_b = auction_match(ta[ia.long()].contiguous(), tb[ib.long()].contiguous())
    assert cost.cpu().numpy().tobytes() == cost_b.cpu().numpy().tobytes()
    assert torch.equal(status, status_b)
    assert status[3] == 2 and status[:3].tolist() == [0, 0, 0] and status[5:].tolist() == [0, 0, 0]
    assert status[4] == am.auction(a[3], b[0])[2]                # (coincident bidders: capped at n = 256, the mirror agrees)
