"""CPU: the exact EMD's host side -- the numpy mirror of csrc/auction.hip (tests/auction_mirror.py) against scipy's Hungarian
solver, its caps and status on degenerate inputs, the constants the library reports, the --emd switch and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import auction_mirror as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hungarian(a, b):
    """The optimum of the true problem in fp64."""
    d = np.sqrt(((a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]) ** 2).sum(-1))
    r, c = linear_sum_assignment(d)
    return float(d[r, c].sum())


def lattice(n_side=8):
    ax = np.arange(n_side, dtype=np.float32)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)


@pytest.mark.parametrize("n", [8, 64, 256])
def test_mirror_reaches_the_hungarian_optimum_within_n_quanta(n):
    """Each quantised cost is within q / 2 of the true one, so the optimum of the quantised problem costs at most n q more than
    the true optimum (and no assignment costs less than the optimum, up to the fp64 sums' rounding)."""
    rng = np.random.default_rng(100 + n)
    for scale in ((1.0, 1.0, 1.0), (1.0, 0.1, 0.01)):
        a = (rng.standard_normal((n, 3)) * scale).astype(np.float32)
        b = (rng.standard_normal((n, 3)) * scale + 0.25).astype(np.float32)
        assign, bids, status, q = am.auction(a, b)
        opt, got = hungarian(a, b), am.cost_of(a, b, assign)
        print("n %d scale %s: optimum %.9g auction %.9g n q %.3g bids %d of %d" % (n, scale, opt, got, n * float(q), bids, am.max_bids(n)))
        assert status == 0 and am.is_permutation(assign)
        assert 0 < bids < am.max_bids(n)
        assert opt - 1e-6 * opt <= got <= opt + n * float(q)


def test_mirror_degenerate_inputs_respect_the_cap_and_report_status():
    rng = np.random.default_rng(7)
    zeros = np.zeros((64, 3), np.float32)
    assign, bids, status, _ = am.auction(zeros, zeros)
    assert status == 2 and bids == 0 and np.array_equal(assign, np.arange(64))
    same = np.full((64, 3), 1.5, np.float32)
    assert am.auction(same, same)[2] == 2
    nan = rng.standard_normal((64, 3)).astype(np.float32)
    nan[17, 1] = np.nan
    assign, bids, status, _ = am.auction(nan, rng.standard_normal((64, 3)).astype(np.float32))
    assert status == 2 and bids == 0 and np.array_equal(assign, np.arange(64))
    inf = nan.copy()
    inf[17, 1] = np.inf
    assert am.auction(zeros, inf)[2] == 2
    huge = np.zeros((2, 3), np.float32)
    huge[1] = 3e38                                               # the extent is finite, its square is not
    assert am.auction(huge, -huge)[2] == 2
    # identical clouds under a permutation: the optimum is 0 and the identity of the permutation
    a = rng.standard_normal((256, 3)).astype(np.float32)
    perm = rng.permutation(256)
    assign, bids, status, _ = am.auction(a, a[perm])
    assert status == 0 and bids <= am.max_bids(256) and am.cost_of(a, a[perm], assign) == 0.0
    assert np.array_equal(perm[assign], np.arange(256))
    # the 8 x 8 x 8 lattice against a shifted, shuffled copy: exact cost ties everywhere
    g = lattice()
    for b in (g[rng.permutation(512)] + np.float32([1, 0, 0]), g[rng.integers(0, 512, 512)]):
        assign, bids, status, q = am.auction(g, b)
        assert am.is_permutation(assign) and status in (0, 1) and bids <= am.max_bids(512)
        if status == 0:
            opt = hungarian(g, b)
            assert opt - 1e-6 * opt <= am.cost_of(g, b, assign) <= opt + 512 * float(q)


def test_mirror_cap_completes_in_index_order(monkeypatch):
    """With the bid cap lowered to a fraction of what the pair needs the mirror stops at it, says so and still returns a
    permutation: what was assigned stays, the free bidders take the free objects in index order."""
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((64, 3)).astype(np.float32), rng.standard_normal((64, 3)).astype(np.float32)
    full = am.auction(a, b)
    assert full[2] == 0
    monkeypatch.setattr(am, "max_bids", lambda n: 200)
    assign, bids, status, _ = am.auction(a, b)
    assert status == 1 and bids <= 200 and am.is_permutation(assign)
    monkeypatch.setattr(am, "max_bids", lambda n: 0)             # nothing assigned at all: the identity
    assign, bids, status, _ = am.auction(a, b)
    assert status == 1 and bids == 0 and np.array_equal(assign, np.arange(64))
    monkeypatch.setattr(am, "max_bids", lambda n: 1 << 40)
    monkeypatch.setattr(am, "max_rounds", lambda n: 1)
    assign, bids, status, _ = am.auction(a, b)
    assert status == 1 and bids == 64 and am.is_permutation(assign)


def test_library_constants_match_the_mirror():
    """Host-only entry points: no device work."""
    from pdgn_amd import _lib, build
    L = ctypes.CDLL(build.build())
    L.pdgn_auction_max_bids.restype = ctypes.c_longlong
    assert L.pdgn_auction_quantum_bits() == am.QUANTUM_BITS == 20
    for n in (1, 2, 63, 64, 65, 256, 512, 1024, 2047, 2048):
        assert L.pdgn_auction_max_bids(n) == am.max_bids(n) == 64 * n * am.phases(n)
    assert 11 <= am.phases(64) <= am.phases(2048) <= 14
    assert L.pdgn_auction_max_bids(0) == L.pdgn_auction_max_bids(2049) == L.pdgn_auction_max_bids(-5) == -1
    # an unsupported size or a null pointer is refused on the host, before any launch
    L.pdgn_auction_assign.argtypes = _lib.SIGNATURES["pdgn_auction_assign"][1]
    one = ctypes.c_void_p(4096)
    for n in (0, -1, am.MAX_N + 1):
        assert L.pdgn_auction_assign(1, n, one, one, one, one, one, None, None) == -1
    assert L.pdgn_auction_assign(1, 64, None, one, one, one, one, None, None) == -1
    assert L.pdgn_auction_assign(1, 64, one, one, ctypes.c_void_p(4098), one, one, None, None) == -1
    assert L.pdgn_auction_assign(0, 64, None, None, None, None, None, None, None) == 0


def test_abi_is_bumped_and_the_entry_points_are_declared():
    from pdgn_amd import _lib
    assert _lib.ABI_VERSION >= 38
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES["pdgn_auction_quantum_bits"] == (i, ())
    assert _lib.SIGNATURES["pdgn_auction_max_bids"] == (ll, (i,))
    assert _lib.SIGNATURES["pdgn_auction_assign"] == (i, (i, i) + (vp,) * 7)
    assert _lib.SIGNATURES["pdgn_auction_assign_indexed"] == (i, (i, i) + (vp,) * 7)
    assert _lib.SIGNATURES["pdgn_auction_cost_grad"] == (i, (i, i) + (vp,) * 7)
    header = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    assert re.search(r"^#define\s+PDGN_AUCTION_MAX_N\s+2048\s*$", header, flags=re.M)


def test_emd_switch_parses():
    from pdgn_amd import train
    base = ["--model_dir", "x"]
    assert train.parse_args(base).emd == "approx"
    assert train.parse_args(base + ["--emd", "auction"]).emd == "auction"
    assert train.parse_args(base + ["--emd", "approx", "--phase", "test"]).emd == "approx"
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--emd", "hungarian"])


def test_host_api_refuses_unequal_sizes_and_unknown_kinds():
    import torch
    from pdgn_amd import evaluation
    from pdgn_amd._lib import PdgnHipError
    from pdgn_amd.structural_losses import auction_match, exact_emd_cost
    with pytest.raises(PdgnHipError):                            # no CPU path
        auction_match(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3))
    with pytest.raises(ValueError):                              # unequal point counts: the approximate EMD's ground
        auction_match(torch.zeros(1, 8, 3), torch.zeros(1, 9, 3))
    with pytest.raises(ValueError):
        exact_emd_cost(torch.zeros(1, 8, 3, requires_grad=True), torch.zeros(1, 9, 3))
    with pytest.raises(ValueError):
        evaluation.compute_all_metrics(torch.zeros(2, 8, 3), torch.zeros(2, 8, 3), emd="exact")
    assert evaluation.EMD_KINDS == ("approx", "auction")
