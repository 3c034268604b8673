"""CPU: the flatness regulariser, the part that needs no GPU -- the numpy mirror of csrc/flatness.hip
(tests/flatness_mirror.py) against the definition in fp64 (numpy.linalg.eigh), the definition against central differences of its own loss,
the exact cases, the poison rules and point classes, the in-degree skew, and the Python surface: losses.flatness' form errors, the command
line, the trainer's argument, flatness.csv."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

import flatness_mirror as fm
import normals_mirror as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24
BASE = ["--model_dir", "m"]
# Measured on the five seeded clouds of tests/normals_mirror.py, k = 8 and 16, eps = 0 and 1e-2 x the mean neighbourhood trace (the figures
# each run prints): the largest relative error of H x the relative gap is 7.24e-7, the largest relative L2 error of the gradient 7.16e-6
# (sphere512, k = 8: a clean sphere, whose gradient is what cancellation leaves of the terms), the largest relative error of the loss
# 3.49e-7.  Each bound is ten times its measured maximum, as section 7q's are: the margin covers other seeds, not other arithmetic.
H_GAP_BOUND = 7.24e-6
GRAD_BOUND = 7.16e-5
LOSS_BOUND = 3.49e-6


@pytest.fixture(scope="module")
def clouds():
    return nm.accuracy_clouds(0)


def _mean_trace(x, idx):
    return float(fm.define64(x[None], idx[None])["eig"][0].sum(axis=1).mean())


# ---------------------------------------------------------------------------- the mirror against the definition in fp64
@pytest.mark.parametrize("floor", [0.0, 1e-2])
@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("name", ["sphere512", "cube512", "noisy512", "sphere64", "blob256"])
def test_the_mirror_agrees_with_the_fp64_definition(clouds, name, k, floor):
    x = clouds[name]
    idx = nm.knn_indices(x, k)
    eps = floor * _mean_trace(x, idx)
    h_gap, grad, loss = fm.against_define64(x, idx, eps)
    print("%s k=%d eps=%.3g: H x gap %.3g (bound %.3g), gradient %.3g (bound %.3g), loss %.3g (bound %.3g)"
          % (name, k, eps, h_gap, H_GAP_BOUND, grad, GRAD_BOUND, loss, LOSS_BOUND))
    assert h_gap <= H_GAP_BOUND and grad <= GRAD_BOUND and loss <= LOSS_BOUND


def test_the_eigenvalues_are_the_normals_mirrors(clouds):
    x = clouds["noisy512"]
    idx = nm.knn_indices(x, 16)
    pts = fm.points(x, idx, 0.0)
    _, eig = nm.estimate_cloud(x, idx)
    assert nm.same_bits(pts["eig"], eig) and not pts["bad"].any() and not pts["degenerate"].any()
    with np.errstate(all="ignore"):
        assert nm.same_bits(pts["sigma"], eig[:, 0] / ((eig[:, 0] + eig[:, 1]) + eig[:, 2]))


# ---------------------------------------------------------------------------- finite differences
@pytest.mark.parametrize("lists", ["knn", "random"])
def test_the_definition_is_the_derivative_of_its_own_loss(clouds, lists):
    """Central differences (h = 1e-6, fp64) of define64's loss at five coordinates; the lists are held constant.  The truncation error
    is h^2 f''' / 6 and the rounding error 2^-53 loss / h, about 1e-11 for a loss of the order of 0.1: 1e-9 leaves two decades."""
    x = clouds["noisy512"][:256].astype(np.float64)
    rng = np.random.default_rng(1)
    idx, eps = (nm.knn_indices(x, 16), 0.0) if lists == "knn" else (fm.random_lists(rng, 1, 256, 16)[0], 1e-3)
    if lists == "random":
        assert (idx[::2, 1] == idx[::2, 0]).all()                   # repeats inside a list
    grad = fm.define64(x[None], idx[None], eps)["grad"][0]
    worst, h = 0.0, 1e-6
    for j, c in ((0, 0), (17, 1), (100, 2), (255, 0), (64, 2)):
        up, down = x.copy(), x.copy()
        up[j, c] += h
        down[j, c] -= h
        fd = (fm.define64(up[None], idx[None], eps)["loss"] - fm.define64(down[None], idx[None], eps)["loss"]) / (2 * h)
        worst = max(worst, abs(fd - grad[j, c]))
    print("%s lists: central differences against the formula %.3g (largest gradient entry %.3g)" % (lists, worst, np.abs(grad).max()))
    assert np.abs(grad).max() > 1e-3 and worst <= 1e-9


# ---------------------------------------------------------------------------- exact cases
def planar_grid():
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2) / 8.0
    return np.concatenate([g, np.full((64, 1), 0.25)], axis=1).astype(F)


def test_a_planar_grid_is_exactly_flat():
    """Section 7q's grid: l0 is an exact zero at every point, so every point is degenerate -- sigma, the loss and every gradient entry are
    exact (positive) zeros."""
    x = planar_grid()
    got = fm.flatness(x[None], nm.knn_indices(x, 9)[None])
    assert np.array_equal(got["sigma"], np.zeros((1, 64), F)) and got["degenerate"].tolist() == [64]
    assert got["loss"] == 0 and got["per_cloud"].tolist() == [0.0]
    assert np.array_equal(got["grad"], np.zeros((1, 64, 3), F)) and not np.signbit(got["grad"]).any() and not np.signbit(got["sigma"]).any()


def test_equal_points_are_degenerate_without_a_floor():
    x = np.tile(np.array([[0.375, -1.5, 0.0625]], F), (10, 1))      # dyadic coordinates, k a power of two: the mean is exact
    for k in (1, 4, 8):
        got = fm.flatness(x[None], nm.knn_indices(x, k)[None], 0.0)
        assert got["degenerate"].tolist() == [10] and got["loss"] == 0 and np.array_equal(got["grad"], np.zeros((1, 10, 3), F))
    got = fm.flatness(x[None], nm.knn_indices(x, 4)[None], 1e-3)     # a floor does not make them live: l0 is not positive
    assert got["degenerate"].tolist() == [10] and got["loss"] == 0


# ---------------------------------------------------------------------------- poison and classes
def _two_clouds(clouds):
    x = np.stack([clouds["sphere64"], clouds["noisy512"][:64]])
    return x, np.stack([nm.knn_indices(c, 8) for c in x])


def _rows_on_the_lists_of(idx, bad, n):
    on = idx[bad].reshape(-1)
    hit = np.zeros(n, bool)
    hit[on[(on >= 0) & (on < n)]] = True
    return hit


def test_an_index_outside_the_cloud_poisons_its_point_and_the_targets_on_its_list(clouds):
    x, idx = _two_clouds(clouds)
    clean = fm.flatness(x, idx)
    assert np.isfinite(clean["grad"]).all() and clean["degenerate"].tolist() == [0, 0]
    bad = idx.copy()
    bad[0, 5, 3], bad[0, 9, 0], bad[0, 11, 7] = 64, -1, 2 ** 31 - 1
    got = fm.flatness(x, bad)
    src = np.zeros(64, bool)
    src[[5, 9, 11]] = True
    assert np.array_equal(np.isnan(got["sigma"][0]), src) and nm.same_bits(got["sigma"][0][~src], clean["sigma"][0][~src])
    assert np.array_equal(np.isnan(got["grad"][0]).all(axis=1), _rows_on_the_lists_of(bad[0], src, 64))
    assert np.array_equal(np.isnan(got["grad"][0]).any(axis=1), np.isnan(got["grad"][0]).all(axis=1))
    assert np.isnan(got["per_cloud"][0]) and np.isnan(got["loss"]) and got["degenerate"].tolist() == [0, 0]
    for key in ("sigma", "grad", "per_cloud"):                      # the other cloud: every bit
        assert nm.same_bits(got[key][1], clean[key][1]), key


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_non_finite_coordinate_poisons_the_points_that_list_it(clouds, value):
    x, idx = _two_clouds(clouds)
    clean = fm.flatness(x, idx)
    y = x.copy()
    y[0, 20, 1] = value
    got = fm.flatness(y, idx)
    src = (idx[0] == 20).any(axis=1)
    assert 1 < src.sum() < 64
    assert np.array_equal(np.isnan(got["sigma"][0]), src) and nm.same_bits(got["sigma"][0][~src], clean["sigma"][0][~src])
    rows = _rows_on_the_lists_of(idx[0], src, 64)
    assert rows[20] and not rows.all()
    assert np.array_equal(np.isnan(got["grad"][0]).all(axis=1), rows) and np.isfinite(got["grad"][0][~rows]).all()
    assert np.isnan(got["per_cloud"][0]) and np.isnan(got["loss"])
    for key in ("sigma", "grad", "per_cloud"):
        assert nm.same_bits(got[key][1], clean[key][1]), key


# ---------------------------------------------------------------------------- in-degree skew
def _gather64(x, idx, pts, coef):
    """The gather of the mirror's own fp32 records in fp64, in no particular order -> (grad, the sum of the absolute values of each
    component's terms)."""
    n, k = idx.shape
    mu, h = pts["mu"].astype(np.float64), pts["h"].astype(np.float64)
    H = np.empty((n, 3, 3))
    for p, (a, b) in enumerate(fm.H_KEYS):
        H[:, a, b] = H[:, b, a] = h[:, p]
    d = x.astype(np.float64)[idx] - mu[:, None, :]                 # (n, k, 3)
    val, mag = np.zeros((n, 3)), np.zeros((n, 3))
    np.add.at(val, idx.reshape(-1), np.einsum("nij,nkj->nki", H, d).reshape(-1, 3))
    np.add.at(mag, idx.reshape(-1), np.einsum("nij,nkj->nki", np.abs(H), np.abs(d)).reshape(-1, 3))
    return float(coef) * val, abs(float(coef)) * mag


@pytest.mark.parametrize("targets", [1, 4])
def test_skewed_in_degrees(clouds, targets):
    """Lists whose every entry is 0 (one target with n k in-edges, no other has one), and lists confined to the targets 0 .. 3 (collisions
    inside every run of 64 edges).  A target without in-edges has a gradient of exactly +0.  The rows that have some are compared with the
    same records summed in fp64 in no order: a row of m terms is added one after the other (m u of the sum of the absolute values, to
    first order) and every term carries the difference's rounding and the five of dot3, so (m + 6) u sum |H| |d|, plus the coefficient's u."""
    x = clouds["noisy512"][:257]
    rng = np.random.default_rng(3)
    n, k = 257, 16
    idx = np.zeros((n, k), np.int32) if targets == 1 else rng.integers(0, 4, size=(n, k)).astype(np.int32)
    coef = fm.coef_of(2, n)
    pts = fm.points(x, idx, 1e-4)
    grad = fm.gather(x, idx, pts["mu"], pts["h"], coef)
    assert np.array_equal(grad[targets:], np.zeros((n - targets, 3), F)) and not np.signbit(grad[targets:]).any()
    assert np.isfinite(grad).all()
    want, mag = _gather64(x, idx, pts, coef)
    m = np.bincount(idx.reshape(-1), minlength=n)[:, None]
    assert m[:targets].sum() == n * k and (targets == 1 or m[:4].min() > 64)
    err, bound = np.abs(grad.astype(np.float64) - want), (m + 7) * U * mag
    print("%d targets: worst error / bound %.3g" % (targets, (err[:targets] / np.maximum(bound[:targets], 1e-300)).max()))
    assert (err <= bound).all()


# ---------------------------------------------------------------------------- the Python surface
def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    from pdgn_amd import _lib, build, losses
    text = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    handle = ctypes.CDLL(build.build())
    vp, ll, f, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float, ctypes.c_int
    assert _lib.SIGNATURES["pdgn_flatness"] == (i, (i, i, i, vp, vp, f, f, vp, vp, vp, vp, vp, vp, vp))
    assert _lib.SIGNATURES["pdgn_flatness_workspace_bytes"] == (ll, (i, i, i, i))
    assert hasattr(handle, "pdgn_flatness") and hasattr(handle, "pdgn_flatness_workspace_bytes")
    define = re.findall(r"^#define\s+PDGN_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M)
    assert len(define) == 1 and int(define[0]) == _lib.ABI_VERSION == handle.pdgn_abi_version() >= 49
    assert losses.FLATNESS_MAX_K == nm.MAX_K == int(re.search(r"#define PDGN_NORMALS_MAX_K (\d+)", text).group(1))
    size = handle.pdgn_flatness_workspace_bytes
    size.restype, size.argtypes = ll, (i, i, i, i)                  # (host only: no device work)
    assert size(2, 100, 8, 0) == 0 and size(2, 100, 8, 1) == 2 * 100 * 48 + 4 * 2 * (2 * 100 + 1 + 800)
    for bad in ((0, 100, 8), (2, 0, 8), (2, 100, 0), (2, 100, 65), (1 << 15, 1 << 12, 16)):
        assert size(*bad, 1) == -1 and size(*bad, 0) == -1, bad
    hip = open(os.path.join(ROOT, "pdgn_amd", "csrc", "flatness.hip")).read()
    assert "NORMATIVE DEFINITION" in hip and '#include "pca3.h"' in hip
    assert '#include "pca3.h"' in open(os.path.join(ROOT, "pdgn_amd", "csrc", "normals.hip")).read()


def test_the_op_refuses_a_wrong_form_before_it_reaches_the_device():
    import torch
    from pdgn_amd import losses
    from pdgn_amd._lib import PdgnHipError
    x = torch.zeros(2, 32, 3)
    for bad in (torch.zeros(3, 4), torch.zeros(2, 4, 5), "cloud"):
        with pytest.raises(ValueError):
            losses.flatness(bad)
    for k in (0, 33, 65, 2.0, True):
        with pytest.raises(ValueError):
            losses.flatness(x, k=k)
    for eps in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            losses.flatness(x, k=8, eps=eps)
        with pytest.raises(ValueError):
            losses.flatness_pass(x, torch.zeros(2, 32, 8, dtype=torch.int32), eps=eps)
    for idx in (torch.zeros(2, 32, 8), torch.zeros(2, 31, 8, dtype=torch.int32), torch.zeros(2, 32, 65, dtype=torch.int32),
                torch.zeros(2, 32, dtype=torch.int32), np.zeros((2, 32, 8), np.int32)):
        with pytest.raises(ValueError):
            losses.flatness(x, idx=idx)
    with pytest.raises(PdgnHipError):                               # the form is fine: the host tensors are what is refused
        losses.flatness(x, k=8)
    with pytest.raises(PdgnHipError):
        losses.flatness(x.transpose(1, 2), idx=torch.zeros(2, 32, 8, dtype=torch.int32))
    assert losses.flatness_floors(1e-3, (256, 512, 1024, 2048)) == [8e-3, 4e-3, 2e-3, 1e-3]
    for bad in ((-1.0, (4, 8)), (1.0, ()), (1.0, (0, 8)), (float("nan"), (4, 8))):
        with pytest.raises(ValueError):
            losses.flatness_floors(*bad)


def test_the_parser_takes_the_flags_and_the_default_namespace_is_what_it_was(capsys):
    from pdgn_amd import train
    args = train.parse_args(BASE)
    assert args.flatness is None and args.flatness_k == 16 and args.flatness_eps is None and args.flatness_eps_factor == 1e-2
    assert not any(k.startswith("flatness") for k in vars(args)) and "flatness" not in str(train.logged_args(args))
    assert train.flatness_arg(args) is None
    got = train.parse_args(BASE + ["--flatness", "0.05", "--flatness_eps", "1e-4", "--flatness_levels", "4,2", "--flatness_k", "12"])
    assert train.flatness_arg(got) == {"weight": 0.05, "k": 12, "eps": 1e-4, "levels": (1, 3)} and "flatness=0.05" in str(train.logged_args(got))
    got = train.parse_args(BASE + ["--flatness", "0.5", "--flatness_eps_factor", "0.1"])
    assert train.flatness_arg(got, eps=2e-5) == {"weight": 0.5, "k": 16, "eps": 2e-5, "levels": (0, 1, 2, 3)} and got.flatness_eps_factor == 0.1
    both = train.parse_args(BASE + ["--flatness", "0.5", "--flatness_eps", "0", "--repulsion", "0.1", "--repulsion_radius", "0.05"])
    assert train.flatness_arg(both)["eps"] == 0.0 and train.repulsion_arg(both)["radius"] == 0.05
    wants = {"needs --flatness": (["--flatness_k", "8"], ["--flatness_eps", "0.1"], ["--flatness_eps_factor", "2"], ["--flatness_levels", "1"]),
             "a finite weight, not negative": (["--flatness", "-1"], ["--flatness", "nan"], ["--flatness", "inf"]),
             "a finite floor, not negative": (["--flatness", "1", "--flatness_eps=-1e-3"], ["--flatness", "1", "--flatness_eps", "inf"]),
             "does not go with --flatness_eps": (["--flatness", "1", "--flatness_eps", "0.1", "--flatness_eps_factor", "2"],),
             "a finite factor, not negative": (["--flatness", "1", "--flatness_eps_factor=-1"], ["--flatness", "1", "--flatness_eps_factor", "nan"]),
             "--flatness_levels:": (["--flatness", "1", "--flatness_levels", "0,1"], ["--flatness", "1", "--flatness_levels", "1,5"],
                                    ["--flatness", "1", "--flatness_levels", "2,2"], ["--flatness", "1", "--flatness_levels", "a"],
                                    ["--flatness", "1", "--flatness_levels", ""]),
             "--flatness_k": (["--flatness", "1", "--flatness_k", "0"], ["--flatness", "1", "--flatness_k", "65"],
                              ["--flatness", "1", "--flatness_k", "64", "--num_point", "256"],        # level 1 has 32 points
                              ["--flatness", "1", "--flatness_k", "64", "--num_point", "256", "--flatness_levels", "1,4"])}
    for message, cases in wants.items():
        for bad in cases:
            with pytest.raises(SystemExit):
                train.parse_args(BASE + bad)
            assert message in capsys.readouterr().err, bad
    assert train.parse_args(BASE + ["--flatness", "1", "--flatness_k", "64", "--num_point", "256", "--flatness_levels", "2,4"]).flatness_k == 64
    for dest in ("flatness", "flatness_k", "flatness_eps", "flatness_eps_factor", "flatness_levels"):
        action = [a for a in train.build_parser()._actions if a.dest == dest]
        assert len(action) == 1 and action[0].default is argparse.SUPPRESS, dest
    assert "--flatness" in train.__doc__


def test_the_flags_reach_the_trainer_only_in_the_train_phase(monkeypatch):
    from pdgn_amd import train, trainer
    got = {}
    monkeypatch.setattr(trainer, "PDGNTrainer", lambda **kw: (got.clear(), got.update(kw))[0] or "trainer")
    args = train.parse_args(BASE + ["--flatness", "0.1", "--flatness_eps", "0.2"])
    assert train.make_trainer(args, "cpu", None, None, flatness=train.flatness_arg(args)) == "trainer"
    assert got["flatness"] == {"weight": 0.1, "k": 16, "eps": 0.2, "levels": (0, 1, 2, 3)}
    assert train.make_trainer(train.parse_args(BASE), "cpu") == "trainer" and "flatness" not in got
    args = train.parse_args(BASE + ["--phase", "test", "--flatness", "0.1", "--flatness_eps", "0.2"])
    assert train.make_trainer(args, "cpu", None, None, flatness=train.flatness_arg(args)) == "trainer" and "flatness" not in got


def test_check_flatness(monkeypatch):
    from pdgn_amd import trainer

    def never(*a, **k):
        raise AssertionError("a network was built")

    monkeypatch.setattr(trainer, "PointGenerator", never)
    monkeypatch.setattr(trainer, "PointDiscriminator", never)
    check = trainer.PDGNTrainer._check_flatness
    assert check({"weight": 0.5}) == {"weight": 0.5, "k": 16, "eps": 0.0, "levels": (0, 1, 2, 3)}
    assert check({"weight": 0, "k": 64, "eps": 1e-3, "levels": [1, 3]}) == {"weight": 0.0, "k": 64, "eps": 1e-3, "levels": (1, 3)}
    good = {"weight": 0.1, "k": 8, "eps": 1e-4}
    for bad in (0.1, "on", {}, {"k": 8}, dict(good, weight=-1.0), dict(good, weight=float("nan")), dict(good, weight=float("inf")),
                dict(good, k=0), dict(good, k=65), dict(good, k=8.0), dict(good, k=True), dict(good, eps=-1e-9), dict(good, eps=float("inf")),
                dict(good, eps=float("nan")), dict(good, levels=()), dict(good, levels=(0, 4)), dict(good, levels=(-1,)),
                dict(good, levels=(1, 1)), dict(good, levels=(2, 1)), dict(good, radius=0.1)):
        with pytest.raises(ValueError):
            trainer.PDGNTrainer(device="cuda:0", distributed=False, flatness=bad)
    with pytest.raises(AssertionError, match="a network was built"):     # a good one gets as far as the networks
        trainer.PDGNTrainer(device="cuda:0", distributed=False, flatness=dict(good, levels=(1, 3)))


def test_a_cpu_trainer_with_and_without_the_term():
    from pdgn_amd.generator import PointGenerator
    from pdgn_amd.trainer import PDGNTrainer
    make = lambda **kw: PDGNTrainer(device="cpu", distributed=False, base_points=16, generator=PointGenerator(256, 20, base_points=16), **kw)
    tr = make()
    assert tr.flatness is None and not [k for k in vars(tr) if "flat" in k and k != "flatness"]
    assert tr._lw[1].tolist() == pytest.approx([1.2, 1.2, 1.2, 1.0, 0.1])
    for call in (tr.flatness_state, lambda: tr.set_flatness(weight=1.0)):
        with pytest.raises(RuntimeError):
            call()
    on = make(flatness={"weight": 0.25, "k": 8, "eps": 1e-3, "levels": (1, 3)})
    assert on.flatness == {"weight": 0.25, "k": 8, "eps": 1e-3, "levels": (1, 3)}
    assert on._lw[1].tolist() == pytest.approx([1.2, 1.2, 1.2, 1.0, 0.1, 0.25]) and on._flat_buf.tolist() == [0.0] * 4
    both = make(repulsion={"weight": 0.5, "radius": 0.05}, flatness={"weight": 0.25})
    assert both._lw[1].tolist() == pytest.approx([1.2, 1.2, 1.2, 1.0, 0.1, 0.5, 0.25])
    both.set_repulsion(weight=0.75)                              # each setter writes its own entry and no other
    assert both._lw[1].tolist() == pytest.approx([1.2, 1.2, 1.2, 1.0, 0.1, 0.75, 0.25])
    both.set_flatness(weight=0.125)
    assert both._lw[1].tolist() == pytest.approx([1.2, 1.2, 1.2, 1.0, 0.1, 0.75, 0.125])
    on.set_flatness(weight=0.5)
    assert on.flatness["weight"] == 0.5 and on._lw[1][5].item() == 0.5
    on.set_flatness(k=12, eps=2e-3)                              # no captured list: allowed
    assert (on.flatness["k"], on.flatness["eps"]) == (12, 2e-3) and on._flatness_floors((32, 64, 128, 256)) == [16e-3, 8e-3, 4e-3, 2e-3]
    on._list = object()
    for change in ({"k": 8}, {"eps": 1e-3}):
        with pytest.raises(RuntimeError):
            on.set_flatness(**change)
    on.set_flatness(weight=0.0, k=12)                            # the weight still may (and an unchanged k)
    assert on._lw[1][5].item() == 0.0
    for bad in ({"weight": -1.0}, {"k": 0}, {"eps": -1.0}):
        with pytest.raises(ValueError):
            on.set_flatness(**bad)
    state = on.flatness_state()
    assert state["per_level"] == [0.0] * 4 and state["total"] == 0.0 and state["degenerate"] == 0 and state["levels"] == (1, 3)


def test_fit_writes_flatness_csv_only_with_the_term(tmp_path):
    """pdgn_amd.fit on a duck-typed trainer: one row per epoch from flatness_state(); no file without the term."""
    import torch
    from pdgn_amd import fit

    class Feeder:
        batches_per_epoch, rank = 2, 0

        def buffers(self):
            return [torch.zeros(1)] * 4, torch.zeros(1), torch.zeros(1)

        def fill(self, *a):
            pass

    class Stub:
        LOG_FORMAT, LOSS_KEYS = fit.LOG_FORMAT, fit.LOSS_KEYS
        device = torch.device("cpu")

        def __init__(self, flatness):
            self.flatness, self.steps = flatness, 0

        def step(self, *a):
            self.steps += 1
            return {k: torch.tensor(float(self.steps)) for k in self.LOSS_KEYS}

        def flatness_state(self):
            return dict(self.flatness, per_level=[0.0, 0.25, 0.0, float(self.steps)], total=0.25 + self.steps, degenerate=3 * self.steps)

    log = tmp_path / "on" / "log.txt"
    log.parent.mkdir()
    fit.fit(Stub({"weight": 0.1, "k": 16, "eps": 0.002, "levels": (1, 3)}), Feeder(), 2, issue="eager", log=str(log))
    rows = (log.parent / "flatness.csv").read_text().splitlines()
    assert rows == ["epoch,weight,k,eps,total,level1,level2,level3,level4,degenerate", "1,0.1,16,0.002,2.25,0,0.25,0,2,6",
                    "2,0.1,16,0.002,4.25,0,0.25,0,4,12"]
    off = tmp_path / "off" / "log.txt"
    off.parent.mkdir()
    fit.fit(Stub(None), Feeder(), 1, issue="eager", log=str(off))
    assert sorted(p.name for p in off.parent.iterdir()) == ["log.txt"]
