"""CPU: the repulsion regulariser and the spacing statistics, the part that needs no GPU -- the header's three
prototypes, the numpy mirror (tests/repulsion_mirror.py) against closed forms and against an fp64 torch restatement with autograd, the
data-parallel identity, losses.repulsion_radii, the command line, and the trainer's argument."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

import repulsion_mirror as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BASE = ["--model_dir", "m"]


def _ulps(a, b):
    a, b = F(a), F(b)
    return abs(float(a) - float(b)) / float(np.spacing(max(abs(a), abs(b))))


# ---------------------------------------------------------------------------- the header
def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    from pdgn_amd import _lib, build, losses
    text = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(build.build())
    vp, ll, f, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float, ctypes.c_int
    want = {"pdgn_repulsion_chunk": (), "pdgn_repulsion": (i, i, vp, f, f, vp, vp, vp, vp, vp, vp),
            "pdgn_repulsion_backward": (ll, vp, vp, vp, vp)}
    for name, argtypes in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert _lib.SIGNATURES[name] == (ctypes.c_int, argtypes), name
        assert hasattr(handle, name), name
    assert re.findall(r"^#define\s+PDGN_REPULSION_MAX_N\s+(\d+)\s*$", code, flags=re.M) == [str(losses.REPULSION_MAX_POINTS)] == ["8192"]
    define = re.findall(r"^#define\s+PDGN_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M)
    assert len(define) == 1 and int(define[0]) == _lib.ABI_VERSION == handle.pdgn_abi_version() >= 42
    assert 1 <= handle.pdgn_repulsion_chunk() <= losses.REPULSION_MAX_POINTS          # (host only: no device work)
    assert "%d entry points" % len(_lib.SIGNATURES) in open(os.path.join(ROOT, "README.md")).read()
    hip = open(os.path.join(ROOT, "pdgn_amd", "csrc", "repulsion.hip")).read()
    assert "atomic" not in hip.split("#include")[1] and "NORMATIVE OPERATION ORDER" in hip


def test_the_constants_are_computed_in_fp64_and_rounded_once():
    from pdgn_amd import losses
    for h, b, n in ((0.3, 35, 2048), (1.0, 1, 2), (0.0123, 3, 257)):
        inv, coef = losses.repulsion_constants(h, b, n)
        assert isinstance(inv, float) and inv == 1.0 / (h * h) and coef == -8.0 * inv / (b * n)
        assert rm.constants(h, b, n) == (F(inv), F(coef))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            losses.repulsion_constants(bad, 1, 2)


# ---------------------------------------------------------------------------- closed forms
def test_two_points_inside_the_radius():
    """d = 1/2, h = 1: t = 3/4 exactly, s_0 = s_1 = 9/16, the loss of the cloud of two (1/2)(2 t^2) = 9/16, and
    dL/dx_0 = 2 t (-2 d / h^2) = -3/2 along the difference: all exact in fp32."""
    x = np.array([[[0.5, 0.0, 0.0], [0.0, 0.0, 0.0]]], dtype=F)
    r = rm.repulsion(x, 1.0)
    assert r["loss"] == F(0.5625) and r["per_cloud"].tolist() == [0.5625] and r["s"].tolist() == [[0.5625, 0.5625]]
    assert r["grad"].tolist() == [[[-1.5, 0.0, 0.0], [1.5, 0.0, 0.0]]]
    assert r["nn2"].tolist() == [[0.25, 0.25]] and r["inside"] == 1.0
    # a general pair: L = (1 - d^2 / h^2)^2 to rounding
    a, b, h = np.array([0.1, -0.2, 0.3]), np.array([0.25, 0.1, 0.2]), 0.7
    d2 = float(((a - b) ** 2).sum())
    r = rm.repulsion(np.array([[a, b]], dtype=F), h)
    want = (1.0 - d2 / (h * h)) ** 2
    assert abs(float(r["loss"]) - want) <= 16 * rm.U * want


def test_two_points_at_or_beyond_the_radius_give_exactly_zero():
    for d in (1.0, 1.5, 1024.0):                                  # d = h exactly: t = 0 fails !(t <= 0)
        r = rm.repulsion(np.array([[[d, 0.0, 0.0], [0.0, 0.0, 0.0]]], dtype=F), 1.0)
        assert r["loss"] == 0.0 and not r["s"].any() and not r["grad"].any() and not np.signbit(r["s"]).any()
        assert r["nn2"].tolist() == [[d * d, d * d]] and r["inside"] == 0.0


def test_a_single_point_has_no_neighbour():
    r = rm.repulsion(np.array([[[1.0, 2.0, 3.0]]], dtype=F), 0.5)
    assert r["loss"] == 0.0 and r["per_cloud"].tolist() == [0.0] and not r["grad"].any()
    assert np.isposinf(r["nn2"]).all() and r["nn2"].shape == (1, 1)


def test_duplicate_points_add_one_each_and_no_gradient():
    p = [0.25, -0.5, 0.125]
    r = rm.repulsion(np.array([[p, p, [10.0, 10.0, 10.0]]], dtype=F), 1.0)
    assert r["s"].tolist() == [[1.0, 1.0, 0.0]] and not r["grad"].any()
    assert r["nn2"][0, :2].tolist() == [0.0, 0.0] and r["nn2"][0, 2] > 100.0
    st = rm.spacing_stats(np.array([[p, p, [10.0, 10.0, 10.0]], [[0, 0, 0], [1, 0, 0], [3, 0, 0]]], dtype=F))
    assert st["duplicates"] == 2 and st["nn_min"] == 0.0
    # three copies: each sees two others
    r = rm.repulsion(np.array([[p, p, p]], dtype=F), 1.0)
    assert r["s"].tolist() == [[2.0, 2.0, 2.0]] and r["loss"] == 2.0


def test_a_nan_coordinate_is_a_nan_loss_for_its_cloud_only():
    x = np.random.default_rng(3).normal(size=(2, 9, 3)).astype(F)
    x[1, 4, 1] = np.nan
    r = rm.repulsion(x, 1.5)
    assert np.isnan(r["loss"]) and np.isnan(r["per_cloud"][1]) and np.isfinite(r["per_cloud"][0])
    assert np.isnan(r["grad"][1]).all() and np.isfinite(r["grad"][0]).all() and np.isnan(r["s"][1]).all()


def test_the_spacing_statistics_of_a_line():
    """Points at 0, 1, 3 and 0, 2, 4, 8 on a line: nearest distances (1, 1, 2) and (2, 2, 2, 4)."""
    a = np.zeros((1, 3, 3), F)
    a[0, :, 0] = [0, 1, 3]
    st = rm.spacing_stats(a)
    d = np.array([1.0, 1.0, 2.0])
    assert st["nn_mean"] == d.mean() and abs(st["nn_cv"] - d.std() / d.mean()) < 1e-15 and st["nn_min"] == 1.0 and st["duplicates"] == 0


# ---------------------------------------------------------------------------- the fp64 restatement
def test_the_mirror_is_the_fp64_restatement_within_the_derived_bound():
    n, h = 200, 2.0                                              # unit-normal clouds: |x_i - x_j|^2 / 2 is chi-squared with 3 degrees, 43 % below 2
    x = np.random.default_rng(11).normal(size=(2, n, 3)).astype(F)
    got, ref = rm.repulsion(x, h), rm.restate64(x, h)
    assert 0.1 < got["inside"] < 0.9
    bound = rm.bounds(ref, n)
    err_g = np.abs(got["grad"].astype(np.float64) - ref["grad"])
    err_s = np.abs(got["s"].astype(np.float64) - ref["s"])
    err_l = abs(float(got["loss"]) - ref["loss"])
    print("N = %d: largest grad error / bound %.3g, s error / bound %.3g, loss error / bound %.3g"
          % (n, rm.worst(err_g, bound["grad"]), rm.worst(err_s, bound["s"]), err_l / bound["loss"]))
    assert (bound["grad"] > 0).mean() > 0.9 and (err_g <= bound["grad"]).all()       # (a point with nobody inside its radius: 0 <= 0)
    assert (err_s <= bound["s"]).all() and err_l <= bound["loss"]
    assert (np.abs(got["nn2"].astype(np.float64) - ref["nn2"]) <= 8 * rm.U * ref["nn2"]).all()
    per = ref["s"].mean(axis=1)
    assert (np.abs(got["per_cloud"].astype(np.float64) - per) <= (n + n / 64.0 + 16) * rm.U * per).all()


def test_the_reduction_runs_in_the_stated_order():
    """Lane 0 adds s[0], s[64], s[128] one after the other before the butterfly: with 2^24 first, a 1 behind it on the same lane is lost and
    a 1 on another lane is not."""
    s = np.zeros(130, F)
    s[0], s[64], s[128] = 2.0 ** 24, 1.0, 1.0
    assert rm.wave_sum(s) == F(2.0 ** 24)
    s[64], s[128], s[1], s[33] = 0.0, 0.0, 1.0, 1.0              # lanes 1 and 33 join at the first stage (1 + 1), lane 0 meets them at the last
    assert rm.wave_sum(s) == F(2.0 ** 24 + 2.0)
    loss, per = rm.reduce(np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], F))
    assert loss == F(3.5) and per.tolist() == [2.0, 5.0]


# ---------------------------------------------------------------------------- data parallelism
def test_a_batch_of_2b_clouds_is_the_mean_of_its_halves():
    """The term is a batch mean: two ranks' values averaged (what the mean all-reduce of the gradients corresponds to) are one rank's at
    twice the batch -- to 2 ulp for the loss; the gradients of a half are exactly twice the whole batch's (coef has b in it: a power of 2)."""
    x = np.random.default_rng(5).normal(size=(4, 65, 3)).astype(F)
    whole, lo, hi = rm.repulsion(x, 0.8), rm.repulsion(x[:2], 0.8), rm.repulsion(x[2:], 0.8)
    mean = F(F(lo["loss"] + hi["loss"]) / F(2))
    assert _ulps(whole["loss"], mean) <= 2, (whole["loss"], mean)
    assert np.array_equal(whole["per_cloud"], np.concatenate([lo["per_cloud"], hi["per_cloud"]]))
    assert np.array_equal(whole["grad"] * F(2), np.concatenate([lo["grad"], hi["grad"]]))


# ---------------------------------------------------------------------------- radii
def test_the_radius_of_a_level_follows_the_square_root_of_its_point_count():
    from pdgn_amd import losses
    assert losses.repulsion_radii(0.05, (256, 512, 1024, 2048)) == [0.05 * 8 ** 0.5, 0.05 * 2.0, 0.05 * 2 ** 0.5, 0.05]
    assert losses.repulsion_radii(1.0, [2048]) == [1.0] and losses.repulsion_radii(2.0, (512, 128)) == [2.0, 4.0]
    for bad in ((0.0, (1, 2)), (-1.0, (1, 2)), (float("nan"), (1, 2)), (float("inf"), (2,)), (1.0, ()), (1.0, (0, 4))):
        with pytest.raises(ValueError):
            losses.repulsion_radii(*bad)


def test_the_op_refuses_what_is_not_a_cloud_before_it_reaches_the_library():
    import torch
    from pdgn_amd import losses
    for bad in (torch.zeros(3, 4), torch.zeros(2, 4, 5), "cloud"):
        with pytest.raises(ValueError):
            losses.repulsion(bad, 1.0)


# ---------------------------------------------------------------------------- the command line
def test_the_parser_takes_the_flags_and_the_default_namespace_is_what_it_was(capsys):
    from pdgn_amd import train
    args = train.parse_args(BASE)
    assert args.repulsion is None and args.repulsion_radius is None and args.repulsion_radius_factor == 1.0 and not args.report_spacing
    assert not any(k.startswith("repulsion") or k == "report_spacing" for k in vars(args)) and "repulsion" not in str(train.logged_args(args))
    assert train.repulsion_arg(args) is None
    got = train.parse_args(BASE + ["--repulsion", "0.05", "--repulsion_radius", "0.04", "--repulsion_levels", "4,2"])
    assert train.repulsion_arg(got) == {"weight": 0.05, "radius": 0.04, "levels": (1, 3)} and "repulsion=0.05" in str(train.logged_args(got))
    got = train.parse_args(BASE + ["--repulsion", "0.5", "--repulsion_radius_factor", "1.5"])
    assert train.repulsion_arg(got, radius=0.03) == {"weight": 0.5, "radius": 0.03, "levels": (0, 1, 2, 3)} and got.repulsion_radius_factor == 1.5
    assert train.parse_args(BASE + ["--report_every", "5", "--report_spacing"]).report_spacing is True
    for bad in (["--repulsion_radius", "0.1"], ["--repulsion_levels", "1"], ["--repulsion_radius_factor", "2"], ["--repulsion", "-1"],
                ["--repulsion", "nan"], ["--repulsion", "inf"], ["--repulsion", "1", "--repulsion_radius", "0"],
                ["--repulsion", "1", "--repulsion_radius", "-2"], ["--repulsion", "1", "--repulsion_radius", "0.1", "--repulsion_radius_factor", "2"],
                ["--repulsion", "1", "--repulsion_radius_factor", "0"], ["--repulsion", "1", "--repulsion_levels", "0,1"],
                ["--repulsion", "1", "--repulsion_levels", "1,5"], ["--repulsion", "1", "--repulsion_levels", "2,2"],
                ["--repulsion", "1", "--repulsion_levels", "a"], ["--repulsion", "1", "--repulsion_levels", ""],
                ["--repulsion", "1", "--num_point", "16384"], ["--report_spacing"]):
        with pytest.raises(SystemExit):
            train.parse_args(BASE + bad)
        assert "error" in capsys.readouterr().err, bad
    for dest in ("repulsion", "repulsion_radius", "repulsion_radius_factor", "repulsion_levels", "report_spacing"):
        action = [a for a in train.build_parser()._actions if a.dest == dest]
        assert len(action) == 1 and action[0].default is argparse.SUPPRESS, dest
    assert "--repulsion" in train.__doc__


def test_the_flags_reach_the_trainer_only_in_the_train_phase(monkeypatch):
    from pdgn_amd import train, trainer
    got = {}
    monkeypatch.setattr(trainer, "PDGNTrainer", lambda **kw: got.update(kw) or "trainer")
    args = train.parse_args(BASE + ["--repulsion", "0.1", "--repulsion_radius", "0.2"])
    assert train.make_trainer(args, "cpu", None, train.repulsion_arg(args)) == "trainer"
    assert got["repulsion"] == {"weight": 0.1, "radius": 0.2, "levels": (0, 1, 2, 3)}
    assert train.make_trainer(train.parse_args(BASE), "cpu") == "trainer" and got["repulsion"] is None
    args = train.parse_args(BASE + ["--phase", "test", "--repulsion", "0.1", "--repulsion_radius", "0.2"])
    assert train.make_trainer(args, "cpu", None, train.repulsion_arg(args)) == "trainer" and got["repulsion"] is None


# ---------------------------------------------------------------------------- the trainer
def test_the_trainer_refuses_a_bad_argument_before_it_builds_anything(monkeypatch):
    from pdgn_amd import trainer

    def never(*a, **k):
        raise AssertionError("a network was built")

    monkeypatch.setattr(trainer, "PointGenerator", never)
    monkeypatch.setattr(trainer, "PointDiscriminator", never)
    good = {"weight": 0.1, "radius": 0.05}
    for bad in (0.1, "on", {}, {"weight": 0.1}, {"radius": 0.1}, dict(good, weight=-1.0), dict(good, weight=float("nan")),
                dict(good, weight=float("inf")), dict(good, radius=0.0), dict(good, radius=-1.0), dict(good, radius=float("inf")),
                dict(good, radius=float("nan")), dict(good, levels=()), dict(good, levels=(0, 4)), dict(good, levels=(-1,)),
                dict(good, levels=(1, 1)), dict(good, levels=(2, 1)), dict(good, per_level=(1, 1, 1, 1))):
        with pytest.raises(ValueError):
            trainer.PDGNTrainer(device="cuda:0", distributed=False, repulsion=bad)
    with pytest.raises(AssertionError, match="a network was built"):     # a good one gets as far as the networks
        trainer.PDGNTrainer(device="cuda:0", distributed=False, repulsion=dict(good, levels=(1, 3)))


def test_a_cpu_trainer_without_the_term_has_nothing_of_it():
    from pdgn_amd.generator import PointGenerator
    from pdgn_amd.trainer import PDGNTrainer
    make = lambda **kw: PDGNTrainer(device="cpu", distributed=False, base_points=16, generator=PointGenerator(256, 20, base_points=16), **kw)
    tr = make()
    assert tr.repulsion is None and not [k for k in vars(tr) if "rep" in k and k != "repulsion"]
    assert tr._lw[1].tolist() == pytest.approx([1.2, 1.2, 1.2, 1.0, 0.1])
    for call in (tr.repulsion_state, lambda: tr.set_repulsion(weight=1.0)):
        with pytest.raises(RuntimeError):
            call()
    on = make(repulsion={"weight": 0.25, "radius": 0.05, "levels": (1, 3)})
    assert on.repulsion == {"weight": 0.25, "radius": 0.05, "levels": (1, 3)}
    assert on._lw[1].tolist() == pytest.approx([1.2, 1.2, 1.2, 1.0, 0.1, 0.25]) and on._rep_buf.tolist() == [0.0] * 4
    on.set_repulsion(weight=0.5)
    assert on.repulsion["weight"] == 0.5 and on._lw[1][5].item() == 0.5 and on._lw[1][:5].tolist() == pytest.approx([1.2, 1.2, 1.2, 1.0, 0.1])
    on.set_repulsion(radius=0.07)                                # no captured list: allowed
    assert on.repulsion["radius"] == 0.07 and on._repulsion_radii((32, 64, 128, 256))[3] == 0.07
    on._list = object()
    with pytest.raises(RuntimeError):
        on.set_repulsion(radius=0.08)
    on.set_repulsion(weight=0.0)                                 # the weight still may
    assert on._lw[1][5].item() == 0.0
    for bad in ({"weight": -1.0}, {"radius": 0.0}):
        with pytest.raises(ValueError):
            on.set_repulsion(**bad)
    state = on.repulsion_state()
    assert state["per_level"] == [0.0] * 4 and state["total"] == 0.0 and state["weight"] == 0.0 and state["levels"] == (1, 3)


def test_fit_writes_repulsion_csv_only_with_the_term(tmp_path):
    """pdgn_amd.fit on a duck-typed trainer: one row per epoch from repulsion_state(); no file without the term."""
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

        def __init__(self, repulsion):
            self.repulsion, self.steps = repulsion, 0

        def step(self, *a):
            self.steps += 1
            return {k: torch.tensor(float(self.steps)) for k in self.LOSS_KEYS}

        def repulsion_state(self):
            return dict(self.repulsion, per_level=[0.0, 1.5, 0.0, float(self.steps)], total=1.5 + self.steps)

    log = tmp_path / "on" / "log.txt"
    log.parent.mkdir()
    fit.fit(Stub({"weight": 0.1, "radius": 0.05, "levels": (1, 3)}), Feeder(), 2, issue="eager", log=str(log))
    rows = (log.parent / "repulsion.csv").read_text().splitlines()
    assert rows == ["epoch,weight,radius,total,level1,level2,level3,level4", "1,0.1,0.05,3.5,0,1.5,0,2", "2,0.1,0.05,5.5,0,1.5,0,4"]
    off = tmp_path / "off" / "log.txt"
    off.parent.mkdir()
    fit.fit(Stub(None), Feeder(), 1, issue="eager", log=str(off))
    assert sorted(p.name for p in off.parent.iterdir()) == ["log.txt"]
