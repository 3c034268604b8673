"""CPU: the choice of adversarial objective, the part that needs no GPU -- the header's three prototypes and five
constants, what losses.adversarial hands to mse_const under "lsgan", the refusals, the numpy mirror (tests/gan_mirror.py) against its own
fp64 closed forms and a finite difference, the command line, and the trainer's argument."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

import gan_mirror as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(k, r) for k in ("hinge", "logistic") for r in ("d_real", "d_fake", "g")]


# ---------------------------------------------------------------------------- the header
def test_the_header_declares_the_three_entry_points_and_the_library_exports_them():
    from pdgn_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(build.build())
    vp, ll, f, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float, ctypes.c_int
    want = {"pdgn_gan_term": (ll, vp, i, i, f, vp, vp),
            "pdgn_gan_term_count": (ll, vp, i, i, f, f, vp, vp, vp),
            "pdgn_gan_term_backward": (ll, vp, i, i, f, vp, vp, vp)}
    for name, argtypes in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert _lib.SIGNATURES[name] == (ctypes.c_int, argtypes), name
        assert hasattr(handle, name), name
    for name, value in (("PDGN_GAN_HINGE", 1), ("PDGN_GAN_LOGISTIC", 2), ("PDGN_GAN_D_REAL", 0), ("PDGN_GAN_D_FAKE", 1), ("PDGN_GAN_G", 2)):
        assert re.findall(r"^#define\s+%s\s+(\d+)\s*$" % name, code, flags=re.M) == [str(value)], name
    define = re.findall(r"^#define\s+PDGN_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M)
    assert len(define) == 1 and int(define[0]) == _lib.ABI_VERSION == handle.pdgn_abi_version() > 40
    from pdgn_amd import losses
    assert losses._GAN_KINDS == gm.KINDS == {"hinge": 1, "logistic": 2}
    assert losses._GAN_ROLES == gm.ROLES == {"d_real": 0, "d_fake": 1, "g": 2}
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "%d entry points" % len(_lib.SIGNATURES) in readme


# ---------------------------------------------------------------------------- losses.adversarial
def _spy(monkeypatch):
    """losses.mse_const and losses.gan_term replaced by recorders of their (normalised) arguments."""
    from pdgn_amd import losses
    seen = {"mse_const": [], "gan_term": []}

    def mse_const(x, target, scale=1.0, count=None):
        seen["mse_const"].append((x, target, scale, count))
        return "mse"

    def gan_term(x, kind, role, scale=1.0, count=None):
        seen["gan_term"].append((x, kind, role, scale, count))
        return "gan"

    monkeypatch.setattr(losses, "mse_const", mse_const)
    monkeypatch.setattr(losses, "gan_term", gan_term)
    return seen


def test_lsgan_is_the_three_mse_const_calls_and_the_others_are_gan_term(monkeypatch):
    from pdgn_amd import losses
    assert losses.GAN_LOSSES == ("lsgan", "hinge", "logistic")
    seen = _spy(monkeypatch)
    x, slot = object(), object()
    assert losses.adversarial(x, "lsgan", "d_real", slot) == "mse"
    assert losses.adversarial(x, "lsgan", "d_fake") == "mse"
    assert losses.adversarial(x, "lsgan", "g") == "mse"
    assert losses.adversarial(x, "lsgan", "d_real") == "mse"
    assert seen["mse_const"] == [(x, 1.0, 0.5, slot), (x, 0.0, 0.5, None), (x, 1.0, 1.0, None), (x, 1.0, 0.5, None)]
    assert all(type(v) is float for call in seen["mse_const"] for v in call[1:3]) and not seen["gan_term"]
    for objective in ("hinge", "logistic"):
        seen["gan_term"].clear()
        assert losses.adversarial(x, objective, "d_real", slot) == "gan"
        assert losses.adversarial(x, objective, "d_fake") == "gan"
        assert losses.adversarial(x, objective, "g") == "gan"
        assert seen["gan_term"] == [(x, objective, "d_real", 1.0, slot), (x, objective, "d_fake", 1.0, None), (x, objective, "g", 1.0, None)]
    assert len(seen["mse_const"]) == 4


def test_lsgan_without_a_count_fits_a_three_argument_mse_const(monkeypatch):
    """tests/torch_standins.mse_const_torch takes (x, target, scale): the CPU trainer tests route the step through it."""
    import torch
    from pdgn_amd import losses
    from torch_standins import mse_const_torch, patch_losses
    patch_losses(monkeypatch)
    x = torch.tensor([[0.25], [1.5], [-2.0]])
    for role, (target, scale) in (("d_real", (1.0, 0.5)), ("d_fake", (0.0, 0.5)), ("g", (1.0, 1.0))):
        assert torch.equal(losses.adversarial(x, "lsgan", role), mse_const_torch(x, target, scale))


def test_unknown_names_raise_value_error():
    import torch
    from pdgn_amd import losses
    x = torch.zeros(3)
    for call in (lambda: losses.adversarial(x, "wgan", "g"), lambda: losses.adversarial(x, "lsgan", "d"), lambda: losses.adversarial(x, "hinge", "real"),
                 lambda: losses.gan_term(x, "lsgan", "g"), lambda: losses.gan_term(x, "wgan", "g"), lambda: losses.gan_term(x, "hinge", "gen"),
                 lambda: losses.gan_term(x, 1, 0), lambda: losses.decision_boundary("wgan"), lambda: losses.decision_boundary(None)):
        with pytest.raises(ValueError):
            call()


def test_decision_boundaries():
    from pdgn_amd import losses
    assert [losses.decision_boundary(o) for o in losses.GAN_LOSSES] == [0.5, 0.0, 0.0]


# ---------------------------------------------------------------------------- the mirror against its closed forms
def _scores(n=35, seed=0):
    return np.random.default_rng(seed).normal(0.0, 2.0, n).astype(np.float32)


@pytest.mark.parametrize("kind, role", PAIRS)
def test_the_fp32_mirror_agrees_with_the_closed_form(kind, role):
    x = _scores()
    for scale in (1.0, 0.5):
        got, want = gm.term(x, kind, role, scale), gm.term64(x, kind, role, scale)
        assert got.dtype == np.float32 and abs(float(got) - want) <= 1e-6 * max(1.0, abs(want)), (got, want)
        dx, dx64 = gm.term_grad(x, kind, role, scale, 3.0), gm.term_grad64(x, kind, role, scale, 3.0)
        assert dx.dtype == np.float32 and dx.shape == (35,) and np.abs(dx - dx64).max() <= 1e-6 * np.abs(dx64).max()


@pytest.mark.parametrize("kind, role", PAIRS)
def test_the_gradient_summed_is_the_finite_difference_of_the_closed_form(kind, role):
    x = _scores(seed=1)
    assert np.abs(np.abs(x.astype(np.float64)) - 1.0).min() > 1e-2           # no score within the step of a hinge's kink
    h = 1e-3
    xd = x.astype(np.float64)
    fd = (gm.term64(xd + h, kind, role, 0.75) - gm.term64(xd - h, kind, role, 0.75)) / (2 * h)
    for grad in (gm.term_grad(x, kind, role, 0.75, 1.0).astype(np.float64).sum(), gm.term_grad64(x, kind, role, 0.75, 1.0).sum()):
        assert abs(grad - fd) <= 1e-6, (grad, fd)


def test_the_mirror_on_values_computed_by_hand():
    x = np.array([0.5, 1.0, 2.0, -1.0, -3.0], dtype=np.float32)
    assert float(gm.term(x, "hinge", "d_real")) == np.float32(np.float32(0.5 + 0.0 + 0.0 + 2.0 + 4.0) / np.float32(5))
    assert float(gm.term(x, "hinge", "d_fake")) == np.float32(np.float32(1.5 + 2.0 + 3.0 + 0.0 + 0.0) / np.float32(5))
    assert float(gm.term(x, "hinge", "g", 2.0)) == np.float32(2.0) * np.float32(np.float32(0.5) / np.float32(5))
    c = np.float32(1) / np.float32(5)
    assert gm.term_grad(x, "hinge", "d_real").tolist() == [-c, 0.0, 0.0, -c, -c]            # the kink x = 1: 0
    assert gm.term_grad(x, "hinge", "d_fake").tolist() == [c, c, c, 0.0, 0.0]               # the kink x = -1: 0
    assert gm.term_grad(x, "hinge", "g").tolist() == [-c] * 5
    assert abs(float(gm.term(np.zeros(4, np.float32), "logistic", "d_real")) - np.log(2.0)) < 2e-7
    assert gm.term_grad(np.zeros(2, np.float32), "logistic", "d_fake").tolist() == [0.25, 0.25]
    assert gm.term_grad(np.zeros(2, np.float32), "logistic", "g").tolist() == [-0.25, -0.25]
    # NaN in, NaN out -- in every kind and role; the other gradients stay finite
    x[2] = np.nan
    for kind, role in PAIRS:
        assert np.isnan(gm.term(x, kind, role)) and np.isnan(gm.term64(x, kind, role))
        for dx in (gm.term_grad(x, kind, role), gm.term_grad64(x, kind, role)):
            assert np.isnan(dx[2]) and np.isfinite(np.delete(dx, 2)).all()
    # saturation: finite, max(t, 0), the gradient exactly 0 or -+1 (times 1 / n)
    big = np.array([100.0, -100.0, 3e38, -3e38], dtype=np.float32)
    for v in big:
        one = np.array([v], dtype=np.float32)
        for role, t in (("d_fake", float(v)), ("d_real", -float(v)), ("g", -float(v))):
            got = float(gm.term(one, "logistic", role))
            assert np.isfinite(got) and abs(got - max(t, 0.0)) <= 2.0 ** -23 * max(t, 0.0) + 1e-37, (v, role, got)
            assert abs(gm.term64(one, "logistic", role) - max(t, 0.0)) <= 1e-37
            d = float(gm.term_grad(one, "logistic", role)[0])     # (sigma(-100) = 3.7e-44 is an fp32 denormal: 0 only where they are flushed)
            assert d == (1.0 if role == "d_fake" else -1.0) if t > 0 else (abs(d) < 1e-37 and (d == 0.0 or abs(v) == 100.0)), (v, role, d)
    assert gm.counts(np.array([0.25, -0.25, 0.0, -0.0, 0.75, np.nan], dtype=np.float32)) == (2, 1, 6)
    assert gm.counts(np.array([0.25, -0.25, 0.0, -0.0, 0.75, np.nan], dtype=np.float32), 0.5) == (1, 4, 6)
    with pytest.raises(ValueError):
        gm.term(x, "lsgan", "g")


def test_the_mirrors_sum_runs_in_the_kernels_order():
    """1024 threads: element 1024 lands on thread 0 BEFORE the butterfly; with 2^24 on thread 0 a 1 added there first is lost, one added
    by another lane of the wave first is not."""
    f = np.zeros(1025, dtype=np.float32)
    f[0], f[1024] = 2.0 ** 24, 1.0
    assert float(gm.block_sum(f)) == 2.0 ** 24                   # (2^24 + 1) on thread 0 rounds to 2^24
    f[1024], f[1], f[33] = 0.0, 1.0, 1.0
    assert float(gm.block_sum(f)) == 2.0 ** 24 + 2.0             # lanes 1 and 33 meet at offset 32 before they reach lane 0


# ---------------------------------------------------------------------------- the command line
BASE = ["--model_dir", "m"]


def test_the_parser_takes_the_three_names_and_the_default_namespace_has_lsgan(capsys):
    from pdgn_amd import train
    args = train.parse_args(BASE)
    assert args.gan_loss == "lsgan" and "gan_loss" not in vars(args) and "gan_loss" not in str(train.logged_args(args))
    for name in ("lsgan", "hinge", "logistic"):
        got = train.parse_args(BASE + ["--gan_loss", name])
        assert got.gan_loss == name and "gan_loss='%s'" % name in str(train.logged_args(got))
    with pytest.raises(SystemExit):
        train.parse_args(BASE + ["--gan_loss", "wgan"])
    assert "invalid choice" in capsys.readouterr().err
    action = [a for a in train.build_parser()._actions if a.dest == "gan_loss"]
    assert len(action) == 1 and action[0].default is argparse.SUPPRESS and "logit" in action[0].help
    target = [a for a in train.build_parser()._actions if a.dest == "d_augment_target"][0]
    assert "decision boundary" in " ".join(target.help.split()) and "decision boundary" in " ".join(train.__doc__.split())


def test_the_flag_reaches_the_trainer(monkeypatch):
    from pdgn_amd import train, trainer
    got = {}
    monkeypatch.setattr(trainer, "PDGNTrainer", lambda **kw: got.update(kw) or "trainer")
    assert train.make_trainer(train.parse_args(BASE + ["--gan_loss", "hinge"]), "cpu") == "trainer" and got["gan_loss"] == "hinge"
    assert train.make_trainer(train.parse_args(BASE), "cpu") == "trainer" and got["gan_loss"] == "lsgan"


# ---------------------------------------------------------------------------- the trainer
def test_the_trainer_refuses_an_unknown_objective_before_it_builds_anything(monkeypatch):
    from pdgn_amd import trainer

    def never(*a, **k):
        raise AssertionError("a network was built")

    monkeypatch.setattr(trainer, "PointGenerator", never)
    monkeypatch.setattr(trainer, "PointDiscriminator", never)
    for bad in ("wgan", "LSGAN", None, 1):
        with pytest.raises(ValueError):
            trainer.PDGNTrainer(device="cuda:0", distributed=False, gan_loss=bad)


def test_a_cpu_trainer_keeps_the_name():
    from pdgn_amd.generator import PointGenerator
    from pdgn_amd.trainer import PDGNTrainer
    for name in ("lsgan", "hinge", "logistic"):
        tr = PDGNTrainer(device="cpu", distributed=False, base_points=16, generator=PointGenerator(256, 20, base_points=16), gan_loss=name)
        assert tr.gan_loss == name
    assert PDGNTrainer(device="cpu", distributed=False, base_points=16, generator=PointGenerator(256, 20, base_points=16)).gan_loss == "lsgan"
