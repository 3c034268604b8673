"""CPU: the averaged generator's host side -- the mirror of its recurrence, the decay's warm-up schedule, the command line, the
header's declarations, and what a trainer on the CPU device can do with it (buffer, by-value swap, checkpoint files; the updates
themselves are HIP kernels and have no CPU form)."""
import os
import re

import numpy as np
import pytest
import torch

import ema_mirror as em
from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_values():
    assert em.decay_at(0.999, 1) == 2.0 / 11.0
    assert em.decay_at(0.999, 10) == 11.0 / 20.0
    assert em.decay_at(0.999, 1000) == 1001.0 / 1010.0
    assert em.decay_at(0.9999, 1000) == 1001.0 / 1010.0
    # crossover: (1 + t) / (10 + t) reaches 0.999 at t = 8990
    assert em.decay_at(0.999, 8989) == 8990.0 / 8999.0 < 0.999
    assert em.decay_at(0.999, 8991) == 0.999 and em.decay_at(0.999, 10 ** 6) == 0.999
    assert abs(float(em.decay_at(0.999, 8990)) - 0.999) < 1e-15
    assert em.decay_at(0.5, 8) == 0.5 and em.decay_at(0.5, 7) == 8.0 / 17.0     # a small decay crosses early: 9 / 18 = 0.5 at t = 8
    omd = em.one_minus_decay(0.999, 1)
    assert omd.dtype == np.float32 and omd == np.float32(1.0 - 2.0 / 11.0)
    assert em.one_minus_decay(0.999, 5000) == np.float32(1.0 - 5001.0 / 5010.0)
    assert em.one_minus_decay(0.999, 20000) == np.float32(1.0 - 0.999)


def test_mirror_rounds_three_times_in_float32():
    rng = np.random.default_rng(0)
    e = rng.standard_normal(4097).astype(np.float32)
    p = (e + rng.standard_normal(4097).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    got = em.ema_update(e, p, 0.999, 7)
    omd = np.float32(1.0 - 8.0 / 17.0)
    want = np.array([np.float32(np.float32(a) + np.float32(omd * np.float32(np.float32(b) - np.float32(a)))) for a, b in zip(e, p)], dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # not the fused form: in float64 with one rounding a visible share of the elements comes out differently
    fused = (e.astype(np.float64) + np.float64(omd) * (p.astype(np.float64) - e.astype(np.float64))).astype(np.float32)
    assert (fused != got).any()
    # the recurrence: t advances by one per snapshot; an average that equals the parameters stays there
    assert np.array_equal(em.ema_run(e, [p, p], 0.999, 7), em.ema_update(em.ema_update(e, p, 0.999, 7), p, 0.999, 8))
    assert np.array_equal(em.ema_update(p, p, 0.999, 3), p)


def test_header_declares_both_entry_points():
    names = declared_symbols()
    assert "pdgn_adam_ema_multi" in names and "pdgn_ema_multi" in names and "pdgn_adam_multi" in names
    text = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    for name in ("pdgn_adam_ema_multi", "pdgn_ema_multi"):
        head = text[:text.index("int " + name + "(")]
        comment = re.sub(r"\s*\n \*\s*", " ", head[head.rindex("/*"):])       # (the comment's line breaks are not the point)
        assert "No reference counterpart" in comment and "State touched" in comment and "llocates nothing" in comment, name


def test_command_line_reaches_the_trainer():
    from pdgn_amd import train
    base = ["--model_dir", "m", "--num_point", "256"]
    assert train.parse_args(base).ema_decay == 0.0
    args = train.parse_args(base + ["--ema_decay", "0.999"])
    assert args.ema_decay == 0.999
    for bad in ("1.0", "-0.1", "1.5"):
        with pytest.raises(SystemExit):
            train.parse_args(base + ["--ema_decay", bad])
    torch.manual_seed(0)
    tr = train.make_trainer(args, "cpu")
    assert tr.ema_decay == 0.999 and tr.ema is not None and len(tr.ema) == len(list(tr.G.parameters()))
    assert all(torch.equal(e, p) and e.data_ptr() % 16 == 0 for e, p in zip(tr.ema, tr.G.parameters()))
    assert tr._stepG.ema is not None and all(s.ema is None for s in tr._stepD)          # the discriminators get no average
    args.phase = "test"                                                                  # the test phase evaluates the file it is given
    assert train.make_trainer(args, "cpu").ema is None
    # with the switch off the first line of the log is what it was before the flag existed
    assert "ema" not in str(train.logged_args(train.parse_args(base)))
    assert "ema_decay=0.999" in str(train.logged_args(train.parse_args(base + ["--ema_decay", "0.999"])))


@pytest.fixture()
def no_flush(monkeypatch):
    from pdgn_amd import fused
    import pdgn_amd.trainer as T
    monkeypatch.setattr(fused, "flush_bn_counters", lambda: None)
    monkeypatch.setattr(T, "flush_bn_counters", lambda: None)


def _small(ema_decay, seed=0):
    from pdgn_amd.generator import PointGenerator
    from pdgn_amd.trainer import PDGNTrainer
    torch.manual_seed(seed)
    return PDGNTrainer(device="cpu", distributed=False, base_points=16, generator=PointGenerator(256, 20, base_points=16), ema_decay=ema_decay)


def test_off_is_off_on_the_host(no_flush, tmp_path):
    from pdgn_amd.trainer import PDGNTrainer
    tr = _small(0.0)
    assert tr.ema is None and tr.ema_buf is None and tr._stepG.ema is None
    with pytest.raises(RuntimeError):
        with tr.averaged_generator():
            pass
    assert len(tr.save(str(tmp_path), 1, "chair")) == 2
    assert sorted(os.listdir(tmp_path)) == ["1_chair_D.pth", "1_chair_G.pth"]
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError):
            PDGNTrainer(device="cpu", distributed=False, ema_decay=bad)


def test_checkpoint_files_swap_and_resume_on_the_host(no_flush, tmp_path):
    from pdgn_amd._lib import PdgnHipError
    tr = _small(0.999)
    params = list(tr.G.parameters())
    with torch.no_grad():
        for i, e in enumerate(tr.ema):
            e.add_(0.01 * (1 + i % 3))                                           # averages that differ from the parameters
    for p in params:
        p.grad = torch.full_like(p, 1e-3)
    tr.optG.step()
    live = [p.detach().clone() for p in params]
    avg = [e.clone() for e in tr.ema]
    # the files
    paths = tr.save(str(tmp_path), 4, "chair")
    assert [os.path.basename(p) for p in paths] == ["4_chair_G.pth", "4_chair_D.pth", "4_chair_G_ema.pth"]
    g, ge = torch.load(paths[0]), torch.load(paths[2])
    assert set(ge) == set(g) | {"ema_decay"} and ge["ema_decay"] == 0.999 and ge["G_epoch"] == 4
    assert list(ge["G_model"]) == list(g["G_model"])
    names = {"module." + n for n, _ in tr.G.named_parameters()}
    for (k, a), (_, b) in zip(ge["G_model"].items(), g["G_model"].items()):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a, b) != (k in names), k                              # averaged parameters, live buffers
    for (n, _), e in zip(tr.G.named_parameters(), avg):
        assert torch.equal(ge["G_model"]["module." + n], e)
    assert str(ge["G_optimizer"]) == str(g["G_optimizer"])
    # the swap is by value and is undone
    ptrs, versions = [p.data_ptr() for p in params], [p._version for p in params]
    with tr.averaged_generator() as G:
        assert G is tr.G and all(torch.equal(p, e) for p, e in zip(params, avg))
        assert [p.data_ptr() for p in params] == ptrs and all(p._version > v for p, v in zip(params, versions))
    assert all(torch.equal(p, l) for p, l in zip(params, live)) and all(torch.equal(e, a) for e, a in zip(tr.ema, avg))
    assert [p.data_ptr() for p in params] == ptrs
    with pytest.raises(KeyError):                                                # ... also when the body raises
        with tr.averaged_generator():
            raise KeyError("x")
    assert all(torch.equal(p, l) for p, l in zip(params, live))
    # resume: from the sibling file; without it, from the loaded parameters
    other = _small(0.999, seed=1)
    assert other.load(paths[0], paths[1]) == 4
    assert all(torch.equal(a, b) for a, b in zip(other.ema, avg)) and all(torch.equal(a, b) for a, b in zip(other.G.parameters(), live))
    os.remove(paths[2])
    assert other.load(paths[0], paths[1]) == 4
    assert all(torch.equal(a, b) for a, b in zip(other.ema, live))
    # the update itself is a HIP kernel: on the CPU device it raises instead of quietly doing something else
    with pytest.raises(PdgnHipError):
        tr._stepG.step()
