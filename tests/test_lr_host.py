"""Learning-rate schedules, the part that needs no GPU: the header's constants and entry points, the host
evaluation against the mirror (tests/lr_mirror.py) bit for bit, the named kinds' knots, validation and the command line."""
import math
import os
import re

import numpy as np
import pytest

import lr_mirror as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.float64(x).view(np.uint64)


# ---------------------------------------------------------------------------- header and mirror
def test_header_defines_the_table_and_exports_the_entry_points():
    from pdgn_amd import _lib, schedule
    text = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    assert re.search(r"^#define PDGN_LR_MAX_KNOTS 16$", text, flags=re.M)
    assert re.search(r"^#define PDGN_LR_TABLE_DOUBLES 33$", text, flags=re.M)
    assert (schedule.MAX_KNOTS, schedule.TABLE_DOUBLES) == (16, 33) == (lm.MAX_KNOTS, lm.TABLE_DOUBLES)
    assert _lib.ABI_VERSION >= 32
    import ctypes
    ret, args = _lib.SIGNATURES["pdgn_adam_sched_multi"]
    assert ret is ctypes.c_int and len(args) == 16 and args[7:12] == (ctypes.c_double,) * 5 and args[-2] is ctypes.c_void_p
    ret, args = _lib.SIGNATURES["pdgn_lr_eval"]
    assert ret is ctypes.c_int and args == (ctypes.c_void_p, ctypes.c_double) + (ctypes.c_void_p,) * 5


KNOT_LISTS = [
    [(0, 1)],
    [(5, 0.25)],
    [(0, 0), (10, 1)],
    [(0.5, 0.1), (10, 1.0), (1000, 0.3), (1001, 0.03)],
    [(3, 0.7), (7, 1e-3), (11, 3.0), (5000.5, 0.0)],
    [(i * i + 1, 1.0 / (i + 1)) for i in range(16)],
]


@pytest.mark.parametrize("knots", KNOT_LISTS, ids=[str(len(k)) + "knots" + str(i) for i, k in enumerate(KNOT_LISTS)])
def test_host_evaluation_equals_the_mirror_bit_for_bit(knots):
    from pdgn_amd import schedule
    tab = lm.table(knots)
    assert np.array_equal(np.array(schedule.words(knots)), tab)
    ts = [t for t, _ in knots]
    grid = [0.0, ts[0] / 2, ts[0] - 1e-9 if ts[0] > 0 else 0.0]                   # before the first knot
    grid += ts                                                                    # on every knot
    for a, b in zip(ts, ts[1:]):                                                  # inside every segment
        grid += [a + (b - a) * w for w in (1e-9, 1 / 3, 0.5, 0.7, 1 - 1e-9)] + [math.floor(a) + 1.0]
    grid += [ts[-1] + 1e-9, ts[-1] + 1, 2.0 ** 24 - 1, 1e30]                      # past the last
    inside = 0
    for t in grid:
        want, got = lm.factor(tab, t), schedule.factor(knots, t)
        assert _bits(want) == _bits(got), (t, want, got)
        assert _bits(schedule.factor(tab, t)) == _bits(got)                       # a table is read like its knots
        assert _bits(schedule.lr_eff(1e-4, knots, t)) == _bits(lm.lr_eff(1e-4, tab, t))
        inside += ts[0] < t < ts[-1]
    assert inside >= 5 * (len(knots) - 1)
    for t, f in knots:                                                            # exactly f_i on a knot
        assert _bits(schedule.factor(knots, t)) == _bits(float(f))
    assert schedule.factor(knots, 0.0) == knots[0][1] == schedule.factor(knots, ts[0])
    assert schedule.factor(knots, 1e9) == knots[-1][1]


def test_a_malformed_table_gives_the_first_factor_in_both():
    from pdgn_amd import schedule
    good = lm.table([(2, 0.5), (10, 1.0), (20, 0.0)])
    for change in ({0: 40.0}, {0: 0.0}, {0: 2.5}, {0: float("nan")}, {3: 1.0}, {5: 10.0}, {3: float("nan")}):
        tab = good.copy()
        for k, v in change.items():
            tab[k] = v
        for t in (0, 5, 15, 100):
            assert lm.factor(tab, t) == 0.5 == schedule.factor(tab, t), (change, t)
    assert schedule.factor(good, 15) == 0.5 == lm.factor(good, 15)


# ---------------------------------------------------------------------------- the named kinds
def test_constant_linear_and_warm_up_knots():
    from pdgn_amd.schedule import factor, knots
    assert knots("constant", 1000) == [(0.0, 1.0)]
    assert knots("constant", 1000, warmup_iters=8) == [(0.0, 0.0), (8.0, 1.0)]
    assert knots("linear", 1000, final_factor=0.25) == [(0.0, 1.0), (1000.0, 0.25)]
    ks = knots("linear", 1032, warmup_iters=8, final_factor=0.5)
    assert ks == [(0.0, 0.0), (8.0, 1.0), (1032.0, 0.5)]
    assert [factor(ks, t) for t in (0, 2, 8, 520, 1032, 5000)] == [0.0, 0.25, 1.0, 0.75, 0.5, 0.5]     # (powers of two: exact)
    with pytest.raises(ValueError):
        knots("linear", 100, warmup_iters=100)
    with pytest.raises(ValueError):
        knots("exponential", 100)


@pytest.mark.parametrize("warm,final", [(0, 0.0), (0, 0.25), (100, 0.0), (64, 0.5)])
def test_cosine_knots_and_the_stated_interpolation_bound(warm, final):
    from pdgn_amd.schedule import factor, knots
    left = 15 if warm else 16
    T = warm + 3000 * (left - 1)                                                  # every knot on a whole update
    ks = knots("cosine", T, warmup_iters=warm, final_factor=final)
    assert len(ks) == 16
    cos = ks[1:] if warm else ks
    assert ks[0] == ((0.0, 0.0) if warm else (0.0, 1.0)) and cos[0] == (float(warm), 1.0) and cos[-1] == (float(T), final)
    assert [t for t, _ in cos] == [warm + 3000.0 * j for j in range(left)]
    for j, (_, f) in enumerate(cos):
        assert abs(f - (final + (1 - final) * (1 + math.cos(math.pi * j / (left - 1))) / 2)) <= 1e-15
    assert all(a[1] > b[1] for a, b in zip(cos, cos[1:]))
    # the chord against the cosine on 1000 points: at most h^2 / 16 of the range, h the knot spacing in u * pi (the docstring's bound)
    h = math.pi / (left - 1)
    bound = h * h / 16 * (1 - final)
    worst = 0.0
    for k in range(1000):
        t = warm + (T - warm) * (k + 0.5) / 1000
        true = final + (1 - final) * (1 + math.cos(math.pi * (t - warm) / (T - warm))) / 2
        worst = max(worst, abs(factor(ks, t) - true))
    print("cosine warm %d final %g: worst chord error %.3e, bound %.3e" % (warm, final, worst, bound))
    assert worst <= bound * (1 + 1e-9) and worst > bound / 4                      # (the bound is not idle: the mid-slope chords come near it)


def test_step_knots_and_too_many_drops():
    from pdgn_amd.schedule import factor, knots
    ks = knots("step", 100, step_iters=30, gamma=0.5)
    assert ks == [(0.0, 1.0), (30.0, 1.0), (31.0, 0.5), (60.0, 0.5), (61.0, 0.25), (90.0, 0.25), (91.0, 0.125)]
    # torch's StepLR: update t (1-based) runs at gamma ** ((t - 1) // step)
    assert all(factor(ks, t) == 0.5 ** ((t - 1) // 30) for t in range(1, 101))
    assert knots("step", 90, step_iters=30, gamma=0.5)[-1] == (61.0, 0.25)        # no drop at the very end
    ks = knots("step", 800, warmup_iters=4, step_iters=100, gamma=0.5)            # seven drops behind a warm-up: all 16 knots
    assert len(ks) == 16 and ks[:3] == [(0.0, 0.0), (4.0, 1.0), (100.0, 1.0)] and ks[-1] == (701.0, 0.5 ** 7)
    with pytest.raises(ValueError):
        knots("step", 801, warmup_iters=4, step_iters=100, gamma=0.5)             # an eighth
    with pytest.raises(ValueError):
        knots("step", 1000, step_iters=100)                                       # nine, no warm-up
    with pytest.raises(ValueError):
        knots("step", 1000)                                                       # no period
    with pytest.raises(ValueError):
        knots("step", 1000, warmup_iters=500, step_iters=400)                     # the first drop inside the warm-up


# ---------------------------------------------------------------------------- validate
@pytest.mark.parametrize("bad", [
    [],
    [(i, 1.0) for i in range(17)],
    [(0, 1), (5, 1), (5, 0.5)],
    [(0, 1), (5, 1), (4, 0.5)],
    [(0, -0.1)],
    [(0, float("nan"))],
    [(0, float("inf"))],
    [(-1, 1.0)],
    [(float("nan"), 1.0)],
    [(0, 1), (float("inf"), 0.5)],
    [1.0, 2.0],
], ids=["n0", "n17", "equal_t", "decreasing_t", "negative_f", "nan_f", "inf_f", "negative_t", "nan_t", "inf_t", "no_pairs"])
def test_validate_raises(bad):
    from pdgn_amd import schedule
    with pytest.raises(ValueError):
        schedule.validate(bad)
    with pytest.raises(ValueError):
        schedule.table(bad)
    with pytest.raises(ValueError):
        schedule.factor(bad, 1)


def test_validate_accepts_and_table_lays_the_words_out():
    from pdgn_amd import schedule
    ks = [(i, 16.0 - i) for i in range(16)]
    assert schedule.validate(ks) == [(float(t), float(f)) for t, f in ks]
    tab = schedule.table([(1, 0.5), (9, 2)])
    assert tab.dtype.is_floating_point and tab.element_size() == 8 and tab.shape == (33,)
    assert tab.tolist() == [2.0, 1.0, 0.5, 9.0, 2.0] + [0.0] * 28


def test_a_trainer_refuses_a_bad_schedule_and_bad_rates_before_it_builds_anything():
    from pdgn_amd.trainer import PDGNTrainer
    for kw in ({"lr_schedule": []}, {"lr_schedule": [(0, 1), (0, 2)]}, {"lr_g": -1.0}, {"lr_d": float("nan")}):
        with pytest.raises(ValueError):
            PDGNTrainer(device="cpu", distributed=False, **kw)


# ---------------------------------------------------------------------------- the command line
BASE = ["--model_dir", "m"]


def test_flags_are_absent_unless_given():
    from pdgn_amd import train
    args = train.parse_args(BASE)
    names = ("lr_g", "lr_d", "lr_schedule", "lr_warmup_iters", "lr_final_factor", "lr_step_epochs", "lr_gamma")
    for holder in (vars(args), vars(train.logged_args(args))):
        assert not any(n in holder for n in names)
    assert "lr_" not in str(train.logged_args(args)).replace("learning_rate", "")
    assert (args.lr_g, args.lr_d, args.lr_schedule, args.lr_warmup_iters, args.lr_final_factor, args.lr_step_epochs, args.lr_gamma) == (
        None, None, None, 0, 0.0, None, 0.1)
    assert train.schedule_knots(args, 10) is None
    args = train.parse_args(BASE + ["--lr_g", "5e-5", "--lr_schedule", "cosine", "--lr_warmup_iters", "100"])
    assert vars(args)["lr_g"] == 5e-5 and "lr_d" not in vars(args) and "lr_schedule='cosine'" in str(train.logged_args(args))
    ks = train.schedule_knots(args, 10)
    assert ks[:2] == [(0.0, 0.0), (100.0, 1.0)] and ks[-1] == (3000.0, 0.0) and len(ks) == 16
    args = train.parse_args(BASE + ["--lr_schedule", "step", "--lr_step_epochs", "100", "--lr_gamma", "0.5", "--max_epoch", "300"])
    assert train.schedule_knots(args, 7) == [(0.0, 1.0), (700.0, 1.0), (701.0, 0.5), (1400.0, 0.5), (1401.0, 0.25)]
    args = train.parse_args(BASE + ["--lr_schedule", "linear", "--lr_final_factor", "0.1", "--max_epoch", "4"])
    assert train.schedule_knots(args, 25) == [(0.0, 1.0), (100.0, 0.1)]


@pytest.mark.parametrize("extra", [
    ["--lr_warmup_iters", "10"],
    ["--lr_final_factor", "0.1"],
    ["--lr_step_epochs", "10"],
    ["--lr_gamma", "0.5"],
    ["--lr_schedule", "step"],
    ["--lr_schedule", "step", "--lr_step_epochs", "0"],
    ["--lr_schedule", "step", "--lr_step_epochs", "10", "--lr_gamma", "0"],
    ["--lr_schedule", "step", "--lr_step_epochs", "10", "--max_epoch", "300"],
    ["--lr_schedule", "step", "--lr_step_epochs", "10", "--lr_final_factor", "0.1"],
    ["--lr_schedule", "cosine", "--lr_step_epochs", "10"],
    ["--lr_schedule", "linear", "--lr_gamma", "0.5"],
    ["--lr_schedule", "constant", "--lr_final_factor", "0.5"],
    ["--lr_schedule", "cosine", "--lr_warmup_iters", "-1"],
    ["--lr_schedule", "cosine", "--lr_final_factor", "-0.5"],
    ["--lr_schedule", "exponential"],
    ["--lr_g", "-1e-4"],
    ["--lr_d", "nan"],
], ids=lambda e: "_".join(x.lstrip("-") for x in e))
def test_bad_combinations_exit_with_an_error(extra, capsys):
    from pdgn_amd import train
    with pytest.raises(SystemExit) as e:
        train.parse_args(BASE + extra)
    assert e.value.code == 2 and "error" in capsys.readouterr().err
