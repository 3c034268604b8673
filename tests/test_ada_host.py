"""CPU: the adaptive discriminator augmentation's host side -- validation before allocation, the numpy restatement of the rule
(tests/ada_mirror.py) on hand-computed cases, its composition over ranks, the command line's flags, and the header's declarations."""
import argparse

import numpy as np
import pytest

import ada_mirror as ada

ONE = 1 << 24


# ---------------------------------------------------------------------------- validation
@pytest.mark.parametrize("bad", [dict(target=1.0), dict(target=-1.0), dict(target=float("nan")), dict(target="high"), dict(interval=0),
                                 dict(interval=2.5), dict(interval=True), dict(span=0), dict(span=-3), dict(span=1.0e5),
                                 dict(p_min=-0.1), dict(p_max=1.1), dict(p_min=0.6, p_max=0.5), dict(p_min=0.6), dict(p_max=0.4),
                                 dict(rate=0.1), dict(targets=0.6)])
def test_bad_adaptive_arguments_raise_before_anything_is_allocated(bad):
    from pdgn_amd.augment import Augment
    with pytest.raises(ValueError):
        Augment(p=0.5, device="cuda:0", adaptive=bad)            # (no GPU on this box: reaching an allocation would be another error)


def test_adaptive_must_be_a_dict_and_p_must_lie_in_its_range():
    from pdgn_amd import augment
    with pytest.raises(ValueError):
        augment.Augment(p=0.5, device="cuda:0", adaptive=0.6)
    with pytest.raises(ValueError):
        augment.Augment(p=0.9, device="cuda:0", adaptive={})     # the default range is [0, 0.8]
    with pytest.raises(ValueError):
        augment.Augment(p=0.1, device="cuda:0", adaptive=dict(p_min=0.2))
    got = augment.validate_adaptive({}, 0.5)
    assert got == augment.ADA_DEFAULTS == dict(target=0.6, interval=4, span=500_000, p_min=0.0, p_max=0.8)
    assert augment.validate_adaptive(dict(target=-0.25, interval=1, span=1, p_min=0.5, p_max=0.5), 0.5)["target"] == -0.25


def test_the_fresh_state_record_is_the_mirrors_and_decodes():
    from pdgn_amd import augment
    params = augment.validate(**dict(augment.DEFAULTS, p=0.25, trans_max=0.0))
    adaptive = augment.validate_adaptive(dict(target=0.5, interval=3, span=1000, p_min=0.125, p_max=0.75), params["p"])
    words = augment.ada_words(params, adaptive)
    assert augment.component_mask(params) == 0b00111             # flip, rotation, scale; no translation, no jitter
    want = ada.fresh(p=0.25, target=0.5, interval=3, span=1000, p_min=0.125, p_max=0.75, mask=0b00111)
    assert words.dtype == np.uint64 and words.shape == (ada.WORDS,) == (augment.ADA_WORDS,) and np.array_equal(words, want)
    d = augment.decode_ada(words)
    assert (d["p"], d["thr"], d["target"], d["interval"], d["span"], d["p_min"], d["p_max"], d["mask"]) == (0.25, ONE // 4, 0.5, 3, 1000, 0.125, 0.75, 7)
    assert (d["updates"], d["iters"], d["last"], d["pos"], d["neg"], d["n"]) == (0, 0, (0, 0, 0), 0, 0, 0) and d["last_net"] == [(0, 0, 0)] * 4
    assert [getattr(augment, "W_" + n) for n in ("TARGET", "INTERVAL", "SPAN", "THR_MIN", "THR_MAX", "MASK", "THR", "POS", "NEG", "N", "ITERS",
                                                 "UPDATES", "LAST_R", "LAST_POS", "LAST_NEG", "LAST_N", "LAST_NET", "NET")] == \
        [ada.TARGET, ada.INTERVAL, ada.SPAN, ada.THR_MIN, ada.THR_MAX, ada.MASK, ada.THR, ada.POS, ada.NEG, ada.N, ada.ITERS, ada.UPDATES,
         ada.LAST_R, ada.LAST_POS, ada.LAST_NEG, ada.LAST_N, ada.LAST_NET, ada.NET]


# ---------------------------------------------------------------------------- the mirror, on cases computed by hand
def _one_update(state, triples, table=None):
    table = np.zeros(16, dtype=np.uint32) if table is None else table
    return ada.tick(state, table, ada.slots_of(triples), 0)


@pytest.mark.parametrize("n, span, want", [(4, 500_000, 33), (140, 500_000, 1174), (4 * 35 * 4, 500_000, 4697), (4, 1 << 30, 1),
                                           (4, 1, ONE), (140, 64, 9175040)])
def test_step_sizes(n, span, want):
    """step = max(1, n 2^24 / (4 span)): 4 * 2^24 / 2e6 = 33.55.., 140 * 2^24 / 2e6 = 1174.4.., 560 * 2^24 / 2e6 = 4697.6.., the floor of 1,
    one iteration over the whole range at span 1 (n = 4: one cloud, four discriminators), 140 * 2^24 / 256."""
    assert ada.step_size(n, span) == want
    st = ada.fresh(p=0.4, target=0.6, interval=1, span=span, p_min=0.0, p_max=1.0)
    each = (n // 4, 0, n // 4)                                   # every score above the boundary: r = 1 > target
    after, _, slots, clock = _one_update(st, [each] * 4)
    assert int(after[ada.THR]) == min(ONE, int(st[ada.THR]) + want) and clock == 1 and not slots.any()
    assert int(after[ada.UPDATES]) == 1 and after.view(np.float64)[ada.LAST_R] == 1.0
    assert [int(v) for v in after[ada.LAST_POS:ada.LAST_N + 1]] == [n, 0, n]


def test_both_directions_both_clamps_and_equality():
    st = ada.fresh(p=0.5, target=0.5, interval=1, span=2, p_min=0.25, p_max=0.75)       # n = 16: step = 16 * 2^24 / 8 = 2^25: over either clamp
    up = _one_update(st, [(4, 0, 4)] * 4)[0]
    down = _one_update(st, [(0, 4, 4)] * 4)[0]
    assert int(up[ada.THR]) == 3 * ONE // 4 and int(down[ada.THR]) == ONE // 4
    st = ada.fresh(p=0.5, target=0.5, interval=1, span=1 << 20, p_min=0.25, p_max=0.75)   # step = 16 * 2^24 / 2^22 = 64
    assert int(_one_update(st, [(4, 0, 4)] * 4)[0][ada.THR]) == ONE // 2 + 64
    assert int(_one_update(st, [(0, 4, 4)] * 4)[0][ada.THR]) == ONE // 2 - 64
    # r == target exactly: pos - neg = n / 2 (12 above, 4 below of 16; and with scores ON the boundary: 8 above, none below)
    for triples in ([(3, 1, 4)] * 4, [(2, 0, 4)] * 4):
        same = _one_update(st, triples)[0]
        assert int(same[ada.THR]) == ONE // 2 and int(same[ada.UPDATES]) == 1 and same.view(np.float64)[ada.LAST_R] == 0.5
    # a NaN batch: n counts, pos and neg do not -> r = 0 < target
    assert int(_one_update(st, [(0, 0, 4)] * 4)[0][ada.THR]) == ONE // 2 - 64


def test_the_mask_keeps_a_zero_range_component_at_zero():
    from pdgn_amd import augment
    params = augment.validate(**dict(augment.DEFAULTS, p=0.5, trans_max=0.0))
    table = augment.table_words(params)
    st = augment.ada_words(params, augment.validate_adaptive(dict(interval=1, span=1 << 20), 0.5))
    after, tab, _, _ = _one_update(st, [(4, 0, 4)] * 4, table)
    thr = ONE // 2 + 64
    assert [int(v) for v in tab[:5]] == [thr, thr, thr, 0, 0] and int(after[ada.THR]) == thr
    assert np.array_equal(tab[5:], table[5:])


def test_an_empty_iteration_neither_counts_nor_updates():
    st = ada.fresh(p=0.5, target=0.6, interval=2, span=1 << 20, p_min=0.0, p_max=1.0)
    table = np.zeros(16, dtype=np.uint32)
    one, _, _, c1 = ada.tick(st, table, ada.slots_of([(4, 0, 4)] * 4), 10)
    assert (int(one[ada.ITERS]), int(one[ada.N]), int(one[ada.UPDATES]), c1) == (1, 16, 0, 11)
    idle, _, _, c2 = ada.tick(one, table, np.zeros(16, dtype=np.int32), c1)
    assert np.array_equal(idle, one) and c2 == 12               # the clock ticks, the interval does not
    two = ada.tick(idle, table, ada.slots_of([(1, 3, 4), (4, 0, 4), (0, 0, 4), (2, 2, 4)]), c2)[0]
    assert (int(two[ada.ITERS]), int(two[ada.N]), int(two[ada.UPDATES])) == (0, 0, 1)
    assert [int(v) for v in two[ada.LAST_POS:ada.LAST_N + 1]] == [23, 5, 32]
    assert [int(v) for v in two[ada.LAST_NET:ada.LAST_NET + 12]] == [5, 3, 8, 8, 0, 8, 4, 0, 8, 6, 2, 8]
    assert not two[ada.NET:ada.NET + 12].any()
    assert two.view(np.float64)[ada.LAST_R] == 18 / 32 and int(two[ada.THR]) == ONE // 2 - 128       # r = 0.5625 < 0.6; 32 * 2^24 / 2^22
    assert ada.update(idle, ada.slots_of([(1, 3, 4), (4, 0, 4), (0, 0, 4), (2, 2, 4)])).tobytes() == two.tobytes()


def test_counts_leave_out_the_boundary_and_nan():
    h = np.float32(0.5)
    x = np.array([h, np.nextafter(h, np.float32(1)), np.nextafter(h, np.float32(0)), np.inf, -np.inf, np.nan, 1.0, 0.0, 0.5], dtype=np.float32)
    assert ada.counts(x) == (3, 3, 9)


# ---------------------------------------------------------------------------- composition over ranks
@pytest.mark.parametrize("B", [3, 35])
def test_two_ranks_summed_are_one_rank_at_twice_the_batch(B):
    rng = np.random.default_rng(B)
    scores = [rng.normal(0.6, 0.3, 2 * B).astype(np.float32) for _ in range(4)]
    for s in scores:
        s[0] = 0.5                                               # one score on the boundary in every network
    st = ada.fresh(p=0.3, target=0.6, interval=1, span=5000)
    whole = ada.slots_of([ada.counts(s) for s in scores])
    halves = [ada.slots_of([ada.counts(s[r * B:(r + 1) * B]) for s in scores]) for r in range(2)]
    assert np.array_equal(halves[0] + halves[1], whole)          # what the SUM all-reduce hands every rank
    want = ada.update(st, whole)
    got = ada.update(st, halves[0] + halves[1])
    assert got.tobytes() == want.tobytes() and int(want[ada.UPDATES]) == 1 and int(want[ada.LAST_N]) == 8 * B
    assert abs(int(want[ada.THR]) - int(st[ada.THR])) == ada.step_size(8 * B, 5000)
    alone = ada.update(st, halves[0])                            # and a rank on its own would have taken half the step
    assert ada.step_size(4 * B, 5000) == abs(int(alone[ada.THR]) - int(st[ada.THR])) or int(alone[ada.THR]) == int(st[ada.THR])


# ---------------------------------------------------------------------------- the command line
BASE = ["--model_dir", "m"]


def test_d_augment_target_needs_d_augment(capsys):
    from pdgn_amd import train
    with pytest.raises(SystemExit):
        train.parse_args(BASE + ["--d_augment_target", "0.6"])
    assert "needs --d_augment" in capsys.readouterr().err


@pytest.mark.parametrize("flag", [["--ada_interval", "2"], ["--ada_span", "64"], ["--ada_p_min", "0.1"], ["--ada_p_max", "0.5"]])
def test_every_ada_flag_needs_d_augment_target(flag, capsys):
    from pdgn_amd import train
    with pytest.raises(SystemExit):
        train.parse_args(BASE + ["--d_augment", "0.2"] + flag)
    assert "needs --d_augment_target" in capsys.readouterr().err
    assert train.parse_args(BASE + ["--d_augment", "0.2", "--d_augment_target", "0.6"] + flag).d_augment_target == 0.6


def test_no_flag_leaves_the_namespace_as_it_was_and_the_flags_reach_the_trainer():
    from pdgn_amd import augment, train
    args = train.parse_args(BASE)
    assert not [k for k in vars(args) if k.startswith("ada_") or k.startswith("d_augment")]
    assert "ada_" not in str(train.logged_args(args)) and "d_augment" not in str(train.logged_args(args))
    assert args.d_augment_target is None and train.adaptive_kwargs(args) is None
    fixed = train.parse_args(BASE + ["--d_augment", "0.5"])
    assert not [k for k in vars(fixed) if k.startswith("ada_") or k == "d_augment_target"]
    assert train._augment_arg(fixed) == dict(augment.DEFAULTS, p=0.5, seed=9999)       # no "adaptive" key: today's object
    new = ("d_augment_target", "ada_interval", "ada_span", "ada_p_min", "ada_p_max")
    assert all(a.default is argparse.SUPPRESS for a in train.build_parser()._actions if a.dest in new)
    assert sorted(a.dest for a in train.build_parser()._actions if a.dest in new) == sorted(new)
    args = train.parse_args(BASE + ["--d_augment", "0.2", "--d_augment_target", "0.6", "--ada_span", "64"])
    assert train.adaptive_kwargs(args) == dict(augment.ADA_DEFAULTS, target=0.6, span=64)
    assert train._augment_arg(args)["adaptive"] == dict(target=0.6, interval=4, span=64, p_min=0.0, p_max=0.8)
    assert "d_augment_target=0.6" in str(train.logged_args(args)) and "ada_span=64" in str(train.logged_args(args))
    for bad in (["--d_augment_target", "1.0"], ["--d_augment_target", "0.6", "--ada_interval", "0"], ["--d_augment_target", "0.6", "--ada_p_max", "0.1"],
                ["--d_augment_target", "0.6", "--ada_span", "0"]):
        with pytest.raises(SystemExit):
            train.parse_args(BASE + ["--d_augment", "0.2"] + bad)


# ---------------------------------------------------------------------------- the header
def test_the_header_declares_both_entry_points_and_the_loader_derives_them():
    import ctypes
    from pdgn_amd import _lib
    assert _lib.ABI_VERSION >= 35
    vp, ll, f = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float
    assert _lib.SIGNATURES["pdgn_mse_const_count"] == (ctypes.c_int, (ll, vp, f, f, f, vp, vp, vp))
    assert _lib.SIGNATURES["pdgn_augment_tick_ada"] == (ctypes.c_int, (vp, vp, vp, vp, ll, ll, ll, ll, vp))
    assert _lib.SIGNATURES["pdgn_augment_tick"] == (ctypes.c_int, (vp, vp))             # the plain tick is what it was
    text = open(_lib.HEADER).read()
    assert "typedef struct pdgn_ada_state" in text and "#define PDGN_ADA_STATE_WORDS 40" in text
