"""CPU: the discriminator augmentation's host side -- argument validation (pdgn_amd.augment), properties of the numpy mirror of
its draws (tests/augment_mirror.py), the table's encoding, and the command line's flags."""
import numpy as np
import pytest

import augment_mirror as am


# ---------------------------------------------------------------------------- validation
@pytest.mark.parametrize("bad", [
    dict(p=-0.1), dict(p=1.5), dict(p=float("nan")), dict(p="half"),
    dict(scale_max=0.9), dict(scale_max=float("inf")),
    dict(rot_max_deg=-1.0), dict(rot_max_deg=float("nan")), dict(rot_max_deg=181.0),
    dict(trans_max=-0.1), dict(trans_max=float("inf")),
    dict(jitter_sigma=-1e-3), dict(jitter_sigma=float("nan")),
    dict(up_axis=3), dict(up_axis=-1), dict(up_axis=1.0), dict(flip_axis=3),
    dict(up_axis=1, flip_axis=1, flip=True),                     # the mirror through the up axis
    dict(seed=-1), dict(seed=1 << 64), dict(rank=-1),
])
def test_bad_arguments_raise_before_anything_is_allocated(bad):
    from pdgn_amd.augment import Augment
    with pytest.raises(ValueError):
        Augment(device="cuda:0", **bad)                          # (no GPU on this box: reaching an allocation would be another error)


def test_equal_axes_are_fine_without_a_flip():
    from pdgn_amd import augment
    assert augment.validate(**dict(augment.DEFAULTS, flip=False, flip_axis=1, up_axis=1))["flip"] is False


def test_thresholds_are_exact_at_zero_and_one_and_the_table_round_trips():
    from pdgn_amd import augment
    assert augment.threshold(0.0) == 0 and augment.threshold(1.0) == 1 << 24 and augment.threshold(0.5) == 1 << 23
    params = augment.validate(p=1.0, rot_max_deg=90.0, scale_max=2.0, flip=True, trans_max=0.25, jitter_sigma=0.01, up_axis=2, flip_axis=0)
    got = augment.decode_table(augment.table_words(params))
    want = am.table(p=1.0, rot_max_deg=90.0, scale_max=2.0, flip=True, trans_max=0.25, jitter_sigma=0.01, up_axis=2, flip_axis=0)
    assert got == want
    # a component whose range is zero is switched off in the table, whatever p says
    zero = augment.decode_table(augment.table_words(augment.validate(p=1.0, rot_max_deg=0.0, scale_max=1.0, flip=False, trans_max=0.0,
                                                                     jitter_sigma=0.0, up_axis=1, flip_axis=0)))
    assert [zero[k] for k in ("thr_flip", "thr_rot", "thr_scale", "thr_trans", "thr_jitter")] == [0] * 5


# ---------------------------------------------------------------------------- the mirror
ROWS = np.arange(64)


def test_p_zero_is_the_identity_exactly():
    tab = am.table(p=0.0, jitter_sigma=0.05)
    for dtype in (np.float64, np.float32):
        aff = am.affine(tab, 7, 3, ROWS, am.tag(2, "fake"), dtype)
        assert np.array_equal(aff[:, :9], np.tile(np.eye(3).reshape(-1), (64, 1))) and np.array_equal(aff[:, 9:], np.zeros((64, 3)))
    assert not am.decisions(tab, 7, 3, ROWS, am.tag(2, "fake")).any()
    assert np.array_equal(am.jitter(tab, 7, 3, ROWS, am.tag(2, "fake"), 16), np.zeros((64, 16, 3)))


def test_p_one_enables_everything():
    assert am.decisions(am.table(p=1.0, jitter_sigma=0.05), 7, 3, ROWS, am.tag(0, "real")).all()


def test_flip_alone_is_an_exact_reflection():
    tab = am.table(p=1.0, rot_max_deg=0.0, scale_max=1.0, flip=True, trans_max=0.0)
    aff = am.affine(tab, 11, 5, ROWS, am.tag(1, "gen"), np.float32)
    for a in aff[:, :9].reshape(-1, 3, 3):
        assert np.linalg.det(a.astype(np.float64)) == -1.0
        assert np.array_equal(a @ a.T, np.eye(3, dtype=np.float32))
    assert np.array_equal(aff[:, 9:], np.zeros((64, 3), dtype=np.float32))


@pytest.mark.parametrize("up_axis,flip_axis", [(1, 0), (2, 0), (0, 2), (1, 2)])
def test_the_matrix_over_its_scale_is_orthogonal(up_axis, flip_axis):
    tab = am.table(p=1.0, up_axis=up_axis, flip_axis=flip_axis)
    d = am.words(3, 9, ROWS, am.tag(3, "real"), am.GROUP_SHAPE)
    s = np.exp(tab["log_scale_max"] * am.unit(d[:, 2]))
    assert (s >= 1 / 1.25 - 1e-7).all() and (s <= 1.25 + 1e-7).all()
    a = am.affine(tab, 3, 9, ROWS, am.tag(3, "real"))[:, :9].reshape(-1, 3, 3) / s[:, None, None]
    err = np.abs(a @ a.transpose(0, 2, 1) - np.eye(3)).max()
    assert err <= 8 * np.finfo(np.float64).eps, err                                # products and sums of three terms of size <= 1
    assert np.allclose(np.linalg.det(a), -1.0, atol=1e-14)                        # flipped (p = 1): improper
    # the up axis is fixed, the translation within its range
    assert np.array_equal(a[:, up_axis, up_axis], np.ones(64))
    t = am.affine(tab, 3, 9, ROWS, am.tag(3, "real"))[:, 9:]
    assert (np.abs(t) <= tab["trans_max"]).all() and (t != 0).any()


def test_enable_decisions_at_one_half_are_fair():
    n = 100_000
    on = am.decisions(am.table(p=0.5, jitter_sigma=0.05), 2024, 17, np.arange(n), am.tag(0, "real"))
    se = np.sqrt(0.25 / n)
    for k in range(5):
        assert abs(on[:, k].mean() - 0.5) <= 5 * se, (k, on[:, k].mean())
    # and pairwise uncorrelated: the five decisions use five different words
    for a in range(5):
        for b in range(a + 1, 5):
            both = (on[:, a] & on[:, b]).mean()
            assert abs(both - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / n), (a, b, both)


def test_the_twelve_sites_have_their_own_tags():
    from pdgn_amd import augment
    tags = [am.tag(n, r) for n in range(4) for r in am.ROLES]
    assert len(set(tags)) == 12 and not set(tags) & set(am.FEEDER_TAGS) and all(0 <= t < 256 for t in tags)
    assert tags == [augment.site_tag(n, r) for n in range(4) for r in augment.ROLES] and augment.ROLES == am.ROLES
    assert [augment.site_index(n, r) for n in range(4) for r in augment.ROLES] == list(range(12))
    from pdgn_amd import data
    assert data._TAG_ORDER in am.FEEDER_TAGS
    # different tags, rows, clocks and seeds draw different words
    base = am.words(1, 2, [3], tags[0], 0)
    for other in (am.words(1, 2, [3], tags[1], 0), am.words(1, 2, [4], tags[0], 0), am.words(1, 3, [3], tags[0], 0),
                  am.words(2, 2, [3], tags[0], 0), am.words(1, 2 + (1 << 32), [3], tags[0], 0)):
        assert not np.array_equal(base, other)
    with pytest.raises(ValueError):
        augment.site_index(4, "real")
    with pytest.raises(ValueError):
        augment.site_index(0, "test")


# ---------------------------------------------------------------------------- the command line
BASE = ["--model_dir", "m"]


@pytest.mark.parametrize("flag", [["--aug_rotate", "90"], ["--aug_scale", "1.5"], ["--aug_flip"], ["--aug_flip", "0"],
                                  ["--aug_translate", "0.2"], ["--aug_jitter", "0.01"]])
def test_every_range_flag_needs_d_augment(flag, capsys):
    from pdgn_amd import train
    with pytest.raises(SystemExit):
        train.parse_args(BASE + flag)
    assert "needs --d_augment" in capsys.readouterr().err
    assert train.parse_args(BASE + ["--d_augment", "0.5"] + flag).d_augment == 0.5


def test_no_flag_leaves_the_namespace_and_the_logged_line_as_they_were():
    from pdgn_amd import train
    args = train.parse_args(BASE)
    assert not [k for k in vars(args) if k.startswith("aug_") or k == "d_augment"]
    assert "aug" not in str(train.logged_args(args))
    assert args.d_augment is None and train.augment_kwargs(args) is None
    # the namespace of a run without the flags is that of the parser with the new flags taken out again
    p = train.build_parser()
    old = [a.dest for a in p._actions if a.dest not in ("help", "d_augment") and not a.dest.startswith("aug_")
           and a.default is not __import__("argparse").SUPPRESS]
    assert sorted(vars(args)) == sorted(old)


def test_d_augment_defaults_and_overrides():
    from pdgn_amd import augment, train
    kw = train.augment_kwargs(train.parse_args(BASE + ["--d_augment", "0.6"]))
    assert kw == dict(augment.DEFAULTS, p=0.6)
    assert (kw["flip"], kw["rot_max_deg"], kw["scale_max"], kw["trans_max"], kw["jitter_sigma"]) == (True, 180.0, 1.25, 0.1, 0.0)
    kw = train.augment_kwargs(train.parse_args(BASE + ["--d_augment", "1", "--aug_rotate", "30", "--aug_scale", "1.1", "--aug_flip", "0",
                                                       "--aug_translate", "0", "--aug_jitter", "0.02"]))
    assert kw == dict(augment.DEFAULTS, p=1.0, rot_max_deg=30.0, scale_max=1.1, flip=False, trans_max=0.0, jitter_sigma=0.02)
    assert "d_augment=0.6" in str(train.logged_args(train.parse_args(BASE + ["--d_augment", "0.6"])))
    for bad in (["--d_augment", "1.5"], ["--d_augment", "0.5", "--aug_scale", "0.5"], ["--d_augment", "0.5", "--aug_rotate", "-3"]):
        with pytest.raises(SystemExit):
            train.parse_args(BASE + bad)
