"""Host: the farthest-point mirror (tests/fps_mirror.py) is a farthest-point sampler, the ABI declares the two entry points of
csrc/fps.hip, and the command line's --subsample.  (BatchFeeder's refusals need a device tensor: tests/test_gpu_fps.py.)"""
import numpy as np
import pytest

import fps_mirror as fpm
from hashweights import lattice_points


def _radius(xyz, order):
    """The distance, in fp64, from each chosen point to the nearest point chosen before it (entry 0: inf)."""
    p = xyz[order].astype(np.float64)
    out = np.full(len(order), np.inf)
    for j in range(1, len(order)):
        out[j] = np.sqrt(((p[:j] - p[j]) ** 2).sum(axis=1).min())
    return out


def _gaussian(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)


CLOUDS = {"lattice": lambda: lattice_points("fps.host", (300, 3), bits=6), "gaussian": lambda: _gaussian(300, 0)}


@pytest.mark.parametrize("kind", sorted(CLOUDS))
@pytest.mark.parametrize("start", [0, 299, 17])
def test_mirror_is_a_farthest_point_sampler(kind, start):
    xyz = CLOUDS[kind]()
    n = xyz.shape[0]
    full = fpm.fps_order(xyz, n, start)
    assert full[0] == start and full.dtype == np.int64
    for m in (1, 2, 37, 256):                                    # order[:m] is a prefix of order[:m']
        assert np.array_equal(fpm.fps_order(xyz, m, start), full[:m])
    distinct = len({tuple(p) for p in xyz.tolist()})
    assert len(set(full[:distinct].tolist())) == distinct        # no index twice while distinct points remain
    r = _radius(xyz, full[:distinct])
    assert np.all(np.diff(r[1:]) <= 0.0)                         # the selection radius never grows
    # each choice IS a farthest point: no point is farther from the chosen set than the one taken (fp64, up to fp32 rounding of d^2)
    for j in (1, 2, 9, 100):
        d2 = ((xyz[:, None, :].astype(np.float64) - xyz[full[:j]][None].astype(np.float64)) ** 2).sum(axis=2).min(axis=1)
        assert d2[full[j]] >= d2.max() * (1 - 4 * 2.0 ** -24)


def test_mirror_breaks_ties_by_the_lowest_index():
    # the corners of a square, each twice: after corner 0 the opposite corner (indices 2 and 6) is farthest -> 2; then 1 and 3 (and 5, 7) tie -> 1
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]] * 2, dtype=np.float32)
    assert fpm.fps_order(sq, 8).tolist() == [0, 2, 1, 3, 0, 0, 0, 0]
    # all-equal points: index 0 after the start, whatever the start
    same = np.full((50, 3), 0.25, dtype=np.float32)
    assert fpm.fps_order(same, 50, 7).tolist() == [7] + [0] * 49
    # every point duplicated: the first copy is the one taken; once the 40 distinct points are used up, index 0 repeats
    xyz = lattice_points("fps.host.dup", (40, 3), bits=6)
    assert len({tuple(p) for p in xyz.tolist()}) == 40
    dup = np.concatenate([xyz, xyz])
    order = fpm.fps_order(dup, 80)
    assert np.array_equal(order[:40], fpm.fps_order(xyz, 40)) and order[:40].max() < 40 and order[40:].tolist() == [0] * 40


def test_mirror_distances_are_the_kernels_chain():
    p = np.array([[0.5, -0.25, 0.125], [1e-3, 2e-3, 3e-3]], dtype=np.float32)
    q = np.array([-0.5, 0.75, 0.0], dtype=np.float32)
    d = fpm.sqdist3(p, q)
    assert d.dtype == np.float32 and d[0] == np.float32(1.0 + 1.0 + 0.015625)            # exact on the lattice
    dx, dy, dz = [np.float64(np.float32(p[1, k] - q[k])) for k in range(3)]
    inner = np.float32(dx * dx)
    inner = np.float32(dy * dy + np.float64(inner))
    assert d[1] == np.float32(dz * dz + np.float64(inner))


def test_start_indices_come_from_the_feeders_generator():
    import feed_mirror as fm
    rows = np.arange(5) + 3
    got = fpm.start_indices(9999, (1 << 32) + 7, rows, 2048)
    words = fm.stream_words(9999, (1 << 32) + 7, rows, fpm.TAG_FPS, 4)[:, 0]
    assert np.array_equal(got, (words.astype(np.uint64) * np.uint64(2048)) >> np.uint64(32))
    assert got.min() >= 0 and got.max() < 2048 and len(set(got.tolist())) > 1
    assert fpm.TAG_FPS not in (0, 1, 2, fm.TAG_Z1, fm.TAG_Z2, fm.TAG_ORDER, 6) and fpm.TAG_FPS < 16     # feed.hip's tags; augment.hip's start at 16
    # a stream of its own: not the words of any other tag
    for tag in range(7):
        assert not np.array_equal(fm.stream_words(9999, 5, rows, tag, 1), fm.stream_words(9999, 5, rows, fpm.TAG_FPS, 1))


def test_pyramid_levels_are_nested_prefixes():
    p4 = np.ascontiguousarray(lattice_points("fps.host.pyr", (3, 64, 3), bits=6).transpose(0, 2, 1))
    levels, order = fpm.pyramid(p4, (8, 16, 32), seed=5, t=11, rows=np.arange(3))
    assert [l.shape for l in levels] == [(3, 3, 8), (3, 3, 16), (3, 3, 32)] and order.shape == (3, 32)
    assert np.array_equal(order[:, 0], fpm.start_indices(5, 11, np.arange(3), 64))
    assert np.array_equal(levels[0], levels[1][:, :, :8]) and np.array_equal(levels[1], levels[2][:, :, :16])
    for b in range(3):
        assert np.array_equal(levels[2][b], p4[b][:, order[b]])


def test_abi_declares_the_entry_points():
    import ctypes
    from pdgn_amd import _lib
    assert _lib.ABI_VERSION >= 36
    vp, i, ull, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_longlong
    assert _lib.SIGNATURES["pdgn_fps_order"] == (i, (i, i, i, vp, vp, vp, vp))
    assert _lib.SIGNATURES["pdgn_feed_fps_pyramid"] == (i, (i, i, i, i, i, vp, ull, ull, ll, vp, vp, vp, vp, vp))
    with open(_lib.HEADER) as f:
        text = f.read()
    assert "#define PDGN_FEED_TAG_FPS %d" % fpm.TAG_FPS in text and "#define PDGN_FPS_MAX_N %d" % fpm.MAX_N in text


def test_subsample_flag_parses_and_is_absent_when_not_given():
    from pdgn_amd import train
    base = ["--model_dir", "m"]
    plain = train.parse_args(base)
    assert "subsample" not in vars(plain) and plain.subsample == "random"
    assert "subsample" not in str(train.logged_args(plain))                     # the log's first line of an unflagged run is unchanged
    for value in ("random", "fps"):
        args = train.parse_args(base + ["--subsample", value])
        assert vars(args)["subsample"] == value and ("subsample='%s'" % value) in str(train.logged_args(args))
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--subsample", "grid"])
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--subsample", "fps", "--num_point", "16384"])
    assert train.parse_args(base + ["--subsample", "random", "--num_point", "16384"]).num_point == 16384


def test_unknown_subsample_is_refused_before_anything_else():
    import torch
    from pdgn_amd.data import BatchFeeder
    with pytest.raises(ValueError, match="subsample"):
        BatchFeeder(torch.zeros(4, 16, 3), 2, (2, 4, 8), seed=0, subsample="grid")
