"""Normal orientation from visibility, the part that needs no GPU: the numpy mirror of csrc/cloudvis.hip
(tests/cloudvis_mirror.py) orients the thin slabs on which the spanning-tree propagation (tests/orient_mirror.py) fails, and tori; its
invariances, its degenerate inputs, and the plumbing (header, ABI, wrappers, command line)."""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import cloudvis_mirror as cm
import normals_mirror as nm
import orient_mirror as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
D = cm.DEFAULTS
SLABS = [(t, seed) for t in (0.04, 0.08) for seed in (0, 1)]
TORI = [(n, seed) for n in (512, 2048) for seed in (0, 1)]
CAP = 0.01                                                         # of the sure points: wrong, and undecided


def _views(n=26):
    from pdgn_amd.meshes import default_views
    return default_views(n)


@functools.lru_cache(maxsize=None)
def _prepared(kind, a, seed):
    """(x, analytic normals, idx, unoriented estimate) of a slab of thickness a or a torus of a points: computed once per session."""
    x, analytic = cm.slab(2048, a, seed) if kind == "slab" else om.torus(a, seed)
    idx = nm.knn_indices(x, D["k"])
    g = nm.estimate_cloud(x, idx)[0]
    for arr in (x, analytic, idx, g):
        arr.setflags(write=False)
    return x, analytic, idx, g


def _visible(x, g, idx, rounds=D["rounds"], views=None, R=D["resolution"]):
    """The mirror at the defaults of pointops.orient_normals_visible -> (o, pooled, stats, votes)."""
    frame = cm.cloud_frame(x)
    radius = D["radius_factor"] * cm.mean_spacing(x)
    splat, bias = cm.quanta(radius, D["bias_factor"] * radius, frame[3], R)
    votes = cm.votes_cloud(x, g, frame, _views() if views is None else views, R, splat, bias)
    return cm.pool_cloud(x, g, idx, votes, rounds) + (votes,)


@pytest.mark.parametrize("t,seed", SLABS)
def test_the_propagation_fails_on_a_thin_slab_and_the_views_do_not(t, seed):
    x, analytic, idx, g = _prepared("slab", t, seed)
    tree = om.orient_cloud(x, g, idx)
    sure, wrong, _ = cm.wrong_and_undecided(tree[0], None, analytic, g)
    print("slab t=%g seed %d: %d sure points; propagation %d wrong, %d weak edges" % (t, seed, sure, wrong, tree[2][2]))
    assert sure > 1000 and wrong >= 0.40 * sure
    o, pooled, stats, _ = _visible(x, g, idx)
    sure, wrong, undecided = cm.wrong_and_undecided(o, pooled, analytic, g)
    print("    views: %d wrong, %d undecided; stats %s" % (wrong, undecided, stats))
    assert wrong <= CAP * sure and undecided <= CAP * sure


@pytest.mark.parametrize("n,seed", TORI)
def test_the_views_orient_a_torus(n, seed):
    x, analytic, idx, g = _prepared("torus", n, seed)
    o, pooled, stats, _ = _visible(x, g, idx)
    sure, wrong, undecided = cm.wrong_and_undecided(o, pooled, analytic, g)
    print("torus n=%d seed %d: %d sure, %d wrong, %d undecided; stats %s" % (n, seed, sure, wrong, undecided, stats))
    assert sure > 0.9 * n and wrong <= CAP * sure and undecided <= CAP * sure


def test_a_permutation_of_the_points_permutes_votes_and_outputs():
    x, _, idx, g = _prepared("torus", 512, 0)
    perm = np.random.default_rng(5).permutation(512)
    inv = np.argsort(perm)
    o, pooled, stats, votes = _visible(x, g, idx)
    o2, pooled2, stats2, votes2 = _visible(x[perm], g[perm], inv[idx[perm]].astype(np.int32))
    assert np.array_equal(votes2, votes[perm]) and np.array_equal(pooled2, pooled[perm]) and nm.same_bits(o2, o[perm]) and stats2 == stats


def test_shuffled_slots_change_no_bit_and_a_repeated_slot_counts_twice():
    x, _, idx, g = _prepared("torus", 512, 1)
    rng = np.random.default_rng(6)
    _, pooled, stats, votes = _visible(x, g, idx, rounds=2)
    shuffled = np.stack([row[rng.permutation(row.size)] for row in idx])
    o2, pooled2, stats2 = cm.pool_cloud(x, g, shuffled, votes, 2)
    assert np.array_equal(pooled2, pooled) and stats2 == stats
    # one more copy of slot 1 in every row: after one round the balance grows by exactly that neighbour's term
    i, j, c = cm.coefficients(x, g, idx[:, 1:2])
    extra = np.zeros(512, dtype=np.int64)
    v0 = votes[:, 0].astype(np.int64) - votes[:, 1].astype(np.int64)
    np.add.at(extra, i, c * v0[j])
    assert (c != 0).sum() > 100
    once = cm.pool_cloud(x, g, idx, votes, 1)[1]
    twice = cm.pool_cloud(x, g, np.concatenate([idx, idx[:, 1:2]], axis=1), votes, 1)[1]
    assert np.array_equal(twice, once + extra) and (extra != 0).any()


def test_no_round_is_the_sign_of_the_raw_votes_and_only_sign_bits_change():
    x, _, idx, g = _prepared("slab", 0.08, 0)
    o, pooled, stats, votes = _visible(x, g, idx, rounds=0)
    v0 = votes[:, 0].astype(np.int64) - votes[:, 1].astype(np.int64)
    assert np.array_equal(pooled, v0) and nm.same_bits(o, np.where((v0 < 0)[:, None], -g, g))
    assert stats == (int((v0 < 0).sum()), int((v0 == 0).sum()), int((votes.sum(axis=1) == 0).sum()), 0)
    for rounds in (1, 2, 4):
        o, pooled, _, _ = _visible(x, g, idx, rounds=rounds)
        changed = o.view(np.uint32) ^ g.view(np.uint32)
        assert np.isin(changed, (0, 0x80000000)).all() and np.array_equal((changed != 0).all(axis=1), pooled < 0)
        assert np.array_equal((changed != 0).any(axis=1), pooled < 0)
    assert votes.max() <= 26 * 256


def test_no_splat_writes_the_own_pixel_only_and_a_splat_beyond_the_image_writes_every_pixel():
    rng = np.random.default_rng(7)
    R = 16
    X, Y, Z = rng.integers(0, 256 * R + 1, 40), rng.integers(0, 256 * R + 1, 40), rng.integers(0, 1 << 21, 40)
    X[:2], Y[:2] = (256 * R, 128), (0, 128 + 256)                    # the rim (clamped to the last pixel), and a pixel centre exactly
    buf = cm.depth_buffer(X, Y, Z, R, 0)
    want = np.full((R, R), cm.EMPTY, dtype=np.int64)
    np.minimum.at(want, (np.minimum(Y >> 8, R - 1), np.minimum(X >> 8, R - 1)), Z)
    assert np.array_equal(buf, want) and (buf != cm.EMPTY).sum() <= 40 and buf[0, R - 1] <= Z[0] and buf[1, 0] <= Z[1]
    assert (cm.depth_buffer(X, Y, Z, R, 256 * R * 2) == Z.min()).all()
    # below a pixel: a disc of 100 sub-pixel units reaches a centre only within 100 of it
    one = cm.depth_buffer(np.array([256 * 3 + 128 + 60]), np.array([256 * 5 + 128 - 80]), np.array([9]), R, 100)
    assert (one != cm.EMPTY).sum() == 1 and one[5, 3] == 9
    far = cm.depth_buffer(np.array([256 * 3 + 255]), np.array([256 * 5]), np.array([9]), R, 100)
    assert (far != cm.EMPTY).sum() == 1 and far[5, 3] == 9            # (no centre within reach: the own pixel alone)


def test_a_point_on_the_rim_of_the_frame_clamps_its_pixel_and_a_zero_normal_casts_no_vote():
    views = _views(6)
    x = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [0.25, 0.25, 0.25]], dtype=F)
    g = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [0, 0, 0]], dtype=F)
    frame = np.array([0, 0, 0, 1], dtype=F)                         # every one of the first four lies ON the ball: X or Y = 2^8 R in some view
    votes, seen = cm.votes_cloud(x, g, frame, views, 16, 0, 0, return_passes=True)
    # the two views along x hold the first two points in ONE pixel, the middle one: each hides the other from behind (bias 0); the
    # views along a normal are the only ones with a vote, one from the front and -- where nothing hides the point -- one from the back
    assert seen.sum() == 5 * 6 - 2 and seen[:, 2:].all()
    assert np.array_equal(votes, np.array([[256, 0], [256, 0], [256, 256], [256, 256], [0, 0]], dtype=np.uint32))
    o, pooled, stats = cm.pool_cloud(x, g, np.zeros((5, 1), dtype=np.int32), votes, 1)
    assert nm.same_bits(o, g) and np.array_equal(pooled, (512, 512, 0, 0, 0)) and stats == (0, 3, 1, 0)


def test_poison_is_contained():
    """A NaN normal, an infinite coordinate, out-of-range and self slots: the dead points get no votes, splat nothing, keep their bits and
    give their neighbours nothing; every other point's result is the one of the cloud without them."""
    x, _, idx, g = (a.copy() for a in _prepared("torus", 512, 0))
    g[10, 1], x[20, 2] = np.nan, np.inf
    idx[30, 3], idx[31, 4], idx[32, 5] = 512, -1, 32
    o, pooled, stats, votes = _visible(x, g, idx)
    assert stats[3] == 2 and (votes[[10, 20]] == 0).all() and (pooled[[10, 20]] == 0).all()
    assert o[10].tobytes() == g[10].tobytes() and o[20].tobytes() == g[20].tobytes()
    keep = np.setdiff1d(np.arange(512), [10, 20])
    remap = np.full(513, -1, dtype=np.int64)
    remap[keep] = np.arange(510)
    sub = remap[np.clip(idx[keep].astype(np.int64), -1, 512)].astype(np.int32)
    frame = cm.cloud_frame(x)                                       # (the dead points do not count towards the frame)
    assert np.array_equal(frame, cm.cloud_frame(x[keep]))
    radius = D["radius_factor"] * cm.mean_spacing(_prepared("torus", 512, 0)[0])
    splat, bias = cm.quanta(radius, D["bias_factor"] * radius, frame[3], 64)
    full = cm.votes_cloud(x, g, frame, _views(), 64, splat, bias)
    part = cm.votes_cloud(x[keep], g[keep], frame, _views(), 64, splat, bias)
    assert np.array_equal(full[keep], part)
    assert np.array_equal(cm.pool_cloud(x, g, idx, full, 2)[1][keep], cm.pool_cloud(x[keep], g[keep], sub, part, 2)[1])


def test_one_point_is_seen_by_every_view():
    x, g = np.array([[0.3, -0.2, 0.1]], dtype=F), np.array([[0.6, 0.0, 0.8]], dtype=F)
    frame = cm.cloud_frame(x)
    assert np.array_equal(frame, np.array([0.3, -0.2, 0.1, 1.0], dtype=F))
    views = _views()
    votes, seen = cm.votes_cloud(x, g, frame, views, 8, 384, 0, return_passes=True)
    assert seen.all()
    s = (views[:, 2, :].astype(np.float64) * g[0]).sum(axis=1)
    assert abs(int(votes[0, 0]) - np.floor(256 * -s[s < 0]).sum()) <= 26 and abs(int(votes[0, 1]) - np.floor(256 * s[s > 0]).sum()) <= 26
    assert votes[0, 0] == votes[0, 1]                               # (the view table holds every direction with its opposite)
    o, pooled, stats = cm.pool_cloud(x, g, np.zeros((1, 1), dtype=np.int32), votes, 4)
    assert pooled[0] == 0 and stats == (0, 1, 0, 0) and nm.same_bits(o, g)


def test_the_header_the_abi_and_the_wrappers():
    from pdgn_amd import _lib, export, pointops, reconstruct
    text = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    assert _lib.ABI_VERSION >= 51
    votes, pool = _lib.SIGNATURES["pdgn_cloud_normal_votes"], _lib.SIGNATURES["pdgn_orient_pool"]
    assert len(votes[1]) == 12 and len(pool[1]) == 13
    assert "%d entry points" % len(_lib.SIGNATURES) in open(os.path.join(ROOT, "README.md")).read()
    assert int(re.search(r"#define PDGN_CLOUDVIS_MAX_ROUNDS (\d+)", text).group(1)) == cm.MAX_ROUNDS == pointops.POOL_MAX_ROUNDS
    assert int(re.search(r"#define PDGN_VISIBLE_MAX_RES (\d+)", text).group(1)) == pointops.VISIBLE_MAX_RESOLUTION
    assert int(re.search(r"#define PDGN_VISIBLE_MAX_VIEWS (\d+)", text).group(1)) == pointops.VISIBLE_MAX_VIEWS
    if os.path.exists(_lib.SO_PATH):
        L = _lib.lib()
        assert L.pdgn_abi_version() == _lib.ABI_VERSION
        assert L.pdgn_cloud_normal_votes(1, 1, None, None, None, None, 6, 8, 0, 0, None, None) == -1
        assert L.pdgn_orient_pool(1, 1, 1, None, None, None, None, 1, None, None, None, None, None) == -1
    # the mirror's defaults are the wrappers'
    for fn in (pointops.normal_votes, pointops.orient_normals_visible):
        par = inspect.signature(fn).parameters
        assert par["views"].default == D["views"] and par["resolution"].default == D["resolution"]
        assert par["radius_factor"].default == D["radius_factor"] and par["bias_factor"].default == D["bias_factor"]
    par = inspect.signature(pointops.orient_normals_visible).parameters
    assert par["rounds"].default == D["rounds"] and par["k"].default == D["k"]
    assert inspect.signature(reconstruct.reconstruct).parameters["orient"].default == "consistent"
    p = export.build_parser()
    args = p.parse_args(["a.npy", "-o", "out", "--orient", "visible", "--orient_views", "14", "--orient_resolution", "96",
                         "--orient_radius_factor", "2.5", "--orient_rounds", "2"])
    assert (args.orient, args.orient_views, args.orient_resolution, args.orient_radius_factor, args.orient_rounds) == ("visible", 14, 96, 2.5, 2)
    assert p.parse_args(["a.npy", "-o", "out"]).orient == "outward"
    for bad in (["--orient_rounds", "2"], ["--orient", "visible", "--orient_rounds", "5"], ["--orient", "visible", "--orient_resolution", "193"],
                ["--orient", "visible", "--orient_views", "7"], ["--orient", "visible", "--orient_radius_factor", "0"]):
        with pytest.raises(SystemExit):
            export.main(["missing.npy", "-o", "out"] + bad)
