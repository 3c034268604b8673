"""CPU: the ragged feeder's host side -- the ABI's two entry points, the permutation of tests/ragged_mirror.py at
small counts and its wrap-around, the mirror against the resampling feeder's mirror on a uniform set, pdgn_amd.clouds.CloudSet's
construction and refusals, the readers and the packed file, the part-annotation split and the command line."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ragged_mirror as gm
import resample_mirror as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------- 1. ABI
def test_abi_declares_and_exports_the_ragged_entry_points():
    from pdgn_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    handle = ctypes.CDLL(build.build())
    vp, ull, ll, i = ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_int
    want = {"pdgn_feed_batch_ragged": (i,) * 6 + (vp, vp, ll, vp, ll, ull, ull, ll, ctypes.c_float) + (vp,) * 7,
            "pdgn_sample_ragged": (i, i, vp, vp, ll, ull, ull, vp, vp)}
    for name, argtypes in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S)), name
        assert _lib.SIGNATURES[name] == (ctypes.c_int, argtypes), name
        assert hasattr(handle, name), name
    define = re.findall(r"^#define\s+PDGN_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M)
    assert len(define) == 1 and int(define[0]) == _lib.ABI_VERSION == handle.pdgn_abi_version() >= 40
    assert "13: the round keys of pdgn_sample_ragged" in text                      # the tag table lists the new tag
    assert gm.TAG_RAGGED == 13 and gm.TAG_RAGGED not in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12) and gm.TAG_RAGGED < 16


# ---------------------------------------------------------------------------- 2. the permutation at every small count
KEYSETS = [rm.round_keys(seed, t, [row])[0] for seed, t, row in
           ((1, 0, 0), (1, 1, 0), (1, 0, 1), (2, 0, 0), (9999, (3 << 32) + 7, 5), (0, 0, 0), ((1 << 63) + 5, 1 << 40, (1 << 32) - 1), (77, 12, 345))]


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1000])
def test_pi_is_a_bijection_at_every_count(M):
    assert len(KEYSETS) == 8
    for keys in KEYSETS:
        pi = gm.perm_columns(M, keys, M)
        assert pi.shape == (M,) and np.array_equal(np.sort(pi), np.arange(M)), (M, keys)
        assert np.array_equal(pi, rm.permute(M, keys.reshape(1, 6))[0])           # the resampling feeder's pi with P = M


@pytest.mark.parametrize("M", [1, 5, 23])
def test_a_short_cloud_is_shown_whole_with_its_duplicates_spread_evenly(M):
    N = 24
    for keys in KEYSETS:
        cols = gm.perm_columns(M, keys, N)
        count = np.bincount(cols, minlength=M)
        assert cols.shape == (N,) and count.shape == (M,)
        assert count.min() >= N // M and count.max() <= -(-N // M) and count.sum() == N, (M, count)
        assert np.array_equal(cols[M:], cols[:N - M])            # column j repeats column j - M


# ---------------------------------------------------------------------------- 3. against the resampling feeder's mirror
@pytest.mark.parametrize("M,N,sizes", [(40, 16, (4, 8, 16)), (16, 16, (3, 6, 9)), (130, 18, (3, 6, 9))])
def test_uniform_set_is_the_resampling_mirrors_batch(M, N, sizes):
    S, B = 7, 3
    clouds = np.random.default_rng(M).standard_normal((S, M, 3)).astype(np.float32)
    for kw in (dict(), dict(rank=1, world=2)):
        mine = gm.MirrorRaggedFeeder(list(clouds), B, sizes, seed=31, num_point=N, **kw)
        theirs = rm.MirrorResampleFeeder(clouds, B, sizes, seed=31, num_point=N, pool=M, **kw)
        assert mine.batches_per_epoch == theirs.batches_per_epoch >= 1
        for epoch in (1, 3):
            for i in range(mine.batches_per_epoch):
                a, a1, a2 = mine.batch(epoch, i)
                b, b1, b2 = theirs.batch(epoch, i)
                for k in range(4):
                    assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (kw, epoch, i, k)
                assert np.array_equal(_bits(a1), _bits(b1)) and np.array_equal(_bits(a2), _bits(b2))


# ---------------------------------------------------------------------------- 4. CloudSet
def _raw_clouds(counts=(1, 2, 3, 5, 17, 64, 200), seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((m, 3)) * rng.uniform(0.5, 4.0) + rng.uniform(-2, 2, 3)).astype(np.float32) for m in counts]


def test_cloudset_refusals():
    from pdgn_amd.clouds import CloudSet
    good = _raw_clouds()
    with pytest.raises(ValueError, match="no clouds"):
        CloudSet.from_clouds([])
    with pytest.raises(ValueError, match="cloud 1.*no points"):
        CloudSet.from_clouds([good[3], np.zeros((0, 3), np.float32)])
    for value in (np.nan, np.inf, -np.inf):
        bad = good[4].copy()
        bad[7, 1] = value
        with pytest.raises(ValueError, match=r"cloud 2 \(c\): point 7 is not finite"):
            CloudSet.from_clouds([good[0], good[1], bad], names=["a", "b", "c"])
    for shape in ((5,), (5, 2), (5, 4), (2, 5, 3), (3, 5)):
        with pytest.raises(ValueError, match=r"\(M,3\)"):
            CloudSet.from_clouds([good[2], np.zeros(shape, np.float32)])
    with pytest.raises(ValueError, match="normalize"):
        CloudSet.from_clouds(good, normalize="global_unit")
    points = np.concatenate(good[:3], 0)
    for off in ([0, 1, 3], [1, 3, 6], [0, 3, 3, 6], [0, 4, 3, 6], [0], [0, 1, 3, 7]):
        with pytest.raises(ValueError):
            CloudSet.from_arrays(points, np.asarray(off, dtype=np.int64))
    with pytest.raises(ValueError):
        CloudSet.from_arrays(points, np.asarray([0.0, 1.0, 3.0, 6.0]))
    with pytest.raises(ValueError, match=r"\(T,3\)"):
        CloudSet.from_arrays(points.reshape(-1, 2), np.asarray([0, 9]))
    ok = CloudSet.from_arrays(points, torch.tensor([0, 1, 3, 6]))
    assert ok.S == 3 and ok.T == 6 and ok.counts().tolist() == [1, 2, 3]


@pytest.mark.parametrize("mode", [None, "shape_unit", "shape_bbox"])
def test_cloudset_normalises_exactly_as_normalize_clouds_does(mode):
    from pdgn_amd.clouds import CloudSet
    from pdgn_amd.data import normalize_clouds
    raw = _raw_clouds(counts=(2, 3, 5, 17, 64, 200, 64, 2048), seed=4)
    cs = CloudSet.from_clouds(raw, normalize=mode)
    assert cs.S == len(raw) and cs.T == sum(len(c) for c in raw) and cs.normalize == mode
    assert cs.points.dtype == torch.float32 and tuple(cs.points.shape) == (cs.T, 3)
    assert cs.off.dtype == torch.int64 and cs.off.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in raw])]).tolist()
    assert cs.counts().tolist() == [len(c) for c in raw]
    for s, c in enumerate(raw):
        want, shift, scale = normalize_clouds(torch.from_numpy(c)[None], mode)
        assert torch.equal(cs.cloud(s), want[0]) if mode is not None else torch.equal(cs.cloud(s), torch.from_numpy(c)), s
        assert torch.equal(cs.cloud(s).view(torch.int32), want[0].view(torch.int32)), s                 # bit for bit
        assert torch.equal(cs.shift[s], shift[0, 0]) and torch.equal(cs.scale[s], scale[0, 0, 0]), s
        assert cs.cloud(s).data_ptr() == cs.points.data_ptr() + 12 * int(cs.off[s])                       # a view
    st = cs.stats(64)
    assert (st["shapes"], st["points"], st["min"], st["max"], st["median"], st["n"], st["shorter"]) == (8, cs.T, 2, 2048, 40.5, 64, 4)
    assert "shorter" not in cs.stats()
    with pytest.raises(IndexError):
        cs.cloud(8)


def test_a_cloud_without_extent_cannot_be_normalised():
    from pdgn_amd.clouds import CloudSet
    one = [np.ones((1, 3), np.float32), _raw_clouds()[4]]
    assert CloudSet.from_clouds(one).S == 2
    for mode in ("shape_unit", "shape_bbox"):
        with pytest.raises(ValueError, match="cloud 0.*without extent"):
            CloudSet.from_clouds(one, normalize=mode)


# ---------------------------------------------------------------------------- 5. readers and the packed file
def _write_root(root, rng):
    """Two categories, a mix of .npy, .pts with 3 columns, .txt with 6 comma-separated columns, .xyz, and a stray README.txt at category
    level -> {sid: {split: [arrays in sorted file-name order]}}."""
    want = {}
    for sid in ("02691156", "03001627"):
        (root / sid).mkdir(parents=True)
        (root / sid / "README.txt").write_text("not a cloud: words, no numbers\n")
        for split, count in (("train", 5), ("val", 2), ("test", 3)):
            folder = root / sid / split
            folder.mkdir()
            clouds = {}
            for j in range(count):
                pc = rng.standard_normal((int(rng.integers(20, 71)), 3)).astype(np.float32)
                kind = ("npy", "pts", "txt", "xyz")[j % 4]
                name = "shape%02d.%s" % (j, kind)
                if kind == "npy":
                    np.save(folder / name, pc)
                elif kind == "txt":                              # ModelNet's resampled files: x,y,z,nx,ny,nz
                    (folder / name).write_text("".join("%r,%r,%r,0.0,1.0,0.0\n" % tuple(float(v) for v in p) for p in pc))
                elif kind == "pts":
                    (folder / name).write_text("".join("%r %r %r\n" % tuple(float(v) for v in p) for p in pc))
                else:                                            # tabs, a label column, an empty line and a comment
                    (folder / name).write_text("# x y z label\n\n" + "".join("%r\t%r\t%r\t3\n" % tuple(float(v) for v in p) for p in pc))
                clouds[name] = pc
            want.setdefault(sid, {})[split] = [clouds[n] for n in sorted(clouds)]
    return want


def _same_root(got, want):
    assert sorted(got) == sorted(want)
    for sid in want:
        assert sorted(got[sid]) == sorted(want[sid])
        for split in want[sid]:
            assert len(got[sid][split]) == len(want[sid][split])
            for a, b in zip(got[sid][split], want[sid][split]):
                assert a.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes(), (sid, split)


def test_pack_round_trip_is_byte_equal_to_reading_the_directory(tmp_path, capsys):
    from pdgn_amd import clouds, meshes
    want = _write_root(tmp_path / "root", np.random.default_rng(11))
    read = clouds.open_ragged_root(str(tmp_path / "root"))
    _same_root(read, want)
    clouds.main(["pack", str(tmp_path / "root"), str(tmp_path / "packed.npz")])
    assert "packed 12 arrays" in capsys.readouterr().out
    with np.load(tmp_path / "packed.npz") as f:
        assert sorted(f.files) == sorted("%s/%s/%s" % (sid, sp, w) for sid in want for sp in want[sid] for w in ("points", "off"))
        assert f["02691156/train/off"].dtype == np.int64 and f["02691156/train/points"].dtype == np.float32
    assert clouds.is_ragged_root(str(tmp_path / "packed.npz")) and not clouds.is_ragged_root(str(tmp_path / "root"))
    assert not meshes.is_mesh_root(str(tmp_path / "packed.npz"))
    _same_root(clouds.open_ragged_root(str(tmp_path / "packed.npz")), read)
    only = clouds.open_ragged_root(str(tmp_path / "packed.npz"), {"03001627"})
    assert sorted(only) == ["03001627"] and sorted(clouds.open_ragged_root(str(tmp_path / "root"), {"03001627"})) == ["03001627"]
    # one CloudSet of a split: the categories in sorted order, short shapes dropped where asked
    cs = clouds.split_cloudset(str(tmp_path / "packed.npz"), "train", "shape_unit")
    flat = want["02691156"]["train"] + want["03001627"]["train"]
    assert cs.S == 10 and cs.dropped == 0 and cs.counts().tolist() == [len(c) for c in flat]
    k = sorted(len(c) for c in flat)[3]
    cut = clouds.split_cloudset(read, "train", None, min_points=k)
    assert cut.dropped == sum(len(c) < k for c in flat) > 0 and cut.S == 10 - cut.dropped and cut.counts().min() >= k
    assert torch.equal(cut.cloud(0), torch.from_numpy([c for c in flat if len(c) >= k][0]))
    with pytest.raises(ValueError, match="no cloud"):
        clouds.split_cloudset(read, "train", None, min_points=1000)
    # an equal-count .npz of the cloud path and a mesh file are not ragged roots
    np.savez(tmp_path / "equal.npz", **{"03001627/train": np.zeros((2, 8, 3), np.float32)})
    assert not clouds.is_ragged_root(str(tmp_path / "equal.npz")) and not clouds.is_ragged_root(str(tmp_path / "missing.npz"))
    with pytest.raises(SystemExit):
        clouds.main(["pack", str(tmp_path / "root")])
    with pytest.raises(ValueError, match="three coordinates"):
        (tmp_path / "bad.pts").write_text("1 2 3\n4 5\n")
        clouds.load_cloud(str(tmp_path / "bad.pts"))


def test_part_layout_makes_the_90_10_split_by_sorted_name(tmp_path):
    from pdgn_amd import clouds
    rng = np.random.default_rng(12)
    root = tmp_path / "part"
    root.mkdir()
    (root / "synsetoffset2category.txt").write_text("Airplane\t02691156\nChair\t03001627\n")
    stored = {}
    for sid, count in (("02691156", 23), ("03001627", 10)):
        (root / sid / "points").mkdir(parents=True)
        (root / sid / "points_label").mkdir()
        for j in rng.permutation(count).tolist():                # (written in another order than the names sort in)
            pc = rng.standard_normal((int(rng.integers(5, 30)), 3)).astype(np.float32)
            (root / sid / "points" / ("%04x.pts" % j)).write_text("".join("%r %r %r\n" % tuple(float(v) for v in p) for p in pc))
            (root / sid / "points_label" / ("%04x.seg" % j)).write_text("1\n" * len(pc))
            stored[(sid, "%04x.pts" % j)] = pc
    clouds.main(["pack", "--layout", "part", str(root), str(tmp_path / "part.npz")])
    got = clouds.open_ragged_root(str(tmp_path / "part.npz"))
    for sid, count in (("02691156", 23), ("03001627", 10)):
        names = sorted(n for s, n in stored if s == sid)
        cut = int(count * 0.9)
        assert cut in (20, 9)
        want = {"train": [stored[(sid, n)] for n in names[:cut]], "test": [stored[(sid, n)] for n in names[cut:]]}
        want["val"] = want["test"]
        _same_root({sid: got[sid]}, {sid: want})


# ---------------------------------------------------------------------------- 6. command line
BASE = ["--model_dir", "toy", "--data_root", "nowhere"]


def test_flags_parse_and_a_run_without_them_has_the_old_namespace():
    from pdgn_amd import train
    args = train.parse_args(BASE + ["--ragged", "--min_points", "30"])
    assert args.ragged is True and args.min_points == 30
    assert "ragged=True" in str(train.logged_args(args)) and "min_points=30" in str(train.logged_args(args))
    plain = train.parse_args(BASE)
    assert "ragged" not in vars(plain) and "min_points" not in vars(plain)
    assert plain.ragged is False and plain.min_points == 1
    assert "ragged" not in str(train.logged_args(plain)) and "min_points" not in str(train.logged_args(plain))
    with pytest.raises(SystemExit):
        train.parse_args(BASE + ["--min_points", "0"])


def test_flags_that_cannot_apply_to_ragged_data_are_refused_with_a_sentence(tmp_path):
    from pdgn_amd import clouds, train
    _write_root(tmp_path / "root", np.random.default_rng(13))
    clouds.pack(str(tmp_path / "root"), str(tmp_path / "packed.npz"))
    for data, extra in ((tmp_path / "packed.npz", []), (tmp_path / "root", ["--ragged"])):
        common = ["--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root", str(data), "--num_point", "16",
                  "--choice", "chair"] + extra
        root = train._ragged_root(train.parse_args(common))
        assert sorted(root) == ["03001627"] and len(root["03001627"]["train"]) == 5
        for phase in ("train", "test"):
            for mode in ("on", "compute"):
                with pytest.raises(SystemExit, match="--mesh_visible %s.*ragged.*no faces" % mode):
                    train.main(common + ["--phase", phase, "--mesh_visible", mode])
            with pytest.raises(SystemExit, match="--resample_pool.*ragged.*no common leading pool"):
                train.main(common + ["--phase", phase, "--resample_pool", "20"])
        assert train._ragged_root(train.parse_args(common + ["--mesh_visible", "off"])) is not None
        with pytest.raises(SystemExit, match="--choice lamp.*no clouds of that category"):
            train._ragged_root(train.parse_args(common[:-2 - len(extra)] + ["--choice", "lamp"] + extra))
    # without --ragged a directory is not ragged data, and open_data_root still refuses its unequal counts
    plain = train.parse_args(["--model_dir", "toy", "--data_root", str(tmp_path / "root"), "--num_point", "16"])
    assert train._ragged_root(plain) is None
    with pytest.raises(ValueError, match="every cloud of a data set must store the same number of points"):
        train.open_data_root(str(tmp_path / "root"))
    with pytest.raises(SystemExit, match="--min_points.*does not hold ragged clouds"):
        train._ragged_root(train.parse_args(["--model_dir", "toy", "--data_root", str(tmp_path / "root"), "--min_points", "5"]))
    with pytest.raises(SystemExit, match="--ragged.*neither a directory"):
        train._ragged_root(train.parse_args(["--model_dir", "toy", "--data_root", str(tmp_path / "nothing.h5"), "--ragged"]))
