"""CPU: the resampling feeder's host side -- the keyed permutation of tests/resample_mirror.py is a bijection
and uniform at the workload's pool, the PC15k directory loader, the tail cut of the test phase and the reports, the command line's and
train()'s refusals, the log's unchanged first line, and the entry point's host-side argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import feed_mirror as fm
import resample_mirror as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- the permutation
def test_half_bits():
    # bits = max(2, bit length of P - 1), h = ceil(bits / 2): even and odd bit counts, the 2^k / 2^k + 1 boundaries
    want = {1: 1, 2: 1, 4: 1, 5: 2, 16: 2, 17: 3, 1024: 5, 1025: 6, 2048: 6, 2049: 6, 4096: 6, 4097: 7, 15000: 7, 16384: 7, 16385: 8}
    for P, h in want.items():
        assert rm.half_bits(P) == h, P
        assert P <= 1 << (2 * h) <= 4 * P


@pytest.mark.parametrize("sizes", [range(1, 301), (1024, 1025, 2048, 2049, 4097, 15000)], ids=["1-300", "boundaries"])
def test_pi_is_a_bijection(sizes):
    for P in sizes:
        keys = rm.round_keys(seed=11 + P, t=P, rows=np.arange(20))          # 20 key sets per P
        assert keys.shape == (20, 6)
        pi = rm.permute(P, keys)
        assert pi.shape == (20, P)
        assert np.array_equal(np.sort(pi, axis=1), np.broadcast_to(np.arange(P), (20, P))), P


def test_keys_are_stream_six_and_depend_on_seed_row_and_t():
    k = rm.round_keys(9999, 5, np.array([0, 1]))
    w0 = fm.philox4x32_10((0, np.array([0, 1]), 5, 6), (9999, 0))
    w1 = fm.philox4x32_10((1, np.array([0, 1]), 5, 6), (9999, 0))
    assert np.array_equal(k, np.concatenate([w0, w1[:, :2]], axis=1))
    hi = rm.round_keys(9999, 5 + (3 << 32), np.array([0]))                   # the high part of t sits above the tag
    assert np.array_equal(hi[0, :4], fm.philox4x32_10((0, 0, 5, 6 | 3 << 8), (9999, 0)))
    base = rm.permute(15000, k[:1], 2048)
    for other in (rm.round_keys(9998, 5, [0]), rm.round_keys(9999, 6, [0]), k[1:]):
        assert not np.array_equal(rm.permute(15000, other, 2048), base)


def test_draws_are_uniform_at_the_workloads_pool():
    """P = 15 000, N = 2048, 4000 independent (row, t) draws.  Inclusion counts per source point against the hypergeometric variance
    e (1 - N / P), and the source index of output column 0 against e0 = 4000 / P: chi^2 / dof in [0.95, 1.05] (dof = 14 999:
    sigma = sqrt(2 / dof) = 0.0115).  Not run at tiny P: with h <= 3 bits the round function is visibly non-uniform and only
    bijectivity is claimed there."""
    P, N, draws = 15000, 2048, 4000
    inclusion, first = np.zeros(P), np.zeros(P)
    for t in range(40):
        pi = rm.permute(P, rm.round_keys(9999, t, np.arange(100)), N)
        assert pi.min() >= 0 and pi.max() < P
        inclusion += np.bincount(pi.ravel(), minlength=P)
        first += np.bincount(pi[:, 0], minlength=P)
    e = draws * N / P
    chi_inclusion = ((inclusion - e) ** 2 / (e * (1 - N / P))).sum() / (P - 1)
    e0 = draws / P
    chi_first = ((first - e0) ** 2 / e0).sum() / (P - 1)
    print("resample: chi^2/dof inclusion %.4f, column 0 %.4f" % (chi_inclusion, chi_first))
    assert 0.95 <= chi_inclusion <= 1.05, chi_inclusion
    assert 0.95 <= chi_first <= 1.05, chi_first


def test_mirror_feeder_draws():
    S, M, N, P, B = 11, 96, 64, 70, 3
    clouds = np.random.default_rng(0).standard_normal((S, M, 3)).astype(np.float32)
    f = rm.MirrorResampleFeeder(clouds, B, (8, 16, 32), seed=3, num_point=N, pool=P)
    ids, idx, w1, w2 = f.draws(1, 0)
    assert [i.shape for i in idx] == [(B, 8), (B, 16), (B, 32), (B, N)]
    assert all(i.max() < P for i in idx) and all(len(set(row)) == N for row in idx[3].tolist())
    plain = fm.MirrorFeeder(clouds, B, (8, 16, 32), seed=3)
    pid, _, p1, p2 = plain.draws(1, 0)
    assert np.array_equal(ids, pid) and np.array_equal(w1, p1) and np.array_equal(w2, p2)     # same order, same noise words
    reals, _, _ = f.batch(1, 0)
    assert [r.shape for r in reals] == [(B, 3, 8), (B, 3, 16), (B, 3, 32), (B, 3, N)]
    assert np.array_equal(reals[3][1, :, 5], clouds[ids[1], idx[3][1, 5]])
    # two ranks at B draw what one rank draws at 2 B
    one = rm.MirrorResampleFeeder(clouds, 4, (8, 16, 32), seed=3, num_point=N, pool=P)
    halves = [rm.MirrorResampleFeeder(clouds, 2, (8, 16, 32), seed=3, rank=r, world=2, num_point=N, pool=P) for r in range(2)]
    for k in range(4):
        assert np.array_equal(np.concatenate([h.draws(2, 1)[1][k] for h in halves]), one.draws(2, 1)[1][k])


# ---------------------------------------------------------------------------- loading
def _write_pc15k(root, M, counts=(("train", 5), ("val", 2), ("test", 3)), cates=("chair",), seed=2):
    from pdgn_amd.data import cate_to_synsetid
    rng = np.random.default_rng(seed)
    made = {}
    for c in cates:
        for sp, n in counts:
            folder = root / cate_to_synsetid[c] / sp
            folder.mkdir(parents=True)
            for j in range(n):
                pc = rng.standard_normal((M, 3)).astype(np.float32)
                np.save(folder / ("%s_%03d.npy" % (sp, n - j)), pc)                  # written in DESCENDING name order
                made[(cate_to_synsetid[c], sp, "%s_%03d.npy" % (sp, n - j))] = pc
    return made


def test_directory_loader(tmp_path):
    from pdgn_amd import train
    from pdgn_amd.data import cate_to_synsetid
    made = _write_pc15k(tmp_path / "pc", 24, cates=("chair", "airplane"))
    (tmp_path / "pc" / "README.txt").write_text("not a category")
    src = train.open_data_root(str(tmp_path / "pc"))
    assert set(src) == {cate_to_synsetid["chair"], cate_to_synsetid["airplane"]}
    for sid in src:
        assert {sp: a.shape for sp, a in src[sid].items()} == {"train": (5, 24, 3), "val": (2, 24, 3), "test": (3, 24, 3)}
        assert src[sid]["train"].dtype == np.float32
        for j in range(5):                                                       # sorted name order
            assert np.array_equal(src[sid]["train"][j], made[(sid, "train", "train_%03d.npy" % (j + 1))])
    only = train.open_data_root(str(tmp_path / "pc"), {cate_to_synsetid["chair"]})
    assert set(only) == {cate_to_synsetid["chair"]}
    # through ShapeNetCore, as the command line goes
    args = train.parse_args(["--model_dir", "m", "--data_root", str(tmp_path / "pc"), "--choice", "chair", "--num_point", "16"])
    ds = train.load_split(args, "train", "shape_unit")
    assert len(ds) == 5 and tuple(ds.stack().shape) == (5, 24, 3) and {d["cate"] for d in ds.pointclouds} == {"chair"}
    args.choice = None
    assert len(train.load_split(args, "test", "shape_bbox")) == 6


def test_directory_loader_refuses_unequal_point_counts(tmp_path):
    from pdgn_amd import train
    from pdgn_amd.data import cate_to_synsetid
    _write_pc15k(tmp_path / "pc", 24)
    np.save(tmp_path / "pc" / cate_to_synsetid["chair"] / "val" / "zz.npy", np.zeros((23, 3), np.float32))
    with pytest.raises(ValueError, match="23 points.*24"):
        train.open_data_root(str(tmp_path / "pc"))
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no .*npy"):
        train.open_data_root(str(tmp_path / "empty"))


@pytest.mark.parametrize("kind", ["dir", "npz"])
def test_reference_clouds_are_the_tails(tmp_path, kind):
    """--phase test and the reports: the LAST num_point points of every stored cloud, cut before normalisation."""
    from pdgn_amd import train
    from pdgn_amd.data import ShapeNetCore, cate_to_synsetid, normalize_clouds
    M, N = 24, 16
    made = _write_pc15k(tmp_path / "pc", M)
    sid = cate_to_synsetid["chair"]
    stored = {sp: np.stack([made[(sid, sp, "%s_%03d.npy" % (sp, j + 1))] for j in range(n)]) for sp, n in (("train", 5), ("val", 2), ("test", 3))}
    root = tmp_path / "pc"
    if kind == "npz":
        root = tmp_path / "toy.npz"
        np.savez(root, **{"%s/%s" % (sid, sp): a for sp, a in stored.items()})
    args = train.parse_args(["--model_dir", "m", "--data_root", str(root), "--choice", "chair", "--num_point", str(N)])
    for split, mode in (("test", "shape_bbox"), ("val", "shape_unit"), ("test", None)):
        ds = train.load_split(args, split, mode, tail=N)
        got = ds.stack()
        assert tuple(got.shape) == (stored[split].shape[0], N, 3)
        want = normalize_clouds(torch.from_numpy(stored[split][:, M - N:]), mode)[0]
        by_id = {d["id"]: d["pointcloud"] for d in ds.pointclouds}
        for j in range(want.shape[0]):
            assert torch.equal(by_id[j], want[j]), (split, mode, j)
    # global_unit: the statistics over the three splits' tails (all three cut alike, or the concatenation fails)
    ds = ShapeNetCore("chair", "test", "global_unit", train.open_data_root(str(root)), tail=N)
    every = torch.from_numpy(np.concatenate([stored[sp][:, M - N:] for sp in ("train", "val", "test")]))
    assert torch.equal(ds.stats["std"], every.reshape(-1).std(dim=0))
    # M == N: the whole cloud, as before
    whole = train.load_split(args, "test", "shape_bbox", tail=M).stack()
    assert torch.equal(whole, train.load_split(args, "test", "shape_bbox").stack())
    # training normalises over all M stored points
    full = train.load_split(args, "train", "shape_unit").stack()
    assert tuple(full.shape) == (5, M, 3)


# ---------------------------------------------------------------------------- command line
def test_flag_is_listed_only_where_given():
    from pdgn_amd import train
    a = train.parse_args(["--model_dir", "m"])
    assert a.resample_pool is None and "resample_pool" not in vars(a)
    first_line = str(train.logged_args(a))
    assert "resample" not in first_line
    keys = re.findall(r"(\w+)=", first_line)                                    # the namespace of the time before the flag existed
    assert sorted(keys) == sorted(["phase", "workers", "gpu", "batch_size", "num_point", "num_k", "learning_rate", "max_epoch", "noise_dim",
                           "optimizer", "debug", "data_root", "log_info", "model_dir", "checkpoint_dir", "snapshot", "choice", "network",
                           "savename", "pretrain_model_G", "pretrain_model_D", "softmax", "dataset", "normalize", "seed", "save_dir",
                           "device"])
    b = train.parse_args(["--model_dir", "m", "--resample_pool", "10000"])
    assert b.resample_pool == 10000 and "resample_pool=10000" in str(train.logged_args(b))


def test_parse_args_refuses_a_pool_below_num_point(capsys):
    from pdgn_amd import train
    with pytest.raises(SystemExit):
        train.parse_args(["--model_dir", "m", "--resample_pool", "2047"])
    assert "--resample_pool 2047" in capsys.readouterr().err
    assert train.parse_args(["--model_dir", "m", "--resample_pool", "2048"]).resample_pool == 2048


def test_train_refusals(tmp_path):
    """Raised after the split is read and before anything touches a device."""
    from pdgn_amd import train
    _write_pc15k(tmp_path / "pc", 24)
    common = ["--model_dir", "m", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root", str(tmp_path / "pc"), "--choice", "chair",
              "--batch_size", "2"]
    with pytest.raises(SystemExit, match="--num_point 32 but the clouds of .* have 24 points"):     # fewer points than asked for: as before
        train.train(train.parse_args(common + ["--num_point", "32"]))
    with pytest.raises(SystemExit, match="--resample_pool 32 but the clouds of .* have 24 points"):
        train.train(train.parse_args(common + ["--num_point", "16", "--resample_pool", "32"]))
    _write_pc15k(tmp_path / "exact", 16)
    exact = [a if a != str(tmp_path / "pc") else str(tmp_path / "exact") for a in common]
    with pytest.raises(SystemExit, match="exactly --num_point 16"):
        train.train(train.parse_args(exact + ["--num_point", "16", "--resample_pool", "16"]))


def test_feeder_signature():
    import inspect
    from pdgn_amd.data import BatchFeeder
    params = inspect.signature(BatchFeeder.__init__).parameters
    assert params["num_point"].default is None and params["pool"].default is None
    assert list(params)[:8] == ["self", "clouds", "batch_size", "sizes", "seed", "rank", "world", "sigma"]


# ---------------------------------------------------------------------------- ABI
def test_resample_entry_point_is_declared_exported_and_checks_on_the_host():
    from pdgn_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    assert re.search(r"\bint\s+pdgn_feed_batch_resample\s*\(", header)
    i, ll, ull, vp, f = ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_float
    assert _lib.SIGNATURES["pdgn_feed_batch_resample"] == (i, (i,) * 8 + (vp, vp, ll, ull, ull, ll, f) + (vp,) * 7)
    assert _lib.ABI_VERSION >= 34
    L = ctypes.CDLL(build.build())
    assert hasattr(L, "pdgn_feed_batch_resample")
    ok = vp(4096)                                                # never dereferenced: every call below is refused before any launch

    def call(B=4, S=13, M=48, P=40, N=32, r=(4, 8, 16), first=0, row0=0, ptrs=(ok,) * 8):
        return L.pdgn_feed_batch_resample(B, S, M, P, N, r[0], r[1], r[2], ptrs[0], ptrs[1], ll(first), ull(1), ull(0), ll(row0),
                                          f(0.2), *ptrs[2:], vp(0))

    invalid = -1                                                 # PDGN_ERR_INVALID
    assert call(N=41) == invalid and call(P=49) == invalid       # N > P, P > M
    assert call(M=0x7fffffff // 3 + 1, P=40, N=32) == invalid    # 3 M beyond the int range
    assert call(first=10) == invalid and call(first=-1) == invalid
    assert call(B=0) == invalid and call(N=0) == invalid and call(r=(4, 0, 16)) == invalid and call(B=65536, S=70000) == invalid
    assert call(row0=-1) == invalid and call(row0=(1 << 32) - 3) == invalid
    for k in range(8):                                           # a null pointer, whichever
        assert call(ptrs=tuple(vp(0) if j == k else ok for j in range(8))) == invalid
    assert call(ptrs=(ok,) * 6 + (vp(4104), ok)) == invalid      # z1 not 16-byte aligned
