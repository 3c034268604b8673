"""CPU: the training feed's host side -- the Philox mirror against the published known answers, the epoch permutation, the
(rank, world) schedule, the index draws, the command line, and the exported entry point's host-side argument checks
(PDGNTrainer.fit's control flow on a recording trainer: tests/test_fit_host.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import feed_mirror as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- Philox
def test_philox_known_answers():
    """The three known answers of Philox4x32-10 published with Random123 (kat_vectors)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert tuple(int(v) for v in fm.philox4x32_10(counter, key)) == want
    # vectorised over counters = the scalar results
    c0 = np.array([0, 0xffffffff, 0x243f6a88], dtype=np.uint64)
    many = fm.philox4x32_10((c0, 0, 0, 0), (0, 0))
    assert tuple(int(v) for v in many[0]) == kat[0][2] and many.shape == (3, 4)


def test_product_philox_equals_the_mirror():
    from pdgn_amd import data
    for seed, epoch, S in ((0, 1, 1), (7, 3, 1001), (2 ** 63 + 5, 2 ** 33 + 1, 64), (9999, 300, 4099)):
        assert np.array_equal(data.epoch_order(seed, epoch, S), fm.epoch_order(seed, epoch, S))


# ---------------------------------------------------------------------------- epoch_order / schedule
def test_epoch_order_is_a_pure_permutation():
    from pdgn_amd.data import epoch_order
    S = 4099
    a = epoch_order(9999, 1, S)
    assert a.dtype == np.int32 and a.shape == (S,)
    assert np.array_equal(np.sort(a), np.arange(S))
    assert np.array_equal(a, epoch_order(9999, 1, S))
    assert not np.array_equal(a, epoch_order(9999, 2, S))
    assert not np.array_equal(a, epoch_order(9998, 1, S))
    assert not np.array_equal(a, np.arange(S))


@pytest.mark.parametrize("W", [2, 8])
def test_schedule_ranks_concatenate_to_the_single_rank_batch(W):
    from pdgn_amd.data import batches_per_epoch
    B, N, sizes = 5, 64, (8, 16, 32)
    S = 3 * B * W + 5
    assert batches_per_epoch(S, B, W) == 3 and batches_per_epoch(S, B * W, 1) == 3
    clouds = np.random.default_rng(0).standard_normal((S, N, 3)).astype(np.float32)
    one = fm.MirrorFeeder(clouds, B * W, sizes, seed=41)
    ranks = [fm.MirrorFeeder(clouds, B, sizes, seed=41, rank=r, world=W) for r in range(W)]
    assert one.batches_per_epoch == 3 and all(f.batches_per_epoch == 3 for f in ranks)
    for epoch in (1, 2):
        seen = []
        for i in range(3):
            ids1, idx1, wa1, wb1 = one.draws(epoch, i)
            parts = [f.draws(epoch, i) for f in ranks]
            per_rank = [set(p[0].tolist()) for p in parts]
            for a in range(W):
                for b in range(a + 1, W):
                    assert not (per_rank[a] & per_rank[b])                          # ranks are disjoint
            assert np.array_equal(np.concatenate([p[0] for p in parts]), ids1)      # cloud ids
            for k in range(3):
                assert np.array_equal(np.concatenate([p[1][k] for p in parts]), idx1[k])   # sub-sample indices
            assert np.array_equal(np.concatenate([p[2] for p in parts]), wa1)       # noise words
            assert np.array_equal(np.concatenate([p[3] for p in parts]), wb1)
            assert one.schedule(epoch, i)[2] == ranks[-1].schedule(epoch, i)[2] == (epoch - 1) * 3 + i
            seen += ids1.tolist()
        assert len(seen) == len(set(seen)) == 3 * B * W                             # no cloud twice in an epoch
    # the streams differ from each other and from iteration to iteration
    _, idx_a, wa, wb = one.draws(1, 0)
    _, idx_b, wa2, _ = one.draws(1, 1)
    assert not np.array_equal(wa, wb) and not np.array_equal(wa, wa2) and not np.array_equal(idx_a[0], idx_b[0])
    assert not np.array_equal(idx_a[1][:, :8], idx_a[0])


def test_index_draws_cover_every_point():
    N = 2048
    w = fm.stream_words(9999, 5, np.arange(2048), 2, 2048)                          # 2^22 draws
    idx = fm.indices_from_words(w, N)
    assert idx.min() >= 0 and idx.max() < N
    counts = np.bincount(idx.ravel(), minlength=N)
    assert counts.min() > 0
    # binomial(2^22, 1/2048): mean 2048, sigma 45.2 -- six sigma either way
    assert 2048 - 6 * 45.3 < counts.min() and counts.max() < 2048 + 6 * 45.3, (counts.min(), counts.max())
    for n in (1, 3, 2047, 4096, 100000):
        i = fm.indices_from_words(w[:4], n)
        assert i.min() >= 0 and i.max() < n


def test_normals_formula():
    w = fm.stream_words(3, 0, np.arange(4096), fm.TAG_Z1, 128)
    z = fm.normals_from_words(w, 0.2)
    n = z.size
    assert abs(z.mean()) < 5 * 0.2 / np.sqrt(n) and abs(z.std() - 0.2) < 5 * 0.2 / np.sqrt(2 * n)
    assert np.isfinite(z).all()
    assert np.abs(fm.normals_from_words(w, 0.2, np.float32) - z).max() < 1e-6


# ---------------------------------------------------------------------------- the feeder's own checks
def test_feeder_has_no_cpu_path_and_refuses_transforms():
    from pdgn_amd._lib import PdgnHipError
    from pdgn_amd.data import BatchFeeder
    with pytest.raises(PdgnHipError):
        BatchFeeder(torch.zeros(9, 32, 3), 4, (4, 8, 16), seed=0)

    class WithTransform:
        transform = staticmethod(lambda d: d)

    with pytest.raises(ValueError, match="transform"):
        BatchFeeder(WithTransform(), 4, (4, 8, 16), seed=0)
    with pytest.raises(ValueError, match="transform"):
        BatchFeeder.from_dataset(WithTransform(), "cuda", 4)


# ---------------------------------------------------------------------------- command line
def test_cli_defaults_are_the_references():
    from pdgn_amd import train
    a = train.parse_args(["--model_dir", "m"])
    want = dict(phase="train", workers=4, gpu=0, batch_size=50, num_point=2048, num_k=20, learning_rate=0.0001, max_epoch=300,
                noise_dim=128, optimizer="adam", debug=True, data_root="/opt/data/private/shapenet/shapenet.hdf5",
                log_info="log_info.txt", model_dir="m", checkpoint_dir="checkpoint", snapshot=20, choice=None, savename=None,
                pretrain_model_G=None, pretrain_model_D=None, softmax="True", dataset="shapenet15k", normalize="shape_bbox",
                seed=9999, save_dir="./results", device="cuda")                                    # main.py:15-41
    for k, v in want.items():
        assert getattr(a, k) == v, k
    b = train.parse_args("--phase test --model_dir m --batch_size 35 --choice chair --snapshot 2 --normalize shape_unit "
                         "--pretrain_model_G 2_chair_G.pth --pretrain_model_D 2_chair_D.pth --network PDGNet_v2 --workers 8".split())
    assert (b.phase, b.batch_size, b.choice, b.snapshot, b.normalize) == ("test", 35, "chair", 2, "shape_unit")


def test_cli_refusals(capsys):
    from pdgn_amd import train
    with pytest.raises(SystemExit):
        train.parse_args([])                                                    # no --model_dir
    with pytest.raises(SystemExit):
        train.parse_args(["--model_dir", "m", "--dataset", "modelnet40"])
    assert "shapenet15k" in capsys.readouterr().err


def test_cli_npz_goes_through_shapenetcore(tmp_path):
    from pdgn_amd import train
    from pdgn_amd.data import cate_to_synsetid
    rng = np.random.default_rng(2)
    arrays = {"%s/%s" % (cate_to_synsetid[c], sp): rng.standard_normal((n, 64, 3)).astype(np.float32)
              for c in ("chair", "airplane") for sp, n in (("train", 5), ("val", 2), ("test", 3))}
    path = tmp_path / "toy.npz"
    np.savez(path, **arrays)
    args = train.parse_args(["--model_dir", "m", "--data_root", str(path), "--choice", "chair", "--num_point", "64"])
    ds = train.load_split(args, "train", "shape_unit")
    assert len(ds) == 5 and tuple(ds.stack().shape) == (5, 64, 3) and {d["cate"] for d in ds.pointclouds} == {"chair"}
    args.choice = None                                                          # every category of the file
    ds = train.load_split(args, "test", "shape_bbox")
    assert len(ds) == 6 and {d["cate"] for d in ds.pointclouds} == {"chair", "airplane"}


# ---------------------------------------------------------------------------- ABI
def test_feed_entry_point_is_declared_exported_and_checks_on_the_host():
    from pdgn_amd import build
    header = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    assert re.search(r"\bint\s+pdgn_feed_batch\s*\(", header)
    L = ctypes.CDLL(build.build())
    assert hasattr(L, "pdgn_feed_batch")
    ll, ull, vp = ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_void_p
    ok = vp(4096)                                                # never dereferenced: every call below is refused before any launch

    def call(B=4, S=13, N=32, r=(4, 8, 16), first=0, row0=0, ptrs=(ok,) * 8):
        return L.pdgn_feed_batch(B, S, N, r[0], r[1], r[2], ptrs[0], ptrs[1], ll(first), ull(1), ull(0), ll(row0),
                                 ctypes.c_float(0.2), *ptrs[2:], vp(0))

    invalid = -1                                                 # PDGN_ERR_INVALID
    assert call(first=10) == invalid                             # first + B > S
    assert call(first=-1) == invalid
    assert call(B=0) == invalid and call(N=0) == invalid and call(r=(4, 0, 16)) == invalid
    for k in range(8):                                           # a null pointer, whichever
        assert call(ptrs=tuple(vp(0) if j == k else ok for j in range(8))) == invalid
