"""CPU: the training feed's host side -- the Philox mirror against the published known answers, the epoch permutation, the
(rank, world) schedule, the index draws, PDGNTrainer.fit's control flow on a recording trainer, the command line, and the
exported entry point's host-side argument checks."""
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


# ---------------------------------------------------------------------------- fit
class RecordingTrainer:
    """What PDGNTrainer.fit touches, recorded."""
    device = torch.device("cpu")

    def __init__(self, B, sizes, loaded_epoch=None):
        from pdgn_amd.trainer import PDGNTrainer
        self.LOG_FORMAT, self.LOSS_KEYS = PDGNTrainer.LOG_FORMAT, PDGNTrainer.LOSS_KEYS
        self.calls, self.saves, self.fed = [], [], []
        self.B, self.sizes = B, sizes
        self._list, self._static = None, None

    def capture_list(self, reals, z1, z2):
        self.calls.append(("capture_list",))
        self._static = {"reals": [r.clone() for r in reals], "z1": z1.clone(), "z2": z2.clone()}
        self._list = object()
        return self

    def _losses(self, z1):
        self.fed.append(z1.clone())
        return {k: torch.tensor(float(len(self.fed)) + 0.125 * j) for j, k in enumerate(self.LOSS_KEYS)}

    def step_list(self, *args, **kw):
        self.calls.append(("step_list", args, kw))
        return self._losses(self._static["z1"])

    def step(self, reals, z1, z2):
        self.calls.append(("step", len(reals)))
        return self._losses(z1)

    def save(self, checkpoint_dir, epoch, category="chair"):
        self.saves.append((checkpoint_dir, epoch, category))


class HostFeeder(fm.MirrorFeeder):
    def buffers(self):
        new = lambda *s: torch.empty(*s, dtype=torch.float32)
        return [new(self.B, 3, r) for r in self.sizes + (self.N,)], new(self.B, 128), new(self.B, 128)


REF_LINE = re.compile(r"^Epoch: \[ *(\d+)\] \[ *(\d+)/ *(\d+)\] time: +\d+m +\d+s d_loss1: (-?\d+\.\d{8}) d_loss2: (-?\d+\.\d{8}) "
                      r"d_loss3: (-?\d+\.\d{8}) d_loss4: (-?\d+\.\d{8}), g_loss: (-?\d+\.\d{8}), similar_loss: (-?\d+\.\d{8})$")


def _fit(**kw):
    from pdgn_amd.trainer import PDGNTrainer
    B, N, sizes = 4, 32, (4, 8, 16)
    S = 3 * B + 1
    clouds = np.random.default_rng(1).standard_normal((S, N, 3)).astype(np.float32)
    feeder = HostFeeder(clouds, B, sizes, seed=17)
    tr = RecordingTrainer(B, sizes)
    lines = []
    last = PDGNTrainer.fit(tr, feeder, log=lines.append, **kw)
    return tr, feeder, lines, last


def test_fit_list_steps_snapshots_and_log():
    from pdgn_amd.trainer import PDGNTrainer
    assert PDGNTrainer.LOG_FORMAT == ("Epoch: [%2d] [%4d/%4d] time: %2dm %2ds d_loss1: %.8f d_loss2: %.8f d_loss3: %.8f "
                                      "d_loss4: %.8f, g_loss: %.8f, similar_loss: %.8f")        # models/PDGNet_v2.py:259
    tr, feeder, lines, last = _fit(epochs=5, snapshot=2, checkpoint_dir="ck", category="chair")
    assert last == 5
    steps = [c for c in tr.calls if c[0] == "step_list"]
    assert len(steps) == 5 * 3 and not any(c[0] == "step" for c in tr.calls)
    assert all(c[1] == () and c[2] == {} for c in steps)                       # step_list() without tensors
    assert tr.calls[0] == ("capture_list",) and sum(c[0] == "capture_list" for c in tr.calls) == 1
    assert tr.saves == [("ck", 2, "chair"), ("ck", 4, "chair"), ("ck", 5, "chair")]   # snapshots + the final save
    assert len(lines) == 15
    for n, line in enumerate(lines):
        m = REF_LINE.match(line)
        assert m, line
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (n // 3 + 1, n % 3 + 1, 3)
        assert float(m.group(4)) == n + 1 and float(m.group(9)) == n + 1 + 0.625       # iteration n's own losses, in order
    # what the step read is the mirror's batch of that iteration
    for n, z in enumerate(tr.fed):
        assert np.array_equal(z.numpy(), feeder.batch(n // 3 + 1, n % 3)[1].astype(np.float32))


def test_fit_resume_starts_at_the_loaded_epoch():
    tr, feeder, lines, last = _fit(epochs=4, start_epoch=3, snapshot=20, checkpoint_dir="ck")
    assert last == 4 and len(lines) == 2 * 3
    assert [int(REF_LINE.match(l).group(1)) for l in lines] == [3, 3, 3, 4, 4, 4]
    assert tr.saves == [("ck", 4, "chair")]
    assert np.array_equal(tr.fed[0].numpy(), feeder.batch(3, 0)[1].astype(np.float32))
    # no checkpoint directory: nothing is saved; on_epoch sees every epoch
    seen = []
    tr, _, _, _ = _fit(epochs=2, snapshot=1, on_epoch=seen.append)
    assert tr.saves == [] and seen == [1, 2]


def test_fit_eager_and_log_to_a_path(tmp_path):
    from pdgn_amd.trainer import PDGNTrainer
    tr, feeder, lines, last = _fit(epochs=1, issue="eager")
    assert [c[0] for c in tr.calls] == ["step"] * 3 and len(lines) == 3
    path = tmp_path / "log_info.txt"
    tr = RecordingTrainer(4, (4, 8, 16))
    PDGNTrainer.fit(tr, feeder, 2, log=str(path))
    got = path.read_text().splitlines()
    assert len(got) == 6 and all(REF_LINE.match(l) for l in got)
    with pytest.raises(ValueError):
        PDGNTrainer.fit(tr, feeder, 1, issue="graph")


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
