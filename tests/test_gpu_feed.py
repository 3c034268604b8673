"""GPU: the batch feeder (csrc/feed.hip through pdgn_amd.data.BatchFeeder) against its host mirror (tests/feed_mirror.py),
PDGNTrainer.fit over it, and the command line's train -> test round trip at toy size."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feed_mirror as fm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 0.2
GUARD = 64                                                       # floats on either side of every output (a multiple of 4: 16-byte alignment kept)
SENTINEL = -12345.0


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _clouds(S, N, seed=0):
    return np.random.default_rng(seed).standard_normal((S, N, 3)).astype(np.float32)


def _guarded(shape, dev):
    """A tensor of `shape` inside a larger sentinel-filled buffer -> (view, whole buffer)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return whole[GUARD:GUARD + n].view(shape), whole


def _guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def _fill(feeder, epoch, i):
    """One feeder.fill into guarded buffers -> ([p1..p4], z1, z2) as numpy; asserts nothing was written outside them."""
    dev = feeder.clouds.device
    made = [_guarded(s, dev) for s in feeder.shapes()[:4]] + [_guarded(feeder.shapes()[4], dev) for _ in range(2)]
    views = [v for v, _ in made]
    feeder.fill(epoch, i, views[:4], views[4], views[5])
    torch.cuda.synchronize()
    for _, whole in made:
        assert _guards_intact(whole)
    out = [v.cpu().numpy() for v in views]
    return out[:4], out[4], out[5]


CONFIGS = [  # B, S, sizes, N, rank, world
    (35, 211, (256, 512, 1024), 2048, 0, 1),
    (35, 211, (512, 1024, 2048), 4096, 0, 1),
    (1, 211, (256, 512, 1024), 2048, 0, 1),
    (35, 211, (256, 512, 1024), 2048, 1, 2),
    (35, 563, (256, 512, 1024), 2048, 7, 8),
    (3, 17, (5, 6, 7), 30, 0, 1),                                # no length a multiple of 4: the element-wise loads and stores
]


@pytest.mark.parametrize("B,S,sizes,N,rank,world", CONFIGS)
def test_clouds_are_bit_equal_to_the_mirror(B, S, sizes, N, rank, world):
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    host = _clouds(S, N)
    feeder = BatchFeeder(torch.from_numpy(host).to(dev), B, sizes, seed=9999, rank=rank, world=world, sigma=SIGMA)
    mirror = fm.MirrorFeeder(host, B, sizes, seed=9999, rank=rank, world=world, sigma=SIGMA)
    assert feeder.batches_per_epoch == mirror.batches_per_epoch >= 1
    for epoch, i in ((1, 0), (1, mirror.batches_per_epoch - 1), (3, 0)):
        reals, z1, z2 = _fill(feeder, epoch, i)
        want, w1, w2 = mirror.batch(epoch, i, np.float64)
        for k in range(4):
            assert reals[k].shape == want[k].shape
            assert np.array_equal(reals[k].view(np.uint32), want[k].view(np.uint32)), (epoch, i, k)
        assert np.abs(z1 - w1).max() < 1e-5 and np.abs(z2 - w2).max() < 1e-5      # (the tight bound: test_noise_*)


def test_noise_against_fp64_and_its_moments():
    """z1, z2 against an fp64 evaluation of the same formula on the same words, over 64 iterations of B = 35 (573,440 normals).
    Bound: 4x the largest deviation of an fp32 numpy evaluation of the formula from the fp64 one ON THESE WORDS (the factor
    is for a different libm).  Measured on an MI355X (ROCm 7.2): device 3.229e-07, numpy fp32 3.229e-07, bound 1.292e-06; z1 mean
    -6.7e-05 / std 0.199862, z2 mean -8.5e-05 / std 0.200120 (5 standard errors: 1.87e-03 / 1.32e-03): profiles/feed_check.txt."""
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    B, S, N, sizes, iters = 35, 35 * 64, 64, (8, 16, 32), 64
    host = _clouds(S, N)
    feeder = BatchFeeder(torch.from_numpy(host).to(dev), B, sizes, seed=2024, sigma=SIGMA)
    mirror = fm.MirrorFeeder(host, B, sizes, seed=2024, sigma=SIGMA)
    assert feeder.batches_per_epoch == iters
    reals, z1, z2 = feeder.buffers()
    got, want, host32 = [], [], []
    for i in range(iters):
        feeder.fill(1, i, reals, z1, z2)
        got.append(torch.stack([z1, z2]).cpu().numpy())
        _, _, w1, w2 = mirror.draws(1, i)
        w = np.stack([w1, w2])
        want.append(fm.normals_from_words(w, SIGMA, np.float64))
        host32.append(fm.normals_from_words(w, SIGMA, np.float32))
    got, want, host32 = np.stack(got), np.stack(want), np.stack(host32)
    assert got.dtype == np.float32 and got.shape == (iters, 2, B, 128)
    host_dev = np.abs(host32.astype(np.float64) - want).max()
    device_dev = np.abs(got.astype(np.float64) - want).max()
    print("feed noise: device max |z - fp64| = %.3e, numpy fp32 = %.3e, bound = %.3e over %d samples" % (device_dev, host_dev, 4 * host_dev, got.size))
    assert device_dev <= 4 * host_dev, (device_dev, host_dev)
    for name, z in (("z1", got[:, 0]), ("z2", got[:, 1])):
        n = z.size
        mean, std = z.astype(np.float64).mean(), z.astype(np.float64).std()
        print("feed noise: %s mean %+.3e (5 s.e. %.3e), std %.6f (sigma %.1f, 5 s.e. %.3e), n = %d"
              % (name, mean, 5 * SIGMA / np.sqrt(n), std, SIGMA, 5 * SIGMA / np.sqrt(2 * n), n))
        assert n == 35 * 128 * 64
        assert abs(mean) <= 5 * SIGMA / np.sqrt(n)
        assert abs(std - SIGMA) <= 5 * SIGMA / np.sqrt(2 * n)


def _raw_feed(clouds, order, B, sizes, first, seed, t, row0):
    """pdgn_feed_batch itself (any t with any `first`)."""
    from pdgn_amd import _lib
    dev = clouds.device
    S, N, _ = clouds.shape
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    p = [new(B, 3, r) for r in tuple(sizes) + (N,)]
    z1, z2 = new(B, 128), new(B, 128)
    ll, ull = ctypes.c_longlong, ctypes.c_ulonglong
    rc = _lib.lib().pdgn_feed_batch(B, S, N, sizes[0], sizes[1], sizes[2], _lib.ptr(clouds), _lib.ptr(order), ll(first), ull(seed),
                                    ull(t), ll(row0), ctypes.c_float(SIGMA), *[_lib.ptr(x) for x in p], _lib.ptr(z1), _lib.ptr(z2),
                                    _lib.stream_of(clouds))
    torch.cuda.synchronize()
    return rc, [x.cpu().numpy() for x in p] + [z1.cpu().numpy(), z2.cpu().numpy()]


def test_feed_is_a_pure_function_of_its_arguments():
    dev = _dev()
    B, S, N, sizes = 35, 211, 2048, (256, 512, 1024)
    clouds = torch.from_numpy(_clouds(S, N)).to(dev)
    order = torch.from_numpy(fm.epoch_order(5, 1, S)).to(dev)
    args = dict(B=B, sizes=sizes, first=70, seed=5, row0=0)
    rc, a = _raw_feed(clouds, order, t=11, **args)
    assert rc == 0
    _, b = _raw_feed(clouds, order, t=11, **args)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))                # launched twice: bit-equal
    _, c = _raw_feed(clouds, order, t=12, **args)
    for k in (0, 1, 2, 4, 5):                                                   # t + 1: every row of p1 p2 p3 z1 z2 changes
        differs = (a[k].reshape(B, -1) != c[k].reshape(B, -1)).any(axis=1)
        assert differs.all(), k
    assert np.array_equal(a[3].view(np.uint32), c[3].view(np.uint32))              # p4 does not depend on t
    _, d = _raw_feed(clouds, order, t=11 + (1 << 32), **args)                   # the high part of t is part of the counter
    assert (a[4] != d[4]).any(axis=1).all() and (a[0].reshape(B, -1) != d[0].reshape(B, -1)).any(axis=1).all()
    # the host-side refusals, with real pointers
    assert _raw_feed(clouds, order, B=B, sizes=sizes, first=S - B + 1, seed=5, t=0, row0=0)[0] == -1
    assert _raw_feed(clouds, order, B=B, sizes=(256, 0, 1024), first=0, seed=5, t=0, row0=0)[0] == -1


# ---------------------------------------------------------------------------- fit
class RecordingFeeder:
    """A BatchFeeder whose every fill is followed by a copy of what it wrote (stream-ordered clones)."""

    def __init__(self, feeder):
        self.inner, self.fed = feeder, []
        self.batches_per_epoch, self.rank = feeder.batches_per_epoch, feeder.rank

    def buffers(self):
        return self.inner.buffers()

    def fill(self, epoch, i, reals, z1, z2):
        self.inner.fill(epoch, i, reals, z1, z2)
        self.fed.append((epoch, i, [r.clone() for r in reals], z1.clone(), z2.clone(), [r.data_ptr() for r in reals] + [z1.data_ptr(), z2.data_ptr()]))


def _equal_feeds(fed, mirror):
    for epoch, i, reals, z1, z2, _ in fed:
        want, w1, w2 = mirror.batch(epoch, i, np.float64)
        for k in range(4):
            assert np.array_equal(reals[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)), (epoch, i, k)
        assert np.abs(z1.cpu().numpy() - w1).max() < 1e-5 and np.abs(z2.cpu().numpy() - w2).max() < 1e-5, (epoch, i)


def _state_tensors(tr):
    ts = []
    for net in [tr.G] + tr.D:
        ts += list(net.parameters()) + list(net.buffers())
    for opt in [tr.optG] + tr.optD:
        for st in opt.state.values():
            ts += [v for v in st.values() if torch.is_tensor(v)]
    return ts


def test_fit_feeds_the_launch_list():
    from pdgn_amd.data import BatchFeeder
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    dev = _dev()
    B, N, sizes = 4, 2048, (256, 512, 1024)
    S = 3 * B + 1
    host = _clouds(S, N, seed=3)
    clouds = torch.from_numpy(host).to(dev)
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    tr.capture_list(synthetic_batch(B, dev), noise(B, dev), noise(B, dev))
    static = [r.data_ptr() for r in tr._static["reals"]] + [tr._static["z1"].data_ptr(), tr._static["z2"].data_ptr()]
    feeder = RecordingFeeder(BatchFeeder(clouds, B, sizes, seed=77))
    mirror = fm.MirrorFeeder(host, B, sizes, seed=77)
    lines = []
    assert tr.fit(feeder, 2, log=lines.append) == 2
    torch.cuda.synchronize()
    assert len(feeder.fed) == len(lines) == 2 * 3
    assert [(e, i) for e, i, *_ in feeder.fed] == [(e, i) for e in (1, 2) for i in range(3)]
    assert all(f[5] == static for f in feeder.fed)                              # written straight into the list's static buffers
    _equal_feeds(feeder.fed, mirror)
    for line in lines:
        vals = [float(tok.rstrip(",")) for tok in line.split("time:")[1].split()[2:][1::2]]
        assert len(vals) == 6 and all(np.isfinite(v) for v in vals), line

    # list versus eager on a fed batch, from identical state (the pattern and the bound of tests/test_gpu_schedule.py:170-192:
    # 2e-3 * max(1, |eager|), line 190).  Both sides must see the SAME bits: the eager step runs on the batch as the feeder
    # writes it into buffers of its own -- checked against the mirror right here, clouds bit for bit, noise within the noise test's bound --
    # and not on the mirror's numpy-evaluated noise.  Measured: at B = 4 the BatchNorms' batch statistics turn the one-ulp
    # difference between the two libms' normals (6e-8) into 5.7e-3 of g_loss, for the eager step and the list alike, while
    # on equal bits list and eager agree to 8e-6 (eager 1.94857490, list 1.94858956; on the mirror's bits both 1.937561).
    one = BatchFeeder(clouds[:B + 1].contiguous(), B, sizes, seed=78)           # one batch per epoch: fit(one, 1) is ONE iteration
    want, w1, w2 = fm.MirrorFeeder(host[:B + 1], B, sizes, seed=78).batch(1, 0, np.float64)
    fed_reals, fed_z1, fed_z2 = one.buffers()
    one.fill(1, 0, fed_reals, fed_z1, fed_z2)
    for got, ref in zip(fed_reals, want):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    _, h1, h2 = fm.MirrorFeeder(host[:B + 1], B, sizes, seed=78).batch(1, 0, np.float32)
    for got, ref, h in ((fed_z1, w1, h1), (fed_z2, w2, h2)):                    # (test_noise_*'s bound, on these words)
        assert np.abs(got.cpu().numpy() - ref).max() <= 4 * np.abs(h - ref).max()
    ts = _state_tensors(tr)
    snap = [t.detach().clone() for t in ts]
    eager = {k: v.item() for k, v in tr.step(fed_reals, fed_z1, fed_z2).items()}
    with torch.no_grad():
        for t, v in zip(ts, snap):
            t.copy_(v)
    assert tr.fit(one, 1) == 1
    listed = {k: v.item() for k, v in tr._static["out"].items()}
    torch.cuda.synchronize()
    assert set(listed) == set(eager) and len(eager) == 6
    for k in eager:
        assert abs(listed[k] - eager[k]) <= 2e-3 * max(1.0, abs(eager[k])), (k, listed[k], eager[k])
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def test_resumed_epoch_is_fed_what_an_uninterrupted_run_is_fed(tmp_path):
    """Feeds only: trajectories are not bit-reproducible and nothing here claims they are."""
    from pdgn_amd.data import BatchFeeder
    from pdgn_amd.trainer import PDGNTrainer
    dev = _dev()
    B, N, sizes = 4, 2048, (256, 512, 1024)
    S = 2 * B + 1
    host = _clouds(S, N, seed=4)
    clouds = torch.from_numpy(host).to(dev)
    new_feeder = lambda: RecordingFeeder(BatchFeeder(clouds, B, sizes, seed=31))

    def new_trainer():
        torch.manual_seed(0)
        tr = PDGNTrainer(device=dev, distributed=False)
        tr.train()
        return tr

    whole = new_feeder()
    assert new_trainer().fit(whole, 2, issue="eager") == 2                      # the uninterrupted run: epochs 1, 2
    first = new_feeder()
    assert new_trainer().fit(first, 1, checkpoint_dir=str(tmp_path), category="chair", issue="eager") == 1
    g, d = str(tmp_path / "1_chair_G.pth"), str(tmp_path / "1_chair_D.pth")
    assert os.path.exists(g) and os.path.exists(d)
    tr = new_trainer()
    start = tr.load(g, d)
    assert start == 1                                                           # the reference resumes AT the stored epoch (:158-160)
    resumed = new_feeder()
    assert tr.fit(resumed, 2, start_epoch=start, issue="eager") == 2
    torch.cuda.synchronize()
    assert [(e, i) for e, i, *_ in resumed.fed] == [(e, i) for e, i, *_ in whole.fed] == [(1, 0), (1, 1), (2, 0), (2, 1)]
    for a, b in zip(resumed.fed, whole.fed):
        for x, y in zip(a[2] + [a[3], a[4]], b[2] + [b[3], b[4]]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    _equal_feeds(resumed.fed[:2], fm.MirrorFeeder(host, B, sizes, seed=31))


def test_cli_train_then_test_round_trip(tmp_path):
    from pdgn_amd.data import cate_to_synsetid
    rng = np.random.default_rng(5)
    sid = cate_to_synsetid["chair"]
    n_test = 6
    np.savez(tmp_path / "toy.npz", **{"%s/%s" % (sid, sp): rng.standard_normal((n, 2048, 3)).astype(np.float32)
                                      for sp, n in (("train", 9), ("val", 2), ("test", n_test))})
    common = [sys.executable, "-m", "pdgn_amd.train", "--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root",
              str(tmp_path / "toy.npz"), "--choice", "chair", "--batch_size", "4", "--seed", "1", "--save_dir", str(tmp_path / "res")]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run(common + ["--phase", "train", "--max_epoch", "1", "--snapshot", "1"], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    ck = tmp_path / "ck" / "toy" / "PDGNet_v2"
    g, d = torch.load(ck / "1_chair_G.pth", map_location="cpu"), torch.load(ck / "1_chair_D.pth", map_location="cpu")
    assert set(g) == {"G_model", "G_optimizer", "G_epoch"} and g["G_epoch"] == 1
    assert set(d) == {"D_epoch"} | {"D_model%d" % i for i in range(1, 5)} | {"D_optimizer%d" % i for i in range(1, 5)}
    log = (tmp_path / "ck" / "toy" / "log_info.txt").read_text().splitlines()
    assert sum(l.startswith("Epoch: [ 1]") for l in log) == 2                    # 9 clouds, batches of 4
    run = subprocess.run(common + ["--phase", "test", "--pretrain_model_G", "1_chair_G.pth", "--pretrain_model_D", "1_chair_D.pth"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    outs = list((tmp_path / "res").iterdir())
    assert len(outs) == 1 and outs[0].name.startswith("GEN_Ours_chair_")
    assert np.load(outs[0] / "out.npy").shape == (n_test, 2048, 3) == np.load(outs[0] / "nonormal_out.npy").shape
    metrics = dict(l.split(": ") for l in (outs[0] / "log.txt").read_text().splitlines())
    assert "jsd" in metrics and "1-NN-CD-acc" in metrics and "lgan_mmd-CD" in metrics and len(metrics) >= 10
    assert all(np.isfinite(float(v)) for v in metrics.values()), metrics
