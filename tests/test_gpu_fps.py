"""GPU: the register-resident farthest-point kernel (csrc/fps.hip) -- pdgn_fps_order through pointops.fps_order against the host
mirror (tests/fps_mirror.py) on lattice clouds and against pdgn_furthestsampling on Gaussian ones; pdgn_feed_fps_pyramid through
BatchFeeder(subsample="fps"); PDGNTrainer.fit over that feeder and the command line's --subsample fps.  Index and feeder outputs sit
inside sentinel-filled guard bands."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feed_mirror as fm
import fps_mirror as fpm
import resample_mirror as rm
from hashweights import lattice_points

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 0.2
GUARD = 64
SENTINEL = -12345.0
INVALID = -1


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lattice(key, shape):
    """Multiples of 2^-6 in [-1, 1): every squared distance is exact in fp32 and ties are plentiful."""
    return lattice_points(key, shape, bits=6)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(shape, dev, dtype=torch.float32):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    return whole[GUARD:GUARD + n].view(shape), whole


def _guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def _raw_order(xyz, m, start=None, b=None, n=None):
    """pdgn_fps_order itself into a guarded index buffer -> (rc, order as numpy, whether anything at all was written)."""
    from pdgn_amd import _lib
    b = xyz.shape[0] if b is None else b
    n = xyz.shape[1] if n is None else n
    view, whole = _guarded((max(b, 1), max(m, 1)), xyz.device, torch.int32)
    rc = _lib.lib().pdgn_fps_order(b, n, m, _lib.ptr(xyz), _lib.ptr(start), _lib.ptr(view), _lib.stream_of(xyz))
    torch.cuda.synchronize()
    assert _guards_intact(whole)
    return rc, view.cpu().numpy(), not bool((whole == SENTINEL).all())


# ---------------------------------------------------------------------------- pdgn_fps_order against the mirror
# the smallest shapes that cross each boundary of the kernel: a partial wave, a wave edge, the workgroup's 512 threads, every step
# of the points per thread (512 x 1 2 4 8 16), the upper limit
SHAPES = [(1, 1, 1), (63, 63, 1), (64, 17, 1), (65, 65, 3), (1000, 256, 2), (1024, 512, 2), (1025, 512, 2), (2048, 1024, 3),
          (2049, 64, 1), (8192, 32, 1),
          (512, 40, 2), (513, 40, 2), (4096, 24, 1), (4097, 24, 1)]


@pytest.mark.parametrize("n,m,b", SHAPES, ids=["n%d-m%d-b%d" % s for s in SHAPES])
def test_order_equals_the_mirror_on_lattice_clouds(n, m, b):
    from pdgn_amd import pointops
    host = _lattice("fps.gpu.%d" % n, (b, n, 3))
    got = pointops.fps_order(torch.from_numpy(host).to(_dev()), m)
    assert got.dtype == torch.int32 and tuple(got.shape) == (b, m)
    np.testing.assert_array_equal(got.cpu().numpy(), fpm.fps_order_batch(host, m))
    rc, raw, _ = _raw_order(torch.from_numpy(host).to(_dev()), m)               # the entry point itself, inside a guard band
    assert rc == 0
    np.testing.assert_array_equal(raw, fpm.fps_order_batch(host, m))


def test_duplicated_and_exhausted_clouds():
    from pdgn_amd import pointops
    dev = _dev()
    half = _lattice("fps.gpu.dup", (2, 300, 3))
    dup = np.concatenate([half, half], axis=1)                                   # every point twice: index i and i + 300
    got = pointops.fps_order(torch.from_numpy(dup).to(dev), 400).cpu().numpy()
    np.testing.assert_array_equal(got, fpm.fps_order_batch(dup, 400))
    for row, cloud in zip(got, half):
        distinct = len({tuple(p) for p in cloud.tolist()})
        assert row[:distinct].max() < 300 and len(set(row[:distinct].tolist())) == distinct       # the first copy, each once
        assert (row[distinct:] == 0).all()                                                        # used up: the lowest index repeats
    # m = n on 200 points of which 50 are distinct
    base = _lattice("fps.gpu.exh", (50, 3))
    assert len({tuple(p) for p in base.tolist()}) == 50
    cloud = base[np.arange(200) % 50][None]
    got = pointops.fps_order(torch.from_numpy(np.ascontiguousarray(cloud)).to(dev), 200).cpu().numpy()
    np.testing.assert_array_equal(got, fpm.fps_order_batch(cloud, 200))
    assert len(set(got[0, :50].tolist())) == 50 and got[0, :50].max() < 50 and (got[0, 50:] == 0).all()
    # all points equal
    same = torch.full((1, 130, 3), 0.25, device=dev)
    assert pointops.fps_order(same, 130, start=77).cpu().tolist() == [[77] + [0] * 129]


@pytest.mark.parametrize("n,m", [(65, 65), (1025, 96), (2048, 64)])
def test_start_indices_per_row(n, m):
    from pdgn_amd import pointops
    dev = _dev()
    host = _lattice("fps.gpu.start.%d" % n, (4, n, 3))
    xyz = torch.from_numpy(host).to(dev)
    start = [n - 1, 0, n // 2, 1]
    want = fpm.fps_order_batch(host, m, start)
    for s in (torch.tensor(start, device=dev), torch.tensor(start, dtype=torch.int32), torch.tensor(start, dtype=torch.int64, device=dev)):
        np.testing.assert_array_equal(pointops.fps_order(xyz, m, s).cpu().numpy(), want)
    np.testing.assert_array_equal(pointops.fps_order(xyz, m, n - 1).cpu().numpy(), fpm.fps_order_batch(host, m, n - 1))
    np.testing.assert_array_equal(pointops.fps_order(xyz, m, None).cpu().numpy(), fpm.fps_order_batch(host, m))


# ---------------------------------------------------------------------------- against pdgn_furthestsampling
@pytest.mark.parametrize("b,n,m", [(3, 2048, 1024), (2, 777, 300)])
def test_order_equals_furthestsampling_on_gaussian_clouds(b, n, m):
    """The same arithmetic and the same tie rule: any difference is a bug of the new kernel."""
    from pdgn_amd import pointops
    xyz = torch.from_numpy(np.random.default_rng(n).standard_normal((b, n, 3)).astype(np.float32)).to(_dev())
    old = pointops.furthestsampling(xyz, m)
    new = pointops.fps_order(xyz, m)
    assert torch.equal(old, new)
    assert all(len(set(row)) == m for row in new.cpu().tolist())


# ---------------------------------------------------------------------------- refusals
def test_invalid_arguments_are_refused_before_any_launch():
    from pdgn_amd import _lib, pointops
    dev = _dev()
    xyz = torch.from_numpy(_lattice("fps.gpu.bad", (2, 100, 3))).to(dev)
    big = torch.zeros(1, 8193, 3, device=dev)
    assert _raw_order(xyz, 10)[0] == 0
    for kw in (dict(xyz=big, m=4), dict(xyz=xyz, m=101), dict(xyz=xyz, m=0), dict(xyz=xyz, m=-1), dict(xyz=xyz, m=4, n=0), dict(xyz=xyz, m=4, b=-1)):
        rc, _, touched = _raw_order(**kw)
        assert rc == INVALID and not touched, {k: v for k, v in kw.items() if k != "xyz"}
    rc, _, touched = _raw_order(xyz, 4, b=0)                                     # b = 0: nothing to do, no launch
    assert rc == 0 and not touched
    assert _lib.lib().pdgn_fps_order(2, 100, 4, None, None, None, _lib.stream_of(xyz)) == INVALID
    assert tuple(pointops.fps_order(torch.zeros(0, 100, 3, device=dev), 5).shape) == (0, 5)
    # the wrapper: the same ranges, and `start` on the host -- the kernel is never handed one outside [0, n)
    for bad in (dict(xyz=big, m=4), dict(xyz=xyz, m=101), dict(xyz=xyz, m=0)):
        with pytest.raises(ValueError):
            pointops.fps_order(**bad)
    for start in (100, -1, torch.tensor([0, 100], device=dev), torch.tensor([-1, 0], device=dev), torch.tensor([0, 1, 2], device=dev),
                  torch.tensor([0.0, 1.0], device=dev)):
        with pytest.raises(ValueError):
            pointops.fps_order(xyz, 4, start)
    # the pyramid's entry point
    B, N = 2, 64
    p4 = torch.zeros(B, 3, N, device=dev)
    made = [_guarded((B, 3, r), dev) for r in (8, 16, 32)]
    ok = dict(B=B, N=N, r1=8, r2=16, r3=32, p4=_lib.ptr(p4), seed=1, t=0, row0=0, p1=_lib.ptr(made[0][0]), p2=_lib.ptr(made[1][0]),
              p3=_lib.ptr(made[2][0]), order=None, stream=_lib.stream_of(p4))
    call = lambda **kw: _lib.lib().pdgn_feed_fps_pyramid(*dict(ok, **kw).values())     # (a dict keeps its keys' order: the prototype's)
    for bad in (dict(B=0), dict(N=8193), dict(r1=0), dict(r1=17), dict(r2=33), dict(r3=65), dict(row0=-1), dict(row0=(1 << 32) - B + 1), dict(p4=None),
                dict(p2=None)):
        assert call(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert all(bool((whole == SENTINEL).all()) for _, whole in made)
    assert call() == 0
    torch.cuda.synchronize()
    assert all(_guards_intact(whole) for _, whole in made)


# ---------------------------------------------------------------------------- the feeder
S, N, SIZES, B = 12, 128, (16, 32, 64), 4


def _split(M=N):
    host = _lattice("fps.gpu.feed", (S, M, 3))
    for cloud in host:
        assert len({tuple(p) for p in cloud.tolist()}) == M                     # the fixture's clouds have distinct points
    return host


def _fill(feeder, epoch, i):
    """One feeder.fill into guarded buffers -> ([p1..p4], z1, z2) as torch tensors on the host."""
    dev = feeder.clouds.device
    made = [_guarded(s, dev) for s in feeder.shapes()[:4]] + [_guarded(feeder.shapes()[4], dev) for _ in range(2)]
    views = [v for v, _ in made]
    feeder.fill(epoch, i, views[:4], views[4], views[5])
    torch.cuda.synchronize()
    for _, whole in made:
        assert _guards_intact(whole)
    out = [v.cpu() for v in views]
    return out[:4], out[4], out[5]


def _structure(reals, sizes):
    """p1 is a prefix of p2, p2 of p3; every column of p3 is a column of p4 and none repeats."""
    p1, p2, p3, p4 = [r.numpy() for r in reals]
    assert np.array_equal(_bits(p1), _bits(p2[:, :, :sizes[0]])) and np.array_equal(_bits(p2), _bits(p3[:, :, :sizes[1]]))
    for b in range(p4.shape[0]):
        cols4 = {tuple(c) for c in _bits(p4[b]).T.tolist()}
        cols3 = [tuple(c) for c in _bits(p3[b]).T.tolist()]
        assert set(cols3) <= cols4 and len(set(cols3)) == sizes[2], b


def test_fps_feeder_against_the_random_feeder_and_the_mirror():
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    host = _split()
    clouds = torch.from_numpy(host).to(dev)
    fps = BatchFeeder(clouds, B, SIZES, seed=9999, sigma=SIGMA, subsample="fps")
    rnd = BatchFeeder(clouds, B, SIZES, seed=9999, sigma=SIGMA, subsample="random")
    mirror = fpm.MirrorFpsFeeder(fm.MirrorFeeder(host, B, SIZES, seed=9999, sigma=SIGMA))
    assert fps.subsample == "fps" and fps._fn.__name__ == "pdgn_feed_batch" and fps._fps.__name__ == "pdgn_feed_fps_pyramid"
    assert fps.shapes() == rnd.shapes() and fps.batches_per_epoch == mirror.batches_per_epoch == 3
    starts = {}
    for epoch, i in ((1, 0), (1, 1), (1, 2), (2, 0)):
        reals, z1, z2 = _fill(fps, epoch, i)
        other, o1, o2 = _fill(rnd, epoch, i)
        assert torch.equal(reals[3], other[3]) and torch.equal(z1, o1) and torch.equal(z2, o2)     # p4, z1, z2: the random feeder's
        want, _, _ = mirror.batch(epoch, i)
        for k in range(4):
            assert np.array_equal(_bits(reals[k].numpy()), _bits(want[k])), (epoch, i, k)
        _structure(reals, SIZES)
        again, a1, a2 = _fill(fps, epoch, i)                                                       # the same (epoch, i) twice
        assert all(torch.equal(x, y) for x, y in zip(reals + [z1, z2], again + [a1, a2]))
        _, rows, t = mirror.schedule(epoch, i)
        starts[(epoch, i)] = fpm.start_indices(9999, t, rows, N)
        p4 = reals[3].numpy()
        for b in range(B):                                                                         # column 0 is the mirror's Philox start
            assert np.array_equal(_bits(reals[2].numpy()[b, :, 0]), _bits(p4[b, :, starts[(epoch, i)][b]]))
    assert (starts[(1, 0)] != starts[(1, 1)]).any() and (starts[(1, 1)] != starts[(1, 2)]).any()   # the next iteration starts elsewhere


def test_fps_feeder_ranks_compose():
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    clouds = torch.from_numpy(_split()).to(dev)
    one = BatchFeeder(clouds, 4, SIZES, seed=7, sigma=SIGMA, subsample="fps")
    ranks = [BatchFeeder(clouds, 2, SIZES, seed=7, rank=r, world=2, sigma=SIGMA, subsample="fps") for r in range(2)]
    assert one.batches_per_epoch == ranks[0].batches_per_epoch == 3
    for epoch, i in ((1, 2), (2, 1)):
        whole = _fill(one, epoch, i)
        parts = [_fill(f, epoch, i) for f in ranks]
        for k in range(4):
            assert torch.equal(torch.cat([p[0][k] for p in parts]), whole[0][k]), (epoch, i, k)
        for k in (1, 2):
            assert torch.equal(torch.cat([p[k] for p in parts]), whole[k])


def test_fps_feeder_on_dense_clouds():
    """M = 300 stored points, a fresh 128 of the leading 200 per visit (pdgn_feed_batch_resample), then the pyramid of THAT draw."""
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    M, P = 300, 200
    host = _split(M)
    clouds = torch.from_numpy(host).to(dev)
    fps = BatchFeeder(clouds, B, SIZES, seed=31, sigma=SIGMA, num_point=N, pool=P, subsample="fps")
    rnd = BatchFeeder(clouds, B, SIZES, seed=31, sigma=SIGMA, num_point=N, pool=P)
    mirror = fpm.MirrorFpsFeeder(rm.MirrorResampleFeeder(host, B, SIZES, seed=31, sigma=SIGMA, num_point=N, pool=P))
    assert fps._fn.__name__ == "pdgn_feed_batch_resample"
    for epoch, i in ((1, 0), (2, 2)):
        reals, z1, z2 = _fill(fps, epoch, i)
        other, o1, o2 = _fill(rnd, epoch, i)
        assert torch.equal(reals[3], other[3]) and torch.equal(z1, o1) and torch.equal(z2, o2)
        want, _, _ = mirror.batch(epoch, i)
        for k in range(4):
            assert np.array_equal(_bits(reals[k].numpy()), _bits(want[k])), (epoch, i, k)
        _structure(reals, SIZES)


def test_random_is_the_feeder_without_the_argument():
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    host = _split(300)
    clouds = torch.from_numpy(host).to(dev)
    for kw in ({"num_point": 300}, {"num_point": N, "pool": 200}):
        plain = BatchFeeder(clouds, B, SIZES, seed=3, sigma=SIGMA, **kw)
        named = BatchFeeder(clouds, B, SIZES, seed=3, sigma=SIGMA, subsample="random", **kw)
        assert plain.subsample == named.subsample == "random" and plain._fps is None and named._fps is None
        assert plain._fn.__name__ == named._fn.__name__
        for epoch, i in ((1, 0), (3, 1)):
            a, b = _fill(plain, epoch, i), _fill(named, epoch, i)
            assert all(torch.equal(x, y) for x, y in zip(a[0] + [a[1], a[2]], b[0] + [b[1], b[2]]))
    # "random" takes what it always took: sizes in any order, above N, clouds above the farthest-point kernel's limit
    BatchFeeder(clouds, B, (64, 32, 16), seed=3, subsample="random")
    BatchFeeder(clouds, B, (16, 32, 400), seed=3)
    BatchFeeder(torch.zeros(2, 8193, 3, device=dev), 1, SIZES, seed=3)


def test_feeder_refusals():
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    clouds = torch.from_numpy(_split()).to(dev)
    BatchFeeder(clouds, B, (16, 16, 128), seed=3, subsample="fps")               # equal sizes and r3 = N are fine
    for bad in (dict(sizes=(32, 16, 64)), dict(sizes=(16, 64, 32)), dict(sizes=(16, 32, 129)), dict(sizes=(16, 32, 64), num_point=48),
                dict(sizes=SIZES, subsample="grid"), dict(sizes=SIZES, subsample=None)):
        with pytest.raises(ValueError):
            BatchFeeder(clouds, B, seed=3, **dict(dict(subsample="fps"), **bad))
    with pytest.raises(ValueError, match="8192"):
        BatchFeeder(torch.zeros(2, 8193, 3, device=dev), 1, SIZES, seed=3, subsample="fps")
    BatchFeeder(torch.zeros(2, 8193, 3, device=dev), 1, SIZES, seed=3, num_point=8192, subsample="fps")   # N counts, not the stored M


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
        self.fed.append((epoch, i, [r.clone() for r in reals], z1.clone(), z2.clone()))


FIT = dict(B=4, N=2048, sizes=(256, 512, 1024))                               # the trainer shape of tests/test_gpu_feed.py's fit tests


def test_fit_two_epochs_and_a_resumed_epoch_is_fed_what_an_uninterrupted_run_is_fed(tmp_path):
    """Feeds only, as in tests/test_gpu_resample.py: trajectories are not bit-reproducible and nothing here claims they are."""
    from pdgn_amd import pointops
    from pdgn_amd.data import BatchFeeder
    from pdgn_amd.trainer import PDGNTrainer
    dev = _dev()
    Bf, Nf, sizes = FIT["B"], FIT["N"], FIT["sizes"]
    Sf = 2 * Bf + 1
    host = np.random.default_rng(4).standard_normal((Sf, Nf, 3)).astype(np.float32)
    clouds = torch.from_numpy(host).to(dev)
    new_feeder = lambda: RecordingFeeder(BatchFeeder(clouds, Bf, sizes, seed=31, subsample="fps"))

    def new_trainer():
        torch.manual_seed(0)
        tr = PDGNTrainer(device=dev, distributed=False)
        tr.train()
        return tr

    whole, lines = new_feeder(), []
    assert new_trainer().fit(whole, 2, issue="eager", log=lines.append) == 2     # the uninterrupted run: epochs 1, 2
    assert len(lines) == 4
    for line in lines:
        vals = [float(tok.rstrip(",")) for tok in line.split("time:")[1].split()[2:][1::2]]
        assert len(vals) == 6 and all(np.isfinite(v) for v in vals), line
    first = new_feeder()
    assert new_trainer().fit(first, 1, checkpoint_dir=str(tmp_path), category="chair", issue="eager") == 1
    tr = new_trainer()
    start = tr.load(str(tmp_path / "1_chair_G.pth"), str(tmp_path / "1_chair_D.pth"))
    assert start == 1
    resumed = new_feeder()
    assert tr.fit(resumed, 2, start_epoch=start, issue="eager") == 2
    torch.cuda.synchronize()
    assert [(e, i) for e, i, *_ in resumed.fed] == [(e, i) for e, i, *_ in whole.fed] == [(1, 0), (1, 1), (2, 0), (2, 1)]
    for a, b in zip(resumed.fed, whole.fed):
        for x, y in zip(a[2] + [a[3], a[4]], b[2] + [b[3], b[4]]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # what was fed: the random feeder's p4, z1, z2 and the farthest-point pyramid of that p4 from the mirror's start index
    mirror = fm.MirrorFeeder(host, Bf, sizes, seed=31)
    for epoch, i, reals, z1, z2 in whole.fed:
        want, w1, w2 = mirror.batch(epoch, i, np.float64)
        assert np.array_equal(_bits(reals[3].cpu().numpy()), _bits(want[3]))
        assert np.abs(z1.cpu().numpy() - w1).max() < 1e-5 and np.abs(z2.cpu().numpy() - w2).max() < 1e-5
        _, rows, t = mirror.schedule(epoch, i)
        starts = torch.from_numpy(fpm.start_indices(31, t, rows, Nf)).to(dev)
        order = pointops.fps_order(reals[3].transpose(1, 2).contiguous(), sizes[2], starts).long()
        p3 = torch.gather(reals[3], 2, order[:, None, :].expand(Bf, 3, sizes[2]))
        assert torch.equal(p3, reals[2]) and torch.equal(reals[1], p3[:, :, :sizes[1]]) and torch.equal(reals[0], p3[:, :, :sizes[0]])
        assert all(len(set(row)) == sizes[2] for row in order.cpu().tolist())


# ---------------------------------------------------------------------------- command line
def test_cli_trains_one_epoch_with_subsample_fps(tmp_path):
    from pdgn_amd.data import cate_to_synsetid
    rng = np.random.default_rng(5)
    sid = cate_to_synsetid["chair"]
    Nc = 64
    for sp, n in (("train", 9), ("val", 2), ("test", 2)):
        (tmp_path / "pc" / sid / sp).mkdir(parents=True)
        for j in range(n):
            np.save(tmp_path / "pc" / sid / sp / ("shape%02d.npy" % j), rng.standard_normal((Nc, 3)).astype(np.float32))
    argv = ["--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root", str(tmp_path / "pc"), "--choice", "chair",
            "--batch_size", "4", "--seed", "1", "--num_point", str(Nc), "--num_k", "4", "--phase", "train", "--max_epoch", "1", "--snapshot", "1",
            "--subsample", "fps"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "pdgn_amd.train"] + argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    ck = tmp_path / "ck" / "toy" / "PDGNet_v2"
    assert (ck / "1_chair_G.pth").exists() and (ck / "1_chair_D.pth").exists()
    log = (tmp_path / "ck" / "toy" / "log_info.txt").read_text().splitlines()
    assert "subsample='fps'" in log[0]
    assert sum(l.startswith("Epoch: [ 1]") for l in log) == 2                    # 9 clouds, batches of 4
