"""GPU: the resampling feeder (csrc/feed.hip: pdgn_feed_batch_resample, through pdgn_amd.data.BatchFeeder(num_point=, pool=) and
directly) against its host mirror (tests/resample_mirror.py), PDGNTrainer.fit over it, and the command line's train -> test round trip
on a PC15k-style directory at toy size.  Every output sits inside a sentinel-filled guard band."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feed_mirror as fm
import resample_mirror as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 0.2
GUARD = 64                                                       # floats on either side of every output (a multiple of 4: 16-byte alignment kept)
SENTINEL = -12345.0
INVALID = -1


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _clouds(S, M, seed=0):
    return np.random.default_rng(seed).standard_normal((S, M, 3)).astype(np.float32)


def _coded_clouds(S, M):
    """data[c, i] = (c, i, c * M + i): every coordinate names its cloud and point (exact in fp32 below 2^24)."""
    c, i = np.meshgrid(np.arange(S), np.arange(M), indexing="ij")
    assert S * M < 1 << 24
    return np.stack([c, i, c * M + i], axis=2).astype(np.float32)


def _guarded(shape, dev):
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


def _raw(clouds, order, B, sizes, P, N, first, seed, t, row0, plain=False, untouched=False):
    """pdgn_feed_batch_resample itself (plain: pdgn_feed_batch on the same arguments) into guarded buffers -> (rc, [p1 .. p4, z1, z2]).
    untouched: assert that not one float was written, inside the outputs or outside."""
    from pdgn_amd import _lib
    dev = clouds.device
    S, M, _ = clouds.shape
    made = [_guarded((B, 3, r), dev) for r in tuple(sizes) + (N,)] + [_guarded((B, 128), dev) for _ in range(2)]
    ptrs = [_lib.ptr(v) for v, _ in made]
    tail = (sizes[0], sizes[1], sizes[2], _lib.ptr(clouds), _lib.ptr(order), first, seed, t, row0, SIGMA, *ptrs, _lib.stream_of(clouds))
    if plain:
        assert M == P == N
        rc = _lib.lib().pdgn_feed_batch(B, S, N, *tail)
    else:
        rc = _lib.lib().pdgn_feed_batch_resample(B, S, M, P, N, *tail)
    torch.cuda.synchronize()
    for _, whole in made:
        assert _guards_intact(whole)
        if untouched:
            assert bool((whole == SENTINEL).all())
    return rc, [v.cpu().numpy() for v, _ in made]


def _mirror_raw(host, order, B, sizes, P, N, first, seed, t, row0):
    """The mirror's [p1 .. p4] for a raw call (any t, any row0)."""
    rows = row0 + np.arange(B)
    pcs = host[np.asarray(order)[first:first + B]]
    idx = [fm.indices_from_words(fm.stream_words(seed, t, rows, k, r), P) for k, r in enumerate(sizes)]
    idx.append(rm.permute(P, rm.round_keys(seed, t, rows), N))
    return [np.ascontiguousarray(np.take_along_axis(pcs, ix[:, :, None], axis=1).transpose(0, 2, 1)) for ix in idx]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


CONFIGS = [  # B, S, sizes, M, P, N, rank, world
    (3, 7, (3, 5, 6), 13, 11, 10, 0, 1),                         # a tail group of fewer than 4 columns, unaligned rows
    (3, 7, (4, 8, 12), 16, 16, 16, 0, 1),                        # N = P = M: a permutation of the whole cloud
    (3, 7, (8, 16, 32), 96, 65, 64, 0, 1),                       # M > P: the stride is M, not P
    (3, 7, (8, 16, 32), 128, 128, 64, 0, 1),                     # P = 2^k
    (3, 7, (8, 16, 32), 130, 129, 64, 0, 1),                     # P = 2^k + 1: one more bit, an odd count of them
    (3, 7, (256, 512, 1024), 15000, 10000, 2048, 0, 1),          # the workload's cloud, PointFlow's pool; several blocks per row
    (2, 13, (8, 16, 32), 96, 65, 64, 1, 3),                      # rank 1 of 3
]


@pytest.mark.parametrize("B,S,sizes,M,P,N,rank,world", CONFIGS)
def test_batches_are_bit_equal_to_the_mirror(B, S, sizes, M, P, N, rank, world):
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    host = _clouds(S, M)
    feeder = BatchFeeder(torch.from_numpy(host).to(dev), B, sizes, seed=9999, rank=rank, world=world, sigma=SIGMA, num_point=N, pool=P)
    mirror = rm.MirrorResampleFeeder(host, B, sizes, seed=9999, rank=rank, world=world, sigma=SIGMA, num_point=N, pool=P)
    assert (feeder.M, feeder.P, feeder.N) == (M, P, N) and feeder._fn.__name__ == "pdgn_feed_batch_resample"
    assert feeder.shapes() == [(B, 3, r) for r in sizes + (N,)] + [(B, 128)]
    assert feeder.batches_per_epoch == mirror.batches_per_epoch >= 1
    for epoch, i in ((1, 0), (1, mirror.batches_per_epoch - 1), (3, 0)):
        reals, z1, z2 = _fill(feeder, epoch, i)
        want, w1, w2 = mirror.batch(epoch, i, np.float64)
        for k in range(4):
            assert reals[k].shape == want[k].shape
            assert np.array_equal(_bits(reals[k]), _bits(want[k])), (epoch, i, k)
        assert np.abs(z1 - w1).max() < 1e-5 and np.abs(z2 - w2).max() < 1e-5      # (byte-equal to pdgn_feed_batch's: test_noise_*)


@pytest.mark.parametrize("t,row0", [((1 << 32) + 5, 0), ((0xABCDEF << 32) | 0xFFFFFFFF, 7), (3, (1 << 32) - 3)],
                         ids=["t=2^32+5", "t=hi24", "row0=2^32-B"])
def test_wide_counters_are_bit_equal_to_the_mirror(t, row0):
    dev = _dev()
    B, S, sizes, M, P, N = 3, 7, (8, 16, 32), 96, 65, 64
    host = _clouds(S, M, seed=1)
    order = fm.epoch_order(5, 1, S)
    rc, got = _raw(torch.from_numpy(host).to(dev), torch.from_numpy(order).to(dev), B, sizes, P, N, 2, 5, t, row0)
    assert rc == 0
    want = _mirror_raw(host, order, B, sizes, P, N, 2, 5, t, row0)
    for k in range(4):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    rows = row0 + np.arange(B)
    for k, tag in ((4, fm.TAG_Z1), (5, fm.TAG_Z2)):
        assert np.abs(got[k] - fm.normals_from_words(fm.stream_words(5, t, rows, tag, 128), SIGMA)).max() < 1e-5
    # the low word alone draws something else: the high part of t is part of the counter
    if t >> 32:
        _, low = _raw(torch.from_numpy(host).to(dev), torch.from_numpy(order).to(dev), B, sizes, P, N, 2, 5, t & 0xFFFFFFFF, row0)
        assert (got[3].reshape(B, -1) != low[3].reshape(B, -1)).any(axis=1).all()


def test_rows_hold_distinct_points_of_the_pool_of_their_cloud():
    dev = _dev()
    B, S, sizes, M, P, N = 5, 9, (8, 16, 32), 200, 150, 64
    host = _coded_clouds(S, M)
    order = fm.epoch_order(12, 1, S)
    rc, out = _raw(torch.from_numpy(host).to(dev), torch.from_numpy(order).to(dev), B, sizes, P, N, 3, 12, 41, 0)
    assert rc == 0
    for k in range(4):
        cloud, point, both = out[k][:, 0].astype(np.int64), out[k][:, 1].astype(np.int64), out[k][:, 2].astype(np.int64)
        assert np.array_equal(cloud, np.broadcast_to(order[3:3 + B, None], cloud.shape)), k       # rows take the clouds order[first + b]
        assert np.array_equal(both, cloud * M + point), k                                          # whole points, never mixed coordinates
        assert point.min() >= 0 and point.max() < P, k                                             # from the pool
        if k == 3:
            assert all(len(set(row)) == N for row in point.tolist())                               # N distinct points per row
    # N = P: every point of the pool exactly once
    rc, out = _raw(torch.from_numpy(host).to(dev), torch.from_numpy(order).to(dev), B, sizes, 150, 150, 3, 12, 41, 0)
    assert rc == 0 and np.array_equal(np.sort(out[3][:, 1].astype(np.int64), axis=1), np.broadcast_to(np.arange(150), (B, 150)))


def test_noise_is_byte_equal_to_the_plain_feeders():
    dev = _dev()
    B, S, sizes = 35, 40, (8, 16, 32)
    order = torch.from_numpy(fm.epoch_order(5, 1, S)).to(dev)
    dense = torch.from_numpy(_clouds(S, 96)).to(dev)
    exact = torch.from_numpy(_clouds(S, 64)).to(dev)
    for t, row0 in ((11, 0), ((7 << 32) + 1, 70)):
        rc_a, a = _raw(dense, order, B, sizes, 80, 64, 2, 77, t, row0)
        rc_b, b = _raw(exact, order, B, sizes, 64, 64, 2, 77, t, row0, plain=True)
        assert rc_a == 0 and rc_b == 0
        assert np.array_equal(_bits(a[4]), _bits(b[4])) and np.array_equal(_bits(a[5]), _bits(b[5]))


def test_feed_is_a_pure_function_of_its_arguments():
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    B, S, sizes, M, P, N = 4, 30, (8, 16, 32), 96, 80, 64
    host = _clouds(S, M, seed=2)
    clouds = torch.from_numpy(host).to(dev)
    order = torch.from_numpy(fm.epoch_order(5, 1, S)).to(dev)
    args = dict(B=B, sizes=sizes, P=P, N=N, first=8)
    _, a = _raw(clouds, order, seed=5, t=11, row0=0, **args)
    changed = {"seed": _raw(clouds, order, seed=6, t=11, row0=0, **args)[1], "t": _raw(clouds, order, seed=5, t=12, row0=0, **args)[1],
               "row": _raw(clouds, order, seed=5, t=11, row0=1, **args)[1]}
    _, b = _raw(clouds, order, seed=5, t=11, row0=0, **args)                   # the same arguments after other launches: the same bytes
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    for what, c in changed.items():                                             # every row of every output draws something else
        for k in range(6):
            assert (a[k].reshape(B, -1) != c[k].reshape(B, -1)).any(axis=1).all(), (what, k)
    # W ranks at batch B are fed what one rank is fed at batch B * W
    W = 3
    one = BatchFeeder(clouds, B * W, sizes, seed=9, sigma=SIGMA, num_point=N, pool=P)
    ranks = [BatchFeeder(clouds, B, sizes, seed=9, rank=r, world=W, sigma=SIGMA, num_point=N, pool=P) for r in range(W)]
    assert one.batches_per_epoch == ranks[0].batches_per_epoch == 2
    for epoch, i in ((1, 1), (2, 0)):
        whole = _fill(one, epoch, i)
        parts = [_fill(f, epoch, i) for f in ranks]
        for k in range(4):
            assert np.array_equal(_bits(np.concatenate([p[0][k] for p in parts])), _bits(whole[0][k])), (epoch, i, k)
        for k in (1, 2):
            assert np.array_equal(_bits(np.concatenate([p[k] for p in parts])), _bits(whole[k]))


def test_default_feeder_is_unchanged():
    """M == N and no pool: pdgn_feed_batch, byte for byte what it writes when called directly and what its mirror says."""
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    B, S, sizes, N = 5, 23, (8, 16, 32), 64
    host = _clouds(S, N, seed=6)
    clouds = torch.from_numpy(host).to(dev)
    for kw in ({}, {"num_point": N}):
        feeder = BatchFeeder(clouds, B, sizes, seed=21, sigma=SIGMA, **kw)
        assert feeder._fn.__name__ == "pdgn_feed_batch" and (feeder.M, feeder.P, feeder.N) == (N, N, N)
        reals, z1, z2 = _fill(feeder, 2, 1)
        want, _, _ = fm.MirrorFeeder(host, B, sizes, seed=21, sigma=SIGMA).batch(2, 1)
        order = torch.from_numpy(fm.epoch_order(21, 2, S)).to(dev)
        rc, direct = _raw(clouds, order, B, sizes, N, N, first=B, seed=21, t=feeder.batches_per_epoch + 1, row0=0, plain=True)
        assert rc == 0
        for k in range(4):
            assert np.array_equal(_bits(reals[k]), _bits(want[k])) and np.array_equal(_bits(reals[k]), _bits(direct[k])), k
        assert np.array_equal(reals[3], host[fm.epoch_order(21, 2, S)[B:2 * B]].transpose(0, 2, 1))           # the whole cloud, in order
        assert np.array_equal(_bits(z1), _bits(direct[4])) and np.array_equal(_bits(z2), _bits(direct[5]))
    with pytest.raises(ValueError):
        BatchFeeder(clouds, B, sizes, seed=21, num_point=N + 1)
    with pytest.raises(ValueError):
        BatchFeeder(clouds, B, sizes, seed=21, num_point=32, pool=31)
    with pytest.raises(ValueError):
        BatchFeeder(clouds, B, sizes, seed=21, num_point=32, pool=N + 1)
    assert BatchFeeder(clouds, B, sizes, seed=21, pool=N)._fn.__name__ == "pdgn_feed_batch_resample"      # a pool asks for the draw


def test_invalid_arguments_are_refused_before_any_launch():
    dev = _dev()
    B, S, sizes, M = 4, 13, (8, 16, 32), 96
    clouds = torch.from_numpy(_clouds(S, M)).to(dev)
    order = torch.from_numpy(fm.epoch_order(5, 1, S)).to(dev)
    ok = dict(B=B, sizes=sizes, P=80, N=64, first=0, seed=5, t=0, row0=0)
    assert _raw(clouds, order, **ok)[0] == 0
    for bad in (dict(N=81), dict(P=97), dict(N=0), dict(P=0, N=0), dict(first=S - B + 1), dict(first=-1), dict(sizes=(8, 0, 32)),
                dict(row0=-1), dict(row0=(1 << 32) - B + 1), dict(B=0)):
        assert _raw(clouds, order, untouched=True, **dict(ok, **bad))[0] == INVALID, bad


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
            assert np.array_equal(_bits(reals[k].cpu().numpy()), _bits(want[k])), (epoch, i, k)
        assert np.abs(z1.cpu().numpy() - w1).max() < 1e-5 and np.abs(z2.cpu().numpy() - w2).max() < 1e-5, (epoch, i)


FIT = dict(B=4, N=2048, sizes=(256, 512, 1024), M=3000, P=2500)               # the trainer shape of tests/test_gpu_feed.py's fit tests


def test_fit_feeds_the_launch_list_fresh_subsets():
    from pdgn_amd.data import BatchFeeder
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    dev = _dev()
    B, N, sizes, M, P = FIT["B"], FIT["N"], FIT["sizes"], FIT["M"], FIT["P"]
    S = 3 * B + 1
    host = _clouds(S, M, seed=3)
    clouds = torch.from_numpy(host).to(dev)
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    tr.capture_list(synthetic_batch(B, dev), noise(B, dev), noise(B, dev))
    static = [r.data_ptr() for r in tr._static["reals"]] + [tr._static["z1"].data_ptr(), tr._static["z2"].data_ptr()]
    feeder = RecordingFeeder(BatchFeeder(clouds, B, sizes, seed=77, num_point=N, pool=P))
    mirror = rm.MirrorResampleFeeder(host, B, sizes, seed=77, num_point=N, pool=P)
    lines = []
    assert tr.fit(feeder, 2, log=lines.append) == 2
    torch.cuda.synchronize()
    assert len(feeder.fed) == len(lines) == 2 * 3
    assert [(e, i) for e, i, *_ in feeder.fed] == [(e, i) for e in (1, 2) for i in range(3)]
    assert all(f[5] == static for f in feeder.fed)                              # written straight into the list's static buffers
    _equal_feeds(feeder.fed, mirror)                                            # after iteration i: the mirror's batch i
    for line in lines:
        vals = [float(tok.rstrip(",")) for tok in line.split("time:")[1].split()[2:][1::2]]
        assert len(vals) == 6 and all(np.isfinite(v) for v in vals), line
    # a cloud visited in both epochs shows two different subsets of its own pool
    seen = {}
    for epoch, i, reals, *_ in feeder.fed:
        ids = mirror.schedule(epoch, i)[0]
        for b, c in enumerate(ids.tolist()):
            seen.setdefault(c, {})[epoch] = set(map(tuple, reals[3][b].t().cpu().numpy().tolist()))
    twice = [c for c, by_epoch in seen.items() if len(by_epoch) == 2]
    assert len(twice) >= S - 2
    for c in twice:
        pool = set(map(tuple, host[c, :P].tolist()))
        first, second = seen[c][1], seen[c][2]
        assert len(first) == len(second) == N and first <= pool and second <= pool and first != second, c
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def test_resumed_epoch_is_fed_what_an_uninterrupted_run_is_fed(tmp_path):
    """Feeds only, as in tests/test_gpu_feed.py: trajectories are not bit-reproducible and nothing here claims they are."""
    from pdgn_amd.data import BatchFeeder
    from pdgn_amd.trainer import PDGNTrainer
    dev = _dev()
    B, N, sizes, M, P = FIT["B"], FIT["N"], FIT["sizes"], FIT["M"], FIT["P"]
    S = 2 * B + 1
    host = _clouds(S, M, seed=4)
    clouds = torch.from_numpy(host).to(dev)
    new_feeder = lambda: RecordingFeeder(BatchFeeder(clouds, B, sizes, seed=31, num_point=N, pool=P))

    def new_trainer():
        torch.manual_seed(0)
        tr = PDGNTrainer(device=dev, distributed=False)
        tr.train()
        return tr

    whole = new_feeder()
    assert new_trainer().fit(whole, 2, issue="eager") == 2                      # the uninterrupted run: epochs 1, 2
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
    _equal_feeds(resumed.fed, rm.MirrorResampleFeeder(host, B, sizes, seed=31, num_point=N, pool=P))


# ---------------------------------------------------------------------------- command line
def test_cli_train_then_test_round_trip_on_a_pc15k_directory(tmp_path, monkeypatch):
    """A PC15k-style directory with M = 96, --num_point 64: --phase train for one epoch as a child process (the parent commit exits
    with "--num_point 64 but the clouds of ... have 96 points"), then --phase test, here in this process so that the reference clouds
    the evaluation is handed can be looked at: they are the normalised tails [M - N, M) of the stored test clouds."""
    from pdgn_amd import evaluation, train
    from pdgn_amd.data import cate_to_synsetid, normalize_clouds
    rng = np.random.default_rng(5)
    sid = cate_to_synsetid["chair"]
    M, N, n_test = 96, 64, 6
    stored = {}
    for sp, n in (("train", 9), ("val", 2), ("test", n_test)):
        (tmp_path / "pc" / sid / sp).mkdir(parents=True)
        stored[sp] = rng.standard_normal((n, M, 3)).astype(np.float32)
        for j in range(n):
            np.save(tmp_path / "pc" / sid / sp / ("shape%02d.npy" % j), stored[sp][j])
    common = ["--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root", str(tmp_path / "pc"), "--choice", "chair",
              "--batch_size", "4", "--seed", "1", "--save_dir", str(tmp_path / "res"), "--num_point", str(N), "--num_k", "4"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "pdgn_amd.train"] + common + ["--phase", "train", "--max_epoch", "1", "--snapshot", "1"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    ck = tmp_path / "ck" / "toy" / "PDGNet_v2"
    assert (ck / "1_chair_G.pth").exists() and (ck / "1_chair_D.pth").exists()
    log = (tmp_path / "ck" / "toy" / "log_info.txt").read_text().splitlines()
    assert sum(l.startswith("Epoch: [ 1]") for l in log) == 2                    # 9 clouds, batches of 4
    assert "resample_pool" not in log[0]

    handed = {}
    real = evaluation.generate_and_evaluate

    def spy(G, ref, *a, **kw):
        handed["ref"] = ref.detach().cpu().clone()
        return real(G, ref, *a, **kw)

    monkeypatch.setattr(evaluation, "generate_and_evaluate", spy)
    out = train.main(common + ["--phase", "test", "--pretrain_model_G", "1_chair_G.pth", "--pretrain_model_D", "1_chair_D.pth"])
    assert os.path.basename(out).startswith("GEN_Ours_chair_")
    assert np.load(os.path.join(out, "out.npy")).shape == (n_test, N, 3)
    metrics = dict(l.split(": ") for l in open(os.path.join(out, "log.txt")).read().splitlines())
    assert "jsd" in metrics and "1-NN-CD-acc" in metrics and all(np.isfinite(float(v)) for v in metrics.values()), metrics
    tails = normalize_clouds(torch.from_numpy(stored["test"][:, M - N:]), "shape_bbox")[0]          # --normalize's default
    ref = handed["ref"]
    assert tuple(ref.shape) == (n_test, N, 3)
    want = {tuple(np.round(c.numpy().ravel()[:6], 5).tolist()) for c in tails}                       # (the data set shuffles the clouds)
    assert {tuple(np.round(c.numpy().ravel()[:6], 5).tolist()) for c in ref} == want
    for c in ref:                                                                                    # each one IS a tail, bit for bit
        assert any(torch.equal(c, w) for w in tails)
