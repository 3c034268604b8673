"""GPU: the ragged feeder -- pdgn_feed_batch_ragged and pdgn_sample_ragged (csrc/feed.hip) on guard-banded buffers
against their host mirror (tests/ragged_mirror.py) and against pdgn_feed_batch_resample on uniform sets, data.RaggedFeeder alone, with the
farthest-point pyramid behind it and inside PDGNTrainer.fit, and the command line on a ragged directory.  Every comparison is exact.

The small shapes are the ones at which this kernel can still go wrong, not the workload's: N = 16 (16-byte stores) and 18 (scalar
stores), shape counts 1, 2, 3, 5, N - 1, N, N + 1, 4 N + 3, 64, 65 -- shorter than, equal to and longer than N in one batch."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feed_mirror as fm
import fps_mirror
import ragged_mirror as gm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 0.2
GUARD = 64                                                       # elements on either side of every output (a multiple of 4: 16-byte alignment kept)
SENTINEL = -12345.0
INVALID = -1


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _counts(S, N):
    pool = [1, 2, 3, 5, N - 1, N, N + 1, 4 * N + 3, 64, 65]
    return [pool[i] for i in (0, 2, 4, 5, 6, 7, 9)] if S == 7 else (pool + pool)[:S]


@functools.lru_cache(maxsize=None)
def _set(S, N, marked=False):
    """(the clouds as a list of numpy arrays, the CloudSet on the device): built once per (S, N), never written.  marked: x = the shape's
    index, y = the point's index inside its shape, z = -y, so that an output column says where it came from."""
    from pdgn_amd.clouds import CloudSet
    rng = np.random.default_rng(1000 * S + N)
    if marked:
        clouds = [np.stack([np.full(m, s), np.arange(m), -np.arange(m)], 1).astype(np.float32) for s, m in enumerate(_counts(S, N))]
    else:
        clouds = [rng.standard_normal((m, 3)).astype(np.float32) for m in _counts(S, N)]
    return clouds, CloudSet.from_clouds(clouds).to(_dev())


@functools.lru_cache(maxsize=None)
def _uniform(S, M):
    from pdgn_amd.clouds import CloudSet
    stack = np.random.default_rng(M).standard_normal((S, M, 3)).astype(np.float32)
    return stack, torch.from_numpy(stack).to(_dev()), CloudSet.from_clouds(list(stack)).to(_dev())


def _guarded(shape, dev):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return whole[GUARD:GUARD + n].view(shape), whole


def _guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def _outputs(B, lens, dev):
    return [_guarded((B, 3, r), dev) for r in lens] + [_guarded((B, 128), dev) for _ in range(2)]


def _finish(made, untouched):
    torch.cuda.synchronize()
    for _, whole in made:
        assert _guards_intact(whole)
        if untouched:
            assert bool((whole == SENTINEL).all())
    return [v.cpu().numpy() for v, _ in made]


def _raw(cs, order, B, lens, first=0, seed=5, t=0, row0=0, untouched=False, **over):
    """pdgn_feed_batch_ragged itself into guarded buffers -> (rc, [p1 .. p4, z1, z2] as numpy).  over: replaces arguments by name (S T
    points off order_ptr p1 .. z2: a tensor, or an int address -- 0 for NULL)."""
    from pdgn_amd import _lib
    dev = cs.points.device
    order = torch.as_tensor(np.asarray(order, dtype=np.int32)).to(dev)
    made = _outputs(B, lens, dev)
    a = dict(S=cs.S, T=cs.T, points=cs.points, off=cs.off, order=order)
    a.update(zip(("p1", "p2", "p3", "p4", "z1", "z2"), (v for v, _ in made)))
    if "order_ptr" in over:
        a["order"] = over.pop("order_ptr")
    a.update(over)
    p = lambda x: x if isinstance(x, int) else _lib.ptr(x)
    rc = _lib.lib().pdgn_feed_batch_ragged(B, a["S"], lens[3], lens[0], lens[1], lens[2], p(a["points"]), p(a["off"]), a["T"], p(a["order"]), first,
                                           seed, t, row0, SIGMA, p(a["p1"]), p(a["p2"]), p(a["p3"]), p(a["p4"]), p(a["z1"]), p(a["z2"]),
                                           _lib.stream_of(cs.points))
    return rc, _finish(made, untouched)


def _raw_plain(data, order, B, lens, first=0, seed=5, t=0, row0=0, resample=None):
    """pdgn_feed_batch (data (S,N,3)) or, with resample = M, pdgn_feed_batch_resample(M = P = M) into guarded buffers."""
    from pdgn_amd import _lib
    dev = data.device
    order = torch.as_tensor(np.asarray(order, dtype=np.int32)).to(dev)
    made = _outputs(B, lens, dev)
    fn = _lib.lib().pdgn_feed_batch if resample is None else _lib.lib().pdgn_feed_batch_resample
    dims = (B, data.shape[0], lens[3]) if resample is None else (B, data.shape[0], resample, resample, lens[3])
    rc = fn(*dims, lens[0], lens[1], lens[2], _lib.ptr(data), _lib.ptr(order), first, seed, t, row0, SIGMA, *[_lib.ptr(v) for v, _ in made],
            _lib.stream_of(data))
    return rc, _finish(made, False)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _fill(feeder, epoch, i):
    """feeder.fill into guarded buffers -> ([p1 .. p4], z1, z2) as numpy."""
    made = [_guarded(s, feeder.device) for s in feeder.shapes()[:4]] + [_guarded(feeder.shapes()[4], feeder.device) for _ in range(2)]
    views = [v for v, _ in made]
    feeder.fill(epoch, i, views[:4], views[4], views[5])
    out = _finish(made, False)
    return out[:4], out[4], out[5]


# ---------------------------------------------------------------------------- 1. bit-equality with the mirror
CONFIGS = [(3, 7, 16, (4, 8, 16), 0, 1), (3, 7, 18, (3, 6, 9), 1, 2), (5, 11, 16, (3, 6, 9), 1, 2), (5, 11, 18, (4, 8, 16), 0, 1),
           (5, 7, 18, (3, 6, 9), 0, 1), (3, 11, 16, (4, 8, 16), 1, 2), (5, 11, 16, (4, 8, 16), 0, 1), (3, 11, 18, (3, 6, 9), 0, 1)]


@pytest.mark.parametrize("B,S,N,sizes,rank,world", CONFIGS)
def test_batches_are_bit_equal_to_the_mirror(B, S, N, sizes, rank, world):
    from pdgn_amd.data import RaggedFeeder
    clouds, cs = _set(S, N)
    feeder = RaggedFeeder(cs, B, sizes, seed=9999, rank=rank, world=world, sigma=SIGMA, num_point=N)
    mirror = gm.MirrorRaggedFeeder(clouds, B, sizes, seed=9999, rank=rank, world=world, sigma=SIGMA, num_point=N)
    assert feeder._fn.__name__ == "pdgn_feed_batch_ragged" and feeder.batches_per_epoch == mirror.batches_per_epoch >= 1
    assert feeder.shapes() == [(B, 3, r) for r in sizes + (N,)] + [(B, 128)]
    zeros = torch.zeros(S, N, 3, device=cs.points.device)
    short = long = 0
    for epoch in (1, 2, 40):
        for i in range(feeder.batches_per_epoch):
            reals, z1, z2 = _fill(feeder, epoch, i)
            want, _, _ = mirror.batch(epoch, i)
            for k in range(4):
                assert _same(reals[k], want[k]), (epoch, i, k)
            ids, rows, t = mirror.schedule(epoch, i)
            m = np.diff(mirror.off)[ids]
            short, long = short + int((m < N).sum()), long + int((m > N).sum())
            # the noise: the bytes of pdgn_feed_batch for the same (seed, t, row0, sigma)
            rc, plain = _raw_plain(zeros, np.arange(S), B, sizes + (N,), seed=9999, t=t, row0=int(rows[0]))
            assert rc == 0 and _same(z1, plain[4]) and _same(z2, plain[5]), (epoch, i)
    assert short > 0 and long > 0                                # shapes shorter and longer than N were fed


WIDE = [((1 << 32) + 5, 0), ((0xABCDEF << 32) | 0xFFFFFFFF, 7), (3, (1 << 32) - 3)]


@pytest.mark.parametrize("t,row0", WIDE)
def test_wide_counters_are_bit_equal_to_the_mirror(t, row0):
    B, S = 3, 7
    for N, sizes in ((16, (4, 8, 16)), (18, (3, 6, 9))):
        clouds, cs = _set(S, N)
        order = fm.epoch_order(5, 1, S)
        rc, got = _raw(cs, order, B, sizes + (N,), first=2, seed=(77 << 32) | 77, t=t, row0=row0)
        assert rc == 0
        want, _, _ = gm.feed_batch_ragged(cs.points.cpu().numpy(), cs.off.cpu().numpy(), order, 2, B, sizes + (N,), (77 << 32) | 77, t, row0)
        for k in range(4):
            assert _same(got[k], want[k]), (N, k)
        rc, plain = _raw_plain(torch.zeros(S, N, 3, device=cs.points.device), order, B, sizes + (N,), first=2, seed=(77 << 32) | 77, t=t, row0=row0)
        assert rc == 0 and _same(got[4], plain[4]) and _same(got[5], plain[5])
        if t >> 32:                                              # the high part of t is part of the counter
            _, low = _raw(cs, order, B, sizes + (N,), first=2, seed=(77 << 32) | 77, t=t & 0xFFFFFFFF, row0=row0)
            assert all(not np.array_equal(got[k], low[k]) for k in range(6))
    # order entries outside [0, S) are clamped, repeated ones are fine
    clouds, cs = _set(7, 16)
    order = [4, 4, -3, 99, 1, 5, 6]
    rc, got = _raw(cs, order, 5, (3, 6, 9, 16), first=1, seed=3, t=t, row0=row0 if row0 + 5 <= 1 << 32 else 0)
    want, _, _ = gm.feed_batch_ragged(cs.points.cpu().numpy(), cs.off.cpu().numpy(), order, 1, 5, (3, 6, 9, 16), 3, t, row0 if row0 + 5 <= 1 << 32 else 0)
    assert rc == 0 and all(_same(got[k], want[k]) for k in range(4))


# ---------------------------------------------------------------------------- 2. every column comes from the row's own shape
@pytest.mark.parametrize("N,sizes", [(16, (4, 8, 16)), (18, (3, 6, 9))])
def test_rows_stay_inside_their_own_shape(N, sizes):
    S = 11
    _, cs = _set(S, N, True)
    counts = _counts(S, N)
    order = fm.epoch_order(8, 3, S)
    for first, t in ((0, 0), (S - 5, 9)):
        rc, got = _raw(cs, order, 5, sizes + (N,), first=first, seed=31, t=t, row0=first)
        assert rc == 0
        for b in range(5):
            c = int(order[first + b])
            M = counts[c]
            for k in range(4):
                x, y, z = got[k][b]
                assert (x == c).all() and (y >= 0).all() and (y < M).all() and np.array_equal(z, -y) and np.array_equal(y, np.round(y)), (b, k)
            occ = np.bincount(got[3][b][1].astype(np.int64), minlength=M)
            if M >= N:
                assert occ.max() == 1 and occ.sum() == N, (b, M)     # N distinct points
            else:
                assert occ.min() >= N // M and occ.max() <= -(-N // M) and occ.sum() == N, (b, M, occ)


# ---------------------------------------------------------------------------- 3. a uniform set is the resampling feeder's
@pytest.mark.parametrize("M,N", [(40, 16), (16, 16)])
def test_uniform_set_is_byte_equal_to_the_resampling_launch(M, N):
    S, B = 7, 3
    _, stack, cs = _uniform(S, M)
    assert cs.counts().tolist() == [M] * S
    order = fm.epoch_order(6, 2, S)
    for sizes in ((4, 8, 16), (3, 6, 9)):
        for first, t, row0 in ((0, 0, 0), (4, (5 << 32) + 1, 70)):
            rc, got = _raw(cs, order, B, sizes + (N,), first=first, seed=77, t=t, row0=row0)
            rc2, want = _raw_plain(stack, order, B, sizes + (N,), first=first, seed=77, t=t, row0=row0, resample=M)
            assert rc == rc2 == 0
            for k in range(6):
                assert _same(got[k], want[k]), (sizes, first, k)
            rc3, plain = _raw_plain(stack[:, :N].contiguous(), order, B, sizes + (N,), first=first, seed=77, t=t, row0=row0)
            assert rc3 == 0 and _same(got[4], plain[4]) and _same(got[5], plain[5])


# ---------------------------------------------------------------------------- 4. a pure function; ranks compose
def test_feed_is_a_pure_function_and_ranks_compose():
    from pdgn_amd.data import RaggedFeeder
    S, N, sizes = 11, 18, (3, 6, 9)
    clouds, cs = _set(S, N)
    order = fm.epoch_order(5, 1, S)
    lens = sizes + (N,)
    _, a = _raw(cs, order, 5, lens, first=2, seed=77, t=11)
    _, b = _raw(cs, order, 5, lens, first=2, seed=77, t=11)
    assert all(_same(a[k], b[k]) for k in range(6))
    for what, kw in (("seed", dict(seed=78, t=11)), ("t", dict(seed=77, t=12)), ("row", dict(seed=77, t=11, row0=1))):
        _, c = _raw(cs, order, 5, lens, first=2, **kw)
        assert all(not np.array_equal(a[k], c[k]) for k in range(6)), what
    W, bb = 2, 2
    one = RaggedFeeder(cs, bb * W, sizes, seed=9, sigma=SIGMA, num_point=N)
    ranks = [RaggedFeeder(cs, bb, sizes, seed=9, rank=r, world=W, sigma=SIGMA, num_point=N) for r in range(W)]
    assert one.batches_per_epoch == ranks[0].batches_per_epoch == 2
    for epoch in (1, 2):
        for i in range(2):
            whole = _fill(one, epoch, i)
            parts = [_fill(f, epoch, i) for f in ranks]
            for k in range(4):
                assert _same(np.concatenate([p[0][k] for p in parts]), whole[0][k]), (epoch, i, k)
            for k in (1, 2):
                assert _same(np.concatenate([p[k] for p in parts]), whole[k])


# ---------------------------------------------------------------------------- 5. refusals
def test_invalid_arguments_are_refused_before_any_launch():
    from pdgn_amd import _lib
    S, N, B = 7, 16, 3
    lens = (4, 8, 16, N)
    _, cs = _set(S, N)
    dev = cs.points.device
    order = fm.epoch_order(5, 1, S)
    d_order = torch.from_numpy(order).to(dev)
    p = lambda x: x if isinstance(x, int) else _lib.ptr(x)
    assert _raw(cs, order, B, lens)[0] == 0
    null = 0
    z_odd = torch.zeros(B * 128 + 4, device=cs.points.device)[1:]
    bad_cases = [dict(B=0), dict(B=65536), dict(S=0), dict(lens=(4, 0, 16, N)), dict(lens=(4, 8, 16, 0)), dict(first=-1), dict(first=S - B + 1),
                 dict(row0=-1), dict(row0=(1 << 32) - B + 1), dict(order_ptr=null), dict(p1=null), dict(p4=null), dict(z1=null), dict(z2=null),
                 dict(z1=z_odd.data_ptr()),                                                     # pdgn_feed_batch's own
                 dict(points=null), dict(off=null),                                             # null set pointers
                 dict(off=cs.off.data_ptr() + 4), dict(points=cs.points.data_ptr() + 2),        # off not 8-byte, points not 4-byte aligned
                 dict(T=0), dict(T=-5), dict(T=1 << 31)]                                        # T < 1; T beyond 2^31 - 1
    for bad in bad_cases:
        kw = dict(bad)
        b, l = kw.pop("B", B), kw.pop("lens", lens)
        made = _outputs(B, [max(r, 1) for r in l], dev)          # (the buffers of a refused B or length are just some buffers)
        a = dict(S=cs.S, T=cs.T, points=cs.points, off=cs.off, order=d_order, first=0, row0=0)
        a.update(zip(("p1", "p2", "p3", "p4", "z1", "z2"), (v for v, _ in made)))
        if "order_ptr" in kw:
            a["order"] = kw.pop("order_ptr")
        a.update(kw)
        rc = _lib.lib().pdgn_feed_batch_ragged(b, a["S"], l[3], l[0], l[1], l[2], p(a["points"]), p(a["off"]), a["T"], p(a["order"]), a["first"], 5, 0,
                                               a["row0"], SIGMA, p(a["p1"]), p(a["p2"]), p(a["p3"]), p(a["p4"]), p(a["z1"]), p(a["z2"]),
                                               _lib.stream_of(cs.points))
        assert rc == INVALID, bad
        _finish(made, True)                                      # nothing was written
    assert _raw(cs, order, B, lens)[0] == 0


# ---------------------------------------------------------------------------- 6. CloudSet.sample
def test_sample_is_the_mirrors_and_a_pure_function_of_seed_and_draw():
    from pdgn_amd import _lib
    from pdgn_amd.clouds import CloudSet
    S, N = 11, 16
    clouds, cs = _set(S, N)
    points, off = cs.points.cpu().numpy(), cs.off.cpu().numpy()
    got = {}
    for n in (16, 18, 1):
        for draw in (0, 1, (1 << 32) + 1):
            out = cs.sample(n, 77, draw)
            torch.cuda.synchronize()
            got[(n, draw)] = out.cpu().numpy()
            assert tuple(out.shape) == (S, n, 3) and _same(got[(n, draw)], gm.sample_ragged(points, off, n, 77, draw)), (n, draw)
    assert _same(cs.sample(16, 77).cpu().numpy(), got[(16, 0)])                        # draw defaults to 0; pure
    assert not np.array_equal(got[(16, 0)], got[(16, 1)]) and not np.array_equal(got[(16, 1)], got[(16, (1 << 32) + 1)])
    assert not np.array_equal(got[(16, 0)], cs.sample(16, 78).cpu().numpy())
    long = [s for s, c in enumerate(clouds) if len(c) >= 64]
    assert long and all(not np.array_equal(got[(16, 0)][s], got[(16, 1)][s]) for s in long)
    # apart from the training draw of the same seed, global row s and iteration 0 = draw 0
    assert long == list(range(long[0], long[0] + len(long)))
    _, train = _raw(cs, np.arange(S), len(long), (4, 8, 16, 16), first=long[0], seed=77, t=0, row0=long[0])
    assert all(not np.array_equal(train[3][b].T, got[(16, 0)][s]) for b, s in enumerate(long))
    # shape s does not depend on which other shapes are in the set: {0..4} against {0..2}
    five = CloudSet.from_clouds(clouds[:5]).to(cs.points.device)
    three = CloudSet.from_clouds(clouds[:3]).to(cs.points.device)
    for n in (16, 18):
        assert _same(five.sample(n, 5, 3).cpu().numpy()[:3], three.sample(n, 5, 3).cpu().numpy())
        assert _same(five.sample(n, 5, 3).cpu().numpy(), got_rows(cs, n, 5, 3)[:5])
    # every point of a sampled shape is one of its own; long shapes give distinct points, short ones all of theirs evenly
    _, marked = _set(S, N, True)
    out = marked.sample(18, 4, 2).cpu().numpy()
    for s, M in enumerate(_counts(S, N)):
        assert (out[s, :, 0] == s).all() and (out[s, :, 1] < M).all() and np.array_equal(out[s, :, 2], -out[s, :, 1])
        occ = np.bincount(out[s, :, 1].astype(np.int64), minlength=M)
        assert occ.min() >= 18 // M and occ.max() <= -(-18 // M)
    # guard bands and refusals, called directly
    L = _lib.lib()
    view, whole = _guarded((S, 18, 3), cs.points.device)
    args = lambda **o: [o.get("S", S), o.get("n", 18), o.get("points", _lib.ptr(cs.points)), o.get("off", _lib.ptr(cs.off)), o.get("T", cs.T), 77, 0,
                        o.get("out", _lib.ptr(view)), _lib.stream_of(cs.points)]
    for bad in (dict(S=0), dict(n=0), dict(points=None), dict(off=None), dict(off=cs.off.data_ptr() + 4), dict(points=cs.points.data_ptr() + 2),
                dict(out=None), dict(out=view.data_ptr() + 2), dict(T=0), dict(T=1 << 31)):
        assert L.pdgn_sample_ragged(*args(**bad)) == INVALID, bad
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all())
    assert L.pdgn_sample_ragged(*args()) == 0
    torch.cuda.synchronize()
    assert _guards_intact(whole) and _same(view.cpu().numpy(), gm.sample_ragged(points, off, 18, 77, 0))


def got_rows(cs, n, seed, draw):
    out = cs.sample(n, seed, draw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------- 7. the farthest-point pyramid behind the launch
@pytest.mark.parametrize("N", [16, 18])
def test_fps_pyramid_composes_with_the_ragged_launch(N):
    from pdgn_amd import pointops
    from pdgn_amd.data import RaggedFeeder
    S, B, sizes = 11, 5, (4, 8, 16)
    _, cs = _set(S, N)
    dev = cs.points.device
    plain = RaggedFeeder(cs, B, sizes, seed=21, sigma=SIGMA, num_point=N)
    fps = RaggedFeeder(cs, B, sizes, seed=21, sigma=SIGMA, num_point=N, subsample="fps")
    for epoch, i in ((1, 0), (1, 1), (3, 1)):
        a, az1, az2 = _fill(plain, epoch, i)
        f, fz1, fz2 = _fill(fps, epoch, i)
        assert _same(f[3], a[3]) and _same(fz1, az1) and _same(fz2, az2)
        for k in range(2):
            assert _same(f[k], f[k + 1][:, :, :sizes[k]])        # p1 c p2 c p3: prefixes
        t = (epoch - 1) * plain.batches_per_epoch + i
        start = fps_mirror.start_indices(21, t, np.arange(B), N)
        p4 = torch.from_numpy(f[3]).to(dev)
        order = pointops.fps_order(p4.transpose(1, 2).contiguous(), sizes[2], start=torch.from_numpy(start.astype(np.int32)).to(dev)).long()
        want = torch.gather(p4, 2, order[:, None, :].expand(B, 3, sizes[2])).cpu().numpy()
        for k, r in enumerate(sizes):
            assert _same(f[k], np.ascontiguousarray(want[:, :, :r])), (epoch, i, k)


# ---------------------------------------------------------------------------- 8. RaggedFeeder inside fit
class RecordingFeeder:
    """A feeder whose every fill is followed by a copy of what it wrote (stream-ordered clones)."""

    def __init__(self, feeder):
        self.inner, self.fed = feeder, []
        self.batches_per_epoch, self.rank = feeder.batches_per_epoch, feeder.rank

    def buffers(self):
        return self.inner.buffers()

    def fill(self, epoch, i, reals, z1, z2):
        self.inner.fill(epoch, i, reals, z1, z2)
        self.fed.append((epoch, i, [r.clone() for r in reals], z1.clone(), z2.clone(), [r.data_ptr() for r in reals] + [z1.data_ptr(), z2.data_ptr()]))


FIT = dict(B=2, N=2048, sizes=(256, 512, 1024), counts=(500, 3000, 2048, 2049, 1000, 4000, 2500))   # the trainer shape of the other feeders' fit tests


@functools.lru_cache(maxsize=None)
def _fit_set(S):
    from pdgn_amd.clouds import CloudSet
    rng = np.random.default_rng(3)
    clouds = [rng.standard_normal((m, 3)).astype(np.float32) for m in FIT["counts"][:S]]
    cs = CloudSet.from_clouds(clouds, normalize="shape_unit")
    return [cs.cloud(s).numpy().copy() for s in range(S)], cs.to(_dev())


def _equal_feeds(fed, mirror):
    for epoch, i, reals, z1, z2, _ in fed:
        want, _, _ = mirror.batch(epoch, i)
        for k in range(4):
            assert _same(reals[k].cpu().numpy(), want[k]), (epoch, i, k)


def test_fit_feeds_the_launch_list_fresh_draws():
    from pdgn_amd.data import RaggedFeeder
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    dev = _dev()
    B, N, sizes = FIT["B"], FIT["N"], FIT["sizes"]
    S = 7
    clouds, cs = _fit_set(S)
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    tr.capture_list(synthetic_batch(B, dev), noise(B, dev), noise(B, dev))
    static = [r.data_ptr() for r in tr._static["reals"]] + [tr._static["z1"].data_ptr(), tr._static["z2"].data_ptr()]
    feeder = RecordingFeeder(RaggedFeeder(cs, B, sizes, seed=77, num_point=N))
    mirror = gm.MirrorRaggedFeeder(clouds, B, sizes, seed=77, num_point=N)
    lines = []
    assert tr.fit(feeder, 2, log=lines.append) == 2
    torch.cuda.synchronize()
    assert [(e, i) for e, i, *_ in feeder.fed] == [(e, i) for e in (1, 2) for i in range(3)] and len(lines) == 6
    assert all(f[5] == static for f in feeder.fed)              # written straight into the list's static buffers
    _equal_feeds(feeder.fed, mirror)                            # after iteration i: the mirror's batch i
    for line in lines:
        vals = [float(tok.rstrip(",")) for tok in line.split("time:")[1].split()[2:][1::2]]
        assert len(vals) == 6 and all(np.isfinite(v) for v in vals), line
    # a shape visited in both epochs shows two different draws of its own points, at every resolution
    seen = {}
    for epoch, i, reals, *_ in feeder.fed:
        for b, c in enumerate(mirror.schedule(epoch, i)[0].tolist()):
            seen.setdefault(c, {})[epoch] = [r[b].t().cpu().numpy() for r in reals]
    twice = [c for c, by_epoch in seen.items() if len(by_epoch) == 2]
    assert len(twice) >= S - 2
    for c in twice:
        own = set(map(tuple, clouds[c].tolist()))
        for k in range(4):
            first, second = seen[c][1][k], seen[c][2][k]
            assert not np.array_equal(first, second), (c, k)
            assert set(map(tuple, first.tolist())) <= own and set(map(tuple, second.tolist())) <= own, (c, k)
        if len(clouds[c]) >= N:
            assert len(set(map(tuple, seen[c][1][3].tolist()))) == N
        else:
            assert set(map(tuple, seen[c][1][3].tolist())) == own
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def test_resumed_epoch_is_fed_what_an_uninterrupted_run_is_fed(tmp_path):
    """Feeds only, as in tests/test_gpu_feed.py: trajectories are not bit-reproducible and nothing here claims they are."""
    from pdgn_amd.data import RaggedFeeder
    from pdgn_amd.trainer import PDGNTrainer
    dev = _dev()
    B, N, sizes = FIT["B"], FIT["N"], FIT["sizes"]
    S = 2 * B + 1
    clouds, cs = _fit_set(S)
    new_feeder = lambda: RecordingFeeder(RaggedFeeder(cs, B, sizes, seed=31, num_point=N))

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
    _equal_feeds(resumed.fed, gm.MirrorRaggedFeeder(clouds, B, sizes, seed=31, num_point=N))


# ---------------------------------------------------------------------------- 9. command line
@pytest.mark.parametrize("num_point", [16, 64])
def test_cli_trains_and_tests_on_a_ragged_directory(tmp_path, num_point):
    """Two categories, counts 20 .. 70: one epoch of --phase train under --ragged as a child process (the first log line and the
    checkpoints), then --phase test (out.npy has the reference set's shape, log.txt the metric lines).  --num_point 16: every shape is
    longer than num_point, and the generator starts from ONE point -- its base levels have fewer points than neighbours, which
    pdgn_feature_knn serves since this feature (tests/test_gpu_knn_small.py); --num_point 64, the size the other feeders' command-line
    tests use: shapes shorter and longer than num_point in the train split."""
    from pdgn_amd import train
    from pdgn_amd.data import cate_to_synsetid
    rng = np.random.default_rng(15)
    n_test = 3
    for cate in ("chair", "lamp"):
        for split, count in (("train", 5), ("val", 2), ("test", n_test)):
            folder = tmp_path / "pc" / cate_to_synsetid[cate] / split
            folder.mkdir(parents=True)
            for j in range(count):
                pc = rng.standard_normal((int(rng.integers(20, 71)), 3)).astype(np.float32)     # (chair / train: 67 55 42 56 22 points)
                if j % 2:
                    (folder / ("s%d.pts" % j)).write_text("".join("%r %r %r\n" % tuple(float(v) for v in p) for p in pc))
                else:
                    np.save(folder / ("s%d.npy" % j), pc)
    common = ["--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root", str(tmp_path / "pc"), "--choice", "chair",
              "--batch_size", "2", "--seed", "1", "--save_dir", str(tmp_path / "res"), "--num_point", str(num_point), "--num_k", "4", "--ragged"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    done = subprocess.run([sys.executable, "-m", "pdgn_amd.train"] + common + ["--phase", "train", "--max_epoch", "1", "--snapshot", "1", "--min_points", "25"],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "ragged clouds, train split: 1 shapes dropped by --min_points 25; 4 shapes" in done.stdout, done.stdout[-2000:]
    ck = tmp_path / "ck" / "toy" / "PDGNet_v2"
    assert (ck / "1_chair_G.pth").exists() and (ck / "1_chair_D.pth").exists()
    log = (tmp_path / "ck" / "toy" / "log_info.txt").read_text().splitlines()
    assert log[0].startswith("Namespace(") and "ragged=True" in log[0] and "min_points=25" in log[0] and "resample_pool" not in log[0]
    assert sum(l.startswith("Epoch: [ 1]") for l in log) == 2                    # 4 of the 5 shapes of the one category, batches of 2
    out = train.main(common + ["--phase", "test", "--pretrain_model_G", "1_chair_G.pth", "--pretrain_model_D", "1_chair_D.pth"])
    assert os.path.basename(out).startswith("GEN_Ours_chair_")
    assert np.load(os.path.join(out, "out.npy")).shape == (n_test, num_point, 3)
    metrics = dict(l.split(": ") for l in open(os.path.join(out, "log.txt")).read().splitlines())
    for key in ("lgan_mmd-CD", "lgan_cov-CD", "1-NN-CD-acc", "jsd"):
        assert key in metrics, metrics
    assert all(np.isfinite(float(v)) for v in metrics.values()), metrics
