"""GPU: the mesh feeder -- pdgn_feed_batch_mesh and pdgn_sample_surface (csrc/feed.hip) called directly on guard-banded
buffers against their host mirror (tests/mesh_mirror.py) bit for bit, an fp64 geometry check that does not go through the mirror,
data.MeshFeeder inside PDGNTrainer.fit on the launch list, and the command line on a packed file and on an .obj directory.

The mesh set: S = 6 ragged shapes of 1, 4, 12, 37, 1000, 2 faces (the last with a degenerate face), |coordinates| in [2^-6, 2^6];
B = 4, N = 130 (no multiple of 4), sizes (8, 17, 64) -- B = 2 where three ranks have to share the six shapes."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feed_mirror as fm
import fps_mirror
import mesh_mirror as mm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 0.2
GUARD = 64                                                       # elements on either side of every output (a multiple of 4: 16-byte alignment kept)
SENTINEL, ISENTINEL = -12345.0, -777
INVALID = -1
B, N, SIZES = 4, 130, (8, 17, 64)
LENS = SIZES + (N,)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _set():
    """(the MeshSet on the host, on the device, its mirror arrays): built once, never written."""
    from pdgn_amd.meshes import MeshSet
    host = MeshSet.from_meshes(mm.ragged_meshes())
    return host, host.to(_dev()), mm.Arrays(host)


def _guarded(shape, dev, dtype=torch.float32):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL if dtype == torch.float32 else ISENTINEL, dtype=dtype, device=dev)
    return whole[GUARD:GUARD + n].view(shape), whole


def _guards_intact(whole):
    s = SENTINEL if whole.dtype == torch.float32 else ISENTINEL
    return bool((whole[:GUARD] == s).all()) and bool((whole[-GUARD:] == s).all())


def _raw(order, first=0, seed=5, t=0, row0=0, B=B, lens=LENS, rec=True, untouched=False, **over):
    """pdgn_feed_batch_mesh itself into guarded buffers -> (rc, [p1 .. p4, z1, z2] as numpy, face_rec or None).  over: replaces
    arguments by name (S V F verts faces face_off alias order_ptr p1 .. z2 face_rec: a tensor, or an int address -- 0 for NULL)."""
    from pdgn_amd import _lib
    _, ms, _ = _set()
    dev = ms.verts.device
    order = torch.as_tensor(np.asarray(order, dtype=np.int32)).to(dev)
    made = [_guarded((B, 3, r), dev) for r in lens] + [_guarded((B, 128), dev) for _ in range(2)]
    if rec:
        made.append(_guarded((B, sum(lens)), dev, torch.int32))
    a = dict(S=ms.S, V=ms.V, F=ms.F, verts=ms.verts, faces=ms.faces, face_off=ms.face_off, alias=ms.alias, order=order,
             face_rec=made[6][0] if rec else None)
    a.update(zip(("p1", "p2", "p3", "p4", "z1", "z2"), (v for v, _ in made[:6])))
    if "order_ptr" in over:
        a["order"] = over.pop("order_ptr")
    a.update(over)
    p = lambda x: x if isinstance(x, int) else _lib.ptr(x)
    rc = _lib.lib().pdgn_feed_batch_mesh(B, a["S"], a["V"], a["F"], lens[3], lens[0], lens[1], lens[2], p(a["verts"]), p(a["faces"]), p(a["face_off"]),
                                         p(a["alias"]), p(a["order"]), first, seed, t, row0, SIGMA, p(a["p1"]), p(a["p2"]), p(a["p3"]), p(a["p4"]),
                                         p(a["z1"]), p(a["z2"]), p(a["face_rec"]), _lib.stream_of(ms.verts))
    torch.cuda.synchronize()
    for _, whole in made:
        assert _guards_intact(whole)
        if untouched:
            assert bool((whole == (SENTINEL if whole.dtype == torch.float32 else ISENTINEL)).all())
    return rc, [v.cpu().numpy() for v, _ in made[:6]], made[6][0].cpu().numpy() if rec else None


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _fill(feeder, epoch, i):
    """feeder.fill into guarded buffers -> ([p1 .. p4], z1, z2) as numpy."""
    made = [_guarded(s, feeder.device) for s in feeder.shapes()[:4]] + [_guarded(feeder.shapes()[4], feeder.device) for _ in range(2)]
    views = [v for v, _ in made]
    feeder.fill(epoch, i, views[:4], views[4], views[5])
    torch.cuda.synchronize()
    for _, whole in made:
        assert _guards_intact(whole)
    out = [v.cpu().numpy() for v in views]
    return out[:4], out[4], out[5]


# ---------------------------------------------------------------------------- 8. bit-equality with the mirror
RAW_CASES = {
    "t>=2^32": dict(order=fm.epoch_order(5, 1, 6), first=2, t=(0xABCDEF << 32) | 0xFFFFFFFF, row0=7),
    "row0=2^32-B": dict(order=fm.epoch_order(5, 1, 6), first=1, t=3, row0=(1 << 32) - B),
    "clamped order": dict(order=[4, 4, -3, 99, 1, 5], first=0, t=1 << 32, row0=0),          # repeated and out-of-range entries
    "clamped order, first>0": dict(order=[0, 2, 7, -1, 4, 4], first=2, t=9, row0=4),
    "aligned, B=1": dict(order=fm.epoch_order(6, 2, 6), first=5, t=2, row0=3, B=1, lens=(8, 16, 64, 128)),
    "aligned": dict(order=fm.epoch_order(6, 2, 6), first=1, t=(1 << 32) + 2, row0=0, lens=(8, 16, 64, 128)),
}


@pytest.mark.parametrize("case", list(RAW_CASES))
def test_raw_calls_are_bit_equal_to_the_mirror(case):
    kw = dict(RAW_CASES[case])
    rc, got, rec = _raw(seed=77, **kw)
    assert rc == 0
    want, wrec = mm.feed_batch_mesh(_set()[2], kw["order"], kw["first"], kw.get("B", B), kw.get("lens", LENS), 77, kw["t"], kw["row0"])
    assert np.array_equal(rec, wrec)
    for k in range(4):
        assert _same(got[k], want[k]), k
    if kw["t"] >> 32:                                            # the high part of t is part of the counter
        _, low, _ = _raw(seed=77, **dict(kw, t=kw["t"] & 0xFFFFFFFF))
        assert all((got[k].reshape(len(got[k]), -1) != low[k].reshape(len(got[k]), -1)).any(axis=1).all() for k in range(4))


def test_feeder_batches_are_bit_equal_to_the_mirror():
    """Through data.MeshFeeder: one rank at B = 4, and rank 1 of 3 at B = 2 (three ranks share the six shapes)."""
    from pdgn_amd.data import MeshFeeder
    host, ms, _ = _set()
    for kw in (dict(batch_size=B), dict(batch_size=2, rank=1, world=3)):
        feeder = MeshFeeder(ms, sizes=SIZES, seed=9999, sigma=SIGMA, num_point=N, **kw)
        mirror = mm.MirrorMeshFeeder(host, sizes=SIZES, seed=9999, sigma=SIGMA, num_point=N, **kw)
        assert feeder._fn.__name__ == "pdgn_feed_batch_mesh" and feeder.batches_per_epoch == mirror.batches_per_epoch == 1
        assert feeder.shapes() == [(kw["batch_size"], 3, r) for r in LENS] + [(kw["batch_size"], 128)]
        for epoch in (1, 2, 40):
            reals, z1, z2 = _fill(feeder, epoch, 0)
            want, w1, w2 = mirror.batch(epoch, 0, np.float64)
            for k in range(4):
                assert _same(reals[k], want[k]), (kw, epoch, k)
            assert np.abs(z1 - w1).max() < 1e-5 and np.abs(z2 - w2).max() < 1e-5           # (byte-equal to pdgn_feed_batch's: below)


# ---------------------------------------------------------------------------- 9. geometry, independent of the mirror
def _geometry_holds(points, faces_rec, shape_ids):
    """points (R, n, 3) fp32, faces_rec (R, n) global faces, shape_ids (R): in fp64, every point lies in the plane of its recorded face
    and inside the triangle, both to within 4 ulp of the largest |coordinate| of the row's shape (four individually rounded operations
    on values of at most twice that size: e1 / e2, the two products and the two sums, together at most 4 ulp per coordinate); no
    recorded face is degenerate and every one belongs to the row's shape.  Returns the worst excess in ulp."""
    host, _, _ = _set()
    verts, faces, off = host.verts.numpy().astype(np.float64), host.faces.numpy().astype(np.int64), host.face_off.numpy()
    worst = 0.0
    for r, c in enumerate(shape_ids):
        gf = faces_rec[r].astype(np.int64)
        assert gf.min() >= off[c] and gf.max() < off[c + 1], (r, c)
        tri = verts[faces[gf]]
        v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        nrm = np.cross(e1, e2)
        twice_area = np.linalg.norm(nrm, axis=1)
        assert (twice_area > 0).all(), "a degenerate face was drawn"
        big = np.abs(verts[np.unique(faces[off[c]:off[c + 1]])]).max()
        ulp = 2.0 ** (np.floor(np.log2(big)) - 23)
        d = points[r].astype(np.float64) - v0
        plane = np.abs((d * nrm).sum(axis=1)) / twice_area
        # barycentric coordinates of the projection; coordinate i times the triangle's altitude over edge i = the distance from that edge
        g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
        b1, b2 = (d * e1).sum(1), (d * e2).sum(1)
        det = g11 * g22 - g12 * g12
        u, v = (g22 * b1 - g12 * b2) / det, (g11 * b2 - g12 * b1) / det
        alt = [twice_area / np.linalg.norm(e2, axis=1), twice_area / np.linalg.norm(e1, axis=1), twice_area / np.linalg.norm(e2 - e1, axis=1)]
        outside = np.maximum.reduce([-u * alt[0], -v * alt[1], -(1.0 - u - v) * alt[2], np.zeros_like(u)])
        worst = max(worst, float(plane.max() / ulp), float(outside.max() / ulp))
    return worst


def test_points_lie_on_their_recorded_faces():
    order = [0, 1, 2, 3, 4, 5]
    for first in (0, 2):
        rc, got, rec = _raw(order, first=first, seed=31, t=first)
        assert rc == 0
        pts = np.concatenate([g.transpose(0, 2, 1) for g in got[:4]], axis=1)        # (B, sum lens, 3): face_rec's column order
        worst = _geometry_holds(pts, rec, order[first:first + B])
        print("first %d: worst deviation %.3f ulp of the shape's largest |coordinate| (bound 4)" % (first, worst))
        assert worst <= 4.0
    assert len(np.unique(rec[2])) > 50                           # (row 2 is the 1000-face shape: many faces; row 3 the two-face one: one)
    assert (rec[3] == _set()[0].face_off[5].item()).all()


# ---------------------------------------------------------------------------- 10. noise, repeatability, guard bands
def test_noise_is_byte_equal_to_the_cloud_feeders_and_the_call_is_pure():
    from pdgn_amd import _lib
    dev = _dev()
    order = fm.epoch_order(5, 1, 6)
    clouds = torch.zeros(6, N, 3, device=dev)
    for t, row0 in ((11, 0), ((7 << 32) + 1, 70)):
        rc, a, rec = _raw(order, first=2, seed=77, t=t, row0=row0)
        rc2, b, rec2 = _raw(order, first=2, seed=77, t=t, row0=row0)                  # the same arguments: the same bytes
        rc3, c, none = _raw(order, first=2, seed=77, t=t, row0=row0, rec=False)       # face_rec = NULL: the same points
        assert rc == rc2 == rc3 == 0 and none is None
        for k in range(6):
            assert _same(a[k], b[k]) and _same(a[k], c[k]), k
        assert np.array_equal(rec, rec2)
        made = [_guarded((B, 3, r), dev) for r in LENS] + [_guarded((B, 128), dev) for _ in range(2)]
        rc = _lib.lib().pdgn_feed_batch(B, 6, N, *SIZES, _lib.ptr(clouds), _lib.ptr(torch.from_numpy(order).to(dev)), 2, 77, t, row0, SIGMA,
                                        *[_lib.ptr(v) for v, _ in made], _lib.stream_of(clouds))
        torch.cuda.synchronize()
        assert rc == 0
        assert _same(a[4], made[4][0].cpu().numpy()) and _same(a[5], made[5][0].cpu().numpy())
    other = {"seed": _raw(order, first=2, seed=78, t=11)[1], "t": _raw(order, first=2, seed=77, t=12)[1], "row": _raw(order, first=2, seed=77, t=11, row0=1)[1]}
    _, a, _ = _raw(order, first=2, seed=77, t=11)
    for what, c in other.items():                                # every row of every output draws something else
        for k in range(6):
            assert (a[k].reshape(B, -1) != c[k].reshape(B, -1)).any(axis=1).all(), (what, k)


# ---------------------------------------------------------------------------- 11. ranks and epochs
def test_ranks_compose_and_visits_differ_and_a_resumed_epoch_repeats():
    from pdgn_amd.data import MeshFeeder
    host, ms, _ = _set()
    W, b = 3, 2
    one = MeshFeeder(ms, b * W, SIZES, seed=9, sigma=SIGMA, num_point=N)
    ranks = [MeshFeeder(ms, b, SIZES, seed=9, rank=r, world=W, sigma=SIGMA, num_point=N) for r in range(W)]
    seen = {}
    for epoch in (1, 2):
        whole = _fill(one, epoch, 0)
        parts = [_fill(f, epoch, 0) for f in ranks]
        for k in range(4):
            assert _same(np.concatenate([p[0][k] for p in parts]), whole[0][k]), (epoch, k)
        for k in (1, 2):
            assert _same(np.concatenate([p[k] for p in parts]), whole[k])
        for row, c in enumerate(fm.epoch_order(9, epoch, 6).tolist()):
            seen.setdefault(c, []).append([whole[0][k][row] for k in range(4)])
    for c, (first, second) in seen.items():                      # a shape visited twice shows two different clouds, at every resolution
        for k in range(4):
            assert not np.array_equal(first[k], second[k]), (c, k)
    # two batches per epoch; iteration 1 of epoch 2 from a fresh feeder (a resumed run) is what the feeder that ran through 1 and 2 wrote
    run = MeshFeeder(ms, 3, SIZES, seed=21, sigma=SIGMA, num_point=N)
    assert run.batches_per_epoch == 2
    fed = {(e, i): _fill(run, e, i) for e in (1, 2) for i in (0, 1)}
    resumed = _fill(MeshFeeder(ms, 3, SIZES, seed=21, sigma=SIGMA, num_point=N), 2, 1)
    for k in range(4):
        assert _same(resumed[0][k], fed[(2, 1)][0][k]) and not np.array_equal(resumed[0][k], fed[(1, 1)][0][k]), k
    assert _same(resumed[1], fed[(2, 1)][1]) and _same(resumed[2], fed[(2, 1)][2])
    mirror = mm.MirrorMeshFeeder(host, 3, SIZES, seed=21, sigma=SIGMA, num_point=N)
    for k in range(4):
        assert _same(resumed[0][k], mirror.batch(2, 1)[0][k]), k


# ---------------------------------------------------------------------------- 12. pdgn_sample_surface
def test_sample_surface_is_the_mirrors_and_apart_from_training_draws():
    host, ms, arrays = _set()
    for n in (1, 63, 256):
        for draw in (0, 1, (5 << 32) | 1):
            got, rec = ms.sample(n, 77, draw, return_faces=True)
            torch.cuda.synchronize()
            want, wrec = mm.sample_surface(arrays, n, 77, draw)
            assert tuple(got.shape) == (6, n, 3) and _same(got.cpu().numpy(), want) and np.array_equal(rec.cpu().numpy(), wrec), (n, draw)
    a, rec = ms.sample(256, 77, 0, return_faces=True)
    assert _same(ms.sample(256, 77).cpu().numpy(), a.cpu().numpy())                   # draw defaults to 0; pure
    b = ms.sample(256, 77, 1)
    c = ms.sample(256, 78, 0)
    a, b, c = a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()
    for s in range(6):
        assert not np.array_equal(a[s], b[s]) and not np.array_equal(a[s], c[s]), s
    worst = _geometry_holds(a, rec.cpu().numpy(), range(6))
    print("sample_surface: worst deviation %.3f ulp (bound 4)" % worst)
    assert worst <= 4.0
    # tag separation: the training draws of shape s at the same seed, global row s, iteration 0 = draw 0 use other streams
    for first in (0, 2):
        _, train, _ = _raw([0, 1, 2, 3, 4, 5], first=first, seed=77, t=0, row0=first, lens=(64, 128, 256, 256))
        for row in range(B):
            mine = set(map(tuple, a[first + row].tolist()))
            for k in range(4):
                theirs = set(map(tuple, train[k][row].T.tolist()))
                assert not (mine & theirs), (first, row, k)
    # guard bands and the unaligned tail (n = 63: scalar stores), called directly
    from pdgn_amd import _lib
    out, whole = _guarded((6, 63, 3), ms.verts.device)
    frec, fwhole = _guarded((6, 63), ms.verts.device, torch.int32)
    rc = _lib.lib().pdgn_sample_surface(6, 63, _lib.ptr(ms.verts), _lib.ptr(ms.faces), _lib.ptr(ms.face_off), _lib.ptr(ms.alias), 77, 0,
                                        _lib.ptr(out), _lib.ptr(frec), _lib.stream_of(ms.verts))
    torch.cuda.synchronize()
    assert rc == 0 and _guards_intact(whole) and _guards_intact(fwhole)
    assert _same(out.cpu().numpy(), mm.sample_surface(arrays, 63, 77, 0)[0])


# ---------------------------------------------------------------------------- 13. refusals
def test_invalid_arguments_are_refused_before_any_launch():
    from pdgn_amd import _lib
    _, ms, _ = _set()
    order = fm.epoch_order(5, 1, 6)
    assert _raw(order)[0] == 0
    odd = ms.alias.data_ptr() + 4                                # 4-byte aligned, not 8
    null = 0
    bad_cases = [dict(B=0), dict(lens=(8, 0, 64, N)), dict(lens=(8, 17, 64, 0)), dict(first=-1), dict(first=6 - B + 1), dict(row0=-1),
                 dict(row0=(1 << 32) - B + 1), dict(order_ptr=null), dict(p1=null), dict(p4=null), dict(z1=null), dict(z2=null),   # pdgn_feed_batch's own
                 dict(verts=null), dict(faces=null), dict(face_off=null), dict(alias=null),                                         # null mesh pointers
                 dict(S=0), dict(S=-1), dict(F=(1 << 31) // 3 + 1), dict(V=(1 << 31) // 3 + 1), dict(alias=odd)]
    for bad in bad_cases:
        assert _raw(order, untouched=True, **bad)[0] == INVALID, bad
    z_odd = torch.zeros(B * 128 + 4, device=ms.verts.device)[1:]
    assert _raw(order, untouched=True, z1=z_odd.data_ptr())[0] == INVALID                  # z1 not 16-byte aligned
    L = _lib.lib()
    out, whole = _guarded((6, 16, 3), ms.verts.device)
    args = lambda **o: [o.get("S", 6), o.get("n", 16)] + [o.get(k, _lib.ptr(getattr(ms, k))) for k in ("verts", "faces", "face_off", "alias")] + \
        [7, 0, o.get("out", _lib.ptr(out)), None, _lib.stream_of(ms.verts)]
    for bad in (dict(S=0), dict(n=0), dict(verts=None), dict(faces=None), dict(face_off=None), dict(alias=None), dict(alias=odd), dict(out=None)):
        assert L.pdgn_sample_surface(*args(**bad)) == INVALID, bad
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all())
    assert L.pdgn_sample_surface(*args()) == 0
    torch.cuda.synchronize()
    assert _guards_intact(whole) and not bool((out == SENTINEL).any())


# ---------------------------------------------------------------------------- 14. MeshFeeder inside fit
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


def test_fit_feeds_the_launch_list_fresh_surface_samples():
    """B = 2 on the default trainer (2048 points, sub-resolutions 256 512 1024: the generator of the existing fit tests), the launch list
    captured once: an epoch from the mesh feeder, one with subsample="fps" behind it, one from the default cloud feeder."""
    from pdgn_amd import pointops
    from pdgn_amd.data import BatchFeeder, MeshFeeder
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    dev = _dev()
    host, ms, _ = _set()
    b, n, sizes = 2, 2048, (256, 512, 1024)
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    tr.capture_list(synthetic_batch(b, dev), noise(b, dev), noise(b, dev))
    static = [r.data_ptr() for r in tr._static["reals"]] + [tr._static["z1"].data_ptr(), tr._static["z2"].data_ptr()]
    mirror = mm.MirrorMeshFeeder(host, b, sizes, seed=77, num_point=n)
    feeder = RecordingFeeder(MeshFeeder(ms, b, sizes, seed=77, num_point=n))
    lines = []
    assert tr.fit(feeder, 1, log=lines.append) == 1
    torch.cuda.synchronize()
    assert [(e, i) for e, i, *_ in feeder.fed] == [(1, 0), (1, 1), (1, 2)] and len(lines) == 3
    assert all(f[5] == static for f in feeder.fed)              # written straight into the list's static buffers
    for epoch, i, reals, z1, z2, _ in feeder.fed:                # after iteration i: the mirror's batch i
        want, w1, w2 = mirror.batch(epoch, i, np.float64)
        for k in range(4):
            assert _same(reals[k].cpu().numpy(), want[k]), (i, k)
        assert np.abs(z1.cpu().numpy() - w1).max() < 1e-5 and np.abs(z2.cpu().numpy() - w2).max() < 1e-5
    for line in lines:
        vals = [float(tok.rstrip(",")) for tok in line.split("time:")[1].split()[2:][1::2]]
        assert len(vals) == 6 and all(np.isfinite(v) for v in vals), line
    # subsample="fps": p4 is the mesh launch's, p1 .. p3 nested prefixes of a farthest-point order of it
    fps = RecordingFeeder(MeshFeeder(ms, b, sizes, seed=77, num_point=n, subsample="fps"))
    assert tr.fit(fps, 1) == 1
    torch.cuda.synchronize()
    for (epoch, i, reals, z1, z2, _), plain in zip(fps.fed, feeder.fed):
        assert torch.equal(reals[3], plain[2][3]) and torch.equal(z1, plain[3]) and torch.equal(z2, plain[4])
        start = fps_mirror.start_indices(77, i, np.arange(b), n)                          # (epoch 1: the global iteration is i)
        order = pointops.fps_order(reals[3].transpose(1, 2).contiguous(), sizes[2], start=torch.from_numpy(start.astype(np.int32)).to(dev)).long()
        for k, r in enumerate(sizes):
            want = torch.gather(reals[3], 2, order[:, None, :r].expand(b, 3, r))
            assert torch.equal(reals[k], want), (i, k)
            assert torch.equal(reals[k], reals[2][:, :, :r])
    # the default cloud feeder on the same list: the bytes of its mirror, as before
    clouds = np.random.default_rng(3).standard_normal((5, n, 3)).astype(np.float32)
    plain = RecordingFeeder(BatchFeeder(torch.from_numpy(clouds).to(dev), b, sizes, seed=77))
    assert plain.inner._fn.__name__ == "pdgn_feed_batch"
    assert tr.fit(plain, 1) == 1
    torch.cuda.synchronize()
    cm = fm.MirrorFeeder(clouds, b, sizes, seed=77)
    for epoch, i, reals, z1, z2, _ in plain.fed:
        want, w1, w2 = cm.batch(epoch, i, np.float64)
        for k in range(4):
            assert _same(reals[k].cpu().numpy(), want[k]), (i, k)
        assert np.abs(z1.cpu().numpy() - w1).max() < 1e-5
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 15. command line
def _write_obj(path, verts, faces):
    with open(path, "w") as f:
        f.write("# written by the test\n")
        for v in verts:
            f.write("v %r %r %r\n" % tuple(float(x) for x in v))
        for t in faces:
            f.write("f %d//1 %d//1 %d//1\n" % tuple(int(i) + 1 for i in t))


@pytest.mark.parametrize("form", ["packed", "directory"])
def test_cli_trains_and_tests_on_meshes(tmp_path, form):
    """Two categories, 5 / 2 / 2 shapes per split, --num_point 64: one epoch of --phase train (the first log line and the checkpoints),
    then --phase test (out.npy and the metric lines), and --resample_pool refused with its reason."""
    from pdgn_amd import meshes
    from pdgn_amd.data import cate_to_synsetid
    rng = np.random.default_rng(15)
    for cate in ("chair", "lamp"):
        for split, count in (("train", 5), ("val", 2), ("test", 2)):
            (tmp_path / "obj" / cate_to_synsetid[cate] / split).mkdir(parents=True)
            for j in range(count):
                _write_obj(tmp_path / "obj" / cate_to_synsetid[cate] / split / ("m%d.obj" % j), *mm.random_mesh(int(rng.integers(4, 40)), rng))
    root = tmp_path / "obj"
    if form == "packed":
        meshes.pack(str(root), str(tmp_path / "packed.npz"))
        root = tmp_path / "packed.npz"
    common = ["--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root", str(root), "--choice", "chair",
              "--batch_size", "2", "--seed", "1", "--save_dir", str(tmp_path / "res"), "--num_point", "64", "--num_k", "4"]
    from pdgn_amd import train
    with pytest.raises(SystemExit, match="--resample_pool.*meshes.*surface"):                  # refused before anything is trained or logged
        train.main(common + ["--phase", "train", "--max_epoch", "1", "--resample_pool", "100"])
    assert not (tmp_path / "ck" / "toy" / "log_info.txt").exists()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    done = subprocess.run([sys.executable, "-m", "pdgn_amd.train"] + common + ["--phase", "train", "--max_epoch", "1", "--snapshot", "1"],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    ck = tmp_path / "ck" / "toy" / "PDGNet_v2"
    assert (ck / "1_chair_G.pth").exists() and (ck / "1_chair_D.pth").exists()
    log = (tmp_path / "ck" / "toy" / "log_info.txt").read_text().splitlines()
    assert log[0].startswith("Namespace(") and "resample_pool" not in log[0] and "subsample" not in log[0]
    assert sum(l.startswith("Epoch: [ 1]") for l in log) == 2                    # 5 shapes of the one category, batches of 2
    out = train.main(common + ["--phase", "test", "--pretrain_model_G", "1_chair_G.pth", "--pretrain_model_D", "1_chair_D.pth"])
    assert os.path.basename(out).startswith("GEN_Ours_chair_")
    assert np.load(os.path.join(out, "out.npy")).shape == (2, 64, 3)
    metrics = dict(l.split(": ") for l in open(os.path.join(out, "log.txt")).read().splitlines())
    assert "jsd" in metrics and "1-NN-CD-acc" in metrics and all(np.isfinite(float(v)) for v in metrics.values()), metrics
