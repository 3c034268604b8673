"""Consistent normal orientation on the device: pdgn_orient_normals bit for bit against its numpy mirror
(tests/orient_mirror.py) -- normals, parents and all four counters -- on estimated and on hostile inputs, under ties, on isolated points;
repeatability, the in-place call, the optional outputs, the refusals, the Python wrappers and the export command line."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import normals_mirror as nm
import orient_mirror as om

pytestmark = pytest.mark.gpu
F = np.float32
# (b, n, k): the smallest call; fewer points than a wave; one past a wave; one past half a workgroup; the k limit with a tail past the
# workgroup's stride of 512; more clouds than the first pass of workgroups at the level-1 shape; several points per thread; the n limit,
# where the launch asks for more LDS than it gets unasked.
SHAPES = [(1, 1, 1), (2, 3, 3), (3, 65, 8), (2, 257, 16), (1, 1000, 64), (35, 256, 16), (4, 2048, 16), (2, 4096, 8)]
SENTINEL = 7.0


def _dev():
    return torch.device("cuda:0")


def _call(x, idx, g, parent=True, stats=True, inplace=False, work=True, b=None, n=None, k=None):
    """The raw entry point on device tensors -> (rc, normals, parent or None, stats or None), sentinel-filled before the call."""
    from pdgn_amd import _lib
    L = _lib.lib()
    B, N, K = idx.shape
    out = g.clone() if inplace else torch.full((B, N, 3), SENTINEL, dtype=torch.float32, device=x.device)
    src = out if inplace else g
    par = torch.full((B, N), 77, dtype=torch.int32, device=x.device) if parent else None
    st = torch.full((B, 4), 77, dtype=torch.int32, device=x.device) if stats else None
    ints = int(L.pdgn_orient_workspace_ints(B, N, K))
    assert ints == B * N * K
    ws = torch.empty((ints,), dtype=torch.int32, device=x.device) if work else None
    rc = L.pdgn_orient_normals(B if b is None else b, N if n is None else n, K if k is None else k, _lib.ptr(x), _lib.ptr(idx),
                               _lib.ptr(src), _lib.ptr(out), _lib.ptr(par), _lib.ptr(st), _lib.ptr(ws), _lib.stream_of(x))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), None if par is None else par.cpu().numpy(), None if st is None else st.cpu().numpy()


def _same(got, want):
    return got[0] == 0 and nm.same_bits(got[1], want[0]) and np.array_equal(got[2], want[1]) and np.array_equal(got[3], want[2])


@pytest.mark.parametrize("b,n,k", SHAPES)
def test_the_kernel_equals_the_mirror_on_estimated_normals_and_knn_lists(b, n, k):
    from pdgn_amd import pointops
    x = np.random.default_rng(40 + n).standard_normal((b, n, 3)).astype(F)
    xd = torch.from_numpy(x).to(_dev())
    kq = min(k, n)
    idx = pointops.knnquery(kq, xd, xd)
    g = pointops.estimate_normals(xd, idx=idx)
    want = om.orient(x, g.cpu().numpy(), idx.cpu().numpy())
    got = _call(xd, idx, g)
    assert _same(got, want)
    assert (want[2][:, 3] == 0).all() and (want[2][:, 0] >= 1).all() and (n < 65 or want[2][:, 1].sum() > 0)
    # the wrappers return what the entry point wrote
    py = pointops.orient_normals(xd, g, idx=idx, return_tree=True)
    assert not py[0].requires_grad and _same((0,) + tuple(t.cpu().numpy() for t in py), want)
    assert nm.same_bits(pointops.orient_normals(xd, g, kq).cpu().numpy(), want[0])
    assert nm.same_bits(pointops.estimate_normals(xd, kq, orient="consistent").cpu().numpy(), want[0])
    n2, e2 = pointops.estimate_normals(xd, idx=idx, orient="consistent", return_eig=True)
    assert nm.same_bits(n2.cpu().numpy(), want[0]) and nm.same_bits(e2.cpu().numpy(), pointops.estimate_normals(xd, idx=idx, return_eig=True)[1].cpu().numpy())


@pytest.mark.parametrize("b,n,k", SHAPES)
def test_the_kernel_equals_the_mirror_on_random_lists_with_repeats_and_poison(b, n, k):
    """Random indices (repeats and self entries are the rule, and every point gets one self entry for certain), one entry of the whole
    call outside its cloud and, where the cloud has more than two points, one NaN normal and one infinite coordinate."""
    rng = np.random.default_rng(50 + n)
    x = rng.standard_normal((b, n, 3)).astype(F)
    g = rng.standard_normal((b, n, 3))
    g = (g / np.linalg.norm(g, axis=2, keepdims=True)).astype(F)
    idx = rng.integers(0, n, size=(b, n, k)).astype(np.int32)
    idx[:, :, 0] = np.arange(n, dtype=np.int32)[None, :]
    idx[b - 1, n // 2, k - 1] = (n, -1, n + 5, 2 ** 31 - 1)[n % 4]
    if n > 2:
        g[0, 1, 2], x[b - 1, n - 1, 0] = np.nan, np.inf
    want = om.orient(x, g, idx)
    assert n <= 2 or want[2][:, 3].sum() == 2
    got = _call(torch.from_numpy(x).to(_dev()), torch.from_numpy(idx).to(_dev()), torch.from_numpy(g).to(_dev()))
    assert _same(got, want)
    assert np.array_equal(got[2] == -2, ~(np.isfinite(x).all(axis=2) & np.isfinite(g).all(axis=2)))


def test_ties_on_a_planar_lattice_go_the_mirrors_way():
    """23 x 29 points in the plane z = 0, normals +-(0, 0, 1) in a seeded mix: every weight is 0 and every point as high as any other, so
    the tie rules decide every round and the root."""
    ii, jj = np.meshgrid(np.arange(23), np.arange(29), indexing="ij")
    x = np.stack([ii.ravel(), jj.ravel(), np.zeros(ii.size)], axis=1).astype(F)[None]
    n = x.shape[1]
    g = np.zeros((1, n, 3), F)
    g[0, :, 2] = np.where(np.random.default_rng(3).integers(0, 2, n) == 1, 1.0, -1.0)
    idx = nm.knn_indices(x[0], 9)[None]
    want = om.orient(x, g, idx)
    assert want[1][0, 0] == -1 and (want[0][0, :, 2] == 1).all() and tuple(want[2][0]) == (1, int((g[0, :, 2] < 0).sum()), 0, 0)
    got = _call(torch.from_numpy(x).to(_dev()), torch.from_numpy(idx).to(_dev()), torch.from_numpy(g).to(_dev()))
    assert _same(got, want)


def test_isolated_points_are_n_components_each_oriented_by_the_z_rule():
    n = 700
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, n, 3)).astype(F)
    g = rng.standard_normal((2, n, 3)).astype(F)
    g[0, :5, 2] = (0.0, -0.0, 1.0, -1.0, -1e-30)
    idx = np.broadcast_to(np.arange(n, dtype=np.int32)[None, :, None], (2, n, 1)).copy()
    got = _call(torch.from_numpy(x).to(_dev()), torch.from_numpy(idx).to(_dev()), torch.from_numpy(g).to(_dev()))
    assert _same(got, om.orient(x, g, idx))
    assert (got[2] == -1).all() and (got[3][:, 0] == n).all() and (got[3][:, 2:] == 0).all()
    flip = g[:, :, 2] < 0
    assert nm.same_bits(got[1], np.where(flip[:, :, None], -g, g)) and np.array_equal(got[3][:, 1], flip.sum(axis=1))
    assert not np.signbit(got[1][0, 0, 2]) and np.signbit(got[1][0, 1, 2])     # (neither zero is below zero: both keep their bits)


def test_two_calls_agree_in_place_equals_out_of_place_and_outputs_may_be_null():
    from pdgn_amd import pointops
    x, _ = om.torus(1500, 7)
    xd = torch.from_numpy(np.stack([x, x[::-1].copy()])).to(_dev())
    idx = pointops.knnquery(12, xd, xd)
    g = pointops.estimate_normals(xd, idx=idx)
    first = _call(xd, idx, g)
    again = _call(xd, idx, g)
    assert first[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], again[1:]))
    inplace = _call(xd, idx, g, inplace=True)
    assert inplace[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], inplace[1:]))
    for kw in (dict(parent=False), dict(stats=False), dict(parent=False, stats=False)):
        rc, out, par, st = _call(xd, idx, g, **kw)
        assert rc == 0 and out.tobytes() == first[1].tobytes()
        assert (par is None or np.array_equal(par, first[2])) and (st is None or np.array_equal(st, first[3]))


def test_every_refusal_writes_nothing():
    from pdgn_amd import _lib, pointops
    xd = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 40, 3)).astype(F)).to(_dev())
    idx = pointops.knnquery(8, xd, xd)
    g = pointops.estimate_normals(xd, idx=idx)
    for kw in (dict(b=0), dict(b=-1), dict(n=0), dict(n=4097), dict(k=0), dict(k=65), dict(b=1 << 20, n=257), dict(work=False)):
        rc, out, par, st = _call(xd, idx, g, **kw)
        assert rc == -1 and (out == SENTINEL).all() and (par == 77).all() and (st == 77).all(), kw
    L = _lib.lib()
    for shape in ((0, 40, 8), (2, 4097, 8), (2, 40, 65), (2, 0, 8), (2, 40, 0)):
        assert L.pdgn_orient_workspace_ints(*shape) == -1
    assert L.pdgn_orient_workspace_ints(2, 4096, 64) == 2 * 4096 * 64
    out = torch.full((2, 40, 3), SENTINEL, device=_dev())
    par = torch.full((2, 40), 77, dtype=torch.int32, device=_dev())
    st = torch.full((2, 4), 77, dtype=torch.int32, device=_dev())
    ws = torch.empty((2 * 40 * 8,), dtype=torch.int32, device=_dev())
    p = _lib.ptr
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 2)
    good = [p(xd), p(idx), p(g), p(out), p(par), p(st), p(ws)]
    for slot in range(7):
        for bad in ([None] if slot not in (4, 5) else []) + [odd((xd, idx, g, out, par, st, ws)[slot])]:
            args = list(good)
            args[slot] = bad
            assert L.pdgn_orient_normals(2, 40, 8, *args, _lib.stream_of(xd)) == -1, (slot, bad)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (par == 77).all() and (st == 77).all()
    for bad in (dict(k=41), dict(k=0), dict(idx=idx[:, :39].contiguous()), dict(idx=idx.long())):
        with pytest.raises((ValueError, TypeError)):
            pointops.orient_normals(xd, g, **bad)
    with pytest.raises(ValueError):
        pointops.orient_normals(xd, g[:, :39].contiguous(), idx=idx)
    with pytest.raises(ValueError):
        pointops.estimate_normals(xd, 8, orient="inward")
    with pytest.raises(ValueError):
        pointops.estimate_normals(torch.zeros(1, 4097, 3, device=_dev()), 8, orient="consistent")


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    count = int([l for l in head.decode("ascii").splitlines() if l.startswith("element vertex")][0].split()[-1])
    return np.array(struct.unpack("<%df" % (6 * count), body), dtype=F).reshape(count, 6)


def test_the_export_command_orients_tori_consistently(tmp_path, capsys):
    from pdgn_amd import export
    clouds, truths = zip(*(om.torus(1024, seed) for seed in (0, 1, 2)))
    np.save(tmp_path / "torus.npy", np.stack(clouds))
    out = export.main([str(tmp_path / "torus.npy"), "-o", str(tmp_path / "plys"), "--normals", "16", "--orient", "consistent"])
    assert "(3 components, " in capsys.readouterr().out
    for i, (x, truth) in enumerate(zip(clouds, truths)):
        rows = _read_ply("%s/cloud_%d.ply" % (out, i))
        assert nm.same_bits(rows[:, :3], x)
        assert ((rows[:, 3:].astype(np.float64) * truth).sum(axis=1) > 0).all()
    # the centroid heuristic on the same file points a fifth of them the wrong way
    out = export.main([str(tmp_path / "torus.npy"), "-o", str(tmp_path / "outward"), "--normals", "16", "--orient", "outward", "--count", "1"])
    rows = _read_ply("%s/cloud_0.ply" % out)
    assert ((rows[:, 3:].astype(np.float64) * truths[0]).sum(axis=1) <= 0).sum() >= 0.2 * 1024
