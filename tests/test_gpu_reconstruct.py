"""Surface reconstruction on the device: pdgn_imls_grid bit for bit against its numpy mirror
(tests/reconstruct_mirror.py), NaN patterns included, with the culling on and off, where it skips everything, nearly everything and nothing,
and on points built to lie within a few ulps of the distance h from brick corners; pdgn_surface_nets_count / _emit bit for bit on those
fields and on synthetic ones; repeatability, the refusals, the Python wrappers, the export command line and the way back to a MeshSet."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import orient_mirror as om
import reconstruct_mirror as rm

pytestmark = pytest.mark.gpu
F = np.float32
# (b, n, R): one point and one cell; a few points and R past one brick; one point past a wave of staged points and R past the workgroup's
# cube of 8; one past 256 and three cubes with a tail; n past two staging chunks of 512 (with a tail) and R = 4 cubes + 1; four whole chunks
SHAPES = [(1, 1, 2), (2, 3, 5), (1, 65, 9), (3, 257, 17), (2, 1100, 33), (1, 2048, 40)]
REGIMES = ("none", "some", "all")
SENTINEL = 7.0


def _dev():
    return torch.device("cuda:0")


KINDS = ("gauss", "sphere", "torus")


def _cloud(kind, n, c):
    """Cloud c of a batch: Gaussian points with random unit normals, the Fibonacci sphere (of radius 1, 0.8, 0.6), or the torus of radii
    1 and 0.4 with analytic normals (seed c)."""
    if kind == "gauss":
        rng = np.random.default_rng(1000 + 7 * n + c)
        g = rng.standard_normal((n, 3))
        return rng.standard_normal((n, 3)).astype(F), (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(F)
    if kind == "sphere":
        return rm.fibonacci_sphere(n, 1.0 - 0.2 * c)
    x, truth = om.torus(n, c)
    return x, truth.astype(F)


def _case(shape_index, kind, regime):
    """-> x (b,n,3), g (b,n,3), grid (b,5): every cloud of the batch of the one kind; the box of every cloud with a margin of a tenth,
    and h by regime: half a voxel (hardly a node within h of a point), the radius at which n balls hold a tenth of the grid's volume (at
    least 0.8 voxels), four times the cube's side."""
    b, n, R = SHAPES[shape_index]
    xs, gs, grid = [], [], []
    for c in range(b):
        x, g = _cloud(kind, n, c)
        lo, hi = x.astype(np.float64).min(axis=0), x.astype(np.float64).max(axis=0)
        half = 0.6 * max(float((hi - lo).max()), 0.5)
        voxel = 2 * half / (R - 1)
        h = {"none": 0.5 * voxel, "some": voxel * max(0.8, (0.1 * R ** 3 * 3 / (4 * np.pi * n)) ** (1 / 3)), "all": 8 * half}[regime]
        xs.append(x), gs.append(g)
        grid.append(np.concatenate([(lo + hi) / 2 - half, [voxel, 1.0 / (h * h)]]).astype(F))
    return np.stack(xs), np.stack(gs), np.stack(grid)


def _field_raw(x, g, grid, R, cull=True, **bad):
    """The raw entry point -> (rc, field (b,R,R,R) numpy), the output sentinel-filled before the call."""
    from pdgn_amd import _lib
    L = _lib.lib()
    b, n, _ = x.shape
    xd, gd, grd = (torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) for a in (x, g, grid))
    host = np.ascontiguousarray(bad.pop("host", grid), dtype=F)
    out = torch.full((b, R, R, R), SENTINEL, dtype=torch.float32, device=_dev())
    rc = L.pdgn_imls_grid(bad.pop("call_b", b), bad.pop("call_n", n), bad.pop("call_R", R), _lib.ptr(xd), _lib.ptr(gd), _lib.ptr(grd),
                          host.ctypes.data_as(ctypes.c_void_p), bad.pop("call_cull", 1 if cull else 0), _lib.ptr(out), _lib.stream_of(xd))
    torch.cuda.synchronize()
    assert not bad
    return rc, out.cpu().numpy()


def _nets_raw(field, grid4):
    """count, torch.cumsum, emit through the raw entry points -> (verts, faces, vert_off, face_off, stats) numpy."""
    from pdgn_amd import _lib
    L = _lib.lib()
    b, R = field.shape[0], field.shape[1]
    fd = torch.from_numpy(np.ascontiguousarray(field)).to(_dev())
    grd = torch.from_numpy(np.ascontiguousarray(grid4, dtype=F)).to(_dev())
    host = np.ascontiguousarray(grid4, dtype=F)
    vflag = torch.full((b, R ** 3), 77, dtype=torch.int32, device=_dev())
    qcnt = torch.full((b, R ** 3), 77, dtype=torch.int32, device=_dev())
    stats = torch.full((b, 4), 77, dtype=torch.int32, device=_dev())
    assert L.pdgn_surface_nets_count(b, R, _lib.ptr(fd), _lib.ptr(vflag), _lib.ptr(qcnt), _lib.ptr(stats), _lib.stream_of(fd)) == 0
    st = stats.cpu().numpy()
    vert_off = np.concatenate([[0], np.cumsum(st[:, 0])]).astype(np.int32)
    face_off = np.concatenate([[0], np.cumsum(st[:, 1])]).astype(np.int32)
    V, Fc = int(vert_off[-1]), int(face_off[-1])
    verts = torch.full((V + 1, 3), SENTINEL, dtype=torch.float32, device=_dev())           # one guard row each: the capacity is exact
    faces = torch.full((Fc + 1, 3), -5, dtype=torch.int32, device=_dev())
    vscan, qscan = torch.cumsum(vflag, dim=1, dtype=torch.int32), torch.cumsum(qcnt, dim=1, dtype=torch.int32)
    vo, fo = torch.from_numpy(vert_off).to(_dev()), torch.from_numpy(face_off).to(_dev())
    rc = L.pdgn_surface_nets_emit(b, R, _lib.ptr(fd), _lib.ptr(grd), host.ctypes.data_as(ctypes.c_void_p), _lib.ptr(vflag), _lib.ptr(vscan),
                                  _lib.ptr(qcnt), _lib.ptr(qscan), _lib.ptr(vo), _lib.ptr(fo), V, Fc, V, Fc, _lib.ptr(verts), _lib.ptr(faces),
                                  _lib.stream_of(fd))
    torch.cuda.synchronize()
    assert rc == 0 and (verts[V] == SENTINEL).all() and (faces[Fc] == -5).all()
    return verts[:V].cpu().numpy(), faces[:Fc].cpu().numpy(), vert_off, face_off, st


def _nets_equal(got, want):
    return all(rm.bits_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, want))


def _check_nets(field, grid):
    from pdgn_amd import reconstruct
    want = rm.surface_nets(field, grid[:, :3], grid[:, 3])
    got = _nets_raw(field, grid[:, :4])
    assert _nets_equal(got, want), (got[4], want[4])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    py = reconstruct.surface_nets(t(field), t(grid[:, :3]), t(grid[:, 3]))
    assert _nets_equal([a.cpu().numpy() for a in py], want)        # the wrapper returns what the raw calls wrote
    return want


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape_index", range(len(SHAPES)))
def test_the_field_and_its_mesh_equal_the_mirror(shape_index, kind, regime):
    from pdgn_amd import _lib, reconstruct
    b, n, R = SHAPES[shape_index]
    chunk = _lib.lib().pdgn_imls_chunk()
    assert chunk == 512 and sorted(s[1] // chunk for s in SHAPES) == [0, 0, 0, 0, 2, 4]         # the counts cross the staging chunk
    x, g, grid = _case(shape_index, kind, regime)
    want = rm.field(x, g, grid[:, :3], grid[:, 3], grid[:, 4], R)  # the plain statement: every live point at every node
    share = float((~np.isnan(want)).mean())
    print(SHAPES[shape_index], kind, regime, "valid share %.3f" % share)
    if regime == "all":
        assert share == 1.0
    elif regime == "none":
        assert share < 0.1
    elif n >= 3:                                                    # "about 10 %": not a copy of "none", and far from "all"
        assert 0.02 < share < 0.3
    for cull in (True, False):
        rc, got = _field_raw(x, g, grid, R, cull=cull)
        assert rc == 0 and rm.bits_equal(got, want), cull
    t = lambda a: torch.from_numpy(a).to(_dev())
    for cull in (True, False):
        py = reconstruct.imls_grid(t(x), t(g), t(grid[:, :3].copy()), t(grid[:, 3].copy()), t(grid[:, 4].copy()), R, cull=cull)
        assert not py.requires_grad and rm.bits_equal(py.cpu().numpy(), want)
    stats = _check_nets(want, grid)[4]
    assert np.array_equal(stats[:, 3], np.isnan(want).reshape(b, -1).sum(axis=1))


def test_points_within_a_few_ulps_of_h_from_brick_corners_are_culled_exactly():
    """R = 17 on a grid whose node positions are not exact in binary; every point sits at the distance h, give or take three ulps per
    coordinate, from a brick's lowest corner, in a direction that leaves the brick: the box test has to keep or drop it as the nodes' own
    t does."""
    R, rng = 17, np.random.default_rng(11)
    origin, voxel = np.array([-0.7, -0.9, -1.1], F), F(0.1371)
    h = 1.5 * float(voxel)
    inv = F(1.0 / (h * h))
    p = rm.axis_positions(origin, voxel, R).astype(np.float64)     # the grid's own fp32 node positions
    pts = []
    for _ in range(700):
        corner = p[4 * rng.integers(1, 4, 3), np.arange(3)]        # a brick's lowest corner
        d = np.abs(rng.standard_normal(3)) * (rng.random(3) < 0.6)
        d = np.array([1.0, 0.0, 0.0])[rng.permutation(3)] if not d.any() else d
        q = (corner - h * d / np.linalg.norm(d)).astype(F)
        for _ in range(int(rng.integers(0, 4))):
            q = np.nextafter(q, np.where(rng.random(3) < 0.5, F(np.inf), F(-np.inf)).astype(F))
        pts.append(q)
    x = np.stack(pts)[None]
    g = rng.standard_normal(x.shape)
    g = (g / np.linalg.norm(g, axis=2, keepdims=True)).astype(F)
    grid = np.concatenate([origin, [voxel, inv]]).astype(F)[None]
    want = rm.field(x, g, grid[:, :3], grid[:, 3], grid[:, 4], R, cull=False)
    skip = rm.brick_skips(x[0], origin, voxel, inv, R)
    assert 0.05 < skip.mean() < 0.999 and rm.bits_equal(rm.field(x, g, grid[:, :3], grid[:, 3], grid[:, 4], R, cull=True), want)
    for cull in (True, False):
        rc, got = _field_raw(x, g, grid, R, cull=cull)
        assert rc == 0 and rm.bits_equal(got, want), cull


def test_dead_points_change_nothing():
    x, g, grid = _case(3, "gauss", "some")
    R = SHAPES[3][2]
    want = _field_raw(x, g, grid, R)[1]
    x2 = np.concatenate([x[:, :100], np.zeros((3, 2, 3), F), x[:, 100:]], axis=1)
    g2 = np.concatenate([g[:, :100], np.ones((3, 2, 3), F), g[:, 100:]], axis=1)
    x2[:, 100, 1], g2[:, 101, 2] = np.inf, np.nan
    rc, got = _field_raw(x2, g2, grid, R)
    assert rc == 0 and rm.bits_equal(got, want)


def _synthetic_fields():
    rng = np.random.default_rng(5)
    R = 11
    random = rng.standard_normal((2, R, R, R)).astype(F)
    random[rng.random(random.shape) < 0.08] = np.nan
    smooth = (np.linalg.norm(np.stack(np.meshgrid(*[np.arange(R) - 4.6] * 3, indexing="ij")), axis=0) - 3.3).astype(F)
    holes = smooth.copy()
    holes[rng.random(holes.shape) < 0.03] = np.nan
    inside, outside = np.full((R, R, R), -1.0, F), np.full((R, R, R), 1.0, F)
    single = outside.copy()
    single[5, 6, 4] = -0.25
    corner = outside.copy()
    corner[0, 0, 0] = corner[R - 1, R - 1, R - 1] = -2.0            # crossings at the grid's rim: open edges only
    plane = np.broadcast_to((np.arange(R, dtype=F) - 5)[None, None, :], (R, R, R)).copy()  # f = 0 on the plane k = 5: outside
    minus = plane.copy()
    minus[:, :, 5] = -0.0
    return np.concatenate([random, np.stack([smooth, holes, inside, outside, single, corner, plane, minus])])


def test_the_extraction_equals_the_mirror_on_synthetic_fields():
    fields = _synthetic_fields()
    b = fields.shape[0]
    grid = np.tile(np.array([[-1.3, 0.2, 0.7, 0.173, 1.0]], F), (b, 1))
    grid[:, 3] *= np.linspace(1.0, 2.0, b).astype(F)
    verts, faces, vert_off, face_off, stats = _check_nets(fields, grid)
    assert stats[0, 0] > 100 and stats[0, 3] > 50 and stats[0, 2] > 0                     # random signs and holes: everything occurs
    assert tuple(stats[2]) != tuple(stats[3]) and stats[3, 2] > 0                         # holes open edges
    assert tuple(stats[4]) == tuple(stats[5]) == (0, 0, 0, 0)                             # all inside, all outside
    assert tuple(stats[6]) == (8, 12, 0, 0) and tuple(stats[7]) == (2, 0, 6, 0)           # one inside node: a closed octahedron-like cell complex
    assert tuple(stats[8]) == tuple(stats[9]) and stats[8, 0] == 100                      # +0 and -0 on the plane are both outside
    from pdgn_amd.reconstruct import mesh_report
    rep = mesh_report(verts[vert_off[6]:vert_off[7]], faces[face_off[6]:face_off[7]])
    assert rep["boundary_edges"] == 0 and rep["euler"] == 2 and rep["oriented"] and rep["volume"] > 0
    plane_v = verts[vert_off[8]:vert_off[9]]
    assert (plane_v[:, 2] == plane_v[0, 2]).all()


def test_two_calls_agree_and_the_single_cell_grid_works():
    x, g, grid = _case(4, "torus", "some")
    first, again = _field_raw(x, g, grid, 33), _field_raw(x, g, grid, 33)
    assert first[0] == 0 and first[1].tobytes() == again[1].tobytes()
    a, b = _nets_raw(first[1], grid[:, :4]), _nets_raw(first[1], grid[:, :4])
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
    cell = np.array([[[[-1, 1], [1, 1]], [[1, 1], [1, 1]]]], F)      # R = 2: one cell, one corner inside
    verts, faces, vert_off, face_off, stats = _check_nets(cell, np.array([[0, 0, 0, 1, 1]], F))
    assert tuple(stats[0]) == (1, 0, 3, 0) and np.allclose(verts, 1 / 6)


def test_every_refusal_writes_nothing():
    from pdgn_amd import _lib, reconstruct
    x, g, grid = _case(1, "torus", "some")
    R = 5
    for bad in (dict(call_b=0), dict(call_n=0), dict(call_R=1), dict(call_R=257), dict(call_b=1 << 20, call_R=256), dict(call_cull=2),
                dict(call_cull=-1)):
        rc, out = _field_raw(x, g, grid, R, **bad)
        assert rc == -1 and (out == SENTINEL).all(), bad
    for col, value in ((3, 0.0), (3, -1.0), (4, 0.0), (4, np.inf), (0, np.nan), (3, np.nan)):
        host = grid.copy()
        host[1, col] = value
        rc, out = _field_raw(x, g, grid, R, host=host)
        assert rc == -1 and (out == SENTINEL).all(), (col, value)
    L, p = _lib.lib(), _lib.ptr
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    xd, gd, grd = t(x), t(g), t(grid)
    out = torch.full((2, R, R, R), SENTINEL, device=_dev())
    host = grid.ctypes.data_as(ctypes.c_void_p)
    odd = lambda q: ctypes.c_void_p(q.data_ptr() + 2)
    for slot, tensor in enumerate((xd, gd, grd, None, out)):
        for bad in [None] + ([odd(tensor)] if tensor is not None else [ctypes.c_void_p(grid.ctypes.data + 2)]):
            args = [p(xd), p(gd), p(grd), host, p(out)]
            args[slot] = bad
            assert L.pdgn_imls_grid(2, 3, R, *args[:4], 1, args[4], _lib.stream_of(xd)) == -1, (slot, bad)
    # the extraction
    fd = t(np.random.default_rng(0).standard_normal((2, R, R, R)).astype(F))
    vflag, qcnt = (torch.full((2, R ** 3), 77, dtype=torch.int32, device=_dev()) for _ in range(2))
    stats = torch.full((2, 4), 77, dtype=torch.int32, device=_dev())
    good = [p(fd), p(vflag), p(qcnt), p(stats)]
    for shape in ((0, R), (2, 1), (2, 257), (1 << 20, 256)):
        assert L.pdgn_surface_nets_count(*shape, *good, _lib.stream_of(fd)) == -1
    for slot, tensor in enumerate((fd, vflag, qcnt, stats)):
        for bad in (None, odd(tensor)):
            args = list(good)
            args[slot] = bad
            assert L.pdgn_surface_nets_count(2, R, *args, _lib.stream_of(fd)) == -1
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (vflag == 77).all() and (qcnt == 77).all() and (stats == 77).all()
    assert L.pdgn_surface_nets_count(2, R, *good, _lib.stream_of(fd)) == 0
    vscan, qscan = torch.cumsum(vflag, dim=1, dtype=torch.int32), torch.cumsum(qcnt, dim=1, dtype=torch.int32)
    st = stats.cpu().numpy()
    V, Fc = int(st[:, 0].sum()), int(st[:, 1].sum())
    assert V > 0 and Fc > 0
    vo = t(np.concatenate([[0], np.cumsum(st[:, 0])]).astype(np.int32))
    fo = t(np.concatenate([[0], np.cumsum(st[:, 1])]).astype(np.int32))
    verts = torch.full((V, 3), SENTINEL, device=_dev())
    faces = torch.full((Fc, 3), -5, dtype=torch.int32, device=_dev())
    g4 = np.ascontiguousarray(grid[:, :4])
    g4d = t(g4)

    def emit(b=2, R=R, host=g4, totals=(V, Fc), caps=(V, Fc), **swap):
        ptrs = dict(field=p(fd), grid=p(g4d), host=host.ctypes.data_as(ctypes.c_void_p), vflag=p(vflag), vscan=p(vscan), qcnt=p(qcnt),
                    qscan=p(qscan), vo=p(vo), fo=p(fo), verts=p(verts), faces=p(faces))
        ptrs.update(swap)
        return L.pdgn_surface_nets_emit(b, R, ptrs["field"], ptrs["grid"], ptrs["host"], ptrs["vflag"], ptrs["vscan"], ptrs["qcnt"],
                                        ptrs["qscan"], ptrs["vo"], ptrs["fo"], totals[0], totals[1], caps[0], caps[1], ptrs["verts"],
                                        ptrs["faces"], _lib.stream_of(fd))
    bad_host = g4.copy()
    bad_host[0, 3] = 0.0
    assert emit(b=0) == -1 and emit(R=1) == -1 and emit(host=bad_host) == -1
    assert emit(caps=(V - 1, Fc)) == -1 and emit(caps=(V, Fc - 1)) == -1                  # an output too small for the counted sizes
    assert emit(totals=(-1, Fc)) == -1 and emit(totals=(V, 2 ** 31), caps=(V, 2 ** 31)) == -1
    for name, tensor in (("field", fd), ("grid", g4d), ("vflag", vflag), ("vscan", vscan), ("qcnt", qcnt), ("qscan", qscan), ("vo", vo),
                         ("fo", fo), ("verts", verts), ("faces", faces)):
        assert emit(**{name: None}) == -1 and emit(**{name: odd(tensor)}) == -1, name
    torch.cuda.synchronize()
    assert (verts == SENTINEL).all() and (faces == -5).all()
    assert emit() == 0
    torch.cuda.synchronize()
    assert not (verts == SENTINEL).any() and (faces >= 0).all()
    # the wrappers
    with pytest.raises(ValueError):
        reconstruct.imls_field(xd, gd, resolution=1)
    with pytest.raises(ValueError):
        reconstruct.imls_field(xd, gd[:, :2].contiguous(), resolution=8)
    with pytest.raises(ValueError):
        reconstruct.imls_field(xd, gd, resolution=8, radius=0.0)
    with pytest.raises(ValueError):
        reconstruct.surface_nets(fd[:, :, :, :4].contiguous(), grd[:, :3], grd[:, 3])


def test_h_too_small_for_any_node_gives_an_empty_mesh():
    from pdgn_amd import reconstruct
    x, g = rm.fibonacci_sphere(64)
    t = lambda a: torch.from_numpy(a).to(_dev())
    xd, gd = t(np.stack([x, x])), t(np.stack([g, g]))
    field, origin, voxel = reconstruct.imls_field(xd, gd, resolution=9, radius=1e-4)
    assert torch.isnan(field).all() and (field.view(torch.int32) == rm.NAN_BITS).all()
    verts, faces, vert_off, face_off, stats = reconstruct.surface_nets(field, origin, voxel)
    assert verts.shape == (0, 3) and faces.shape == (0, 3) and faces.dtype == torch.int32
    assert (vert_off == 0).all() and (face_off == 0).all() and stats.cpu().tolist() == [[0, 0, 0, 729]] * 2


def _read_mesh_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    V = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    Fc = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    assert "property list uchar int vertex_indices" in lines and len(body) == 12 * V + 13 * Fc
    verts = np.array(struct.unpack("<%df" % (3 * V), body[:12 * V]), dtype=F).reshape(V, 3)
    rec = np.frombuffer(body[12 * V:], dtype=[("count", "u1"), ("index", "<i4", (3,))])
    assert (rec["count"] == 3).all()
    return verts, rec["index"].astype(np.int32)


# seeds of om.torus(2048, seed) on which the chain of numpy mirrors (normals_mirror at k = 16, orient_mirror, reconstruct_mirror at
# R = 40, radius_factor 5) gives a closed manifold torus on the host: tests/test_reconstruct_host.py asserts it for these
EXPORT_SEEDS = rm.EXPORT_SEEDS


def test_the_export_command_meshes_saved_tori(tmp_path, capsys):
    from pdgn_amd import export
    from pdgn_amd.reconstruct import mesh_report
    clouds = np.stack([om.torus(2048, seed)[0] for seed in EXPORT_SEEDS])
    np.save(tmp_path / "tori.npy", clouds)
    out = export.main([str(tmp_path / "tori.npy"), "-o", str(tmp_path / "plys"), "--mesh", "40"])
    said = capsys.readouterr().out
    assert "normals from 16 neighbours" in said and "(3 components, " in said and " 0 open edges, 0 non-manifold edges" in said
    for i in range(len(EXPORT_SEEDS)):
        verts, faces = _read_mesh_ply("%s/mesh_%d.ply" % (out, i))
        rep = mesh_report(verts, faces)
        print(EXPORT_SEEDS[i], rep)
        assert rep["boundary_edges"] == 0 and rep["nonmanifold_edges"] == 0 and rep["euler"] == 0 and rep["components"] == 1
        assert rep["oriented"] and abs(rep["volume"] / (2 * np.pi ** 2 * 0.16) - 1) < 0.10
        assert open("%s/cloud_%d.ply" % (out, i), "rb").read().count(b"property float") == 6
    out = export.main([str(tmp_path / "tori.npy"), "-o", str(tmp_path / "objs"), "--mesh", "40", "--mesh_format", "obj", "--count", "1",
                       "--mesh_radius", "0.22", "--orient", "consistent"])     # (closed on the chain of mirrors too: h near 5 spacings)
    from pdgn_amd.meshes import load_obj
    v, f = load_obj("%s/mesh_0.obj" % out)
    rep = mesh_report(v, f)
    assert rep["euler"] == 0 and rep["boundary_edges"] == 0 and rep["nonmanifold_edges"] == 0 and f.shape[0] > 500


def test_the_reconstructed_sphere_resamples_as_the_mirrors_mesh_does():
    """reconstruct -> to_meshset -> MeshSet.sample: the Chamfer distance of 2048 surface samples to the input is no larger than the same
    figure from the mirror's mesh (the two meshes are equal bit for bit, so the samples are too)."""
    from pdgn_amd import reconstruct
    x, g = rm.fibonacci_sphere(512)
    t = lambda a: torch.from_numpy(a).to(_dev())
    verts, faces, vert_off, face_off, stats = reconstruct.reconstruct(t(x[None]), t(g[None]), resolution=32, radius_factor=3.0)
    h = 3.0 * float(reconstruct.mean_spacing(t(x[None]))[0])
    origin, voxel, inv = (a.cpu().numpy() for a in reconstruct.grid_for(t(x[None]), 32, h))
    f = rm.field_cloud(x, g, origin[0], voxel[0], inv[0], 32, cull=True).reshape(32, 32, 32)
    mv, mf, mstats = rm.surface_nets_cloud(f, origin[0], voxel[0])

    def chamfer(mesh_v, mesh_f, vo, fo):
        s = reconstruct.to_meshset(mesh_v, mesh_f, vo, fo).to(_dev()).sample(2048, 3)[0].cpu().numpy().astype(np.float64)
        d2 = ((s[:, None, :] - x.astype(np.float64)[None, :, :]) ** 2).sum(-1)
        return d2.min(axis=1).mean() + d2.min(axis=0).mean()
    got = chamfer(verts, faces, vert_off, face_off)
    want = chamfer(mv, mf, [0, mv.shape[0]], [0, mf.shape[0]])
    print("chamfer", got, want, tuple(stats[0].tolist()), mstats)
    assert got <= want and want < 0.02 and tuple(stats[0].tolist()) == mstats
