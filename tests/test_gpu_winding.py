"""Generalized winding numbers on the device: pdgn_winding_number bit for bit against the numpy mirror
(tests/winding_mirror.py) on T, w and inside -- shapes at the group and chunk edges, dead and zero-area faces, a shape without a live
face, every split, points in any order, two runs -- then the definition's fixed cases, the refusals, and what is built on it:
meshes.signed_distance, meshes.occupancy_grid, evaluation.volume_iou, reconstruct.mesh_error(signed=True),
evaluation.surface_fidelity(signed=True) and the occupancy / check commands."""
import ctypes

import numpy as np
import pytest
import torch

import reconstruct_mirror as rm
import winding_mirror as wm

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 7.0
SPLITS = (0, 1, 2, 3, 7)
COUNTS = (1, 65, 257, 600)                                         # a lone face; one past a group of 64; one past a chunk of 256; chunks and a tail
SHAPE = np.asarray([3, 1, 3, 0, 2, 2])                             # repeats, out of order
NMAX = 300


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _four_shapes():
    """verts, faces, face_off of four shapes with COUNTS faces, a few of them of zero area (b == c) in every shape but the lone face;
    `hidden`: a mask that hides a third of the faces and every face of shape 1."""
    rng = np.random.default_rng(77)
    meshes = [wm.random_triangles(1, rng, scale=0.6), wm.first_faces(wm.torus_grid(9, 4), 65), wm.random_triangles(257, rng, scale=0.4),
              wm.torus_grid(20, 15)]
    verts, faces, face_off = wm.concatenate(meshes)
    assert tuple(np.diff(face_off)) == COUNTS
    for s in (1, 2, 3):
        for j in rng.choice(np.arange(face_off[s], face_off[s + 1]), 4, replace=False):
            faces[j, 2] = faces[j, 1]
    t = verts.astype(np.float64)[faces]
    area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    assert (area == 0).sum() == 12
    hidden = rng.uniform(size=faces.shape[0]) < 2 / 3
    hidden[0] = True
    hidden[face_off[1]:face_off[2]] = False
    return verts, faces, face_off, area > 0, hidden


def _points():
    rng = np.random.default_rng(78)
    return rng.uniform(-1.6, 1.6, (SHAPE.shape[0], NMAX, 3)).astype(F)


_WANT = {}


def _mirror(which):
    """The mirror's (T, w, inside) of the NMAX points of every cloud, computed once per set of live faces and shared."""
    if which not in _WANT:
        verts, faces, face_off, positive, hidden = _four_shapes()
        live = positive if which == "all" else positive & hidden
        _WANT[which] = wm.winding(_points(), verts, faces, face_off, SHAPE, live)
    return _WANT[which]


class Prepared:
    """The raw prepare launch of csrc/meshdist.hip on a mesh: the records this kernel reads."""

    def __init__(self, verts, faces, face_off, live=None, order=None):
        from pdgn_amd import _lib
        L = _lib.lib()
        self.S, self.V, self.F = len(face_off) - 1, verts.shape[0], faces.shape[0]
        goff = np.concatenate([[0], np.cumsum(-(-np.diff(np.asarray(face_off, dtype=np.int64)) // L.pdgn_mesh_dist_group()))]).astype(np.int32)
        G = int(goff[-1])
        self.verts, self.faces, self.face_off = _t(verts.astype(F)), _t(faces.astype(np.int32)), _t(np.asarray(face_off).astype(np.int32))
        d_live = _t((np.ones(self.F) if live is None else np.asarray(live)).astype(np.int32))
        d_order = None if order is None else _t(np.asarray(order).astype(np.int32))
        self.records = torch.full((self.F + 1, 12), SENTINEL, dtype=torch.float32, device=_dev())
        groups = torch.empty(max(G, 1), 8, dtype=torch.float32, device=_dev())
        rc = L.pdgn_mesh_dist_prepare(self.S, self.V, self.F, G, _lib.ptr(self.verts), _lib.ptr(self.faces), _lib.ptr(self.face_off),
                                      _lib.ptr(_t(goff)), _lib.ptr(d_live), _lib.ptr(d_order), _lib.ptr(self.records), _lib.ptr(groups),
                                      _lib.stream_of(self.verts))
        torch.cuda.synchronize()
        assert rc == 0 and (self.records[self.F] == SENTINEL).all()


def _raw(prep, points, ids, splits=0, inside=True, **bad):
    """The raw entry point on points (B,N,3) against the shapes ids (B) -> (rc, T, w, inside) numpy; outputs and workspace sentinel-filled
    with one guard row each.  bad: arguments of the call by name, replaced."""
    from pdgn_amd import _lib
    L = _lib.lib()
    B, N, _ = points.shape
    xd, sd = _t(points), _t(np.asarray(ids).astype(np.int32))
    T = torch.full((B * N + 1,), -7, dtype=torch.int64, device=_dev())
    w = torch.full((B * N + 1,), SENTINEL, dtype=torch.float32, device=_dev())
    ins = torch.full((B * N + 1,), -5, dtype=torch.int32, device=_dev())
    nbytes = max(0, L.pdgn_winding_workspace_bytes(B, N, prep.F, bad.get("splits", splits)))      # (-1 for splits the call will refuse)
    assert nbytes % 8 == 0
    work = torch.full((nbytes // 8 + 1,), -9, dtype=torch.int64, device=_dev())
    args = {"b": B, "n": N, "S": prep.S, "F": prep.F, "xyz": _lib.ptr(xd), "shape": _lib.ptr(sd), "face_off": _lib.ptr(prep.face_off),
            "records": _lib.ptr(prep.records), "splits": splits, "workspace": _lib.ptr(work) if nbytes else None, "T": _lib.ptr(T),
            "w": _lib.ptr(w), "inside": _lib.ptr(ins) if inside else None}
    args.update(bad)
    rc = L.pdgn_winding_number(*args.values(), _lib.stream_of(xd))
    torch.cuda.synchronize()
    assert T[B * N] == -7 and w[B * N] == SENTINEL and ins[B * N] == -5 and work[nbytes // 8] == -9
    if rc == 0 and nbytes and not bad:
        assert (work[:nbytes // 8] != -9).all()                    # every entry of the workspace was written
    return rc, T[:B * N].reshape(B, N).cpu().numpy(), w[:B * N].reshape(B, N).cpu().numpy(), ins[:B * N].reshape(B, N).cpu().numpy()


def _same(got, want):
    return all(wm.bits_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 300])
def test_the_kernel_equals_the_mirror(N):
    from pdgn_amd.meshes import MeshSet, _winding, winding_number
    verts, faces, face_off, positive, hidden = _four_shapes()
    xyz = _points()[:, :N].copy()
    rng = np.random.default_rng(N)
    shuffle = np.stack([rng.permutation(N) for _ in range(SHAPE.shape[0])])
    shuffled = np.take_along_axis(xyz, shuffle[..., None], axis=1)
    order = np.concatenate([face_off[s] + rng.permutation(face_off[s + 1] - face_off[s]) for s in range(4)])
    for which, live in (("all", positive), ("visible", positive & hidden)):
        want = [a[:, :N] for a in _mirror(which)]
        assert (want[0] != wm.T_BAD).all() and (N < NMAX or 0 < want[2].sum() < want[2].size)
        if which == "visible":                                     # shape 1 has no live face
            assert (want[0][1] == 0).all() and (want[1][1].view(np.uint32) == 0).all()
        moved = [np.take_along_axis(a, shuffle, 1) for a in want]
        preps = [Prepared(verts, faces, face_off, live), Prepared(verts, faces, face_off, live, order)]
        for splits in SPLITS:
            for prep in preps:
                rc, *got = _raw(prep, xyz, SHAPE, splits)
                assert rc == 0 and _same(got, want), (which, splits)
            rc, *got = _raw(preps[0], shuffled, SHAPE, splits)
            assert rc == 0 and _same(got, moved), (which, splits)
        rc, *again = _raw(preps[1], xyz, SHAPE, 3)                  # a second run
        assert rc == 0 and _same(again, want)
        rc, T, w, ins = _raw(preps[0], xyz, SHAPE, 2, inside=False)  # inside = NULL: the other two all the same
        assert rc == 0 and _same([T, w], want[:2]) and (ins == -5).all()
    # the wrapper: masks that leave every shape a visible face (a MeshSet needs one), visible_only and sort_points both ways, every split
    mask = hidden.copy()
    mask[face_off[1] + int(np.argmax(positive[face_off[1]:face_off[2]]))] = True
    ms = MeshSet.from_arrays(verts, faces, face_off, visible=mask.astype(np.uint32)).to(_dev())
    for visible_only in (False, True):
        want = [a[:, :N] for a in wm.winding(xyz, verts, faces, face_off, SHAPE, positive & mask)] if visible_only else \
            [a[:, :N] for a in _mirror("all")]
        for sort_points in (False, True):
            for splits in SPLITS + (None,):
                got = _winding(_t(xyz), ms, torch.from_numpy(SHAPE), visible_only, sort_points, splits, "winding_number")
                assert _same([g.cpu().numpy() for g in got], want), (visible_only, sort_points, splits)
        w, T = winding_number(_t(xyz), ms, SHAPE, visible_only=visible_only, return_sum=True)
        assert _same([T.cpu().numpy(), w.cpu().numpy()], want[:2])
        assert torch.equal(winding_number(_t(xyz), ms, SHAPE, visible_only=visible_only).view(torch.int32), w.view(torch.int32))


def test_fixed_cases_on_the_device():
    v, f = wm.icosphere(1)
    off = np.asarray([0, f.shape[0]], dtype=np.int32)
    rng = np.random.default_rng(15)
    pts = rng.standard_normal((1, 70, 3)).astype(F)

    def both(verts, faces, face_off, points, ids, live=None):
        want = wm.winding(points, verts, faces, face_off, ids, live)
        for splits in (1, 3):
            rc, *got = _raw(Prepared(verts, faces, face_off, live), points, ids, splits)
            assert rc == 0 and _same(got, want), splits
        return want

    # points at vertices; inside, outside
    T, w, ins = both(v, f, off, v[None, :12], [0])
    assert (np.abs(w - 0.5) < 0.2).all()
    io = np.asarray([[(0, 0, 0), (0.3, 0.2, -0.1), (2, 0, 0), (0, -3, 1)]], dtype=F)
    T, w, ins = both(v, f, off, io, [0])
    assert ins.tolist() == [[1, 1, 0, 0]]
    # points on axis-aligned faces of the unit box: half a turn's worth from the other faces
    bv, bf = wm.box_mesh(0.0, 1.0)
    p = np.asarray([[(0.25, 0.5, 0.0), (0.0, 0.75, 0.125), (1.0, 0.5, 0.5), (0.5, 0.5, 0.5), (0.5, 0.5, 1.5)]], dtype=F)
    T, w, ins = both(bv, bf, np.asarray([0, 12], dtype=np.int32), p, [0])
    assert (np.abs(w[0, :3] - 0.5) < 1e-6).all() and ins[0, 3:].tolist() == [1, 0]
    # degenerate faces that the caller calls live: b == c gives exactly 0
    dv = np.asarray([(0, 0, 0), (1, 0, 0), (1, 0, 0), (2, 0, 0), (0, 0, 0)], dtype=F)
    df = np.asarray([(0, 1, 2), (3, 4, 4), (0, 0, 0)], dtype=np.int32)
    T, w, ins = both(dv, df, np.asarray([0, 3], dtype=np.int32), pts, [0])
    assert (T == 0).all() and (w.view(np.uint32) == 0).all()
    # a shape with no live face, and a shape index out of range: T = 0, w = +0
    two = np.concatenate([pts, pts, pts])
    off2 = np.asarray([0, 40, 80], dtype=np.int32)
    dead = np.concatenate([np.zeros(40, np.int32), np.ones(40, np.int32)])
    want = wm.winding(two[:2], v, f, off2, [0, 1], dead)
    rc, *got = _raw(Prepared(v, f, off2, dead), two, [0, 1, 2], 2)
    assert rc == 0 and _same([g[:2] for g in got], want)
    for c in (0, 2):
        assert (got[0][c] == 0).all() and (got[1][c].view(np.uint32) == 0).all() and (got[2][c] == 0).all()
    # points that are not finite, alone and between finite ones in one workgroup, whatever the shape holds
    bad = pts.copy()
    bad[0, 0, 0], bad[0, 1, 1], bad[0, 2, 2], bad[0, 40] = np.nan, np.inf, -np.inf, np.nan
    for live in (None, np.zeros(f.shape[0], np.int32)):
        T, w, ins = both(v, f, off, bad, [0], live)
        hit = [0, 1, 2, 40]
        assert (T[0, hit] == wm.T_BAD).all() and (w[0, hit].view(np.uint32) == wm.NAN_BITS).all() and (ins[0, hit] == 0).all()
        assert (np.delete(T[0], hit) != wm.T_BAD).all() and np.isfinite(np.delete(w[0], hit)).all()
    rc, T, w, ins = _raw(Prepared(v, f, off), np.full((1, 5, 3), np.nan, dtype=F), [0], 2)
    assert rc == 0 and (T == wm.T_BAD).all() and (w.view(np.uint32) == wm.NAN_BITS).all() and (ins == 0).all()


def test_refusals_leave_the_sentinels():
    v, f = wm.icosphere(0)
    prep = Prepared(v, f, np.asarray([0, 20], dtype=np.int32))
    pts = np.zeros((2, 9, 3), dtype=F)
    odd = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    for bad in ({"b": 0}, {"n": 0}, {"S": 0}, {"F": 0}, {"F": (1 << 28) + 1}, {"splits": -1}, {"splits": 4097}, {"xyz": None}, {"shape": None},
                {"face_off": None}, {"records": None}, {"T": None}, {"w": None}, {"records": odd(prep.records, 4)},
                {"xyz": odd(prep.verts, 2)}, {"b": 1 << 16, "n": 1 << 15}, {"b": (1 << 23) + 1, "n": 1}, {"b": 1 << 12, "n": 1, "splits": 4096}):
        rc, T, w, ins = _raw(prep, pts, [0, 0], **bad)
        assert rc == -1 and (T == -7).all() and (w == SENTINEL).all() and (ins == -5).all(), bad
    for splits in (2, 7):                                          # more than one part needs its workspace, 8-byte aligned; T too
        spare = torch.zeros(64, dtype=torch.int64, device=_dev())
        for bad in ({"workspace": None}, {"workspace": odd(spare, 4)}, {"T": odd(spare, 4)}):
            rc, T, w, ins = _raw(prep, pts, [0, 0], splits, **bad)
            assert rc == -1 and (T == -7).all() and (w == SENTINEL).all() and (ins == -5).all() and (spare == 0).all(), bad
    rc, T, w, ins = _raw(prep, pts, [0, 0])
    assert rc == 0 and (T != -7).all() and (ins == 1).all()        # the centre of an icosahedron


def test_signed_distance():
    from pdgn_amd.meshes import MeshSet, point_to_mesh, signed_distance
    rng = np.random.default_rng(23)
    meshes = [wm.icosphere(2), wm.torus_grid(24, 12)]
    verts, faces, face_off = wm.concatenate(meshes)
    ms = MeshSet.from_meshes(meshes).to(_dev())
    hole = (rng.uniform(-0.3, 0.3, (64, 3)) * (1, 1, 0.5)).astype(F)                        # inside the ring's hole: outside the torus
    tube = np.stack([np.cos(np.arange(64.0)), np.sin(np.arange(64.0)), np.zeros(64)], axis=1) + rng.uniform(-0.2, 0.2, (64, 3))
    x = np.stack([rng.uniform(-1.5, 1.5, (428, 3)).astype(F)] * 3)
    x = np.concatenate([x, np.stack([hole] * 3), np.stack([tube.astype(F)] * 3)], axis=1)
    shape = [1, 0, 1]
    sd, face, inside = signed_distance(_t(x), ms, shape)
    T, w, want = wm.winding(x, verts, faces, face_off, shape)
    assert inside.dtype == torch.bool and (inside.cpu().numpy() == (want != 0)).all()
    assert not inside[0, 428:492].any() and inside[0, 492:].all() and inside[1, 428:492].all()
    d2, f2 = point_to_mesh(_t(x), ms, shape)
    assert torch.equal(face, f2) and torch.equal(sd.abs().view(torch.int32), torch.sqrt(d2).view(torch.int32))
    assert ((sd < 0) == inside).all() and 100 < int(inside.sum()) < inside.numel() - 100
    bad = x[:1, :5].copy()
    bad[0, 0, 0] = np.nan
    sd, face, inside = signed_distance(_t(bad), ms, [0])
    assert torch.isnan(sd[0, 0]) and face[0, 0] == -1 and not inside[0, 0] and torch.isfinite(sd[0, 1:]).all()


def test_occupancy_and_volume_iou_of_two_boxes():
    from pdgn_amd.evaluation import volume_iou
    from pdgn_amd.meshes import MeshSet, occupancy_grid
    (alo, ahi), (blo, bhi) = (2 / 16, 10 / 16), (6 / 16, 14 / 16)
    a, b = MeshSet.from_meshes([wm.box_mesh(alo, ahi)]).to(_dev()), MeshSet.from_meshes([wm.box_mesh(blo, bhi)]).to(_dev())
    unit = ((0, 0, 0), (1, 1, 1))
    occ, origin, voxel = occupancy_grid(a, resolution=16, bounds=unit)
    assert occ.shape == (1, 16, 16, 16) and occ.dtype == torch.bool and origin.tolist() == [[0, 0, 0]] and voxel.tolist() == [1 / 16]
    want = torch.zeros(16, 16, 16, dtype=torch.bool)
    want[2:10, 2:10, 2:10] = True
    assert torch.equal(occ[0].cpu(), want)
    out = volume_iou(a, b, resolution=16, bounds=unit)
    assert [int(out[k][0]) for k in ("count_a", "count_b", "intersection", "union")] == [512, 512, 64, 960]
    assert out["iou"].dtype == torch.float64 and float(out["iou"][0]) == 64 / 960
    # both in one set, named by shape, in slabs of two planes; and the default bounds: the union box grown by 5 % a side
    from pdgn_amd import meshes
    ab = MeshSet.from_meshes([wm.box_mesh(alo, ahi), wm.box_mesh(blo, bhi)]).to(_dev())
    old, meshes.OCCUPANCY_SLAB_POINTS = meshes.OCCUPANCY_SLAB_POINTS, 2 * 2 * 256
    try:
        occ2, _, _ = occupancy_grid(ab, [1, 0], 16, unit)
    finally:
        meshes.OCCUPANCY_SLAB_POINTS = old
    assert torch.equal(occ2[1], occ[0]) and int(occ2[0].sum()) == 512 and int((occ2[0] & occ2[1]).sum()) == 64
    out = volume_iou(ab, ab, [0], [1], resolution=24)
    assert 0.0 < float(out["iou"][0]) < 0.2 and int(out["union"][0]) == int(out["count_a"][0] + out["count_b"][0] - out["intersection"][0])


def test_volume_iou_of_an_icosphere_and_itself_scaled_equals_the_mirror():
    from pdgn_amd.evaluation import volume_iou
    from pdgn_amd.meshes import MeshSet, cubic_grid, occupancy_grid
    R = 32
    v, f = wm.icosphere(1)
    small = ((v.astype(np.float64) * 0.8).astype(F), f)
    verts, faces, face_off = wm.concatenate([(v, f), small])
    ms = MeshSet.from_meshes([(v, f), small]).to(_dev())
    out = volume_iou(ms, ms, [0], [1], resolution=R)
    origin, voxel = cubic_grid(v.min(axis=0)[None].astype(np.float64), v.max(axis=0)[None].astype(np.float64), R, 0.05)
    centres = wm.cell_centres(origin[0], voxel[0], R)
    T, w, ins = wm.winding(np.stack([centres, centres]), verts, faces, face_off, [0, 1])
    a, b = ins[0] != 0, ins[1] != 0
    assert [int(out[k][0]) for k in ("count_a", "count_b", "intersection", "union")] == [a.sum(), b.sum(), (a & b).sum(), (a | b).sum()]
    assert float(out["iou"][0]) == (a & b).sum() / (a | b).sum() and not (b & ~a).any()
    assert abs(float(out["iou"][0]) - 0.8 ** 3) < 0.03               # similar solids: the ratio of the volumes
    occ, o, vx = occupancy_grid(ms, [0], R)
    assert o.cpu().numpy().tolist() == origin.tolist() and vx.cpu().numpy().tolist() == voxel.tolist()
    assert (occ[0].cpu().numpy().reshape(-1) == a).all()


def test_mesh_error_signed_of_a_reconstructed_sphere():
    """The reconstruction of tests/test_gpu_p2m.py's sphere (a Fibonacci sphere of 2048 points on R = 33 nodes per axis) against the
    icosphere of level 4.  That test asserts that the two surfaces are within one voxel v (relative to the radius 1) of each other in the
    mean; a solid between the balls of radius 1 - v and 1 + v has an IoU with the unit ball of at least ((1 - v) / (1 + v))^3.  The signed
    mean cannot exceed the unsigned one in magnitude.  Measured: section 7u."""
    from pdgn_amd import reconstruct
    from pdgn_amd.meshes import MeshSet
    R, n = 33, 2048
    x, g = rm.fibonacci_sphere(n)
    field, origin, voxel = reconstruct.imls_field(_t(x[None]), _t(g[None]), R)
    mesh = reconstruct.surface_nets(field, origin, voxel)
    ms = MeshSet.from_meshes([wm.icosphere(4)]).to(_dev())
    plain = reconstruct.mesh_error(*mesh[:4], ms, samples=2048)
    err = reconstruct.mesh_error(*mesh[:4], ms, samples=2048, signed=True)
    assert list(err)[:len(plain)] == list(plain) and all(torch.equal(err[k], plain[k]) for k in plain)
    assert set(err) - set(plain) == {"to_reference_signed_mean", "iou"}
    v = float(voxel[0])
    signed, mean, iou = float(err["to_reference_signed_mean"][0]), float(err["to_reference_mean"][0]), float(err["iou"][0])
    print("mesh_error(signed=True): voxel %.4f, to_reference_mean %.6f, signed mean %+.6f, iou %.6f (bound %.6f)" % (
        v, mean, signed, iou, ((1 - v) / (1 + v)) ** 3))
    assert err["iou"].shape == (1,) and ((1 - v) / (1 + v)) ** 3 <= iou <= 1.0
    assert abs(signed) <= mean


def test_surface_fidelity_signed():
    from pdgn_amd.evaluation import surface_fidelity
    from pdgn_amd.meshes import MeshSet
    ms = MeshSet.from_meshes([wm.icosphere(3)] * 2).to(_dev())
    unit, _ = rm.fibonacci_sphere(512)
    clouds = _t(np.stack([(unit.astype(np.float64) * 0.9).astype(F), (unit.astype(np.float64) * 1.1).astype(F)]))
    plain = surface_fidelity(clouds, ms)
    out = surface_fidelity(clouds, ms, signed=True)
    assert list(out)[:len(plain) - 1] == list(plain)[:-1] and set(out) - set(plain) == {"inside_fraction", "signed_mean"}
    for k in plain:
        if k != "mean":
            assert torch.equal(out[k], plain[k]), k
            assert out["mean"][k] == plain["mean"][k]
    assert out["inside_fraction"].tolist() == [1.0, 0.0]
    assert torch.equal(out["signed_mean"], out["accuracy_mean"] * torch.tensor([-1.0, 1.0], dtype=torch.float64, device=_dev()))
    assert out["mean"]["inside_fraction"] == 0.5


def test_the_occupancy_and_check_commands(tmp_path, capsys):
    from pdgn_amd import meshes
    verts, faces, face_off = wm.concatenate([wm.icosphere(2), wm.torus_grid(16, 8)])
    np.savez(tmp_path / "packed.npz", **{"03001627/val/verts": verts, "03001627/val/faces": faces, "03001627/val/face_off": face_off})
    meshes.main(["occupancy", str(tmp_path / "packed.npz"), str(tmp_path / "occ.npz"), "--resolution", "12", "--shape", "1,0", "--device", "cuda:0"])
    assert "2 grids of 12^3 cells" in capsys.readouterr().out
    with np.load(tmp_path / "occ.npz") as f:
        assert f["occupancy"].shape == (2, 12 ** 3 // 8) and f["occupancy"].dtype == np.uint8 and int(f["resolution"]) == 12
        assert f["origin"].shape == (2, 3) and f["voxel"].shape == (2,) and f["shape"].tolist() == [1, 0]
        grids = np.unpackbits(f["occupancy"], axis=1)[:, :12 ** 3].reshape(2, 12, 12, 12).astype(bool)
    ms = meshes.MeshSet.from_arrays(verts, faces, face_off).to(_dev())
    occ, _, _ = meshes.occupancy_grid(ms, [1, 0], 12)
    assert (occ.cpu().numpy() == grids).all() and grids[1, 6, 6, 6] and not grids[0, 6, 6, 6] and grids[0].any()
    meshes.main(["check", str(tmp_path / "packed.npz"), "--samples", "512", "--device", "cuda:0"])
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 4 and lines[0].split() == ["shape", "w_min", "w_max", "fractional"] and "closed and consistently oriented" in lines[3]
    rep = meshes.winding_report(ms, 512)
    assert (np.abs(rep["w_min"]) < 1e-5).all() and (np.abs(rep["w_max"] - 1) < 1e-5).all() and (rep["fractional"] == 0).all()
    # a shape with flipped faces is told apart
    flipped = faces.copy()
    flipped[:160] = flipped[:160, ::-1]
    rep = meshes.winding_report(meshes.MeshSet.from_arrays(verts, flipped, face_off).to(_dev()), 512)
    assert rep["fractional"][0] > 0.5 and rep["fractional"][1] == 0
    # distance --signed: the signed columns after the others
    unit, _ = rm.fibonacci_sphere(64)
    np.save(tmp_path / "clouds.npy", np.stack([unit * F(0.5), unit]))
    meshes.main(["distance", str(tmp_path / "clouds.npy"), str(tmp_path / "packed.npz"), "--shape", "0,0", "--signed", "--device", "cuda:0"])
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[0].split()[-2:] == ["inside_fraction", "signed_mean"] and float(lines[1].split()[-2]) == 1.0 and float(lines[1].split()[-1]) < -0.4
