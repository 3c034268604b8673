"""Point-to-surface distance on the device: pdgn_mesh_dist_prepare / pdgn_point_mesh_distance bit for bit against
the numpy mirror (tests/p2m_mirror.py) on d2, face and closest -- random triangles, slivers and a torus; points far away, on the surface
and mixed; the culling on and off; points and face records in any order; shapes as identity, permuted and repeated -- then the
definition's corner cases, repeatability, the refusals, sampled points against their own shape, the visible surface, the gradient of
losses.surface_distance, evaluation.surface_fidelity against closed forms and reconstruct.mesh_error on a reconstructed sphere."""
import ctypes

import numpy as np
import pytest
import torch

import p2m_mirror as pm
import reconstruct_mirror as rm

pytestmark = pytest.mark.gpu
F = np.float32
ULP = 2.0 ** -24
BOUND = 64.0
SENTINEL = 7.0
# (B, N, faces per shape): the smallest call; ragged face counts; one point past a wave; one past a chunk of 256 slots with a tail of one
# slot, ragged, and one point past a run of 256 points; several staging chunks with a tail and several runs with a tail; whole chunks and runs
CASES = [(1, 1, [1]), (2, 3, [3, 1]), (1, 65, [20]), (3, 257, [80, 257, 1]), (2, 1100, [1280, 1030]), (1, 2048, [512])]
KINDS = ("random", "sliver", "torus")
REGIMES = ("far", "surface", "mixed")


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _shape_mesh(kind, count, rng):
    if kind == "random":
        return pm.random_triangles(count, rng, scale=0.4)
    if kind == "sliver":
        return pm.slivers(count, rng, 1e-4)
    return pm.first_faces(pm.torus_grid(max(3, -(-count // 16)), 8), count)


def _case(case, kind, regime):
    """-> verts, faces, face_off of the case's shapes and xyz (B,N,3): points in a box five units away from the mesh (every face is about
    as far: little is culled), on the faces (nearly everything is culled), or half in the mesh's box and half on the faces."""
    B, N, counts = CASES[case]
    rng = np.random.default_rng(100 * case + 10 * KINDS.index(kind) + REGIMES.index(regime))
    meshes = [_shape_mesh(kind, c, rng) for c in counts]
    verts, faces, face_off = pm.concatenate(meshes)
    xyz = np.empty((B, N, 3), dtype=F)
    for c, (v, f) in enumerate(meshes):
        far = (rng.uniform(-1, 1, (N, 3)) + (5.0, 0.0, 0.0)).astype(F)
        on, _ = pm.points_on_faces(v, f, N, rng)
        box = rng.uniform(v.min(axis=0) - 0.2, v.max(axis=0) + 0.2, (N, 3)).astype(F)
        xyz[c] = {"far": far, "surface": on, "mixed": np.where((np.arange(N) % 2 == 0)[:, None], box, on)}[regime]
    return verts, faces, face_off, xyz


class Prepared:
    """The raw prepare launch on a mesh: records and groups with a guard row each."""

    def __init__(self, verts, faces, face_off, live=None, order=None):
        from pdgn_amd import _lib
        L = _lib.lib()
        self.S, self.V, self.F = len(face_off) - 1, verts.shape[0], faces.shape[0]
        group = L.pdgn_mesh_dist_group()
        goff = np.concatenate([[0], np.cumsum(-(-np.diff(face_off.astype(np.int64)) // group))]).astype(np.int32)
        self.G = int(goff[-1])
        assert 12 * self.F + 8 * self.G <= L.pdgn_mesh_dist_workspace_floats(self.S, self.F)
        self.verts, self.faces, self.face_off, self.group_off = _t(verts.astype(F)), _t(faces.astype(np.int32)), _t(face_off.astype(np.int32)), _t(goff)
        self.live = _t((np.ones(self.F) if live is None else np.asarray(live)).astype(np.int32))
        self.order = None if order is None else _t(np.asarray(order).astype(np.int32))
        self.records = torch.full((self.F + 1, 12), SENTINEL, dtype=torch.float32, device=_dev())
        self.groups = torch.full((self.G + 1, 8), SENTINEL, dtype=torch.float32, device=_dev())
        rc = L.pdgn_mesh_dist_prepare(self.S, self.V, self.F, self.G, _lib.ptr(self.verts), _lib.ptr(self.faces), _lib.ptr(self.face_off),
                                      _lib.ptr(self.group_off), _lib.ptr(self.live), _lib.ptr(self.order), _lib.ptr(self.records),
                                      _lib.ptr(self.groups), _lib.stream_of(self.verts))
        torch.cuda.synchronize()
        assert rc == 0 and (self.records[self.F] == SENTINEL).all() and (self.groups[self.G] == SENTINEL).all()


def _raw(prep, points, ids, cull=1, closest=True, **bad):
    """The raw entry point on points (B,N,3) against the shapes ids (B) -> (rc, d2 (B,N), face (B,N), closest (B,N,3)) numpy; outputs
    sentinel-filled, one guard row each.  bad: arguments of the call by name, replaced."""
    from pdgn_amd import _lib
    B, N, _ = points.shape
    xd, sd = _t(points), _t(np.asarray(ids).astype(np.int32))
    d2 = torch.full((B * N + 1,), SENTINEL, dtype=torch.float32, device=_dev())
    face = torch.full((B * N + 1,), -5, dtype=torch.int32, device=_dev())
    q = torch.full((B * N + 1, 3), SENTINEL, dtype=torch.float32, device=_dev())
    args = {"b": B, "n": N, "S": prep.S, "F": prep.F, "G": prep.G, "xyz": _lib.ptr(xd), "shape": _lib.ptr(sd), "face_off": _lib.ptr(prep.face_off),
            "group_off": _lib.ptr(prep.group_off), "records": _lib.ptr(prep.records), "groups": _lib.ptr(prep.groups), "cull": cull,
            "d2": _lib.ptr(d2), "face": _lib.ptr(face), "closest": _lib.ptr(q) if closest else None}
    args.update(bad)
    rc = _lib.lib().pdgn_point_mesh_distance(*args.values(), _lib.stream_of(xd))
    torch.cuda.synchronize()
    assert d2[B * N] == SENTINEL and face[B * N] == -5 and (q[B * N] == SENTINEL).all()
    return rc, d2[:B * N].reshape(B, N).cpu().numpy(), face[:B * N].reshape(B, N).cpu().numpy(), q[:B * N].reshape(B, N, 3).cpu().numpy()


def _same(got, want):
    return all(pm.bits_equal(a, b) for a, b in zip(got, want))


def _within_shape_permutation(face_off, rng):
    return np.concatenate([face_off[s] + rng.permutation(face_off[s + 1] - face_off[s]) for s in range(len(face_off) - 1)])


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_kernel_equals_the_mirror(case, kind, regime):
    from pdgn_amd.meshes import MeshSet, point_to_mesh
    B, N, counts = CASES[case]
    verts, faces, face_off, xyz = _case(case, kind, regime)
    rng = np.random.default_rng(case)
    S = len(counts)
    # every (cloud, shape) pair once: the result is a pure function of the point and the shape's faces
    table = {}

    def mirror(shape):
        out = [np.empty((B, N), F), np.empty((B, N), np.int32), np.empty((B, N, 3), F)]
        for c, s in enumerate(shape):
            if (c, s) not in table:
                table[(c, s)] = pm.point_to_mesh(xyz[c:c + 1], verts, faces, face_off, [s])
            for dst, src in zip(out, table[(c, s)]):
                dst[c] = src[0]
        return out

    preps = [Prepared(verts, faces, face_off), Prepared(verts, faces, face_off, order=_within_shape_permutation(face_off, rng))]
    shapes = [np.arange(B) % S, (np.arange(B)[::-1]) % S, np.zeros(B, dtype=np.int64) + (S - 1)]     # identity, a permutation, repeats
    shuffle = np.stack([rng.permutation(N) for _ in range(B)])
    shuffled = np.take_along_axis(xyz, shuffle[..., None], axis=1)
    for shape in shapes:
        want = mirror(shape)
        assert np.isfinite(want[0]).all() and (want[1] >= 0).all()
        moved = [np.take_along_axis(want[0], shuffle, 1), np.take_along_axis(want[1], shuffle, 1), np.take_along_axis(want[2], shuffle[..., None], 1)]
        for prep in preps:
            for cull in (1, 0):
                rc, *got = _raw(prep, xyz, shape, cull)
                assert rc == 0 and _same(got, want), (shape, cull)
                rc, *got = _raw(prep, shuffled, shape, cull)
                assert rc == 0 and _same(got, moved), (shape, cull)
    # the wrapper: the module's defaults, and every coherence option the other way
    ms = MeshSet.from_arrays(verts, faces, face_off).to(_dev())
    want = mirror(shapes[1])
    for options in ({}, {"sort_points": False, "sort_faces": True}, {"sort_points": True, "sort_faces": False, "cull": False}):
        got = point_to_mesh(_t(xyz), ms, torch.from_numpy(shapes[1]), return_closest=True, **options)
        assert _same([g.cpu().numpy() for g in got], want), options


def test_the_culling_leaves_faces_out_where_it_claims_to():
    """Not a timing: a torus in array order, 64 points a little off the faces of its first group.  The records of a group on the far side
    of the ring are then overwritten with a triangle collapsed onto point 0 while the group's box stays what the prepare launch wrote:
    culled, the group is never visited and the bits are those of the clean records; not culled, it is, and point 0 finds distance zero."""
    verts, faces = pm.torus_grid(64, 16)                            # 2048 faces, 32 groups in array order around the ring
    face_off = np.asarray([0, faces.shape[0]], dtype=np.int32)
    rng = np.random.default_rng(5)
    pts, _ = pm.points_on_faces(verts, faces[:64], 64, rng)
    pts = (pts + rng.uniform(-0.01, 0.01, pts.shape)).astype(F)
    prep = Prepared(verts, faces, face_off)
    want = pm.point_to_mesh(pts[None], verts, faces, face_off)
    assert (want[0] > 0).all()
    for cull in (1, 0):
        rc, *got = _raw(prep, pts[None], [0], cull)
        assert rc == 0 and _same(got, want)
    for k in range(3):
        prep.records[1024:1088, 4 * k:4 * k + 3] = _t(pts[0])
    rc, *got = _raw(prep, pts[None], [0], 1)
    assert rc == 0 and _same(got, want)
    rc, *got = _raw(prep, pts[None], [0], 0)
    assert rc == 0 and got[0][0, 0] == 0 and 1024 <= got[1][0, 0] < 1088 and pm.bits_equal(got[0][0, 1:], want[0][0, 1:])


def test_definition_cases_on_the_device():
    v, f = pm.icosphere(0)
    rng = np.random.default_rng(15)
    pts = rng.standard_normal((1, 64, 3)).astype(F)
    one = np.asarray([0, 20], dtype=np.int32)
    # duplicate faces: the lowest index wins whatever the slot order
    faces = np.concatenate([f, f[::-1], f])
    off = np.asarray([0, 60], dtype=np.int32)
    want = pm.point_to_mesh(pts, v, faces, off)
    for order in (None, np.arange(60)[::-1].copy(), rng.permutation(60)):
        for cull in (1, 0):
            rc, *got = _raw(Prepared(v, faces, off, order=order), pts, [0], cull)
            assert rc == 0 and _same(got, want) and (got[1] < 20).all()
    # points exactly on shared vertices; on the midpoint of a shared edge
    want = pm.point_to_mesh(v[None, :12], v, f, one)
    rc, *got = _raw(Prepared(v, f, one, order=rng.permutation(20)), v[None, :12], [0])
    assert rc == 0 and _same(got, want) and (got[0] == 0).all()
    assert [int(x) for x in got[1][0]] == [min(j for j in range(20) if i in f[j]) for i in range(12)]
    quad_v = np.asarray([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], dtype=F)
    quad_f = np.asarray([(0, 2, 3), (0, 1, 2)], dtype=np.int32)
    mid = np.asarray([[(0.5, 0.5, 0.0), (0.25, 0.25, 0.0), (0.5, 0.5, 2.0)]], dtype=F)
    for order in (None, [1, 0]):
        rc, *got = _raw(Prepared(quad_v, quad_f, np.asarray([0, 2], dtype=np.int32), order=order), mid, [0])
        assert rc == 0 and (got[1] == 0).all() and pm.bits_equal(got[0], np.asarray([[0, 0, 4]], dtype=F))
    # dead faces are never returned; a shape with no live face, and a shape index out of range: NaN, -1, NaN
    live = np.ones(20, dtype=np.int32)
    live[::2] = 0
    rc, *got = _raw(Prepared(v, f, one, live=live), pts, [0])
    assert rc == 0 and _same(got, pm.point_to_mesh(pts, v, f, one, live=live)) and (got[1] % 2 == 1).all()
    two, off2 = np.concatenate([pts, pts, pts]), np.asarray([0, 10, 20], dtype=np.int32)
    dead = np.concatenate([np.zeros(10, np.int32), np.ones(10, np.int32)])
    for cull in (1, 0):
        rc, *got = _raw(Prepared(v, f, off2, live=dead), two, [0, 1, 2], cull)
        assert rc == 0 and _same(got, pm.point_to_mesh(two, v, f, off2, [0, 1, 2], live=dead))
        for c in (0, 2):
            assert (got[0][c].view(np.uint32) == pm.NAN_BITS).all() and (got[1][c] == -1).all() and (got[2][c].view(np.uint32) == pm.NAN_BITS).all()
    # points that are not finite, alone in their wave and among others
    bad = pts.copy()
    bad[0, 0, 0], bad[0, 1, 1], bad[0, 2, 2], bad[0, 40] = np.nan, np.inf, -np.inf, np.nan
    for cull in (1, 0):
        rc, *got = _raw(Prepared(v, f, one), bad, [0], cull)
        assert rc == 0 and _same(got, pm.point_to_mesh(bad, v, f, one))
        assert (got[1][0, [0, 1, 2, 40]] == -1).all() and (got[0][0, [0, 1, 2, 40]].view(np.uint32) == pm.NAN_BITS).all()
        rc, *got = _raw(Prepared(v, f, one), np.full((1, 5, 3), np.nan, dtype=F), [0], cull)
        assert rc == 0 and (got[1] == -1).all()
    # a degenerate face that the caller calls live: the clamps' fmax / fmin semantics, on both sides alike
    deg_v = np.asarray([(0, 0, 0), (0, 0, 0), (1, 0, 0), (2, 0, 0)], dtype=F)
    deg_f = np.asarray([(0, 1, 1), (0, 2, 3)], dtype=np.int32)
    off = np.asarray([0, 2], dtype=np.int32)
    rc, *got = _raw(Prepared(deg_v, deg_f, off), pts, [0])
    assert rc == 0 and _same(got, pm.point_to_mesh(pts, deg_v, deg_f, off))
    # closest = NULL: the other two outputs all the same
    rc, d2, face, q = _raw(Prepared(v, f, one), pts, [0], closest=False)
    assert rc == 0 and _same([d2, face], pm.point_to_mesh(pts, v, f, one)[:2]) and (q == SENTINEL).all()


def test_two_runs_and_every_coherence_option_give_the_same_bits():
    from pdgn_amd.meshes import MeshSet, point_to_mesh
    rng = np.random.default_rng(21)
    ms = MeshSet.from_meshes([pm.torus_grid(20, 10), pm.icosphere(2), pm.slivers(150, rng, 1e-4)]).to(_dev())
    x = _t(rng.uniform(-1.5, 1.5, (5, 700, 3)).astype(F))
    shape = torch.tensor([2, 0, 1, 1, 0])
    first = point_to_mesh(x, ms, shape, return_closest=True)
    for options in ({}, {"cull": False}, {"sort_points": False}, {"sort_faces": True}, {"sort_faces": False}, {"sort_points": False, "sort_faces": True, "cull": False}):
        again = point_to_mesh(x, ms, shape, return_closest=True, **options)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again)), options
    assert set(ms._mesh_dist) == {(False, True), (False, False)}    # prepared once per option, cached on the object


def test_refusals_leave_the_sentinels():
    v, f = pm.icosphere(0)
    one = np.asarray([0, 20], dtype=np.int32)
    prep = Prepared(v, f, one)
    pts = np.zeros((2, 9, 3), dtype=F)
    from pdgn_amd import _lib
    odd = ctypes.c_void_p(prep.records.data_ptr() + 4)
    for bad in ({"b": 0}, {"n": 0}, {"S": 0}, {"F": 0}, {"G": 0}, {"G": 3}, {"cull": 2}, {"cull": -1}, {"xyz": None}, {"shape": None},
                {"face_off": None}, {"group_off": None}, {"records": None}, {"groups": None}, {"d2": None}, {"face": None},
                {"records": odd}, {"groups": ctypes.c_void_p(prep.groups.data_ptr() + 8)}, {"xyz": ctypes.c_void_p(prep.verts.data_ptr() + 2)},
                {"b": 1 << 16, "n": 1 << 15}, {"b": (1 << 23) + 1, "n": 1}):
        rc, d2, face, q = _raw(prep, pts, [0, 0], **bad)
        assert rc == -1 and (d2 == SENTINEL).all() and (face == -5).all() and (q == SENTINEL).all(), bad
    rc, d2, face, q = _raw(prep, pts, [0, 0])
    assert rc == 0 and (d2 != SENTINEL).all()
    # the prepare launch
    L = _lib.lib()
    rec = torch.full((21, 12), SENTINEL, dtype=torch.float32, device=_dev())
    grp = torch.full((2, 8), SENTINEL, dtype=torch.float32, device=_dev())
    good = {"S": 1, "V": 12, "F": 20, "G": 1, "verts": _lib.ptr(prep.verts), "faces": _lib.ptr(prep.faces), "face_off": _lib.ptr(prep.face_off),
            "group_off": _lib.ptr(prep.group_off), "live": _lib.ptr(prep.live), "order": None, "records": _lib.ptr(rec), "groups": _lib.ptr(grp)}
    for bad in ({"S": 0}, {"V": 0}, {"F": 0}, {"G": 0}, {"G": 2}, {"verts": None}, {"faces": None}, {"face_off": None}, {"group_off": None},
                {"live": None}, {"records": None}, {"groups": None}, {"records": ctypes.c_void_p(rec.data_ptr() + 4)}):
        assert L.pdgn_mesh_dist_prepare(*{**good, **bad}.values(), _lib.stream_of(rec)) == -1, bad
    torch.cuda.synchronize()
    assert (rec == SENTINEL).all() and (grp == SENTINEL).all()
    assert L.pdgn_mesh_dist_prepare(*good.values(), _lib.stream_of(rec)) == 0
    torch.cuda.synchronize()
    assert (rec[:20] != SENTINEL).any() and (rec[20] == SENTINEL).all() and (grp[1] == SENTINEL).all()


def test_sampled_points_and_the_visible_surface():
    from pdgn_amd.meshes import MeshSet, point_to_mesh
    rng = np.random.default_rng(31)
    meshes = [pm.icosphere(2), pm.torus_grid(24, 12), pm.slivers(100, rng, 1e-4)]
    ms = MeshSet.from_meshes(meshes).to(_dev())
    pts, drawn = ms.sample(300, 9, return_faces=True)
    d2, face = point_to_mesh(pts, ms)
    M = float(ms.verts.abs().max())
    assert float(d2.double().sqrt().max()) <= BOUND * ULP * M       # every sampled point lies on its own shape
    off = ms.face_off.cpu().numpy()
    for c in range(3):
        assert ((face[c] >= int(off[c])) & (face[c] < int(off[c + 1]))).all()
    # visible_only: a masked face is never returned, and the distance to the visible surface is never below the one to all of it
    mask = np.ones(ms.F, dtype=np.uint32)
    mask[rng.permutation(ms.F)[:ms.F // 2]] = 0
    mask[off[:-1]] = 1
    vis = MeshSet.from_meshes(meshes, visible=mask).to(_dev())
    x = _t(rng.uniform(-1.3, 1.3, (3, 400, 3)).astype(F))
    d_all, f_all = point_to_mesh(x, vis)
    d_vis, f_vis, q_vis = point_to_mesh(x, vis, visible_only=True, return_closest=True)
    assert (_t(mask.astype(np.int32))[f_vis.long()] != 0).all() and (d_vis >= d_all).all() and (d_vis > d_all).any()
    want = pm.point_to_mesh(x.cpu().numpy(), vis.verts.cpu().numpy(), vis.faces.cpu().numpy(), off, live=mask)
    assert _same([d_vis.cpu().numpy(), f_vis.cpu().numpy(), q_vis.cpu().numpy()], want)


def test_the_gradient_of_surface_distance():
    """Against central differences of the mirror's expressions in float64, at points away from the medial axis: the mirror's gap between
    the best and the second-best face is at least 0.01 in distance, the step 1e-3 (a distance is 1-Lipschitz, so the gap outlives the step
    five times over, and with it the closest feature: on a shared edge or vertex the gap is zero).  d2 is a quadratic in p while the closest feature stays
    the same, so the differences are exact up to float64 rounding; the analytic side is 2 (p - closest) in fp32: closest = p - n h carries
    the relative errors of n (a few ulps / sin of the face's angle) and of h (a dozen roundings), times a distance below one, and the
    difference one more rounding of M -- well below 2 * 16 ulps of M.  The bound: 64 * 2^-24 * M per component."""
    from pdgn_amd.losses import surface_distance
    from pdgn_amd.meshes import MeshSet
    rng = np.random.default_rng(41)
    meshes = [pm.icosphere(1), pm.torus_grid(12, 6)]
    ms = MeshSet.from_meshes(meshes).to(_dev())
    verts, faces, off = ms.verts.cpu().numpy(), ms.faces.cpu().numpy(), ms.face_off.cpu().numpy()
    shape = [1, 0, 1]
    xyz = rng.uniform(-1.4, 1.4, (3, 256, 3)).astype(F)
    keep = np.zeros((3, 256), dtype=bool)
    numeric = np.zeros((3, 256, 3))
    h = 1e-3
    for c, s in enumerate(shape):
        tri = verts[faces[off[s]:off[s + 1]]]
        best = pm.closest_of(xyz[c], tri, np.arange(tri.shape[0]))[0]
        keep[c] = np.sqrt(pm.runner_up(xyz[c], tri).astype(np.float64)) - np.sqrt(best.astype(np.float64)) >= 0.01
        for k in range(3):
            step = np.zeros(3)
            step[k] = h
            up = pm.face_values(xyz[c].astype(np.float64) + step, tri[:, 0], tri[:, 1], tri[:, 2], dtype=np.float64)[0].min(axis=1)
            down = pm.face_values(xyz[c].astype(np.float64) - step, tri[:, 0], tri[:, 1], tri[:, 2], dtype=np.float64)[0].min(axis=1)
            numeric[c, :, k] = (up - down) / (2 * h)
    assert keep.sum() >= 100
    x = _t(xyz).requires_grad_(True)
    weight = _t(rng.uniform(0.5, 2.0, (3, 256)).astype(F))
    d2 = surface_distance(x, ms, shape, reduction="none")
    (d2 * weight).sum().backward()
    got = (x.grad / weight[..., None]).cpu().numpy().astype(np.float64)
    M = max(float(np.abs(verts).max()), float(np.abs(xyz).max()))
    err = np.abs(got - numeric)[keep].max()
    print("gradient: worst error %.3g = %.2f ulps of M over %d points" % (err, err / (ULP * M), keep.sum()))
    assert err <= BOUND * ULP * M
    # reductions; NaN points give a zero gradient and are left out of the mean
    bad = xyz.copy()
    bad[0, 0, 0] = np.nan
    y = _t(bad).requires_grad_(True)
    mean = surface_distance(y, ms, shape)
    mean.backward()
    none = surface_distance(_t(bad), ms, shape, reduction="none")
    assert torch.isnan(none[0, 0]) and torch.isfinite(mean) and torch.allclose(mean, torch.nansum(none) / (3 * 256 - 1))
    assert (y.grad[0, 0] == 0).all() and torch.isfinite(y.grad).all()
    assert torch.allclose(surface_distance(_t(bad), ms, shape, reduction="sum"), torch.nansum(none))
    assert ms.verts.grad is None


def test_surface_fidelity_on_an_icosphere():
    """Closed forms: the icosphere of level 3 is inscribed in the unit sphere, its faces at most sag = 1 - (the least distance of a face's
    plane from the centre) inside it.  A point of the unit sphere is then at most sag from it (the point below it on the face's plane is
    nearer than that, or a neighbouring face is nearer still -- the polyhedron is convex); a point at radius 1.1 is at least 0.1 away (the
    polyhedron lies inside the unit ball) and at most 0.1 + sag (along its ray)."""
    from pdgn_amd.evaluation import surface_fidelity
    from pdgn_amd.meshes import MeshSet
    level, N = 3, 2048
    sag = pm.icosphere_sag(level)
    assert 0 < sag < 0.02
    ms = MeshSet.from_meshes([pm.icosphere(level)] * 2).to(_dev())
    unit, _ = rm.fibonacci_sphere(N)
    clouds = _t(np.stack([unit, (unit.astype(np.float64) * 1.1).astype(F)]))
    slack = BOUND * ULP * 1.1
    out = surface_fidelity(clouds, ms, thresholds=(0.02, 0.05))
    for key in ("accuracy_mean", "accuracy_rms", "accuracy_max", "completeness_mean", "completeness_rms", "completeness_max", "precision@0.02",
                "recall@0.02", "fscore@0.02", "precision@0.05", "recall@0.05", "fscore@0.05"):
        assert out[key].shape == (2,) and out[key].dtype == torch.float64 and torch.isfinite(out[key]).all(), key
        assert abs(out["mean"][key] - float(out[key].mean())) < 1e-12
    a = {k: out["accuracy_" + k].cpu().numpy() for k in ("mean", "rms", "max")}
    assert 0 < a["mean"][0] <= a["rms"][0] <= a["max"][0] <= sag + slack
    assert 0.1 - slack <= a["mean"][1] <= a["rms"][1] <= a["max"][1] <= 0.1 + sag + slack
    # thresholds above the sag: every point of the unit cloud is within them, none of the scaled one
    assert out["precision@0.02"].tolist() == [1.0, 0.0] and out["precision@0.05"].tolist() == [1.0, 0.0]
    # the surface samples lie on the polyhedron, each within (sag + the lattice's covering radius) of the unit cloud; the golden-angle
    # lattice of N points covers the sphere with caps of less than twice its mean spacing sqrt(4 pi / N)
    cover = 2.0 * np.sqrt(4 * np.pi / N)
    c = out["completeness_max"].cpu().numpy()
    assert 0 < c[0] <= sag + cover and 0.1 - slack <= c[1] <= 0.1 + sag + 1.1 * cover
    assert float(out["recall@0.05"][1]) == 0.0 and float(out["fscore@0.05"][1]) == 0.0
    assert 0 < float(out["recall@0.05"][0]) <= 1.0 and float(out["fscore@0.05"][0]) > 0
    # one cloud against a chosen shape, fewer samples
    one = surface_fidelity(clouds[1:], ms, shape=[0], samples=500)
    assert abs(float(one["accuracy_mean"][0]) - a["mean"][1]) < 1e-12


def test_mesh_error_of_a_reconstructed_sphere():
    """reconstruct of a Fibonacci sphere on R = 33 nodes per axis against the icosphere of level 4 (sag 0.002): finite, and below one voxel
    in the mean in both directions."""
    from pdgn_amd import reconstruct
    from pdgn_amd.meshes import MeshSet
    R, n = 33, 2048
    x, g = rm.fibonacci_sphere(n)
    xd, gd = _t(x[None]), _t(g[None])
    field, origin, voxel = reconstruct.imls_field(xd, gd, R)
    mesh = reconstruct.surface_nets(field, origin, voxel)
    ms = MeshSet.from_meshes([pm.icosphere(4)]).to(_dev())
    err = reconstruct.mesh_error(*mesh[:4], ms, samples=2048)
    v = float(voxel[0])
    for key in ("to_reference_mean", "to_reference_rms", "to_reference_max", "to_reconstruction_mean", "to_reconstruction_rms",
                "to_reconstruction_max"):
        assert err[key].shape == (1,) and torch.isfinite(err[key]).all(), key
    print("mesh_error: voxel %.4f, %s" % (v, {k: float(t[0]) for k, t in err.items()}))
    assert 0 < float(err["to_reference_mean"][0]) < v and 0 < float(err["to_reconstruction_mean"][0]) < v
    assert float(err["to_reference_mean"][0]) <= float(err["to_reference_rms"][0]) <= float(err["to_reference_max"][0])


def test_the_distance_command(tmp_path, capsys):
    from pdgn_amd import meshes
    ms = meshes.MeshSet.from_meshes([pm.icosphere(2), pm.torus_grid(16, 8)])
    ms.save(tmp_path / "set.npz")
    unit, _ = rm.fibonacci_sphere(128)
    np.save(tmp_path / "clouds.npy", np.stack([unit, unit]).transpose(0, 2, 1))        # (S,3,N) as the test phase saves them
    meshes.main(["distance", str(tmp_path / "clouds.npy"), str(tmp_path / "set.npz"), "--shape", "0,0", "--device", "cuda:0"])
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 4 and lines[0].split()[:2] == ["cloud", "accuracy_mean"] and lines[3].split()[0] == "mean"
    assert float(lines[1].split()[1]) == float(lines[2].split()[1]) <= pm.icosphere_sag(2) + 1e-6


def test_a_report_with_fidelity_and_one_without(tmp_path):
    """fidelity.csv of a report on a tiny mesh set whose reference clouds are draw 0 of its shapes, normalised cloud by cloud; the floor is
    checked at construction (a set in another frame is refused); the report without the option writes the files it wrote before, and the
    one with it the same sheet and the same metrics beside the new file."""
    from pdgn_amd.data import normalize_clouds
    from pdgn_amd.meshes import MeshSet
    from pdgn_amd.report import SnapshotReporter
    from pdgn_amd.trainer import PDGNTrainer
    dev = _dev()
    rng = np.random.default_rng(61)
    shapes = [pm.icosphere(1), pm.torus_grid(12, 6), pm.icosphere(2, 0.7), pm.torus_grid(9, 5, 0.8, 0.3), pm.random_triangles(30, rng), pm.icosphere(0)]
    ms = MeshSet.from_meshes(shapes).to(dev)
    raw = ms.sample(2048, 4, draw=0)
    val, shift, scale = normalize_clouds(raw, "shape_bbox")
    val = val.contiguous()
    framed = ms.in_frame(shift.reshape(-1, 3), scale.reshape(-1))
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    common = dict(every=1, batch_size=4, normalize="shape_bbox", seed=9, rows=3, cell=64)
    with pytest.raises(ValueError, match="do not lie on"):
        SnapshotReporter(tr, val, tmp_path / "bad", fidelity=ms, **common)                  # the raw frame
    with pytest.raises(ValueError, match="MeshSet of the 5 reference"):
        SnapshotReporter(tr, val[:5].contiguous(), tmp_path / "bad", fidelity=framed, **common)
    plain = SnapshotReporter(tr, val, tmp_path / "plain", **common)
    with_it = SnapshotReporter(tr, val, tmp_path / "with", fidelity=framed, **common)
    for epoch in (1, 2):
        plain(epoch), with_it(epoch)
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["metrics.csv", "preview_1.png", "preview_2.png"]
    assert sorted(p.name for p in (tmp_path / "with").iterdir()) == ["fidelity.csv", "metrics.csv", "preview_1.png", "preview_2.png"]
    assert not (tmp_path / "bad").exists()
    for name in ("preview_1.png", "preview_2.png"):
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "with" / name).read_bytes()
    strip = lambda text: [line.rsplit(",", 1)[0] for line in text.splitlines()]            # (the last column is the seconds the report took)
    assert strip((tmp_path / "plain" / "metrics.csv").read_text()) == strip((tmp_path / "with" / "metrics.csv").read_text())
    lines = (tmp_path / "with" / "fidelity.csv").read_text().splitlines()
    assert lines[0] == ",".join(SnapshotReporter.FIDELITY_HEADER) and len(lines) == 3 and [l.split(",")[0] for l in lines[1:]] == ["1", "2"]
    row = [float(v) for v in lines[1].split(",")[1:]]
    most = max(float(val.abs().max()), float(framed.verts.abs().max()))
    assert 0 <= row[3] <= row[4] <= row[5] <= SnapshotReporter.FIDELITY_FLOOR_ULPS * ULP * most           # the floor: the val clouds lie on their shapes
    assert row[5] < row[0] <= row[1] <= row[2] and np.isfinite(row).all()                   # an untrained generator's clouds do not
    assert lines[1].split(",")[1:] == lines[2].split(",")[1:]                             # nothing was trained in between: the same clouds
    assert with_it.last_fidelity[0] == 2 and with_it.last_fidelity[2] == with_it.fidelity_floor
