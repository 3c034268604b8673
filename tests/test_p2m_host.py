"""Point-to-surface distance on the host: the numpy mirror of csrc/meshdist.hip (tests/p2m_mirror.py) against an
independent float64 oracle, the culling bound with zero exceptions, the order independence and the definition's corner cases, the header's
prototypes, and every refusal of the Python surface that happens before a library call."""
import re

import numpy as np
import pytest
import torch

import p2m_mirror as pm

F = np.float32
ULP = 2.0 ** -24
BOUND = 64.0                                                       # |sqrt(d2_fp32) - d_fp64| <= BOUND * 2^-24 * M, M the largest |coordinate|


def _worst_ratio(verts, faces, points):
    """The largest |sqrt(d2) - d_oracle| / (2^-24 M) of the points against the whole mesh."""
    d2, face, q = pm.closest_of(points, verts[faces], np.arange(faces.shape[0]))
    oracle = pm.distance_f64(points, verts[faces])
    M = max(float(np.abs(verts[faces]).max()), float(np.abs(points).max()))
    assert np.isfinite(d2).all() and (face >= 0).all()
    # the closest point the mirror reports is at the distance it reports, and inside the face's box
    lo, hi = pm.face_box(*(verts[faces[face]][:, k] for k in range(3)))
    assert ((q >= lo) & (q <= hi)).all()
    return float(np.abs(np.sqrt(d2.astype(np.float64)) - oracle).max() / (ULP * M))


def _mesh(kind, rng):
    if kind == "random":
        return pm.random_triangles(300, rng)
    if kind.startswith("sliver"):
        return pm.slivers(300, rng, float(kind[6:]))
    if kind == "icosphere":
        return pm.icosphere(2)
    return pm.torus_grid(24, 12)


KINDS = ("random", "sliver1e-2", "sliver1e-4", "sliver1e-6", "icosphere", "torus")


@pytest.mark.parametrize("offset", (0.0, 100.0))
@pytest.mark.parametrize("kind", KINDS)
def test_the_mirror_agrees_with_the_float64_oracle(kind, offset):
    """Points far from the mesh, points on faces (barycentric in float64, rounded) and points a sliver's width off them.  Measured worst
    ratio over all cases: 1.6; the bound is 64."""
    rng = np.random.default_rng(11)
    v, f = _mesh(kind, rng)
    on, _ = pm.points_on_faces(v, f, 400, rng)
    width = float(kind[6:]) if kind.startswith("sliver") else 1e-3
    near = on + (rng.standard_normal(on.shape) * width).astype(F)
    move = lambda a: (a.astype(np.float64) + offset).astype(F)
    worst = 0.0
    for name, pts in (("far", rng.uniform(-2, 2, (400, 3)).astype(F)), ("on", on), ("near", near)):
        ratio = _worst_ratio(move(v), f, move(pts))
        print("%s %s offset %g: worst ratio %.3f" % (kind, name, offset, ratio))
        worst = max(worst, ratio)
    assert worst <= BOUND


@pytest.mark.parametrize("kind", KINDS)
def test_points_on_their_own_face(kind):
    """The distance to the OWN face alone (not the minimum over the mesh) of points drawn on it stays within the bound."""
    rng = np.random.default_rng(12)
    v, f = _mesh(kind, rng)
    pts, own = pm.points_on_faces(v, f, 600, rng)
    tri = v[f[own]]
    d2 = np.stack([pm.face_values(pts[i:i + 1], tri[i:i + 1, 0], tri[i:i + 1, 1], tri[i:i + 1, 2])[0][0, 0] for i in range(pts.shape[0])])
    oracle, _ = pm.closest_f64(pts, tri[:, 0], tri[:, 1], tri[:, 2])
    M = max(float(np.abs(v).max()), float(np.abs(pts).max()))
    ratio = float(np.abs(np.sqrt(d2.astype(np.float64)) - oracle).max() / (ULP * M))
    print("%s own face: worst ratio %.3f" % (kind, ratio))
    assert ratio <= BOUND


def test_sampled_points_lie_on_their_own_face():
    """mesh_mirror's sampler (what MeshSet.sample draws): every point within the bound of the face it was drawn from."""
    import mesh_mirror as mm
    from pdgn_amd.meshes import MeshSet
    ms = MeshSet.from_meshes([pm.icosphere(1), pm.torus_grid(9, 7), pm.slivers(40, np.random.default_rng(3), 1e-4)])
    pts, gf = mm.sample_surface(mm.Arrays(ms), 200, 5)
    verts, faces = ms.verts.numpy(), ms.faces.numpy()
    for c in range(ms.S):
        tri = verts[faces[gf[c]]]
        d2 = np.stack([pm.face_values(pts[c, i:i + 1], tri[i:i + 1, 0], tri[i:i + 1, 1], tri[i:i + 1, 2])[0][0, 0] for i in range(200)])
        assert np.sqrt(d2.astype(np.float64)).max() <= BOUND * ULP * float(np.abs(verts).max())


def _nudged(x, rng, most=3):
    """x moved by -most .. most ulps."""
    out = x.copy()
    for _ in range(most):
        step = rng.integers(-1, 2, x.shape)
        out = np.where(step > 0, np.nextafter(out, F(np.inf)), np.where(step < 0, np.nextafter(out, F(-np.inf)), out))
    return out.astype(F)


@pytest.mark.parametrize("offset", (0.0, 100.0))
def test_the_culling_bound_has_no_exception(offset):
    """LB <= d2_f for a point against a face's box, and for a box of points against a box of faces, over random triangles, slivers and a
    torus; with points within a few ulps of the sides and corners of face boxes."""
    rng = np.random.default_rng(13)
    meshes = [pm.random_triangles(128, rng, scale=0.3), pm.slivers(128, rng, 1e-4), pm.torus_grid(16, 4)]
    for v, f in meshes:
        v = (v.astype(np.float64) + offset).astype(F)
        a, b, c = (v[f[:, k]] for k in range(3))
        lo, hi = pm.face_box(a, b, c)
        pick = rng.integers(0, f.shape[0], 256)
        side = np.where(rng.integers(0, 2, (256, 3)) > 0, lo[pick], hi[pick])
        inside = (lo[pick] + (hi[pick] - lo[pick]) * rng.uniform(0, 1, (256, 3)).astype(F)).astype(F)
        mixed = np.where(rng.integers(0, 2, (256, 3)) > 0, side, inside)
        pts = np.concatenate([rng.uniform(-1.5, 1.5, (256, 3)).astype(F) + F(offset), _nudged(side, rng), _nudged(mixed, rng)])
        d2, _ = pm.face_values(pts, a, b, c)                       # (P,F)
        lb = pm.lower_bound(lo[None], hi[None], pts[:, None], pts[:, None])
        assert lb.dtype == F and not (lb > d2).any()
        # boxes of 64 faces against boxes of 64 points: the bound holds for every member pair
        for _ in range(8):
            fs, ps = rng.choice(f.shape[0], 64, replace=False), rng.choice(pts.shape[0], 64, replace=False)
            if rng.integers(0, 2):                                 # coherent sets as well: neighbours in the arrays
                f0, p0 = rng.integers(0, f.shape[0] - 64 + 1), rng.integers(0, pts.shape[0] - 64 + 1)
                fs, ps = np.arange(f0, f0 + 64), np.arange(p0, p0 + 64)
            glb = pm.lower_bound(lo[fs].min(axis=0), hi[fs].max(axis=0), pts[ps].min(axis=0), pts[ps].max(axis=0))
            assert not (glb > d2[np.ix_(ps, fs)]).any()
            flb = pm.lower_bound(lo[fs], hi[fs], pts[ps].min(axis=0)[None], pts[ps].max(axis=0)[None])       # a face against the box of points
            assert not (flb[None, :] > d2[np.ix_(ps, fs)]).any()


@pytest.mark.parametrize("kind", ("random", "sliver1e-4", "torus"))
def test_the_result_does_not_depend_on_the_order_of_the_faces(kind):
    rng = np.random.default_rng(14)
    v, f = _mesh(kind, rng)
    pts = np.concatenate([rng.uniform(-1.5, 1.5, (200, 3)).astype(F), pm.points_on_faces(v, f, 200, rng)[0], v[f[:50, 0]]])
    index = np.arange(f.shape[0])
    want = pm.closest_of(pts, v[f], index, step=97)
    perm = rng.permutation(f.shape[0])
    got = pm.closest_of(pts, v[f[perm]], index[perm], step=64)
    assert all(pm.bits_equal(a, b) for a, b in zip(got, want))


def test_definition_cases():
    v, f = pm.icosphere(0)
    # duplicate faces: the lowest index wins, whatever the order they are visited in
    faces = np.concatenate([f, f[::-1], f])
    off = np.asarray([0, faces.shape[0]], dtype=np.int32)
    rng = np.random.default_rng(15)
    pts = rng.standard_normal((1, 64, 3)).astype(F)
    d2, face, q = pm.point_to_mesh(pts, v, faces, off)
    assert (face < 20).all() and (face >= 0).all()
    # points exactly on shared vertices and edge midpoints (of edges whose midpoint is exact in fp32: halves of sums of neighbours)
    on_vertex = v[:12]
    d2v, facev, qv = pm.point_to_mesh(on_vertex[None], v, f, np.asarray([0, 20], dtype=np.int32))
    assert (d2v == 0).all() and pm.bits_equal(qv[0], on_vertex)
    for i in range(12):
        assert facev[0, i] == min(j for j in range(20) if i in f[j])
    cube_v = np.asarray([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], dtype=F)
    cube_f = np.asarray([(0, 2, 3), (0, 1, 2)], dtype=np.int32)    # the shared edge is the diagonal, its midpoint exact
    mid = np.asarray([[(0.5, 0.5, 0.0), (0.25, 0.25, 0.0), (0.5, 0.5, 2.0)]], dtype=F)
    d2m, facem, qm = pm.point_to_mesh(mid, cube_v, cube_f, np.asarray([0, 2], dtype=np.int32))
    assert (facem == 0).all() and pm.bits_equal(d2m, np.asarray([[0, 0, 4]], dtype=F))
    # dead faces are never returned; a shape whose faces are all dead gives NaN / -1 / NaN
    live = np.ones(20, dtype=np.int32)
    live[::2] = 0
    d2l, facel, _ = pm.point_to_mesh(pts, v, f, np.asarray([0, 20], dtype=np.int32), live=live)
    assert (facel % 2 == 1).all() and (d2l >= pm.point_to_mesh(pts, v, f, np.asarray([0, 20], dtype=np.int32))[0]).all()
    two = np.concatenate([pts, pts])
    off2 = np.asarray([0, 10, 20], dtype=np.int32)
    dead = np.concatenate([np.zeros(10, np.int32), np.ones(10, np.int32)])
    d2d, faced, qd = pm.point_to_mesh(two, v, f, off2, live=dead)
    assert (d2d[0].view(np.uint32) == pm.NAN_BITS).all() and (faced[0] == -1).all() and (qd[0].view(np.uint32) == pm.NAN_BITS).all()
    assert np.isfinite(d2d[1]).all() and (faced[1] >= 10).all()
    # points that are not finite
    bad = pts.copy()
    bad[0, 0, 0], bad[0, 1, 1], bad[0, 2, 2] = np.nan, np.inf, -np.inf
    d2b, faceb, qb = pm.point_to_mesh(bad, v, f, np.asarray([0, 20], dtype=np.int32))
    assert (d2b[0, :3].view(np.uint32) == pm.NAN_BITS).all() and (faceb[0, :3] == -1).all() and (qb[0, :3].view(np.uint32) == pm.NAN_BITS).all()
    assert pm.bits_equal(d2b[0, 3:], d2[0, 3:] if False else pm.point_to_mesh(pts, v, f, np.asarray([0, 20], dtype=np.int32))[0][0, 3:])
    # a degenerate face that is visited all the same (live is the caller's word): clamps with fmax / fmin semantics, no NaN result
    deg_v = np.asarray([(0, 0, 0), (0, 0, 0), (1, 0, 0), (2, 0, 0)], dtype=F)
    deg_f = np.asarray([(0, 1, 1), (0, 2, 3)], dtype=np.int32)
    d2g, faceg, qg = pm.point_to_mesh(pts, deg_v, deg_f, np.asarray([0, 2], dtype=np.int32))
    assert np.isfinite(d2g).all() and np.isfinite(qg).all()


def test_the_header_declares_the_entry_points():
    from pdgn_amd import _lib
    import ctypes
    i, ll, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    assert _lib.ABI_VERSION >= 46
    assert _lib.SIGNATURES["pdgn_mesh_dist_group"] == (i, ()) and _lib.SIGNATURES["pdgn_mesh_dist_chunk"] == (i, ())
    assert _lib.SIGNATURES["pdgn_mesh_dist_workspace_floats"] == (ll, (i, i))
    assert _lib.SIGNATURES["pdgn_mesh_dist_prepare"] == (i, (i, i, i, i) + (vp,) * 8 + (vp,))
    assert _lib.SIGNATURES["pdgn_point_mesh_distance"] == (i, (i,) * 5 + (vp,) * 6 + (i,) + (vp,) * 3 + (vp,))
    handle = ctypes.CDLL(_lib.SO_PATH)
    assert handle.pdgn_mesh_dist_group() == pm.GROUP and handle.pdgn_mesh_dist_chunk() == pm.CHUNK
    handle.pdgn_mesh_dist_workspace_floats.restype = ll
    assert handle.pdgn_mesh_dist_workspace_floats(3, 1000) == 12 * 1000 + 8 * (1000 // 64 + 3)
    assert handle.pdgn_mesh_dist_workspace_floats(0, 10) == -1 and handle.pdgn_mesh_dist_workspace_floats(1, 0) == -1
    assert handle.pdgn_mesh_dist_workspace_floats(1, (1 << 31) // 3 + 1) == -1
    with open(_lib.HEADER) as fh:
        text = fh.read()
    assert re.search(r"csrc/meshdist\.hip", text)


@pytest.fixture
def no_library(monkeypatch):
    """Any library call is a failure: the refusals below come before it."""
    from pdgn_amd import _lib

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


def _set(visible=None):
    from pdgn_amd.meshes import MeshSet
    meshes = [pm.icosphere(0), pm.torus_grid(5, 4)]
    return MeshSet.from_meshes(meshes, visible=visible)


def test_point_to_mesh_refuses_before_any_library_call(no_library):
    from pdgn_amd.meshes import point_to_mesh
    ms = _set()
    x = torch.zeros(2, 7, 3)
    for bad in (x[0], x.double(), torch.zeros(2, 7, 2), x.numpy(), torch.zeros(2, 0, 3)):
        with pytest.raises(ValueError, match="point_to_mesh"):
            point_to_mesh(bad, ms)
    with pytest.raises(ValueError, match="MeshSet"):
        point_to_mesh(x, "meshes.npz")
    with pytest.raises(ValueError, match="3 clouds and 2 shapes"):
        point_to_mesh(torch.zeros(3, 7, 3), ms)
    for bad in (torch.zeros(2), torch.zeros(3, dtype=torch.int64), torch.zeros(2, 1, dtype=torch.int64), [0.0, 1.0]):
        with pytest.raises(ValueError, match="shape is"):
            point_to_mesh(x, ms, shape=bad)
    for bad in ([0, 2], [-1, 0], torch.tensor([5, 0])):
        with pytest.raises(ValueError, match="shape index"):
            point_to_mesh(x, ms, shape=bad)
    with pytest.raises(ValueError, match="visibility masks"):
        point_to_mesh(x, ms, visible_only=True)


def test_surface_fidelity_and_mesh_error_refuse_before_any_library_call(no_library):
    from pdgn_amd.evaluation import surface_fidelity
    from pdgn_amd.losses import surface_distance
    from pdgn_amd.reconstruct import mesh_error
    ms = _set()
    x = torch.zeros(2, 7, 3)
    for bad in (x[0], x.double(), x.numpy()):
        with pytest.raises(ValueError, match="surface_fidelity"):
            surface_fidelity(bad, ms)
    with pytest.raises(ValueError, match="MeshSet"):
        surface_fidelity(x, None)
    with pytest.raises(ValueError, match="samples"):
        surface_fidelity(x, ms, samples=0)
    for bad in ((0.0,), (float("nan"),), (0.01, float("inf"))):
        with pytest.raises(ValueError, match="thresholds"):
            surface_fidelity(x, ms, thresholds=bad)
    with pytest.raises(ValueError, match="shape index"):
        surface_fidelity(x, ms, shape=[0, 9])
    with pytest.raises(ValueError, match="3 clouds and 2 shapes"):
        surface_fidelity(torch.zeros(3, 7, 3), ms)
    with pytest.raises(ValueError, match="visibility masks"):
        surface_fidelity(x, ms, visible_only=True)
    with pytest.raises(ValueError, match="reduction"):
        surface_distance(x, ms, reduction="median")
    v, f = pm.icosphere(0)
    one = (v, f, np.asarray([0, 12]), np.asarray([0, 20]))
    with pytest.raises(ValueError, match="MeshSet"):
        mesh_error(*one, "meshes.npz")
    with pytest.raises(ValueError, match="prefix sums"):
        mesh_error(v, f, np.asarray([0, 12, 12]), np.asarray([0, 20]), ms)
    with pytest.raises(ValueError, match="samples"):
        mesh_error(*one, ms, shape=[0], samples=0)
    with pytest.raises(ValueError, match="1 clouds and 2 shapes"):
        mesh_error(*one, ms)
    with pytest.raises(ValueError, match="shape index"):
        mesh_error(*one, ms, shape=[2])


def test_the_distance_command_refuses_bad_arguments(tmp_path, no_library):
    from pdgn_amd import meshes
    with pytest.raises(SystemExit, match="usage"):
        meshes.main(["distance", "a.npy"])
    np.save(tmp_path / "c.npy", np.zeros((2, 5, 4), dtype=F))
    with pytest.raises(SystemExit, match="clouds are"):
        meshes.main(["distance", str(tmp_path / "c.npy"), str(tmp_path / "m.npz")])
    np.save(tmp_path / "d.npy", np.zeros((2, 5, 3), dtype=F))
    with pytest.raises(SystemExit, match="usage"):
        meshes.main(["distance", str(tmp_path / "d.npy"), str(tmp_path / "m.npz"), "--frobnicate"])
    with pytest.raises(SystemExit, match="integers"):
        meshes.main(["distance", str(tmp_path / "d.npy"), str(tmp_path / "m.npz"), "--shape", "a,b"])
