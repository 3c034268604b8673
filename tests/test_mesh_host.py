"""CPU: the mesh feeder's host side -- the ABI's two entry points, the .obj reader, the alias tables of
pdgn_amd.meshes.MeshSet against the areas they encode, the face and barycentric draws of tests/mesh_mirror.py against their
distributions, the closed-form surface normalisation against data.normalize_clouds of a large sample, packing and the refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_mirror as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- 1. ABI
def test_abi_declares_and_exports_the_mesh_entry_points():
    from pdgn_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    handle = ctypes.CDLL(build.build())
    vp, ull, ll, i = ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_int
    want = {"pdgn_feed_batch_mesh": (i,) * 8 + (vp,) * 5 + (ll, ull, ull, ll, ctypes.c_float) + (vp,) * 8,
            "pdgn_sample_surface": (i, i, vp, vp, vp, vp, ull, ull, vp, vp, vp)}
    for name, argtypes in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S)), name
        assert _lib.SIGNATURES[name] == (ctypes.c_int, argtypes), name
        assert hasattr(handle, name), name
    define = re.findall(r"^#define\s+PDGN_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M)
    assert len(define) == 1 and int(define[0]) == _lib.ABI_VERSION == handle.pdgn_abi_version() >= 37


# ---------------------------------------------------------------------------- 2. the .obj reader
OBJ = """# a comment
mtllib nothing.mtl
g group
v 0 0 0
v 1 0 0   # a trailing comment
v 1 1 0
v 0 1 0
vn 0 0 1
vt 0.5 0.5
usemtl shiny
f 1 2 3
f 1/1/1 2/2/2 3/3/3
f 1//1 3//1 4//1
f 1 2 3 4
v 0.5 2 0
f 1 2 3 4 5
f -1 -2 -3
f -5/1 -4/2 -3
s off
"""


def test_obj_reader(tmp_path):
    from pdgn_amd.meshes import load_obj
    (tmp_path / "a.obj").write_text(OBJ)
    verts, faces = load_obj(tmp_path / "a.obj")
    assert verts.dtype == np.float32 and faces.dtype == np.int32
    assert np.array_equal(verts, np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 2, 0]], dtype=np.float32))
    assert faces.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3],                 # a triangle, a/b/c, a//c
                              [0, 1, 2], [0, 2, 3],                            # the quad, as a fan
                              [0, 1, 2], [0, 2, 3], [0, 3, 4],                 # the pentagon
                              [4, 3, 2], [0, 1, 2]]                            # negative indices: relative to the five vertices read so far
    # a negative index counts from the vertices read SO FAR
    (tmp_path / "b.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf -3 -2 -1\nv 5 5 5\nv 6 5 5\nv 5 6 5\nf -3 -2 -1\n")
    assert load_obj(tmp_path / "b.obj")[1].tolist() == [[0, 1, 2], [3, 4, 5]]
    for bad in ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 -4\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n"):
        (tmp_path / "bad.obj").write_text(bad)
        with pytest.raises(ValueError, match="bad.obj"):
            load_obj(tmp_path / "bad.obj")


# ---------------------------------------------------------------------------- 3. alias tables
def _areas_with_zeros(F, rng):
    areas = 2.0 ** rng.uniform(-10, 0, F)
    areas[0] = 1.0
    if F >= 2:
        areas[1] = 2.0 ** -10
    zeros = {1: [], 2: [1], 4: [2], 37: [3, 17, 36], 1000: [0, 5, 500, 501, 999]}[F]
    areas[zeros] = 0.0
    if F == 1000:
        areas[1] = 1.0                                           # (face 0 is empty here: keep the span 2^-10 .. 1)
    return areas


def implied_probabilities(thr, alias):
    """p_f = (thr_f + sum over g with alias_g = f of (2^32 - thr_g)) / (F 2^32), in exact integer arithmetic until the last division."""
    F = len(thr)
    num = [int(t) for t in thr]
    for g in range(F):
        num[int(alias[g])] += (1 << 32) - int(thr[g])
    assert sum(num) == F << 32
    return num


@pytest.mark.parametrize("F", [1, 2, 4, 37, 1000])
def test_alias_tables_encode_the_areas(F):
    from pdgn_amd.meshes import MeshSet, face_areas
    rng = np.random.default_rng(F)
    ms = MeshSet.from_meshes([mm.soup_with_areas(_areas_with_zeros(F, rng), rng), mm.soup_with_areas([0.5, 0.0, 0.25], rng)])
    assert ms.S == 2 and ms.F == F + 3 and ms.face_off.tolist() == [0, F, F + 3]
    thr, alias = ms.alias_records()
    area = face_areas(ms.verts.numpy(), ms.faces.numpy())
    assert (area[:F] == 0).sum() == {1: 0, 2: 1, 4: 1, 37: 3, 1000: 5}[F]
    for a, b in ((0, F), (F, F + 3)):                            # every shape has its own table, its aliases local to it
        n = b - a
        assert alias[a:b].max() < n
        num = implied_probabilities(thr[a:b], alias[a:b])
        want = area[a:b] / area[a:b].sum()
        err = sum(abs(num[f] / float(n << 32) - want[f]) for f in range(n))
        assert err <= 2.0 ** -30, err
        for f in range(n):
            if area[a + f] == 0.0:
                assert num[f] == 0 and thr[a + f] == 0 and not np.any(alias[a:b] == f)       # probability exactly zero


# ---------------------------------------------------------------------------- 4. face selection through the mirror
@pytest.mark.parametrize("seed", [9999, 1234567891011])
def test_faces_are_drawn_in_proportion_to_their_areas(seed):
    """One shape of 512 faces, areas log-uniform in [2^-8, 1], 2^20 draws: the smallest expected count is about 40, so Pearson's chi^2
    against n * a_f has dof = 511 degrees of freedom, mean dof and variance 2 dof; chi^2 / dof must lie in 1 +- 5 sqrt(2 / dof)."""
    from pdgn_amd.meshes import MeshSet, face_areas
    rng = np.random.default_rng(4)
    F, n = 512, 1 << 20
    ms = MeshSet.from_meshes([mm.soup_with_areas(2.0 ** rng.uniform(-8, 0, F), rng)])
    m = mm.Arrays(ms)
    w0, w1, _, _ = mm.words(seed, [0], n, 0, 0, mm.TAG_SURFACE)
    counts = np.bincount(mm.select_faces(m, np.zeros(1, dtype=np.int64), w0, w1).reshape(-1), minlength=F)
    area = face_areas(m.verts, m.faces)
    expected = n * area / area.sum()
    assert expected.min() > 30
    dof = F - 1
    chi2 = float(((counts - expected) ** 2 / expected).sum()) / dof
    print("chi^2 / dof = %.4f (bound 1 +- %.4f)" % (chi2, 5 * np.sqrt(2.0 / dof)))
    assert abs(chi2 - 1.0) <= 5 * np.sqrt(2.0 / dof), chi2


# ---------------------------------------------------------------------------- 5. the barycentric draw
def test_barycentric_draw_is_uniform_on_the_triangle():
    """Uniform on the triangle = Dirichlet(1,1,1): E[u^a v^b] = 2 a! b! / (a + b + 2)!, so E u = E v = 1/3, E u^2 = 1/6, E uv = 1/12,
    Var u = 1/18, Var u^2 = 1/15 - 1/36, Var uv = 1/90 - 1/144; the sample means of 2^18 draws within five standard errors."""
    n = 1 << 18
    _, _, w2, w3 = mm.words(77, [0], n, 0, 0, mm.TAG_SURFACE)
    a, b, u, v = mm.barycentric(w2, w3)
    assert a.min() >= 0 and b.min() >= 0 and (a + b).max() <= 1 << 24           # exactly inside, as integers
    assert u.dtype == v.dtype == np.float32
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, a) and np.array_equal(v.astype(np.float64) * 2.0 ** 24, b)
    assert (u >= 0).all() and (v >= 0).all() and (u.astype(np.float64) + v.astype(np.float64) <= 1.0).all()
    u, v = u.astype(np.float64).reshape(-1), v.astype(np.float64).reshape(-1)
    for name, x, mean, var in (("u", u, 1 / 3, 1 / 18), ("v", v, 1 / 3, 1 / 18), ("u^2", u * u, 1 / 6, 1 / 15 - 1 / 36),
                               ("uv", u * v, 1 / 12, 1 / 90 - 1 / 144)):
        se = np.sqrt(var / n)
        print("%-4s mean %.6f, expected %.6f, %.2f standard errors" % (name, x.mean(), mean, (x.mean() - mean) / se))
        assert abs(x.mean() - mean) <= 5 * se, name
    # and the point is that combination of the corners
    from pdgn_amd.meshes import MeshSet
    tri = (np.asarray([[1, 2, 3], [2, 2, 3], [1, 4, 3]], dtype=np.float32), np.asarray([[0, 1, 2]], dtype=np.int32))
    p, gf = mm.sample_surface(mm.Arrays(MeshSet.from_meshes([tri])), 4096, 77)
    assert (gf == 0).all()
    assert np.array_equal(p[0, :, 0], np.float32(1) + u[:4096].astype(np.float32)) and np.array_equal(p[0, :, 1], np.float32(2) + v[:4096].astype(np.float32) * np.float32(2))
    assert (p[0, :, 2] == 3).all()


# ---------------------------------------------------------------------------- 6. the surface normalisation
def _tetrahedron():
    v = np.asarray([[1, 1, 1], [3, 1.5, 1], [1.5, 4, 1.25], [2, 2, 5]], dtype=np.float32)
    return v, np.asarray([[0, 1, 2], [0, 1, 3], [1, 2, 3], [0, 2, 3]], dtype=np.int32)


def _cube():
    v = np.asarray([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float32) + np.float32([2, -3, 0.5])
    quads = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    return v, np.asarray([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)


def _random200():
    rng = np.random.default_rng(6)
    v = (rng.standard_normal((120, 3)) * (1.0, 0.5, 2.0) + (0.3, -1.0, 2.0)).astype(np.float32)
    return v, np.stack([rng.permutation(120)[:3] for _ in range(200)]).astype(np.int32)


def test_surface_normalisation_is_the_limit_of_the_point_normalisation():
    """Closed-form shift / scale of 'shape_unit' against data.normalize_clouds of 2^18 mirror samples of the raw surface.  The sample's
    per-axis mean has a standard error of (the axis' std) / 2^9 <= 2e-3 scale and its std a relative one below 2e-3: both are held to
    1e-2 (of the scale: the unit a shift is measured in), five standard errors with room."""
    from pdgn_amd.data import normalize_clouds
    from pdgn_amd.meshes import MeshSet
    shapes = [_tetrahedron(), _cube(), _random200()]
    raw = MeshSet.from_meshes(shapes)
    unit = MeshSet.from_meshes(shapes, normalize="shape_unit")
    assert raw.normalize is None and torch.equal(raw.shift, torch.zeros(3, 3)) and torch.equal(raw.scale, torch.ones(3))
    pts, _ = mm.sample_surface(mm.Arrays(raw), 1 << 18, 31)
    _, shift, scale = normalize_clouds(torch.from_numpy(pts), "shape_unit")
    for c in range(3):
        d = (unit.shift[c] - shift[c, 0]).abs().max().item() / scale[c].item()
        r = abs(unit.scale[c].item() / scale[c].item() - 1.0)
        print("shape %d: shift off by %.2e scale, scale by %.2e relative" % (c, d, r))
        assert d <= 1e-2 and r <= 1e-2, (c, d, r)
    # the cube's are known: its centre, and per axis E x^2 = 1/4 + (4 / 6) / 12 about it (two faces at +-1/2, four spanning the axis)
    assert np.allclose(unit.shift[1].numpy(), [2.5, -2.5, 1.0], atol=1e-6)
    cube = mm.Arrays(unit)
    used = np.unique(cube.faces[cube.face_off[1]:cube.face_off[2]])
    assert np.allclose(np.abs(cube.verts[used]), 0.5 / unit.scale[1].item(), rtol=1e-6)          # the normalised vertices
    # the stored vertices are (raw - shift) / scale, and the normalised surface is centred (its pooled std is not one: the point
    # normalisation divides by the std of the UNSHIFTED coordinates, and so does this)
    for c in range(3):
        used = np.unique(cube.faces[cube.face_off[c]:cube.face_off[c + 1]])
        want = (raw.verts.numpy()[used].astype(np.float64) - unit.shift[c].numpy().astype(np.float64)) / float(unit.scale[c])
        assert np.allclose(cube.verts[used], want, rtol=1e-5, atol=1e-6)
    pts, _ = mm.sample_surface(cube, 1 << 16, 31)
    assert np.abs(pts.astype(np.float64).mean(axis=1)).max() <= 5 * 1.5 / 2 ** 8     # (no axis' std exceeds 1.5 of the pooled one here)
    # shape_bbox: the vertex box of the faces of positive area, exactly what normalize_clouds makes of those vertices
    v, f = _tetrahedron()
    far = np.concatenate([v, np.float32([[100, 100, 100]])])     # a vertex only a degenerate face names does not count
    box = MeshSet.from_meshes([(far, np.concatenate([f, np.int32([[0, 4, 4]])])), _cube()], normalize="shape_bbox")
    for c, vv in enumerate((v, _cube()[0])):
        _, shift, scale = normalize_clouds(torch.from_numpy(vv)[None], "shape_bbox")
        assert torch.equal(box.shift[c], shift[0, 0]) and torch.equal(box.scale[c], scale[0, 0, 0])
    b = mm.Arrays(box)
    used = np.unique(b.faces[b.face_off[1]:b.face_off[2]])
    assert b.verts[used].min() == -1.0 and b.verts[used].max() == 1.0
    for mode in ("global_unit", "shape_half", "shape_34", "unit"):
        with pytest.raises(ValueError, match="normalize"):
            MeshSet.from_meshes(shapes, normalize=mode)


# ---------------------------------------------------------------------------- 7. packing and refusals
def _write_obj(path, verts, faces):
    with open(path, "w") as f:
        for v in verts:
            f.write("v %r %r %r\n" % tuple(float(x) for x in v))
        for t in faces:
            f.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


def test_pack_round_trips_a_directory(tmp_path):
    from pdgn_amd import meshes
    rng = np.random.default_rng(8)
    made = {}
    for sid in ("03001627", "02691156"):
        for split, count in (("train", 3), ("val", 1), ("test", 2)):
            (tmp_path / "obj" / sid / split).mkdir(parents=True)
            for name in ["m%02d" % j for j in range(count)][::-1]:          # written in reverse: read in sorted order
                v, f = mm.random_mesh(int(rng.integers(1, 9)), rng)
                _write_obj(tmp_path / "obj" / sid / split / (name + ".obj"), v, f)
                made[(sid, split, name)] = (v, f)
    (tmp_path / "obj" / "03001627" / "train" / "notes.txt").write_text("not a mesh")
    assert meshes.is_mesh_root(tmp_path / "obj")
    meshes.main(["pack", str(tmp_path / "obj"), str(tmp_path / "packed.npz")])
    assert meshes.is_mesh_root(tmp_path / "packed.npz")
    with np.load(tmp_path / "packed.npz") as f:
        assert sorted(f.files) == sorted("%s/%s/%s" % (sid, sp, k) for sid in ("03001627", "02691156") for sp in ("train", "val", "test")
                                         for k in ("verts", "faces", "face_off"))
    loaded, read = meshes.load_packed(tmp_path / "packed.npz"), meshes.read_obj_root(str(tmp_path / "obj"))
    for sid in ("03001627", "02691156"):
        for split, count in (("train", 3), ("val", 1), ("test", 2)):
            verts, faces, face_off = loaded[sid][split]
            assert verts.dtype == np.float32 and faces.dtype == np.int32 and face_off.dtype == np.int32 and face_off.shape == (count + 1,)
            for x, y in zip(loaded[sid][split], read[sid][split]):
                assert x.dtype == y.dtype and np.array_equal(x, y)
            vat = 0
            for j in range(count):                               # shape j of the split IS file m<j>.obj, bit for bit
                v, f = made[(sid, split, "m%02d" % j)]
                assert np.array_equal(faces[face_off[j]:face_off[j + 1]] - vat, f)
                assert np.array_equal(verts[vat:vat + len(v)].view(np.uint32), v.view(np.uint32))
                vat += len(v)
            assert vat == len(verts)
    assert sorted(meshes.load_packed(tmp_path / "packed.npz", {"02691156"})) == ["02691156"]
    ms = meshes.split_meshset(loaded, "train", "shape_unit")
    assert ms.S == 6 and ms.normalize == "shape_unit"
    ms.save(tmp_path / "set.npz")
    back = meshes.MeshSet.load(tmp_path / "set.npz")
    assert back.normalize == "shape_unit" and (back.S, back.V, back.F) == (ms.S, ms.V, ms.F)
    for k in meshes.MeshSet._FIELDS:
        assert torch.equal(getattr(back, k), getattr(ms, k)) and getattr(back, k).dtype == getattr(ms, k).dtype, k


def test_meshset_refuses_what_the_kernels_would_trust():
    from pdgn_amd.meshes import MeshSet
    rng = np.random.default_rng(9)
    good = mm.random_mesh(5, rng)
    v, f = mm.random_mesh(4, rng)
    flat = f.copy()
    flat[:, 2] = flat[:, 1]
    nan = v.copy()
    nan[1, 2] = np.nan
    beyond = f.copy()
    beyond[2, 0] = len(v)
    for bad, what in (((v, flat), "positive area"), ((nan, f), "finite"), ((v, beyond), "vertex"), ((v, f[:0]), "positive area")):
        with pytest.raises(ValueError, match="shape 1.*" + what):
            MeshSet.from_meshes([good, bad, good])
        with pytest.raises(ValueError, match=r"shape 1 \(lamp\).*" + what):
            MeshSet.from_meshes([good, bad, good], names=["chair", "lamp", "sofa"])
    assert MeshSet.from_meshes([good, (v, f), good]).S == 3


def test_open_data_root_is_unchanged_on_clouds(tmp_path):
    from pdgn_amd import meshes, train
    rng = np.random.default_rng(10)
    clouds = {"03001627/train": rng.standard_normal((3, 8, 3)).astype(np.float32), "03001627/test": rng.standard_normal((2, 8, 3)).astype(np.float32)}
    np.savez(tmp_path / "clouds.npz", **clouds)
    assert not meshes.is_mesh_root(tmp_path / "clouds.npz")
    got = train.open_data_root(str(tmp_path / "clouds.npz"))
    assert sorted(got) == ["03001627"] and sorted(got["03001627"]) == ["test", "train"]
    for key, want in clouds.items():
        sid, split = key.split("/")
        assert np.array_equal(got[sid][split], want)
    for j in range(3):
        (tmp_path / "pc" / "03001627" / "train").mkdir(parents=True, exist_ok=True)
        np.save(tmp_path / "pc" / "03001627" / "train" / ("c%d.npy" % j), clouds["03001627/train"][j])
    assert not meshes.is_mesh_root(tmp_path / "pc")
    got = train.open_data_root(str(tmp_path / "pc"))
    assert sorted(got) == ["03001627"] and np.array_equal(got["03001627"]["train"], clouds["03001627/train"])
    assert train.open_data_root("/some/where/shapenet.hdf5") == "/some/where/shapenet.hdf5" and not meshes.is_mesh_root("/some/where/shapenet.hdf5")
