"""CPU: the host side of visible-surface sampling -- the ABI's entry points, the view table and the frames of
pdgn_amd.meshes, the definition of csrc/visible.hip as tests/visible_mirror.py spells it on scenes with a known answer, and what a
MeshSet makes of a mask: the alias tables, the normalisation, storage, packing and the command line's refusal."""
import ctypes
import os
import re

import numpy as np
import pytest

import visible_cases as vc
import visible_mirror as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- 1. ABI
def test_abi_declares_and_exports_the_visibility_entry_points():
    from pdgn_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdgn_hip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(build.build())
    vp, i = ctypes.c_void_p, ctypes.c_int
    want = {"pdgn_mesh_visibility": (i, i, i, vp, vp, vp, vp, vp, i, i, vp, vp), "pdgn_mesh_visibility_bias_cover": (),
            "pdgn_mesh_visibility_bias_small": (i,)}
    for name, argtypes in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert _lib.SIGNATURES[name] == (ctypes.c_int, argtypes), name
        assert hasattr(handle, name), name
    assert _lib.ABI_VERSION == handle.pdgn_abi_version() >= 39
    # the constants of the definition: the header's, the library's and the mirror's are the same numbers
    assert int(re.search(r"#define\s+PDGN_VISIBLE_BIAS_COVER\s+(\d+)", text).group(1)) == handle.pdgn_mesh_visibility_bias_cover() == vm.BIAS_COVER == 1 << 10
    for R in (16, 17, 100, 128, 192):
        assert handle.pdgn_mesh_visibility_bias_small(R) == vm.bias_small(R) == int(1.5 * (2.0 / R) * 2 ** 20)
    assert handle.pdgn_mesh_visibility_bias_small(15) == handle.pdgn_mesh_visibility_bias_small(193) == -1


# ---------------------------------------------------------------------------- 2. views and frames
@pytest.mark.parametrize("n", [6, 14, 26])
def test_default_views(n):
    from pdgn_amd.meshes import default_views
    v = default_views(n)
    assert v.shape == (n, 3, 3) and v.dtype == np.float32
    assert v.tobytes() == default_views(n).tobytes() == default_views(26)[:n].tobytes()
    gram = np.einsum("vij,vkj->vik", v.astype(np.float64), v.astype(np.float64))
    assert np.abs(gram - np.eye(3)).max() <= 1e-7
    assert np.all(np.linalg.det(v.astype(np.float64)) > 0.99)                        # right-handed, every one
    look = -v[:, 2].astype(np.float64)                                                # where the eye is
    grid = np.rint(look / np.abs(look).max(axis=1)[:, None]).astype(int)
    assert len({tuple(g) for g in grid}) == n and not np.any(np.all(grid == 0, axis=1))
    assert sorted(np.abs(grid).sum(axis=1).tolist()) == sorted([1] * 6 + [3] * min(8, n - 6) + [2] * max(0, n - 14))
    assert not np.signbit(v[v == 0]).any()


def test_views_from_directions_and_refusals():
    from pdgn_amd.meshes import default_views, view_bases
    v = view_bases([[0, 0, 2.0], [1, 2, 3]])
    assert np.array_equal(v[0, 2], [0, 0, -1]) and np.abs(v[1].astype(np.float64) @ v[1].astype(np.float64).T - np.eye(3)).max() <= 1e-7
    with pytest.raises(ValueError):
        default_views(7)
    with pytest.raises(ValueError):
        view_bases([[0, 0, 0]])


def test_shape_frames_on_a_cube_and_a_ragged_set():
    from pdgn_amd.meshes import shape_frames
    v, f = vc.box((1.0, 2.0, 3.0), (3.0, 4.0, 5.0))
    fr = shape_frames(v, f, [0, 12])
    assert fr.dtype == np.float32 and fr.shape == (1, 4)
    assert np.array_equal(fr[0, :3], [2, 3, 4]) and fr[0, 3] == np.float32(np.sqrt(3.0) * (1 + 2.0 ** -10))
    # ragged: a vertex that only a face of zero area names, and one that no face names, do not count
    far = np.asarray([[100, 100, 100], [-50, 0, 0]], dtype=np.float32)
    v2 = np.concatenate([v, far], 0)
    f2 = np.concatenate([f, [[0, 24, 24]]], 0).astype(np.int32)
    tri = np.asarray([[0, 0, 0], [4, 0, 0], [0, 2, 0]], dtype=np.float32)
    verts, faces, off = vc.pack_set([(v2, f2), (tri, np.asarray([[0, 1, 2]], dtype=np.int32)), (tri, np.asarray([[0, 1, 1]], dtype=np.int32))])
    fr = shape_frames(verts, faces, off)
    assert np.array_equal(fr[0], shape_frames(v, f, [0, 12])[0])
    assert np.array_equal(fr[1, :3], [2, 1, 0]) and fr[1, 3] == np.float32(np.sqrt(5.0) * (1 + 2.0 ** -10))
    assert np.array_equal(fr[2], [0, 0, 0, 1])                                         # nothing of positive area: a frame nothing is snapped with
    for c in range(2):                                                                 # every counted vertex is inside the ball
        p = verts[np.unique(faces[off[c]:off[c + 1]][:12])].astype(np.float64)
        assert np.all(np.linalg.norm(p - fr[c, :3], axis=1) < fr[c, 3])


# ---------------------------------------------------------------------------- 3. the mirror on scenes with a known answer
def _mirror(mesh, views, R, frame=None):
    from pdgn_amd.meshes import default_views, shape_frames
    verts, faces, off = vc.pack_set([mesh])
    table = default_views(views) if np.ndim(views) == 0 else views
    return vm.visibility(verts, faces, off, shape_frames(verts, faces, off) if frame is None else frame, table, R)


def test_dead_faces_are_the_faces_of_area_zero():
    from pdgn_amd.meshes import face_areas
    rng = np.random.default_rng(3)
    verts, faces, _ = vc.pack_set(vc.ragged_set())
    collinear = np.asarray([[0, 0, 0], [1, 2, 3], [2, 4, 6], [1e-20, 0, 0], [0, 1e-20, 0]], dtype=np.float32)
    verts = np.concatenate([verts, collinear, (collinear * rng.uniform(1e-30, 1e-10)).astype(np.float32)], 0)
    V = verts.shape[0]
    faces = np.concatenate([faces, [[V - 10, V - 9, V - 8], [V - 10, V - 7, V - 6], [V - 5, V - 4, V - 3], [V - 5, V - 2, V - 1]]], 0)
    dead = vm.dead_faces(verts, faces)
    assert np.array_equal(dead, face_areas(verts, faces) == 0.0) and 3 <= dead.sum() < faces.shape[0]


@pytest.mark.parametrize("views", [6, 26])
def test_mirror_hides_a_cube_inside_a_closed_cube(views):
    mask = _mirror(vc.nested_cubes(), views, 32)
    assert np.all(mask[:12] != 0) and np.all(mask[12:] == 0), mask
    assert np.all(mask < (1 << views))
    if views == 6:                                               # a side of the outer cube is seen by the one view that faces it, at least
        from pdgn_amd.meshes import default_views
        eye = -default_views(6)[:, 2]
        for side in range(6):
            normal = np.zeros(3)
            normal[side // 2] = 1.0 if side % 2 else -1.0
            v = int(np.argmax(eye @ normal))
            assert np.all(mask[2 * side:2 * side + 2] >> v & 1), (side, mask)


def test_mirror_one_face_alone_passes_in_every_view():
    tri = (np.asarray([[0.1, 0.2, 0.3], [1.0, 0.1, -0.2], [0.3, 0.9, 0.5]], dtype=np.float32), np.asarray([[0, 1, 2]], dtype=np.int32))
    for views, R in ((6, 16), (26, 64)):
        assert _mirror(tri, views, R).tolist() == [(1 << views) - 1]


def test_mirror_a_face_edge_on_takes_the_fallback():
    """Seen from +x (view 0 of the table): a wall at x = 0.5, and three triangles in planes through the line of sight (A2 = 0 there):
    one far behind the wall, one just behind it by less than BIAS_SMALL, one beside it in front of nothing."""
    from pdgn_amd.meshes import default_views
    R, rho = 64, 2.0
    views = default_views(6)
    assert np.array_equal(views[0, 2], [-1, 0, 0])
    near = 0.5 - 0.5 * vm.bias_small(R) * rho / 2.0 ** 20         # (half the bias behind the wall)
    wall = vc.box((0.5, -0.5, -0.5), (0.5, 0.5, 0.5), sides=[1])
    edge = lambda x, y: (np.asarray([[x, y, 0.0], [x - 0.05, y, 0.0], [x, y, 0.2]], dtype=np.float32), np.asarray([[0, 1, 2]], dtype=np.int32))
    mesh = vc.join(wall, edge(-0.5, 0.1), edge(near, -0.2), edge(-0.5, 1.0))
    frame = np.asarray([[0, 0, 0, rho]], dtype=np.float32)
    snapped = vm.snap(mesh[0], frame[0], views[0], R)
    for f in (2, 3, 4):
        assert vm._coverage(snapped[mesh[1][f]], R) is None       # no centre covered in this view: the fallback decides
    mask = _mirror(mesh, views, R, frame)
    assert [int(m) & 1 for m in mask] == [1, 1, 0, 1, 1], mask
    assert np.all(mask != 0)                                     # (the view from -x sees what the wall hides)


def test_mirror_on_the_pixel_grid_by_hand():
    """visible_cases.grid_shape under the identity view at R = 16: vertices on pixel centres, corners and the image border."""
    mesh = vc.grid_shape()
    frame = np.asarray([[0, 0, 0, vc.GRID_RHO]], dtype=np.float32)
    snapped = vm.snap(mesh[0], frame[0], np.eye(3, dtype=np.float32), 16)
    assert np.array_equal(snapped[:, :2], np.rint(mesh[0][:, :2].astype(np.float64) * 256 + 2048).astype(np.int64))       # a unit is a pixel
    assert np.array_equal(snapped[:, 2], np.rint(mesh[0][:, 2].astype(np.float64) * 2 ** 17 + 2 ** 20).astype(np.int64))
    py, px, zp = vm._coverage(snapped[mesh[1][3]], 16)
    assert sorted(zip(px.tolist(), py.tolist())) == [(8, 8), (8, 9), (9, 8)] and set(zp.tolist()) == {(1 << 20) - (1 << 17)}
    assert vm._coverage(snapped[mesh[1][4]], 16) is None and len(vm._coverage(snapped[mesh[1][5]], 16)[0]) == 1
    assert len(vm._coverage(snapped[mesh[1][1]], 16)[0]) == 16 * 17 // 2                 # the diagonal's centres are inside: edges are inclusive
    mask = _mirror(mesh, np.eye(3, dtype=np.float32)[None], 16, frame)
    assert mask.tolist() == vc.GRID_MASKS


# ---------------------------------------------------------------------------- 4. a MeshSet with masks
def implied_probabilities(thr, alias):
    """p_f F 2^32 = thr_f + sum over g with alias_g = f of (2^32 - thr_g), in exact integer arithmetic (as tests/test_mesh_host.py)."""
    num = [int(t) for t in thr]
    for g in range(len(thr)):
        num[int(alias[g])] += (1 << 32) - int(thr[g])
    assert sum(num) == len(thr) << 32
    return num


def _nested_set(normalize):
    from pdgn_amd.meshes import MeshSet
    mesh = vc.nested_cubes(2)
    mask = _mirror(mesh, 6, 16)
    assert np.all(mask[:48] != 0) and np.all(mask[48:] == 0)
    other = vc.box((0, 0, 0), (1, 2, 3))
    masks = np.concatenate([mask, np.ones(12, np.uint32)])
    return MeshSet.from_meshes([mesh, other], normalize, visible=masks), MeshSet.from_meshes([vc.box(-1.0, 1.0, 2), other], normalize), masks


@pytest.mark.parametrize("normalize", [None, "shape_unit", "shape_bbox"])
def test_a_masked_meshset_draws_from_the_visible_faces_only(normalize):
    from pdgn_amd.meshes import face_areas
    ms, outer, masks = _nested_set(normalize)
    assert ms.F == 108 and np.array_equal(ms.visible.numpy().view(np.uint32), masks)
    thr, alias = ms.alias_records()
    hidden = np.arange(48, 96)
    assert np.all(thr[hidden] == 0) and not np.isin(alias[:96], hidden).any()
    area = np.where(masks != 0, face_areas(ms.verts.numpy(), ms.faces.numpy()), 0.0)
    for a, b in ((0, 96), (96, 108)):
        num = implied_probabilities(thr[a:b], alias[a:b])
        want = area[a:b] / area[a:b].sum()
        err = sum(abs(num[f] / float((b - a) << 32) - want[f]) for f in range(b - a))
        assert err <= 2.0 ** -30, err
        assert all(num[f] == 0 for f in range(b - a) if masks[a + f] == 0)
    # the normalisation is that of the visible surface: the outer cube alone
    assert np.array_equal(ms.shift.numpy(), outer.shift.numpy()) and np.array_equal(ms.scale.numpy(), outer.scale.numpy())
    assert np.array_equal(ms.verts.numpy()[:54], outer.verts.numpy()[:54])
    st = ms.visible_stats()
    assert st["hidden"].tolist() == [48, 0] and st["faces"].tolist() == [96, 12] and st["total_hidden"] == 48 and st["total_faces"] == 108
    assert abs(st["kept"][0] - 24.0 / 30.0) < 1e-6 and st["kept"][1] == 1.0
    if normalize is None:                                        # (the total is over the set's own coordinates: raw here)
        assert abs(st["total_kept"] - (24.0 + 22.0) / (30.0 + 22.0)) < 1e-6
    assert outer.visible is None and outer.visible_stats()["total_hidden"] == 0


def test_masks_change_the_normalisation_where_hidden_faces_reach_further():
    """shape_bbox: the vertex box is that of the visible faces of positive area."""
    from pdgn_amd.meshes import MeshSet
    mesh = vc.join(vc.box(-1.0, 1.0), vc.box(-3.0, -2.0))
    masks = np.asarray([1] * 12 + [0] * 12, dtype=np.uint32)
    ms, alone = MeshSet.from_meshes([mesh], "shape_bbox", visible=masks), MeshSet.from_meshes([vc.box(-1.0, 1.0)], "shape_bbox")
    assert np.array_equal(ms.shift.numpy(), alone.shift.numpy()) and np.array_equal(ms.scale.numpy(), alone.scale.numpy())
    assert not np.array_equal(MeshSet.from_meshes([mesh], "shape_bbox").shift.numpy(), alone.shift.numpy())


def test_a_shape_with_every_face_masked_is_refused_by_name():
    from pdgn_amd.meshes import MeshSet
    meshes = [vc.box(-1.0, 1.0), vc.box(0.0, 1.0)]
    masks = np.asarray([3] * 12 + [0] * 12, dtype=np.uint32)
    with pytest.raises(ValueError, match=r"shape 1 \(inner\): no visible face of positive area"):
        MeshSet.from_meshes(meshes, names=["outer", "inner"], visible=masks)
    degenerate = (meshes[1][0], np.concatenate([meshes[1][1], [[0, 1, 1]]], 0).astype(np.int32))
    with pytest.raises(ValueError, match="shape 1: no visible face of positive area"):       # (the one visible face has no area)
        MeshSet.from_meshes([meshes[0], degenerate], visible=np.asarray([3] * 12 + [0] * 12 + [1], dtype=np.uint32))
    with pytest.raises(ValueError, match="23 visibility masks for 24 faces"):
        MeshSet.from_meshes(meshes, visible=masks[:23])


def test_save_and_load_carry_the_masks(tmp_path):
    from pdgn_amd.meshes import MeshSet
    ms, outer, masks = _nested_set("shape_unit")
    ms.save(tmp_path / "masked.npz")
    back = MeshSet.load(tmp_path / "masked.npz")
    assert back.normalize == "shape_unit" and back.visible.dtype == ms.visible.dtype and np.array_equal(back.visible.numpy(), ms.visible.numpy())
    for k in MeshSet._FIELDS:
        assert np.array_equal(getattr(back, k).numpy(), getattr(ms, k).numpy()), k
    assert np.array_equal(back.to("cpu").visible.numpy(), ms.visible.numpy())
    outer.save(tmp_path / "plain.npz")
    with np.load(tmp_path / "plain.npz") as f:
        assert sorted(f.files) == sorted(MeshSet._FIELDS + ("normalize",))                 # a file without masks is the file it was
    plain = MeshSet.load(tmp_path / "plain.npz")
    assert plain.visible is None and plain.to("cpu").visible is None and np.array_equal(plain.alias.numpy(), outer.alias.numpy())


# ---------------------------------------------------------------------------- 5. packing and the command line
def _write_obj(path, verts, faces):
    with open(path, "w") as f:
        for v in verts:
            f.write("v %r %r %r\n" % tuple(float(x) for x in v))
        for t in faces:
            f.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


def test_pack_without_visible_writes_the_keys_it_wrote(tmp_path, capsys):
    from pdgn_amd import meshes
    for split, mesh in (("train", vc.nested_cubes()), ("test", vc.box(0.0, 1.0))):
        (tmp_path / "obj" / "03001627" / split).mkdir(parents=True)
        _write_obj(tmp_path / "obj" / "03001627" / split / "a.obj", *mesh)
    meshes.main(["pack", str(tmp_path / "obj"), str(tmp_path / "a.npz")])
    assert "packed 6 arrays" in capsys.readouterr().out
    with np.load(tmp_path / "a.npz") as f:
        assert sorted(f.files) == sorted("03001627/%s/%s" % (s, k) for s in ("train", "test") for k in ("verts", "faces", "face_off"))
    root = meshes.open_mesh_root(str(tmp_path / "a.npz"))
    assert all(len(t) == 3 for splits in root.values() for t in splits.values())
    assert meshes.load_packed_visible(str(tmp_path / "a.npz")) == {} and root.visible == {} and not meshes.has_stored_visible(root, "train")
    with pytest.raises(ValueError, match="visible='stored'.*no visibility masks.*pack"):
        meshes.split_meshset(root, "train", visible="stored")
    with pytest.raises(ValueError, match="visible is None, a dict"):
        meshes.split_meshset(root, "train", visible=True)
    assert meshes.split_meshset(root, "train").visible is None
    for bad in (["pack", "a"], ["pack", "a", "b", "--views", "6"], ["pack", "a", "b", "--visible", "--views"], ["pack", "a", "b", "--what"]):
        with pytest.raises(SystemExit, match="--visible"):
            meshes.main(bad)
    # stored masks come back through load_packed_visible and split_meshset(..., "stored"), the 3-tuples stay 3-tuples
    with np.load(tmp_path / "a.npz") as f:
        arrays = {k: f[k] for k in f.files}
    arrays["03001627/train/visible"] = np.asarray([5] * 12 + [0] * 12, dtype=np.uint32)
    np.savez(tmp_path / "b.npz", **arrays)
    root = meshes.open_mesh_root(str(tmp_path / "b.npz"))
    assert all(len(t) == 3 for splits in root.values() for t in splits.values()) and meshes.is_mesh_root(str(tmp_path / "b.npz"))
    assert meshes.has_stored_visible(root, "train") and not meshes.has_stored_visible(root, "test")
    ms = meshes.split_meshset(str(tmp_path / "b.npz"), "train", "shape_unit", visible="stored")
    assert ms.visible.numpy().view(np.uint32).tolist() == [5] * 12 + [0] * 12 and ms.visible_stats()["total_hidden"] == 12


def test_mesh_visible_with_clouds_is_refused_with_its_reason(tmp_path):
    from pdgn_amd import train
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "clouds.npz", **{"03001627/%s" % s: rng.standard_normal((3, 64, 3)).astype(np.float32) for s in ("train", "val", "test")})
    common = ["--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root", str(tmp_path / "clouds.npz"), "--choice", "chair",
              "--num_point", "64", "--device", "cpu"]
    for phase in ("train", "test"):
        with pytest.raises(SystemExit, match="--mesh_visible on.*point clouds.*per face of a mesh"):
            train.main(common + ["--phase", phase, "--mesh_visible", "on"])
    with pytest.raises(SystemExit):
        train.parse_args(common + ["--mesh_views", "6"])                             # goes with --mesh_visible
    with pytest.raises(SystemExit):
        train.parse_args(common + ["--mesh_visible", "on", "--mesh_visible_res", "200"])
    args = train.parse_args(common + ["--mesh_visible", "compute", "--mesh_views", "14"])
    assert (args.mesh_visible, args.mesh_views, args.mesh_visible_res) == ("compute", 14, 128)
    plain = train.parse_args(common)
    assert plain.mesh_visible == "off" and "mesh_visible" not in vars(plain) and "mesh_views" not in vars(plain)
