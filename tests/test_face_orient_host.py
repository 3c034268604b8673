"""CPU: the host side of face orientation from visibility -- the definition of pdgn_mesh_face_votes as
tests/face_orient_mirror.py spells it, on the pixel grid by hand and on meshes with a known outward side, the decision rule, what a MeshSet
does with its flips, and packing and the command line with the device call replaced by the mirror."""
import ctypes
import os
import re

import numpy as np
import pytest

import face_orient_mirror as fm
import visible_cases as vc
import visible_mirror as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- 1. ABI
def test_abi_declares_and_exports_the_votes_entry_point():
    from pdgn_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdgn_hip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(build.build())
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert re.search(r"\bint\s+pdgn_mesh_face_votes\s*\(", text)
    assert _lib.SIGNATURES["pdgn_mesh_face_votes"] == (ctypes.c_int, (i, i, i, vp, vp, vp, vp, vp, i, i, vp, vp, vp))
    assert hasattr(handle, "pdgn_mesh_face_votes")
    assert _lib.ABI_VERSION == handle.pdgn_abi_version() >= 50
    assert "%d entry points" % len(_lib.SIGNATURES) in open(os.path.join(ROOT, "README.md")).read()


# ---------------------------------------------------------------------------- 2. the mirror on the pixel grid, by hand
def _votes(mesh, views, R, frame=None):
    from pdgn_amd.meshes import default_views, shape_frames
    verts, faces, off = vc.pack_set([mesh])
    table = default_views(views) if np.ndim(views) == 0 else views
    return fm.votes(verts, faces, off, shape_frames(verts, faces, off) if frame is None else frame, table, R)


def test_votes_on_the_pixel_grid_by_hand():
    """visible_cases.grid_shape under the identity view at R = 16, a unit a pixel.  Every face is stored counter-clockwise in the (x, y)
    plane: its normal points along +z, away from the eye, so the view sees its BACK.  The half at z = 0.5 covers the 136 centres with
    px <= py: the 16 on the diagonal lie behind the half at z = 0 and (8, 9) behind the triangle at z = -1, which leaves 119; the half at
    z = 0 covers the 136 with px >= py and loses (8, 8) and (9, 8) to that triangle: 134.  The triangle at z = -1 is in front of
    everything at its three centres; the sub-pixel face votes once through the fallback; the triangle at z = 1, the corner triangle at
    z = 2 (occluded) and the needle (dead) vote nothing."""
    verts, faces = vc.grid_shape()
    frame = np.asarray([[0, 0, 0, vc.GRID_RHO]], dtype=np.float32)
    eye = np.eye(3, dtype=np.float32)[None]
    front, back, mask = _votes((verts, faces), eye, 16, frame)
    assert front.dtype == back.dtype == mask.dtype == np.uint32
    assert front.tolist() == [0] * 7 and back.tolist() == [119, 134, 0, 3, 1, 0, 0]
    assert mask.tolist() == vc.GRID_MASKS == vm.visibility(verts, faces, [0, 7], frame, eye, 16).tolist()
    # two faces read the other way round: their votes change columns, nothing else moves
    turned = faces.copy()
    turned[[1, 3]] = turned[[1, 3]][:, [0, 2, 1]]
    front, back, mask2 = _votes((verts, turned), eye, 16, frame)
    assert front.tolist() == [0, 134, 0, 3, 0, 0, 0] and back.tolist() == [119, 0, 0, 0, 1, 0, 0] and mask2.tolist() == mask.tolist()
    # seen from the other side (x kept, y and z turned about x): the same faces show their fronts
    behind = np.asarray([[[1, 0, 0], [0, -1, 0], [0, 0, -1]]], dtype=np.float32)
    front, back, _ = _votes((verts, faces), behind, 16, frame)
    assert not back.any() and front[0] > 100 and front[2] > 0 and front[4] == 0      # (the sub-pixel face is now behind the halves)


# ---------------------------------------------------------------------------- 3. meshes with a known outward side
def torus(nu=16, nv=8, major=0.7, minor=0.3):
    """A torus about the z axis, outward-oriented: the normal of (a, b, c) is d/du x d/dv."""
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    verts = np.stack([(major + minor * np.cos(v)) * np.cos(u), (major + minor * np.cos(v)) * np.sin(u), minor * np.sin(v)], -1).reshape(-1, 3)
    at = lambda i, j: (i % nu) * nv + j % nv
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            faces += [(a, b, c), (a, c, d)]
    return verts.astype(np.float32), np.asarray(faces, dtype=np.int32)


def _outward(verts, faces, ring=None):
    """Per face: the normal dotted with the direction from the centre (ring: from the nearest point of the circle of that radius)."""
    v = verts.astype(np.float64)
    p0, p1, p2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n, c = np.cross(p1 - p0, p2 - p0), (p0 + p1 + p2) / 3.0
    if ring is not None:
        foot = np.concatenate([c[:, :2] / np.linalg.norm(c[:, :2], axis=1)[:, None] * ring, np.zeros((c.shape[0], 1))], 1)
        c = c - foot
    return (n * c).sum(axis=1)


def _apply(faces, flip):
    return np.where(flip[:, None], faces[:, [0, 2, 1]], faces)


@pytest.mark.parametrize("name", ["box", "sphere", "torus"])
def test_random_flips_are_undone(name):
    from pdgn_amd.meshes import orientation_from_votes
    verts, faces = {"box": lambda: vc.box(-1.0, 1.0, 2), "sphere": lambda: vc.sphere(4), "torus": torus}[name]()
    ring = 0.7 if name == "torus" else None
    if name == "torus":
        assert np.all(_outward(verts, faces, ring) > 0)
    else:
        assert np.any(_outward(verts, faces) < 0)                # as stored, opposite sides have opposite handedness
    rng = np.random.default_rng(0)
    faces = _apply(faces, rng.random(faces.shape[0]) < 0.5)
    front, back, _ = _votes((verts, faces), 26, 32)
    rule = orientation_from_votes(front, back, [0, faces.shape[0]])
    assert not rule["undecided"].any() and rule["undecided_count"].tolist() == [0]
    assert rule["flipped"].tolist() == [int(rule["flip"].sum())] and 0 < rule["flip"].sum() < faces.shape[0]
    assert np.all(_outward(verts, _apply(faces, rule["flip"]), ring) > 0)
    assert not rule["two_sided"].any()


def test_nested_cubes_the_hidden_faces_keep_their_order():
    from pdgn_amd.meshes import orientation_from_votes
    verts, faces = vc.nested_cubes()
    front, back, mask = _votes((verts, faces), 26, 32)
    rule = orientation_from_votes(front, back, [0, 24])
    assert not front[12:].any() and not back[12:].any() and not mask[12:].any()
    assert rule["undecided"].tolist() == [False] * 12 + [True] * 12 and not rule["flip"][12:].any()
    assert rule["undecided_count"].tolist() == [12] and rule["two_sided_count"].tolist() == [0]
    assert np.all(_outward(verts[:24], _apply(faces, rule["flip"])[:12]) > 0)


def test_an_open_quad_is_two_sided():
    from pdgn_amd.meshes import orientation_from_votes
    quad = vc.box((0.0, 0.0, 0.0), (1.0, 1.0, 0.0), sides=[5])
    assert quad[1].shape[0] == 2
    front, back, _ = _votes(quad, 26, 32)
    rule = orientation_from_votes(front, back)
    assert np.all(front > 0) and np.all(back > 0) and rule["two_sided"].tolist() == [True, True]
    assert "flipped" not in rule                                 # (no face_off: no per-shape counts)


def test_the_decision_rule_on_votes_made_by_hand():
    from pdgn_amd.meshes import orientation_from_votes
    front = np.asarray([0, 5, 1, 4, 1, 5, 7, 0, 4000000000], dtype=np.uint32)
    back = np.asarray([0, 5, 4, 1, 5, 1, 0, 7, 1000000000], dtype=np.uint32)
    rule = orientation_from_votes(front, back, [0, 4, 4, 9])
    assert rule["flip"].tolist() == [False, False, True, False, True, False, False, True, False]
    assert rule["undecided"].tolist() == [True, True] + [False] * 7
    assert rule["two_sided"].tolist() == [False, True, True, True, False, False, False, False, True]      # 0/0 no, 5/5 1/4 yes, 1/5 no
    assert rule["flipped"].tolist() == [1, 0, 2] and rule["undecided_count"].tolist() == [2, 0, 0] and rule["two_sided_count"].tolist() == [3, 0, 1]
    assert rule["front"].dtype == np.uint32 and rule["flip"].dtype == bool and rule["flipped"].dtype == np.int64
    with pytest.raises(ValueError):
        orientation_from_votes(front, back[:3])


# ---------------------------------------------------------------------------- 4. a MeshSet with flips
def _flipped_set(normalize=None):
    from pdgn_amd.meshes import MeshSet
    meshes = [vc.sphere(3), vc.nested_cubes(), torus(8, 4)]
    F = sum(f.shape[0] for _, f in meshes)
    flip = np.random.default_rng(5).random(F) < 0.5
    return meshes, flip, MeshSet.from_meshes(meshes, normalize, flip=flip)


@pytest.mark.parametrize("normalize", [None, "shape_unit"])
def test_oriented_exchanges_two_columns_and_shares_the_rest(normalize):
    from pdgn_amd.meshes import MeshSet, face_areas
    meshes, flip, ms = _flipped_set(normalize)
    plain = MeshSet.from_meshes(meshes, normalize)
    assert ms.flip.dtype.is_floating_point is False and np.array_equal(ms.flip.numpy(), flip)
    assert all(np.array_equal(getattr(ms, k).numpy(), getattr(plain, k).numpy()) for k in MeshSet._FIELDS)      # stored only: the geometry is as given
    turned = ms.oriented()
    assert turned.flip is None and turned.visible is None and turned.normalize == normalize
    assert np.array_equal(turned.faces.numpy(), _apply(ms.faces.numpy(), flip)) and turned.faces.is_contiguous()
    assert turned.verts is ms.verts and turned.alias is ms.alias and turned.shift is ms.shift and turned.scale is ms.scale
    # the table may be shared: a face read backwards has the same area, bit for bit, and so the same records
    a, b = face_areas(ms.verts.numpy(), ms.faces.numpy()), face_areas(turned.verts.numpy(), turned.faces.numpy())
    assert a.tobytes() == b.tobytes()
    rebuilt = MeshSet.from_arrays(turned.verts.numpy(), turned.faces.numpy(), turned.face_off.numpy())
    if normalize is None:
        assert rebuilt.alias.numpy().tobytes() == ms.alias.numpy().tobytes()
    # twice: the faces it started from
    again = MeshSet(turned.verts, turned.faces, turned.face_off, turned.alias, turned.shift, turned.scale, flip=ms.flip).oriented()
    assert np.array_equal(again.faces.numpy(), ms.faces.numpy())
    ms.__dict__["_mesh_dist"] = {"stale": 1}
    assert "_mesh_dist" not in ms.oriented().__dict__            # nothing prepared for the old order is carried over
    with pytest.raises(ValueError, match="no orientation flips.*pack --orient"):
        plain.oriented()
    with pytest.raises(ValueError, match="orientation flips for %d faces" % ms.F):
        MeshSet.from_meshes(meshes, flip=flip[:-1])


def test_flips_and_masks_travel_together():
    from pdgn_amd.meshes import MeshSet
    meshes, flip, _ = _flipped_set()
    F = flip.shape[0]
    masks = np.ones(F, dtype=np.uint32)
    masks[np.arange(F) % 7 == 3] = 0
    ms = MeshSet.from_meshes(meshes, "shape_unit", visible=masks, flip=flip)
    turned = ms.oriented()
    assert turned.visible is ms.visible and turned.flip is None
    moved = ms.in_frame(np.zeros((ms.S, 3), np.float32), np.full(ms.S, 2.0, np.float32))
    assert moved.flip is ms.flip and np.array_equal(moved.to("cpu").flip.numpy(), flip)


def test_save_and_load_carry_the_flips(tmp_path):
    from pdgn_amd.meshes import MeshSet
    meshes, flip, ms = _flipped_set("shape_unit")
    ms.save(tmp_path / "flipped.npz")
    back = MeshSet.load(tmp_path / "flipped.npz")
    assert back.flip.dtype == ms.flip.dtype and np.array_equal(back.flip.numpy(), flip) and back.visible is None
    assert all(np.array_equal(getattr(back, k).numpy(), getattr(ms, k).numpy()) for k in MeshSet._FIELDS)
    assert np.array_equal(back.oriented().faces.numpy(), ms.oriented().faces.numpy())
    plain = MeshSet.from_meshes(meshes, "shape_unit")
    plain.save(tmp_path / "plain.npz")
    with np.load(tmp_path / "plain.npz") as f:
        assert sorted(f.files) == sorted(MeshSet._FIELDS + ("normalize",))                 # a file without flips is the file it was
    assert MeshSet.load(tmp_path / "plain.npz").flip is None and MeshSet.load(tmp_path / "plain.npz").to("cpu").flip is None


# ---------------------------------------------------------------------------- 5. packing and the command line, the device call replaced by the mirror
def _write_obj(path, verts, faces):
    with open(path, "w") as f:
        for v in verts:
            f.write("v %r %r %r\n" % tuple(float(x) for x in v))
        for t in faces:
            f.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


@pytest.fixture
def mirrored(monkeypatch):
    """pdgn_amd.meshes with face_orientation and face_visibility answered by the mirrors (6 views at R = 16 whatever is asked for); the
    list of the calls made."""
    from pdgn_amd import meshes
    calls = []

    def orientation(verts, faces, face_off, views=26, resolution=128, device=None, return_mask=False):
        calls.append(("orientation", views, resolution, return_mask))
        front, back, mask = fm.votes(verts, faces, face_off, meshes.shape_frames(verts, faces, face_off), meshes.default_views(6), 16)
        out = meshes.orientation_from_votes(front, back, face_off)
        if return_mask:
            out["mask"] = mask
        return out

    def visibility(verts, faces, face_off, views=26, resolution=128, device=None):
        calls.append(("visibility", views, resolution))
        return vm.visibility(verts, faces, face_off, meshes.shape_frames(verts, faces, face_off), meshes.default_views(6), 16)

    monkeypatch.setattr(meshes, "face_orientation", orientation)
    monkeypatch.setattr(meshes, "face_visibility", visibility)
    return meshes, calls


def _obj_root(tmp_path):
    for split, mesh in (("train", vc.nested_cubes()), ("val", vc.box(0.0, 1.0))):
        (tmp_path / "obj" / "03001627" / split).mkdir(parents=True)
        _write_obj(tmp_path / "obj" / "03001627" / split / "a.obj", *mesh)
    return str(tmp_path / "obj")


def test_pack_orient_alone_and_with_visible(tmp_path, capsys, mirrored):
    meshes, calls = mirrored
    root = _obj_root(tmp_path)
    keys = lambda *what: sorted("03001627/%s/%s" % (s, k) for s in ("train", "val") for k in ("verts", "faces", "face_off") + what)
    meshes.main(["pack", root, str(tmp_path / "plain.npz")])
    assert calls == [] and "flipped" not in capsys.readouterr().out
    meshes.main(["pack", root, str(tmp_path / "o.npz"), "--orient", "--views", "6", "--resolution", "64"])
    said = capsys.readouterr().out
    assert calls == [("orientation", 6, 64, False)] * 2
    assert "03001627/train: 6 of 24 faces flipped, 12 undecided, 0 two-sided" in said and "packed 8 arrays" in said, said
    del calls[:]
    meshes.main(["pack", root, str(tmp_path / "vo.npz"), "--visible", "--orient"])
    assert calls == [("orientation", 26, 128, True)] * 2          # one pass serves both
    with np.load(tmp_path / "plain.npz") as p, np.load(tmp_path / "o.npz") as o, np.load(tmp_path / "vo.npz") as vo:
        assert sorted(p.files) == keys() and sorted(o.files) == keys("flip") and sorted(vo.files) == keys("flip", "visible")
        assert all(np.array_equal(p[k], o[k]) and np.array_equal(p[k], vo[k]) for k in p.files)        # the geometry is as read
        assert o["03001627/train/flip"].dtype == bool and np.array_equal(o["03001627/train/flip"], vo["03001627/train/flip"])
        assert vo["03001627/train/visible"].dtype == np.uint32 and not vo["03001627/train/visible"][12:].any()
        flip = o["03001627/train/flip"]
    # the box stores opposite sides with opposite handedness: half its outer faces are turned, the hidden cube is left alone
    assert flip[:12].sum() == 6 and not flip[12:].any()
    verts, faces = vc.nested_cubes()
    assert np.all(_outward(verts, _apply(faces, flip)[:12]) > 0)
    assert meshes.load_packed_flip(str(tmp_path / "plain.npz")) == {} and list(meshes.load_packed_flip(str(tmp_path / "o.npz"))["03001627"]) == ["train", "val"]
    # through split_meshset
    opened, bare = meshes.open_mesh_root(str(tmp_path / "o.npz")), meshes.open_mesh_root(str(tmp_path / "plain.npz"))
    assert meshes.has_stored_flip(opened, "train") and not meshes.has_stored_flip(bare, "train") and bare.flip == {} and not meshes.has_stored_flip(opened, "test")
    assert all(len(t) == 3 for splits in opened.values() for t in splits.values())
    ms = meshes.split_meshset(opened, "train", orient="stored")
    assert np.array_equal(ms.flip.numpy(), flip) and ms.visible is None and meshes.split_meshset(opened, "train").flip is None
    del calls[:]
    both = meshes.split_meshset(bare, "train", visible={"views": 6}, orient={"views": 6})
    assert calls == [("orientation", 6, 128, True)] and np.array_equal(both.flip.numpy(), flip) and both.visible is not None
    del calls[:]
    apart = meshes.split_meshset(bare, "train", visible={"views": 6}, orient={"views": 14})
    assert calls == [("visibility", 6, 128), ("orientation", 14, 128, False)] and np.array_equal(apart.visible.numpy(), both.visible.numpy())
    with pytest.raises(ValueError, match="orient='stored'.*no orientation flips.*pack DIR OUT.npz --orient"):
        meshes.split_meshset(bare, "train", orient="stored")
    with pytest.raises(ValueError, match="orient is None, a dict"):
        meshes.split_meshset(bare, "train", orient=True)


def test_the_commands_refuse_orient_where_no_flips_are_stored(tmp_path, mirrored):
    meshes, _ = mirrored
    from pdgn_amd.meshes import MeshSet
    root = _obj_root(tmp_path)
    plain, saved = str(tmp_path / "plain.npz"), str(tmp_path / "set.npz")
    meshes.main(["pack", root, plain])
    MeshSet.from_meshes([vc.box(0.0, 1.0)]).save(saved)
    np.save(tmp_path / "c.npy", np.zeros((1, 8, 3), np.float32))
    for path in (plain, saved):
        for argv in (["check", path, "--orient"], ["occupancy", path, str(tmp_path / "occ.npz"), "--resolution", "8", "--orient"],
                     ["distance", str(tmp_path / "c.npy"), path, "--signed", "--orient"], ["render", path, "-o", str(tmp_path / "s.png"), "--orient"]):
            with pytest.raises(SystemExit, match=r"--orient: .* holds no orientation flips.*pack --orient writes them"):
                meshes.main(argv + ["--device", "cpu"])
    for bad in (["pack", "a", "b", "--views", "6"], ["pack", "a", "b", "--orient", "--views"], ["pack", "a", "b", "--orient", "--what"],
                ["check", plain, "--orient", "6"]):
        with pytest.raises(SystemExit, match="--orient"):
            meshes.main(bad)
    assert "--orient" in meshes.USAGE.splitlines()[0] and all("[--orient]" in line for line in meshes.USAGE.splitlines())
