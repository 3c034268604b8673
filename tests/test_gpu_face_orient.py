"""GPU: pdgn_mesh_face_votes (csrc/visible.hip) -- bit-equality of the votes and the masks with
tests/face_orient_mirror.py on the visibility tests' ragged set at their four (resolution, views) pairs and at the sweep's remainders, the
masks against pdgn_mesh_visibility itself, order-independence and repeatability, the refusals, and what the flips are for: meshes stored
with mixed handedness get a winding number of 1 inside and 0 outside, through MeshSet, packing and the command line."""
import functools

import numpy as np
import pytest
import torch

import face_orient_mirror as fm
import visible_cases as vc
import winding_mirror as wm

pytestmark = pytest.mark.gpu
GUARD, POISON = 64, 0x5A5A5A5A
INVALID = -1


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(verts, faces, off, frame, views, R, stream=None, untouched=False, over=None, entry="pdgn_mesh_face_votes"):
    """The entry point itself into poisoned, guarded buffers -> (rc, votes (F,2) uint32, mask (F) uint32 numpy).  over: replaces an
    argument by name (S V F NV, or a pointer: None for NULL; a NULL mask comes back as None).  entry pdgn_mesh_visibility: the masks of
    that entry point on the same arguments (votes None)."""
    from pdgn_amd import _lib
    dev = _dev()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    a = dict(verts=t(verts, np.float32), faces=t(faces, np.int32), face_off=t(off, np.int32), frame=t(frame, np.float32),
             views=t(np.asarray(views).reshape(-1, 3, 3), np.float32))
    F = int(np.asarray(faces).shape[0])
    whole = torch.full((3 * F + 4 * GUARD,), POISON, dtype=torch.int32, device=dev)
    a.update(S=len(off) - 1, V=int(np.asarray(verts).shape[0]), F=F, NV=int(a["views"].shape[0]), R=R,
             votes=whole[GUARD:GUARD + 2 * F], mask=whole[3 * GUARD + 2 * F:3 * GUARD + 3 * F])
    a.update(over or {})
    p = lambda x: _lib.ptr(x)
    s = torch.cuda.current_stream(dev) if stream is None else stream
    torch.cuda.synchronize()                                     # (the poison is in place before a side stream may run)
    front = (a["S"], a["V"], a["F"], p(a["verts"]), p(a["faces"]), p(a["face_off"]), p(a["frame"]), p(a["views"]), a["NV"], a["R"], p(a["mask"]))
    with torch.cuda.stream(s):
        if entry == "pdgn_mesh_visibility":
            rc = _lib.lib().pdgn_mesh_visibility(*front, _lib.stream_of(whole))
        else:
            rc = _lib.lib().pdgn_mesh_face_votes(*front, p(a["votes"]), _lib.stream_of(whole))
    torch.cuda.synchronize()
    got = whole.cpu().numpy().view(np.uint32)
    written = np.zeros(got.shape[0], dtype=bool)
    if rc == 0 and not untouched:
        written[GUARD:GUARD + 2 * F] = entry != "pdgn_mesh_visibility"
        written[3 * GUARD + 2 * F:3 * GUARD + 3 * F] = a["mask"] is not None
    assert np.all(got[~written] == POISON), "a guard word, or a buffer of a refused call, was written"
    votes = got[GUARD:GUARD + 2 * F].reshape(F, 2).copy() if entry != "pdgn_mesh_visibility" else None
    return rc, votes, (got[3 * GUARD + 2 * F:3 * GUARD + 3 * F].copy() if a["mask"] is not None else None)


def _views(NV):
    from pdgn_amd.meshes import default_views, view_bases
    if NV == 1:                                                  # the identity: the grid shape's units are pixels at R = 16
        return np.eye(3, dtype=np.float32)[None]
    if NV <= 26:
        return default_views(26)[:NV]
    return np.concatenate([default_views(26), view_bases(np.random.default_rng(NV).standard_normal((NV - 26, 3)))], 0)


@functools.lru_cache(maxsize=None)
def _ragged():
    verts, faces, off = vc.pack_set(vc.ragged_set())
    return verts, faces, off, vc.ragged_frames(verts, faces, off)


# ---------------------------------------------------------------------------- 1. bit-equality with the mirror and with the visibility kernel
@pytest.mark.parametrize("R,NV", [(16, 1), (64, 6), (128, 26), (192, 32)])
def test_votes_and_masks_are_bit_equal_to_the_mirror(R, NV):
    """The lane path and the wave path (the twelve-face shape's faces are larger than the image, their vertices clamped), the fallback
    (the slivers), a dead face, 64 KB and 144 KB of LDS."""
    verts, faces, off, frame = _ragged()
    assert np.diff(off).tolist() == [1, 2, 12, 37, 150, 400, 24, 7]
    views = _views(NV)
    rc, votes, mask = _run(verts, faces, off, frame, views, R)
    assert rc == 0
    front, back, want_mask = fm.votes(verts, faces, off, frame, views, R)
    assert np.array_equal(votes[:, 0], front), np.flatnonzero(votes[:, 0] != front)[:20]
    assert np.array_equal(votes[:, 1], back), np.flatnonzero(votes[:, 1] != back)[:20]
    assert np.array_equal(mask, want_mask), np.flatnonzero(mask != want_mask)[:20]
    assert not votes[2].any() and mask[2] == 0                   # the face of zero area in 3D
    assert votes.max() > 32 and np.any(votes.sum(axis=1) == 1)   # a face that a wave counted, and a single vote
    if (R, NV) == (16, 1):                                       # the grid shape, by hand: tests/test_face_orient_host.py
        assert votes[off[-2]:, 0].tolist() == [0] * 7 and votes[off[-2]:, 1].tolist() == [119, 134, 0, 3, 1, 0, 0]
    # the masks are the visibility kernel's, byte for byte, and a caller that wants none passes NULL
    rc, _, seen = _run(verts, faces, off, frame, views, R, entry="pdgn_mesh_visibility")
    assert rc == 0 and seen.tobytes() == mask.tobytes()
    rc, alone, none = _run(verts, faces, off, frame, views, R, over=dict(mask=None))
    assert rc == 0 and none is None and alone.tobytes() == votes.tobytes()


@pytest.mark.parametrize("F", [vc.FACE_STRIDE - 1, vc.FACE_STRIDE, vc.FACE_STRIDE + 1])
def test_sweep_remainders_are_bit_equal_to_the_mirror(F):
    from pdgn_amd.meshes import shape_frames
    rng = np.random.default_rng(F)
    verts, faces, off = vc.pack_set([vc.random_ball(F, rng), vc.random_ball(3, rng)])
    frame, views = shape_frames(verts, faces, off), _views(6)[[0, 5]]
    rc, votes, mask = _run(verts, faces, off, frame, views, 32)
    front, back, want_mask = fm.votes(verts, faces, off, frame, views, 32)
    assert rc == 0 and np.array_equal(votes, np.stack([front, back], 1)) and np.array_equal(mask, want_mask)
    assert np.any(votes[vc.FACE_STRIDE - 2:F] != 0)              # (the faces around the stride's end are not all hidden ones)


# ---------------------------------------------------------------------------- 2. order and repeatability
@functools.lru_cache(maxsize=None)
def _order_case():
    from pdgn_amd.meshes import shape_frames
    rng = np.random.default_rng(33)
    meshes = vc.ragged_set(seed=1, sizes=(1, 37, 600)) + [vc.join(vc.box(-1.0, 1.0, 4), vc.rod(16))]
    verts, faces, off = vc.pack_set(meshes)
    frame = shape_frames(verts, faces, off)
    rc, votes, mask = _run(verts, faces, off, frame, _views(6), 64)
    assert rc == 0 and 0 < np.count_nonzero(votes.sum(axis=1)) < votes.shape[0] and votes[:, 0].any() and votes[:, 1].any()
    return meshes, verts, faces, off, frame, votes, mask, rng.integers(1 << 30)


def test_two_runs_are_byte_equal_and_a_side_stream_gives_the_same():
    meshes, verts, faces, off, frame, votes, mask, _ = _order_case()
    rc, again, again_mask = _run(verts, faces, off, frame, _views(6), 64)
    assert rc == 0 and again.tobytes() == votes.tobytes() and again_mask.tobytes() == mask.tobytes()
    rc, side, side_mask = _run(verts, faces, off, frame, _views(6), 64, stream=torch.cuda.Stream(_dev()))
    assert rc == 0 and side.tobytes() == votes.tobytes() and side_mask.tobytes() == mask.tobytes()
    assert votes.max() <= 6 * 64 * 64 and np.all(mask < 64)      # fully rewritten from the poisoned buffers


def test_permuted_faces_give_permuted_rows_and_reversed_shapes_the_same_rows():
    meshes, verts, faces, off, frame, votes, mask, seed = _order_case()
    rng = np.random.default_rng(seed)
    perms = [rng.permutation(f.shape[0]) for _, f in meshes]
    v2, f2, o2 = vc.pack_set([(v, f[p]) for (v, f), p in zip(meshes, perms)])
    rc, got, got_mask = _run(v2, f2, o2, frame, _views(6), 64)
    assert rc == 0
    for c, p in enumerate(perms):
        assert np.array_equal(got[off[c]:off[c + 1]], votes[off[c]:off[c + 1]][p]), c
        assert np.array_equal(got_mask[off[c]:off[c + 1]], mask[off[c]:off[c + 1]][p]), c
    v3, f3, o3 = vc.pack_set(meshes[::-1])
    rc, got, got_mask = _run(v3, f3, o3, frame[::-1], _views(6), 64)
    assert rc == 0
    S = len(meshes)
    for c in range(S):
        assert np.array_equal(got[o3[S - 1 - c]:o3[S - c]], votes[off[c]:off[c + 1]]), c
        assert np.array_equal(got_mask[o3[S - 1 - c]:o3[S - c]], mask[off[c]:off[c + 1]]), c


# ---------------------------------------------------------------------------- 3. refusals
def test_invalid_arguments_are_refused_with_votes_and_mask_untouched():
    verts, faces, off, frame = _ragged()
    views = _views(6)
    many = np.concatenate([_views(32), _views(6)[:1]], 0)
    assert _run(verts, faces, off, frame, many, 64, untouched=True)[0] == INVALID                                # NV = 33
    for bad in (dict(NV=0), dict(NV=-1), dict(NV=33), dict(R=15), dict(R=193), dict(R=0), dict(S=0), dict(V=0), dict(F=0),
                dict(verts=None), dict(faces=None), dict(face_off=None), dict(frame=None), dict(views=None), dict(votes=None)):
        assert _run(verts, faces, off, frame, views, bad.pop("R", 64), untouched=True, over=bad)[0] == INVALID, bad
    F = faces.shape[0]
    odd = torch.zeros(3 * F + 8, dtype=torch.int32, device=_dev()).view(torch.uint8)                            # a pointer that is not 4-byte aligned
    for name, n in (("votes", 8 * F), ("mask", 4 * F)):
        assert _run(verts, faces, off, frame, views, 64, untouched=True, over={name: odd[1:1 + n]})[0] == INVALID, name
    assert not odd.any()
    for rho in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        for c in (0, len(off) - 2):
            f = frame.copy()
            f[c, 3] = rho
            assert _run(verts, faces, off, f, views, 64, untouched=True)[0] == INVALID, (rho, c)
    assert _run(verts, faces, off, frame, views, 64)[0] == 0                                                     # and the call they all spoil runs


# ---------------------------------------------------------------------------- 4. the point of it all
INSIDE = {"box": [(0.0, 0.0, 0.0), (0.5, -0.3, 0.6), (-0.7, 0.7, -0.7)], "sphere": [(0.0, 0.0, 0.0), (0.4, 0.3, -0.2), (0.0, -0.6, 0.0)]}
OUTSIDE = {"box": [(1.5, 0.0, 0.0), (0.0, -1.3, 0.4), (1.3, 1.3, 1.3)], "sphere": [(1.3, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 0.0, -1.5)]}


@functools.lru_cache(maxsize=None)
def _stored():
    """box(-1, 1, 2), sphere(4) and the nested cubes as stored, with the orientation and the masks of one device pass."""
    from pdgn_amd.meshes import MeshSet, face_orientation
    meshes = [vc.box(-1.0, 1.0, 2), vc.sphere(4), vc.nested_cubes()]
    verts, faces, off = vc.pack_set(meshes)
    result = face_orientation(verts, faces, off, device=_dev(), return_mask=True)
    return meshes, result, MeshSet.from_meshes(meshes, visible=result["mask"], flip=result["flip"]).to(_dev())


def test_face_orientation_agrees_with_the_mirror_and_with_face_visibility():
    from pdgn_amd.meshes import default_views, face_orientation, face_visibility, orientation_from_votes, shape_frames
    meshes, result, _ = _stored()
    verts, faces, off = vc.pack_set(meshes)
    got = face_orientation(verts, faces, off, views=6, resolution=32, device=_dev(), return_mask=True)
    front, back, mask = fm.votes(verts, faces, off, shape_frames(verts, faces, off), default_views(6), 32)
    want = orientation_from_votes(front, back, off)
    assert sorted(got) == sorted(list(want) + ["mask"]) and all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in want)
    assert np.array_equal(got["mask"], mask) and np.array_equal(got["mask"], face_visibility(verts, faces, off, views=6, resolution=32, device=_dev()))
    assert "mask" not in face_orientation(verts, faces, off, views=6, resolution=32, device=_dev())
    # the default ring: every face of the box and of the sphere is decided, the hidden cube is not, nothing is a sheet
    assert result["undecided_count"].tolist() == [0, 0, 12] and result["two_sided_count"].tolist() == [0, 0, 0]
    assert result["flipped"].tolist() == [24, 96, 6] and np.array_equal(result["mask"], face_visibility(verts, faces, off, device=_dev()))


def test_oriented_meshes_have_a_sign():
    from pdgn_amd.meshes import MeshSet, winding_number, winding_report
    meshes, result, ms = _stored()
    before = winding_report(MeshSet.from_meshes(meshes[:2]).to(_dev()), samples=2048)
    assert np.all(before["fractional"] > 0.5), before
    turned = ms.oriented()
    after = winding_report(turned, samples=2048)
    assert np.all(after["fractional"][:2] <= 0.01), after
    verts, faces = turned.verts.cpu().numpy(), turned.faces.cpu().numpy()
    off = turned.face_off.cpu().numpy()
    for c, name in enumerate(("box", "sphere")):
        pts = np.asarray(INSIDE[name] + OUTSIDE[name], dtype=np.float32)
        want = np.asarray([1.0] * 3 + [0.0] * 3)
        tri = verts[faces[off[c]:off[c + 1]]]
        exact = wm.winding_f64(pts, tri)
        assert np.abs(exact - want).max() < 1e-9, (name, exact)                       # the oriented mesh, on the CPU: outward, closed
        if name == "box":                                                             # (at least 0.2 from the surface)
            assert np.all(np.abs(np.abs(pts).max(axis=1) - 1.0) >= 0.2)
        else:
            assert np.all(np.abs(np.linalg.norm(pts, axis=1) - 1.0) >= 0.2 + 0.07)    # (the facets of sphere(4) dip 0.07 below the sphere)
        w = winding_number(torch.from_numpy(pts[None]).to(_dev()), turned, shape=[c]).cpu().numpy()[0]
        assert np.abs(w - want).max() <= 0.05, (name, w)
        stored = winding_number(torch.from_numpy(pts[None]).to(_dev()), ms, shape=[c]).cpu().numpy()[0]
        assert np.abs(stored - want).max() > 0.05, (name, stored)                     # as stored the same points give fractions
    # the nested cubes: the hidden cube keeps its stored order (it is counted); the visible surface alone is the outer cube, oriented
    pts = torch.tensor([[(0.0, 0.0, 0.0), (0.75, 0.0, 0.1), (-0.3, 0.8, -0.7), (1.4, 0.0, 0.0)]], device=_dev())
    w = winding_number(pts, turned, shape=[2], visible_only=True).cpu().numpy()[0]
    assert np.abs(w - np.asarray([1.0, 1.0, 1.0, 0.0])).max() <= 0.05, w
    assert not result["flip"][off[2] + 12:].any() and result["undecided"][off[2] + 12:].all()


def test_sampling_an_oriented_set_draws_the_same_faces():
    _, result, ms = _stored()
    pts, rec = ms.sample(2048, 7, return_faces=True)
    pts2, rec2 = ms.oriented().sample(2048, 7, return_faces=True)
    assert torch.equal(rec, rec2)
    same = (pts == pts2).all(dim=2).cpu().numpy()
    flipped = result["flip"][rec.cpu().numpy()]
    assert same[~flipped].all() and not same[flipped].all()      # the barycentric pair of a flipped face is mirrored: other points of it


# ---------------------------------------------------------------------------- 5. packing and the command line
def _write_obj(path, verts, faces):
    with open(path, "w") as f:
        for v in verts:
            f.write("v %r %r %r\n" % tuple(float(x) for x in v))
        for t in faces:
            f.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


def test_pack_visible_orient_round_trip_and_check_orient(tmp_path, capsys):
    from pdgn_amd import meshes
    for j, mesh in enumerate((vc.box(-1.0, 1.0, 2), vc.sphere(4))):
        (tmp_path / "obj" / "03001627" / "val").mkdir(parents=True, exist_ok=True)
        _write_obj(tmp_path / "obj" / "03001627" / "val" / ("m%d.obj" % j), *mesh)
    both, plain = str(tmp_path / "both.npz"), str(tmp_path / "plain.npz")
    meshes.main(["pack", str(tmp_path / "obj"), both, "--visible", "--orient"])
    assert "03001627/val: 120 of 240 faces flipped, 0 undecided, 0 two-sided" in capsys.readouterr().out
    meshes.pack(str(tmp_path / "obj"), plain)
    with np.load(both) as f, np.load(plain) as g:
        assert sorted(set(f.files) - set(g.files)) == ["03001627/val/flip", "03001627/val/visible"]
        assert all(np.array_equal(f[k], g[k]) for k in g.files)
    stored = meshes.split_meshset(both, "val", visible="stored", orient="stored")
    opts = {"device": _dev()}
    computed = meshes.split_meshset(meshes.open_mesh_root(plain), "val", visible=opts, orient=dict(opts))
    assert torch.equal(stored.flip, computed.flip) and torch.equal(stored.visible, computed.visible) and stored.flip.sum() == 120
    verts, faces, off = (x.numpy() for x in (stored.verts, stored.faces, stored.face_off))
    assert np.array_equal(stored.visible.numpy().view(np.uint32), meshes.face_visibility(verts, faces, off, device=_dev()))
    meshes.main(["check", plain, "--samples", "1024"])
    assert "closed and consistently oriented" not in capsys.readouterr().out
    meshes.main(["check", both, "--samples", "1024", "--orient"])
    said = capsys.readouterr().out.splitlines()
    assert said[-2].startswith("as stored:") and "signs are not to be trusted" in said[-2], said
    assert said[-1].startswith("oriented:") and said[-1].endswith("closed and consistently oriented"), said
    with pytest.raises(SystemExit, match="pack --orient"):
        meshes.main(["check", plain, "--orient"])
