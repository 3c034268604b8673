"""GPU: pdgn_mesh_visibility (csrc/visible.hip) -- bit-equality with tests/visible_mirror.py on a ragged set at
four (resolution, views) pairs and at the block-size remainders, scenes with a known answer, order-independence and repeatability,
the refusals, and the masks' way through MeshSet, the feeder, packing and the command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import visible_cases as vc
import visible_mirror as vm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, POISON = 64, 0x5A5A5A5A
INVALID = -1


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(verts, faces, off, frame, views, R, stream=None, untouched=False, over=None):
    """pdgn_mesh_visibility itself into a poisoned, guarded buffer -> (rc, mask uint32 numpy).  over: replaces an argument by name (S V F
    NV, or a pointer: None for NULL)."""
    from pdgn_amd import _lib
    dev = _dev()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    a = dict(verts=t(verts, np.float32), faces=t(faces, np.int32), face_off=t(off, np.int32), frame=t(frame, np.float32),
             views=t(np.asarray(views).reshape(-1, 3, 3), np.float32))
    F = int(np.asarray(faces).shape[0])
    whole = torch.full((F + 2 * GUARD,), POISON, dtype=torch.int32, device=dev)
    a.update(S=len(off) - 1, V=int(np.asarray(verts).shape[0]), F=F, NV=int(a["views"].shape[0]), R=R, mask=whole[GUARD:GUARD + F])
    a.update(over or {})
    p = lambda x: _lib.ptr(x)
    s = torch.cuda.current_stream(dev) if stream is None else stream
    torch.cuda.synchronize()                                     # (the poison is in place before a side stream may run)
    with torch.cuda.stream(s):
        rc = _lib.lib().pdgn_mesh_visibility(a["S"], a["V"], a["F"], p(a["verts"]), p(a["faces"]), p(a["face_off"]), p(a["frame"]), p(a["views"]),
                                             a["NV"], a["R"], p(a["mask"]), _lib.stream_of(whole))
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert np.all(got[:GUARD] == POISON) and np.all(got[GUARD + F:] == POISON), "a guard word was written"
    if untouched:
        assert np.all(got == POISON), "a refused call wrote"
    return rc, got[GUARD:GUARD + F].view(np.uint32).copy()


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


# ---------------------------------------------------------------------------- 1. bit-equality with the mirror
@pytest.mark.parametrize("R,NV", [(16, 1), (64, 6), (128, 26), (192, 32)])
def test_masks_are_bit_equal_to_the_mirror(R, NV):
    verts, faces, off, frame = _ragged()
    assert np.diff(off).tolist() == [1, 2, 12, 37, 150, 400, 24, 7]
    views = _views(NV)
    rc, got = _run(verts, faces, off, frame, views, R)
    assert rc == 0
    want = vm.visibility(verts, faces, off, frame, views, R)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:20]
    assert got[2] == 0 and np.all(got < (1 << NV) if NV < 32 else True)              # the face of zero area in 3D keeps 0
    if (R, NV) == (16, 1):                                       # the grid shape, by hand: see visible_cases.grid_shape
        assert got[off[-2]:].tolist() == vc.GRID_MASKS, got[off[-2]:]


def test_the_ragged_set_holds_what_it_should():
    """A face larger than the image (vertices clamped at the border), sub-pixel faces that cover no centre, vertices exactly on pixel
    centres and on the image border -- at R = 16 under the identity view, from the mirror's own snap."""
    verts, faces, off, frame = _ragged()
    R, view = 16, np.eye(3, dtype=np.float32)
    snapped = vm.snap(verts[faces[off[2]:off[3]].reshape(-1)], frame[2], view, R)
    assert np.any(snapped[:, :2] == 0) and np.any(snapped[:, :2] == R << 8)                  # clamped: the face reaches outside the image
    grid = vm.snap(verts[faces[off[-2]:].reshape(-1)], frame[-1], view, R)
    assert np.any(grid[:, 0] % 256 == 128) and np.any(grid[:, :2] == 0) and np.any(grid[:, :2] == R << 8)
    tiny = vm.snap(verts[faces[off[5]]], frame[5], view, R)                                  # face 0 of the 400: a sliver
    assert vm._coverage(tiny, R) is None


@pytest.mark.parametrize("F", [vc.FACE_STRIDE - 1, vc.FACE_STRIDE, vc.FACE_STRIDE + 1])
def test_block_size_remainders_are_bit_equal_to_the_mirror(F):
    from pdgn_amd.meshes import shape_frames
    rng = np.random.default_rng(F)
    verts, faces, off = vc.pack_set([vc.random_ball(F, rng), vc.random_ball(3, rng)])
    frame, views = shape_frames(verts, faces, off), _views(6)[[0, 5]]
    rc, got = _run(verts, faces, off, frame, views, 32)
    assert rc == 0 and np.array_equal(got, vm.visibility(verts, faces, off, frame, views, 32))
    assert np.any(got[vc.FACE_STRIDE - 2:F] != 0)                # (the faces around the stride's end are not all hidden ones)


# ---------------------------------------------------------------------------- 2. known answers, no mirror
def _vis(mesh, views=26, R=128):
    from pdgn_amd.meshes import face_visibility
    verts, faces, off = vc.pack_set([mesh])
    return face_visibility(verts, faces, off, views=views, resolution=R, device=_dev())


def test_a_cube_inside_a_closed_cube_is_hidden():
    mask = _vis(vc.nested_cubes(8))
    assert mask.dtype == np.uint32 and mask.shape == (2 * 768,)
    assert np.all(mask[:768] != 0) and np.all(mask[768:] == 0), (np.flatnonzero(mask[:768] == 0), np.flatnonzero(mask[768:]))


def test_every_face_of_a_convex_body_is_visible():
    mesh = vc.sphere(40)
    assert mesh[1].shape[0] == 19200
    mask = _vis(mesh)
    assert np.all(mask != 0), np.flatnonzero(mask == 0)[:20]


def test_a_rod_thinner_than_a_pixel():
    from pdgn_amd.meshes import face_areas
    rod = vc.rod(64)
    assert rod[1].shape[0] == 4 * 64 * 2 and np.all(face_areas(*rod) > 0)
    assert np.all(_vis(rod) != 0)
    inside = _vis(vc.join(vc.box(-1.0, 1.0, 8), rod))
    assert np.all(inside[:768] != 0) and np.all(inside[768:] == 0), np.flatnonzero(inside[768:])


def test_an_open_box_lets_one_view_in():
    from pdgn_amd.meshes import default_views
    mesh = vc.join(vc.box(-1.0, 1.0, sides=[0, 1, 2, 3, 4]), vc.box(-0.25, 0.25))        # no lid at z = +1
    mask = _vis(mesh, views=6)
    eye = -default_views(6)[:, 2]
    v_in = int(np.argmax(eye @ np.asarray([0.0, 0.0, 1.0])))
    inner = mask[10:]
    assert inner[10:12].tolist() == [1 << v_in] * 2, (inner, v_in)                       # side 5 of the inner cube: towards the opening
    assert inner[8:10].tolist() == [0, 0], inner                                         # side 4: towards the floor
    assert np.all(mask[:10] != 0)


def test_two_coincident_quads_are_both_visible():
    quad = vc.box((-1, -1, 0.0), (1, 1, 0.0), sides=[5])
    mask = _vis(vc.join(quad, quad))
    assert np.all(mask != 0) and np.array_equal(mask[:2], mask[2:])


# ---------------------------------------------------------------------------- 3. order and repeatability
@functools.lru_cache(maxsize=None)
def _order_case():
    rng = np.random.default_rng(33)
    meshes = vc.ragged_set(seed=1, sizes=(1, 37, 600)) + [vc.join(vc.box(-1.0, 1.0, 4), vc.rod(16))]
    verts, faces, off = vc.pack_set(meshes)
    from pdgn_amd.meshes import shape_frames
    frame = shape_frames(verts, faces, off)
    rc, mask = _run(verts, faces, off, frame, _views(6), 64)
    assert rc == 0 and 0 < np.count_nonzero(mask) < mask.shape[0]
    return meshes, verts, faces, off, frame, mask, rng.integers(1 << 30)


def test_two_runs_are_byte_equal_and_a_side_stream_gives_the_same():
    meshes, verts, faces, off, frame, mask, _ = _order_case()
    rc, again = _run(verts, faces, off, frame, _views(6), 64)
    assert rc == 0 and again.tobytes() == mask.tobytes()
    rc, side = _run(verts, faces, off, frame, _views(6), 64, stream=torch.cuda.Stream(_dev()))
    assert rc == 0 and side.tobytes() == mask.tobytes()
    assert not np.any(mask == np.uint32(POISON)) and np.all(mask < 64)                   # fully rewritten from the poisoned buffer


def test_permuted_faces_give_permuted_masks_and_reversed_shapes_the_same_masks():
    from pdgn_amd.meshes import shape_frames
    meshes, verts, faces, off, frame, mask, seed = _order_case()
    rng = np.random.default_rng(seed)
    perms = [rng.permutation(f.shape[0]) for _, f in meshes]
    v2, f2, o2 = vc.pack_set([(v, f[p]) for (v, f), p in zip(meshes, perms)])
    rc, got = _run(v2, f2, o2, frame, _views(6), 64)
    assert rc == 0
    for c, p in enumerate(perms):
        assert np.array_equal(got[off[c]:off[c + 1]], mask[off[c]:off[c + 1]][p]), c
    v3, f3, o3 = vc.pack_set(meshes[::-1])
    rc, got = _run(v3, f3, o3, frame[::-1], _views(6), 64)
    assert rc == 0 and np.array_equal(shape_frames(v3, f3, o3), frame[::-1])
    S = len(meshes)
    for c in range(S):
        assert np.array_equal(got[o3[S - 1 - c]:o3[S - c]], mask[off[c]:off[c + 1]]), c


# ---------------------------------------------------------------------------- 4. refusals
def test_invalid_arguments_are_refused_with_the_mask_untouched():
    verts, faces, off, frame = _ragged()
    views = _views(6)
    many = np.concatenate([_views(32), _views(6)[:1]], 0)
    assert _run(verts, faces, off, frame, many, 64, untouched=True)[0] == INVALID                                # NV = 33
    for bad in (dict(NV=0), dict(NV=-1), dict(NV=33), dict(R=15), dict(R=193), dict(R=0), dict(S=0), dict(V=0), dict(F=0),
                dict(verts=None), dict(faces=None), dict(face_off=None), dict(frame=None), dict(views=None)):
        assert _run(verts, faces, off, frame, views, bad.pop("R", 64), untouched=True, over=bad)[0] == INVALID, bad
    from pdgn_amd import _lib
    dev = _dev()
    d = [torch.from_numpy(a).to(dev) for a in (verts, faces, off, frame, views)]
    assert _lib.lib().pdgn_mesh_visibility(len(off) - 1, verts.shape[0], faces.shape[0], *[_lib.ptr(x) for x in d], 6, 64, None,
                                           _lib.stream_of(d[0])) == INVALID                                       # mask = NULL
    for rho in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        for c in (0, len(off) - 2):
            f = frame.copy()
            f[c, 3] = rho
            assert _run(verts, faces, off, f, views, 64, untouched=True)[0] == INVALID, (rho, c)
    assert _run(verts, faces, off, frame, views, 64)[0] == 0                                                     # and the call they all spoil runs


# ---------------------------------------------------------------------------- 5. end to end
@functools.lru_cache(maxsize=None)
def _masked_set():
    from pdgn_amd.meshes import MeshSet, face_visibility
    meshes = [vc.nested_cubes(), vc.join(vc.box(-1.0, 1.0), vc.rod(8))]
    verts, faces, off = vc.pack_set(meshes)
    mask = face_visibility(verts, faces, off, device=_dev())
    assert np.all(mask[:12] != 0) and np.all(mask[12:24] == 0) and np.all(mask[24:36] != 0) and np.all(mask[36:] == 0)
    return meshes, mask, MeshSet.from_meshes(meshes, "shape_unit", visible=mask).to(_dev())


def test_sampling_a_masked_set_draws_no_hidden_face():
    meshes, mask, ms = _masked_set()
    pts, rec = ms.sample(4096, 11, return_faces=True)
    rec = rec.cpu().numpy()
    assert not np.any(mask[rec] == 0)
    assert set(rec[0].tolist()) == set(range(12)) and set(rec[1].tolist()) == set(range(24, 36))    # every visible face, at least once
    assert ms.visible_stats()["hidden"].tolist() == [12, int(meshes[1][1].shape[0]) - 12]


def test_the_feeder_draws_no_hidden_face_and_without_masks_feeds_the_same_bytes():
    from pdgn_amd.data import MeshFeeder
    from pdgn_amd.meshes import MeshSet
    meshes, mask, ms = _masked_set()
    n, sizes = 128, (16, 32, 64)
    feeder = MeshFeeder(ms, 2, sizes, seed=3, num_point=n)
    reals, z1, z2 = feeder.buffers()
    rec = torch.full((2, n + sum(sizes)), -1, dtype=torch.int32, device=_dev())
    for i in range(3):
        feeder.fill(i + 1, 0, reals, z1, z2)                     # (uploads the epoch's order), then the same launch with the record
        feeder._launch(0, i * feeder.batches_per_epoch, 0, reals, z1, z2, face_rec=rec)
        torch.cuda.synchronize()
        drawn = rec.cpu().numpy()
        assert drawn.min() >= 0 and not np.any(mask[drawn] == 0), i
    # visible=None: the set, and what the feeder makes of it, are those of a set built without the argument
    plain, none = MeshSet.from_meshes(meshes, "shape_unit"), MeshSet.from_meshes(meshes, "shape_unit", visible=None)
    assert none.visible is None and all(torch.equal(getattr(plain, k), getattr(none, k)) for k in MeshSet._FIELDS)
    outs = []
    for s in (plain, none):
        f = MeshFeeder(s.to(_dev()), 2, sizes, seed=3, num_point=n)
        r, a, b = f.buffers()
        f.fill(1, 0, r, a, b)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy().tobytes() for t in r + [a, b]])
    assert outs[0] == outs[1]


def _write_obj(path, verts, faces):
    with open(path, "w") as f:
        for v in verts:
            f.write("v %r %r %r\n" % tuple(float(x) for x in v))
        for t in faces:
            f.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


def _obj_root(tmp_path):
    from pdgn_amd.data import cate_to_synsetid
    sid = cate_to_synsetid["chair"]
    train = [vc.nested_cubes(), vc.join(vc.box(-1.0, 1.0), vc.rod(8)), vc.box(0.0, 1.0), vc.join(vc.box(-2.0, 2.0, 2), vc.box(-1.0, 0.0))]
    for split, meshes in (("train", train), ("val", train[:2]), ("test", train[1:3])):
        (tmp_path / "obj" / sid / split).mkdir(parents=True)
        for j, mesh in enumerate(meshes):
            _write_obj(tmp_path / "obj" / sid / split / ("m%d.obj" % j), *mesh)
    return tmp_path / "obj", sid


def test_packed_masks_equal_computed_ones_and_the_cli_trains_and_tests_on_them(tmp_path, capsys):
    from pdgn_amd import meshes, train
    root, sid = _obj_root(tmp_path)
    meshes.main(["pack", str(root), str(tmp_path / "masked.npz"), "--visible", "--views", "6"])
    meshes.pack(str(root), str(tmp_path / "plain.npz"))
    with np.load(tmp_path / "masked.npz") as f, np.load(tmp_path / "plain.npz") as g:
        assert sorted(set(f.files) - set(g.files)) == ["%s/%s/visible" % (sid, s) for s in ("test", "train", "val")]
        assert all(np.array_equal(f[k], g[k]) for k in g.files) and f["%s/train/visible" % sid].dtype == np.uint32
    stored = meshes.split_meshset(str(tmp_path / "masked.npz"), "train", "shape_unit", visible="stored")
    computed = meshes.split_meshset(meshes.open_mesh_root(str(tmp_path / "plain.npz")), "train", "shape_unit", visible={"views": 6, "device": _dev()})
    assert torch.equal(stored.visible, computed.visible) and torch.equal(stored.alias, computed.alias)
    hidden = stored.visible_stats()["hidden"].tolist()
    assert hidden == [12, int(vc.rod(8)[1].shape[0]), 0, 12]
    # the command line: two iterations on the four meshes, then the test phase, both with masked draws
    common = ["--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root", str(tmp_path / "masked.npz"), "--choice", "chair",
              "--batch_size", "2", "--seed", "1", "--save_dir", str(tmp_path / "res"), "--num_point", "64", "--num_k", "4", "--mesh_visible", "on"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    done = subprocess.run([sys.executable, "-m", "pdgn_amd.train"] + common + ["--phase", "train", "--max_epoch", "1", "--snapshot", "1"],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    line = [l for l in done.stdout.splitlines() if l.startswith("--mesh_visible on, train split (stored masks)")]
    assert len(line) == 1 and "%d of %d faces hidden" % (sum(hidden), stored.F) in line[0], done.stdout[-2000:]
    log = (tmp_path / "ck" / "toy" / "log_info.txt").read_text().splitlines()
    assert sum(l.startswith("Epoch: [ 1]") for l in log) == 2 and not any("faces hidden" in l for l in log)
    capsys.readouterr()
    out = train.main(common[:-1] + ["compute", "--mesh_views", "6", "--phase", "test", "--pretrain_model_G", "1_chair_G.pth",
                                    "--pretrain_model_D", "1_chair_D.pth"])
    said = capsys.readouterr().out
    assert "--mesh_visible compute, test split (6 views at 128)" in said and "faces hidden" in said
    assert np.load(os.path.join(out, "out.npy")).shape == (2, 64, 3)
    assert not any("faces hidden" in l for l in open(os.path.join(out, "log.txt")).read().splitlines())
    # the reference draws are masked ones: draw 0 of the masked test split, through the same normalisation
    args = train.parse_args(common + ["--phase", "test"])
    ref = train.reference_clouds(args, "test", _dev(), meshes.open_mesh_root(str(tmp_path / "masked.npz")))
    ms = meshes.split_meshset(str(tmp_path / "masked.npz"), "test", visible="stored").to(_dev())
    pts, rec = ms.sample(64, 1, draw=0, return_faces=True)
    from pdgn_amd.data import normalize_point_clouds
    assert torch.equal(ref, normalize_point_clouds(pts, args.normalize).contiguous())
    assert not np.any(ms.visible.cpu().numpy()[rec.cpu().numpy()] == 0) and ms.visible_stats()["total_hidden"] > 0
