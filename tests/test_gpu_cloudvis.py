"""Normal orientation from visibility on the device: pdgn_cloud_normal_votes and pdgn_orient_pool bit for bit
against their numpy mirror (tests/cloudvis_mirror.py) -- votes, normals, balances and all four counters -- on estimated and on hostile
inputs, over the rounds and the disc sizes; repeatability, the in-place call, the optional outputs, the refusals, the Python wrappers,
the reconstruction beyond the propagation's 4096 points and the export command line."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import cloudvis_mirror as cm
import normals_mirror as nm
import orient_mirror as om
import reconstruct_mirror as rm

pytestmark = pytest.mark.gpu
F = np.float32
# (b, n, k, NV, R): the smallest call; fewer points than a wave; one past a wave, several clouds; one past a workgroup; the flagship cloud;
# beyond the propagation's 4096 points with the largest depth buffer (144 KB of LDS: the launch opts in)
SHAPES = [(1, 1, 1, 6, 8), (2, 3, 3, 6, 16), (3, 65, 8, 14, 32), (2, 257, 16, 26, 64), (1, 2048, 16, 26, 64), (1, 5000, 8, 26, 192)]
SPLAT, BIAS = 384, 4096                                            # 1.5 pixels; 2^-8 of the frame's radius
SENTINEL = 7.0


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _views(nv):
    from pdgn_amd.meshes import default_views
    return default_views(nv)


def _votes(x, g, frame, views, R, splat=SPLAT, bias=BIAS, **over):
    """The raw entry point on device tensors -> (rc, votes (b,n,2) uint32), sentinel-filled before the call."""
    from pdgn_amd import _lib
    b, n, _ = x.shape
    votes = torch.full((b, n, 2), 77, dtype=torch.int32, device=x.device)
    a = dict(b=b, n=n, NV=views.shape[0], R=R, splat=splat, bias=bias)
    a.update(over)
    rc = _lib.lib().pdgn_cloud_normal_votes(a["b"], a["n"], _lib.ptr(x), _lib.ptr(g), _lib.ptr(frame), _lib.ptr(views), a["NV"], a["R"], a["splat"],
                                            a["bias"], _lib.ptr(votes), _lib.stream_of(x))
    torch.cuda.synchronize()
    return rc, votes.cpu().numpy().view(np.uint32)


def _pool(x, idx, g, votes, rounds, pooled=True, stats=True, inplace=False, work=True, **over):
    """The raw entry point -> (rc, normals, pooled or None, stats or None), sentinel-filled before the call."""
    from pdgn_amd import _lib
    b, n, k = idx.shape
    out = g.clone() if inplace else torch.full((b, n, 3), SENTINEL, dtype=torch.float32, device=x.device)
    src = out if inplace else g
    po = torch.full((b, n), 77, dtype=torch.int64, device=x.device) if pooled else None
    st = torch.full((b, 4), 77, dtype=torch.int32, device=x.device) if stats else None
    ws = torch.empty((2, b, n), dtype=torch.int64, device=x.device) if work else None
    a = dict(b=b, n=n, k=k, rounds=rounds)
    a.update(over)
    rc = _lib.lib().pdgn_orient_pool(a["b"], a["n"], a["k"], _lib.ptr(x), _lib.ptr(idx), _lib.ptr(src), _lib.ptr(votes), a["rounds"], _lib.ptr(out),
                                     _lib.ptr(po), _lib.ptr(st), _lib.ptr(ws), _lib.stream_of(x))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), None if po is None else po.cpu().numpy(), None if st is None else st.cpu().numpy()


def _same(got, want):
    return got[0] == 0 and nm.same_bits(got[1], want[0]) and np.array_equal(got[2], want[1]) and np.array_equal(got[3], want[2])


def _both_against_the_mirror(x, g, idx, nv, R, rounds=(1,), splat=SPLAT, bias=BIAS):
    """Votes, then the pooling on them, device against mirror; x, g, idx numpy.  Returns the votes."""
    from pdgn_amd import pointops
    xd, gd, id_ = _t(x), _t(g), _t(idx)
    frame, views = pointops.cloud_frames(xd), _t(_views(nv))
    rc, votes = _votes(xd, gd, frame, views, R, splat, bias)
    want = cm.votes(x, g, frame.cpu().numpy(), views.cpu().numpy(), R, splat, bias)
    assert rc == 0 and np.array_equal(votes, want)
    assert votes.max() <= nv * 256
    vd = _t(votes.view(np.int32))
    for r in rounds:
        assert _same(_pool(xd, id_, gd, vd, r), cm.pool(x, g, idx, votes, r)), r
    return votes


def _clouds(kind, b, n):
    if kind == "gauss":
        return np.random.default_rng(60 + n).standard_normal((b, n, 3)).astype(F)
    return np.stack([cm.slab(n, 0.08, seed)[0] for seed in range(b)])


@pytest.mark.parametrize("kind", ["gauss", "slab"])
@pytest.mark.parametrize("b,n,k,nv,R", SHAPES)
def test_both_kernels_equal_the_mirror_on_estimated_normals_and_knn_lists(b, n, k, nv, R, kind):
    from pdgn_amd import pointops
    x = _clouds(kind, b, n)
    xd = _t(x)
    idx = pointops.knnquery(k, xd, xd)
    g = pointops.estimate_normals(xd, idx=idx)
    votes = _both_against_the_mirror(x, g.cpu().numpy(), idx.cpu().numpy(), nv, R)
    assert votes.sum() > 0
    frame = pointops.cloud_frames(xd).cpu().numpy()
    assert np.allclose(frame, np.stack([cm.cloud_frame(c) for c in x]), rtol=1e-6, atol=0)


@pytest.mark.parametrize("b,n,k,nv,R", SHAPES)
def test_both_kernels_equal_the_mirror_on_random_lists_with_repeats_and_poison(b, n, k, nv, R):
    """Random indices (repeats and self entries are the rule, and every point gets one self entry for certain), one entry of the whole
    call outside its cloud and, where the cloud has more than two points, one NaN normal and one infinite coordinate."""
    rng = np.random.default_rng(70 + n)
    x = rng.standard_normal((b, n, 3)).astype(F)
    g = rng.standard_normal((b, n, 3))
    g = (g / np.linalg.norm(g, axis=2, keepdims=True)).astype(F)
    idx = rng.integers(0, n, size=(b, n, k)).astype(np.int32)
    idx[:, :, 0] = np.arange(n, dtype=np.int32)[None, :]
    idx[b - 1, n // 2, k - 1] = (n, -1, n + 5, 2 ** 31 - 1)[n % 4]
    if n > 2:
        g[0, 1, 2], x[b - 1, n - 1, 0] = np.nan, np.inf
    votes = _both_against_the_mirror(x, g, idx, nv, R, rounds=(1, 2))
    if n > 2:
        assert (votes[0, 1] == 0).all() and (votes[b - 1, n - 1] == 0).all()


def test_the_rounds_and_the_disc_sizes():
    """rounds 0, 1, 2 and 4 (both halves of the workspace, either one last); no disc, a disc below a pixel, a disc beyond the image."""
    from pdgn_amd import pointops
    x = _clouds("slab", 2, 257)
    xd = _t(x)
    idx = pointops.knnquery(16, xd, xd)
    g = pointops.estimate_normals(xd, idx=idx).cpu().numpy()
    idx = idx.cpu().numpy()
    seen = [_both_against_the_mirror(x, g, idx, 14, 16, rounds=(0, 1, 2, 3, 4), splat=s, bias=b) for s, b in ((0, 0), (100, 1 << 12), (256 * 16 * 2, 1 << 14))]
    assert seen[0].sum() > seen[2].sum() > 0                        # (a disc as wide as the image hides all but the nearest layer)


def test_two_calls_agree_in_place_equals_out_of_place_and_outputs_may_be_null():
    from pdgn_amd import pointops
    x, _ = om.torus(1500, 7)
    xd = _t(np.stack([x, x[::-1].copy()]))
    idx = pointops.knnquery(12, xd, xd)
    g = pointops.estimate_normals(xd, idx=idx)
    frame, views = pointops.cloud_frames(xd), _t(_views(26))
    v1, v2 = _votes(xd, g, frame, views, 64), _votes(xd, g, frame, views, 64)
    assert v1[0] == 0 and v2[0] == 0 and v1[1].tobytes() == v2[1].tobytes() and np.array_equal(v1[1][0], v1[1][1][::-1])
    vd = _t(v1[1].view(np.int32))
    for rounds in (1, 2):
        first = _pool(xd, idx, g, vd, rounds)
        again = _pool(xd, idx, g, vd, rounds)
        assert first[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], again[1:]))
        inplace = _pool(xd, idx, g, vd, rounds, inplace=True)
        assert inplace[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], inplace[1:]))
        for kw in (dict(pooled=False), dict(stats=False), dict(pooled=False, stats=False)):
            rc, out, po, st = _pool(xd, idx, g, vd, rounds, **kw)
            assert rc == 0 and out.tobytes() == first[1].tobytes()
            assert (po is None or np.array_equal(po, first[2])) and (st is None or np.array_equal(st, first[3]))


def test_every_refusal_writes_nothing():
    from pdgn_amd import _lib, pointops
    xd = _t(np.random.default_rng(1).standard_normal((2, 40, 3)).astype(F))
    idx = pointops.knnquery(8, xd, xd)
    g = pointops.estimate_normals(xd, idx=idx)
    frame, views = pointops.cloud_frames(xd), _t(_views(6))
    for kw in (dict(b=0), dict(n=0), dict(b=1 << 20, n=257), dict(NV=0), dict(NV=33), dict(R=0), dict(R=193), dict(splat=-1), dict(bias=-1)):
        rc, votes = _votes(xd, g, frame, views, **dict(dict(R=16), **kw))
        assert rc == -1 and (votes == 77).all(), kw
    rc, good_votes = _votes(xd, g, frame, views, 16)
    assert rc == 0
    vd = _t(good_votes.view(np.int32))
    for kw in (dict(b=0), dict(n=0), dict(b=1 << 20, n=257), dict(k=0), dict(k=65), dict(rounds=-1), dict(rounds=5), dict(work=False)):
        over = dict(kw)
        rc, out, po, st = _pool(xd, idx, g, vd, over.pop("rounds", 1), **over)
        assert rc == -1 and (out == SENTINEL).all() and (po == 77).all() and (st == 77).all(), kw
    L, p = _lib.lib(), _lib.ptr
    odd = lambda t, by=2: ctypes.c_void_p(t.data_ptr() + by)
    votes = torch.full((2, 40, 2), 77, dtype=torch.int32, device=_dev())
    tens = (xd, g, frame, views, votes)
    for slot in range(5):
        for bad in (None, odd(tens[slot])):
            args = [p(t) for t in tens]
            args[slot] = bad
            assert L.pdgn_cloud_normal_votes(2, 40, *args[:4], 6, 16, SPLAT, BIAS, args[4], _lib.stream_of(xd)) == -1, (slot, bad)
    out = torch.full((2, 40, 3), SENTINEL, device=_dev())
    po = torch.full((2, 40), 77, dtype=torch.int64, device=_dev())
    st = torch.full((2, 4), 77, dtype=torch.int32, device=_dev())
    ws = torch.empty((2, 2, 40), dtype=torch.int64, device=_dev())
    tens = (xd, idx, g, vd, out, po, st, ws)                        # the argument order, `rounds` between votes and normals_out
    for slot in range(8):
        bads = ([] if slot in (5, 6) else [None]) + [odd(tens[slot])] + ([odd(tens[slot], 4)] if slot in (5, 7) else [])
        for bad in bads:
            args = [p(t) for t in tens]
            args[slot] = bad
            assert L.pdgn_orient_pool(2, 40, 8, *args[:4], 1, *args[4:], _lib.stream_of(xd)) == -1, (slot, bad)
    torch.cuda.synchronize()
    assert (votes == 77).all() and (out == SENTINEL).all() and (po == 77).all() and (st == 77).all()
    for bad in (dict(k=41), dict(k=0), dict(rounds=5), dict(rounds=-1), dict(resolution=0), dict(resolution=193), dict(views=7), dict(radius=-1.0),
                dict(radius_factor=0.0), dict(bias_factor=-1.0), dict(idx=idx[:, :39].contiguous()), dict(idx=idx.long())):
        with pytest.raises((ValueError, TypeError)):
            pointops.orient_normals_visible(xd, g, **bad)
    with pytest.raises(ValueError):
        pointops.normal_votes(xd, g[:, :39].contiguous())
    with pytest.raises(ValueError, match="give a radius"):
        pointops.normal_votes(torch.zeros(1, 8193, 3, device=_dev()), torch.zeros(1, 8193, 3, device=_dev()))


def test_the_wrappers_return_what_the_entry_points_write():
    from pdgn_amd import pointops, reconstruct
    x = _clouds("slab", 3, 300)
    xd = _t(x)
    idx = pointops.knnquery(16, xd, xd)
    g = pointops.estimate_normals(xd, idx=idx)
    front, back, q = pointops.normal_votes(xd, g, views=14, resolution=48, return_quanta=True)
    assert front.dtype == torch.int32 and not front.requires_grad and q["views"].shape == (14, 3, 3)
    assert torch.equal(q["frame"], pointops.cloud_frames(xd))
    # the integers are the batch means of the clouds' own, in fp64, rounded once
    rho = q["frame"][:, 3].double().cpu().numpy()
    radius = 2.0 * np.array([cm.mean_spacing(c) for c in x])
    assert abs(q["splat"] - (radius / rho).mean() * 48 * 128) <= 0.5 + 1e-3 and abs(q["bias"] - (0.25 * radius / rho).mean() * 2 ** 20) <= 0.5 + 2.0
    rc, votes = _votes(xd, g, q["frame"], q["views"], 48, q["splat"], q["bias"])
    assert rc == 0 and np.array_equal(votes[:, :, 0], front.cpu().numpy().view(np.uint32)) and np.array_equal(votes[:, :, 1], back.cpu().numpy().view(np.uint32))
    assert np.array_equal(votes, cm.votes(x, g.cpu().numpy(), q["frame"].cpu().numpy(), q["views"].cpu().numpy(), 48, q["splat"], q["bias"]))
    given = 2.0 * reconstruct.mean_spacing(xd)                     # (the same fp64 values the default takes)
    f2, b2 = pointops.normal_votes(xd, g, views=_views(14), resolution=48, radius=given, bias=0.25 * given)
    assert torch.equal(f2, front) and torch.equal(b2, back)
    for rounds in (0, 1, 3):
        o, (f3, b3, pooled), stats = pointops.orient_normals_visible(xd, g, idx=idx, rounds=rounds, views=14, resolution=48, return_votes=True,
                                                                     return_stats=True)
        raw = _pool(xd, idx, g, _t(votes.view(np.int32)), rounds)
        assert torch.equal(f3, front) and torch.equal(b3, back) and not o.requires_grad
        assert _same(raw, (o.cpu().numpy(), pooled.cpu().numpy(), stats.cpu().numpy()))
    plain = pointops.orient_normals_visible(xd, g, 16)
    assert isinstance(plain, torch.Tensor)
    assert nm.same_bits(pointops.estimate_normals(xd, 16, orient="visible").cpu().numpy(), plain.cpu().numpy())
    n2, e2 = pointops.estimate_normals(xd, idx=idx, orient="visible", return_eig=True)
    assert nm.same_bits(n2.cpu().numpy(), plain.cpu().numpy()) and nm.same_bits(e2.cpu().numpy(), pointops.estimate_normals(xd, idx=idx, return_eig=True)[1].cpu().numpy())


def test_estimate_normals_visible_orients_the_slab_that_consistent_gets_wrong():
    from pdgn_amd import pointops
    x, analytic = cm.slab(2048, 0.08, 0)
    xd = _t(x[None])
    g = pointops.estimate_normals(xd, 16).cpu().numpy()[0]
    o, (_, _, pooled), stats = pointops.orient_normals_visible(xd, _t(g[None]), 16, return_votes=True, return_stats=True)
    assert nm.same_bits(pointops.estimate_normals(xd, 16, orient="visible").cpu().numpy(), o.cpu().numpy())
    sure, wrong, undecided = cm.wrong_and_undecided(o.cpu().numpy()[0], pooled.cpu().numpy()[0], analytic, g)
    print("visible: %d sure, %d wrong, %d undecided, stats %s" % (sure, wrong, undecided, stats.tolist()))
    assert sure > 1000 and wrong <= 0.01 * sure and undecided <= 0.01 * sure
    tree = pointops.estimate_normals(xd, 16, orient="consistent").cpu().numpy()[0]
    sure, wrong, _ = cm.wrong_and_undecided(tree, None, analytic, g)
    print("consistent: %d sure, %d wrong" % (sure, wrong))
    assert wrong >= 0.40 * sure


def test_reconstruct_visible_closes_a_torus_beyond_the_propagations_limit():
    from pdgn_amd import reconstruct
    x, _ = om.torus(5000, 0)
    xd = _t(x[None])
    # h = 0.14 is five mean spacings of this cloud, so the discs take two of them, as the default does for smaller clouds
    verts, faces, vert_off, face_off, stats = reconstruct.reconstruct(xd, resolution=64, radius=0.14, orient="visible")
    rep = reconstruct.mesh_report(verts, faces)
    print(rep, stats.tolist())
    assert rep["faces"] > 500 and rep["boundary_edges"] == 0 and rep["nonmanifold_edges"] == 0 and rep["euler"] == 0 and rep["components"] == 1
    assert rep["oriented"] and rep["volume"] > 0
    with pytest.raises(ValueError):
        reconstruct.reconstruct(xd, resolution=64, radius=0.14, orient="consistent")
    with pytest.raises(ValueError):
        reconstruct.reconstruct(xd, resolution=64, radius=0.14, orient="outward")


def _read_mesh_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    verts = np.frombuffer(body, dtype="<f4", count=3 * nv).reshape(nv, 3)
    rec = np.frombuffer(body, dtype=[("count", "u1"), ("index", "<i4", (3,))], count=nf, offset=12 * nv)
    return verts, rec["index"]


def test_the_export_command_meshes_saved_tori_with_visible_normals(tmp_path, capsys):
    from pdgn_amd import export
    from pdgn_amd.reconstruct import mesh_report
    clouds, truths = zip(*(om.torus(2048, seed) for seed in rm.EXPORT_SEEDS))
    np.save(tmp_path / "tori.npy", np.stack(clouds))
    out = export.main([str(tmp_path / "tori.npy"), "-o", str(tmp_path / "plys"), "--orient", "visible", "--mesh", "40"])
    said = capsys.readouterr().out
    assert "normals from 16 neighbours" in said and " points undecided, " in said and " 0 open edges, 0 non-manifold edges" in said
    for i in range(len(rm.EXPORT_SEEDS)):
        verts, faces = _read_mesh_ply("%s/mesh_%d.ply" % (out, i))
        rep = mesh_report(verts, faces)
        print(rm.EXPORT_SEEDS[i], rep)
        assert rep["boundary_edges"] == 0 and rep["nonmanifold_edges"] == 0 and rep["euler"] == 0 and rep["components"] == 1
        assert rep["oriented"] and abs(rep["volume"] / (2 * np.pi ** 2 * 0.16) - 1) < 0.10
        raw = open("%s/cloud_%d.ply" % (out, i), "rb").read()
        rows = np.array(struct.unpack("<%df" % (6 * 2048), raw.split(b"end_header\n", 1)[1]), dtype=F).reshape(2048, 6)
        assert nm.same_bits(rows[:, :3], clouds[i]) and ((rows[:, 3:].astype(np.float64) * truths[i]).sum(axis=1) > 0).all()
