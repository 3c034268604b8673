"""Generalized winding numbers on the host: the numpy mirror of csrc/winding.hip (tests/winding_mirror.py) -- its
arctangent against float64 arctan2, its winding numbers against a float64 oracle of the same formula, the order independence that the
integer sums buy, the definition's fixed cases and exact occupancy counts -- and what the host interface refuses before it calls the
library.  The figures these tests print are the ones section 7u records."""
import ctypes
import re

import numpy as np
import pytest
import torch

import winding_mirror as wm

F = np.float32
UNIT = 2.0 ** -22
# Measured by the sweeps below: the largest error of natan2 in units of 2^-22 (numpy's float32 arctan2 on the same pairs: 1.32), and the
# largest |w - w_fp64| of the mirror per case -- mesh, placement and kind of point (KINDS).  The tests' bounds are 4 and 16 times these,
# margins for the inputs the sweeps did not draw (the second is the margin of tests/test_p2m_host.py for the same kind of figure).
NATAN2_MEASURED = 1.13
KINDS = ("box", "far", "on faces", "a width off")
W_MEASURED = {
    0.0: {
        'icosphere 2': (1.45e-07, 8.78e-09, 9.06e-07, 8.94e-07),
        'icosphere 3': (1.19e-07, 2.01e-08, 9.54e-07, 6.23e-07),
        'icosphere 4': (7.60e-08, 2.41e-08, 7.15e-07, 7.15e-07),
        'torus 72 x 72': (6.23e-08, 6.26e-08, 1.07e-06, 1.34e-06),
        'random triangles': (4.06e-07, 1.43e-08, 2.80e-06, 2.84e-06),
        'slivers 1e-2': (8.52e-07, 2.12e-08, 1.93e-04, 8.28e-06),
        'slivers 1e-4': (4.34e-08, 1.25e-08, 2.50e-01, 1.63e-01),
    },
    100.0: {
        'icosphere 2': (1.19e-07, 8.30e-09, 1.83e-06, 1.04e-06),
        'icosphere 3': (1.19e-07, 1.51e-08, 5.96e-07, 4.77e-07),
        'icosphere 4': (5.96e-08, 3.52e-08, 3.58e-07, 3.58e-07),
        'torus 72 x 72': (2.38e-07, 5.74e-08, 3.00e-07, 1.31e-06),
        'random triangles': (2.47e-07, 2.28e-08, 6.51e-07, 5.46e-06),
        'slivers 1e-2': (1.11e-05, 1.75e-08, 2.07e-04, 8.50e-06),
        'slivers 1e-4': (2.50e-07, 2.33e-08, 2.49e-01, 1.96e-01),
    },
}


def _ulps_around(x, k=3):
    out = [F(x)]
    for _ in range(k):
        out.insert(0, np.nextafter(out[0], F(-np.inf)))
        out.append(np.nextafter(out[-1], F(np.inf)))
    return np.asarray(out, dtype=F)


def _natan2_error(y, x):
    y, x = np.asarray(y, dtype=F), np.asarray(x, dtype=F)
    want = np.where(y == 0, 0.0, np.arctan2(y.astype(np.float64), x.astype(np.float64)))
    return float(np.abs(wm.natan2(y, x).astype(np.float64) - want).max() / UNIT)


def test_natan2_against_float64():
    rng = np.random.default_rng(0)
    worst = {}
    worst["random"] = _natan2_error(rng.standard_normal(1 << 20), rng.standard_normal(1 << 20))
    axes = np.asarray([(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1), (0, 0), (-0.0, -1.0), (0.0, -0.0)], dtype=F)
    worst["axes and diagonals"] = _natan2_error(axes[:, 0], axes[:, 1])
    # ratios within 3 ulps of the break points of the reduction, both ways round, every quadrant, magnitudes 2^-60 .. 2^60
    ratios = np.concatenate([_ulps_around(b) for b in wm.BREAKS])
    ys, xs = [], []
    for m in (2.0 ** np.arange(-60, 61, 4)).astype(F):
        for sy in (1, -1):
            for sx in (1, -1):
                ys += [sy * ratios * m, sy * np.full_like(ratios, m)]
                xs += [sx * np.full_like(ratios, m), sx * ratios * m]
    worst["break points"] = _natan2_error(np.concatenate(ys), np.concatenate(xs))
    e = rng.integers(-60, 61, (2, 1 << 18))
    worst["magnitudes"] = _natan2_error(rng.standard_normal(1 << 18) * 2.0 ** e[0], rng.standard_normal(1 << 18) * 2.0 ** e[1])
    print("natan2, largest error in units of 2^-22: %s" % {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 4 * NATAN2_MEASURED
    # the fixed cases: y == 0 gives +0 whatever x is, a NaN in gives the canonical NaN out
    for x in (1.0, -1.0, 0.0, -0.0, np.inf, -np.inf, 1e-30, -1e30):
        for y in (0.0, -0.0):
            assert wm.natan2(F(y), F(x)).view(np.uint32) == 0, (y, x)
    for y, x in ((np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (0.0, np.nan), (np.nan, 0.0)):
        assert wm.natan2(F(y), F(x)).view(np.uint32) == wm.NAN_BITS, (y, x)
    assert wm.natan2(F(1), F(0)) == wm.PI_2 and wm.natan2(F(-1), F(0)) == -wm.PI_2 and wm.natan2(F(1), F(1)) == wm.PI_4
    assert wm.natan2(F(1e-30), F(-1)) == wm.PI and wm.natan2(F(-1e-30), F(-1)) == -wm.PI
    assert np.abs(wm.natan2(F(3), rng.standard_normal(1000).astype(F))).max() <= wm.PI


# ---------------------------------------------------------------------------- the mirror's w against the oracle
def _convex_inside(p, v, f, shift):
    t = v.astype(np.float64)[f]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return (((p[:, None, :].astype(np.float64) - t[None, :, 0]) * n[None]).sum(-1) < 0).all(axis=1)


def _torus_inside(p, v, f, shift, R=1.0, r=0.4):
    p = p.astype(np.float64) - shift
    return (np.hypot(p[:, 0], p[:, 1]) - R) ** 2 + p[:, 2] ** 2 < r * r


def _meshes():
    rng = np.random.default_rng(3)
    return [("icosphere 2", wm.icosphere(2), _convex_inside, 1e-3), ("icosphere 3", wm.icosphere(3), _convex_inside, 1e-3),
            ("icosphere 4", wm.icosphere(4), _convex_inside, 1e-3), ("torus 72 x 72", wm.torus_grid(72, 72), _torus_inside, 1e-3),
            ("random triangles", wm.random_triangles(300, rng, scale=0.4), None, 1e-3), ("slivers 1e-2", wm.slivers(300, rng, 1e-2), None, 1e-2),
            ("slivers 1e-4", wm.slivers(300, rng, 1e-4), None, 1e-4)]


def _normals(v, f):
    t = v.astype(np.float64)[f]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


P = 96


@pytest.mark.parametrize("offset", [0.0, 100.0])
def test_the_mirror_against_the_oracle(offset):
    """Per mesh and kind of point, the largest |w - w_fp64|; the oracle sees the same fp32 vertices and points.  A point ON a face is
    on the jump of the winding number: there num is a rounding error, its sign is the side the rounded point fell to, and fp32 and
    float64 may each pick either, and fp32 may also find exactly 0 and take the mean -- so for those points alone the difference is taken
    modulo the steps of 1/2 that one face can make.  A point one width off a sliver of width 1e-4 is where fp32 runs out: num, the volume of
    the tetrahedron, is 1e-8 of the product of its edges, which is the rounding error of the triple product (Limits).  On the
    closed meshes, at the points farther than 0.01 from the surface, rint(w_fp64) is 1 inside and 0 outside and the integer comparison
    T >= T_HALF says the same, without exception."""
    from p2m_mirror import distance_f64
    rng = np.random.default_rng(int(offset) + 11)
    shift = np.asarray([offset, -offset, offset])
    worst, checked = {}, 0
    for name, (v0, f), inside_of, width in _meshes():
        v = (v0.astype(np.float64) + shift).astype(F)
        tri = v[f]
        lo, hi = v0.min(axis=0) - 0.3, v0.max(axis=0) + 0.3
        on, drawn = wm.points_on_faces(v, f, P, rng)
        off = (on.astype(np.float64) + _normals(v, f)[drawn] * width * rng.choice([-1.0, 1.0], (P, 1))).astype(F)
        far = rng.standard_normal((P, 3))
        far = far / np.linalg.norm(far, axis=1, keepdims=True) * 1e3 + shift
        kinds = {"box": (rng.uniform(lo, hi, (4 * P, 3)) + shift).astype(F), "far": far.astype(F), "on faces": on, "a width off": off}
        for kind, pts in kinds.items():
            T, w, ins = wm.winding(pts[None], v, f, [0, f.shape[0]], check=False)
            w64 = wm.winding_f64(pts, tri)
            assert np.isfinite(w).all()
            d = np.abs(w[0].astype(np.float64) - w64)
            if kind == "on faces":
                d = np.minimum(np.minimum(d, np.abs(d - 0.5)), np.abs(d - 1.0))
            worst[(name, kind)] = float(d.max())
            if inside_of is not None and kind in ("box", "far"):
                clear = distance_f64(pts, tri) > 0.01
                truth = inside_of(pts, v, f, shift)
                assert (np.rint(w64[clear]) == truth[clear]).all(), (name, kind)
                assert (ins[0][clear] == truth[clear]).all(), (name, kind)
                assert ((T[0] >= wm.T_HALF) == (ins[0] != 0)).all()
                checked += int(clear.sum())
    names = [m[0] for m in _meshes()]
    print("offset %g: largest |w - w_fp64| per mesh over %s; %d points of closed meshes classified\n%s" % (
        offset, KINDS, checked, "\n".join("    %r: (%s)," % (n, ", ".join("%.2e" % worst[(n, k)] for k in KINDS)) for n in names)))
    assert checked >= 1000
    for n in names:
        for k, recorded in zip(KINDS, W_MEASURED[offset][n]):
            assert worst[(n, k)] <= 16 * recorded, (n, k, worst[(n, k)], recorded)


def test_order_independence_of_the_mirror():
    rng = np.random.default_rng(5)
    v, f = wm.torus_grid(20, 10)
    pts = rng.uniform(-1.5, 1.5, (200, 3)).astype(F)
    T, bad = wm.sum_terms(pts, v[f])
    assert not bad.any()
    perm = rng.permutation(f.shape[0])
    assert (wm.sum_terms(pts, v[f[perm]])[0] == T).all()
    for parts in (1, 2, 3, 7):
        cuts = [k * f.shape[0] // parts for k in range(parts + 1)]
        order = rng.permutation(parts)
        total = np.zeros_like(T)
        for k in order:
            total = total + wm.sum_terms(pts, v[f[perm[cuts[k]:cuts[k + 1]]]])[0]
        assert (total == T).all(), parts
    assert (wm.sum_terms(pts, v[f], step=7)[0] == T).all()
    # the rounding to w and the comparison are functions of T alone
    assert wm.bits_equal(wm.finish(T, bad)[1], (T.astype(np.float64) * wm.K).astype(F))


def test_fixed_cases():
    v, f = wm.icosphere(1)
    off = [0, f.shape[0]]
    # a point at a vertex: the faces that meet there give exactly 0, the others half a turn together
    T, w, ins = wm.winding(v[None, :5], v, f, off)
    assert np.isfinite(w).all() and (np.abs(w - 0.5) < 0.2).all()
    terms, bad = wm.face_terms(v[:1], v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    assert not bad.any() and (terms[0][(f == 0).any(axis=1)] == 0).all() and (terms[0][~(f == 0).any(axis=1)] != 0).all()
    # a point on an axis-aligned face: num is exactly 0 and so is its term; the unit box's other faces give exactly half a turn's worth
    bv, bf = wm.box_mesh(0.0, 1.0)
    p = np.asarray([[0.25, 0.5, 0.0], [0.0, 0.75, 0.125], [1.0, 0.5, 0.5]], dtype=F)
    terms, bad = wm.face_terms(p, bv[bf[:, 0]], bv[bf[:, 1]], bv[bf[:, 2]])
    on_plane = np.stack([(bv[bf][:, :, k] == p[i, k]).all(axis=1) for i, k in ((0, 2), (1, 0), (2, 0))])
    assert on_plane.sum() == 6 and (terms[on_plane] == 0).all() and not bad.any()
    T, w, ins = wm.winding(p[None], bv, bf, [0, 12])
    assert (np.abs(w - 0.5) < 1e-6).all()
    # a degenerate face gives nothing at every point
    dv = np.asarray([(0, 0, 0), (1, 0, 0), (1, 0, 0), (2, 0, 0), (0, 0, 0)], dtype=F)
    pts = np.random.default_rng(1).standard_normal((1, 50, 3)).astype(F)
    for face in ((0, 1, 2), (3, 4, 4), (0, 0, 0)):                  # b == c: cross(B, C) is exactly 0, and with it num and the term
        T, w, ins = wm.winding(pts, dv, np.asarray([face]), [0, 1])
        assert (T == 0).all() and (w.view(np.uint32) == 0).all() and (ins == 0).all(), face
    for face in ((0, 1, 3), (0, 4, 1), (1, 3, 2)):                  # collinear corners, a == b, a == c: num is a rounding error of a zero volume
        T, w, ins = wm.winding(pts, dv, np.asarray([face]), [0, 1])
        assert (np.abs(w) < 1e-6).all() and (ins == 0).all(), face
    # a shape with no live face; a shape index out of range
    T, w, ins = wm.winding(np.concatenate([pts, pts]), v, f, [0, 0, f.shape[0]], shape=[0, 1], live=np.zeros(f.shape[0]))
    assert (T == 0).all() and (w.view(np.uint32) == 0).all() and (ins == 0).all()
    # points that are not finite: the sentinels, whatever the shape holds
    bad_pts = pts.copy()
    bad_pts[0, 0, 0], bad_pts[0, 1, 1], bad_pts[0, 2, 2] = np.nan, np.inf, -np.inf
    for live in (None, np.zeros(f.shape[0])):
        T, w, ins = wm.winding(bad_pts, v, f, off, live=live)
        assert (T[0, :3] == wm.T_BAD).all() and (w[0, :3].view(np.uint32) == wm.NAN_BITS).all() and (ins[0, :3] == 0).all()
        assert (T[0, 3:] != wm.T_BAD).all() and np.isfinite(w[0, 3:]).all()
    # inside and outside of a closed shape, and a flipped one
    io = np.asarray([[(0, 0, 0), (0.3, 0.2, -0.1), (2, 0, 0), (0, -3, 1)]], dtype=F)
    T, w, ins = wm.winding(io, v, f, off)
    assert ins.tolist() == [[1, 1, 0, 0]] and np.abs(w - [[1, 1, 0, 0]]).max() < 1e-6
    T2, w2, ins2 = wm.winding(io, v, f[:, ::-1], off)
    assert np.abs(w2 + w).max() < 1e-6 and ins2.tolist() == [[0, 0, 0, 0]]        # (c, b, a) is another order of operations: not the same bits
    # a subnormal intermediate is refused by the checked form
    with pytest.raises(AssertionError, match="subnormal"):
        wm.winding(np.asarray([[(1e-30, 1e-30, 1.0)]], dtype=F), np.asarray([(0, 0, 0), (1e-20, 0, 0), (0, 1e-20, 0)], dtype=F),
                   np.asarray([(0, 1, 2)]), [0, 1])


BOXES = ((2 / 16, 10 / 16), (6 / 16, 14 / 16))


def test_exact_occupancy_counts():
    """Two axis-aligned boxes on the R = 16 grid of [0, 1]^3: no cell centre lies on a face; 8^3 cells each, 4^3 in both."""
    centres = wm.cell_centres((0, 0, 0), 1 / 16, 16)
    assert centres.shape == (4096, 3) and centres[1].tolist() == [1 / 32, 1 / 32, 3 / 32]
    occ = []
    for lo, hi in BOXES:
        v, f = wm.box_mesh(lo, hi)
        T, w, ins = wm.winding(centres[None], v, f, [0, 12])
        want = ((centres > lo) & (centres < hi)).all(axis=1)
        assert (ins[0] == want).all() and np.abs(w[0] - want).max() < 1e-6
        occ.append(ins[0] != 0)
    counts = int(occ[0].sum()), int(occ[1].sum()), int((occ[0] & occ[1]).sum()), int((occ[0] | occ[1]).sum())
    assert counts == (512, 512, 64, 960) and counts[2] / counts[3] == 64 / 960


# ---------------------------------------------------------------------------- the header, the host-only entry points, the refusals
def test_the_header_declares_the_entry_points():
    from pdgn_amd import _lib
    i, ll, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    assert _lib.ABI_VERSION >= 47
    assert _lib.SIGNATURES["pdgn_winding_half_turn"] == (ll, ())
    assert _lib.SIGNATURES["pdgn_winding_splits"] == (i, (i, i, i))
    assert _lib.SIGNATURES["pdgn_winding_workspace_bytes"] == (ll, (i, i, i, i))
    assert _lib.SIGNATURES["pdgn_winding_number"] == (i, (i,) * 4 + (vp,) * 4 + (i,) + (vp,) * 4 + (vp,))
    handle = ctypes.CDLL(_lib.SO_PATH)
    handle.pdgn_winding_half_turn.restype = handle.pdgn_winding_workspace_bytes.restype = ll
    assert handle.pdgn_winding_half_turn() == wm.T_HALF == int(np.rint(np.pi * 2.0 ** 32))
    assert abs(wm.K * 2.0 ** 33 * np.pi - 1.0) < 2.0 ** -52 and abs(wm.T_HALF * wm.K - 0.5) < 1e-10
    for b, n, faces in ((1, 256, 100352), (1, 1, 1), (35, 2048, 10368), (1, 257, 300), (3, 300, 600), (600, 256, 5000), (1, 64, 1 << 28)):
        assert handle.pdgn_winding_splits(b, n, faces) == wm.splits_for(b, n, faces), (b, n, faces)
    assert handle.pdgn_winding_splits(1, 256, 100352) == 196 and handle.pdgn_winding_splits(35, 2048, 10368) == 8
    assert handle.pdgn_winding_splits(1, 1 << 20, 100352) == 1 and handle.pdgn_winding_splits(1, 256, 600) == 1
    assert handle.pdgn_winding_workspace_bytes(2, 300, 600, 1) == 0 and handle.pdgn_winding_workspace_bytes(2, 300, 600, 7) == 8 * 7 * 600
    assert handle.pdgn_winding_workspace_bytes(1, 256, 100352, 0) == 8 * 196 * 256
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, (1 << 28) + 1), (1 << 16, 1 << 15, 1)):
        assert handle.pdgn_winding_splits(*bad) == -1 and handle.pdgn_winding_workspace_bytes(*bad, 1) == -1, bad
    assert handle.pdgn_winding_workspace_bytes(1, 1, 1, -1) == -1 and handle.pdgn_winding_workspace_bytes(1, 1, 1, 4097) == -1
    with open(_lib.HEADER) as fh:
        text = fh.read()
    assert re.search(r"csrc/winding\.hip", text) and "No reference\n * counterpart" in text


@pytest.fixture
def no_library(monkeypatch):
    """Any library call is a failure: the refusals below come before it."""
    from pdgn_amd import _lib

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", boom)


def _set():
    from pdgn_amd.meshes import MeshSet
    return MeshSet.from_meshes([wm.icosphere(0), wm.torus_grid(5, 4)])


def test_the_host_interface_refuses_before_any_library_call(no_library):
    from pdgn_amd import meshes
    from pdgn_amd.evaluation import volume_iou
    ms = _set()
    x = torch.zeros(2, 7, 3)
    for fn, name in ((meshes.winding_number, "winding_number"), (meshes.signed_distance, "point_to_mesh")):
        for bad in (x[0], x.double(), torch.zeros(2, 7, 2), x.numpy(), torch.zeros(2, 0, 3)):
            with pytest.raises(ValueError, match=name):
                fn(bad, ms)
        with pytest.raises(ValueError, match="MeshSet"):
            fn(x, "meshes.npz")
        with pytest.raises(ValueError, match="3 clouds and 2 shapes"):
            fn(torch.zeros(3, 7, 3), ms)
        with pytest.raises(ValueError, match="shape index"):
            fn(x, ms, shape=[0, 2])
        with pytest.raises(ValueError, match="visibility masks"):
            fn(x, ms, visible_only=True)
    with pytest.raises(ValueError, match="splits"):
        meshes.winding_number(x, ms, splits=-1)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="resolution"):
            meshes.occupancy_grid(ms, resolution=bad)
        with pytest.raises(ValueError, match="resolution"):
            volume_iou(ms, ms, resolution=bad)
    with pytest.raises(ValueError, match="MeshSet"):
        meshes.occupancy_grid(None)
    with pytest.raises(ValueError, match="shape index"):
        meshes.occupancy_grid(ms, shape=[2])
    with pytest.raises(ValueError, match="MeshSets"):
        volume_iou(ms, "b.npz")
    with pytest.raises(ValueError, match="2 shapes against 1"):
        volume_iou(ms, ms, shape_b=[0])
    with pytest.raises(ValueError, match="MeshSet"):
        meshes.winding_report([])
    with pytest.raises(ValueError, match="samples"):
        meshes.winding_report(ms, samples=0)
    # the grids' arithmetic is host numpy
    origin, voxel = meshes.cubic_grid([[0, 0, 0]], [[1, 2, 4]], 8, 0.25)
    assert origin.dtype == F and origin.tolist() == [[-2.5, -2.0, -1.0]] and voxel.tolist() == [0.75]
    origin, voxel = meshes.bounds_grid(((0, 0, 0), (1, 1, 1)), 2, 16)
    assert origin.tolist() == [[0, 0, 0]] * 2 and voxel.tolist() == [1 / 16] * 2
    for bad in (((0, 0, 0), (0, 0, 0)), ((0, 0), (1, 1)), ((0, 0, 0), (np.inf, 1, 1)), 5):
        with pytest.raises(ValueError, match="occupancy_grid"):
            meshes.bounds_grid(bad, 2, 16)


def test_the_commands_refuse_bad_arguments(tmp_path, no_library):
    from pdgn_amd import meshes
    for argv in (["occupancy", "m.npz"], ["check"], ["occupancy", "m.npz", "o.npz"], ["occupancy", "m.npz", "o.npz", "--resolution", "x"],
                 ["occupancy", "m.npz", "o.npz", "--frobnicate"], ["check", "m.npz", "--samples", "many"], ["check", "m.npz", "--signed"]):
        with pytest.raises(SystemExit, match="usage"):
            meshes.main(argv)
    with pytest.raises(SystemExit, match="integers"):
        meshes.main(["occupancy", "m.npz", "o.npz", "--resolution", "8", "--shape", "a"])
