"""The triangle rasteriser's definition (csrc/render.hip: pdgn_render_sheet_mesh) on the host: its numpy mirror
(tests/mesh_render_mirror.py) against facts that need no kernel, and the forms report.MeshColumn and report.render_sheet accept and
refuse before anything touches a device."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import mesh_render_mirror as mm
import render_mirror as rm

F = np.float32
CELL = rm.LATTICE_CELL
AXIS = rm.LATTICE_VIEWS["axis"]                                   # u = 80 x + 64, v = -80 y + 64, d = -0.4375 z + 0.5: exact on the 2^-8 lattice
TILTED = rm.LATTICE_VIEWS["tilted"]
LIGHT = np.array([0.0, 0.0, -1.0], dtype=F)                       # the axis view's viewing direction


def _lat(*k):
    return [v / 256.0 for v in k]


def _square(z=0.0):
    """Corners at X, Y in {639, 1279} sixteenths of a pixel (u = 0.3125 k + 64): the centres 16 p + 8 inside are p = 40 .. 79."""
    x0, x1 = _lat(-77, 51)
    y0, y1 = _lat(77, -51)
    verts = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], dtype=F)
    return verts, np.array([[0, 1, 2], [0, 2, 3]])


def _one(verts, faces, shade="flat", mask=None, base=0, view=AXIS, cell=CELL):
    return mm.render([mm.mesh_column(verts, faces, [[0, len(faces), base]], mask, shade)], view, LIGHT, cell)


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(4000).astype(F), rng.standard_normal(4000).astype(F)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.standard_normal(4000) * 2.0 ** -rng.integers(1, 30, 4000))).astype(F)
    got = mm.fma32(a, b, c)
    for i in range(4000):                                          # cancelling sums: where a double rounding would show
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], F(-np.inf)), np.nextafter(got[i], F(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i
    # a tie of the fp64 sum that the fused operation does not see: 1 + 2^-24 + 2^-60 rounds up in one step, to even (down) in two
    a1, b1 = F(1 + 2.0 ** -12), F(1 + 2.0 ** -12)                  # product 1 + 2^-11 + 2^-24
    assert mm.fma32(a1, b1, F(2.0 ** -60)) == F(1 + 2.0 ** -11 + 2.0 ** -23)
    assert mm.fma32(a1, b1, F(-2.0 ** -60)) == F(1 + 2.0 ** -11)


def test_a_square_of_two_triangles_covers_exactly_the_centres_inside_it():
    verts, faces = _square()
    for shade, tone in (("flat", 255), ("depth", 255 - ((1 << 23) >> 17))):
        img = _one(verts, faces, shade)
        want = np.zeros((CELL, CELL), np.uint8)
        want[40:80, 40:80] = tone                                  # one depth, one normal facing the light: no hole along the diagonal
        assert np.array_equal(img, want), shade
        assert np.array_equal(_one(verts, faces[::-1, ::-1], shade), want)          # clockwise faces: two-sided
    # each triangle alone covers the diagonal's centres: the edge is inclusive on both sides
    a, b = _one(verts, faces[:1]) != 0, _one(verts, faces[1:]) != 0
    both = a & b
    assert both.sum() == 40 and np.array_equal(np.nonzero(both)[0], np.nonzero(both)[1])


def test_the_nearer_of_two_overlapping_triangles_wins_whichever_comes_first():
    far, faces = _square(z=_lat(-64)[0])
    near = _square(z=_lat(64)[0])[0] + np.array(_lat(16, 16, 0), dtype=F)
    verts = np.concatenate([far, near])
    order = np.concatenate([faces, faces + 4])
    a = _one(verts, order, "depth")
    b = _one(verts, order[::-1], "depth")
    assert np.array_equal(a, b)
    _, _, key, _ = rm.point_keys(np.array([far[0], near[0]]), AXIS)
    tone_far, tone_near = (int(k) & 0xFF for k in key)
    assert tone_near > tone_far
    assert a[60, 60] == tone_near and a[79, 41] == tone_far       # inside both / inside the far square alone
    assert set(np.unique(a)) == {0, tone_far, tone_near}
    assert (a == tone_near).sum() == 40 * 40                       # the whole near square shows


def test_shuffling_the_faces_changes_no_byte():
    verts, faces = mm.icosphere(2, 0.7)
    rng = np.random.default_rng(1)
    for shade in ("flat", "depth"):
        want = _one(verts, faces, shade, view=TILTED)
        assert (want != 0).sum() > 3000
        for _ in range(2):
            assert np.array_equal(_one(verts, faces[rng.permutation(len(faces))], shade, view=TILTED), want)


def test_a_face_writes_nothing_outside_its_own_cell():
    verts, faces = _square()
    straddling = verts + np.array(_lat(160, 0, 0), dtype=F)        # X from 1439 to 2079: the cell ends at 2048
    outside = verts + np.array(_lat(300, 0, 0), dtype=F)           # X from 2139 to 2779: in the neighbouring cell's area altogether
    assert mm.snap(outside, AXIS, CELL)[0].min() >= 16 * CELL
    empty = mm.mesh_column(np.zeros((1, 3), F), np.zeros((0, 3), np.int64), [[0, 0, 0], [0, 0, 0]])
    for v in (straddling, outside):
        col = mm.mesh_column(v, faces, [[0, 2, 0], [0, 0, 0]])
        img = mm.render([col, empty, col], AXIS, LIGHT, CELL)
        assert not img[:, CELL:2 * CELL].any() and not img[CELL:].any()
        assert np.array_equal(img[:CELL, :CELL], img[:CELL, 2 * CELL:])
    img = mm.render([mm.mesh_column(straddling, faces, [[0, 2, 0]])], AXIS, LIGHT, CELL)
    want = np.zeros((CELL, CELL), np.uint8)
    want[40:80, 90:128] = 255                                      # centres 16 p + 8 >= 1439: p >= 90
    assert np.array_equal(img, want)
    assert not mm.render([mm.mesh_column(outside, faces, [[0, 2, 0]])], AXIS, LIGHT, CELL).any()
    # a vertex beyond the guard band is clamped onto it (the face is drawn distorted, never out of bounds)
    X = mm.snap(np.array([[30.0, 0, 0], [-30.0, 0, 0]], F), AXIS, CELL)[0]
    assert list(X) == [32 * CELL, -16 * CELL]


def test_dead_faces_draw_nothing():
    verts, faces = _square()
    assert _one(verts, faces).any()
    assert not _one(verts, [[0, 1, 1], [2, 2, 2]]).any()                            # zero area
    collinear = np.array([_lat(-64, -64, 0), _lat(0, 0, 0), _lat(64, 64, 0)], dtype=F)
    assert not _one(collinear, [[0, 1, 2]]).any() and not _one(collinear, [[0, 1, 2]], "depth").any()
    assert not _one(verts, [[0, 1, 4], [0, -1, 2]]).any()                           # an index outside [0, V)
    assert not _one(verts, faces, base=2).any() and not _one(verts, faces, base=-1).any()        # ... after adding the base
    for bad in (np.nan, np.inf):
        v = verts.copy()
        v[0, 2] = bad
        assert not _one(v, faces).any() and not _one(v, faces, "depth").any()       # both faces use vertex 0
    assert not _one(verts, faces, mask=[0, 0]).any()
    half = _one(verts, faces, mask=[7, 0])
    assert np.array_equal(half, _one(verts, faces[:1])) and 0 < (half != 0).sum() < 1600
    # a range that leaves the face array is clipped to it; a count of 0 or less draws nothing
    col = mm.mesh_column(verts, faces, [[-3, 4, 0], [1, 100, 0], [0, 0, 0], [0, -5, 0]])
    img = mm.render([col], AXIS, LIGHT, CELL)
    assert np.array_equal(img[:CELL], _one(verts, faces[:1])) and np.array_equal(img[CELL:2 * CELL], _one(verts, faces[1:]))
    assert not img[2 * CELL:].any()


def test_a_vertex_and_a_splatted_point_share_their_pixel_and_depth():
    pts = rm.lattice_clouds(1, 512, seed=3)[0][0]
    for view in (AXIS, TILTED):
        iu, iv, key, valid = rm.point_keys(pts, view)
        X, Y, Z, finite = mm.snap(pts, view, CELL)
        assert valid.all() and finite.all()
        assert np.array_equal(Z, (key >> np.uint32(8)).astype(np.int64))            # the same q
        u, v, _ = rm.project(pts, view, np.float64)
        free = (np.abs(u * 16) < 16 * CELL) & (np.abs(v * 16) < 16 * CELL)           # (not on the guard band's clamp)
        assert free.sum() > 300
        assert np.abs(X - u * 16)[free].max() <= 0.5 and np.abs(Y - v * 16)[free].max() <= 0.5
    # the axis view puts lattice points on whole sixteenths: the vertex's pixel is the point's
    iu, iv, _, _ = rm.point_keys(pts, AXIS)
    X, Y, _, _ = mm.snap(pts, AXIS, CELL)
    inside = (iu >= 0) & (iu < CELL) & (iv >= 0) & (iv < CELL)
    assert inside.sum() > 100 and np.array_equal(X[inside] >> 4, iu[inside]) and np.array_equal(Y[inside] >> 4, iv[inside])


def test_the_depth_shade_of_a_fronto_parallel_face_is_the_splats():
    for k in (-256, -100, 0, 37, 256):
        verts, faces = _square(z=k / 256.0)
        img = _one(verts, faces, "depth")
        splat = rm.render([np.array([[_lat(0, 0, k)]], dtype=F)], AXIS, CELL, 0)
        (py,), (px,) = np.nonzero(splat[:CELL, :CELL])
        assert img[py, px] == splat[py, px] != 0 and set(np.unique(img)) == {0, splat[py, px]}


def test_flat_shade_follows_the_lit_splats_constants():
    import normals_mirror as nm
    rng = np.random.default_rng(5)
    p = rng.standard_normal((200, 3, 3)).astype(F)
    light = np.array([0.6, 0.0, -0.8], dtype=F)
    shade, alive = mm.flat_shade(p[:, 0], p[:, 1], p[:, 2], light)
    assert alive.all() and shade.min() >= 48 and shade.max() <= 255
    n = np.cross((p[:, 1] - p[:, 0]).astype(np.float64), (p[:, 2] - p[:, 0]).astype(np.float64))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(shade.astype(np.int64) - nm.lit_shade(n.astype(F), light).astype(np.int64)).max() <= 1
    tiny = np.array([[0, 0, 0], [1e-30, 0, 0], [0, 1e-30, 0]], dtype=F)            # the products underflow: the normal is lost
    assert not mm.flat_shade(tiny[None, 0], tiny[None, 1], tiny[None, 2], light)[1][0]


# ---------------------------------------------------------------------------- report.MeshColumn and render_sheet, without a device
def _host_column(rows=2, **kw):
    from pdgn_amd.report import MeshColumn
    verts, faces = mm.icosphere(0)
    return MeshColumn(torch.from_numpy(verts), torch.from_numpy(faces.astype(np.int32)), [0] * rows, [len(faces)] * rows, [0] * rows, **kw)


def test_render_sheet_checks_the_form_of_mesh_columns_before_the_device():
    from pdgn_amd._lib import PdgnHipError
    from pdgn_amd.report import MeshColumn, render_sheet
    verts, faces = mm.icosphere(0)
    tv, tf = torch.from_numpy(verts), torch.from_numpy(faces.astype(np.int32))
    for bad in (lambda: MeshColumn(tv.double(), tf, [0], [20], [0]), lambda: MeshColumn(tv, tf.long(), [0], [20], [0]),
                lambda: MeshColumn(tv, tf.reshape(-1), [0], [20], [0]), lambda: MeshColumn(tv[:, :2], tf, [0], [20], [0]),
                lambda: MeshColumn(tv, tf, [0], [20], [0], mask=torch.ones(20, dtype=torch.int64)),
                lambda: MeshColumn(tv, tf, [0], [20], [0], mask=torch.ones(19, dtype=torch.int32)),
                lambda: MeshColumn(tv, tf, [0, 0], [20], [0]), lambda: MeshColumn(tv, tf, [0.0], [20], [0]),
                lambda: MeshColumn(tv, tf, [0], [20], [0], shade="phong")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        MeshColumn(verts, tf, [0], [20], [0])
    col, cloud = _host_column(2), torch.zeros(2, 16, 3)
    with pytest.raises(ValueError, match="normals\\[1\\]"):
        render_sheet([cloud, col], normals=[None, torch.zeros(2, 20, 3)])
    with pytest.raises(ValueError, match="normals\\[0\\]"):
        render_sheet([col, cloud], normals=["estimate", None])
    with pytest.raises(ValueError, match="one entry per cloud list"):
        render_sheet([col, cloud], normals=[None])
    with pytest.raises(ValueError, match="same number of rows"):
        render_sheet([cloud, _host_column(3)])
    with pytest.raises(ValueError, match="same number of rows"):
        render_sheet([_host_column(3), col])
    with pytest.raises(ValueError):
        render_sheet([col, cloud.double()])
    with pytest.raises(TypeError):
        render_sheet([col, cloud.numpy()])
    with pytest.raises(ValueError):
        render_sheet([col] * 9)
    for columns in ([col], [cloud, col], [col, cloud]):            # the form is right: what is left is that there is no CPU path
        with pytest.raises(PdgnHipError):
            render_sheet(columns)
        with pytest.raises(PdgnHipError):
            render_sheet(columns, normals="estimate", fit=True)


def test_mesh_column_ranges_from_surface_nets_and_from_a_meshset():
    from pdgn_amd.meshes import MeshSet
    from pdgn_amd.report import MeshColumn
    v0, f0 = mm.icosphere(0)
    v1, f1 = mm.box_mesh()
    v2, f2 = mm.icosphere(1, 0.5)
    # surface nets' form: faces local to their cloud, offsets of B + 1 entries; the middle cloud has no face
    verts = torch.from_numpy(np.concatenate([v0, v1, v2]))
    faces = torch.from_numpy(np.concatenate([f0, f2]).astype(np.int32))
    vert_off = torch.tensor([0, 12, 20, 20 + len(v2)], dtype=torch.int32)
    face_off = torch.tensor([0, 20, 20, 100], dtype=torch.int32)
    col = MeshColumn.from_surface_nets(verts, faces, vert_off, face_off)
    assert col.rows == 3 and col.range.dtype == torch.int32 and col.shade == "flat" and col.mask is None
    assert col.range.tolist() == [[0, 20, 0], [20, 0, 12], [20, 80, 20]]
    assert col.face_begin.tolist() == [0, 20, 20] and col.face_count.tolist() == [20, 0, 80] and col.vert_base.tolist() == [0, 12, 20]
    with pytest.raises(ValueError):
        MeshColumn.from_surface_nets(verts, faces, vert_off, face_off[:-1])
    # a mesh set: global indices, base 0, any shape per row
    ms = MeshSet.from_meshes([(v0, f0), (v1, f1), (v2, f2)])
    col = MeshColumn.from_meshset(ms)
    assert col.range.tolist() == [[0, 20, 0], [20, 12, 0], [32, 80, 0]] and col.verts is not None and col.faces.dtype == torch.int32
    assert MeshColumn.from_meshset(ms, [2, 0, 2, 1]).range.tolist() == [[32, 80, 0], [0, 20, 0], [32, 80, 0], [20, 12, 0]]
    assert MeshColumn.from_meshset(ms, torch.tensor([1]), shade="depth").range.tolist() == [[20, 12, 0]]
    for bad in ([3], [-1], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            MeshColumn.from_meshset(ms, bad)
    with pytest.raises(ValueError, match="visibility masks"):
        MeshColumn.from_meshset(ms, visible_only=True)
    seen = np.ones(ms.F, np.uint32)
    seen[3] = 0
    masked = MeshSet.from_meshes([(v0, f0), (v1, f1), (v2, f2)], visible=seen)
    col = MeshColumn.from_meshset(masked, [0], visible_only=True)
    assert col.mask.dtype == torch.int32 and col.mask.tolist() == seen.tolist()
    assert MeshColumn.from_meshset(masked, [0]).mask is None


def test_fitted_and_in_frames_follow_fit_unit_sphere():
    from pdgn_amd.meshes import MeshSet
    from pdgn_amd.report import MeshColumn, fit_frames, fit_unit_sphere
    v0, f0 = mm.icosphere(1, 0.3)
    v1, f1 = mm.box_mesh(2.0)
    ms = MeshSet.from_meshes([(v0 + F(5.0), f0), (v1 * np.array([1, 2, 3], F), f1)])
    col = MeshColumn.from_meshset(ms, [1, 0, 1])
    centre, scale = col.frames()
    assert torch.allclose(centre, torch.tensor([[0.0, 0, 0], [5.0, 5, 5], [0.0, 0, 0]]), atol=1e-6)
    assert torch.allclose(scale, torch.tensor([2.0 * 14 ** 0.5, 0.3, 2.0 * 14 ** 0.5]), rtol=1e-6)
    fit = col.fitted()
    assert fit.verts is not col.verts and fit.faces is col.faces and torch.equal(fit.range, col.range)
    norms = fit.verts.norm(dim=1)
    assert abs(float(norms[:len(v0)].max()) - 1) < 1e-6 and abs(float(norms[len(v0):].max()) - 1) < 1e-6
    assert torch.equal(col.verts, ms.verts)                        # a copy moved, the set's own vertices stay
    # a row without a face: nothing moves, nothing fails
    none = MeshColumn(ms.verts, ms.faces, [0, 0], [0, 0], [0, 0]).fitted()
    assert torch.equal(none.verts, ms.verts)
    # vertices that ARE the points of a cloud, moved into the cloud's frame, are the fitted cloud's points bit for bit
    g = torch.Generator().manual_seed(3)
    pcs = torch.randn(2, 30, 3, generator=g) * 3 + 1
    tri = torch.arange(30, dtype=torch.int32).reshape(10, 3)
    col = MeshColumn.from_surface_nets(pcs.reshape(-1, 3).contiguous(), torch.cat([tri, tri]), torch.tensor([0, 30, 60]), torch.tensor([0, 10, 20]))
    moved = col.in_frames(*fit_frames(pcs))
    assert torch.equal(moved.verts.reshape(2, 30, 3), fit_unit_sphere(pcs))
