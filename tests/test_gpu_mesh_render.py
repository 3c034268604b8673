"""The triangle rasteriser on the device (csrc/render.hip: pdgn_render_sheet_mesh; pdgn_amd/report.py: MeshColumn, render_sheet;
DESIGN.md section 7v): byte for byte against its numpy mirror (tests/mesh_render_mirror.py) in every regime of the kernel, the mixed
sheets against the cloud-only and mesh-only ones, the reporter's mesh column and the two command lines."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_render_mirror as mm
import render_mirror as rm

pytestmark = pytest.mark.gpu
F = np.float32
AXIS = rm.LATTICE_VIEWS["axis"]
LIGHT = (0.3, -0.5, -0.8)


def _dev():
    return torch.device("cuda:0")


def _light():
    from pdgn_amd.report import _light
    return _light(LIGHT, False)


def _column(verts, faces, ranges, mask=None, shade="flat"):
    """The same column for the device and for the mirror."""
    from pdgn_amd.report import MeshColumn
    dev = _dev()
    ranges = np.asarray(ranges, dtype=np.int64).reshape(-1, 3)
    col = MeshColumn(torch.from_numpy(np.ascontiguousarray(verts, dtype=F)).to(dev),
                     torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)).to(dev), ranges[:, 0], ranges[:, 1], ranges[:, 2],
                     None if mask is None else torch.from_numpy(np.asarray(mask, dtype=np.int32)).to(dev), shade)
    return col, mm.mesh_column(verts, np.asarray(faces).reshape(-1, 3), ranges, mask, shade)


def _stack(meshes):
    """[(verts, faces)] -> verts, global faces, ranges with base 0."""
    verts, faces, ranges, at, fat = [], [], [], 0, 0
    for v, f in meshes:
        verts.append(v)
        faces.append(np.asarray(f, dtype=np.int64).reshape(-1, 3) + at)
        ranges.append([fat, len(f), 0])
        at, fat = at + len(v), fat + len(f)
    return np.concatenate(verts), np.concatenate(faces), ranges


def _check(pairs, view, cell, what):
    from pdgn_amd.report import render_sheet
    got = render_sheet([p[0] for p in pairs], view=view, cell=cell, light=LIGHT)
    want = mm.render([p[1] for p in pairs], view, _light(), cell)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    again = render_sheet([p[0] for p in pairs], view=view, cell=cell, light=LIGHT)
    got = got.cpu().numpy()
    print("%s: %d pixels differ of %d, %d lit" % (what, int((got != want).sum()), want.size, int((want != 0).sum())))
    assert np.array_equal(got, want), what
    assert np.array_equal(again.cpu().numpy(), want), what + " (second run)"
    return want


@pytest.mark.parametrize("shade", ["flat", "depth"])
@pytest.mark.parametrize("cell,rows", [(16, 1), (33, 2), (128, 3)])
def test_icospheres_and_a_triangle_larger_than_the_cell_equal_the_mirror(cell, rows, shade):
    """Column 0: one icosphere of 320 faces per row, of growing size and off the centre (the lane path at cell 16 and 33, both paths at
    128).  Column 1: a single triangle larger than the cell in every row -- clipping and the wave path.  The default view: arbitrary fp32."""
    from pdgn_amd.report import default_view
    view = default_view(cell)
    spheres = []
    for r in range(rows):
        v, f = mm.icosphere(2, 0.45 + 0.25 * r)
        spheres.append((v + np.array([0.1 * r, -0.07 * r, 0.05], F), f))
    big = [(np.array([[-4.0, -3.0, 0.3 * r], [5.0, -2.5, -0.4], [0.5 * r, 6.0, 0.2]], F), [[0, 1, 2]]) for r in range(rows)]
    pairs = [_column(*_stack(spheres), shade=shade), _column(*_stack(big), shade=shade)]
    want = _check(pairs, view, cell, "cell %d rows %d %s" % (cell, rows, shade))
    assert all((want[r * cell:(r + 1) * cell, :cell] != 0).any() for r in range(rows))
    assert (want[:, cell:] != 0).sum() > rows * cell * cell // 4


@pytest.mark.parametrize("shade", ["flat", "depth"])
def test_thresholds_empty_rows_dead_faces_masks_and_the_guard_band_equal_the_mirror(shade):
    cell = 128
    lat = lambda *k: [v / 256.0 for v in k]                                           # noqa: E731  (X = 5 kx + 1024, Y = -5 ky + 1024)
    # row 0: two faces whose clipped boxes hold exactly MESH_SMALL_BOX pixels (a lane's) and one more (a wave's)
    edge_v = np.array([lat(-77, 141, 10), lat(-51, 141, -20), lat(-77, 128, 40), lat(-77, 109, 0), lat(-43, 109, 90), lat(-77, 100, -90)], F)
    edge_f = np.array([[0, 1, 2], [3, 4, 5]])
    assert mm.box_pixels(edge_v, edge_f, 0, AXIS, cell) == [mm.SMALL_BOX, mm.SMALL_BOX + 1]
    # row 2: dead faces of every kind among live ones
    sq = np.array([lat(-77, 77, 0), lat(51, 77, 30), lat(51, -51, 60), lat(-77, -51, -30), [np.nan, 0, 0], lat(0, 0, 0), lat(64, 64, 64),
                   [0, np.inf, 0]], F)
    # (two of zero area, a NaN vertex, an infinite vertex; indices outside the array: test_dead_indices_at_the_ends_of_the_vertex_array)
    dead_f = np.array([[0, 1, 2], [0, 1, 1], [0, 2, 3], [0, 1, 4], [3, 5, 6], [5, 5, 5], [1, 2, 7], [0, 5, 6]])
    live = np.array([0, 2, 4, 7])
    # row 3: a mask over an icosphere; rows 4, 5: icospheres that reach into the guard band and beyond it (clamped: drawn distorted)
    ico_v, ico_f = mm.icosphere(2, 0.6)
    mask_ico = (np.arange(len(ico_f)) % 3 != 0).astype(np.int32) * 5
    meshes = [(edge_v, edge_f), (np.zeros((1, 3), F), np.zeros((0, 3), np.int64)), (sq, dead_f), (ico_v, ico_f),
              (ico_v * F(3.5) + np.array([0.4, 0, 0], F), ico_f), (ico_v * F(9.0), ico_f)]
    verts, faces, ranges = _stack(meshes)
    mask = np.ones(len(faces), np.int32)
    mask[ranges[3][0]:ranges[3][0] + len(ico_f)] = mask_ico
    pair = _column(verts, faces, ranges, mask, shade)
    want = _check([pair], AXIS, cell, "special rows %s" % shade)
    lit = [(want[r * cell:(r + 1) * cell] != 0).sum() for r in range(6)]
    assert lit[0] > 20 and lit[1] == 0 and lit[2] > 1000 and lit[3] > 1000 and lit[4] > 4000 and lit[5] > 4000
    # the dead faces alone (and the live ones masked away) draw nothing at all
    only_dead = np.ones(len(faces), np.int32)
    only_dead[ranges[2][0] + live] = 0
    dead_pair = _column(verts, faces, [ranges[2]], only_dead, shade)
    assert not _check([dead_pair], AXIS, cell, "dead faces %s" % shade).any()


def test_dead_indices_at_the_ends_of_the_vertex_array():
    """Indices below 0 and at V after adding the base: dead; the neighbours V - 1 and 0: alive."""
    cell = 128
    lat = lambda *k: [v / 256.0 for v in k]                                           # noqa: E731
    verts = np.array([lat(-77, 77, 0), lat(51, 77, 30), lat(51, -51, 60), lat(-77, -51, -30)], F)
    faces = np.array([[0, 1, 2], [0, 2, 3], [1, 2, 4], [-1, 0, 1]])
    pair = _column(verts, faces, [[0, 4, 0], [2, 2, 0], [0, 4, 1], [0, 4, -1], [0, 100, 0], [-7, 8, 0]])
    want = _check([pair], AXIS, cell, "index ends")
    lit = [(want[r * cell:(r + 1) * cell] != 0).sum() for r in range(6)]
    # rows: all four faces (two alive); the two dead ones; base 1 and base -1 (other faces die); ranges that leave the face array, clipped
    assert lit[0] == 1600 and lit[1] == 0 and 0 < lit[2] < 1600 and 0 < lit[3] < 1600 and lit[4] == 1600 and 0 < lit[5] < 1600


def test_shuffled_faces_draw_the_same_bytes():
    from pdgn_amd.report import default_view, render_sheet
    cell = 96
    view = default_view(cell)
    v, f = mm.icosphere(2, 0.9)
    big = np.array([[-4.0, -3.0, 0.0], [5.0, -2.5, -0.4], [0.5, 6.0, 0.2]], F)
    verts, faces = np.concatenate([v, big]), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]])
    rng = np.random.default_rng(11)
    first = None
    for trial in range(3):
        order = faces if trial == 0 else faces[rng.permutation(len(faces))]
        for shade in ("flat", "depth"):
            img = render_sheet([_column(verts, order, [[0, len(order), 0]], shade=shade)[0]], view=view, cell=cell, light=LIGHT).cpu().numpy()
            if trial == 0:
                first = dict(first or {}, **{shade: img})
                assert (img != 0).all()                            # the big triangle lies behind the sphere and fills the cell
            assert np.array_equal(img, first[shade]), (trial, shade)


@pytest.fixture(scope="module")
def sphere_clouds():
    g = torch.Generator().manual_seed(21)
    pts = torch.randn(2, 512, 3, generator=g)
    pts = pts / pts.norm(dim=2, keepdim=True) * torch.tensor([0.8, 0.5]).view(2, 1, 1)
    return pts.contiguous().to(_dev())


def test_surface_nets_local_indices_and_a_meshset_of_them_draw_the_same_bytes(sphere_clouds):
    from pdgn_amd.reconstruct import reconstruct, to_meshset
    from pdgn_amd.report import MeshColumn, default_view, fit_frames, fit_unit_sphere, render_sheet
    cell = 64
    view = default_view(cell)
    verts, faces, vert_off, face_off, _ = reconstruct(sphere_clouds, resolution=16)
    local = MeshColumn.from_surface_nets(verts, faces, vert_off, face_off)
    counts = local.face_count.tolist()
    assert min(counts) > 50
    ms = to_meshset(verts, faces, vert_off, face_off).to(_dev())
    glob = MeshColumn.from_meshset(ms)
    assert glob.vert_base.tolist() == [0, 0] and local.vert_base.tolist() == vert_off[:-1].tolist() and local.vert_base[1] > 0
    a = render_sheet([local], view=view, cell=cell, light=LIGHT).cpu().numpy()
    b = render_sheet([glob], view=view, cell=cell, light=LIGHT).cpu().numpy()
    want = mm.render([mm.mesh_column(verts.cpu().numpy(), faces.cpu().numpy(), local.range.cpu().numpy())], view, _light(), cell)
    assert np.array_equal(a, b) and np.array_equal(a, want) and all((want[r * cell:(r + 1) * cell] != 0).sum() > 200 for r in range(2))
    # in the clouds' frames the mesh lies where the fitted clouds lie: fit=True of the mesh alone and the cloud's frame agree to a voxel
    framed = local.in_frames(*fit_frames(sphere_clouds))
    sheet = render_sheet([fit_unit_sphere(sphere_clouds), framed], cell=cell).cpu().numpy()
    for r in range(2):
        cloud, mesh = (sheet[r * cell:(r + 1) * cell, c * cell:(c + 1) * cell] != 0 for c in range(2))
        rows_c, rows_m = np.nonzero(cloud.any(axis=1))[0], np.nonzero(mesh.any(axis=1))[0]
        assert abs(rows_c[0] - rows_m[0]) <= 4 and abs(rows_c[-1] - rows_m[-1]) <= 4      # (R = 16: a voxel is about four pixels)
    assert np.array_equal(render_sheet([local], cell=cell, fit=True).cpu().numpy(), render_sheet([local.fitted()], cell=cell).cpu().numpy())


def _direct(clouds, normals, view, light, cell, radius):
    """pdgn_render_sheet / pdgn_render_sheet_lit called as the library exports them: point-major (B,N,3) clouds."""
    from pdgn_amd import _lib
    L = _lib.lib()
    B, n = clouds[0].shape[0], len(clouds)
    ws = torch.empty(L.pdgn_render_workspace_bytes(B, n, cell) // 4, dtype=torch.int32, device=_dev())
    image = torch.empty((B * cell, n * cell), dtype=torch.uint8, device=_dev())
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in clouds])
    counts = (ctypes.c_int * n)(*[t.shape[1] for t in clouds])
    v = np.ascontiguousarray(view, dtype=F)
    if normals is None:
        rc = L.pdgn_render_sheet(B, n, ptrs, counts, 0, v.ctypes.data_as(ctypes.c_void_p), cell, radius, _lib.ptr(ws), _lib.ptr(image),
                                 _lib.stream_of(image))
    else:
        nptrs = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in normals])
        rc = L.pdgn_render_sheet_lit(B, n, ptrs, nptrs, counts, 0, v.ctypes.data_as(ctypes.c_void_p), light.ctypes.data_as(ctypes.c_void_p), cell,
                                     radius, _lib.ptr(ws), _lib.ptr(image), _lib.stream_of(image))
    assert rc == 0
    torch.cuda.synchronize()
    return image.cpu().numpy()


def test_mixed_sheets_and_sheets_without_a_mesh(sphere_clouds):
    """(cloud, mesh, lit cloud): the cloud columns are those of a cloud-only call, the mesh column that of a mesh-only one.  Without a mesh
    column render_sheet is pdgn_render_sheet / pdgn_render_sheet_lit called directly."""
    from pdgn_amd import _lib
    from pdgn_amd.report import default_view, render_sheet
    cell, radius = 48, 2
    view = default_view(cell)
    g = torch.Generator().manual_seed(4)
    other = (torch.rand(2, 300, 3, generator=g) - 0.5).to(_dev()).contiguous()
    nrm = sphere_clouds / sphere_clouds.norm(dim=2, keepdim=True)
    v, f = mm.icosphere(2, 0.8)
    mesh = _column(np.concatenate([v, v * F(0.5)]), np.concatenate([f, f + len(v)]), [[0, len(f), 0], [len(f), len(f), 0]])[0]
    mixed = render_sheet([other, mesh, sphere_clouds], view=view, cell=cell, radius=radius, normals=[None, None, nrm], light=LIGHT).cpu().numpy()
    clouds_only = render_sheet([other, sphere_clouds], view=view, cell=cell, radius=radius, normals=[None, nrm], light=LIGHT).cpu().numpy()
    mesh_only = render_sheet([mesh], view=view, cell=cell, radius=radius, light=LIGHT).cpu().numpy()
    assert all((part != 0).any() for part in (clouds_only[:, :cell], clouds_only[:, cell:], mesh_only))
    assert np.array_equal(mixed[:, :cell], clouds_only[:, :cell]) and np.array_equal(mixed[:, 2 * cell:], clouds_only[:, cell:])
    assert np.array_equal(mixed[:, cell:2 * cell], mesh_only)
    # depth-shaded clouds beside a mesh, the (B,3,N) layout included, and "estimate" meaning the cloud columns
    plain = render_sheet([mesh, other.transpose(1, 2).contiguous(), sphere_clouds], view=view, cell=cell, radius=radius).cpu().numpy()
    want = render_sheet([other, sphere_clouds], view=view, cell=cell, radius=radius).cpu().numpy()
    assert np.array_equal(plain[:, cell:], want)
    est = render_sheet([sphere_clouds, mesh], view=view, cell=cell, radius=radius, normals="estimate").cpu().numpy()
    want = render_sheet([sphere_clouds], view=view, cell=cell, radius=radius, normals="estimate").cpu().numpy()
    assert np.array_equal(est[:, :cell], want)
    # no mesh column: the entry points render_sheet always went through
    light = _light()
    assert np.array_equal(render_sheet([other, sphere_clouds], view=view, cell=cell, radius=radius).cpu().numpy(),
                          _direct([other, sphere_clouds], None, view, None, cell, radius))
    assert np.array_equal(clouds_only, _direct([other, sphere_clouds], [None, nrm], view, light, cell, radius))
    # what the library refuses of a mesh sheet, before any launch
    L = _lib.lib()
    assert L.pdgn_render_sheet_mesh(2, 1, None, None, None, 0, None, None, None, None, None, None, None, None, None, cell, radius, None, None, None) == -1
    with pytest.raises(_lib.PdgnHipError):
        render_sheet([mesh], cell=5000)
    with pytest.raises(_lib.PdgnHipError):
        render_sheet([mesh, other], radius=17)


def _state_tensors(tr):
    ts = []
    for net in [tr.G] + tr.D:
        ts += list(net.parameters()) + list(net.buffers())
    for opt in [tr.optG] + tr.optD:
        for st in opt.state.values():
            ts += [v for v in st.values() if torch.is_tensor(v)]
    return ts


def test_a_reporter_with_a_mesh_column(tmp_path, monkeypatch):
    """A tiny trainer, one step old: mesh=16 writes a sheet six cells wide and leaves the training state as found; without `mesh` the
    preview is byte for byte that of a reporter constructed without the argument."""
    from pdgn_amd import report
    from pdgn_amd.data import normalize_clouds
    from pdgn_amd.report import SnapshotReporter
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    dev = _dev()
    rows, cell = 2, 48
    g = torch.Generator().manual_seed(4)
    val = torch.randn(5, 2048, 3, generator=g)
    val = normalize_clouds((val / val.norm(dim=2, keepdim=True)).contiguous(), "shape_bbox")[0].to(dev).contiguous()
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    tr.step(synthetic_batch(4, dev), noise(4, dev), noise(4, dev))
    torch.cuda.synchronize()
    common = dict(every=1, batch_size=4, normalize="shape_bbox", seed=9, rows=rows, cell=cell)
    with_mesh = SnapshotReporter(tr, val, tmp_path / "mesh", mesh=16, **common)
    plain = SnapshotReporter(tr, val, tmp_path / "plain", **common)
    off = SnapshotReporter(tr, val, tmp_path / "off", mesh=None, **common)
    ts = _state_tensors(tr)
    before = [t.detach().clone() for t in ts]
    modes = [m.training for net in [tr.G] + tr.D for m in net.modules()]
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    drawn, render = [], report.render_sheet

    def recording(columns, **kw):                                  # what the reporter hands to the rasteriser
        drawn.append(list(columns))
        return render(columns, **kw)

    with monkeypatch.context() as patch:
        patch.setattr(report, "render_sheet", recording)
        assert with_mesh(1) is not None
    torch.cuda.synchronize()
    after = _state_tensors(tr)
    assert len(after) == len(before) > 100 and all(a is t for a, t in zip(after, ts)) and all(torch.equal(a, b) for a, b in zip(after, before))
    assert modes == [m.training for net in [tr.G] + tr.D for m in net.modules()] and all(modes)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    img = rm.read_png((tmp_path / "mesh" / "preview_1.png").read_bytes())
    assert img.shape == (rows * cell, 6 * cell)
    # The last column shows something exactly where the reconstruction has a face.  (A generator one step old draws a blob a few 1e-4
    # wide with outliers around it: no grid node has data, the reconstruction has no face -- empty cells, not an error.  What the
    # column shows of a generator that draws surfaces: the next test.)
    (columns,) = drawn
    assert len(columns) == 6 and all(isinstance(c, torch.Tensor) for c in columns[:5]) and isinstance(columns[5], report.MeshColumn)
    faces = columns[5].face_count.cpu().numpy()
    print("reporter mesh column: faces per row %s, %d pixels lit" % (faces.tolist(), int((img[:, 5 * cell:] != 0).sum())))
    for r in range(rows):
        assert (img[r * cell:(r + 1) * cell, 5 * cell:] != 0).any() == bool(faces[r] > 0)
    assert all((img[:, c * cell:(c + 1) * cell] != 0).any() for c in range(5))
    assert plain(1) is not None and off(1) is not None
    a, b = (tmp_path / "plain" / "preview_1.png").read_bytes(), (tmp_path / "off" / "preview_1.png").read_bytes()
    assert rm.read_png(a).shape == (rows * cell, 5 * cell) and a == b
    assert np.array_equal(rm.read_png(a)[:, 4 * cell:], img[:, 4 * cell:5 * cell])       # the reference column is the same with the mesh column
    assert sorted(p.name for p in (tmp_path / "mesh").iterdir()) == ["metrics.csv", "preview_1.png"]
    with pytest.raises(ValueError):
        SnapshotReporter(tr, val, tmp_path / "bad", mesh=1, **common)


class _SphereGenerator(torch.nn.Module):
    """A generator whose clouds are surfaces: four nested samples of a sphere whose radius follows z.  What a reporter asks of a
    generator: the four outputs as (B,3,n), the train / eval flag, the forward hints."""

    def __init__(self):
        super().__init__()
        d = torch.randn(2048, 3, generator=torch.Generator().manual_seed(12))
        self.register_buffer("dirs", d / d.norm(dim=1, keepdim=True))
        self.gain = torch.nn.Parameter(torch.ones(1))

    def forward(self, z):
        r = (0.5 + 0.2 * torch.tanh(z[:, :1])) * self.gain                         # (B,1)
        return [(self.dirs[:n].t()[None] * r[:, :, None]).contiguous() for n in (256, 512, 1024, 2048)]

    def forward_hints(self):
        return []

    def restore_forward_hints(self, hints):
        pass


class _SphereTrainer:
    ema = None

    def __init__(self, dev):
        self.G = _SphereGenerator().to(dev).train()


def test_the_reporters_mesh_columns_show_the_surfaces(tmp_path):
    """mesh=16 on a generator that draws spheres: column 5 is their reconstruction, where the finest clouds are; with fidelity= a column 6
    shows the validation shapes themselves."""
    from pdgn_amd.meshes import MeshSet
    from pdgn_amd.report import SnapshotReporter
    dev = _dev()
    rows, cell = 2, 48
    shapes = [mm.icosphere(2, 0.4 + 0.1 * i) for i in range(4)]
    ms = MeshSet.from_meshes([(v + F(0.05 * i), f) for i, (v, f) in enumerate(shapes)]).to(dev)
    val = ms.sample(2048, seed=3).contiguous()
    tr = _SphereTrainer(dev)
    common = dict(every=1, batch_size=4, normalize=None, seed=9, rows=rows, cell=cell)
    assert SnapshotReporter(tr, val, tmp_path / "six", mesh=16, **common)(1) is not None
    img = rm.read_png((tmp_path / "six" / "preview_1.png").read_bytes())
    assert img.shape == (rows * cell, 6 * cell) and tr.G.training
    for r in range(rows):
        cloud, mesh = (img[r * cell:(r + 1) * cell, c * cell:(c + 1) * cell] != 0 for c in (3, 5))
        assert mesh.sum() > cell * cell // 4                       # a filled disc where the cloud is a sprinkle of points ...
        (cy, my), (cx, mx) = ((np.nonzero(m.any(axis=a))[0] for m in (cloud, mesh)) for a in (1, 0))
        assert max(abs(cy[0] - my[0]), abs(cy[-1] - my[-1]), abs(cx[0] - mx[0]), abs(cx[-1] - mx[-1])) <= 5      # ... in the cloud's frame
    assert SnapshotReporter(tr, val, tmp_path / "seven", mesh=16, fidelity=ms, **common)(1) is not None
    seven = rm.read_png((tmp_path / "seven" / "preview_1.png").read_bytes())
    assert seven.shape == (rows * cell, 7 * cell) and np.array_equal(seven[:, :6 * cell], img)
    assert all((seven[r * cell:(r + 1) * cell, 6 * cell:] != 0).sum() > cell * cell // 4 for r in range(rows))
    assert sorted(p.name for p in (tmp_path / "seven").iterdir()) == ["fidelity.csv", "metrics.csv", "preview_1.png"]


def test_command_lines_write_sheets_of_the_right_size(tmp_path, capsys):
    from pdgn_amd import meshes, report
    v0, f0 = mm.icosphere(1, 1.0)
    v1, f1 = mm.icosphere(2, 3.0)
    packed = tmp_path / "two.npz"
    np.savez(packed, **{"00000001/val/verts": np.concatenate([v0, v1 + F(7.0)]), "00000001/val/faces": np.concatenate([f0, f1 + len(v0)]).astype(np.int32),
                        "00000001/val/face_off": np.array([0, len(f0), len(f0) + len(f1)], np.int32)})
    out = tmp_path / "sheet.png"
    meshes.main(["render", str(packed), "-o", str(out), "--cell", "40", "--rows", "8", "--split", "val"])
    img = rm.read_png(out.read_bytes())
    assert img.shape == (2 * 40, 40) and all((img[r * 40:(r + 1) * 40] != 0).sum() > 400 for r in range(2))     # fitted: each fills its cell
    meshes.main(["render", str(packed), "-o", str(out), "--cell", "24", "--rows", "1", "--shade", "depth", "--shape", "1,0,1"])
    img = rm.read_png(out.read_bytes())
    assert img.shape == (24, 3 * 24) and np.array_equal(img[:, :24], img[:, 48:]) and (img[:, 24:48] != 0).any()
    with pytest.raises(SystemExit):
        meshes.main(["render", str(packed), "-o", str(out), "--visible"])             # the file holds no masks
    with pytest.raises(SystemExit):
        meshes.main(["render", str(packed), "--shade", "phong"])
    g = torch.Generator().manual_seed(8)
    pts = torch.randn(4, 512, 3, generator=g)
    np.save(tmp_path / "out.npy", (pts / pts.norm(dim=2, keepdim=True)).numpy())
    report.main([str(tmp_path / "out.npy"), "-o", str(out), "--mesh", "16", "--rows", "2", "--cell", "32"])
    img = rm.read_png(out.read_bytes())
    assert img.shape == (2 * 32, 4 * 32)                           # two cloud columns, each with its reconstruction beside it
    assert all((img[r * 32:(r + 1) * 32, c * 32:(c + 1) * 32] != 0).any() for r in range(2) for c in range(4))
    capsys.readouterr()
