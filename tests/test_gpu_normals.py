"""Surface normals on the device: pdgn_estimate_normals bit for bit against its numpy mirror
(tests/normals_mirror.py) in every launch regime, its refusals, the lit sheet byte for byte against the mirror, the surface variation
statistics, and a lit report with surface statistics that leaves the training state as it found it."""
import csv
import ctypes

import numpy as np
import pytest
import torch

import normals_mirror as nm
import render_mirror as rm

pytestmark = pytest.mark.gpu
F = np.float32
# (b, n, k): the smallest call; fewer points than a wave; one past a wave; one past a block of 256; the k limit; the level-1 shape, where
# the block size changes (35 x 256: workgroups of 64 threads, as in (2, 257, 16) and (1, 1000, 64)).  Then the launches of 256-thread
# workgroups, which copy a cloud of at most PDGN_NORMALS_STAGE_MAX_N = 4096 points into LDS first: 130 clouds of 257 points (a tail of
# one point in every second workgroup), the threshold itself and one point above it (gathers from L2 again).
SHAPES = [(1, 1, 1), (2, 3, 3), (3, 65, 8), (2, 257, 16), (1, 1000, 64), (35, 256, 16), (130, 257, 4), (16, 4096, 4), (16, 4097, 4)]


def _dev():
    return torch.device("cuda:0")


def _cloud(b, n, seed):
    return np.random.default_rng(seed).standard_normal((b, n, 3)).astype(F)


def _call(x, idx, orient=0, o=(0.0, 0.0, 0.0), eig=True, k=None, b=None, n=None):
    """The raw entry point on device tensors -> (rc, normals, eig or None)."""
    from pdgn_amd import _lib
    B, N, _ = x.shape
    normals = torch.full((B, N, 3), 7.0, dtype=torch.float32, device=x.device)
    e = torch.full((B, N, 3), 7.0, dtype=torch.float32, device=x.device) if eig else None
    rc = _lib.lib().pdgn_estimate_normals(B if b is None else b, N if n is None else n, idx.shape[2] if k is None else k, _lib.ptr(x),
                                          _lib.ptr(idx), orient, o[0], o[1], o[2], _lib.ptr(normals), _lib.ptr(e), _lib.stream_of(x))
    torch.cuda.synchronize()
    return rc, normals.cpu().numpy(), None if e is None else e.cpu().numpy()


@pytest.mark.parametrize("b,n,k", SHAPES)
def test_the_kernel_equals_the_mirror_bit_for_bit_on_knn_lists(b, n, k):
    from pdgn_amd import pointops
    x = _cloud(b, n, 10 + n)
    xd = torch.from_numpy(x).to(_dev())
    idx = pointops.knnquery(k, xd, xd)
    assert (idx[:, :, 0].cpu() == torch.arange(n, dtype=torch.int32)).all()     # the point itself comes first
    want_n, want_e = nm.estimate(x, idx.cpu().numpy())
    rc, got_n, got_e = _call(xd, idx)
    assert rc == 0 and nm.same_bits(got_n, want_n) and nm.same_bits(got_e, want_e)
    assert np.isfinite(want_n).all() and (want_e[..., 0] <= want_e[..., 1]).all() and (want_e[..., 1] <= want_e[..., 2]).all()
    # eig = NULL writes the same normals; the Python wrapper returns what the entry point wrote
    rc, alone, none = _call(xd, idx, eig=False)
    assert rc == 0 and none is None and nm.same_bits(alone, want_n)
    if k <= n:
        py_n, py_e = pointops.estimate_normals(xd, k, return_eig=True)
        assert not py_n.requires_grad and nm.same_bits(py_n.cpu().numpy(), want_n) and nm.same_bits(py_e.cpu().numpy(), want_e)
        assert nm.same_bits(pointops.estimate_normals(xd, idx=idx).cpu().numpy(), want_n)


@pytest.mark.parametrize("b,n,k", SHAPES)
def test_the_kernel_equals_the_mirror_on_random_lists_with_repeats_and_poison(b, n, k):
    """Random indices (repeats are the rule), one entry of the whole call outside its cloud and, where the cloud has more than two points,
    one NaN and one infinite coordinate: NaNs in exactly the mirror's positions, every other bit equal."""
    rng = np.random.default_rng(20 + n)
    x = _cloud(b, n, 30 + n)
    idx = rng.integers(0, n, size=(b, n, k)).astype(np.int32)
    idx[b - 1, n // 2, k - 1] = (n, -1, n + 5, 2 ** 31 - 1)[n % 4]
    if n > 2:
        x[0, 1, 2], x[b - 1, n - 1, 0] = np.nan, np.inf
    want_n, want_e = nm.estimate(x, idx)
    assert np.isnan(want_n[b - 1, n // 2]).all() and (n <= 2 or np.isnan(want_n).any(axis=2).sum() > 1)
    assert n <= 3 or np.isfinite(want_n).any()
    rc, got_n, got_e = _call(torch.from_numpy(x).to(_dev()), torch.from_numpy(idx).to(_dev()))
    assert rc == 0 and nm.same_bits(got_n, want_n) and nm.same_bits(got_e, want_e)
    assert np.array_equal(np.isnan(got_n).all(axis=2), np.isnan(got_n).any(axis=2))      # a poisoned point is poisoned whole
    assert np.array_equal(np.isnan(got_n).all(axis=2), np.isnan(got_e).all(axis=2))


@pytest.mark.parametrize("orient,o", [(1, (0.3, -0.2, 0.9)), (2, (0.1, 0.0, -0.2)), (3, (0.1, 0.0, -0.2)), (3, (0.0, 0.0, 0.0))])
def test_the_sign_modes_equal_the_mirror(orient, o):
    from pdgn_amd import pointops
    x = nm.accuracy_clouds(0)["noisy512"][None]
    xd = torch.from_numpy(x).to(_dev())
    idx = pointops.knnquery(16, xd, xd)
    want_n, want_e = nm.estimate(x, idx.cpu().numpy(), orient, o)
    rc, got_n, got_e = _call(xd, idx, orient, o)
    assert rc == 0 and nm.same_bits(got_n, want_n) and nm.same_bits(got_e, want_e)
    kind = {1: "direction", 2: "towards", 3: "away"}[orient]
    assert nm.same_bits(pointops.estimate_normals(xd, 16, orient=(kind, o)).cpu().numpy(), want_n)
    plain = nm.estimate(x, idx.cpu().numpy())[0]
    assert np.array_equal(np.abs(got_n), np.abs(plain)) and not np.array_equal(got_n, plain)


def test_every_refusal_writes_nothing():
    from pdgn_amd import _lib, pointops
    xd = torch.from_numpy(_cloud(2, 40, 1)).to(_dev())
    idx = pointops.knnquery(8, xd, xd)
    inf, nan = float("inf"), float("nan")
    cases = [dict(b=0), dict(b=-1), dict(n=0), dict(k=0), dict(k=65), dict(b=1 << 20, n=257), dict(orient=-1), dict(orient=4),
             dict(orient=1, o=(nan, 0.0, 1.0)), dict(orient=2, o=(0.0, inf, 1.0)), dict(orient=3, o=(0.0, 0.0, -inf))]
    for kw in cases:
        rc, normals, eig = _call(xd, idx, **kw)
        assert rc == -1 and (normals == 7.0).all() and (eig == 7.0).all(), kw
    assert _call(xd, idx, orient=0, o=(nan, inf, 0.0))[0] == 0                  # o is not read under orient 0
    L = _lib.lib()
    normals, eig = torch.full((2, 40, 3), 7.0, device=_dev()), torch.full((2, 40, 3), 7.0, device=_dev())
    s = _lib.stream_of(xd)
    p = _lib.ptr
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 2)
    for args in ((None, p(idx), p(normals), p(eig)), (p(xd), None, p(normals), p(eig)), (p(xd), p(idx), None, p(eig)),
                 (odd(xd), p(idx), p(normals), p(eig)), (p(xd), odd(idx), p(normals), p(eig)), (p(xd), p(idx), odd(normals), p(eig)),
                 (p(xd), p(idx), p(normals), odd(eig))):
        assert L.pdgn_estimate_normals(2, 40, 8, args[0], args[1], 0, 0.0, 0.0, 0.0, args[2], args[3], s) == -1
    torch.cuda.synchronize()
    assert (normals == 7.0).all() and (eig == 7.0).all()
    with pytest.raises(ValueError):
        pointops.estimate_normals(xd, 41)                                       # k <= N where the lists are made here
    with pytest.raises(ValueError):
        pointops.estimate_normals(xd, 8, orient=("sideways", (0, 0, 1)))
    with pytest.raises(ValueError):
        pointops.estimate_normals(xd, 8, orient=("away", (0, 1)))
    with pytest.raises(ValueError):
        pointops.estimate_normals(xd, idx=idx[:1])
    with pytest.raises(_lib.PdgnHipError):
        pointops.estimate_normals(xd, idx=idx, orient=("away", (0.0, nan, 0.0)))


# ---------------------------------------------------------------------------- the lit sheet
# dyadic views for cells of 16 pixels (entries multiples of 2^-6: with coordinates on the 2^-8 lattice every operation of the projection is
# exact, tests/render_mirror.py)
SMALL_VIEWS = {
    "axis": np.array([[10.0, 0.0, 0.0, 8.0], [0.0, -10.0, 0.0, 8.0], [0.0, 0.0, -0.4375, 0.5]], dtype=F),
    "tilted": np.array([[7.5, 0.0, -5.25, 8.0], [2.25, -8.25, 3.25, 8.0], [-0.25, -0.203125, -0.359375, 0.5]], dtype=F),
}


def _raw_sheet(clouds, view, cell, radius):
    """pdgn_render_sheet itself on point-major device clouds."""
    from pdgn_amd import _lib
    L = _lib.lib()
    B = clouds[0].shape[0]
    ws = torch.empty(L.pdgn_render_workspace_bytes(B, len(clouds), cell) // 4, dtype=torch.int32, device=_dev())
    image = torch.empty((B * cell, len(clouds) * cell), dtype=torch.uint8, device=_dev())
    ptrs = (ctypes.c_void_p * len(clouds))(*[t.data_ptr() for t in clouds])
    counts = (ctypes.c_int * len(clouds))(*[t.shape[1] for t in clouds])
    view = np.ascontiguousarray(view, dtype=F)
    assert L.pdgn_render_sheet(B, len(clouds), ptrs, counts, 0, view.ctypes.data_as(ctypes.c_void_p), cell, radius, _lib.ptr(ws), _lib.ptr(image),
                               _lib.stream_of(image)) == 0
    torch.cuda.synchronize()
    return image.cpu().numpy()


@pytest.mark.parametrize("name", sorted(SMALL_VIEWS))
def test_the_lit_sheet_equals_the_mirror_and_a_null_column_is_the_depth_sheet(name, monkeypatch):
    from pdgn_amd import _lib
    from pdgn_amd.report import render_sheet
    rows, cell, n, radius = 2, 16, 50, 1
    view = SMALL_VIEWS[name]
    rng = np.random.default_rng(41)
    # coordinates on the 2^-8 lattice of [-1, 1]^3, (2, 50, 3) and (2, 25, 3): part of each cloud leaves its cell
    clouds = [(rng.integers(-256, 257, size=(rows, m, 3)).astype(np.float64) / 256.0).astype(F) for m in (n, n // 2)]
    normals = rng.standard_normal((rows, n, 3))
    normals = (normals / np.linalg.norm(normals, axis=2, keepdims=True)).astype(F)
    normals[0, 3] = np.nan                                                      # a poisoned point is drawn in the darkest shade
    normals[1, 4] *= F(1.5)                                                     # ... and an overlong normal is clamped
    light = np.array([0.25, -0.5, 0.75], F)
    unit = light / np.sqrt((light * light).sum(dtype=F))
    dev = [torch.from_numpy(c).to(_dev()) for c in clouds]
    got = render_sheet(dev, view=view, cell=cell, radius=radius, normals=[torch.from_numpy(normals).to(_dev()), None], light=light).cpu().numpy()
    want = nm.render_lit(clouds, [normals, None], view, unit, cell, radius)
    print("lit %s: %d pixels differ of %d, %d lit, shades %d .. %d" % (name, int((got != want).sum()), want.size, int((want != 0).sum()),
                                                                        want[:, :cell][want[:, :cell] != 0].min(), want[:, :cell].max()))
    assert np.array_equal(got, want)
    depth = _raw_sheet(dev, view, cell, radius)
    assert np.array_equal(got[:, cell:], depth[:, cell:]) and not np.array_equal(got[:, :cell], depth[:, :cell])
    assert np.array_equal((got != 0), (depth != 0))                             # the shade changes, the coverage does not
    # the same with the lit column channel-major: the normals stay point-major
    cm = render_sheet([dev[0].transpose(1, 2).contiguous(), dev[1]], view=view, cell=cell, radius=radius,
                      normals=[torch.from_numpy(normals).to(_dev()), None], light=light)
    assert np.array_equal(cm.cpu().numpy(), want)
    # the default light is the viewing direction
    row = view[2, :3]
    headlit = render_sheet(dev, view=view, cell=cell, radius=radius, normals=[torch.from_numpy(normals).to(_dev()), None]).cpu().numpy()
    assert np.array_equal(headlit, nm.render_lit(clouds, [normals, None], view, row / np.sqrt((row * row).sum(dtype=F)), cell, radius))
    # without `normals` render_sheet is pdgn_render_sheet: the lit entry point is not called
    L = _lib.lib()
    calls = []
    entry = L.pdgn_render_sheet_lit
    monkeypatch.setattr(L, "pdgn_render_sheet_lit", lambda *a: calls.append(1) or entry(*a))
    assert np.array_equal(render_sheet(dev, view=view, cell=cell, radius=radius).cpu().numpy(), depth) and not calls
    assert np.array_equal(depth, rm.render(clouds, view, cell, radius))
    all_null = render_sheet(dev, view=view, cell=cell, radius=radius, normals=[None, None])
    assert calls and np.array_equal(all_null.cpu().numpy(), depth)


def test_estimated_normals_light_a_sheet_repeatably():
    from pdgn_amd import pointops
    from pdgn_amd.report import fit_unit_sphere, render_sheet
    x = torch.from_numpy(nm.accuracy_clouds(0)["sphere512"][None].repeat(2, axis=0)).to(_dev())
    a = render_sheet([x, x.transpose(1, 2).contiguous(), x.transpose(1, 2)], cell=64, fit=True, normals="estimate", normals_k=12)
    b = render_sheet([x, x.transpose(1, 2).contiguous(), x.transpose(1, 2)], cell=64, fit=True, normals="estimate", normals_k=12)
    given = render_sheet(x, cell=64, fit=True, normals=[pointops.estimate_normals(fit_unit_sphere(x), 12)])
    a = a.cpu().numpy()
    assert torch.equal(torch.from_numpy(a), b.cpu())
    assert np.array_equal(a[:, :64], a[:, 64:128]) and np.array_equal(a[:, :64], a[:, 128:]) and np.array_equal(a[:, :64], given.cpu().numpy())
    lit = a[:, :64][a[:, :64] != 0]
    # a lit sphere shows the whole range of shades (255 itself needs |n . l| == 1 to the last bit: no estimated normal promises that)
    assert lit.min() >= 48 and 250 <= lit.max() <= 255 and len(np.unique(lit)) > 50


# ---------------------------------------------------------------------------- surface variation
def test_surface_stats_on_a_plane_a_sphere_a_noisy_sphere_and_duplicates():
    from pdgn_amd import evaluation as ev
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2) / 8.0
    plane = np.concatenate([g, np.full((64, 1), 0.25)], axis=1).astype(F)
    got = ev.surface_stats(torch.from_numpy(np.stack([plane, plane[::-1].copy()])).to(_dev()), k=9)
    assert got == {"sv_mean": 0.0, "sv_p90": 0.0, "degenerate": 0}
    assert ev.surface_stats(torch.from_numpy(plane[None]).to(_dev())) == {"sv_mean": 0.0, "sv_p90": 0.0, "degenerate": 0}      # k = 16
    clouds = nm.accuracy_clouds(0)
    clean = ev.surface_stats(torch.from_numpy(clouds["sphere512"][None]).to(_dev()))
    noisy = ev.surface_stats(torch.from_numpy(clouds["noisy512"][None]).to(_dev()))
    print("surface variation: sphere %r, with 5 %% radial noise %r" % (clean, noisy))
    assert 0.0 < clean["sv_mean"] < noisy["sv_mean"] < 1.0 / 3 and clean["sv_p90"] < noisy["sv_p90"] and clean["sv_mean"] < clean["sv_p90"]
    assert clean["degenerate"] == 0 and noisy["degenerate"] == 0
    # against the mirror's eigenvalues, in fp64 numpy
    x = clouds["noisy512"]
    xd = torch.from_numpy(x[None]).to(_dev())
    from pdgn_amd import pointops
    eig = nm.estimate_cloud(x, pointops.knnquery(16, xd, xd)[0].cpu().numpy())[1].astype(np.float64)
    sigma = np.maximum(eig[:, 0], 0.0) / ((eig[:, 0] + eig[:, 1]) + eig[:, 2])
    assert abs(noisy["sv_mean"] - sigma.mean()) <= 1e-12 and abs(noisy["sv_p90"] - np.quantile(sigma, 0.9)) <= 1e-12
    # every point of the first cloud is the same point (dyadic coordinates: the mean is exact, the trace an exact zero)
    dup = np.stack([np.tile(np.array([[0.375, -1.5, 0.0625]], F), (512, 1)), clouds["sphere512"]])
    both = ev.surface_stats(torch.from_numpy(dup).to(_dev()), batch=1)
    assert both["degenerate"] == 512 and both["sv_mean"] == pytest.approx(clean["sv_mean"] / 2, rel=1e-12)
    for bad in (dict(k=0), dict(k=600), dict(batch=0)):
        with pytest.raises(ValueError):
            ev.surface_stats(torch.from_numpy(dup).to(_dev()), **bad)


# ---------------------------------------------------------------------------- the report
def _state_tensors(tr):
    ts = []
    for net in [tr.G] + tr.D:
        ts += list(net.parameters()) + list(net.buffers())
    for opt in [tr.optG] + tr.optD:
        for st in opt.state.values():
            ts += [v for v in st.values() if torch.is_tensor(v)]
    return ts


def _toy_clouds(S, N, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(S, N, 3, generator=g)
    return ((pts - pts.mean(dim=1, keepdim=True)) / pts.reshape(S, -1).std(dim=1).view(S, 1, 1)).contiguous()


def test_a_lit_report_with_surface_statistics_leaves_training_alone(tmp_path):
    from pdgn_amd.data import BatchFeeder, normalize_clouds
    from pdgn_amd.report import SnapshotReporter
    from pdgn_amd.trainer import PDGNTrainer
    dev = _dev()
    B, N, rows, cell = 4, 2048, 3, 64
    feeder = BatchFeeder(_toy_clouds(2 * B + 1, N, 3).to(dev), B, (256, 512, 1024), seed=5)
    val = normalize_clouds(_toy_clouds(6, N, 4), "shape_bbox")[0].to(dev).contiguous()
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    reals, z1, z2 = feeder.buffers()
    feeder.fill(1, 0, reals, z1, z2)
    tr.step(reals, z1, z2)                                                      # (so that the optimizers have state to leave alone)
    torch.cuda.synchronize()
    plain = SnapshotReporter(tr, val, tmp_path / "plain", every=1, batch_size=B, normalize="shape_bbox", seed=9, rows=rows, cell=cell)
    lit = SnapshotReporter(tr, val, tmp_path / "report", every=1, batch_size=B, normalize="shape_bbox", seed=9, rows=rows, cell=cell,
                           lit=True, surface=True)
    ts = _state_tensors(tr)
    before = [t.detach().clone() for t in ts]
    modes = [m.training for net in [tr.G] + tr.D for m in net.modules()]
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    assert lit(1) is not None and lit(2) is not None
    torch.cuda.synchronize()
    after = _state_tensors(tr)
    assert len(after) == len(before) > 100 and all(a is t for a, t in zip(after, ts))
    assert all(a.detach().cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(after, before))
    assert modes == [m.training for net in [tr.G] + tr.D for m in net.modules()] and all(modes)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    assert sorted(p.name for p in (tmp_path / "report").iterdir()) == ["metrics.csv", "preview_1.png", "preview_2.png", "surface.csv"]
    with open(tmp_path / "report" / "surface.csv") as f:
        table = list(csv.reader(f))
    assert table[0] == list(SnapshotReporter.SURFACE_HEADER) and [r[0] for r in table[1:]] == ["1", "2"]
    assert all(len(r) == 6 and np.isfinite([float(v) for v in r]).all() for r in table[1:])
    assert table[1][3:5] == table[2][3:5] and 0.0 < float(table[1][3]) < 1.0 / 3        # the val clouds do not change
    assert lit.last_surface[0] == 2 and lit.last_surface[2] is lit.cache["val_surface"]
    # the lit sheet covers the pixels the depth sheet covers, in other shades; the plain reporter writes what it always wrote
    assert plain(1) is not None
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["metrics.csv", "preview_1.png"]
    a = rm.read_png((tmp_path / "report" / "preview_1.png").read_bytes())
    b = rm.read_png((tmp_path / "plain" / "preview_1.png").read_bytes())
    assert a.shape == b.shape == (rows * cell, 5 * cell)
    assert np.array_equal(a[:, 4 * cell:] != 0, b[:, 4 * cell:] != 0) and not np.array_equal(a[:, 4 * cell:], b[:, 4 * cell:])
    assert b[b != 0].min() >= 128 and a[a != 0].min() < 128 and a[a != 0].min() >= 48
