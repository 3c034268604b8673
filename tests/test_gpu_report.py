"""Snapshot reports on the device (pdgn_amd/report.py, csrc/render.hip): the rasteriser bit for bit against its numpy mirror
(tests/render_mirror.py) on inputs whose projection is exact, its properties on random clouds, the cheap metrics against the
full evaluation's CD entries, and a report inside `fit` that leaves the training state as it found it."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_mirror as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(rm.LATTICE_VIEWS))
@pytest.mark.parametrize("radius", [0, 1, 3])
@pytest.mark.parametrize("B,N", [(1, 256), (1, 2048), (35, 256), (35, 2048)])
def test_sheet_is_bit_equal_to_the_mirror_on_lattice_inputs(name, radius, B, N):
    """Coordinates on the 2^-8 lattice, a dyadic view: every fp32 operation of the projection is exact (checked on the host,
    tests/test_report_host.py), so the image must equal the mirror's.  Two columns of different point counts, one handed over
    point-major, one in the reference's (B,3,N) layout; points outside their cell and 64 points piled on one pixel included."""
    from pdgn_amd.report import render_sheet
    view, cell = rm.LATTICE_VIEWS[name], rm.LATTICE_CELL
    clouds = rm.lattice_clouds(B, N, seed=100 + B + N)
    want = rm.render(clouds, view, cell, radius)
    dev_clouds = [torch.from_numpy(clouds[0]).to(_dev()),
                  torch.from_numpy(np.ascontiguousarray(clouds[1].transpose(0, 2, 1))).to(_dev())]
    got = render_sheet(dev_clouds, view=view, cell=cell, radius=radius)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B * cell, 2 * cell)
    got = got.cpu().numpy()
    print("lattice %s r=%d B=%d N=%d: %d pixels differ of %d, %d lit" % (name, radius, B, N, int((got != want).sum()), want.size,
                                                                          int((want != 0).sum())))
    assert np.array_equal(got, want)
    # the generator's own output form, a (B,3,N) view of point-major memory, is taken as it is
    as_view = render_sheet([dev_clouds[0].transpose(1, 2), dev_clouds[1]], view=view, cell=cell, radius=radius)
    assert np.array_equal(as_view.cpu().numpy(), want)


@pytest.mark.parametrize("radius", [0, 2])
def test_random_clouds_render_repeatably_and_cover_their_points(radius):
    from pdgn_amd.report import default_view, fit_unit_sphere, render_sheet
    cell, B = 96, 5
    g = torch.Generator().manual_seed(7)
    clouds = [fit_unit_sphere(torch.randn(B, n, 3, generator=g)).to(_dev()) * s for n, s in ((512, 1.0), (2048, 1.6))]   # the second leaves its cells
    a = render_sheet(clouds, cell=cell, radius=radius)
    b = render_sheet(clouds, cell=cell, radius=radius)
    assert torch.equal(a, b)
    img = a.cpu().numpy()
    view = default_view(cell)
    eps = 1e-3                                                                  # fp32 fused chain against fp64: far below this
    for c, pts in enumerate(clouds):
        u, v, _ = rm.project(pts.cpu().numpy(), view, np.float64)
        for bi in range(B):
            cellimg = img[bi * cell:(bi + 1) * cell, c * cell:(c + 1) * cell]
            reach = np.zeros((cell, cell), dtype=bool)
            for du in (-eps, eps):
                for dv in (-eps, eps):
                    iu, iv = np.floor(u[bi] + du).astype(int), np.floor(v[bi] + dv).astype(int)
                    for dy in range(-radius, radius + 1):
                        for dx in range(-radius, radius + 1):
                            if dx * dx + dy * dy > radius * radius:             # the disc, not its bounding square
                                continue
                            px, py = iu + dx, iv + dy
                            ok = (px >= 0) & (px < cell) & (py >= 0) & (py < cell)
                            reach[py[ok], px[ok]] = True
            assert not (cellimg != 0)[~reach].any()                              # lit pixels lie within `radius` of a point of this cell
            sure = (np.floor(u[bi] - eps) == np.floor(u[bi] + eps)) & (np.floor(v[bi] - eps) == np.floor(v[bi] + eps))
            iu, iv = np.floor(u[bi]).astype(int), np.floor(v[bi]).astype(int)
            inside = sure & (iu >= 0) & (iu < cell) & (iv >= 0) & (iv < cell)
            assert inside.sum() > 100 and (cellimg[iv[inside], iu[inside]] != 0).all()   # every in-cell point's pixel is lit
    assert (img[:, cell:] != 0).any() and (img[:, :cell] != 0).any()


def test_render_sheet_refuses_what_the_kernel_does_not_take():
    from pdgn_amd._lib import PdgnHipError
    from pdgn_amd.report import render_sheet
    x = torch.zeros(2, 16, 3, device=_dev())
    with pytest.raises(PdgnHipError):
        render_sheet(x, radius=17)
    with pytest.raises(PdgnHipError):
        render_sheet(x, cell=5000)
    with pytest.raises(ValueError):
        render_sheet([x] * 9)
    with pytest.raises(ValueError):
        render_sheet([x, x[:1]])


def _small_generator():
    from pdgn_amd.generator import PointGenerator
    torch.manual_seed(2)
    return PointGenerator(base_points=16).to(_dev())


def test_quick_metrics_equal_the_cd_entries_of_the_full_evaluation(monkeypatch):
    """The same kernels produce both results: 1e-6 relative.  The EMD kernel is not launched; a warm cache skips the ref-vs-ref
    pass; the generator's mode and torch's RNG state are left alone."""
    from pdgn_amd import _lib, evaluation as ev
    from pdgn_amd.data import normalize_clouds
    from pdgn_amd.report import QUICK_KEYS, quick_metrics
    G = _small_generator().eval()
    ref = (normalize_clouds(torch.randn(10, 256, 3, device=_dev()) * 0.3, "shape_bbox")[0] * 0.45).contiguous()
    _, full = ev.generate_and_evaluate(G, ref, batch_size=4, normalize="shape_bbox", rng=torch.Generator().manual_seed(5))
    L = _lib.lib()
    calls = {"emd": 0, "cd": 0}
    emd_entry, cd_entry = L.pdgn_emd_cost_indexed, L.pdgn_chamfer_gram_indexed

    def counted(name, fn):
        def call(*a):
            calls[name] += 1
            return fn(*a)
        return call

    monkeypatch.setattr(L, "pdgn_emd_cost_indexed", counted("emd", emd_entry))
    monkeypatch.setattr(L, "pdgn_chamfer_gram_indexed", counted("cd", cd_entry))
    G.train()
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(_dev())
    cache = {}
    quick = quick_metrics(G, ref, 4, "shape_bbox", torch.Generator().manual_seed(5), cache)
    assert G.training and all(m.training for m in G.modules())
    assert calls == {"emd": 0, "cd": 3}                                         # ref-ref, sample-ref, sample-sample
    again = quick_metrics(G, ref, 4, "shape_bbox", torch.Generator().manual_seed(5), cache)
    assert calls == {"emd": 0, "cd": 5}                                         # the ref-vs-ref pass is not repeated
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(_dev()), dev_state)
    assert set(quick) == set(QUICK_KEYS) == set(again)
    for k in QUICK_KEYS:
        a, b, c = float(quick[k]), float(full[k]), float(again[k])
        print("%-16s quick %.9g full %.9g" % (k, a, b))
        assert abs(a - b) <= 1e-6 * abs(b) and a == c, (k, a, b, c)
    ev.pairwise_emd_cd(ref[:2], ref[:2])                                        # the wrapper does see the full path's launch
    assert calls["emd"] == 1


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


def test_fit_with_a_reporter_writes_reports_and_leaves_training_alone(tmp_path, monkeypatch):
    from pdgn_amd import report
    from pdgn_amd.data import BatchFeeder, normalize_clouds
    from pdgn_amd.report import QUICK_KEYS, SnapshotReporter
    from pdgn_amd.trainer import PDGNTrainer
    dev = _dev()
    B, N, rows, cell = 4, 2048, 3, 64
    feeder = BatchFeeder(_toy_clouds(2 * B + 1, N, 3).to(dev), B, (256, 512, 1024), seed=5)
    val = normalize_clouds(_toy_clouds(6, N, 4), "shape_bbox")[0].to(dev).contiguous()
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    reporter = SnapshotReporter(tr, val, tmp_path / "report", every=1, batch_size=B, normalize="shape_bbox", seed=9, rows=rows, cell=cell)
    seen, drawn = [], []
    render = report.render_sheet

    def recording(clouds, **kw):                                               # what the reporter hands to the rasteriser
        drawn.append(([c.detach().clone() for c in clouds], kw))
        return render(clouds, **kw)

    monkeypatch.setattr(report, "render_sheet", recording)

    def hook(epoch):
        torch.cuda.synchronize()
        ts = _state_tensors(tr)
        before = [t.detach().clone() for t in ts]
        modes = [m.training for net in [tr.G] + tr.D for m in net.modules()]
        cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
        hints = tr.G.forward_hints()
        assert len(hints) == 4 and all(h.get("_rows_hint", 0) > 0 for h in hints)     # (left by forwards of B = 4 samples; a report forwards 3)
        seen.append(reporter(epoch))
        torch.cuda.synchronize()
        now = tr.G.forward_hints()
        assert [sorted(h) for h in now] == [sorted(h) for h in hints]
        assert all(a[k] is b[k] or a[k] == b[k] for a, b in zip(now, hints) for k in a)
        after = _state_tensors(tr)
        assert len(after) == len(before) and len(before) > 100
        assert all(a is t for a, t in zip(after, ts))                           # the same tensors ...
        assert all(torch.equal(a, b) for a, b in zip(after, before))            # ... holding the same values
        assert modes == [m.training for net in [tr.G] + tr.D for m in net.modules()] and all(modes)
        assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)

    lines = []
    assert tr.fit(feeder, 2, log=lines.append, on_epoch=hook) == 2
    torch.cuda.synchronize()
    assert len(lines) == 4 and [s[0] for s in seen] == [1, 2]
    sheets = []
    for epoch in (1, 2):
        img = rm.read_png((tmp_path / "report" / ("preview_%d.png" % epoch)).read_bytes())
        assert img.shape == (rows * cell, 5 * cell)                             # 256 .. 2048 and the reference column
        assert all((img[:, c * cell:(c + 1) * cell] != 0).any() for c in range(5))
        sheets.append(img)
    assert np.array_equal(sheets[0][:, 4 * cell:], sheets[1][:, 4 * cell:])     # the reference column does not change
    # what a sheet shows.  The PNG is, bit for bit, the rasteriser's image of the clouds the reporter drew (the rasteriser is
    # bitwise repeatable); those are the generator's four outputs for the reporter's fixed noise, in eval mode, and the first
    # `rows` held-out clouds.  The generator's outputs are compared as floats, with the parity bound of this repository (1e-4
    # relative, README; 1e-5 absolute for coordinates near zero of clouds of unit scale): a forward is not promised to be
    # bitwise repeatable, and a pixel is a discontinuous function of a coordinate.
    assert len(drawn) == 2 and all(kw == {"cell": cell, "radius": 1, "fit": True} for _, kw in drawn)
    assert np.array_equal(render(drawn[1][0], **drawn[1][1]).cpu().numpy(), sheets[1])

    def expected_clouds():
        tr.G.eval()
        with torch.no_grad():
            z = torch.randn(rows, 128, generator=torch.Generator(device=dev).manual_seed(9), device=dev)
            out = [o.clone() for o in tr.G(z)]
        tr.G.train()
        return out + [val[:rows]]

    hints = tr.G.forward_hints()
    want = expected_clouds()
    tr.G.restore_forward_hints(hints)
    assert [tuple(c.shape) for c in drawn[1][0]] == [(rows, 3, n) for n in (256, 512, 1024, 2048)] + [(rows, N, 3)]
    for got, ref in zip(drawn[1][0], want):
        assert torch.allclose(got, ref, rtol=1e-4, atol=1e-5)
    assert torch.equal(drawn[1][0][4], val[:rows])
    # the same noise every time: a second report at the same parameters draws the same clouds
    reporter(2)
    assert len(drawn) == 3
    for again, first in zip(drawn[2][0], drawn[1][0]):
        assert torch.allclose(again, first, rtol=1e-4, atol=1e-5)
    assert not torch.allclose(drawn[0][0][3], drawn[1][0][3], rtol=1e-4, atol=1e-5)   # ... and epoch 1's differ: the parameters moved
    with open(tmp_path / "report" / "metrics.csv") as f:
        table = list(csv.reader(f))
    assert table[0] == ["epoch"] + list(QUICK_KEYS) + ["seconds"] and [r[0] for r in table[1:]] == ["1", "2", "2"]
    assert all(len(r) == len(table[0]) and np.isfinite([float(v) for v in r]).all() for r in table[1:])
    assert reporter(3) is not None and reporter.every == 1                      # outside fit as well
    reporter.every = 2
    assert reporter(3) is None                                                  # not a multiple of `every`: nothing happens
    # the list captured before the reports still runs, and computes what it computes without a report in front of it: the same
    # iteration from the same state, once plainly and once behind a report (the step sums with float atomics, so not bit for
    # bit: the bound of list against eager, tests/test_gpu_schedule.py, 2e-3 * max(1, |value|))
    ts = _state_tensors(tr)
    snap = [t.detach().clone() for t in ts]
    plain = {k: v.item() for k, v in tr.step_list().items()}
    torch.cuda.synchronize()
    with torch.no_grad():
        for t, v in zip(ts, snap):
            t.copy_(v)
    assert reporter(4) is not None
    behind = {k: v.item() for k, v in tr.step_list().items()}
    torch.cuda.synchronize()
    assert set(plain) == set(behind) and len(plain) == 6
    for k in plain:
        print("step_list %-13s plain %.8f behind a report %.8f" % (k, plain[k], behind[k]))
        assert np.isfinite(plain[k]) and abs(behind[k] - plain[k]) <= 2e-3 * max(1.0, abs(plain[k])), (k, plain[k], behind[k])
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def test_cli_train_with_reports_then_render_the_test_phase_output(tmp_path):
    from pdgn_amd.data import cate_to_synsetid
    rng = np.random.default_rng(6)
    sid = cate_to_synsetid["chair"]
    np.savez(tmp_path / "toy.npz", **{"%s/%s" % (sid, sp): rng.standard_normal((n, 2048, 3)).astype(np.float32)
                                      for sp, n in (("train", 9), ("val", 5), ("test", 6))})
    common = [sys.executable, "-m", "pdgn_amd.train", "--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root",
              str(tmp_path / "toy.npz"), "--choice", "chair", "--batch_size", "4", "--seed", "1", "--save_dir", str(tmp_path / "res")]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run(common + ["--phase", "train", "--max_epoch", "1", "--snapshot", "1", "--report_every", "1", "--report_rows", "4"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    rep = tmp_path / "ck" / "toy" / "report"
    assert sorted(p.name for p in rep.iterdir()) == ["metrics.csv", "preview_1.png"]
    assert rm.read_png((rep / "preview_1.png").read_bytes()).shape == (4 * 128, 5 * 128)
    assert len((rep / "metrics.csv").read_text().splitlines()) == 2
    run = subprocess.run(common + ["--phase", "test", "--pretrain_model_G", "1_chair_G.pth", "--pretrain_model_D", "1_chair_D.pth"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    (out,) = list((tmp_path / "res").iterdir())
    sheet = tmp_path / "sheet.png"
    run = subprocess.run([sys.executable, "-m", "pdgn_amd.report", str(out / "out.npy"), "-o", str(sheet), "--rows", "3"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    img = rm.read_png(sheet.read_bytes())
    assert img.shape == (3 * 128, 2 * 128)                                      # six clouds: two columns of three
    # fitted into the unit sphere, every cloud lies inside the frame: each cell shows its cloud (a generator one epoch old
    # may well draw a blob of a few pixels: how many is not this test's business)
    assert all((img[r * 128:(r + 1) * 128, c * 128:(c + 1) * 128] != 0).any() for r in range(3) for c in range(2))
