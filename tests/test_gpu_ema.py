"""The averaged generator: pdgn_adam_ema_multi / pdgn_ema_multi (csrc/adam.hip) against pdgn_adam_multi and
the host mirror (tests/ema_mirror.py), the trainer's buffer through the eager step, the launch list and torch's own optimizer
kernel, the by-value swap of `averaged_generator()`, the third checkpoint file, resuming, the reports and the command line."""
import csv
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ema_mirror as em
import ema_worker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, EPS = 1e-4, 0.5, 0.999, 1e-8


def _state_tensors(tr):
    ts = []
    for net in [tr.G] + tr.D:
        ts += list(net.parameters()) + list(net.buffers())
    for opt in [tr.optG] + tr.optD:
        for st in opt.state.values():
            ts += [v for v in st.values() if torch.is_tensor(v)]
    return ts + ([tr.ema_buf] if tr.ema_buf is not None else [])


def _drop_list(tr):
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 1. the kernels
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 5, 100003, 5 * 4096] + [17 + 13 * i for i in range(80)]     # 90 tensors: two launches
OFFSET = {"p": {5: 1, 7: 3}, "g": {8: 1}, "m": {}, "v": {9: 2}, "e": {6: 1, 7: 3}}      # floats past a 16-byte boundary: 4-byte aligned only


def _lists(seed):
    """{name: [tensor per size]} for p, g, m, v, e: views of one buffer each, every view on a 16-byte boundary except those of
    OFFSET; the same values for the same seed."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = {}
    for name in "pgmve":
        slot = lambda n: (n + 3) // 4 * 4 + 4
        buf = torch.randn(sum(slot(n) for n in SIZES), device="cuda", generator=gen)
        if name == "g":
            buf *= 0.01
        if name == "v":
            buf = buf.abs() * 1e-4
        if name == "m":
            buf *= 0.01
        views, off = [], 0
        for i, n in enumerate(SIZES):
            o = off + OFFSET[name].get(i, 0)
            views.append(buf[o:o + n])
            off += slot(n)
        assert buf.data_ptr() % 16 == 0
        out[name] = views
    return out


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _counts(ts):
    return (ctypes.c_longlong * len(ts))(*[t.numel() for t in ts])


def _d(x):
    return ctypes.c_double(x)


@pytest.mark.parametrize("t", [1, 7, 5000])
def test_fused_launch_equals_adam_then_mirror_and_the_average_alone(t):
    from pdgn_amd import _lib
    L = _lib.lib()
    a, b, c = _lists(11), _lists(11), _lists(11)
    assert any(x.data_ptr() % 16 for x in a["p"]) and any(x.data_ptr() % 16 for x in a["e"]) and all(x.data_ptr() % 4 == 0 for x in a["e"])
    assert all(torch.equal(x, y) for k in "pgmve" for x, y in zip(a[k], b[k]))
    step = torch.tensor([float(t)], device="cuda")
    stream = _lib.stream_of(step)
    n = len(SIZES)
    decay = 0.999
    e0 = [e.cpu().numpy().copy() for e in a["e"]]
    p0 = [p.clone() for p in a["p"]]
    # a: pdgn_adam_multi alone, then the average alone;  b: the fused launch;  c: the average alone at decay 0.5 (the other branch of the min)
    _lib.check(L.pdgn_adam_multi(n, _arr(a["p"]), _arr(a["g"]), _arr(a["m"]), _arr(a["v"]), _counts(a["p"]), _d(LR), _d(B1), _d(B2), _d(EPS),
                                 _lib.ptr(step), stream), "pdgn_adam_multi")
    _lib.check(L.pdgn_adam_ema_multi(n, _arr(b["p"]), _arr(b["g"]), _arr(b["m"]), _arr(b["v"]), _arr(b["e"]), _counts(b["p"]), _d(LR), _d(B1),
                                     _d(B2), _d(EPS), _d(decay), _lib.ptr(step), stream), "pdgn_adam_ema_multi")
    torch.cuda.synchronize()
    assert any(not torch.equal(x, y) for x, y in zip(a["p"], p0))                # the step moved the parameters
    for k in "pmv":
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), (k, i, SIZES[i])
    for i, (e, start, p) in enumerate(zip(b["e"], e0, a["p"])):
        want = em.ema_update(start, p.cpu().numpy(), decay, t)
        assert np.array_equal(e.cpu().numpy(), want), (i, SIZES[i])
        assert not np.array_equal(want, start) or SIZES[i] < 4
    assert all(torch.equal(x, y) for x, y in zip(a["g"], c["g"]))                # read-only
    _lib.check(L.pdgn_ema_multi(n, _arr(a["e"]), _arr(a["p"]), _counts(a["p"]), _d(decay), _lib.ptr(step), stream), "pdgn_ema_multi")
    _lib.check(L.pdgn_ema_multi(n, _arr(c["e"]), _arr(a["p"]), _counts(a["p"]), _d(0.5), _lib.ptr(step), stream), "pdgn_ema_multi")
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(a["e"], b["e"])):
        assert torch.equal(x, y), (i, SIZES[i])                                  # adam, then the average alone == the fused launch
    for i, (e, start, p) in enumerate(zip(c["e"], e0, a["p"])):
        assert np.array_equal(e.cpu().numpy(), em.ema_update(start, p.cpu().numpy(), 0.5, t)), (i, SIZES[i])
    # nothing was written outside the tensors: the gaps between the views still hold what they held (the untouched copy's bytes)
    ref = _lists(11)
    for k in "pmve":
        base, base_ref = b[k][0]._base, ref[k][0]._base
        mask = torch.ones_like(base, dtype=torch.bool)
        for view in b[k]:
            o = (view.data_ptr() - base.data_ptr()) // 4
            mask[o:o + view.numel()] = False
        assert int(mask.sum()) > 0 and torch.equal(base[mask], base_ref[mask]), k


def test_invalid_arguments_are_refused_before_any_launch():
    from pdgn_amd import _lib
    L = _lib.lib()
    x = _lists(3)
    keep = [t.clone() for k in "pmve" for t in x[k]]
    step = torch.tensor([3.0], device="cuda")
    stream = _lib.stream_of(step)
    n = len(SIZES)
    P, G, M, V, E, N = _arr(x["p"]), _arr(x["g"]), _arr(x["m"]), _arr(x["v"]), _arr(x["e"]), _counts(x["p"])

    def fused(n=n, P=P, G=G, M=M, V=V, E=E, N=N, decay=0.999, step=_lib.ptr(step), lr=LR, b1=B1):
        return L.pdgn_adam_ema_multi(n, P, G, M, V, E, N, _d(lr), _d(b1), _d(B2), _d(EPS), _d(decay), step, stream)

    def alone(n=n, E=E, P=P, N=N, decay=0.999, step=_lib.ptr(step)):
        return L.pdgn_ema_multi(n, E, P, N, _d(decay), step, stream)

    def with_entry(ts, i, value):
        arr = _arr(ts)
        arr[i] = value
        return arr

    bad_counts = _counts(x["p"])
    bad_counts[80] = 0
    null = ctypes.c_void_p(0)
    INVALID = -1
    for rc in (fused(n=0), fused(decay=1.0), fused(decay=-0.001), fused(decay=float("nan")), fused(E=None), fused(P=None), fused(N=None),
               fused(step=null), fused(E=with_entry(x["e"], 70, None)), fused(E=with_entry(x["e"], 3, x["e"][3].data_ptr() + 2)),
               fused(P=with_entry(x["p"], 89, x["p"][89].data_ptr() + 1)), fused(N=bad_counts), fused(lr=-1.0), fused(b1=1.0),
               alone(n=0), alone(decay=1.0), alone(decay=-0.5), alone(decay=float("nan")), alone(E=None), alone(P=None), alone(N=None),
               alone(step=null), alone(E=with_entry(x["e"], 88, None)), alone(P=with_entry(x["p"], 2, x["p"][2].data_ptr() + 2)),
               alone(N=bad_counts)):
        assert rc == INVALID
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, [t for k in "pmve" for t in x[k]]))       # nothing ran
    e0 = [e.cpu().numpy().copy() for e in x["e"]]
    assert alone(decay=0.0) == 0                                                 # decay 0 is inside the range: e + 1 * (p - e), rounded as ever
    torch.cuda.synchronize()
    for e, start, p in zip(x["e"], e0, x["p"]):
        assert np.array_equal(e.cpu().numpy(), em.ema_update(start, p.cpu().numpy(), 0.0, 3))


# ---------------------------------------------------------------------------- 2. the trainer, and 4. the swap
def test_trainer_average_follows_the_mirror_and_the_swap_is_by_value(tmp_path, monkeypatch):
    from pdgn_amd import report
    from pdgn_amd.data import normalize_clouds
    from pdgn_amd.generator import PointGenerator, load_reference_state_dict
    tr, reals, z1, z2 = ema_worker.trainer_scenario()
    dev = tr.device
    params = list(tr.G.parameters())
    # ---- the third file, and what `averaged_generator()` computes
    paths = tr.save(str(tmp_path), 2, "chair")
    assert [os.path.basename(p) for p in paths] == ["2_chair_G.pth", "2_chair_D.pth", "2_chair_G_ema.pth"]
    g, ge = torch.load(paths[0]), torch.load(paths[2])
    assert set(ge) == set(g) | {"ema_decay"} and ge["ema_decay"] == 0.999 and list(ge["G_model"]) == list(g["G_model"])
    for (name, p), e in zip(tr.G.named_parameters(), tr._ema_in_module_order()):
        assert torch.equal(g["G_model"]["module." + name], p.detach().cpu()) and torch.equal(ge["G_model"]["module." + name], e.cpu())
    for k in set(g["G_model"]) - {"module." + n for n, _ in tr.G.named_parameters()}:
        assert torch.equal(g["G_model"][k], ge["G_model"][k])                    # the live buffers
    fresh = PointGenerator().to(dev)
    load_reference_state_dict(fresh, ge["G_model"])
    fresh.eval()
    z = torch.randn(4, 128, generator=torch.Generator(device=dev).manual_seed(5), device=dev) * 0.2
    ts = _state_tensors(tr)
    before = [t.detach().clone() for t in ts]
    ptrs = [p.data_ptr() for p in params]
    hints = tr.G.forward_hints()
    with torch.no_grad():
        fresh(z)                                                                 # (its first forward leaves the row count the
        want = [o.clone() for o in fresh(z)]                                     #  operands' arithmetic is chosen by: generator.py)
        with tr.averaged_generator() as G:
            assert G is tr.G and [p.data_ptr() for p in params] == ptrs
            assert all(torch.equal(p, e) for p, e in zip(tr.optG.param_groups[0]["params"], tr.ema))
            G.eval()
            G(z)
            inside = [o.clone() for o in G(z)]
            G.train()
        tr.G.eval()
        tr.G(z)
        live = [o.clone() for o in tr.G(z)]
        tr.G.train()
    tr.G.restore_forward_hints(hints)
    torch.cuda.synchronize()
    for lvl, (a, b, c) in enumerate(zip(inside, want, live)):
        print("level %d: |averaged - file| max %.3e, |averaged - live| max %.3e" % (lvl, (a - b).abs().max().item(), (a - c).abs().max().item()))
    for lvl, (a, b, c) in enumerate(zip(inside, want, live)):
        assert torch.equal(a, b), lvl                                            # the averaged generator IS the written file's
        assert not torch.equal(a, c), lvl                                        # ... and not the live one
    after = _state_tensors(tr)
    assert len(after) == len(before) and all(x is y for x, y in zip(after, ts))
    assert all(torch.equal(x, y) for x, y in zip(after, before))
    # ---- a report shows the averaged generator and leaves everything, the averages included, as found
    val = normalize_clouds(torch.randn(6, 2048, 3, generator=torch.Generator().manual_seed(4)), "shape_bbox")[0].to(dev).contiguous()
    drawn = []
    render = report.render_sheet
    monkeypatch.setattr(report, "render_sheet", lambda clouds, **kw: drawn.append([c.detach().clone() for c in clouds]) or render(clouds, **kw))
    rep = report.SnapshotReporter(tr, val, tmp_path / "report", every=1, batch_size=4, normalize="shape_bbox", seed=9, rows=3, cell=64)
    assert rep(1) is not None
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(_state_tensors(tr), before))
    now = tr.G.forward_hints()
    assert [sorted(h) for h in now] == [sorted(h) for h in hints] and all(h["_rows_hint"] == k["_rows_hint"] for h, k in zip(now, hints))
    with torch.no_grad(), tr.averaged_generator() as G:
        G.eval()
        zr = torch.randn(3, 128, generator=torch.Generator(device=dev).manual_seed(9), device=dev)
        shown = [o.clone() for o in G(zr)]
        G.train()
    tr.G.restore_forward_hints(hints)
    for got, ref in zip(drawn[0], shown):                                        # (the bound of tests/test_gpu_report.py for drawn clouds)
        assert torch.allclose(got, ref, rtol=1e-4, atol=1e-5)
    with open(tmp_path / "report" / "metrics.csv") as f:
        table = list(csv.reader(f))
    assert table[0] == ["epoch"] + list(report.QUICK_KEYS) + ["seconds"] and len(table) == 2
    # ---- the list captured before all this still runs, and keeps averaging
    e_before = [e.clone() for e in tr.ema]
    out = tr.step_list(None, z1, z2)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).item() for v in out.values())
    t = float(tr.optG.state[params[0]]["step"])
    for e, start, p in zip(tr.ema, e_before, tr.optG.param_groups[0]["params"]):
        assert np.array_equal(e.cpu().numpy(), em.ema_update(start.cpu().numpy(), p.detach().cpu().numpy(), 0.999, t))
    # ---- 5. save and resume
    from pdgn_amd.trainer import PDGNTrainer
    paths = tr.save(str(tmp_path), 3, "chair")
    torch.manual_seed(7)
    other = PDGNTrainer(device=dev, distributed=False, ema_decay=0.999)
    other.train()
    assert other.load(paths[0], paths[1]) == 3
    assert all(torch.equal(a, b) for a, b in zip(other.ema, tr.ema)) and all(torch.equal(a, b) for a, b in zip(other.G.parameters(), params))
    # the decay's warm-up continues from Adam's restored step count: one eager step (the optimizer's own step + the average alone)
    e_before = [e.clone() for e in other.ema]
    other.step(reals, z1, z2)
    torch.cuda.synchronize()
    assert float(other.optG.state[other.optG.param_groups[0]["params"][0]]["step"]) == t + 1
    for e, start, p in zip(other.ema, e_before, other.optG.param_groups[0]["params"]):
        assert np.array_equal(e.cpu().numpy(), em.ema_update(start.cpu().numpy(), p.detach().cpu().numpy(), 0.999, t + 1))
    os.remove(paths[2])
    assert other.load(paths[0], paths[1]) == 3
    assert all(torch.equal(a, b) for a, b in zip(other.ema, params))             # no file of averages: they start from the parameters
    _drop_list(tr)


def test_trainer_average_with_torchs_optimizer_kernel_in_a_child_process():
    env = dict(os.environ, PDGN_OWN_ADAM="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ema_worker.py")], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=600)
    assert run.returncode == 0 and "ema worker ok: PDGN_OWN_ADAM=0" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]


# ---------------------------------------------------------------------------- 3. off is off
def test_off_is_off(tmp_path):
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    dev = torch.device("cuda:0")
    torch.manual_seed(2)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    assert tr.ema_decay == 0.0 and tr.ema is None and tr.ema_buf is None and tr._ema_spare is None and tr._stepG.ema is None
    with pytest.raises(RuntimeError):
        with tr.averaged_generator():
            pass
    reals, z1, z2 = synthetic_batch(4, dev), noise(4, dev), noise(4, dev)
    for _ in range(2):
        tr.step(reals, z1, z2)
    torch.cuda.synchronize()
    assert tr.ema is None and tr._stepG._ema_table is None and tr._stepG.route == "own"
    assert len(tr.save(str(tmp_path), 1, "chair")) == 2
    assert sorted(os.listdir(tmp_path)) == ["1_chair_D.pth", "1_chair_G.pth"]


# ---------------------------------------------------------------------------- 6. the command line
def test_cli_trains_with_an_averaged_generator_and_evaluates_it(tmp_path):
    from pdgn_amd.data import cate_to_synsetid
    rng = np.random.default_rng(6)
    sid = cate_to_synsetid["chair"]
    np.savez(tmp_path / "toy.npz", **{"%s/%s" % (sid, sp): rng.standard_normal((n, 2048, 3)).astype(np.float32)
                                      for sp, n in (("train", 9), ("val", 5), ("test", 6))})
    common = [sys.executable, "-m", "pdgn_amd.train", "--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root",
              str(tmp_path / "toy.npz"), "--choice", "chair", "--batch_size", "4", "--seed", "1", "--save_dir", str(tmp_path / "res")]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run(common + ["--phase", "train", "--max_epoch", "1", "--snapshot", "1", "--ema_decay", "0.999", "--report_every", "1",
                                   "--report_rows", "4"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    ck = tmp_path / "ck" / "toy"
    assert sorted(p.name for p in (ck / "PDGNet_v2").iterdir()) == ["1_chair_D.pth", "1_chair_G.pth", "1_chair_G_ema.pth"]
    assert sorted(p.name for p in (ck / "report").iterdir()) == ["metrics.csv", "preview_1.png"]
    assert len((ck / "report" / "metrics.csv").read_text().splitlines()) == 2
    assert "ema_decay=0.999" in (ck / "log_info.txt").read_text().splitlines()[0]
    g, ge = torch.load(ck / "PDGNet_v2" / "1_chair_G.pth"), torch.load(ck / "PDGNet_v2" / "1_chair_G_ema.pth")
    assert ge["ema_decay"] == 0.999 and any(not torch.equal(a, b) for a, b in zip(g["G_model"].values(), ge["G_model"].values()))
    run = subprocess.run(common + ["--phase", "test", "--pretrain_model_G", "1_chair_G_ema.pth", "--pretrain_model_D", "1_chair_D.pth"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    (out,) = list((tmp_path / "res").iterdir())
    clouds = np.load(out / "out.npy")
    assert clouds.shape == (6, 2048, 3) and np.isfinite(clouds).all()
