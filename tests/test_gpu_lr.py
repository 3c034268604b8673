"""Learning-rate schedules on the device: pdgn_adam_sched_multi's four kernels against the unscheduled entry
points at the mirror's rate (tests/lr_mirror.py), pdgn_lr_eval against the mirror, LeanAdamStep's three routes, the launch list
reading the table (not a baked value), per-network rates, and resuming."""
import ctypes

import numpy as np
import pytest
import torch

import lr_mirror as lm

pytestmark = pytest.mark.gpu
LR, B1, B2, EPS, DECAY = 1e-4, 0.5, 0.999, 1e-8, 0.999
NETS = ("G", "D1", "D2", "D3", "D4")


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _counts(ts):
    return (ctypes.c_longlong * len(ts))(*[t.numel() for t in ts])


def _device_table(tab):
    return torch.from_numpy(np.asarray(tab, dtype=np.float64)).cuda()


# ---------------------------------------------------------------------------- 1. the kernels
# the lists of tests/test_gpu_ema.py: sizes 1 / 3 / 4097, several chunks, tensors at 4-byte-only offsets (the scalar path), and 79
# tensors: more than one launch holds (72, or 64 with the averages)
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 5, 5 * 4096] + [17 + 13 * i for i in range(70)]
OFFSET = {"p": {5: 1, 7: 3}, "g": {8: 1}, "m": {}, "v": {9: 2}, "e": {6: 1, 7: 3}}      # floats past a 16-byte boundary
KNOTS4 = [(3, 0.5), (7, 1.25), (10000, 0.2), (15000, 0.05)]                            # t = 1 before, 7 on a knot, 5000 inside, 20000 past


def _lists(seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = {}
    for name in "pgmve":
        slot = lambda n: (n + 3) // 4 * 4 + 4
        buf = torch.randn(sum(slot(n) for n in SIZES), device="cuda", generator=gen)
        if name in "gm":
            buf *= 0.01
        if name == "v":
            buf = buf.abs() * 1e-4
        views, off = [], 0
        for i, n in enumerate(SIZES):
            o = off + OFFSET[name].get(i, 0)
            views.append(buf[o:o + n])
            off += slot(n)
        assert buf.data_ptr() % 16 == 0
        out[name] = views
    return out


def _bases(x, keys="pgmve"):
    return {k: x[k][0]._base.clone() for k in keys}


def _same(a, b, keys):
    for k in keys:
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), (k, i, SIZES[i])


def _adam(x, lr, t, ema, record=None, sched=None):
    """One launch set on the lists x at step count t: the unscheduled entry points (sched None) or pdgn_adam_sched_multi."""
    from pdgn_amd import _lib
    L = _lib.lib()
    step = torch.tensor([float(t)], device="cuda")
    n, N, s = len(x["p"]), _counts(x["p"]), _lib.stream_of(step)
    P, G, M, V, E = _arr(x["p"]), _arr(x["g"]), _arr(x["m"]), _arr(x["v"]), _arr(x["e"])
    rec = _lib.ptr(record) if record is not None else None
    if sched is not None:
        rc = L.pdgn_adam_sched_multi(n, P, G, M, V, E if ema else None, N, lr, B1, B2, EPS, DECAY if ema else 0.0, _lib.ptr(step), rec,
                                     _lib.ptr(sched), s)
    elif record is None:
        rc = (L.pdgn_adam_ema_multi(n, P, G, M, V, E, N, lr, B1, B2, EPS, DECAY, _lib.ptr(step), s) if ema else
              L.pdgn_adam_multi(n, P, G, M, V, N, lr, B1, B2, EPS, _lib.ptr(step), s))
    else:
        rc = (L.pdgn_adam_ema_guard_multi(n, P, G, M, V, E, N, lr, B1, B2, EPS, DECAY, _lib.ptr(step), rec, s) if ema else
              L.pdgn_adam_guard_multi(n, P, G, M, V, N, lr, B1, B2, EPS, _lib.ptr(step), rec, s))
    _lib.check(rc, "adam")
    torch.cuda.synchronize()
    assert float(step) == float(t)                                                # the launches read the counter, never write it


def _measure(grads, max_norm=0.0):
    from pdgn_amd import _lib
    L = _lib.lib()
    n, counts = len(grads), _counts(grads)
    ws = torch.zeros(L.pdgn_gradnorm_workspace_doubles(n, counts), dtype=torch.float64, device="cuda")
    rec = torch.zeros(8, dtype=torch.float32, device="cuda")
    _lib.check(L.pdgn_gradnorm_multi(n, _arr(grads), counts, max_norm, _lib.ptr(ws), ws.numel(), _lib.ptr(rec), _lib.stream_of(rec)), "gradnorm")
    torch.cuda.synchronize()
    return rec


@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("t", [1, 7, 5000, 20000])
def test_scheduled_launch_equals_the_unscheduled_one_at_the_mirrors_rate(t, ema):
    tab = lm.table(KNOTS4)
    sched = _device_table(tab)
    rate = float(lm.lr_eff(LR, tab, t))
    f = float(lm.factor(tab, t))
    assert {1: f == 0.5, 7: f == 1.25, 5000: 0.2 < f < 1.25, 20000: f == 0.05}[t] and rate != LR
    keys = "pmve" if ema else "pmv"
    # ---- no guard: the unscheduled launch given the Python float lr * f(t)
    a, b, c = _lists(21), _lists(21), _lists(21)
    assert any(x.data_ptr() % 16 for x in a["p"]) and all(x.data_ptr() % 4 == 0 for x in a["p"])
    _adam(a, rate, t, ema)
    _adam(b, LR, t, ema, sched=sched)
    _same(a, b, keys)
    _adam(c, LR, t, ema)                                                          # (the factor did something: not the base rate's result)
    assert any(not torch.equal(x, y) for x, y in zip(c["p"], b["p"])) and all(torch.equal(x, y) for x, y in zip(c["m"], b["m"]))
    ref = _bases(_lists(21))
    for k in "g" + ("" if ema else "e"):                                          # read-only; without the average e is not touched
        assert torch.equal(b[k][0]._base, ref[k]), k
    for k in keys:                                                                # nothing written between the views
        mask = torch.ones_like(ref[k], dtype=torch.bool)
        for view in b[k]:
            o = (view.data_ptr() - b[k][0]._base.data_ptr()) // 4
            mask[o:o + view.numel()] = False
        assert int(mask.sum()) > 0 and torch.equal(b[k][0]._base[mask], ref[k][mask]), k
    # ---- behind a guard: coef == 1, then coef < 1, against the unscheduled guarded launch at the mirror's rate
    for seed, half in ((22, False), (23, True)):
        a, b = _lists(seed), _lists(seed)
        norm = float(torch.cat([g.double().reshape(-1) for g in b["g"]]).norm())
        rec = _measure(b["g"], 0.5 * norm if half else 0.0)
        coef = float(rec[1])
        assert float(rec[2]) == 1.0 and (0.49 < coef < 0.51 if half else coef == 1.0)
        _adam(a, rate, t, ema, record=rec)
        _adam(b, LR, t, ema, record=rec, sched=sched)
        _same(a, b, keys)
        assert any(not torch.equal(x, y) for x, y in zip(b["p"], _lists(seed)["p"]))
    # ---- a non-finite gradient: every buffer byte-identical
    b = _lists(24)
    b["g"][6][-1] = float("nan")
    before = _bases(b)
    rec = _measure(b["g"], 1.0)
    assert float(rec[2]) == 0.0
    _adam(b, LR, t, ema, record=rec, sched=sched)
    after = _bases(b)
    for k in "pgmve":
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k


def test_invalid_schedule_arguments_are_refused_before_any_launch():
    from pdgn_amd import _lib
    L = _lib.lib()
    x = _lists(3)
    before = _bases(x)
    step = torch.tensor([3.0], device="cuda")
    sched = _device_table(lm.table(KNOTS4))
    odd = torch.zeros(70, dtype=torch.float32, device="cuda")[1:]                 # 4 bytes past an 8-byte boundary
    n, N, s = len(SIZES), _counts(x["p"]), _lib.stream_of(step)
    P, G, M, V = _arr(x["p"]), _arr(x["g"]), _arr(x["m"]), _arr(x["v"])
    call = lambda sc, lr=LR: L.pdgn_adam_sched_multi(n, P, G, M, V, None, N, lr, B1, B2, EPS, 0.0, _lib.ptr(step), None, sc, s)
    assert call(None) == -1 and call(_lib.ptr(odd)) == -1 and call(_lib.ptr(sched), -1.0) == -1
    out2, out32 = torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(1, device="cuda")
    ev = lambda sc=_lib.ptr(sched), lr=LR, st=_lib.ptr(step), o2=_lib.ptr(out2), o32=_lib.ptr(out32): L.pdgn_lr_eval(sc, lr, st, None, o2, o32, s)
    assert ev(sc=None) == -1 and ev(sc=_lib.ptr(odd)) == -1 and ev(lr=float("nan")) == -1 and ev(st=None) == -1
    assert ev(o2=None) == -1 and ev(o2=_lib.ptr(odd)) == -1 and ev(o32=None) == -1
    torch.cuda.synchronize()
    after = _bases(x)
    assert all(torch.equal(before[k], after[k]) for k in "pgmve") and float(out2.abs().sum()) == 0.0 and float(out32) == 0.0


# ---------------------------------------------------------------------------- 2. pdgn_lr_eval
KNOTS_EVAL = [(2, 0.125), (10, 1.0), (1000, 0.3), (100000, 0.01)]
COUNTS = [1, 2, 9, 10, 11, 999, 1000, 2 ** 24 - 1]


def _eval(sched, lr, step_value, applied=None):
    from pdgn_amd import _lib
    step = torch.tensor([float(step_value)], device="cuda")
    out2 = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    out32 = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    rec = None
    if applied is not None:
        rec = torch.tensor([1.0, 1.0, float(applied), 1.0 - applied, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().pdgn_lr_eval(_lib.ptr(sched), lr, _lib.ptr(step), _lib.ptr(rec) if rec is not None else None, _lib.ptr(out2),
                                       _lib.ptr(out32), _lib.stream_of(step)), "pdgn_lr_eval")
    torch.cuda.synchronize()
    assert float(step) == float(step_value)
    return out2.cpu().numpy(), out32.cpu().numpy()[0]


@pytest.mark.parametrize("how", ["no_guard", "applied", "skipped"])
def test_lr_eval_equals_the_mirror_bit_for_bit(how):
    tab = lm.table(KNOTS_EVAL)
    sched = _device_table(tab)
    lr = 3e-4
    seen = set()
    for t in COUNTS:
        # the update ABOUT to happen is update t: the counter holds t - 1, or t itself behind a record that says "skipped"
        out2, out32 = _eval(sched, lr, t if how == "skipped" else t - 1, {"no_guard": None, "applied": 1.0, "skipped": 0.0}[how])
        f, rate = lm.factor(tab, t), lm.lr_eff(lr, tab, t)
        assert out2[0].view(np.uint64) == np.float64(f).view(np.uint64), (t, out2[0], f)
        assert out2[1].view(np.uint64) == np.float64(rate).view(np.uint64), (t, out2[1], rate)
        assert out32.dtype == np.float32 and out32 == np.float32(out2[1]) == lm.lr32(lr, tab, t)
        seen.add(float(f))
    assert len(seen) == len(COUNTS) - 1 and {0.125, 1.0, 0.3} <= seen              # (t = 1 and 2 share f_0; on a knot exactly f_i)


def test_a_malformed_table_on_the_device_gives_the_first_factor():
    good = lm.table(KNOTS_EVAL)
    for change in ({0: 40.0}, {3: 1.0}, {0: 0.0}, {0: 2.5}, {0: float("nan")}, {7: float("nan")}):     # n = 40; t_1 < t_0; ...
        tab = good.copy()
        for k, v in change.items():
            tab[k] = v
        for t in (1, 500, 10 ** 6):
            out2, out32 = _eval(_device_table(tab), 1.0, t - 1)
            assert out2[0] == 0.125 == lm.factor(tab, t) and out2[1] == 0.125 and out32 == np.float32(0.125), (change, t, out2)
    out2, _ = _eval(_device_table(good), 1.0, 499)
    assert out2[0] != 0.125 and out2[0] == lm.factor(good, 500)


# ---------------------------------------------------------------------------- 3. the routes out of LeanAdamStep.step
def _small_optimizer(seed=4, **kw):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, device="cuda", generator=gen)) for n in (5, 4097, 300)]
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 0.01
    kw = dict(dict(capturable=True, fused=True), **kw)
    return torch.optim.Adam(params, lr=LR, betas=(B1, B2), **kw), params


def test_every_route_applies_the_scheduled_rate():
    from pdgn_amd.trainer import LeanAdamStep
    knots = [(0, 0.2), (10, 0.7)]                                                 # t = 1: 0.25 inside the segment
    tab = lm.table(knots)
    assert abs(float(lm.factor(tab, 1)) - 0.25) < 1e-15
    sched = _device_table(tab)
    opt, params = _small_optimizer()
    twin_opt, twin_params = _small_optimizer()
    lean, twin = LeanAdamStep(opt, sched=sched), LeanAdamStep(twin_opt)
    rates = []

    def both(t, rate):
        before = [p.detach().clone() for p in params]
        twin_opt.param_groups[0]["lr"] = rate
        lean.step(), twin.step()
        torch.cuda.synchronize()
        assert float(opt.state[params[0]]["step"]) == t == float(twin_opt.state[twin_params[0]]["step"])
        assert opt.param_groups[0]["lr"] == LR and isinstance(opt.param_groups[0]["lr"], float)      # the base rate, a Python float
        worst = max(float(((p - q).abs() / (p - b).abs().clamp_min(1e-30)).max()) for p, q, b in zip([x.detach() for x in params], [x.detach() for x in twin_params], before))
        print("update %d at rate %.17g: largest |p - p_twin| / |p - p_old| = %.3g" % (t, rate, worst))
        rates.append(rate)
        return all(torch.equal(p, q) for p, q in zip(params, twin_params)) and all(not torch.equal(p, b) for p, b in zip(params, before))

    # 1: the optimizer's first, ordinary step() -- torch's kernel with the fp32 device scalar in the group for the call
    assert both(1, float(lm.lr32(LR, tab, 1)))
    assert lean.lists and float(lean.lr32) == lm.lr32(LR, tab, 1) and lean.lr_out.cpu().numpy()[1] == lm.lr_eff(LR, tab, 1)
    # 2: the lean route on the own kernel -- the fp64 rate, evaluated inside the launch (no pdgn_lr_eval: lr32 is still update 1's)
    assert both(2, float(lm.lr_eff(LR, tab, 2)))
    assert lean.route == "own" and float(lean.lr32) == lm.lr32(LR, tab, 1)
    # 3: the lean route with the own kernel switched off on the instances -- torch._fused_adam_ with the scalar as its lr
    lean._OWN = twin._OWN = False
    assert both(3, float(lm.lr32(LR, tab, 3)))
    assert float(lean.lr32) == lm.lr32(LR, tab, 3) and lean.lists
    assert len(set(rates)) == 3 and float(lm.lr32(LR, tab, 3)) != float(lm.lr_eff(LR, tab, 3))


def test_an_optimizer_that_cannot_take_a_tensor_rate_raises():
    from pdgn_amd._lib import PdgnHipError
    from pdgn_amd.trainer import LeanAdamStep
    sched = _device_table(lm.table([(0, 0.5)]))
    for kw in (dict(capturable=False, fused=False), dict(capturable=False, fused=True), dict(capturable=True, fused=False, foreach=True)):
        opt, params = _small_optimizer(**kw)
        lean = LeanAdamStep(opt, sched=sched)
        before = [p.detach().clone() for p in params]
        with pytest.raises(PdgnHipError):
            lean.step()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, params)) and opt.param_groups[0]["lr"] == LR
    opt, params = _small_optimizer()
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3, device="cuda"))]})
    with pytest.raises(PdgnHipError):
        LeanAdamStep(opt, sched=sched).step()


# ---------------------------------------------------------------------------- 4.-6. the trainer
B = 2


def _batch(dev):
    from pdgn_amd.trainer import noise, synthetic_batch
    return synthetic_batch(B, dev), noise(B, dev), noise(B, dev)


def _params(tr):
    return [[p.detach().clone() for p in net.parameters()] for net in [tr.G] + tr.D]


def _moved(before, tr):
    return [any(not torch.equal(a, b) for a, b in zip(snap, net.parameters())) for snap, net in zip(before, [tr.G] + tr.D)]


def _held_steps(tr):
    return [int(float(o.state[o.param_groups[0]["params"][0]]["step"])) for o in [tr.optG] + tr.optD]


def _drop_list(tr):
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def frozen():
    """A trainer whose schedule is the factor 0 throughout, with its launch list captured: (trainer, parameters before the capture,
    the list's info)."""
    from pdgn_amd.trainer import PDGNTrainer
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    tr = PDGNTrainer(device=dev, distributed=False, lr_schedule=[(0, 0.0)])
    tr.train()
    before = _params(tr)
    tr.capture_list(*_batch(dev))
    torch.cuda.synchronize()
    yield tr, before, tr._list.info
    _drop_list(tr)


def test_the_launch_list_reads_the_table_not_a_baked_value(frozen):
    tr, before, _info = frozen
    assert tr.lr_table is not None and tr.lr_table.dtype == torch.float64 and tr.lr_table.numel() == 33
    assert all(s.sched is tr.lr_table for s in [tr._stepG] + tr._stepD)
    captured = tr._list
    tr.step_list()
    torch.cuda.synchronize()
    moment = [o.state[o.param_groups[0]["params"][0]]["exp_avg"].clone() for o in [tr.optG] + tr.optD]
    steps1 = _held_steps(tr)
    tr.step_list()
    torch.cuda.synchronize()
    # the warm-up iterations of the capture and both replays were real updates -- at the factor 0: no parameter of any network moved
    assert _moved(before, tr) == [False] * 5
    steps2 = _held_steps(tr)
    assert steps2 == [s + 1 for s in steps1] and min(steps1) >= 3                 # (two warm-up iterations, then the replay)
    assert all(not torch.equal(m, o.state[o.param_groups[0]["params"][0]]["exp_avg"]) and float(m.abs().max()) > 0
               for m, o in zip(moment, [tr.optG] + tr.optD))
    state = tr.lr_state()
    assert [state[k]["step"] for k in NETS] == steps2 and all(state[k]["factor"] == 0.0 and state[k]["lr"] == 0.0 for k in NETS)
    # the same table, overwritten in place; the same list, not captured again
    where = tr.lr_table.data_ptr()
    tr.set_lr_schedule([(0, 1.0)])
    assert tr.lr_table.data_ptr() == where and tr._list is captured
    tr.step_list()
    torch.cuda.synchronize()
    assert _moved(before, tr) == [True] * 5 and tr._list is captured
    state = tr.lr_state()
    assert [state[k]["step"] for k in NETS] == [s + 1 for s in steps2] == _held_steps(tr)
    assert all(state[k]["factor"] == 1.0 and state[k]["lr"] == 1e-4 for k in NETS)
    with pytest.raises(ValueError):
        tr.set_lr_schedule([(0, 1.0), (0, 0.5)])
    assert tr.lr_table.cpu().tolist() == [1.0, 0.0, 1.0] + [0.0] * 30             # a refused schedule leaves the table alone


def test_per_network_rates_and_no_table_without_a_schedule(frozen):
    from pdgn_amd.trainer import PDGNTrainer
    _tr, _before, scheduled_info = frozen
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    tr = PDGNTrainer(device=dev, distributed=False, lr_g=0.0, lr_d=1e-4)
    tr.train()
    assert tr.lr_table is None and all(s.sched is None for s in [tr._stepG] + tr._stepD)
    assert tr.optG.param_groups[0]["lr"] == 0.0 and all(o.param_groups[0]["lr"] == 1e-4 for o in tr.optD)
    before = _params(tr)
    batch = _batch(dev)
    tr.step(*batch), tr.step(*batch)                                              # torch's route, then the own kernel
    torch.cuda.synchronize()
    assert _moved(before, tr) == [False, True, True, True, True]
    state = tr.lr_state()
    assert state["G"] == {"step": 2, "factor": 1.0, "lr": 0.0} and state["D3"] == {"step": 2, "factor": 1.0, "lr": 1e-4}
    with pytest.raises(RuntimeError):
        tr.set_lr_schedule([(0, 1.0)])
    # neither a schedule nor per-network rates: no table, and the list of a scheduled twin has the same nodes
    torch.manual_seed(7)
    plain = PDGNTrainer(device=dev, distributed=False)
    plain.train()
    assert plain.lr_table is None and plain.per_network_lr is False and all(s.sched is None for s in [plain._stepG] + plain._stepD)
    plain.capture_list(*batch)
    torch.cuda.synchronize()
    try:
        print("launch lists: unscheduled %s | scheduled %s" % (plain._list.info, scheduled_info))
        assert plain._list.info == scheduled_info
    finally:
        _drop_list(plain)


def test_a_resumed_run_continues_the_schedule(tmp_path):
    from pdgn_amd.trainer import PDGNTrainer
    dev = torch.device("cuda:0")
    knots = [(0, 0.0), (4, 1.0), (100, 0.5)]
    torch.manual_seed(8)
    tr = PDGNTrainer(device=dev, distributed=False, lr_g=5e-5, lr_schedule=knots)
    tr.train()
    batch = _batch(dev)
    for _ in range(3):
        tr.step(*batch)
    state = tr.lr_state()
    assert state["G"] == {"step": 3, "factor": 0.75, "lr": 5e-5 * 0.75} and state["D1"] == {"step": 3, "factor": 0.75, "lr": 1e-4 * 0.75}
    files = tr.save(str(tmp_path), 1)
    ck = torch.load(files[0], map_location="cpu")
    assert ck["G_optimizer"]["param_groups"][0]["lr"] == 5e-5                     # the base rate, a float; no table in the file
    assert sorted(ck) == ["G_epoch", "G_model", "G_optimizer"]
    assert torch.load(files[1], map_location="cpu")["D_optimizer2"]["param_groups"][0]["lr"] == 1e-4
    torch.manual_seed(9)
    fresh = PDGNTrainer(device=dev, distributed=False, lr_g=5e-5, lr_schedule=knots)
    fresh.train()
    assert fresh.lr_state()["G"] == {"step": 0, "factor": 0.0, "lr": 0.0}
    fresh.load(files[0], files[1])
    assert fresh.lr_state() == state
    before = _params(fresh)
    fresh.step(*batch)                                                            # update 4, at the full rate: the counter was restored
    assert fresh.lr_state()["G"] == {"step": 4, "factor": 1.0, "lr": 5e-5} and _moved(before, fresh) == [True] * 5
