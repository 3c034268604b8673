"""The gradient guard: pdgn_gradnorm_multi's record against an fp64 norm and the host mirror
(tests/gradguard_mirror.py), the guarded Adam launches against the unguarded ones (identity, clipping, skip), LeanAdamStep's routes
(own kernel here, torch's in a child process), the trainer's eager step and launch list with poisoned gradients, and `fit`."""
import csv
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gradguard_mirror as gm
import gradguard_worker as gw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, EPS, DECAY = 1e-4, 0.5, 0.999, 1e-8, 0.999
SIZES = gw.SIZES
OFFSET = {"p": {5: 1, 7: 3}, "g": {8: 1, 3: 2}, "m": {}, "v": {9: 2}, "e": {6: 1, 7: 3}}      # floats past a 16-byte boundary: 4-byte aligned only
INVALID = -1


def _lists(seed, sizes=SIZES):
    """{name: [tensor per size]} for p, g, m, v, e: views of one buffer each, on 16-byte boundaries except those of OFFSET; the
    gradients with one magnitude per tensor, 1e-4 .. 1e2."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    mags = gw.magnitudes()
    out = {}
    for name in "pgmve":
        slot = lambda n: (n + 3) // 4 * 4 + 4
        buf = torch.randn(sum(slot(n) for n in sizes), device="cuda", generator=gen)
        if name == "v":
            buf = buf.abs() * 1e-4
        if name == "m":
            buf *= 0.01
        views, off = [], 0
        for i, n in enumerate(sizes):
            o = off + OFFSET[name].get(i, 0)
            views.append(buf[o:o + n])
            if name == "g":
                views[-1] *= mags[i % len(mags)]
            off += slot(n)
        out[name] = views
    return out


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _counts(ts):
    return (ctypes.c_longlong * len(ts))(*[t.numel() for t in ts])


class Guard:
    """A record and a workspace for one list, and the call."""

    def __init__(self, grads):
        from pdgn_amd import _lib
        self.L, self._lib = _lib.lib(), _lib
        self.n, self.counts = len(grads), _counts(grads)
        need = self.L.pdgn_gradnorm_workspace_doubles(self.n, self.counts)
        assert need == sum((g.numel() + 4095) // 4096 for g in grads)
        self.ws = torch.full((need,), float("nan"), dtype=torch.float64, device="cuda")
        self.rec = torch.zeros(8, dtype=torch.float32, device="cuda")

    def __call__(self, grads, max_norm=0.0):
        lib = self._lib
        lib.check(self.L.pdgn_gradnorm_multi(self.n, _arr(grads), self.counts, max_norm, lib.ptr(self.ws), self.ws.numel(), lib.ptr(self.rec),
                                             lib.stream_of(self.rec)), "pdgn_gradnorm_multi")
        torch.cuda.synchronize()
        host = self.rec.cpu()
        ints = host.view(torch.int32)
        return {"norm": host[0].numpy()[()], "coef": host[1].numpy()[()], "applied": float(host[2]), "found_inf": float(host[3]),
                "n_applied": int(ints[4]), "n_skipped": int(ints[5]), "bits": host.clone()}


def _norm64(grads):
    return torch.cat([g.double().reshape(-1) for g in grads]).norm().cpu().numpy()[()]


# ---------------------------------------------------------------------------- 1. the norm and the record
def test_norm_is_the_fp64_norm_and_repeats_bit_for_bit():
    g = _lists(5)["g"]
    assert any(x.data_ptr() % 16 for x in g)
    for grads in (g, g + [x.clone() for x in g]):                                # 89 tensors: one launch; 178: two
        guard = Guard(grads)
        want64 = _norm64(grads)
        first = guard(grads)
        second = guard(grads)
        print("%d tensors: norm %.9g, fp64 %.17g, %d ulp" % (len(grads), first["norm"], want64, gm.ulps(first["norm"], np.float32(want64))))
        assert gm.ulps(first["norm"], np.float32(want64)) <= 2
        assert first["coef"] == 1.0 and first["applied"] == 1.0 and first["found_inf"] == 0.0
        assert torch.equal(first["bits"][:4], second["bits"][:4])                # two runs on the same bytes: the same bits
        assert (first["n_applied"], first["n_skipped"], second["n_applied"], second["n_skipped"]) == (1, 0, 2, 0)
        assert gm.ulps(first["norm"], gm.record(gm.total_of([x.cpu().numpy() for x in grads]), 0.0)["norm"]) <= 2
        # the clip factor: below the norm, above it, and the two spellings of "no clipping"
        for max_norm in (0.5 * float(want64), 0.01, 2.0 * float(want64)):
            got = guard(grads, max_norm)
            want = np.float32(min(1.0, max_norm / (want64 + 1e-6)))
            assert gm.ulps(got["coef"], want) <= 2 and got["applied"] == 1.0, (max_norm, got["coef"], want)
            assert (got["coef"] < 1.0) == (max_norm < want64)
        for max_norm in (0.0, -1.0, float("inf")):
            assert guard(grads, max_norm)["coef"] == 1.0


def test_huge_and_tiny_entries_are_squared_in_fp64():
    sizes = [5, 4097, 3, 4096]
    grads = [torch.full((n,), v, device="cuda") for n, v in zip(sizes, (1e30, 1e-30, -2e30, 1e-30))]
    guard = Guard(grads)
    got = guard(grads, 1.0)
    want64 = np.sqrt(np.float64(5) * np.float64(np.float32(1e30)) ** 2 + np.float64(3) * np.float64(np.float32(2e30)) ** 2
                     + np.float64(8193) * np.float64(np.float32(1e-30)) ** 2)
    assert got["applied"] == 1.0 and np.isfinite(got["norm"]) and gm.ulps(got["norm"], np.float32(want64)) <= 2
    assert gm.ulps(got["coef"], np.float32(1.0 / (want64 + 1e-6))) <= 2
    tiny = [torch.full((n,), 1e-30, device="cuda") for n in (4097, 1)]           # fp32 squares would all be zero
    got = Guard(tiny)(tiny)
    assert gm.ulps(got["norm"], np.float32(np.sqrt(np.float64(4098)) * np.float64(np.float32(1e-30)))) <= 2 and got["norm"] > 0


# ---------------------------------------------------------------------------- 2. non-finite
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("where", [gw.I_4097, gw.I_1])
def test_one_non_finite_element_is_seen(value, where):
    g = _lists(6)["g"]
    guard = Guard(g)
    assert guard(g, 1.0)["applied"] == 1.0
    g[where][-1] = value                                                         # the last element of the 4097 tensor / the 1-element tensor
    for k in (1, 2):
        got = guard(g, 1.0)
        assert got["applied"] == 0.0 and got["found_inf"] == 1.0 and got["coef"] == 1.0 and not np.isfinite(got["norm"])
        assert (got["n_applied"], got["n_skipped"]) == (1, k)
    want = gm.record(gm.total_of([x.cpu().numpy() for x in g]), 1.0)
    assert want["applied"] == 0.0 and want["coef"] == 1.0


def test_invalid_arguments_are_refused_before_any_launch():
    from pdgn_amd import _lib
    L = _lib.lib()
    x = _lists(3)
    g = x["g"]
    guard = Guard(g)
    n, G, N, ws, rec, stream = len(g), _arr(g), _counts(g), guard.ws, guard.rec, _lib.stream_of(guard.rec)
    keep = [t.clone() for k in "pmve" for t in x[k]]
    bad_counts = _counts(g)
    bad_counts[80] = 0
    hole = _arr(g)
    hole[3] = None
    odd = _arr(g)
    odd[4] = g[4].data_ptr() + 2

    def norm(n=n, G=G, N=N, max_norm=1.0, ws=_lib.ptr(ws), size=ws.numel(), rec=_lib.ptr(rec)):
        return L.pdgn_gradnorm_multi(n, G, N, max_norm, ws, size, rec, stream)

    null = ctypes.c_void_p(0)
    assert L.pdgn_gradnorm_workspace_doubles(0, N) == -1 and L.pdgn_gradnorm_workspace_doubles(n, bad_counts) == -1
    assert L.pdgn_gradnorm_workspace_doubles(n, None) == -1
    for rc in (norm(n=0), norm(G=None), norm(N=None), norm(N=bad_counts), norm(G=hole), norm(G=odd), norm(max_norm=float("nan")),
               norm(ws=null), norm(ws=ctypes.c_void_p(ws.data_ptr() + 4)), norm(size=ws.numel() - 1), norm(rec=null),
               norm(rec=ctypes.c_void_p(rec.data_ptr() + 2))):
        assert rc == INVALID
    step = torch.tensor([3.0], device="cuda")
    P, M, V, E = _arr(x["p"]), _arr(x["m"]), _arr(x["v"]), _arr(x["e"])
    for record in (null, ctypes.c_void_p(rec.data_ptr() + 1)):
        assert L.pdgn_adam_guard_multi(n, P, G, M, V, N, LR, B1, B2, EPS, _lib.ptr(step), record, stream) == INVALID
        assert L.pdgn_adam_ema_guard_multi(n, P, G, M, V, E, N, LR, B1, B2, EPS, DECAY, _lib.ptr(step), record, stream) == INVALID
        assert L.pdgn_ema_guard_multi(n, E, P, N, DECAY, _lib.ptr(step), record, stream) == INVALID
    assert L.pdgn_adam_guard_multi(n, P, G, M, V, bad_counts, LR, B1, B2, EPS, _lib.ptr(step), _lib.ptr(rec), stream) == INVALID
    assert L.pdgn_adam_ema_guard_multi(n, P, G, M, V, E, N, LR, B1, B2, EPS, 1.0, _lib.ptr(step), _lib.ptr(rec), stream) == INVALID
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, [t for k in "pmve" for t in x[k]]))       # nothing ran
    assert not rec.any().item() and torch.isnan(ws).all().item()


# ---------------------------------------------------------------------------- 3.-5. the guarded Adam launches
def _adam(x, ema, record=None, step=7.0, g=None):
    from pdgn_amd import _lib
    L = _lib.lib()
    t = torch.tensor([step], device="cuda")
    n, N, s = len(x["p"]), _counts(x["p"]), _lib.stream_of(t)
    P, G, M, V, E = _arr(x["p"]), _arr(g if g is not None else x["g"]), _arr(x["m"]), _arr(x["v"]), _arr(x["e"])
    if record is None:
        rc = (L.pdgn_adam_ema_multi(n, P, G, M, V, E, N, LR, B1, B2, EPS, DECAY, _lib.ptr(t), s) if ema else
              L.pdgn_adam_multi(n, P, G, M, V, N, LR, B1, B2, EPS, _lib.ptr(t), s))
    else:
        rc = (L.pdgn_adam_ema_guard_multi(n, P, G, M, V, E, N, LR, B1, B2, EPS, DECAY, _lib.ptr(t), _lib.ptr(record), s) if ema else
              L.pdgn_adam_guard_multi(n, P, G, M, V, N, LR, B1, B2, EPS, _lib.ptr(t), _lib.ptr(record), s))
    _lib.check(rc, "adam")
    torch.cuda.synchronize()


def _same(a, b, keys):
    for k in keys:
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), (k, i, SIZES[i])


def _bases(x, keys="pgmve"):
    return {k: x[k][0]._base.clone() for k in keys}


@pytest.mark.parametrize("ema", [False, True])
def test_guarded_adam_identity_clipping_and_skip(ema):
    keys = "pmve" if ema else "pmv"
    # ---- 3. coef == 1, applied == 1: the unguarded launch's bytes
    a, b = _lists(11), _lists(11)
    guard = Guard(b["g"])
    rec = guard(b["g"])
    assert rec["coef"] == 1.0 and rec["applied"] == 1.0
    p0 = [p.clone() for p in a["p"]]
    _adam(a, ema)
    _adam(b, ema, guard.rec)
    assert any(not torch.equal(x, y) for x, y in zip(a["p"], p0))
    _same(a, b, keys)
    # ---- 4. max_norm at half the norm: the unguarded launch on g * coef (formed by torch in fp32), and g is not written
    a, b = _lists(12), _lists(12)
    g_before = _bases(b, "g")["g"]
    rec = guard(b["g"], 0.5 * float(_norm64(b["g"])))
    assert 0.49 < rec["coef"] < 0.51
    coef = guard.rec[1]                                                          # read back from the record, on the device
    scaled = [g * coef for g in a["g"]]
    assert all(s.dtype == torch.float32 for s in scaled)
    _adam(a, ema, g=scaled)
    _adam(b, ema, guard.rec)
    _same(a, b, keys)
    assert torch.equal(b["g"][0]._base, g_before)
    c = _lists(12)
    _adam(c, ema)
    assert any(not torch.equal(x, y) for x, y in zip(c["m"], b["m"]))            # (the factor did something)
    # ---- 5. applied == 0: nothing is touched (the gaps between the views included)
    b = _lists(13)
    b["g"][gw.I_4097][-1] = float("nan")
    before = _bases(b)
    assert guard(b["g"], 1.0)["applied"] == 0.0
    _adam(b, ema, guard.rec)
    if ema:
        from pdgn_amd import _lib
        t = torch.tensor([7.0], device="cuda")
        _lib.check(_lib.lib().pdgn_ema_guard_multi(len(SIZES), _arr(b["e"]), _arr(b["p"]), _counts(b["p"]), DECAY, _lib.ptr(t),
                                                   _lib.ptr(guard.rec), _lib.stream_of(t)), "pdgn_ema_guard_multi")
        torch.cuda.synchronize()
    after = _bases(b)
    for k in "pgmve":
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k
    if ema:                                                                      # ... and applied, the guarded average alone is the plain one
        b, c = _lists(14), _lists(14)
        from pdgn_amd import _lib
        t = torch.tensor([7.0], device="cuda")
        assert guard(b["g"])["applied"] == 1.0
        _lib.check(_lib.lib().pdgn_ema_guard_multi(len(SIZES), _arr(b["e"]), _arr(b["p"]), _counts(b["p"]), DECAY, _lib.ptr(t),
                                                   _lib.ptr(guard.rec), _lib.stream_of(t)), "pdgn_ema_guard_multi")
        _lib.check(_lib.lib().pdgn_ema_multi(len(SIZES), _arr(c["e"]), _arr(c["p"]), _counts(c["p"]), DECAY, _lib.ptr(t), _lib.stream_of(t)),
                   "pdgn_ema_multi")
        torch.cuda.synchronize()
        _same(b, c, "e")
        assert any(not torch.equal(x, y) for x, y in zip(b["e"], _lists(14)["e"]))


# ---------------------------------------------------------------------------- 6. LeanAdamStep
@pytest.mark.parametrize("poison_at", [3, 1])                                    # 1: the optimizer's first, ordinary step() -- torch's route
def test_lean_adam_step_skips_the_poisoned_update(poison_at):
    assert gw.lean_scenario(poison_at=poison_at) == 4


def test_lean_adam_step_with_torchs_optimizer_kernel_in_a_child_process():
    env = dict(os.environ, PDGN_OWN_ADAM="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gradguard_worker.py")], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0 and run.stdout.count("gradguard worker ok: PDGN_OWN_ADAM=0") == 2, run.stdout[-2000:] + run.stderr[-3000:]


def test_an_optimizer_that_cannot_take_the_flag_raises():
    from pdgn_amd._lib import PdgnHipError
    from pdgn_amd.trainer import GradGuard, LeanAdamStep
    params = [torch.nn.Parameter(torch.randn(n, device="cuda")) for n in (5, 4097)]
    opt = torch.optim.Adam(params, lr=1e-4)                                      # neither fused nor capturable
    lean = LeanAdamStep(opt, guard=GradGuard(params))
    before = [p.detach().clone() for p in params]
    for p in params:
        p.grad = torch.randn_like(p)
    with pytest.raises(PdgnHipError):
        lean.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, params))


# ---------------------------------------------------------------------------- 7. the trainer
def _train_state(tr):
    """Every parameter, moment, step counter and the average (NOT the BatchNorm buffers: the forward pass writes them before any
    gradient exists)."""
    ts = []
    for net in [tr.G] + tr.D:
        ts += list(net.parameters())
    for opt in [tr.optG] + tr.optD:
        for st in opt.state.values():
            ts += [v for v in st.values() if torch.is_tensor(v)]
    return ts + ([tr.ema_buf] if tr.ema_buf is not None else [])


def _drop_list(tr):
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def _poisonable(tr):
    """A tensor hook on one parameter of each network that multiplies its gradient by a device scalar: 1.0 (exact) or NaN.  Gradient
    side only: no non-finite value ever enters a forward pass.  Registered before any capture: the multiplication is part of the list."""
    scalar = torch.ones((), device=tr.device)
    for net in [tr.G] + tr.D:
        list(net.parameters())[-1].register_hook(lambda g, s=scalar: g * s)
    return scalar


def _close(a, b):
    for k in a:
        x, y = float(a[k]), float(b[k])
        print("%-13s guard off %.9g  on %.9g  diff %.3g" % (k, x, y, abs(x - y)))
    return all(abs(float(a[k]) - float(b[k])) <= 1e-5 * max(1.0, abs(float(a[k]))) for k in a)


def test_trainer_eager_and_list_skip_poisoned_iterations():
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    dev = torch.device("cuda:0")
    B = 4
    reals, z1, z2 = synthetic_batch(B, dev), noise(B, dev), noise(B, dev)
    torch.manual_seed(2)
    off = PDGNTrainer(device=dev, distributed=False, ema_decay=DECAY)
    torch.manual_seed(2)
    on = PDGNTrainer(device=dev, distributed=False, ema_decay=DECAY, grad_guard=True)
    off.train(), on.train()
    assert off.guards is None and off.guard_buf is None and off._stepG.guard is None and on.clip_grad_norm is None
    with pytest.raises(RuntimeError):
        off.guard_state()
    assert all(torch.equal(a, b) for a, b in zip(_train_state(off), _train_state(on)))
    scalar = _poisonable(on)                                                     # before any capture
    seeded_tensors = [t for net in [on.G] + on.D for t in list(net.parameters()) + list(net.buffers())] + [on.ema_buf]
    seeded = [t.detach().clone() for t in seeded_tensors]
    keys = PDGNTrainer.GUARD_KEYS

    def counters():
        s = on.guard_state()
        assert list(s) == list(keys) and all(set(v) == {"norm", "coef", "applied", "skipped"} for v in s.values())
        return [s[k]["applied"] for k in keys], [s[k]["skipped"] for k in keys], s

    def poisoned_then_clean(issue, label):
        a0, s0, _ = counters()
        before = [t.detach().clone() for t in _train_state(on)]
        scalar.fill_(float("nan"))
        issue()
        a1, s1, st = counters()
        assert s1 == [s + 1 for s in s0] and a1 == a0, (label, a0, a1, s0, s1)
        assert all(not np.isfinite(st[k]["norm"]) for k in keys)
        after = _train_state(on)
        assert len(after) == len(before)
        for i, (x, y) in enumerate(zip(before, after)):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (label, i)
        scalar.fill_(1.0)
        out = issue()
        a2, s2, st = counters()
        assert a2 == [a + 1 for a in a1] and s2 == s1 and all(np.isfinite(st[k]["norm"]) and st[k]["norm"] > 0 for k in keys), label
        assert all(torch.isfinite(v).item() for v in out.values())
        assert any(not torch.equal(x, y) for x, y in zip(before, _train_state(on)))

    # ---- eager: one iteration from the seeded state, guard off against on
    a = {k: v.clone() for k, v in off.step(reals, z1, z2).items()}
    b = {k: v.clone() for k, v in on.step(reals, z1, z2).items()}
    torch.cuda.synchronize()
    assert _close(a, b)
    applied, skipped, st = counters()
    assert applied == [1] * 5 and skipped == [0] * 5 and all(st[k]["coef"] == 1.0 and st[k]["norm"] > 0 for k in keys)
    poisoned_then_clean(lambda: on.step(reals, z1, z2), "eager")
    # ---- the launch list: the same iteration from the same seeded state (capture_list's warm-up iterations are real updates, so
    # the seeded values are put back by value behind the capture: parameters, buffers, the average; Adam's state as it starts, zero)
    on.capture_list(reals, z1, z2)
    torch.cuda.synchronize()
    a_before, s_before, _ = counters()
    with torch.no_grad():
        for t, v in zip(seeded_tensors, seeded):
            t.copy_(v)
        for opt in [on.optG] + on.optD:
            for st in opt.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
    b = {k: v.clone() for k, v in on.step_list(None, z1, z2).items()}
    torch.cuda.synchronize()
    assert _close(a, b)
    applied, skipped, _ = counters()
    assert applied == [x + 1 for x in a_before] and skipped == s_before == [1] * 5
    assert all(float(st["step"]) == 1.0 for opt in [on.optG] + on.optD for st in opt.state.values())
    poisoned_then_clean(lambda: on.step_list(None, z1, z2), "list")
    assert torch.isfinite(on.ema_buf).all().item()
    _drop_list(on)


# ---------------------------------------------------------------------------- 8. fit
def test_fit_writes_the_norms_and_stops_after_consecutive_skips(tmp_path):
    from pdgn_amd.data import BatchFeeder
    from pdgn_amd.trainer import GradGuardError, PDGNTrainer
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    c = torch.randn(12, 2048, 3, generator=g)
    clouds = ((c - c.mean(dim=1, keepdim=True)) / c.reshape(12, -1).std(dim=1).view(12, 1, 1)).to(dev).contiguous()
    feeder = BatchFeeder(clouds, 4, (256, 512, 1024), seed=3)
    nb = feeder.batches_per_epoch
    torch.manual_seed(2)
    tr = PDGNTrainer(device=dev, distributed=False, ema_decay=DECAY, clip_grad_norm=5.0)
    tr.train()
    assert tr.grad_guard and tr.guards[0].max_norm == 5.0
    scalar = _poisonable(tr)
    lines = []
    log = tmp_path / "log.txt"
    assert tr.fit(feeder, 2, log=str(log), issue="list") == 2
    with open(tmp_path / "grad_norms.csv") as f:
        table = list(csv.reader(f))
    assert table[0][:2] == ["epoch", "iter"] and table[0][-1] == "skipped_total" and len(table[0]) == 13
    assert len(table) == 1 + 2 * nb and len(log.read_text().splitlines()) == 2 * nb
    assert [(int(r[0]), int(r[1])) for r in table[1:]] == [(e, i) for e in (1, 2) for i in range(1, nb + 1)]
    vals = np.array([[float(v) for v in r[2:12]] for r in table[1:]])
    assert np.isfinite(vals).all() and (vals[:, 0::2] > 0).all() and (vals[:, 1::2] <= 1.0).all() and (vals[:, 1::2] > 0).all()
    assert all(int(r[-1]) == 0 for r in table[1:])
    assert log.read_text().splitlines()[0].startswith("Epoch: [ 1] [   1/%4d] time:" % nb)          # the reference's line, as it was
    # ---- the poison held on: three iterations, a checkpoint of finite values, and the error
    scalar.fill_(float("nan"))
    before = [t.detach().clone() for t in _train_state(tr)]
    ck = tmp_path / "ck"
    os.makedirs(ck)
    with pytest.raises(GradGuardError):
        tr.fit(feeder, 9, start_epoch=3, checkpoint_dir=str(ck), log=lines.append, issue="list", guard_max_skips=3,
               grad_norms=str(tmp_path / "poisoned.csv"))
    torch.cuda.synchronize()
    assert len(lines) == 3
    with open(tmp_path / "poisoned.csv") as f:
        rows = list(csv.reader(f))[1:]
    assert len(rows) == 3 and [int(r[-1]) for r in rows] == [5, 10, 15]
    assert all(torch.equal(x, y) for x, y in zip(before, _train_state(tr)))
    assert sorted(os.listdir(ck)) == ["3_chair_D.pth", "3_chair_G.pth", "3_chair_G_ema.pth"]
    scalar.fill_(1.0)
    torch.manual_seed(7)
    other = PDGNTrainer(device=dev, distributed=False, ema_decay=DECAY)
    assert other.load(str(ck / "3_chair_G.pth"), str(ck / "3_chair_D.pth")) == 3
    for name in sorted(os.listdir(ck)):
        def walk(v):
            if torch.is_tensor(v):
                assert not v.is_floating_point() or torch.isfinite(v).all().item(), name
            elif isinstance(v, dict):
                for w in v.values():
                    walk(w)
            elif isinstance(v, (list, tuple)):
                for w in v:
                    walk(w)
        walk(torch.load(ck / name))
    assert all(torch.equal(a, b) for a, b in zip(other.G.parameters(), tr.G.parameters()))
    _drop_list(tr)
