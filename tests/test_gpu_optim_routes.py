"""LeanAdamStep's dispatch against the C ABI it dispatches to (DESIGN.md sections 7d-7f): in every cell of {average} x {guard} x
{schedule} x {own kernel on / off} four steps of a LeanAdamStep and of a twin optimizer driven by the documented sequence, written
out below with direct calls, must leave the same bits; `route` names the path each step took; and a launch the library refuses
leaves the optimizer's state as it was."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
LR, B1, B2, EPS, DECAY = 1e-4, 0.5, 0.999, 1e-8, 0.999
# 75 tensors: more than one Adam launch carries (72 without averages, 64 with them), sizes on both sides of the 4096-element chunk
SIZES = [1, 5, 4095, 4096, 4097] + [17 + 13 * i for i in range(70)]
I_4097 = SIZES.index(4097)
KNOTS = [(0, 0.2), (10, 0.7)]                                    # every step's rate differs, and the fp64 and fp32 routes differ in bits
STEPS = 4
CELLS = list(itertools.product([False, True], repeat=4))         # (ema, guard, sched, own)
CELL_IDS = ["-".join(n if on else "no" + n for n, on in zip(("ema", "guard", "sched", "own"), c)) for c in CELLS]


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _counts(ts):
    return (ctypes.c_longlong * len(ts))(*[t.numel() for t in ts])


def _bits(ts):
    return torch.cat([t.detach().reshape(-1).view(torch.int32) for t in ts])


def _gradients(t, poisoned=False):
    """Step t's gradients: fixed by the seed, one NaN in the 4097-element tensor's where asked."""
    gen = torch.Generator(device="cuda").manual_seed(100 + t)
    grads = [torch.randn(n, device="cuda", generator=gen) * 0.01 for n in SIZES]
    if poisoned:
        grads[I_4097][-1] = float("nan")
    return grads


def _optimizer(ema):
    gen = torch.Generator(device="cuda").manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(n, device="cuda", generator=gen)) for n in SIZES]
    opt = torch.optim.Adam(params, lr=LR, betas=(B1, B2), capturable=True, fused=True)
    return params, opt, ([p.detach().clone() for p in params] if ema else None)


class Twin:
    """The documented sequence, by direct calls: what LeanAdamStep.step() must be equal to, bit for bit."""

    def __init__(self, ema, guard, sched, own, max_norm):
        from pdgn_amd import _lib, schedule
        self.L, self._lib = _lib.lib(), _lib
        self.params, self.opt, self.ema = _optimizer(ema)
        self.own, self.max_norm = own, max_norm
        self.n, self.N = len(SIZES), _counts(self.params)
        self.rec = self.ws = self.sched = None
        if guard:
            self.rec = torch.zeros(8, dtype=torch.float32, device="cuda")
            self.ws = torch.zeros(self.L.pdgn_gradnorm_workspace_doubles(self.n, self.N), dtype=torch.float64, device="cuda")
        if sched:
            self.sched = schedule.table(KNOTS, torch.device("cuda"))
            self.lr_out = torch.zeros(2, dtype=torch.float64, device="cuda")
            self.lr32 = torch.zeros((), dtype=torch.float32, device="cuda")
        self.t = 0

    def _ptr(self, t):
        return self._lib.ptr(t) if t is not None else None

    def _measure(self, grads):
        if self.rec is not None:
            self._lib.check(self.L.pdgn_gradnorm_multi(self.n, _arr(grads), self.N, self.max_norm, self._lib.ptr(self.ws), self.ws.numel(),
                                                       self._lib.ptr(self.rec), self._lib.stream_of(self.rec)), "pdgn_gradnorm_multi")

    def _eval_lr(self, step):
        self._lib.check(self.L.pdgn_lr_eval(self._lib.ptr(self.sched), LR, self._lib.ptr(step), self._ptr(self.rec), self._lib.ptr(self.lr_out),
                                            self._lib.ptr(self.lr32), self._lib.stream_of(step)), "pdgn_lr_eval")
        return self.lr32

    def _average(self, step):
        if self.ema is None:
            return
        E, P, s = _arr(self.ema), _arr(self.params), self._lib.stream_of(step)
        if self.rec is not None:
            self._lib.check(self.L.pdgn_ema_guard_multi(self.n, E, P, self.N, DECAY, self._lib.ptr(step), self._lib.ptr(self.rec), s), "ema_guard")
        else:
            self._lib.check(self.L.pdgn_ema_multi(self.n, E, P, self.N, DECAY, self._lib.ptr(step), s), "ema")

    def step(self, grads):
        self.t += 1
        for p, g in zip(self.params, grads):
            p.grad = g
        if self.t == 1:
            self._first(grads)
        elif self.own:
            self._own(grads)
        else:
            self._torch(grads)

    def _first(self, grads):
        """The optimizer's first, ordinary step: `found_inf` and the tensor rate in the group for the call."""
        opt, group = self.opt, self.opt.param_groups[0]
        self._measure(grads)
        if self.rec is not None:
            with torch.no_grad():
                torch._foreach_mul_(grads, self.rec[1])
            opt.grad_scale, opt.found_inf = None, self.rec[3]
        if self.sched is not None:
            group["lr"] = self._eval_lr(torch.zeros(1, dtype=torch.float32, device="cuda"))        # (no counter yet: zero)
        opt.step()
        group["lr"] = LR
        if self.rec is not None:
            opt.grad_scale = opt.found_inf = None
        self._average(opt.state[self.params[0]]["step"])

    def _lists(self):
        st, ps = self.opt.state, self.params
        return [st[p]["exp_avg"] for p in ps], [st[p]["exp_avg_sq"] for p in ps], [st[p]["step"] for p in ps]

    def _advance(self, steps):
        with torch.no_grad():
            torch._foreach_add_(steps, 1 if self.rec is None else [self.rec[2]] * len(steps))

    def _own(self, grads):
        """Norm launches, counters, then the ONE entry point include/pdgn_hip.h names for the combination."""
        L, ptr = self.L, self._lib.ptr
        m, v, steps = self._lists()
        self._measure(grads)
        self._advance(steps)
        P, G, M, V, s = _arr(self.params), _arr(grads), _arr(m), _arr(v), self._lib.stream_of(steps[0])
        E = _arr(self.ema) if self.ema is not None else None
        decay = DECAY if self.ema is not None else 0.0
        if self.sched is not None:
            rc = L.pdgn_adam_sched_multi(self.n, P, G, M, V, E, self.N, LR, B1, B2, EPS, decay, ptr(steps[0]), self._ptr(self.rec),
                                         ptr(self.sched), s)
        elif self.ema is not None and self.rec is not None:
            rc = L.pdgn_adam_ema_guard_multi(self.n, P, G, M, V, E, self.N, LR, B1, B2, EPS, DECAY, ptr(steps[0]), ptr(self.rec), s)
        elif self.ema is not None:
            rc = L.pdgn_adam_ema_multi(self.n, P, G, M, V, E, self.N, LR, B1, B2, EPS, DECAY, ptr(steps[0]), s)
        elif self.rec is not None:
            rc = L.pdgn_adam_guard_multi(self.n, P, G, M, V, self.N, LR, B1, B2, EPS, ptr(steps[0]), ptr(self.rec), s)
        else:
            rc = L.pdgn_adam_multi(self.n, P, G, M, V, self.N, LR, B1, B2, EPS, ptr(steps[0]), s)
        self._lib.check(rc, "pdgn_adam*")

    def _torch(self, grads):
        """Norm launches, the rate from the counter before its increment, counters, gradients scaled by coef, torch's fused kernel
        with the flag as `found_inf`, the stand-alone average."""
        m, v, steps = self._lists()
        self._measure(grads)
        lr = self._eval_lr(steps[0]) if self.sched is not None else LR
        self._advance(steps)
        with torch.no_grad():
            if self.rec is not None:
                torch._foreach_mul_(grads, self.rec[1])
            torch._fused_adam_(self.params, grads, m, v, [], steps, amsgrad=False, lr=lr, beta1=B1, beta2=B2, weight_decay=0.0, eps=EPS,
                               maximize=False, grad_scale=None, found_inf=self.rec[3] if self.rec is not None else None)
        self._average(steps[0])


def _state(params, opt, ema, record, lr):
    """Everything a step may write, as flat int32 words."""
    out = {"p": _bits(params)}
    for key in ("exp_avg", "exp_avg_sq", "step"):
        out[key] = _bits([opt.state[p][key] for p in params])
    if ema is not None:
        out["ema"] = _bits(ema)
    if record is not None:
        out["record"] = _bits([record])
    if lr is not None:
        out["lr_out"], out["lr32"] = _bits([lr[0]]), _bits([lr[1]])
    return out


def _drive(ema, guard, sched, own):
    """Four steps of a LeanAdamStep and of its twin on the same gradients; yields (t, lean, its state, the twin's state) behind each."""
    from pdgn_amd import schedule
    from pdgn_amd.trainer import GradGuard, LeanAdamStep
    # half the first step's norm: coef < 1 from the first step on
    max_norm = 0.5 * float(torch.cat([g.double() for g in _gradients(1)]).norm()) if guard else None
    params, opt, avg = _optimizer(ema)
    lean = LeanAdamStep(opt, avg, DECAY if ema else 0.0, GradGuard(params, max_norm) if guard else None,
                        schedule.table(KNOTS, torch.device("cuda")) if sched else None)
    lean._OWN = own
    twin = Twin(ema, guard, sched, own, max_norm)
    for t in range(1, STEPS + 1):
        poisoned = guard and t == 3
        for p, g in zip(params, _gradients(t, poisoned)):
            p.grad = g
        lean.step()
        twin.step(_gradients(t, poisoned))
        torch.cuda.synchronize()
        yield (t, lean,
               _state(params, opt, avg, lean.guard.record if guard else None, (lean.lr_out, lean.lr32) if sched else None),
               _state(twin.params, twin.opt, twin.ema, twin.rec, (twin.lr_out, twin.lr32) if sched else None))


@pytest.mark.parametrize("ema,guard,sched,own", CELLS, ids=CELL_IDS)
def test_every_cell_equals_the_documented_sequence_bit_for_bit(ema, guard, sched, own):
    before = None
    for t, _lean, got, want in _drive(ema, guard, sched, own):
        assert got.keys() == want.keys()
        for key in want:
            assert torch.equal(got[key], want[key]), (t, key, int((got[key] != want[key]).sum()))
        counters = got["step"].view(torch.float32)
        if guard:
            record = got["record"].view(torch.float32)
            if t == 3:                                           # the poisoned step is skipped: nothing but the record moved
                assert float(record[2]) == 0.0 and all(torch.equal(got[k], before[k]) for k in got if k not in ("record", "lr_out", "lr32"))
            else:
                assert float(record[2]) == 1.0 and 0.0 < float(record[1]) < 1.0
            assert bool((counters == (t if t < 3 else t - 1)).all())            # step 4 is applied with t = 3
        else:
            assert bool((counters == t).all())
        assert before is None or not torch.equal(got["p"], before["p"]) or (guard and t == 3)
        before = got


@pytest.mark.parametrize("ema,guard,sched,own", CELLS, ids=CELL_IDS)
def test_route_names_the_path_of_every_step(ema, guard, sched, own):
    routes = []
    for _t, lean, _got, _want in _drive(ema, guard, sched, own):
        routes.append(lean.route)
    assert routes == ["public"] + ["own" if own else "torch"] * (STEPS - 1)


@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
def test_a_refused_own_launch_leaves_the_state_as_it_was(guarded):
    """A negative rate is refused by the library on the host, before any launch: step() raises, and parameters, moments and every
    step counter -- advanced in front of the launch -- are what they were."""
    from pdgn_amd._lib import PdgnHipError
    from pdgn_amd.trainer import GradGuard, LeanAdamStep
    params, opt, _ = _optimizer(False)
    lean = LeanAdamStep(opt, guard=GradGuard(params) if guarded else None)
    lean._OWN = True
    assert lean.route is None
    for t in (1, 2):
        for p, g in zip(params, _gradients(t)):
            p.grad = g
        lean.step()
    assert lean.route == "own"
    before = _state(params, opt, None, None, None)
    assert bool((before["step"].view(torch.float32) == 2.0).all())
    opt.param_groups[0]["lr"] = -1.0
    with pytest.raises(PdgnHipError):
        lean.step()
    torch.cuda.synchronize()
    after = _state(params, opt, None, None, None)
    for key in before:
        assert torch.equal(before[key], after[key]), key
    opt.param_groups[0]["lr"] = LR                               # and the next update is the third
    lean.step()
    torch.cuda.synchronize()
    assert lean.route == "own" and bool((_state(params, opt, None, None, None)["step"].view(torch.float32) == 3.0).all())
