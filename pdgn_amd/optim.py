"""The optimizer step of one network (DESIGN.md sections 7d-7f): the flat gradient buffer of its all-reduce (`FlatGrads`), the
gradient guard's device record (`GradGuard`), and `LeanAdamStep`, which issues a fused, capturable `torch.optim.Adam`'s update
through csrc/adam.hip or torch's private fused call on cached lists.  The trainer (pdgn_amd/trainer.py) builds five of each."""
import ctypes
import os

import torch
import torch.distributed as dist

from . import _lib
from . import fit as _fit
from . import schedule as _schedule
from .fit import GUARD_RECORD_FLOATS
from .fused import clear_zero_colsum, reset_zero_arena


def _fp32_lists(*lists):
    """What the multi-tensor launches of csrc/adam.hip take: lists of contiguous fp32 tensors on one ROCm device, every list as
    long as the first and its i-th tensor as large as the first's."""
    first = lists[0]
    return bool(first) and first[0].is_cuda and all(
        len(lst) == len(first) and all(t.dtype == torch.float32 and t.is_contiguous() and t.device == f.device and t.numel() == f.numel()
                                       for t, f in zip(lst, first)) for lst in lists)


def _pointer_table(tensors):
    """The HOST array of device pointers those launches read a list from."""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _count_table(tensors):
    return (ctypes.c_longlong * len(tensors))(*[t.numel() for t in tensors])


class FlatGrads:
    """One contiguous fp32 buffer per network for the gradient all-reduce.

    Single process: autograd simply assigns fresh ``.grad`` tensors (``begin`` clears them, so no
    per-parameter accumulate kernel runs) and the optimiser consumes them.  Data parallel: after the
    backward one multi-tensor copy packs the gradients into the buffer, ONE collective reduces the
    whole network (G: 50.8 MB, D1-4: 6.8 MB) and the parameters' ``.grad`` become views of it."""

    def __init__(self, params, first=None):
        """first: the parameters whose gradients a backward pass completes FIRST (the deepest block's); they are laid
        out in front and form the early bucket of reduce_early()."""
        ps = [p for p in params if p.requires_grad]
        early = {id(p) for p in (first or [])}
        self.params = [p for p in ps if id(p) in early] + [p for p in ps if id(p) not in early]
        self.n_early = sum(1 for p in ps if id(p) in early)
        # every gradient starts on a 16-byte boundary of the buffer (zero padding between them: the optimizer kernels' float4 path
        # -- csrc/adam.hip, torch's fused Adam alike -- needs it once .grad are these views)
        slot = lambda p: (p.numel() + 3) // 4 * 4
        total = sum(slot(p) for p in self.params)
        ref = self.params[0]
        self.buf = torch.zeros(total, dtype=ref.dtype, device=ref.device)
        self.views, off = [], 0
        for i, p in enumerate(self.params):
            if i == self.n_early:
                self.early_numel = off
            self.views.append(self.buf[off:off + p.numel()].view_as(p))
            off += slot(p)
        if self.n_early == len(self.params):
            self.early_numel = off
        self._early_work, self._early_done = None, False
        self._armed, self._arrived, self._hooks, self._group = False, 0, [], None

    def begin(self):
        """Before a backward: drop the old gradients (autograd then writes, never accumulates)."""
        for p in self.params:
            p.grad = None
        self._early_work, self._early_done = None, False
        self._arrived = 0
        clear_zero_colsum()
        if self.params and self.params[0].is_cuda:
            reset_zero_arena(self.params[0].device, self)

    def resume(self):
        """A further backward pass whose gradients will be ADDED to the ones already there (the second half of a split
        discriminator update): nothing is cleared, only the zero arena is re-opened on the current stream."""
        if self.params and self.params[0].is_cuda:
            reset_zero_arena(self.params[0].device, self)

    def zero_(self):                       # kept for callers that accumulate into the views
        self.buf.zero_()

    def pack(self):
        """Gather the fresh .grad tensors into the flat buffer and re-point .grad at its views (the early bucket only
        if reduce_early() has not already taken it: its slice may be inside a running all-reduce)."""
        self._pack(self.n_early if self._early_done else 0, len(self.params))

    def _pack(self, lo, hi):
        views, params = self.views[lo:hi], self.params[lo:hi]
        have = [(v, p) for v, p in zip(views, params) if p.grad is not None]
        missing = [v for v, p in zip(views, params) if p.grad is None]
        if have:
            self._copy([v for v, _ in have], [p.grad for _, p in have], (lo, hi) if len(have) == hi - lo else None)
        for v in missing:
            v.zero_()
        for v, p in zip(views, params):
            p.grad = v

    def _copy(self, dsts, srcs, full=None):
        """views <- fresh gradients: one launch of csrc/adam.hip's multi-tensor copy per 128 tensors (torch._foreach_copy_: 82 us for
        the generator's 160 gradients); anything but contiguous fp32 CUDA tensors of equal sizes goes torch's way."""
        if os.environ.get("PDGN_OWN_ADAM", "1") == "1" and _fp32_lists(dsts, srcs):
            # (full = (lo, hi): every view of that range takes part -- the views are static, their pointer and size arrays are built once)
            cache = self.__dict__.setdefault("_copy_cache", {})
            hit = cache.get(full) if full is not None else None
            if hit is None:
                hit = (_pointer_table(dsts), _count_table(dsts))
                if full is not None:
                    cache[full] = hit
            _lib.check(_lib.lib().pdgn_copy_multi(len(dsts), hit[0], _pointer_table(srcs), hit[1], _lib.stream_of(dsts[0])), "pdgn_copy_multi")
            return
        torch._foreach_copy_(dsts, srcs)

    def arm_early(self, on=True, group=None):
        """Let the backward itself start the early bucket's all-reduce: a post-accumulate-grad hook on every early
        parameter counts the gradients that HAVE ARRIVED since begin(), and the one that completes the bucket calls
        reduce_early().  Arrival, not a position in the graph, is the trigger: autograd runs a node created before the
        forward (the re-associated operands of PointGenerator.preassemble) after everything of higher sequence number
        that is ready, so "the backward has reached the block's input" does not say that the block's weight gradients
        exist (the early all-reduce then ran on zero-filled slices while AccumulateGrad was still to write
        them).  A parameter that receives no gradient in some backward simply leaves the bucket to all_reduce_mean()."""
        self._armed, self._group = bool(on), group
        if on and not self._hooks and self.n_early:
            for p in self.params[:self.n_early]:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._arrival))

    def _arrival(self, _param):
        if not self._armed or self._early_done:
            return
        self._arrived += 1
        if self._arrived == self.n_early:
            self.reduce_early(self._group)

    def reduce_early(self, group=None):
        """Called from inside the backward once the early bucket's gradients exist (arm_early): pack them and start their
        all-reduce (asynchronous: on RCCL's stream, underneath the rest of the backward).  all_reduce_mean() later
        reduces the rest and joins.  No-op without a process group or without an early bucket, and REFUSED while a
        gradient of the bucket is still missing (its slice would be zero-filled under a running collective)."""
        if self._early_done or self.n_early == 0 or not (dist.is_available() and dist.is_initialized()):
            return
        rec = _recorder(self.buf.device)
        if _capturing(self.buf.device) and rec is None:
            return
        if any(p.grad is None for p in self.params[:self.n_early]):
            return
        self._pack(0, self.n_early)
        self._early_done = True
        if rec is not None:                                      # launch-list capture: the collective becomes a host point of the list

            def start(fg=self, group=group):
                fg._early_work = dist.all_reduce(fg.buf[:fg.early_numel], op=dist.ReduceOp.SUM, group=group, async_op=True)
            rec.point(start)
            return
        self._early_work = dist.all_reduce(self.buf[:self.early_numel], op=dist.ReduceOp.SUM, group=group, async_op=True)

    def all_reduce_mean(self, group=None):
        """Average over ranks (RCCL all-reduce over xGMI when the backend is nccl)."""
        if dist.is_available() and dist.is_initialized():
            rec, early = _recorder(self.buf.device), self._early_done
            if rec is not None:                                  # launch-list capture: the sum is a host point; the division is captured
                rec.point(lambda: self._reduce_sum(group, early))
            else:
                self._reduce_sum(group, early)
            if dist.get_world_size(group) > 1:
                self.buf.div_(dist.get_world_size(group))

    def _reduce_sum(self, group, early):
        """The sum over ranks of `also_sum` and of the buffer.  early: reduce_early() took the early bucket in this backward -- the
        rest is reduced here and the early work joined."""
        self._sum_also(group)
        if early:
            if self.early_numel < self.buf.numel():
                dist.all_reduce(self.buf[self.early_numel:], op=dist.ReduceOp.SUM, group=group)
            self._early_work.wait()
            self._early_work = None
        else:
            dist.all_reduce(self.buf, op=dist.ReduceOp.SUM, group=group)

    also_sum = ()                                               # small integer tensors all-reduced (SUM) with this buffer, at its host point

    def _sum_also(self, group=None):
        for t in self.also_sum:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)


def _capturing(device):
    return device.type == "cuda" and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _recorder(device):
    """The active host-point recorder of a launch-list capture (replay.Recorder), or None."""
    if device.type != "cuda":
        return None
    from . import replay
    rec = replay.recorder()
    return rec if rec is not None and _capturing(device) else None


class GradGuard:
    """One network's gradient guard: the device-side record that pdgn_gradnorm_multi writes from the network's
    whole gradient list and the guarded optimizer launches read, the fp64 workspace of the reduction, and the clipping bound.

    record: 8 fp32 words of device memory laid out as pdgn_guard_record (a row of the trainer's `guard_buf`), zero at the start;
    `applied`, `found_inf` and `coef` are 0-dim views of it -- the device values LeanAdamStep hands to torch (`_foreach_add_` on the
    step counters, `found_inf` of torch's fused kernel, `_foreach_mul_` on the gradients): the host never reads them inside a step.
    max_norm: None / 0 / inf = no clipping (coef is exactly 1)."""

    def __init__(self, params, max_norm=None, record=None):
        params = list(params)
        dev = params[0].device
        self.max_norm = 0.0 if max_norm is None else float(max_norm)
        if self.max_norm != self.max_norm or self.max_norm < 0:
            raise ValueError("clip_grad_norm must be a positive number (or None), got %r" % (max_norm,))
        self.record = record if record is not None else torch.zeros(GUARD_RECORD_FLOATS, dtype=torch.float32, device=dev)
        if (self.record.dtype != torch.float32 or self.record.numel() != GUARD_RECORD_FLOATS or not self.record.is_contiguous()
                or self.record.device != dev):
            raise ValueError("guard record: %d contiguous fp32 words on the parameters' device" % GUARD_RECORD_FLOATS)
        self.coef, self.applied, self.found_inf = self.record[1], self.record[2], self.record[3]
        self.counters = self.record.view(torch.int32)[4:6]
        counts = _count_table(params)
        # pdgn_gradnorm_workspace_doubles(): one partial per 4096-element chunk (the library checks the size it is given; on the CPU
        # device the trainer can be built and inspected, the launches themselves raise)
        self.workspace = torch.zeros(sum((p.numel() + 4095) // 4096 for p in params), dtype=torch.float64, device=dev)
        self._n, self._counts = len(params), counts

    def measure(self, grads):
        """record <- norm, coef, applied of this gradient list: the partial launches and the finalising one, on the current stream."""
        if len(grads) != self._n or not _fp32_lists(grads) or any(g.numel() != c for g, c in zip(grads, self._counts)):
            raise _lib.PdgnHipError("the gradient guard reads one contiguous fp32 gradient per parameter on a ROCm device; this list "
                                    "cannot be guarded")
        _lib.check(_lib.lib().pdgn_gradnorm_multi(self._n, _pointer_table(grads), self._counts, self.max_norm, _lib.ptr(self.workspace),
                                                  self.workspace.numel(), _lib.ptr(self.record), _lib.stream_of(grads[0])),
                   "pdgn_gradnorm_multi")

    decode = staticmethod(_fit.decode_guard_record)

    def state(self):
        """The record as a dict (synchronises: a device-to-host copy on the current stream)."""
        return self.decode(self.record.cpu())


class LeanAdamStep:
    """`optimizer.step()` of a fused, capturable `torch.optim.Adam` without its per-call Python (profile hooks, `_init_group`,
    grouping by device and dtype: ~0.3 ms of host time per call, five calls per training step -- tools/host_prof.py): after the
    first, ordinary step the same two calls torch makes -- `_foreach_add_` on the step counters, `_fused_adam_` on the parameter /
    gradient / moment lists -- are issued on lists cached here.  The state stays the optimizer's own (checkpoints, broadcasts and
    `state_dict()` are untouched); anything unusual (a parameter without gradient, several groups, amsgrad, weight decay, a
    non-fused optimizer, step hooks, replaced state tensors) keeps calling `optimizer.step()`; the invariants are re-checked on
    every call.  `torch._fused_adam_` / `torch._foreach_add_` are private torch entry points (written against torch 2.10): a
    changed signature falls back to `optimizer.step()` for good.

    ema / ema_decay (the generator's optimizer under `PDGNTrainer(ema_decay=...)`): one fp32 tensor per parameter, in the order of
    the optimizer's group, holding the exponential moving average of that parameter.  Every route out of `step` updates it on the
    same stream, right behind the parameters: the own Adam kernel in its own launch (pdgn_adam_ema_multi), every other route with
    pdgn_ema_multi behind the optimizer step (csrc/adam.hip: the same expressions, the same bits).

    guard (a GradGuard; None: nothing below exists): `step` first runs the norm launches on the gradients as they are at that moment
    -- behind the all-reduce under data parallelism, so every rank decides from the same bytes -- then advances the step counters by
    the DEVICE value `applied` and runs the guarded launch (pdgn_adam_guard_multi / pdgn_adam_ema_guard_multi).  A skipped update
    leaves parameters, moments, counters and the average byte-identical.  The routes through torch (`optimizer.step()`,
    `torch._fused_adam_`) scale the gradients in place by `coef` beforehand -- the one case where the guard writes g -- and hand the
    flag to torch's kernel as `found_inf`, which makes it return early (and `optimizer.step()` take its increment back); the average
    behind them is pdgn_ema_guard_multi.  An optimizer that cannot take `found_inf` (not fused, not capturable) raises: no route
    applies an unguarded update while the guard is on.

    sched (a learning-rate table, schedule.table(): 33 fp64 words on the parameters' device; None: nothing below exists): the rate
    of every update is lr * f(t), with lr the Python float of the group -- it stays the BASE rate -- and t the count of that update
    (DESIGN.md section 7f).  The own kernel evaluates the table itself (pdgn_adam_sched_multi: no launch more).  The routes through
    torch -- the first, ordinary `optimizer.step()`, the fall-backs, `PDGN_OWN_ADAM=0` / `torch._fused_adam_` -- run pdgn_lr_eval on the
    same stream first and hand torch's fused, capturable kernel the resulting fp32 device scalar as a tensor `lr` (for
    `optimizer.step()` it sits in the group for the duration of the call): on those routes the rate is lr * f(t) ROUNDED TO FP32.  An
    optimizer that cannot take a tensor rate (not fused, not capturable, several groups) raises: no route applies the unscheduled
    rate while a schedule is set.  The table is read, never replaced: overwrite it in place to change the schedule."""

    def __init__(self, opt, ema=None, ema_decay=0.0, guard=None, sched=None):
        self.opt, self.lists, self._table, self._route = opt, None, None, None
        self.ema, self.ema_decay, self._ema_table = (list(ema) if ema else None), float(ema_decay), None
        self.guard = guard
        self.sched = sched
        if sched is not None:
            if not (torch.is_tensor(sched) and sched.dtype == torch.float64 and sched.numel() == _schedule.TABLE_DOUBLES
                    and sched.is_contiguous()):
                raise ValueError("lr schedule: a contiguous torch.float64 tensor of %d words (schedule.table)" % _schedule.TABLE_DOUBLES)
            self.lr_out = torch.zeros(2, dtype=torch.float64, device=sched.device)      # {f, lr_eff} of the last pdgn_lr_eval
            self.lr32 = torch.zeros((), dtype=torch.float32, device=sched.device)       # lr_eff as torch's kernel takes it

    @property
    def route(self):
        """Which way the last `step()` went: None before the first, "public" (`optimizer.step()`), "torch" (`torch._fused_adam_` on the
        cached lists) or "own" (csrc/adam.hip)."""
        return self._route

    def reset(self):
        """The optimizer's state tensors were replaced (load_state_dict): rebuild the lists after the next ordinary step."""
        self.lists = None
        self._table = None
        self._ema_table = None

    def _eval_lr(self, step=None):
        """lr32 <- (float)(lr * f(t)) for the update about to happen, t = step + 1 (step + applied behind a guard, whose record is
        complete by now): one one-thread launch on the current stream.  step: the optimizer's device-side counter (default: the
        first parameter's; zero before the optimizer's first step has made one)."""
        opt = self.opt
        if len(opt.param_groups) != 1 or not all(g.get("fused") and g.get("capturable") for g in opt.param_groups):
            raise _lib.PdgnHipError("a learning-rate schedule reaches torch's Adam as a tensor `lr`, which takes a fused, capturable "
                                    "optimizer with one parameter group; the unscheduled rate is not an option")
        g = opt.param_groups[0]
        if isinstance(g["lr"], torch.Tensor):
            raise _lib.PdgnHipError("a learning-rate schedule multiplies a Python float base rate; this group's lr is a tensor")
        if step is None:
            st = opt.state.get(g["params"][0])
            step = st["step"] if st and "step" in st else torch.zeros(1, dtype=torch.float32, device=self.sched.device)
        if not (torch.is_tensor(step) and step.is_cuda and step.dtype == torch.float32 and step.device == self.sched.device):
            raise _lib.PdgnHipError("a learning-rate schedule reads Adam's step count on the device: a capturable optimizer on the "
                                    "table's device is required")
        _lib.check(_lib.lib().pdgn_lr_eval(_lib.ptr(self.sched), float(g["lr"]), _lib.ptr(step),
                                           _lib.ptr(self.guard.record) if self.guard is not None else None, _lib.ptr(self.lr_out),
                                           _lib.ptr(self.lr32), _lib.stream_of(self.sched)), "pdgn_lr_eval")
        return self.lr32

    def _public_step(self, measured=False):
        """`optimizer.step()` itself, with the average behind it.  Guarded: the gradients are measured and scaled by coef first
        (measured: that has happened already), and the optimizer takes the skip flag as `found_inf`, as it does from a GradScaler.
        Scheduled: the fp32 device scalar sits in the group while torch runs, the float is back afterwards (checkpoints and the lean
        step's invariants see the base rate)."""
        opt, guard = self.opt, self.guard
        if guard is not None:
            if len(opt.param_groups) != 1 or not all(g.get("fused") and g.get("capturable") for g in opt.param_groups):
                raise _lib.PdgnHipError("the gradient guard hands its skip flag to torch's fused, capturable Adam as `found_inf`; this "
                                        "optimizer cannot take it, and an unguarded update is not an option")
            params = opt.param_groups[0]["params"]
            if any(p.grad is None for p in params):
                raise _lib.PdgnHipError("the gradient guard needs a gradient for every parameter of the optimizer")
            if not measured:
                grads = [p.grad for p in params]
                guard.measure(grads)
                with torch.no_grad():
                    torch._foreach_mul_(grads, guard.coef)
            opt.grad_scale, opt.found_inf = None, guard.found_inf
        g = base = None
        try:
            if self.sched is not None:
                lr32 = self._eval_lr()
                g = opt.param_groups[0]
                base, g["lr"] = g["lr"], lr32
            opt.step()
        finally:
            if g is not None:
                g["lr"] = base
            if guard is not None:
                opt.grad_scale = opt.found_inf = None
        self._ema_alone()
        self._route = "public"

    def _ema_alone(self):
        """e <- e + (1 - d_t)(p - e) behind an optimizer step that was not pdgn_adam_ema_multi: one launch per 128 tensors on the
        current stream; t is the optimizer's own device-side step count (already incremented by that step).  There is no torch
        form of it: anything but fp32 CUDA tensors and a device-side fp32 counter raises."""
        if self.ema is None:
            return
        ps = self.opt.param_groups[0]["params"]
        step = self.opt.state[ps[0]]["step"]
        n = len(ps)
        tab = self._ema_table
        if tab is None or tab[0] != n or tab[2][0] != ps[0].data_ptr() or tab[2][n - 1] != ps[n - 1].data_ptr():
            if not _fp32_lists(ps, self.ema):
                raise _lib.PdgnHipError("the averaged generator needs contiguous fp32 parameters on a ROCm device (pdgn_amd has no CPU path)")
            tab = self._ema_table = (n, _pointer_table(self.ema), _pointer_table(ps), _count_table(ps))
        if not (torch.is_tensor(step) and step.is_cuda and step.dtype == torch.float32):
            raise _lib.PdgnHipError("the averaged generator reads Adam's step count on the device: a capturable optimizer is required")
        if self.guard is not None:                               # skipped on the device with the update in front of it
            _lib.check(_lib.lib().pdgn_ema_guard_multi(n, tab[1], tab[2], tab[3], self.ema_decay, _lib.ptr(step), _lib.ptr(self.guard.record),
                                                       _lib.stream_of(ps[0])), "pdgn_ema_guard_multi")
            return
        _lib.check(_lib.lib().pdgn_ema_multi(n, tab[1], tab[2], tab[3], self.ema_decay, _lib.ptr(step), _lib.stream_of(ps[0])), "pdgn_ema_multi")

    _OWN = os.environ.get("PDGN_OWN_ADAM", "1") == "1"           # A/B switch: 0 = torch._fused_adam_

    def _own_tables(self, ps, grads, exp_avgs, exp_avg_sqs, steps):
        """The route of a lean step, decided before anything is launched: (table, ema table or None) when csrc/adam.hip takes the list,
        None when torch's kernel does -- the switch is off, or the list is anything but contiguous fp32 CUDA tensors.  The pointer
        tables are built here once and checked against the lists' ends afterwards (`reset` and every other place that drops `lists`
        drops them).  The kernels read ONE step count, steps[0]: torch keeps one per tensor, and a loaded state whose counts differ
        would get steps[0]'s bias corrections -- not checked, since comparing them is a host read of device counters, which a
        capturing stream refuses."""
        if not self._OWN or not ps or not ps[0].is_cuda:
            return None
        n = len(ps)
        tab = self._table
        if tab is None or tab[0] != n or tab[1][0] != ps[0].data_ptr() or tab[2][n - 1] != exp_avgs[n - 1].data_ptr():
            if not _fp32_lists(ps, exp_avgs, exp_avg_sqs) or steps[0].dtype != torch.float32:
                return None
            tab = self._table = (n, _pointer_table(ps), _pointer_table(exp_avgs), _pointer_table(exp_avg_sqs), _count_table(ps))
        if any(t.dtype != torch.float32 or not t.is_contiguous() for t in grads):
            return None
        et = None
        if self.ema is not None:                                 # the average rides in the same launches
            et = self._ema_table
            if et is None or et[0] != n or et[2][0] != tab[1][0] or et[2][n - 1] != tab[1][n - 1]:
                return None                                      # (not validated yet, or other parameters: _ema_alone checks and raises)
        return tab, et

    def _own_launch(self, tables, grads, step, g):
        """The whole list in ceil(n / 72) launches of csrc/adam.hip (64 with the averages), one workgroup per 4096 elements (torch's
        fused kernel: 64 K-element chunks, five launches and 230 us for the generator's 12.7 M parameters at the end of every
        iteration).  The pointers travel in the kernel arguments: nothing to upload, and a recorded iteration re-issues them as they
        were.  One entry point per (ema, guard), and one for the four scheduled kernels, which takes every argument of the others."""
        (n, p, m, v, counts), et = tables
        ema, guard, sched = et is not None, self.guard is not None, self.sched is not None
        L = _lib.lib()
        if sched:
            fn = L.pdgn_adam_sched_multi
        elif ema:
            fn = L.pdgn_adam_ema_guard_multi if guard else L.pdgn_adam_ema_multi
        else:
            fn = L.pdgn_adam_guard_multi if guard else L.pdgn_adam_multi
        args = (n, p, _pointer_table(grads), m, v)
        if ema or sched:
            args += (et[1] if ema else None,)
        args += (counts, g["lr"], g["betas"][0], g["betas"][1], g["eps"])
        if ema or sched:
            args += (self.ema_decay,)
        args += (_lib.ptr(step),)
        if guard or sched:
            args += (_lib.ptr(self.guard.record) if guard else None,)
        if sched:
            args += (_lib.ptr(self.sched),)
        _lib.check(fn(*args, _lib.stream_of(step)), fn.__name__)

    def step(self):
        opt = self.opt
        if self.lists is None:
            self._public_step()
            g = opt.param_groups[0]
            ok = (len(opt.param_groups) == 1 and g.get("fused") and g.get("capturable") and not g.get("amsgrad")
                  and not g.get("maximize") and not g.get("differentiable") and g.get("weight_decay", 0) == 0
                  and not isinstance(g["lr"], torch.Tensor) and all(p.grad is not None for p in g["params"])
                  and os.environ.get("PDGN_LEAN_ADAM", "1") == "1")
            if ok:
                ps, st = list(g["params"]), opt.state
                self.lists = (ps, [st[p]["exp_avg"] for p in ps], [st[p]["exp_avg_sq"] for p in ps], [st[p]["step"] for p in ps])
            else:
                self.lists = False
            return
        if self.lists is False:
            self._public_step()
            return
        ps, exp_avgs, exp_avg_sqs, steps = self.lists
        grads = [p.grad for p in ps]
        g = opt.param_groups[0]
        # cheap invariants, every call: one group over the same parameters, no weight decay / amsgrad / maximize, a Python float
        # learning rate, the optimizer's own state tensors still the cached ones, no step hooks, every gradient present
        st0 = opt.state.get(ps[0]) if ps else None
        if (len(opt.param_groups) != 1 or len(g["params"]) != len(ps) or g.get("weight_decay", 0) != 0 or g.get("amsgrad")
                or g.get("maximize") or isinstance(g["lr"], torch.Tensor) or st0 is None or st0.get("exp_avg") is not exp_avgs[0]
                or opt._optimizer_step_pre_hooks or opt._optimizer_step_post_hooks or any(gr is None for gr in grads)):
            self.reset()                                         # re-validated after the next ordinary step
            self._public_step()
            return
        self._lean_step(ps, grads, exp_avgs, exp_avg_sqs, steps, g)

    def _lean_step(self, ps, grads, exp_avgs, exp_avg_sqs, steps, g):
        """The update on the cached lists: the route, decided once; behind a guard the norm launches; on torch's route the schedule's
        rate as a device scalar, from the counter BEFORE its increment; counters += 1, or += applied (a device value) behind a guard;
        then the own launch -- or torch's fused kernel, behind a guard on gradients scaled in place by coef and with the flag as its
        `found_inf`, and the average behind it."""
        guard = self.guard
        own = self._own_tables(ps, grads, exp_avgs, exp_avg_sqs, steps)
        if guard is not None:
            guard.measure(grads)
        lr = g["lr"]
        if self.sched is not None and own is None:
            lr = self._eval_lr(steps[0])                         # (behind the norm launches: t = step + applied)
        # (the list form, as torch's own capturable optimizers take `found_inf` back: `_foreach_add_(list, Tensor)` reads its tensor on
        #  the host, which a capturing stream refuses)
        inc = 1 if guard is None else [guard.applied] * len(steps)
        scaled = False
        with torch.no_grad():
            torch._foreach_add_(steps, inc)
            try:
                if own is not None:
                    self._own_launch(own, grads, steps[0], g)
                    self._route = "own"
                    return
                if guard is not None:
                    torch._foreach_mul_(grads, guard.coef)
                    scaled = True
                torch._fused_adam_(ps, grads, exp_avgs, exp_avg_sqs, [], steps, amsgrad=False, lr=lr, beta1=g["betas"][0],
                                   beta2=g["betas"][1], weight_decay=0.0, eps=g["eps"], maximize=False, grad_scale=None,
                                   found_inf=guard.found_inf if guard is not None else None)
            except _lib.PdgnHipError:                            # a refused own launch applied nothing: the counters get their increment back
                torch._foreach_sub_(steps, inc)
                raise
            except TypeError:                                    # the private op's signature changed (another torch version): undo the
                torch._foreach_sub_(steps, inc)                  # counters and take the public path from now on (the gradients may be
                self.reset()                                     # scaled already: not twice)
                self.lists = False
                self._public_step(measured=scaled)
                return
        self._ema_alone()
        self._route = "torch"
