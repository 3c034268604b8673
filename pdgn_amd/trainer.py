"""One PDGN training iteration (models/PDGNet_v2.py:171-256) and its batch-axis data parallelism.

Reference parallelism: single-process ``nn.DataParallel`` (:101-105) -- per-replica BatchNorm
statistics, gradients summed onto GPU 0.  Here: one process per GPU, local batch per rank,
BatchNorm statistics stay local (same semantics), and gradients are all-reduced over RCCL/xGMI
as ONE flat fp32 buffer per network (G: 50.8 MB, D1-4: 6.8 MB) -- parameters' ``.grad`` tensors
are views into that buffer, so there is no bucket copy in or out.

The epoch loop over a feeder (`PDGNTrainer.fit`) and its logs are in pdgn_amd/fit.py; the flat gradient buffer, the gradient guard
and the optimizer step (`FlatGrads`, `GradGuard`, `LeanAdamStep`) are in pdgn_amd/optim.py and importable from here as before.
"""
import contextlib
import os
import warnings

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib
from . import fit as _fit
from . import schedule as _schedule
from . import streams as _streams
from .fused import flush_bn_counters, hold_bn_counters, release_zero_arena
from .generator import PointDiscriminator, PointGenerator
from . import losses
from .fit import GUARD_RECORD_FLOATS, GradGuardError          # (defined beside the loop that reads and raises them)
from .losses import LocalPairLoss
from .optim import FlatGrads, GradGuard, LeanAdamStep        # (tests and tools import them from here too)

PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))   # get_local_pair calls :232-237


class DeterminismWarning(UserWarning):
    """The library's deterministic mode is on, but the operation at hand has no fixed-order form yet."""


def _warn_if_deterministic(what):
    """The deterministic mode (pdgn_amd.set_deterministic, or torch's flag) covers the reference-compatible pointops /
    nn_distance adjoints; the training step still sums with float atomics: say so instead of
    letting a user who asked for repeatable runs believe they have them."""
    if _lib.deterministic():
        warnings.warn("PDGNTrainer.%s: deterministic mode is on, but the training step has no fixed-order form yet -- its "
                      "weight gradients and adjoints still sum with float atomics, so runs are not bitwise repeatable "
                      "(DESIGN.md section 5)" % what, DeterminismWarning, stacklevel=3)


def world_size():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class PDGNTrainer:
    """Generator + D1..D4 + their Adam optimisers (lr 1e-4, betas (0.5, 0.999), :121-125) and the
    op sequence of one iteration.  ``step`` returns the six logged losses (:259-261) as 0-dim
    device tensors (no host sync inside the step).

    ema_decay > 0 keeps an exponential moving average of the generator's parameters (`ema`: one view per parameter of the flat
    `ema_buf`), updated by the generator's optimizer step itself (LeanAdamStep); `averaged_generator()`
    puts it into the generator for a while, `save` writes it as `<epoch>_<category>_G_ema.pth`.  0: nothing of this exists.

    lr_g / lr_d: the base rate of the generator's optimizer / of the four discriminators' (None: `lr`).  lr_schedule: a knot list
    [(t, factor), ...] (schedule.knots / schedule.validate) or None.  With one, the trainer owns ONE device table (`lr_table`, 33
    fp64 words) that all five optimizers' launches evaluate at their own step count: rate = base * f(t);
    `param_groups[..]["lr"]` stays the Python float base rate, so checkpoints are what they were.  `set_lr_schedule` overwrites the
    table in place (a captured launch list follows it with no recapture), `lr_state` reads the current rates.  With none of the
    three nothing of this exists: no buffer, no launch, the same kernels and the same list.

    augment: None, an augment.Augment, or a dict of its arguments.  With one, every cloud a discriminator sees -- all twelve calls of
    an iteration -- goes through a random similarity transform drawn on the device: `aug` owns the parameter
    table, the clock and the optional record buffer; the iteration opens with ONE extra launch, the clock's tick; `set_augment`
    overwrites the table in place, `aug_state` reads it back.  The shape-preserving loss sees the un-augmented clouds.  None: `aug`
    is None, no buffer, no launch, and the discriminators' forward is the code it was.  With augment={..., "adaptive": {...}} p is
    steered on the device: the four real-batch loss terms count into `aug.slots`, the tick folds them.

    gan_loss: the adversarial objective of all twelve terms of an iteration (losses.adversarial): "lsgan", the
    reference's least squares and the default -- the launches it always had --, "hinge" or "logistic" (non-saturating), on the
    discriminators' raw scores; `gan_loss` keeps the name.  The kind is baked into the launches (a captured list keeps the one it was
    captured with), adds none, and is not written into checkpoints.  The adaptive augmentation counts the real scores against the
    objective's decision boundary: 1/2 under "lsgan", 0 otherwise.

    repulsion: None, or {"weight": w, "radius": h, "levels": (0, 1, 2, 3)} (levels optional).  With one, the generator's loss gains
    w * sum_l losses.repulsion(gen_l, h_l) over the named levels of pass #2's clouds: h is the finest level's
    radius, h_l = losses.repulsion_radii's.  The term is a batch MEAN like the adversarial ones, so data parallelism needs no factor
    for it.  `out["g_loss"]` includes it, `out["repulsion_loss"]` is the unweighted sum over the levels, `repulsion_state()` reads the
    per-level values; `set_repulsion(weight=...)` overwrites the weight in place (a captured list follows), a new radius needs a
    recapture.  Every sum of the term runs in a fixed order: under `set_deterministic` it adds no non-determinism of its own (the
    step's other sums still warn).  None: `repulsion` is None, no buffer, no launch, the same list and the same six `out` keys.

    flatness: None, or {"weight": w, "k": 16, "eps": e, "levels": (0, 1, 2, 3)} (k, eps and levels optional).  With one, the generator's
    loss gains w * sum_l losses.flatness(gen_l, k, eps=e_l) over the named levels of pass #2's clouds: the batch
    mean of the surface variation of every point's k nearest neighbours (one pdgn_knnquery per level, on the detached cloud); e is the
    finest level's floor, e_l = losses.flatness_floors'.  A batch MEAN like repulsion: no world-size factor.  `out["g_loss"]` includes
    it, `out["flatness_loss"]` is the unweighted sum over the levels, `flatness_state()` reads the per-level values and the number of
    degenerate points; `set_flatness(weight=...)` overwrites the weight in place (a captured list follows), a new k or eps needs a
    recapture.  Fixed-order sums, no float atomics.  May be combined with `repulsion`.  None: `flatness` is None, no buffer, no launch,
    the same list and the same `out` keys."""

    def __init__(self, device="cuda", lr=1e-4, num_k=20, base_points=128, generator=None,
                 discriminators=None, distributed=None, ema_decay=0.0, grad_guard=False, clip_grad_norm=None,
                 lr_g=None, lr_d=None, lr_schedule=None, augment=None, gan_loss="lsgan", repulsion=None, flatness=None):
        if gan_loss not in losses.GAN_LOSSES:                    # (raises before anything is allocated)
            raise ValueError("gan_loss must be one of %s, got %r" % (", ".join(losses.GAN_LOSSES), gan_loss))
        self.gan_loss = gan_loss
        self.repulsion = None if repulsion is None else self._check_repulsion(repulsion)     # (raises before anything is allocated)
        self.flatness = None if flatness is None else self._check_flatness(flatness)
        if not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError("ema_decay must be in [0, 1), got %r" % (ema_decay,))
        self.ema_decay = float(ema_decay)
        if clip_grad_norm is not None and not float(clip_grad_norm) > 0.0:
            raise ValueError("clip_grad_norm must be positive (or None), got %r" % (clip_grad_norm,))
        self.clip_grad_norm = None if clip_grad_norm is None else float(clip_grad_norm)
        self.grad_guard = bool(grad_guard) or self.clip_grad_norm is not None
        for name, rate in (("lr", lr), ("lr_g", lr_g), ("lr_d", lr_d)):
            if rate is not None and not float(rate) >= 0.0:
                raise ValueError("%s must not be negative, got %r" % (name, rate))
        self.per_network_lr = lr_g is not None or lr_d is not None
        lr_g, lr_d = float(lr if lr_g is None else lr_g), float(lr if lr_d is None else lr_d)
        knots = None if lr_schedule is None else _schedule.validate(lr_schedule)     # (raises before anything is allocated)
        self.device = torch.device(device)
        self.aug = None
        if augment is not None:
            from . import augment as _augment
            if isinstance(augment, dict):
                # (under data parallelism every rank draws for its own global rows: rank * B + b)
                rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
                augment = _augment.Augment(**dict({"rank": rank, "device": self.device}, **augment))      # (validates; raises before allocating)
            elif not isinstance(augment, _augment.Augment):
                raise TypeError("augment: None, an augment.Augment or a dict of its arguments, got %r" % (type(augment),))
            self.aug = augment
        self.G = (generator or PointGenerator(num_k=num_k, base_points=base_points)).to(self.device)
        self.D = [d.to(self.device) for d in
                  (discriminators or [PointDiscriminator(i, (2 * base_points) << (i - 1)) for i in (1, 2, 3, 4)])]
        self.local_pair = LocalPairLoss(20)
        self.distributed = world_size() > 1 if distributed is None else distributed
        # the deepest block's gradients are complete when the backward reaches that block's input: they form the early
        # bucket whose all-reduce runs underneath the rest of the backward (PDGN_BUCKETS=0: one all-reduce at the end)
        self._buckets = os.environ.get("PDGN_BUCKETS", "1") == "1"
        deepest = (list(self.G.bilateral4.parameters()) + list(self.G.mlp4.parameters())) if self._buckets and hasattr(self.G, "bilateral4") else None
        self.gradG = FlatGrads(self.G.parameters(), first=deepest)
        if self.distributed and self._buckets:
            self.gradG.arm_early()
        self.gradD = [FlatGrads(d.parameters()) for d in self.D]
        if self.distributed and self.aug is not None and self.aug.adaptive is not None:
            # the adaptive augmentation's counts are summed over the ranks where the generator's gradients are: that all-reduce is
            # ordered behind all four real-batch terms (G's backward passes through every D after its update), and the next tick behind it
            self.gradG.also_sum = [self.aug.slots]
        cap = self.device.type == "cuda"                     # device-side step counter: graph-capturable
        adam = lambda m, lr: torch.optim.Adam(m.parameters(), lr=lr, betas=(0.5, 0.999), capturable=cap, fused=cap and os.environ.get("PDGN_FUSED_ADAM", "1") == "1")
        self.optG, self.optD = adam(self.G, lr_g if self.per_network_lr else lr), [adam(d, lr_d if self.per_network_lr else lr) for d in self.D]
        # one table for the five optimizers: its address is in every scheduled launch, its contents are set_lr_schedule's to change
        self.lr_table = None if knots is None else _schedule.table(knots, self.device)
        self.ema_buf = self.ema = self._ema_spare = None
        if self.ema_decay > 0:
            # one flat buffer, every average on a 16-byte boundary of it (the kernels' float4 path), in the optimizer's order
            self.ema_buf, self.ema = self._flat_like(self.optG.param_groups[0]["params"])
        self.guard_buf = self.guards = None
        if self.grad_guard:
            # one record per network (G, D1..D4: the rows of guard_buf), each with its own workspace -- the five updates run on
            # five streams; the bound applies to each network separately, as torch.nn.utils.clip_grad_norm_ per module would
            self.guard_buf = torch.zeros(len(self.GUARD_KEYS), GUARD_RECORD_FLOATS, dtype=torch.float32, device=self.device)
            self.guards = [GradGuard(o.param_groups[0]["params"], self.clip_grad_norm, self.guard_buf[i])
                           for i, o in enumerate([self.optG] + self.optD)]
        guard_of = lambda i: self.guards[i] if self.guards is not None else None
        self._stepG = LeanAdamStep(self.optG, self.ema, self.ema_decay, guard_of(0), self.lr_table)
        self._stepD = [LeanAdamStep(o, guard=guard_of(1 + i), sched=self.lr_table) for i, o in enumerate(self.optD)]
        # stream-overlapped schedule of the eager step (see _step_overlapped); PDGN_OVERLAP=0 turns it off
        self.overlap = cap and os.environ.get("PDGN_OVERLAP", "1") == "1"
        self._side = None
        self._lw = {}
        if self.repulsion is not None:
            self._rep_buf = torch.zeros(4, dtype=torch.float32, device=self.device)       # the last iteration's value per level
            self._rep_zero = torch.zeros((), dtype=torch.float32, device=self.device)     # (a level that is not in `levels`)
        if self.flatness is not None:
            self._flat_buf = torch.zeros(4, dtype=torch.float32, device=self.device)      # the last iteration's value per level
            self._flat_zero = torch.zeros((), dtype=torch.float32, device=self.device)
            self._flat_deg = {}                                  # level -> (B) int32: the last iteration's degenerate points per cloud
        for ws in {1, world_size() if self.distributed else 1}:
            self._loss_weights(ws)
        self._early_tail = os.environ.get("PDGN_EARLY_TAIL", "1") == "1"
        self._split_d = os.environ.get("PDGN_SPLIT_D", "1") == "1"
        self._defer_d = os.environ.get("PDGN_DEFER_D", "1") == "1"
        self._ema_from_parameters()
        self.sync_replicas()

    GUARD_KEYS = _fit.GUARD_KEYS

    def guard_state(self):
        """{network: {norm, coef, applied, skipped}} for G, D1..D4: norm and clip factor of each network's LAST gradient list, and
        the running numbers of applied and skipped updates.  Synchronises the device.  Guard on only."""
        if self.guards is None:
            raise RuntimeError("guard_state(): this trainer has no gradient guard (grad_guard=False, clip_grad_norm=None)")
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        host = self.guard_buf.cpu()
        return {k: GradGuard.decode(host[i]) for i, k in enumerate(self.GUARD_KEYS)}

    @staticmethod
    def _check_repulsion(cfg):
        """{"weight", "radius", "levels"} validated: weight finite and >= 0, radius finite and > 0, levels a non-empty ascending
        subset of (0, 1, 2, 3)."""
        if not isinstance(cfg, dict) or set(cfg) - {"weight", "radius", "levels"} or not {"weight", "radius"} <= set(cfg):
            raise ValueError("repulsion: None or {'weight': w, 'radius': h, 'levels': (0, 1, 2, 3)}, got %r" % (cfg,))
        weight, radius = float(cfg["weight"]), float(cfg["radius"])
        if not (0.0 <= weight < float("inf")):
            raise ValueError("repulsion weight must be finite and not negative, got %r" % (cfg["weight"],))
        if not (0.0 < radius < float("inf")):
            raise ValueError("repulsion radius must be finite and positive, got %r" % (cfg["radius"],))
        levels = tuple(int(l) for l in cfg.get("levels", (0, 1, 2, 3)))
        if not levels or list(levels) != sorted(set(levels)) or levels[0] < 0 or levels[-1] > 3:
            raise ValueError("repulsion levels: a non-empty ascending subset of (0, 1, 2, 3), got %r" % (cfg.get("levels"),))
        return {"weight": weight, "radius": radius, "levels": levels}

    def set_repulsion(self, weight=None, radius=None):
        """Change the repulsion term.  weight: written INTO the loss-weight vectors -- the tensors a launch list has baked in: the
        next `step_list()` (or eager step) uses it, with no recapture.  radius: a launch ARGUMENT, so a captured list or graph keeps
        the one it was captured with: raises while one exists.  Raises on a trainer built without `repulsion`."""
        if self.repulsion is None:
            raise RuntimeError("set_repulsion(): this trainer was built without repulsion; build it with one (e.g. weight 0.0)")
        fresh = self._check_repulsion({"weight": self.repulsion["weight"] if weight is None else weight,
                                       "radius": self.repulsion["radius"] if radius is None else radius,
                                       "levels": self.repulsion["levels"]})
        if radius is not None and fresh["radius"] != self.repulsion["radius"] and (
                getattr(self, "_list", None) is not None or getattr(self, "_graphs", None)):
            raise RuntimeError("set_repulsion(radius=...): the radius is an argument of the captured launches; capture again with the new one")
        self.repulsion = fresh
        with torch.no_grad():
            for w in self._lw.values():
                w[5:6].fill_(fresh["weight"])

    def repulsion_state(self):
        """{weight, radius, levels, radii, per_level, total}: the parameters, the radius of each of the four levels for the last
        iteration's cloud sizes (None before the first), and the last iteration's unweighted value per level (0 for a level that is not
        in `levels`) with their sum.  Synchronises the device."""
        if self.repulsion is None:
            raise RuntimeError("repulsion_state(): this trainer was built without repulsion")
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        per = [float(v) for v in self._rep_buf.cpu()]
        return dict(self.repulsion, radii=self.__dict__.get("_rep_radii"), per_level=per, total=float(sum(per)))

    def _repulsion_radii(self, sizes):
        """The four levels' radii for these point counts (cached: the same sizes every iteration)."""
        key = (self.repulsion["radius"],) + tuple(int(n) for n in sizes)
        if self.__dict__.get("_rep_key") != key:
            self._rep_key, self._rep_radii = key, losses.repulsion_radii(key[0], key[1:])
        return self._rep_radii

    def _repulsion_total(self, rep):
        """The four per-level values (0-dim tensors, or None for a level that is off) -> their unweighted sum; the values are kept
        in the trainer's 4-float buffer for `repulsion_state`."""
        vals = torch.stack([r if r is not None else self._rep_zero for r in rep])
        # (an elementwise launch, not copy_: a captured 16-byte copy_ is a memcpy node of a shape the launch list does not re-issue)
        torch.add(vals.detach(), self._rep_zero, out=self._rep_buf)
        return vals.sum()

    @staticmethod
    def _check_flatness(cfg):
        """{"weight", "k", "eps", "levels"} validated: weight finite and >= 0, k an integer in [1, 64], eps finite and >= 0, levels a
        non-empty ascending subset of (0, 1, 2, 3)."""
        if not isinstance(cfg, dict) or set(cfg) - {"weight", "k", "eps", "levels"} or "weight" not in cfg:
            raise ValueError("flatness: None or {'weight': w, 'k': 16, 'eps': e, 'levels': (0, 1, 2, 3)}, got %r" % (cfg,))
        weight, eps, k = float(cfg["weight"]), float(cfg.get("eps", 0.0)), cfg.get("k", 16)
        if not (0.0 <= weight < float("inf")):
            raise ValueError("flatness weight must be finite and not negative, got %r" % (cfg["weight"],))
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= losses.FLATNESS_MAX_K:
            raise ValueError("flatness k must be an integer from 1 to %d, got %r" % (losses.FLATNESS_MAX_K, k))
        if not (0.0 <= eps < float("inf")):
            raise ValueError("flatness eps must be finite and not negative, got %r" % (cfg.get("eps"),))
        levels = tuple(int(l) for l in cfg.get("levels", (0, 1, 2, 3)))
        if not levels or list(levels) != sorted(set(levels)) or levels[0] < 0 or levels[-1] > 3:
            raise ValueError("flatness levels: a non-empty ascending subset of (0, 1, 2, 3), got %r" % (cfg.get("levels"),))
        return {"weight": weight, "k": k, "eps": eps, "levels": levels}

    def set_flatness(self, weight=None, k=None, eps=None):
        """Change the flatness term.  weight: written INTO the loss-weight vectors -- the tensors a launch list has baked in: the next
        `step_list()` (or eager step) uses it, with no recapture.  k, eps: launch ARGUMENTS, so a captured list or graph keeps the ones
        it was captured with: raises while one exists.  Raises on a trainer built without `flatness`."""
        if self.flatness is None:
            raise RuntimeError("set_flatness(): this trainer was built without flatness; build it with one (e.g. weight 0.0)")
        fresh = self._check_flatness({"weight": self.flatness["weight"] if weight is None else weight,
                                      "k": self.flatness["k"] if k is None else k,
                                      "eps": self.flatness["eps"] if eps is None else eps, "levels": self.flatness["levels"]})
        if (fresh["k"], fresh["eps"]) != (self.flatness["k"], self.flatness["eps"]) and (
                getattr(self, "_list", None) is not None or getattr(self, "_graphs", None)):
            raise RuntimeError("set_flatness(k=..., eps=...): k and eps are arguments of the captured launches; capture again with the new ones")
        self.flatness = fresh
        with torch.no_grad():
            for w in self._lw.values():
                w[self._flat_at:self._flat_at + 1].fill_(fresh["weight"])

    def flatness_state(self):
        """{weight, k, eps, levels, floors, per_level, total, degenerate}: the parameters, the floor of each of the four levels for the
        last iteration's cloud sizes (None before the first), the last iteration's unweighted value per level (0 for a level that is
        not in `levels`) with their sum, and its number of degenerate points over the levels.  Synchronises the device."""
        if self.flatness is None:
            raise RuntimeError("flatness_state(): this trainer was built without flatness")
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        per = [float(v) for v in self._flat_buf.cpu()]
        return dict(self.flatness, floors=self.__dict__.get("_flat_floors"), per_level=per, total=float(sum(per)),
                    degenerate=int(sum(int(d.sum()) for d in self._flat_deg.values())))

    def _flatness_floors(self, sizes):
        """The four levels' floors for these point counts (cached: the same sizes every iteration)."""
        key = (self.flatness["eps"],) + tuple(int(n) for n in sizes)
        if self.__dict__.get("_flat_key") != key:
            self._flat_key, self._flat_floors = key, losses.flatness_floors(key[0], key[1:])
        return self._flat_floors

    def _flatness_level(self, level, cloud, floors):
        """Level l's term (0-dim, differentiable), or None where the level is off; the degenerate counts go to the level's own buffer."""
        if level not in self.flatness["levels"]:
            return None
        deg = self._flat_deg.get(level)
        if deg is None or deg.shape[0] != cloud.shape[0]:
            deg = self._flat_deg[level] = torch.zeros(cloud.shape[0], dtype=torch.int32, device=self.device)
        return losses.flatness(cloud, self.flatness["k"], eps=floors[level], degenerate=deg)

    def _flatness_total(self, flat):
        """As `_repulsion_total`: the four per-level values -> their unweighted sum, kept in the 4-float buffer for `flatness_state`."""
        vals = torch.stack([f if f is not None else self._flat_zero for f in flat])
        torch.add(vals.detach(), self._flat_zero, out=self._flat_buf)
        return vals.sum()

    def set_lr_schedule(self, knots):
        """Replace the schedule: the knots are validated and written INTO the trainer's table -- the same tensor at the same
        address, which the launch list has baked in: the next `step_list()` (or eager step) runs on the new schedule, with no
        recapture.  Raises on a trainer built without `lr_schedule` (it has no table, and its launches read none)."""
        if self.lr_table is None:
            raise RuntimeError("set_lr_schedule(): this trainer was built without an lr_schedule; build it with one (e.g. [(0, 1.0)])")
        fresh = _schedule.table(knots, "cpu")                    # validates; raises before the table is touched
        with torch.no_grad():
            self.lr_table.copy_(fresh)

    def set_augment(self, **changes):
        """Change augmentation parameters (augment.Augment's: p, rot_max_deg, scale_max, flip, trans_max, jitter_sigma, up_axis,
        flip_axis): validated, then written INTO the trainer's table -- the same tensor at the same address, which the launch list
        has baked in: the next `step_list()` (or eager step) draws with the new values, with no recapture.  Raises on a trainer
        built without `augment` (it has no table, and its launches read none).  Adaptive: also target,
        interval, span, p_min, p_max, written into the state record in place; p sets the current value."""
        if self.aug is None:
            raise RuntimeError("set_augment(): this trainer was built without augment; build it with one (e.g. augment={'p': 0.0})")
        self.aug.set(**changes)

    def aug_state(self):
        """{clock, params, records}: the number of iterations begun, the table as it is on the device (thresholds of 2^24, axes,
        ranges in radians / log-scale) and, with record=True, the (12, B, 12) affine maps of the last iteration (row 3 * network +
        role, role = real | fake | gen; per sample the 3 x 3 matrix row-major, then the translation); adaptive: also "ada"
        (augment.decode_ada).  Synchronises the device."""
        if self.aug is None:
            raise RuntimeError("aug_state(): this trainer was built without augment")
        return self.aug.state()

    def lr_state(self):
        """{network: {step, factor, lr}} for G, D1..D4: the count of the network's last applied update, the schedule's factor at
        that count (1.0 without a schedule) and the rate that update ran at, base * factor in fp64 -- the host evaluation
        (schedule.factor) of the table as it is on the device.  Before a network's first update: step 0 and the schedule at 0.
        Synchronises the device."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        tab = None if self.lr_table is None else self.lr_table.cpu()
        out = {}
        for key, opt in zip(self.GUARD_KEYS, [self.optG] + self.optD):
            g = opt.param_groups[0]
            st = opt.state.get(g["params"][0])
            step = float(st["step"]) if st and "step" in st else 0.0
            f = 1.0 if tab is None else _schedule.factor(tab, step)
            out[key] = {"step": int(step), "factor": f, "lr": float(g["lr"]) * f}
        return out

    @staticmethod
    def _flat_like(params):
        slot = lambda p: (p.numel() + 3) // 4 * 4
        buf = torch.zeros(sum(slot(p) for p in params), dtype=torch.float32, device=params[0].device)
        views, off = [], 0
        for p in params:
            views.append(buf[off:off + p.numel()].view_as(p))
            off += slot(p)
        return buf, views

    def _ema_from_parameters(self):
        """The averages start from the parameters as they are now (construction; a checkpoint without averages)."""
        if self.ema is not None:
            with torch.no_grad():
                torch._foreach_copy_(self.ema, [p.detach() for p in self.optG.param_groups[0]["params"]])

    @contextlib.contextmanager
    def averaged_generator(self):
        """`with trainer.averaged_generator():` -- inside, `trainer.G` computes with the averaged parameters (and its live
        BatchNorm buffers); afterwards the trained ones are back, bit for bit.  The swap is BY VALUE: the launch list has the
        parameters' addresses baked in, so the tensors stay where they are.  On entry the device is synchronised, the
        parameters are saved to a spare buffer and overwritten with the averages; on exit the saved values are copied back.
        The copies are torch's in-place ones, which bump the parameters' version counters: PointDeconv recognises stale
        pre-assembled operands by (data_ptr, _version), and a raw pdgn_copy_multi would leave operands of the OTHER weights
        looking current.  The pre-assembled operands are dropped on both sides anyway, and the forward hints are put back as
        the snapshot reports do.  Not for use between `capture` graphs' replays or inside a step."""
        if self.ema is None:
            raise RuntimeError("averaged_generator(): this trainer keeps no averaged generator (ema_decay=0)")
        params = self.optG.param_groups[0]["params"]
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        if self._ema_spare is None:
            self._ema_spare = self._flat_like(params)
        own = hasattr(self.G, "forward_hints")                   # (a caller's own generator module may keep no such state)
        hints = self.G.forward_hints() if own else None
        with torch.no_grad():
            torch._foreach_copy_(self._ema_spare[1], [p.detach() for p in params])
            torch._foreach_copy_(list(params), self.ema)
        if own:
            self.G.drop_preassembled()
        try:
            yield self.G
        finally:
            with torch.no_grad():
                torch._foreach_copy_(list(params), self._ema_spare[1])
            if own:
                self.G.drop_preassembled()
                self.G.restore_forward_hints(hints)

    def sync_replicas(self, src=0):
        """nn.DataParallel replicates module 0's parameters and buffers onto every device each forward
        (models/PDGNet_v2.py:101-105); with one process per GPU the replicas are made identical ONCE -- here, and
        after load() -- by broadcasting rank `src`'s parameters, buffers and Adam state; identical averaged gradients
        keep the parameters identical afterwards (BatchNorm running statistics stay per replica, as they do under
        DataParallel, where only replica 0's survive).  No-op in a single process."""
        if not (self.distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return
        with torch.no_grad():
            for net in [self.G] + self.D:
                flat = [t for t in list(net.parameters()) + list(net.buffers())]
                for dtype in sorted({t.dtype for t in flat}, key=str):   # same order on every rank
                    group = [t for t in flat if t.dtype == dtype]
                    buf = torch.cat([t.reshape(-1) for t in group])
                    dist.broadcast(buf, src)
                    off = 0
                    for t in group:
                        t.copy_(buf[off:off + t.numel()].view_as(t))
                        off += t.numel()
            for opt in [self.optG] + self.optD:
                for st in opt.state.values():
                    for v in st.values():
                        if torch.is_tensor(v):
                            dist.broadcast(v, src)
            if self.ema_buf is not None:
                dist.broadcast(self.ema_buf, src)
            if self.lr_table is not None:
                dist.broadcast(self.lr_table, src)

    def train(self):
        self.G.train()
        for d in self.D:
            d.train()

    # ---- checkpoints in the reference's own two-file format (models/PDGNet_v2.py:384-408 save, :331-382 load)
    @staticmethod
    def _ref_model_state(module):
        # the reference wraps every net in nn.DataParallel (:101-105): its files carry 'module.'-prefixed keys
        return {"module." + k: v.detach().cpu() for k, v in module.state_dict().items()}

    @staticmethod
    def _ref_optim_state(opt):
        sd = opt.state_dict()
        state = {}
        for i, st in sd["state"].items():
            # capturable/fused Adam keeps `step` as a device tensor; the reference's torch 1.7 Adam holds an int
            state[i] = {k: (int(v.item()) if k == "step" else v.detach().cpu()) if torch.is_tensor(v) else v
                        for k, v in st.items()}
        keep = ("lr", "betas", "eps", "weight_decay", "amsgrad", "params")
        groups = [{k: g[k] for k in keep} for g in sd["param_groups"]]
        return {"state": state, "param_groups": groups}

    def save(self, checkpoint_dir, index_epoch, category="chair"):
        """Writes `<epoch>_<category>_G.pth` / `_D.pth` with the reference's keys (:391-407) so that either code
        base can resume from the other's files.  With an averaged generator also `<epoch>_<category>_G_ema.pth`: G.pth's layout
        with the AVERAGED parameters under `G_model` (buffers: the live ones) plus `ema_decay`, so that either code base's
        `--phase test --pretrain_model_G <epoch>_<category>_G_ema.pth` evaluates the averaged generator; returned third.  With adaptive
        augmentation also `<epoch>_<category>_aug.pth` (augment.Augment.checkpoint: the state record, the slots, the table, the
        parameters); returned last.  G.pth / D.pth are what they were either way."""
        os.makedirs(checkpoint_dir, exist_ok=True)
        stem = os.path.join(checkpoint_dir, "%s_%s" % (index_epoch, category))
        held = hold_bn_counters(False)
        flush_bn_counters()
        hold_bn_counters(held)
        torch.save({"G_model": self._ref_model_state(self.G), "G_optimizer": self._ref_optim_state(self.optG),
                    "G_epoch": index_epoch}, stem + "_G.pth")
        dfile = {"D_epoch": index_epoch}
        for i, (d, o) in enumerate(zip(self.D, self.optD), 1):
            dfile["D_model%d" % i] = self._ref_model_state(d)
            dfile["D_optimizer%d" % i] = self._ref_optim_state(o)
        torch.save(dfile, stem + "_D.pth")
        extra = ()
        if self.aug is not None and self.aug.adaptive is not None:
            # p is state (it cannot be derived, unlike the clock): a sibling file, G.pth / D.pth stay what they were
            torch.save(self.aug.checkpoint(), stem + "_aug.pth")
            extra = (stem + "_aug.pth",)
        if self.ema is not None:
            model = self._ref_model_state(self.G)
            for (name, p), e in zip(self.G.named_parameters(), self._ema_in_module_order()):
                assert model["module." + name].shape == e.shape, name
                model["module." + name] = e.detach().cpu().clone()
            torch.save({"G_model": model, "G_optimizer": self._ref_optim_state(self.optG), "G_epoch": index_epoch,
                        "ema_decay": self.ema_decay}, stem + "_G_ema.pth")
            return (stem + "_G.pth", stem + "_D.pth", stem + "_G_ema.pth") + extra
        return (stem + "_G.pth", stem + "_D.pth") + extra

    def _ema_in_module_order(self):
        """The averages in `G.named_parameters()` order (they are kept in the optimizer's, which is the same list today)."""
        by_id = {id(p): e for p, e in zip(self.optG.param_groups[0]["params"], self.ema)}
        return [by_id[id(p)] for p in self.G.parameters()]

    @staticmethod
    def _load_optim(opt, sd):
        groups = []
        for mine, theirs in zip(opt.state_dict()["param_groups"], sd["param_groups"]):
            g = dict(mine)                                   # keep this build's capturable/fused/foreach flags
            g.update({k: theirs[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad") if k in theirs})
            groups.append(g)
        opt.load_state_dict({"state": sd["state"], "param_groups": groups})

    def load(self, path_G, path_D):
        """Resume from a reference (or own) checkpoint pair; returns the stored epoch (:352, :374).
        A missing file raises FileNotFoundError (the reference calls exit(), :345-347).  With an averaged generator: the
        averages come from the sibling `..._G_ema.pth` of `..._G.pth` where it exists, else they start from the loaded
        parameters; the warm-up of the decay needs no state of its own (it reads Adam's restored step count).  Adaptive augmentation:
        its state comes from the sibling `..._aug.pth` where it exists, else it stays as constructed."""
        from .generator import load_reference_state_dict
        g = torch.load(path_G, map_location="cpu")
        d = torch.load(path_D, map_location="cpu")
        load_reference_state_dict(self.G, g["G_model"])
        self._load_optim(self.optG, g["G_optimizer"])
        for i, (m, o) in enumerate(zip(self.D, self.optD), 1):
            load_reference_state_dict(m, d["D_model%d" % i])
            self._load_optim(o, d["D_optimizer%d" % i])
        for st in [self._stepG] + self._stepD:                   # the optimizers' state tensors are new objects now
            st.reset()
        if self.ema is not None:
            sibling = str(path_G)[:-len("_G.pth")] + "_G_ema.pth" if str(path_G).endswith("_G.pth") else None
            if sibling is not None and os.path.exists(sibling):
                avg = torch.load(sibling, map_location="cpu")["G_model"]
                avg = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in avg.items()}
                with torch.no_grad():
                    for (name, _), e in zip(self.G.named_parameters(), self._ema_in_module_order()):
                        e.copy_(avg[name])
            else:
                self._ema_from_parameters()
        if self.aug is not None and self.aug.adaptive is not None:
            sibling = str(path_G)[:-len("_G.pth")] + "_aug.pth" if str(path_G).endswith("_G.pth") else None
            if sibling is not None and os.path.exists(sibling):  # (else: the constructed state)
                self.aug.restore(torch.load(sibling, map_location="cpu"))
        self.sync_replicas()
        return g["G_epoch"]

    def _loss_weights(self, ws):
        """(1.2, 1.2, 1.2, 1, 0.1*ws): weights of the four adversarial terms and of the shape loss (:254); the shape loss
        is a batch SUM, so under data parallelism it is scaled by the world size before the mean all-reduce."""
        w = self._lw.get(ws)
        if w is None:                                            # created outside any graph capture (see __init__)
            base = [1.2, 1.2, 1.2, 1.0, 0.1 * ws]
            if self.repulsion is not None:                       # one more entry of the weighted sum: a batch mean, no world-size factor
                base.append(self.repulsion["weight"])
            if self.flatness is not None:                        # and one more: a batch mean as well
                self._flat_at = len(base)
                base.append(self.flatness["weight"])
            w = self._lw[ws] = torch.tensor(base, dtype=torch.float32, device=self.device)
        return w

    def _freeze_D(self, frozen):
        params = self.__dict__.get("_d_params")
        if params is None:                                       # (module.parameters() walks the module tree: 0.4 ms per call)
            params = self.__dict__["_d_params"] = [p for d in self.D for p in d.parameters()]
        for p in params:
            p.requires_grad_(not frozen)

    def similar_terms(self, clouds, pairs, own=None):
        """{(a, b): (like_mu, like_cov)} of get_local_pair (:232-237) for the given resolution pairs.  `own` caches
        the statistics of cloud a around itself across calls (they are shared by all pairs (a, .))."""
        terms, own = {}, ({} if own is None else own)
        for a, b in pairs:
            if a not in own:
                cl = clouds[a].transpose(1, 2).contiguous()
                own[a] = self.local_pair.stats(cl, cl)
            terms[(a, b)] = self.local_pair(clouds[a], clouds[b], self_stats=own[a])
        return terms

    @staticmethod
    def _sum_terms(terms):
        return torch.stack([terms[p][0] for p in PAIRS] + [terms[p][1] for p in PAIRS]).sum()

    def similar_loss(self, clouds):
        """Sum of the 6 like_mu and the 6 like_cov terms, in the reference's order (:251-252)."""
        return self._sum_terms(self.similar_terms(clouds, PAIRS))

    # The iteration is written as six SEGMENTS separated by the five gradient all-reduces, so that
    # each segment can be captured into a hipGraph (no RCCL call inside a capture) and replayed:
    #   0: G(z1) under no_grad (:179) + D1 forward/backward        -> all-reduce grad D1
    #   1..3: Adam D_i (:191) + D_{i+1} forward/backward           -> all-reduce grad D_{i+1}
    #   4: Adam D4 + G(z2), local-pair losses, D(gen), backward    -> all-reduce grad G
    #   5: Adam G (:256)
    def _seg_d(self, st, i):
        D, obj = self.D[i], self.gan_loss
        self.gradD[i].begin()
        if self.aug is None:
            lossD = losses.adversarial(D(st["reals"][i]), obj, "d_real") + losses.adversarial(D(st["fakes"][i]), obj, "d_fake")
        else:
            lossD = (losses.adversarial(D(st["reals"][i], self.aug.at(i, "real")), obj, "d_real", self._aug_counter(i))
                     + losses.adversarial(D(st["fakes"][i], self.aug.at(i, "fake")), obj, "d_fake"))
        lossD.backward()
        st["out"]["d_loss%d" % (i + 1)] = lossD.detach()

    def _aug_counter(self, i):
        """Adaptive augmentation: the slot D_i's REAL-batch term counts into; None otherwise.  The fake and the
        generator's terms never count."""
        return self.aug.counter(i) if self.aug is not None and self.aug.adaptive is not None else None

    # The same update in two halves (overlapped schedule): lossD = mse(D(real), 1) / 2 + mse(D(fake), 0) / 2 (:186-190) is
    # a sum of two terms that share nothing but the parameters, and the REAL term does not depend on the generator at all.
    # Its forward and backward are issued at the start of the iteration and run underneath generator pass #1 (whose first
    # three blocks are small kernels that leave the chip idle); when the fake cloud exists only the fake term's forward
    # and backward are left on the discriminator's chain, which was as long as the generator's own.
    # Same order of D's forward calls (real, then fake: BatchNorm running statistics), gradients summed once.
    def _seg_d_real(self, st, i):
        D = self.D[i]
        self.gradD[i].begin()
        params = self.gradD[i].params
        loss_r = losses.adversarial(D(st["reals"][i]) if self.aug is None else D(st["reals"][i], self.aug.at(i, "real")), self.gan_loss, "d_real", self._aug_counter(i))
        st["d_half"][i] = (loss_r.detach(), torch.autograd.grad(loss_r, params))

    def _seg_d_fake(self, st, i):
        D = self.D[i]
        fg = self.gradD[i]
        fg.resume()
        loss_f = losses.adversarial(D(st["fakes"][i]) if self.aug is None else D(st["fakes"][i], self.aug.at(i, "fake")), self.gan_loss, "d_fake")
        loss_r, g_real = st["d_half"][i]
        st.setdefault("keep", []).append(loss_r)            # (it may have been computed on another stream than this half runs on: it must
                                                            #  not return to that stream's pool before the sum below has RUN)
        g_fake = torch.autograd.grad(loss_f, fg.params)
        torch._foreach_add_(g_real, g_fake)
        for p, g in zip(fg.params, g_real):
            p.grad = g
        st["d_half"][i] = None
        st["out"]["d_loss%d" % (i + 1)] = loss_r + loss_f.detach()

    def _segment(self, st, k):
        if k == 0:
            if self.aug is not None:
                self.aug.tick()                                  # the iteration's draws: every discriminator call below reads this clock
            # generator pass #1 (:179): only its detached outputs are ever used => no graph needed;
            # BatchNorm running statistics update exactly as in the reference.
            with torch.no_grad():
                st["fakes"] = self.G(self._z(st, "z1"))
            self._seg_d(st, 0)
        elif k in (1, 2, 3):
            self._stepD[k - 1].step()
            self._seg_d(st, k)
        elif k == 4:
            self._stepD[3].step()
            self.gradG.begin()
            # The reference lets lossG.backward() also fill the discriminators' .grad and throws
            # that away at the next zero_grad (:183); freezing D skips those weight-gradient GEMMs.
            self._freeze_D(True)
            gen = self.G(self._z(st, "z2"))
            similar = self.similar_loss(gen)
            g_loss = [losses.adversarial(self.D[i](gen[i]) if self.aug is None else self.D[i](gen[i], self.aug.at(i, "gen")), self.gan_loss, "g") for i in range(4)]
            adv = 1.2 * g_loss[0] + 1.2 * g_loss[1] + 1.2 * g_loss[2] + g_loss[3]
            if self.repulsion is not None:
                radii = self._repulsion_radii([c.shape[2] for c in gen])
                rep = self._repulsion_total([losses.repulsion(gen[l], radii[l]) if l in self.repulsion["levels"] else None for l in range(4)])
                adv = adv + self._lw[1][5] * rep                 # (the weight as the device holds it: set_repulsion reaches a captured graph)
                st["out"]["repulsion_loss"] = rep.detach()
            if self.flatness is not None:
                floors = self._flatness_floors([c.shape[2] for c in gen])
                flat = self._flatness_total([self._flatness_level(l, gen[l], floors) for l in range(4)])
                adv = adv + self._lw[1][self._flat_at] * flat    # (the weight as the device holds it, as above)
                st["out"]["flatness_loss"] = flat.detach()
            lossG = adv + 0.1 * similar
            # MSE is a batch MEAN, the shape loss a batch SUM (chamfer_loss.py:16-20): to reproduce
            # one reference step at the global batch, scale the sum term by world_size before the
            # mean all-reduce.
            ws = st["ws"]
            (adv + (0.1 * ws) * similar if ws > 1 else lossG).backward()
            self._freeze_D(False)
            st["out"]["g_loss"], st["out"]["similar_loss"] = lossG.detach(), similar.detach()
        else:
            self._stepG.step()

    def _z(self, st, name):
        """Noise of a generator pass: the caller's tensor, or -- when it is None -- drawn on the
        device inside the step (z ~ N(0, 0.2^2), :178/:228), which keeps a captured iteration free
        of host-side inputs."""
        z = st[name]
        return z if z is not None else torch.randn(st["B"], 128, device=self.device) * 0.2

    def _comm(self, k):
        """Collective that follows segment k (RCCL all-reduce of one flat gradient buffer)."""
        if self.distributed and k < 5:
            fg = self.gradD[k] if k < 4 else self.gradG
            fg.pack()
            fg.all_reduce_mean()

    def _state(self, reals, z1, z2):
        B = reals[0].shape[0]
        return {"reals": reals, "z1": z1, "z2": z2, "B": B, "out": {}, "ws": world_size() if self.distributed else 1}

    def step(self, reals, z1, z2):
        """reals: four tensors (B,3,N_k); z1 / z2: noise (B,128) of the two generator passes
        (:178, :228).  Returns dict of 0-dim device tensors (no host sync inside the step)."""
        _warn_if_deterministic("step")
        if self.overlap:
            return self._step_overlapped(reals, z1, z2)
        st = self._state(reals, z1, z2)
        for k in range(6):
            self._segment(st, k)
            self._comm(k)
        release_zero_arena()
        return st["out"]

    def _step_overlapped(self, reals, z1, z2, st=None):
        """Same iteration, scheduled for the GPU: the four discriminator updates are independent of each other
        and of everything the generator does after emitting their resolution, and they are chains of small
        kernels (D1-D3 see 256-1024 points) that leave most CUs idle.  D_k's update (forward real + fake,
        backward, all-reduce, Adam) is enqueued on its own HIP stream the moment G(z1) has produced level k,
        so it runs underneath the deeper levels' GEMMs / gather-sums; D4's runs underneath G(z2).  In the same
        way D_k(G(z2)_k) (behind D_k's update, on D_k's stream) and the loss pairs that end at level k start from
        G(z2)'s stage hook; the default stream joins all of them before the backward.  Results are those of the
        sequential order (the reference's D updates do not read each other)."""
        # num_batches_tracked: the iteration's increments in one launch at its end (fused.hold_bn_counters)
        held_counts = hold_bn_counters(True)
        try:
            return self._step_overlapped_body(reals, z1, z2, st)
        finally:
            hold_bn_counters(held_counts)
            flush_bn_counters()

    def _step_overlapped_body(self, reals, z1, z2, st=None):
        st = st if st is not None else self._state(reals, z1, z2)
        main = torch.cuda.current_stream(self.device)
        pl = _streams.plan(self.device)                     # streams by measured hardware queue (streams.py)
        self._side, self._side_lp = pl.d, pl.lp
        st["fakes"] = [None] * 4
        st["keep"] = []
        mark = st.get("mark") or (lambda name: None)        # tools/phase_events.py: HIP events on the default stream
        mark("start")
        if st.get("tag_streams"):
            # capture for a launch list (capture_list): a captured graph does not say which stream a node was recorded
            # on, so every stream of the schedule opens with a marker node carrying its id (csrc/replay.hip)
            from . import replay as _replay
            _replay.mark(_replay.MAIN, main)
        if self.aug is not None:
            # The augmentation clock ticks once, HERE: on the issuing stream, before any side stream forks from it (each of them waits
            # for `main` before its first launch of the iteration), and behind the previous iteration, whose chains were all joined
            # into this stream at its end -- so every discriminator launch of this iteration, on whichever stream, reads this value.
            self.aug.tick()
        if st.get("tag_streams"):
            for sid, s in enumerate(list(pl.d) + [pl.lp, pl.knn], 1):
                s.wait_stream(main)
                _replay.mark(sid, s)

        # D_k's update starts on the DEVICE when level k exists (an event recorded in the stage hook), but its ~150
        # launches are issued by the host only after the whole generator pass has been issued: with a host that runs
        # ahead (steady state) the device sees the same schedule, and right after a synchronise -- the first timed step
        # of a benchmark, the first step after a checkpoint -- the default stream is not left idle while the host
        # works through three discriminator updates between the generator's blocks (G(z1) forward of such a step:
        # 15-25 ms before).
        levels = []

        def d_mark(level, cloud):
            st["fakes"][level] = cloud
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            levels.append((level, ev))
            if level < 3:
                mark("G(z1) level %d" % (level + 1))

        split = self._split_d

        def d_update(level, ev):
            side = self._side[level]
            side.wait_event(ev)
            with torch.cuda.stream(side), torch.enable_grad():
                if split:
                    self._seg_d_fake(st, level)
                else:
                    self._seg_d(st, level)
                self._comm(level)
                self._stepD[level].step()

        # The generator's re-associated GEMM operands (and, on the bf16 matrix cores, their pre-split planes) depend on the
        # parameters only: built once for both passes, with grad enabled -- pass #2's backward reaches the conv weights through
        # them.  (On the issuing stream: built on the idle kNN stream behind an event the iteration faulted at B = 35 --
        # the adjoint of the assembly then runs on that stream too -- and the four launches are ~60 us.)
        # Under data parallelism with the early gradient bucket the DEEPEST block's operands are pre-assembled for pass #1
        # only (no graph): pass #2 assembles them inside its forward, so that the adjoint of that assembly -- the conv
        # weights' gradients, 69 % of the early bucket -- runs right behind the block's backward instead of at the very end
        # (autograd orders ready nodes by creation: a node made before the forward goes last).
        pre_ok = hasattr(self.G, "preassemble") and os.environ.get("PDGN_PREASM", "1") == "1"
        if pre_ok:
            with torch.enable_grad():
                self.G.preassemble(deepest_without_graph=self.distributed and self._buckets)
        # (Rule for anything added to this schedule: a side stream may wait for events of the ISSUING stream only.  hipStreamEndCapture
        # (ROCm 7.2) recurses without bound -- a segmentation fault inside hip::Stream::EndCapture -- as soon as one captured side stream
        # waits for an event recorded on ANOTHER side stream; round 6 ran pass #1 on D4's stream beside pass #2 that way and routed
        # every dependency through the issuing stream.  It measured slower -- the iteration is bound by the sum of its kernels -- and
        # is in git at 5c84567 (trainer.py, PDGN_PASS1_SIDE))
        if split:
            st["d_half"] = [None] * 4
            for level, side in enumerate(self._side):
                side.wait_stream(main)                      # (the real batch / targets may have been produced on `main`)
                with torch.cuda.stream(side), torch.enable_grad():
                    self._seg_d_real(st, level)

        def d_now(level, cloud):
            d_mark(level, cloud)
            d_update(*levels.pop())

        hook1 = d_mark if self._defer_d else d_now
        with torch.no_grad():
            self.G(self._z(st, "z1"), stage_hook=hook1)
        for level, ev in levels:
            d_update(level, ev)
        mark("G(z1) level 4")
        self.gradG.begin()
        self._freeze_D(True)
        # The shape-preserving loss (12 kNN + Chamfer terms) and the four D(gen) passes read the clouds and nothing of
        # each other: they run on their own streams, forward and (autograd keeps an op's backward on its forward's
        # stream) backward.  They also do not need the whole forward: pair (a, k) and D_k(gen_k) only need level k, so
        # they are enqueued from the generator's stage hook and run underneath the deeper blocks; after the forward
        # only D4(gen) and the three pairs with the 2048-point cloud are left to wait for.  Being created last, those
        # are also the first adjoints autograd issues -- the ones block 4's backward waits for.
        terms, own, g_loss, gen_so_far = {}, {}, [None] * 4, []
        early = self._early_tail
        rep, rep_on = [None] * 4, self.repulsion is not None
        # (the levels arrive one at a time; the generator's clouds have the real batch's point counts -- D_k sees both)
        radii = self._repulsion_radii([r.shape[2] for r in st["reals"]]) if rep_on else None
        flat, flat_on = [None] * 4, self.flatness is not None
        floors = self._flatness_floors([r.shape[2] for r in st["reals"]]) if flat_on else None

        def repel(level, cloud):                            # level l's all-pairs launch, on the local-pair stream (which has waited for `main`)
            if level in self.repulsion["levels"]:
                rep[level] = losses.repulsion(cloud, radii[level])

        def d_gen(level, cloud):                            # D_k(G(z2)_k) behind D_k's update, on D_k's stream
            side = self._side[level]
            side.wait_stream(main)
            with torch.cuda.stream(side):
                g_loss[level] = losses.adversarial(self.D[level](cloud) if self.aug is None else self.D[level](cloud, self.aug.at(level, "gen")), self.gan_loss, "g")

        def tail(level, cloud):
            gen_so_far.append(cloud)
            if level >= 1 or rep_on or flat_on:
                self._side_lp.wait_stream(main)
                with torch.cuda.stream(self._side_lp):
                    if level >= 1:
                        terms.update(self.similar_terms(gen_so_far, [(a, level) for a in range(level)], own))
                    if rep_on:
                        repel(level, cloud)
                    if flat_on:                             # level l's neighbour search and flatness launches, on the same stream
                        flat[level] = self._flatness_level(level, cloud, floors)
            d_gen(level, cloud)

        gen = self.G(self._z(st, "z2"), stage_hook=tail if early else None)
        mark("G(z2) forward")
        if not early:
            self._side_lp.wait_stream(main)
            with torch.cuda.stream(self._side_lp):
                terms = self.similar_terms(gen, PAIRS)
                if rep_on:
                    for level in range(4):
                        repel(level, gen[level])
                if flat_on:
                    for level in range(4):
                        flat[level] = self._flatness_level(level, gen[level], floors)
            for i, side in enumerate(self._side):
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    g_loss[i] = losses.adversarial(self.D[i](gen[i]) if self.aug is None else self.D[i](gen[i], self.aug.at(i, "gen")), self.gan_loss, "g")
        for side in self._side:
            main.wait_stream(side)
        main.wait_stream(self._side_lp)
        mark("wait: D(gen) + local-pair forward")
        similar = self._sum_terms(terms)
        # 1.2*(g1+g2+g3) + g4 + 0.1*similar (:254) as one weighted sum: this sits between the joins and the backward,
        # where every launch is on the critical path (three launches here and one in backward instead of eight and five)
        ws = st["ws"]
        if rep_on:                                          # one more entry of the weighted sum; its weight is the vector's last element
            repulsion = self._repulsion_total(rep)
            st["out"]["repulsion_loss"] = repulsion.detach()
        if flat_on:                                         # and one more, behind it
            flatness = self._flatness_total(flat)
            st["out"]["flatness_loss"] = flatness.detach()
        terms = torch.stack(g_loss + [similar] + ([repulsion] if rep_on else []) + ([flatness] if flat_on else []))
        lossG = (terms * self._loss_weights(1)).sum()
        (lossG if ws == 1 else (terms * self._loss_weights(ws)).sum()).backward()
        mark("backward")
        self._freeze_D(False)
        st["out"]["g_loss"], st["out"]["similar_loss"] = lossG.detach(), similar.detach()
        self._comm(4)
        self._stepG.step()
        if pre_ok:
            self.G.drop_preassembled()
        release_zero_arena()                                # no later backward may receive slices of this step's arena
        mark("all-reduce + Adam G")
        return st["out"]

    # ---------------------------------------------------------------- hipGraph replay
    def capture(self, reals, z1=None, z2=None, warmup=3):
        """Capture the iteration into hipGraphs (static input buffers, one shared memory pool):
        ~2500 kernel launches become one graph launch (six when gradients are all-reduced
        between segments).  (Drawing the noise on the device inside the capture is not used: a
        captured torch.randn faulted on this ROCm build.)

        ROCm 7.2 note (measured on MI355X): an eager kernel enqueued between two graph launches
        on the same stream is NOT reliably ordered against them (replays with `copy_` of the
        inputs in between fault, the same replays with a stream synchronise around the copies,
        or with no eager work in between, are clean) -- hence `_sync()` around every eager
        operation that sits between replays."""
        self._static = self._state([r.clone() for r in reals], z1.clone() if z1 is not None else None,
                                   z2.clone() if z2 is not None else None)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                for k in range(6):
                    self._segment(self._static, k)
                    self._comm(k)
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        # One graph per run of segments between collectives: the whole iteration when there is
        # nothing to all-reduce, six graphs (replayed with the all-reduces between them) otherwise.
        groups = [[k] for k in range(6)] if self.distributed else [list(range(6))]
        self._graphs, pool = [], None
        if self.overlap and not self.distributed:
            # the stream-overlapped schedule as ONE graph: the side streams fork from / join the capturing stream
            g = torch.cuda.CUDAGraph()
            defer, self._defer_d = self._defer_d, False       # capture order = node order of the replay: keep D_k's
            try:                                              # nodes next to the level that feeds them
                with torch.cuda.graph(g):
                    self._step_overlapped(None, None, None, st=self._static)
            finally:
                self._defer_d = defer
            self._graphs.append((g, 5))
            release_zero_arena()                            # the arena of the capture lives in the graph's private pool
            return self
        for group in groups:
            g = torch.cuda.CUDAGraph()
            # thread_local: with a communicator alive its watchdog thread polls events (hipEventQuery) at any time; under
            # the default "global" capture mode such a call from ANOTHER thread invalidates the capture (and surfaced as an
            # abort when the process group was destroyed, one run in four)
            with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
                for k in group:
                    self._segment(self._static, k)
            pool = g.pool()
            self._graphs.append((g, group[-1]))
            self._comm(group[-1])
        release_zero_arena()
        return self

    # ---------------------------------------------------------------- launch-list replay (csrc/replay.hip)
    def capture_list(self, reals, z1, z2, warmup=2):
        """Record the stream-overlapped iteration ONCE (stream capture into a hipGraph that is kept but never instantiated)
        and turn it into a launch list: `step_list` then re-issues the same ~1300 launches with plain HIP calls on the
        streams the eager schedule uses -- ~4 us of host time per launch instead of ~20 (autograd nodes, allocations,
        ctypes), and none of hipGraphLaunch's own scheduling (slower than eager here).
        Data parallel: a collective cannot be captured, so every gradient all-reduce -- D_k's on D_k's stream, the generator's
        early bucket from inside the backward, the rest behind it -- is recorded as a HOST POINT (a marker node, replay.Recorder):
        `step_list` issues the list in ranges and makes the RCCL calls between them, on the streams and at the places of the
        eager schedule (packing, the division by the world size and the optimizer steps are ordinary captured launches).
        The `warmup` iterations are real optimizer updates."""
        from . import replay
        if not self.overlap:
            raise RuntimeError("capture_list: stream-overlapped schedule only")
        _warn_if_deterministic("capture_list")
        self._static = self._state([r.clone() for r in reals], z1.clone(), z2.clone())
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup):                          # allocator pools, the optimizers' lean lists, arena sizes
                self._step_overlapped(None, None, None, st=self._state(self._static["reals"], self._static["z1"], self._static["z2"]))
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        if self.distributed and dist.is_available() and dist.is_initialized():
            # The process group's watchdog thread polls the completion events of the collectives it still lists (every 100 ms).
            # Such a poll while this thread captures ends the process (measured on ROCm 7.2: "operation not permitted on an
            # event last recorded in a capturing stream", one capture in three): the warm-up's collectives are complete after
            # the synchronise above -- give the watchdog its next rounds to drop them, so that it holds nothing during the capture.
            #   What is deterministic is done first: every Work handle this trainer still holds has been waited for and is
            # dropped (a step ends with `_early_work = None`: FlatGrads.all_reduce_mean), the device is idle (the synchronise above),
            # so every collective the watchdog lists is COMPLETE and it removes them on its next pass -- which nothing in the public
            # API lets this thread observe or force.  The wait below therefore depends on the watchdog's poll period (100 ms in
            # torch 2.10): five periods by default, PDGN_CAPTURE_QUIESCE_S to change it.  The failure mode is an abort inside the
            # watchdog thread, not an exception: there is no fallback to fall back to, which is why the margin is 5x.
            for fg in (self.gradG, *self.gradD):
                if getattr(fg, "_early_work", None) is not None:
                    fg._early_work.wait()
                    fg._early_work = None
            import time
            time.sleep(float(os.environ.get("PDGN_CAPTURE_QUIESCE_S", "0.5")))
        g = torch.cuda.CUDAGraph(keep_graph=True)            # the recorded graph is read back, never launched
        defer, self._defer_d = self._defer_d, False           # capture order = issue order of the replay: D_k's launches
        self._static["tag_streams"] = True                   # next to the level that feeds them
        rec = replay.Recorder()
        try:
            with rec, torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._step_overlapped(None, None, None, st=self._static)
        finally:
            self._defer_d = defer
            self._static.pop("tag_streams", None)
        release_zero_arena()                                # the capture's arena lives in the graph's private pool
        self._list = replay.LaunchList(g)
        if len(self._list.points) != len(rec.fns):
            raise RuntimeError("capture_list: %d host points recorded, %d found in the list" % (len(rec.fns), len(self._list.points)))
        self._list_points = [(pos, rec.fns[i], label) for pos, i, label in self._list.points]
        # the iteration's last launch on the issuing stream must be behind everything else (the next iteration's input copies and
        # the caller's reads of the losses are ordered against THAT stream only): every chain's last node must reach it
        info = self._list.info
        if info["chains"] != info["labelled"] or not self._list.joined:
            raise RuntimeError("capture_list: %d chains, %d tagged, joined=%s: a launch on an untagged stream, or a side stream whose "
                               "last launch the issuing stream never waits for" % (info["chains"], info["labelled"], self._list.joined))
        self._list_spare = [torch.cuda.Stream(device=self.device) for _ in range(2)]
        self._list_done = None
        self._list_pace = float(os.environ.get("PDGN_LIST_PACE", "1.0"))     # 1.0: the previous iteration's end
        return self

    def step_list(self, reals=None, z1=None, z2=None):
        """One iteration from the launch list of `capture_list`.  Inputs, when given, are copied into the static buffers
        first (ordinary launches on the current stream: plain stream order, no synchronisation needed)."""
        from . import replay
        st = self._static
        if reals is not None:
            for d, s in zip(st["reals"], reals):
                if d.data_ptr() != s.data_ptr():
                    d.copy_(s)
        if z1 is not None:
            st["z1"].copy_(z1)
            st["z2"].copy_(z2)
        pl = _streams.plan(self.device)                      # the eager schedule's streams for the current stream
        streams = {replay.MAIN: torch.cuda.current_stream(self.device), replay.LP: pl.lp, replay.KNN: pl.knn}
        for i, s in enumerate(pl.d):
            streams[replay.D0 + i] = s
        self._list.bind(streams, self._list_spare)
        # One iteration in flight: the list is issued in ~5 ms, the device needs ~6x that.  A host that runs several
        # iterations ahead fills the runtime's queues, blocks inside a launch for ONE stream and starves the others
        # (measured: 30.5 ms/step unbounded, 30.7 with two iterations in flight, 29.2 with one; the eager host's 25 ms
        # per iteration paced it by accident).  The wait is on an event recorded after `_list_pace` of the issuing stream's
        # launches of the previous iteration: 1.0 (the default, the measured best) = its end.
        if self._list_done is not None:
            self._list_done.synchronize()
        cut = self._list.position(replay.MAIN, self._list_pace)
        # the list in ranges: [.. cut) | pacing event | .. and, under data parallelism, every host point's collective behind the
        # range that ends with its marker, on the stream the marker was recorded on
        stops = sorted([(cut, 0, None, None)] + [(pos + 1, 1, fn, label) for pos, fn, label in self._list_points], key=lambda t: t[:2])
        lo = 0
        for at, kind, fn, label in stops:
            if at > lo:
                self._list.launch(lo, at)
                lo = at
            if kind == 0:
                if self._list_done is None:
                    self._list_done = torch.cuda.Event()
                self._list_done.record(streams[replay.MAIN])
            else:
                with torch.cuda.stream(streams[label]):
                    fn()
        self._list.launch(lo)
        return st["out"]

    # ---------------------------------------------------------------- the training loop (models/PDGNet_v2.py:157-269)
    LOG_FORMAT, LOSS_KEYS = _fit.LOG_FORMAT, _fit.LOSS_KEYS

    def fit(self, feeder, epochs, start_epoch=1, snapshot=20, checkpoint_dir=None, category="chair", issue="list", log=None,
            on_epoch=None, guard_max_skips=50, grad_norms=None, lr_log=None, aug_log=None, repulsion_log=None, flatness_log=None):
        """PDGNet_v2.train (:157-269): epochs start_epoch .. epochs over `feeder` (data.BatchFeeder: `batches_per_epoch` and
        `fill(epoch, i, reals, z1, z2)`), a checkpoint every `snapshot` epochs and after the last one (:266-268; rank 0 writes
        them), one log line per iteration in the reference's format (:259).  Returns the last epoch.  Resuming: pass what
        `load` returned as start_epoch -- the reference starts AT the stored epoch (:158-160), and the feed of an epoch is a
        pure function of (seed, epoch, batch), so the resumed epoch sees the batches an uninterrupted run saw.

        issue="list": the feeder writes into the static buffers of `capture_list` and `step_list()` runs without arguments --
        one launch and no torch op in front of the list.  The list is captured on first use from the first batch (its
        warm-up iterations are real optimizer updates on that batch).  issue="eager": trainer-owned buffers and `step`.
        The losses stay on the device: every iteration stacks them and copies them, non-blocking, into one of two pinned host
        rows; the line of iteration n is written after iteration n + 1 has been issued, when that copy is long complete.
        log: a callable taking the line, or a path (appended to); on_epoch: called with the epoch number after each epoch.

        With a gradient guard the five records travel with the losses, in the same pinned rows behind the
        same events, every iteration (also without a log).  The log line stays the reference's; `grad_norms` (a path; default:
        grad_norms.csv beside a log given as a path, else none) gets one row per iteration: epoch, iter, norm and coef of G, D1..D4,
        and the total number of skipped updates so far.  After `guard_max_skips` consecutive iterations in which some one network
        skipped its update, a checkpoint of the current epoch is written (checkpoint_dir given, rank 0) and GradGuardError raised:
        the parameters are the last finite ones (the guard's counters are not part of a checkpoint).  Once a network is one skip
        short of that, the line of an iteration is awaited right behind it instead of one iteration later, so that no further
        iteration is issued.

        With a learning-rate schedule or per-network rates, `lr_log` (a path; default: lr.csv beside a log
        given as a path, else none) gets one row -- epoch, step_G, lr_G, lr_D1 .. lr_D4, from `lr_state()` -- wherever a checkpoint is
        written or `on_epoch` is called: points at which the host waits for the device anyway.  Rank 0 only; without either, no file.

        With augmentation the clock is set to (start_epoch - 1) * batches_per_epoch behind any capture_list
        warm-up: iteration i of epoch e draws at (e - 1) * nb + i, whether the run was interrupted or not.  The clock is derived,
        not stored: checkpoints are what they were.  With ADAPTIVE augmentation (section 7i) `aug_log` (a path; default: aug.csv beside a
        log given as a path, else none) gets one row -- epoch, clock, p, updates, last_r, r_D1 .. r_D4 (the last update's (pos - neg) / n
        per discriminator) -- wherever lr.csv would get one.  Rank 0 only; without adaptive augmentation, no file.

        With the repulsion term `repulsion_log` (a path; default: repulsion.csv beside a log given as a path, else
        none) gets one row per EPOCH -- epoch, weight, radius, total, level1 .. level4: `repulsion_state()` after the epoch's last
        iteration, one synchronise per epoch.  Rank 0 only; without the term, no file and no synchronise.

        With the flatness term `flatness_log` (default: flatness.csv beside a log given as a path) gets one row per
        EPOCH in the same way -- epoch, weight, k, eps, total, level1 .. level4, degenerate: `flatness_state()`."""
        return _fit.fit(self, feeder, epochs, start_epoch, snapshot, checkpoint_dir, category, issue, log, on_epoch, guard_max_skips,
                        grad_norms, lr_log, aug_log, repulsion_log, flatness_log)

    def _sync(self):
        torch.cuda.current_stream(self.device).synchronize()

    def step_graphed(self, reals=None, z1=None, z2=None):
        """Replay of `capture`.  Inputs, when given, are copied into the static buffers first."""
        st = self._static
        copies = []
        if reals is not None:
            copies += [(d, s) for d, s in zip(st["reals"], reals) if d.data_ptr() != s.data_ptr()]
        if z1 is not None and st["z1"] is not None:
            copies += [(st["z1"], z1), (st["z2"], z2)]
        if copies:
            self._sync()
            for d, s in copies:
                d.copy_(s)
            self._sync()
        for g, last in self._graphs:
            g.replay()
            if self.distributed and last < 5:
                self._sync()
                fg = self.gradD[last] if last < 4 else self.gradG
                fg._early_work, fg._early_done = None, False        # begin() is captured Python: it does not re-run
                self._comm(last)
                self._sync()
        return st["out"]


def synthetic_batch(B, device, seed=9999, n_points=2048, resolutions=(256, 512, 1024, 2048)):
    """ShapeNet-shaped synthetic real clouds: (B,2048,3) ~ N(0,1),
    per-shape `shape_unit` normalisation (datasets_4point.py:335-337, :353), sub-resolutions
    drawn WITH replacement (:374-379), transposed to (B,3,N) (:184)."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(B, n_points, 3, generator=g)
    pts = (pts - pts.mean(dim=1, keepdim=True)) / pts.reshape(B, -1).std(dim=1).view(B, 1, 1)
    reals = []
    for r in resolutions:
        if r == n_points:
            sub = pts
        else:
            sel = torch.randint(0, n_points, (B, r), generator=g)
            sub = torch.gather(pts, 1, sel.unsqueeze(2).expand(B, r, 3))
        reals.append(sub.transpose(1, 2).contiguous().to(device))
    return reals


def noise(B, device, generator=None):
    """z ~ N(0, 0.2^2), (B,128) (:178, :228)."""
    return (torch.randn(B, 128, generator=generator) * 0.2).to(device)
