"""Discriminator augmentation (csrc/augment.hip): every cloud a discriminator sees -- real, generated, and the
generator's own pass through it -- goes through a fresh random similarity transform (flip, rotation about the up axis, isotropic
scale, translation) plus optional per-point jitter, drawn on the device and differentiable, so nothing of it leaks into the
generator (DiffAugment, Zhao et al. 2020; ADA, Karras et al. 2020).  The kernel that applies it writes the (B*N, 3) rows
`PointDiscriminator.forward` starts from: for a real batch it takes the place of that forward's transpose copy; a generated cloud is
a (B,3,N) view of point-major rows, read as it lies -- one launch where torch needed none, and one more in the generator's backward.

`Augment` owns the device state: the parameter table (64 bytes; `set` overwrites it in place, so a captured launch list follows),
the clock (one 64-bit word, advanced by `tick()` -- one small launch per iteration -- and read by the kernels themselves), and
with record=True a (12, B, 12) buffer into which every call site writes the affine map it used.  The draws are a pure function
of (seed, clock, global row, call site): include/pdgn_hip.h has the layout, tests/augment_mirror.py the numpy restatement.

The clock counts the iterations BEGUN; the launches of the iteration in flight draw at t = clock - 1.  `set_clock(c)` therefore
means "the next iteration draws at t = c", and after it the clock reads c + 1.

adaptive={...} (ADA, Karras et al. 2020): p is steered on the device.  The real-batch loss terms count D_i's
scores above and below the decision boundary 0.5 into `slots` (int32[16], `counter(i)`), and `tick()` -- pdgn_augment_tick_ada in
place of pdgn_augment_tick -- folds them into `ada` (pdgn_ada_state, 40 64-bit words) and every `interval` iterations moves the
thresholds one integer step towards r = (POS - NEG) / N = target.  tests/ada_mirror.py is the numpy restatement."""
import math

import numpy as np
import torch

from . import _lib
from ._fn import Function

ROLES = ("real", "fake", "gen")                                  # D's update on the data, D's update on G(z1), G's own pass through D
NETWORKS = 4
TAG_BASE = 16                                                    # PDGN_AUG_TAG_BASE: the feeder's tags are 0 .. 5 (include/pdgn_hip.h)
TABLE_WORDS = 16
# The defaults, chosen once (the command line's too): mirror and full rotation about the up axis cost a shape nothing (ShapeNet's
# shapes are upright, y up, and left/right symmetric as a class), scale and shift stay small against the unit-normalised clouds
# (shape_unit: extent ~1), jitter is off -- it is the one component that changes a cloud's local statistics.
DEFAULTS = dict(p=0.5, rot_max_deg=180.0, scale_max=1.25, flip=True, trans_max=0.1, jitter_sigma=0.0, up_axis=1, flip_axis=0)


def site_index(network, role):
    """0 .. 11: the row of the record buffer, and tag - TAG_BASE, of discriminator `network` (0 .. 3 = D1 .. D4) in `role`."""
    if not (isinstance(network, (int, np.integer)) and 0 <= network < NETWORKS):
        raise ValueError("network: 0 .. 3 (D1 .. D4), got %r" % (network,))
    if role not in ROLES:
        raise ValueError("role: one of %s, got %r" % (ROLES, role))
    return 3 * int(network) + ROLES.index(role)


def site_tag(network, role):
    return TAG_BASE + site_index(network, role)


def validate(p, rot_max_deg, scale_max, flip, trans_max, jitter_sigma, up_axis, flip_axis):
    """The parameters as a dict of plain Python values, or ValueError.  p in [0, 1]; rot_max_deg, trans_max, jitter_sigma finite and
    not negative (rot_max_deg at most 180); scale_max finite and at least 1; axes in 0 .. 2; with flip on, flip_axis != up_axis (a
    rotation about the up axis and a mirror THROUGH it would turn shapes upside down)."""
    def number(name, v, lo, hi=None):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number, got %r" % (name, v)) from None
        if not math.isfinite(f) or f < lo or (hi is not None and f > hi):
            raise ValueError("%s must be finite and %s, got %r" % (name, ("in [%g, %g]" % (lo, hi)) if hi is not None else ("at least %g" % lo), v))
        return f
    out = {"p": number("p", p, 0.0, 1.0), "rot_max_deg": number("rot_max_deg", rot_max_deg, 0.0, 180.0),
           "scale_max": number("scale_max", scale_max, 1.0), "flip": bool(flip), "trans_max": number("trans_max", trans_max, 0.0),
           "jitter_sigma": number("jitter_sigma", jitter_sigma, 0.0)}
    for name, a in (("up_axis", up_axis), ("flip_axis", flip_axis)):
        if not (isinstance(a, (int, np.integer)) and not isinstance(a, bool) and 0 <= a <= 2):
            raise ValueError("%s must be 0, 1 or 2, got %r" % (name, a))
        out[name] = int(a)
    if out["flip"] and out["flip_axis"] == out["up_axis"]:
        raise ValueError("flip_axis must differ from up_axis (%d): the mirror goes through a horizontal axis" % out["up_axis"])
    return out


ADA_DEFAULTS = dict(target=0.6, interval=4, span=500_000, p_min=0.0, p_max=0.8)     # (Karras et al. 2020: r_t target 0.6, every 4 minibatches, 500 k images)
ADA_WORDS, ADA_SLOT_WORDS = 40, 16                               # PDGN_ADA_STATE_WORDS, PDGN_ADA_SLOT_WORDS
ADA_BOUNDARY = 0.5                                               # least-squares discriminators: real -> 1, fake -> 0
# word indices of pdgn_ada_state (include/pdgn_hip.h)
(W_TARGET, W_INTERVAL, W_SPAN, W_THR_MIN, W_THR_MAX, W_MASK, W_THR, W_POS, W_NEG, W_N, W_ITERS, W_UPDATES, W_LAST_R, W_LAST_POS,
 W_LAST_NEG, W_LAST_N, W_LAST_NET, W_NET) = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 28)


def validate_adaptive(adaptive, p):
    """The adaptive parameters as a dict of plain Python values (ADA_DEFAULTS where a name is missing), or ValueError: target strictly
    inside (-1, 1); interval an integer in [1, 2^20], span an integer in [1, 2^40]; 0 <= p_min <= p <= p_max <= 1."""
    if not isinstance(adaptive, dict):
        raise ValueError("adaptive: None or a dict of %s, got %r" % (sorted(ADA_DEFAULTS), adaptive))
    unknown = set(adaptive) - set(ADA_DEFAULTS)
    if unknown:
        raise ValueError("unknown adaptive parameters: %s" % sorted(unknown))
    a = dict(ADA_DEFAULTS, **adaptive)
    out = {}
    for name in ("target", "p_min", "p_max"):
        try:
            out[name] = float(a[name])
        except (TypeError, ValueError):
            raise ValueError("%s must be a number, got %r" % (name, a[name])) from None
    if not -1.0 < out["target"] < 1.0:                           # (NaN fails both)
        raise ValueError("target must lie strictly inside (-1, 1), got %r" % (a["target"],))
    for name, hi in (("interval", 1 << 20), ("span", 1 << 40)):
        v = a[name]
        if not (isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 1 <= v <= hi):
            raise ValueError("%s must be an integer in [1, 2^%d], got %r" % (name, hi.bit_length() - 1, v))
        out[name] = int(v)
    if not 0.0 <= out["p_min"] <= out["p_max"] <= 1.0:
        raise ValueError("0 <= p_min <= p_max <= 1 required, got p_min %r, p_max %r" % (a["p_min"], a["p_max"]))
    if not out["p_min"] <= float(p) <= out["p_max"]:
        raise ValueError("p = %r lies outside [p_min, p_max] = [%r, %r]" % (p, out["p_min"], out["p_max"]))
    return out


def component_mask(params):
    """Five bits, flip .. jitter: the components whose threshold follows p (a component whose range is zero keeps threshold 0)."""
    on = (params["flip"], params["rot_max_deg"] > 0, params["scale_max"] > 1, params["trans_max"] > 0, params["jitter_sigma"] > 0)
    return sum(1 << k for k, e in enumerate(on) if e)


def ada_words(params, adaptive):
    """The 40 words of a FRESH pdgn_ada_state (accumulators and counters zero) as a uint64 array."""
    w = np.zeros(ADA_WORDS, dtype=np.uint64)
    w.view(np.float64)[W_TARGET] = adaptive["target"]
    w[W_INTERVAL], w[W_SPAN] = adaptive["interval"], adaptive["span"]
    w[W_THR_MIN], w[W_THR_MAX] = threshold(adaptive["p_min"]), threshold(adaptive["p_max"])
    w[W_MASK], w[W_THR] = component_mask(params), threshold(params["p"])
    return w


def decode_ada(words):
    """pdgn_ada_state as it is on the device -> the "ada" dict of `Augment.state()`."""
    w = np.ascontiguousarray(words).view(np.uint64)
    f = w.view(np.float64)
    triples = lambda at: [tuple(int(v) for v in w[at + 3 * i:at + 3 * i + 3]) for i in range(NETWORKS)]
    return {"p": int(w[W_THR]) / float(1 << 24), "thr": int(w[W_THR]), "target": float(f[W_TARGET]), "interval": int(w[W_INTERVAL]),
            "span": int(w[W_SPAN]), "thr_min": int(w[W_THR_MIN]), "thr_max": int(w[W_THR_MAX]), "p_min": int(w[W_THR_MIN]) / float(1 << 24),
            "p_max": int(w[W_THR_MAX]) / float(1 << 24), "mask": int(w[W_MASK]), "pos": int(w[W_POS]), "neg": int(w[W_NEG]), "n": int(w[W_N]),
            "iters": int(w[W_ITERS]), "net": triples(W_NET), "updates": int(w[W_UPDATES]), "last_r": float(f[W_LAST_R]),
            "last": (int(w[W_LAST_POS]), int(w[W_LAST_NEG]), int(w[W_LAST_N])), "last_net": triples(W_LAST_NET)}


def threshold(p):
    """round(p 2^24): a component is enabled iff (word >> 8) < threshold -- 0 never, 2^24 always."""
    return int(round(float(p) * (1 << 24)))


def table_words(params):
    """The 16 words of pdgn_aug_table for validated parameters, as a uint32 array.  A component whose range is zero gets
    threshold 0: it draws nothing that matters and is exactly the identity."""
    thr = threshold(params["p"])
    w = np.zeros(TABLE_WORDS, dtype=np.uint32)
    f = w.view(np.float32)
    w[0] = thr if params["flip"] else 0
    w[1] = thr if params["rot_max_deg"] > 0 else 0
    w[2] = thr if params["scale_max"] > 1 else 0
    w[3] = thr if params["trans_max"] > 0 else 0
    w[4] = thr if params["jitter_sigma"] > 0 else 0
    w.view(np.int32)[5], w.view(np.int32)[6] = params["flip_axis"], params["up_axis"]
    f[7] = np.float32(math.radians(params["rot_max_deg"]))
    f[8] = np.float32(math.log(params["scale_max"]))
    f[9] = np.float32(params["trans_max"])
    f[10] = np.float32(params["jitter_sigma"])
    return w


def decode_table(words):
    """pdgn_aug_table as it is on the device -> a dict (thresholds, axes, ranges in the kernel's units)."""
    w = np.ascontiguousarray(words).view(np.uint32)             # (int32 or uint32 words)
    f = w.view(np.float32)
    return {"thr_flip": int(w[0]), "thr_rot": int(w[1]), "thr_scale": int(w[2]), "thr_trans": int(w[3]), "thr_jitter": int(w[4]),
            "flip_axis": int(w[5]), "up_axis": int(w[6]), "rot_max": float(f[7]), "log_scale_max": float(f[8]),
            "trans_max": float(f[9]), "sigma": float(f[10])}


class AugmentRows(Function):
    """x (B,3,N) -> rows (B*N,3) = A_b x + t_b (+ jitter) by pdgn_augment_rows_fwd; backward dx = A_b^T d_rows by
    pdgn_augment_rows_bwd, which re-derives A_b from the same counter words (the clock must not tick in between: forward and
    backward of a call site belong to one iteration)."""

    @staticmethod
    def forward(ctx, x, aug, site):
        # the generator's clouds are (B,3,N) views of point-major rows: read as they lie, and their gradient written the same way
        ctx.aug, ctx.site, ctx.shape = aug, site, x.shape
        ctx.point_major = x.dim() == 3 and not x.is_contiguous() and x.transpose(1, 2).is_contiguous()
        return aug._forward(x, site, ctx.point_major)

    @staticmethod
    def backward(ctx, d_rows):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return ctx.aug._backward(d_rows, ctx.site, ctx.shape, ctx.point_major), None, None


class AugmentSite:
    """One of the twelve call sites: what `PointDiscriminator.forward(x, aug=...)` takes."""

    def __init__(self, aug, network, role):
        self.aug, self.network, self.role, self.index = aug, network, role, site_index(network, role)

    def rows(self, x):
        return AugmentRows.apply(x, self.aug, self.index)


class Augment:
    def __init__(self, p=DEFAULTS["p"], rot_max_deg=DEFAULTS["rot_max_deg"], scale_max=DEFAULTS["scale_max"], flip=DEFAULTS["flip"],
                 trans_max=DEFAULTS["trans_max"], jitter_sigma=DEFAULTS["jitter_sigma"], up_axis=DEFAULTS["up_axis"],
                 flip_axis=DEFAULTS["flip_axis"], seed=9999, record=False, rank=0, device="cuda", adaptive=None):
        self.params = validate(p, rot_max_deg, scale_max, flip, trans_max, jitter_sigma, up_axis, flip_axis)    # raises before anything is allocated
        self.adaptive = None if adaptive is None else validate_adaptive(adaptive, self.params["p"])
        if not (isinstance(seed, (int, np.integer)) and 0 <= seed < 1 << 64):
            raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
        if not (isinstance(rank, (int, np.integer)) and rank >= 0):
            raise ValueError("rank must be a non-negative integer, got %r" % (rank,))
        self.seed, self.rank, self.record = int(seed), int(rank), bool(record)
        self.device = torch.device(device)
        self.table = torch.from_numpy(table_words(self.params).view(np.int32).copy()).to(self.device)
        self.clock = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.records = None                                      # (12, B, 12) with record=True, allocated at the first call (B is the caller's)
        self._sites = [[AugmentSite(self, n, r) for r in ROLES] for n in range(NETWORKS)]
        lib = _lib.lib()
        self._fwd, self._bwd, self._tick = lib.pdgn_augment_rows_fwd, lib.pdgn_augment_rows_bwd, lib.pdgn_augment_tick
        self.ada = self.slots = None                             # adaptive only: pdgn_ada_state (40 x int64) and the four count slots (16 x int32)
        if self.adaptive is not None:
            self.ada = torch.from_numpy(ada_words(self.params, self.adaptive).view(np.int64).copy()).to(self.device)
            self.slots = torch.zeros(ADA_SLOT_WORDS, dtype=torch.int32, device=self.device)
            self._counters = [self.slots[4 * i:4 * i + 4] for i in range(NETWORKS)]
            self._tick_ada = lib.pdgn_augment_tick_ada

    # ------------------------------------------------------------------ the parameters
    def set(self, **changes):
        """Overwrite parameters IN PLACE (same tensor, same address: launches that have the table's address baked in read the new
        values from their next run on).  Validates the merged set first; raises without touching the table.
        Adaptive: the five adaptive parameters are accepted too and written into the state record in place; `p` sets the CURRENT
        threshold (it must lie inside [p_min, p_max]); without `p` the thresholds keep the device's current value (read back:
        synchronises), so changing a component's range only recomputes the mask."""
        known = set(self.params) | (set(ADA_DEFAULTS) if self.adaptive is not None else set())
        unknown = set(changes) - known
        if unknown:
            raise ValueError("unknown augmentation parameters: %s" % sorted(unknown))
        if self.adaptive is None:
            merged = validate(**dict(self.params, **changes))
            fresh = torch.from_numpy(table_words(merged).view(np.int32).copy())
            with torch.no_grad():
                self.table.copy_(fresh)
            self.params = merged
            return
        ada_changes = {k: v for k, v in changes.items() if k in ADA_DEFAULTS}
        own = {k: v for k, v in changes.items() if k not in ADA_DEFAULTS}
        if "p" not in own:                                       # the device's p, exactly: thr 2^-24 rounds back to thr
            own["p"] = int(self.ada[W_THR].item()) / float(1 << 24)
        merged = validate(**dict(self.params, **own))
        adaptive = validate_adaptive(dict(self.adaptive, **ada_changes), merged["p"])
        head = ada_words(merged, adaptive)[:W_THR + 1]           # the parameters, the mask and thr: words 0 .. 6, one contiguous copy
        with torch.no_grad():
            self.table.copy_(torch.from_numpy(table_words(merged).view(np.int32).copy()))
            self.ada[:W_THR + 1].copy_(torch.from_numpy(head.view(np.int64).copy()))
        self.params, self.adaptive = merged, adaptive

    # ------------------------------------------------------------------ the clock
    def tick(self):
        """Open an iteration: clock += 1 by one launch on the current stream (capturable); adaptive: the same single launch also
        folds the previous iteration's counts and, when due, moves the thresholds."""
        if self.adaptive is not None:
            a = self.adaptive                                    # (the parameters travel for the entry point's checks only: the kernel reads the record)
            _lib.check(self._tick_ada(_lib.ptr(self.clock), _lib.ptr(self.ada), _lib.ptr(self.slots), _lib.ptr(self.table), a["interval"], a["span"],
                                      threshold(a["p_min"]), threshold(a["p_max"]), _lib.stream_of(self.clock)), "pdgn_augment_tick_ada")
            return
        _lib.check(self._tick(_lib.ptr(self.clock), _lib.stream_of(self.clock)), "pdgn_augment_tick")

    def counter(self, network):
        """The 16-byte slot into which discriminator `network`'s real-batch loss term stores (pos, neg, n): what
        `losses.mse_const(..., count=)` takes.  Adaptive only."""
        if self.adaptive is None:
            raise RuntimeError("counter(): this Augment is not adaptive (adaptive=None): nothing counts")
        if not (isinstance(network, (int, np.integer)) and 0 <= network < NETWORKS):
            raise ValueError("network: 0 .. 3 (D1 .. D4), got %r" % (network,))
        return self._counters[network]

    def set_clock(self, t):
        """The next iteration (the next `tick`) draws at t.  A copy on the current stream."""
        if not (isinstance(t, (int, np.integer)) and 0 <= t < 1 << 62):
            raise ValueError("clock must be a non-negative integer, got %r" % (t,))
        with torch.no_grad():
            self.clock.fill_(int(t))

    # ------------------------------------------------------------------ the call sites
    def at(self, network, role):
        site_index(network, role)
        return self._sites[network][ROLES.index(role)]

    def rows(self, x, network, role):
        """x (B,3,N) -> (B*N,3): the augmented cloud in the discriminators' row layout, differentiable wrt x."""
        return AugmentRows.apply(x, self, site_index(network, role))

    def _check(self, t, name):
        _lib.require(t, name, torch.float32)
        if t.device != self.table.device:
            raise _lib.PdgnHipError("%s lives on %s, the augmentation state on %s" % (name, t.device, self.table.device))

    def _forward(self, x, site, point_major=False):
        if x.dim() != 3 or x.shape[1] != 3:
            raise ValueError("x must be (B,3,N), got %s" % (tuple(x.shape),))
        B, _, N = x.shape
        if point_major:
            x = x.transpose(1, 2)                                # (B,N,3), contiguous: the same memory
        x = x.contiguous()
        self._check(x, "x")
        rows = torch.empty(B * N, 3, dtype=torch.float32, device=x.device)
        rec = None
        if self.record:
            if self.records is None or self.records.shape[1] != B:
                self.records = torch.zeros(3 * NETWORKS, B, 12, dtype=torch.float32, device=self.device)
            rec = self.records[site]
        _lib.check(self._fwd(B, N, _lib.ptr(x), int(point_major), _lib.ptr(rows), _lib.ptr(rec), _lib.ptr(self.table), _lib.ptr(self.clock), self.seed,
                             self.rank * B, TAG_BASE + site, _lib.stream_of(x)), "pdgn_augment_rows_fwd")
        return rows

    def _backward(self, d_rows, site, shape, point_major=False):
        B, _, N = shape
        d_rows = d_rows.contiguous()
        self._check(d_rows, "d_rows")
        dx = torch.empty((B, N, 3) if point_major else (B, 3, N), dtype=torch.float32, device=d_rows.device)
        _lib.check(self._bwd(B, N, _lib.ptr(d_rows), _lib.ptr(dx), int(point_major), _lib.ptr(self.table), _lib.ptr(self.clock), self.seed,
                             self.rank * B, TAG_BASE + site, _lib.stream_of(d_rows)), "pdgn_augment_rows_bwd")
        return dx.transpose(1, 2) if point_major else dx

    # ------------------------------------------------------------------ what was drawn
    def state(self):
        """{clock, params (the table as it is on the device, decoded), records ((12, B, 12) numpy or None)}; adaptive: also "ada"
        (`decode_ada`: current p and thr, the parameters, accumulators, interval progress, updates, last_r, the last update's
        totals and per-network triples).  Synchronises."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        out = {"clock": int(self.clock.item()), "params": decode_table(self.table.cpu().numpy().view(np.uint32)),
               "records": None if self.records is None else self.records.cpu().numpy()}
        if self.adaptive is not None:
            out["ada"] = decode_ada(self.ada.cpu().numpy())
        return out

    # ------------------------------------------------------------------ persistence (adaptive: p is state, it cannot be derived)
    def checkpoint(self):
        """What `PDGNTrainer.save` writes beside G.pth / D.pth: the state record's words, the slots, the table, the parameters."""
        if self.adaptive is None:
            raise RuntimeError("checkpoint(): this Augment is not adaptive: its state is derived (the clock) or constant (the table)")
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return {"ada_state": self.ada.cpu().clone(), "slots": self.slots.cpu().clone(), "table": self.table.cpu().clone(),
                "params": dict(self.params), "adaptive": dict(self.adaptive)}

    def restore(self, saved):
        """`checkpoint()`'s dict back into this object, in place (same addresses).  Validates first."""
        if self.adaptive is None:
            raise RuntimeError("restore(): this Augment is not adaptive")
        params = validate(**saved["params"])
        adaptive = validate_adaptive(saved["adaptive"], params["p"])
        ada, slots, table = saved["ada_state"], saved["slots"], saved["table"]
        if (tuple(ada.shape), ada.dtype) != ((ADA_WORDS,), torch.int64) or (tuple(slots.shape), slots.dtype) != ((ADA_SLOT_WORDS,), torch.int32) \
                or (tuple(table.shape), table.dtype) != ((TABLE_WORDS,), torch.int32):
            raise ValueError("restore(): not an adaptive augmentation checkpoint")
        with torch.no_grad():
            self.ada.copy_(ada), self.slots.copy_(slots), self.table.copy_(table)
        self.params, self.adaptive = params, adaptive
