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
means "the next iteration draws at t = c", and after it the clock reads c + 1."""
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
                 flip_axis=DEFAULTS["flip_axis"], seed=9999, record=False, rank=0, device="cuda"):
        self.params = validate(p, rot_max_deg, scale_max, flip, trans_max, jitter_sigma, up_axis, flip_axis)    # raises before anything is allocated
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

    # ------------------------------------------------------------------ the parameters
    def set(self, **changes):
        """Overwrite parameters IN PLACE (same tensor, same address: launches that have the table's address baked in read the new
        values from their next run on).  Validates the merged set first; raises without touching the table."""
        unknown = set(changes) - set(self.params)
        if unknown:
            raise ValueError("unknown augmentation parameters: %s" % sorted(unknown))
        merged = validate(**dict(self.params, **changes))
        fresh = torch.from_numpy(table_words(merged).view(np.int32).copy())
        with torch.no_grad():
            self.table.copy_(fresh)
        self.params = merged

    # ------------------------------------------------------------------ the clock
    def tick(self):
        """Open an iteration: clock += 1 by one launch on the current stream (capturable)."""
        _lib.check(self._tick(_lib.ptr(self.clock), _lib.stream_of(self.clock)), "pdgn_augment_tick")

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
        """{clock, params (the table as it is on the device, decoded), records ((12, B, 12) numpy or None)}.  Synchronises."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return {"clock": int(self.clock.item()), "params": decode_table(self.table.cpu().numpy().view(np.uint32)),
                "records": None if self.records is None else self.records.cpu().numpy()}
