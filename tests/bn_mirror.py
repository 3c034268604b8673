"""Host mirror of the channels-last BatchNorm kernels (csrc/bnact.hip): numpy only, float64 with float32 wherever the kernels round
to float32, written from the formulas the kernels quote, so that tests can demand equal bits.  Test infrastructure: the product never
imports it.

    statistics   three partial layouts (own pivot [gy][2C], raw [gy][2C], block-shifted [nparts][3C]) and their finalisers:
                 ms = s1/R, var = max(s2/R - ms*ms, 0), mean = ms + pivot;  per block mb = pv + s*inv, a += n*mb,
                 b += (sq - s*s*inv) + n*mb*mb, mean = a/R, var = max(b/R - mean*mean, 0);  invstd = fp32(1/sqrt(var + eps)),
                 scale = gamma*invstd, shift = beta - fp32(mean)*scale; running statistics with the unbiased variance (R > 1)
    apply        y = act(fma(x, scale, shift)) [* mul]; interleaved: x row b*N + n, channel 2c + j -> y row b*2N + j*N + n, channel c
    backward     dz = dy [*mul] * act'(z) (act' decided by z > 0); bsums = [sum dz | sum dz*xhat]; cb = scale*invstd*fp32(s2/R),
                 ca = scale*fp32(s1/R) - cb*mean; dx = fma(scale, dz, -ca) - cb*x; dmul = dy*act(z)
    max-pool     apply form: ymax = max_n act(z), yarg = the LOWEST row attaining ymax;  one-pass form: yarg = the lowest row attaining
                 the largest x (scale >= 0) or the smallest x (scale < 0), ymax = act(fma(x[yarg], scale, shift))
                 adjoint: dz[b,c] = dout*act'(z at yarg), dx = (n == yarg ? scale*dz : 0) - ca - cb*x

The build uses -ffp-contract=off: the only fused multiply-adds are the explicit ones, mirrored by `fma32` (the float64 product is exact,
the float64 sum is rounded once more to float32; the elements whose float64 sum lies within one float64 ulp of a float32 rounding
midpoint are recomputed in rational arithmetic).

Exactness.  The sums are the only place where a kernel's order of operations could show.  `Guard` collects, while the mirror runs,
every float32 sum (terms and their absolute values), every float64 sum and every float64 -> float32 rounding of a finaliser;
`assert_exact` then proves that each float32 partial sum is a float32 in every order (all terms multiples of one power of two, the sum
of |terms| below 2^24 of them), the same for the float64 sums (2^53), and that each rounded float64 value moved by +-2 float64 ulps
rounds to the same float32 (so the bits cannot depend on whether the device's float64 sqrt or division is correctly rounded).

Every function takes `mut`, a set of names from MUTANTS: deliberately wrong variants, used by tests/test_bn_mirror_host.py to show that
the case table tells each of them from the mirror."""
from fractions import Fraction

import numpy as np

import wgs_mirror as wm

F32, F64 = np.float32, np.float64
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
SLOPE = F32(0.01)
CSRC = wm.CSRC
NO = frozenset()
MUTANTS = ("last_block_full", "spare_rows", "no_pivot", "biased_running_var", "pre_bias_in_mean", "drop_last_slice", "ties_highest",
           "no_min_branch", "kink_grad_one", "interleave_2n", "ca_without_mean")


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------- the launchers' constants, read from their text
def source_constants():
    t = wm._read("bnact.hip")
    one = wm._one
    c = {"MP_SPLIT": int(one(t, r"#define MP_SPLIT (\d+)\n", "max-pool splits")),
         "MP_CGB": int(one(t, r"while \(p < cg && p < (\d+)\) p <<= 1;", "max-pool column groups per block")),
         "FB_MIN": int(one(t, r"if \(nparts < (\d+)\) return 0;", "shortest sliced list")),
         "FB64_MIN": int(one(t, r"if \(nparts <= (\d+)\) return 0;", "shortest 64-channel sliced list")),
         "FB64_MAX": int(one(t, r"return \(int\)\(s64 < 2 \? 2 : \(s64 > (\d+) \? \1 : s64\)\);", "64-channel slice clamp")),
         "FB_WG": int(one(t, r"long long s = (\d+) / \(c / 4 > 0 \? c / 4 : 1\);", "workgroups wanted")),
         "FB_MAX": int(one(t, r"s = s > (\d+) \? \1 : s;", "four-channel slice clamp")),
         "FB_PER": int(one(t, r"while \(s > 1 && nparts / s < (\d+)\) s >>= 1;", "rows per slice"))}
    one(t, r"long long s64 = nparts / 64;", "64-channel slices")
    one(t, r"const int slices = scratch \? fb_slices\(c, nparts\) : 0;", "the scratch == NULL fallback")
    one(t, r"const int per = \(int\)\(\(nparts \+ slices - 1\) / slices\);", "rows per slice")
    one(t, r"if \(rows < 1 \|\| c < 4 \|\| c % 4 \|\| nparts < 1 \|\| nparts > 0x7fffffffLL \|\| block_rows < 1 \|\|\n"
           r"\s+nparts \* \(long long\)block_rows < rows\)", "block finaliser refusals")
    one(t, r"if \(interleave_n < 0 \|\| \(interleave_n > 0 && \(rows % interleave_n \|\| mul\)\)\) return PDGN_ERR_INVALID;\n"
           r"\s+int cgb, gx, gy, rpb;\n\s+cl_geometry\(rows, c, &cgb, &gx, &gy, &rpb\);\n\s+hipLaunchKernelGGL\(cl_apply_kernel", "apply refusals")
    return c


_CONST = None


def constants():
    global _CONST
    if _CONST is None:
        _CONST = source_constants()
    return _CONST


# ---------------------------------------------------------------------------- launch rules
def cl_geometry(R, C):
    """csrc/bn_geom.h restated on its own -> (cgb, gx, gy, rows_per_block); the host test holds it against wgs_mirror.cl_geometry."""
    cg, p = C // 4, 1
    while p < cg and p < 256:
        p <<= 1
    gx, rl = cdiv(cg, p), 256 // p
    rows = min(max(cdiv(R, max(1, 1024 // gx)), rl * 16), 65536)
    rows = cdiv(rows, rl) * rl
    return p, gx, cdiv(R, rows), rows


def mp_geometry(C):
    """-> (cgb, gx, row lanes) of the max-pool kernels."""
    cg, p = C // 4, 1
    while p < cg and p < constants()["MP_CGB"]:
        p <<= 1
    return p, cdiv(cg, p), 256 // p


def mp_splits(n):
    """The [n0, n1) row ranges of the MP_SPLIT splits of a sample (those beyond the data are empty)."""
    S = constants()["MP_SPLIT"]
    per = cdiv(n, S)
    return [(min(n, s * per), min(n, s * per + per)) for s in range(S)]


def fb_slices(c, nparts):
    k = constants()
    if nparts < k["FB_MIN"]:
        return 0
    if c % 64 == 0:
        if nparts <= k["FB64_MIN"]:
            return 0
        return int(min(max(nparts // 64, 2), k["FB64_MAX"]))
    s = min(k["FB_WG"] // max(c // 4, 1), k["FB_MAX"])
    while s > 1 and nparts // s < k["FB_PER"]:
        s >>= 1
    return 0 if s < 2 else s


def per_slice(nparts, slices):
    return cdiv(nparts, slices)


def slice_counts(nparts, slices, used):
    """How many of the `used` row-holding partial rows each slice holds."""
    per = per_slice(nparts, slices)
    return [max(0, min(used, s * per + per) - s * per) for s in range(slices)]


def blocks_scratch_doubles(c, nparts):
    return fb_slices(c, nparts) * 2 * c


def regime(rows, c, nparts, block_rows, scratch=True):
    """Which form pdgn_bn_stats_from_gemm_partials takes: "one_launch", "slice4", "slice64", or "invalid" where it refuses."""
    if rows < 1 or c < 4 or c % 4 or nparts < 1 or nparts > 0x7fffffff or block_rows < 1 or nparts * block_rows < rows:
        return "invalid"
    s = fb_slices(c, nparts) if scratch else 0
    return "one_launch" if s < 2 else ("slice64" if c % 64 == 0 else "slice4")


# ---------------------------------------------------------------------------- the exactness guard
class Guard:
    """What `assert_exact` checks, collected while the mirror runs."""

    def __init__(self):
        self.sums32, self.sums64, self.rounded = [], [], []

    def sum32(self, what, terms, starts=None):
        """A float32 sum over axis 0 of `terms`, in whatever order (starts: one sum per segment of rows beginning there)."""
        self.sums32.append((what, np.asarray(terms, dtype=F64), starts))

    def sum64(self, what, terms):
        self.sums64.append((what, np.asarray(terms, dtype=F64), None))

    def round32(self, what, v):
        self.rounded.append((what, np.asarray(v, dtype=F64)))


def column_quanta(t):
    """Per column of t (rows, cols): the largest power of two <= 1 dividing all its values (NaN: none down to 2^-80)."""
    q, pending = np.full(t.shape[1], np.nan), np.ones(t.shape[1], bool)
    for k in range(81):
        s = t[:, pending] * 2.0 ** k
        idx = np.nonzero(pending)[0][(s == np.rint(s)).all(0)]
        q[idx], pending[idx] = 2.0 ** -k, False
        if not pending.any():
            break
    return q


def _order_free(what, terms, bits, starts=None):
    """Every partial sum over axis 0 is exact in a format of `bits` significand bits, in every order: per destination either all terms
    are multiples of one quantum with the sum of |terms| below 2^bits quanta, or at most two terms are non-zero and their sum is exact
    (one addition: nothing to reorder)."""
    t = terms.reshape(terms.shape[0], -1)
    if not t.size:
        return
    if not np.isfinite(t).all():
        raise AssertionError("%s: a term is not finite" % what)
    total = np.abs(t).sum(0) if starts is None else np.add.reduceat(np.abs(t), starts, axis=0).max(0)
    with np.errstate(invalid="ignore"):
        lattice = total < 2.0 ** bits * column_quanta(t)
    for j in np.nonzero(~lattice)[0]:
        col = t[:, j][t[:, j] != 0]
        ok = starts is None and len(col) <= 2 and (bits == 53 or F64(F32(col.sum())) == col.sum())
        if not ok:
            raise AssertionError("%s: destination %d: sum of |terms| is not below 2^%d quanta" % (what, j, bits))


def assert_exact(guard):
    """Bit equality with a device is then independent of the device's order of summation and of the last bit of its float64
    division and square root (see the module docstring)."""
    for what, terms, starts in guard.sums32:
        if not np.array_equal(terms, terms.astype(F32).astype(F64)):
            raise AssertionError("%s: a term is not a float32" % what)
        _order_free(what, terms, 24, starts)
    for what, terms, _ in guard.sums64:
        _order_free(what, terms, 53)
    for what, v in guard.rounded:
        lo = hi = v
        for _ in range(2):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        with np.errstate(over="ignore"):
            if not (np.array_equal(lo.astype(F32), v.astype(F32)) and np.array_equal(hi.astype(F32), v.astype(F32))):
                raise AssertionError("%s: a float64 value lies within 2 ulps of a float32 rounding midpoint" % what)


# ---------------------------------------------------------------------------- float32 arithmetic
def f32(a):
    return np.asarray(a, dtype=F64).astype(F32)


def _round_fraction32(fr):
    """A Fraction correctly rounded to float32 (nearest, ties to even)."""
    a = F32(float(fr))                                             # within an ulp: the answer is a or a neighbour
    cands = sorted({float(a), float(np.nextafter(a, F32(-np.inf))), float(np.nextafter(a, F32(np.inf)))})
    best = min(cands, key=lambda v: (abs(Fraction(v) - fr), int(np.float32(v).view(np.uint32)) & 1))
    return F32(best)


def fma32(a, b, c):
    """The single-rounded float32 fma(a, b, c) of float32 arrays."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    shape = a.shape
    a, b, c = a.reshape(-1), b.reshape(-1), c.reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        z = a.astype(F64) * b.astype(F64) + c.astype(F64)          # exact product, one rounding
        r = z.astype(F32)
        risky = np.isfinite(z) & ((np.nextafter(z, -np.inf).astype(F32) != r) | (np.nextafter(z, np.inf).astype(F32) != r))
    if risky.any():
        r = r.copy()
        at = np.nonzero(risky)[0]
        # (lattice inputs repeat: one rational evaluation per distinct operand triple)
        triples, inverse = np.unique(np.stack([a[at], b[at], c[at]], 1).view(np.uint32), axis=0, return_inverse=True)
        fixed = r[at]
        for j, t in enumerate(triples.view(F32)):
            fr = Fraction(float(t[0])) * Fraction(float(t[1])) + Fraction(float(t[2]))
            if fr != 0:                                            # (an exact zero keeps the sign the float64 sum gave it)
                fixed[inverse.reshape(-1) == j] = _round_fraction32(fr)
        r[at] = fixed
    return r.reshape(shape)


def act_fwd(z, act):
    z = np.asarray(z, F32)
    if act == ACT_RELU:
        return np.where(z > 0, z, F32(0.0)).astype(F32)            # fmaxf(z, 0): +0 for z = -0 is one of C's two permitted answers
    if act == ACT_LEAKY:
        return np.where(z > 0, z, SLOPE * z).astype(F32)
    return z


def act_grad(z, act, mut=NO):
    pos = (z >= 0) if "kink_grad_one" in mut else (z > 0)
    if act == ACT_RELU:
        return np.where(pos, F32(1), F32(0)).astype(F32)
    if act == ACT_LEAKY:
        return np.where(pos, F32(1), SLOPE).astype(F32)
    return np.ones(np.shape(z), F32)


def relu_zero_sign_free(z, act):
    """Where the sign of a zero output is not the kernel's to decide: fmaxf(-0, +0)."""
    return (act == ACT_RELU) & (np.asarray(z) == 0) & np.signbit(z)


# ---------------------------------------------------------------------------- the three partial layouts
def partials_own_pivot(X, guard=None, raw=False):
    """[gy][2C] float64 as cl_stats_kernel leaves them: per row block the sums of x - x[0] and of its square (raw: of x itself, the
    layout pdgn_bn_stats_from_partials consumes without a pivot)."""
    X = np.asarray(X, dtype=F64)
    R, C = X.shape
    cgb, gx, gy, rpb = cl_geometry(R, C)
    d = X if raw else f32(X - X[0]).astype(F64)
    part = np.zeros((gy, 2 * C), F64)
    for g in range(gy):
        blk = d[g * rpb:(g + 1) * rpb]
        part[g, :C], part[g, C:] = blk.sum(0), (blk * blk).sum(0)
    if guard is not None:
        guard.sum32("sum (x - pivot)", d)
        guard.sum32("sum (x - pivot)^2", d * d)
    return part


def partials_blocks(X, block_rows, nparts, spare=np.nan, guard=None):
    """[nparts][3C] float32, block-shifted: sum (x - pv_b) | sum (x - pv_b)^2 | pv_b with pv_b the block's first row; the last block is
    short; the rows beyond ceil(R / block_rows) hold `spare`."""
    X = np.asarray(X, dtype=F64)
    R, C = X.shape
    used = cdiv(R, block_rows)
    assert used <= nparts
    part = np.full((nparts, 3 * C), spare, F64)
    starts = np.arange(used) * block_rows
    d = X - X[np.repeat(starts, block_rows)[:R]]
    part[:used, :C], part[:used, C:2 * C] = np.add.reduceat(d, starts, axis=0), np.add.reduceat(d * d, starts, axis=0)
    part[:used, 2 * C:] = X[starts]
    if guard is not None:
        guard.sum32("block sum", d, starts)
        guard.sum32("block sum of squares", d * d, starts)
    return part.astype(F32)


# ---------------------------------------------------------------------------- finalisers
def _finish(mean, var, R, C, eps, momentum, gamma, beta, pre_bias, rm, rv, guard, mut):
    """From the float64 mean and (clamped) variance: stats [scale | shift | mean | invstd] and the running buffers."""
    eps = F64(F32(eps))
    with np.errstate(divide="ignore"):
        inv64 = 1.0 / np.sqrt(var + eps)
    norm_mean = mean + (np.asarray(pre_bias, F64) if (pre_bias is not None and "pre_bias_in_mean" in mut) else 0.0)
    if guard is not None:
        guard.round32("1/sqrt(var + eps)", inv64)
        guard.round32("mean", norm_mean)
    invstd, mean32 = inv64.astype(F32), norm_mean.astype(F32)
    g = np.ones(C, F32) if gamma is None else np.asarray(gamma, F32)
    b = np.zeros(C, F32) if beta is None else np.asarray(beta, F32)
    scale = g * invstd
    out = {"stats": np.concatenate([scale, b - mean32 * scale, mean32, invstd]).astype(F32), "mean64": mean, "var64": var}
    if rm is not None:
        unbiased = var * F64(R) / F64(R - 1) if (R > 1 and "biased_running_var" not in mut) else var
        if guard is not None:
            guard.round32("unbiased variance", unbiased)
        mb = mean.astype(F32) + (np.asarray(pre_bias, F32) if pre_bias is not None else F32(0.0))
        m = F32(momentum)
        out["running_mean"] = ((F32(1.0) - m) * np.asarray(rm, F32) + m * mb).astype(F32)
        out["running_var"] = ((F32(1.0) - m) * np.asarray(rv, F32) + m * unbiased.astype(F32)).astype(F32)
    return out


def finalize_sums(part, R, pivot, eps=1e-5, momentum=0.1, gamma=None, beta=None, pre_bias=None, rm=None, rv=None, guard=None, mut=NO):
    """cl_finalize_kernel: `part` [n][2C] (float32 values) summed in float64; pivot (C) or None."""
    part = np.asarray(part, dtype=F64)
    C = part.shape[1] // 2
    if guard is not None:
        guard.sum64("sum of partials", part)
    s1, s2 = part[:, :C].sum(0), part[:, C:].sum(0)
    ms = s1 / F64(R)
    var = np.maximum(s2 / F64(R) - ms * ms, 0.0)
    mean = ms + (np.asarray(pivot, F64) if (pivot is not None and "no_pivot" not in mut) else 0.0)
    return _finish(mean, var, R, C, eps, momentum, gamma, beta, pre_bias, rm, rv, guard, mut)


def block_terms(part, R, block_rows, mut=NO):
    """The per-block contributions (a_p, b_p) [used][C] of the block finalisers, in the kernels' order of float64 operations."""
    part = np.asarray(part, dtype=F64)
    nparts, C = part.shape[0], part.shape[1] // 3
    used = nparts if "spare_rows" in mut else min(nparts, cdiv(R, block_rows))
    left = R - np.arange(used, dtype=np.int64) * block_rows
    full = (left >= block_rows) | ("last_block_full" in mut)
    n = np.where(full, block_rows, left).astype(F64)[:, None]
    with np.errstate(divide="ignore"):
        inv = np.where(full, 1.0 / F64(block_rows), 1.0 / left.astype(F64))[:, None]
    s, sq, pv = part[:used, :C], part[:used, C:2 * C], part[:used, 2 * C:]
    mb = pv + s * inv
    return n * mb, (sq - s * s * inv) + n * mb * mb


def finalize_blocks(part, R, block_rows, slices=0, eps=1e-5, momentum=0.1, gamma=None, beta=None, pre_bias=None, rm=None, rv=None,
                    guard=None, mut=NO):
    """cl_finalize_blocks_kernel (slices < 2) or the slice + join pair: `part` [nparts][3C] float32."""
    nparts, C = part.shape[0], part.shape[1] // 3
    ta, tb = block_terms(part, R, block_rows, mut)
    if slices > 1 and "drop_last_slice" in mut:
        keep = (slices - 1) * per_slice(nparts, slices)
        ta, tb = ta[:keep], tb[:keep]
    if guard is not None:
        guard.sum64("sum n*mean_b", ta)
        guard.sum64("sum M2_b + n*mean_b^2", tb)
    mean = ta.sum(0) / F64(R)
    var = np.maximum(tb.sum(0) / F64(R) - mean * mean, 0.0)
    return _finish(mean, var, R, C, eps, momentum, gamma, beta, pre_bias, rm, rv, guard, mut)


def rational_blocks(part, R, block_rows, eps):
    """The exact mean, biased and unbiased variance (Fractions) and 1/sqrt(var + eps) (float64, from 60 decimal digits) of the given
    float32 partials: what the rounded tier holds a device within one float32 ulp of."""
    import decimal
    part = np.asarray(part, dtype=F64)
    C, used = part.shape[1] // 3, min(part.shape[0], cdiv(R, block_rows))
    ctx = decimal.Context(prec=60)
    means, vars_, unb, inv = [], [], [], []
    for c in range(C):
        a = b = Fraction(0)
        for p in range(used):
            n = min(block_rows, R - p * block_rows)
            s, sq, pv = Fraction(float(part[p, c])), Fraction(float(part[p, C + c])), Fraction(float(part[p, 2 * C + c]))
            mb = pv + s / n
            a += n * mb
            b += (sq - s * s / n) + n * mb * mb
        mean = a / R
        var = max(b / R - mean * mean, Fraction(0))
        ve = var + Fraction(float(F32(eps)))
        root = ctx.sqrt(ctx.divide(decimal.Decimal(ve.numerator), decimal.Decimal(ve.denominator)))
        means.append(mean)
        vars_.append(var)
        unb.append(var * R / (R - 1) if R > 1 else var)
        inv.append(float(ctx.divide(decimal.Decimal(1), root)))
    return means, vars_, unb, np.array(inv, F64)


def eval_stats(C, eps, gamma, beta, pre_bias, rm, rv, invstd=None):
    """cl_eval_stats_kernel.  invstd: the device's own (rsqrtf is the hardware's approximation, not correctly rounded: the test
    bounds it and restates the rest from it); default the correctly rounded one."""
    ve = np.asarray(rv, F32) + F32(eps)
    if invstd is None:
        invstd = (1.0 / np.sqrt(ve.astype(F64))).astype(F32)
    g = np.ones(C, F32) if gamma is None else np.asarray(gamma, F32)
    b = np.zeros(C, F32) if beta is None else np.asarray(beta, F32)
    m = (np.asarray(rm, F32) - (np.asarray(pre_bias, F32) if pre_bias is not None else F32(0.0))).astype(F32)
    return np.concatenate([g * invstd, b - m * g * invstd, m, invstd]).astype(F32)


# ---------------------------------------------------------------------------- apply, backward
def split_stats(stats):
    C = len(stats) // 4
    s = np.asarray(stats, F32)
    return s[:C], s[C:2 * C], s[2 * C:3 * C], s[3 * C:]


def interleave(y, N, mut=NO):
    """(rows, C) -> (2 rows, C / 2): x row b*N + n, channel 2c + j  ->  y row b*2N + j*N + n, channel c."""
    rows, C = y.shape
    B = rows // N
    out = np.empty((2 * rows, C // 2), y.dtype)
    v = y.reshape(B, N, C // 2, 2)
    if "interleave_2n" in mut:
        out.reshape(B, N, 2, C // 2)[:] = v.transpose(0, 1, 3, 2)
    else:
        out.reshape(B, 2, N, C // 2)[:] = v.transpose(0, 3, 1, 2)
    return out


def deinterleave(dy, N, mut=NO):
    rows2, C2 = dy.shape
    B = rows2 // (2 * N)
    if "interleave_2n" in mut:
        return np.ascontiguousarray(dy.reshape(B, N, 2, C2).transpose(0, 1, 3, 2)).reshape(B * N, 2 * C2)
    return np.ascontiguousarray(dy.reshape(B, 2, N, C2).transpose(0, 2, 3, 1)).reshape(B * N, 2 * C2)


def apply(X, stats, act, mul=None, interleave_n=0, mut=NO):
    """pdgn_bn_act_forward -> (y float32, z float32)."""
    sc, sh, _, _ = split_stats(stats)
    z = fma32(np.asarray(X, F32), sc, sh)
    y = act_fwd(z, act)
    if mul is not None:
        y = (y * np.asarray(mul, F32)).astype(F32)
    return (interleave(y, interleave_n, mut) if interleave_n else y), z


def backward(X, dy, stats, act, training, mul=None, interleave_n=0, guard=None, mut=NO):
    """pdgn_bn_act_backward -> dict(bsums (2C), dx, dmul, coef (2C))."""
    X = np.asarray(X, F32)
    R, C = X.shape
    sc, sh, mu, is_ = split_stats(stats)
    g = deinterleave(np.asarray(dy, F32), interleave_n, mut) if interleave_n else np.asarray(dy, F32)
    z = fma32(X, sc, sh)
    gm = (g * np.asarray(mul, F32)).astype(F32) if mul is not None else g
    dz = (gm * act_grad(z, act, mut)).astype(F32)
    xhat = ((X - mu).astype(F32) * is_).astype(F32)
    t2 = dz.astype(F64) * xhat.astype(F64)
    if guard is not None:
        guard.sum32("sum dz", dz)
        guard.sum32("sum dz*xhat", t2)
    s1, s2 = dz.astype(F64).sum(0), t2.sum(0)
    coef = _coef(s1, s2, R, sc, mu, is_, training, guard, mut)
    ca, cb = coef[:C], coef[C:]
    dx = (fma32(sc, dz, -ca) - (cb * X).astype(F32)).astype(F32)
    dmul = (g * act_fwd(z, act)).astype(F32)
    return {"bsums": np.concatenate([s1, s2]).astype(F32), "dx": dx, "dmul": dmul, "coef": coef, "z": z}


def _coef(s1, s2, R, sc, mu, is_, training, guard, mut):
    C = len(sc)                                                   # (s1, s2 are exact sums: their float32 rounding needs no guard)
    if not training:
        return np.zeros(2 * C, F32)
    m1, m2 = s1 / F64(R), s2 / F64(R)
    if guard is not None:
        guard.round32("s1/R", m1)
        guard.round32("s2/R", m2)
    cb = ((sc * is_).astype(F32) * m2.astype(F32)).astype(F32)
    ca = (sc * m1.astype(F32)).astype(F32)
    if "ca_without_mean" not in mut:
        ca = (ca - (cb * mu).astype(F32)).astype(F32)
    return np.concatenate([ca, cb]).astype(F32)


# ---------------------------------------------------------------------------- max-pool tails
def _first_extreme(v, largest, mut):
    """Per (sample, channel) of v (B, N, C): the row of the largest / smallest value, the lowest such row."""
    if "ties_highest" in mut:
        r = v[:, ::-1]
        return v.shape[1] - 1 - (np.argmax(r, axis=1) if largest else np.argmin(r, axis=1))
    return np.argmax(v, axis=1) if largest else np.argmin(v, axis=1)


def maxpool_apply(X, stats, act, B, N, mut=NO):
    """pdgn_bn_act_maxpool -> (ymax (B, C) float32, yarg (B, C) int32, unique (B, C) bool: the maximum is attained once)."""
    y, _ = apply(X, stats, act)
    y = y.reshape(B, N, -1)
    arg = _first_extreme(y, True, mut)
    ymax = np.take_along_axis(y, arg[:, None, :], 1)[:, 0]
    return ymax, arg.astype(np.int32), (y == ymax[:, None, :]).sum(1) == 1


def maxpool_pick(X, stats, act, B, N, mut=NO):
    """cl_stats_max_kernel + cl_max_pick_kernel given the finalised stats -> (ymax, yarg)."""
    X = np.asarray(X, F32).reshape(B, N, -1)
    sc, sh, _, _ = split_stats(stats)
    up = (sc >= 0) | ("no_min_branch" in mut)
    arg = np.where(up[None, :], _first_extreme(X, True, mut), _first_extreme(X, False, mut))
    best = np.take_along_axis(X, arg[:, None, :], 1)[:, 0]
    return act_fwd(fma32(best, sc, sh), act), arg.astype(np.int32)


def maxpool_stats(X, B, N, guard=None, **kw):
    """The statistics half of pdgn_bn_stats_act_maxpool: own-pivot partials per (sample, split), cl_finalize_kernel over B*MP_SPLIT rows."""
    X = np.asarray(X, dtype=F64)
    C = X.shape[1]
    d = f32(X - X[0]).astype(F64).reshape(B, N, C)
    part = np.zeros((B, constants()["MP_SPLIT"], 2 * C), F64)
    for s, (n0, n1) in enumerate(mp_splits(N)):
        part[:, s, :C], part[:, s, C:] = d[:, n0:n1].sum(1), (d[:, n0:n1] ** 2).sum(1)
    if guard is not None:
        guard.sum32("sum (x - pivot)", d.reshape(B * N, C))
        guard.sum32("sum (x - pivot)^2", d.reshape(B * N, C) ** 2)
    return finalize_sums(part.reshape(-1, 2 * C), B * N, X[0], guard=guard, **kw)


def maxpool_backward(X, dout, yarg, stats, act, training, B, N, guard=None, mut=NO):
    """pdgn_bn_act_maxpool_backward -> dict(bsums, dx, dz, coef)."""
    X = np.asarray(X, F32)
    C = X.shape[1]
    sc, sh, mu, is_ = split_stats(stats)
    v = np.take_along_axis(X.reshape(B, N, C), np.asarray(yarg, np.int64)[:, None, :], 1)[:, 0]
    dz = (np.asarray(dout, F32) * act_grad(fma32(v, sc, sh), act, mut)).astype(F32)
    xhat = ((v - mu).astype(F32) * is_).astype(F32)
    t2 = dz.astype(F64) * xhat.astype(F64)
    if guard is not None:
        guard.sum64("sum dz", dz)
        guard.sum64("sum dz*xhat", t2)
    coef = _coef(dz.astype(F64).sum(0), t2.sum(0), B * N, sc, mu, is_, training, guard, mut)
    ca, cb = coef[:C], coef[C:]
    hit = np.arange(N)[None, :, None] == np.asarray(yarg)[:, None, :]
    top = np.where(hit, (sc * dz).astype(F32)[:, None, :], F32(0.0)).astype(F32)
    dx = ((top - ca).astype(F32) - (cb * X.reshape(B, N, C)).astype(F32)).astype(F32).reshape(B * N, C)
    return {"bsums": np.concatenate([dz.astype(F64).sum(0), t2.sum(0)]).astype(F32), "dx": dx, "dz": dz, "coef": coef}
