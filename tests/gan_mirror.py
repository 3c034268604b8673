"""The hinge and the non-saturating logistic GAN terms (include/pdgn_hip.h: pdgn_gan_term, _count, _backward)
restated on the host in numpy.  `term` / `term_grad` compute in fp32 with every operation its own rounding and the kernel's summation
order -- thread t of 1024 adds its elements t, t + 1024, ... in that order, a xor butterfly 32 .. 1 over each wave of 64, then the
sixteen wave totals in index order --, which for the hinge (additions, comparisons and one division: all correctly rounded) is the
kernel's result bit for bit; for the logistic kind they use numpy's fp32 exp / log1p and are close, not equal.  `term64` /
`term_grad64` are the fp64 closed forms, the reference of the logistic kind.  `counts` is what pdgn_gan_term_count stores."""
import numpy as np

KINDS = {"hinge": 1, "logistic": 2}
ROLES = {"d_real": 0, "d_fake": 1, "g": 2}
THREADS, WAVE = 1024, 64
F32 = np.float32


def _check(kind, role):
    if kind not in KINDS or role not in ROLES:
        raise ValueError("kind %r / role %r" % (kind, role))


def _f32(x, kind, role):
    """f(x) elementwise in fp32."""
    x = np.asarray(x, dtype=F32).reshape(-1)
    with np.errstate(all="ignore"):
        if kind == "hinge":
            if role == "g":
                return -x
            v = (F32(1) - x) if role == "d_real" else (F32(1) + x)
            return np.where(v > 0, v, np.where(v == v, F32(0), v)).astype(F32)
        t = x if role == "d_fake" else -x
        soft = np.log1p(np.exp(-np.abs(t)).astype(F32)).astype(F32)
        return (np.where(t > 0, t, F32(0)).astype(F32) + soft).astype(F32)      # fmaxf(t, 0): 0 for a NaN t, soft carries the NaN


def block_sum(f):
    """The kernel's fp32 sum of the terms f, in its order."""
    f = np.asarray(f, dtype=F32).reshape(-1)
    acc = np.zeros(THREADS, dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(0, f.size, THREADS):
            chunk = f[k:k + THREADS]
            acc[:chunk.size] = acc[:chunk.size] + chunk
        v = acc.reshape(THREADS // WAVE, WAVE)
        lanes = np.arange(WAVE)
        off = WAVE // 2
        while off:
            v = (v + v[:, lanes ^ off]).astype(F32)
            off >>= 1
        s = F32(0)
        for w in range(THREADS // WAVE):
            s = F32(s + v[w, 0])
    return s


def term(x, kind, role, scale=1.0):
    """out[0] of pdgn_gan_term as an fp32 scalar."""
    _check(kind, role)
    f = _f32(x, kind, role)
    with np.errstate(all="ignore"):
        return F32(F32(scale) * F32(block_sum(f) / F32(f.size)))


def _sigmoid32(t):
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(t)).astype(F32)
        return np.where(t >= 0, F32(1) / (F32(1) + e), e / (F32(1) + e)).astype(F32)


def term_grad(x, kind, role, scale=1.0, g=1.0):
    """dx of pdgn_gan_term_backward, fp32, in x's shape flattened."""
    _check(kind, role)
    x = np.asarray(x, dtype=F32).reshape(-1)
    with np.errstate(all="ignore"):
        c = F32(F32(F32(g) * F32(scale)) / F32(x.size))
        if kind == "hinge":
            if role == "g":
                d = np.where(x == x, F32(-1), x)
            else:
                v = (F32(1) - x) if role == "d_real" else (F32(1) + x)
                d = np.where(v > 0, F32(-1) if role == "d_real" else F32(1), np.where(v == v, F32(0), v))
        else:
            d = _sigmoid32(x) if role == "d_fake" else -_sigmoid32(-x)
        return (c * d.astype(F32)).astype(F32)


def _f64(x, kind, role):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        if kind == "hinge":
            if role == "g":
                return -x
            v = 1.0 - x if role == "d_real" else 1.0 + x
            return np.where(v > 0, v, np.where(v == v, 0.0, v))
        return np.logaddexp(0.0, x if role == "d_fake" else -x)


def term64(x, kind, role, scale=1.0):
    """scale * mean f(x) in fp64 from the (fp32) scores: the closed form."""
    _check(kind, role)
    f = _f64(x, kind, role)
    with np.errstate(all="ignore"):
        return np.float64(scale) * (f.sum() / np.float64(f.size))


def _sigmoid64(t):
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(t))
        return np.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def term_grad64(x, kind, role, scale=1.0, g=1.0):
    """g * scale / n * f'(x) in fp64; the hinge's kink has derivative 0."""
    _check(kind, role)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        c = np.float64(g) * np.float64(scale) / np.float64(x.size)
        if kind == "hinge":
            if role == "g":
                d = np.where(x == x, -1.0, x)
            else:
                v = 1.0 - x if role == "d_real" else 1.0 + x
                d = np.where(v > 0, -1.0 if role == "d_real" else 1.0, np.where(v == v, 0.0, v))
        else:
            d = _sigmoid64(x) if role == "d_fake" else -_sigmoid64(-x)
        return c * d


def counts(x, boundary=0.0):
    """(pos, neg, n) of fp32 scores: a score equal to the boundary and a NaN count to neither."""
    x = np.asarray(x, dtype=F32).reshape(-1)
    b = F32(boundary)
    with np.errstate(invalid="ignore"):
        return int((x > b).sum()), int((x < b).sum()), int(x.size)
