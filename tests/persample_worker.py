"""The per-sample layer kernels (csrc/skinny.hip, csrc/small_mlp.hip) straight through the C ABI for tests/test_gpu_persample.py.
Every output is the interior of a `Pitched` buffer: rows x cols floats inside a sentinel-filled allocation of rows + 2 rows of `ld`
floats with Banded's margins (tests/wgs_worker.py) around it.  After a call the interior must hold no sentinel, and the pitch gap, the
rows past R and the margins must hold nothing else.  Operands are uploaded in their own pitch with NaN in the gap (an element a
kernel must not read).  Every function returns a dict of bit patterns (uint32); `twice` runs a call a second time and demands the same
bytes."""
import ctypes

import numpy as np
import torch

from persample_cases import pad4, pitched
from wgs_worker import SENT_NAN, Banded, _api, _sync, bits, dev  # noqa: F401  (re-exported)

EXTRA_ROWS = 2


class Pitched:
    def __init__(self, rows, cols, ld=None, zero=False):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.band = Banded((rows + EXTRA_ROWS) * self.ld, True)
        self.grid = self.band.ints.view(rows + EXTRA_ROWS, self.ld)
        self.t = self.band.t
        if zero:                                                    # (pdgn_skinny_nn adds into a zero-filled C)
            self.band.t.view(rows + EXTRA_ROWS, self.ld)[:rows, :cols] = 0.0

    def check(self, what):
        assert self.band.margins_intact(), "%s wrote outside a buffer" % what
        inside = int((self.grid[:self.rows, :self.cols] == SENT_NAN).sum())
        assert inside == 0, "%s left %d elements of an output unwritten" % (what, inside)
        outside = int((self.grid == SENT_NAN).sum())
        want = self.grid.numel() - self.rows * self.cols
        assert outside == want, "%s wrote %d elements past its rows or columns" % (what, want - outside)

    def untouched(self):
        return self.band.margins_intact() and int((self.grid == SENT_NAN).sum()) == self.grid.numel()

    def bits(self):
        return self.grid[:self.rows, :self.cols].cpu().numpy().view(np.uint32)


def _opt(a):
    return dev(a) if a is not None else None


def twice(fn, *args, **kw):
    first, second = fn(*args, **kw), fn(*args, **kw)
    for k in first:
        assert (first[k] is None and second[k] is None) or np.array_equal(first[k], second[k]), \
            "%s: a second run gives other bytes in %s" % (fn.__name__, k)
    return first


# ---------------------------------------------------------------------------- csrc/skinny.hip
def call_nt(A, B, bias, pads, act, entry):
    """pdgn_skinny_nt (entry "nt") / pdgn_skinny_nt_act: A (R, K), B (N, K) -> C (R, N)."""
    L, ptr, stream = _api()
    (R, K), N = A.shape, B.shape[0]
    lda, ldb, ldc = K + pads[0], K + pads[1], N + pads[2]
    a, b, bi = dev(pitched(A, lda)), dev(pitched(B, ldb)), _opt(bias)
    C = Pitched(R, N, ldc)
    if entry == "nt":
        assert act == 0
        rc = L.pdgn_skinny_nt(R, N, K, ptr(a), lda, ptr(b), ldb, ptr(bi), ptr(C.t), ldc, stream)
    else:
        rc = L.pdgn_skinny_nt_act(R, N, K, ptr(a), lda, ptr(b), ldb, ptr(bi), ptr(C.t), ldc, act, stream)
    _sync(rc, "pdgn_skinny_" + entry)
    C.check("pdgn_skinny_" + entry)
    return dict(C=C.bits())


def call_nn(A, B, P, pads, act):
    """pdgn_skinny_nn (P None) / pdgn_skinny_nn_masked: A (R, K), B (K, N), P (R, K) -> C (R, N), zero-filled before the call."""
    L, ptr, stream = _api()
    (R, K), N = A.shape, B.shape[1]
    lda, ldp, ldb, ldc = pad4(K) + pads[0], K + pads[1], N + pads[2], N + pads[3]
    a, b = dev(pitched(A, lda)), dev(pitched(B, ldb))
    C = Pitched(R, N, ldc, zero=True)
    if P is None:
        rc, what = L.pdgn_skinny_nn(R, N, K, ptr(a), lda, ptr(b), ldb, ptr(C.t), ldc, stream), "pdgn_skinny_nn"
    else:
        p = dev(pitched(P, ldp))
        rc = L.pdgn_skinny_nn_masked(R, N, K, ptr(a), lda, ptr(p), ldp, act, ptr(b), ldb, ptr(C.t), ldc, stream)
        what = "pdgn_skinny_nn_masked"
    _sync(rc, what)
    C.check(what)
    return dict(C=C.bits())


def call_tn(A, B, pads):
    """pdgn_skinny_tn: A (R, N), B (R, K) -> C (N, K), a column slice of a wider matrix."""
    L, ptr, stream = _api()
    (R, N), K = A.shape, B.shape[1]
    lda, ldb, ldc = N + pads[0], K + pads[1], K + pads[2]
    a, b = dev(pitched(A, lda)), dev(pitched(B, ldb))
    C = Pitched(N, K, ldc)
    _sync(L.pdgn_skinny_tn(R, N, K, ptr(a), lda, ptr(b), ldb, ptr(C.t), ldc, stream), "pdgn_skinny_tn")
    C.check("pdgn_skinny_tn")
    return dict(C=C.bits())


# ---------------------------------------------------------------------------- csrc/small_mlp.hip
def _holding(a):
    p = Pitched(1, a.size)
    p.band.t.view(1 + EXTRA_ROWS, a.size)[0].copy_(torch.from_numpy(np.array(a)))       # (a copy: the cached operands are read-only)
    return p


def call_sm_forward(act, bn, eps, momentum, x, W, bias, gamma, beta, rm, rv, saved=True):
    """pdgn_small_mlp_forward -> y, pre, stat, rm, rv (None where not asked for); saved=False hands pre = stat = NULL."""
    L, ptr, stream = _api()
    (R, K), N = x.shape, W.shape[0]
    xd, Wd = dev(x), dev(W)
    bi, g, b = _opt(bias), _opt(gamma), _opt(beta)
    rmb, rvb = (_holding(rm), _holding(rv)) if rm is not None else (None, None)
    y = Pitched(R, N)
    pre = Pitched(R, N) if saved else None
    stat = Pitched(1, 2 * N) if (saved and bn) else None
    rc = L.pdgn_small_mlp_forward(R, K, N, act, bn, eps, momentum, ptr(xd), ptr(Wd), ptr(bi), ptr(g), ptr(b),
                                  ptr(rmb.t) if rmb else None, ptr(rvb.t) if rvb else None, ptr(y.t), ptr(pre.t) if pre else None,
                                  ptr(stat.t) if stat else None, stream)
    _sync(rc, "pdgn_small_mlp_forward")
    for buf in (y, pre, stat, rmb, rvb):
        if buf is not None:
            buf.check("pdgn_small_mlp_forward")
    return dict(y=y.bits(), pre=pre.bits() if pre else None, stat=stat.bits().reshape(-1) if stat else None,
                rm=rmb.bits().reshape(-1) if rmb else None, rv=rvb.bits().reshape(-1) if rvb else None)


def call_sm_backward(act, bn, x, dy, pre, stat, gamma, beta, nulls=()):
    """pdgn_small_mlp_backward -> dpre, dgamma, dbeta, dbias, dW; `nulls` names the outputs handed as NULL (dgamma / dbeta are
    NULL without BatchNorm anyway: the kernel has nothing to write there)."""
    L, ptr, stream = _api()
    (R, K), N = x.shape, dy.shape[1]
    xd, dyd, pd, sd, g, b = dev(x), dev(dy), dev(pre), _opt(stat), _opt(gamma), _opt(beta)
    out = dict(dpre=Pitched(R, N), dgamma=Pitched(1, N) if bn else None, dbeta=Pitched(1, N) if bn else None, dbias=Pitched(1, N),
               dW=Pitched(N, K))
    for name in nulls:
        out[name] = None
    p = lambda buf: ptr(buf.t) if buf is not None else None         # noqa: E731
    rc = L.pdgn_small_mlp_backward(R, K, N, act, bn, ptr(xd), ptr(dyd), ptr(pd), ptr(sd), ptr(g), ptr(b), p(out["dpre"]),
                                   p(out["dgamma"]), p(out["dbeta"]), p(out["dbias"]), p(out["dW"]), stream)
    _sync(rc, "pdgn_small_mlp_backward")
    for buf in out.values():
        if buf is not None:
            buf.check("pdgn_small_mlp_backward")
    return {k: (v.bits().reshape(-1) if k in ("dgamma", "dbeta", "dbias") else v.bits()) if v is not None else None
            for k, v in out.items()}


# ---------------------------------------------------------------------------- refusals
def call_refused(entry, kind):
    """One refused argument list -> (return code, every output untouched).  Every entry point returns before a launch on these
    (the argument checks are the first statements of the entry points in csrc/skinny.hip and csrc/small_mlp.hip)."""
    L, ptr, stream = _api()
    zeros = torch.zeros(64 * 640, device="cuda")
    outs = [Pitched(32, 32) for _ in range(7)]
    o = [ptr(b.t) for b in outs]
    z = ptr(zeros)
    off4 = ctypes.c_void_p(zeros.data_ptr() + 4)
    R = {"R0": 0, "R65": 65}.get(kind, 8)
    act = {"act3": 3, "act0": 0}.get(kind, 2)
    if entry in ("nt", "act"):
        K, N, lda = (6 if kind == "K_mod4" else 8), 8, {"lda_short": 4, "pitch_mod4": 9}.get(kind, 8)
        A, B = (off4 if kind == "misaligned" else z), (None if kind == "null_operand" else z)
        if entry == "nt":
            rc = L.pdgn_skinny_nt(R, N, K, A, lda, B, 8, None, o[0], 8, stream)
        else:
            rc = L.pdgn_skinny_nt_act(R, N, K, A, lda, B, 8, None, o[0], 8, act, stream)
    elif entry in ("nn", "nnm"):
        K, N, lda = 8, (6 if kind == "N_mod4" else 8), {"lda_short": 4, "pitch_mod4": 9}.get(kind, 8)
        A = off4 if kind == "misaligned" else z
        if entry == "nn":
            rc = L.pdgn_skinny_nn(R, N, K, None if kind == "null_operand" else A, lda, z, 8, o[0], 8, stream)
        else:
            rc = L.pdgn_skinny_nn_masked(R, N, K, A, lda, None if kind == "null_operand" else z, 8, act, z, 8, o[0], 8, stream)
    elif entry == "tn":
        rc = L.pdgn_skinny_tn(R, 8, 8, z, 4 if kind == "lda_short" else 8, None if kind == "null_operand" else z, 8, o[0], 8, stream)
    else:
        r, k = (64, 636) if kind == "beyond_sm_ok" else (R, 8)
        if entry == "smf":
            bn = 2 if kind == "bn2_no_running" else 1
            rm, rv = (None, None) if kind == "bn2_no_running" else (o[1], o[2])
            rc = L.pdgn_small_mlp_forward(r, k, 8, act, bn, 1e-5, 0.1, z, z, None, None, None, rm, rv, o[0], o[3], o[4], stream)
        else:
            rc = L.pdgn_small_mlp_backward(r, k, 8, act, 1, z, z, z, None if kind == "bn_no_stat" else z, None, None, o[0], o[1], o[2],
                                           o[3], o[4], stream)
    torch.cuda.synchronize()
    return rc, all(b.untouched() for b in outs)
