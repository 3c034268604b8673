"""The BatchNorm entry points (csrc/bnact.hip) straight through the C ABI for tests/test_gpu_bn.py.  Every output and every scratch
buffer is a `Banded` slice (tests/wgs_worker.py) of a sentinel-filled allocation: the margins must be intact after a call, no sentinel
may be left inside an output, and sentinels must be left exactly where include/pdgn_hip.h says a call does not write.  Every function
returns bit patterns (uint32) unless it says otherwise; `twice` runs a call a second time and demands the same bytes."""
import numpy as np
import torch

from wgs_worker import INVALID, SENT_NAN, Banded, _api, _sync, bits, dev  # noqa: F401  (re-exported)


def _opt(a):
    return dev(a) if a is not None else None


def _filled(a, floats=True):
    """A Banded buffer holding `a`."""
    a = np.ascontiguousarray(a)
    b = Banded(a.size, floats)
    b.t.copy_(torch.from_numpy(a.reshape(-1)))
    return b


def _whole(what, *bufs):
    for b in bufs:
        assert b.margins_intact(), "%s wrote outside a buffer" % what
    for b in bufs:
        assert b.sentinels_left() == 0, "%s left %d elements of an output unwritten" % (what, b.sentinels_left())


def twice(fn, *args, **kw):
    first, second = fn(*args, **kw), fn(*args, **kw)
    for a, b in zip(first, second):
        assert np.array_equal(a, b), "%s: a second run gives other bytes" % fn.__name__
    return first


def _stats_out(C, run):
    stats = Banded(4 * C, True)
    rm, rv = (_filled(run["rm"]), _filled(run["rv"])) if run is not None else (None, None)
    return stats, rm, rv


# ---------------------------------------------------------------------------- statistics
def device_stats(X, p, run, eps, momentum):
    """pdgn_bn_stats -> stats (4C), running_mean, running_var bits and the gy partial rows (gy, 2C) as float32.  The 2C floats behind
    the partial rows belong to the backward's coefficients and stay untouched."""
    import bn_mirror as bm
    L, ptr, stream = _api()
    R, C = X.shape
    gy = bm.cl_geometry(R, C)[2]
    floats = L.pdgn_bn_scratch_floats(R, C)
    assert floats == gy * 2 * C + 2 * C
    x, scr = dev(X), Banded(floats, True)
    stats, rm, rv = _stats_out(C, run)
    g, b, pb = _opt(p["gamma"]), _opt(p["beta"]), _opt(p["pre_bias"])
    _sync(L.pdgn_bn_stats(R, C, eps, momentum, ptr(x), ptr(g), ptr(b), ptr(pb), ptr(rm.t), ptr(rv.t), ptr(scr.t), ptr(stats.t), stream), "pdgn_bn_stats")
    _whole("pdgn_bn_stats", stats, rm, rv)
    assert scr.margins_intact() and scr.sentinels_left(0, gy * 2 * C) == 0
    assert scr.sentinels_left(gy * 2 * C) == 2 * C, "pdgn_bn_stats wrote the coefficient row behind its partial rows"
    return stats.bits(), rm.bits(), rv.bits(), scr.t[:gy * 2 * C].cpu().numpy().reshape(gy, 2 * C)


def device_from_partials(part, R, C, p, run, eps, momentum):
    """pdgn_bn_stats_from_partials on uploaded raw partial rows (gy, 2C)."""
    L, ptr, stream = _api()
    d = dev(part)
    stats, rm, rv = _stats_out(C, run)
    g, b, pb = _opt(p["gamma"]), _opt(p["beta"]), _opt(p["pre_bias"])
    _sync(L.pdgn_bn_stats_from_partials(R, C, eps, momentum, ptr(g), ptr(b), ptr(pb), ptr(rm.t), ptr(rv.t), ptr(d), ptr(stats.t), stream),
          "pdgn_bn_stats_from_partials")
    _whole("pdgn_bn_stats_from_partials", stats, rm, rv)
    return stats.bits(), rm.bits(), rv.bits()


def device_from_blocks(part, R, C, block_rows, p, run, eps, momentum, with_scratch=True):
    """pdgn_bn_stats_from_gemm_partials on uploaded block-shifted partial rows (nparts, 3C), spare rows included.  The fp64 scratch
    (pdgn_bn_blocks_scratch_doubles elements, or NULL) is banded too: the first launch must fill all of it."""
    import bn_mirror as bm
    L, ptr, stream = _api()
    nparts = part.shape[0]
    nd = L.pdgn_bn_blocks_scratch_doubles(C, nparts)
    assert nd == bm.blocks_scratch_doubles(C, nparts)
    d = dev(part)
    scr = Banded(2 * nd, True) if (with_scratch and nd > 0) else None
    stats, rm, rv = _stats_out(C, run)
    g, b, pb = _opt(p["gamma"]), _opt(p["beta"]), _opt(p["pre_bias"])
    _sync(L.pdgn_bn_stats_from_gemm_partials(R, C, nparts, block_rows, eps, momentum, ptr(g), ptr(b), ptr(pb), ptr(rm.t) if rm else None,
                                             ptr(rv.t) if rv else None, ptr(d), ptr(stats.t), ptr(scr.t) if scr else None, stream),
          "pdgn_bn_stats_from_gemm_partials")
    _whole("pdgn_bn_stats_from_gemm_partials", stats, *([rm, rv] if rm else []))
    if scr is not None:
        assert scr.margins_intact(), "pdgn_bn_stats_from_gemm_partials wrote outside its scratch"
        left = scr.ints.view(-1, 2)
        assert not bool(((left[:, 0] == SENT_NAN) & (left[:, 1] == SENT_NAN)).any()), "a slice left its scratch row unwritten"
    return (stats.bits(),) + ((rm.bits(), rv.bits()) if rm else ())


def device_blocks_refused(rows, c, nparts, block_rows):
    L, ptr, stream = _api()
    part = torch.zeros(4096, device="cuda")
    stats, scr, rm, rv = Banded(1024, True), Banded(1024, True), Banded(1024, True), Banded(1024, True)
    rc = L.pdgn_bn_stats_from_gemm_partials(rows, c, nparts, block_rows, 1e-5, 0.1, None, None, None, ptr(rm.t), ptr(rv.t), ptr(part), ptr(stats.t),
                                            ptr(scr.t), stream)
    torch.cuda.synchronize()
    return rc, all(b.sentinels_left() == 1024 and b.margins_intact() for b in (stats, scr, rm, rv))


def device_eval(C, p, run, eps):
    """pdgn_bn_eval_stats -> stats bits; the running buffers are inputs and must not change."""
    L, ptr, stream = _api()
    stats, rm, rv = _stats_out(C, run)
    g, b, pb = _opt(p["gamma"]), _opt(p["beta"]), _opt(p["pre_bias"])
    _sync(L.pdgn_bn_eval_stats(C, eps, ptr(g), ptr(b), ptr(pb), ptr(rm.t), ptr(rv.t), ptr(stats.t), stream), "pdgn_bn_eval_stats")
    _whole("pdgn_bn_eval_stats", stats, rm, rv)
    assert np.array_equal(rm.bits(), bits(run["rm"])) and np.array_equal(rv.bits(), bits(run["rv"]))
    return (stats.bits(),)


# ---------------------------------------------------------------------------- apply, backward
def device_forward(X, stats, act, mul, inter):
    L, ptr, stream = _api()
    R, C = X.shape
    x, s, m = dev(X), dev(stats), _opt(mul)
    y = Banded(R * C, True)
    _sync(L.pdgn_bn_act_forward(R, C, act, ptr(x), ptr(s), ptr(m), ptr(y.t), inter, stream), "pdgn_bn_act_forward")
    _whole("pdgn_bn_act_forward", y)
    return (y.bits().reshape((2 * R, C // 2) if inter else (R, C)),)


def device_backward(X, dy, stats, act, training, mul, inter, want_dmul=True):
    """pdgn_bn_act_backward -> bsums (2C), dx (R, C), dmul (R, C) | None, and the coefficient row [ca | cb] the call leaves behind
    the gy partial rows of its scratch."""
    import bn_mirror as bm
    L, ptr, stream = _api()
    R, C = X.shape
    gy = bm.cl_geometry(R, C)[2]
    x, g, s, m = dev(X), dev(dy), dev(stats), _opt(mul)
    scr, bs, dx = Banded(L.pdgn_bn_scratch_floats(R, C), True), Banded(2 * C, True), Banded(R * C, True)
    dmul = Banded(R * C, True) if want_dmul else None
    _sync(L.pdgn_bn_act_backward(R, C, act, int(training), ptr(x), ptr(g), ptr(m), ptr(s), ptr(scr.t), ptr(bs.t), ptr(dx.t),
                                 ptr(dmul.t) if want_dmul else None, inter, stream), "pdgn_bn_act_backward")
    _whole("pdgn_bn_act_backward", scr, bs, dx, *([dmul] if want_dmul else []))
    out = (bs.bits(), dx.bits().reshape(R, C), scr.bits()[gy * 2 * C:])
    return out + ((dmul.bits().reshape(R, C),) if want_dmul else ())


def device_apply_refused(rows, c, inter, mul):
    """Both entry points: PDGN_ERR_INVALID, nothing touched."""
    L, ptr, stream = _api()
    act = 3 if mul == "act3" else 1
    x = torch.zeros(4096, device="cuda")
    m = x if mul is True else None
    bufs = [Banded(1024, True) for _ in range(5)]
    y, scr, bs, dx, dmul = bufs
    rc1 = L.pdgn_bn_act_forward(rows, c, act, ptr(x), ptr(x), ptr(m), ptr(y.t), inter, stream)
    rc2 = L.pdgn_bn_act_backward(rows, c, act, 1, ptr(x), ptr(x), ptr(m), ptr(x), ptr(scr.t), ptr(bs.t), ptr(dx.t), ptr(dmul.t), inter, stream)
    torch.cuda.synchronize()
    return rc1, rc2, all(b.sentinels_left() == 1024 and b.margins_intact() for b in bufs)


# ---------------------------------------------------------------------------- max-pool tails
def device_maxpool_apply(X, stats, act, b, n):
    """pdgn_bn_act_maxpool -> ymax bits (b, c), yarg (b, c) int32."""
    L, ptr, stream = _api()
    c = X.shape[1]
    x, s = dev(X), dev(stats)
    floats = L.pdgn_bn_maxpool_scratch_floats(b, c)
    assert floats == 2 * b * 16 * c
    scr, ymax, yarg = Banded(floats, True), Banded(b * c, True), Banded(b * c, False)
    _sync(L.pdgn_bn_act_maxpool(b, n, c, act, ptr(x), ptr(s), ptr(scr.t), ptr(ymax.t), ptr(yarg.t), stream), "pdgn_bn_act_maxpool")
    _whole("pdgn_bn_act_maxpool", ymax, yarg)
    assert scr.margins_intact()
    return ymax.bits().reshape(b, c), yarg.ints.cpu().numpy().reshape(b, c)


def device_maxpool_onepass(X, p, run, act, b, n, eps, momentum):
    """pdgn_bn_stats_act_maxpool -> stats, running_mean, running_var, ymax bits; yarg int32."""
    L, ptr, stream = _api()
    c = X.shape[1]
    x = dev(X)
    floats = L.pdgn_bn_stats_maxpool_scratch_floats(b, c)
    assert floats == 6 * b * 16 * c
    scr, ymax, yarg = Banded(floats, True), Banded(b * c, True), Banded(b * c, False)
    stats, rm, rv = _stats_out(c, run)
    g, be, pb = _opt(p["gamma"]), _opt(p["beta"]), _opt(p["pre_bias"])
    _sync(L.pdgn_bn_stats_act_maxpool(b, n, c, act, eps, momentum, ptr(x), ptr(g), ptr(be), ptr(pb), ptr(rm.t), ptr(rv.t), ptr(scr.t),
                                      ptr(stats.t), ptr(ymax.t), ptr(yarg.t), stream), "pdgn_bn_stats_act_maxpool")
    _whole("pdgn_bn_stats_act_maxpool", stats, rm, rv, ymax, yarg)
    assert scr.margins_intact()
    return stats.bits(), rm.bits(), rv.bits(), ymax.bits().reshape(b, c), yarg.ints.cpu().numpy().reshape(b, c)


def device_maxpool_backward(X, dout, yarg, stats, act, training, b, n):
    """pdgn_bn_act_maxpool_backward -> bsums (2c), dx (b*n, c), and its scratch [dz (b, c) | ca | cb]."""
    L, ptr, stream = _api()
    c = X.shape[1]
    x, d, a, s = dev(X), dev(dout), dev(yarg), dev(stats)
    scr, bs, dx = Banded(b * c + 2 * c, True), Banded(2 * c, True), Banded(b * n * c, True)
    _sync(L.pdgn_bn_act_maxpool_backward(b, n, c, act, int(training), ptr(x), ptr(d), ptr(a), ptr(s), ptr(scr.t), ptr(bs.t), ptr(dx.t), stream),
          "pdgn_bn_act_maxpool_backward")
    _whole("pdgn_bn_act_maxpool_backward", scr, bs, dx)
    return bs.bits(), dx.bits().reshape(b * n, c), scr.bits()


def device_maxpool_refused(b, n, c, act):
    """All three entry points: PDGN_ERR_INVALID; yarg, ymax, stats, dx and the scratch untouched."""
    L, ptr, stream = _api()
    x = torch.zeros(4096, device="cuda")
    arg = torch.zeros(4096, dtype=torch.int32, device="cuda")
    bufs = [Banded(1024, True) for _ in range(7)] + [Banded(1024, False)]
    scr, ymax, stats, rm, rv, bs, dx, yarg = bufs
    rcs = (L.pdgn_bn_act_maxpool(b, n, c, act, ptr(x), ptr(x), ptr(scr.t), ptr(ymax.t), ptr(yarg.t), stream),
           L.pdgn_bn_stats_act_maxpool(b, n, c, act, 1e-5, 0.1, ptr(x), None, None, None, ptr(rm.t), ptr(rv.t), ptr(scr.t), ptr(stats.t),
                                       ptr(ymax.t), ptr(yarg.t), stream),
           L.pdgn_bn_act_maxpool_backward(b, n, c, act, 1, ptr(x), ptr(x), ptr(arg), ptr(x), ptr(scr.t), ptr(bs.t), ptr(dx.t), stream))
    torch.cuda.synchronize()
    return rcs, all(b_.sentinels_left() == 1024 and b_.margins_intact() for b_ in bufs)
