"""GPU: the hinge and the non-saturating logistic GAN objectives -- pdgn_gan_term, _count and _backward called
directly on guard-banded buffers against the numpy restatement (tests/gan_mirror.py: bit for bit for the hinge, the fp64 closed form for
the logistic kind), NaN and infinities, the counts, autograd against torch ops, the refusals, and the trainer: every call site of both
schedules, the launch list, the adaptive augmentation's boundary, and the default's twelve mse_const calls.

Largest errors measured on an MI355X with this file's inputs (all n, all roles, both scales; every test prints its own):
logistic forward |out - term64| / |term64| 1.40e-7 (n = 1025; bound 2e-6), logistic backward max_i |dx_i - term_grad64_i| / |term_grad64_i|
2.09e-7 (n = 4097; bound 1e-6).  At x = +-100 the vanishing side of the logistic gradient is c * 3.78e-44, an fp32 denormal, not 0: the
fp64 closed form is that number too (sigma(-100) = 3.7e-44), so these elements -- the only ones where the closed form is below 1e-37, with
those at +-3e38 where it is 0 -- are held to the closed form within three steps of the denormal grid, or to an exact 0."""
import ctypes

import numpy as np
import pytest
import torch

import gan_mirror as gm

pytestmark = pytest.mark.gpu
GUARD = 64
SENTINEL_F, SENTINEL_I = -12345.0, -777
SEED = 4242
EVERYTHING = dict(rot_max_deg=180.0, scale_max=1.25, flip=True, trans_max=0.1, jitter_sigma=0.0)
PAIRS = [(k, r) for k in ("hinge", "logistic") for r in ("d_real", "d_fake", "g")]
FWD_N = [1, 35, 63, 64, 65, 1023, 1024, 1025, 4097]
BWD_N = FWD_N + [16385]                                          # one past 64 blocks of 256: the grid-stride loop turns
FWD_REL, BWD_REL = 2e-6, 1e-6                                    # the logistic kind against the fp64 closed form
DENORMAL = 2.0 ** -149                                           # the spacing of fp32 below 2^-126
ONE = np.float32(1)
PLANTED = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(ONE, np.float32(2)), np.nextafter(ONE, np.float32(0)), np.nextafter(-ONE, np.float32(-2)),
                    np.nextafter(-ONE, np.float32(0)), 1e-30, -1e-30, 100.0, -100.0, 3e38, -3e38], dtype=np.float32)
HUGE = slice(12, 14)                                             # the two planted values that swamp an fp32 sum


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _scores(n, seed, huge=True):
    """fp32 scores ~ N(0, 2); the leading ones are the planted values (as many as n has room for): +-0, +-1 exactly and their fp32
    neighbours on both sides, +-1e-30, +-100, +-3e38.  huge=False: without the last pair, under which a sum says little about the rest."""
    x = np.random.default_rng(seed).normal(0.0, 2.0, n).astype(np.float32)
    sp = PLANTED if huge else PLANTED[:HUGE.start]
    x[:min(n, sp.size)] = sp[:min(n, sp.size)]
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _forward(x, kind, role, scale, dev, boundary=None, prefill=None):
    """pdgn_gan_term (boundary None) or pdgn_gan_term_count on guard-banded `out` and slot -> (out as fp32, the slot's first three words)."""
    from pdgn_amd import _lib
    out_whole = torch.full((2 * GUARD + 1,), SENTINEL_F, dtype=torch.float32, device=dev)
    slot_whole = torch.full((2 * GUARD + 4,), SENTINEL_I, dtype=torch.int32, device=dev)
    out, slot = out_whole[GUARD:GUARD + 1], slot_whole[GUARD:GUARD + 4]
    if prefill is not None:
        slot[:3] = torch.tensor(prefill, dtype=torch.int32, device=dev)
    L, k, r = _lib.lib(), gm.KINDS[kind], gm.ROLES[role]
    if boundary is None:
        rc = L.pdgn_gan_term(x.numel(), _lib.ptr(x), k, r, scale, _lib.ptr(out), _lib.stream_of(x))
    else:
        rc = L.pdgn_gan_term_count(x.numel(), _lib.ptr(x), k, r, scale, boundary, _lib.ptr(out), _lib.ptr(slot), _lib.stream_of(x))
    torch.cuda.synchronize()
    assert rc == 0
    ow, sw = out_whole.cpu().numpy(), slot_whole.cpu().numpy()
    assert (ow[:GUARD] == SENTINEL_F).all() and (ow[GUARD + 1:] == SENTINEL_F).all()
    if boundary is None:
        assert (sw == SENTINEL_I).all()
        return ow[GUARD], None
    assert (sw[:GUARD] == SENTINEL_I).all() and (sw[GUARD + 3:] == SENTINEL_I).all()         # word 3 of the slot and everything around it
    return ow[GUARD], tuple(int(v) for v in sw[GUARD:GUARD + 3])


def _backward(x, kind, role, scale, g, dev):
    """pdgn_gan_term_backward into a guard-banded dx -> dx as numpy fp32."""
    from pdgn_amd import _lib
    n = x.numel()
    whole = torch.full((2 * GUARD + n,), SENTINEL_F, dtype=torch.float32, device=dev)
    dx = whole[GUARD:GUARD + n]
    gt = torch.tensor([g], dtype=torch.float32, device=dev)
    rc = _lib.lib().pdgn_gan_term_backward(n, _lib.ptr(x), gm.KINDS[kind], gm.ROLES[role], scale, _lib.ptr(gt), _lib.ptr(dx), _lib.stream_of(x))
    torch.cuda.synchronize()
    assert rc == 0
    w = whole.cpu().numpy()
    assert (w[:GUARD] == SENTINEL_F).all() and (w[GUARD + n:] == SENTINEL_F).all()
    return w[GUARD:GUARD + n].copy()


def _rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


# ---------------------------------------------------------------------------- 1. the kernels against the mirror
@pytest.mark.parametrize("n", FWD_N)
def test_forward_is_the_mirror_bit_for_bit_for_the_hinge_and_the_closed_form_for_the_logistic_kind(n):
    dev = _dev()
    worst = 0.0
    for huge in (True, False):
        host = _scores(n, n, huge)
        x = torch.from_numpy(host).to(dev)
        for kind, role in PAIRS:
            for scale in (1.0, 0.375):
                out, _ = _forward(x, kind, role, scale, dev)
                counted, triple = _forward(x, kind, role, scale, dev, boundary=0.0, prefill=(5, 6, 7))   # stored, not added to
                assert _bits(counted) == _bits(out), (kind, role, n, counted, out)
                assert triple == gm.counts(host, 0.0)
                if kind == "hinge":
                    want = gm.term(host, kind, role, scale)
                    assert _bits(out) == _bits(want), (kind, role, n, scale, out, want)
                else:
                    want = gm.term64(host, kind, role, scale)
                    assert want > 0.0 and np.isfinite(out)       # every term is positive: no cancellation
                    err = _rel(out, want)
                    worst = max(worst, err)
                    assert err <= FWD_REL, (kind, role, n, scale, huge, out, want, err)
    print("logistic forward, n = %d: largest |out - term64| / |term64| = %.3g" % (n, worst))


@pytest.mark.parametrize("n", BWD_N)
def test_backward_is_the_mirror_bit_for_bit_for_the_hinge_and_the_closed_form_for_the_logistic_kind(n):
    dev = _dev()
    host = _scores(n, 1000 + n)
    x = torch.from_numpy(host).to(dev)
    worst = 0.0
    for kind, role in PAIRS:
        for scale, g in ((1.0, 1.0), (0.375, 3.0)):
            dx = _backward(x, kind, role, scale, g, dev)
            if kind == "hinge":
                want = gm.term_grad(host, kind, role, scale, g)
                assert np.array_equal(_bits(dx), _bits(want)), (kind, role, n, np.flatnonzero(_bits(dx) != _bits(want))[:8])
                continue
            want = gm.term_grad64(host, kind, role, scale, g)
            tiny = np.abs(want) < 1e-37
            # The closed form itself is below 1e-37 at exactly the planted saturated scores -- sigma(-100) = 3.7e-44, sigma(-3e38) = 0 --
            # and nowhere else: those are left out of the relative comparison and held to the exact values below instead.
            sat = np.zeros(n, dtype=bool)
            sat[:min(n, PLANTED.size)] = (np.abs(PLANTED[:min(n, PLANTED.size)]) >= 100.0) & ((PLANTED[:min(n, PLANTED.size)] < 0) == (role == "d_fake"))
            assert np.array_equal(tiny, sat), (kind, role, n, np.flatnonzero(tiny != sat)[:8])
            assert not tiny[PLANTED.size:].any()                 # none of the N(0, 2) scores is left out
            err = np.abs(dx[~tiny].astype(np.float64) - want[~tiny]) / np.abs(want[~tiny])
            worst = max(worst, float(err.max()))
            assert err.max() <= BWD_REL, (kind, role, n, int(np.argmax(err)), float(err.max()))
            # saturation: the gradient is exactly 0 or -+1 (times c = g * scale / n).  At +-100 the vanishing side is c * sigma(-100) =
            # c * 3.7e-44, which fp32 can still represent as a denormal: 0 where the device's exp flushes it, the closed form to three
            # steps of the denormal grid (exp, the quotient, the product) where it does not
            c = np.float32(np.float32(np.float32(g) * np.float32(scale)) / np.float32(n))
            for i in range(min(n, PLANTED.size)):
                if abs(PLANTED[i]) < 100.0:
                    continue
                if sat[i]:
                    assert dx[i] == 0.0 or (abs(PLANTED[i]) == 100.0 and abs(float(dx[i]) - want[i]) <= 3 * DENORMAL), (kind, role, n, i, dx[i], want[i])
                else:
                    assert dx[i] == (c if role == "d_fake" else -c), (kind, role, n, i, dx[i], c)
    print("logistic backward, n = %d: largest |dx - term_grad64| / |term_grad64| = %.3g" % (n, worst))


@pytest.mark.parametrize("v", [100.0, -100.0, 3e38, -3e38])
def test_saturated_logistic_scores_give_finite_losses_and_exact_gradients(v):
    """softplus(t) = max(t, 0) to rounding, never inf; the gradient exactly 0 or -+1 -- alone and among ordinary scores."""
    dev = _dev()
    one = np.array([v], dtype=np.float32)
    x = torch.from_numpy(one).to(dev)
    for role, t in (("d_real", -v), ("d_fake", v), ("g", -v)):
        out, _ = _forward(x, "logistic", role, 1.0, dev)
        dx = _backward(x, "logistic", role, 1.0, 1.0, dev)
        assert np.isfinite(out) and abs(float(out) - max(t, 0.0)) <= 2.0 ** -23 * max(t, 0.0) + 1e-37, (v, role, out)
        if t > 0:
            assert dx[0] == (1.0 if role == "d_fake" else -1.0), (v, role, dx)
        else:                                                    # sigma(-100) = 3.7e-44: an fp32 denormal, or 0 where exp flushes it
            ref = gm.term_grad64(one, "logistic", role)[0]
            assert dx[0] == 0.0 or (abs(v) == 100.0 and abs(float(dx[0]) - ref) <= 3 * DENORMAL), (v, role, dx, ref)
        print("logistic %s at x = %g: out = %r, dx = %r" % (role, v, float(out), float(dx[0])))


# ---------------------------------------------------------------------------- 2. NaN and infinities
@pytest.mark.parametrize("kind, role", PAIRS)
def test_a_nan_score_is_a_nan_loss_and_a_nan_gradient_and_infinities_are_the_mirrors(kind, role):
    dev = _dev()
    base = np.random.default_rng(7).normal(0.0, 2.0, 35).astype(np.float32)
    for special in (np.nan, np.inf, -np.inf):
        host = base.copy()
        host[7] = special
        x = torch.from_numpy(host).to(dev)
        out, triple = _forward(x, kind, role, 1.0, dev, boundary=0.0)
        dx = _backward(x, kind, role, 1.0, 1.0, dev)
        assert triple == gm.counts(host, 0.0) and triple[2] == 35
        others = np.delete(dx, 7)
        assert np.isfinite(others).all() and (others != 0).any()
        want_out, want_dx = gm.term(host, kind, role, 1.0), gm.term_grad(host, kind, role, 1.0, 1.0)
        if np.isnan(special):
            assert np.isnan(out) and np.isnan(dx[7]) and np.isnan(want_out) and np.isnan(want_dx[7])
            assert triple[0] + triple[1] == 34                   # the counts leave the NaN out
        elif kind == "hinge":
            assert _bits(out) == _bits(want_out) and np.array_equal(_bits(dx), _bits(want_dx)), (special, out, want_out)
        else:
            assert _bits(dx[7]) == _bits(want_dx[7]) and abs(float(dx[7])) in (0.0, float(np.float32(1) / np.float32(35))), (special, dx[7])
            if np.isinf(want_out):
                assert out == want_out
            else:
                assert _rel(out, gm.term64(host, kind, role, 1.0)) <= FWD_REL
            ref = gm.term_grad64(host, kind, role, 1.0, 1.0)
            assert (np.abs(others - np.delete(ref, 7)) <= BWD_REL * np.abs(np.delete(ref, 7))).all()


# ---------------------------------------------------------------------------- 3. the counts
def test_the_counts_use_the_objectives_boundary():
    from pdgn_amd import losses
    dev = _dev()
    host = np.array([0.25, -0.25, 0.0, -0.0, 0.75, np.nan], dtype=np.float32)
    x = torch.from_numpy(host).to(dev)
    for objective, want in (("hinge", (2, 1, 6)), ("logistic", (2, 1, 6)), ("lsgan", (1, 4, 6))):
        slot = torch.full((4,), SENTINEL_I, dtype=torch.int32, device=dev)
        plain = losses.adversarial(x, objective, "d_real")
        counted = losses.adversarial(x, objective, "d_real", slot)
        torch.cuda.synchronize()
        assert tuple(slot.cpu().tolist()) == want + (SENTINEL_I,), (objective, slot)
        assert want == gm.counts(host, losses.decision_boundary(objective))
        assert np.isnan(plain.item()) and np.isnan(counted.item())
    host = _scores(1025, 5)
    x = torch.from_numpy(host).to(dev)
    for boundary in (0.0, 0.3, -1.0):
        _, triple = _forward(x, "hinge", "d_real", 1.0, dev, boundary=boundary)
        assert triple == gm.counts(host, boundary) and triple[0] + triple[1] <= 1025
    slot = torch.zeros(4, dtype=torch.int32, device=dev)
    losses.gan_term(x, "logistic", "d_real", count=slot)
    assert tuple(slot.cpu().tolist()[:3]) == gm.counts(host, 0.0)


# ---------------------------------------------------------------------------- 4. autograd
def _torch_term(x, kind, role):
    import torch.nn.functional as F
    if kind == "hinge":
        return {"d_real": lambda: F.relu(1.0 - x), "d_fake": lambda: F.relu(1.0 + x), "g": lambda: -x}[role]().mean()
    return F.softplus(x if role == "d_fake" else -x).mean()


@pytest.mark.parametrize("kind, role", PAIRS)
def test_gan_term_differentiates_like_the_same_formula_in_torch_ops(kind, role):
    """Both sides are fp32: the op within 2e-6 / 1e-6 of the closed form (above), torch's own relu / softplus and mean of 35 within as
    much again -- twice those bounds."""
    from pdgn_amd import losses
    dev = _dev()
    host = np.random.default_rng(11).normal(0.0, 2.0, (35, 2)).astype(np.float32)
    up = torch.tensor(2.5, device=dev)                           # an upstream gradient != 1, a 0-dim device tensor
    a = torch.from_numpy(host[:, :1].copy()).to(dev).requires_grad_(True)
    b = a.detach().clone().requires_grad_(True)
    got, want = losses.gan_term(a, kind, role, 0.75), 0.75 * _torch_term(b, kind, role)
    assert got.shape == () and got.dtype == torch.float32
    got.backward(up)
    want.backward(up)
    assert abs(got.item() - want.item()) <= 2 * FWD_REL * abs(want.item())
    assert a.grad.shape == (35, 1) and ((a.grad - b.grad).abs() <= 2 * BWD_REL * b.grad.abs()).all()
    # a non-contiguous input: column 0 of a (35, 2) leaf
    c = torch.from_numpy(host).to(dev).requires_grad_(True)
    d = c.detach().clone().requires_grad_(True)
    assert not c[:, :1].is_contiguous()
    slot = torch.zeros(4, dtype=torch.int32, device=dev)
    (losses.gan_term(c[:, :1], kind, role, 0.75, count=slot) * up).backward()
    (0.75 * _torch_term(d[:, :1], kind, role) * up).backward()
    assert torch.equal(c.grad[:, 0], a.grad[:, 0]) and not c.grad[:, 1].any()
    assert ((c.grad - d.grad).abs() <= 2 * BWD_REL * d.grad.abs()).all()
    assert tuple(slot.cpu().tolist()[:3]) == gm.counts(host[:, 0], 0.0)
    with pytest.raises(TypeError):
        losses.gan_term(a, kind, role, count=torch.zeros(4, device=dev))
    with pytest.raises(ValueError):
        losses.gan_term(a, kind, role, count=torch.zeros(2, dtype=torch.int32, device=dev))


# ---------------------------------------------------------------------------- 5. refusals
def test_bad_arguments_are_refused_and_nothing_is_launched():
    from pdgn_amd import _lib
    dev = _dev()
    L = _lib.lib()
    x, g = torch.ones(8, device=dev), torch.ones(1, device=dev)
    out, dx = torch.full((1,), SENTINEL_F, device=dev), torch.full((8,), SENTINEL_F, device=dev)
    slot = torch.full((4,), SENTINEL_I, dtype=torch.int32, device=dev)
    s, p = _lib.stream_of(x), _lib.ptr
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 2)
    H, LG, R = gm.KINDS["hinge"], gm.KINDS["logistic"], gm.ROLES["d_real"]
    for n, kind, role in ((0, H, R), (-1, H, R), (8, 0, R), (8, 3, R), (8, -1, R), (8, LG, 3), (8, H, -1)):
        assert L.pdgn_gan_term(n, p(x), kind, role, 1.0, p(out), s) == -1
        assert L.pdgn_gan_term_count(n, p(x), kind, role, 1.0, 0.0, p(out), p(slot), s) == -1
        assert L.pdgn_gan_term_backward(n, p(x), kind, role, 1.0, p(g), p(dx), s) == -1
    assert L.pdgn_gan_term(8, None, H, R, 1.0, p(out), s) == -1 and L.pdgn_gan_term(8, p(x), H, R, 1.0, None, s) == -1
    assert L.pdgn_gan_term(8, odd(x), H, R, 1.0, p(out), s) == -1 and L.pdgn_gan_term(8, p(x), H, R, 1.0, odd(out), s) == -1
    assert L.pdgn_gan_term_count(1 << 31, p(x), H, R, 1.0, 0.0, p(out), p(slot), s) == -1
    assert L.pdgn_gan_term_count(8, p(x), H, R, 1.0, 0.0, p(out), None, s) == -1
    assert L.pdgn_gan_term_count(8, p(x), H, R, 1.0, 0.0, p(out), odd(slot), s) == -1
    assert L.pdgn_gan_term_count(8, None, H, R, 1.0, 0.0, p(out), p(slot), s) == -1
    assert L.pdgn_gan_term_backward(8, p(x), H, R, 1.0, None, p(dx), s) == -1
    assert L.pdgn_gan_term_backward(8, p(x), H, R, 1.0, p(g), None, s) == -1
    assert L.pdgn_gan_term_backward(8, p(x), H, R, 1.0, p(g), odd(dx), s) == -1
    torch.cuda.synchronize()
    assert (out == SENTINEL_F).all() and (dx == SENTINEL_F).all() and (slot == SENTINEL_I).all()


# ---------------------------------------------------------------------------- 6. the trainer
def _trainer(dev, gan_loss=None, augment=None, overlap=True):
    from pdgn_amd.trainer import PDGNTrainer
    torch.manual_seed(0)
    kw = {} if gan_loss is None else {"gan_loss": gan_loss}
    tr = PDGNTrainer(device=dev, distributed=False, augment=augment, **kw)
    tr.train()
    if not overlap:
        tr.overlap = False                                       # the sequential schedule's call sites (_seg_d, segment 4)
    return tr


def _inputs(dev, B=4):
    from pdgn_amd.trainer import noise, synthetic_batch
    g = torch.Generator().manual_seed(1)
    return synthetic_batch(B, dev), noise(B, dev, generator=g), noise(B, dev, generator=g)


def _drop_list(tr):
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def _record_scores(tr):
    """Forward hooks on D1..D4: per network the outputs of an iteration in call order -- real, fake, gen."""
    seen = [[] for _ in tr.D]
    handles = [d.register_forward_hook(lambda mod, args, out, i=i: seen[i].append(out.detach().clone())) for i, d in enumerate(tr.D)]
    return seen, handles


def _one_recorded_step(tr, dev):
    reals, z1, z2 = _inputs(dev)
    seen, handles = _record_scores(tr)
    out = tr.step(reals, z1, z2)
    torch.cuda.synchronize()
    for h in handles:
        h.remove()
    scores = [[t.cpu().numpy().reshape(-1) for t in per] for per in seen]
    assert all(len(per) == 3 and all(s.shape == (4,) for s in per) for per in scores)
    return {k: v.item() for k, v in out.items()}, {k: v.dtype for k, v in out.items()}, scores


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("objective", ["hinge", "logistic"])
def test_every_adversarial_term_of_a_step_is_the_objectives(objective, overlap):
    dev = _dev()
    tr = _trainer(dev, objective, overlap=overlap)
    assert tr.gan_loss == objective and bool(tr.overlap) == overlap
    out, dtypes, scores = _one_recorded_step(tr, dev)
    assert all(np.isfinite(v) for v in out.values()) and all(d == torch.float32 for d in dtypes.values())
    for i, (real, fake, gen) in enumerate(scores):
        got = np.float32(out["d_loss%d" % (i + 1)])
        if objective == "hinge":
            want = np.float32(gm.term(real, objective, "d_real") + gm.term(fake, objective, "d_fake"))
            assert _bits(got) == _bits(want), (i, got, want)
        else:
            want = gm.term64(real, objective, "d_real") + gm.term64(fake, objective, "d_fake")
            print("d_loss%d: %r against %r, relative %.3g" % (i + 1, float(got), want, _rel(got, want)))
            assert _rel(got, want) <= FWD_REL, (i, got, want)
    t = [gm.term64(per[2], objective, "g") for per in scores]
    want = 1.2 * (t[0] + t[1] + t[2]) + t[3]
    got = float(out["g_loss"]) - 0.1 * float(out["similar_loss"])
    print("%s, overlap %s: g_loss %r, similar_loss %r, adversarial part %r against %r, relative %.3g"
          % (objective, overlap, out["g_loss"], out["similar_loss"], got, want, _rel(got, want)))
    assert _rel(got, want) <= (1e-6 if objective == "hinge" else FWD_REL), (got, want)


def test_a_hinge_launch_list_has_the_default_lists_launches():
    dev = _dev()
    reals, z1, z2 = _inputs(dev)
    tr = _trainer(dev, "hinge")
    tr.capture_list(reals, z1, z2)
    for _ in range(2):
        out = tr.step_list()
        torch.cuda.synchronize()
        assert len(out) == 6 and all(np.isfinite(v.item()) for v in out.values())
    info = dict(tr._list.info)
    _drop_list(tr)
    plain = _trainer(dev, "lsgan")
    plain.capture_list(reals, z1, z2)
    want = dict(plain._list.info)
    _drop_list(plain)
    print("launch list, hinge: %s | lsgan: %s" % (info, want))
    assert info["nodes"] == want["nodes"] and info["kernels"] == want["kernels"]


def test_the_adaptive_augmentation_counts_hinge_scores_against_zero():
    dev = _dev()
    tr = _trainer(dev, "hinge", dict(EVERYTHING, p=0.5, seed=SEED, adaptive=dict(target=0.6, interval=1, span=64)))
    _, _, scores = _one_recorded_step(tr, dev)
    s1 = tr.aug_state()
    assert s1["ada"]["updates"] == 0 and s1["clock"] == 1        # the tick that opens the NEXT iteration folds this one's counts
    want = [gm.counts(per[0], 0.0) for per in scores]
    slots = tr.aug.slots.cpu().numpy().reshape(4, 4)
    assert [tuple(int(v) for v in row[:3]) for row in slots] == want and (slots[:, 3] == 0).all()
    reals, z1, z2 = _inputs(dev)
    tr.step(reals, z1, z2)
    s2 = tr.aug_state()
    a = s2["ada"]
    assert a["updates"] == 1 and a["last"][2] == 16 and a["last_net"] == want
    assert a["last"] == tuple(sum(t[j] for t in want) for j in range(3))


def test_lsgan_given_explicitly_is_twelve_mse_const_calls_and_no_gan_term(monkeypatch):
    from pdgn_amd import losses
    dev = _dev()
    calls = {"mse_const": [], "gan_term": []}
    real_mse, real_gan = losses.mse_const, losses.gan_term

    def mse_const(x, target, scale=1.0, count=None):
        calls["mse_const"].append((float(target), float(scale), count is not None))
        return real_mse(x, target, scale, count)

    def gan_term(*a, **k):
        calls["gan_term"].append(a)
        return real_gan(*a, **k)

    monkeypatch.setattr(losses, "mse_const", mse_const)
    monkeypatch.setattr(losses, "gan_term", gan_term)
    for overlap in (True, False):
        tr = _trainer(dev, "lsgan", overlap=overlap)
        assert tr.gan_loss == "lsgan" and _trainer(dev).gan_loss == "lsgan"
        calls["mse_const"].clear()
        reals, z1, z2 = _inputs(dev)
        out = tr.step(reals, z1, z2)
        torch.cuda.synchronize()
        assert all(np.isfinite(v.item()) for v in out.values())
        assert sorted(calls["mse_const"]) == sorted([(1.0, 0.5, False)] * 4 + [(0.0, 0.5, False)] * 4 + [(1.0, 1.0, False)] * 4), calls["mse_const"]
        assert not calls["gan_term"]
