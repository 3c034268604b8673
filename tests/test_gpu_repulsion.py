"""GPU: the repulsion regulariser and the spacing statistics -- pdgn_repulsion and pdgn_repulsion_backward called
directly on guard-banded buffers against the numpy restatement (tests/repulsion_mirror.py), bit for bit; every combination of NULL
outputs; autograd against the fp64 restatement within the derived bound; NaN; the refusals; evaluation.spacing_stats; the trainer in both
schedules and from a launch list; the reporter's spacing.csv.  Every test prints the figures it asserts on.

Measured on an MI355X with this file's inputs: the gradient's largest error is 0.032 of the derived bound and the loss's 0.0037 (n = 200);
in the trainer (B = 4, weight 10, radius four mean nearest-neighbour distances of the untrained generator's finest clouds) the per-level
values are 180.3 / 203.8 / 110.7 / 31.4, bit-equal to the mirror's, and g_loss - 0.1 similar_loss - adversarial part is within 4.7e-8 of
w * repulsion_loss under both schedules; from the launch list at weight 0, g_loss is within 3.1e-8 of its recomposition."""
import csv
import ctypes
import itertools

import numpy as np
import pytest
import torch

import repulsion_mirror as rm

pytestmark = pytest.mark.gpu
GUARD = 64
SENTINEL = -12345.0
F = np.float32
# unit-normal clouds: |x_i - x_j|^2 / 2 is chi-squared with three degrees of freedom, so h = 2 holds 43 % of the pairs (P[chi2_3 < 2]),
# h = 1.5 holds 24 % and h = 3 holds 79 %: both sides of `!(t <= 0)` run at every size that has pairs to speak of
RADIUS = 2.0


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _chunk():
    from pdgn_amd import _lib
    return int(_lib.lib().pdgn_repulsion_chunk())


def _sizes():
    c = _chunk()
    return sorted({1, 2, 63, 64, 65, 255, 256, 257, c - 1, c, c + 1, 2048})


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _cloud(b, n, seed):
    return np.random.default_rng(seed).normal(size=(b, n, 3)).astype(F)


def _banded(count, dev):
    whole = torch.full((2 * GUARD + count,), SENTINEL, dtype=torch.float32, device=dev)
    return whole, whole[GUARD:GUARD + count]


def _call(host, radius, dev, per_cloud=True, grad=True, nn2=True):
    """pdgn_repulsion through the C ABI into guard-banded outputs -> {loss, s, per_cloud, grad, nn2} as numpy (None where NULL was passed)."""
    from pdgn_amd import _lib, losses
    b, n, _ = host.shape
    x = torch.from_numpy(host).to(dev)
    inv, coef = losses.repulsion_constants(radius, b, n)
    bufs = {"s": _banded(b * n, dev), "loss": _banded(1, dev), "per_cloud": _banded(b, dev) if per_cloud else None,
            "grad": _banded(3 * b * n, dev) if grad else None, "nn2": _banded(b * n, dev) if nn2 else None}
    p = lambda k: _lib.ptr(bufs[k][1]) if bufs[k] is not None else None
    rc = _lib.lib().pdgn_repulsion(b, n, _lib.ptr(x), inv, coef, p("s"), p("loss"), p("per_cloud"), p("grad"), p("nn2"), _lib.stream_of(x))
    torch.cuda.synchronize()
    assert rc == 0
    out = {}
    for k, pair in bufs.items():
        if pair is None:
            out[k] = None
            continue
        w = pair[0].cpu().numpy()
        assert (w[:GUARD] == SENTINEL).all() and (w[w.size - GUARD:] == SENTINEL).all(), k
        out[k] = w[GUARD:w.size - GUARD].copy()
    out["loss"] = out["loss"][0]
    out["s"], out["grad"] = out["s"].reshape(b, n), None if out["grad"] is None else out["grad"].reshape(b, n, 3)
    out["nn2"] = None if out["nn2"] is None else out["nn2"].reshape(b, n)
    return out


_MIRROR = {}


def _mirror(b, n, radius=RADIUS):
    """The mirror of the case (b, n): computed once, shared, never modified."""
    key = (b, n, radius)
    if key not in _MIRROR:
        host = _cloud(b, n, 1000 * b + n)
        _MIRROR[key] = (host, rm.repulsion(host, radius))
    return _MIRROR[key]


# ---------------------------------------------------------------------------- 1. the kernel against the mirror
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, "chunk-1", "chunk", "chunk+1", 2048])
def test_the_kernel_is_the_mirror_bit_for_bit(n, b):
    dev = _dev()
    if isinstance(n, str):
        n = _chunk() + {"chunk-1": -1, "chunk": 0, "chunk+1": 1}[n]
    assert n in _sizes()
    # A fraction strictly between 10 % and 90 % needs pairs to take it of.  n = 1 has none (nothing to assert); one cloud of two points
    # has ONE unordered pair, which is inside or outside: that case runs at two radii, one on either side, and both are compared.
    radii = [RADIUS]
    if n == 2 and b == 1:
        host = _cloud(1, 2, 1002)
        d = float(np.sqrt(((host[0, 0].astype(np.float64) - host[0, 1]) ** 2).sum()))
        radii = [0.5 * d, 2.0 * d]
        assert [rm.repulsion(host, h)["inside"] for h in radii] == [0.0, 1.0]
    for h in radii:
        host, want = _mirror(b, n, h)
        if n > 2 or (n == 2 and b == 3):
            print("b = %d, n = %d, h = %g: %.1f %% of the ordered pairs inside" % (b, n, h, 100 * want["inside"]))
            assert 0.1 <= want["inside"] <= 0.9
        got = _call(host, h, dev)
        for k in ("s", "nn2", "grad", "per_cloud"):
            assert _same(got[k], want[k]), (k, n, b, np.flatnonzero(_bits(got[k]).ravel() != _bits(want[k]).ravel())[:8])
        assert _bits(got["loss"]) == _bits(want["loss"]), (n, b, got["loss"], want["loss"])
        if n == 1:
            assert np.isposinf(got["nn2"]).all() and got["loss"] == 0.0 and not got["grad"].any()


def test_every_combination_of_null_outputs_leaves_the_others_bits():
    dev = _dev()
    host, want = _mirror(3, 257)
    for per_cloud, grad, nn2 in itertools.product((False, True), repeat=3):
        got = _call(host, RADIUS, dev, per_cloud, grad, nn2)
        assert _bits(got["loss"]) == _bits(want["loss"]) and _same(got["s"], want["s"])
        for k, on in (("per_cloud", per_cloud), ("grad", grad), ("nn2", nn2)):
            assert (got[k] is None) == (not on) and (not on or _same(got[k], want[k])), (k, per_cloud, grad, nn2)


def test_two_calls_on_the_same_input_are_bit_equal():
    dev = _dev()
    host = _cloud(3, 1500, 77)
    a, b = _call(host, RADIUS, dev), _call(host, RADIUS, dev)
    assert all(_same(a[k], b[k]) for k in ("loss", "s", "per_cloud", "grad", "nn2"))


# ---------------------------------------------------------------------------- 2. autograd
def test_the_op_differentiates_like_the_fp64_restatement_and_an_upstream_gradient_scales_exactly():
    from pdgn_amd import losses
    dev = _dev()
    n = 200
    host = _cloud(2, n, 11)
    ref = rm.restate64(host, RADIUS)
    bound = rm.bounds(ref, n)
    x = torch.from_numpy(host).to(dev).requires_grad_(True)
    loss = losses.repulsion(x, RADIUS)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    torch.cuda.synchronize()
    g1 = x.grad.cpu().numpy()
    err = np.abs(g1.astype(np.float64) - ref["grad"])
    print("n = %d: largest gradient error / bound %.3g, loss error / bound %.3g"
          % (n, rm.worst(err, bound["grad"]), abs(loss.item() - ref["loss"]) / bound["loss"]))
    assert (err <= bound["grad"]).all() and abs(loss.item() - ref["loss"]) <= bound["loss"]
    want = rm.repulsion(host, RADIUS)
    assert _same(g1, want["grad"]) and _bits(loss.item()) == _bits(want["loss"])          # an upstream 1 changes no bit
    # an upstream gradient other than 1: every element is the saved gradient times it, one fp32 product
    up = torch.tensor(2.5, device=dev)
    y = torch.from_numpy(host).to(dev).requires_grad_(True)
    losses.repulsion(y, RADIUS).backward(up)
    assert _same(y.grad.cpu().numpy(), F(2.5) * want["grad"])
    z = torch.from_numpy(host).to(dev).requires_grad_(True)
    (losses.repulsion(z, RADIUS) * 0.3).backward()
    assert _same(z.grad.cpu().numpy(), F(0.3) * want["grad"])
    # the generator's layout: a (B,3,N) view of point-major memory goes in as it is, and its gradient comes back in that layout
    base = torch.from_numpy(host).to(dev)
    cm = base.transpose(1, 2).detach().requires_grad_(True)
    assert cm.shape == (2, 3, n) and not cm.is_contiguous()
    lc = losses.repulsion(cm, RADIUS)
    lc.backward()
    assert _bits(lc.item()) == _bits(want["loss"]) and cm.grad.shape == (2, 3, n) and _same(cm.grad.transpose(1, 2).cpu().numpy(), want["grad"])
    # a (B,3,N) tensor that IS contiguous: copied to point-major inside
    cc = base.transpose(1, 2).contiguous().requires_grad_(True)
    lcc = losses.repulsion(cc, RADIUS)
    lcc.backward()
    assert _bits(lcc.item()) == _bits(want["loss"]) and _same(cc.grad.transpose(1, 2).cpu().numpy(), want["grad"])


def test_the_backward_entry_point_on_guard_banded_buffers():
    from pdgn_amd import _lib
    dev = _dev()
    count = 3 * 257 * 1025 + 1                                   # past 1024 blocks of 256: the grid-stride loop turns
    grad = torch.from_numpy(np.random.default_rng(2).normal(size=count).astype(F)).to(dev)
    g = torch.tensor([-1.75], device=dev)
    whole, dx = _banded(count, dev)
    assert _lib.lib().pdgn_repulsion_backward(count, _lib.ptr(grad), _lib.ptr(g), _lib.ptr(dx), _lib.stream_of(grad)) == 0
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + count:] == SENTINEL).all()
    assert _same(w[GUARD:GUARD + count], F(-1.75) * grad.cpu().numpy())


# ---------------------------------------------------------------------------- 3. NaN
def test_a_nan_coordinate_is_a_nan_loss_and_nan_gradients_for_its_cloud_only():
    dev = _dev()
    host = _cloud(3, 130, 5).copy()
    host[1, 70, 2] = np.nan
    got, want = _call(host, RADIUS, dev), rm.repulsion(host, RADIUS)
    assert np.isnan(got["loss"]) and np.isnan(want["loss"])
    assert np.isnan(got["grad"][1]).all() and np.isnan(got["s"][1]).all() and np.isnan(got["per_cloud"][1])
    for c in (0, 2):
        assert np.isfinite(got["grad"][c]).all() and got["grad"][c].any() and np.isfinite(got["per_cloud"][c])
        assert _same(got["grad"][c], want["grad"][c]) and _same(got["s"][c], want["s"][c]) and _same(got["nn2"][c], want["nn2"][c])
    assert _same(got["nn2"], want["nn2"])                        # (a NaN distance is never the smaller one)


# ---------------------------------------------------------------------------- 4. refusals
def test_bad_arguments_are_refused_and_nothing_is_launched():
    from pdgn_amd import _lib
    dev = _dev()
    L = _lib.lib()
    b, n = 2, 8
    x, g = torch.ones(b, n, 3, device=dev), torch.ones(1, device=dev)
    new = lambda count: torch.full((count,), SENTINEL, device=dev)
    s, loss, pc, grad, nn2, dx = new(b * n), new(1), new(b), new(3 * b * n), new(b * n), new(3 * b * n)
    st, p = _lib.stream_of(x), _lib.ptr
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 2)
    call = lambda **kw: L.pdgn_repulsion(*[kw.get(k, v) for k, v in (("b", b), ("n", n), ("xyz", p(x)), ("inv", 1.0), ("coef", -0.5), ("s", p(s)),
                                                                     ("loss", p(loss)), ("pc", p(pc)), ("grad", p(grad)), ("nn2", p(nn2)), ("st", st))])
    for kw in ({"b": 0}, {"b": -1}, {"n": 0}, {"n": -3}, {"n": 8193}, {"b": 1 << 20, "n": 512}, {"inv": 0.0}, {"inv": -1.0}, {"inv": float("inf")},
               {"inv": float("nan")}, {"coef": float("nan")}, {"coef": float("inf")}, {"xyz": None}, {"s": None}, {"loss": None}, {"xyz": odd(x)},
               {"s": odd(s)}, {"loss": odd(loss)}, {"pc": odd(pc)}, {"grad": odd(grad)}, {"nn2": odd(nn2)}):
        assert call(**kw) == -1, kw
    for args in ((0, p(grad), p(g), p(dx)), (-1, p(grad), p(g), p(dx)), (8, None, p(g), p(dx)), (8, p(grad), None, p(dx)), (8, p(grad), p(g), None),
                 (8, odd(grad), p(g), p(dx)), (8, p(grad), odd(g), p(dx)), (8, p(grad), p(g), odd(dx))):
        assert L.pdgn_repulsion_backward(*args, st) == -1, args
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in (s, loss, pc, grad, nn2, dx))
    from pdgn_amd import losses
    with pytest.raises(ValueError):
        losses.repulsion(torch.zeros(1, 8193, 3, device=dev), 1.0)
    with pytest.raises(ValueError):
        losses.repulsion(x, 0.0)


# ---------------------------------------------------------------------------- 5. spacing statistics
def test_spacing_stats_on_a_jittered_grid_and_on_planted_duplicates_match_numpy():
    from pdgn_amd import evaluation as ev
    dev = _dev()
    rng = np.random.default_rng(8)
    ax = np.arange(12, dtype=np.float64)
    grid = np.stack(np.meshgrid(ax, ax, ax[:3], indexing="ij"), -1).reshape(-1, 3)             # 432 points, unit spacing
    clouds = np.stack([grid + rng.normal(0.0, sigma, grid.shape) for sigma in (0.0, 0.05, 0.2, 0.4, 1.0)]).astype(F)
    got, want = ev.spacing_stats(torch.from_numpy(clouds).to(dev), batch=2), rm.spacing_stats(clouds)      # three launches
    print("jittered grid: %s" % got)
    for k in ("nn_mean", "nn_cv", "nn_min"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    assert got["duplicates"] == want["duplicates"] == 0
    one = ev.spacing_stats(torch.from_numpy(clouds[:1]).to(dev))
    assert one["nn_mean"] == 1.0 and one["nn_cv"] == 0.0 and one["nn_min"] == 1.0               # the grid itself: perfectly even
    assert ev.spacing_stats(torch.from_numpy(clouds[4:]).to(dev))["nn_cv"] > ev.spacing_stats(torch.from_numpy(clouds[1:2]).to(dev))["nn_cv"]
    planted = _cloud(3, 300, 21).copy()
    planted[0, 17] = planted[0, 200]
    planted[2, 5] = planted[2, 6] = planted[2, 299]
    got, want = ev.spacing_stats(torch.from_numpy(planted).to(dev)), rm.spacing_stats(planted)
    print("planted duplicates: %s" % got)
    assert got["duplicates"] == want["duplicates"] == 5 and got["nn_min"] == 0.0
    for k in ("nn_mean", "nn_cv"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    with pytest.raises(ValueError):
        ev.spacing_stats(torch.zeros(2, 1, 3, device=dev))


# ---------------------------------------------------------------------------- 6. the trainer
def _trainer(dev, repulsion=None, overlap=True):
    from pdgn_amd.trainer import PDGNTrainer
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False, **({} if repulsion is None else {"repulsion": repulsion}))
    tr.train()
    if not overlap:
        tr.overlap = False                                       # the sequential schedule (segment 4)
    return tr


def _inputs(dev, B=4):
    from pdgn_amd.trainer import noise, synthetic_batch
    g = torch.Generator().manual_seed(1)
    return synthetic_batch(B, dev), noise(B, dev, generator=g), noise(B, dev, generator=g)


def _drop_list(tr):
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def _radius_for(tr, dev, z, factor=4.0):
    """A radius at which an untrained generator's clouds have neighbours to repel: `factor` times the mean nearest-neighbour distance of
    its finest clouds for this noise (a forward without a graph)."""
    from pdgn_amd import evaluation as ev
    with torch.no_grad():
        finest = tr.G(z)[3].transpose(1, 2).contiguous()
    return factor * ev.spacing_stats(finest)["nn_mean"]


def _lsgan_g(scores):
    return float(((scores.astype(np.float64) - 1.0) ** 2).mean())


# The weight and the radius factor of the trainer tests put w * repulsion_loss at the scale of g_loss itself: the recomposition
# g_loss - 0.1 similar_loss - adversarial part subtracts fp32 numbers of g_loss's size, so its error is a few 2^-24 of g_loss, and the
# 1e-6 bound, which is relative to w * repulsion_loss, holds only a term that is not a small part of it.
WEIGHT = 10.0


@pytest.mark.parametrize("overlap", [True, False])
def test_a_step_with_the_term_is_the_mirrors_sum_over_the_levels(overlap):
    from pdgn_amd import losses
    dev = _dev()
    tr = _trainer(dev, {"weight": WEIGHT, "radius": 1.0}, overlap)
    assert bool(tr.overlap) == overlap
    reals, z1, z2 = _inputs(dev)
    h = _radius_for(tr, dev, z2)
    tr.set_repulsion(radius=h)                                   # no list yet: allowed
    clouds, scores = [], [[] for _ in tr.D]
    handles = [tr.G.register_forward_hook(lambda mod, args, out: clouds.append([c.detach().clone() for c in out]))]
    handles += [d.register_forward_hook(lambda mod, args, out, i=i: scores[i].append(out.detach().clone())) for i, d in enumerate(tr.D)]
    out = tr.step(reals, z1, z2)
    torch.cuda.synchronize()
    for hd in handles:
        hd.remove()
    assert len(clouds) == 2 and all(len(per) == 3 for per in scores)
    assert sorted(out) == sorted(["d_loss1", "d_loss2", "d_loss3", "d_loss4", "g_loss", "similar_loss", "repulsion_loss"])
    vals = {k: v.item() for k, v in out.items()}
    assert all(np.isfinite(v) for v in vals.values()) and all(v.dtype == torch.float32 and v.shape == () for v in out.values())
    gen = clouds[1]                                              # the second pass's four clouds, (B,3,N)
    sizes = [c.shape[2] for c in gen]
    radii = losses.repulsion_radii(h, sizes)
    state = tr.repulsion_state()
    assert sizes == [256, 512, 1024, 2048] and state["radii"] == radii and state["radius"] == h and state["weight"] == WEIGHT
    want = [rm.repulsion(c.transpose(1, 2).contiguous().cpu().numpy(), r) for c, r in zip(gen, radii)]
    for l in range(4):
        print("overlap %s, level %d (n = %d, h = %.4g): %r against the mirror's %r, %.1f %% of the pairs inside"
              % (overlap, l + 1, sizes[l], radii[l], state["per_level"][l], float(want[l]["loss"]), 100 * want[l]["inside"]))
        assert _bits(state["per_level"][l]) == _bits(want[l]["loss"]), l
        assert want[l]["loss"] > 0
    total = sum(float(w["loss"]) for w in want)                  # four positive fp32 values added on the device: three roundings
    assert abs(vals["repulsion_loss"] - total) <= 4 * rm.U * total and abs(state["total"] - total) <= 4 * rm.U * total
    adv = 1.2 * sum(_lsgan_g(scores[i][2].cpu().numpy()) for i in range(3)) + _lsgan_g(scores[3][2].cpu().numpy())
    got, term = vals["g_loss"] - 0.1 * vals["similar_loss"] - adv, WEIGHT * vals["repulsion_loss"]
    print("overlap %s: g_loss %r, similar_loss %r, adversarial part %r, remainder %r against w * repulsion_loss %r, relative %.3g"
          % (overlap, vals["g_loss"], vals["similar_loss"], adv, got, term, abs(got - term) / term))
    assert abs(got - term) <= 1e-6 * term


def test_without_the_term_the_op_is_never_called_and_out_has_six_keys(monkeypatch):
    from pdgn_amd import losses
    dev = _dev()
    calls = []

    def spy(*a, **k):
        calls.append(a)
        raise AssertionError("losses.repulsion was called")

    monkeypatch.setattr(losses, "repulsion", spy)
    for overlap in (True, False):
        tr = _trainer(dev, None, overlap)
        assert tr.repulsion is None
        out = tr.step(*_inputs(dev))
        torch.cuda.synchronize()
        assert sorted(out) == sorted(tr.LOSS_KEYS) and len(out) == 6 and all(np.isfinite(v.item()) for v in out.values())
    assert not calls


def test_a_launch_list_with_the_term_replays_and_follows_the_weight_without_recapture():
    dev = _dev()
    reals, z1, z2 = _inputs(dev)
    tr = _trainer(dev, {"weight": WEIGHT, "radius": 1.0})
    tr.set_repulsion(radius=_radius_for(tr, dev, z2))
    scores = [[] for _ in tr.D]                                  # the score tensors themselves: the captured ones are the list's static buffers
    handles = [d.register_forward_hook(lambda mod, args, out, i=i: scores[i].append(out.detach())) for i, d in enumerate(tr.D)]
    tr.capture_list(reals, z1, z2)
    for hd in handles:
        hd.remove()
    gen_scores = [per[-1] for per in scores]                     # D_k's last call of the captured iteration: D_k(G(z2)_k)
    for _ in range(2):
        out = tr.step_list()
        torch.cuda.synchronize()
        vals = {k: v.item() for k, v in out.items()}
        print("launch list with the term: %s" % vals)
        assert len(vals) == 7 and all(np.isfinite(v) for v in vals.values()) and vals["repulsion_loss"] > 0
    state = tr.repulsion_state()
    assert abs(state["total"] - vals["repulsion_loss"]) <= 4 * rm.U * state["total"] and all(v > 0 for v in state["per_level"])
    with pytest.raises(RuntimeError):
        tr.set_repulsion(radius=2.0 * tr.repulsion["radius"])    # an argument of the captured launches
    before = vals["g_loss"]
    tr.set_repulsion(weight=0.0)                                 # the vector the list's weighted sum reads: no recapture
    out = tr.step_list()
    torch.cuda.synchronize()
    vals = {k: v.item() for k, v in out.items()}
    t = [_lsgan_g(s.detach().cpu().numpy()) for s in gen_scores]
    want = 1.2 * (t[0] + t[1] + t[2]) + t[3] + 0.1 * vals["similar_loss"]
    print("weight 0: g_loss %r (before: %r) against 1.2 (g1 + g2 + g3) + g4 + 0.1 similar = %r, relative %.3g; repulsion_loss %r"
          % (vals["g_loss"], before, want, abs(vals["g_loss"] - want) / want, vals["repulsion_loss"]))
    assert abs(vals["g_loss"] - want) <= 1e-6 * want and vals["repulsion_loss"] > 0 and before > vals["g_loss"]
    info = dict(tr._list.info)
    _drop_list(tr)
    print("launch list with the term: %s" % info)


def test_a_default_trainers_list_has_the_counts_of_another_default_trainers():
    dev = _dev()
    reals, z1, z2 = _inputs(dev)
    infos = []
    for _ in range(2):
        tr = _trainer(dev)
        tr.capture_list(reals, z1, z2)
        out = tr.step_list()
        torch.cuda.synchronize()
        assert len(out) == 6
        infos.append(dict(tr._list.info))
        _drop_list(tr)
    print("launch list, default: %s | default again: %s" % tuple(infos))
    assert infos[0]["nodes"] == infos[1]["nodes"] and infos[0]["kernels"] == infos[1]["kernels"]


# ---------------------------------------------------------------------------- 7. the reporter
def _state_tensors(tr):
    ts = []
    for net in [tr.G] + tr.D:
        ts += list(net.parameters()) + list(net.buffers())
    for opt in [tr.optG] + tr.optD:
        for st in opt.state.values():
            ts += [v for v in st.values() if torch.is_tensor(v)]
    return ts


def test_the_reporter_writes_spacing_csv_only_when_asked_and_leaves_training_alone(tmp_path):
    from pdgn_amd.data import normalize_clouds
    from pdgn_amd.report import SnapshotReporter
    dev = _dev()
    tr = _trainer(dev)
    tr.step(*_inputs(dev))                                       # optimizer state exists
    val = normalize_clouds(torch.from_numpy(_cloud(6, 2048, 4)), "shape_bbox")[0].to(dev).contiguous()
    make = lambda d, **kw: SnapshotReporter(tr, val, tmp_path / d, every=1, batch_size=4, normalize="shape_bbox", seed=9, rows=2, cell=32, **kw)
    torch.cuda.synchronize()
    ts = _state_tensors(tr)
    before = [t.detach().clone() for t in ts]
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    on = make("on", spacing=True)
    assert on(1) is not None and on(2) is not None
    torch.cuda.synchronize()
    after = _state_tensors(tr)
    assert len(after) == len(before) > 100 and all(a is t for a, t in zip(after, ts)) and all(torch.equal(a, b) for a, b in zip(after, before))
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    assert all(m.training for net in [tr.G] + tr.D for m in net.modules())
    with open(tmp_path / "on" / "spacing.csv") as f:
        table = list(csv.reader(f))
    print("spacing.csv: %s" % table)
    assert table[0] == ["epoch", "gen nn_mean", "gen nn_cv", "val nn_mean", "val nn_cv", "gen duplicates"]
    assert [r[0] for r in table[1:]] == ["1", "2"] and all(len(r) == 6 and np.isfinite([float(v) for v in r]).all() for r in table[1:])
    want = rm.spacing_stats(val.cpu().numpy())
    assert abs(float(table[1][3]) - want["nn_mean"]) <= 1e-8 * want["nn_mean"] and abs(float(table[1][4]) - want["nn_cv"]) <= 1e-8 * want["nn_cv"]
    assert table[1][3:5] == table[2][3:5] and on.last_spacing[0] == 2
    with open(tmp_path / "on" / "metrics.csv") as f:
        assert next(csv.reader(f))[0] == "epoch"
    off = make("off")
    assert off(1) is not None and off.last_spacing is None
    assert sorted(p.name for p in (tmp_path / "off").iterdir()) == ["metrics.csv", "preview_1.png"]
