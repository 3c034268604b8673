"""GPU: the flatness regulariser -- pdgn_flatness called directly on guard-banded buffers against the numpy
restatement (tests/flatness_mirror.py), bit for bit, in every block size, on both sides of the LDS staging threshold and with skewed
in-degrees; the eigenvalues against pdgn_estimate_normals'; the grad = NULL path; the refusals; autograd; evaluation.surface_stats; the
trainer in both schedules and from a launch list, alone and beside the repulsion term; flatness.csv.  Every test prints the figures it
asserts on."""
import ctypes

import numpy as np
import pytest
import torch

import flatness_mirror as fm
import normals_mirror as nm

pytestmark = pytest.mark.gpu
GUARD = 64
SENTINEL = -12345.0
F = np.float32
U = 2.0 ** -24
# (b, n, k): one point; a list as long as the cloud; one-wave workgroups with a tail; 128 threads; k at its limit; 35 x 256 (64 threads,
# 140 workgroups); 130 x 257 (256 threads, staged, a tail of one point); 16 x 4096 (staged, at the limit) and 16 x 4097 (not staged)
SHAPES = [(1, 1, 1), (2, 3, 3), (3, 65, 8), (2, 257, 16), (1, 1000, 64), (35, 256, 16), (130, 257, 4), (16, 4096, 4), (16, 4097, 4)]
EPS = 1e-3                                                        # unit-normal clouds: the neighbourhood traces are of the order of 0.01 .. 1


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cloud(b, n, seed):
    return np.random.default_rng(seed).normal(size=(b, n, 3)).astype(F)


def _banded(count, dev, dtype=torch.float32):
    whole = torch.full((2 * GUARD + count,), SENTINEL if dtype.is_floating_point else int(SENTINEL), dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + count]


def _call(host, idx, eps, dev, coef=None, per_cloud=True, degenerate=True, grad=True, ws=None):
    """pdgn_flatness through the C ABI into guard-banded outputs -> {loss, sigma, per_cloud, degenerate, grad} as numpy (None where NULL
    was passed).  ws: a tensor to pass as the workspace (default: one of the size the library asks for, where grad is asked for)."""
    from pdgn_amd import _lib
    b, n, _ = host.shape
    k = idx.shape[2]
    x, ix = torch.from_numpy(host).to(dev), torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
    L = _lib.lib()
    coef = 1.0 / (float(b) * float(n)) if coef is None else coef
    if grad and ws is None:
        size = L.pdgn_flatness_workspace_bytes(b, n, k, 1)
        assert size > 0 and size % 4 == 0
        ws = torch.empty(size // 4, dtype=torch.int32, device=dev)
    bufs = {"sigma": _banded(b * n, dev), "loss": _banded(1, dev), "per_cloud": _banded(b, dev) if per_cloud else None,
            "degenerate": _banded(b, dev, torch.int32) if degenerate else None, "grad": _banded(3 * b * n, dev) if grad else None}
    p = lambda key: _lib.ptr(bufs[key][1]) if bufs[key] is not None else None
    rc = L.pdgn_flatness(b, n, k, _lib.ptr(x), _lib.ptr(ix), eps, coef, p("sigma"), p("loss"), p("per_cloud"), p("degenerate"), p("grad"),
                         _lib.ptr(ws), _lib.stream_of(x))
    torch.cuda.synchronize()
    assert rc == 0
    out = {}
    for key, pair in bufs.items():
        if pair is None:
            out[key] = None
            continue
        w = pair[0].cpu().numpy()
        assert (w[:GUARD] == F(SENTINEL).astype(w.dtype)).all() and (w[w.size - GUARD:] == F(SENTINEL).astype(w.dtype)).all(), key
        out[key] = w[GUARD:w.size - GUARD].copy()
    out["loss"] = out["loss"][0]
    out["sigma"], out["grad"] = out["sigma"].reshape(b, n), None if out["grad"] is None else out["grad"].reshape(b, n, 3)
    return out


def _knn(host, k, dev):
    from pdgn_amd import pointops
    x = torch.from_numpy(host).to(dev)
    return pointops.knnquery(k, x, x).cpu().numpy()


_CASES = {}


def _case(shape, lists, dev):
    """(cloud, lists) of a case: computed once, shared, never modified.  "knn": the device's own neighbour search on a clean cloud.
    "random": uniform lists with repeats inside a list, one entry outside the cloud, a NaN and an infinite coordinate."""
    key = (shape, lists)
    if key not in _CASES:
        b, n, k = shape
        host = _cloud(b, n, 1000 * b + n + k)
        if lists == "knn":
            idx = _knn(host, k, dev)
        else:
            rng = np.random.default_rng(7 * n + k)
            idx = fm.random_lists(rng, b, n, k)
            idx[0, n // 2, 0] = n
            host[0, 0, 1] = np.nan
            host[b - 1, n - 1, 2] = np.inf
        _CASES[key] = (host, idx)
    return _CASES[key]


def _compare(got, want, what):
    for key in ("sigma", "per_cloud", "grad"):
        assert nm.same_bits(got[key], want[key]), (what, key)
    assert nm.same_bits(np.array([got["loss"]]), np.array([want["loss"]])), (what, "loss")
    assert np.array_equal(got["degenerate"], want["degenerate"]), (what, "degenerate")


# ---------------------------------------------------------------------------- 1. the kernel against the mirror
@pytest.mark.parametrize("eps", [0.0, EPS])
@pytest.mark.parametrize("lists", ["knn", "random"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_the_kernels_are_the_mirror_bit_for_bit(shape, lists, eps):
    dev = _dev()
    host, idx = _case(shape, lists, dev)
    got = _call(host, idx, eps, dev)
    want = fm.flatness(host, idx, eps)
    nan_rows = int(np.isnan(want["grad"]).any(axis=2).sum())
    print("%s %s eps %g: loss %r, degenerate %d, NaN sigma %d, NaN gradient rows %d, largest |grad| %.3g"
          % (shape, lists, eps, float(want["loss"]), int(want["degenerate"].sum()), int(np.isnan(want["sigma"]).sum()), nan_rows,
             float(np.nanmax(np.abs(want["grad"]))) if not np.isnan(want["grad"]).all() else float("nan")))
    if lists == "knn":
        assert np.isfinite(want["grad"]).all() and np.isfinite(want["loss"])
        if shape[1] > 3 * shape[2]:
            assert want["loss"] > 0 and np.abs(want["grad"]).max() > 0
    else:
        assert np.isnan(want["loss"]) and np.isnan(want["per_cloud"][0]) and np.isnan(want["per_cloud"][-1])
        assert nan_rows >= 1 or shape[1] == 1                     # (one point whose only entry lies outside: no target at all)
        if shape[0] > 2:                                          # the clouds between the poisoned ones are clean
            assert np.isfinite(want["per_cloud"][1:-1]).all() and np.isfinite(want["grad"][1:-1]).all()
    _compare(got, want, (shape, lists, eps))


@pytest.mark.parametrize("eps", [0.0, EPS])
@pytest.mark.parametrize("targets", [1, 4])
def test_skewed_in_degrees_are_the_mirror_bit_for_bit(targets, eps):
    """Every entry 0: one row of the transpose holds all n k edges.  Entries confined to 0 .. 3: collisions inside every run of 64 edges."""
    dev = _dev()
    b, n, k = 2, 257, 16
    host = _cloud(b, n, 31)
    rng = np.random.default_rng(5)
    idx = np.zeros((b, n, k), np.int32) if targets == 1 else rng.integers(0, 4, size=(b, n, k)).astype(np.int32)
    got, want = _call(host, idx, eps, dev), fm.flatness(host, idx, eps)
    print("%d targets, eps %g: loss %r, degenerate %s, gradient of the targets %s" % (targets, eps, float(want["loss"]), want["degenerate"].tolist(),
                                                                                      want["grad"][0, :targets].tolist()))
    assert np.array_equal(got["grad"][:, targets:], np.zeros((b, n - targets, 3), F)) and not np.signbit(got["grad"][:, targets:]).any()
    _compare(got, want, (targets, eps))


def test_the_planar_grid_is_exactly_flat_on_the_device():
    dev = _dev()
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2) / 8.0
    x = np.concatenate([g, np.full((64, 1), 0.25)], axis=1).astype(F)[None]
    got = _call(x, nm.knn_indices(x[0], 9)[None], 0.0, dev)
    assert got["degenerate"].tolist() == [64] and got["loss"] == 0 and not np.signbit(got["loss"])
    assert np.array_equal(got["sigma"], np.zeros((1, 64), F)) and np.array_equal(got["grad"], np.zeros((1, 64, 3), F))
    assert not np.signbit(got["grad"]).any()


# ---------------------------------------------------------------------------- 2. the eigenvalues are pdgn_estimate_normals'
@pytest.mark.parametrize("eps", [0.0, EPS])
@pytest.mark.parametrize("lists", ["knn", "random"])
@pytest.mark.parametrize("shape", [(2, 257, 16), (35, 256, 16), (16, 4097, 4)], ids=lambda s: "%dx%dx%d" % s)
def test_sigma_is_made_of_the_eigenvalues_estimate_normals_writes(shape, lists, eps):
    from pdgn_amd import pointops
    dev = _dev()
    host, idx = _case(shape, lists, dev)
    got = _call(host, idx, eps, dev, grad=False)
    _, eig = pointops.estimate_normals(torch.from_numpy(host).to(dev), idx=torch.from_numpy(idx).to(dev), return_eig=True)
    eig = eig.cpu().numpy()
    with np.errstate(all="ignore"):
        q = ((eig[..., 0] + eig[..., 1]) + eig[..., 2]) + F(eps)
        bad = np.isnan(eig).any(axis=2)                             # (estimate_normals poisons exactly the points the definition calls bad)
        deg = ~bad & (~(eig[..., 0] > 0) | ~(q > 0))
        want = np.where(deg, F(0.0), eig[..., 0] / q).astype(F)
    print("%s %s eps %g: %d bad, %d degenerate points" % (shape, lists, eps, int(bad.sum()), int(deg.sum())))
    assert nm.same_bits(got["sigma"], want) and np.array_equal(got["degenerate"], deg.sum(axis=1))


# ---------------------------------------------------------------------------- 3. paths
def test_without_a_gradient_the_other_outputs_keep_their_bits_and_the_workspace_is_not_touched():
    dev = _dev()
    host, idx = _case((35, 256, 16), "random", dev)
    full = _call(host, idx, EPS, dev)
    poisoned = torch.full((4096,), 0x5A5A5A5A, dtype=torch.int32, device=dev)      # far too small for the gradient: it must not be read
    for per_cloud, degenerate in ((True, True), (False, True), (True, False), (False, False)):
        got = _call(host, idx, EPS, dev, per_cloud=per_cloud, degenerate=degenerate, grad=False, ws=poisoned)
        assert got["grad"] is None and nm.same_bits(got["sigma"], full["sigma"]) and nm.same_bits(np.array([got["loss"]]), np.array([full["loss"]]))
        assert got["per_cloud"] is None if not per_cloud else nm.same_bits(got["per_cloud"], full["per_cloud"])
        assert got["degenerate"] is None if not degenerate else np.array_equal(got["degenerate"], full["degenerate"])
        assert (poisoned == 0x5A5A5A5A).all()
    null = _call(host, idx, EPS, dev, grad=False)                   # and with ws = NULL
    assert nm.same_bits(null["sigma"], full["sigma"]) and np.array_equal(null["degenerate"], full["degenerate"])
    light = _call(host, idx, EPS, dev, per_cloud=False, degenerate=False)
    assert nm.same_bits(light["grad"], full["grad"]) and nm.same_bits(light["sigma"], full["sigma"])


def test_two_calls_on_the_same_input_are_bit_equal():
    dev = _dev()
    host, idx = _case((16, 4097, 4), "knn", dev)
    a, b = _call(host, idx, EPS, dev), _call(host, idx, EPS, dev)
    for key in ("sigma", "per_cloud", "grad"):
        assert nm.same_bits(a[key], b[key]), key
    assert a["loss"] == b["loss"] and np.array_equal(a["degenerate"], b["degenerate"])


# ---------------------------------------------------------------------------- 4. refusals
def test_bad_arguments_are_refused_and_nothing_is_launched():
    from pdgn_amd import _lib
    dev = _dev()
    L = _lib.lib()
    b, n, k = 2, 8, 4
    x, idx = torch.ones(b, n, 3, device=dev), torch.zeros(b, n, k, dtype=torch.int32, device=dev)
    new = lambda count: torch.full((count,), SENTINEL, device=dev)
    sigma, loss, pc, grad = new(b * n), new(1), new(b), new(3 * b * n)
    deg = torch.full((b,), -777, dtype=torch.int32, device=dev)
    ws = torch.full((L.pdgn_flatness_workspace_bytes(b, n, k, 1) // 4 + 4,), -777, dtype=torch.int32, device=dev)
    st, p = _lib.stream_of(x), _lib.ptr
    odd = lambda t, by=2: ctypes.c_void_p(t.data_ptr() + by)
    names = (("b", b), ("n", n), ("k", k), ("xyz", p(x)), ("idx", p(idx)), ("eps", 0.0), ("coef", 0.5), ("sigma", p(sigma)), ("loss", p(loss)),
             ("pc", p(pc)), ("deg", p(deg)), ("grad", p(grad)), ("ws", p(ws)), ("st", st))
    call = lambda **kw: L.pdgn_flatness(*[kw.get(key, v) for key, v in names])
    for kw in ({"b": 0}, {"b": -1}, {"n": 0}, {"n": -3}, {"k": 0}, {"k": 65}, {"k": -1}, {"b": 1 << 15, "n": 1 << 12, "k": 16},
               {"eps": -1e-6}, {"eps": float("inf")}, {"eps": float("nan")}, {"coef": float("nan")}, {"coef": float("inf")},
               {"xyz": None}, {"idx": None}, {"sigma": None}, {"loss": None}, {"ws": None}, {"xyz": odd(x)}, {"idx": odd(idx)},
               {"sigma": odd(sigma)}, {"loss": odd(loss)}, {"pc": odd(pc)}, {"deg": odd(deg)}, {"grad": odd(grad)}, {"ws": odd(ws, 4)},
               {"ws": odd(ws, 8)}):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in (sigma, loss, pc, grad)) and (deg == -777).all() and (ws == -777).all()
    assert call(grad=None, ws=None) == 0 and call() == 0            # the same arguments with nothing wrong are taken
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 5. autograd
def test_the_op_differentiates_like_the_mirror_and_an_upstream_gradient_scales_exactly():
    from pdgn_amd import losses, pointops
    dev = _dev()
    b, n, k = 3, 300, 12
    host = _cloud(b, n, 77)
    x = torch.from_numpy(host).to(dev)
    idx = pointops.knnquery(k, x, x)
    want = fm.flatness(host, idx.cpu().numpy(), EPS)
    up = F(-2.5)
    grads, values = [], []
    for layout in ("B3N", "BN3"):
        leaf = (x.transpose(1, 2).contiguous() if layout == "B3N" else x.clone()).requires_grad_(True)
        deg = torch.full((b,), -1, dtype=torch.int32, device=dev)
        loss = losses.flatness(leaf, k=k, eps=EPS, degenerate=deg)
        (loss * float(up)).backward()
        torch.cuda.synchronize()
        g = leaf.grad.transpose(1, 2) if layout == "B3N" else leaf.grad
        grads.append(g.contiguous().cpu().numpy())
        values.append(loss.detach().cpu().numpy())
        assert deg.tolist() == want["degenerate"].tolist()
    print("autograd: loss %r, largest |grad| %.3g" % (float(values[0]), np.abs(grads[0]).max()))
    assert nm.same_bits(values[0], want["loss"]) and nm.same_bits(values[1], want["loss"])
    with np.errstate(all="ignore"):
        assert nm.same_bits(grads[0], up * want["grad"]) and nm.same_bits(grads[1], grads[0])
    given = losses.flatness(x.clone().requires_grad_(True), idx=idx, eps=EPS)    # the caller's lists: the same node
    assert nm.same_bits(given.detach().cpu().numpy(), want["loss"])
    with pytest.raises(ValueError):
        losses.flatness(x, k=n + 1)


# ---------------------------------------------------------------------------- 6. the metric
def test_per_cloud_without_a_floor_is_surface_stats_mean():
    """per_cloud at eps = 0 on clouds without a degenerate point is evaluation.surface_stats' sv_mean computed in fp32: the same
    eigenvalues, sigma rounded to fp32 per point and summed in fp32 in one wave's order, against fp64 throughout.  Tolerance: ten times the
    difference the MIRROR shows between its fp32 per_cloud and the fp64 mean of its own eigenvalues' sigma, for this cloud and the device's
    lists.  Measured on an MI355X: the mirror shows 1.38e-9 (relative 3.06e-8) on 4 x 512 noisy-sphere points, k = 16, and the device differs by 1.38e-9."""
    from pdgn_amd import evaluation as ev, losses, pointops
    dev = _dev()
    rng = np.random.default_rng(12)
    v = rng.standard_normal((4, 512, 3))
    host = (v / np.linalg.norm(v, axis=2, keepdims=True) * (1.0 + 0.05 * rng.standard_normal((4, 512, 1)))).astype(F)
    x = torch.from_numpy(host).to(dev)
    idx = pointops.knnquery(16, x, x)
    _, pc, _, _, deg = losses.flatness_pass(x, idx, 0.0, grad=False, per_cloud=True)
    stats = ev.surface_stats(x, k=16)
    mirror = fm.flatness(host, idx.cpu().numpy(), 0.0, grad=False)
    e = mirror["eig"].astype(np.float64)
    sv64 = (np.maximum(e[..., 0], 0.0) / ((e[..., 0] + e[..., 1]) + e[..., 2])).mean(axis=1).mean()
    shown = abs(float(mirror["per_cloud"].astype(np.float64).mean()) - sv64)
    got = abs(float(pc.double().mean().item()) - stats["sv_mean"])
    print("per_cloud mean %r against sv_mean %r: difference %.3g; the mirror shows %.3g (relative %.3g)"
          % (float(pc.double().mean().item()), stats["sv_mean"], got, shown, shown / sv64))
    assert deg.tolist() == [0] * 4 and stats["degenerate"] == 0 and shown > 0
    assert got <= 10 * shown


# ---------------------------------------------------------------------------- 7. the trainer
def _trainer(dev, overlap=True, **kw):
    from pdgn_amd.trainer import PDGNTrainer
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False, **kw)
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


FLAT = {"weight": 10.0, "k": 16, "eps": 1e-6, "levels": (0, 2, 3)}


def test_without_the_term_neither_entry_point_is_called_and_out_has_six_keys(monkeypatch):
    from pdgn_amd import losses
    dev = _dev()

    def never(*a, **k):
        raise AssertionError("a flatness entry point was called")

    monkeypatch.setattr(losses, "flatness", never)
    monkeypatch.setattr(losses, "flatness_pass", never)
    for overlap in (True, False):
        tr = _trainer(dev, overlap)
        assert tr.flatness is None
        out = tr.step(*_inputs(dev))
        torch.cuda.synchronize()
        assert sorted(out) == sorted(tr.LOSS_KEYS) and len(out) == 6 and all(np.isfinite(v.item()) for v in out.values())


@pytest.mark.parametrize("overlap", [True, False])
def test_a_step_with_the_term_is_flatness_pass_summed_over_the_named_levels(overlap):
    from pdgn_amd import losses, pointops
    dev = _dev()
    tr = _trainer(dev, overlap, flatness=FLAT)
    assert bool(tr.overlap) == overlap
    clouds = []
    handle = tr.G.register_forward_hook(lambda mod, args, out: clouds.append([c.detach().clone() for c in out]))
    out = tr.step(*_inputs(dev))
    torch.cuda.synchronize()
    handle.remove()
    assert sorted(out) == sorted(list(tr.LOSS_KEYS) + ["flatness_loss"]) and all(np.isfinite(v.item()) for v in out.values())
    gen = [c.transpose(1, 2).contiguous() for c in clouds[1]]       # the second pass's four clouds, point-major
    sizes = [c.shape[1] for c in gen]
    state = tr.flatness_state()
    floors = losses.flatness_floors(FLAT["eps"], sizes)
    assert sizes == [256, 512, 1024, 2048] and state["floors"] == floors == [8e-6, 4e-6, 2e-6, 1e-6]
    want, degenerate = [], 0
    for l in range(4):
        if l not in FLAT["levels"]:
            want.append(0.0)
            continue
        loss, _, _, _, deg = losses.flatness_pass(gen[l], pointops.knnquery(FLAT["k"], gen[l], gen[l]), floors[l], grad=False)
        want.append(loss.item())
        degenerate += int(deg.sum())
    print("overlap %s: per level %s against flatness_pass %s, degenerate %d" % (overlap, state["per_level"], want, state["degenerate"]))
    assert state["per_level"] == want and want[1] == 0.0 and all(want[l] > 0 for l in FLAT["levels"]) and state["degenerate"] == degenerate
    total = sum(want)                                            # three positive fp32 values added on the device
    assert abs(out["flatness_loss"].item() - total) <= 4 * U * total and abs(state["total"] - total) <= 4 * U * total


def _lsgan_g(scores):
    return float(((scores.detach().cpu().numpy().astype(np.float64) - 1.0) ** 2).mean())


def test_a_launch_list_with_the_term_replays_and_follows_the_weight_without_recapture():
    dev = _dev()
    reals, z1, z2 = _inputs(dev)
    tr = _trainer(dev, flatness=FLAT)
    scores = [[] for _ in tr.D]                                  # the score tensors themselves: the captured ones are the list's static buffers
    handles = [d.register_forward_hook(lambda mod, args, out, i=i: scores[i].append(out.detach())) for i, d in enumerate(tr.D)]
    tr.capture_list(reals, z1, z2)
    for hd in handles:
        hd.remove()
    gen_scores = [per[-1] for per in scores]                     # D_k's last call of the captured iteration: D_k(G(z2)_k)

    def recomposed(vals, weight):                                # 1.2 (g1 + g2 + g3) + g4 + 0.1 similar + w flatness, in fp64
        t = [_lsgan_g(s) for s in gen_scores]
        return 1.2 * (t[0] + t[1] + t[2]) + t[3] + 0.1 * vals["similar_loss"] + weight * vals["flatness_loss"]

    for _ in range(2):
        out = tr.step_list()
        torch.cuda.synchronize()
        vals = {k: v.item() for k, v in out.items()}
        print("launch list with the term: %s" % vals)
        assert len(vals) == 7 and all(np.isfinite(v) for v in vals.values()) and vals["flatness_loss"] > 0
    state = tr.flatness_state()
    assert abs(state["total"] - vals["flatness_loss"]) <= 4 * U * state["total"]
    # the weighted sum adds fp32 numbers of g_loss's size: its error is a few 2^-24 of g_loss, 1e-6 leaves a decade (as the repulsion test's)
    want = recomposed(vals, FLAT["weight"])
    print("weight %g: g_loss %r against its recomposition %r, relative %.3g" % (FLAT["weight"], vals["g_loss"], want, abs(vals["g_loss"] - want) / want))
    assert abs(vals["g_loss"] - want) <= 1e-6 * want and FLAT["weight"] * vals["flatness_loss"] > 1e-3 * want
    for change in ({"k": 8}, {"eps": 1e-3}):
        with pytest.raises(RuntimeError):
            tr.set_flatness(**change)                            # arguments of the captured launches
    tr.set_flatness(weight=0.0)                                  # the vector the list's weighted sum reads: no recapture
    out = tr.step_list()
    torch.cuda.synchronize()
    vals = {k: v.item() for k, v in out.items()}
    want = recomposed(vals, 0.0)
    print("weight 0: g_loss %r against %r, relative %.3g; flatness_loss %r" % (vals["g_loss"], want, abs(vals["g_loss"] - want) / want, vals["flatness_loss"]))
    assert abs(vals["g_loss"] - want) <= 1e-6 * want and vals["flatness_loss"] > 0
    print("launch list with the term: %s" % dict(tr._list.info))
    _drop_list(tr)


def test_repulsion_and_flatness_together():
    dev = _dev()
    reals, z1, z2 = _inputs(dev)
    tr = _trainer(dev, flatness=FLAT, repulsion={"weight": 0.5, "radius": 0.05})
    out = tr.step(reals, z1, z2)
    torch.cuda.synchronize()
    assert sorted(out) == sorted(list(tr.LOSS_KEYS) + ["flatness_loss", "repulsion_loss"]) and all(np.isfinite(v.item()) for v in out.values())
    assert tr._lw[1].tolist() == pytest.approx([1.2, 1.2, 1.2, 1.0, 0.1, 0.5, 10.0])
    assert tr.flatness_state()["total"] > 0 and tr.repulsion_state()["total"] >= 0
    tr.capture_list(reals, z1, z2)
    out = tr.step_list()
    torch.cuda.synchronize()
    assert len(out) == 8 and all(np.isfinite(v.item()) for v in out.values())
    _drop_list(tr)


def test_fit_writes_flatness_csv(tmp_path):
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    B = 4
    clouds = torch.from_numpy(_cloud(B + 1, 2048, 3)).to(dev)
    tr = _trainer(dev, flatness=FLAT)
    log = tmp_path / "log.txt"
    assert tr.fit(BatchFeeder(clouds, B, (256, 512, 1024), seed=5), 1, log=str(log)) == 1      # one batch per epoch
    torch.cuda.synchronize()
    rows = (tmp_path / "flatness.csv").read_text().splitlines()
    print("flatness.csv: %s" % rows)
    assert rows[0] == "epoch,weight,k,eps,total,level1,level2,level3,level4,degenerate" and len(rows) == 2
    cells = rows[1].split(",")
    assert cells[:4] == ["1", "10", "16", "1e-06"] and float(cells[4]) > 0 and float(cells[6]) == 0.0 and int(cells[9]) >= 0
    state = tr.flatness_state()
    assert float(cells[4]) == pytest.approx(state["total"], rel=1e-8)
    _drop_list(tr)
