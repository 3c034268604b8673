"""GPU: deterministic mode (pdgn_amd.set_deterministic).  The fixed-order adjoints of the reference-
compatible scatter-adds -- grouping, interpolation, gathering, the nndistance gradient -- on adversarial inputs (hub points
that collect thousands of contributions, values spanning 2^-20 .. 2^20 with both signs, so that the order of a sum shows in
its bits): two runs bit-equal, within the summation bound of an fp64 reference and of the default (atomic) path; the same
through autograd under torch.use_deterministic_algorithms(True); and a training step run in the mode warning that it is
not covered yet."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -23                                                  # fp32 unit roundoff (round to nearest: 2^-24; doubled for the bound)


@pytest.fixture(autouse=True)
def restore_mode():
    from pdgn_amd import _lib
    explicit, value, torch_flag = _lib._DET_EXPLICIT, _lib.deterministic(), torch.are_deterministic_algorithms_enabled()
    yield
    torch.use_deterministic_algorithms(torch_flag)
    _lib.set_deterministic(value if explicit else None)


def _values(shape, gen):
    """Magnitudes 2^-20 .. 2^20, random signs."""
    mag = torch.pow(2.0, torch.randint(-20, 21, shape, generator=gen).double()) * (1 + torch.rand(shape, generator=gen, dtype=torch.float64))
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


def _hub_idx(shape, n, gen, hub_frac=0.6):
    """Indices in [0, n): a fraction on two hub points, the rest uniform."""
    idx = torch.randint(0, n, shape, generator=gen, dtype=torch.int32)
    hub = torch.rand(shape, generator=gen) < hub_frac
    return torch.where(hub, torch.randint(0, 2, shape, generator=gen, dtype=torch.int32), idx)


def _scatter64(terms, idx, n):
    """(b, c, E) terms scattered onto (b, c, n) by idx (b, E) in fp64, and the per-output sum of |terms| and count."""
    b, c, E = terms.shape
    ix = idx.long().view(b, 1, E).expand(b, c, E)
    ref = torch.zeros((b, c, n), dtype=torch.float64).scatter_add_(2, ix, terms.double())
    absum = torch.zeros((b, c, n), dtype=torch.float64).scatter_add_(2, ix, terms.double().abs())
    cnt = torch.zeros((b, n), dtype=torch.float64).scatter_add_(1, idx.long(), torch.ones((b, E), dtype=torch.float64))
    return ref, absum, cnt.view(b, 1, n)


def _within(got, ref, absum, cnt, factor=1.0):
    err = (got.double().cpu() - ref).abs()
    bound = factor * U * (cnt + 2) * absum + 1e-30
    assert bool((err <= bound).all()), float((err / bound).max())


def _call(name, *args):
    from pdgn_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args), name)


def _run_grouping(det, grad_out, idx, n, init):
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    b, c, m, ns = grad_out.shape
    out = init.clone()
    if det:
        ws = _lib.det_workspace(out.device, (b, n, m * ns))
        _call("pdgn_grouping_backward_det", b, c, n, m, ns, ptr(grad_out), ptr(idx), ptr(ws), ptr(out), stream_of(out))
    else:
        _call("pdgn_grouping_backward", b, c, n, m, ns, ptr(grad_out), ptr(idx), ptr(out), stream_of(out))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("b,c,n,m,ns", [(2, 5, 512, 1024, 16), (1, 3, 20000, 2048, 8), (3, 70, 64, 128, 32)])
def test_grouping_backward_fixed_order(b, c, n, m, ns):
    gen = torch.Generator().manual_seed(11)
    grad_out = _values((b, c, m, ns), gen)
    idx = _hub_idx((b, m, ns), n, gen)
    init = _values((b, c, n), gen)                              # the adjoint accumulates into the caller's buffer
    g, i, z = grad_out.cuda(), idx.cuda(), init.cuda()
    first, second = _run_grouping(True, g, i, n, z), _run_grouping(True, g, i, n, z)
    assert torch.equal(first, second)
    ref, absum, cnt = _scatter64(grad_out.view(b, c, m * ns), idx.view(b, m * ns), n)
    ref += init.double()
    absum += init.double().abs()
    _within(first, ref, absum, cnt)
    _within(_run_grouping(False, g, i, n, z), ref, absum, cnt)


@pytest.mark.parametrize("b,c,n,m", [(2, 6, 4096, 256), (1, 2, 1000, 20000)])
def test_interpolation_backward_fixed_order(b, c, n, m):
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    gen = torch.Generator().manual_seed(12)
    grad_out = _values((b, c, n), gen)
    idx = _hub_idx((b, n, 3), m, gen)
    weight = torch.rand((b, n, 3), generator=gen)
    g, i, w = grad_out.cuda(), idx.cuda(), weight.cuda()

    def run(det):
        out = torch.zeros((b, c, m), device="cuda")
        if det:
            ws = _lib.det_workspace(out.device, (b, m, 3 * n))
            _call("pdgn_interpolation_backward_det", b, c, n, m, ptr(g), ptr(i), ptr(w), ptr(ws), ptr(out), stream_of(out))
        else:
            _call("pdgn_interpolation_backward", b, c, n, m, ptr(g), ptr(i), ptr(w), ptr(out), stream_of(out))
        torch.cuda.synchronize()
        return out

    first, second = run(True), run(True)
    assert torch.equal(first, second)
    terms = (grad_out.double().unsqueeze(-1) * weight.double().unsqueeze(1)).reshape(b, c, 3 * n)
    ref, absum, cnt = _scatter64(terms, idx.view(b, 3 * n), m)
    _within(first, ref, absum, cnt, 2.0)                        # (+ the rounding of each product)
    _within(run(False), ref, absum, cnt, 2.0)


@pytest.mark.parametrize("b,c,n,m", [(2, 4, 300, 5000), (4, 130, 64, 777)])
def test_gathering_backward_fixed_order(b, c, n, m):
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    gen = torch.Generator().manual_seed(13)
    grad_out = _values((b, c, m), gen)
    idx = _hub_idx((b, m), n, gen)
    g, i = grad_out.cuda(), idx.cuda()

    def run(det):
        out = torch.zeros((b, c, n), device="cuda")
        if det:
            ws = _lib.det_workspace(out.device, (b, n, m))
            _call("pdgn_gathering_backward_det", b, c, n, m, ptr(g), ptr(i), ptr(ws), ptr(out), stream_of(out))
        else:
            _call("pdgn_gathering_backward", b, c, n, m, ptr(g), ptr(i), ptr(out), stream_of(out))
        torch.cuda.synchronize()
        return out

    first, second = run(True), run(True)
    assert torch.equal(first, second)
    ref, absum, cnt = _scatter64(grad_out, idx, n)
    _within(first, ref, absum, cnt)
    _within(run(False), ref, absum, cnt)


def _hub_clouds(b, n, m, gen):
    """Cloud 1: two points near the origin, the rest far away; cloud 2: most points around the origin -> two hub points of
    cloud 1 collect most of cloud 2's nearest-neighbour gradients (and the reverse: many cloud-1 points share a neighbour)."""
    a = torch.rand((b, n, 3), generator=gen) * 10 + 5
    a[:, :2] = torch.rand((b, 2, 3), generator=gen) * 0.01
    q = torch.rand((b, m, 3), generator=gen) * 0.5
    q[:, : m // 8] = torch.rand((b, m // 8, 3), generator=gen) * 10 + 5
    return a, q


def _nndist_ref64(a, q, idx1, idx2, gd1, gd2):
    a, q, gd1, gd2 = a.double(), q.double(), gd1.double(), gd2.double()
    b = a.shape[0]
    g1 = torch.zeros_like(a)
    g2 = torch.zeros_like(q)
    ab1, ab2 = torch.zeros_like(a), torch.zeros_like(q)
    for bs in range(b):
        i1, i2 = idx1[bs].long(), idx2[bs].long()
        v = 2 * gd1[bs].unsqueeze(1) * (a[bs] - q[bs][i1])
        g1[bs] += v
        g2[bs].index_add_(0, i1, -v)
        ab1[bs] += v.abs()
        ab2[bs].index_add_(0, i1, v.abs())
        w = 2 * gd2[bs].unsqueeze(1) * (q[bs] - a[bs][i2])
        g2[bs] += w
        g1[bs].index_add_(0, i2, -w)
        ab2[bs] += w.abs()
        ab1[bs].index_add_(0, i2, w.abs())
    n1 = 1 + torch.stack([torch.bincount(idx2[bs].long(), minlength=a.shape[1]) for bs in range(b)]).double().unsqueeze(-1)
    n2 = 1 + torch.stack([torch.bincount(idx1[bs].long(), minlength=q.shape[1]) for bs in range(b)]).double().unsqueeze(-1)
    return (g1, ab1, n1), (g2, ab2, n2)


@pytest.mark.parametrize("b,n,m", [(2, 1024, 4096), (3, 3000, 500)])
def test_nndistance_grad_fixed_order(b, n, m):
    import importlib
    from pdgn_amd import _lib
    nd = importlib.import_module("pdgn_amd.structural_losses.nn_distance")
    gen = torch.Generator().manual_seed(14)
    a, q = _hub_clouds(b, n, m, gen)
    gd1, gd2 = _values((b, n), gen), _values((b, m), gen)
    A, Q = a.cuda(), q.cuda()
    _, idx1, _, idx2 = nd.NNDistance(A, Q)

    def run(det):
        _lib.set_deterministic(det)
        out = nd.NNDistanceGrad(A, Q, idx1, idx2, gd1.cuda(), gd2.cuda())
        torch.cuda.synchronize()
        return out

    (f1, f2), (s1, s2) = run(True), run(True)
    assert torch.equal(f1, s1) and torch.equal(f2, s2)
    refs = _nndist_ref64(a, q, idx1.cpu(), idx2.cpu(), gd1, gd2)
    for got in ((f1, f2), run(False)):
        for g, (ref, absum, cnt) in zip(got, refs):
            _within(g, ref, absum, cnt, 2.0)


def test_autograd_under_torch_flag_is_bit_repeatable():
    """pointops grouping / interpolation / gathering and nn_distance through autograd with only torch's flag set."""
    from pdgn_amd import _lib, pointops
    from pdgn_amd.structural_losses import nn_distance          # (the autograd function)
    _lib.set_deterministic(None)                                # follow torch
    torch.use_deterministic_algorithms(True)
    assert _lib.deterministic()
    gen = torch.Generator().manual_seed(15)
    b, c, n, m, ns = 2, 8, 700, 600, 16
    feats = _values((b, c, n), gen).cuda()
    gidx = _hub_idx((b, m, ns), n, gen).cuda()
    sidx = _hub_idx((b, m), n, gen).cuda()
    iidx = _hub_idx((b, 2 * n, 3), n, gen).cuda()
    iw = torch.rand((b, 2 * n, 3), generator=gen).cuda()
    up = _values((b, c, m, ns), gen).cuda()
    a, q = _hub_clouds(b, 900, 1500, gen)
    gd1, gd2 = _values((b, 900), gen).cuda(), _values((b, 1500), gen).cuda()

    def once():
        f = feats.clone().requires_grad_(True)
        x = pointops.grouping(f, gidx)
        loss = (x * up).sum() + (pointops.gathering(f, sidx) * up[..., 0]).sum() \
            + (pointops.interpolation(f, iidx, iw) * feats.repeat(1, 1, 2)).sum()
        loss.backward()
        pa, pq = a.cuda().requires_grad_(True), q.cuda().requires_grad_(True)
        d1, d2 = nn_distance(pa, pq)
        ((d1 * gd1).sum() + (d2 * gd2).sum()).backward()
        torch.cuda.synchronize()
        return f.grad, pa.grad, pq.grad

    for x, y in zip(once(), once()):
        assert torch.equal(x, y)


def test_step_warns_that_it_is_not_covered():
    """The mode covers the pointops / nn_distance adjoints only: a training step run with it on (here through torch's flag)
    says that it is not bitwise repeatable; with the mode off it says nothing."""
    import warnings
    from pdgn_amd import _lib
    from pdgn_amd.trainer import DeterminismWarning, PDGNTrainer, noise, synthetic_batch
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    B = 6
    reals = synthetic_batch(B, dev)
    g = torch.Generator().manual_seed(9)
    z1, z2 = noise(B, dev, g), noise(B, dev, g)
    _lib.set_deterministic(False)
    with warnings.catch_warnings():
        warnings.simplefilter("error", DeterminismWarning)
        tr.step(reals, z1, z2)
    _lib.set_deterministic(None)
    torch.use_deterministic_algorithms(True, warn_only=True)
    with pytest.warns(DeterminismWarning, match="not bitwise repeatable"):
        out = tr.step(reals, z1, z2)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v)) for v in out.values())
