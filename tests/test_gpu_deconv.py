"""GPU parity of the point-deconvolution stack: feature-space kNN, window gather-sum, PointDeconv,
PointGenerator / discriminators and one G+D step, all through the HIP C ABI.
Float tolerance 1e-4 relative (BASELINE.json north_star); kNN indices exact outside near-ties."""
import copy

import numpy as np
import pytest
import torch

from step_checks import assert_block_gradients, check_step_gradients
from hashweights import fill_module, hash_tensor
from oracle import pdgnet_ref
from torch_standins import EdgeGatherSumTorch

pytestmark = pytest.mark.gpu
ROOT_DIR = __import__('os').path.dirname(__import__('os').path.dirname(__import__('os').path.abspath(__file__)))


def dev(a):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.cuda()


def knn_agreement(x, k, idx_gpu):
    """Rows whose oracle top-(k+2) distances are separated by more than the fp32 Gram-form
    rounding must match exactly; near-tie rows are excused (SURVEY.md section 7 'hard parts')."""
    idx_ref, dist = pdgnet_ref.feature_knn(x.double(), k)
    ds = dist.sort(dim=2)[0][:, :, :k + 2]
    scale = dist.abs().amax(dim=2, keepdim=True) + 1e-12
    safe = ((ds[:, :, 1:] - ds[:, :, :-1]) / scale).amin(dim=2) > 2e-6
    same = (idx_ref == idx_gpu.cpu().long()).all(dim=2)
    return safe, same


@pytest.mark.parametrize("B,F,N,k", [(2, 6, 24, 5), (3, 32, 128, 10), (2, 64, 256, 10), (2, 128, 512, 10),
                                     (2, 256, 1024, 10), (1, 256, 2048, 10), (2, 7, 100, 4), (1, 40, 1500, 16)])
def test_feature_knn(B, F, N, k):
    from pdgn_amd.deconv import feature_knn
    x = torch.from_numpy(np.random.default_rng(F + N).standard_normal((B, F, N)).astype(np.float32))
    idx = feature_knn(dev(x), k)
    assert idx.dtype == torch.int32 and idx.shape == (B, N, k)
    safe, same = knn_agreement(x, k, idx)
    assert safe.float().mean() > 0.9
    assert same[safe].all(), "kNN differs on %d well-separated rows" % int((~same[safe]).sum())
    assert same.float().mean() > 0.99


@pytest.mark.parametrize("B,Fc,Fv,N,k", [(3, 32, 32, 256, 10), (2, 64, 64, 512, 10), (2, 128, 128, 1024, 10), (2, 24, 40, 200, 6)])
def test_feature_knn_ignores_channels_constant_over_the_points(B, Fc, Fv, N, k):
    """A block's input is cat([g broadcast over the points, x]) (models/PDGNet_v2.py:708) and the reference builds the graph from that
    tensor (:447-458).  The broadcast channels add (g_f - g_f)^2 = 0 to every pairwise distance, so the graph of the varying channels
    alone -- what deconv.start_feature_knn builds since round 6 -- is the same graph: equal to the fp64 graph of the CONCATENATED
    tensor on every row whose distances are separated by more than rounding, and to the HIP graph of the concatenated tensor on
    >= 99 % of all rows (there the Gram form's cancellation noise 2|g|^2 - 2|g|^2 flips near-ties)."""
    from pdgn_amd import deconv
    from pdgn_amd.deconv import feature_knn, start_feature_knn
    rng = np.random.default_rng(Fc + N)
    xt = torch.from_numpy(rng.standard_normal((B, N, Fv)).astype(np.float32))
    const = torch.from_numpy((3.0 * rng.standard_normal((B, Fc))).astype(np.float32))
    full = torch.cat((const.unsqueeze(2).expand(-1, -1, N), xt.transpose(1, 2)), 1).contiguous()        # (B, Fc + Fv, N)
    assert not deconv._KNN_CONST
    idx, ready = start_feature_knn(dev(xt), dev(const), k)
    if ready is not None:
        ready.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(idx, feature_knn(dev(xt.transpose(1, 2).contiguous()), k))
    safe, same = knn_agreement(full, k, idx)                       # the oracle sees the concatenated tensor
    assert safe.float().mean() > 0.9
    assert same[safe].all(), "graph differs from the concatenated tensor's on %d well-separated rows" % int((~same[safe]).sum())
    agree = (idx == feature_knn(dev(full), k)).all(dim=2).float().mean().item()
    assert agree > 0.99, agree


def test_feature_knn_golden(golden):
    from pdgn_amd.deconv import feature_knn
    g = golden("edge_features.npz")
    idx = feature_knn(dev(g["x"]), int(g["k"]))
    np.testing.assert_array_equal(idx.cpu().numpy(), g["idx"])


def test_feature_knn_duplicates_drop_rank0():
    from pdgn_amd.deconv import feature_knn
    x = torch.zeros(1, 4, 40)
    x[0, :, 20:] = 1.0                     # two clusters of identical points: ties by index
    idx = feature_knn(dev(x), 6).cpu()
    assert idx[0, 0].tolist() == [1, 2, 3, 4, 5, 6]        # rank 0 (= index 0) dropped
    assert idx[0, 5].tolist() == [1, 2, 3, 4, 5, 6]        # rank 0 is index 0, NOT self (ref quirk)
    assert idx[0, 30].tolist() == [21, 22, 23, 24, 25, 26]


@pytest.mark.parametrize("F,N", [(32, 256), (64, 512), (256, 1024)])
def test_feature_knn_mass_ties_on_the_producer_consumer_kernel(F, N):
    """Regular shapes (the persistent producer / consumer kernel): clusters of 100 identical points -- more equal distances
    than a survivor queue holds (in-scan merges) and more than 32 entries at the K-th distance (the general merge path);
    integer features, so every distance is exact and the expected graph is the index order inside the query's cluster."""
    from pdgn_amd.deconv import feature_knn
    k = 10
    cluster = torch.arange(N) // 100
    x = (cluster.float() * 3.0).view(1, 1, N).expand(2, F, N).contiguous()
    x[1] = x[1].flip(-1)                                    # second sample: clusters in reverse index order
    idx = feature_knn(dev(x), k).cpu()
    for b in range(2):
        cl = cluster if b == 0 else cluster.flip(0)
        for q in (0, 1, 57, 99, 100, 163, N - 57, N - 1):
            members = torch.nonzero(cl == cl[q]).flatten().tolist()
            assert len(members) >= k + 1
            assert idx[b, q].tolist() == members[1:k + 1], (b, q)      # rank 0 (the cluster's first index) dropped


@pytest.mark.parametrize("B,N,k,ldy,spec", [(2, 50, 10, 64, (6, 5, 8, 0, 48)), (2, 33, 10, 40, (10, 1, 3, 1, 31)),
                                            (3, 64, 10, 32, (1, 10, 16, 0, 16)), (2, 40, 4, 24, (3, 2, 4, 4, -1)),
                                            (2, 512, 10, 7200, (6, 5, 1024, 0, 6144)),
                                            # ragged for the cache-aware task mapping: rows not a multiple of the block's, a partial last chunk
                                            (3, 1000, 10, 1912, (6, 5, 160, 0, 960)), (3, 1000, 10, 1912, (10, 1, 72, 1120, 1840))])
def test_window_gather_sum_forward_backward(B, N, k, ldy, spec):
    from pdgn_amd.deconv import EdgeGatherSum
    rng = np.random.default_rng(N)
    Y = torch.from_numpy(rng.standard_normal((B, N, ldy)).astype(np.float32))
    idx = torch.from_numpy(rng.integers(0, N, (B, N, k)).astype(np.int32))
    T, P, C, off, offc = spec
    bias = torch.from_numpy(rng.standard_normal(C).astype(np.float32))
    Yg, bg = dev(Y).requires_grad_(True), dev(bias).requires_grad_(True)
    (out,) = EdgeGatherSum.apply(Yg, dev(idx), (spec,), bg)
    Yc, bc = Y.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    (ref,) = EdgeGatherSumTorch.apply(Yc, idx, (spec,), bc)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-5)
    gout = torch.from_numpy(rng.standard_normal((B, N, P, C)).astype(np.float32))
    out.backward(dev(gout))
    ref.backward(gout)
    np.testing.assert_allclose(Yg.grad.cpu().numpy(), Yc.grad.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(bg.grad.cpu().numpy(), bc.grad.numpy(), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("min_rows", [1024, 1], ids=["dispatch", "own_kernels"])
@pytest.mark.parametrize("name", ["plain_k4", "bilateral_k4", "plain_k10", "bilateral_k10"])
def test_pointdeconv_golden(golden, name, min_rows, monkeypatch):
    """The reference's own block classes (models/PDGNet_v2.py:547-650): outputs, input and parameter gradients, BatchNorm
    buffers.  The fixtures are 32-64 rows, which the dispatch of fused.LinearCL hands to torch's matmul; the
    `own_kernels` arm lowers that threshold to one row, so that every dense layer of the block -- forward, input
    gradient and weight gradient -- runs on pdgn_gemm_nt / _nn / _tn / the thin kernels and the reference's grad_x /
    grad_pc / grad.<param> vectors bite on them."""
    from pdgn_amd import fused
    from pdgn_amd.deconv import PointDeconv
    monkeypatch.setattr(fused, "_OWN_MIN_ROWS", min_rows)
    g = golden("deconv_%s.npz" % name)
    bilateral = name.startswith("bilateral")
    mod = fill_module(PointDeconv(int(g["F"]), int(g["Fout"]), int(g["k"]), bilateral=bilateral), salt=3).cuda()
    x = dev(g["x"]).requires_grad_(True)
    pc = dev(g["pc"]).requires_grad_(True) if bilateral else None
    mod.train()
    y = mod(x, pc)                                     # kNN graph from the HIP kernel
    if float(g["knn_margin"]) > 1e-5:
        np.testing.assert_allclose(y.detach().cpu().numpy(), g["y_train"], rtol=1e-4, atol=2e-5)
    x.grad = None
    mod2 = fill_module(PointDeconv(int(g["F"]), int(g["Fout"]), int(g["k"]), bilateral=bilateral), salt=3).cuda()
    mod2.train()
    y = mod2(x, pc, idx=dev(g["idx"].astype(np.int32)))  # oracle graph: pure float parity
    np.testing.assert_allclose(y.detach().cpu().numpy(), g["y_train"], rtol=1e-4, atol=2e-5)
    y.backward(dev(g["gout"]))
    assert_block_gradients(mod2, g, x, pc)                     # 5e-6 of each tensor's scale: 2x the worst measured (step_checks.py)
    for n, b in mod2.named_buffers():
        if "num_batches" not in n:
            np.testing.assert_allclose(b.cpu().numpy(), g["stat." + n], rtol=1e-4, atol=1e-5, err_msg=n)
    mod2.eval()
    with torch.no_grad():
        y_ev = mod2(x, pc, idx=dev(g["idx"].astype(np.int32)))
    np.testing.assert_allclose(y_ev.cpu().numpy(), g["y_eval"], rtol=1e-4, atol=2e-5)


def block_big_errors(g, mode):
    """One forward / backward of the F = 128, N = 512 bilateral block in arithmetic `mode` against the imported reference's fixture
    (tests/golden/deconv_bilateral_big.npz): {name: (error vs the reference's fp32 run, error vs the reference's fp64 run, the fp32
    reference's own distance from its fp64 run)} -- every error as max |a - b| / max |b| of the tensor -- and the contraction log."""
    from hashweights import hash_tensor
    from pdgn_amd import _lib, fused
    from pdgn_amd.deconv import PointDeconv
    _lib.set_gemm_mode(mode)
    F, Fo, k, N, B = (int(g[n]) for n in ("F", "Fout", "k", "N", "B"))
    name = "bilateral_big"
    mod = fill_module(PointDeconv(F, Fo, k, bilateral=True), salt=3).cuda().train()
    x = hash_tensor(name + "_x", (B, F, N)).cuda().requires_grad_(True)
    pc = hash_tensor(name + "_pc", (B, 3, N)).cuda().requires_grad_(True)
    gout = hash_tensor(name + "_gout", (B, Fo, 2 * N)).cuda()
    log = fused.GEMM_LOG = []
    y = mod(x, pc, idx=dev(g["idx"].astype(np.int32)))              # the reference's own graph: pure float parity
    y.backward(gout)
    torch.cuda.synchronize()
    fused.GEMM_LOG = None

    def rel(a, b):
        return float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))
    yn = y.detach().cpu().numpy()
    out = {"y": (rel(yn, g["y_train"]), rel(yn, g["y_train64"]), float(g["ref32_err_y"])),
           "y_elementwise": float((np.abs(yn.astype(np.float64) - g["y_train"]) / (1e-4 * np.abs(g["y_train"]) + 2e-5)).max()),
           "grad_x": (rel(x.grad.cpu().numpy(), g["grad_x"]), rel(x.grad.cpu().numpy(), g["grad_x64"]), float(g["ref32_err_grad_x"])),
           "grad_pc": (rel(pc.grad.cpu().numpy(), g["grad_pc"]), rel(pc.grad.cpu().numpy(), g["grad_pc64"]), float(g["ref32_err_grad_pc"]))}
    gmax = max(float(g["gmax." + n]) for n, _ in mod.named_parameters())
    for n, p in mod.named_parameters():
        stride = int(g["gstride." + n])
        got = p.grad.reshape(-1)[::stride].cpu().numpy().astype(np.float64)
        if float(g["gmax." + n]) < 1e-6 * gmax:                    # a bias in front of a training-mode BatchNorm: analytically zero
            out["zero." + n] = float(np.abs(got - g["grad." + n]).max() / gmax)
        else:
            amax = float(g["gmax." + n])
            out["grad." + n] = (float(np.abs(got - g["grad." + n]).max() / amax), float(np.abs(got - g["grad64." + n]).max() / amax),
                                float(g["ref32_err." + n]))
            out["norm." + n] = abs(float(p.grad.double().norm()) / float(g["gnorm." + n]) - 1.0)
    for n, b in mod.named_buffers():
        if "num_batches" not in n:
            out["stat." + n] = float((np.abs(b.cpu().numpy().astype(np.float64) - g["stat." + n]) / (1e-4 * np.abs(g["stat." + n]) + 1e-5)).max())
    return out, log


@pytest.mark.parametrize("mode", ["x2", "x3", "fp32"])
def test_bilateral_block_at_a_two_part_shape_against_the_reference(golden, mode):
    """VERDICT r5 missing #2 / next #1c: the reference's bilateral_upsample_edgeConv (models/PDGNet_v2.py:590-650), IMPORTED and run
    in gen_golden.py at F = 128, Fout = 128, N = 512, B = 4, k = 10 -- a shape whose per-point product (2048 x 6432 x 128) and
    conv2 dense half (2048 x 256 x 2560) run on the big-tile two-part kernels in the default mode -- against this code in all
    three arithmetic modes.  y: the north star's 1e-4 (elementwise, + 2e-5) against the reference's fp32 run.  Gradients: at this
    size the reference's fp32 run is itself up to 9e-5 (grad_x, grad_pc) and 6e-4 (conv_all.4's bias gradient, a difference of
    nearly cancelling terms) of a tensor's largest element away from THE SAME reference evaluated in fp64 (stored beside it:
    ref32_err.*), so a bound against the fp32 run alone would measure the reference's rounding.  Held here: against the fp64
    run, every gradient within 2.5e-6 of its tensor's largest element (measured 0.8e-7 .. 1.1e-6 in all three modes,
    profiles/r06_block_big_error.txt: this code is 10 - 1000x closer to the exact gradients than the fp32 reference is);
    against the fp32 run, within 5e-6 + 1.5 x the reference's own distance from fp64; parameter-gradient norms to 2e-5;
    BatchNorm buffers to 1e-4."""
    from pdgn_amd import _lib
    g = golden("deconv_bilateral_big.npz")
    try:
        err, log = block_big_errors(g, mode)
    finally:
        _lib.set_gemm_mode(_lib.DEFAULT_GEMM_MODE)
    assert err["y_elementwise"] <= 1.0, err["y_elementwise"]
    assert err["y"][1] <= 2e-6, err["y"]
    for n, e in err.items():
        if n.startswith("grad"):
            vs32, vs64, ref = e
            assert vs64 <= 2.5e-6, (mode, n, e)
            assert vs32 <= 5e-6 + 1.5 * ref, (mode, n, e)
        elif n.startswith("zero."):
            assert e <= 1e-6, (mode, n, e)
        elif n.startswith("norm."):
            assert e <= 2e-5, (mode, n, e)
        elif n.startswith("stat."):
            assert e <= 1.0, (mode, n, e)
    # the products the fixture is there for ran on the library's own kernels at the shapes named above
    shapes = {(kind, m, n, k) for kind, m, n, k in log}
    assert ("nt", 2048, 6432, 128) in shapes and ("nt", 2048, 256, 2560) in shapes, sorted(shapes)


def test_generator_golden(golden):
    from pdgn_amd.generator import PointDiscriminator, PointGenerator
    g = golden("generator_b6.npz")
    G = fill_module(PointGenerator(), salt=1).cuda().train()
    with torch.no_grad():
        outs = G(dev(g["z"]), idx=[dev(g["idx%d" % i].astype(np.int32)) for i in (1, 2, 3, 4)])
    for i, o in enumerate(outs):
        gold = g["p%d" % (i + 1)]
        np.testing.assert_allclose(o.cpu().numpy(), gold, rtol=1e-4, atol=1e-4 * np.abs(gold).max())
    for i in (1, 2, 3, 4):
        D = fill_module(PointDiscriminator(i), salt=9 + i).cuda().train()
        with torch.no_grad():
            np.testing.assert_allclose(D(dev(g["p%d" % i])).cpu().numpy(), g["d%d" % i], rtol=1e-4, atol=1e-5)
    # with its own kNN graphs the generator must reproduce the reference except where a graph
    # near-tie flipped: compare stage 1 (a single graph) only when that graph was well separated
    G2 = fill_module(PointGenerator(), salt=1).cuda().train()
    with torch.no_grad():
        own = G2(dev(g["z"]))
    assert all(torch.isfinite(o).all() for o in own)
    if float(g["knn_margins"][0]) > 1e-5:
        np.testing.assert_allclose(own[0].cpu().numpy(), g["p1"], rtol=1e-4, atol=1e-4)


def _composed_step(B, graph, monkeypatch):
    from pdgn_amd import deconv
    from pdgn_amd.trainer import PDGNTrainer
    from torch_standins import feature_knn_torch
    if graph == "fp64":
        monkeypatch.setattr(deconv, "feature_knn", lambda x, k: feature_knn_torch(x.double(), k))
    tr = PDGNTrainer(device="cuda", distributed=False)
    fill_module(tr.G, salt=1)
    for i, d in enumerate(tr.D):
        fill_module(d, salt=10 + i)
    tr.train()
    reals = [dev(hash_tensor("real%d" % i, (B, 3, n), 0.8)) for i, n in enumerate((256, 512, 1024, 2048))]
    out = tr.step(reals, dev(hash_tensor("step_z1", (B, 128), 0.2)), dev(hash_tensor("step_z2", (B, 128), 0.2)))
    return tr, out


def _raw_sums(part, M, block, N):
    """[sum x | sum x^2] per column from BLOCK-SHIFTED partials (rows of [sum (x - pv) | sum (x - pv)^2 | pv] over blocks of
    `block` rows, pv = the block's first row), in fp64."""
    p = part.double().cpu().numpy()
    nb = np.clip(M - np.arange(p.shape[0]) * block, 0, block).astype(np.float64)[:, None]
    s, q, pv = p[:, :N], p[:, N:2 * N], p[:, 2 * N:]
    live = nb[:, 0] > 0
    s, q, pv, nb = s[live], q[live], pv[live], nb[live]
    return np.concatenate([(s + nb * pv).sum(0), (q + 2 * pv * s + nb * pv * pv).sum(0)])


LOSS_KEYS = ("d_loss1", "d_loss2", "d_loss3", "d_loss4", "g_loss", "similar_loss")


@pytest.mark.parametrize("graph", ["fp64", "hip"])
def test_one_step_vs_composed_reference(golden, monkeypatch, graph):
    """models/PDGNet_v2.py:171-256 at B=4, hash weights, against the composed-reference fixture.
    The reference's Gram-form fp32 distances make the kNN graph itself rounding-dependent (a CUDA
    run of the reference differs from its own CPU run the same way), so parity is split as
    SURVEY.md section 7 prescribes: (fp64) with a rounding-free graph the whole iteration --
    losses and an Adam-updated weight slice -- matches to 2e-3; (hip) with the HIP kernel's graph
    (identical to torch's fp32 graph on this device, see test_feature_knn) the losses stay within
    the spread that graph near-ties cause at this tiny batch (the tight arm is the B=16 fixture below)."""
    g = golden("step_b4.npz")
    tr, out = _composed_step(4, graph, monkeypatch)
    # (hip): WHICH near-ties flip depends on the rounding pattern of everything upstream -- at B=4 the BatchNorm1d
    # layers amplify 1e-6 differences (a fused layer that merely sums in another order, as accurate against fp64 as
    # torch's, moved similar_loss by 23 %).  The arithmetic is pinned by the fp64 arm; this arm only checks that the
    # iteration with the device's own graphs lands in the same regime.
    for key in LOSS_KEYS:
        if graph == "fp64":
            np.testing.assert_allclose(out[key].item(), g[key], rtol=2e-3, err_msg=key)
        else:
            band = 0.1 if key.startswith("d_loss") else 0.5
            assert abs(out[key].item() - float(g[key])) <= band * abs(float(g[key])), (key, out[key].item(), float(g[key]))
    if graph == "fp64":
        np.testing.assert_allclose(tr.G.fc1[0].weight.detach()[:4, :8].cpu().numpy(), g["g_fc1_w_after"],
                                   rtol=1e-2, atol=1e-5)


@pytest.mark.parametrize("B", [8, 35])
def test_one_step_with_the_references_own_graphs(golden, monkeypatch, B):
    """The whole iteration with the kNN graphs forced equal on both sides at every stage:
    tests/golden/step_b8_graphs.npz holds, next to the losses, the eight graphs the reference's get_edge_features[_xyz]
    picked (four blocks x two generator passes).  Feeding them to the HIP step in call order leaves pure arithmetic:
    all six losses to 2e-3 and -- what pins the BACKWARD of the whole network, own MFMA kernels included (VERDICT r2,
    weak #1) -- the norm of the generator's gradient, the gradient norm of EVERY generator parameter, leading slices of
    thirteen of them (and of three per discriminator) and the first Adam update in units of the learning rate, all from
    the reference's lossG.backward() / lossD.backward() (models/PDGNet_v2.py:189-256).
    B=35 is BASELINE.json configs[1]'s own batch (README.md:34-45 `--batch_size 35`; VERDICT r3, missing #1): the same
    numbers at the batch the metric is quoted on (tests/golden/step_b35_graphs.npz, gen_golden.py --graphs35)."""
    from pdgn_amd import deconv
    g = golden("step_b%d_graphs.npz" % B)
    graphs = [dev(g["graph%d" % i].astype(np.int32)) for i in range(8)]
    calls = []

    def forced(x, k):
        i = len(calls)
        calls.append(tuple(x.shape))
        assert graphs[i].shape == (x.shape[0], x.shape[2], k), (i, x.shape, graphs[i].shape)
        return graphs[i]
    monkeypatch.setattr(deconv, "feature_knn", forced)
    tr, out = _composed_step(B, "forced", monkeypatch)
    assert len(calls) == 8
    for key in LOSS_KEYS:
        np.testing.assert_allclose(out[key].item(), float(g[key]), rtol=2e-3, err_msg=key)
    check_step_gradients(tr, g)


def test_one_step_b16_device_graphs(golden, monkeypatch):
    """The same iteration at B=16 with the device's OWN kNN graphs against the reference's CPU run (losses only,
    tests/golden/step_b16.npz).  The reference's Gram-form fp32 distances make the graph itself rounding-dependent (its
    CPU graph, a CUDA graph and this device's graph differ in near-ties); with BatchNorm over 16 samples the spread this
    causes is a few percent, against +-50 % at B=4.  Arithmetic is pinned by the forced-graph test above."""
    g = golden("step_b16.npz")
    tr, out = _composed_step(16, "hip", monkeypatch)
    for key in LOSS_KEYS:
        np.testing.assert_allclose(out[key].item(), float(g[key]), rtol=8e-2, err_msg=key)


def test_config_c1_batch2_plumbing(golden, monkeypatch):
    """BASELINE.json configs[0] (batch_size = 2): tests/golden/step_b2.npz.  BatchNorm1d over TWO samples amplifies fp32
    rounding ~100x per stage (the fp32 reference is 5e-3 away from its own fp64 evaluation, tests/test_generator_host.py),
    so this is the plumbing check the config asks for: the iteration runs at B=2, every loss is finite and lands in the
    reference's regime (measured spread at this batch: up to 15 % on d_loss4 between two equally accurate fp32 evaluations)."""
    g = golden("step_b2.npz")
    tr, out = _composed_step(2, "fp64", monkeypatch)
    for key in LOSS_KEYS:
        assert np.isfinite(out[key].item())
        np.testing.assert_allclose(out[key].item(), float(g[key]), rtol=0.5, err_msg=key)


def test_feature_knn_equals_torch_fp32_graph_on_device():
    """Same-precision check: on generator activations the HIP graph equals the graph torch's own
    fp32 bmm + stable sort picks on this GPU for >= 99.9% of the rows."""
    from pdgn_amd.deconv import feature_knn
    from torch_standins import feature_knn_torch
    torch.manual_seed(3)
    for F, N in ((32, 128), (64, 256), (128, 512), (256, 1024)):
        x = torch.nn.functional.leaky_relu(torch.randn(8, F, N, device="cuda"))
        same = (feature_knn(x, 10) == feature_knn_torch(x, 10)).all(dim=2).float().mean().item()
        assert same > 0.999, (F, N, same)


def test_full_size_step_properties():
    """BASELINE.json configs[1] shape (B=35, 256->2048): one iteration runs, losses are finite,
    every G parameter receives a finite gradient, kNN rows are duplicate-free."""
    from pdgn_amd.deconv import feature_knn
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    torch.manual_seed(9999)
    tr = PDGNTrainer(device="cuda", distributed=False)
    tr.train()
    B = 35
    reals = synthetic_batch(B, "cuda")
    assert [r.shape[2] for r in reals] == [256, 512, 1024, 2048]
    out = tr.step(reals, noise(B, "cuda"), noise(B, "cuda"))
    assert all(torch.isfinite(v) for v in out.values())
    grads = [p.grad for p in tr.G.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and sum(g.abs().sum() for g in grads) > 0
    x = torch.randn(B, 256, 1024, device="cuda")
    idx = feature_knn(x, 10).long()
    srt = idx.sort(dim=2)[0]
    assert (srt[:, :, 1:] != srt[:, :, :-1]).all()
    assert (idx != torch.arange(1024, device="cuda").view(1, -1, 1)).all()   # self is rank 0 for random data


@pytest.mark.parametrize("rows,C,act,use_mul,training", [(1000, 16, "leaky_relu", True, True), (5000, 64, "leaky_relu", False, True),
                                                         (3333, 1024, "leaky_relu", True, True), (777, 24, "relu", False, True),
                                                         (2048, 512, "relu", False, False), (100000, 32, "none", True, True)])
def test_fused_bn_act_vs_torch(rows, C, act, use_mul, training):
    from pdgn_amd.fused import bn_act
    from torch_standins import bn_act_torch
    rng = np.random.default_rng(rows + C)
    x = torch.from_numpy((rng.standard_normal((rows, C)) * 2 + 0.7).astype(np.float32))
    mul = torch.from_numpy(rng.standard_normal((rows, C)).astype(np.float32)) if use_mul else None
    gout = torch.from_numpy(rng.standard_normal((rows, C)).astype(np.float32))
    res = []
    for impl, to in ((bn_act, dev), (bn_act_torch, lambda t: t.double())):
        bn = torch.nn.BatchNorm1d(C)
        fill_module(bn, salt=2)
        bn = bn.cuda() if impl is bn_act else bn.double()
        bn.train(training)
        xi = to(x).requires_grad_(True)
        mi = to(mul).requires_grad_(True) if use_mul else None
        y = impl(xi, bn, training, act=act, mul=mi)
        y.backward(to(gout))
        res.append([t.detach().cpu().double().numpy() for t in
                    (y, xi.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)
                    + ((mi.grad,) if use_mul else ())])
    names = ["y", "dx", "dgamma", "dbeta", "running_mean", "running_var", "dmul"]
    for name, a, b in zip(names, *res):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(b).max()), err_msg=name)


@pytest.mark.parametrize("B,N,C2,training", [(3, 50, 24, True), (5, 128, 64, True), (2, 1024, 512, True), (4, 33, 16, False)])
def test_fused_bn_act_interleaved_store(B, N, C2, training):
    """bn_act(..., interleave_n=N): BatchNorm + ReLU of a block's conv2 output (B*N, 2F) stored as the interleaved (B*2N, F) cloud
    (models/PDGNet_v2.py:645-647) by the apply pass itself, and its adjoint reading dy in that layout -- against the torch form
    (BatchNorm, ReLU, then view / permute / reshape) in fp64: values, input gradient, parameter gradients, running statistics."""
    from pdgn_amd.fused import bn_act
    from torch_standins import bn_act_torch
    rng = np.random.default_rng(B * N + C2)
    x = torch.from_numpy((rng.standard_normal((B * N, C2)) * 1.5 - 0.3).astype(np.float32))
    gout = torch.from_numpy(rng.standard_normal((B * 2 * N, C2 // 2)).astype(np.float32))
    res = []
    for impl, to in ((bn_act, dev), (bn_act_torch, lambda t: t.double())):
        bn = torch.nn.BatchNorm1d(C2)
        fill_module(bn, salt=4)
        bn = bn.cuda() if impl is bn_act else bn.double()
        bn.train(training)
        xi = to(x).requires_grad_(True)
        y = impl(xi, bn, training, act="relu", interleave_n=N)
        assert tuple(y.shape) == (B * 2 * N, C2 // 2)
        y.backward(to(gout))
        res.append([t.detach().cpu().double().numpy() for t in (y, xi.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)])
    # and the layout itself, spelled out: row b*2N + j*N + n, channel c  <-  row b*N + n, channel 2c + j
    for name, a, b in zip(["y", "dx", "dgamma", "dbeta", "running_mean", "running_var"], *res):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(b).max()), err_msg=name)
    y_cpu = res[1][0].reshape(B, 2, N, C2 // 2)
    bn = torch.nn.BatchNorm1d(C2)
    fill_module(bn, salt=4)
    bn = bn.double().train(training)
    plain = torch.relu(bn(x.double())).detach().numpy().reshape(B, N, C2 // 2, 2)
    np.testing.assert_allclose(y_cpu, plain.transpose(0, 3, 1, 2), rtol=1e-12)


@pytest.mark.parametrize("shift", [30.0, 300.0, 1000.0])
def test_bn_act_large_mean(shift):
    """|mean| >> std (round-1 advice): the statistics pass sums x - x[0] (shifted sums), so that the variance does not
    cancel -- output, input gradient and running statistics against fp64 at the north star's 1e-4."""
    from pdgn_amd.fused import bn_act
    rows, C = 50000, 64
    g = torch.Generator(device="cuda").manual_seed(int(shift))
    x = (torch.randn(rows, C, device="cuda", generator=g) * torch.linspace(0.5, 2.0, C, device="cuda") + shift).requires_grad_(True)
    gout = torch.randn(rows, C, device="cuda", generator=g)
    bn = torch.nn.BatchNorm1d(C).cuda().train()
    y = bn_act(x, bn, True, act="none")                     # (an activation's kink would make the gradient check ill-posed)
    y.backward(gout)
    xr = x.detach().double().requires_grad_(True)
    ref_bn = torch.nn.BatchNorm1d(C).cuda().double().train()
    yr = ref_bn(xr)
    yr.backward(gout.double())
    assert (y.detach().double() - yr.detach()).abs().max().item() < 1e-4
    assert (x.grad.double() - xr.grad).abs().max().item() < 1e-4 * max(1.0, xr.grad.abs().max().item())
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), ref_bn.running_mean.cpu().numpy(), rtol=1e-5)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), ref_bn.running_var.cpu().numpy(), rtol=2e-4)


def test_graphed_step_equals_eager_step():
    """hipGraph replay (trainer.capture / step_graphed) reproduces the eager iteration."""
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    B = 4
    reals = synthetic_batch(B, "cuda")
    zs = [(noise(B, "cuda", torch.Generator().manual_seed(i)), noise(B, "cuda", torch.Generator().manual_seed(50 + i)))
          for i in range(3)]
    res = []
    for graphed in (False, True):
        torch.manual_seed(11)
        tr = PDGNTrainer(device="cuda", distributed=False)
        tr.train()
        if graphed:
            state = [p.detach().clone() for p in tr.G.parameters()]
            tr.capture(reals, *zs[0], warmup=1)
            # capture ran warm-up iterations: restore the initial weights / optimiser moments
            with torch.no_grad():
                for p, q in zip(tr.G.parameters(), state):
                    p.copy_(q)
        outs = []
        for z1, z2 in zs:
            o = (tr.step_graphed if graphed else tr.step)(reals, z1, z2)
            outs.append({k: v.item() for k, v in o.items()})
        res.append(outs)
    # the first replayed iteration sees the same G weights as the eager one (D and Adam states
    # differ after the capture warm-up, so only generator-side forward quantities are compared)
    assert all(np.isfinite(list(o.values())).all() for o in res[1])
    np.testing.assert_allclose(res[1][0]["similar_loss"], res[0][0]["similar_loss"], rtol=2e-2)


@pytest.mark.parametrize("B,N,k,specs", [(2, 50, 10, ((6, 5, 8, 0, 48),)),                       # ldy = 56, one spec tiles it
                                         (3, 300, 10, ((6, 5, 16, 0, 96), (10, 1, 8, 112, 192), (1, 10, 4, 200, 204))),
                                         (2, 1024, 10, ((6, 5, 128, 0, 768), (10, 1, 64, 896, 1536))),
                                         (3, 1000, 10, ((6, 5, 160, 0, 960), (10, 1, 72, 1120, 1840)))])
def test_window_gather_sum_backward_csr_path(B, N, k, specs):
    """Specs that tile dY completely take the atomic-free transposed-graph adjoint."""
    from pdgn_amd.deconv import EdgeGatherSum
    ldy = sum(T * C + (C if offc >= 0 else 0) for (T, P, C, off, offc) in specs)
    rng = np.random.default_rng(N + ldy)
    Y = torch.from_numpy(rng.standard_normal((B, N, ldy)).astype(np.float32))
    idx = torch.from_numpy(rng.integers(0, N, (B, N, k)).astype(np.int32))
    idx[:, :, 0] = 3                                          # a hub with in-degree N
    biases = [torch.from_numpy(rng.standard_normal(C).astype(np.float32)) for (T, P, C, off, offc) in specs]
    Yg = dev(Y).requires_grad_(True)
    bg = [dev(b_).requires_grad_(True) for b_ in biases]
    outs = EdgeGatherSum.apply(Yg, dev(idx), specs, *bg)
    Yc = Y.double().requires_grad_(True)
    bc = [b_.double().requires_grad_(True) for b_ in biases]
    refs = EdgeGatherSumTorch.apply(Yc, idx, specs, *bc)
    gouts = [torch.from_numpy(rng.standard_normal(tuple(r.shape)).astype(np.float32)) for r in refs]
    torch.autograd.backward(outs, [dev(g_) for g_ in gouts])
    torch.autograd.backward(refs, [g_.double() for g_ in gouts])
    for o, r in zip(outs, refs):
        np.testing.assert_allclose(o.detach().cpu().numpy(), r.detach().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(Yg.grad.cpu().numpy(), Yc.grad.numpy(), rtol=1e-4, atol=1e-4)
    for a_, b_ in zip(bg, bc):
        np.testing.assert_allclose(a_.grad.cpu().numpy(), b_.grad.numpy(), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("M,N,K", [(35840, 12832, 256), (35840, 12832, 128), (71680, 1024, 256), (358400, 512, 64),
                                   (35840, 512, 5120), (17920, 256, 2560), (5000, 20, 12), (1024, 4, 4), (100003, 132, 68),
                                   (71680, 64, 16), (358400, 64, 16), (71680, 64, 4)])
def test_gemm_tn_direct(M, N, K):
    """pdgn_gemm_tn called through the C ABI itself (no dispatch in between) on every large weight-gradient shape
    of the step: dW = dY^T X within 1e-5 of an fp64 reference, measured against sum |dy||x| as for any fp32 accumulation."""
    import ctypes
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x = torch.randn(M, K, device="cuda", generator=g)
    dy = torch.randn(M, N, device="cuda", generator=g)
    dw = torch.zeros(N, K, device="cuda")
    assert _lib.lib().pdgn_gemm_tn(ctypes.c_longlong(M), N, K, ptr(dy), ptr(x), ptr(dw), stream_of(dy)) == 0
    rows = min(M, 40000)                                        # fp64 on a row sample (exact), fp32 matmul on all rows
    scale = (dy.abs().t().matmul(x.abs())).clamp_min(1e-6)
    assert ((dw - dy.t().matmul(x)).abs() / scale).max().item() < 2e-5
    dw2 = torch.zeros(N, K, device="cuda")
    assert _lib.lib().pdgn_gemm_tn(ctypes.c_longlong(rows), N, K, ptr(dy), ptr(x), ptr(dw2), stream_of(dy)) == 0
    ref64 = dy[:rows].double().t().matmul(x[:rows].double())
    scale64 = dy[:rows].abs().double().t().matmul(x[:rows].abs().double()).clamp_min(1e-6)
    assert ((dw2.double() - ref64).abs() / scale64).max().item() < 1e-5


@pytest.mark.parametrize("cfg", [None, 0, 1, 3])
@pytest.mark.parametrize("gemm", ["x2", "x3", "fp32", "x3_16"])
@pytest.mark.parametrize("M,N,K", [(35840, 12832, 128), (71680, 1024, 256), (358400, 512, 64), (35840, 512, 5120),
                                   (17920, 256, 2560), (100003, 132, 68), (5000, 64, 128), (40, 128, 64), (8960, 3232, 32)])
def test_gemm_tn_big_direct(M, N, K, cfg, monkeypatch, gemm):
    """pdgn_gemm_tn_big through the C ABI (weight gradient on the pdgn_gemm_nt kernel with both operands transposed and
    the row reduction split stream-K): dW = dY^T X against fp32 matmul on all rows and fp64 on a row sample, every
    configuration the entry point can pick; dW needs no zero-fill by the caller (poisoned with NaN here)."""
    import ctypes
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    from pdgn_amd import _lib as _sw
    _sw.set_gemm_config(cfg)                                   # forced tile configuration | None: the launch model's pick
    _sw.set_gemm_mode(gemm)                                    # csrc/gemm_x3.hip (the default) | csrc/gemm_nt.hip; conftest resets both
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x = torch.randn(M, K, device="cuda", generator=g)
    dy = torch.randn(M, N, device="cuda", generator=g)
    dw = torch.full((N, K), float("nan"), device="cuda")
    assert _lib.lib().pdgn_gemm_tn_big(ctypes.c_longlong(M), N, K, ptr(dy), N, ptr(x), K, ptr(dw), 0, stream_of(dy)) == 0
    scale = (dy.abs().t().matmul(x.abs())).clamp_min(1e-6)
    assert ((dw - dy.t().matmul(x)).abs() / scale).max().item() < 2e-5
    rows = min(M, 40000)
    dw2 = torch.full((N, K), float("nan"), device="cuda")
    assert _lib.lib().pdgn_gemm_tn_big(ctypes.c_longlong(rows), N, K, ptr(dy), N, ptr(x), K, ptr(dw2), 0, stream_of(dy)) == 0
    ref64 = dy[:rows].double().t().matmul(x[:rows].double())
    scale64 = dy[:rows].abs().double().t().matmul(x[:rows].abs().double()).clamp_min(1e-6)
    assert ((dw2.double() - ref64).abs() / scale64).max().item() < 1e-5


@pytest.mark.parametrize("M,N,K", [(35840, 512, 256), (5000, 20, 12), (1024, 3, 64), (100003, 132, 68), (71680, 64, 3),
                                   (2048, 6, 3), (300, 64, 64)])
def test_linear_cl_autograd(M, N, K):
    """LinearCL end to end (forward, input / weight / bias / addend gradients), including the channel counts that are
    zero-padded for the kernels (k = 3: xyz layers, n = 3: the heads' last conv) and the sub-threshold torch path."""
    from pdgn_amd.fused import linear_cl
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g)
    b = torch.randn(N, device="cuda", generator=g)
    add = torch.randn(M, N, device="cuda", generator=g)
    dy = torch.randn(M, N, device="cuda", generator=g)
    res = []
    for fn, cast in ((linear_cl, lambda t: t), (lambda x_, w_, b_, a_: torch.nn.functional.linear(x_, w_, b_) + a_, lambda t: t.double())):
        leaves = [cast(t).clone().requires_grad_(True) for t in (x, w, b, add)]
        y = fn(*leaves)
        y.backward(cast(dy))
        res.append([y.detach()] + [l.grad for l in leaves])
    sc = float(M) ** 0.5
    for name, got, ref, atol in zip(("y", "dx", "dw", "db", "dadd"), res[0], res[1], (1e-4 * K, 1e-4 * N, 2e-4 * sc, 2e-4 * sc, 0.0)):
        np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=atol + 1e-6, err_msg=name)


@pytest.mark.parametrize("M,N,K", [(71680, 64, 3), (1024, 3, 64), (2049, 32, 3), (5001, 3, 32), (1500, 4, 64), (1030, 64, 4),
                                   (1024, 128, 1), (3000, 2, 256), (1100, 48, 3)])
@pytest.mark.parametrize("bias", [True, False])
def test_thin_layers(M, N, K, bias):
    """The xyz-in / xyz-out layers (<= 4 channels on one side) on pdgn_thin_nt / pdgn_thin_tn: forward, the BatchNorm partials
    of the k <= 4 form, input / weight / bias gradients against fp64."""
    from pdgn_amd import fused
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g)
    b = torch.randn(N, device="cuda", generator=g) if bias else None
    dy = torch.randn(M, N, device="cuda", generator=g)
    fused.GEMM_LOG = []
    try:
        leaves = [t.clone().requires_grad_(True) for t in (x, w)] + ([b.clone().requires_grad_(True)] if bias else [None])
        y, part = fused.linear_cl(leaves[0], leaves[1], leaves[2], None, True)
        y.backward(dy)
        kinds = [e[0] for e in fused.GEMM_LOG]
    finally:
        fused.GEMM_LOG = None
    assert kinds == ["thin", "thin", "thin_tn"], kinds                       # no padded launch on the MFMA kernels
    ref = [t.double().clone().requires_grad_(True) for t in (x, w)] + ([b.double().clone().requires_grad_(True)] if bias else [None])
    yr = torch.nn.functional.linear(*ref)
    yr.backward(dy.double())
    sc = float(M) ** 0.5
    for name, got, want, atol in (("y", y.detach(), yr.detach(), 1e-4 * K), ("dx", leaves[0].grad, ref[0].grad, 1e-4 * N),
                                  ("dw", leaves[1].grad, ref[1].grad, 2e-4 * sc)) + \
            ((("db", leaves[2].grad, ref[2].grad, 2e-4 * sc),) if bias else ()):
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=atol + 1e-6, err_msg=name)
    if K <= 4:
        part, block = part                                                   # (partials, rows per block) as linear_cl hands them on
        assert part is not None and part.shape[1] == 3 * N and block == 256
        tot = _raw_sums(part, M, 256, N)
        np.testing.assert_allclose(tot[:N], yr.detach().sum(0).cpu().numpy(), rtol=1e-4, atol=1e-3 * sc)
        np.testing.assert_allclose(tot[N:], (yr.detach() ** 2).sum(0).cpu().numpy(), rtol=1e-4, atol=1e-3 * sc)
    else:
        assert part is None


@pytest.mark.parametrize("M,k,C", [(1000, 10, 16), (3584, 10, 512), (77, 4, 24), (500, 32, 3)])
def test_softmax_slots_permute(M, k, C):
    from pdgn_amd.fused import softmax_slots_permute
    from torch_standins import softmax_slots_permute_torch
    rng = np.random.default_rng(M + C)
    h = torch.from_numpy((rng.standard_normal((M, k, C)) * 3).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((M, k // 2, 2 * C)).astype(np.float32))
    hd = dev(h).requires_grad_(True)
    w = softmax_slots_permute(hd)
    w.backward(dev(g))
    hr = h.double().requires_grad_(True)
    wr = softmax_slots_permute_torch(hr)
    wr.backward(g.double())
    np.testing.assert_allclose(w.detach().cpu().numpy(), wr.detach().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(hd.grad.cpu().numpy(), hr.grad.numpy(), rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("M,k,C,training", [(1000, 10, 16, True), (1792, 10, 512, True), (77, 4, 24, True), (300, 10, 64, False)])
def test_bn_softmax_slots_permute(M, k, C, training):
    """conv_all.4 + LeakyReLU + slot softmax + interleave in one pass vs BatchNorm -> act -> softmax in fp64."""
    import torch.nn as nn
    from pdgn_amd.fused import bn_softmax_slots_permute
    from torch_standins import bn_softmax_slots_permute_torch
    rng = np.random.default_rng(M + C)
    x = torch.from_numpy((rng.standard_normal((M * k, C)) * 2 + 0.5).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((M, k // 2, 2 * C)).astype(np.float32))
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)))
        bn.bias.copy_(torch.from_numpy(rng.uniform(-0.5, 0.5, C).astype(np.float32)))
        bn.running_mean.copy_(torch.from_numpy(rng.uniform(-0.2, 0.8, C).astype(np.float32)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(2.0, 5.0, C).astype(np.float32)))
    import copy
    bnr = copy.deepcopy(bn).double()
    bnd = bn.cuda()
    xd = dev(x).requires_grad_(True)
    w = bn_softmax_slots_permute(xd, bnd, training, k)
    w.backward(dev(g))
    xr = x.double().requires_grad_(True)
    wr = bn_softmax_slots_permute_torch(xr, bnr, training, k)
    wr.backward(g.double())
    np.testing.assert_allclose(w.detach().cpu().numpy(), wr.detach().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(xd.grad.cpu().numpy(), xr.grad.numpy(), rtol=2e-3, atol=2e-6)
    np.testing.assert_allclose(bnd.weight.grad.cpu().numpy(), bnr.weight.grad.numpy(), rtol=2e-3, atol=1e-4)
    np.testing.assert_allclose(bnd.bias.grad.cpu().numpy(), bnr.bias.grad.numpy(), rtol=2e-3, atol=1e-4)
    if training:
        np.testing.assert_allclose(bnd.running_mean.cpu().numpy(), bnr.running_mean.numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(bnd.running_var.cpu().numpy(), bnr.running_var.numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("M,k,C,training", [(640, 10, 16, True), (896, 10, 256, True), (33, 4, 24, True), (200, 10, 64, False), (150, 16, 32, True), (120, 20, 32, True),
                                            (96, 6, 32, True)])
def test_bilateral_weighting(M, k, C, training):
    """both BatchNorms + activations + slot softmax + interleave + product in one pass vs the same chain in fp64.  k = 4, 10:
    the fused adjoint, which recomputes the softmax weights from x (they are never written); k = 6: the generic chain of
    separate adjoint kernels over the saved weights."""
    import copy
    import torch.nn as nn
    from pdgn_amd.fused import bilateral_weighting
    from torch_standins import bilateral_weighting_torch
    rng = np.random.default_rng(M + C)
    x = torch.from_numpy((rng.standard_normal((M * k, C)) * 2 + 0.5).astype(np.float32))
    u = torch.from_numpy((rng.standard_normal((M * k // 2, 2 * C)) * 1.5 - 0.2).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((M * k // 2, 2 * C)).astype(np.float32))
    pb = torch.from_numpy(rng.standard_normal(C).astype(np.float32))
    bns = []
    for ch in (C, 2 * C):
        bn = nn.BatchNorm2d(ch)
        with torch.no_grad():
            bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, ch).astype(np.float32)))
            bn.bias.copy_(torch.from_numpy(rng.uniform(-0.5, 0.5, ch).astype(np.float32)))
            bn.running_mean.copy_(torch.from_numpy(rng.uniform(-0.2, 0.8, ch).astype(np.float32)))
            bn.running_var.copy_(torch.from_numpy(rng.uniform(2.0, 5.0, ch).astype(np.float32)))
        bns.append(bn)
    ref_bns = [copy.deepcopy(b).double() for b in bns]
    dev_bns = [b.cuda() for b in bns]
    xd, ud = dev(x).requires_grad_(True), dev(u).requires_grad_(True)
    y = bilateral_weighting(xd, dev_bns[0], ud, dev_bns[1], training, k, pre_bias_x=dev(pb) if training else None)
    y.backward(dev(g))
    xr, ur = x.double().requires_grad_(True), u.double().requires_grad_(True)
    yr = bilateral_weighting_torch(xr, ref_bns[0], ur, ref_bns[1], training, k, pre_bias_x=pb.double() if training else None)
    yr.backward(g.double())
    np.testing.assert_allclose(y.detach().cpu().numpy(), yr.detach().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(xd.grad.cpu().numpy(), xr.grad.numpy(), rtol=2e-3, atol=2e-6)
    np.testing.assert_allclose(ud.grad.cpu().numpy(), ur.grad.numpy(), rtol=2e-3, atol=2e-6)
    for a, b in zip(dev_bns, ref_bns):
        np.testing.assert_allclose(a.weight.grad.cpu().numpy(), b.weight.grad.numpy(), rtol=2e-3, atol=1e-4)
        np.testing.assert_allclose(a.bias.grad.cpu().numpy(), b.bias.grad.numpy(), rtol=2e-3, atol=1e-4)
        if training:
            np.testing.assert_allclose(a.running_mean.cpu().numpy(), b.running_mean.numpy(), rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(a.running_var.cpu().numpy(), b.running_var.numpy(), rtol=1e-5, atol=1e-6)
    with torch.no_grad():                                       # no-grad path: w is not written, same y
        y2 = bilateral_weighting(dev(x), copy.deepcopy(dev_bns[0]), dev(u), copy.deepcopy(dev_bns[1]), False, k)
        yr2 = bilateral_weighting_torch(x.double(), ref_bns[0], u.double(), ref_bns[1], False, k)
    np.testing.assert_allclose(y2.cpu().numpy(), yr2.numpy(), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("b,n,k,T,P,C", [(3, 64, 10, 6, 5, 64), (2, 128, 10, 6, 5, 1024), (2, 50, 4, 3, 2, 8), (3, 1000, 10, 6, 5, 160),
                                         (5, 700, 8, 4, 5, 96)])
def test_window_gather_sum_with_statistics_epilogue(b, n, k, T, P, C):
    """pdgn_window_gather_sum_stats: the same output bit for bit, and BatchNorm statistics (incl. running buffers)
    finished from its partials equal to a statistics pass over the output"""
    import ctypes
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    L = _lib.lib()
    L.pdgn_bn_scratch_floats.restype = ctypes.c_longlong
    rng = np.random.default_rng(b * n + C)
    ldy = T * C + C
    Y = dev(rng.standard_normal((b, n, ldy)).astype(np.float32))
    idx = dev(rng.integers(0, n, (b, n, k)).astype(np.int32))
    bias = dev(rng.standard_normal((b, C)).astype(np.float32))
    out0 = torch.empty((b, n, P, C), device="cuda")
    out1 = torch.empty_like(out0)
    assert L.pdgn_window_gather_sum(b, n, k, ldy, T, P, C, C, 0, ptr(Y), ptr(idx), ptr(bias), C, ptr(out0), stream_of(Y)) == 0
    rows = b * n * P
    scr = torch.empty(L.pdgn_bn_scratch_floats(ctypes.c_longlong(rows), C), device="cuda")
    assert L.pdgn_window_gather_sum_stats(b, n, k, ldy, T, P, C, C, 0, ptr(Y), ptr(idx), ptr(bias), C, ptr(out1), ptr(scr),
                                          stream_of(Y)) == 0
    assert torch.equal(out0, out1)
    g = dev(rng.uniform(0.5, 1.5, C).astype(np.float32)); be = dev(rng.uniform(-0.5, 0.5, C).astype(np.float32))
    res = []
    for mode in (0, 1):
        rm = torch.zeros(C, device="cuda"); rv = torch.ones(C, device="cuda"); stats = torch.empty(4 * C, device="cuda")
        if mode == 0:
            scr2 = torch.empty_like(scr)
            assert L.pdgn_bn_stats(ctypes.c_longlong(rows), C, ctypes.c_float(1e-5), ctypes.c_float(0.1), ptr(out0), ptr(g), ptr(be),
                                   None, ptr(rm), ptr(rv), ptr(scr2), ptr(stats), stream_of(Y)) == 0
        else:
            assert L.pdgn_bn_stats_from_partials(ctypes.c_longlong(rows), C, ctypes.c_float(1e-5), ctypes.c_float(0.1), ptr(g),
                                                 ptr(be), None, ptr(rm), ptr(rv), ptr(scr), ptr(stats), stream_of(Y)) == 0
        res.append((stats, rm, rv))
    for a, c in zip(res[0], res[1]):
        torch.testing.assert_close(a, c, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("F_,Fo,k,bilateral,Fc", [(8, 8, 4, False, 0), (16, 8, 10, True, 0), (16, 24, 10, True, 8), (64, 64, 10, True, 32),
                                                   (32, 16, 4, False, 16)])
def test_assemble_weights_kernel_vs_torch(F_, Fo, k, bilateral, Fc):
    """the one-launch weight re-association (and its adjoint) against PointDeconv._assemble's torch ops"""
    from pdgn_amd.deconv import AssembleWeights, PointDeconv
    torch.manual_seed(F_ + k)
    m = PointDeconv(F_, Fo, k, bilateral=bilateral).cuda()
    Wcat, Wb, T, P = m._assemble()
    gcat = torch.randn_like(Wcat)
    gb = torch.randn_like(Wb)
    params = [m.inte_conv_hk[0].weight, m.conv2.conv.weight] + ([m.conv_fea[0].weight] if bilateral else [])
    want = torch.autograd.grad([Wcat, Wb], params, [gcat, gb])
    C, V, B2 = AssembleWeights.apply(m.inte_conv_hk[0].weight, m.conv2.conv.weight, m.conv_fea[0].weight if bilateral else None,
                                     F_, Fo, k, T, Fc)
    got_cat = V if Fc == 0 else torch.cat([C, V], 1)
    assert (C is None) == (Fc == 0)
    torch.testing.assert_close(got_cat, Wcat, rtol=1e-6, atol=1e-6)
    assert torch.equal(B2, Wb)
    outs = [V, B2] if Fc == 0 else [C, V, B2]
    gouts = [gcat, gb] if Fc == 0 else [gcat[:, :Fc].contiguous(), gcat[:, Fc:].contiguous(), gb]
    got = torch.autograd.grad(outs, params, gouts)
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-6)
    if Fc:                                                       # a missing upstream gradient counts as zero
        got2 = torch.autograd.grad([V, B2], params, [gcat[:, Fc:].contiguous(), gb], allow_unused=True)
        gz = gcat.clone(); gz[:, :Fc] = 0
        want2 = torch.autograd.grad(m._assemble()[:2], params, [gz, gb])
        for a, b in zip(got2, want2):
            torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-6)


def test_config_c4_reference_blocks_fixture(golden):
    """BASELINE.json configs[3] against the reference's OWN block classes (Note C4):
    tests/golden/generator_c4_b4.npz was computed by a reference PointGenerator whose fc1 / bilateral1..4 were swapped
    for base-256 instances of the reference classes (tests/golden/gen_golden.py::gen_c4).  The HIP generator with
    base_points=256, the same hashed weights and the graphs the reference picked reproduces its four clouds
    (512 ... 4096 points) and D4's score to 1e-4."""
    from pdgn_amd.generator import PointDiscriminator, PointGenerator
    g = golden("generator_c4_b4.npz")
    G = fill_module(PointGenerator(base_points=256), salt=21).cuda().train()
    with torch.no_grad():
        outs = G(dev(g["z"]), idx=[dev(g["idx%d" % i].astype(np.int32)) for i in (1, 2, 3, 4)])
    assert [o.shape[2] for o in outs] == [512, 1024, 2048, 4096]
    for i, o in enumerate(outs):
        gold = g["p%d" % (i + 1)]
        np.testing.assert_allclose(o.cpu().numpy(), gold, rtol=1e-4, atol=1e-4 * np.abs(gold).max(), err_msg="p%d" % (i + 1))
    D4 = fill_module(PointDiscriminator(4, 4096), salt=13).cuda().train()
    with torch.no_grad():
        np.testing.assert_allclose(D4(dev(g["p4"])).cpu().numpy(), g["d4"], rtol=1e-4, atol=1e-5)


def test_config_c4_full_batch_properties():
    """C4 at its full size (B=35, 512 -> 4096 points): one iteration runs, every loss and every updated generator
    parameter is finite, the clouds have the four resolutions, and the 4096-point kNN rows are duplicate-free."""
    from pdgn_amd.deconv import feature_knn
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    torch.manual_seed(9999)
    B, res = 35, (512, 1024, 2048, 4096)
    tr = PDGNTrainer(device="cuda", base_points=256, distributed=False)
    tr.train()
    losses = tr.step(synthetic_batch(B, "cuda", n_points=4096, resolutions=res), noise(B, "cuda"), noise(B, "cuda"))
    assert all(torch.isfinite(v).item() for v in losses.values())
    assert all(torch.isfinite(p).all().item() for p in tr.G.parameters())
    with torch.no_grad():
        clouds = tr.G(noise(B, "cuda"))
    assert [c.shape for c in clouds] == [(B, 3, n) for n in res]
    x = torch.nn.functional.leaky_relu(torch.randn(4, 256, 2048, device="cuda"))
    idx = feature_knn(x, 10).long()
    srt = idx.sort(dim=2)[0]
    assert (srt[:, :, 1:] != srt[:, :, :-1]).all()
    del tr
    torch.cuda.empty_cache()


def test_config_c4_four_stage_512_to_4096():
    """BASELINE.json configs[3] ("4-stage 256->4096"; SURVEY.md section 8 Note C4: base 256 points):
    the size-generic blocks run one iteration at 512/1024/2048/4096 points; outputs have the right
    shapes, losses are finite, and the generator matches the oracle restatement composed from the
    same blocks on the oracle's kNN graphs."""
    from pdgn_amd.generator import PointGenerator
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    B = 3
    G = fill_module(PointGenerator(base_points=256), salt=21).cuda().train()
    R = fill_module(pdgnet_ref.PointGeneratorRef(base_points=256), salt=21).train()
    z = hash_tensor("c4_z", (B, 128), 0.2)
    idxs = []

    def grab(mod, inp):
        idxs.append(pdgnet_ref.feature_knn(inp[0], mod.k)[0])
    hooks = [m.register_forward_pre_hook(grab) for m in
             (R.bilateral1.upsample_cov[0], R.bilateral2.upsample_cov, R.bilateral3.upsample_cov, R.bilateral4.upsample_cov)]
    with torch.no_grad():
        ref = R(z)
        out = G(dev(z), idx=[dev(i.to(torch.int32)) for i in idxs])
    for h in hooks:
        h.remove()
    assert [o.shape[2] for o in out] == [512, 1024, 2048, 4096]
    for o, r in zip(out, ref):
        np.testing.assert_allclose(o.cpu().numpy(), r.numpy(), rtol=1e-3, atol=2e-3 * float(r.abs().max()))
    torch.manual_seed(1)
    tr = PDGNTrainer(device="cuda", base_points=256, distributed=False)
    tr.train()
    res = (512, 1024, 2048, 4096)
    losses = tr.step(synthetic_batch(B, "cuda", n_points=4096, resolutions=res), noise(B, "cuda"), noise(B, "cuda"))
    assert all(torch.isfinite(v).item() for v in losses.values())


@pytest.mark.parametrize("cfg", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("gemm", ["x2", "x3", "fp32", "x3_16"])
@pytest.mark.parametrize("M,N,K", [(35840, 512, 128), (5000, 132, 36), (129, 8, 4), (71680, 1024, 256), (35840, 512, 5120),
                                   (17920, 64, 6432), (8960, 3232, 32), (1000, 36, 20), (358400, 64, 16)])
def test_gemm_nt_with_epilogues(M, N, K, cfg, monkeypatch, gemm):
    """pdgn_gemm_nt through the C ABI, every tile configuration (_lib.set_gemm_config) and the launch model's own pick:
    C = A W^T (plain: the stream-K tail may run), and C = A W^T + bias + addend with the column-statistics partials."""
    import ctypes
    import os
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    from pdgn_amd import _lib as _sw
    _sw.set_gemm_config(cfg)                                   # forced tile configuration | None: the launch model's pick
    _sw.set_gemm_mode(gemm)                                    # csrc/gemm_x3.hip (the default) | csrc/gemm_nt.hip; conftest resets both
    L = _lib.lib()
    L.pdgn_gemm_nt_stat_rows.restype = ctypes.c_longlong
    g = torch.Generator(device="cuda").manual_seed(M + N)
    A = torch.randn(M, K, device="cuda", generator=g)
    W = torch.randn(N, K, device="cuda", generator=g)
    bias = torch.randn(N, device="cuda", generator=g)
    add = torch.randn(M, N, device="cuda", generator=g)
    rows = min(M, 30000)                                        # fp64 reference on a row sample, fp32 matmul on all rows
    scale = (A.abs() @ W.abs().t()) + 1
    C = torch.full((M, N), float("nan"), device="cuda")
    assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(A), K, ptr(W), K, None, None, 0, ptr(C), N, None, stream_of(A)) == 0
    assert ((C - A @ W.t()).abs() / scale).max().item() < 2e-5
    ref = A[:rows].double() @ W.double().t()
    assert ((C[:rows].double() - ref).abs() / scale[:rows].double()).max().item() < 1e-5
    nparts = L.pdgn_gemm_nt_stat_rows(ctypes.c_longlong(M), N, K)
    part = torch.full((nparts, 3 * N), float("nan"), device="cuda")
    C2 = torch.full((M, N), float("nan"), device="cuda")
    assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(A), K, ptr(W), K, ptr(bias), ptr(add), N, ptr(C2), N, ptr(part),
                          stream_of(A)) == 0
    ref2 = (A @ W.t() + bias + add)
    assert ((C2 - ref2).abs() / scale).max().item() < 2e-5
    c64 = C2.double()
    tot = _raw_sums(part, M, L.pdgn_gemm_nt_stat_block_rows(ctypes.c_longlong(M), N, K), N)
    np.testing.assert_allclose(tot[:N], c64.sum(0).cpu().numpy(), rtol=1e-4, atol=1e-4 * float(c64.abs().sum(0).max()))
    np.testing.assert_allclose(tot[N:], (c64 * c64).sum(0).cpu().numpy(), rtol=1e-4)


@pytest.mark.parametrize("cfg", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("gemm", ["x2", "x3", "fp32", "x3_16"])
@pytest.mark.parametrize("M,N,K", [(35840, 128, 512), (5000, 132, 36), (129, 8, 4), (17920, 2560, 256), (35840, 5120, 512),
                                   (17920, 64, 6432), (1000, 36, 20), (71680, 256, 1024)])
def test_gemm_nn_input_gradient_form(M, N, K, cfg, monkeypatch, gemm):
    """pdgn_gemm_nn through the C ABI: C = A (M x K) Wt (K x N), the second operand row-major as the layer's own
    (C_out x C_in) weight -- every tile configuration and the launch model's pick; plain and with bias + addend + statistics."""
    import ctypes
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    from pdgn_amd import _lib as _sw
    _sw.set_gemm_config(cfg)                                   # forced tile configuration | None: the launch model's pick
    _sw.set_gemm_mode(gemm)                                    # csrc/gemm_x3.hip (the default) | csrc/gemm_nt.hip; conftest resets both
    L = _lib.lib()
    L.pdgn_gemm_nt_stat_rows.restype = ctypes.c_longlong
    g = torch.Generator(device="cuda").manual_seed(M + N + 1)
    A = torch.randn(M, K, device="cuda", generator=g)
    Wt = torch.randn(K, N, device="cuda", generator=g)
    bias = torch.randn(N, device="cuda", generator=g)
    add = torch.randn(M, N, device="cuda", generator=g)
    scale = (A.abs() @ Wt.abs()) + 1
    C = torch.full((M, N), float("nan"), device="cuda")
    assert L.pdgn_gemm_nn(ctypes.c_longlong(M), N, K, ptr(A), K, ptr(Wt), N, None, None, 0, ptr(C), N, None, stream_of(A)) == 0
    assert ((C - A @ Wt).abs() / scale).max().item() < 2e-5
    rows = min(M, 30000)
    ref = A[:rows].double() @ Wt.double()
    assert ((C[:rows].double() - ref).abs() / scale[:rows].double()).max().item() < 1e-5
    nparts = L.pdgn_gemm_nt_stat_rows(ctypes.c_longlong(M), N, K)
    part = torch.full((nparts, 3 * N), float("nan"), device="cuda")
    C2 = torch.full((M, N), float("nan"), device="cuda")
    assert L.pdgn_gemm_nn(ctypes.c_longlong(M), N, K, ptr(A), K, ptr(Wt), N, ptr(bias), ptr(add), N, ptr(C2), N, ptr(part),
                          stream_of(A)) == 0
    assert ((C2 - (A @ Wt + bias + add)).abs() / scale).max().item() < 2e-5
    c64 = C2.double()
    tot = _raw_sums(part, M, L.pdgn_gemm_nt_stat_block_rows(ctypes.c_longlong(M), N, K), N)
    np.testing.assert_allclose(tot[:N], c64.sum(0).cpu().numpy(), rtol=1e-4, atol=1e-4 * float(c64.abs().sum(0).max()))


@pytest.mark.parametrize("shape", ["x3_32", "x3_16"])
@pytest.mark.parametrize("M,N,K", [(9000, 512, 1280), (4100, 132, 260), (20000, 64, 64), (2500, 12832, 128), (3000, 256, 8)])
def test_gemm_presplit_second_operand(M, N, K, shape):
    """pdgn_split_bf16x3 + pdgn_gemm_nt_ps (csrc/split.hip, the PW instances of gemm_x3_kernel): the weight split ONCE into its three
    bf16 parts instead of by every workgroup's loader.  The planes hold exactly the loader's parts, so (i) they reassemble to the
    fp32 weight up to 2^-24, (ii) the product equals the unsplit entry point's -- bit for bit when no stream-K tail (float
    atomics) is involved, to rounding otherwise -- with bias, addend and statistics partials, (iii) the planes of the TRANSPOSE
    give the input gradient dX = dY W of pdgn_gemm_nn, and all of it against fp64."""
    import ctypes
    from pdgn_amd import _lib, fused
    from pdgn_amd._lib import ptr, stream_of
    L = _lib.lib()
    _lib.set_gemm_mode(shape)                                  # either bf16 matrix instruction: bit-identity holds WITHIN a shape
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * 0.3
    bias = torch.randn(N, device="cuda", generator=g)
    add = torch.randn(M, N, device="cuda", generator=g)
    pl = fused.split_planes(w, True)
    assert pl is not None and pl.p.shape[:2] == (3, N) and pl.t.shape[:2] == (3, K)
    parts = (pl.p[:, :, :K].to(torch.int32) << 16).view(torch.float32)          # bf16 bit patterns -> fp32
    assert (parts.double().sum(0) - w.double()).abs().max().item() <= 2.0 ** -23 * w.abs().max().item()
    assert torch.equal(pl.t[:, :, :N], pl.p[:, :, :K].transpose(1, 2))
    ref = a.double() @ w.double().t() + bias.double() + add.double()
    mag = a.double().abs() @ w.double().abs().t() + 1.0
    c0, c1 = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    L.pdgn_gemm_nt_stat_rows.restype = ctypes.c_longlong
    nrows = L.pdgn_gemm_nt_stat_rows(ctypes.c_longlong(M), N, K)
    p0, p1 = torch.zeros(nrows, 3 * N, device="cuda"), torch.zeros(nrows, 3 * N, device="cuda")
    wp = ctypes.c_longlong(N * pl.p.shape[2])
    assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(w), K, ptr(bias), ptr(add), N, ptr(c0), N, ptr(p0), stream_of(a)) == 0
    assert L.pdgn_gemm_nt_ps(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(pl.p), pl.p.shape[2], wp, 3, ptr(bias), ptr(add), N, ptr(c1), N, ptr(p1),
                             None, 0, 1, 0, None, 0, stream_of(a)) == 0
    assert torch.equal(c0, c1) and torch.equal(p0, p1)          # launches with statistics have no stream-K tail: identical
    assert ((c1.double() - ref).abs() / mag).max().item() < 1e-6
    # plain launch (may carry a stream-K tail with float atomics): equal to rounding
    assert L.pdgn_gemm_nt_ps(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(pl.p), pl.p.shape[2], wp, 3, None, None, 0, ptr(c1), N, None, None, 0, 1, 0,
                             None, 0, stream_of(a)) == 0
    assert ((c1.double() - a.double() @ w.double().t()).abs() / mag).max().item() < 1e-6
    # input gradient through the planes of W^T against pdgn_gemm_nn
    dy = torch.randn(M, N, device="cuda", generator=g)
    d0, d1 = torch.empty(M, K, device="cuda"), torch.empty(M, K, device="cuda")
    assert L.pdgn_gemm_nn(ctypes.c_longlong(M), K, N, ptr(dy), N, ptr(w), K, None, None, 0, ptr(d0), K, None, stream_of(a)) == 0
    assert L.pdgn_gemm_nt_ps(ctypes.c_longlong(M), K, N, ptr(dy), N, ptr(pl.t), pl.t.shape[2], ctypes.c_longlong(K * pl.t.shape[2]), 3, None, None, 0,
                             ptr(d1), K, None, None, 0, 1, 0, None, 0, stream_of(a)) == 0
    refd = dy.double() @ w.double()
    magd = dy.double().abs() @ w.double().abs() + 1.0
    assert ((d1.double() - refd).abs() / magd).max().item() < 1e-6 and ((d0 - d1).abs().double() / magd).max().item() < 1e-6
    # refused where it cannot be what it says: the fp32-instruction mode
    _lib.set_gemm_mode("fp32")
    assert L.pdgn_gemm_nt_ps(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(pl.p), pl.p.shape[2], wp, 3, None, None, 0, ptr(c1), N, None, None, 0, 1, 0,
                             None, 0, stream_of(a)) == -1
    _lib.set_gemm_mode("x3")


@pytest.mark.parametrize("R,N,K,pitch", [(35, 12832, 128, 0), (35, 256, 512, 768), (35, 3232, 32, 0), (64, 1600, 64, 0), (1, 20, 8, 0),
                                         (35, 4096, 128, 0), (48, 132, 1024, 0), (35, 8192, 32, 0)])
def test_skinny_products(R, N, K, pitch):
    """csrc/skinny.hip: the three products of a per-sample operand (R <= 64 rows) with a large matrix -- y = x W^T (+ b), dx = dy W,
    dW = dy^T x -- against fp64, with a column slice of a wider weight (row pitch) as the large operand and as the gradient's target."""
    from pdgn_amd import fused
    g = torch.Generator(device="cuda").manual_seed(R + N + K)
    ld = pitch or K
    Wfull = torch.randn(N, ld, device="cuda", generator=g) * 0.2
    W = Wfull[:, :K]
    x = torch.randn(R, K, device="cuda", generator=g)
    b = torch.randn(N, device="cuda", generator=g)
    dy = torch.randn(R, N, device="cuda", generator=g)
    y = fused.skinny_nt(x, W, b)
    ref = x.double() @ W.double().t() + b.double()
    assert (y.double() - ref).abs().max().item() < 1e-5 * (x.abs().double() @ W.abs().double().t()).max().item()
    if N % 4 == 0:
        import ctypes
        from pdgn_amd import _lib
        from pdgn_amd._lib import ptr, stream_of
        dx = torch.zeros(R, K, device="cuda")                            # straight through the C ABI: every reduction length
        assert _lib.lib().pdgn_skinny_nn(R, K, N, ptr(dy), N, ptr(W), W.stride(0), ptr(dx), K, stream_of(dy)) == 0
        refx = dy.double() @ W.double()
        assert (dx.double() - refx).abs().max().item() < 2e-5 * (dy.abs().double() @ W.abs().double()).max().item()
    target = torch.full((N, ld), float("nan"), device="cuda")
    dW = fused.skinny_tn(dy, x, out=target[:, :K])
    refw = dy.double().t() @ x.double()
    assert (dW.double() - refw).abs().max().item() < 1e-5 * (dy.abs().double().t() @ x.abs().double()).max().item()
    assert pitch == 0 or torch.isnan(target[:, K:]).all()              # nothing written outside the slice
    # and through autograd (PointDeconv's constant-channel contribution)
    if N % 4 == 0:
        xi, Wi = x.clone().requires_grad_(True), W.clone().contiguous().requires_grad_(True)
        fused.skinny_linear(xi, Wi).backward(dy)
        assert (xi.grad.double() - refx).abs().max().item() < 2e-5 * max(1.0, refx.abs().max().item())
        assert (Wi.grad.double() - refw).abs().max().item() < 2e-5 * max(1.0, refw.abs().max().item())


def test_linear_cl_with_planes_equals_without():
    """LinearCL with a pre-split weight (forward + input gradient through the planes) against the same layer without: the
    deconvolution blocks' two large contractions take this path (PointDeconv.assembled)."""
    from pdgn_amd import fused
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(6000, 256, device="cuda", generator=g)
    w = (torch.randn(384, 256, device="cuda", generator=g) * 0.2).requires_grad_(True)
    add = torch.randn(6000, 384, device="cuda", generator=g)
    gout = torch.randn(6000, 384, device="cuda", generator=g)
    res = []
    for use in (False, True):
        xi = x.clone().requires_grad_(True)
        w.grad = None
        planes = fused.split_planes(w.detach(), True) if use else None
        assert (planes is not None) == use
        y = fused.linear_cl(xi, w, None, add, planes=planes)
        y.backward(gout)
        res.append((y.detach().clone(), xi.grad.clone(), w.grad.clone()))
    for a_, b_ in zip(*res):
        assert (a_ - b_).abs().max().item() <= 1e-5 * max(1.0, b_.abs().max().item())


@pytest.mark.parametrize("scale", [1.0, 1e15, 1e-15])
@pytest.mark.parametrize("M,N,K", [(4099, 132, 100), (35840, 512, 5120), (35840, 256, 128), (8960, 3232, 32), (40000, 512, 2560)])
def test_gemm_x3_is_as_accurate_as_the_fp32_matrix_instructions(M, N, K, scale, monkeypatch):
    """csrc/gemm_x3.hip multiplies fp32 operands as three bf16 parts each (six bf16 MFMA products per fp32 product, fp32
    accumulation).  Against fp64, relative to sum_k |a| |w|: its error stays below 1e-6 and within 1.25x of the error of the
    fp32 matrix instructions (csrc/gemm_nt.hip, _lib.set_gemm_mode('fp32')) on the same operands -- measured 0.7-0.95x -- for all three
    operand layouts, and over the fp32 exponent range (bf16 shares it: no scaling of the operands is involved)."""
    import ctypes
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(M + K)
    rows = min(M, 8192)
    A = torch.randn(M, K, device="cuda", generator=g) * torch.rand(M, 1, device="cuda", generator=g) * 3 * scale
    W = torch.randn(N, K, device="cuda", generator=g)
    dY = torch.randn(M, N, device="cuda", generator=g) * scale
    a64, w64, d64 = A[:rows].double(), W.double(), dY[:rows].double()
    ref = {"nt": a64 @ w64.t(), "nn": d64 @ w64, "tn": d64.t() @ a64}
    mag = {"nt": a64.abs() @ w64.abs().t(), "nn": d64.abs() @ w64.abs(), "tn": d64.abs().t() @ a64.abs()}
    err = {}
    for mode in ("x2", "x3_32", "x3_16", "fp32"):             # two fp16 parts where they pay; both bf16 matrix instructions; the fp32 ones
        _lib.set_gemm_mode(mode)
        C = torch.empty(M, N, device="cuda")
        assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(A), K, ptr(W), K, None, None, 0, ptr(C), N, None, stream_of(A)) == 0
        dX = torch.empty(M, K, device="cuda")
        assert L.pdgn_gemm_nn(ctypes.c_longlong(M), K, N, ptr(dY), N, ptr(W), K, None, None, 0, ptr(dX), K, None, stream_of(A)) == 0
        out = {"nt": C[:rows], "nn": dX[:rows]}
        if N >= 64 and K >= 64:
            dW = torch.empty(N, K, device="cuda")
            assert L.pdgn_gemm_tn_big(ctypes.c_longlong(rows), N, K, ptr(dY), N, ptr(A), K, ptr(dW), 0, stream_of(A)) == 0
            out["tn"] = dW
        for kind, o in out.items():
            assert torch.isfinite(o).all()
            err[mode, kind] = ((o.double() - ref[kind]).abs() / mag[kind].clamp_min(1e-300)).max().item()
    for (mode, kind), e in err.items():
        assert e < 1e-6, (mode, kind, e)
        if mode in ("x3_32", "x2"):                            # six bf16 partial products smallest first / three fp16 ones (exact products, half the accumulations)
            assert e <= 1.25 * err["fp32", kind] + 2e-8, (mode, kind, e, err["fp32", kind])
        if mode == "x3_16":
            # the 16x16x32 arm adds a chunk's six partial products LARGEST first (the order that lets one set of fragment
            # registers serve consecutive chunks, gemm_x3.hip): five roundings at the sum's magnitude per chunk instead of one --
            # measured up to 1.6x the fp32 instructions' error on short reductions, still below 1e-6 of sum |a||w|
            assert e <= 2.0 * err["fp32", kind] + 2e-8, (mode, kind, e, err["fp32", kind])


def _spread(n, gen, binades=30.0):
    """n powers of two spanning 2^-binades .. 1 (the largest exactly 1)."""
    e = -torch.floor(torch.rand(n, device="cuda", generator=gen) * (binades + 1.0)).clamp_max(binades)
    e[0], e[-1] = 0.0, -binades
    return torch.pow(2.0, e)


@pytest.mark.parametrize("M,N,K", [(20000, 512, 2560), (35840, 512, 5120)])
def test_two_part_rows_spanning_thirty_binades(M, N, K):
    """VERDICT r5 weak #1 / ADVICE r5 (medium): the two-part arithmetic used ONE power-of-two scale per operand, so a row 2^-26 below
    the operand's largest value kept 12 bits -- and a dX row depends on its own dY row only.  Round 6 scales every row of an operand
    (as the kernel sees it: a transposed operand's columns) by its own power of two.  Here the rows of both operands span
    2^-30 .. 1 of the operand's maximum, and the error of EVERY element against fp64, relative to that element's own
    sum_k |a||w| (a component-wise bound: no row hides behind the operand's norm), must stay within 2x the fp32 matrix
    instructions' on the same operands, for all three layouts (nt: rows of A and W; nn: rows of dY, columns of the transposed W;
    tn: columns of dY and X) -- and the calls must really have run on two parts."""
    import ctypes
    from pdgn_amd import _lib, fused
    from pdgn_amd._lib import ptr, stream_of
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    rows = min(M, 8192)
    # nt: C = A W^T, A (M, K) and W (N, K) with rows spanning; nn: dX = dY Wt, dY (M, N) rows and Wt (N, K) COLUMNS spanning;
    # tn: dW = dY2^T X2 over the first `rows` rows, columns of both spanning
    A = torch.randn(M, K, device="cuda", generator=g) * _spread(M, g)[:, None]
    W = torch.randn(N, K, device="cuda", generator=g) * _spread(N, g)[:, None]
    dY = torch.randn(M, N, device="cuda", generator=g) * _spread(M, g)[:, None]
    Wt = torch.randn(N, K, device="cuda", generator=g) * _spread(K, g)[None, :]
    dY2 = torch.randn(rows, N, device="cuda", generator=g) * _spread(N, g)[None, :]
    X2 = torch.randn(rows, K, device="cuda", generator=g) * _spread(K, g)[None, :]
    _lib.set_gemm_mode("x2")
    assert fused.two_part(M, N, K, (M + N) * K * 4) and fused.two_part(M, K, N, (M + K) * N * 4)
    tn_two = fused.two_part(N, K, rows, 0)                       # (its column maxima are handed in below: nothing left to scan)
    assert tn_two
    cm_dy, cm_x = fused.operand_maxima(dY2, rows=False, cols=True), fused.operand_maxima(X2, rows=False, cols=True)
    assert torch.equal(cm_dy, dY2.abs().amax(0).view(torch.int32)) and torch.equal(cm_x, X2.abs().amax(0).view(torch.int32))
    a64, w64, d64, t64, y64, x64 = (t.double() for t in (A[:rows], W, dY[:rows], Wt, dY2, X2))
    ref = {"nt": a64 @ w64.t(), "nn": d64 @ t64, "tn": y64.t() @ x64}
    mag = {"nt": a64.abs() @ w64.abs().t(), "nn": d64.abs() @ t64.abs(), "tn": y64.abs().t() @ x64.abs()}
    err = {}
    for mode in ("x2", "x3", "fp32"):
        _lib.set_gemm_mode(mode)
        C = torch.empty(M, N, device="cuda")
        assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(A), K, ptr(W), K, None, None, 0, ptr(C), N, None, stream_of(A)) == 0
        dX = torch.empty(M, K, device="cuda")
        assert L.pdgn_gemm_nn(ctypes.c_longlong(M), K, N, ptr(dY), N, ptr(Wt), K, None, None, 0, ptr(dX), K, None, stream_of(A)) == 0
        dW = torch.empty(N, K, device="cuda")
        if mode == "x2":
            assert L.pdgn_gemm_set_operand_scales(ptr(cm_dy), ptr(cm_x)) == 0
        assert L.pdgn_gemm_tn_big(ctypes.c_longlong(rows), N, K, ptr(dY2), N, ptr(X2), K, ptr(dW), 0, stream_of(A)) == 0
        for kind, o in (("nt", C[:rows]), ("nn", dX[:rows]), ("tn", dW)):
            assert torch.isfinite(o).all()
            rel = (o.double() - ref[kind]).abs() / mag[kind].clamp_min(1e-300)
            err[mode, kind] = rel.max().item()
            err[mode, kind, "rows"] = rel.amax(1)
    _lib.set_gemm_mode("x2")
    for kind in ("nt", "nn", "tn"):
        assert err["x2", kind] <= 2.0 * err["fp32", kind] + 2e-8, (kind, err["x2", kind], err["x3", kind], err["fp32", kind])
        assert err["x2", kind] < 1e-6
        # per output row as well: the worst row of the two-part form against the worst row of the fp32 instructions
        assert err["x2", kind, "rows"].max().item() <= 2.0 * err["fp32", kind, "rows"].max().item() + 2e-8
    # (that the x2 arm is the two-part kernel, not a silent three-part fallback: a hand-over of ZERO maxima -- scale 2^126 --
    # must overflow the scaled operands)
    zeros = torch.zeros(max(M, N, K), dtype=torch.int32, device="cuda")
    C = torch.empty(M, N, device="cuda")
    assert L.pdgn_gemm_set_operand_scales(ptr(zeros), ptr(zeros)) == 0
    assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(A), K, ptr(W), K, None, None, 0, ptr(C), N, None, stream_of(A)) == 0
    assert not torch.isfinite(C).all()


@pytest.mark.parametrize("M,N,K", [(17920, 256, 2560), (35840, 12832, 128)])
def test_two_part_layer_with_points_of_small_gradient(M, N, K):
    """The same through LinearCL (pre-split planes, handed-in row maxima, the backward's own scans): activations and output
    gradients whose ROWS (points) span 2^-30 .. 1 -- every element of y, dX against fp64 relative to its own sum |.||.|; dW (a sum
    over all rows) relative to its own sum as well."""
    from pdgn_amd import _lib, fused
    _lib.set_gemm_mode("x2")
    g = torch.Generator(device="cuda").manual_seed(M + N + K + 1)
    x = torch.randn(M, K, device="cuda", generator=g) * _spread(M, g)[:, None]
    w = torch.randn(N, K, device="cuda", generator=g) * 0.2 * _spread(N, g, 12.0)[:, None]
    dy = torch.randn(M, N, device="cuda", generator=g) * _spread(M, g)[:, None]
    pl = fused.split_planes(w, True, rows=M, dy_maxima_free=True, x_maxima_free=True)
    assert pl.parts_p == 2 and pl.parts_t == 2
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = fused.linear_cl(xg, wg, None, None, planes=pl, x_max=fused.operand_maxima(x))
    y.backward(dy)
    rows = min(M, 4096)
    x64, w64, d64 = x[:rows].double(), w.double(), dy[:rows].double()
    for name, got, ref, mag in (("y", y.detach()[:rows], x64 @ w64.t(), x64.abs() @ w64.abs().t()),
                                ("dx", xg.grad[:rows], d64 @ w64, d64.abs() @ w64.abs())):
        assert ((got.double() - ref).abs() / mag.clamp_min(1e-300)).max().item() < 2e-6, name
    dwref = dy.double().t() @ x.double()
    dwmag = dy.double().abs().t() @ x.double().abs()
    assert ((wg.grad.double() - dwref).abs() / dwmag.clamp_min(1e-300)).max().item() < 2e-6


@pytest.mark.parametrize("ratio", [30.0, 300.0, 1000.0])
def test_epilogue_statistics_large_mean(ratio):
    """|mean| >> std through the PRODUCER path: linear_cl(want_stats=True) -> bn_act with the
    GEMM's / thin layer's block-shifted partials against fp64 -- normalised output at the north star's 1e-4 where raw
    fp32 sums (E[x^2] - mean^2) are off by 3e-3 .. 3e-2 (tools/bn_shift.py)."""
    import torch.nn as nn
    from pdgn_amd import fused
    g = torch.Generator(device="cuda").manual_seed(int(ratio))
    for M, K, N in ((35840, 64, 128), (8960, 3, 64)):
        x = torch.randn(M, K, device="cuda", generator=g)
        w = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5
        add = torch.full((M, N), ratio, device="cuda") if K > 4 else None      # a large common offset: mean / std = ratio
        b = None if K > 4 else torch.full((N,), ratio, device="cuda")
        bn = nn.BatchNorm1d(N).cuda().train()
        y, part = fused.linear_cl(x, w, b, add, True)
        assert part is not None and part[0].shape[1] == 3 * N and part[1] in (64, 80, 128, 256)      # (partials, rows per block)
        out = fused.bn_act(y, bn, True, act="none", partials=part)
        y64 = y.double()
        want = (y64 - y64.mean(0)) / torch.sqrt(y64.var(0, unbiased=False) + bn.eps)
        err = (out.double() - want).abs().max().item()
        assert err < 1e-4 * max(1.0, want.abs().max().item()), (M, K, N, ratio, err)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), (0.9 + 0.1 * y64.var(0, unbiased=True)).float().cpu().numpy(),
                                   rtol=1e-4)


def test_gemm_nt_strided_operands():
    """Row pitches larger than the logical widths (views into wider matrices) for A, W, the addend and C."""
    import ctypes
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    M, N, K = 5000, 96, 72
    g = torch.Generator(device="cuda").manual_seed(5)
    Abig = torch.randn(M, K + 24, device="cuda", generator=g)
    Wbig = torch.randn(N, K + 8, device="cuda", generator=g)
    Dbig = torch.randn(M, N + 4, device="cuda", generator=g)
    Cbig = torch.zeros(M, N + 32, device="cuda")
    A, W, D, C = Abig[:, 4:4 + K], Wbig[:, :K], Dbig[:, 4:], Cbig[:, 16:16 + N]
    assert _lib.lib().pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(A), A.stride(0), ptr(W), W.stride(0), None, ptr(D), D.stride(0),
                                   ptr(C), C.stride(0), None, stream_of(A)) == 0
    ref = A.double() @ W.double().t() + D.double()
    assert (C.double() - ref).abs().max().item() < 1e-4
    assert Cbig[:, :16].abs().max().item() == 0 and Cbig[:, 16 + N:].abs().max().item() == 0


@pytest.mark.parametrize("B,N,C,training", [(4, 300, 64, True), (35, 2048, 1024, True), (3, 17, 8, True), (5, 512, 256, False)])
def test_fused_bn_act_maxpool_vs_torch(B, N, C, training):
    from pdgn_amd.fused import bn_act_maxpool, flush_bn_counters
    from torch_standins import bn_act_maxpool_torch
    rng = np.random.default_rng(B * N + C)
    x = torch.from_numpy((rng.standard_normal((B * N, C)) * 1.5 + 0.3).astype(np.float32))
    gout = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32))
    res = []
    for impl, to in ((bn_act_maxpool, dev), (bn_act_maxpool_torch, lambda t: t.double())):
        bn = torch.nn.BatchNorm1d(C)
        fill_module(bn, salt=5)
        bn = bn.cuda() if impl is bn_act_maxpool else bn.double()
        bn.train(training)
        xi = to(x).requires_grad_(True)
        y = impl(xi, bn, training, B, N)
        y.backward(to(gout))
        flush_bn_counters()
        res.append([t.detach().cpu().double().numpy() for t in
                    (y, xi.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)])
        if impl is bn_act_maxpool and training:
            assert int(bn.num_batches_tracked) == 1
    for name, a, b in zip(["y", "dx", "dgamma", "dbeta", "running_mean", "running_var"], *res):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(b).max()), err_msg=name)


@pytest.mark.parametrize("B,N,C,K,frozen", [(35, 2048, 1024, 256, True), (6, 256, 256, 128, True), (4, 1024, 512, 256, True),
                                            (3, 700, 64, 40, True), (35, 2048, 1024, 256, False), (6, 256, 256, 128, False),
                                            (5, 512, 512, 256, False), (3, 640, 64, 16, False)])
def test_last_layer_adjoint_without_the_dense_gradient(B, N, C, K, frozen):
    """dense -> BatchNorm1d -> LeakyReLU -> MaxPool1d (a discriminator's last per-point layer): pdgn_dense_bn_maxpool_backward
    (dh = S W - 1 ca^T W - h W^T diag(cb) W, dW = S^T h - ca 1^T h - diag(cb) W h^T h) against fp64 torch and against the
    two-Function path it replaces; frozen = the generator's update (input gradient only)."""
    from pdgn_amd import fused
    from torch_standins import bn_act_maxpool_torch
    rng = np.random.default_rng(B + N + C + K)
    h0 = torch.from_numpy(rng.standard_normal((B * N, K)).astype(np.float32))
    W0 = torch.from_numpy((rng.standard_normal((C, K)) / np.sqrt(K)).astype(np.float32))
    bias0 = torch.from_numpy(rng.standard_normal(C).astype(np.float32))
    gout = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32))
    res = {}
    for name in ("closed", "dense", "torch"):
        to = (lambda t: t.double()) if name == "torch" else dev
        bn = torch.nn.BatchNorm1d(C)
        fill_module(bn, salt=7)
        bn = bn.double() if name == "torch" else bn.cuda()
        bn.train(True)
        for p in bn.parameters():
            p.requires_grad_(not frozen)
        h = to(h0).requires_grad_(True)
        W, bias = to(W0).requires_grad_(not frozen), to(bias0).requires_grad_(not frozen)
        if name == "torch":
            y = bn_act_maxpool_torch(h @ W.t(), bn, True, B, N, pre_bias=bias)
        else:
            x, part = fused.linear_cl(h, W, None, None, True)
            y = fused.bn_act_maxpool(x, bn, True, B, N, pre_bias=bias, partials=part,
                                     dense=fused.DenseInput(h, W) if name == "closed" else None)
            assert "BNActMaxPool" in type(y.grad_fn).__name__
            assert (y.grad_fn.dense is not None) == (name == "closed"), "the closed form was (not) taken"
        y.backward(to(gout))
        fused.flush_bn_counters()
        if name != "torch":
            assert not fused._INPUT_GRADS, "the placeholder was consumed"
        got = [y, h.grad] + ([] if frozen else [W.grad, bn.weight.grad, bn.bias.grad, bias.grad])
        res[name] = [t.detach().cpu().double().numpy() for t in got]
    names = ["y", "dh", "dW", "dgamma", "dbeta", "dbias"]
    for i, ref in enumerate(res["torch"]):
        scale = max(1e-6, np.abs(ref).max())
        if names[i] == "dbias":                                       # analytically zero: both sides hold rounding residue
            wscale = np.abs(res["torch"][2]).max()
            assert np.abs(res["closed"][i]).max() <= 1e-4 * wscale and np.abs(ref).max() <= 1e-4 * wscale
            continue
        np.testing.assert_allclose(res["closed"][i], ref, rtol=1e-4, atol=1e-4 * scale, err_msg=names[i])
        np.testing.assert_allclose(res["dense"][i], ref, rtol=1e-4, atol=1e-4 * scale, err_msg=names[i] + " (dense path)")


@pytest.mark.parametrize("case", ["no_fold", "bias_in_gemm", "other_producer", "second_consumer"])
def test_closed_tail_is_refused_when_its_input_is_not_the_plain_dense_output(case, monkeypatch):
    """the closed-form tail hands LinearCL a placeholder instead of dx, which is only right when the
    max-pool's input IS h W^T, straight from that LinearCL.  With a bias added in between (PDGN_FOLD_BIAS=0), a bias or
    addend inside the GEMM, or another producer, the dense path must be taken; every gradient then equals fp64 torch.
    A second consumer of the GEMM's output would receive the placeholder: LinearCL raises instead of using NaNs."""
    from pdgn_amd import fused
    from torch_standins import bn_act_maxpool_torch
    B, N, C, K = 4, 512, 128, 64
    rng = np.random.default_rng(11)
    h0 = torch.from_numpy(rng.standard_normal((B * N, K)).astype(np.float32))
    W0 = torch.from_numpy((rng.standard_normal((C, K)) / np.sqrt(K)).astype(np.float32))
    bias0 = torch.from_numpy(rng.standard_normal(C).astype(np.float32))
    gout = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32))
    if case == "no_fold":
        monkeypatch.setattr(fused, "_NO_FOLD", True)
    res = {}
    for name in ("hip", "torch"):
        to = (lambda t: t.double()) if name == "torch" else dev
        bn = torch.nn.BatchNorm1d(C)
        fill_module(bn, salt=7)
        bn = (bn.double() if name == "torch" else bn.cuda()).train(True)
        h = to(h0).requires_grad_(True)
        W, bias = to(W0).requires_grad_(True), to(bias0).requires_grad_(True)
        if name == "torch":
            x = h @ W.t() + (bias if case == "bias_in_gemm" else 0.0)
            y = bn_act_maxpool_torch(x * (2.0 if case == "other_producer" else 1.0), bn, True, B, N,
                                     pre_bias=None if case == "bias_in_gemm" else bias)
            extra = x.sum() if case == "second_consumer" else 0.0
        else:
            x = fused.linear_cl(h, W, bias if case == "bias_in_gemm" else None)
            xin = x * 2.0 if case == "other_producer" else x
            y = fused.bn_act_maxpool(xin, bn, True, B, N, pre_bias=None if case == "bias_in_gemm" else bias,
                                     dense=fused.DenseInput(h, W))
            if case != "second_consumer":
                assert y.grad_fn.dense is None, "the closed form must be refused here"
            extra = x.sum() if case == "second_consumer" else 0.0
        if case == "second_consumer" and name == "hip":
            # x feeds the max-pool tail (closed form: placeholder) AND a sum: autograd adds both gradients -> not the placeholder
            # any more, the NaN spreads into the sum instead of a plausible number -- or LinearCL sees the bare placeholder and raises
            try:
                (y * to(gout)).sum().add(extra).backward()
            except RuntimeError as e:
                assert "placeholder" in str(e)
            else:
                assert not torch.isfinite(h.grad).all(), "a mis-routed placeholder must not produce finite gradients"
            fused.clear_zero_colsum()
            return
        (y * to(gout)).sum().add(extra).backward()
        fused.flush_bn_counters()
        res[name] = [t.detach().cpu().double().numpy() for t in (y, h.grad, W.grad, bn.weight.grad, bn.bias.grad)]
    for i, (a, ref) in enumerate(zip(res["hip"], res["torch"])):
        np.testing.assert_allclose(a, ref, rtol=1e-4, atol=1e-4 * max(1e-6, np.abs(ref).max()), err_msg=str(i))


def test_last_layer_adjoint_on_the_fp32_matrix_instructions():
    """The closed-form adjoint issues its three products through pdgn_gemm_nt / pdgn_gemm_tn_big: the same entry under PDGN_GEMM=fp32."""
    from pdgn_amd import _lib
    _lib.set_gemm_mode("fp32")
    test_last_layer_adjoint_without_the_dense_gradient(6, 256, 256, 128, False)
    test_last_layer_adjoint_without_the_dense_gradient(4, 1024, 512, 256, True)


@pytest.mark.parametrize("B,N,C", [(35, 2048, 1024), (4, 300, 64), (3, 17, 8)])
def test_maxpool_tail_statistics_and_extremes_in_one_pass(B, N, C):
    """bn_act_maxpool in training mode WITHOUT statistics from the producer: pdgn_bn_stats_act_maxpool keeps max and min of x per split
    and picks by the sign of the channel's scale -- channels with negative and zero gamma included -- against the torch stand-in
    (values, input / parameter gradients, running statistics)."""
    from pdgn_amd.fused import bn_act_maxpool, flush_bn_counters
    from torch_standins import bn_act_maxpool_torch
    rng = np.random.default_rng(B * N + C)
    x = torch.from_numpy((rng.standard_normal((B * N, C)) * 1.5 + 0.3).astype(np.float32))
    gout = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32))
    gamma = torch.from_numpy(rng.standard_normal(C).astype(np.float32))            # both signs
    gamma[0] = 0.0
    res = []
    for impl, to in ((bn_act_maxpool, dev), (bn_act_maxpool_torch, lambda t: t.double())):
        bn = torch.nn.BatchNorm1d(C)
        fill_module(bn, salt=5)
        with torch.no_grad():
            bn.weight.copy_(gamma)
        bn = bn.cuda() if impl is bn_act_maxpool else bn.double()
        bn.train(True)
        xi = to(x).requires_grad_(True)
        y = impl(xi, bn, True, B, N)
        y.backward(to(gout))
        flush_bn_counters()
        res.append([t.detach().cpu().double().numpy() for t in (y, xi.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)])
    for name, a, b in zip(["y", "dx", "dgamma", "dbeta", "running_mean", "running_var"], *res):
        if name == "dx":                                            # channel 0 (gamma = 0): every row ties, any of them may take the
            a, b = a[:, 1:], b[:, 1:]                               # gradient (and with it dgamma[0] = sum dz * xhat at that row)
        if name == "dgamma":
            a, b = a[1:], b[1:]
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(b).max()), err_msg=name)


def test_bias_feeding_training_batchnorm_gets_analytic_zero_grad():
    """sum_rows d(BN input) == 0 in training mode: the producer's bias gradient is returned as exact zeros and
    the full pass over dy is skipped; the skipped sum is rounding residue (checked here), eval mode is untouched."""
    import torch.nn as nn
    from pdgn_amd import fused
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    lin = nn.Linear(64, 128).to(dev)
    bn = nn.BatchNorm1d(128).to(dev)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    x = torch.randn(4096, 64, device=dev)
    t = torch.randn(4096, 128, device=dev)
    for training in (True, False):
        lin.zero_grad()
        h = fused.linear_cl(x, lin.weight, lin.bias)
        h.retain_grad()
        y = fused.bn_act(h, bn, training, act="leaky_relu")
        (y * t).sum().backward()
        resid = h.grad.sum(0).abs().max().item()
        scale = h.grad.abs().sum(0).max().item()
        if training:
            assert torch.count_nonzero(lin.bias.grad).item() == 0
            assert resid <= 1e-5 * scale                      # what the skipped row-sum would have produced
        else:
            torch.testing.assert_close(lin.bias.grad, h.grad.sum(0), rtol=1e-4, atol=1e-4 * scale)
            assert resid > 1e-3 * scale


@pytest.mark.parametrize("training", [True, False])
def test_pre_bias_folded_into_batchnorm(training):
    """bn_act(x, pre_bias=b) == bn_act(x + b): outputs, running statistics and gradients (the producer's bias is
    never added to the tensor; training: its gradient is the analytic zero; eval: falls back to the explicit add)."""
    import copy
    import torch.nn as nn
    from pdgn_amd import fused
    torch.manual_seed(13)
    dev_ = torch.device("cuda:0")
    bn_a = nn.BatchNorm1d(64).to(dev_)
    with torch.no_grad():
        bn_a.weight.uniform_(0.5, 1.5); bn_a.bias.uniform_(-0.5, 0.5)
        bn_a.running_mean.uniform_(-0.3, 0.3); bn_a.running_var.uniform_(0.5, 2.0)
    bn_b = copy.deepcopy(bn_a)
    x = torch.randn(5000, 64, device=dev_)
    bias_a = (torch.randn(64, device=dev_) * 0.7).requires_grad_(True)
    bias_b = bias_a.detach().clone().requires_grad_(True)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    t = torch.randn(5000, 64, device=dev_)
    ya = fused.bn_act(xa, bn_a, training, pre_bias=bias_a)
    yb = fused.bn_act(xb + bias_b, bn_b, training)
    torch.testing.assert_close(ya, yb, rtol=1e-5, atol=1e-5)
    (ya * t).sum().backward()
    (yb * t).sum().backward()
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(bn_a.weight.grad, bn_b.weight.grad, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(bn_a.bias.grad, bn_b.bias.grad, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(bn_a.running_mean, bn_b.running_mean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(bn_a.running_var, bn_b.running_var, rtol=1e-5, atol=1e-6)
    if training:
        assert torch.count_nonzero(bias_a.grad).item() == 0
        assert bias_b.grad.abs().max().item() <= 1e-4 * xb.grad.abs().sum(0).max().item()
    else:
        torch.testing.assert_close(bias_a.grad, bias_b.grad, rtol=1e-4, atol=1e-4)
        with torch.no_grad():                                    # no-grad eval: folded into the eval statistics
            torch.testing.assert_close(fused.bn_act(x, bn_a, False, pre_bias=bias_a), fused.bn_act(x + bias_a, bn_a, False),
                                       rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("groups,group_rows,C,pitch", [(1, 71680, 64, 0), (35, 2048, 256, 0), (1, 35, 256, 0), (35, 512, 128, 6432),
                                                        (35, 10240, 16, 0), (3, 7, 1024, 0), (2, 100, 48, 0)])
def test_group_colsum(groups, group_rows, C, pitch):
    """pdgn_group_colsum (bias gradients / per-sample sums of the adjoints) against fp64 torch, also on a column slice of a wider
    matrix (the per-sample biases of the edge convolutions) and on a channel count it leaves to torch."""
    from pdgn_amd import fused
    g = torch.Generator(device="cuda").manual_seed(groups * group_rows + C)
    rows = groups * group_rows
    full = torch.randn(rows, pitch or C, device="cuda", generator=g)
    x = full[:, 8:8 + C] if pitch else full
    got = fused.group_colsum(x, group_rows if groups > 1 else None)
    ref = x.double().view(groups, group_rows, C).sum(dim=1) if not pitch else x.double().reshape(groups, group_rows, C).sum(dim=1)
    assert got.shape == (groups, C)
    bound = x.double().abs().reshape(groups, group_rows, C).sum(dim=1).max().item()
    assert (got.double() - ref).abs().max().item() <= 2e-6 * bound


@pytest.mark.parametrize("frozen", [True, False])
@pytest.mark.parametrize("R,dims", [(35, (1024, 512, 256, 64, 1)), (35, (256, 128, 64, 1)), (8, (512, 256, 64, 1)), (3, (20, 12, 1))])
def test_discriminator_head_on_the_skinny_kernels(R, dims, frozen):
    """A discriminator's nn.Linear + LeakyReLU head (no BatchNorm) through fused.small_sequential: forward on pdgn_skinny_nt_act;
    with FROZEN parameters (the generator's update) the input gradient is one launch per layer (pdgn_skinny_nn_masked, act' applied
    on load); trainable, pdgn_small_mlp_backward with the activation's derivative read off y.  Against torch's own nn.Sequential."""
    import copy
    import torch.nn as nn
    from pdgn_amd import fused
    torch.manual_seed(R + dims[0])
    layers = []
    for a, b in zip(dims[:-2], dims[1:-1]):
        layers += [nn.Linear(a, b), nn.LeakyReLU(inplace=True)]
    layers.append(nn.Linear(dims[-2], dims[-1]))
    ref = nn.Sequential(*layers).cuda()
    mine = copy.deepcopy(ref)
    for p in mine.parameters():
        p.requires_grad_(not frozen)
    x = torch.randn(R, dims[0], device="cuda")
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    t = torch.randn(R, dims[-1], device="cuda")
    ya = fused.small_sequential(mine, xa, True)
    yb = ref(xb)
    torch.testing.assert_close(ya, yb, rtol=2e-4, atol=2e-5)
    (ya * t).sum().backward()
    (yb * t).sum().backward()
    scale = xb.grad.abs().max().item()
    assert (xa.grad - xb.grad).abs().max().item() <= 1e-4 * scale
    if not frozen:
        for (n1, p1), (n2, p2) in zip(mine.named_parameters(), ref.named_parameters()):
            scale = max(p2.grad.abs().max().item(), 1e-6)
            assert (p1.grad - p2.grad).abs().max().item() <= 1e-4 * scale + 1e-7, n1


@pytest.mark.parametrize("R,dims,training", [(35, (128, 256, 256), True), (35, (64, 64, 512), True), (6, (32, 48), True),
                                             (35, (512, 128), False), (64, (1000, 16), True), (64, (632, 16), True)])
def test_small_sequential_vs_torch(R, dims, training):
    """Linear + BatchNorm1d + LeakyReLU groups on a few rows as single launches vs the same nn.Sequential in torch:
    outputs, input / parameter gradients, running statistics, num_batches_tracked.  (64, (1000, 16)) is beyond the fused launch's
    LDS (64 * 1004 * 4 + 1024 bytes > 160 KiB): small_sequential leaves it to torch, and the case pins that hand-over; (64, (632, 16))
    is the widest layer that 64 rows -- a full wave, no idle lane -- run on csrc/small_mlp.hip."""
    import copy
    import torch.nn as nn
    from pdgn_amd import fused
    torch.manual_seed(R + dims[0])
    layers = []
    for a, b in zip(dims[:-1], dims[1:]):
        layers += [nn.Linear(a, b), nn.BatchNorm1d(b), nn.LeakyReLU(inplace=True)]
    ref = nn.Sequential(*layers).cuda()
    with torch.no_grad():
        for m in ref:
            if isinstance(m, nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.5, 0.5)
                m.running_mean.uniform_(-0.3, 0.3); m.running_var.uniform_(0.5, 2.0)
    mine = copy.deepcopy(ref)
    ref.train(training); mine.train(training)
    x = torch.randn(R, dims[0], device="cuda")
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    t = torch.randn(R, dims[-1], device="cuda")
    ya = fused.small_sequential(mine, xa, training)
    fused.flush_bn_counters()
    yb = ref(xb)
    torch.testing.assert_close(ya, yb, rtol=2e-4, atol=2e-5)
    (ya * t).sum().backward()
    (yb * t).sum().backward()
    torch.testing.assert_close(xa.grad, xb.grad, rtol=2e-3, atol=2e-5)
    wscale = max(p.grad.abs().max().item() for n, p in ref.named_parameters() if n.endswith("weight"))
    for (n1, p1), (n2, p2) in zip(mine.named_parameters(), ref.named_parameters()):
        if training and n1.endswith(".bias") and int(n1.split(".")[0]) % 3 == 0:
            # bias of a Linear in front of a training-mode BatchNorm: analytically zero, both sides hold rounding residue
            assert p1.grad.abs().max().item() <= 1e-4 * wscale and p2.grad.abs().max().item() <= 1e-4 * wscale, n1
            continue
        scale = max(p2.grad.abs().max().item(), 1e-6)
        assert (p1.grad - p2.grad).abs().max().item() <= 2e-3 * scale + 1e-6, n1
    for (n1, b1), (n2, b2) in zip(mine.named_buffers(), ref.named_buffers()):
        torch.testing.assert_close(b1.float(), b2.float(), rtol=1e-5, atol=1e-6, msg=n1)


@pytest.mark.parametrize("B,N,C", [(3, 128, 32), (35, 1024, 128), (2, 300, 20), (4, 129, 6)])
def test_point_max_forward_backward(B, N, C):
    """MaxPool2d((1,N)) over the points (models/PDGNet_v2.py:699): values, and the gradient routed to the argmax."""
    from pdgn_amd.fused import point_max
    rng = np.random.default_rng(B * N + C)
    x = torch.from_numpy(rng.standard_normal((B, N, C)).astype(np.float32))
    x[0, 5, 0] = x[0, 77 % N, 0] = 9.0                       # a tie: the lowest point index takes the gradient
    g = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32))
    xg = dev(x).requires_grad_(True)
    out = point_max(xg)
    out.backward(dev(g))
    ref = x.max(dim=1)[0]
    assert torch.equal(out.detach().cpu(), ref)
    arg = torch.zeros(B, C, dtype=torch.long)
    for b in range(B):
        for c in range(C):
            arg[b, c] = int(torch.nonzero(x[b, :, c] == ref[b, c])[0])
    want = torch.zeros_like(x).scatter_(1, arg.unsqueeze(1), g.unsqueeze(1))
    assert torch.equal(xg.grad.cpu(), want)


@pytest.mark.parametrize("gemm", ["x2", "x3", "fp32", "x3_16"])
def test_gemm_nt_ex_masked_lanes_in_a_fresh_process(gemm):
    """The extended epilogue on a tile that is wider than the problem (N = 36 < 64) in a FRESH process: lanes past the last column
    are masked with an out-of-range offset, which only works against a BOUNDED buffer descriptor -- the per-group bias table's
    descriptor was unbounded (round 3), the masked lanes read row_bias + 1 GiB, and that faulted exactly when nothing was mapped
    there, i.e. in a small fresh process and never in the long test run (found in round 4 by running this case alone)."""
    import subprocess
    import sys
    code = (
        "import ctypes, sys, torch; sys.path.insert(0, %r); from pdgn_amd import _lib; from pdgn_amd._lib import ptr, stream_of;"
        "_lib.set_gemm_mode(%r); L = _lib.lib(); M, N, K = 1000, 36, 20;"
        "A = torch.randn(M, K, device='cuda'); W = torch.randn(N, K, device='cuda'); rb = torch.randn(M, N + 4, device='cuda')[:, :N];"
        "C = torch.empty(M, N, device='cuda');"
        "rc = L.pdgn_gemm_nt_ex(ctypes.c_longlong(M), N, K, ptr(A), K, ptr(W), K, None, None, 0, ptr(C), N, None, ptr(rb), rb.stride(0), 1, 2,"
        " None, 0, 0, stream_of(A)); torch.cuda.synchronize();"
        "ref = torch.nn.functional.leaky_relu(A.double() @ W.double().t() + rb.double());"
        "assert rc == 0 and (C.double() - ref).abs().max().item() < 1e-4; print('ok')" % (ROOT_DIR, gemm))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-1500:]


@pytest.mark.parametrize("cfg", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("gemm", ["x2", "x3", "fp32", "x3_16"])
@pytest.mark.parametrize("M,N,K,rpg", [(35840, 256, 128, 1024), (5000, 132, 36, 250), (8960, 64, 256, 8960), (1000, 36, 20, 1)])
def test_gemm_nt_extended_epilogue(M, N, K, rpg, cfg, monkeypatch, gemm):
    """pdgn_gemm_nt_ex through the C ABI, every tile configuration: bias per group of rows + LeakyReLU on the result (the
    heads' first layer), and the LeakyReLU-derivative gate on the transposed-weight form (their backward), against fp64."""
    import ctypes
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    from pdgn_amd import _lib as _sw
    _sw.set_gemm_config(cfg)                                   # forced tile configuration | None: the launch model's pick
    _sw.set_gemm_mode(gemm)                                    # csrc/gemm_x3.hip (the default) | csrc/gemm_nt.hip; conftest resets both
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    A = torch.randn(M, K, device="cuda", generator=g)
    W = torch.randn(N, K, device="cuda", generator=g)
    bias = torch.randn(N, device="cuda", generator=g)
    groups = -(-M // rpg)
    rb = torch.randn(groups, N + 4, device="cuda", generator=g)[:, :N]          # pitch > width
    C = torch.full((M, N), float("nan"), device="cuda")
    assert L.pdgn_gemm_nt_ex(ctypes.c_longlong(M), N, K, ptr(A), K, ptr(W), K, ptr(bias), None, 0, ptr(C), N, None, ptr(rb),
                             rb.stride(0), rpg, 2, None, 0, 0, stream_of(A)) == 0
    grp = torch.arange(M, device="cuda") // rpg
    ref = torch.nn.functional.leaky_relu(A.double() @ W.double().t() + bias.double() + rb.double()[grp])
    scale = (A.abs() @ W.abs().t()) + 1
    assert ((C.double() - ref).abs() / scale.double()).max().item() < 1e-5
    # transposed-weight form with a gate: C2 = (A2 Wt) * lrelu'(gate)
    A2 = torch.randn(M, N, device="cuda", generator=g)
    gate = torch.randn(M, K + 8, device="cuda", generator=g)[:, :K]
    C2 = torch.full((M, K), float("nan"), device="cuda")
    assert L.pdgn_gemm_nt_ex(ctypes.c_longlong(M), K, N, ptr(A2), N, ptr(W), K, None, None, 0, ptr(C2), K, None, None, 0, 1, 0,
                             ptr(gate), gate.stride(0), 1, stream_of(A)) == 0
    ref2 = (A2.double() @ W.double()) * torch.where(gate > 0, 1.0, 0.01).double()
    scale2 = (A2.abs() @ W.abs()) + 1
    assert ((C2.double() - ref2).abs() / scale2.double()).max().item() < 1e-5


@pytest.mark.parametrize("B,M,Fo,nc", [(3, 512, 64, 512), (2, 2048, 256, 256), (5, 256, 32, 512)])
def test_head_mlp_vs_torch(B, M, Fo, nc):
    """fused.HeadMLP (mlp1..4 with the per-sample term, activations and their derivatives in GEMM epilogues) against the same
    head on cat([g broadcast, x]) in fp64 torch: output, input gradients and every parameter gradient."""
    import torch.nn as nn
    from pdgn_amd.fused import HeadMLP
    torch.manual_seed(B * M + Fo)
    head = nn.Sequential(nn.Conv1d(nc + Fo, 256, 1), nn.LeakyReLU(), nn.Conv1d(256, 64, 1), nn.LeakyReLU(), nn.Conv1d(64, 3, 1)).cuda()
    x = torch.randn(B * M, Fo, device="cuda", requires_grad=True)
    g = torch.randn(B, nc, device="cuda", requires_grad=True)
    dp = torch.randn(B * M, 3, device="cuda")
    w2 = lambda c: c.weight.view(c.weight.shape[0], c.weight.shape[1])
    p = HeadMLP.apply(x, g, w2(head[0]), head[0].bias, w2(head[2]), head[2].bias, w2(head[4]), head[4].bias, B)
    p.backward(dp)
    got = [p.detach(), x.grad, g.grad] + [q.grad.reshape(q.grad.shape[0], -1) if q.grad.dim() == 3 else q.grad for q in head.parameters()]
    ref = nn.Sequential(nn.Conv1d(nc + Fo, 256, 1), nn.LeakyReLU(), nn.Conv1d(256, 64, 1), nn.LeakyReLU(), nn.Conv1d(64, 3, 1)).double().cuda()
    ref.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
    xr, gr = x.detach().double().requires_grad_(True), g.detach().double().requires_grad_(True)
    inp = torch.cat((gr.unsqueeze(2).expand(-1, -1, M), xr.view(B, M, Fo).transpose(1, 2)), 1)       # (B, nc + Fo, M)
    pr = ref(inp).transpose(1, 2).reshape(B * M, 3)
    pr.backward(dp.double())
    want = [pr.detach(), xr.grad, gr.grad] + [q.grad.reshape(q.grad.shape[0], -1) if q.grad.dim() == 3 else q.grad for q in ref.parameters()]
    names = ["p", "dx", "dg", "dW0", "db0", "dW2", "db2", "dW3", "db3"]
    for n, a, b in zip(names, got, want):
        tol = 1e-4 * max(1.0, float(b.abs().max()))
        assert (a.double() - b).abs().max().item() < tol * (20 if n.startswith("d") and n != "dx" else 1), n


@pytest.mark.parametrize("M,N,K", [(35840, 512, 5120), (17920, 256, 2560), (9000, 132, 1284), (4100, 64, 6432), (8960, 128, 1280),
                                   (36000, 128, 2048), (35840, 128, 12832), (20100, 132, 900)])      # (the last three: the flattened layout)
def test_stream_k_tail_without_atomics(M, N, K):
    """Round 5: a launch whose tiles do not fill the last round of workgroups finishes its leftover tiles as split-K partial tiles
    in a caller-provided workspace + a reduce kernel (csrc/gemm_x3.hip: pdgn_gemm_tail_workspace_floats / pdgn_gemm_set_tail_workspace)
    instead of fp32 atomics into zero-filled rows: against fp64, against the atomic form, bit-identical from run to run, with bias
    and addend, on partial edge tiles; and the hand-over is consumed by exactly one call."""
    import ctypes
    from pdgn_amd import _lib, fused
    from pdgn_amd._lib import ptr, stream_of
    L = _lib.lib()
    L.pdgn_gemm_tail_workspace_floats.restype = ctypes.c_longlong
    need = L.pdgn_gemm_tail_workspace_floats(ctypes.c_longlong(M), N, K, 0)
    cfg = L.pdgn_gemm_nt_config(ctypes.c_longlong(M), N, K, 0)
    assert (need > 0) == (cfg >= 16), (need, cfg)                       # a tail exactly where the launch model plans one
    assert L.pdgn_gemm_tail_workspace_floats(ctypes.c_longlong(M), N, K, 1) == 0      # launches with statistics have no tail
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g)
    bias = torch.randn(N, device="cuda", generator=g)
    add = torch.randn(M, N, device="cuda", generator=g)
    ref = a.double() @ w.double().t() + bias.double() + add.double()
    mag = a.double().abs() @ w.double().abs().t() + 1.0

    def run(with_ws):
        c = torch.full((M, N), float("nan"), device="cuda")
        ws = torch.empty(max(need, 1), device="cuda")
        if with_ws and need:
            assert L.pdgn_gemm_set_tail_workspace(ptr(ws), ctypes.c_longlong(need)) == 0
        assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(w), K, ptr(bias), ptr(add), N, ptr(c), N, None, stream_of(a)) == 0
        torch.cuda.synchronize()
        return c
    c1, c2, c_atomic = run(True), run(True), run(False)
    assert ((c1.double() - ref).abs() / mag).max().item() < 1e-6
    assert ((c_atomic.double() - ref).abs() / mag).max().item() < 1e-6
    assert torch.equal(c1, c2), "the workspace form sums a tile's slices in a fixed order"
    # consumed by ONE call: the second call after one hand-over runs the atomic form (and is still right)
    ws = torch.empty(max(need, 1), device="cuda")
    if need:
        assert L.pdgn_gemm_set_tail_workspace(ptr(ws), ctypes.c_longlong(need)) == 0
    for _ in range(2):
        c = torch.full((M, N), float("nan"), device="cuda")
        assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(w), K, None, None, 0, ptr(c), N, None, stream_of(a)) == 0
        assert ((c.double() - (a.double() @ w.double().t())).abs() / mag).max().item() < 1e-6
    # too small a buffer is ignored (atomic form), never overrun
    if need:
        small = torch.empty(need // 2, device="cuda")
        assert L.pdgn_gemm_set_tail_workspace(ptr(small), ctypes.c_longlong(need // 2)) == 0
        c = torch.full((M, N), float("nan"), device="cuda")
        assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(w), K, None, None, 0, ptr(c), N, None, stream_of(a)) == 0
        assert torch.isfinite(c).all()
    # the Python wrappers hand it over themselves: linear layers through fused.gemm_nt are deterministic now
    assert torch.equal(fused.gemm_nt(a, w, bias), fused.gemm_nt(a, w, bias))



@pytest.mark.parametrize("M,N,K", [(20000, 512, 2560), (35840, 12832, 128), (17920, 2560, 256)])
def test_gemm_two_part_planes_and_maxima(M, N, K):
    """Mode "x2" (the default): a product whose time is its matrix-core work runs on TWO scaled fp16 parts per value and three fp16
    MFMA products (gemm_x3.hip NP = 2), every ROW of an operand scaled by its own power of two (round 6).  pdgn_gemm_two_part says
    where; pdgn_split_f16x2 writes a weight's two planes (row r scaled by 2^e_r, e_r from that row's largest magnitude) with the
    rows' maxima behind them -- they reassemble to the weight to 2^-22 of each ROW's maximum; the product through the planes equals
    the unsplit entry point's bit for bit (same parts, same order), with the activations' row maxima scanned by the call or handed
    in from pdgn_absmax_rows_cols, over the fp32 exponent range; against fp64 below 1e-6 of sum |a||w|; two-part planes are refused
    for a shape the launch model gives another tile."""
    import ctypes
    from pdgn_amd import _lib, fused
    from pdgn_amd._lib import ptr, stream_of
    L = _lib.lib()
    _lib.set_gemm_mode("x2")
    assert fused.two_part(M, N, K, M * K * 4) and not fused.two_part(3000, 256, 8, 0) and not fused.two_part(M, N, K, 1 << 40)
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    for scale in (1.0, 3e-18, 7e12):
        a = torch.randn(M, K, device="cuda", generator=g) * scale
        w = torch.randn(N, K, device="cuda", generator=g) * 0.3
        bias = torch.randn(N, device="cuda", generator=g) * scale
        pl = fused.split_planes(w, True, rows=M)
        assert pl.parts_p == 2 and pl.p.shape[:2] == (2, N)
        h, l = pl.p[0, :, :K].view(torch.float16).double(), pl.p[1, :, :K].view(torch.float16).double()
        npl = 2 * N * pl.p.shape[2]
        rmax = pl.p._base[npl:npl + 2 * N].view(torch.int32)      # the rows' maxima (bit patterns), right behind the two planes
        assert torch.equal(rmax, w.abs().amax(1).view(torch.int32))
        e = 14 - torch.floor(torch.log2(w.abs().amax(1).double()))
        wmax = w.abs().amax(1, keepdim=True).double()
        assert bool(((wmax[:, 0] * 2.0 ** e >= 2.0 ** 14) & (wmax[:, 0] * 2.0 ** e < 2.0 ** 15)).all())
        assert bool((((h + l) * (2.0 ** -e)[:, None] - w.double()).abs() <= 2.0 ** -22 * wmax).all())
        if pl.parts_t == 2:                                        # the transposed planes: the COLUMNS' maxima behind them
            tmax = pl.t._base[2 * K * pl.t.shape[2]:2 * K * pl.t.shape[2] + 2 * K].view(torch.int32)
            assert torch.equal(tmax, w.abs().amax(0).view(torch.int32))
            ht, lt = pl.t[0, :, :N].view(torch.float16).double(), pl.t[1, :, :N].view(torch.float16).double()
            et = 14 - torch.floor(torch.log2(w.abs().amax(0).double()))
            assert bool((((ht + lt) * (2.0 ** -et)[:, None] - w.double().t()).abs() <= 2.0 ** -22 * w.abs().amax(0).double()[:, None]).all())
        ref = a.double() @ w.double().t() + bias.double()
        mag = a.double().abs() @ w.double().abs().t() + abs(scale)
        c0, c1, c2 = (torch.empty(M, N, device="cuda") for _ in range(3))
        wp = ctypes.c_longlong(N * pl.p.shape[2])
        # (a tail workspace with every call: partial tiles summed in a fixed order, so that equal arithmetic gives equal bits)
        ws = fused._tail_workspace(L, M, N, K, False, a.device)
        assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(w), K, ptr(bias), None, 0, ptr(c0), N, None, stream_of(a)) == 0
        ws = fused._tail_workspace(L, M, N, K, False, a.device)
        assert L.pdgn_gemm_nt_ps(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(pl.p), pl.p.shape[2], wp, 2, ptr(bias), None, 0, ptr(c1), N, None,
                                 None, 0, 1, 0, None, 0, stream_of(a)) == 0
        slot = fused.operand_maxima(a)                           # the caller's own scan, handed to the next call
        assert slot is not None and torch.equal(slot, a.abs().amax(1).view(torch.int32))
        rm, cm = fused.operand_maxima(a, rows=True, cols=True)   # one pass: rows and columns
        assert torch.equal(rm, slot) and torch.equal(cm, a.abs().amax(0).view(torch.int32))
        ws = fused._tail_workspace(L, M, N, K, False, a.device)
        assert L.pdgn_gemm_set_operand_scales(ptr(slot), None) == 0
        assert L.pdgn_gemm_nt_ps(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(pl.p), pl.p.shape[2], wp, 2, ptr(bias), None, 0, ptr(c2), N, None,
                                 None, 0, 1, 0, None, 0, stream_of(a)) == 0
        torch.cuda.synchronize()
        del ws
        assert torch.equal(c1, c2) and torch.equal(c0, c1)         # same parts, same products, same order: with or without the planes / the hand-over
        for c in (c0, c1):
            assert torch.isfinite(c).all() and ((c.double() - ref).abs() / mag).max().item() < 1e-6
    # two-part planes run on the 256 x 128 tile whatever the launch model would pick for three parts -- here for 300 rows -- unless
    # the launch emits BatchNorm partials, whose geometry is the pick's
    small = torch.randn(300, K, device="cuda", generator=g)
    cs = torch.empty(300, N, device="cuda")
    if (L.pdgn_gemm_nt_config(ctypes.c_longlong(300), N, K, 1) & 15) != 0:
        assert L.pdgn_gemm_nt_ps(ctypes.c_longlong(300), N, K, ptr(small), K, ptr(pl.p), pl.p.shape[2], wp, 2, None, None, 0, ptr(cs), N, None,
                                 None, 0, 1, 0, None, 0, stream_of(a)) == 0
        refs = small.double() @ w.double().t()
        mags = small.double().abs() @ w.double().abs().t() + 1.0
        assert ((cs.double() - refs).abs() / mags).max().item() < 1e-6
        L.pdgn_gemm_nt_stat_rows.restype = ctypes.c_longlong
        part = torch.empty(L.pdgn_gemm_nt_stat_rows(ctypes.c_longlong(300), N, K), 3 * N, device="cuda")
        assert L.pdgn_gemm_nt_ps(ctypes.c_longlong(300), N, K, ptr(small), K, ptr(pl.p), pl.p.shape[2], wp, 2, None, None, 0, ptr(cs), N, ptr(part),
                                 None, 0, 1, 0, None, 0, stream_of(a)) == -1
        assert fused.planes_fit(pl.p, 300, N, K) and not fused.planes_fit(pl.p, 300, N, K, True)
    # which planes to make: from ~2 GFLOP on when the activations' maxima are free, never for a handful of rows or a short reduction
    assert fused.two_part_planes(17920, 256, 2560, 0) and fused.two_part_planes(35840, 512, 256, 0) and fused.two_part_planes(17920, 6432, 64, 17920 * 64 * 4)
    assert not fused.two_part_planes(17920, 256, 2560, 17920 * 2560 * 4) and not fused.two_part_planes(200, 256, 2560, 0) and not fused.two_part_planes(17920, 256, 16, 0)


@pytest.mark.parametrize("M,N,K", [(35840, 12832, 128), (17920, 6432, 64), (17920, 3232, 32), (9001, 2028, 64), (4099, 4100, 128), (300000, 512, 64)])
def test_row_panel_kernel_of_the_short_reductions(M, N, K):
    """csrc/gemm_rp.hip (round 6): the products with a short reduction and a wide result -- the per-point tap product of a block,
    35840 x 12832 x 128 at stage 4 -- on two-part planes with a plain epilogue run on the row-panel kernel (A resident in registers
    as fragments, weight tiles streamed through LDS, XCD-partitioned).  Same scaling, same split, same three partial products in
    the same order as gemm_x3.hip's two-part form: where pdgn_gemm_nt takes two parts itself the results are bit-identical;
    everywhere against fp64 below 1e-6 of every element's own sum |a||w| -- with the rows of both operands spanning 2^-30 .. 1,
    ragged row / column counts, panels that end inside a workgroup's range."""
    import ctypes
    from pdgn_amd import _lib, fused
    from pdgn_amd._lib import ptr, stream_of
    L = _lib.lib()
    _lib.set_gemm_mode("x2")
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    a = torch.randn(M, K, device="cuda", generator=g) * _spread(M, g)[:, None]
    w = torch.randn(N, K, device="cuda", generator=g) * 0.3 * _spread(N, g)[:, None]
    pl = fused.split_planes(w, False, rows=M, x_maxima_free=True)
    assert pl.parts_p == 2
    L.pdgn_gemm_nt_ps_workspace_floats.restype = ctypes.c_longlong
    assert L.pdgn_gemm_nt_ps_workspace_floats(ctypes.c_longlong(M), N, K, 2, 0) == 0      # (the row-panel kernel: no stream-K tail)
    c = torch.full((M, N), float("nan"), device="cuda")
    wp = ctypes.c_longlong(N * pl.p.shape[2])
    am = fused.operand_maxima(a)
    for hand in (True, False):                                   # A's row maxima handed in / scanned by the call
        c.fill_(float("nan"))
        if hand:
            assert L.pdgn_gemm_set_operand_scales(ptr(am), None) == 0
        assert L.pdgn_gemm_nt_ps(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(pl.p), pl.p.shape[2], wp, 2, None, None, 0, ptr(c), N, None,
                                 None, 0, 1, 0, None, 0, stream_of(a)) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(c).all()
        rows = torch.cat([torch.arange(0, min(M, 3000), device="cuda"), torch.arange(max(0, M - 3000), M, device="cuda")])
        ref = a[rows].double() @ w.double().t()
        mag = (a[rows].double().abs() @ w.double().abs().t()).clamp_min(1e-300)
        assert ((c[rows].double() - ref).abs() / mag).max().item() < 1e-6
    if fused.two_part(M, N, K, 0):                               # the tile kernel's two-part form on the same operands: the same bits
        c0 = torch.empty(M, N, device="cuda")
        wm = fused.operand_maxima(w)
        ws = fused._tail_workspace(L, M, N, K, False, a.device)
        assert L.pdgn_gemm_set_operand_scales(ptr(am), ptr(wm)) == 0
        assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(w), K, None, None, 0, ptr(c0), N, None, stream_of(a)) == 0
        torch.cuda.synchronize()
        del ws
        assert torch.equal(c0, c)
    # through LinearCL: forward on the row-panel kernel, the gradients on the tile kernels
    xg, wg = a.clone().requires_grad_(True), w.clone().requires_grad_(True)
    pl2 = fused.split_planes(w, True, rows=M, dy_maxima_free=True, x_maxima_free=True)
    y = fused.linear_cl(xg, wg, planes=pl2, x_max=am)
    assert torch.equal(y.detach(), c)


@pytest.mark.parametrize("ratio", [0.0, 300.0])
@pytest.mark.parametrize("M,N,K", [(40960, 512, 64), (40999, 516, 64), (179200, 256, 64), (20000, 1024, 128)])
def test_row_panel_kernel_emits_batchnorm_partials(M, N, K, ratio):
    """The row-panel kernel with stat_part (the edge-level layer in front of the bilateral weighting, conv_all.3: 358400 x 512 x 64
    at stage 4): one partial row per 256-row panel of the result (the workgroup's eight waves join their 32-row sums on the panel's
    first row as the pivot) -- sum (x - pv), sum (x - pv)^2, pv --
    through linear_cl(want_stats=True, planes=two-part planes) -> bn_act(partials=...) against fp64: normalised output at 1e-4, also
    with |mean| >> std (ratio: the weight rows get a common offset direction), ragged row / column counts, the result itself equal
    to the call without partials, running statistics."""
    import torch.nn as nn
    from pdgn_amd import _lib, fused
    _lib.set_gemm_mode("x2")
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x = torch.randn(M, K, device="cuda", generator=g) + (1.0 if ratio else 0.0)
    w = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5 + ratio / K
    pl = fused.split_planes(w, False, rows=M, x_maxima_free=True)
    assert pl.parts_p == 2
    y0 = fused.linear_cl(x, w, planes=pl)
    y, part = fused.linear_cl(x, w, None, None, True, planes=pl)
    assert part is not None and part[1] == 256 and part[0].shape == ((M + 255) // 256, 3 * N)
    # the partial rows themselves: sums of (y - pv) and its square over each panel's rows, pv = the panel's first row
    p0 = part[0].double().view(-1, 3, N)
    yp = torch.nn.functional.pad(y.double(), (0, 0, 0, p0.shape[0] * 256 - M)).view(-1, 256, N)
    live = (torch.arange(p0.shape[0] * 256, device="cuda").view(-1, 256, 1) < M).double()
    d = (yp - yp[:, :1]) * live
    assert torch.equal(part[0].view(-1, 3, N)[:, 2], y[::256])
    scale = d.abs().sum(1).max().item()
    assert (p0[:, 0] - d.sum(1)).abs().max().item() < 2e-5 * scale and (p0[:, 1] - (d * d).sum(1)).abs().max().item() < 2e-5 * (d * d).sum(1).max().item()
    assert torch.equal(y, y0)
    bn = nn.BatchNorm1d(N).cuda().train()
    out = fused.bn_act(y, bn, True, act="none", partials=part)
    y64 = y.double()
    want = (y64 - y64.mean(0)) / torch.sqrt(y64.var(0, unbiased=False) + bn.eps)
    err = (out.double() - want).abs().max().item()
    assert err < 1e-4 * max(1.0, want.abs().max().item()), (M, N, K, ratio, err)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), (0.9 + 0.1 * y64.var(0, unbiased=True)).float().cpu().numpy(), rtol=1e-4)
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), (0.1 * y64.mean(0)).float().cpu().numpy(), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("M,N,K", [(17920, 256, 2560), (8960, 128, 1280), (17920, 6432, 64), (17920, 64, 6432), (4100, 132, 260)])
def test_two_part_planes_on_the_big_tile_for_mid_size_products(M, N, K):
    """Two-part planes + handed-in maxima on shapes the launch model gives other tiles for three parts (conv2's dense half and the
    per-point product at stages 2-3, an input gradient with a long reduction, a ragged one): through LinearCL forward and backward
    against fp64, tail workspaces included."""
    from pdgn_amd import _lib, fused
    _lib.set_gemm_mode("x2")
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * 0.2
    add = torch.randn(M, N, device="cuda", generator=g)
    dy = torch.randn(M, N, device="cuda", generator=g)
    pl = fused.split_planes(w, True, rows=M, dy_maxima_free=True, x_maxima_free=True)
    if 2.0 * M * N * K >= 2e9:
        assert pl.parts_p == 2 and pl.parts_t == 2
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = fused.linear_cl(xg, wg, None, add, planes=pl, x_max=fused.operand_maxima(x) if pl.parts_p == 2 else None)
    y.backward(dy)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = x64 @ w64.t() + add.double()
    y64.backward(dy.double())
    for name, got, ref, mag in (("y", y.detach(), y64.detach(), x.double().abs() @ w.double().abs().t() + 1.0),
                                ("dx", xg.grad, x64.grad, dy.double().abs() @ w.double().abs() + 1.0),
                                ("dw", wg.grad, w64.grad, dy.double().abs().t() @ x.double().abs() + 1.0)):
        assert ((got.double() - ref).abs() / mag).max().item() < 2e-6, name


@pytest.mark.parametrize("C", [64, 128, 512])
def test_bilateral_weighting_emits_its_output_maxima(C):
    """want_max: the pass that writes inte = act(BN(u)) * w also leaves the ROW maxima of |inte| as conv2's (M, k C) first operand
    (what the two-part contraction scales it by, row by row) -- the maxima a scan of the result finds, same result as without."""
    import torch.nn as nn
    from pdgn_amd import fused
    M, k = 3000, 10
    g = torch.Generator(device="cuda").manual_seed(9)      # (C / 2 = 32: half a wave per point; 64, 256: whole waves, the stage shapes)
    x = torch.randn(M * k, C, device="cuda", generator=g) * 2
    u = torch.randn(M * k // 2, 2 * C, device="cuda", generator=g) * 50
    bx, bu = nn.BatchNorm2d(C).cuda(), nn.BatchNorm2d(2 * C).cuda()
    y0 = fused.bilateral_weighting(x, bx, u, bu, True, k)
    y1, slot, cslot = fused.bilateral_weighting(x, bx, u, bu, True, k, want_max=True)
    assert torch.equal(y0, y1) and slot.shape == (M,)
    assert cslot is not None and bool((cslot.view(torch.float32) >= y1.view(M, -1).abs().amax(0)).all())      # (the BatchNorm parameters want gradients: a column bound comes along)
    assert torch.equal(slot, y1.view(M, -1).abs().amax(1).view(torch.int32))     # y as the (M, k C) operand of conv2's dense half


@pytest.mark.parametrize("M,C", [(20000, 512), (3000, 128)])
def test_bilateral_weighting_bounds_its_column_maxima_for_the_weight_gradient(M, C):
    """When a backward pass will follow, bilateral_weighting hands conv2's weight gradient (which takes inte transposed and scales it
    column by column) an upper BOUND of inte's column maxima from the BatchNorm parameters alone -- |gamma| sqrt(n - 1) + |beta|:
    never below the true maximum (no scaled value can leave fp16's range), within 2^9 of it, same y; and the two-part weight
    gradient computed with the bound is as accurate against fp64 as with the exact maxima."""
    import ctypes
    import torch.nn as nn
    from pdgn_amd import _lib, fused
    from pdgn_amd._lib import ptr, stream_of
    k = 10
    g = torch.Generator(device="cuda").manual_seed(M + C)
    x = (torch.randn(M * k, C, device="cuda", generator=g) * 2).requires_grad_(True)
    u = (torch.randn(M * k // 2, 2 * C, device="cuda", generator=g) * torch.rand(1, 2 * C, device="cuda", generator=g) * 50).requires_grad_(True)
    bx, bu = nn.BatchNorm2d(C).cuda(), nn.BatchNorm2d(2 * C).cuda()
    with torch.no_grad():
        bu.weight.copy_(torch.randn(2 * C, device="cuda", generator=g))
        bu.bias.copy_(torch.randn(2 * C, device="cuda", generator=g))
    bx0, bu0 = copy.deepcopy(bx), copy.deepcopy(bu)
    with torch.no_grad():
        y0 = fused.bilateral_weighting(x, bx0, u, bu0, True, k)
    y1, rmax, cmax = fused.bilateral_weighting(x, bx, u, bu, True, k, want_max=True)
    assert torch.equal(y0, y1.detach())
    assert torch.equal(rmax, y1.detach().view(M, -1).abs().amax(1).view(torch.int32))
    true = y1.detach().view(M, -1).abs().amax(0)
    bound = cmax.view(torch.float32)
    # (never below; and not absurdly above: sqrt(n) / (the ~4.5 sigma a column reaches x the softmax weight of its largest entry):
    # 2^7 .. 2^11 here -- of the 16 binades over which a value keeps 22 bits, 5 .. 9 remain, and the dW check below says what that costs)
    assert cmax.shape == (k * C,) and bool((bound >= true).all()) and bool((bound <= true.clamp_min(1e-30) * 65536).all()), \
        float((bound / true.clamp_min(1e-30)).max())
    if M < 10000:
        return
    # the weight gradient dW = dOut^T inte on two parts with the bound / with the exact column maxima, against fp64
    L = _lib.lib()
    _lib.set_gemm_mode("x2")
    N = 512
    X = y1.detach().view(M, k * C)
    dO = torch.randn(M, N, device="cuda", generator=g)
    ref = dO.double().t() @ X.double()
    mag = dO.double().abs().t() @ X.double().abs()
    errs = []
    cd = fused.operand_maxima(dO, rows=False, cols=True)
    for cx in (cmax, fused.operand_maxima(X, rows=False, cols=True)):
        dW = torch.empty(N, k * C, device="cuda")
        assert L.pdgn_gemm_set_operand_scales(ptr(cd), ptr(cx)) == 0
        assert L.pdgn_gemm_tn_big(ctypes.c_longlong(M), N, k * C, ptr(dO), N, ptr(X), k * C, ptr(dW), 0, stream_of(dO)) == 0
        errs.append(((dW.double() - ref).abs() / mag.clamp_min(1e-300)).max().item())
    print('dW error with the bound / with exact column maxima:', errs, 'bound / true max up to', float((bound / true.clamp_min(1e-30)).max()))
    assert errs[0] < 1e-6 and errs[0] <= 1.25 * errs[1] + 2e-8, errs


@pytest.mark.parametrize("B,N,k,specs", [(3, 300, 10, ((6, 5, 16, 0, 96), (10, 1, 8, 112, 192), (1, 10, 4, 200, 204))),
                                         (2, 1024, 10, ((6, 5, 128, 0, 768), (10, 1, 64, 896, 1536)))])
def test_gather_sum_adjoint_leaves_the_maxima_of_dy(B, N, k, specs):
    """The kernels that WRITE dY (one call per spec into the same tensor) collect the ROW maxima of |dY| in one array, the first
    call zero-filling it: the maxima a scan of the finished dY finds -- both kernel forms (the per-wave task kernel for the
    large specs, the per-element one for the small) -- and dY itself is unchanged."""
    import ctypes
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    from pdgn_amd.deconv import transposed_graph
    L = _lib.lib()
    ldy = sum(T * C + (C if offc >= 0 else 0) for (T, P, C, off, offc) in specs)
    g = torch.Generator(device="cuda").manual_seed(N + ldy)
    idx = torch.randint(0, N, (B, N, k), device="cuda", generator=g, dtype=torch.int32)
    idx[:, :, 0] = 3
    rowptr, edges = transposed_graph(idx)
    douts = [torch.randn(B, N, P, C, device="cuda", generator=g) * (10.0 ** i) for i, (T, P, C, off, offc) in enumerate(specs)]
    res = []
    for slot in (None, torch.full((B * N,), 7, dtype=torch.int32, device="cuda")):     # (garbage in the array: the first call clears it)
        dY = torch.full((B, N, ldy), float("nan"), device="cuda")
        for i, ((T, P, C, off, offc), dout) in enumerate(zip(specs, douts)):
            assert L.pdgn_window_gather_sum_backward_csr(B, N, k, ldy, T, P, C, off, offc, ptr(dout), ptr(rowptr), ptr(edges), ptr(dY),
                                                         ptr(slot), 1 if i == 0 else 0, stream_of(dY)) == 0
        res.append(dY)
    assert torch.equal(res[0], res[1]) and torch.isfinite(res[1]).all()
    assert torch.equal(slot, res[1].view(B * N, ldy).abs().amax(1).view(torch.int32))


def test_handovers_belong_to_the_next_call_only():
    """A tail workspace and operand maxima handed over for "the next contraction call" are consumed by THAT call even when it is
    refused: a later call must not pick them up.  Here the refused call gets maxima of zero (exponent 126: every product would
    overflow) and a workspace that is then freed; the valid call after it scans its operands itself and is right."""
    import ctypes
    from pdgn_amd import _lib, fused
    from pdgn_amd._lib import ptr, stream_of
    L = _lib.lib()
    _lib.set_gemm_mode("x2")
    M, N, K = 20000, 512, 2560
    g = torch.Generator(device="cuda").manual_seed(11)
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g)
    c = torch.empty(M, N, device="cuda")
    zeros = torch.zeros(M, dtype=torch.int32, device="cuda")
    ws = fused._tail_workspace(L, M, N, K, False, a.device)
    assert L.pdgn_gemm_set_operand_scales(ptr(zeros), ptr(zeros)) == 0
    assert L.pdgn_gemm_nt(ctypes.c_longlong(M), 3, K, ptr(a), K, ptr(w), K, None, None, 0, ptr(c), N, None, stream_of(a)) == -1     # n % 4: refused
    del ws
    assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(w), K, None, None, 0, ptr(c), N, None, stream_of(a)) == 0
    ref = a.double() @ w.double().t()
    mag = a.double().abs() @ w.double().abs().t()
    assert torch.isfinite(c).all() and ((c.double() - ref).abs() / mag).max().item() < 1e-6
    # ... and handed-over maxima ARE used by the call they are meant for (zero maxima: the scaled operands overflow fp16)
    assert L.pdgn_gemm_set_operand_scales(ptr(zeros), ptr(zeros)) == 0
    assert L.pdgn_gemm_nt(ctypes.c_longlong(M), N, K, ptr(a), K, ptr(w), K, None, None, 0, ptr(c), N, None, stream_of(a)) == 0
    assert not torch.isfinite(c).all()


@pytest.mark.parametrize("M,N,K", [(35840, 512, 5120), (35840, 12832, 128), (17920, 256, 2560), (40000, 128, 64), (100003, 132, 68)])
def test_weight_gradient_slices_without_atomics(M, N, K):
    """pdgn_gemm_tn_big with a workspace (pdgn_gemm_tn_big_workspace_floats + pdgn_gemm_set_tail_workspace): the k slices' partial tiles
    are summed by the reduce kernel in slice order -- against fp64, against the atomic form, bit-identical from run to run, dW not
    zero-filled by anyone (poisoned with NaN here)."""
    import ctypes
    from pdgn_amd import _lib
    from pdgn_amd._lib import ptr, stream_of
    L = _lib.lib()
    L.pdgn_gemm_tn_big_workspace_floats.restype = ctypes.c_longlong
    need = L.pdgn_gemm_tn_big_workspace_floats(ctypes.c_longlong(M), N, K)
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x = torch.randn(M, K, device="cuda", generator=g)
    dy = torch.randn(M, N, device="cuda", generator=g)
    rows = min(M, 20000)
    ref = dy[:rows].double().t() @ x[:rows].double()
    mag = dy[:rows].double().abs().t() @ x[:rows].double().abs() + 1.0

    def run(with_ws, m):
        dw = torch.full((N, K), float("nan"), device="cuda")
        n_ = L.pdgn_gemm_tn_big_workspace_floats(ctypes.c_longlong(m), N, K)
        ws = torch.empty(max(n_, 1), device="cuda")
        if with_ws and n_:
            assert L.pdgn_gemm_set_tail_workspace(ptr(ws), ctypes.c_longlong(n_)) == 0
        assert L.pdgn_gemm_tn_big(ctypes.c_longlong(m), N, K, ptr(dy), N, ptr(x), K, ptr(dw), 0, stream_of(dy)) == 0
        torch.cuda.synchronize()
        return dw
    a, b, c = run(True, rows), run(True, rows), run(False, rows)
    assert ((a.double() - ref).abs() / mag).max().item() < 1e-6 and ((c.double() - ref).abs() / mag).max().item() < 1e-6
    if need:
        assert torch.equal(a, b), "slices summed in a fixed order"
    full = run(True, M)
    assert torch.isfinite(full).all()
