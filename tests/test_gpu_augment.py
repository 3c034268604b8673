"""GPU: the discriminator augmentation -- the three entry points of csrc/augment.hip called directly on guard-banded buffers against
the numpy mirror (tests/augment_mirror.py), AugmentRows' gradient, and the trainer: twelve call sites, the clock under eager steps,
the launch list and fit, set_augment in place, and the command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_mirror as am

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                                                       # floats on either side of every output (a multiple of 4: 16-byte alignment kept)
SENTINEL = -12345.0
EPS = float(np.finfo(np.float32).eps)
EVERYTHING = dict(p=1.0, rot_max_deg=180.0, scale_max=1.25, flip=True, trans_max=0.1, jitter_sigma=0.0)
# B, N, floats the bases are shifted by (1: no 16-byte alignment -> the element-wise path), the cloud stored point-major (a (B,3,N) view
# of (B,N,3) rows, as the generator's clouds are)
SHAPES = [(3, 5, 0, 0), (2, 256, 0, 0), (2, 256, 1, 0), (35, 2048, 0, 0), (3, 5, 0, 1), (2, 256, 0, 1), (2, 256, 1, 1), (35, 2048, 0, 1)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _guarded(shape, dev, shift=0):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=torch.float32, device=dev)
    return whole[GUARD + shift:GUARD + shift + n].view(shape), whole, shift


def _intact(whole, shift):
    return bool((whole[:GUARD + shift] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def _table(dev, **params):
    from pdgn_amd import augment
    words = augment.table_words(augment.validate(**dict(augment.DEFAULTS, **params)))
    return torch.from_numpy(words.view(np.int32).copy()).to(dev), augment.decode_table(words)


def _clock(dev, t):
    """A clock word under which launches draw at t (the clock counts the iterations begun: t + 1)."""
    return torch.tensor([t + 1], dtype=torch.int64, device=dev)


def _x(B, N, dev, shift=0, seed=0, pm=0):
    """(host (B,3,N), device (B,3,N)): the device tensor contiguous, or with pm a view of point-major (B,N,3) memory."""
    host = np.random.default_rng(seed).standard_normal((B, 3, N)).astype(np.float32)
    whole = torch.zeros(B * 3 * N + 4 + shift, dtype=torch.float32, device=dev)
    flat = whole[shift:shift + B * 3 * N]
    x = flat.view(B, N, 3).transpose(1, 2) if pm else flat.view(B, 3, N)
    x.copy_(torch.from_numpy(host))
    return host, x


def _fwd(x, table, clock, seed, row0, tag, shift=0, affine=True, pm=0):
    """pdgn_augment_rows_fwd itself on guard-banded outputs -> (rc, rows (B*N,3), affine (B,12) or None) as numpy."""
    from pdgn_amd import _lib
    B, _, N = x.shape
    rows, rows_whole, rs = _guarded((B * N, 3), x.device, shift)
    aff, aff_whole, fs = _guarded((B, 12), x.device) if affine else (None, None, 0)
    assert (x.transpose(1, 2) if pm else x).is_contiguous()
    rc = _lib.lib().pdgn_augment_rows_fwd(B, N, _lib.ptr(x), pm, _lib.ptr(rows), _lib.ptr(aff), _lib.ptr(table), _lib.ptr(clock),
                                          ctypes.c_ulonglong(seed), ctypes.c_longlong(row0), tag, _lib.stream_of(x))
    torch.cuda.synchronize()
    assert _intact(rows_whole, rs) and (aff is None or _intact(aff_whole, fs))
    if rc == 0:
        assert not bool((rows == SENTINEL).any()) and (aff is None or not bool((aff == SENTINEL).any()))    # every element written
    return rc, rows.cpu().numpy(), None if aff is None else aff.cpu().numpy()


def _bwd(d_rows, B, N, table, clock, seed, row0, tag, shift=0, pm=0):
    """-> (rc, dx as a logical (B,3,N) numpy array)."""
    from pdgn_amd import _lib
    dx, whole, s = _guarded((B, N, 3) if pm else (B, 3, N), d_rows.device, shift)
    rc = _lib.lib().pdgn_augment_rows_bwd(B, N, _lib.ptr(d_rows), _lib.ptr(dx), pm, _lib.ptr(table), _lib.ptr(clock), ctypes.c_ulonglong(seed),
                                          ctypes.c_longlong(row0), tag, _lib.stream_of(d_rows))
    torch.cuda.synchronize()
    assert _intact(whole, s)
    if rc == 0:
        assert not bool((dx == SENTINEL).any())
    return rc, np.ascontiguousarray((dx.transpose(1, 2) if pm else dx).cpu().numpy())


def _decisions_of(aff, tab):
    """flip, rotation, scale, translation as they can be read off an affine map (B,12) drawn with every range non-zero."""
    a = aff[:, :9].reshape(-1, 3, 3).astype(np.float64)
    u = tab["up_axis"]
    return np.stack([np.linalg.det(a) < 0,                       # the mirror
                     a[:, (u + 1) % 3, (u + 2) % 3] != 0,         # -s sin(theta): zero without a rotation
                     a[:, u, u] != 1.0,                           # s on the fixed axis
                     (aff[:, 9:] != 0).any(axis=1)], axis=1)


# An affine map against the fp64 mirror where the sample is too small for the 4x rule's maximum to mean much (a handful of maps): an
# entry is fl(s * r) with |r| <= 1, s <= scale_max; sincosf and expf within 2 ulp each (2 eps absolute on r, 2 eps relative on s), the
# angle rot_max * v rounded once in fp32 (pi eps / 2 = 1.6 eps absolute on r), the product eps / 2: below 6.1 eps scale_max; 8 leaves
# a margin.  Any other draw differs in the first digits.
MAP_TOL = 8 * EPS * EVERYTHING["scale_max"]


# ---------------------------------------------------------------------------- kernel level
def test_affine_against_fp64():
    """affine_out over 32 clocks of B = 35 (1120 maps, every component enabled) against the fp64 mirror; the bound is 4x the largest
    deviation of the fp32 numpy evaluation on the same words.  Measured on an MI355X (ROCm 7.2): profiles/aug_check.txt."""
    dev = _dev()
    B, N, seed, tag = 35, 8, 2024, am.tag(0, "gen")
    _, x = _x(B, N, dev)
    table, tab = _table(dev, **EVERYTHING)
    got = np.concatenate([_fwd(x, table, _clock(dev, t), seed, 0, tag)[2] for t in range(32)])
    want = np.concatenate([am.affine(tab, seed, t, np.arange(B), tag, np.float64) for t in range(32)])
    host32 = np.concatenate([am.affine(tab, seed, t, np.arange(B), tag, np.float32) for t in range(32)])
    host_dev, device_dev = np.abs(host32.astype(np.float64) - want).max(), np.abs(got.astype(np.float64) - want).max()
    print("augment affine: device max |a - fp64| = %.3e, numpy fp32 = %.3e, bound = %.3e over %d values" % (device_dev, host_dev, 4 * host_dev, got.size))
    assert got.shape == (32 * 35, 12) and device_dev <= 4 * host_dev, (device_dev, host_dev)
    assert device_dev <= MAP_TOL


@pytest.mark.parametrize("B,N,shift,pm", SHAPES)
def test_forward_is_the_fp32_evaluation_of_its_own_affine_and_the_affine_is_the_mirrors(B, N, shift, pm):
    dev = _dev()
    seed, t, tag = 9999, 12, am.tag(1, "fake")
    host, x = _x(B, N, dev, shift, pm=pm)
    table, tab = _table(dev, **dict(EVERYTHING, p=0.5))
    rc, rows, aff = _fwd(x, table, _clock(dev, t), seed, 0, tag, shift, pm=pm)
    assert rc == 0
    want_on = am.decisions(tab, seed, t, np.arange(B), tag)
    assert np.array_equal(_decisions_of(aff, tab), want_on[:, :4])                 # enabled components: exactly the mirror's
    assert np.abs(aff - am.affine(tab, seed, t, np.arange(B), tag)).max() <= MAP_TOL     # (the tight bound: test_affine_against_fp64)
    assert np.array_equal(rows.view(np.uint32), am.rows_fp32(aff, host).view(np.uint32))      # sigma = 0: bit for bit
    _, rows2, none = _fwd(x, table, _clock(dev, t), seed, 0, tag, shift, affine=False, pm=pm)        # without affine_out: the same rows
    assert none is None and np.array_equal(rows.view(np.uint32), rows2.view(np.uint32))


@pytest.mark.parametrize("B,N,shift,pm", SHAPES)
def test_p_zero_is_the_transpose(B, N, shift, pm):
    dev = _dev()
    host, x = _x(B, N, dev, shift, pm=pm)
    table, _ = _table(dev, **dict(EVERYTHING, p=0.0, jitter_sigma=0.05))
    rc, rows, aff = _fwd(x, table, _clock(dev, 3), 1, 0, am.tag(0, "real"), shift, pm=pm)
    assert rc == 0
    assert np.array_equal(aff, np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]).astype(np.float32), (B, 1)))
    assert np.array_equal(rows, x.transpose(1, 2).reshape(B * N, 3).cpu().numpy())
    assert np.array_equal(rows, host.transpose(0, 2, 1).reshape(B * N, 3))


@pytest.mark.parametrize("B,N,shift,pm", SHAPES)
def test_backward_is_the_fp32_evaluation_of_the_transposed_affine(B, N, shift, pm):
    dev = _dev()
    seed, t, tag = 5, 1 << 33, am.tag(3, "gen")
    host, x = _x(B, N, dev, shift, pm=pm)
    table, tab = _table(dev, **EVERYTHING)
    clock = _clock(dev, t)
    _, _, aff = _fwd(x, table, clock, seed, 0, tag, shift, pm=pm)
    dy_host = np.random.default_rng(1).standard_normal((B * N, 3)).astype(np.float32)
    whole = torch.zeros(B * N * 3 + 4 + shift, dtype=torch.float32, device=dev)
    dy = whole[shift:shift + B * N * 3].view(B * N, 3)
    dy.copy_(torch.from_numpy(dy_host))
    rc, dx = _bwd(dy, B, N, table, clock, seed, 0, tag, shift, pm=pm)
    assert rc == 0
    assert np.array_equal(dx.view(np.uint32), am.grad_fp32(aff, dy_host, B, N).view(np.uint32))


def test_a_rank_draws_its_global_rows():
    dev = _dev()
    seed, t, tag, N = 31, 7, am.tag(2, "real"), 256
    host, x = _x(8, N, dev)
    table, _ = _table(dev, **dict(EVERYTHING, jitter_sigma=0.02))
    _, rows8, aff8 = _fwd(x, table, _clock(dev, t), seed, 0, tag)                   # one rank at B = 8
    _, rows4, aff4 = _fwd(x[4:].contiguous(), table, _clock(dev, t), seed, 4, tag)  # rank 1 of 2 at B = 4: row0 = rank * B
    assert np.array_equal(aff4.view(np.uint32), aff8[4:].view(np.uint32))
    assert np.array_equal(rows4.view(np.uint32), rows8[4 * N:].view(np.uint32))


def test_jitter_against_fp64_and_its_moments():
    """rows(sigma) - rows(sigma = 0), same draws otherwise, against the fp64 mirror's normals.  The device forms fl(o + j): the fp32
    host evaluation of the same formula is fl(o + j32) - o with the device's own sigma = 0 rows o, and the bound 4x ITS largest
    deviation from the fp64 normals (test_noise_against_fp64_and_its_moments' rule and factor)."""
    dev = _dev()
    B, N, sigma, seed, t, tag = 35, 2048, 0.02, 2024, 40, am.tag(3, "fake")
    host, x = _x(B, N, dev)
    off, _ = _table(dev, **EVERYTHING)
    on, tab = _table(dev, **dict(EVERYTHING, jitter_sigma=sigma))
    _, rows0, aff0 = _fwd(x, off, _clock(dev, t), seed, 0, tag)
    _, rows1, aff1 = _fwd(x, on, _clock(dev, t), seed, 0, tag)
    assert np.array_equal(aff0.view(np.uint32), aff1.view(np.uint32))
    want = am.jitter(tab, seed, t, np.arange(B), tag, N, np.float64).reshape(B * N, 3)
    j32 = am.jitter(tab, seed, t, np.arange(B), tag, N, np.float32).reshape(B * N, 3)
    got = rows1.astype(np.float64) - rows0.astype(np.float64)
    host32 = (rows0 + j32).astype(np.float64) - rows0.astype(np.float64)
    host_dev, device_dev = np.abs(host32 - want).max(), np.abs(got - want).max()
    print("augment jitter: device max |d - fp64| = %.3e, numpy fp32 = %.3e, bound = %.3e over %d samples" % (device_dev, host_dev, 4 * host_dev, got.size))
    assert device_dev <= 4 * host_dev, (device_dev, host_dev)
    n = got.size
    mean, std = got.mean(), got.std()
    print("augment jitter: mean %+.3e (5 s.e. %.3e), std %.6f (sigma %.2f, 5 s.e. %.3e), n = %d"
          % (mean, 5 * sigma / np.sqrt(n), std, sigma, 5 * sigma / np.sqrt(2 * n), n))
    assert n == 35 * 2048 * 3
    assert abs(mean) <= 5 * sigma / np.sqrt(n) and abs(std - sigma) <= 5 * sigma / np.sqrt(2 * n)
    # p = 0.5: the samples the mirror leaves alone are left alone, bit for bit
    half, tab_half = _table(dev, **dict(EVERYTHING, p=0.5, jitter_sigma=sigma))
    _, rows_h, aff_h = _fwd(x, half, _clock(dev, t), seed, 0, tag)
    jit_on = am.decisions(tab_half, seed, t, np.arange(B), tag)[:, 4]
    plain = am.rows_fp32(aff_h, host).reshape(B, N, 3)
    same = (rows_h.reshape(B, N, 3).view(np.uint32) == plain.view(np.uint32)).all(axis=(1, 2))
    assert 0 < jit_on.sum() < B and np.array_equal(same, ~jit_on)


def test_draws_are_a_pure_function_of_seed_clock_row_and_tag():
    dev = _dev()
    B, N = 4, 256
    _, x = _x(B, N, dev)
    table, _ = _table(dev, **EVERYTHING)
    base = dict(seed=5, t=11, row0=0, tag=am.tag(0, "real"))
    run = lambda **kw: _fwd(x, table, _clock(dev, dict(base, **kw)["t"]), dict(base, **kw)["seed"], dict(base, **kw)["row0"], dict(base, **kw)["tag"])
    rc, rows_a, aff_a = run()
    _, rows_b, aff_b = run()
    assert rc == 0 and np.array_equal(aff_a.view(np.uint32), aff_b.view(np.uint32)) and np.array_equal(rows_a.view(np.uint32), rows_b.view(np.uint32))
    for change in (dict(seed=6), dict(seed=5 + (1 << 32)), dict(t=12), dict(t=11 + (1 << 32)), dict(row0=1 << 20), dict(tag=am.tag(0, "fake")),
                   dict(tag=am.tag(1, "real"))):
        _, _, aff_c = run(**change)
        assert (aff_c != aff_a).any(axis=1).all(), change                          # every sample's map changes
    _, _, shifted = run(row0=1)                                                     # row0 + b is the counter word: rows slide
    assert np.array_equal(shifted[:-1].view(np.uint32), aff_a[1:].view(np.uint32))
    # the tick: one launch, clock + 1; then the launches draw one later
    from pdgn_amd import _lib
    clock = _clock(dev, 11)
    assert _lib.lib().pdgn_augment_tick(_lib.ptr(clock), _lib.stream_of(clock)) == 0
    assert clock.item() == 13
    _, _, aff_t = _fwd(x, table, clock, 5, 0, am.tag(0, "real"))
    assert np.array_equal(aff_t.view(np.uint32), run(t=12)[2].view(np.uint32))
    # host-side refusals, with real pointers
    assert _fwd(x, table, clock, 5, 0, 5)[0] == -1                                 # a feeder tag
    assert _fwd(x, table, clock, 5, 0, am.TAG_BASE + 12)[0] == -1
    assert _fwd(x, table, clock, 5, (1 << 32) - 1, am.tag(0, "real"))[0] == -1
    assert _fwd(x, table, clock, 5, -1, am.tag(0, "real"))[0] == -1


@pytest.mark.parametrize("pm", [0, 1])
def test_autograd_through_augment_rows_against_fp64(pm):
    """torch.autograd.grad through AugmentRows against an fp64 torch evaluation of the mirror's map.  Bound per point n of sample b:
    |dx[b,:,n] - ref| <= 8 eps ||A_b||_F ||dy[b*N+n]||.  dx_j = sum_i A_ij dy_i has three products and two sums: at most
    (1/2 + 1) eps sum_i |A_ij dy_i| of rounding; the device's A itself is within ~4 eps ||A_:j|| of the fp64 one (the angle
    rot_max * v rounded once: pi eps / 2 absolute, which moves cos and sin by as much; sincosf, expf and the product s * r about
    an eps / 2 .. eps each, relative to s = ||A_:j||).  With Cauchy-Schwarz that is 5.6 eps ||A_:j|| ||dy||; 8 with ||A||_F >= ||A_:j||
    leaves the libm room."""
    from pdgn_amd.augment import Augment
    dev = _dev()
    B, N, seed = 3, 37, 77
    aug = Augment(seed=seed, record=True, device=dev, **EVERYTHING)
    aug.set_clock(20)
    aug.tick()                                                   # draws at t = 20
    host = np.random.default_rng(2).standard_normal((B, 3, N)).astype(np.float32)
    leaf = torch.from_numpy(np.ascontiguousarray(host.transpose(0, 2, 1)) if pm else host).to(dev).requires_grad_(True)
    x = leaf.transpose(1, 2) if pm else leaf                     # pm: a (B,3,N) view of point-major rows, as the generator's clouds are
    rows = aug.rows(x, 2, "gen")
    assert rows.shape == (B * N, 3) and rows.requires_grad
    dy = torch.from_numpy(np.random.default_rng(3).standard_normal((B * N, 3)).astype(np.float32)).to(dev)
    (dx,) = torch.autograd.grad(rows, x, dy)
    assert dx.shape == (B, 3, N) and dx.stride() == x.stride()
    st = aug.state()
    assert st["clock"] == 21
    tab = st["params"]
    A64 = torch.from_numpy(am.affine(tab, seed, 20, np.arange(B), am.tag(2, "gen"))).to(dev)
    x64 = x.detach().double().requires_grad_(True)
    ref_rows = torch.einsum("bij,bjn->bni", A64[:, :9].view(B, 3, 3), x64) + A64[:, None, 9:]
    (ref,) = torch.autograd.grad(ref_rows.reshape(B * N, 3), x64, dy.double())
    err = (dx.double() - ref).norm(dim=1)                                          # (B, N)
    bound = 8 * EPS * A64[:, :9].norm(dim=1)[:, None] * dy.double().view(B, N, 3).norm(dim=2)
    print("augment autograd: max err / (eps ||A|| ||dy||) = %.3f (bound 8)" % (err / (bound / 8)).max().item())
    assert bool((err <= bound).all())
    assert np.abs(rows.detach().double().cpu().numpy() - ref_rows.detach().reshape(B * N, 3).cpu().numpy()).max() < 1e-5
    assert np.abs(st["records"][3 * 2 + 2] - A64.cpu().numpy()).max() <= MAP_TOL and not st["records"][:8].any()      # this site's row, and only it
    # a cloud that needs no gradient gets none, and no backward launch
    assert not aug.rows(x.detach(), 0, "real").requires_grad


# ---------------------------------------------------------------------------- trainer level
SEED = 4242


def _trainer(dev, augment):
    from pdgn_amd.trainer import PDGNTrainer
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False, augment=augment)
    tr.train()
    return tr


def _inputs(dev, B=4):
    from pdgn_amd.trainer import noise, synthetic_batch
    g = torch.Generator().manual_seed(1)
    return synthetic_batch(B, dev), noise(B, dev, generator=g), noise(B, dev, generator=g)


def _records_are_the_mirrors(records, tab, t, B=4):
    """All twelve sites at once, each against the mirror at ITS tag and this t (MAP_TOL: 48 maps are no sample for the 4x rule)."""
    assert records.shape == (12, B, 12)
    want = np.stack([am.affine(tab, SEED, t, np.arange(B), am.tag(n, r), np.float64) for n in range(4) for r in am.ROLES])
    assert np.abs(records - want).max() <= MAP_TOL, (t, np.abs(records - want).max())
    assert np.array_equal(records == 0, want == 0)                                  # the entries no component touches


def test_one_eager_step_draws_at_twelve_sites_and_advances_the_clock():
    dev = _dev()
    tr = _trainer(dev, dict(EVERYTHING, seed=SEED, record=True))
    assert tr.aug_state()["clock"] == 0 and tr.aug_state()["records"] is None
    tr.aug.set_clock(5)
    out = tr.step(*_inputs(dev))
    st = tr.aug_state()
    assert st["clock"] == 6                                                        # one tick
    assert all(np.isfinite(v.item()) for v in out.values()) and len(out) == 6
    rec = st["records"]
    _records_are_the_mirrors(rec, st["params"], 5)
    flat = rec.reshape(12, -1)
    assert all((flat[a] != flat[b]).any() for a in range(12) for b in range(a + 1, 12))     # twelve different draws
    assert all((rec[s, a] != rec[s, b]).any() for s in range(12) for a in range(4) for b in range(a + 1, 4))


def test_the_launch_list_follows_the_clock_and_the_table_with_no_host_value():
    dev = _dev()
    tr = _trainer(dev, dict(EVERYTHING, seed=SEED, record=True))
    reals, z1, z2 = _inputs(dev)
    tr.capture_list(reals, z1, z2)
    the_list = tr._list
    c = tr.aug_state()["clock"]
    assert c >= 1                                                                  # the warm-up and the capture's own iterations ticked
    tr.step_list()
    first = tr.aug_state()
    tr.step_list()
    second = tr.aug_state()
    assert (first["clock"], second["clock"]) == (c + 1, c + 2)
    _records_are_the_mirrors(first["records"], first["params"], c)
    _records_are_the_mirrors(second["records"], second["params"], c + 1)
    assert (first["records"].reshape(12 * 4, 12) != second["records"].reshape(12 * 4, 12)).any(axis=1).all()
    # the eager step at the same clock draws the same bits
    tr.aug.set_clock(c)
    tr.step(reals, z1, z2)
    again = tr.aug_state()
    assert again["clock"] == c + 1 and np.array_equal(again["records"].view(np.uint32), first["records"].view(np.uint32))
    # the table, overwritten in place: the same list object, no recapture
    table_ptr = tr.aug.table.data_ptr()
    tr.set_augment(p=0.0)
    out = tr.step_list()
    off = tr.aug_state()
    assert tr._list is the_list and tr.aug.table.data_ptr() == table_ptr and off["clock"] == c + 2
    identity = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]).astype(np.float32)
    assert np.array_equal(off["records"], np.broadcast_to(identity, (12, 4, 12)))
    assert len(out) == 6 and all(np.isfinite(v.item()) for v in out.values())
    assert off["params"]["thr_rot"] == 0 and first["params"]["thr_rot"] == 1 << 24
    with pytest.raises(ValueError):
        tr.set_augment(p=2.0)
    with pytest.raises(ValueError):
        tr.set_augment(sigma=0.1)                                                  # not a parameter's name
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def test_p_zero_is_the_unaugmented_trainer_and_no_augment_is_no_state():
    """The bound is the project's list-versus-eager one, 2e-3 * max(1, |.|) (tests/test_gpu_feed.py:243)."""
    dev = _dev()
    plain, zero = _trainer(dev, None), _trainer(dev, dict(EVERYTHING, p=0.0, seed=SEED))
    assert plain.aug is None and not any(hasattr(plain, a) for a in ("aug_table", "aug_clock", "aug_records", "table", "clock", "records"))
    for call in (lambda: plain.set_augment(p=0.5), plain.aug_state):
        with pytest.raises(RuntimeError):
            call()
    reals, z1, z2 = _inputs(dev)
    want = {k: v.item() for k, v in plain.step(reals, z1, z2).items()}
    got = {k: v.item() for k, v in zero.step(reals, z1, z2).items()}
    assert set(got) == set(want) and len(want) == 6
    for k in want:
        print("p = 0 against no augmentation: %s %.8f / %.8f" % (k, got[k], want[k]))
        assert abs(got[k] - want[k]) <= 2e-3 * max(1.0, abs(want[k])), (k, got[k], want[k])
    # the discriminator's forward: without a site it is the code it was, with one at p = 0 the same numbers
    D = plain.D[0].eval()
    with torch.no_grad():
        a, b, c = D(reals[0]), D(reals[0], None), D(reals[0], zero.aug.at(0, "real"))
    assert torch.equal(a, b) and torch.allclose(a, c, rtol=1e-5, atol=1e-6)


def test_fit_sets_the_clock_and_a_resumed_epoch_draws_what_the_uninterrupted_run_drew():
    """Draws only: trajectories are not bit-reproducible and nothing here claims they are."""
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    B, N, sizes = 4, 2048, (256, 512, 1024)
    clouds = torch.from_numpy(np.random.default_rng(4).standard_normal((2 * B + 1, N, 3)).astype(np.float32)).to(dev)
    feeder = lambda: BatchFeeder(clouds, B, sizes, seed=31)
    assert feeder().batches_per_epoch == 2
    whole = _trainer(dev, dict(EVERYTHING, seed=SEED, record=True))
    assert whole.fit(feeder(), 2) == 2                                             # launch list: its warm-up iterations tick too
    a = whole.aug_state()
    assert a["clock"] == 4
    _records_are_the_mirrors(a["records"], a["params"], 3)                         # epoch 2, batch 1: (2 - 1) * 2 + 1
    whole._list, whole._list_points, whole._static = None, [], None
    resumed = _trainer(dev, dict(EVERYTHING, seed=SEED, record=True))
    assert resumed.fit(feeder(), 2, start_epoch=2, issue="eager") == 2
    b = resumed.aug_state()
    assert b["clock"] == 4 and np.array_equal(a["records"].view(np.uint32), b["records"].view(np.uint32))
    torch.cuda.synchronize()


def test_cli_trains_with_d_augment(tmp_path):
    from pdgn_amd.data import cate_to_synsetid
    rng = np.random.default_rng(5)
    sid = cate_to_synsetid["chair"]
    np.savez(tmp_path / "toy.npz", **{"%s/%s" % (sid, sp): rng.standard_normal((n, 2048, 3)).astype(np.float32)
                                      for sp, n in (("train", 9), ("val", 2), ("test", 6))})
    cmd = [sys.executable, "-m", "pdgn_amd.train", "--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root",
           str(tmp_path / "toy.npz"), "--choice", "chair", "--batch_size", "4", "--seed", "1", "--save_dir", str(tmp_path / "res"),
           "--phase", "train", "--max_epoch", "1", "--snapshot", "1", "--d_augment", "0.5"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    log = (tmp_path / "ck" / "toy" / "log_info.txt").read_text().splitlines()
    assert "d_augment=0.5" in log[0]
    lines = [l for l in log if l.startswith("Epoch: [ 1]")]
    assert len(lines) == 2                                                         # 9 clouds, batches of 4
    for line in lines:
        vals = [float(tok.rstrip(",")) for tok in line.split("time:")[1].split()[2:][1::2]]
        assert len(vals) == 6 and all(np.isfinite(v) for v in vals), line
