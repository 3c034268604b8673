"""GPU: the adaptive discriminator augmentation -- pdgn_mse_const_count and pdgn_augment_tick_ada called
directly against the numpy restatement (tests/ada_mirror.py), the composition over ranks, and the trainer: no launch added, the
threshold's identity per update, set_augment in place, pinned adaptivity, persistence, fit's aug.csv and the command line."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ada_mirror as ada

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SENTINEL_F, SENTINEL_I = -12345.0, -777
ONE = 1 << 24
SEED = 4242
EVERYTHING = dict(rot_max_deg=180.0, scale_max=1.25, flip=True, trans_max=0.1, jitter_sigma=0.0)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _scores(n, seed, specials=True):
    """fp32 scores around the boundary; with `specials` the leading ones are 0.5 itself, its two fp32 neighbours, +-inf and NaN
    (as many as n has room for)."""
    x = np.random.default_rng(seed).normal(0.5, 0.3, n).astype(np.float32)
    if specials:
        h = np.float32(0.5)
        sp = np.array([h, np.nextafter(h, np.float32(1)), np.nextafter(h, np.float32(0)), np.inf, -np.inf, np.nan], dtype=np.float32)
        x[:min(n, sp.size)] = sp[:min(n, sp.size)]
    return x


def _count_call(x, target, scale, dev, prefill=None):
    """pdgn_mse_const_count itself on guard-banded `out` and slot -> (out bits, the slot's four words)."""
    from pdgn_amd import _lib
    out_whole = torch.full((2 * GUARD + 1,), SENTINEL_F, dtype=torch.float32, device=dev)
    slot_whole = torch.full((2 * GUARD + 4,), SENTINEL_I, dtype=torch.int32, device=dev)
    out, slot = out_whole[GUARD:GUARD + 1], slot_whole[GUARD:GUARD + 4]
    if prefill is not None:
        slot[:3] = torch.tensor(prefill, dtype=torch.int32, device=dev)
    rc = _lib.lib().pdgn_mse_const_count(x.numel(), _lib.ptr(x), target, scale, 0.5, _lib.ptr(out), _lib.ptr(slot), _lib.stream_of(x))
    torch.cuda.synchronize()
    assert rc == 0
    ow, sw = out_whole.cpu().numpy(), slot_whole.cpu().numpy()
    assert (ow[:GUARD] == SENTINEL_F).all() and (ow[GUARD + 1:] == SENTINEL_F).all()
    assert (sw[:GUARD] == SENTINEL_I).all() and (sw[GUARD + 3:] == SENTINEL_I).all()         # word 3 of the slot and everything around it
    return ow[GUARD:GUARD + 1].view(np.uint32)[0], sw[GUARD:GUARD + 3].tolist()


@pytest.mark.parametrize("n", [1, 35, 63, 64, 65, 1023, 1024, 1025, 4099])
def test_mse_const_count_is_mse_const_plus_the_mirrors_counts(n):
    from pdgn_amd import _lib, losses
    dev = _dev()
    for specials, (target, scale) in ((True, (1.0, 0.5)), (False, (1.0, 0.5)), (False, (0.0, 1.0))):
        host = _scores(n, n, specials)
        x = torch.from_numpy(host).to(dev)
        plain = torch.full((1,), SENTINEL_F, dtype=torch.float32, device=dev)
        assert _lib.lib().pdgn_mse_const(n, _lib.ptr(x), target, scale, _lib.ptr(plain), _lib.stream_of(x)) == 0
        want_bits = plain.cpu().numpy().view(np.uint32)[0]
        bits, triple = _count_call(x, target, scale, dev)
        assert bits == want_bits, (n, specials, hex(bits), hex(want_bits))
        assert tuple(triple) == ada.counts(host), (n, specials, triple, ada.counts(host))
        bits2, triple2 = _count_call(x, target, scale, dev, prefill=(5, 6, 7))           # stored, not added to
        assert bits2 == want_bits and triple2 == triple
    # autograd: the gradient of mse_const(..., count=slot) is mse_const(...)'s, bit for bit
    host = _scores(n, 100 + n, specials=False)
    a = torch.from_numpy(host).to(dev).requires_grad_(True)
    b = torch.from_numpy(host).to(dev).requires_grad_(True)
    slot = torch.zeros(4, dtype=torch.int32, device=dev)
    la, lb = losses.mse_const(a, 1.0, 0.5), losses.mse_const(b, 1.0, 0.5, count=slot)
    (3.0 * la).backward()
    (3.0 * lb).backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    assert tuple(slot.cpu().tolist()[:3]) == ada.counts(host)


def test_mse_const_count_refuses_bad_arguments():
    from pdgn_amd import _lib, losses
    dev = _dev()
    L = _lib.lib()
    x, out, slot = torch.zeros(8, device=dev), torch.zeros(1, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    s = _lib.stream_of(x)
    p = _lib.ptr
    odd = lambda t: __import__("ctypes").c_void_p(t.data_ptr() + 2)
    assert L.pdgn_mse_const_count(0, p(x), 1.0, 0.5, 0.5, p(out), p(slot), s) == -1
    assert L.pdgn_mse_const_count(1 << 31, p(x), 1.0, 0.5, 0.5, p(out), p(slot), s) == -1
    assert L.pdgn_mse_const_count(8, None, 1.0, 0.5, 0.5, p(out), p(slot), s) == -1
    assert L.pdgn_mse_const_count(8, p(x), 1.0, 0.5, 0.5, None, p(slot), s) == -1
    assert L.pdgn_mse_const_count(8, p(x), 1.0, 0.5, 0.5, p(out), None, s) == -1
    assert L.pdgn_mse_const_count(8, p(x), 1.0, 0.5, 0.5, p(out), odd(slot), s) == -1
    with pytest.raises(TypeError):
        losses.mse_const(x, 1.0, 0.5, count=torch.zeros(4, device=dev))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- the tick against the mirror
UP, DOWN, EQ, EMPTY = [(4, 0, 4)] * 4, [(0, 4, 4)] * 4, [(3, 1, 4)] * 4, [(0, 0, 0)] * 4
MIXED = [(1, 3, 4), (4, 0, 4), (0, 0, 4), (2, 1, 4)]


def _schedule(interval):
    """Blocks of `interval` equal iterations (target 0.5: EQ gives r == target exactly), an empty iteration in the middle of the second."""
    seq = []
    for k, block in enumerate([UP, DOWN, EQ, UP, UP, MIXED, DOWN, DOWN, DOWN]):
        for j in range(interval):
            if k == 1 and j == interval // 2:
                seq.append(EMPTY)
            seq.append(block)
    return seq


@pytest.mark.parametrize("interval, span", [(1, 8), (4, 8), (1, 1 << 20), (4, 1 << 20), (4, 1 << 40)])
def test_the_adaptive_tick_is_the_mirror_word_for_word(interval, span):
    """span 8: every step crosses a clamp (16 interval 2^24 / 32 = interval / 2 of the range); 2^20: steps of 64 interval inside it;
    2^40: the max(1, .) floor.  trans_max = 0: a masked component.  The clock starts three ticks short of 2^32."""
    from pdgn_amd import _lib, augment
    dev = _dev()
    L = _lib.lib()
    params = augment.validate(**dict(augment.DEFAULTS, p=0.5, trans_max=0.0))
    adaptive = augment.validate_adaptive(dict(target=0.5, interval=interval, span=span, p_min=0.25, p_max=0.75), 0.5)
    st_h, tab_h = augment.ada_words(params, adaptive), augment.table_words(params)
    clock_h = (1 << 32) - 3
    st = torch.from_numpy(st_h.view(np.int64).copy()).to(dev)
    tab = torch.from_numpy(tab_h.view(np.int32).copy()).to(dev)
    clock = torch.tensor([clock_h], dtype=torch.int64, device=dev)
    plain_clock = clock.clone()
    slots = torch.zeros(16, dtype=torch.int32, device=dev)
    seq = _schedule(interval)
    assert len(seq) >= 3 * interval
    seen = set()
    for it, triples in enumerate(seq):
        s_h = ada.slots_of(triples)
        slots.copy_(torch.from_numpy(s_h))
        rc = L.pdgn_augment_tick_ada(_lib.ptr(clock), _lib.ptr(st), _lib.ptr(slots), _lib.ptr(tab), interval, span, ONE // 4, 3 * ONE // 4,
                                     _lib.stream_of(clock))
        assert rc == 0
        assert L.pdgn_augment_tick(_lib.ptr(plain_clock), _lib.stream_of(clock)) == 0
        before = int(st_h[ada.THR])
        st_h, tab_h, s_h, clock_h = ada.tick(st_h, tab_h, s_h, clock_h)
        torch.cuda.synchronize()
        assert st.cpu().numpy().tobytes() == st_h.tobytes(), (it, st.cpu().numpy().view(np.uint64), st_h)
        assert tab.cpu().numpy().tobytes() == tab_h.tobytes(), it
        assert not slots.cpu().numpy().any()
        assert int(clock.item()) == clock_h == int(plain_clock.item()) == (1 << 32) - 3 + it + 1
        after = int(st_h[ada.THR])
        seen.add("up" if after > before else "down" if after < before else "same")
        seen.update({"lo"} if after == ONE // 4 else {"hi"} if after == 3 * ONE // 4 else set())
    assert int(st_h[ada.UPDATES]) == 9 and [int(v) for v in tab_h[:5]] == [int(st_h[ada.THR])] * 3 + [0, 0]
    assert {"up", "down", "same"} <= seen and (span != 8 or {"lo", "hi"} <= seen)


def test_the_adaptive_tick_refuses_bad_arguments():
    import ctypes
    from pdgn_amd import _lib
    dev = _dev()
    L = _lib.lib()
    clock, st = torch.zeros(1, dtype=torch.int64, device=dev), torch.from_numpy(ada.fresh().view(np.int64).copy()).to(dev)
    slots, tab = torch.zeros(16, dtype=torch.int32, device=dev), torch.zeros(16, dtype=torch.int32, device=dev)
    s, p = _lib.stream_of(clock), _lib.ptr
    off = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)
    good = (4, 500_000, 0, ONE)
    for args in ((None, p(st), p(slots), p(tab)) + good, (p(clock), None, p(slots), p(tab)) + good, (p(clock), p(st), None, p(tab)) + good,
                 (p(clock), p(st), p(slots), None) + good, (off(clock, 4), p(st), p(slots), p(tab)) + good,
                 (p(clock), off(st, 4), p(slots), p(tab)) + good, (p(clock), p(st), off(slots, 2), p(tab)) + good,
                 (p(clock), p(st), p(slots), off(tab, 2)) + good, (p(clock), p(st), p(slots), p(tab), 0, 500_000, 0, ONE),
                 (p(clock), p(st), p(slots), p(tab), 4, 0, 0, ONE), (p(clock), p(st), p(slots), p(tab), 4, 500_000, 5, 4),
                 (p(clock), p(st), p(slots), p(tab), 4, 500_000, 0, ONE + 1)):
        assert L.pdgn_augment_tick_ada(*args, s) == -1
    torch.cuda.synchronize()
    assert int(clock.item()) == 0                                # nothing was launched


# ---------------------------------------------------------------------------- two "ranks" in one process
@pytest.mark.parametrize("B", [3, 35])
def test_two_ranks_whose_slots_are_summed_are_one_rank_at_twice_the_batch(B):
    from pdgn_amd import losses
    from pdgn_amd.augment import Augment
    dev = _dev()
    kw = dict(EVERYTHING, p=0.3, seed=SEED, device=dev, adaptive=dict(target=0.6, interval=1, span=5000))
    ranks, whole = [Augment(rank=r, **kw) for r in range(2)], Augment(rank=0, **kw)
    scores = [torch.from_numpy(_scores(2 * B, 10 * B + i, specials=i == 0)).to(dev) for i in range(4)]
    for i, s in enumerate(scores):
        losses.mse_const(s, 1.0, 0.5, count=whole.counter(i))
        for r, aug in enumerate(ranks):
            losses.mse_const(s[r * B:(r + 1) * B].contiguous(), 1.0, 0.5, count=aug.counter(i))
    assert tuple(whole.slots.cpu().tolist()[:3]) == ada.counts(scores[0].cpu().numpy())
    total = ranks[0].slots + ranks[1].slots                      # what the SUM all-reduce leaves on every rank
    assert torch.equal(total, whole.slots)
    for aug in ranks:
        aug.slots.copy_(total)
    for aug in ranks + [whole]:
        aug.tick()
    want = whole.state()
    assert want["ada"]["updates"] == 1 and want["ada"]["last"][2] == 8 * B and want["ada"]["thr"] == round(0.3 * ONE) - ada.step_size(8 * B, 5000)
    for aug in ranks:
        assert aug.ada.cpu().numpy().tobytes() == whole.ada.cpu().numpy().tobytes()
        assert aug.table.cpu().numpy().tobytes() == whole.table.cpu().numpy().tobytes()
        assert not aug.slots.cpu().numpy().any()


# ---------------------------------------------------------------------------- the trainer
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


def _drop_list(tr):
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def _one_update_happened(before, after):
    """The call opened with ONE tick, which folded the previous iteration's counts (interval 1): one update, of all 4 B = 16 scores,
    and the threshold is the mirror's step from the one before."""
    a, b = after["ada"], before["ada"]
    assert a["updates"] == b["updates"] + 1 and after["clock"] == before["clock"] + 1
    pos, neg, n = a["last"]
    assert n == 16 and pos + neg <= n and all(t[2] == 4 for t in a["last_net"])
    assert (pos, neg, n) == tuple(sum(t[j] for t in a["last_net"]) for j in range(3))
    thr, r = ada.step_thr(b["thr"], pos, neg, n, b["target"], b["span"], b["thr_min"], b["thr_max"])
    assert a["thr"] == thr and a["last_r"] == r
    want = [thr if a["mask"] >> k & 1 else 0 for k in range(5)]
    assert [after["params"][k] for k in ("thr_flip", "thr_rot", "thr_scale", "thr_trans", "thr_jitter")] == want
    assert (a["iters"], a["pos"], a["neg"], a["n"]) == (0, 0, 0, 0)


def test_the_trainer_steers_p_from_its_own_real_scores_with_no_launch_added():
    """The first iteration of a fresh trainer opens with a tick that finds empty slots: it cannot update (the rule: the tick that opens
    the NEXT iteration does).  From the second call on every call makes exactly one update."""
    dev = _dev()
    tr = _trainer(dev, dict(EVERYTHING, p=0.5, seed=SEED, adaptive=dict(target=0.6, interval=1, span=64)))
    reals, z1, z2 = _inputs(dev)
    s0 = tr.aug_state()
    assert s0["ada"]["updates"] == 0 and s0["ada"]["thr"] == ONE // 2 and s0["ada"]["mask"] == 0b01111
    tr.step(reals, z1, z2)
    s1 = tr.aug_state()
    assert s1["ada"]["updates"] == 0 and s1["clock"] == 1
    slots = tr.aug.slots.cpu().numpy().reshape(4, 4)
    assert (slots[:, 2] == 4).all() and (slots[:, 0] + slots[:, 1] <= 4).all() and (slots[:, 3] == 0).all()
    tr.step(reals, z1, z2)
    s2 = tr.aug_state()
    _one_update_happened(s1, s2)
    assert s2["ada"]["last_net"] == [tuple(int(v) for v in row[:3]) for row in slots]
    tr.capture_list(reals, z1, z2)
    the_list, state_ptr, table_ptr = tr._list, tr.aug.ada.data_ptr(), tr.aug.table.data_ptr()
    before = tr.aug_state()
    assert before["ada"]["updates"] > s2["ada"]["updates"]       # the warm-up iterations are real ones
    for _ in range(2):
        out = tr.step_list()
        after = tr.aug_state()
        _one_update_happened(before, after)
        assert len(out) == 6 and all(np.isfinite(v.item()) for v in out.values())
        before = after
    # set_augment between two replays: the same list, the same state at the same address
    tr.set_augment(target=-0.5, p=0.25, span=128)
    mid = tr.aug_state()
    assert (mid["ada"]["thr"], mid["ada"]["target"], mid["ada"]["span"], mid["params"]["thr_rot"]) == (ONE // 4, -0.5, 128, ONE // 4)
    assert mid["ada"]["updates"] == before["ada"]["updates"]
    tr.step_list()
    after = tr.aug_state()
    _one_update_happened(mid, after)
    assert tr._list is the_list and tr.aug.ada.data_ptr() == state_ptr and tr.aug.table.data_ptr() == table_ptr
    with pytest.raises(ValueError):
        tr.set_augment(p=0.9)                                    # outside [p_min, p_max] = [0, 0.8]
    with pytest.raises(ValueError):
        tr.set_augment(interval=0)
    assert tr.aug_state()["ada"]["thr"] == after["ada"]["thr"]
    info = dict(tr._list.info)
    _drop_list(tr)
    fixed = _trainer(dev, dict(EVERYTHING, p=0.5, seed=SEED))
    fixed.capture_list(reals, z1, z2)
    want = dict(fixed._list.info)
    _drop_list(fixed)
    print("launch list, adaptive: %s | fixed p: %s" % (info, want))
    assert info["nodes"] == want["nodes"] and info["kernels"] == want["kernels"]


def test_adaptivity_pinned_to_a_constant_is_the_fixed_p_trainer_and_off_is_off():
    dev = _dev()
    pinned = _trainer(dev, dict(EVERYTHING, p=0.5, seed=SEED, record=True, adaptive=dict(interval=1, span=1, p_min=0.5, p_max=0.5)))
    fixed = _trainer(dev, dict(EVERYTHING, p=0.5, seed=SEED, record=True))
    assert "ada" not in fixed.aug_state() and fixed.aug.ada is None and fixed.aug.slots is None
    reals, z1, z2 = _inputs(dev)
    for t in (7, 8, 9):
        states = []
        for tr in (pinned, fixed):
            tr.aug.set_clock(t)
            tr.step(reals, z1, z2)
            states.append(tr.aug_state())
        a, b = states
        assert a["clock"] == b["clock"] == t + 1 and a["params"] == b["params"]
        assert pinned.aug.table.cpu().numpy().tobytes() == fixed.aug.table.cpu().numpy().tobytes()
        assert a["records"].shape == (12, 4, 12) and np.array_equal(a["records"].view(np.uint32), b["records"].view(np.uint32))
    assert pinned.aug_state()["ada"]["updates"] == 2 and pinned.aug_state()["ada"]["thr"] == ONE // 2


def test_an_augment_without_adaptive_has_no_state_and_no_counter():
    from pdgn_amd.augment import Augment
    dev = _dev()
    aug = Augment(p=0.5, device=dev)
    assert aug.adaptive is None and aug.ada is None and aug.slots is None
    aug.tick()
    st = aug.state()
    assert "ada" not in st and st["clock"] == 1
    for call in (lambda: aug.counter(0), aug.checkpoint):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        aug.set(target=0.5)                                      # an adaptive parameter's name on a fixed-p object


def test_the_state_is_saved_beside_the_pair_and_restored(tmp_path):
    dev = _dev()
    ad = dict(target=0.6, interval=2, span=64)
    tr = _trainer(dev, dict(EVERYTHING, p=0.5, seed=SEED, adaptive=ad))
    reals, z1, z2 = _inputs(dev)
    for _ in range(4):
        tr.step(reals, z1, z2)
    paths = tr.save(str(tmp_path / "a"), 3, "toy")
    assert len(paths) == 3 and paths[2].endswith("3_toy_aug.pth") and all(os.path.exists(p) for p in paths)
    words, table, slots = tr.aug.ada.cpu().numpy().copy(), tr.aug.table.cpu().numpy().copy(), tr.aug.slots.cpu().numpy().copy()
    assert tr.aug_state()["ada"]["updates"] == 1 and tr.aug_state()["ada"]["iters"] == 1 and slots.any()
    fresh = _trainer(dev, dict(EVERYTHING, p=0.1, seed=SEED, adaptive=dict(target=0.3, interval=5, span=999)))
    ptr = fresh.aug.ada.data_ptr()
    assert fresh.load(paths[0], paths[1]) == 3
    assert fresh.aug.ada.data_ptr() == ptr and fresh.aug.ada.cpu().numpy().tobytes() == words.tobytes()
    assert fresh.aug.table.cpu().numpy().tobytes() == table.tobytes() and fresh.aug.slots.cpu().numpy().tobytes() == slots.tobytes()
    assert fresh.aug.adaptive == tr.aug.adaptive and fresh.aug_state()["ada"] == tr.aug_state()["ada"]
    # a fixed-p trainer writes no sibling; its pair leaves an adaptive trainer's constructed state alone; an adaptive pair loads into it
    fixed = _trainer(dev, dict(EVERYTHING, p=0.5, seed=SEED))
    assert fixed.load(paths[0], paths[1]) == 3 and "ada" not in fixed.aug_state()
    plain = fixed.save(str(tmp_path / "b"), 4, "toy")
    assert len(plain) == 2 and sorted(os.listdir(tmp_path / "b")) == ["4_toy_D.pth", "4_toy_G.pth"]
    other = _trainer(dev, dict(EVERYTHING, p=0.1, seed=SEED, adaptive=dict(target=0.3, interval=5, span=999)))
    constructed = other.aug.ada.cpu().numpy().copy()
    assert other.load(plain[0], plain[1]) == 4
    assert other.aug.ada.cpu().numpy().tobytes() == constructed.tobytes() and other.aug_state()["ada"]["thr"] == round(0.1 * ONE)


def test_fit_writes_aug_csv(tmp_path):
    from pdgn_amd.data import BatchFeeder
    dev = _dev()
    B, N, sizes = 4, 2048, (256, 512, 1024)
    clouds = torch.from_numpy(np.random.default_rng(4).standard_normal((2 * B + 1, N, 3)).astype(np.float32)).to(dev)
    feeder = BatchFeeder(clouds, B, sizes, seed=31)
    assert feeder.batches_per_epoch == 2
    tr = _trainer(dev, dict(EVERYTHING, p=0.2, seed=SEED, adaptive=dict(target=0.6, interval=1, span=64)))
    assert tr.fit(feeder, 2, log=str(tmp_path / "log.txt"), on_epoch=lambda e: None) == 2
    _drop_list(tr)
    rows = list(csv.reader(open(tmp_path / "aug.csv")))
    assert rows[0] == ["epoch", "clock", "p", "updates", "last_r", "r_D1", "r_D2", "r_D3", "r_D4"]
    assert [r[0] for r in rows[1:]] == ["1", "2"] and [r[1] for r in rows[1:]] == ["2", "4"]
    for r in rows[1:]:
        assert 0.0 <= float(r[2]) <= 0.8 and int(r[3]) >= 1 and all(-1.0 <= float(v) <= 1.0 for v in r[4:])
    assert float(rows[2][2]) == tr.aug_state()["ada"]["p"] and int(rows[2][3]) > int(rows[1][3])
    # a fixed-p fit writes no such file
    fixed = _trainer(dev, dict(EVERYTHING, p=0.2, seed=SEED))
    os.makedirs(tmp_path / "f")
    fixed.fit(BatchFeeder(clouds, B, sizes, seed=31), 1, issue="eager", log=str(tmp_path / "f" / "log.txt"), on_epoch=lambda e: None)
    assert sorted(os.listdir(tmp_path / "f")) == ["log.txt"]


def test_cli_trains_with_d_augment_target(tmp_path):
    from pdgn_amd.data import cate_to_synsetid
    rng = np.random.default_rng(5)
    sid = cate_to_synsetid["chair"]
    np.savez(tmp_path / "toy.npz", **{"%s/%s" % (sid, sp): rng.standard_normal((n, 2048, 3)).astype(np.float32)
                                      for sp, n in (("train", 9), ("val", 2), ("test", 6))})
    cmd = [sys.executable, "-m", "pdgn_amd.train", "--model_dir", "toy", "--checkpoint_dir", str(tmp_path / "ck"), "--data_root",
           str(tmp_path / "toy.npz"), "--choice", "chair", "--batch_size", "4", "--seed", "1", "--save_dir", str(tmp_path / "res"),
           "--phase", "train", "--max_epoch", "1", "--snapshot", "1", "--d_augment", "0.2", "--d_augment_target", "0.6", "--ada_span", "64"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    log = (tmp_path / "ck" / "toy" / "log_info.txt").read_text().splitlines()
    assert "d_augment=0.2" in log[0] and "d_augment_target=0.6" in log[0] and "ada_span=64" in log[0]
    assert len([l for l in log if l.startswith("Epoch: [ 1]")]) == 2                 # 9 clouds, batches of 4
    rows = list(csv.reader(open(tmp_path / "ck" / "toy" / "aug.csv")))
    assert len(rows) == 2 and rows[0][:3] == ["epoch", "clock", "p"] and rows[1][0] == "1" and 0.0 <= float(rows[1][2]) <= 0.8
    assert sorted(os.listdir(tmp_path / "ck" / "toy" / "PDGNet_v2")) == ["1_chair_D.pth", "1_chair_G.pth", "1_chair_aug.pth"]
