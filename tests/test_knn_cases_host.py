"""The feature-kNN cases on the host (tests/knn_cases.py): the premise of the exact cases, the integer reference against the float64
stand-in, the regimes every case exists for, and the judge of float rows against an fp32 stand-in and two planted errors."""
import numpy as np
import pytest
import torch

import knn_cases as kc
from torch_standins import feature_knn_torch

IDS = [c.id for c in kc.CASES]


@pytest.mark.parametrize("case", kc.CASES, ids=IDS)
def test_guard_and_integer_reference_equals_float64_standin(case):
    x, keys, idx, sq = kc.prepared(case)
    kc.guard(x, keys)
    assert int(np.abs(x).max()) <= kc.vmax_of(case.f) and kc.dispatch(case.f, case.n, case.k)[0] != "small"
    ref = feature_knn_torch(torch.tensor(x, dtype=torch.float64), case.k).numpy()
    np.testing.assert_array_equal(idx, ref)
    np.testing.assert_array_equal(sq, (x.astype(np.float64) ** 2).sum(1).astype(np.int64))


@pytest.mark.parametrize("case", kc.CASES, ids=IDS)
def test_case_reaches_its_regimes(case):
    counts = kc.regimes(case)
    kc.check_expect(case, counts)
    if counts["kernel"] == "pc":                              # knn_flush_select_multi's "more than 128 entries" cannot happen
        assert counts["final_entries_max"] <= kc.FKP_QCAP + kc.SELECT_MAX < 128


def test_guard_refuses_what_is_not_exact():
    x = kc.make_input(1, 8, 16, "wide").copy()
    x[0, 0, 0] = 0.5
    with pytest.raises(AssertionError):
        kc.guard(x)
    x = np.full((1, 64, 16), 257.0, np.float32)                       # integers, but 4 f vmax^2 > 2^24
    x[0, :, 1] = -257.0
    with pytest.raises(AssertionError):
        kc.guard(x)


def test_kinds_tie_as_described():
    def tied(case_id, top):
        _, keys, _, _ = kc.prepared(kc.BY_ID[case_id])
        s = np.sort(keys[0][0], 1)[:, :top]
        return float((s[:, 1:] == s[:, :-1]).any(1).mean())
    assert tied("1x32x128-k10-narrow", 12) > 0.5
    assert tied("1x32x4096-k10-wide", 12) < 0.01
    x = kc.make_input(2, 64, 512, "mixed")
    for b in range(2):
        for r in range(3):
            same = x[b][:, r * 4::12]
            assert same.shape[1] >= 42 and (same == same[:, :1]).all()


def test_sixteen_bit_threshold_bounds_the_kth_value():
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.integers(0, 1 << 24, (50, 64)).astype(np.float32), -rng.random((10, 64), np.float32),
                        np.full((1, 64), np.inf, np.float32)])
    for K in (1, 11, 32):
        kth, ub = np.sort(v, 1)[:, K - 1], kc.kth_ub16(v, K)
        assert (ub >= kth).all() and (ub[:-1] <= np.maximum(kth[:-1] * 1.008, kth[:-1] * 0.992)).all() and ub[-1] == np.inf


def test_persistent_map_of_the_stage_shapes():
    owned = kc.persistent_map(17, 640)                                   # 20 tiles per sample; XCD 0: samples 0, 8, 16
    assert len(owned) == 256 and owned[0] == [(0, 0), (8, 12)] and owned[8 * 31] == [(8, 11)]
    assert [len(w) for w in owned[0::8]] == [2] * 28 + [1] * 4
    assert [len(w) for w in owned[1::8]] == [2] * 8 + [1] * 24           # XCD 1: samples 1 and 9, 40 tiles on 32 workgroups
    one = kc.persistent_map(1, 128)
    assert len(one) == 32 and one[0] == [(0, 0)] and one[24] == [(0, 3)] and sum(len(w) for w in one) == 4


# ------------------------------------------------------------------------------------------------------------------ the row judge
JUDGE_SHAPES = [(2, 6, 24, 5), (2, 32, 516, 10), (1, 62, 1000, 10)]


@pytest.mark.parametrize("B,f,n,k", JUDGE_SHAPES)
def test_judge_accepts_fp32_standin(B, f, n, k):
    x = kc.gaussian(B, f, n)
    ok, used = kc.judge_rows(x, feature_knn_torch(torch.from_numpy(x), k).numpy(), k)
    assert ok.all() and used < 0.25, (int((~ok).sum()), used)


@pytest.mark.parametrize("B,f,n,k", JUDGE_SHAPES)
def test_judge_rejects_planted_errors(B, f, n, k):
    x = kc.gaussian(B, f, n)
    x64 = torch.from_numpy(x).double()
    order = (-2 * torch.bmm(x64.transpose(1, 2), x64) + (x64 ** 2).sum(1).unsqueeze(2) + (x64 ** 2).sum(1).unsqueeze(1)).argsort(dim=2).numpy()
    good = order[:, :, 1:k + 1]
    assert kc.judge_rows(x, good, k)[0].all()
    # one neighbour replaced by the row's median-distance point, in one row per sample
    bad = good.copy()
    rows = [3 % n, n // 2]
    for b in range(B):
        bad[b, rows[b % 2], k // 2] = order[b, rows[b % 2], n // 2]
    ok = kc.judge_rows(x, bad, k)[0]
    for b in range(B):
        assert not ok[b, rows[b % 2]] and ok[b].sum() == n - 1
    # ranks 2..k+1 instead of ranks 1..k, on every row
    assert not kc.judge_rows(x, order[:, :, 2:k + 2], k)[0].any()
    # and what no graph may hold: a repeated index, an index out of range
    rep = good.copy()
    rep[0, 0, 1] = rep[0, 0, 0]
    oob = good.copy()
    oob[0, 1, 0] = n
    assert not kc.judge_rows(x, rep, k)[0][0, 0] and not kc.judge_rows(x, oob, k)[0][0, 1]


def test_finite_reference_maps_back():
    x, at = kc.poison(kc.make_input(2, 7, 100, "wide"))
    ref, fin = kc.int_graph_finite(x, 4)
    assert (~fin).sum() == 6 and all(not fin[b, p] for b in range(2) for p in at[b])
    assert (ref[~fin] == -1).all() and (ref[fin] >= 0).all() and fin[np.arange(2)[:, None, None], ref.clip(0)][fin].all()
    far = x.copy()                                                            # the poisoned points moved far away instead
    for b in range(2):
        far[b][:, ~fin[b]] = 3.0 * 255
    np.testing.assert_array_equal(kc.int_graph(far, 4)[0][fin], ref[fin])


def test_judge_tolerates_a_swap_inside_the_bound_only():
    """Two points one ulp apart in one channel: their order is below fp32 resolution for every other query, so either order passes
    (and uses a part of the bound); two clearly separated neighbours swapped do not.  (As QUERIES the two points fail the judge
    whatever is returned -- the dropped rank 0 must be clearly before the first returned point, and their twin is not: the judged
    inputs are Gaussian and hold no such pair.)"""
    n, k, q = 64, 63, 20
    x = kc.gaussian(1, 16, n)
    x[0, :, 10] = x[0, :, 9]
    x[0, 0, 10] = np.nextafter(x[0, 0, 9], np.float32(np.inf))
    others = np.ones(n, bool)
    others[[9, 10]] = False
    x64 = x[0].astype(np.float64)
    d = ((x64[:, :, None] - x64[:, None, :]) ** 2).sum(0)
    good = np.argsort(d, axis=1, kind="stable")[None, :, 1:k + 1]
    ok, used = kc.judge_rows(x, good, k)
    assert ok[0, others].all() and not ok[0, ~others].any() and used == 0.0
    a, b = (int(np.nonzero(good[0, q] == p)[0][0]) for p in (9, 10))
    assert abs(a - b) == 1
    swapped = good.copy()
    swapped[0, q, [a, b]] = swapped[0, q, [b, a]]
    ok, used = kc.judge_rows(x, swapped, k)
    assert ok[0, others].all() and 0.0 < used < 1.0, used
    far = good.copy()
    far[0, q, [0, 5]] = far[0, q, [5, 0]]
    ok, _ = kc.judge_rows(x, far, k)
    assert not ok[0, q] and ok[0, others].sum() == n - 3
