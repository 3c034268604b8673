"""tests/persample_cases.py on the host: the exactness guard and the variance guard of every case, the restated launch arithmetic of
csrc/skinny.hip and csrc/small_mlp.hip against the figures the kernels' comments and callers state, and that every regime the
GPU module is meant to enter is entered by at least one case.  No GPU."""
import numpy as np
import pytest

import persample_cases as pc


def _id(case):
    return type(case).__name__.lower() + "-" + case.name


EXACT = [c for c in pc.all_cases() if c.data in ("int", "bn")]
BN = [c for c in pc.SM_CASES if c.data == "bn"]


@pytest.mark.parametrize("case", EXACT, ids=_id)
def test_every_sum_of_an_integer_case_is_exact_in_any_order(case):
    worst = pc.exact_guard(case)
    print("%s: max sum |a||b| = %d = 2^%.2f" % (_id(case), worst, np.log2(max(worst, 1))))
    assert worst < pc.LIMIT
    ops = {pc.NT: pc.nt_operands, pc.NN: pc.nn_operands, pc.TN: pc.tn_operands, pc.SM: pc.sm_operands}[type(case)](case)
    for name in ("A", "B", "x", "W", "bias"):
        v = ops.get(name)
        if v is not None:
            assert v.dtype == np.float32 and np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 7
            assert (v == 0).any() or v.size < 64                      # zeros included (15 values: a small operand may draw none)


@pytest.mark.parametrize("case", BN, ids=_id)
def test_batchnorm_cases_have_integer_pre_and_variance_at_least_one(case):
    o = pc.sm_operands(case)
    pre = o["ref"]["pre"]
    assert np.array_equal(pre, np.rint(pre)) and np.abs(pre).max() < pc.LIMIT
    var = pc.variance_guard(case)
    print("%s: smallest variance %s (draw %d)" % (case.name, var, o["attempt"]))
    assert var is None or var >= 1.0
    assert case.act == 0 or np.abs(o["ref"]["z"]).min() > 1e-3
    # the shapes whose gradients are analytically zero stay out of bn_mode 1 (module docstring)
    assert not (case.bn == 1 and (case.K == 1 or case.R == 2))


def test_masked_cases_hold_both_zeros_and_both_smallest_subnormals():
    for case in pc.NN_CASES:
        if not case.masked:
            continue
        P = pc.nn_operands(case)["P"]
        bits = set(P.view(np.uint32).reshape(-1).tolist())
        assert {0x00000000, 0x80000000, 0x00000001, 0x80000001} <= bits, case.name
        assert (P > 1).any() and (P < -1).any()


def test_launch_arithmetic_restated():
    """The figures the issue's regimes name, from the restated arithmetic."""
    L = pc.nt_launch(35, 17, 68)
    assert L["split"] and L["kchunks"] == 5 and L["per"] == 2 and L["owned"] == (2, 2, 1, 0)
    assert pc.nt_launch(1, 1, 4)["owned"] == (1, 0, 0, 0) and pc.nt_launch(64, 20, 256)["owned"] == (4, 4, 4, 4)
    assert pc.nt_launch(3, 4095, 4)["split"] and not pc.nt_launch(35, 4096, 4)["split"]
    L = pc.nt_launch(35, 4100, 20)
    assert L["grid"] == 65 and L["idle_waves"] == 3 and L["partial_columns"]
    L = pc.nn_launch(35, 64, 2050)
    assert (L["kchunks"], L["slices"], L["per"], L["gy"], L["last"]) == (129, 16, 9, 15, 3)
    L = pc.nn_launch(17, 68, 4100)
    assert (L["kchunks"], L["gx"], L["slices"], L["per"], L["gy"], L["last"]) == (257, 2, 32, 9, 29, 5)
    for k in (1, 3, 5, 16, 19, 127, 128):
        assert pc.nn_launch(35, 64, k)["single"]
    L = pc.tn_launch(5, 6400, 120)
    assert (L["gx"], L["gy"], L["kblocks"], L["strided"]) == (100, 5, 8, True)
    assert not pc.tn_launch(35, 65, 40)["strided"]
    L = pc.sm_launch(64, 632, 3)
    assert L["ok"] and L["lds_bwd"] == 160 * 1024 and 64 * 636 * 4 + 1024 == 160 * 1024
    assert not pc.sm_ok(64, 636, 3, 0, 0) and not pc.sm_ok(35, 1028, 3, 0, 0) and not pc.sm_ok(65, 4, 4, 0, 0)
    assert not pc.sm_ok(64, 1000, 16, 2, 1)                           # (what test_small_sequential_vs_torch's R = 64 case asked for)
    L = pc.sm_launch(35, 1024, 4)
    assert L["ok"] and L["attr_fwd"] and L["attr_bwd"]
    L = pc.sm_launch(35, 260, 9)
    assert L["vec"] and L["dw_rounds"] == 2 and not L["attr_fwd"]
    assert not pc.sm_launch(35, 21, 5)["vec"] and pc.sm_launch(35, 21, 5)["dead_waves"] == 3


def test_every_regime_is_entered_by_some_case():
    tags = set()
    for case in pc.all_cases():
        tags |= pc.reached(case)
    missing = [t for t in pc.REQUIRED if t not in tags]
    assert not missing, missing


def test_contracts_of_the_entry_points_hold_for_every_case():
    """No case hands a kernel what include/pdgn_hip.h excludes."""
    for c in pc.NT_CASES:
        assert 1 <= c.R <= 64 and c.K % 4 == 0 and c.pads[0] % 4 == 0 and c.pads[1] % 4 == 0 and c.pads[2] >= 0
    for c in pc.NN_CASES:
        assert 1 <= c.R <= 64 and c.N % 4 == 0 and c.pads[0] % 4 == 0 and c.pads[2] % 4 == 0 and min(c.pads) >= 0
        assert c.masked == (c.act in (1, 2))
    for c in pc.TN_CASES:
        assert 1 <= c.R <= 64 and min(c.pads) >= 0
    for c in pc.SM_CASES:
        assert pc.sm_ok(c.R, c.K, c.N, c.act, c.bn) and (c.bn != 2 or c.running) and (c.bn or not (c.affine or c.running))
    names = [_id(c) for c in pc.all_cases()]
    assert len(set(names)) == len(names)
    assert max(c.R * max(c.N, c.K) for c in pc.all_cases()) <= 64 * 12832
    assert len(set(pc.REFUSED)) == len(pc.REFUSED)
