"""tests/gemm_cases.py checked on the CPU: every case passes the guard of its kind of data, every required regime tag is carried by
some case at 256 CUs, the shapes named in the module enter the regimes they were chosen for, the library's launch-model queries
(host code: csrc/gemm_plan.h) equal the module's restatement for every case, and the numpy mirrors of the two splits
(csrc/split.hip, csrc/gemm_x3.hip's loaders) reassemble their inputs within the bounds the kernels' headers state."""
import numpy as np
import pytest

import gemm_cases as gc

CUS = 256
F32, F64 = np.float32, np.float64
ORDERED = sorted(gc.CASES, key=lambda c: gc.operand_key(c) + (c.name,))       # equal operands next to each other: one generation


@pytest.mark.parametrize("case", ORDERED, ids=lambda c: c.name)
def test_every_case_passes_the_guard_of_its_data(case):
    d = gc.describe(case, CUS)
    assert not d.get("refused"), "two-part planes with partials need the 256 x 128 tile to be the pick"
    kind = gc.data_kind(case)
    if kind in ("int", "int1"):
        assert gc.exact_guard(case) < gc.LIMIT
        o = gc.operands(case)
        for x in (o["a"], o["w"]):
            assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= (1 if kind == "int1" else 7) and (x == 0).any()
        if "stats" in case.epi:
            assert kind == "int1" and gc.stat_guard(case, gc.stat_block_rows(case, CUS)) < gc.LIMIT
    elif kind == "normal":
        assert case.epi == () or case.epi == ("hand",)
    else:
        assert gc.level_guard(case) < gc.LIMIT
        o = gc.operands(case)
        assert not any(e in case.epi for e in ("bias", "addend", "rb1", "rb12", "act", "gate"))
        lv, sc = (o["w"], o["sw"]) if case.data.endswith("_w") else (o["a"], o["sa"])
        assert sc.max() - sc.min() >= 16                              # the rows' scales span many binades
        h, m, l = gc.split_bf16x3(lv)
        assert np.array_equal(h.astype(F64) + m.astype(F64) + l.astype(F64), lv.astype(F64))      # the split loses nothing
        hh, ll = gc.split_f16x2(lv, gc.absmax_bits(lv, 1))
        if kind == "two_level":
            back = (hh.astype(F64) + ll.astype(F64)) * gc.x2_unscale(gc.absmax_bits(lv, 1)).astype(F64)[:, None]
            assert np.array_equal(back, lv.astype(F64)) and (ll != 0).mean() > 0.5
        else:
            assert gc.kernel_dims(case)[2] <= 64 or case.name == "l3_x3_tail_atomic"
            assert gc.low_part_share(case) >= 0.25 and (m != 0).mean() >= 0.5
            assert case.mode in ("x3", "fp32")


def test_every_required_tag_is_carried_by_some_case():
    cov = gc.coverage(CUS)
    missing = [t for t in gc.REQUIRED if not cov.get(t)]
    assert not missing, missing
    assert len(set(gc.REQUIRED)) == len(gc.REQUIRED)


def _tags(fam, cfg, m, n, k, mode=None, entry="nt"):
    c = gc.Case("probe", entry, m, n, k, mode or fam, cfg, 32, (), gc.NOPAD, "int")
    pre = "%s.%d:" % ("x2" if entry == "ps2" else fam, cfg)
    return {t[len(pre):] for t in gc.reached(c, CUS) if t.startswith(pre)}, gc.describe(c, CUS)


def test_the_named_shapes_enter_their_regimes_at_256_cus():
    for fam, cfgs in (("x3", range(3)), ("fp32", range(4))):
        for cfg in cfgs:
            t, d = _tags(fam, cfg, 100, 8, 4)
            assert {"one_partial_tile", "k_tail", "k4", "ragged_m", "ragged_n"} <= t and d["plan"].grid_dp == 1
            t, d = _tags(fam, cfg, 100, 8, 1028)
            assert {"tail_only", "one_partial_tile"} <= t and d["plan"].grid_sk == 2          # a 2-workgroup atomic tail ...
            if fam == "x3":
                assert {"tail_aligned", "tail_atomic"} <= t and d["tail"].s_tail == 33 and d["tail"].seg == 0      # ... or 33 aligned slices
                assert d["ws_floats"] == 33 * d["tile"].BM * d["tile"].BN
    for fam, cfg, m in (("x3", 0, 2400), ("x3", 1, 1100), ("x3", 2, 1100), ("fp32", 0, 2400), ("fp32", 1, 1100), ("fp32", 3, 1100)):
        assert "multigroup" in _tags(fam, cfg, m, 8, 4)[0]
        assert {"multigroup", "tail_only"} <= _tags(fam, cfg, m, 8, 1028)[0]
    assert "multigroup" not in _tags("fp32", 2, 1100, 8, 4)[0] and "multigroup" in _tags("fp32", 2, 33000, 132, 4)[0]
    for cfg, shape in ((0, (17000, 8, 1028)), (1, (17000, 8, 1028)), (2, (33000, 8, 516))):
        t, d = _tags("x3", cfg, *shape)
        assert {"tail_only", "tail_flat"} <= t and d["tail"].seg == 2
    for fam, cfg, shape in (("x3", 0, (66000, 8, 4)), ("x3", 1, (33000, 8, 4)), ("x3", 2, (66000, 68, 4)), ("fp32", 0, (66000, 8, 4)),
                            ("fp32", 1, (66000, 8, 4)), ("fp32", 2, (33000, 132, 4)), ("fp32", 3, (33000, 132, 4))):
        assert "rounds_no_tail" in _tags(fam, cfg, *shape)[0], (fam, cfg)
        t, d = _tags(fam, cfg, shape[0], 8 if shape[1] == 68 else shape[1], 1028)
        assert "rounds_plus_tail" in t, (fam, cfg)
        assert fam != "x3" or "tail_aligned" in t
    # (the square fp32 tile runs two workgroups per CU: 33000 rows of 8 columns are half a round there)
    assert "rounds_no_tail" not in _tags("fp32", 1, 33000, 8, 4)[0]
    for cfg, shape in ((0, (9000, 1028, 1028)), (1, (9000, 520, 1028)), (2, (33000, 132, 1028))):
        t, d = _tags("x3", cfg, *shape)
        assert {"rounds_plus_tail", "tail_flat"} <= t and d["tail"].seg >= 2
    t, d = _tags("x3", 0, 9000, 1028, 1028, mode="x2", entry="ps2")
    assert {"rounds_plus_tail", "tail_flat"} <= t and d["two"] and d["eight_waves"]


def test_launch_arithmetic_restated():
    big, sq, nar = gc.X3_TILES
    assert [160 * 1024 // (2 * (t.BM + t.BN) * 32 * 4) for t in gc.FP32_TILES] == [t.WG for t in gc.FP32_TILES] == [1, 2, 2, 3]      # gemm_nt.hip: NtCfg::WG_PER_CU
    assert gc.dp_grid(big, 258, 256, 1) == 256 and gc.dp_grid(big, 1000, 256, 1) == 256 and gc.dp_grid(big, 4096, 256, 1) == 512
    assert gc.dp_grid(gc.FP32_TILES[0], 4096, 256, 8) == 1024 and gc.dp_grid(big, 4096, 256, 8) == 512
    assert gc.chunk_us(big, 1) == 2.0 * 256 * 128 * 32 / 760e3
    pl = gc.plan(big, 100, 8, 1028, True, CUS)
    assert (pl.tiles_m, pl.tiles_n, pl.kchunks, pl.grid_dp, pl.grid_sk, pl.sk_per_wg) == (1, 1, 33, 0, 2, 17)
    assert gc.plan(big, 100, 8, 1028, False, CUS).grid_sk == 0
    # the weight gradients' slices: 45 tiles on 256 slots: 5 slices of the 282 chunks of 9000 rows, 57 chunks each
    pl = gc.plan(big, 1028, 1084, 9000, True, CUS)
    assert gc.at_slices(big, pl, CUS) == 5 and gc.cdiv(pl.kchunks, 5) == 57
    assert gc.x2_pays("x2", 0, 9000, 1084, 1028, 0) and not gc.x2_pays("x2", 0, 9000, 1084, 1024, 0)
    assert not gc.x2_pays("x2", 0, 9000, 1084, 1028, 9000 * 1028 * 4 + 1084 * 1028 * 4 + 10 ** 8)
    assert not gc.x2_pays("x3", 0, 9000, 1084, 1028, 0) and not gc.x2_pays("x2", 1, 9000, 1084, 1028, 0)
    assert gc.rp_takes(4099, 3908, 32) and not gc.rp_takes(4095, 4100, 128) and not gc.rp_takes(4099, 3900, 64) and not gc.rp_takes(4099, 4100, 256)
    # a forced configuration: the fp32 kernel's fourth reads as the narrow x3 tile; the tall fp32 tile is not a weight-gradient tile
    assert gc.pick("x3", 100, 8, 4, False, CUS, 3) == 2 and gc.pick("fp32", 100, 8, 4, False, CUS, 2, no_tall=True) == 1


@pytest.mark.parametrize("case", ORDERED, ids=lambda c: c.name)
def test_launch_model_queries_equal_the_restatement_on_the_host(case):
    """The comparison of tests/test_gpu_gemm_exact.py's query test, the same assertions, wherever the library loads: the queries are host
    code (csrc/gemm_plan.h), which without a device plans for 256 CUs.  No device pointer is passed and nothing is launched.  The
    switches are process-wide and tests/conftest.py resets them after gpu-marked tests only: this test puts back what it found."""
    import torch
    from pdgn_amd import _lib
    L = _lib.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else CUS
    found = (L.pdgn_gemm_set_mode(-1), L.pdgn_gemm_set_config(-2), L.pdgn_gemm_set_shape(-2))      # (-1 / -2 / -2: leave, tell)
    try:
        L.pdgn_gemm_set_mode({"fp32": 0, "x3": 1, "x2": 2}[case.mode])
        L.pdgn_gemm_set_config(-1 if case.cfg is None else case.cfg)
        if case.mode != "fp32":
            L.pdgn_gemm_set_shape(case.shape)
        gc.check_launch_model_queries(L, case, cus)
    finally:
        L.pdgn_gemm_set_mode(found[0])
        L.pdgn_gemm_set_config(found[1])
        L.pdgn_gemm_set_shape(0x1000 | found[2])
        assert (L.pdgn_gemm_set_mode(-1), L.pdgn_gemm_set_config(-2), L.pdgn_gemm_set_shape(-2)) == found


# ---------------------------------------------------------------------------- the split mirrors
def test_bf16x3_mirror_reassembles_within_the_headers_bound():
    """gemm_x3.hip: x = h + m + l (+ e), |m| <= 2^-8 |x|, |l| <= 2^-16 |x|, |e| <= 2^-25 |x| -- for values whose parts are normal
    numbers.  bf16 has fp32's exponent range, so below 2^-126 the parts are multiples of 2^-133 and the error is absolute (at most
    2^-134); and a value above 2^127 (2 - 2^-8) = 3.3962e38 rounds UP to infinity in h (1e38 itself, and everything up to 3.3962e38,
    splits like any other value): its remainder is -inf and l is NaN -- the three-part product of such a value is not finite."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(20000) * np.exp2(rng.integers(-90, 120, size=20000))).astype(F32)
    x = np.concatenate([x, gc.edge_rows()[:7].ravel()])
    h, m, l = (p.astype(F64) for p in gc.split_bf16x3(x))
    x64 = x.astype(F64)
    ax = np.abs(x64)
    normal = ax >= 2.0 ** -100
    assert np.all(np.abs(m)[normal] <= 2.0 ** -8 * ax[normal]) and np.all(np.abs(l)[normal] <= 2.0 ** -16 * ax[normal])
    assert np.all(np.abs(x64 - (h + m + l))[normal] <= 2.0 ** -25 * ax[normal])
    assert np.all(np.abs(x64 - (h + m + l))[~normal] <= 2.0 ** -134)
    assert np.array_equal(np.signbit(gc.split_bf16x3(np.array([-0.0, 0.0], dtype=F32))[0]), [True, False])
    # every part is a bf16: nothing below bit 16
    for p in gc.split_bf16x3(x):
        assert not (p.view(np.uint32) & 0xffff).any()
    edge = np.array([1e38, 3.3961e38, 3.3963e38, 3.4028235e38, -3.4e38], dtype=F32)
    eh, em, el = gc.split_bf16x3(edge)
    assert np.isfinite(eh[:2]).all() and np.isinf(eh[2:]).all() and np.isnan(el[2:]).all()
    assert np.all(np.abs(edge[:2].astype(F64) - (eh[:2].astype(F64) + em[:2] + el[:2])) <= 2.0 ** -25 * np.abs(edge[:2].astype(F64)))


def test_x2_exponent_and_scale_field_restated():
    bits = lambda v: np.array([v], dtype=F32).view(np.uint32)[0]
    for v, e in ((1.0, 14), (1.99, 14), (2.0, 13), (0.5, 15), (65504.0, -1), (3.4e38, -113), (2.0 ** -100, 114), (2.0 ** -112, 126),
                 (2.0 ** -113, 126), (2.0 ** -126, 126), (1e-40, 126), (0.0, 126)):
        assert gc.x2_exponent(bits(v)) == e, v
        assert gc.x2_scale(np.array([bits(v)]))[0] == F32(2.0) ** e and gc.x2_unscale(np.array([bits(v)]))[0] == F32(2.0) ** -e
    assert gc.x2_exponent(0x7f800000) == -114 and gc.x2_scale_field(0x7f800000) == 13          # Inf / NaN: the largest field
    assert gc.x2_scale_field(0) == 253 and gc.x2_scale_field(bits(2.0 ** 127)) == 14 and gc.x2_scale_field(0x7fffffff) == 13
    # the field is 127 + e wherever neither clamp acts
    f = np.arange(1, 255, dtype=np.int64) << 23
    assert np.array_equal(gc.x2_scale_field(f), np.clip(127 + gc.x2_exponent(f), 1, 253))


def test_f16x2_mirror_reassembles_within_the_headers_bound():
    """gemm_x3.hip: row r times 2^e_r, e_r = 14 - floor(log2 max |x|): the maximum lands in [2^14, 2^15); x 2^e = h + l keeps 22
    bits while |x| is within 2^-16 of its row's maximum, an absolute 2^-39 of the maximum below (the existing bound: 2^-22 of the
    row's maximum everywhere).  An all-zero row: e clamps to 126, both parts zero."""
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((64, 40)) * np.exp2(rng.integers(-30, 1, size=(64, 40))) * np.exp2(rng.integers(-100, 100, size=(64, 1)))).astype(F32)
    x = np.concatenate([x, gc.edge_rows()])
    mb = gc.absmax_bits(x, 1)
    h, l = gc.split_f16x2(x, mb)
    assert np.isfinite(h.astype(F64)).all() and np.isfinite(l.astype(F64)).all()
    mx = np.abs(x.astype(F64)).max(1)
    e = gc.x2_exponent(mb)
    live = (e > -126) & (e < 126)
    sm = np.ldexp(mx, e)
    assert np.all((sm[live] >= 2.0 ** 14) & (sm[live] < 2.0 ** 15))
    back = np.ldexp(h.astype(F64) + l.astype(F64), -e[:, None])
    err = np.abs(back - x.astype(F64))
    assert np.all(err[live] <= 2.0 ** -22 * mx[live, None])
    near = live[:, None] & (np.abs(x.astype(F64)) >= 2.0 ** -16 * mx[:, None])
    assert np.all(err[near] <= 2.0 ** -22 * np.abs(x.astype(F64))[near])
    assert np.all(err[live] <= np.maximum(2.0 ** -22 * np.abs(x.astype(F64)), 2.0 ** -39 * mx[:, None])[live])
    # the clamped rows: all zero -> zero parts; subnormals only -> scaled by 2^126, what fp16 holds of them
    assert e[64] == 126 and not h[64].any() and not l[64].any()
    assert e[64 + 4] == 126 and np.all(err[64 + 4] <= 2.0 ** -126 * 2.0 ** -24)
    assert np.array_equal(np.signbit(h[64 + 1][:2]), [False, True])


def test_normal_reference_is_the_mirror_of_the_arithmetic_not_fp64():
    """The dropped partial products (am wl, al wm, al wl; al wl for two parts) are what separates the mirror from fp64: the mirror is
    within the header's per-product bound of fp64 -- 2^-23 (three parts) / 2^-21 (two parts) of sum |a||w| -- and not equal to it."""
    c = gc.BY_NAME["normal_x3_nt"]
    o = gc.operands(c)
    ref = gc.mirror_product(o["a"], o["w"], "fp32")
    mag = np.abs(o["a"]).astype(F64) @ np.abs(o["w"]).astype(F64).T
    for mode, bound in (("x3", 2.0 ** -23), ("x2", 2.0 ** -21)):
        got = gc.mirror_product(o["a"], o["w"], mode)
        assert np.all(np.abs(got - ref) <= bound * mag) and np.abs(got - ref).max() > 0
