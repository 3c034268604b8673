"""The dense contraction kernels (csrc/gemm_x3.hip, gemm_x3_16.hip, gemm_x3_h2.hip, gemm_nt.hip, gemm_rp.hip, split.hip) pinned
exactly, through the C ABI, in every tile and tail regime of tests/gemm_cases.py: on exact data (small integers, two- and
three-level dyadic values with per-row scales) every mode, tile, instruction shape and tail form -- with a workspace, with one a float
too small, with none: fp32 atomics -- must return the bits of the fp64 product; on random normal data the numpy mirror of the split
arithmetic within the fp32 accumulation bound.  The launch-model queries are compared with the module's restatement of the launch
arithmetic, case by case, and the split kernels with the numpy mirrors bit for bit.  Outputs are pre-filled with NaN inside guard
bands of a sentinel that must come back untouched."""
import functools

import numpy as np
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ORDERED = sorted(gc.CASES, key=lambda c: gc.operand_key(c) + (c.name,))       # equal operands next to each other: one upload, one product
BAND, SENT = 3, -12345.5                                            # guard rows in front of and behind every output, their value
NAN = float("nan")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _L():
    from pdgn_amd import _lib
    _lib.ensure_scale_slots()
    return _lib.lib()


def _switch(c):
    """The case's process-wide switches (tests/conftest.py puts the defaults back)."""
    from pdgn_amd import _lib
    _lib.set_gemm_config(c.cfg)
    _lib.set_gemm_mode({"fp32": "fp32", "x2": "x2"}.get(c.mode, "x3_16" if c.shape == 16 else "x3_32"))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def pitched(x, ld, fill=NAN):
    """x (rows x cols) on the device with row pitch ld, the pad columns filled (NaN: a kernel that used one would show it)."""
    t = torch.full((x.shape[0], ld), fill, device="cuda", dtype=torch.float32)
    t[:, :x.shape[1]] = x if isinstance(x, torch.Tensor) else dev(x)
    return t


def banded(rows, ld, fill=NAN):
    full = torch.full(((rows + 2 * BAND) * ld,), SENT, device="cuda", dtype=torch.float32)
    view = full[BAND * ld:(BAND + rows) * ld].view(rows, ld)
    view.fill_(fill)
    return full, view


def bands_intact(full, rows, ld):
    return bool((full[:BAND * ld] == SENT).all()) and bool((full[(BAND + rows) * ld:] == SENT).all())


@functools.lru_cache(maxsize=2)
def device_operands(key):
    """a (M x K), w (N x K) on the device and their fp64 product (M x N) as a numpy array -- exact for the exact kinds of data."""
    M, N, K, data = key
    a, w, _, _ = gc.base_operands(M, N, K, data)
    da, dw = dev(a), dev(w)
    prod = None
    if data != "normal":
        prod = (da.double() @ dw.double().t()).cpu().numpy()
    return da, dw, prod


def test_every_required_tag_is_carried_on_this_device():
    cov = gc.coverage(_cus())
    missing = [t for t in gc.REQUIRED if not cov.get(t)]
    assert not missing, (_cus(), missing)


@pytest.mark.parametrize("case", ORDERED, ids=lambda c: c.name)
def test_launch_model_queries_equal_the_restatement(case):
    """pdgn_gemm_nt_config, the three workspace queries, the launch-info grid, the row-panel and two-part questions and the statistics
    geometry under the case's switches against tests/gemm_cases.py at this device's CU count."""
    _switch(case)
    gc.check_launch_model_queries(_L(), case, _cus())


def _planes(L, c, w_dev, N, K, ldw_pad, stream):
    """The second operand's planes from pdgn_split_bf16x3 / pdgn_split_f16x2 (direct calls: they work at any size)."""
    from pdgn_amd._lib import ptr
    parts = 3 if c.entry == "ps3" else 2
    ld = gc.cdiv(K, 8) * 8 + ldw_pad
    stride = N * ld + 8
    buf = torch.full((parts * stride + 2 * N + 16,), 0x7fc1, device="cuda", dtype=torch.int16)      # (a NaN in either format)
    src = pitched(w_dev, K + 4)
    fn = L.pdgn_split_bf16x3 if parts == 3 else L.pdgn_split_f16x2
    assert fn(N, K, ptr(src), K + 4, ptr(buf), ld, stride, None, 0, 0, stream) == 0
    return buf, ld, stride, parts


def _run(L, c, d, da, dw, o, ws_mode):
    """One call of the case's entry point.  ws_mode: "ws" (the workspace the query asks for), "short" (one float less), "none".
    Returns (C as numpy M x N, statistics partials or None)."""
    from pdgn_amd._lib import ptr, stream_of
    M, N, K = d["M"], d["N"], d["K"]
    st = stream_of(da)
    pa, pw, pc, padd = c.pads
    stats = "stats" in c.epi
    keep = []
    if c.entry in ("tn_big", "tn"):
        ldc = N
    else:
        ldc = N + pc
    cfull, C = banded(M, ldc, 0.0 if "zeroed" in c.epi else NAN)
    part = pfull = None
    if stats:
        plain = int(not any(e in c.epi for e in ("bias", "addend", "rb1", "rb12", "act", "gate")))
        nrows = (L.pdgn_gemm_nt_ps_stat_rows(M, N, K, 2, plain) if c.entry == "ps2" else L.pdgn_gemm_nt_stat_rows(M, N, K))
        pfull, part = banded(nrows, 3 * N)
    bias = dev(o["bias"]) if o["bias"] is not None else None
    add = pitched(o["addend"], N + padd) if o["addend"] is not None else None
    rb = pitched(o["row_bias"], N + padd) if o["row_bias"] is not None else None
    gate = pitched(o["gate"], N + padd, 1.0) if o["gate"] is not None else None
    act = 2 if "act" in c.epi else 0
    need = d["ws_floats"]
    wsfull = None
    if need and ws_mode != "none":
        wsfull = torch.full((need + 2048,), SENT, device="cuda", dtype=torch.float32)
        assert L.pdgn_gemm_set_tail_workspace(ptr(wsfull[1024:]), need if ws_mode == "ws" else need - 1) == 0
    if "hand" in c.epi:
        ma, mw = dev(gc.absmax_bits(o["a"], 1).view(np.int32)), dev(gc.absmax_bits(o["w"], 1).view(np.int32))
        keep += [ma, mw]
        assert L.pdgn_gemm_set_operand_scales(ptr(ma), ptr(mw)) == 0
    if c.entry == "tn":
        C.zero_()                                                  # (pdgn_gemm_tn: the caller zero-fills)
        dy, x = da.t().contiguous(), dw.t().contiguous()
        rc = L.pdgn_gemm_tn(K, M, N, ptr(dy), ptr(x), ptr(C), st)
    elif c.entry == "tn_big":
        dy, x = pitched(da.t(), M + pa), pitched(dw.t(), N + pw)
        rc = L.pdgn_gemm_tn_big(K, M, N, ptr(dy), M + pa, ptr(x), N + pw, ptr(C), int("zeroed" in c.epi), st)
    elif c.entry in ("nn", "ex_t"):
        A, Wt = pitched(da, K + pa), pitched(dw.t(), N + pw)
        if c.entry == "nn":
            rc = L.pdgn_gemm_nn(M, N, K, ptr(A), K + pa, ptr(Wt), N + pw, ptr(bias), ptr(add), N + padd if add is not None else 0, ptr(C), ldc,
                                ptr(part), st)
        else:
            rc = L.pdgn_gemm_nt_ex(M, N, K, ptr(A), K + pa, ptr(Wt), N + pw, ptr(bias), ptr(add), N + padd if add is not None else 0, ptr(C), ldc,
                                   ptr(part), ptr(rb), N + padd, o["rpg"], act, ptr(gate), N + padd, 1, st)
    elif c.entry in ("ps3", "ps2"):
        A = pitched(da, K + pa)
        buf, ld, stride, parts = _planes(L, c, dw, N, K, pw, st)
        rc = L.pdgn_gemm_nt_ps(M, N, K, ptr(A), K + pa, ptr(buf), ld, stride, parts, ptr(bias), ptr(add), N + padd if add is not None else 0,
                               ptr(C), ldc, ptr(part), ptr(rb), N + padd, o["rpg"], act, ptr(gate), N + padd, st)
    else:
        A, W = pitched(da, K + pa), pitched(dw, K + pw)
        if c.entry == "nt":
            rc = L.pdgn_gemm_nt(M, N, K, ptr(A), K + pa, ptr(W), K + pw, ptr(bias), ptr(add), N + padd if add is not None else 0, ptr(C), ldc,
                                ptr(part), st)
        else:
            rc = L.pdgn_gemm_nt_ex(M, N, K, ptr(A), K + pa, ptr(W), K + pw, ptr(bias), ptr(add), N + padd if add is not None else 0, ptr(C), ldc,
                                   ptr(part), ptr(rb), N + padd, o["rpg"], act, ptr(gate), N + padd, 0, st)
    assert rc == 0, (c.name, ws_mode, rc)
    torch.cuda.synchronize()
    assert bands_intact(cfull, M, ldc), "the output's guard rows were written"
    assert bool(torch.isnan(C[:, N:]).all()), "the output's pad columns were written"
    if wsfull is not None:
        assert bool((wsfull[:1024] == SENT).all()) and bool((wsfull[1024 + need:] == SENT).all()), "the workspace was overrun"
        if ws_mode == "ws":
            assert bool((wsfull[1024:1024 + need] != SENT).any()), "the workspace was handed over and not used: an atomic tail"
        if ws_mode == "short":
            assert bool((wsfull == SENT).all()), "a workspace one float too small must not be used"
    if pfull is not None:
        assert bands_intact(pfull, part.shape[0], 3 * N)
    return C[:, :N].cpu().numpy(), (part.cpu().numpy() if part is not None else None)


def _check_stats(c, part, y32, block_rows, exact):
    """sum (x - pv) | sum (x - pv)^2 | pv per block of block_rows rows of the float32 result; the blocks past the last row hold no sum."""
    M, N = y32.shape
    want = gc.stat_reference(y32, block_rows)
    got = part.reshape(part.shape[0], 3, N).astype(F64)
    nb = want.shape[0]
    assert part.shape[0] >= nb
    assert np.array_equal(got[:nb, 2], want[:, 2]), "pv is the block's first row"
    if exact:
        assert np.array_equal(got[:nb, 0], want[:, 0]) and np.array_equal(got[:nb, 1], want[:, 1])
    else:
        # inexact values: the block's fp32 sums within (rows + 4) 2^-23 of the sums of magnitudes
        for b in range(nb):
            blk = y32[b * block_rows:(b + 1) * block_rows].astype(F64)
            dd = np.abs(blk - blk[:1])
            u = (block_rows + 4) * gc.U
            assert np.all(np.abs(got[b, 0] - want[b, 0]) <= u * dd.sum(0)) and np.all(np.abs(got[b, 1] - want[b, 1]) <= u * (dd * dd).sum(0))
    assert not got[nb:, :2].any(), "blocks past the last row must hold empty sums"


@pytest.mark.parametrize("case", ORDERED, ids=lambda c: c.name)
def test_case_against_the_exact_reference(case):
    c, cus, L = case, _cus(), _L()
    _switch(c)
    d = gc.describe(c, cus)
    M, N, K = d["M"], d["N"], d["K"]
    da, dw, prod = device_operands(gc.operand_key(c))
    o = gc.operands(c)
    ref = gc.reference(c, product=prod)
    exact = c.data != "normal"
    stats = "stats" in c.epi
    if exact:
        ref32 = ref.astype(F32)
        assert np.array_equal(ref32.astype(F64), ref), "the exact result must be representable in float32"
    else:
        bound = (K + 4) * gc.U * (np.abs(o["a"]).astype(F64) @ np.abs(o["w"]).astype(F64).T)
    if stats:
        block = gc.stat_block_rows(c, cus)
        lib_block = (L.pdgn_gemm_nt_ps_stat_block_rows(M, N, K, 2, int(c.epi == ("stats",))) if c.entry == "ps2"
                     else L.pdgn_gemm_nt_stat_block_rows(M, N, K))
        assert lib_block == block
    ways = gc.tail_ways(d)
    for way in ways:
        got, part = _run(L, c, d, da, dw, o, way)
        assert np.isfinite(got).all(), (c.name, way)
        if exact:
            bad = got != ref32
            assert not bad.any(), (c.name, way, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], ref32[bad][:4])
        else:
            err = np.abs(got.astype(F64) - ref)
            assert np.all(err <= bound), (c.name, way, float((err / np.maximum(bound, 1e-300)).max()))
        if stats:
            # (exact sums: integer results only -- not behind LeakyReLU's 0.01f, not over rows of different binary scales)
            _check_stats(c, part, got, block, c.data in ("int", "int1") and "act" not in c.epi and "gate" not in c.epi)


# ---------------------------------------------------------------------------- the split kernels against the numpy mirrors
def _split_input():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((70, 40)) * np.exp2(rng.integers(-20, 20, size=(70, 1))) * np.exp2(rng.integers(-18, 1, size=(70, 40)))).astype(F32)
    x[rng.random(x.shape) < 0.1] = 0.0
    return np.concatenate([x, gc.edge_rows(40)])                     # 78 x 40: neither a multiple of 32


def _same_bits_or_nan(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint16 if got.dtype == np.float16 else np.uint32)[~nan],
                          want.view(np.uint16 if want.dtype == np.float16 else np.uint32)[~nan]), what


def test_split_bf16x3_planes_equal_the_mirror():
    """Planes, transposed planes, the pad columns [cols, ld) at zero, nothing written between or behind the planes; ragged rows and
    columns, the edge values of gemm_cases.edge_rows.  Above 3.3962e38 the h part is infinite (and l a NaN) on the device as in the
    mirror."""
    from pdgn_amd._lib import ptr, stream_of
    L = _L()
    x = _split_input()
    rows, cols = x.shape
    ld, ldt = 48, 88
    stride, stride_t = rows * ld + 8, cols * ldt + 16
    src = pitched(x, cols + 4)
    P = torch.full((3 * stride + 8,), 0x7fc1, device="cuda", dtype=torch.int16)
    PT = torch.full((3 * stride_t + 8,), 0x7fc1, device="cuda", dtype=torch.int16)
    assert L.pdgn_split_bf16x3(rows, cols, ptr(src), cols + 4, ptr(P), ld, stride, ptr(PT), ldt, stride_t, stream_of(src)) == 0
    torch.cuda.synchronize()
    p, pt = P.cpu().numpy().view(np.uint16), PT.cpu().numpy().view(np.uint16)
    for i, part in enumerate(gc.split_bf16x3(x)):
        plane = p[i * stride:i * stride + rows * ld].reshape(rows, ld)
        got = (plane[:, :cols].astype(np.uint32) << 16).view(F32)
        _same_bits_or_nan(got, part, "plane %d" % i)
        assert not plane[:, cols:].any(), "pad columns hold zeros"
        assert (p[i * stride + rows * ld:(i + 1) * stride] == 0x7fc1).all()
        plane_t = pt[i * stride_t:i * stride_t + cols * ldt].reshape(cols, ldt)
        _same_bits_or_nan((plane_t[:, :rows].astype(np.uint32) << 16).view(F32), np.ascontiguousarray(part.T), "transposed plane %d" % i)
        assert not plane_t[:, rows:].any()
        assert (pt[i * stride_t + cols * ldt:(i + 1) * stride_t] == 0x7fc1).all()
    assert (p[3 * stride:] == 0x7fc1).all() and (pt[3 * stride_t:] == 0x7fc1).all()
    # planes that do not hold whole rows are refused: the last row's pad columns would be written into the next plane / past the third
    for fn in (L.pdgn_split_bf16x3, L.pdgn_split_f16x2):
        assert fn(rows, cols, ptr(src), cols + 4, ptr(P), ld, (rows - 1) * ld + cols, None, 0, 0, stream_of(src)) == -1
        assert fn(rows, cols, ptr(src), cols + 4, None, 0, 0, ptr(PT), ldt, (cols - 1) * ldt + rows + 2, stream_of(src)) == -1


def test_split_f16x2_planes_and_maxima_equal_the_mirror():
    """The two scaled fp16 planes, the rows' maxima at element offset 2 plane_stride, the transposed planes (scaled by the COLUMN
    maxima, which sit behind them), pads at zero; all-zero and subnormal rows (e clamps to 126), 65504, magnitudes near 1e38."""
    from pdgn_amd._lib import ptr, stream_of
    L = _L()
    x = _split_input()
    rows, cols = x.shape
    ld, ldt = 48, 88
    stride, stride_t = rows * ld + 8, cols * ldt + 16
    src = pitched(x, cols + 4)
    P = torch.full((2 * stride + 2 * rows + 8,), 0x7fc1, device="cuda", dtype=torch.int16)
    PT = torch.full((2 * stride_t + 2 * cols + 8,), 0x7fc1, device="cuda", dtype=torch.int16)
    assert L.pdgn_split_f16x2(rows, cols, ptr(src), cols + 4, ptr(P), ld, stride, ptr(PT), ldt, stride_t, stream_of(src)) == 0
    torch.cuda.synchronize()
    p, pt = P.cpu().numpy().view(np.uint16), PT.cpu().numpy().view(np.uint16)
    rmax, cmax = gc.absmax_bits(x, 1), gc.absmax_bits(x, 0)
    assert np.array_equal(p[2 * stride:2 * stride + 2 * rows].view(np.uint32), rmax)
    assert np.array_equal(pt[2 * stride_t:2 * stride_t + 2 * cols].view(np.uint32), cmax)
    assert (p[2 * stride + 2 * rows:] == 0x7fc1).all() and (pt[2 * stride_t + 2 * cols:] == 0x7fc1).all()
    for i, (part, part_t) in enumerate(zip(gc.split_f16x2(x, rmax), gc.split_f16x2(np.ascontiguousarray(x.T), cmax))):
        plane = p[i * stride:i * stride + rows * ld].reshape(rows, ld)
        _same_bits_or_nan(np.ascontiguousarray(plane[:, :cols]).view(np.float16), part, "plane %d" % i)
        assert not plane[:, cols:].any()
        assert (p[i * stride + rows * ld:(i + 1) * stride] == 0x7fc1).all()
        plane_t = pt[i * stride_t:i * stride_t + cols * ldt].reshape(cols, ldt)
        _same_bits_or_nan(np.ascontiguousarray(plane_t[:, :rows]).view(np.float16), part_t, "transposed plane %d" % i)
        assert not plane_t[:, rows:].any()
        assert (pt[i * stride_t + cols * ldt:(i + 1) * stride_t] == 0x7fc1).all()


@pytest.mark.parametrize("rows,cols,pad", [(78, 40, 4), (1000, 132, 4), (70, 5124, 0), (4099, 64, 0), (3, 4, 0)])
def test_absmax_rows_cols_equals_numpy(rows, cols, pad):
    from pdgn_amd._lib import ptr, stream_of
    L = _L()
    rng = np.random.default_rng(rows + cols)
    x = (rng.standard_normal((rows, cols)) * np.exp2(rng.integers(-40, 40, size=(rows, 1)))).astype(F32)
    if (rows, cols) == (78, 40):
        x = _split_input()
    x[rng.random(x.shape) < 0.05] = -0.0
    src = pitched(x, cols + pad)
    rm = torch.full((rows + 8,), -1, device="cuda", dtype=torch.int32)
    cm = torch.full((cols + 8,), -1, device="cuda", dtype=torch.int32)
    for want_r, want_c in ((True, True), (True, False), (False, True)):
        rm.fill_(-1), cm.fill_(-1)
        assert L.pdgn_absmax_rows_cols(rows, cols, ptr(src), cols + pad, ptr(rm) if want_r else None, ptr(cm) if want_c else None, stream_of(src)) == 0
        torch.cuda.synchronize()
        r, cc = rm.cpu().numpy(), cm.cpu().numpy()
        if want_r:
            assert np.array_equal(r[:rows].view(np.uint32), gc.absmax_bits(x, 1))
        if want_c:
            assert np.array_equal(cc[:cols].view(np.uint32), gc.absmax_bits(x, 0))
        assert (r[rows:] == -1).all() and (cc[cols:] == -1).all() and (want_r or (r == -1).all()) and (want_c or (cc == -1).all())
