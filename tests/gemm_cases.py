"""The cases of tests/test_gpu_gemm_exact.py: the dense contraction kernels (csrc/gemm_x3.hip and its two other translation units,
csrc/gemm_nt.hip, csrc/gemm_rp.hip, csrc/split.hip) in every tile and tail regime, with their operands and references.  Shared by
the host test (tests/test_gemm_cases_host.py: guards, regime coverage, the library's queries and the split mirrors, no GPU) and the
GPU module.

The launch arithmetic of csrc/gemm_plan.h (`gemm_plan`, `gemm_dp_grid`, `gemm_tail_layout`, `gemm_at_slices`, the two pick rules,
`x2_pays`) and gemm_rp.hip's `rp_takes` and the launchers' allow_sk rule are restated here with the CU count as a parameter: the
cost formulas are IEEE double arithmetic, evaluated in the order the C++ evaluates them, so the picks reproduce exactly.
`describe` turns a case into what its call launches, `reached` into the regime tags it enters, REQUIRED lists the tags that at
least one case must carry, and `check_launch_model_queries` compares the built library's queries with the restatement.

Four kinds of data, each with a guard that the host test checks for every case that uses it:
  "int"          float32 integers with |v| <= 7, zeros included; row r of an operand (as the kernel sees it) is capped at
                 INT_CAPS[r % 8] (a cap of 0 is an all-zero row), so that the rows' maxima -- the two-part mode's scales -- differ
                 from row to row.  Every product and every partial sum, in any order, is an integer below 2^24 (`exact_guard`, the
                 epilogue's terms included): every mode, tile, instruction shape and tail form -- the fp32 atomics of a stream-K
                 tail too -- returns the int64 product bit for bit.  LeakyReLU's 0.01f is no dyadic number: where it applies the
                 reference is ONE float32 multiply of the exact value.  Cases with statistics partials take values in {-1, 0, 1}
                 (`stat_guard`: the squared sums of a block stay below 2^24) and the three fields are exact integers too.
  "two_level"    A[m, :] = 2^s_m (p + q 2^-12), p in {+-1, +-2}, q in {-1, 0, 1}, s_m in [-20, 20] per row; W[n, :] = 2^t_n v with
                 integers |v| <= 3 ("two_level_w": the operands swapped).  One operand has one part only, so every product is
                 ah wh + (am | al) wh: terms that both split arithmetics keep, each exact.  Guard per output, in units of the
                 quantum 2^-12: sum_k |a / 2^s| |w / 2^t| < 2^12; the k = 1028 cases thin W until it holds.  Expected: the fp64
                 product, which is representable in float32 (asserted), bit for bit.  A wrong row's scale, a scale applied to the
                 wrong side or a dropped low part fails outright.
  "three_level"  (x3 and fp32, k <= 64, and one stream-K tail at k = 1028) a third level, p + q 2^-10 + r 2^-19: the bf16 split has
                 a non-zero l for 4/9 of the values (h = p, m = q 2^-10, l = r 2^-19 -- the mirror reassembles every value
                 exactly); guard with quantum 2^-19, which the one-part operand meets with at most five non-zeros per row.
                 ("three_level_w": swapped.)
  "normal"       random normal data for what exact data cannot reach, BOTH operands with low parts.  The reference is the numpy
                 mirror of the arithmetic -- the six (x3) or three (x2) partial products of the mirrored parts, summed in fp64; all
                 of them under fp32 -- and the bound the fp32 accumulation's, (K + 4) 2^-23 sum |a||w| (U, as in
                 tests/persample_cases.py): it separates the split's error from the accumulation's.

No GPU import in this file."""
import collections
import functools

import numpy as np

F32, F64 = np.float32, np.float64
SLOPE = np.float32(0.01)
LIMIT = 2 ** 24
U = 2.0 ** -23                                                      # the product bound's unit: (K + 4) U sum|a||w|
NT_BK, GROUP_M = 32, 8
INT_CAPS = (7, 3, 1, 7, 2, 0, 5, 7)


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------- the launch arithmetic, restated
# fam "x3": gemm_plan.h's X3_TILES (gemm_x3.hip's X3Big, X3Square, X3Narrow); fam "fp32": FP32_TILES (gemm_nt.hip's NtBig, NtSquare,
# NtTall, NtNarrow).  WG: workgroups per CU; stat_div: a statistics block is BM / stat_div rows (one per wave row).
Tile = collections.namedtuple("Tile", "fam cfg BM BN WG rate stat_div")
X3_TILES = (Tile("x3", 0, 256, 128, 1, 760, 2), Tile("x3", 1, 128, 128, 1, 660, 2), Tile("x3", 2, 128, 64, 2, 540, 2))
FP32_TILES = (Tile("fp32", 0, 256, 128, 1, 1.0, 4), Tile("fp32", 1, 128, 128, 2, 1.0, 2), Tile("fp32", 2, 160, 64, 2, 0.95, 2),
              Tile("fp32", 3, 128, 64, 3, 0.95, 2))
TILES = {"x3": X3_TILES, "fp32": FP32_TILES}
Plan = collections.namedtuple("Plan", "tiles_m tiles_n kchunks grid_dp dp_tiles grid_sk sk_per_wg cost rounds tail slots")
Tail = collections.namedtuple("Tail", "t_tail s_tail per_tail grid seg per_flat floats")


def chunk_us(tile, w):
    if tile.fam == "x3":
        return 2.0 * tile.BM * tile.BN * NT_BK * w / (tile.rate * 1e3)
    return 2.0 * tile.BM * tile.BN * NT_BK * w / (0.56e6 * tile.rate)


def dp_grid(tile, tiles, slots, kc):
    tpw = ((64 if tile.fam == "x3" else 32) + kc - 1) // kc
    tpw = 1 if tpw < 1 else (8 if tpw > 8 else tpw)
    g = (tiles + tpw - 1) // tpw
    lo = tiles if tiles < slots else slots
    return lo if g < lo else g


def plan(tile, m, n, k, allow_sk, cus):
    """gemm_plan.h::gemm_plan."""
    tiles_m, tiles_n, kc = cdiv(m, tile.BM), cdiv(n, tile.BN), cdiv(k, NT_BK)
    T = tiles_m * tiles_n
    slots = cus * tile.WG
    rounds = T // slots
    tail = T - rounds * slots
    ov = 2.0 if tile.fam == "x3" else 2.5
    full = float(rounds) * (kc + ov) * chunk_us(tile, tile.WG)
    dp_tiles, grid_dp, grid_sk, sk_per_wg = T, dp_grid(tile, T, slots, kc), 0, 0
    cost = full + ((kc + ov) * chunk_us(tile, (tail + cus - 1) // cus) if tail else 0.0)
    if allow_sk and tail > 0:
        iters = tail * kc
        for cand in (slots, cus, iters // 16):
            g = 1 if cand < 1 else (slots if cand > slots else cand)
            g = g if g < iters else iters
            per = (iters + g - 1) // g
            if per < 8 and g > 1:
                continue
            g = (iters + per - 1) // per
            zero_rows = float(m - ((rounds * slots) // (GROUP_M * tiles_n)) * GROUP_M * tile.BM)
            c = (full + (per + ov) * chunk_us(tile, (g + cus - 1) // cus) + float(g + tail) * tile.BM * tile.BN * 4 / 1.3e6 +
                 zero_rows * n * 4 / 3.0e6 + 4.0)
            if c < cost:
                cost, dp_tiles = c, rounds * slots
                grid_dp = dp_grid(tile, rounds * slots, slots, kc) if rounds else 0
                grid_sk, sk_per_wg = g, per
    return Plan(tiles_m, tiles_n, kc, grid_dp, dp_tiles, grid_sk, sk_per_wg, cost, rounds, tail, slots)


def tail_layout(tile, pl, cus):
    """gemm_plan.h::gemm_tail_layout: how the stream-K tail of a plan is laid out when its partial tiles go to a workspace."""
    if not pl.grid_sk:
        return Tail(0, 0, 0, 0, 0, 0, 0)
    T, slots = pl.tiles_m * pl.tiles_n, cus * tile.WG
    t_tail = T - pl.dp_tiles
    s_tail = max(1, slots // t_tail)
    s_tail = min(s_tail, pl.kchunks)
    per_tail = cdiv(pl.kchunks, s_tail)
    s_tail = cdiv(pl.kchunks, per_tail)
    grid = s_tail * t_tail
    iters = t_tail * pl.kchunks
    if grid * 5 < slots * 4 and iters >= slots * 8:
        per_flat = cdiv(iters, slots)
        grid = cdiv(iters, per_flat)
        seg = (per_flat + pl.kchunks - 2) // pl.kchunks + 1
        return Tail(t_tail, s_tail, per_tail, grid, seg, per_flat, grid * seg * tile.BM * tile.BN)
    return Tail(t_tail, s_tail, per_tail, grid, 0, 0, grid * tile.BM * tile.BN)


def at_slices(tile, pl, cus):
    """gemm_plan.h::gemm_at_slices: non-empty k slices per tile of a split-K weight gradient."""
    T, slots = pl.tiles_m * pl.tiles_n, cus * tile.WG
    S = min(slots // T, pl.kchunks)
    per = cdiv(pl.kchunks, S)
    return cdiv(pl.kchunks, per)


def pick(fam, m, n, k, stats, cus, forced=None, no_tall=False):
    """gemm_plan.h::gemm_pick_x3 / gemm_pick_fp32: the tile configuration, forced or the launch model's."""
    if fam == "x3":
        if forced is not None:
            return 2 if forced > 2 else forced
        c = [plan(t, m, n, k, not stats, cus).cost for t in X3_TILES]
        best = 0
        for i in (1, 2):
            if c[i] < c[best]:
                best = i
        return best
    if forced is not None:
        return 1 if (no_tall and forced == 2) else forced
    c = [plan(t, m, n, k, not stats, cus).cost for t in FP32_TILES]
    best = 1
    for i in range(4):
        if c[i] < c[best] * 0.97 and not (no_tall and i == 2):
            best = i
    return best


def x2_pays(mode, cfg, m, n, k, scan_bytes):
    if mode != "x2" or cfg != 0 or k < 128 or m >= (1 << 28):
        return False
    flops = 2.0 * float(m) * n * k
    return flops >= 2e10 and float(scan_bytes) <= 4.5e-3 * flops


def rp_takes(m, n, k):
    return k in (32, 64, 128) and n >= 128 and m >= 4096 and float(m) * n >= 1.6e7 and m < (1 << 28)


# ---------------------------------------------------------------------------- the split mirrors
def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even) as float32: v_cvt_pk_bf16_f32 (finite values; a value that rounds past the largest
    bf16, above 2^127 (2 - 2^-8), becomes infinity as on the device)."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return r.astype(np.uint32).view(F32)


def split_bf16x3(x):
    """split.hip::sp_split / gemm_x3.hip::x3_split_pair: h = rn(x), m = rn(x - h), l = rn(x - h - m), the remainders exact in fp32.
    Returns the three parts as float32 arrays."""
    x = np.ascontiguousarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = bf16_rne(x)
        ra = (x - h).astype(F32)
        m = bf16_rne(ra)
        sa = (ra - m).astype(F32)
        return h, m, bf16_rne(sa)


def absmax_bits(x, axis):
    """The maxima of |x| along an axis as bit patterns (unsigned order = magnitude order)."""
    x = np.ascontiguousarray(x, dtype=F32)
    return (x.view(np.uint32) & 0x7fffffff).max(axis=axis).astype(np.uint32)


def x2_exponent(maxbits):
    """gemm_shared.h::x2_exponent: e = 14 - floor(log2 max), clamped to +-126 (a zero or subnormal maximum: field 0 -> 126)."""
    e = 14 - ((np.asarray(maxbits, dtype=np.int64) >> 23) - 127)
    return np.clip(e, -126, 126)


def x2_scale_field(maxbits):
    """gemm_shared.h::x2_scale_field: the exponent field of 2^e, 268 - field(max), clamped to 1 .. 253."""
    return np.clip(268 - (np.asarray(maxbits, dtype=np.int64) >> 23), 1, 253)


def x2_scale(maxbits):
    return (x2_scale_field(maxbits).astype(np.uint32) << 23).view(F32)


def x2_unscale(maxbits):
    return ((254 - x2_scale_field(maxbits)).astype(np.uint32) << 23).view(F32)


def split_f16x2(x, maxbits):
    """split.hip::sp_split2 / gemm_x3.hip::conv_pair (NP = 2) for a matrix whose ROWS have the maxima `maxbits`: x 2^e (a float32
    multiply), h = rn16 of it, l = rn16 of the float32 remainder.  Returns (h, l) as float16 arrays."""
    x = np.ascontiguousarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        a2 = (x * x2_scale(maxbits)[:, None]).astype(F32)
        h = a2.astype(np.float16)
        l = (a2 - h.astype(F32)).astype(F32).astype(np.float16)
    return h, l


def mirror_product(a, w, mode):
    """What the split arithmetic multiplies, summed in fp64: the six partial products of the bf16 parts (x3), the three of the scaled
    fp16 parts times the two un-scales (x2), all of them (fp32).  a (M x K), w (N x K) as the kernel sees them."""
    if mode == "fp32":
        return a.astype(F64) @ w.astype(F64).T
    if mode == "x3":
        ah, am, al = (p.astype(F64) for p in split_bf16x3(a))
        wh, wm, wl = (p.astype(F64) for p in split_bf16x3(w))
        return al @ wh.T + am @ wm.T + ah @ wl.T + am @ wh.T + ah @ wm.T + ah @ wh.T
    ma, mw = absmax_bits(a, 1), absmax_bits(w, 1)
    ah, al = (p.astype(F64) for p in split_f16x2(a, ma))
    wh, wl = (p.astype(F64) for p in split_f16x2(w, mw))
    s = al @ wh.T + ah @ wl.T + ah @ wh.T
    return s * x2_unscale(ma).astype(F64)[:, None] * x2_unscale(mw).astype(F64)[None, :]


# ---------------------------------------------------------------------------- the cases
# entry: nt | nn | ex | ex_t (pdgn_gemm_nt_ex, transposed_w 0 / 1) | ps3 | ps2 (pdgn_gemm_nt_ps, three bf16 / two fp16 planes) |
#        tn_big | tn.  m, n, k are the ENTRY POINT's (tn_big / tn: m is the reduction, dW is n x k).
# mode:  fp32 | x3 | x2;  cfg: None (the launch model's pick) or a forced tile;  shape: 32 | 16 (pdgn_gemm_set_shape, x3 only).
# epi:   a tuple of "bias", "addend", "stats", "rb1" / "rb12" (row_bias, rows_per_group 1 / 12), "act", "gate", "hand" (both operands'
#        maxima handed over with pdgn_gemm_set_operand_scales), "zeroed" (tn_big: dw_is_zero = 1 on a zeroed dW).
# pads:  (lda - cols(A), ldw - cols(W), ldc - n, ldadd - n), multiples of 4 (planes: ldw is cols rounded up to 8, + pads[1]).
Case = collections.namedtuple("Case", "name entry m n k mode cfg shape epi pads data")
NOPAD = (0, 0, 0, 0)


def _c(name, entry, m, n, k, mode, cfg=None, shape=32, epi=(), pads=NOPAD, data="int"):
    return Case(name, entry, m, n, k, mode, cfg, shape, tuple(epi), tuple(pads), data)


def kernel_dims(c):
    """(M, N, K) as the kernel sees them: a weight gradient's rows are dY's columns, its reduction the rows."""
    return (c.n, c.k, c.m) if c.entry in ("tn_big", "tn") else (c.m, c.n, c.k)


def has_epi(c):
    return any(e in c.epi for e in ("rb1", "rb12", "act", "gate"))


def describe(c, cus):
    """What the call of case c launches on a device of `cus` CUs: dict(fam, tile, plan, allow_sk, kernel, two, tail, at_floats, ...).
    kernel: "tile" (gemm_x3 / gemm_nt), "row_panel" (gemm_rp.hip), "tn" (gemm_tn.hip: not modelled)."""
    M, N, K = kernel_dims(c)
    d = dict(M=M, N=N, K=K, kernel="tile", two=False, splitk=False, at_floats=0, tail=Tail(0, 0, 0, 0, 0, 0, 0), ws_floats=0)
    if c.entry == "tn":
        d.update(kernel="tn", fam="tn", tile=None, plan=None, allow_sk=False)
        return d
    stats = "stats" in c.epi
    ldc = N + (0 if c.entry == "tn_big" else c.pads[2])
    allow_sk = not stats and ldc == N and not has_epi(c)
    fam = "fp32" if c.mode == "fp32" else "x3"
    plain = not any(e in c.epi for e in ("bias", "addend", "rb1", "rb12", "act", "gate"))
    if c.entry == "ps2" and c.mode == "x2" and plain and rp_takes(M, N, K):
        d.update(kernel="row_panel", fam="rp", tile=None, plan=None, allow_sk=False, two=True)
        return d
    # (a weight gradient: the pick over (n, k, m), no statistics; fp32: no_tall)
    cfg = pick(fam, M, N, K, stats or has_epi(c), cus, c.cfg, no_tall=(c.entry == "tn_big"))
    d["picked"] = cfg
    if c.entry == "ps2":
        d["refused"] = stats and cfg != 0                            # (a launch with partials keeps the pick's geometry)
        cfg = 0
    tile = TILES[fam][cfg]
    pl = plan(tile, M, N, K, allow_sk, cus)
    d.update(fam=fam, tile=tile, plan=pl, allow_sk=allow_sk)
    if fam == "fp32":
        return d
    scan = 0 if "hand" in c.epi else (M * K + N * K) * 4
    d["two"] = c.entry == "ps2" or (c.entry in ("nt", "nn", "ex", "ex_t", "tn_big") and x2_pays(c.mode, cfg, M, N, K, scan))
    d["eight_waves"] = d["two"] and not stats
    T = pl.tiles_m * pl.tiles_n
    if c.entry == "tn_big":
        d["splitk"] = T <= cus * tile.WG
        if d["splitk"]:
            d["at_floats"] = at_slices(tile, pl, cus) * T * tile.BM * tile.BN
            d["ws_floats"] = d["at_floats"]
        return d
    d["tail"] = tail_layout(tile, pl, cus)
    d["ws_floats"] = d["tail"].floats
    return d


def tail_ways(d):
    """How the GPU module runs a described case: a call that wants a workspace (a stream-K tail or a split-K weight gradient on the
    matrix cores) runs with it ("ws"), with one a float too small ("short": must fall back to the atomics) and with none."""
    return ("ws", "short", "none") if d["ws_floats"] else ("none",)


def check_launch_model_queries(L, c, cus):
    """pdgn_gemm_nt_config, the three workspace queries, the launch-info grid, the row-panel and two-part questions and the statistics
    geometry of the library L (the ctypes handle, case c's switches in force) against this module's restatement at `cus` CUs -- the
    device's count, or the 256 the library assumes where it finds no device.  Host-side queries only: nothing is launched."""
    import ctypes
    M, N, K = kernel_dims(c)
    fam = "fp32" if c.mode == "fp32" else "x3"
    for ws in (0, 1):
        t = pick(fam, M, N, K, bool(ws), cus, c.cfg)
        tile = TILES[fam][t]
        pl = plan(tile, M, N, K, not ws, cus)
        assert L.pdgn_gemm_nt_config(M, N, K, ws) == t + (16 if pl.grid_sk else 0), (ws, t, pl)
        floats = 0 if fam == "fp32" else tail_layout(tile, pl, cus).floats
        assert L.pdgn_gemm_tail_workspace_floats(M, N, K, ws) == floats, (ws, t, pl)
        assert (floats > 0) == (fam == "x3" and pl.grid_sk > 0)
        if fam == "x3":
            assert L.pdgn_gemm_nt_ps_workspace_floats(M, N, K, 3, ws) == floats
            # two-part planes run on the 256 x 128 tile: its tail's floats, none with statistics.  The library answers 0 outright for a
            # shape the row-panel kernel can take, whatever the mode and the epilogue; that is no quirk to pin, because such a shape
            # (k <= 128: at most 4 chunks) never plans a tail on this tile -- asserted here from the restated plan, not from the rule
            big = X3_TILES[0]
            two = 0 if ws else tail_layout(big, plan(big, M, N, K, True, cus), cus).floats
            assert not (rp_takes(M, N, K) and two), "a row-panel shape that plans a tail: the library's shortcut would lose it"
            assert L.pdgn_gemm_nt_ps_workspace_floats(M, N, K, 2, ws) == two, ws
    ts = TILES[fam][pick(fam, M, N, K, True, cus, c.cfg)]
    assert L.pdgn_gemm_nt_stat_rows(M, N, K) == cdiv(M, ts.BM) * ts.stat_div
    assert L.pdgn_gemm_nt_stat_block_rows(M, N, K) == ts.BM // ts.stat_div      # BM / 4 on the big fp32 tile, BM / 2 elsewhere
    if fam == "fp32":
        assert L.pdgn_gemm_tn_big_workspace_floats(M, N, K) == 0 and L.pdgn_gemm_two_part(M, N, K, 0) == 0
        return
    for parts in (3, 2):
        sym, grid = ctypes.c_void_p(), ctypes.c_int(-1)
        assert L.pdgn_gemm_nt_ps_launch_info(M, N, K, parts, ctypes.byref(sym), ctypes.byref(grid)) == 0
        tile = X3_TILES[0 if parts == 2 else pick("x3", M, N, K, False, cus, c.cfg)]
        assert grid.value == plan(tile, M, N, K, True, cus).grid_dp, (parts, tile)
        for plain in (0, 1):
            takes = c.mode == "x2" and parts == 2 and plain == 1 and rp_takes(M, N, K)
            assert L.pdgn_gemm_nt_ps_row_panel(M, N, K, parts, plain) == int(takes)
            assert L.pdgn_gemm_nt_ps_stat_block_rows(M, N, K, parts, plain) == (256 if takes else ts.BM // ts.stat_div)
            assert L.pdgn_gemm_nt_ps_stat_rows(M, N, K, parts, plain) == (cdiv(M, 256) if takes else cdiv(M, ts.BM) * ts.stat_div)
    for scan in (0, (M * K + N * K) * 4):
        assert L.pdgn_gemm_two_part(M, N, K, scan) == int(x2_pays(c.mode, pick("x3", M, N, K, False, cus, c.cfg), M, N, K, scan))
    # the weight gradient of the same kernel-side problem: dW (M x N) over K rows
    d = describe(c._replace(entry="tn_big", m=K, n=M, k=N, epi=(), pads=NOPAD), cus)
    assert L.pdgn_gemm_tn_big_workspace_floats(K, M, N) == d["at_floats"], d
    d = describe(c, cus)
    if d["kernel"] == "tile" and c.entry != "tn_big":
        assert d["ws_floats"] == (d["tail"].floats if d["plan"].grid_sk else 0)


def reached(c, cus):
    """The regime tags case c enters on a device of `cus` CUs."""
    d = describe(c, cus)
    M, N, K = d["M"], d["N"], d["K"]
    tags = {"mode:" + c.mode, "entry:" + c.entry, "data:" + c.data}
    if d["kernel"] == "tn":
        return tags
    if d["kernel"] == "row_panel":
        tags |= {"loader:row_panel", "loader:row_panel_k%d" % K}
        if "stats" in c.epi:
            tags.add("epi:stats_row_panel")
        return tags
    tile, pl = d["tile"], d["plan"]
    fam = "x2" if d["two"] else d["fam"]
    pre = "%s.%d:" % (fam, tile.cfg)
    T = pl.tiles_m * pl.tiles_n
    t = set()
    if T == 1 and (M < tile.BM or N < tile.BN):
        t.add("one_partial_tile")
    if K % NT_BK:
        t.add("k_tail")
    if K == 4:
        t.add("k4")
    if M % tile.BM:
        t.add("ragged_m")
    if N % tile.BN:
        t.add("ragged_n")
    if pl.tiles_m > GROUP_M and pl.tiles_m % GROUP_M:
        t.add("multigroup")
    if d["splitk"]:
        tags |= {"loader:tn_big_splitk", pre + "tn_big_splitk"}
    else:
        if c.entry == "tn_big" and d["fam"] == "x3":                  # (the fp32 weight gradient has one path only)
            tags |= {"loader:tn_big_general", pre + "tn_big_general"}
        if pl.rounds >= 1 and not pl.grid_sk:
            t.add("rounds_no_tail")
        if pl.grid_dp and pl.grid_sk:
            t.add("rounds_plus_tail")
        if pl.grid_sk and not pl.grid_dp:
            t.add("tail_only")
        if pl.grid_sk and d["fam"] == "x3" and c.entry != "tn_big":
            ways = tail_ways(d)
            if "ws" in ways:
                t.add("tail_flat" if d["tail"].seg >= 2 else "tail_aligned")      # (a flattened layout has seg >= 2: per_flat >= 8)
            if "short" in ways and "none" in ways:
                t.add("tail_atomic")
    tags |= {pre + x for x in t}
    if c.entry == "nt":
        tags.add("loader:nt")
    if c.entry in ("nn", "ex_t"):
        tags.add("loader:nn")
    if c.entry == "ps3":
        tags.add("loader:presplit3")
    if c.entry == "ps2":
        tags.add("loader:presplit2_eight_waves" if d["eight_waves"] else "loader:presplit2_four_waves")
    if d["two"] and c.entry in ("nt", "nn", "tn_big"):
        tags.add("loader:two_part_unsplit_" + c.entry)
    if c.mode != "fp32" and not d["two"]:
        tags.add("shape:%d" % c.shape)
    for e in c.epi:
        if e not in ("hand", "zeroed"):
            tags.add("epi:" + e)
    if {"bias", "addend", "stats", "rb12", "act", "gate"} <= set(c.epi):
        tags.add("epi:all")
    if c.pads[0] and c.pads[1]:
        tags.add("epi:strided_operands")
    if c.entry != "tn_big" and c.pads[2]:
        tags.add("epi:ldc_forbids_tail")
    if "addend" in c.epi and c.pads[3]:
        tags.add("epi:addend_ldadd")
    return tags


# The regime shapes (m, n, k), found with this module's own restatement at 256 CUs; `reached` decides, not this list.
def _regimes(fam, cfg, mode, entry="nt", shape=32, label=None):
    """One case per tile / tail regime of a tile; cfg is forced (the model's own pick is covered by the loader and epilogue cases)."""
    big, sq = cfg == 0, cfg == 1
    shapes = [("partial", 100, 8, 4), ("multigroup", 2400 if big else 1100, 8, 4), ("tail_only", 100, 8, 1028),
              ("tail_multigroup", 2400 if big else 1100, 8, 1028)]
    if fam == "x3":
        shapes += [("tail_flat", 17000 if cfg < 2 else 33000, 8, 1028 if cfg < 2 else 516),
                   ("rounds", 66000 if cfg != 1 else 33000, 8 if cfg < 2 else 68, 4),
                   ("rounds_tail", 66000 if cfg != 1 else 33000, 8, 1028),
                   ("rounds_flat", 9000 if cfg < 2 else 33000, 1028 if big else 520 if sq else 132, 1028)]
    else:
        wide = cfg >= 2
        shapes += [("rounds", 33000 if wide else 66000, 132 if wide else 8, 4),
                   ("rounds_tail", 33000 if wide else 66000, 132 if wide else 8, 1028)]
    tag = label or ("%s%d" % (mode, cfg))
    return [_c("%s_%s_%s" % (tag, entry, nm), entry, m, n, k, mode, cfg, shape) for nm, m, n, k in shapes]


CASES = []
for _cfg in range(3):
    CASES += _regimes("x3", _cfg, "x3")
    CASES += _regimes("x3", _cfg, "x3", shape=16, label="x3s16_%d" % _cfg)[:3]
for _cfg in range(4):
    CASES += _regimes("fp32", _cfg, "fp32")
CASES += _regimes("x3", 0, "x2", entry="ps2")                      # the two-part instances: pre-split planes at any size (256 x 128 only)

CASES += [
    # ---- loader forms, the launch model's own pick unless the tag needs a tile
    _c("nn_x3_partial", "nn", 100, 8, 4, "x3"),
    _c("nn_x3_tail", "nn", 2400, 8, 1028, "x3", 0),
    _c("nn_x3_ragged", "nn", 1100, 132, 68, "x3", pads=(4, 8, 0, 0)),
    _c("nn_x3s16_ragged", "nn", 1100, 132, 68, "x3", 1, 16),
    _c("nn_fp32_ragged", "nn", 1100, 132, 68, "fp32", pads=(4, 8, 0, 0)),
    _c("nn_fp32_tail", "nn", 2400, 8, 1028, "fp32", 0),
    _c("nt_x3_pick_ragged", "nt", 1100, 132, 68, "x3", pads=(4, 8, 0, 0)),
    _c("nt_x2_pick_ragged", "nt", 1100, 132, 68, "x2"),
    _c("nt_fp32_pick_ragged", "nt", 1100, 132, 68, "fp32", pads=(4, 8, 0, 0)),
    _c("ps3_x3_partial", "ps3", 100, 8, 4, "x3"),
    _c("ps3_x3_k12", "ps3", 300, 132, 12, "x3", pads=(4, 8, 0, 0)),
    _c("ps3_x3_tail_big", "ps3", 2400, 8, 1028, "x3", 0),
    _c("ps3_x3_tail_flat_square", "ps3", 17000, 8, 1028, "x3", 1),
    _c("ps3_x3_rounds_tail_narrow", "ps3", 66000, 8, 1028, "x3", 2),
    _c("ps3_x3s16_tail_big", "ps3", 2400, 8, 1028, "x3", 0, 16),
    _c("ps3_x3s16_ragged_narrow", "ps3", 1100, 132, 68, "x3", 2, 16),
    _c("ps2_x2_ragged", "ps2", 1100, 132, 68, "x2", pads=(4, 8, 0, 0)),
    _c("ps2_x3mode_ragged", "ps2", 1100, 132, 68, "x3"),
    _c("ps2_x3mode_row_panel_shape", "ps2", 4099, 3908, 32, "x3"),        # (only mode x2 has the row panel: two-part planes on the tile kernel here)
    _c("ps2_x2_four_waves_stats", "ps2", 1100, 132, 68, "x2", 0, epi=("stats",), data="int1"),
    _c("ps2_x2_four_waves_bias_stats", "ps2", 600, 260, 36, "x2", 0, epi=("bias", "addend", "stats"), data="int1"),
    _c("ps2_x2_row_panel_k128", "ps2", 4099, 4100, 128, "x2"),
    _c("ps2_x2_row_panel_k64", "ps2", 4099, 3908, 64, "x2", epi=("stats",), data="int1"),
    _c("ps2_x2_row_panel_k32", "ps2", 4099, 3908, 32, "x2"),
    _c("tn_big_x3_splitk", "tn_big", 1028, 132, 68, "x3"),
    _c("tn_big_x3_splitk_big", "tn_big", 4100, 260, 132, "x3", 0),
    _c("tn_big_x3_splitk_ragged_reduction", "tn_big", 1027, 132, 68, "x3", 2, epi=("zeroed",)),
    _c("tn_big_x3s16_splitk", "tn_big", 1028, 132, 68, "x3", 1, 16),
    _c("tn_big_x3_general", "tn_big", 100, 4100, 1028, "x3", 2),
    _c("tn_big_x3_general_zeroed", "tn_big", 68, 4100, 1028, "x3", 2, epi=("zeroed",)),
    _c("tn_big_fp32", "tn_big", 1028, 132, 68, "fp32"),
    _c("tn_big_fp32_big", "tn_big", 4100, 260, 132, "fp32", 0),
    _c("tn_small", "tn", 1000, 8, 4, "x3"),
    _c("tn_k32", "tn", 3000, 132, 32, "x3"),
    _c("tn_k256", "tn", 1027, 68, 132, "x3"),
    # ---- two parts from unsplit operands, at the x2_pays threshold (k >= 128, 20 GFLOP, the maxima handed over: a scan of zero bytes)
    _c("nt_x2_unsplit", "nt", 9000, 1084, 1028, "x2", 0, epi=("hand",)),
    _c("nn_x2_unsplit", "nn", 9000, 1084, 1028, "x2", 0, epi=("hand",)),
    _c("tn_big_x2_unsplit", "tn_big", 9000, 1028, 1084, "x2", 0, epi=("hand",)),
    _c("nt_x2_unsplit_two_level", "nt", 9000, 1084, 1028, "x2", 0, epi=("hand",), data="two_level"),
    _c("nn_x2_unsplit_two_level_w", "nn", 9000, 1084, 1028, "x2", 0, epi=("hand",), data="two_level_w"),
    _c("tn_big_x2_unsplit_two_level", "tn_big", 512, 4420, 4420, "x2", 0, epi=("hand",), data="two_level"),      # (T > slots: the general path)
]

# ---- epilogues, separately and all together, per kernel family (tile-kernel epilogues are one code path per family)
_ALL = ("bias", "addend", "stats", "rb12", "act", "gate")
for _mode, _cfgs in (("x3", (0, 1, 2)), ("fp32", (0, 1, 2, 3)), ("x2", (None,))):
    for _cfg in _cfgs:
        _t = "%s%s" % (_mode, "" if _cfg is None else _cfg)
        CASES += [_c("epi_%s_all" % _t, "ex", 600, 132, 36, _mode, _cfg, epi=_ALL, pads=(4, 8, 4, 8), data="int1"),
                  _c("epi_%s_stats" % _t, "nt", 600, 132, 36, _mode, _cfg, epi=("stats",), data="int1")]
    CASES += [
        _c("epi_%s_bias" % _mode, "nt", 300, 132, 36, _mode, epi=("bias",)),
        _c("epi_%s_addend_ldadd" % _mode, "nt", 300, 132, 36, _mode, epi=("addend",), pads=(0, 0, 0, 8)),
        _c("epi_%s_bias_addend_tail" % _mode, "nt", 2400, 8, 1028, _mode, 0, epi=("bias", "addend"), pads=(0, 0, 0, 4)),
        _c("epi_%s_rb1" % _mode, "ex", 300, 132, 36, _mode, epi=("rb1",)),
        _c("epi_%s_rb12" % _mode, "ex", 300, 132, 36, _mode, epi=("rb12",)),
        _c("epi_%s_act" % _mode, "ex", 300, 132, 36, _mode, epi=("act",)),
        _c("epi_%s_gate" % _mode, "ex", 300, 132, 36, _mode, epi=("gate",)),
        _c("epi_%s_t_all" % _mode, "ex_t", 300, 132, 36, _mode, epi=_ALL, pads=(4, 8, 4, 8), data="int1"),
        _c("epi_%s_ldc_forbids_tail" % _mode, "nt", 2400, 8, 1028, _mode, 0, pads=(4, 4, 4, 0)),
    ]
CASES += [
    _c("epi_x3s16_all", "ex", 600, 132, 36, "x3", 1, 16, epi=_ALL, pads=(4, 8, 4, 8), data="int1"),
    _c("epi_ps3_all", "ps3", 600, 132, 36, "x3", epi=_ALL, pads=(4, 8, 4, 8), data="int1"),
    _c("epi_ps2_all", "ps2", 600, 132, 36, "x2", 0, epi=_ALL, pads=(4, 8, 4, 8), data="int1"),
    _c("epi_ps3_bias_addend_tail", "ps3", 2400, 8, 1028, "x3", 0, epi=("bias", "addend")),
    _c("epi_ps2_bias_addend_tail", "ps2", 2400, 8, 1028, "x2", 0, epi=("bias", "addend")),
]

# ---- the low parts: two levels (per-row scales), three levels (k <= 64, x3 and fp32), one case per tile and loader form
for _mode, _cfgs in (("x3", (0, 1, 2)), ("fp32", (0, 1, 2, 3))):
    for _cfg in _cfgs:
        for _entry in ("nt", "nn") + (("ps3",) if _mode == "x3" else ()):
            CASES.append(_c("l3_%s%d_%s" % (_mode, _cfg, _entry), _entry, 300, 132, 36, _mode, _cfg,
                            data="three_level" if _entry != "nn" else "three_level_w"))
        if _cfg != 2:
            CASES.append(_c("l3_%s%d_tn_big" % (_mode, _cfg), "tn_big", 60, 132, 68, _mode, _cfg, data="three_level"))
CASES += [
    _c("l3_x3s16_nt", "nt", 300, 132, 36, "x3", 1, 16, data="three_level"),
    _c("l3_x3s16_nt_w", "nt", 300, 132, 36, "x3", 0, 16, data="three_level_w"),
    _c("l3_x3s16_ps3", "ps3", 300, 132, 36, "x3", 2, 16, data="three_level"),
    _c("l3_x3_nt_w", "nt", 300, 132, 64, "x3", data="three_level_w"),
    _c("l3_x3_ps3_w", "ps3", 300, 132, 64, "x3", data="three_level_w"),
    _c("l3_x3_tail_atomic", "nt", 100, 8, 1028, "x3", 1, data="three_level"),
    _c("l2_x3_nt", "nt", 300, 132, 260, "x3", data="two_level"),
    _c("l2_x3_nt_w", "nt", 300, 132, 260, "x3", data="two_level_w"),
    _c("l2_x3_tail", "nt", 2400, 8, 1028, "x3", 0, data="two_level"),
    _c("l2_x3_tail_flat", "nt", 17000, 8, 1028, "x3", 1, data="two_level_w"),
    _c("l2_fp32_nt", "nt", 300, 132, 260, "fp32", data="two_level"),
    _c("l2_fp32_tail", "nt", 2400, 8, 1028, "fp32", 0, data="two_level_w"),
    _c("l2_ps2_x2", "ps2", 300, 132, 260, "x2", data="two_level"),
    _c("l2_ps2_x2_w", "ps2", 300, 132, 260, "x2", data="two_level_w"),
    _c("l2_ps2_x2_tail", "ps2", 2400, 8, 1028, "x2", data="two_level"),
    _c("l2_ps2_x2_tail_w", "ps2", 2400, 8, 1028, "x2", data="two_level_w"),
    _c("l2_ps2_x2_rounds_flat", "ps2", 9000, 1028, 1028, "x2", data="two_level"),
    _c("l2_ps2_x2_four_waves", "ps2", 300, 132, 260, "x2", 0, epi=("stats",), data="two_level"),
    _c("l2_ps2_row_panel", "ps2", 4099, 4100, 128, "x2", data="two_level"),
    _c("l2_ps2_row_panel_w", "ps2", 4099, 3908, 32, "x2", data="two_level_w"),
    _c("l2_ps3_x3", "ps3", 300, 132, 260, "x3", data="two_level_w"),
    _c("l2_nn_x3", "nn", 300, 132, 260, "x3", data="two_level"),
    _c("l2_tn_big_x3", "tn_big", 516, 132, 68, "x3", data="two_level"),
    # ---- both operands with low parts: the mirror of the arithmetic as reference
    _c("normal_x3_nt", "nt", 300, 132, 68, "x3", data="normal"),
    _c("normal_x3s16_nt", "nt", 300, 132, 68, "x3", 1, 16, data="normal"),
    _c("normal_x3_nn", "nn", 300, 132, 68, "x3", data="normal"),
    _c("normal_x3_ps3", "ps3", 300, 132, 68, "x3", data="normal"),
    _c("normal_x3_tail", "nt", 100, 8, 1028, "x3", 0, data="normal"),
    _c("normal_ps2_x2", "ps2", 300, 132, 68, "x2", data="normal"),
    _c("normal_ps2_x2_tail", "ps2", 100, 8, 1028, "x2", data="normal"),
    _c("normal_ps2_row_panel", "ps2", 4099, 3908, 32, "x2", data="normal"),
    _c("normal_fp32_nt", "nt", 300, 132, 68, "fp32", data="normal"),
    _c("normal_tn_big_x3", "tn_big", 516, 132, 68, "x3", data="normal"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "case names must be unique"


def _required():
    req = []
    tile_tags = ("one_partial_tile", "k_tail", "k4", "ragged_m", "ragged_n", "multigroup", "rounds_no_tail", "rounds_plus_tail",
                 "tail_only")
    for cfg in range(3):
        req += ["x3.%d:%s" % (cfg, t) for t in tile_tags + ("tail_aligned", "tail_flat", "tail_atomic", "tn_big_splitk")]
    for cfg in range(4):
        req += ["fp32.%d:%s" % (cfg, t) for t in tile_tags]
    req += ["x2.0:%s" % t for t in tile_tags + ("tail_aligned", "tail_flat", "tail_atomic", "tn_big_splitk")]
    req += ["x3.2:tn_big_general"]
    req += ["loader:" + t for t in ("nt", "nn", "tn_big_splitk", "tn_big_general", "presplit3", "presplit2_eight_waves",
                                    "presplit2_four_waves", "row_panel_k32", "row_panel_k64", "row_panel_k128", "two_part_unsplit_nt",
                                    "two_part_unsplit_nn", "two_part_unsplit_tn_big")]
    req += ["epi:" + t for t in ("bias", "addend", "addend_ldadd", "stats", "stats_row_panel", "rb1", "rb12", "act", "gate", "all",
                                 "strided_operands", "ldc_forbids_tail")]
    req += ["shape:32", "shape:16", "mode:fp32", "mode:x3", "mode:x2"]
    req += ["entry:" + e for e in ("nt", "nn", "ex", "ex_t", "ps3", "ps2", "tn_big", "tn")]
    req += ["data:" + d for d in ("int", "int1", "two_level", "two_level_w", "three_level", "three_level_w", "normal")]
    return tuple(req)


REQUIRED = _required()


def coverage(cus):
    """tag -> names of the cases that carry it on a device of `cus` CUs."""
    cov = collections.defaultdict(list)
    for c in CASES:
        for t in reached(c, cus):
            cov[t].append(c.name)
    return cov


# ---------------------------------------------------------------------------- the operands
def hash_name(s):
    h = 2166136261
    for ch in s.encode():
        h = ((h ^ ch) * 16777619) % (2 ** 32)
    return h


def _ints(rng, rows, cols, cap):
    """Integers with |v| <= min(cap, INT_CAPS[row % 8]) as float32."""
    caps = np.minimum(np.array(INT_CAPS, dtype=np.int8)[np.arange(rows) % 8], cap)[:, None]
    v = rng.integers(-7, 8, size=(rows, cols), dtype=np.int8)
    return np.clip(v, -caps, caps).astype(F32)


def _levels(rng, rows, cols, offsets):
    """2^s_row (p + sum_i q_i offsets[i]), p in {+-1, +-2}, q_i in {-1, 0, 1}, s_row in [-20, 20]: float32 (exact) and the scales."""
    p = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=(rows, cols))
    for off in offsets:
        p = p + rng.integers(-1, 2, size=(rows, cols)) * off
    s = rng.integers(-20, 21, size=rows)
    x = np.ldexp(p, s[:, None])
    x32 = x.astype(F32)
    assert np.array_equal(x32.astype(F64), x)
    return x32, s


def _one_part(rng, rows, cols, density=None, nonzeros=None):
    """2^t_row v with integers |v| <= 3, thinned to a density of non-zeros or to `nonzeros` per row."""
    v = rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=(rows, cols))
    if nonzeros is not None:
        keep = np.zeros((rows, cols), dtype=bool)
        np.put_along_axis(keep, rng.integers(0, cols, size=(rows, nonzeros)), True, axis=1)
        v = np.where(keep, v, 0.0)
    elif density is not None and density < 1.0:
        v = np.where(rng.random((rows, cols)) < density, v, 0.0)
    t = rng.integers(-20, 21, size=rows)
    return np.ldexp(v, t[:, None]).astype(F32), t


LEVELS = {"two_level": (2.0 ** -12,), "three_level": (2.0 ** -10, 2.0 ** -19)}
QUANTUM = {"two_level": 2.0 ** -12, "three_level": 2.0 ** -19}


def data_kind(c):
    return c.data[:-2] if c.data.endswith("_w") else c.data


def operand_key(c):
    """Cases with equal keys share their two operands (and the GPU module its fp64 product of them)."""
    return kernel_dims(c) + (c.data,)


@functools.lru_cache(maxsize=3)
def base_operands(M, N, K, data):
    """a (M x K), w (N x K) float32 as the kernel sees them, and the rows' binary scales (sa, sw; None where the kind has none)."""
    rng = np.random.default_rng(hash_name("%d_%d_%d_%s" % (M, N, K, data)) % (2 ** 31))
    swap = data.endswith("_w")
    kind = data[:-2] if swap else data
    if kind in ("int", "int1"):
        cap = 1 if kind == "int1" else 7
        return _ints(rng, M, K, cap), _ints(rng, N, K, cap), None, None
    if kind == "normal":
        a = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-6, 7, size=(M, 1)))).astype(F32)
        w = (rng.standard_normal((N, K)) * 0.3 * np.exp2(rng.integers(-6, 7, size=(N, 1)))).astype(F32)
        return a, w, None, None
    rl, rw = (N, M) if swap else (M, N)                               # rows of the levelled / of the one-part operand
    lv, s = _levels(rng, rl, K, LEVELS[kind])
    if kind == "two_level":
        op, t = _one_part(rng, rw, K, density=1.0 if K <= 512 else 0.5)
    else:
        op, t = _one_part(rng, rw, K, nonzeros=5)
    return (op, lv, t, s) if swap else (lv, op, s, t)


def operands(c):
    """The operands of case c AS THE KERNEL SEES THEM -- a (M x K), w (N x K) float32, both row-major over the reduction -- and the
    epilogue's: dict(a, w, sa, sw, bias, addend, row_bias, rpg, gate).  The GPU module lays them out as the entry point wants
    them (transposed for nn / tn_big, pitched by c.pads)."""
    M, N, K = kernel_dims(c)
    a, w, sa, sw = base_operands(M, N, K, c.data)
    o = dict(a=a, w=w, sa=sa, sw=sw, bias=None, addend=None, row_bias=None, rpg=1, gate=None)
    rng = np.random.default_rng(hash_name(c.name) % (2 ** 31))
    e = 1 if c.data == "int1" else 7
    if "bias" in c.epi:
        o["bias"] = rng.integers(-e, e + 1, size=N).astype(F32)
    if "addend" in c.epi:
        o["addend"] = rng.integers(-e, e + 1, size=(M, N)).astype(F32)
    for rb, rpg in (("rb1", 1), ("rb12", 12)):
        if rb in c.epi:
            o["row_bias"], o["rpg"] = rng.integers(-e, e + 1, size=(cdiv(M, rpg), N)).astype(F32), rpg
    if "gate" in c.epi:
        o["gate"] = rng.integers(-2, 3, size=(M, N)).astype(F32)      # (zeros included: the derivative at 0 is the slope)
    return o


def epilogue_bound(c):
    """What the epilogue can add to |A W^T| (integers)."""
    e = 1 if c.data == "int1" else 7
    return e * sum(1 for x in ("bias", "addend", "rb1", "rb12") if x in c.epi)


def exact_guard(c):
    """"int" data: an upper bound of max over the outputs of sum_k |a||w| (Hoelder: the largest row sum of |a| times the largest |w|,
    or the other way round, whichever is smaller) plus the epilogue's terms, which must stay below 2^24: every partial sum in any
    order is then an exactly representable integer."""
    o = operands(c)
    a, w = np.abs(o["a"]).astype(F64), np.abs(o["w"]).astype(F64)
    b = min(a.sum(1).max() * w.max(), w.sum(1).max() * a.max())
    return b + epilogue_bound(c)


def stat_guard(c, block_rows):
    """Cases with statistics partials: |x| <= X = exact_guard, so |x - pv| <= 2 X and a block's sum of squares <= rows (2 X)^2,
    which must stay below 2^24 (and with it the plain sums)."""
    x = exact_guard(c)
    return block_rows * (2.0 * x) ** 2


def level_guard(c):
    """two_level / three_level data: max over the outputs of sum_k |a / 2^s||w / 2^t| in units of the data's quantum (an upper bound:
    the levelled operand's largest magnitude times the one-part operand's largest row sum), which must stay below 2^24."""
    o = operands(c)
    kind = data_kind(c)
    a = np.abs(np.ldexp(o["a"].astype(F64), -o["sa"][:, None]))
    w = np.abs(np.ldexp(o["w"].astype(F64), -o["sw"][:, None]))
    lv, op = (w, a) if c.data.endswith("_w") else (a, w)
    return lv.max() * op.sum(1).max() / QUANTUM[kind]


def low_part_share(c):
    """three_level data: the share of the levelled operand's values whose bf16 split has a non-zero l."""
    o = operands(c)
    return float(np.mean(split_bf16x3(o["w"] if c.data.endswith("_w") else o["a"])[2] != 0))


def reference(c, mode=None, product=None):
    """The expected result of case c in fp64 (M x N as the kernel sees it), before the cast to float32, with the epilogue applied in
    the kernel's order: bias, addend, row_bias, LeakyReLU (ONE float32 multiply of the exact value), gate (a float32 multiply).
    Exact data: the fp64 product is exact (`product`: the same fp64 product computed elsewhere).  "normal": the mirror of the
    mode's arithmetic."""
    o = operands(c)
    if c.data == "normal":
        y = mirror_product(o["a"], o["w"], mode or c.mode)
    elif product is not None:
        y = product
    else:
        y = o["a"].astype(F64) @ o["w"].astype(F64).T
    if o["bias"] is not None:
        y = y + o["bias"].astype(F64)[None, :]
    if o["addend"] is not None:
        y = y + o["addend"].astype(F64)
    if o["row_bias"] is not None:
        y = y + o["row_bias"].astype(F64)[np.arange(y.shape[0]) // o["rpg"]]
    if "act" in c.epi:
        y32 = y.astype(F32)
        y = np.where(y32 > 0, y32, SLOPE * y32).astype(F64)
    if o["gate"] is not None:
        y32 = y.astype(F32)
        y = (y32 * np.where(o["gate"] > 0, F32(1.0), SLOPE)).astype(F64)
    return y


def stat_reference(y32, block_rows):
    """The statistics partials of a float32 result (M x N) in blocks of block_rows rows: (sum (x - pv), sum (x - pv)^2, pv) in fp64,
    pv the block's first row; only the blocks that hold rows."""
    M, N = y32.shape
    nb = cdiv(M, block_rows)
    out = np.zeros((nb, 3, N), dtype=F64)
    for b in range(nb):
        blk = y32[b * block_rows:(b + 1) * block_rows].astype(F64)
        d = blk - blk[:1]
        out[b, 0], out[b, 1], out[b, 2] = d.sum(0), (d * d).sum(0), blk[0]
    return out


def stat_block_rows(c, cus):
    """Rows of the result that one statistics partial covers: BM / 4 on the big fp32 tile, BM / 2 elsewhere, 256 on the row panel."""
    d = describe(c, cus)
    if d["kernel"] == "row_panel":
        return 256
    return d["tile"].BM // d["tile"].stat_div


# Edge values of the split mirrors and kernels: one row each (a row's maximum sets the two-part scale)
def edge_rows(cols=40):
    big = F32(1e38)
    rows = [
        np.zeros(cols),                                              # an all-zero row: e clamps to 126
        np.array([0.0, -0.0, 1.0, -1.0] * (cols // 4)),
        np.array([65504.0, -65504.0, 1.0, 2.0 ** -20 * 65504.0, 2.0 ** -30 * 65504.0, 0.0, 3.0, -5.0] * (cols // 8)),
        np.array([1.0, 2.0 ** -20, 2.0 ** -30, -2.0 ** -20, 1.0 + 2.0 ** -12, 0.75, -2.0 ** -24, 2.0 ** -16] * (cols // 8)),
        np.array([1e-45, -1e-45, 1e-40, 3e-39, 0.0, -1e-42, 5e-41, 1.1754942e-38] * (cols // 8)),     # subnormals only
        np.array([1e-40, 1.0, -1e-45, 2.0 ** -126, 2.0 ** -100, 0.0, -3.0, 1e-38] * (cols // 8)),      # subnormals under a normal maximum
        np.array([big, -big, big * F32(0.5), 1.0, 2.0 ** 100, -3e38, 1.7e38, 2.0 ** 126] * (cols // 8)),
        np.array([3.3e38, 1.0, -3.4e38, 2.0 ** 127, 0.0, 1e30, -1e38, 3.0e38] * (cols // 8)),           # bf16's h overflows here
    ]
    with np.errstate(over="ignore"):
        return np.stack(rows).astype(F32)
