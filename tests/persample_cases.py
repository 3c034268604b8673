"""The cases of tests/test_gpu_persample.py: the per-sample layer kernels (csrc/skinny.hip: nt / nt_act / nn / nn_masked / tn;
csrc/small_mlp.hip: forward / backward) in every launch regime, with their operands and references.  Shared by the host test
(tests/test_persample_host.py: guards and regime coverage, no GPU) and, through tests/persample_worker.py, by the GPU module.

Three kinds of data:
  "int"     small integers stored as float32 (|v| <= 7, zeros included, fixed seed): every product and every partial sum, in any
            order, is an integer below 2^24 (`exact_guard`), so the matrix-instruction chains, the split-K joins, the atomics and
            small_mlp's FMA chain must reproduce the int64 result bit for bit.  LeakyReLU's 0.01f is no dyadic number: where it
            applies the reference is ONE float32 multiply of the exact value.
  "normal"  random normal float32: bounded against float64 of the same float32 inputs.
  BatchNorm cases (bn_mode 1 / 2) have integer x, W, bias (an exact integer `pre`) whose per-channel batch variance is >= 1 (so invstd
            amplifies nothing; `variance_guard`), random gamma / beta / running buffers / dy, and a float64 restatement of the
            formulas in csrc/small_mlp.hip's comments as reference.  Two kinds of case are kept out because a gradient would be
            analytically zero and the bound (relative to the gradient's own scale) would measure rounding residue: bn_mode 1 at
            K == 1 (dW == 0: x is a multiple of xhat) and at R == 2 (dpre ~ 0: xhat = +-1); both shapes run in the other modes.

The launch arithmetic of both files is restated here (`nt_launch`, `nn_launch`, `tn_launch`, `sm_launch`); `reached` turns it into
the regime tags a case enters and REQUIRED lists the tags that at least one case must carry."""
import collections
import functools

import numpy as np

F32, F64 = np.float32, np.float64
EPS, MOMENTUM = 1e-5, 0.1
SLOPE = np.float32(0.01)
LIMIT = 2 ** 24
U = 2.0 ** -23                                                      # the product bound's unit: (K + 4) U sum|a||b|

NT = collections.namedtuple("NT", "name R N K pads bias act entry data")          # pads: lda - K, ldb - K, ldc - N
NN = collections.namedtuple("NN", "name R N K pads masked act data")              # pads: lda - pad4(K), ldp - K, ldb - N, ldc - N
TN = collections.namedtuple("TN", "name R N K pads data")                         # pads: lda - N, ldb - K, ldc - K
SM = collections.namedtuple("SM", "name R K N act bn bias affine running data")


def cdiv(a, b):
    return (a + b - 1) // b


def pad4(v):
    return cdiv(v, 4) * 4


# ---------------------------------------------------------------------------- the launch arithmetic, restated
def nt_launch(R, N, K):
    """pdgn_skinny_nt_act: SPLIT below N = 4096 (one workgroup per 16 columns, its four waves split the 16-deep chunks of K),
    else a wave per 16 columns, 64 per workgroup."""
    kchunks = cdiv(K, 16)
    split = N < 4096
    if split:
        per = cdiv(kchunks, 4)
        owned = tuple(max(0, min(kchunks, w * per + per) - w * per) for w in range(4))
        grid, idle_waves = cdiv(N, 16), 0
    else:
        per, owned = kchunks, (kchunks,) * 4
        grid = cdiv(N, 64)
        idle_waves = sum(1 for w in range(4) if ((grid - 1) * 4 + w) * 16 >= N)
    return dict(split=split, kchunks=kchunks, per=per, owned=owned, grid=grid, idle_waves=idle_waves, partial_columns=N % 16 != 0)


def nn_launch(R, N, K):
    """pdgn_skinny_nn / _nn_masked: 64 columns per workgroup, ~256 workgroups, at least 8 chunks per K slice."""
    kchunks, gx = cdiv(K, 16), cdiv(N, 64)
    slices = max(1, 256 // gx)
    slices = max(1, min(slices, kchunks // 8))
    per = cdiv(kchunks, slices)
    gy = cdiv(kchunks, per)
    return dict(kchunks=kchunks, gx=gx, slices=slices, per=per, gy=gy, last=kchunks - (gy - 1) * per, single=gy == 1,
                scalar_tail=K % 4 != 0)


def tn_launch(R, N, K):
    gx, kblocks = cdiv(N, 64), cdiv(K, 16)
    gy = 1 if 512 // gx < 1 else min(512 // gx, kblocks)
    return dict(gx=gx, gy=gy, kblocks=kblocks, strided=gy < kblocks)


def sm_ok(r, k, n, act, bn):
    return 1 <= r <= 64 and 1 <= k <= 1024 and n >= 1 and 0 <= act <= 2 and 0 <= bn <= 2 and r * (k + 4) * 4 + 1024 <= 160 * 1024


def sm_launch(R, K, N):
    vec = K % 4 == 0
    fwd, bwd = R * (K + 4) * 4, (R * (K + 4) + 256) * 4
    return dict(ok=sm_ok(R, K, N, 0, 0), vec=vec, grid=cdiv(N, 4), dead_waves=cdiv(N, 4) * 4 - N, lds_fwd=fwd, lds_bwd=bwd,
                attr_fwd=fwd > 64 * 1024, attr_bwd=bwd > 64 * 1024, dw_rounds=cdiv(K, 256) if vec else cdiv(K, 64))


# ---------------------------------------------------------------------------- the tables
NT_CASES = [
    NT("r1_n1_k4", 1, 1, 4, (4, 8, 3), False, 0, "nt", "int"),
    NT("r16_n15_k12_relu", 16, 15, 12, (4, 4, 1), True, 1, "act", "int"),
    NT("r17_n16_k20_leaky", 17, 16, 20, (8, 4, 2), False, 2, "act", "int"),
    NT("r35_n17_k68_leaky", 35, 17, 68, (4, 12, 5), True, 2, "act", "int"),
    NT("r64_n20_k256", 64, 20, 256, (4, 4, 4), True, 0, "nt", "int"),
    NT("r35_n20_k68_relu", 35, 20, 68, (4, 4, 1), False, 1, "act", "int"),
    NT("r64_n17_k4_act0", 64, 17, 4, (4, 4, 3), True, 0, "act", "int"),
    NT("r3_n4095_k4_leaky", 3, 4095, 4, (4, 4, 1), True, 2, "act", "int"),           # the last N of the SPLIT kernel
    NT("r35_n4096_k4_relu", 35, 4096, 4, (4, 4, 2), True, 1, "act", "int"),          # the first of the per-wave kernel
    NT("r35_n4100_k20_leaky", 35, 4100, 20, (4, 8, 3), False, 2, "act", "int"),      # its last workgroup: one wave with 4 columns, three idle
    NT("r17_n4096_k68", 17, 4096, 68, (4, 4, 1), True, 0, "nt", "int"),
    NT("normal_r35_n20_k68", 35, 20, 68, (4, 4, 1), False, 0, "nt", "normal"),
    NT("normal_r17_n4100_k20_leaky", 17, 4100, 20, (4, 4, 1), False, 2, "act", "normal"),
]
NN_CASES = [
    NN("r1_n4_k1", 1, 4, 1, (0, 0, 4, 1), False, 0, "int"),
    NN("r17_n60_k3", 17, 60, 3, (4, 0, 4, 3), False, 0, "int"),
    NN("r35_n64_k5", 35, 64, 5, (0, 0, 8, 2), False, 0, "int"),
    NN("r64_n68_k16", 64, 68, 16, (4, 0, 4, 1), False, 0, "int"),
    NN("r35_n4_k19", 35, 4, 19, (0, 0, 4, 5), False, 0, "int"),
    NN("r17_n68_k127", 17, 68, 127, (4, 0, 4, 1), False, 0, "int"),
    NN("r64_n60_k128", 64, 60, 128, (4, 0, 4, 4), False, 0, "int"),
    NN("r35_n64_k2050", 35, 64, 2050, (4, 0, 4, 1), False, 0, "int"),                # 129 chunks: 14 slices of 9 and one of 3
    NN("r17_n68_k4100", 17, 68, 4100, (4, 0, 4, 3), False, 0, "int"),                # gx = 2; 257 chunks: 28 slices of 9 and one of 5
    NN("r64_n4_k2050", 64, 4, 2050, (0, 0, 4, 1), False, 0, "int"),
    NN("normal_r35_n64_k2050", 35, 64, 2050, (4, 0, 4, 1), False, 0, "normal"),
    NN("masked_r35_n64_k16_relu", 35, 64, 16, (4, 3, 4, 1), True, 1, "int"),
    NN("masked_r17_n68_k128_relu", 17, 68, 128, (4, 1, 4, 2), True, 1, "int"),
    NN("masked_r64_n60_k4100_relu", 64, 60, 4100, (4, 5, 4, 1), True, 1, "int"),
    NN("masked_r35_n4_k19_relu", 35, 4, 19, (4, 2, 4, 3), True, 1, "int"),           # K % 4 != 0: only through the ABI
    NN("masked_r1_n64_k2050_relu", 1, 64, 2050, (0, 1, 4, 1), True, 1, "int"),
    NN("masked_r35_n64_k16_leaky", 35, 64, 16, (4, 3, 4, 1), True, 2, "normal"),
    NN("masked_r17_n68_k4100_leaky", 17, 68, 4100, (4, 1, 4, 2), True, 2, "normal"),
    NN("masked_r64_n4_k19_leaky", 64, 4, 19, (4, 2, 4, 3), True, 2, "normal"),
]
TN_CASES = [
    TN("r1_n1_k1", 1, 1, 1, (3, 2, 5), "int"),
    TN("r3_n15_k15", 3, 15, 15, (1, 1, 1), "int"),
    TN("r4_n16_k16", 4, 16, 16, (4, 0, 16), "int"),
    TN("r5_n17_k17", 5, 17, 17, (3, 3, 7), "int"),
    TN("r35_n65_k40", 35, 65, 40, (1, 2, 3), "int"),
    TN("r64_n17_k40", 64, 17, 40, (0, 0, 24), "int"),
    TN("r5_n6400_k120", 5, 6400, 120, (0, 4, 8), "int"),                            # gx = 100, gy = 5 < kblocks = 8: the strided loop
    TN("normal_r35_n65_k40", 35, 65, 40, (1, 2, 3), "normal"),
]
SM_CASES = [
    #   name                       R    K    N  act bn  bias  affine running
    SM("r1_k1_n1",                 1,   1,   1, 0, 0, False, False, False, "int"),
    SM("r2_k3_n3_relu",            2,   3,   3, 1, 0, True,  False, False, "int"),
    SM("r35_k4_n4_leaky",          35,  4,   4, 2, 0, True,  False, False, "int"),
    SM("r63_k5_n5_relu",           63,  5,   5, 1, 0, False, False, False, "int"),
    SM("r64_k20_n9_leaky",         64,  20,  9, 2, 0, True,  False, False, "int"),
    SM("r35_k21_n5",               35,  21,  5, 0, 0, True,  False, False, "int"),
    SM("r35_k260_n9_relu",         35,  260, 9, 1, 0, True,  False, False, "int"),     # second round of the dW lane loop
    SM("r35_k1024_n4_leaky",       35, 1024, 4, 2, 0, False, False, False, "int"),     # dynamic LDS above 64 KiB in both kernels
    SM("r64_k632_n3_relu",         64,  632, 3, 1, 0, True,  False, False, "int"),     # sm_ok's limit; the backward asks for 160 KiB
    SM("normal_r35_k20_n9_leaky",  35,  20,  9, 2, 0, True,  False, False, "normal"),
    SM("normal_r63_k21_n5_relu",   63,  21,  5, 1, 0, True,  False, False, "normal"),
    SM("bn1_r1_k4_n4_leaky",       1,   4,   4, 2, 1, True,  True,  True,  "bn"),      # R == 1: var 0, biased variance into running_var
    SM("bn1_r35_k20_n9_leaky",     35,  20,  9, 2, 1, True,  True,  True,  "bn"),
    SM("bn1_r63_k5_n5_relu",       63,  5,   5, 1, 1, False, True,  False, "bn"),      # no running buffers (track_running_stats=False)
    SM("bn1_r64_k21_n3",           64,  21,  3, 0, 1, True,  False, True,  "bn"),      # gamma / beta NULL, no activation, scalar form
    SM("bn1_r35_k260_n5_relu",     35,  260, 5, 1, 1, True,  True,  True,  "bn"),
    SM("bn1_r35_k1024_n3_leaky",   35, 1024, 3, 2, 1, True,  True,  True,  "bn"),
    SM("bn2_r2_k3_n4_leaky",       2,   3,   4, 2, 2, True,  True,  True,  "bn"),
    SM("bn2_r35_k4_n9",            35,  4,   9, 0, 2, False, False, True,  "bn"),
    SM("bn2_r64_k632_n5_relu",     64,  632, 5, 1, 2, True,  True,  True,  "bn"),
    SM("bn2_r1_k1_n1_relu",        1,   1,   1, 1, 2, True,  True,  True,  "bn"),
]
# (entry point, what is wrong, the return code): every one returns before any launch (csrc/skinny.hip, csrc/small_mlp.hip: the
# argument checks are the first statements of the entry points; -2 is the 16-byte pointer / pitch % 4 check behind them)
_SK3 = ("nt", "act", "nn", "nnm")
REFUSED = ([(e, k, -1) for e in _SK3 + ("tn", "smf", "smb") for k in ("R0", "R65")] +
           [(e, "lda_short", -1) for e in _SK3 + ("tn",)] +
           [(e, "null_operand", -1) for e in _SK3 + ("tn",)] +
           [(e, "misaligned", -2) for e in _SK3] + [(e, "pitch_mod4", -2) for e in _SK3] +
           [("nt", "K_mod4", -1), ("act", "K_mod4", -1), ("nn", "N_mod4", -1), ("nnm", "N_mod4", -1),
            ("act", "act3", -1), ("nnm", "act3", -1), ("nnm", "act0", -1), ("smf", "act3", -1), ("smb", "act3", -1),
            ("smf", "beyond_sm_ok", -1), ("smb", "beyond_sm_ok", -1), ("smf", "bn2_no_running", -1), ("smb", "bn_no_stat", -1)])


def by_name(table, name):
    (case,) = [c for c in table if c.name == name]
    return case


# ---------------------------------------------------------------------------- regimes
def reached(case):
    """The regime tags a case enters, from the restated launch arithmetic."""
    tags = set()
    if isinstance(case, NT):
        L = nt_launch(case.R, case.N, case.K)
        kind = "nt/split" if L["split"] else "nt/perwave"
        tags |= {"%s/R=%d" % (kind, case.R), "%s/N=%d" % (kind, case.N), "%s/K=%d" % (kind, case.K), "%s/act%d" % (kind, case.act),
                 "%s/%s" % (kind, "bias" if case.bias else "no_bias"), "nt/entry_" + case.entry, "nt/data_" + case.data}
        if L["split"]:
            tags.add("nt/split/empty_waves=%d" % sum(1 for o in L["owned"] if o == 0))
            tags.add("nt/split/per=%d" % L["per"])
        else:
            tags.add("nt/perwave/idle_waves=%d" % L["idle_waves"])
            tags.add("nt/perwave/kchunks=%d" % L["kchunks"])
        if all(p > 0 for p in case.pads):
            tags.add(kind + "/pitched")
    elif isinstance(case, NN):
        L = nn_launch(case.R, case.N, case.K)
        kind = "nnm" if case.masked else "nn"
        tags |= {"%s/R=%d" % (kind, case.R), "%s/N=%d" % (kind, case.N), "%s/K=%d" % (kind, case.K), "%s/data_%s" % (kind, case.data),
                 "%s/%s" % (kind, "single" if L["single"] else "atomics"), "%s/gx=%d" % (kind, L["gx"])}
        if not L["single"]:
            tags.add("%s/per=%d_last=%d" % (kind, L["per"], L["last"]))
        if L["scalar_tail"]:
            tags.add(kind + "/scalar_tail")
        if case.masked:
            tags.add("nnm/act%d" % case.act)
            if case.K + case.pads[1] != pad4(case.K) + case.pads[0]:
                tags.add("nnm/ldp!=lda")
    elif isinstance(case, TN):
        L = tn_launch(case.R, case.N, case.K)
        tags |= {"tn/R=%d" % case.R, "tn/N=%d" % case.N, "tn/K=%d" % case.K, "tn/data_" + case.data}
        if L["strided"]:
            tags.add("tn/strided_gx=%d_gy=%d_kblocks=%d" % (L["gx"], L["gy"], L["kblocks"]))
        if case.pads[2] > 0:
            tags.add("tn/column_slice")
    else:
        L = sm_launch(case.R, case.K, case.N)
        tags |= {"sm/R=%d" % case.R, "sm/K=%d" % case.K, "sm/N=%d" % case.N, "sm/act%d_bn%d" % (case.act, case.bn),
                 "sm/bias" if case.bias else "sm/no_bias", "sm/vec" if L["vec"] else "sm/scalar", "sm/data_" + case.data}
        if case.bn:
            tags.add("sm/bn%d_%s" % (case.bn, "affine" if case.affine else "no_affine"))
            tags.add("sm/bn%d_%s" % (case.bn, "running" if case.running else "no_running"))
        if L["attr_fwd"] and L["attr_bwd"]:
            tags.add("sm/lds_above_64k")
        if L["lds_bwd"] == 160 * 1024 and case.R * (case.K + 4) * 4 + 1024 == 160 * 1024:
            tags.add("sm/lds_limit")
        if L["dw_rounds"] == 2:
            tags.add("sm/dw_second_round")
        if L["dead_waves"] and case.bn:
            tags.add("sm/bn_dead_waves")
    return tags


REQUIRED = (
    ["nt/split/R=%d" % r for r in (1, 16, 17, 35, 64)] + ["nt/split/N=%d" % n for n in (1, 15, 16, 17, 20)] +
    ["nt/split/K=%d" % k for k in (4, 12, 20, 68, 256)] + ["nt/split/act%d" % a for a in (0, 1, 2)] +
    ["nt/split/bias", "nt/split/no_bias", "nt/split/pitched", "nt/split/empty_waves=3", "nt/split/empty_waves=2", "nt/split/empty_waves=1",
     "nt/split/empty_waves=0", "nt/split/per=2", "nt/split/N=4095", "nt/perwave/N=4096", "nt/perwave/N=4100", "nt/perwave/idle_waves=0",
     "nt/perwave/idle_waves=3", "nt/perwave/kchunks=5", "nt/perwave/R=17", "nt/perwave/R=35", "nt/perwave/pitched", "nt/entry_nt",
     "nt/entry_act", "nt/data_normal"] + ["nt/perwave/act%d" % a for a in (0, 1, 2)] +
    ["nn/N=%d" % n for n in (4, 60, 64, 68)] + ["nn/K=%d" % k for k in (1, 3, 5, 16, 19, 127, 128, 2050, 4100)] +
    ["nn/R=%d" % r for r in (1, 17, 35, 64)] +
    ["nn/single", "nn/atomics", "nn/scalar_tail", "nn/per=9_last=3", "nn/per=9_last=5", "nn/gx=2", "nn/data_normal"] +
    ["nnm/K=%d" % k for k in (16, 128, 4100, 19, 2050)] +
    ["nnm/act1", "nnm/act2", "nnm/ldp!=lda", "nnm/scalar_tail", "nnm/single", "nnm/atomics", "nnm/data_int", "nnm/data_normal"] +
    ["tn/R=%d" % r for r in (1, 3, 4, 5, 35, 64)] + ["tn/N=%d" % n for n in (1, 15, 16, 17, 65)] +
    ["tn/K=%d" % k for k in (1, 15, 16, 17, 40)] + ["tn/strided_gx=100_gy=5_kblocks=8", "tn/column_slice", "tn/data_normal"] +
    ["sm/R=%d" % r for r in (1, 2, 35, 63, 64)] + ["sm/K=%d" % k for k in (1, 3, 4, 5, 20, 21, 260, 1024, 632)] +
    ["sm/N=%d" % n for n in (1, 3, 4, 5, 9)] + ["sm/act%d_bn%d" % (a, b) for a in (0, 1, 2) for b in (0, 1, 2)] +
    ["sm/bias", "sm/no_bias", "sm/vec", "sm/scalar", "sm/data_normal", "sm/bn1_affine", "sm/bn1_no_affine", "sm/bn2_affine",
     "sm/bn2_no_affine", "sm/bn1_running", "sm/bn1_no_running", "sm/lds_above_64k", "sm/lds_limit", "sm/dw_second_round",
     "sm/bn_dead_waves"])


def all_cases():
    return NT_CASES + NN_CASES + TN_CASES + SM_CASES


# ---------------------------------------------------------------------------- operands
def _seed(case):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(type(case).__name__ + case.name)) % (2 ** 31)


def _ints(rng, shape):
    return rng.integers(-7, 8, size=shape).astype(F32)


def _draw(rng, shape, data):
    return _ints(rng, shape) if data == "int" else rng.standard_normal(shape).astype(F32)


def pitched(a, ld):
    """`a` (rows, cols) in rows of `ld` floats; the gap holds NaN: an operand element a kernel must not read."""
    out = np.full((a.shape[0], ld), np.nan, F32)
    out[:, :a.shape[1]] = a
    return out


def act_f32(z, act):
    """The kernels' activation in float32: LeakyReLU is ONE float32 multiply by 0.01f."""
    z = np.asarray(z, F32)
    if act == 2:
        return np.where(z > 0, z, SLOPE * z).astype(F32)
    return np.where(z > 0, z, F32(0)).astype(F32) if act == 1 else z


def act_f64(z, act):
    return np.where(z > 0, z, (F64(SLOPE) if act == 2 else 0.0) * z) if act else z


def actg(z, act, dtype):
    """act'(z): 1 where z > 0, else 0.01f (LeakyReLU) / 0 (ReLU)."""
    if act == 0:
        return np.ones(np.shape(z), dtype)
    return np.where(np.asarray(z) > 0, dtype(1), dtype(SLOPE) if act == 2 else dtype(0)).astype(dtype)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def nt_operands(case):
    """A (R, K), B (N, K), bias (N) | None; `mag` = sum |a||b| (+ |bias|); exact: `want` float32, else `ref` float64."""
    rng = np.random.default_rng(_seed(case))
    A, B = _draw(rng, (case.R, case.K), case.data), _draw(rng, (case.N, case.K), case.data)
    bias = _draw(rng, (case.N,), case.data) if case.bias else None
    z = A.astype(F64) @ B.astype(F64).T + (bias.astype(F64) if case.bias else 0.0)
    mag = np.abs(A).astype(F64) @ np.abs(B).astype(F64).T + (np.abs(bias).astype(F64) if case.bias else 0.0)
    d = dict(A=A, B=B, bias=bias, mag=mag)
    if case.data == "int":
        d["want"] = act_f32(z.astype(F32), case.act)
    else:
        d["ref"] = act_f64(z, case.act)
    return _freeze(d)


P_PLANTS = np.array([0.0, -0.0, 1e-45, -1e-45, 3.0, -2.0, 0.5, -7.0], F32)       # both zeros, the smallest subnormal of each sign


@functools.lru_cache(maxsize=None)
def nn_operands(case):
    """A (R, K), B (K, N), P (R, K) | None; the mask is applied as the kernel does: a[r][k] *= neg where !(P > 0)."""
    rng = np.random.default_rng(_seed(case))
    A, B = _draw(rng, (case.R, case.K), case.data), _draw(rng, (case.K, case.N), case.data)
    d = dict(A=A, B=B, P=None)
    if case.masked:
        P = P_PLANTS[rng.integers(0, len(P_PLANTS), size=(case.R, case.K))]
        n = min(len(P_PLANTS), P.size)
        P.reshape(-1)[:n] = P_PLANTS[:n]                            # (every plant at least once)
        d["P"] = P
        m64 = actg(P, case.act, F64)
    else:
        m64 = np.ones(A.shape, F64)
    Am = A.astype(F64) * m64
    d["mag"] = np.abs(Am) @ np.abs(B).astype(F64)
    ref = Am @ B.astype(F64)
    if case.data == "int":
        d["want"] = ref.astype(F32)
    else:
        d["ref"] = ref
    return _freeze(d)


@functools.lru_cache(maxsize=None)
def tn_operands(case):
    """A (R, N), B (R, K) -> C (N, K) = A^T B."""
    rng = np.random.default_rng(_seed(case))
    A, B = _draw(rng, (case.R, case.N), case.data), _draw(rng, (case.R, case.K), case.data)
    ref = A.astype(F64).T @ B.astype(F64)
    d = dict(A=A, B=B, mag=np.abs(A).astype(F64).T @ np.abs(B).astype(F64))
    d["want" if case.data == "int" else "ref"] = ref.astype(F32) if case.data == "int" else ref
    return _freeze(d)


def sm_reference64(case, x, W, bias, gamma, beta, rm, rv, dy):
    """float64 restatement of csrc/small_mlp.hip (forward and adjoint) on float32 inputs."""
    R = case.R
    x64, W64 = x.astype(F64), W.astype(F64)
    pre = x64 @ W64.T + (bias.astype(F64) if bias is not None else 0.0)
    ga = gamma.astype(F64) if gamma is not None else np.ones(case.N)
    be = beta.astype(F64) if beta is not None else np.zeros(case.N)
    out = dict(pre=pre)
    if case.bn == 1:
        mean = pre.sum(0) / R
        var = ((pre - mean) ** 2).sum(0) / R
        invstd = 1.0 / np.sqrt(var + F64(F32(EPS)))
        out["var"] = var
        if rm is not None:
            mom = F64(F32(MOMENTUM))
            out["rm"] = (1 - mom) * rm.astype(F64) + mom * mean
            out["rv"] = (1 - mom) * rv.astype(F64) + mom * (var * R / (R - 1) if R > 1 else var)
    elif case.bn == 2:
        mean, invstd = rm.astype(F64), 1.0 / np.sqrt(rv.astype(F64) + F64(F32(EPS)))
        out["var"] = rv.astype(F64)
    if case.bn:
        xhat = (pre - mean) * invstd
        z = xhat * ga + be
        out["stat"] = np.concatenate([mean, invstd])
    else:
        z = pre
    out["z"], out["y"] = z, act_f64(z, case.act)
    dz = dy.astype(F64) * actg(z, case.act, F64)
    if case.bn:
        s1, s2 = dz.sum(0), (dz * xhat).sum(0)
        out["dbeta"], out["dgamma"] = s1, s2
        dp = ga * invstd * (dz - s1 / R - xhat * (s2 / R)) if case.bn == 1 else ga * invstd * dz
    else:
        dp = dz
    out["dpre"], out["dbias"], out["dW"] = dp, dp.sum(0), dp.T @ x64
    return out


@functools.lru_cache(maxsize=None)
def sm_operands(case):
    """x (R, K), W (N, K), bias, gamma, beta, rm, rv (None where the case has none), dy (R, N) and the references.
    "int": `want_*` float32, bit for bit (dy integer; LeakyReLU's dpre is the one rounding dy * 0.01f, so its dW / dbias are bounded).
    "normal": `ref` float64 with `mag_*`.  "bn": `ref` float64; integer x, W, bias redrawn (fixed sequence of seeds) until every
    channel's batch variance is >= 1 and no |z| is below 1e-3 (the activation's branch is the same in float32 and float64)."""
    for attempt in range(200):
        rng = np.random.default_rng(_seed(case) + 7919 * attempt)
        kind = "normal" if case.data == "normal" else "int"
        x, W = _draw(rng, (case.R, case.K), kind), _draw(rng, (case.N, case.K), kind)
        bias = _draw(rng, (case.N,), kind) if case.bias else None
        gamma = beta = rm = rv = None
        if case.bn and case.affine:
            gamma = (rng.uniform(0.5, 1.5, case.N) * rng.choice([-1.0, 1.0], case.N)).astype(F32)
            beta = rng.uniform(-0.5, 0.5, case.N).astype(F32)
        if case.bn and case.running:
            rm, rv = rng.uniform(-0.3, 0.3, case.N).astype(F32), rng.uniform(1.0, 2.0, case.N).astype(F32)
        dy = _ints(rng, (case.R, case.N)) if case.data == "int" else rng.standard_normal((case.R, case.N)).astype(F32)
        ref = sm_reference64(case, x, W, bias, gamma, beta, rm, rv, dy)
        if case.data != "bn":
            break
        if (case.R == 1 or (ref["var"] >= 1.0).all()) and (case.act == 0 or np.abs(ref["z"]).min() > 1e-3):
            break
    else:
        raise AssertionError("no draw of %s passes the variance guard" % case.name)
    d = dict(x=x, W=W, bias=bias, gamma=gamma, beta=beta, rm=rm, rv=rv, dy=dy, ref=ref, attempt=attempt)
    d["mag_pre"] = np.abs(x).astype(F64) @ np.abs(W).astype(F64).T + (np.abs(bias).astype(F64) if case.bias else 0.0)
    if case.data == "int":
        pre = ref["pre"].astype(F32)
        d["want_pre"], d["want_y"] = pre, act_f32(pre, case.act)
        d["want_dpre"] = (dy * actg(d["want_y"], case.act, F32)).astype(F32)           # pre handed as y: the same sign
        d["exact_sums"] = case.act != 2
        dp64 = d["want_dpre"].astype(F64)
        d["want_dbias"], d["want_dW"] = dp64.sum(0).astype(F32), (dp64.T @ x.astype(F64)).astype(F32)
        d["ref_dbias"], d["ref_dW"] = dp64.sum(0), dp64.T @ x.astype(F64)
        d["mag_dbias"], d["mag_dW"] = np.abs(dp64).sum(0), np.abs(dp64).T @ np.abs(x).astype(F64)
    elif case.data == "normal":
        dp64 = ref["dpre"]
        d["mag_dbias"], d["mag_dW"] = np.abs(dp64).sum(0), np.abs(dp64).T @ np.abs(x).astype(F64)
    return _freeze(d)


# ---------------------------------------------------------------------------- guards
def exact_guard(case):
    """max sum |a||b| of every sum an "int" case makes, in int64; must stay below 2^24."""
    i64 = lambda a: np.abs(a).astype(np.int64)                     # noqa: E731
    if isinstance(case, NT):
        o = nt_operands(case)
        return int((i64(o["A"]) @ i64(o["B"]).T + (i64(o["bias"]) if case.bias else 0)).max())
    if isinstance(case, NN):
        o = nn_operands(case)
        return int((i64(o["A"]) @ i64(o["B"])).max())
    if isinstance(case, TN):
        o = tn_operands(case)
        return int((i64(o["A"]).T @ i64(o["B"])).max())
    o = sm_operands(case)
    fwd = int((i64(o["x"]) @ i64(o["W"]).T + (i64(o["bias"]) if case.bias else 0)).max())
    if case.data == "bn" or case.act == 2:                          # (LeakyReLU's dpre is no integer: those sums are bounded, not exact)
        return fwd
    dp = i64(o["want_dpre"])
    return max(fwd, int(dp.sum(0).max()), int((dp.T @ i64(o["x"])).max()))


def variance_guard(case):
    """The smallest variance invstd is made of (batch variance, or the running variance in bn_mode 2); R == 1 in bn_mode 1 has
    variance 0 by construction and pre - mean == 0 exactly, so there is nothing to amplify: reported as None."""
    o = sm_operands(case)
    if case.bn == 1 and case.R == 1:
        assert (o["ref"]["var"] == 0).all()
        return None
    return float(o["ref"]["var"].min())
