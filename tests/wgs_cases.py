"""The exact cases of tests/test_gpu_wgs.py, built once: inputs from hashweights (dyadic lattices, no RNG), expected results from
tests/wgs_mirror.py, every one passed through the mirror's `assert_exact` before it is handed out.  Shared by the host test
(tests/test_wgs_mirror_host.py), the GPU module and its child processes (tests/wgs_worker.py).

Every case names the kernel it is meant to reach; `check_table` asserts that through wgs_mirror.regime.  The shapes are the smallest
that reach a regime: the forward / statistics threshold n*P*(C/4) >= 65536 is met by n = 1024, P = 4, C = 64 and missed by n = 1023;
the adjoint's n*T*(C/4) >= 65536 by n = 171, T = 6, C = 256 and missed by n = 170.

Every graph (kind "planted") holds: a hub (point 3) in slot 0 of every query; query 1 naming the hub in all k slots; point n - 2 with
in-degree 0; the extreme indices 0 and n - 1 (in the last slot of the queries n - 1 and 0).  Where a shape cannot hold them all
(n < 6, or k = 1, where the queries 0 and n - 1 name n - 1 and 0 instead of the hub) it holds those it can."""
import collections
import functools

import numpy as np

import wgs_mirror as wm
from hashweights import lattice_points, unit_hash
from localpair_cases import quarter_steps

Fwd = collections.namedtuple("Fwd", "name b n k ldy spec bias want bits", defaults=(2,))
Adj = collections.namedtuple("Adj", "name b n k ldy specs wants")
Graph = collections.namedtuple("Graph", "b n k kind")
E2E = collections.namedtuple("E2E", "name b n k ldy specs biases pitch tiled")

HUB = 3
S6, S3 = (6, 4, 64, 64, 0), (3, 4, 64, 64, 0)          # centre block first, taps behind it: a non-zero tap offset

# bias: None, "shared", or the per-sample pitch in floats
FORWARD = [
    # -- fwd_scalar, one cause each
    Fwd("scalar_C", 2, 37, 5, 28, (3, 3, 6, 0, 20), "shared", "fwd_scalar"),             # C % 4
    Fwd("scalar_ldy", 2, 37, 5, 34, (3, 3, 8, 0, 24), "shared", "fwd_scalar"),           # ldy % 4
    Fwd("scalar_off", 2, 37, 5, 36, (3, 3, 8, 2, 28), None, "fwd_scalar"),               # off % 4
    Fwd("scalar_offc", 2, 37, 5, 36, (3, 3, 8, 0, 26), "shared", "fwd_scalar"),          # offc % 4
    Fwd("scalar_pitch", 2, 37, 5, 32, (3, 3, 8, 0, 24), 10, "fwd_scalar"),               # bias pitch % 4
    # -- fwd_flat4
    Fwd("flat4_small", 3, 50, 10, 56, (6, 5, 8, 0, 48), 12, "fwd_flat4", 4),             # far below the threshold
    Fwd("flat4_under_T6", 2, 1023, 9, 448, S6, "shared", "fwd_flat4"),                   # 65472 units
    Fwd("flat4_under_T3", 1, 1023, 6, 256, S3, None, "fwd_flat4", 3),
    Fwd("flat4_T9", 1, 1024, 12, 640, (9, 4, 64, 0, 576), "shared", "fwd_flat4"),        # over the threshold, T > 8
    Fwd("flat4_T10", 1, 1024, 13, 704, (10, 4, 64, 0, 640), None, "fwd_flat4"),
    # -- fwd_xcd6: exactly 65536 units; C / 4 = 16 is below one chunk; b * nchunk = 2
    Fwd("xcd6_at", 2, 1024, 9, 448, S6, "shared", "fwd_xcd6"),
    Fwd("xcd6_P3_ragged2", 2, 1366, 8, 448, (6, 3, 64, 0, 384), None, "fwd_xcd6", 3),    # n*P = 4098 = 32*128 + 2: row lanes past the end at every width
    Fwd("xcd6_P1_two_chunks", 1, 1024, 6, 1792, (6, 1, 256, 0, 1536), "shared", "fwd_xcd6"),   # P = 1: no reciprocal; two full chunks
    Fwd("xcd6_three_chunks", 3, 304, 8, 2016, (6, 3, 288, 0, 1728), "shared", "fwd_xcd6"),     # C / 4 = 72 = 32 + 32 + 8; 9 tasks
    # -- fwd_xcd_rt
    Fwd("xcd_rt_T3", 1, 1024, 6, 256, S3, None, "fwd_xcd_rt", 3),
    Fwd("xcd_rt_T1", 2, 1024, 4, 128, (1, 4, 64, 0, 64), 80, "fwd_xcd_rt"),              # per-sample bias, pitch 80 > C
    Fwd("xcd_rt_T8", 1, 1024, 11, 576, (8, 4, 64, 0, 512), "shared", "fwd_xcd_rt"),
    Fwd("xcd_rt_T0", 3, 1024, 4, 64, (0, 4, 64, 0, 0), "shared", "fwd_xcd_rt", 4),       # bias + centre alone
    Fwd("xcd_rt_nocentre", 2, 1024, 6, 192, (3, 4, 64, 0, -1), None, "fwd_xcd_rt"),
    Fwd("xcd_rt_P7_ragged13", 1, 587, 10, 320, (4, 7, 64, 0, 256), "shared", "fwd_xcd_rt"),    # n*P = 4109 = 128*32 + 13
    Fwd("xcd_rt_one_chunk", 3, 512, 5, 384, (2, 4, 128, 0, 256), 132, "fwd_xcd_rt"),     # C / 4 = 32: exactly one chunk; pitch 132
    # (for the narrower chunk widths of the child processes: C / 4 = 20 = 8 + 8 + 4 = 16 + 4, and C / 4 = 8)
    Fwd("xcd_rt_cv20", 1, 820, 5, 240, (2, 4, 80, 0, 160), "shared", "fwd_xcd_rt"),
    Fwd("xcd_rt_cv8", 1, 2048, 5, 96, (2, 4, 32, 0, 64), None, "fwd_xcd_rt"),
]

STATS = [
    Fwd("geom6_small", 3, 64, 10, 448, (6, 5, 64, 0, 384), "shared", "stats_geom6"),
    Fwd("geom6_under", 2, 1023, 9, 448, S6, "shared", "stats_geom6"),
    Fwd("geom_rt_T3", 2, 50, 4, 32, (3, 2, 8, 0, 24), 12, "stats_geom_rt", 4),
    Fwd("geom_rt_T8", 2, 100, 11, 72, (8, 4, 8, 0, 64), None, "stats_geom_rt"),
    Fwd("geom_rt_T0", 2, 100, 4, 8, (0, 4, 8, 0, 0), "shared", "stats_geom_rt"),
    Fwd("geom_rt_under_T1", 1, 1023, 4, 128, (1, 4, 64, 0, 64), None, "stats_geom_rt"),
    # 65536 units, yet the BatchNorm geometry has gy = 62 row blocks for b = 65 samples: the task mapping needs one per sample
    Fwd("geom_rt_gy_below_b", 65, 8, 2, 16384, (1, 2, 16384, 0, -1), None, "stats_geom_rt"),
    Fwd("xcd6_at", 2, 1024, 9, 448, S6, "shared", "stats_xcd6"),
    Fwd("xcd6_spare", 2, 1367, 8, 448, (6, 3, 64, 0, 384), "shared", "stats_xcd6", 3),   # gy = 33, b * bpt = 26: 7 spare partial rows
    Fwd("xcd6_chunks", 3, 304, 8, 2016, (6, 3, 288, 0, 1728), "shared", "stats_xcd6"),   # C / 4 = 72 = 4 * 16 + 8; 41 spare rows
    Fwd("xcd_rt_T1", 1, 1024, 4, 128, (1, 4, 64, 0, 64), None, "stats_xcd_rt"),
    Fwd("xcd_rt_T3", 2, 1024, 6, 256, S3, 80, "stats_xcd_rt", 3),
    Fwd("xcd_rt_T8", 1, 1024, 11, 576, (8, 4, 64, 0, 512), "shared", "stats_xcd_rt"),
    Fwd("xcd_rt_T0", 3, 1024, 4, 64, (0, 4, 64, 0, 0), "shared", "stats_xcd_rt"),
    Fwd("xcd_rt_nocentre_P7", 1, 587, 10, 256, (4, 7, 64, 0, -1), None, "stats_xcd_rt"),
    Fwd("xcd_rt_cv20", 1, 820, 5, 240, (2, 4, 80, 0, 160), "shared", "stats_xcd_rt"),    # C / 4 = 20 = 16 + 4 (and 8 + 8 + 4 in a child)
]
# what pdgn_window_gather_sum_stats documents as refused
STATS_REFUSED = [
    Fwd("T9", 2, 40, 12, 80, (9, 4, 8, 0, 72), None, "invalid"),
    Fwd("C", 2, 40, 5, 28, (3, 3, 6, 0, 20), None, "invalid"),
    Fwd("ldy", 2, 40, 5, 34, (3, 3, 8, 0, 24), None, "invalid"),
    Fwd("off", 2, 40, 5, 36, (3, 3, 8, 2, 28), None, "invalid"),
    Fwd("offc", 2, 40, 5, 36, (3, 3, 8, 0, 26), None, "invalid"),
    Fwd("pitch", 2, 40, 5, 32, (3, 3, 8, 0, 24), 10, "invalid"),
    Fwd("b0", 0, 40, 5, 32, (3, 3, 8, 0, 24), None, "invalid"),
    Fwd("window", 2, 40, 5, 32, (3, 4, 8, 0, 24), None, "invalid"),                      # T + P - 1 > k
]

TRANSPOSE = [Graph(1, 1, 1, "planted"), Graph(3, 1, 31, "planted"), Graph(1, 1000, 10, "planted"), Graph(3, 1000, 1, "planted"),
             Graph(3, 1025, 31, "planted"), Graph(1, 1025, 10, "allone"), Graph(3, 1000, 31, "allone")]
TRANSPOSE_REFUSED = [Graph(1, 40, 32, "planted"), Graph(1, 40, 0, "planted"), Graph(1, 0, 4, "planted")]

A6 = (6, 5, 256, 0, 1536)
ADJOINT = [                                               # through the CSR entry point AND the atomic one
    Adj("small_under_T6", 2, 170, 10, 1792, (A6,), ("csr_small",)),                       # 65280 units; C / 4 = 64
    Adj("xcd6_at", 2, 171, 10, 1792, (A6,), ("csr_xcd6",)),                               # 65664; n = 4 * 42 + 3
    Adj("small_T9", 1, 120, 10, 2560, ((9, 2, 256, 0, 2304),), ("csr_small",)),           # 69120 units, T = 9
    Adj("small_under_T10", 2, 163, 10, 1760, ((10, 1, 160, 0, 1600),), ("csr_small",)),   # 65200; C / 4 = 40
    Adj("xcd10_at", 2, 164, 10, 1760, ((10, 1, 160, 0, 1600),), ("csr_xcd10",)),          # 65600
    Adj("xcd10_cv44", 1, 149, 10, 1936, ((10, 1, 176, 0, 1760),), ("csr_xcd10",)),        # C / 4 = 44: a partial chunk at every width
    Adj("xcd_rt_T1", 1, 820, 10, 640, ((1, 10, 320, 0, 320),), ("csr_xcd_rt",)),          # C / 4 = 80: a chunk and a quarter
    Adj("small_under_T4", 1, 255, 6, 1280, ((4, 3, 256, 0, 1024),), ("csr_small",)),
    Adj("xcd_rt_T4", 3, 256, 6, 1280, ((4, 3, 256, 0, 1024),), ("csr_xcd_rt",)),          # exactly 65536
    Adj("xcd_rt_T8_nocentre", 2, 205, 10, 1280, ((8, 3, 160, 0, -1),), ("csr_xcd_rt",)),
    Adj("small_nocentre", 2, 50, 4, 24, ((3, 2, 4, 4, -1),), ("csr_small",)),             # columns 0..3 and 16..23 belong to nobody
    Adj("small_T0", 2, 61, 3, 16, ((0, 3, 16, 0, 0),), ("csr_small",)),                   # the centre block alone
    Adj("tile3", 2, 256, 10, 1488, ((4, 3, 256, 0, 1024), (10, 1, 16, 1280, 1440), (0, 7, 32, 0, 1456)),
        ("csr_xcd_rt", "csr_small", "csr_small")),
    Adj("tile2", 1, 171, 10, 3392, (A6, (10, 1, 160, 1792, -1)), ("csr_xcd6", "csr_xcd10")),
]
ATOMIC_ONLY = [
    Adj("unaligned", 2, 37, 5, 28, ((3, 3, 6, 0, 20),), ("bwd_atomic",)),
    Adj("gap", 2, 150, 6, 60, ((3, 4, 8, 0, 24), (2, 2, 6, 34, -1)), ("bwd_atomic", "bwd_atomic")),      # 32..33 and 46..59 untouched
]

# EdgeGatherSum end to end.  specs may carry the sixth field (want_stats); biases: None, "shared" or "sample" (column slices of ONE
# packed (b, pitch) tensor, in spec order)
END_TO_END = [
    E2E("tiled", 2, 300, 10, 208, ((6, 5, 16, 0, 96, True), (10, 1, 8, 112, 192), (1, 10, 4, 200, 204)), ("shared", "shared", None), 0, True),
    E2E("gap", 2, 150, 6, 60, ((3, 4, 8, 0, 24), (2, 2, 6, 34, -1)), ("shared", None), 0, False),
    E2E("sample_bias", 3, 200, 10, 288, ((6, 5, 16, 0, 96), (10, 1, 16, 112, 272)), ("sample", "sample"), 40, True),
]

# the reduced lists of the child processes (tests/wgs_worker.py): both sides of every threshold and the chunk edges
WORKER_FORWARD = ["flat4_under_T6", "xcd6_at", "flat4_under_T3", "xcd_rt_T3", "xcd6_P3_ragged2", "xcd_rt_P7_ragged13",
                  "xcd6_P1_two_chunks", "xcd6_three_chunks", "xcd_rt_one_chunk", "xcd_rt_T1", "xcd_rt_cv20", "xcd_rt_cv8"]
WORKER_STATS = ["geom6_under", "xcd6_at", "xcd6_spare", "xcd6_chunks", "xcd_rt_T3", "xcd_rt_nocentre_P7", "xcd_rt_cv20"]
WORKER_ADJOINT = ["small_under_T6", "xcd6_at", "xcd10_at", "xcd10_cv44", "xcd_rt_T1", "xcd_rt_T8_nocentre", "tile3"]
# one child per line: the three chunk widths belong to three different entry points and share a child
WORKER_SETTINGS = [{"PDGN_WGS_XCD": "0"},
                   {"PDGN_WGS_CW": "8", "PDGN_WGS_SCW": "8", "PDGN_WGS_BCW": "8"},
                   {"PDGN_WGS_CW": "16", "PDGN_WGS_SCW": "32", "PDGN_WGS_BCW": "16"},
                   {"PDGN_WGS_CW": "64", "PDGN_WGS_SCW": "64", "PDGN_WGS_BCW": "32"}]


def by_name(table, name):
    (case,) = [c for c in table if c.name == name]
    return case


def switches(setting):
    """A child's environment -> (xcd, {entry: cw}) as wgs_mirror.regime / geometry take them."""
    xcd = int(setting.get("PDGN_WGS_XCD", "1"))
    cw = {e: int(setting[v]) if v in setting else None for e, v in (("fwd", "PDGN_WGS_CW"), ("stats", "PDGN_WGS_SCW"), ("csr", "PDGN_WGS_BCW"))}
    return xcd, cw


# ---------------------------------------------------------------------------- inputs
def graph(b, n, k, kind="planted", key="wgs"):
    """idx (b, n, k) int32 from unit_hash, with the plants of the module docstring."""
    hub = HUB % n
    if kind == "allone":
        return np.full((b, n, k), hub, np.int32)
    assert kind == "planted", kind
    u = (unit_hash("%s/idx/%d/%d/%d" % (key, b, n, k), b * n * k).astype(np.float64) + 1.0) / 2.0
    idx = np.minimum(np.floor(u * n), n - 1).astype(np.int32).reshape(b, n, k)
    idx[:, :, 0] = hub                               # the hub: in-degree >= n
    if n >= 2:
        idx[:, 1, :] = hub                           # one query, k times the same point
    idx[:, 0, k - 1] = n - 1                         # the extreme indices
    idx[:, n - 1, k - 1] = 0
    if n >= 6:
        idx[idx == n - 2] = n - 3                    # a point nobody names
    return idx


def planted(idx):
    """Which of the plants a graph holds: (hub in slot 0 of every query, a one-point query, an in-degree-0 point, both extremes)."""
    b, n, k = idx.shape
    hub = HUB % n
    deg = np.stack([np.bincount(s.reshape(-1), minlength=n) for s in idx])
    return (bool((idx[:, :, 0] == hub).all()), bool(n >= 2 and (idx[:, 1, :] == hub).all()), bool((deg == 0).any(axis=1).all()),
            bool((deg[:, 0] > 0).all() and (deg[:, n - 1] > 0).all()))


def dyadic_dout(key, shape):
    return quarter_steps(key, shape) + np.float32(0.0)                  # (+ 0: no negative zeros, so bit patterns can be compared)


def _bias_of(case, key):
    """-> (flat float32 array | None, bias_bstride)."""
    C = case.spec[2]
    if case.bias is None:
        return None, 0
    if case.bias == "shared":
        return lattice_points(key + "/bias", (C,), case.bits), 0
    return lattice_points(key + "/bias", (case.b * case.bias,), case.bits), case.bias


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def forward_reference(case):
    """Inputs and the guarded mirror results of one FORWARD / STATS case: Y, idx, bias (flat | None), bstride, out (float64), and the
    exact column totals `total`, `total_sq` of out."""
    key = "wgs/fwd/" + case.name
    q = 2.0 ** -case.bits
    Y = lattice_points(key + "/Y", (case.b, case.n, case.ldy), case.bits)
    idx = graph(case.b, case.n, case.k, key=key)
    bias, bstride = _bias_of(case, key)
    wm.assert_exact(Y, q)
    out = wm.gather_sum(Y, idx, case.spec, bias, bstride)
    wm.assert_exact(out, q, wm.gather_sum(Y, idx, case.spec, bias, bstride, absolute=True))
    total, total_sq = wm.partial_totals(out)
    # the statistics kernels add |out| <= sum |terms| and out^2 into float32 partial sums: bounded by the whole column's
    wm.assert_exact(total, q, np.abs(out).reshape(-1, out.shape[-1]).sum(0))
    wm.assert_exact(total_sq, q * q, total_sq)
    return _freeze(dict(Y=Y, idx=idx, bias=bias, bstride=bstride, out=out, total=total, total_sq=total_sq))


@functools.lru_cache(maxsize=None)
def adjoint_reference(case):
    """idx, one dout per spec, the guarded dY (float64; zero where no spec writes), the covered columns, the transposed graph and the
    row maxima over the covered columns."""
    key = "wgs/adj/" + case.name
    idx = graph(case.b, case.n, case.k, key=key)
    douts, dY, bound = [], 0.0, 0.0
    for i, spec in enumerate(case.specs):
        d = dyadic_dout("%s/dout/%d" % (key, i), (case.b, case.n, spec[1], spec[2]))
        g, a = wm.gather_sum_adjoint(d, idx, spec, case.n, case.ldy)
        douts.append(d)
        dY, bound = dY + g, bound + a
    wm.assert_exact(dY, 0.25, bound)
    covered, once = wm.covered_columns(case.specs, case.ldy)
    assert once, case.name
    out = dict(idx=idx, dY=dY, covered=covered, maxima=wm.row_maxima(dY[:, :, covered]))
    if case.k <= 31:
        out["rowptr"], out["records"] = wm.transpose(idx)
    _freeze(out)
    out["douts"] = tuple(douts)
    for d in douts:
        d.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def graph_reference(case):
    idx = graph(case.b, case.n, case.k, case.kind, key="wgs/transpose")
    rowptr, records = wm.transpose(idx)
    return _freeze(dict(idx=idx, rowptr=rowptr, records=records))


@functools.lru_cache(maxsize=None)
def end_to_end_reference(case):
    """Y, idx, the biases (flat float32 arrays; per-sample ones of pitch C, packed by the test), douts, and the guarded outs, dY and bias
    gradients."""
    key = "wgs/e2e/" + case.name
    bits, q = 2, 0.25
    Y = lattice_points(key + "/Y", (case.b, case.n, case.ldy), bits)
    idx = graph(case.b, case.n, case.k, key=key)
    biases, outs, douts, dbias, dY, bound = [], [], [], [], 0.0, 0.0
    for i, (spec, kind) in enumerate(zip(case.specs, case.biases)):
        spec = spec[:5]
        T, P, C, off, offc = spec
        bias = None if kind is None else lattice_points("%s/bias/%d" % (key, i), (C,) if kind == "shared" else (case.b, C), bits)
        stride = C if kind == "sample" else 0
        out = wm.gather_sum(Y, idx, spec, bias, stride)
        wm.assert_exact(out, q, wm.gather_sum(Y, idx, spec, bias, stride, absolute=True))
        d = dyadic_dout("%s/dout/%d" % (key, i), (case.b, case.n, P, C))
        g, a = wm.gather_sum_adjoint(d, idx, spec, case.n, case.ldy)
        dY, bound = dY + g, bound + a
        if kind is not None:
            axes = (0, 1, 2) if kind == "shared" else (1, 2)
            db = d.astype(np.float64).sum(axis=axes)
            wm.assert_exact(db, 0.25, np.abs(d).astype(np.float64).sum(axis=axes))
            dbias.append(db)
        else:
            dbias.append(None)
        biases.append(bias)
        outs.append(out)
        douts.append(d)
    wm.assert_exact(dY, 0.25, bound)
    covered, once = wm.covered_columns([s[:5] for s in case.specs], case.ldy)
    assert once and bool(covered.all()) == case.tiled, case.name
    for a in [Y, idx, dY] + biases + outs + douts + dbias:
        if a is not None:
            a.setflags(write=False)
    return dict(Y=Y, idx=idx, biases=biases, outs=outs, douts=douts, dbias=dbias, dY=dY)


# ---------------------------------------------------------------------------- the table against the launchers' predicates
def check_table():
    """Every case reaches the kernel its line names (wgs_mirror.regime restates the launchers)."""
    for c in FORWARD:
        assert wm.regime("fwd", c.b, c.n, c.k, c.ldy, c.spec, c.bias) == c.want, c
    for c in STATS + STATS_REFUSED:
        assert wm.regime("stats", c.b, c.n, c.k, c.ldy, c.spec, c.bias) == c.want, c
    for c in TRANSPOSE:
        assert wm.regime("transpose", c.b, c.n, c.k, 0, None) == "transpose", c
    for c in TRANSPOSE_REFUSED:
        assert wm.regime("transpose", c.b, c.n, c.k, 0, None) == "invalid", c
    for c in ADJOINT:
        assert tuple(wm.regime("csr", c.b, c.n, c.k, c.ldy, s) for s in c.specs) == c.wants, c
    for c in ADJOINT + ATOMIC_ONLY:
        assert all(wm.regime("bwd", c.b, c.n, c.k, c.ldy, s) == "bwd_atomic" for s in c.specs), c
    for table in (FORWARD, STATS, STATS_REFUSED, ADJOINT, ATOMIC_ONLY, END_TO_END):
        assert len({c.name for c in table}) == len(table)


check_table()
