"""Host mirror of the window gather-sum family (csrc/wgs.hip): numpy only, float64, written from the formulas the kernels quote, so
that tests can demand equal bits on inputs whose arithmetic is exact in float32.

    forward      out[b,n,p,c] = bias[b*bias_bstride + c] + Y[b,n,offc+c] + sum_{t<T} Y[b, idx[b,n,p+t], off + t*C + c]
                 (offc < 0: no centre term; T = 0: bias and centre alone)
    adjoint      dY[b,j,off+t*C+c] = sum_{(n',s) in in(j), 0 <= s-t < P} dout[b,n',s-t,c],  dY[b,j,offc+c] = sum_p dout[b,j,p,c]
    transpose    in(j) = {(n', s): idx[b,n',s] == j}, one record n'*32 + s per edge, rowptr the exclusive running in-degree
    statistics   per column of `out` viewed as (b*n*P, C): sum and sum of squares
    row maxima   the bit pattern of max_c |dY[b,j,c]|

A spec is (T, P, C, off, offc), as in pdgn_amd.deconv.EdgeGatherSum.

Exactness.  Every operation is a sum of float32 values.  With Y and bias on a dyadic lattice (hashweights.lattice_points) and dout in
quarter steps, every term is a multiple of a power of two (the `quantum`) and every sum stays far below 2^24 quanta: each partial sum
is then a float32 in whatever order the additions are made -- register accumulators, cross-lane exchanges, atomics.  `assert_exact`
(tests/localpair_mirror.py) checks exactly that on the host before a device result is compared.

`regime` restates the launchers' dispatch predicates; the constants in them are READ from the sources' text, so a launcher that
changes makes the host test fail instead of leaving this file stale."""
import os
import re

import numpy as np

from localpair_mirror import assert_exact  # noqa: F401  (the guard, re-exported)

F64 = np.float64
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pdgn_amd", "csrc")


# ---------------------------------------------------------------------------- forward
def _bias_rows(bias, bias_bstride, b, C):
    if bias is None:
        return np.zeros((b, C), F64)
    flat = np.asarray(bias, dtype=F64).reshape(-1)
    return np.stack([flat[s * bias_bstride: s * bias_bstride + C] for s in range(b)])


def gather_sum(Y, idx, spec, bias=None, bias_bstride=0, absolute=False):
    """Y (b, n, ldy), idx (b, n, k), bias a flat array read at [s * bias_bstride + c] (bias_bstride 0: shared) or None
    -> out (b, n, P, C) float64.  absolute: the sum of the terms' absolute values instead (what `assert_exact` bounds)."""
    T, P, C, off, offc = spec
    Y, idx = np.asarray(Y, dtype=F64), np.asarray(idx, dtype=np.int64)
    if absolute:
        Y = np.abs(Y)
    b, n, _ = Y.shape
    bias_rows = _bias_rows(bias, bias_bstride, b, C)
    out = np.zeros((b, n, P, C), F64)
    out += (np.abs(bias_rows) if absolute else bias_rows)[:, None, None, :]
    if offc >= 0:
        out += Y[:, :, None, offc:offc + C]
    rows = np.arange(b)[:, None, None]
    for t in range(T):
        out += Y[rows, idx[:, :, t:t + P], off + t * C: off + (t + 1) * C]
    return out


# ---------------------------------------------------------------------------- adjoint
def gather_sum_adjoint(dout, idx, spec, n, ldy):
    """dout (b, n, P, C), idx (b, n, k) -> (dY, abs): dY (b, n, ldy) float64, zero in the columns the spec does not cover, and the sum
    of |terms| behind every element."""
    T, P, C, off, offc = spec
    dout, idx = np.asarray(dout, dtype=F64), np.asarray(idx, dtype=np.int64)
    b = dout.shape[0]
    assert dout.shape == (b, n, P, C) and idx.shape[:2] == (b, n)
    res = []
    for g in (dout, np.abs(dout)):
        dY = np.zeros((b, n, ldy), F64)
        for s in range(b):
            for t in range(T):
                dst = dY[s, :, off + t * C: off + (t + 1) * C]
                for slot in range(t, t + P):                             # the in-edges (n', slot) with 0 <= slot - t < P
                    np.add.at(dst, idx[s, :, slot], g[s, :, slot - t, :])
            if offc >= 0:
                dY[s, :, offc:offc + C] += g[s].sum(1)
        res.append(dY)
    return res[0], res[1]


def covered_columns(specs, ldy):
    """Boolean (ldy,): the columns of dY that the specs write; and whether every covered column is covered once."""
    hits = np.zeros(ldy, np.int64)
    for T, P, C, off, offc in specs:
        hits[off:off + T * C] += 1
        if offc >= 0:
            hits[offc:offc + C] += 1
    return hits > 0, bool((hits <= 1).all())


# ---------------------------------------------------------------------------- transposed graph
def transpose(idx):
    """idx (b, n, k) -> rowptr (b, n + 1) int32, the exclusive cumulative in-degree of every sample, and records (b, n * k) int32:
    every source point's records n' * 32 + s in ascending order, the points' lists one after the other (rowptr delimits them)."""
    idx = np.asarray(idx, dtype=np.int64)
    b, n, k = idx.shape
    assert k <= 31
    rowptr = np.zeros((b, n + 1), np.int32)
    records = np.empty((b, n * k), np.int32)
    rec = (np.arange(n)[:, None] * 32 + np.arange(k)[None, :]).reshape(-1)
    for s in range(b):
        src = idx[s].reshape(-1)
        rowptr[s, 1:] = np.cumsum(np.bincount(src, minlength=n))
        records[s] = rec[np.lexsort((rec, src))]
    return rowptr, records


def sort_rows(rowptr, edges):
    """A device's edges (b, n * k) with every source point's segment sorted: comparable with `transpose`'s records."""
    rowptr, edges = np.asarray(rowptr, dtype=np.int64), np.asarray(edges)
    out = np.empty_like(edges)
    for s in range(edges.shape[0]):
        seg = np.repeat(np.arange(rowptr.shape[1] - 1), np.diff(rowptr[s]))
        out[s] = edges[s][np.lexsort((edges[s], seg))]
    return out


# ---------------------------------------------------------------------------- statistics, maxima
def partial_totals(out):
    """out (..., C) float64 -> (sum, sum of squares) per column over all rows, exact in float64 for guarded cases."""
    o = np.asarray(out, dtype=F64).reshape(-1, np.shape(out)[-1])
    return o.sum(0), (o * o).sum(0)


def row_maxima(dY):
    """dY (b, n, cols) float64 -> uint32 (b, n): the float32 bit pattern of every row's max |dY|."""
    return np.abs(np.asarray(dY, dtype=F64)).max(axis=-1).astype(np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- the launchers' constants, read from their text
def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(text, pattern, what):
    found = re.findall(pattern, text)
    if len(found) != 1:
        raise AssertionError("csrc: expected exactly one `%s` (%s), found %d: the launcher changed, restate tests/wgs_mirror.py"
                             % (pattern, what, len(found)))
    return found[0]


def source_constants():
    """Everything `regime` depends on, parsed out of wgs.hip and bn_geom.h."""
    w, g = _read("wgs.hip"), _read("bn_geom.h")
    c = {}
    c["WGS_THREADS"] = int(_one(w, r"#define WGS_THREADS (\d+)\n", "block size"))
    c["WGS_XU"] = int(_one(w, r"#define WGS_XU (\d+) ", "rows in flight"))
    c["CW"] = int(_one(w, r'wgs_cw\("PDGN_WGS_CW", (\d+)\)', "forward chunk width"))
    c["SCW"] = int(_one(w, r'wgs_cw\("PDGN_WGS_SCW", (\d+)\)', "statistics chunk width"))
    c["BCW"] = int(_one(w, r'wgs_cw\("PDGN_WGS_BCW", (\d+)\)', "adjoint chunk width"))
    _one(w, r"return \(w == 8 \|\| w == 16 \|\| w == 32 \|\| w == 64\) \? w : dflt;", "accepted chunk widths")
    c["FWD_MIN"] = int(_one(w, r"if \(v4 && xcd && T <= 8 && \(long long\)n \* P \* \(C / 4\) >= (\d+) && wgs_slabs_ok\(n, k, ldy, P, C\)\)",
                            "forward predicate"))
    c["STATS_MIN"] = int(_one(w, r"if \(xcd && \(long long\)n \* P \* \(C / 4\) >= (\d+) && gy >= b && wgs_slabs_ok\(n, k, ldy, P, C\)\)",
                              "statistics predicate"))
    c["STATS_ROWS_MAX"] = int(_one(w, r"if \(blocks <= 0x7fffffffLL && rows <= (\d+)\)", "statistics row bound"))
    c["CSR_MIN"] = int(_one(w, r"if \(xcd && \(T <= 8 \|\| T == 10\) && \(long long\)n \* T \* \(C / 4\) >= (\d+) && wgs_slabs_ok\(n, k, ldy, P, C\)\)",
                            "CSR adjoint predicate"))
    _one(w, r"const bool v4 = \(C % 4 == 0\) && \(ldy % 4 == 0\) && \(off % 4 == 0\) && \(offc < 0 \|\| offc % 4 == 0\) &&\n"
            r"\s+\(!bias \|\| \(bias_bstride % 4 == 0 && \(\(size_t\)bias & 15\) == 0\)\);", "float4 predicate")
    _one(w, r"if \(!wgs_ok\(b, n, k, ldy, T, P, C, off, offc\) \|\| b < 1 \|\| T > 8\) return PDGN_ERR_INVALID;", "statistics refusals")
    _one(w, r"if \(\(C % 4\) \|\| \(ldy % 4\) \|\| \(off % 4\) \|\| \(offc >= 0 && offc % 4\) \|\| \(bias && bias_bstride % 4\)\) return PDGN_ERR_INVALID;",
         "statistics alignment refusals")
    _one(w, r"if \(!wgs_ok\(b, n, k, ldy, T, P, C, off, offc\) \|\| C % 4 \|\| ldy % 4 \|\| off % 4 \|\| \(offc >= 0 && offc % 4\) \|\| k > 31\)",
         "CSR adjoint refusals")
    _one(w, r"if \(b < 0 \|\| n < 1 \|\| k < 1 \|\| k > 31 \|\| \(long long\)n \* 32 > 0x7fffffffLL\) return PDGN_ERR_INVALID;", "transpose refusals")
    _one(w, r"return b >= 0 && n >= 1 && k >= 1 && T >= 0 && \(T >= 1 \|\| offc >= 0\) && P >= 1 && C >= 1 && T \+ P - 1 <= k && off >= 0 &&\n"
            r"\s+off \+ T \* C <= ldy && \(offc < 0 \|\| offc \+ C <= ldy\);", "wgs_ok")
    _one(w, r"return \(long long\)n \* ldy \* 4 < 0x7fffffffLL && \(long long\)n \* P \* C \* 4 < 0x7fffffffLL && \(long long\)n \* k \* 4 < 0x7fffffffLL &&\n"
            r"\s+\(long long\)n \* P \* P < 0x100000000LL && ldy \* 4LL < \(1 << 24\) && \(long long\)P \* C \* 4 < \(1 << 24\) && n < \(1 << 24\) &&\n"
            r"\s+\(long long\)n \* P < \(1 << 24\);", "wgs_slabs_ok")
    if len(re.findall(r"if \(T == 6\)", w)) != 4 or len(re.findall(r"else if \(T == 10\)", w)) != 1:
        raise AssertionError("csrc/wgs.hip: the compile-time tap counts of the launchers changed")
    _one(w, r"const int bpt = cdiv\(\(long long\)n \* P, WGS_THREADS / cw \* WGS_XU\);", "forward blocks per task")
    _one(w, r"bpt = cdiv\(n, WGS_THREADS / 64\);", "adjoint blocks per task")
    _one(w, r"const int RLU = WGS_THREADS / cw \* WGS_XU;\n\s+int bpt = gy / b;\n\s+int rows = cdiv\(\(long long\)n \* P, bpt\);\n"
            r"\s+rows = cdiv\(rows, RLU\) \* RLU;\n\s+bpt = cdiv\(\(long long\)n \* P, rows\);", "statistics blocks per task")
    c["BN_THREADS"] = int(_one(g, r"#define BN_THREADS (\d+)\n", "BatchNorm block size"))
    c["BN_WANT"] = int(_one(g, r"long long want = (\d+) / \*gx;", "workgroups in flight"))
    c["BN_MIN_LANES"] = int(_one(g, r"const long long min_rows = \(long long\)rl \* (\d+);", "rows per lane"))
    c["BN_ROWS_MAX"] = int(_one(g, r"rows = rows > (\d+) \? \1 : rows;", "row cap"))
    _one(g, r"while \(p < cg && p < BN_THREADS\) p <<= 1;", "column groups per block")
    return c


_CONST = None


def constants():
    global _CONST
    if _CONST is None:
        _CONST = source_constants()
    return _CONST


def cdiv(a, b):
    return -(-a // b)


def cl_geometry(R, C):
    """csrc/bn_geom.h -> (cgb, gx, gy, rows_per_block)."""
    k = constants()
    cg = C // 4
    p = 1
    while p < cg and p < k["BN_THREADS"]:
        p <<= 1
    gx = cdiv(cg, p)
    rl = k["BN_THREADS"] // p
    want = max(1, k["BN_WANT"] // gx)
    rows = max(cdiv(R, want), rl * k["BN_MIN_LANES"])
    rows = min(rows, k["BN_ROWS_MAX"])
    rows = cdiv(rows, rl) * rl
    return p, gx, cdiv(R, rows), rows


def wgs_ok(b, n, k, ldy, spec):
    T, P, C, off, offc = spec
    return (b >= 0 and n >= 1 and k >= 1 and T >= 0 and (T >= 1 or offc >= 0) and P >= 1 and C >= 1 and T + P - 1 <= k and off >= 0
            and off + T * C <= ldy and (offc < 0 or offc + C <= ldy))


def wgs_slabs_ok(n, k, ldy, P, C):
    return (n * ldy * 4 < 0x7fffffff and n * P * C * 4 < 0x7fffffff and n * k * 4 < 0x7fffffff and n * P * P < 0x100000000
            and ldy * 4 < (1 << 24) and P * C * 4 < (1 << 24) and n < (1 << 24) and n * P < (1 << 24))


def _aligned(ldy, spec, bias_kind):
    T, P, C, off, offc = spec
    pitch_ok = not isinstance(bias_kind, int) or bias_kind % 4 == 0          # bias_kind: None, "shared" or the per-sample pitch
    return C % 4 == 0 and ldy % 4 == 0 and off % 4 == 0 and (offc < 0 or offc % 4 == 0) and pitch_ok


def _cw(which, cw):
    d = constants()[which]
    return cw if cw in (8, 16, 32, 64) else d


def geometry(entry, b, n, k, ldy, spec, cw=None):
    """The numbers of a task-mapped launch (whether or not `regime` takes it): chunk width, chunks, tasks, rows (forward, statistics)
    or source points (adjoint) per block, blocks per task, and for the statistics the BatchNorm geometry's gy and its spare rows."""
    T, P, C, off, offc = spec
    c = constants()
    if entry == "fwd":
        w = _cw("CW", cw)
        per = c["WGS_THREADS"] // w * c["WGS_XU"]
        g = dict(cw=w, per_block=per, bpt=cdiv(n * P, per))
    elif entry == "stats":
        w = _cw("SCW", cw)
        gy = cl_geometry(b * n * P, C)[2]
        g = dict(cw=w, gy=gy)
        if gy >= b:
            rlu = c["WGS_THREADS"] // w * c["WGS_XU"]
            rows = cdiv(cdiv(n * P, gy // b), rlu) * rlu
            g.update(per_block=rows, bpt=cdiv(n * P, rows))
            g["spare"] = gy - b * g["bpt"]
    else:
        assert entry == "csr", entry
        w = _cw("BCW", cw)
        g = dict(cw=w, per_block=c["WGS_THREADS"] // 64, bpt=cdiv(n, c["WGS_THREADS"] // 64))
    g["nchunk"] = cdiv(C // 4, w)
    g["ntasks"] = b * g["nchunk"]
    return g


def regime(entry, b, n, k, ldy, spec, bias_kind=None, xcd=1, cw=None):
    """Which kernel an entry point launches: entry "fwd" (pdgn_window_gather_sum), "stats" (.._stats), "bwd" (.._backward), "csr"
    (.._backward_csr) or "transpose" (pdgn_knn_graph_transpose: spec is ignored).  bias_kind: None, "shared" or an int, the
    per-sample pitch (the pointer is assumed 16-byte aligned).  xcd: PDGN_WGS_XCD; cw: PDGN_WGS_CW / _SCW / _BCW of that entry.
    "invalid" where the entry point returns PDGN_ERR_INVALID."""
    c = constants()
    if entry == "transpose":
        return "transpose" if (b >= 0 and n >= 1 and 1 <= k <= 31 and n * 32 <= 0x7fffffff) else "invalid"
    T, P, C, off, offc = spec
    if not wgs_ok(b, n, k, ldy, spec):
        return "invalid"
    tt = {6: "6", 10: "10"}
    if entry == "fwd":
        if not _aligned(ldy, spec, bias_kind):
            return "fwd_scalar"
        if xcd and T <= 8 and n * P * (C // 4) >= c["FWD_MIN"] and wgs_slabs_ok(n, k, ldy, P, C):
            return "fwd_xcd6" if T == 6 else "fwd_xcd_rt"
        return "fwd_flat4"
    if entry == "stats":
        if b < 1 or T > 8 or not _aligned(ldy, spec, bias_kind):
            return "invalid"
        if xcd and n * P * (C // 4) >= c["STATS_MIN"] and cl_geometry(b * n * P, C)[2] >= b and wgs_slabs_ok(n, k, ldy, P, C) \
                and geometry("stats", b, n, k, ldy, spec, cw)["per_block"] <= c["STATS_ROWS_MAX"]:
            return "stats_xcd6" if T == 6 else "stats_xcd_rt"
        return "stats_geom6" if T == 6 else "stats_geom_rt"
    if entry == "bwd":
        return "bwd_atomic"
    assert entry == "csr", entry
    if not _aligned(ldy, spec, None) or k > 31:
        return "invalid"
    if xcd and (T <= 8 or T == 10) and n * T * (C // 4) >= c["CSR_MIN"] and wgs_slabs_ok(n, k, ldy, P, C):
        return "csr_xcd" + tt.get(T, "_rt")
    return "csr_small"


REGIMES = {"fwd": ("fwd_scalar", "fwd_flat4", "fwd_xcd6", "fwd_xcd_rt"),
           "stats": ("stats_geom6", "stats_geom_rt", "stats_xcd6", "stats_xcd_rt"),
           "csr": ("csr_small", "csr_xcd6", "csr_xcd10", "csr_xcd_rt"),
           "bwd": ("bwd_atomic",), "transpose": ("transpose",)}
