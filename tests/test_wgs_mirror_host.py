"""The reference of tests/test_gpu_wgs.py checked on the host: tests/wgs_mirror.py against the float64 torch stand-in
(tests/torch_standins.py) and its autograd, its exactness guard on every case the GPU module compares bit for bit, and the case table
of tests/wgs_cases.py against the launchers' predicates as csrc/wgs.hip and csrc/bn_geom.h state them today."""
import numpy as np
import pytest
import torch

import wgs_cases as wc
import wgs_mirror as wm
from torch_standins import EdgeGatherSumTorch


def _name(case):
    return case.name if hasattr(case, "name") else "-".join(map(str, case))


# ---------------------------------------------------------------------------- the mirror against torch
@pytest.mark.parametrize("b,n,k,ldy,specs,kinds", [
    (2, 23, 6, 40, ((3, 4, 8, 0, 24), (2, 2, 4, 32, -1)), ("shared", "sample")),          # a tap-only spec, a per-sample bias
    (3, 17, 10, 56, ((6, 5, 8, 0, 48),), (None,)),
    (1, 9, 4, 30, ((0, 4, 5, 0, 3), (4, 1, 3, 8, 20), (1, 4, 7, 23, -1)), ("sample", None, "shared")),   # T = 0; overlapping reads
])
def test_mirror_equals_the_torch_standin_and_its_autograd(b, n, k, ldy, specs, kinds):
    rng = np.random.default_rng(n * ldy + k)
    Y = rng.standard_normal((b, n, ldy))
    idx = rng.integers(0, n, (b, n, k)).astype(np.int32)
    idx[:, :, 0] = 2
    biases = [None if kind is None else rng.standard_normal((s[2],) if kind == "shared" else (b, s[2])) for s, kind in zip(specs, kinds)]
    douts = [rng.standard_normal((b, n, s[1], s[2])) for s in specs]
    Yt = torch.from_numpy(Y).requires_grad_(True)
    bt = [None if v is None else torch.from_numpy(v).requires_grad_(True) for v in biases]
    refs = EdgeGatherSumTorch.apply(Yt, torch.from_numpy(idx), specs, *bt)
    torch.autograd.backward(refs, [torch.from_numpy(d) for d in douts])
    dY = np.zeros_like(Y)
    for s, kind, bias, dout, ref in zip(specs, kinds, biases, douts, refs):
        pitch = 7                                                 # per-sample rows at a pitch wider than C
        flat = bias
        if kind == "sample":
            flat = np.zeros(b * (s[2] + pitch))
            for i in range(b):
                flat[i * (s[2] + pitch): i * (s[2] + pitch) + s[2]] = bias[i]
        out = wm.gather_sum(Y, idx, s, flat, s[2] + pitch if kind == "sample" else 0)
        np.testing.assert_allclose(out, ref.detach().numpy(), rtol=1e-12, atol=1e-12)
        g, a = wm.gather_sum_adjoint(dout, idx, s, n, ldy)
        assert (a >= np.abs(g) - 1e-12).all()
        dY += g
    np.testing.assert_allclose(dY, Yt.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_mirror_transpose_lists_every_edge_once_and_reproduces_the_adjoint():
    idx = wc.graph(2, 40, 5, key="host/transpose")
    rowptr, records = wm.transpose(idx)
    assert rowptr.dtype == np.int32 and (rowptr[:, 0] == 0).all() and (rowptr[:, -1] == 40 * 5).all()
    spec = (3, 3, 4, 0, -1)
    dout = wc.dyadic_dout("host/transpose/dout", (2, 40, 3, 4)).astype(np.float64)
    want = wm.gather_sum_adjoint(dout, idx, spec, 40, 12)[0]
    got = np.zeros_like(want)
    for s in range(2):
        assert sorted(records[s].tolist()) == sorted((np.arange(40)[:, None] * 32 + np.arange(5)).reshape(-1).tolist())
        for j in range(40):
            recs = records[s, rowptr[s, j]:rowptr[s, j + 1]]
            assert (np.diff(recs) > 0).all() and all(idx[s, r >> 5, r & 31] == j for r in recs)
            for r in recs:
                for t in range(3):
                    if 0 <= (r & 31) - t < 3:
                        got[s, j, t * 4:(t + 1) * 4] += dout[s, r >> 5, (r & 31) - t]
    assert np.array_equal(got, want)
    shuffled = records.copy()
    shuffled[0, rowptr[0, wc.HUB]:rowptr[0, wc.HUB + 1]] = shuffled[0, rowptr[0, wc.HUB]:rowptr[0, wc.HUB + 1]][::-1]
    assert np.array_equal(wm.sort_rows(rowptr, shuffled), records)


def test_row_maxima_are_bit_patterns_of_the_absolute_maximum():
    d = np.array([[[0.25, -3.5, 1.0], [0.0, 0.0, 0.0]]])
    assert wm.row_maxima(d).tolist() == [[np.float32(3.5).view(np.uint32), 0]]
    s, q = wm.partial_totals(d)
    assert s.tolist() == [0.25, -3.5, 1.0] and q.tolist() == [0.0625, 12.25, 1.0]


# ---------------------------------------------------------------------------- the guard on every case
@pytest.mark.parametrize("case", wc.FORWARD + wc.STATS, ids=_name)
def test_guard_accepts_every_forward_and_statistics_case(case):
    ref = wc.forward_reference(case)                              # (runs assert_exact on Y, out, and both column totals)
    T, P, C, off, offc = case.spec
    assert ref["out"].shape == (case.b, case.n, P, C) and ref["total"].shape == (C,)
    assert (ref["bias"] is None) == (case.bias is None)
    if isinstance(case.bias, int):
        assert ref["bstride"] == case.bias and ref["bias"].shape == (case.b * case.bias,)
    plants = wc.planted(ref["idx"])
    assert plants == (True, True, True, True), plants
    assert ref["Y"].min() == -1.0 and ref["Y"].max() < 1.0 and len(np.unique(ref["Y"])) == 2 ** (case.bits + 1)       # the whole lattice is in use


@pytest.mark.parametrize("case", wc.ADJOINT + wc.ATOMIC_ONLY, ids=_name)
def test_guard_accepts_every_adjoint_case(case):
    ref = wc.adjoint_reference(case)
    assert ref["dY"].shape == (case.b, case.n, case.ldy) and wc.planted(ref["idx"]) == (True, True, True, True)
    assert not ref["dY"][:, :, ~ref["covered"]].any()
    for d in ref["douts"]:
        assert not np.signbit(d[d == 0]).any() and np.array_equal(d * 4, np.rint(d * 4)) and np.abs(d).max() == 2.0
    hub = ref["rowptr"][:, wc.HUB + 1] - ref["rowptr"][:, wc.HUB]
    assert (hub >= case.n + case.k - 1).all() and (np.diff(ref["rowptr"], axis=1)[:, case.n - 2] == 0).all()
    for T, P, C, off, offc in case.specs:                         # nobody names point n - 2: its tap columns are exactly zero
        assert not ref["dY"][:, case.n - 2, off:off + T * C].any()


@pytest.mark.parametrize("case", wc.TRANSPOSE, ids=_name)
def test_transposed_graph_cases_hold_their_plants(case):
    ref = wc.graph_reference(case)
    deg = np.diff(ref["rowptr"], axis=1)
    assert ref["rowptr"].shape == (case.b, case.n + 1) and (deg.sum(1) == case.n * case.k).all()
    if case.kind == "allone":
        assert (deg[:, wc.HUB % case.n] == case.n * case.k).all()
    elif case.n >= 6 and case.k >= 2:
        assert wc.planted(ref["idx"]) == (True, True, True, True)
    elif case.n >= 6:                                             # k = 1: the queries 0 and n - 1 carry the extremes instead of the hub
        assert wc.planted(ref["idx"])[2:] == (True, True) and (deg[:, wc.HUB] == case.n - 2).all()
    assert {c.k for c in wc.TRANSPOSE} == {1, 10, 31} and {c.b for c in wc.TRANSPOSE} == {1, 3}
    assert {c.n for c in wc.TRANSPOSE} == {1, 1000, 1025} and [c.k for c in wc.TRANSPOSE_REFUSED][0] == 32


@pytest.mark.parametrize("case", wc.END_TO_END, ids=_name)
def test_guard_accepts_the_end_to_end_cases(case):
    ref = wc.end_to_end_reference(case)
    assert len(ref["outs"]) == len(case.specs) and ref["dY"].shape == (case.b, case.n, case.ldy)
    for kind, db, spec in zip(case.biases, ref["dbias"], case.specs):
        assert (db is None) == (kind is None) and (db is None or db.shape == ((spec[2],) if kind == "shared" else (case.b, spec[2])))
    # the per-sample bias gradient is taken from dY's centre columns (EdgeGatherSum.backward): the same numbers
    for kind, db, spec in zip(case.biases, ref["dbias"], case.specs):
        if kind == "sample":
            assert spec[4] >= 0 and np.array_equal(ref["dY"][:, :, spec[4]:spec[4] + spec[2]].sum(1), db)


def test_guard_rejects_what_is_not_exact():
    case = wc.by_name(wc.FORWARD, "flat4_small")
    ref = wc.forward_reference(case)
    bad = ref["Y"].copy()
    bad[1, 7, 3] = np.float32(0.3)
    with pytest.raises(AssertionError, match="multiple"):
        wm.assert_exact(wm.gather_sum(bad, ref["idx"], case.spec), 2.0 ** -case.bits)
    big = ref["Y"] + np.float32(2.0 ** 22)                       # eight terms of 2^22 on a 2^-4 lattice: past 2^24 quanta
    with pytest.raises(AssertionError, match="2\\^24"):
        wm.assert_exact(wm.gather_sum(big, ref["idx"], case.spec), 2.0 ** -case.bits, wm.gather_sum(big, ref["idx"], case.spec, absolute=True))


# ---------------------------------------------------------------------------- the table against the launchers
def test_constants_are_read_from_the_sources():
    c = wm.source_constants()
    assert c == {"WGS_THREADS": 256, "WGS_XU": 4, "CW": 32, "SCW": 16, "BCW": 64, "FWD_MIN": 65536, "STATS_MIN": 65536,
                 "STATS_ROWS_MAX": 65536, "CSR_MIN": 65536, "BN_THREADS": 256, "BN_WANT": 1024, "BN_MIN_LANES": 16, "BN_ROWS_MAX": 65536}
    with pytest.raises(AssertionError, match="launcher changed"):
        wm._one("if (v4 && xcd && T <= 9)", r"T <= 8 && ", "a predicate that is gone")
    assert wm.cl_geometry(8192, 64) == (16, 1, 32, 256) and wm.cl_geometry(1040, 16384) == (256, 16, 62, 17)


def test_every_regime_is_reached_and_named_by_its_case():
    wc.check_table()
    hit = {c.want for c in wc.FORWARD + wc.STATS + wc.STATS_REFUSED} | {w for c in wc.ADJOINT + wc.ATOMIC_ONLY for w in c.wants}
    hit.add(wm.regime("transpose", 1, 8, 4, 0, None))
    assert hit == {r for names in wm.REGIMES.values() for r in names} | {"invalid"}
    # the causes of the scalar kernel, one at a time
    for c in wc.FORWARD:
        if c.want == "fwd_scalar":
            T, P, C, off, offc = c.spec
            causes = [C % 4 != 0, c.ldy % 4 != 0, off % 4 != 0, offc % 4 != 0, isinstance(c.bias, int) and c.bias % 4 != 0]
            assert sum(causes) == 1, c
    assert len([c for c in wc.FORWARD if c.want == "fwd_scalar"]) == 5
    assert {c.spec[0] for c in wc.FORWARD if c.want == "fwd_xcd_rt"} >= {0, 1, 3, 8}
    assert {c.spec[0] for c in wc.STATS if c.want == "stats_xcd_rt"} >= {0, 1, 3, 8} <= {c.spec[0] for c in wc.STATS if c.want == "stats_geom_rt"}
    assert {s[0] for c in wc.ADJOINT for s, w in zip(c.specs, c.wants) if w == "csr_xcd_rt"} >= {1, 4, 8}
    assert {s[2] // 4 for c in wc.ADJOINT for s, w in zip(c.specs, c.wants) if w.startswith("csr_xcd")} >= {40, 64, 80}
    assert {c.spec[1] for c in wc.FORWARD if c.want.startswith("fwd_xcd")} >= {1, 3, 7}
    for want in ("fwd_xcd", "stats_xcd"):
        table = wc.FORWARD if want == "fwd_xcd" else wc.STATS
        mapped = [c for c in table if c.want.startswith(want)]
        assert any(c.spec[4] < 0 for c in mapped) and any(c.bias is None for c in mapped) and any(c.bias == "shared" for c in mapped)
        assert any(isinstance(c.bias, int) and c.bias > c.spec[2] for c in mapped)
    assert any(s[4] < 0 for c in wc.ADJOINT for s, w in zip(c.specs, c.wants) if w.startswith("csr_xcd"))
    assert any(s[0] == 0 for c in wc.ADJOINT for s in c.specs) and any(c.n % 4 for c in wc.ADJOINT if "csr_xcd6" in c.wants)
    assert {len(c.specs) for c in wc.ADJOINT if wm.covered_columns(c.specs, c.ldy)[0].all()} >= {1, 2, 3}


def test_every_threshold_has_a_case_on_each_side():
    k = wm.constants()
    units = lambda c: c.n * c.spec[1] * (c.spec[2] // 4)
    for table, lo, hi, key in ((wc.FORWARD, "fwd_flat4", "fwd_xcd", "FWD_MIN"), (wc.STATS, "stats_geom", "stats_xcd", "STATS_MIN")):
        for T in (6, 3 if table is wc.FORWARD else 1):
            under = [c for c in table if c.spec[0] == T and c.want.startswith(lo) and k[key] - c.spec[1] * (c.spec[2] // 4) <= units(c) < k[key]]
            at = [c for c in table if c.spec[0] == T and c.want.startswith(hi) and units(c) == k[key]]
            assert under and at, (key, T)
            assert any(u.spec == a.spec and u.n + 1 == a.n for u in under for a in at)       # one point apart, nothing else differs
    # T <= 8 on the forward path: the first T beyond it and T = 10, over the threshold, stay on the flat kernel
    assert {c.spec[0] for c in wc.FORWARD if c.want == "fwd_flat4" and units(c) >= k["FWD_MIN"]} == {9, 10}
    adj = [(c, s, w) for c in wc.ADJOINT for s, w in zip(c.specs, c.wants) if len(c.specs) == 1]
    for T, hi in ((6, "csr_xcd6"), (10, "csr_xcd10"), (4, "csr_xcd_rt")):
        step = [s for c, s, w in adj if s[0] == T][0]
        step = T * (step[2] // 4)
        assert [c for c, s, w in adj if s[0] == T and w == "csr_small" and k["CSR_MIN"] - step <= c.n * step < k["CSR_MIN"]], T
        assert [c for c, s, w in adj if s[0] == T and w == hi and k["CSR_MIN"] <= c.n * step < k["CSR_MIN"] + step], T
    assert [c for c, s, w in adj if s[0] == 9 and w == "csr_small" and c.n * 9 * (s[2] // 4) >= k["CSR_MIN"]]
    # gy >= b: a shape over the statistics threshold whose BatchNorm geometry has fewer row blocks than samples
    c = wc.by_name(wc.STATS, "geom_rt_gy_below_b")
    assert units(c) >= k["STATS_MIN"] and wm.cl_geometry(c.b * c.n * c.spec[1], c.spec[2])[2] < c.b and wm.wgs_slabs_ok(c.n, c.k, c.ldy, c.spec[1], c.spec[2])


def test_task_mapping_edges_at_every_chunk_width():
    """Ragged rows (a row lane whose first row is past the end included), chunks below / exactly / beyond the width, a task count
    that is no multiple of the 8 dealt out per round, spare partial rows: at the default widths and at those of the child processes."""
    fwd_widths = [None] + [wc.switches(s)[1]["fwd"] for s in wc.WORKER_SETTINGS[1:]]
    for cw in fwd_widths:
        names = [c.name for c in wc.FORWARD if c.want.startswith("fwd_xcd")] if cw is None else wc.WORKER_FORWARD
        geo = [(c, wm.geometry("fwd", c.b, c.n, c.k, c.ldy, c.spec, cw)) for c in (wc.by_name(wc.FORWARD, nm) for nm in names)]
        lanes = lambda g: g["per_block"] // wm.constants()["WGS_XU"]
        tail = [(c.n * c.spec[1]) % g["per_block"] for c, g in geo]
        assert any(0 < t < lanes(g) for t, (c, g) in zip(tail, geo)), cw      # some row lanes of the last block start past the end
        assert any(t >= lanes(g) for t, (c, g) in zip(tail, geo)) and any(t == 0 for t in tail), cw
        cvs = [(c.spec[2] // 4, g["cw"]) for c, g in geo]
        assert any(cv < w for cv, w in cvs) or cw == 8            # (C / 4 = 4 would take n * P = 16384 rows)
        assert any(cv == w for cv, w in cvs) and any(cv > w and cv % w for cv, w in cvs), cw
        assert any(g["ntasks"] % 8 for c, g in geo)
    for cw in [None] + [wc.switches(s)[1]["stats"] for s in wc.WORKER_SETTINGS[1:]]:
        names = [c.name for c in wc.STATS if c.want.startswith("stats_xcd")] if cw is None else [n for n in wc.WORKER_STATS if "xcd" in n]
        geo = [wm.geometry("stats", c.b, c.n, c.k, c.ldy, c.spec, cw) for c in (wc.by_name(wc.STATS, nm) for nm in names)]
        assert any(g["spare"] > 0 for g in geo) and any(g["spare"] == 0 for g in geo) and any(g["nchunk"] > 1 for g in geo), cw
        assert any((c.spec[2] // 4) % g["cw"] for c, g in zip((wc.by_name(wc.STATS, nm) for nm in names), geo)), cw
    for cw in [None] + [wc.switches(s)[1]["csr"] for s in wc.WORKER_SETTINGS[1:]]:
        names = [c.name for c in wc.ADJOINT] if cw is None else wc.WORKER_ADJOINT
        geo = [(c, s, wm.geometry("csr", c.b, c.n, c.k, c.ldy, s, cw)) for c in (wc.by_name(wc.ADJOINT, nm) for nm in names)
               for s, w in zip(c.specs, c.wants) if w.startswith("csr_xcd")]
        assert any(c.n % g["per_block"] for c, s, g in geo) and any((s[2] // 4) % g["cw"] for c, s, g in geo), cw
        assert any((s[2] // 4) == g["cw"] for c, s, g in geo) or cw is not None
    assert sorted(wc.switches(s) != (1, {"fwd": None, "stats": None, "csr": None}) for s in wc.WORKER_SETTINGS) == [True] * 4
    assert {s.get("PDGN_WGS_CW") for s in wc.WORKER_SETTINGS} == {None, "8", "16", "64"}
    assert {s.get("PDGN_WGS_SCW") for s in wc.WORKER_SETTINGS} == {None, "8", "32", "64"}
    assert {s.get("PDGN_WGS_BCW") for s in wc.WORKER_SETTINGS} == {None, "8", "16", "32"}
    assert wc.WORKER_SETTINGS[0] == {"PDGN_WGS_XCD": "0"}
