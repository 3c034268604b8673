"""The cases of tests/test_gpu_wgs_adjoint.py: the task-mapped CSR adjoint (csrc/wgs.hip, wgs_bwd_csr_xcd_kernel) on graphs whose
in-degrees are chosen against the way the chunk-width-64 body walks a source point's records -- 64 per wave-wide record load,
WGS_BU (WGS_BU1 where P = 1) in-edges per group of row loads; both numbers are READ from wgs.hip's text.  Inputs and the exactness
guard are those of tests/wgs_cases.py (quarter-step dout, wgs_mirror.assert_exact before anything is handed out); shared by the
host test (tests/test_wgs_adjoint_host.py), the GPU module and its child process (tests/wgs_adjoint_worker.py).

A graph (b, n, k >= 10) holds, in every sample:
    point 5..14     in-degrees 0, 1, 3, BU, BU + 1, BU1, BU1 + 1, 64, 65, 130 (DEGREES, in this order)
    point 20        a hub all of whose 100 records carry slot 2
    point 21        a hub whose 120 records carry the slots 8 and 9 alone: outside the window of every tap t < 4 at T = 6, P = 5,
                    t < 8 at T = 10, P = 1, t < 2 at T = 4, P = 7 -- those taps of row 21 must come out as +0.0
    points 30..     everything else
The exactness guard rejects NONE of the table's entries (checked on the host: with |dout| <= 2 in quarter steps the largest sum of
|terms| at one destination is 130 * 5 * 8 = 5200 quanta, far below 2^24)."""
import functools
import os

import numpy as np

import wgs_cases as wc
import wgs_mirror as wm

K = 10
HUB_SLOT, HUB_OUT = 20, 21
FIRST, FILL0 = 5, 30
MULT = (37, 39, 41, 43, 45, 47, 49, 53, 55)                  # per-sample strides of the designated records (no multiple of 17 = sqrt(289))


def load_groups():
    """(WGS_BU, WGS_BU1) as csrc/wgs.hip defines them."""
    with open(os.path.join(wm.CSRC, "wgs.hip")) as f:
        w = f.read()
    return (int(wm._one(w, r"#define WGS_BU (\d+) ", "in-edges per load group")),
            int(wm._one(w, r"#define WGS_BU1 (\d+) ", "in-edges per load group at P = 1")))


BU, BU1 = load_groups()
DEGREES = (0, 1, 3, BU, BU + 1, BU1, BU1 + 1, 64, 65, 130)

# name, b, n, k, ldy, specs, wants: 64 untouched columns in front of and behind what the spec covers
CASES = [
    wc.Adj("T10_P1_C256_b3", 3, 128, K, 2944, ((10, 1, 256, 64, 2624),), ("csr_xcd10",)),          # 3 tasks
    wc.Adj("T10_P1_C256_b9", 9, 128, K, 2944, ((10, 1, 256, 64, 2624),), ("csr_xcd10",)),          # 9 tasks
    wc.Adj("T6_P5_C512_b3", 3, 128, K, 3712, ((6, 5, 512, 64, 3136),), ("csr_xcd6",)),             # 6 tasks
    wc.Adj("T6_P5_C512_b9", 9, 128, K, 3712, ((6, 5, 512, 64, 3136),), ("csr_xcd6",)),             # 18 tasks
    wc.Adj("T4_P7_C512", 3, 128, K, 2688, ((4, 7, 512, 64, 2112),), ("csr_xcd_rt",)),              # exactly 65536 units
    wc.Adj("T4_P7_C512_nocentre", 3, 128, K, 2176, ((4, 7, 512, 64, -1),), ("csr_xcd_rt",)),
    wc.Adj("T10_P1_C176", 3, 160, K, 2064, ((10, 1, 176, 64, 1824),), ("csr_xcd10",)),             # C / 4 = 44: lanes past CV
    wc.Adj("T10_P2_C256_k11", 3, 128, 11, 2944, ((10, 2, 256, 64, 2624),), ("csr_xcd10",)),         # ten taps with a window: the unstaged loop
    wc.Adj("T6_P1_C512", 3, 128, K, 3712, ((6, 1, 512, 64, 3136),), ("csr_xcd6",)),                # one row per in-edge, slots 6..9 feed no tap
]


def graph(b, n, k=K):
    """idx (b, n, K) int32 with the plants of the module docstring."""
    assert n >= 128 and b <= len(MULT)
    idx = np.full((b, n, k), -1, np.int64)
    idx[:, :100, 2] = HUB_SLOT
    idx[:, :60, 8] = HUB_OUT
    idx[:, :60, 9] = HUB_OUT
    want = np.concatenate([np.full(d, FIRST + i) for i, d in enumerate(DEGREES)])
    for s in range(b):
        free = np.argwhere(idx[s] < 0)                       # (query, slot), row-major
        perm = (np.arange(len(want)) * MULT[s]) % len(want)
        take = np.zeros(len(free), bool)
        take[np.arange(len(want)) * 3] = True                # every third free cell: the lists mix slots and queries
        cells, rest = free[take], free[~take]
        idx[s, cells[:, 0], cells[:, 1]] = want[perm]
        idx[s, rest[:, 0], rest[:, 1]] = FILL0 + (np.arange(len(rest)) * (7 + 2 * s)) % (n - FILL0)
    return idx.astype(np.int32)


def in_degrees(idx):
    return np.stack([np.bincount(s.reshape(-1), minlength=idx.shape[1]) for s in idx])


@functools.lru_cache(maxsize=None)
def reference(case):
    """As wgs_cases.adjoint_reference, on this module's graph."""
    key = "wgs/adjx/" + case.name
    idx = graph(case.b, case.n, case.k)
    douts, dY, bound = [], 0.0, 0.0
    for i, spec in enumerate(case.specs):
        d = wc.dyadic_dout("%s/dout/%d" % (key, i), (case.b, case.n, spec[1], spec[2]))
        g, a = wm.gather_sum_adjoint(d, idx, spec, case.n, case.ldy)
        douts.append(d)
        dY, bound = dY + g, bound + a
    wm.assert_exact(dY, 0.25, bound)
    covered, once = wm.covered_columns(case.specs, case.ldy)
    assert once, case.name
    out = dict(idx=idx, dY=dY, covered=covered, maxima=wm.row_maxima(dY[:, :, covered]), worst=float(bound.max()) / 0.25)
    out["rowptr"], out["records"] = wm.transpose(idx)
    for v in list(out.values()) + douts:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    out["douts"] = tuple(douts)
    return out


def empty_taps(spec):
    """The taps whose window holds neither slot 8 nor slot 9."""
    T, P = spec[0], spec[1]
    return [t for t in range(T) if not any(0 <= s - t < P for s in (8, 9))]


def check_table(xcd=1, cw=None):
    for c in CASES:
        want = c.wants if xcd else ("csr_small",) * len(c.specs)
        assert tuple(wm.regime("csr", c.b, c.n, c.k, c.ldy, s, xcd=xcd, cw=cw) for s in c.specs) == want, c
    assert len({c.name for c in CASES}) == len(CASES)
