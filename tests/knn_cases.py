"""Inputs of the feature-kNN tests (tests/test_knn_cases_host.py, tests/test_gpu_feature_knn.py) whose graph is a matter of integers,
the host model that says which branch of csrc/feat_knn.hip / csrc/wave_select.h a case reaches, and the judge of float rows.

Exact cases.  Features are integer-valued fp32 with |v| <= vmax and 4 f vmax^2 <= 2^24: every partial sum of the Gram product and of
|x|^2 is an integer below 2^24 in any summation order, and so is the key (-2 <x_i, x_j> + |x_i|^2) + |x_j|^2 = |x_i - x_j|^2.  The key
is therefore exact whatever the matrix cores do internally, and the expected graph is an int64 Gram, a stable argsort per row and
ranks 1..k.  `guard` asserts all of that on a case before anything is compared.

Regime model.  `regimes` is a host model of the FILTER only, not of the arithmetic (the keys are exact): per query and 512-candidate
chunk the lane minima, the threshold (exact K-th for the general kernel, the 16-bit upper bound for the producer / consumer kernel,
the running list's K-th only after a merge), the survivors per 64-candidate step against the queue capacity, and the entry count at
the final threshold; plus the Gram-loop choice per strip and the tile-to-workgroup arithmetic of fk_persistent_grid on 256 CUs.  Every
case names the counts it exists for (`expect`); the host test asserts them, so a case cannot drift off its branch when a capacity is
retuned."""
import functools

import numpy as np

KEY_MAX = 1 << 24
# the constants of csrc/feat_knn.hip and csrc/wave_select.h the model mirrors
FK_QB, FK_NC, FK_WAVES = 32, 512, 4
WSEL_PQCAP = 128                    # general kernel: queue entries per query; merged when more than WSEL_PQCAP - 64 are queued
FKP_QCAP = 64                       # producer / consumer kernel: a step that would not fit merges first
FKP_QPW = 4                         # queries per consumer wave
SELECT_MAX = 32                     # knn_flush_select_multi: more entries at the threshold take the ranked merge
CUS = 256

KINDS = ("wide", "narrow", "clusters", "mixed")


def vmax_of(f):
    """Largest v with 4 f v^2 < 2^24, at most 255."""
    v = int(np.sqrt(KEY_MAX / (4.0 * f)))
    while 4 * f * v * v >= KEY_MAX:
        v -= 1
    return min(v, 255)


class Case:
    def __init__(self, B, f, n, k, kind, why, expect, cluster=100):
        self.B, self.f, self.n, self.k, self.kind, self.why, self.expect, self.cluster = B, f, n, k, kind, why, expect, cluster

    @property
    def id(self):
        return "%dx%dx%d-k%d-%s" % (self.B, self.f, self.n, self.k, self.kind)

    def __repr__(self):
        return "Case(%s)" % self.id


def make_input(B, f, n, kind, cluster=100):
    """(B, f, n) float32 with integer values, fixed seed per (shape, kind)."""
    rng = np.random.default_rng([B, f, n, KINDS.index(kind)])
    vmax = vmax_of(f)
    if kind == "wide":
        x = rng.integers(-vmax, vmax + 1, (B, f, n))
    elif kind == "narrow":
        x = rng.integers(-3, 4, (B, f, n))
    elif kind == "clusters":                                   # blocks of identical points; odd samples in reverse index order
        x = np.broadcast_to(3 * (np.arange(n) // cluster), (B, f, n)).copy()
        x[1::2] = x[1::2, :, ::-1]
    elif kind == "mixed":                                      # every fourth point copies one of three vectors, the rest are wide
        x = rng.integers(-vmax, vmax + 1, (B, f, n))
        proto = rng.integers(-vmax, vmax + 1, (B, f, 3))
        i = np.arange(0, n, 4)
        x[:, :, i] = proto[:, :, (i // 4) % 3]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x.astype(np.float32))


def int_keys(x):
    """int64 keys (n, n) of ONE sample x (f, n) of integer-valued features."""
    xi = x.astype(np.int64)
    sq = (xi * xi).sum(0)
    return (-2 * (xi.T @ xi) + sq[:, None]) + sq[None, :], sq


def int_graph(x, k, keys=None):
    """Ranks 1..k of the stable (key, index) order of every row: (B, n, k) int32, and the integer norms (B, n) int64."""
    idx, sqs = [], []
    for b in range(x.shape[0]):
        key, sq = int_keys(x[b]) if keys is None else keys[b]
        idx.append(np.argsort(key, axis=1, kind="stable")[:, 1:k + 1])
        sqs.append(sq)
    return np.stack(idx).astype(np.int32), np.stack(sqs)


def guard(x, keys=None):
    """The premise of an exact case: integer features, 4 f vmax^2 <= 2^24, and every key in [0, 2^24]."""
    assert x.dtype == np.float32 and np.isfinite(x).all() and (x == np.rint(x)).all(), "features are not integers"
    assert 4 * x.shape[1] * int(np.abs(x).max()) ** 2 <= KEY_MAX, "4 f vmax^2 > 2^24"
    for b in range(x.shape[0]):
        key, sq = int_keys(x[b]) if keys is None else keys[b]
        assert key.min() >= 0 and key.max() <= KEY_MAX and sq.max() <= KEY_MAX, (b, int(key.min()), int(key.max()))


@functools.lru_cache(maxsize=None)
def _prepared(case_id):
    """Input, keys, expected graph and norms of a case: computed once per process and shared, never modified."""
    c = BY_ID[case_id]
    x = make_input(c.B, c.f, c.n, c.kind, c.cluster)
    keys = [int_keys(x[b]) for b in range(c.B)]
    idx, sq = int_graph(x, c.k, keys)
    for a in (x, idx, sq):
        a.setflags(write=False)
    return x, keys, idx, sq


def prepared(case):
    return _prepared(case.id)


# ------------------------------------------------------------------------------------------------------------- non-finite inputs
def poison(x):
    """A copy of x with three poisoned points per sample (a NaN, a +inf and a -inf in one channel each), and their indices (B, 3)."""
    B, f, n = x.shape
    rng = np.random.default_rng([B, f, n, 99])
    y = x.copy()
    at = np.stack([rng.choice(n, 3, replace=False) for _ in range(B)])
    for b in range(B):
        for p, v in zip(at[b], (np.nan, np.inf, -np.inf)):
            y[b, rng.integers(f), p] = v
    return y, at


def int_graph_finite(x, k):
    """The integer graph over the FINITE points only, mapped back to the original indices (what the reference's sort gives: a
    poisoned point's key is NaN or +inf for every finite query); rows of poisoned queries are -1.  Also the finite mask (B, n)."""
    B, f, n = x.shape
    fin = np.isfinite(x).all(1)
    out = np.full((B, n, k), -1, np.int32)
    for b in range(B):
        keep = np.nonzero(fin[b])[0]
        sub, _ = int_graph(x[b:b + 1][:, :, keep], k)
        out[b, keep] = keep[sub[0]]
    return out, fin


# ------------------------------------------------------------------------------------------------------------------ regime model
def dispatch(f, n, k):
    """(kernel, FH) pdgn_feature_knn launches."""
    if n < k + 1:
        return "small", 0
    fh = (f + 1) // 2
    FH = 16 if fh <= 16 else 32 if fh <= 32 else 64 if fh <= 64 else 128
    return ("pc" if f == 2 * FH and n % 128 == 0 else "general"), FH


def _key32(d):
    """The order-preserving integer image of fp32 values the kernels bisect on."""
    b = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))


def _unkey32(key):
    key = key.astype(np.uint32)
    return np.where(key & np.uint32(0x80000000) != 0, key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(np.float32)


def kth_ub16(vals, K):
    """16-bit upper bound of the K-th smallest of every row of `vals` (wave_topk_append_multi), never past +inf."""
    key = np.sort(_key32(vals), axis=1)[:, K - 1]
    return _unkey32(np.minimum(key | np.uint32(0xffff), np.uint32(0xff800000)))


class _Rows:
    """Survivor queues and running lists (distances only) of all queries of one sample."""

    def __init__(self, rows, K, width):
        self.K = K
        self.cnt = np.zeros(rows, np.int64)
        self.queue = np.full((rows, width), np.inf, np.float32)
        self.listd = np.full((rows, K), np.inf, np.float32)
        self.merges = np.zeros(rows, np.int64)

    def merge(self, m):
        self.listd[m] = np.sort(np.concatenate([self.listd[m], self.queue[m]], 1), 1)[:, :self.K]
        self.queue[m] = np.inf
        self.cnt[m] = 0
        self.merges[m] += 1

    def append(self, d, keep):
        pos = self.cnt[:, None] + np.cumsum(keep, 1) - 1
        r = np.broadcast_to(np.arange(d.shape[0])[:, None], d.shape)
        self.queue[r[keep], pos[keep]] = d[keep]
        self.cnt += keep.sum(1)


def _chunks(D, n):
    for t0 in range(0, n, FK_NC):
        tn = min(FK_NC, n - t0)
        steps = (tn + 63) // 64
        C = np.full((D.shape[0], steps * 64), np.inf, np.float32)
        C[:, :tn] = D[:, t0:t0 + tn]
        yield C.reshape(D.shape[0], steps, 64)


def _filter_general(D, K):
    """wave_topk_append per chunk, knn_flush when a step starts with more than WSEL_PQCAP - 64 queued: in-scan merges per row."""
    st = _Rows(D.shape[0], K, WSEL_PQCAP)
    for C in _chunks(D, D.shape[1]):
        tau = np.minimum(np.sort(C.min(1), 1)[:, K - 1], st.listd[:, K - 1])
        for s in range(C.shape[1]):
            m = st.cnt > WSEL_PQCAP - 64
            if m.any():
                st.merge(m)
                tau = np.minimum(tau, st.listd[:, K - 1])
            d = C[:, s]
            st.append(d, (d <= tau[:, None]) & (d < np.inf))
            assert st.cnt.max() <= WSEL_PQCAP
    return st.merges


def _filter_pc(D, K):
    """wave_topk_append_multi per chunk with knn_flush_ranked on overflow, then the entry count of knn_flush_select_multi at its
    16-bit threshold: in-scan merges per row, slow final merges per row, the largest number of entries a final merge sees."""
    st = _Rows(D.shape[0], K, FKP_QCAP + 64)
    fmax = np.float32(3.402823466e38)
    for C in _chunks(D, D.shape[1]):
        tau = np.minimum(np.minimum(kth_ub16(C.min(1), K), st.listd[:, K - 1]), fmax)
        for s in range(C.shape[1]):
            d = C[:, s]
            keep = d <= tau[:, None]
            m = st.cnt + keep.sum(1) > FKP_QCAP
            if m.any():
                st.merge(m)
                tau = np.minimum(tau, st.listd[:, K - 1])
                keep &= d <= tau[:, None]
            st.append(d, keep)
            assert st.cnt.max() <= FKP_QCAP
    entries = np.concatenate([st.queue[:, :FKP_QCAP], st.listd], 1)
    total = int((st.cnt + np.isfinite(st.listd).sum(1)).max())
    key = _key32(entries)
    ub = (np.sort(key, 1)[:, K - 1] & np.uint32(0xffff0000)) | np.uint32(0xffff)
    at_threshold = ((key <= ub[:, None]) & (entries < np.inf)).sum(1)
    return st.merges, at_threshold > SELECT_MAX, total


def _gram_general(f, n, FH):
    """Which Gram loop every live 128-candidate strip of the general kernel takes, and how its lanes load."""
    vec_ok = n % 4 == 0
    out = dict(fast_strips=0, guarded_strips=0, vector_lanes=0, scalar_lanes=0, min_strip=FK_NC)
    for t0 in range(0, n, FK_NC):
        tn = min(FK_NC, n - t0)
        for wave in range(FK_WAVES):
            strip = 128 * wave
            if strip >= tn:
                continue
            out["min_strip"] = min(out["min_strip"], min(128, tn - strip))
            if vec_ok and t0 + strip + 128 <= n and 2 * FH == f:
                out["fast_strips"] += 1
                continue
            out["guarded_strips"] += 1
            for a4 in range(0, 128, 4):                       # the lane's four candidates
                cand = t0 + strip + a4
                if vec_ok and cand + 3 < n:
                    out["vector_lanes"] += 1
                elif cand < n:
                    out["scalar_lanes"] += 1
    return out


def persistent_map(B, n):
    """fk_persistent_grid and the kernel's tile walk: per workgroup the list of (sample, tile) it owns."""
    tiles = n // FK_QB
    wpx = min(CUS // 8, ((B + 7) // 8) * tiles)
    owned = []
    for pid in range(8 * wpx):
        xcd, slot = pid & 7, pid >> 3
        ns = (B - xcd + 7) // 8
        T = ns * tiles if ns > 0 else 0
        owned.append([(xcd + 8 * (j // tiles), j % tiles) for j in range(slot, T, wpx)])
    return owned


def regimes(case):
    """Counts of the branches the case reaches (see the module docstring)."""
    B, f, n, k = case.B, case.f, case.n, case.k
    kernel, FH = dispatch(f, n, k)
    K = k + 1
    _, keys, _, _ = prepared(case)
    out = dict(kernel=kernel, FH=FH, K=K, rows=B * n, chunks=(n + FK_NC - 1) // FK_NC, tail_chunk=n - FK_NC * ((n - 1) // FK_NC),
               pad_channels=2 * FH - f, odd_f=f % 2, n_mod_4=n % 4)
    merges, slow, mixed, total = [], [], 0, 0
    for b in range(B):
        D = keys[b][0].astype(np.float32)                     # exact: integers up to 2^24
        if kernel == "general":
            merges.append(_filter_general(D, K))
        else:
            mg, sl, tot = _filter_pc(D, K)
            merges.append(mg)
            slow.append(sl)
            q = sl.reshape(-1, FKP_QPW).sum(1)
            mixed += int(((q > 0) & (q < FKP_QPW)).sum())
            total = max(total, tot)
    merges = np.concatenate(merges)
    out.update(inscan_merges=int(merges.sum()), rows_inscan=int((merges > 0).sum()))
    if kernel == "general":
        out.update(_gram_general(f, n, FH))
        out["last_wg_queries"] = n - FK_QB * ((n - 1) // FK_QB)
    else:
        owned = persistent_map(B, n)
        per = [len(w) for w in owned]
        out.update(slow_final=int(np.concatenate(slow).sum()), quartets_mixed=mixed, final_entries_max=total,
                   idle_producer_waves=FK_WAVES - (out["tail_chunk"] + 127) // 128, workgroups=len(owned),
                   tiles_per_wg_max=max(per), tiles_per_wg_min=min(p for p in per if p), idle_wgs=sum(p == 0 for p in per),
                   wgs_spanning_samples=sum(len({s for s, _ in w}) > 1 for w in owned),
                   xcds_without_sample=max(0, 8 - B))
        assert sorted(t for w in owned for t in w) == [(s, t) for s in range(B) for t in range(n // FK_QB)]
    return out


def check_expect(case, counts):
    """The regimes a case exists for, as (count, op, value) with value a number or the name of another count."""
    ops = {"==": lambda a, b: a == b, ">=": lambda a, b: a >= b, "<=": lambda a, b: a <= b, ">": lambda a, b: a > b}
    for name, op, value in case.expect:
        want = counts[value] if isinstance(value, str) and value in counts else value
        assert ops[op](counts[name], want), "%s: %s = %r, expected %s %r" % (case.id, name, counts[name], op, want)


G, P = ("kernel", "==", "general"), ("kernel", "==", "pc")
CASES = [
    # ------------------------------------------------------------------------------------------------------------ general kernel
    Case(2, 5, 11, 10, "wide", "n = k+1, f odd, scalar loads",
         [G, ("K", "==", 11), ("rows", "==", 22), ("odd_f", "==", 1), ("vector_lanes", "==", 0), ("scalar_lanes", ">", 0)]),
    Case(2, 33, 130, 10, "narrow", "f odd with a zero-padded channel pair; n % 4 == 2; a strip of 2 candidates",
         [G, ("FH", "==", 32), ("pad_channels", "==", 31), ("odd_f", "==", 1), ("n_mod_4", "==", 2), ("min_strip", "==", 2),
          ("vector_lanes", "==", 0)]),
    Case(1, 3, 257, 4, "narrow", "FH = 16 with f = 3; n odd",
         [G, ("FH", "==", 16), ("n_mod_4", "==", 1), ("fast_strips", "==", 0)]),
    Case(3, 32, 516, 10, "wide", "fast loop on chunk 0; tail chunk of 4 candidates; last workgroup with 4 queries",
         [G, ("FH", "==", 16), ("fast_strips", "==", 4), ("guarded_strips", "==", 1), ("tail_chunk", "==", 4),
          ("last_wg_queries", "==", 4), ("scalar_lanes", "==", 0)]),
    Case(2, 64, 1000, 16, "narrow", "fast strips plus a partial strip, on vector loads",
         [G, ("fast_strips", "==", 7), ("guarded_strips", "==", 1), ("min_strip", "==", 104), ("vector_lanes", "==", 26),
          ("scalar_lanes", "==", 0)]),
    Case(1, 62, 1000, 10, "wide", "f != 2*FH: guarded loop, vector loads",
         [G, ("FH", "==", 32), ("pad_channels", "==", 2), ("fast_strips", "==", 0), ("guarded_strips", "==", 8),
          ("scalar_lanes", "==", 0)]),
    Case(2, 256, 513, 31, "wide", "FH = 128; K = 32; tail chunk of one candidate",
         [G, ("FH", "==", 128), ("K", "==", 32), ("tail_chunk", "==", 1), ("min_strip", "==", 1), ("vector_lanes", "==", 0)]),
    Case(1, 40, 1500, 31, "wide", "three chunks of >= 32 survivors: in-scan knn_flush",
         [G, ("K", "==", 32), ("chunks", "==", 3), ("rows_inscan", "==", "rows"), ("scalar_lanes", "==", 0)]),
    Case(1, 6, 700, 10, "clusters", "queue overflow by ties inside a chunk",
         [G, ("rows_inscan", "==", "rows"), ("chunks", "==", 2)], cluster=150),
    # --------------------------------------------------------------------------------------------- producer / consumer kernel
    Case(1, 32, 128, 10, "narrow", "one 128-candidate chunk; three producer waves idle; seven XCDs without a sample",
         [P, ("chunks", "==", 1), ("tail_chunk", "==", 128), ("idle_producer_waves", "==", 3), ("xcds_without_sample", "==", 7),
          ("idle_wgs", "==", 28)]),
    Case(9, 32, 128, 10, "wide", "XCD 0 owns samples 0 and 8; the other XCDs have 4 tiles for 8 workgroups",
         [P, ("workgroups", "==", 64), ("idle_wgs", "==", 28), ("tiles_per_wg_max", "==", 1)]),
    Case(17, 32, 640, 10, "wide", "XCD 0 has 60 tiles on 32 workgroups, the second tile of a workgroup belongs to another sample; "
         "tail chunk of 128; per-tile state reset",
         [P, ("workgroups", "==", 256), ("tiles_per_wg_max", "==", 2), ("tiles_per_wg_min", "==", 1), ("wgs_spanning_samples", ">=", 28),
          ("chunks", "==", 2), ("tail_chunk", "==", 128), ("idle_producer_waves", "==", 3), ("idle_wgs", "==", 0)]),
    Case(9, 32, 1024, 10, "narrow", "XCD 0 has 2 tiles per workgroup, the others 1; two chunks",
         [P, ("tiles_per_wg_max", "==", 2), ("tiles_per_wg_min", "==", 1), ("chunks", "==", 2), ("wgs_spanning_samples", "==", 32)]),
    Case(2, 64, 512, 10, "mixed", "slow and fast final merges in one quartet",
         [P, ("quartets_mixed", ">=", 250), ("slow_final", ">=", 256), ("rows_inscan", "==", 0)]),
    Case(2, 128, 640, 31, "wide", "K = 32; in-scan merge on every row; slow final merge on a large part of the rows",
         [P, ("K", "==", 32), ("rows_inscan", "==", "rows"), ("slow_final", ">=", 128), ("quartets_mixed", ">=", 32)]),
    Case(2, 256, 1024, 10, "wide", "FH = 128 (ring depth 8); vmax 127",
         [P, ("FH", "==", 128), ("chunks", "==", 2)]),
    Case(2, 32, 1024, 10, "clusters", "the mass-ties input, every row compared",
         [P, ("rows_inscan", ">=", 2000), ("slow_final", ">=", 1000)]),
    Case(1, 32, 4096, 10, "wide", "the 4096-point level: 8 chunks; in-scan ranked merge on every row without ties; 4 tiles per workgroup",
         [P, ("chunks", "==", 8), ("rows_inscan", "==", "rows"), ("tiles_per_wg_max", "==", 4), ("tiles_per_wg_min", "==", 4),
          ("idle_wgs", "==", 224)]),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ------------------------------------------------------------------------------------------------------------ judge of float rows
def row_bound(x64):
    """E_ij = (f + 4) 2^-24 (|x_i| + |x_j|)^2 of one sample (f, n): the worst case of the fp32 key against the fp64 one.  The dot
    product's f rounded partial sums err by at most f u |x_i||x_j| (u = 2^-24), doubled by the factor -2; either norm by f u |x|^2 / 2
    more than once over; the two additions round results of at most (|x_i| + |x_j|)^2 -- together below (f + 4) u (|x_i| + |x_j|)^2."""
    nrm = np.sqrt((x64 * x64).sum(0))
    return (x64.shape[0] + 4) * 2.0 ** -24 * (nrm[:, None] + nrm[None, :]) ** 2


def judge_rows(x, idx, k):
    """Every row of a float graph against fp64 distances D and the bound E = row_bound: a row passes if its k indices are in range
    and distinct, consecutive returned distances do not decrease by more than the sum of their bounds, and no unreturned point is
    nearer than the last returned one by more than the sum of their bounds -- except at most one point that is also that clearly
    before the FIRST returned one (the dropped rank 0).  Returns ok (B, n) and the largest fraction of a bound a passing row used."""
    B, f, n = x.shape
    idx = np.asarray(idx).astype(np.int64)
    ok = np.zeros((B, n), bool)
    used = 0.0
    tiny = np.finfo(np.float64).tiny
    for b in range(B):
        x64 = x[b].astype(np.float64)
        sq = (x64 * x64).sum(0)
        D = (-2.0 * (x64.T @ x64) + sq[:, None]) + sq[None, :]
        E = row_bound(x64)
        inr = ((idx[b] >= 0) & (idx[b] < n)).all(1)
        r = np.where(inr[:, None], idx[b], 0)
        s = np.sort(r, 1)
        distinct = (s[:, 1:] != s[:, :-1]).all(1)
        Dr, Er = np.take_along_axis(D, r, 1), np.take_along_axis(E, r, 1)
        drop, both = Dr[:, :-1] - Dr[:, 1:], np.maximum(Er[:, :-1] + Er[:, 1:], tiny)
        ordered = (drop <= both).all(1)
        unret = np.ones((n, n), bool)
        np.put_along_axis(unret, r, False, 1)
        gap_last, bnd_last = Dr[:, -1:] - D, np.maximum(E + Er[:, -1:], tiny)
        nearer = unret & (gap_last > bnd_last)
        rank0 = nearer & (Dr[:, :1] - D > E + Er[:, :1])
        nn = nearer.sum(1)
        complete = (nn == 0) | ((nn == 1) & (rank0.sum(1) == 1))
        ok[b] = inr & distinct & ordered & complete
        frac = np.maximum((drop / both).max(1, initial=0.0), np.where(unret & ~rank0, gap_last / bnd_last, 0.0).max(1))
        if ok[b].any():
            used = max(used, float(frac[ok[b]].max()))
    return ok, used


def gaussian(B, f, n):
    """Zero-mean Gaussian float input of the judged cases, as test_feature_knn draws it."""
    return np.random.default_rng(f + n).standard_normal((B, f, n)).astype(np.float32)


FLOAT_SHAPES = [(2, 6, 24, 5), (3, 32, 128, 10), (2, 64, 256, 10), (2, 128, 512, 10), (2, 256, 1024, 10), (1, 256, 2048, 10),
                (2, 7, 100, 4), (1, 40, 1500, 16), (2, 32, 516, 10), (1, 62, 1000, 10)]
NONFINITE_SHAPES = [(2, 32, 256, 10), (2, 7, 100, 4)]


if __name__ == "__main__":                                      # the counts of every case, for whoever retunes a capacity
    for case in CASES:
        print(case.id, "--", case.why)
        print("   ", regimes(case))
