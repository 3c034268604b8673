"""The adaptive discriminator augmentation's rule (include/pdgn_hip.h: pdgn_ada_state, pdgn_augment_tick_ada)
restated on the host: integers as Python ints taken from / stored into numpy uint64 words (every intermediate is asserted to fit
the kernel's 64-bit arithmetic), r in numpy float64.  `tick` is the whole launch on the 40 state words, the 16 table words and the 16
slot words; `step_thr` the threshold's move alone; `counts` what pdgn_mse_const_count stores."""
import numpy as np

import augment_mirror as am  # noqa: F401  (the table's layout: words 0 .. 4 are the five thresholds)

WORDS, SLOT_WORDS, NETWORKS = 40, 16, 4
(TARGET, INTERVAL, SPAN, THR_MIN, THR_MAX, MASK, THR, POS, NEG, N, ITERS, UPDATES, LAST_R, LAST_POS, LAST_NEG, LAST_N, LAST_NET,
 NET) = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 28)
ONE = 1 << 24
U64 = 1 << 64


def fresh(p=0.5, target=0.6, interval=4, span=500_000, p_min=0.0, p_max=0.8, mask=0b01111):
    """A state record with empty accumulators, as a uint64 array."""
    w = np.zeros(WORDS, dtype=np.uint64)
    w.view(np.float64)[TARGET] = target
    w[INTERVAL], w[SPAN], w[MASK] = interval, span, mask
    w[THR_MIN], w[THR_MAX], w[THR] = int(round(p_min * ONE)), int(round(p_max * ONE)), int(round(p * ONE))
    return w


def counts(x, boundary=0.5):
    """(pos, neg, n) of fp32 scores: a score equal to the boundary and a NaN count to neither."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    b = np.float32(boundary)
    with np.errstate(invalid="ignore"):
        return int((x > b).sum()), int((x < b).sum()), int(x.size)


def slots_of(triples):
    """Four (pos, neg, n) -> the int32[16] slot tensor's contents (word 3 of every slot unused)."""
    s = np.zeros(SLOT_WORDS, dtype=np.int32)
    for i, t in enumerate(triples):
        s[4 * i:4 * i + 3] = t
    return s


def step_size(n, span):
    q = (n << 24) // (4 * span)
    assert (n << 24) < U64 and 4 * span < U64
    return max(1, q)


def step_thr(thr, pos, neg, n, target, span, thr_min, thr_max):
    """(thr after one update, r): r = (pos - neg) / n in float64, one integer step towards the target, clamped."""
    assert n > 0 and abs(pos - neg) < 1 << 53 and n < 1 << 53          # the operands of the division are exact
    r = np.float64(pos - neg) / np.float64(n)
    step = step_size(n, span)
    if r > np.float64(target):
        thr += step
    elif r < np.float64(target):
        thr -= step
    return min(max(thr, thr_min), thr_max), float(r)


def tick(state, table, slots, clock):
    """One pdgn_augment_tick_ada: -> (state, table, slots, clock) afterwards, fresh arrays; the inputs are left unchanged."""
    st, tab = np.array(state, dtype=np.uint64), np.array(table).view(np.uint32).copy()
    c = np.asarray(slots).view(np.uint32).astype(np.uint64)
    clock = (int(clock) + 1) % U64
    per = [int(c[4 * i + j]) for i in range(NETWORKS) for j in range(3)]
    P, G, n_it = sum(per[0::3]), sum(per[1::3]), sum(per[2::3])
    zero = np.zeros(SLOT_WORDS, dtype=np.int32)
    if n_it == 0:
        return st, tab, zero, clock
    pos, neg, n, iters = int(st[POS]) + P, int(st[NEG]) + G, int(st[N]) + n_it, int(st[ITERS]) + 1
    net = [int(st[NET + i]) + per[i] for i in range(12)]
    if iters < int(st[INTERVAL]):
        st[POS], st[NEG], st[N], st[ITERS] = pos, neg, n, iters
        st[NET:NET + 12] = net
        return st, tab, zero, clock
    thr, r = step_thr(int(st[THR]), pos, neg, n, st.view(np.float64)[TARGET], int(st[SPAN]), int(st[THR_MIN]), int(st[THR_MAX]))
    st[THR] = thr
    for k in range(5):
        if int(st[MASK]) >> k & 1:
            tab[k] = thr
    st.view(np.float64)[LAST_R] = r
    st[LAST_POS], st[LAST_NEG], st[LAST_N] = pos, neg, n
    st[LAST_NET:LAST_NET + 12] = net
    st[NET:NET + 12] = 0
    st[POS] = st[NEG] = st[N] = st[ITERS] = 0
    st[UPDATES] = int(st[UPDATES]) + 1
    return st, tab, zero, clock


def update(state, slots, table=None, clock=0):
    """`tick` for callers that hold the state alone: -> the state afterwards (a table of zeros and a clock of 0 stand in)."""
    return tick(state, np.zeros(16, dtype=np.uint32) if table is None else table, slots, clock)[0]
