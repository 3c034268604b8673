"""Host mirror of csrc/auction.hip (pdgn_auction_assign): the integer forward auction with epsilon scaling, in numpy.

The same quantisation in the same fp32 operation order, the same epsilon schedule, the same Jacobi rounds and the same two tie
rules, so that assignment, bid count and status equal the kernel's element for element:

  cmax   the diagonal of the bounding box of both clouds, fp32, every operation rounded on its own
  q      cmax * 2^-QUANTUM_BITS;  C_ij = rint(sqrt(dx*dx + dy*dy + dz*dz) / q);  S_ij = C_ij * (n + 1)
  eps    max(1, ((n + 1) << QUANTUM_BITS) / 4), then max(1, eps // 5) per phase, the last phase at eps = 1
  round  every unassigned bidder i takes the object with the smallest key (S_ij + price_j) << 11 | ((j - i) mod n) -- among equal
         values the first object at or after its own index -- and bids price_j1 + (w2 - w1) + eps, w2 the second smallest key's
         value; per object the highest bid wins, equal bids go to the lowest bidder; the loser and the displaced owner bid again
  caps   a phase runs at most max_rounds(n) rounds and a pair makes at most max_bids(n) bids; a bid of 2^PRICE_BITS or more
         counts as a cap; a capped pair keeps what it has assigned and the rest is completed in index order (status 1)
"""
import numpy as np

QUANTUM_BITS = 20
EPS_DIVISOR = 5
ROT_BITS = 11                     # (j - i) mod n < 2048
PRICE_BITS = 51                   # a bid at or above 2^51 would not fit the packed keys
MAX_N = 2048
F = np.float32


def phases(n):
    eps, count = max(1, ((n + 1) << QUANTUM_BITS) // 4), 1
    while eps > 1:
        eps, count = max(1, eps // EPS_DIVISOR), count + 1
    return count


def max_bids(n):
    return 64 * n * phases(n)


def max_rounds(n):
    return 16 * n + 64


def cmax_of(a, b):
    """fp32 diagonal of the joint bounding box; NaN when a coordinate is not finite."""
    pts = np.concatenate([a, b], axis=0).astype(F)
    if not np.isfinite(pts).all():
        return F(np.nan)
    with np.errstate(over="ignore", invalid="ignore"):
        e = (pts.max(axis=0) - pts.min(axis=0)).astype(F)
        s = F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2]))
        return F(np.sqrt(s))


def quantum_of(cmax):
    return F(cmax * F(2.0 ** -QUANTUM_BITS))


def degenerate(cmax):
    """The pairs decided before the loop: no finite positive quantum (all points equal, a non-finite coordinate or extent, an extent
    below 2^-106)."""
    return not (np.isfinite(cmax) and quantum_of(cmax) >= np.finfo(F).tiny)


def int_costs(a_rows, b, q):
    """C_ij for the bidders `a_rows` (k,3) against every object (n,3): int64 (k,n)."""
    d = a_rows[:, None, :].astype(F) - b[None, :, :].astype(F)
    s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F)
    s = (s + d[..., 2] * d[..., 2]).astype(F)
    return np.rint(np.sqrt(s).astype(F) / q).astype(np.int64)


def auction(a, b):
    """a, b (n,3) fp32 -> (assign (n,) int32: object of bidder i, bids, status, quantum)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    n = a.shape[0]
    assert 1 <= n <= MAX_N and b.shape == a.shape
    ident = np.arange(n, dtype=np.int32)
    cmax = cmax_of(a, b)
    if degenerate(cmax):
        return ident, 0, 2, F(0)
    q = quantum_of(cmax)
    if n == 1:
        return ident, 0, 0, q
    price = np.zeros(n, np.int64)
    assign = np.full(n, -1, np.int64)
    owner = np.full(n, -1, np.int64)
    eps = max(1, ((n + 1) << QUANTUM_BITS) // 4)
    bids, capped = 0, False
    jj = np.arange(n, dtype=np.int64)
    while True:
        assign[:] = -1
        owner[:] = -1
        free = np.arange(n, dtype=np.int64)
        rounds = 0
        while free.size:
            if rounds >= max_rounds(n) or bids + free.size > max_bids(n):
                capped = True
                break
            rounds += 1
            bids += free.size
            w = int_costs(a[free], b, q) * (n + 1) + price[None, :]
            key = (w << ROT_BITS) | ((jj[None, :] - free[:, None]) % n)
            order = np.argpartition(key, 1, axis=1)[:, :2]
            k0 = np.take_along_axis(key, order, axis=1)
            swap = k0[:, 0] > k0[:, 1]
            j1 = np.where(swap, order[:, 1], order[:, 0])
            w1 = np.minimum(k0[:, 0], k0[:, 1]) >> ROT_BITS
            w2 = np.maximum(k0[:, 0], k0[:, 1]) >> ROT_BITS
            bid = price[j1] + (w2 - w1) + eps
            if (bid >= (1 << PRICE_BITS)).any():                 # (the round's bids are counted; none of them is applied)
                capped = True
                break
            # per object: the highest bid, the lowest bidder among equals
            rank = np.lexsort((free, -bid, j1))
            first = np.ones(rank.size, bool)
            first[1:] = j1[rank][1:] != j1[rank][:-1]
            win = rank[first]
            lose = rank[~first]
            old = owner[j1[win]]
            assign[old[old >= 0]] = -1
            owner[j1[win]] = free[win]
            price[j1[win]] = bid[win]
            assign[free[win]] = j1[win]
            free = np.sort(np.concatenate([free[lose], old[old >= 0]]))
        if capped or eps == 1:
            break
        eps = max(1, eps // EPS_DIVISOR)
    status = 0
    if capped:
        status = 1
        taken = np.zeros(n, bool)
        taken[assign[assign >= 0]] = True
        assign[assign < 0] = np.flatnonzero(~taken)              # index order on both sides
    return assign.astype(np.int32), int(bids), status, q


def cost_of(a, b, assign):
    """fp64 cost of an assignment."""
    return float(np.sqrt(((a.astype(np.float64) - b.astype(np.float64)[assign]) ** 2).sum(axis=1)).sum())


def is_permutation(assign):
    return np.array_equal(np.sort(np.asarray(assign, np.int64)), np.arange(len(assign)))
