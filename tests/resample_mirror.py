"""Host mirror of the resampling feeder (csrc/feed.hip: pdgn_feed_batch_resample; pdgn_amd.data.BatchFeeder with num_point / pool):
the same pure function of (seed, epoch, iteration, global row) in numpy, on top of tests/feed_mirror.py.  Test infrastructure: the
product never imports it.

The permutation (include/pdgn_hip.h, pdgn_feed_batch_resample): a balanced Feistel network of six rounds on 2h bits,
h = ceil(max(2, bit length of P - 1) / 2), round function F(r, k) = (((r ^ k) * 0x9E3779B1) mod 2^32) >> (32 - h), cycle-walked
into [0, P); the six round keys of a (row, t) are Philox words of the counters (0 | 1, global row, t lo, 6 | t hi24 << 8)."""
import numpy as np

import feed_mirror as fm

TAG_PERM = 6
ROUNDS = 6
GOLDEN = 0x9E3779B1


def half_bits(P):
    return (max(2, int(P - 1).bit_length()) + 1) // 2


def round_keys(seed, t, rows):
    """(len(rows), 6) uint32: words 0 1 2 3 of group 0 and words 0 1 of group 1 of stream 6."""
    return fm.stream_words(seed, t, rows, TAG_PERM, 8)[:, :ROUNDS]


def feistel_pass(x, h, keys):
    """One pass over [0, 2^(2h)); x (..., n) uint64, keys (..., 6) broadcast against it along the last axis."""
    x = np.asarray(x, dtype=np.uint64)
    hh, mask = np.uint64(h), np.uint64((1 << h) - 1)
    L, R = x >> hh, x & mask
    for i in range(ROUNDS):
        k = np.asarray(keys[..., i], dtype=np.uint64)[..., None]
        f = (((R ^ k) * np.uint64(GOLDEN)) & fm.MASK) >> np.uint64(32 - h)
        L, R = R, L ^ f
    return (L << hh) | R


def permute(P, keys, n=None):
    """pi(0 .. n-1) for every key set: keys (K, 6) -> (K, n) int64, every value in [0, P).  n defaults to P (the whole permutation)."""
    keys = np.asarray(keys).reshape(-1, ROUNDS)
    n = P if n is None else n
    h = half_bits(P)
    x = np.broadcast_to(np.arange(n, dtype=np.uint64), (keys.shape[0], n)).copy()
    todo = np.ones(x.shape, dtype=bool)
    passes = 0
    while todo.any():
        y = feistel_pass(x, h, keys)
        x = np.where(todo, y, x)
        todo &= x >= np.uint64(P)
        passes += 1
        assert passes <= 1 << (2 * h), "the walk left its cycle"
    return x.astype(np.int64)


class MirrorResampleFeeder(fm.MirrorFeeder):
    """pdgn_amd.data.BatchFeeder(clouds (S,M,3), ..., num_point=N, pool=P) on the host."""

    def __init__(self, clouds, batch_size, sizes, seed, rank=0, world=1, sigma=0.2, num_point=None, pool=None):
        super().__init__(clouds, batch_size, sizes, seed, rank, world, sigma)
        self.M = self.N
        self.N = self.M if num_point is None else int(num_point)
        self.P = self.M if pool is None else int(pool)
        assert 1 <= self.N <= self.P <= self.M

    def draws(self, epoch, i):
        """(cloud ids, [index arrays (B, r_k) of p1 p2 p3, (B, N) of p4], z1 words, z2 words)."""
        ids, rows, t = self.schedule(epoch, i)
        idx = [fm.indices_from_words(fm.stream_words(self.seed, t, rows, k, r), self.P) for k, r in enumerate(self.sizes)]
        idx.append(permute(self.P, round_keys(self.seed, t, rows), self.N))
        return ids, idx, fm.stream_words(self.seed, t, rows, fm.TAG_Z1, fm.NOISE_DIM), fm.stream_words(self.seed, t, rows, fm.TAG_Z2, fm.NOISE_DIM)

    def batch(self, epoch, i, dtype=np.float32):
        ids, idx, w1, w2 = self.draws(epoch, i)
        pcs = self.clouds[ids]
        reals = [np.ascontiguousarray(np.take_along_axis(pcs, ix[:, :, None], axis=1).transpose(0, 2, 1)) for ix in idx]
        return reals, fm.normals_from_words(w1, self.sigma, dtype), fm.normals_from_words(w2, self.sigma, dtype)
