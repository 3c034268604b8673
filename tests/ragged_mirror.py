"""Host mirror of the ragged feeder (csrc/feed.hip: pdgn_feed_batch_ragged, pdgn_sample_ragged; pdgn_amd.data.RaggedFeeder,
pdgn_amd.clouds.CloudSet.sample): the same pure function of (seed, epoch, iteration, global row) in numpy, on top of tests/feed_mirror.py
and tests/resample_mirror.py.  Test infrastructure: the product never imports it.

The definition (include/pdgn_hip.h): row b takes shape c = order[first + b], lo = off[c], M_c = off[c+1] - lo;
p4[b,:,j] = points[lo + pi_c(j mod M_c)] with pi_c the resampling feeder's keyed Feistel permutation of [0, M_c) (round keys: stream 6 of the
row); pk[b,:,j] = points[lo + ((word * M_c) >> 32)] from the streams 0 1 2; the noise is the plain feeder's.  pdgn_sample_ragged: the round
keys are words of the counters (0 | 1, s, draw lo, 13 | draw hi24 << 8)."""
import numpy as np

import feed_mirror as fm
from resample_mirror import ROUNDS, permute, round_keys

TAG_RAGGED = 13


def perm_columns(M, keys, n):
    """pi(j mod M) for j < n and one key set (6 words) -> (n) int64 in [0, M)."""
    pi = permute(int(M), np.asarray(keys).reshape(1, ROUNDS), min(int(M), int(n)))[0]
    return pi[np.arange(int(n)) % int(M)]


def sample_keys(seed, draw, S):
    """(S, 6) uint32: the round keys of pdgn_sample_ragged for shapes 0 .. S-1 (the shape index sits where the global row does)."""
    return fm.stream_words(seed, draw, np.arange(S), TAG_RAGGED, 8)[:, :ROUNDS]


def clamp_order(order, S):
    return np.clip(np.asarray(order, dtype=np.int64), 0, S - 1)


def feed_batch_ragged(points, off, order, first, B, lens, seed, t, row0, sigma=0.2, dtype=np.float32):
    """pdgn_feed_batch_ragged -> ([p1, p2, p3, p4] as (B,3,len) fp32, z1, z2 in `dtype`).  points (T,3) fp32, off (S+1), lens = (r1, r2, r3, N)."""
    points, off = np.asarray(points, dtype=np.float32), np.asarray(off, dtype=np.int64)
    ids = clamp_order(order, off.shape[0] - 1)[first:first + B]
    rows = (int(row0) + np.arange(B)) & 0xFFFFFFFF
    keys = round_keys(seed, t, rows)
    out = [np.empty((B, 3, r), dtype=np.float32) for r in lens]
    for b, c in enumerate(ids.tolist()):
        lo, M = int(off[c]), int(off[c + 1] - off[c])
        for k in range(3):
            idx = fm.indices_from_words(fm.stream_words(seed, t, rows[b:b + 1], k, lens[k]), M)[0]
            out[k][b] = points[lo + idx].T
        out[3][b] = points[lo + perm_columns(M, keys[b], lens[3])].T
    z = [fm.normals_from_words(fm.stream_words(seed, t, rows, tag, fm.NOISE_DIM), sigma, dtype) for tag in (fm.TAG_Z1, fm.TAG_Z2)]
    return out, z[0], z[1]


def sample_ragged(points, off, n, seed, draw):
    """pdgn_sample_ragged -> (S, n, 3) fp32."""
    points, off = np.asarray(points, dtype=np.float32), np.asarray(off, dtype=np.int64)
    S = off.shape[0] - 1
    keys = sample_keys(seed, draw, S)
    out = np.empty((S, n, 3), dtype=np.float32)
    for s in range(S):
        lo, M = int(off[s]), int(off[s + 1] - off[s])
        out[s] = points[lo + perm_columns(M, keys[s], n)]
    return out


class MirrorRaggedFeeder:
    """pdgn_amd.data.RaggedFeeder on the host: `clouds` a list of (M_s,3) arrays (what the CloudSet holds, already normalised)."""

    def __init__(self, clouds, batch_size, sizes, seed, rank=0, world=1, sigma=0.2, num_point=2048):
        clouds = [np.asarray(c, dtype=np.float32) for c in clouds]
        self.points = np.concatenate(clouds, 0)
        self.off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)
        self.S, self.N = len(clouds), int(num_point)
        self.B, self.sizes, self.seed, self.rank, self.world, self.sigma = batch_size, tuple(sizes)[:3], seed, rank, world, sigma
        self.batches_per_epoch = fm.batches_per_epoch(self.S, batch_size, world)

    def schedule(self, epoch, i):
        """(shape ids (B), global rows (B), global iteration t) of batch i of `epoch` on this rank."""
        first = (i * self.world + self.rank) * self.B
        ids = fm.epoch_order(self.seed, epoch, self.S)[first:first + self.B]
        return ids, self.rank * self.B + np.arange(self.B), (epoch - 1) * self.batches_per_epoch + i

    def batch(self, epoch, i, dtype=np.float32):
        first = (i * self.world + self.rank) * self.B
        t = (epoch - 1) * self.batches_per_epoch + i
        return feed_batch_ragged(self.points, self.off, fm.epoch_order(self.seed, epoch, self.S), first, self.B, self.sizes + (self.N,),
                                 self.seed, t, self.rank * self.B, self.sigma, dtype)
