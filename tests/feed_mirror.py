"""Host mirror of the batch feeder (csrc/feed.hip, pdgn_amd.data.BatchFeeder): the same pure function of
(seed, epoch, iteration, global row) in numpy.  Test infrastructure: the product never imports it.

Counter layout (include/pdgn_hip.h, pdgn_feed_batch): key = (seed lo, seed hi); counter = (group j, global row,
t lo, tag | t hi24 << 8); tags 0 1 2 = index streams of p1 p2 p3, 3 4 = z1 z2, 5 = the epoch permutation
(counter (group, epoch lo, epoch hi, 5))."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
TAG_Z1, TAG_Z2, TAG_ORDER = 3, 4, 5
NOISE_DIM = 128


def philox4x32_10(counter, key):
    """counter: four broadcastable arrays of 32-bit words, key: two -> (..., 4) uint32 (Salmon et al., SC'11)."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def _key(seed):
    return (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def stream_words(seed, t, rows, tag, n):
    """The first n words of stream `tag` for each global row of `rows` at global iteration t -> (len(rows), n) uint32."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    groups = np.arange((n + 3) // 4, dtype=np.uint64).reshape(1, -1)
    c3 = tag | (((t >> 32) & 0xFFFFFF) << 8)
    w = philox4x32_10((groups, rows, t & 0xFFFFFFFF, c3), _key(seed))
    return w.reshape(rows.shape[0], -1)[:, :n]


def indices_from_words(w, N):
    """(w * N) >> 32."""
    return ((w.astype(np.uint64) * np.uint64(N)) >> S32).astype(np.int64)


def normals_from_words(w, sigma, dtype=np.float64):
    """Box-Muller on word pairs (0,1), (2,3), ...: columns (2i, 2i+1) = sigma * sqrt(-2 ln u1) * (cos, sin)(2 pi u2),
    evaluated in `dtype` (fp64: the reference of the tests; fp32: the formula as the kernel spells it)."""
    f = dtype
    u1 = ((w[..., 0::2] >> np.uint32(8)).astype(f) + f(1)) * f(2.0 ** -24)
    u2 = (w[..., 1::2] >> np.uint32(8)).astype(f) * f(2.0 ** -24)
    rad = np.sqrt(f(-2) * np.log(u1))
    ang = (f(np.float32(6.2831855)) if f is np.float32 else f(2 * np.pi)) * u2
    out = np.empty(w.shape, dtype=f)
    out[..., 0::2] = f(sigma) * (rad * np.cos(ang))
    out[..., 1::2] = f(sigma) * (rad * np.sin(ang))
    return out


def epoch_order(seed, epoch, S):
    """Stable argsort of S Philox words keyed by (seed, epoch)."""
    groups = np.arange((S + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((groups, epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF, TAG_ORDER), _key(seed)).reshape(-1)[:S]
    return np.argsort(w, kind="stable").astype(np.int32)


def batches_per_epoch(S, B, world=1):
    return S // (B * world)


class MirrorFeeder:
    """pdgn_amd.data.BatchFeeder on the host: `batch` returns numpy arrays, `fill` writes them into torch tensors."""

    def __init__(self, clouds, batch_size, sizes, seed, rank=0, world=1, sigma=0.2):
        self.clouds = np.ascontiguousarray(np.asarray(clouds, dtype=np.float32))
        self.S, self.N, _ = self.clouds.shape
        self.B, self.sizes, self.seed, self.rank, self.world, self.sigma = batch_size, tuple(sizes)[:3], seed, rank, world, sigma
        self.batches_per_epoch = batches_per_epoch(self.S, batch_size, world)

    def schedule(self, epoch, i):
        """(cloud ids (B), global rows (B), global iteration t) of batch i of `epoch` on this rank."""
        first = (i * self.world + self.rank) * self.B
        ids = epoch_order(self.seed, epoch, self.S)[first:first + self.B]
        rows = self.rank * self.B + np.arange(self.B)
        return ids, rows, (epoch - 1) * self.batches_per_epoch + i

    def draws(self, epoch, i):
        """(cloud ids, [index arrays (B, r_k)], z1 words, z2 words)."""
        ids, rows, t = self.schedule(epoch, i)
        idx = [indices_from_words(stream_words(self.seed, t, rows, k, r), self.N) for k, r in enumerate(self.sizes)]
        return ids, idx, stream_words(self.seed, t, rows, TAG_Z1, NOISE_DIM), stream_words(self.seed, t, rows, TAG_Z2, NOISE_DIM)

    def batch(self, epoch, i, dtype=np.float32):
        """([p1, p2, p3, p4] as (B,3,r) fp32, z1, z2 in `dtype`)."""
        ids, idx, w1, w2 = self.draws(epoch, i)
        pcs = self.clouds[ids]
        reals = [np.ascontiguousarray(np.take_along_axis(pcs, ix[:, :, None], axis=1).transpose(0, 2, 1)) for ix in idx]
        reals.append(np.ascontiguousarray(pcs.transpose(0, 2, 1)))
        return reals, normals_from_words(w1, self.sigma, dtype), normals_from_words(w2, self.sigma, dtype)

    def fill(self, epoch, i, reals, z1, z2):
        import torch
        r, a, b = self.batch(epoch, i)
        for d, s in zip(reals, r):
            d.copy_(torch.from_numpy(s))
        z1.copy_(torch.from_numpy(a))
        z2.copy_(torch.from_numpy(b))
