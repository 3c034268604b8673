"""Host mirror of the register-resident farthest-point kernel (csrc/fps.hip: pdgn_fps_order, pdgn_feed_fps_pyramid) and of
pdgn_amd.data.BatchFeeder(subsample="fps"), in numpy.  Test infrastructure: the product never imports it.

Arithmetic as the kernel spells it, fp32 throughout: d = fma(dz,dz, fma(dy,dy, dx*dx)) with the differences rounded to fp32; the
running minimum starts at 1e10 and is min(); a round takes the FIRST index of the largest minimum (np.argmax).  The fused
multiply-adds are evaluated in fp64 and rounded once to fp32: the product of two fp32 values is exact in fp64, and the sum is exact
there whenever it fits 53 bits -- always on lattice inputs (hashweights.lattice_points), where every distance is exact in fp32
anyway; on arbitrary inputs a double rounding can differ from the fused result in the last bit, so the tests compare the kernel with
this mirror on lattices only.

The start index of the feeder's pyramid: word 0 of the Philox counter (0, global row, t lo, TAG_FPS | t hi24 << 8) of
tests/feed_mirror.py's generator, reduced to [0, N) by (word * N) >> 32."""
import numpy as np

import feed_mirror as fm

TAG_FPS = 7                                                      # PDGN_FEED_TAG_FPS (include/pdgn_hip.h)
MAX_N = 8192                                                     # PDGN_FPS_MAX_N
F32 = np.float32


def sqdist3(points, q):
    """(n,3) fp32, (3,) fp32 -> (n,) fp32: csrc/common.h's sqdist3, each fma rounded once."""
    d = (points.astype(F32) - q.astype(F32)).astype(F32).astype(np.float64)
    acc = (d[:, 0] * d[:, 0]).astype(F32)
    acc = (d[:, 1] * d[:, 1] + acc.astype(np.float64)).astype(F32)
    return (d[:, 2] * d[:, 2] + acc.astype(np.float64)).astype(F32)


def fps_order(xyz, m, start=0):
    """One cloud (n,3) -> (m,) int64: order[0] = start, then m - 1 rounds."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    n = xyz.shape[0]
    assert 1 <= m <= n and 0 <= start < n
    mind = np.full(n, 1e10, dtype=F32)
    order = np.empty(m, dtype=np.int64)
    order[0] = start
    for j in range(1, m):
        mind = np.minimum(mind, sqdist3(xyz, xyz[order[j - 1]]))
        order[j] = int(np.argmax(mind))                          # the first index of the maximum
    return order


def fps_order_batch(xyz, m, start=None):
    """(b,n,3) -> (b,m) int32; start: None (0), an int or (b,) ints."""
    b = xyz.shape[0]
    start = np.zeros(b, dtype=np.int64) if start is None else np.broadcast_to(np.asarray(start, dtype=np.int64), (b,))
    return np.stack([fps_order(xyz[i], m, int(start[i])) for i in range(b)]).astype(np.int32) if b else np.zeros((0, m), np.int32)


def start_indices(seed, t, rows, N):
    """The pyramid's start index for each global row at global iteration t -> (len(rows),) int64."""
    return fm.indices_from_words(fm.stream_words(seed, t, rows, TAG_FPS, 1), N)[:, 0]


def pyramid(p4, sizes, seed, t, rows):
    """p4 (B,3,N) fp32, the three level sizes -> ([p1, p2, p3] as (B,3,r) fp32, order (B,r3) int64): pk[b,:,j] = p4[b,:,order[b,j]]."""
    p4 = np.asarray(p4, dtype=F32)
    B, _, N = p4.shape
    r1, r2, r3 = sizes
    assert 1 <= r1 <= r2 <= r3 <= N <= MAX_N
    starts = start_indices(seed, t, rows, N)
    order = np.stack([fps_order(p4[b].T, r3, int(starts[b])) for b in range(B)])
    full = np.take_along_axis(p4, order[:, None, :], axis=2)
    return [np.ascontiguousarray(full[:, :, :r]) for r in (r1, r2, r3)], order


class MirrorFpsFeeder:
    """BatchFeeder(subsample="fps") on the host: `base` is the mirror of the same feeder with subsample="random"
    (feed_mirror.MirrorFeeder or resample_mirror.MirrorResampleFeeder); p4, z1, z2 are its, p1..p3 the pyramid of its p4."""

    def __init__(self, base):
        self.base = base
        self.batches_per_epoch = base.batches_per_epoch

    def schedule(self, epoch, i):
        return self.base.schedule(epoch, i)

    def batch(self, epoch, i, dtype=np.float32):
        reals, z1, z2 = self.base.batch(epoch, i, dtype)
        _, rows, t = self.base.schedule(epoch, i)
        levels, _ = pyramid(reals[3], self.base.sizes, self.base.seed, t, rows)
        return levels + [reals[3]], z1, z2
