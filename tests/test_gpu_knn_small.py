"""GPU: pdgn_feature_knn on clouds of fewer points than ranks (n <= k: csrc/feat_knn.hip's small-cloud kernel), which is what the base
levels of a generator for very few points ask for (--num_point 16 starts from ONE point).  Integer-valued features, so that the key
(-2 <x_i,x_j> + |x_i|^2) + |x_j|^2 is exact in fp32 and the expected order, ties by index included, is a matter of integers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _expected(x, k):
    """x (B,F,N) integer-valued -> (B,N,k): the ascending order of the key with ties by index, rank 0 dropped, the slots no point is
    left for repeating rank 0."""
    B, F, N = x.shape
    xi = x.astype(np.int64)
    out = np.empty((B, N, k), dtype=np.int32)
    for b in range(B):
        sq = (xi[b] * xi[b]).sum(0)
        key = -2 * (xi[b].T @ xi[b]) + sq[:, None] + sq[None, :]
        for i in range(N):
            order = np.lexsort((np.arange(N), key[i]))
            ranks = list(order[1:k + 1])
            out[b, i] = ranks + [order[0]] * (k - len(ranks))
    return out


@pytest.mark.parametrize("B,F,N,k", [(2, 3, 1, 2), (2, 5, 2, 2), (3, 32, 4, 10), (2, 64, 8, 10), (1, 7, 10, 10), (2, 6, 31, 31), (1, 256, 3, 5)])
def test_small_clouds_get_every_other_point_then_themselves(B, F, N, k):
    from pdgn_amd.deconv import feature_knn
    rng = np.random.default_rng(100 * N + k)
    x = rng.integers(-3, 4, (B, F, N)).astype(np.float32)           # (few values: many exact ties, duplicates of a point included)
    idx = feature_knn(torch.from_numpy(x).cuda(), k)
    torch.cuda.synchronize()
    got = idx.cpu().numpy()
    assert got.shape == (B, N, k) and got.min() >= 0 and got.max() < N
    assert np.array_equal(got, _expected(x, k)), (B, F, N, k)
    for b in range(B):                                           # N - 1 distinct points lead, and the padding is one index
        for i in range(N):
            assert len(set(got[b, i, :N - 1].tolist())) == N - 1 and len(set(got[b, i, N - 1:].tolist())) == 1
