"""numpy restatement of csrc/repulsion.hip (include/pdgn_hip.h: pdgn_repulsion): the operation order of that
file's header block, looped over j and vectorised over i.  numpy's float32 ufuncs round every operation on its own, as the kernel's
__fsub_rn / __fmul_rn / __fadd_rn do, so the two agree bit for bit.  Used by tests/test_repulsion_host.py and
tests/test_gpu_repulsion.py; imports nothing of pdgn_amd."""
import numpy as np

F = np.float32
WAVE = 64


def constants(radius, b, n):
    """(inv_h2, coef) as the launch gets them: 1 / h^2 and -8 / (h^2 b n), each computed in fp64 and rounded once to fp32."""
    inv = 1.0 / (float(radius) * float(radius))
    return F(inv), F(-8.0 * inv / (float(b) * float(n)))


def cloud_pass(x, inv):
    """One cloud x (n, 3) fp32 -> (s (n), g (n, 3) before the coefficient, nn2 (n), ordered pairs inside the radius)."""
    x = np.ascontiguousarray(x, dtype=F)
    n = x.shape[0]
    idx = np.arange(n)
    s, g, nn2, inside = np.zeros(n, F), np.zeros((n, 3), F), np.full(n, np.inf, F), 0
    inv, one = F(inv), F(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            d = x - x[j]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            other = idx != j
            nn2 = np.where(other & (d2 < nn2), d2, nn2)
            t = one - d2 * inv
            on = other & ~(t <= 0)
            s = np.where(on, s + t * t, s)
            g = np.where(on[:, None], g + t[:, None] * d, g)
            inside += int(on.sum())
    return s, g, nn2, inside


def wave_sum(row):
    """P_c: 64 lane sums over i = lane, lane + 64, ... ascending, then the xor butterfly 32, 16, .., 1 (every lane ends equal)."""
    row = np.asarray(row, dtype=F)
    p = np.zeros(WAVE, F)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(0, row.shape[0], WAVE):
            part = row[k:k + WAVE]
            p[:part.shape[0]] = p[:part.shape[0]] + part
        lanes = np.arange(WAVE)
        off = WAVE // 2
        while off:
            p = p + p[lanes ^ off]
            off //= 2
    return p[0]


def reduce(s):
    """s (b, n) -> (loss, per_cloud (b)): the reduction launch."""
    b, n = s.shape
    totals = [wave_sum(s[c]) for c in range(b)]
    T = 0.0
    for p in totals:
        T = T + float(p)
    with np.errstate(invalid="ignore", over="ignore"):
        per_cloud = np.array([F(float(p) / float(n)) for p in totals], dtype=F)
        return F(T / (float(b) * float(n))), per_cloud


def repulsion(x, radius):
    """x (b, n, 3) -> {loss, per_cloud, grad, nn2, s, inside}: what pdgn_repulsion stores for inv_h2, coef = constants(radius, b, n);
    `inside` is the fraction of ordered pairs (i, j != i) that took the branch (0 at n = 1)."""
    x = np.ascontiguousarray(x, dtype=F)
    b, n, _ = x.shape
    inv, coef = constants(radius, b, n)
    s, grad, nn2 = np.empty((b, n), F), np.empty((b, n, 3), F), np.empty((b, n), F)
    inside = 0
    for c in range(b):
        s[c], g, nn2[c], k = cloud_pass(x[c], inv)
        with np.errstate(invalid="ignore", over="ignore"):
            grad[c] = coef * g
        inside += k
    loss, per_cloud = reduce(s)
    return {"loss": loss, "per_cloud": per_cloud, "grad": grad, "nn2": nn2, "s": s,
            "inside": inside / float(b * n * (n - 1)) if n > 1 else 0.0}


U = 2.0 ** -24                                                    # the unit roundoff of fp32


def restate64(x, radius):
    """The same function in fp64 torch ops with autograd (no operation order to speak of): {loss, grad (b,n,3), s (b,n), nn2 (b,n)} and the
    sums of the absolute values of each component's terms that the error bounds are made of: "grad_abs" (b,n,3) = |c| sum_j |t d_k|
    (s and the loss are sums of positive terms: their own values).  All numpy fp64."""
    import torch
    X = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    b, n, _ = X.shape
    d = X[:, :, None, :] - X[:, None, :, :]
    d2 = (d * d).sum(-1)
    off = ~torch.eye(n, dtype=torch.bool).expand(b, n, n)
    t = torch.where(off, (1.0 - d2 / (float(radius) * float(radius))).clamp_min(0.0), torch.zeros_like(d2))
    s = (t * t).sum(-1)
    loss = s.sum() / float(b * n)
    loss.backward()
    c = 8.0 / (float(radius) * float(radius) * b * n)
    grad_abs = c * (t.detach()[..., None] * d.detach().abs()).sum(2)
    nn2 = torch.where(off, d2.detach(), torch.full_like(d2, float("inf"))).min(-1)[0]
    return {"loss": float(loss.detach()), "grad": X.grad.numpy(), "s": s.detach().numpy(), "nn2": nn2.numpy(), "grad_abs": grad_abs.numpy()}


def bounds(ref, n):
    """The allowed fp32 errors against `restate64`, derived, per component: a thread adds at most n terms one after the other (n u of the
    sum of their absolute values, to first order) and every term carries a handful of roundings of its own -- the three differences, the
    five operations of d2, the two of t, the product, the coefficient: 8 u -- so (n + 8) u sum_j |term_j|.  The loss adds the reduction on
    top of the s_i: at most n / 64 + 6 more fp32 additions per value (a lane's strided sum, the butterfly) and two roundings to and from
    fp64: (n + n / 64 + 16) u loss, all terms being positive."""
    return {"grad": (n + 8) * U * ref["grad_abs"], "s": (n + 8) * U * ref["s"], "loss": (n + n / 64.0 + 16) * U * ref["loss"]}


def worst(err, bound):
    """The largest err / bound over the components whose bound is not zero (for a test's printed figure)."""
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def spacing_stats(clouds):
    """evaluation.spacing_stats in fp64 numpy from the mirror's nn2: {nn_mean, nn_cv, nn_min, duplicates}."""
    clouds = np.ascontiguousarray(clouds, dtype=F)
    nn2 = np.stack([cloud_pass(c, F(1.0))[2] for c in clouds]).astype(np.float64)
    d = np.sqrt(nn2)
    mean = d.mean(axis=1)
    return {"nn_mean": float(mean.mean()), "nn_cv": float((d.std(axis=1) / mean).mean()), "nn_min": float(d.min()),
            "duplicates": int((nn2 == 0).sum())}
