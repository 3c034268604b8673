"""Losses of the PDGN training step: Chamfer (utils/chamfer_loss.py:13-38) and the
shape-preserving local-statistics loss (models/PDGNet_v2.py:127-155), on fused HIP kernels
(csrc/localpair.hip): no (B,M,N) distance matrix, no (B,3,M,20) grouped tensor, no bmm."""

import torch
import torch.nn as nn
from ._fn import Function

from . import _lib, pointops
from ._lib import check, ptr, require, stream_of
from .fused import _zeros

F32, I32 = torch.float32, torch.int32


class ChamferGram(Function):
    """x (B,M,D), y (B,N,D) -> (min_j P[i,j] (B,M), min_i P[i,j] (B,N)) with the reference's
    Gram-form P = |x_i|^2 + |y_j|^2 - 2<x_i,y_j> (chamfer_loss.py:22-38)."""

    @staticmethod
    def forward(ctx, x, y):
        x, y = x.contiguous(), y.contiguous()
        require(x, "x", F32, 3)
        require(y, "y", F32, 3)
        b, m, d = x.shape
        n = y.shape[1]
        minx = torch.empty((b, m), dtype=F32, device=x.device)
        miny = torch.empty((b, n), dtype=F32, device=x.device)
        argx = torch.empty((b, m), dtype=I32, device=x.device)
        argy = torch.empty((b, n), dtype=I32, device=x.device)
        check(_lib.lib().pdgn_chamfer_gram(b, m, n, d, ptr(x), ptr(y), ptr(minx), ptr(argx), ptr(miny), ptr(argy),
                                           stream_of(x)), "pdgn_chamfer_gram")
        ctx.save_for_backward(x, y, argx, argy)
        ctx.mark_non_differentiable(argx, argy)
        return minx, miny

    @staticmethod
    def backward(ctx, gminx, gminy):
        x, y, argx, argy = ctx.saved_tensors
        b, m, d = x.shape
        n = y.shape[1]
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        gminx, gminy = gminx.contiguous(), gminy.contiguous()
        check(_lib.lib().pdgn_chamfer_gram_grad(b, m, n, d, ptr(x), ptr(y), ptr(gminx), ptr(argx), ptr(gminy),
                                                ptr(argy), ptr(gx), ptr(gy), stream_of(x)),
              "pdgn_chamfer_gram_grad")
        return gx, gy


def chamfer_min(x, y):
    return ChamferGram.apply(x, y)


class ChamferSum(Function):
    """scale * (sum_i min_j P + sum_j min_i P) as ONE autograd node: the minima of both directions land in one
    buffer (one reduction), and the adjoint feeds the uniform upstream gradient straight to the scatter kernel --
    the per-term sum / add / div / expand launches of the 12 local-pair terms disappear."""

    @staticmethod
    def forward(ctx, x, y, scale):
        x, y = x.contiguous(), y.contiguous()
        require(x, "x", F32, 3)
        require(y, "y", F32, 3)
        b, m, d = x.shape
        n = y.shape[1]
        mins = torch.empty((b * (m + n),), dtype=F32, device=x.device)
        args = torch.empty((b * (m + n),), dtype=I32, device=x.device)
        minx, miny, argx, argy = mins[:b * m], mins[b * m:], args[:b * m], args[b * m:]
        check(_lib.lib().pdgn_chamfer_gram(b, m, n, d, ptr(x), ptr(y), ptr(minx), ptr(argx), ptr(miny), ptr(argy),
                                           stream_of(x)), "pdgn_chamfer_gram")
        ctx.save_for_backward(x, y, args)
        ctx.scale = float(scale)
        out = torch.empty((), dtype=F32, device=x.device)
        check(_lib.lib().pdgn_scaled_sum(b * (m + n), ptr(mins), ctx.scale, ptr(out), stream_of(x)), "pdgn_scaled_sum")
        return out

    @staticmethod
    def backward(ctx, g):
        x, y, args = ctx.saved_tensors
        b, m, d = x.shape
        n = y.shape[1]
        gbuf = torch.empty((b * (m + n) * d,), dtype=F32, device=x.device)      # gx | gy: one zero-fill inside the call
        gx, gy = gbuf[:b * m * d].view(b, m, d), gbuf[b * m * d:].view(b, n, d)
        g = g.contiguous()
        check(_lib.lib().pdgn_chamfer_gram_grad_uniform(b, m, n, d, ptr(x), ptr(y), ptr(g), ctx.scale,
                                                        ptr(args[:b * m]), ptr(args[b * m:]), ptr(gx), ptr(gy), stream_of(x)),
              "pdgn_chamfer_gram_grad_uniform")
        return gx, gy, None


class MseConst(Function):
    """scale * nn.MSELoss()(x, target * ones_like(x)) -- the adversarial terms mse(D(x), 1) / mse(D(x), 0) with their 1/2
    (models/PDGNet_v2.py:186-190, 246-250) -- as one launch forward and one backward (csrc/loss_small.hip)."""

    @staticmethod
    def forward(ctx, x, target, scale, count=None):
        x = x.contiguous()
        require(x, "x", F32)
        out = torch.empty((), dtype=F32, device=x.device)
        if count is None:
            check(_lib.lib().pdgn_mse_const(x.numel(), ptr(x), target, scale, ptr(out), stream_of(x)), "pdgn_mse_const")
        else:                                                    # the same value bit for bit, and (#{x > 1/2}, #{x < 1/2}, n) stored into the slot
            check(_lib.lib().pdgn_mse_const_count(x.numel(), ptr(x), target, scale, 0.5, ptr(out), ptr(count), stream_of(x)), "pdgn_mse_const_count")
        ctx.save_for_backward(x)
        ctx.cfg = (float(target), float(scale))
        return out

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        target, scale = ctx.cfg
        dx = torch.empty_like(x)
        g = g.contiguous()
        check(_lib.lib().pdgn_mse_const_backward(x.numel(), ptr(x), target, scale, ptr(g), ptr(dx), stream_of(x)), "pdgn_mse_const_backward")
        return dx, None, None, None


def mse_const(x, target, scale=1.0, count=None):
    """scale * mean((x - target)^2) (MseConst).  count: None, or a slot of the adaptive augmentation (`Augment.counter(i)`: four int32
    words on x's device) into which the same launch stores how many x lie above / below the decision boundary 0.5, and their number."""
    if count is not None:
        require(count, "count", torch.int32)
        if count.numel() < 3 or count.device != x.device:
            raise ValueError("count: at least three int32 words on %s" % (x.device,))
    return MseConst.apply(x, float(target), float(scale), count)


GAN_LOSSES = ("lsgan", "hinge", "logistic")
_GAN_KINDS = {"hinge": 1, "logistic": 2}                        # PDGN_GAN_HINGE, PDGN_GAN_LOGISTIC (0: least squares, which is mse_const)
_GAN_ROLES = {"d_real": 0, "d_fake": 1, "g": 2}                 # PDGN_GAN_D_REAL, PDGN_GAN_D_FAKE, PDGN_GAN_G


class GanTerm(Function):
    """scale * mean f(x) of a discriminator's raw scores x for the hinge or the non-saturating logistic objective (include/pdgn_hip.h:
    pdgn_gan_term) -- like MseConst one launch forward and one backward (csrc/loss_small.hip), in the same summation order."""

    @staticmethod
    def forward(ctx, x, kind, role, scale, count=None):
        x = x.contiguous()
        require(x, "x", F32)
        out = torch.empty((), dtype=F32, device=x.device)
        if count is None:
            check(_lib.lib().pdgn_gan_term(x.numel(), ptr(x), kind, role, scale, ptr(out), stream_of(x)), "pdgn_gan_term")
        else:                                                    # the same value bit for bit, and (#{x > 0}, #{x < 0}, n) stored into the slot
            check(_lib.lib().pdgn_gan_term_count(x.numel(), ptr(x), kind, role, scale, 0.0, ptr(out), ptr(count), stream_of(x)), "pdgn_gan_term_count")
        ctx.save_for_backward(x)
        ctx.cfg = (kind, role, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        kind, role, scale = ctx.cfg
        dx = torch.empty_like(x)
        g = g.contiguous()
        check(_lib.lib().pdgn_gan_term_backward(x.numel(), ptr(x), kind, role, scale, ptr(g), ptr(dx), stream_of(x)), "pdgn_gan_term_backward")
        return dx, None, None, None, None


def gan_term(x, kind, role, scale=1.0, count=None):
    """scale * mean f(x) (GanTerm) of raw scores x.  kind "hinge": f = max(0, 1 - x) for role "d_real", max(0, 1 + x) for "d_fake", -x for
    "g"; kind "logistic" (non-saturating): f = softplus(-x), softplus(x), softplus(-x).  A NaN score gives a NaN term and a NaN gradient.
    count: as mse_const's, with the decision boundary of a logit, 0."""
    if kind not in _GAN_KINDS:
        raise ValueError("kind: 'hinge' or 'logistic', got %r" % (kind,))
    if role not in _GAN_ROLES:
        raise ValueError("role: 'd_real', 'd_fake' or 'g', got %r" % (role,))
    if count is not None:
        require(count, "count", torch.int32)
        if count.numel() < 3 or count.device != x.device:
            raise ValueError("count: at least three int32 words on %s" % (x.device,))
    return GanTerm.apply(x, _GAN_KINDS[kind], _GAN_ROLES[role], float(scale), count)


def decision_boundary(objective):
    """The score at which a discriminator trained on `objective` is undecided: 1/2 between least squares' targets 0 and 1, 0 for a logit.
    The adaptive augmentation's statistic counts the real batch's scores above and below it."""
    if objective not in GAN_LOSSES:
        raise ValueError("objective: one of %s, got %r" % (", ".join(GAN_LOSSES), objective))
    return 0.5 if objective == "lsgan" else 0.0


_LSGAN = {"d_real": (1.0, 0.5), "d_fake": (0.0, 0.5), "g": (1.0, 1.0)}     # (target, scale): models/PDGNet_v2.py:186-190, 246-250


def adversarial(x, objective, role, count=None):
    """One adversarial term of the training step on the scores x = D(cloud), with the objective's own scale: "lsgan" is the reference's
    mse(x, 1) / 2, mse(x, 0) / 2 and mse(x, 1) -- `mse_const`, reached through this module's attribute --, "hinge" and "logistic" the
    textbook forms (gan_term at scale 1, without the reference's 1/2).  count: the real-batch term's slot of the adaptive augmentation;
    it counts against decision_boundary(objective)."""
    if objective not in GAN_LOSSES:
        raise ValueError("objective: one of %s, got %r" % (", ".join(GAN_LOSSES), objective))
    if role not in _GAN_ROLES:
        raise ValueError("role: 'd_real', 'd_fake' or 'g', got %r" % (role,))
    if objective == "lsgan":
        target, scale = _LSGAN[role]
        return mse_const(x, target, scale) if count is None else mse_const(x, target, scale, count)
    return gan_term(x, objective, role, 1.0, count)


REPULSION_MAX_POINTS = 8192                                      # PDGN_REPULSION_MAX_N


def repulsion_constants(radius, b, n):
    """(inv_h2, coef) of pdgn_repulsion for b clouds of n points at radius h: 1 / h^2 and -8 / (h^2 b n), each computed in fp64; the
    call rounds each once to fp32."""
    radius = float(radius)
    if not (radius > 0.0 and radius < float("inf")):
        raise ValueError("radius must be positive and finite, got %r" % (radius,))
    inv = 1.0 / (radius * radius)
    return inv, -8.0 * inv / (float(b) * float(n))


def repulsion_pass(x, radius, grad=True, nn2=False, per_cloud=False):
    """The all-pairs launch on x (B,N,3), point-major and contiguous: (loss 0-dim, per_cloud (B) | None, grad (B,N,3) | None,
    nn2 (B,N) | None); an output that is not asked for is passed as NULL and not computed.  No autograd (losses.repulsion is the
    differentiable form; evaluation.spacing_stats the metric)."""
    require(x, "x", F32, 3)
    b, n, three = x.shape
    if three != 3:
        raise ValueError("x must be (B,N,3), got %s" % (tuple(x.shape),))
    if not 1 <= n <= REPULSION_MAX_POINTS:
        raise ValueError("repulsion takes clouds of 1 to %d points, got %d" % (REPULSION_MAX_POINTS, n))
    inv, coef = repulsion_constants(radius, b, n)
    s = torch.empty((b, n), dtype=F32, device=x.device)
    loss = torch.empty((), dtype=F32, device=x.device)
    pc = torch.empty((b,), dtype=F32, device=x.device) if per_cloud else None
    g = torch.empty((b, n, 3), dtype=F32, device=x.device) if grad else None
    nn = torch.empty((b, n), dtype=F32, device=x.device) if nn2 else None
    check(_lib.lib().pdgn_repulsion(b, n, ptr(x), inv, coef, ptr(s), ptr(loss), ptr(pc), ptr(g), ptr(nn), stream_of(x)), "pdgn_repulsion")
    return loss, pc, g, nn


class Repulsion(Function):
    """x (B,N,3) -> (1 / (B N)) sum_b sum_i sum_{j != i} max(0, 1 - |x_i - x_j|^2 / h^2)^2 as ONE autograd node (csrc/repulsion.hip):
    the forward launch computes the gradient too and saves it, the backward multiplies it by the upstream scalar."""

    @staticmethod
    def forward(ctx, x, radius):
        loss, _, g, _ = repulsion_pass(x, radius)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, up):
        g, = ctx.saved_tensors
        dx = torch.empty_like(g)
        up = up.contiguous()
        check(_lib.lib().pdgn_repulsion_backward(g.numel(), ptr(g), ptr(up), ptr(dx), stream_of(g)), "pdgn_repulsion_backward")
        return dx, None


def repulsion(cloud, radius):
    """The repulsion regulariser of a batch of clouds: the batch MEAN over clouds and points of
    s_i = sum_{j != i} max(0, 1 - |x_i - x_j|^2 / radius^2)^2 -- zero when no two points of a cloud are closer than `radius`.
    cloud: (B,3,N) as the generator returns it (its transpose is the contiguous point-major memory: no copy), or point-major (B,N,3);
    (B,3,3) reads as (B,3,N).  One launch and the reduction forward, one launch backward; every sum in a fixed order (bitwise
    repeatable); a NaN coordinate gives a NaN loss and NaN gradients for its cloud."""
    if not isinstance(cloud, torch.Tensor) or cloud.dim() != 3 or 3 not in cloud.shape[1:]:
        raise ValueError("cloud must be a (B,3,N) or (B,N,3) tensor")
    x = cloud.transpose(1, 2) if cloud.shape[1] == 3 else cloud
    return Repulsion.apply(x.contiguous(), float(radius))


def repulsion_radii(radius, sizes):
    """The radius per level: radius * sqrt(N_finest / N_l) for the point counts `sizes` -- `radius` is the finest level's, and points
    spread over a surface have spacing proportional to N^-1/2."""
    sizes = [int(n) for n in sizes]
    if not sizes or min(sizes) < 1:
        raise ValueError("sizes: at least one positive point count, got %r" % (sizes,))
    radius = float(radius)
    if not (radius > 0.0 and radius < float("inf")):
        raise ValueError("radius must be positive and finite, got %r" % (radius,))
    finest = max(sizes)
    return [radius * (float(finest) / float(n)) ** 0.5 for n in sizes]


FLATNESS_MAX_K = 64                                              # PDGN_NORMALS_MAX_K


def _flatness_eps(eps):
    eps = float(eps)
    if not (0.0 <= eps < float("inf")):
        raise ValueError("eps must be finite and not negative, got %r" % (eps,))
    return eps


def flatness_pass(x, idx, eps=0.0, grad=True, per_cloud=False, degenerate=None):
    """pdgn_flatness on x (B,N,3), point-major and contiguous, with the neighbour lists idx (B,N,k) int32: (loss 0-dim, per_cloud (B) |
    None, grad (B,N,3) | None, sigma (B,N), degenerate (B) int32 -- the caller's tensor where one is given); without `grad` no record is
    written and nothing is transposed.  No autograd (losses.flatness is the differentiable form; evaluation.surface_stats the metric)."""
    eps = _flatness_eps(eps)
    require(x, "x", F32, 3)
    require(idx, "idx", I32, 3)
    b, n, three = x.shape
    if three != 3:
        raise ValueError("x must be (B,N,3), got %s" % (tuple(x.shape),))
    k = idx.shape[2]
    if tuple(idx.shape[:2]) != (b, n) or not 1 <= k <= FLATNESS_MAX_K or idx.device != x.device:
        raise ValueError("idx must be (B,N,k) = (%d,%d,1..%d) on %s, got %s" % (b, n, FLATNESS_MAX_K, x.device, tuple(idx.shape)))
    L = _lib.lib()
    size = L.pdgn_flatness_workspace_bytes(b, n, k, 1 if grad else 0)
    if size < 0:
        raise _lib.PdgnHipError("pdgn_flatness_workspace_bytes: argument outside the supported range")
    sigma = torch.empty((b, n), dtype=F32, device=x.device)
    loss = torch.empty((), dtype=F32, device=x.device)
    pc = torch.empty((b,), dtype=F32, device=x.device) if per_cloud else None
    if degenerate is None:
        deg = torch.empty((b,), dtype=I32, device=x.device)
    else:
        deg = require(degenerate, "degenerate", I32, 1)
        if deg.shape[0] != b or deg.device != x.device:
            raise ValueError("degenerate must be (B) = (%d) int32 on %s" % (b, x.device))
    g = torch.empty((b, n, 3), dtype=F32, device=x.device) if grad else None
    ws = torch.empty((size // 4,), dtype=I32, device=x.device) if grad else None
    check(L.pdgn_flatness(b, n, k, ptr(x), ptr(idx), eps, 1.0 / (float(b) * float(n)), ptr(sigma), ptr(loss), ptr(pc), ptr(deg), ptr(g),
                          ptr(ws), stream_of(x)), "pdgn_flatness")
    return loss, pc, g, sigma, deg


class Flatness(Function):
    """x (B,N,3), idx (B,N,k) -> the batch mean of the surface variation as ONE autograd node (csrc/flatness.hip): the forward computes the
    gradient too and saves it, the backward multiplies it by the upstream scalar (pdgn_repulsion_backward).  Nothing flows to idx."""

    @staticmethod
    def forward(ctx, x, idx, eps, degenerate=None):
        loss, _, g, _, _ = flatness_pass(x, idx, eps, degenerate=degenerate)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, up):
        g, = ctx.saved_tensors
        dx = torch.empty_like(g)
        up = up.contiguous()
        check(_lib.lib().pdgn_repulsion_backward(g.numel(), ptr(g), ptr(up), ptr(dx), stream_of(g)), "pdgn_repulsion_backward")
        return dx, None, None, None


def flatness(cloud, k=16, idx=None, eps=0.0, degenerate=None):
    """The flatness regulariser of a batch of clouds: the batch MEAN over clouds and points of Pauly's surface
    variation sigma_i = l0 / (l0 + l1 + l2 + eps) of the covariance of point i's k neighbours -- zero where every neighbourhood is flat.
    cloud: (B,3,N) as the generator returns it, or point-major (B,N,3); (B,3,3) reads as (B,3,N).  idx: the neighbour lists (B,N,k)
    int32, or None: pointops.knnquery(k, x, x) of the detached cloud (k <= N).  The lists are data: the neighbour choice is not
    differentiated.  degenerate: None, or a (B) int32 tensor that receives every cloud's number of degenerate points (sigma = 0: coincident
    points, an exactly flat neighbourhood).  Every sum in a fixed order (bitwise repeatable, no float atomics); a NaN coordinate gives a NaN loss and NaN
    gradients on its neighbourhoods' points."""
    if not isinstance(cloud, torch.Tensor) or cloud.dim() != 3 or 3 not in cloud.shape[1:]:
        raise ValueError("cloud must be a (B,3,N) or (B,N,3) tensor")
    eps = _flatness_eps(eps)
    x = cloud.transpose(1, 2) if cloud.shape[1] == 3 else cloud
    n = x.shape[1]
    if idx is None:
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(FLATNESS_MAX_K, n):
            raise ValueError("k must be an integer from 1 to min(%d, N = %d), got %r" % (FLATNESS_MAX_K, n, k))
    elif not isinstance(idx, torch.Tensor) or idx.dtype != I32 or idx.dim() != 3 or tuple(idx.shape[:2]) != (x.shape[0], n) or not 1 <= idx.shape[2] <= FLATNESS_MAX_K:
        raise ValueError("idx must be an int32 tensor (B,N,k) = (%d,%d,1..%d)" % (x.shape[0], n, FLATNESS_MAX_K))
    x = x.contiguous()
    if idx is None:
        with torch.no_grad():
            idx = pointops.knnquery(k, x.detach(), x.detach())
    return Flatness.apply(x, idx.contiguous(), eps, degenerate)


def flatness_floors(eps, sizes):
    """The floor per level: eps * N_finest / N_l for the point counts `sizes` -- `eps` is the finest level's, and a neighbourhood's trace
    scales with the squared spacing, about 1 / N."""
    sizes = [int(n) for n in sizes]
    if not sizes or min(sizes) < 1:
        raise ValueError("sizes: at least one positive point count, got %r" % (sizes,))
    eps = _flatness_eps(eps)
    finest = max(sizes)
    return [eps * float(finest) / float(n) for n in sizes]


class SurfaceDistance(Function):
    """xyz (B,N,3) -> d2 (B,N), the squared distance of every point to the surface of its shape, as ONE autograd node over
    meshes.point_to_mesh (csrc/meshdist.hip): the forward launch returns the closest points and saves them, the backward is the tensor
    expression 2 g (p - closest), zero where d2 is NaN.  Nothing flows to the mesh."""

    @staticmethod
    def forward(ctx, xyz, meshset, shape, visible_only):
        from .meshes import point_to_mesh
        d2, face, closest = point_to_mesh(xyz, meshset, shape, visible_only, return_closest=True)
        ctx.save_for_backward(xyz, closest, d2)
        ctx.mark_non_differentiable(face)
        return d2, face

    @staticmethod
    def backward(ctx, g, _):
        xyz, closest, d2 = ctx.saved_tensors
        dx = (2.0 * g)[..., None] * (xyz - closest)
        return torch.where(torch.isnan(d2)[..., None], torch.zeros_like(dx), dx), None, None, None


def surface_distance(xyz, meshset, shape=None, reduction="mean", visible_only=False):
    """The squared distance of the points of xyz (B,N,3) to the surface of shape[c] of a meshes.MeshSet,
    differentiable in xyz: d d2 / d p = 2 (p - closest point), exact wherever the closest point is unique (away from the medial axis).
    reduction: "none" -> (B,N) with NaN at a point that is not finite; "sum" / "mean" -> over the points whose d2 is not NaN (0 where
    there is none).  Unsigned, and not differentiable in the mesh."""
    if reduction not in ("none", "sum", "mean"):
        raise ValueError("surface_distance: reduction is 'none', 'sum' or 'mean', got %r" % (reduction,))
    d2, _ = SurfaceDistance.apply(xyz, meshset, shape, bool(visible_only))
    if reduction == "none":
        return d2
    valid = ~torch.isnan(d2)
    total = torch.where(valid, d2, torch.zeros_like(d2)).sum()
    return total if reduction == "sum" else total / valid.sum().clamp_min(1)


def chamfer_sum(x, y, scale=1.0):
    """scale * ChamferLoss-style sum of both directions' minima (utils/chamfer_loss.py:16-20)."""
    return ChamferSum.apply(x, y, scale)


class LocalStats(Function):
    """xyz (B,N,3), idx (B,M,K) int32 -> mu (B,M,3), cov (B,M,9): grouping (:142-145) +
    compute_mean_covariance (:127-134) in one pass; backward scatters onto xyz."""

    @staticmethod
    def forward(ctx, xyz, idx):
        require(xyz, "xyz", F32, 3)
        require(idx, "idx", I32, 3)
        b, n, _ = xyz.shape
        _, m, k = idx.shape
        mu = torch.empty((b, m, 3), dtype=F32, device=xyz.device)
        cov = torch.empty((b, m, 9), dtype=F32, device=xyz.device)
        check(_lib.lib().pdgn_local_stats(b, n, m, k, ptr(xyz), ptr(idx), ptr(mu), ptr(cov), stream_of(xyz)),
              "pdgn_local_stats")
        ctx.save_for_backward(xyz, idx)
        return mu, cov

    @staticmethod
    def backward(ctx, dmu, dcov):
        xyz, idx = ctx.saved_tensors
        b, n, _ = xyz.shape
        _, m, k = idx.shape
        dxyz = _zeros(tuple(xyz.shape), xyz.device)           # (a slice of the backward pass's zero arena: no fill launch)
        dmu, dcov = dmu.contiguous(), dcov.contiguous()
        check(_lib.lib().pdgn_local_stats_backward(b, n, m, k, ptr(xyz), ptr(idx), ptr(dmu), ptr(dcov), ptr(dxyz),
                                                   stream_of(xyz)), "pdgn_local_stats_backward")
        return dxyz, None


def local_stats(xyz, idx):
    return LocalStats.apply(xyz, idx)


def knnquery(nsample, xyz, new_xyz):
    return pointops.knnquery(nsample, xyz, new_xyz)


class ChamferLoss(nn.Module):
    """utils/chamfer_loss.py:13-38: SUM (not mean) over batch and points of the row minima and
    the column minima of the Gram-form pairwise matrix."""

    def forward(self, preds, gts):
        return chamfer_sum(gts, preds, 1.0)


def compute_mean_covariance(points):
    """models/PDGNet_v2.py:127-134 (torch ops; kept for API parity).  points (R,3,k)."""
    mu = points.mean(dim=-1, keepdim=True)
    tmp = points - mu
    return mu, torch.bmm(tmp, tmp.transpose(1, 2)) / points.shape[-1]


class LocalPairLoss(nn.Module):
    """get_local_pair :136-155: neighbourhood (k = 20) means and covariances of both clouds around
    pt1's points, compared with Chamfer, divided by M."""

    def __init__(self, nsample=20):
        super().__init__()
        self.nsample = nsample
        self.chamfer_loss = ChamferLoss()

    def stats(self, cloud_cl, query_cl):
        """cloud (B,N,3), queries (B,M,3) point-major -> (mu (B,M,3), cov (B,M,9))."""
        idx = knnquery(self.nsample, cloud_cl, query_cl)
        return local_stats(cloud_cl, idx)

    def forward(self, pt1, pt2, self_stats=None):
        """pt1 (B,3,M), pt2 (B,3,N>=M).  `self_stats` = stats(pt1, pt1) when the caller already has
        them (pt1 is grouped around itself identically in every pair it heads, :232-237)."""
        M = pt1.shape[2]
        new_xyz = pt1.transpose(1, 2).contiguous()
        mu1, var1 = self_stats if self_stats is not None else self.stats(new_xyz, new_xyz)
        mu2, var2 = self.stats(pt2.transpose(1, 2).contiguous(), new_xyz)
        return chamfer_sum(mu2, mu1, 1.0 / float(M)), chamfer_sum(var2, var1, 1.0 / float(M))
