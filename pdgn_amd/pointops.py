"""Drop-in for the reference's ``lib/pointops/functions/pointops.py`` on MI355X.

Same callables, argument order, dtypes and autograd contract as the reference
(file:line cited per symbol); the native side is libpdgn_hip.so (include/pdgn_hip.h)
instead of the ``pointops_cuda`` pybind module.  Differences, all deliberate:
  * outputs are allocated on the INPUT's device (the reference uses the legacy
    ``torch.cuda.IntTensor(...)`` constructors = current device, pointops.py:425-426);
  * kernels run on torch's current stream (the reference's grouping/interpolation use the
    legacy null stream, grouping_cuda_kernel.cu:85);
  * launch failures raise ``PdgnHipError`` (the reference calls ``exit(-1)``).
There is no CPU path: CPU tensors raise.
"""
from typing import Tuple

import numpy as np
import torch
import torch.nn as nn
from ._fn import Function

from . import _lib
from ._lib import check, ptr, require, stream_of

F32, I32 = torch.float32, torch.int32


# ------------------------------------------------------------------ hot-path Functions
class KNNQuery(Function):
    """pointops.py:408-434.  (nsample, xyz (b,n,3), new_xyz (b,m,3)|None) -> idx (b,m,nsample) int32."""

    @staticmethod
    def forward(ctx, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor = None) -> torch.Tensor:
        if new_xyz is None:
            new_xyz = xyz
        require(xyz, "xyz", F32, 3)
        require(new_xyz, "new_xyz", F32, 3)
        b, m, _ = new_xyz.size()
        n = xyz.size(1)
        idx = torch.empty((b, m, nsample), dtype=I32, device=xyz.device)
        dist2 = torch.empty((b, m, nsample), dtype=F32, device=xyz.device)
        check(_lib.lib().pdgn_knnquery(b, n, m, int(nsample), ptr(xyz), ptr(new_xyz), ptr(idx),
                                       ptr(dist2), stream_of(xyz)), "pdgn_knnquery")
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None


knnquery = KNNQuery.apply


def knnquery_with_dist(nsample, xyz, new_xyz=None):
    """Like ``knnquery`` but also returns the squared distances the kernel computes
    (the reference writes and then drops them, pointops.py:426-428)."""
    if new_xyz is None:
        new_xyz = xyz
    require(xyz, "xyz", F32, 3)
    require(new_xyz, "new_xyz", F32, 3)
    b, m, _ = new_xyz.size()
    idx = torch.empty((b, m, nsample), dtype=I32, device=xyz.device)
    dist2 = torch.empty((b, m, nsample), dtype=F32, device=xyz.device)
    check(_lib.lib().pdgn_knnquery(b, xyz.size(1), m, int(nsample), ptr(xyz), ptr(new_xyz), ptr(idx),
                                   ptr(dist2), stream_of(xyz)), "pdgn_knnquery")
    return idx, dist2


_ORIENT = {"direction": 1, "towards": 2, "away": 3}


@torch.no_grad()
def estimate_normals(xyz, k=16, idx=None, orient=None, return_eig=False):
    """Per-point surface normals from the covariance of each point's k nearest neighbours (pdgn_estimate_normals, csrc/normals.hip,
    DESIGN.md section 7q; no reference counterpart).  xyz (B,N,3) fp32 on the device -> normals (B,N,3); with return_eig=True
    (normals, eig (B,N,3)), the neighbourhood covariance's eigenvalues ascending.  idx: (B,N,k') int32 neighbour lists of the caller's
    (`k` is then ignored); None: knnquery(k, xyz, xyz), which needs k <= N.  orient: None (the component of largest magnitude is made
    non-negative), ("direction", v) (n . v >= 0), ("towards", p) (n . (p - x) >= 0) or ("away", p) (n . (x - p) >= 0), v / p three
    numbers, or "consistent" (the estimate with orient=None, then orient_normals with the same lists: N <= 4096, k <= 64), or "visible"
    (the estimate with orient=None, then orient_normals_visible at its defaults with the same lists: any N, k <= 64; thin sheets, which
    "consistent" gets wrong).  A point with
    an index outside the cloud or a non-finite neighbour gets NaNs.  NOT differentiable: the results carry no graph (the differentiable
    flatness loss on the same eigenvalues is losses.flatness)."""
    require(xyz, "xyz", F32, 3)
    if xyz.shape[2] != 3:
        raise ValueError("xyz must be (B,N,3), got %s" % (tuple(xyz.shape),))
    b, n, _ = xyz.shape
    if idx is None:
        if not 1 <= int(k) <= n:
            raise ValueError("estimate_normals: k = %r neighbours of a cloud of %d points" % (k, n))
        idx = knnquery(int(k), xyz, xyz)
    else:
        require(idx, "idx", I32, 3)
        if tuple(idx.shape[:2]) != (b, n) or idx.device != xyz.device:
            raise ValueError("idx must be (B,N,k) on xyz's device, got %s for xyz %s" % (tuple(idx.shape), tuple(xyz.shape)))
    mode, o = 0, (0.0, 0.0, 0.0)
    consistent = isinstance(orient, str) and orient == "consistent"
    visible = isinstance(orient, str) and orient == "visible"
    if orient is not None and not consistent and not visible:
        bad = "orient must be None, \"consistent\", \"visible\" or (\"direction\" | \"towards\" | \"away\", three numbers), got %r" % (orient,)
        try:
            kind, o = orient
            mode, o = _ORIENT[kind], tuple(float(v) for v in o)
        except (KeyError, TypeError, ValueError):
            raise ValueError(bad) from None
        if len(o) != 3:
            raise ValueError(bad)
    if consistent and n > ORIENT_MAX_N:
        raise ValueError("estimate_normals: orient=\"consistent\" takes clouds of at most %d points, got %d" % (ORIENT_MAX_N, n))
    normals = torch.empty((b, n, 3), dtype=F32, device=xyz.device)
    eig = torch.empty((b, n, 3), dtype=F32, device=xyz.device) if return_eig else None
    check(_lib.lib().pdgn_estimate_normals(b, n, idx.shape[2], ptr(xyz), ptr(idx), mode, o[0], o[1], o[2], ptr(normals), ptr(eig),
                                           stream_of(xyz)), "pdgn_estimate_normals")
    if consistent:
        normals = orient_normals(xyz, normals, idx=idx)
    if visible:
        normals = orient_normals_visible(xyz, normals, idx=idx)
    return (normals, eig) if return_eig else normals


ORIENT_MAX_N = 4096                                                # PDGN_ORIENT_MAX_N
ORIENT_MAX_K = 64                                                  # PDGN_NORMALS_MAX_K


@torch.no_grad()
def orient_normals(xyz, normals, k=16, idx=None, return_tree=False):
    """A consistent sign for the normals of every cloud (pdgn_orient_normals, csrc/orient.hip; no reference
    counterpart): the sign is propagated along a minimum spanning tree of the symmetrised neighbour graph under the weight 1 - |n_u . n_v|,
    from the highest point of each connected component, whose normal is turned upwards.  xyz (B,N,3), normals (B,N,3) fp32 on the device
    (estimate_normals' with orient=None) -> normals (B,N,3), a new tensor that differs from the input in sign bits alone; with
    return_tree=True (normals, parent (B,N) int32: the tree parent, -1 a component's root, -2 a point with a non-finite coordinate or normal,
    stats (B,4) int32: components, normals flipped, tree edges across more than 60 degrees, dead points).  idx as in estimate_normals: (B,N,k')
    int32 lists of the caller's (`k` is then ignored), or None: knnquery(k, xyz, xyz).  N <= 4096, k' <= 64.  NOT differentiable."""
    require(xyz, "xyz", F32, 3)
    if xyz.shape[2] != 3:
        raise ValueError("xyz must be (B,N,3), got %s" % (tuple(xyz.shape),))
    require(normals, "normals", F32, 3)
    if normals.shape != xyz.shape or normals.device != xyz.device:
        raise ValueError("normals must be (B,N,3) on xyz's device, got %s for xyz %s" % (tuple(normals.shape), tuple(xyz.shape)))
    b, n, _ = xyz.shape
    if not 1 <= n <= ORIENT_MAX_N or b < 1:
        raise ValueError("orient_normals: clouds of 1 .. %d points, got %s" % (ORIENT_MAX_N, tuple(xyz.shape)))
    if idx is None:
        if not 1 <= int(k) <= min(n, ORIENT_MAX_K):
            raise ValueError("orient_normals: k = %r neighbours of a cloud of %d points (at most %d)" % (k, n, ORIENT_MAX_K))
        idx = knnquery(int(k), xyz, xyz)
    else:
        require(idx, "idx", I32, 3)
        if tuple(idx.shape[:2]) != (b, n) or idx.device != xyz.device:
            raise ValueError("idx must be (B,N,k) on xyz's device, got %s for xyz %s" % (tuple(idx.shape), tuple(xyz.shape)))
        if not 1 <= idx.shape[2] <= ORIENT_MAX_K:
            raise ValueError("orient_normals: lists of 1 .. %d neighbours, got %d" % (ORIENT_MAX_K, idx.shape[2]))
    L = _lib.lib()
    out = torch.empty_like(normals)
    parent = torch.empty((b, n), dtype=I32, device=xyz.device) if return_tree else None
    stats = torch.empty((b, 4), dtype=I32, device=xyz.device) if return_tree else None
    work = torch.empty((int(L.pdgn_orient_workspace_ints(b, n, idx.shape[2])),), dtype=I32, device=xyz.device)
    check(L.pdgn_orient_normals(b, n, idx.shape[2], ptr(xyz), ptr(idx), ptr(normals), ptr(out), ptr(parent), ptr(stats), ptr(work),
                                stream_of(xyz)), "pdgn_orient_normals")
    return (out, parent, stats) if return_tree else out


VISIBLE_MAX_VIEWS, VISIBLE_MAX_RESOLUTION = 32, 192                # PDGN_VISIBLE_MAX_VIEWS, PDGN_VISIBLE_MAX_RES
VISIBLE_SPACING_MAX_N = 8192                                       # PDGN_REPULSION_MAX_N: the all-pairs launch behind radius=None
POOL_MAX_ROUNDS = 4                                                # PDGN_CLOUDVIS_MAX_ROUNDS


def _cloud_pair(xyz, normals, what):
    require(xyz, "xyz", F32, 3)
    require(normals, "normals", F32, 3)
    if xyz.shape[2] != 3 or xyz.shape[0] < 1 or xyz.shape[1] < 1:
        raise ValueError("%s: xyz must be (B,N,3) with B, N >= 1, got %s" % (what, tuple(xyz.shape)))
    if normals.shape != xyz.shape or normals.device != xyz.device:
        raise ValueError("%s: normals must be (B,N,3) on xyz's device, got %s for xyz %s" % (what, tuple(normals.shape), tuple(xyz.shape)))
    return xyz.shape[0], xyz.shape[1]


@torch.no_grad()
def cloud_frames(xyz):
    """(B,4) fp32 (centre, radius) per cloud: the centre of the box of its points and the largest distance of a point from it times
    (1 + 2^-10), in fp64 torch ops on the device, rounded once -- meshes.shape_frames' rule for points.  Points with a non-finite
    coordinate do not count; a cloud without a finite point, or of one repeated point, gets the radius 1."""
    require(xyz, "xyz", F32, 3)
    if xyz.shape[2] != 3 or xyz.shape[0] < 1 or xyz.shape[1] < 1:
        raise ValueError("cloud_frames: xyz must be (B,N,3) with B, N >= 1, got %s" % (tuple(xyz.shape),))
    x = xyz.double()
    ok = torch.isfinite(x).all(dim=2, keepdim=True)
    lo = torch.where(ok, x, torch.full_like(x, float("inf"))).amin(dim=1)
    hi = torch.where(ok, x, torch.full_like(x, float("-inf"))).amax(dim=1)
    ctr = torch.where(ok.any(dim=1), (lo + hi) / 2, torch.zeros_like(lo))
    d2 = torch.where(ok[:, :, 0], ((x - ctr[:, None, :]) ** 2).sum(dim=2), torch.zeros_like(x[:, :, 0])).amax(dim=1)
    rho = d2.sqrt() * (1.0 + 2.0 ** -10)
    rho = torch.where(rho > 0, rho, torch.ones_like(rho))
    return torch.cat([ctr, rho[:, None]], dim=1).float().contiguous()


def _view_table(views, what):
    from .meshes import default_views, view_bases
    table = default_views(views) if np.ndim(views) == 0 else np.asarray(views.cpu() if isinstance(views, torch.Tensor) else views)
    table = view_bases(table) if table.ndim == 2 else np.ascontiguousarray(table, dtype=np.float32)
    if table.ndim != 3 or table.shape[1:] != (3, 3) or not 1 <= table.shape[0] <= VISIBLE_MAX_VIEWS:
        raise ValueError("%s: views are a count, (NV,3) directions or (NV,3,3) bases, at most %d, got %s" % (what, VISIBLE_MAX_VIEWS, table.shape,))
    return table


@torch.no_grad()
def normal_votes(xyz, normals, views=26, resolution=64, radius=None, radius_factor=2.0, bias=None, bias_factor=0.25, return_quanta=False):
    """From which side a ring of orthographic views sees every point (pdgn_cloud_normal_votes, csrc/cloudvis.hip; no
    reference counterpart): per (cloud, view) a depth buffer into which every point is splatted as a disc, then every point that is at
    most `bias` behind its own pixel's nearest depth votes with the weight (int)(256 min(|n . e_z|, 1)) for the side of it the view sees.
    xyz, normals (B,N,3) fp32 on the device -> (front, back) (B,N) int32: front counts the views the normal faces.  views as in
    meshes.face_visibility: 6 / 14 / 26, (NV,3) directions to look from, or (NV,3,3) bases.  resolution: pixels per image side, 1 .. 192.
    radius: the disc's, in the units of xyz, a number or (B); None: radius_factor times each cloud's mean nearest-neighbour distance (the
    all-pairs launch of reconstruct.mean_spacing: clouds of at most 8192 points then; a given radius has no limit).  bias: a depth in the
    units of xyz, a number or (B); None: bias_factor times the radius.  The launch takes ONE disc radius in sub-pixel units (256 to the
    pixel) and ONE bias in depth quanta (2^-20 of a frame's radius) for the whole batch: the batch means of radius / rho R 2^7 and of
    bias / rho 2^20 over the clouds' frames (cloud_frames), in fp64, each rounded once.  return_quanta=True appends {"splat", "bias"
    (those two integers), "frame" (B,4), "views" (NV,3,3) device tensors}: what a restatement of the kernel is fed.  NOT differentiable."""
    b, n = _cloud_pair(xyz, normals, "normal_votes")
    R = int(resolution)
    if not 1 <= R <= VISIBLE_MAX_RESOLUTION:
        raise ValueError("normal_votes: resolution %r, between 1 and %d pixels per side" % (resolution, VISIBLE_MAX_RESOLUTION))
    table = torch.from_numpy(_view_table(views, "normal_votes")).to(xyz.device)
    frame = cloud_frames(xyz)
    if radius is None:
        if not float(radius_factor) > 0:
            raise ValueError("normal_votes: radius_factor must be positive, got %r" % (radius_factor,))
        if n > VISIBLE_SPACING_MAX_N:
            raise ValueError("normal_votes: radius=None measures the spacing of clouds of at most %d points, got %d: give a radius"
                             % (VISIBLE_SPACING_MAX_N, n))
        from .reconstruct import mean_spacing
        radius = float(radius_factor) * mean_spacing(xyz)
    radius = torch.as_tensor(radius, dtype=torch.float64, device=xyz.device).expand(b)
    if bias is None:
        if not float(bias_factor) >= 0:
            raise ValueError("normal_votes: bias_factor must not be negative, got %r" % (bias_factor,))
        bias = float(bias_factor) * radius
    bias = torch.as_tensor(bias, dtype=torch.float64, device=xyz.device).expand(b)
    rho = frame[:, 3].double()
    splat_q, bias_q = float((radius / rho).mean() * (R * 128.0)), float((bias / rho).mean() * 1048576.0)
    if not (0 <= splat_q < 2 ** 30 and 0 <= bias_q < 2 ** 30):
        raise ValueError("normal_votes: radius and bias must be finite and not negative (a disc of %r sub-pixel units, a bias of %r quanta)" % (splat_q, bias_q))
    splat_q, bias_q = int(np.rint(splat_q)), int(np.rint(bias_q))
    votes = torch.empty((b, n, 2), dtype=I32, device=xyz.device)
    check(_lib.lib().pdgn_cloud_normal_votes(b, n, ptr(xyz), ptr(normals), ptr(frame), ptr(table), int(table.shape[0]), R, splat_q, bias_q,
                                             ptr(votes), stream_of(xyz)), "pdgn_cloud_normal_votes")
    front, back = votes[:, :, 0].contiguous(), votes[:, :, 1].contiguous()
    if return_quanta:
        return front, back, {"splat": splat_q, "bias": bias_q, "frame": frame, "views": table}
    return front, back


@torch.no_grad()
def orient_normals_visible(xyz, normals, k=16, idx=None, rounds=1, views=26, resolution=64, radius=None, radius_factor=2.0, bias=None,
                           bias_factor=0.25, return_votes=False, return_stats=False):
    """The sign of every normal from visibility (pdgn_cloud_normal_votes and pdgn_orient_pool, csrc/cloudvis.hip; no
    reference counterpart): `normal_votes`, then `rounds` (0 .. 4) Jacobi rounds in which a point adds to twice its own balance
    front - back the balances of its neighbours that lie in its tangent plane and agree with its normal line, then a negative balance turns
    the normal round.  Where orient_normals propagates a sign along a tree -- across a thin sheet at no cost, to 4096 points at most --
    this asks the outside directly: sheets thinner than a neighbourhood and clouds of any size.  It needs views that can see the surface:
    the inside of a cavity no view reaches stays undecided, or takes its neighbours' sign.  xyz, normals (B,N,3) fp32 on the device
    (estimate_normals' with orient=None) -> normals (B,N,3), a new tensor that differs from the input in sign bits alone (a point with
    balance 0 keeps its bits)[, with return_votes=True (front, back (B,N) int32, pooled (B,N) int64: the final balance)][, with
    return_stats=True stats (B,4) int32: normals flipped, live points undecided, live points no view saw, dead points (a non-finite
    coordinate or normal)].  idx as in orient_normals: (B,N,k') int32 lists, or None: knnquery(k, xyz, xyz); k' <= 64.  The remaining
    arguments are normal_votes'.  NOT differentiable."""
    b, n = _cloud_pair(xyz, normals, "orient_normals_visible")
    if not 0 <= int(rounds) <= POOL_MAX_ROUNDS:
        raise ValueError("orient_normals_visible: rounds between 0 and %d, got %r" % (POOL_MAX_ROUNDS, rounds))
    if idx is None:
        if not 1 <= int(k) <= min(n, ORIENT_MAX_K):
            raise ValueError("orient_normals_visible: k = %r neighbours of a cloud of %d points (at most %d)" % (k, n, ORIENT_MAX_K))
        idx = knnquery(int(k), xyz, xyz)
    else:
        require(idx, "idx", I32, 3)
        if tuple(idx.shape[:2]) != (b, n) or idx.device != xyz.device:
            raise ValueError("idx must be (B,N,k) on xyz's device, got %s for xyz %s" % (tuple(idx.shape), tuple(xyz.shape)))
        if not 1 <= idx.shape[2] <= ORIENT_MAX_K:
            raise ValueError("orient_normals_visible: lists of 1 .. %d neighbours, got %d" % (ORIENT_MAX_K, idx.shape[2]))
    front, back = normal_votes(xyz, normals, views, resolution, radius, radius_factor, bias, bias_factor)
    votes = torch.stack([front, back], dim=2).contiguous()
    out = torch.empty_like(normals)
    pooled = torch.empty((b, n), dtype=torch.int64, device=xyz.device) if return_votes else None
    stats = torch.empty((b, 4), dtype=I32, device=xyz.device) if return_stats else None
    work = torch.empty((2, b, n), dtype=torch.int64, device=xyz.device)
    check(_lib.lib().pdgn_orient_pool(b, n, idx.shape[2], ptr(xyz), ptr(idx), ptr(normals), ptr(votes), int(rounds), ptr(out), ptr(pooled),
                                      ptr(stats), ptr(work), stream_of(xyz)), "pdgn_orient_pool")
    result = (out,) + (((front, back, pooled),) if return_votes else ()) + ((stats,) if return_stats else ())
    return result if len(result) > 1 else out


class Grouping(Function):
    """pointops.py:122-151.  features (b,c,n), idx (b,m,nsample) -> (b,c,m,nsample);
    backward = scatter-add into (b,c,n)."""

    @staticmethod
    def forward(ctx, features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        require(features, "features", F32, 3)
        require(idx, "idx", I32, 3)
        b, c, n = features.size()
        _, m, nsample = idx.size()
        output = torch.empty((b, c, m, nsample), dtype=F32, device=features.device)
        check(_lib.lib().pdgn_grouping_forward(b, c, n, m, nsample, ptr(features), ptr(idx), ptr(output),
                                               stream_of(features)), "pdgn_grouping_forward")
        ctx.for_backwards = (idx, n)
        return output

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        idx, n = ctx.for_backwards
        b, c, m, nsample = grad_out.size()
        grad_features = torch.zeros((b, c, n), dtype=F32, device=grad_out.device)
        grad_out_data = grad_out.data.contiguous()
        if _lib.deterministic():                         # fixed order: a gather over the sorted transpose of idx
            ws = _lib.det_workspace(grad_out.device, (b, n, m * nsample))
            check(_lib.lib().pdgn_grouping_backward_det(b, c, n, m, nsample, ptr(grad_out_data), ptr(idx), ptr(ws),
                                                        ptr(grad_features), stream_of(grad_out_data)),
                  "pdgn_grouping_backward_det")
            return grad_features, None
        check(_lib.lib().pdgn_grouping_backward(b, c, n, m, nsample, ptr(grad_out_data), ptr(idx),
                                                ptr(grad_features), stream_of(grad_out_data)),
              "pdgn_grouping_backward")
        return grad_features, None


grouping = Grouping.apply


class NearestNeighbor(Function):
    """pointops.py:61-83.  unknown (b,n,3), known (b,m,3) -> (dist (b,n,3) = sqrt(dist2), idx (b,n,3))."""

    @staticmethod
    def forward(ctx, unknown: torch.Tensor, known: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        require(unknown, "unknown", F32, 3)
        require(known, "known", F32, 3)
        b, n, _ = unknown.size()
        m = known.size(1)
        dist2 = torch.empty((b, n, 3), dtype=F32, device=unknown.device)
        idx = torch.empty((b, n, 3), dtype=I32, device=unknown.device)
        check(_lib.lib().pdgn_nearestneighbor(b, n, m, ptr(unknown), ptr(known), ptr(dist2), ptr(idx),
                                              stream_of(unknown)), "pdgn_nearestneighbor")
        ctx.mark_non_differentiable(idx)
        return torch.sqrt(dist2), idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None


nearestneighbor = NearestNeighbor.apply


class Interpolation(Function):
    """pointops.py:86-119.  features (b,c,m), idx/weight (b,n,3) -> (b,c,n); grad wrt features."""

    @staticmethod
    def forward(ctx, features: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
        require(features, "features", F32, 3)
        require(idx, "idx", I32, 3)
        require(weight, "weight", F32, 3)
        b, c, m = features.size()
        n = idx.size(1)
        ctx.interpolation_for_backward = (idx, weight, m)
        output = torch.empty((b, c, n), dtype=F32, device=features.device)
        check(_lib.lib().pdgn_interpolation_forward(b, c, m, n, ptr(features), ptr(idx), ptr(weight),
                                                    ptr(output), stream_of(features)),
              "pdgn_interpolation_forward")
        return output

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        idx, weight, m = ctx.interpolation_for_backward
        b, c, n = grad_out.size()
        grad_features = torch.zeros((b, c, m), dtype=F32, device=grad_out.device)
        grad_out_data = grad_out.data.contiguous()
        if _lib.deterministic():
            ws = _lib.det_workspace(grad_out.device, (b, m, 3 * n))
            check(_lib.lib().pdgn_interpolation_backward_det(b, c, n, m, ptr(grad_out_data), ptr(idx), ptr(weight), ptr(ws),
                                                             ptr(grad_features), stream_of(grad_out_data)),
                  "pdgn_interpolation_backward_det")
            return grad_features, None, None
        check(_lib.lib().pdgn_interpolation_backward(b, c, n, m, ptr(grad_out_data), ptr(idx), ptr(weight),
                                                     ptr(grad_features), stream_of(grad_out_data)),
              "pdgn_interpolation_backward")
        return grad_features, None, None


interpolation = Interpolation.apply


# ------------------------------------------------------------------ pure-torch members of the API
def pairwise_distances(x, y=None):
    """pointops.py:346-365."""
    x_norm = (x ** 2).sum(1).view(-1, 1)
    if y is not None:
        y_t, y_norm = y.transpose(0, 1), (y ** 2).sum(1).view(1, -1)
    else:
        y_t, y_norm = x.transpose(0, 1), x_norm.view(1, -1)
    return torch.clamp(x_norm + y_norm - 2.0 * torch.mm(x, y_t), 0.0, np.inf)


def _naive_sorted_idx(xyz, new_xyz):
    if new_xyz is None:
        new_xyz = xyz
    dist = (new_xyz.unsqueeze(2) - xyz.unsqueeze(1)).pow(2).sum(dim=3)
    return torch.sort(dist, dim=2)[1]


def knnquery_naive(nsample, xyz, new_xyz=None):
    """pointops.py:368-405 (torch sort of the full distance matrix)."""
    return _naive_sorted_idx(xyz, new_xyz)[:, :, 0:nsample].int()


def knnquery_exclude(nsample, xyz, new_xyz=None):
    """pointops.py:437-474: ranks 1..nsample."""
    return _naive_sorted_idx(xyz, new_xyz)[:, :, 1:nsample + 1].int()


class Gathering(Function):
    """pointops.py:33-58.  features (b,c,n), idx (b,m) int32 -> (b,c,m); backward = scatter-add into (b,c,n)."""

    @staticmethod
    def forward(ctx, features, idx):
        require(features, "features", F32, 3)
        require(idx, "idx", I32, 2)
        b, c, n = features.shape
        m = idx.shape[1]
        out = torch.empty((b, c, m), dtype=F32, device=features.device)
        check(_lib.lib().pdgn_gathering_forward(b, c, n, m, ptr(features), ptr(idx), ptr(out), stream_of(features)),
              "pdgn_gathering_forward")
        ctx.for_backwards = (idx, c, n)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, c, n = ctx.for_backwards
        b, m = idx.shape
        grad_out = grad_out.contiguous()
        grad = torch.zeros((b, c, n), dtype=F32, device=grad_out.device)
        if _lib.deterministic():
            ws = _lib.det_workspace(grad_out.device, (b, n, m))
            check(_lib.lib().pdgn_gathering_backward_det(b, c, n, m, ptr(grad_out), ptr(idx), ptr(ws), ptr(grad),
                                                         stream_of(grad_out)), "pdgn_gathering_backward_det")
            return grad, None
        check(_lib.lib().pdgn_gathering_backward(b, c, n, m, ptr(grad_out), ptr(idx), ptr(grad), stream_of(grad_out)),
              "pdgn_gathering_backward")
        return grad, None


gathering = Gathering.apply
featuregather = Gathering.apply            # pointops.py:225-260: same contraction (max_feature (b,c,n), idx (b,m))


def grouping_int(features, idx):
    """pointops.py:154-173: int64 features (b,c,n), idx (b,m,ns) int32 -> (b,c,m,ns) int64."""
    require(features, "features", torch.int64, 3)
    require(idx, "idx", I32, 3)
    b, c, n = features.shape
    _, m, ns = idx.shape
    out = torch.empty((b, c, m, ns), dtype=torch.int64, device=features.device)
    check(_lib.lib().pdgn_grouping_int_forward(b, c, n, m, ns, ptr(features), ptr(idx), ptr(out), stream_of(features)),
          "pdgn_grouping_int_forward")
    return out


def ballquery(radius, nsample, xyz, new_xyz):
    """pointops.py:176-198 / ballquery_cuda_kernel.cu:47-80: the first <= nsample points with d2 < r^2 in index
    order, padded with the first hit (idx 0 when the ball is empty: the output starts zeroed, :190)."""
    require(xyz, "xyz", F32, 3)
    require(new_xyz, "new_xyz", F32, 3)
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx = torch.zeros((b, m, nsample), dtype=I32, device=xyz.device)
    check(_lib.lib().pdgn_ballquery(b, n, m, radius, int(nsample), ptr(new_xyz), ptr(xyz), ptr(idx), stream_of(xyz)), "pdgn_ballquery")
    return idx


def furthestsampling(xyz, m):
    """pointops.py:12-30 / sampling_cuda_kernel.cu:59-168: iterative farthest point sampling from point 0."""
    require(xyz, "xyz", F32, 3)
    b, n, _ = xyz.shape
    idx = torch.zeros((b, m), dtype=I32, device=xyz.device)
    temp = torch.full((b, n), 1e10, dtype=F32, device=xyz.device)
    check(_lib.lib().pdgn_furthestsampling(b, n, int(m), ptr(xyz), ptr(temp), ptr(idx), stream_of(xyz)),
          "pdgn_furthestsampling")
    return idx


FPS_MAX_N = 8192                                                 # PDGN_FPS_MAX_N (include/pdgn_hip.h)


def fps_order(xyz, m, start=None):
    """Farthest-point order of xyz (b,n,3), n <= FPS_MAX_N: (b,m) int32 with order[:,0] = start (default 0) and every later entry
    the point farthest from the ones before it, exact ties to the lowest index -- from start 0 index for index what
    `furthestsampling` returns, computed with the cloud in registers (csrc/fps.hip: the feeder's kernel).  start: None, an int or
    a (b,) integer tensor, every entry in [0, n) (checked here, on the host: the kernel is never handed another)."""
    require(xyz, "xyz", F32, 3)
    b, n, c = xyz.shape
    m = int(m)
    if c != 3:
        raise ValueError("xyz must be (b,n,3), got %s" % (tuple(xyz.shape),))
    if not 1 <= n <= FPS_MAX_N:
        raise ValueError("fps_order: n = %d, supported 1 .. %d (furthestsampling has no limit)" % (n, FPS_MAX_N))
    if not 1 <= m <= n:
        raise ValueError("fps_order: m = %d, need 1 <= m <= n = %d" % (m, n))
    if start is not None:
        if isinstance(start, torch.Tensor):
            if start.dtype.is_floating_point or start.dtype == torch.bool or tuple(start.shape) != (b,):
                raise ValueError("start: an int or a (b,) integer tensor")
            start = start.to(device=xyz.device, dtype=I32).contiguous()
        else:
            start = torch.full((b,), int(start), dtype=I32, device=xyz.device)
        if b and not (0 <= int(start.min()) and int(start.max()) < n):
            raise ValueError("start: every entry in [0, %d)" % n)
    order = torch.empty((b, m), dtype=I32, device=xyz.device)
    check(_lib.lib().pdgn_fps_order(b, n, m, ptr(xyz), ptr(start), ptr(order), stream_of(xyz)), "pdgn_fps_order")
    return order


def featuredistribute(max_xyz, xyz):
    """pointops.py:201-222: index of the nearest max_xyz (b,n,3) point for every xyz (b,m,3) point."""
    require(max_xyz, "max_xyz", F32, 3)
    require(xyz, "xyz", F32, 3)
    b, n, _ = max_xyz.shape
    m = xyz.shape[1]
    out = torch.empty((b, m), dtype=I32, device=xyz.device)
    check(_lib.lib().pdgn_featuredistribute(b, n, m, ptr(max_xyz), ptr(xyz), ptr(out), stream_of(xyz)),
          "pdgn_featuredistribute")
    return out


def labelstat_idx(nsample, label_stat, idx):
    """pointops.py:291-315: new_label_stat[b,j,:] = sum_s label_stat[b, idx[b,j,s], :] (int32)."""
    require(label_stat, "label_stat", I32, 3)
    require(idx, "idx", I32, 3)
    b, n, nclass = label_stat.shape
    m = idx.shape[1]
    out = torch.empty((b, m, nclass), dtype=I32, device=idx.device)
    check(_lib.lib().pdgn_labelstat_idx(b, n, m, int(nsample), nclass, ptr(label_stat), ptr(idx), ptr(out),
                                        stream_of(idx)), "pdgn_labelstat_idx")
    return out


def labelstat_ballrange(radius, xyz, new_xyz, label_stat):
    """pointops.py:263-288: label histogram over all points with d2 < r^2."""
    require(xyz, "xyz", F32, 3)
    require(new_xyz, "new_xyz", F32, 3)
    require(label_stat, "label_stat", I32, 3)
    b, n, nclass = label_stat.shape
    m = new_xyz.shape[1]
    out = torch.empty((b, m, nclass), dtype=I32, device=xyz.device)
    check(_lib.lib().pdgn_labelstat_ballrange(b, n, m, radius, nclass, ptr(new_xyz), ptr(xyz),
                                              ptr(label_stat), ptr(out), stream_of(xyz)), "pdgn_labelstat_ballrange")
    return out


def labelstat_and_ballquery(radius, nsample, xyz, new_xyz, label_stat):
    """pointops.py:318-343 -> (new_label_stat (b,m,nclass), idx (b,m,nsample)): ball query whose kept hits are also
    summed into the label histogram."""
    require(xyz, "xyz", F32, 3)
    require(new_xyz, "new_xyz", F32, 3)
    require(label_stat, "label_stat", I32, 3)
    b, n, nclass = label_stat.shape
    m = new_xyz.shape[1]
    out = torch.empty((b, m, nclass), dtype=I32, device=xyz.device)
    idx = torch.zeros((b, m, nsample), dtype=I32, device=xyz.device)
    check(_lib.lib().pdgn_labelstat_and_ballquery(b, n, m, radius, int(nsample), nclass, ptr(new_xyz),
                                                  ptr(xyz), ptr(label_stat), ptr(idx), ptr(out), stream_of(xyz)), "pdgn_labelstat_and_ballquery")
    return out, idx


# ------------------------------------------------------------------ grouping Modules
class _QueryBase(nn.Module):
    def __init__(self, radius=None, nsample=32, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def _query(self, xyz, new_xyz, nsample=None):
        nsample = self.nsample if nsample is None else nsample
        if self.radius is not None:
            return ballquery(self.radius, nsample, xyz, new_xyz)
        return knnquery(nsample, xyz, new_xyz)


class Gen_QueryAndGroupXYZ(_QueryBase):
    """pointops.py:670-703 -- the one PDGNet_v2 uses (models/PDGNet_v2.py:115):
    xyz (b,n,3), new_xyz (b,m,3) -> grouped xyz (b,3,m,nsample)."""

    def forward(self, xyz: torch.Tensor, new_xyz: torch.Tensor = None) -> torch.Tensor:
        if new_xyz is None:
            new_xyz = xyz
        idx = self._query(xyz, new_xyz)
        return grouping(xyz.transpose(1, 2).contiguous(), idx)


class QueryAndGroup(_QueryBase):
    """pointops.py:525-566."""
    _dilate = 1

    def forward(self, xyz, new_xyz=None, features=None, idx=None):
        if new_xyz is None:
            new_xyz = xyz
        if idx is None:
            idx = self._query(xyz, new_xyz, self._dilate * self.nsample)
            if self._dilate > 1:                              # QueryAndGroup_Dilate :593-596
                pick = np.random.permutation(self._dilate * self.nsample)[:self.nsample]
                idx = idx[:, :, torch.as_tensor(pick, device=idx.device)].contiguous()
        grouped_xyz = grouping(xyz.transpose(1, 2).contiguous(), idx)
        grouped_xyz = grouped_xyz - new_xyz.transpose(1, 2).unsqueeze(-1)
        if features is not None:
            grouped_features = grouping(features, idx)
            if self.use_xyz:
                return torch.cat([grouped_xyz, grouped_features], dim=1)
            return grouped_features
        assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
        return grouped_xyz


class QueryAndGroup_Dilate(QueryAndGroup):
    """pointops.py:568-615: query 2*nsample neighbours, keep a random half."""
    _dilate = 2


class Le_QueryAndGroup(_QueryBase):
    """pointops.py:617-668: returns (grouped_xyz - centre, grouped features)."""

    def forward(self, xyz, new_xyz=None, features=None, idx=None):
        if new_xyz is None:
            new_xyz = xyz
        if idx is None:
            idx = self._query(xyz, new_xyz)
        grouped_xyz = grouping(xyz.transpose(1, 2).contiguous(), idx)
        grouped_xyz = grouped_xyz - new_xyz.transpose(1, 2).unsqueeze(-1)
        if features is not None:
            return grouped_xyz, grouping(features, idx)
        assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
        return grouped_xyz, grouped_xyz


class Le_QueryAndGroup_SameSize(Le_QueryAndGroup):
    """pointops.py:476-522 (the reference dereferences new_xyz before its None check, :497-499;
    here the check comes first)."""

    def forward(self, xyz, new_xyz=None, features=None, idx=None):
        if new_xyz is None:
            new_xyz = xyz
        assert xyz.size() == new_xyz.size()
        return super().forward(xyz, new_xyz, features, idx)


class Le_QueryAndGroup_OnlyFeature(_QueryBase):
    """pointops.py:705-751."""

    def forward(self, xyz, new_xyz=None, features=None, idx=None):
        if new_xyz is None:
            new_xyz = xyz
        if idx is None:
            idx = self._query(xyz, new_xyz)
        assert features is not None, "Le_QueryAndGroup_OnlyFeature needs features"
        return grouping(features, idx)


class GroupAll(nn.Module):
    """pointops.py:753-777."""

    def __init__(self, use_xyz: bool = True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is not None:
            grouped_features = features.unsqueeze(2)
            if self.use_xyz:
                return torch.cat([grouped_xyz, grouped_features], dim=1)
            return grouped_features
        return grouped_xyz
