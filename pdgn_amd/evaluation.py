"""Evaluation metrics of PDGN's test phase (evaluation/evaluation_metrics.py:26-200) on the fused
MI355X kernels.

The reference loops over the samples in Python and, for each, expands it against every reference
batch before calling the CD / EMD extensions (``_pairwise_EMD_CD_`` :85-121; "may take about 2 hours",
README.md:47).  Here the (N_sample x N_ref) matrices are filled by the pair-list kernels
``pdgn_chamfer_gram_indexed`` / ``pdgn_emd_cost_indexed``: no expanded clouds, no (B,N,N) or (B,m,n)
temporaries, tens of thousands of pairs per launch.  MMD / COV / 1-NNA are the reference's small
torch reductions over those matrices.
"""

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from ._lib import check, ptr, require, stream_of

F32, I32 = torch.float32, torch.int32
_MAX_PAIRS = 32768          # per launch (grid.y limit of the Chamfer kernel, scratch of the EMD kernel)
_MAX_AUCTION_PAIRS = 2048   # per launch of the exact EMD: 8 workgroups per CU -- about a second at 2048 points, about 20 s if every pair runs to its cap


def _pair_lists(S, R, start, stop, device):
    p = torch.arange(start, stop, device=device, dtype=torch.int64)
    return (p // R).to(I32).contiguous(), (p % R).to(I32).contiguous()


def shard_pairs(total, fill, group=None):
    """Rows of the evaluation matrices are independent: rank r of the process group fills the
    r-th contiguous slice of the flat pair index space with `fill(start, stop) -> tuple of (stop-start,) tensors`, the
    slices are all-gathered (a few MB) and every rank returns the full-length tensors.  Every rank must call this with
    the same `total`; without a process group it is `fill(0, total)`."""
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    if world == 1:
        return tuple(fill(0, total))
    rank = dist.get_rank(group)
    chunk = -(-total // world)
    lo, hi = min(total, rank * chunk), min(total, (rank + 1) * chunk)
    full = []
    for t in fill(lo, hi):
        pad = t.new_zeros(chunk)
        pad[:hi - lo] = t
        parts = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(parts, pad, group=group)
        full.append(torch.cat(parts)[:total])
    return tuple(full)


EMD_KINDS = ("approx", "auction")


def _emd_kind(emd):
    if emd not in EMD_KINDS:
        raise ValueError("emd must be one of %s, got %r" % (EMD_KINDS, emd))
    return emd


def pairwise_emd_cd(sample_pcs, ref_pcs, batch_size=None, shard_over_ranks=False, group=None, emd="approx"):
    """_pairwise_EMD_CD_ (:85-121): all_cd, all_emd of shape (N_sample, N_ref).
    CD = mean_i min_j P + mean_j min_i P with the Gram-form P of distChamfer (:35-45);
    EMD = match_cost / N (:26-31).  `batch_size` is accepted for signature parity and ignored.
    shard_over_ranks: every rank of `group` holds the same two sets and computes 1/world of the pairs (`shard_pairs`).
    emd: "approx" -- the reference's approxmatch (pdgn_emd_cost_indexed), what published numbers use -- or "auction": the exact
    matching of equal-sized clouds (pdgn_auction_assign_indexed), its cost / N."""
    return _pairwise(sample_pcs, ref_pcs, True, shard_over_ranks, group, _emd_kind(emd))[:2]


def pairwise_cd(sample_pcs, ref_pcs, batch_size=None, shard_over_ranks=False, group=None):
    """The Chamfer half of `pairwise_emd_cd` alone: all_cd (N_sample, N_ref), the same launches in the same order and therefore
    the same bits; the EMD kernel is not launched (the cheap metrics of a training run's snapshot reports, pdgn_amd/report.py)."""
    return _pairwise(sample_pcs, ref_pcs, False, shard_over_ranks, group)[0]


def _pairwise(sample_pcs, ref_pcs, with_emd, shard_over_ranks, group, emd="approx"):
    require(sample_pcs, "sample_pcs", F32, 3)
    require(ref_pcs, "ref_pcs", F32, 3)
    S, N, _ = sample_pcs.shape
    R, M, _ = ref_pcs.shape
    dev = sample_pcs.device
    L = _lib.lib()
    auction = with_emd and emd == "auction"
    if auction and N != M:
        raise ValueError("emd=\"auction\" matches clouds of equal size (got %d and %d points)" % (N, M))

    def fill(lo, hi):
        cd = torch.empty(hi - lo, dtype=F32, device=dev)
        emd = torch.empty(hi - lo if with_emd else 0, dtype=F32, device=dev)
        status = torch.empty(hi - lo if auction else 0, dtype=I32, device=dev)
        for start in range(lo, hi, _MAX_PAIRS):
            stop = min(hi, start + _MAX_PAIRS)
            npairs = stop - start
            ia, ib = _pair_lists(S, R, start, stop, dev)
            minx = torch.empty((npairs, N), dtype=F32, device=dev)
            miny = torch.empty((npairs, M), dtype=F32, device=dev)
            argx = torch.empty((npairs, N), dtype=I32, device=dev)
            argy = torch.empty((npairs, M), dtype=I32, device=dev)
            check(L.pdgn_chamfer_gram_indexed(npairs, N, M, 3, ptr(sample_pcs), ptr(ia), ptr(ref_pcs), ptr(ib),
                                              ptr(minx), ptr(argx), ptr(miny), ptr(argy), stream_of(sample_pcs)),
                  "pdgn_chamfer_gram_indexed")
            # distChamfer returns (P.min(1), P.min(2)) = (per ref point, per sample point); :108 adds their means
            cd[start - lo:stop - lo] = miny.mean(dim=1) + minx.mean(dim=1)
            if not with_emd:
                continue
            if auction:
                out = torch.empty((npairs,), dtype=F32, device=dev)
                for first in range(0, npairs, _MAX_AUCTION_PAIRS):             # (a pair's result does not depend on the launch it is in)
                    count = min(npairs - first, _MAX_AUCTION_PAIRS)
                    check(L.pdgn_auction_assign_indexed(count, N, ptr(sample_pcs), ptr(ia[first:]), ptr(ref_pcs), ptr(ib[first:]), ptr(out[first:]),
                                                        ptr(status[start - lo + first:]), stream_of(sample_pcs)), "pdgn_auction_assign_indexed")
                emd[start - lo:stop - lo] = out / float(N)
                continue
            temp = torch.empty(L.pdgn_emd_cost_temp_floats(npairs, N, M), dtype=F32, device=dev)
            out = torch.empty((npairs,), dtype=F32, device=dev)
            check(L.pdgn_emd_cost_indexed(npairs, N, M, ptr(sample_pcs), ptr(ia), ptr(ref_pcs), ptr(ib), ptr(temp),
                                          ptr(out), stream_of(sample_pcs)), "pdgn_emd_cost_indexed")
            emd[start - lo:stop - lo] = out / float(N)
        return (cd, emd, status) if auction else (cd, emd) if with_emd else (cd,)

    out = shard_pairs(S * R, fill, group) if shard_over_ranks else fill(0, S * R)
    mats = tuple(t.view(S, R) for t in out[:2])
    return mats + (int((out[2] != 0).sum()) if auction else 0,) if with_emd else mats


def emd_cd(sample_pcs, ref_pcs, batch_size=None, reduced=True, emd="approx"):
    """EMD_CD (:48-82): paired (i, i) Chamfer and EMD (emd: as in `pairwise_emd_cd`)."""
    S = sample_pcs.shape[0]
    assert S == ref_pcs.shape[0], "REF:%d SMP:%d" % (ref_pcs.shape[0], S)
    from .losses import chamfer_min
    from .structural_losses import emd_cost, exact_emd_cost
    if _emd_kind(emd) == "auction":
        emd_cost = exact_emd_cost
    minx, miny = chamfer_min(sample_pcs.contiguous(), ref_pcs.contiguous())
    cd = miny.mean(dim=1) + minx.mean(dim=1)
    emd = emd_cost(sample_pcs.contiguous(), ref_pcs.contiguous()) / float(sample_pcs.shape[1])
    if reduced:
        cd, emd = cd.mean(), emd.mean()
    return {"MMD-CD": cd, "MMD-EMD": emd}


def lgan_mmd_cov(all_dist):
    """:157-169."""
    N_sample, N_ref = all_dist.size(0), all_dist.size(1)
    min_val_fromsmp, min_idx = torch.min(all_dist, dim=1)
    min_val, _ = torch.min(all_dist, dim=0)
    cov = torch.tensor(float(min_idx.unique().view(-1).size(0)) / float(N_ref)).to(all_dist)
    return {"lgan_mmd": min_val.mean(), "lgan_cov": cov, "lgan_mmd_smp": min_val_fromsmp.mean()}


def knn(Mxx, Mxy, Myy, k, sqrt=False):
    """1-NN two-sample test (:123-154)."""
    n0, n1 = Mxx.size(0), Myy.size(0)
    label = torch.cat((torch.ones(n0), torch.zeros(n1))).to(Mxx)
    M = torch.cat((torch.cat((Mxx, Mxy), 1), torch.cat((Mxy.transpose(0, 1), Myy), 1)), 0)
    if sqrt:
        M = M.abs().sqrt()
    inf_diag = torch.diag(float("inf") * torch.ones(n0 + n1).to(Mxx))
    _, idx = (M + inf_diag).topk(k, 0, False)
    count = torch.zeros(n0 + n1).to(Mxx)
    for i in range(k):
        count = count + label.index_select(0, idx[i])
    pred = torch.ge(count, (float(k) / 2) * torch.ones(n0 + n1).to(Mxx)).float()
    s = {"tp": (pred * label).sum(), "fp": (pred * (1 - label)).sum(),
         "fn": ((1 - pred) * label).sum(), "tn": ((1 - pred) * (1 - label)).sum()}
    s.update({"precision": s["tp"] / (s["tp"] + s["fp"] + 1e-10), "recall": s["tp"] / (s["tp"] + s["fn"] + 1e-10),
              "acc_t": s["tp"] / (s["tp"] + s["fn"] + 1e-10), "acc_f": s["tn"] / (s["tn"] + s["fp"] + 1e-10),
              "acc": torch.eq(label, pred).float().mean()})
    return s


def reduce_metrics(all_dist, Mxx, Mxy, Myy, tag="CD"):
    """The reduction stage of compute_all_metrics (:179-199) for ONE distance: MMD / COV from `all_dist` (the transposed
    sample-vs-reference matrix) and the 1-NN accuracies from the three matrices, under compute_all_metrics' keys
    ("lgan_mmd-<tag>", ..., "1-NN-<tag>-acc").  Small torch reductions on whatever device the matrices live on: no library call."""
    results = {"%s-%s" % (k, tag): v for k, v in lgan_mmd_cov(all_dist).items()}
    results.update({"1-NN-%s-%s" % (tag, k): v for k, v in knn(Mxx, Mxy, Myy, 1).items() if "acc" in k})
    return results


def compute_all_metrics(sample_pcs, ref_pcs, batch_size=None, accelerated_cd=False, shard_over_ranks=False, group=None, emd="approx"):
    """compute_all_metrics (:172-200): MMD / COV (CD and EMD) and 1-NNA from three all-pairs passes.
    shard_over_ranks: all ranks call with the same sets, each computes 1/world of every matrix (`shard_pairs`).
    emd: as in `pairwise_emd_cd`; under "auction" the dict has one more key, "emd-capped": the number of pairs, over the three
    matrices, whose auction did not end at an optimum (a tensor like the other entries)."""
    results = {}
    def matrices(a, b):                                          # (all_cd, all_emd, pairs not at an optimum: 0 under "approx")
        return _pairwise(a, b, True, shard_over_ranks, group, emd)

    _emd_kind(emd)
    M_rs_cd, M_rs_emd, c_rs = matrices(sample_pcs, ref_pcs)
    results.update({"%s-CD" % k: v for k, v in lgan_mmd_cov(M_rs_cd.t()).items()})
    results.update({"%s-EMD" % k: v for k, v in lgan_mmd_cov(M_rs_emd.t()).items()})
    M_rr_cd, M_rr_emd, c_rr = matrices(ref_pcs, ref_pcs)
    M_ss_cd, M_ss_emd, c_ss = matrices(sample_pcs, sample_pcs)
    results.update({"1-NN-CD-%s" % k: v for k, v in knn(M_rr_cd, M_rs_cd, M_ss_cd, 1).items() if "acc" in k})
    results.update({"1-NN-EMD-%s" % k: v for k, v in knn(M_rr_emd, M_rs_emd, M_ss_emd, 1).items() if "acc" in k})
    if emd == "auction":
        results["emd-capped"] = torch.tensor(float(c_rs + c_rr + c_ss)).to(M_rs_emd)
    return results


# ---------------------------------------------------------------------------- spacing (no reference counterpart)
@torch.no_grad()
def spacing_stats(clouds, batch=64):
    """How evenly the points of each cloud are spread, from the distance d_i of every point to the nearest OTHER point of its cloud
    (the all-pairs launch of losses.repulsion with no gradient: pdgn_repulsion, `batch` clouds per launch).  clouds (S,N,3), N >= 2 ->
    {"nn_mean": the mean over clouds of the per-cloud mean of d, "nn_cv": the mean over clouds of the per-cloud coefficient of variation
    std(d) / mean(d) (population std; 0.52 for a Poisson sample of a surface, towards 0 as the spacing evens out), "nn_min": the smallest
    d, "duplicates": the number of points with d == 0}, Python numbers.  The reductions are fp64 torch ops on the device."""
    from .losses import repulsion_pass
    require(clouds, "clouds", F32, 3)
    S, N, _ = clouds.shape
    if S < 1 or N < 2 or int(batch) < 1:
        raise ValueError("spacing_stats takes at least one cloud of at least two points and a positive batch, got %s, batch %r" % (tuple(clouds.shape), batch))
    nn2 = torch.cat([repulsion_pass(clouds[lo:lo + int(batch)], 1.0, grad=False, nn2=True)[3] for lo in range(0, S, int(batch))])
    d = nn2.double().sqrt()
    mean = d.mean(dim=1)
    return {"nn_mean": float(mean.mean()), "nn_cv": float((d.std(dim=1, unbiased=False) / mean).mean()), "nn_min": float(d.min()),
            "duplicates": int((nn2 == 0).sum())}


# ---------------------------------------------------------------------------- surface variation (no reference counterpart)
@torch.no_grad()
def surface_stats(clouds, k=16, batch=64):
    """How thin the sheet is that the points of each cloud lie on: the surface variation sigma_i = max(lambda0, 0) / (lambda0 + lambda1 +
    lambda2) of every point's k-neighbourhood covariance (Pauly et al. 2002; pointops.estimate_normals' eigenvalues, `batch` clouds per
    launch): 0 on a plane, up to 1/3 where the neighbourhood has no direction, and what noise ACROSS the surface raises.  clouds (S,N,3),
    N >= 2, k <= N -> {"sv_mean": the mean over clouds of the per-cloud mean of sigma, "sv_p90": the mean over clouds of the per-cloud
    90th percentile, "degenerate": the number of points left out of both -- zero trace (all k neighbours equal) or non-finite eigenvalues},
    Python numbers; a cloud with no point left counts 0 towards both means.  The reductions are fp64 torch ops on the device."""
    from .pointops import estimate_normals
    require(clouds, "clouds", F32, 3)
    S, N, _ = clouds.shape
    if S < 1 or N < 2 or int(batch) < 1:
        raise ValueError("surface_stats takes at least one cloud of at least two points and a positive batch, got %s, batch %r" % (tuple(clouds.shape), batch))
    eig = torch.cat([estimate_normals(clouds[lo:lo + int(batch)], k, return_eig=True)[1] for lo in range(0, S, int(batch))]).double()
    trace = (eig[..., 0] + eig[..., 1]) + eig[..., 2]
    live = torch.isfinite(trace) & (trace > 0)
    sigma = torch.where(live, eig[..., 0].clamp_min(0.0) / torch.where(live, trace, torch.ones_like(trace)), torch.full_like(trace, float("nan")))
    count = live.sum(dim=1)
    mean = torch.where(count > 0, torch.nan_to_num(sigma).sum(dim=1) / count.clamp_min(1), torch.zeros_like(trace[:, 0]))
    p90 = torch.nan_to_num(torch.nanquantile(sigma, 0.9, dim=1))
    return {"sv_mean": float(mean.mean()), "sv_p90": float(p90.mean()), "degenerate": int((~live).sum())}


# ---------------------------------------------------------------------------- distance to the surface (no reference counterpart)
def _distance_summary(d, prefix, out):
    """mean, RMS and max over dim 1 of distances d (B,n) fp64, NaN entries left out (NaN where a row has none)."""
    valid = ~torch.isnan(d)
    count = valid.sum(dim=1)
    z = torch.where(valid, d, torch.zeros_like(d))
    none = torch.full_like(z[:, 0], float("nan"))
    out[prefix + "_mean"] = torch.where(count > 0, z.sum(dim=1) / count.clamp_min(1), none)
    out[prefix + "_rms"] = torch.where(count > 0, ((z * z).sum(dim=1) / count.clamp_min(1)).sqrt(), none)
    out[prefix + "_max"] = torch.where(count > 0, torch.where(valid, d, torch.full_like(d, float("-inf"))).amax(dim=1), none)
    return valid, count


SURFACE_SAMPLE_SEED = 0x5F1D                                      # the seed of surface_fidelity's draw of the surface (draw 0)


@torch.no_grad()
def surface_fidelity(clouds, meshset, shape=None, samples=None, thresholds=(0.01, 0.02), visible_only=False, signed=False):
    """How well clouds (B,N,3) lie on, and cover, the surfaces of shape[c] of a meshes.MeshSet (PU-Net's P2F and the precision / recall of
    Tatarchenko et al. 2019).  A dict of (B) fp64 tensors on the clouds' device:
      accuracy_mean / _rms / _max      the distance (NOT squared) of the cloud's points to the surface (meshes.point_to_mesh: exact to the
                                       triangles, no sampling floor)
      completeness_mean / _rms / _max  the distance from `samples` points of the surface (MeshSet.sample, draw 0; default N) to the nearest
                                       point of the cloud (the nn_distance kernel)
      precision@t, recall@t, fscore@t  per threshold t: the share of the cloud's points within t of the surface, of the surface samples
                                       within t of the cloud, and their harmonic mean (0 where both are 0)
    and under "mean", a dict of the batch means of all of them as Python numbers.  Points that are not finite are left out of every
    statistic.  signed=True (shapes that `meshes.winding_report` calls closed) adds
      inside_fraction                  the share of the cloud's points whose winding number is at least one half
      signed_mean                      the mean of the distance, negated at those points: which side of the surface the cloud errs on
    after the other keys, which keep their values."""
    from .meshes import MeshSet, _shape_argument, _winding, point_to_mesh
    from .structural_losses import nn_distance
    if not isinstance(clouds, torch.Tensor) or clouds.dim() != 3 or clouds.shape[2] != 3 or clouds.dtype != F32:
        raise ValueError("surface_fidelity: clouds is a (B,N,3) float32 tensor")
    if not isinstance(meshset, MeshSet):
        raise ValueError("surface_fidelity: meshset is a MeshSet, got %s" % type(meshset).__name__)
    B, N, _ = clouds.shape
    samples = N if samples is None else int(samples)
    if samples < 1:
        raise ValueError("surface_fidelity: samples is a positive count, got %r" % (samples,))
    thresholds = tuple(float(t) for t in thresholds)
    if any(not (t > 0.0 and t < float("inf")) for t in thresholds):
        raise ValueError("surface_fidelity: thresholds are positive and finite, got %r" % (thresholds,))
    shape_h = _shape_argument(shape, B, meshset.S, "surface_fidelity")
    if visible_only and meshset.visible is None:
        raise ValueError("surface_fidelity: visible_only needs a mesh set built with visibility masks")
    out = {}
    d2, _ = point_to_mesh(clouds, meshset, shape_h, visible_only)
    acc = d2.double().sqrt()
    acc_valid, acc_count = _distance_summary(acc, "accuracy", out)
    surface = meshset.sample(samples, SURFACE_SAMPLE_SEED, 0)[torch.from_numpy(shape_h).to(clouds.device)].contiguous()
    finite = torch.isfinite(clouds).all(dim=2, keepdim=True)
    far = torch.where(finite, clouds, torch.full_like(clouds, 1e18)).contiguous()          # a point that is not finite is nobody's neighbour
    comp = nn_distance(surface, far)[0].double().sqrt()
    _distance_summary(comp, "completeness", out)
    for t in thresholds:
        precision = (acc_valid & (acc <= t)).sum(dim=1).double() / acc_count.clamp_min(1)
        recall = (comp <= t).sum(dim=1).double() / samples
        both = precision + recall
        out["precision@%g" % t], out["recall@%g" % t] = precision, recall
        out["fscore@%g" % t] = torch.where(both > 0, 2 * precision * recall / both.clamp_min(1e-300), torch.zeros_like(both))
    if signed:
        inside = (_winding(clouds, meshset, shape_h, visible_only, None, None, "surface_fidelity")[2] != 0) & acc_valid
        none = torch.full_like(acc[:, 0], float("nan"))
        out["inside_fraction"] = torch.where(acc_count > 0, inside.sum(dim=1).double() / acc_count.clamp_min(1), none)
        z = torch.where(acc_valid, torch.where(inside, -acc, acc), torch.zeros_like(acc))
        out["signed_mean"] = torch.where(acc_count > 0, z.sum(dim=1) / acc_count.clamp_min(1), none)
    out["mean"] = {k: float(torch.nanmean(v)) for k, v in out.items()}
    return out


# ---------------------------------------------------------------------------- volume overlap (no reference counterpart)
@torch.no_grad()
def volume_iou(meshset_a, meshset_b, shape_a=None, shape_b=None, resolution=64, bounds=None):
    """Volumetric intersection over union of shape_a[c] of one meshes.MeshSet and shape_b[c] of another (None: all of a set's shapes, in
    order): both occupancies (meshes.occupancy_grid: the winding number at the cell centres) on ONE grid of `resolution` cells per axis
    per pair -- bounds = (lo, hi) as for occupancy_grid, or None: the union of the two shapes' boxes, grown by 5 % of its longest side
    and made cubic.  -> {"iou" (B) fp64 = intersection / union (NaN where the union is empty), "intersection", "union", "count_a",
    "count_b" (B) int64: counts of cells}, on the sets' device.  A ratio of integer counts: nothing in it depends on an order."""
    from .meshes import MeshSet, _occupancy, _resolution_argument, _shape_list, bounds_grid, cubic_grid, shape_boxes
    if not isinstance(meshset_a, MeshSet) or not isinstance(meshset_b, MeshSet):
        raise ValueError("volume_iou: both sets are MeshSets, got %s and %s" % (type(meshset_a).__name__, type(meshset_b).__name__))
    R = _resolution_argument(resolution, "volume_iou")
    sa, sb = _shape_list(shape_a, meshset_a.S, "volume_iou"), _shape_list(shape_b, meshset_b.S, "volume_iou")
    if sa.shape[0] != sb.shape[0] or sa.shape[0] < 1:
        raise ValueError("volume_iou: %d shapes against %d -- the pairs are shape_a[c] with shape_b[c]" % (sa.shape[0], sb.shape[0]))
    if meshset_a.verts.device != meshset_b.verts.device:
        raise ValueError("volume_iou: the sets are on %s and %s" % (meshset_a.verts.device, meshset_b.verts.device))
    if bounds is None:
        (alo, ahi), (blo, bhi) = shape_boxes(meshset_a, sa), shape_boxes(meshset_b, sb)
        origin, voxel = cubic_grid(np.minimum(alo, blo), np.maximum(ahi, bhi), R, 0.05)
    else:
        origin, voxel = bounds_grid(bounds, sa.shape[0], R)
    a, b = _occupancy(meshset_a, sa, R, origin, voxel).flatten(1), _occupancy(meshset_b, sb, R, origin, voxel).flatten(1)
    inter, union = (a & b).sum(dim=1), (a | b).sum(dim=1)
    iou = torch.where(union > 0, inter.double() / union.clamp_min(1).double(), torch.full_like(inter, float("nan"), dtype=torch.float64))
    return {"iou": iou, "intersection": inter, "union": union, "count_a": a.sum(dim=1), "count_b": b.sum(dim=1)}


# ---------------------------------------------------------------------------- JSD (evaluation_metrics.py:206-321)
def unit_cube_grid_point_cloud(resolution, clip_sphere=False, device="cpu"):
    """Cell centres of a resolution^3 grid over the unit cube (:206-224); clip_sphere keeps |c| <= 0.5."""
    spacing = 1.0 / float(resolution - 1)
    ax = torch.arange(resolution, dtype=F32, device=device) * spacing - 0.5
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1)
    if clip_sphere:
        grid = grid.reshape(-1, 3)
        grid = grid[grid.double().norm(dim=1) <= 0.5]
    return grid, spacing


def occupancy_grid_counters(pclouds, grid_resolution, in_sphere=False):
    """grid_counters and per-cell Bernoulli counts of entropy_of_occupancy_grid (:242-283): every point votes for
    its nearest grid cell.  The reference loops over clouds with sklearn's NearestNeighbors; here ALL points go
    through one brute-force 1-NN launch (pdgn_knnquery) and two bincounts."""
    from . import pointops
    require(pclouds, "pclouds", F32, 3)
    S, N, _ = pclouds.shape
    grid, _ = unit_cube_grid_point_cloud(grid_resolution, in_sphere, device=pclouds.device)
    grid = grid.reshape(1, -1, 3).contiguous()
    G = grid.shape[1]
    idx = pointops.knnquery(1, grid, pclouds.reshape(1, S * N, 3).contiguous()).view(S, N).long()
    counters = torch.bincount(idx.reshape(-1), minlength=G).double()
    cloud = torch.arange(S, device=pclouds.device).view(S, 1).expand(S, N)
    pairs = torch.unique(cloud.reshape(-1) * G + idx.reshape(-1))          # one vote per (cloud, cell)
    bernoulli = torch.bincount(pairs % G, minlength=G).double()
    return counters, bernoulli


def _entropy(p, base=None):
    p = p / p.sum()
    nz = p > 0
    h = -(p[nz] * torch.log(p[nz])).sum()
    return h / torch.log(torch.tensor(float(base), dtype=p.dtype, device=p.device)) if base else h


def entropy_of_occupancy_grid(pclouds, grid_resolution, in_sphere=False):
    """:242-283 -> (mean Bernoulli entropy per cell, grid_counters)."""
    counters, bern = occupancy_grid_counters(pclouds, grid_resolution, in_sphere)
    p = bern[bern > 0] / float(pclouds.shape[0])
    q = 1.0 - p
    h = -(p * torch.log(p)).sum() - (q[q > 0] * torch.log(q[q > 0])).sum()
    return h / counters.numel(), counters


def jensen_shannon_divergence(P, Q):
    """:286-305 (base-2 entropies)."""
    if bool((P < 0).any()) or bool((Q < 0).any()):
        raise ValueError("Negative values.")
    if P.numel() != Q.numel():
        raise ValueError("Non equal size.")
    P_, Q_ = P / P.sum(), Q / Q.sum()
    return _entropy((P_ + Q_) / 2.0, 2) - (_entropy(P_, 2) + _entropy(Q_, 2)) / 2.0


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, resolution=28):
    """:227-239: JSD between the occupancy distributions of two sets of clouds (unit-sphere grid)."""
    s = entropy_of_occupancy_grid(sample_pcs, resolution, True)[1]
    r = entropy_of_occupancy_grid(ref_pcs, resolution, True)[1]
    return jensen_shannon_divergence(s, r)


# ---------------------------------------------------------------------------- the test phase (models/PDGNet_v2.py:296-331)
@torch.no_grad()
def generate_clouds(generator, n, batch_size, normalize=None, rng=None, device=None):
    """The generation of PDGNet_v2.test (:300-312): ceil(n / batch_size) batches of z ~ N(0, 1) from `rng`, the finest cloud of
    each, truncated to n -> (clouds normalised with `normalize`, clouds as generated), both (n, N, 3)."""
    from .data import normalize_point_clouds
    dev = device if device is not None else next(generator.parameters()).device
    gen = []
    for _ in range((n + batch_size - 1) // batch_size):
        z = torch.randn(batch_size, 128, generator=rng, device=dev if rng is None or rng.device.type != "cpu" else "cpu").to(dev)
        gen.append(generator(z)[3].transpose(2, 1).contiguous())
    raw = torch.cat(gen, dim=0)[:n].contiguous()
    return normalize_point_clouds(raw, normalize), raw


@torch.no_grad()
def generate_and_evaluate(generator, ref_pcs, batch_size, normalize=None, rng=None, with_jsd=True, return_raw=False, emd="approx"):
    """PDGNet_v2.test: draw ceil(N_ref / batch_size) batches of z ~ N(0, 1) (:304 -- sigma 1, unlike training's
    0.2), keep the finest cloud of each, truncate to N_ref, normalise like the reference set (`normalize` =
    the data set's scale mode: shape_unit / shape_bbox / None), then compute_all_metrics (+ 'jsd').
    Returns (generated clouds (N_ref, N, 3), results dict of floats-on-device); with return_raw also, third, the clouds as
    generated, before the normalisation (the reference's `nonormal_out.npy`, :309).  emd: as in `compute_all_metrics`."""
    gen_pcs, raw = generate_clouds(generator, ref_pcs.shape[0], batch_size, normalize, rng, ref_pcs.device)
    results = compute_all_metrics(gen_pcs, ref_pcs, batch_size, emd=emd)
    if with_jsd:
        results["jsd"] = jsd_between_point_cloud_sets(gen_pcs, ref_pcs)
    return (gen_pcs, results, raw) if return_raw else (gen_pcs, results)
