"""From an oriented point cloud back to a triangle mesh, on the device (csrc/reconstruct.hip; no reference
counterpart): an implicit-moving-least-squares signed-distance field on a regular grid (pdgn_imls_grid), then its iso-surface by surface
nets (pdgn_surface_nets_count, an exclusive scan by torch.cumsum, pdgn_surface_nets_emit) -- the rest of Hoppe et al.'s pipeline after
pointops.estimate_normals and pointops.orient_normals.

    verts, faces, vert_off, face_off, stats = reconstruct(xyz)                     # normals estimated and oriented first
    report = mesh_report(verts[vert_off[0]:vert_off[1]], faces[face_off[0]:face_off[1]])
    clouds = to_meshset(verts, faces, vert_off, face_off).to(device).sample(2048, seed=0)

Nothing here is differentiable.  `mesh_report` is host numpy."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require, stream_of

F32, I32 = torch.float32, torch.int32
MIN_RESOLUTION, MAX_RESOLUTION = 2, 256                            # PDGN_RECON_MIN_R, PDGN_RECON_MAX_R
VISIBLE_DISC_OF_SUPPORT = 0.4                                      # orient="visible" with a given support h: the disc's radius is 0.4 h (2 of the default 5 spacings)


def _clouds(xyz, name="xyz"):
    require(xyz, name, F32, 3)
    if xyz.shape[2] != 3 or xyz.shape[0] < 1 or xyz.shape[1] < 1:
        raise ValueError("%s must be (B,N,3) with B, N >= 1, got %s" % (name, tuple(xyz.shape)))
    return xyz


def _resolution(resolution, b):
    R = int(resolution)
    if not MIN_RESOLUTION <= R <= MAX_RESOLUTION or b * R ** 3 >= 2 ** 31:
        raise ValueError("resolution %r: between %d and %d nodes per axis, B R^3 below 2^31 (B = %d)" % (resolution, MIN_RESOLUTION, MAX_RESOLUTION, b))
    return R


@torch.no_grad()
def mean_spacing(xyz):
    """(B) fp64: every cloud's mean distance to the nearest other point (the all-pairs launch of evaluation.spacing_stats, pdgn_repulsion's
    nn2 output); points with a non-finite distance are left out."""
    from .losses import repulsion_pass
    nn2 = torch.cat([repulsion_pass(xyz[lo:lo + 64], 1.0, grad=False, nn2=True)[3] for lo in range(0, xyz.shape[0], 64)])
    d = nn2.double().sqrt()
    ok = torch.isfinite(d)
    return torch.where(ok, d, torch.zeros_like(d)).sum(dim=1) / ok.sum(dim=1).clamp_min(1)


@torch.no_grad()
def grid_for(xyz, resolution, radius):
    """The grid of every cloud: the cube around its bounding box's centre with half-side (largest half-extent + h), R = resolution nodes
    per axis.  xyz (B,N,3); radius: h as a number or a (B) tensor -> origin (B,3), voxel (B), inv = 1 / h^2 (B), computed in fp64 torch
    ops and rounded once: the fp32 values pdgn_imls_grid takes.  Points with a non-finite coordinate do not count towards the box."""
    _clouds(xyz)
    b = xyz.shape[0]
    R = _resolution(resolution, b)
    h = torch.as_tensor(radius, dtype=torch.float64, device=xyz.device).expand(b)
    x = xyz.double()
    ok = torch.isfinite(x).all(dim=2, keepdim=True)
    lo = torch.where(ok, x, torch.full_like(x, float("inf"))).amin(dim=1)
    hi = torch.where(ok, x, torch.full_like(x, float("-inf"))).amax(dim=1)
    half = ((hi - lo) / 2).amax(dim=1) + h
    origin = (lo + hi) / 2 - half[:, None]
    return origin.float().contiguous(), (2.0 * half / (R - 1)).float().contiguous(), (1.0 / (h * h)).float().contiguous()


@torch.no_grad()
def imls_grid(xyz, normals, origin, voxel, inv, resolution, cull=True):
    """pdgn_imls_grid on explicit grids: xyz, normals (B,N,3), origin (B,3), voxel (B), inv (B) fp32 on the device -> field (B,R,R,R); a
    node with no point within h is NaN.  cull=False visits every point at every node instead of leaving out, per brick of nodes, those
    that cannot reach it (measurement and tests: the results are the same bit for bit)."""
    _clouds(xyz)
    _clouds(normals, "normals")
    b, n, _ = xyz.shape
    R = _resolution(resolution, b)
    if normals.shape != xyz.shape or normals.device != xyz.device:
        raise ValueError("normals must be (B,N,3) on xyz's device, got %s for xyz %s" % (tuple(normals.shape), tuple(xyz.shape)))
    grid = torch.cat([origin.reshape(b, 3), voxel.reshape(b, 1), inv.reshape(b, 1)], dim=1).to(device=xyz.device, dtype=F32).contiguous()
    host = grid.cpu().numpy()                                       # the copy the entry point checks on the host
    if not (np.isfinite(host).all() and (host[:, 3:] > 0).all()):
        raise ValueError("imls_grid: origin, voxel and inv must be finite, voxel and inv positive")
    field = torch.empty((b, R, R, R), dtype=F32, device=xyz.device)
    check(_lib.lib().pdgn_imls_grid(b, n, R, ptr(xyz), ptr(normals), ptr(grid), host.ctypes.data_as(ctypes.c_void_p), 1 if cull else 0,
                                    ptr(field), stream_of(xyz)), "pdgn_imls_grid")
    return field


@torch.no_grad()
def imls_field(xyz, normals, resolution=64, radius=None, radius_factor=5.0):
    """The signed-distance field of oriented clouds: xyz, normals (B,N,3) -> (field (B,R,R,R), origin (B,3), voxel (B)).  radius: the
    support h of the weight (1 - d^2 / h^2)^2, a number or (B); None: per cloud, radius_factor times its mean nearest-neighbour distance
    (clouds of at most 8192 points then).  Negative inside, NaN where no point is within h."""
    _clouds(xyz)
    if radius is None:
        if not float(radius_factor) > 0:
            raise ValueError("radius_factor must be positive, got %r" % (radius_factor,))
        radius = float(radius_factor) * mean_spacing(xyz)
    origin, voxel, inv = grid_for(xyz, resolution, radius)
    return imls_grid(xyz, normals, origin, voxel, inv, resolution), origin, voxel


@torch.no_grad()
def surface_nets(field, origin, voxel):
    """The iso-surface f = 0 of field (B,R,R,R) (NaN: no data; f < 0: inside) on the grids origin (B,3), voxel (B): one vertex per cell
    the surface crosses, one quad (two triangles, counter-clockwise seen from outside) per grid edge it crosses.
    -> verts (V,3) fp32, faces (F,3) int32 LOCAL to their cloud, vert_off (B+1) int32, face_off (B+1) int32, stats (B,4) int32: vertices,
    faces, open edges (a crossed edge with a cell around it outside the grid or without data), invalid nodes; concatenated over the
    batch, vertices by ascending cell, faces by ascending (node, axis)."""
    require(field, "field", F32, 4)
    b, R = field.shape[0], field.shape[1]
    if b < 1 or tuple(field.shape[1:]) != (R, R, R):
        raise ValueError("field must be (B,R,R,R), got %s" % (tuple(field.shape),))
    _resolution(R, b)
    dev = field.device
    grid = torch.cat([origin.reshape(b, 3), voxel.reshape(b, 1)], dim=1).to(device=dev, dtype=F32).contiguous()
    host = grid.cpu().numpy()
    if not (np.isfinite(host).all() and (host[:, 3] > 0).all()):
        raise ValueError("surface_nets: origin and voxel must be finite, voxel positive")
    L = _lib.lib()
    nodes = R ** 3
    vflag = torch.empty((b, nodes), dtype=I32, device=dev)
    qcnt = torch.empty((b, nodes), dtype=I32, device=dev)
    stats = torch.empty((b, 4), dtype=I32, device=dev)
    check(L.pdgn_surface_nets_count(b, R, ptr(field), ptr(vflag), ptr(qcnt), ptr(stats), stream_of(field)), "pdgn_surface_nets_count")
    vscan = torch.cumsum(vflag, dim=1, dtype=I32)                   # inclusive, per cloud
    qscan = torch.cumsum(qcnt, dim=1, dtype=I32)
    counts = stats.cpu()
    zero = torch.zeros(1, dtype=torch.int64)
    vert_off = torch.cat([zero, counts[:, 0].long().cumsum(0)])
    face_off = torch.cat([zero, counts[:, 1].long().cumsum(0)])
    V, Fc = int(vert_off[-1]), int(face_off[-1])
    if max(V, Fc) > (2 ** 31 - 1) // 3:
        raise ValueError("surface_nets: %d vertices and %d faces, beyond what 32-bit offsets hold" % (V, Fc))
    vert_off, face_off = vert_off.to(I32).to(dev), face_off.to(I32).to(dev)
    verts = torch.empty((V, 3), dtype=F32, device=dev)
    faces = torch.empty((Fc, 3), dtype=I32, device=dev)
    check(L.pdgn_surface_nets_emit(b, R, ptr(field), ptr(grid), host.ctypes.data_as(ctypes.c_void_p), ptr(vflag), ptr(vscan), ptr(qcnt),
                                   ptr(qscan), ptr(vert_off), ptr(face_off), V, Fc, V, Fc, ptr(verts) if V else None,
                                   ptr(faces) if Fc else None, stream_of(field)), "pdgn_surface_nets_emit")
    return verts, faces, vert_off, face_off, stats


@torch.no_grad()
def reconstruct(xyz, normals=None, k=16, resolution=64, radius=None, radius_factor=5.0, orient="consistent"):
    """Clouds to meshes: xyz (B,N,3) -> surface_nets' five results.  normals: oriented normals (B,N,3); None: knnquery(k),
    estimate_normals and, by `orient`, "consistent": orient_normals (clouds of at most 4096 points, k at most 64, then) or "visible":
    orient_normals_visible at its defaults (k at most 64; no limit on the points where `radius` is given, and where it is given the
    discs of the depth pass take 0.4 of it: two of the five spacings the default support spans)."""
    _clouds(xyz)
    if orient not in ("consistent", "visible"):
        raise ValueError("reconstruct: orient is \"consistent\" or \"visible\", got %r" % (orient,))
    if normals is None:
        from .pointops import estimate_normals, knnquery, orient_normals, orient_normals_visible
        if not 1 <= int(k) <= xyz.shape[1]:
            raise ValueError("reconstruct: k = %r neighbours of a cloud of %d points" % (k, xyz.shape[1]))
        idx = knnquery(int(k), xyz, xyz)
        if orient == "visible":
            disc = None if radius is None else torch.as_tensor(radius, dtype=torch.float64, device=xyz.device) * VISIBLE_DISC_OF_SUPPORT
            normals = orient_normals_visible(xyz, estimate_normals(xyz, idx=idx), idx=idx, radius=disc)
        else:
            normals = orient_normals(xyz, estimate_normals(xyz, idx=idx), idx=idx)
    field, origin, voxel = imls_field(xyz, normals, resolution, radius, radius_factor)
    return surface_nets(field, origin, voxel)


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def mesh_report(verts, faces, components=True):
    """What kind of surface a triangle list is (host numpy): verts (V,3), faces (F,3) -> {"vertices", "faces", "edges", "boundary_edges"
    (used by one triangle), "nonmanifold_edges" (by more than two), "oriented" (every interior edge is used once in each direction),
    "components" (of the vertices that faces use), "euler" (V - E + F over the used vertices), "area", "volume" (signed: positive where
    the triangles are counter-clockwise seen from outside)}.  components=False leaves that
    count out (None): it is a union-find in a Python loop over the edges, the one slow part."""
    v = _host(verts).astype(np.float64).reshape(-1, 3)
    f = _host(faces).astype(np.int64).reshape(-1, 3)
    if f.shape[0] and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("mesh_report: a face names a vertex outside the %d vertices" % v.shape[0])
    used = np.unique(f)
    half = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    lo, hi = half.min(axis=1), half.max(axis=1)
    key = lo * max(v.shape[0], 1) + hi
    uniq, inv, count = np.unique(key, return_inverse=True, return_counts=True)
    forward = np.bincount(inv, weights=(half[:, 0] < half[:, 1]), minlength=uniq.size)
    interior = count == 2
    root = np.arange(v.shape[0])

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a
    for a, b in zip((uniq // max(v.shape[0], 1)).tolist(), (uniq % max(v.shape[0], 1)).tolist()) if components else ():
        ra, rb = find(a), find(b)
        if ra != rb:
            root[ra] = rb
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return {"vertices": int(used.size), "faces": int(f.shape[0]), "edges": int(uniq.size),
            "boundary_edges": int((count == 1).sum()), "nonmanifold_edges": int((count > 2).sum()),
            "oriented": bool((forward[interior] == 1).all()),
            "components": len({find(i) for i in used.tolist()}) if components else None,
            "euler": int(used.size - uniq.size + f.shape[0]),
            "area": float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()),
            "volume": float((a * np.cross(b, c)).sum() / 6.0)}


def to_meshset(verts, faces, vert_off, face_off, normalize=None):
    """surface_nets' result as a meshes.MeshSet (on the host; `.to(device)` moves it): faces become global vertex indices, which is what
    MeshSet.from_arrays takes.  A cloud without a face of positive area is a ValueError there."""
    from .meshes import MeshSet
    f = _host(faces).astype(np.int64).reshape(-1, 3)
    voff, foff = _host(vert_off).astype(np.int64), _host(face_off).astype(np.int64)
    return MeshSet.from_arrays(_host(verts), f + np.repeat(voff[:-1], np.diff(foff))[:, None], foff, normalize)


MESH_ERROR_SEED = 0x3E5E                                          # the seed of mesh_error's two draws (draw 0 of each set)


@torch.no_grad()
def mesh_error(verts, faces, vert_off, face_off, meshset, shape=None, samples=4096, signed=False, iou_resolution=64):
    """The two-sided sampled distance between reconstructed meshes (surface_nets' verts, faces, vert_off, face_off: B meshes) and the
    surfaces they came from (shape[c] of `meshset`, on the device; None: mesh c against shape c): `samples` points of each surface are
    measured against the other (MeshSet.sample, then meshes.point_to_mesh).  -> a dict of (B) fp64 tensors, distances (not squared):
    to_reference_mean / _rms / _max (from the reconstruction to the reference surface) and to_reconstruction_mean / _rms / _max.
    signed=True (the reference shapes closed and consistently oriented) adds to_reference_signed_mean -- the same
    distances as to_reference_mean, negated where the sample lies inside the reference: positive means the reconstruction lies outside
    -- and iou, evaluation.volume_iou of the two on iou_resolution cells per axis."""
    from .evaluation import _distance_summary, volume_iou
    from .meshes import MeshSet, _shape_argument, _winding, point_to_mesh
    if not isinstance(meshset, MeshSet):
        raise ValueError("mesh_error: meshset is a MeshSet, got %s" % type(meshset).__name__)
    B = int(_host(face_off).shape[0]) - 1
    if B < 1 or int(_host(vert_off).shape[0]) != B + 1:
        raise ValueError("mesh_error: vert_off and face_off are (B+1) prefix sums over at least one mesh")
    if int(samples) < 1:
        raise ValueError("mesh_error: samples is a positive count, got %r" % (samples,))
    shape_h = _shape_argument(shape, B, meshset.S, "mesh_error")
    dev = meshset.verts.device
    ours = to_meshset(verts, faces, vert_off, face_off).to(dev)
    out = {}
    mine = ours.sample(int(samples), MESH_ERROR_SEED, 0)
    to_reference = point_to_mesh(mine, meshset, shape_h)[0].double().sqrt()
    _distance_summary(to_reference, "to_reference", out)
    theirs = meshset.sample(int(samples), MESH_ERROR_SEED, 0)[torch.from_numpy(shape_h).to(dev)].contiguous()
    _distance_summary(point_to_mesh(theirs, ours)[0].double().sqrt(), "to_reconstruction", out)
    if signed:
        inside = _winding(mine, meshset, shape_h, False, None, None, "mesh_error")[2] != 0
        _distance_summary(torch.where(inside, -to_reference, to_reference), "to_reference_signed", out)
        del out["to_reference_signed_rms"], out["to_reference_signed_max"]
        out["iou"] = volume_iou(ours, meshset, None, shape_h, iou_resolution)["iou"]
    return out
