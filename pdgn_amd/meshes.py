"""Triangle meshes as training data: the form ShapeNetCore is distributed in, resident on the device, so that every visit of a shape
is a fresh i.i.d. sample of its surface (data.MeshFeeder -> csrc/feed.hip: pdgn_feed_batch_mesh).

`load_obj` reads the geometry of a Wavefront .obj; `MeshSet` holds a set of shapes as the four arrays the kernels take -- vertices,
global faces, the shapes' face ranges and one alias table (Walker 1977 / Vose 1991) per shape, which picks a face with probability
proportional to its area from one 8-byte load -- normalised in closed form over the SURFACE; `MeshSet.sample` draws held-out clouds
(pdgn_sample_surface).  `python -m pdgn_amd.meshes pack DIR OUT.npz` packs a directory <synsetid>/<split>/*.obj into one file.

Visible-surface sampling: `face_visibility` asks the device which faces some view of a ring can see
(csrc/visible.hip: pdgn_mesh_visibility); a `MeshSet` built with `visible=mask` gives the others weight zero wherever the area is used,
so they are never drawn.  `pack --visible` stores the masks beside the meshes.

Face orientation: `face_orientation` asks the same depth pass which SIDE of every face the views see
(pdgn_mesh_face_votes); a face seen mostly from its back is stored the wrong way round.  A `MeshSet` carries the answer as `flip`,
`MeshSet.oriented()` applies it, and the signed quantities below then mean something on raw CAD meshes.  `pack --orient` stores the flips.

Distances and sides (DESIGN.md sections 7t and 7u): `point_to_mesh` is the closest point of a shape's faces (csrc/meshdist.hip),
`winding_number` the generalized winding number about them (csrc/winding.hip) -- 1 inside a closed, consistently oriented shape, 0
outside -- and on the two `signed_distance`, `occupancy_grid` and `winding_report`; the commands `distance`, `occupancy` and `check`.

Looking at a set: the command `render` draws its shapes as shaded triangles into a preview sheet
(report.MeshColumn, csrc/render.hip: pdgn_render_sheet_mesh), with --visible only the faces the sampler would draw from.
"""
import os
import sys

import numpy as np

NORMALIZE = (None, "shape_unit", "shape_bbox")
SPLITS = ("train", "val", "test")


def load_obj(path):
    """(verts float32 (V,3), faces int32 (F,3)) of a Wavefront .obj: `v` and `f` lines only; `f a/b/c` and `f a//c` forms (the vertex
    index is the first field), negative indices (relative to the vertices read so far), polygons as triangle fans; everything else
    (vn, vt, g, usemtl, comments, ...) is ignored.  An index outside the file's vertices is a ValueError."""
    verts, faces, where = [], [], []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError("%s:%d: a vertex has three coordinates" % (path, ln))
                verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
            elif tok[0] == "f":
                idx = []
                for field in tok[1:]:
                    i = int(field.split("/", 1)[0])
                    if i == 0 or -i > len(verts):
                        raise ValueError("%s:%d: vertex index %d of %d vertices read so far" % (path, ln, i, len(verts)))
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                if len(idx) < 3:
                    raise ValueError("%s:%d: a face has at least three vertices" % (path, ln))
                for k in range(1, len(idx) - 1):
                    faces.append((idx[0], idx[k], idx[k + 1]))
                    where.append(ln)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if faces.size and faces.max() >= len(verts):
        bad = int(np.argmax(faces.max(axis=1) >= len(verts)))
        raise ValueError("%s:%d: vertex index %d, the file has %d vertices" % (path, where[bad], int(faces[bad].max()) + 1, len(verts)))
    return np.asarray(verts, dtype=np.float32).reshape(-1, 3), faces.astype(np.int32)


def face_areas(verts, faces):
    """Triangle areas in fp64."""
    v = np.asarray(verts, dtype=np.float64)
    v0, v1, v2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return 0.5 * np.linalg.norm(np.cross(v1 - v0, v2 - v0), axis=1)


def alias_table(area):
    """Vose's alias method in fp64 for one shape: (threshold uint32 (F), alias uint32 (F)).  A draw takes a slot s uniformly and a word
    w uniformly in [0, 2^32): face s where w < threshold[s], else face alias[s]; so face f has probability
    (threshold[f] + sum over slots g with alias[g] = f of (2^32 - threshold[g])) / (F 2^32), area[f] / sum(area) up to the rounding of the
    thresholds to 32 bits (2 * 2^-32 over all faces together).  A face of area zero has threshold 0 and is nobody's alias: never drawn.
    A slot that keeps every draw has threshold 2^32 - 1 and is its own alias."""
    area = np.asarray(area, dtype=np.float64)
    F = area.shape[0]
    total = float(area.sum())
    if not (F >= 1 and np.all(area >= 0.0) and np.isfinite(total) and total > 0.0):
        raise ValueError("alias_table: areas must be finite, not negative and not all zero")
    p = (area * (F / total)).tolist()
    prob, alias = [1.0] * F, list(range(F))
    small = sorted((i for i in range(F) if p[i] < 1.0), key=lambda i: p[i] == 0.0)       # (popped from the end: the empty faces first)
    large = [i for i in range(F) if p[i] >= 1.0]
    while small and large:
        s, l = small.pop(), large[-1]
        prob[s], alias[s] = p[s], l
        p[l] = (p[l] + p[s]) - 1.0
        if p[l] < 1.0:
            small.append(large.pop())
    for s in small:                                              # (rounding left them just below one: they keep every draw)
        assert area[s] > 0.0
    thr = np.minimum(np.floor(np.asarray(prob) * 4294967296.0 + 0.5), 4294967295.0).astype(np.uint32)
    return thr, np.asarray(alias, dtype=np.uint32)


def _per_shape(values, face_off):
    """Sums of per-face rows over every shape's face range."""
    return np.add.reduceat(values, face_off[:-1], axis=0)


def surface_statistics(verts, faces, face_off, area=None):
    """Per shape, over its SURFACE (uniform density on the faces, in fp64): (centroid (S,3), std (S)) -- the limits, for infinitely many
    surface samples, of the per-axis mean and of the standard deviation of all coordinates pooled about their pooled mean, which is
    what data.normalize_clouds(., "shape_unit") takes as shift and scale.  Triangle moments: E[x] = s / 3, E[x x^T] = (sum_i v_i v_i^T +
    s s^T) / 12 with s = v0 + v1 + v2, area-weighted over the shape."""
    v = np.asarray(verts, dtype=np.float64)
    area = face_areas(v, faces) if area is None else area
    tri = v[faces]                                               # (F,3 corners,3)
    s = tri.sum(axis=1)
    total = _per_shape(area, face_off)
    centroid = _per_shape(area[:, None] * s / 3.0, face_off) / total[:, None]
    second = _per_shape(area * ((tri * tri).sum(axis=(1, 2)) + (s * s).sum(axis=1)) / 12.0, face_off) / total      # E[x^2 + y^2 + z^2]
    pooled = centroid.sum(axis=1) / 3.0
    return centroid, np.sqrt(np.maximum(second / 3.0 - pooled * pooled, 0.0))


# ---------------------------------------------------------------------------- visible faces (csrc/visible.hip)
def _directions():
    """The 26 directions of {-1,0,1}^3 without the origin: the 6 axes, then the 8 corners, then the 12 edge midpoints."""
    grid = [(x, y, z) for x in (1, 0, -1) for y in (1, 0, -1) for z in (1, 0, -1) if (x, y, z) != (0, 0, 0)]
    return np.asarray(sorted(grid, key=lambda d: ({1: 0, 3: 1, 2: 2}[abs(d[0]) + abs(d[1]) + abs(d[2])],)), dtype=np.float64)


def view_bases(directions):
    """(NV,3,3) fp32 rows (e_x, e_y, e_z) of the views that look at the centre FROM the given directions (NV,3): e_z = -d / |d| (depth
    grows away from the eye), e_x = a x e_z normalised with a the coordinate axis of the smallest |d| component (the first of equals),
    e_y = e_z x e_x; in fp64, rounded to fp32 at the end."""
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    norm = np.linalg.norm(d, axis=1)
    if not (d.shape[0] >= 1 and np.all(np.isfinite(d)) and np.all(norm > 0)):
        raise ValueError("view_bases: directions are finite and not zero")
    ez = -d / norm[:, None]
    a = np.eye(3)[np.argmin(np.abs(ez), axis=1)]
    ex = np.cross(a, ez)
    ex /= np.linalg.norm(ex, axis=1)[:, None]
    ey = np.cross(ez, ex)
    return np.ascontiguousarray((np.stack([ex, ey, ez], 1) + 0.0).astype(np.float32))      # (+ 0.0: no negative zeros)


def default_views(n=26):
    """The view table of `face_visibility`: n = 6 (the axes), 14 (and the corners) or 26 (and the edge midpoints) directions."""
    if n not in (6, 14, 26):
        raise ValueError("default_views: 6, 14 or 26 views, got %r" % (n,))
    return view_bases(_directions()[:n])


def shape_frames(verts, faces, face_off):
    """(S,4) fp32 (centre, radius) per shape: the centre of the box of the vertices of its faces of positive area, and the largest
    distance of such a vertex from it times (1 + 2^-10), in fp64; (0, 0, 0, 1) for a shape without such a face."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    area = face_areas(v, faces)
    out = np.zeros((len(face_off) - 1, 4), dtype=np.float64)
    out[:, 3] = 1.0
    for c in range(out.shape[0]):
        f = faces[face_off[c]:face_off[c + 1]][area[face_off[c]:face_off[c + 1]] > 0.0]
        if f.shape[0]:
            p = v[np.unique(f)]
            ctr = (p.min(axis=0) + p.max(axis=0)) / 2.0
            out[c, :3], out[c, 3] = ctr, np.sqrt(((p - ctr) ** 2).sum(axis=1).max()) * (1.0 + 2.0 ** -10)
    return out.astype(np.float32)


def _view_arguments(verts, faces, face_off, views, device, what):
    """The front of `face_visibility` and `face_orientation`: the checks, the view table and the frames, and everything on the device
    -> (S, V, F, NV, [verts, faces, face_off, frame, views] device tensors)."""
    import torch
    from . import _lib
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    face_off = np.ascontiguousarray(face_off, dtype=np.int32).reshape(-1)
    S, V, F = face_off.shape[0] - 1, verts.shape[0], faces.shape[0]
    if S < 1 or face_off[0] != 0 or face_off[-1] != F or np.any(np.diff(face_off) < 0):
        raise ValueError("%s: face_off must ascend from 0 to the number of faces over at least one shape" % what)
    if F and (faces.min() < 0 or faces.max() >= V):
        raise ValueError("%s: a face names a vertex outside the %d vertices" % (what, V))
    table = default_views(views) if np.ndim(views) == 0 else np.asarray(views)
    table = view_bases(table) if table.ndim == 2 else np.ascontiguousarray(table, dtype=np.float32)
    if table.ndim != 3 or table.shape[1:] != (3, 3):
        raise ValueError("%s: views are a count, (NV,3) directions or (NV,3,3) bases, got %s" % (what, table.shape,))
    frame = shape_frames(verts, faces, face_off)
    dev = torch.device("cuda" if device is None else device)
    tensors = [torch.from_numpy(a).to(dev) for a in (verts, faces, face_off, frame, table)]
    _lib.require(tensors[0], "the vertices", torch.float32, 2)
    return S, V, F, int(table.shape[0]), tensors


def face_visibility(verts, faces, face_off, views=26, resolution=128, device=None):
    """mask (F) uint32 numpy: bit v set where face f passes the depth test of view v (pdgn_mesh_visibility; the definition is the header
    block of csrc/visible.hip).  views: 6 / 14 / 26 (`default_views`), an (NV,3) array of directions to look from, or an (NV,3,3) table
    of bases; raw or normalised geometry alike (the frame of `shape_frames` makes the result the same up to the snap)."""
    import torch
    from . import _lib
    S, V, F, NV, d = _view_arguments(verts, faces, face_off, views, device, "face_visibility")
    mask = torch.zeros(F, dtype=torch.int32, device=d[0].device)
    _lib.check(_lib.lib().pdgn_mesh_visibility(S, V, F, *[_lib.ptr(x) for x in d], NV, int(resolution), _lib.ptr(mask),
                                               _lib.stream_of(d[0])), "pdgn_mesh_visibility")
    return mask.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------- face orientation from visibility (csrc/visible.hip)
def orientation_from_votes(front, back, face_off=None):
    """The decision rule on the votes of pdgn_mesh_face_votes, front and back (F) counts: {"front", "back" (F) uint32, "flip" (F) bool:
    back > front -- a tie, a dead face and an unseen face keep their order --, "undecided" (F): front == back, "two_sided" (F): both sides
    were seen and the rarer one at least a quarter as often as the other (min > 0 and 4 min >= max: a sheet, an open table top; no flip
    gives it a sign)[, with face_off (S+1): "flipped", "undecided_count", "two_sided_count" (S) int64 per shape]}."""
    front, back = (np.ascontiguousarray(np.asarray(x).astype(np.uint32, copy=False)).reshape(-1) for x in (front, back))
    if front.shape != back.shape:
        raise ValueError("orientation_from_votes: %d front and %d back counts" % (front.shape[0], back.shape[0]))
    lo, hi = np.minimum(front, back).astype(np.int64), np.maximum(front, back).astype(np.int64)
    out = {"front": front, "back": back, "flip": back > front, "undecided": front == back, "two_sided": (lo > 0) & (4 * lo >= hi)}
    if face_off is not None:
        off = np.asarray(face_off, dtype=np.int64).reshape(-1)
        per = lambda flag: np.diff(np.concatenate([[0], np.cumsum(flag.astype(np.int64))])[off])     # (an empty shape counts 0)
        out.update(flipped=per(out["flip"]), undecided_count=per(out["undecided"]), two_sided_count=per(out["two_sided"]))
    return out


def face_orientation(verts, faces, face_off, views=26, resolution=128, device=None, return_mask=False):
    """Which way round every face is stored, from which of its sides a ring of views sees (pdgn_mesh_face_votes; the definition is the
    second header block of csrc/visible.hip; Takayama et al. 2014): `orientation_from_votes` of the device's votes, with the per-shape
    counts[, and "mask" (F) uint32, exactly `face_visibility`'s masks for the same arguments, from the same depth pass].  The arguments
    are `face_visibility`'s."""
    import torch
    from . import _lib
    S, V, F, NV, d = _view_arguments(verts, faces, face_off, views, device, "face_orientation")
    votes = torch.zeros(F, 2, dtype=torch.int32, device=d[0].device)
    mask = torch.zeros(F, dtype=torch.int32, device=d[0].device) if return_mask else None
    _lib.check(_lib.lib().pdgn_mesh_face_votes(S, V, F, *[_lib.ptr(x) for x in d], NV, int(resolution), _lib.ptr(mask), _lib.ptr(votes),
                                               _lib.stream_of(d[0])), "pdgn_mesh_face_votes")
    votes = votes.cpu().numpy().view(np.uint32)
    out = orientation_from_votes(votes[:, 0], votes[:, 1], d[2].cpu().numpy())
    if return_mask:
        out["mask"] = mask.cpu().numpy().view(np.uint32)
    return out


class MeshSet:
    """S shapes as the device arrays of pdgn_feed_batch_mesh / pdgn_sample_surface (include/pdgn_hip.h): verts (V,3) fp32, faces (F,3)
    int32 global vertex indices, face_off (S+1) int32, alias (F,2) int32 holding the bits of the uint32 records (threshold, alias local
    to the shape); shift (S,3) / scale (S) fp32: the normalisation that was applied ((raw - shift) / scale).  Built by `from_meshes` /
    `from_arrays`, which guarantee what the kernels trust: every shape owns a face of positive area, every index is inside the vertex
    array, every alias inside its shape.  visible (F) or None: the view masks the set was built with -- a face whose mask is 0 has
    weight zero in the table (threshold 0, nobody's alias: never drawn) and in the normalisation.  flip (F) bool or None: the faces
    `face_orientation` found stored the wrong way round; carried only -- the geometry stays as given until `oriented()` applies it."""

    def __init__(self, verts, faces, face_off, alias, shift, scale, normalize=None, visible=None, flip=None):
        self.verts, self.faces, self.face_off, self.alias, self.shift, self.scale = verts, faces, face_off, alias, shift, scale
        self.normalize = normalize
        self.visible = visible                                   # (F) int32, the bits of the uint32 masks of `face_visibility`, or None
        self.flip = flip                                         # (F) bool: `face_orientation`'s "flip", or None
        self.S, self.V, self.F = int(face_off.shape[0]) - 1, int(verts.shape[0]), int(faces.shape[0])

    # ------------------------------------------------------------------ construction (host, numpy)
    @classmethod
    def from_meshes(cls, meshes, normalize=None, names=None, visible=None, flip=None):
        """meshes: a list of (verts (V_c,3), faces (F_c,3) indices into that shape's own vertices); visible, flip: as `from_arrays`."""
        meshes = list(meshes)
        if not meshes:
            raise ValueError("MeshSet: no shapes")
        name = (lambda c: "shape %d" % c) if names is None else (lambda c: "shape %d (%s)" % (c, names[c]))
        verts, faces, face_off, at = [], [], [0], 0
        for c, (v, f) in enumerate(meshes):
            v, f = np.asarray(v), np.asarray(f)
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
                raise ValueError("%s: vertices are (V,3) and faces (F,3), got %s and %s" % (name(c), v.shape, f.shape))
            if f.shape[0] and (f.min() < 0 or f.max() >= v.shape[0]):
                raise ValueError("%s: a face names vertex %d, the shape has %d vertices" % (name(c), int(f.max() if f.max() >= v.shape[0] else f.min()), v.shape[0]))
            if not np.isfinite(v).all():
                raise ValueError("%s: vertex %d is not finite" % (name(c), int(np.argmax(~np.isfinite(v).all(axis=1)))))
            verts.append(v.astype(np.float32, copy=False))
            faces.append(f.astype(np.int64) + at)
            at += v.shape[0]
            face_off.append(face_off[-1] + f.shape[0])
        return cls.from_arrays(np.concatenate(verts, 0), np.concatenate(faces, 0), np.asarray(face_off), normalize, names, visible, flip)

    @classmethod
    def from_arrays(cls, verts, faces, face_off, normalize=None, names=None, visible=None, flip=None):
        """From the concatenated form (what `pack` stores): verts (V,3), faces (F,3) GLOBAL indices, face_off (S+1).  visible: (F) masks
        (`face_visibility`); a face whose mask is 0 counts as a face of area zero in the table, the normalisation and the vertex box.
        flip: (F) booleans (`face_orientation`), stored with the set and nothing else: the faces keep the order they came in."""
        import torch
        if normalize not in NORMALIZE:
            raise ValueError("MeshSet: normalize %r -- meshes take None, 'shape_unit' or 'shape_bbox' (global_unit, shape_half and shape_34 "
                             "are defined on stored clouds only)" % (normalize,))
        name = (lambda c: "shape %d" % c) if names is None else (lambda c: "shape %d (%s)" % (c, names[c]))
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        face_off = np.asarray(face_off, dtype=np.int64).reshape(-1)
        S, V, F = face_off.shape[0] - 1, verts.shape[0], faces.shape[0]
        if S < 1 or face_off[0] != 0 or face_off[-1] != F or np.any(np.diff(face_off) < 0):
            raise ValueError("MeshSet: face_off must ascend from 0 to the number of faces over at least one shape")
        if 3 * max(V, F) > 0x7FFFFFFF:
            raise ValueError("MeshSet: %d vertices and %d faces, the kernels index 3 V and 3 F with 32 bits" % (V, F))
        shape_of = np.repeat(np.arange(S), np.diff(face_off))
        if F and (faces.min() < 0 or faces.max() >= V):
            c = int(shape_of[np.argmax((faces.min(axis=1) < 0) | (faces.max(axis=1) >= V))])
            raise ValueError("%s: a face names a vertex outside the %d vertices" % (name(c), V))
        used = np.zeros(V, dtype=bool)
        used[faces.reshape(-1)] = True
        owner = np.full(V, -1, dtype=np.int64)
        owner[faces.reshape(-1)] = np.repeat(shape_of, 3)
        if np.any(owner[faces] != shape_of[:, None]):
            raise ValueError("MeshSet: two shapes share a vertex; every shape brings its own vertices")
        bad = used & ~np.isfinite(verts).all(axis=1)
        if bad.any():
            raise ValueError("%s: vertex %d is not finite" % (name(int(owner[np.argmax(bad)])), int(np.argmax(bad))))
        area = face_areas(verts, faces)
        for c in range(S):
            if not np.any(area[face_off[c]:face_off[c + 1]] > 0.0):
                raise ValueError("%s: no face of positive area (%d faces)" % (name(c), face_off[c + 1] - face_off[c]))
        if visible is not None:
            visible = np.ascontiguousarray(np.asarray(visible).astype(np.uint32, copy=False)).reshape(-1)
            if visible.shape[0] != F:
                raise ValueError("MeshSet: %d visibility masks for %d faces" % (visible.shape[0], F))
            area = np.where(visible != 0, area, 0.0)
            for c in range(S):
                if not np.any(area[face_off[c]:face_off[c + 1]] > 0.0):
                    raise ValueError("%s: no visible face of positive area (%d faces, every mask is 0)" % (name(c), face_off[c + 1] - face_off[c]))
        # the normalisation, over the surface
        if normalize == "shape_unit" and visible is not None:      # over the visible faces alone: the sums of a set that holds no others, bit for bit
            keep = visible != 0
            kept_off = np.concatenate([[0], np.cumsum(_per_shape(keep.astype(np.int64), face_off))])
            shift, scale = surface_statistics(verts, faces[keep], kept_off, area[keep])
        elif normalize == "shape_unit":
            shift, scale = surface_statistics(verts, faces, face_off, area)
        elif normalize == "shape_bbox":                          # data.normalize_clouds' expressions, in fp32, on the vertices of the faces of positive area
            shift, scale = np.zeros((S, 3), np.float32), np.ones(S, np.float32)
            for c in range(S):
                f = faces[face_off[c]:face_off[c + 1]][area[face_off[c]:face_off[c + 1]] > 0.0]
                lo, hi = verts[f.reshape(-1)].min(axis=0), verts[f.reshape(-1)].max(axis=0)
                shift[c], scale[c] = (lo + hi) / np.float32(2), (hi - lo).max() / np.float32(2)
        else:
            shift, scale = np.zeros((S, 3)), np.ones(S)
        if normalize is not None:
            if not np.all(scale > 0):
                raise ValueError("%s: its surface has no extent" % name(int(np.argmin(scale > 0))))
            own = np.where(used, owner, 0)
            moved = ((verts.astype(np.float64) - np.asarray(shift, np.float64)[own]) / np.asarray(scale, np.float64)[own][:, None]).astype(np.float32)
            verts = np.where(used[:, None], moved, verts)
            area = face_areas(verts, faces)                      # (a uniform scale per shape: the same table up to rounding; built from what is drawn from)
            if visible is not None:
                area = np.where(visible != 0, area, 0.0)
        if flip is not None:
            flip = np.ascontiguousarray(np.asarray(flip).astype(bool, copy=False)).reshape(-1)
            if flip.shape[0] != F:
                raise ValueError("MeshSet: %d orientation flips for %d faces" % (flip.shape[0], F))
        alias = np.empty((F, 2), dtype=np.uint32)
        for c in range(S):
            a, b = face_off[c], face_off[c + 1]
            alias[a:b, 0], alias[a:b, 1] = alias_table(area[a:b])
        t = torch.from_numpy
        return cls(t(verts), t(faces.astype(np.int32)), t(face_off.astype(np.int32)), t(alias.view(np.int32)),
                   t(np.asarray(shift, np.float32)), t(np.asarray(scale, np.float32)), normalize,
                   None if visible is None else t(visible.view(np.int32).copy()), None if flip is None else t(flip.copy()))

    # ------------------------------------------------------------------ storage and placement
    _FIELDS = ("verts", "faces", "face_off", "alias", "shift", "scale")

    def save(self, path):
        extra = {} if self.visible is None else {"visible": self.visible.cpu().numpy()}
        if self.flip is not None:
            extra["flip"] = self.flip.cpu().numpy()
        np.savez(path, normalize=np.asarray("" if self.normalize is None else self.normalize),
                 **{k: getattr(self, k).cpu().numpy() for k in self._FIELDS}, **extra)

    @classmethod
    def load(cls, path):
        import torch
        with np.load(path) as f:
            mode = str(f["normalize"])
            return cls(*(torch.from_numpy(f[k]) for k in cls._FIELDS), normalize=mode or None,
                       visible=torch.from_numpy(f["visible"]) if "visible" in f.files else None,
                       flip=torch.from_numpy(f["flip"].astype(bool, copy=False)) if "flip" in f.files else None)

    def to(self, device):
        return MeshSet(*(getattr(self, k).to(device).contiguous() for k in self._FIELDS), normalize=self.normalize,
                       visible=None if self.visible is None else self.visible.to(device).contiguous(),
                       flip=None if self.flip is None else self.flip.to(device).contiguous())

    def in_frame(self, shift, scale):
        """The same shapes with every vertex v of shape s at (v - shift[s]) / scale[s], in fp32 as data.normalize_clouds moves points:
        shift (S,3), scale (S) tensors.  The frame of clouds that were drawn from this set and then normalised one by one (the reports'
        reference clouds): a point drawn on a face stays within a few ulps of the moved face.  Faces, tables and masks are shared."""
        import torch
        shift = torch.as_tensor(shift, dtype=torch.float32, device=self.verts.device).reshape(self.S, 3)
        scale = torch.as_tensor(scale, dtype=torch.float32, device=self.verts.device).reshape(self.S)
        if not (torch.isfinite(shift).all() and torch.isfinite(scale).all() and (scale > 0).all()):
            raise ValueError("MeshSet.in_frame: shifts are finite, scales finite and positive")
        counts = (self.face_off[1:] - self.face_off[:-1]).long()
        shape_of = torch.repeat_interleave(torch.arange(self.S, device=self.verts.device), counts)
        owner = torch.full((self.V,), -1, dtype=torch.long, device=self.verts.device)
        owner[self.faces.long().reshape(-1)] = shape_of.repeat_interleave(3)
        used = owner >= 0
        own = owner.clamp_min(0)
        verts = torch.where(used[:, None], (self.verts - shift[own]) / scale[own][:, None], self.verts).contiguous()
        return MeshSet(verts, self.faces, self.face_off, self.alias, self.shift + self.scale[:, None] * shift, self.scale * scale,
                       normalize=self.normalize, visible=self.visible, flip=self.flip)

    def oriented(self):
        """The set with its stored flips applied: a face whose `flip` is set has its second and third vertex exchanged, so that its
        normal points the other way (`winding_number` and everything signed read the order).  Vertices, alias table, masks, shift and
        scale are shared -- the area of a face read backwards is the same fp64 number, so the table is the table --, flip is None, and
        nothing prepared for the old order (`mesh_dist_records`) is carried over.  `sample()` on the result draws from the same faces in
        the same proportions, the same face index for every point, but not the same points: the barycentric pair of a flipped face is
        mirrored."""
        import torch
        if self.flip is None:
            raise ValueError("MeshSet.oriented: the set holds no orientation flips (face_orientation computes them, pack --orient stores them)")
        flip = self.flip.to(self.faces.device).bool()
        faces = torch.where(flip[:, None], self.faces[:, [0, 2, 1]], self.faces).contiguous()
        return MeshSet(self.verts, faces, self.face_off, self.alias, self.shift, self.scale, normalize=self.normalize, visible=self.visible)
    def visible_stats(self):
        """What the masks leave out: {"faces", "hidden" (S) int64, "kept" (S) the share of every shape's area that is still drawn from,
        "total_faces", "total_hidden", "total_kept" (of the summed area)}; without masks nothing is hidden."""
        verts, faces, off = self.verts.cpu().numpy(), self.faces.cpu().numpy().astype(np.int64), self.face_off.cpu().numpy().astype(np.int64)
        area = face_areas(verts, faces)
        seen = np.ones(self.F, dtype=bool) if self.visible is None else self.visible.cpu().numpy() != 0
        total, kept = _per_shape(area, off), _per_shape(np.where(seen, area, 0.0), off)
        hidden = _per_shape((~seen).astype(np.int64), off)
        return {"faces": np.diff(off), "hidden": hidden, "kept": kept / total, "total_faces": self.F, "total_hidden": int(hidden.sum()),
                "total_kept": float(kept.sum() / total.sum())}

    def alias_records(self):
        """(threshold, alias) as two uint32 numpy arrays (F)."""
        rec = self.alias.cpu().numpy().view(np.uint32)
        return rec[:, 0].copy(), rec[:, 1].copy()

    # ------------------------------------------------------------------ held-out draws
    def sample(self, n, seed, draw=0, return_faces=False):
        """(S,n,3): n i.i.d. points of every shape's surface (pdgn_sample_surface), a pure function of (seed, draw); its streams are
        apart from every training draw of the same seed.  return_faces: also the (S,n) int32 global face index of every point."""
        import torch
        from . import _lib
        _lib.require(self.verts, "the mesh set's vertices", torch.float32, 2)
        out = torch.empty(self.S, int(n), 3, dtype=torch.float32, device=self.verts.device)
        rec = torch.empty(self.S, int(n), dtype=torch.int32, device=self.verts.device) if return_faces else None
        _lib.check(_lib.lib().pdgn_sample_surface(self.S, int(n), _lib.ptr(self.verts), _lib.ptr(self.faces), _lib.ptr(self.face_off),
                                                  _lib.ptr(self.alias), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF,
                                                  _lib.ptr(out), _lib.ptr(rec), _lib.stream_of(self.verts)), "pdgn_sample_surface")
        return (out, rec) if return_faces else out


# ---------------------------------------------------------------------------- point-to-surface distance (csrc/meshdist.hip)
SORT_POINTS = True                                               # the coherence options' defaults, each what measured faster at 10 k faces
SORT_FACES = False                                               # (profiles/p2m_cost.txt): points in Morton order, faces as given


def _morton30(x, lo, hi):
    """int64 Morton codes of 10 bits per axis of x (...,3) inside the box [lo, hi] (broadcasting); a coordinate that is not finite counts
    as the box's low side.  Only the ORDER the codes give is used, and no result depends on it."""
    import torch
    span = (hi - lo).clamp_min(1e-30)
    q = (torch.nan_to_num((x - lo) / span, nan=0.0, posinf=0.0, neginf=0.0).clamp(0.0, 1.0) * 1023.0).to(torch.int64)
    q = (q | (q << 16)) & 0x030000FF
    q = (q | (q << 8)) & 0x0300F00F
    q = (q | (q << 4)) & 0x030C30C3
    q = (q | (q << 2)) & 0x09249249
    return (q[..., 0] << 2) | (q[..., 1] << 1) | q[..., 2]


def mesh_dist_records(meshset, visible_only=False, sort_faces=None):
    """The prepared form of a mesh set for `point_to_mesh` (pdgn_mesh_dist_prepare), cached on the object per (visible_only, sort_faces):
    {"records", "groups", "group_off", "G", "live"}.  live = face_areas > 0 in fp64, and under visible_only the set's masks != 0."""
    import torch
    from . import _lib
    sort_faces = SORT_FACES if sort_faces is None else bool(sort_faces)
    if visible_only and meshset.visible is None:
        raise ValueError("point_to_mesh: visible_only needs a mesh set built with visibility masks")
    cache = meshset.__dict__.setdefault("_mesh_dist", {})
    key = (bool(visible_only), sort_faces)
    if key in cache:
        return cache[key]
    L = _lib.lib()
    group = L.pdgn_mesh_dist_group()
    _lib.require(meshset.verts, "the mesh set's vertices", torch.float32, 2)
    dev = meshset.verts.device
    S, V, F = meshset.S, meshset.V, meshset.F
    faces_h, off_h = meshset.faces.cpu().numpy().astype(np.int64), meshset.face_off.cpu().numpy().astype(np.int64)
    live = face_areas(meshset.verts.cpu().numpy(), faces_h) > 0.0
    if visible_only:
        live &= meshset.visible.cpu().numpy() != 0
    group_off = np.concatenate([[0], np.cumsum(-(-np.diff(off_h) // group))]).astype(np.int32)
    G = int(group_off[-1])
    order = None
    if sort_faces:
        centre = meshset.verts[meshset.faces.long()].mean(dim=1)                           # (F,3)
        shape_of = torch.repeat_interleave(torch.arange(S, device=dev), torch.from_numpy(np.diff(off_h)).to(dev))
        lo = torch.full((S, 3), float("inf"), device=dev).scatter_reduce(0, shape_of[:, None].expand(-1, 3), centre, "amin")
        hi = torch.full((S, 3), float("-inf"), device=dev).scatter_reduce(0, shape_of[:, None].expand(-1, 3), centre, "amax")
        code = (shape_of << 30) | _morton30(centre, lo[shape_of], hi[shape_of])
        order = torch.argsort(code, stable=True).to(torch.int32).contiguous()
    space = torch.empty(int(L.pdgn_mesh_dist_workspace_floats(S, F)), dtype=torch.float32, device=dev)
    records, groups = space[:12 * F], space[12 * F:12 * F + 8 * G]
    d_live, d_goff = torch.from_numpy(live.astype(np.int32)).to(dev), torch.from_numpy(group_off).to(dev)
    _lib.check(L.pdgn_mesh_dist_prepare(S, V, F, G, _lib.ptr(meshset.verts), _lib.ptr(meshset.faces), _lib.ptr(meshset.face_off),
                                        _lib.ptr(d_goff), _lib.ptr(d_live), _lib.ptr(order), _lib.ptr(records), _lib.ptr(groups),
                                        _lib.stream_of(meshset.verts)), "pdgn_mesh_dist_prepare")
    cache[key] = {"records": records, "groups": groups, "group_off": d_goff, "G": G, "live": live, "space": space}
    return cache[key]


def _shape_argument(shape, B, S, what):
    """`shape` of point_to_mesh and its callers as a (B) int64 numpy array, checked."""
    if shape is None:
        if B != S:
            raise ValueError("%s: %d clouds and %d shapes -- say which shape each cloud is measured against (shape=...)" % (what, B, S))
        return np.arange(B, dtype=np.int64)
    host = shape.detach().cpu().numpy() if hasattr(shape, "detach") else np.asarray(shape)
    if host.ndim != 1 or host.shape[0] != B or host.dtype.kind not in "iu":
        raise ValueError("%s: shape is (B) = (%d) integers, got %s %s" % (what, B, host.dtype, host.shape))
    if host.size and (host.min() < 0 or host.max() >= S):
        raise ValueError("%s: shape index %d, the mesh set has %d shapes" % (what, int(host.max() if host.max() >= S else host.min()), S))
    return host.astype(np.int64)


def _meshset_argument(meshset, visible_only, what):
    if not isinstance(meshset, MeshSet):
        raise ValueError("%s: meshset is a MeshSet, got %s" % (what, type(meshset).__name__))
    if visible_only and meshset.visible is None:
        raise ValueError("%s: visible_only needs a mesh set built with visibility masks" % what)


def _query_arguments(xyz, meshset, shape, visible_only, what):
    """The checks every query of points against a mesh set opens with -> (B, N, shape (B) int64 numpy)."""
    import torch
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 3 or xyz.shape[2] != 3 or xyz.dtype != torch.float32:
        raise ValueError("%s: xyz is a (B,N,3) float32 tensor, got %s" % (
            what, "%s %s" % (xyz.dtype, tuple(xyz.shape)) if isinstance(xyz, torch.Tensor) else type(xyz).__name__))
    _meshset_argument(meshset, False, what)
    B, N, _ = xyz.shape
    if B < 1 or N < 1 or B * N > 0x7FFFFFFF:
        raise ValueError("%s: %d clouds of %d points; at least one point, and B N below 2^31" % (what, B, N))
    shape_h = _shape_argument(shape, B, meshset.S, what)
    _meshset_argument(meshset, visible_only, what)
    if xyz.device != meshset.verts.device:
        raise ValueError("%s: xyz is on %s, the mesh set on %s" % (what, xyz.device, meshset.verts.device))
    return B, N, shape_h


def _sorted_points(xyz, sort_points):
    """(xyz as the kernels take it, perm): every cloud's points in Morton order; perm None: as given (sort_points off, or one point)."""
    import torch
    from . import _lib
    xyz = _lib.require(xyz.detach().contiguous(), "xyz", torch.float32, 3)
    if not (SORT_POINTS if sort_points is None else bool(sort_points)) or xyz.shape[1] <= 1:
        return xyz, None
    finite = torch.nan_to_num(xyz, nan=0.0, posinf=0.0, neginf=0.0)
    perm = torch.argsort(_morton30(xyz, finite.amin(dim=1, keepdim=True), finite.amax(dim=1, keepdim=True)), dim=1, stable=True)
    return torch.gather(xyz, 1, perm[..., None].expand(-1, -1, 3)).contiguous(), perm


def _unsorted(perm, *tensors):
    """The kernel's results (B,N) or (B,N,3) back in the caller's point order; None stays None."""
    if perm is None:
        return tensors
    return tuple(t if t is None else t.new_empty(t.shape).scatter_(1, perm if t.dim() == 2 else perm[..., None].expand_as(t), t) for t in tensors)


def point_to_mesh(xyz, meshset, shape=None, visible_only=False, cull=True, return_closest=False, sort_points=None, sort_faces=None):
    """The closest point of a triangle set (pdgn_point_mesh_distance; the definition is the header block of csrc/meshdist.hip): xyz (B,N,3)
    fp32 on the mesh set's device; shape (B) integers, the shape each cloud is measured against (repeats and any order; None: cloud c
    against shape c, B == S) -> d2 (B,N) the least squared distance to a live face, face (B,N) int32 the global index of the face that
    attains it (the lowest on ties)[, closest (B,N,3)]; NaN, -1, NaN for a point that is not finite.  Live: positive area and, under
    visible_only, a visibility mask that is not 0 (the distance to the visible surface).  cull, sort_points (the points go to the kernel
    in Morton order and the results are scattered back) and sort_faces (the records are in Morton order of the centroids) change no bit;
    None: the module's defaults.  Unsigned; no autograd (losses.surface_distance is the differentiable form)."""
    import torch
    from . import _lib
    B, N, shape_h = _query_arguments(xyz, meshset, shape, visible_only, "point_to_mesh")
    rec = mesh_dist_records(meshset, visible_only, sort_faces)
    xyz, perm = _sorted_points(xyz, sort_points)
    dev = xyz.device
    d_shape = torch.from_numpy(shape_h.astype(np.int32)).to(dev)
    d2 = torch.empty(B, N, dtype=torch.float32, device=dev)
    face = torch.empty(B, N, dtype=torch.int32, device=dev)
    closest = torch.empty(B, N, 3, dtype=torch.float32, device=dev) if return_closest else None
    _lib.check(_lib.lib().pdgn_point_mesh_distance(B, N, meshset.S, meshset.F, rec["G"], _lib.ptr(xyz), _lib.ptr(d_shape),
                                                   _lib.ptr(meshset.face_off), _lib.ptr(rec["group_off"]), _lib.ptr(rec["records"]),
                                                   _lib.ptr(rec["groups"]), 1 if cull else 0, _lib.ptr(d2), _lib.ptr(face),
                                                   _lib.ptr(closest), _lib.stream_of(xyz)), "pdgn_point_mesh_distance")
    d2, face, closest = _unsorted(perm, d2, face, closest)
    return (d2, face, closest) if return_closest else (d2, face)


# ---------------------------------------------------------------------------- generalized winding numbers (csrc/winding.hip)
def _winding(xyz, meshset, shape, visible_only, sort_points, splits, what):
    """The checks and the launch of `winding_number` -> (T (B,N) int64, w (B,N) fp32, inside (B,N) int32), all from the kernel."""
    import torch
    from . import _lib
    B, N, shape_h = _query_arguments(xyz, meshset, shape, visible_only, what)
    splits = 0 if splits is None else int(splits)
    if splits < 0:
        raise ValueError("%s: splits is None or 0 (the library chooses) or a count of parts, got %d" % (what, splits))
    rec = mesh_dist_records(meshset, visible_only)
    L = _lib.lib()
    if splits == 0:                                              # from the largest face count among the shapes named, which the host knows
        counts = meshset.__dict__.get("_face_counts")
        if counts is None:
            counts = meshset.__dict__["_face_counts"] = np.diff(meshset.face_off.cpu().numpy().astype(np.int64))
        splits = L.pdgn_winding_splits(B, N, max(1, int(counts[shape_h].max())))
        _lib.check(min(splits, 0), "pdgn_winding_splits")
    xyz, perm = _sorted_points(xyz, sort_points)
    dev = xyz.device
    d_shape = torch.from_numpy(shape_h.astype(np.int32)).to(dev)
    nbytes = L.pdgn_winding_workspace_bytes(B, N, meshset.F, splits)
    _lib.check(min(nbytes, 0), "pdgn_winding_workspace_bytes")
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=dev) if nbytes else None
    T = torch.empty(B, N, dtype=torch.int64, device=dev)
    w = torch.empty(B, N, dtype=torch.float32, device=dev)
    inside = torch.empty(B, N, dtype=torch.int32, device=dev)
    _lib.check(L.pdgn_winding_number(B, N, meshset.S, meshset.F, _lib.ptr(xyz), _lib.ptr(d_shape), _lib.ptr(meshset.face_off),
                                     _lib.ptr(rec["records"]), splits, _lib.ptr(work), _lib.ptr(T), _lib.ptr(w), _lib.ptr(inside),
                                     _lib.stream_of(xyz)), "pdgn_winding_number")
    return _unsorted(perm, T, w, inside)


def winding_number(xyz, meshset, shape=None, visible_only=False, sort_points=None, splits=None, return_sum=False):
    """The generalized winding number (pdgn_winding_number; the definition is the header block of csrc/winding.hip): xyz (B,N,3) fp32 on
    the mesh set's device; shape, visible_only and sort_points as for `point_to_mesh` -> w (B,N) fp32: 1 inside a closed, consistently
    oriented shape, 0 outside, NaN for a point that is not finite[, T (B,N) int64: the sum of the faces' half solid angles in units of
    2^-32, of which w is a rounding; INT64_MIN where w is NaN].  splits: None / 0, the library divides a shape's faces over as many
    workgroups as cover the chip; k: exactly k parts.  Neither it nor sort_points changes a bit.  No autograd."""
    T, w, _ = _winding(xyz, meshset, shape, visible_only, sort_points, splits, "winding_number")
    return (w, T) if return_sum else w


def signed_distance(xyz, meshset, shape=None, visible_only=False):
    """(sd (B,N) fp32, face (B,N) int32, inside (B,N) bool): sqrt(d2) of `point_to_mesh`, negated where the winding number is at least
    one half (the kernel's integer comparison); NaN, -1, False for a point that is not finite.  The sign means something on shapes whose
    faces are consistently oriented (`winding_report`)."""
    import torch
    d2, face = point_to_mesh(xyz, meshset, shape, visible_only)
    inside = _winding(xyz, meshset, shape, visible_only, None, None, "signed_distance")[2] != 0
    d = torch.sqrt(d2)
    return torch.where(inside, -d, d), face, inside


def _shape_list(shape, S, what):
    """A list of shapes to work on (None: all S of them) as an int64 numpy array, checked like `_shape_argument`."""
    if shape is None:
        return np.arange(S, dtype=np.int64)
    host = shape.detach().cpu().numpy() if hasattr(shape, "detach") else np.asarray(shape)
    if host.size < 1:
        raise ValueError("%s: shape names at least one shape" % what)
    return _shape_argument(host.reshape(-1) if host.ndim == 0 else host, int(host.size), S, what)


def shape_boxes(meshset, shape=None, visible_only=False):
    """(lo, hi) float64 numpy (S',3): the boxes of the vertices of the live faces of the shapes `shape` (None: all of them)."""
    shape_h = _shape_list(shape, meshset.S, "shape_boxes")
    live = mesh_dist_records(meshset, visible_only)["live"]
    verts, faces = meshset.verts.cpu().numpy().astype(np.float64), meshset.faces.cpu().numpy().astype(np.int64)
    off = meshset.face_off.cpu().numpy().astype(np.int64)
    lo, hi = np.zeros((shape_h.shape[0], 3)), np.zeros((shape_h.shape[0], 3))
    for k, s in enumerate(shape_h):
        f = faces[off[s]:off[s + 1]][live[off[s]:off[s + 1]]]
        if f.shape[0]:
            lo[k], hi[k] = verts[f.reshape(-1)].min(axis=0), verts[f.reshape(-1)].max(axis=0)
    return lo, hi


def cubic_grid(lo, hi, resolution, pad):
    """(origin (S',3) fp32, voxel (S') fp32) of R cells per axis over the boxes [lo, hi] (S',3) grown by `pad` of their longest side on
    every side and made cubic about their centres, in float64, rounded at the end."""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1, 3), np.asarray(hi, dtype=np.float64).reshape(-1, 3)
    side = (hi - lo).max(axis=1) * (1.0 + 2.0 * float(pad))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (side > 0).all()):
        raise ValueError("occupancy_grid: every box is finite and has an extent")
    return ((lo + hi) / 2.0 - side[:, None] / 2.0).astype(np.float32), (side / int(resolution)).astype(np.float32)


def bounds_grid(bounds, count, resolution):
    """`cubic_grid` without padding of a caller's bounds = (lo, hi), each (3) or (count,3): the grid starts at lo."""
    try:
        lo, hi = (np.broadcast_to(np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64), (count, 3)) for x in bounds)
    except (TypeError, ValueError):
        raise ValueError("occupancy_grid: bounds is a pair (lo, hi), each (3) or (%d,3)" % count) from None
    side = (hi - lo).max(axis=1)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (side > 0).all()):
        raise ValueError("occupancy_grid: every box is finite and has an extent")
    return np.ascontiguousarray(lo, dtype=np.float32), (side / int(resolution)).astype(np.float32)


OCCUPANCY_SLAB_POINTS = 1 << 22                                   # queries per launch of occupancy_grid, over all its shapes


def _occupancy(meshset, shape_h, resolution, origin, voxel, visible_only=False):
    """occ (S',R,R,R) bool on the device: T >= half a turn at the cell centres origin + (i + 0.5) voxel (the fp32 product, then the fp32
    sum), index order (x, y, z); planes of x in slabs of at most OCCUPANCY_SLAB_POINTS queries."""
    import torch
    from . import _lib
    dev = meshset.verts.device
    R, Sq = int(resolution), int(shape_h.shape[0])
    half = _lib.lib().pdgn_winding_half_turn()
    o, v = torch.from_numpy(np.ascontiguousarray(origin, dtype=np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(voxel, dtype=np.float32)).to(dev)
    axes = (torch.arange(R, dtype=torch.float32, device=dev) + 0.5)[None, :, None] * v[:, None, None] + o[:, None, :]      # (S',R,3)
    occ = torch.empty(Sq, R, R, R, dtype=torch.bool, device=dev)
    planes = max(1, min(R, OCCUPANCY_SLAB_POINTS // (Sq * R * R)))
    for x0 in range(0, R, planes):
        k = min(planes, R - x0)
        q = torch.stack([axes[:, x0:x0 + k, 0][:, :, None, None].expand(Sq, k, R, R), axes[:, :, 1][:, None, :, None].expand(Sq, k, R, R),
                         axes[:, :, 2][:, None, None, :].expand(Sq, k, R, R)], dim=-1).reshape(Sq, k * R * R, 3).contiguous()
        T = _winding(q, meshset, shape_h, visible_only, False, None, "occupancy_grid")[0]
        occ[:, x0:x0 + k] = (T >= half).reshape(Sq, k, R, R)
    return occ


def _resolution_argument(resolution, what):
    R = int(resolution)
    if R < 1 or R > 1024:
        raise ValueError("%s: resolution is 1 .. 1024 cells per axis, got %r" % (what, resolution))
    return R


def occupancy_grid(meshset, shape=None, resolution=64, bounds=None, pad=0.05, visible_only=False):
    """Which cells of a grid lie inside a shape (the winding number at the cell centres, `winding_number`'s integer comparison):
    -> (occ (S',R,R,R) bool indexed (shape, x, y, z), origin (S',3) fp32, voxel (S') fp32), cell (i, j, k)'s centre being
    origin + (i + 0.5, j + 0.5, k + 0.5) voxel.  shape: the shapes to grid (None: all).  bounds: (lo, hi), each (3) or (S',3) -- the grid
    starts at lo and its cubic cells are the longest side / R wide; None: every shape's own box, grown by `pad` of its longest side on
    every side and made cubic.  The queries go out in slabs of planes, so the memory taken besides the result stays bounded."""
    import torch
    _meshset_argument(meshset, False, "occupancy_grid")
    R = _resolution_argument(resolution, "occupancy_grid")
    shape_h = _shape_list(shape, meshset.S, "occupancy_grid")
    _meshset_argument(meshset, visible_only, "occupancy_grid")
    if bounds is None:
        origin, voxel = cubic_grid(*shape_boxes(meshset, shape_h, visible_only), R, pad)
    else:
        origin, voxel = bounds_grid(bounds, shape_h.shape[0], R)
    occ = _occupancy(meshset, shape_h, R, origin, voxel, visible_only)
    dev = meshset.verts.device
    return occ, torch.from_numpy(origin).to(dev), torch.from_numpy(voxel).to(dev)


def winding_report(meshset, samples=4096, seed=0):
    """Whether the shapes of a set are closed and consistently oriented enough for the signed quantities to mean anything: per shape, the
    winding number at `samples` uniform points of its box (grown by 5 % of its longest side) -> {"w_min", "w_max" (S) float64 numpy,
    "fractional" (S): the share of the points with |w - rint(w)| > 0.05}.  A watertight, outward-oriented shape gives 0, 1 and a share
    of 0 up to the points that fall within a hair of the surface; flipped or missing faces show as values in between."""
    import torch
    _meshset_argument(meshset, False, "winding_report")
    if int(samples) < 1:
        raise ValueError("winding_report: samples is a positive count, got %r" % (samples,))
    lo, hi = shape_boxes(meshset)
    grow = 0.05 * (hi - lo).max(axis=1, keepdims=True)
    u = torch.rand(meshset.S, int(samples), 3, dtype=torch.float64, generator=torch.Generator().manual_seed(int(seed)))
    pts = (torch.from_numpy(lo - grow)[:, None, :] + u * torch.from_numpy(hi - lo + 2 * grow)[:, None, :]).float().to(meshset.verts.device)
    w = winding_number(pts.contiguous(), meshset).double()
    frac = ((w - torch.round(w)).abs() > 0.05).double().mean(dim=1)
    return {"w_min": w.amin(dim=1).cpu().numpy(), "w_max": w.amax(dim=1).cpu().numpy(), "fractional": frac.cpu().numpy()}


# ---------------------------------------------------------------------------- directories and packed files
def read_obj_root(root, synsetids=None):
    """A directory <synsetid>/<split>/*.obj -> {synsetid: {split: (verts, faces GLOBAL within the split, face_off)}}, the files of a
    split in sorted name order; raw geometry.  synsetids: these categories only."""
    out = {}
    for sid in sorted(os.listdir(root)):
        if not os.path.isdir(os.path.join(root, sid)) or (synsetids is not None and sid not in synsetids):
            continue
        for split in SPLITS:
            folder = os.path.join(root, sid, split)
            if not os.path.isdir(folder):
                continue
            verts, faces, face_off, at = [], [], [0], 0
            for fname in sorted(n for n in os.listdir(folder) if n.endswith(".obj")):
                v, f = load_obj(os.path.join(folder, fname))
                verts.append(v)
                faces.append(f + np.int32(at))
                at += v.shape[0]
                face_off.append(face_off[-1] + f.shape[0])
            if verts:
                out.setdefault(sid, {})[split] = (np.concatenate(verts, 0), np.concatenate(faces, 0).astype(np.int32),
                                                  np.asarray(face_off, dtype=np.int32))
    if not out:
        raise ValueError("%s: no <synsetid>/<split>/*.obj meshes found" % (root,))
    return out


def _masks_and_flips(verts, faces, face_off, visible, orient):
    """(mask or None, orientation dict or None) of `pack` and `split_meshset`, visible and orient each None or a dict of options: where
    both are asked for with the same options, one `face_orientation` call -- one depth pass per view -- serves both."""
    if visible is not None and orient is not None and visible == orient:
        result = face_orientation(verts, faces, face_off, return_mask=True, **orient)
        return result["mask"], result
    return (None if visible is None else face_visibility(verts, faces, face_off, **visible),
            None if orient is None else face_orientation(verts, faces, face_off, **orient))


def pack(root, out_path, visible=None, orient=None, report=None):
    """Write the directory's meshes as one .npz with the keys "<synsetid>/<split>/{verts,faces,face_off}" (raw, un-normalised).
    visible: a dict of `face_visibility` options (views, resolution, device) -- one more array "<synsetid>/<split>/visible" per split,
    the (F) uint32 masks, computed on the device; orient: a dict of `face_orientation` options -- "<synsetid>/<split>/flip", the (F)
    booleans, the geometry stays as read; both None: the file is what it was before either existed.  report: a callable that gets
    (synsetid, split, orientation dict) per split oriented."""
    arrays = {}
    for sid, splits in read_obj_root(root).items():
        for split, (v, f, off) in splits.items():
            arrays["%s/%s/verts" % (sid, split)], arrays["%s/%s/faces" % (sid, split)], arrays["%s/%s/face_off" % (sid, split)] = v, f, off
            mask, result = _masks_and_flips(v, f, off, visible, orient)
            if mask is not None:
                arrays["%s/%s/visible" % (sid, split)] = mask
            if result is not None:
                arrays["%s/%s/flip" % (sid, split)] = result["flip"]
                if report is not None:
                    report(sid, split, result)
    np.savez(out_path, **arrays)
    return sorted(arrays)


def load_packed(path, synsetids=None):
    """The mapping `read_obj_root` returns, from a file `pack` wrote."""
    out = {}
    with np.load(path) as f:
        for key in f.files:
            sid, split, what = key.split("/")
            if what == "verts" and (synsetids is None or sid in synsetids):
                out.setdefault(sid, {})[split] = tuple(f["%s/%s/%s" % (sid, split, k)] for k in ("verts", "faces", "face_off"))
    return out


def load_packed_visible(path, synsetids=None):
    """{synsetid: {split: (F) uint32 masks}} of the splits of a packed file that `pack --visible` stored masks for (empty: none)."""
    out = {}
    with np.load(path) as f:
        for key in f.files:
            sid, split, what = key.split("/")
            if what == "visible" and (synsetids is None or sid in synsetids):
                out.setdefault(sid, {})[split] = f[key].astype(np.uint32, copy=False)
    return out


def load_packed_flip(path, synsetids=None):
    """{synsetid: {split: (F) bool flips}} of the splits of a packed file that `pack --orient` stored flips for (empty: none)."""
    out = {}
    with np.load(path) as f:
        for key in f.files:
            sid, split, what = key.split("/")
            if what == "flip" and (synsetids is None or sid in synsetids):
                out.setdefault(sid, {})[split] = f[key].astype(bool, copy=False)
    return out


def is_mesh_root(path):
    """Whether a --data_root holds meshes: an .npz with "<synsetid>/<split>/verts" keys, or a directory with a <synsetid>/<split>/*.obj."""
    path = str(path)
    if os.path.isdir(path):
        for sid in sorted(os.listdir(path)):
            for split in SPLITS:
                folder = os.path.join(path, sid, split)
                if os.path.isdir(folder) and any(n.endswith(".obj") for n in os.listdir(folder)):
                    return True
        return False
    if path.endswith(".npz") and os.path.exists(path):
        with np.load(path) as f:
            return any(k.count("/") == 2 and k.endswith("/verts") for k in f.files)
    return False


class MeshRoot(dict):
    """The mapping `open_mesh_root` returns; `visible`, `flip`: what `load_packed_visible` and `load_packed_flip` found beside the
    meshes ({} for a directory)."""
    visible = {}
    flip = {}


def open_mesh_root(path, synsetids=None):
    if os.path.isdir(path):
        return MeshRoot(read_obj_root(str(path), synsetids))
    root = MeshRoot(load_packed(path, synsetids))
    root.visible = load_packed_visible(path, synsetids)
    root.flip = load_packed_flip(path, synsetids)
    return root


def has_stored_visible(root, split):
    """Whether every category of an opened root that has the split has stored masks for it."""
    stored = getattr(root, "visible", {})
    sids = [sid for sid in sorted(root) if split in root[sid]]
    return bool(sids) and all(split in stored.get(sid, {}) for sid in sids)


def has_stored_flip(root, split):
    """Whether every category of an opened root that has the split has stored orientation flips for it."""
    stored = getattr(root, "flip", {})
    sids = [sid for sid in sorted(root) if split in root[sid]]
    return bool(sids) and all(split in stored.get(sid, {}) for sid in sids)


def split_meshset(root, split, normalize=None, visible=None, orient=None):
    """One MeshSet of a split over every category of an opened root (`open_mesh_root`, or the path of one), categories in sorted order.
    visible: None (every face is drawn from), a dict of `face_visibility` options (views, resolution, device: the masks are computed
    now) or "stored" (the masks `pack --visible` wrote; an error where the data holds none).  orient: the same three for the set's
    `flip` -- None, a dict of `face_orientation` options or "stored" (what `pack --orient` wrote); two equal dicts share one device pass.
    The flips are carried, not applied: `.oriented()` applies them."""
    if isinstance(root, (str, os.PathLike)):
        root = open_mesh_root(root)
    parts = [root[sid][split] for sid in sorted(root) if split in root[sid]]
    if not parts:
        raise ValueError("the mesh data has no %r split" % split)
    if visible is not None and not isinstance(visible, dict) and visible != "stored":
        raise ValueError("split_meshset: visible is None, a dict of face_visibility options or 'stored', got %r" % (visible,))
    if orient is not None and not isinstance(orient, dict) and orient != "stored":
        raise ValueError("split_meshset: orient is None, a dict of face_orientation options or 'stored', got %r" % (orient,))
    if orient == "stored" and not has_stored_flip(root, split):
        raise ValueError("orient='stored': the mesh data holds no orientation flips for its %r split (python -m pdgn_amd.meshes pack DIR "
                         "OUT.npz --orient writes them)" % split)
    if visible == "stored" and not has_stored_visible(root, split):
        raise ValueError("visible='stored': the mesh data holds no visibility masks for its %r split (python -m pdgn_amd.meshes pack DIR "
                         "OUT.npz --visible writes them)" % split)
    verts, faces, face_off, at, fat = [], [], [np.zeros(1, np.int64)], 0, 0
    for v, f, off in parts:
        verts.append(v)
        faces.append(f.astype(np.int64) + at)
        face_off.append(off[1:].astype(np.int64) + fat)
        at, fat = at + v.shape[0], fat + int(off[-1])
    verts, faces, face_off = np.concatenate(verts, 0), np.concatenate(faces, 0), np.concatenate(face_off, 0)
    mask, result = _masks_and_flips(verts, faces, face_off, visible if isinstance(visible, dict) else None,
                                    orient if isinstance(orient, dict) else None)
    flip = None if result is None else result["flip"]
    if visible == "stored":
        mask = np.concatenate([root.visible[sid][split] for sid in sorted(root) if split in root[sid]], 0)
    if orient == "stored":
        flip = np.concatenate([root.flip[sid][split] for sid in sorted(root) if split in root[sid]], 0)
    return MeshSet.from_arrays(verts, faces, face_off, normalize, visible=mask, flip=flip)


USAGE = ("usage: python -m pdgn_amd.meshes pack DIR OUT.npz [--visible] [--orient] [--views 6|14|26] [--resolution R]\n"
         "       python -m pdgn_amd.meshes distance CLOUDS.npy MESHES.npz [--shape I,J,...] [--visible] [--signed] [--orient] [--split val] "
         "[--device cuda]\n"
         "       python -m pdgn_amd.meshes occupancy MESHES.npz OUT.npz --resolution R [--shape I,J,...] [--visible] [--orient] [--split val] "
         "[--device cuda]\n"
         "       python -m pdgn_amd.meshes check MESHES.npz [--samples N] [--orient] [--split val] [--device cuda]\n"
         "       python -m pdgn_amd.meshes render MESHES.npz -o sheet.png [--split val] [--shape I,J,...] [--rows N] [--cols N] [--cell C] "
         "[--visible] [--orient] [--shade flat|depth] [--device cuda]")


def distance_table(result):
    """The `surface_fidelity` dict as the lines `distance` prints: one row per cloud, then the batch means."""
    cols = [k for k in result if k != "mean"]
    lines = ["cloud " + " ".join("%22s" % k for k in cols)]
    B = int(result[cols[0]].shape[0])
    for c in range(B):
        lines.append("%5d " % c + " ".join("%22.9g" % float(result[k][c]) for k in cols))
    lines.append(" mean " + " ".join("%22.9g" % result["mean"][k] for k in cols))
    return lines


def _options(rest, opts, flags=(), valued=("--shape", "--split", "--device")):
    """The commands' options: `flags` set opts[name] = True, `valued` take the next word."""
    rest = list(rest)
    while rest:
        flag = rest.pop(0)
        if flag in flags:
            opts[flag[2:]] = True
        elif flag in valued and rest:
            opts[flag[2:]] = rest.pop(0)
        else:
            raise SystemExit(USAGE)
    return opts


def _shape_option(text):
    if text is None:
        return None
    try:
        return np.asarray([int(s) for s in text.split(",")], dtype=np.int64)
    except ValueError:
        raise SystemExit("--shape takes integers separated by commas\n" + USAGE) from None


def _open_meshset(path, split, visible, orient=False):
    """MESHES.npz of the commands: a file `pack` wrote (one split of it, raw geometry) or one `MeshSet.save` wrote.  orient: the set must
    carry orientation flips (the caller applies them: `.oriented()`)."""
    with np.load(path) as f:
        packed = any(k.count("/") == 2 for k in f.files)
    if not packed:
        ms = MeshSet.load(path)
        if orient and ms.flip is None:
            raise SystemExit("--orient: %s holds no orientation flips (pack --orient writes them)" % (path,))
        return ms
    root = open_mesh_root(path)
    if visible and not has_stored_visible(root, split):
        raise SystemExit("--visible: %s holds no visibility masks for its %r split (pack --visible writes them)" % (path, split))
    if orient and not has_stored_flip(root, split):
        raise SystemExit("--orient: %s holds no orientation flips for its %r split (pack --orient writes them)" % (path, split))
    try:
        return split_meshset(root, split, visible="stored" if visible else None, orient="stored" if orient else None)
    except ValueError as e:
        raise SystemExit(str(e)) from None


def _distance_main(argv):
    """distance CLOUDS.npy MESHES.npz: CLOUDS (S,N,3) or (S,3,N), in the meshes' frame."""
    import torch
    from .evaluation import surface_fidelity
    opts = _options(argv[2:], {"shape": None, "visible": False, "signed": False, "orient": False, "split": "val", "device": "cuda"},
                    ("--visible", "--signed", "--orient"))
    clouds = np.load(argv[0])
    if clouds.ndim != 3 or 3 not in clouds.shape[1:]:
        raise SystemExit("%s: clouds are (S,N,3) or (S,3,N), got %s" % (argv[0], clouds.shape))
    if clouds.shape[2] != 3:
        clouds = clouds.transpose(0, 2, 1)
    shape = _shape_option(opts["shape"])
    ms = _open_meshset(argv[1], opts["split"], opts["visible"], opts["orient"])
    ms = ms.oriented() if opts["orient"] else ms
    dev = torch.device(opts["device"])
    try:
        result = surface_fidelity(torch.from_numpy(np.ascontiguousarray(clouds, dtype=np.float32)).to(dev), ms.to(dev), shape,
                                  visible_only=opts["visible"], **({"signed": True} if opts["signed"] else {}))
    except ValueError as e:
        raise SystemExit(str(e)) from None
    print("\n".join(distance_table(result)))


def _occupancy_main(argv):
    """occupancy MESHES.npz OUT.npz --resolution R: OUT holds "occupancy" (S',ceil(R^3 / 8)) uint8 -- np.packbits of every shape's (R,R,R)
    grid in (x, y, z) order -- with "resolution", "origin" (S',3), "voxel" (S') and "shape" (S')."""
    import torch
    opts = _options(argv[2:], {"shape": None, "visible": False, "orient": False, "resolution": None, "split": "val", "device": "cuda"},
                    ("--visible", "--orient"), ("--shape", "--split", "--device", "--resolution"))
    if opts["resolution"] is None or not opts["resolution"].isdigit():
        raise SystemExit("occupancy takes --resolution R\n" + USAGE)
    shape = _shape_option(opts["shape"])
    ms = _open_meshset(argv[0], opts["split"], opts["visible"], opts["orient"]).to(torch.device(opts["device"]))
    ms = ms.oriented() if opts["orient"] else ms
    try:
        occ, origin, voxel = occupancy_grid(ms, shape, int(opts["resolution"]), visible_only=opts["visible"])
    except ValueError as e:
        raise SystemExit(str(e)) from None
    occ = occ.cpu().numpy()
    np.savez(argv[1], occupancy=np.packbits(occ.reshape(occ.shape[0], -1), axis=1), resolution=np.asarray(occ.shape[1]),
             origin=origin.cpu().numpy(), voxel=voxel.cpu().numpy(), shape=np.arange(ms.S) if shape is None else shape)
    print("%d grids of %d^3 cells into %s; cells inside: %s" % (occ.shape[0], occ.shape[1], argv[1],
                                                              " ".join(str(int(c)) for c in occ.reshape(occ.shape[0], -1).sum(axis=1))))


def _check_main(argv):
    """check MESHES.npz: `winding_report`, one row per shape; --orient: as stored and with the stored flips applied, side by side."""
    import torch
    opts = _options(argv[1:], {"samples": "4096", "orient": False, "split": "val", "device": "cuda"}, ("--orient",),
                    ("--samples", "--split", "--device"))
    if not opts["samples"].isdigit():
        raise SystemExit(USAGE)
    ms = _open_meshset(argv[0], opts["split"], False, opts["orient"]).to(torch.device(opts["device"]))
    verdict = lambda r: ("closed and consistently oriented" if r["fractional"].max() <= 0.01
                         else "open, self-intersecting or inconsistently oriented shapes: signs are not to be trusted")
    rep = winding_report(ms, int(opts["samples"]))
    if not opts["orient"]:
        print("shape %12s %12s %12s" % ("w_min", "w_max", "fractional"))
        for c in range(ms.S):
            print("%5d %12.6f %12.6f %12.4f" % (c, rep["w_min"][c], rep["w_max"][c], rep["fractional"][c]))
        print("worst fractional share %.4f: %s" % (rep["fractional"].max(), verdict(rep)))
        return
    after = winding_report(ms.oriented(), int(opts["samples"]))
    flipped = _per_shape(ms.flip.cpu().numpy().astype(np.int64), ms.face_off.cpu().numpy().astype(np.int64))
    print("shape %8s | %12s %12s %12s | %12s %12s %12s" % ("flipped", "w_min", "w_max", "fractional", "w_min", "w_max", "fractional"))
    print("      %8s | %38s | %38s" % ("", "as stored", "oriented"))
    for c in range(ms.S):
        print("%5d %8d | %12.6f %12.6f %12.4f | %12.6f %12.6f %12.4f" % (c, flipped[c], rep["w_min"][c], rep["w_max"][c], rep["fractional"][c],
                                                                       after["w_min"][c], after["w_max"][c], after["fractional"][c]))
    print("as stored: worst fractional share %.4f: %s" % (rep["fractional"].max(), verdict(rep)))
    print("oriented:  worst fractional share %.4f: %s" % (after["fractional"].max(), verdict(after)))


def _render_main(argv):
    """render MESHES.npz -o sheet.png: the shapes as flat-lit (or depth-shaded) triangles, `rows` down and up to `cols` across, column by
    column (report.MeshColumn, csrc/render.hip: pdgn_render_sheet_mesh); --visible: only the faces the sampler would draw from."""
    import torch
    from .report import MAX_COLUMNS, MESH_SHADES, MeshColumn, render_sheet, write_png
    opts = _options(argv[1:], {"o": "sheet.png", "shape": None, "visible": False, "split": "val", "device": "cuda", "rows": "8",
                               "cols": str(MAX_COLUMNS), "cell": "128", "shade": "flat", "orient": False}, ("--visible", "--orient"),
                    ("--shape", "--split", "--device", "--rows", "--cols", "--cell", "--shade", "--o"))
    if not all(opts[k].isdigit() and int(opts[k]) > 0 for k in ("rows", "cols", "cell")) or opts["shade"] not in MESH_SHADES:
        raise SystemExit(USAGE)
    ms = _open_meshset(argv[0], opts["split"], opts["visible"], opts["orient"])
    ms = ms.oriented() if opts["orient"] else ms
    if opts["visible"] and ms.visible is None:
        raise SystemExit("--visible: %s holds no visibility masks" % argv[0])
    try:
        picks = _shape_list(_shape_option(opts["shape"]), ms.S, "render")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    rows = min(int(opts["rows"]), len(picks))
    cols = min(int(opts["cols"]), MAX_COLUMNS, -(-len(picks) // rows))
    picks = np.asarray(picks, dtype=np.int64)[:rows * cols]
    ms = ms.to(torch.device(opts["device"]))
    off = ms.face_off.cpu().numpy().astype(np.int64)
    columns = []
    for j in range(cols):
        sub = picks[j * rows:(j + 1) * rows]
        begin, count = np.zeros(rows, np.int64), np.zeros(rows, np.int64)          # (the last column may end early: empty cells)
        begin[:len(sub)], count[:len(sub)] = off[sub], off[sub + 1] - off[sub]
        columns.append(MeshColumn(ms.verts, ms.faces, begin, count, np.zeros(rows, np.int64), ms.visible if opts["visible"] else None,
                                  opts["shade"]))
    sheet = render_sheet(columns, cell=int(opts["cell"]), fit=True)
    write_png(opts["o"], sheet)
    print("%s: %d shapes, %d x %d pixels" % (opts["o"], len(picks), sheet.shape[1], sheet.shape[0]))
    return opts["o"]


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) >= 2 and argv[0] == "render":
        return _render_main([a if a != "-o" else "--o" for a in argv[1:]])
    if len(argv) >= 3 and argv[0] == "distance":
        return _distance_main(argv[1:])
    if len(argv) >= 3 and argv[0] == "occupancy":
        return _occupancy_main(argv[1:])
    if len(argv) >= 2 and argv[0] == "check":
        return _check_main(argv[1:])
    if len(argv) < 3 or argv[0] != "pack":
        raise SystemExit(USAGE)
    opts, rest, given, orient = {"views": 26, "resolution": 128}, argv[3:], False, False
    while rest:
        flag = rest.pop(0)
        if flag == "--visible":
            given = True
        elif flag == "--orient":
            orient = True
        elif flag in ("--views", "--resolution") and rest and rest[0].isdigit():
            opts[flag[2:]] = int(rest.pop(0))
        else:
            raise SystemExit(USAGE)
    if not (given or orient) and opts != {"views": 26, "resolution": 128}:
        raise SystemExit("--views and --resolution go with --visible or --orient\n" + USAGE)
    said = lambda sid, split, r: print("%s/%s: %d of %d faces flipped, %d undecided, %d two-sided" % (
        sid, split, int(r["flip"].sum()), r["flip"].shape[0], int(r["undecided"].sum()), int(r["two_sided"].sum())))
    keys = pack(argv[1], argv[2], opts if given else None, dict(opts) if orient else None, said)
    print("packed %d arrays into %s" % (len(keys), argv[2]))


if __name__ == "__main__":
    main()
