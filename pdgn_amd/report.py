"""Snapshot reports of a training run, written by the training process itself: a preview sheet of what the generator makes at
all four resolutions (csrc/render.hip, pdgn_render_sheet -> an 8-bit grey PNG) and one line of cheap held-out metrics
(CD-only MMD / COV / 1-NNA and JSD: the all-pairs Chamfer pair-list kernel, never the EMD kernel).

    reporter = SnapshotReporter(trainer, val_clouds, out_dir, every=20, batch_size=35, normalize="shape_bbox", seed=9999)
    trainer.fit(feeder, epochs, on_epoch=reporter)
    python -m pdgn_amd.train ... --report_every 20
    python -m pdgn_amd.report results/GEN_Ours_chair_<time>/out.npy -o sheet.png [--lit] [--mesh R]

A column of a sheet may be a list of triangle meshes (`MeshColumn`: pdgn_render_sheet_mesh) -- a reconstruction
beside its cloud, the shapes of a meshes.MeshSet; `SnapshotReporter(mesh=R)` / `--report_mesh` adds the former to every preview.

A report does not touch training: it runs under no_grad in eval mode after a device synchronise, draws from generators of its
own (torch's global RNG state is left alone), and leaves every parameter, buffer and optimizer state as it found them
(DESIGN.md section 7c).  Where the trainer keeps an averaged generator (`PDGNTrainer(ema_decay=...)`, section 7d) the sheet and the
metrics are the averaged generator's: the report runs inside `trainer.averaged_generator()`, and the averages are left as found too.
"""
import argparse
import contextlib
import ctypes
import math
import os
import struct
import sys
import time
import zlib

import numpy as np
import torch

from . import _lib

MAX_COLUMNS = 8
QUICK_KEYS = ("lgan_mmd-CD", "lgan_cov-CD", "lgan_mmd_smp-CD", "1-NN-CD-acc_t", "1-NN-CD-acc_f", "1-NN-CD-acc", "jsd")
FULL_KEYS = QUICK_KEYS[:3] + ("lgan_mmd-EMD", "lgan_cov-EMD", "lgan_mmd_smp-EMD") + QUICK_KEYS[3:6] + (
    "1-NN-EMD-acc_t", "1-NN-EMD-acc_f", "1-NN-EMD-acc", "jsd")


# ---------------------------------------------------------------------------- the sheet
def default_view(cell=128, yaw=-35.0, pitch=25.0, fill=0.48):
    """The fixed three-quarter view: a 3 x 4 fp32 matrix (rows: pixel column u, pixel row v, depth d in [0, 1] with 0 nearest;
    include/pdgn_hip.h, pdgn_render_sheet) that maps a cloud inside the unit sphere into a cell of `cell` pixels.  The cloud's
    y axis points up (ShapeNetCore.GRAVITATIONAL_AXIS); the camera turns `yaw` degrees about it, then tilts `pitch` degrees
    down; orthographic, the unit sphere spans `fill` * cell pixels either side of the cell's centre.  Built in fp32."""
    f = np.float32
    cy, sy = f(math.cos(math.radians(yaw))), f(math.sin(math.radians(yaw)))
    cp, sp = f(math.cos(math.radians(pitch))), f(math.sin(math.radians(pitch)))
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=f)
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]], dtype=f)
    cam = rx @ ry                                                # camera axes: x right, y up, z towards the viewer
    s, half = f(fill) * f(cell), f(cell) * f(0.5)
    view = np.zeros((3, 4), dtype=f)
    view[0, :3], view[0, 3] = s * cam[0], half
    view[1, :3], view[1, 3] = -s * cam[1], half                  # image rows grow downwards
    view[2, :3], view[2, 3] = f(-0.5) * cam[2], f(0.5)
    return view


def fit_unit_sphere(pcs):
    """(B, N, 3) -> each cloud centred on its bounding box and scaled to touch the unit sphere (what `default_view` frames)."""
    lo, hi = pcs.min(dim=1, keepdim=True)[0], pcs.max(dim=1, keepdim=True)[0]
    centred = pcs - (lo + hi) / 2
    return (centred / centred.norm(dim=2).max(dim=1)[0].clamp_min(1e-12).view(-1, 1, 1)).contiguous()


def fit_frames(pcs):
    """(B, N, 3) -> (centre (B,3), scale (B)): what `fit_unit_sphere` applies, (pcs - centre) / scale in its own operations -- the frame a
    `MeshColumn.in_frames` takes, so that a cloud column and a mesh of it are drawn in one frame."""
    lo, hi = pcs.min(dim=1, keepdim=True)[0], pcs.max(dim=1, keepdim=True)[0]
    centre = (lo + hi) / 2
    return centre.reshape(-1, 3), (pcs - centre).norm(dim=2).max(dim=1)[0].clamp_min(1e-12)


MESH_SHADES = {"flat": 0, "depth": 1}


class MeshColumn:
    """One column of triangle meshes for `render_sheet` (csrc/render.hip: pdgn_render_sheet_mesh): verts (V,3) fp32,
    faces (F,3) int32, and per row of the sheet face_begin, face_count and vert_base (B integers each; tensors or sequences): row b draws
    the faces face_begin[b] .. face_begin[b] + face_count[b] - 1 with vert_base[b] added to their indices; a row with face_count 0 is an
    empty cell.  mask: (F) int32 or None, a face whose word is 0 is not drawn.  shade: "flat" (one shade per face from its normal and the
    sheet's light, the default) or "depth".  Built on the host or on the device; `render_sheet` wants it on the clouds' device."""

    def __init__(self, verts, faces, face_begin, face_count, vert_base, mask=None, shade="flat"):
        if shade not in MESH_SHADES:
            raise ValueError("MeshColumn: shade is \"flat\" or \"depth\", got %r" % (shade,))
        for name, t in (("verts", verts), ("faces", faces)) + ((("mask", mask),) if mask is not None else ()):
            if not isinstance(t, torch.Tensor):
                raise TypeError("MeshColumn: %s must be a torch.Tensor" % name)
        if verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3:
            raise ValueError("MeshColumn: verts must be fp32 (V,3), got %s %s" % (verts.dtype, tuple(verts.shape)))
        if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
            raise ValueError("MeshColumn: faces must be int32 (F,3), got %s %s" % (faces.dtype, tuple(faces.shape)))
        if mask is not None and (mask.dtype != torch.int32 or tuple(mask.shape) != (faces.shape[0],)):
            raise ValueError("MeshColumn: mask must be int32 (F) = (%d), got %s %s" % (faces.shape[0], mask.dtype, tuple(mask.shape)))
        parts = []
        for name, t in (("face_begin", face_begin), ("face_count", face_count), ("vert_base", vert_base)):
            t = torch.as_tensor(t)
            if t.dim() != 1 or t.dtype not in (torch.int32, torch.int64) or t.shape[0] < 1:
                raise ValueError("MeshColumn: %s must be (B) integers, got %s %s" % (name, t.dtype, tuple(t.shape)))
            parts.append(t.to(device=verts.device, dtype=torch.int32))
        if not parts[0].shape == parts[1].shape == parts[2].shape:
            raise ValueError("MeshColumn: face_begin, face_count and vert_base must hold one entry per row, got %s" % ([tuple(t.shape) for t in parts],))
        if not (faces.device == verts.device and (mask is None or mask.device == verts.device)):
            raise ValueError("MeshColumn: verts, faces and mask must live on one device")
        self.verts, self.faces, self.mask, self.shade = verts.contiguous(), faces.contiguous(), None if mask is None else mask.contiguous(), shade
        self.range = torch.stack(parts, dim=1).contiguous()     # (B,3) int32: (first face, face count, vertex base)
        self.rows = int(self.range.shape[0])

    face_begin = property(lambda self: self.range[:, 0])
    face_count = property(lambda self: self.range[:, 1])
    vert_base = property(lambda self: self.range[:, 2])

    @classmethod
    def from_surface_nets(cls, verts, faces, vert_off, face_off, mask=None, shade="flat"):
        """reconstruct.surface_nets' (or reconstruct's) result as it is: indices local to their cloud, the base of row b is vert_off[b]."""
        vert_off, face_off = torch.as_tensor(vert_off), torch.as_tensor(face_off)
        if vert_off.dim() != 1 or vert_off.shape != face_off.shape or vert_off.shape[0] < 2:
            raise ValueError("MeshColumn.from_surface_nets: vert_off and face_off are (B+1) offsets, got %s and %s" % (tuple(vert_off.shape), tuple(face_off.shape)))
        return cls(verts, faces, face_off[:-1], face_off[1:] - face_off[:-1], vert_off[:-1], mask, shade)

    @classmethod
    def from_meshset(cls, meshset, shape=None, visible_only=False, shade="flat"):
        """Shapes of a meshes.MeshSet, one per row: global indices, base 0.  shape: None (every shape of the set, in order) or (B) integers
        (meshes._shape_argument's forms); visible_only: only the faces whose view mask is not 0 are drawn (the set must hold masks)."""
        from .meshes import _shape_argument
        if visible_only and meshset.visible is None:
            raise ValueError("MeshColumn.from_meshset: visible_only needs a mesh set built with visibility masks")
        B = meshset.S if shape is None else len(shape)
        pick = torch.from_numpy(_shape_argument(shape, B, meshset.S, "MeshColumn.from_meshset")).to(meshset.face_off.device)
        off = meshset.face_off.long()
        return cls(meshset.verts, meshset.faces, off[pick], off[pick + 1] - off[pick], torch.zeros_like(pick),
                   meshset.visible if visible_only else None, shade)

    def _corners(self):
        """(row (T) int64, vertex (T) int64) of every corner of every face the rows draw that names a vertex inside the array."""
        dev = self.verts.device
        F, V = int(self.faces.shape[0]), int(self.verts.shape[0])
        begin = self.range[:, 0].long().clamp(0, F)
        end = (self.range[:, 0].long() + self.range[:, 1].long().clamp_min(0)).clamp(0, F)
        count = (end - begin).clamp_min(0)
        row = torch.repeat_interleave(torch.arange(self.rows, device=dev), count)
        start = torch.cumsum(count, 0) - count
        face = begin[row] + (torch.arange(int(row.shape[0]), device=dev) - start[row])
        vid = self.faces[face].long() + self.range[:, 2].long()[row][:, None]
        ok = ((vid >= 0) & (vid < V)).all(dim=1)
        return row[ok].repeat_interleave(3), vid[ok].reshape(-1)

    def frames(self):
        """(centre (B,3), scale (B)) that `fitted` applies: per row the centre of the box of the vertices its faces use and their largest
        distance from it (NaN / 1e-12 for a row without a face)."""
        row, vid = self._corners()
        pts = self.verts[vid]
        idx = row[:, None].expand(-1, 3)
        lo = torch.full((self.rows, 3), float("inf"), device=pts.device).scatter_reduce(0, idx, pts, "amin")
        hi = torch.full((self.rows, 3), float("-inf"), device=pts.device).scatter_reduce(0, idx, pts, "amax")
        centre = (lo + hi) / 2
        reach = torch.zeros(self.rows, device=pts.device).scatter_reduce(0, row, (pts - centre[row]).norm(dim=1), "amax")
        return centre, reach.clamp_min(1e-12)

    def in_frames(self, centre, scale):
        """The same column with every vertex v that row b's faces use at (v - centre[b]) / scale[b], in fp32: centre (B,3), scale (B)
        (`fit_frames` of the clouds the meshes belong to).  A copy of verts; faces, ranges and mask are shared.  Rows own their vertices
        (those of a MeshSet and of surface nets do): a vertex two rows use takes the frame of one of them."""
        centre = torch.as_tensor(centre, dtype=torch.float32, device=self.verts.device).reshape(self.rows, 3)
        scale = torch.as_tensor(scale, dtype=torch.float32, device=self.verts.device).reshape(self.rows)
        row, vid = self._corners()
        verts = self.verts.clone()
        verts[vid] = (self.verts[vid] - centre[row]) / scale[row][:, None]
        out = MeshColumn.__new__(MeshColumn)
        out.verts, out.faces, out.mask, out.shade, out.range, out.rows = verts, self.faces, self.mask, self.shade, self.range, self.rows
        return out

    def fitted(self):
        """Every row centred on the box of its vertices and scaled to touch the unit sphere: `fit_unit_sphere` for meshes."""
        return self.in_frames(*self.frames())

    def to(self, device):
        out = MeshColumn.__new__(MeshColumn)
        out.verts, out.faces, out.range = self.verts.to(device), self.faces.to(device), self.range.to(device)
        out.mask, out.shade, out.rows = None if self.mask is None else self.mask.to(device), self.shade, self.rows
        return out


def _column(t, name, fit):
    """One cloud list as the kernel takes it: (tensor whose memory is (B,N,3) or (B,3,N) contiguous, N, channel_major)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise _lib.PdgnHipError("%s must live on a ROCm device (pdgn_amd has no CPU path)" % name)
    if t.dtype != torch.float32 or t.dim() != 3 or 3 not in t.shape[1:]:
        raise ValueError("%s must be fp32 (B,3,N) or (B,N,3), got %s %s" % (name, t.dtype, tuple(t.shape)))
    point_major = t.shape[2] == 3                                # (B,3,3) reads as point-major
    if fit:
        return fit_unit_sphere(t if point_major else t.transpose(1, 2)), (t.shape[1] if point_major else t.shape[2]), False
    n = t.shape[1] if point_major else t.shape[2]
    if t.is_contiguous():
        return t, n, not point_major
    if t.transpose(1, 2).is_contiguous():                        # the generator's outputs: (B,3,N) views of (B,N,3) memory
        return t, n, point_major
    return t.contiguous(), n, not point_major


def _normals_form(normals, ncols, k):
    """The form of render_sheet's `normals` argument, checked before anything touches the device -> a list of `ncols` entries."""
    if isinstance(normals, str):
        normals = [normals] * ncols
    if isinstance(normals, torch.Tensor) or not isinstance(normals, (list, tuple)) or len(normals) != ncols:
        raise ValueError("normals must be None, \"estimate\" or a list with one entry per cloud list (%d)" % ncols)
    for i, entry in enumerate(normals):
        if isinstance(entry, str) and entry != "estimate":
            raise ValueError("normals[%d]: %r is not \"estimate\"" % (i, entry))
        if entry is not None and not isinstance(entry, (str, torch.Tensor)):
            raise TypeError("normals[%d] must be a torch.Tensor, \"estimate\" or None" % i)
    if int(k) < 1:
        raise ValueError("normals_k must be at least 1, got %r" % (k,))
    return list(normals)


def _normals(normals, held, k, B, dev):
    """render_sheet's `normals` argument (a list: _normals_form) -> one (B,N,3) contiguous fp32 tensor or None per column."""
    from .pointops import estimate_normals
    out = []
    for i, (entry, column) in enumerate(zip(normals, held)):
        if entry is None:                                        # (a mesh column's entry is None and so is what is held of it)
            out.append(None)
            continue
        t, n, cm = column
        if isinstance(entry, str):
            pts = (t if t.shape[2] == 3 else t.transpose(1, 2)).contiguous()     # point-major, as _column reads the shape
            out.append(estimate_normals(pts, min(int(k), n)))
        else:
            if not entry.is_cuda:
                raise _lib.PdgnHipError("normals[%d] must live on a ROCm device (pdgn_amd has no CPU path)" % i)
            if entry.dtype != torch.float32 or tuple(entry.shape) != (B, n, 3) or entry.device != dev:
                raise ValueError("normals[%d] must be fp32 (%d,%d,3) on the clouds' device, got %s %s" % (i, B, n, entry.dtype, tuple(entry.shape)))
            out.append(entry.contiguous())
    return out


def _light(v, from_view):
    """The light's direction as the kernel takes it: three fp32 numbers of unit length (from_view: v is the 3 x 4 view, whose depth row
    is the viewing direction)."""
    v = np.asarray(v, dtype=np.float32)
    v = v[2, :3] if from_view else v.reshape(-1)
    if v.shape != (3,) or not np.isfinite(v).all() or not np.any(v != 0):
        raise ValueError("light must be three finite numbers, not all zero, got %r" % (v,))
    return np.ascontiguousarray(v / np.sqrt((v * v).sum(dtype=np.float32)), dtype=np.float32)


def render_sheet(clouds, view=None, cell=128, radius=1, fit=False, normals=None, normals_k=16, light=None):
    """A contact sheet of clouds: one row per sample, one column per entry of `clouds` (a tensor, or a list of up to 8; each
    (B,3,N) -- the reference's layout, the generator's outputs as they are -- or point-major (B,N,3), fp32 on the device, the
    same B) -> (B * cell, len(clouds) * cell) uint8 device tensor.  view: 3 x 4 fp32 (default `default_view(cell)`); radius: the
    splat's radius in pixels; fit: centre and scale every cloud into the unit sphere first.  One launch sequence on the current
    stream; bitwise repeatable.
    normals: None -- every column shaded by depth, pdgn_render_sheet, what this function always did -- or, for sheets lit by their surface
    normals (pdgn_render_sheet_lit, DESIGN.md section 7q: two-sided, so the normals need no consistent orientation), "estimate" (every
    column: pointops.estimate_normals of the cloud as it is drawn, from its `normals_k` nearest neighbours) or a list with one entry per
    column: a (B,N,3) fp32 tensor of the column's normals, point-major whatever the cloud's layout, "estimate", or None (that column stays
    shaded by depth).  light: three numbers, the direction of the light, normalised here in fp32; default: the viewing direction, `view`
    row 2's first three entries.
    An entry of `clouds` may be a `MeshColumn`: that column shows triangle meshes, one per row, rasterised into the same sheet
    (pdgn_render_sheet_mesh), flat-lit by `light` or shaded by depth as the column says; fit=True fits it with
    `MeshColumn.fitted()`; its entry of a `normals` list must be None ("estimate" for every column means every CLOUD column).  A sheet
    without a MeshColumn goes through the entry points it always went through."""
    cols = [clouds] if isinstance(clouds, torch.Tensor) else list(clouds)
    if not 1 <= len(cols) <= MAX_COLUMNS:
        raise ValueError("render_sheet takes 1 to %d cloud lists, got %d" % (MAX_COLUMNS, len(cols)))
    view = np.ascontiguousarray(np.asarray(default_view(cell) if view is None else view, dtype=np.float32))
    if view.shape != (3, 4):
        raise ValueError("view must be 3 x 4, got %s" % (view.shape,))
    if any(isinstance(c, MeshColumn) for c in cols):
        return _render_sheet_mesh(cols, view, cell, radius, fit, normals, normals_k, light)
    if normals is not None:
        normals = _normals_form(normals, len(cols), normals_k)
        light = _light(view if light is None else light, light is None)
    held = [_column(t, "clouds[%d]" % i, fit) for i, t in enumerate(cols)]
    B, dev = cols[0].shape[0], cols[0].device
    if any(t.shape[0] != B or t.device != dev for t in cols):
        raise ValueError("every cloud list must hold the same number of clouds on the same device")
    if normals is not None:
        normals = _normals(normals, held, normals_k, B, dev)
    L = _lib.lib()
    nbytes = L.pdgn_render_workspace_bytes(B, len(cols), int(cell))
    if nbytes < 0:
        raise _lib.PdgnHipError("pdgn_render_workspace_bytes: argument outside the supported range")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        image = torch.empty((B * int(cell), len(cols) * int(cell)), dtype=torch.uint8, device=dev)
        ptrs = (ctypes.c_void_p * len(cols))(*[t.data_ptr() for t, _, _ in held])
        counts = (ctypes.c_int * len(cols))(*[n for _, n, _ in held])
        mask = sum(1 << i for i, (_, _, cm) in enumerate(held) if cm)
        if normals is not None:
            nptrs = (ctypes.c_void_p * len(cols))(*[None if t is None else t.data_ptr() for t in normals])
            _lib.check(L.pdgn_render_sheet_lit(B, len(cols), ptrs, nptrs, counts, mask, view.ctypes.data_as(ctypes.c_void_p),
                                               light.ctypes.data_as(ctypes.c_void_p), int(cell), int(radius), _lib.ptr(ws), _lib.ptr(image),
                                               _lib.stream_of(image)), "pdgn_render_sheet_lit")
            return image
        _lib.check(L.pdgn_render_sheet(B, len(cols), ptrs, counts, mask, view.ctypes.data_as(ctypes.c_void_p), int(cell), int(radius),
                                       _lib.ptr(ws), _lib.ptr(image), _lib.stream_of(image)), "pdgn_render_sheet")
    return image


def _render_sheet_mesh(cols, view, cell, radius, fit, normals, normals_k, light):
    """render_sheet for a sheet with at least one MeshColumn: pdgn_render_sheet_mesh.  The form of every argument is checked before
    anything touches the device."""
    ncols = len(cols)
    is_mesh = [isinstance(c, MeshColumn) for c in cols]
    if isinstance(normals, str):                                 # "estimate": every cloud column
        normals = [None if m else normals for m in is_mesh]
    if normals is not None:
        normals = _normals_form(normals, ncols, normals_k)
        for i, m in enumerate(is_mesh):
            if m and normals[i] is not None:
                raise ValueError("normals[%d] must be None: clouds[%d] is a MeshColumn, which is shaded from its faces" % (i, i))
    light = _light(view if light is None else light, light is None)
    rows = []
    for i, c in enumerate(cols):
        if is_mesh[i]:
            rows.append(c.rows)
            continue
        if not isinstance(c, torch.Tensor):
            raise TypeError("clouds[%d] must be a torch.Tensor or a MeshColumn" % i)
        if c.dtype != torch.float32 or c.dim() != 3 or 3 not in c.shape[1:]:
            raise ValueError("clouds[%d] must be fp32 (B,3,N) or (B,N,3), got %s %s" % (i, c.dtype, tuple(c.shape)))
        rows.append(int(c.shape[0]))
    B = rows[0]
    if any(r != B for r in rows):
        raise ValueError("every column must hold the same number of rows, got %s" % (rows,))
    devices = [(c.verts if m else c).device for c, m in zip(cols, is_mesh)]
    dev = devices[0]
    if dev.type != "cuda":
        raise _lib.PdgnHipError("clouds[0] must live on a ROCm device (pdgn_amd has no CPU path)")
    if any(d != dev for d in devices):
        raise ValueError("every column must live on the same device")
    held = [None if m else _column(c, "clouds[%d]" % i, fit) for i, (c, m) in enumerate(zip(cols, is_mesh))]
    meshes = [(c.fitted() if fit else c) if m else None for c, m in zip(cols, is_mesh)]
    normals = [None] * ncols if normals is None else _normals(normals, held, normals_k, B, dev)
    L = _lib.lib()
    nbytes = L.pdgn_render_workspace_bytes(B, ncols, int(cell))
    if nbytes < 0:
        raise _lib.PdgnHipError("pdgn_render_workspace_bytes: argument outside the supported range")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        image = torch.empty((B * int(cell), ncols * int(cell)), dtype=torch.uint8, device=dev)
        one = torch.zeros((1, 3), dtype=torch.float32, device=dev)               # the vertex array of a column that has no vertex at all
        voidp, ints = ctypes.c_void_p * ncols, ctypes.c_int * ncols
        verts = [None if m is None else (m.verts if m.verts.shape[0] else one) for m in meshes]
        ptrs = voidp(*[None if h is None else h[0].data_ptr() for h in held])
        nptrs = voidp(*[None if t is None else t.data_ptr() for t in normals])
        counts = ints(*[0 if h is None else h[1] for h in held])
        major = sum(1 << i for i, h in enumerate(held) if h is not None and h[2])
        mverts = voidp(*[None if v is None else v.data_ptr() for v in verts])
        mfaces = voidp(*[None if m is None or not m.faces.shape[0] else m.faces.data_ptr() for m in meshes])
        mrange = voidp(*[None if m is None else m.range.data_ptr() for m in meshes])
        mmask = voidp(*[None if m is None or m.mask is None or not m.faces.shape[0] else m.mask.data_ptr() for m in meshes])
        nverts = ints(*[0 if v is None else int(v.shape[0]) for v in verts])
        nfaces = ints(*[0 if m is None else int(m.faces.shape[0]) for m in meshes])
        shades = ints(*[0 if m is None else MESH_SHADES[m.shade] for m in meshes])
        _lib.check(L.pdgn_render_sheet_mesh(B, ncols, ptrs, nptrs, counts, major, mverts, mfaces, mrange, mmask, nverts, nfaces, shades,
                                            view.ctypes.data_as(ctypes.c_void_p), light.ctypes.data_as(ctypes.c_void_p), int(cell), int(radius),
                                            _lib.ptr(ws), _lib.ptr(image), _lib.stream_of(image)), "pdgn_render_sheet_mesh")
    return image


# ---------------------------------------------------------------------------- PNG (8-bit grey, filter type 0)
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, image):
    """A (H, W) uint8 array (numpy, or a tensor on any device) as an 8-bit greyscale PNG; zlib and struct only."""
    if isinstance(image, torch.Tensor):
        image = image.detach().cpu().numpy()
    image = np.ascontiguousarray(image)
    if image.dtype != np.uint8 or image.ndim != 2 or 0 in image.shape:
        raise ValueError("write_png takes a non-empty (H, W) uint8 image, got %s %s" % (image.dtype, image.shape))
    h, w = image.shape
    raw = np.zeros((h, w + 1), dtype=np.uint8)                   # every scanline starts with its filter type: 0, none
    raw[:, 1:] = image
    data = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(data)
    return path


# ---------------------------------------------------------------------------- cheap held-out metrics
@torch.no_grad()
def quick_metrics(generator, ref_pcs, batch_size, normalize=None, rng=None, cache=None):
    """The CD entries and the JSD of evaluation.generate_and_evaluate without its EMD passes: generation as there (sigma-1 noise
    from `rng`, the finest cloud, truncated to the reference set's size, normalised with `normalize`) with the generator in
    eval mode (its mode is put back), all-pairs Chamfer from the pair-list kernel (evaluation.pairwise_cd), the reductions of
    evaluation.reduce_metrics, under compute_all_metrics' keys (`QUICK_KEYS`).  cache: a dict that keeps what depends on the
    reference set alone -- its ref-vs-ref matrix and its occupancy counters -- between calls."""
    from . import evaluation as ev
    cache = {} if cache is None else cache
    ident = (ref_pcs.data_ptr(), tuple(ref_pcs.shape), ref_pcs._version)
    if cache.get("ref") != ident:
        cache.clear()
        cache["ref"] = ident
        cache["M_rr"] = ev.pairwise_cd(ref_pcs, ref_pcs)
        cache["ref_counters"] = ev.entropy_of_occupancy_grid(ref_pcs, 28, True)[1]
    was_training = generator.training
    generator.eval()
    try:
        gen_pcs, _ = ev.generate_clouds(generator, ref_pcs.shape[0], batch_size, normalize, rng, ref_pcs.device)
    finally:
        generator.train(was_training)
    M_rs = ev.pairwise_cd(gen_pcs, ref_pcs)
    M_ss = ev.pairwise_cd(gen_pcs, gen_pcs)
    cache["generated"] = (gen_pcs, M_rs)                         # (for SnapshotReporter(fidelity=...): the clouds and their Chamfer matrix)
    results = ev.reduce_metrics(M_rs.t(), cache["M_rr"], M_rs, M_ss, "CD")
    results["jsd"] = ev.jensen_shannon_divergence(ev.entropy_of_occupancy_grid(gen_pcs, 28, True)[1], cache["ref_counters"])
    return results


# ---------------------------------------------------------------------------- the fit hook
class SnapshotReporter:
    """`fit(on_epoch=SnapshotReporter(...))`: at every epoch that is a multiple of `every`, on rank 0, write
    `<out_dir>/preview_<epoch>.png` (`rows` samples down; the generator's four resolutions and a column of reference clouds
    across) and append a row to `<out_dir>/metrics.csv` (epoch, `QUICK_KEYS` -- with full=True `FULL_KEYS`, through
    compute_all_metrics and its EMD passes, the approximate EMD or with emd="auction" the exact one and an `emd-capped` column --
    and the seconds the report took).  The preview's noise and the metrics' noise
    come from generators seeded the same way at every report, so sheets and rows are comparable across epochs.  Training
    state is left as found; the generator's train / eval flag is put back.  spacing=True: every report also appends epoch, gen nn_mean,
    gen nn_cv, val nn_mean, val nn_cv, gen duplicates -- evaluation.spacing_stats of as many generated clouds as there are reference clouds
    (the metrics' noise stream, normalised like them) and of the reference clouds -- to `<out_dir>/spacing.csv`;
    metrics.csv is what it was.  lit=True: the sheet's columns are shaded by surface normals estimated from each cloud's 16 nearest
    neighbours (render_sheet(normals="estimate")) instead of by depth.  surface=True: every report also appends epoch,
    gen sv_mean, gen sv_p90, val sv_mean, val sv_p90, gen degenerate -- evaluation.surface_stats of the same generated clouds and of the
    reference clouds -- to `<out_dir>/surface.csv`.  With neither, every file is what it was.  fidelity=meshset: a
    meshes.MeshSet on the reference clouds' device whose shape c is the surface reference cloud c was drawn from, in the clouds' own frame
    (MeshSet.in_frame) -- the constructor measures the reference clouds against it and refuses a set they do not lie on.  Every report then
    appends epoch, gen acc_mean, gen acc_rms, gen acc_max, val acc_mean, val acc_rms, val acc_max to `<out_dir>/fidelity.csv`: the distance
    of every generated cloud's points to the surface of the validation shape nearest to it in the Chamfer matrix the report computes anyway
    (meshes.point_to_mesh; per cloud, then averaged over the clouds), and the same of the reference clouds against their own shapes -- the
    floor, a few ulps of the coordinates.  mesh=R: the sheet gets one more column after the reference clouds,
    reconstruct() of the finest generated clouds of its rows at grid resolution R as flat-lit triangles in those clouds' frames, and where
    fidelity= holds the validation shapes a further one, the first `rows` of them (only their visible faces where the set has masks): 6 or 7
    columns; a row whose reconstruction has no face is an empty cell.  None: every file is what it was."""
    FIDELITY_HEADER = ("epoch", "gen acc_mean", "gen acc_rms", "gen acc_max", "val acc_mean", "val acc_rms", "val acc_max")
    FIDELITY_FLOOR_ULPS = 256.0                                  # the kernel's own bound (64) and the roundings of the sampler and of the frame

    SPACING_HEADER = ("epoch", "gen nn_mean", "gen nn_cv", "val nn_mean", "val nn_cv", "gen duplicates")
    SURFACE_HEADER = ("epoch", "gen sv_mean", "gen sv_p90", "val sv_mean", "val sv_p90", "gen degenerate")

    def __init__(self, trainer, ref_pcs, out_dir, every, batch_size, normalize, seed, rows=8, full=False, rank=0, cell=128, radius=1, emd="approx",
                 spacing=False, lit=False, surface=False, fidelity=None, mesh=None):
        _lib.require(ref_pcs, "ref_pcs", torch.float32, 3)
        self.trainer, self.ref, self.out_dir = trainer, ref_pcs, str(out_dir)
        self.every, self.batch_size, self.normalize, self.seed = int(every), int(batch_size), normalize, int(seed)
        self.rows, self.full, self.rank, self.cell, self.radius = min(int(rows), ref_pcs.shape[0]), bool(full), int(rank), int(cell), int(radius)
        if self.rows < 1:
            raise ValueError("a report needs at least one row and one reference cloud")
        self.cache = {}
        from .evaluation import EMD_KINDS
        if emd not in EMD_KINDS:
            raise ValueError("emd must be one of %s, got %r" % (EMD_KINDS, emd))
        self.emd = emd
        self.keys = FULL_KEYS if self.full else QUICK_KEYS
        if self.full and self.emd == "auction":                  # the exact EMD's rows say how many pairs did not end at an optimum
            self.keys = self.keys + ("emd-capped",)
        self.last = None                                         # (epoch, {key: float}, seconds) of the latest report
        self.spacing = bool(spacing)
        self.last_spacing = None                                 # (epoch, generated clouds' stats, reference clouds' stats)
        self.lit, self.surface = bool(lit), bool(surface)
        self.last_surface = None                                 # (epoch, generated clouds' stats, reference clouds' stats)
        self.fidelity, self.last_fidelity = fidelity, None       # last: (epoch, generated clouds' (mean, rms, max), reference clouds')
        if fidelity is not None:
            self.fidelity_floor = self._check_fidelity(fidelity)
        self.mesh = None if mesh is None else int(mesh)           # the grid resolution of the sheet's reconstruction column
        if self.mesh is not None:
            from .reconstruct import _resolution
            _resolution(self.mesh, self.rows)

    def _mesh_sheet(self, outs):
        """The sheet with mesh=R: the cloud columns fitted as `render_sheet(fit=True)` fits them, then reconstruct() of the finest
        generated clouds at resolution R as flat-lit triangles in those clouds' frames, then (fidelity=) the first `rows` validation
        shapes themselves, fitted on their own.  A row whose reconstruction has no face is an empty cell."""
        from .reconstruct import reconstruct
        clouds = [(o if o.shape[2] == 3 else o.transpose(1, 2)).contiguous() for o in outs + [self.ref[:self.rows]]]
        finest = clouds[len(outs) - 1]
        columns = [fit_unit_sphere(c) for c in clouds]
        columns.append(MeshColumn.from_surface_nets(*reconstruct(finest, resolution=self.mesh)[:4]).in_frames(*fit_frames(finest)))
        if self.fidelity is not None:
            shapes = MeshColumn.from_meshset(self.fidelity, np.arange(self.rows), visible_only=self.fidelity.visible is not None)
            columns.append(shapes.fitted())
        return render_sheet(columns, cell=self.cell, radius=self.radius, **({"normals": "estimate"} if self.lit else {}))

    def _accuracy(self, clouds, shape=None):
        """(mean, rms, max) of the clouds' distance to their shapes of self.fidelity, per cloud and then averaged over the clouds."""
        from .evaluation import _distance_summary
        from .meshes import point_to_mesh
        out = {}
        d2, _ = point_to_mesh(clouds.contiguous(), self.fidelity, shape, visible_only=self.fidelity.visible is not None)
        _distance_summary(d2.double().sqrt(), "acc", out)
        return tuple(float(torch.nanmean(out[k])) for k in ("acc_mean", "acc_rms", "acc_max"))

    def _check_fidelity(self, fidelity):
        from .meshes import MeshSet
        if not isinstance(fidelity, MeshSet) or fidelity.S != self.ref.shape[0] or fidelity.verts.device != self.ref.device:
            raise ValueError("fidelity must be a MeshSet of the %d reference clouds' shapes on their device" % self.ref.shape[0])
        floor = self._accuracy(self.ref)
        most = max(float(self.ref.abs().max()), float(fidelity.verts[fidelity.faces.long().reshape(-1)].abs().max()))
        if not floor[2] <= self.FIDELITY_FLOOR_ULPS * 2.0 ** -24 * most:
            raise ValueError("fidelity: the reference clouds do not lie on the mesh set's shapes (largest distance %.3g, coordinates up to %.3g): "
                             "it must hold the shapes the clouds are draw 0 of, in the clouds' frame (MeshSet.in_frame)" % (floor[2], most))
        return floor

    def _generator(self, offset):
        return torch.Generator(device=self.ref.device).manual_seed(self.seed + offset)

    @torch.no_grad()
    def __call__(self, epoch):
        if self.every <= 0 or epoch % self.every or self.rank != 0:
            return None
        from . import evaluation as ev
        t0 = time.perf_counter()
        dev = self.ref.device
        torch.cuda.synchronize(dev)
        G = self.trainer.G
        was_training = G.training
        hints = G.forward_hints()                                # (what the eager step's next pre-assembly would read: generator.py)
        G.eval()
        # with an averaged generator the report shows THAT one (what one would evaluate or ship): its parameters by value for
        # the duration of the report, the live BatchNorm buffers
        averaged = self.trainer.averaged_generator() if getattr(self.trainer, "ema", None) is not None else contextlib.nullcontext()
        try:
            with averaged:
                z = torch.randn(self.rows, 128, generator=self._generator(0), device=dev)
                if self.mesh is not None:
                    sheet = self._mesh_sheet(list(G(z)))
                else:
                    sheet = render_sheet(list(G(z)) + [self.ref[:self.rows]], cell=self.cell, radius=self.radius, fit=True,
                                         **({"normals": "estimate"} if self.lit else {}))
                if self.full:
                    _, results = ev.generate_and_evaluate(G, self.ref, self.batch_size, self.normalize, self._generator(1), emd=self.emd)
                else:
                    results = quick_metrics(G, self.ref, self.batch_size, self.normalize, self._generator(1), self.cache)
                results = {k: float(results[k]) for k in self.keys}
                image = sheet.cpu().numpy()
                if self.spacing or self.surface or (self.fidelity is not None and self.full):
                    gen_pcs, _ = ev.generate_clouds(G, self.ref.shape[0], self.batch_size, self.normalize, self._generator(1), dev)
                if self.fidelity is not None:
                    # the clouds the metrics were computed on and their Chamfer matrix (the quick metrics keep both; the full ones do not)
                    clouds, M_rs = (gen_pcs, ev.pairwise_cd(gen_pcs, self.ref)) if self.full else self.cache["generated"]
                    fidelity = (self._accuracy(clouds, M_rs.argmin(dim=1)), self.fidelity_floor)
                if self.spacing:
                    if "val_spacing" not in self.cache:          # (the reference set does not change between reports)
                        self.cache["val_spacing"] = ev.spacing_stats(self.ref, self.batch_size)
                    spacing = (ev.spacing_stats(gen_pcs, self.batch_size), self.cache["val_spacing"])
                if self.surface:
                    if "val_surface" not in self.cache:
                        self.cache["val_surface"] = ev.surface_stats(self.ref, batch=self.batch_size)
                    surface = (ev.surface_stats(gen_pcs, batch=self.batch_size), self.cache["val_surface"])
        finally:
            G.train(was_training)
            G.restore_forward_hints(hints)
        os.makedirs(self.out_dir, exist_ok=True)
        write_png(os.path.join(self.out_dir, "preview_%d.png" % epoch), image)
        seconds = time.perf_counter() - t0
        path = os.path.join(self.out_dir, "metrics.csv")
        fresh = not os.path.exists(path) or os.path.getsize(path) == 0
        with open(path, "a") as f:
            if fresh:
                f.write(",".join(("epoch",) + self.keys + ("seconds",)) + "\n")
            f.write(",".join([str(epoch)] + ["%.9g" % results[k] for k in self.keys] + ["%.3f" % seconds]) + "\n")
        self.last = (epoch, results, seconds)
        if self.spacing:
            gen, val = spacing
            path = os.path.join(self.out_dir, "spacing.csv")
            fresh = not os.path.exists(path) or os.path.getsize(path) == 0
            with open(path, "a") as f:
                if fresh:
                    f.write(",".join(self.SPACING_HEADER) + "\n")
                f.write(",".join([str(epoch)] + ["%.9g" % v for v in (gen["nn_mean"], gen["nn_cv"], val["nn_mean"], val["nn_cv"])]
                                 + ["%d" % gen["duplicates"]]) + "\n")
            self.last_spacing = (epoch, gen, val)
        if self.surface:
            gen, val = surface
            path = os.path.join(self.out_dir, "surface.csv")
            fresh = not os.path.exists(path) or os.path.getsize(path) == 0
            with open(path, "a") as f:
                if fresh:
                    f.write(",".join(self.SURFACE_HEADER) + "\n")
                f.write(",".join([str(epoch)] + ["%.9g" % v for v in (gen["sv_mean"], gen["sv_p90"], val["sv_mean"], val["sv_p90"])]
                                 + ["%d" % gen["degenerate"]]) + "\n")
            self.last_surface = (epoch, gen, val)
        if self.fidelity is not None:
            gen, val = fidelity
            path = os.path.join(self.out_dir, "fidelity.csv")
            fresh = not os.path.exists(path) or os.path.getsize(path) == 0
            with open(path, "a") as f:
                if fresh:
                    f.write(",".join(self.FIDELITY_HEADER) + "\n")
                f.write(",".join([str(epoch)] + ["%.9g" % v for v in gen + val]) + "\n")
            self.last_fidelity = (epoch, gen, val)
        return self.last


# ---------------------------------------------------------------------------- python -m pdgn_amd.report
def build_parser():
    p = argparse.ArgumentParser(prog="python -m pdgn_amd.report", description="render a saved (S, N, 3) array of clouds (the test "
                                "phase's out.npy) as a preview sheet")
    p.add_argument("clouds", help=".npy file holding (S, N, 3) or (S, 3, N) clouds")
    p.add_argument("-o", "--output", default="sheet.png")
    p.add_argument("--rows", type=int, default=8, help="clouds per column")
    p.add_argument("--cols", type=int, default=MAX_COLUMNS, help="columns (at most %d)" % MAX_COLUMNS)
    p.add_argument("--cell", type=int, default=128, help="pixels per cell side")
    p.add_argument("--radius", type=int, default=1, help="splat radius in pixels")
    p.add_argument("--device", default="cuda")
    p.add_argument("--lit", action="store_true", help="shade by surface normals estimated from each cloud's 16 nearest neighbours (two-sided "
                   "headlight shading) instead of by depth")
    p.add_argument("--mesh", type=int, nargs="?", const=64, default=None, metavar="R", help="beside every cloud column, the surface reconstructed "
                   "from its clouds at grid resolution R (default 64) as flat-lit triangles in the clouds' frames; half as many cloud columns")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    pcs = np.load(args.clouds)
    if pcs.ndim != 3 or 3 not in pcs.shape[1:]:
        raise SystemExit("%s: expected (S, N, 3) or (S, 3, N), got %s" % (args.clouds, pcs.shape))
    if pcs.shape[2] != 3:
        pcs = pcs.transpose(0, 2, 1)
    rows = max(1, min(args.rows, pcs.shape[0]))
    cols = max(1, min(args.cols, MAX_COLUMNS // 2 if args.mesh is not None else MAX_COLUMNS, pcs.shape[0] // rows))
    dev = torch.device(args.device)
    pcs = torch.from_numpy(np.ascontiguousarray(pcs[:rows * cols], dtype=np.float32)).to(dev)
    if args.mesh is not None:
        from .reconstruct import reconstruct
        columns = []
        for j in range(cols):
            part = pcs[j * rows:(j + 1) * rows].contiguous()
            columns += [fit_unit_sphere(part), MeshColumn.from_surface_nets(*reconstruct(part, resolution=args.mesh)[:4]).in_frames(*fit_frames(part))]
        sheet = render_sheet(columns, cell=args.cell, radius=args.radius, **({"normals": "estimate"} if args.lit else {}))
    else:
        sheet = render_sheet([pcs[j * rows:(j + 1) * rows] for j in range(cols)], cell=args.cell, radius=args.radius, fit=True,
                             **({"normals": "estimate"} if args.lit else {}))
    write_png(args.output, sheet)
    print("%s: %d clouds, %d x %d pixels" % (args.output, rows * cols, sheet.shape[1], sheet.shape[0]))
    return args.output


if __name__ == "__main__":
    main()
    sys.exit(0)
