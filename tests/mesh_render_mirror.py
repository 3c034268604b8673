"""numpy restatement of the triangle rasteriser of csrc/render.hip (include/pdgn_hip.h: pdgn_render_sheet_mesh), on
top of tests/render_mirror.py and tests/normals_mirror.py, which spell the cloud columns: the operation order of the kernel's header
block, np.float32 arithmetic up to the snap and in the flat shade, int64 after the snap.  The fused multiply-adds of the projection are
exact here for any input (`fma32`), not only for the lattice inputs render_mirror's own `_fma` is exact on.  Used by
tests/test_mesh_render_host.py and tests/test_gpu_mesh_render.py; imports nothing of pdgn_amd."""
import numpy as np

import normals_mirror as nm
import render_mirror as rm

F = np.float32
SUB = 16                                                          # 4 sub-pixel bits
SMALL_BOX = 32                                                    # the kernel's lane / wave threshold (MESH_SMALL_BOX): pixels of the clipped box
SHADES = {"flat": 0, "depth": 1}


def fma32(a, b, c):
    """a * b + c with ONE rounding to fp32, for fp32 a, b, c.  The product is exact in fp64; the fp64 sum is rounded to odd (Boldo and
    Melquiond 2008: its error, exact from the two-sum, moves an inexact even result to its odd neighbour), and fp64 rounded to odd and
    then to nearest in fp32 is the correctly rounded fp32 result, fp64 having more than two bits beyond fp32's."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        odd = np.where(err > 0, np.nextafter(s, np.inf), np.nextafter(s, -np.inf))
        return np.where(fix, odd, s).astype(F)


def project(pts, view):
    """pts (..., 3) fp32, view (3, 4) -> u, v, d in fp32: the __fmaf_rn chain of render_splat_kernel."""
    pts = np.asarray(pts, dtype=F)
    m = np.asarray(view, dtype=F)
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    return tuple(fma32(m[r, 2], z, fma32(m[r, 1], y, fma32(m[r, 0], x, m[r, 3]))) for r in range(3))


def depth_q(d):
    """The splat's q of a finite depth: min((unsigned)(clamp(d, 0, 1) * 2^24), 2^24 - 1)."""
    dc = np.clip(np.asarray(d, F), F(0), F(1)).astype(F)
    return np.minimum((dc * F(16777216.0)).astype(np.int64), 0xFFFFFF)


def snap(pts, view, cell):
    """-> X, Y, Z (int64) and `finite` (bool) per vertex; X, Y, Z are 0 where the vertex is not finite."""
    u, v, d = project(pts, view)
    finite = np.isfinite(u) & np.isfinite(v) & np.isfinite(d)
    s = F(SUB * cell)
    with np.errstate(all="ignore"):
        X = np.clip(np.rint(np.where(finite, u, F(0)) * F(16)), -s, F(2) * s).astype(np.int64)
        Y = np.clip(np.rint(np.where(finite, v, F(0)) * F(16)), -s, F(2) * s).astype(np.int64)
    Z = depth_q(np.where(finite, d, F(0)))
    return X, Y, Z, finite


def flat_shade(p0, p1, p2, light):
    """The flat-lit shade of faces with fp32 corners p0, p1, p2 (F, 3) -> (shade (F) uint32, alive (F) bool)."""
    l = np.asarray(light, dtype=F).reshape(3)
    with np.errstate(all="ignore"):
        e1, e2 = (p1 - p0).astype(F), (p2 - p0).astype(F)
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        alive = (length > 0) & np.isfinite(length)
        c = np.abs((nx * l[0] + ny * l[1]) + nz * l[2]) / length
        c = np.where(c >= 0, c, F(0.0)).astype(F)
        c = np.where(c > 1, F(1.0), c).astype(F)
        shade = np.uint32(48) + (F(207.0) * np.where(alive, c, F(0))).astype(np.uint32)
    assert nx.dtype == F and length.dtype == F and c.dtype == F
    return shade, alive


def edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def face_setup(verts, faces, base, mask, shade, view, light, cell):
    """Everything of a list of faces that does not depend on the pixel: a list with one entry per face, None for a dead one, else
    (P0, P1, P2 as (X, Y, Z) Python ints after the swap, A2, the flat shade, (bx, by, bw, bh) the clipped box)."""
    verts = np.ascontiguousarray(verts, dtype=F).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = verts.shape[0]
    idx = faces + int(base)
    alive = ((idx >= 0) & (idx < V)).all(axis=1)
    if mask is not None:
        alive &= np.asarray(mask).reshape(-1) != 0
    safe = np.where(alive[:, None], idx, 0)
    p = verts[safe]                                               # (F, 3 corners, 3)
    X, Y, Z, finite = snap(p, view, cell)
    alive &= finite.all(axis=1)
    tone = np.zeros(faces.shape[0], np.uint32)
    if shade == "flat":
        tone, lit = flat_shade(p[:, 0], p[:, 1], p[:, 2], light)
        alive &= lit
    else:
        assert shade == "depth", shade
    out = []
    for f in range(faces.shape[0]):
        if not alive[f]:
            out.append(None)
            continue
        P = [(int(X[f, k]), int(Y[f, k]), int(Z[f, k])) for k in range(3)]
        a2 = edge(P[0][0], P[0][1], P[1][0], P[1][1], P[2][0], P[2][1])
        if a2 < 0:
            P[1], P[2], a2 = P[2], P[1], -a2
        box = (0, 0, 0, 0)
        if a2 != 0:
            xs, ys = [q[0] for q in P], [q[1] for q in P]
            px0, px1 = max((min(xs) + 7) >> 4, 0), min((max(xs) - 8) >> 4, cell - 1)
            py0, py1 = max((min(ys) + 7) >> 4, 0), min((max(ys) - 8) >> 4, cell - 1)
            if px1 >= px0 and py1 >= py0:
                box = (px0, py0, px1 - px0 + 1, py1 - py0 + 1)
        out.append((P[0], P[1], P[2], a2, int(tone[f]), box))
    return out


def draw_faces(cellkeys, setup, shade):
    """Rasterise `face_setup`'s faces into one cell's (cell, cell) uint32 keys, in place."""
    for t in setup:
        if t is None:
            continue
        P0, P1, P2, a2, tone, (bx, by, bw, bh) = t
        if a2 == 0 or bw * bh == 0:
            continue
        px, py = np.meshgrid(np.arange(bx, bx + bw, dtype=np.int64), np.arange(by, by + bh, dtype=np.int64))
        cx, cy = (2 * px + 1) * 8, (2 * py + 1) * 8
        w0 = edge(P1[0], P1[1], P2[0], P2[1], cx, cy)
        w1 = edge(P2[0], P2[1], P0[0], P0[1], cx, cy)
        w2 = edge(P0[0], P0[1], P1[0], P1[1], cx, cy)
        assert np.array_equal(w0 + w1 + w2, np.full_like(w0, a2))
        cov = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
        num = w0 * P0[2] + w1 * P1[2] + w2 * P2[2]               # below 2^61
        q = (num[cov] // a2).astype(np.uint32)
        tones = np.uint32(255) - (q >> np.uint32(17)) if shade == "depth" else np.uint32(tone)
        np.minimum.at(cellkeys, (py[cov], px[cov]), (q << np.uint32(8)) | tones)


def mesh_column(verts, faces, ranges, mask=None, shade="flat"):
    """A mesh column of `sheet_keys`: verts (V,3), faces (F,3), ranges (rows,3) = (first face, face count, vertex base)."""
    return {"verts": np.ascontiguousarray(verts, dtype=F).reshape(-1, 3), "faces": np.asarray(faces, dtype=np.int64).reshape(-1, 3),
            "range": np.asarray(ranges, dtype=np.int64).reshape(-1, 3), "mask": None if mask is None else np.asarray(mask).reshape(-1),
            "shade": shade}


def sheet_keys(columns, view, light, cell, radius=1):
    """columns: a list whose entries are a `mesh_column`, a cloud (B, N, 3) array, or a (cloud, normals (B, N, 3) or None) pair ->
    (B * cell, len(columns) * cell) uint32 keys."""
    rows = [c["range"].shape[0] if isinstance(c, dict) else (c[0] if isinstance(c, tuple) else c).shape[0] for c in columns]
    B = rows[0]
    assert all(r == B for r in rows)
    keys = np.full((B * cell, len(columns) * cell), rm.EMPTY, dtype=np.uint32)
    for c, col in enumerate(columns):
        if not isinstance(col, dict):
            pts, normals = col if isinstance(col, tuple) else (col, None)
            part = nm.sheet_keys_lit([pts], [normals], view, light, cell, radius)
            keys[:, c * cell:(c + 1) * cell] = part
            continue
        nf = col["faces"].shape[0]
        for b in range(B):
            first, count, base = (int(v) for v in col["range"][b])
            f0, f1 = max(first, 0), min(first + max(count, 0), nf)
            if f1 <= f0:
                continue
            setup = face_setup(col["verts"], col["faces"][f0:f1], base, None if col["mask"] is None else col["mask"][f0:f1], col["shade"],
                               view, light, cell)
            draw_faces(keys[b * cell:(b + 1) * cell, c * cell:(c + 1) * cell], setup, col["shade"])
    return keys


def render(columns, view, light, cell, radius=1):
    return rm.resolve(sheet_keys(columns, view, light, cell, radius))


def box_pixels(verts, faces, base, view, cell):
    """Pixels of every face's clipped box (0 for a dead or degenerate one): which side of SMALL_BOX a test's face sits on."""
    setup = face_setup(verts, faces, base, None, "depth", view, None, cell)
    return [0 if t is None else t[5][2] * t[5][3] for t in setup]


# ---------------------------------------------------------------------------- meshes of the tests
def icosphere(level=2, radius=1.0):
    """(verts (V,3) fp32 on the sphere, faces (T,3) int64, counter-clockwise seen from outside): 20 * 4^level faces (level 2: 320)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, g = {}, []

        def between(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = between(a, b), between(b, c), between(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.ascontiguousarray(np.asarray(v) * radius, dtype=F), np.asarray(f, dtype=np.int64)


def box_mesh(half=0.55):
    """An axis-aligned cube of 12 faces, counter-clockwise seen from outside."""
    v = np.asarray([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * half
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return np.ascontiguousarray(v, dtype=F), np.asarray(f, dtype=np.int64)
