"""numpy restatement of csrc/meshdist.hip (include/pdgn_hip.h: pdgn_mesh_dist_prepare, pdgn_point_mesh_distance): the
per-face value in the header block's NORMATIVE ORDER -- float32 arrays throughout, one ufunc per rounding, np.fmax / np.fmin for the clamps --
the lexicographic minimum over the live faces, the culling bound, and what the tests compare them with: an independent closest-point routine
in float64 (the barycentric region walk of Ericson 5.1.5), and the meshes the cases are built from."""
import numpy as np

F32 = np.float32
NAN_BITS = 0x7FC00000
GROUP, CHUNK = 64, 256                                             # MD_GROUP, MD_CHUNK


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _nan(shape):
    return np.full(shape, NAN_BITS, dtype=np.uint32).view(F32)


def dot3(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z over the last axis, every operation rounded to fp32."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def clamp(x, lo, hi):
    return np.fmin(np.fmax(x, lo), hi)


def face_box(a, b, c):
    return np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)


def face_values(p, a, b, c, dtype=F32):
    """NORMATIVE ORDER: p (P,3), faces a, b, c (F,3), all fp32 -> d2 (P,F), q (P,F,3).  dtype=np.float64: the same expressions in
    float64 (the smooth function the gradient test differentiates), bit for bit nothing."""
    p, a, b, c = (np.ascontiguousarray(x, dtype=dtype) for x in (p, a, b, c))
    zero, one = dtype(0), dtype(1)
    with np.errstate(all="ignore"):
        lo, hi = face_box(a, b, c)
        P = p[:, None, :]
        us = [b - a, c - b, a - c]
        ws = [P - a[None], P - b[None], P - c[None]]
        best, best_q = None, None
        for k, s in enumerate((a, b, c)):
            u, w = us[k][None], ws[k]
            t = clamp(dot3(w, u) / dot3(u, u), zero, one)
            q = clamp(s[None] + u * t[..., None], lo[None], hi[None])
            d = P - q
            d2 = dot3(d, d)
            if k == 0:
                best, best_q = d2, q
            else:
                take = d2 < best
                best, best_q = np.where(take, d2, best), np.where(take[..., None], q, best_q)
        n = cross(us[0], c - a)
        nn = dot3(n, n)
        N = n[None]
        counts = (nn > zero)[None] & (dot3(N, cross(us[0][None], ws[0])) >= zero) & (dot3(N, cross(us[1][None], ws[1])) >= zero) \
            & (dot3(N, cross(us[2][None], ws[2])) >= zero)
        h = dot3(N, P - best_q) / nn[None]
        q = clamp(P - N * h[..., None], lo[None], hi[None])
        d = P - q
        d2 = dot3(d, d)
        take = counts & (d2 < best)
        best, best_q = np.where(take, d2, best), np.where(take[..., None], q, best_q)
    assert best.dtype == dtype and best_q.dtype == dtype
    return best, best_q


def keys(d2, index):
    """bits(d2) << 32 | f as uint64; 2^64 - 1 where d2 is NaN (never wins)."""
    k = (np.ascontiguousarray(d2, dtype=F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(index, dtype=np.uint64)
    return np.where(np.isnan(d2), np.uint64(0xFFFFFFFFFFFFFFFF), k)


def closest_of(p, tri, index, step=2048):
    """One cloud against the faces tri (F,3,3) with the indices `index` (F): (d2 (P), face (P) int32, closest (P,3)), the lexicographic
    minimum of (d2_f, f); NaN / -1 / NaN for a point that is not finite and where nothing wins."""
    p = np.ascontiguousarray(p, dtype=F32).reshape(-1, 3)
    tri, index = np.asarray(tri, dtype=F32).reshape(-1, 3, 3), np.asarray(index, dtype=np.int64).reshape(-1)
    P = p.shape[0]
    top = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = np.full(P, top, dtype=np.uint64)
    best_q = _nan((P, 3))
    rows = np.arange(P)
    for f0 in range(0, tri.shape[0], step):
        t = tri[f0:f0 + step]
        d2, q = face_values(p, t[:, 0], t[:, 1], t[:, 2])
        k = keys(d2, index[f0:f0 + step][None, :])
        j = np.argmin(k, axis=1)
        take = k[rows, j] < best
        best = np.where(take, k[rows, j], best)
        best_q = np.where(take[:, None], q[rows, j], best_q)
    live = np.isfinite(p).all(axis=1) & (best != top)
    d2 = np.where(live, (best >> np.uint64(32)).astype(np.uint32).view(F32), _nan(P))
    face = np.where(live, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return d2, face, np.where(live[:, None], best_q, _nan((P, 3)))


def runner_up(p, tri):
    """(P) fp32: the second smallest d2_f of every point over the faces tri (inf with fewer than two): with the smallest, the gap that
    tells how far a point is from the medial axis."""
    tri = np.asarray(tri, dtype=F32).reshape(-1, 3, 3)
    d2, _ = face_values(p, tri[:, 0], tri[:, 1], tri[:, 2])
    d2 = np.where(np.isnan(d2), F32(np.inf), d2)
    return np.sort(d2, axis=1)[:, 1] if tri.shape[0] > 1 else np.full(d2.shape[0], np.inf, dtype=F32)


def point_to_mesh(xyz, verts, faces, face_off, shape=None, live=None):
    """pdgn_point_mesh_distance: xyz (B,N,3) against the live faces of shape[c] -> d2 (B,N), face (B,N) int32 global, closest (B,N,3)."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    verts, faces = np.asarray(verts, dtype=F32), np.asarray(faces, dtype=np.int64)
    B, N = xyz.shape[:2]
    shape = np.arange(B) if shape is None else np.asarray(shape)
    live = np.ones(faces.shape[0], dtype=bool) if live is None else np.asarray(live) != 0
    d2, face, q = _nan((B, N)), np.full((B, N), -1, dtype=np.int32), _nan((B, N, 3))
    for c in range(B):
        s = int(shape[c])
        if not 0 <= s < len(face_off) - 1:
            continue
        index = np.arange(face_off[s], face_off[s + 1])
        index = index[live[index]]
        if index.size:
            d2[c], face[c], q[c] = closest_of(xyz[c], verts[faces[index]], index)
    return d2, face, q


def lower_bound(flo, fhi, plo, phi):
    """CULLING: dot3(m, m), m_a = max(max(flo_a - phi_a, plo_a - fhi_a), 0), in fp32."""
    flo, fhi, plo, phi = (np.asarray(x, dtype=F32) for x in (flo, fhi, plo, phi))
    with np.errstate(all="ignore"):
        m = np.fmax(np.fmax(flo - phi, plo - fhi), F32(0))
        return dot3(m, m)


# ---------------------------------------------------------------------------- the independent oracle (float64, another algorithm)
def _d64(a, b):
    return (a * b).sum(axis=-1)


def closest_f64(p, a, b, c):
    """The closest point of triangle (a, b, c) to p by the barycentric region walk (Ericson, Real-Time Collision Detection, 5.1.5), in
    float64; the arguments broadcast over leading axes.  -> (distance, closest point)."""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (p, a, b, c)))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _d64(ab, ap), _d64(ac, ap)
    bp = p - b
    d3, d4 = _d64(ab, bp), _d64(ac, bp)
    cp = p - c
    d5, d6 = _d64(ab, cp), _d64(ac, cp)
    # the sub-areas as triple products n . (x p x y p): Lagrange's identity turns them into the book's d1 d4 - d3 d2 and so on, but those
    # are differences of products of order one for a value of the order of the face's area squared -- on a sliver of width 1e-6 they
    # lose every digit even in float64 (the walk then ends in the wrong region: 1.8e-5 for a point 1.4e-7 from its face)
    n = np.cross(ab, ac)
    vc, vb, va = _d64(n, np.cross(ap, bp)), _d64(n, np.cross(cp, ap)), _d64(n, np.cross(bp, cp))
    with np.errstate(all="ignore"):
        denom = 1.0 / (va + vb + vc)
        q = a + ab * (vb * denom)[..., None] + ac * (vc * denom)[..., None]
        done = np.zeros(q.shape[:-1], dtype=bool)

        def region(where, value):
            nonlocal q, done
            where = where & ~done
            q = np.where(where[..., None], value, q)
            done = done | where

        region((d1 <= 0) & (d2 <= 0), a)
        region((d3 >= 0) & (d4 <= d3), b)
        region((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * (d1 / (d1 - d3))[..., None])
        region((d6 >= 0) & (d5 <= d6), c)
        region((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * (d2 / (d2 - d6))[..., None])
        region((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None])
    return np.sqrt(_d64(p - q, p - q)), q


def distance_f64(p, tri, step=1024):
    """(P) float64: the least oracle distance of every point over the faces tri (F,3,3)."""
    p, tri = np.asarray(p, dtype=np.float64).reshape(-1, 3), np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    out = np.full(p.shape[0], np.inf)
    for f0 in range(0, tri.shape[0], step):
        t = tri[f0:f0 + step]
        d, _ = closest_f64(p[:, None, :], t[None, :, 0], t[None, :, 1], t[None, :, 2])
        out = np.minimum(out, d.min(axis=1))
    return out


# ---------------------------------------------------------------------------- meshes the tests are run on
def icosphere(level, radius=1.0):
    """(verts (V,3) fp32 on the sphere, faces (20 * 4^level, 3) int32), outward winding."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1),
         (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius).astype(F32), np.asarray(f, dtype=np.int32)


def icosphere_sag(level):
    """The largest distance from the unit sphere to the icosphere of that level inscribed in it: 1 - the least distance of a face's plane
    from the centre, in float64 (the sag of the flattest face's circumscribed cap)."""
    v, f = icosphere(level)
    t = v.astype(np.float64)[f]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return float(1.0 - ((n * t[:, 0]).sum(axis=1) / np.linalg.norm(n, axis=1)).min())


def torus_grid(nu, nv, R=1.0, r=0.4):
    """The torus of radii R and r as a grid of nu x nv quads, two triangles each: (verts (nu nv,3) fp32, faces (2 nu nv,3) int32)."""
    u, w = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    verts = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    at = lambda a, b: ((a % nu) * nv + (b % nv)).reshape(-1)
    q0, q1, q2, q3 = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
    faces = np.stack([np.stack([q0, q1, q2], 1), np.stack([q0, q2, q3], 1)], axis=1).reshape(-1, 3)
    return verts.astype(F32), faces.astype(np.int32)


def random_triangles(count, rng, scale=1.0, spread=1.0):
    """`count` separate triangles: corners within `scale` of a centre drawn in [-spread, spread]^3."""
    tri = rng.uniform(-spread, spread, (count, 1, 3)) + rng.uniform(-scale, scale, (count, 3, 3))
    return tri.reshape(-1, 3).astype(F32), np.arange(3 * count, dtype=np.int32).reshape(-1, 3)


def slivers(count, rng, width, spread=1.0):
    """`count` separate slivers: a unit-length edge in a random direction and a third corner `width` away from a random point of it."""
    s = rng.uniform(-spread, spread, (count, 3))
    e = rng.standard_normal((count, 3))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    side = np.cross(e, rng.standard_normal((count, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    third = s + e * rng.uniform(0.05, 0.95, (count, 1)) + side * width
    tri = np.stack([s, s + e, third], axis=1)
    return tri.reshape(-1, 3).astype(F32), np.arange(3 * count, dtype=np.int32).reshape(-1, 3)


def first_faces(mesh, count):
    """The first `count` faces of a mesh with the vertices they use, renumbered."""
    v, f = mesh
    assert count <= f.shape[0]
    f = f[:count]
    used, inverse = np.unique(f.reshape(-1), return_inverse=True)
    return v[used], inverse.reshape(-1, 3).astype(np.int32)


def points_on_faces(verts, faces, count, rng):
    """`count` points on random faces, barycentric in float64 and rounded to fp32 -> (points (count,3), the faces drawn (count))."""
    f = rng.integers(0, faces.shape[0], count)
    w = rng.dirichlet((1.0, 1.0, 1.0), count)
    t = verts.astype(np.float64)[faces[f]]
    return (t * w[..., None]).sum(axis=1).astype(F32), f


def concatenate(meshes):
    """A list of (verts, faces) -> verts, global faces, face_off."""
    verts, faces, off, at = [], [], [0], 0
    for v, f in meshes:
        verts.append(v), faces.append(f.astype(np.int64) + at)
        at += v.shape[0]
        off.append(off[-1] + f.shape[0])
    return np.concatenate(verts).astype(F32), np.concatenate(faces).astype(np.int32), np.asarray(off, dtype=np.int32)
