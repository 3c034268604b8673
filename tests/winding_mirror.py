"""numpy restatement of csrc/winding.hip (include/pdgn_hip.h: pdgn_winding_number): the half solid angle of a face in
the header block's NORMATIVE ORDER -- float32 arrays throughout, one ufunc per rounding -- the routine natan2, the 2^-32 fixed-point terms
and their int64 sums, and what the tests compare them with: the same van Oosterom-Strackee formula in float64 with np.arctan2 and a plain
float64 sum.  The meshes are those of tests/p2m_mirror.py.

Equality with the device is only claimed on normal numbers and zeros: `winding` asserts that no fp32 intermediate of its inputs is
subnormal (check=False lifts it for the accuracy sweeps, which compare with float64 and not with the device)."""
import numpy as np

from p2m_mirror import (F32, NAN_BITS, bits_equal, concatenate, cross, dot3, first_faces, icosphere, points_on_faces,  # noqa: F401
                        random_triangles, slivers, torus_grid)

T_HALF = 13493037705                                               # llrint(pi 2^32): WN_T_HALF
T_BAD = -2 ** 63                                                   # INT64_MIN: WN_T_BAD
K = float.fromhex("0x1.45f306dc9c883p-35")                         # the double nearest 1 / (2^33 pi): WN_K
CHUNK = 256                                                        # WN_CHUNK
TARGET_BLOCKS = 2048                                               # WN_TARGET_BLOCKS
MAX_SPLITS = 4096                                                  # WN_MAX_SPLITS
TINY = F32(2.0 ** -126)

PI, PI_2, PI_4 = (np.uint32(b).view(F32) for b in (0x40490FDB, 0x3FC90FDB, 0x3F490FDB))
TAN_PI_8 = np.uint32(0x3ED413CD).view(F32)                         # 0.41421357
C9, C7, C5, C3 = F32(8.05374449538e-2), F32(-1.38776856032e-1), F32(1.99777106478e-1), F32(-3.33329491539e-1)
BREAKS = (TAN_PI_8, F32(1.0))                                      # the ratios at which natan2 changes its path


class _Check:
    """Collects whether any fp32 intermediate was subnormal."""

    def __init__(self, on):
        self.on = on

    def __call__(self, x):
        if self.on:
            m = np.abs(x)
            assert not ((m > 0) & (m < TINY)).any(), "an fp32 intermediate is subnormal: the mirror and the device are not held to agree"
        return x


def natan2(y, x, chk=None):
    """The normative fp32 arctangent of y / x in [-pi, pi]: 0 wherever y == 0, NaN where either is NaN (and where both are infinite)."""
    chk = chk or _Check(False)
    y, x = np.broadcast_arrays(np.asarray(y, dtype=F32), np.asarray(x, dtype=F32))
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        mx, mn = np.fmax(ax, ay), np.fmin(ax, ay)
        r = chk(mn / mx)
        big = r > TAN_PI_8
        z = np.where(big, chk((r - F32(1)) / (r + F32(1))), r)
        zz = chk(z * z)
        poly = chk(chk(chk(chk(chk(chk(C9 * zz) + C7) * zz) + C5) * zz) + C3)
        a = chk(chk(chk(poly * zz) * z) + z)
        a = np.where(big, PI_4 + a, a)
        a = np.where(ay > ax, PI_2 - a, a)
        a = np.where(x < 0, PI - a, a)
        a = np.where(y < 0, -a, a)
        a = np.where(y == 0, F32(0), a)
        a = np.where(np.isnan(x) | np.isnan(y), np.uint32(NAN_BITS).view(F32), a)
    assert a.dtype == F32
    return a


def half_angles(p, a, b, c, chk=None):
    """NORMATIVE ORDER: p (P,3), faces a, b, c (F,3), all fp32 -> h (P,F) fp32, half the signed solid angle of every face at every point."""
    chk = chk or _Check(False)
    p, a, b, c = (np.ascontiguousarray(x, dtype=F32) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        P = p[:, None, :]
        A, B, C = chk(a[None] - P), chk(b[None] - P), chk(c[None] - P)

        def dot(u, v):
            return chk(chk(chk(u[..., 0] * v[..., 0]) + chk(u[..., 1] * v[..., 1])) + chk(u[..., 2] * v[..., 2]))

        def crs(u, v):
            return np.stack([chk(chk(u[..., 1] * v[..., 2]) - chk(u[..., 2] * v[..., 1])), chk(chk(u[..., 2] * v[..., 0]) - chk(u[..., 0] * v[..., 2])),
                             chk(chk(u[..., 0] * v[..., 1]) - chk(u[..., 1] * v[..., 0]))], axis=-1)

        la, lb, lc = np.sqrt(dot(A, A)), np.sqrt(dot(B, B)), np.sqrt(dot(C, C))
        num = dot(A, crs(B, C))
        den = chk(chk(chk(chk(la * lb) * lc) + chk(dot(A, B) * lc)) + chk(chk(dot(B, C) * la) + chk(dot(C, A) * lb)))
        h = natan2(num, den, chk)
    assert h.dtype == F32
    return h


def face_terms(p, a, b, c, check=False):
    """-> (t (P,F) int64 = llrint((double) h 2^32), 0 where h is not finite; bad (P,F): h is not finite)."""
    h = half_angles(p, a, b, c, _Check(check))
    bad = ~np.isfinite(h)
    t = np.rint(np.where(bad, 0.0, h.astype(np.float64)) * 4294967296.0).astype(np.int64)
    return t, bad


def sum_terms(p, tri, step=2048, check=False):
    """One cloud against the faces tri (F,3,3): (T (P) int64, bad (P)); the plain sum, no sentinel yet."""
    p = np.ascontiguousarray(p, dtype=F32).reshape(-1, 3)
    tri = np.asarray(tri, dtype=F32).reshape(-1, 3, 3)
    T, bad = np.zeros(p.shape[0], dtype=np.int64), ~np.isfinite(p).all(axis=1)
    for f0 in range(0, tri.shape[0], step):
        t = tri[f0:f0 + step]
        terms, b = face_terms(p[~bad], t[:, 0], t[:, 1], t[:, 2], check)
        T[~bad] += terms.sum(axis=1)
        bad[~bad] |= b.any(axis=1)
    return T, bad


def finish(T, bad):
    """(T with the sentinel, w fp32, inside int32) from the sums and the flags."""
    T = np.where(bad, np.int64(T_BAD), T)
    w = np.where(bad, np.uint32(NAN_BITS).view(F32), (np.where(bad, 0, T).astype(np.float64) * K).astype(F32))
    return T, w.astype(F32), (T >= T_HALF).astype(np.int32)


def winding(xyz, verts, faces, face_off, shape=None, live=None, check=True):
    """pdgn_winding_number: xyz (B,N,3) against the live faces of shape[c] -> T (B,N) int64, w (B,N) fp32, inside (B,N) int32."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    verts, faces = np.asarray(verts, dtype=F32), np.asarray(faces, dtype=np.int64)
    B, N = xyz.shape[:2]
    shape = np.arange(B) if shape is None else np.asarray(shape)
    live = np.ones(faces.shape[0], dtype=bool) if live is None else np.asarray(live) != 0
    T, w, inside = np.empty((B, N), np.int64), np.empty((B, N), F32), np.empty((B, N), np.int32)
    for c in range(B):
        s = int(shape[c])
        index = np.arange(face_off[s], face_off[s + 1]) if 0 <= s < len(face_off) - 1 else np.zeros(0, dtype=np.int64)
        index = index[live[index]]
        T[c], w[c], inside[c] = finish(*sum_terms(xyz[c], verts[faces[index]], check=check))
    return T, w, inside


def splits_for(b, n, faces):
    """pdgn_winding_splits: the parts the library takes for splits = 0."""
    blocks, chunks = b * -(-n // CHUNK), -(-faces // CHUNK)
    return int(max(1, min(-(-TARGET_BLOCKS // blocks), chunks // 2, MAX_SPLITS)))


# ---------------------------------------------------------------------------- the oracle (float64, np.arctan2, a plain sum)
def winding_f64(p, tri, step=2048):
    """(P) float64: the generalized winding number of the faces tri (F,3,3) at the points p."""
    p, tri = np.asarray(p, dtype=np.float64).reshape(-1, 3), np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    out = np.zeros(p.shape[0])
    for f0 in range(0, tri.shape[0], step):
        t = tri[f0:f0 + step]
        A, B, C = t[None, :, 0] - p[:, None], t[None, :, 1] - p[:, None], t[None, :, 2] - p[:, None]
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (A, B, C))
        num = (A * np.cross(B, C)).sum(axis=-1)
        den = la * lb * lc + (A * B).sum(-1) * lc + (B * C).sum(-1) * la + (C * A).sum(-1) * lb
        out += np.where(num == 0, 0.0, np.arctan2(num, den)).sum(axis=1)
    return out / (2.0 * np.pi)


# ---------------------------------------------------------------------------- meshes and grids of the occupancy tests
def box_mesh(lo, hi):
    """The axis-aligned box [lo, hi]^3 as 12 triangles, outward winding: (verts (8,3) fp32, faces (12,3) int32)."""
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), 3), np.broadcast_to(np.asarray(hi, dtype=np.float64), 3)
    v = np.asarray([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)])
    q = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return v.astype(F32), np.asarray(f, dtype=np.int32)


def cell_centres(origin, voxel, R):
    """(R^3,3) fp32: origin + (i + 0.5) voxel per axis, index order (x, y, z) with z fastest, in the order the host interface spells:
    the fp32 product and sum."""
    origin, voxel = np.asarray(origin, dtype=F32), F32(voxel)
    axes = [origin[k] + (np.arange(R, dtype=F32) + F32(0.5)) * voxel for k in range(3)]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)
    return np.ascontiguousarray(g.reshape(-1, 3), dtype=F32)
