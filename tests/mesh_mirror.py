"""Host mirror of the mesh feeder (csrc/feed.hip: pdgn_feed_batch_mesh, pdgn_sample_surface; pdgn_amd.data.MeshFeeder): the construction of
include/pdgn_hip.h restated in numpy on pdgn_amd.data._philox4x32_10 -- one Philox call per output column, the face through the shape's
alias table, folded integer barycentric coordinates, the point in individually rounded fp32 operations.  Test infrastructure: the
product never imports it.  The schedule and the noise are tests/feed_mirror.py's."""
import numpy as np

import feed_mirror as fm
from pdgn_amd.data import _philox4x32_10

TAG_MESH, TAG_SURFACE = 8, 12
ONE = 1 << 24


class Arrays:
    """The four arrays of a pdgn_amd.meshes.MeshSet on the host."""

    def __init__(self, meshset):
        self.verts = meshset.verts.cpu().numpy()
        self.faces = meshset.faces.cpu().numpy().astype(np.int64)
        self.face_off = meshset.face_off.cpu().numpy().astype(np.int64)
        self.thr, self.alias = (a.astype(np.uint64) for a in meshset.alias_records())
        self.S = self.face_off.shape[0] - 1


def words(seed, rows, cols, lo, hi24, tag):
    """w0 .. w3, each (len(rows), cols) uint64: the call of counter (j, row, lo, tag | hi24 << 8) for j < cols."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    j = np.broadcast_to(np.arange(cols, dtype=np.uint64).reshape(1, -1), (rows.shape[0], cols))
    full = lambda v: np.full(j.shape, v, dtype=np.uint64)
    return _philox4x32_10(j.copy(), np.broadcast_to(rows, j.shape).copy(), full(lo), full(tag | (hi24 << 8)), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def select_faces(m, shape_ids, w0, w1):
    """Global face index per draw: shape_ids (R) the shape of every row of w0, w1 (R, n)."""
    base = m.face_off[shape_ids].reshape(-1, 1)
    Fc = (m.face_off[shape_ids + 1] - m.face_off[shape_ids]).reshape(-1, 1).astype(np.uint64)
    s = ((w0 * Fc) >> np.uint64(32)).astype(np.int64)
    keep = w1 < m.thr[base + s]
    return base + np.where(keep, s, m.alias[base + s].astype(np.int64))


def barycentric(w2, w3):
    """(a, b) integers in [0, 2^24] with a + b <= 2^24, and (u, v) = (a, b) * 2^-24 as fp32 (exact)."""
    a, b = (w2 >> np.uint64(8)).astype(np.int64), (w3 >> np.uint64(8)).astype(np.int64)
    fold = a + b > ONE
    a, b = np.where(fold, ONE - a, a), np.where(fold, ONE - b, b)
    return a, b, a.astype(np.float32) * np.float32(2.0 ** -24), b.astype(np.float32) * np.float32(2.0 ** -24)


def points(m, gf, u, v):
    """(..., 3) fp32: p = (v0 + u * e1) + v * e2, every operation rounded to fp32 (numpy's fp32 arithmetic is)."""
    tri = m.verts[m.faces[gf]]                                   # (..., 3 corners, 3)
    v0, v1, v2 = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
    e1, e2 = v1 - v0, v2 - v0
    out = (v0 + u[..., None] * e1) + v[..., None] * e2
    assert out.dtype == np.float32
    return out


def draw(m, seed, shape_ids, rows, cols, lo, hi24, tag):
    """-> (points (R, cols, 3) fp32, global faces (R, cols))."""
    w0, w1, w2, w3 = words(seed, rows, cols, lo, hi24, tag)
    gf = select_faces(m, np.asarray(shape_ids, dtype=np.int64), w0, w1)
    _, _, u, v = barycentric(w2, w3)
    return points(m, gf, u, v), gf


def feed_batch_mesh(m, order, first, B, lens, seed, t, row0):
    """pdgn_feed_batch_mesh's ([p1 .. p4] as (B,3,r) fp32, face_rec (B, sum lens) int64); lens = (r1, r2, r3, N)."""
    ids = np.clip(np.asarray(order, dtype=np.int64)[first:first + B], 0, m.S - 1)
    rows = (row0 + np.arange(B)) & 0xFFFFFFFF
    out, rec = [], []
    for k, r in enumerate(lens):
        p, gf = draw(m, seed, ids, rows, r, t & 0xFFFFFFFF, (t >> 32) & 0xFFFFFF, TAG_MESH + k)
        out.append(np.ascontiguousarray(p.transpose(0, 2, 1)))
        rec.append(gf)
    return out, np.concatenate(rec, axis=1)


def sample_surface(m, n, seed, draw_index=0):
    """pdgn_sample_surface's ((S,n,3) fp32, (S,n) faces)."""
    ids = np.arange(m.S)
    return draw(m, seed, ids, ids, n, draw_index & 0xFFFFFFFF, (draw_index >> 32) & 0xFFFFFF, TAG_SURFACE)


class MirrorMeshFeeder:
    """pdgn_amd.data.MeshFeeder on the host."""

    def __init__(self, meshset, batch_size, sizes, seed, rank=0, world=1, sigma=0.2, num_point=2048):
        self.m = meshset if isinstance(meshset, Arrays) else Arrays(meshset)
        self.S, self.B, self.N, self.sizes = self.m.S, batch_size, num_point, tuple(sizes)[:3]
        self.seed, self.rank, self.world, self.sigma = seed, rank, world, sigma
        self.batches_per_epoch = fm.batches_per_epoch(self.S, batch_size, world)

    def schedule(self, epoch, i):
        first = (i * self.world + self.rank) * self.B
        return fm.epoch_order(self.seed, epoch, self.S), first, self.rank * self.B, (epoch - 1) * self.batches_per_epoch + i

    def batch(self, epoch, i, dtype=np.float32, with_faces=False):
        order, first, row0, t = self.schedule(epoch, i)
        reals, rec = feed_batch_mesh(self.m, order, first, self.B, self.sizes + (self.N,), self.seed, t, row0)
        rows = row0 + np.arange(self.B)
        z = [fm.normals_from_words(fm.stream_words(self.seed, t, rows, tag, fm.NOISE_DIM), self.sigma, dtype) for tag in (fm.TAG_Z1, fm.TAG_Z2)]
        return (reals, z[0], z[1], rec) if with_faces else (reals, z[0], z[1])


# ---------------------------------------------------------------------------- meshes the tests are run on
def soup_with_areas(areas, rng):
    """One shape of len(areas) separate right triangles with (about) the given areas, somewhere in [-4, 4]^3; area 0: a face that
    names one vertex twice (its area is exactly zero in any arithmetic)."""
    verts, faces = [], []
    for a in areas:
        o, leg = rng.uniform(-4, 4, 3), np.sqrt(2.0 * a)
        at = len(verts)
        verts += [o, o + (leg, 0, 0), o + (0, leg, 0)] if a > 0 else [o, o + (1, 0, 0), o + (0, 1, 0)]
        faces.append((at, at + 1, at + 2) if a > 0 else (at, at + 1, at + 1))
    return np.asarray(verts, dtype=np.float32), np.asarray(faces, dtype=np.int32)


def random_mesh(F, rng, degenerate=()):
    """A shape of F faces over shared vertices, every |coordinate| log-uniform in [2^-6, 2^6]; the faces listed in `degenerate` name
    one vertex twice."""
    V = max(3, F // 2 + 2)
    verts = (2.0 ** rng.uniform(-6, 6, (V, 3)) * rng.choice([-1.0, 1.0], (V, 3))).astype(np.float32)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int32)
    for f in degenerate:
        faces[f, 2] = faces[f, 1]
    return verts, faces


RAGGED = (1, 4, 12, 37, 1000, 2)


def ragged_meshes(seed=0):
    """The device tests' set: S = 6 shapes of 1, 4, 12, 37, 1000, 2 faces, the second face of the two-face shape degenerate."""
    rng = np.random.default_rng(seed)
    return [random_mesh(F, rng, degenerate=(1,) if F == 2 else ()) for F in RAGGED]
