"""numpy restatement of csrc/reconstruct.hip (include/pdgn_hip.h: pdgn_imls_grid, pdgn_surface_nets_count / _emit):
the implicit-moving-least-squares field on a regular grid and the surface-nets mesh of it, every fp32 operation rounded on its own and
every decision a comparison, so that the kernels and this file agree bit for bit.  Used by tests/test_reconstruct_host.py and
tests/test_gpu_reconstruct.py; imports nothing of pdgn_amd.

NORMATIVE ORDER, THE FIELD (one cloud: x (n,3), g (n,3), origin o (3), voxel v, inv = 1 / h^2, R nodes per axis; dot3 as in
tests/normals_mirror.py: (a.x b.x + a.y b.y) + a.z b.z):
    node (i,j,k), id (i R + j) R + k, at p_a = o_a + (float)i_a * v
    point j is live iff its six values are finite; a dead point is skipped
    sw = sf = +0;  for j ascending over the live points:
        d = p - x_j;  d2 = dot3(d, d);  t = 1 - d2 * inv;  where t > 0:  w = t * t,  sw = sw + w,  sf = sf + w * dot3(d, g_j)
    f = sw > 0 ? sf / sw : NaN (0x7FC00000): an invalid node, no point within h
Adding a term with w = 0 changes no bit, so points may be culled for a brick of nodes where the test of `brick_skips` proves t <= 0.

THE MESH (C = R - 1 cells per axis, cell id (i C + j) C + k, corner (a,b,c) of a cell is node (i+a, j+b, k+c); inside iff f < 0):
    active cell   all eight corners valid, 1 to 7 of them inside
    its vertex    edges in the order axis A = 0, 1, 2, offsets (u,v) = (0,0), (1,0), (0,1), (1,1) on axes (A+1)%3, (A+2)%3; on an edge whose
                  ends differ in "inside": t = f0 / (f0 - f1), the crossing is the low corner's offset with t on axis A; the three local
                  coordinates are summed in edge order from +0, m crossings;  pos_a = o_a + v * ((float)cell_a + sum_a / (float)m)
    quads         node N, axis A with N + e_A in range, both ends valid and differing in "inside"; the cells N + u e_A1 + w e_A2 for (u,w)
                  = (-1,-1), (0,-1), (0,0), (-1,0); all four in range and active: q in that order if N is inside, reversed if not, the
                  triangles (q0,q1,q2), (q0,q2,q3); otherwise the edge is open
    order         vertices by ascending cell id, faces by ascending 3 (node id) + A, indices local to the cloud
    counters      vertices, faces, open edges, invalid nodes"""
import numpy as np

from normals_mirror import dot3

F = np.float32
BRICK = 4
NAN_BITS = 0x7FC00000
MIN_R, MAX_R = 2, 256
CELLS = ((-1, -1), (0, -1), (0, 0), (-1, 0))
EXPORT_SEEDS = (0, 1, 5)                                            # tori the export test meshes on the device (of 0 .. 7, which all hold)


def bits_equal(got, want):
    """Equal in every bit, NaN payloads included."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def axis_positions(origin, voxel, R):
    """(R,3): p[i, a] = o_a + (float)i * v, one multiplication and one addition."""
    i = np.arange(R, dtype=F)
    return (np.asarray(origin, dtype=F)[None, :] + (i * F(voxel)).astype(F)[:, None]).astype(F)


def node_positions(origin, voxel, R):
    """(R^3,3) in node-id order."""
    p = axis_positions(origin, voxel, R)
    ii, jj, kk = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    return np.stack([p[ii.ravel(), 0], p[jj.ravel(), 1], p[kk.ravel(), 2]], axis=1)


def live_points(x, g):
    return np.isfinite(x).all(axis=1) & np.isfinite(g).all(axis=1)


def brick_skips(x, origin, voxel, inv, R):
    """(n, nb, nb, nb) bool, nb = ceil(R / BRICK): True where point j provably has t <= 0 at every node of the brick.  The brick's nodes
    lie in the box [lo, hi] of its first and last node's positions (p is monotone in the index); per axis m = max(lo - x, x - hi, 0) is
    at most |p - x| rounded, for every node of the brick, because a correctly rounded subtraction is monotone; products and sums of
    non-negative numbers are monotone too, so the t of (m.x, m.y, m.z) bounds every node's t from above: no slack is needed."""
    p = axis_positions(origin, voxel, R)
    nb = (R + BRICK - 1) // BRICK
    first = np.arange(nb) * BRICK
    last = np.minimum(first + BRICK - 1, R - 1)
    with np.errstate(all="ignore"):
        m = []
        for a in range(3):
            lo, hi = p[first, a][None, :], p[last, a][None, :]
            xa = x[:, a][:, None]
            m.append(np.maximum(np.maximum(lo - xa, xa - hi), F(0.0)).astype(F))           # (n, nb)
        mx, my, mz = m[0][:, :, None, None], m[1][:, None, :, None], m[2][:, None, None, :]
        d2 = ((mx * mx + my * my) + mz * mz).astype(F)
        t = (F(1.0) - d2 * F(inv)).astype(F)
        return ~(t > 0)


def field_cloud(x, g, origin, voxel, inv, R, cull=False, skip=None):
    """One cloud -> f (R^3,) fp32.  cull=False visits every live point at every node (the normative statement); cull=True leaves out, per
    brick, the points `brick_skips` names (what the kernel does); skip: an explicit (n, nb, nb, nb) mask in place of brick_skips'."""
    x = np.ascontiguousarray(x, dtype=F)
    g = np.ascontiguousarray(g, dtype=F)
    n = x.shape[0]
    assert x.shape == (n, 3) and g.shape == (n, 3) and n >= 1 and MIN_R <= R <= MAX_R
    origin, voxel, inv = np.asarray(origin, dtype=F).reshape(3), F(voxel), F(inv)
    assert voxel > 0 and inv > 0 and np.isfinite(voxel) and np.isfinite(inv)
    sw, sf = np.zeros(R ** 3, dtype=F), np.zeros(R ** 3, dtype=F)
    live = live_points(x, g)
    culled = cull or skip is not None
    with np.errstate(all="ignore"):
        if not culled:
            # every node at once, per axis first: d_a depends on the node's index along a alone (the same values in the same order)
            pa = axis_positions(origin, voxel, R)
            sw3, sf3 = sw.reshape(R, R, R), sf.reshape(R, R, R)
            for j in np.nonzero(live)[0]:
                d = (pa - x[j][None, :]).astype(F)                  # (R,3)
                sq, dg = (d * d).astype(F), (d * g[j][None, :]).astype(F)
                d2 = ((sq[:, None, 0] + sq[None, :, 1]).astype(F)[:, :, None] + sq[None, None, :, 2]).astype(F)
                t = (F(1.0) - (d2 * inv).astype(F)).astype(F)
                on = t > 0
                w = (t * t).astype(F)
                dn = ((dg[:, None, 0] + dg[None, :, 1]).astype(F)[:, :, None] + dg[None, None, :, 2]).astype(F)
                np.add(sw3, w, out=sw3, where=on)
                np.add(sf3, (w * dn).astype(F), out=sf3, where=on)
        else:
            # per point, the nodes of the bricks that keep it
            if skip is None:
                skip = brick_skips(np.where(live[:, None], x, F(0.0)), origin, voxel, inv, R)
            P = node_positions(origin, voxel, R)
            nb = skip.shape[1]
            ids = np.arange(R ** 3).reshape(R, R, R)
            nodes_of = {}
            for j in np.nonzero(live)[0]:
                kept = np.nonzero(~skip[j].reshape(-1))[0]
                if kept.size == 0:
                    continue
                for br in kept.tolist():
                    if br not in nodes_of:
                        bi, bj, bk = br // (nb * nb), (br // nb) % nb, br % nb
                        nodes_of[br] = ids[bi * BRICK:(bi + 1) * BRICK, bj * BRICK:(bj + 1) * BRICK, bk * BRICK:(bk + 1) * BRICK].reshape(-1)
                sel = np.concatenate([nodes_of[br] for br in kept.tolist()])
                d = (P[sel] - x[j][None, :]).astype(F)
                d2 = dot3(d, d).astype(F)
                t = (F(1.0) - (d2 * inv).astype(F)).astype(F)
                on = t > 0
                w = (t * t).astype(F)
                term = (w * dot3(d, np.broadcast_to(g[j], d.shape)).astype(F)).astype(F)
                sw[sel] = np.where(on, (sw[sel] + w).astype(F), sw[sel])
                sf[sel] = np.where(on, (sf[sel] + term).astype(F), sf[sel])
        f = np.where(sw > 0, (sf / np.where(sw > 0, sw, F(1.0))).astype(F), F(0.0)).astype(F)
    fb = f.view(np.uint32).copy()
    fb[~(sw > 0)] = NAN_BITS
    return fb.view(F)


def field(x, g, origin, voxel, inv, R, cull=False):
    """x (b,n,3), g (b,n,3), origin (b,3), voxel (b), inv (b) -> (b, R, R, R)."""
    return np.stack([field_cloud(xc, gc, o, v, s, R, cull=cull).reshape(R, R, R)
                     for xc, gc, o, v, s in zip(np.asarray(x, dtype=F), np.asarray(g, dtype=F), origin, voxel, inv)])


# ---------------------------------------------------------------------------- the mesh
def _corner(a, R, off):
    C = R - 1
    return a[off[0]:off[0] + C, off[1]:off[1] + C, off[2]:off[2] + C]


def active_cells(f):
    """f (R,R,R) -> (C,C,C) bool."""
    R = f.shape[0]
    valid, inside = ~np.isnan(f), f < 0
    allvalid = np.ones((R - 1,) * 3, dtype=bool)
    nin = np.zeros((R - 1,) * 3, dtype=np.int32)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                allvalid &= _corner(valid, R, (a, b, c))
                nin += _corner(inside, R, (a, b, c))
    return allvalid & (nin >= 1) & (nin <= 7)


def surface_nets_cloud(f, origin, voxel):
    """One cloud: f (R,R,R) -> (verts (V,3) fp32, faces (F,3) int32, (vertices, faces, open edges, invalid nodes))."""
    f = np.ascontiguousarray(f, dtype=F)
    R = f.shape[0]
    assert f.shape == (R, R, R) and MIN_R <= R <= MAX_R
    C = R - 1
    origin, voxel = np.asarray(origin, dtype=F).reshape(3), F(voxel)
    valid = ~np.isnan(f)
    with np.errstate(invalid="ignore"):
        inside = f < 0
    active = active_cells(f)
    # ---- vertices
    ssum = [np.zeros((C, C, C), dtype=F) for _ in range(3)]
    m = np.zeros((C, C, C), dtype=np.int32)
    with np.errstate(all="ignore"):
        for A in range(3):
            A1, A2 = (A + 1) % 3, (A + 2) % 3
            for v in (0, 1):
                for u in (0, 1):
                    lo = [0, 0, 0]
                    lo[A1], lo[A2] = u, v
                    hi = list(lo)
                    hi[A] = 1
                    f0, f1 = _corner(f, R, lo), _corner(f, R, hi)
                    cross = active & (_corner(inside, R, lo) != _corner(inside, R, hi))
                    t = (f0 / (f0 - f1).astype(F)).astype(F)
                    local = [None, None, None]
                    local[A], local[A1], local[A2] = t, np.full((C, C, C), u, dtype=F), np.full((C, C, C), v, dtype=F)
                    for a in range(3):
                        ssum[a] = np.where(cross, (ssum[a] + local[a]).astype(F), ssum[a])
                    m += cross
        cells = np.nonzero(active.reshape(-1))[0]
        ci = np.stack(np.unravel_index(cells, (C, C, C)), axis=1)
        mf = m.reshape(-1)[cells].astype(F)
        verts = np.empty((cells.size, 3), dtype=F)
        for a in range(3):
            q = (ssum[a].reshape(-1)[cells] / mf).astype(F)
            verts[:, a] = (origin[a] + (voxel * (ci[:, a].astype(F) + q).astype(F)).astype(F)).astype(F)
    rank = np.full(C ** 3, -1, dtype=np.int64)
    rank[cells] = np.arange(cells.size)
    rank = rank.reshape(C, C, C)
    # ---- quads
    keys, quads, opened = [], [], 0
    for A in range(3):
        A1, A2 = (A + 1) % 3, (A + 2) % 3
        e = [0, 0, 0]
        e[A] = 1
        sl0 = tuple(slice(0, R - e[a]) for a in range(3))
        sl1 = tuple(slice(e[a], R) for a in range(3))
        cross = valid[sl0] & valid[sl1] & (inside[sl0] != inside[sl1])
        N = np.stack(np.nonzero(cross), axis=1)                     # (E,3), ascending node id
        if N.shape[0] == 0:
            continue
        ok = np.ones(N.shape[0], dtype=bool)
        q = np.zeros((N.shape[0], 4), dtype=np.int64)
        for s, (u, w) in enumerate(CELLS):
            c = N.copy()
            c[:, A1] += u
            c[:, A2] += w
            inr = ((c >= 0) & (c < C)).all(axis=1)
            cs = np.where(inr[:, None], c, 0)
            r = rank[cs[:, 0], cs[:, 1], cs[:, 2]]
            ok &= inr & (r >= 0)
            q[:, s] = r
        opened += int((~ok).sum())
        N, q = N[ok], q[ok]
        rev = ~inside[N[:, 0], N[:, 1], N[:, 2]]
        q[rev] = q[rev][:, ::-1]
        keys.append(3 * ((N[:, 0] * R + N[:, 1]) * R + N[:, 2]) + A)
        quads.append(q)
    if keys:
        keys, quads = np.concatenate(keys), np.concatenate(quads)
        quads = quads[np.argsort(keys, kind="stable")]
        faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
    else:
        faces = np.zeros((0, 3), dtype=np.int32)
    return verts, faces, (int(cells.size), int(faces.shape[0]), opened, int((~valid).sum()))


def surface_nets(f, origin, voxel):
    """f (b,R,R,R) -> (verts (V,3), faces (F,3) int32 local to their cloud, vert_off (b+1) int32, face_off (b+1) int32, stats (b,4) int32)."""
    out = [surface_nets_cloud(fc, o, v) for fc, o, v in zip(f, origin, voxel)]
    stats = np.array([r[2] for r in out], dtype=np.int32).reshape(-1, 4)
    off = lambda col: np.concatenate([[0], np.cumsum(stats[:, col])]).astype(np.int32)
    return (np.concatenate([r[0] for r in out]).reshape(-1, 3), np.concatenate([r[1] for r in out]).reshape(-1, 3), off(0), off(1), stats)


# ---------------------------------------------------------------------------- the grid and the whole chain
def nn_mean(x):
    """Mean distance to the nearest other point, fp64."""
    x64 = np.asarray(x, dtype=np.float64)
    d2 = ((x64[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    return float(np.sqrt(d2.min(axis=1)).mean())


def grid_for(x, resolution, radius):
    """The cube around the bounding box's centre with half-side (largest half-extent + h): (origin (3), voxel, inv) as fp32 values."""
    x64 = np.asarray(x, dtype=np.float64)
    x64 = x64[np.isfinite(x64).all(axis=1)]
    lo, hi = x64.min(axis=0), x64.max(axis=0)
    half = float(((hi - lo) / 2).max()) + float(radius)
    return ((lo + hi) / 2 - half).astype(F), F(2.0 * half / (resolution - 1)), F(1.0 / (float(radius) * float(radius)))


def reconstruct_cloud(x, g, resolution, radius=None, radius_factor=5.0):
    """-> (verts, faces, stats, (origin, voxel, inv), field)."""
    h = radius_factor * nn_mean(np.asarray(x)[live_points(np.asarray(x, dtype=F), np.asarray(g, dtype=F))]) if radius is None else float(radius)
    origin, voxel, inv = grid_for(x, resolution, h)
    f = field_cloud(x, g, origin, voxel, inv, resolution, cull=True).reshape((resolution,) * 3)
    verts, faces, stats = surface_nets_cloud(f, origin, voxel)
    return verts, faces, stats, (origin, voxel, inv), f


# ---------------------------------------------------------------------------- inputs the tests share
def fibonacci_sphere(n, radius=1.0):
    """n points on the sphere by the golden-angle spiral -> (points (n,3) fp32, outward unit normals (n,3) fp32)."""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    u = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    return (radius * u).astype(F), u.astype(F)
