"""Scenes of the visibility tests (tests/test_visible_host.py, tests/test_gpu_visible.py): small meshes with a known answer, and the
ragged set the kernel is compared with tests/visible_mirror.py on.  A mesh is (verts (V,3) float32, faces (F,3) int32, local)."""
import numpy as np

FACE_STRIDE = 256                                                # faces a workgroup of csrc/visible.hip takes per sweep


def box(lo, hi, n=1, sides=range(6)):
    """An axis-aligned box of 12 n^2 faces (2 n^2 per side, every side with vertices of its own).  sides: 0 1 the faces x = lo, hi;
    2 3: y; 4 5: z."""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), 3), np.broadcast_to(np.asarray(hi, np.float64), 3)
    verts, faces = [], []
    g = np.linspace(0.0, 1.0, n + 1)
    u, v = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    cell = np.asarray([(i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1) for i in range(n) for j in range(n)])
    for side in sides:
        axis, top = side // 2, side % 2
        p = np.empty((u.shape[0], 3))
        p[:, axis] = hi[axis] if top else lo[axis]
        a, b = [k for k in range(3) if k != axis]
        p[:, a], p[:, b] = lo[a] + u * (hi[a] - lo[a]), lo[b] + v * (hi[b] - lo[b])
        at = sum(x.shape[0] for x in verts)
        verts.append(p)
        faces.append(np.concatenate([cell[:, [0, 1, 2]], cell[:, [0, 2, 3]]], 0) + at)
    return np.concatenate(verts, 0).astype(np.float32), np.concatenate(faces, 0).astype(np.int32)


def join(*meshes):
    """One shape of several meshes."""
    verts, faces, at = [], [], 0
    for v, f in meshes:
        verts.append(v)
        faces.append(f + np.int32(at))
        at += v.shape[0]
    return np.concatenate(verts, 0), np.concatenate(faces, 0)


def nested_cubes(n=1):
    """A cube [-1, 1]^3 (the first 12 n^2 faces) around a copy of half the size (the last 12 n^2)."""
    return join(box(-1.0, 1.0, n), box(-0.5, 0.5, n))


def sphere(n):
    """The cube of 12 n^2 faces pushed onto the unit sphere: a convex body."""
    v, f = box(-1.0, 1.0, n)
    v = v.astype(np.float64)
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32), f


def rod(n=64):
    """A rod 0.01 x 0.01 x 1 along z: four long sides of n segments of two faces each, no caps."""
    h, z = 0.005, np.linspace(-0.5, 0.5, n + 1)
    ring = np.asarray([(-h, -h), (h, -h), (h, h), (-h, h)])
    verts = np.asarray([(x, y, zz) for zz in z for x, y in ring], dtype=np.float32)
    faces = []
    for k in range(n):
        for s in range(4):
            a, b, c, d = 4 * k + s, 4 * k + (s + 1) % 4, 4 * (k + 1) + (s + 1) % 4, 4 * (k + 1) + s
            faces += [(a, b, c), (a, c, d)]
    return verts, np.asarray(faces, dtype=np.int32)


def pack_set(meshes):
    """(verts, faces GLOBAL, face_off) of a list of meshes."""
    verts, faces, off, at = [], [], [0], 0
    for v, f in meshes:
        verts.append(np.asarray(v, np.float32))
        faces.append(np.asarray(f, np.int32) + np.int32(at))
        at += v.shape[0]
        off.append(off[-1] + f.shape[0])
    return np.concatenate(verts, 0), np.concatenate(faces, 0), np.asarray(off, dtype=np.int32)


def random_ball(F, rng, scale=1.0):
    """F triangles over shared vertices uniform in the ball of radius `scale`, edge lengths mixed: a third of the faces are slivers
    around one vertex (smaller than a pixel at any resolution used)."""
    V = max(3, F // 2 + 2)
    d = rng.standard_normal((V, 3))
    verts = (scale * d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0, 1, (V, 1)) ** (1.0 / 3.0))
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)])
    extra, tiny = [], []
    for f in range(0, F, 3):                                     # a sliver: two fresh vertices within 1e-3 of the face's first one
        at = V + len(extra)
        extra += [verts[faces[f, 0]] + rng.uniform(-1e-3, 1e-3, 3) * scale, verts[faces[f, 0]] + rng.uniform(-1e-3, 1e-3, 3) * scale]
        tiny.append((f, at))
    verts = np.concatenate([verts, np.asarray(extra).reshape(-1, 3)], 0)
    for f, at in tiny:
        faces[f, 1], faces[f, 2] = at, at + 1
    return verts.astype(np.float32), faces.astype(np.int32)


def ragged_set(seed=0, sizes=(1, 2, 12, 37, 150, 400)):
    """The mirror's set: random shapes of the given face counts (the two-face shape holds a face of zero area in 3D), then the nested
    cubes, then `grid_shape`.  `ragged_frames` gives the frames the tests use with it."""
    rng = np.random.default_rng(seed)
    meshes = []
    for F in sizes:
        v, f = random_ball(F, rng, scale=float(2.0 ** rng.integers(-3, 4)))
        if F == 2:
            f[1, 2] = f[1, 1]
        meshes.append((v, f))
    meshes.append(nested_cubes())
    meshes.append(grid_shape())
    return meshes


def ragged_frames(verts, faces, face_off, twelve=2):
    """shape_frames, except: the radius of shape `twelve` (the twelve-face one) is a quarter of its extent, so that its faces reach far
    outside the image and their vertices clamp (faces larger than the image), and the last shape (the grid) has the frame (0, 0, 0, 8)."""
    from pdgn_amd.meshes import shape_frames
    frame = shape_frames(verts, faces, face_off)
    frame[twelve, 3] /= np.float32(4)
    frame[-1] = (0.0, 0.0, 0.0, GRID_RHO)
    return frame


# what the identity view sees of `grid_shape` at R = 16, by hand: the half at z = 0.5 away from the diagonal, the half at z = 0, not the
# triangle at z = 1 behind the two, the two at z = -1 and z = -2 in front of everything (the second through the fallback), not the
# corner triangle at z = 2 (its one centre lies on its hypotenuse, behind the first half), not the needle
GRID_MASKS = [1, 1, 0, 1, 1, 0, 0]
GRID_RHO = 8.0                                                   # the radius `grid_frames` gives the grid shape: a pixel of R = 16 is one unit


def grid_shape():
    """Triangles in planes of constant z whose corners are whole and half units inside [-8, 8]^2: with the frame (0, 0, 0, 8) and the
    view along z at R = 16 a unit is a pixel, half-integers are pixel centres, +-8 the image border.  The corner (8, 8, 0) / (-8, -8, 0)
    pair keeps the box's centre at the origin."""
    tris = [((-8, -8, 0.5), (8, 8, 0.5), (-8, 8, 0.5)),           # the other half, behind the next one along the shared diagonal
            ((-8, -8, 0), (8, -8, 0), (8, 8, 0)),               # half the image, its hypotenuse through pixel corners, two sides on the border
            ((-7.5, -7.5, 1), (-4.5, -7.5, 1), (-7.5, -4.5, 1)),  # corners on pixel centres
            ((0.5, 0.5, -1), (1.5, 0.5, -1), (0.5, 1.5, -1)),     # one pixel's neighbourhood: covers exactly its three corner centres
            ((2, 2, -2), (2.25, 2, -2), (2, 2.25, -2)),           # smaller than a pixel, no centre inside
            ((-8, 8, 2), (-8, 7, 2), (-7, 8, 2)),                 # in the image's corner
            ((3.5, -2.5, 3), (3.5, -2.5, 3.5), (3.5, -2.5, 4))]   # a needle along z (zero area)
    verts = np.asarray([p for t in tris for p in t], dtype=np.float32)
    return verts, np.arange(verts.shape[0], dtype=np.int32).reshape(-1, 3)
