"""pdgn_mesh_face_votes (csrc/visible.hip, the second header block) in numpy: tests/visible_mirror.py's snap, dead faces and depth
buffer, then per (face, view) the count of the covered centres that pass the depth test, added to the front or the back column by the
sign of S = edge(P0, P1, P2) on the snapped integers in the STORED vertex order.  The convention: S < 0, the view sees the FRONT -- the
side from which the stored vertices run counter-clockwise, the side the normal e1 x e2 points to (an outward-oriented closed mesh shows
only fronts); S > 0, the BACK; S = 0, edge-on, no vote.  int64 after the snap."""
import numpy as np

from visible_mirror import BIAS_COVER, bias_small, dead_faces, depth_buffer, snap


def _side(P):
    """S of a snapped face P (3,3) int64 in its stored order."""
    (x0, y0), (x1, y1), (x2, y2) = ((int(r[0]), int(r[1])) for r in P)
    return (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)


def votes(verts, faces, face_off, frame, views, R):
    """(front (F) uint32, back (F) uint32, mask (F) uint32): verts (V,3), faces (F,3) GLOBAL, face_off (S+1), frame (S,4), views (NV,3,3)."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int64)
    views = np.asarray(views, np.float32).reshape(-1, 3, 3)
    count = np.zeros((faces.shape[0], 2), dtype=np.int64)
    mask = np.zeros(faces.shape[0], dtype=np.uint32)
    dead = dead_faces(verts, faces)
    small = bias_small(R)
    for c in range(len(face_off) - 1):
        a, b = int(face_off[c]), int(face_off[c + 1])
        used, local = np.unique(faces[a:b], return_inverse=True)
        local = local.reshape(-1, 3)
        for v in range(views.shape[0]):
            snapped = snap(verts[used], frame[c], views[v], R)
            buf, cov = depth_buffer(snapped, local, dead[a:b], R)
            for f in range(a, b):
                if dead[f]:
                    continue
                P = snapped[local[f - a]]
                S, cf = _side(P), cov[f - a]
                if cf is not None:
                    n = int(np.count_nonzero(cf[2] <= buf[cf[0], cf[1]] + BIAS_COVER))
                    seen = n > 0
                else:
                    px, py = min(int(P[:, 0].sum()) // 3 >> 8, R - 1), min(int(P[:, 1].sum()) // 3 >> 8, R - 1)
                    seen = int(P[:, 2].sum()) // 3 <= int(buf[py, px]) + small
                    n = 1 if seen and S != 0 else 0
                count[f, 1 if S > 0 else 0] += n
                if seen:
                    mask[f] |= np.uint32(1 << v)
    assert count.max(initial=0) < 1 << 32
    return count[:, 0].astype(np.uint32), count[:, 1].astype(np.uint32), mask
