"""Point clouds out of the project in a form mesh tools read: binary little-endian PLY, with per-point normals where wanted (what Poisson
reconstruction, MeshLab and Blender take).

    write_ply("chair.ply", xyz, normals)
    python -m pdgn_amd.export results/GEN_Ours_chair_<time>/out.npy -o plys --count 16 --normals 16 --orient outward
    python -m pdgn_amd.export results/GEN_Ours_chair_<time>/out.npy -o plys --count 16 --normals 16 --orient consistent
    python -m pdgn_amd.export results/GEN_Ours_chair_<time>/out.npy -o plys --count 16 --normals 16 --orient visible
    python -m pdgn_amd.export results/GEN_Ours_chair_<time>/out.npy -o plys --count 16 --mesh 64
    write_ply("chair_mesh.ply", verts, faces=faces);  write_obj("chair_mesh.obj", verts, faces)

The writers are struct and numpy only, as report.write_png is; only the command line's --normals and --mesh touch the device
(pointops.estimate_normals; --orient consistent: pointops.orient_normals, section 7r; --orient visible: pointops.orient_normals_visible, section 7z; --mesh: reconstruct.imls_field and
reconstruct.surface_nets, section 7s)."""
import argparse
import os
import struct
import sys

import numpy as np

PLY_PROPERTIES = ("x", "y", "z", "nx", "ny", "nz")
CONSISTENT_MAX_POINTS = 4096                                       # PDGN_ORIENT_MAX_N
VISIBLE_MAX_POINTS = 8192                                          # PDGN_REPULSION_MAX_N: the spacing behind --orient_radius_factor
MESH_FORMATS = ("ply", "obj")
MESH_BATCH_NODES = 1 << 24                                         # --mesh: clouds per field launch so that B R^3 floats stay at 64 MB


def write_ply(path, xyz, normals=None, faces=None):
    """One cloud or mesh as a binary little-endian PLY: xyz (N,3), normals (N,3) or None (numpy arrays, or tensors on any device) -> a
    vertex element of N records `float x y z` (with normals: `float x y z nx ny nz`), the values' fp32 bits as they are (NaNs included).
    faces (F,3) integers below N, or None: with faces an `element face F` follows, `property list uchar int vertex_indices`, every record
    the byte 3 and three int32; without, the file has no face element at all."""
    def host(a, name):
        if hasattr(a, "detach"):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1 or a.dtype.kind != "f":
            raise ValueError("write_ply: %s must be a non-empty (N,3) float array, got %s %s" % (name, a.dtype, a.shape))
        return a.astype("<f4")
    rows = host(xyz, "xyz")
    if normals is not None:
        nrm = host(normals, "normals")
        if nrm.shape != rows.shape:
            raise ValueError("write_ply: %d points and %d normals" % (rows.shape[0], nrm.shape[0]))
        rows = np.concatenate([rows, nrm], axis=1)
    header = ["ply", "format binary_little_endian 1.0", "comment pdgn_amd.export", "element vertex %d" % rows.shape[0]]
    header += ["property float %s" % name for name in PLY_PROPERTIES[:rows.shape[1]]]
    payload = np.ascontiguousarray(rows).tobytes()
    assert len(payload) == struct.calcsize("<%df" % rows.size)
    if faces is not None:
        tri = _triangles(faces, rows.shape[0], "write_ply")
        header += ["element face %d" % tri.shape[0], "property list uchar int vertex_indices"]
        rec = np.empty(tri.shape[0], dtype=[("count", "u1"), ("index", "<i4", (3,))])
        rec["count"], rec["index"] = 3, tri
        payload += rec.tobytes()
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii") + payload)
    return path


def _triangles(faces, count, who):
    if hasattr(faces, "detach"):
        faces = faces.detach().cpu().numpy()
    tri = np.asarray(faces)
    if tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu":
        raise ValueError("%s: faces must be an (F,3) integer array, got %s %s" % (who, tri.dtype, tri.shape))
    if tri.size and (tri.min() < 0 or tri.max() >= count):
        raise ValueError("%s: a face names a vertex outside the %d vertices" % (who, count))
    return tri.astype("<i4")


def write_obj(path, verts, faces):
    """One mesh as a Wavefront OBJ in plain text: `v x y z` lines with nine significant digits (an fp32 value survives the round trip),
    then `f a b c` lines, indices from 1.  verts (V,3) floats, faces (F,3) integers below V (numpy arrays, or tensors on any device)."""
    if hasattr(verts, "detach"):
        verts = verts.detach().cpu().numpy()
    v = np.asarray(verts)
    if v.ndim != 2 or v.shape[1] != 3 or v.dtype.kind != "f":
        raise ValueError("write_obj: verts must be a (V,3) float array, got %s %s" % (v.dtype, v.shape))
    tri = _triangles(faces, v.shape[0], "write_obj")
    with open(path, "w") as f:
        f.write("# pdgn_amd.export\n")
        f.writelines("v %.9g %.9g %.9g\n" % tuple(row) for row in v.astype(np.float32).tolist())
        f.writelines("f %d %d %d\n" % tuple(row) for row in (tri + 1).tolist())
    return path


class _Given(argparse.Action):
    """Stores the value and notes that the option was on the command line (--mesh changes --orient's default)."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "_given", True)


def build_parser():
    p = argparse.ArgumentParser(prog="python -m pdgn_amd.export", description="write clouds of a saved (S, N, 3) array (the test phase's "
                                "out.npy) as PLY files, one per cloud")
    p.add_argument("clouds", help=".npy file holding (S, N, 3) or (S, 3, N) clouds")
    p.add_argument("-o", "--output", required=True, metavar="DIR", help="directory for cloud_<index>.ply (created)")
    p.add_argument("--first", type=int, default=0, help="index of the first cloud written")
    p.add_argument("--count", type=int, default=None, help="clouds written (default: all from --first on)")
    p.add_argument("--normals", type=int, default=None, metavar="K", help="add per-point normals estimated from the K nearest neighbours "
                   "(pointops.estimate_normals; needs the device)")
    p.add_argument("--orient", choices=["outward", "consistent", "visible", "none"], default="outward", action=_Given, help="--normals: outward (default) turns every "
                   "normal away from its cloud's centroid -- a heuristic that is right for roughly convex shapes and wrong inside concavities; "
                   "consistent propagates the sign along a minimum spanning tree of the neighbour graph from each component's highest point "
                   "(what Poisson reconstruction needs; clouds of at most %d points); visible asks a ring of orthographic views which side of "
                   "every point they see and pools the answers over each point's tangent plane (thin sheets -- seats, table tops --, which "
                   "consistent gets wrong; needs views that reach the surface); none leaves the sign convention of the estimate "
                   "(largest component non-negative)" % CONSISTENT_MAX_POINTS)
    p.add_argument("--orient_views", type=int, choices=[6, 14, 26], default=None, help="--orient visible: the number of views (default 26)")
    p.add_argument("--orient_resolution", type=int, default=None, metavar="R", help="--orient visible: pixels per side of a view's depth "
                   "buffer, 1 .. 192 (default 64)")
    p.add_argument("--orient_radius_factor", type=float, default=None, metavar="F", help="--orient visible: a point is splatted as a disc "
                   "of F times its cloud's mean nearest-neighbour distance (default 2)")
    p.add_argument("--orient_rounds", type=int, default=None, metavar="N", help="--orient visible: pooling rounds, 0 .. 4 (default 1)")
    p.add_argument("--mesh", type=int, default=None, metavar="R", help="also reconstruct every cloud's surface on a grid of R nodes per axis "
                   "(reconstruct.imls_field and surface_nets; needs the device) and write mesh_<index>.<ext> beside the cloud; implies "
                   "--normals 16 --orient consistent unless they are given, and refuses --orient none")
    p.add_argument("--mesh_radius", type=float, default=None, metavar="H", help="--mesh: the support radius h of the field's weight")
    p.add_argument("--mesh_radius_factor", type=float, default=None, metavar="F", help="--mesh: h = F times each cloud's mean "
                   "nearest-neighbour distance (default 5; not together with --mesh_radius)")
    p.add_argument("--mesh_format", choices=MESH_FORMATS, default="ply")
    p.add_argument("--device", default="cuda")
    return p


def main(argv=None):
    """`outward` is ("away", centroid): a heuristic for roughly convex shapes, not a globally consistent orientation.  `consistent` is
    spanning-tree propagation (pointops.orient_normals), all selected clouds in one batched call."""
    p = build_parser()
    args = p.parse_args(argv)
    if args.mesh is None:
        if args.mesh_radius is not None or args.mesh_radius_factor is not None or args.mesh_format != "ply":
            p.error("--mesh_radius, --mesh_radius_factor and --mesh_format go with --mesh")
    else:
        if args.orient == "none":
            p.error("--mesh needs oriented normals: --orient outward, consistent or visible, not none")
        if not 2 <= args.mesh <= 256:
            p.error("--mesh %d: between 2 and 256 nodes per axis" % args.mesh)
        if args.mesh_radius is not None and args.mesh_radius_factor is not None:
            p.error("--mesh_radius and --mesh_radius_factor exclude each other")
        for name in ("mesh_radius", "mesh_radius_factor"):
            if getattr(args, name) is not None and not getattr(args, name) > 0:
                p.error("--%s must be positive" % name)
        if args.normals is None:
            args.normals = 16
        if not getattr(args, "orient_given", False):
            args.orient = "consistent"
    visible_opts = ("orient_views", "orient_resolution", "orient_radius_factor", "orient_rounds")
    if args.orient != "visible" and any(getattr(args, name) is not None for name in visible_opts):
        p.error("--orient_views, --orient_resolution, --orient_radius_factor and --orient_rounds go with --orient visible")
    if args.orient == "visible":
        if args.orient_resolution is not None and not 1 <= args.orient_resolution <= 192:
            p.error("--orient_resolution %d: between 1 and 192 pixels per side" % args.orient_resolution)
        if args.orient_radius_factor is not None and not args.orient_radius_factor > 0:
            p.error("--orient_radius_factor must be positive")
        if args.orient_rounds is not None and not 0 <= args.orient_rounds <= 4:
            p.error("--orient_rounds %d: between 0 and 4" % args.orient_rounds)
    pcs = np.load(args.clouds)
    if pcs.ndim != 3 or 3 not in pcs.shape[1:]:
        raise SystemExit("%s: expected (S, N, 3) or (S, 3, N), got %s" % (args.clouds, pcs.shape))
    if pcs.shape[2] != 3:
        pcs = pcs.transpose(0, 2, 1)
    if not 0 <= args.first < pcs.shape[0] or (args.count is not None and args.count < 1):
        p.error("--first %d --count %r: the file holds %d clouds" % (args.first, args.count, pcs.shape[0]))
    if args.normals is not None and not 1 <= args.normals <= pcs.shape[1]:
        p.error("--normals %d: between 1 and the clouds' %d points" % (args.normals, pcs.shape[1]))
    if args.normals is not None and args.orient == "consistent":
        if pcs.shape[1] > CONSISTENT_MAX_POINTS:
            p.error("--orient consistent: clouds of at most %d points, the file's have %d" % (CONSISTENT_MAX_POINTS, pcs.shape[1]))
        if args.normals > 64:
            p.error("--orient consistent: --normals at most 64, got %d" % args.normals)
    if args.normals is not None and args.orient == "visible":
        if pcs.shape[1] > VISIBLE_MAX_POINTS:
            p.error("--orient visible: the spacing is measured on clouds of at most %d points, the file's have %d" % (VISIBLE_MAX_POINTS, pcs.shape[1]))
        if args.normals > 64:
            p.error("--orient visible: --normals at most 64, got %d" % args.normals)
    stop = pcs.shape[0] if args.count is None else min(pcs.shape[0], args.first + args.count)
    pcs = np.ascontiguousarray(pcs[args.first:stop], dtype=np.float32)
    normals = [None] * pcs.shape[0]
    tree = ""
    if args.normals is not None:
        import torch
        from .pointops import estimate_normals
        dev = torch.device(args.device)
        if args.orient == "consistent":                          # (no centroid argument: every cloud in one batched call)
            from .pointops import knnquery, orient_normals
            x = torch.from_numpy(pcs).to(dev)
            idx = knnquery(args.normals, x, x)
            oriented, _, stats = orient_normals(x, estimate_normals(x, idx=idx), idx=idx, return_tree=True)
            normals = list(oriented.cpu().numpy())
            tree = " (%d components, %d weak tree edges)" % tuple(stats[:, [0, 2]].sum(dim=0).tolist())
        elif args.orient == "visible":                            # (every cloud in one batched call)
            from .pointops import knnquery, orient_normals_visible
            x = torch.from_numpy(pcs).to(dev)
            idx = knnquery(args.normals, x, x)
            opts = {"views": args.orient_views, "resolution": args.orient_resolution, "radius_factor": args.orient_radius_factor,
                    "rounds": args.orient_rounds}
            oriented, stats = orient_normals_visible(x, estimate_normals(x, idx=idx), idx=idx, return_stats=True,
                                                     **{name: v for name, v in opts.items() if v is not None})
            normals = list(oriented.cpu().numpy())
            tree = " (%d points undecided, %d unseen by every view)" % tuple(stats[:, [1, 2]].sum(dim=0).tolist())
        else:
            for i in range(pcs.shape[0]):                        # (a cloud at a time: the centroid is an argument of the launch)
                x = torch.from_numpy(pcs[i:i + 1]).to(dev)
                orient = ("away", x[0].double().mean(dim=0).tolist()) if args.orient == "outward" else None
                normals[i] = estimate_normals(x, args.normals, orient=orient)[0].cpu().numpy()
    meshes, mesh = [], ""
    if args.mesh is not None:
        meshes, totals = _meshes(pcs, np.stack(normals), args, torch.device(args.device))
        mesh = "; meshes at %d nodes per axis: %d vertices, %d faces, %d open edges, %d non-manifold edges" % ((args.mesh,) + totals)
    os.makedirs(args.output, exist_ok=True)
    for i in range(pcs.shape[0]):
        write_ply(os.path.join(args.output, "cloud_%d.ply" % (args.first + i)), pcs[i], normals[i])
    for i, (verts, faces) in enumerate(meshes):
        path = os.path.join(args.output, "mesh_%d.%s" % (args.first + i, args.mesh_format))
        if args.mesh_format == "obj":
            write_obj(path, verts, faces)
        elif verts.shape[0]:
            write_ply(path, verts, faces=faces)
        else:                                                    # (a PLY may be empty, write_ply's clouds may not)
            with open(path, "wb") as f:
                f.write(b"ply\nformat binary_little_endian 1.0\ncomment pdgn_amd.export\nelement vertex 0\nproperty float x\nproperty float y\n"
                        b"property float z\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n")
    print("%s: %d clouds%s" % (args.output, pcs.shape[0], "" if args.normals is None else ", normals from %d neighbours" % args.normals) + tree + mesh)
    return args.output


def _meshes(pcs, normals, args, dev):
    """--mesh: ([(verts, faces) numpy, one per cloud], (vertices, faces, open edges, non-manifold edges) over the run); a few clouds per
    field launch."""
    import torch
    from . import reconstruct
    per = max(1, MESH_BATCH_NODES // args.mesh ** 3)
    out, totals = [], [0, 0, 0, 0]
    for lo in range(0, pcs.shape[0], per):
        x = torch.from_numpy(pcs[lo:lo + per]).to(dev)
        g = torch.from_numpy(np.ascontiguousarray(normals[lo:lo + per], dtype=np.float32)).to(dev)
        field, origin, voxel = reconstruct.imls_field(x, g, args.mesh, args.mesh_radius,
                                                      5.0 if args.mesh_radius_factor is None else args.mesh_radius_factor)
        verts, faces, vert_off, face_off, stats = reconstruct.surface_nets(field, origin, voxel)
        verts, faces, vert_off, face_off, stats = (t.cpu().numpy() for t in (verts, faces, vert_off, face_off, stats))
        for c in range(x.shape[0]):
            v, f = verts[vert_off[c]:vert_off[c + 1]], faces[face_off[c]:face_off[c + 1]]
            out.append((v, f))
            totals[3] += reconstruct.mesh_report(v, f, components=False)["nonmanifold_edges"]
        for col in range(3):
            totals[col] += int(stats[:, col].sum())
    return out, tuple(totals)


if __name__ == "__main__":
    main()
    sys.exit(0)
