#!/usr/bin/env python3
"""What the point-to-surface distance costs (meshes.point_to_mesh: pdgn_mesh_dist_prepare, pdgn_point_mesh_distance):
python3 tools/p2m_cost.py [--launches L] [--out FILE]          (FILE defaults to profiles/p2m_cost.txt)

One child process under `rocprofv3 --kernel-trace --stats` and nothing else in it: 35 clouds of 2048 points -- draws of the surface with
2 % Gaussian noise, which is where a generator's output lies -- against one mesh of about 1 k (icosphere of level 3), 10 k (torus grid
72 x 72) and 100 k faces (torus grid 224 x 224), all 35 clouds against the one shape.  Per mesh, every combination of
    cull     on / off
    points   as drawn (i.i.d.: no two neighbours in memory are neighbours in space) / in Morton order
    faces    shuffled (a face soup) / as the generator wrote them (rows of the grid) / records in Morton order of the centroids
L launches each through the raw entry point, so that a launch is the kernel alone; the prepare launch per face order; and, timed with
device events in the same child, what the wrapper adds per call to put the points in Morton order and the results back (argsort, gather,
three scatters).  All variants of a mesh are checked to give the same bits.  The times are the kernels' own from the trace, in issue
order."""
import argparse
import csv
import glob
import itertools
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N = 35, 2048
MESHES = (("1 k", "icosphere", 3), ("10 k", "torus", 72), ("100 k", "torus", 224))
FACE_ORDERS = ("shuffled", "given", "sorted")


def _mesh(kind, size):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import p2m_mirror as pm
    return pm.icosphere(size) if kind == "icosphere" else pm.torus_grid(size, size)


def child(launches):
    import numpy as np
    import torch
    from pdgn_amd import _lib, meshes
    dev = torch.device("cuda:0")
    L = _lib.lib()
    shape = torch.zeros(B, dtype=torch.int32, device=dev)
    for label, kind, size in MESHES:
        verts, faces = _mesh(kind, size)
        rng = np.random.default_rng(size)
        sets = {"given": meshes.MeshSet.from_meshes([(verts, faces)]).to(dev)}
        perm = rng.permutation(faces.shape[0])
        sets["shuffled"] = meshes.MeshSet.from_meshes([(verts, faces[perm])]).to(dev)
        sets["sorted"] = sets["shuffled"]
        ms = sets["given"]
        g = torch.Generator(device=dev).manual_seed(size)
        x = torch.cat([ms.sample(N, 7, draw=c) for c in range(B)]) + 0.02 * torch.randn(B, N, 3, device=dev, generator=g)
        x = x.contiguous()
        lo, hi = x.amin(dim=1, keepdim=True), x.amax(dim=1, keepdim=True)
        order = torch.argsort(meshes._morton30(x, lo, hi), dim=1, stable=True)
        points = {"as drawn": x, "Morton": torch.gather(x, 1, order[..., None].expand(-1, -1, 3)).contiguous()}
        results = {}
        for face_order in FACE_ORDERS:
            rec = meshes.mesh_dist_records(sets[face_order], sort_faces=face_order == "sorted")      # (one prepare launch in the trace)
            m = sets[face_order]
            for point_order, cull in itertools.product(points, (1, 0)):
                p = points[point_order]
                d2 = torch.empty(B, N, dtype=torch.float32, device=dev)
                face = torch.empty(B, N, dtype=torch.int32, device=dev)
                for _ in range(launches):
                    _lib.check(L.pdgn_point_mesh_distance(B, N, m.S, m.F, rec["G"], _lib.ptr(p), _lib.ptr(shape), _lib.ptr(m.face_off),
                                                          _lib.ptr(rec["group_off"]), _lib.ptr(rec["records"]), _lib.ptr(rec["groups"]), cull,
                                                          _lib.ptr(d2), _lib.ptr(face), None, _lib.stream_of(p)), "pdgn_point_mesh_distance")
                torch.cuda.synchronize()
                if point_order == "Morton":
                    d2 = torch.empty_like(d2).scatter_(1, order, d2)
                results[(face_order, point_order, cull)] = d2
        first = results[("given", "as drawn", 1)]
        same = all(torch.equal(first.view(torch.int32), r.view(torch.int32)) for r in results.values())
        # the wrapper's own work for sort_points, device events around 20 calls
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms_sort = []
        for _ in range(20):
            start.record()
            finite = torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
            o = torch.argsort(meshes._morton30(x, finite.amin(dim=1, keepdim=True), finite.amax(dim=1, keepdim=True)), dim=1, stable=True)
            xs = torch.gather(x, 1, o[..., None].expand(-1, -1, 3)).contiguous()
            a, b = torch.empty_like(first).scatter_(1, o, first), torch.empty_like(face).scatter_(1, o, face)
            stop.record()
            stop.synchronize()
            ms_sort.append(start.elapsed_time(stop))
        print(json.dumps({"mesh": label, "faces": int(faces.shape[0]), "same_bits": bool(same), "mean_distance": float(first.double().sqrt().mean()),
                          "sort_points_us": statistics.median(ms_sort) * 1e3, "kept": [int(xs.numel()), int(a.numel()), int(b.numel())]}))


def traced(launches):
    out = tempfile.mkdtemp(prefix="p2m_cost_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--launches", str(launches)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            raise RuntimeError("rocprofv3 child failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
        checks = [json.loads(l) for l in run.stdout.splitlines() if l.startswith("{")]
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        by = {"md_distance_kernel": [], "md_prepare_kernel": []}
        for r in rows:
            for key in by:
                if key in r["Kernel_Name"]:
                    by[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        return checks, by
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p2m_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.child:
        return child(args.launches)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    checks, by = traced(args.launches)                             # (this process never touches the GPU)
    say("pdgn_point_mesh_distance, rocprofv3 --kernel-trace --stats, %d clouds of %d points (surface draws with 2 %% noise) against one mesh, "
        "%d launches per variant, one process; kernel times in us, median (min .. max):" % (B, N, args.launches))
    dist, prep = by["md_distance_kernel"], by["md_prepare_kernel"]
    per_mesh = len(FACE_ORDERS) * 4 * args.launches
    assert len(dist) == per_mesh * len(MESHES) and len(prep) == len(MESHES) * len(FACE_ORDERS), (len(dist), len(prep))
    med = {}
    for mi, check in enumerate(checks):
        say("%s faces (%d): all variants the same bits: %s; mean distance %.4g; the wrapper's Morton order of the points and the way back: "
            "%.1f us per call (device events)" % (check["mesh"], check["faces"], check["same_bits"], check["mean_distance"], check["sort_points_us"]))
        at = mi * per_mesh
        for fi, face_order in enumerate(FACE_ORDERS):
            say("  faces %-8s  prepare launch %8.2f us" % (face_order, prep[mi * len(FACE_ORDERS) + fi]))
            for point_order, cull in itertools.product(("as drawn", "Morton"), (1, 0)):
                g = dist[at:at + args.launches]
                at += args.launches
                med[(check["mesh"], face_order, point_order, cull)] = statistics.median(g)
                say("    points %-8s cull %d: %10.2f (%10.2f .. %10.2f)" % (point_order, cull, statistics.median(g), min(g), max(g)))
    for check in checks:
        m = check["mesh"]
        say("%s: culled, faces sorted - shuffled: %+.1f us (points Morton); points Morton - as drawn: %+.1f us kernel, %+.1f us with the wrapper's "
            "sorting (faces sorted)" % (m, med[(m, "sorted", "Morton", 1)] - med[(m, "shuffled", "Morton", 1)],
                                        med[(m, "sorted", "Morton", 1)] - med[(m, "sorted", "as drawn", 1)],
                                        med[(m, "sorted", "Morton", 1)] - med[(m, "sorted", "as drawn", 1)] + check["sort_points_us"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
