#!/usr/bin/env python3
"""What surface reconstruction costs (pdgn_amd/reconstruct.py, `python -m pdgn_amd.export --mesh R`):
python3 tools/recon_cost.py [--rounds R] [--launches L] [--out FILE] [--no-trace]   (FILE defaults to profiles/recon_cost.txt)

  kernels   per shape -- 256, 512, 1024, 2048 points at R = 64 and 128 nodes per axis, B = 16, h = 5 mean spacings -- L calls of
            pointops.knnquery(16, x, x), estimate_normals, orient_normals, reconstruct.imls_grid with culling, the same without, and
            reconstruct.surface_nets, and nothing else, in one child process under `rocprofv3 --kernel-trace --stats` (a kernel trace
            only: counters are never collected in the same run): the kernels' own times per shape.  The clouds are unit spheres with 2 %
            radial noise.
  export    pdgn_amd.export.main on a saved array of 16 such clouds of 2048 points in FRESH child processes, the second call of each
            child timed (host clock; the call ends with device-to-host copies, so it is synchronised), the arms `--normals 16 --orient
            consistent` and `--mesh 64` alternating over R rounds on one box."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, K, FACTOR = 16, 16, 5.0
LEVELS = (256, 512, 1024, 2048)
RESOLUTIONS = (64, 128)
EXPORT_CLOUDS, EXPORT_POINTS, EXPORT_MESH = 16, 2048, 64
# (key, part of the kernel's name, launches per call of the child's loop)
KERNELS = (("imls_kernel", "imls_kernel", 2), ("sn_cells_kernel", "sn_cells_kernel", 1), ("sn_quads_kernel", "sn_quads_kernel", 1),
           ("sn_emit_kernel", "sn_emit_kernel", 1), ("orient_kernel", "orient_kernel", 1), ("normals_kernel", "normals_kernel", 1),
           ("knnquery", "knn", 1))


def shells(count, points, seed=9999):
    import torch
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(count, points, 3, generator=g)
    return (c / c.norm(dim=2, keepdim=True) * (1.0 + 0.02 * torch.randn(count, points, 1, generator=g))).contiguous()


def kernels_child(launches):
    """The child of the kernel trace.  Per shape: `launches` turns of the neighbour search, the normals, the orientation and the
    extraction, then `launches` field launches with culling and `launches` without (so a shape's field launches come in that order)."""
    import torch
    from pdgn_amd import pointops, reconstruct
    dev = torch.device("cuda:0")
    for R in RESOLUTIONS:
        for n in LEVELS:
            x = shells(B, n, seed=n).to(dev)
            h = FACTOR * reconstruct.mean_spacing(x)
            origin, voxel, inv = reconstruct.grid_for(x, R, h)
            for _ in range(launches):
                idx = pointops.knnquery(K, x, x)
                g = pointops.estimate_normals(x, idx=idx)
                o = pointops.orient_normals(x, g, idx=idx)
            for cull in (True, False):
                for _ in range(launches):
                    field = reconstruct.imls_grid(x, o, origin, voxel, inv, R, cull=cull)
            for _ in range(launches):
                verts, faces, vert_off, face_off, stats = reconstruct.surface_nets(field, origin, voxel)
            torch.cuda.synchronize()
            print(json.dumps({"R": R, "n": n, "valid": float((~torch.isnan(field)).float().mean()), "stats": stats.sum(dim=0).tolist(),
                              "h": float(h.mean())}))


def traced(launches):
    """([the child's JSON lines], {kernel: [(us, full name), in issue order]}) of the child under rocprofv3."""
    out = tempfile.mkdtemp(prefix="recon_cost_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--kernels-child", "--launches", str(launches)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            raise RuntimeError("rocprofv3 child failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
        checks = [json.loads(l) for l in run.stdout.splitlines() if l.startswith("{")]
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        by = {}
        for r in rows:
            name = r["Kernel_Name"].split("(")[0]
            key = next((k for k, part, _ in KERNELS if part in name.lower()), None)
            if key:
                by.setdefault(key, []).append(((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, name))
        return checks, by
    finally:
        shutil.rmtree(out, ignore_errors=True)


def export_child(arm, clouds):
    """The export command twice in this process -> one JSON line with the second call's time."""
    from pdgn_amd import export
    out = tempfile.mkdtemp(prefix="recon_cost_export_")
    extra = ["--mesh", str(EXPORT_MESH)] if arm == "mesh" else ["--normals", str(K), "--orient", "consistent"]
    try:
        ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            export.main([clouds, "-o", out] + extra)
            ms.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"arm": arm, "ms": ms[1], "first_ms": ms[0], "files": len(os.listdir(out))}))
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=5, help="calls per shape in the traced child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--export-child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.kernels_child:
        return kernels_child(args.launches)
    if args.export_child:
        return export_child(*args.export_child)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # (this process never touches the GPU: every measurement is a child's)
    if not args.no_trace:
        L = args.launches
        checks, by = traced(L)
        shapes = [(R, n) for R in RESOLUTIONS for n in LEVELS]
        say("(a) the kernels alone, rocprofv3 --kernel-trace --stats, %d calls per shape, B = %d, k = %d, h = %g mean spacings, one process; "
            "unit spheres with 2 %% radial noise; median us (min .. max):" % (L, B, K, FACTOR))
        med = {}
        for key, _, per_call in KERNELS:
            v = by.get(key, [])
            if len(v) != per_call * L * len(shapes):
                say("  %-16s %d launches in the trace, %d expected: not attributed" % (key, len(v), per_call * L * len(shapes)))
                continue
            for s, (R, n) in enumerate(shapes):
                group = [us for us, _ in v[s * per_call * L:(s + 1) * per_call * L]]
                parts = (("culled", group[:L]), ("un-culled", group[L:])) if key == "imls_kernel" else (("", group),)
                for label, g in parts:
                    med[(key, label, R, n)] = statistics.median(g)
                    say("  %-16s %-9s R = %3d n = %4d: %10.1f (%10.1f .. %10.1f)" % (key, label, R, n, statistics.median(g), min(g), max(g)))
        for R, n in shapes:
            if ("imls_kernel", "culled", R, n) in med:
                c, u = med[("imls_kernel", "culled", R, n)], med[("imls_kernel", "un-culled", R, n)]
                visits = B * R ** 3 * n
                say("  R = %3d n = %4d: un-culled %.2f ms = %.1f G visits/s; culled %.3f ms, %.1f times faster"
                    % (R, n, u / 1e3, visits / u / 1e3, c / 1e3, u / c))
        for c in checks:
            say("  R = %3d n = %4d: h %.4f, %.3f of the nodes valid; vertices, faces, open edges, invalid nodes over the %d clouds: %s"
                % (c["R"], c["n"], c["h"], c["valid"], B, " ".join(str(v) for v in c["stats"])))
    import numpy as np
    work = tempfile.mkdtemp(prefix="recon_cost_clouds_")
    try:
        clouds = os.path.join(work, "clouds.npy")
        np.save(clouds, shells(EXPORT_CLOUDS, EXPORT_POINTS).numpy())
        arms = ["consistent", "mesh"]
        res, recs = {a: [] for a in arms}, {}
        for r in range(args.rounds):
            for arm in (arms if r % 2 == 0 else arms[::-1]):
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--export-child", arm, clouds], cwd=ROOT,
                                     capture_output=True, text=True, timeout=600)
                line = [l for l in run.stdout.splitlines() if l.startswith("{")]
                if run.returncode != 0 or not line:
                    raise RuntimeError("export child %s failed:\n%s" % (arm, run.stdout[-2000:] + run.stderr[-2000:]))
                rec = json.loads(line[0])
                res[arm].append(rec["ms"])
                recs[arm] = rec
                print("round %d %-10s %.1f ms" % (r, arm, rec["ms"]), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    say("(b) python -m pdgn_amd.export on %d clouds of %d points, the second call of a fresh process:" % (EXPORT_CLOUDS, EXPORT_POINTS))
    for arm, flags in zip(arms, ("--normals %d --orient consistent" % K, "--mesh %d" % EXPORT_MESH)):
        v = res[arm]
        say("  %-34s ms mean %.1f min %.1f max %.1f spread %.1f over %d rounds; first call %.0f ms; %d files"
            % (flags, sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v), recs[arm]["first_ms"], recs[arm]["files"]))
    say("  mesh - consistent: %+.1f ms per export" % (sum(res["mesh"]) / len(res["mesh"]) - sum(res["consistent"]) / len(res["consistent"])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
