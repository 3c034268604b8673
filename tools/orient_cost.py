#!/usr/bin/env python3
"""What consistent normal orientation costs (pointops.orient_normals, `python -m pdgn_amd.export --orient consistent`; DESIGN.md
section 7r):  python3 tools/orient_cost.py [--rounds R] [--out FILE] [--no-trace]   (FILE defaults to profiles/orient_cost.txt)

  kernels   20 calls of pointops.knnquery(16, x, x) + pointops.estimate_normals(x, idx=...) + pointops.orient_normals(x, g, idx=...) at
            each of the four level shapes of B = 35 (256, 512, 1024, 2048 points, k = 16) and nothing else in one child process under
            `rocprofv3 --kernel-trace --stats`: the three kernels' own times, per shape, and the orientation kernel's time per round
            (a cloud of n live points takes n rounds).  The clouds are unit spheres with 2 % radial noise.
  export    pdgn_amd.export.main on a saved array of 16 such clouds of 2048 points, --normals 16, in FRESH child processes, the second
            call of each child timed (host clock; the call ends with the device-to-host copies, so it is synchronised), the arms
            --orient outward and --orient consistent alternating over R rounds on one box."""
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
B, K = 35, 16
LEVELS = (256, 512, 1024, 2048)
EXPORT_CLOUDS, EXPORT_POINTS = 16, 2048
KERNELS = (("orient_kernel", "orient_kernel"), ("normals_kernel", "normals_kernel"), ("knnquery", "knn"))


def shells(count, points, seed=9999):
    import torch
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(count, points, 3, generator=g)
    return (c / c.norm(dim=2, keepdim=True) * (1.0 + 0.02 * torch.randn(count, points, 1, generator=g))).contiguous()


def kernels_child(launches):
    """The child of the kernel trace: per level shape, `launches` calls of the neighbour search, the normals kernel and the orientation."""
    import torch
    from pdgn_amd import pointops
    dev = torch.device("cuda:0")
    for n in LEVELS:
        x = shells(B, n, seed=n).to(dev)
        for _ in range(launches):
            idx = pointops.knnquery(K, x, x)
            g = pointops.estimate_normals(x, idx=idx)
            o, parent, stats = pointops.orient_normals(x, g, idx=idx, return_tree=True)
        torch.cuda.synchronize()
        outward = ((o * x).sum(-1) > 0).float().mean().item()
        print(json.dumps({"n": n, "outward": outward, "stats": stats.sum(dim=0).tolist()}))


def traced(launches):
    """([the child's JSON lines], {kernel: [(us, full name), in issue order]}) of the child under rocprofv3."""
    out = tempfile.mkdtemp(prefix="orient_cost_trace_")
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
            key = next((k for k, part in KERNELS if part in name.lower()), None)
            if key:
                by.setdefault(key, []).append(((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, name))
        return checks, by
    finally:
        shutil.rmtree(out, ignore_errors=True)


def export_child(arm, clouds):
    """`python -m pdgn_amd.export CLOUDS --normals 16 --orient ARM` twice in this process -> one JSON line with the second call's time."""
    from pdgn_amd import export
    out = tempfile.mkdtemp(prefix="orient_cost_export_")
    try:
        ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            export.main([clouds, "-o", out, "--normals", str(K), "--orient", arm])
            ms.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"arm": arm, "ms": ms[1], "first_ms": ms[0], "files": len(os.listdir(out))}))
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20, help="calls per level shape in the traced child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_cost.txt"), help="results file ('' for none)")
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
        launches = args.launches
        checks, by = traced(launches)
        say("(a) the kernels alone, rocprofv3 --kernel-trace --stats, %d calls of knnquery + estimate_normals + orient_normals per level shape "
            "of B = %d, k = %d, one process; unit spheres with 2 %% radial noise:" % (launches, B, K))
        med = {}
        for name, v in sorted(by.items()):
            # issue order: the four shapes one after the other, `launches` launches each
            for k, n in zip(range(0, len(v), launches), LEVELS):
                g = [us for us, _ in v[k:k + launches]]
                med[(name, n)] = statistics.median(g)
                say("  %-16s n = %4d: %3d launches, median %9.2f us, min %9.2f, max %9.2f   (%s)"
                    % (name, n, len(g), statistics.median(g), min(g), max(g), v[k][1][:48]))
        for n in LEVELS:
            if all((name, n) in med for name, _ in KERNELS):
                say("  n = %4d: orient %.3f us per round; orient / (knnquery + normals) = %.1f"
                    % (n, med[("orient_kernel", n)] / n, med[("orient_kernel", n)] / (med[("knnquery", n)] + med[("normals_kernel", n)])))
        for c in checks:
            say("  n = %4d: %.4f of the oriented normals point away from the centre; components, flipped, weak, dead over the %d clouds: %s"
                % (c["n"], c["outward"], B, " ".join(str(v) for v in c["stats"])))
    import numpy as np
    work = tempfile.mkdtemp(prefix="orient_cost_clouds_")
    try:
        clouds = os.path.join(work, "clouds.npy")
        np.save(clouds, shells(EXPORT_CLOUDS, EXPORT_POINTS).numpy())
        arms = ["outward", "consistent"]
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
    say("(b) python -m pdgn_amd.export on %d clouds of %d points, --normals %d, the second call of a fresh process:" % (EXPORT_CLOUDS, EXPORT_POINTS, K))
    for arm in arms:
        v = res[arm]
        say("  --orient %-10s ms mean %.1f min %.1f max %.1f spread %.1f over %d rounds; first call %.0f ms; %d files"
            % (arm, sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v), recs[arm]["first_ms"], recs[arm]["files"]))
    say("  consistent - outward: %+.1f ms per export" % (sum(res["consistent"]) / len(res["consistent"]) - sum(res["outward"]) / len(res["outward"])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
