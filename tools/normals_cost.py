#!/usr/bin/env python3
"""What surface normals cost (pointops.estimate_normals, lit sheets and surface statistics in the reports):
python3 tools/normals_cost.py [--rounds R] [--parent DIR] [--out FILE] [--no-trace]   (FILE defaults to profiles/normals_cost.txt)

  kernels   20 calls of pointops.knnquery(16, x, x) + pointops.estimate_normals(x, idx=...) at each of the four level shapes of B = 35
            (256, 512, 1024, 2048 points, k = 16) and nothing else in one child process under `rocprofv3 --kernel-trace --stats`: the
            neighbour search's and the normals kernel's own times, per shape.  The clouds are unit spheres with 2 % radial noise.
  report    one SnapshotReporter call (8 rows, 140 held-out clouds of 2048 points, batches of 35, the quick metrics) in FRESH child
            processes on a freshly initialised trainer, the third call of each child timed (host clock around a synchronised call), the
            arms alternating over R rounds on one box: this tree's plain report, this tree with lit=True and surface=True, and -- with
            --parent DIR, a built checkout of the parent commit -- the parent's plain report.  The held-out clouds' statistics are cached
            after the first call, as in a training run."""
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
B, N, K, VAL = 35, 2048, 16, 140
LEVELS = (256, 512, 1024, 2048)


def shells(count, points, dev, seed=9999):
    import torch
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(count, points, 3, generator=g)
    c = c / c.norm(dim=2, keepdim=True) * (1.0 + 0.02 * torch.randn(count, points, 1, generator=g))
    return c.to(dev).contiguous()


def kernels_child(launches):
    """The child of the kernel trace: per level shape, `launches` calls of the neighbour search and of the normals kernel."""
    import torch
    from pdgn_amd import pointops
    dev = torch.device("cuda:0")
    for n in LEVELS:
        x = shells(B, n, dev, seed=n)
        for _ in range(launches):
            idx = pointops.knnquery(K, x, x)
            normals, eig = pointops.estimate_normals(x, idx=idx, return_eig=True)
        torch.cuda.synchronize()
        sv = (eig[..., 0].double().clamp_min(0) / eig.double().sum(-1)).mean().item()
        print(json.dumps({"n": n, "finite": bool(torch.isfinite(normals).all().item()), "sv_mean": sv}))


def traced(launches):
    """([the child's JSON lines], {kernel: [(us, full name), in issue order]}) of the child under rocprofv3."""
    out = tempfile.mkdtemp(prefix="normals_cost_trace_")
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
            key = "normals_kernel" if "normals_kernel" in name else "knnquery" if "knn" in name.lower() else None
            if key:
                by.setdefault(key, []).append(((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, name))
        return checks, by
    finally:
        shutil.rmtree(out, ignore_errors=True)


def report_child(arm):
    """One arm of the report in this process -> one JSON line.  arm: plain | lit | parent (= plain, on whatever tree this file lies in)."""
    import torch
    from pdgn_amd.data import normalize_clouds
    from pdgn_amd.report import SnapshotReporter
    from pdgn_amd.trainer import PDGNTrainer
    dev = torch.device("cuda:0")
    val = normalize_clouds(shells(VAL, N, dev), "shape_bbox")[0].contiguous()
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    out = tempfile.mkdtemp(prefix="normals_cost_report_")
    try:
        kw = {"lit": True, "surface": True} if arm == "lit" else {}
        reporter = SnapshotReporter(tr, val, out, every=1, batch_size=B, normalize="shape_bbox", seed=9, rows=8, **kw)
        ms = []
        for epoch in (1, 2, 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reporter(epoch)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec = {"arm": arm, "ms": ms[2], "first_ms": ms[0], "files": sorted(os.listdir(out))}
        if arm == "lit":
            rec["surface"] = {"gen": reporter.last_surface[1], "val": reporter.last_surface[2]}
        print(json.dumps(rec))
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20, help="calls per level shape in the traced child")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its plain report as a third arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--report-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.kernels_child:
        return kernels_child(args.launches)
    if args.report_child:
        return report_child(args.report_child)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # (this process never touches the GPU: every measurement is a child's)
    if not args.no_trace:
        launches = args.launches
        checks, by = traced(launches)
        say("(a) the kernels alone, rocprofv3 --kernel-trace --stats, %d calls of knnquery + estimate_normals per level shape of B = %d, k = %d, "
            "one process; unit spheres with 2 %% radial noise:" % (launches, B, K))
        med = {}
        for name, v in sorted(by.items()):
            # issue order: the four shapes one after the other, `launches` launches each
            for k, n in zip(range(0, len(v), launches), LEVELS):
                g = [us for us, _ in v[k:k + launches]]
                med[(name, n)] = statistics.median(g)
                say("  %-16s n = %4d: %3d launches, median %8.2f us, min %8.2f, max %8.2f   (%s)"
                    % (name, n, len(g), statistics.median(g), min(g), max(g), v[k][1][:48]))
        for n in LEVELS:
            if ("normals_kernel", n) in med and ("knnquery", n) in med:
                say("  n = %4d: normals / knnquery = %.3f; %.2f G points / s" % (n, med[("normals_kernel", n)] / med[("knnquery", n)],
                                                                              B * n / med[("normals_kernel", n)] / 1e3))
        for c in checks:
            say("  n = %4d: normals %s, mean surface variation %.6g" % (c["n"], "finite" if c["finite"] else "NOT FINITE", c["sv_mean"]))
    arms = (["parent"] if args.parent else []) + ["plain", "lit"]
    if args.parent:
        args.parent = os.path.abspath(args.parent)
        shutil.copy(os.path.abspath(__file__), os.path.join(args.parent, "tools", "normals_cost.py"))
    res, recs = {a: [] for a in arms}, {}
    for r in range(args.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            cwd = args.parent if arm == "parent" else ROOT
            run = subprocess.run([sys.executable, os.path.join(cwd, "tools", "normals_cost.py"), "--report-child", arm],
                                 cwd=cwd, capture_output=True, text=True, timeout=600)
            line = [l for l in run.stdout.splitlines() if l.startswith("{")]
            if run.returncode != 0 or not line:
                raise RuntimeError("report child %s failed:\n%s" % (arm, run.stdout[-2000:] + run.stderr[-2000:]))
            rec = json.loads(line[0])
            res[arm].append(rec["ms"])
            recs[arm] = rec
            print("round %d %-8s %.1f ms" % (r, arm, rec["ms"]), flush=True)
    names = {"parent": "parent commit, plain report", "plain": "this tree, plain report", "lit": "this tree, lit=True surface=True"}
    say("(b) one report (8 rows, %d held-out clouds of %d points, batches of %d, quick metrics), the third call of a fresh process:" % (VAL, N, B))
    for arm in arms:
        v = res[arm]
        say("  %-36s ms mean %.1f min %.1f max %.1f spread %.1f over %d rounds; first call %.0f ms; files %s"
            % (names[arm], sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v), recs[arm]["first_ms"], " ".join(recs[arm]["files"])))
    mean = {a: sum(res[a]) / len(res[a]) for a in arms}
    s = recs["lit"]["surface"]
    say("  lit - plain: %+.1f ms per report; generated sv_mean %.6g sv_p90 %.6g degenerate %d; held-out sv_mean %.6g sv_p90 %.6g"
        % (mean["lit"] - mean["plain"], s["gen"]["sv_mean"], s["gen"]["sv_p90"], s["gen"]["degenerate"], s["val"]["sv_mean"], s["val"]["sv_p90"]))
    if args.parent:
        say("  plain - parent: %+.1f ms; the parent's run-to-run spread %.1f ms" % (mean["plain"] - mean["parent"], max(res["parent"]) - min(res["parent"])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
