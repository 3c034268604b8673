#!/usr/bin/env python3
"""What normal orientation from visibility (pdgn_cloud_normal_votes and pdgn_orient_pool) costs beside the steps
it follows and the propagation it stands beside:
python3 tools/visible_orient_cost.py [--calls K] [--rounds R] [--out FILE]   (FILE defaults to profiles/visible_orient_cost.txt)

  kernels   B = 35 tori of 256 / 512 / 1024 / 2048 points, and B = 4 of 15 000: K calls each of knnquery(16), estimate_normals,
            orient_normals (not at 15 000: beyond its limit) and orient_normals_visible at its defaults (at 15 000 with a given radius of
            two expected spacings: the spacing launch holds 8192 points), one child process per shape under `rocprofv3 --kernel-trace
            --stats` (a run of its own, kernel trace only), every kernel by name.
  export    `export --normals 16 --orient consistent` against `--orient visible` on 16 tori of 2048 points, the arms alternating over R
            rounds in ONE child process, wall clock of the whole call (writing the files included).
The expectation is written into the file before the first GPU step.  Every GPU step is a child process under its own `timeout`; the
tool stops at the first step that fails."""
import argparse
import csv
import glob
import json
import math
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import mesh_cost as mc                                           # noqa: E402  (its `step`)

SHAPES = ((35, 256), (35, 512), (35, 1024), (35, 2048), (4, 15000))
K, EXPORTED = 16, 16
NAMES = ("knn", "normals", "orient_kernel", "repulsion", "cloudvis")
EXPECTATION = """expectation, written before the first run (nothing is measured yet):
  votes    a workgroup per (cloud, view): 35 x 26 = 910 workgroups of 256 threads, each reading its cloud once per pass (24 n bytes from
           L2) and issuing about 10 LDS minima per point; at n = 2048 that is 8 points per thread and pass, nothing sequential: tens of
           microseconds, far below the propagation's 2.7 ms at that shape (section 7r), and growing linearly in n where the propagation
           grows faster than n.  At 15 000 points, B = 4, 104 workgroups of 59 points per thread: still below a millisecond.
  pooling  one thread per point and 16 slots of 32 gathered bytes per round: of the order of the normals kernel (11 us at 35 x 2048),
           the apply launch a few microseconds.
  spacing  radius=None adds the all-pairs launch of reconstruct.mean_spacing, n^2 per cloud: expected to be the largest part of the
           default call at 2048 points, and of the order of the knn launch (117 us at 35 x 2048).
  export   --orient visible replaces one 2.7 ms class launch by launches of tens of microseconds: the call is dominated by the host
           (reading, writing 16 files), so the two arms differ by less than their spread.
measured:"""


def tori(b, n, dev):
    """(b,n,3) points on the torus R = 1, r = 0.4 (uniform in the two angles, seeded: a cost run needs no uniform density)."""
    import torch
    g = torch.Generator().manual_seed(1000 + n)
    u, v = torch.rand(b, n, generator=g, dtype=torch.float64) * 2 * math.pi, torch.rand(b, n, generator=g, dtype=torch.float64) * 2 * math.pi
    ring = 1.0 + 0.4 * torch.cos(v)
    return torch.stack([ring * torch.cos(u), ring * torch.sin(u), 0.4 * torch.sin(v)], dim=2).float().contiguous().to(dev)


def kernels_child(b, n, calls):
    import torch
    from pdgn_amd import pointops
    dev = torch.device("cuda:0")
    x = tori(b, n, dev)
    radius = None if n <= pointops.VISIBLE_SPACING_MAX_N else 2.0 * 0.5 * math.sqrt(4 * math.pi ** 2 * 0.4 / n)   # two expected spacings
    for _ in range(calls):
        idx = pointops.knnquery(K, x, x)
    for _ in range(calls):
        g = pointops.estimate_normals(x, idx=idx)
    if n <= pointops.ORIENT_MAX_N:
        for _ in range(calls):
            pointops.orient_normals(x, g, idx=idx)
    for _ in range(calls):
        o, stats = pointops.orient_normals_visible(x, g, idx=idx, radius=radius, return_stats=True)
    torch.cuda.synchronize()
    print(json.dumps({"stats": stats.sum(dim=0).tolist()}))


def _trace(cmd, cwd):
    """{kernel name: [ms]} of the kernels of NAMES of a child under rocprofv3, and what the child printed."""
    out = tempfile.mkdtemp(prefix="visible_orient_cost_trace_")
    try:
        said = mc.step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + cmd, cwd, 600)
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        rows = {}
        for r in csv.DictReader(open(path)):
            if any(s in r["Kernel_Name"] for s in NAMES):
                rows.setdefault(r["Kernel_Name"].split("(")[0], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
        return rows, said
    finally:
        shutil.rmtree(out, ignore_errors=True)


def export_child(rounds):
    """Both arms in this process, alternating -> one JSON line of seconds per round."""
    import contextlib
    import io
    import numpy as np
    import torch
    from pdgn_amd import export
    root = tempfile.mkdtemp(prefix="visible_orient_cost_export_")
    try:
        np.save(os.path.join(root, "tori.npy"), tori(EXPORTED, 2048, torch.device("cpu")).numpy())
        arms = ("consistent", "visible")
        res = {a: [] for a in arms}
        said = {}
        for r in range(rounds + 1):                              # (round 0 warms up)
            for arm in (arms if r % 2 else arms[::-1]):
                buf = io.StringIO()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(buf):
                    export.main([os.path.join(root, "tori.npy"), "-o", os.path.join(root, arm), "--normals", str(K), "--orient", arm])
                if r:
                    res[arm].append(time.perf_counter() - t0)
                said[arm] = buf.getvalue().strip().split(": ", 1)[-1]
        print(json.dumps({"seconds": res, "said": said}))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5, help="calls of each function in a traced child")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the export arms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visible_orient_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--kernels-child", nargs=2, type=int, default=None, metavar=("B", "N"), help=argparse.SUPPRESS)
    ap.add_argument("--export-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.kernels_child[0], args.kernels_child[1], args.calls)
    if args.export_child:
        return export_child(args.rounds)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                             # (after every line: what was measured before a step failed stays)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(EXPECTATION)
    # (this process never touches the GPU: every measurement is a child's)
    say("tori, k = %d, 26 views at R = 64, one pooling round, rocprofv3 --kernel-trace --stats, %d calls of each function, us per launch "
        "(median, min .. max) [launches]:" % (K, args.calls))
    for b, n in SHAPES:
        rows, said = _trace([sys.executable, os.path.abspath(__file__), "--kernels-child", str(b), str(n), "--calls", str(args.calls)], ROOT)
        rec = json.loads([l for l in said.splitlines() if l.startswith("{")][0])
        say("  B = %d, N = %d  (flipped, undecided, unseen, dead over the batch: %s)" % (b, n, rec["stats"]))
        for name in sorted(rows):
            v = [1e3 * ms for ms in rows[name]]
            say("    %-44s %9.1f  (%.1f .. %.1f) [%d]" % (name[:44], statistics.median(v), min(v), max(v), len(v)))
    out = mc.step([sys.executable, os.path.abspath(__file__), "--export-child", "--rounds", str(args.rounds)], ROOT, 900)
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][0])
    for arm in ("consistent", "visible"):
        v = rec["seconds"][arm]
        say("export of %d clouds of 2048 points, --normals %d --orient %s: s per call mean %.3f min %.3f max %.3f over %d rounds, one process; %s"
            % (EXPORTED, K, arm, sum(v) / len(v), min(v), max(v), len(v), rec["said"][arm]))


if __name__ == "__main__":
    main()
