#!/usr/bin/env python3
"""What the flatness regulariser (PDGNTrainer(flatness=...)) costs:
python3 tools/flatness_cost.py [--rounds R] [--iters K] [--parent DIR] [--out FILE] [--no-trace]   (FILE defaults to profiles/flatness_cost.txt)

  kernels   20 rounds of pointops.knnquery, pointops.estimate_normals and losses.flatness (forward and backward, on the same lists) at each
            of the four level shapes of B = 35, k = 16 (256, 512, 1024, 2048 points) and nothing else in one child process under
            `rocprofv3 --kernel-trace --stats` (no counters): the per-point kernel's, the transposition's launches', the gather's, the
            reduction's and the backward scale's own times beside the normals kernel's and the neighbour search's, per shape, and the two
            yardsticks: per-point kernel / normals kernel, transposition / neighbour search.  The clouds are noisy unit spheres.
  fit       fit's inner loop (feeder.fill into the launch list's static buffers + step_list()) in FRESH child processes, K iterations
            each after 20 of warm-up, the arms alternating over R rounds on one box: this tree without the term, with it (weight 0.05,
            all four levels, k = 16, the floor calibrated from the feeder as the command line does), and -- with --parent DIR, a built
            checkout of the parent commit -- the parent's code on its loop.  Per arm: ms per iteration by device events, mean and
            spread over the rounds, and the launch list's node and kernel counts.
Every child runs under its own `timeout -k 10`; the first one that fails ends the run."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, SIZES, S, K = 35, 2048, (256, 512, 1024), 512, 16
LEVELS = (256, 512, 1024, 2048)
EPS = 1e-5
# the kernels of one round, by a substring of their names, in the order of the report
KERNELS = (("knn3_", "pdgn_knnquery"), ("normals_kernel", "pdgn_estimate_normals"), ("flat_point_kernel", "per-point kernel"),
           ("repulsion_reduce_kernel", "reduction"), ("flat_transpose_kernel", "transposition: workgroup"),
           ("det_count_kernel", "transposition: count"), ("det_scan_fill_kernel", "transposition: scan + fill"),
           ("flat_gather_kernel", "gather"), ("repulsion_bwd_kernel", "backward scale"))


def clouds(count, points, dev):
    import torch
    g = torch.Generator().manual_seed(9999)
    c = torch.randn(count, points, 3, generator=g)
    return ((c - c.mean(dim=1, keepdim=True)) / c.reshape(count, -1).std(dim=1).view(count, 1, 1)).to(dev).contiguous()


def kernels_child(launches):
    """The child of the kernel trace: per level shape, `launches` rounds of the neighbour search, the normals and the op."""
    import torch
    from pdgn_amd import losses, pointops
    dev = torch.device("cuda:0")
    for n in LEVELS:
        g = torch.Generator(device=dev).manual_seed(n)
        v = torch.randn(B, n, 3, device=dev, generator=g)
        x = (v / v.norm(dim=2, keepdim=True) * (1.0 + 0.05 * torch.randn(B, n, 1, device=dev, generator=g))).contiguous().requires_grad_(True)
        for _ in range(launches):
            x.grad = None
            with torch.no_grad():
                idx = pointops.knnquery(K, x.detach(), x.detach())
                pointops.estimate_normals(x.detach(), idx=idx, return_eig=True)
            loss = losses.flatness(x, idx=idx, eps=EPS)
            loss.backward()
        torch.cuda.synchronize()
        print(json.dumps({"n": n, "loss": loss.item(), "finite": bool(torch.isfinite(x.grad).all().item())}))


def traced(launches):
    """([the child's JSON lines], {label: [(us, full name) per launch, in issue order]}) of the child under rocprofv3."""
    out = tempfile.mkdtemp(prefix="flatness_cost_trace_")
    try:
        cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.abspath(__file__), "--kernels-child", "--iters", str(launches)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if run.returncode != 0:
            raise RuntimeError("rocprofv3 child failed (%d):\n%s" % (run.returncode, run.stdout[-2000:] + run.stderr[-2000:]))
        checks = [json.loads(l) for l in run.stdout.splitlines() if l.startswith("{")]
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        by = {}
        for r in rows:
            name = r["Kernel_Name"].split("(")[0]
            for part, label in KERNELS:
                if part in name:
                    by.setdefault(label, []).append(((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, name))
        return checks, by
    finally:
        shutil.rmtree(out, ignore_errors=True)


def fit_child(arm, iters):
    """One arm of the fit loop in this process -> one JSON line.  arm: off | on | parent (= off, on whatever tree this file lies in)."""
    import torch
    from pdgn_amd.data import BatchFeeder
    from pdgn_amd.trainer import PDGNTrainer
    dev = torch.device("cuda:0")
    feeder = BatchFeeder(clouds(S, N, dev), B, SIZES, seed=9999)
    nb = feeder.batches_per_epoch
    kw, eps = {}, None
    if arm == "on":
        from pdgn_amd.train import calibrate_flatness_eps
        eps, _ = calibrate_flatness_eps(feeder, K)
        kw = {"flatness": {"weight": 0.05, "k": K, "eps": eps}}
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False, **kw)
    tr.train()
    reals, z1, z2 = feeder.buffers()
    feeder.fill(1, 0, reals, z1, z2)
    tr.capture_list(reals, z1, z2)
    st = tr._static

    def block(first, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(first, first + k):
            feeder.fill(1 + i // nb, i % nb, st["reals"], st["z1"], st["z2"])
            tr.step_list()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k

    block(0, 20)
    ms = block(20, iters)
    finite = all(torch.isfinite(v).item() for v in st["out"].values())
    info = tr._list.info
    rec = {"arm": arm, "ms_per_iter": ms, "finite": finite, "nodes": info["nodes"], "kernels": info["kernels"], "eps": eps}
    if arm == "on":
        state = tr.flatness_state()
        rec["state"], rec["degenerate"] = state["per_level"], state["degenerate"]
    print(json.dumps(rec))
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=60, help="iterations per fit child")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its fit loop as a third arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flatness_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--fit-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.kernels_child:
        return kernels_child(args.iters)
    if args.fit_child:
        return fit_child(args.fit_child, args.iters)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # (this process never touches the GPU: every measurement is a child's)
    if not args.no_trace:
        launches = 20
        checks, by = traced(launches)
        say("(a) rocprofv3 --kernel-trace --stats, %d rounds of knnquery + estimate_normals + flatness forward and backward per level shape of B = %d, "
            "k = %d, one process; noisy unit spheres, eps %g; medians in us:" % (launches, B, K, EPS))
        med = {}
        for _, label in KERNELS:
            v = by.get(label, [])
            per = len(v) // len(LEVELS)                            # issue order: the four shapes one after the other
            for i, n in enumerate(LEVELS):
                g = [us for us, _ in v[i * per:(i + 1) * per]]
                if not g:
                    continue
                med[(label, n)] = statistics.median(g) * (per // launches)      # (a label with several launches per round: their sum)
                say("  %-28s n = %4d: %3d launches, median %8.2f us, min %8.2f, max %8.2f   (%s)"
                    % (label, n, len(g), statistics.median(g), min(g), max(g), v[i * per][1][:40]))
        for n in LEVELS:
            point, normals = med.get(("per-point kernel", n)), med.get(("pdgn_estimate_normals", n))
            trans = sum(med.get((label, n), 0.0) for label in ("transposition: workgroup", "transposition: count", "transposition: scan + fill"))
            knn = med.get(("pdgn_knnquery", n))
            if point and normals and knn:
                say("  n = %4d: per-point / normals = %.2f; transposition %.1f us against the neighbour search's %.1f us (%.2f); gather %.1f us"
                    % (n, point / normals, trans, knn, trans / knn, med.get(("gather", n), float("nan"))))
        for c in checks:
            say("  n = %4d: loss %.6g, gradient %s" % (c["n"], c["loss"], "finite" if c["finite"] else "NOT FINITE"))
    arms = (["parent"] if args.parent else []) + ["off", "on"]
    if args.parent:
        args.parent = os.path.abspath(args.parent)
        shutil.copy(os.path.abspath(__file__), os.path.join(args.parent, "tools", "flatness_cost.py"))
    res, recs = {a: [] for a in arms}, {}
    for r in range(args.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            cwd = args.parent if arm == "parent" else ROOT
            run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(cwd, "tools", "flatness_cost.py"), "--fit-child", arm,
                                  "--iters", str(args.iters)], cwd=cwd, capture_output=True, text=True)
            line = [l for l in run.stdout.splitlines() if l.startswith("{")]
            if run.returncode != 0 or not line:
                raise RuntimeError("fit child %s failed (%d):\n%s" % (arm, run.returncode, run.stdout[-2000:] + run.stderr[-2000:]))
            rec = json.loads(line[0])
            assert rec["finite"], rec
            res[arm].append(rec["ms_per_iter"])
            recs[arm] = rec
            print("round %d %-8s %.3f ms/iter" % (r, arm, rec["ms_per_iter"]), flush=True)
    names = {"parent": "parent commit", "off": "this tree, no flatness", "on": "this tree, flatness 0.05 on 4 levels"}
    say("(b) fit's loop, B = %d, clouds of %d points, sizes %s:" % (B, N, SIZES))
    for arm in arms:
        v = res[arm]
        say("  %-38s ms/iter mean %.3f min %.3f max %.3f spread %.3f over %d rounds x %d iterations; list: %d nodes, %d kernels"
            % (names[arm], sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v), args.iters, recs[arm]["nodes"], recs[arm]["kernels"]))
    mean = {a: sum(res[a]) / len(res[a]) for a in arms}
    say("  on - off: %+.3f ms/iter; calibrated eps %.6g; last iteration's value per level %s, %d degenerate points"
        % (mean["on"] - mean["off"], recs["on"]["eps"], ", ".join("%.4g" % v for v in recs["on"]["state"]), recs["on"]["degenerate"]))
    if args.parent:
        say("  off - parent: %+.3f ms/iter; the parent's run-to-run spread %.3f ms; list counts %s"
            % (mean["off"] - mean["parent"], max(res["parent"]) - min(res["parent"]),
               "equal" if (recs["off"]["nodes"], recs["off"]["kernels"]) == (recs["parent"]["nodes"], recs["parent"]["kernels"]) else "DIFFERENT"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
