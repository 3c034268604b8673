#!/usr/bin/env python3
"""What the per-iteration N-point draw of the feeder (data.BatchFeeder(num_point=)) costs:
python3 tools/resample_cost.py [--rounds R] [--iters K] [--parent DIR] [--out FILE] [--no-trace]   (FILE defaults to profiles/feed_resample.txt)

  launches  200 launches of each feed kernel and nothing else in one child process under `rocprofv3 --kernel-trace --stats`, B = 35,
            256 .. 2048 points: pdgn_feed_batch on clouds of 2048 points against pdgn_feed_batch_resample on clouds of M = 15 000 points
            (pool = M): the kernels' own times.
  fit       fit's inner loop (feeder.fill into the launch list's static buffers + step_list()) in FRESH child processes, K iterations
            each after 20 of warm-up, the arms alternating over R rounds on one box: this tree on clouds of 2048 points (plain), on clouds
            of 15 000 points drawn to 2048 (resample), and -- with --parent DIR, a built checkout of the parent commit -- the parent's code
            on the plain loop.  Per arm: ms per iteration by device events, mean and spread over the rounds."""
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
B, N, M, SIZES, S = 35, 2048, 15000, (256, 512, 1024), 512


def clouds(points, dev):
    import torch
    g = torch.Generator().manual_seed(9999)
    c = torch.randn(S, points, 3, generator=g)
    return ((c - c.mean(dim=1, keepdim=True)) / c.reshape(S, -1).std(dim=1).view(S, 1, 1)).to(dev).contiguous()


def feeder_of(arm, dev):
    from pdgn_amd.data import BatchFeeder
    if arm == "resample":
        return BatchFeeder(clouds(M, dev), B, SIZES, seed=9999, num_point=N)
    return BatchFeeder(clouds(N, dev), B, SIZES, seed=9999)


def kernels_child(launches):
    """The child of the kernel trace: `launches` fills of each feeder."""
    import torch
    dev = torch.device("cuda:0")
    for arm in ("plain", "resample"):
        f = feeder_of(arm, dev)
        reals, z1, z2 = f.buffers()
        for i in range(launches):
            f.fill(1 + i // f.batches_per_epoch, i % f.batches_per_epoch, reals, z1, z2)
    torch.cuda.synchronize()


def traced(launches):
    """{kernel name: (launches, median us, min us, max us)} of the feed kernels of the child under rocprofv3."""
    out = tempfile.mkdtemp(prefix="resample_cost_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--kernels-child", "--iters", str(launches)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            raise RuntimeError("rocprofv3 child failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        by = {}
        for r in csv.DictReader(open(path)):
            if "feed_batch_kernel" in r["Kernel_Name"]:
                by.setdefault(r["Kernel_Name"].split("(")[0], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        return {k: (len(v), statistics.median(v), min(v), max(v)) for k, v in by.items()}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def fit_child(arm, iters):
    """One arm of the fit loop in this process -> one JSON line.  arm: plain | resample | parent (= plain, on whatever tree this file lies in)."""
    import torch
    from pdgn_amd.trainer import PDGNTrainer
    dev = torch.device("cuda:0")
    feeder = feeder_of(arm, dev)
    nb = feeder.batches_per_epoch
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
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
    print(json.dumps({"arm": arm, "ms_per_iter": ms, "finite": finite}))
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=60, help="iterations per fit child (launches per feeder of the traced child)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its fit loop as a third arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_resample.txt"), help="results file ('' for none)")
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
        say("feed kernels alone, B = %d, %d .. %d points, rocprofv3 --kernel-trace --stats, 200 launches each, one process:" % (B, SIZES[0], N))
        for k, (n, med, lo, hi) in sorted(traced(200).items()):
            say("  %-40s %4d launches, median %6.2f us, min %6.2f, max %6.2f" % (k[:40], n, med, lo, hi))
        say("  (<false>: pdgn_feed_batch, clouds of %d points; <true>: pdgn_feed_batch_resample, clouds of %d points, pool %d, drawn to %d)" % (N, M, M, N))
    arms = (["parent"] if args.parent else []) + ["plain", "resample"]
    if args.parent:
        args.parent = os.path.abspath(args.parent)
        shutil.copy(os.path.abspath(__file__), os.path.join(args.parent, "tools", "resample_cost.py"))
    res = {a: [] for a in arms}
    for r in range(args.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            cwd = args.parent if arm == "parent" else ROOT
            run = subprocess.run([sys.executable, os.path.join(cwd, "tools", "resample_cost.py"), "--fit-child", arm, "--iters", str(args.iters)],
                                 cwd=cwd, capture_output=True, text=True, timeout=600)
            line = [l for l in run.stdout.splitlines() if l.startswith("{")]
            if run.returncode != 0 or not line:
                raise RuntimeError("fit child %s failed:\n%s" % (arm, run.stdout[-2000:] + run.stderr[-2000:]))
            rec = json.loads(line[0])
            assert rec["finite"], rec
            res[arm].append(rec["ms_per_iter"])
            print("round %d %-8s %.3f ms/iter" % (r, arm, rec["ms_per_iter"]), flush=True)
    names = {"parent": "parent commit, clouds of %d" % N, "plain": "this tree, clouds of %d" % N, "resample": "this tree, %d drawn to %d" % (M, N)}
    for arm in arms:
        v = res[arm]
        say("fit loop, %-30s ms/iter mean %.3f min %.3f max %.3f spread %.3f over %d rounds x %d iterations"
            % (names[arm], sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v), args.iters))
    mean = {a: sum(res[a]) / len(res[a]) for a in arms}
    say("resample - plain: %+.3f ms/iter" % (mean["resample"] - mean["plain"]))
    if args.parent:
        say("plain - parent: %+.3f ms/iter; the parent's run-to-run spread %.3f ms" % (mean["plain"] - mean["parent"], max(res["parent"]) - min(res["parent"])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
