#!/usr/bin/env python3
"""What feeding from ragged clouds (data.RaggedFeeder) costs:
python3 tools/ragged_cost.py [--rounds R] [--iters K] [--parent DIR] [--out FILE] [--no-trace]   (FILE defaults to profiles/feed_ragged.txt)

  launches  200 launches of each feed kernel and nothing else in one child process under `rocprofv3 --kernel-trace --stats` (a run of
            its own), B = 35, 256 .. 2048 points: pdgn_feed_batch_ragged against pdgn_feed_batch_resample (feed_batch_kernel<true>) on ONE
            uniform set (512 shapes of 3000 points: the same points, as a stack and as a CloudSet), then pdgn_feed_batch_ragged on a set
            whose counts are spread over 500 .. 4000: the kernels' own times.
  fit       fit's inner loop (feeder.fill into the launch list's static buffers + step_list()) in FRESH child processes, K iterations
            each after 20 of warm-up, the arms alternating over R rounds (at least 4) on one box: with --parent DIR, a built checkout of
            the parent commit, the parent's code on equal-sized clouds of 2048 points; this tree on the same clouds; this tree on the
            ragged set.  Per arm: ms per iteration by device events, mean and spread over the rounds.
No number is fixed in advance: the yardstick is the parent arm and its own round-to-round spread -- a difference inside that spread is
"nothing visible", one outside it is reported with the numbers.  A report, not a gate.
Every GPU step is a child process under its own `timeout`; the tool stops at the first step that fails."""
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
B, N, M, SIZES, S = 35, 2048, 3000, (256, 512, 1024), 512
LO, HI = 500, 4000                                               # the ragged set's counts


def stack(points, dev):
    import torch
    g = torch.Generator().manual_seed(9999)
    c = torch.randn(S, points, 3, generator=g)
    return ((c - c.mean(dim=1, keepdim=True)) / c.reshape(S, -1).std(dim=1).view(S, 1, 1)).to(dev).contiguous()


def cloudset(kind, dev):
    """uniform: the shapes of stack(M) as a CloudSet; spread: S shapes of LO .. HI points (evenly spaced counts, shuffled)."""
    import numpy as np
    import torch
    from pdgn_amd.clouds import CloudSet
    if kind == "uniform":
        c = stack(M, "cpu")
        return CloudSet.from_arrays(c.reshape(-1, 3).numpy(), np.arange(S + 1, dtype=np.int64) * M).to(dev)
    rng = np.random.default_rng(9999)
    counts = rng.permutation(np.linspace(LO, HI, S).astype(np.int64))
    g = torch.Generator().manual_seed(9999)
    return CloudSet.from_clouds([torch.randn(int(m), 3, generator=g).numpy() for m in counts], normalize="shape_unit").to(dev)


def feeder_of(arm, dev):
    from pdgn_amd import data
    if arm == "resample":
        return data.BatchFeeder(stack(M, dev), B, SIZES, seed=9999, num_point=N)
    if arm in ("uniform", "spread", "ragged"):
        return data.RaggedFeeder(cloudset("spread" if arm == "ragged" else arm, dev), B, SIZES, seed=9999, num_point=N)
    return data.BatchFeeder(stack(N, dev), B, SIZES, seed=9999)


def kernels_child(launches, arm):
    """The child of a kernel trace: `launches` fills of one feeder."""
    import torch
    dev = torch.device("cuda:0")
    f = feeder_of(arm, dev)
    reals, z1, z2 = f.buffers()
    for i in range(launches):
        f.fill(1 + i // f.batches_per_epoch, i % f.batches_per_epoch, reals, z1, z2)
    torch.cuda.synchronize()


def step(cmd, cwd, limit):
    """One GPU step: a child under its own `timeout`; anything but a clean exit stops the tool."""
    run = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, capture_output=True, text=True)
    if run.returncode != 0:
        raise SystemExit("step failed (exit %d), stopping: %s\n%s" % (run.returncode, " ".join(cmd), run.stdout[-2000:] + run.stderr[-2000:]))
    return run.stdout


def traced(launches, arm):
    """(kernel name, launches, median us, min us, max us) of the feed kernel of one child under rocprofv3."""
    out = tempfile.mkdtemp(prefix="ragged_cost_trace_")
    try:
        step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
              "--kernels-child", arm, "--iters", str(launches)], ROOT, 300)
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        by = {}
        for r in csv.DictReader(open(path)):
            if "feed_batch" in r["Kernel_Name"]:
                by.setdefault(r["Kernel_Name"].split("(")[0], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        if len(by) != 1:
            raise SystemExit("trace of %s: expected one feed kernel, found %r" % (arm, sorted(by)))
        (name, v), = by.items()
        return name, len(v), statistics.median(v), min(v), max(v)
    finally:
        shutil.rmtree(out, ignore_errors=True)


def fit_child(arm, iters):
    """One arm of the fit loop in this process -> one JSON line.  arm: plain | ragged | parent (= plain, on whatever tree this file lies in)."""
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
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=60, help="iterations per fit child")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its fit loop on equal-sized clouds as a third arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_ragged.txt"), help="results file ('' for none)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 children")
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--fit-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.kernels_child:
        return kernels_child(args.iters, args.kernels_child)
    if args.fit_child:
        return fit_child(args.fit_child, args.iters)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # (this process never touches the GPU: every measurement is a child's)
    if not args.no_trace:
        say("feed kernels alone, B = %d, %d .. %d points, rocprofv3 --kernel-trace --stats, 200 launches each, one process per line:" % (B, SIZES[0], N))
        what = {"resample": "pdgn_feed_batch_resample, %d clouds of %d points" % (S, M),
                "uniform": "pdgn_feed_batch_ragged, the same clouds as a CloudSet",
                "spread": "pdgn_feed_batch_ragged, %d shapes of %d .. %d points" % (S, LO, HI)}
        med = {}
        for arm in ("resample", "uniform", "spread"):
            name, n, med[arm], lo, hi = traced(200, arm)
            say("  %-28s %4d launches, median %6.2f us, min %6.2f, max %6.2f   (%s)" % (name[:28], n, med[arm], lo, hi, what[arm]))
        say("  ragged - resample on the uniform set: %+.2f us; spread - uniform: %+.2f us" % (med["uniform"] - med["resample"], med["spread"] - med["uniform"]))
    arms = (["parent"] if args.parent else []) + ["plain", "ragged"]
    if args.parent:
        args.parent = os.path.abspath(args.parent)
        shutil.copy(os.path.abspath(__file__), os.path.join(args.parent, "tools", "ragged_cost.py"))
    res = {a: [] for a in arms}
    for r in range(args.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            cwd = args.parent if arm == "parent" else ROOT
            out = step([sys.executable, os.path.join(cwd, "tools", "ragged_cost.py"), "--fit-child", arm, "--iters", str(args.iters)], cwd, 300)
            line = [l for l in out.splitlines() if l.startswith("{")]
            if not line:
                raise SystemExit("fit child %s printed no result, stopping:\n%s" % (arm, out[-2000:]))
            rec = json.loads(line[0])
            if not rec["finite"]:
                raise SystemExit("fit child %s: a loss is not finite, stopping: %r" % (arm, rec))
            res[arm].append(rec["ms_per_iter"])
            print("round %d %-8s %.3f ms/iter" % (r, arm, rec["ms_per_iter"]), flush=True)
    names = {"parent": "parent commit, clouds of %d" % N, "plain": "this tree, clouds of %d" % N, "ragged": "this tree, ragged %d .. %d" % (LO, HI)}
    for arm in arms:
        v = res[arm]
        say("fit loop, %-30s ms/iter mean %.3f min %.3f max %.3f spread %.3f over %d rounds x %d iterations"
            % (names[arm], sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v), args.iters))
    mean = {a: sum(res[a]) / len(res[a]) for a in arms}
    spread = {a: max(res[a]) - min(res[a]) for a in arms}
    say("ragged - plain: %+.3f ms/iter" % (mean["ragged"] - mean["plain"]))
    if args.parent:
        say("plain - parent: %+.3f ms/iter; ragged - parent: %+.3f ms/iter; the parent arm's round-to-round spread: %.3f ms"
            % (mean["plain"] - mean["parent"], mean["ragged"] - mean["parent"], spread["parent"]))
        for arm in ("plain", "ragged"):
            d = mean[arm] - mean["parent"]
            say("%s arm against the parent arm: %s" % (arm, "nothing visible (inside the parent arm's spread)" if abs(d) <= spread["parent"]
                                                      else "%+.3f ms/iter, outside the parent arm's spread of %.3f" % (d, spread["parent"])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
