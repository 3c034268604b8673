#!/usr/bin/env python3
"""What the averaged generator (PDGNTrainer(ema_decay=...)) costs: python3 tools/ema_cost.py [--rounds R]
[--block K] [--steps N] [--out FILE] [--no-trace]   (FILE defaults to profiles/ema_cost.txt)

  launches  the generator's optimizer step alone -- its 160 parameters with torch's Adam state, random gradients, N steps through
            trainer.LeanAdamStep -- once without and once with the list of averages, each in a child process of its own under
            `rocprofv3 --kernel-trace --stats`: per launch (by grid) the median kernel time, their sum per step, bytes moved per
            second.  (Back to back on an otherwise idle device: the launches of an iteration run behind a backward pass.)
  A/B       two trainers from the same seed in THIS process, B = 35, 256 -> 2048 points, one without (a) and one with (b) the average,
            each with its own launch list: blocks of K iterations of fit's inner loop (feeder.fill + step_list()), alternating, R
            rounds.  Per arm: ms per iteration, mean and block-to-block spread; (b) - (a) next to arm (a)'s spread.  Arm (a)'s code
            path is the one of a trainer built without the argument; both lists' node counts (`_list.info`) are printed -- the
            average adds no launch."""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, N, SIZES, S = 35, 2048, (256, 512, 1024), 4096


def clouds(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(n, N, 3, generator=g)
    return ((c - c.mean(dim=1, keepdim=True)) / c.reshape(n, -1).std(dim=1).view(n, 1, 1)).to(dev).contiguous()


def optimizer_only(ema, steps):
    """The child of the kernel trace: the generator's optimizer step alone."""
    from pdgn_amd.generator import PointGenerator
    from pdgn_amd.trainer import LeanAdamStep, PDGNTrainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    G = PointGenerator().to(dev)
    params = list(G.parameters())
    opt = torch.optim.Adam(params, lr=1e-4, betas=(0.5, 0.999), capturable=True, fused=True)
    avg = PDGNTrainer._flat_like(params)[1] if ema else None
    if avg is not None:
        with torch.no_grad():
            torch._foreach_copy_(avg, [p.detach() for p in params])
    lean = LeanAdamStep(opt, avg, 0.999 if ema else 0.0)
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    for _ in range(steps + 1):                                   # (the first one is the optimizer's own step)
        lean.step()
    torch.cuda.synchronize()
    assert lean.route == "own"
    print("parameters %d in %d tensors" % (sum(p.numel() for p in params), len(params)))


def traced(ema, steps):
    """{(kernel, blocks): [us, ...]} of the Adam launches of one child under rocprofv3, and the parameter count."""
    out = tempfile.mkdtemp(prefix="ema_cost_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--child", "on" if ema else "off", "--steps", str(steps)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            raise RuntimeError("rocprofv3 child failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
        nparams = int(run.stdout.split("parameters ")[1].split()[0])
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        rows = [r for r in csv.DictReader(open(path)) if "adam_" in r["Kernel_Name"] and "multi_kernel" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        by = {}
        for r in rows:
            name = "adam_ema_multi_kernel" if "adam_ema" in r["Kernel_Name"] else "adam_multi_kernel"
            by.setdefault((name, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])), []).append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        return by, nparams
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--steps", type=int, default=60, help="optimizer steps per traced child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 children")
    ap.add_argument("--child", choices=("on", "off"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ema_cost.py measures on the GPU"
    if args.child:
        return optimizer_only(args.child == "on", args.steps)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- the launches (children first: this process has not touched the GPU yet)
    if not args.no_trace:
        per_step = {}
        for ema in (False, True):
            by, nparams = traced(ema, args.steps)
            total = 0.0
            parts = []
            for (name, blocks), us in sorted(by.items(), key=lambda kv: -kv[0][1]):
                us = us[min(5, len(us) // 2):]                   # (the first launches of a kernel: cold)
                total += statistics.median(us)
                parts.append("%s x %d workgroups: median %.2f us (min %.2f, max %.2f, %d launches)"
                             % (name, blocks, statistics.median(us), min(us), max(us), len(us)))
            per_step[ema] = total
            nbytes = nparams * (36 if ema else 28)
            say("generator's optimizer step %s the average (%d parameters, %d B per parameter = %.1f MB): %s; sum of medians %.2f us per "
                "step = %.2f TB/s" % ("WITH" if ema else "without", nparams, 36 if ema else 28, nbytes / 1e6, "; ".join(parts), total,
                                     nbytes / total / 1e6))
        say("the average in the optimizer's launches: %+.2f us per step (the same number of launches, rocprofv3 --kernel-trace --stats, "
            "%d steps per arm back to back on an idle device)" % (per_step[True] - per_step[False], args.steps))

    # ---- A/B of fit's inner loop
    from pdgn_amd.data import BatchFeeder
    from pdgn_amd.trainer import PDGNTrainer
    dev = torch.device("cuda:0")
    feeder = BatchFeeder(clouds(S, 9999, dev), B, SIZES, seed=9999)
    nb = feeder.batches_per_epoch
    arms = {}
    for key, decay in (("a", 0.0), ("b", 0.999)):
        torch.manual_seed(0)
        tr = PDGNTrainer(device=dev, distributed=False, ema_decay=decay)
        tr.train()
        reals, z1, z2 = feeder.buffers()
        feeder.fill(1, 0, reals, z1, z2)
        tr.capture_list(reals, z1, z2)
        arms[key] = tr
        say("(%s) ema_decay=%g: launch list %s" % (key, decay, tr._list.info))
    same = arms["a"]._list.info == arms["b"]._list.info
    say("the two lists have the same node counts: %s" % same)
    count = {"a": 0, "b": 0}

    def block(key, k):
        tr = arms[key]
        st = tr._static
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(k):
            i = count[key]
            count[key] += 1
            feeder.fill(1 + i // nb, i % nb, st["reals"], st["z1"], st["z2"])
            tr.step_list()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k, (time.perf_counter() - t0) * 1e3 / k

    for key in ("a", "b"):
        block(key, 20)
    res = {"a": [], "b": []}
    for r in range(args.rounds):
        for key in (("a", "b") if r % 2 == 0 else ("b", "a")):
            res[key].append(block(key, args.block))
    finite = all(torch.isfinite(v).item() for tr in arms.values() for v in tr._static["out"].values())
    say("A/B: %d rounds x %d iterations per arm, alternating (the order within a round alternates too); losses finite: %s.  Both arms "
        "run fit's inner loop (feeder.fill into the list's static buffers + step_list()) in THIS process, on trainers built from the "
        "same seed; arm (a) is a trainer built without ema_decay -- the code path this change leaves alone -- not a separate build of "
        "the parent" % (args.rounds, args.block, finite))
    mean, spread = {}, {}
    for key, name in (("a", "no averaged generator"), ("b", "ema_decay=0.999")):
        for j, clock in enumerate(("device events", "host clock")):
            v = [x[j] for x in res[key]]
            mean[key, j], spread[key, j] = sum(v) / len(v), max(v) - min(v)
            say("(%s) %-24s %-13s ms/iter mean %.3f min %.3f max %.3f spread %.3f" % (key, name, clock, mean[key, j], min(v), max(v), max(v) - min(v)))
    diff = mean["b", 0] - mean["a", 0]
    say("(b) - (a): %+.3f ms/iter by device events, %+.3f by the host clock; arm (a)'s block-to-block spread %.3f ms: the difference is %s "
        "that spread + 0.1 ms" % (diff, mean["b", 1] - mean["a", 1], spread["a", 0], "within" if diff <= spread["a", 0] + 0.1 else "ABOVE"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for tr in arms.values():
        tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
