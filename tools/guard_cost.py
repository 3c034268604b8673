#!/usr/bin/env python3
"""What the gradient guard (PDGNTrainer(grad_guard=True)) costs: python3 tools/guard_cost.py [--rounds R]
[--block K] [--steps N] [--out FILE] [--no-trace]   (FILE defaults to profiles/guard_cost.txt)

  launches  the generator's optimizer step alone -- its 160 parameters with torch's Adam state and the average, random gradients,
            through trainer.LeanAdamStep -- in ONE child process under `rocprofv3 --kernel-trace --stats`, two optimizers side by side,
            one without and one with the guard, stepped alternately N times: per kernel (by name and grid) the median time, their
            sum per step for each arm.  (Back to back on an otherwise idle device; a wall clock does not resolve these launches.)
  A/B       two trainers from the same seed in THIS process, B = 35, 256 -> 2048 points, one without (a) and one with (b) the guard,
            each with its own launch list: blocks of K iterations of fit's inner loop (feeder.fill + step_list()), alternating, R
            rounds.  Per arm: ms per iteration, mean and block-to-block spread; (b) - (a) next to arm (a)'s spread; both lists' node
            counts (`_list.info`): the guard adds, per network, the norm launches, the finalising launch and one counter update."""
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
KERNELS = ("adam_multi_kernel", "adam_ema_multi_kernel", "adam_guard_multi_kernel", "adam_ema_guard_multi_kernel",
           "gradnorm_partial_kernel", "gradnorm_final_kernel")


def clouds(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(n, N, 3, generator=g)
    return ((c - c.mean(dim=1, keepdim=True)) / c.reshape(n, -1).std(dim=1).view(n, 1, 1)).to(dev).contiguous()


def optimizer_only(steps):
    """The child of the kernel trace: the generator's optimizer step alone, guard off and on, alternating."""
    from pdgn_amd.generator import PointGenerator
    from pdgn_amd.trainer import GradGuard, LeanAdamStep, PDGNTrainer
    dev = torch.device("cuda:0")
    arms = []
    for guarded in (False, True):
        torch.manual_seed(0)
        G = PointGenerator().to(dev)
        params = list(G.parameters())
        opt = torch.optim.Adam(params, lr=1e-4, betas=(0.5, 0.999), capturable=True, fused=True)
        avg = PDGNTrainer._flat_like(params)[1]
        with torch.no_grad():
            torch._foreach_copy_(avg, [p.detach() for p in params])
        lean = LeanAdamStep(opt, avg, 0.999, GradGuard(params) if guarded else None)
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        arms.append((lean, params))
    for _ in range(steps + 1):                                   # (the first one is the optimizer's own step)
        for lean, _p in arms:
            lean.step()
    torch.cuda.synchronize()
    assert all(lean.route == "own" for lean, _p in arms)
    assert arms[1][0].guard.state()["applied"] == steps + 1
    print("parameters %d in %d tensors" % (sum(p.numel() for p in arms[0][1]), len(arms[0][1])))


def traced(steps):
    """{(kernel, blocks): [us, ...]} of the optimizer's launches of the child under rocprofv3, and the parameter count."""
    out = tempfile.mkdtemp(prefix="guard_cost_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--steps", str(steps)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            raise RuntimeError("rocprofv3 child failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
        nparams = int(run.stdout.split("parameters ")[1].split()[0])
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        by = {}
        for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
            name = next((k for k in KERNELS if r["Kernel_Name"].split("(")[0].endswith(k)), None)
            if name is not None:
                by.setdefault((name, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])), []).append(
                    (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        return by, nparams
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--steps", type=int, default=60, help="optimizer steps per arm in the traced child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guard_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "guard_cost.py measures on the GPU"
    if args.child:
        return optimizer_only(args.steps)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- the launches (the child first: this process has not touched the GPU yet)
    if not args.no_trace:
        by, nparams = traced(args.steps)
        total = {False: 0.0, True: 0.0}
        for (name, blocks), us in sorted(by.items(), key=lambda kv: (kv[0][0], -kv[0][1])):
            us = us[min(5, len(us) // 2):]                       # (the first launches of a kernel: cold)
            guarded = "guard" in name or "gradnorm" in name
            total[guarded] += statistics.median(us)
            say("%-28s x %4d workgroups: median %6.2f us (min %.2f, max %.2f, %d launches)  [guard %s]"
                % (name, blocks, statistics.median(us), min(us), max(us), len(us), "on" if guarded else "off"))
        say("generator's optimizer step (%d parameters, with the average), sum of the launches' medians per step: guard off %.2f us, guard "
            "on %.2f us: %+.2f us (the gradients, %.1f MB, read once more: at least %.1f us at 8 TB/s; rocprofv3 --kernel-trace --stats, one "
            "process, the two arms stepped alternately %d times on an idle device; torch's counter update -- one multi-tensor add per "
            "step in both arms -- is not in these sums)" % (nparams, total[False], total[True], total[True] - total[False], nparams * 4 / 1e6,
                                                           nparams * 4 / 8e6, args.steps))

    # ---- A/B of fit's inner loop
    from pdgn_amd.data import BatchFeeder
    from pdgn_amd.trainer import PDGNTrainer
    dev = torch.device("cuda:0")
    feeder = BatchFeeder(clouds(S, 9999, dev), B, SIZES, seed=9999)
    nb = feeder.batches_per_epoch
    arms = {}
    for key, guard in (("a", False), ("b", True)):
        torch.manual_seed(0)
        tr = PDGNTrainer(device=dev, distributed=False, grad_guard=guard)
        tr.train()
        reals, z1, z2 = feeder.buffers()
        feeder.fill(1, 0, reals, z1, z2)
        tr.capture_list(reals, z1, z2)
        arms[key] = tr
        say("(%s) grad_guard=%s: launch list %s" % (key, guard, tr._list.info))
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
    state = arms["b"].guard_state()
    say("A/B: %d rounds x %d iterations per arm, alternating (the order within a round alternates too); losses finite: %s; arm (b)'s "
        "records: %s.  Both arms run fit's inner loop (feeder.fill into the list's static buffers + step_list()) in THIS process, on "
        "trainers built from the same seed; arm (a) is a trainer built without the argument -- the code path this change leaves alone -- "
        "not a separate build of the parent" % (args.rounds, args.block, finite,
                                                "; ".join("%s norm %.3g applied %d skipped %d" % (k, v["norm"], v["applied"], v["skipped"]) for k, v in state.items())))
    mean, spread = {}, {}
    for key, name in (("a", "no guard"), ("b", "grad_guard=True")):
        for j, clock in enumerate(("device events", "host clock")):
            v = [x[j] for x in res[key]]
            mean[key, j], spread[key, j] = sum(v) / len(v), max(v) - min(v)
            say("(%s) %-16s %-13s ms/iter mean %.3f min %.3f max %.3f spread %.3f" % (key, name, clock, mean[key, j], min(v), max(v), max(v) - min(v)))
    say("(b) - (a): %+.3f ms/iter by device events, %+.3f by the host clock; arm (a)'s block-to-block spread %.3f ms"
        % (mean["b", 0] - mean["a", 0], mean["b", 1] - mean["a", 1], spread["a", 0]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for tr in arms.values():
        tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
