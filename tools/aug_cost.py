#!/usr/bin/env python3
"""What the discriminator augmentation (PDGNTrainer(augment=...)) costs: python3 tools/aug_cost.py [--rounds R]
[--iters K] [--parent DIR] [--out FILE] [--no-trace]   (FILE defaults to profiles/aug_cost.txt)

  launches  the four discriminators' chains alone -- D1..D4 forward and backward to the cloud at B = 35, 256 .. 2048 points, the
            generator's own pass through them -- in two child processes under `rocprofv3 --kernel-trace --stats`, augmentation off
            and on: launches per iteration, the summed kernel time per iteration, and the kernels that differ.
  fit       fit's inner loop (feeder.fill into the launch list's static buffers + step_list()) in FRESH child processes, K
            iterations each after 20 of warm-up, the arms alternating over R rounds on one box: this tree with augmentation off,
            with it on (the defaults at p = 0.5), and -- with --parent DIR, a built checkout of the parent commit (tools/ab_trees.sh
            says how to make one) -- the parent's code on the same loop.  Per arm: ms per iteration by device events, mean and
            spread over the rounds, and the launch list's node counts."""
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
B, N, SIZES, S = 35, 2048, (256, 512, 1024), 4096


def clouds(n, seed, dev):
    import torch
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(n, N, 3, generator=g)
    return ((c - c.mean(dim=1, keepdim=True)) / c.reshape(n, -1).std(dim=1).view(n, 1, 1)).to(dev).contiguous()


def chains_child(arm, iters):
    """The child of the kernel trace: D1..D4 forward + backward to the cloud, `iters` times."""
    import torch
    from pdgn_amd.generator import PointDiscriminator
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    Ds = [PointDiscriminator(i, 128 << i).to(dev).train() for i in (1, 2, 3, 4)]
    for d in Ds:
        for p in d.parameters():
            p.requires_grad_(False)                              # the generator's pass: frozen discriminators
    aug = None
    if arm == "on":
        from pdgn_amd.augment import Augment
        aug = Augment(p=0.5, device=dev)
    leaves = [torch.randn(B, 128 << i, 3, device=dev, requires_grad=True) for i in (1, 2, 3, 4)]
    xs = [l.transpose(1, 2) for l in leaves]                     # (B,3,N) views of point-major rows, as the generator's clouds are
    for _ in range(iters):
        if aug is not None:
            aug.tick()
        loss = sum((d(x) if aug is None else d(x, aug.at(i, "gen"))).sum() for i, (d, x) in enumerate(zip(Ds, xs)))
        torch.autograd.grad(loss, leaves)
    torch.cuda.synchronize()


def traced(arm, iters):
    """(launches per iteration, us per iteration, {kernel: (launches per iteration, median us)}) of the child under rocprofv3."""
    out = tempfile.mkdtemp(prefix="aug_cost_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--chains-child", arm, "--iters", str(iters)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            raise RuntimeError("rocprofv3 child failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        by, total_us, n = {}, 0.0, 0
        for r in csv.DictReader(open(path)):
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            by.setdefault(r["Kernel_Name"].split("(")[0].split("<")[0], []).append(us)
            total_us += us
            n += 1
        return n / iters, total_us / iters, {k: (len(v) / iters, statistics.median(v)) for k, v in by.items()}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def fit_child(arm, iters):
    """One arm of the fit loop in this process -> one JSON line.  arm: off | on | parent (= off, on whatever tree this file lies in)."""
    import torch
    from pdgn_amd.data import BatchFeeder
    from pdgn_amd.trainer import PDGNTrainer
    dev = torch.device("cuda:0")
    feeder = BatchFeeder(clouds(S, 9999, dev), B, SIZES, seed=9999)
    nb = feeder.batches_per_epoch
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False, **({"augment": {"p": 0.5, "seed": 9999}} if arm == "on" else {}))
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
    print(json.dumps({"arm": arm, "ms_per_iter": ms, "finite": finite, "list": tr._list.info}))
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=60, help="iterations per fit child (and of the traced chains)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its fit loop as a third arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aug_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 children")
    ap.add_argument("--chains-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--fit-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.chains_child:
        return chains_child(args.chains_child, args.iters)
    if args.fit_child:
        return fit_child(args.fit_child, args.iters)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- the discriminators' chains (this process never touches the GPU: every measurement is a child's)
    if not args.no_trace:
        got = {arm: traced(arm, 20) for arm in ("off", "on")}
        for arm in ("off", "on"):
            n, us, _ = got[arm]
            say("D1..D4 forward + backward to the cloud, B = %d, augmentation %-3s: %.1f launches per iteration, %.1f us of kernel time per "
                "iteration (rocprofv3 --kernel-trace --stats, 20 iterations, one process)" % (B, arm, n, us))
        off, on = got["off"][2], got["on"][2]
        for k in sorted(set(off) | set(on)):
            a, b = off.get(k, (0.0, 0.0)), on.get(k, (0.0, 0.0))
            if abs(a[0] - b[0]) > 1e-9:
                say("  %-60s off: %4.1f per iteration, median %6.2f us | on: %4.1f per iteration, median %6.2f us" % (k[:60], a[0], a[1], b[0], b[1]))
        say("launches per iteration: on - off = %+.1f (the tick, and per discriminator one augment_rows_fwd and one _bwd: a generated cloud is a "
            "(B,3,N) view of point-major rows, for which torch's transpose + reshape is a view and launches nothing)" % (got["on"][0] - got["off"][0]))

    # ---- fit's loop, arms alternating in fresh processes
    arms = (["parent"] if args.parent else []) + ["off", "on"]
    if args.parent:
        args.parent = os.path.abspath(args.parent)
        shutil.copy(os.path.abspath(__file__), os.path.join(args.parent, "tools", "aug_cost.py"))
    res, info = {a: [] for a in arms}, {}
    for r in range(args.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            cwd = args.parent if arm == "parent" else ROOT
            run = subprocess.run([sys.executable, os.path.join(cwd, "tools", "aug_cost.py"), "--fit-child", arm, "--iters", str(args.iters)],
                                 cwd=cwd, capture_output=True, text=True, timeout=600)
            line = [l for l in run.stdout.splitlines() if l.startswith("{")]
            if run.returncode != 0 or not line:
                raise RuntimeError("fit child %s failed:\n%s" % (arm, run.stdout[-2000:] + run.stderr[-2000:]))
            rec = json.loads(line[0])
            assert rec["finite"], rec
            res[arm].append(rec["ms_per_iter"])
            info[arm] = rec["list"]
            print("round %d %-6s %.3f ms/iter" % (r, arm, rec["ms_per_iter"]), flush=True)
    names = {"parent": "parent commit", "off": "this tree, augment=None", "on": "this tree, augment p=0.5"}
    for arm in arms:
        v = res[arm]
        say("fit loop, %-26s ms/iter mean %.3f min %.3f max %.3f spread %.3f over %d rounds x %d iterations; launch list %s"
            % (names[arm], sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v), args.iters, info[arm]))
    mean = {a: sum(res[a]) / len(res[a]) for a in arms}
    say("on - off: %+.3f ms/iter, %+d list nodes (%+d kernels)" % (mean["on"] - mean["off"], info["on"]["nodes"] - info["off"]["nodes"],
                                                                  info["on"]["kernels"] - info["off"]["kernels"]))
    if args.parent:
        say("off - parent: %+.3f ms/iter, %+d list nodes; the parent's run-to-run spread %.3f ms" % (mean["off"] - mean["parent"],
                                                                                                  info["off"]["nodes"] - info["parent"]["nodes"],
                                                                                                  max(res["parent"]) - min(res["parent"])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
