#!/usr/bin/env python3
"""What the adaptive discriminator augmentation (PDGNTrainer(augment={..., "adaptive": {...}})) costs:
python3 tools/ada_cost.py [--rounds R] [--iters K] [--parent DIR] [--out FILE] [--no-trace]   (FILE defaults to profiles/ada_cost.txt)

  launches  the launches the feature touches, alone -- the tick and the four real-batch loss terms on B = 35 scores -- in two child
            processes under `rocprofv3 --kernel-trace --stats`, fixed p and adaptive: launches per iteration and the kernels' times.
  fit       fit's inner loop (feeder.fill into the launch list's static buffers + step_list()) in FRESH child processes, K
            iterations each after 20 of warm-up, the arms alternating over R rounds on one box: this tree at a fixed p = 0.5
            (adaptive=None), this tree adaptive from p = 0.5 (the defaults), and -- with --parent DIR, a built checkout of the parent
            commit (tools/ab_trees.sh says how to make one) -- the parent's fixed-p run on the same loop.  Per arm: ms per iteration
            by device events, median and spread over the rounds, and the launch list's node counts.
Two expectations are judged: (a) fixed p in this tree is the parent's run -- the same list, a time inside the parent's own spread;
(b) adaptive adds no launch and no time beyond that spread."""
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


def terms_child(arm, iters):
    """The child of the kernel trace: the tick and the four real-batch terms (forward only), `iters` times."""
    import torch
    from pdgn_amd import losses
    from pdgn_amd.augment import Augment
    dev = torch.device("cuda:0")
    aug = Augment(p=0.5, device=dev, **({"adaptive": {}} if arm == "ada" else {}))
    scores = [torch.rand(B, 1, device=dev) for _ in range(4)]
    for _ in range(iters):
        aug.tick()
        for i, s in enumerate(scores):
            if arm == "ada":
                losses.mse_const(s, 1.0, 0.5, count=aug.counter(i))
            else:
                losses.mse_const(s, 1.0, 0.5)
    torch.cuda.synchronize()


def traced(arm, iters):
    """(launches per iteration, us per iteration, {kernel: (launches per iteration, median us)}) of the child under rocprofv3."""
    out = tempfile.mkdtemp(prefix="ada_cost_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--terms-child", arm, "--iters", str(iters)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            raise RuntimeError("rocprofv3 child failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        by, total_us, n = {}, 0.0, 0
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"].split("(")[0].split("<")[0]
            if "tick" not in name and "mse_const" not in name:   # (torch.rand's fill: not the feature's)
                continue
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            by.setdefault(name, []).append(us)
            total_us += us
            n += 1
        return n / iters, total_us / iters, {k: (len(v) / iters, statistics.median(v)) for k, v in by.items()}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def fit_child(arm, iters):
    """One arm of the fit loop in this process -> one JSON line.  arm: fixed | ada | parent (= fixed, on whatever tree this file lies in)."""
    import torch
    from pdgn_amd.data import BatchFeeder
    from pdgn_amd.trainer import PDGNTrainer
    dev = torch.device("cuda:0")
    feeder = BatchFeeder(clouds(S, 9999, dev), B, SIZES, seed=9999)
    nb = feeder.batches_per_epoch
    torch.manual_seed(0)
    augment = {"p": 0.5, "seed": 9999}
    if arm == "ada":
        augment["adaptive"] = {}
    tr = PDGNTrainer(device=dev, distributed=False, augment=augment)
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
    rec = {"arm": arm, "ms_per_iter": ms, "finite": finite, "list": tr._list.info}
    if arm == "ada":
        a = tr.aug_state()["ada"]
        rec["ada"] = {"p": a["p"], "updates": a["updates"], "last_r": a["last_r"]}
    print(json.dumps(rec))
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=60, help="iterations per fit child (and of the traced terms)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its fixed-p fit loop as a third arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ada_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 children")
    ap.add_argument("--terms-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--fit-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.terms_child:
        return terms_child(args.terms_child, args.iters)
    if args.fit_child:
        return fit_child(args.fit_child, args.iters)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- the launches the feature touches (this process never touches the GPU: every measurement is a child's)
    if not args.no_trace:
        got = {arm: traced(arm, 50) for arm in ("fixed", "ada")}
        for arm in ("fixed", "ada"):
            n, us, by = got[arm]
            say("tick + four real-batch terms, B = %d, %-5s: %.1f launches per iteration, %.2f us of kernel time per iteration "
                "(rocprofv3 --kernel-trace --stats, 50 iterations, one process)" % (B, arm, n, us))
            for k in sorted(by):
                say("  %-60s %4.1f per iteration, median %6.2f us" % (k[:60], by[k][0], by[k][1]))
        say("launches per iteration: ada - fixed = %+.1f; kernel time %+.2f us per iteration" % (got["ada"][0] - got["fixed"][0],
                                                                                             got["ada"][1] - got["fixed"][1]))

    # ---- fit's loop, arms alternating in fresh processes
    arms = (["parent"] if args.parent else []) + ["fixed", "ada"]
    if args.parent:
        args.parent = os.path.abspath(args.parent)
        shutil.copy(os.path.abspath(__file__), os.path.join(args.parent, "tools", "ada_cost.py"))
    res, info, last = {a: [] for a in arms}, {}, {}
    for r in range(args.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            cwd = args.parent if arm == "parent" else ROOT
            run = subprocess.run([sys.executable, os.path.join(cwd, "tools", "ada_cost.py"), "--fit-child", arm, "--iters", str(args.iters)],
                                 cwd=cwd, capture_output=True, text=True, timeout=600)
            line = [l for l in run.stdout.splitlines() if l.startswith("{")]
            if run.returncode != 0 or not line:
                raise RuntimeError("fit child %s failed:\n%s" % (arm, run.stdout[-2000:] + run.stderr[-2000:]))
            rec = json.loads(line[0])
            assert rec["finite"], rec
            res[arm].append(rec["ms_per_iter"])
            info[arm], last[arm] = rec["list"], rec
            print("round %d %-6s %.3f ms/iter" % (r, arm, rec["ms_per_iter"]), flush=True)
    names = {"parent": "parent commit, fixed p=0.5", "fixed": "this tree, fixed p=0.5", "ada": "this tree, adaptive"}
    med = {a: statistics.median(res[a]) for a in arms}
    spread = {a: max(res[a]) - min(res[a]) for a in arms}
    for arm in arms:
        v = res[arm]
        say("fit loop, %-27s ms/iter median %.3f min %.3f max %.3f spread %.3f over %d rounds x %d iterations; launch list %s"
            % (names[arm], med[arm], min(v), max(v), spread[arm], len(v), args.iters, info[arm]))
    say("adaptive after its run: %s" % (last["ada"]["ada"],))
    ref = "parent" if args.parent else "fixed"
    d_nodes, d_kernels = info["ada"]["nodes"] - info["fixed"]["nodes"], info["ada"]["kernels"] - info["fixed"]["kernels"]
    d_ms = med["ada"] - med["fixed"]
    say("ada - fixed: %+.3f ms/iter (medians), %+d list nodes (%+d kernels); the %s arm's run-to-run spread %.3f ms"
        % (d_ms, d_nodes, d_kernels, ref, spread[ref]))
    say("expectation (b), adaptive adds no launch and no time beyond that spread: %s"
        % ("CONFIRMED" if d_nodes == 0 and d_kernels == 0 and d_ms <= spread[ref] else "REFUTED"))
    if args.parent:
        a_nodes, a_ms = info["fixed"]["nodes"] - info["parent"]["nodes"], med["fixed"] - med["parent"]
        say("fixed - parent: %+.3f ms/iter (medians), %+d list nodes (%+d kernels); the parent's run-to-run spread %.3f ms"
            % (a_ms, a_nodes, info["fixed"]["kernels"] - info["parent"]["kernels"], spread["parent"]))
        say("expectation (a), adaptive=None is the parent's fixed-p run (same list, time inside the parent's spread): %s"
            % ("CONFIRMED" if a_nodes == 0 and info["fixed"]["kernels"] == info["parent"]["kernels"] and abs(a_ms) <= spread["parent"] else "REFUTED"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
