#!/usr/bin/env python3
"""What the farthest-point pyramid of the feeder (data.BatchFeeder(subsample="fps")) costs:
python3 tools/fps_cost.py [--rounds R] [--iters K] [--parent DIR] [--out FILE] [--no-trace]   (FILE defaults to profiles/fps_feed.txt)

  kernels   20 launches of pdgn_fps_order (csrc/fps.hip) and of pdgn_furthestsampling (csrc/pointops_extra.hip) on the same clouds at
            b = 35, n = 2048, m = 1024 and b = 35, n = 4096, m = 2048, and 20 fills of the "fps" feeder at B = 35, 256 .. 2048 points,
            and nothing else in one child process under `rocprofv3 --kernel-trace --stats`: the kernels' own times.  The child also
            checks that the two kernels return the same indices at both shapes.
  fit       fit's inner loop (feeder.fill into the launch list's static buffers + step_list()) in FRESH child processes, K iterations
            each after 20 of warm-up, the arms alternating over R rounds on one box: this tree with subsample="random", with
            subsample="fps", and -- with --parent DIR, a built checkout of the parent commit -- the parent's code on its (random)
            loop.  Per arm: ms per iteration by device events, mean and spread over the rounds."""
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
B, N, SIZES, S = 35, 2048, (256, 512, 1024), 512
SHAPES = ((35, 2048, 1024), (35, 4096, 2048))


def clouds(count, points, dev):
    import torch
    g = torch.Generator().manual_seed(9999)
    c = torch.randn(count, points, 3, generator=g)
    return ((c - c.mean(dim=1, keepdim=True)) / c.reshape(count, -1).std(dim=1).view(count, 1, 1)).to(dev).contiguous()


def feeder_of(arm, dev):
    from pdgn_amd.data import BatchFeeder
    if arm == "fps":
        return BatchFeeder(clouds(S, N, dev), B, SIZES, seed=9999, subsample="fps")
    return BatchFeeder(clouds(S, N, dev), B, SIZES, seed=9999)     # (random, parent: the call the parent commit knows)


def kernels_child(launches):
    """The child of the kernel trace: `launches` calls of each sampler at each shape, then `launches` fills of the "fps" feeder."""
    import torch
    from pdgn_amd import pointops
    dev = torch.device("cuda:0")
    for b, n, m in SHAPES:
        xyz = clouds(b, n, dev)
        for _ in range(launches):
            old = pointops.furthestsampling(xyz, m)
            new = pointops.fps_order(xyz, m)
        torch.cuda.synchronize()
        print(json.dumps({"shape": [b, n, m], "equal": bool(torch.equal(old, new))}))
    f = feeder_of("fps", dev)
    reals, z1, z2 = f.buffers()
    for i in range(launches):
        f.fill(1 + i // f.batches_per_epoch, i % f.batches_per_epoch, reals, z1, z2)
    torch.cuda.synchronize()


def traced(launches):
    """([the child's JSON lines], {kernel name: [us per launch, in issue order]}) of the child under rocprofv3: in issue order, so that
    the two shapes of one kernel name can be told apart by position."""
    out = tempfile.mkdtemp(prefix="fps_cost_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--kernels-child", "--iters", str(launches)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            raise RuntimeError("rocprofv3 child failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
        checks = [json.loads(l) for l in run.stdout.splitlines() if l.startswith("{")]
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        by = {}
        for r in rows:
            name = r["Kernel_Name"].split("(")[0]
            if "fps_reg_kernel" in name or "fps_kernel" in name:
                by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        return checks, by
    finally:
        shutil.rmtree(out, ignore_errors=True)


def fit_child(arm, iters):
    """One arm of the fit loop in this process -> one JSON line.  arm: random | fps | parent (= random, on whatever tree this file lies in)."""
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
    ap.add_argument("--iters", type=int, default=60, help="iterations per fit child")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its fit loop as a third arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps_feed.txt"), help="results file ('' for none)")
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
        say("(a) the samplers alone, rocprofv3 --kernel-trace --stats, %d launches per kernel and shape, one process, the two kernels alternating:" % launches)
        for name, v in sorted(by.items()):
            # issue order: shape 0's launches, then shape 1's, then (fps_reg_kernel<.., true> only) the feeder's
            groups = [v[k:k + launches] for k in range(0, len(v), launches)]
            for g in groups:
                say("  %-44s %3d launches, median %9.2f us, min %9.2f, max %9.2f" % (name[:44], len(g), statistics.median(g), min(g), max(g)))
        say("  fps_kernel: pdgn_furthestsampling; fps_reg_kernel<PPT, false>: pdgn_fps_order (PPT 4: b, n, m = %d, %d, %d; PPT 8: %d, %d, %d);"
            % (SHAPES[0] + SHAPES[1]))
        say("  fps_kernel's two lines: those two shapes in that order; fps_reg_kernel<4, true>: pdgn_feed_fps_pyramid, B = %d, N = %d, sizes %s" % (B, N, SIZES))
        for c in checks:
            say("  indices of the two kernels at b, n, m = %s: %s" % (tuple(c["shape"]), "equal" if c["equal"] else "DIFFERENT"))
    arms = (["parent"] if args.parent else []) + ["random", "fps"]
    if args.parent:
        args.parent = os.path.abspath(args.parent)
        shutil.copy(os.path.abspath(__file__), os.path.join(args.parent, "tools", "fps_cost.py"))
    res = {a: [] for a in arms}
    for r in range(args.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            cwd = args.parent if arm == "parent" else ROOT
            run = subprocess.run([sys.executable, os.path.join(cwd, "tools", "fps_cost.py"), "--fit-child", arm, "--iters", str(args.iters)],
                                 cwd=cwd, capture_output=True, text=True, timeout=600)
            line = [l for l in run.stdout.splitlines() if l.startswith("{")]
            if run.returncode != 0 or not line:
                raise RuntimeError("fit child %s failed:\n%s" % (arm, run.stdout[-2000:] + run.stderr[-2000:]))
            rec = json.loads(line[0])
            assert rec["finite"], rec
            res[arm].append(rec["ms_per_iter"])
            print("round %d %-8s %.3f ms/iter" % (r, arm, rec["ms_per_iter"]), flush=True)
    names = {"parent": "parent commit", "random": 'this tree, subsample="random"', "fps": 'this tree, subsample="fps"'}
    say("(b) fit's loop, B = %d, clouds of %d points, sizes %s:" % (B, N, SIZES))
    for arm in arms:
        v = res[arm]
        say("  %-30s ms/iter mean %.3f min %.3f max %.3f spread %.3f over %d rounds x %d iterations"
            % (names[arm], sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v), args.iters))
    mean = {a: sum(res[a]) / len(res[a]) for a in arms}
    say("  fps - random: %+.3f ms/iter" % (mean["fps"] - mean["random"]))
    if args.parent:
        say("  random - parent: %+.3f ms/iter; the parent's run-to-run spread %.3f ms" % (mean["random"] - mean["parent"], max(res["parent"]) - min(res["parent"])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
