#!/usr/bin/env python3
"""What feeding from triangle meshes (data.MeshFeeder) costs:
python3 tools/mesh_cost.py [--rounds R] [--iters K] [--parent DIR] [--out FILE] [--no-trace]   (FILE defaults to profiles/feed_mesh.txt)

  launches  200 launches of each feed kernel and nothing else in one child process under `rocprofv3 --kernel-trace --stats`, B = 35,
            256 .. 2048 points: pdgn_feed_batch_mesh on meshes of a few thousand faces against pdgn_feed_batch_resample on clouds of
            M = 15 000 points (feed_batch_kernel<true>): the kernels' own times.
  fit       fit's inner loop (feeder.fill into the launch list's static buffers + step_list()) in FRESH child processes, K iterations
            each after 20 of warm-up, the arms alternating over R rounds (at least 4) on one box: with --parent DIR, a built checkout of
            the parent commit, the parent's code on clouds of 2048 points; this tree on the same clouds; this tree on meshes.  Per arm: ms
            per iteration by device events, mean and spread over the rounds.  The mesh arm passes if it is within one arm's own
            run-to-run spread of the parent arm.
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
B, N, M, SIZES, S = 35, 2048, 15000, (256, 512, 1024), 512
GRID = 48                                                        # a mesh: a GRID x GRID height field, 2 GRID^2 = 4608 faces


def clouds(points, dev):
    import torch
    g = torch.Generator().manual_seed(9999)
    c = torch.randn(S, points, 3, generator=g)
    return ((c - c.mean(dim=1, keepdim=True)) / c.reshape(S, -1).std(dim=1).view(S, 1, 1)).to(dev).contiguous()


def meshes(dev):
    """S bumpy height fields of 4608 faces each, normalised over their surfaces (21 MB of vertices and faces, 19 MB of alias records)."""
    import numpy as np
    from pdgn_amd.meshes import MeshSet
    rng = np.random.default_rng(9999)
    i, j = np.meshgrid(np.arange(GRID), np.arange(GRID), indexing="ij")
    at = lambda a, b: (a * (GRID + 1) + b).reshape(-1)
    faces = np.concatenate([np.stack([at(i, j), at(i + 1, j), at(i, j + 1)], 1), np.stack([at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)], 1)])
    x, y = np.meshgrid(np.linspace(-1, 1, GRID + 1), np.linspace(-1, 1, GRID + 1), indexing="ij")
    shapes = []
    for _ in range(S):
        a, b, c = rng.uniform(0.5, 4.0, 3)
        shapes.append((np.stack([x, np.sin(a * x) * np.cos(b * y) + 0.1 * c * x * y, y], 2).reshape(-1, 3).astype(np.float32), faces.astype(np.int32)))
    return MeshSet.from_meshes(shapes, normalize="shape_unit").to(dev)


def feeder_of(arm, dev):
    from pdgn_amd import data
    if arm == "mesh":
        return data.MeshFeeder(meshes(dev), B, SIZES, seed=9999, num_point=N)
    if arm == "resample":
        return data.BatchFeeder(clouds(M, dev), B, SIZES, seed=9999, num_point=N)
    return data.BatchFeeder(clouds(N, dev), B, SIZES, seed=9999)


def kernels_child(launches):
    """The child of the kernel trace: `launches` fills of each feeder."""
    import torch
    dev = torch.device("cuda:0")
    for arm in ("resample", "mesh"):
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


def traced(launches):
    """{kernel name: (launches, median us, min us, max us)} of the feed kernels of the child under rocprofv3."""
    out = tempfile.mkdtemp(prefix="mesh_cost_trace_")
    try:
        step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
              "--kernels-child", "--iters", str(launches)], ROOT, 300)
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        by = {}
        for r in csv.DictReader(open(path)):
            if "feed_batch" in r["Kernel_Name"]:
                by.setdefault(r["Kernel_Name"].split("(")[0], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        return {k: (len(v), statistics.median(v), min(v), max(v)) for k, v in by.items()}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def fit_child(arm, iters):
    """One arm of the fit loop in this process -> one JSON line.  arm: plain | mesh | parent (= plain, on whatever tree this file lies in)."""
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
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its fit loop on clouds as a third arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_mesh.txt"), help="results file ('' for none)")
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
        say("  (feed_batch_kernel<true>: pdgn_feed_batch_resample, %d clouds of %d points drawn to %d; feed_batch_mesh_kernel: pdgn_feed_batch_mesh, "
            "%d meshes of %d faces)" % (S, M, N, S, 2 * GRID * GRID))
    arms = (["parent"] if args.parent else []) + ["plain", "mesh"]
    if args.parent:
        args.parent = os.path.abspath(args.parent)
        shutil.copy(os.path.abspath(__file__), os.path.join(args.parent, "tools", "mesh_cost.py"))
    res = {a: [] for a in arms}
    for r in range(args.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            cwd = args.parent if arm == "parent" else ROOT
            out = step([sys.executable, os.path.join(cwd, "tools", "mesh_cost.py"), "--fit-child", arm, "--iters", str(args.iters)], cwd, 300)
            line = [l for l in out.splitlines() if l.startswith("{")]
            if not line:
                raise SystemExit("fit child %s printed no result, stopping:\n%s" % (arm, out[-2000:]))
            rec = json.loads(line[0])
            if not rec["finite"]:
                raise SystemExit("fit child %s: a loss is not finite, stopping: %r" % (arm, rec))
            res[arm].append(rec["ms_per_iter"])
            print("round %d %-8s %.3f ms/iter" % (r, arm, rec["ms_per_iter"]), flush=True)
    names = {"parent": "parent commit, clouds of %d" % N, "plain": "this tree, clouds of %d" % N, "mesh": "this tree, meshes of %d faces" % (2 * GRID * GRID)}
    for arm in arms:
        v = res[arm]
        say("fit loop, %-34s ms/iter mean %.3f min %.3f max %.3f spread %.3f over %d rounds x %d iterations"
            % (names[arm], sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v), args.iters))
    mean = {a: sum(res[a]) / len(res[a]) for a in arms}
    spread = {a: max(res[a]) - min(res[a]) for a in arms}
    say("mesh - plain: %+.3f ms/iter" % (mean["mesh"] - mean["plain"]))
    if args.parent:
        say("plain - parent: %+.3f ms/iter; mesh - parent: %+.3f ms/iter; run-to-run spread: parent %.3f, mesh %.3f ms"
            % (mean["plain"] - mean["parent"], mean["mesh"] - mean["parent"], spread["parent"], spread["mesh"]))
        say("mesh arm within one arm's own spread of the parent arm: %s" % ("yes" if mean["mesh"] - mean["parent"] <= max(spread["parent"], spread["mesh"]) else "NO"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
