#!/usr/bin/env python3
"""What the repulsion regulariser (PDGNTrainer(repulsion=...)) costs:
python3 tools/repulsion_cost.py [--rounds R] [--iters K] [--parent DIR] [--out FILE] [--no-trace]   (FILE defaults to profiles/repulsion_cost.txt)

  kernels   20 calls of losses.repulsion, forward and backward, at each of the four level shapes of B = 35 (256, 512, 1024, 2048 points)
            and nothing else in one child process under `rocprofv3 --kernel-trace --stats`: the all-pairs kernel's, the reduction's and
            the backward scale's own times, per shape.  The clouds are unit-normal, the radius holds 43 % of the pairs.
  fit       fit's inner loop (feeder.fill into the launch list's static buffers + step_list()) in FRESH child processes, K iterations
            each after 20 of warm-up, the arms alternating over R rounds on one box: this tree without the term, with it (weight 0.05,
            all four levels, the radius calibrated from the feeder as the command line does), and -- with --parent DIR, a built
            checkout of the parent commit -- the parent's code on its loop.  Per arm: ms per iteration by device events, mean and
            spread over the rounds, and the launch list's node and kernel counts."""
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
LEVELS = (256, 512, 1024, 2048)
RADIUS = 2.0                        # unit-normal clouds: P[chi2_3 < 2] = 43 % of the pairs inside


def clouds(count, points, dev):
    import torch
    g = torch.Generator().manual_seed(9999)
    c = torch.randn(count, points, 3, generator=g)
    return ((c - c.mean(dim=1, keepdim=True)) / c.reshape(count, -1).std(dim=1).view(count, 1, 1)).to(dev).contiguous()


def kernels_child(launches):
    """The child of the kernel trace: per level shape, `launches` forward + backward calls of the op."""
    import torch
    from pdgn_amd import losses
    dev = torch.device("cuda:0")
    for n in LEVELS:
        x = torch.randn(B, n, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(n)).requires_grad_(True)
        for _ in range(launches):
            x.grad = None
            loss = losses.repulsion(x, RADIUS)
            loss.backward()
        torch.cuda.synchronize()
        print(json.dumps({"n": n, "loss": loss.item(), "finite": bool(torch.isfinite(x.grad).all().item())}))


def traced(launches):
    """([the child's JSON lines], {kernel name: [us per launch, in issue order]}) of the child under rocprofv3."""
    out = tempfile.mkdtemp(prefix="repulsion_cost_trace_")
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
            if "repulsion" in name:
                by.setdefault("repulsion_kernel" if "repulsion_kernel" in name else name, []).append(
                    ((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, name))
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
    kw, radius = {}, None
    if arm == "on":
        from pdgn_amd.train import calibrate_repulsion_radius
        radius, _ = calibrate_repulsion_radius(feeder)
        kw = {"repulsion": {"weight": 0.05, "radius": radius}}
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
    rec = {"arm": arm, "ms_per_iter": ms, "finite": finite, "nodes": info["nodes"], "kernels": info["kernels"], "radius": radius}
    if arm == "on":
        rec["state"] = tr.repulsion_state()["per_level"]
    print(json.dumps(rec))
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=60, help="iterations per fit child")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its fit loop as a third arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repulsion_cost.txt"), help="results file ('' for none)")
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
        say("(a) the op alone, rocprofv3 --kernel-trace --stats, %d forward + backward calls per level shape of B = %d, one process; unit-normal "
            "clouds, radius %g (43 %% of the pairs inside):" % (launches, B, RADIUS))
        for name, v in sorted(by.items()):
            # issue order: the four shapes one after the other, `launches` launches each
            for k, n in zip(range(0, len(v), launches), LEVELS):
                g = [us for us, _ in v[k:k + launches]]
                full = v[k][1]
                say("  %-28s n = %4d: %3d launches, median %8.2f us, min %8.2f, max %8.2f   (%s)"
                    % (name[:28], n, len(g), statistics.median(g), min(g), max(g), full[:40]))
        pairs = sum(B * n * (n - 1) for n in LEVELS)
        fwd = sum(statistics.median([us for us, _ in by["repulsion_kernel"][k:k + launches]]) for k in range(0, 4 * launches, launches)) if "repulsion_kernel" in by else float("nan")
        say("  all four levels: %.1f M ordered pairs, %.1f us of all-pairs kernel time: %.2f G pairs / s" % (pairs / 1e6, fwd, pairs / fwd / 1e3))
        for c in checks:
            say("  n = %4d: loss %.6g, gradient %s" % (c["n"], c["loss"], "finite" if c["finite"] else "NOT FINITE"))
    arms = (["parent"] if args.parent else []) + ["off", "on"]
    if args.parent:
        args.parent = os.path.abspath(args.parent)
        shutil.copy(os.path.abspath(__file__), os.path.join(args.parent, "tools", "repulsion_cost.py"))
    res, recs = {a: [] for a in arms}, {}
    for r in range(args.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            cwd = args.parent if arm == "parent" else ROOT
            run = subprocess.run([sys.executable, os.path.join(cwd, "tools", "repulsion_cost.py"), "--fit-child", arm, "--iters", str(args.iters)],
                                 cwd=cwd, capture_output=True, text=True, timeout=600)
            line = [l for l in run.stdout.splitlines() if l.startswith("{")]
            if run.returncode != 0 or not line:
                raise RuntimeError("fit child %s failed:\n%s" % (arm, run.stdout[-2000:] + run.stderr[-2000:]))
            rec = json.loads(line[0])
            assert rec["finite"], rec
            res[arm].append(rec["ms_per_iter"])
            recs[arm] = rec
            print("round %d %-8s %.3f ms/iter" % (r, arm, rec["ms_per_iter"]), flush=True)
    names = {"parent": "parent commit", "off": "this tree, no repulsion", "on": "this tree, repulsion 0.05 on 4 levels"}
    say("(b) fit's loop, B = %d, clouds of %d points, sizes %s:" % (B, N, SIZES))
    for arm in arms:
        v = res[arm]
        say("  %-38s ms/iter mean %.3f min %.3f max %.3f spread %.3f over %d rounds x %d iterations; list: %d nodes, %d kernels"
            % (names[arm], sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v), args.iters, recs[arm]["nodes"], recs[arm]["kernels"]))
    mean = {a: sum(res[a]) / len(res[a]) for a in arms}
    say("  on - off: %+.3f ms/iter; calibrated radius %.6g; last iteration's value per level %s"
        % (mean["on"] - mean["off"], recs["on"]["radius"], ", ".join("%.4g" % v for v in recs["on"]["state"])))
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
