#!/usr/bin/env python3
"""What a change to the dense layers' host code (pdgn_amd/fused.py: dense_route, LinearCL, the NT frame, the hand-overs) did to the
step, this tree against a built checkout of the parent commit, alternating within one session on one GPU:

    python3 tools/dense_route_cost.py --parent _prev [--out profiles/dense_route.txt]

  launch lists  tr._list.info behind one eager step and capture_list at B = 4, the default trainer and one with ema_decay,
                grad_guard, clip_grad_norm and lr_schedule set: equal, count for count
  GEMM_LOG      the multiset of (kind, m, n, k) of one step at B = 4 (as tools/gemm_shapes.py takes it): identical
  step time     bench.py --gpus 1 --steps 20 --warmup 5, three runs per tree: the new mean within the parent's max - min
  host time     linear_cl forward + backward, wall time of 200 calls behind 20 of warm-up with no synchronise inside, a planes-route
                shape with statistics and an own-route shape, three processes per tree: the new mean at most the parent's mean
                plus the parent's max - min.  (The backward runs on the autograd engine's device thread: the hand-over to it and
                back is in that wall time, in one of two regimes per process, ~70 or ~150 us; the forward alone under no_grad, the
                issuing thread only, is listed beside it.)

Every measurement is a child process under a time limit; the first one that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(ema_decay=0.999, grad_guard=True, clip_grad_norm=1.0, lr_schedule=[(0, 0.2), (10, 0.7)])
HOST_SHAPES = {"planes, statistics (6000 x 384 x 256)": (6000, 384, 256, True), "own kernel (5000 x 20 x 12)": (5000, 20, 12, False)}


def lists():
    """(child) launch-list info of both trainers and the step's GEMM log, one JSON line."""
    from collections import Counter
    import torch
    from pdgn_amd import fused
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    out = {}
    for name, kw in (("default", {}), ("all", ALL)):
        torch.manual_seed(0)
        tr = PDGNTrainer(device="cuda", distributed=False, **kw)
        tr.train()
        reals, z1, z2 = synthetic_batch(4, "cuda"), noise(4, "cuda"), noise(4, "cuda")
        tr.step(reals, z1, z2)
        if name == "default":
            fused.GEMM_LOG = []
            tr.step(reals, z1, z2)
            torch.cuda.synchronize()
            log, fused.GEMM_LOG = Counter(fused.GEMM_LOG), None
            out["gemm_log"] = sorted([list(k) + [v] for k, v in log.items()])
        tr.capture_list(reals, z1, z2)
        torch.cuda.synchronize()
        out[name] = tr._list.info
        del tr
    print(json.dumps(out))


def host():
    """(child) us per linear_cl call, issue only, per shape: forward + backward, and the forward alone; one JSON line."""
    import torch
    from pdgn_amd import fused
    out = {}
    for name, (m, n, k, planes) in HOST_SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn(m, k, device="cuda", generator=g).requires_grad_(True)
        w = torch.randn(n, k, device="cuda", generator=g).requires_grad_(True)
        dy = torch.randn(m, n, device="cuda", generator=g)
        pl = fused.split_planes(w.detach(), True) if planes else None

        def forward():
            return fused.linear_cl(x, w, None, None, True, planes=pl)[0] if planes else fused.linear_cl(x, w)

        def both():
            torch.autograd.grad(forward(), (x, w), dy)

        def alone():
            with torch.no_grad():
                forward()
        for call, what in ((both, "forward + backward"), (alone, "forward alone")):
            for _ in range(20):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(200):
                call()
            out["%-38s %s" % (name, what)] = (time.perf_counter() - t0) / 200 * 1e6
            torch.cuda.synchronize()
    print(json.dumps(out))


def child(tree, args, limit):
    """The last line of a child's output, as JSON; the child runs in `tree` with that tree's package."""
    env = dict(os.environ, PDGN_TREE=tree)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + args, cwd=tree, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("FAILED (%d) in %s: %s\n%s" % (r.returncode, tree, " ".join(args), (r.stdout + r.stderr)[-2000:]))
    print("   (ran %s in %s)" % (" ".join(os.path.basename(v) for v in args[:3]), tree), file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def verdict(parent, new, one_sided=False):
    mp, mn, spread = sum(parent) / len(parent), sum(new) / len(new), max(parent) - min(parent)
    ok = (mn - mp <= spread) if one_sided else (abs(mn - mp) <= spread)
    return "parent %s mean %.3f spread (max - min) %.3f | new %s mean %.3f | difference %+.3f %s the parent's spread" % (
        " ".join("%.3f" % v for v in parent), mp, spread, " ".join("%.3f" % v for v in new), mn, mn - mp, "WITHIN" if ok else "OUTSIDE")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    trees = {"parent": os.path.abspath(a.parent), "new": ROOT}
    me = os.path.abspath(__file__)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    got = {tag: child(tree, [me, "--child", "lists"], 420) for tag, tree in trees.items()}
    say("1. Launch lists (tr._list.info behind one eager step and capture_list, B = 4)")
    for cfg in ("default", "all"):
        for tag in ("new", "parent"):
            say("   %s %s %s" % (tag, cfg, got[tag][cfg]))
        say("   %s: %s" % (cfg, "equal, node count for node count" if got["new"][cfg] == got["parent"][cfg] else "DIFFERENT"))
    say("   (all: ema_decay=0.999, grad_guard=True, clip_grad_norm=1.0, lr_schedule=[(0, 0.2), (10, 0.7)])")
    say("2. GEMM_LOG of one step at B = 4: %d distinct (kind, m, n, k), %d launches; parent %d distinct, %d launches: %s" % (
        len(got["new"]["gemm_log"]), sum(e[-1] for e in got["new"]["gemm_log"]), len(got["parent"]["gemm_log"]),
        sum(e[-1] for e in got["parent"]["gemm_log"]), "IDENTICAL multisets" if got["new"]["gemm_log"] == got["parent"]["gemm_log"] else "DIFFERENT"))
    ms = {"parent": [], "new": []}
    for _ in range(3):
        for tag in ("parent", "new"):
            ms[tag].append(child(trees[tag], ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], 420)["ms_per_step"])
    say("3. Device time: python3 bench.py --gpus 1 --steps 20 --warmup 5, ms_per_step, three runs per commit, alternating")
    say("   " + verdict(ms["parent"], ms["new"]))
    us = {"parent": [], "new": []}
    for _ in range(3):
        for tag in ("parent", "new"):
            us[tag].append(child(trees[tag], [me, "--child", "host"], 180))
    say("4. Host time of one linear_cl forward + backward: 20 calls of warm-up, then 200 calls by time.perf_counter with no synchronise")
    say("   inside; us per call; one process per repeat, three per commit, alternating")
    for name in us["new"][0]:
        say("   %-58s %s" % (name, verdict([u[name] for u in us["parent"]], [u[name] for u in us["new"]], one_sided=True)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        sys.path.insert(0, os.environ.get("PDGN_TREE", ROOT))
        {"lists": lists, "host": host}[sys.argv[2]]()
    else:
        main()
