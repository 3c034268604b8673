#!/usr/bin/env python3
"""What feeding a training iteration costs: python3 tools/feed_ab.py [--rounds R] [--block K] [--out FILE]

One process, B = 35, 256 -> 2048 points, S = 4096 synthetic clouds on the device, the launch list captured once.  After a
warm-up of every arm, three arms alternate in blocks of K iterations, R rounds (R * K >= 200 iterations per arm):
  (a) step_list(None, z1, z2) on one fixed batch            -- what bench.py measures
  (b) a batch built with torch ops (index_select by a slice of a permutation, randint + gather per resolution, transposes,
      randn * 0.2) handed to step_list(reals, z1, z2)       -- what a user writes without the feeder
  (c) feeder.fill into the list's static buffers + step_list()  -- PDGNTrainer.fit's path
Per block: ms per iteration by device events around the block, and by a host clock from the block's first call to a
synchronise behind its last.  Per arm: the mean over blocks and the spread (max - min) between blocks of the SAME arm, which
is the resolution of every difference printed below it.  Also: the feed launch alone (back-to-back launches by device
events) against its byte floor (bytes written + bytes gathered over the 8 TB/s HBM peak), and the host time of one
`fill` call."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pdgn_amd.data import BatchFeeder  # noqa: E402
from pdgn_amd.trainer import PDGNTrainer  # noqa: E402

B, N, SIZES, S, SIGMA = 35, 2048, (256, 512, 1024), 4096, 0.2
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "feed_ab.py measures on the GPU"
    assert args.rounds * args.block >= 200
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator().manual_seed(9999)
    clouds = torch.randn(S, N, 3, generator=g)
    clouds = ((clouds - clouds.mean(dim=1, keepdim=True)) / clouds.reshape(S, -1).std(dim=1).view(S, 1, 1)).to(dev).contiguous()
    feeder = BatchFeeder(clouds, B, SIZES, seed=9999, sigma=SIGMA)
    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    reals, z1, z2 = feeder.buffers()
    feeder.fill(1, 0, reals, z1, z2)
    tr.capture_list(reals, z1, z2)
    st = tr._static
    fixed_z1, fixed_z2 = z1.clone(), z2.clone()
    perm = torch.randperm(S, device=dev)
    nb = feeder.batches_per_epoch
    count = {"b": 0, "c": 0}

    def arm_a():
        tr.step_list(None, fixed_z1, fixed_z2)

    def arm_b():
        i = count["b"] % nb
        count["b"] += 1
        pcs = clouds.index_select(0, perm[i * B:(i + 1) * B])
        rs = []
        for r in SIZES:
            sel = torch.randint(0, N, (B, r), device=dev)
            rs.append(torch.gather(pcs, 1, sel.unsqueeze(2).expand(B, r, 3)).transpose(1, 2).contiguous())
        rs.append(pcs.transpose(1, 2).contiguous())
        tr.step_list(rs, torch.randn(B, 128, device=dev) * SIGMA, torch.randn(B, 128, device=dev) * SIGMA)

    def arm_c():
        i = count["c"]
        count["c"] += 1
        feeder.fill(1 + i // nb, i % nb, st["reals"], st["z1"], st["z2"])
        tr.step_list()

    arms = (("a", arm_a), ("b", arm_b), ("c", arm_c))
    for _, fn in arms:                                           # warm-up: every arm's shapes and allocations
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    res = {k: {"dev": [], "host": []} for k, _ in arms}
    for _ in range(args.rounds):
        for k, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.block):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[k]["host"].append((time.perf_counter() - t0) * 1e3 / args.block)
            res[k]["dev"].append(e0.elapsed_time(e1) / args.block)
    finite = all(torch.isfinite(v).item() for v in st["out"].values())
    say("feed_ab: B=%d %d->%d S=%d, %d rounds x %d iterations per arm (%d per arm), one process; losses finite: %s"
        % (B, SIZES[0], N, S, args.rounds, args.block, args.rounds * args.block, finite))
    say("arm  what                                   ms/iter (device events)      ms/iter (host clock + sync)")
    say("                                            mean    min    max  spread    mean    min    max  spread")
    names = {"a": "step_list(None, z1, z2), fixed batch", "b": "torch-built batch + step_list(r,z,z)", "c": "feeder.fill + step_list()"}
    mean = {}
    for k, _ in arms:
        row = []
        for clock in ("dev", "host"):
            v = res[k][clock]
            m = sum(v) / len(v)
            mean[k, clock] = (m, max(v) - min(v))
            row += [m, min(v), max(v), max(v) - min(v)]
        say("(%s)  %-38s %6.3f %6.3f %6.3f %6.3f   %6.3f %6.3f %6.3f %6.3f" % ((k, names[k]) + tuple(row)))
    for clock, label in (("dev", "device events"), ("host", "host clock")):
        spread = max(mean[k, clock][1] for k in "abc")
        say("%s: (c) - (a) = %+.3f ms, (c) - (b) = %+.3f ms, (b) - (a) = %+.3f ms; largest block-to-block spread of one arm %.3f ms"
            % (label, mean["c", clock][0] - mean["a", clock][0], mean["c", clock][0] - mean["b", clock][0],
               mean["b", clock][0] - mean["a", clock][0], spread))

    # the feed launch alone: back-to-back launches on an idle device, and the host side of one call
    n = 2000
    for _ in range(20):
        feeder.fill(1, 0, st["reals"], st["z1"], st["z2"])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for i in range(n):
        feeder.fill(1, i % nb, st["reals"], st["z1"], st["z2"])
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    written = 4 * B * (3 * (sum(SIZES) + N) + 2 * 128)
    gathered = 4 * B * 3 * (sum(SIZES) + N)
    floor_us = (written + gathered) / HBM_PEAK * 1e6
    per_us = e0.elapsed_time(e1) * 1e3 / n
    say("feed launch alone: %.2f us per launch back to back by device events over %d launches, %.2f us of host time per fill call (where "
        "the two agree the host's issue rate is what was timed; the kernel's own time comes from a kernel trace); writes %d B + gathers "
        "%d B -> byte floor %.2f us at 8 TB/s = %.1f%% of that time: launch-bound at this size"
        % (per_us, n, (t1 - t0) * 1e6 / n, written, gathered, floor_us, 100 * floor_us / per_us))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
