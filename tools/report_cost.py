#!/usr/bin/env python3
"""What a snapshot report costs next to the training it interrupts: python3 tools/report_cost.py [--rounds R] [--block K]
[--val V] [--out FILE] [--sheet-only]   (FILE defaults to profiles/report_cost.txt)

One process, B = 35, 256 -> 2048 points, S = 4096 synthetic training clouds (117 iterations per epoch) and V synthetic
held-out clouds (no data file is read: the sizes are what matters to the cost), the launch list captured once.
  sheet    render_sheet of 35 x 5 cells (the generator's four outputs as they are + 35 reference clouds, fit=True and the raw
           launch sequence alone): device events over back-to-back calls, host clock per synchronised call
  metrics  quick_metrics on the V clouds, cold (with the ref-vs-ref pass) and warm
  report   one whole SnapshotReporter call (8 rows, PNG and CSV written)
  A/B      blocks of K iterations of fit's inner loop (feeder.fill + step_list()), alternating: (a) nothing in between -- the
           code path of fit without a reporter, which this change does not touch -- and (b) a report in front of the block
           (outside the block's clock).  Per arm: ms per iteration, mean and block-to-block spread.
--sheet-only stops after the sheet (for a kernel trace of the three launches)."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pdgn_amd import report  # noqa: E402
from pdgn_amd.data import BatchFeeder, normalize_clouds  # noqa: E402
from pdgn_amd.trainer import PDGNTrainer  # noqa: E402

B, N, SIZES, S = 35, 2048, (256, 512, 1024), 4096


def clouds(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(n, N, 3, generator=g)
    return ((c - c.mean(dim=1, keepdim=True)) / c.reshape(n, -1).std(dim=1).view(n, 1, 1)).to(dev).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--val", type=int, default=662)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--sheet-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "report_cost.py measures on the GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, n):
        """(device-event ms per call back to back, host ms per call with a synchronise behind each)"""
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
            torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n, (time.perf_counter() - t0) * 1e3 / n

    torch.manual_seed(0)
    tr = PDGNTrainer(device=dev, distributed=False)
    tr.train()
    val = normalize_clouds(clouds(args.val, 1, dev), "shape_bbox")[0].contiguous()
    tr.G.eval()
    with torch.no_grad():
        outs = [o.detach() for o in tr.G(torch.randn(B, 128, device=dev))]
    tr.G.train()
    cols = outs + [val[:B]]
    fitted = [report.fit_unit_sphere(c.transpose(1, 2) if c.shape[1] == 3 else c) for c in cols]
    raw = timed(lambda: report.render_sheet(fitted), 200)
    full = timed(lambda: report.render_sheet(cols, fit=True), 200)
    say("sheet 35 x 5 cells of 128 px (2240 x 640), %d points per row: launch sequence alone %.1f us by device events back to back, "
        "%.1f us host clock per synchronised call; with the unit-sphere fit (torch ops) %.1f / %.1f us"
        % (sum(c.shape[1] for c in fitted), raw[0] * 1e3, raw[1] * 1e3, full[0] * 1e3, full[1] * 1e3))
    if args.sheet_only:
        return

    def metrics(cache):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = report.quick_metrics(tr.G, val, B, "shape_bbox", torch.Generator(device=dev).manual_seed(3), cache)
        float(r["jsd"])
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    cache = {}
    metrics({})                                                  # warm-up of every shape
    cold = metrics(cache)
    warm = [metrics(cache) for _ in range(3)]
    say("quick_metrics on %d synthetic held-out clouds of %d points (B = %d): cold %.2f s (with the ref-vs-ref pass), warm %.2f s "
        "(min of 3; max %.2f)" % (args.val, N, B, cold, min(warm), max(warm)))

    feeder = BatchFeeder(clouds(S, 9999, dev), B, SIZES, seed=9999)
    reals, z1, z2 = feeder.buffers()
    feeder.fill(1, 0, reals, z1, z2)
    tr.capture_list(reals, z1, z2)
    st = tr._static
    nb = feeder.batches_per_epoch
    tmp = tempfile.mkdtemp(prefix="report_cost_")
    rep = report.SnapshotReporter(tr, val, tmp, every=1, batch_size=B, normalize="shape_bbox", seed=9999)
    count = [0]

    def block(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(k):
            i = count[0]
            count[0] += 1
            feeder.fill(1 + i // nb, i % nb, st["reals"], st["z1"], st["z2"])
            tr.step_list()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k, (time.perf_counter() - t0) * 1e3 / k

    block(20)
    rep(1)
    block(20)
    res = {"a": [], "b": []}
    reports = []
    for r in range(args.rounds):
        res["a"].append(block(args.block))
        reports.append(rep(r + 2)[2])
        res["b"].append(block(args.block))
    finite = all(torch.isfinite(v).item() for v in st["out"].values())
    say("one default report (8 rows, preview PNG + CD-only metrics row): %.2f s mean of %d (min %.2f, max %.2f)"
        % (sum(reports) / len(reports), len(reports), min(reports), max(reports)))
    say("A/B: %d rounds x %d iterations per arm, alternating; losses finite: %s.  Both arms run fit's inner loop (feeder.fill into the "
        "list's static buffers + step_list()) in THIS process: arm (a) is the loop of fit without a reporter, whose code (trainer.py, "
        "data.py, the step's kernels) is the same as before reports existed, not a separate build of it" % (args.rounds, args.block, finite))
    mean = {}
    for k, name in (("a", "no report in front of the block"), ("b", "a report in front of the block")):
        for j, clock in enumerate(("device events", "host clock")):
            v = [x[j] for x in res[k]]
            mean[k, j] = sum(v) / len(v)
            say("(%s) %-32s %-13s ms/iter mean %.3f min %.3f max %.3f spread %.3f" % (k, name, clock, mean[k, j], min(v), max(v), max(v) - min(v)))
    epoch_s = mean["a", 1] * nb / 1e3
    per = sum(reports) / len(reports)
    say("(b) - (a): %+.3f ms/iter by device events, %+.3f by the host clock" % (mean["b", 0] - mean["a", 0], mean["b", 1] - mean["a", 1]))
    say("an epoch of %d iterations: %.2f s; the 20 epochs between two snapshots: %.1f s; one default report: %.2f s = %.1f%% of them"
        % (nb, epoch_s, 20 * epoch_s, per, 100 * per / (20 * epoch_s)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
