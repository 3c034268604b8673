#!/usr/bin/env python3
"""What the exact EMD (csrc/auction.hip) costs next to the approximate one:
python3 tools/auction_cost.py [--rounds R] [--pairs P] [--clouds S] [--out FILE]   (FILE defaults to profiles/auction_cost.txt)

  kernels   pdgn_auction_assign_indexed against pdgn_emd_cost_indexed on the same P = 512 pairs of 2048 x 2048 points (the eval_c5
            shape, tools/eval_full.py's clouds): one warm-up launch each, then R rounds with the two kernels alternating in one
            process, device events around each launch; us per pair, median / min / max over the rounds.  One batched launch on the
            first 64 pairs reports the bids made and the status counts.
  metrics   the wall time of evaluation.compute_all_metrics on S sample and S reference clouds of 2048 points (3 S^2 pairs) with
            emd="approx" and emd="auction", after a warm-up on 8 clouds, and the EMD entries of both."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2048


def clouds(count, seed, dev):
    """Unit-scale Gaussian clouds, each centred and scaled to unit variance, times 0.25: the size of a normalised shape."""
    import torch
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(count, N, 3, generator=g) * torch.tensor([1.0, 0.6, 0.35])
    c = (c - c.mean(dim=1, keepdim=True)) / c.reshape(count, -1).std(dim=1).view(count, 1, 1)
    return (0.25 * c).to(dev).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--clouds", type=int, default=128, help="sample clouds = reference clouds of the compute_all_metrics run (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auction_cost.txt"), help="results file ('' for none)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from pdgn_amd import _lib, evaluation
    from pdgn_amd._lib import check, ptr, stream_of
    from pdgn_amd.structural_losses import auction_match
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = ["$ python3 tools/auction_cost.py " + " ".join(sys.argv[1:]), "device: %s, %s, %d CUs, %.0f GB" % ((torch.cuda.get_device_name(dev),) + (lambda pr: (pr.gcnArchName, pr.multi_processor_count, pr.total_memory / 2 ** 30))(
                 torch.cuda.get_device_properties(dev)))]
    print(lines[0], flush=True)

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- (a) the two pair-list kernels
    P = args.pairs
    smp, ref = clouds(32, 1, dev), clouds(32, 2, dev)
    p = torch.arange(P, device=dev)
    ia, ib = (p % 32).to(torch.int32).contiguous(), ((p // 32 + p) % 32).to(torch.int32).contiguous()
    cost_x = torch.empty(P, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    cost_a = torch.empty(P, device=dev)
    temp = torch.empty(L.pdgn_emd_cost_temp_floats(P, N, N), device=dev)

    def exact():
        check(L.pdgn_auction_assign_indexed(P, N, ptr(smp), ptr(ia), ptr(ref), ptr(ib), ptr(cost_x), ptr(status), stream_of(smp)),
              "pdgn_auction_assign_indexed")

    def approx():
        check(L.pdgn_emd_cost_indexed(P, N, N, ptr(smp), ptr(ia), ptr(ref), ptr(ib), ptr(temp), ptr(cost_a), stream_of(smp)), "pdgn_emd_cost_indexed")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / P

    exact(), approx()
    torch.cuda.synchronize()
    us = {"auction": [], "approx": []}
    for r in range(args.rounds):
        for name, fn in ((("auction", exact), ("approx", approx)) if r % 2 == 0 else (("approx", approx), ("auction", exact))):
            us[name].append(timed(fn))
    say("(a) %d pairs of %d x %d points, one launch each, %d rounds alternating in one process, device events:" % (P, N, N, args.rounds))
    for name, entry in (("auction", "pdgn_auction_assign_indexed"), ("approx", "pdgn_emd_cost_indexed")):
        v = us[name]
        say("  %-28s us per pair: median %9.2f min %9.2f max %9.2f   (%.2f ms per launch)"
            % (entry, statistics.median(v), min(v), max(v), statistics.median(v) * P / 1e3))
    ratio = statistics.median(us["auction"]) / statistics.median(us["approx"])
    say("  auction / approx: %.1f x" % ratio)
    say("  status of the %d pairs: %d optimal, %d capped, %d degenerate; exact / approximate cost: mean %.4f min %.4f max %.4f"
        % (P, int((status == 0).sum()), int((status == 1).sum()), int((status == 2).sum()), float((cost_x / cost_a).mean()),
           float((cost_x / cost_a).min()), float((cost_x / cost_a).max())))
    k = min(64, P)
    _, _, st, bids = auction_match(smp[ia[:k].long()].contiguous(), ref[ib[:k].long()].contiguous(), with_bids=True)
    say("  bids per pair, first %d pairs: mean %.0f (%.1f n) max %d of the cap %d" % (k, float(bids.double().mean()), float(bids.double().mean()) / N,
                                                                                   int(bids.max()), L.pdgn_auction_max_bids(N)))

    # ---- (b) the whole evaluation
    S = args.clouds
    if S > 0:
        smp, ref = clouds(S, 3, dev), clouds(S, 4, dev)
        for kind in evaluation.EMD_KINDS:
            evaluation.compute_all_metrics(smp[:8].contiguous(), ref[:8].contiguous(), emd=kind)
        say("(b) compute_all_metrics, %d sample and %d reference clouds of %d points (%d pairs in three matrices), wall seconds:" % (S, S, N, 3 * S * S))
        secs = {}
        for kind in evaluation.EMD_KINDS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = evaluation.compute_all_metrics(smp, ref, emd=kind)
            torch.cuda.synchronize()
            secs[kind] = time.perf_counter() - t0
            say('  emd="%s": %8.3f s   lgan_mmd-EMD %.6f lgan_cov-EMD %.4f 1-NN-EMD-acc %.4f%s'
                % (kind, secs[kind], float(res["lgan_mmd-EMD"]), float(res["lgan_cov-EMD"]), float(res["1-NN-EMD-acc"]),
                   "   emd-capped %d" % int(res["emd-capped"]) if "emd-capped" in res else ""))
        say("  auction / approx: %.1f x" % (secs["auction"] / secs["approx"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
