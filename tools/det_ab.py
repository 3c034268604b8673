#!/usr/bin/env python3
"""Cost of the deterministic mode where it applies: the backward of pointops grouping / interpolation / gathering and of
nn_distance, default (float atomics) against fixed order (csrc/det.hip: CSR transpose + ordered gather), interleaved.
python3 tools/det_ab.py [--repeats R] [--iters N]: per shape and form the median over R repeats of the mean time of N calls
(hipEvent-timed, synchronised between repeats), workspace allocation included (the autograd functions allocate it per call).
Includes the hub case (60 % of the indices on two points) next to uniform indices."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pdgn_amd import _lib, pointops  # noqa: E402
from pdgn_amd.structural_losses import nn_distance  # noqa: E402


def idx_of(shape, n, gen, hub):
    idx = torch.randint(0, n, shape, generator=gen, dtype=torch.int32)
    if hub:
        idx = torch.where(torch.rand(shape, generator=gen) < 0.6, torch.randint(0, 2, shape, generator=gen, dtype=torch.int32), idx)
    return idx.cuda()


def cases(gen):
    """name -> callable running one backward (autograd, the public route)."""
    out = {}
    for hub in (False, True):
        tag = "hub" if hub else "uniform"
        b, c, n, m, ns = 8, 64, 2048, 2048, 32                   # E = m * ns = 65536 per batch
        f = torch.randn(b, c, n, device="cuda", requires_grad=True)
        gi = idx_of((b, m, ns), n, gen, hub)
        go = torch.randn(b, c, m, ns, device="cuda")
        y = pointops.grouping(f, gi)
        out["grouping b8 c64 n2048 m2048 ns32 %s" % tag] = (lambda y=y, g=go, f=f: torch.autograd.grad(y, f, g, retain_graph=True))
        b, c, n, m = 8, 128, 2048, 512
        f2 = torch.randn(b, c, m, device="cuda", requires_grad=True)
        ii = idx_of((b, n, 3), m, gen, hub)
        iw = torch.rand(b, n, 3, device="cuda")
        y2 = pointops.interpolation(f2, ii, iw)
        g2 = torch.randn(b, c, n, device="cuda")
        out["interpolation b8 c128 n2048 m512 %s" % tag] = (lambda y=y2, g=g2, f=f2: torch.autograd.grad(y, f, g, retain_graph=True))
        f3 = torch.randn(b, c, n, device="cuda", requires_grad=True)
        si = idx_of((b, 512), n, gen, hub)
        y3 = pointops.gathering(f3, si)
        g3 = torch.randn(b, c, 512, device="cuda")
        out["gathering b8 c128 n2048 m512 %s" % tag] = (lambda y=y3, g=g3, f=f3: torch.autograd.grad(y, f, g, retain_graph=True))
    a = torch.rand(8, 2048, 3, device="cuda", requires_grad=True)
    q = torch.rand(8, 2048, 3, device="cuda", requires_grad=True)
    d1, d2 = nn_distance(a, q)
    gd1, gd2 = torch.randn_like(d1), torch.randn_like(d2)
    out["nn_distance b8 n2048 m2048"] = lambda: torch.autograd.grad((d1, d2), (a, q), (gd1, gd2), retain_graph=True)
    return out


def time_one(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    runs = cases(gen)
    print("%-48s %12s %12s %8s" % ("backward (autograd)", "default ms", "fixed ms", "ratio"))
    for name, fn in runs.items():
        for det in (False, True):                               # warm-up of both forms (allocator, code objects)
            _lib.set_deterministic(det)
            time_one(fn, 2)
        t = {False: [], True: []}
        for _ in range(args.repeats):
            for det in (False, True):
                _lib.set_deterministic(det)
                t[det].append(time_one(fn, args.iters))
        a, b = statistics.median(t[False]), statistics.median(t[True])
        print("%-48s %12.4f %12.4f %8.2f" % (name, a, b, b / a))
    _lib.set_deterministic(None)


if __name__ == "__main__":
    main()
