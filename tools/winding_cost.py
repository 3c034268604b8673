#!/usr/bin/env python3
"""What the generalized winding number costs (meshes.winding_number: pdgn_winding_number):
python3 tools/winding_cost.py [--launches L] [--out FILE]          (FILE defaults to profiles/winding_cost.txt)

One child process under `rocprofv3 --kernel-trace --stats` and nothing else in it, no counters:
  * 35 clouds of 2048 points -- the surface draws with 2 % noise of tools/p2m_cost.py -- against one mesh of 1280 (icosphere of level 3),
    10368 (torus grid 72 x 72) and 100352 faces (torus grid 224 x 224): pdgn_point_mesh_distance with cull = 0 on the same inputs (the
    yardstick: every face at every point, as here), pdgn_winding_number with splits = 0 (the library's choice) and with splits = 1;
  * 1 cloud of 256 points against the 100352-face mesh, splits = 1 against splits = 0: what the split is for;
  * meshes.occupancy_grid at R = 64 of the 10368-face mesh: its launches in the trace, and the whole call timed with device events.
L launches each through the raw entry point, so that a launch is the kernels alone; a call with more than one part is its two kernels
together.  Every split of a case is checked to give the same bits.  The times are the kernels' own from the trace, in issue order."""
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
B, N = 35, 2048
MESHES = (("1 k", "icosphere", 3), ("10 k", "torus", 72), ("100 k", "torus", 224))
SMALL_N, GRID_R = 256, 64


def _mesh(kind, size):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import p2m_mirror as pm
    return pm.icosphere(size) if kind == "icosphere" else pm.torus_grid(size, size)


def child(launches):
    import torch
    from pdgn_amd import _lib, meshes
    dev = torch.device("cuda:0")
    L = _lib.lib()

    def winding(ms, rec, x, splits):
        b, n = x.shape[:2]
        shape = torch.zeros(b, dtype=torch.int32, device=dev)
        nbytes = L.pdgn_winding_workspace_bytes(b, n, ms.F, splits)
        work = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
        T = torch.empty(b, n, dtype=torch.int64, device=dev)
        w = torch.empty(b, n, dtype=torch.float32, device=dev)
        for _ in range(launches):
            _lib.check(L.pdgn_winding_number(b, n, ms.S, ms.F, _lib.ptr(x), _lib.ptr(shape), _lib.ptr(ms.face_off), _lib.ptr(rec["records"]),
                                             splits, _lib.ptr(work), _lib.ptr(T), _lib.ptr(w), None, _lib.stream_of(x)), "pdgn_winding_number")
        torch.cuda.synchronize()
        return T, w

    kept = {}
    for label, kind, size in MESHES:
        verts, faces = _mesh(kind, size)
        ms = meshes.MeshSet.from_meshes([(verts, faces)]).to(dev)
        kept[label] = ms
        g = torch.Generator(device=dev).manual_seed(size)
        x = (torch.cat([ms.sample(N, 7, draw=c) for c in range(B)]) + 0.02 * torch.randn(B, N, 3, device=dev, generator=g)).contiguous()
        rec = meshes.mesh_dist_records(ms)
        shape = torch.zeros(B, dtype=torch.int32, device=dev)
        d2 = torch.empty(B, N, dtype=torch.float32, device=dev)
        face = torch.empty(B, N, dtype=torch.int32, device=dev)
        for _ in range(launches):
            _lib.check(L.pdgn_point_mesh_distance(B, N, ms.S, ms.F, rec["G"], _lib.ptr(x), _lib.ptr(shape), _lib.ptr(ms.face_off),
                                                  _lib.ptr(rec["group_off"]), _lib.ptr(rec["records"]), _lib.ptr(rec["groups"]), 0,
                                                  _lib.ptr(d2), _lib.ptr(face), None, _lib.stream_of(x)), "pdgn_point_mesh_distance")
        torch.cuda.synchronize()
        T0, w0 = winding(ms, rec, x, 0)
        T1, w1 = winding(ms, rec, x, 1)
        print(json.dumps({"case": label, "faces": int(faces.shape[0]), "parts": L.pdgn_winding_splits(B, N, ms.F),
                          "same_bits": bool(torch.equal(T0, T1) and torch.equal(w0.view(torch.int32), w1.view(torch.int32))),
                          "inside_share": float((T0 >= L.pdgn_winding_half_turn()).double().mean())}))
        if label == "100 k":
            xs = x[:1, :SMALL_N].contiguous()
            T1, w1 = winding(ms, rec, xs, 1)
            T0, w0 = winding(ms, rec, xs, 0)
            print(json.dumps({"case": "small", "faces": int(faces.shape[0]), "parts": L.pdgn_winding_splits(1, SMALL_N, ms.F),
                              "same_bits": bool(torch.equal(T0, T1) and torch.equal(w0.view(torch.int32), w1.view(torch.int32)))}))
    ms = kept["10 k"]
    meshes.occupancy_grid(ms, resolution=8)                        # (warm: torch's own kernels of the wrapper)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    wall = []
    for _ in range(launches):
        start.record()
        occ, _, _ = meshes.occupancy_grid(ms, resolution=GRID_R)
        stop.record()
        stop.synchronize()
        wall.append(start.elapsed_time(stop))
    print(json.dumps({"case": "grid", "faces": ms.F, "cells_inside": int(occ.sum()), "call_ms": statistics.median(wall),
                      "parts": L.pdgn_winding_splits(1, GRID_R ** 3, ms.F)}))


def traced(launches):
    out = tempfile.mkdtemp(prefix="winding_cost_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--launches", str(launches)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            raise RuntimeError("rocprofv3 child failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
        checks = {c["case"]: c for c in (json.loads(l) for l in run.stdout.splitlines() if l.startswith("{"))}
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        dist, calls = [], []                                       # a winding call: its sum kernel and, with more than one part, the finish kernel
        for r in rows:
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            if "md_distance_kernel" in r["Kernel_Name"]:
                dist.append(us)
            elif "wn_sum_kernel" in r["Kernel_Name"]:
                calls.append([us, 0.0])
            elif "wn_finish_kernel" in r["Kernel_Name"]:
                calls[-1][1] = us
        return checks, dist, calls
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.child:
        return child(args.launches)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    checks, dist, calls = traced(args.launches)                    # (this process never touches the GPU)
    n = args.launches
    assert len(dist) == n * len(MESHES) and len(calls) == n * (2 * len(MESHES) + 2) + 1 + n, (len(dist), len(calls))

    def take(k):
        group = calls[:k]
        del calls[:k]
        total = [a + b for a, b in group]
        return statistics.median(total), min(total), max(total), statistics.median(b for _, b in group)

    say("pdgn_winding_number, rocprofv3 --kernel-trace --stats, %d launches per variant, one process; kernel times in us, median (min .. max); "
        "a call with more than one part is its two kernels together:" % n)
    say("%d clouds of %d points (surface draws with 2 %% noise) against one mesh; the yardstick is pdgn_point_mesh_distance with cull = 0 on the "
        "same inputs:" % (B, N))
    for mi, (label, _, _) in enumerate(MESHES):
        c = checks[label]
        y = dist[mi * n:(mi + 1) * n]
        auto, one = take(n), take(n)
        per = 1e3 * auto[0] / (B * N * c["faces"] / 1e3)
        say("  %s faces (%d): yardstick %10.2f (%10.2f .. %10.2f);  splits = 0 (%d parts) %10.2f (%10.2f .. %10.2f), of which the finish kernel "
            "%.2f;  splits = 1 %10.2f (%10.2f .. %10.2f);  ratio to the yardstick %.3f;  %.2f ns per point and 1000 faces;  both splits the same "
            "bits: %s;  share of the points inside: %.3f" % (label, c["faces"], statistics.median(y), min(y), max(y), c["parts"], *auto[:3], auto[3],
                                                             *one[:3], auto[0] / statistics.median(y), per, c["same_bits"], c["inside_share"]))
        if label == "100 k":
            s = checks["small"]
            one, auto = take(n), take(n)
            say("1 cloud of %d points against the %d-face mesh: splits = 1 %10.2f (%10.2f .. %10.2f);  splits = 0 (%d parts) %10.2f (%10.2f .. "
                "%10.2f), of which the finish kernel %.2f;  the split is %.1f times faster;  the same bits: %s" % (
                    SMALL_N, s["faces"], *one[:3], s["parts"], *auto[:3], auto[3], one[0] / auto[0], s["same_bits"]))
    g = checks["grid"]
    take(1)                                                        # the warm call at R = 8
    grid = take(n)
    say("occupancy_grid at R = %d of the %d-face mesh (%d cells inside, %d parts): the winding kernels of a call %10.2f (%10.2f .. %10.2f); the "
        "whole call, device events: %.2f ms" % (GRID_R, g["faces"], g["cells_inside"], g["parts"], *grid[:3], g["call_ms"]))
    assert not calls
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
