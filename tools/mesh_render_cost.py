#!/usr/bin/env python3
"""What drawing meshes into a preview sheet costs (report.MeshColumn: pdgn_render_sheet_mesh):
python3 tools/mesh_render_cost.py [--launches L] [--out FILE]          (FILE defaults to profiles/mesh_render_cost.txt)

One child process under `rocprofv3 --kernel-trace --stats` and nothing else in it, no counters.  Sheets of 8 rows x 1 column, cell 128:
  (a) the triangle kernel on the surface-nets meshes of 8 clouds of 2048 points (noisy spheres) at R = 64: many faces of a few pixels;
  (b) the triangle kernel on a box of 12 faces per row that fills the cell: few faces of thousands of pixels (the wave path);
  the yardstick: pdgn_render_sheet_lit's splat kernel on the clouds of (a), with normals, at the same sheet size;
  reconstruct() itself on the same clouds: its kernels in the trace between two markers (a one-point pdgn_render_sheet each), and the
  call timed with device events.
L launches each through the raw entry point; the times are the kernels' own from the trace, in issue order.  Then, in a second child
process without the profiler, one snapshot report (8 rows, 35 validation clouds, a generator that draws spheres) with and without
mesh=64: the `seconds` column of its metrics.csv."""
import argparse
import csv
import ctypes
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, N, CELL, R = 8, 2048, 128, 64


def _clouds(dev, count=ROWS):
    import torch
    g = torch.Generator().manual_seed(5)
    d = torch.randn(count, N, 3, generator=g)
    d = d / d.norm(dim=2, keepdim=True) * (0.9 + 0.01 * torch.randn(count, N, 1, generator=g))
    return d.contiguous().to(dev)


def child(launches):
    import numpy as np
    import torch
    from pdgn_amd import _lib
    from pdgn_amd.pointops import estimate_normals
    from pdgn_amd.reconstruct import reconstruct
    from pdgn_amd.report import MeshColumn, _light, default_view
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mesh_render_mirror as mm
    dev = torch.device("cuda:0")
    L = _lib.lib()
    view = default_view(CELL)
    light = _light(view, True)
    clouds = _clouds(dev)
    normals = estimate_normals(clouds, 16)
    ws = torch.empty(L.pdgn_render_workspace_bytes(ROWS, 1, CELL) // 4, dtype=torch.int32, device=dev)
    image = torch.empty((ROWS * CELL, CELL), dtype=torch.uint8, device=dev)
    one = ctypes.c_void_p * 1
    vp, lp = view.ctypes.data_as(ctypes.c_void_p), light.ctypes.data_as(ctypes.c_void_p)

    def mesh_sheet(col):
        for _ in range(launches):
            _lib.check(L.pdgn_render_sheet_mesh(ROWS, 1, one(None), one(None), (ctypes.c_int * 1)(0), 0, one(col.verts.data_ptr()),
                                                one(col.faces.data_ptr()), one(col.range.data_ptr()), one(None),
                                                (ctypes.c_int * 1)(col.verts.shape[0]), (ctypes.c_int * 1)(col.faces.shape[0]), (ctypes.c_int * 1)(0),
                                                vp, lp, CELL, 1, _lib.ptr(ws), _lib.ptr(image), _lib.stream_of(image)), "pdgn_render_sheet_mesh")
        torch.cuda.synchronize()
        return int((image != 0).sum())

    dot, dot_ws, dot_image = torch.zeros(1, 1, 3, device=dev), torch.empty(16, dtype=torch.int32, device=dev), torch.empty((4, 4), dtype=torch.uint8, device=dev)

    def marker():                                                  # a one-point depth-shaded sheet: the only render_splat_kernel launches of this process
        _lib.check(L.pdgn_render_sheet(1, 1, one(dot.data_ptr()), (ctypes.c_int * 1)(1), 0, vp, 4, 0, _lib.ptr(dot_ws), _lib.ptr(dot_image),
                                       _lib.stream_of(dot_image)), "pdgn_render_sheet")

    reconstruct(clouds[:1], resolution=8)                          # (warm: torch's own kernels of the wrapper)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    wall = []
    for _ in range(launches):
        marker()
        start.record()
        verts, faces, vert_off, face_off, stats = reconstruct(clouds, resolution=R)
        stop.record()
        stop.synchronize()
        marker()
        wall.append(start.elapsed_time(stop))
    torch.cuda.synchronize()
    nets = MeshColumn.from_surface_nets(verts, faces, vert_off, face_off)
    lit_a = mesh_sheet(nets)
    bv, bf = mm.box_mesh(0.577)
    box = MeshColumn(torch.from_numpy(np.tile(bv, (ROWS, 1))).to(dev), torch.from_numpy(np.tile(bf, (ROWS, 1)).astype(np.int32)).to(dev),
                     [12 * r for r in range(ROWS)], [12] * ROWS, [8 * r for r in range(ROWS)])
    lit_b = mesh_sheet(box)
    for _ in range(launches):
        _lib.check(L.pdgn_render_sheet_lit(ROWS, 1, one(clouds.data_ptr()), one(normals.data_ptr()), (ctypes.c_int * 1)(N), 0, vp, lp, CELL, 1,
                                           _lib.ptr(ws), _lib.ptr(image), _lib.stream_of(image)), "pdgn_render_sheet_lit")
    torch.cuda.synchronize()
    print(json.dumps({"faces_a": int(faces.shape[0]), "lit_a": lit_a, "faces_b": 12 * ROWS, "lit_b": lit_b, "lit_splat": int((image != 0).sum()),
                      "reconstruct_ms": statistics.median(wall)}))


class _Spheres:
    """A trainer whose generator draws spheres (what a report asks of one), so that the reconstruction has surfaces to find."""
    ema = None

    def __init__(self, dev):
        import torch

        class G(torch.nn.Module):
            def __init__(self):
                super().__init__()
                d = torch.randn(N, 3, generator=torch.Generator().manual_seed(12))
                self.register_buffer("dirs", d / d.norm(dim=1, keepdim=True))
                self.gain = torch.nn.Parameter(torch.ones(1))

            def forward(self, z):
                r = (0.5 + 0.2 * torch.tanh(z[:, :1])) * self.gain
                return [(self.dirs[:n].t()[None] * r[:, :, None]).contiguous() for n in (256, 512, 1024, 2048)]

            def forward_hints(self):
                return []

            def restore_forward_hints(self, hints):
                pass
        self.G = G().to(dev)


def child_report():
    import torch
    from pdgn_amd.report import SnapshotReporter
    dev = torch.device("cuda:0")
    val = _clouds(dev, 35)
    out = tempfile.mkdtemp(prefix="mesh_render_cost_report_")
    try:
        seconds = {}
        for name, extra in (("plain", {}), ("mesh", {"mesh": R})):
            rep = SnapshotReporter(_Spheres(dev), val, os.path.join(out, name), every=1, batch_size=35, normalize=None, seed=9999, rows=ROWS, **extra)
            rep(1)                                                 # (warm: the kernels' first launches)
            seconds[name] = [rep(1)[2] for _ in range(3)]
        print(json.dumps(seconds))
    finally:
        shutil.rmtree(out, ignore_errors=True)


def traced(launches):
    out = tempfile.mkdtemp(prefix="mesh_render_cost_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--launches", str(launches)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            raise RuntimeError("rocprofv3 child failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
        (facts,) = [json.loads(l) for l in run.stdout.splitlines() if l.startswith("{")]
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        mesh, splat, recon, inside = [], [], [], False
        for r in rows:
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            name = r["Kernel_Name"]
            if "render_mesh_kernel" in name:
                mesh.append(us)
            elif "render_splat_lit_kernel" in name:
                splat.append(us)
            elif "render_splat_kernel" in name:                    # the markers around a reconstruct call
                inside = not inside
                if inside:
                    recon.append(0.0)
            elif inside and "render_" not in name:                 # (not the markers' own clear and resolve)
                recon[-1] += us
        return facts, mesh, splat, recon
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_render_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-report", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.child:
        return child(args.launches)
    if args.child_report:
        return child_report()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    facts, mesh, splat, recon = traced(args.launches)              # (this process never touches the GPU)
    n = args.launches
    assert len(mesh) == 2 * n and len(splat) == n, (len(mesh), len(splat), len(recon))
    med = lambda v: (statistics.median(v), min(v), max(v))        # noqa: E731
    a, b, s = med(mesh[:n]), med(mesh[n:]), med(splat)
    rc = med(recon) if len(recon) == n else (float("nan"),) * 3    # (the markers were not found in the trace: the device events remain)
    say("pdgn_render_sheet_mesh, rocprofv3 --kernel-trace --stats, %d launches per case, one process; kernel times in us, median (min .. max); "
        "sheets of %d rows x 1 column, cell %d:" % (n, ROWS, CELL))
    say("  (a) surface-nets meshes of %d clouds of %d points at R = %d, %d faces: render_mesh_kernel %9.2f (%9.2f .. %9.2f); %d pixels lit; "
        "%.2f ns per lit pixel, %.2f ns per face" % (ROWS, N, R, facts["faces_a"], *a, facts["lit_a"], 1e3 * a[0] / facts["lit_a"],
                                                     1e3 * a[0] / facts["faces_a"]))
    say("  (b) a box of 12 faces per row filling the cell, %d faces: render_mesh_kernel %9.2f (%9.2f .. %9.2f); %d pixels lit (every one "
        "covered by a front and a back face); %.2f ns per lit pixel; (b) / (a) per lit pixel: %.2f" % (
            facts["faces_b"], *b, facts["lit_b"], 1e3 * b[0] / facts["lit_b"], (b[0] / facts["lit_b"]) / (a[0] / facts["lit_a"])))
    say("  yardstick, render_splat_lit_kernel on the clouds of (a) with normals, radius 1: %9.2f (%9.2f .. %9.2f); %d pixels lit" % (*s, facts["lit_splat"]))
    say("  reconstruct(resolution = %d) on the same clouds: its kernels (torch's own among them) %9.2f (%9.2f .. %9.2f); the whole call, device "
        "events: %.2f ms" % (R, *rc, facts["reconstruct_ms"]))
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-report"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    if run.returncode != 0:
        raise RuntimeError("report child failed:\n" + run.stdout[-2000:] + run.stderr[-2000:])
    (seconds,) = [json.loads(l) for l in run.stdout.splitlines() if l.startswith("{")]
    say("one snapshot report, %d rows, 35 validation clouds, a generator that draws spheres, no profiler; the `seconds` column, three reports "
        "after a warm one: without mesh %s; with mesh = %d %s" % (ROWS, " ".join("%.3f" % v for v in seconds["plain"]), R,
                                                                  " ".join("%.3f" % v for v in seconds["mesh"])))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
