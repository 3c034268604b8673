#!/usr/bin/env python3
"""What face orientation from visibility (pdgn_mesh_face_votes) costs beside the visibility pass it grew from:
python3 tools/face_orient_cost.py [--calls K] [--rounds R] [--parent DIR] [--out FILE]   (FILE defaults to profiles/face_orient_cost.txt)

  kernels   on the 512 meshes of 4608 faces of tools/mesh_cost.py, 26 views at R = 128 (the shapes tools/visible_cost.py uses), K calls
            each of face_visibility, face_orientation and face_orientation(return_mask=True) in ONE child process under
            `rocprofv3 --kernel-trace --stats` (a run of its own): visible_kernel<false> and visible_kernel<true> by name.  With
            --parent DIR (a built checkout of the parent commit) the parent's own tools/visible_cost.py pass child under the same trace,
            in the same run of this tool: the baseline the ratio is taken against.
  pack      `pack --visible` against `pack --visible --orient` on a directory of the first 64 of those meshes as .obj files, the arms
            alternating over R rounds in ONE child process, wall clock of the whole call (reading the files included) and of the device
            calls alone.
The expectation is written into the file before the first GPU step.  Every GPU step is a child process under its own `timeout`; the
tool stops at the first step that fails."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import mesh_cost as mc                                           # noqa: E402  (its meshes and its `step`)

VIEWS, RES, PACKED = 26, 128, 64
EXPECTATION = """expectation, written before the first run (nothing is measured yet):
  kernels  the vote pass shares the visibility kernel's first sweep (the depth minima) bit for bit; its second sweep cannot stop at a
           face's first visible centre, so it looks at every centre of every face once more: slower than the visibility pass, by at most
           the cost of the first sweep again (below 2 x) where faces are small, as on these %d-face meshes at R = %d.  The mask output
           costs one OR per (face, view) on top.
  pack     one depth pass serves both outputs: --visible --orient costs the vote kernel in place of the visibility kernel, not both
measured:""" % (2 * mc.GRID * mc.GRID, RES)


def _arrays(dev, count=None):
    plain = mc.meshes(dev)
    verts, faces, off = plain.verts.cpu().numpy(), plain.faces.cpu().numpy(), plain.face_off.cpu().numpy()
    if count is None:
        return verts, faces, off
    return verts[:faces[:off[count]].max() + 1], faces[:off[count]], off[:count + 1]


def kernels_child(calls):
    import torch
    from pdgn_amd.meshes import face_orientation, face_visibility
    dev = torch.device("cuda:0")
    verts, faces, off = _arrays(dev)
    for _ in range(calls):
        mask = face_visibility(verts, faces, off, views=VIEWS, resolution=RES, device=dev)
    for _ in range(calls):
        alone = face_orientation(verts, faces, off, views=VIEWS, resolution=RES, device=dev)
    for _ in range(calls):
        both = face_orientation(verts, faces, off, views=VIEWS, resolution=RES, device=dev, return_mask=True)
    assert (both["mask"] == mask).all() and (both["front"] == alone["front"]).all() and (both["back"] == alone["back"]).all()
    print(json.dumps({"faces": int(mask.shape[0]), "hidden": int((mask == 0).sum()), "flipped": int(both["flip"].sum()),
                      "undecided": int(both["undecided"].sum()), "two_sided": int(both["two_sided"].sum())}))


def _trace(cmd, cwd):
    """The (kernel name, ms) rows of the visibility kernels of a child under rocprofv3, in launch order, and what the child printed."""
    out = tempfile.mkdtemp(prefix="face_orient_cost_trace_")
    try:
        said = mc.step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + cmd, cwd, 600)
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
                      for r in csv.DictReader(open(path)) if "visible_kernel" in r["Kernel_Name"])
        return [(name, ms) for _, name, ms in rows], said
    finally:
        shutil.rmtree(out, ignore_errors=True)


def _stat(v):
    return "%d launches, median %.2f ms, min %.2f, max %.2f" % (len(v), statistics.median(v), min(v), max(v))


def pack_child(rounds):
    """Both arms in this process, alternating -> one JSON line of seconds per round."""
    import torch
    from pdgn_amd import meshes
    dev = torch.device("cuda:0")
    verts, faces, off = _arrays(dev, PACKED)
    root = tempfile.mkdtemp(prefix="face_orient_cost_obj_")
    try:
        folder = os.path.join(root, "obj", "03001627", "train")
        os.makedirs(folder)
        for c in range(PACKED):
            f = faces[off[c]:off[c + 1]]
            lo = int(f.min())
            with open(os.path.join(folder, "m%03d.obj" % c), "w") as fh:
                fh.write("".join("v %r %r %r\n" % tuple(float(x) for x in p) for p in verts[lo:int(f.max()) + 1]))
                fh.write("".join("f %d %d %d\n" % tuple(int(i) - lo + 1 for i in t) for t in f))
        opts = {"views": VIEWS, "resolution": RES, "device": dev}
        arms = {"visible": (opts, None), "visible+orient": (opts, dict(opts))}
        res = {"pack": {a: [] for a in arms}, "device": {a: [] for a in arms}}
        for r in range(rounds + 1):                              # (round 0 warms up)
            for arm in (sorted(arms) if r % 2 else sorted(arms)[::-1]):
                t0 = time.perf_counter()
                meshes.pack(os.path.join(root, "obj"), os.path.join(root, "out.npz"), *arms[arm])
                t1 = time.perf_counter()
                if arm == "visible":
                    meshes.face_visibility(verts, faces, off, **opts)
                else:
                    meshes.face_orientation(verts, faces, off, return_mask=True, **opts)
                t2 = time.perf_counter()
                if r:
                    res["pack"][arm].append(t1 - t0)
                    res["device"][arm].append(t2 - t1)
        print(json.dumps(res))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3, help="calls of each function in the traced child")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the pack arms")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its visibility kernel as the baseline")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_orient_cost.txt"), help="results file ('' for none)")
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--pack-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.calls)
    if args.pack_child:
        return pack_child(args.rounds)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                             # (after every line: what was measured before a step failed stays)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(EXPECTATION)
    # (this process never touches the GPU: every measurement is a child's)
    say("%d meshes of %d faces, %d views at R = %d, rocprofv3 --kernel-trace --stats, %d calls of each function:"
        % (mc.S, 2 * mc.GRID * mc.GRID, VIEWS, RES, args.calls))
    base = None
    if args.parent:
        cwd = os.path.abspath(args.parent)
        rows, _ = _trace([sys.executable, os.path.join(cwd, "tools", "visible_cost.py"), "--pass-child", "--iters", str(args.calls)], cwd)
        base = statistics.median([ms for _, ms in rows])
        say("  parent commit, pdgn_mesh_visibility (visible_kernel), its own process:   %s" % _stat([ms for _, ms in rows]))
    rows, said = _trace([sys.executable, os.path.abspath(__file__), "--kernels-child", "--calls", str(args.calls)], ROOT)
    rec = json.loads([l for l in said.splitlines() if l.startswith("{")][0])
    vis = [ms for name, ms in rows if "<true>" not in name]
    vote = [ms for name, ms in rows if "<true>" in name]
    if len(vis) != args.calls or len(vote) != 2 * args.calls:
        raise SystemExit("the trace holds %d and %d launches, expected %d and %d" % (len(vis), len(vote), args.calls, 2 * args.calls))
    alone, both = vote[:args.calls], vote[args.calls:]
    say("  this tree, pdgn_mesh_visibility (visible_kernel<false>):                 %s" % _stat(vis))
    say("  this tree, pdgn_mesh_face_votes, mask = NULL (visible_kernel<true>):     %s" % _stat(alone))
    say("  this tree, pdgn_mesh_face_votes with the mask (visible_kernel<true>):    %s" % _stat(both))
    m = statistics.median
    say("  votes with the mask / visibility, this tree: %.2f x; votes alone / visibility: %.2f x" % (m(both) / m(vis), m(alone) / m(vis)))
    if base is not None:
        say("  against the parent's visibility kernel: visibility %.2f x, votes with the mask %.2f x, votes alone %.2f x"
            % (m(vis) / base, m(both) / base, m(alone) / base))
    say("  %d of %d faces hidden; %d flipped, %d undecided, %d two-sided (height fields: open sheets seen from above and below)"
        % (rec["hidden"], rec["faces"], rec["flipped"], rec["undecided"], rec["two_sided"]))
    out = mc.step([sys.executable, os.path.abspath(__file__), "--pack-child", "--rounds", str(args.rounds)], ROOT, 900)
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][0])
    for what, label in (("pack", "pack of %d .obj files (reading them included)" % PACKED), ("device", "the device call alone, %d meshes" % PACKED)):
        for arm in ("visible", "visible+orient"):
            v = rec[what][arm]
            say("%s, --%s: s per call mean %.3f min %.3f max %.3f over %d rounds, one process"
                % (label, arm.replace("+", " --"), sum(v) / len(v), min(v), max(v), len(v)))
    mean = lambda what, arm: sum(rec[what][arm]) / len(rec[what][arm])
    say("--visible --orient - --visible: pack %+.3f s, device call %+.3f s" % (mean("pack", "visible+orient") - mean("pack", "visible"),
                                                                             mean("device", "visible+orient") - mean("device", "visible")))


if __name__ == "__main__":
    main()
