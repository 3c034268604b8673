#!/usr/bin/env python3
"""What visible-surface sampling (pdgn_mesh_visibility) costs:
python3 tools/visible_cost.py [--rounds R] [--iters K] [--parent DIR] [--out FILE] [--no-trace]   (FILE defaults to profiles/mesh_visible.txt)

  pass      pdgn_mesh_visibility alone on the 512 meshes of 4608 faces of tools/mesh_cost.py, 26 views at R = 128, three calls in one
            child process under `rocprofv3 --kernel-trace --stats` (a run of its own): the kernel's own time, once per run or per `pack`.
  feed      pdgn_feed_batch_mesh with a masked alias table against an unmasked one, alternating in ONE child process: R rounds of 200
            launches per arm by device events, B = 35, 256 .. 2048 points.  The tool's meshes are height fields, of which some view sees
            every face; so that the masked table has zero-weight records to step over, the masked arm also clears the mask of every
            third face (what is measured is the kernel on such a table, not where the zeros came from).
  fit       fit's inner loop in FRESH child processes, K iterations each after 20 of warm-up, the arms alternating over R rounds: with
            --parent DIR (a built checkout of the parent commit) the parent's own mesh arm; this tree on the unmasked set; this tree on
            the masked set.  Judged against the parent arm's own run-to-run spread, as tools/mesh_cost.py judges.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import mesh_cost as mc                                           # noqa: E402  (its meshes, its fit child, its `step`)

VIEWS, RES = 26, 128
EXPECTATION = """expectation, written before the first run (nobody has measured either number):
  pass   a one-off of the order of a second for a category: %d shapes x %d views = %d workgroups of one depth buffer each, two sweeps over
         %d faces per workgroup, two workgroups per CU (64 KB of LDS each)
  feed   the masked table is the same kernel on the same bytes per point (a face of weight zero is a record nobody draws): no difference
         outside the arms' own run-to-run spread; the same for the fit loop against the parent commit
measured:""" % (mc.S, VIEWS, mc.S * VIEWS, 2 * mc.GRID * mc.GRID)


def mesh_sets(dev):
    """(unmasked, masked, masks, faces the pass itself hid): tools/mesh_cost.py's set and the same set rebuilt with the masks of its own
    (normalised) geometry, every third face's mask cleared on top."""
    from pdgn_amd.meshes import MeshSet, face_visibility
    plain = mc.meshes(dev)
    verts, faces, off = plain.verts.cpu().numpy(), plain.faces.cpu().numpy(), plain.face_off.cpu().numpy()
    mask = face_visibility(verts, faces, off, views=VIEWS, resolution=RES, device=dev)
    found = int((mask == 0).sum())
    mask[::3] = 0
    return plain, MeshSet.from_arrays(verts, faces, off, "shape_unit", visible=mask).to(dev), mask, found


def pass_child(calls):
    import torch
    from pdgn_amd.meshes import face_visibility
    dev = torch.device("cuda:0")
    plain = mc.meshes(dev)
    verts, faces, off = plain.verts.cpu().numpy(), plain.faces.cpu().numpy(), plain.face_off.cpu().numpy()
    for _ in range(calls):
        mask = face_visibility(verts, faces, off, views=VIEWS, resolution=RES, device=dev)
    print(json.dumps({"faces": int(mask.shape[0]), "hidden": int((mask == 0).sum())}))


def traced(calls):
    """((launches, median ms, min, max) of visible_kernel, the child's JSON line) under rocprofv3."""
    out = tempfile.mkdtemp(prefix="visible_cost_trace_")
    try:
        said = mc.step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
                        "--pass-child", "--iters", str(calls)], ROOT, 600)
        path = max(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
        v = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in csv.DictReader(open(path)) if "visible_kernel" in r["Kernel_Name"]]
        return (len(v), statistics.median(v), min(v), max(v)), json.loads([l for l in said.splitlines() if l.startswith("{")][0])
    finally:
        shutil.rmtree(out, ignore_errors=True)


def feed_child(rounds, launches=200):
    """Both tables in this process, alternating -> one JSON line {arm: [us per launch, per round]}."""
    import torch
    from pdgn_amd import data
    dev = torch.device("cuda:0")
    plain, masked, mask, found = mesh_sets(dev)
    feeders = {"unmasked": data.MeshFeeder(plain, mc.B, mc.SIZES, seed=9999, num_point=mc.N),
               "masked": data.MeshFeeder(masked, mc.B, mc.SIZES, seed=9999, num_point=mc.N)}
    res = {k: [] for k in feeders}
    for r in range(rounds + 1):                                  # (round 0 warms up)
        for arm in (sorted(feeders) if r % 2 else sorted(feeders)[::-1]):
            f = feeders[arm]
            reals, z1, z2 = f.buffers()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(launches):
                f.fill(1 + i // f.batches_per_epoch, i % f.batches_per_epoch, reals, z1, z2)
            e1.record()
            torch.cuda.synchronize()
            if r:
                res[arm].append(e0.elapsed_time(e1) * 1e3 / launches)
    print(json.dumps({"us": res, "hidden": int((mask == 0).sum()), "found": found, "faces": int(mask.shape[0])}))


def fit_child(arm, iters):
    """tools/mesh_cost.py's fit child on this tree's unmasked or masked set."""
    import torch
    from pdgn_amd import data
    dev = torch.device("cuda:0")
    plain, masked = mesh_sets(dev)[:2]
    mc.feeder_of = lambda _arm, _dev: data.MeshFeeder(masked if arm == "masked" else plain, mc.B, mc.SIZES, seed=9999, num_point=mc.N)
    mc.fit_child(arm, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=60, help="iterations per fit child (calls of the pass child)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its fit loop on the same meshes as a third arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_visible.txt"), help="results file ('' for none)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--no-fit", action="store_true", help="skip the fit arms")
    ap.add_argument("--pass-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--feed-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--fit-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.pass_child:
        return pass_child(args.iters)
    if args.feed_child:
        return feed_child(args.rounds)
    if args.fit_child:
        return fit_child(args.fit_child, args.iters)
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
    if not args.no_trace:
        (n, med, lo, hi), rec = traced(3)
        say("pass alone, %d meshes of %d faces, %d views at R = %d, rocprofv3 --kernel-trace --stats, one process: visible_kernel %d launches, "
            "median %.1f ms, min %.1f, max %.1f; %d of %d faces hidden" % (mc.S, 2 * mc.GRID * mc.GRID, VIEWS, RES, n, med, lo, hi, rec["hidden"], rec["faces"]))
    out = mc.step([sys.executable, os.path.abspath(__file__), "--feed-child", "--rounds", str(args.rounds)], ROOT, 600)
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][0])
    for arm, v in sorted(rec["us"].items()):
        say("pdgn_feed_batch_mesh, %-8s table: us per launch mean %.2f min %.2f max %.2f spread %.2f over %d rounds x 200 launches, one process"
            % (arm, sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v)))
    say("  (%d of %d faces have weight zero in the masked table: %d hidden by the pass, every third face cleared on top)" % (rec["hidden"], rec["faces"], rec["found"]))
    if args.no_fit:
        return
    arms = (["parent"] if args.parent else []) + ["unmasked", "masked"]
    res = {a: [] for a in arms}
    for r in range(args.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            if arm == "parent":                                  # the parent's own tool, its own mesh arm: the same meshes
                cwd = os.path.abspath(args.parent)
                cmd = [sys.executable, os.path.join(cwd, "tools", "mesh_cost.py"), "--fit-child", "mesh", "--iters", str(args.iters)]
            else:
                cwd, cmd = ROOT, [sys.executable, os.path.abspath(__file__), "--fit-child", arm, "--iters", str(args.iters)]
            line = [l for l in mc.step(cmd, cwd, 300).splitlines() if l.startswith("{")]
            if not line or not json.loads(line[0])["finite"]:
                raise SystemExit("fit child %s: no finite result, stopping" % arm)
            res[arm].append(json.loads(line[0])["ms_per_iter"])
            print("round %d %-8s %.3f ms/iter" % (r, arm, res[arm][-1]), flush=True)
    for arm in arms:
        v = res[arm]
        say("fit loop, %-8s ms/iter mean %.3f min %.3f max %.3f spread %.3f over %d rounds x %d iterations"
            % (arm, sum(v) / len(v), min(v), max(v), max(v) - min(v), len(v), args.iters))
    mean = {a: sum(res[a]) / len(res[a]) for a in arms}
    say("masked - unmasked: %+.3f ms/iter" % (mean["masked"] - mean["unmasked"]))
    if args.parent:
        spread = max(res["parent"]) - min(res["parent"])
        say("unmasked - parent: %+.3f ms/iter; masked - parent: %+.3f ms/iter; the parent arm's run-to-run spread: %.3f ms"
            % (mean["unmasked"] - mean["parent"], mean["masked"] - mean["parent"], spread))


if __name__ == "__main__":
    main()
