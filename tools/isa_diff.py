#!/usr/bin/env python3
"""Machine code of the library's kernels at two revisions, kernel by kernel: python3 tools/isa_diff.py [OLD [NEW]]
(default OLD = HEAD~1, NEW = the working tree).  Every csrc/*.hip of either revision is compiled device-only for gfx950 with
the build's flags (pdgn_amd/build.py), disassembled with llvm-objdump, and split per kernel symbol; a kernel present at both
revisions must have the same instructions (addresses and the symbol's own offsets stripped).  Prints one line per source
file and a summary: kernels equal / changed / only at one revision.  Host-only: no GPU."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pdgn_amd import build  # noqa: E402

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
OBJDUMP = os.path.join(ROCM, "llvm", "bin", "llvm-objdump")


def export(rev, dst):
    """csrc/ and include/ of `rev` (None: the working tree) into dst."""
    if rev is None:                                              # (the sources include ../../include/pdgn_hip.h: keep the layout)
        os.makedirs(os.path.join(dst, "pdgn_amd"))
        subprocess.check_call(["cp", "-r", os.path.join(ROOT, "pdgn_amd", "csrc"), os.path.join(dst, "pdgn_amd")])
        subprocess.check_call(["cp", "-r", os.path.join(ROOT, "include"), dst])
        return
    for sub in ("pdgn_amd/csrc", "include"):
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, sub], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)


def kernels(src, out):
    name = os.path.basename(src)
    cmd = ([os.path.join(ROCM, "bin", "hipcc")] + build.FLAGS + build.EXTRA_FLAGS.get(name, [])
           + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", out])
    subprocess.run(cmd, check=True, capture_output=True)
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", out], check=True, capture_output=True,
                          text=True).stdout
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^\s*[0-9a-f]*\s*<(.+)>:$", line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif cur and line.strip() and not line.startswith("Disassembly"):
            funcs[cur].append(re.sub(r"<[^>]*>|//.*$", "", line).strip())
    for body in funcs.values():                                      # "...": the zero bytes llvm-objdump skips between a function's end and
        while body and body[-1] == "...":                            # the next one's aligned start -- there or not by the function's place
            body.pop()                                               # in the section (the last one has none), not by its code
    return funcs


def main():
    old = sys.argv[1] if len(sys.argv) > 1 else "HEAD~1"
    new = sys.argv[2] if len(sys.argv) > 2 else None
    with tempfile.TemporaryDirectory() as tmp:
        trees = {}
        for tag, rev in (("old", old), ("new", new)):
            d = os.path.join(tmp, tag)
            os.makedirs(d)
            export(rev, d)
            trees[tag] = d
        names = sorted(set(os.listdir(os.path.join(trees["old"], "pdgn_amd", "csrc"))) | set(os.listdir(os.path.join(trees["new"], "pdgn_amd", "csrc"))))
        names = [n for n in names if n.endswith(".hip")]
        jobs = [(tag, n) for n in names for tag in trees if os.path.exists(os.path.join(trees[tag], "pdgn_amd", "csrc", n))]
        with ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", "8"))) as ex:
            res = dict(zip(jobs, ex.map(lambda j: kernels(os.path.join(trees[j[0]], "pdgn_amd", "csrc", j[1]),
                                                          os.path.join(tmp, j[0] + "_" + j[1] + ".co")), jobs)))
    equal = changed = only = 0
    for n in names:
        a, b = res.get(("old", n), {}), res.get(("new", n), {})
        same = [k for k in a if k in b and a[k] == b[k]]
        diff = [k for k in a if k in b and a[k] != b[k]]
        solo = sorted(set(a) ^ set(b))
        equal, changed, only = equal + len(same), changed + len(diff), only + len(solo)
        print("%-20s equal %4d  changed %3d  only at one revision %3d%s" % (n, len(same), len(diff), len(solo),
                                                                           ("  CHANGED: " + " ".join(diff)) if diff else ""))
    print("kernels: equal %d, changed %d, only at one revision %d (%s -> %s)" % (equal, changed, only, old, new or "working tree"))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
