"""Child process of tests/test_gpu_wgs_adjoint.py (python tests/wgs_adjoint_worker.py OUT.npz, started with PDGN_WGS_BCW in the
environment: the launcher reads it once per process): every case of tests/wgs_adjoint_cases.py through the CSR entry point, the bits
handed back."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import wgs_adjoint_cases as ac  # noqa: E402
import wgs_worker as ww  # noqa: E402

if __name__ == "__main__":
    res = {}
    for case in ac.CASES:
        ref = ac.reference(case)
        rowptr, edges = ww.device_transpose(ref["idx"])
        res[case.name + "/dY"], res[case.name + "/max"] = ww.device_csr(case, ref, rowptr, edges)
    np.savez(sys.argv[1], **res)
    print("wgs adjoint worker ok: " + " ".join("%s=%s" % (v, os.environ[v]) for v in sorted(os.environ) if v.startswith("PDGN_WGS_")))
