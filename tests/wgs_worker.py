"""The window gather-sum family (csrc/wgs.hip) straight through the C ABI, every output a slice of a larger, sentinel-filled
allocation: shared by tests/test_gpu_wgs.py and its child processes (python tests/wgs_worker.py OUT.npz, started with PDGN_WGS_XCD,
PDGN_WGS_CW, PDGN_WGS_SCW or PDGN_WGS_BCW in the environment -- the launchers read them once per process -- so that the kernel
instances behind those switches run the reduced lists of tests/wgs_cases.py; the parent compares what comes back with the mirror)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import wgs_cases as wc  # noqa: E402
import wgs_mirror as wm  # noqa: E402

SENT_INT = 0x5A5A5A5A            # what integer outputs hold before a call
SENT_NAN = 0x7FC5A5A5            # ... and float outputs: a NaN, so a sum that started from it, or a hole, cannot pass for a result
MARGIN = 64                      # 4-byte elements in front of and behind every output: 256 bytes, alignment unchanged
INVALID = -1


class Banded:
    """`numel` 4-byte elements with MARGIN sentinel elements on either side, one allocation."""

    def __init__(self, numel, floats, interior=None):
        self.numel, self.sentinel = int(numel), SENT_NAN if floats else SENT_INT
        self.raw = torch.full((self.numel + 2 * MARGIN,), self.sentinel, dtype=torch.int32, device="cuda")
        inner = self.raw[MARGIN:MARGIN + self.numel]
        self.ints = inner
        self.t = inner.view(torch.float32) if floats else inner
        assert self.numel == 0 or self.t.data_ptr() % 256 == 0
        if interior is not None:
            self.t.fill_(interior)

    def margins_intact(self):
        return bool((self.raw[:MARGIN] == self.sentinel).all()) and bool((self.raw[MARGIN + self.numel:] == self.sentinel).all())

    def sentinels_left(self, lo=0, hi=None):
        """How many elements of [lo, hi) still hold the sentinel's bits."""
        return int((self.ints[lo:hi] == self.sentinel).sum())

    def bits(self):
        return self.ints.cpu().numpy().view(np.uint32)


def bits(a):
    """The float32 bit patterns of an array (float64 expectations are rounded first: they are float32 values, the guard saw to it)."""
    return np.ascontiguousarray(np.asarray(a).astype(np.float32)).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                   # (a copy: the cached references are read-only)


def _api():
    from pdgn_amd import _lib
    return _lib.lib(), _lib.ptr, _lib.stream_of(torch.empty(1, device="cuda"))


def _sync(rc, what):
    assert rc == 0, "%s returned %d" % (what, rc)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- forward, statistics
def device_forward(case, ref):
    """pdgn_window_gather_sum -> out (b, n, P, C) as uint32 bit patterns."""
    L, ptr, stream = _api()
    T, P, C, off, offc = case.spec
    Y, idx = dev(ref["Y"]), dev(ref["idx"])
    bias = dev(ref["bias"]) if ref["bias"] is not None else None
    out = Banded(case.b * case.n * P * C, True)
    _sync(L.pdgn_window_gather_sum(case.b, case.n, case.k, case.ldy, T, P, C, off, offc, ptr(Y), ptr(idx), ptr(bias), ref["bstride"],
                                   ptr(out.t), stream), "pdgn_window_gather_sum")
    assert out.margins_intact(), "pdgn_window_gather_sum wrote outside out"
    assert out.sentinels_left() == 0, "pdgn_window_gather_sum left %d elements of out unwritten" % out.sentinels_left()
    return out.bits().reshape(case.b, case.n, P, C)


def device_stats(case, ref):
    """pdgn_window_gather_sum_stats -> out bits (b, n, P, C), the gy partial rows (gy, 2C) float32.  The scratch has
    pdgn_bn_scratch_floats floats: the partial rows, then 2C floats that belong to the BatchNorm backward and stay untouched."""
    L, ptr, stream = _api()
    T, P, C, off, offc = case.spec
    Y, idx = dev(ref["Y"]), dev(ref["idx"])
    bias = dev(ref["bias"]) if ref["bias"] is not None else None
    rows = case.b * case.n * P
    floats = L.pdgn_bn_scratch_floats(rows, C)
    gy = wm.cl_geometry(rows, C)[2]
    assert floats == gy * 2 * C + 2 * C
    out, scr = Banded(rows * C, True), Banded(floats, True)
    _sync(L.pdgn_window_gather_sum_stats(case.b, case.n, case.k, case.ldy, T, P, C, off, offc, ptr(Y), ptr(idx), ptr(bias), ref["bstride"],
                                         ptr(out.t), ptr(scr.t), stream), "pdgn_window_gather_sum_stats")
    assert out.margins_intact() and scr.margins_intact(), "pdgn_window_gather_sum_stats wrote outside out / scratch"
    assert out.sentinels_left() == 0
    assert scr.sentinels_left(gy * 2 * C) == 2 * C, "the scratch behind the partial rows was written"
    return out.bits().reshape(case.b, case.n, P, C), scr.t[:gy * 2 * C].cpu().numpy().reshape(gy, 2 * C)


def device_stats_refused(case):
    """A refused argument list: PDGN_ERR_INVALID, and neither out nor the scratch is touched."""
    L, ptr, stream = _api()
    T, P, C, off, offc = case.spec
    Y = torch.zeros(max(1, case.b) * case.n * case.ldy, device="cuda")
    idx = torch.zeros(max(1, case.b) * case.n * case.k, dtype=torch.int32, device="cuda")
    bias = torch.zeros(max(1, case.b) * 16, device="cuda") if case.bias is not None else None
    out, scr = Banded(1024, True), Banded(1024, True)
    rc = L.pdgn_window_gather_sum_stats(case.b, case.n, case.k, case.ldy, T, P, C, off, offc, ptr(Y), ptr(idx), ptr(bias),
                                        case.bias if isinstance(case.bias, int) else 0, ptr(out.t), ptr(scr.t), stream)
    torch.cuda.synchronize()
    return rc, out.sentinels_left() == 1024 and scr.sentinels_left() == 1024 and out.margins_intact() and scr.margins_intact()


# ---------------------------------------------------------------------------- transposed graph, adjoints
def device_transpose(idx):
    """pdgn_knn_graph_transpose on idx (b, n, k) int32 (numpy) -> rowptr (b, n + 1), edges (b, n * k) int32, still on the device."""
    L, ptr, stream = _api()
    b, n, k = idx.shape
    d = dev(idx)
    rowptr, edges, scratch = Banded(b * (n + 1), False), Banded(b * n * k, False), Banded(2 * b * n, False)
    _sync(L.pdgn_knn_graph_transpose(b, n, k, ptr(d), ptr(rowptr.t), ptr(edges.t), ptr(scratch.t), stream), "pdgn_knn_graph_transpose")
    assert rowptr.margins_intact() and edges.margins_intact() and scratch.margins_intact(), "pdgn_knn_graph_transpose wrote outside its outputs"
    return rowptr.t.view(b, n + 1), edges.t.view(b, n * k)


def device_csr(case, ref, rowptr, edges, with_max=True):
    """Every spec of the case through pdgn_window_gather_sum_backward_csr into ONE dY that starts as NaN (max_init = 1 on the first
    spec, 0 after) -> dY bits (b, n, ldy), max_out bits (b, n) | None."""
    L, ptr, stream = _api()
    dY = Banded(case.b * case.n * case.ldy, True)
    mx = Banded(case.b * case.n, False) if with_max else None
    for i, (spec, dout) in enumerate(zip(case.specs, ref["douts"])):
        T, P, C, off, offc = spec
        d = dev(dout)
        _sync(L.pdgn_window_gather_sum_backward_csr(case.b, case.n, case.k, case.ldy, T, P, C, off, offc, ptr(d), ptr(rowptr), ptr(edges),
                                                    ptr(dY.t), ptr(mx.t) if with_max else None, 1 if i == 0 else 0, stream),
              "pdgn_window_gather_sum_backward_csr")
    assert dY.margins_intact() and (mx is None or mx.margins_intact()), "pdgn_window_gather_sum_backward_csr wrote outside dY / max_out"
    return dY.bits().reshape(case.b, case.n, case.ldy), (mx.bits().reshape(case.b, case.n) if with_max else None)


def device_atomic(case, ref):
    """Every spec through pdgn_window_gather_sum_backward into one dY that starts at zero -> dY bits (b, n, ldy)."""
    L, ptr, stream = _api()
    dY = Banded(case.b * case.n * case.ldy, True, interior=0.0)
    idx = dev(ref["idx"])
    for spec, dout in zip(case.specs, ref["douts"]):
        T, P, C, off, offc = spec
        d = dev(dout)
        _sync(L.pdgn_window_gather_sum_backward(case.b, case.n, case.k, case.ldy, T, P, C, off, offc, ptr(d), ptr(idx), ptr(dY.t), stream),
              "pdgn_window_gather_sum_backward")
    assert dY.margins_intact(), "pdgn_window_gather_sum_backward wrote outside dY"
    return dY.bits().reshape(case.b, case.n, case.ldy)


def expected_dy_bits(case, ref):
    """The mirror's dY as bit patterns, the NaN sentinel in the columns no spec writes (what a CSR run must leave there)."""
    want = bits(ref["dY"])
    want[:, :, ~ref["covered"]] = SENT_NAN
    return want


def run_reduced_lists():
    """What a child process runs: {name: array} of every output, as bit patterns (float32 for the partial rows)."""
    res = {}
    for name in wc.WORKER_FORWARD:
        case = wc.by_name(wc.FORWARD, name)
        res["fwd/" + name] = device_forward(case, wc.forward_reference(case))
    for name in wc.WORKER_STATS:
        case = wc.by_name(wc.STATS, name)
        res["stats/" + name + "/out"], res["stats/" + name + "/part"] = device_stats(case, wc.forward_reference(case))
    for name in wc.WORKER_ADJOINT:
        case = wc.by_name(wc.ADJOINT, name)
        ref = wc.adjoint_reference(case)
        rowptr, edges = device_transpose(ref["idx"])
        res["csr/" + name + "/dY"], res["csr/" + name + "/max"] = device_csr(case, ref, rowptr, edges)
    return res


if __name__ == "__main__":
    np.savez(sys.argv[1], **run_reduced_lists())
    print("wgs worker ok: " + " ".join("%s=%s" % (v, os.environ[v]) for v in sorted(os.environ) if v.startswith("PDGN_WGS_")))
