"""csrc/wgs.hip in every dispatch regime, bit for bit: the forward gather-sum (scalar, flat float4, both task-mapped kernels), the
same with the BatchNorm partial statistics (both mappings, the zeroed spare rows), the transposed graph, the CSR adjoint (the small
kernel and the three task-mapped ones, tilings of two and three specs, the row maxima) and the atomic adjoint -- against
tests/wgs_mirror.py (float64 numpy) on dyadic inputs whose every partial sum is a float32 (tests/wgs_cases.py runs the exactness guard
on each case before anything is compared; tests/test_wgs_mirror_host.py checks mirror, guard and case table on the host).  Every
output is a slice of a sentinel-filled allocation (tests/wgs_worker.py): nothing beside it may change, nothing inside it may be left
out.  Every comparison is an equality of bit patterns."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wgs_cases as wc
import wgs_mirror as wm
import wgs_worker as ww
from wgs_worker import bits, dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _name(case):
    return case.name if hasattr(case, "name") else "-".join(map(str, case))


def check_partials(part, ref):
    """Every partial row finite; their float64 column totals are the mirror's exact sums."""
    C = ref["out"].shape[-1]
    assert np.isfinite(part).all(), "a partial row is not finite"
    got = part.astype(np.float64).sum(0)
    np.testing.assert_array_equal(got[:C], ref["total"])
    np.testing.assert_array_equal(got[C:], ref["total_sq"])


# ---------------------------------------------------------------------------- A. forward
@pytest.mark.parametrize("case", wc.FORWARD, ids=_name)
def test_forward_equals_the_mirror_bit_for_bit(case):
    ref = wc.forward_reference(case)
    np.testing.assert_array_equal(ww.device_forward(case, ref), bits(ref["out"]))


# ---------------------------------------------------------------------------- B. forward with statistics
@pytest.mark.parametrize("case", wc.STATS, ids=_name)
def test_statistics_epilogue_output_and_partial_rows_exact(case):
    ref = wc.forward_reference(case)
    out, part = ww.device_stats(case, ref)
    np.testing.assert_array_equal(out, bits(ref["out"]))
    check_partials(part, ref)


@pytest.mark.parametrize("case", wc.STATS_REFUSED, ids=_name)
def test_statistics_entry_point_refuses_what_it_documents(case):
    rc, untouched = ww.device_stats_refused(case)
    assert rc == ww.INVALID and untouched


# ---------------------------------------------------------------------------- C. transposed graph
@pytest.mark.parametrize("case", wc.TRANSPOSE, ids=_name)
def test_transposed_graph_rowptr_and_records(case):
    ref = wc.graph_reference(case)
    rowptr, edges = ww.device_transpose(ref["idx"])
    rowptr, edges = rowptr.cpu().numpy(), edges.cpu().numpy()
    np.testing.assert_array_equal(rowptr, ref["rowptr"])
    np.testing.assert_array_equal(wm.sort_rows(rowptr, edges), ref["records"])
    if case.kind == "allone":                                     # one row holds all n * k edges
        assert (np.diff(rowptr, axis=1).max(axis=1) == case.n * case.k).all()


@pytest.mark.parametrize("case", wc.TRANSPOSE_REFUSED, ids=_name)
def test_transposed_graph_refuses_a_slot_count_the_record_cannot_hold(case):
    from pdgn_amd import _lib
    L, ptr = _lib.lib(), _lib.ptr
    idx = torch.zeros(4096, dtype=torch.int32, device="cuda")
    rowptr, edges, scratch = ww.Banded(4096, False), ww.Banded(4096, False), ww.Banded(4096, False)
    rc = L.pdgn_knn_graph_transpose(case.b, case.n, case.k, ptr(idx), ptr(rowptr.t), ptr(edges.t), ptr(scratch.t), _lib.stream_of(idx))
    torch.cuda.synchronize()
    assert rc == ww.INVALID
    for buf in (rowptr, edges, scratch):
        assert buf.sentinels_left() == 4096 and buf.margins_intact()


# ---------------------------------------------------------------------------- D. adjoints
@pytest.mark.parametrize("case", wc.ADJOINT, ids=_name)
def test_csr_adjoint_writes_every_element_once_and_agrees_with_the_atomic_one(case):
    """dY starts as NaN and ends as the mirror's bits where a spec writes and as the NaN it was elsewhere; max_out (zero-filled by
    the first spec's launch alone) is the rows' maxima; a second run, and a run without max_out, give the same bytes; the atomic
    entry point, from zeros, gives the same bits in the covered columns and leaves the others zero."""
    ref = wc.adjoint_reference(case)
    rowptr, edges = ww.device_transpose(ref["idx"])
    np.testing.assert_array_equal(rowptr.cpu().numpy(), ref["rowptr"])
    want = ww.expected_dy_bits(case, ref)
    dY, mx = ww.device_csr(case, ref, rowptr, edges)
    np.testing.assert_array_equal(dY, want)
    np.testing.assert_array_equal(mx, ref["maxima"])
    again, mx2 = ww.device_csr(case, ref, rowptr, edges)
    assert np.array_equal(again, dY) and np.array_equal(mx2, mx)
    plain, none = ww.device_csr(case, ref, rowptr, edges, with_max=False)
    assert none is None and np.array_equal(plain, dY)
    atomic = ww.device_atomic(case, ref)
    cov = ref["covered"]
    np.testing.assert_array_equal(atomic[:, :, cov], dY[:, :, cov])
    assert not atomic[:, :, ~cov].any()


@pytest.mark.parametrize("case", wc.ATOMIC_ONLY, ids=_name)
def test_atomic_adjoint_exact_with_unaligned_specs_and_gaps(case):
    ref = wc.adjoint_reference(case)
    got = ww.device_atomic(case, ref)
    np.testing.assert_array_equal(got, bits(ref["dY"]))
    assert not got[:, :, ~ref["covered"]].any()
    assert got[:, wc.HUB].any() and not got[:, case.n - 2][:, np.concatenate([np.arange(s[3], s[3] + s[0] * s[2]) for s in case.specs])].any()


# ---------------------------------------------------------------------------- E. EdgeGatherSum end to end
@pytest.mark.parametrize("case", wc.END_TO_END, ids=_name)
def test_edge_gather_sum_outputs_and_gradients_exact(case):
    from pdgn_amd.deconv import EdgeGatherSum
    ref = wc.end_to_end_reference(case)
    Y, idx = dev(ref["Y"]).requires_grad_(True), dev(ref["idx"])
    packed = None
    if case.pitch:                                                # per-sample biases: column slices of one (b, pitch) tensor
        host = np.zeros((case.b, case.pitch), np.float32)
        o = 0
        for b_ in ref["biases"]:
            host[:, o:o + b_.shape[1]] = b_
            o += b_.shape[1]
        packed = dev(host).requires_grad_(True)
    biases, o = [], 0
    for kind, b_ in zip(case.biases, ref["biases"]):
        if kind == "sample":
            biases.append(packed[:, o:o + b_.shape[1]])
            assert biases[-1].stride(0) == case.pitch > b_.shape[1]
            o += b_.shape[1]
        else:
            biases.append(dev(b_).requires_grad_(True) if kind == "shared" else None)
    torch.empty(Y.numel() + 4096, device="cuda").fill_(float("nan"))      # leave the allocator's free blocks dirty
    outs = EdgeGatherSum.apply(Y, idx, case.specs, *biases)
    n_out = len(case.specs)
    for got, want in zip(outs[:n_out], ref["outs"]):
        np.testing.assert_array_equal(bits(got.detach().cpu().numpy()), bits(want))
    stats = [i for i, s in enumerate(case.specs) if len(s) > 5 and s[5]]
    for part, i in zip(outs[n_out:], stats):                      # the partial rows of a want_stats spec
        C = case.specs[i][2]
        gy = wm.cl_geometry(case.b * case.n * case.specs[i][1], C)[2]
        total, total_sq = wm.partial_totals(ref["outs"][i])
        rows = part[:gy * 2 * C].cpu().numpy().reshape(gy, 2 * C).astype(np.float64).sum(0)
        np.testing.assert_array_equal(rows[:C], total)
        np.testing.assert_array_equal(rows[C:], total_sq)
    torch.autograd.backward(outs[:n_out], [dev(d) for d in ref["douts"]])
    np.testing.assert_array_equal(bits(Y.grad.cpu().numpy()), bits(ref["dY"]))
    assert (getattr(idx, "_pdgn_csr", None) is not None) == case.tiled        # the atomic-free path exactly when the specs tile dY
    o = 0
    for kind, b_, want in zip(case.biases, biases, ref["dbias"]):
        if kind == "shared":
            np.testing.assert_array_equal(bits(b_.grad.cpu().numpy()), bits(want))
        elif kind == "sample":
            np.testing.assert_array_equal(bits(packed.grad[:, o:o + want.shape[1]].cpu().numpy()), bits(want))
            o += want.shape[1]
    if packed is not None:
        assert not packed.grad[:, o:].any()


def test_transposed_graph_is_rebuilt_for_another_index_tensor_of_equal_shape():
    from pdgn_amd.deconv import transposed_graph
    a = wc.graph_reference(wc.Graph(3, 1000, 10, "planted"))
    other = np.ascontiguousarray(a["idx"][:, ::-1, ::-1])         # the same shape, another graph
    assert not np.array_equal(other, a["idx"])
    want_rowptr, want_records = wm.transpose(other)
    ia, ib = dev(a["idx"]), dev(other)
    ra, ea = transposed_graph(ia)
    rb, eb = transposed_graph(ib)
    assert transposed_graph(ia)[0] is ra and rb is not ra         # memoised per tensor, not per shape
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ra.cpu().numpy(), a["rowptr"])
    np.testing.assert_array_equal(wm.sort_rows(ra.cpu().numpy(), ea.cpu().numpy()), a["records"])
    np.testing.assert_array_equal(rb.cpu().numpy(), want_rowptr)
    np.testing.assert_array_equal(wm.sort_rows(rb.cpu().numpy(), eb.cpu().numpy()), want_records)


# ---------------------------------------------------------------------------- F. the process-wide switches
@pytest.mark.parametrize("setting", wc.WORKER_SETTINGS, ids=lambda s: ",".join("%s=%s" % kv for kv in sorted(s.items())))
def test_kernel_instances_behind_the_switches_in_a_child_process(setting, tmp_path):
    """PDGN_WGS_XCD=0 sends every shape to the flat / BatchNorm-geometry / small kernels; PDGN_WGS_CW, _SCW and _BCW select the
    other chunk widths of the task-mapped ones.  The launchers read them once per process: a fresh child runs the reduced lists and
    hands its bits back; wgs_mirror.regime says which kernel each of them was."""
    xcd, cw = wc.switches(setting)
    for name in wc.WORKER_FORWARD:
        c = wc.by_name(wc.FORWARD, name)
        assert wm.regime("fwd", c.b, c.n, c.k, c.ldy, c.spec, c.bias, xcd=xcd, cw=cw["fwd"]) == (c.want if xcd else "fwd_flat4")
    for name in wc.WORKER_STATS:
        c = wc.by_name(wc.STATS, name)
        assert wm.regime("stats", c.b, c.n, c.k, c.ldy, c.spec, c.bias, xcd=xcd, cw=cw["stats"]) == (c.want if xcd else c.want.replace("xcd", "geom"))
    for name in wc.WORKER_ADJOINT:
        c = wc.by_name(wc.ADJOINT, name)
        assert tuple(wm.regime("csr", c.b, c.n, c.k, c.ldy, s, xcd=xcd, cw=cw["csr"]) for s in c.specs) == (c.wants if xcd else ("csr_small",) * len(c.specs))
    out = str(tmp_path / "child.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PDGN_WGS_")}
    env.update(setting, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wgs_worker.py"), out], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=300)
    said = "wgs worker ok: " + " ".join("%s=%s" % kv for kv in sorted(setting.items()))
    assert run.returncode == 0 and said in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
    got = np.load(out)
    seen = set()
    for name in wc.WORKER_FORWARD:
        ref = wc.forward_reference(wc.by_name(wc.FORWARD, name))
        np.testing.assert_array_equal(got["fwd/" + name], bits(ref["out"]), err_msg=name)
        seen.add("fwd/" + name)
    for name in wc.WORKER_STATS:
        ref = wc.forward_reference(wc.by_name(wc.STATS, name))
        np.testing.assert_array_equal(got["stats/%s/out" % name], bits(ref["out"]), err_msg=name)
        check_partials(got["stats/%s/part" % name], ref)
        seen.update(("stats/%s/out" % name, "stats/%s/part" % name))
    for name in wc.WORKER_ADJOINT:
        case = wc.by_name(wc.ADJOINT, name)
        ref = wc.adjoint_reference(case)
        np.testing.assert_array_equal(got["csr/%s/dY" % name], ww.expected_dy_bits(case, ref), err_msg=name)
        np.testing.assert_array_equal(got["csr/%s/max" % name], ref["maxima"], err_msg=name)
        seen.update(("csr/%s/dY" % name, "csr/%s/max" % name))
    assert seen == set(got.files)
