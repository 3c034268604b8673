"""The task-mapped CSR adjoint (csrc/wgs.hip, wgs_bwd_csr_xcd_kernel) where its chunk-width-64 body can go wrong: source points
whose in-degree is 0, 1, odd, exactly a load group and one more (WGS_BU, WGS_BU1: read from the source by tests/wgs_adjoint_cases.py),
exactly one wave-wide record load, one more, and a third trip (64, 65, 130); a hub all of whose records carry one slot; a hub whose
records lie outside some taps' windows (those taps are +0.0); 44 column groups (lanes past CV); task counts that are no multiple of
8; max_out absent, zero-filled by the launch, and merged into a pre-filled array; the edge-lane body behind PDGN_WGS_BCW=32
in a child process.  The method is that of tests/test_gpu_wgs.py: C ABI
into NaN / 0x5A5A5A5A banded allocations, quarter-step inputs behind the mirror's exactness guard (it rejects none of the entries:
tests/test_wgs_adjoint_host.py), equality of bit patterns."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wgs_adjoint_cases as ac
import wgs_worker as ww

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = list(range(ac.FIRST, ac.FIRST + len(ac.DEGREES))) + [ac.HUB_SLOT, ac.HUB_OUT]


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_adjoint_bits_untouched_columns_and_row_maxima(case):
    ref = ac.reference(case)
    rowptr, edges = ww.device_transpose(ref["idx"])
    np.testing.assert_array_equal(rowptr.cpu().numpy(), ref["rowptr"])
    want = ww.expected_dy_bits(case, ref)
    dY, mx = ww.device_csr(case, ref, rowptr, edges)                 # max_init = 1 on a sentinel-filled array
    for j in PLANTED:                                                # the planted rows first: a failure names the in-degree
        np.testing.assert_array_equal(dY[:, j], want[:, j], err_msg="source point %d" % j)
    np.testing.assert_array_equal(dY, want)
    np.testing.assert_array_equal(mx, ref["maxima"])
    T, P, C, off, offc = case.specs[0]
    for t in ac.empty_taps(case.specs[0]):                           # +0.0, not -0.0, not the NaN it was
        assert not dY[:, ac.HUB_OUT, off + t * C: off + (t + 1) * C].any()
    plain, none = ww.device_csr(case, ref, rowptr, edges, with_max=False)     # max_out NULL
    assert none is None and np.array_equal(plain, dY)


@pytest.mark.parametrize("name", ["T10_P1_C256_b3", "T6_P5_C512_b3"])
def test_max_out_is_merged_into_a_prefilled_array_when_max_init_is_0(name):
    (case,) = [c for c in ac.CASES if c.name == name]
    ref = ac.reference(case)
    rowptr, edges = ww.device_transpose(ref["idx"])
    L, ptr, stream = ww._api()
    T, P, C, off, offc = case.specs[0]
    pre = np.where(np.arange(case.b * case.n) % 2 == 0, 0x7F000000, 0).astype(np.uint32).reshape(case.b, case.n)   # 2^127 / 0
    dY, mx = ww.Banded(case.b * case.n * case.ldy, True), ww.Banded(case.b * case.n, False)
    mx.t.copy_(torch.from_numpy(pre.view(np.int32).reshape(-1)))
    d = ww.dev(ref["douts"][0])
    ww._sync(L.pdgn_window_gather_sum_backward_csr(case.b, case.n, case.k, case.ldy, T, P, C, off, offc, ptr(d), ptr(rowptr), ptr(edges),
                                                   ptr(dY.t), ptr(mx.t), 0, stream), "pdgn_window_gather_sum_backward_csr")
    assert dY.margins_intact() and mx.margins_intact()
    np.testing.assert_array_equal(dY.bits().reshape(case.b, case.n, case.ldy), ww.expected_dy_bits(case, ref))
    np.testing.assert_array_equal(mx.bits().reshape(case.b, case.n), np.maximum(pre, ref["maxima"]))


def test_the_edge_lane_body_behind_the_chunk_width_switch_in_a_child_process(tmp_path):
    """PDGN_WGS_BCW=32 keeps the narrower widths' body (two edge lanes per column): the same cases, the same bits.  The launcher
    reads the switch once per process."""
    setting = {"PDGN_WGS_BCW": "32"}
    ac.check_table(cw=32)
    out = str(tmp_path / "child.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PDGN_WGS_")}
    env.update(setting, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wgs_adjoint_worker.py"), out], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    said = "wgs adjoint worker ok: " + " ".join("%s=%s" % kv for kv in sorted(setting.items()))
    assert run.returncode == 0 and said in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
    got = np.load(out)
    for case in ac.CASES:
        ref = ac.reference(case)
        np.testing.assert_array_equal(got[case.name + "/dY"], ww.expected_dy_bits(case, ref), err_msg=case.name)
        np.testing.assert_array_equal(got[case.name + "/max"], ref["maxima"], err_msg=case.name)
    assert set(got.files) == {c.name + s for c in ac.CASES for s in ("/dY", "/max")}
