"""CPU: the case table of tests/test_gpu_wgs_adjoint.py against the launcher's predicates (wgs_mirror.regime), the planted
in-degrees against the load groups read from csrc/wgs.hip, and the exactness guard on every entry (it rejects none)."""
import numpy as np
import pytest

import wgs_adjoint_cases as ac
import wgs_mirror as wm


def test_table_reaches_the_task_mapped_kernels_at_both_chunk_widths():
    ac.check_table()
    ac.check_table(cw=32)
    assert {w for c in ac.CASES for w in c.wants} == {"csr_xcd6", "csr_xcd10", "csr_xcd_rt"}
    for c in ac.CASES:                                            # task counts that are no multiple of 8
        assert wm.geometry("csr", c.b, c.n, c.k, c.ldy, c.specs[0])["ntasks"] % 8, c
    assert any(wm.geometry("csr", c.b, c.n, c.k, c.ldy, c.specs[0])["nchunk"] * 64 > c.specs[0][2] // 4 for c in ac.CASES)


def test_load_groups_meet_the_depths_the_kernel_was_built_for():
    assert ac.BU >= 4 and ac.BU1 >= 8 and 64 % ac.BU == 0 and 64 % ac.BU1 == 0


@pytest.mark.parametrize("b,n", [(3, 128), (9, 128), (3, 160)])
def test_graph_holds_the_planted_in_degrees(b, n):
    idx = ac.graph(b, n)
    assert idx.min() >= 0 and idx.max() < n
    deg = ac.in_degrees(idx)
    for i, d in enumerate(ac.DEGREES):
        assert (deg[:, ac.FIRST + i] == d).all(), (i, d)
    assert (deg[:, ac.HUB_SLOT] == 100).all() and (deg[:, ac.HUB_OUT] == 120).all()
    for s in range(b):
        q, slot = np.nonzero(idx[s] == ac.HUB_SLOT)
        assert set(slot) == {2}
        q, slot = np.nonzero(idx[s] == ac.HUB_OUT)
        assert set(slot) == {8, 9}
        for i, d in enumerate(ac.DEGREES[-3:]):                   # the long lists mix slots
            assert len(set(np.nonzero(idx[s] == ac.FIRST + 7 + i)[1])) > 4
    assert b == 1 or not np.array_equal(idx[0], idx[1])


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_guard_accepts_every_entry_and_the_hubs_show(case):
    ref = ac.reference(case)                                      # (wgs_mirror.assert_exact inside: raises where a sum is inexact)
    assert ref["worst"] < 2.0 ** 24
    spec = case.specs[0]
    T, P, C, off, offc = spec
    empty = ac.empty_taps(spec)
    assert empty, case.name
    for t in empty:
        assert not ref["dY"][:, ac.HUB_OUT, off + t * C: off + (t + 1) * C].any()
    assert ref["dY"][:, ac.HUB_OUT, off + (T - 1) * C: off + T * C].any() or T <= 8 and P == 1
    assert not ref["dY"][:, ac.FIRST, off: off + T * C].any()     # in-degree 0
    assert ref["dY"][:, ac.FIRST + 9, off: off + T * C].any()
    np.testing.assert_array_equal(np.diff(ref["rowptr"], axis=1), ac.in_degrees(ref["idx"]))
