"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/pdgn_hip.h
declares; the product refuses to run without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(pdgn_\w+)\s*\(", text)))


def test_library_builds_and_exports_every_declared_symbol():
    from pdgn_amd import build
    so = build.build()
    handle = ctypes.CDLL(so)
    names = declared_symbols()
    assert len(names) >= 13
    for name in names:
        assert hasattr(handle, name), "missing export: " + name
    from pdgn_amd import _lib
    assert handle.pdgn_abi_version() == _lib.ABI_VERSION


def test_no_cpu_fallback():
    from pdgn_amd import pointops
    from pdgn_amd._lib import PdgnHipError
    xyz = torch.zeros(1, 8, 3)
    with pytest.raises(PdgnHipError):
        pointops.knnquery(4, xyz, xyz)
    with pytest.raises(PdgnHipError):
        pointops.grouping(torch.zeros(1, 3, 8), torch.zeros(1, 2, 2, dtype=torch.int32))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "pdgn_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "/root/reference" not in src, f


def test_host_side_rules_of_the_contractions():
    """The host-only queries of the dense contractions (no device work: they run here): which arithmetic a call takes, which planes
    to make, how much workspace its tail wants -- the rules DESIGN.md section 4 states, and their mutual consistency."""
    from pdgn_amd import build
    L = ctypes.CDLL(build.build())
    L.pdgn_gemm_tail_workspace_floats.restype = ctypes.c_longlong
    L.pdgn_gemm_nt_ps_workspace_floats.restype = ctypes.c_longlong
    L.pdgn_gemm_tn_big_workspace_floats.restype = ctypes.c_longlong
    ll = ctypes.c_longlong
    old = L.pdgn_gemm_set_mode(2)
    try:
        # two parts for unsplit operands: the 256 x 128 tile, k >= 128, >= 20 GFLOP, <= 4.5 B to scan per kflop
        assert L.pdgn_gemm_two_part(ll(35840), 512, 5120, ll(35840 * 5120 * 4)) == 1
        assert L.pdgn_gemm_two_part(ll(35840), 12832, 128, ll(0)) == 1
        assert L.pdgn_gemm_two_part(ll(35840), 128, 12832, ll(35840 * 12832 * 4)) == 0       # 1.8 GB to scan for 118 GFLOP
        assert L.pdgn_gemm_two_part(ll(358400), 512, 64, ll(0)) == 0 and L.pdgn_gemm_two_part(ll(3000), 256, 8, ll(0)) == 0
        # ... for pre-split planes: from ~2 GFLOP on
        assert L.pdgn_gemm_two_part_planes(ll(17920), 256, 2560, ll(0)) == 1 and L.pdgn_gemm_two_part_planes(ll(17920), 6432, 64, ll(17920 * 64 * 4)) == 1
        assert L.pdgn_gemm_two_part_planes(ll(17920), 256, 2560, ll(17920 * 2560 * 4)) == 0 and L.pdgn_gemm_two_part_planes(ll(200), 256, 2560, ll(0)) == 0
        # workspaces: three-part planes = the unsplit call's; two-part planes = the 256 x 128 tile's; none with statistics
        for m, n, k in ((35840, 512, 5120), (17920, 256, 2560), (35840, 128, 12832), (4100, 132, 260)):
            assert L.pdgn_gemm_nt_ps_workspace_floats(ll(m), n, k, 3, 0) == L.pdgn_gemm_tail_workspace_floats(ll(m), n, k, 0)
            assert L.pdgn_gemm_nt_ps_workspace_floats(ll(m), n, k, 2, 1) == 0 and L.pdgn_gemm_tail_workspace_floats(ll(m), n, k, 1) == 0
            assert L.pdgn_gemm_nt_ps_workspace_floats(ll(m), n, k, 2, 0) % (256 * 128) == 0
        assert L.pdgn_gemm_nt_ps_workspace_floats(ll(35840), 128, 12832, 2, 0) > 0             # 140 tiles on 256 CUs: the flattened tail
        assert L.pdgn_gemm_tn_big_workspace_floats(ll(35840), 512, 5120) > 0 and L.pdgn_gemm_tn_big_workspace_floats(ll(35840), 512, 5120) % (256 * 128) == 0
        L.pdgn_gemm_set_mode(1)
        assert L.pdgn_gemm_two_part(ll(35840), 512, 5120, ll(0)) == 0 and L.pdgn_gemm_two_part_planes(ll(17920), 256, 2560, ll(0)) == 0
        L.pdgn_gemm_set_mode(0)
        assert L.pdgn_gemm_tail_workspace_floats(ll(35840), 512, 5120, 0) == 0 and L.pdgn_gemm_tn_big_workspace_floats(ll(35840), 512, 5120) == 0
    finally:
        L.pdgn_gemm_set_mode(old)


# ---------------------------------------------------------------------------- the header is the ABI: signatures derived from it
def _header_text():
    return open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()


def _package_sources():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "pdgn_amd")):
        for f in sorted(files):
            if f.endswith(".py"):
                yield os.path.relpath(os.path.join(dirpath, f), ROOT), open(os.path.join(dirpath, f)).read()


def test_every_prototype_is_parsed_and_applied_to_the_handle():
    from pdgn_amd import _lib, build
    build.build()
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    declared = re.findall(r"\b(pdgn_\w+)\s*\(", text)
    assert len(declared) == len(set(declared)) >= 141
    assert sorted(_lib.SIGNATURES) == sorted(declared)
    assert set(declared_symbols()) <= set(_lib.SIGNATURES)
    L = _lib.lib()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
        assert restype in (ctypes.c_int, ctypes.c_longlong), name
    # a few read by eye from the header: every kind of parameter the vocabulary has
    vp, i, ll, f, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double
    assert _lib.SIGNATURES["pdgn_abi_version"] == (i, ())
    assert _lib.SIGNATURES["pdgn_bn_scratch_floats"] == (ll, (ll, i))
    assert _lib.SIGNATURES["pdgn_det_workspace_ints"] == (ll, (i, i, ll))
    assert _lib.SIGNATURES["pdgn_gemm_two_part"] == (i, (ll, i, i, ll))
    assert _lib.SIGNATURES["pdgn_spin"] == (i, (ctypes.c_uint, vp))
    assert _lib.SIGNATURES["pdgn_scaled_sum"] == (i, (ll, vp, f, vp, vp))
    assert _lib.SIGNATURES["pdgn_ema_multi"] == (i, (i, vp, vp, vp, d, vp, vp))
    assert _lib.SIGNATURES["pdgn_sample_bias"] == (i, (i, i, i, vp, vp, vp, vp, vp, vp, vp, vp))
    assert _lib.SIGNATURES["pdgn_feed_batch"] == (i, (i,) * 6 + (vp, vp, ll, ctypes.c_ulonglong, ctypes.c_ulonglong, ll, f) + (vp,) * 7)


def test_every_entry_point_the_package_calls_is_declared():
    from pdgn_amd import _lib
    called = {}
    for path, src in _package_sources():
        for name in re.findall(r"\.\s*(pdgn_\w+)\b", src):
            called.setdefault(name, path)
    assert len(called) >= 100                                    # (the regex still finds the call sites)
    missing = {n: p for n, p in called.items() if n not in _lib.SIGNATURES}
    assert not missing, "called through the library but not declared in include/pdgn_hip.h: %s" % missing


def test_no_marshalling_at_the_call_sites():
    for path, src in _package_sources():
        if path == os.path.join("pdgn_amd", "_lib.py"):
            continue
        assert not re.search(r"\.restype\s*=", src), path
        assert not re.search(r"ctypes\.c_(longlong|float|double|int)\(", src), path
    lib_src = dict(_package_sources())[os.path.join("pdgn_amd", "_lib.py")]
    assert len(re.findall(r"\.restype\b", lib_src)) == 1         # the one loop over the header's prototypes


def test_plain_python_ints_are_not_truncated():
    """Through _lib.lib() a bare int reaches a `long long` parameter whole and a `long long` result comes back whole: the same
    answers as the wrapped calls of test_host_side_rules_of_the_contractions on a handle of its own."""
    from pdgn_amd import _lib, build
    W = ctypes.CDLL(build.build())                               # the wrapped way: restype and c_longlong by hand
    for name in ("pdgn_gemm_tail_workspace_floats", "pdgn_gemm_nt_ps_workspace_floats", "pdgn_gemm_tn_big_workspace_floats",
                 "pdgn_bn_scratch_floats", "pdgn_det_workspace_ints", "pdgn_emd_cost_temp_floats"):
        getattr(W, name).restype = ctypes.c_longlong
    ll = ctypes.c_longlong
    L = _lib.lib()
    old = L.pdgn_gemm_set_mode(2)                                # (one library image: the switch is shared by both handles)
    try:
        assert L.pdgn_gemm_tail_workspace_floats(35840, 128, 12832, 0) == W.pdgn_gemm_tail_workspace_floats(ll(35840), 128, 12832, 0)
        for m, n, k in ((35840, 512, 5120), (17920, 256, 2560), (35840, 128, 12832), (4100, 132, 260)):
            for ws in (0, 1):
                assert L.pdgn_gemm_tail_workspace_floats(m, n, k, ws) == W.pdgn_gemm_tail_workspace_floats(ll(m), n, k, ws)
                for parts in (2, 3):
                    assert L.pdgn_gemm_nt_ps_workspace_floats(m, n, k, parts, ws) == W.pdgn_gemm_nt_ps_workspace_floats(ll(m), n, k, parts, ws)
            assert L.pdgn_gemm_tn_big_workspace_floats(m, n, k) == W.pdgn_gemm_tn_big_workspace_floats(ll(m), n, k)
        assert L.pdgn_gemm_nt_ps_workspace_floats(35840, 128, 12832, 2, 0) > 0 and L.pdgn_gemm_tn_big_workspace_floats(35840, 512, 5120) > 0
        # a `long long` argument above 2^32: 1.8 GB to scan, and the low 32 bits alone (0) would say "nothing to scan"
        big = 35840 * 12832 * 4
        assert big < 2 ** 32 < 4 * big and (4 * big) % 2 ** 32 != 4 * big
        for scan in (0, big, 4 * big, 2 ** 32, 2 ** 32 + 1, 2 ** 40):
            for m, n, k in ((35840, 128, 12832), (35840, 512, 5120), (35840, 12832, 128)):
                assert L.pdgn_gemm_two_part(m, n, k, scan) == W.pdgn_gemm_two_part(ll(m), n, k, ll(scan)), (m, n, k, scan)
                assert L.pdgn_gemm_two_part_planes(m, n, k, scan) == W.pdgn_gemm_two_part_planes(ll(m), n, k, ll(scan)), (m, n, k, scan)
        assert L.pdgn_gemm_two_part(35840, 512, 5120, 0) == 1 and L.pdgn_gemm_two_part(35840, 512, 5120, 2 ** 32) == 0
        assert L.pdgn_gemm_two_part(35840, 128, 12832, big) == 0
        # `long long` results above 2^31, and wrapped arguments are still taken
        rows = 2 ** 33 + 5
        assert L.pdgn_det_workspace_ints(3, 7, rows) == W.pdgn_det_workspace_ints(3, 7, ll(rows)) == 3 * (2 * 7 + 1 + rows)
        assert L.pdgn_det_workspace_ints(3, 7, ll(rows)) == 3 * (2 * 7 + 1 + rows)
        assert L.pdgn_bn_scratch_floats(rows, 64) == W.pdgn_bn_scratch_floats(ll(rows), 64)
        assert L.pdgn_emd_cost_temp_floats(2 ** 31, 2048, 2048) == W.pdgn_emd_cost_temp_floats(ll(2 ** 31), 2048, 2048) > 2 ** 31
    finally:
        L.pdgn_gemm_set_mode(old)
    with pytest.raises(ctypes.ArgumentError):
        L.pdgn_gemm_two_part(35840.0, 128, 12832, 0)             # a float where the header says long long is refused, not reinterpreted


def test_parser_refuses_what_it_cannot_classify():
    from pdgn_amd import _lib
    ok = "#define PDGN_ABI_VERSION 7\ntypedef void *pdgn_stream_t;\n"
    ver, sigs = _lib.parse_header(ok + "/* int pdgn_not_this(int a); */\nlong long pdgn_a(long long rows, const float *const *x,\n"
                                  "   unsigned *m, unsigned int us, double lr, float eps, pdgn_stream_t s);\nint pdgn_b(void);\n")
    vp = ctypes.c_void_p
    assert ver == 7 and sigs == {"pdgn_a": (ctypes.c_longlong, (ctypes.c_longlong, vp, vp, ctypes.c_uint, ctypes.c_double, ctypes.c_float, vp)),
                                 "pdgn_b": (ctypes.c_int, ())}
    for bad in ("int pdgn_c(size_t n);", "int pdgn_c(short n);", "int pdgn_c(int);", "int pdgn_c(int a, ...);", "int pdgn_c(int a[4]);",
                "int pdgn_c(struct thing t);", "float pdgn_c(int a);", "void pdgn_c(int a);", "int *pdgn_c(int a);", "int pdgn_c();",
                "int pdgn_c(int (*cb)(int));", "int pdgn_b(void); int pdgn_b(int again);", "static inline int pdgn_c(int a) { return a; }"):
        with pytest.raises(_lib.PdgnHipError):
            _lib.parse_header(ok + "int pdgn_b(void);\n" * (not bad.startswith("int pdgn_b")) + bad + "\n")
    with pytest.raises(_lib.PdgnHipError):
        _lib.parse_header("int pdgn_b(void);\n")                 # no version


def test_one_abi_number():
    from pdgn_amd import _lib, build
    define = re.findall(r"^#define\s+PDGN_ABI_VERSION\s+(\d+)\s*$", _header_text(), flags=re.M)
    assert len(define) == 1
    handle = ctypes.CDLL(build.build())
    assert _lib.ABI_VERSION == int(define[0]) == handle.pdgn_abi_version() == _lib.lib().pdgn_abi_version()
    for path, src in _package_sources():                         # and no second copy of the number to bump
        assert not re.search(r"ABI_VERSION\s*=\s*\d", src), path
    for f in os.listdir(os.path.join(ROOT, "pdgn_amd", "csrc")):
        src = open(os.path.join(ROOT, "pdgn_amd", "csrc", f)).read()
        if "pdgn_abi_version" in src:
            assert f == "abi.hip" and "return PDGN_ABI_VERSION;" in src
