"""ctypes loader for libpdgn_hip.so (the C ABI declared in include/pdgn_hip.h).

There is NO CPU fallback: if the library is missing or a tensor is not on a ROCm device the
call raises.  Building is explicit (`python -m pdgn_amd.build` / `__graft_entry__.build()`).
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libpdgn_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "pdgn_hip.h")
_lib = None


class PdgnHipError(RuntimeError):
    pass


# The header is the ABI: the vocabulary of its prototypes, and nothing else, is understood here.
_RETURNS = {"int": ctypes.c_int, "long long": ctypes.c_longlong}
_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint,
            "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float, "double": ctypes.c_double,
            "pdgn_stream_t": ctypes.c_void_p}


def parse_header(text):
    """(PDGN_ABI_VERSION, {name: (restype, argtypes)}) of every prototype `RET pdgn_name(ARGS);` in the text of a header.  A
    parameter with a `*` is a pointer (c_void_p), every other one is `TYPE name` with TYPE in _SCALARS; a prototype with anything
    else in it raises PdgnHipError -- a wrong guess here is a wrong argument on the device."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    version = re.search(r"^[ \t]*#[ \t]*define[ \t]+PDGN_ABI_VERSION[ \t]+(\d+)[ \t]*$", text, flags=re.M)
    if version is None:
        raise PdgnHipError("no `#define PDGN_ABI_VERSION <number>` in the header")
    signatures = {}
    for stmt in re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).split(";"):
        if not re.search(r"\bpdgn_\w+\s*\(", stmt):
            continue
        proto = " ".join(stmt.split())
        m = re.fullmatch(r"(.*?) ?\b(pdgn_\w+) ?\((.*)\)", proto)
        if m is None or m.group(1) not in _RETURNS or m.group(2) in signatures:
            raise PdgnHipError("include/pdgn_hip.h: cannot read the prototype `%s;`" % proto)
        argtypes = []
        for arg in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            words = [w for w in arg.split() if w != "const"]
            if "*" in arg and "(" not in arg and "[" not in arg:
                ctype = ctypes.c_void_p
            else:
                ctype = _SCALARS.get(" ".join(words[:-1])) if words and words[-1].isidentifier() else None
            if ctype is None:
                raise PdgnHipError("include/pdgn_hip.h: cannot read the parameter `%s` of `%s;`" % (arg.strip(), proto))
            argtypes.append(ctype)
        signatures[m.group(2)] = (_RETURNS[m.group(1)], tuple(argtypes))
    return int(version.group(1)), signatures


with open(HEADER) as _f:
    ABI_VERSION, SIGNATURES = parse_header(_f.read())


def lib():
    """Load (once) and return the ctypes handle of libpdgn_hip.so, every entry point with the restype / argtypes of its prototype in
    include/pdgn_hip.h: call sites pass plain Python ints and floats, ptr() / stream_of() handles, None or ctypes arrays."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise PdgnHipError(
                "libpdgn_hip.so is not built (%s missing): run `python -m pdgn_amd.build`; "
                "pdgn_amd has no CPU fallback" % SO_PATH)
        handle = ctypes.CDLL(SO_PATH)
        got = handle.pdgn_abi_version()
        if got != ABI_VERSION:
            raise PdgnHipError("libpdgn_hip.so ABI %d != expected %d: rebuild" % (got, ABI_VERSION))
        for name, (restype, argtypes) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError:
                raise PdgnHipError("libpdgn_hip.so does not export %s, which include/pdgn_hip.h declares: rebuild" % name) from None
            fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
        if handle.pdgn_gemm_set_mode(-1) == 2:                     # the default mode: a ring on the current device now (raw ctypes callers);
            ensure_scale_slots(handle=handle)                      # the wrappers move it if the contractions run on another one
    return _lib


_SCALE_SLOTS = {}               # device index -> the ring handed to the library (one process drives one GPU; kept alive here)


def ensure_scale_slots(device=None, handle=None):
    """Two-part contractions (csrc/gemm_x3.hip): the arena of the library's own operand-maxima scans is the caller's memory -- the
    library never allocates.  64 MB on the device the contractions run on, used round-robin (a scanned operand takes 4 bytes per
    kernel-side row: at most 0.3 MB; an iteration makes a few dozen scans inside the library and at most two iterations are in
    flight); called by the contraction wrappers, so that the arena lives on the device in use whatever device was current when the
    library was loaded."""
    if not torch.cuda.is_available():
        return
    idx = torch.cuda.current_device() if device is None or device.index is None else device.index
    if _SCALE_SLOTS.get("attached") == idx:
        return
    if idx not in _SCALE_SLOTS:
        _SCALE_SLOTS[idx] = torch.zeros(1 << 24, dtype=torch.int32, device=torch.device("cuda", idx))
    t = _SCALE_SLOTS[idx]
    check((handle or lib()).pdgn_gemm_set_scale_slots(ptr(t), t.numel() * 4), "pdgn_gemm_set_scale_slots")
    _SCALE_SLOTS["attached"] = idx


def stream_of(t):
    """hipStream_t of torch's current stream on t's device (raw handle: this runs ~3000 times per training step)."""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(t.device.index))


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def check(rc, what):
    if rc != 0:
        if rc == -1:
            raise PdgnHipError("%s: argument outside the supported range" % what)
        raise PdgnHipError("%s: HIP launch failed with hipError_t %d" % (what, rc))


def require(t, name, dtype, dim=None):
    """Reference preconditions (pointops.py:129-130, knnquery_cuda.cpp:12-14) + dtype/device."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise PdgnHipError("%s must live on a ROCm device (pdgn_amd has no CPU path)" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    assert t.is_contiguous(), "%s must be contiguous" % name
    if dim is not None and t.dim() != dim:
        raise ValueError("%s must have %d dims, got %d" % (name, dim, t.dim()))
    return t


def gemm_mode():
    """'x3' (fp32 products as six bf16 MFMA products, csrc/gemm_x3.hip -- the default) or 'fp32' (the fp32 matrix instructions,
    csrc/gemm_nt.hip): what pdgn_gemm_nt / _nn / _nt_ex / _tn_big launch.  PDGN_GEMM in the environment sets the initial value."""
    return _MODE_NAMES[lib().pdgn_gemm_set_mode(-1)]


_MODE_NAMES = {0: "fp32", 1: "x3", 2: "x2"}
DEFAULT_GEMM_MODE = os.environ.get("PDGN_GEMM") or "x2"          # what the library starts in (it reads the same variable at first use)


def matrix_core_mode():
    """True in the two modes that multiply split operands on the bf16 / fp16 matrix cores (csrc/gemm_x3.hip)."""
    return gemm_mode() != "fp32"


def set_gemm_mode(mode):
    """Select the arithmetic of the dense contractions for this process: "x3" (bf16 matrix cores, three parts per value; the
    process default's matrix instruction per instance class), "x3_16" / "x3_32" (every class on v_mfma_f32_16x16x32_bf16 /
    _32x32x16_bf16), "x2" (fp16 matrix cores, two scaled parts per value), "fp32" (fp32 matrix instructions); returns the previous
    mode's name ("x3" | "x2" | "fp32").  Pre-split weights (fused.split_planes) belong to the mode they were made in."""
    m = str(mode)
    if m == "x2":
        ensure_scale_slots()
    old = lib().pdgn_gemm_set_mode(0 if m.startswith("f") else 2 if m == "x2" else 1)
    if not m.startswith("f"):                                      # (any matrix-core mode without a suffix: the process default's instruction per class)
        lib().pdgn_gemm_set_shape(16 if m.endswith("_16") else 32 if m.endswith("_32") else -1)
    return _MODE_NAMES[old]


def set_gemm_shape(shape):
    """Select the bf16 matrix instruction of the dense contractions (32: v_mfma_f32_32x32x16_bf16, 16: v_mfma_f32_16x16x32_bf16)
    for this process; returns the previous shape.  Measurement / tests (PDGN_X3_SHAPE sets the process default)."""
    return lib().pdgn_gemm_set_shape(int(shape))


def set_gemm_config(cfg):
    """Force a tile configuration of pdgn_gemm_nt / _nn (0 .. 3; None or -1: the launch model's pick).  Measurement / tests.
    Returns the previous value (-1: automatic)."""
    return lib().pdgn_gemm_set_config(-1 if cfg is None else int(cfg))


# ---------------------------------------------------------------------------- deterministic mode
_DET_EXPLICIT = bool(os.environ.get("PDGN_DETERMINISTIC"))       # the environment counts as an explicit setting (the library reads it too)
_det_synced = None                                               # the value last handed to the library while following torch's flag


def deterministic():
    """Whether the library's deterministic mode is in force: the value set by `set_deterministic` (or PDGN_DETERMINISTIC in the
    environment); with neither, torch.are_deterministic_algorithms_enabled() at call time; pdgn_set_deterministic holds the value.
    What the mode covers: the backward of pointops grouping / interpolation / gathering and of nn_distance run in a fixed order
    (bitwise repeatable).  The training step is NOT covered yet: PDGNTrainer.step / capture_list warn (DeterminismWarning)
    when they run with the mode on."""
    global _det_synced
    if _DET_EXPLICIT:
        return bool(lib().pdgn_set_deterministic(-1))
    on = torch.are_deterministic_algorithms_enabled()
    if on != _det_synced:                                        # the library's own choices follow the same value
        lib().pdgn_set_deterministic(int(on))
        _det_synced = on
    return on


def set_deterministic(on):
    """Turn the deterministic mode on (True) or off (False) for this process, overriding torch's flag; None returns to following
    torch.are_deterministic_algorithms_enabled().  Returns the previous value (True / False, what `deterministic()` said)."""
    global _DET_EXPLICIT, _det_synced
    old = deterministic()
    if on is None:
        _DET_EXPLICIT, _det_synced = False, None
        deterministic()
    else:
        lib().pdgn_set_deterministic(1 if on else 0)
        _DET_EXPLICIT = True
    return old


def det_workspace(device, *transposes):
    """Integer workspace of a fixed-order scatter adjoint: pdgn_det_workspace_ints per (b, targets, edges) transpose it makes."""
    L = lib()
    ints = sum(L.pdgn_det_workspace_ints(int(b), int(t), int(e)) for b, t, e in transposes)
    return torch.empty(ints, dtype=torch.int32, device=device)
