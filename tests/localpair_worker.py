"""The Chamfer kernels of csrc/localpair.hip through the C ABI, argmins included: shared by tests/test_gpu_localpair.py and its child
process (python tests/localpair_worker.py OUT.npz, run there with PDGN_CHAMFER_LDS=0 -- the switch is read once per process -- so
that a shape the LDS adjoint would take goes through the zero-fill and the global-atomic kernel instead)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import localpair_cases as lc  # noqa: E402

SENTINEL = 777.25            # what every output buffer holds before a call: a sum that started from it is not the mirror's
PAD = 64                     # floats of guard band behind (and, for two buffers, between) the gradient buffers


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                   # (a copy: the cached references are read-only)


def device_chamfer(x, y, ia=None, ib=None):
    """pdgn_chamfer_gram (or, with pair lists, pdgn_chamfer_gram_indexed) on device tensors -> minx, argx, miny, argy."""
    from pdgn_amd import _lib
    m, d = x.shape[1:]
    n = y.shape[1]
    b = x.shape[0] if ia is None else ia.numel()
    minx = torch.full((b, m), SENTINEL, device=x.device)
    miny = torch.full((b, n), SENTINEL, device=x.device)
    argx = torch.full((b, m), -7, dtype=torch.int32, device=x.device)
    argy = torch.full((b, n), -7, dtype=torch.int32, device=x.device)
    L, ptr = _lib.lib(), _lib.ptr
    if ia is None:
        rc = L.pdgn_chamfer_gram(b, m, n, d, ptr(x), ptr(y), ptr(minx), ptr(argx), ptr(miny), ptr(argy), _lib.stream_of(x))
    else:
        rc = L.pdgn_chamfer_gram_indexed(b, m, n, d, ptr(x), ptr(ia), ptr(y), ptr(ib), ptr(minx), ptr(argx), ptr(miny), ptr(argy),
                                         _lib.stream_of(x))
    _lib.check(rc, "pdgn_chamfer_gram")
    torch.cuda.synchronize()
    return minx, argx, miny, argy


def device_chamfer_grad(x, y, argx, argy, gminx=None, gminy=None, uniform=None, layout="one"):
    """pdgn_chamfer_gram_grad (gminx, gminy) or pdgn_chamfer_gram_grad_uniform (uniform = (g tensor, scale)) into buffers that start
    out full of SENTINEL.  layout "one": gy begins where gx ends, as losses.ChamferSum allocates them (one zero-fill in the
    fallback); "two": PAD floats lie between them, as with losses.ChamferGram's two allocations (two fills).  The guard bands
    must come back untouched.  -> gx (b, m, d), gy (b, n, d)."""
    from pdgn_amd import _lib
    b, m, d = x.shape
    n = y.shape[1]
    nx, ny = b * m * d, b * n * d
    gap = 0 if layout == "one" else PAD
    buf = torch.full((nx + gap + ny + PAD,), SENTINEL, device=x.device)
    gx, gy = buf[:nx], buf[nx + gap:nx + gap + ny]
    assert (gy.data_ptr() == gx.data_ptr() + 4 * nx) == (layout == "one")
    L, ptr = _lib.lib(), _lib.ptr
    if uniform is None:
        rc = L.pdgn_chamfer_gram_grad(b, m, n, d, ptr(x), ptr(y), ptr(gminx), ptr(argx), ptr(gminy), ptr(argy), ptr(gx), ptr(gy),
                                      _lib.stream_of(x))
    else:
        rc = L.pdgn_chamfer_gram_grad_uniform(b, m, n, d, ptr(x), ptr(y), ptr(uniform[0]), uniform[1], ptr(argx), ptr(argy), ptr(gx),
                                              ptr(gy), _lib.stream_of(x))
    _lib.check(rc, "pdgn_chamfer_gram_grad")
    torch.cuda.synchronize()
    assert bool((buf[nx:nx + gap] == SENTINEL).all()) and bool((buf[nx + gap + ny:] == SENTINEL).all()), "wrote outside gx / gy"
    return gx.view(b, m, d), gy.view(b, n, d)


def f32(a):
    return np.asarray(a).astype(np.float32)


def run_case(case, layouts=("one", "two")):
    """Forward and both adjoints of one exact case on the device, every result compared bit for bit with the mirror
    (localpair_cases.chamfer_reference).  -> {name: numpy array} of the device's results (the adjoints of the last layout)."""
    ref = lc.chamfer_reference(case)
    x, y = dev(ref["x"]), dev(ref["y"])
    minx, argx, miny, argy = device_chamfer(x, y)
    out = dict(minx=minx.cpu().numpy(), argx=argx.cpu().numpy(), miny=miny.cpu().numpy(), argy=argy.cpu().numpy())
    np.testing.assert_array_equal(out["argx"], ref["argx"])
    np.testing.assert_array_equal(out["argy"], ref["argy"])
    np.testing.assert_array_equal(out["minx"], f32(ref["minx"]))
    np.testing.assert_array_equal(out["miny"], f32(ref["miny"]))
    g = torch.tensor([lc.UNIFORM_G], device=x.device)
    for layout in layouts:
        gx, gy = device_chamfer_grad(x, y, argx, argy, dev(ref["gminx"]), dev(ref["gminy"]), layout=layout)
        ux, uy = device_chamfer_grad(x, y, argx, argy, uniform=(g, lc.UNIFORM_SCALE), layout=layout)
        out.update(gx=gx.cpu().numpy(), gy=gy.cpu().numpy(), ux=ux.cpu().numpy(), uy=uy.cpu().numpy())
        for k in ("gx", "gy", "ux", "uy"):
            np.testing.assert_array_equal(out[k], f32(ref[k]), err_msg="%s, layout %s" % (k, layout))
    return out


if __name__ == "__main__":
    res = run_case(lc.WORKER_CASE)
    np.savez(sys.argv[1], **res)
    print("localpair worker ok: PDGN_CHAMFER_LDS=%s" % os.environ.get("PDGN_CHAMFER_LDS", "1"))
