"""CPU: the gradient guard's host side -- the header's declarations and the ctypes signatures read from them,
the mirror of the record's expressions at their corners, the command line, and what a trainer on the CPU device shows of the guard
(the launches themselves are HIP kernels and have no CPU form)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gradguard_mirror as gm
from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pdgn_gradnorm_workspace_doubles", "pdgn_gradnorm_multi", "pdgn_adam_guard_multi", "pdgn_adam_ema_guard_multi", "pdgn_ema_guard_multi")


def test_header_declares_the_entry_points_and_the_record():
    from pdgn_amd import _lib
    names = declared_symbols()
    assert all(n in names for n in NEW[1:]) and all(n in _lib.SIGNATURES for n in NEW)      # (declared_symbols lists the `int` ones)
    text = open(os.path.join(ROOT, "include", "pdgn_hip.h")).read()
    assert _lib.ABI_VERSION >= 31
    V, I, D, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
    sig = _lib.SIGNATURES
    assert sig["pdgn_gradnorm_workspace_doubles"] == (LL, (I, V))
    assert sig["pdgn_gradnorm_multi"] == (I, (I, V, V, D, V, LL, V, V))
    assert sig["pdgn_adam_guard_multi"] == (I, sig["pdgn_adam_multi"][1][:-1] + (V, V))          # ... step, guard, stream
    assert sig["pdgn_adam_ema_guard_multi"] == (I, sig["pdgn_adam_ema_multi"][1][:-1] + (V, V))
    assert sig["pdgn_ema_guard_multi"] == (I, sig["pdgn_ema_multi"][1][:-1] + (V, V))
    for name in ("pdgn_gradnorm_multi", "pdgn_adam_guard_multi"):
        head = text[:text.index("int " + name + "(")]
        comment = re.sub(r"\s*\n \*\s*", " ", head[head.rindex("/*"):])
        assert "tate touched" in comment and "PDGN_ERR_INVALID" in comment and "before any launch" in comment, name
    # the record: eight 4-byte words in the order the Python side reads them
    body = re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct pdgn_guard_record"):text.index("} pdgn_guard_record;")], flags=re.S)
    fields = [" ".join(f.split()) for f in body[body.index("{") + 1:].split(";") if f.strip()]
    assert fields == ["float norm", "float coef", "float applied", "float found_inf", "unsigned n_applied", "unsigned n_skipped",
                      "unsigned reserved[2]"]
    from pdgn_amd.trainer import GUARD_RECORD_FLOATS
    assert GUARD_RECORD_FLOATS == 8


def test_mirror_corner_cases():
    r = gm.record(np.float64(25.0), 10.0)
    assert r["norm"] == np.float32(5.0) and r["coef"] == np.float32(1.0) and r["applied"] == 1.0 and r["found_inf"] == 0.0
    r = gm.record(np.float64(25.0), 2.5)
    assert r["coef"] == np.float32(2.5 / (5.0 + 1e-6)) and r["coef"].dtype == np.float32 and r["coef"] < 0.5
    for max_norm in (0.0, -3.0, float("inf")):                                   # "no clipping": exactly one
        assert gm.record(np.float64(1e12), max_norm)["coef"] == np.float32(1.0)
    r = gm.record(np.float64(0.0), 1.0)                                          # a norm of zero: 1 / 1e-6 is cut at one, nothing divides by zero
    assert r["norm"] == 0.0 and r["coef"] == np.float32(1.0) and r["applied"] == 1.0
    r = gm.record(np.float64(0.0), 1e-9)
    assert r["coef"] == np.float32(1e-9 / 1e-6)
    for total in (np.float64("nan"), np.float64("inf")):                         # a non-finite total: skipped, and no factor
        r = gm.record(total, 1.0)
        assert r["applied"] == 0.0 and r["found_inf"] == 1.0 and r["coef"] == np.float32(1.0) and not np.isfinite(r["norm"])
    # squares in float64: 1e30 neither overflows nor swallows its neighbours' order of magnitude, 1e-30 does not vanish
    big = gm.total_of([np.full(5, 1e30, np.float32), np.full(7, 1e-30, np.float32)])
    assert np.isfinite(big) and gm.record(big, 0.0)["applied"] == 1.0 and gm.ulps(gm.record(big, 0.0)["norm"], np.float32(np.sqrt(5.0) * 1e30)) <= 1
    assert gm.total_of([np.full(4, 1e-30, np.float32)]) > 0 and np.float32(1e-30) * np.float32(1e-30) == 0
    for bad in (np.nan, np.inf, -np.inf):
        assert gm.record(gm.total_of([np.array([1.0, bad], np.float32), np.ones(3, np.float32)]), 1.0)["applied"] == 0.0
    assert gm.ulps(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1


def test_command_line_reaches_the_trainer():
    from pdgn_amd import train
    from pdgn_amd._lib import PdgnHipError
    base = ["--model_dir", "m", "--num_point", "256"]
    args = train.parse_args(base)
    assert args.grad_guard is False and args.clip_grad_norm is None and args.guard_max_skips == 50
    assert "guard" not in str(train.logged_args(args)) and "clip" not in str(train.logged_args(args))       # the log's first line, as it was
    assert train.parse_args(base + ["--grad_guard"]).grad_guard is True
    args = train.parse_args(base + ["--clip_grad_norm", "2.5", "--guard_max_skips", "7"])
    assert args.grad_guard is True and args.clip_grad_norm == 2.5 and args.guard_max_skips == 7              # clipping implies the guard
    for bad in (["--clip_grad_norm", "0"], ["--clip_grad_norm", "-1"], ["--guard_max_skips", "0"]):
        with pytest.raises(SystemExit):
            train.parse_args(base + bad)
    torch.manual_seed(0)
    tr = train.make_trainer(args, "cpu")
    assert tr.grad_guard and tr.clip_grad_norm == 2.5 and len(tr.guards) == 5 and tr.guard_buf.shape == (5, 8)
    assert all(g.max_norm == 2.5 and g.record.data_ptr() == tr.guard_buf[i].data_ptr() for i, g in enumerate(tr.guards))
    assert tr._stepG.guard is tr.guards[0] and [s.guard for s in tr._stepD] == tr.guards[1:]
    for g, opt in zip(tr.guards, [tr.optG] + tr.optD):
        assert g.workspace.dtype == torch.float64 and g.workspace.numel() == sum((p.numel() + 4095) // 4096 for p in opt.param_groups[0]["params"])
    state = tr.guard_state()
    assert list(state) == ["G", "D1", "D2", "D3", "D4"]
    assert all(v == {"norm": 0.0, "coef": 0.0, "applied": 0, "skipped": 0} for v in state.values())
    tr.guard_buf.view(torch.int32)[1, 4:6] = torch.tensor([7, 2], dtype=torch.int32)
    tr.guard_buf[1, :2] = torch.tensor([3.5, 0.25])
    assert tr.guard_state()["D1"] == {"norm": 3.5, "coef": 0.25, "applied": 7, "skipped": 2}
    for p in tr.D[0].parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(PdgnHipError):                                            # the launches are HIP kernels: no quiet CPU form
        tr._stepD[0].step()
    args.phase = "test"
    assert train.make_trainer(args, "cpu").guards is None


def test_off_is_off_on_the_host():
    from pdgn_amd.generator import PointGenerator
    from pdgn_amd.trainer import PDGNTrainer
    torch.manual_seed(0)
    tr = PDGNTrainer(device="cpu", distributed=False, base_points=16, generator=PointGenerator(256, 20, base_points=16))
    assert tr.grad_guard is False and tr.guards is None and tr.guard_buf is None
    assert tr._stepG.guard is None and all(s.guard is None for s in tr._stepD)
    with pytest.raises(RuntimeError):
        tr.guard_state()
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            PDGNTrainer(device="cpu", distributed=False, base_points=16, generator=PointGenerator(256, 20, base_points=16), clip_grad_norm=bad)
    assert PDGNTrainer(device="cpu", distributed=False, base_points=16, generator=PointGenerator(256, 20, base_points=16),
                       clip_grad_norm=1.0).grad_guard is True
