"""CPU: the deterministic-mode switch (pdgn_set_deterministic, pdgn_amd.set_deterministic / deterministic): declared and
exported, set / query round trip, the environment default, and the rule that the library follows torch's flag until the
mode is set explicitly.  Every check that touches the process-wide switch runs in a fresh interpreter."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code, **env):
    e = dict(os.environ)
    e.pop("PDGN_DETERMINISTIC", None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split()


def test_switch_is_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdgn_hip.h")).read(), flags=re.S)
    for name in ("pdgn_set_deterministic", "pdgn_grouping_backward_det", "pdgn_interpolation_backward_det",
                 "pdgn_gathering_backward_det", "pdgn_nndistance_grad_det", "pdgn_det_workspace_ints"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
    from pdgn_amd import build
    handle = ctypes.CDLL(build.build())
    for name in ("pdgn_set_deterministic", "pdgn_grouping_backward_det", "pdgn_interpolation_backward_det",
                 "pdgn_gathering_backward_det", "pdgn_nndistance_grad_det", "pdgn_det_workspace_ints"):
        assert hasattr(handle, name), name
    handle.pdgn_det_workspace_ints.restype = ctypes.c_longlong
    assert handle.pdgn_det_workspace_ints(3, 100, ctypes.c_longlong(700)) == 3 * (2 * 100 + 1 + 700)


def test_c_round_trip_returns_the_previous_value():
    out = _run("from pdgn_amd import _lib\n"
               "L = _lib.lib()\n"
               "print(L.pdgn_set_deterministic(-1), L.pdgn_set_deterministic(1), L.pdgn_set_deterministic(-1),"
               " L.pdgn_set_deterministic(0), L.pdgn_set_deterministic(-1), L.pdgn_set_deterministic(7), L.pdgn_set_deterministic(-1))")
    assert out == ["0", "0", "1", "1", "0", "0", "1"]


def test_default_is_off():
    assert _run("import pdgn_amd\nprint(pdgn_amd.deterministic())") == ["False"]


def test_python_round_trip_and_reexports():
    out = _run("import pdgn_amd\nfrom pdgn_amd import _lib\n"
               "assert pdgn_amd.set_deterministic is _lib.set_deterministic and pdgn_amd.deterministic is _lib.deterministic\n"
               "print(pdgn_amd.set_deterministic(True), pdgn_amd.deterministic(), _lib.lib().pdgn_set_deterministic(-1))\n"
               "print(pdgn_amd.set_deterministic(False), pdgn_amd.deterministic(), _lib.lib().pdgn_set_deterministic(-1))")
    assert out == ["False", "True", "1", "True", "False", "0"]


def test_environment_default():
    code = "import pdgn_amd\nfrom pdgn_amd import _lib\nprint(pdgn_amd.deterministic(), _lib.lib().pdgn_set_deterministic(-1))"
    assert _run(code, PDGN_DETERMINISTIC="1") == ["True", "1"]
    assert _run(code, PDGN_DETERMINISTIC="0") == ["False", "0"]
    # an explicit environment setting is not overridden by torch's flag
    assert _run("import torch, pdgn_amd\ntorch.use_deterministic_algorithms(True)\nprint(pdgn_amd.deterministic())",
                PDGN_DETERMINISTIC="0") == ["False"]


def test_follows_torch_until_set_and_explicit_setting_wins():
    out = _run("import torch, pdgn_amd\nfrom pdgn_amd import _lib\n"
               "r = [pdgn_amd.deterministic()]\n"
               "torch.use_deterministic_algorithms(True)\n"
               "r += [pdgn_amd.deterministic(), _lib.lib().pdgn_set_deterministic(-1)]\n"
               "torch.use_deterministic_algorithms(False)\n"
               "r += [pdgn_amd.deterministic(), _lib.lib().pdgn_set_deterministic(-1)]\n"
               "pdgn_amd.set_deterministic(True)\n"
               "r += [pdgn_amd.deterministic()]\n"
               "pdgn_amd.set_deterministic(False)\n"
               "torch.use_deterministic_algorithms(True)\n"
               "r += [pdgn_amd.deterministic()]\n"
               "pdgn_amd.set_deterministic(None)\n"
               "r += [pdgn_amd.deterministic()]\n"
               "print(*r)")
    assert out == ["False", "True", "1", "False", "0", "True", "False", "True"]


def test_trainer_warns_while_the_step_is_not_covered():
    out = _run("import warnings\n"
               "import pdgn_amd\nfrom pdgn_amd import trainer\n"
               "with warnings.catch_warnings(record=True) as w:\n"
               "    warnings.simplefilter('always')\n"
               "    trainer._warn_if_deterministic('step')\n"
               "    n_off = len(w)\n"
               "    pdgn_amd.set_deterministic(True)\n"
               "    trainer._warn_if_deterministic('step')\n"
               "print(n_off, len(w), w[-1].category.__name__)")
    assert out == ["0", "1", "DeterminismWarning"]


def test_package_import_stays_light():
    """The re-exports are lazy: importing the package (the build path does) loads neither torch nor the library."""
    assert _run("import sys, pdgn_amd\nfrom pdgn_amd import build\nprint('torch' in sys.modules)")[0] == "False"
