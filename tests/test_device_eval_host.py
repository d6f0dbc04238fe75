"""CPU-only tests of the device-array front end: the package still imports without torch, the torch layer imports and validates its
arguments before any GPU work, and without a GPU its constructor fails as RxmdEngine does."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_api as oa
import rxmd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FF_RDX = os.path.join(oa.INP, "ffield_rdx")


def test_importing_the_package_does_not_import_torch():
    """bench.py spawns its ranks from a parent that must not hold torch; the torch layer is a module of its own"""
    code = ("import sys; sys.path.insert(0, %r); import rxmd_amd; "
            "assert 'torch' not in sys.modules, 'import rxmd_amd pulled in torch'; "
            "assert 'rxmd_amd.torch_front' not in sys.modules; print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_torch_front_imports_and_binds_the_new_symbol():
    from rxmd_amd import torch_front
    assert callable(torch_front.ReaxFF) and hasattr(rxmd_amd.RxmdEngine, "evaluate_device")
    assert hasattr(rxmd_amd.load_library(), "rxmd_hip_evaluate_device")


class _StubEngine:
    """counts calls: validation must raise before the engine is reached"""
    calls = 0

    def evaluate_device(self, *a, **kw):
        self.calls += 1
        raise AssertionError("the engine was called with an invalid tensor")


def _stub_model(n):
    import torch
    from rxmd_amd import torch_front
    m = torch_front.ReaxFF.__new__(torch_front.ReaxFF)
    m.engine = _StubEngine(); m.device = torch.device("cuda", 0); m.natoms = n
    m.types = torch.ones(n, dtype=torch.int32); m.gid = None
    return m


@pytest.mark.parametrize("what,match", [("cpu", "CUDA"), ("float32", "float64"), ("shape", "shape")])
def test_evaluate_refuses_a_wrong_tensor_before_any_gpu_work(what, match):
    import torch
    m = _stub_model(5)
    pos = {"cpu": torch.zeros(5, 3, dtype=torch.float64), "float32": torch.zeros(5, 3, dtype=torch.float32),
           "shape": torch.zeros(5, 2, dtype=torch.float64)}[what]
    for call in (m.evaluate, m.energy, m):
        with pytest.raises(ValueError, match=match):
            call(pos)
    with pytest.raises(ValueError):
        m.evaluate(np.zeros((5, 3)))
    assert m.engine.calls == 0


def test_constructor_fails_as_the_engine_does_without_a_gpu():
    import torch
    from rxmd_amd import system, torch_front
    names, frac, lat = system.read_xyz(os.path.join(oa.INP, "rdx.xyz"))
    if not torch.cuda.is_available():
        with pytest.raises(rxmd_amd.RxmdError) as ei:
            torch_front.ReaxFF(FF_RDX, lat, np.ones(4, np.int32))
        assert ei.value.code == -6 and "no CPU path" in str(ei.value)
    with pytest.raises(rxmd_amd.RxmdError) as ei:
        torch_front.ReaxFF("/nonexistent/ffield", lat, np.ones(4, np.int32))
    assert ei.value.code == -2
