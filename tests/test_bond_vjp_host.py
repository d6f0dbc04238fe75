"""CPU-only tests of the bond-order VJP (rxmd_hip_bonds_vjp_device): the header declares it, the library exports it, its ctypes and torch mirrors
exist, the torch layer validates its arguments before any engine call, and the package still imports without torch."""
import os
import re
import subprocess
import sys

import pytest

import rxmd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_prototype():
    hdr = open(os.path.join(ROOT, "include", "rxmd_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int rxmd_hip_bonds_vjp_device(rxmd_handle h, int flags, double bo_min, long long E, const double *grad_bo, const double *grad_bo3, "
            "const double *grad_vec3, double *grad_pos3, void *stream);") in flat


def test_the_library_and_both_mirrors_carry_the_vjp():
    from rxmd_amd import _lib, torch_front
    assert hasattr(rxmd_amd.load_library(), "rxmd_hip_bonds_vjp_device")
    sym = {s[0]: s for s in _lib.SYMBOLS}
    assert "rxmd_hip_bonds_vjp_device" in sym and len(sym["rxmd_hip_bonds_vjp_device"][2]) == 9
    assert callable(rxmd_amd.RxmdEngine.bonds_vjp_device) and callable(torch_front.ReaxFF.bond_orders)


class _StubEngine:
    """counts calls: validation must raise before the engine is reached"""
    calls = 0

    def _called(self, *a, **kw):
        self.calls += 1
        raise AssertionError("the engine was called with an invalid argument")

    evaluate_device = bonds_device = bonds_vjp_device = _called


def _stub_model(n):
    import torch
    from rxmd_amd import torch_front
    m = torch_front.ReaxFF.__new__(torch_front.ReaxFF)
    m.engine = _StubEngine(); m.device = torch.device("cuda", 0); m.natoms = n
    m.types = torch.ones(n, dtype=torch.int32); m.gid = None
    return m


@pytest.mark.parametrize("bad", ["x", None, True, [0.3], 1j])
def test_bond_orders_refuses_a_threshold_that_is_no_real_number(bad, monkeypatch):
    import torch
    from rxmd_amd import torch_front
    monkeypatch.setattr(torch_front, "_check_pos", lambda *a: None)      # (cannot pass without a GPU tensor: the check behind it is the one that speaks)
    m = _stub_model(5)
    with pytest.raises(ValueError, match="bo_min"):
        m.bond_orders(torch.zeros(5, 3, dtype=torch.float64), bo_min=bad)
    assert m.engine.calls == 0


@pytest.mark.parametrize("bad", [1, 0, "yes", None])
def test_bond_orders_refuses_components_that_is_no_bool(bad, monkeypatch):
    import torch
    from rxmd_amd import torch_front
    monkeypatch.setattr(torch_front, "_check_pos", lambda *a: None)
    m = _stub_model(5)
    with pytest.raises(ValueError, match="components"):
        m.bond_orders(torch.zeros(5, 3, dtype=torch.float64), components=bad)
    assert m.engine.calls == 0


def test_bond_orders_refuses_bad_positions():
    import torch
    m = _stub_model(5)
    for bad in ("x", torch.zeros(5, 3, dtype=torch.float32), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(5, 3, dtype=torch.float64)):   # the last: not on the GPU
        with pytest.raises(ValueError, match="pos"):
            m.bond_orders(bad)
    assert m.engine.calls == 0


def test_importing_the_package_still_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import rxmd_amd; "
            "assert 'torch' not in sys.modules, 'import rxmd_amd pulled in torch'; "
            "assert hasattr(rxmd_amd.RxmdEngine, 'bonds_vjp_device'); print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
