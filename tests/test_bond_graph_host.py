"""CPU-only tests of the bond-order graph on device arrays: the symbol, its ctypes and torch mirrors exist, the torch layer validates its
arguments before any engine call, and the package still imports without torch."""
import os
import subprocess
import sys

import pytest

import rxmd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_and_both_mirrors_carry_the_bond_graph():
    from rxmd_amd import _lib, torch_front
    assert hasattr(rxmd_amd.load_library(), "rxmd_hip_get_bonds_device")
    assert "rxmd_hip_get_bonds_device" in {s[0] for s in _lib.SYMBOLS}
    assert callable(rxmd_amd.RxmdEngine.bonds_device) and callable(torch_front.ReaxFF.bond_graph)
    hdr = open(os.path.join(ROOT, "include", "rxmd_hip.h")).read()
    assert "#define RXMD_BONDS_GID 1" in hdr
    from rxmd_amd import engine
    assert engine.BONDS_GID == 1


class _StubEngine:
    """counts calls: validation must raise before the engine is reached"""
    calls = 0

    def _called(self, *a, **kw):
        self.calls += 1
        raise AssertionError("the engine was called with an invalid argument")

    evaluate_device = bonds_device = _called


def _stub_model(n):
    import torch
    from rxmd_amd import torch_front
    m = torch_front.ReaxFF.__new__(torch_front.ReaxFF)
    m.engine = _StubEngine(); m.device = torch.device("cuda", 0); m.natoms = n
    m.types = torch.ones(n, dtype=torch.int32); m.gid = None
    return m


@pytest.mark.parametrize("bad", ["x", None, True, [0.3], 1j])
def test_bond_graph_refuses_a_threshold_that_is_no_real_number(bad):
    m = _stub_model(5)
    with pytest.raises(ValueError, match="bo_min"):
        m.bond_graph(bo_min=bad)
    assert m.engine.calls == 0


@pytest.mark.parametrize("bad", [1, 0, "yes", None])
def test_bond_graph_refuses_components_that_is_no_bool(bad):
    m = _stub_model(5)
    with pytest.raises(ValueError, match="components"):
        m.bond_graph(components=bad)
    assert m.engine.calls == 0


@pytest.mark.parametrize("bad", ["x", True, [0.3]])
def test_evaluate_refuses_a_bad_bond_graph_argument_before_the_engine_is_called(bad, monkeypatch):
    """the position check comes first and cannot pass without a GPU tensor: it is stubbed out so that the check behind it is the one that speaks"""
    import torch
    from rxmd_amd import torch_front
    monkeypatch.setattr(torch_front, "_check_pos", lambda *a: None)
    m = _stub_model(5)
    with pytest.raises(ValueError, match="bo_min"):
        m.evaluate(torch.zeros(5, 3, dtype=torch.float64), bond_graph=bad)
    assert m.engine.calls == 0


def test_importing_the_package_still_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import rxmd_amd; "
            "assert 'torch' not in sys.modules, 'import rxmd_amd pulled in torch'; "
            "assert hasattr(rxmd_amd.RxmdEngine, 'bonds_device'); print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
