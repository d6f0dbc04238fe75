"""CPU-only tests of the 10 A pair graph on device arrays: the symbol and its ctypes and torch mirrors exist with the signature of the header, the
header documents every flag and refusal of the call, the torch layer validates its arguments before any engine call, and the package still imports
without torch."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import rxmd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "rxmd_hip.h")).read()


def test_the_library_and_both_mirrors_carry_the_pair_graph():
    from rxmd_amd import _lib, engine, torch_front
    assert hasattr(rxmd_amd.load_library(), "rxmd_hip_get_pairs_device")
    assert callable(rxmd_amd.RxmdEngine.pairs_device) and callable(torch_front.ReaxFF.pair_graph)
    assert "#define RXMD_PAIRS_GID 1" in HDR and engine.PAIRS_GID == 1


def test_the_ctypes_signature_is_the_one_of_the_header():
    from rxmd_amd import _lib
    m = re.search(r"long long rxmd_hip_get_pairs_device\(([^)]*)\);", HDR)
    assert m, "the header does not declare rxmd_hip_get_pairs_device"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["rxmd_handle h", "int flags", "double r_cut", "long long capacity", "long long *src", "long long *dst", "int *shift3",
                      "double *vec3", "double *hval", "void *stream"]
    (name, res, args), = [s for s in _lib.SYMBOLS if s[0] == "rxmd_hip_get_pairs_device"]
    assert res is C.c_longlong
    assert args == [C.c_void_p, C.c_int, C.c_double, C.c_longlong] + [C.c_void_p] * 6
    fn = rxmd_amd.load_library().rxmd_hip_get_pairs_device
    assert fn.restype is C.c_longlong and list(fn.argtypes) == args


def test_the_header_documents_every_flag_and_refusal():
    m = re.search(r"/\* The 10 A pair graph.*?\*/", HDR, re.S)
    assert m, "no comment in front of rxmd_hip_get_pairs_device"
    doc = " ".join(m.group(0).replace("\n *", " ").split())      # (one line: a phrase may be broken over two comment lines)
    for word in ("RXMD_PAIRS_GID", "RXMD_E_STATE", "RXMD_E_ARG", "unknown bits in flags", "negative capacity", "non-finite r_cut", "reach", "12.5 A",
                 "vprocs other than 1 1 1", "shift3", "count only", "capacity < E", "set_lattice", "src == dst", "MULTIGRAPH", "fp32 matrix stream",
                 "isQEq", "eta", "One host wait"):
        assert word in doc, "the header comment does not mention %r" % word


class _StubEngine:
    """counts calls: validation must raise before the engine is reached"""
    calls = 0

    def _called(self, *a, **kw):
        self.calls += 1
        raise AssertionError("the engine was called with an invalid argument")

    evaluate_device = pairs_device = _called


def _stub_model(n):
    import torch
    from rxmd_amd import torch_front
    m = torch_front.ReaxFF.__new__(torch_front.ReaxFF)
    m.engine = _StubEngine(); m.device = torch.device("cuda", 0); m.natoms = n
    m.types = torch.ones(n, dtype=torch.int32); m.gid = None
    return m


@pytest.mark.parametrize("bad", ["x", None, True, [6.5], 1j])
def test_pair_graph_refuses_a_cut_off_that_is_no_real_number(bad):
    m = _stub_model(5)
    with pytest.raises(ValueError, match="r_cut"):
        m.pair_graph(bad)
    assert m.engine.calls == 0


@pytest.mark.parametrize("bad", [1, 0, "yes", None])
def test_pair_graph_refuses_values_that_is_no_bool(bad):
    m = _stub_model(5)
    with pytest.raises(ValueError, match="values"):
        m.pair_graph(6.5, values=bad)
    assert m.engine.calls == 0


def test_pair_graph_refuses_positions_and_cells_of_the_wrong_kind():
    import torch
    m = _stub_model(5)
    with pytest.raises(ValueError, match="pos"):
        m.pair_graph(6.5, pos=torch.zeros(5, 3, dtype=torch.float64))        # a CPU tensor
    with pytest.raises(ValueError, match="pos"):
        m.pair_graph(6.5, pos=[[0.0, 0.0, 0.0]] * 5)
    with pytest.raises(ValueError, match="cell"):
        m.pair_graph(6.5, cell=torch.eye(3, dtype=torch.float32))
    assert m.engine.calls == 0


def test_importing_the_package_still_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import rxmd_amd; "
            "assert 'torch' not in sys.modules, 'import rxmd_amd pulled in torch'; "
            "assert hasattr(rxmd_amd.RxmdEngine, 'pairs_device'); print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
