"""The fixtures of the mixed-precision charge solver (tests/golden/*_f32matrix_tight.npz, written by tests/golden/make_f32_matrix_golden.py) and the
host-visible surface of the switch -- no GPU needed.

A fixture holds the fixed point of the 10 A matrix whose values were rounded once to REAL(4), computed by a scratch copy of the plain-C oracle.
It must really be that solution: away from the unmodified oracle's charges by what the rounding does (measured on the CPU: q_err 5.4e-7 on RDX,
1.8e-7 on ice), and not further; the total potential energy, a second-order quantity of a variational solve, agrees far more closely.
"""
import os
import numpy as np
import pytest

import oracle_api as oa
from parity import q_err

KW = dict(QEq_tol=1e-12, NMAXQEq=2000)
CASES = [("rdx168", (1, 1, 1)), ("ice644", (6, 4, 4))]


def fixture(case):
    return np.load(os.path.join(oa.GOLD, "%s_f32matrix_tight.npz" % case))


@pytest.mark.parametrize("case,mc", CASES)
def test_fixture_holds_the_solution_of_the_rounded_matrix(case, mc):
    g = fixture(case)
    ff, names, frac, lat = oa.make_system(case)
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=mc)
    o = oa.Oracle(ff, lat2, ranks, **KW); o.qeq(); o.force()
    assert (g["gid"] == o.gids()).all()
    dq = q_err(g["q"], o.charges())
    dpe = abs(g["pe"][0] - o.energy()[0]) / abs(o.energy()[0])
    print("%s: fixture against the unmodified oracle: q_err %.2e, total PE %.2e relative" % (case, dq, dpe))
    assert 1e-8 <= dq <= 2e-6
    assert dpe <= 1e-9
    assert g["f"].shape == (len(g["gid"]), 3) and g["pe"].shape == (14,) and np.isfinite(float(g["Est"]))
    if case == "rdx168":
        assert int(g["md_steps"]) == 40 and g["md_pos"].shape == (168, 3) and g["md_q"].shape == (168,) and np.isfinite(float(g["md_Etot"]))


def test_library_exports_the_precision_switch():
    import rxmd_amd
    L = rxmd_amd.load_library()
    for name in ("rxmd_hip_set_qeq_precision", "rxmd_hip_get_qeq_precision"):
        assert hasattr(L, name), name
    header = open(os.path.join(oa.ROOT, "include", "rxmd_hip.h")).read()
    assert "int rxmd_hip_set_qeq_precision(rxmd_handle h, int matrix_bits);" in header
    assert "int rxmd_hip_get_qeq_precision(rxmd_handle h, int *requested_bits, int *in_use_bits);" in header


def test_engine_class_has_the_precision_methods():
    import rxmd_amd
    assert callable(getattr(rxmd_amd.RxmdEngine, "set_qeq_precision", None))
    assert callable(getattr(rxmd_amd.RxmdEngine, "qeq_precision", None))


def test_options_text_names_the_environment_switch():
    from rxmd_amd import _lib
    text = _lib.describe_options()
    rows = [l for l in text.split("\n") if l.startswith("| `RXMD_QEQ_F32`")]
    assert len(rows) == 1 and "PQEq" in rows[0]
    one_trip = [l for l in text.split("\n") if l.startswith("| `RXMD_SPMV_ONE_TRIP`")]
    assert len(one_trip) == 1 and "RXMD_QEQ_F32" in one_trip[0]        # ignored while the float stream is in use: its row says so
