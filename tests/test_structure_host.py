"""CPU-only tests of the on-device structure statistics (rxmd_hip_structure_*): the header, _lib.SYMBOLS and the ctypes argument lists agree; the
normalisation of rxmd_amd/structure.py on hand-made counts (an ideal-gas profile gives g = 1, n(r) is the running sum, absent types give zeros,
S(q) of an ideal gas is the delta term, merge sums ranks); and the gate of the GPU tests' yardstick: on the disordered boxes at most 1e-5 of the
brute-force samples lie near a bin edge (structure_reference.py), so the L1 rule of test_gpu_structure.py cannot hide a failure."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rxmd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "rxmd_hip.h")).read()

SIGNATURES = {
    "rxmd_hip_structure_begin": (["rxmd_handle h", "double r_max", "int nbins_r", "int nshells", "const double *angle_cut", "int nbins_angle"],
                                 [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "rxmd_hip_structure_sample": (["rxmd_handle h"], [C.c_void_p]),
    "rxmd_hip_structure_get": (["rxmd_handle h", "long long *pair_counts", "long long pair_capacity", "long long *angle_counts", "long long angle_capacity",
                                "long long *atoms_per_type", "double *volume_sum", "long long *frames"],
                               [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "rxmd_hip_structure_end": (["rxmd_handle h"], [C.c_void_p]),
}


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_header_symbol_table_and_ctypes_agree(name):
    from rxmd_amd import _lib
    params, args = SIGNATURES[name]
    m = re.search(r"\nint %s\(([^)]*)\);" % name, HDR)
    assert m, "the header does not declare %s" % name
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == params
    (_, res, bound), = [s for s in _lib.SYMBOLS if s[0] == name]
    assert res is C.c_int and bound == args
    fn = getattr(rxmd_amd.load_library(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == args


def test_the_engine_mirror_exists_and_the_header_documents_the_call():
    for meth in ("structure_begin", "structure_sample", "structure_counts", "structure_end"):
        assert callable(getattr(rxmd_amd.RxmdEngine, meth))
    m = re.search(r"/\* Structure statistics of a live engine.*?\*/", HDR, re.S)
    assert m, "no comment in front of rxmd_hip_structure_begin"
    doc = " ".join(m.group(0).replace("\n *", " ").split())
    for word in ("RXMD_E_ARG", "RXMD_E_STATE", "nbins_r <= 4096", "nshells <= 4", "nbins_angle <= 360", "strictly ascending", "12.5 A", "DIRECTED", "TWICE",
                 "exactly 180", "TRUE volume", "PER RANK", "shortest perpendicular width", "NOTHING is written", "does not reset", "Integer atomics"):
        assert word in doc, "the header comment does not mention %r" % word


def test_structure_module_needs_neither_torch_nor_the_library():
    code = ("import sys; sys.path.insert(0, %r); from rxmd_amd import structure; "
            "assert 'torch' not in sys.modules, 'rxmd_amd.structure pulled in torch'; print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ---- the normalisation on hand-made counts -------------------------------------------------------------------------------------------------------
def _ideal_gas(nso=3, present=(0, 2), natoms=(600, 0, 200), frames=4, volume=8000.0, r_max=8.0, nbr=160):
    """counts an ideal gas would give in expectation (not integers: the functions only divide): a resident of type a sees 4 pi r^2 dr rho_b
    partners of type b in the shell of bin k"""
    from rxmd_amd import structure
    npt = np.array(natoms, np.float64)
    c = dict(pair_counts=np.zeros((nso, nso, nbr)), angle_counts=np.zeros((0, nso, nso, nso, 0), np.int64), atoms_per_type=npt * frames,
             volume_sum=volume * frames, frames=frames, r_max=r_max, angle_cuts=[])
    r = structure.r_centres(c); dr = r_max / nbr
    for a in present:
        for b in present:
            c["pair_counts"][a, b] = frames * npt[a] * 4.0 * np.pi * r * r * dr * npt[b] / volume
    return c


def test_an_ideal_gas_profile_gives_g_equal_one_and_zeros_for_absent_types():
    from rxmd_amd import structure
    c = _ideal_gas()
    g = structure.g_ab(c)
    assert g.shape == (3, 3, 160) and np.isfinite(g).all()
    for a in range(3):
        for b in range(3):
            if a == 1 or b == 1:
                assert (g[a, b] == 0.0).all()                  # the absent type: zeros, not NaN
            else:
                assert np.allclose(g[a, b], 1.0, rtol=1e-13, atol=0.0)
    s = structure.s_ab(c, [0.5, 1.0, 4.0])
    assert s.shape == (3, 3, 3) and np.isfinite(s).all()
    assert np.allclose(s[0, 0], 1.0, atol=1e-12) and np.allclose(s[2, 2], 1.0, atol=1e-12) and np.allclose(s[0, 2], 0.0, atol=1e-12)   # g = 1: the delta term alone
    assert (s[1] == 0.0).all() and (s[:, 1] == 0.0).all()


def test_n_of_r_is_the_running_sum_per_atom_and_sample():
    from rxmd_amd import structure
    rng = np.random.default_rng(3)
    pair = rng.integers(0, 50, (2, 2, 7)).astype(np.int64)
    c = dict(pair_counts=pair, angle_counts=np.zeros((0, 2, 2, 2, 0), np.int64), atoms_per_type=np.array([30, 12], np.int64), volume_sum=3000.0,
             frames=3, r_max=3.5, angle_cuts=[])
    n = structure.n_ab(c)
    for a in range(2):
        for b in range(2):
            for k in range(7):
                assert n[a, b, k] == pair[a, b, :k + 1].sum() / c["atoms_per_type"][a]
    assert np.allclose(structure.r_centres(c), (np.arange(7) + 0.5) * 0.5)
    # g by the reference's formula written out: counts / (4 pi r^2 dr rho * c_b * N_a frames), rho = N / mean V
    rho = (42 / 3) / (3000.0 / 3)
    want = pair[0, 1] / (4 * np.pi * structure.r_centres(c) ** 2 * 0.5 * rho * (12 / 42) * 30)
    assert np.allclose(structure.g_ab(c)[0, 1], want, rtol=1e-14, atol=0.0)


def test_angle_distribution_and_merge():
    from rxmd_amd import structure
    ang = np.zeros((2, 2, 2, 2, 4), np.int64)
    ang[0, 1, 0, 1] = [2, 0, 6, 0]; ang[1, 1, 0, 1] = [2, 4, 6, 4]
    c = dict(pair_counts=np.ones((2, 2, 3), np.int64), angle_counts=ang, atoms_per_type=np.array([8, 0], np.int64), volume_sum=10.0, frames=2, r_max=3.0,
             angle_cuts=[2.0, 3.0])
    d = structure.angle_distribution(c)
    assert np.isfinite(d).all() and np.allclose(d[0, 1, 0, 1], np.array([2, 0, 6, 0]) / (8 * 8.0)) and np.allclose(d[1, 1, 0, 1], np.array([2, 4, 6, 4]) / (16 * 8.0))
    assert (d[:, :, 1] == 0).all() and (d[0, 0, 0, 0] == 0).all()                      # a centre type that is absent, a triple that never occurred
    assert np.allclose(structure.angle_centres(c), [22.5, 67.5, 112.5, 157.5])
    m = structure.merge([c, c])
    assert np.array_equal(m["pair_counts"], 2 * c["pair_counts"]) and np.array_equal(m["angle_counts"], 2 * ang) and list(m["atoms_per_type"]) == [16, 0]
    assert m["frames"] == 2 and m["volume_sum"] == 10.0 and (c["angle_counts"] == ang).all()
    with pytest.raises(ValueError):
        structure.merge([c, dict(c, frames=3)])


# ---- the gate of the yardstick ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rdx-shaken", "rdx-denser", "rdx-dilute"])
def test_near_edge_share_of_the_brute_force_on_disordered_boxes(case):
    import structure_reference as sr
    from graph_support import brute_force
    pos, type0, lat, nso = sr.host_positions(case)
    bf = brute_force(pos, lat, sr.R_MAX)
    p = sr.bin_pairs(bf, type0, nso, sr.R_MAX, sr.NBINS_R)
    a = sr.bin_angles(bf, type0, nso, sr.SHELLS, sr.NBINS_A)
    print("%s: pairs %d, near-edge %d, gap %.2e A; angles per shell %s, near-edge per shell %s, gap to a cut %.2e A"
          % (case, p["samples"], p["near"], p["gap"], list(a["samples"]), list(a["near_samples"]), a["gap"]))
    assert p["gap"] > sr.GAP_TOL and a["gap"] > sr.GAP_TOL
    assert p["near"] <= sr.SHARE_CAP * p["samples"]
    assert a["near_samples"][-1] <= sr.SHARE_CAP * a["samples"][-1]
    assert p["counts"].sum() == p["samples"] and a["counts"][-1].sum() == 2 * a["samples"][-1]
