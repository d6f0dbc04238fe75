"""rxmd_hip_get_bonds_device and its mirrors (RxmdEngine.bonds_device, torch_front.ReaxFF.bond_graph): the bond-order graph of the last FORCE as
coordinate arrays in device memory.

The yardstick is the host path of the SAME engine in the SAME state: RxmdEngine.bonds() + atoms()["gid"], which is held to the oracle per slot
(test_gpu_parity.check_bond_order_taps / parity.compare_bond_order_taps) and to the reference's .bnd file (test_gpu_output.py).  Both paths copy the same
stored doubles and the same global ids, so every comparison with it is exact (np.array_equal).

Bounds that are not exact, and where they come from:
  * the three parts of the bond order: k_bo_full forms BO(1) = (BO(0) - BO(2)) - BO(3) (bo.F90:215); adding the parts again is four rounded operations
    on numbers no larger than BO(0), each within half an ulp of BO(0): |sum - BO(0)| <= 2 eps BO(0).  Asserted at 4 eps BO(0).
  * images: vec - (pos[dst] - pos[src]) must be a lattice vector.  A coordinate in a box of tens of Angstrom carries a rounding of ~1e-14 in
    normalised units; a wrong partner or image is off by a bond length over a box edge, ~1e-1.  Asserted at 1e-9 (normalised).
  * |vec| <= maxrc, the largest bond cut-off of the force field (RxmdEngine.cutoffs), and > 0.
"""
import numpy as np
import pytest
import torch

import oracle_api as oa
from npt_reference import hmat
from parity import _engine, code as _code
from graph_support import _offlattice_engine, _host_coo, _device_coo, _ref, _model, _dev, DEV, EPS, SENT_I, SENT_F, KW5

pytestmark = pytest.mark.gpu


def _check_gid_mode(e, label):
    a, hs, hd, hb = _host_coo(e)
    E, s, d, b, _, _ = _device_coo(e, as_gid=True)
    print(label, "natoms", len(a["gid"]), "directed bonds", E, "atoms without a bond", int((e.bonds()[0] == 0).sum()), "longest list", int(e.bonds()[0].max()))
    assert E == len(hb) and E > 0
    assert np.array_equal(s, hs) and np.array_equal(d, hd) and np.array_equal(b, hb)
    return a, hs, hd, hb


def _check_images(vec, s, d, pos, lat, label):
    """vec - (pos[d] - pos[s]) is a lattice vector, and every edge has its mirror image with the opposite vector"""
    Hi = np.linalg.inv(hmat(lat))
    frac = (vec - (pos[d] - pos[s])) @ Hi.T
    shift = np.rint(frac)
    off_int = np.abs(frac - shift).max()
    edges = {}
    for k in range(len(s)):
        edges[(int(s[k]), int(d[k]), int(shift[k, 0]), int(shift[k, 1]), int(shift[k, 2]))] = k
    assert len(edges) == len(s), "two edges with the same ends and image"
    worst = 0.0
    for (i, j, n0, n1, n2), k in edges.items():
        r = edges.get((j, i, -n0, -n1, -n2))
        assert r is not None, "edge (%d, %d) has no mirror image" % (i, j)
        worst = max(worst, np.abs((vec[k] + vec[r]) @ Hi.T).max())
    print(label, "distance from a lattice vector (normalised) %.2e" % off_int, "edges through an image", int((shift != 0).any(axis=1).sum()), "of", len(s),
          "vec + mirror vec (normalised) %.2e" % worst)
    assert off_int <= 1e-9 and worst <= 1e-9


def _check_index_mode(e, label):
    a, hs, hd, hb = _check_gid_mode(e, label)
    n = len(a["gid"])
    E, s, d, b, parts, vec = _device_coo(e, as_gid=False)
    assert E == len(hb) and s.min() >= 0 and d.min() >= 0 and s.max() < n and d.max() < n
    assert np.array_equal(a["gid"][s], hs) and np.array_equal(a["gid"][d], hd) and np.array_equal(b, hb)
    sum_err = np.abs(parts.sum(axis=1) - b) / np.maximum(b, 1e-300)
    length = np.linalg.norm(vec, axis=1)
    maxrc = e.cutoffs()[1]
    print(label, "parts: min %.3e  |sum - bo| / bo max %.2e" % (parts.min(), sum_err.max()), " |vec| in [%.4f, %.4f], maxrc %.4f" % (length.min(), length.max(), maxrc))
    assert np.isfinite(parts).all() and (parts >= 0.0).all()
    assert (np.abs(parts.sum(axis=1) - b) <= 4 * EPS * b).all()
    assert (length > 0.0).all() and (length <= maxrc).all()
    _check_images(vec, s, d, a["pos"], e.lattice, label)


# ---- 1. global ids equal the host list ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rdx168", "mos2_tri324", "sicnp-pqeq", "rdx-dilute", "rdx-denser", "rdx168-step3"])
def test_gid_mode_equals_the_host_list(case):
    if case == "rdx168":
        e = _engine("rdx168", (1, 1, 1))
    elif case == "mos2_tri324":
        e = _engine("mos2_tri324", (3, 3, 2))
    elif case == "sicnp-pqeq":
        e = _engine("sicnp", (1, 1, 1), pqeq=oa.PQEQ_SICNP)
    elif case == "rdx168-step3":
        e = _engine("rdx168", (1, 1, 1)); e.thermostat(0, 300.0)
    else:
        e = _offlattice_engine(case, **KW5)
    e.QEq(); e.FORCE()
    if case == "rdx168-step3":
        e.step(3)
    cnt = e.bonds()[0]
    if case == "rdx-dilute":
        assert (cnt == 0).any()                    # empty rows in the scan
    if case == "rdx-denser":
        assert cnt.max() > 24
    _check_gid_mode(e, case)
    e.close()


# ---- 2. threshold ------------------------------------------------------------------------------------------------------------------------
def test_threshold_selects_in_order():
    e = _engine("rdx168", (1, 1, 1)); e.QEq(); e.FORCE()
    _, hs, hd, hb = _host_coo(e, bo_min=0.3)
    E0 = e.bonds_device(0, 0, 0, 0, as_gid=True)
    E, s, d, b, _, _ = _device_coo(e, bo_min=0.3, as_gid=True)
    print("rdx168: E(0) %d, E(0.3) %d, largest bond order %.4f" % (E0, E, e.bonds()[2].max()))
    assert 0 < E < E0 and E == len(hb)
    assert np.array_equal(s, hs) and np.array_equal(d, hd) and np.array_equal(b, hb)
    top = float(e.bonds()[2].max()) + 1.0
    Ez, s, d, b, parts, vec = _device_coo(e, bo_min=top, as_gid=True, capacity=16)
    assert Ez == 0
    assert (s == SENT_I).all() and (d == SENT_I).all() and (b == SENT_F).all() and (parts == SENT_F).all() and (vec == SENT_F).all()
    e.close()


# ---- 3. local indices, the parts of the bond order, bond vectors -------------------------------------------------------------------------
@pytest.mark.parametrize("case,mc", [("rdx168", (1, 1, 1)), ("mos2_tri324", (3, 3, 2))])
def test_index_mode_components_and_vectors(case, mc):
    e = _engine(case, mc); e.QEq(); e.FORCE()
    _check_index_mode(e, case)
    e.close()


# ---- 4. both other ghost builds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["RXMD_NO_STAGE_PAIRS", "RXMD_FORCE_STAGED"])
def test_index_mode_behind_the_staged_ghost_builds(env, monkeypatch):
    monkeypatch.setenv(env, "1")                   # (options are read when the engine is created)
    e = _engine("rdx168", (1, 1, 1)); e.QEq(); e.FORCE()
    _check_index_mode(e, "rdx168 " + env)
    e.close()


# ---- 5. growth of the bond tables --------------------------------------------------------------------------------------------------------
def test_scratch_follows_the_growth_of_the_bond_tables(monkeypatch):
    monkeypatch.setenv("RXMD_BOND_CAP", "1024")
    e = _engine("rdx222", (2, 2, 2)); e.QEq(); e.FORCE()
    assert e.stats()["nbonds"] > 1024
    _check_gid_mode(e, "rdx222 from 1024 bonds")
    e.close()


# ---- 6. capacity and refusals ------------------------------------------------------------------------------------------------------------


def test_capacity_and_refusals():
    e = _engine("rdx168", (1, 1, 1))
    buf = torch.zeros(8, dtype=torch.int64, device=DEV); p = buf.data_ptr()
    assert _code(lambda: e.bonds_device(0, 0, 0, 0)) == -7                      # before the first FORCE
    e.QEq(); e.FORCE()
    E = e.bonds_device(0, 0, 0, 0)
    got = _device_coo(e, capacity=E - 1)
    assert got[0] == E and (got[1] == SENT_I).all() and (got[2] == SENT_I).all() and all((x == SENT_F).all() for x in got[3:])
    got = _device_coo(e, capacity=E)
    assert got[0] == E and (got[1] != SENT_I).all() and (got[2] != SENT_I).all() and all((x != SENT_F).all() for x in got[3:])
    e.set_lattice(e.lattice)
    assert _code(lambda: e.bonds_device(0, 0, 0, 0)) == -7                      # the lists are stale
    e.QEq(); e.FORCE()
    assert e.bonds_device(0, 0, 0, 0) == E
    raw = lambda flags, bo_min, cap, s, d, b: e._chk(e.L.rxmd_hip_get_bonds_device(e.h, flags, bo_min, cap, s, d, b, None, None, None))
    assert _code(lambda: raw(2, 0.0, 8, p, p, p)) == -1                         # unknown flag bit
    assert _code(lambda: raw(3, 0.0, 0, None, None, None)) == -1
    assert _code(lambda: e.bonds_device(-1, p, p, p)) == -1                     # negative capacity
    assert _code(lambda: e.bonds_device(0, 0, 0, 0, bo_min=float("nan"))) == -1
    assert _code(lambda: e.bonds_device(0, 0, 0, 0, bo_min=float("inf"))) == -1
    assert _code(lambda: e.bonds_device(8, p, 0, p)) == -1                      # src without dst
    assert _code(lambda: e.bonds_device(8, 0, 0, p)) == -1
    assert (buf == 0).all()
    e.close()
    # local indices on an engine of a decomposed box: an argument error, raised before the state is looked at (no atoms, no transport)
    import rxmd_amd
    ff, names, frac, lat = oa.make_system("rdx168")
    e2 = rxmd_amd.RxmdEngine(ff, lat, vprocs=(2, 1, 1))
    assert _code(lambda: e2.bonds_device(0, 0, 0, 0)) == -1
    assert _code(lambda: e2.bonds_device(8, p, p, p)) == -1
    assert _code(lambda: e2.bonds_device(0, 0, 0, 0, as_gid=True)) == -7        # global ids are fine there: only the state is missing
    e2.close()


# ---- 7. torch ----------------------------------------------------------------------------------------------------------------------------
def _torch_case(shift):
    """rdx168 handed over in a random permutation (gid = the original ids), optionally every atom moved by a lattice vector"""
    r = _ref("rdx168", (1, 1, 1))
    n = len(r["pos"])
    rng = np.random.default_rng(20250211)
    perm = rng.permutation(n)
    pos = r["pos"][perm]
    if shift:
        pos = pos + rng.integers(-3, 4, size=(n, 3)).astype(np.float64) @ hmat(r["lat"]).T
    m = _model(dict(r, type=r["type"][perm], gid=r["gid"][perm]))
    return r, m, r["gid"][perm], pos, _dev(pos)


@pytest.mark.parametrize("shift", [False, True], ids=["caller-order", "anywhere-in-space"])
def test_torch_graph_in_the_callers_order(shift):
    r, m, gid, pos, tpos = _torch_case(shift)
    out = m.evaluate(tpos, bond_graph=0.0)
    g = out["bonds"]
    _, hs, hd, hb = _host_coo(m.engine)
    ei = g["edge_index"].cpu().numpy()
    assert np.array_equal(gid[ei[0]], hs) and np.array_equal(gid[ei[1]], hd) and np.array_equal(g["bond_order"].cpu().numpy(), hb)
    _check_images(g["edge_vec"].cpu().numpy(), ei[0], ei[1], pos, r["lat"], "torch, shifted" if shift else "torch")
    m.close()


def test_torch_types_shapes_and_state():
    import rxmd_amd
    r, m, gid, pos, tpos = _torch_case(False)
    with pytest.raises(rxmd_amd.RxmdError) as ei:
        m.bond_graph()
    assert ei.value.code == -7
    plain = m.evaluate(tpos)
    assert set(plain) == {"energy", "forces", "charges", "pe", "virial"}
    out = m.evaluate(tpos, bond_graph=0.3)
    assert set(out) == set(plain) | {"bonds"} and set(out["bonds"]) == {"edge_index", "bond_order", "edge_vec"}
    g = m.bond_graph(bo_min=0.3, components=True)
    E = g["bond_order"].shape[0]
    assert set(g) == {"edge_index", "bond_order", "edge_vec", "bond_order_parts"} and E > 0
    assert g["edge_index"].dtype == torch.int64 and g["edge_index"].shape == (2, E)
    assert g["bond_order"].dtype == torch.float64 and g["bond_order"].shape == (E,)
    assert g["edge_vec"].dtype == torch.float64 and g["edge_vec"].shape == (E, 3)
    assert g["bond_order_parts"].dtype == torch.float64 and g["bond_order_parts"].shape == (E, 3)
    assert all(t.device == m.device and not t.requires_grad for t in g.values())
    assert (g["bond_order"] >= 0.3).all()
    for k in ("edge_index", "bond_order", "edge_vec"):
        assert torch.equal(g[k], out["bonds"][k])
    none = m.bond_graph(bo_min=1e3)                                 # nothing selected: empty tensors of the documented shapes
    assert none["edge_index"].shape == (2, 0) and none["bond_order"].shape == (0,) and none["edge_vec"].shape == (0, 3)
    m.close()


def test_torch_graph_on_a_side_stream():
    r, m, gid, pos, tpos = _torch_case(False)
    ref = m.evaluate(tpos, bond_graph=0.3)["bonds"]
    ref_sum = (ref["bond_order"].sum(), ref["edge_vec"].abs().sum(), ref["edge_index"].sum())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.randn(2048, 2048, device=DEV) @ torch.randn(2048, 2048, device=DEV)   # work in front of the producer on this stream
        p = tpos + 0.0 * big[0, 0].double()                                                # the input is produced on s ...
        g = m.evaluate(p, bond_graph=0.3)["bonds"]
        side_sum = (g["bond_order"].sum(), g["edge_vec"].abs().sum(), g["edge_index"].sum())   # ... and the graph reduced there
        side = {k: v * 1 for k, v in g.items()}
    s.synchronize()
    assert torch.isfinite(big).all()
    for k in ref:
        assert torch.equal(side[k], ref[k]), k
    assert all(torch.equal(a, b) for a, b in zip(side_sum, ref_sum))
    m.close()
