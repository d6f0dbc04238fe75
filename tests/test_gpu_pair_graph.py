"""rxmd_hip_get_pairs_device and its mirrors (RxmdEngine.pairs_device, torch_front.ReaxFF.pair_graph): the engine's 10 A list as a radius graph in
coordinate arrays in device memory.

The yardstick of the selection is a brute force in numpy over the positions and the lattice the SAME engine reports (atoms(), lattice): every
image n with |n_a| <= ceil(r_cut |row a of H^-1|), every pair with d <= r_cut, i != j or n != 0.  It is computed once per system at the largest
cut-off and filtered for the smaller ones.  The yardstick of the values and of the whole list are the engine's debug taps 6 / 7 and the oracle's
taps 104 / 108, which test_gpu_parity holds to each other.

Bounds, and where they come from:
  * vec3 against the brute force: 1e-12 A absolute.  Both sides subtract coordinates of at most 45 A (ulp 7e-15) and the image adds up to three
    lattice vectors of that size: a few ulps, ~5e-14; a wrong image is off by a box edge.  Derived, not measured.
  * shift3 and the multiset of (src, dst, shift): exact.  The test first asserts that no brute-force distance lies within 1e-8 A of r_cut, so the
    roundings above cannot move an edge across the cut-off.
  * per-row sums of hval against tap 7 / tap 108: rtol 1e-12, the tolerance of test_gpu_parity.py:81 (same numbers, another summation order).
  * hval entry by entry against numpy on the oracle's table (qeq_table, hval_of_r2, check_hval_entries): 8 eps |h|, three rounded operations on
    either side of (1 - t) T[itb] + t T[itb + 1]; the reference is taken in the four forms a compiler's FMA contraction of its two inner products
    leaves, one form must hold all entries of a system (all ranks), and at most 2 entries per system may match at the float next to float32(|vec|^2).  Derived in check_hval_entries.  fp32 stream: exact.
  * torch, d/dpos of sum |vec|^2 against 2 (scatter(vec, dst) - scatter(vec, src)): both sides sum the same <= ~300 terms of magnitude <= 2 r_cut
    per atom in different orders: <= 300 eps x 300 x 13 A = 2.6e-10; asserted at 1e-9.
  * the QEq stationarity chi + H q = const from the exported matrix: no number fixed in advance; the engine's charges are allowed ten times the
    spread the ORACLE's charges give with the same exported matrix (both solvers stop on an energy criterion).  Printed by the test.
"""
import math

import numpy as np
import pytest
import torch

import oracle_api as oa
import offlattice_systems as ol
from npt_reference import hmat
from parity import _engine, _oracle, code as _code
from graph_support import (_make, rebuild, brute_force, _select, device_coo, qeq_table, check_hval_entries, _ref, _model, _dev,
                           DEV, SENT_I, SENT_F, KW5, TIGHT, CUTS, EDGES)

pytestmark = pytest.mark.gpu


def check_against_brute_force(e, bf, r_cut, label, as_gid=False):
    a = e.atoms()
    ref_keys, ref_vec, gap = _select(bf, r_cut)
    E, s, d, sh, vec, hv = device_coo(e, r_cut, as_gid=as_gid)
    if as_gid:
        local = {int(g): k for k, g in enumerate(a["gid"])}
        s = np.array([local[int(g)] for g in s], dtype=np.int64); d = np.array([local[int(g)] for g in d], dtype=np.int64)
    keys = np.concatenate([s[:, None], d[:, None], sh.astype(np.int64)], axis=1)
    o = np.lexsort(keys.T[::-1])
    keys, vec_s = keys[o], vec[o]
    err = np.abs(vec_s - ref_vec).max() if len(keys) == len(ref_keys) and E > 0 else float("nan")
    print("%s r_cut %.1f: E %d (brute force %d), smallest gap to r_cut %.2e A, max |vec - brute force| %.2e A, edges through an image %d, src == dst %d"
          % (label, r_cut, E, len(ref_keys), gap, err, int((sh != 0).any(axis=1).sum()), int((s == d).sum())))
    assert E == len(ref_keys)
    assert np.array_equal(keys, ref_keys), "the multiset of (src, dst, shift) differs from the brute force"
    assert err <= 1e-12
    assert (s[:-1] <= s[1:]).all(), "edges are not in resident order"
    assert np.isfinite(hv).all()
    return keys


# ---- 1. brute-force equality ---------------------------------------------------------------------------------------------------------------
_BF = {}


def _system(case):
    """engine after QEq + FORCE and the brute force at 9.5 A over ITS positions (computed once per system, shared)"""
    e = _make(case); e.QEq(); e.FORCE()
    if case not in _BF:
        a = e.atoms()
        _BF[case] = brute_force(a["pos"], e.lattice, max(CUTS))
        for arr in _BF[case]:
            arr.setflags(write=False)
    return e, _BF[case]


@pytest.mark.parametrize("case", list(EDGES))
def test_equals_the_brute_force_radius_graph(case):
    e, bf = _system(case)
    st = e.stats()
    print(case, "natoms", st["natoms"], "longest row", st["max_n10"], "stride", st["n10_stride"], "streams_by_place", st["streams_by_place"], "win_in_use",
          st["win_in_use"], "nb10 written / sticky", e.debug(15, cap=2))
    if case == "rdx-denser":
        assert st["max_n10"] > 1024
    if case == "rdx-dilute":
        assert st["max_n10"] < 128
    for build in ("first build", "second build"):
        if build == "second build":
            entries = rebuild(e)
            print(case, "second build: 4-byte entries written", entries, "streams_by_place", e.stats()["streams_by_place"])
            # the slot route is met where the windows run and no atom meets its own image (rdx168) / no window overflows (rdx-denser)
            assert entries == (case in ("rdx168", "rdx168-z9.42", "rdx-denser"))
        for r_cut, want in zip(CUTS, EDGES[case]):
            keys = check_against_brute_force(e, bf, r_cut, case + ", " + build)
            assert len(keys) == want
    if case == "rdx168-z9.42":                     # (keys: those of 9.5 A) every atom sees itself one box up and one box down
        own = keys[keys[:, 0] == keys[:, 1]]
        print("rdx168-z9.42 at 9.5 A: edges with src == dst:", len(own))
        assert len(own) == 2 * 168 and (own[:, 2:4] == 0).all() and (np.abs(own[:, 4]) == 1).all()
    if case == "rdx168":                           # (keys: those of 9.5 A) the self-image box: a multigraph
        pairs = {}
        for k in keys:
            pairs.setdefault((int(k[0]), int(k[1])), set()).add(tuple(int(x) for x in k[2:]))
        multi = sum(1 for v in pairs.values() if len(v) > 1)
        print("rdx168 at 9.5 A: (src, dst) pairs that occur through two or more images:", multi)
        assert multi > 0
    e.close()


# ---- 2. the whole list ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rdx168", "rdx-shaken", "ice644"])
def test_whole_list_counts_and_row_sums_equal_the_taps(case):
    if case in ol.SYSTEMS:
        o = ol.oracle(case, **KW5)
    else:
        o = _oracle(case, {"ice644": (6, 4, 4)}.get(case, (1, 1, 1)), **KW5)
    o.qeq(); o.force()
    e = _make(case, **KW5); e.QEq(); e.FORCE()
    n = e.natoms
    E, s, d, sh, vec, hv = device_coo(e, 0.0)
    cnt = np.bincount(s, minlength=n)
    assert np.array_equal(cnt, e.debug(6).astype(int)) and np.array_equal(cnt, o.get(104)[:n].astype(int))
    assert E == e.stats()["nnz10"] == e.pairs_device(0, 0, 0, r_cut=-1.0)
    off = np.concatenate([[0], np.cumsum(cnt)])
    rows = np.array([math.fsum(hv[off[i]:off[i + 1]]) for i in range(n)])
    t7, t108 = e.debug(7), o.get(108)[:n]
    print(case, "E", E, "row sums vs tap 7: max rel %.2e, vs tap 108: max rel %.2e" % (np.abs(rows / t7 - 1).max(), np.abs(rows / t108 - 1).max()))
    assert np.allclose(rows, t7, rtol=1e-12, atol=0.0) and np.allclose(rows, t108, rtol=1e-12, atol=0.0)
    assert (np.linalg.norm(vec, axis=1) <= 10.0 * (1 + 1e-12)).all()
    e.close()


# ---- 2b. hval entry by entry ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", ["rdx168", "rdx-shaken"])
def test_hval_entry_by_entry_equals_the_table_lookup(case):
    o = ol.oracle(case, **KW5) if case in ol.SYSTEMS else _oracle(case, (1, 1, 1), **KW5)
    ff = ol.build(case)[0] if case in ol.SYSTEMS else oa.make_system(case)[0]
    tab = qeq_table(o, ff)
    e = _make(case); e.QEq(); e.FORCE()
    typ = e.atoms()["type"]
    E, s, d, sh, vec, hv = device_coo(e, 0.0)
    assert E == e.stats()["nnz10"] and (hv != 0.0).any()
    check_hval_entries(vec, hv, typ[s], typ[d], tab, case)
    e.close()


# ---- 3. order and determinism --------------------------------------------------------------------------------------------------------------
def test_a_cut_off_filters_the_whole_list_in_order_and_two_calls_return_the_same_bits():
    e = _make("rdx-shaken"); e.QEq(); e.FORCE()
    assert not rebuild(e)                          # the slot route
    whole = device_coo(e, 0.0)
    part = device_coo(e, 6.5)
    keep = np.linalg.norm(whole[4], axis=1) <= 6.5
    assert 0 < part[0] < whole[0] and part[0] == int(keep.sum())
    for got, ref in zip(part[1:], whole[1:]):
        assert np.array_equal(got, ref[keep])
    again = device_coo(e, 6.5)
    assert all(np.array_equal(x, y) for x, y in zip(part[1:], again[1:]))
    assert e.pairs_device(0, 0, 0, r_cut=6.5) == part[0]                          # count only
    only = device_coo(e, 6.5, want=(False, False, False))                      # the optional arrays left out: untouched, the others the same
    assert np.array_equal(only[1], part[1]) and np.array_equal(only[2], part[2])
    assert (only[3] == SENT_I).all() and (only[4] == SENT_F).all() and (only[5] == SENT_F).all()
    e.close()


# ---- 4. every layout gives one graph ---------------------------------------------------------------------------------------------------------
VARIANTS = [None, "RXMD_STREAMS_BY_PLACE=0", "RXMD_NB10_ALWAYS=1", "RXMD_SPMV_NO_WIN=1", "RXMD_FORCE_STAGED=1", "RXMD_NO_STAGE_PAIRS=1"]
_DEFAULT = {}


def _layout_run(env, monkeypatch):
    if env:
        k, v = env.split("=")
        monkeypatch.setenv(k, v)                   # (options are read when the engine is created)
    e = _make("rdx-shaken"); e.QEq(); e.FORCE()
    rebuild(e)                                     # the second build of the engine: the layout the options ask for
    st = e.stats()
    flags_before = e.debug(15, cap=2).copy()
    out = dict(part=device_coo(e, 6.5), whole=device_coo(e, 0.0), stats=st, nb10=flags_before, nb10_after=e.debug(15, cap=2).copy())
    if env is None:
        # a call on an engine whose build left the 4-byte entries out must not make later builds write them: the flags of debug tap 15 (written,
        # sticky) stay (0, 0) through the call and through the next build, which reports the same layout; the kernel timers of the list build
        # are not compared -- no statistic counts the stream's bytes, the two flags are what the engine itself decides by (lists.hip: needs_nb10)
        rebuild(e)
        out["nb10_next_build"] = e.debug(15, cap=2).copy(); out["stats_next_build"] = e.stats()
        out["part_next_build"] = device_coo(e, 6.5)
    e.close()
    return out


@pytest.mark.parametrize("env", VARIANTS, ids=[v or "default" for v in VARIANTS])
def test_every_layout_of_the_list_gives_the_same_graph(env, monkeypatch):
    if "run" not in _DEFAULT:
        with pytest.MonkeyPatch.context() as mp:
            for v in VARIANTS[1:]:
                mp.delenv(v.split("=")[0], raising=False)
            _DEFAULT["run"] = _layout_run(None, mp)
    ref = _DEFAULT["run"]
    if env is None:
        st = ref["stats"]
        print("default: streams_by_place", st["streams_by_place"], "win_in_use", st["win_in_use"], "nb10 written / sticky", ref["nb10"], "->", ref["nb10_after"],
              "-> next build", ref["nb10_next_build"])
        assert st["streams_by_place"] == 1 and st["win_in_use"] == 1
        assert list(ref["nb10"]) == [0.0, 0.0], "the default build of this box was expected to leave the 4-byte entries out (the slot route)"
        assert list(ref["nb10_after"]) == [0.0, 0.0] and list(ref["nb10_next_build"]) == [0.0, 0.0]
        assert ref["stats_next_build"]["streams_by_place"] == 1 and ref["stats_next_build"]["win_in_use"] == 1
        assert all(np.array_equal(x, y) for x, y in zip(ref["part"][1:], ref["part_next_build"][1:]))
        return
    run = _layout_run(env, monkeypatch)
    st = run["stats"]
    print(env, ": streams_by_place", st["streams_by_place"], "win_in_use", st["win_in_use"], "nb10 written / sticky", run["nb10"])
    if env == "RXMD_STREAMS_BY_PLACE=0":
        assert st["streams_by_place"] == 0 and st["win_in_use"] == 1 and run["nb10"][0] == 0.0      # slots, rows by atom
    if env == "RXMD_NB10_ALWAYS=1":
        assert st["streams_by_place"] == 1 and run["nb10"][0] == 1.0                                 # entries, rows by place
    if env == "RXMD_SPMV_NO_WIN=1":
        assert st["win_in_use"] == 0 and run["nb10"][0] == 1.0                                       # entries, no windows
    for which in ("part", "whole"):
        assert run[which][0] == ref[which][0]
        for name, got, want in zip(("src", "dst", "shift3", "vec3", "hval"), run[which][1:], ref[which][1:]):
            assert np.array_equal(got, want), "%s: %s differs from the default layout" % (env, name)


# ---- 5. state --------------------------------------------------------------------------------------------------------------------------------
def test_after_steps_the_graph_is_that_of_the_last_force():
    e = _make("rdx168"); e.thermostat(0, 300.0); e.QEq(); e.FORCE(); e.step(3)
    bf = brute_force(e.atoms()["pos"], e.lattice, 6.5)
    check_against_brute_force(e, bf, 6.5, "rdx168 after step(3)")
    e.close()


def test_the_fp32_matrix_stream_exports_widened_floats():
    e = _make("rdx-shaken"); e.set_qeq_precision(32); e.QEq(); e.FORCE()
    assert e.qeq_precision()[0] == 32
    E, s, d, sh, vec, hv = device_coo(e, 0.0)
    assert np.array_equal(hv, hv.astype(np.float32).astype(np.float64)) and (hv != 0).any()
    cnt = np.bincount(s, minlength=e.natoms)
    off = np.concatenate([[0], np.cumsum(cnt)])
    rows = np.array([math.fsum(hv[off[i]:off[i + 1]]) for i in range(e.natoms)])
    assert np.allclose(rows, e.debug(7), rtol=1e-12, atol=0.0)
    e64 = _make("rdx-shaken"); e64.QEq(); e64.FORCE()
    h64 = device_coo(e64, 0.0)[5]
    assert np.array_equal(hv, h64.astype(np.float32).astype(np.float64))          # the double value rounded once
    e.close(); e64.close()


def test_pqeq_engine_in_gid_mode_and_its_longer_reach():
    e = _engine("sicnp", (1, 1, 1), pqeq=oa.PQEQ_SICNP); e.QEq(); e.FORCE()
    bf = brute_force(e.atoms()["pos"], e.lattice, 12.0)
    check_against_brute_force(e, bf, 6.5, "sicnp PQEq, global ids", as_gid=True)
    check_against_brute_force(e, bf, 12.0, "sicnp PQEq, global ids", as_gid=True)     # inside the 12.5 A reach of a PQEq engine
    assert _code(lambda: e.pairs_device(0, 0, 0, r_cut=12.6)) == -1
    E, s, d, sh, vec, hv = device_coo(e, 0.0)
    assert np.allclose(np.bincount(s, weights=hv, minlength=e.natoms), e.debug(7), rtol=1e-10, atol=0.0)
    e.close()
    plain = _make("rdx168"); plain.QEq(); plain.FORCE()
    assert plain.pairs_device(0, 0, 0, r_cut=10.0) > 0
    assert _code(lambda: plain.pairs_device(0, 0, 0, r_cut=12.0)) == -1
    plain.close()


# ---- 6. refusals and capacity ------------------------------------------------------------------------------------------------------------------
def test_capacity_and_refusals():
    e = _make("rdx168")
    buf = torch.zeros(8, dtype=torch.int64, device=DEV); p = buf.data_ptr()
    assert _code(lambda: e.pairs_device(0, 0, 0)) == -7                         # no list yet
    e.QEq()
    Eq = e.pairs_device(0, 0, 0, r_cut=6.5)                                      # the list of a QEq call alone will do
    e.FORCE()
    E = e.pairs_device(0, 0, 0, r_cut=6.5)
    assert E == Eq == 19676
    got = device_coo(e, 6.5, capacity=E - 1)
    assert got[0] == E and all((x == SENT_I).all() for x in got[1:4]) and all((x == SENT_F).all() for x in got[4:])
    got = device_coo(e, 6.5, capacity=E + 5)
    assert got[0] == E and all((x[:E] != SENT_I).all() for x in got[1:3]) and all((x[:E] != SENT_F).all() for x in got[4:])
    assert all((x[E:] == SENT_I).all() for x in got[1:4]) and all((x[E:] == SENT_F).all() for x in got[4:])
    e.set_lattice(e.lattice)
    assert _code(lambda: e.pairs_device(0, 0, 0)) == -7                         # the lists are stale
    e.QEq(); e.FORCE()
    assert e.pairs_device(0, 0, 0, r_cut=6.5) == E
    e.set_atoms_rxff(e.get_atoms_rxff())
    assert _code(lambda: e.pairs_device(0, 0, 0)) == -7
    e.QEq(); e.FORCE()
    raw = lambda flags, r_cut, cap, s, d: e._chk(e.L.rxmd_hip_get_pairs_device(e.h, flags, r_cut, cap, s, d, None, None, None, None))
    assert _code(lambda: raw(2, 0.0, 8, p, p)) == -1                            # unknown flag bit
    assert _code(lambda: raw(3, 0.0, 0, None, None)) == -1
    assert _code(lambda: e.pairs_device(-1, p, p)) == -1                        # negative capacity
    assert _code(lambda: e.pairs_device(-1, 0, 0)) == -1
    assert _code(lambda: e.pairs_device(0, 0, 0, r_cut=float("nan"))) == -1
    assert _code(lambda: e.pairs_device(0, 0, 0, r_cut=float("inf"))) == -1
    assert _code(lambda: e.pairs_device(0, 0, 0, r_cut=float("-inf"))) == -1
    assert _code(lambda: e.pairs_device(0, 0, 0, r_cut=10.0 + 1e-9)) == -1      # beyond the reach of the list
    assert _code(lambda: e.pairs_device(8, p, 0)) == -1                         # src without dst
    assert _code(lambda: e.pairs_device(8, 0, p)) == -1
    assert (buf == 0).all()
    e.close()
    # local indices or shifts on an engine of a decomposed box: an argument error, raised before the state is looked at (no atoms, no transport)
    import rxmd_amd
    ff, names, frac, lat = oa.make_system("rdx168")
    e2 = rxmd_amd.RxmdEngine(ff, lat, vprocs=(2, 1, 1))
    assert _code(lambda: e2.pairs_device(0, 0, 0)) == -1
    assert _code(lambda: e2.pairs_device(8, p, p)) == -1
    assert _code(lambda: e2.pairs_device(8, p, p, shift_ptr=p, as_gid=True)) == -1
    assert _code(lambda: e2.pairs_device(8, p, p, vec_ptr=p, h_ptr=p, as_gid=True)) == -7   # global ids with vec3 / hval are fine there: only the state is missing
    e2.close()


# ---- 7. torch ----------------------------------------------------------------------------------------------------------------------------------
def _torch_case(shift, case="rdx168", **kw):
    """the system handed over in a random permutation (gid = the original ids), optionally every atom moved by a lattice vector"""
    r = _ref(case, (1, 1, 1))
    n = len(r["pos"])
    rng = np.random.default_rng(20250314)
    perm = rng.permutation(n)
    pos = r["pos"][perm]
    if shift:
        pos = pos + rng.integers(-3, 4, size=(n, 3)).astype(np.float64) @ hmat(r["lat"]).T
    m = _model(dict(r, type=r["type"][perm], gid=r["gid"][perm]), **kw)
    return r, m, perm, pos, _dev(pos)


@pytest.mark.parametrize("shift", [False, True], ids=["caller-order", "anywhere-in-space"])
def test_torch_graph_for_the_callers_positions(shift):
    r, m, perm, pos, tpos = _torch_case(shift)
    import rxmd_amd
    with pytest.raises(rxmd_amd.RxmdError) as ei:
        m.pair_graph(6.5)
    assert ei.value.code == -7
    m.evaluate(tpos)
    g0 = m.pair_graph(6.5, values=True)                        # the engine's own arrays
    g = m.pair_graph(6.5, pos=tpos)
    E = g0["vec"].shape[0]
    assert E == 19676 and set(g0) == {"edge_index", "shifts", "vec", "h"} and set(g) == {"edge_index", "shifts", "vec"}
    assert g0["edge_index"].dtype == torch.int64 and g0["edge_index"].shape == (2, E) and g0["shifts"].dtype == torch.int64 and g0["shifts"].shape == (E, 3)
    assert g0["vec"].dtype == torch.float64 and g0["vec"].shape == (E, 3) and g0["h"].dtype == torch.float64 and g0["h"].shape == (E,)
    assert all(t.device == m.device and not t.requires_grad for t in g0.values())
    assert torch.equal(g["edge_index"], g0["edge_index"])
    src, dst = g["edge_index"]
    cell = torch.tensor(hmat(r["lat"]).T, dtype=torch.float64, device=DEV)
    assert (m.cell() - cell).abs().max().item() <= 1e-13
    mine = tpos[dst] - tpos[src] + g["shifts"].double() @ cell   # vec from the caller's pos and the returned shifts
    err = (mine - g0["vec"]).abs().max().item()
    print("shifted" if shift else "in the box", ": max |vec(pos, shifts) - vec3| %.2e A; edges whose shift changed %d" % (err, int((g["shifts"] != g0["shifts"]).any(dim=1).sum())))
    assert err <= 1e-12 and (g["vec"] - g0["vec"]).abs().max().item() <= 1e-12
    if not shift:
        assert torch.equal(g["shifts"], g0["shifts"])          # inside the box the caller's positions are the engine's
    else:
        assert (g["shifts"] != g0["shifts"]).any()
    # the same graph as the brute force over the caller's positions wrapped by the engine
    keys = torch.cat([g0["edge_index"].T, g0["shifts"]], dim=1).cpu().numpy()
    bf = brute_force(m.engine.atoms()["pos"], r["lat"], 6.5)
    assert np.array_equal(keys[np.lexsort(keys.T[::-1])], _select(bf, 6.5)[0])
    none = m.pair_graph(1e-3, values=True)                     # nothing selected: empty tensors of the documented shapes
    assert none["edge_index"].shape == (2, 0) and none["shifts"].shape == (0, 3) and none["vec"].shape == (0, 3) and none["h"].shape == (0,)
    m.close()


def test_torch_vec_is_differentiable_in_pos_and_cell():
    r, m, perm, pos, tpos = _torch_case(True)
    p = tpos.clone().requires_grad_(True)
    m.evaluate(p)
    cell = m.cell().requires_grad_(True)
    g = m.pair_graph(6.5, pos=p, cell=cell)
    assert g["vec"].requires_grad and not g["shifts"].requires_grad and not g["edge_index"].requires_grad
    loss = (g["vec"] ** 2).sum()
    gp, gc = torch.autograd.grad(loss, (p, cell))
    src, dst = g["edge_index"]
    v = g["vec"].detach()
    closed = 2.0 * (torch.zeros_like(tpos).index_add_(0, dst, v) - torch.zeros_like(tpos).index_add_(0, src, v))
    err = (gp - closed).abs().max().item()
    closed_cell = 2.0 * g["shifts"].double().T @ v
    err_c = (gc - closed_cell).abs().max().item() / max(closed_cell.abs().max().item(), 1.0)
    print("d sum|vec|^2 / dpos against the closed form: max abs %.2e (largest component %.2e); d / dcell: rel %.2e" % (err, closed.abs().max().item(), err_c))
    assert err <= 1e-9 and err_c <= 1e-12
    m.close()


def test_torch_graph_on_a_side_stream():
    r, m, perm, pos, tpos = _torch_case(False)
    m.evaluate(tpos)
    ref = m.pair_graph(6.5, pos=tpos, values=True)
    ref_sum = (ref["h"].sum(), ref["vec"].abs().sum(), ref["edge_index"].sum())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.randn(2048, 2048, device=DEV) @ torch.randn(2048, 2048, device=DEV)   # work in front of the producer on this stream
        p = tpos + 0.0 * big[0, 0].double()                                                # the input is produced on s ...
        m.evaluate(p)
        g = m.pair_graph(6.5, pos=p, values=True)
        side_sum = (g["h"].sum(), g["vec"].abs().sum(), g["edge_index"].sum())             # ... and the graph reduced there
        side = {k: v * 1 for k, v in g.items()}
    s.synchronize()
    assert torch.isfinite(big).all()
    for k in ref:
        assert torch.equal(side[k], ref[k]), k
    assert all(torch.equal(a, b) for a, b in zip(side_sum, ref_sum))
    m.close()


def test_exported_matrix_is_the_qeq_operator_of_the_converged_charges():
    """chi + H q is the same number on every atom at the solution of QEq (the Lagrange multiplier of the charge constraint); H = eta on the diagonal
    + the exported COO values.  Measured on one MI355X (NOTES.md): see the values the test prints."""
    from rxmd_amd import system
    r, m, perm, pos, tpos = _torch_case(False, **TIGHT)
    out = m.evaluate(tpos)
    g = m.pair_graph(0.0, values=True)
    n = m.natoms
    info = np.zeros(64)
    L = m.engine.L
    import ctypes as C
    L.rxmd_host_ffield_table(str(r["ff"]).encode(), None, 6, info.ctypes.data_as(C.c_void_p), 64)
    nso = int(info[0])
    chi_t, eta_t = info[5:5 + nso], info[5 + nso:5 + 2 * nso]
    typ = r["type"][perm]
    chi = torch.tensor(chi_t[typ - 1], dtype=torch.float64, device=DEV); eta = torch.tensor(eta_t[typ - 1], dtype=torch.float64, device=DEV)
    H = torch.sparse_coo_tensor(g["edge_index"], g["h"], (n, n)).coalesce()           # (a pair through several images: the values add up)

    def spread(q):
        mu = chi + eta * q + torch.sparse.mm(H, q[:, None])[:, 0]
        return (mu.max() - mu.min()).item(), mu.mean().item()

    s_engine, mu_engine = spread(out["charges"])
    s_oracle, mu_oracle = spread(torch.tensor(r["q"][perm], dtype=torch.float64, device=DEV))
    print("spread of chi + H q over the atoms: engine's charges %.3e, oracle's charges %.3e (mean %.6f / %.6f)" % (s_engine, s_oracle, mu_engine, mu_oracle))
    assert s_oracle < 1e-3 * abs(mu_oracle), "the exported matrix is not the operator the oracle's charges solve"
    assert s_engine <= 10.0 * s_oracle
    m.close()
