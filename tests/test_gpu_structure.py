"""rxmd_hip_structure_* and its mirror (RxmdEngine.structure_begin / _sample / _counts / _end): partial pair counts and bond-angle counts accumulated
on the device from the 10 A list.

The yardstick is structure_reference.py: the brute force over all images of test_gpu_pair_graph.py, from the positions, types and lattice the SAME
engine reports, binned in numpy by the formulas of the header.  Its rules (check_counts): L1(device, brute force) <= 2 x near-edge increments per
array, sums over the bins exact per type pair and per shell and type triple once no distance lies within 1e-8 A of r_max or a shell cut, near-edge
share <= 1e-5 on the disordered boxes.  Everything else here is exact: counts are integers.

Shapes: rdx168 (rows of ~366 entries: several 64-lane batches; edges below 2 r_max: partners repeat through images; first build = 4-byte entries),
rdx168-z9.42 (an atom meets its own image), rdx-denser (up to 238 neighbours inside 6 A: more than one staging tile of 128; 1,048-entry rows),
rdx-dilute (167 angles in the 2 A shell, most triples empty, one atom without a bond; its second build walks the window slots), mos2_tri324
(triclinic, types 2 and 3 only, empty 2 A shell, angles exactly on bin edges).  The binnings of test_binnings_on_rdx168 are the sizes at which the
kernels take another path: every row type in one walk of the LDS histogram, several walks, and no LDS at all (structure.hip: SP_HCAP, SA_HCAP)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle_api as oa
import offlattice_systems as ol
import structure_reference as sr
import structure_worker
from ranks import run_ranks
from npt_reference import hmat
from parity import _engine, build_system, rec10, code as _code
from graph_support import _make, rebuild, brute_force, KW5

pytestmark = pytest.mark.gpu

_BF = {}


def _nso(e):
    return e._nso()


def _reference(e, key, r_bf):
    """brute force over the engine's own positions, once per key, read-only"""
    if key not in _BF:
        a = e.atoms()
        bf = brute_force(a["pos"], e.lattice, r_bf)
        for arr in bf:
            arr.setflags(write=False)
        _BF[key] = (bf, a["type"].astype(np.int64) - 1)
    return _BF[key]


def _sample_once(e, r_max, nbr, cuts, nba):
    e.structure_begin(r_max, nbr, cuts, nba)
    e.structure_sample()
    return e.structure_counts()


def _volume(lat):
    return abs(np.linalg.det(hmat(lat)))


def _check_sums(e, c, frames=1):
    t = e.atoms()["type"]
    assert c["frames"] == frames
    assert np.array_equal(c["atoms_per_type"], frames * np.bincount(t - 1, minlength=_nso(e)))
    assert abs(c["volume_sum"] - frames * _volume(e.lattice)) <= 1e-12 * c["volume_sum"]


def _check_increment(e, before, after, label):
    """what the samples between two reads added is the brute-force structure of the engine's present positions (one sample) -> that increment"""
    a = e.atoms()
    bf = brute_force(a["pos"], e.lattice, sr.R_MAX)
    type0 = a["type"].astype(np.int64) - 1
    nso = _nso(e)
    inc = {k: after[k] - before[k] for k in ("pair_counts", "angle_counts", "atoms_per_type")}
    sr.check_counts(label, inc["pair_counts"], inc["angle_counts"], sr.bin_pairs(bf, type0, nso, sr.R_MAX, sr.NBINS_R),
                    sr.bin_angles(bf, type0, nso, sr.SHELLS, sr.NBINS_A), disordered=False)
    assert np.array_equal(inc["atoms_per_type"], np.bincount(type0, minlength=nso))
    return inc


# ---- 1. shapes against the brute force -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rdx168", "rdx168-z9.42", "rdx-denser", "rdx-dilute", "mos2_tri324"])
def test_counts_equal_the_brute_force(case):
    e = _make(case); e.QEq(); e.FORCE()
    st = e.stats()
    bf, type0 = _reference(e, case, sr.R_MAX)
    nso = _nso(e)
    ref_p = sr.bin_pairs(bf, type0, nso, sr.R_MAX, sr.NBINS_R)
    ref_a = sr.bin_angles(bf, type0, nso, sr.SHELLS, sr.NBINS_A)
    print(case, "natoms", st["natoms"], "longest row", st["max_n10"], "nso", nso)
    first = None
    for build in ("first build", "second build"):
        if build == "second build":
            entries = rebuild(e)
            print(case, "second build: 4-byte entries written", entries, "streams_by_place", e.stats()["streams_by_place"])
            if case == "rdx-dilute":
                assert not entries                             # the window-slot route
        c = _sample_once(e, sr.R_MAX, sr.NBINS_R, sr.SHELLS, sr.NBINS_A)
        assert c["pair_counts"].shape == (nso, nso, sr.NBINS_R) and c["angle_counts"].shape == (3, nso, nso, nso, sr.NBINS_A)
        sr.check_counts(case + ", " + build, c["pair_counts"], c["angle_counts"], ref_p, ref_a, disordered=case in ol.SYSTEMS)
        _check_sums(e, c)
        if first is None:
            first = c
        else:                                                  # the same positions through another layout: the same counts
            assert np.array_equal(c["pair_counts"], first["pair_counts"]) and np.array_equal(c["angle_counts"], first["angle_counts"])
    ang = c["angle_counts"]
    if case == "rdx168-z9.42":                                 # every atom is its own partner one box up and one box down
        own = bf[0][(bf[0][:, 0] == bf[0][:, 1]) & (bf[2] < sr.R_MAX)]
        assert len(own) == 2 * 168
    if case == "rdx-denser":
        inside = np.bincount(bf[0][bf[2] < sr.SHELLS[-1], 0])
        print("rdx-denser: most neighbours inside 6 A:", inside.max())
        assert inside.max() > 128 and st["max_n10"] > 1024     # more than one staging tile
    if case == "rdx-dilute":
        assert ref_a["samples"][0] == 167 and ang[0].sum() == 2 * 167
    if case == "mos2_tri324":
        assert ang[0].sum() == 0 and ref_a["samples"][0] == 0   # the empty 2 A shell
        used = sorted(set(type0))
        assert used == [1, 2]                                  # the ffield's types 2 and 3
        for t in set(range(nso)) - set(used):                  # whole rows and columns stay zero
            assert c["pair_counts"][t].sum() == 0 and c["pair_counts"][:, t].sum() == 0
            assert ang[:, t].sum() == 0 and ang[:, :, t].sum() == 0 and ang[:, :, :, t].sum() == 0 and c["atoms_per_type"][t] == 0
    e.structure_end(); e.close()


@pytest.mark.parametrize("binning", [(10.0, 1000, (2.0, 4.0, 6.0), 180),     # the reference's own settings: 0.01 A bins; all 16 pair slices in one walk
                                     (10.0, 1000, (), 180),                   # no shells
                                     (9.5, 190, (2.0, 4.0, 6.0), 1),          # one angle bin: every centre type in one walk
                                     (9.5, 2000, (6.0,), 180),                # two row types per pair walk, three centre types per angle walk
                                     (9.5, 4096, (1.5, 3.0, 4.5, 6.0), 360)],  # no slice fits either LDS histogram: global atomics; four shells
                         ids=["reference", "noshells", "oneanglebin", "twowalks", "global"])
def test_binnings_on_rdx168(binning):
    r_max, nbr, cuts, nba = binning
    e = _make("rdx168"); e.QEq(); e.FORCE()
    bf, type0 = _reference(e, "rdx168@10", 10.0)
    nso = _nso(e)
    c = _sample_once(e, r_max, nbr, cuts, nba)
    ref_p = sr.bin_pairs(bf, type0, nso, r_max, nbr)
    ref_a = sr.bin_angles(bf, type0, nso, cuts, nba) if cuts else None
    assert c["angle_counts"].shape == (len(cuts), nso, nso, nso, nba if cuts else 0)
    sr.check_counts("rdx168 %r" % (binning,), c["pair_counts"], c["angle_counts"], ref_p, ref_a, disordered=False)
    _check_sums(e, c)
    e.structure_end(); e.close()


@pytest.mark.parametrize("env", ["RXMD_STREAMS_BY_PLACE=0", "RXMD_NB10_ALWAYS=1", "RXMD_SPMV_NO_WIN=1"])
def test_every_layout_of_the_list_gives_identical_counts(env, monkeypatch):
    def run():
        e = _make("rdx168"); e.QEq(); e.FORCE(); rebuild(e)
        c = _sample_once(e, sr.R_MAX, sr.NBINS_R, sr.SHELLS, sr.NBINS_A)
        st = e.stats(); nb10 = e.debug(15, cap=2)[0]
        e.close()
        return c, st, nb10
    if "default" not in _BF:
        with pytest.MonkeyPatch.context() as m:
            for v in ("RXMD_STREAMS_BY_PLACE", "RXMD_NB10_ALWAYS", "RXMD_SPMV_NO_WIN"):
                m.delenv(v, raising=False)
            _BF["default"] = run()
    ref, st0, _ = _BF["default"]
    k, v = env.split("=")
    monkeypatch.setenv(k, v)                       # (options are read when the engine is created)
    c, st, nb10 = run()
    print(env, ": streams_by_place", st["streams_by_place"], "win_in_use", st["win_in_use"], "nb10 written", nb10)
    if env == "RXMD_STREAMS_BY_PLACE=0":
        assert st["streams_by_place"] == 0
    if env == "RXMD_NB10_ALWAYS=1":
        assert nb10 == 1.0
    if env == "RXMD_SPMV_NO_WIN=1":
        assert st["win_in_use"] == 0
    assert c["pair_counts"].sum() > 0 and c["angle_counts"].sum() > 0
    assert np.array_equal(c["pair_counts"], ref["pair_counts"]) and np.array_equal(c["angle_counts"], ref["angle_counts"])
    assert np.array_equal(c["atoms_per_type"], ref["atoms_per_type"])


# ---- 2. accumulation and state ---------------------------------------------------------------------------------------------------------------------
def test_samples_accumulate_and_follow_the_last_force_of_step():
    e = _make("rdx168"); e.thermostat(0, 300.0); e.QEq(); e.FORCE()
    e.structure_begin(sr.R_MAX, sr.NBINS_R, sr.SHELLS, sr.NBINS_A)
    e.structure_sample()
    one = e.structure_counts()
    e.structure_sample()
    two = e.structure_counts()
    for k in ("pair_counts", "angle_counts", "atoms_per_type"):
        assert np.array_equal(two[k], 2 * one[k]), k          # the same state twice: identical counts
    assert two["frames"] == 2 and two["volume_sum"] == 2 * one["volume_sum"]
    assert np.array_equal(e.structure_counts()["pair_counts"], two["pair_counts"])       # reading does not reset
    e.step(3)
    e.structure_sample()
    three = e.structure_counts()
    _check_sums(e, three, frames=3)
    # the increment is the structure of the positions the engine reports now: those of the last step's FORCE
    fresh = _check_increment(e, two, three, "rdx168 after step(3)")
    assert not np.array_equal(fresh["pair_counts"], one["pair_counts"])                   # the atoms did move
    e.structure_begin(sr.R_MAX, sr.NBINS_R)                     # begin again: replaced, from zero, no shells
    z = e.structure_counts()
    assert z["frames"] == 0 and z["volume_sum"] == 0.0 and z["pair_counts"].sum() == 0 and z["angle_counts"].size == 0 and z["atoms_per_type"].sum() == 0
    e.structure_sample()
    assert np.array_equal(e.structure_counts()["pair_counts"], fresh["pair_counts"])
    e.structure_end(); e.close()


def test_variable_cell_books_the_new_volume_and_keeps_the_accumulators():
    e = _make("rdx168"); e.QEq(); e.FORCE()
    e.structure_begin(sr.R_MAX, sr.NBINS_R, sr.SHELLS, sr.NBINS_A)
    e.structure_sample()
    one = e.structure_counts()
    lat0 = e.lattice
    v0 = _volume(lat0)
    lat1 = [lat0[0] * 1.03, lat0[1] * 0.99, lat0[2] * 1.02] + list(lat0[3:])
    e.set_lattice(lat1)
    assert _code(e.structure_sample) == -7                     # the list is stale
    same = e.structure_counts()
    assert same["frames"] == 1 and np.array_equal(same["pair_counts"], one["pair_counts"])       # the accumulators persist, the refused sample added nothing
    e.set_qeq_precision(32); e.set_qeq_precision(64)
    e.QEq(); e.FORCE()
    e.structure_sample()
    two = e.structure_counts()
    v1 = _volume(e.lattice)
    assert abs(v1 / v0 - 1.03 * 0.99 * 1.02) < 1e-12
    assert two["frames"] == 2 and abs(two["volume_sum"] - (v0 + v1)) <= 1e-12 * (v0 + v1)
    _check_increment(e, one, two, "rdx168 strained")           # the strained box, from the positions and the lattice the engine reports
    e.set_atoms_rxff(e.get_atoms_rxff())                       # set_atoms between samples: the accumulators persist
    assert _code(e.structure_sample) == -7
    e.QEq()                                                    # the list of a QEq call alone will do
    e.structure_sample()
    three = e.structure_counts()
    assert three["frames"] == 3 and abs(three["volume_sum"] - (v0 + 2 * v1)) <= 1e-12 * three["volume_sum"]
    _check_increment(e, two, three, "rdx168 strained, atoms set again")
    e.structure_end(); e.close()


# ---- 3. ranks ------------------------------------------------------------------------------------------------------------------------------------


def test_rank_summed_counts_equal_the_single_rank_counts(tmp_path):
    from rxmd_amd import structure
    base = dict(case="rdx222", mc=(2, 2, 2), shaken=(2048, 0.05), kw=KW5, begin=(sr.R_MAX, sr.NBINS_R, sr.SHELLS, sr.NBINS_A), dir=str(tmp_path))
    spec = dict(base, vp=(2, 1, 1))
    run_ranks(structure_worker.structure_rank, 2, spec, timeout=600)
    dicts = []
    for r in range(2):
        with np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) as f:
            assert str(f["transport_error"]) == "None" and bool(f["doubled"]) and int(f["messages_of_a_sample"]) == 0      # no collective, no message
            dicts.append(dict(pair_counts=f["pair_counts"], angle_counts=f["angle_counts"], atoms_per_type=f["atoms_per_type"], volume_sum=float(f["volume_sum"]),
                              frames=int(f["frames"]), r_max=sr.R_MAX, angle_cuts=list(sr.SHELLS), natoms=int(f["natoms"])))
    print("residents per rank", [d["natoms"] for d in dicts], "pair counts per rank", [int(d["pair_counts"].sum()) for d in dicts])
    assert all(d["natoms"] > 0 for d in dicts) and sum(d["natoms"] for d in dicts) == 1344
    whole = structure.merge(dicts)
    import rxmd_amd
    ff, lat, ranks, vs = build_system(dict(base, vp=(1, 1, 1)))
    e = rxmd_amd.RxmdEngine(ff, lat, **KW5)
    e.set_atoms_rxff(rec10(ranks[0])); e.QEq(); e.FORCE()
    one = _sample_once(e, sr.R_MAX, sr.NBINS_R, sr.SHELLS, sr.NBINS_A)
    for k in ("pair_counts", "angle_counts", "atoms_per_type"):
        assert np.array_equal(whole[k], one[k]), k
    assert whole["frames"] == one["frames"] == 1 and abs(whole["volume_sum"] - one["volume_sum"]) <= 1e-12 * one["volume_sum"]
    assert one["pair_counts"].sum() > 400000 and one["angle_counts"][-1].sum() > 1000000
    e.structure_end(); e.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_capacity():
    e = _make("rdx168")
    L, h = e.L, e.h
    assert _code(e.structure_sample) == -7                     # no begin
    assert _code(lambda: e._chk(L.rxmd_hip_structure_get(h, None, 0, None, 0, None, None, None))) == -7
    e.structure_end()                                          # nothing to do
    cuts = lambda *c: np.array(c, np.float64)
    begin = lambda r_max, nbr, nsh, cut, nba: e._chk(L.rxmd_hip_structure_begin(h, r_max, nbr, nsh, None if cut is None else cut.ctypes.data, nba))
    for bad in [(0.0, 100, 0, None, 0), (-1.0, 100, 0, None, 0), (float("nan"), 100, 0, None, 0), (float("inf"), 100, 0, None, 0), (10.0 + 1e-9, 100, 0, None, 0),
                (9.5, 0, 0, None, 0), (9.5, 4097, 0, None, 0), (9.5, 100, -1, None, 0), (9.5, 100, 5, cuts(1, 2, 3, 4, 5), 180),
                (9.5, 100, 2, None, 180), (9.5, 100, 2, cuts(2, 2), 180), (9.5, 100, 2, cuts(4, 2), 180), (9.5, 100, 1, cuts(0.0), 180),
                (9.5, 100, 1, cuts(9.6), 180), (9.5, 100, 1, cuts(float("nan")), 180), (9.5, 100, 1, cuts(6), 0), (9.5, 100, 1, cuts(6), 361)]:
        assert _code(lambda: begin(*bad)) == -1, bad
    assert _code(e.structure_sample) == -7                     # a refused begin left no accumulators
    begin(10.0, 4096, 4, cuts(2, 4, 6, 10.0), 360)             # the limits themselves are fine
    begin(9.5, 1, 0, None, -5)                                 # no shells: nbins_angle is not looked at
    e.structure_begin(9.5, 190, (2.0, 4.0, 6.0), 180)
    assert _code(e.structure_sample) == -7                     # no list yet
    e.QEq()
    e.structure_sample()                                       # the list of a QEq call alone will do
    e.FORCE()
    nso = _nso(e)
    npair, nang = nso * nso * 190, 3 * nso ** 3 * 180
    SENT = -777
    pair = np.full(npair + 3, SENT, np.int64); ang = np.full(nang + 3, SENT, np.int64); npt = np.full(nso + 3, SENT, np.int64)
    get = lambda pc, ac: e._chk(L.rxmd_hip_structure_get(h, pair.ctypes.data, pc, ang.ctypes.data, ac, npt.ctypes.data, None, None))
    assert _code(lambda: get(npair - 1, nang)) == -1 and _code(lambda: get(npair, nang - 1)) == -1 and _code(lambda: get(0, 0)) == -1
    assert (pair == SENT).all() and (ang == SENT).all() and (npt == SENT).all()                 # a short capacity writes nothing
    get(npair + 3, nang + 3)
    assert (pair[:npair] >= 0).all() and pair[:npair].sum() > 0 and (pair[npair:] == SENT).all() and (ang[nang:] == SENT).all() and (npt[nso:] == SENT).all()
    assert npt[:nso].sum() == 168
    fr = np.zeros(1, np.int64)
    e._chk(L.rxmd_hip_structure_get(h, None, 0, None, 0, None, None, fr.ctypes.data_as(C.POINTER(C.c_longlong))))   # any pointer may be NULL
    assert fr[0] == 1
    e.structure_end()
    assert _code(e.structure_sample) == -7
    e.close()


def test_pqeq_engine_and_its_longer_reach():
    e = _engine("sicnp", (1, 1, 1), pqeq=oa.PQEQ_SICNP); e.QEq(); e.FORCE()
    assert _code(lambda: e.structure_begin(12.6, 126)) == -1
    bf, type0 = _reference(e, "sicnp", 12.5)
    nso = _nso(e)
    c = _sample_once(e, 12.5, 250, (2.0, 3.5), 90)
    sr.check_counts("sicnp PQEq", c["pair_counts"], c["angle_counts"], sr.bin_pairs(bf, type0, nso, 12.5, 250), sr.bin_angles(bf, type0, nso, (2.0, 3.5), 90), disordered=False)
    _check_sums(e, c)
    e.structure_end(); e.close()
    plain = _make("rdx168")
    assert _code(lambda: plain.structure_begin(12.5, 125)) == -1
    plain.close()
