"""Work whose result nothing reads, left out: the 4-byte entry stream of the 10 A list when every kernel of the build reads the 2-byte window
slots (RXMD_NB10_ALWAYS=1 keeps it), and ENbond's pair and self energies on the steps of a step(n) call behind which nobody reads energies.
Neither changes a force, a charge, a row sum or an iteration count.

How "the same" is judged here.  The only additions of FORCE whose order is not fixed are atomics: the acceptor forces of the hydrogen-bond sweep
and the per-workgroup energy and virial sums.  Two runs of ONE configuration therefore differ in last bits wherever those reach, and after a
step also in everything downstream of the forces.  Every comparison across configurations is held to that spread, measured in the same test
from runs of one configuration: the difference may be at most 4 x the spread (two maxima of the same distribution), and where the spread
is zero the quantities must be equal.  On these small boxes a last-bit difference is a rare event of a run, so the spread is taken over NSPREAD
runs (the largest difference between any two of them), not over two: two runs agree exactly more often than not.
"""
import os
import numpy as np
import pytest

import oracle_api as oa
from parity import FTOL, ETOL, f_err, e_err

pytestmark = pytest.mark.gpu

KW = dict(QEq_tol=1e-12, NMAXQEq=2000, qeq_mode=1)
NSPREAD = 6


def _ice_perturbed():
    """ice Ih with the benchmark's kick (the file holds exactly collinear O-H...O triples): Gaussian, sigma 0.02 A, default_rng(12345)"""
    lines = open(os.path.join(oa.INP, "ice-1h_real.xyz")).read().split("\n")
    n0 = int(lines[0].split()[0]); lat = [float(x) for x in lines[1].split()[:6]]
    rng = np.random.default_rng(12345)
    names, frac = [], []
    for l in lines[2:2 + n0]:
        el, x, y, z = l.split()[:4]
        names.append(el); frac.append((np.array([float(x), float(y), float(z)]) + rng.normal(0.0, 0.02, 3)) / np.array(lat[:3]))
    return os.path.join(oa.INP, "ffield_water"), names, np.array(frac), lat


def _system(case):
    return _ice_perturbed() if case == "ice" else oa.make_system(case)


def _engine(case, mc, monkeypatch, always, env=(), **kw):
    import rxmd_amd
    from rxmd_amd import system
    for k in ("RXMD_NB10_ALWAYS", "RXMD_NONBOND_WIN", "RXMD_SPMV_WIN"):
        monkeypatch.delenv(k, raising=False)
    if always:
        monkeypatch.setenv("RXMD_NB10_ALWAYS", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    ff, names, frac, lat = _system(case)
    lat3, rec = system.geninit(ff, names, frac, lat, mc=mc)
    e = rxmd_amd.RxmdEngine(ff, lat3, **dict(KW, **kw))
    e.set_atoms_rxff(rec)
    return e


def _stream(e):
    """(the last list build wrote the 4-byte entries, a reader once found them missing)"""
    v = e.debug(15, cap=2)
    return bool(v[0]), bool(v[1])


def _run(case, mc, monkeypatch, always, nsteps=3):
    """QEq(); FORCE(); step(nsteps) -> the state behind FORCE and behind the steps"""
    e = _engine(case, mc, monkeypatch, always)
    n = e.natoms
    e.set_velocities(np.random.default_rng(7).normal(0.0, 0.02, (n, 3)))
    it0, est0 = e.QEq(); pe0 = e.FORCE().copy(); a0 = e.atoms()
    out = dict(it0=it0, q0=a0["q"].copy(), f0=a0["f"].copy(), pe0=pe0, rows0=e.debug(7).copy(), n100=e.debug(6).copy(), stream0=_stream(e), win=e.stats()["win_in_use"])
    e.energy()                                   # (reads and clears the stress accumulators: astr below is the steps' own)
    e.step(nsteps)
    a = e.atoms(); en = e.energy()
    out.update(q=a["q"].copy(), f=a["f"].copy(), pos=a["pos"].copy(), v=a["v"].copy(), pe=en["PE"].copy(), astr=en["astr"].copy(), rows=e.debug(7).copy(),
               iters=e.stats()["qeq_iters_total"], stream=_stream(e))
    e.close()
    return out


def _within(name, x, refs, report):
    """|x - refs[0]| <= 4 max |refs[i] - refs[j]| (refs: runs of one configuration), equality where they all agree"""
    refs = [np.asarray(r, float) for r in refs]
    spread = max(float(np.abs(a - b).max()) for n, a in enumerate(refs) for b in refs[n + 1:]); cross = float(np.abs(np.asarray(x, float) - refs[0]).max())
    report.append("%s: cross %.3e spread %.3e" % (name, cross, spread))
    print(report[-1])
    assert cross <= 4.0 * spread, report[-1]


def _stream_off_equals_stream_on(case, mc, monkeypatch, expect_off):
    ons = [_run(case, mc, monkeypatch, True) for _ in range(NSPREAD)]; off = _run(case, mc, monkeypatch, False)
    on1, on2 = ons[0], ons[1]
    assert all(o["stream0"][0] and o["stream"][0] for o in ons)
    # the first build of an engine has no earlier windows to count on; from the second build on the default leaves the entries out -- unless the box
    # is one in which an atom meets its own image (row forms, self-image flag: the entries are read)
    assert off["stream0"] == (True, False) and off["stream"] == ((not expect_off), False), (off["stream0"], off["stream"])
    assert off["win"] == on1["win"] == 1          # (the matrix pass runs over the windows in every box; the self-image check sends ENbond alone to its row form)
    rep = []
    # behind QEq + FORCE nothing has moved yet: charges, row sums, row lengths and the iteration count exactly
    for k in ("q0", "rows0", "n100"):
        assert np.array_equal(off[k], on1[k]) and np.array_equal(on2[k], on1[k]), k
    assert off["it0"] == on1["it0"] == on2["it0"]
    _within("f0", off["f0"], [o["f0"] for o in ons], rep)
    _within("pe0", off["pe0"], [o["pe0"] for o in ons], rep)
    # behind three steps: exactly where two runs of one configuration agree exactly, within their spread elsewhere
    assert off["iters"] == on1["iters"] or len(set(o["iters"] for o in ons)) > 1, (off["iters"], [o["iters"] for o in ons])
    for k in ("q", "rows", "f", "pos", "pe", "astr"):
        _within(k, off[k], [o[k] for o in ons], rep)
    assert off["pe"][11] != 0.0 and off["pe"][12] != 0.0
    return rep


def test_stream_off_equals_stream_on(monkeypatch):
    """RDX 3 x 3 x 3 (4,536 atoms: window groups in the interior and groups with image partners).  QEq(); FORCE(); step(3) with the entry stream
    always written (twice: the spread) and with the default."""
    _stream_off_equals_stream_on("rdx333", (3, 3, 3), monkeypatch, True)


def test_stream_off_equals_stream_on_rdx222(monkeypatch):
    """RDX 2 x 2 x 2 (1,344 atoms; 26.4 x 23.1 x 21.4 A: every edge just above two cut-offs + 1 A, so the window forms still run and every group has
    image partners): the default leaves the entries out here too."""
    _stream_off_equals_stream_on("rdx222", (2, 2, 2), monkeypatch, True)


def test_stream_stays_on_where_an_atom_meets_its_own_image(monkeypatch):
    """RDX 1 x 1 x 1 (168 atoms, 13 A edges): the self-image check forces the row forms of the matrix pass and of ENbond, which read the entries and
    their self-image flag -- the default writes them."""
    _stream_off_equals_stream_on("rdx168", (1, 1, 1), monkeypatch, False)


@pytest.mark.parametrize("case,mc,slots", [("ice", (3, 3, 3), False), ("ice", (5, 3, 3), True), ("rdx333", (3, 3, 3), True)])
def test_hydrogen_bonds_from_slots(case, mc, slots, monkeypatch):
    """The hydrogen-bond sweep finds a donor row's partners through the window slots when the entries were not written.  Perturbed ice Ih and RDX:
    Ehb = PE(10) and the forces of a FORCE behind one step (the second list build: the first one of an engine always writes the entries), with and
    without the stream and against the oracle.  Ice 3 x 3 x 3 (14.3 x 24.7 x 22.0 A) is a box in which an atom meets its own image: the entries stay;
    5 x 3 x 3 (23.8 A) is the smallest ice box that runs the slot form."""
    def run(always):
        e = _engine(case, mc, monkeypatch, always)
        e.QEq(); e.FORCE(); e.step(1)
        st = _stream(e)
        a = e.atoms(); pe = e.energy()["PE"].copy()
        e.close()
        return a, pe, st
    ons = [run(True) for _ in range(NSPREAD)]; a0, pe0, s0 = run(False)
    assert all(s[0] for _, _, s in ons) and s0 == ((not slots), False)
    rep = []
    _within("Ehb", pe0[10], [pe[10] for _, pe, _ in ons], rep)
    _within("f", a0["f"], [a["f"] for a, _, _ in ons], rep)
    _within("pos", a0["pos"], [a["pos"] for a, _, _ in ons], rep)
    assert (pe0[10] != 0.0) == (case != "ice")    # (the water force field has no hydrogen-bond row for H: no donors, pot.F90:595 -- the sweep is not launched on ice)
    # the oracle: one step from the same start (the engine's state after step(1) = the oracle's after step(1): forces of the new positions)
    ff, names, frac, lat = _system(case)
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=mc)
    o = oa.Oracle(ff, lat2, ranks, **{k: v for k, v in KW.items() if k != "qeq_mode"})
    o.qeq(); o.force(); o.step(1)
    assert (a0["gid"] == o.gids()).all()
    print("vs oracle: f %.3e  Ehb %.6e against %.6e" % (f_err(a0["f"], o.forces()), pe0[10], o.energy()[10]))
    assert f_err(a0["f"], o.forces()) <= FTOL
    assert abs(pe0[10] - o.energy()[10]) <= ETOL * abs(o.energy()[10])


def test_fall_back_after_a_lost_window(monkeypatch):
    """RDX 3 x 3 x 3 with the stream off, one step; then (a) the same atoms in an engine of the row form of ENbond (RXMD_NONBOND_WIN=0): its FORCE
    against the window engine's, forces within FTOL and energies within ETOL of each other as every pair of forms of one operator in the parity tests;
    (b) a reader of the entries on the window engine itself -- debug tap 11, which checks every entry against its slot: the build that left them out is
    swept again (nb10_valid -> rebuild), every slot leads back to its entry, and the engine writes the stream from then on."""
    e = _engine("rdx333", (3, 3, 3), monkeypatch, False)
    e.QEq(); e.FORCE(); e.step(1)
    assert _stream(e) == (False, False)
    rec = e.get_atoms_rxff(); a = e.atoms(); pe = e.energy()["PE"].copy()
    rows = e.debug(7).copy(); n10 = e.debug(6).astype(int)
    ok = e.debug(11).astype(int)
    assert _stream(e) == (True, True)
    assert (ok == n10).all(), int((ok != n10).sum())
    assert np.array_equal(e.debug(7), rows) and np.array_equal(e.debug(6).astype(int), n10)        # the second sweep wrote the same matrix
    pe_again = e.FORCE(); a_again = e.atoms()
    assert f_err(a_again["f"], a["f"]) <= 1e-12 and e_err(pe_again, pe) <= 1e-12                   # (acceptor atomics, energy sums)
    e.step(1)
    assert _stream(e) == (True, True)
    e.close()
    import rxmd_amd
    monkeypatch.setenv("RXMD_NONBOND_WIN", "0")
    from rxmd_amd import system
    ff, names, frac, lat = _system("rdx333")
    lat3, _ = system.geninit(ff, names, frac, lat, mc=(3, 3, 3))
    r = rxmd_amd.RxmdEngine(ff, lat3, **KW)
    r.set_atoms_rxff(rec)                         # positions, velocities and charges of the window engine behind its step
    per = r.FORCE(); ar = r.atoms()
    assert _stream(r)[0]
    r.close()
    order = np.argsort(ar["gid"]); order0 = np.argsort(a["gid"])
    print("row form vs window form: f %.3e  E %.3e" % (f_err(ar["f"][order], a["f"][order0]), e_err(per, pe)))
    assert f_err(ar["f"][order], a["f"][order0]) <= FTOL
    assert e_err(per, pe) <= ETOL


def _energies_of_the_last_step(case, mc, monkeypatch):
    def run(chunks):
        e = _engine(case, mc, monkeypatch, False)
        e.set_velocities(np.random.default_rng(7).normal(0.0, 0.02, (e.natoms, 3)))
        e.QEq(); e.FORCE(); e.energy()
        for c in chunks:
            e.step(c)
        a = e.atoms(); en = e.energy(); e.close()
        return dict(pos=a["pos"], v=a["v"], f=a["f"], q=a["q"], pe=en["PE"].copy(), astr=en["astr"].copy())
    aa = [run([5]) for _ in range(NSPREAD)]; b = run([1] * 5)
    a1 = aa[0]
    rep = []
    for k in ("pos", "v", "f", "q"):
        _within(k, b[k], [a[k] for a in aa], rep)
    _within("PE(11:13)", b["pe"][11:14], [a["pe"][11:14] for a in aa], rep)
    _within("astr", b["astr"], [a["astr"] for a in aa], rep)
    # no energy of an earlier step leaked in, the last step did not lose its own: PE(11:13) are those of ONE force evaluation (five of them would be
    # five times as large, none of them zero), and the block sums to PE(0)
    for r in (a1, b):
        assert r["pe"][11] != 0.0 and r["pe"][12] != 0.0 and r["pe"][13] != 0.0
        assert abs(r["pe"][0] - r["pe"][1:14].sum()) <= 1e-12 * abs(r["pe"][0])
    assert np.abs(b["pe"][11:14] - a1["pe"][11:14]).max() <= 1e-9 * np.abs(a1["pe"][11:14]).max()
    return rep


def test_energies_of_the_last_step(monkeypatch):
    """step(5) against five step(1) calls from the same start, RDX 3 x 3 x 3: only the last step of a call forms ENbond's energies; positions, velocities,
    forces and charges do not know the difference, PE(11:13) and the stress accumulators (summed over all five steps) agree to the order of their sums."""
    _energies_of_the_last_step("rdx333", (3, 3, 3), monkeypatch)


def test_energies_of_the_last_step_rdx222(monkeypatch):
    """the same on RDX 2 x 2 x 2"""
    _energies_of_the_last_step("rdx222", (2, 2, 2), monkeypatch)


def test_energies_of_the_last_step_row_form(monkeypatch):
    """the same through the row form of ENbond (RDX 1 x 1 x 1: a box in which an atom meets its own image)"""
    _energies_of_the_last_step("rdx168", (1, 1, 1), monkeypatch)
