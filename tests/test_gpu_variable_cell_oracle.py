"""Variable cell against an oracle that changes its own lattice.

rxmd_hip_set_lattice and the Berendsen barostat inside rxmd_hip_step have no counterpart in the reference, whose box is fixed at start-up.
The oracle has the same operation in plain C (rxo_set_lattice, pinned against its own set-up by tests/test_oracle_variable_cell.py) and
tests/npt_reference.py restates the coupling rule around it, so the whole NPT path is compared state by state: shape changes (every
entry of the remap matrix), PQEq shells under shear, sequences of lattices on one engine, couplings inside one step() call, `every` > 1,
the per-axis mode, a triclinic cell, qstep, isQEq 2, PQEq, a coupling that lowers a bond-cell count inside step() (capacity growth), and
two ranks over a host transport.  Each scenario asserts that the path it is about was really taken.

Gates (none is new): static evaluations QTOL / FTOL / ETOL of test_gpu_parity and astr 1e-9; positions right after set_lattice 1e-11 A
(two exact routes); trajectories of <= 8 steps pos and v 1e-9, KE 1e-7 (test_md_trajectory_tight); the squeezed boxes pos 1e-8 A, forces
1e-5 (test_migration_across_periodic_boundary_keeps_reference_order).  Lattice: astr agrees to 1e-9 and d(mu)/mu ~ (mu^3 - 1)/3 dP/P with
|mu - 1| <= 0.1, so one coupling adds at most ~1e-10 relative: every length is gated at n_couplings x 1e-10, p6 at 1e-9 of its largest
component; where the clamp binds mu is 1 +- max_strain exactly on both sides and the lattices agree to 1e-14 per coupling.
Velocities are one seeded numpy draw given to both programs.  Run with -s for the measured margins."""
import functools
import numpy as np
import pytest

import oracle_api as oa
import npt_reference as npt
from ranks import run_ranks
import vc_worker
from parity import _engine, q_err, f_err, e_err, sheared, lattice_sequence, QTOL, FTOL, ETOL

pytestmark = pytest.mark.gpu

TIGHT = dict(QEq_tol=1e-12, NMAXQEq=2000)
MC = {"rdx222": (2, 2, 2), "ice644": (6, 4, 4), "mos2_tri324": (3, 3, 2), "sicnp547": (1, 1, 1)}
BAR = dict(tau_fs=25.0, bulk=15.0)


def velocities(n, seed, sigma):
    return np.random.default_rng(seed).normal(0.0, sigma, (n, 3))


def oracle_for(case, vp=(1, 1, 1), v=None, **kw):
    """(oracle, lattice, per-rank records); v is [natoms, 3] in gid order"""
    ff, names, frac, lat = oa.make_system(case)
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=MC[case], vprocs=vp)
    pq = oa.PQEQ_SICNP if case.startswith("sicnp") else None
    v0 = None if v is None else [v[r["gid"] - 1] for r in ranks]
    o = oa.Oracle(ff, lat2, ranks, vprocs=vp, v0=v0, pqeq=pq, **{**TIGHT, **kw})
    if pq:
        o.set_pqeq_clean(1)                              # a look-up beyond the cut-off yields zero, as in the engine (test_pqeq_md_against_the_clean_oracle)
    return o, [float(x) for x in lat2], ranks


def engine_for(case, v=None, **kw):
    if case.startswith("sicnp"):
        kw = dict(pqeq=oa.PQEQ_SICNP, **kw)
    e = _engine(case, MC[case], **{**TIGHT, **kw})
    if v is not None:
        e.set_velocities(v)                              # one rank: the local order of the records is the gid order
    return e


def assert_sheared(L0, L1):
    M = npt.remap_matrix(L0, L1)
    assert min(abs(M[0, 1]), abs(M[0, 2]), abs(M[1, 2])) >= 1e-3, M
    return M


def static_compare(e, o, tag, pqeq=False):
    """QEq + FORCE on both, from whatever state they are in: gid order, q, f, 14 energies, astr"""
    e.energy(); o.astr(reset=True)                       # both accumulators start from zero
    e.QEq(); pe = e.FORCE(); a = e.atoms(); astr = e.energy()["astr"]
    o.qeq(); o.force(); po = o.energy(); ostr = o.astr(reset=True)
    assert (a["gid"] == o.gids()).all(), tag
    dq, df = q_err(a["q"], o.charges()), f_err(a["f"], o.forces())
    de = np.abs(pe - po).max() / abs(po[0]) if pqeq else e_err(pe, po)
    ds = np.abs(astr - ostr).max() / np.abs(ostr).max()
    print("%s: q %.2e (gate %.0e)  f %.2e (%.0e)  energies %.2e (%.0e%s)  astr %.2e (1e-09)" % (tag, dq, QTOL, df, FTOL, de, ETOL, " of the total" if pqeq else "", ds))
    assert dq <= QTOL and df <= FTOL, tag
    assert de <= ETOL, tag                               # (PQEq: on the scale of the total, as test_pqeq_md_against_the_clean_oracle gates it)
    assert ds <= 1e-9, tag
    return pe


# ------------------------------------------------------------------------------------------------ 1-3: set_lattice
@pytest.mark.parametrize("case", ["rdx222", "mos2_tri324", "ice644"])
def test_shape_change_against_the_oracle(case):
    """1: lengths and all three angles change, so every entry of the upper triangle of M = H' H^-1 is non-zero"""
    e = engine_for(case); o, L0, _ = oracle_for(case)
    static_compare(e, o, "1 %s at L0" % case)            # a live engine: lists, charges, forces of L0 exist
    L1 = sheared(L0)
    M = assert_sheared(L0, L1)
    p0 = e.atoms()["pos"]
    e.set_lattice(L1); o.set_lattice(L1)
    assert e.lattice == L1
    a = e.atoms()
    dp, dm = np.abs(a["pos"] - o.pos()).max(), np.abs(a["pos"] - p0 @ M.T).max()
    print("1 %s sheared: positions against the oracle %.2e A, against M r in numpy %.2e A (gate 1e-11); M upper triangle %s" % (case, dp, dm, M[np.triu_indices(3, 1)]))
    assert (a["gid"] == o.gids()).all()
    assert dp <= 1e-11 and dm <= 1e-11
    static_compare(e, o, "1 %s sheared" % case)
    e.close()


def test_pqeq_shells_under_shear_against_the_oracle():
    """2: the shell displacements go through the same M (not its transpose, not its diagonal).

    After the first PQEq call the oracle's charges and shells are handed to the engine, so the evaluation behind the shear starts from one
    state (the equal start of test_set_lattice_equals_a_fresh_engine_and_the_oracle).  Without that the sheared evaluation inherits the
    exit noise of the call before it and misses QTOL: PQEq's CG leaves when Est stops changing at QEq_tol relative, which bounds the
    charges at ~sqrt(QEq_tol) only.  Measured at QEq_tol 1e-12 without the hand-over: engine 20 iterations, oracle 24, charges 2.25e-6,
    astr 3.7e-9, energies 1.5e-9 of the total; at QEq_tol 1e-16 (both converged) charges 3.4e-12, forces 2.4e-9, shells 1.3e-13 A."""
    e = engine_for("sicnp547"); o, L0, _ = oracle_for("sicnp547")
    static_compare(e, o, "2 sicnp547 at L0", pqeq=True)
    assert np.abs(e.shells()).max() > 1e-6 and np.abs(o.spos()).max() > 1e-6, "the shells must have moved before the lattice changes"
    assert np.abs(e.shells() - o.spos()).max() <= 1e-7
    e.set_shells(o.spos()); e.set_charges(o.charges())
    d0 = e.shells()
    L1 = sheared(L0)
    M = assert_sheared(L0, L1)
    e.set_lattice(L1); o.set_lattice(L1)
    d1 = e.shells()
    dm, do = np.abs(d1 - d0 @ M.T).max() / np.abs(d0).max(), np.abs(d1 - o.spos()).max()
    print("2 shells after the shear: against M d in numpy %.2e relative (gate 1e-13), against the oracle %.2e A (gate 1e-11)" % (dm, do))
    assert dm <= 1e-13                                   # the engine's own map (the gate of test_pqeq_shells_follow_the_lattice)
    assert do <= 1e-11                                   # equal shells through two exact routes, as the positions
    assert np.abs(e.atoms()["pos"] - o.pos()).max() <= 1e-11
    static_compare(e, o, "2 sicnp547 sheared", pqeq=True)
    ds = np.abs(e.shells() - o.spos()).max()
    print("2 shells after PQEq at the sheared box: %.2e A (gate 1e-07)" % ds)
    assert ds <= 1e-7                                    # (the gate of test_pqeq_md_against_the_clean_oracle)
    e.close()


def test_pqeq_calls_repeated_without_moving_the_atoms():
    """Found while diagnosing 2: the shells move at the end of every PQEq call, and the matrix rows of the 10 A list (shell-core values,
    field term) are formed from them.  A second QEq() with the atoms where they were re-used the rows of the old shells: charges 1.4e-2
    from the oracle at the second call, 2.8e-2 at the third (any box, no lattice change needed); MD steps rebuild the lists and never saw it."""
    e = engine_for("sicnp547"); o, _, _ = oracle_for("sicnp547")
    for k in range(3):
        static_compare(e, o, "PQEq call %d at unmoved atoms" % (k + 1), pqeq=True)
        ds = np.abs(e.shells() - o.spos()).max()
        print("   shells %.2e A (gate 1e-07), largest displacement %.2e A" % (ds, np.abs(o.spos()).max()))
        assert ds <= 1e-7
    e.close()


def test_a_sequence_of_lattices_on_one_engine():
    e = engine_for("rdx222"); o, L0, _ = oracle_for("rdx222")
    n = e.natoms
    pe0 = static_compare(e, o, "3 rdx222 at L0")
    st0 = e.stats()
    prev = L0
    for name, L in lattice_sequence(L0, e.cutoffs()[1]):
        e.set_lattice(L); o.set_lattice(L)
        st = e.stats()
        if name == "expanded":
            assert all(st["cells10"][a] > st0["cells10"][a] for a in range(3)), (st0["cells10"], st["cells10"])   # the re-allocation branches of apply_lattice
        if name == "sheared":
            assert_sheared(prev, L)
        if name == "compressed":
            assert st["cells3"][2] == st0["cells3"][2] - 1 and list(st["cells3"][:2]) == list(st0["cells3"][:2])
        if name == "back at L0":
            e.set_charges(np.zeros(n)); o.set_charges(np.zeros(n))       # the start vector of the first evaluation
        assert list(o.info()[1:4]) == list(st["cells3"])
        print("3 %s: cells10 %s cells3 %s nbuffer %d" % (name, list(st["cells10"]), list(st["cells3"]), st["nbuffer"]))
        assert np.abs(e.atoms()["pos"] - o.pos()).max() <= 1e-11
        pe = static_compare(e, o, "3 rdx222 " + name)
        prev = L
    d = e_err(pe, pe0)
    print("3 back at L0 against the first evaluation: energies %.2e (gate 1e-10)" % d)
    assert d <= 1e-10
    e.close()


# ------------------------------------------------------------------------------------------------ 4-9: the barostat, one rank
def gate_lattice(tag, lat, ref, ncoup, clamped):
    tol = ncoup * (1e-14 if clamped else 1e-10)
    d = max(abs(lat[a] - ref[a]) / ref[a] for a in range(3))
    print("%s: lattice %.2e relative (gate %.0e)" % (tag, d, tol))
    assert d <= tol, tag
    assert list(lat[3:]) == list(ref[3:]), tag


def gate_coupling(tag, st, row, ncoup, clamped_axes=()):
    dp = np.abs(st["p6"] - row["p6"]).max() / np.abs(row["p6"]).max()
    dmu = np.abs(st["mu"] - row["mu"]).max()
    dv = abs(st["volume"] - npt.volume(row["lat"])) / st["volume"]
    print("%s: p6 %.2e of its largest component (gate 1e-09)  mu %.2e (1e-10)  volume %.2e  P %s GPa  mu %s" % (tag, dp, dmu, dv, np.round(row["p6"][:3], 4), row["mu"]))
    assert dp <= 1e-9, tag
    assert dmu <= 1e-10, tag                             # one coupling's share of the lattice gate
    assert dv <= 3e-10 * ncoup + 1e-13, tag              # the volume BEFORE the remap, of a lattice inside the lattice gate (three lengths)
    for k in clamped_axes:
        assert st["mu"][k] == row["mu"][k], tag


def gate_state(tag, e, o, hot=False, pqeq=False):
    """final positions, velocities, charges, forces, energies, kinetic energy of the trajectory, by gid"""
    a = e.atoms(); en = e.energy()
    ie, io = np.argsort(a["gid"]), np.argsort(o.gids())
    same_order = (a["gid"] == o.gids()).all()
    dx, dv = np.abs(a["pos"][ie] - o.pos()[io]).max(), np.abs(a["v"][ie] - o.vel()[io]).max()
    dq, df = q_err(a["q"][ie], o.charges()[io]), f_err(a["f"][ie], o.forces()[io])
    po = o.energy()
    de = np.abs(en["PE"] - po).max() / abs(po[0]) if pqeq else e_err(en["PE"], po)
    dk = abs(en["KE"] - o.kinetic()) / abs(o.kinetic())
    xt, ft = (1e-8, 1e-5) if hot else (1e-9, FTOL)
    print("%s: pos %.2e A (gate %.0e)  v %.2e (%.0e)  q %.2e (%.0e)  f %.2e (%.0e)  energies %.2e (%.0e)  KE %.2e (1e-07)  same local order %s  max|f| %.1f"
          % (tag, dx, xt, dv, xt, dq, QTOL, df, ft, de, ETOL, dk, same_order, np.abs(o.forces()).max()))
    assert same_order, tag
    assert dx <= xt and dv <= xt, tag
    assert dq <= QTOL and df <= ft, tag
    assert de <= ETOL and dk <= 1e-7, tag
    if pqeq:
        ds = np.abs(e.shells()[ie] - o.spos()[io]).max()
        print("%s: shells %.2e A (gate 1e-07)" % (tag, ds))
        assert ds <= 1e-7, tag


def input_lattice(case):
    ff, names, frac, lat = oa.make_system(case)
    return [float(lat[a] * MC[case][a]) for a in range(3)] + [float(x) for x in lat[3:6]]


def compressed_rdx():
    L0 = input_lattice("rdx222")
    return [x * 0.97 for x in L0[:3]] + L0[3:]


def reference_npt(case, v, L, nsteps, pre=0, qstep=1, vp=(1, 1, 1), okw=None, **bar):
    """the oracle's half of a barostat scenario: set to L, QEq + FORCE, `pre` NVE steps, then nsteps under the barostat"""
    o, L0, ranks = oracle_for(case, vp=vp, v=v, **(okw or {}))
    if qstep != 1:
        o.set_qstep(qstep)
    if list(L) != list(L0):
        o.set_lattice(L)
    o.qeq(); o.force()
    if pre:
        o.step(pre)
    Lf, rows = npt.berendsen_run(o, L, nsteps, steps_done=pre, **{**BAR, **bar})
    return o, Lf, rows, ranks


def engine_npt(case, v, L, pre=0, ekw=None, **bar):
    e = engine_for(case, v=v, **(ekw or {}))
    if list(L) != e.lattice:
        e.set_lattice(L)
    e.QEq(); e.FORCE()
    if pre:
        e.step(pre)
    b = {**BAR, **bar}
    e.set_barostat(b["mode"], p0=b["p0"], tau_fs=b["tau_fs"], bulk_modulus=b["bulk"], every=b.get("every", 1), max_strain=b.get("max_strain", 0.01), axes=b.get("axes", 7))
    return e


S4 = dict(mode=1, p0=0.0, every=1, max_strain=0.01)


@functools.lru_cache(None)
def reference_s4():
    return reference_npt("rdx222", velocities(1344, 21, 0.02), compressed_rdx(), 5, **S4)


@pytest.mark.parametrize("qeq_mode", [0, 1])
def test_isotropic_coupling_every_step(qeq_mode):
    """4: rdx222 3 % compressed, 5 couplings inside ONE step(5) call and as 5 x step(1)"""
    v, L = velocities(1344, 21, 0.02), compressed_rdx()
    o, Lf, rows, _ = reference_s4()
    assert len(rows) == 5
    e = engine_npt("rdx222", v, L, ekw=dict(qeq_mode=qeq_mode), **S4)
    e.step(5)
    st = e.barostat_state()
    assert st["couplings"] == 5
    tag = "4 qeq_mode %d step(5)" % qeq_mode
    gate_lattice(tag, e.lattice, Lf, 5, False); gate_coupling(tag, st, rows[-1], 5); gate_state(tag, e, o)
    L_one = e.lattice
    e.close()
    e = engine_npt("rdx222", v, L, ekw=dict(qeq_mode=qeq_mode), **S4)
    for k in range(5):
        e.step(1)
        tag = "4 qeq_mode %d 5 x step(1), coupling %d" % (qeq_mode, k + 1)
        st = e.barostat_state()
        assert st["couplings"] == k + 1
        gate_lattice(tag, e.lattice, rows[k]["new"], k + 1, False); gate_coupling(tag, st, rows[k], k + 1)
    gate_state("4 qeq_mode %d 5 x step(1)" % qeq_mode, e, o)
    assert e.lattice == L_one                            # the two call shapes: bit for bit
    e.close()


def test_coupling_every_third_step():
    """5: 2 NVE steps, then every = 3 and step(7): the total step count decides, so couplings fall at steps 3, 6, 9 inside the one call"""
    v, L = velocities(1344, 22, 0.02), compressed_rdx()
    bar = dict(mode=1, p0=0.0, every=3, max_strain=0.01)
    o, Lf, rows, _ = reference_npt("rdx222", v, L, 7, pre=2, **bar)
    assert [r["step"] for r in rows] == [3, 6, 9]
    e = engine_npt("rdx222", v, L, pre=2, **bar)
    e.step(7)
    st = e.barostat_state()
    assert st["couplings"] == 3
    gate_lattice("5 every 3", e.lattice, Lf, 3, False); gate_coupling("5 every 3", st, rows[-1], 3); gate_state("5 every 3", e, o)
    e.close()


def test_per_axis_mode_with_three_targets():
    """6: mode 2, three distinct targets, y switched off by the axes mask"""
    v, L = velocities(1344, 23, 0.02), compressed_rdx()
    bar = dict(mode=2, p0=(400.0, 0.0, -50.0), every=1, max_strain=0.002, axes=5)
    o, Lf, rows, _ = reference_npt("rdx222", v, L, 5, **bar)
    for r in rows:
        assert r["mu"][1] == 1.0 and len({r["mu"][0], r["mu"][1], r["mu"][2]}) == 3, r["mu"]
        assert r["mu"][0] == 1.0 - 0.002 and r["mu"][2] == 1.0 + 0.002      # the clamp binds on both moving axes
    e = engine_npt("rdx222", v, L, **bar)
    e.step(5)
    st = e.barostat_state()
    assert st["couplings"] == 5
    assert st["mu"][1] == 1.0 and e.lattice[1] == L[1]
    assert len(set(st["mu"])) == 3
    gate_lattice("6 per axis", e.lattice, Lf, 5, True); gate_coupling("6 per axis", st, rows[-1], 5, clamped_axes=(0, 1, 2)); gate_state("6 per axis", e, o)
    e.close()


@pytest.mark.parametrize("kw", [dict(qstep=3), dict(isQEq=2)], ids=["qstep3", "isQEq2"])
def test_triclinic_cell_under_the_barostat(kw):
    """7: mos2_tri324 (gamma = 120 degrees), isotropic; charges every third step only, and the extended-Lagrangian mode"""
    v = velocities(972, 24, 0.01)
    L = input_lattice("mos2_tri324")
    bar = dict(mode=1, p0=0.0, every=1, max_strain=0.01)
    okw = dict(isQEq=2) if "isQEq" in kw else None
    o, Lf, rows, _ = reference_npt("mos2_tri324", v, L, 5, qstep=kw.get("qstep", 1), okw=okw, **bar)
    assert len(rows) == 5 and all(abs(r["mu"][0] - 1.0) > 1e-7 for r in rows)
    e = engine_npt("mos2_tri324", v, L, ekw=kw, **bar)
    e.step(5)
    st = e.barostat_state()
    assert st["couplings"] == 5
    assert e.lattice[3:] == L[3:]                        # angles: bit for bit
    tag = "7 triclinic " + str(kw)
    gate_lattice(tag, e.lattice, Lf, 5, False); gate_coupling(tag, st, rows[-1], 5); gate_state(tag, e, o)
    e.close()


def test_pqeq_under_the_barostat():
    """8: sicnp547 with PQEq against the clean oracle, 5 couplings"""
    v = velocities(547, 25, 0.01)
    L = input_lattice("sicnp547")
    bar = dict(mode=1, p0=0.0, every=1, max_strain=0.01)
    o, Lf, rows, _ = reference_npt("sicnp547", v, L, 5, **bar)
    e = engine_npt("sicnp547", v, L, **bar)
    e.step(5)
    st = e.barostat_state()
    assert st["couplings"] == 5
    gate_lattice("8 PQEq", e.lattice, Lf, 5, False); gate_coupling("8 PQEq", st, rows[-1], 5); gate_state("8 PQEq", e, o, pqeq=True)
    e.close()


def squeezed_lattice(L0, maxrc, vpz):
    """z just above a bond-cell threshold of the local box: a per-axis barostat whose clamp binds drives it through"""
    cz = int(L0[2] / vpz / maxrc)
    return L0[:2] + [vpz * (cz * maxrc + (0.12 if vpz == 1 else 0.10))] + L0[3:], cz


S9 = dict(mode=2, p0=(0.0, 0.0, 2000.0), every=1, max_strain=0.002, axes=4)


def test_a_coupling_lowers_a_cell_count_inside_step():
    """9: cc_z drops 6 -> 5 at a coupling inside step(6); the engine (default capacity) grows in place inside the call"""
    v = velocities(1344, 26, 0.02)
    o0, L0, _ = oracle_for("rdx222")
    L, cz = squeezed_lattice(L0, o0.info()[0], 1)
    o, Lf, rows, _ = reference_npt("rdx222", v, L, 6, **S9)
    assert all(r["mu"][2] == 1.0 - 0.002 for r in rows) and o.info()[3] == cz - 1
    e = engine_npt("rdx222", v, L, **S9)
    st0 = e.stats()
    assert st0["cells3"][2] == cz == 6
    e.step(6)
    st1, bs = e.stats(), e.barostat_state()
    print("9 capacity before the call %d, after it %d; cells3 %s -> %s; cells10 %s -> %s" % (st0["nbuffer"], st1["nbuffer"], list(st0["cells3"]), list(st1["cells3"]), list(st0["cells10"]), list(st1["cells10"])))
    assert bs["couplings"] == 6
    assert st1["cells3"][2] == 5
    assert st1["nbuffer"] > st0["nbuffer"]               # growth happened inside step()
    assert e.lattice[0] == L[0] and e.lattice[1] == L[1]
    gate_lattice("9 squeezed", e.lattice, Lf, 6, True); gate_coupling("9 squeezed", bs, rows[-1], 6, clamped_axes=(0, 1, 2)); gate_state("9 squeezed", e, o, hot=True)
    e.close()


# ------------------------------------------------------------------------------------------------ 10, 11: two ranks over gloo


def two_ranks(job):
    """two spawned children on one GPU under one time limit; a dead rank fails the test, nothing is retried"""
    return run_ranks(vc_worker.npt_rank, 2, job, timeout=600)


def gate_two_ranks(tag, res, o, rows, clamped, hot):
    """rows: the reference's couplings that the ranks recorded (every one, or the last one of a single step() call)"""
    l0, l1 = res[0]["lattices"], res[1]["lattices"]
    assert l0 == l1                                      # both ranks hold the same lattice, bit for bit
    assert len(l0) == len(rows)
    for k, (ncoup, row) in enumerate(rows):
        gate_lattice("%s coupling %d" % (tag, ncoup), l0[k], row["new"], ncoup, clamped)
        dp = np.abs(np.array(res[0]["p6"][k]) - row["p6"]).max() / np.abs(row["p6"]).max()
        assert dp <= 1e-9, (tag, k, dp)
        if clamped:
            assert list(res[0]["mu"][k]) == list(row["mu"])
    xt, ft = (1e-8, 1e-5) if hot else (1e-9, FTOL)
    pe = np.array(res[0]["pe"]) + np.array(res[1]["pe"]); ke = res[0]["ke"] + res[1]["ke"]
    for r in range(2):
        a = {k: np.array(x) for k, x in res[r]["atoms"].items()}
        ie, io = np.argsort(a["gid"]), np.argsort(o.gids(r))
        assert (a["gid"][ie] == o.gids(r)[io]).all(), "the two programs hold different atoms on rank %d" % r
        dx, dv = np.abs(a["pos"][ie] - o.pos(r)[io]).max(), np.abs(a["v"][ie] - o.vel(r)[io]).max()
        dq, df = q_err(a["q"][ie], o.charges(r)[io]), f_err(a["f"][ie], o.forces(r)[io])
        print("%s rank %d (%d residents): pos %.2e A (gate %.0e)  v %.2e  q %.2e (%.0e)  f %.2e (%.0e)" % (tag, r, len(ie), dx, xt, dv, dq, QTOL, df, ft))
        assert dx <= xt and dv <= xt and dq <= QTOL and df <= ft, (tag, r)
    de, dk = e_err(pe, o.energy()), abs(ke - o.kinetic()) / abs(o.kinetic())
    print("%s: summed energies %.2e (gate %.0e)  KE %.2e (1e-07)" % (tag, de, ETOL, dk))
    assert de <= ETOL and dk <= 1e-7, tag


def test_two_ranks_isotropic_against_the_two_rank_oracle():
    """10: vprocs (2,1,1), 5 isotropic couplings; every lattice and each rank's final state against the oracle in the same decomposition.
    The box is the input crystal (what test_two_ranks_couple_to_the_same_lattice runs), to which the velocity gate of
    test_md_trajectory_tight applies: in the 3 % compressed box of scenario 4 (111 GPa, forces 25 times those of the crystal at rest) the
    CG noise of the charges (1e-8 .. 1e-7 at QEq_tol 1e-12) reaches the velocities through the forces and the gate is met with no room
    (measured there: one rank 8.2e-10 .. 8.7e-10, two ranks 4.9e-10 and 1.014e-09)."""
    v, L = velocities(1344, 27, 0.02), input_lattice("rdx222")
    bar = dict(mode=1, p0=0.0, every=1, max_strain=0.01)
    o, Lf, rows, _ = reference_npt("rdx222", v, L, 5, vp=(2, 1, 1), **bar)
    assert all(abs(r["mu"][0] - 1.0) > 1e-6 for r in rows)       # every coupling moves the box
    res = two_ranks(dict(vp=(2, 1, 1), seed=27, sigma=0.02, lattice=L, nsteps=5, one_call=False, bar={**BAR, **bar}))
    assert all(r["couplings"] == 5 for r in res)
    gate_two_ranks("10 two ranks (2,1,1)", res, o, list(enumerate(rows, 1)), False, False)


def test_two_ranks_split_along_the_squeezed_axis():
    """11: vprocs (1,1,2), the local cc_z drops 3 -> 2 on both ranks inside step(6).  The host transport's exchange buffer is the host's:
    grow_capacity leaves it as it is, so the largest message after the drop is reported against its size."""
    v = velocities(1344, 28, 0.02)
    o0, L0, _ = oracle_for("rdx222", vp=(1, 1, 2))
    L, cz = squeezed_lattice(L0, o0.info()[0], 2)
    assert cz == 3
    o, Lf, rows, _ = reference_npt("rdx222", v, L, 6, vp=(1, 1, 2), **S9)
    assert all(r["mu"][2] == 1.0 - 0.002 for r in rows) and o.info()[3] == cz - 1
    res = two_ranks(dict(vp=(1, 1, 2), seed=28, sigma=0.02, lattice=L, nsteps=6, one_call=True, bar={**BAR, **S9}))
    for r in res:
        print("11 rank %d: cells3 %s -> %s, nbuffer %d -> %d, exchange buffer %d doubles, largest message %d doubles"
              % (r["rank"], r["cells3"][0], r["cells3"][1], r["nbuffer"][0], r["nbuffer"][1], r["xbuf_doubles"], r["max_message"]))
        assert r["cells3"][0][2] == 3 and r["cells3"][1][2] == 2
        assert r["couplings"] == 6
        assert r["max_message"] <= r["xbuf_doubles"]
    assert rows[-1]["new"] == Lf
    gate_two_ranks("11 two ranks (1,1,2)", res, o, [(6, rows[-1])], True, True)
