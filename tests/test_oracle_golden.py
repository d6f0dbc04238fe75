"""Pins the plain-C oracle (oracle/rxmd_oracle.c) against golden vectors produced by the REAL
reference (tests/golden/make_golden.py -> oracle/_ref/rxmd).  CPU only.

Dump resolution of the reference is f20.12, so 'exact' here means |diff| <= 1e-11 absolute.
"""
import os
import numpy as np
import pytest
import oracle_api as oa

GOLD = oa.GOLD


def _run(case, mc, steps=0, **kw):
    g = np.load(os.path.join(GOLD, case + ".npz"))
    ff, names, frac, lat = oa.make_system(case)
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff, lg=kw.get("lg", False)), mc=mc)
    o = oa.Oracle(ff, lat2, ranks, **kw)
    iters = [o.qeq()]
    o.force()
    pe0 = o.energy()
    for _ in range(steps):
        o.step(1)
        iters.append(o.L.rxo_qeq_iters(o.w))
    return g, o, iters, pe0


def _compare(g, o, ftol=1e-10, qtol=1e-11):
    gid = o.gids()
    order = np.argsort(gid)
    gorder = np.argsort(g["gid"])
    assert (gid[order] == g["gid"][gorder]).all()
    dq = np.abs(o.charges()[order] - g["charge"][gorder]).max()
    df = np.abs(o.forces()[order] - g["force"][gorder]).max()
    dp = np.abs(o.pos()[order] - g["pos"][gorder]).max()
    assert dp < 1e-11, dp
    assert dq < qtol, dq
    assert df < ftol, df
    return dq, df


def _check_energy(g, pe, n, row=0):
    m = g["mdstep"][row]   # step TE PE KE E1 E2-4 E5-7 E8-9 E10 E11-13 ...
    ref = np.array([m[2], m[4], m[5], m[6], m[7], m[8], m[9]]) * n
    got = np.array([pe[0], pe[1], pe[2:5].sum(), pe[5:8].sum(), pe[8:10].sum(), pe[10], pe[11:14].sum()])
    # printed with es13.5 / es11.3 -> 6 and 4 significant digits
    assert abs(got[0] - ref[0]) <= 1e-5 * abs(ref[0])
    assert np.all(np.abs(got[1:] - ref[1:]) <= 1.1e-3 * np.abs(ref[1:]) + 1e-12)


def test_rdx168_default_tolerance_bitpath():
    g, o, iters, pe = _run("rdx168_tol7", (1, 1, 1))
    assert iters[0] == int(g["qeq_iters"][0]) == 35
    _compare(g, o)
    _check_energy(g, pe, 168)
    # per-iteration Est trace of the reference (printed es25.15)
    tr = o.trace(); ref = g["qeq_trace_last"]
    assert len(tr) == len(ref)
    assert np.allclose(tr[:, 0], ref[:, 3], rtol=1e-13, atol=0)
    # known answers quoted in SURVEY 8(c)
    assert abs(tr[-1, 0] - (-1.260035970464605E+02)) < 1e-10


def test_rdx168_step0_energies_match_the_references_published_sample_output():
    """the only known answer the reference itself publishes: README.md:157 (168-atom RDX, default rxmd.in)"""
    g, o, iters, pe = _run("rdx168_tol7", (1, 1, 1))
    oa.check_readme_known_answer(np.asarray(pe))


def test_rdx168_tight():
    g, o, iters, pe = _run("rdx168_tight", (1, 1, 1), QEq_tol=1e-12, NMAXQEq=2000)
    assert iters[0] == int(g["qeq_iters"][0])
    _compare(g, o)


def test_rdx168_no_qeq_forces_only():
    g, o, iters, pe = _run("rdx168_noqeq", (1, 1, 1), isQEq=0)
    _compare(g, o)
    _check_energy(g, pe, 168)


def test_rdx168_md10_trajectory():
    g, o, iters, pe = _run("rdx168_md10", (1, 1, 1), steps=10)
    assert iters == [int(x) for x in g["qeq_iters"]]
    _compare(g, o, ftol=1e-9, qtol=1e-10)


def test_hessian_rowsums_and_counts():
    g = np.load(os.path.join(GOLD, "rdx168_tol7.npz"))
    ff, names, frac, lat = oa.make_system("rdx168")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff))
    o = oa.Oracle(ff, lat2, ranks)
    o.qeq()
    assert (o.get(104).astype(int) == g["hess_nnz"]).all()
    assert np.allclose(o.get(108), g["hess_rowsum"], rtol=1e-13)


@pytest.mark.parametrize("case,mc,steps", [("rdx222_tight", (2, 2, 2), 0), ("rdx222_md5", (2, 2, 2), 5)])
def test_rdx222(case, mc, steps):
    kw = dict(QEq_tol=1e-12, NMAXQEq=2000) if "tight" in case else {}
    g, o, iters, pe = _run(case, mc, steps=steps, **kw)
    assert iters == [int(x) for x in g["qeq_iters"]]
    _compare(g, o, ftol=1e-9, qtol=1e-10)
    if steps == 0:
        _check_energy(g, pe, 1344)


def test_ice_type_order_and_zero_hbond():
    g, o, iters, pe = _run("ice644_tight", (6, 4, 4), QEq_tol=1e-12, NMAXQEq=2000)
    assert iters[0] == int(g["qeq_iters"][0])
    _compare(g, o, ftol=1e-9)
    assert pe[10] == 0.0          # hydrogen is hard-coded as type 2; water ffield has H = 1  
    _check_energy(g, pe, 2304)


@pytest.mark.parametrize("case,steps", [("rdx222_v211_tight", 0), ("rdx222_v222_tight", 0), ("rdx222_v222_md3", 3),
                                        ("example2_v211_md3", 3)])        # the last: the reference's examples/2-reaxff-dc under mpirun -np 2
def test_multirank_world_vs_real_mpi_reference(case, steps):
    """the oracle's in-process multi-rank world against the reference run under real MPI (conda MPICH) at the same vprocs"""
    g = np.load(os.path.join(GOLD, case + ".npz"))
    vp = tuple(int(x) for x in g["vprocs"]); mc = tuple(int(x) for x in g["mc"])
    ff, names, frac, lat = oa.make_system(case)
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=mc, vprocs=vp)
    o = oa.Oracle(ff, lat2, ranks, vprocs=vp, QEq_tol=1e-12, NMAXQEq=2000)
    iters = [o.qeq()]; o.force()
    for _ in range(steps):
        o.step(1); iters.append(o.L.rxo_qeq_iters(o.w))
    assert iters == [int(x) for x in g["qeq_iters"]]
    for r in range(len(ranks)):
        assert (o.gids(r) == g["gid_%d" % r]).all()
        assert np.abs(o.charges(r) - g["charge_%d" % r]).max() < 1e-10
        assert np.abs(o.forces(r) - g["force_%d" % r]).max() < 1e-9
        assert np.abs(o.pos(r) - g["pos_%d" % r]).max() < 1e-11


def _multirank_oracle(case, **kw):
    g = np.load(os.path.join(GOLD, case + ".npz"))
    vp = tuple(int(x) for x in g["vprocs"]); mc = tuple(int(x) for x in g["mc"])
    ff, names, frac, lat = oa.make_system(case)
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=mc, vprocs=vp)
    return g, oa.Oracle(ff, lat2, ranks, vprocs=vp, **kw), len(ranks)


def _compare_ranks(g, o, nranks, qtol=1e-10, ftol=1e-9):
    for r in range(nranks):
        assert (o.gids(r) == g["gid_%d" % r]).all()
        assert np.abs(o.charges(r) - g["charge_%d" % r]).max() < qtol
        assert np.abs(o.forces(r) - g["force_%d" % r]).max() < ftol
        assert np.abs(o.pos(r) - g["pos_%d" % r]).max() < 1e-11


@pytest.mark.parametrize("case,steps,efield", [("sicnp211_v211_pqeq_tight", 0, None), ("sicnp222_v222_pqeq_tight", 0, None), ("sicnp211_v211_pqeq_md3", 3, None),
                                               ("sicnp211_v211_pqeq_efieldx_md3", 3, (1, 0.05))])
def test_multirank_pqeq_vs_real_mpi_reference(case, steps, efield):
    """PQEq BETWEEN RANKS (round 6): the SiC nanoparticle replicated to one particle per rank, `mpiexec -np 2 / 8 rxmd_mpi --pqeq` --
    shell displacements ride in the COPY and MOVE records (comm.F90:122,129-131,153,165-167), the shell halo and the CG vectors cross the
    rank boundary and are forwarded x -> y -> z through edge and corner ranks on 2 x 2 x 2.  The faithful oracle mode reproduces the
    reference's per-rank order, charges and forces, iteration counts included; with the field the per-step LinearMomentum sums
    (main.F90:70-71,766-797) are all-reduced.  Step 0 has every shell on its core (no beyond-cut-off look-up): there the clean mode --
    what the HIP engine computes -- must give the same numbers bit for bit."""
    g, o, nr = _multirank_oracle(case, pqeq=oa.PQEQ_SICNP, QEq_tol=1e-12, NMAXQEq=2000)
    if efield:
        o.set_efield(*efield)
    iters = [o.qeq()]; o.force()
    for _ in range(steps):
        o.step(1); iters.append(o.L.rxo_qeq_iters(o.w))
    assert iters == [int(x) for x in g["qeq_iters"]]
    _compare_ranks(g, o, nr)
    if steps == 0:
        assert o.pqeq_stale() == 0
        g2, o2, _ = _multirank_oracle(case, pqeq=oa.PQEQ_SICNP, QEq_tol=1e-12, NMAXQEq=2000)
        o2.set_pqeq_clean(1); o2.qeq(); o2.force()
        for r in range(nr):
            assert np.array_equal(o2.charges(r), o.charges(r)) and np.array_equal(o2.forces(r), o.forces(r))


def test_multirank_extended_lagrangian_vs_real_mpi_reference():
    """isQEq 2 on two ranks, 10 steps: one CG step per MD step, the fictitious charges qsfp / qsfv integrated by the driver and carried
    by MODE_MOVE with their atom (comm.F90:159-163)"""
    g, o, nr = _multirank_oracle("rdx222_v211_lex_md10", isQEq=2)
    o.qeq(); o.force(); o.step(10)
    _compare_ranks(g, o, nr)


@pytest.mark.parametrize("mode,kw", [(4, dict(vsfact=0.9)), (5, dict(treq=300.0)), (7, dict(treq=300.0)), (8, dict(treq=300.0))])
def test_multirank_velocity_scaling_modes_vs_real_mpi_reference(mode, kw):
    """mdmode 4/5/7/8 on two ranks from the reference's own two-rank restart file: per-element counts and kinetic energies, the total
    kinetic energy and the momentum removal are MPI_ALLREDUCEd (main.F90:699,738,783)"""
    g = np.load(os.path.join(GOLD, "rdx222_v211_thermo%d.npz" % mode))
    ff = oa.make_system("rdx222")[0]
    o, recs, lat = oa.oracle_from_rxff(ff, g["restart_rxff"], QEq_tol=1e-12, NMAXQEq=2000)
    assert len(recs) == 2
    o.qeq(); o.force()
    n = sum(len(r) for r in recs)
    for nstep in range(7):
        if nstep % 3 == 0:
            o.thermostat(mode, gke=o.kinetic() / n, **kw)
        o.step(1)
    _compare_ranks(g, o, 2, qtol=1e-10, ftol=1e-8)


@pytest.mark.parametrize("case,steps", [("sicnp547_pqeq_tol7", 0), ("sicnp547_pqeq_tight", 0), ("sicnp547_pqeq_md5", 5)])
def test_pqeq_sicnp_against_reference(case, steps):
    """PQEq path (pqeq.F90, ENbond_PQEq, shell update) of the oracle against the reference run with --pqeq on conf/init.sicnp"""
    kw = dict(QEq_tol=1e-12, NMAXQEq=2000) if "tight" in case else {}
    g, o, iters, pe = _run(case, (1, 1, 1), steps=steps, pqeq=oa.PQEQ_SICNP, **kw)
    assert iters == [int(x) for x in g["qeq_iters"]]
    _compare(g, o, ftol=1e-9, qtol=1e-10)
    if steps == 0:
        _check_energy(g, pe, 547)
        assert (o.get(104).astype(int) == g["hess_nnz"]).all()
        assert np.allclose(o.get(108), g["hess_rowsum"], rtol=1e-13)
    # step 0 has every shell on its core: no core-shell / shell-shell lookup can fall outside the cutoff when the core pair is
    # inside.  Once shells move it happens (170 times in these 5 steps) and the reference then re-uses the previous pair's value
    # (module.F90:401 returns without touching its outputs); the oracle restates that, which is why the trajectory still matches.
    assert (o.pqeq_stale() == 0) == (steps == 0)


def test_pressure_column_of_the_mdstep_line():
    """ss of the reference's MDstep line (main.F90:233,252,261; f8.2) = sum(astr(1:3))/3/MDBOX*USTRS: pins the virial
    (pot.F90:65-72, positions of residents AND ghosts times their pre-fold forces) and the kinetic part (main.F90:86-94)"""
    USTRS = 6.94728103
    g = np.load(os.path.join(GOLD, "rdx168_md10.npz"))
    ff, names, frac, lat = oa.make_system("rdx168")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff))
    o = oa.Oracle(ff, lat2, ranks)
    o.qeq(); o.force()
    for row in range(len(g["mdstep"])):
        a = o.astr(reset=True)
        ss = a[:3].sum() / 3.0 / o.mdbox() * USTRS
        assert abs(ss - g["mdstep"][row][11]) <= 0.0051, (row, ss, g["mdstep"][row][11])
        o.step(1)


def test_extended_lagrangian_charges_isQEq2():
    """isQEq = 2 (qeq.F90:51-57,66; main.F90:67-68,98): one CG step per call from the mixed fictitious charges"""
    g, o, iters, pe = _run("rdx168_lex_md10", (1, 1, 1), steps=10, isQEq=2)
    _compare(g, o, ftol=1e-9, qtol=1e-10)
    assert all(i <= 1 for i in iters)


@pytest.mark.parametrize("mode,kw", [(4, dict(vsfact=0.9)), (5, dict(treq=300.0)), (7, dict(treq=300.0)), (8, dict(treq=300.0))])
def test_velocity_scaling_modes_from_a_restart_file(mode, kw):
    """mdmode 4/5/7/8 (main.F90:45-61, ScaleTemperature, AdjustTemperature, LinearMomentum): 7 steps with sstep 3 continued from the
    reference's own restart file (20 NVE steps), against the reference's dump of the last step"""
    g = np.load(os.path.join(GOLD, "rdx168_thermo%d.npz" % mode))
    ff = oa.make_system("rdx168")[0]
    o, recs, lat = oa.oracle_from_rxff(ff, g["restart_rxff"], QEq_tol=1e-12, NMAXQEq=2000)
    o.qeq(); o.force()
    n = len(recs[0])
    for nstep in range(7):
        if nstep % 3 == 0:
            o.thermostat(mode, gke=o.kinetic() / n, **kw)
        o.step(1)
    _compare(g, o, ftol=1e-8, qtol=1e-10)


def test_pqeq_with_electric_field():
    """--efield 3 0.05: field force on cores (EEfield, module.F90:359-383), on shells (pqeq.F90:205) and the momentum removal of
    every step (main.F90:70-71), 3 MD steps against the reference"""
    g = np.load(os.path.join(GOLD, "sicnp547_pqeq_efield_md3.npz"))
    ff, names, frac, lat = oa.make_system("sicnp")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff))
    o = oa.Oracle(ff, lat2, ranks, pqeq=oa.PQEQ_SICNP, QEq_tol=1e-12, NMAXQEq=2000)
    o.set_efield(3, 0.05)
    o.qeq(); o.force(); o.step(3)
    _compare(g, o, ftol=1e-9, qtol=1e-10)


def _pqeq_frame(txt):
    """PQEq trajectory frame (WriteXYZ, fileio.F90:241-355): per atom position 3es20.12, charge es20.12, global id i9, shell displacement 3es20.12"""
    t = str(txt).split("\n")[2:-1]
    val = np.array([[float(x) for x in l[3:83].split()] + [float(x) for x in l[92:].split()] for l in t])
    ids = np.array([int(l[83:92]) for l in t])
    o = np.argsort(ids)
    return ids[o], val[o, :3], val[o, 3], val[o, 4:]


def test_pqeq_md_on_an_isolated_cluster_has_no_stale_lookup_and_matches_the_reference():
    """PQEq MD pinned to the reference WITHOUT the stale-value artefact: an isolated 26-atom SiC + O2 cluster (diameter 11.1 A) in a
    40 A box has no pair anywhere near the 12.5 A cut-off, so no core-shell / shell-shell look-up can fall outside it
    (pqeq_stale() == 0 in faithful mode) and the reference's own 8-step trajectory (field along x, shells moving) is the clean one.
    Both oracle modes must therefore give the SAME numbers, and both must be the reference's: positions, charges, forces of its
    dump and the shell displacements of its frame."""
    g = np.load(os.path.join(GOLD, "sicfrag26_pqeq_efieldx_md8.npz"))
    ff, names, frac, lat = oa.make_system("sicfrag")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff))
    ids, xpos, xq, xsp = _pqeq_frame(g["xyz_last"])
    res = []
    for clean in (0, 1):
        o = oa.Oracle(ff, lat2, ranks, pqeq=oa.PQEQ_SICNP, QEq_tol=1e-12, NMAXQEq=2000)
        o.set_efield(1, 0.05); o.set_pqeq_clean(clean)
        iters = [o.qeq()]; o.force()
        for _ in range(8):
            o.step(1); iters.append(o.L.rxo_qeq_iters(o.w))
        assert o.pqeq_stale() == 0
        assert iters == [int(x) for x in g["qeq_iters"]]
        _compare(g, o, ftol=1e-9, qtol=1e-10)
        order = np.argsort(o.gids())
        assert (o.gids()[order] == ids).all()
        assert np.abs(o.spos()[order] - xsp).max() <= 1e-12
        assert np.abs(o.charges()[order] - xq).max() <= 1e-11
        assert np.linalg.norm(xsp, axis=1).max() > 1e-3          # the shells did move (8 clipped 1e-3 A moves at most)
        res.append((o.charges().copy(), o.forces().copy(), o.spos().copy()))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


def test_low_gradient_dispersion_tables():
    """--lg: the LG ffield format (param.F90:83-86,107-109,197-200) and the table terms of init.F90:496-514, on the reference's own
    conf/init.rdx.lg input; step 0 at the tight tolerance, then the 5-step trajectory with its iteration counts"""
    g, o, iters, pe = _run("rdx168_lg_tight", (1, 1, 1), QEq_tol=1e-12, NMAXQEq=2000, lg=True)
    assert iters[0] == int(g["qeq_iters"][0])
    _compare(g, o)
    _check_energy(g, pe, 168)
    g0 = np.load(os.path.join(GOLD, "rdx168_tight.npz"))
    assert abs(g["mdstep"][0][2] - g0["mdstep"][0][2]) > 1e-3       # not the plain RDX answer: the correction is really on
    g, o, iters, pe = _run("rdx168_lg_md5", (1, 1, 1), steps=5, lg=True)
    assert iters == [int(x) for x in g["qeq_iters"]]
    _compare(g, o, ftol=1e-9, qtol=1e-10)


def test_reference_example3_frame_including_its_stale_lookup_artefact():
    """examples/3-reaxpq+ as shipped (polyethylene 2x3x5, PQEq with a parameter file that lists only C and H, field along x): in this
    12.7 A box the 12.5 A PQEq cut-off makes the reference re-use the previous pair's table values on ~1,500 lookups beyond the
    cut-off (module.F90:401).  The reference-faithful oracle mode reproduces the reference's frame after 20 steps to dump precision;
    the clean mode (what the HIP engine computes) differs from it by exactly the artefact: single charges by ~1e-2, shells by the clip."""
    g = np.load(os.path.join(GOLD, "example3.npz"))
    ff, names, frac, lat = oa.make_system("example3")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=(2, 3, 5))
    t = str(g["xyz_last"]).split("\n")[2:-1]
    ref = np.array([[float(x) for x in l[3:83].split()] + [float(x) for x in l[92:].split()] for l in t])
    ids = np.array([int(l[83:92]) for l in t])
    out = {}
    for clean in (0, 1):
        o = oa.Oracle(ff, lat2, ranks, pqeq=oa.PQEQ_EXAMPLE3)
        o.set_efield(1, 0.01); o.set_pqeq_clean(clean)
        o.qeq(); o.force()
        assert abs(o.energy()[0] / 360 - g["mdstep"][0][2]) <= 1e-5 * abs(g["mdstep"][0][2])
        o.step(20)
        order = np.argsort(o.gids())
        q = o.charges()[order][ids - 1]; sp = o.spos()[order][ids - 1]; pos = o.pos()[order][ids - 1]
        out[clean] = (np.abs(pos - ref[:, :3]).max(), np.abs(q - ref[:, 3]).max(), np.abs(sp - ref[:, 4:]).max(), o.pqeq_stale())
    assert out[0][0] <= 1e-10 and out[0][1] <= 1e-12 and out[0][2] <= 1e-12 and out[0][3] > 1000
    assert out[1][0] <= 1e-5 and 1e-3 < out[1][1] <= 3e-2 and out[1][2] <= 2.5e-3


@pytest.mark.parametrize("case", ["fes576_md3", "mos2_216_md3", "mos2_tri324_md3", "sic512_md3", "aloslab180_md3", "pbt2272_md2"])
def test_other_force_fields_and_systems_the_reference_ships(case):
    """conf/init.fes (pyrite, a 10-type ffield), conf/init.mos2.ortho (4 types), conf/init.sic (zinc-blende SiC) and conf/init.aloslab
    (alumina slab, 5 types), conf/init.a-polys/PBT (amorphous poly(butylene terephthalate), 2,272 atoms): ffield parsing, cut-offs and
    every energy term on systems other than RDX; 2-3 MD steps at tight tolerance"""
    g = np.load(os.path.join(GOLD, case + ".npz"))
    g2, o, iters, pe = _run(case, tuple(int(x) for x in g["mc"]), steps=int(g["nsteps"]), QEq_tol=1e-12, NMAXQEq=2000)
    assert iters == [int(x) for x in g["qeq_iters"]]
    _compare(g, o, ftol=1e-9, qtol=1e-10)


def test_charges_every_third_step_only():
    """rxmd.in `QEq 1 2000 1.d-12 3`: QEq runs when mod(nstep, qstep) == 0 (main.F90:77), the charges are frozen in between"""
    g = np.load(os.path.join(GOLD, "rdx168_qstep3_md7.npz"))
    ff, names, frac, lat = oa.make_system("rdx168")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff))
    o = oa.Oracle(ff, lat2, ranks, QEq_tol=1e-12, NMAXQEq=2000)
    o.set_qstep(3)
    iters = [o.qeq()]; o.force()
    for s in range(7):
        o.step(1)
        if s % 3 == 0:
            iters.append(o.L.rxo_qeq_iters(o.w))
    assert iters == [int(x) for x in g["qeq_iters"]]
    _compare(g, o, ftol=1e-9, qtol=1e-10)


def test_bond_file_and_pdb_formatters_against_the_references_files():
    """rxmd_amd.system.format_bnd / format_pdb (the host side of RxmdEngine.write_bnd / write_pdb) fed with the oracle's state after the
    same 10 steps, against the files the reference wrote with --isBondFile --isPDB (WriteBND fileio.F90:27-148, WritePDB :151-238):
    line structure, ids, partner order and the fixed columns exactly, the printed numbers to their last digit."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from rxmd_amd import system
    g = np.load(os.path.join(GOLD, "rdx168_md10.npz"))
    ff, names, frac, lat = oa.make_system("rdx168")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=(1, 1, 1))
    o = oa.Oracle(ff, lat2, ranks); o.qeq(); o.force(); o.step(10)
    nbr, bo = o.bonds()
    gid = o.gids(); n = len(gid); gall = o.get(106).astype(np.int64); typ = o.get(4).astype(int)
    cnt = (nbr[:n] > 0).sum(axis=1)
    pg = np.zeros((n, 32), np.int64); b = np.zeros((n, 32))
    for i in range(n):
        pg[i, :cnt[i]] = gall[nbr[i, :cnt[i]] - 1]; b[i, :cnt[i]] = bo[i, :cnt[i]]
    mine = system.format_bnd(gid, typ, o.pos(), cnt, pg, b).split("\n"); theirs = str(g["bnd_last"]).split("\n")
    assert len(mine) == len(theirs) == n + 1
    same = 0
    for x, y in zip(mine[:-1], theirs[:-1]):
        tx, ty = x.split(), y.split()
        assert len(tx) == len(ty) and tx[0] == ty[0] and tx[4:6] == ty[4:6] and tx[6::2] == ty[6::2], (x, y)
        assert np.abs(np.array([float(v) for v in tx[1:4] + tx[7::2]]) - np.array([float(v) for v in ty[1:4] + ty[7::2]])).max() <= 1.01e-3
        same += x == y
    assert same >= 0.97 * n, same
    tnames = [""] + oa.ffield_names(ff)
    mine = system.format_pdb(tnames, gid, typ, o.pos(), o.charges(), astr=(1e9, 1e9, 1e9)).split("\n"); theirs = str(g["pdb_last"]).split("\n")
    assert len(mine) == len(theirs) == n + 1
    same = 0
    for x, y in zip(mine[:-1], theirs[:-1]):
        assert len(x) == len(y) == 66 and x[:30] == y[:30] and x[60:] == y[60:] == "******", (x, y)
        assert max(abs(float(x[30 + 8 * c:38 + 8 * c]) - float(y[30 + 8 * c:38 + 8 * c])) for c in range(3)) <= 1.01e-3
        assert abs(float(x[54:60]) - float(y[54:60])) <= 1.01e-2
        same += x == y
    assert same >= 0.97 * n, same


def test_off_lattice_systems_stay_in_their_regimes():
    """The dense, dilute and shaken boxes of test_gpu_offlattice.py (offlattice_systems.py), built with the oracle alone: each must keep the property it
    exists for -- bond lists longer than 15 / 24, 10 A rows longer than 512 / 1024 or shorter than 128, an atom without a bond -- and the box compressed
    to 0.70 must run into the reference's MAXNEIGHBS trap (main.F90:402-407).  A change of the inputs or of the oracle that moves a case out of its
    regime shows here, without a GPU."""
    import offlattice_systems as ol
    seen = {}
    for name in ol.NAMES:
        o = ol.oracle(name, isQEq=1, NMAXQEq=5, QEq_tol=1e-300)
        assert o.qeq() == 5
        o.force()
        seen[name] = ol.regime(o)
        ol.check_gates(name, seen[name])
        assert np.isfinite(o.energy()).all() and np.isfinite(o.forces()).all()
    assert seen["rdx-dense"]["natoms"] == 1344 and seen["ice-dense"]["natoms"] == 2304
    assert seen["rdx-dense"]["max_nb"] <= 24 < seen["rdx-denser"]["max_nb"] <= 30       # the two sides of the angle kernel's 8 / 4 centres per wavefront
    assert 12 < seen["rdx-shaken"]["max_nb"] <= 15 and 12 < seen["ice-dense"]["max_nb"] <= 15   # eight centres per wavefront, packed torsion instance
    with pytest.raises(RuntimeError, match="overflow of max # in neighbor list"):
        o = ol.oracle("rdx-trap", isQEq=1, NMAXQEq=5, QEq_tol=1e-300)
        o.qeq(); o.force()
