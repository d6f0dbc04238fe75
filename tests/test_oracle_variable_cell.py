"""The oracle's own lattice change (rxo_set_lattice, tests/oracle_api.py Oracle.set_lattice) and the numpy Berendsen loop around it
(tests/npt_reference.py), pinned before the engine is compared with them (tests/test_gpu_variable_cell_oracle.py).

The reference has no such routine, so the yardstick is the oracle's set-up itself: an oracle moved to a lattice must be the oracle that
rxo_init builds at that lattice from the same normalised records.  The fresh one gets its positions as H' s and the live one as
H' (H^-1 r): two exact routes that differ by rounding only (matinv costs a few ulps times the box length), so positions are gated at
1e-11 A and, at QEq_tol 1e-12 from equal start charges, energies at 1e-10 relative, charges and forces at 1e-8 and astr at 1e-9 (the
project's gates for "the same computation, inputs differ by rounding", test_set_lattice_equals_a_fresh_engine_and_the_oracle)."""
import numpy as np
import pytest

import oracle_api as oa
import npt_reference as npt
from parity import q_err, f_err, e_err

TIGHT = dict(QEq_tol=1e-12, NMAXQEq=2000)
SYSTEMS = {"rdx222": (2, 2, 2), "ice644": (6, 4, 4), "mos2_tri324": (3, 3, 2), "sicnp547": (1, 1, 1)}


def build(case, lat=None, vp=(1, 1, 1), ranks=None, **kw):
    """(oracle, lattice of the input, the per-rank records) of a named system; with PQEq for sicnp (clean look-ups: the stale ones of the
    reference depend on the pair order of everything computed before, which a fresh oracle has not computed)"""
    ff, names, frac, lat0 = oa.make_system(case)
    lat2, rk = oa.geninit(names, frac, lat0, oa.ffield_names(ff), mc=SYSTEMS[case], vprocs=vp)
    pq = oa.PQEQ_SICNP if case.startswith("sicnp") else None
    o = oa.Oracle(ff, lat or lat2, ranks or rk, vprocs=vp, pqeq=pq, **TIGHT, **kw)
    if pq:
        o.set_pqeq_clean(1)
    return o, [float(x) for x in lat2], rk


def changed_lattice(kind, L0, maxrc, vp):
    """the lattice changes of the issue, for any box: lengths only; angles and lengths (every entry of the remap matrix's upper triangle
    is exercised); the smallest compression of one axis that lowers a bond-cell count; the smallest length change that changes a 10 A
    mesh count"""
    L = list(L0)
    if kind == "lengths":
        return [L[0] * 0.98, L[1] * 1.02, L[2] * 1.01] + L[3:]
    if kind == "angles":
        return [L[0] * 1.03, L[1] * 0.98, L[2] * 1.01, L[3] - 3.0, L[4] + 2.0, L[5] - 2.5]
    lb = np.array(L[:3]) / np.array(vp)
    if kind == "cc":
        x = lb / maxrc
        a = int(np.argmin(x - np.floor(x)))
        L[a] = vp[a] * (np.floor(x[a]) * maxrc - 0.05)
        return L
    if kind == "nbcc":
        x = lb / 3.0
        up, dn = np.ceil(x + 1e-12) - x, x - np.floor(x)
        a = int(np.argmin(np.minimum(up, dn)))
        L[a] = vp[a] * 3.0 * ((np.floor(x[a]) - 0.02) if dn[a] <= up[a] else (np.floor(x[a]) + 1.02))
        return L
    raise KeyError(kind)


def evaluate(o):
    o.astr(reset=True); it = o.qeq(); o.force()
    n = o.nranks
    return dict(it=it, gid=[o.gids(r) for r in range(n)], pos=[o.pos(r) for r in range(n)], q=[o.charges(r) for r in range(n)],
                f=[o.forces(r) for r in range(n)], spos=[o.spos(r) for r in range(n)], pe=o.energy(), astr=o.astr(reset=False))


def compare(a, b, tag="", pqeq_rounded=False):
    """the live oracle's evaluation a against the fresh one's b; pqeq_rounded: see test_set_lattice_equals_a_fresh_oracle"""
    figs = dict(pos=0.0, q=0.0, f=0.0)
    for r in range(len(b["gid"])):
        assert (a["gid"][r] == b["gid"][r]).all(), "gid order"
        figs["pos"] = max(figs["pos"], np.abs(a["pos"][r] - b["pos"][r]).max())
        figs["q"] = max(figs["q"], q_err(a["q"][r], b["q"][r]))
        figs["f"] = max(figs["f"], f_err(a["f"][r], b["f"][r]))
    figs["pe"] = e_err(a["pe"], b["pe"])
    figs["astr"] = np.abs(a["astr"] - b["astr"]).max() / np.abs(b["astr"]).max()
    print("%s live vs fresh: pos %.2e A, q %.2e, f %.2e, energies %.2e, astr %.2e, CG iterations %d / %d" % (tag, figs["pos"], figs["q"], figs["f"], figs["pe"], figs["astr"], a["it"], b["it"]))
    assert figs["pos"] <= 1e-11
    if pqeq_rounded:
        figs["pe_total"] = np.abs(a["pe"] - b["pe"]).max() / abs(b["pe"][0])
        print("   energies on the scale of the total %.2e" % figs["pe_total"])
        assert figs["q"] <= 1e-6 and figs["f"] <= 1e-6      # QTOL, FTOL of the parity tests; the energies are printed (see the docstring)
        return figs
    assert figs["q"] <= 1e-8 and figs["f"] <= 1e-8
    assert figs["pe"] <= 1e-10
    assert figs["astr"] <= 1e-9
    return figs


def fresh_like(case, live, L1, vp, rk, q, shells=None, v=None, lex=None):
    """a fresh oracle at L1 from the records rk, given the start charges (and shells, velocities, Lex state) of the live one"""
    f, _, _ = build(case, lat=L1, vp=vp, ranks=rk, q0=q, v0=v)
    for r in range(f.nranks):
        if shells is not None:
            f.set_shells(shells[r], r)
        if lex is not None:
            f.set_lex(lex[r][0], lex[r][1], r)
    return f


CASES = [(c, k, (1, 1, 1)) for c in SYSTEMS for k in ("lengths", "angles", "cc", "nbcc")] + \
        [(c, k, vp) for c in ("rdx222", "ice644", "mos2_tri324") for k in ("angles", "cc") for vp in ((2, 1, 1), (1, 1, 2))] + \
        [("rdx222", "nbcc", (1, 1, 2)), ("sicnp547", "angles", (2, 1, 1))]


@pytest.mark.parametrize("case,kind,vp", CASES)
def test_set_lattice_equals_a_fresh_oracle(case, kind, vp):
    """set_lattice(L1), QEq, FORCE on a live oracle against a fresh oracle built at L1 from the same records and start charges.

    PQEq (sicnp547) does NOT meet the 1e-10 energy gate in this form, and the cause is not set_lattice.  Measured live against fresh:
    charges 1e-8 .. 2.6e-7, forces <= 5e-9, energy terms 7e-9 .. 8.3e-7 of their own size, from positions 2e-13 A apart.  With the step
    length of the PQEq CG kept in double (a scratch build) the gap stays (5e-6): it is not the REAL(4) step length.  PQEq's CG leaves when
    Est stops changing at QEq_tol relative, after 16-24 iterations, which at 1e-12 is decided by rounding: the charges it stops at are
    defined to ~1e-7 only (the engine shows the same against a fresh engine, test_pqeq_shells_follow_the_lattice).  Handed the live
    oracle's positions and shells bit for bit, the fresh oracle reproduces the live one EXACTLY (0.0 in every quantity, the same iteration
    count).  So the check is split for PQEq, each half at or inside the gate: (i) positions within 1e-11 A of H' s and shells within
    rounding of M d; (ii) with those inputs made bit-equal, QEq + FORCE within the gates (measured: identical) -- which is what pins the
    box-dependent state; (iii) with the rounded inputs, the parity gates QTOL and FTOL on charges and forces, the energies printed (largest
    term difference 4e-11 .. 1.3e-9 of the total energy).  Every other system is held to the gates as they stand, in both forms."""
    o, L0, rk = build(case, vp=vp)
    pq = case.startswith("sicnp")
    i0 = o.info()
    L1 = changed_lattice(kind, L0, i0[0], vp)
    o.qeq(); o.force()                                   # a live oracle: lists, charges, forces, astr (and moved PQEq shells) of L0 exist
    n = o.nranks
    q0 = [o.charges(r) for r in range(n)]; d0 = [o.spos(r) for r in range(n)]
    v0, f0 = [o.vel(r) for r in range(n)], [o.forces(r) for r in range(n)]
    if pq:
        assert max(np.abs(d).max() for d in d0) > 1e-6, "the shells must have moved before the lattice changes"
    o.set_lattice(L1)
    i1 = o.info()
    M = npt.remap_matrix(L0, L1)
    if kind == "angles":
        assert min(abs(M[0, 1]), abs(M[0, 2]), abs(M[1, 2])) >= 1e-3, M
    if kind == "cc":
        assert (i1[1:4] <= i0[1:4]).all() and (i1[1:4] < i0[1:4]).any(), (i0[1:7], i1[1:7])
    if kind == "nbcc":
        assert (i1[4:7] != i0[4:7]).any(), (i0[1:7], i1[1:7])
    for r in range(n):                                   # what set_lattice must leave alone
        assert np.array_equal(o.charges(r), q0[r]) and np.array_equal(o.vel(r), v0[r]) and np.array_equal(o.forces(r), f0[r])
        if pq:
            assert np.abs(o.spos(r) - d0[r] @ M.T).max() <= 1e-13 * max(np.abs(d0[r]).max(), 1e-300) + 1e-18
    a = evaluate(o)
    f = fresh_like(case, o, L1, vp, rk, q0, shells=[d @ M.T for d in d0] if pq else None)
    assert (f.info()[1:14] == i1[1:14]).all()            # cc, nbcc, lcsize, nblcsize, mesh size: what rxo_init derives at L1
    tag = "%s %s %s:" % (case, kind, vp)
    compare(a, evaluate(f), tag, pqeq_rounded=pq)
    # the same with bit-equal inputs: what is left is the box-dependent state alone
    o2, _, _ = build(case, vp=vp)
    o2.qeq(); o2.force(); o2.set_lattice(L1)
    g = fresh_like(case, o2, L1, vp, rk, q0)
    for r in range(n):
        assert np.abs(g.pos(r) - o2.pos(r)).max() <= 1e-11
        g.set_pos(o2.pos(r), r)
        if pq:
            g.set_shells(o2.spos(r), r)
    compare(evaluate(o2), evaluate(g), tag + " bit-equal inputs,")


@pytest.mark.parametrize("case,vp", [("rdx222", (1, 1, 1)), ("mos2_tri324", (2, 1, 1)), ("ice644", (1, 1, 2))])
def test_there_and_back(case, vp):
    """L0 -> L1 (angles and lengths) -> L0: the positions return to 1e-11 A and QEq + FORCE give the L0 energies again to 1e-10
    (not with PQEq: every PQEq call moves the shells, so no evaluation repeats an earlier one)"""
    o, L0, rk = build(case, vp=vp)
    e0 = evaluate(o)
    q0 = e0["q"]
    L1 = changed_lattice("angles", L0, o.info()[0], vp)
    o.set_lattice(L1); evaluate(o)
    o.set_lattice(L0)
    for r in range(o.nranks):
        assert np.abs(o.pos(r) - e0["pos"][r]).max() <= 1e-11
        o.set_charges(np.zeros(len(q0[r])), r)           # the start vector of the first evaluation
    e1 = evaluate(o)
    d = e_err(e1["pe"], e0["pe"])
    print("%s %s there and back: energies %.2e" % (case, vp, d))
    assert d <= 1e-10


def test_rejected_lattices_change_nothing():
    o, L0, _ = build("mos2_tri324")
    o.qeq(); o.force()
    maxrc = o.info()[0]
    p0, i0 = o.pos(), o.info()
    for L in ([-L0[0]] + L0[1:], L0[:3] + [90.0, 90.0, 180.0], L0[:3] + [120.0, 120.0, 120.0], [L0[0], L0[1], 0.9 * maxrc] + L0[3:]):
        with pytest.raises(RuntimeError):
            o.set_lattice(L)
        assert np.array_equal(o.pos(), p0) and (o.info() == i0).all()
    o2, L2, _ = build("rdx222", vp=(1, 1, 2))
    with pytest.raises(RuntimeError, match="shorter than maxrc"):
        o2.set_lattice(L2[:2] + [1.9 * o2.info()[0]] + L2[3:])      # the LOCAL box is what counts


def _velocities(n, seed, sigma):
    return np.random.default_rng(seed).normal(0.0, sigma, (n, 3))


def _by_rank(v, rk):
    return [v[g["gid"] - 1] for g in rk]


def squeezed_rdx(vp):
    """recipe of the squeezed box: rdx222 with z just above a bond-cell threshold, driven down by a per-axis barostat whose clamp binds"""
    o, L0, rk = build("rdx222", vp=vp)
    maxrc = o.info()[0]
    cz = int(L0[2] / vp[2] / maxrc)
    L = L0[:2] + [vp[2] * (cz * maxrc + (0.12 if vp[2] == 1 else 0.10))] + L0[3:]
    return L0, L, rk, cz


def test_berendsen_run_adds_nothing_between_couplings():
    """every larger than the run: bit for bit step(n)"""
    v = _velocities(1344, 5, 0.02)
    runs = []
    for helper in (False, True):
        o, L0, rk = build("rdx222", v0=[v])
        o.qeq(); o.force()
        if helper:
            L, rows = npt.berendsen_run(o, L0, 4, 1, 0.0, 25.0, 15.0, every=100)
            assert rows == [] and L == L0
        else:
            o.step(4)
        runs.append((o.pos(), o.vel(), o.charges(), o.forces(), o.astr(reset=False), o.energy()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_berendsen_pressure_bookkeeping_written_down_twice():
    """one coupling by hand (every = 2, one step already taken): the step that couples is the one whose total count becomes 2, its sums are
    astr after minus astr before that step, the volume is the one of the lattice the step ran at"""
    v = _velocities(1344, 6, 0.02)
    def start():
        o, L0, _ = build("rdx222", v0=[v]); o.qeq(); o.force(); o.step(1); return o, L0
    o, L0 = start()
    L, rows = npt.berendsen_run(o, L0, 3, 1, 1.0, 25.0, 15.0, every=2, max_strain=0.01, steps_done=1)
    assert [r["step"] for r in rows] == [2, 4]
    h, _ = start()
    a0 = h.astr(reset=False); h.step(1); a1 = h.astr(reset=False)
    a, b, c = L0[:3]
    P = (a1 - a0) / (a * b * c) * 6.94728103             # (orthorhombic)
    assert np.abs(rows[0]["p6"] - P).max() <= 1e-13 * np.abs(P).max()
    mu = np.cbrt(1.0 - 2 * 0.25 / 25.0 * (1.0 - P[:3].mean()) / 15.0)
    assert 0.99 < mu < 1.01 and abs(mu - 1.0) > 1e-6
    assert np.abs(rows[0]["mu"] - mu).max() <= 1e-15
    assert rows[0]["new"] == [a * rows[0]["mu"][0], b * rows[0]["mu"][1], c * rows[0]["mu"][2]] + L0[3:]
    h.set_lattice(rows[0]["new"]); h.step(1)             # step 3: no coupling
    a2 = h.astr(reset=False); h.step(1); a3 = h.astr(reset=False)
    P2 = (a3 - a2) / npt.volume(rows[0]["new"]) * 6.94728103
    assert np.abs(rows[1]["p6"] - P2).max() <= 1e-13 * np.abs(P2).max()


@pytest.mark.parametrize("vp", [(1, 1, 1), (1, 1, 2)])
def test_state_after_five_couplings_is_what_init_builds(vp):
    """the squeezed box: a per-axis barostat compresses z through a bond-cell threshold (cc_z drops inside the run).  The live oracle's state
    handed to a fresh oracle at the final lattice gives the same QEq + FORCE: the box-dependent state of an oracle that changed its lattice
    six times is what rxo_init would have made"""
    L0, L, rk, cz = squeezed_rdx(vp)
    v = _velocities(1344, 11, 0.02)
    o, _, _ = build("rdx222", vp=vp, v0=_by_rank(v, rk))
    o.set_lattice(L); o.qeq(); o.force()
    assert o.info()[3] == cz
    Lf, rows = npt.berendsen_run(o, L, 6, 2, (0.0, 0.0, 2000.0), 25.0, 15.0, every=1, max_strain=0.002, axes=4)
    assert len(rows) == 6 and all(r["mu"][2] == 1.0 - 0.002 and r["mu"][0] == 1.0 and r["mu"][1] == 1.0 for r in rows)
    assert o.info()[3] == cz - 1 and Lf[0] == L[0] and Lf[1] == L[1]
    n = o.nranks
    Hi = np.linalg.inv(npt.hmat(Lf))
    vpa = np.array(vp, float)
    state = []
    for r in range(n):
        obox = np.array([r % vp[0], (r // vp[0]) % vp[1], r // (vp[0] * vp[1])]) / vpa
        state.append(dict(rnorm=o.pos(r) @ Hi.T - obox, type=o.types(r), gid=o.gids(r)))
    q, vv, lex = [o.charges(r) for r in range(n)], [o.vel(r) for r in range(n)], [o.lex(r) for r in range(n)]
    f = fresh_like("rdx222", o, Lf, vp, state, q, v=vv, lex=lex)
    assert (f.info()[1:14] == o.info()[1:14]).all()
    compare(evaluate(o), evaluate(f), "rdx222 %s after 6 couplings:" % (vp,))
    print("   max |f| %.1f kcal/mol/A, residents per rank %s" % (max(np.abs(o.forces(r)).max() for r in range(n)), [len(o.gids(r)) for r in range(n)]))
