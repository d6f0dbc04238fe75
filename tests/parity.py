"""Support module (pytest does not collect it): what the GPU tests, the ranks they spawn and scripts/ share when they hold the engine to the oracle --
the engine and the oracle of a named system, the parity metrics and their tolerances (derived in tests/test_gpu_parity.py), the ten-double record
of a rank, and the lattices and perturbed crystals that more than one file builds.  Nothing here imports rxmd_amd before it is called, so a
CPU-only test can use the metrics."""
import numpy as np

import oracle_api as oa

QTOL = 1e-6
FTOL = 1e-6
ETOL = 1e-9


def _engine(case, mc, **kw):
    import rxmd_amd
    from rxmd_amd import system
    ff, names, frac, lat = oa.make_system(case)
    lat3, rec = system.geninit(ff, names, frac, lat, mc=mc, lg=kw.get("lg", False))
    e = rxmd_amd.RxmdEngine(ff, lat3, **kw)
    e.set_atoms_rxff(rec)
    return e


def _oracle(case, mc, **kw):
    ff, names, frac, lat = oa.make_system(case)
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff, lg=kw.get("lg", False)), mc=mc)
    return oa.Oracle(ff, lat2, ranks, **kw)


def q_err(q, qref):
    qrms = np.sqrt((qref ** 2).mean())
    return (np.abs(q - qref) / np.maximum(np.abs(qref), max(qrms, 1e-300))).max()


def f_err(f, fref):
    frms = np.sqrt((fref ** 2).mean())
    return (np.abs(f - fref).max(axis=1) / np.maximum(np.abs(fref).max(axis=1), frms)).max()


def e_err(pe, pref):
    return max(abs(a - b) / abs(b) for a, b in zip(pe, pref) if abs(b) > 1e-6)


def compare_bond_order_taps(E, O, n, box, rtol=1e-10):
    """E: the engine's taps, O: the oracle's.  Tolerance 1e-10, not 1e-12: the reference sends ALL positions through normalised coordinates and
    back in every COPYATOMS call (comm.F90:222-227,260-264; two calls per CG iteration), which moves them by ~1e-12 A before FORCE sees
    them; the engine keeps the residents where they are.  1e-12 A x d(BO')/dr of a few per A = the 1e-11 measured on delta'."""
    gidG = O["gidG"]
    for k in ("deltap", "delta", "cd"):
        assert np.abs(E[k] - O[k]).max() <= rtol * max(np.abs(O[k]).max(), 1.0), k
    cnt = E["cnt"]
    assert np.array_equal(cnt, O["cnt"].astype(cnt.dtype))
    for i in range(n):
        c = int(cnt[i])
        ge, go = E["pg"][i, :c], gidG[O["nbr"][i, :c] - 1]
        ie, io = np.lexsort((E["bo"][i, :c], ge)), np.lexsort((O["bo"][i, :c], go))      # an atom can be bonded to two images of one partner in a one-cell box
        assert np.array_equal(ge[ie], go[io])
        assert np.abs(E["bo"][i, :c][ie] - O["bo"][i, :c][io]).max(initial=0.0) <= rtol
    # ccbnd.  The reference evaluates a torsion i-j-k-l once, from the centre atom with the smaller gid, and scatters the coefficient of the
    # far bond k-l to WHICHEVER IMAGES of k and l that centre atom sees (pot.F90:1188-1215 -> ForceB); the engine books the far bond from k's
    # own visit of the torsion, i.e. on the image of k that is a centre atom there.  Forces are linear in ccbnd and
    # translation invariant, so after the CPBK fold both give the same forces, but per INDEX the two differ for atoms whose torsions cross
    # the box.  What must agree: ccbnd summed over the images of an atom, and ccbnd per index for atoms deeper inside the box than any
    # torsion reaches (3 bonds < 12 A) -- none in the boxes of 1-2 cut-offs, most of a 36k-atom box.
    G = len(gidG)
    scale = max(np.abs(O["cc"]).max(), 1.0)
    se = np.bincount(gidG, weights=E["cc"][:G]); so = np.bincount(gidG, weights=O["cc"][:G])
    assert np.abs(se - so).max() <= 1e-9 * scale
    depth = np.minimum(O["pos"][:n], box - O["pos"][:n]).min(axis=1)
    deep = depth > 12.0
    if deep.any():
        assert np.abs(E["cc"][:n][deep] - O["cc"][:n][deep]).max() <= 1e-9 * scale
    return int(deep.sum())


def code(call):
    """the error code the engine refuses `call` with, 0 if it does not"""
    import rxmd_amd
    try:
        call()
    except rxmd_amd.RxmdError as ex:
        return ex.code
    return 0


def rec10(rank, v=None):
    """the rxff record block of one rank, dict(rnorm, type, gid): rnorm, v, q = 0, type + gid * 1e-13"""
    n = len(rank["type"])
    rec = np.zeros((n, 10))
    rec[:, 0:3] = rank["rnorm"]
    if v is not None:
        rec[:, 3:6] = v
    rec[:, 7] = rank["type"] + rank["gid"] * 1e-13
    return rec


def _rec10_from_oracle(o, lat):
    """rxff.bin records of the oracle's present state (orthorhombic box, one rank)"""
    n = len(o.gids())
    rec = np.zeros((n, 10))
    rec[:, 0:3] = o.pos() / np.asarray(lat[:3]); rec[:, 3:6] = o.vel(); rec[:, 6] = o.charges()
    rec[:, 7] = o.types() + o.gids() * 1e-13
    return rec


# ---- lattices of the variable-cell tests that the poisoned run and the streams-by-place test walk through as well -------------------------------
def sheared(L0):
    """lengths times (1.03, 0.98, 1.01), alpha - 3, beta + 2, gamma - 2.5 degrees"""
    return [L0[0] * 1.03, L0[1] * 0.98, L0[2] * 1.01, L0[3] - 3.0, L0[4] + 2.0, L0[5] - 2.5]


def lattice_sequence(L0, maxrc):
    """3: expansion that adds 10 A grid cells on every axis, shear, z compressed below a bond-cell threshold, back"""
    cz = int(L0[2] / maxrc)
    return [("expanded", [L0[0] * 1.05, L0[1] * 1.05, L0[2] * 1.10] + L0[3:]), ("sheared", sheared(L0)),
            ("compressed", L0[:2] + [cz * maxrc - 0.05] + L0[3:]), ("back at L0", list(L0))]


# ---- perturbed RDX crystals ---------------------------------------------------------------------------------------------------------------------
# Three builders side by side, on purpose: _perturbed_rdx (tests/test_gpu_scale.py and its ranks), perturbed_rdx (tests/test_gpu_streams_by_place.py and
# its poisoned child) and build_system (the decomposed boxes of the graph and structure tests).  They differ in seed, size, in whether the box is
# scaled or dealt to a rank grid, and in how the velocities are drawn, and the goldens and yardsticks of their tests hang on exactly those draws.
MC = (6, 6, 6)
KW = dict(QEq_tol=1e-300, NMAXQEq=100)


def _perturbed_rdx(vprocs=(1, 1, 1)):
    """RDX 6x6x6 as geninit lays it out, every atom displaced by N(0, 0.05 A) per component, velocities N(0, 0.05) (230 K); with vprocs the
    atoms are dealt to the domains of the rank grid the way geninit does (geninit.F90:493-527) -> (ffield, lattice, per-rank dicts, per-rank v)"""
    ff, names, frac, lat = oa.make_system("rdx168")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=MC)
    rng = np.random.default_rng(2026)
    n = len(ranks[0]["type"])
    rn = ranks[0]["rnorm"] + rng.normal(0, 0.05, (n, 3)) / np.asarray(lat2[:3])
    # back into [0, 1) like geninit (geninit.F90:476-480) and every COPYATOMS(MODE_MOVE) leave them: a resident outside the box is not
    # a state the reference's driver produces (its QEq ghost shell of exactly rctap would miss partners of such an atom)
    rn = rn - np.floor(rn)
    v = rng.normal(0, 0.05, (n, 3))
    if tuple(vprocs) == (1, 1, 1):
        ranks[0]["rnorm"] = rn
        return ff, lat2, ranks, v
    vp = np.array(vprocs)
    dom = (rn * vp).astype(np.int64)
    sid = dom[:, 0] + dom[:, 1] * vp[0] + dom[:, 2] * vp[0] * vp[1]
    out, vs = [], []
    for p in range(int(vp.prod())):
        sel = np.nonzero(sid == p)[0]
        obox = (1.0 / vp) * np.array([p % vp[0], (p // vp[0]) % vp[1], p // (vp[0] * vp[1])])
        out.append(dict(rnorm=rn[sel] - obox, type=ranks[0]["type"][sel].copy(), gid=ranks[0]["gid"][sel].copy()))
        vs.append(v[sel].copy())
    return ff, lat2, out, vs


# `run` and its constants belong to ONE family of tests, the layouts of the 10 A streams (tests/test_gpu_streams_by_place.py and its poisoned child,
# tests/streams_place_worker.py): it sets and clears the environment switches of that comparison through the caller's monkeypatch.  It stands here
# with the builder it is used with, only because a test module may not be the library of a worker.
SWITCH = "RXMD_STREAMS_BY_PLACE"
PLACE_KW = dict(QEq_tol=1e-7, NMAXQEq=500, qeq_mode=1)      # (qeq_mode 1: the run-ahead CG loop in row order, the path of the benchmark)
CLEAN = (SWITCH, "RXMD_FORCE_STAGED", "RXMD_FORCE_REMOTE", "RXMD_NB10_ALWAYS", "RXMD_SPMV_WIN", "RXMD_NONBOND_WIN", "RXMD_QEQ_F32")


def perturbed_rdx(mc, scale=1.0, sigma=0.05):
    """the recipe of test_gpu_scale.py: RDX as geninit lays it out, every atom displaced by N(0, sigma A) per component (default_rng(2026)), wrapped
    into [0, 1), velocities N(0, 0.05); scale multiplies the three edges (the normalised coordinates stay) -> (ffield, lattice, rec10)"""
    ff, names, frac, lat = oa.make_system("rdx168")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff), mc=mc)
    lat2 = [lat2[0] * scale, lat2[1] * scale, lat2[2] * scale] + list(lat2[3:6])
    rng = np.random.default_rng(2026)
    r = ranks[0]
    n = len(r["type"])
    rn = r["rnorm"] + rng.normal(0, sigma, (n, 3)) / np.asarray(lat2[:3])
    rn = rn - np.floor(rn)
    return ff, lat2, rec10(dict(r, rnorm=rn), rng.normal(0, 0.05, (n, 3)))


def run(ff, lat, rec, place, monkeypatch, nsteps=3, env=(), bits=None, rccl=False, before=None, **kw):
    """QEq(); FORCE(); step(nsteps) on a fresh engine with the switch set -> what the layouts are compared on, behind FORCE (0) and behind the steps"""
    import rxmd_amd
    for k in CLEAN:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(SWITCH, str(place))
    for k, v in env:
        monkeypatch.setenv(k, v)
    e = rxmd_amd.RxmdEngine(ff, lat, **dict(PLACE_KW, **kw))
    if rccl:
        e.init_rccl(e.rccl_unique_id(), 0, 1)
    e.set_atoms_rxff(rec)
    if bits:
        e.set_qeq_precision(bits)
    out = {}
    if before:
        before(e, out)
    it0, _ = e.QEq(); e.FORCE(); a = e.atoms(); st = e.stats()
    out.update(it0=it0, est0=e.debug(13).copy(), q0=a["q"].copy(), f0=a["f"].copy(), rows0=e.debug(7).copy(), layout0=st["streams_by_place"], stats0=st,
               tap14=e.debug(14, cap=2).copy())      # (1 if the poison pattern is on, an element of the value stream that no kernel writes)
    e.step(nsteps)
    a = e.atoms(); st = e.stats()
    out.update(est=e.debug(13).copy(), q=a["q"].copy(), f=a["f"].copy(), pos=a["pos"].copy(), gid=a["gid"].copy(), rows=e.debug(7).copy(), iters=st["qeq_iters_total"],
               layout=st["streams_by_place"], stats=st, stride=st["n10_stride"])
    e.close()
    return out


def slab_system():
    """RDX-168 squeezed into the lower 44 % of a box 1/0.35 times as long in x: at vprocs 2x1x1 rank 1 owns NO atom"""
    ff, names, frac, lat = oa.make_system("rdx168")
    frac2 = frac.copy(); frac2[:, 0] = frac2[:, 0] * 0.35
    lat2 = list(lat); lat2[0] = lat[0] / 0.35
    return ff, names, frac2, lat2


def mode_velocities(gid, seed, sigma, ntotal):
    """seeded velocities that depend only on the GLOBAL atom id (the same atom gets the same draw on every decomposition)"""
    v = np.random.default_rng(seed).normal(0.0, sigma, (ntotal + 1, 3))
    return v[gid]


def build_system(spec):
    """spec: dict(case, mc, vp, slab, shaken=(seed, sigma in A), v=(seed, sigma, natoms of the whole system)) -> (ffield, lattice of the whole
    box, per-rank dict(rnorm, type, gid) as rxff.bin would hold them, per-rank velocities or None)"""
    vp = tuple(spec["vp"]); mc = tuple(spec.get("mc", (1, 1, 1)))
    if spec.get("slab"):
        ff, names, frac, lat = slab_system()
    else:
        ff, names, frac, lat = oa.make_system(spec["case"])
    ffn = oa.ffield_names(ff)
    if not spec.get("shaken"):
        lat2, ranks = oa.geninit(names, frac, lat, ffn, mc=mc, vprocs=vp)
    else:
        # _perturbed_rdx at another size and seed: the lattice positions displaced by N(0, sigma) per component, back into [0, 1)
        # as geninit and every migration leave them, then dealt to the domains of the rank grid the way geninit does (geninit.F90:493-527)
        seed, sigma = spec["shaken"]
        lat2, one = oa.geninit(names, frac, lat, ffn, mc=mc)
        assert tuple(lat2[3:6]) == (90.0, 90.0, 90.0)
        n = len(one[0]["type"])
        rn = one[0]["rnorm"] + np.random.default_rng(seed).normal(0, sigma, (n, 3)) / np.asarray(lat2[:3], dtype=np.float64)
        rn = rn - np.floor(rn)
        v3 = np.array(vp)
        dom = (rn * v3).astype(np.int64)
        sid = dom[:, 0] + dom[:, 1] * v3[0] + dom[:, 2] * v3[0] * v3[1]
        ranks = []
        for p in range(int(v3.prod())):
            sel = np.nonzero(sid == p)[0]
            obox = (1.0 / v3) * np.array([p % v3[0], (p // v3[0]) % v3[1], p // (v3[0] * v3[1])])
            ranks.append(dict(rnorm=rn[sel] - obox, type=one[0]["type"][sel].copy(), gid=one[0]["gid"][sel].copy()))
    vs = [mode_velocities(r["gid"], *spec["v"]) for r in ranks] if spec.get("v") else None
    return ff, [float(x) for x in lat2], ranks, vs
