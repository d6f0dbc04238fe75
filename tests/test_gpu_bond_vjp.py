"""rxmd_hip_bonds_vjp_device and its mirrors (RxmdEngine.bonds_vjp_device, torch_front.ReaxFF.bond_orders): the gradient of any function of the
bond-order graph with respect to the positions.

Engines run with isQEq = 0 wherever charges are not what a test is about: bond orders do not depend on them.

The finite-difference tests share one loss, L = sum_e w(gid_src, gid_dst) bo_e [+ sum_k w_k(..) parts_ek + sum_c u_c(..) vec_ec], with fixed
pseudo-random weights in [-1, 1) keyed by the global ids of an edge's ends, so the order of the edges does not matter.  L is summed exactly
(math.fsum): the terms that a displacement does not reach are bit-equal at +h and -h and cancel.

Bound of every finite-difference case, as the issue of this feature sets it:
    max |vjp - fd(h/2)|  <=  max |fd(h) - fd(h/2)|  +  1e-9 max|g|          h = 1e-4 A, 4 atoms x 3 components
The first term is three times the truncation error of fd(h/2) for an exact gradient (central differences: error ~ h^2), the second covers the
round-off of L / h (a few 1e-11 of max|g| on these systems).  Every case prints its bound next to what it measured, and asserts that the set of
selected (gid, gid) edges is the same at +h and -h: an edge that enters or leaves a list is a jump of L, not a slope.

The ice unit cell: the issue asks for a unit cell in which an atom bonds to its OWN image.  No such box exists for the engine: it refuses a box
edge below the largest bond cut-off (RXMD_E_ARG, "local box smaller than the bond cutoff"; engine.hip, geometry_for), and a bond with one's own
image is as long as a box edge.  The oracle finds none in the ice unit cell either (4.754 x 8.234 x 7.346 A against a largest bond cut-off of 2.6 A:
80 directed bonds, none of an atom with itself).  The engine accepts that cell, so it is the case, without the self-bond: 24 residents among 27
images of each; 20 of its 80 directed bonds reach a periodic image, whose share is folded back onto the resident.  It runs last in the file.
"""
import math

import numpy as np
import pytest
import torch

import oracle_api as oa
import offlattice_systems as ol
from parity import _engine, code as _code
from graph_support import _device_coo, _offlattice_engine

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = 1e-4
SENT = -777.25
NOQ = dict(isQEq=0)


# ---- weights keyed by global ids ---------------------------------------------------------------------------------------------------------
def _w(gs, gd, salt):
    """a fixed number in [-1, 1) per (gid, gid, salt): splitmix-style mixing of the three"""
    with np.errstate(over="ignore"):
        x = gs.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) ^ gd.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F) ^ np.uint64((salt + 1) * 0x165667B19E3779F9 % 2 ** 64)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0


def _weights(s, d, full):
    """(w [E], wparts [E, 3] or None, u [E, 3] or None) for edges with global ids s -> d"""
    w = _w(s, d, 0)
    if not full:
        return w, None, None
    return w, np.stack([_w(s, d, 1 + k) for k in range(3)], 1), np.stack([_w(s, d, 4 + k) for k in range(3)], 1)


def _loss(s, d, bo, parts, vec, full):
    w, wp, u = _weights(s, d, full)
    terms = [w * bo]
    if full:
        terms += [(wp * parts).ravel(), (u * vec).ravel()]
    return math.fsum(np.concatenate(terms).tolist())


def _edge_set(s, d):
    k = np.lexsort((d, s))
    return np.stack([s[k], d[k]], 1)


def _dev(a, dt=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV)


def _vjp(e, bo_min=0.0, full=True, as_gid=True):
    """the VJP of the loss above on the engine's current state -> grad [natoms, 3] (numpy)"""
    E, s, d, bo, parts, vec = _device_coo(e, bo_min=bo_min, as_gid=True)
    w, wp, u = _weights(s, d, full)
    tw = _dev(w); twp = _dev(wp) if full else None; tu = _dev(u) if full else None
    g = torch.full((e.natoms, 3), SENT, dtype=torch.float64, device=DEV)
    e.bonds_vjp_device(E, g.data_ptr(), grad_bo_ptr=tw.data_ptr(), grad_bo3_ptr=twp.data_ptr() if full else 0, grad_vec_ptr=tu.data_ptr() if full else 0,
                       bo_min=bo_min, as_gid=as_gid, stream=torch.cuda.current_stream().cuda_stream)
    return g.cpu().numpy()


class _Forward:
    """the existing forward path on device arrays: evaluate_device + bonds_device of one engine, atoms in the order and with the ids of atoms()"""

    def __init__(self, e):
        a = e.atoms()
        self.e, self.n, self.pos0, self.gid = e, len(a["gid"]), a["pos"].copy(), a["gid"].copy()
        self.ttype, self.tgid = _dev(a["type"], torch.int32), _dev(a["gid"], torch.int64)
        self.f = torch.empty((self.n, 3), dtype=torch.float64, device=DEV); self.q = torch.empty(self.n, dtype=torch.float64, device=DEV)

    def __call__(self, pos, bo_min=0.0):
        tpos = _dev(pos)
        self.e.evaluate_device(self.n, self.ttype.data_ptr(), tpos.data_ptr(), self.f.data_ptr(), self.q.data_ptr(), gid_ptr=self.tgid.data_ptr(),
                               stream=torch.cuda.current_stream().cuda_stream)
        return _device_coo(self.e, bo_min=bo_min, as_gid=True)[1:]


def _fd_check(label, loss_at, pos0, atoms, g, gmax):
    """central differences of loss_at(pos) -> (L, edge set) at h and h / 2 for the three components of `atoms`, against the rows of g"""
    fd = {}
    for h in (H, H / 2):
        out = np.zeros((len(atoms), 3))
        for a, i in enumerate(atoms):
            for c in range(3):
                p = pos0.copy(); p[i, c] += h
                Lp, ep = loss_at(p)
                p = pos0.copy(); p[i, c] -= h
                Lm, em = loss_at(p)
                assert np.array_equal(ep, em), "%s: the selected edges differ between +h and -h (atom %d, component %d, h %g)" % (label, i, c, h)
                out[a, c] = (Lp - Lm) / (2 * h)
        fd[h] = out
    err = np.abs(g[atoms] - fd[H / 2]).max()
    trunc = np.abs(fd[H] - fd[H / 2]).max()
    bound = trunc + 1e-9 * gmax
    print("%s: atoms %s  max|g| %.6e  max|vjp - fd(h/2)| %.3e  bound %.3e (= max|fd(h) - fd(h/2)| %.3e + 1e-9 max|g|)  ratio err/trunc %.3f"
          % (label, list(atoms), gmax, err, bound, trunc, err / max(trunc, 1e-300)))
    assert gmax > 0.0 and np.isfinite(g).all()
    assert err <= bound, (label, err, bound)


def _four_atoms(n, must=None):
    atoms = [0, n // 3, (2 * n) // 3, n - 1]
    if must is not None and must not in atoms:
        atoms[1] = must
    return atoms


# ---- 1. against the reference --------------------------------------------------------------------------------------------------------------
def test_against_central_differences_of_the_oracle():
    e = _engine("rdx168", (1, 1, 1), **NOQ); e.FORCE()
    g = _vjp(e, full=False)
    a = e.atoms()
    ff, names, frac, lat = oa.make_system("rdx168")
    lat2, ranks = oa.geninit(names, frac, lat, oa.ffield_names(ff))
    o = oa.Oracle(ff, lat2, ranks, isQEq=0)
    assert np.array_equal(o.gids(), a["gid"])

    def loss_at(pos):
        o.set_pos(pos); o.force()
        n = len(pos)
        gid = o.get(106).astype(np.int64)
        nbr, bo = o.bonds()
        m = nbr[:n] > 0
        s, d = np.repeat(gid[:n], m.sum(1)), gid[nbr[:n][m] - 1]
        return _loss(s, d, bo[:n][m], None, None, False), _edge_set(s, d)

    _fd_check("oracle, rdx168", loss_at, a["pos"].copy(), _four_atoms(len(a["gid"])), g, np.abs(g).max())
    e.close()


# ---- 2. against the engine's forward path ------------------------------------------------------------------------------------------------------
def _forward_case(case):
    if case in ("rdx168", "rdx168-bo-only", "rdx168-0.3"):
        e = _engine("rdx168", (1, 1, 1), **NOQ)
    elif case == "mos2_tri324":
        e = _engine("mos2_tri324", (3, 3, 2), **NOQ)
    elif case == "ice111":
        e = _engine("ice", (1, 1, 1), **NOQ)
    elif case == "ice333":
        e = _engine("ice", (3, 3, 3), **NOQ)
    else:
        e = _offlattice_engine(case, **NOQ)
    return e


def _run_forward_case(case):
    e = _forward_case(case)
    fw = _Forward(e)
    bo_min = 0.3 if case == "rdx168-0.3" else 0.0
    full = case != "rdx168-bo-only"
    s, d, bo, parts, vec = fw(fw.pos0, bo_min)
    cnt = e.bonds()[0]
    must = None
    if case == "rdx-dilute":
        assert (cnt == 0).any()
        must = int(np.nonzero(cnt == 0)[0][0])                    # an atom without a bond: its row is empty, its gradient comes from nowhere
    if case == "rdx-denser":
        assert cnt.max() > 24 and (bo == 0.0).sum() > 0
    if case == "rdx168-0.3":
        assert 0 < len(bo) < e.bonds_device(0, 0, 0, 0)
    img = np.abs(vec - (fw.pos0[np.searchsorted(fw.gid, d)] - fw.pos0[np.searchsorted(fw.gid, s)])).max(1) > 1e-6 if np.all(np.diff(fw.gid) > 0) else None
    print(case, "natoms", fw.n, "edges", len(bo), "longest list", int(cnt.max()), "zero bond orders", int((bo == 0.0).sum()),
          "edges through a periodic image", "n/a" if img is None else int(img.sum()))
    g = _vjp(e, bo_min=bo_min, full=full)
    if must is not None:
        print(case, "gradient of the atom without a bond", g[must])

    def loss_at(pos):
        s, d, bo, parts, vec = fw(pos, bo_min)
        return _loss(s, d, bo, parts, vec, full), _edge_set(s, d)

    _fd_check(case, loss_at, fw.pos0, _four_atoms(fw.n, must), g, np.abs(g).max())
    e.close()


@pytest.mark.parametrize("case", ["rdx168", "rdx168-bo-only", "rdx168-0.3", "mos2_tri324", "rdx-denser", "rdx-dilute", "ice333"])
def test_against_central_differences_of_the_forward_path(case):
    _run_forward_case(case)


# ---- 3. translation invariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rdx168", "sicnp-pqeq", "rdx168-step3"])
def test_the_gradient_sums_to_zero(case):
    """|sum g| / sum |g| <= 10 x |sum f| / sum |f| of the same engine's forces: the same assembly with the same rounding; 10 x covers the different
    magnitudes of the terms"""
    if case == "sicnp-pqeq":
        e = _engine("sicnp", (1, 1, 1), pqeq=oa.PQEQ_SICNP)
    else:
        e = _engine("rdx168", (1, 1, 1))
    if case == "rdx168-step3":
        e.thermostat(0, 300.0)
    e.QEq(); e.FORCE()
    if case == "rdx168-step3":
        e.step(3)
    g = _vjp(e)
    f = e.atoms()["f"]
    rg = np.abs(g.sum(0)).max() / np.abs(g).sum()
    rf = np.abs(f.sum(0)).max() / np.abs(f).sum()
    print("%s: |sum g| / sum |g| %.3e   bound 10 x |sum f| / sum |f| = %.3e" % (case, rg, 10 * rf))
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    assert rg <= 10 * rf
    e.close()


# ---- 4. the engine is untouched ----------------------------------------------------------------------------------------------------------------
def _observables(e):
    """everything the entry points hand out, read twice over: atoms (positions, velocities, forces, charges), the rxff records, the energies, and the
    stress accumulators -- get_energy reads AND resets those, so a second read returns exactly what was added since: nothing"""
    a = e.atoms()
    en = e.energy()
    return dict(rec=e.get_atoms_rxff().copy(), f=a["f"].copy(), pe=en["PE"].copy(), ke=en["KE"], qsum=en["qsum"], astr=en["astr"].copy())


def test_the_engine_is_untouched_and_the_call_repeats_its_bits():
    """Two engines run QEq, FORCE and three steps on the ice box (2304 atoms; no hydrogen-bond acceptor atomics there, so its forces are bit-equal from
    engine to engine: test_gpu_parity.test_forces_and_charges_are_bitwise_reproducible_run_to_run).  One of them calls the VJP after FORCE and between the
    steps; both make the same reads.
    Across the two engines, per step:
      * the rxff records (positions, velocities, charges, extended-Lagrangian state), the forces and the bond graph are bit-identical;
      * PE and astr agree at the bound the suite uses for sums that FORCE forms with global atomics (test_gpu_parity: rtol = atol-scale 1e-12).  Both are
        such sums: the 14 energies (atomicAdd(pe + k, ...) in every energy kernel), and the stress accumulators -- k_stress_partial / k_stress_final add
        the virial in a fixed order, but INTO accumulators that ENbond's pair virial (nonbonded.hip: atomicAdd(pe + 16 + c, s), one per workgroup) and
        the torsions' image terms (torsions.hip: atomicAdd(pe + 16.., t0 * F0)) have reached in scheduling order.  astr is compared relative to its
        largest component: the order-dependent error of such a sum scales with its terms, and all six components are sums of r_a f_b terms of one scale.
        Each figure is printed; where two engines happen to produce the same bits that is printed too.
    On ONE engine, where bits are a statement about the VJP: get_energy before and after the VJP calls returns the same PE, kinetic energy and charge
    sum, and stress accumulators that received nothing in between (exact zeros: get_energy resets them); atoms() and the records return the same bits."""
    runs = []
    for with_vjp in (False, True):
        e = _engine("ice644", (6, 4, 4)); e.QEq(); e.FORCE()
        if with_vjp:
            g1 = _vjp(e); g2 = _vjp(e)
            assert np.array_equal(g1, g2) and np.abs(g1).max() > 0
            g3 = _vjp(e, bo_min=0.3, full=False)
            assert np.array_equal(g3, _vjp(e, bo_min=0.3, full=False))
        steps = []
        for _ in range(3):
            e.step(1)
            before = _observables(e)
            assert np.abs(before["astr"]).max() > 0
            if with_vjp:
                _vjp(e); _vjp(e, bo_min=0.3, full=False)
            after = _observables(e)
            for k in ("rec", "f", "pe", "ke", "qsum"):
                assert np.array_equal(before[k], after[k]), k
            assert (after["astr"] == 0.0).all()
            steps.append(before)
        runs.append(dict(steps=steps, coo=_device_coo(e, as_gid=True)))
        e.close()
    a, b = runs
    for k, (x, y) in enumerate(zip(a["steps"], b["steps"])):
        scale = np.abs(x["astr"]).max()
        d_pe = (np.abs(x["pe"] - y["pe"]) / np.maximum(np.abs(x["pe"]), 1.0)).max()
        d_astr = np.abs(x["astr"] - y["astr"]).max() / scale
        print("step %d, engine without against engine with the VJP: PE max relative difference %.2e, astr max difference / largest component %.2e (bound 1e-12 each)%s"
              % (k + 1, d_pe, d_astr, "; both bit-equal" if d_pe == 0.0 and d_astr == 0.0 else ""))
        assert np.array_equal(x["rec"], y["rec"]) and np.array_equal(x["f"], y["f"]) and x["ke"] == y["ke"] and x["qsum"] == y["qsum"]
        assert np.allclose(x["pe"], y["pe"], rtol=1e-12, atol=1e-12)
        assert np.allclose(x["astr"], y["astr"], rtol=1e-12, atol=1e-12 * scale)
    assert a["coo"][0] == b["coo"][0] and all(np.array_equal(x, y) for x, y in zip(a["coo"][1:], b["coo"][1:]))


def test_the_bond_tables_still_hold_the_last_force_under_poisoned_scratch(monkeypatch):
    """RXMD_POISON_ALLOC=1: every buffer starts as NaN / -1 and the per-step scratch is refilled before every rebuild.  The VJP reads A0..A3, dBOp and
    dln* of the last FORCE and its own scratch: a finite gradient, equal to the one of a plain engine bit for bit (the ice box: its trajectory is
    bit-equal from engine to engine)"""
    e = _engine("ice644", (6, 4, 4)); e.QEq(); e.FORCE(); e.step(2)
    ref = _vjp(e); e.close()
    monkeypatch.setenv("RXMD_POISON_ALLOC", "1")
    e = _engine("ice644", (6, 4, 4)); e.QEq(); e.FORCE(); e.step(2)
    g = _vjp(e); e.close()
    assert np.isfinite(g).all() and np.abs(g).max() > 0 and np.array_equal(g, ref)


# ---- 5. exchange forms -------------------------------------------------------------------------------------------------------------------------
_DEFAULT_FORM = {}


@pytest.mark.parametrize("env", [("RXMD_FORCE_STAGED",), ("RXMD_FORCE_STAGED", "RXMD_FORCE_REMOTE"), ("RXMD_NO_STAGE_PAIRS",)], ids="+".join)
def test_every_single_rank_exchange_form_folds_the_same_bits(env, monkeypatch):
    for k in ("RXMD_FORCE_STAGED", "RXMD_FORCE_REMOTE", "RXMD_NO_STAGE_PAIRS"):
        monkeypatch.delenv(k, raising=False)
    if not _DEFAULT_FORM:
        e = _engine("rdx168", (1, 1, 1), **NOQ); e.FORCE()
        _DEFAULT_FORM["g"] = _vjp(e); e.close()
    for k in env:
        monkeypatch.setenv(k, "1")                 # (options are read when the engine is created)
    e = _engine("rdx168", (1, 1, 1), **NOQ)
    if "RXMD_FORCE_REMOTE" in env:
        e.init_rccl(e.rccl_unique_id(), 0, 1)
    e.FORCE()
    g = _vjp(e); e.close()
    assert np.abs(g).max() > 0 and np.array_equal(g, _DEFAULT_FORM["g"])


# ---- 6. growth of the bond tables --------------------------------------------------------------------------------------------------------------
def _dilute_then_dense():
    """rdx168 with every edge stretched by 1.5 (4,866 table entries, ghost rows included; the oracle's count), FORCE and a first VJP there; then the
    lattice as it was (21,894 entries), FORCE and a second VJP -> (entries at either lattice, both gradients)"""
    e = _engine("rdx168", (1, 1, 1), **NOQ)
    lat = list(e.lattice)
    e.set_lattice([1.5 * lat[0], 1.5 * lat[1], 1.5 * lat[2]] + lat[3:])
    e.FORCE()
    n0 = e.stats()["nbonds"]
    g0 = _vjp(e)
    e.set_lattice(lat)
    e.FORCE()
    n1 = e.stats()["nbonds"]
    g1 = _vjp(e)
    e.close()
    return n0, n1, g0, g1


def test_scratch_follows_the_growth_of_the_bond_tables(monkeypatch):
    """RXMD_BOND_CAP=8192 holds the tables of the stretched box and not those of the box as it was: the first VJP allocates its scratch at the small
    capacity, the second finds the tables grown and allocates again.  Both gradients equal those of an engine whose tables never grow, bit for bit"""
    monkeypatch.delenv("RXMD_BOND_CAP", raising=False)
    n0, n1, ref0, ref1 = _dilute_then_dense()
    monkeypatch.setenv("RXMD_BOND_CAP", "8192")
    m0, m1, g0, g1 = _dilute_then_dense()
    print("table entries: stretched box %d, box as it was %d, capacity at the first VJP call 8192" % (m0, m1))
    assert (m0, m1) == (n0, n1) and m0 <= 8192 < m1
    assert np.abs(g0).max() > 0 and np.abs(g1).max() > 0
    assert np.array_equal(g0, ref0) and np.array_equal(g1, ref1)
    # tables that have grown before the first call (the form of test_gpu_bond_graph)
    e = _engine("rdx168", (1, 1, 1), **NOQ); e.FORCE()
    assert e.stats()["nbonds"] > 8192
    g = _vjp(e); e.close()
    assert np.abs(g).max() > 0 and np.isfinite(g).all()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import rxmd_amd
    e = _engine("rdx168", (1, 1, 1), **NOQ)
    n = e.natoms
    out = torch.full((n, 3), SENT, dtype=torch.float64, device=DEV)
    big = torch.ones(3 * 4096, dtype=torch.float64, device=DEV)
    o, b = out.data_ptr(), big.data_ptr()
    assert _code(lambda: e.bonds_vjp_device(8, o, grad_bo_ptr=b)) == -7                 # before the first FORCE
    e.FORCE()
    E = e.bonds_device(0, 0, 0, 0)
    assert 0 < E <= 4096
    for wrong in (E - 1, E + 1, 0):
        assert _code(lambda: e.bonds_vjp_device(wrong, o, grad_bo_ptr=b)) == -1         # not the count of this selection
    assert _code(lambda: e.bonds_vjp_device(E, o, grad_bo_ptr=b, bo_min=0.3)) == -1     # E of another threshold
    assert _code(lambda: e.bonds_vjp_device(E, 0, grad_bo_ptr=b)) == -1                 # no output
    assert _code(lambda: e.bonds_vjp_device(E, o)) == -1                                # no gradient at all
    assert _code(lambda: e.bonds_vjp_device(-1, o, grad_bo_ptr=b)) == -1
    assert _code(lambda: e.bonds_vjp_device(E, o, grad_bo_ptr=b, bo_min=float("nan"))) == -1
    raw = lambda flags: e._chk(e.L.rxmd_hip_bonds_vjp_device(e.h, flags, 0.0, E, b, None, None, o, None))
    assert _code(lambda: raw(2)) == -1 and _code(lambda: raw(3)) == -1                   # unknown flag bits
    torch.cuda.synchronize()
    assert (out == SENT).all()                                                          # nothing was written by any refused call
    e.bonds_vjp_device(E, o, grad_bo_ptr=b)
    e.bonds_vjp_device(E, o, grad_vec_ptr=b, as_gid=True)                               # each gradient alone is enough; the flag only names the selection
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == SENT).any()
    for stale in (lambda: e.set_lattice(e.lattice), lambda: e.set_charges(np.zeros(n))):
        stale()
        assert _code(lambda: e.bonds_vjp_device(E, o, grad_bo_ptr=b)) == -7             # the lists are stale
        e.FORCE()
        e.bonds_vjp_device(E, o, grad_bo_ptr=b)
    e.close()
    ff, names, frac, lat = oa.make_system("rdx168")
    e2 = rxmd_amd.RxmdEngine(ff, lat, vprocs=(2, 1, 1))
    assert _code(lambda: e2.bonds_vjp_device(8, o, grad_bo_ptr=b)) == -1                 # an argument error, raised before the state is looked at
    assert _code(lambda: e2.bonds_vjp_device(8, o, grad_bo_ptr=b, as_gid=True)) == -1
    e2.close()


# ---- 8. torch ----------------------------------------------------------------------------------------------------------------------------------
def _torch_model():
    from rxmd_amd.torch_front import ReaxFF
    e = _engine("rdx168", (1, 1, 1), **NOQ)
    a = e.atoms(); lat = list(e.lattice); e.close()
    ff = oa.make_system("rdx168")[0]
    rng = np.random.default_rng(20250311)
    perm = rng.permutation(len(a["gid"]))
    m = ReaxFF(ff, lat, a["type"][perm], gid=a["gid"][perm], **NOQ)
    return m, a["gid"][perm], a["pos"][perm]


def _torch_loss(out, gid, n):
    ei = out["edge_index"]
    s, d = gid[ei[0].cpu().numpy()], gid[ei[1].cpu().numpy()]
    w, wp, u = _weights(s, d, True)
    cn = torch.zeros(n, dtype=torch.float64, device=DEV).index_add(0, ei[0], out["bond_order"])
    L = 0.5 * out["energy"] + (_dev(w) * out["bond_order"]).sum() + (_dev(u) * out["edge_vec"]).sum() + (cn[0] - 3.0) ** 2
    g_bo = w + 2.0 * (cn[0].item() - 3.0) * (ei[0].cpu().numpy() == 0)
    return L, g_bo, u


def test_torch_backward_is_minus_forces_plus_the_vjp():
    m, gid, pos = _torch_model()
    n = len(gid)
    tpos = _dev(pos).requires_grad_(True)
    out = m.bond_orders(tpos, bo_min=0.3)
    assert set(out) == {"energy", "edge_index", "bond_order", "edge_vec", "forces", "charges"}
    assert out["bond_order"].requires_grad and out["edge_vec"].requires_grad and out["energy"].requires_grad
    assert not out["edge_index"].requires_grad and not out["forces"].requires_grad and not out["charges"].requires_grad
    L, g_bo, u = _torch_loss(out, gid, n)
    L.backward()
    E = out["bond_order"].shape[0]
    gp = torch.full((n, 3), SENT, dtype=torch.float64, device=DEV)
    tg, tu = _dev(g_bo), _dev(u)
    m.engine.bonds_vjp_device(E, gp.data_ptr(), grad_bo_ptr=tg.data_ptr(), grad_vec_ptr=tu.data_ptr(), bo_min=0.3, stream=torch.cuda.current_stream().cuda_stream)
    want = -0.5 * out["forces"] + gp
    err = (tpos.grad - want).abs().max().item()
    print("torch: max|pos.grad - (-0.5 f + vjp)| %.3e of max %.3e" % (err, want.abs().max().item()))
    assert torch.equal(tpos.grad, want)
    # the graph is the one bond_graph returns, and bond_graph still hands out constants
    g = m.bond_graph(bo_min=0.3)
    assert all(not t.requires_grad for t in g.values())
    for k in ("edge_index", "bond_order", "edge_vec"):
        assert torch.equal(g[k], out[k].detach())
    # components, a loss that uses the parts alone: the other gradients arrive as None
    tpos2 = _dev(pos).requires_grad_(True)
    out2 = m.bond_orders(tpos2, components=True)
    assert out2["bond_order_parts"].shape == (out2["bond_order"].shape[0], 3)
    assert ((out2["bond_order_parts"].sum(1) - out2["bond_order"]).abs() <= 4 * np.finfo(np.float64).eps * out2["bond_order"]).all()   # (the bound of test_gpu_bond_graph)
    out2["bond_order_parts"][:, 1].sum().backward()
    assert torch.isfinite(tpos2.grad).all() and tpos2.grad.abs().max() > 0
    m.close()


def test_torch_non_contiguous_positions_and_a_side_stream():
    m, gid, pos = _torch_model()
    n = len(gid)
    tpos = _dev(pos).requires_grad_(True)
    L, _, _ = _torch_loss(m.bond_orders(tpos, bo_min=0.3), gid, n)
    L.backward()
    wide = torch.zeros((n, 6), dtype=torch.float64, device=DEV)
    wide[:, ::2] = _dev(pos)
    wide.requires_grad_(True)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    L2, _, _ = _torch_loss(m.bond_orders(view, bo_min=0.3), gid, n)
    L2.backward()
    assert torch.equal(wide.grad[:, ::2], tpos.grad) and (wide.grad[:, 1::2] == 0).all()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.randn(2048, 2048, device=DEV) @ torch.randn(2048, 2048, device=DEV)   # work in front of the producer on this stream
        p = (_dev(pos) + 0.0 * big[0, 0].double()).requires_grad_(True)
        L3, _, _ = _torch_loss(m.bond_orders(p, bo_min=0.3), gid, n)
        L3.backward()
        side = p.grad * 1
    s.synchronize()
    assert torch.equal(side, tpos.grad)            # (not L itself: it holds the energy, which FORCE sums with global atomics)
    m.close()


def test_torch_backward_after_another_evaluation_raises():
    m, gid, pos = _torch_model()
    for later in (lambda p: m.evaluate(p), lambda p: m.energy(p), lambda p: m.bond_orders(p), lambda p: m.set_lattice(m.engine.lattice)):
        tpos = _dev(pos).requires_grad_(True)
        out = m.bond_orders(tpos)
        later(_dev(pos))
        with pytest.raises(RuntimeError, match="before the next evaluation"):
            out["bond_order"].sum().backward()
    tpos = _dev(pos).requires_grad_(True)
    m.bond_orders(tpos)["bond_order"].sum().backward()             # in order: fine
    assert torch.isfinite(tpos.grad).all()
    m.close()


# ---- the ice unit cell (last: the one box of this file that no other test of the suite builds) ----------------------------------------------------
def test_against_central_differences_of_the_forward_path_ice_unit_cell():
    _run_forward_case("ice111")
