"""rxmd_hip_evaluate_device and its torch front end (rxmd_amd.torch_front.ReaxFF): QEq + FORCE on tensors that live on the device.

Held to the oracle at the project's tolerances (QTOL, FTOL, ETOL of test_gpu_parity; 1e-8 for the virial, 1e-7 for forces from injected
charges -- the bounds of the existing tests that make the same comparison through host arrays) and to the array-shaped entry points, which run
the same kernels.  The oracle runs once per system (tight tolerance) and its results are shared, unmodified, by the tests below.

No finite-difference test: central differences of pe[0] against -f.d do not converge on these boxes because the charge solve is not smooth
at that scale ("Ill-conditioned charge problems").
"""
import numpy as np
import pytest
import torch

import oracle_api as oa
from npt_reference import hmat
from parity import _engine, q_err, f_err, e_err, QTOL, FTOL, ETOL
from graph_support import _ref, _model, _dev, TIGHT, DEV, EPS

pytestmark = pytest.mark.gpu


def _arrays_run(r, pos, natoms=None, typ=None, gid=None, **kw):
    """the existing path through host arrays on a fresh engine: QEq_arrays + FORCE_arrays -> (q, f, pe)"""
    import rxmd_amd
    n = natoms or len(pos)
    typ = r["type"] if typ is None else typ
    gid = r["gid"] if gid is None else gid
    e = rxmd_amd.RxmdEngine(r["ff"], r["lat"], **kw)
    atype = np.ascontiguousarray(typ[:n] + gid[:n] * 1e-13); p = np.asfortranarray(pos[:n]); q = np.zeros(n)
    e.QEq_arrays(atype, p, q, n)
    f, pe = e.FORCE_arrays(atype, p, q, n)
    e.close()
    return q.copy(), np.ascontiguousarray(f), pe


# ---- 1. parity against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mc", [("rdx168", (1, 1, 1)), ("ice644", (6, 4, 4)), ("mos2_tri324", (3, 3, 2))])
def test_parity_against_the_oracle(case, mc):
    r = _ref(case, mc)
    m = _model(r, **TIGHT)
    pos = _dev(r["pos"])
    out = m.evaluate(pos)
    q, f, pe, vir = out["charges"].cpu().numpy(), out["forces"].cpu().numpy(), out["pe"].numpy(), out["virial"].numpy()
    figs = dict(q=q_err(q, r["q"]), f=f_err(f, r["f"]), e=e_err(pe, r["pe"]), virial=np.abs(vir - r["astr"]).max() / np.abs(r["astr"]).max())
    print(case, figs)
    assert figs["q"] <= QTOL and figs["f"] <= FTOL and figs["e"] <= ETOL
    assert figs["virial"] <= 1e-8
    assert out["energy"].dim() == 0 and out["energy"].dtype == torch.float64 and out["energy"].is_cuda and out["energy"].item() == pe[0]
    assert out["forces"].shape == (len(q), 3) and out["charges"].shape == (len(q),) and not out["pe"].is_cuda and not out["virial"].is_cuda
    # atoms inside the box keep their coordinates bit for bit, in the caller's order; the accumulators of energy() hold what a plain FORCE leaves
    assert np.array_equal(m.engine.debug(3, 3)[:len(q)], r["pos"])
    assert np.array_equal(pos.cpu().numpy(), r["pos"])
    assert np.array_equal(m.engine.energy()["astr"], vir)
    m.close()


# ---- 2. same kernels, same answer ------------------------------------------------------------------------------------------------------
def test_same_answer_as_the_array_entry_points():
    """Run-to-run noise of the existing path, measured here: two fresh engines through QEq_arrays + FORCE_arrays on the same atoms (the H-bond
    acceptor forces and the 14 energies take global atomics, test_forces_and_charges_are_bitwise_reproducible_run_to_run).  The device path must
    agree with the second of them to 100 x that floor and never worse than the project tolerances.  A measured floor of exactly zero says the
    noise is below what a double resolves, so the floor is taken as at least one ulp (2.2e-16 in these relative metrics)."""
    r = _ref("rdx168", (1, 1, 1))
    q1, f1, pe1 = _arrays_run(r, r["pos"], **TIGHT)
    q2, f2, pe2 = _arrays_run(r, r["pos"], **TIGHT)
    floor = dict(q=max(q_err(q1, q2), EPS), f=max(f_err(f1, f2), EPS), e=max(e_err(pe1, pe2), EPS))
    print("run-to-run floor of the array path:", floor)
    m = _model(r, **TIGHT)
    out = m.evaluate(_dev(r["pos"]))
    figs = dict(q=q_err(out["charges"].cpu().numpy(), q2), f=f_err(out["forces"].cpu().numpy(), f2), e=e_err(out["pe"].numpy(), pe2))
    print("device path against the array path:", figs)
    assert figs["q"] <= min(100 * floor["q"], QTOL)
    assert figs["f"] <= min(100 * floor["f"], FTOL)
    assert figs["e"] <= min(100 * floor["e"], ETOL)
    m.close()


# ---- 3. images -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mc", [("rdx168", (1, 1, 1)), ("mos2_tri324", (3, 3, 2))])
def test_atoms_anywhere_in_space_are_wrapped_into_the_box(case, mc):
    r = _ref(case, mc)
    n = len(r["pos"])
    rng = np.random.default_rng(20240611)
    shift = rng.integers(-3, 4, size=(n, 3)).astype(np.float64) @ hmat(r["lat"]).T          # row i: n1 a1 + n2 a2 + n3 a3
    assert np.abs(shift).max() > 0.0
    pin = r["pos"] + shift
    m = _model(r, isQEq=0)
    pos = _dev(pin)
    out = m.evaluate(pos, q0=_dev(r["q"]))
    wrapped = m.engine.debug(3, 3)[:n]
    figs = dict(f=f_err(out["forces"].cpu().numpy(), r["f"]), e=e_err(out["pe"].numpy(), r["pe"]), dr=np.abs(wrapped - r["pos"]).max(),
                dr_bound=64 * EPS * np.abs(pin).max())
    print(case, figs)
    assert figs["f"] <= 1e-7 and figs["e"] <= ETOL                  # the bounds of test_injected_oracle_charges_isolate_force_kernels
    assert figs["dr"] <= figs["dr_bound"]
    assert np.array_equal(pos.cpu().numpy(), pin)                   # the caller's tensor is never written
    assert np.array_equal(out["charges"].cpu().numpy(), r["q"])     # isQEq = 0: the charges handed in are the charges used
    m.close()


# ---- 4. box faces ----------------------------------------------------------------------------------------------------------------------
def test_atoms_on_the_box_faces():
    r = _ref("rdx168", (1, 1, 1))
    a = r["lat"][0]
    ix = np.argsort(r["pos"][:, 0]); iy = np.argsort(r["pos"][:, 1])
    i0, i1 = int(ix[0]), int(ix[-1])                                # the atoms nearest to the two x faces, and the lowest in y that is neither
    i2 = int([i for i in iy if i not in (i0, i1)][0])
    on, ref = r["pos"].copy(), r["pos"].copy()
    on[i0, 0] = -1e-18; on[i1, 0] = a; on[i2, 1] = 0.0
    ref[i0, 0] = 0.0; ref[i1, 0] = 0.0; ref[i2, 1] = 0.0
    m = _model(r, isQEq=0)
    q0 = _dev(r["q"])
    f_on = m.evaluate(_dev(on), q0=q0)["forces"].cpu().numpy()
    w = m.engine.debug(3, 3)[:len(on)]
    f_ref = m.evaluate(_dev(ref), q0=q0)["forces"].cpu().numpy()
    print("faces: f_err", f_err(f_on, f_ref), "wrapped x of the atom at -1e-18:", w[i0, 0], "of the atom at a:", w[i1, 0], "y of the atom at 0:", w[i2, 1])
    assert w[i0, 0] == a                                            # -1e-18 wraps to exactly one box length
    assert f_err(f_on, f_ref) <= 1e-7
    m.close()


# ---- 5. a trajectory through repeated calls --------------------------------------------------------------------------------------------
def test_trajectory_through_repeated_calls_and_a_changing_atom_count():
    r = _ref("rdx168", (1, 1, 1))
    H = hmat(r["lat"])
    rng = np.random.default_rng(7)
    A = _engine("rdx168", (1, 1, 1), **TIGHT)
    A.thermostat(0, 300.0); A.QEq(); A.FORCE()
    q_prev = A.atoms()["q"].copy()
    m = _model(r, **TIGHT)
    for step in range(6):
        A.step(1)
        a = A.atoms()
        n = len(a["gid"])
        m.set_atoms(a["type"], a["gid"])                            # A's order (migration may have changed it)
        pin = a["pos"] + rng.integers(-3, 4, size=(n, 3)).astype(np.float64) @ H.T
        out = m.evaluate(_dev(pin), q0=_dev(q_prev) if step == 0 else None)
        figs = (q_err(out["charges"].cpu().numpy(), a["q"]), f_err(out["forces"].cpu().numpy(), a["f"]))
        print("step", step + 1, "q_err %.2e f_err %.2e" % figs)
        assert figs[0] <= QTOL and figs[1] <= FTOL
        if step == 2:                                               # natoms changes once: without the last 8 atoms, then with them again
            for k in (n - 8, n):
                m.set_atoms(a["type"][:k], a["gid"][:k])
                out = m.evaluate(_dev(pin[:k]))
                qf, ff, _ = _arrays_run(r, a["pos"], natoms=k, typ=a["type"], gid=a["gid"], **TIGHT)
                figs = (q_err(out["charges"].cpu().numpy(), qf), f_err(out["forces"].cpu().numpy(), ff))
                print("  natoms", k, "q_err %.2e f_err %.2e against a fresh engine" % figs)
                assert figs[0] <= QTOL and figs[1] <= FTOL
    A.close(); m.close()


# ---- 6. autograd -----------------------------------------------------------------------------------------------------------------------
def _ice_model():
    """ice (no hydrogen-bond term in this force field file: forces are bitwise reproducible), fixed charges by type so that every call is the same function"""
    r = _ref("ice644", (6, 4, 4))
    m = _model(r, isQEq=0)
    q0 = _dev(r["q"])
    f0 = m.evaluate(_dev(r["pos"]), q0=q0)["forces"]               # later calls with q0 = None keep these charges
    return r, m, q0, f0


def test_autograd_gives_minus_the_forces():
    r, m, q0, f0 = _ice_model()
    pos = _dev(r["pos"]).requires_grad_(True)
    e = m(pos)
    assert e.dim() == 0 and e.requires_grad
    (g,) = torch.autograd.grad(e, pos)
    assert torch.equal(g, -f0)
    pos.grad = None
    (2.5 * m(pos)).backward()
    assert torch.equal(pos.grad, -2.5 * f0)
    # a second derivative is refused
    e = m(pos)
    (g,) = torch.autograd.grad(e, pos, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), pos)
    m.close()


def test_non_contiguous_positions():
    r, m, q0, f0 = _ice_model()
    n = len(r["pos"])
    wide = torch.zeros((n, 6), dtype=torch.float64, device=DEV)
    wide[:, ::2] = _dev(r["pos"])
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert torch.equal(m.evaluate(view)["forces"], f0)
    leaf = _dev(r["pos"]).t().contiguous().t().requires_grad_(True)      # [n, 3] with strides (1, n)
    assert not leaf.is_contiguous()
    m.energy(leaf).backward()
    assert leaf.grad.shape == leaf.shape and torch.equal(leaf.grad, -f0)
    m.close()


def test_inputs_and_outputs_on_a_side_stream():
    r, m, q0, f0 = _ice_model()
    base = _dev(r["pos"])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.randn(2048, 2048, device=DEV) @ torch.randn(2048, 2048, device=DEV)   # work in front of the producer on this stream
        p = base + 0.0 * big[0, 0].double()                                                # the input is produced on s ...
        out = m.evaluate(p)
        f_side = out["forces"] * 1.0                                                       # ... and the output consumed there
    s.synchronize()
    assert torch.isfinite(big).all()
    assert torch.equal(f_side, f0)
    m.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import rxmd_amd
    from rxmd_amd import system
    from rxmd_amd.torch_front import ReaxFF
    r = _ref("rdx168", (1, 1, 1))
    n = len(r["pos"])
    pos = _dev(r["pos"])
    for kw in (dict(isQEq=2), dict(vprocs=(2, 1, 1))):
        m = _model(r, **kw)
        with pytest.raises(rxmd_amd.RxmdError) as ei:
            m.evaluate(pos)
        assert ei.value.code == -1, kw
        m.close()
    ff, names, frac, lat = oa.make_system("sicnp")
    lat3, rec = system.geninit(ff, names, frac, lat)
    m = ReaxFF(ff, lat3, np.rint(rec[:, 7]).astype(np.int32), pqeq=oa.PQEQ_SICNP)
    with pytest.raises(rxmd_amd.RxmdError) as ei:
        m.evaluate(torch.zeros((len(rec), 3), dtype=torch.float64, device=DEV))
    assert ei.value.code == -1 and "pqeq" in str(ei.value).lower()
    m.close()
    # natoms above the capacity the first call sized the engine for
    m = _model(r, isQEq=0)
    m.evaluate(pos, q0=_dev(r["q"]))
    cap = m.engine.stats()["nbuffer"]
    k = cap // n + 1
    m.set_atoms(np.tile(r["type"], k))
    with pytest.raises(rxmd_amd.RxmdError) as ei:
        m.evaluate(pos.repeat(k, 1))
    assert ei.value.code == -3
    # a type outside the ffield: the code the array path gives for it, from the first call (sizing, on the host) and from a later one (device error word)
    bad = r["type"].copy(); bad[5] = 99
    with pytest.raises(rxmd_amd.RxmdError) as ea:
        _arrays_run(r, r["pos"], typ=bad, isQEq=0)
    m.set_atoms(bad, r["gid"])
    with pytest.raises(rxmd_amd.RxmdError) as ei:
        m.evaluate(pos)
    assert ei.value.code == ea.value.code == -1 and "type" in str(ei.value)
    m.close()
    m = ReaxFF(r["ff"], r["lat"], bad, isQEq=0)
    with pytest.raises(rxmd_amd.RxmdError) as ei:
        m.evaluate(pos)
    assert ei.value.code == ea.value.code
    m.close()
