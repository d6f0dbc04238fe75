"""The mixed-precision charge solver: rxmd_hip_set_qeq_precision(h, 32) / RXMD_QEQ_F32=1.

With 32 requested the 10 A sweep rounds every matrix value ONCE to REAL(4); the window pass of the CG streams those values as float (6 instead of
10 bytes per entry), the row pass and the row sums of the CG start vector read the same rounded values as double, and every product, sum, vector
and scalar stays double.  So the engine solves for the fixed point of the rounded matrix -- the fixtures tests/golden/*_f32matrix_tight.npz hold it,
computed by a scratch copy of the plain-C oracle with the same single rounding (tests/golden/make_f32_matrix_golden.py) -- and it does so through
every form of the pass.

Bounds.  Against the fixture: the project's own parity tolerances, unchanged.  Against the UNMODIFIED oracle: four times what the rounding was
measured to do on the CPU (q_err 5.4e-7, f_err 7.9e-6, worst energy term 2.5e-7 on RDX; smaller on ice); the total potential energy reacts in
second order (QEq is variational: 4e-11 measured, bound 1e-9).  All at QEq_tol 1e-12: at 1e-7 the CG exits by chance (tests/test_gpu_parity.py).
"""
import functools
import os
import numpy as np
import pytest

import oracle_api as oa
from parity import QTOL, FTOL, ETOL, q_err, f_err, e_err, _engine, _oracle

pytestmark = pytest.mark.gpu

KW = dict(QEq_tol=1e-12, NMAXQEq=2000)
CASES = [("rdx168", (1, 1, 1)), ("ice644", (6, 4, 4))]
RXMD_E_ARG = -1


def fixture(case):
    return np.load(os.path.join(oa.GOLD, "%s_f32matrix_tight.npz" % case))


@functools.lru_cache(maxsize=None)
def full_precision(case, mc):
    """the unmodified oracle at the tight tolerance, once per system: (gid, q, f, pe, row sums of the matrix)"""
    o = _oracle(case, mc, **KW); o.qeq(); o.force()
    out = (o.gids(), o.charges(), o.forces(), o.energy(), o.get(108))
    for a in out:
        a.setflags(write=False)
    return out


def engine32(case, mc, **kw):
    e = _engine(case, mc, **KW, **kw)
    assert e.qeq_precision() == (64, 64)
    e.set_qeq_precision(32)
    assert e.qeq_precision()[0] == 32
    return e


@pytest.mark.parametrize("qeq_mode", [0, 1])
@pytest.mark.parametrize("case,mc", CASES)
def test_fixed_point_of_the_rounded_matrix(case, mc, qeq_mode):
    g = fixture(case)
    e = engine32(case, mc, qeq_mode=qeq_mode)
    it, est = e.QEq(); pe = e.FORCE(); a = e.atoms()
    assert e.qeq_precision() == (32, 32)
    assert e.stats()["win_in_use"] == 1 and e.stats()["place_draws"] == 0
    assert (a["gid"] == g["gid"]).all()
    print("%s mode %d against the rounded-matrix fixture: q_err %.2e f_err %.2e e_err %.2e Est %.2e (%d iterations)" % (
        case, qeq_mode, q_err(a["q"], g["q"]), f_err(a["f"], g["f"]), e_err(pe, g["pe"]), abs(est - float(g["Est"])) / abs(est), it))
    assert q_err(a["q"], g["q"]) <= QTOL
    assert f_err(a["f"], g["f"]) <= FTOL
    assert e_err(pe, g["pe"]) <= ETOL
    assert abs(est - float(g["Est"])) <= 1e-9 * abs(est)
    e.close()


@pytest.mark.parametrize("case,mc", CASES)
def test_close_to_the_full_precision_solution(case, mc):
    gid, q, f, pref, rowsum = full_precision(case, mc)
    e = engine32(case, mc)
    e.QEq(); pe = e.FORCE(); a = e.atoms()
    assert e.qeq_precision() == (32, 32)
    assert (a["gid"] == gid).all()
    rs = e.debug(7)                                   # row sums of the double stream: the same rounded values the float stream holds
    drow = (np.abs(rs - rowsum) / np.abs(rowsum)).max()
    dpe = abs(pe[0] - pref[0]) / abs(pref[0])
    print("%s against the unmodified oracle: q_err %.2e f_err %.2e e_err %.2e total PE %.2e row sums %.2e" % (
        case, q_err(a["q"], q), f_err(a["f"], f), e_err(pe, pref), dpe, drow))
    assert q_err(a["q"], q) <= 2e-6
    assert f_err(a["f"], f) <= 3e-5
    assert e_err(pe, pref) <= 1e-6
    assert dpe <= 1e-9
    assert 1e-9 <= drow <= 1e-7                       # the mode is really on: ~430 roundings of 2^-24 per row (1e-8 emulated), and nothing coarser
    e.close()


def _same_operator(res):
    """Charges and Est as tightly as test_window_pass_and_row_pass_are_the_same_operator asks of two forms of the double pass (1e-7, 1e-9), its
    energy bound and its iteration-by-iteration comparison of the Est traces.  The forces are printed, not gated: where a run leaves its loop is
    decided by |Est / Est_prev - 1| < 1e-12 on the rounding of a row sum, and the forces amplify the charges' distance from the fixed point ~15-fold
    (RDX: q_err 5.4e-7 <-> f_err 7.9e-6 for the same perturbation).  Measured on RDX 2 x 2 x 2, qeq_mode 0: the row pass left after 73 iterations, the
    window pass after 92, first three Est values bit-identical, q_err 5.8e-8, f_err 1.08e-6; qeq_mode 1: 80 / 92 iterations, 1.5e-8, 1.5e-7."""
    ref = res[0]
    fig = []
    for r in res[1:]:
        tw, tr = ref["trace"], r["trace"]
        m = min(len(tw), len(tr))
        fig.append(dict(name=r["name"], q=q_err(r["q"], ref["q"]), f=f_err(r["f"], ref["f"]), e=e_err(r["pe"], ref["pe"]), est=abs(r["est"] - ref["est"]) / abs(ref["est"]), m=m, iters=(len(tw) - 1, len(tr) - 1),
                        trace=np.abs(tw[:m] - tr[:m]).max() / np.abs(tr[:m]).max(), first3=np.abs(tw[:3] - tr[:3]).max() / np.abs(tr[:3]).max()))
        print("%(name)s against the float window pass: q_err %(q).2e f_err %(f).2e e_err %(e).2e Est %(est).2e; Est traces over %(m)d iterations (%(iters)s) %(trace).2e, first three %(first3).2e" % fig[-1])
    for g in fig:
        assert g["q"] <= 1e-7, g
        assert g["est"] <= 1e-9, g
        assert g["e"] <= 1e-8, g
        assert g["m"] >= 10 and g["trace"] <= 5e-5, g
        assert g["first3"] <= 1e-10, g             # start vector and first two iterations: rounding of the row sums only


@pytest.mark.parametrize("qeq_mode", [0, 1])
def test_same_operator_on_every_path(qeq_mode, monkeypatch):
    """32 requested in every run (through the environment): the float window pass, the row pass on the rounded double stream (in_use 64) and the
    interior / boundary split of a staged single rank apply the same matrix -- the Est traces agree iteration by iteration."""
    monkeypatch.setenv("RXMD_QEQ_F32", "1")
    g = None
    res = []
    for env, in_use, win in ((None, 32, 1), ("RXMD_SPMV_WIN", 64, 0), ("RXMD_FORCE_STAGED", 32, 1)):
        if env:
            monkeypatch.setenv(env, "0" if env == "RXMD_SPMV_WIN" else "1")
        e = _engine("rdx222", (2, 2, 2), qeq_mode=qeq_mode, **KW)
        assert e.qeq_precision() == (32, 64)
        it, est = e.QEq(); pe = e.FORCE(); a = e.atoms()
        assert e.qeq_precision() == (32, in_use) and e.stats()["win_in_use"] == win, (env, e.qeq_precision(), e.stats()["win_in_use"])
        assert g is None or (a["gid"] == g).all()
        g = a["gid"]
        res.append(dict(name=env or "window", q=a["q"].copy(), f=a["f"].copy(), pe=pe, est=est, trace=e.debug(13, cap=4096).copy()))
        e.close()
        if env:
            monkeypatch.delenv(env)
    _same_operator(res)


def test_same_operator_extended_lagrangian(monkeypatch):
    """isQEq = 2 (one CG iteration per MD step, qeq_mode 1 prepass): five steps through the float window pass and through the row pass"""
    monkeypatch.setenv("RXMD_QEQ_F32", "1")
    res = []
    for win in ("1", "0"):
        monkeypatch.setenv("RXMD_SPMV_WIN", win)
        e = _engine("rdx222", (2, 2, 2), isQEq=2, qeq_mode=1)
        it, est = e.QEq(); e.FORCE(); e.step(5)
        a = e.atoms()
        assert e.qeq_precision() == (32, 32 if win == "1" else 64)
        res.append((a["q"].copy(), a["f"].copy(), a["pos"].copy(), est))
        e.close()
    assert q_err(res[0][0], res[1][0]) <= 1e-7 and f_err(res[0][1], res[1][1]) <= 5e-7
    assert np.abs(res[0][2] - res[1][2]).max() <= 1e-9
    assert abs(res[0][3] - res[1][3]) <= 1e-9 * abs(res[1][3])


def test_live_switch_on_one_engine():
    """64 -> 32 -> 64 on a live engine.  Every solve starts from the same charges (QEq starts its CG from the charges it finds, qeq.F90:41, so they are
    put back before each call): the 32 solve reaches the fixture, the second 64 solve repeats the first bit for bit, and both equal an engine on
    which the switch was never touched -- 64 is exactly the path as it was."""
    g = fixture("rdx168")
    e = _engine("rdx168", (1, 1, 1), **KW)
    q0 = e.atoms()["q"].copy()
    it64, est64 = e.QEq(); q64 = e.atoms()["q"].copy()
    assert e.qeq_precision() == (64, 64)
    e.set_qeq_precision(32); e.set_charges(q0)
    e.QEq(); q32 = e.atoms()["q"].copy()
    assert e.qeq_precision() == (32, 32)
    assert q_err(q32, g["q"]) <= QTOL and not np.array_equal(q32, q64)
    e.set_qeq_precision(64); e.set_charges(q0)
    it, est = e.QEq(); qb = e.atoms()["q"].copy(); pe = e.FORCE(); fb = e.atoms()["f"].copy()
    assert e.qeq_precision() == (64, 64)
    assert it == it64 and est == est64 and np.array_equal(qb, q64)
    e.close()
    u = _engine("rdx168", (1, 1, 1), **KW)            # the feature never touched
    itu, estu = u.QEq(); qu = u.atoms()["q"].copy(); peu = u.FORCE()
    assert itu == it64 and estu == est64 and np.array_equal(qu, q64)
    assert f_err(fb, u.atoms()["f"]) <= 1e-12 and e_err(pe, peu) <= 1e-12      # (the hydrogen-bond atomics add in arrival order: forces are not bitwise repeatable)
    u.close()


def test_trajectory_40_steps_from_rest():
    g = fixture("rdx168")
    e = engine32("rdx168", (1, 1, 1))
    e.QEq(); e.FORCE(); e.step(int(g["md_steps"]))
    a = e.atoms(); en = e.energy()
    etot = en["KE"] + en["PE"][0]
    assert e.qeq_precision() == (32, 32)
    assert (a["gid"] == g["md_gid"]).all()
    dx, dq, de = np.abs(a["pos"] - g["md_pos"]).max(), q_err(a["q"], g["md_q"]), abs(etot - float(g["md_Etot"]))
    print("40 steps against the rounded-matrix fixture: max|dx| %.2e A, q_err %.2e, |dE_tot| %.2e kcal/mol (KE %.3e)" % (dx, dq, de, en["KE"]))
    # the tolerances of test_md_trajectory_tight: positions 1e-9 A, charges QTOL; E_tot = KE + PE(0) within its 1e-7 of KE plus ETOL of PE(0)
    assert dx <= 1e-9
    assert dq <= QTOL
    assert de <= 1e-7 * abs(en["KE"]) + ETOL * abs(en["PE"][0])
    o = _oracle("rdx168", (1, 1, 1), **KW); o.qeq(); o.force(); o.step(int(g["md_steps"]))
    assert (a["gid"] == o.gids()).all()
    dxo, deo = np.abs(a["pos"] - o.pos()).max(), abs(etot - (o.kinetic() + o.energy()[0]))
    print("40 steps against the unmodified oracle: max|dx| %.2e A, |dE_tot| %.2e kcal/mol" % (dxo, deo))
    assert dxo <= 2e-8                                # 6 x the 3.4e-9 the rounding does on the CPU: room for chaotic growth
    assert deo <= 5e-6                                # 11 x the emulated 4.4e-7
    e.close()


def test_argument_errors(monkeypatch):
    import rxmd_amd
    e = _engine("rdx168", (1, 1, 1), **KW)
    with pytest.raises(rxmd_amd.engine.RxmdError) as ei:
        e.set_qeq_precision(16)
    assert ei.value.code == RXMD_E_ARG and e.qeq_precision() == (64, 64)
    e.close()
    p = _engine("sicnp", (1, 1, 1), pqeq=oa.PQEQ_SICNP, QEq_tol=1e-7, NMAXQEq=500)
    with pytest.raises(rxmd_amd.engine.RxmdError) as ei:
        p.set_qeq_precision(32)
    assert ei.value.code == RXMD_E_ARG
    it, est = p.QEq()                                 # ... and the engine still runs, at 64
    assert it >= 1 and np.isfinite(est) and p.qeq_precision() == (64, 64)
    p.set_qeq_precision(64)                           # (asking for what is in force is no error)
    p.close()
    monkeypatch.setenv("RXMD_QEQ_F32", "1")           # the environment switch is ignored for PQEq
    p = _engine("sicnp", (1, 1, 1), pqeq=oa.PQEQ_SICNP, QEq_tol=1e-7, NMAXQEq=500)
    assert p.qeq_precision() == (64, 64)
    it, est = p.QEq()
    assert it >= 1 and p.qeq_precision() == (64, 64)
    p.close()
