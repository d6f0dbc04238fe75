"""Run by test_gpu_parity.py::test_poisoned_allocations in a process of its own (RXMD_POISON_ALLOC is read once per process): every engine
buffer starts as 0xFF bytes -- NaN for doubles, -1 for indices -- and the per-step scratch is filled with the pattern again before every rebuild.
A kernel that read an element nobody wrote this step would turn charges, forces or energies into NaN or trap on an index."""
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
import oracle_api as oa
from parity import _engine, _oracle, q_err, f_err, e_err, lattice_sequence

assert os.environ.get("RXMD_POISON_ALLOC") == "1"
kw = dict(QEq_tol=1e-12, NMAXQEq=2000)


def gate_static(tag, e, q0, f0, pe0, pqeq):
    """QEq + FORCE of the engine against (q0, f0 by gid, pe0): 1e-6 for q and f, 1e-9 for E (PQEq 5e-9)"""
    e.QEq(); pe = e.FORCE()
    tap = e.debug(14, cap=2)
    assert tap[0] == 1.0 and np.isnan(tap[1]), tap          # the pattern is on, and an element no kernel writes still holds it
    a = e.atoms()
    assert np.isfinite(a["q"]).all() and np.isfinite(a["f"]).all() and np.isfinite(pe).all()
    ie = np.argsort(a["gid"])
    errs = (q_err(a["q"][ie], q0), f_err(a["f"][ie], f0), e_err(pe, pe0))
    print(tag, "step 0: q %.2e f %.2e E %.2e" % errs, "PE", ["%.6g" % (x - y) for x, y in zip(pe, pe0)], flush=True)
    assert errs[0] <= 1e-6 and errs[1] <= 1e-6 and errs[2] <= (5e-9 if pqeq else 1e-9), errs      # (PQEq: PE(12) and PE(13) are large sums of opposite sign, their 1e-7 CG noise cancels in PE(0) only)


def finite_state(e):
    a = e.atoms(); en = e.energy()
    assert np.isfinite(a["q"]).all() and np.isfinite(a["f"]).all() and np.isfinite(a["pos"]).all() and np.isfinite(en["PE"]).all() and np.isfinite(en["KE"])
    return a


def gate_run(tag, e, ref, steps, pqeq):
    gate_static(tag, e, ref["q0"], ref["f0"], ref["pe0"], pqeq)
    e.step(steps)
    a = finite_state(e)
    ie = np.argsort(a["gid"])
    assert np.abs(a["pos"][ie] - ref["pos1"]).max() <= 1e-9
    assert q_err(a["q"][ie], ref["q1"]) <= 1e-6 and f_err(a["f"][ie], ref["f1"]) <= 1e-6


refs = {}
for case, mc, extra, steps in (("rdx222", (2, 2, 2), {}, 3), ("sicnp", (1, 1, 1), dict(pqeq=oa.PQEQ_SICNP), 2)):
    o = _oracle(case, mc, **kw, **extra)                        # (the oracle once per case: most of this test's time is its PQEq solve on the host)
    if extra:
        o.set_pqeq_clean(1)
    o.qeq(); o.force()
    io = np.argsort(o.gids())
    ref = refs[case] = dict(q0=o.charges()[io].copy(), f0=o.forces()[io].copy(), pe0=o.energy().copy())
    o.step(steps)
    io1 = np.argsort(o.gids())
    ref.update(pos1=o.pos()[io1].copy(), q1=o.charges()[io1].copy(), f1=o.forces()[io1].copy())
    for qeq_mode in (1, 0):
        e = _engine(case, mc, qeq_mode=qeq_mode, **kw, **extra)
        gate_run("%s qeq_mode %d" % (case, qeq_mode), e, ref, steps, bool(extra))
        e.close()

# ---- the pattern refill after a re-allocation: every growth path of the engine's buffers under the switch (a table entry with a stale size
# would write the pattern past the new block, or leave the new block's tail unfilled)
# (a) the bond tables grow in the first build (test_bond_tables_grow_on_demand), against the oracle run of above
os.environ["RXMD_BOND_CAP"] = "1024"
try:
    e = _engine("rdx222", (2, 2, 2), qeq_mode=1, **kw)
finally:
    del os.environ["RXMD_BOND_CAP"]
gate_run("(a) rdx222 bond tables from 1024", e, refs["rdx222"], 3, False)
assert e.stats()["nbonds"] > 1024
e.close()

# (b) set_lattice: the grid-sized buffers are re-allocated at the expansion, every per-atom buffer at the compression (parity.lattice_sequence);
# the oracle follows through its own set_lattice and the same steps
o = _oracle("rdx222", (2, 2, 2), **kw)
e = _engine("rdx222", (2, 2, 2), **kw)
seq = dict(lattice_sequence(list(e.lattice), e.cutoffs()[1]))
o.qeq(); o.force()
gate_static("(b) rdx222 at L0", e, refs["rdx222"]["q0"], refs["rdx222"]["f0"], refs["rdx222"]["pe0"], False)      # a live engine: lists, charges, forces of L0 exist
st0 = e.stats()
for name in ("expanded", "compressed"):
    e.set_lattice(seq[name]); o.set_lattice(seq[name])
    st = e.stats()
    print("(b)", name, "cells10", list(st["cells10"]), "nbuffer", st0["nbuffer"], "->", st["nbuffer"], flush=True)
    if name == "expanded":
        assert all(st["cells10"][a] > st0["cells10"][a] for a in range(3)), (st0["cells10"], st["cells10"])
    else:
        assert st["nbuffer"] > st0["nbuffer"], (st0["nbuffer"], st["nbuffer"])
    o.qeq(); o.force()
    io = np.argsort(o.gids())
    gate_static("(b) rdx222 " + name, e, o.charges()[io], o.forces()[io], o.energy(), False)
    e.step(2); o.step(2)
    finite_state(e)
    st0 = st
e.close()

# (c), (d) the row stride of the 10 A list grows (nb10, hess, sl10; with PQEq also hsc: the only path that re-allocates it): the SiC particle in a
# box widened 3 x along x (test_row_stride_of_the_10A_list_grows_...), against an engine created with the grown stride, which takes no growth path
import rxmd_amd
from rxmd_amd import system
ff, names, frac, lat = oa.make_system("sicnp")
lat3, rec = system.geninit(ff, names, frac, lat, mc=(1, 1, 1))
lat_wide = list(lat3); lat_wide[0] *= 3.0
rec2 = rec.copy(); rec2[:, 0] = rec2[:, 0] / 3.0
for tag, extra, gates in (("(c) sicnp wide", {}, (1e-12, 1e-11, 1e-12)), ("(d) sicnp wide PQEq", dict(pqeq=oa.PQEQ_SICNP), (1e-6, 1e-6, 5e-9))):
    res = []
    stride = 0                                                # first engine: sized from the mean density, has to grow
    for run in range(2):
        e = rxmd_amd.RxmdEngine(ff, lat_wide, **kw, **extra, **(dict(maxneighbs10=stride) if stride else {}))
        e.set_atoms_rxff(rec2)
        s0 = e.stats()["n10_stride"]
        e.QEq(); pe = e.FORCE()
        s1 = e.stats()["n10_stride"]
        assert (s1 > s0) if run == 0 else (s1 == s0 == stride), (run, s0, s1, stride)
        stride = s1
        e.step(2)
        a = finite_state(e)
        assert np.isfinite(pe).all()
        ig = np.argsort(a["gid"])
        res.append((a["q"][ig].copy(), a["f"][ig].copy(), pe.copy()))
        e.close()
    errs = (q_err(res[0][0], res[1][0]), f_err(res[0][1], res[1][1]), e_err(res[0][2], res[1][2]))
    print(tag, "stride grown to %d, against the engine created with it: q %.2e (gate %.0e) f %.2e (%.0e) E %.2e (%.0e)" % (stride, errs[0], gates[0], errs[1], gates[1], errs[2], gates[2]), flush=True)
    assert errs[0] <= gates[0] and errs[1] <= gates[1] and errs[2] <= gates[2], errs
print("POISON-OK")
