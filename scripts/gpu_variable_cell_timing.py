"""Cost of the variable cell on the headline workload (RDX 18^3 = 979,776 atoms, bench.py's run parameters, qeq_mode 1): ms per step of
NVE, of the isotropic barostat coupling on every step and on every 10th, and the wall time of rxmd_hip_set_lattice without and with
capacity growth.  One JSON object on stdout.  Usage: python scripts/gpu_variable_cell_timing.py [--steps 20] [--warmup 3]"""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cells", type=int, default=18)
    a = ap.parse_args()
    import bench
    import rxmd_amd
    from rxmd_amd import system
    ff, names, frac, lat, cells, wname, pqeq = bench.make_workload("rdx", a.cells)
    cfg = system.parse_rxmd_in(os.path.join(bench.INP, "rxmd.in"))
    lat_super, rec = system.geninit(ff, names, frac, lat, mc=cells)
    e = rxmd_amd.RxmdEngine(ff, lat_super, isQEq=cfg["isQEq"], NMAXQEq=cfg["NMAXQEq"], QEq_tol=cfg["QEq_tol"], qstep=cfg["qstep"],
                            dt_fs=cfg["dt"], qeq_mode=1)
    e.set_atoms_rxff(rec)
    e.QEq(); e.FORCE(); e.step(a.warmup)
    out = {"workload": wname, "atoms": len(rec), "steps": a.steps, "warmup": a.warmup, "qeq_mode": 1}

    def timed_steps():
        t0 = time.perf_counter(); e.step(a.steps); return (time.perf_counter() - t0) * 1e3 / a.steps   # step() returns after its stream is idle

    out["ms_per_step_nve"] = timed_steps()
    # weak coupling (tau 1000 fs, max_strain 1e-3): the box barely moves, what is timed is the coupling itself
    e.set_barostat(1, p0=0.0, tau_fs=1000.0, bulk_modulus=15.0, every=1, max_strain=1e-3)
    e.step(a.warmup)
    out["ms_per_step_barostat_every1"] = timed_steps()
    e.set_barostat(1, p0=0.0, tau_fs=1000.0, bulk_modulus=15.0, every=10, max_strain=1e-3)
    out["ms_per_step_barostat_every10"] = timed_steps()
    e.set_barostat(0)
    out["ms_per_step_nve_again"] = timed_steps()
    out["couplings"] = e.barostat_state()["couplings"]
    L = e.lattice
    nb0 = e.stats()["nbuffer"]
    t0 = time.perf_counter(); e.set_lattice([L[0] * 1.0001, L[1] * 1.0001, L[2] * 1.0001] + L[3:]); ms = (time.perf_counter() - t0) * 1e3
    out["ms_set_lattice_no_growth"] = ms
    out["nbuffer_after_no_growth"] = e.stats()["nbuffer"]
    # z just below the next multiple of the bond cut-off: one fewer reference cell along z, a wider normalised ghost shell, more atom slots
    _, maxrc = e.cutoffs()
    L = e.lattice
    cz = int(L[2] / maxrc)
    t0 = time.perf_counter(); e.set_lattice(L[:2] + [cz * maxrc - 0.01] + L[3:]); ms = (time.perf_counter() - t0) * 1e3
    st = e.stats()
    out["ms_set_lattice_with_growth"] = ms
    out["nbuffer_before"] = nb0; out["nbuffer_after_growth"] = st["nbuffer"]; out["cells3_after_growth"] = st["cells3"]
    e.QEq(); e.FORCE()
    out["ms_per_step_nve_after_growth"] = timed_steps()
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
