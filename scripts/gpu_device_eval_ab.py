"""Wall time of one QEq + FORCE pair on the same positions through the two array-shaped routes: host arrays in the reference's shapes
(RxmdEngine.QEq_arrays + FORCE_arrays: upload, run, download) and device tensors (rxmd_amd.torch_front.ReaxFF.evaluate: nothing crosses
PCIe but the 14 energies and the virial).  RDX 6x6x6 (36,288 atoms) and the benchmark size 18x18x18 (979,776 atoms), bench.py's run
parameters, one process, each leg after warm-up, every pair from zero charges (the same CG work on both sides), the placement search of
the window pass off on both sides.  A host clock around calls that return after the engine's stream is idle.  One JSON object per size.
Usage: python scripts/gpu_device_eval_ab.py [--reps 10] [--warmup 2] [--cells 6 18]"""
import argparse, json, os, sys, time

os.environ["RXMD_PLACE_TRIES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, nargs="+", default=[6, 18])
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import rxmd_amd
    from rxmd_amd import system
    from rxmd_amd.torch_front import ReaxFF
    cfg = system.parse_rxmd_in(os.path.join(bench.INP, "rxmd.in"))
    kw = dict(isQEq=1, NMAXQEq=cfg["NMAXQEq"], QEq_tol=cfg["QEq_tol"], qeq_mode=1)
    for c in a.cells:
        ff, names, frac, lat, cells, wname, pqeq = bench.make_workload("rdx", c)
        lat_super, rec = system.geninit(ff, names, frac, lat, mc=cells)
        n = len(rec)
        e = rxmd_amd.RxmdEngine(ff, lat_super, **kw)
        e.set_atoms_rxff(rec)
        at = e.atoms()                                   # real coordinates, types, gids as the engine holds them
        e.close()
        typ, gid, pos = at["type"], at["gid"], at["pos"]
        out = {"workload": wname, "atoms": n, "reps": a.reps, "warmup": a.warmup, "QEq_tol": cfg["QEq_tol"], "qeq_mode": 1, "RXMD_PLACE_TRIES": 1}

        # leg 1: host arrays in the reference's shapes
        e = rxmd_amd.RxmdEngine(ff, lat_super, **kw)
        atype = np.ascontiguousarray(typ + gid * 1e-13); posf = np.asfortranarray(pos)
        ms = []
        for k in range(a.warmup + a.reps):
            q = np.zeros(n)
            posf[0, 0] += 1e-13 * (k + 1)                # (new positions for the entry point: it keeps its lists for arrays it has seen)
            t0 = time.perf_counter()
            e.QEq_arrays(atype, posf, q, n)
            f, pe_h = e.FORCE_arrays(atype, posf, q, n)
            ms.append((time.perf_counter() - t0) * 1e3)
        it_h = e.stats()["qeq_iters_last"]
        e.close()
        out["ms_pair_host_arrays"] = float(np.median(ms[a.warmup:])); out["ms_pair_host_arrays_min_max"] = [min(ms[a.warmup:]), max(ms[a.warmup:])]

        # leg 2: device tensors
        m = ReaxFF(ff, lat_super, typ, gid=gid, **kw)
        p = torch.as_tensor(np.ascontiguousarray(pos), device="cuda:0"); q0 = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        ms = []
        for k in range(a.warmup + a.reps):
            p[0, 0] += 1e-13 * (k + 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = m.evaluate(p, q0=q0)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        it_d = m.engine.stats()["qeq_iters_last"]
        pe_d = o["pe"].numpy()
        out["ms_pair_device_tensors"] = float(np.median(ms[a.warmup:])); out["ms_pair_device_tensors_min_max"] = [min(ms[a.warmup:]), max(ms[a.warmup:])]
        out["qeq_iters_last"] = [it_h, it_d]
        out["pe0_rel_diff"] = abs(pe_d[0] - pe_h[0]) / abs(pe_h[0])
        out["f_max_abs_diff"] = float(np.abs(o["forces"].cpu().numpy() - np.ascontiguousarray(f[:n])).max())
        m.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
