"""Wall time of getting the bond-order graph of the last FORCE out of the engine: the host route (RxmdEngine.bonds: four device-to-host copies,
a serial loop over the atoms, padded [natoms][32] arrays) against the device route (RxmdEngine.bonds_device: count, then fill into preallocated
torch tensors; flag + exclusive sum + fill, one host wait each for the count).  RDX at the benchmark size 18x18x18 (979,776 atoms) by default,
one rank, after QEq + FORCE with bench.py's run parameters, one process.  The device legs: bo_min 0 and 0.3, with and without the optional
outputs (the three parts of the bond order and the bond vector).  A host clock around a synchronised call, median of --reps after --warmup.
One JSON object per size.
Usage: python scripts/gpu_bond_graph_ab.py [--reps 10] [--warmup 2] [--cells 18]"""
import argparse, json, os, sys, time

os.environ["RXMD_PLACE_TRIES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, nargs="+", default=[18])
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import rxmd_amd
    from rxmd_amd import system
    cfg = system.parse_rxmd_in(os.path.join(bench.INP, "rxmd.in"))
    kw = dict(isQEq=1, NMAXQEq=cfg["NMAXQEq"], QEq_tol=cfg["QEq_tol"], qeq_mode=1)
    dev = "cuda:0"

    def timed(call):
        ms = []
        for _ in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = ms[a.warmup:]
        return dict(median=float(np.median(ms)), min=min(ms), max=max(ms))

    for c in a.cells:
        ff, names, frac, lat, cells, wname, pqeq = bench.make_workload("rdx", c)
        lat_super, rec = system.geninit(ff, names, frac, lat, mc=cells)
        e = rxmd_amd.RxmdEngine(ff, lat_super, **kw)
        e.set_atoms_rxff(rec)
        e.QEq(); e.FORCE()
        n = e.natoms
        out = {"workload": wname, "atoms": n, "reps": a.reps, "warmup": a.warmup}
        out["ms_host_bonds"] = timed(lambda: e.bonds())
        cnt, pg, bo = e.bonds()
        out["directed_bonds"] = int(cnt.sum())
        for bo_min in (0.0, 0.3):
            E = e.bonds_device(0, 0, 0, 0, bo_min=bo_min)
            src = torch.empty(E, dtype=torch.int64, device=dev); dst = torch.empty_like(src)
            b = torch.empty(E, dtype=torch.float64, device=dev)
            parts = torch.empty((E, 3), dtype=torch.float64, device=dev); vec = torch.empty_like(parts)
            tag = "bo_min_%g" % bo_min
            out["selected_" + tag] = E
            out["ms_device_count_" + tag] = timed(lambda: e.bonds_device(0, 0, 0, 0, bo_min=bo_min))

            def pair(extra):
                e.bonds_device(0, 0, 0, 0, bo_min=bo_min)
                e.bonds_device(E, src.data_ptr(), dst.data_ptr(), b.data_ptr(), bo3_ptr=parts.data_ptr() if extra else 0, vec_ptr=vec.data_ptr() if extra else 0, bo_min=bo_min)
            out["ms_device_count_fill_" + tag] = timed(lambda: pair(False))
            out["ms_device_count_fill_parts_vec_" + tag] = timed(lambda: pair(True))
        # the two routes hold the same numbers (local indices -> global ids on the host)
        gid = e.atoms()["gid"]
        E = e.bonds_device(0, 0, 0, 0)
        src = torch.empty(E, dtype=torch.int64, device=dev); dst = torch.empty_like(src); b = torch.empty(E, dtype=torch.float64, device=dev)
        e.bonds_device(E, src.data_ptr(), dst.data_ptr(), b.data_ptr())
        mask = np.arange(pg.shape[1])[None, :] < cnt[:, None]
        out["same_as_host"] = bool(np.array_equal(gid[src.cpu().numpy()], np.repeat(gid, cnt)) and np.array_equal(gid[dst.cpu().numpy()], pg[mask])
                                   and np.array_equal(b.cpu().numpy(), bo[mask]))
        e.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
