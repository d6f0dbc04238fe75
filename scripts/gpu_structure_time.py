"""Device time of one structure_sample (RxmdEngine.structure_sample: residents per type, the pair pass, the angle pass; structure.hip) next to the
export route it replaces.  RDX at the benchmark size 18x18x18 (979,776 atoms) by default, one rank, after QEq + FORCE and a second list build (the
window-slot route, the state a caller meets in a loop of steps) with bench.py's run parameters, one process, one state.  Legs:
  * structure_sample with r_max 10 A, 1000 bins, no shells (the pair pass);
  * the same with shells (2, 4, 6) A and 180 angle bins (pair pass + angle pass);
  * pairs_device count-only at r_cut = 10 A: the same row walk without histogramming, the floor of the pair pass;
  * the whole-list fill of pairs_device (src, dst, shift3, vec3): what a g(r) in torch would have to export first.
A host clock around a synchronised call, median of --reps after --warmup (structure_sample itself makes no host wait: the device is synchronised
behind it).  Writes the table to --out (default profiles/structure_stats.txt) and prints one JSON object.
Usage: python scripts/gpu_structure_time.py [--reps 5] [--warmup 2] [--cells 18] [--out profiles/structure_stats.txt]"""
import argparse, json, os, sys, time

os.environ["RXMD_PLACE_TRIES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_stats.txt"))
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
        return float(np.median(ms[a.warmup:])), float(min(ms[a.warmup:])), float(max(ms[a.warmup:]))

    ff, names, frac, lat, cells, wname, pqeq = bench.make_workload("rdx", a.cells)
    lat_super, rec = system.geninit(ff, names, frac, lat, mc=cells)
    e = rxmd_amd.RxmdEngine(ff, lat_super, **kw)
    e.set_atoms_rxff(rec)
    e.QEq(); e.FORCE()
    e.set_charges(e.atoms()["q"]); e.QEq(); e.FORCE()          # the second build: partners through the window slots
    st = e.stats()
    n, nnz = e.natoms, st["nnz10"]
    route = 2 if e.debug(15, cap=2)[0] == 0.0 else 4
    out = {"workload": wname, "atoms": n, "list_entries": int(nnz), "reps": a.reps, "warmup": a.warmup, "route_bytes": route}
    lines = ["structure statistics on the device (scripts/gpu_structure_time.py): %s, %d atoms, %d list entries, decode through the %s"
             % (wname, n, nnz, "2-byte window slots" if route == 2 else "4-byte entries"),
             "host clock around synchronised calls, ms: median (min .. max) of %d after %d, one process, one state" % (a.reps, a.warmup), "",
             "%-58s %10s   %s" % ("leg", "ms", "counted per sample")]

    def leg(tag, call, what):
        med, lo, hi = timed(call)
        out[tag] = dict(ms=med, ms_min=lo, ms_max=hi, counted=what)
        lines.append("%-58s %10.3f   (%.3f .. %.3f)   %s" % (tag, med, lo, hi, what))

    e.structure_begin(10.0, 1000)
    leg("structure_sample r_max 10, 1000 bins, no shells", e.structure_sample, "")
    c = e.structure_counts()
    pairs = int(c["pair_counts"].sum() // c["frames"])
    lines[-1] = lines[-1] + "%d pair counts" % pairs
    out["structure_sample r_max 10, 1000 bins, no shells"]["counted"] = dict(pairs=pairs)
    e.structure_begin(10.0, 1000, (2.0, 4.0, 6.0), 180)
    leg("structure_sample + shells (2, 4, 6) A, 180 angle bins", e.structure_sample, "")
    c = e.structure_counts()
    angles = [int(x.sum() // (2 * c["frames"])) for x in c["angle_counts"]]
    lines[-1] = lines[-1] + "%d pair counts, angles per shell %s" % (pairs, angles)
    out["structure_sample + shells (2, 4, 6) A, 180 angle bins"]["counted"] = dict(pairs=pairs, angles_per_shell=angles)
    e.structure_end()
    E10 = e.pairs_device(0, 0, 0, r_cut=10.0)
    leg("pairs_device count-only, r_cut 10 A", lambda: e.pairs_device(0, 0, 0, r_cut=10.0), "%d edges" % E10)
    E = e.pairs_device(0, 0, 0, r_cut=0.0)
    src = torch.empty(E, dtype=torch.int64, device=dev); dst = torch.empty_like(src)
    shift = torch.empty((E, 3), dtype=torch.int32, device=dev); vec = torch.empty((E, 3), dtype=torch.float64, device=dev)
    leg("pairs_device whole-list fill (src, dst, shift3, vec3)", lambda: e.pairs_device(E, src.data_ptr(), dst.data_ptr(), shift_ptr=shift.data_ptr(), vec_ptr=vec.data_ptr(), r_cut=0.0),
        "%d edges, %.1f GB written" % (E, E * 52 / 1e9))
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
