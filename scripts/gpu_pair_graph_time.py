"""Device time of getting the 10 A pair graph out of the engine (RxmdEngine.pairs_device: count per row, 64-bit exclusive sum, fill into preallocated
torch tensors).  RDX at the benchmark size 18x18x18 (979,776 atoms) by default, one rank, after QEq + FORCE with bench.py's run parameters, one
process.  Legs: r_cut 5 A and the whole list (r_cut 0), each with src / dst / shift3 / vec3 and with hval on top.  A host clock around a synchronised
call (the call has one host wait of its own, for the count), median of --reps after --warmup; the count-only call and the fill call, which
counts again before it fills (count + exclusive sum + fill): a caller that counts, allocates and fills pays both.
Next to each time: edges, the algorithmic bytes of the leg (pair_graph.hip: per list entry 2 or 4 bytes of slot / entry + 4 of perm + 24 of position
in either pass; per selected entry 16 + 12 + 24 out, + 8 in and 8 out for hval) and that byte count over the time as a fraction of the 6.87 TB/s
plain-stream rate VERDICT.md quotes.  As a yardstick: rxmd_stats.ms_k_list10 of the same process, the sweep that BUILDS the list (per build).
Writes the table to --out (default profiles/pair_graph.txt) and prints one JSON object.
Usage: python scripts/gpu_pair_graph_time.py [--reps 5] [--warmup 2] [--cells 18] [--out profiles/pair_graph.txt]"""
import argparse, json, os, sys, time

os.environ["RXMD_PLACE_TRIES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STREAM_TBS = 6.87


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_graph.txt"))
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
        return float(np.median(ms[a.warmup:]))

    ff, names, frac, lat, cells, wname, pqeq = bench.make_workload("rdx", a.cells)
    lat_super, rec = system.geninit(ff, names, frac, lat, mc=cells)
    e = rxmd_amd.RxmdEngine(ff, lat_super, **kw)
    e.set_atoms_rxff(rec)
    e.QEq(); e.FORCE()
    # a second list build at the same positions: the first build of an engine always writes the 4-byte entries, every later one of a default engine
    # leaves them out (lists.hip: needs_nb10) -- the state a caller meets in a loop of evaluations or steps.  (FORCE behind QEq does not build again.)
    builds = 2
    e.set_charges(e.atoms()["q"]); e.QEq(); e.FORCE()
    st = e.stats()
    n, nnz = e.natoms, st["nnz10"]
    route = 2 if e.debug(15, cap=2)[0] == 0.0 else 4          # bytes per list entry of the stream the kernels decode: window slots or 4-byte entries
    out = {"workload": wname, "atoms": n, "list_entries": int(nnz), "reps": a.reps, "warmup": a.warmup, "route_bytes": route,
           "streams_by_place": st["streams_by_place"], "ms_k_list10_per_build": st["ms_k_list10"] / builds}
    lines = ["10 A pair graph on device arrays (scripts/gpu_pair_graph_time.py): %s, %d atoms, %d list entries, decode through the %s"
             % (wname, n, nnz, "2-byte window slots" if route == 2 else "4-byte entries"),
             "host clock around synchronised calls, median of %d after %d; bytes = algorithmic bytes of the leg; fraction of the %.2f TB/s plain-stream rate"
             % (a.reps, a.warmup, STREAM_TBS),
             "yardstick: ms_k_list10 (the sweep that builds the list) %.3f ms per build" % out["ms_k_list10_per_build"], "",
             "%-28s %12s %10s %10s %10s %9s" % ("leg", "edges", "ms count", "ms fill", "GB (fill)", "of stream")]
    for r_cut in (5.0, 0.0):
        E = e.pairs_device(0, 0, 0, r_cut=r_cut)
        src = torch.empty(E, dtype=torch.int64, device=dev); dst = torch.empty_like(src)
        shift = torch.empty((E, 3), dtype=torch.int32, device=dev)
        vec = torch.empty((E, 3), dtype=torch.float64, device=dev); hv = torch.empty(E, dtype=torch.float64, device=dev)
        ms_count = timed(lambda: e.pairs_device(0, 0, 0, r_cut=r_cut))
        for with_h in (False, True):
            def fill():
                e.pairs_device(E, src.data_ptr(), dst.data_ptr(), shift_ptr=shift.data_ptr(), vec_ptr=vec.data_ptr(), h_ptr=hv.data_ptr() if with_h else 0, r_cut=r_cut)
            ms = timed(fill)
            walk = nnz * (route + 4 + 24)              # one pass over the list: the stream, perm, the partner's position
            nbytes = (walk if r_cut > 0 else 8 * n) + walk + E * (16 + 12 + 24 + (16 if with_h else 0))   # the fill call counts again, then fills
            tag = ("r_cut %.0f A" % r_cut if r_cut > 0 else "whole list") + (" + hval" if with_h else "")
            frac = nbytes / (ms * 1e-3) / (STREAM_TBS * 1e12)
            out[tag] = dict(edges=int(E), ms_count_call=ms_count, ms_fill_call=ms, gbytes=nbytes / 1e9, fraction_of_stream=frac)
            lines.append("%-28s %12d %10.3f %10.3f %10.2f %9.3f" % (tag, E, ms_count, ms, nbytes / 1e9, frac))
        del src, dst, shift, vec, hv
        torch.cuda.empty_cache()
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
