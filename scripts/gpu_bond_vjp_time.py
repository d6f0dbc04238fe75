"""Time of one vector-Jacobian product of the bond-order graph (RxmdEngine.bonds_vjp_device: select + scan + five kernels + the ghost fold + egress,
one host wait for the count) on RDX at the benchmark size 18x18x18 (979,776 atoms, 5,225,472 directed bonds), one rank, after QEq + FORCE with
bench.py's run parameters, one process.  Two legs: grad_bo alone, and all three gradients (bond order, its three parts, the bond vector).
An event pair on torch's current stream around --calls consecutive calls after --warmup calls; milliseconds per call = elapsed / calls.
Next to it, from the same engine: count + fill of the graph itself (RxmdEngine.bonds_device, timed the same way) and rxmd_stats.ms_k_assemble of
one FORCE, the force assembly this call resembles.  One JSON object per size.
Usage: python scripts/gpu_bond_vjp_time.py [--calls 20] [--warmup 3] [--cells 18]"""
import argparse, json, os, sys

os.environ["RXMD_PLACE_TRIES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cells", type=int, nargs="+", default=[18])
    a = ap.parse_args()
    import torch
    import bench
    import rxmd_amd
    from rxmd_amd import system
    cfg = system.parse_rxmd_in(os.path.join(bench.INP, "rxmd.in"))
    kw = dict(isQEq=1, NMAXQEq=cfg["NMAXQEq"], QEq_tol=cfg["QEq_tol"], qeq_mode=1)
    dev = "cuda:0"

    def per_call(call):
        for _ in range(a.warmup):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.calls):
            call()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.calls

    for c in a.cells:
        ff, names, frac, lat, cells, wname, pqeq = bench.make_workload("rdx", c)
        lat_super, rec = system.geninit(ff, names, frac, lat, mc=cells)
        e = rxmd_amd.RxmdEngine(ff, lat_super, **kw)
        e.set_atoms_rxff(rec)
        e.QEq(); e.FORCE()
        e.reset_timers(); e.FORCE()
        n = e.natoms
        out = {"workload": wname, "atoms": n, "calls": a.calls, "warmup": a.warmup, "ms_k_assemble_one_force": e.stats()["ms_k_assemble"]}
        stream = torch.cuda.current_stream().cuda_stream
        for bo_min in (0.0, 0.3):
            E = e.bonds_device(0, 0, 0, 0, bo_min=bo_min)
            tag = "bo_min_%g" % bo_min
            out["selected_" + tag] = E
            src = torch.empty(E, dtype=torch.int64, device=dev); dst = torch.empty_like(src)
            b = torch.empty(E, dtype=torch.float64, device=dev)
            parts = torch.empty((E, 3), dtype=torch.float64, device=dev); vec = torch.empty_like(parts)

            def graph(extra):
                e.bonds_device(0, 0, 0, 0, bo_min=bo_min, stream=stream)
                e.bonds_device(E, src.data_ptr(), dst.data_ptr(), b.data_ptr(), bo3_ptr=parts.data_ptr() if extra else 0, vec_ptr=vec.data_ptr() if extra else 0,
                               bo_min=bo_min, stream=stream)
            out["ms_graph_count_fill_" + tag] = per_call(lambda: graph(False))
            out["ms_graph_count_fill_parts_vec_" + tag] = per_call(lambda: graph(True))
            g_bo = torch.randn(E, dtype=torch.float64, device=dev); g_parts = torch.randn((E, 3), dtype=torch.float64, device=dev); g_vec = torch.randn((E, 3), dtype=torch.float64, device=dev)
            gpos = torch.empty((n, 3), dtype=torch.float64, device=dev)
            out["ms_vjp_grad_bo_" + tag] = per_call(lambda: e.bonds_vjp_device(E, gpos.data_ptr(), grad_bo_ptr=g_bo.data_ptr(), bo_min=bo_min, stream=stream))
            first = gpos.clone()
            out["ms_vjp_all_three_" + tag] = per_call(lambda: e.bonds_vjp_device(E, gpos.data_ptr(), grad_bo_ptr=g_bo.data_ptr(), grad_bo3_ptr=g_parts.data_ptr(),
                                                                                 grad_vec_ptr=g_vec.data_ptr(), bo_min=bo_min, stream=stream))
            e.bonds_vjp_device(E, gpos.data_ptr(), grad_bo_ptr=g_bo.data_ptr(), bo_min=bo_min, stream=stream)
            out["repeats_its_bits_" + tag] = bool(torch.equal(first, gpos))
            out["sum_over_atoms_" + tag] = [float(x) for x in gpos.sum(0).cpu()]
        e.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
