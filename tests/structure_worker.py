"""worker of tests/test_gpu_structure.py (spawned by torch.multiprocessing): one rank of a decomposed box that samples its structure statistics once
and writes its counts dict to a file.  The system comes from graph_worker.build_system, which the parent uses for the single-rank engine too."""
import os, sys, traceback
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))

import graph_worker
import mr_worker


def structure_rank(rank, world, port, spec, out):
    """spec: the keys of graph_worker.build_system and dict(kw=engine keywords, begin=(r_max, nbins_r, angle_cuts, nbins_angle), dir)"""
    try:
        dist = mr_worker._init(rank, world, port)
        import torch
        import rxmd_amd
        from rxmd_amd.comm import TorchTransport
        ff, lat, ranks, vs = graph_worker.build_system(spec)
        e = rxmd_amd.RxmdEngine(ff, lat, vprocs=tuple(spec["vp"]), myid=rank, device=0, qeq_mode=1, **spec["kw"])
        tr = TorchTransport(mode="staged", device=torch.device("cuda", 0), capacity_doubles=1 << 21)
        tr.attach(e)
        e.set_atoms_rxff(graph_worker.rec10(ranks[rank]))
        e.QEq(); e.FORCE()
        r_max, nbr, cuts, nba = spec["begin"]
        e.structure_begin(r_max, nbr, cuts, nba)
        e.structure_sample()
        c = e.structure_counts()
        n_exchange = tr.n_exchange
        e.structure_sample()                                   # a second sample: no message may be sent for it
        c2 = e.structure_counts()
        np.savez(os.path.join(spec["dir"], "rank%d.npz" % rank), pair_counts=c["pair_counts"], angle_counts=c["angle_counts"], atoms_per_type=c["atoms_per_type"],
                 volume_sum=c["volume_sum"], frames=c["frames"], natoms=e.natoms, doubled=np.array_equal(c2["pair_counts"], 2 * c["pair_counts"]),
                 messages_of_a_sample=tr.n_exchange - n_exchange, transport_error=repr(tr.error))
        out[rank] = dict(ok=True)
        e.structure_end(); e.close()
        dist.barrier(); dist.destroy_process_group()
    except Exception:
        out[rank] = dict(error=traceback.format_exc())
