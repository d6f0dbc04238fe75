"""rank function of tests/test_gpu_structure.py (started by ranks.run_ranks): one rank of a decomposed box that samples its structure statistics once
and writes its counts dict to a file.  The system comes from parity.build_system, which the parent uses for the single-rank engine too."""
import os
import numpy as np

import ranks
from parity import build_system, rec10


@ranks.entry
def structure_rank(rank, world, spec):
    """spec: the keys of parity.build_system and dict(kw=engine keywords, begin=(r_max, nbins_r, angle_cuts, nbins_angle), dir)"""
    import rxmd_amd
    ff, lat, recs, vs = build_system(spec)
    e = rxmd_amd.RxmdEngine(ff, lat, vprocs=tuple(spec["vp"]), myid=rank, device=0, qeq_mode=1, **spec["kw"])
    tr = ranks.staged_transport(1 << 21)
    tr.attach(e)
    e.set_atoms_rxff(rec10(recs[rank]))
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
    e.structure_end(); e.close()
    return dict(ok=True)
