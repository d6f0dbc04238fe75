"""rank function of tests/test_gpu_graphs_multirank.py (started by ranks.run_ranks): one rank of a decomposed box that exports its bond-order
graph and its 10 A pair graph with global ids and writes them to a file; parity.build_system is shared with the parent, which gives the multi-rank
oracle the same per-rank records"""
import json, os
import numpy as np

import ranks
from parity import build_system, rec10, code as _code
from graph_support import device_coo, _device_coo, _host_coo


def _pairs(e, r_cut):
    """count only, then the fill into sentinel-filled tensors three entries longer than the count -> (count, whole arrays)"""
    cnt = e.pairs_device(0, 0, 0, r_cut=r_cut, as_gid=True)
    E, s, d, sh, vec, hv = device_coo(e, r_cut, as_gid=True, capacity=cnt + 3, want=(False, True, True))
    return cnt, E, s, d, vec, hv


def _bonds(e, bo_min):
    cnt = e.bonds_device(0, 0, 0, 0, bo_min=bo_min, as_gid=True)
    return (cnt,) + _device_coo(e, bo_min=bo_min, as_gid=True, capacity=cnt + 3)


def _state(e, cuts, tag, out):
    """everything the parent holds to its references, of the engine's present state, under keys that start with `tag`"""
    a = e.atoms()
    for k in ("gid", "type", "pos", "q"):
        out[tag + k] = a[k]
    out[tag + "stats"] = json.dumps({k: (v if isinstance(v, (int, float, str)) else repr(v)) for k, v in e.stats().items()})
    cnt, pg_, bo = e.bonds()
    out[tag + "hb_cnt"], out[tag + "hb_pg"], out[tag + "hb_bo"] = cnt, pg_, bo
    out[tag + "dbg6"], out[tag + "dbg7"] = e.debug(6), e.debug(7)
    same = True
    for bo_min in (0.0, 0.3):
        _, hs, hd, hb = _host_coo(e, bo_min=bo_min if bo_min else None)
        first = _bonds(e, bo_min)
        again = _bonds(e, bo_min)
        same = same and all(np.array_equal(x, y) for x, y in zip(first, again))
        for name, arr in zip(("cnt", "E", "src", "dst", "bo", "bo3", "vec"), first):
            out["%sbd%.1f_%s" % (tag, bo_min, name)] = arr
        out["%shost%.1f_src" % (tag, bo_min)], out["%shost%.1f_dst" % (tag, bo_min)], out["%shost%.1f_bo" % (tag, bo_min)] = hs, hd, hb
    for r_cut in cuts:
        first = _pairs(e, r_cut)
        again = _pairs(e, r_cut)
        same = same and all(np.array_equal(x, y) for x, y in zip(first, again))
        for name, arr in zip(("cnt", "E", "src", "dst", "vec", "hval"), first):
            out["%spd%.3f_%s" % (tag, r_cut, name)] = arr
    out[tag + "same_bits"] = same


@ranks.entry
def graph_rank(rank, world, spec):
    """one rank of a vprocs run; all ranks share GPU 0, messages host-staged over gloo.  spec: the keys of build_system and dict(kw=engine keywords,
    pqeq, f32, steps, cuts=cut-offs of the pair graph (0 = the whole list), cuts_after=those after step(steps), dir=where rank r writes rank<r>.npz)"""
    import torch
    import oracle_api as oa
    import rxmd_amd
    vp = tuple(spec["vp"])
    ff, lat, recs, vs = build_system(spec)
    kw = dict(spec.get("kw") or dict(QEq_tol=1e-12, NMAXQEq=2000))
    if spec.get("slab"):
        kw["nbuffer"] = 20000
    e = rxmd_amd.RxmdEngine(ff, lat, vprocs=vp, myid=rank, device=0, qeq_mode=spec.get("qeq_mode", 1), pqeq=oa.PQEQ_SICNP if spec.get("pqeq") else None, **kw)
    tr = ranks.staged_transport(1 << 21)
    tr.attach(e)
    e.set_atoms_rxff(rec10(recs[rank], None if vs is None else vs[rank]))
    if spec.get("f32"):
        e.set_qeq_precision(32)
    res = {}
    buf = torch.zeros(8, dtype=torch.int64, device="cuda:0"); p = buf.data_ptr()
    e.QEq()
    for r_cut in (6.5, 0.0):                                      # the list of a QEq call alone
        for name, arr in zip(("cnt", "E", "src", "dst", "vec", "hval"), _pairs(e, r_cut)):
            res["q_pd%.3f_%s" % (r_cut, name)] = arr
    pe = e.FORCE()
    res["codes"] = np.array([_code(lambda: e.bonds_device(0, 0, 0, 0)), _code(lambda: e.bonds_device(8, p, p, p)),
                             _code(lambda: e.pairs_device(0, 0, 0)), _code(lambda: e.pairs_device(8, p, p)),
                             _code(lambda: e.pairs_device(8, p, p, shift_ptr=p, as_gid=True))])
    res["refused_calls_wrote_nothing"] = bool((buf == 0).all().item())
    res["maxrc"] = e.cutoffs()[1]
    res["qeq_precision"] = np.array(e.qeq_precision())
    _state(e, spec["cuts"], "s0_", res)
    if spec.get("steps"):
        e.step(spec["steps"])
        _state(e, spec["cuts_after"], "s1_", res)
    res["transport"] = np.array([tr.n_exchange, tr.n_allreduce]); res["transport_error"] = repr(tr.error)
    np.savez(os.path.join(spec["dir"], "rank%d.npz" % rank), **res)
    e.close()
    return dict(ok=True)
