"""worker of tests/test_gpu_graphs_multirank.py (spawned by torch.multiprocessing): one rank of a decomposed box that exports its bond-order
graph and its 10 A pair graph with global ids and writes them to a file; `build_system` is shared with the parent, which gives the multi-rank
oracle the same per-rank records"""
import json, os, sys, traceback
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))

import mr_worker


def build_system(spec):
    """spec: dict(case, mc, vp, slab, shaken=(seed, sigma in A), v=(seed, sigma, natoms of the whole system)) -> (ffield, lattice of the whole
    box, per-rank dict(rnorm, type, gid) as rxff.bin would hold them, per-rank velocities or None)"""
    import oracle_api as oa
    vp = tuple(spec["vp"]); mc = tuple(spec.get("mc", (1, 1, 1)))
    if spec.get("slab"):
        ff, names, frac, lat = mr_worker.slab_system()
    else:
        ff, names, frac, lat = oa.make_system(spec["case"])
    ffn = oa.ffield_names(ff)
    if not spec.get("shaken"):
        lat2, ranks = oa.geninit(names, frac, lat, ffn, mc=mc, vprocs=vp)
    else:
        # test_gpu_scale._perturbed_rdx at another size and seed: the lattice positions displaced by N(0, sigma) per component, back into [0, 1)
        # as geninit and every migration leave them, then dealt to the domains of the rank grid the way geninit does (geninit.F90:493-527)
        seed, sigma = spec["shaken"]
        lat2, one = oa.geninit(names, frac, lat, ffn, mc=mc)
        assert tuple(lat2[3:6]) == (90.0, 90.0, 90.0)
        n = len(one[0]["type"])
        rn = one[0]["rnorm"] + np.random.default_rng(seed).normal(0, sigma, (n, 3)) / np.asarray(lat2[:3], dtype=np.float64)
        rn = rn - np.floor(rn)
        v3 = np.array(vp)
        dom = (rn * v3).astype(np.int64)
        sid = dom[:, 0] + dom[:, 1] * v3[0] + dom[:, 2] * v3[0] * v3[1]
        ranks = []
        for p in range(int(v3.prod())):
            sel = np.nonzero(sid == p)[0]
            obox = (1.0 / v3) * np.array([p % v3[0], (p // v3[0]) % v3[1], p // (v3[0] * v3[1])])
            ranks.append(dict(rnorm=rn[sel] - obox, type=one[0]["type"][sel].copy(), gid=one[0]["gid"][sel].copy()))
    vs = [mr_worker.mode_velocities(r["gid"], *spec["v"]) for r in ranks] if spec.get("v") else None
    return ff, [float(x) for x in lat2], ranks, vs


def rec10(rank, v=None):
    n = len(rank["type"])
    rec = np.zeros((n, 10))
    rec[:, 0:3] = rank["rnorm"]; rec[:, 7] = rank["type"] + rank["gid"] * 1e-13
    if v is not None:
        rec[:, 3:6] = v
    return rec


def _code(call):
    import rxmd_amd
    try:
        call()
    except rxmd_amd.RxmdError as ex:
        return ex.code
    return 0


def _pairs(e, r_cut, pg):
    """count only, then the fill into sentinel-filled tensors three entries longer than the count -> (count, whole arrays)"""
    cnt = e.pairs_device(0, 0, 0, r_cut=r_cut, as_gid=True)
    E, s, d, sh, vec, hv = pg.device_coo(e, r_cut, as_gid=True, capacity=cnt + 3, want=(False, True, True))
    return cnt, E, s, d, vec, hv


def _bonds(e, bo_min, bg):
    cnt = e.bonds_device(0, 0, 0, 0, bo_min=bo_min, as_gid=True)
    return (cnt,) + bg._device_coo(e, bo_min=bo_min, as_gid=True, capacity=cnt + 3)


def _state(e, cuts, tag, out, pg, bg):
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
        _, hs, hd, hb = bg._host_coo(e, bo_min=bo_min if bo_min else None)
        first = _bonds(e, bo_min, bg)
        again = _bonds(e, bo_min, bg)
        same = same and all(np.array_equal(x, y) for x, y in zip(first, again))
        for name, arr in zip(("cnt", "E", "src", "dst", "bo", "bo3", "vec"), first):
            out["%sbd%.1f_%s" % (tag, bo_min, name)] = arr
        out["%shost%.1f_src" % (tag, bo_min)], out["%shost%.1f_dst" % (tag, bo_min)], out["%shost%.1f_bo" % (tag, bo_min)] = hs, hd, hb
    for r_cut in cuts:
        first = _pairs(e, r_cut, pg)
        again = _pairs(e, r_cut, pg)
        same = same and all(np.array_equal(x, y) for x, y in zip(first, again))
        for name, arr in zip(("cnt", "E", "src", "dst", "vec", "hval"), first):
            out["%spd%.3f_%s" % (tag, r_cut, name)] = arr
    out[tag + "same_bits"] = same


def graph_rank(rank, world, port, spec, out):
    """one rank of a vprocs run; all ranks share GPU 0, messages host-staged over gloo.  spec: the keys of build_system and dict(kw=engine keywords,
    pqeq, f32, steps, cuts=cut-offs of the pair graph (0 = the whole list), cuts_after=those after step(steps), dir=where rank r writes rank<r>.npz)"""
    try:
        dist = mr_worker._init(rank, world, port)
        import torch
        import oracle_api as oa
        import rxmd_amd
        from rxmd_amd.comm import TorchTransport
        import test_gpu_pair_graph as pg
        import test_gpu_bond_graph as bg
        vp = tuple(spec["vp"])
        ff, lat, ranks, vs = build_system(spec)
        kw = dict(spec.get("kw") or dict(QEq_tol=1e-12, NMAXQEq=2000))
        if spec.get("slab"):
            kw["nbuffer"] = 20000
        e = rxmd_amd.RxmdEngine(ff, lat, vprocs=vp, myid=rank, device=0, qeq_mode=spec.get("qeq_mode", 1), pqeq=oa.PQEQ_SICNP if spec.get("pqeq") else None, **kw)
        tr = TorchTransport(mode="staged", device=torch.device("cuda", 0), capacity_doubles=1 << 21)
        tr.attach(e)
        e.set_atoms_rxff(rec10(ranks[rank], None if vs is None else vs[rank]))
        if spec.get("f32"):
            e.set_qeq_precision(32)
        res = {}
        buf = torch.zeros(8, dtype=torch.int64, device="cuda:0"); p = buf.data_ptr()
        e.QEq()
        for r_cut in (6.5, 0.0):                                      # the list of a QEq call alone
            for name, arr in zip(("cnt", "E", "src", "dst", "vec", "hval"), _pairs(e, r_cut, pg)):
                res["q_pd%.3f_%s" % (r_cut, name)] = arr
        pe = e.FORCE()
        res["codes"] = np.array([_code(lambda: e.bonds_device(0, 0, 0, 0)), _code(lambda: e.bonds_device(8, p, p, p)),
                                 _code(lambda: e.pairs_device(0, 0, 0)), _code(lambda: e.pairs_device(8, p, p)),
                                 _code(lambda: e.pairs_device(8, p, p, shift_ptr=p, as_gid=True))])
        res["refused_calls_wrote_nothing"] = bool((buf == 0).all().item())
        res["maxrc"] = e.cutoffs()[1]
        res["qeq_precision"] = np.array(e.qeq_precision())
        _state(e, spec["cuts"], "s0_", res, pg, bg)
        if spec.get("steps"):
            e.step(spec["steps"])
            _state(e, spec["cuts_after"], "s1_", res, pg, bg)
        res["transport"] = np.array([tr.n_exchange, tr.n_allreduce]); res["transport_error"] = repr(tr.error)
        np.savez(os.path.join(spec["dir"], "rank%d.npz" % rank), **res)
        out[rank] = dict(ok=True)
        e.close()
        dist.barrier(); dist.destroy_process_group()
    except Exception:
        out[rank] = dict(error=traceback.format_exc())
