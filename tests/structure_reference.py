"""The yardstick of the structure statistics (TEST INFRASTRUCTURE, shared by test_structure_host.py, test_gpu_structure.py and its worker): the brute
force over all images of test_gpu_pair_graph.py, binned in numpy by the formulas of include/rxmd_hip.h.

Rounding can move a sample across a bin edge or a cut-off.  Both sides subtract coordinates below 45 A, so r is good to about 5e-14 A and a bin
coordinate to about 1e-11.  A sample is NEAR AN EDGE when its bin coordinate (r nbins_r / r_max, theta nbins_angle / 180) lies within 1e-9 of an
integer, or |cos| > 1 - 1e-12 (acos loses the digits there); distances within 1e-8 A of r_max or of a shell cut are refused outright (`gap`).
The rules the tests hold the device to (check_counts):
  * L1 distance between a device array and its brute-force array <= 2 x the near-edge INCREMENTS of that array (a moved sample takes 1 from one
    counter and adds 1 to another; an angle sample increments two counters in every shell it is booked in);
  * the sums over the bins per type pair, and per shell and type triple, are exact;
  * on disordered boxes the near-edge share is at most 1e-5 of the samples, so that the L1 rule cannot hide a failure."""
import numpy as np

EDGE_TOL = 1e-9          # bin coordinate to the nearest integer
COS_TOL = 1e-12          # 1 - |cos|
GAP_TOL = 1e-8           # A, distance to r_max or a shell cut
SHARE_CAP = 1e-5         # near-edge samples / samples on a disordered box

R_MAX, NBINS_R, SHELLS, NBINS_A = 9.5, 190, (2.0, 4.0, 6.0), 180     # the binning of the shape tests


def host_positions(case):
    """(pos [n, 3], type0 [n], lattice, nso) of an off-lattice system WITHOUT an engine: rnorm times the H matrix (what set_atoms_rxff computes)"""
    import offlattice_systems as ol
    import oracle_api as oa
    from npt_reference import hmat
    ff, lat2, ranks, v = ol.build(case)
    pos = ranks[0]["rnorm"] @ hmat(lat2).T
    return pos, np.asarray(ranks[0]["type"], np.int64) - 1, lat2, len(oa.ffield_names(ff))


def bin_pairs(bf, type0, nso, r_max, nbins_r):
    """-> dict(counts [nso, nso, nbins_r], samples, near (near-edge increments), gap (smallest |r - r_max|))"""
    keys, vecs, dist = bf
    sel = dist < r_max
    x = dist[sel] * nbins_r / r_max
    k = np.minimum(x.astype(np.int64), nbins_r - 1)
    a, b = type0[keys[sel, 0]], type0[keys[sel, 1]]
    counts = np.bincount((a * nso + b) * nbins_r + k, minlength=nso * nso * nbins_r).reshape(nso, nso, nbins_r).astype(np.int64)
    near = int((np.abs(x - np.rint(x)) < EDGE_TOL).sum())
    return dict(counts=counts, samples=int(sel.sum()), near=near, gap=float(np.abs(dist - r_max).min()) if len(dist) else np.inf)


def bin_angles(bf, type0, nso, cuts, nbins_a):
    """-> dict(counts [nshells, nso, nso, nso, nbins_a], samples [nshells] (unordered pairs inside each shell), near (near-edge increments of the
    array), near_samples [nshells], gap (smallest |r - cut| over the cuts))"""
    keys, vecs, dist = bf
    cuts = np.asarray(cuts, np.float64)
    nsh = len(cuts)
    gap = min(float(np.abs(dist - c).min()) for c in cuts) if len(dist) else np.inf
    sel = dist < cuts[-1]
    src, dst, d = keys[sel, 0], keys[sel, 1], dist[sel]
    u = vecs[sel] / d[:, None]
    shell = np.searchsorted(cuts, d, side="right")             # the first l with d < cuts[l]
    n = len(type0)
    start = np.searchsorted(src, np.arange(n + 1))             # (the brute force is sorted by src)
    size = nsh * nso ** 3 * nbins_a
    exact = np.zeros(size, np.int64)                           # booked at max(l_j, l_k) only; the shells above follow by a running sum
    near_exact = np.zeros(nsh, np.int64); samples_exact = np.zeros(nsh, np.int64)
    for i in range(n):
        s, e = start[i], start[i + 1]
        if e - s < 2:
            continue
        ju, ku = np.triu_indices(e - s, 1)
        c = (u[s:e] @ u[s:e].T)[ju, ku]
        theta = np.arccos(np.clip(c, -1.0, 1.0)) * 180.0 / np.pi
        x = theta * nbins_a / 180.0
        m = np.minimum(x.astype(np.int64), nbins_a - 1)
        l = np.maximum(shell[s:e][ju], shell[s:e][ku])
        tj, tk, ti = type0[dst[s:e]][ju], type0[dst[s:e]][ku], type0[i]
        exact += np.bincount((((l * nso + tj) * nso + ti) * nso + tk) * nbins_a + m, minlength=size)
        exact += np.bincount((((l * nso + tk) * nso + ti) * nso + tj) * nbins_a + m, minlength=size)
        nearf = (np.abs(x - np.rint(x)) < EDGE_TOL) | (np.abs(c) > 1.0 - COS_TOL)
        near_exact += np.bincount(l[nearf], minlength=nsh)
        samples_exact += np.bincount(l, minlength=nsh)
    counts = np.cumsum(exact.reshape(nsh, nso, nso, nso, nbins_a), axis=0)
    near = int(sum(2 * (nsh - l) * near_exact[l] for l in range(nsh)))
    return dict(counts=counts, samples=np.cumsum(samples_exact), near=near, near_samples=np.cumsum(near_exact), gap=gap)


def check_counts(label, got_pair, got_angle, ref_pair, ref_angle, disordered):
    """the rules of this module's docstring; ref_angle None: no shells.  Prints every figure before it asserts."""
    l1p = int(np.abs(got_pair - ref_pair["counts"]).sum())
    print("%s pairs: samples %d, near-edge increments %d, gap to r_max %.2e A, L1(device, brute force) %d" % (label, ref_pair["samples"], ref_pair["near"], ref_pair["gap"], l1p))
    assert ref_pair["gap"] > GAP_TOL, "a distance lies within 1e-8 A of r_max"
    assert got_pair.shape == ref_pair["counts"].shape
    assert np.array_equal(got_pair.sum(axis=2), ref_pair["counts"].sum(axis=2)), "the pair counts per type pair differ"
    assert l1p <= 2 * ref_pair["near"]
    if disordered:
        assert ref_pair["near"] <= SHARE_CAP * ref_pair["samples"]
    if ref_angle is None:
        return
    l1a = int(np.abs(got_angle - ref_angle["counts"]).sum())
    print("%s angles: samples per shell %s, near-edge per shell %s, near-edge increments %d, gap to a cut %.2e A, L1(device, brute force) %d"
          % (label, list(ref_angle["samples"]), list(ref_angle["near_samples"]), ref_angle["near"], ref_angle["gap"], l1a))
    assert ref_angle["gap"] > GAP_TOL, "a distance lies within 1e-8 A of a shell cut"
    assert got_angle.shape == ref_angle["counts"].shape
    assert np.array_equal(got_angle.sum(axis=-1), ref_angle["counts"].sum(axis=-1)), "the angle counts per shell and type triple differ"
    assert l1a <= 2 * ref_angle["near"]
    if disordered:
        assert ref_angle["near_samples"][-1] <= SHARE_CAP * ref_angle["samples"][-1]
