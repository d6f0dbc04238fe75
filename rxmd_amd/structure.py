"""Normalisation of the structure statistics an engine accumulates on the device (RxmdEngine.structure_counts, include/rxmd_hip.h:
rxmd_hip_structure_*): partial pair distributions g_ab(r), running coordination n_ab(r), partial structure factors S_ab(q) and bond-angle
distributions, as pure functions of the counts dict.  numpy only: no GPU, no torch.

The formulas are those of the reference's offline analysis (util/stat/stat.f90:162-250, 266-283) with two deliberate differences:
  * the density uses the MEAN TRUE volume of the sampled frames (volume_sum / frames); the reference multiplies the three lattice lengths of one
    frame, which is the volume of an orthorhombic cell only;
  * bin k stands for its centre r = (k + 0.5) dr; the reference evaluates the shell volume and the r-integral at k dr, the bin's upper edge.
The reference's num_atoms_per_type * num_sample_frames is atoms_per_type here (the device sums the residents of every sample), so a run whose
composition changes between samples is normalised by what was actually sampled.  angle_counts is twice the reference's table ba (it books 0.5
each way); the normalised distribution is a ratio and does not see the factor.  A type that is absent from the run gives rows of zeros, never NaN.

A decomposed run has one dict per rank: sum them first with merge()."""
import numpy as np

_SUMMED = ("pair_counts", "angle_counts", "atoms_per_type")


def merge(dicts):
    """the dicts of the ranks of ONE run (same binning, same samples) -> the dict of the whole box: counts and atoms_per_type are summed; volume_sum
    and frames are those of the whole box on every rank and are taken from the first"""
    dicts = list(dicts)
    if not dicts:
        raise ValueError("merge: no dicts")
    out = dict(dicts[0])
    for key in _SUMMED:
        out[key] = np.array(dicts[0][key], dtype=np.int64, copy=True)
    for d in dicts[1:]:
        if d["frames"] != out["frames"] or d["r_max"] != out["r_max"] or list(d["angle_cuts"]) != list(out["angle_cuts"]):
            raise ValueError("merge: the dicts are not of one run (frames, r_max or angle_cuts differ)")
        for key in _SUMMED:
            if np.shape(d[key]) != out[key].shape:
                raise ValueError("merge: %s has another shape" % key)
            out[key] += d[key]
    return out


def _safe_div(num, den):
    num = np.asarray(num, np.float64); den = np.broadcast_to(np.asarray(den, np.float64), num.shape)
    out = np.zeros(num.shape)
    np.divide(num, den, out=out, where=den > 0)
    return out


def _basics(c):
    pair = np.asarray(c["pair_counts"], np.float64)
    npt = np.asarray(c["atoms_per_type"], np.float64)          # residents of each type summed over the samples = N_a * frames
    nbr = pair.shape[2]
    dr = float(c["r_max"]) / nbr
    ntot = npt.sum()
    conc = npt / ntot if ntot > 0 else np.zeros_like(npt)      # stat.f90:335
    rho = ntot / c["volume_sum"] if c["volume_sum"] > 0 else 0.0   # (sum N / frames) / (sum V / frames), stat.f90:144 with the mean true volume
    return pair, npt, conc, rho, dr


def r_centres(c):
    """bin centres (k + 0.5) dr [A]"""
    nbr = np.shape(c["pair_counts"])[2]
    return (np.arange(nbr) + 0.5) * (float(c["r_max"]) / nbr)


def g_ab(c):
    """partial pair distribution g_ab(r_k), [nso, nso, nbins_r]: counts / (prefactor * prefactor2), prefactor = 4 pi r^2 dr rho (the ideal-gas
    count of a shell), prefactor2 = c_b N_a frames (stat.f90:176-184)"""
    pair, npt, conc, rho, dr = _basics(c)
    prefactor = 4.0 * np.pi * r_centres(c) ** 2 * dr * rho
    prefactor2 = conc[None, :] * npt[:, None]
    return _safe_div(pair, prefactor[None, None, :] * prefactor2[:, :, None])


def n_ab(c):
    """running coordination number n_ab up to the UPPER edge of bin k, [nso, nso, nbins_r]: the running sum of the counts per atom of type a and
    sample (stat.f90:166-171)"""
    pair, npt, conc, rho, dr = _basics(c)
    return _safe_div(np.cumsum(pair, axis=2), npt[:, None, None])


def s_ab(c, q):
    """partial structure factor S_ab(q) for wave numbers q [1/A], [nso, nso, len(q)]: delta_ab + 4 pi rho sqrt(c_a c_b) sum_k r^2 (g_ab - 1)
    sin(q r) / (q r) dr over the sampled range (stat.f90:216-250).  A pair of types with an absent member gives zeros."""
    pair, npt, conc, rho, dr = _basics(c)
    q = np.atleast_1d(np.asarray(q, np.float64))
    r = r_centres(c)
    g = g_ab(c)
    kernel = r[None, :] ** 2 * np.sinc(np.outer(q, r) / np.pi) * dr          # [q, k]; np.sinc(x) = sin(pi x) / (pi x): the q -> 0 limit is exact
    integral = np.einsum("abk,qk->abq", g - 1.0, kernel)
    s = 4.0 * np.pi * rho * np.sqrt(np.outer(conc, conc))[:, :, None] * integral
    s += np.eye(len(npt))[:, :, None]
    present = (npt > 0)[:, None] & (npt > 0)[None, :]
    return np.where(present[:, :, None], s, 0.0)


def angle_centres(c):
    """bin centres of the angle histogram [degrees]"""
    nba = np.shape(c["angle_counts"])[-1]
    return (np.arange(nba) + 0.5) * (180.0 / nba)


def angle_distribution(c):
    """normalised bond-angle distributions, [nshells, nso, nso, nso, nbins_angle] indexed (shell, end j, centre i, end k, bin): the counts of a
    (shell, triple) divided by their sum over the bins and by N_i frames, the reference's normalisation (stat.f90:266-283); a triple that never
    occurred gives zeros"""
    ang = np.asarray(c["angle_counts"], np.float64)
    npt = np.asarray(c["atoms_per_type"], np.float64)
    if ang.size == 0:
        return ang.copy()
    total = ang.sum(axis=-1, keepdims=True)
    return _safe_div(ang, total * npt[None, None, :, None, None])
