"""A Berendsen barostat around the lattice-changing oracle, in plain numpy (TEST INFRASTRUCTURE: no GPU import).

It restates the documented rule of rxmd_hip_set_barostat, not the kernel: on a step whose TOTAL MD step count becomes a multiple
of `every` the step's own stress sums (astr after the step minus astr at its head: this step's virial plus m v v) over the volume of the
lattice the step ran at, times 6.94728103, are the pressure tensor [GPa]; mu_k = clip(cbrt(1 - every dt / tau (p0 - P) / B), 1 +- max_strain)
(mode 1: P the mean of the three diagonals, p0[0], one mu; mode 2: per axis, mu = 1 where the `axes` bit is clear); the lengths are multiplied
by mu, the angles kept, and the oracle is set to the new lattice (Oracle.set_lattice: normalised coordinates kept, the next half-kick uses
the forces of the old box)."""
import numpy as np

GPA = 6.94728103          # main.F90:252


def volume(lat):
    a, b, c = lat[:3]
    ca, cb, cg = np.cos(np.radians(lat[3:6]))
    return a * b * c * np.sqrt(1.0 - ca * ca - cb * cb - cg * cg + 2.0 * ca * cb * cg)


def hmat(lat):
    """GetBoxParams (init.F90:610-633): columns are the lattice vectors"""
    la, lb, lc = lat[:3]
    al, be, ga = np.radians(lat[3:6])
    hh1 = lc * (np.cos(al) - np.cos(be) * np.cos(ga)) / np.sin(ga)
    hh2 = lc * np.sqrt(1.0 - np.cos(al) ** 2 - np.cos(be) ** 2 - np.cos(ga) ** 2 + 2 * np.cos(al) * np.cos(be) * np.cos(ga)) / np.sin(ga)
    return np.array([[la, lb * np.cos(ga), lc * np.cos(be)], [0.0, lb * np.sin(ga), hh1], [0.0, 0.0, hh2]])


def remap_matrix(lat_old, lat_new):
    """M = H' H^-1: r' = M r keeps the normalised coordinates"""
    return hmat(lat_new) @ np.linalg.inv(hmat(lat_old))


def mu_np(p6, mode, p0, rate, B, max_strain, axes=7):
    mu = np.ones(3)
    for k in range(3):
        if mode == 1:
            mu[k] = np.cbrt(1.0 - rate * (p0[0] - (p6[0] + p6[1] + p6[2]) / 3.0) / B)
        elif (axes >> k) & 1:
            mu[k] = np.cbrt(1.0 - rate * (p0[k] - p6[k]) / B)
    return np.clip(mu, 1.0 - max_strain, 1.0 + max_strain)


def berendsen_run(oracle, lattice, nsteps, mode, p0, tau_fs, bulk, every=1, max_strain=0.01, axes=7, dt_fs=0.25, steps_done=0):
    """nsteps MD steps of `oracle` (which stands at `lattice` and has taken `steps_done` steps) under the barostat.
    Returns (final lattice, [dict(step, lat, new, p6, mu) per coupling]); step is the total MD step count at the coupling."""
    p0 = [float(p0)] * 3 if np.isscalar(p0) else [float(x) for x in p0]
    lat = [float(x) for x in lattice]
    rows = []
    for s in range(nsteps):
        total = steps_done + s + 1
        if total % every != 0:
            oracle.step(1)
            continue
        head = oracle.astr(reset=False)
        oracle.step(1)
        p6 = (oracle.astr(reset=False) - head) / volume(lat) * GPA
        mu = mu_np(p6, mode, p0, every * dt_fs / tau_fs, bulk, max_strain, axes)
        new = [lat[k] * mu[k] for k in range(3)] + lat[3:]
        oracle.set_lattice(new)
        rows.append(dict(step=total, lat=lat, new=new, p6=p6, mu=mu))
        lat = new
    return lat, rows
