// bonded_common.h -- what the units of the bonded terms share (bonded.hip, angles.hip, torsions.hip, hbonds.hip): the constants of the reference's
// module.F90, the block-level energy sum, and the derivative of an angle's cosine.
#pragma once
#include "engine.h"

namespace rxmd {

static constexpr double MINBO0 = 1e-4, cutof2_esub = 1e-4;                                        // module.F90:61-62
static constexpr double MAXANGLE = 0.999999999999, MINANGLE = -0.999999999999, NSMALL = 1e-10;   // module.F90:85-87
static constexpr double PI_ = 3.14159265358979;                                                  // module.F90:90

// sum over the block, then one atomic per block into the energy accumulator
__device__ inline void block_energy_add(double v, double *dst) {
  __shared__ double sm[8];
  v = wave_sum64(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < (blockDim.x >> 6); ++k) s += sm[k];
    if (s != 0.0) atomicAdd(dst, s);
  }
}
__device__ inline double ipow7(double a) { const double a2 = a * a, a4 = a2 * a2; return (a * a2) * a4; }

struct V3 { double x, y, z; };
__device__ inline double dot(const V3 &a, const V3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// derivative of cos(i,j,k) (ForceA3, pot.F90:1462-1521): forces on i and on k; j gets -(fi+fk)
__device__ inline void angle_forces(double coeff, const V3 &rij, double nij, const V3 &rjk, double njk, V3 &fi, V3 &fk) {
  const double C00 = nij * nij, C01 = dot(rij, rjk), C11 = njk * njk;
  const double coCC = coeff * (1.0 / (nij * njk));
  const double Ci1 = -(C01 / C00), Ck2 = C01 / C11;
  fi.x = coCC * (Ci1 * rij.x + rjk.x); fi.y = coCC * (Ci1 * rij.y + rjk.y); fi.z = coCC * (Ci1 * rij.z + rjk.z);
  // fjk = -coCC*(Ck1*rij + Ck2*rjk), Ck1 = -1 ; force on k is -fjk
  fk.x = coCC * (-rij.x + Ck2 * rjk.x); fk.y = coCC * (-rij.y + Ck2 * rjk.y); fk.z = coCC * (-rij.z + Ck2 * rjk.z);
}

constexpr int WSLOT = 31;   // bonded slots a wavefront-per-centre kernel stages in LDS (MAXNEIGHBS = 30; slot 31 = the centre atom itself)

}  // namespace rxmd
