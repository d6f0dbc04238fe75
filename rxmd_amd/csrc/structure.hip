// structure.hip -- rxmd_hip_structure_*: structure statistics of a live engine, accumulated on the device from the 10 A list of the last build:
// partial pair counts per (type, type, r bin) -- from which rxmd_amd/structure.py forms g_ab(r), n_ab(r), S_ab(q) -- and bond-angle counts per
// (shell, type, centre type, type, angle bin).  The reference does this offline (util/stat: reads XYZ frames, builds its own voxel list on the CPU);
// here the list is already on the device, the kernels only READ it (pair_walk.h: the row walk of the pair graph) and write int64 counters.
// Nothing here is on the path of qeq(), force() or step(); an engine that never calls structure_begin allocates and launches nothing.
//
// Three launches per sample, on the engine's stream:
//   k_struct_types   residents per type -> ntype[nso] (accumulated like everything else).  The other two kernels read it: the types with ntype > 0
//                    are the PRESENT types, numbered 0 .. np - 1 (TypeMap), and the LDS histograms are laid out over those -- an ffield names
//                    more types than a run uses (ffield_rdx: 7, RDX: 4).  A ghost partner of a type no resident of this rank ever had is not
//                    in the map: its increments go to global memory one by one.
// One wavefront per resident row in the other two; a persistent grid of two workgroups per CU, each over a contiguous chunk of rows, counts into
// 32-bit LDS histograms and flushes them ONCE with 64-bit global atomic adds (integers only: the counts do not depend on order, grid or layout).
//   k_struct_pairs   entry -> partner j -> r = sqrt(d.d) (the expression of k_pair_count) -> r < r_max: LDS[(a - a0, b, k)] += 1, a = present type of
//                    the row (wave-uniform), b = of the partner, k = (int)(r nbins_r / r_max).  The LDS holds SP_HCAP counters = the slices [b][k]
//                    of as many row types a as fit (4 present types x 1000 bins: all 16 slices, 64,000 bytes); with more, the workgroup walks its
//                    chunk once per group of row types and skips the rows of the others (a skipped row costs one type read); when not even ONE
//                    slice fits (np nbins_r > SP_HCAP) every increment is a global atomic.
//   k_struct_angles  per row the entries inside the largest shell are compacted, in list order, into LDS tiles of SA_TILE (unit vector, shell
//                    index = first l with r < cut[l], type); all pairs j < k inside a tile, and all pairs of tile A with every later tile B (filled
//                    by walking the row again: one walk when the shell holds <= SA_TILE neighbours, the usual case).  A pair is counted ONCE in
//                    LDS at (max(l_j, l_k), t_j, t_k, m); the flush adds the count to both (t_j, t_i, t_k) and (t_k, t_i, t_j) of every shell from
//                    that one up.  The LDS holds SA_HCAP counters = the slices [l][t_j][t_k][m] of as many centre types as fit (3 shells x 4 x 4
//                    present types x 180 bins = 8,640: one), walked as above; no slice fits: global atomics per pair.
// A workgroup's chunk is bounded so that no 32-bit counter can overflow (Engine::structure_sample).
#include "pair_walk.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace rxmd {

constexpr int SG_MAXSHELLS = 4;
constexpr int SG_MAXTYPES = 16;                   // (the engine refuses an ffield with more than 15 types: the packed 10 A list entry)
constexpr int SP_WAVES = 16, SP_HCAP = 16000;     // pair pass: rows (wavefronts) of a workgroup; 32-bit LDS counters (64,000 bytes: two workgroups per CU)
constexpr int SA_WAVES = 4, SA_TILE = 128, SA_HCAP = 8704;   // angle pass: rows of a workgroup; staged neighbours per tile (two tiles per row); LDS counters
static_assert(SP_HCAP * 4 + 3 * SG_MAXTYPES * 4 <= 65536, "the pair pass keeps its histogram in 64 KB of LDS");
static_assert(SA_WAVES * 2 * SA_TILE * (3 * 8 + 4) + SA_HCAP * 4 + 3 * SG_MAXTYPES * 4 <= 65536, "the angle pass keeps its tiles and its histogram in 64 KB of LDS");

struct StructArgs {                               // by value
  int nso, nbr, nsh, nba;
  double rmax, cut[SG_MAXSHELLS];
  const int *type;                                // 1-based ffield type per atom slot, ghosts included
  unsigned long long *pair, *angle, *ntype;       // [nso][nso][nbr], [nsh][nso][nso][nso][nba], [nso]
};

struct PairRow { int n; size_t row; const int *wk; double xi, yi, zi; };   // a row's length, its place in the streams, its group's window, its atom
__device__ inline PairRow pair_row(const PairList &L, int i) {              // (the set-up of k_pair_count)
  PairRow R;
  R.n = min(L.n10[i] & N10_COUNT, L.S10);
  const int place = (L.byplace || L.slots) ? L.rpos[i] : 0;
  R.row = static_cast<size_t>(L.byplace ? place : i) * L.S10;
  R.wk = L.slots ? L.win_k + static_cast<size_t>(place / WIN_ROWS) * WIN_MAXUNITS : nullptr;
  R.xi = L.x[i]; R.yi = L.y[i]; R.zi = L.z[i];
  return R;
}
__device__ inline int type0(const StructArgs &A, int j) { return min(max(A.type[j] - 1, 0), A.nso - 1); }   // 0-based, clamped: it indexes the counters

__global__ void __launch_bounds__(256) k_struct_types(int N, StructArgs A) {
  __shared__ unsigned tc[SG_MAXTYPES];
  if (threadIdx.x < SG_MAXTYPES) tc[threadIdx.x] = 0;
  __syncthreads();
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < N; i += 256LL * gridDim.x) atomicAdd(&tc[type0(A, static_cast<int>(i))], 1u);
  __syncthreads();
  if (threadIdx.x < A.nso && tc[threadIdx.x]) atomicAdd(&A.ntype[threadIdx.x], static_cast<unsigned long long>(tc[threadIdx.x]));
}

// the present types of this rank, in LDS: cmap[type] = its number or -1, cinv[number] = type
struct TypeMap { int np, cmap[SG_MAXTYPES], cinv[SG_MAXTYPES]; };
__device__ inline void build_type_map(const StructArgs &A, TypeMap &T) {     // ends with a barrier
  if (threadIdx.x == 0) {
    int np = 0;
    for (int t = 0; t < SG_MAXTYPES; ++t) {
      const bool present = t < A.nso && A.ntype[t] > 0;
      T.cmap[t] = present ? np : -1;
      if (present) T.cinv[np++] = t;
    }
    T.np = np;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(64 * SP_WAVES) k_struct_pairs(PairList L, StructArgs A, int chunk) {
  __shared__ unsigned h[SP_HCAP];
  __shared__ TypeMap T;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const long long first = static_cast<long long>(blockIdx.x) * chunk;
  const int r0 = static_cast<int>(min(first, static_cast<long long>(L.N))), r1 = static_cast<int>(min(first + chunk, static_cast<long long>(L.N)));
  for (int t = threadIdx.x; t < SP_HCAP; t += 64 * SP_WAVES) h[t] = 0;
  build_type_map(A, T);
  const int np = T.np, slice = np * A.nbr;                    // a row type's counters: [present partner type][bin]
  const bool lds = slice > 0 && slice <= SP_HCAP;
  const int na_pass = lds ? min(SP_HCAP / slice, np) : max(np, 1);   // row types per walk (no LDS: one walk)
  const double scale = static_cast<double>(A.nbr);
  for (int a0 = 0; a0 < np; a0 += na_pass) {
    const int na = min(na_pass, np - a0);
    for (int i = r0 + w; i < r1; i += SP_WAVES) {
      const int a = __builtin_amdgcn_readfirstlane(type0(A, i));
      const int ca = T.cmap[a];                                // (a resident's type is present: k_struct_types counted it)
      if (ca < a0 || ca >= a0 + na) continue;                  // this row's type belongs to another walk
      const PairRow R = pair_row(L, i);
      unsigned *hl = h + (lds ? (ca - a0) * slice : 0);
      unsigned long long *hg = A.pair + static_cast<size_t>(a) * A.nso * A.nbr;
      for (int c0 = 0; c0 < R.n; c0 += 64) {
        const int kk = c0 + lane;
        if (kk >= R.n) continue;
        const int j = L.perm[pair_partner_pos(L, R.row, R.wk, kk)];
        const double d0 = L.x[j] - R.xi, d1 = L.y[j] - R.yi, d2 = L.z[j] - R.zi;
        const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        if (!(r < A.rmax)) continue;
        const int k = min(static_cast<int>(r * scale / A.rmax), A.nbr - 1);   // (the min only guards the array against a quotient rounded up to nbr)
        const int b = type0(A, j), cb = T.cmap[b];
        if (lds && cb >= 0) atomicAdd(&hl[cb * A.nbr + k], 1u); else atomicAdd(&hg[b * A.nbr + k], 1ULL);
      }
    }
    __syncthreads();
    if (lds)                                                   // (a thread clears what it flushed: the next walk starts from zeros)
      for (int t = threadIdx.x; t < na * slice; t += 64 * SP_WAVES) {
        const unsigned c = h[t];
        if (!c) continue;
        h[t] = 0;
        const int a = T.cinv[a0 + t / slice], b = T.cinv[(t % slice) / A.nbr], k = t % A.nbr;
        atomicAdd(&A.pair[(static_cast<size_t>(a) * A.nso + b) * A.nbr + k], static_cast<unsigned long long>(c));
      }
    __syncthreads();
  }
}

// ---- angles ----------------------------------------------------------------------------------------------------------------------------------
struct AngleTile { double *ux, *uy, *uz; int *code; };        // one wavefront's tile in LDS; code = shell index << 16 | type << 8 | present number (0xff: none)

// walks the whole row; the entries inside the largest shell get consecutive numbers in list order, those numbered [lo, lo + SA_TILE) are staged.
// Returns how many the shell holds (wave-uniform)
__device__ inline int stage_tile(const PairList &L, const StructArgs &A, const TypeMap &T, const PairRow &R, int lane, int lo, const AngleTile &S) {
  const double cmax = A.cut[A.nsh - 1];
  int base = 0;
  for (int c0 = 0; c0 < R.n; c0 += 64) {
    const int kk = c0 + lane;
    bool in = false;
    int j = 0;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, r = 0.0;
    if (kk < R.n) {
      j = L.perm[pair_partner_pos(L, R.row, R.wk, kk)];
      d0 = L.x[j] - R.xi; d1 = L.y[j] - R.yi; d2 = L.z[j] - R.zi;
      r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      in = r < cmax && r > 0.0;                                // (r = 0: two atoms on one point have no direction)
    }
    const unsigned long long m = __ballot(in);
    if (in) {
      const int s = base + __popcll(m & ((1ULL << lane) - 1ULL)) - lo;
      if (s >= 0 && s < SA_TILE) {
        int l = 0;
        while (l < A.nsh - 1 && !(r < A.cut[l])) ++l;
        const int t = type0(A, j);
        S.ux[s] = d0 / r; S.uy[s] = d1 / r; S.uz[s] = d2 / r;
        S.code[s] = (l << 16) | (t << 8) | (T.cmap[t] & 0xff);
      }
    }
    base += __popcll(m);
  }
  wave_lds_sync();
  return base;
}

// hl: the LDS slice of this row's centre type, or nullptr: global atomics
__device__ inline void book_angle(const StructArgs &A, unsigned *hl, int np, int ti, double c, int cj, int ck) {
  c = fmin(fmax(c, -1.0), 1.0);
  const double theta = acos(c) * 180.0 / 3.14159265358979323846;
  const int m = min(static_cast<int>(theta * A.nba / 180.0), A.nba - 1);
  const int l = max(cj >> 16, ck >> 16), pj = cj & 0xff, pk = ck & 0xff;
  if (hl && pj != 0xff && pk != 0xff) { atomicAdd(&hl[((l * np + pj) * np + pk) * A.nba + m], 1u); return; }
  const int tj = (cj >> 8) & 0xff, tk = (ck >> 8) & 0xff;
  for (int l2 = l; l2 < A.nsh; ++l2) {
    atomicAdd(&A.angle[(((static_cast<size_t>(l2) * A.nso + tj) * A.nso + ti) * A.nso + tk) * A.nba + m], 1ULL);
    atomicAdd(&A.angle[(((static_cast<size_t>(l2) * A.nso + tk) * A.nso + ti) * A.nso + tj) * A.nba + m], 1ULL);
  }
}

__global__ void __launch_bounds__(64 * SA_WAVES) k_struct_angles(PairList L, StructArgs A, int chunk) {
  __shared__ double su[SA_WAVES][2][3][SA_TILE];
  __shared__ int sc[SA_WAVES][2][SA_TILE];
  __shared__ unsigned h[SA_HCAP];
  __shared__ TypeMap T;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const long long first = static_cast<long long>(blockIdx.x) * chunk;
  const int r0 = static_cast<int>(min(first, static_cast<long long>(L.N))), r1 = static_cast<int>(min(first + chunk, static_cast<long long>(L.N)));
  const AngleTile TA{su[w][0][0], su[w][0][1], su[w][0][2], sc[w][0]}, TB{su[w][1][0], su[w][1][1], su[w][1][2], sc[w][1]};
  for (int t = threadIdx.x; t < SA_HCAP; t += 64 * SA_WAVES) h[t] = 0;
  build_type_map(A, T);
  const int np = T.np, slice = A.nsh * np * np * A.nba;       // a centre type's counters: [shell][present end type][present end type][bin]
  const bool lds = slice > 0 && slice <= SA_HCAP;
  const int na_pass = lds ? min(SA_HCAP / slice, np) : max(np, 1);
  for (int a0 = 0; a0 < np; a0 += na_pass) {
    const int na = min(na_pass, np - a0);
    for (int i = r0 + w; i < r1; i += SA_WAVES) {
      const int ti = __builtin_amdgcn_readfirstlane(type0(A, i));
      const int ci = T.cmap[ti];
      if (ci < a0 || ci >= a0 + na) continue;
      const PairRow R = pair_row(L, i);
      unsigned *hl = lds ? h + (ci - a0) * slice : nullptr;
      const int M = stage_tile(L, A, T, R, lane, 0, TA);
      const int nt = (M + SA_TILE - 1) / SA_TILE;
      for (int ta = 0; ta < nt; ++ta) {
        if (ta > 0) stage_tile(L, A, T, R, lane, ta * SA_TILE, TA);
        const int ca = min(SA_TILE, M - ta * SA_TILE);
        for (int j = 0; j + 1 < ca; ++j) {                     // pairs inside tile A: j wave-uniform, k across the lanes
          const double ux = TA.ux[j], uy = TA.uy[j], uz = TA.uz[j];
          const int cj = TA.code[j];
          for (int k = j + 1 + lane; k < ca; k += 64) book_angle(A, hl, np, ti, ux * TA.ux[k] + uy * TA.uy[k] + uz * TA.uz[k], cj, TA.code[k]);
        }
        for (int tb = ta + 1; tb < nt; ++tb) {                 // pairs of tile A with a later tile
          wave_lds_sync();                                     // (the reads of tile B's last filling are done)
          stage_tile(L, A, T, R, lane, tb * SA_TILE, TB);
          const int cb = min(SA_TILE, M - tb * SA_TILE);
          for (int j = 0; j < ca; ++j) {
            const double ux = TA.ux[j], uy = TA.uy[j], uz = TA.uz[j];
            const int cj = TA.code[j];
            for (int k = lane; k < cb; k += 64) book_angle(A, hl, np, ti, ux * TB.ux[k] + uy * TB.uy[k] + uz * TB.uz[k], cj, TB.code[k]);
          }
        }
        wave_lds_sync();                                       // (before tile A is filled again)
      }
    }
    __syncthreads();
    if (lds)
      for (int t = threadIdx.x; t < na * slice; t += 64 * SA_WAVES) {
        const unsigned c = h[t];
        if (!c) continue;
        h[t] = 0;
        int rem = t;
        const int ti = T.cinv[a0 + rem / slice]; rem %= slice;
        const int m = rem % A.nba; rem /= A.nba;
        const int tk = T.cinv[rem % np]; rem /= np;
        const int tj = T.cinv[rem % np], l = rem / np;
        for (int l2 = l; l2 < A.nsh; ++l2) {                   // tj == tk: the same counter twice, 2 c in all
          atomicAdd(&A.angle[(((static_cast<size_t>(l2) * A.nso + tj) * A.nso + ti) * A.nso + tk) * A.nba + m], static_cast<unsigned long long>(c));
          atomicAdd(&A.angle[(((static_cast<size_t>(l2) * A.nso + tk) * A.nso + ti) * A.nso + tj) * A.nba + m], static_cast<unsigned long long>(c));
        }
      }
    __syncthreads();
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
void Engine::structure_begin(double r_max, int nbins_r, int nshells, const double *angle_cut, int nbins_angle) {
  if (!std::isfinite(r_max) || !(r_max > 0.0)) throw EngineError(RXMD_E_ARG, "structure_begin: r_max must be a positive finite number");
  if (r_max > ff.rctap) throw EngineError(RXMD_E_ARG, "structure_begin: r_max is beyond the reach of the list (" + std::to_string(ff.rctap) + " A, the taper cut-off)");
  if (nbins_r < 1 || nbins_r > 4096) throw EngineError(RXMD_E_ARG, "structure_begin: nbins_r must be in 1..4096");
  if (nshells < 0 || nshells > SG_MAXSHELLS) throw EngineError(RXMD_E_ARG, "structure_begin: nshells must be in 0..4");
  if (nshells > 0) {
    if (!angle_cut) throw EngineError(RXMD_E_ARG, "structure_begin: angle_cut is NULL");
    if (nbins_angle < 1 || nbins_angle > 360) throw EngineError(RXMD_E_ARG, "structure_begin: nbins_angle must be in 1..360");
    for (int l = 0; l < nshells; ++l)
      if (!std::isfinite(angle_cut[l]) || !(angle_cut[l] > (l ? angle_cut[l - 1] : 0.0)) || angle_cut[l] > r_max)
        throw EngineError(RXMD_E_ARG, "structure_begin: angle_cut must be strictly ascending with 0 < angle_cut[l] <= r_max");
  }
  if (ff.nso >= SG_MAXTYPES) throw EngineError(RXMD_E_ARG, "more than 15 atom types do not fit the packed 10 A list entry");   // (the message of set-up)
  const size_t nso = static_cast<size_t>(ff.nso);
  sg_on = false;
  sg_rmax = r_max; sg_nbr = nbins_r; sg_nsh = nshells; sg_nba = nshells > 0 ? nbins_angle : 0;
  for (int l = 0; l < SG_MAXSHELLS; ++l) sg_cut[l] = l < nshells ? angle_cut[l] : 0.0;
  sg_npair = nso * nso * nbins_r; sg_nangle = static_cast<size_t>(nshells) * nso * nso * nso * sg_nba;
  regrow_group(G_STRUCT, sg_npair + sg_nangle + nso);          // (Fill::Zero)
  RX_HIP(hipMemsetAsync(sg_acc, 0, (sg_npair + sg_nangle + nso) * sizeof(long long), stream));   // on the stream the kernels run on
  sg_volume = 0.0; sg_frames = 0;
  sg_on = true;
}

void Engine::structure_end() {
  if (!sg_on && !sg_acc) return;
  sync_stream();
  bufs.free_group(G_STRUCT);
  sg_on = false;
}

void Engine::structure_sample() {
  if (!sg_on) throw EngineError(RXMD_E_STATE, "structure_sample: no accumulators, call rxmd_hip_structure_begin first");
  if (!atoms_set || !lists_valid) throw EngineError(RXMD_E_STATE, "no 10 A list: call rxmd_hip_qeq or rxmd_hip_force first");
  if (force_pending) finish_force();
  if (N > 0) {
    if (!nb10_valid && !win_valid) require_nb10();
    StructArgs A;
    A.nso = ff.nso; A.nbr = sg_nbr; A.nsh = sg_nsh; A.nba = sg_nba; A.rmax = sg_rmax;
    for (int l = 0; l < SG_MAXSHELLS; ++l) A.cut[l] = sg_cut[l];
    A.type = type;
    A.pair = reinterpret_cast<unsigned long long *>(sg_acc); A.angle = A.pair + sg_npair; A.ntype = A.angle + sg_nangle;
    const PairList L = pair_list(0.0);
    // rows of a workgroup: two workgroups per CU, and few enough rows that a 32-bit LDS counter cannot overflow (a row adds at most S10 pair
    // counts, S10 (S10 - 1) / 2 angle counts)
    auto grid_of = [&](int waves, long long per_row, int &chunk) {
      long long c = (static_cast<long long>(N) + 2LL * num_cu - 1) / (2LL * num_cu);
      c = std::max<long long>((c + waves - 1) / waves * waves, waves);
      c = std::min(c, std::max<long long>(0xFFFFFFFFLL / std::max<long long>(per_row, 1), 1));
      chunk = static_cast<int>(c);
      return static_cast<int>((static_cast<long long>(N) + c - 1) / c);
    };
    int chunk = 0;
    k_struct_types<<<std::min(nblk(N, 256), 2 * num_cu), 256, 0, stream>>>(N, A);
    const int gp = grid_of(SP_WAVES, S10, chunk);
    k_struct_pairs<<<gp, 64 * SP_WAVES, 0, stream>>>(L, A, chunk);
    if (sg_nsh > 0) {
      const int ga = grid_of(SA_WAVES, static_cast<long long>(S10) * std::max(S10 - 1, 1) / 2, chunk);
      k_struct_angles<<<ga, 64 * SA_WAVES, 0, stream>>>(L, A, chunk);
    }
    RX_HIP(hipGetLastError());
  }
  sg_volume += box.volume; ++sg_frames;
}

void Engine::structure_get(long long *pair_counts, long long pair_capacity, long long *angle_counts, long long angle_capacity, long long *atoms_per_type,
                           double *volume_sum, long long *frames) {
  if (!sg_on) throw EngineError(RXMD_E_STATE, "structure_get: no accumulators, call rxmd_hip_structure_begin first");
  if (pair_counts && pair_capacity < static_cast<long long>(sg_npair)) throw EngineError(RXMD_E_ARG, "structure_get: pair_capacity is below nso * nso * nbins_r = " + std::to_string(sg_npair));
  if (angle_counts && angle_capacity < static_cast<long long>(sg_nangle)) throw EngineError(RXMD_E_ARG, "structure_get: angle_capacity is below nshells * nso^3 * nbins_angle = " + std::to_string(sg_nangle));
  sync_stream();
  if (pair_counts && sg_npair) RX_HIP(hipMemcpy(pair_counts, sg_acc, sg_npair * sizeof(long long), hipMemcpyDeviceToHost));
  if (angle_counts && sg_nangle) RX_HIP(hipMemcpy(angle_counts, sg_acc + sg_npair, sg_nangle * sizeof(long long), hipMemcpyDeviceToHost));
  if (atoms_per_type) RX_HIP(hipMemcpy(atoms_per_type, sg_acc + sg_npair + sg_nangle, static_cast<size_t>(ff.nso) * sizeof(long long), hipMemcpyDeviceToHost));
  if (volume_sum) *volume_sum = sg_volume;
  if (frames) *frames = sg_frames;
}

}  // namespace rxmd
