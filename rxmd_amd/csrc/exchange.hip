// exchange.hip -- COPYATOMS: the six-stage exchange of reference src/comm.F90 restated MI355X-first.  Ghost-atom build (MODE_COPY), migration
// (MODE_MOVE), vector halos (MODE_QCOPY1/2) and the ghost-force fold (MODE_CPBK): on one rank as 26 image segments, between ranks as a walk
// over rounds of one or two stages (select -> pack -> send_recv -> unpack); the direct vector halo.  The byte transport is rccl_comm.hip or
// the host's callbacks (rxmd_comm_ops).
#include "engine.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

namespace rxmd {

static const int cptridx_[7] = {0, 0, 0, 2, 2, 4, 4};  // comm.F90:61
static const int dinv_[7] = {0, 2, 1, 4, 3, 6, 5};     // comm.F90:60

// ---------------------------------------------------------------------------------------------
// kernels: coordinates, slab flags, append, halo
struct BoxDev { double H[9], Hi[9], obox[3], lbox[3]; };
static BoxDev boxdev(const Box &b) {
  const DevBox m = dev_box(b);
  BoxDev d;
  for (int k = 0; k < 9; ++k) { d.H[k] = m.H[k]; d.Hi[k] = m.Hi[k]; }
  for (int a = 0; a < 3; ++a) { d.obox[a] = b.obox[a]; d.lbox[a] = b.lbox[a]; }
  return d;
}

// xu2xs (reference src/main.F90:596-616): normalised local coordinates of atoms [i0,i1)
__global__ void k_to_normalised(BoxDev B, int i0, int i1, const double *x, const double *y, const double *z, double *sx, double *sy, double *sz) {
  const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= i1) return;
  const double r0 = x[i], r1 = y[i], r2 = z[i];
  sx[i] = (B.Hi[0] * r0 + B.Hi[1] * r1 + B.Hi[2] * r2) - B.obox[0];
  sy[i] = (B.Hi[3] * r0 + B.Hi[4] * r1 + B.Hi[5] * r2) - B.obox[1];
  sz[i] = (B.Hi[6] * r0 + B.Hi[7] * r1 + B.Hi[8] * r2) - B.obox[2];
}
// xs2xu (reference src/main.F90:641-660)
__global__ void k_to_real(BoxDev B, int i0, int i1, const double *sx, const double *sy, const double *sz, double *x, double *y, double *z) {
  const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= i1) return;
  const double r0 = sx[i] + B.obox[0], r1 = sy[i] + B.obox[1], r2 = sz[i] + B.obox[2];
  x[i] = B.H[0] * r0 + B.H[1] * r1 + B.H[2] * r2;
  y[i] = B.H[3] * r0 + B.H[4] * r1 + B.H[5] * r2;
  z[i] = B.H[6] * r0 + B.H[7] * r1 + B.H[8] * r2;
}

// inBuffer (reference src/comm.F90:551-576) over the scan range of one exchange stage
__global__ void k_slab_flags(int nscan, int dflag, double lbox, double dr, const double *s, const int *type, int skip_dead, int *flags) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n > nscan) return;
  int f = 0;
  if (n < nscan) {
    const double rr = s[n];
    f = (dflag & 1) ? (lbox - dr < rr) : (rr <= dr);
    if (skip_dead && type[n] <= 0) f = 0;
  }
  flags[n] = f;   // flags[nscan] = 0 so that scanout[nscan] is the total
}

// store_atoms + append_atoms for a self-exchange stage of MODE_COPY (reference src/comm.F90:367-453,456-528)
__global__ void k_append_ghosts(int nscan, int base, int N, int axis, double sft, const int *flags, const int *scanout,
                                double *sx, double *sy, double *sz, int *type, long long *gid, double *q, int *gsrc, int *groot, int *sendlist) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= nscan || !flags[n]) return;
  const int k = scanout[n], m = base + k;
  double a = sx[n], b = sy[n], c = sz[n];
  if (axis == 0) a += sft; else if (axis == 1) b += sft; else c += sft;
  sx[m] = a; sy[m] = b; sz[m] = c;
  type[m] = type[n]; gid[m] = gid[n]; q[m] = q[n];
  gsrc[m] = n; groot[m] = (n < N) ? n : groot[n];
  sendlist[k] = n;
}

__global__ void k_refresh2(int N, int G, const int *groot, double2 *v) {
  const int g = N + blockIdx.x * blockDim.x + threadIdx.x;
  if (g < G) v[g] = v[groot[g]];
}
__global__ void k_refresh1(int N, int G, const int *groot, double *v) {
  const int g = N + blockIdx.x * blockDim.x + threadIdx.x;
  if (g < G) v[g] = v[groot[g]];
}
// append_atoms for MODE_CPBK (reference src/comm.F90:474-482): one stage, sources are unique within a stage
__global__ void k_fold_stage(int g0, int g1, const int *gsrc, double *fx, double *fy, double *fz) {
  const int m = g0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= g1) return;
  const int n = gsrc[m];
  fx[n] += fx[m]; fy[n] += fy[m]; fz[n] += fz[m];
}

// A walk over the six exchange stages goes round by round.  A round is one stage {d} or, where the + and the - stage of an axis travel together,
// the two stages {d0, d0 + 1} of that axis: both scan the same atoms (residents and the ghosts of EARLIER axes, comm.F90:55-66), and their send
// lists, ghost slots and messages lie back to back.  Forward {1,2},{3,4},{5,6} or {1}..{6}; the force fold walks the same rounds backwards.
static inline int n_rounds(bool pairs) { return pairs ? 3 : 6; }
static inline Engine::Round round_at(int i, bool pairs, bool reverse) {
  const int k = reverse ? n_rounds(pairs) - 1 - i : i;
  return pairs ? Engine::Round{2 * k + 1, 2} : Engine::Round{k + 1, 1};
}
static inline double stage_shift(int d, double lbox) { return (d & 1) ? -lbox : lbox; }   // xshift, comm.F90:531-548

// The selection of a round: inBuffer flags of its one or two stages over the same nscan atoms, their scans, the totals -- ONE host wait.
// dr: the ghost shell of the axis, or 0 for the migration, which also skips the slots of atoms that already left (skip_dead).
void Engine::select_round(Round r, int nscan, double dr, int skip_dead, int total[2]) {
  const int axis = (r.d0 - 1) / 2;
  for (int k = 0; k < r.n; ++k)
    k_slab_flags<<<nblk(nscan + 1, 256), 256, 0, stream>>>(nscan, r.d0 + k, box.lbox[axis], dr, spos[axis], type, skip_dead, sel_flags(k));
  for (int k = 0; k < r.n; ++k) {
    size_t tb = cubtmp_bytes;
    RX_HIP(hipcub::DeviceScan::ExclusiveSum(cubtmp, tb, sel_flags(k), sel_scan(k), nscan + 1, stream));
  }
  for (int k = 0; k < r.n; ++k) RX_HIP(hipMemcpyAsync(h_cnt + H_CNT_ROUND0 + k, sel_scan(k) + nscan, sizeof(int), hipMemcpyDeviceToHost, stream));
  sync_stream();
  total[0] = h_cnt[H_CNT_ROUND0]; total[1] = r.n > 1 ? h_cnt[H_CNT_ROUND1] : 0;   // counts arrive in pinned host memory
}

void Engine::ghost_build() {
  if (!multi() && stage_pairs) ghost_build_fused();          // single rank: three kernels, one host wait
  else ghost_build_staged();                                  // (RXMD_NO_STAGE_PAIRS=1 on a single rank: the staged form, every stage delivered locally)
}

// ---------------------------------------------------------------------------------------------
// Single rank, round 5: COPYATOMS(MODE_COPY) and COPYATOMS(MODE_MOVE) without the per-axis host waits.
// The six-stage exchange of a rank that is its own neighbour on every axis (comm.F90:55-100 with self copies) is a fixed function of each
// RESIDENT's normalised coordinates: stage d scans everything the stages of the earlier axes appended, and an image inherits the
// coordinates of its source on the other axes, so whether "the x-image of atom n" is flagged by the y stage is a property of n.  The
// ghost array of the staged build is therefore 26 SEGMENTS laid end to end -- one per non-empty combination (ex, ey, ez), e in
// {none, U: near the upper face, shifted by -lbox, L: near the lower face, shifted by +lbox} -- in stage order and, inside a stage,
// in the order the stage scans its sources (residents, then the segments of the earlier stages in their order); inside a segment the
// residents keep their index order.  That is what the index-ordered force rule (pot.F90:113-144) needs, and it is exactly what
// flag -> scan -> append per stage produced (tests: ghost order against the CPU restatement of the reference, and against the staged path of this file,
// RXMD_NO_STAGE_PAIRS=1).  Three kernels: per-workgroup counts of the 26 predicates (+ normalised coordinates), one scan per
// segment over the workgroups, placement.  One host wait (the totals) instead of three; migration: none.
// MODE_MOVE is the same structure with EXCLUSIVE predicates (an atom leaves through at most one face per axis: its segment is the
// triple of faces it crossed) and dr = 0; a mover's final slot = (atoms that stay) + (movers of earlier segments) + (its rank).
__constant__ unsigned char c_seg_need[26] = {1, 2, 4, 5, 6, 8, 9, 10, 16, 17, 18, 20, 21, 22, 24, 25, 26, 32, 33, 34, 36, 37, 38, 40, 41, 42};   // bit 0/1: x U/L, 2/3: y, 4/5: z
__constant__ signed char c_seg_of[43] = {-1, 0, 1, -1, 2, 3, 4, -1, 5, 6, 7, -1, -1, -1, -1, -1, 8, 9, 10, -1, 11, 12, 13, -1, 14, 15, 16, -1, -1, -1, -1, -1, 17, 18, 19, -1, 20, 21, 22, -1, 23, 24, 25};
static const int seg_stage_first_[8] = {0, 0, 1, 2, 5, 8, 17, 26};     // first segment of stage d (1..6), [7] = end
struct SegGeom { double lbox[3], dr[3]; };
__device__ inline unsigned seg_code(const SegGeom &sg, double s0, double s1, double s2) {     // inBuffer, comm.F90:551-576, both faces of the three axes
  unsigned c = 0u;
  c |= (sg.lbox[0] - sg.dr[0] < s0) ? 1u : 0u;  c |= (s0 <= sg.dr[0]) ? 2u : 0u;
  c |= (sg.lbox[1] - sg.dr[1] < s1) ? 4u : 0u;  c |= (s1 <= sg.dr[1]) ? 8u : 0u;
  c |= (sg.lbox[2] - sg.dr[2] < s2) ? 16u : 0u; c |= (s2 <= sg.dr[2]) ? 32u : 0u;
  return c;
}
template <bool MOVE> __device__ inline bool seg_pred(unsigned code, unsigned need) { return MOVE ? code == need : (code & need) == need; }

// pass 1: normalised coordinates of the residents (xu2xs), their face code, and per workgroup how many of its atoms each segment takes
// (MOVE: slot 26 = the atoms that stay).  cnt[seg * nblocks + block].
template <bool MOVE>
__global__ void __launch_bounds__(256) k_seg_count(int N, BoxDev B, SegGeom sg, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                   double *__restrict__ sx, double *__restrict__ sy, double *__restrict__ sz, const int *__restrict__ type,
                                                   unsigned char *__restrict__ code_out, int *__restrict__ cnt) {
  __shared__ int s_w[27][4];
  const int n = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned code = 0u; bool live = false;
  if (n < N) {
    const double r0 = x[n], r1 = y[n], r2 = z[n];
    const double a = (B.Hi[0] * r0 + B.Hi[1] * r1 + B.Hi[2] * r2) - B.obox[0], b = (B.Hi[3] * r0 + B.Hi[4] * r1 + B.Hi[5] * r2) - B.obox[1],
                 c = (B.Hi[6] * r0 + B.Hi[7] * r1 + B.Hi[8] * r2) - B.obox[2];
    sx[n] = a; sy[n] = b; sz[n] = c;
    live = !MOVE || type[n] > 0;
    if (live) code = seg_code(sg, a, b, c);
    code_out[n] = static_cast<unsigned char>(code | (live ? 0u : 128u));
  }
  const unsigned long long any = __ballot(code != 0u);
  for (int s = 0; s < 26; ++s) {
    int c_ = 0;
    if (any) c_ = __popcll(__ballot(live && seg_pred<MOVE>(code, c_seg_need[s])));
    if (lane == 0) s_w[s][w] = c_;
  }
  if (MOVE) { const int c_ = __popcll(__ballot(live && code == 0u)); if (lane == 0) s_w[26][w] = c_; }
  __syncthreads();
  if (threadIdx.x < (MOVE ? 27 : 26)) cnt[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x] = s_w[threadIdx.x][0] + s_w[threadIdx.x][1] + s_w[threadIdx.x][2] + s_w[threadIdx.x][3];
}
// pass 2: one workgroup per segment: exclusive prefix of its per-workgroup counts in place, its total -> tot[seg]
// hpub (the ghost build of one rank): the total also goes straight into pinned host memory, tagged with the build's sequence number in the upper half of
// the word -- the host polls these words instead of waiting for a copy behind the placement kernel (pinned_wait)
__global__ void __launch_bounds__(256) k_seg_scan(int nblocks, int *__restrict__ cnt, int *__restrict__ tot, unsigned long long *hpub = nullptr, unsigned seq = 0u) {
  __shared__ int s_p[256];
  int *c = cnt + static_cast<size_t>(blockIdx.x) * nblocks;
  const int per = (nblocks + 255) / 256, b0 = threadIdx.x * per, b1 = min(b0 + per, nblocks);
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += c[b];
  s_p[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = threadIdx.x >= o ? s_p[threadIdx.x - o] : 0;
    __syncthreads();
    s_p[threadIdx.x] += v;
    __syncthreads();
  }
  int run = s_p[threadIdx.x] - sum;
  for (int b = b0; b < b1; ++b) { const int v = c[b]; c[b] = run; run += v; }
  if (threadIdx.x == 255) {
    tot[blockIdx.x] = s_p[255];
    if (hpub) __hip_atomic_store(hpub + blockIdx.x, (static_cast<unsigned long long>(seq) << 32) | static_cast<unsigned>(s_p[255]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// rank of this thread's atom among the atoms of its workgroup that segment `need` takes (lanes before it + wavefronts before it), from the
// per-wavefront counts in LDS
template <bool MOVE>
__device__ inline int seg_rank_in_block(const int (*s_w)[4], int s, bool pred, int lane, int w) {
  const unsigned long long m = __ballot(pred);
  int r = __popcll(m & ((1ULL << lane) - 1ULL));
  for (int q = 0; q < w; ++q) r += s_w[s][q];
  return r;
}
// pass 3 (MODE_COPY): every resident writes its images: shifted normalised and real coordinates (xshift comm.F90:531-548, xs2xu), type, gid,
// charge, its source in the stage scan (gsrc: the image of the same atom in the parent segment, or the resident), its root, the send list
__global__ void __launch_bounds__(256) k_seg_place_ghosts(int N, int NB, BoxDev B, SegGeom sg, const unsigned char *__restrict__ code_in, const int *__restrict__ cnt, const int *__restrict__ tot,
                                                          double *__restrict__ sx, double *__restrict__ sy, double *__restrict__ sz, double *__restrict__ x, double *__restrict__ y, double *__restrict__ z,
                                                          int *__restrict__ type, long long *__restrict__ gid, double *__restrict__ q, int *__restrict__ gsrc, int *__restrict__ groot, int *__restrict__ sendidx) {
  __shared__ int s_w[26][4], s_base[27];
  const int n = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned code = n < N ? code_in[n] : 0u;
  if (threadIdx.x == 0) { int o = N; for (int s = 0; s < 26; ++s) { s_base[s] = o; o += tot[s]; } s_base[26] = o; }
  const unsigned long long any = __ballot(code != 0u);
  if (__syncthreads_or(any != 0ULL) == 0) return;                       // an interior workgroup: nothing to place
  for (int s = 0; s < 26; ++s) {
    const int c_ = any ? __popcll(__ballot(seg_pred<false>(code, c_seg_need[s]))) : 0;
    if (lane == 0) s_w[s][w] = c_;
  }
  __syncthreads();
  if (!any) return;                                                      // (wave-uniform)
  double a0 = 0.0, b0 = 0.0, c0 = 0.0, qn = 0.0; int tn = 0; long long gn = 0;
  if (code) { a0 = sx[n]; b0 = sy[n]; c0 = sz[n]; qn = q[n]; tn = type[n]; gn = gid[n]; }
  for (int s = 0; s < 26; ++s) {
    const unsigned need = c_seg_need[s];
    const bool p = seg_pred<false>(code, need);
    const int r = seg_rank_in_block<false>(s_w, s, p, lane, w);
    const unsigned pneed = need >= 16u ? (need & 15u) : (need >= 4u ? (need & 3u) : 0u);      // the same atom one stage earlier
    int src = n;
    if (pneed) { const int ps = c_seg_of[pneed]; const int rp = seg_rank_in_block<false>(s_w, ps, seg_pred<false>(code, pneed), lane, w); src = s_base[ps] + cnt[static_cast<size_t>(ps) * gridDim.x + blockIdx.x] + rp; }
    if (!p) continue;
    const int m = s_base[s] + cnt[static_cast<size_t>(s) * gridDim.x + blockIdx.x] + r;
    if (m >= NB) continue;                                               // over capacity: the host sees the totals and raises the reference's trap
    double a = a0, b = b0, c = c0;
    if (need & 1u) a += -sg.lbox[0]; if (need & 2u) a += sg.lbox[0];
    if (need & 4u) b += -sg.lbox[1]; if (need & 8u) b += sg.lbox[1];
    if (need & 16u) c += -sg.lbox[2]; if (need & 32u) c += sg.lbox[2];
    sx[m] = a; sy[m] = b; sz[m] = c;
    const double r0 = a + B.obox[0], r1 = b + B.obox[1], r2 = c + B.obox[2];
    x[m] = B.H[0] * r0 + B.H[1] * r1 + B.H[2] * r2; y[m] = B.H[3] * r0 + B.H[4] * r1 + B.H[5] * r2; z[m] = B.H[6] * r0 + B.H[7] * r1 + B.H[8] * r2;
    type[m] = tn; gid[m] = gn; q[m] = qn;
    gsrc[m] = src; groot[m] = n; sendidx[m - N] = src;
  }
}

void Engine::ghost_build_fused() {
  const BoxDev B = boxdev(box);
  SegGeom sg;
  for (int a = 0; a < 3; ++a) { sg.lbox[a] = box.lbox[a]; sg.dr[a] = shell[a]; }
  const int nbk = nblk(N, 256);
  ensure_seg_buffers(nbk);
  k_seg_count<false><<<nbk, 256, 0, stream>>>(N, B, sg, pos[0], pos[1], pos[2], spos[0], spos[1], spos[2], type, seg_code_, seg_cnt);
  // The one host wait of the ghost build: the ghost count sizes every launch behind it.  The scan kernel hands the 26 totals to the host through pinned
  // memory (round 6, late): the host has them while the placement kernel still runs and queues the next kernels behind it -- until then a copy behind the
  // placement kernel and a stream synchronisation left the GPU idle for ~35 us per step.
  const unsigned seq = ++pub_seq;
  k_seg_scan<<<26, 256, 0, stream>>>(nbk, seg_cnt, seg_tot, h_pub, seq);
  k_seg_place_ghosts<<<nbk, 256, 0, stream>>>(N, NB, B, sg, seg_code_, seg_cnt, seg_tot, spos[0], spos[1], spos[2], pos[0], pos[1], pos[2], type, gid, q, gsrc, groot, sendidx);
  pinned_wait(26, seq, "ghost counts");
  for (int s = 0; s < 26; ++s) h_seg[s] = static_cast<int>(h_pub[s] & 0xffffffffull);
  copyptr[0] = N; sendoff[1] = 0;
  for (int d = 1; d <= 6; ++d) {
    long long t = 0;
    for (int s = seg_stage_first_[d]; s < seg_stage_first_[d + 1]; ++s) t += h_seg[s];
    if (static_cast<long long>(copyptr[d - 1]) + t > NB)
      throw EngineError(RXMD_E_NBUFFER, "over capacity in append_atoms: residents+ghosts exceed NBUFFER=" + std::to_string(NB));
    copyptr[d] = copyptr[d - 1] + static_cast<int>(t); sendoff[d + 1] = sendoff[d] + static_cast<int>(t);
  }
  G = copyptr[6];
  ghosts_valid = true;
  st.nghost_force = G - N; st.nghost_qeq = G - N;
}

// pass 3 (MODE_MOVE): every atom goes to its final slot of scratch copies (atoms that stay keep their order, movers follow segment by segment),
// shifted on the axes it crossed; pass 4 copies back and forms the real coordinates of everything (xs2xu).  Both leave at once when nobody moved.
struct MoveArrays { double *d[12]; double *t[12]; int nd; long long *gid, *gid_t; int *type, *type_t; };
__global__ void __launch_bounds__(256) k_seg_place_move(int N, SegGeom sg, const unsigned char *__restrict__ code_in, const int *__restrict__ cnt, const int *__restrict__ tot, MoveArrays A) {
  __shared__ int s_w[27][4], s_base[27];
  int movers = 0;
  for (int s = 0; s < 26; ++s) movers += tot[s];
  if (movers == 0) return;                                               // (uniform over the whole launch)
  const int n = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned cf = n < N ? code_in[n] : 128u;
  const bool live = (cf & 128u) == 0u; const unsigned code = cf & 63u;
  if (threadIdx.x == 0) { int o = tot[26]; for (int s = 0; s < 26; ++s) { s_base[s] = o; o += tot[s]; } s_base[26] = 0; }
  for (int s = 0; s < 27; ++s) {
    const int c_ = __popcll(__ballot(live && (s < 26 ? code == c_seg_need[s] : code == 0u)));
    if (lane == 0) s_w[s][w] = c_;
  }
  __syncthreads();
  if (!live) return;
  const int s = code ? c_seg_of[code] : 26;                              // (a code with both faces of an axis cannot occur: lbox < s and s <= 0 exclude each other)
  if (s < 0) return;
  // rank among the atoms of this workgroup with the same segment: every lane needs the ballot of ITS segment; segments are few, walk the ones present
  int r = 0;
  for (int t_ = 0; t_ < 27; ++t_) {
    const unsigned long long m = __ballot(s == t_);
    if (s == t_) { r = __popcll(m & ((1ULL << lane) - 1ULL)); for (int q = 0; q < w; ++q) r += s_w[t_][q]; }
  }
  const int m = s_base[s] + cnt[static_cast<size_t>(s) * gridDim.x + blockIdx.x] + r;
  for (int a = 0; a < A.nd; ++a) {
    double v = A.d[a][n];
    if (a < 3) { const unsigned up = 1u << (2 * a), lo = 2u << (2 * a); if (code & up) v += -sg.lbox[a]; if (code & lo) v += sg.lbox[a]; }   // d[0..2] = normalised x, y, z
    A.t[a][m] = v;
  }
  A.gid_t[m] = A.gid[n]; A.type_t[m] = A.type[n];
}
__global__ void __launch_bounds__(256) k_seg_finish_move(int N, BoxDev B, const int *__restrict__ tot, MoveArrays A, double *__restrict__ x, double *__restrict__ y, double *__restrict__ z) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  int movers = 0;
  for (int s = 0; s < 26; ++s) movers += tot[s];
  if (movers) {
    for (int a = 0; a < A.nd; ++a) A.d[a][n] = A.t[a][n];
    A.gid[n] = A.gid_t[n]; A.type[n] = A.type_t[n];
  }
  const double r0 = A.d[0][n] + B.obox[0], r1 = A.d[1][n] + B.obox[1], r2 = A.d[2][n] + B.obox[2];
  x[n] = B.H[0] * r0 + B.H[1] * r1 + B.H[2] * r2; y[n] = B.H[3] * r0 + B.H[4] * r1 + B.H[5] * r2; z[n] = B.H[6] * r0 + B.H[7] * r1 + B.H[8] * r2;
}

void Engine::migrate_fused() {
  // Single rank only: every resident is LIVE (type > 0) -- an atom that leaves through a face comes back in through the opposite one, nothing
  // is ever handed to another rank, so N does not change and there is no dead slot to compact out (the staged path, which several ranks run,
  // does both: k_pack_move marks type = -1, comm.F90:440, and the compaction behind the stages shrinks N).
  const BoxDev B = boxdev(box);
  SegGeom sg;
  for (int a = 0; a < 3; ++a) { sg.lbox[a] = box.lbox[a]; sg.dr[a] = 0.0; }
  const int nbk = nblk(N, 256);
  ensure_seg_buffers(nbk);
  k_seg_count<true><<<nbk, 256, 0, stream>>>(N, B, sg, pos[0], pos[1], pos[2], spos[0], spos[1], spos[2], type, seg_code_, seg_cnt);
  k_seg_scan<<<27, 256, 0, stream>>>(nbk, seg_cnt, seg_tot);
  // scratch: force + bonded scratch arrays as targets (they are recomputed every step), as the staged path does
  MoveArrays A{};
  double *src[12] = {spos[0], spos[1], spos[2], vel[0], vel[1], vel[2], q, qsfp, qsfv, shl[0], shl[1], shl[2]};
  double *tmp[12] = {frc[0], frc[1], frc[2], cds, cd, cc_, deltap, delta, nlp, A0, A1, A2};
  A.nd = ff.pqeq ? 12 : 9;
  for (int a = 0; a < 12; ++a) { A.d[a] = src[a]; A.t[a] = tmp[a]; }
  A.gid = gid; A.gid_t = reinterpret_cast<long long *>(dDlp); A.type = type; A.type_t = perm_in;
  k_seg_place_move<<<nbk, 256, 0, stream>>>(N, sg, seg_code_, seg_cnt, seg_tot, A);
  k_seg_finish_move<<<nbk, 256, 0, stream>>>(N, B, seg_tot, A, pos[0], pos[1], pos[2]);
  G = N;
  lists_valid = false; ghosts_valid = false;
  st.natoms = N;
}

void Engine::ensure_seg_buffers(int nbk) {
  if (nbk <= seg_blocks_cap) return;
  bufs.free_group(G_SEG);
  seg_blocks_cap = nbk + nbk / 4 + 16;
  bufs.alloc_group(*this, G_SEG, static_cast<size_t>(seg_blocks_cap));
  if (!h_seg) bufs.alloc_group(*this, G_SEG_PINNED);
}

void Engine::halo_refresh(double2 *v2, double *v1) {
  if (multi()) { if (v2) halo_staged(reinterpret_cast<double *>(v2), 2); if (v1) halo_staged(v1, 1); return; }
  if (G <= N) return;
  if (v2) k_refresh2<<<nblk(G - N, 256), 256, 0, stream>>>(N, G, groot, v2);
  if (v1) k_refresh1<<<nblk(G - N, 256), 256, 0, stream>>>(N, G, groot, v1);
}

// ---------------------------------------------------------------------------------------------
// multi-rank: the same six stages with pack -> send_recv -> unpack (reference src/comm.F90:68-86).  A stage whose
// partner is this rank (vprocs(axis) == 1) is a device copy; otherwise the host-supplied transport moves the bytes.
__global__ void k_pack_ghosts(int nscan, int axis, double sft, const int *flags, const int *scanout, const double *sx, const double *sy, const double *sz,
                              const int *type, const long long *gid, const double *q, double *buf, int *sendlist, int nres, int myid, const long long *gowner) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= nscan || !flags[n]) return;
  const int k = scanout[n];
  double a = sx[n], b = sy[n], c = sz[n];
  if (axis == 0) a += sft; else if (axis == 1) b += sft; else c += sft;
  double *o = buf + 6 * static_cast<size_t>(k);
  // the type word also carries who owns the atom: (owner's local index * 1024 + owner rank) * 64 + type, exact in a double.  A resident is its
  // own owner; a ghost that is forwarded keeps the owner it arrived with (direct vector halo, engine.h)
  const long long own = (n < nres) ? (static_cast<long long>(n) * 1024 + myid) : gowner[n];
  o[0] = a; o[1] = b; o[2] = c; o[3] = static_cast<double>(own * 64 + type[n]); o[4] = static_cast<double>(gid[n]); o[5] = q[n];
  sendlist[k] = n;
}
__global__ void k_unpack_ghosts(int cnt, int base, const double *buf, double *sx, double *sy, double *sz, int *type, long long *gid, double *q, int *gsrc, long long *gowner) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  const double *o = buf + 6 * static_cast<size_t>(k);
  const int m = base + k;
  const long long w = llrint(o[3]);
  sx[m] = o[0]; sy[m] = o[1]; sz[m] = o[2]; type[m] = static_cast<int>(w & 63); gid[m] = llrint(o[4]); q[m] = o[5];
  gowner[m] = w >> 6;
  gsrc[m] = -1;
}
__global__ void k_pack_vec(int cnt, int ncomp, const int *sendlist, const double *v, double *buf) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  const int n = sendlist[k];
  for (int c = 0; c < ncomp; ++c) buf[static_cast<size_t>(k) * ncomp + c] = v[static_cast<size_t>(n) * ncomp + c];
}
__global__ void k_unpack_vec(int cnt, int ncomp, int base, const double *buf, double *v) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  for (int c = 0; c < ncomp; ++c) v[static_cast<size_t>(base + k) * ncomp + c] = buf[static_cast<size_t>(k) * ncomp + c];
}
__global__ void k_pack_force(int g0, int cnt, const double *fx, const double *fy, const double *fz, double *buf) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  buf[3 * static_cast<size_t>(k)] = fx[g0 + k]; buf[3 * static_cast<size_t>(k) + 1] = fy[g0 + k]; buf[3 * static_cast<size_t>(k) + 2] = fz[g0 + k];
}
__global__ void k_add_force(int cnt, const int *sendlist, const double *buf, double *fx, double *fy, double *fz) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  const int n = sendlist[k];      // unique within a stage
  fx[n] += buf[3 * static_cast<size_t>(k)]; fy[n] += buf[3 * static_cast<size_t>(k) + 1]; fz[n] += buf[3 * static_cast<size_t>(k) + 2];
}

// The migration sizes its message buffers from what THIS rank sends.  The RCCL transport learns the incoming size first and grows the
// buffers (grow_xbuf_keep_send); a callback transport (rxmd_comm_ops: torch.distributed, the host-staged MPI binding) has one call
// per message and would have to fail after its size exchange, leaving the peer inside its payload exchange.  With callbacks and the
// engine's own buffers the receive side is therefore sized for the worst case the ghost build already allocates (NBUFFER x 6 doubles:
// more migrants than a rank can hold); host-supplied buffers keep their contract (the callback gets the capacity).
size_t Engine::migrate_xbuf_doubles(size_t from_send_count) const {
  if (nccl || !multi() || (!xbuf_owned && xbuf_doubles > 0)) return from_send_count;
  return std::max(from_send_count, static_cast<size_t>(NB) * 6);
}

void Engine::ensure_xbuf(size_t doubles) {
  if (doubles <= xbuf_doubles) return;
  if (!xbuf_owned && xbuf_doubles > 0) throw EngineError(RXMD_E_COMM, "host-supplied exchange buffers are too small");
  bufs.free_group(G_XBUF);
  xbuf_doubles = doubles + doubles / 4 + 4096;
  bufs.alloc_group(*this, G_XBUF, xbuf_doubles);
  xbuf_owned = true;
}

// a message announced by its size message does not fit: the engine's own buffers grow with the packed send data kept (a caller that
// sized them from its send count only, as the migration does, needs no worst case); host-supplied buffers cannot grow
void Engine::grow_xbuf_keep_send(size_t need, size_t keep) {
  if (!xbuf_owned) throw EngineError(RXMD_E_NBUFFER, "incoming message larger than the host-supplied exchange buffers");
  double *old_send = xbuf_send, *old_recv = xbuf_recv;            // (the old pair outlives the allocation of the new one: the table takes the new blocks over)
  const size_t cap = need + need / 4 + 4096;
  bufs.alloc_group(*this, G_XBUF, cap);                         // (throws with the old pair and xbuf_doubles untouched)
  xbuf_doubles = cap;
  if (keep > 0) RX_HIP(hipMemcpyAsync(xbuf_send, old_send, sizeof(double) * keep, hipMemcpyDeviceToDevice, stream));
  sync_stream();
  dev_free(old_send); dev_free(old_recv);
}

// One round of send_recv (comm.F90:291-364): message k of the round goes to the neighbour of stage d0 + k (reverse: comes back from it).  The
// messages lie back to back: xbuf_send = [message of d0 | message of d0 + 1], xbuf_recv likewise, all of a round in flight at once.
// counts_known: nrecv[] holds what the ghost build announced (vector halos, force fold), and comes back as what arrived; otherwise the
// sizes travel first (ghost build, migration) and nrecv[] is the answer.
void Engine::exchange_round(Round r, bool reverse, const long long nsend[2], long long nrecv[2], bool counts_known) {
  int to[2] = {0, 0}, from[2] = {0, 0};
  for (int k = 0; k < r.n; ++k) {
    const int d = r.d0 + k;
    to[k] = reverse ? target_node[dinv_[d]] : target_node[d];
    from[k] = reverse ? target_node[d] : target_node[dinv_[d]];
  }
  const long long ns = nsend[0] + (r.n > 1 ? nsend[1] : 0);
  if (to[0] == cfg.myid && from[0] == cfg.myid && !(force_remote && nccl)) {              // the axis is not split: every partner is this rank (comm.F90:305-315)
    for (int k = 0; k < r.n; ++k) {
      if (counts_known && nsend[k] != nrecv[k]) throw EngineError(RXMD_E_COMM, "self exchange with unequal send and receive counts");
      nrecv[k] = nsend[k];
    }
    if (ns > 0) RX_HIP(hipMemcpyAsync(xbuf_recv, xbuf_send, sizeof(double) * ns, hipMemcpyDeviceToDevice, stream));
    return;
  }
  if (nccl) { rccl_exchange_round(r.n, to, from, nsend, nrecv, counts_known); return; }   // native: stays in stream order
  if (!has_comm || !comm.exchange) throw EngineError(RXMD_E_COMM, "vprocs > 1 needs a transport: call rxmd_hip_set_comm first");
  sync_stream();                        // the messages must be packed before the transport reads them
  long long so = 0, ro = 0;
  for (int k = 0; k < r.n; ++k) {       // one call per message; a known count goes through exchange_known where the transport has it
    const long long nr = (counts_known && comm.exchange_known)
                             ? comm.exchange_known(comm.ctx, to[k], xbuf_send + so, nsend[k], from[k], xbuf_recv + ro, nrecv[k])
                             : comm.exchange(comm.ctx, to[k], xbuf_send + so, nsend[k], from[k], xbuf_recv + ro, static_cast<long long>(xbuf_doubles) - ro);
    if (nr < 0) throw EngineError(RXMD_E_COMM, "exchange callback failed");
    nrecv[k] = nr; so += nsend[k]; ro += nr;
  }
}

// COPYATOMS(MODE_COPY) stage by stage: select -> pack -> send_recv -> unpack per round.  On a single rank (RXMD_NO_STAGE_PAIRS=1; the 26-segment
// form above is what runs otherwise) a stage appends its selection to the rank's own arrays instead (store_atoms + append_atoms in one kernel).
void Engine::ghost_build_staged() {
  const BoxDev B = boxdev(box);
  const bool local = !multi();
  // own buffers: sized once for the worst case; host-supplied buffers (rxmd_hip_set_exchange_buffers): each round asks for what its
  // messages need, the receive side is bounded by the transport (the callbacks get the capacity, the RCCL path checks it)
  const bool xb_fixed = !xbuf_owned && xbuf_doubles > 0;
  if (!local && !xb_fixed) ensure_xbuf(static_cast<size_t>(NB) * 6);
  k_to_normalised<<<nblk(N, 256), 256, 0, stream>>>(B, 0, N, pos[0], pos[1], pos[2], spos[0], spos[1], spos[2]);
  copyptr[0] = N;
  sendoff[1] = 0;
  for (int i = 0; i < n_rounds(stage_pairs); ++i) {           // paired: three rounds and six host waits per ghost build instead of six and twelve
    const Round r = round_at(i, stage_pairs, false);
    const int nscan = copyptr[cptridx_[r.d0]], axis = (r.d0 - 1) / 2, base = copyptr[r.d0 - 1];
    int t[2], c[2];
    select_round(r, nscan, shell[axis], 0, t);
    c[0] = t[0]; c[1] = t[1];                                 // delivered locally: what a stage selects is what it appends
    if (!local) {
      if (sendoff[r.d0] + t[0] + t[1] > NB) throw EngineError(RXMD_E_NBUFFER, "over capacity in store_atoms (send list)");
      if (xb_fixed) ensure_xbuf(6 * (static_cast<size_t>(t[0]) + t[1]));
      long long nsend[2] = {6LL * t[0], 6LL * t[1]}, nrecv[2] = {0, 0};
      for (int k = 0, off = 0; k < r.n; off += t[k], ++k)
        if (t[k] > 0)
          k_pack_ghosts<<<nblk(nscan, 256), 256, 0, stream>>>(nscan, axis, stage_shift(r.d0 + k, box.lbox[axis]), sel_flags(k), sel_scan(k), spos[0], spos[1], spos[2], type, gid, q,
                                                              xbuf_send + 6LL * off, sendidx + sendoff[r.d0] + off, N, cfg.myid, gowner);
      exchange_round(r, false, nsend, nrecv, false);
      c[0] = static_cast<int>(nrecv[0] / 6); c[1] = static_cast<int>(nrecv[1] / 6);
    }
    if (static_cast<long long>(base) + c[0] + c[1] > NB)
      throw EngineError(RXMD_E_NBUFFER, "over capacity in append_atoms: residents+ghosts exceed NBUFFER=" + std::to_string(NB));
    for (int k = 0; k < r.n; ++k) { sendoff[r.d0 + k + 1] = sendoff[r.d0 + k] + t[k]; copyptr[r.d0 + k] = copyptr[r.d0 + k - 1] + c[k]; }
    if (local) {
      for (int k = 0; k < r.n; ++k)
        if (t[k] > 0)
          k_append_ghosts<<<nblk(nscan, 256), 256, 0, stream>>>(nscan, copyptr[r.d0 + k - 1], N, axis, stage_shift(r.d0 + k, box.lbox[axis]), sel_flags(k), sel_scan(k), spos[0], spos[1], spos[2],
                                                                type, gid, q, gsrc, groot, sendidx + sendoff[r.d0 + k]);
    } else if (c[0] + c[1] > 0)
      k_unpack_ghosts<<<nblk(c[0] + c[1], 256), 256, 0, stream>>>(c[0] + c[1], base, xbuf_recv, spos[0], spos[1], spos[2], type, gid, q, gsrc, gowner);
  }
  G = copyptr[6];
  if (G > N) k_to_real<<<nblk(G - N, 256), 256, 0, stream>>>(B, N, G, spos[0], spos[1], spos[2], pos[0], pos[1], pos[2]);
  ghosts_valid = true;
  st.nghost_force = G - N; st.nghost_qeq = G - N;
  if (!local && halo_direct) direct_halo_setup();   // owners and index lists of this build's ghosts (engine.h)
}

// ---- direct vector halo (RXMD_HALO_DIRECT=1; engine.h) -----------------------------------------------------------------------------
__global__ void k_dh_keys(int N, int G, const long long *__restrict__ gowner, int *__restrict__ keys, int *__restrict__ vals) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= G - N) return;
  keys[t] = static_cast<int>(gowner[N + t] & 1023); vals[t] = N + t;
}
__global__ void k_dh_offsets(int np, int n, const int *__restrict__ keys_sorted, int *__restrict__ off) {     // off[p] = first position whose owner rank is >= p
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > np) return;
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys_sorted[mid] < p) lo = mid + 1; else hi = mid; }
  off[p] = lo;
}
__global__ void k_dh_requests(int n, const int *__restrict__ ghost, const long long *__restrict__ gowner, double *__restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = static_cast<double>(gowner[ghost[k]] >> 10);
}
__global__ void k_dh_to_int(int n, const double *__restrict__ in, int *__restrict__ out, int nres, int *err) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const long long i = llrint(in[k]);
  if (i < 0 || i >= nres) { atomicCAS(&err[0], DERR_NONE, DERR_GRID); out[k] = 0; return; }   // a request for an atom this rank does not own
  out[k] = static_cast<int>(i);
}
__global__ void k_dh_unpack(int cnt, int ncomp, const int *__restrict__ ghost, const double *__restrict__ buf, double *__restrict__ v) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  const int m = ghost[k];
  for (int c = 0; c < ncomp; ++c) v[static_cast<size_t>(m) * ncomp + c] = buf[static_cast<size_t>(k) * ncomp + c];
}

// segment p of xbuf_send goes to rank p, segment p of xbuf_recv comes from rank p (offsets in atoms, ncomp doubles each): RCCL -- every
// peer in ONE group; callbacks -- np - 1 shifted send_recv rounds (to = me + r, from = me - r: every rank is in the same round at the same
// time, and every rank always posts both halves, as the transports expect); the rank's own segment is a device copy
void Engine::exchange_many(const std::vector<long long> &soff, const std::vector<long long> &roff, int ncomp) {
  const int me = cfg.myid, np = nprocs;
  const bool self_remote = force_remote && nccl;
  if (!self_remote) {
    const long long sc = (soff[me + 1] - soff[me]) * ncomp, rc = (roff[me + 1] - roff[me]) * ncomp;
    if (sc != rc) throw EngineError(RXMD_E_COMM, "direct halo: a rank disagrees with itself about its own images");
    if (sc > 0) RX_HIP(hipMemcpyAsync(xbuf_recv + roff[me] * ncomp, xbuf_send + soff[me] * ncomp, sizeof(double) * sc, hipMemcpyDeviceToDevice, stream));
  }
  if (nccl) { rccl_exchange_many(soff, roff, ncomp); return; }
  if (np == 1) return;
  if (!has_comm || !comm.exchange) throw EngineError(RXMD_E_COMM, "vprocs > 1 needs a transport: call rxmd_hip_set_comm first");
  sync_stream();
  for (int r = 1; r < np; ++r) {
    const int to = (me + r) % np, from = (me - r + np) % np;
    const long long sc = (soff[to + 1] - soff[to]) * ncomp, rc = (roff[from + 1] - roff[from]) * ncomp;
    const long long got = comm.exchange_known ? comm.exchange_known(comm.ctx, to, xbuf_send + soff[to] * ncomp, sc, from, xbuf_recv + roff[from] * ncomp, rc)
                                              : comm.exchange(comm.ctx, to, xbuf_send + soff[to] * ncomp, sc, from, xbuf_recv + roff[from] * ncomp, static_cast<long long>(xbuf_doubles) - roff[from] * ncomp);
    if (got != rc) throw EngineError(RXMD_E_COMM, "direct halo: message size differs from what the request phase announced");
  }
}

// after a ghost build: group the ghosts by owner rank, tell every rank how many of its atoms each other rank needs (one all-reduce of an
// np x np table), send the owners their index lists
void Engine::direct_halo_setup() {
  dh_ready = false;
  const int np = nprocs, me = cfg.myid, ng = G - N;
  if (np > 1000) throw EngineError(RXMD_E_ARG, "direct halo: more than 1000 ranks");
  dh_need_off.assign(np + 1, 0); dh_serve_off.assign(np + 1, 0);
  if (ng > 0) {
    k_dh_keys<<<nblk(ng, 256), 256, 0, stream>>>(N, G, gowner, dh_keys, dh_vals);
    size_t tb = cubtmp_bytes;
    RX_HIP(hipcub::DeviceRadixSort::SortPairs(cubtmp, tb, dh_keys, dh_keys2, dh_vals, dh_ghost, ng, 0, 10, stream));
  }
  k_dh_offsets<<<nblk(np + 1, 256), 256, 0, stream>>>(np, ng, dh_keys2, dh_off);
  std::vector<int> off(np + 1);
  RX_HIP(hipMemcpyAsync(off.data(), dh_off, sizeof(int) * (np + 1), hipMemcpyDeviceToHost, stream));
  sync_stream();
  for (int p = 0; p <= np; ++p) dh_need_off[p] = off[p];
  std::vector<double> table(static_cast<size_t>(np) * np, 0.0);                 // table[a * np + b] = atoms of rank b that rank a holds as ghosts
  for (int p = 0; p < np; ++p) table[static_cast<size_t>(me) * np + p] = static_cast<double>(off[p + 1] - off[p]);
  if (np > 1) allreduce_host(table.data(), np * np);
  for (int p = 0; p < np; ++p) dh_serve_off[p + 1] = dh_serve_off[p] + static_cast<long long>(table[static_cast<size_t>(p) * np + me]);
  const long long nserve = dh_serve_off[np];
  ensure_xbuf(static_cast<size_t>(std::max<long long>(std::max<long long>(ng, nserve), 1)) * 3);      // up to three components per atom (PQEq shells)
  if (nserve > dh_serve_cap) { bufs.free_group(G_DH_SERVE); dh_serve_cap = static_cast<int>(nserve + nserve / 4 + 1024); bufs.alloc_group(*this, G_DH_SERVE, static_cast<size_t>(dh_serve_cap)); }
  if (ng > 0) k_dh_requests<<<nblk(ng, 256), 256, 0, stream>>>(ng, dh_ghost, gowner, xbuf_send);
  exchange_many(dh_need_off, dh_serve_off, 1);                                   // my requests out, the other ranks' requests in
  if (nserve > 0) k_dh_to_int<<<nblk(nserve, 256), 256, 0, stream>>>(static_cast<int>(nserve), xbuf_recv, dh_serve, N, d_err);
  dh_ready = true;
}

void Engine::halo_direct_exchange(double *v, int ncomp) {
  const int ng = G - N;
  const long long nserve = dh_serve_off[nprocs];
  if (nserve > 0) k_pack_vec<<<nblk(nserve, 256), 256, 0, stream>>>(static_cast<int>(nserve), ncomp, dh_serve, v, xbuf_send);
  exchange_many(dh_serve_off, dh_need_off, ncomp);
  if (ng > 0) k_dh_unpack<<<nblk(ng, 256), 256, 0, stream>>>(ng, ncomp, dh_ghost, xbuf_recv, v);
}

// MODE_QCOPY1 / MODE_QCOPY2 (comm.F90:187-212): ghost slots of an ncomp-interleaved vector, round by round.  The send lists and the ghost slots of
// a round are contiguous: one pack, one exchange, one unpack -- three rounds per halo when the stages pair, six otherwise.
void Engine::halo_staged(double *v, int ncomp) {
  // QCOPY1 / QCOPY2 (comm.F90:2-100 with MODE_QCOPY*): on the second stream the part the main stream waits for is measured at the join
  Timed kt(this, &st.ms_halo, in_comm_region ? nullptr : &st.ms_halo_exposed, &st.halo_calls, 1);
  if (halo_direct && dh_ready) { halo_direct_exchange(v, ncomp); return; }
  const bool pairs = known_counts_pair();
  for (int i = 0; i < n_rounds(pairs); ++i) {
    const Round r = round_at(i, pairs, false);
    const int dl = r.d0 + r.n - 1, ns = sendoff[dl + 1] - sendoff[r.d0], cnt = copyptr[dl] - copyptr[r.d0 - 1];   // dl: the last stage of the round
    if (ns > 0) k_pack_vec<<<nblk(ns, 256), 256, 0, stream>>>(ns, ncomp, sendidx + sendoff[r.d0], v, xbuf_send);
    long long nsend[2] = {0, 0}, want[2] = {0, 0}, nrecv[2];
    for (int k = 0; k < r.n; ++k) { nsend[k] = static_cast<long long>(stage_sends(r.d0 + k)) * ncomp; want[k] = static_cast<long long>(stage_ghosts(r.d0 + k)) * ncomp; }
    nrecv[0] = want[0]; nrecv[1] = want[1];
    exchange_round(r, false, nsend, nrecv, true);
    if (nrecv[0] != want[0] || nrecv[1] != want[1]) throw EngineError(RXMD_E_COMM, "halo size changed between the ghost build and a vector exchange");
    if (cnt > 0) k_unpack_vec<<<nblk(cnt, 256), 256, 0, stream>>>(cnt, ncomp, copyptr[r.d0 - 1], xbuf_recv, v);
  }
}

// MODE_CPBK (comm.F90:74-78,385-396,474-482): the rounds backwards, z first; inside a round the sums of the higher stage land first (6 then 5), which
// keeps the reference's summation order 6,5,4,...  On a single rank a ghost's force goes straight to its source.  The three arrays folded are the
// caller's: FORCE passes frc, the bond-order VJP (bond_vjp.hip) its per-atom gradient -- any per-atom vector with ghost slots folds the same way.
void Engine::fold_ghost_forces(double *fx, double *fy, double *fz) {
  const bool local = !multi(), pairs = !local && known_counts_pair();
  for (int i = 0; i < n_rounds(pairs); ++i) {
    const Round r = round_at(i, pairs, true);
    const int g0 = copyptr[r.d0 - 1], cnt = copyptr[r.d0 + r.n - 1] - g0;
    if (local) {
      for (int d = r.d0 + r.n - 1; d >= r.d0; --d)
        if (copyptr[d] > copyptr[d - 1]) k_fold_stage<<<nblk(copyptr[d] - copyptr[d - 1], 256), 256, 0, stream>>>(copyptr[d - 1], copyptr[d], gsrc, fx, fy, fz);
      continue;
    }
    if (cnt > 0) k_pack_force<<<nblk(cnt, 256), 256, 0, stream>>>(g0, cnt, fx, fy, fz, xbuf_send);
    long long nsend[2] = {0, 0}, want[2] = {0, 0}, nrecv[2];
    for (int k = 0; k < r.n; ++k) { nsend[k] = 3LL * stage_ghosts(r.d0 + k); want[k] = 3LL * stage_sends(r.d0 + k); }
    nrecv[0] = want[0]; nrecv[1] = want[1];
    exchange_round(r, true, nsend, nrecv, true);
    if (nrecv[0] != want[0] || nrecv[1] != want[1]) throw EngineError(RXMD_E_COMM, "returned force count does not match the stage send list");
    for (int d = r.d0 + r.n - 1; d >= r.d0; --d)      // sources are unique within a stage, not within a round
      if (stage_sends(d) > 0)
        k_add_force<<<nblk(stage_sends(d), 256), 256, 0, stream>>>(stage_sends(d), sendidx + sendoff[d], xbuf_recv + 3LL * (sendoff[d] - sendoff[r.d0]), fx, fy, fz);
  }
}

// ---------------------------------------------------------------------------------------------
// COPYATOMS(MODE_MOVE) (reference src/comm.F90 with dr = 0): atoms that left [0,lbox) re-enter through
// the periodic image (or go to the neighbour rank) and are appended after the residents; survivors
// are compacted in order (comm.F90:238-257).  All positions take the normalise -> real round trip.
__global__ void k_move_append(int nscan, int base, int axis, double sft, const int *flags, const int *scanout,
                              double *sx, double *sy, double *sz, double *vx, double *vy, double *vz,
                              int *type, long long *gid, double *q, double *qsfp, double *qsfv) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= nscan || !flags[n]) return;
  const int m = base + scanout[n];
  double a = sx[n], b = sy[n], c = sz[n];
  if (axis == 0) a += sft; else if (axis == 1) b += sft; else c += sft;
  sx[m] = a; sy[m] = b; sz[m] = c; vx[m] = vx[n]; vy[m] = vy[n]; vz[m] = vz[n];
  type[m] = type[n]; gid[m] = gid[n]; q[m] = q[n]; qsfp[m] = qsfp[n]; qsfv[m] = qsfv[n];
  type[n] = -1;   // comm.F90:440
}
// the same append for one more per-atom array (PQEq shell displacement, unshifted: comm.F90:165-167); runs before k_move_append
__global__ void k_move_append_extra(int nscan, int base, const int *flags, const int *scanout, double *a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= nscan || !flags[n]) return;
  a[base + scanout[n]] = a[n];
}
__global__ void k_pack_extra3(int nscan, const int *flags, const int *scanout, int W, int o, const double *a0, const double *a1, const double *a2, double *buf) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= nscan || !flags[n]) return;
  double *p = buf + static_cast<size_t>(W) * scanout[n] + o;
  p[0] = a0[n]; p[1] = a1[n]; p[2] = a2[n];
}
__global__ void k_unpack_extra3(int cnt, int base, int W, int o, const double *buf, double *a0, double *a1, double *a2) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  const double *p = buf + static_cast<size_t>(W) * k + o;
  a0[base + k] = p[0]; a1[base + k] = p[1]; a2[base + k] = p[2];
}
__global__ void k_alive_flags(int n, const int *type, int *flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) flags[i] = (i < n && type[i] > 0) ? 1 : 0;
}
template <class T>
__global__ void k_compact(int n, const int *flags, const int *scanout, const T *src, T *dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flags[i]) dst[scanout[i]] = src[i];
}

__global__ void k_pack_move(int nscan, int axis, double sft, const int *flags, const int *scanout, const double *sx, const double *sy, const double *sz,
                            const double *vx, const double *vy, const double *vz, int *type, const long long *gid, const double *q,
                            const double *qsfp, const double *qsfv, double *buf, int W) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= nscan || !flags[n]) return;
  double a = sx[n], b = sy[n], c = sz[n];
  if (axis == 0) a += sft; else if (axis == 1) b += sft; else c += sft;
  double *o = buf + static_cast<size_t>(W) * scanout[n];
  o[0] = a; o[1] = b; o[2] = c; o[3] = vx[n]; o[4] = vy[n]; o[5] = vz[n];
  o[6] = static_cast<double>(type[n]); o[7] = static_cast<double>(gid[n]); o[8] = q[n]; o[9] = qsfp[n]; o[10] = qsfv[n];
  type[n] = -1;   // comm.F90:440
}
__global__ void k_unpack_move(int cnt, int base, const double *buf, double *sx, double *sy, double *sz, double *vx, double *vy, double *vz,
                              int *type, long long *gid, double *q, double *qsfp, double *qsfv, int W) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  const double *o = buf + static_cast<size_t>(W) * k;
  const int m = base + k;
  sx[m] = o[0]; sy[m] = o[1]; sz[m] = o[2]; vx[m] = o[3]; vy[m] = o[4]; vz[m] = o[5];
  type[m] = static_cast<int>(llrint(o[6])); gid[m] = llrint(o[7]); q[m] = o[8]; qsfp[m] = o[9]; qsfv[m] = o[10];
}

void Engine::migrate() {
  if (!multi() && stage_pairs) { migrate_fused(); return; }     // single rank: four kernels, no host wait
  const BoxDev B = boxdev(box);
  const bool local = !multi();                   // single rank, RXMD_NO_STAGE_PAIRS=1: a mover is appended to the rank's own arrays, no message
  const int W = ff.pqeq ? 14 : 11;               // doubles per record; + shell displacement (comm.F90:153,165-167)
  k_to_normalised<<<nblk(N, 256), 256, 0, stream>>>(B, 0, N, pos[0], pos[1], pos[2], spos[0], spos[1], spos[2]);
  int cp[7];
  cp[0] = N;
  int moved = 0;
  // the two stages of an axis are independent here too (an atom cannot leave through both faces of one axis): selections, size messages and
  // payloads of both together, as in the ghost build
  for (int i = 0; i < n_rounds(stage_pairs); ++i) {
    const Round r = round_at(i, stage_pairs, false);
    const int nscan = cp[cptridx_[r.d0]], axis = (r.d0 - 1) / 2, base = cp[r.d0 - 1];
    int t[2], c[2];
    select_round(r, nscan, 0.0, 1, t);
    c[0] = t[0]; c[1] = t[1];
    if (!local) {
      ensure_xbuf(migrate_xbuf_doubles(static_cast<size_t>(std::max(t[0] + t[1], 1)) * W + 4096));
      long long nsend[2] = {static_cast<long long>(W) * t[0], static_cast<long long>(W) * t[1]}, nrecv[2] = {0, 0};
      double *b = xbuf_send;
      for (int k = 0; k < r.n; b += static_cast<size_t>(W) * t[k], ++k) {
        if (t[k] == 0) continue;
        if (ff.pqeq) k_pack_extra3<<<nblk(nscan, 256), 256, 0, stream>>>(nscan, sel_flags(k), sel_scan(k), W, 11, shl[0], shl[1], shl[2], b);
        k_pack_move<<<nblk(nscan, 256), 256, 0, stream>>>(nscan, axis, stage_shift(r.d0 + k, box.lbox[axis]), sel_flags(k), sel_scan(k), spos[0], spos[1], spos[2], vel[0], vel[1], vel[2],
                                                          type, gid, q, qsfp, qsfv, b, W);
      }
      exchange_round(r, false, nsend, nrecv, false);
      c[0] = static_cast<int>(nrecv[0] / W); c[1] = static_cast<int>(nrecv[1] / W);
    }
    if (static_cast<long long>(base) + c[0] + c[1] > NB) throw EngineError(RXMD_E_NBUFFER, "over capacity in append_atoms (MODE_MOVE)");
    for (int k = 0; k < r.n; ++k) cp[r.d0 + k] = cp[r.d0 + k - 1] + c[k];
    if (local) {
      for (int k = 0; k < r.n; ++k) {
        if (t[k] == 0) continue;
        if (ff.pqeq)
          for (int a = 0; a < 3; ++a) k_move_append_extra<<<nblk(nscan, 256), 256, 0, stream>>>(nscan, cp[r.d0 + k - 1], sel_flags(k), sel_scan(k), shl[a]);
        k_move_append<<<nblk(nscan, 256), 256, 0, stream>>>(nscan, cp[r.d0 + k - 1], axis, stage_shift(r.d0 + k, box.lbox[axis]), sel_flags(k), sel_scan(k), spos[0], spos[1], spos[2],
                                                            vel[0], vel[1], vel[2], type, gid, q, qsfp, qsfv);
      }
    } else if (c[0] + c[1] > 0) {
      k_unpack_move<<<nblk(c[0] + c[1], 256), 256, 0, stream>>>(c[0] + c[1], base, xbuf_recv, spos[0], spos[1], spos[2], vel[0], vel[1], vel[2], type, gid, q, qsfp, qsfv, W);
      if (ff.pqeq) k_unpack_extra3<<<nblk(c[0] + c[1], 256), 256, 0, stream>>>(c[0] + c[1], base, W, 11, xbuf_recv, shl[0], shl[1], shl[2]);
    }
    moved += t[0] + t[1] + c[0] + c[1];
  }
  int newN = N;
  if (moved > 0) {
    const int n = cp[6];
    k_alive_flags<<<nblk(n + 1, 256), 256, 0, stream>>>(n, type, flags);
    size_t tb = cubtmp_bytes;
    RX_HIP(hipcub::DeviceScan::ExclusiveSum(cubtmp, tb, flags, scanout, n + 1, stream));
    RX_HIP(hipMemcpyAsync(h_cnt + H_CNT_ROUND0, scanout + n, sizeof(int), hipMemcpyDeviceToHost, stream));
    sync_stream();
    newN = h_cnt[H_CNT_ROUND0];   // counts arrive in pinned host memory
    if (newN > rows10) throw EngineError(RXMD_E_NBUFFER, "resident count grew beyond the 10 A list capacity");
    // scratch: reuse force + bonded scratch arrays as compaction targets (they are recomputed every step)
    double *tmpd[9] = {frc[0], frc[1], frc[2], cds, cd, cc_, deltap, delta, nlp};
    double *srcd[9] = {spos[0], spos[1], spos[2], vel[0], vel[1], vel[2], q, qsfp, qsfv};
    for (int a = 0; a < 9; ++a) {
      k_compact<double><<<nblk(n, 256), 256, 0, stream>>>(n, flags, scanout, srcd[a], tmpd[a]);
      RX_HIP(hipMemcpyAsync(srcd[a], tmpd[a], sizeof(double) * newN, hipMemcpyDeviceToDevice, stream));
    }
    if (ff.pqeq) {
      double *ts[3] = {A0, A1, A2};
      for (int a = 0; a < 3; ++a) {
        k_compact<double><<<nblk(n, 256), 256, 0, stream>>>(n, flags, scanout, shl[a], ts[a]);
        RX_HIP(hipMemcpyAsync(shl[a], ts[a], sizeof(double) * newN, hipMemcpyDeviceToDevice, stream));
      }
    }
    k_compact<long long><<<nblk(n, 256), 256, 0, stream>>>(n, flags, scanout, gid, reinterpret_cast<long long *>(dDlp));
    RX_HIP(hipMemcpyAsync(gid, dDlp, sizeof(long long) * newN, hipMemcpyDeviceToDevice, stream));
    k_compact<int><<<nblk(n, 256), 256, 0, stream>>>(n, flags, scanout, type, perm_in);
    RX_HIP(hipMemcpyAsync(type, perm_in, sizeof(int) * newN, hipMemcpyDeviceToDevice, stream));
  }
  N = newN; G = N;
  k_to_real<<<nblk(N, 256), 256, 0, stream>>>(B, 0, N, spos[0], spos[1], spos[2], pos[0], pos[1], pos[2]);
  lists_valid = false; ghosts_valid = false;
  st.natoms = N;
}

}  // namespace rxmd
