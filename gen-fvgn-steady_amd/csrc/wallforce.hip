// Wall forces (gfv/wallforce.py): the pressure and the viscous force of the fluid on a body, and their moment, per
// graph and per sampled field, summed on the device.  TWO launches behind the launch that advances the field (gfv_rollout_advance,
// gfv_march_advance); both follow the clock word that launch writes and read it, and the record rec[8] (the window: include/gfv.h
// GFV_WINDOW_RECORD, gfv_window.h), as they find them:
//   c = *clock;  take = gfv_window_take(rec, c)
// Only the last arriver of the second launch writes the record, so the pair decides alike.
//
//   gfv_wall_force_grad   lane (j, c), c < 3, over the Nb end nodes of the selected faces: the WLSQ gradient of channel c at node
//                         bnode[j] - the arithmetic of wlsq_fwd_kernel (csrc/fvm.hip) on phi_c(i) = x_backup[i, c] / uvp_dim[3 b + c]
//                         (one fp32 division) - with its first two entries KEPT IN DOUBLE: gb [Nb, 3, 2].
//   gfv_wall_force_sum    one wave per chunk of at most 64 selected faces (never across a graph): per face the six terms
//                         (Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv) in double from the fp32 data and gb; lane l adds the rows beg + l,
//                         beg + l + 64, ... in ascending order, the 64 lane sums fold by gfv_wave_sum, one double per chunk and sum
//                         goes to partial [n_wchunks, 6].  The workgroup that arrives last (all-fence form: the partials are plain
//                         stores of other workgroups) folds them per graph (gfv_fold_chunks<6>, gfv_wave_sum) into the ring's row
//                         n % keep, then gfv_window_commit.
// take false: the first launch reads and writes nothing, the second moves no history word.  No floating-point atomics, no sum
// across graphs, an order that does not depend on the grid: the same inputs give the same bits.  The rule in full: include/gfv.h.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_lu.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"
#include "gfv_window.h"

namespace {

constexpr int WF_TPB = 256;
static_assert(GFV_WALL_FORCE_SUMS == 6 && GFV_WALL_FORCE_CHUNK == 64, "include/gfv.h");

// ---- 1. the body nodes' gradients: wlsq_fwd_kernel's arithmetic, 4 lanes per node (the fourth idle), the result in double ------
template <int M>
__global__ __launch_bounds__(WF_TPB) void wall_grad_kernel(const float* __restrict__ x_backup, const float* __restrict__ uvp_dim,
                                                           const int* __restrict__ batch, const int* __restrict__ rowptr,
                                                           const int* __restrict__ outn, const float* __restrict__ Bp,
                                                           const float* __restrict__ An, const float* __restrict__ rn,
                                                           const int* __restrict__ bnode, int Nb, const int* clock, const int* rec,
                                                           double* __restrict__ gb) {
  if (!gfv_window_take(rec, *clock)) return;
  const int t = blockIdx.x * WF_TPB + threadIdx.x;
  const int j = t >> 2, c = t & 3;
  if (j >= Nb || c >= 3) return;
  const int i = bnode[j];
  const float dim = uvp_dim[3 * batch[i] + c];      // (a stencil never leaves its graph)
  lu_t rhs[M];
#pragma unroll
  for (int q = 0; q < M; ++q) rhs[q] = 0.0;
  const lu_t pi = (lu_t)(x_backup[(size_t)i * 12 + c] / dim);
  const int beg = rowptr[i], end = rowptr[i + 1];
  // 4 stencil entries per trip, their loads in flight together; the accumulation stays entry by entry (wlsq_fwd_kernel)
  int k = beg;
  for (; k + 4 <= end; k += 4) {
    lu_t dv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) dv[u] = (lu_t)(x_backup[(size_t)outn[k + u] * 12 + c] / dim) - pi;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float* b = Bp + (size_t)(k + u) * M;
#pragma unroll
      for (int q = 0; q < M; ++q) rhs[q] += (lu_t)b[q] * dv[u];
    }
  }
  for (; k < end; ++k) {
    const lu_t d = (lu_t)(x_backup[(size_t)outn[k] * 12 + c] / dim) - pi;
    const float* b = Bp + (size_t)k * M;
#pragma unroll
    for (int q = 0; q < M; ++q) rhs[q] += (lu_t)b[q] * d;
  }
  LU<M> m;
  load_An(An, rn, i, m);
#pragma unroll
  for (int q = 0; q < M; ++q) rhs[q] = rhs[q] / (lu_t)rn[(size_t)i * M + q];
  lu_factor(m);
  lu_solve(m, rhs);
  gb[((size_t)j * 3 + c) * 2] = rhs[0];
  gb[((size_t)j * 3 + c) * 2 + 1] = rhs[1];
}

// ---- 2. the six sums per chunk, and the last arriver's fold into the ring -------------------------------------------------------
struct SumArgs {
  const float* x_backup;   // [N, 12]
  const float* uvp_dim;    // [B, 3]
  const float* theta;      // [B, ld_theta]: columns 3 and 4 are read
  int ld_theta;
  const float* pos;        // [N, 2]
  const float* fpos;       // [E, 2]
  const float* kS;         // [Sg, 2]
  const int* es;           // [E]
  const int* er;           // [E]
  const int* wface;        // [Nf, 4] = (f, k, ja, jb)
  const int* wchunk_beg;   // [n_wchunks]
  const int* wchunk_end;   // [n_wchunks]
  const int* gwchunk_ptr;  // [B + 1]
  int n_wchunks, Nf, B;
  const float* origin;     // [B, 2]
  const double* gb;        // [Nb, 3, 2]
  const int* clock;
  int* rec;
  double* partial;         // [n_wchunks, 6]
  double* hist;            // [keep, B, 6]
  int* hist_clock;         // [keep]
  int keep;
};

__global__ __launch_bounds__(WF_TPB) void wall_sum_kernel(const SumArgs A) {
  // ---- the record and the clock as the launch finds them: read by every thread before the arrival below ----------------------
  const int c = *A.clock;
  const int last = A.rec[GFV_WIN_LAST], n = A.rec[GFV_WIN_N];
  const bool take = gfv_window_take(A.rec, c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * (WF_TPB / 64) + wave;
  if (take && q < A.n_wchunks) {
    const int b = gfv_chunk_graph(A.gwchunk_ptr, A.B, q);
    const double th3 = (double)A.theta[(size_t)b * A.ld_theta + 3], th4 = (double)A.theta[(size_t)b * A.ld_theta + 4];
    const float dp = A.uvp_dim[3 * b + 2];
    const double ox = (double)A.origin[2 * b], oy = (double)A.origin[2 * b + 1];
    double s[GFV_WALL_FORCE_SUMS];
#pragma unroll
    for (int k = 0; k < GFV_WALL_FORCE_SUMS; ++k) s[k] = 0.0;
    const int beg = A.wchunk_beg[q], end = min(A.wchunk_end[q], A.Nf);
    for (int row = beg + lane; row < end; row += 64) {
      const int4 w = *reinterpret_cast<const int4*>(A.wface + (size_t)row * 4);
      const int f = w.x, ns = A.es[f], nr = A.er[f];
      const float fx = A.fpos[2 * f], fy = A.fpos[2 * f + 1];
      const float rsx = fx - A.pos[2 * ns], rsy = fy - A.pos[2 * ns + 1];       // (fp32, as face_fwd_kernel forms them)
      const float rrx = fx - A.pos[2 * nr], rry = fy - A.pos[2 * nr + 1];
      const double ps = (double)(A.x_backup[(size_t)ns * 12 + 2] / dp), pr = (double)(A.x_backup[(size_t)nr * 12 + 2] / dp);
      const double* ga = A.gb + (size_t)w.z * 6;                                // [c][a] of the sender, then of the receiver
      const double* gr = A.gb + (size_t)w.w * 6;
      const double Sx = (double)A.kS[2 * (size_t)w.y], Sy = (double)A.kS[2 * (size_t)w.y + 1];
      const double vs = ps + ((double)rsx * ga[4] + (double)rsy * ga[5]);
      const double vr = pr + ((double)rrx * gr[4] + (double)rry * gr[5]);
      const double pf = 0.5 * (vs + vr);
      const double fpx = (th3 * pf) * Sx, fpy = (th3 * pf) * Sy;
      const double gux = 0.5 * (ga[0] + gr[0]), guy = 0.5 * (ga[1] + gr[1]);
      const double gvx = 0.5 * (ga[2] + gr[2]), gvy = 0.5 * (ga[3] + gr[3]);
      const double fvx = -(th4 * (gux * Sx + guy * Sy)), fvy = -(th4 * (gvx * Sx + gvy * Sy));
      const double ax = (double)fx - ox, ay = (double)fy - oy;
      s[0] += fpx; s[1] += fpy; s[2] += fvx; s[3] += fvy;
      s[4] += ax * fpy - ay * fpx;
      s[5] += ax * fvy - ay * fvx;
    }
#pragma unroll
    for (int k = 0; k < GFV_WALL_FORCE_SUMS; ++k) s[k] = gfv_wave_sum(s[k]);
    if (lane < GFV_WALL_FORCE_SUMS) {
      double v = s[0];
#pragma unroll
      for (int k = 1; k < GFV_WALL_FORCE_SUMS; ++k) v = lane == k ? s[k] : v;
      A.partial[(size_t)q * GFV_WALL_FORCE_SUMS + lane] = v;
    }
  }
  if (!gfv_arrive_last_all_fence(A.rec + GFV_WIN_COUNTER)) return;
  // ---- the fold, per graph: every partial is in place -------------------------------------------------------------------------
  if (take) {
    const size_t slot = (size_t)((unsigned)n % (unsigned)A.keep);
    for (int b = wave; b < A.B; b += WF_TPB / 64) {
      double s[GFV_WALL_FORCE_SUMS];
      gfv_fold_chunks<GFV_WALL_FORCE_SUMS>(A.partial, A.gwchunk_ptr[b], min(A.gwchunk_ptr[b + 1], A.n_wchunks), lane, s);
#pragma unroll
      for (int k = 0; k < GFV_WALL_FORCE_SUMS; ++k) s[k] = gfv_wave_sum(s[k]);
      if (lane == 0) {
        double* h = A.hist + (slot * A.B + b) * GFV_WALL_FORCE_SUMS;
#pragma unroll
        for (int k = 0; k < GFV_WALL_FORCE_SUMS; ++k) h[k] = s[k];
      }
    }
    if (threadIdx.x == 0) A.hist_clock[slot] = c;
  }
  if (threadIdx.x == 0) gfv_window_commit(A.rec, c, last, n, take);
}

}  // namespace

extern "C" int gfv_wall_force_grad(const float* x_backup, const float* uvp_dim, const int32_t* batch, const int32_t* x_rowptr,
                                   const int32_t* x_out, const float* x_B, const float* An, const float* rn, const int32_t* bnode,
                                   int32_t Nb, int32_t terms, const int32_t* clock, const int32_t* rec, double* gb, void* stream) {
  if (!x_backup || !uvp_dim || !batch || !x_rowptr || !x_out || !x_B || !An || !rn || !bnode || !clock || !rec || !gb)
    return GFV_ERR_ARG;
  if (Nb < 1) return GFV_ERR_ARG;
  if (terms != 2 && terms != 5 && terms != 9 && terms != 14) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(x_backup) & 15) || (reinterpret_cast<size_t>(gb) & 7)) return GFV_ERR_ARG;
  // a launch that samples (the host cannot know), per node and channel: about ten stencil entries of (index 4 B, value 4 B, moment
  // vector), the matrix and its row norms, two doubles out
  GfvProfScope ps_(GFV_K_MISC, 0, 3.0 * Nb * (10.0 * (8.0 + 4.0 * terms) + 4.0 * terms * terms + 4.0 * terms + 16.0), stream);
  const dim3 grid(((long)Nb * 4 + WF_TPB - 1) / WF_TPB), block(WF_TPB);
#define WF_GRAD(MM)                                                                                                          \
  GFV_LAUNCH(wall_grad_kernel<MM>, grid, block, 0, (hipStream_t)stream, x_backup, uvp_dim, (const int*)batch,                \
             (const int*)x_rowptr, (const int*)x_out, x_B, An, rn, (const int*)bnode, (int)Nb, (const int*)clock,            \
             (const int*)rec, gb)
  if (terms == 2) WF_GRAD(2);
  else if (terms == 5) WF_GRAD(5);
  else if (terms == 9) WF_GRAD(9);
  else WF_GRAD(14);
#undef WF_GRAD
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_wall_force_sum(const float* x_backup, const float* uvp_dim, const float* theta, int32_t ld_theta,
                                  const float* pos, const float* fpos, const float* kS, const int32_t* es, const int32_t* er,
                                  const int32_t* wface, const int32_t* wchunk_beg, const int32_t* wchunk_end,
                                  const int32_t* gwchunk_ptr, int32_t n_wchunks, int32_t Nf, int32_t B, const float* origin,
                                  const double* gb, const int32_t* clock, int32_t* rec, double* partial, double* hist,
                                  int32_t* hist_clock, int32_t keep, void* stream) {
  if (!x_backup || !uvp_dim || !theta || !pos || !fpos || !kS || !es || !er || !wface || !wchunk_beg || !wchunk_end ||
      !gwchunk_ptr || !origin || !gb || !clock || !rec || !partial || !hist || !hist_clock)
    return GFV_ERR_ARG;
  if (n_wchunks < 1 || Nf < 1 || B < 1 || keep < 1 || ld_theta < 5) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(x_backup) & 15) || (reinterpret_cast<size_t>(wface) & 15)) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(gb) & 7) || (reinterpret_cast<size_t>(partial) & 7) || (reinterpret_cast<size_t>(hist) & 7))
    return GFV_ERR_ARG;
  SumArgs A;
  A.x_backup = x_backup; A.uvp_dim = uvp_dim; A.theta = theta; A.ld_theta = ld_theta; A.pos = pos; A.fpos = fpos; A.kS = kS;
  A.es = (const int*)es; A.er = (const int*)er; A.wface = (const int*)wface; A.wchunk_beg = (const int*)wchunk_beg;
  A.wchunk_end = (const int*)wchunk_end; A.gwchunk_ptr = (const int*)gwchunk_ptr; A.n_wchunks = n_wchunks; A.Nf = Nf; A.B = B;
  A.origin = origin; A.gb = gb; A.clock = (const int*)clock; A.rec = (int*)rec; A.partial = partial; A.hist = hist;
  A.hist_clock = (int*)hist_clock; A.keep = keep;
  // a launch that samples, per face: the table row, two end nodes of (index, position, pressure, six doubles), the face centre and
  // vector; per chunk six doubles out and in again
  GfvProfScope ps_(GFV_K_MISC, 0, (16.0 + 2.0 * (4.0 + 8.0 + 4.0 + 48.0) + 16.0) * Nf + 96.0 * n_wchunks, stream);
  GFV_LAUNCH(wall_sum_kernel, dim3((n_wchunks + WF_TPB / 64 - 1) / (WF_TPB / 64)), dim3(WF_TPB), 0, (hipStream_t)stream, A);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
