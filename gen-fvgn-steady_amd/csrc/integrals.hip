// Flow integrals (gfv/integrals.py): the kinetic energy, the enstrophy, the norms of the discrete divergence and the
// balance of inflow against outflow of a run, per graph and per sampled field, summed on the device; optionally the cell vorticity
// and the cell divergence of the sampled field.  ONE launch behind the launch that advances the field (gfv_rollout_advance,
// gfv_march_advance); it follows the clock word that launch writes and reads it, and the record rec[8] (the window: include/gfv.h
// GFV_WINDOW_RECORD, gfv_window.h), as it finds them:
//   c = *clock;  take = gfv_window_take(rec, c)
//
//   gfv_flow_integrals    one wave per chunk of at most 64 cells (never across a graph): per cell the closed-polygon sums over its
//                         incidences - D = sum u_f . S, Gamma = sum (v_f S.x - u_f S.y), u_f the mean of the face's two ends - and
//                         the mean of the vertices, all in double from the fp32 data (no gradient, no LU); lane l adds the ten
//                         terms of the cells beg + l, beg + l + 64, ... in ascending order and takes fmax of the two others, the
//                         64 lane values fold by gfv_wave_sum (the maxima: the same exchanges with fmax), twelve doubles per chunk go to partial
//                         [n_cchunks, 12].  The workgroup that arrives last (all-fence form: the partials are plain stores of
//                         twelve lanes of other workgroups' waves) folds them per graph (gfv_fold_chunks<10, 12>, the maxima by
//                         the same walk with fmax, then the butterflies) into the ring's row n % keep, then gfv_window_commit.
// take false: no word of partial, hist, hist_clock or cell_out moves.  No floating-point atomics, no sum across graphs, an order
// that does not depend on the grid: the same inputs give the same bits.  The rule in full: include/gfv.h.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"
#include "gfv_window.h"

namespace {

constexpr int FI_TPB = 256;
constexpr int FI_WAVES = FI_TPB / 64;
constexpr int FI_COLS = GFV_FLOW_SUMS + GFV_FLOW_MAXS;
static_assert(GFV_FLOW_SUMS == 10 && GFV_FLOW_MAXS == 2 && GFV_FLOW_CHUNK == 64 && GFV_FLOW_RECORD == GFV_WINDOW_RECORD,
              "include/gfv.h");

// maximum over the 64 lanes of a wave in double, by gfv_wave_sum's exchanges (every lane gets the result, the same bits)
static __device__ __forceinline__ double wave_fmax(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

struct FlowArgs {
  const float* x_backup;   // [N, 12]
  const float* uvp_dim;    // [B, 3]
  const int* crow;         // [C + 1]
  const int* kface;        // [Sg]
  const int* knode;        // [Sg]
  const float* kS;         // [Sg, 2]
  const int* btype;        // [Sg]
  const int* es;           // [E]
  const int* er;           // [E]
  const float* area;       // [C]
  const int* cchunk_beg;   // [n_cchunks]
  const int* cchunk_end;   // [n_cchunks]
  const int* gcchunk_ptr;  // [B + 1]
  int n_cchunks, C, B;
  const int* clock;
  int* rec;
  double* partial;         // [n_cchunks, 12]
  double* hist;            // [keep, B, 12]
  int* hist_clock;         // [keep]
  int keep;
  double* cell_out;        // [C, 2] or NULL
};

__global__ __launch_bounds__(FI_TPB) void flow_integrals_kernel(const FlowArgs A) {
  // ---- the record and the clock as the launch finds them: read by every thread before the arrival below ----------------------
  const int c = *A.clock;
  const int last = A.rec[GFV_WIN_LAST], n = A.rec[GFV_WIN_N];
  const bool take = gfv_window_take(A.rec, c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * FI_WAVES + wave;
  if (take && q < A.n_cchunks) {
    const int b = gfv_chunk_graph(A.gcchunk_ptr, A.B, q);
    const float du = A.uvp_dim[3 * b], dv = A.uvp_dim[3 * b + 1], dp = A.uvp_dim[3 * b + 2];   // (a cell's nodes lie in its graph)
    double s[GFV_FLOW_SUMS], mx[GFV_FLOW_MAXS];
#pragma unroll
    for (int k = 0; k < GFV_FLOW_SUMS; ++k) s[k] = 0.0;
#pragma unroll
    for (int k = 0; k < GFV_FLOW_MAXS; ++k) mx[k] = 0.0;
    const int beg = A.cchunk_beg[q], end = min(A.cchunk_end[q], A.C);
    for (int cell = beg + lane; cell < end; cell += 64) {
      const int k0 = A.crow[cell], k1 = A.crow[cell + 1];
      double D = 0.0, G = 0.0, su = 0.0, sv = 0.0, sp = 0.0, fin = 0.0, fout = 0.0, foth = 0.0;
      for (int k = k0; k < k1; ++k) {
        const int f = A.kface[k], nv = A.knode[k], bt = A.btype[k];
        const int ns = A.es[f], nr = A.er[f];
        const float2 S = *reinterpret_cast<const float2*>(A.kS + 2 * (size_t)k);
        const float4 rs = *reinterpret_cast<const float4*>(A.x_backup + (size_t)ns * 12);
        const float4 rr = *reinterpret_cast<const float4*>(A.x_backup + (size_t)nr * 12);
        const float4 rv = *reinterpret_cast<const float4*>(A.x_backup + (size_t)nv * 12);
        const double us = (double)(rs.x / du), vs = (double)(rs.y / dv);
        const double ur = (double)(rr.x / du), vr = (double)(rr.y / dv);
        const double uf = 0.5 * (us + ur), vf = 0.5 * (vs + vr);
        const double Sx = (double)S.x, Sy = (double)S.y;
        const double d = uf * Sx + vf * Sy;
        const double g = vf * Sx - uf * Sy;
        D += d;
        G += g;
        su += (double)(rv.x / du);
        sv += (double)(rv.y / dv);
        sp += (double)(rv.z / dp);
        fin += bt == 1 ? d : 0.0;       // (a sum that starts from +0.0 is never -0.0: adding +0.0 leaves its bits)
        fout += bt == 2 ? d : 0.0;
        foth += bt == 3 ? d : 0.0;
      }
      const double nn = (double)(k1 - k0);
      const double ubar = su / nn, vbar = sv / nn, pbar = sp / nn;
      const double a = (double)A.area[cell];
      s[0] += a;
      s[1] += (0.5 * (ubar * ubar + vbar * vbar)) * a;
      s[2] += (0.5 * (G * G)) / a;
      s[3] += (D * D) / a;
      s[4] += D;
      s[5] += G;
      s[6] += pbar * a;
      s[7] += fin;
      s[8] += fout;
      s[9] += foth;
      mx[0] = fmax(mx[0], fabs(D) / a);
      mx[1] = fmax(mx[1], fabs(G) / a);
      if (A.cell_out) {
        A.cell_out[2 * (size_t)cell] = G / a;
        A.cell_out[2 * (size_t)cell + 1] = D / a;
      }
    }
#pragma unroll
    for (int k = 0; k < GFV_FLOW_SUMS; ++k) s[k] = gfv_wave_sum(s[k]);
#pragma unroll
    for (int k = 0; k < GFV_FLOW_MAXS; ++k) mx[k] = wave_fmax(mx[k]);
    if (lane < FI_COLS) {
      double v = s[0];
#pragma unroll
      for (int k = 1; k < GFV_FLOW_SUMS; ++k) v = lane == k ? s[k] : v;
#pragma unroll
      for (int k = 0; k < GFV_FLOW_MAXS; ++k) v = lane == GFV_FLOW_SUMS + k ? mx[k] : v;
      A.partial[(size_t)q * FI_COLS + lane] = v;
    }
  }
  if (!gfv_arrive_last_all_fence(A.rec + GFV_WIN_COUNTER)) return;
  // ---- the fold, per graph: every partial is in place -------------------------------------------------------------------------
  if (take) {
    const size_t slot = (size_t)((unsigned)n % (unsigned)A.keep);
    for (int b = wave; b < A.B; b += FI_WAVES) {
      const int c0 = A.gcchunk_ptr[b], c1 = min(A.gcchunk_ptr[b + 1], A.n_cchunks);
      double s[GFV_FLOW_SUMS], mx[GFV_FLOW_MAXS];
      gfv_fold_chunks<GFV_FLOW_SUMS, FI_COLS>(A.partial, c0, c1, lane, s);
#pragma unroll
      for (int k = 0; k < GFV_FLOW_MAXS; ++k) mx[k] = 0.0;
      for (int j = c0 + lane; j < c1; j += 64) {
#pragma unroll
        for (int k = 0; k < GFV_FLOW_MAXS; ++k)
          mx[k] = fmax(mx[k], gfv_ld_agent(A.partial + (size_t)FI_COLS * j + GFV_FLOW_SUMS + k));
      }
#pragma unroll
      for (int k = 0; k < GFV_FLOW_SUMS; ++k) s[k] = gfv_wave_sum(s[k]);
#pragma unroll
      for (int k = 0; k < GFV_FLOW_MAXS; ++k) mx[k] = wave_fmax(mx[k]);
      if (lane == 0) {
        double* h = A.hist + (slot * A.B + b) * FI_COLS;
#pragma unroll
        for (int k = 0; k < GFV_FLOW_SUMS; ++k) h[k] = s[k];
#pragma unroll
        for (int k = 0; k < GFV_FLOW_MAXS; ++k) h[GFV_FLOW_SUMS + k] = mx[k];
      }
    }
    if (threadIdx.x == 0) A.hist_clock[slot] = c;
  }
  if (threadIdx.x == 0) gfv_window_commit(A.rec, c, last, n, take);
}

}  // namespace

extern "C" int gfv_flow_integrals(const float* x_backup, const float* uvp_dim, const int32_t* crow, const int32_t* kface,
                                  const int32_t* knode, const float* kS, const int32_t* btype, const int32_t* es,
                                  const int32_t* er, const float* area, const int32_t* cchunk_beg, const int32_t* cchunk_end,
                                  const int32_t* gcchunk_ptr, int32_t n_cchunks, int32_t C, int32_t B, const int32_t* clock,
                                  int32_t* rec, double* partial, double* hist, int32_t* hist_clock, int32_t keep, double* cell_out,
                                  void* stream) {
  if (!x_backup || !uvp_dim || !crow || !kface || !knode || !kS || !btype || !es || !er || !area || !cchunk_beg || !cchunk_end ||
      !gcchunk_ptr || !clock || !rec || !partial || !hist || !hist_clock)
    return GFV_ERR_ARG;
  if (n_cchunks < 1 || C < 1 || B < 1 || keep < 1) return GFV_ERR_ARG;
  if (reinterpret_cast<size_t>(x_backup) & 15) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(kS) & 7) || (reinterpret_cast<size_t>(partial) & 7) || (reinterpret_cast<size_t>(hist) & 7) || (reinterpret_cast<size_t>(cell_out) & 7))
    return GFV_ERR_ARG;
  FlowArgs A;
  A.x_backup = x_backup; A.uvp_dim = uvp_dim; A.crow = (const int*)crow; A.kface = (const int*)kface; A.knode = (const int*)knode;
  A.kS = kS; A.btype = (const int*)btype; A.es = (const int*)es; A.er = (const int*)er; A.area = area;
  A.cchunk_beg = (const int*)cchunk_beg; A.cchunk_end = (const int*)cchunk_end; A.gcchunk_ptr = (const int*)gcchunk_ptr;
  A.n_cchunks = n_cchunks; A.C = C; A.B = B; A.clock = (const int*)clock; A.rec = (int*)rec; A.partial = partial; A.hist = hist;
  A.hist_clock = (int*)hist_clock; A.keep = keep; A.cell_out = cell_out;
  // a launch that samples (the host cannot know; nor the tables' length: about four incidences per cell), per incidence the face,
  // the vertex, the type, two end indices, the vector and 16 B of three rows; per cell the row pointer, the area and two doubles
  // out; per chunk twelve doubles out and in again
  GfvProfScope ps_(GFV_K_MISC, 0, (4.0 * (12.0 + 8.0 + 8.0 + 48.0) + 8.0 + (cell_out ? 16.0 : 0.0)) * C + 192.0 * n_cchunks, stream);
  GFV_LAUNCH(flow_integrals_kernel, dim3((n_cchunks + FI_WAVES - 1) / FI_WAVES), dim3(FI_TPB), 0, (hipStream_t)stream, A);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
