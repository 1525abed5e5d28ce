// Time march (gfv/march.py; the reference's solve_with_grad_GPU.py:133-209 with the --residual_tolerance /
// --max_inner_steps it declares and never wires up): ONE launch per training step, behind the backward and in front of the
// optimiser's launches, that decides ON THE DEVICE whether this inner iteration ends the open time level.
//
// With the record march[16] (include/gfv.h) AS THE LAUNCH FINDS IT - every workgroup reads it, r0 and the losses before anything
// is written; the workgroup that arrives last writes it (the discipline of grad_accum_kernel, csrc/misc.hip):
//   done set:      apply = 0, held += 1; nothing else changes (the Adam, guard and log launches behind it read apply == 0)
//   done not set:  apply = 1, seen += 1; r[b] = gfv_weighted_residual of graph b (the argument of the training loss's log);
//                  inner == 0: r0[b] = r[b];  conv[b] = (tol >= 0 && r[b] <= tol * r0[b]) || (abs_tol >= 0 && r[b] <= abs_tol)
//                  k = inner + 1;  latch = (all conv && k >= min_inner) || k >= max_inner
//     no latch:    inner = k.  No row of x_backup is read or written.
//     latch:       x_backup[:, 0:3] = uvp_node; x = x_backup; snap[level % keep] = uvp_node (keep > 0); history row `level`;
//                  inner = 0; level += 1; done = level >= target (or the history is full)
// Summation order of the two norms of a history row: csrc/gfv_reduce.h (rollout_advance's; no floating-point atomics).
// Arrival on march[7]: the all-fence form on a latching launch (the last arriver folds the others' partial sums), the no-data form
// otherwise (it reads nothing another workgroup wrote).  Which of the two is taken is the same in every workgroup: it follows from
// words that nobody writes before all have arrived.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"

namespace {

constexpr int MA_WAVES = 4, MA_TPB = 64 * MA_WAVES;
enum { MR_MAX_INNER = 0, MR_MIN_INNER = 1, MR_INNER = 2, MR_APPLY = 3, MR_TOL = 4, MR_ABS_TOL = 5, MR_LEVEL = 6, MR_COUNTER = 7,
       MR_TARGET = 8, MR_DONE = 9, MR_SEEN = 10, MR_HELD = 11, MR_KEEP = 12 };
static_assert(MR_APPLY == 3, "the Adam, guard and log launches read the apply word where accum[3] is");

struct MarchArgs {
  const float* uvp_node;      // [N,3]
  float* x_backup;            // [N,12]
  float* x;                   // [N,12]
  const int* chunk_beg;       // [n_chunks]
  const int* chunk_end;
  const int* gchunk_ptr;      // [B+1]
  const float* losses;        // [B,4]
  double* partial;            // [n_chunks,2]
  const float* hyper;         // [8]: 5, 6, 7 = w_cont, w_mom, w_press
  int* march;                 // [16]
  float* r0;                  // [B]
  unsigned* history;          // [max_levels, GFV_MARCH_HEAD + GFV_MARCH_GRAPH * B]
  float* snap;                // [keep_cap, N, 3] or NULL
  int* mirror;                // pinned, device-mapped: {seen, level, done}; or NULL
  int N, n_chunks, B, max_levels, keep_cap;
};

static __device__ __forceinline__ float march_residual(const MarchArgs& A, int b, float wc, float wm, float wp) {
  const float* l = A.losses + 4 * (size_t)b;
  return gfv_weighted_residual(l[0], l[1], l[2], l[3], wc, wm, wp);
}

static __device__ __forceinline__ void march_mirror(int* mirror, int seen, int level, int done) {
  if (!mirror) return;
  __hip_atomic_store(mirror + 1, level, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(mirror + 2, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(mirror, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(MA_TPB) void march_advance_kernel(const MarchArgs A) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int* rec = A.march;
  // ---- the record as the launch finds it: read by every thread before the arrival below --------------------------------------
  const int done = rec[MR_DONE], inner = rec[MR_INNER], level = rec[MR_LEVEL];
  const int max_inner = max(rec[MR_MAX_INNER], 1);
  const int min_inner = min(max(rec[MR_MIN_INNER], 1), max_inner);
  const float tol = __int_as_float(rec[MR_TOL]), abs_tol = __int_as_float(rec[MR_ABS_TOL]);
  const int keep = min(max(rec[MR_KEEP], 0), A.keep_cap);
  const float wc = A.hyper[5], wm = A.hyper[6], wp = A.hyper[7];
  int conv = 1;
  if (!done) {
    for (int b = tid; b < A.B; b += MA_TPB) {
      const float r = march_residual(A, b, wc, wm, wp);
      const float rb = inner == 0 ? r : A.r0[b];
      const float bound = tol * rb;                                   // (one fp32 rounding; a NaN compares false)
      conv &= ((tol >= 0.f && r <= bound) || (abs_tol >= 0.f && r <= abs_tol)) ? 1 : 0;
    }
  }
  const int all_conv = __syncthreads_and(conv);
  const int k = inner + 1;
  const bool converged = all_conv && k >= min_inner, capped = k >= max_inner;
  const bool latch = !done && (converged || capped);

  if (!latch) {
    if (!gfv_arrive_last_nodata(rec + MR_COUNTER)) return;            // (true on thread 0 of the last workgroup only)
    rec[MR_COUNTER] = 0;
    int seen = rec[MR_SEEN];
    if (done) {
      rec[MR_APPLY] = 0;
      rec[MR_HELD] += 1;
    } else {
      rec[MR_APPLY] = 1;
      seen += 1;
      rec[MR_SEEN] = seen;
      if (inner == 0)
        for (int b = 0; b < A.B; ++b) A.r0[b] = march_residual(A, b, wc, wm, wp);
      rec[MR_INNER] = k;
    }
    march_mirror(A.mirror, seen, level, done);
    return;
  }

  // ---- latch: the statements of TrainStep.advance_time() + the history row -----------------------------------------------------
  const bool room = level >= 0 && level < A.max_levels;
  float* snap = (keep > 0 && level >= 0) ? A.snap + (size_t)(level % keep) * (size_t)A.N * 3 : nullptr;
  const int c = blockIdx.x * MA_WAVES + wave;
  if (c < A.n_chunks) {
    const int beg = A.chunk_beg[c], end = min(A.chunk_end[c], A.N);
    double d2 = 0.0, n2 = 0.0;
    for (int i = beg + lane; i < end; i += 64) {
      if (i < 0) continue;
      const float4 u = gfv_advance_row(A.uvp_node, A.x_backup, A.x, i, true, d2, n2);
      if (snap) {
        float* s3 = snap + (size_t)i * 3;
        s3[0] = u.x; s3[1] = u.y; s3[2] = u.z;
      }
    }
    d2 = gfv_wave_sum(d2);
    n2 = gfv_wave_sum(n2);
    if (lane == 0) {
      A.partial[2 * (size_t)c] = d2;
      A.partial[2 * (size_t)c + 1] = n2;
    }
  }
  if (!gfv_arrive_last_all_fence(rec + MR_COUNTER)) return;
  const int row_words = GFV_MARCH_HEAD + GFV_MARCH_GRAPH * A.B;
  unsigned* row = A.history + (size_t)(room ? level : 0) * row_words;
  for (int b = wave; b < A.B; b += MA_WAVES) {
    const int c0 = A.gchunk_ptr[b], c1 = min(A.gchunk_ptr[b + 1], A.n_chunks);
    double s[2];
    gfv_fold_chunks(A.partial, c0, c1, lane, s);
    const double d2 = gfv_wave_sum(s[0]), n2 = gfv_wave_sum(s[1]);
    const float r = march_residual(A, b, wc, wm, wp);
    const float rb = inner == 0 ? r : A.r0[b];
    if (room) {
      unsigned* h = row + GFV_MARCH_HEAD + GFV_MARCH_GRAPH * b;
      if (lane < 4) h[lane] = __float_as_uint(A.losses[4 * b + lane]);
      if (lane == 4) h[4] = __float_as_uint(rb);
      if (lane == 5) h[5] = __float_as_uint(r);
      if (lane == 6) h[6] = __float_as_uint((float)sqrt(d2));
      if (lane == 7) h[7] = __float_as_uint((float)sqrt(n2));
    }
    if (inner == 0 && lane == 0) A.r0[b] = r;                          // (inner == 0: no lane read r0[b])
  }
  __syncthreads();
  if (tid == 0) {
    const int seen = rec[MR_SEEN] + 1, next = level + 1;
    const int now_done = (next >= rec[MR_TARGET] || next >= A.max_levels) ? 1 : 0;
    if (room) {
      row[0] = (unsigned)level;
      row[1] = (unsigned)k;
      row[2] = (converged ? GFV_MARCH_CONVERGED : 0u) | (capped ? GFV_MARCH_CAPPED : 0u);
      row[3] = (unsigned)seen;
      for (int w = 4; w < GFV_MARCH_HEAD; ++w) row[w] = 0u;
    }
    rec[MR_APPLY] = 1;
    rec[MR_SEEN] = seen;
    rec[MR_INNER] = 0;
    rec[MR_LEVEL] = next;
    rec[MR_DONE] = now_done;
    rec[MR_COUNTER] = 0;
    march_mirror(A.mirror, seen, next, now_done);
  }
}

}  // namespace

extern "C" int gfv_march_advance(const float* uvp_node, float* x_backup, float* x, int32_t N, const int32_t* chunk_beg,
                                 const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B,
                                 const float* losses, double* partial_ws, const float* hyper, int32_t* march, float* r0,
                                 void* history, int32_t max_levels, int32_t max_inner, int32_t min_inner, float* snap, int32_t keep,
                                 int32_t* mirror_dev, void* stream) {
  if (!uvp_node || !x_backup || !x || !chunk_beg || !chunk_end || !gchunk_ptr || !losses || !partial_ws || !hyper || !march ||
      !r0 || !history || (keep > 0 && !snap))
    return GFV_ERR_ARG;
  if (N <= 0 || n_chunks <= 0 || B <= 0 || max_levels <= 0 || keep < 0) return GFV_ERR_ARG;
  if (max_inner < 1 || min_inner < 1 || min_inner > max_inner) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(x_backup) | reinterpret_cast<size_t>(x)) & 15) return GFV_ERR_ARG;
  // What the host can know of the traffic: a launch that does not latch reads the record, the weights, the losses and r0; one that
  // latches moves gfv_rollout_advance's rows (+ 12 N per snapshot).  Only with max_inner == 1 is every live launch a latching one.
  const double small = 64.0 + 32.0 + 20.0 * B, rows = (12.0 + 48.0 + 16.0 + 48.0 + (keep > 0 ? 12.0 : 0.0)) * N;
  GfvProfScope ps_(GFV_K_MISC, 0, max_inner == 1 ? rows + small : small, stream);
  const MarchArgs a{uvp_node, x_backup, x, chunk_beg, chunk_end, gchunk_ptr, losses, partial_ws, hyper, march, r0,
                    static_cast<unsigned*>(history), snap, mirror_dev, N, n_chunks, B, max_levels, keep};
  GFV_LAUNCH(march_advance_kernel, dim3((n_chunks + MA_WAVES - 1) / MA_WAVES), dim3(MA_TPB), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
