// Evaluation over a device pool (gfv/evaluate.py): what a forward-only step over one batch says about each of its graphs, as ONE
// launch behind the step - a 16-float record per graph, written to the row of the graph's POOL ENTRY in a table [n_entries, 16]:
//   0-3    losses[b, 0:4] (cont, mom_x, mom_y, press), bit copies
//   4-6    || pred - cur ||_2 per channel u, v, p     pred = uvp_node, cur = x_raw[:, 0:3] (the entry's own state)
//   7-9    || pred ||_2
//   10-12  || pred - tgt ||_2                          NaN for a graph without a target (target3 is then not read at all)
//   13-15  || tgt ||_2                                 NaN likewise
// The entry of every graph and its "has a target" bit travel by value in the launch's argument block (as the indices of
// gfv_pool_assemble do: a buffer the host rewrites for the next batch would race with a launch that is still queued), so the
// launch is issued eagerly behind a replayed step and is never part of a recorded list.
// Summation order: csrc/gfv_reduce.h (twelve sums per chunk; the arrival counter is left at zero; all-fence form).
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"

namespace {

constexpr int EV_WAVES = 4;
constexpr int EV_SUMS = 12;
constexpr int MAXB = GFV_POOL_MAX_GRAPHS;
static_assert(MAXB <= 64, "the target flags of a batch are one 64-bit mask");
static_assert(GFV_EVAL_RECORD == 16, "the fold writes one lane per column");

struct EvalArgs {
  const float* uvp_node;      // [N,3]
  const float* x_raw;         // [N,12]
  const float* target3;       // [N,3], read only over the graphs whose bit is set
  const int* chunk_beg;       // [n_chunks]
  const int* chunk_end;
  const int* gchunk_ptr;      // [B+1]
  const float* losses;        // [B,4]
  float* table;               // [n_entries,16]
  double* partial;            // [n_chunks,12]
  int* counter;               // arrival counter
  int N, n_chunks, B;
  unsigned long long has_target;
  int entry[MAXB];
};

__global__ __launch_bounds__(64 * EV_WAVES) void eval_collect_kernel(const EvalArgs A) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.x * EV_WAVES + wave;
  if (c < A.n_chunks) {
    const int b = gfv_chunk_graph(A.gchunk_ptr, A.B, c);
    const bool tgt = (A.has_target >> b) & 1ull;
    const int beg = A.chunk_beg[c], end = min(A.chunk_end[c], A.N);
    double s[EV_SUMS];
#pragma unroll
    for (int k = 0; k < EV_SUMS; ++k) s[k] = 0.0;
    for (int i = beg + lane; i < end; i += 64) {
      if (i < 0) continue;
      const float4 r0 = *reinterpret_cast<const float4*>(A.x_raw + (size_t)i * 12);
      const float* u = A.uvp_node + (size_t)i * 3;
      const float u0 = u[0], u1 = u[1], u2 = u[2];
      const float e0 = u0 - r0.x, e1 = u1 - r0.y, e2 = u2 - r0.z;
      s[0] += (double)e0 * (double)e0; s[1] += (double)e1 * (double)e1; s[2] += (double)e2 * (double)e2;
      s[3] += (double)u0 * (double)u0; s[4] += (double)u1 * (double)u1; s[5] += (double)u2 * (double)u2;
      if (tgt) {
        const float* t = A.target3 + (size_t)i * 3;
        const float t0 = t[0], t1 = t[1], t2 = t[2];
        const float f0 = u0 - t0, f1 = u1 - t1, f2 = u2 - t2;
        s[6] += (double)f0 * (double)f0; s[7] += (double)f1 * (double)f1; s[8] += (double)f2 * (double)f2;
        s[9] += (double)t0 * (double)t0; s[10] += (double)t1 * (double)t1; s[11] += (double)t2 * (double)t2;
      }
    }
#pragma unroll
    for (int k = 0; k < EV_SUMS; ++k) s[k] = gfv_wave_sum(s[k]);
    if (lane == 0) {
      double* p = A.partial + (size_t)EV_SUMS * c;
#pragma unroll
      for (int k = 0; k < EV_SUMS; ++k) p[k] = s[k];
    }
  }
  if (!gfv_arrive_last_all_fence(A.counter)) return;
  for (int b = wave; b < A.B; b += EV_WAVES) {
    const int c0 = A.gchunk_ptr[b], c1 = min(A.gchunk_ptr[b + 1], A.n_chunks);
    const bool tgt = (A.has_target >> b) & 1ull;
    double s[EV_SUMS];
    gfv_fold_chunks(A.partial, c0, c1, lane, s);
    double mine = 0.0;          // lane 4 + k keeps sum k
#pragma unroll
    for (int k = 0; k < EV_SUMS; ++k) {
      const double v = gfv_wave_sum(s[k]);
      if (lane == 4 + k) mine = v;
    }
    // (per-lane vector stores: one lane per column of the record)
    if (lane < GFV_EVAL_RECORD) {
      unsigned* row = reinterpret_cast<unsigned*>(A.table + (size_t)GFV_EVAL_RECORD * A.entry[b]);
      unsigned bits;
      if (lane < 4) bits = reinterpret_cast<const unsigned*>(A.losses)[4 * b + lane];
      else if (lane >= 10 && !tgt) bits = 0x7fc00000u;
      else bits = __float_as_uint((float)sqrt(mine));
      row[lane] = bits;
    }
  }
  __syncthreads();
  if (tid == 0) *A.counter = 0;
}

}  // namespace

extern "C" int gfv_eval_collect(const float* uvp_node, const float* x_raw, const float* target3, int32_t N,
                                const int32_t* chunk_beg, const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks,
                                int32_t B, const float* losses, const int32_t* entry, const int32_t* has_target,
                                float* table, int32_t n_entries, double* partial_ws, int32_t* counter, void* stream) {
  if (!uvp_node || !x_raw || !chunk_beg || !chunk_end || !gchunk_ptr || !losses || !entry || !has_target || !table ||
      !partial_ws || !counter)
    return GFV_ERR_ARG;
  if (N <= 0 || n_chunks <= 0 || B <= 0 || B > MAXB || n_entries <= 0) return GFV_ERR_ARG;
  if (reinterpret_cast<size_t>(x_raw) & 15) return GFV_ERR_ARG;
  EvalArgs a{uvp_node, x_raw, target3, chunk_beg, chunk_end, gchunk_ptr, losses, table, partial_ws, counter, N, n_chunks, B, 0ull, {}};
  for (int b = 0; b < B; ++b) {
    if (entry[b] < 0 || entry[b] >= n_entries) return GFV_ERR_ARG;
    for (int q = 0; q < b; ++q)
      if (entry[q] == entry[b]) return GFV_ERR_ARG;        // one writer per row of the table
    a.entry[b] = entry[b];
    if (has_target[b]) a.has_target |= 1ull << b;
  }
  if (a.has_target && !target3) return GFV_ERR_ARG;
  // rows: uvp [N,3] read, 16 B of x_raw [N,12] read, target3 [N,3] read over the graphs that have one (the node counts of the
  // graphs are on the device: with any flag set every row is priced with a target - an upper bound)
  GfvProfScope ps_(GFV_K_MISC, 0, (12.0 + 16.0 + (a.has_target ? 12.0 : 0.0)) * N, stream);
  GFV_LAUNCH(eval_collect_kernel, dim3((n_chunks + EV_WAVES - 1) / EV_WAVES), dim3(64 * EV_WAVES), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
