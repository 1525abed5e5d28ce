// The end of a forward-only rollout step (gfv/rollout.py; the reference's solve_without_grad_GPU.py:117-173) as ONE launch:
//   x_backup[:, 0:3] = uvp_node;  x = x_backup            the write-back of the predicted field and the restore of the
//                                                         un-normalised node state the next step's input preparation reads
//   history[k, b, 0:4] = losses[b, 0:4]                   the step's four residual losses
//   history[k, b, 4]   = || uvp_new - uvp_prev ||_2       over the nodes of graph b (uvp_prev: what x_backup[:, 0:3] held)
//   history[k, b, 5]   = || uvp_new ||_2
//   k = state[0], advanced by the launch itself (state[0] = k + 1), so that one recorded launch list replays K times.
// Summation order: csrc/gfv_reduce.h (the arrival counter is state[1], left at zero; all-fence form).
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"

namespace {

constexpr int RO_WAVES = 4;

struct RolloutArgs {
  const float* uvp_node;      // [N,3]
  float* x_backup;            // [N,12]
  float* x;                   // [N,12]
  const int* chunk_beg;       // [n_chunks]
  const int* chunk_end;
  const int* gchunk_ptr;      // [B+1]
  const float* losses;        // [B,4]
  double* partial;            // [n_chunks,2]
  float* history;             // [K_max,B,6]
  int* state;                 // [2]: step counter, arrival counter
  int N, n_chunks, B, K_max;
};

__global__ __launch_bounds__(64 * RO_WAVES) void rollout_advance_kernel(const RolloutArgs A) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.x * RO_WAVES + wave;
  if (c < A.n_chunks) {
    const int beg = A.chunk_beg[c], end = min(A.chunk_end[c], A.N);
    double d2 = 0.0, n2 = 0.0;
    for (int i = beg + lane; i < end; i += 64) {
      if (i < 0) continue;
      gfv_advance_row(A.uvp_node, A.x_backup, A.x, i, true, d2, n2);
    }
    d2 = gfv_wave_sum(d2);
    n2 = gfv_wave_sum(n2);
    if (lane == 0) {
      A.partial[2 * (size_t)c] = d2;
      A.partial[2 * (size_t)c + 1] = n2;
    }
  }
  if (!gfv_arrive_last_all_fence(A.state + 1)) return;
  const int k = gfv_ld_agent(A.state);
  const bool room = k >= 0 && k < A.K_max;   // (a full history is not written past: the host raises before it comes to that)
  for (int b = wave; b < A.B && room; b += RO_WAVES) {
    const int c0 = A.gchunk_ptr[b], c1 = min(A.gchunk_ptr[b + 1], A.n_chunks);
    double s[2];
    gfv_fold_chunks(A.partial, c0, c1, lane, s);
    const double d2 = gfv_wave_sum(s[0]), n2 = gfv_wave_sum(s[1]);
    float* h = A.history + ((size_t)k * A.B + b) * 6;
    if (lane < 4) h[lane] = A.losses[4 * b + lane];
    if (lane == 4) h[4] = (float)sqrt(d2);
    if (lane == 5) h[5] = (float)sqrt(n2);
  }
  __syncthreads();
  // (per-lane vector stores of the two counters)
  if (tid == 0) {
    if (room) A.state[0] = k + 1;
    A.state[1] = 0;
  }
}

}  // namespace

extern "C" int gfv_rollout_advance(const float* uvp_node, float* x_backup, float* x, int32_t N, const int32_t* chunk_beg,
                                   const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B,
                                   const float* losses, double* partial_ws, float* history, int32_t K_max, int32_t* state,
                                   void* stream) {
  if (!uvp_node || !x_backup || !x || !chunk_beg || !chunk_end || !gchunk_ptr || !losses || !partial_ws || !history || !state)
    return GFV_ERR_ARG;
  if (N <= 0 || n_chunks <= 0 || B <= 0 || K_max <= 0) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(x_backup) | reinterpret_cast<size_t>(x)) & 15) return GFV_ERR_ARG;
  // rows: uvp [N,3] read, x_backup [N,12] read, 16 B of it and x [N,12] written
  GfvProfScope ps_(GFV_K_MISC, 0, (12.0 + 48.0 + 16.0 + 48.0) * N, stream);
  const RolloutArgs a{uvp_node, x_backup, x, chunk_beg, chunk_end, gchunk_ptr, losses, partial_ws, history, state, N, n_chunks, B, K_max};
  GFV_LAUNCH(rollout_advance_kernel, dim3((n_chunks + RO_WAVES - 1) / RO_WAVES), dim3(64 * RO_WAVES), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
