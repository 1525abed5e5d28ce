// The end of a forward-only rollout step (gfv/rollout.py; the reference's solve_without_grad_GPU.py:117-173) as ONE launch:
//   x_backup[:, 0:3] = uvp_node;  x = x_backup            the write-back of the predicted field and the restore of the
//                                                         un-normalised node state the next step's input preparation reads
//   history[k, b, 0:4] = losses[b, 0:4]                   the step's four residual losses
//   history[k, b, 4]   = || uvp_new - uvp_prev ||_2       over the nodes of graph b (uvp_prev: what x_backup[:, 0:3] held)
//   history[k, b, 5]   = || uvp_new ||_2
//   k = state[0], advanced by the launch itself (state[0] = k + 1), so that one recorded launch list replays K times.
// Summation order (fixed, independent of the grid and of timing): the node chunks of the plan (at most a few dozen rows each,
// never across a graph) - one wave per chunk, a lane sums its rows in ascending order in double, the 64 lanes fold by a xor
// butterfly; the workgroup that arrives last (an integer arrival counter, state[1], left at zero) folds the chunks of each graph:
// lane l takes chunks l, l + 64, ... in ascending order, then the same butterfly.  No floating-point atomics.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"

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

__device__ __forceinline__ double ro_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(64 * RO_WAVES) void rollout_advance_kernel(const RolloutArgs A) {
  __shared__ int s_last;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.x * RO_WAVES + wave;
  if (c < A.n_chunks) {
    const int beg = A.chunk_beg[c], end = min(A.chunk_end[c], A.N);
    double d2 = 0.0, n2 = 0.0;
    for (int i = beg + lane; i < end; i += 64) {
      if (i < 0) continue;
      const float* u = A.uvp_node + (size_t)i * 3;
      const float u0 = u[0], u1 = u[1], u2 = u[2];
      float4* xb = reinterpret_cast<float4*>(A.x_backup + (size_t)i * 12);
      float4* xo = reinterpret_cast<float4*>(A.x + (size_t)i * 12);
      float4 r0 = xb[0];
      const float4 r1 = xb[1], r2 = xb[2];
      const float e0 = u0 - r0.x, e1 = u1 - r0.y, e2 = u2 - r0.z;
      d2 += ((double)e0 * (double)e0 + (double)e1 * (double)e1) + (double)e2 * (double)e2;
      n2 += ((double)u0 * (double)u0 + (double)u1 * (double)u1) + (double)u2 * (double)u2;
      r0.x = u0; r0.y = u1; r0.z = u2;
      xb[0] = r0;
      xo[0] = r0; xo[1] = r1; xo[2] = r2;
    }
    d2 = ro_wave_sum(d2);
    n2 = ro_wave_sum(n2);
    if (lane == 0) {
      A.partial[2 * (size_t)c] = d2;
      A.partial[2 * (size_t)c + 1] = n2;
    }
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) s_last = atomicAdd(A.state + 1, 1) == (int)gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  const int k = __hip_atomic_load(A.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool room = k >= 0 && k < A.K_max;   // (a full history is not written past: the host raises before it comes to that)
  for (int b = wave; b < A.B && room; b += RO_WAVES) {
    const int c0 = A.gchunk_ptr[b], c1 = min(A.gchunk_ptr[b + 1], A.n_chunks);
    double d2 = 0.0, n2 = 0.0;
    for (int q = c0 + lane; q < c1; q += 64) {
      d2 += __hip_atomic_load(A.partial + 2 * (size_t)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      n2 += __hip_atomic_load(A.partial + 2 * (size_t)q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    d2 = ro_wave_sum(d2);
    n2 = ro_wave_sum(n2);
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
