// Chunk sums and last-arriver folds: what the kernels that end in "every workgroup leaves double partial sums, the workgroup that
// arrives last folds them" share - the wave butterfly, the loads that bypass the L1, the arrival on an integer counter in each of
// the four forms in use (DESIGN.md 5m says which kernel uses which, and why), the fold of per-chunk partials, and the per-row body
// of a rollout / sweep step.  Device inline functions only.
//
// Summation order (rollout_advance, sweep_advance, eval_collect, anderson_gram; tests/chunk_sums_ref.py restates it in numpy and
// tests/test_chunk_sums_gpu.py compares bit for bit).  Fixed, independent of the grid, of timing and of a graph's neighbours in
// the batch; no floating-point atomics, so the same inputs give the same bits run after run:
//   * per row: differences in fp32, squares, products and every sum in double; where a sum is over the three channels of a row
//     it is grouped ((c0 + c1) + c2);
//   * per chunk of the plan (rows chunk_beg[c] .. min(chunk_end[c], N) - 1; at most a few dozen rows, never across a graph): one
//     wave; lane l adds the rows beg + l, beg + l + 64, ... in ascending order, starting from +0.0; the 64 lane sums fold by a
//     xor butterfly, levels 32, 16, ... 1 (gfv_wave_sum; Anderson's aa_tree_sum forms the same tree in LDS); one double per
//     chunk and sum is left in the launch's workspace;
//   * per graph, by the workgroup that arrives last (chunks gchunk_ptr[b] .. min(gchunk_ptr[b + 1], n_chunks) - 1): one wave;
//     lane l adds the chunk sums c0 + l, c0 + l + 64, ... in ascending order (gfv_fold_chunks), then the same butterfly;
//   * a norm is the square root of the graph's sum in double, rounded to fp32 once.
#pragma once
#include "gfv_common.h"

// sum over the 64 lanes of a wave in double: v[l] += v[l ^ o], o = 32, 16, ... 1 (every lane gets the result, the same bits)
static __device__ __forceinline__ double gfv_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// maximum by the same exchanges (gfv_wave_max of gfv_common.h pairs the lanes in another order: not shown equal for NaNs and -0)
static __device__ __forceinline__ float gfv_wave_max_shfl(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// A load that another workgroup's store of THIS launch may have produced: agent scope, served by the L2 (it bypasses this CU's
// L1, which no other CU's store refreshes).  gfv_st_agent is the matching write-through store.
template <typename T>
static __device__ __forceinline__ T gfv_ld_agent(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
static __device__ __forceinline__ void gfv_st_agent(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the graph that owns chunk c (gchunk_ptr [B + 1] ascending; a chunk never crosses a graph)
static __device__ __forceinline__ int gfv_chunk_graph(const int* gchunk_ptr, int B, int c) {
  int b = 0;
  while (b < B - 1 && gchunk_ptr[b + 1] <= c) ++b;
  return b;
}

// ---- arrival on an integer counter: "is this workgroup the last to arrive?" ---------------------------------------------------
// One function per form.  The calling rule of all four: EVERY thread of the workgroup calls it, outside divergent control flow
// (each contains __syncthreads()); the counter is zero when the launch starts and whoever is last puts it back to zero after its
// fold.  All workgroups of a one-dimensional grid arrive on one counter, except where a count n is given.  The rule they follow
// (cdna_hip_programming.md, Guideline 16; a CU's L1 is never refreshed by another CU's stores, the XCDs' L2s are not coherent):
// an agent-scope release by the producer before the counter says so, an agent-scope acquire - or only loads that bypass the L1 -
// by the consumer after it.

// All-fence (Guideline 16's rule with plain stores: release and acquire are both in __threadfence()): every thread fences, then
// the leader counts.
//   before: any thread of the workgroup may have made the stores to hand over, plain stores included;
//   after (true, block-uniform): every workgroup's stores are visible behind the trailing fence (the folds still use gfv_ld_agent).
static __device__ __forceinline__ bool gfv_arrive_last_all_fence(int* counter) {
  __shared__ int s_last;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(counter, 1) == (int)gridDim.x - 1;
  __syncthreads();
  if (!s_last) return false;
  __threadfence();
  return true;
}

// Leader-fence (Guideline 16: one lane's release covers stores that a barrier ordered before it): the leader alone fences, counts.
//   before: the stores to hand over are thread 0's own, or are ordered before this call by a __syncthreads() of the caller;
//   n workgroups arrive on this counter; `enabled` (block-uniform) false: nothing is counted and nobody is last;
//   after (true, block-uniform): as the all-fence form.
static __device__ __forceinline__ bool gfv_arrive_last_leader_fence(int* counter, int n, bool enabled = true) {
  __shared__ int s_last;
  if (threadIdx.x == 0) {
    s_last = 0;
    if (enabled) {
      __threadfence();
      s_last = atomicAdd(counter, 1) == n - 1;
    }
  }
  __syncthreads();
  if (!s_last) return false;
  __threadfence();
  return true;
}

// Write-through (Guideline 16, recipe R1, with L1-bypassing loads in place of the acquire): no fence at all (a release fence
// writes back the L2's dirty lines - behind a backward that is the whole gradient).
//   before: every byte to hand over was stored by thread 0 with gfv_st_agent; this call waits for those stores (vmcnt) before
//   it counts;
//   after (true, block-uniform): the others' bytes may be read with gfv_ld_agent ONLY - a plain load may hit a stale L1 line.
static __device__ __forceinline__ bool gfv_arrive_last_writethrough(int* counter) {
  __shared__ int s_last;
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the partial has left this CU before the counter says so
    s_last = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
  }
  __syncthreads();
  return s_last != 0;
}

// No data (no hand-off in Guideline 16's sense): relaxed, no fence - the last arriver needs nothing the others WROTE,
// only that every thread of every workgroup is past its READS of the words it is about to overwrite (the barrier before the add).
//   after: true on thread 0 of the last workgroup only; it may overwrite those words, and may read no other workgroup's stores.
static __device__ __forceinline__ bool gfv_arrive_last_nodata(int* counter) {
  __syncthreads();
  if (threadIdx.x != 0) return false;
  return __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
}

// The last arriver's fold of K sums per chunk (partial [n_chunks, K]): lane l takes chunks c0 + l, c0 + l + 64, ... < c1 in
// ascending order into s[K].  The caller folds the 64 lanes (gfv_wave_sum, or Anderson's tree in LDS).  LD: the doubles of a
// chunk's row where it holds more than the K sums (the flow integrals' two maxima behind their ten sums).
template <int K, int LD = K>
static __device__ __forceinline__ void gfv_fold_chunks(const double* partial, int c0, int c1, int lane, double (&s)[K]) {
  static_assert(LD >= K, "a row holds its K sums");
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.0;
  for (int q = c0 + lane; q < c1; q += 64) {
    const double* p = partial + (size_t)LD * q;
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += gfv_ld_agent(p + k);
  }
}

// Row i of a rollout / sweep step.  live: x_backup[i, 0:3] = uvp_node[i] (the write-back of the predicted field), with
// d2 += || uvp_new - uvp_prev ||^2 and n2 += || uvp_new ||^2 of the row; frozen (a sweep slot that is done): x_backup is left
// alone.  Either way x[i] = x_backup[i] (the un-normalised state the next input preparation reads).  Returns the row's first
// four columns as they are now.
static __device__ __forceinline__ float4 gfv_advance_row(const float* uvp_node, float* x_backup, float* x, int i, bool live,
                                                         double& d2, double& n2) {
  float4* xb = reinterpret_cast<float4*>(x_backup + (size_t)i * 12);
  float4* xo = reinterpret_cast<float4*>(x + (size_t)i * 12);
  float4 r0 = xb[0];
  const float4 r1 = xb[1], r2 = xb[2];
  if (live) {
    const float* u = uvp_node + (size_t)i * 3;
    const float u0 = u[0], u1 = u[1], u2 = u[2];
    const float e0 = u0 - r0.x, e1 = u1 - r0.y, e2 = u2 - r0.z;
    d2 += ((double)e0 * (double)e0 + (double)e1 * (double)e1) + (double)e2 * (double)e2;
    n2 += ((double)u0 * (double)u0 + (double)u1 * (double)u1) + (double)u2 * (double)u2;
    r0.x = u0; r0.y = u1; r0.z = u2;
    xb[0] = r0;
  }
  xo[0] = r0; xo[1] = r1; xo[2] = r2;
  return r0;
}
