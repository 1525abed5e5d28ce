// Observation term of the training objective (gfv/observe.py; semantics in include/gfv.h): a weighted squared
// misfit between the network's own nodal prediction - phi[:, 0:3] = BC(10 tanh(dec / 10)), re-dimensionalised as the returned
// field is - and measured values, added per graph inside the logarithm of the training loss.  Three launches:
//   gfv_obs_fwd     behind the forward: S_b = sum w e^2 and W_b = sum w per graph in double, in the fixed order of
//                   csrc/gfv_reduce.h (two sums per chunk); the workgroup that arrives last folds them, writes the record
//                   rec[b] = (obs_b, W_b, gobs_b, tot_b) and OVERWRITES loss and gloss with the tail launch's own arithmetic
//   gfv_obs_bwd     between the finite-volume adjoint and the decoder's backward: one thread per node adds into g_dec
//   gfv_obs_gather  pool path: fills the batch-sized value / weight buffers from per-entry tensors whose addresses travel by
//                   value in the argument block (never part of a recorded list)
// Arrival of gfv_obs_fwd: the write-through form (gfv_arrive_last_writethrough).  The launch runs behind a forward that has
// just written every activation, where an agent-scope release fence per workgroup would pay for the L2's write-back (DESIGN.md
// 5m); a workgroup hands over eight doubles at most, gathered in LDS and stored by thread 0 with agent-scope stores, and the last
// arriver reads them with gfv_ld_agent only (gfv_fold_chunks).  The counter is left at zero.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"

namespace {

enum { NT_NORMAL = 0, NT_INFLOW = 1, NT_OUTFLOW = 2, NT_WALL = 3, NT_PRESS = 4, NT_INWALL = 5 };   // (csrc/fvm.hip)

constexpr int OB_WAVES = 4;
constexpr int MAXB = GFV_POOL_MAX_GRAPHS;
static_assert(MAXB <= 64, "the loss tail gives every graph a lane of one wave");
static_assert(GFV_OBS_RECORD == 4, "a record is one float4");

// e = pred - t of one element, fp32: pred = (phi * uvp_dim) * sigma, the order of cell_to_node_kernel (csrc/fvm.hip)
static __device__ __forceinline__ float obs_misfit(float phi, float dim, float sig, float t) { return (phi * dim) * sig - t; }

struct ObsFwdArgs {
  const float* phi;          // [N,8], channels 0..2 = uvp_new
  const float* target;       // [N,3]
  const float* weight;       // [N,3]
  const int* chunk_beg;      // [n_chunks]
  const int* chunk_end;
  const int* gchunk_ptr;     // [B+1]
  const float* uvp_dim;      // [B,3]
  const float* sigma;        // [B,3]
  const float* losses;       // [B,4]
  const float* hyper;        // [8]
  const float* w_obs;        // [1]
  double* partial;           // [n_chunks,2]
  int* counter;
  float* rec;                // [B,4]
  float* loss;               // [1]
  float* gloss;              // [B,4]
  int N, n_chunks, B;
};

__global__ __launch_bounds__(64 * OB_WAVES) void obs_fwd_kernel(const ObsFwdArgs A) {
  __shared__ double s_part[OB_WAVES][2];
  __shared__ float s_obs[MAXB], s_w[MAXB], s_red[64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.x * OB_WAVES + wave;
  if (c < A.n_chunks) {
    const int b = gfv_chunk_graph(A.gchunk_ptr, A.B, c);
    const float d0 = A.uvp_dim[3 * b], d1 = A.uvp_dim[3 * b + 1], d2 = A.uvp_dim[3 * b + 2];
    const float g0 = A.sigma[3 * b], g1 = A.sigma[3 * b + 1], g2 = A.sigma[3 * b + 2];
    const int beg = A.chunk_beg[c], end = min(A.chunk_end[c], A.N);
    double S = 0.0, W = 0.0;
    for (int i = beg + lane; i < end; i += 64) {
      if (i < 0) continue;
      const float* w = A.weight + (size_t)i * 3;
      const float w0 = w[0], w1 = w[1], w2 = w[2];
      if (w0 == 0.f && w1 == 0.f && w2 == 0.f) continue;       // (adds +0.0 to both sums: the same bits as skipping)
      const float4 p = *reinterpret_cast<const float4*>(A.phi + (size_t)i * 8);
      const float* t = A.target + (size_t)i * 3;
      double q0 = 0.0, q1 = 0.0, q2 = 0.0;
      // an element with weight 0 is skipped before its target enters any arithmetic (it may be NaN)
      if (w0 != 0.f) { const float e = obs_misfit(p.x, d0, g0, t[0]); q0 = (double)w0 * ((double)e * (double)e); }
      if (w1 != 0.f) { const float e = obs_misfit(p.y, d1, g1, t[1]); q1 = (double)w1 * ((double)e * (double)e); }
      if (w2 != 0.f) { const float e = obs_misfit(p.z, d2, g2, t[2]); q2 = (double)w2 * ((double)e * (double)e); }
      S += (q0 + q1) + q2;
      W += ((double)w0 + (double)w1) + (double)w2;
    }
    S = gfv_wave_sum(S);
    W = gfv_wave_sum(W);
    if (lane == 0) { s_part[wave][0] = S; s_part[wave][1] = W; }
  }
  __syncthreads();
  if (tid == 0) {
    // thread 0 stores the workgroup's partials write-through: what gfv_arrive_last_writethrough hands over
    const int c0 = blockIdx.x * OB_WAVES;
    for (int k = 0; k < OB_WAVES && c0 + k < A.n_chunks; ++k) {
      gfv_st_agent(A.partial + 2 * (size_t)(c0 + k), s_part[k][0]);
      gfv_st_agent(A.partial + 2 * (size_t)(c0 + k) + 1, s_part[k][1]);
    }
  }
  if (!gfv_arrive_last_writethrough(A.counter)) return;
  // ---- the last arriver: per-graph folds (agent-scope loads only), then the loss with fvm_tail_kernel's arithmetic ----------------
  for (int b = wave; b < A.B; b += OB_WAVES) {
    const int c0 = A.gchunk_ptr[b], c1 = min(A.gchunk_ptr[b + 1], A.n_chunks);
    double s[2];
    gfv_fold_chunks(A.partial, c0, c1, lane, s);
    const double S = gfv_wave_sum(s[0]), W = gfv_wave_sum(s[1]);
    if (lane == 0) {
      s_obs[b] = W == 0.0 ? 0.f : (float)(S / W);
      s_w[b] = (float)W;
    }
  }
  __syncthreads();
  const int B = A.B;
  if (tid < 64) {
    const float wc = A.hyper[5], wm = A.hyper[6], wp = A.hyper[7], wo = *A.w_obs;
    float s = 0.f;
    for (int g = tid; g < B; g += 64) {
      const float* l = A.losses + 4 * g;
      const float obs = s_obs[g];
      const float tot = gfv_weighted_residual(l[0], l[1], l[2], l[3], wc, wm, wp) + wo * obs;
      s += logf(tot);
      const float inv = 1.0f / (tot * (float)B);
      A.gloss[4 * g] = wc * inv; A.gloss[4 * g + 1] = wm * inv; A.gloss[4 * g + 2] = wm * inv; A.gloss[4 * g + 3] = wp * inv;
      *reinterpret_cast<float4*>(A.rec + 4 * g) = make_float4(obs, s_w[g], wo * inv, tot);
    }
    s_red[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    float a = 0.f;
    for (int i = 0; i < 64; ++i) a += s_red[i];
    *A.loss = a / (float)B;
    *A.counter = 0;
  }
}

__global__ __launch_bounds__(256) void obs_bwd_kernel(const float* __restrict__ rec, const float* __restrict__ dec,
                                                      const float* __restrict__ phi, const float* __restrict__ target,
                                                      const float* __restrict__ weight, const int* __restrict__ batch,
                                                      const int* __restrict__ node_type, const float* __restrict__ uvp_dim,
                                                      const float* __restrict__ sigma, float* __restrict__ gdec, int N, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float w0 = weight[3 * (size_t)i], w1 = weight[3 * (size_t)i + 1], w2 = weight[3 * (size_t)i + 2];
  const int nt = node_type[i];
  // where phi_bwd_kernel (csrc/fvm.hip) lets gradient through
  const bool uv = !(nt == NT_WALL || nt == NT_INFLOW || nt == NT_PRESS || nt == NT_INWALL), pr = nt != NT_PRESS;
  const bool on0 = uv && w0 != 0.f, on1 = uv && w1 != 0.f, on2 = pr && w2 != 0.f;
  if (!(on0 || on1 || on2)) return;                    // (not written at all)
  const int b = batch[i];
  if (b < 0 || b >= B) return;
  const float4 r = *reinterpret_cast<const float4*>(rec + 4 * (size_t)b);     // (obs, W, gobs, tot)
  const float W = r.y, gobs = r.z;
  const float4 p = *reinterpret_cast<const float4*>(phi + (size_t)i * 8);
  const float* t = target + (size_t)i * 3;
  const float* d = dec + (size_t)i * 3;
  float* g = gdec + (size_t)i * 3;
  if (on0) {
    const float dim = uvp_dim[3 * b], sig = sigma[3 * b], e = obs_misfit(p.x, dim, sig, t[0]), th = tanhf(d[0] / 10.f);
    g[0] += gobs * (2.f * w0 * e * (dim * sig) / W) * (1.f - th * th);
  }
  if (on1) {
    const float dim = uvp_dim[3 * b + 1], sig = sigma[3 * b + 1], e = obs_misfit(p.y, dim, sig, t[1]), th = tanhf(d[1] / 10.f);
    g[1] += gobs * (2.f * w1 * e * (dim * sig) / W) * (1.f - th * th);
  }
  if (on2) {
    const float dim = uvp_dim[3 * b + 2], sig = sigma[3 * b + 2], e = obs_misfit(p.z, dim, sig, t[2]), th = tanhf(d[2] / 10.f);
    g[2] += gobs * (2.f * w2 * e * (dim * sig) / W) * (1.f - th * th);
  }
}

struct ObsGatherArgs {
  float* dst_values;                // [>= sum rows, 3]
  float* dst_weights;
  int B;
  int off[MAXB + 1];                // first row of graph b in the batch
  const float* values[MAXB];        // [rows_b, 3] or NULL: no observations, zero weights
  const float* weights[MAXB];
};

// grid (blocks over the 3 * rows words of the largest graph, B)
__global__ __launch_bounds__(256) void obs_gather_kernel(const ObsGatherArgs A) {
  const int b = blockIdx.y;
  const long n = 3L * (A.off[b + 1] - A.off[b]);
  const float* v = A.values[b];
  const float* w = A.weights[b];
  const size_t base = 3 * (size_t)A.off[b];
  for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += 256L * gridDim.x) {
    if (v) {
      A.dst_values[base + k] = v[k];
      A.dst_weights[base + k] = w[k];
    } else {
      A.dst_weights[base + k] = 0.f;          // (the values of an unobserved graph are never read)
    }
  }
}

}  // namespace

extern "C" int gfv_obs_fwd(const float* phi, const float* target, const float* weight, int32_t N, const int32_t* chunk_beg,
                           const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, const float* uvp_dim,
                           const float* sigma, const float* losses, const float* hyper, const float* w_obs, double* partial_ws,
                           int32_t* counter, float* rec, float* loss, float* gloss, void* stream) {
  if (!phi || !target || !weight || !chunk_beg || !chunk_end || !gchunk_ptr || !uvp_dim || !sigma || !losses || !hyper || !w_obs ||
      !partial_ws || !counter || !rec || !loss || !gloss)
    return GFV_ERR_ARG;
  if (N <= 0 || n_chunks <= 0 || B <= 0 || B > MAXB) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(phi) & 15) || (reinterpret_cast<size_t>(rec) & 15) || (reinterpret_cast<size_t>(partial_ws) & 7))
    return GFV_ERR_ARG;
  const ObsFwdArgs a{phi, target, weight, chunk_beg, chunk_end, gchunk_ptr, uvp_dim, sigma, losses, hyper, w_obs, partial_ws,
                     counter, rec, loss, gloss, N, n_chunks, B};
  // rows: 16 B of phi [N,8], target and weight [N,3]
  GfvProfScope ps_(GFV_K_MISC, 0, (16.0 + 12.0 + 12.0) * N, stream);
  GFV_LAUNCH(obs_fwd_kernel, dim3((n_chunks + OB_WAVES - 1) / OB_WAVES), dim3(64 * OB_WAVES), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_obs_bwd(const float* rec, const float* dec, const float* phi, const float* target, const float* weight,
                           const int32_t* batch, const int32_t* node_type, const float* uvp_dim, const float* sigma, int32_t N,
                           int32_t B, float* g_dec, void* stream) {
  if (!rec || !dec || !phi || !target || !weight || !batch || !node_type || !uvp_dim || !sigma || !g_dec) return GFV_ERR_ARG;
  if (N < 0 || B <= 0 || B > MAXB) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(phi) & 15) || (reinterpret_cast<size_t>(rec) & 15)) return GFV_ERR_ARG;
  if (N == 0) return GFV_OK;
  // rows: weight, node type, batch always; phi, target, dec and g_dec (read + write) where a channel contributes - an upper bound
  GfvProfScope ps_(GFV_K_MISC, 0, (12.0 + 4.0 + 4.0 + 16.0 + 12.0 + 12.0 + 24.0) * N, stream);
  GFV_LAUNCH(obs_bwd_kernel, dim3(gfv_div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, rec, dec, phi, target, weight, batch,
             node_type, uvp_dim, sigma, g_dec, (int)N, (int)B);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_obs_gather(const float* const* values, const float* const* weights, const int32_t* rows, int32_t B,
                              float* dst_values, float* dst_weights, int64_t dst_rows, void* stream) {
  if (!values || !weights || !rows || !dst_values || !dst_weights) return GFV_ERR_ARG;
  if (B <= 0 || B > MAXB || dst_rows < 0) return GFV_ERR_ARG;
  ObsGatherArgs a{};
  a.dst_values = dst_values;
  a.dst_weights = dst_weights;
  a.B = B;
  long total = 0;
  int most = 0;
  for (int b = 0; b < B; ++b) {
    if (rows[b] < 0) return GFV_ERR_ARG;
    if ((values[b] == nullptr) != (weights[b] == nullptr)) return GFV_ERR_ARG;
    a.off[b] = (int)total;
    a.values[b] = values[b];
    a.weights[b] = weights[b];
    total += rows[b];
    if (total > dst_rows || total > 0x7fffffffL / 3) return GFV_ERR_ARG;
    most = rows[b] > most ? rows[b] : most;
  }
  a.off[B] = (int)total;
  if (most == 0) return GFV_OK;
  int gx = gfv_div_up(3L * most, 256);
  if (gx > 1024) gx = 1024;
  GfvProfScope ps_(GFV_K_MISC, 0, 48.0 * total, stream);
  GFV_LAUNCH(obs_gather_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
