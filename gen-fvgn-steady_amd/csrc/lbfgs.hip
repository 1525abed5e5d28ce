// L-BFGS on flat fp32 vectors (gfv/optim.py LBFGS; the reference's solve_with_grad_GPU_LBFGS.py:67-202 through
// torch.optim.LBFGS): the search direction in FOUR launches whatever the history size m is, and no host synchronisation while
// it is computed.
//
// Form: the "vector-free" two-loop recursion.  With the basis B = {s_0..s_m, y_0..y_m, g} (ring slots of m + 1 pairs: m stored
// ones and the candidate, so that a REJECTED candidate costs the oldest pair nothing) and the matrix M = B B^T of their dot
// products (double, kept on the device, three rows renewed per iteration), torch's recursion
//     q = -g;  for i = k-1..0: al_i = ro_i (s_i . q), q -= al_i y_i;  r = H q;  for i = 0..k-1: be_i = ro_i (y_i . r), r += (al_i - be_i) s_i
// runs on the COEFFICIENTS of q and r over B, every dot product a row of M times the coefficient vector; the direction is then
// one pass d = -sum_j delta_j b_j.  Same gamma = ys / y.y, same skip rule (ys > 1e-10) as torch/optim/lbfgs.py.
//   gfv_lbfgs_pair      y_c = g - g_prev, s_c = t d into the free ring slot c = (head + count) % (m + 1);  g_prev = g
//   gfv_lbfgs_multidot  s_c, y_c, g against every live row: per-workgroup partials over a 4096-column tile (double)
//   gfv_lbfgs_coef      ONE workgroup: folds the partials in a fixed order into M, accepts or rejects the candidate (head and
//                       count live on the device), runs the recursion in double, writes delta, g.d and the result block
//   gfv_lbfgs_combine   d = -sum_j delta_j b_j, the per-element sum in double rounded once;  max|d|
//   gfv_lbfgs_dot       masked copy of a gradient + its dot with d, max|.|, ||.||_1 (a line-search trial point): the workgroup
//                       that arrives last (an integer arrival counter, left at zero: csrc/gfv_reduce.h, all-fence form) folds
//   gfv_lbfgs_axpy      p = x0 + t d on the non-padding elements
//
// INVARIANT - padding is not data.  The flat layout starts every tensor on a 16-byte boundary (gfv.engine.GradStore) and the
// padding slots of a flat gradient hold whatever a workspace held (include/gfv.h, the weight-gradient launches).  A dot
// product would see them, so the gradient enters this file only through gfv_lbfgs_dot's masked copy (padding forced to zero,
// by selection: a NaN there is not multiplied away); every vector derived from it here (s, y, d, g_prev) is therefore zero in
// padding, and gfv_lbfgs_axpy does not write the parameters' padding.
//
// Determinism: every sum has a fixed order (lane-sequential, xor butterfly, waves in order, workgroups in ascending order);
// max|d| is an integer atomicMax on the bits of non-negative floats.  No floating-point atomics, no grid barrier, no spin wait.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_reduce.h"

namespace {

constexpr int LB_MAX_SLOTS = 129;                 // history_size <= 128, + the candidate
constexpr int LB_MAX_R = 2 * LB_MAX_SLOTS + 1;    // rows of the basis
constexpr int LB_THREADS = 256;
constexpr int LB_Q = 4;                           // float4 per thread and row: a tile is 4096 columns
constexpr int LB_TILE4 = LB_THREADS * LB_Q;
constexpr int LB_COEF_THREADS = 1024;
constexpr int LB_PARTS = 4;

__device__ __forceinline__ double lb_dot4(const float4 a, const float4 b, double acc) {
  acc += (double)a.x * (double)b.x;
  acc += (double)a.y * (double)b.y;
  acc += (double)a.z * (double)b.z;
  acc += (double)a.w * (double)b.w;
  return acc;
}
// the ring as the device holds it (clamped: a damaged state block must not become an address)
__device__ __forceinline__ void lb_ring(const int* state, int m1, int& head, int& count) {
  head = min(max(state[0], 0), m1 - 1);
  count = min(max(state[1], 0), m1 - 1);
}
// row r of the basis (s slots 0..m1-1, y slots m1..2 m1-1, g = 2 m1) is one of the k oldest-first slots from head, or g
__device__ __forceinline__ bool lb_live(int r, int m1, int head, int k) {
  if (r == 2 * m1) return true;
  int j = (r < m1 ? r : r - m1) - head;
  if (j < 0) j += m1;
  return j < k;
}

__global__ __launch_bounds__(LB_THREADS) void lbfgs_pair_kernel(float4* S, float4* Y, int m1, long n4, const int* state,
                                                                const float4* g, float4* g_prev, const float4* d, float t,
                                                                int first) {
  const long i = (long)blockIdx.x * LB_THREADS + threadIdx.x;
  if (i >= n4) return;
  const float4 gv = g[i];
  if (!first) {
    int head, count;
    lb_ring(state, m1, head, count);
    const long c = (head + count) % m1;
    const float4 gp = g_prev[i], dv = d[i];
    Y[c * n4 + i] = make_float4(gv.x - gp.x, gv.y - gp.y, gv.z - gp.z, gv.w - gp.w);
    S[c * n4 + i] = make_float4(t * dv.x, t * dv.y, t * dv.z, t * dv.w);
  }
  g_prev[i] = gv;
}

// mode: 0 = an iteration with a candidate pair, 1 = the first iteration (no pair: only g . g), 2 = rebuilding M after a
// checkpoint was loaded (a candidate that coef accepts unconditionally; g is not looked at by the caller)
__global__ __launch_bounds__(LB_THREADS) void lbfgs_multidot_kernel(const float4* S, const float4* Y, int m1, long n4,
                                                                    const int* state, const float4* g, double* partial, int mode) {
  __shared__ double s_acc[LB_MAX_R][4][3];
  __shared__ double s_l1[4];
  __shared__ float s_mx[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int head, count;
  lb_ring(state, m1, head, count);
  const bool cand = mode != 1;
  const int k = count + (cand ? 1 : 0);
  const int c = (head + count) % m1;
  const int R = 2 * m1 + 1;
  // (out-of-range columns load the last one and are zeroed as VALUES: a select between addresses would put the zero in scratch)
  auto lb_keep = [](float4 v, bool keep) {
    return make_float4(keep ? v.x : 0.f, keep ? v.y : 0.f, keep ? v.z : 0.f, keep ? v.w : 0.f);
  };
  const long col0 = (long)blockIdx.x * LB_TILE4 + tid;   // the thread's columns: col0 + q * LB_THREADS
  float4 rs[LB_Q], ry[LB_Q], rg[LB_Q];
#pragma unroll
  for (int q = 0; q < LB_Q; ++q) {
    const bool in = col0 + q * LB_THREADS < n4;
    const long col = in ? col0 + q * LB_THREADS : n4 - 1;
    rg[q] = lb_keep(g[col], in);
    rs[q] = lb_keep(S[(long)c * n4 + col], in && cand);
    ry[q] = lb_keep(Y[(long)c * n4 + col], in && cand);
  }
  const int rows = 2 * k;
  for (int j0 = 0; j0 < rows; j0 += 4) {
    float4 v[4][LB_Q];
    int phys[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = min(j0 + u, rows - 1);
      const bool is_s = j < k;
      const int slot = (head + (is_s ? j : j - k)) % m1;
      phys[u] = is_s ? slot : m1 + slot;
      const float4* row = (is_s ? S : Y) + (long)slot * n4;
#pragma unroll
      for (int q = 0; q < LB_Q; ++q) {
        const bool in = col0 + q * LB_THREADS < n4;
        v[u][q] = lb_keep(row[in ? col0 + q * LB_THREADS : n4 - 1], in);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
      for (int q = 0; q < LB_Q; ++q) {
        a0 = lb_dot4(v[u][q], rs[q], a0);
        a1 = lb_dot4(v[u][q], ry[q], a1);
        a2 = lb_dot4(v[u][q], rg[q], a2);
      }
      a0 = gfv_wave_sum(a0);
      a1 = gfv_wave_sum(a1);
      a2 = gfv_wave_sum(a2);
      if (lane == 0 && j0 + u < rows) {   // (past the end: the last row again, not stored)
        s_acc[phys[u]][wave][0] = a0;
        s_acc[phys[u]][wave][1] = a1;
        s_acc[phys[u]][wave][2] = a2;
      }
    }
  }
  {   // the row g, and its maximum and 1-norm
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, l1 = 0.0;
    float mx = 0.f;
#pragma unroll
    for (int q = 0; q < LB_Q; ++q) {
      a0 = lb_dot4(rg[q], rs[q], a0);
      a1 = lb_dot4(rg[q], ry[q], a1);
      a2 = lb_dot4(rg[q], rg[q], a2);
      l1 += ((double)fabsf(rg[q].x) + (double)fabsf(rg[q].y)) + ((double)fabsf(rg[q].z) + (double)fabsf(rg[q].w));
      mx = fmaxf(fmaxf(mx, fmaxf(fabsf(rg[q].x), fabsf(rg[q].y))), fmaxf(fabsf(rg[q].z), fabsf(rg[q].w)));
    }
    a0 = gfv_wave_sum(a0);
    a1 = gfv_wave_sum(a1);
    a2 = gfv_wave_sum(a2);
    l1 = gfv_wave_sum(l1);
    mx = gfv_wave_max_shfl(mx);
    if (lane == 0) {
      s_acc[2 * m1][wave][0] = a0;
      s_acc[2 * m1][wave][1] = a1;
      s_acc[2 * m1][wave][2] = a2;
      s_l1[wave] = l1;
      s_mx[wave] = mx;
    }
  }
  __syncthreads();
  double* out = partial + (size_t)blockIdx.x * (3 * R + 2);
  for (int o = tid; o < 3 * R; o += LB_THREADS) {
    const int r = o / 3, a = o - 3 * r;
    if (lb_live(r, m1, head, k)) out[o] = ((s_acc[r][0][a] + s_acc[r][1][a]) + s_acc[r][2][a]) + s_acc[r][3][a];
  }
  if (tid == 0) {
    out[3 * R] = (double)fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    out[3 * R + 1] = ((s_l1[0] + s_l1[1]) + s_l1[2]) + s_l1[3];
  }
}

struct CoefArgs {
  int* state;              // [8]: head, count
  double* M;               // [R, R]
  const double* partial;   // [nwg, 3 R + 2]
  double* delta;           // [R]
  double* res;             // [16]: g.d, max|g|, ||g||_1, accepted, H_diag, count, -, -, (bits of max|d|), ...
  int m1, nwg, mode;
};

__global__ __launch_bounds__(LB_COEF_THREADS) void lbfgs_coef_kernel(const CoefArgs A) {
  __shared__ double s_part[LB_PARTS][3 * LB_MAX_R + 2];
  __shared__ double s_al[LB_MAX_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int m1 = A.m1, R = 2 * m1 + 1, nout = 3 * R + 2;
  int head, count;
  lb_ring(A.state, m1, head, count);
  const bool cand = A.mode != 1;
  const int k = count + (cand ? 1 : 0);
  const int c = (head + count) % m1;
  // fold the workgroups' partials: four ascending quarters per output, then the quarters in order
  const int per = (A.nwg + LB_PARTS - 1) / LB_PARTS;
  for (int id = tid; id < LB_PARTS * nout; id += LB_COEF_THREADS) {
    const int part = id / nout, o = id - part * nout;
    const bool is_max = o == 3 * R;
    double acc = 0.0;
    if (o >= 3 * R || lb_live(o / 3, m1, head, k)) {
      const int w1 = min(A.nwg, (part + 1) * per);
      for (int w = part * per; w < w1; ++w) {
        const double v = A.partial[(size_t)w * nout + o];
        acc = is_max ? fmax(acc, v) : acc + v;
      }
    }
    s_part[part][o] = acc;
  }
  __syncthreads();
  for (int o = tid; o < nout; o += LB_COEF_THREADS) {
    const double p0 = s_part[0][o], p1 = s_part[1][o], p2 = s_part[2][o], p3 = s_part[3][o];
    if (o >= 3 * R) {
      A.res[o == 3 * R ? 1 : 2] = o == 3 * R ? fmax(fmax(p0, p1), fmax(p2, p3)) : ((p0 + p1) + p2) + p3;
      continue;
    }
    const int r = o / 3, a = o - 3 * r;
    if (!lb_live(r, m1, head, k) || (!cand && a < 2)) continue;
    if (A.mode == 2 && (a == 2 || r == 2 * m1)) continue;   // (a rebuild does not look at g)
    const int arow = a == 0 ? c : a == 1 ? m1 + c : 2 * m1;
    const double v = ((p0 + p1) + p2) + p3;
    A.M[(size_t)arow * R + r] = v;
    A.M[(size_t)r * R + arow] = v;
  }
  __threadfence();
  __syncthreads();
  if (tid >= 64) return;
  // ---- one wave from here on -------------------------------------------------------------------------------------
  const double* M = A.M;
  auto ldM = [&](int row, int r) { return gfv_ld_agent(M + (size_t)row * R + r); };
  double H = A.res[4];
  int accepted = 0;
  if (A.mode == 1) {
    head = 0; count = 0; H = 1.0;
  } else {
    const double ys = ldM(c, m1 + c), yy = ldM(m1 + c, m1 + c);
    accepted = A.mode == 2 || ys > 1e-10;
    if (accepted) {
      if (count == m1 - 1) head = (head + 1) % m1; else count += 1;
      if (A.mode == 0) H = ys / yy;
    }
  }
  if (lane == 0) {
    A.state[0] = head; A.state[1] = count;
    A.res[3] = (double)accepted; A.res[4] = H; A.res[5] = (double)count;
    reinterpret_cast<unsigned int*>(A.res + 8)[0] = 0u;   // max|d|: gfv_lbfgs_combine raises it
  }
  if (A.mode == 2) return;
  constexpr int E = (LB_MAX_R + 63) / 64;
  // The coefficients sit in LOGICAL order - position i < m1 is s of the i-th oldest pair, m1 + i its y, 2 m1 is g - so that the
  // order of every sum, and with it every bit of the direction, does not depend on where the ring's head happens to be (a
  // history loaded from a checkpoint starts at slot 0, the run that wrote it had turned).
  double cf[E];
  int phys[E];   // the row of M / the basis behind each of the lane's positions
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int l = lane + 64 * e;
    cf[e] = l == 2 * m1 ? -1.0 : 0.0;
    phys[e] = l < m1 ? (head + l) % m1 : l < 2 * m1 ? m1 + (head + l - m1) % m1 : 2 * m1;
  }
  auto row_dot = [&](int row) {
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (lane + 64 * e < R && cf[e] != 0.0) acc += cf[e] * ldM(row, phys[e]);
    }
    return gfv_wave_sum(acc);
  };
  auto add_at = [&](int r, double v) {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (lane + 64 * e == r) cf[e] += v;
  };
  volatile double* al = s_al;
  for (int i = count - 1; i >= 0; --i) {
    const int slot = (head + i) % m1;
    const double ro = 1.0 / ldM(slot, m1 + slot);
    const double a = row_dot(slot) * ro;
    al[i] = a;
    add_at(m1 + i, -a);
  }
#pragma unroll
  for (int e = 0; e < E; ++e) cf[e] *= H;
  for (int i = 0; i < count; ++i) {
    const int slot = (head + i) % m1;
    const double ro = 1.0 / ldM(slot, m1 + slot);
    const double be = row_dot(m1 + slot) * ro;
    add_at(i, al[i] - be);
  }
  const double gtd = row_dot(2 * m1);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if (lane + 64 * e < R) A.delta[phys[e]] = -cf[e];
  }
  if (lane == 0) A.res[0] = gtd;
}

__global__ __launch_bounds__(LB_THREADS) void lbfgs_combine_kernel(const float4* S, const float4* Y, int m1, long n4, const int* state,
                                                                   const float4* g, const double* delta, float4* d, double* res) {
  const long i = (long)blockIdx.x * LB_THREADS + threadIdx.x;
  const bool in = i < n4;
  const long ii = in ? i : n4 - 1;
  int head, count;
  lb_ring(state, m1, head, count);
  const int rows = 2 * count;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int j0 = 0; j0 < rows; j0 += 8) {
    float4 v[8];
    double cf[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = min(j0 + u, rows - 1);
      const bool is_s = j < count;
      const int slot = (head + (is_s ? j : j - count)) % m1;
      cf[u] = j0 + u < rows ? delta[is_s ? slot : m1 + slot] : 0.0;
      v[u] = ((is_s ? S : Y) + (long)slot * n4)[ii];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {   // (past the end: coefficient +0.0 on the last row again - the sums keep their bits)
      a0 += cf[u] * (double)v[u].x;
      a1 += cf[u] * (double)v[u].y;
      a2 += cf[u] * (double)v[u].z;
      a3 += cf[u] * (double)v[u].w;
    }
  }
  const float4 gv = g[ii];
  const double cg = delta[2 * m1];
  a0 += cg * (double)gv.x;
  a1 += cg * (double)gv.y;
  a2 += cg * (double)gv.z;
  a3 += cg * (double)gv.w;
  const float4 o = make_float4((float)-a0, (float)-a1, (float)-a2, (float)-a3);
  float mx = 0.f;
  if (in) {
    d[i] = o;
    mx = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w)));
  }
  mx = gfv_wave_max_shfl(mx);
  // non-negative floats order as their bits: an integer maximum, exact and independent of the order of arrival
  if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(reinterpret_cast<unsigned int*>(res + 8), __float_as_uint(mx));
}

__global__ __launch_bounds__(LB_THREADS) void lbfgs_dot_kernel(const float4* a, const unsigned int* mask, float4* copy_out,
                                                               const float4* b, long n4, double* partial, int* counter, double* out) {
  __shared__ double s_red[4][3];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double dot = 0.0, l1 = 0.0;
  float mx = 0.f;
#pragma unroll
  for (int q = 0; q < LB_Q; ++q) {
    const long i = (long)blockIdx.x * LB_TILE4 + q * LB_THREADS + tid;
    if (i < n4) {
      float4 v = a[i];
      {
        const unsigned int mk = mask[i];
        v.x = (mk & 0x000000ffu) ? v.x : 0.f;
        v.y = (mk & 0x0000ff00u) ? v.y : 0.f;
        v.z = (mk & 0x00ff0000u) ? v.z : 0.f;
        v.w = (mk & 0xff000000u) ? v.w : 0.f;
      }
      copy_out[i] = v;
      dot = lb_dot4(v, b[i], dot);
      l1 += ((double)fabsf(v.x) + (double)fabsf(v.y)) + ((double)fabsf(v.z) + (double)fabsf(v.w));
      mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
  }
  dot = gfv_wave_sum(dot);
  l1 = gfv_wave_sum(l1);
  mx = gfv_wave_max_shfl(mx);
  if (lane == 0) { s_red[wave][0] = dot; s_red[wave][1] = (double)mx; s_red[wave][2] = l1; }
  __syncthreads();
  if (tid == 0) {
    double* p = partial + 3 * (size_t)blockIdx.x;
    p[0] = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
    p[1] = fmax(fmax(s_red[0][1], s_red[1][1]), fmax(s_red[2][1], s_red[3][1]));
    p[2] = ((s_red[0][2] + s_red[1][2]) + s_red[2][2]) + s_red[3][2];
  }
  if (!gfv_arrive_last_all_fence(counter)) return;
  dot = 0.0; l1 = 0.0;
  double dmx = 0.0;
  for (int w = tid; w < (int)gridDim.x; w += LB_THREADS) {
    dot += gfv_ld_agent(partial + 3 * (size_t)w);
    dmx = fmax(dmx, gfv_ld_agent(partial + 3 * (size_t)w + 1));
    l1 += gfv_ld_agent(partial + 3 * (size_t)w + 2);
  }
  dot = gfv_wave_sum(dot);
  l1 = gfv_wave_sum(l1);
  mx = gfv_wave_max_shfl((float)dmx);
  __syncthreads();
  if (lane == 0) { s_red[wave][0] = dot; s_red[wave][1] = (double)mx; s_red[wave][2] = l1; }
  __syncthreads();
  if (tid == 0) {
    out[0] = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
    out[1] = fmax(fmax(s_red[0][1], s_red[1][1]), fmax(s_red[2][1], s_red[3][1]));
    out[2] = ((s_red[0][2] + s_red[1][2]) + s_red[2][2]) + s_red[3][2];
    *counter = 0;
  }
}

__global__ __launch_bounds__(LB_THREADS) void lbfgs_axpy_kernel(float4* p, const float4* x0, const float4* d, float t,
                                                                const unsigned int* mask, long n4) {
  const long i = (long)blockIdx.x * LB_THREADS + threadIdx.x;
  if (i >= n4) return;
  const unsigned int mk = mask[i];
  const float4 x = x0[i], dv = d[i];
  float4 o = p[i];
  if (mk & 0x000000ffu) o.x = fmaf(t, dv.x, x.x);
  if (mk & 0x0000ff00u) o.y = fmaf(t, dv.y, x.y);
  if (mk & 0x00ff0000u) o.z = fmaf(t, dv.z, x.z);
  if (mk & 0xff000000u) o.w = fmaf(t, dv.w, x.w);
  p[i] = o;
}

inline bool lb_bad(const void* p) { return !p || (reinterpret_cast<size_t>(p) & 15); }
inline bool lb_bad_dims(int32_t m1, int64_t n) { return m1 < 2 || m1 > LB_MAX_SLOTS || n <= 0 || (n & 3) || n > ((int64_t)1 << 40); }
inline int lb_tiles(int64_t n) { return (int)((n / 4 + LB_TILE4 - 1) / LB_TILE4); }

}  // namespace

extern "C" size_t gfv_lbfgs_workspace_doubles(int32_t slots, int64_t n) {
  if (lb_bad_dims(slots, n)) return 0;
  return (size_t)lb_tiles(n) * (3 * (2 * slots + 1) + 2);
}

extern "C" int gfv_lbfgs_pair(float* S, float* Y, int32_t slots, int64_t n, const int32_t* state, const float* g, float* g_prev,
                              const float* d, double t, int32_t first, void* stream) {
  if (lb_bad(S) || lb_bad(Y) || lb_bad(g) || lb_bad(g_prev) || lb_bad(d) || lb_bad(state) || lb_bad_dims(slots, n)) return GFV_ERR_ARG;
  const long n4 = n / 4;
  GFV_LAUNCH(lbfgs_pair_kernel, dim3((n4 + LB_THREADS - 1) / LB_THREADS), dim3(LB_THREADS), 0, (hipStream_t)stream,
             reinterpret_cast<float4*>(S), reinterpret_cast<float4*>(Y), (int)slots, n4, (const int*)state,
             reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(g_prev), reinterpret_cast<const float4*>(d), (float)t,
             (int)first);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_lbfgs_multidot(const float* S, const float* Y, int32_t slots, int64_t n, const int32_t* state, const float* g,
                                  double* partial_ws, int32_t mode, void* stream) {
  if (lb_bad(S) || lb_bad(Y) || lb_bad(g) || lb_bad(partial_ws) || lb_bad(state) || lb_bad_dims(slots, n) || mode < 0 || mode > 2)
    return GFV_ERR_ARG;
  GFV_LAUNCH(lbfgs_multidot_kernel, dim3(lb_tiles(n)), dim3(LB_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(S),
             reinterpret_cast<const float4*>(Y), (int)slots, (long)(n / 4), (const int*)state, reinterpret_cast<const float4*>(g),
             partial_ws, (int)mode);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_lbfgs_coef(int32_t* state, double* M, const double* partial_ws, double* delta, double* res, int32_t slots,
                              int64_t n, int32_t mode, void* stream) {
  if (lb_bad(state) || lb_bad(M) || lb_bad(partial_ws) || lb_bad(delta) || lb_bad(res) || lb_bad_dims(slots, n) || mode < 0 || mode > 2)
    return GFV_ERR_ARG;
  const CoefArgs a{state, M, partial_ws, delta, res, (int)slots, lb_tiles(n), (int)mode};
  GFV_LAUNCH(lbfgs_coef_kernel, dim3(1), dim3(LB_COEF_THREADS), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_lbfgs_combine(const float* S, const float* Y, int32_t slots, int64_t n, const int32_t* state, const float* g,
                                 const double* delta, float* d, double* res, void* stream) {
  if (lb_bad(S) || lb_bad(Y) || lb_bad(g) || lb_bad(delta) || lb_bad(d) || lb_bad(res) || lb_bad(state) || lb_bad_dims(slots, n))
    return GFV_ERR_ARG;
  const long n4 = n / 4;
  GFV_LAUNCH(lbfgs_combine_kernel, dim3((n4 + LB_THREADS - 1) / LB_THREADS), dim3(LB_THREADS), 0, (hipStream_t)stream,
             reinterpret_cast<const float4*>(S), reinterpret_cast<const float4*>(Y), (int)slots, n4, (const int*)state,
             reinterpret_cast<const float4*>(g), delta, reinterpret_cast<float4*>(d), res);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_lbfgs_dot(const float* a, const uint8_t* mask, float* copy_out, const float* b, int64_t n, double* partial_ws,
                             int32_t* counter, double* out, void* stream) {
  if (lb_bad(a) || lb_bad(mask) || lb_bad(copy_out) || lb_bad(b) || lb_bad(partial_ws) || lb_bad(counter) || lb_bad(out) || n <= 0 ||
      (n & 3))
    return GFV_ERR_ARG;
  GFV_LAUNCH(lbfgs_dot_kernel, dim3(lb_tiles(n)), dim3(LB_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(a),
             reinterpret_cast<const unsigned int*>(mask), reinterpret_cast<float4*>(copy_out), reinterpret_cast<const float4*>(b),
             (long)(n / 4), partial_ws, (int*)counter, out);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_lbfgs_axpy(float* p, const float* x0, const float* d, double t, const uint8_t* mask, int64_t n, void* stream) {
  if (lb_bad(p) || lb_bad(x0) || lb_bad(d) || lb_bad(mask) || n <= 0 || (n & 3)) return GFV_ERR_ARG;
  const long n4 = n / 4;
  GFV_LAUNCH(lbfgs_axpy_kernel, dim3((n4 + LB_THREADS - 1) / LB_THREADS), dim3(LB_THREADS), 0, (hipStream_t)stream,
             reinterpret_cast<float4*>(p), reinterpret_cast<const float4*>(x0), reinterpret_cast<const float4*>(d), (float)t,
             reinterpret_cast<const unsigned int*>(mask), n4);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
