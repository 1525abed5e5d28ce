// Anderson acceleration AA(m) of the steady-state rollout (gfv/rollout.py, gfv/anderson.py): TWO launches between the
// forward-only step and gfv_rollout_advance, decided on the device so that one recorded launch list serves every step.
// Per graph b, over its node rows x 3 channels in fp32:  x = x_backup[:, 0:3],  g = uvp_node (the model's output),  f = g - x.
//   gfv_anderson_gram   per row: f; with a previous pair, ring column dF[head] = f - f_prev, dG[head] = g - g_prev (fp32); then
//                       f_prev = f, g_prev = g.  Over the mk = min(cnt + has_prev, m) valid columns (the new one included), in
//                       double: the upper triangle of dF^T dF, dF^T f, ||f||^2, ||g||^2.  The workgroup that arrives last decides
//                       per graph (restart / plain step / solve), writes gamma[b] in ring-slot order and the row aa[k, b].
//   gfv_anderson_mix    rows of a graph with depth > 0:  uvp_node = g - (1-beta) f - sum_j gamma_j (dG_j - (1-beta) dF_j), j in
//                       ascending ring slot, in double, rounded to fp32 once.  Rows of a graph with depth 0 are not written.
// The difference form keeps a row whose g never changes (a Dirichlet node: dG = 0, f = 0 exactly) bit for bit.
// Summation order: csrc/gfv_reduce.h, with the butterfly's tree formed in LDS (aa_tree_sum); the arrival counter is left at zero
// (all-fence form).  The sums of a graph do not depend on its neighbours in the batch.
// The column loops are unrolled at compile time over GFV_AA_MAX_DEPTH slots with run-time (wave-uniform) masks: every accumulator
// has a constant index and stays in a register.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"

namespace {

constexpr int AA_WAVES = 4;
constexpr int MD = GFV_AA_MAX_DEPTH;
constexpr int AA_TRI = MD * (MD + 1) / 2;     // upper triangle of the Gram matrix, row-major over ring slots i <= j
constexpr int AA_P = GFV_AA_PARTIALS;         // [tri | dF^T f | ||f||^2 | ||g||^2]
static_assert(MD == 8 && AA_P == AA_TRI + MD + 2 && AA_P <= 64, "one lane per partial sum");

__host__ __device__ constexpr int aa_tri(int i, int j) { return i * MD - i * (i - 1) / 2 + (j - i); }   // i <= j

struct GramArgs {
  const float* uvp_node;      // [N,3]  g
  const float* x_backup;      // [N,12] x = columns 0:3
  const int* chunk_beg;       // [n_chunks]
  const int* chunk_end;
  const int* gchunk_ptr;      // [B+1]
  float* f_prev;              // [N,3]
  float* g_prev;              // [N,3]
  float* dF;                  // [m][N,3]
  float* dG;                  // [m][N,3]
  int* aa_state;              // [B,4]: cnt, head, has_prev, restarts
  double* r_prev;             // [B]
  double* gamma;              // [B,8]
  double* partial;            // [n_chunks, AA_P]
  int* counter;               // arrival counter
  float* table;               // [K_max,B,4]
  const int* step;            // the rollout's step counter
  double reg, restart;
  int N, n_chunks, B, K_max, m, start;
};

struct MixArgs {
  float* uvp_node;            // [N,3]
  const float* f_cur;         // [N,3]: f of this step (what the gram launch left in f_prev)
  const int* chunk_beg;
  const int* chunk_end;
  const int* gchunk_ptr;
  const float* dF;
  const float* dG;
  const double* gamma;        // [B,8]
  const float* table;         // [K_max,B,4]
  const int* step;
  double omb;                 // 1 - beta
  int N, n_chunks, B, K_max, m;
};

// the ring slots that hold a valid column: the mk newest, counted back from `newest`
__device__ __forceinline__ int aa_valid_mask(int newest, int mk, int m) {
  int mask = 0;
#pragma unroll
  for (int s = 0; s < MD; ++s) {
    int age = newest - s;
    if (age < 0) age += m;
    if (s < m && age < mk) mask |= 1 << s;
  }
  return mask;
}

// The butterfly of gfv_wave_sum for AA_P sums at once.  Every lane has put its AA_P values into the wave's LDS tile t[q][lane]
// (rows padded to AA_LD); lane q then adds the 64 values of row q in the butterfly's own tree - level o = 32, 16, ... 1:
// v[l] = v[l] + v[l + o] for l < o, which is what lane 0 of the butterfly computes (v[l] + v[l ^ o], addition commutes) - so the
// result has the butterfly's bits, at 64 independent LDS reads per lane instead of 6 dependent exchanges per sum.
constexpr int AA_LD = 65;
__device__ __forceinline__ void aa_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double aa_tree_sum(const double* row) {
  double v[64];
#pragma unroll
  for (int l = 0; l < 64; ++l) v[l] = row[l];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
    for (int l = 0; l < o; ++l) v[l] = v[l] + v[l + o];
  }
  return v[0];
}

__device__ __forceinline__ bool aa_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }   // false for NaN

__global__ __launch_bounds__(64 * AA_WAVES) void anderson_gram_kernel(const GramArgs A) {
  __shared__ double s_tile[AA_WAVES][AA_P][AA_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.x * AA_WAVES + wave;
  const int m = A.m;
  double (*tile)[AA_LD] = s_tile[wave];
  if (c < A.n_chunks) {
    const int b = gfv_chunk_graph(A.gchunk_ptr, A.B, c);
    const int* st = A.aa_state + 4 * b;
    const int cnt = __builtin_amdgcn_readfirstlane(min(max(st[0], 0), m));
    const int head = __builtin_amdgcn_readfirstlane(min(max(st[1], 0), m - 1));
    const int has_prev = __builtin_amdgcn_readfirstlane(st[2] != 0);
    const int mk = min(cnt + has_prev, m);
    const int vmask = __builtin_amdgcn_readfirstlane(has_prev ? aa_valid_mask(head, mk, m) : 0);
    const size_t col = (size_t)A.N * 3;
    const int beg = A.chunk_beg[c], end = min(A.chunk_end[c], A.N);
    double s[AA_P];
#pragma unroll
    for (int q = 0; q < AA_P; ++q) s[q] = 0.0;
    for (int i = beg + lane; i < end; i += 64) {
      if (i < 0) continue;
      const size_t r = (size_t)i * 3;
      const float* u = A.uvp_node + r;
      const float* xb = A.x_backup + (size_t)i * 12;
      const float g0 = u[0], g1 = u[1], g2 = u[2];
      const float f0 = g0 - xb[0], f1 = g1 - xb[1], f2 = g2 - xb[2];
      float n0 = 0.f, n1 = 0.f, n2 = 0.f;       // the new column of dF
      if (has_prev) {
        const float* fp = A.f_prev + r;
        const float* gp = A.g_prev + r;
        n0 = f0 - fp[0]; n1 = f1 - fp[1]; n2 = f2 - fp[2];
        float* df = A.dF + head * col + r;
        float* dg = A.dG + head * col + r;
        df[0] = n0; df[1] = n1; df[2] = n2;
        dg[0] = g0 - gp[0]; dg[1] = g1 - gp[1]; dg[2] = g2 - gp[2];
      }
      A.f_prev[r] = f0; A.f_prev[r + 1] = f1; A.f_prev[r + 2] = f2;
      A.g_prev[r] = g0; A.g_prev[r + 1] = g1; A.g_prev[r + 2] = g2;
      double d[MD][3];
#pragma unroll
      for (int j = 0; j < MD; ++j) {
        d[j][0] = d[j][1] = d[j][2] = 0.0;
        if ((vmask >> j) & 1) {
          if (j == head) {
            d[j][0] = (double)n0; d[j][1] = (double)n1; d[j][2] = (double)n2;
          } else {
            const float* p = A.dF + j * col + r;
            d[j][0] = (double)p[0]; d[j][1] = (double)p[1]; d[j][2] = (double)p[2];
          }
        }
      }
      const double e0 = (double)f0, e1 = (double)f1, e2 = (double)f2;
#pragma unroll
      for (int j = 0; j < MD; ++j) {
        if (!((vmask >> j) & 1)) continue;
#pragma unroll
        for (int l = j; l < MD; ++l) {
          if (!((vmask >> l) & 1)) continue;
          s[aa_tri(j, l)] += (d[j][0] * d[l][0] + d[j][1] * d[l][1]) + d[j][2] * d[l][2];
        }
        s[AA_TRI + j] += (d[j][0] * e0 + d[j][1] * e1) + d[j][2] * e2;
      }
      s[AA_TRI + MD] += (e0 * e0 + e1 * e1) + e2 * e2;
      s[AA_TRI + MD + 1] += ((double)g0 * (double)g0 + (double)g1 * (double)g1) + (double)g2 * (double)g2;
    }
#pragma unroll
    for (int q = 0; q < AA_P; ++q) tile[q][lane] = s[q];
    aa_wave_sync();
    if (lane < AA_P) A.partial[(size_t)AA_P * c + lane] = aa_tree_sum(tile[lane]);      // lane q folds sum q
  }
  if (!gfv_arrive_last_all_fence(A.counter)) return;
  const int k = gfv_ld_agent(A.step);
  const bool room = k >= 0 && k < A.K_max;    // (a full table is not written past and nothing is mixed: the host raises before)
  for (int b = wave; b < A.B; b += AA_WAVES) {
    const int c0 = A.gchunk_ptr[b], c1 = min(A.gchunk_ptr[b + 1], A.n_chunks);
    int* st = A.aa_state + 4 * b;
    const int cnt = __builtin_amdgcn_readfirstlane(min(max(st[0], 0), m));
    const int head = __builtin_amdgcn_readfirstlane(min(max(st[1], 0), m - 1));
    const int has_prev = __builtin_amdgcn_readfirstlane(st[2] != 0);
    int restarts = st[3];
    const int mk = min(cnt + has_prev, m);
    const int vmask = __builtin_amdgcn_readfirstlane(has_prev ? aa_valid_mask(head, mk, m) : 0);
    double s[AA_P];
    gfv_fold_chunks(A.partial, c0, c1, lane, s);
    aa_wave_sync();                      // (the tile's last readers: this wave's own chunk, or the graph before)
#pragma unroll
    for (int t = 0; t < AA_P; ++t) tile[t][lane] = s[t];
    aa_wave_sync();
    if (lane < AA_P) tile[lane][64] = aa_tree_sum(tile[lane]);       // (column 64 is the rows' padding)
    aa_wave_sync();
#pragma unroll
    for (int t = 0; t < AA_P; ++t) s[t] = tile[t][64];
    // ---- the decision: every lane computes the same values, single lanes store them
    const double ff = s[AA_TRI + MD], gg = s[AA_TRI + MD + 1];
    const double rf = sqrt(ff);
    const double rp = A.r_prev[b];
    double gam[MD];
#pragma unroll
    for (int j = 0; j < MD; ++j) gam[j] = 0.0;
    int depth = 0, flags = 0, n_cnt = mk, n_head = head, n_prev = 1;
    if (has_prev && mk > 0) n_head = head + 1 == m ? 0 : head + 1;
    if (!room) {
      n_cnt = cnt; n_head = head; n_prev = has_prev;      // nothing is decided for a step that has no row
    } else if (!aa_finite(ff)) {
      flags = GFV_AA_NONFINITE; n_cnt = 0; n_prev = 0; n_head = head; ++restarts;
    } else if (has_prev && A.restart > 0.0 && rf > A.restart * rp) {
      flags = GFV_AA_GROWTH; n_cnt = 0; n_head = head; ++restarts;
    } else if (mk > 0 && k >= A.start) {
      double tr = 0.0;
#pragma unroll
      for (int j = 0; j < MD; ++j)
        if ((vmask >> j) & 1) tr += s[aa_tri(j, j)];
      const double lam = A.reg * tr / (double)mk;
      // Cholesky of the masked system: an unused slot is a row of the identity with a zero right-hand side (gamma = 0 exactly)
      double Lm[MD][MD], y[MD], inv[MD];
      bool ok = true;
#pragma unroll
      for (int i = 0; i < MD; ++i) {
        const bool vi = (vmask >> i) & 1;
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          const bool vj = (vmask >> j) & 1;
          Lm[i][j] = (vi && vj) ? s[aa_tri(j, i)] + (i == j ? lam : 0.0) : (i == j ? 1.0 : 0.0);
        }
        y[i] = vi ? s[AA_TRI + i] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < MD; ++j) {
        inv[j] = 1.0;
        if (!((vmask >> j) & 1)) continue;          // (an identity row: its column of L is zero below the diagonal)
        double dj = Lm[j][j];
#pragma unroll
        for (int t = 0; t < j; ++t) dj -= Lm[j][t] * Lm[j][t];
        if (!(dj > 0.0)) ok = false;
        inv[j] = 1.0 / sqrt(dj);                    // one division per pivot: the column and both substitutions multiply
#pragma unroll
        for (int i = j + 1; i < MD; ++i) {
          double v = Lm[i][j];
#pragma unroll
          for (int t = 0; t < j; ++t) v -= Lm[i][t] * Lm[j][t];
          Lm[i][j] = v * inv[j];
        }
      }
#pragma unroll
      for (int i = 0; i < MD; ++i) {
        if (!((vmask >> i) & 1)) continue;          // (y = 0)
        double v = y[i];
#pragma unroll
        for (int t = 0; t < i; ++t) v -= Lm[i][t] * y[t];
        y[i] = v * inv[i];
      }
#pragma unroll
      for (int i = MD - 1; i >= 0; --i) {
        if (!((vmask >> i) & 1)) continue;          // (gamma = 0)
        double v = y[i];
#pragma unroll
        for (int t = i + 1; t < MD; ++t) v -= Lm[t][i] * gam[t];
        gam[i] = v * inv[i];
      }
#pragma unroll
      for (int i = 0; i < MD; ++i) ok = ok && aa_finite(gam[i]);
      if (ok) {
        depth = mk;
      } else {
        flags = GFV_AA_SINGULAR; n_cnt = 0; n_head = head; ++restarts;
#pragma unroll
        for (int j = 0; j < MD; ++j) gam[j] = 0.0;
      }
    }
    // (per-lane vector stores: one writer per word)
    double mine = 0.0;
#pragma unroll
    for (int j = 0; j < MD; ++j)
      if (lane == j) mine = gam[j];
    if (lane < MD) A.gamma[(size_t)MD * b + lane] = mine;
    if (lane == 8) st[0] = n_cnt;
    if (lane == 9) st[1] = n_head;
    if (lane == 10) st[2] = n_prev;
    if (lane == 11) st[3] = restarts;
    if (lane == 12 && room) A.r_prev[b] = rf;
    if (room) {
      float* row = A.table + ((size_t)k * A.B + b) * 4;
      if (lane == 16) row[0] = (float)rf;
      if (lane == 17) row[1] = (float)sqrt(gg);
      if (lane == 18) row[2] = (float)depth;
      if (lane == 19) row[3] = (float)flags;
    }
  }
  __syncthreads();
  if (tid == 0) *A.counter = 0;
}

__global__ __launch_bounds__(64 * AA_WAVES) void anderson_mix_kernel(const MixArgs A) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.x * AA_WAVES + wave;
  if (c >= A.n_chunks) return;
  const int k = A.step[0];
  if (k < 0 || k >= A.K_max) return;
  const int b = gfv_chunk_graph(A.gchunk_ptr, A.B, c);
  const int depth = (int)A.table[((size_t)k * A.B + b) * 4 + 2];
  if (depth <= 0) return;
  double gam[MD];
#pragma unroll
  for (int j = 0; j < MD; ++j) gam[j] = A.gamma[(size_t)MD * b + j];
  const int m = A.m;
  const double omb = A.omb;
  const size_t col = (size_t)A.N * 3;
  const int beg = A.chunk_beg[c], end = min(A.chunk_end[c], A.N);
  for (int i = beg + lane; i < end; i += 64) {
    if (i < 0) continue;
    const size_t r = (size_t)i * 3;
    float* u = A.uvp_node + r;
    double v[3] = {(double)u[0], (double)u[1], (double)u[2]};
    if (omb != 0.0) {
      const float* f = A.f_cur + r;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) v[ch] = v[ch] - omb * (double)f[ch];
    }
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < MD; ++j) {
      if (j >= m || gam[j] == 0.0) continue;      // (an unused slot has gamma = 0 exactly and may hold stale values)
      const float* dg = A.dG + j * col + r;
      double t[3] = {(double)dg[0], (double)dg[1], (double)dg[2]};
      if (omb != 0.0) {
        const float* df = A.dF + j * col + r;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) t[ch] = t[ch] - omb * (double)df[ch];
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[ch] += gam[j] * t[ch];
    }
    u[0] = (float)(v[0] - acc[0]);
    u[1] = (float)(v[1] - acc[1]);
    u[2] = (float)(v[2] - acc[2]);
  }
}

bool aa_bad_tables(const void* a, const void* b, const void* c, int32_t N, int32_t n_chunks, int32_t B, int32_t K_max, int32_t m) {
  return !a || !b || !c || N <= 0 || n_chunks <= 0 || B <= 0 || K_max <= 0 || m < 1 || m > MD;
}

}  // namespace

extern "C" int gfv_anderson_gram(const float* uvp_node, const float* x_backup, int32_t N, const int32_t* chunk_beg,
                                 const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, int32_t m,
                                 double reg, double restart, int32_t start, float* f_prev, float* g_prev, float* dF, float* dG,
                                 int32_t* aa_state, double* r_prev, double* gamma, double* partial_ws, int32_t* counter,
                                 float* aa_table, int32_t K_max, const int32_t* step, void* stream) {
  if (!uvp_node || !x_backup || !f_prev || !g_prev || !dF || !dG || !aa_state || !r_prev || !gamma || !partial_ws || !counter ||
      !aa_table || !step)
    return GFV_ERR_ARG;
  if (aa_bad_tables(chunk_beg, chunk_end, gchunk_ptr, N, n_chunks, B, K_max, m)) return GFV_ERR_ARG;
  if (!(reg >= 0.0)) return GFV_ERR_ARG;                                   // negative or NaN
  if (!(restart >= 0.0) || (restart > 0.0 && restart <= 1.0)) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(r_prev) | reinterpret_cast<size_t>(gamma) | reinterpret_cast<size_t>(partial_ws)) & 7)
    return GFV_ERR_ARG;
  // rows: uvp [N,3] and 12 B of x_backup read, f_prev / g_prev read and written, one ring column of dF / dG written, up to m of
  // dF read (the upper bound is priced)
  GfvProfScope ps_(GFV_K_MISC, 0, (12.0 + 12.0 + 4 * 12.0 + 2 * 12.0 + 12.0 * m) * N, stream);
  const GramArgs a{uvp_node, x_backup, chunk_beg, chunk_end, gchunk_ptr, f_prev, g_prev, dF, dG, aa_state, r_prev, gamma,
                   partial_ws, counter, aa_table, step, reg, restart, N, n_chunks, B, K_max, m, start};
  GFV_LAUNCH(anderson_gram_kernel, dim3((n_chunks + AA_WAVES - 1) / AA_WAVES), dim3(64 * AA_WAVES), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_anderson_mix(float* uvp_node, const float* f_cur, int32_t N, const int32_t* chunk_beg, const int32_t* chunk_end,
                                const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, int32_t m, double beta, const float* dF,
                                const float* dG, const double* gamma, const float* aa_table, int32_t K_max, const int32_t* step,
                                void* stream) {
  if (!uvp_node || !f_cur || !dF || !dG || !gamma || !aa_table || !step) return GFV_ERR_ARG;
  if (aa_bad_tables(chunk_beg, chunk_end, gchunk_ptr, N, n_chunks, B, K_max, m)) return GFV_ERR_ARG;
  if (!(beta > 0.0) || beta > 1.0) return GFV_ERR_ARG;                     // outside (0, 1] or NaN
  if (reinterpret_cast<size_t>(gamma) & 7) return GFV_ERR_ARG;
  // rows of an accelerated graph: uvp read and written, up to m columns of dG (and, with beta < 1, f and dF) read
  GfvProfScope ps_(GFV_K_MISC, 0, (24.0 + 12.0 * m * (beta < 1.0 ? 2 : 1) + (beta < 1.0 ? 12.0 : 0.0)) * N, stream);
  const MixArgs a{uvp_node, f_cur, chunk_beg, chunk_end, gchunk_ptr, dF, dG, gamma, aa_table, step, 1.0 - beta, N, n_chunks, B, K_max, m};
  GFV_LAUNCH(anderson_mix_kernel, dim3((n_chunks + AA_WAVES - 1) / AA_WAVES), dim3(64 * AA_WAVES), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
