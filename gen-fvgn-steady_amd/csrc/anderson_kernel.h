// Anderson acceleration AA(m), the two kernels, written ONCE for both forms:
//   rollout form (SLOT = false; csrc/anderson.hip: gfv_anderson_gram / gfv_anderson_mix, behind gfv/rollout.py) - rings addressed
//     by batched node row, the step index is the rollout's step counter, the record is the row aa_table[k, b];
//   slot form (SLOT = true; csrc/sweep_anderson.hip: gfv_sweep_anderson_gram / gfv_sweep_anderson_mix, behind gfv/sweep.py) - a
//     ring row is b * ring_stride + (the node's index inside its own graph), so that a swap of a neighbour to an entry of another
//     size moves nothing under a live slot's columns; the step index is the slot's own age; a slot whose `done` is set when the
//     launch starts is skipped entirely; a step whose fp32 quotient || f || / || g || is below ctl.tol is a plain step (depth 0,
//     the column kept), so that a step that can latch always advances to the model's own output; the record is aa_slot[b] and
//     the counts aa_count[b].
// The per-row arithmetic, the 46-sum fold, the decision (Cholesky included) and the mix are the same instructions in both forms:
// what differs is addressing, the step index, the liveness test and where the record goes, all behind `if (SLOT)` on a template
// constant.
// Per graph b, over its node rows x 3 channels in fp32:  x = x_backup[:, 0:3],  g = uvp_node (the model's output),  f = g - x.
//   gram   per row: f; with a previous pair, ring column dF[head] = f - f_prev, dG[head] = g - g_prev (fp32); then
//          f_prev = f, g_prev = g.  Over the mk = min(cnt + has_prev, m) valid columns (the new one included), in
//          double: the upper triangle of dF^T dF, dF^T f, ||f||^2, ||g||^2.  The workgroup that arrives last decides
//          per graph (restart / plain step / solve), writes gamma[b] in ring-slot order and the record.
//   mix    rows of a graph with depth > 0:  uvp_node = g - (1-beta) f - sum_j gamma_j (dG_j - (1-beta) dF_j), j in
//          ascending ring slot, in double, rounded to fp32 once.  Rows of a graph with depth 0 are not written.
// The difference form keeps a row whose g never changes (a Dirichlet node: dG = 0, f = 0 exactly) bit for bit.
// Summation order: csrc/gfv_reduce.h, with the butterfly's tree formed in LDS (aa_tree_sum); the arrival counter is left at zero
// (all-fence form).  The sums of a graph do not depend on its neighbours in the batch.
// The column loops are unrolled at compile time over GFV_AA_MAX_DEPTH slots with run-time (wave-uniform) masks: every accumulator
// has a constant index and stays in a register.
#pragma once
#include "../../include/gfv.h"
#include "gfv_common.h"
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
  float* f_prev;              // [R,3]     R = N (rollout form) or B * ring_stride (slot form)
  float* g_prev;              // [R,3]
  float* dF;                  // [m][R,3]
  float* dG;                  // [m][R,3]
  int* aa_state;              // [B,4]: cnt, head, has_prev, restarts
  double* r_prev;             // [B]
  double* gamma;              // [B,8]
  double* partial;            // [n_chunks, AA_P]
  int* counter;               // arrival counter
  float* table;               // rollout form: [K_max,B,4]
  const int* step;            // rollout form: the rollout's step counter
  const float* ctl;           // slot form: the sweep's control words; ctl[0] is tol
  const int* slots;           // slot form: [B,4] age, streak, done, reserved (read only)
  float* aa_slot;             // slot form: [B,4] (|| f ||, || g ||, depth, flags) of the slot's last live step
  int* aa_count;              // slot form: [B,4] accelerated steps, NONFINITE, GROWTH, SINGULAR restarts
  double reg, restart;
  int N, n_chunks, B, K_max, m, start, ring_stride;
};

struct MixArgs {
  float* uvp_node;            // [N,3]
  const float* f_cur;         // [R,3]: f of this step (what the gram launch left in f_prev)
  const int* chunk_beg;
  const int* chunk_end;
  const int* gchunk_ptr;
  const float* dF;
  const float* dG;
  const double* gamma;        // [B,8]
  const float* table;         // rollout form: [K_max,B,4]
  const int* step;
  const int* slots;           // slot form
  const float* aa_slot;       // slot form
  double omb;                 // 1 - beta
  int N, n_chunks, B, K_max, m, ring_stride;
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

// Where node row i of graph b lives in the rings: the row itself (rollout form), or the node's index inside its own graph placed
// in the slot's region (slot form; -1 for a node that does not fit the stride: the host refuses such an entry, nothing is
// touched here).
template <bool SLOT>
__device__ __forceinline__ long aa_ring_row(const int* chunk_beg, const int* gchunk_ptr, int b, int i, int ring_stride) {
  if (!SLOT) return i;
  const int local = i - chunk_beg[gchunk_ptr[b]];
  if (local < 0 || local >= ring_stride) return -1;
  return (long)b * ring_stride + local;
}

template <bool SLOT>
__global__ __launch_bounds__(64 * AA_WAVES) void anderson_gram_kernel(const GramArgs A) {
  __shared__ double s_tile[AA_WAVES][AA_P][AA_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.x * AA_WAVES + wave;
  const int m = A.m;
  double (*tile)[AA_LD] = s_tile[wave];
  if (c < A.n_chunks) {
    const int b = gfv_chunk_graph(A.gchunk_ptr, A.B, c);
    const bool live = !SLOT || __builtin_amdgcn_readfirstlane(A.slots[4 * b + 2]) == 0;   // (a frozen slot: nothing changes)
    if (live) {
      const int* st = A.aa_state + 4 * b;
      const int cnt = __builtin_amdgcn_readfirstlane(min(max(st[0], 0), m));
      const int head = __builtin_amdgcn_readfirstlane(min(max(st[1], 0), m - 1));
      const int has_prev = __builtin_amdgcn_readfirstlane(st[2] != 0);
      const int mk = min(cnt + has_prev, m);
      const int vmask = __builtin_amdgcn_readfirstlane(has_prev ? aa_valid_mask(head, mk, m) : 0);
      const size_t col = SLOT ? (size_t)A.B * A.ring_stride * 3 : (size_t)A.N * 3;
      const int beg = A.chunk_beg[c], end = min(A.chunk_end[c], A.N);
      double s[AA_P];
#pragma unroll
      for (int q = 0; q < AA_P; ++q) s[q] = 0.0;
      for (int i = beg + lane; i < end; i += 64) {
        if (i < 0) continue;
        const long rr = aa_ring_row<SLOT>(A.chunk_beg, A.gchunk_ptr, b, i, A.ring_stride);
        if (rr < 0) continue;
        const size_t r = (size_t)rr * 3;
        const float* u = A.uvp_node + (size_t)i * 3;
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
  }
  if (!gfv_arrive_last_all_fence(A.counter)) return;
  const int k_roll = SLOT ? 0 : gfv_ld_agent(A.step);
  const float tol = SLOT ? A.ctl[0] : 0.f;
  for (int b = wave; b < A.B; b += AA_WAVES) {
    if (SLOT && A.slots[4 * b + 2] != 0) continue;      // (wave-uniform: the whole wave skips a frozen slot)
    const int k = SLOT ? A.slots[4 * b] : k_roll;       // the step index: the slot's own age, or the rollout's counter
    // (rollout form: a full table is not written past and nothing is mixed: the host raises before)
    const bool room = SLOT || (k >= 0 && k < A.K_max);
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
    } else if (SLOT && (float)rf / (float)sqrt(gg) < tol) {
      // slot form: the quotient the advance forms as `rel` is below tol - a plain step, the column kept (a step that can latch
      // advances to the model's own output)
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
      float* row = SLOT ? A.aa_slot + (size_t)b * 4 : A.table + ((size_t)k * A.B + b) * 4;
      if (lane == 16) row[0] = (float)rf;
      if (lane == 17) row[1] = (float)sqrt(gg);
      if (lane == 18) row[2] = (float)depth;
      if (lane == 19) row[3] = (float)flags;
    }
    if (SLOT) {
      int* n = A.aa_count + 4 * b;
      if (lane == 20 && depth > 0) n[0] += 1;
      if (lane == 21 && flags == GFV_AA_NONFINITE) n[1] += 1;
      if (lane == 22 && flags == GFV_AA_GROWTH) n[2] += 1;
      if (lane == 23 && flags == GFV_AA_SINGULAR) n[3] += 1;
    }
  }
  __syncthreads();
  if (tid == 0) *A.counter = 0;
}

template <bool SLOT>
__global__ __launch_bounds__(64 * AA_WAVES) void anderson_mix_kernel(const MixArgs A) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.x * AA_WAVES + wave;
  if (c >= A.n_chunks) return;
  const int k = SLOT ? 0 : A.step[0];
  if (!SLOT && (k < 0 || k >= A.K_max)) return;
  const int b = gfv_chunk_graph(A.gchunk_ptr, A.B, c);
  if (SLOT && A.slots[4 * b + 2] != 0) return;                   // (a frozen slot's record is that of its last live step)
  const int depth = (int)(SLOT ? A.aa_slot[(size_t)b * 4 + 2] : A.table[((size_t)k * A.B + b) * 4 + 2]);
  if (depth <= 0) return;
  double gam[MD];
#pragma unroll
  for (int j = 0; j < MD; ++j) gam[j] = A.gamma[(size_t)MD * b + j];
  const int m = A.m;
  const double omb = A.omb;
  const size_t col = SLOT ? (size_t)A.B * A.ring_stride * 3 : (size_t)A.N * 3;
  const int beg = A.chunk_beg[c], end = min(A.chunk_end[c], A.N);
  for (int i = beg + lane; i < end; i += 64) {
    if (i < 0) continue;
    const long rr = aa_ring_row<SLOT>(A.chunk_beg, A.gchunk_ptr, b, i, A.ring_stride);
    if (rr < 0) continue;
    const size_t r = (size_t)rr * 3;
    float* u = A.uvp_node + (size_t)i * 3;
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

inline bool aa_bad_tables(const void* a, const void* b, const void* c, int32_t N, int32_t n_chunks, int32_t B, int32_t m) {
  return !a || !b || !c || N <= 0 || n_chunks <= 0 || B <= 0 || m < 1 || m > MD;
}
// reg negative or NaN; restart negative, NaN or in (0, 1]
inline bool aa_bad_gram_numbers(double reg, double restart) {
  return !(reg >= 0.0) || !(restart >= 0.0) || (restart > 0.0 && restart <= 1.0);
}
inline bool aa_bad_beta(double beta) { return !(beta > 0.0) || beta > 1.0; }      // outside (0, 1] or NaN
inline bool aa_misaligned8(const void* a, const void* b, const void* c) {
  return ((reinterpret_cast<size_t>(a) | reinterpret_cast<size_t>(b) | reinterpret_cast<size_t>(c)) & 7) != 0;
}
// bytes per node row the gram / mix launches move (the upper bound over the ring columns is priced)
inline double aa_gram_bytes(int m) { return 12.0 + 12.0 + 4 * 12.0 + 2 * 12.0 + 12.0 * m; }
inline double aa_mix_bytes(int m, double beta) { return 24.0 + 12.0 * m * (beta < 1.0 ? 2 : 1) + (beta < 1.0 ? 12.0 : 0.0); }

}  // namespace
