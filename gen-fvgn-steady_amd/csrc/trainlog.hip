// Training log (gfv/trainlog.py): what a training step leaves behind for the host to read once per epoch - two
// launches issued eagerly behind the optimiser launches of a step, never part of a recorded list (the per-graph losses differ per
// recorded list, the pool entries per step).
//
// gfv_train_log_norms: per bucket of (offset, count) segments of the flat buffers, sum g^2, sum p^2 and the count of non-finite
// g, in double.  Summation order - fixed, a function of the LOGICAL index j = 0 .. n - 1 of a bucket's concatenated elements
// (segment after segment in table order) alone: not of the grid, of timing, of where a segment lies in memory or of which load
// instruction fetched an element; no floating-point atomics (tests/trainlog_ref.py restates it in numpy, bit for bit):
//   * per element: the fp32 value widened to double and squared (exact); the non-finite mark is 1.0 or 0.0;
//   * per chunk c of a bucket (logical elements 1024 c .. min(1024 (c + 1), n) - 1): one wave; lane l adds, starting from +0.0,
//     the elements of its quads 1024 c + 256 r + 4 l + (0, 1, 2, 3), r = 0, 1, 2, 3, in ascending logical order; the 64 lane
//     sums fold by the xor butterfly of gfv_wave_sum (levels 32 .. 1); three doubles per chunk go to the workspace;
//   * per bucket, by the workgroup that arrives last: one wave; lane l adds the chunk sums l, l + 64, ... of the bucket in
//     ascending order (gfv_fold_chunks), then the same butterfly.
// Loads: a quad that lies inside one segment at a 16-byte aligned address is one 16-byte load per buffer, any other quad is
// read by element - the values and their order are the same either way.  Parameters start on 16-byte boundaries, so a
// segment is read by 16-byte loads wherever its offset in memory and its logical offset in the bucket agree modulo 4.
// Nothing outside a segment is read.  Hand-off of the partials: the write-through arrival of gfv_reduce.h (thread 0 stores the
// workgroup's twelve doubles with gfv_st_agent, the fold reads with gfv_ld_agent; no fence - a release fence here would write
// back what Adam has just left dirty in the L2: all of p, m and v).
//
// gfv_train_log_append: one workgroup writes one ring row, advances the 64-bit cursor and updates the per-entry table in slot
// order (one thread: an entry may appear twice in a batch, the later slot wins).  Row and table layouts: include/gfv.h.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"

namespace {

constexpr int TL_WAVES = 4;
constexpr int TL_CHUNK = GFV_TRAIN_LOG_CHUNK;
constexpr int TL_QUADS = TL_CHUNK / 256;        // quads per lane and chunk
constexpr int TL_SUMS = 3;
constexpr int MAXB = GFV_POOL_MAX_GRAPHS;
static_assert(TL_CHUNK % 256 == 0, "a chunk is whole rounds of 64 quads");

// bucket_tab [K, 4] int64: {first segment, one past the last segment, first chunk, elements}
enum { BT_SEG0 = 0, BT_SEG1 = 1, BT_CHUNK0 = 2, BT_ELEMS = 3 };

static __device__ __forceinline__ long tl_chunks(long n) { return (n + TL_CHUNK - 1) / TL_CHUNK; }

// the segment that holds logical element j (j below the bucket's element count: the walk ends inside the table)
struct SegCursor {
  const long* segs;
  int s;
  long lo, hi, off;
  __device__ __forceinline__ void seek(long j) {
    while (j >= hi) {
      ++s;
      lo = hi;
      off = segs[2 * s];
      hi = lo + segs[2 * s + 1];
    }
  }
};

static __device__ __forceinline__ void tl_add(float gv, float pv, double (&s)[TL_SUMS]) {
  const double gd = (double)gv, pd = (double)pv;
  s[0] += gd * gd;
  s[1] += pd * pd;
  s[2] += (fabsf(gv) <= 3.402823466e+38f) ? 0.0 : 1.0;      // (false for inf and NaN)
}

__global__ __launch_bounds__(64 * TL_WAVES) void train_log_norms_kernel(const float* __restrict__ g, const float* __restrict__ p,
                                                                        const long* __restrict__ segs,
                                                                        const long* __restrict__ bucket_tab, int K, int n_chunks,
                                                                        int vec_ok, double* sums, double* partial, int* counter) {
  __shared__ double red[TL_WAVES][TL_SUMS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.x * TL_WAVES + wave;
  double s[TL_SUMS] = {0.0, 0.0, 0.0};
  if (c < n_chunks) {
    int k = 0;
    while (k < K - 1 && bucket_tab[4 * (k + 1) + BT_CHUNK0] <= c) ++k;
    const long* bt = bucket_tab + 4 * k;
    const long n = bt[BT_ELEMS];
    const long base = (long)(c - bt[BT_CHUNK0]) * TL_CHUNK;
    SegCursor cur{segs, (int)bt[BT_SEG0], 0, 0, 0};
    cur.off = segs[2 * cur.s];
    cur.hi = segs[2 * cur.s + 1];
    for (int r = 0; r < TL_QUADS; ++r) {
      const long j0 = base + 256 * r + 4 * lane;
      if (j0 >= n) break;
      cur.seek(j0);
      const long a = cur.off + (j0 - cur.lo);
      if (vec_ok && j0 + 4 <= cur.hi && (a & 3) == 0) {
        const float4 gv = *reinterpret_cast<const float4*>(g + a);
        const float4 pv = *reinterpret_cast<const float4*>(p + a);
        tl_add(gv.x, pv.x, s); tl_add(gv.y, pv.y, s); tl_add(gv.z, pv.z, s); tl_add(gv.w, pv.w, s);
      } else {
        for (int e = 0; e < 4; ++e) {
          const long j = j0 + e;
          if (j >= n) break;
          cur.seek(j);
          const long i = cur.off + (j - cur.lo);
          tl_add(g[i], p[i], s);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < TL_SUMS; ++q) s[q] = gfv_wave_sum(s[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < TL_SUMS; ++q) red[wave][q] = s[q];
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 0; w < TL_WAVES; ++w) {
      const int cw = blockIdx.x * TL_WAVES + w;
      if (cw >= n_chunks) break;
#pragma unroll
      for (int q = 0; q < TL_SUMS; ++q) gfv_st_agent(partial + (size_t)TL_SUMS * cw + q, red[w][q]);
    }
  }
  if (!gfv_arrive_last_writethrough(counter)) return;
  for (int k = wave; k < K; k += TL_WAVES) {
    const long* bt = bucket_tab + 4 * k;
    const int c0 = (int)bt[BT_CHUNK0], c1 = c0 + (int)tl_chunks(bt[BT_ELEMS]);
    double f[TL_SUMS];
    gfv_fold_chunks(partial, c0, min(c1, n_chunks), lane, f);
#pragma unroll
    for (int q = 0; q < TL_SUMS; ++q) f[q] = gfv_wave_sum(f[q]);
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < TL_SUMS; ++q) sums[TL_SUMS * k + q] = f[q];
    }
  }
  if (tid == 0) *counter = 0;     // (every thread of this workgroup is past its read of s_last: reusable by the next launch)
}

struct AppendArgs {
  unsigned* ring;             // [capacity, row_words]
  unsigned long long* cursor; // appends so far
  const float* state;         // adam_state
  const float* hyper;
  const float* loss;
  const unsigned* losses;     // [B, 4]
  const unsigned* guard;      // guard[8] or NULL
  const int* accum;           // accum[8] or NULL
  const unsigned* sums;       // [K, 3] doubles as word pairs, or NULL with K == 0
  int* table;                 // [n_entries, 8] or NULL
  int capacity, max_graphs, K, B, row_words;
  int entry[MAXB];
};

constexpr int AP_TPB = 256;

__global__ __launch_bounds__(AP_TPB) void train_log_append_kernel(const AppendArgs A) {
  const int tid = threadIdx.x;
  const unsigned long long ord = *A.cursor;
  unsigned* row = A.ring + (size_t)(ord % (unsigned long long)A.capacity) * A.row_words;
  const int MG = A.max_graphs;
  const int terms0 = GFV_TRAIN_LOG_HEAD, entry0 = terms0 + 4 * MG, sums0 = GFV_TRAIN_LOG_HEAD + ((5 * MG + 1) & ~1);
  const int decision = A.guard ? (int)A.guard[4] : 0;
  const int apply = A.accum ? A.accum[3] : 1;
  const int applied = (apply != 0 && (decision & (GFV_GUARD_SKIP_NONFINITE | GFV_GUARD_SKIP_FLAG)) == 0) ? 1 : 0;
  for (int w = tid; w < A.row_words; w += AP_TPB) {
    unsigned v = 0u;
    if (w < terms0) {
      switch (w) {
        case 0: v = (unsigned)(ord & 0xffffffffull); break;
        case 1: v = (unsigned)(ord >> 32); break;
        case 2: v = __float_as_uint(A.state[0]); break;
        case 3: v = __float_as_uint(A.loss[0]); break;
        case 4: v = __float_as_uint(A.hyper[0]); break;
        case 5: v = (unsigned)A.B; break;
        case 6: v = A.guard ? A.guard[2] : 0x7fc00000u; break;
        case 7: v = A.guard ? A.guard[3] : 0x3f800000u; break;
        case 8: v = (unsigned)decision; break;
        case 9: v = (unsigned)apply; break;
        case 10: v = (unsigned)applied; break;
        default: break;
      }
    } else if (w < entry0) {
      const int q = w - terms0;
      v = q < 4 * A.B ? A.losses[q] : 0u;
    } else if (w < entry0 + MG) {
      v = (unsigned)A.entry[w - entry0];
    } else if (w >= sums0) {
      v = A.sums[w - sums0];
    }
    row[w] = v;
  }
  if (tid == 0 && A.table) {
    for (int b = 0; b < A.B; ++b) {
      const int e = A.entry[b];
      if (e < 0) continue;
      int* t = A.table + (size_t)GFV_TRAIN_LOG_ENTRY_RECORD * e;
      t[0] += 1;
      t[1] = (int)(unsigned)(ord & 0xffffffffull);
#pragma unroll
      for (int q = 0; q < 4; ++q) t[2 + q] = (int)A.losses[4 * b + q];
      t[6] = 0;
      t[7] = 0;
    }
  }
  __syncthreads();                 // every thread has read the cursor
  if (tid == 0) *A.cursor = ord + 1ull;
}

}  // namespace

extern "C" int64_t gfv_train_log_chunks(int64_t n_elems) { return n_elems <= 0 ? 0 : (n_elems + TL_CHUNK - 1) / TL_CHUNK; }

// workspace = [arrival counter: int32 in an 8-byte header, zero between launches][n_chunks x 3 partial sums: double]
extern "C" size_t gfv_train_log_workspace_bytes(int64_t n_chunks) {
  return 8 + (size_t)(n_chunks > 0 ? n_chunks : 0) * TL_SUMS * sizeof(double);
}

extern "C" int32_t gfv_train_log_row_words(int32_t max_graphs, int32_t K) {
  if (max_graphs < 1 || max_graphs > MAXB || K < 0 || K > GFV_TRAIN_LOG_MAX_BUCKETS) return GFV_ERR_ARG;
  return GFV_TRAIN_LOG_HEAD + ((5 * max_graphs + 1) & ~1) + 2 * TL_SUMS * K;
}

extern "C" int gfv_train_log_norms(const float* g, const float* p, const int64_t* segs, const int64_t* bucket_tab, int32_t K,
                                   int64_t n_chunks, double* sums, void* workspace, void* stream) {
  if (K < 0 || K > GFV_TRAIN_LOG_MAX_BUCKETS) return GFV_ERR_ARG;
  if (K == 0) return GFV_OK;
  if (!g || !p || !segs || !bucket_tab || !sums || !workspace || (reinterpret_cast<size_t>(workspace) & 7)) return GFV_ERR_ARG;
  if (n_chunks < 1 || n_chunks > 0x7fffffffll - TL_WAVES) return GFV_ERR_ARG;
  // g and p read once over the segments: 8 bytes per element, priced by the chunk count (an upper bound)
  GfvProfScope ps_(GFV_K_MISC, 0, 8.0 * TL_CHUNK * (double)n_chunks, stream);
  static_assert(sizeof(long) == sizeof(int64_t), "segment table words");
  const int vec_ok = ((reinterpret_cast<size_t>(g) | reinterpret_cast<size_t>(p)) & 15) == 0;
  int* counter = reinterpret_cast<int*>(workspace);
  double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + 8);
  GFV_LAUNCH(train_log_norms_kernel, dim3((unsigned)((n_chunks + TL_WAVES - 1) / TL_WAVES)), dim3(64 * TL_WAVES), 0,
             (hipStream_t)stream, g, p, reinterpret_cast<const long*>(segs), reinterpret_cast<const long*>(bucket_tab), (int)K,
             (int)n_chunks, vec_ok, sums, partial, counter);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_train_log_append(void* ring, int32_t capacity, int32_t max_graphs, int32_t K, int64_t* cursor,
                                    const float* state, const float* hyper, const float* loss, const float* losses, int32_t B,
                                    const float* guard, const float* accum, const int32_t* entry, const double* sums,
                                    int32_t* table, int32_t n_entries, void* stream) {
  if (!ring || capacity < 1 || max_graphs < 1 || max_graphs > MAXB || B < 1 || B > max_graphs) return GFV_ERR_ARG;
  if (K < 0 || K > GFV_TRAIN_LOG_MAX_BUCKETS || (K > 0 && !sums)) return GFV_ERR_ARG;
  if (!cursor || !state || !hyper || !loss || !losses || (table && n_entries < 1)) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(ring) & 7) || (reinterpret_cast<size_t>(cursor) & 7)) return GFV_ERR_ARG;
  AppendArgs a{reinterpret_cast<unsigned*>(ring), reinterpret_cast<unsigned long long*>(cursor), state, hyper, loss,
               reinterpret_cast<const unsigned*>(losses), reinterpret_cast<const unsigned*>(guard),
               reinterpret_cast<const int*>(accum), reinterpret_cast<const unsigned*>(sums), table, capacity, max_graphs, K, B,
               gfv_train_log_row_words(max_graphs, K), {}};
  for (int b = 0; b < max_graphs; ++b) {
    const int e = (entry && b < B) ? entry[b] : -1;
    if (e < -1 || (table && e >= n_entries)) return GFV_ERR_ARG;
    a.entry[b] = e;
  }
  GfvProfScope ps_(GFV_K_MISC, 0, 4.0 * a.row_words, stream);
  GFV_LAUNCH(train_log_append_kernel, dim3(1), dim3(AP_TPB), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
