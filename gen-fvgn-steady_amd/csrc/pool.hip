// Pool training (gfv/pool.py BatchArena, gfv/pool_trainer.py): a batch of any entries of the device-resident pool assembled into
// FIXED memory by one launch, the prediction written back by one launch.  Contract: include/gfv.h (gfv_pool_*).
// Reference: the per-step host batching of Load_mesh/Graph_loader.py:405-480,830-1006 and Data_Pool.payback (370-396).
//
// Assembly.  The batched tensor of an attribute is the concatenation of the entries' pieces; a workgroup owns PA_QUADS 16-byte
// quads of that DESTINATION range, so the grid follows the bytes moved and every store is an aligned 16-byte store whatever word
// a piece starts at.  The piece starts and the index offsets of the batch are a prefix sum over the B entries, formed by every
// workgroup for its own attribute from the device-resident table (B <= 64 loads); the entry indices travel by value.
//
// Renewal (gfv/pool.py DevicePool.renew; Data_Pool.reset_env -> init_env, Graph_loader.py:154-229, Load_mesh.py:80-131): the
// boundary conditions of K entries re-drawn and their fields restarted by one elementwise launch, the K records by value.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"

namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_QUADS = 1024;                 // 16 KiB of destination per workgroup, four quads per thread
constexpr int MAXB = GFV_POOL_MAX_GRAPHS, MAXA = GFV_POOL_MAX_ATTRS, HEAD = GFV_POOL_ROW_HEAD;

struct PoolK {
  const long long* tab;       // device table
  int row;                    // int64 per table row
  int A, B, slice_chunk;
  int idx[MAXB];
  int info[MAXA];
  int* dst[MAXA];
  int blk0[MAXA + 1];         // first workgroup of every attribute; blk0[A] = the workgroup of the small arrays
  int* small[6];
};

// offset kind -> size of an entry (head columns: n, e, c, k, s, nchunk)
__device__ __forceinline__ long long pool_size_of(const long long* head, int kind) {
  switch (kind) {
    case 1: return head[0];
    case 2: return head[1];
    case 3: return 2 * head[1];
    case 4: return head[2];
    case 5: return head[3];
    case 6: return head[4];
    default: return 0;
  }
}

__device__ void pool_small_arrays(const PoolK& K) {
  __shared__ int s_n[MAXB + 1], s_c[MAXB + 1], s_q[MAXB + 1];
  const int tid = threadIdx.x, B = K.B, CH = K.slice_chunk;
  if (tid == 0) {
    int n = 0, c = 0, q = 0;
    for (int b = 0; b < B; ++b) {
      const long long* head = K.tab + (size_t)K.idx[b] * K.row;
      s_n[b] = n; s_c[b] = c; s_q[b] = q;
      const int nb = (int)head[0];
      n += nb; c += (int)head[2]; q += (nb + CH - 1) / CH;
    }
    s_n[B] = n; s_c[B] = c; s_q[B] = q;
  }
  __syncthreads();
  for (int b = tid; b <= B; b += PA_THREADS) {
    K.small[0][b] = s_n[b];   // gnode_ptr
    K.small[1][b] = s_c[b];   // gcell_ptr
    K.small[2][b] = s_q[b];   // gchunk_ptr
    K.small[3][b] = b;        // gunit_ptr
  }
  for (int b = 0; b < B; ++b) {
    const int n0 = s_n[b], n1 = s_n[b + 1], q0 = s_q[b], nq = s_q[b + 1] - q0;
    for (int j = tid; j < nq; j += PA_THREADS) {
      const int beg = n0 + j * CH;
      K.small[4][q0 + j] = beg;
      K.small[5][q0 + j] = min(beg + CH, n1);
    }
  }
}

__global__ __launch_bounds__(PA_THREADS) void pool_assemble_kernel(const PoolK K) {
  __shared__ int s_start[MAXB + 1];            // first destination word of every piece (s_start[B] = words of the batch)
  __shared__ int s_off[MAXB];                  // index offset of every piece
  __shared__ const int* s_src[MAXB];
  const int tid = threadIdx.x, blk = blockIdx.x, B = K.B;
  if (blk >= K.blk0[K.A]) {
    pool_small_arrays(K);
    return;
  }
  int a = 0;
  while (blk >= K.blk0[a + 1]) ++a;            // (uniform: at most MAXA steps)
  const int info = K.info[a], mode = info & 15, kind = (info >> 4) & 15;
  if (tid == 0) {
    long long start = 0, off = 0;
    for (int b = 0; b < B; ++b) {
      const long long* rowp = K.tab + (size_t)K.idx[b] * K.row;
      long long w = rowp[HEAD + K.A + a];
      if (mode == GFV_POOL_ROWPTR && b + 1 < B) w -= 1;    // n_i words per entry, n_last + 1 for the last one
      s_start[b] = (int)start;
      s_off[b] = (int)off;
      s_src[b] = reinterpret_cast<const int*>(rowp[HEAD + a]);
      start += w;
      off += pool_size_of(rowp, kind);
    }
    s_start[B] = (int)start;
  }
  __syncthreads();
  const int total = s_start[B];
  int* __restrict__ dst = K.dst[a];
  const bool add = mode == GFV_POOL_ADD || mode == GFV_POOL_ROWPTR;
  int b = 0;
  const long q0 = (long)(blk - K.blk0[a]) * PA_QUADS;
#pragma unroll
  for (int u = 0; u < PA_QUADS / PA_THREADS; ++u) {
    const long w0l = 4 * (q0 + u * PA_THREADS + tid);
    if (w0l >= total) break;
    const int w0 = (int)w0l;
    while (w0 >= s_start[b + 1]) ++b;          // (pieces of zero words are stepped over; w0 < total = s_start[B])
    if (w0 + 4 <= s_start[b + 1]) {
      // the whole quad belongs to one piece
      int4 v;
      if (mode == GFV_POOL_FILL) {
        v = make_int4(b, b, b, b);
      } else {
        const int* __restrict__ s = s_src[b] + (w0 - s_start[b]);
        if ((reinterpret_cast<size_t>(s) & 15) == 0) v = *reinterpret_cast<const int4*>(s);
        else v = make_int4(s[0], s[1], s[2], s[3]);
        if (add) { const int o = s_off[b]; v.x += o; v.y += o; v.z += o; v.w += o; }
      }
      *reinterpret_cast<int4*>(dst + w0) = v;
    } else {
      // a quad across a piece boundary, or the last words of the tensor: word by word
      int bb = b;
      const int w1 = min(w0 + 4, total);
      for (int w = w0; w < w1; ++w) {
        while (w >= s_start[bb + 1]) ++bb;
        int v = bb;
        if (mode != GFV_POOL_FILL) {
          v = s_src[bb][w - s_start[bb]];
          if (add) v += s_off[bb];
        }
        dst[w] = v;
      }
    }
  }
}

struct PaybackK {
  const long long* tab;
  int row, A, x_attr, B;
  int idx[MAXB];
  const float* uvp;
  float* raw;
  int N;
};

__global__ __launch_bounds__(256) void pool_payback_kernel(const PaybackK K) {
  __shared__ int s_n[MAXB + 1];
  __shared__ float* s_x[MAXB];                 // nullptr: a later position of the batch holds the same entry - skipped
  const int tid = threadIdx.x, B = K.B;
  if (tid == 0) {
    int n = 0;
    for (int b = 0; b < B; ++b) {
      const long long* rowp = K.tab + (size_t)K.idx[b] * K.row;
      s_n[b] = n;
      n += (int)rowp[0];
      bool later = false;
      for (int c = b + 1; c < B; ++c) later = later || K.idx[c] == K.idx[b];
      s_x[b] = later ? nullptr : reinterpret_cast<float*>(rowp[HEAD + K.x_attr]);
    }
    s_n[B] = n;
  }
  __syncthreads();
  const int N = min(K.N, s_n[B]);
  for (int i = blockIdx.x * 256 + tid; i < N; i += gridDim.x * 256) {
    int lo = 0, hi = B;                        // the graph of node i: s_n[lo] <= i < s_n[lo + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (i >= s_n[mid]) lo = mid; else hi = mid;
    }
    const float u0 = K.uvp[3 * (size_t)i], u1 = K.uvp[3 * (size_t)i + 1], u2 = K.uvp[3 * (size_t)i + 2];
    if (float* x = s_x[lo]) {
      float* r = x + 12 * (size_t)(i - s_n[lo]);
      r[0] = u0; r[1] = u1; r[2] = u2;
    }
    if (K.raw) {
      float* r = K.raw + 12 * (size_t)i;
      r[0] = u0; r[1] = u1; r[2] = u2;
    }
  }
}

// Renewal.  Elementwise: a workgroup owns RN_THREADS nodes of ONE entry (blk0: the first workgroup of every record), a thread one
// node.  The float64 profile keeps the operation order of DevicePool.reset_env's torch expression - every torch op there is a
// kernel of its own, so nothing is fused: contraction is off here whatever the build flags say.
constexpr int RN_THREADS = 256;
constexpr int NT_INFLOW = 1, NT_WALL = 3, NT_PRESS_POINT = 4, NT_IN_WALL = 5;   // NodeType (gfv/meshgen.py)

struct RenewK {
  gfv_renew_rec_t rec[MAXB];
  int blk0[MAXB + 1];
  int K;
};

#pragma clang fp contract(off)
__device__ __forceinline__ void renew_profile(const gfv_renew_rec_t& r, int kind, double px, double py, double lo, double hi,
                                              float& u, float& v, float& p) {
  u = 0.0f; v = 0.0f; p = 0.0f;
  switch (kind) {
    case GFV_RENEW_PARABOLIC: {
      const double yy = py - lo;
      const double d = (hi - lo) - 0.0;        // (max - min of yy: min(yy) is py_min - py_min)
      const double t1 = (6.0 * r.U) * yy;
      const double t2 = d - yy;
      const double t3 = d * d;
      u = (float)(t1 * (t2 / t3));
      break;
    }
    case GFV_RENEW_UNIFORM:
      u = (float)r.U;
      break;
    case GFV_RENEW_UNIFORM_AOA:
      u = (float)r.U * (float)r.cos_aoa;
      v = (float)r.U * (float)r.sin_aoa;
      break;
    case GFV_RENEW_TAYLOR_GREEN: {
      const double pi = 3.141592653589793;
      const double ax = (2.0 * pi) * px, ay = (2.0 * pi) * py, bx = (4.0 * pi) * px, by = (4.0 * pi) * py;
      u = (float)((r.U * sin(ax)) * cos(ay));
      v = (float)(((-r.U) * cos(ax)) * sin(ay));
      p = (float)(((-0.25) * r.U) * (cos(bx) + cos(by)));
      break;
    }
    default: break;
  }
}

__global__ __launch_bounds__(RN_THREADS) void pool_renew_kernel(const RenewK K) {
  const int blk = blockIdx.x;
  int lo = 0, hi = K.K;                        // the record of this workgroup: blk0[lo] <= blk < blk0[lo + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk >= K.blk0[mid]) lo = mid; else hi = mid;
  }
  const gfv_renew_rec_t& r = K.rec[lo];
  const int first = blk == K.blk0[lo];
  const int i = (blk - K.blk0[lo]) * RN_THREADS + (int)threadIdx.x;
  if (first && threadIdx.x < 13) {
    const int t = threadIdx.x;
    if (t < 9) r.theta[t] = r.coef[t];
    else if (t == 9) r.dt[0] = r.coef[9];
    else r.uvp_dim[t - 10] = r.coef[t];
  }
  if (i >= r.N) return;
  const double px = r.pos[2 * (size_t)i], py = r.pos[2 * (size_t)i + 1];
  const int nt = r.node_type[i];
  float u, v, p;
  renew_profile(r, r.init_kind, px, py, r.yrange[0], r.yrange[1], u, v, p);
  if (nt == NT_INFLOW || nt == NT_IN_WALL || nt == NT_PRESS_POINT) {
    float pi_;                                 // (the inlet call's pressure is not used: Load_mesh.py:109-118)
    renew_profile(r, r.inlet_kind, px, py, r.yrange[2], r.yrange[3], u, v, pi_);
  }
  if (nt == NT_WALL) { u = 0.0f; v = 0.0f; }
  if (nt == NT_IN_WALL) { u = u / 2.0f; v = v / 2.0f; p = p / 2.0f; }
  const float inv_u = 1.0f / (float)r.U;
  float* y = r.y + 2 * (size_t)i;
  y[0] = u * inv_u;
  y[1] = v * inv_u;
  float* x = r.x + 12 * (size_t)i;
  x[0] = u; x[1] = v; x[2] = p;
#pragma unroll
  for (int c = 0; c < 9; ++c) x[3 + c] = r.coef[c];
}

// what both entry points check of (table, batch) on the host
bool pool_batch_ok(const int64_t* table_host, const int64_t* table_dev, int32_t n_entries, int32_t n_attrs, const int32_t* idx,
                   int32_t B) {
  if (!table_host || !table_dev || !idx || n_entries < 1 || n_attrs < 1 || n_attrs > MAXA) return false;
  if (B < 1 || B > MAXB) return false;
  for (int b = 0; b < B; ++b)
    if (idx[b] < 0 || idx[b] >= n_entries) return false;
  return true;
}

}  // namespace

extern "C" size_t gfv_pool_args_bytes(void) { return sizeof(gfv_pool_args_t); }

extern "C" size_t gfv_pool_table_bytes(int32_t n_entries, int32_t n_attrs) {
  if (n_entries < 0 || n_attrs < 0) return 0;
  return (size_t)n_entries * (size_t)(HEAD + 2 * n_attrs) * sizeof(int64_t);
}

extern "C" int gfv_pool_table_check(const int64_t* table_host, int32_t n_entries, int32_t n_attrs, const int32_t* attr_info) {
  if (!table_host || !attr_info || n_entries < 1 || n_attrs < 1 || n_attrs > MAXA) return GFV_ERR_ARG;
  const int row = HEAD + 2 * n_attrs;
  for (int i = 0; i < n_entries; ++i) {
    const int64_t* r = table_host + (size_t)i * row;
    for (int k = 0; k < 6; ++k)
      if (r[k] < 0 || r[k] > 0x3fffffff) return GFV_ERR_ARG;
    for (int a = 0; a < n_attrs; ++a) {
      const int mode = attr_info[a] & 15, kind = (attr_info[a] >> 4) & 15;
      const int64_t src = r[HEAD + a], words = r[HEAD + n_attrs + a];
      if (mode > GFV_POOL_FILL || kind > 6 || words < 0 || words > 0x7fffffff) return GFV_ERR_ARG;
      if (mode == GFV_POOL_ROWPTR && words < 1) return GFV_ERR_ARG;
      if (mode != GFV_POOL_FILL && words > 0 && (src == 0 || (src & 3))) return GFV_ERR_ARG;
    }
  }
  return GFV_OK;
}

extern "C" int gfv_pool_assemble(const gfv_pool_args_t* args, void* stream) {
  if (!args) return GFV_ERR_ARG;
  const gfv_pool_args_t& g = *args;
  if (!pool_batch_ok(g.table_host, g.table_dev, g.n_entries, g.n_attrs, g.idx, g.B)) return GFV_ERR_ARG;
  if (g.B > g.max_graphs || g.slice_chunk < 1 || g.max_chunks < 0) return GFV_ERR_ARG;
  for (int k = 0; k < 6; ++k)
    if (!g.small[k]) return GFV_ERR_ARG;
  const int A = g.n_attrs, row = HEAD + 2 * A;
  PoolK K;
  K.tab = reinterpret_cast<const long long*>(g.table_dev);
  K.row = row; K.A = A; K.B = g.B; K.slice_chunk = g.slice_chunk;
  for (int b = 0; b < MAXB; ++b) K.idx[b] = b < g.B ? g.idx[b] : 0;
  double bytes = 0.0;
  int blocks = 0;
  for (int a = 0; a < MAXA; ++a) {
    K.info[a] = a < A ? g.attr_info[a] : 0;
    K.dst[a] = a < A ? reinterpret_cast<int*>(g.dst[a]) : nullptr;
    K.blk0[a] = blocks;
    if (a >= A) continue;
    const int mode = g.attr_info[a] & 15;
    if (mode > GFV_POOL_FILL || ((g.attr_info[a] >> 4) & 15) > 6) return GFV_ERR_ARG;
    long long words = 0;
    for (int b = 0; b < g.B; ++b) {
      long long w = g.table_host[(size_t)g.idx[b] * row + HEAD + A + a];
      if (w < 0) return GFV_ERR_ARG;
      if (mode == GFV_POOL_ROWPTR) {
        if (w < 1) return GFV_ERR_ARG;
        if (b + 1 < g.B) w -= 1;
      }
      words += w;
    }
    if (words > g.dst_cap_words[a] || words > 0x7fffffffLL) return GFV_ERR_ARG;   // the batch does not fit the arena
    if (words > 0 && (!g.dst[a] || (reinterpret_cast<size_t>(g.dst[a]) & 15))) return GFV_ERR_ARG;
    blocks += (int)((words + 4 * PA_QUADS - 1) / (4 * PA_QUADS));
    bytes += (mode == GFV_POOL_FILL ? 4.0 : 8.0) * (double)words;
  }
  for (int a = A; a <= MAXA; ++a) K.blk0[a] = blocks;
  K.blk0[A] = blocks;
  long long chunks = 0, nodes = 0;
  for (int b = 0; b < g.B; ++b) {
    const int64_t n = g.table_host[(size_t)g.idx[b] * row];
    if (n < 0) return GFV_ERR_ARG;
    nodes += n;
    chunks += (n + g.slice_chunk - 1) / g.slice_chunk;
  }
  if (chunks > g.max_chunks || nodes > 0x7fffffffLL) return GFV_ERR_ARG;
  for (int k = 0; k < 6; ++k) K.small[k] = g.small[k];
  GfvProfScope ps_(GFV_K_MISC, 0, bytes, stream);
  GFV_LAUNCH(pool_assemble_kernel, dim3(blocks + 1), dim3(PA_THREADS), 0, (hipStream_t)stream, K);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_pool_payback(const int64_t* table_host, const int64_t* table_dev, int32_t n_entries, int32_t n_attrs,
                                int32_t x_attr, const int32_t* idx, int32_t B, const float* uvp_node, int64_t N, float* raw,
                                void* stream) {
  if (!pool_batch_ok(table_host, table_dev, n_entries, n_attrs, idx, B)) return GFV_ERR_ARG;
  if (!uvp_node || x_attr < 0 || x_attr >= n_attrs) return GFV_ERR_ARG;
  const int row = HEAD + 2 * n_attrs;
  long long nodes = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t* r = table_host + (size_t)idx[b] * row;
    if (r[0] < 0 || r[HEAD + n_attrs + x_attr] != 12 * r[0] || (r[0] > 0 && !r[HEAD + x_attr])) return GFV_ERR_ARG;
    nodes += r[0];
  }
  if (nodes != N || N < 1 || N > 0x7fffffffLL) return GFV_ERR_ARG;
  PaybackK K;
  K.tab = reinterpret_cast<const long long*>(table_dev);
  K.row = row; K.A = n_attrs; K.x_attr = x_attr; K.B = B;
  for (int b = 0; b < MAXB; ++b) K.idx[b] = b < B ? idx[b] : 0;
  K.uvp = uvp_node; K.raw = raw; K.N = (int)N;
  GfvProfScope ps_(GFV_K_MISC, 0, (12.0 + 12.0 + (raw ? 12.0 : 0.0)) * (double)N, stream);
  long wgs = (N + 255) / 256;
  if (wgs > 2048) wgs = 2048;
  GFV_LAUNCH(pool_payback_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, K);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_pool_renew(const gfv_renew_rec_t* recs, int32_t K, void* stream) {
  if (!recs || K < 1 || K > MAXB) return GFV_ERR_ARG;
  RenewK R;
  long long blocks = 0;
  double bytes = 0.0;
  for (int k = 0; k < K; ++k) {
    const gfv_renew_rec_t& r = recs[k];
    if (!r.x || !r.y || !r.theta || !r.dt || !r.uvp_dim || !r.node_type || !r.pos || !r.yrange) return GFV_ERR_ARG;
    if (r.N < 1 || r.U == 0.0 || !(r.U - r.U == 0.0)) return GFV_ERR_ARG;      // (U - U != 0: infinite or NaN)
    if (r.inlet_kind < GFV_RENEW_NONE || r.inlet_kind > GFV_RENEW_TAYLOR_GREEN) return GFV_ERR_ARG;
    if (r.init_kind < GFV_RENEW_NONE || r.init_kind > GFV_RENEW_TAYLOR_GREEN) return GFV_ERR_ARG;
    for (int j = 0; j < k; ++j)
      if (recs[j].x == r.x) return GFV_ERR_ARG;                                 // one writer per entry
    R.rec[k] = r;
    R.blk0[k] = (int)blocks;
    blocks += (r.N + RN_THREADS - 1) / RN_THREADS;
    bytes += (16.0 + 4.0 + 48.0 + 8.0) * (double)r.N;
  }
  if (blocks > 0x7fffffffLL) return GFV_ERR_ARG;
  for (int k = K; k < MAXB; ++k) { R.rec[k] = recs[0]; R.blk0[k] = (int)blocks; }
  R.blk0[MAXB] = (int)blocks;
  R.K = K;
  GfvProfScope ps_(GFV_K_MISC, 0, bytes, stream);
  GFV_LAUNCH(pool_renew_kernel, dim3((unsigned)blocks), dim3(RN_THREADS), 0, (hipStream_t)stream, R);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
