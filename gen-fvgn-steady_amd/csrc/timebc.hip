// Unsteady boundary data (gfv/timebc.py): the Dirichlet velocity targets and the source coefficient as functions of
// time, rewritten on the device for the field about to be computed.  ONE launch behind the launch that advances the field
// (gfv_rollout_advance, gfv_march_advance); it follows the clock word that launch writes, the idea of GFV_SCHED_FOLLOW.
//
// With c = *clock + 1 + ctl[0] (the field about to be computed), per graph b: t = (double)c * (double)dt[b], g_v and g_s the two
// waveforms of b's records at t (include/gfv.h has the formulas; every operation is ONE IEEE double operation in the order
// written there, nothing contracted - the unit is built with -ffp-contract=off like the rest of the library):
//   row i of graph b, node_type[i] in the mask:  y[i, 0:2] = (float)(g_v * (double)y0[i, 0:2])            (velocity channel on)
//   every row i of graph b:                      x_backup[i, 8] = x[i, 8] = (float)(g_s * (double)theta0[b])  (source channel on)
//   thread b < B:                                theta5[b * ld] = the same float;  hist[c - 1, b] = (t, g_v, g_s)
// The kernel reads y0, theta0, the records and the tables and writes y, theta5, the feature column and the history: it never reads
// what it writes, so a launch that finds the clock it found before (an inner iteration or a held step of a march) writes the same
// bits again.  No arrival counter, no atomics, no grid barrier: a thread needs nothing another thread wrote.  One thread per row;
// the threads of a graph read the same record words (one cache line, broadcast).
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"

namespace {

constexpr int TB_TPB = 256;
constexpr double TB_TWO_PI = 6.283185307179586;   // the double nearest 2 pi (numpy's 2.0 * np.pi)
static_assert(GFV_TIME_BC_RECORD == 8 && GFV_TIME_BC_TABLE_MAX == 1024 && GFV_TIME_BC_HIST == 3, "include/gfv.h");

struct TimeBcArgs {
  const int* clock;        // one word: fields written so far
  const int* ctl;          // [GFV_TIME_BC_CTL]: word 0 the clock offset
  const double* rec;       // [B, 2, GFV_TIME_BC_RECORD]
  const double* tab;       // [B, 2, 2, GFV_TIME_BC_TABLE_MAX]: times, values of the slot (b, channel); may be NULL without tables
  const float* dt;         // [B]
  const int* batch;        // [N]
  const int* node_type;    // [N]
  const float* y0;         // [N, 2]
  float* y;                // [N, 2]
  const float* theta0;     // [B]
  float* theta5;           // element (b, 5) at theta5[b * ld_theta]
  float* x_backup;         // [N, 12] or NULL
  float* x;                // [N, 12] or NULL
  double* hist;            // [K_max, B, 3] or NULL
  int ld_theta, N, B, K_max, type_mask, channels;
};

// g(t) of one record; tab_slot: the slot's times [TABLE_MAX] followed by its values [TABLE_MAX]
__device__ double tb_wave(const double* __restrict__ r, const double* __restrict__ tab_slot, double t) {
  const int kind = (int)r[0];
  switch (kind) {
    case GFV_TIME_BC_CONST:
      return r[1];
    case GFV_TIME_BC_RAMP_LINEAR:
    case GFV_TIME_BC_RAMP_SMOOTH: {
      const double g0 = r[1], g1 = r[2], t0 = r[3], t1 = r[4];
      double s = (t - t0) / (t1 - t0);
      s = fmin(fmax(s, 0.0), 1.0);
      if (kind == GFV_TIME_BC_RAMP_SMOOTH) {
        const double s2 = s * s, w = 3.0 - 2.0 * s;
        s = s2 * w;
      }
      const double d = g1 - g0, p = d * s;
      return g0 + p;
    }
    case GFV_TIME_BC_SINE: {
      const double mean = r[1], amp = r[2], freq = r[3], phase = r[4], start = r[5];
      const double tau = fmax(t - start, 0.0);
      const double w = TB_TWO_PI * freq, a = w * tau, arg = a + phase;
      const double p = amp * sin(arg);
      return mean + p;
    }
    case GFV_TIME_BC_TABLE:
    case GFV_TIME_BC_TABLE_PERIODIC: {
      int n = (int)r[1];
      if (!tab_slot || n < 1) return 1.0;
      n = min(n, GFV_TIME_BC_TABLE_MAX);
      const double* T = tab_slot;
      const double* V = tab_slot + GFV_TIME_BC_TABLE_MAX;
      const double ta = T[0], tb = T[n - 1];
      if (kind == GFV_TIME_BC_TABLE_PERIODIC && n >= 2) {
        const double span = tb - ta;
        double m = fmod(t - ta, span);
        if (m < 0.0) m = m + span;
        t = ta + m;
      }
      if (t <= ta) return V[0];
      if (t >= tb) return V[n - 1];
      int lo = 0, hi = n - 1;                     // T[lo] <= t < T[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (T[mid] <= t) lo = mid; else hi = mid;
      }
      const double f = (t - T[lo]) / (T[hi] - T[lo]);
      const double d = V[hi] - V[lo], p = d * f;
      return V[lo] + p;
    }
    default:
      return 1.0;                                  // (GFV_TIME_BC_NONE: the identity)
  }
}

__global__ __launch_bounds__(TB_TPB) void time_bc_kernel(const TimeBcArgs A) {
  const long long cl = (long long)(*A.clock) + 1 + (long long)A.ctl[0];
  const double c = (double)cl;
  const int i = blockIdx.x * TB_TPB + threadIdx.x;
  const bool vel = (A.channels & 1) != 0, src = (A.channels & 2) != 0;
  if (i < A.N) {
    const int b = A.batch[i];
    if (b >= 0 && b < A.B) {
      const double t = c * (double)A.dt[b];
      const double* r = A.rec + (size_t)b * 2 * GFV_TIME_BC_RECORD;
      const double* ts = A.tab ? A.tab + (size_t)b * 4 * GFV_TIME_BC_TABLE_MAX : nullptr;
      const int nt = A.node_type[i];
      if (vel && nt >= 0 && nt < 32 && ((A.type_mask >> nt) & 1)) {
        const double g = tb_wave(r, ts, t);
        const float2 base = *reinterpret_cast<const float2*>(A.y0 + 2 * (size_t)i);
        float2 out;
        out.x = (float)(g * (double)base.x);
        out.y = (float)(g * (double)base.y);
        *reinterpret_cast<float2*>(A.y + 2 * (size_t)i) = out;
      }
      if (src && (A.x_backup || A.x)) {
        const double g = tb_wave(r + GFV_TIME_BC_RECORD, ts ? ts + 2 * GFV_TIME_BC_TABLE_MAX : nullptr, t);
        const float v = (float)(g * (double)A.theta0[b]);
        if (A.x_backup) A.x_backup[(size_t)i * 12 + 8] = v;
        if (A.x) A.x[(size_t)i * 12 + 8] = v;
      }
    }
  }
  if (i < A.B) {
    const int b = i;
    const double t = c * (double)A.dt[b];
    const double* r = A.rec + (size_t)b * 2 * GFV_TIME_BC_RECORD;
    const double* ts = A.tab ? A.tab + (size_t)b * 4 * GFV_TIME_BC_TABLE_MAX : nullptr;
    const double gv = vel ? tb_wave(r, ts, t) : 1.0;
    const double gs = src ? tb_wave(r + GFV_TIME_BC_RECORD, ts ? ts + 2 * GFV_TIME_BC_TABLE_MAX : nullptr, t) : 1.0;
    if (src) A.theta5[(size_t)b * A.ld_theta] = (float)(gs * (double)A.theta0[b]);
    if (A.hist && cl >= 1 && cl <= (long long)A.K_max) {
      double* h = A.hist + ((size_t)(cl - 1) * A.B + b) * GFV_TIME_BC_HIST;
      h[0] = t;
      h[1] = gv;
      h[2] = gs;
    }
  }
}

}  // namespace

extern "C" int gfv_time_bc_update(const int32_t* clock, const int32_t* ctl, const double* rec, const double* tab, const float* dt,
                                  const int32_t* batch, const int32_t* node_type, int32_t N, int32_t B, const float* y0, float* y,
                                  const float* theta0, float* theta5, int32_t ld_theta, float* x_backup, float* x, double* hist,
                                  int32_t K_max, int32_t type_mask, int32_t channels, void* stream) {
  if (!clock || !ctl || !rec || !dt || !batch || !node_type) return GFV_ERR_ARG;
  if (N < 1 || B < 1 || (channels & ~3) || !(channels & 3) || (type_mask & ~63)) return GFV_ERR_ARG;
  if ((channels & 1) && (!y0 || !y || y0 == y || ((reinterpret_cast<size_t>(y0) | reinterpret_cast<size_t>(y)) & 7))) return GFV_ERR_ARG;
  if ((channels & 2) && (!theta0 || !theta5 || ld_theta < 1)) return GFV_ERR_ARG;
  if (hist && K_max < 1) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(rec) | reinterpret_cast<size_t>(tab) | reinterpret_cast<size_t>(hist)) & 7) return GFV_ERR_ARG;
  // 8 B of y0 read and 8 B of y written per masked row (the host does not know how many: all of them here), batch and node type
  // read, the feature column written twice
  GfvProfScope ps_(GFV_K_MISC, 0, ((channels & 1) ? 16.0 : 0.0) * N + 8.0 * N + ((channels & 2) ? 8.0 : 0.0) * N, stream);
  const TimeBcArgs a{clock, ctl, rec, tab, dt, batch, node_type, y0, y, theta0, theta5, x_backup, x, hist,
                     ld_theta, N, B, K_max, type_mask, channels};
  const int rows = N > B ? N : B;
  GFV_LAUNCH(time_bc_kernel, dim3((rows + TB_TPB - 1) / TB_TPB), dim3(TB_TPB), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
