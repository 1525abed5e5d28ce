// Adaptive time step of a march (gfv/timescheme.py `StepControl`): the step sized to a Courant-number target and the
// variable-step form of BDF2, decided on the device.  TWO launches behind the launch that advances the field, in place of the one
// of csrc/timescheme.hip; both follow the same clock word and read it, and the records, as they find them.
//
//   gfv_step_control_rate   one thread per cell: the cell's Courant rate (1 / time), a wavefront maximum per graph and one integer
//                           atomicMax on the float's bits per wavefront and graph into the rate slot of the clock's parity (the
//                           rates are >= +0, so the order of the bits is the order of the floats and the maximum is exact in any
//                           order); the other slot is cleared for the clock that comes next.  The workgroup that arrives last
//                           (gfv_reduce.h, the all-fence form: the atomics are the stores handed over) runs the controller per
//                           graph: dt_next, omega, the time, dt_eff, the history row.
//   gfv_step_control_rows   csrc/timescheme.hip's stream kernel with omega[b] read from the per-graph state the launch in front of
//                           it wrote: one thread per node row, float4 / float2 accesses.
//
// Parity: the launch at clock c reads dts[c & 1] (the step that produced field c) and writes dts[(c + 1) & 1] (the step that will
// produce field c + 1); it reads times[(c & 1) ^ 1] and writes times[c & 1]; it adds to rate[c & 1] - idempotent, a maximum - and
// clears rate[(c & 1) ^ 1]; the ring as in csrc/timescheme.hip.  No word it reads is one it writes, so a launch that finds the
// clock it found before writes the same bits everywhere.  The rule in full: include/gfv.h.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"

namespace {

constexpr int SC_TPB = 256;
enum { TS_SCHEME = 0, TS_BASE = 1 };
enum { SC_TBASE = 0, SC_COUNTER = 1 };
enum { SC_COURANT = 0, SC_GROW = 1, SC_SHRINK = 2, SC_MIN_FACTOR = 3, SC_MAX_FACTOR = 4 };
enum { SC_DT = 0, SC_OMEGA = 1, SC_CO = 2, SC_RATE = 3 };
static_assert(GFV_STEP_CONTROL_RECORD == 4 && GFV_STEP_CONTROL_PARAMS == 8 && GFV_STEP_CONTROL_STATE == 4, "include/gfv.h");
static_assert(GFV_TIME_SCHEME_BDF2 == 2, "include/gfv.h");

struct RateArgs {
  const float* x_backup;
  const float* uvp_dim;
  const float* dt;
  const int* crow;
  const int* knode;
  const float* kS;
  const float* area;
  const int* cbatch;
  int C, B;
  const int* clock;
  const int* rec;
  int* crec;
  const float* par;
  const float* dt0;
  const double* time0;
  unsigned int* rate;
  float* dts;
  double* times;
  float* state;
  float* dt_eff;
  int* hist_clock;
  float* hist;
  double* hist_time;
  int keep;
};

__global__ __launch_bounds__(SC_TPB) void step_rate_kernel(const RateArgs A) {
  const int c = *A.clock;
  const int p = c & 1, B = A.B;
  const int j = blockIdx.x * SC_TPB + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // the slot of the clock that comes next: nothing of this launch reads it (write-through: it shares lines with the atomics' slot)
  if (j < B) gfv_st_agent(A.rate + (p ^ 1) * B + j, 0u);
  float r = 0.f;
  int b = -1;
  if (j < A.C) {
    b = A.cbatch[j];
    const int k0 = A.crow[j], k1 = A.crow[j + 1];
    if (k1 > k0) {
      const float du = A.uvp_dim[3 * b], dv = A.uvp_dim[3 * b + 1];
      float sx = 0.f, sy = 0.f;
      for (int k = k0; k < k1; ++k) {
        const float2 uv = *reinterpret_cast<const float2*>(A.x_backup + (size_t)A.knode[k] * 12);
        sx += uv.x / du;
        sy += uv.y / dv;
      }
      const float n = (float)(k1 - k0);
      const float mx = sx / n, my = sy / n;
      float acc = 0.f;
      for (int k = k0; k < k1; ++k) {
        const float2 S = *reinterpret_cast<const float2*>(A.kS + 2 * (size_t)k);
        acc += fabsf(mx * S.x + my * S.y);
      }
      r = acc / (2.0f * A.area[j]);
      r = r > 0.f ? r : 0.f;                    // (+0 for -0, a NaN or a cell of negative area: only bits of floats >= +0 are compared)
    }
  }
  // the wavefront's maximum per graph: cbatch ascends, so a wavefront holds one graph, or a few where graphs meet
  unsigned long long live = __ballot(b >= 0);
  while (live) {
    const int first = __ffsll(live) - 1;
    const int b0 = __shfl(b, first, 64);
    const float m = gfv_wave_max_shfl(b == b0 ? r : 0.f);
    if (lane == first) atomicMax(A.rate + p * B + b0, __float_as_uint(m));
    if (b == b0) b = -1;
    live = __ballot(b >= 0);
  }
  if (!gfv_arrive_last_all_fence(A.crec + SC_COUNTER)) return;
  // ---- the controller, per graph: every maximum is in place -------------------------------------------------------------------
  const bool active = A.rec[TS_SCHEME] == GFV_TIME_SCHEME_BDF2 && c > A.rec[TS_BASE];
  const bool first_clock = c <= A.crec[SC_TBASE];
  const float courant = A.par[SC_COURANT], grow = A.par[SC_GROW], shrink = A.par[SC_SHRINK];
  const float fmin_ = A.par[SC_MIN_FACTOR], fmax_ = A.par[SC_MAX_FACTOR];
  const int slot = (int)((unsigned)c % (unsigned)A.keep);
  for (int t = threadIdx.x; t < B; t += SC_TPB) {
    const float rate = __uint_as_float(gfv_ld_agent(A.rate + p * B + t));
    const float dt_plan = A.dt[t];
    const float dt_last = first_clock ? A.dt0[t] : A.dts[p * B + t];
    const float co = rate * dt_last;
    float fac = co > 0.f ? courant / co : grow;
    fac = fminf(fmaxf(fac, shrink), grow);
    float dn = dt_last * fac;
    dn = fminf(fmaxf(dn, fmin_ * dt_plan), fmax_ * dt_plan);
    const float w = dn / dt_last;
    const float de = active ? dn / ((1.0f + 2.0f * w) / (1.0f + w)) : dn;     // (omega = 1: dn / 1.5f, csrc/timescheme.hip's bits)
    const double tm = first_clock ? A.time0[t] : A.times[(p ^ 1) * B + t] + (double)dt_last;
    A.dts[(p ^ 1) * B + t] = dn;
    A.times[p * B + t] = tm;
    A.state[SC_DT * B + t] = dn;
    A.state[SC_OMEGA * B + t] = w;
    A.state[SC_CO * B + t] = co;
    A.state[SC_RATE * B + t] = rate;
    A.dt_eff[t] = de;
    A.hist[((size_t)slot * 2 + 0) * B + t] = dn;
    A.hist[((size_t)slot * 2 + 1) * B + t] = co;
    A.hist_time[(size_t)slot * B + t] = tm;
  }
  if (threadIdx.x == 0) {
    A.hist_clock[slot] = c;
    A.crec[SC_COUNTER] = 0;                     // (reusable by the next launch)
  }
}

__global__ __launch_bounds__(SC_TPB) void step_rows_kernel(const float* __restrict__ x_backup, const int* __restrict__ batch,
                                                           const float* __restrict__ uvp_dim, int N, const int* __restrict__ clock,
                                                           const int* __restrict__ rec, const float* __restrict__ omega, float* ring,
                                                           float* __restrict__ ustar) {
  const int scheme = rec[TS_SCHEME], base = rec[TS_BASE];
  const int c = *clock;
  const bool active = scheme == GFV_TIME_SCHEME_BDF2 && c > base;
  const int i = blockIdx.x * SC_TPB + threadIdx.x;
  if (i >= N) return;
  const size_t slot = (size_t)(c & 1), n2 = 2 * (size_t)N;
  const float4 r = *reinterpret_cast<const float4*>(x_backup + (size_t)i * 12);
  const int b = batch[i];
  const float du = uvp_dim[3 * b], dv = uvp_dim[3 * b + 1];
  float su = r.x, sv = r.y;
  if (active) {
    const float w = omega[b];
    const float q = (1.0f + 2.0f * w) / (w * w);                              // (omega = 1: 3.0f, csrc/timescheme.hip's bits)
    const float2 pv = *reinterpret_cast<const float2*>(ring + (slot ^ 1) * n2 + 2 * (size_t)i);
    su = r.x + (r.x - pv.x) / q;
    sv = r.y + (r.y - pv.y) / q;
  }
  *reinterpret_cast<float2*>(ring + slot * n2 + 2 * (size_t)i) = make_float2(r.x, r.y);
  *reinterpret_cast<float2*>(ustar + 2 * (size_t)i) = make_float2(su / du, sv / dv);
}

}  // namespace

extern "C" int gfv_step_control_rate(const float* x_backup, const float* uvp_dim, const float* dt, const int32_t* crow,
                                     const int32_t* knode, const float* kS, const float* area, const int32_t* cbatch, int32_t C,
                                     int32_t B, const int32_t* clock, const int32_t* rec, int32_t* crec, const float* par,
                                     const float* dt0, const double* time0, uint32_t* rate, float* dts, double* times, float* state,
                                     float* dt_eff, int32_t* hist_clock, float* hist, double* hist_time, int32_t keep,
                                     void* stream) {
  if (!x_backup || !uvp_dim || !dt || !crow || !knode || !kS || !area || !cbatch || !clock || !rec || !crec || !par || !dt0 ||
      !time0 || !rate || !dts || !times || !state || !dt_eff || !hist_clock || !hist || !hist_time)
    return GFV_ERR_ARG;
  if (C < 1 || B < 1 || keep < 1) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(x_backup) & 15) || (reinterpret_cast<size_t>(kS) & 7)) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(time0) & 7) || (reinterpret_cast<size_t>(times) & 7) || (reinterpret_cast<size_t>(hist_time) & 7))
    return GFV_ERR_ARG;
  RateArgs A;
  A.x_backup = x_backup; A.uvp_dim = uvp_dim; A.dt = dt; A.crow = (const int*)crow; A.knode = (const int*)knode; A.kS = kS;
  A.area = area; A.cbatch = (const int*)cbatch; A.C = C; A.B = B; A.clock = (const int*)clock; A.rec = (const int*)rec;
  A.crec = (int*)crec; A.par = par; A.dt0 = dt0; A.time0 = time0; A.rate = (unsigned int*)rate; A.dts = dts; A.times = times;
  A.state = state; A.dt_eff = dt_eff; A.hist_clock = (int*)hist_clock; A.hist = hist; A.hist_time = hist_time; A.keep = keep;
  // per cell: crow, cbatch, area and about four incidences of (knode 4 B, the row's velocity 8 B, kS 8 B)
  GfvProfScope ps_(GFV_K_MISC, 0, (12.0 + 4.0 * 20.0) * C, stream);
  const int n = C > B ? C : B;
  GFV_LAUNCH(step_rate_kernel, dim3((n + SC_TPB - 1) / SC_TPB), dim3(SC_TPB), 0, (hipStream_t)stream, A);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_step_control_rows(const float* x_backup, const int32_t* batch, const float* uvp_dim, int32_t N, int32_t B,
                                     const int32_t* clock, const int32_t* rec, const float* state, float* ring, float* ustar,
                                     void* stream) {
  if (!x_backup || !batch || !uvp_dim || !clock || !rec || !state || !ring || !ustar) return GFV_ERR_ARG;
  if (N < 1 || B < 1) return GFV_ERR_ARG;
  if (reinterpret_cast<size_t>(x_backup) & 15) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(ring) & 7) || (reinterpret_cast<size_t>(ustar) & 7)) return GFV_ERR_ARG;
  // as gfv_time_scheme_update's active launch, and omega[b]
  GfvProfScope ps_(GFV_K_MISC, 0, (16.0 + 4.0 + 4.0 + 8.0 + 8.0 + 8.0) * N, stream);
  GFV_LAUNCH(step_rows_kernel, dim3((N + SC_TPB - 1) / SC_TPB), dim3(SC_TPB), 0, (hipStream_t)stream, x_backup, (const int*)batch,
             uvp_dim, (int)N, (const int*)clock, (const int*)rec, state + (size_t)SC_OMEGA * B, ring, ustar);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
