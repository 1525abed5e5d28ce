// Time differencing of a march (gfv/timescheme.py): the history a second-order backward difference (BDF2) needs,
// kept on the device.  ONE launch behind the launch that advances the field (gfv_march_advance, or TrainStep.advance_time()'s two
// copies); it follows a clock word that counts the fields written, the idea of gfv_field_stats_update.
//
// With the record rec[4] (include/gfv.h) and *clock AS THE LAUNCH FINDS THEM - both are read-only here, the host writes them:
//   c = *clock (x_backup holds field c);  active = scheme == 2 && c > base
//   row i of graph b = batch[i], channel k in {0, 1}:
//     cur = x_backup[i, k];  ring[c & 1][i][k] = cur
//     active:    prev = ring[(c & 1) ^ 1][i][k];  s = cur + (cur - prev) / 3.0f;  ustar[i][k] = s / uvp_dim[3 b + k]
//     otherwise: ustar[i][k] = cur / uvp_dim[3 b + k]      (prep_apply's uv_old, csrc/misc.hip: the same operation, the same bits)
//   thread t < B:  dt_eff[t] = active ? dt[t] / 1.5f : dt[t]
// One thread per row; no atomics, no cross-row sum, no arrival: the launch reads only the ring slot it does not write, so no word
// it writes is read by another workgroup of it, and a launch that finds the same clock writes the same bits again.  A launch that
// finds the clock advanced by one overwrites field c - 2 with field c and reads field c - 1: that is the whole rotation.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"

namespace {

constexpr int TS_TPB = 256;
enum { TS_SCHEME = 0, TS_BASE = 1 };
static_assert(GFV_TIME_SCHEME_RECORD == 4 && GFV_TIME_SCHEME_BDF1 == 1 && GFV_TIME_SCHEME_BDF2 == 2, "include/gfv.h");

__global__ __launch_bounds__(TS_TPB) void time_scheme_kernel(const float* __restrict__ x_backup, const int* __restrict__ batch,
                                                             const float* __restrict__ uvp_dim, const float* __restrict__ dt, int N,
                                                             int B, const int* __restrict__ clock, const int* __restrict__ rec,
                                                             float* ring, float* __restrict__ ustar, float* __restrict__ dt_eff) {
  const int scheme = rec[TS_SCHEME], base = rec[TS_BASE];
  const int c = *clock;
  const bool active = scheme == GFV_TIME_SCHEME_BDF2 && c > base;
  const int i = blockIdx.x * TS_TPB + threadIdx.x;
  if (i < B) dt_eff[i] = active ? dt[i] / 1.5f : dt[i];
  if (i >= N) return;
  const size_t slot = (size_t)(c & 1), n2 = 2 * (size_t)N;
  const float4 r = *reinterpret_cast<const float4*>(x_backup + (size_t)i * 12);
  const int b = batch[i];
  const float du = uvp_dim[3 * b], dv = uvp_dim[3 * b + 1];
  float su = r.x, sv = r.y;
  if (active) {
    const float2 p = *reinterpret_cast<const float2*>(ring + (slot ^ 1) * n2 + 2 * (size_t)i);
    su = r.x + (r.x - p.x) / 3.0f;
    sv = r.y + (r.y - p.y) / 3.0f;
  }
  *reinterpret_cast<float2*>(ring + slot * n2 + 2 * (size_t)i) = make_float2(r.x, r.y);
  *reinterpret_cast<float2*>(ustar + 2 * (size_t)i) = make_float2(su / du, sv / dv);
}

}  // namespace

extern "C" int gfv_time_scheme_update(const float* x_backup, const int32_t* batch, const float* uvp_dim, const float* dt, int32_t N,
                                      int32_t B, const int32_t* clock, const int32_t* rec, float* ring, float* ustar,
                                      float* dt_eff, void* stream) {
  if (!x_backup || !batch || !uvp_dim || !dt || !clock || !rec || !ring || !ustar || !dt_eff) return GFV_ERR_ARG;
  if (N < 1 || B < 1) return GFV_ERR_ARG;
  if (reinterpret_cast<size_t>(x_backup) & 15) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(ring) & 7) || (reinterpret_cast<size_t>(ustar) & 7)) return GFV_ERR_ARG;
  // an active launch (the host cannot know): 16 B of the row and the graph index read, one ring slot read, the other written, ustar
  // written
  GfvProfScope ps_(GFV_K_MISC, 0, (16.0 + 4.0 + 8.0 + 8.0 + 8.0) * N, stream);
  const int n = N > B ? N : B;
  GFV_LAUNCH(time_scheme_kernel, dim3((n + TS_TPB - 1) / TS_TPB), dim3(TS_TPB), 0, (hipStream_t)stream, x_backup, (const int*)batch,
             uvp_dim, dt, (int)N, (int)B, (const int*)clock, (const int*)rec, ring, ustar, dt_eff);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
