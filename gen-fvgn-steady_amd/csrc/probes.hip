// Probes (gfv/probes.py): the value and the gradient of the field at fixed points of the mesh, per sampled field, kept
// on the device.  ONE launch behind the launch that advances the field (gfv_rollout_advance, gfv_march_advance); it follows the clock
// word that launch writes and reads it, and the record rec[8] (the window: include/gfv.h GFV_WINDOW_RECORD, gfv_window.h), as it
// finds them:
//   c = *clock;  take = gfv_window_take(rec, c)
// A probe's value is a fixed linear functional of the node values: the point-in-cell search, the WLSQ systems of the cell's vertices
// and the merge of their stencils are done once, in float64, when the object is attached (gfv/probes.py build_tables), and what is
// left for a step is a short sparse dot product per probe:
//   one wave per probe p (four per workgroup); lane l takes the entries pw_ptr[p] + l, + l + 64, ... < pw_ptr[p + 1] in ascending
//   order: phi_c = x_backup[pw_node[e], c] / uvp_dim[3 batch[pw_node[e]] + c] (one fp32 division, then double) and
//   s[3 c + j] += pw_w[e, j] * phi_c (each product and each sum one double operation, from +0.0); the 64 lane sums fold by
//   gfv_wave_sum; lanes 0 .. 8 store the nine doubles into the ring's row n % keep.
// No workgroup reads what another wrote, so the arrival is the no-data form of gfv_reduce.h (as csrc/fieldstats.hip): thread 0 of
// the workgroup that arrives last writes the row's clock and the record.  take false: no history word moves.  No floating-point
// atomics, an order that does not depend on the grid: the same inputs give the same bits.  The rule in full: include/gfv.h.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"
#include "gfv_window.h"

namespace {

constexpr int PR_TPB = 256;
constexpr int PR_WAVES = PR_TPB / 64;
static_assert(GFV_PROBE_SUMS == 9, "include/gfv.h");

__global__ __launch_bounds__(PR_TPB) void probe_sample_kernel(const float* __restrict__ x_backup, const float* __restrict__ uvp_dim,
                                                              const int* __restrict__ batch, const int* __restrict__ pw_ptr,
                                                              const int* __restrict__ pw_node, const double* __restrict__ pw_w,
                                                              int P, const int* clock, int* rec, double* __restrict__ hist,
                                                              int* __restrict__ hist_clock, int keep) {
  // ---- the record and the clock as the launch finds them: read by every thread before the arrival below ----------------------
  const int c = *clock;
  const int last = rec[GFV_WIN_LAST], n = rec[GFV_WIN_N];
  const bool take = gfv_window_take(rec, c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * PR_WAVES + wave;
  const size_t slot = (size_t)((unsigned)n % (unsigned)keep);
  if (take && p < P) {
    double s[GFV_PROBE_SUMS];
#pragma unroll
    for (int q = 0; q < GFV_PROBE_SUMS; ++q) s[q] = 0.0;
    const int beg = pw_ptr[p], end = pw_ptr[p + 1];
    for (int e = beg + lane; e < end; e += 64) {
      const int i = pw_node[e];
      const float4 r = *reinterpret_cast<const float4*>(x_backup + (size_t)i * 12);
      const float* dim = uvp_dim + 3 * (size_t)batch[i];
      const double* w = pw_w + (size_t)e * 3;
      const double w0 = w[0], w1 = w[1], w2 = w[2];
      const double phi[3] = {(double)(r.x / dim[0]), (double)(r.y / dim[1]), (double)(r.z / dim[2])};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        s[3 * ch] += w0 * phi[ch];
        s[3 * ch + 1] += w1 * phi[ch];
        s[3 * ch + 2] += w2 * phi[ch];
      }
    }
#pragma unroll
    for (int q = 0; q < GFV_PROBE_SUMS; ++q) s[q] = gfv_wave_sum(s[q]);
    if (lane < GFV_PROBE_SUMS) {
      double v = s[0];
#pragma unroll
      for (int q = 1; q < GFV_PROBE_SUMS; ++q) v = lane == q ? s[q] : v;
      hist[(slot * (size_t)P + (size_t)p) * GFV_PROBE_SUMS + lane] = v;
    }
  }
  if (!gfv_arrive_last_nodata(rec + GFV_WIN_COUNTER)) return;         // (true on thread 0 of the last workgroup only)
  if (take) hist_clock[slot] = c;
  gfv_window_commit(rec, c, last, n, take);
}

}  // namespace

extern "C" int gfv_probe_sample(const float* x_backup, const float* uvp_dim, const int32_t* batch, const int32_t* pw_ptr,
                                const int32_t* pw_node, const double* pw_w, int32_t P, const int32_t* clock, int32_t* rec,
                                double* hist, int32_t* hist_clock, int32_t keep, void* stream) {
  if (!x_backup || !uvp_dim || !batch || !pw_ptr || !pw_node || !pw_w || !clock || !rec || !hist || !hist_clock) return GFV_ERR_ARG;
  if (P < 1 || keep < 1) return GFV_ERR_ARG;
  if (reinterpret_cast<size_t>(x_backup) & 15) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(pw_w) & 7) || (reinterpret_cast<size_t>(hist) & 7)) return GFV_ERR_ARG;
  // a launch that samples (the host cannot know; nor the tables' length: about thirty entries per probe), per entry the index, the
  // graph, 16 B of the row and three doubles; per probe nine doubles out
  GfvProfScope ps_(GFV_K_MISC, 0, (30.0 * (4.0 + 4.0 + 16.0 + 24.0) + 8.0 + 72.0) * P, stream);
  GFV_LAUNCH(probe_sample_kernel, dim3((P + PR_WAVES - 1) / PR_WAVES), dim3(PR_TPB), 0, (hipStream_t)stream, x_backup, uvp_dim,
             (const int*)batch, (const int*)pw_ptr, (const int*)pw_node, pw_w, (int)P, (const int*)clock, (int*)rec, hist,
             (int*)hist_clock, (int)keep);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
