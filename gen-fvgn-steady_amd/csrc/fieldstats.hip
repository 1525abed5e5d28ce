// Field statistics (gfv/fieldstats.py): the time mean, the variances, the Reynolds shear stress u'v' and the extremes
// of the node field over a window of a run, kept on the device.  ONE launch behind the launch that advances the field
// (gfv_rollout_advance, gfv_march_advance); it follows a clock word that launch writes, the idea of GFV_SCHED_FOLLOW.
//
// With the record rec[8] AS THE LAUNCH FINDS IT (the window: include/gfv.h GFV_WINDOW_RECORD, gfv_window.h) - every workgroup reads
// it and *clock before anything is written; the workgroup that arrives last writes it (no-data arrival of gfv_reduce.h: it needs
// nothing another workgroup wrote):
//   c = *clock;  take = gfv_window_take(rec, c)
//   take false:  no row and no state element is read or written
//   take true:   per row, x = x_backup[i, 0:3]
//     n == 0:    K = min = max = x; the seven sums = +0.0 (a reset needs no memset)
//     n > 0:     d = (double)x - (double)K; S1 += d; S2uu += du * du; S2vv += dv * dv; S2pp += dp * dp; S2uv += du * dv (each
//                product and each sum one double operation); min = fminf(min, x); max = fmaxf(max, x)
//   last arriver: gfv_window_commit
// One thread per row, no cross-row sum, no floating-point atomics: the same inputs give the same bits whatever the grid.  The state
// is planar (sums [7, N], aux [9, N]): consecutive lanes touch consecutive addresses of every plane.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"
#include "gfv_window.h"

namespace {

constexpr int FS_TPB = 256;
static_assert(GFV_FIELD_STATS_SUMS == 7 && GFV_FIELD_STATS_AUX == 9, "include/gfv.h");

__global__ __launch_bounds__(FS_TPB) void field_stats_kernel(const float* __restrict__ x_backup, int N, const int* clock, int* rec,
                                                             double* __restrict__ sums, float* __restrict__ aux) {
  // ---- the record and the clock as the launch finds them: read by every thread before the arrival below -----------------------
  const int c = *clock;
  const int last = rec[GFV_WIN_LAST], n = rec[GFV_WIN_N];
  const bool take = gfv_window_take(rec, c);
  const int i = blockIdx.x * FS_TPB + threadIdx.x;
  if (take && i < N) {
    const size_t n_ = (size_t)N;
    const float4 r = *reinterpret_cast<const float4*>(x_backup + (size_t)i * 12);
    const float x[3] = {r.x, r.y, r.z};
    float* k_ = aux + i;                   // planes 0..2: K;  3..5: min;  6..8: max
    double* s = sums + i;                  // planes 0..2: S1; 3..5: S2uu, S2vv, S2pp; 6: S2uv
    if (n == 0) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        k_[q * n_] = x[q];
        k_[(3 + q) * n_] = x[q];
        k_[(6 + q) * n_] = x[q];
      }
#pragma unroll
      for (int q = 0; q < GFV_FIELD_STATS_SUMS; ++q) s[q * n_] = 0.0;
    } else {
      double d[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        d[q] = (double)x[q] - (double)k_[q * n_];
        s[q * n_] = s[q * n_] + d[q];
        const double sq = d[q] * d[q];
        s[(3 + q) * n_] = s[(3 + q) * n_] + sq;
        k_[(3 + q) * n_] = fminf(k_[(3 + q) * n_], x[q]);
        k_[(6 + q) * n_] = fmaxf(k_[(6 + q) * n_], x[q]);
      }
      const double uv = d[0] * d[1];
      s[6 * n_] = s[6 * n_] + uv;
    }
  }
  if (!gfv_arrive_last_nodata(rec + GFV_WIN_COUNTER)) return;         // (true on thread 0 of the last workgroup only)
  gfv_window_commit(rec, c, last, n, take);
}

}  // namespace

extern "C" int gfv_field_stats_update(const float* x_backup, int32_t N, const int32_t* clock, int32_t* rec, double* sums,
                                      float* aux, void* stream) {
  if (!x_backup || !clock || !rec || !sums || !aux) return GFV_ERR_ARG;
  if (N < 1) return GFV_ERR_ARG;
  if (reinterpret_cast<size_t>(x_backup) & 15) return GFV_ERR_ARG;
  // a launch that samples (the host cannot know): 16 B of the row read, the seven sums read and written, min / max read and
  // written, the shift read
  GfvProfScope ps_(GFV_K_MISC, 0, (16.0 + 112.0 + 48.0 + 12.0) * N, stream);
  GFV_LAUNCH(field_stats_kernel, dim3((N + FS_TPB - 1) / FS_TPB), dim3(FS_TPB), 0, (hipStream_t)stream, x_backup, (int)N,
             (const int*)clock, (int*)rec, sums, aux);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
