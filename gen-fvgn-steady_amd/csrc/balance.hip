// Loss balancing on the device (gfv/balance.py; the constants of the reference's utils/get_param.py:59-61): ONE wave
// per training step, behind the step's optimiser launches, that observes the step's residual terms losses[B, 4], advances the
// record rec[GFV_BALANCE_RECORD] (include/gfv.h: the layout and the rule, restated in tests/balance_ref.py) and, on a publish,
// writes the three weights where the loss launch, its gradient and the march read them - hyper[5..7].
//
// Every lane reads the record, the hold word and the rows b = lane, lane + 64, ... of losses; the 64 partial sums are folded by a
// fixed butterfly (every lane ends with the same bits), so the statistic depends on B alone; all lanes compute the same update in
// double; then lane 0 writes.  One wave: the loads stand in front of the stores in program order, no atomics, no arrival counter.
// The unit is built with -ffp-contract=off like the rest of the library: every product and sum below is one IEEE double
// operation, as in the Python statements they restate; only exp() may differ from the host's libm in its last bits.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"

namespace {

// 32-bit words of the record
enum { BW_KIND = 0, BW_WARMUP = 1, BW_EVERY = 2, BW_N = 3, BW_N_APPLIED = 4, BW_N_UPDATES = 5, BW_N_SKIPPED = 6 };
// doubles of the record
enum { BD_DECAY = 4, BD_FLOOR = 5, BD_ALPHA = 6, BD_TAU = 7, BD_G = 8, BD_W0 = 11, BD_POWER = 14, BD_M = 15, BD_S = 18, BD_SREF = 21,
       BD_LAM = 24, BD_W = 27 };
static_assert(2 * BD_DECAY > BW_N_SKIPPED + 1 && BD_W + 3 <= GFV_BALANCE_RECORD, "words and doubles do not overlap and end inside");
static_assert(GFV_BALANCE_LANES == 64, "one wave of 64 lanes holds the partial sums");

static __device__ __forceinline__ double max2(double a, double b) { return a > b ? a : b; }   // Python's max(a, b)

__global__ __launch_bounds__(GFV_BALANCE_LANES) void loss_balance_kernel(const float* __restrict__ losses, const int B, double* rec,
                                                                         float* hyper, const int* hold) {
  const int lane = threadIdx.x;
  int* w = reinterpret_cast<int*>(rec);
  double* d = rec;
  // ---- the record, the hold word and the terms as the launch finds them -----------------------------------------------------------
  const int kind = w[BW_KIND], warmup = w[BW_WARMUP], every = w[BW_EVERY] < 1 ? 1 : w[BW_EVERY];
  int n = w[BW_N], n_applied = w[BW_N_APPLIED], n_updates = w[BW_N_UPDATES];
  const int n_skipped = w[BW_N_SKIPPED];
  const double decay = d[BD_DECAY], floor_ = d[BD_FLOOR], alpha = d[BD_ALPHA], tau = d[BD_TAU];
  double power = d[BD_POWER];
  double g[3], w0[3], m[3], sref[3], lam[3], wt[3], s[3], mh[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    g[k] = d[BD_G + k];
    w0[k] = d[BD_W0 + k];
    m[k] = d[BD_M + k];
    sref[k] = d[BD_SREF + k];
    lam[k] = d[BD_LAM + k];
    wt[k] = d[BD_W + k];
  }
  const bool applied = hold ? *hold != 0 : true;
  double p[3] = {0.0, 0.0, 0.0};
  for (int b = lane; b < B; b += GFV_BALANCE_LANES) {
    const float* r = losses + 4 * (size_t)b;
    p[0] = p[0] + (double)r[0];
    p[1] = p[1] + ((double)r[1] + (double)r[2]);
    p[2] = p[2] + (double)r[3];
  }
#pragma unroll
  for (int h = GFV_BALANCE_LANES / 2; h >= 1; h >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = p[k] + __shfl_xor(p[k], h, GFV_BALANCE_LANES);   // (p_j + p_(j^h): the same bits in both lanes)
  }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s[k] = p[k] / (double)B;
    ok = ok && s[k] >= 0.0 && s[k] <= 1.7976931348623157e308;        // (a NaN compares false)
  }
  if (!ok) {
    if (lane == 0) w[BW_N_SKIPPED] = n_skipped + 1;
    return;
  }

  // ---- the observation ----------------------------------------------------------------------------------------------------------------
  n += 1;
  power = power * decay;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    m[k] = decay * m[k] + (1.0 - decay) * s[k];
    mh[k] = m[k] / (1.0 - power);
    if (n == 1) sref[k] = mh[k];
  }
  if (applied) n_applied += 1;
  const bool publish = applied && n > warmup && n_applied % every == 0;
  if (publish) {
    if (kind == GFV_BALANCE_PROGRESS) {
      double z[3], e[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) z[k] = (mh[k] / max2(sref[k], floor_)) / tau;
      const double zm = max2(max2(z[0], z[1]), z[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) e[k] = exp(z[k] - zm);
      const double E = (e[0] + e[1]) + e[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        lam[k] = alpha * lam[k] + (1.0 - alpha) * (3.0 * (e[k] / E));
        wt[k] = w0[k] * lam[k];
        sref[k] = mh[k];
      }
    } else {
      const double R0 = (w0[0] * mh[0] + w0[1] * mh[1]) + w0[2] * mh[2], G = (g[0] + g[1]) + g[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) wt[k] = ((g[k] / G) * R0) / max2(mh[k], floor_);
    }
    n_updates += 1;
  }

  // ---- outputs: plain vector stores -------------------------------------------------------------------------------------------------
  if (lane == 0) {
    w[BW_N] = n;
    w[BW_N_APPLIED] = n_applied;
    w[BW_N_UPDATES] = n_updates;
    d[BD_POWER] = power;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      d[BD_M + k] = m[k];
      d[BD_S + k] = s[k];
      d[BD_SREF + k] = sref[k];
      d[BD_LAM + k] = lam[k];
      d[BD_W + k] = wt[k];
      if (publish) hyper[5 + k] = (float)wt[k];
    }
  }
}

}  // namespace

extern "C" int gfv_loss_balance(const float* losses, int32_t B, double* rec, float* hyper, const int32_t* hold_or_null, void* stream) {
  if (!losses || !rec || !hyper || B < 1) return GFV_ERR_ARG;
  if (reinterpret_cast<size_t>(rec) & 7) return GFV_ERR_ARG;
  GfvProfScope ps_(GFV_K_MISC, 0, 16.0 * B + 16.0 * GFV_BALANCE_RECORD + 12.0, stream);
  GFV_LAUNCH(loss_balance_kernel, dim3(1), dim3(GFV_BALANCE_LANES), 0, (hipStream_t)stream, losses, (int)B, rec, hyper,
             reinterpret_cast<const int*>(hold_or_null));
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
