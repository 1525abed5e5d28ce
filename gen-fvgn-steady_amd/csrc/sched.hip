// Learning-rate schedules on the device (gfv/schedule.py; the reference's utils/scheduler.py and torch's
// ReduceLROnPlateau): ONE wave that recomputes the rate from the record sched[GFV_SCHED_RECORD] (include/gfv.h) and writes it where
// the Adam launches read it - hyper[0] and the lr word of every group row.
//
// Every lane reads the record, the counter and the metric; all of them compute the same rate in double; then lane 0 writes the
// record and hyper[0], lane k < n_groups the lr word of group row k.  One wave: the loads stand in front of the stores in
// program order, no atomics, no arrival counter.  The unit is built with -ffp-contract=off like the rest of the library: every
// product and sum below is one IEEE double operation, as in the Python statements they restate (tests/sched_ref.py); only
// pow() may differ from the host's libm in its last bits.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"

namespace {

// 32-bit words of the record
enum { SW_KIND = 0, SW_EPOCH = 1, SW_N_MILESTONES = 2, SW_NUM_BAD = 3, SW_COOLDOWN_LEFT = 4, SW_PATIENCE = 5, SW_COOLDOWN = 6,
       SW_WARMUP = 7, SW_STEP_MILESTONE = 8, SW_EXP_MILESTONE = 9, SW_TOTAL_EPOCH = 10, SW_FOLLOW_CAP = 11, SW_MILESTONES = 40 };
// doubles of the record
enum { SD_LR = 8, SD_BASE_LR = 9, SD_MIN_LR = 10, SD_GAMMA = 11, SD_EXPGAMMA = 12, SD_DECAY_STEPS = 13, SD_START_LR = 14,
       SD_BEST = 15, SD_FACTOR = 16, SD_THRESHOLD = 17, SD_EPS = 18, SD_MULTIPLIER = 19 };
static_assert(SW_MILESTONES + GFV_SCHED_MAX_MILESTONES <= 2 * GFV_SCHED_RECORD, "the milestones end inside the record");
static_assert(2 * SD_LR >= 16 && SW_MILESTONES >= 2 * (SD_MULTIPLIER + 1), "words, doubles and milestones do not overlap");

struct SchedArgs {
  double* rec;            // [GFV_SCHED_RECORD]
  float* hyper;           // [8]: word 0 is written
  float* group_table;     // the table of gfv_adam_step_groups_dev or NULL: word 0 of rows 1 .. n_groups is written
  const double* scales;   // [n_groups]
  const double* table;    // [table_len] or NULL
  const float* metric;    // one float or NULL
  const int* counter;     // one int32 or NULL
  int mode, n_groups, table_len;
};

static __device__ __forceinline__ double clamp0(double v) { return v > 0.0 ? v : 0.0; }   // Python's max(v, 0)

__global__ __launch_bounds__(64) void lr_schedule_kernel(const SchedArgs A) {
  const int lane = threadIdx.x;
  int* w = reinterpret_cast<int*>(A.rec);
  double* d = A.rec;
  // ---- the record as the launch finds it ---------------------------------------------------------------------------------------
  const int kind = w[SW_KIND];
  int epoch = w[SW_EPOCH];
  double lr = d[SD_LR], best = d[SD_BEST];
  int num_bad = w[SW_NUM_BAD], cool = w[SW_COOLDOWN_LEFT];
  const double base = d[SD_BASE_LR], min_lr = d[SD_MIN_LR], gamma = d[SD_GAMMA], expgamma = d[SD_EXPGAMMA];
  const double decay = d[SD_DECAY_STEPS];
  const int total = w[SW_TOTAL_EPOCH];

  if (A.mode == GFV_SCHED_TICK) {
    if (epoch < 0x7fffffff) epoch += 1;
  } else if (A.mode == GFV_SCHED_FOLLOW && kind != GFV_SCHED_PLATEAU) {
    int c = *A.counter;
    const int cap = w[SW_FOLLOW_CAP];
    if (cap >= 0 && c > cap) c = cap;
    if (c != epoch) epoch = c;
  }

  switch (kind) {
    case GFV_SCHED_STEPEXP: {
      const int m1 = w[SW_STEP_MILESTONE], m2 = w[SW_EXP_MILESTONE];
      const double start = d[SD_START_LR];
      if (epoch < m1) lr = start;
      else if (epoch < m2) lr = start * gamma;
      else lr = min_lr + clamp0(base * gamma - min_lr) * pow(expgamma, (double)(epoch - m2) / decay);
      break;
    }
    case GFV_SCHED_EXP:
      lr = min_lr + clamp0(base - min_lr) * pow(gamma, (double)epoch / decay);
      break;
    case GFV_SCHED_GRADUAL: {
      const int n_ms = min(max(w[SW_N_MILESTONES], 0), GFV_SCHED_MAX_MILESTONES), upto = min(epoch, total);
      int hit = 0;
      for (int i = 0; i < n_ms; ++i) hit += w[SW_MILESTONES + i] <= upto ? 1 : 0;
      const double stepped = base * pow(gamma, (double)hit);
      lr = epoch > total ? min_lr + clamp0(stepped - min_lr) * pow(expgamma, (double)(epoch - total) / decay) : stepped;
      break;
    }
    case GFV_SCHED_TABLE:
      if (A.table && A.table_len > 0) lr = A.table[min(max(epoch, 0), A.table_len - 1)];
      break;
    case GFV_SCHED_PLATEAU: {
      const int warm = w[SW_WARMUP];
      if (warm > 0 && epoch <= warm) {
        const double mult = d[SD_MULTIPLIER];
        lr = mult == 1.0 ? base * ((double)epoch / (double)warm) : base * ((mult - 1.0) * (double)epoch / (double)warm + 1.0);
      } else if (A.mode == GFV_SCHED_TICK && A.metric) {
        const double a = (double)*A.metric;
        if (a < best * (1.0 - d[SD_THRESHOLD])) {          // (a NaN compares false: a bad epoch)
          best = a;
          num_bad = 0;
        } else {
          num_bad += 1;
        }
        if (cool > 0) {
          cool -= 1;
          num_bad = 0;
        }
        if (num_bad > w[SW_PATIENCE]) {
          const double scaled = lr * d[SD_FACTOR], lower = min_lr > scaled ? min_lr : scaled;
          if (lr - lower > d[SD_EPS]) lr = lower;
          cool = w[SW_COOLDOWN];
          num_bad = 0;
        }
      }
      break;
    }
    default:
      break;                                               // (an unknown kind: the rate of the record, written out)
  }

  // ---- outputs: plain vector stores ----------------------------------------------------------------------------------------------
  if (A.group_table && lane < A.n_groups) A.group_table[8 * (1 + lane)] = (float)(lr * A.scales[lane]);
  if (lane == 0) {
    A.hyper[0] = (float)lr;
    w[SW_EPOCH] = epoch;
    w[SW_NUM_BAD] = num_bad;
    w[SW_COOLDOWN_LEFT] = cool;
    d[SD_LR] = lr;
    d[SD_BEST] = best;
  }
}

}  // namespace

extern "C" int gfv_lr_schedule(double* rec, int32_t mode, float* hyper, float* group_table, const double* scales, int32_t n_groups,
                               const double* table, int32_t table_len, const float* metric, const int32_t* counter, void* stream) {
  if (!rec || !hyper) return GFV_ERR_ARG;
  if (mode != GFV_SCHED_EVAL && mode != GFV_SCHED_TICK && mode != GFV_SCHED_FOLLOW) return GFV_ERR_ARG;
  if (mode == GFV_SCHED_FOLLOW && !counter) return GFV_ERR_ARG;
  if (n_groups < 0 || n_groups > GFV_MAX_PARAM_GROUPS) return GFV_ERR_ARG;
  if (group_table && n_groups > 0 && !scales) return GFV_ERR_ARG;
  if (table_len < 0 || (table_len > 0 && !table)) return GFV_ERR_ARG;
  if (reinterpret_cast<size_t>(rec) & 7) return GFV_ERR_ARG;
  GfvProfScope ps_(GFV_K_MISC, 0, 8.0 * GFV_SCHED_RECORD + 4.0 + (group_table ? 12.0 * n_groups : 0.0), stream);
  const SchedArgs a{rec, hyper, group_table, scales, table, metric, counter, mode, group_table ? n_groups : 0, table_len};
  GFV_LAUNCH(lr_schedule_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
