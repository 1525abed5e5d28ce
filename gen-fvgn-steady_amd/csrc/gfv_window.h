// The sampling window of the launches that sample a run from behind its advance launch (field statistics, wall forces, probes): the
// record's words, the decision and the last arriver's commit, once.  The record and the rule: include/gfv.h, GFV_WINDOW_RECORD.
// Every thread reads *clock and the record AS THE LAUNCH FINDS THEM (gfv_window_take; rec[GFV_WIN_LAST], rec[GFV_WIN_N]) BEFORE its
// arrival on rec + GFV_WIN_COUNTER - in whichever form of gfv_reduce.h the kernel needs; the one thread that is last commits.
// Device inline functions only.
#pragma once
#include "../../include/gfv.h"

enum { GFV_WIN_START, GFV_WIN_STRIDE, GFV_WIN_STOP, GFV_WIN_LAST, GFV_WIN_N, GFV_WIN_COUNTER, GFV_WIN_ENABLED };   // words [0] .. [6]
static_assert(GFV_WINDOW_RECORD == 8 && GFV_FIELD_STATS_RECORD == 8 && GFV_WALL_FORCE_RECORD == 8 &&
              GFV_PROBE_RECORD == 8, "include/gfv.h");

// is the field of clock c sampled?  (a stride < 1 is read as 1; a negative stop is no end)
static __device__ __forceinline__ bool gfv_window_take(const int* rec, int c) {
  const int start = rec[GFV_WIN_START], stride = max(rec[GFV_WIN_STRIDE], 1), stop = rec[GFV_WIN_STOP];
  const int last = rec[GFV_WIN_LAST], enabled = rec[GFV_WIN_ENABLED];
  return enabled != 0 && c != last && c >= start && (stop < 0 || c < stop) &&
         ((long long)c - (long long)start) % (long long)stride == 0;
}

// the last arriver's three stores (last, n: as the launch found them): the clock followed, a sample counted, the counter reusable
static __device__ __forceinline__ void gfv_window_commit(int* rec, int c, int last, int n, bool take) {
  if (c != last) rec[GFV_WIN_LAST] = c;
  if (take) rec[GFV_WIN_N] = n + 1;
  rec[GFV_WIN_COUNTER] = 0;
}
