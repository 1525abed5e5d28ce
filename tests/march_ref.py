"""The rule of the march launch (include/gfv.h gfv_march_advance) restated in numpy.

Written from the header's paragraph, not from the kernel: tests/test_march_gpu.py compares the kernel with it launch by launch.
fp32 where the kernel's arithmetic is fp32 (the weighted residual, the product tol * r0, the field differences); float64 sums in
the order of tests/chunk_sums_ref.py for the two norms of a history row.  Nothing here touches a GPU.
"""
import numpy as np

import chunk_sums_ref as CS

MAX_INNER, MIN_INNER, INNER, APPLY, TOL, ABS_TOL, LEVEL, COUNTER, TARGET, DONE, SEEN, HELD, KEEP = range(13)
RECORD, HEAD, GRAPH, CONVERGED, CAPPED = 16, 8, 8, 1, 2

f32 = np.float32


def residual(losses, w_cont, w_mom, w_press):
    """losses [B, 4] = (cont, mom_x, mom_y, press) -> r [B] in fp32: every product and sum rounded, added left to right."""
    l = np.asarray(losses, dtype=f32)
    wc, wm, wp = f32(w_cont), f32(w_mom), f32(w_press)
    with np.errstate(all="ignore"):
        r = ((wp * l[:, 3] + wc * l[:, 0]) + wm * l[:, 1]) + wm * l[:, 2]
    assert r.dtype == f32
    return r


def converged(r, r0, tol, abs_tol):
    """[B] bool: (tol >= 0 and r <= tol * r0) or (abs_tol >= 0 and r <= abs_tol); the product one fp32 rounding, NaN -> False."""
    tol, abs_tol = f32(tol), f32(abs_tol)
    with np.errstate(all="ignore"):
        bound = tol * np.asarray(r0, dtype=f32)
        assert bound.dtype == f32
        return ((tol >= 0) & (r <= bound)) | ((abs_tol >= 0) & (r <= abs_tol))


def decide(inner, conv_all, min_inner, max_inner):
    """-> (k, converged flag, capped flag); the launch latches when either flag is set."""
    k = inner + 1
    return k, bool(conv_all) and k >= min_inner, k >= max_inner


class MarchRef:
    """The buffers a sequence of march launches works on, and `launch()`: one launch applied to them."""

    def __init__(self, x_backup, chunk_beg, chunk_end, gchunk_ptr, weights, max_inner, min_inner, tol, abs_tol, target,
                 max_levels, keep):
        self.x_backup = np.array(x_backup, dtype=f32)
        self.x = self.x_backup.copy()
        self.N = self.x_backup.shape[0]
        self.cb, self.ce, self.gcp = (np.asarray(a, dtype=np.int64) for a in (chunk_beg, chunk_end, gchunk_ptr))
        self.B = len(self.gcp) - 1
        self.w = tuple(weights)
        self.rec = np.zeros(RECORD, dtype=np.int32)
        self.rec[[MAX_INNER, MIN_INNER, TARGET, KEEP]] = (max_inner, min_inner, target, keep)
        self.rec[[TOL, ABS_TOL]] = np.array([tol, abs_tol], dtype=f32).view(np.int32)
        self.r0 = np.zeros(self.B, dtype=f32)
        self.max_levels = max_levels
        self.hist = np.zeros((max_levels, HEAD + GRAPH * self.B), dtype=np.int32)
        self.snap = np.zeros((keep, self.N, 3), dtype=f32)

    def launch(self, uvp, losses):
        rec = self.rec
        if rec[DONE]:
            rec[APPLY] = 0
            rec[HELD] += 1
            return "held"
        uvp, losses = np.asarray(uvp, dtype=f32), np.asarray(losses, dtype=f32)
        inner, level = int(rec[INNER]), int(rec[LEVEL])
        tol, abs_tol = rec[[TOL, ABS_TOL]].view(f32)
        r = residual(losses, *self.w)
        r0 = r.copy() if inner == 0 else self.r0.copy()
        k, conv, cap = decide(inner, converged(r, r0, tol, abs_tol).all(), int(rec[MIN_INNER]), int(rec[MAX_INNER]))
        rec[APPLY] = 1
        rec[SEEN] += 1
        self.r0 = r0
        if not (conv or cap):
            rec[INNER] = k
            return "open"
        if level < self.max_levels:
            terms = CS.diff_norm_terms(uvp, self.x_backup[:, 0:3])
            sums = CS.graph_sums(CS.chunk_sums(terms, self.cb, self.ce, self.N), self.gcp)
            row = self.hist[level]
            row[:] = 0
            row[0:4] = (level, k, (CONVERGED if conv else 0) | (CAPPED if cap else 0), rec[SEEN])
            per = np.zeros((self.B, GRAPH), dtype=f32)
            per[:, 0:4] = losses
            per[:, 4], per[:, 5] = r0, r
            per[:, 6], per[:, 7] = CS.norm32(sums[:, 0]), CS.norm32(sums[:, 1])
            row[HEAD:] = per.reshape(-1).view(np.int32)
        keep = int(rec[KEEP])
        if keep > 0:
            self.snap[level % keep] = uvp
        self.x_backup[:, 0:3] = uvp
        self.x = self.x_backup.copy()
        rec[INNER] = 0
        rec[LEVEL] = level + 1
        rec[DONE] = 1 if (level + 1 >= rec[TARGET] or level + 1 >= self.max_levels) else 0
        return "latched"
