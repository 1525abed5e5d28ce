"""The summation order of the training log's bucket sums (include/gfv.h gfv_train_log_norms; csrc/trainlog.hip, header comment),
restated in numpy.  Written from that paragraph, not from the kernel: tests/test_trainlog_gpu.py compares the kernel with it bit
for bit.

A bucket is a list of (offset, count) segments into the flat buffers; its elements are numbered j = 0 .. n - 1 in the order of the
concatenated segments, and the order of summation is a function of j alone:

  * per element: the fp32 value widened to float64 and squared (exact); the non-finite mark is 1.0 or 0.0;
  * per chunk c (elements 1024 c .. min(1024 (c + 1), n) - 1): lane l of 64 adds, starting from +0.0, the elements
    1024 c + 256 r + 4 l + (0, 1, 2, 3) for r = 0, 1, 2, 3 in ascending order; the 64 lane sums fold by a xor butterfly, levels
    32, 16, ... 1 (v[l] = v[l] + v[l ^ o]);
  * per bucket: lane l adds the chunk sums l, l + 64, ... in ascending order, starting from +0.0, then the same butterfly.

(An index past n contributes nothing; adding +0.0 in its place leaves every bit of a sum of non-negative terms as it is, which is
how the padding below stands for "nothing".)"""
import numpy as np

LANES, CHUNK, ROUNDS, QUAD = 64, 1024, 4, 4
assert CHUNK == ROUNDS * LANES * QUAD


def butterfly(v):
    """v [64, ...] float64 -> what every lane holds after the levels 32 .. 1."""
    v = np.array(v, dtype=np.float64)
    lane = np.arange(LANES)
    o = LANES // 2
    while o >= 1:
        with np.errstate(invalid="ignore"):
            v = v + v[lane ^ o]
        o //= 2
    return v[0]


def gather(flat, segs):
    """The bucket's elements in logical order."""
    flat = np.asarray(flat)
    return np.concatenate([flat[int(o):int(o) + int(k)] for o, k in segs]) if len(segs) else flat[:0]


def ordered_sum(terms):
    """terms [n] float64, one per logical element -> the bucket's sum in the order above."""
    terms = np.asarray(terms, dtype=np.float64)
    n = terms.shape[0]
    n_chunks = (n + CHUNK - 1) // CHUNK
    pad = np.zeros(n_chunks * CHUNK, dtype=np.float64)
    pad[:n] = terms
    q = pad.reshape(n_chunks, ROUNDS, LANES, QUAD).transpose(0, 2, 1, 3).reshape(n_chunks, LANES, ROUNDS * QUAD)
    chunk = np.zeros(n_chunks, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(n_chunks):
            lane = np.zeros(LANES, dtype=np.float64)
            for i in range(ROUNDS * QUAD):
                lane = lane + q[c, :, i]
            chunk[c] = butterfly(lane)
        lane = np.zeros(LANES, dtype=np.float64)
        for c0 in range(0, n_chunks, LANES):
            m = min(LANES, n_chunks - c0)
            lane[:m] = lane[:m] + chunk[c0:c0 + m]
    return butterfly(lane)


def bucket_sums(g, p, segs):
    """-> (sum g^2, sum p^2, count of non-finite g) of one bucket: two float64 and an int, g and p fp32 flat buffers."""
    gv = gather(np.asarray(g, dtype=np.float32), segs).astype(np.float64)
    pv = gather(np.asarray(p, dtype=np.float32), segs).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        gs, ps = ordered_sum(gv * gv), ordered_sum(pv * pv)
    bad = ordered_sum((~np.isfinite(gv)).astype(np.float64))
    return gs, ps, int(bad)


def same_bits(a, b):
    """Bit equality of float64 values, NaN equal to NaN of the same bits."""
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))
