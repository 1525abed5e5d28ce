"""The summation order of the chunked double sums (csrc/gfv_reduce.h, "Summation order"), restated in numpy.

Written from that paragraph, not from the kernels: tests/test_chunk_sums_gpu.py compares the kernels with it bit for bit.

  * per row: differences in fp32, squares and every sum in float64;
  * per chunk (rows chunk_beg[c] .. min(chunk_end[c], N) - 1): lane l of 64 adds the rows beg + l, beg + l + 64, ... in ascending
    order, starting from +0.0; the 64 lane sums fold by a xor butterfly, levels 32, 16, ... 1 (v[l] = v[l] + v[l ^ o]);
  * per graph (chunks gchunk_ptr[b] .. min(gchunk_ptr[b + 1], n_chunks) - 1): lane l adds the chunk sums c0 + l, c0 + l + 64, ...
    in ascending order, then the same butterfly;
  * a norm is np.float32(np.sqrt(.)) of the graph's sum: the square root in float64, rounded to fp32 once.
"""
import numpy as np

LANES = 64


def butterfly(v):
    """v [64, K] float64 -> [K]: what every lane holds after the levels 32 ... 1 (a + b == b + a bit for bit, so all lanes agree)."""
    v = np.array(v, dtype=np.float64)
    lane = np.arange(LANES)
    o = LANES // 2
    while o >= 1:
        v = v + v[lane ^ o]
        o //= 2
    assert (v == v[0]).all() or np.isnan(v).any()
    return v[0]


def lane_strided(values, beg, end):
    """values [*, K] float64: lane l adds values[beg + l], values[beg + l + 64], ... (< end) in ascending order -> [64, K]."""
    acc = np.zeros((LANES, values.shape[1]), dtype=np.float64)
    for j in range(beg, end, LANES):
        n = min(LANES, end - j)
        acc[:n] = acc[:n] + values[j:j + n]
    return acc


def chunk_sums(terms, chunk_beg, chunk_end, N):
    """terms [N, K] float64 (one value per row and sum) -> the per-chunk sums [n_chunks, K]."""
    return np.stack([butterfly(lane_strided(terms, int(b), min(int(e), N))) for b, e in zip(chunk_beg, chunk_end)])


def graph_sums(partial, gchunk_ptr):
    """per-chunk sums [n_chunks, K] -> per-graph sums [B, K]."""
    n_chunks = partial.shape[0]
    return np.stack([butterfly(lane_strided(partial, int(gchunk_ptr[b]), min(int(gchunk_ptr[b + 1]), n_chunks)))
                     for b in range(len(gchunk_ptr) - 1)])


def norm32(s):
    return np.float32(np.sqrt(np.asarray(s, dtype=np.float64)))


def sq(a):
    """fp32 values -> their squares in float64 (exact: 24-bit significands)."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    return a * a


def diff_norm_terms(new, old):
    """The two sums of a rollout / sweep step per row: ((e0^2 + e1^2) + e2^2) with e = new - old in fp32, and the same of new."""
    e = np.asarray(new, np.float32) - np.asarray(old, np.float32)
    assert e.dtype == np.float32
    d, n = sq(e), sq(new)
    return np.stack([(d[:, 0] + d[:, 1]) + d[:, 2], (n[:, 0] + n[:, 1]) + n[:, 2]], axis=1)


def eval_terms(pred, cur, tgt, row_has_target):
    """The twelve sums of an evaluation per row: per channel (pred - cur)^2, pred^2, (pred - tgt)^2, tgt^2; the last six are
    +0.0 on the rows of a graph without a target."""
    pred, cur, tgt = (np.asarray(a, np.float32) for a in (pred, cur, tgt))
    t = np.concatenate([sq(pred - cur), sq(pred), sq(pred - tgt), sq(tgt)], axis=1)
    t[~row_has_target, 6:] = 0.0
    return t


# ---- the one shape of tests/test_chunk_sums_gpu.py ------------------------------------------------------------------------
# B = 3 graphs of 1, 6 and 70 chunks: 77 chunks (no multiple of the 4 waves of a workgroup), one graph with more than 64 (a fold
# lane takes two).  Rows per chunk 1 .. 100 (a lane adds one row, two rows or none); the last chunk's end lies past N.
ROWS = [[37], [1, 100, 64, 65, 17, 63], [1 + (37 * j + 11) % 100 for j in range(70)]]
OVERHANG = 5


def tables():
    """-> chunk_beg, chunk_end, gchunk_ptr (int32), N, the graph of every row [N]."""
    rows = np.array([r for g in ROWS for r in g], dtype=np.int64)
    assert rows.min() == 1 and rows.max() == 100 and len(rows) == 77
    end = np.cumsum(rows)
    beg = end - rows
    N = int(end[-1])
    end[-1] += OVERHANG
    gcp = np.concatenate(([0], np.cumsum([len(g) for g in ROWS])))
    row_graph = np.repeat(np.arange(len(ROWS)), [sum(g) for g in ROWS])
    return beg.astype(np.int32), end.astype(np.int32), gcp.astype(np.int32), N, row_graph


def fields(N, seed):
    """fp32 fields whose magnitudes spread over about 1e3, so that another order of any of the sums moves its last bits."""
    rng = np.random.default_rng(seed)
    spread = lambda shape: (rng.standard_normal(shape) * 10.0 ** rng.uniform(-1.5, 1.5, shape)).astype(np.float32)
    return dict(uvp=spread((N, 3)), x_backup=spread((N, 12)), target=spread((N, 3)),
                losses=rng.uniform(0.1, 2.0, (len(ROWS), 4)).astype(np.float32))
