"""The sampling window (include/gfv.h GFV_WINDOW_RECORD) restated in plain Python: the record's words, the decision and what the
last arriver writes.  Written from the header's paragraph, not from csrc/gfv_window.h.  tests/fieldstats_ref.py and
tests/wallforce_ref.py build on it.  Nothing here touches a GPU.
"""
START, STRIDE, STOP, LAST, N, COUNTER, ENABLED = range(7)
RECORD = 8


def take(rec, c):
    """Whether a sampler's launches that find the record `rec` and the clock value `c` sample."""
    start, stride, stop = int(rec[START]), max(int(rec[STRIDE]), 1), int(rec[STOP])
    return bool(rec[ENABLED] != 0 and c != int(rec[LAST]) and c >= start and (stop < 0 or c < stop) and (c - start) % stride == 0)


def commit(rec, c, taken):
    """What the last arriver writes: the clock is followed, a sample counted, the counter back to zero."""
    if c != int(rec[LAST]):
        rec[LAST] = c
    if taken:
        rec[N] += 1
    rec[COUNTER] = 0
