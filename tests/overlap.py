"""Which C calls of different threads ran at the same time, from their wall-clock intervals.  Test infrastructure: no GPU, no NumPy.

The library does not say which query context served a call (on purpose: include/otters_hip.h has no symbol for it).  A context's `mu`
is held from acquire to release, that is for nearly the whole C call, so two calls on one store whose intervals overlap by a good part
cannot both have run on the store's own context: one of them ran on a worker.  "A good part" is half of the shorter call — the few
microseconds a call spends before it acquires and after it releases never amount to that."""


def pairs(intervals):
    """intervals: (thread, t0_ns, t1_ns) triples.  Returns the pairs (a, b) of triples from DIFFERENT threads whose common part is
    non-empty and at least half of the shorter of the two calls."""
    iv = sorted(intervals, key=lambda x: (x[1], x[2]))
    out = []
    for i, a in enumerate(iv):
        for b in iv[i + 1:]:
            if b[1] >= a[2]:  # sorted by start: nothing later begins inside a
                break
            if a[0] == b[0]:
                continue
            common = min(a[2], b[2]) - b[1]
            shorter = min(a[2] - a[1], b[2] - b[1])
            if common > 0 and 2 * common >= shorter:
                out.append((a, b))
    return out
