"""The expected answer of a batch with a row mask per query (ott_query_masks): ONE oracle call per query with
row_mask = common & mask_b, canonical ties; Manhattan through tests/manhattan_ref.py."""
import numpy as np

import manhattan_ref as M


def keep_of(n, common, mask):
    """common & mask over n rows; a mask shorter than n keeps the rows behind it (src/vec.rs:234); None = every row"""
    keep = np.ones(n, bool)
    for m in (common, mask):
        if m is not None:
            m = np.asarray(m, bool)
            keep[:min(n, m.size)] &= m[:n]
    return keep


def expected(oracle, rows, queries, masks, metric, take, k, cmp=0, thr=0.0, common=None):
    """[hits of query b alone with common & masks[b]] for every b; `query` of every hit is b"""
    out = []
    for b, mask in enumerate(masks):
        keep = keep_of(rows.shape[0], common, mask)
        if int(metric) == 3:
            h = M.query(rows, queries[b], take, k, cmp, thr, row_mask=keep)
        else:
            h = oracle.vec_query(rows, queries[b][None], int(metric), take, k, cmp, thr, row_mask=keep, ties=oracle.TIES_CANONICAL)
        h = h.copy()
        h["query"] = b
        out.append(h)
    return out
