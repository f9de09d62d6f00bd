"""The normative numpy model of ott_query_sparse.  Row r has entries (i_0 < i_1 < ..., v_j); query b has distinct
indices with weights w.  S = +0.0f; for j ascending, wherever i_j is one of the query's, S = fl(S + fl(v_j * w(i_j))): IEEE f32, round
to nearest even, one rounded operation at a time, nothing fused, no flush to zero.  Row r is a CANDIDATE of query b iff one of its
indices is one of the query's, whatever the values are.  Candidates survive the masks, a NaN S drops the row, the filter acts on S,
the order is the canonical one (S under `take`, equal S to the lower row); hit.query = b.

score_row is the definition, one row at a time.  scores does the same serial sum for every row at once (position p of all rows in
one numpy operation); scores_dense is what the kernel evaluates — every entry times a dense weight table, the overlap tracked
apart — and must give the same bits (tests/test_sparse_cpu.py)."""
import numpy as np

import manhattan_ref as M

F32 = np.float32


def csr(rows):
    """list of (indices, values) -> (indptr u64, indices u32, values f32)"""
    ptr = np.zeros(len(rows) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(i) for i, _ in rows], dtype=np.uint64)
    idx = np.concatenate([np.asarray(i, np.uint32) for i, _ in rows]) if rows else np.zeros(0, np.uint32)
    val = np.concatenate([np.asarray(v, np.float32) for _, v in rows]) if rows else np.zeros(0, np.float32)
    return ptr, idx.astype(np.uint32), val.astype(np.float32)


def score_row(idx, val, q_idx, q_val):
    """(S, overlap) of one row and one query: THE DEFINITION"""
    w = {int(i): F32(x) for i, x in zip(q_idx, q_val)}
    S, overlap = F32(0.0), False
    with np.errstate(all="ignore"):
        for i, v in zip(idx, val):
            if int(i) in w:
                S = F32(S + F32(F32(v) * w[int(i)]))
                overlap = True
    return S, overlap


def _table(q_idx, q_val, vocab):
    w = np.zeros(vocab, np.float32)
    present = np.zeros(vocab, bool)
    w[np.asarray(q_idx, np.int64)] = np.asarray(q_val, np.float32)
    present[np.asarray(q_idx, np.int64)] = True
    return w, present


def scores(indptr, indices, values, queries, vocab, dense=False):
    """(S[nq, n] f32, cand[nq, n] bool).  dense = False: the definition (only shared entries are added); True: every entry is
    multiplied by the dense table and added, the overlap comes from the presence bits"""
    indptr = np.asarray(indptr, np.int64)
    n = indptr.size - 1
    lens = np.diff(indptr)
    S = np.zeros((len(queries), n), np.float32)
    cand = np.zeros((len(queries), n), bool)
    with np.errstate(all="ignore"):
        for b, (q_idx, q_val) in enumerate(queries):
            w, present = _table(q_idx, q_val, vocab)
            for p in range(int(lens.max()) if n else 0):  # serial in the row's index order, all rows at once
                rows = np.flatnonzero(lens > p)
                e = indptr[rows] + p
                i = indices[e].astype(np.int64)
                m = present[i]
                if dense:
                    S[b, rows] = S[b, rows] + values[e] * w[i]
                else:
                    S[b, rows[m]] = S[b, rows[m]] + values[e[m]] * w[i[m]]
                cand[b, rows[m]] = True
    assert S.dtype == np.float32
    return S, cand


def expected(S, cand, take, k, cmp=0, thr=0.0, keep=None):
    """[hits of query b]: candidates that survive `keep`, NaN dropped, the filter on S, canonical order, cut at k; `query` = b"""
    out = []
    for b in range(S.shape[0]):
        mask = cand[b] if keep is None else cand[b] & np.asarray(keep, bool)
        h = M.select_canonical(S[b][None], take, k, cmp, thr, mask).copy()
        h["query"] = b
        out.append(h)
    return out


def query(indptr, indices, values, queries, vocab, take, k, cmp=0, thr=0.0, keep=None):
    S, cand = scores(indptr, indices, values, queries, vocab)
    return expected(S, cand, take, k, cmp, thr, keep)
