"""Wide top-K (include/hhfm.h "Wide K") restated in numpy — TEST INFRASTRUCTURE ONLY.

The order is tf.nn.top_k's: score descending, index ascending on equal scores,
``np.lexsort((idx, -score))``.  ``blockwise`` restates the catalog route for
catalogs beyond the dense limit: a select per block of items, each merged into
a running list; it must equal the one-shot select (the order is total).
"""
import numpy as np

F32 = np.float32
NO_IDX = 0x7fffffff
NARROW_MAX_K = 64
MAX_K = 1024
BLOCK_ITEMS = 16384


def topk_row(row, K, ids=None):
    """(scores float32 [K], ids int64 [K]) of one row; ``ids`` default to the
    column numbers.  Fewer than K entries: -inf / NO_IDX behind them."""
    row = np.asarray(row, F32)
    ids = np.arange(len(row), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    order = np.lexsort((ids, -row.astype(np.float64)))[:K]
    s = np.full(K, -np.inf, F32)
    i = np.full(K, NO_IDX, np.int64)
    s[:len(order)] = row[order]
    i[:len(order)] = ids[order]
    return s, i


def topk(scores, K, base=0):
    """tf.nn.top_k(scores, K) -> (float32 [B, K], int32 [B, K] = base + column)."""
    scores = np.asarray(scores, F32)
    out_s = np.empty((len(scores), K), F32)
    out_i = np.empty((len(scores), K), np.int64)
    for b, row in enumerate(scores):
        out_s[b], out_i[b] = topk_row(row, K)
    real = out_i != NO_IDX
    out_i[real] += base
    return out_s, out_i.astype(np.int32)


def merge(lists_s, lists_i, K=None):
    """R sorted lists [R, B, K] -> [B, K]; (-inf, NO_IDX) slots are empty and
    rank behind every entry."""
    lists_s = np.asarray(lists_s, F32)
    lists_i = np.asarray(lists_i, np.int64)
    R, B, K0 = lists_s.shape
    K = K0 if K is None else K
    out_s = np.empty((B, K), F32)
    out_i = np.empty((B, K), np.int64)
    for b in range(B):
        out_s[b], out_i[b] = topk_row(lists_s[:, b].reshape(-1), K, lists_i[:, b].reshape(-1))
    return out_s, out_i.astype(np.int32)


def blockwise(scores, K, base=0, block=BLOCK_ITEMS):
    """The blocked route: per block of ``block`` columns a select with the
    block's id base (a short block contributes what it has), each merged into
    the running list."""
    scores = np.asarray(scores, F32)
    run = None
    for c0 in range(0, scores.shape[1], block):
        cur = topk(scores[:, c0:c0 + block], K, base + c0)
        run = cur if run is None else merge(np.stack([run[0], cur[0]]),
                                            np.stack([run[1], cur[1]]))
    return run


def topk_admissible(scores, K, excluded, base=0):
    """Top K over the columns that ``excluded[b]`` (column numbers) does not
    name."""
    scores = np.asarray(scores, F32)
    out_s = np.empty((len(scores), K), F32)
    out_i = np.empty((len(scores), K), np.int64)
    for b, row in enumerate(scores):
        keep = np.setdiff1d(np.arange(len(row)), np.asarray(list(excluded[b]), np.int64))
        out_s[b], out_i[b] = topk_row(row[keep], K, keep)
    return out_s, (out_i + base).astype(np.int32)
