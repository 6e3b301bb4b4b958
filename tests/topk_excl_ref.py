"""Numpy restatement of the exclusion lists — TEST INFRASTRUCTURE ONLY.

include/hhfm.h "Exclusion lists": per query a strictly ascending list of table
rows that a catalog top-K leaves out, as CSR arrays ``ptr`` int64 [B + 1] and
``rows`` int32 [ptr[B]].  Here:

* ``lists_from_pf``: the lists hhfm_pf_exclusion_lists builds from a
  positive_feedback dict (key = every column of a row but the item -> set of
  item ids): the key's items ascending, nothing for an unknown key, the row's
  own item left out under ``keep_own``;
* ``csr`` / ``uncsr``: sequences <-> the CSR arrays;
* ``filtered_topk``: the top K of a score matrix's non-excluded columns under
  (score descending, index ascending) — tf.nn.top_k's order over what is left.
  A row outside the shard, a negative one or one past the table only fails to
  match a column, as in the library.
"""
import numpy as np

F32 = np.float32


def row_key(row, item_col=1):
    return tuple(int(x) for c, x in enumerate(row) if c != item_col)


def lists_from_pf(pf, rows, item_col=1, keep_own=False):
    """-> list of B ascending int64 arrays."""
    out = []
    for row in np.asarray(rows):
        items = set(int(x) for x in pf.get(row_key(row, item_col), ()))
        if keep_own:
            items.discard(int(row[item_col]))
        out.append(np.array(sorted(items), dtype=np.int64))
    return out


def csr(lists):
    """-> (ptr int64 [B + 1], rows int32 [total], longest list)."""
    ptr = np.zeros(len(lists) + 1, np.int64)
    for b, x in enumerate(lists):
        ptr[b + 1] = ptr[b] + len(x)
    flat = np.concatenate([np.asarray(x, np.int64) for x in lists]) if len(lists) \
        else np.zeros(0, np.int64)
    return ptr, flat.astype(np.int32), max((len(x) for x in lists), default=0)


def uncsr(ptr, rows):
    ptr = np.asarray(ptr)
    return [np.asarray(rows[ptr[b]:ptr[b + 1]], np.int64) for b in range(len(ptr) - 1)]


def filtered_topk(scores, K, lists, row_begin, lo=0, cnt=None, gbase=0):
    """scores float32 [B, N]: column i is table row ``row_begin + i``.  The
    shard is columns [lo, lo + cnt); ids are gbase + offset in the shard.
    -> (float32 [B, K] — the picked elements' own bits —, int32 [B, K])."""
    scores = np.asarray(scores, F32)
    cnt = scores.shape[1] - lo if cnt is None else cnt
    out_s = np.empty((len(scores), K), F32)
    out_i = np.empty((len(scores), K), np.int32)
    for b, row in enumerate(scores):
        sub = row[lo:lo + cnt]
        off = np.asarray(lists[b], np.int64) - (row_begin + lo)
        keep = np.ones(cnt, bool)
        keep[off[(off >= 0) & (off < cnt)]] = False
        idx = np.flatnonzero(keep)
        assert len(idx) >= K, "a list may not run the range short of K"
        order = idx[np.argsort(-sub[idx], kind="stable")[:K]]
        out_s[b] = sub[order]
        out_i[b] = order + gbase
    return out_s, out_i
