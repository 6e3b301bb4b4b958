"""HHFM with MAX / MEAN pooling — TEST INFRASTRUCTURE ONLY.

A numpy restatement of the pooled graph of OurModel7.py (Pooling1C :124 /
:255, Pooling1T :141 / :267, Pooling1F :168 / :292 set to tf.reduce_max or
tf.reduce_mean) in the arithmetic include/hhfm.h "Pooling" fixes:

  ``hybrid`` / ``score_rows`` / ``catalog_scores``   the fp32 forward
  ``exact_rows`` / ``exact_catalog``                 its float64 value and Σ|terms|
  ``train_step``                                     one fp32 training step
  ``hhfm_pool_grad64``                               the float64 loss and gradient with
                                                     the propagated magnitude ``mag``,
                                                     in the form of train_ref.hhfm_grad64
  ``hhfm_pool_case``                                 seeded inputs with planted rows

A pool's gradient is linear once its selection is fixed: every value v of a
pool receives weight · d, weight 1 (sum), 1/n (mean) or 1/(number of values
equal to the maximum) for those values and 0 for the others (max; TF
_MinOrMaxGrad).  ``pool_weights`` takes every selection from the fp32 values —
table rows, and fp32-pooled stack members — as train_ref.tie_mask does for the
negatives, so float64 never re-decides what fp32 saw as equal or largest.
"""
import numpy as np

from oracle import fm_oracle as orc
from tests import train_ref as tr

F32, F64 = np.float32, np.float64
SUM, MAX, MEAN = 0, 1, 2
_NAMES = {"sum": SUM, "max": MAX, "mean": MEAN}


def modes_of(pooling):
    """(ctx, time, final) as 0 / 1 / 2 from names or POOL_* values."""
    return tuple(_NAMES.get(m, m) for m in pooling)


def _cols(rng_):
    return list(range(rng_[0], rng_[1])) if rng_[1] > rng_[0] else []


def _pool(rows, mode):
    """rows [B, n, k] -> [B, k] in rows.dtype: sum ((r0 + r1) + ...), max, or
    that sum divided once by n."""
    if mode == MAX:
        return rows.max(1)
    acc = rows[:, 0]
    for j in range(1, rows.shape[1]):
        acc = acc + rows[:, j]
    return acc / rows.dtype.type(rows.shape[1]) if mode == MEAN else acc


def _final(members, mode):
    if len(members) == 1:
        return members[0]
    return _pool(np.stack(members, 1), mode)


def hybrid(E, X, ctx, tim, pooling, ucol=0, dtype=F32, parts=False):
    """h [B, k]: the final pool over {user, context pool, time pool}."""
    mc, mt, mf = modes_of(pooling)
    E = np.asarray(E, dtype)
    X = np.asarray(X, np.int64)
    members = [E[X[:, ucol]]]
    if _cols(ctx):
        members.append(_pool(E[X[:, _cols(ctx)]], mc))
    if _cols(tim):
        members.append(_pool(E[X[:, _cols(tim)]], mt))
    h = _final(members, mf)
    return (h, members) if parts else h


def score_rows(X, E, ctx, tim, pooling, ucol=0, icol=1):
    """PositiveFeadback [B] in fp32 (OurModel7.py:171)."""
    h = hybrid(E, X, ctx, tim, pooling, ucol)
    it = np.asarray(E, F32)[np.asarray(X, np.int64)[:, icol]]
    return (h * it).sum(1, dtype=F32)


def catalog_scores(A, E, n_user, n_item, ctx, tim, pooling):
    """[B, n_item] fp32 scores of OurModel7.py:294."""
    h = hybrid(E, A, ctx, tim, pooling)
    item = np.asarray(E, F32)[n_user:n_user + n_item]
    return (h[:, None, :] * item[None, :, :]).sum(2, dtype=F32)


def _abs_hybrid(E, X, ctx, tim, pooling, ucol=0):
    """The pooled graph over |rows| in float64: Σ|terms| per element (max of
    magnitudes bounds |max|, the mean keeps its 1/n)."""
    return hybrid(np.abs(np.asarray(E, F64)), X, ctx, tim, pooling, ucol, F64)


def exact_rows(X, E, ctx, tim, pooling, ucol=0, icol=1):
    """-> float64 score and Σ|terms| per row, from the fp32 table."""
    E64 = np.asarray(E, F32).astype(F64)
    it = E64[np.asarray(X, np.int64)[:, icol]]
    h = hybrid(E64, X, ctx, tim, pooling, ucol, F64)
    return (h * it).sum(1), (_abs_hybrid(E64, X, ctx, tim, pooling, ucol) * np.abs(it)).sum(1)


def exact_catalog(A, E, n_user, ctx, tim, pooling):
    """oracle.parity.hhfm_exact for the pooled h: float64 scores of (query b,
    item offsets ids) and their Σ|terms|."""
    E64 = np.asarray(E, F32).astype(F64)
    h = hybrid(E64, A, ctx, tim, pooling, dtype=F64)
    ah = _abs_hybrid(E64, A, ctx, tim, pooling)

    def exact(b, ids):
        it = E64[n_user + np.asarray(ids, np.int64)]
        return it @ h[b], np.abs(it) @ ah[b]
    return exact


# ---------------------------------------------------------------------------
# gradient
# ---------------------------------------------------------------------------
def _sel(values, mode):
    """values [B, n, k] (fp32) -> float64 weights [B, n, k] of the pool's gradient."""
    n = values.shape[1]
    if mode == SUM:
        return np.ones(values.shape, F64)
    if mode == MEAN:
        return np.full(values.shape, 1.0 / n, F64)
    ind = (values == values.max(1, keepdims=True)).astype(F64)
    return ind / ind.sum(1, keepdims=True)


def pool_weights(X, E, ctx, tim, pooling):
    """-> cols, W [B, len(cols), k]: dh_e reaches E[X[b, cols[j]], e] as
    W[b, j, e] · dh_e.  cols = [0] + context columns + time columns; every
    selection from fp32 values."""
    mc, mt, mf = modes_of(pooling)
    E32 = np.asarray(E, F32)
    X = np.asarray(X, np.int64)
    h, members = hybrid(E32, X, ctx, tim, pooling, parts=True)
    wf = _sel(np.stack(members, 1), mf) if len(members) > 1 else np.ones((len(X), 1, E32.shape[1]))
    cols, W, m = [0], [wf[:, :1]], 1
    for rng_, mode in ((ctx, mc), (tim, mt)):
        if _cols(rng_):
            cols += _cols(rng_)
            W.append(wf[:, m:m + 1] * _sel(E32[X[:, _cols(rng_)]], mode))
            m += 1
    return cols, np.concatenate(W, 1)


def tie_mask(X, Neg, E, ctx, tim, pooling):
    """train_ref.tie_mask with the pooled h: the negatives whose table row is
    bit-identical to the row of the float64 maximum."""
    X, Neg = np.asarray(X, np.int64), np.asarray(Neg, np.int64)
    E32 = np.ascontiguousarray(E, F32)
    E64 = E32.astype(F64)
    cols, W = pool_weights(X, E32, ctx, tim, pooling)
    h = (W * E64[X[:, cols]]).sum(1)
    best = np.einsum("bc,bjc->bj", h, E64[Neg]).argmax(1)
    top = E32[Neg[np.arange(len(Neg)), best]]
    return (E32[Neg].view(np.uint32) == top.view(np.uint32)[:, None, :]).all(2)


def hhfm_pool_grad64(X, Neg, E, ctx, tim, ties, pooling):
    """train_ref.hhfm_grad64 for the pooled h -> loss, dE, magE, info.  With
    the selections fixed (``pool_weights``) h = Σ_j W_j · E[x_j] exactly, so
    the float64 forward is that sum in column order and the gradient of column
    j is W_j · dh; with (sum, sum, sum) every weight is 1.0 and this is
    hhfm_grad64 operation for operation."""
    X, Neg = np.asarray(X, np.int64), np.asarray(Neg, np.int64)
    cols, W = pool_weights(X, E, ctx, tim, pooling)
    E = np.asarray(E, F64)
    ties = np.asarray(ties, bool)
    h = (W * E[X[:, cols]]).sum(1)
    it = E[X[:, 1]]
    n = E[Neg]                                          # [B, NG, k]
    pos = (h * it).sum(1)
    neg = np.einsum("bc,bjc->bj", h, n)
    mx = neg.max(1)
    assert ties.any(1).all() and np.all(neg[ties] == np.repeat(mx, ties.sum(1)))
    nt = ties.sum(1)
    wt = ties / nt[:, None]
    ah = np.abs(h)
    fh = (W * np.abs(E[X[:, cols]])).sum(1)             # |factor| of the item / negative terms
    S = (ah * np.abs(it)).sum(1) + (np.einsum("bc,bjc->bj", ah, np.abs(n)) * wt).sum(1)
    gap = np.where(ties, np.inf, mx[:, None] - neg).min(1)
    z = pos - mx
    sg = 1.0 / (1.0 + np.exp(-z))
    g = sg - 1.0                                        # d(−log σ(z))/dz
    a = np.abs(g) + S
    nbar = (wt[:, :, None] * n).sum(1)
    nabar = (wt[:, :, None] * np.abs(n)).sum(1)
    dh = g[:, None] * (it - nbar)
    mh = a[:, None] * (np.abs(it) + nabar)
    dE, mE = np.zeros_like(E), np.zeros_like(E)
    np.add.at(dE, X[:, 1], g[:, None] * h)
    np.add.at(mE, X[:, 1], a[:, None] * fh)
    for j in range(Neg.shape[1]):
        np.add.at(dE, Neg[:, j], -(g * wt[:, j])[:, None] * h)
        np.add.at(mE, Neg[:, j], (a * wt[:, j])[:, None] * fh)
    for j, c in enumerate(cols):
        np.add.at(dE, X[:, c], W[:, j] * dh)
        np.add.at(mE, X[:, c], W[:, j] * mh)
    return -np.log(sg).sum(), dE, mE, dict(z=z, margin=float((gap / S).min()), nt=nt)


def loss64(X, Neg, E, ctx, tim, pooling):
    """The float64 loss of the pooled graph itself (max and mean evaluated in
    float64, nothing fixed): what central differences are taken of."""
    X, Neg = np.asarray(X, np.int64), np.asarray(Neg, np.int64)
    E = np.asarray(E, F64)
    h = hybrid(E, X, ctx, tim, pooling, dtype=F64)
    pos = (h * E[X[:, 1]]).sum(1)
    mx = np.einsum("bc,bjc->bj", h, E[Neg]).max(1)
    return -np.log(1.0 / (1.0 + np.exp(-(pos - mx)))).sum()


def train_step(X, Neg, E, slot, lr, lam, ctx, tim, pooling, optimizer="adagrad", step=1,
               grad_only=False):
    """One fp32 step of OUR.partial_fit with the pooled h (oracle.fm_oracle.
    hhfm_train_step's arithmetic; the update is its tf_apply) -> loss, E, slot
    (``grad_only``: -> loss, dE without the l2 term)."""
    X, Neg = np.asarray(X, np.int64), np.asarray(Neg, np.int64)
    E = np.asarray(E, F32)
    cols, W = pool_weights(X, E, ctx, tim, pooling)
    W = W.astype(F32)
    h = hybrid(E, X, ctx, tim, pooling)
    it = E[X[:, 1]]
    pos = (h * it).sum(1, dtype=F32)
    neg = (h[:, None, :] * E[Neg]).sum(2, dtype=F32)
    mx = neg.max(1)
    z = pos - mx
    sg = (1.0 / (1.0 + np.exp(-z))).astype(F32)
    loss = F32(-np.sum(np.log(sg), dtype=F64) + lam * np.sum(E.astype(F64) ** 2) / 2)
    g = sg - F32(1)
    ind = (neg == mx[:, None]).astype(F32)
    ind /= ind.sum(1, keepdims=True)
    dh = g[:, None] * (it - (ind[:, :, None] * E[Neg]).sum(1))
    dE = np.zeros_like(E)
    np.add.at(dE, X[:, 1], g[:, None] * h)
    for j in range(Neg.shape[1]):
        np.add.at(dE, Neg[:, j], -(g * ind[:, j])[:, None] * h)
    for j, c in enumerate(cols):
        np.add.at(dE, X[:, c], W[:, j] * dh)
    if grad_only:
        return loss, dE
    dE += F32(lam) * E
    rows = np.concatenate([X.reshape(-1), Neg.reshape(-1)]) if lam == 0 else None
    E, slot = orc.tf_apply(optimizer, E, dE, slot, lr, step, rows)
    return loss, E, slot


# ---------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------
# name: (case of train_ref.HHFM_CASES the inputs derive from, k, pooling)
POOL_CASES = {
    "ctx_ng10_k4_max": ("ctx_ng10_k8", 4, ("max", "max", "max")),
    "ctx_ng1_k64_mean": ("ctx_ng1_k64", 64, ("mean", "mean", "mean")),
    "ctx_ng10_k128_maxsum": ("ctx_ng10_k8", 128, ("max", "max", "sum")),
    "both_ng10_k200_max": ("both_ng10_k100", 200, ("max", "max", "max")),
    "both_ng10_k64_meanmaxsum": ("both_ng10_k100", 64, ("mean", "max", "sum")),
    "both_ng2_k4_summaxmean": ("both_ng2_k8", 4, ("sum", "max", "mean")),
    "both_ng10_k64_summeanmax": ("both_ng10_k100", 64, ("sum", "mean", "max")),
    "both_ng16_k128_b1_mean": ("both_ng16_k128_b1", 128, ("mean", "mean", "mean")),
    "time_ng10_k64_max": ("time_ng10_k64", 64, ("max", "max", "max")),
    "time_ng16_k200_meanmax": ("time_ng16_k100", 200, ("sum", "mean", "max")),
    "none_ng10_k128_max": ("none_ng10_k128", 128, ("max", "max", "max")),
    "none_ng1_k4_b1_mean": ("none_ng1_k8_b1", 4, ("mean", "mean", "mean")),
}
PLANTED_ROWS = 9   # rows 0..4 train_ref.hhfm_case's, 5..8 below


def _lead_ok(X, E, ctx, tim, pooling):
    """Per row: at every element the largest stack member leads the second by
    more than 4·(nc + nt + 2)·2⁻²⁴·Σ|rows| (fp32 and float64 then select alike)."""
    _, members = hybrid(E, X, ctx, tim, pooling, parts=True)
    if len(members) < 2:
        return np.ones(len(X), bool)
    m = np.sort(np.stack(members, 1).astype(F64), 1)
    fields = [0] + _cols(ctx) + _cols(tim)
    mag = np.abs(np.asarray(E, F64)[np.asarray(X, np.int64)[:, fields]]).sum(1)
    thr = 4.0 * (len(fields) + 1) * 2.0 ** -24 * mag
    return ((m[:, -1] - m[:, -2]) > thr).all(1)


def hhfm_pool_case(name):
    """-> X, Neg, E, ctx, tim, ties, pooling, info.  train_ref.hhfm_case's
    rows (its planted rows 0..4 included: row 4 holds a context / time id equal
    to the user id) at this case's k, and when B > 8 and the layout has fields:
      row 5  one context (time) id twice in a row
      row 6  two context (time) ids with bit-identical table rows
      row 7  context (time) values all negative at element 0
    When the final pool is max over a computed member (a sum or mean pool),
    rows that fail ``_lead_ok`` get a fresh user until they pass;
    info["redrawn"] counts them."""
    base, k, pooling = POOL_CASES[name]
    layout, NG, _, B = tr.HHFM_CASES[base]
    fd, td = tr.LAYOUTS[layout]
    X, Neg, E0, ctx, tim, _ = tr.hhfm_case(base)
    rng = np.random.default_rng(sorted(POOL_CASES).index(name) + 900)
    M = E0.shape[0]
    # a table of this case's k; train_ref's row-3 twin rows stay twins
    std = (0.3 / (k * (1 + fd + td)) ** 0.5) ** 0.5
    E = rng.normal(0, std, (M, k)).astype(F32)
    if B > 4 and NG >= 2:
        E[Neg[3, 1]] = E[Neg[3, 0]]
    f = _cols(ctx) + _cols(tim)
    if B > 8 and len(f) >= 2:
        X[5, f[1]] = X[5, f[0]]
        if X[6, f[1]] == X[6, f[0]]:
            X[6, f[1]] = X[6, f[0]] + 1
        a, b = X[6, f[0]], X[6, f[1]]
        neg = list(X[7, f]) + ([a] if b in X[7, f] else [])   # the twin of a negative row too
        E[neg, 0] = -np.abs(E[neg, 0]) - F32(0.01)
        E[b] = E[a]
    mc, mt, mf = modes_of(pooling)
    computed = (fd and mc != MAX) or (td and mt != MAX)
    redrawn = 0
    if mf == MAX and computed:
        bad = np.flatnonzero(~_lead_ok(X, E, ctx, tim, pooling))
        for r in bad:
            for _ in range(50):
                X[r, 0] = rng.integers(0, tr.NU)
                if r == 4 and f:
                    X[r, f[0]] = X[r, 0]       # train_ref's plant: a field id equal to the user id
                if _lead_ok(X[r:r + 1], E, ctx, tim, pooling)[0]:
                    break
            else:
                raise AssertionError(f"{name}: row {r} finds no user with a clear lead")
        redrawn = len(bad)
    ties = tie_mask(X, Neg, E, ctx, tim, pooling)
    return X, Neg, E, ctx, tim, ties, pooling, dict(redrawn=redrawn, rows=B)
