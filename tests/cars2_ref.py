"""numpy restatement of CARS2 (Newcode/CARS2.py) — TEST INFRASTRUCTURE ONLY.

The graph is restated in the reference's own op order (CARS2.py:85-121 for the
rows and the loss, :171-187 for the catalog) — NOT in the folded association
the device uses (include/hhfm.h "CARS2") — in float32 by default and in float64
on request.  ``exact_*`` return (float64 value, Σ|elementary products|), the
two inputs of the project's score bar (tests/helpers.kappa_check,
oracle/parity.topk_tie_swaps).  ``grad64`` is the analytic gradient of the data
loss with the per-element magnitudes of tests/train_ref.py's bound, and
``train_step`` replays one TF-1.x optimizer step (oracle.fm_oracle.tf_apply).

A weight set is a dict UI [n_ui, D], Context [Mc, Dc], W [D, Dp, Dc],
Z [D, Dq, Dc], A [Dp], B [Dq]; a row is (user id, item id, context id).
"""
import numpy as np

from oracle import fm_oracle as orc

F32, F64 = np.float32, np.float64
NAMES = ("UI", "Context", "W", "Z", "A", "B")


def dims(D):
    """(Dc, Dp, Dq) of CARS2.py:54-56."""
    return int(D / 2.5), int(D / 5), int(D / 2.5)


def weights(seed, n_ui, Mc, D, std=0.3, ab=True):
    """A seeded weight set (legacy RandomState: a frozen stream, so fixtures
    can record the seed instead of the arrays).  ``ab=False``: A = B = 0, the
    reference's initial value (CARS2.py:160-163)."""
    Dc, Dp, Dq = dims(D)
    r = np.random.RandomState(seed)
    n = lambda *s: r.normal(0.0, std, s).astype(F32)   # noqa: E731
    Wt = dict(UI=n(n_ui, D), Context=n(Mc, Dc), W=n(D, Dp, Dc), Z=n(D, Dq, Dc), A=n(Dp), B=n(Dq))
    if not ab:
        Wt["A"][:] = 0
        Wt["B"][:] = 0
    return Wt


def _cast(Wt, dtype):
    return {k: np.asarray(Wt[k], dtype) for k in NAMES}


def _left(v, T3):
    """tf.reshape(tf.matmul(v, tf.reshape(T3, [D, -1])), [-1, P, Dc])  (:90, :93)"""
    D, P, Dc = T3.shape
    return (v @ T3.reshape(D, -1)).reshape(-1, P, Dc)


def _bilinear(v, T3, c):
    """reduce_sum(multiply(left, expand_dims(c, 1)), axis=2)  (:91, :94)"""
    return (_left(v, T3) * c[:, None, :]).sum(2)


def _feedback(u, i, c, W):
    """(:103-105)"""
    pik = _bilinear(u, W["W"], c)
    qjk = _bilinear(i, W["Z"], c)
    return ((u * i).sum(1, keepdims=True) + (pik * W["A"]).sum(1, keepdims=True)
            + (qjk * W["B"]).sum(1, keepdims=True))


def score_rows(X, Wt, dtype=F32):
    """PositiveFeadback [B, 1] for rows X [B, 3]."""
    X = np.asarray(X, np.int64)
    W = _cast(Wt, dtype)
    return _feedback(W["UI"][X[:, 0]], W["UI"][X[:, 1]], W["Context"][X[:, 2]], W)


def catalog_scores(q, Wt, n_user, n_item, dtype=F32):
    """CARS2.topk's Feedback [B, n_item] for queries q [B, 2] = (user, context
    id)  (:174-185)."""
    q = np.asarray(q, np.int64)
    W = _cast(Wt, dtype)
    users = W["UI"][q[:, 0]]
    items = W["UI"][n_user:n_user + n_item]
    c = W["Context"][q[:, 1]]
    pik = _bilinear(users, W["W"], c)
    left = _left(items, W["Z"])[None]                                  # 1, n, Dq, Dc
    qjk = (left * c[:, None, None, :]).sum(3)                          # B, n, Dq
    return users @ items.T + (pik * W["A"]).sum(1, keepdims=True) + (qjk * W["B"]).sum(2)


def top_k(scores, K):
    return orc.top_k(scores, K)


def loss(X, Fea, Neg, Wt, lam, dtype=F32):
    """self.loss (:87, :103-121) for X [B, 2], Fea [B], Neg [B, NG]."""
    X, Fea, Neg = (np.asarray(a, np.int64) for a in (X, Fea, Neg))
    W = _cast(Wt, dtype)
    u, i = W["UI"][X[:, 0]], W["UI"][X[:, 1]]
    n = W["UI"][Neg].sum(1)
    c = W["Context"][Fea]
    pos = _feedback(u, i, c, W)
    neg = _feedback(u, n, c, W)
    out = -np.sum(np.log(1.0 / (1.0 + np.exp(-(pos - neg)))), dtype=F64)
    if lam > 0:
        out = out + sum(lam * np.sum(np.asarray(Wt[k], F64) ** 2) / 2 for k in NAMES)
    return dtype(out)


def _abs(Wt):
    return {k: np.abs(np.asarray(Wt[k], F64)) for k in NAMES}


def _folds(W):
    WA = np.einsum("dpc,p->dc", W["W"], W["A"])
    ZB = np.einsum("dqc,q->dc", W["Z"], W["B"])
    return WA, ZB


def exact_rows(X, Wt):
    """-> (score float64 [B], Σ|elementary products| [B], trilinear share [B])."""
    X = np.asarray(X, np.int64)
    W, A = _cast(Wt, F64), _abs(Wt)
    s = score_rows(X, Wt, F64)[:, 0]
    aWA, aZB = _folds(A)
    au, ai, ac = A["UI"][X[:, 0]], A["UI"][X[:, 1]], A["Context"][X[:, 2]]
    tri = ((au @ aWA) * ac).sum(1) + ((ai @ aZB) * ac).sum(1)
    mag = (au * ai).sum(1) + tri
    del W
    return s, mag, tri / mag


def exact_catalog(q, Wt, n_user):
    """-> f(b, items) = (scores float64, Σ|elementary products|) of query b
    over the item offsets ``items``: the ``exact`` of helpers.topk_tie_swaps."""
    q = np.asarray(q, np.int64)
    W, A = _cast(Wt, F64), _abs(Wt)
    WA, ZB = _folds(W)
    aWA, aZB = _folds(A)

    def exact(b, items):
        items = np.asarray(items, np.int64) + n_user
        u, c = W["UI"][q[b, 0]], W["Context"][q[b, 1]]
        au, ac = A["UI"][q[b, 0]], A["Context"][q[b, 1]]
        it, ait = W["UI"][items], A["UI"][items]
        s = it @ (u + ZB @ c) + u @ (WA @ c)
        mag = ait @ (au + aZB @ ac) + au @ (aWA @ ac)
        return s, mag
    return exact


def min_top_gap(q, Wt, n_user, n_item, top=21):
    """The least gap between adjacent scores among a query's ``top`` best, as
    a fraction of that query's largest Σ|terms| (float64)."""
    exact = exact_catalog(q, Wt, n_user)
    worst = np.inf
    for b in range(len(q)):
        s, mag = exact(b, np.arange(n_item))
        t = np.sort(s)[::-1][:top]
        worst = min(worst, float(np.min(t[:-1] - t[1:]) / mag.max()))
    return worst


def grad64(X, Fea, Neg, Wt):
    """-> loss, {name: gradient}, {name: magnitude}, x of the DATA loss
    −Σ log σ(x_b) in float64 (include/hhfm.h "CARS2"); magnitudes as in
    tests/train_ref.py: Σ_rows (|g_b| + S_b)·|factor|."""
    X, Fea, Neg = (np.asarray(a, np.int64) for a in (X, Fea, Neg))
    W, A = _cast(Wt, F64), _abs(Wt)
    _, ZB = _folds(W)
    _, aZB = _folds(A)
    u, i, c = W["UI"][X[:, 0]], W["UI"][X[:, 1]], W["Context"][Fea]
    au, ac = A["UI"][X[:, 0]], A["Context"][Fea]
    dl = i - W["UI"][Neg].sum(1)
    adl = A["UI"][X[:, 1]] + A["UI"][Neg].sum(1)
    GB, aGB = c @ ZB.T, ac @ aZB.T                       # [B, D]
    x = (u * dl).sum(1) + (dl * GB).sum(1)
    S = (au * adl).sum(1) + (adl * aGB).sum(1)
    sg = 1.0 / (1.0 + np.exp(-x))
    g = sg - 1.0
    a = np.abs(g) + S
    G = {k: np.zeros_like(W[k]) for k in NAMES}
    M = {k: np.zeros_like(W[k]) for k in NAMES}
    np.add.at(G["UI"], X[:, 0], g[:, None] * dl)
    np.add.at(M["UI"], X[:, 0], a[:, None] * adl)
    np.add.at(G["UI"], X[:, 1], g[:, None] * (u + GB))
    np.add.at(M["UI"], X[:, 1], a[:, None] * (au + aGB))
    for j in range(Neg.shape[1]):
        np.add.at(G["UI"], Neg[:, j], -g[:, None] * (u + GB))
        np.add.at(M["UI"], Neg[:, j], a[:, None] * (au + aGB))
    np.add.at(G["Context"], Fea, g[:, None] * (dl @ ZB))
    np.add.at(M["Context"], Fea, a[:, None] * (adl @ aZB))
    T = np.einsum("b,bd,bc->dc", g, dl, c)
    aT = np.einsum("b,bd,bc->dc", a, adl, ac)
    G["Z"] = np.einsum("q,dc->dqc", W["B"], T)
    M["Z"] = np.einsum("q,dc->dqc", A["B"], aT)
    G["B"] = np.einsum("dqc,dc->q", W["Z"], T)
    M["B"] = np.einsum("dqc,dc->q", A["Z"], aT)
    return -np.log(sg).sum(), G, M, x


def train_step(X, Fea, Neg, Wt, slots, lr, lam, optimizer="adagrad", step=1):
    """One partial_fit with TF-1.x semantics -> (loss, weights, slots).  The
    gradient is grad64's rounded to float32 plus λ·var; with λ > 0 every
    variable is dense, at λ = 0 UI and Context are IndexedSlices (UI's rows:
    X and Neg; Context's: Fea)."""
    lam = lam if lam > 0 else 0.0
    ls = loss(X, Fea, Neg, Wt, lam)
    _, G, _, _ = grad64(X, Fea, Neg, Wt)
    rows = {"UI": np.concatenate([np.asarray(X).reshape(-1), np.asarray(Neg).reshape(-1)]),
            "Context": np.asarray(Fea).reshape(-1)}
    new, ns = {}, {}
    for k in NAMES:
        var = np.asarray(Wt[k], F32)
        g = (G[k] + lam * var.astype(F64)).astype(F32)
        r = rows.get(k) if lam == 0 else None
        new[k], ns[k] = orc.tf_apply(optimizer, var, g, slots[k], lr, step, r)
    return ls, new, ns


# ---------------------------------------------------------------------------
# seeded catalog cases of tests/test_gpu_cars2.py (the CPU test holds cars2_ref
# itself — float32 in the reference's order against float64 — to the tie cap
# the GPU lists are held to)
# ---------------------------------------------------------------------------
MAX_TIES = 2
# name: (n_user, n_item, queries, Mc, D, seed)
CATALOG_CASES = {"dense": (50, 4082, 300, 11, 16, 11), "stream": (50, 20000, 130, 37, 64, 12)}
# UI at std 0.3; the context-side variables at 0.12, where the trilinear terms
# carry about a third of Σ|terms| instead of nearly all of it (asserted >= 10 %)
CATALOG_STD, CATALOG_TRI_STD = 0.3, 0.12


def catalog_case(name, bf16=False):
    """-> (weights, q [B, 2], n_user, n_item); ``bf16``: UI rounded to bf16,
    what a bf16 table holds."""
    from oracle.parity import bf16_round
    nu, ni, B, Mc, D, seed = CATALOG_CASES[name]
    Wt = weights(seed, nu + ni, Mc, D, CATALOG_TRI_STD)
    r = np.random.RandomState(seed + 1000)
    Wt["UI"] = r.normal(0.0, CATALOG_STD, Wt["UI"].shape).astype(F32)
    if bf16:
        Wt["UI"] = bf16_round(Wt["UI"])
    q = np.stack([r.randint(0, nu, B), r.randint(0, Mc, B)], 1).astype(np.int32)
    return Wt, q, nu, ni


def catalog_reference(Wt, q, n_user, n_item, dtype=F32):
    """catalog_scores for a large catalog -> [B, n_item]: the same graph with
    the contraction over the context factor (:182) as one matrix product
    instead of the [B, n, Dq, Dc] broadcast, which would not fit in memory."""
    q = np.asarray(q, np.int64)
    W = _cast(Wt, dtype)
    users, items, c = W["UI"][q[:, 0]], W["UI"][n_user:n_user + n_item], W["Context"][q[:, 1]]
    pik = _bilinear(users, W["W"], c)
    left = _left(items, W["Z"])                                        # n, Dq, Dc
    qjk = (left.reshape(-1, left.shape[2]) @ c.T).reshape(n_item, -1, len(q))   # n, Dq, B
    return (users @ items.T + (pik * W["A"]).sum(1, keepdims=True)
            + np.einsum("nqb,q->bn", qjk, W["B"]))


def catalog_mag(Wt, q, n_user, n_item):
    """Per query, the largest Σ|elementary products| over the catalog."""
    exact = exact_catalog(q, Wt, n_user)
    return np.array([exact(b, np.arange(n_item))[1].max() for b in range(len(q))])[:, None]
