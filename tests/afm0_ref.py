"""Float64 references of AFM without attention (include/hhfm.h "AFM without
attention"; Newcode/AFM.py:103-148 with self.attention false) — TEST
INFRASTRUCTURE ONLY — and the seeded inputs of tests/test_gpu_afm0.py.

    x_c  = ½[(Σ_f e_f,c)² − Σ_f e_f,c²]      d_c = x_c / keep · bin_c
    out  = Σ_c d_c·P_c + Σ_f w[x_f] + w0      loss = Σ_b (y_b − out_b)²/2

``out64`` / ``catalog64`` / ``grad64`` are float64; Σ|terms| follows
tests/test_gpu_kernels._fm_scale (½(s² + q) per column, here times |P_c|·m).
``grad64`` also returns, per parameter element, the magnitude of
tests/train_ref.py,

    mag = Σ_rows (|g_b| + S_b) · |factor|

the 1e-5 score bar propagated to first order: |factor| is the absolute-value
sum of what multiplies g_b in that element's gradient — |P_c|·m·(Σ_f|e_f| −
|e_f|) for dE, m·½(s² + q) for dP (x_c as the kernel forms it), 1 for dw / dw0.
``grad32`` is the fp32 oracle (float32, np.add.at), ``step`` the optimizer
replay with TF's sparse (E, w) / dense (w0, P) rules on oracle.fm_oracle.tf_apply,
``min_top_gap`` the catalog's tie margin.
"""
import functools

import numpy as np

from oracle import fm_oracle as orc
from oracle.parity import bf16_round

F32, F64 = np.float32, np.float64
NAMES = ("E", "w", "w0", "P")
BAR = 1e-5


def weights(seed, M, k):
    """E at std 0.3, w at std 0.1, w0 = 0.02 and P drawn N(1, 0.3) — not ones:
    at P ≡ 1 a kernel that drops P passes."""
    rng = np.random.default_rng(seed)
    return dict(E=rng.normal(0, 0.3, (M, k)).astype(F32), w=rng.normal(0, 0.1, M).astype(F32),
                w0=F32(0.02), P=rng.normal(1.0, 0.3, k).astype(F32))


def _m(mask, keep, shape):
    if mask is None:
        return np.ones(shape, F64)
    return np.asarray(mask, F64).reshape(shape) / F64(keep)


def out64(X, E, w, w0, P, mask=None, keep=1.0):
    """-> out [B], Σ|terms| [B] (float64); ``mask`` [B, k] of 0 / 1 with ``keep``."""
    X = np.asarray(X, np.int64)
    E, w, P = np.asarray(E, F64), np.asarray(w, F64).reshape(-1), np.asarray(P, F64).reshape(-1)
    e = E[X]
    s, q = e.sum(1), (e * e).sum(1)
    m = _m(mask, keep, s.shape)
    out = (0.5 * (s * s - q) * m * P).sum(1) + w[X].sum(1) + float(w0)
    S = (0.5 * (s * s + q) * m * np.abs(P)).sum(1) + np.abs(w[X]).sum(1) + abs(float(w0))
    return out, S


def loss64(X, y, E, w, w0, P, mask=None, keep=1.0):
    out, _ = out64(X, E, w, w0, P, mask, keep)
    r = np.asarray(y, F64).reshape(-1) - out
    return float(0.5 * (r * r).sum())


def catalog64(q, E, w, w0, P, n_user, n_item):
    """The library's catalog definition -> scores [B, n_item], Σ|terms|
    [B, n_item], cst [B]: out of the row with column 1 replaced by item i."""
    q = np.asarray(q, np.int64)
    E, w, P = np.asarray(E, F64), np.asarray(w, F64).reshape(-1), np.asarray(P, F64).reshape(-1)
    cols = [c for c in range(q.shape[1]) if c != 1]
    e = E[q[:, cols]]
    qs, qq = e.sum(1), (e * e).sum(1)
    wq = w[q[:, cols]]
    cst = (P * 0.5 * (qs * qs - qq)).sum(1) + wq.sum(1) + float(w0)
    acst = (np.abs(P) * 0.5 * (qs * qs + qq)).sum(1) + np.abs(wq).sum(1) + abs(float(w0))
    it = E[n_user:n_user + n_item]
    wi = w[n_user:n_user + n_item]
    score = (P * qs) @ it.T + wi[None, :] + cst[:, None]
    mag = (np.abs(P) * np.abs(e).sum(1)) @ np.abs(it).T + np.abs(wi)[None, :] + acst[:, None]
    return score, mag, cst


def min_top_gap(q, Wt, n_user, n_item, K):
    """The least gap between adjacent float64 scores among a query's K + 1 best,
    as a fraction of that query's largest Σ|terms|."""
    score, mag, _ = catalog64(q, Wt["E"], Wt["w"], Wt["w0"], Wt["P"], n_user, n_item)
    t = -np.sort(-score, axis=1)[:, :min(K + 1, n_item)]
    if t.shape[1] < 2:
        return np.inf
    return float(((t[:, :-1] - t[:, 1:]).min(1) / mag.max(1)).min())


def grad64(X, y, E, w, w0, P, mask=None, keep=1.0):
    """-> loss, {E, w, w0, P: gradient}, {…: magnitude} of Σ(y − out)²/2."""
    X = np.asarray(X, np.int64)
    y = np.asarray(y, F64).reshape(-1)
    E, w, P = np.asarray(E, F64), np.asarray(w, F64).reshape(-1), np.asarray(P, F64).reshape(-1)
    e = E[X]
    s, q = e.sum(1), (e * e).sum(1)
    m = _m(mask, keep, s.shape)
    out, S = out64(X, E, w, w0, P, mask, keep)
    g = out - y
    a = np.abs(g) + S
    ae = np.abs(e)
    sa = ae.sum(1)
    dE, mE = np.zeros_like(E), np.zeros_like(E)
    dw, mw = np.zeros_like(w), np.zeros_like(w)
    for f in range(X.shape[1]):
        np.add.at(dE, X[:, f], g[:, None] * P * m * (s - e[:, f]))
        np.add.at(mE, X[:, f], a[:, None] * np.abs(P) * m * (sa - ae[:, f]))
        np.add.at(dw, X[:, f], g)
        np.add.at(mw, X[:, f], a)
    dP = (g[:, None] * 0.5 * (s * s - q) * m).sum(0)
    mP = (a[:, None] * 0.5 * (s * s + q) * m).sum(0)
    G = dict(E=dE, w=dw, w0=g.sum(), P=dP)
    Mg = dict(E=mE, w=mw, w0=a.sum(), P=mP)
    return float(0.5 * (g * g).sum()), G, Mg


def grad32(X, y, E, w, w0, P, mask=None, keep=1.0):
    """The fp32 oracle: the same sums in float32 with np.add.at -> loss, {…}."""
    X = np.asarray(X, np.int64)
    y = np.asarray(y, F32).reshape(-1)
    E, w, P = np.asarray(E, F32), np.asarray(w, F32).reshape(-1), np.asarray(P, F32).reshape(-1)
    e = E[X]
    s, q = e.sum(1, dtype=F32), (e * e).sum(1, dtype=F32)
    m = np.ones(s.shape, F32) if mask is None else np.asarray(mask, F32).reshape(s.shape) / F32(keep)
    x = (F32(0.5) * (s * s - q) * m).astype(F32)
    out = ((x * P).sum(1, dtype=F32) + w[X].sum(1, dtype=F32) + F32(w0)).astype(F32)
    g = (out - y).astype(F32)
    dE, dw = np.zeros_like(E), np.zeros_like(w)
    for f in range(X.shape[1]):
        np.add.at(dE, X[:, f], (g[:, None] * P * m * (s - e[:, f])).astype(F32))
        np.add.at(dw, X[:, f], g)
    dP = np.zeros_like(P)
    for b in range(len(X)):
        dP += g[b] * x[b]
    loss = F32(0.5) * (g.astype(F64) ** 2).sum()
    return float(loss), dict(E=dE, w=dw, w0=g.sum(dtype=F32), P=dP)


def slots(o, Wt):
    """Initial slots per variable (TF: Adagrad 0.1, Momentum 0, Adam m = v = 0)."""
    def one(v):
        v = np.asarray(v, F32)
        return {"adagrad": np.full_like(v, 0.1), "momentum": np.zeros_like(v),
                "adam": np.zeros(2 * v.size, F32), "sgd": None}[o]
    return {n: one(Wt[n]) for n in NAMES}


def step(X, y, Wt, sl, lr, o, t, mask=None, keep=1.0):
    """One TF step replayed in float32 from ``Wt`` / ``sl``: E and w sparse
    (IndexedSlices: Momentum on the batch's rows only, Adam's sparse rule on
    every row), w0 and P dense -> loss, new weights, new slots, the gradients."""
    loss, G = grad32(X, y, Wt["E"], Wt["w"], Wt["w0"], Wt["P"], mask, keep)
    X = np.asarray(X, np.int64)
    rows = X if X.size else np.zeros(0, np.int64)
    W1, S1 = {}, {}
    W1["E"], S1["E"] = orc.tf_apply(o, Wt["E"], G["E"], sl["E"], lr, t, rows)
    W1["w"], S1["w"] = orc.tf_apply(o, Wt["w"], G["w"], sl["w"], lr, t, rows)
    w0n, S1["w0"] = orc.tf_apply(o, F32(Wt["w0"]), F32(G["w0"]), sl["w0"], lr, t)
    W1["w0"] = F32(w0n)
    W1["P"], S1["P"] = orc.tf_apply(o, Wt["P"], G["P"], sl["P"], lr, t)
    return loss, W1, S1, G


# ---------------------------------------------------------------------------
# seeded inputs of the gradient-parity cases (tests/test_gpu_afm0.py, and the
# CPU check of the fp32 oracle in tests/test_afm0_ref.py)
# ---------------------------------------------------------------------------
# name: (F, k, B, M, keep)
GRAD_CASES = {
    "F2_k4_B1": (2, 4, 1, 30, 1.0),
    "F5_k64_B300_M30": (5, 64, 300, 30, 1.0),
    "F16_k256_B65": (16, 256, 65, 400, 1.0),
    "F5_k20_B4097": (5, 20, 4097, 2000, 1.0),
    "F5_k64_B300_M30_keep": (5, 64, 300, 30, 0.5),
    "F16_k256_B65_keep": (16, 256, 65, 400, 0.5),
}


SEED = 2016 | 3 << 32     # the step's dropout seed in the keep < 1 cases


def case_mask(name):
    """-> (mask [B, k] or None, keep): dropout.h site 2 (n = k, r = the batch
    row) under SEED, from tests/dropout_ref.py's restatement — the GPU test
    reads the same back from hhfm_dropout_mask."""
    from tests import dropout_ref as dref
    F, k, B, M, keep = GRAD_CASES[name]
    if keep >= 1:
        return None, keep
    return dref.binary(SEED, dref.SITE_AFM_VEC, B, k, keep), keep


def grad_case(name):
    """-> X [B, F] int32, y (±1), weights.  Σ_c P_c·½(s² − q) has ~k·F²/2 terms
    of ±σ²: σ keeps |out| near 1 at every shape (tests/train_ref.fm_case)."""
    F, k, B, M, _ = GRAD_CASES[name]
    rng = np.random.default_rng(sorted(GRAD_CASES).index(name) + 500)
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    if B > 2:
        X[1, F - 1] = X[1, 0]          # one id twice in a row
        X[2, :] = X[2, F - 1]          # the same id in every column
    std = min(0.3, (k * F * F / 2.0) ** -0.25)
    Wt = dict(E=rng.normal(0, std, (M, k)).astype(F32), w=rng.normal(0, 0.3, M).astype(F32),
              w0=F32(0.02), P=rng.normal(1.0, 0.3, k).astype(F32))
    y = rng.choice([-1.0, 1.0], B).astype(F32)
    return X, y, Wt


# ---------------------------------------------------------------------------
# catalog cases (tests/test_gpu_afm0.py; their tie margins are asserted on the
# CPU in tests/test_afm0_ref.py)
# ---------------------------------------------------------------------------
CAT_ITEMS = (20, 64, 65, 1025, 4100, 70000)
CAT_B = (1, 8, 300)
CAT_K = (16, 64, 128)
CAT_NU, CAT_F, CAT_CTX, CAT_TOPK = 50, 5, 12, 20
CAT_POOL = 600          # candidate queries drawn per case; the first 300 clean ones are used
CAT_DUP = (5, 17, 900)  # item offsets given one table row and one w in the designed tie case


def _top(score, mag, K):
    """Per query the K + 1 best in tf.nn.top_k's order -> ids, scores, Σ|terms|."""
    n = score.shape[1]
    take = min(K + 1, n)
    if n > take:
        part = np.argpartition(-score, take - 1, axis=1)[:, :take]
    else:
        part = np.tile(np.arange(n), (len(score), 1))
    ps = np.take_along_axis(score, part, 1)
    order = np.lexsort((part, -ps), axis=1)
    ids = np.take_along_axis(part, order, 1)
    return ids.astype(np.int32), np.take_along_axis(score, ids, 1), np.take_along_axis(mag, ids, 1)


@functools.lru_cache(maxsize=None)
def catalog_case(n_item, k, bf16=False, dup=False):
    """One table per (n_item, k) and its 300 gap-clean queries; B = 1 and 8
    take the first rows.  A pool of CAT_POOL queries is drawn from the recorded
    seed and a query is kept when no two adjacent float64 scores among its
    top K + 1 lie within 1e-5 of its largest Σ|terms| (``dup``: exact zeros
    between the duplicated items aside) -> dict with the weights (bf16: the
    table already rounded), q [300, F], the rejected pool positions, and per
    query the float64 top K ids / scores / Σ|terms| and ``gap`` (the least
    adjacent gap / Σ|terms| among the kept queries)."""
    K = CAT_TOPK
    M = CAT_NU + n_item + CAT_CTX
    seed = 7000 + 13 * n_item % 1000 + k + (1 if bf16 else 0) + (2 if dup else 0)
    rng = np.random.default_rng(seed)
    std = min(0.3, (k * CAT_F * CAT_F / 2.0) ** -0.25)
    Wt = dict(E=rng.normal(0, std, (M, k)).astype(F32), w=rng.normal(0, 0.1, M).astype(F32),
              w0=F32(0.02), P=rng.normal(1.0, 0.3, k).astype(F32))
    if bf16:
        Wt["E"] = bf16_round(Wt["E"])
    if dup:
        a = CAT_NU + np.asarray(CAT_DUP)
        Wt["E"][a] = Wt["E"][a[0]]
        Wt["w"][a] = F32(15.0)         # above every other score: the three lead each list
    cols = [rng.integers(0, CAT_NU, CAT_POOL), rng.integers(CAT_NU, CAT_NU + n_item, CAT_POOL)]
    cols += [rng.integers(CAT_NU + n_item, M, CAT_POOL) for _ in range(CAT_F - 2)]
    pool = np.stack(cols, 1).astype(np.int32)
    score, mag, _ = catalog64(pool, Wt["E"], Wt["w"], Wt["w0"], Wt["P"], CAT_NU, n_item)
    ids, ts, tm = _top(score, mag, K)
    gaps = ts[:, :-1] - ts[:, 1:]
    if dup:
        gaps = np.where(gaps == 0, np.inf, gaps)
    rel = gaps.min(1) / mag.max(1)
    del score, mag
    clean = np.flatnonzero(rel > BAR)
    assert len(clean) >= max(CAT_B), (n_item, k, len(clean))
    keep = clean[:max(CAT_B)]
    rejected = [int(i) for i in range(int(keep[-1]) + 1) if i not in set(keep.tolist())]
    return dict(Wt=Wt, n_user=CAT_NU, n_item=n_item, K=K, seed=seed, q=pool[keep],
                rejected=rejected, ids=ids[keep, :K], score=ts[keep, :K], mag=tm[keep, :K],
                gap=float(rel[keep].min()))
