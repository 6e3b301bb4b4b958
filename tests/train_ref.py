"""Float64 references of the FM and HHFM training gradients — TEST
INFRASTRUCTURE ONLY — and the seeded inputs of tests/test_gpu_train_grad.py.

``fm_grad64`` / ``hhfm_grad64`` return, for every parameter element, the
gradient of the reference's loss (FM.py:123-126, OurModel7.py:171-184 at
λ = 0) and its magnitude

    mag = Σ_rows (|g_b| + S_b) · |factor|

g_b = dL/d(out) of row b, S_b the forward score's Σ|terms| (what
tests/test_gpu_kernels._fm_scale / _hhfm_scale compute), |factor| the
absolute-value sum of what multiplies g_b in that element's gradient.  A
forward score that is off by the project's bar (1e-5 · S_b) moves g_b by as
much, so 1e-5 · mag is that same bar propagated to first order — not a new
tolerance.  Both are pinned against central finite differences of a float64
loss in tests/test_train_ref.py.

reduce_max's gradient is split between tied maxima (TF _MaxGrad).  Which
negatives tie is an input of ``hhfm_grad64`` (a boolean mask), so float64
never re-decides what fp32 saw as equal; ``tie_mask`` derives it from the
table rows' bits and ``hhfm_grad64`` reports how far the best untied
negative lies below the maximum.
"""
import numpy as np

F64 = np.float64


def fm_grad64(X, y, E, w, w0):
    """-> loss, (dE, dw, dw0), (magE, magw, magw0) of Σ(y − out)²/2."""
    X = np.asarray(X, np.int64)
    y = np.asarray(y, F64).reshape(-1)
    E = np.asarray(E, F64)
    w = np.asarray(w, F64).reshape(-1)
    w0 = float(w0)
    e = E[X]                                            # [B, F, k]
    s = e.sum(1)
    q = (e * e).sum(1)
    wx = w[X]
    out = (0.5 * (s * s - q)).sum(1) + wx.sum(1) + w0
    S = (0.5 * (s * s + q)).sum(1) + np.abs(wx).sum(1) + abs(w0)
    g = out - y
    a = np.abs(g) + S
    ae = np.abs(e)
    sa = ae.sum(1)
    dE, mE = np.zeros_like(E), np.zeros_like(E)
    dw, mw = np.zeros_like(w), np.zeros_like(w)
    for f in range(X.shape[1]):
        np.add.at(dE, X[:, f], g[:, None] * (s - e[:, f]))      # ∂out/∂e_f = Σe − e_f
        np.add.at(mE, X[:, f], a[:, None] * (sa - ae[:, f]))
        np.add.at(dw, X[:, f], g)
        np.add.at(mw, X[:, f], a)
    return 0.5 * (g * g).sum(), (dE, dw, g.sum()), (mE, mw, a.sum())


def _field_cols(ctx, tim):
    cols = []
    for lo, hi in (ctx, tim):
        if hi > lo:
            cols += list(range(lo, hi))
    return cols


def tie_mask(X, Neg, E, ctx, tim):
    """[B, NG] mask of the negatives whose table row is bit-identical to the
    row of the float64 maximum (the same id twice, or two ids with equal rows)."""
    X, Neg = np.asarray(X, np.int64), np.asarray(Neg, np.int64)
    E32 = np.ascontiguousarray(E, np.float32)
    E = E32.astype(F64)
    h = E[X[:, 0]] + E[X[:, _field_cols(ctx, tim)]].sum(1)
    best = np.einsum("bc,bjc->bj", h, E[Neg]).argmax(1)
    top = E32[Neg[np.arange(len(Neg)), best]]
    return (E32[Neg].view(np.uint32) == top.view(np.uint32)[:, None, :]).all(2)


def hhfm_grad64(X, Neg, E, ctx, tim, ties):
    """-> loss, dE, magE, info of −Σ log σ(pos − max_j neg_j), h = u + Σctx +
    Σtime over the column ranges ``ctx`` / ``tim`` (empty when hi <= lo).
    ``ties`` [B, NG] marks the negatives that share the maximum.  info: z per
    row, and ``margin`` = the least (max − best untied negative) / S_b."""
    X, Neg = np.asarray(X, np.int64), np.asarray(Neg, np.int64)
    E = np.asarray(E, F64)
    ties = np.asarray(ties, bool)
    cols = [0] + _field_cols(ctx, tim)
    h = E[X[:, cols]].sum(1)
    it = E[X[:, 1]]
    n = E[Neg]                                          # [B, NG, k]
    pos = (h * it).sum(1)
    neg = np.einsum("bc,bjc->bj", h, n)
    mx = neg.max(1)
    assert ties.any(1).all() and np.all(neg[ties] == np.repeat(mx, ties.sum(1)))
    nt = ties.sum(1)
    wt = ties / nt[:, None]
    ah = np.abs(h)
    fh = np.abs(E[X[:, cols]]).sum(1)                   # |factor| of the item / negative terms
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
    for c in cols:
        np.add.at(dE, X[:, c], dh)
        np.add.at(mE, X[:, c], mh)
    return -np.log(sg).sum(), dE, mE, dict(z=z, margin=float((gap / S).min()), nt=nt)


def ratio(delta, before, after, grad, mag):
    """Largest |Δ − grad64| / (1e-5 · mag + 2^-23 · max(|before|, |after|)):
    the bound of tests/test_gpu_train_grad.py (second term: the rounding of
    the subtraction Δ = before − after).  0/0 (an untouched element) is 0."""
    delta, grad, mag = (np.asarray(x, F64).reshape(-1) for x in (delta, grad, mag))
    big = np.maximum(np.abs(np.asarray(before, F64)), np.abs(np.asarray(after, F64))).reshape(-1)
    err = np.abs(delta - grad)
    bound = 1e-5 * mag + 2.0 ** -23 * big
    r = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    r[(bound == 0) & (err > 0)] = np.inf
    return float(r.max())


# ---------------------------------------------------------------------------
# seeded inputs (shared by the GPU tests and the CPU check of the fp32 oracle)
# ---------------------------------------------------------------------------
# name: (k, F, B, M, hot user, planted rows)
FM_CASES = {
    "k4": (4, 5, 257, 50, False, True),
    "k20": (20, 5, 257, 50, False, True),
    "k64": (64, 5, 257, 50, False, True),
    "k68": (68, 5, 257, 50, False, True),
    "k128": (128, 5, 257, 50, False, True),
    "k200": (200, 5, 257, 50, False, True),
    "F1": (20, 1, 257, 50, False, False),
    "F2": (20, 2, 257, 50, False, True),
    "F12": (20, 12, 257, 50, False, True),
    "B1_hot": (20, 5, 1, 50, True, False),
    "B63_hot": (20, 5, 63, 50, True, True),
    "B2049_hot": (20, 5, 2049, 50, True, True),
    "B32773": (4, 2, 32773, 2000, False, False),
    "F65": (4, 65, 3, 200, False, False),
}


def fm_case(name):
    """-> X [B, F] int32, y, E, w, w0.  Planted: row 1 holds one id twice,
    row 2 the same id in every column; ``hot``: every row shares user 0."""
    k, F, B, M, hot, plant = FM_CASES[name]
    rng = np.random.default_rng(sorted(FM_CASES).index(name) + 100)
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    if hot:
        X[:, 0] = 0
    if plant:
        X[1, F - 1] = X[1, 0]
        X[2, :] = X[2, F - 1]
    # Σ_c ½(s² − q) has ~k·F²/2 terms of ±σ²: σ keeps |out| near 1 at every k
    std = min(0.3, (k * F * F / 2.0) ** -0.25)
    E = rng.normal(0, std, (M, k)).astype(np.float32)
    w = rng.normal(0, 0.3, M).astype(np.float32)
    y = rng.integers(0, 2, B).astype(np.float32)
    return X, y, E, w, np.float32(0.02)


# name: (layout, NG, k, B); layout -> (context columns, time columns)
LAYOUTS = {"ctx": (3, 0), "time": (0, 3), "both": (3, 2), "none": (0, 0)}
HHFM_CASES = {
    "ctx_ng10_k8": ("ctx", 10, 8, 257),
    "time_ng10_k64": ("time", 10, 64, 257),
    "both_ng10_k100": ("both", 10, 100, 257),
    "none_ng10_k128": ("none", 10, 128, 257),
    "ctx_ng1_k64": ("ctx", 1, 64, 257),
    "both_ng2_k8": ("both", 2, 8, 257),
    "time_ng16_k100": ("time", 16, 100, 257),
    "none_ng16_k8": ("none", 16, 8, 257),
    "both_ng16_k128_b1": ("both", 16, 128, 1),
    "none_ng1_k8_b1": ("none", 1, 8, 1),
}
NU, NI, NC = 40, 120, 5      # users, items, values per context column


def hhfm_case(name):
    """-> X [B, ncols] int32, Neg [B, NG] int32, E, ctx range, time range,
    ties.  Rows [user, item, ctx..., time...]; time columns hold item ids
    (OurModel7's jiaju layout).  Planted when B > 4:
      row 0  the maximum negative's id a second time        (NG >= 2)
      row 1  all NG negatives the same id
      row 2  a negative equal to the positive item, the others below it (z = 0)
      row 3  two negative ids whose table rows are bit-identical and the
             maximum: the gradient is split across two rows   (NG >= 2)
      row 4  a context / time id equal to the user id         (layout != none)
    """
    layout, NG, k, B = HHFM_CASES[name]
    fd, td = LAYOUTS[layout]
    rng = np.random.default_rng(sorted(HHFM_CASES).index(name) + 200)
    M = NU + NI + fd * NC
    cols = [rng.integers(0, NU, B), rng.integers(NU, NU + NI, B)]
    for f in range(fd):
        cols.append(rng.integers(NU + NI + f * NC, NU + NI + (f + 1) * NC, B))
    for _ in range(td):
        cols.append(rng.integers(NU, NU + NI, B))
    X = np.stack(cols, 1).astype(np.int32)
    Neg = rng.integers(NU, NU + NI, (B, NG)).astype(np.int32)
    # h·i has k terms of (1 + fd + td)·σ² each: σ keeps |pos − max neg| <= 4
    std = (0.3 / (k * (1 + fd + td)) ** 0.5) ** 0.5
    E = rng.normal(0, std, (M, k)).astype(np.float32)
    ctx = (2, 2 + fd) if fd else (0, 0)
    tim = (2 + fd, 2 + fd + td) if td else (0, 0)
    if B > 4:
        if fd + td:
            X[4, 2] = X[4, 0]
        items = np.arange(NU, NU + NI)

        def scores(r):      # h·item of every item (h does not depend on the row's item)
            E64 = E.astype(F64)
            return E64[items] @ E64[X[r, [0] + _field_cols(ctx, tim)]].sum(0)

        def below(r, top, n):
            s = scores(r)
            return rng.choice(items[s < s[top - NU] - 0.05], n)

        if NG >= 2:
            # the best item that no column of row 3 holds, and a twin of it
            free = items[~np.isin(items, X[3])]
            a = free[scores(3)[free - NU].argmax()]
            b = free[free != a][0]
            E[b] = E[a]
            Neg[3, 0], Neg[3, 1] = a, b
            Neg[3, 2:] = below(3, a, NG - 2)
            j = scores(0)[Neg[0] - NU].argmax()
            Neg[0, (j + 1) % NG] = Neg[0, j]
        Neg[1, :] = Neg[1, 0]
        X[2, 1] = items[scores(2).argmax()]
        Neg[2, 0] = X[2, 1]
        Neg[2, 1:] = below(2, X[2, 1], NG - 1)
    return X, Neg, E, ctx, tim, tie_mask(X, Neg, E, ctx, tim)
