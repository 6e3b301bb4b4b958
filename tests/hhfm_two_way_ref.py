"""Two-way HHFM — TEST INFRASTRUCTURE ONLY.

A numpy restatement of the reference graph with its three commented-out
additions (OurModel7.py:124, :141, :168 "#2-way stack hybrid feature") put
back, in the arithmetic include/hhfm.h "Two-way pooling" fixes.  Built on
tests/hhfm_pool_ref.py (the one-way pools):

  ``mix``                                a pool's P1, P2 and P1 + P2 from its rows
  ``stack2``                             H1, H2 from the stack members
  ``hybrid2``                            h [B, k] in fp32 (or any dtype)
  ``score_rows2`` / ``catalog_scores2``  the fp32 forward
  ``exact_rows2`` / ``exact_catalog2``   its float64 value and Σ|terms| (a product's
                                         magnitude is the product of magnitudes)
  ``grad64``                             the float64 loss and gradient with every max
                                         selection fixed from the fp32 values
  ``loss64``                             the float64 loss, nothing fixed
  ``train_step2``                        one fp32 training step
  ``TWO_WAY_CASES`` / ``two_way_case``   seeded inputs with planted rows

Pairs are (i, j), i < j, i outer — the reference's loop order (:115-117,
:132-134, :159-161).  With every selection fixed the graph is a polynomial of
degree 4 in the rows: P1 = Σ a_i r_i, P2 = Σ b_ij r_i r_j, mix = P1 + P2,
H1 = Σ c_m s_m, H2 = Σ d_mn s_m s_n over the members s = (u, mix_c, mix_t).
"""
import numpy as np

from oracle import fm_oracle as orc
from tests import hhfm_pool_ref as pr
from tests import train_ref as tr

F32, F64 = np.float32, np.float64
SUM, MAX, MEAN = pr.SUM, pr.MAX, pr.MEAN
modes_of = pr.modes_of
_cols = pr._cols


def pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def _products(vals):
    """vals [B, n, k] -> [B, n(n-1)/2, k]: one rounded multiply each."""
    return np.stack([vals[:, i] * vals[:, j] for i, j in pairs(vals.shape[1])], 1)


def mix(rows, m1, m2):
    """rows [B, n, k], n >= 2 -> P1, P2, P1 + P2."""
    assert rows.shape[1] >= 2, "a present pool needs two rows"
    p1 = pr._pool(rows, m1)
    p2 = pr._pool(_products(rows), m2)
    return p1, p2, p1 + p2


def stack2(members, mf, mf2):
    """members: list of [B, k], at least two -> H1, H2."""
    assert len(members) >= 2, "the stack needs two members"
    s = np.stack(members, 1)
    return pr._pool(s, mf), pr._pool(_products(s), mf2)


def hybrid2(E, X, ctx, tim, pooling, pooling2, ucol=0, dtype=F32, parts=False):
    """h [B, k] = H1 + H2.  ``parts``: also a dict of the intermediate values
    (ctx / time: (P1, P2, mix); members; H1; H2)."""
    mc, mt, mf = modes_of(pooling)
    mc2, mt2, mf2 = modes_of(pooling2)
    E = np.asarray(E, dtype)
    X = np.asarray(X, np.int64)
    members = [E[X[:, ucol]]]
    info = {}
    if _cols(ctx):
        info["ctx"] = mix(E[X[:, _cols(ctx)]], mc, mc2)
        members.append(info["ctx"][2])
    if _cols(tim):
        info["time"] = mix(E[X[:, _cols(tim)]], mt, mt2)
        members.append(info["time"][2])
    h1, h2 = stack2(members, mf, mf2)
    h = h1 + h2
    info.update(members=members, H1=h1, H2=h2)
    return (h, info) if parts else h


def score_rows2(X, E, ctx, tim, pooling, pooling2, ucol=0, icol=1):
    h = hybrid2(E, X, ctx, tim, pooling, pooling2, ucol)
    it = np.asarray(E, F32)[np.asarray(X, np.int64)[:, icol]]
    return (h * it).sum(1, dtype=F32)


def catalog_scores2(A, E, n_user, n_item, ctx, tim, pooling, pooling2):
    h = hybrid2(E, A, ctx, tim, pooling, pooling2)
    item = np.asarray(E, F32)[n_user:n_user + n_item]
    return (h[:, None, :] * item[None, :, :]).sum(2, dtype=F32)


def _abs_hybrid2(E64, X, ctx, tim, pooling, pooling2, ucol=0):
    return hybrid2(np.abs(E64), X, ctx, tim, pooling, pooling2, ucol, F64)


def pair_share(X, E, ctx, tim, pooling, pooling2, ucol=0):
    """Per row: the part of Σ_e |terms of h_e| that the pair terms (P2 of
    either pool, inside H1 and H2, and H2 itself) carry: 1 − Σ|one-way h| /
    Σ|two-way h| over magnitudes."""
    E64 = np.abs(np.asarray(E, F32).astype(F64))
    two = _abs_hybrid2(E64, X, ctx, tim, pooling, pooling2, ucol).sum(1)
    one = pr.hybrid(E64, X, ctx, tim, pooling, ucol, F64).sum(1)
    return 1.0 - one / two


def exact_rows2(X, E, ctx, tim, pooling, pooling2, ucol=0, icol=1):
    """-> float64 score and Σ|terms| per row, from the fp32 table."""
    E64 = np.asarray(E, F32).astype(F64)
    it = E64[np.asarray(X, np.int64)[:, icol]]
    h = hybrid2(E64, X, ctx, tim, pooling, pooling2, ucol, F64)
    ah = _abs_hybrid2(E64, X, ctx, tim, pooling, pooling2, ucol)
    return (h * it).sum(1), (ah * np.abs(it)).sum(1)


def exact_catalog2(A, E, n_user, ctx, tim, pooling, pooling2):
    E64 = np.asarray(E, F32).astype(F64)
    h = hybrid2(E64, A, ctx, tim, pooling, pooling2, dtype=F64)
    ah = _abs_hybrid2(E64, A, ctx, tim, pooling, pooling2)

    def exact(b, ids):
        it = E64[n_user + np.asarray(ids, np.int64)]
        return it @ h[b], np.abs(it) @ ah[b]
    return exact


# ---------------------------------------------------------------------------
# gradient
# ---------------------------------------------------------------------------
class _Fixed:
    """Every selection of the graph taken from the fp32 forward (pool_weights'
    rule): float64 weights of each pool towards its values."""

    def __init__(self, X, E, ctx, tim, pooling, pooling2):
        mc, mt, mf = modes_of(pooling)
        mc2, mt2, mf2 = modes_of(pooling2)
        E32 = np.asarray(E, F32)
        self.X = np.asarray(X, np.int64)
        _, info = hybrid2(E32, self.X, ctx, tim, pooling, pooling2, parts=True)
        self.pools = []                                   # (cols, W1, W2)
        for rng_, key, m1, m2 in ((ctx, "ctx", mc, mc2), (tim, "time", mt, mt2)):
            if _cols(rng_):
                rows = E32[self.X[:, _cols(rng_)]]
                self.pools.append((_cols(rng_), pr._sel(rows, m1), pr._sel(_products(rows), m2)))
        s = np.stack(info["members"], 1)
        self.WF1, self.WF2 = pr._sel(s, mf), pr._sel(_products(s), mf2)

    def forward(self, E):
        """E float64 (or magnitudes) -> h, members, pool rows."""
        members, rows = [E[self.X[:, 0]]], []
        for cols, W1, W2 in self.pools:
            r = E[self.X[:, cols]]
            rows.append(r)
            members.append((W1 * r).sum(1) + (W2 * _products(r)).sum(1))
        s = np.stack(members, 1)
        h = (self.WF1 * s).sum(1) + (self.WF2 * _products(s)).sum(1)
        return h, s, rows

    def backward(self, dh, s, rows, out, absolute=False):
        """Adds d loss / d E rows (or, ``absolute``, their magnitudes from
        magnitude inputs) for dh [B, k] into ``out``."""
        n = s.shape[1]
        ds = [self.WF1[:, m] * dh for m in range(n)]
        for p, (i, j) in enumerate(pairs(n)):
            ds[i] = ds[i] + self.WF2[:, p] * dh * s[:, j]
            ds[j] = ds[j] + self.WF2[:, p] * dh * s[:, i]
        np.add.at(out, self.X[:, 0], ds[0])
        for m, ((cols, W1, W2), r) in enumerate(zip(self.pools, rows), 1):
            dr = [W1[:, i] * ds[m] for i in range(len(cols))]
            for p, (i, j) in enumerate(pairs(len(cols))):
                dr[i] = dr[i] + W2[:, p] * ds[m] * r[:, j]
                dr[j] = dr[j] + W2[:, p] * ds[m] * r[:, i]
            for i, c in enumerate(cols):
                np.add.at(out, self.X[:, c], dr[i])


def tie_mask2(X, Neg, E, ctx, tim, pooling, pooling2):
    """pr.tie_mask with the two-way h."""
    X, Neg = np.asarray(X, np.int64), np.asarray(Neg, np.int64)
    E32 = np.ascontiguousarray(E, F32)
    h = _Fixed(X, E32, ctx, tim, pooling, pooling2).forward(E32.astype(F64))[0]
    best = np.einsum("bc,bjc->bj", h, E32.astype(F64)[Neg]).argmax(1)
    top = E32[Neg[np.arange(len(Neg)), best]]
    return (E32[Neg].view(np.uint32) == top.view(np.uint32)[:, None, :]).all(2)


def grad64(X, Neg, E, ctx, tim, ties, pooling, pooling2):
    """pr.hhfm_pool_grad64 for the two-way h -> loss, dE, magE, info."""
    X, Neg = np.asarray(X, np.int64), np.asarray(Neg, np.int64)
    fx = _Fixed(X, E, ctx, tim, pooling, pooling2)
    E = np.asarray(E, F64)
    A = np.abs(E)
    ties = np.asarray(ties, bool)
    h, s, rows = fx.forward(E)
    fh, sa, rowsa = fx.forward(A)                           # Σ|terms| of h
    it, n = E[X[:, 1]], E[Neg]
    pos = (h * it).sum(1)
    neg = np.einsum("bc,bjc->bj", h, n)
    mx = neg.max(1)
    assert ties.any(1).all() and np.all(neg[ties] == np.repeat(mx, ties.sum(1)))
    nt = ties.sum(1)
    wt = ties / nt[:, None]
    S = (fh * np.abs(it)).sum(1) + (np.einsum("bc,bjc->bj", fh, np.abs(n)) * wt).sum(1)
    gap = np.where(ties, np.inf, mx[:, None] - neg).min(1)
    z = pos - mx
    sg = 1.0 / (1.0 + np.exp(-z))
    g = sg - 1.0
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
    fx.backward(dh, s, rows, dE)
    fx.backward(mh, sa, rowsa, mE)
    return -np.log(sg).sum(), dE, mE, dict(z=z, margin=float((gap / S).min()), nt=nt)


def loss64(X, Neg, E, ctx, tim, pooling, pooling2):
    """The float64 loss of the two-way graph itself, nothing fixed."""
    X, Neg = np.asarray(X, np.int64), np.asarray(Neg, np.int64)
    E = np.asarray(E, F64)
    h = hybrid2(E, X, ctx, tim, pooling, pooling2, dtype=F64)
    pos = (h * E[X[:, 1]]).sum(1)
    mx = np.einsum("bc,bjc->bj", h, E[Neg]).max(1)
    return -np.log(1.0 / (1.0 + np.exp(-(pos - mx)))).sum()


def train_step2(X, Neg, E, slot, lr, lam, ctx, tim, pooling, pooling2, optimizer="adagrad",
                step=1, grad_only=False):
    """pr.train_step with the two-way h: the fp32 forward, the backward through
    the fixed selections in fp32."""
    X, Neg = np.asarray(X, np.int64), np.asarray(Neg, np.int64)
    E = np.asarray(E, F32)
    fx = _Fixed(X, E, ctx, tim, pooling, pooling2)
    fx.WF1, fx.WF2 = fx.WF1.astype(F32), fx.WF2.astype(F32)
    fx.pools = [(c, a.astype(F32), b.astype(F32)) for c, a, b in fx.pools]
    h = hybrid2(E, X, ctx, tim, pooling, pooling2)
    _, s, rows = fx.forward(E)
    it = E[X[:, 1]]
    pos = (h * it).sum(1, dtype=F32)
    neg = (h[:, None, :] * E[Neg]).sum(2, dtype=F32)
    mx = neg.max(1)
    sg = (1.0 / (1.0 + np.exp(-(pos - mx)))).astype(F32)
    loss = F32(-np.sum(np.log(sg), dtype=F64) + lam * np.sum(E.astype(F64) ** 2) / 2)
    g = sg - F32(1)
    ind = (neg == mx[:, None]).astype(F32)
    ind /= ind.sum(1, keepdims=True)
    dh = g[:, None] * (it - (ind[:, :, None] * E[Neg]).sum(1))
    dE = np.zeros_like(E)
    np.add.at(dE, X[:, 1], g[:, None] * h)
    for j in range(Neg.shape[1]):
        np.add.at(dE, Neg[:, j], -(g * ind[:, j])[:, None] * h)
    fx.backward(dh, s, rows, dE)
    if grad_only:
        return loss, dE
    dE += F32(lam) * E
    touched = np.concatenate([X.reshape(-1), Neg.reshape(-1)]) if lam == 0 else None
    E, slot = orc.tf_apply(optimizer, E, dE, slot, lr, step, touched)
    return loss, E, slot


# ---------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------
MMM, EEE, SSS = ("max",) * 3, ("mean",) * 3, ("sum",) * 3
# five sextuples: each mode at each of the six pools at least once
SEXTUPLES = [(MMM, MMM), (EEE, EEE), (SSS, SSS), (("max", "mean", "sum"), ("mean", "sum", "max")),
             (("sum", "max", "mean"), ("max", "mean", "sum"))]
# name: (case of train_ref.HHFM_CASES the rows derive from, k, pooling, pooling2)
TWO_WAY_CASES = {
    "ctx_ng10_k4_max": ("ctx_ng10_k8", 4, MMM, MMM),
    "ctx_ng1_k64_mean": ("ctx_ng1_k64", 64, EEE, EEE),
    "ctx_ng10_k128_sum": ("ctx_ng10_k8", 128, SSS, SSS),
    "time_ng10_k64_max": ("time_ng10_k64", 64, MMM, MMM),
    "time_ng16_k200_mixed": ("time_ng16_k100", 200, ("sum", "mean", "max"), ("max", "sum", "mean")),
    "both_ng10_k200_max": ("both_ng10_k100", 200, MMM, MMM),
    "both_ng10_k64_mixed": ("both_ng10_k100", 64, ("max", "mean", "sum"), ("mean", "sum", "max")),
    "both_ng2_k4_mixed": ("both_ng2_k8", 4, ("sum", "max", "mean"), ("max", "mean", "sum")),
    "both_ng16_k128_b1_mean": ("both_ng16_k128_b1", 128, EEE, EEE),
}


def _lead(vals, mag, R):
    """vals [B, n, k] fp32 values of one max pool, mag [B, k] their Σ|terms|:
    per row, the largest is bit-equal to the runner-up (a tie fp32 and float64
    both see) or leads it by more than 4·R·2⁻²⁴·mag at every element."""
    if vals.shape[1] < 2:
        return np.ones(len(vals), bool)
    m = np.sort(vals.astype(F64), 1)
    lead = m[:, -1] - m[:, -2]
    return ((lead == 0) | (lead > 4.0 * R * 2.0 ** -24 * mag)).all(1)


def admissible(X, E, ctx, tim, pooling, pooling2):
    """Per row: every max pool of either level selects alike in fp32 and in
    float64 (pr._lead_ok's rule, extended by the products).  R counts the fp32
    roundings on the path to the pool's values: 1 for a product of table rows
    (its pool of table rows itself has none and always passes), and for the
    stack n + npairs + 2 per mix (its sums, the division, the add) plus one for
    a member product."""
    mc, mt, mf = modes_of(pooling)
    mc2, mt2, mf2 = modes_of(pooling2)
    E32 = np.asarray(E, F32)
    X = np.asarray(X, np.int64)
    A = np.abs(E32.astype(F64))
    ok = np.ones(len(X), bool)
    _, info = hybrid2(E32, X, ctx, tim, pooling, pooling2, parts=True)
    _, ainfo = hybrid2(A, X, ctx, tim, pooling, pooling2, dtype=F64, parts=True)
    R = 0
    for rng_, m2 in ((ctx, mc2), (tim, mt2)):
        if _cols(rng_):
            n = len(_cols(rng_))
            R = max(R, n + n * (n - 1) // 2 + 2)
            if m2 == MAX:
                ok &= _lead(_products(E32[X[:, _cols(rng_)]]),
                            _products(A[X[:, _cols(rng_)]]).max(1), 1)
    s, sa = np.stack(info["members"], 1), np.stack(ainfo["members"], 1)
    if mf == MAX:
        ok &= _lead(s, sa.sum(1), R)
    if mf2 == MAX:
        ok &= _lead(_products(s), _products(sa).sum(1), 2 * R + 1)
    return ok


def two_way_case(name):
    """-> X, Neg, E, ctx, tim, ties, pooling, pooling2, info.  pr.hhfm_pool_case's
    construction (train_ref.hhfm_case's rows with its planted rows 0..4 — row 3
    a reduce_max tie among the negatives, row 4 a field id equal to the user
    id — then row 5 one id twice in a pool, row 6 two ids with bit-identical
    rows, row 7 all-negative values at element 0) on a table whose std makes
    the pair terms matter; the negatives of rows 0 .. 3 are planted again under
    the two-way h (``plant``), so that row 3's twins are the maximum here too.
    Rows that fail ``admissible``, |z| <= 4 or the BPR
    margin get a fresh user (and, failing that, fresh fields) from the case's
    own stream until they pass; info["redrawn"] counts them."""
    base, k, pooling, pooling2 = TWO_WAY_CASES[name]
    layout, NG, _, B = tr.HHFM_CASES[base]
    fd, td = tr.LAYOUTS[layout]
    X, Neg, E0, ctx, tim, _ = tr.hhfm_case(base)
    rng = np.random.default_rng(sorted(TWO_WAY_CASES).index(name) + 1900)
    M = E0.shape[0]
    E = rng.normal(0, (0.5 / k) ** 0.25, (M, k)).astype(F32) * F32(0.7)
    f = _cols(ctx) + _cols(tim)
    items = np.arange(tr.NU, tr.NU + tr.NI)
    if B > 8:
        X[5, f[1]] = X[5, f[0]]
        if X[6, f[1]] == X[6, f[0]]:
            X[6, f[1]] = X[6, f[0]] + 1
        a, b = X[6, f[0]], X[6, f[1]]
        neg = list(X[7, f]) + ([a] if b in X[7, f] else [])
        E[neg, 0] = -np.abs(E[neg, 0]) - F32(0.01)
        E[b] = E[a]

    def scores(r):          # float64 h·item of every item under the two-way h
        E64 = E.astype(F64)
        return E64[items] @ hybrid2(E64, X[r:r + 1], ctx, tim, pooling, pooling2, dtype=F64)[0]

    def low(r, n):          # n items from the lower-scoring half
        return rng.choice(items[np.argsort(scores(r))[:tr.NI // 2]], n)

    twin = None
    if B > 4 and NG >= 2:   # train_ref.hhfm_case's row 3 under this h: the best free item and a twin
        free = items[~np.isin(items, X[[3, 5, 6, 7]] if B > 8 else X[3])]
        a = free[scores(3)[free - tr.NU].argmax()]
        b = free[free != a][0]
        E[b] = E[a]
        twin = (a, b)

    def plant(r):           # the negatives of train_ref.hhfm_case's rows 0 .. 3
        if B <= 4:
            return
        if r == 0 and NG >= 2:
            j = scores(0)[Neg[0] - tr.NU].argmax()
            Neg[0, (j + 1) % NG] = Neg[0, j]
        elif r == 1:
            Neg[1, :] = Neg[1, 0]
        elif r == 2:
            X[2, 1] = items[scores(2).argmax()]
            Neg[2, 0] = X[2, 1]
            Neg[2, 1:] = low(2, NG - 1)
        elif r == 3 and twin:
            Neg[3, :2] = twin
            Neg[3, 2:] = low(3, NG - 2)

    def row_ok(r):
        sl = slice(r, r + 1)
        if not admissible(X[sl], E, ctx, tim, pooling, pooling2)[0]:
            return False
        t = tie_mask2(X[sl], Neg[sl], E, ctx, tim, pooling, pooling2)
        if B > 4 and r == 3 and twin and not t[0, :2].all():
            return False                    # the twins must be the maximum
        info = grad64(X[sl], Neg[sl], E, ctx, tim, t, pooling, pooling2)[3]
        return abs(info["z"][0]) <= 4 and info["margin"] > 1e-5

    redrawn = 0
    for r in range(B):
        plant(r)
        if row_ok(r):
            continue
        redrawn += 1
        for t in range(200):
            X[r, 0] = rng.integers(0, tr.NU)
            if r == 4:
                X[r, f[0]] = X[r, 0]
            elif t >= 10 and r > 7:        # a near-tie inside a pool: fields of another row
                X[r, f] = X[rng.integers(8, B), f]
            plant(r)
            if row_ok(r):
                break
        else:
            raise AssertionError(f"{name}: row {r} finds no admissible user")
    ties = tie_mask2(X, Neg, E, ctx, tim, pooling, pooling2)
    return X, Neg, E, ctx, tim, ties, pooling, pooling2, dict(redrawn=redrawn, rows=B)
