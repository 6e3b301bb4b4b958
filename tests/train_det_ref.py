"""The orders of the deterministic training steps (include/hhfm.h
"Deterministic training steps"), restated in numpy float32 — TEST
INFRASTRUCTURE ONLY — and two inputs whose every contribution is exact in
fp32, so the ordered sums are known answers to the bit.

* ``segment_scatter``: dE[id] = the fp32 sum of the id's contributions in
  ascending occurrence index, started from the first one.
* ``scalar_sum``: 256 partials, partial t = rows t, t + 256, … ascending from
  0, then the partials in ascending t from 0 (float32 for g, float64 for the
  loss, which is rounded to float32 once: ``loss_sum``).

FM known answer (``fm_known``): row b = [0, 1 + b], E[0] = 0, w = 0, w0 = 0,
E[1 + b][c] = m·2^e (|m| <= 15, e in [−10, 0]), y_b = ±n·2^f (n in [1, 15],
f in [−8, 12]).  Then s = E[1 + b], ½(s² − q) = 0, out = 0, g_b = −y_b, the
contribution to dE[0][c] is −y_b·E[1 + b][c] (an 8-bit product) and the one
to dE[1 + b] is ±0.

HHFM known answer (``hhfm_known``): layout "none", NG = 1, one hot item; user
rows are non-zero only in columns 0–3, item and negative rows only in columns
4–7, so pos = neg = 0, z = 0, σ = ½, g = gt = −½ exactly.
"""
import numpy as np

F32, F64 = np.float32, np.float64


def ordered_sum(values, dtype=F32):
    """values[0] + values[1] + … one rounding per add, started from values[0]."""
    values = np.asarray(values, dtype)
    acc = values[0].copy()
    for v in values[1:]:
        acc = (acc + v).astype(dtype)
    return acc


def segment_scatter(ids, contribs, M):
    """ids [n] in occurrence order, contribs [n, ...] float32 (the caller leaves
    out an occurrence that adds nothing) -> dense [M, ...] float32 of the
    per-id ordered sums, 0 where an id has no occurrence."""
    ids = np.asarray(ids, np.int64)
    contribs = np.asarray(contribs, F32)
    out = np.zeros((M,) + contribs.shape[1:], F32)
    order = np.argsort(ids, kind="stable")          # ascending o inside each id
    bounds = np.flatnonzero(np.diff(ids[order])) + 1
    for seg in np.split(order, bounds):
        out[ids[seg[0]]] = ordered_sum(contribs[seg])
    return out


def scalar_sum(rows, dtype=F32):
    """The scalar order: 256 strided partials from 0, then ascending from 0."""
    rows = np.asarray(rows, dtype).reshape(-1)
    part = np.zeros(256, dtype)
    for t in range(min(256, len(rows))):
        acc = dtype(0)
        for v in rows[t::256]:
            acc = dtype(acc + v)
        part[t] = acc
    tot = dtype(0)
    for p in part:
        tot = dtype(tot + p)
    return tot


def loss_sum(rows64):
    """Row losses (float64) in the scalar order, rounded to float32 once."""
    return F32(scalar_sum(rows64, F64))


def _small(rng, shape, emin, emax, mmin=-15, mmax=15):
    m = rng.integers(mmin, mmax + 1, shape).astype(F64)
    e = rng.integers(emin, emax + 1, shape)
    return (m * 2.0 ** e).astype(F32)


# a seed at which the reversed order and two seeded permutations each change the
# bits of dw[0] and of >= half of dE[0]'s columns (tests/test_train_det_ref.py)
FM_KNOWN_SEED = 8


def fm_known(B=3001, k=8, seed=FM_KNOWN_SEED):
    """-> dict: X [B, 2] int32, y, E [B + 1, k], and the expected gradients
    dE, dw, dw0 (float32, the documented orders), the row contributions to
    dE[0] (``c0`` [B, k]) and g [B], and the float64 loss Σ y²/2."""
    rng = np.random.default_rng(seed)
    M = B + 1
    X = np.stack([np.zeros(B, np.int64), 1 + np.arange(B)], 1).astype(np.int32)
    E = np.zeros((M, k), F32)
    E[1:] = _small(rng, (B, k), -10, 0)
    sign = rng.choice([-1.0, 1.0], B)
    y = (sign * rng.integers(1, 16, B) * 2.0 ** rng.integers(-8, 13, B)).astype(F32)
    g = (-y).astype(F32)
    c0 = (g[:, None] * E[1:]).astype(F32)            # exact: 4-bit × 4-bit mantissas
    dE = np.zeros((M, k), F32)
    dE[0] = ordered_sum(c0)
    dw = np.zeros(M, F32)
    dw[0] = ordered_sum(g)
    dw[1:] = g
    loss64 = 0.5 * (y.astype(F64) ** 2)
    return dict(X=X, y=y, E=E, M=M, k=k, g=g, c0=c0, dE=dE, dw=dw, dw0=scalar_sum(g),
                loss=loss_sum(loss64), loss64=float(loss64.sum()))


def hhfm_known(B=1031, k=8, seed=11):
    """-> dict: X [B, 2] (user, item) int32, Neg [B, 1], E, and the expected
    dE (float32, the documented order over o = 3·b + slot: item, negative,
    user) with the occurrence list (``ids``, ``contribs``) it was summed from."""
    assert k == 8
    rng = np.random.default_rng(seed)
    NU, NN = 37, 5
    item = NU
    M = NU + 1 + NN
    users = (np.arange(B) % NU).astype(np.int32)
    negs = (NU + 1 + (np.arange(B) * 7) % NN).astype(np.int32)
    E = np.zeros((M, k), F32)
    E[:NU, :4] = _small(rng, (NU, 4), -10, 0)
    E[NU:, 4:] = _small(rng, (1 + NN, 4), -10, 0)
    X = np.stack([users, np.full(B, item, np.int32)], 1).astype(np.int32)
    Neg = negs[:, None].copy()
    g = F32(-0.5)
    h = E[users]                                     # layout "none": h = E[user]
    it, ng = E[X[:, 1]], E[negs]
    dh = (g * it - g * ng).astype(F32)               # exact whether fused or not
    ids = np.stack([X[:, 1], negs, users], 1).reshape(-1)
    contribs = np.stack([g * h, -g * h, dh], 1).reshape(-1, k).astype(F32)
    return dict(X=X, Neg=Neg, E=E, M=M, k=k, ids=ids, contribs=contribs,
                dE=segment_scatter(ids, contribs, M), item=item,
                loss64=float(B * -np.log(F64(0.5))))
