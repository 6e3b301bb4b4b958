"""The orders of the deterministic attention=0 AFM step (include/hhfm.h "AFM
without attention", hhfm_afm_noatt_train_step_det), restated in numpy float32
— TEST INFRASTRUCTURE ONLY — on tests/train_det_ref.py's ``segment_scatter``
and ``scalar_sum``, and an input whose forward is exact in fp32, so that the
restatement is a known answer to the bit.

* dE[id][c], dw[id]: occurrence o = b·F + f; contribution gc·(S_b[c] − e)
  with gc = g_b·P_c (· bin / keep), every product rounded on its own; a
  dropped column adds nothing; dw: g_b.  The fp32 sum of the id's
  contributions in ascending o, started from the first one.
* dP[c]: v_bc = g_b·(x_bc / keep · bin_bc) in the scalar order.
* dw0: g_b in the scalar order; the loss: g_b²/2 in double in the scalar
  order, rounded to float once.

``noatt_known``: rows [0, 1 + b] (id 0 is hot), every table entry m·2^e with
|m| <= 15, e in [−3, 0], P_c in ±{1, 2, 3}, w, w0 and y multiples of 2^−6.
Then s, q, x = e_0·e_b, d, out, r and g are exact in fp32 in any order of
addition (out is an integer multiple of 2^−6 below 2^24 of them), and only
the documented products and sums round.
"""
import numpy as np

from tests.train_det_ref import _small, loss_sum, scalar_sum, segment_scatter

F32, F64 = np.float32, np.float64


def forward32(X, y, E, w, w0, P, mask=None, keep=1.0):
    """The row pass in float32, field order: S [B, k], d [B, k] (x / keep ·
    bin), g [B], the row losses in float64."""
    X = np.asarray(X, np.int64)
    B, F = X.shape
    k = E.shape[1]
    s, q = np.zeros((B, k), F32), np.zeros((B, k), F32)
    for f in range(F):
        v = E[X[:, f]]
        s = (s + v).astype(F32)
        q = (q + (v * v).astype(F32)).astype(F32)
    x = (F32(0.5) * ((s * s).astype(F32) - q).astype(F32)).astype(F32)
    if mask is not None:
        x = ((x / F32(keep)).astype(F32) * np.asarray(mask, F32)).astype(F32)
    t = (x.astype(F64) * np.asarray(P, F64)).sum(1)   # exact inputs: any order, the same float
    assert np.array_equal(t, t.astype(F32).astype(F64)), "the known-answer forward must be exact"
    fb = np.zeros(B, F32)
    for f in range(F):
        fb = (fb + w[X[:, f]]).astype(F32)
    out = ((t.astype(F32) + fb).astype(F32) + F32(w0)).astype(F32)
    r = (np.asarray(y, F32) - out).astype(F32)
    g = (-r).astype(F32)
    return s, x, g, 0.5 * (r.astype(F64) * r.astype(F64))


def step_ref(X, y, E, w, w0, P, mask=None, keep=1.0):
    """-> dict(dE, dw, dw0, dP, loss): the documented orders."""
    X = np.asarray(X, np.int64)
    B, F = X.shape
    M, k = E.shape
    P = np.asarray(P, F32)
    S, d, g, l64 = forward32(X, y, E, w, w0, P, mask, keep)
    gc = (g[:, None] * P[None, :]).astype(F32)
    if mask is not None:
        gc = ((gc * np.asarray(mask, F32)).astype(F32) / F32(keep)).astype(F32)
    dE = np.zeros((M, k), F32)
    ids = X.reshape(-1)                                   # o = b·F + f
    b_of = np.repeat(np.arange(B), F)
    contrib = (gc[b_of] * (S[b_of] - E[ids]).astype(F32)).astype(F32)
    kept = np.ones((B * F, k), bool) if mask is None else np.asarray(mask)[b_of] != 0
    for c in range(k):                                    # a dropped column adds nothing
        sel = kept[:, c]
        if sel.any():
            dE[:, c] = segment_scatter(ids[sel], contrib[sel, c], M)
    dw = segment_scatter(ids, g[b_of], M)
    v = (g[:, None] * d).astype(F32)
    dP = np.array([scalar_sum(v[:, c]) for c in range(k)], F32)
    return dict(dE=dE, dw=dw, dw0=scalar_sum(g), dP=dP, loss=loss_sum(l64),
                loss64=float(l64.sum()))


def noatt_known(B=1031, k=8, seed=5):
    """-> dict: X [B, 2] int32, y, E [B + 1, k], w, w0, P, M, k."""
    rng = np.random.default_rng(seed)
    M = B + 1
    X = np.stack([np.zeros(B, np.int64), 1 + np.arange(B)], 1).astype(np.int32)
    E = _small(rng, (M, k), -3, 0)
    E[E == 0] = F32(0.5)
    P = (rng.choice([-1.0, 1.0], k) * rng.integers(1, 4, k)).astype(F32)
    w = (rng.integers(-31, 32, M) * 2.0 ** -6).astype(F32)
    w0 = F32(0.25)
    y = (rng.choice([-1.0, 1.0], B) * rng.integers(1, 64, B) * 2.0 ** -6).astype(F32)
    return dict(X=X, y=y, E=E, w=w, w0=w0, P=P, M=M, k=k)
