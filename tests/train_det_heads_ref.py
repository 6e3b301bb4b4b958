"""The orders of the deterministic AFM / DeepFM training steps (include/hhfm.h
"Deterministic AFM and DeepFM steps"), restated in numpy float32 — TEST
INFRASTRUCTURE ONLY — and four inputs whose every contribution is an exact
fp32 product (<= 12 mantissa bits), so the ordered sums are known answers to
the bit.

* table and w: ``train_det_ref.segment_scatter`` over o = b·F + f, as for FM.
* dense head gradients (AFM dP, dp, db; DeepFM dWp): ``head_sum`` — per column
  the scalar order of ``train_det_ref.scalar_sum`` over the rows' values.

All four use y_b = ±n·2^f of ``fm_known`` (g_b = −y_b because out = 0) and
small-mantissa values m·2^e, |m| <= 15 (``train_det_ref._small``):

1. ``afm_table_known``  F = 2, rows [0, 1 + b], E[0] = 0, w = w0 = 0: the one
   pair product is 0, the softmax of one logit is exactly 1, s_p = 0, out = 0,
   dlogit = 0, so dZ = DP = dW = 0 and the contribution to dE[0][c] is
   (g_b·P_c)·E[1 + b][c]; dw[0] the ordered sum of g, dw0 its scalar order.
2. ``afm_head_known``   F = 2, rows [u_b, v_b] (37 users, 5 hot items), P = 0,
   w = w0 = 0: out = 0, dP[c] the scalar order of g_b·(E[u_b][c]·E[v_b][c]);
   E, dp, db, dW get zero.
3. ``dfm_table_known``  F = 2, k = 8, layers [8, 4], rows [0, 1 + b], E[0] = 0,
   w = 0, bp = 0, the deep part of Wp 0: every layer delta is 0, dX0 = 0,
   ½(s² − q) = 0, out = 0; the contribution to dE[0][c] is
   (g_b·Wp[F + c])·E[1 + b][c] and to dw[0] g_b·Wp[0].
4. ``dfm_head_known``   the same rows, Wp = 0, layers and biases 0 (h_L = 0):
   dWp[1] is the scalar order of g_b·w[1 + b], the rest of dWp is 0.
"""
import functools

import numpy as np

from tests.train_det_ref import (F32, F64, _small, loss_sum, ordered_sum, scalar_sum,
                                 segment_scatter)

# a seed at which the reversed order and two seeded permutations each change
# the bits of >= half the columns of every case (tests/test_train_det_heads_ref.py)
KNOWN_SEED = 8


def head_sum(rows):
    """rows [B, n] float32 -> [n]: per column, 256 partials (partial t = rows
    t, t + 256, … ascending from 0), then the partials ascending from 0."""
    rows = np.asarray(rows, F32)
    B, n = rows.shape
    part = np.zeros((256, n), F32)
    for b in range(B):                                   # ascending b = ascending in every t
        part[b % 256] = part[b % 256] + rows[b]
    tot = np.zeros(n, F32)
    for t in range(256):
        tot = tot + part[t]
    return tot


def _small_nz(rng, shape, emin, emax):
    """m·2^e with 1 <= |m| <= 15."""
    v = _small(rng, shape, emin, emax, 1, 15)
    return (v * rng.choice([-1.0, 1.0], shape)).astype(F32)


def _labels(rng, B):
    sign = rng.choice([-1.0, 1.0], B)
    return (sign * rng.integers(1, 16, B) * 2.0 ** rng.integers(-8, 13, B)).astype(F32)


def _hot_rows(B):
    """rows [0, 1 + b]: id 0 in every row, every other id once."""
    return np.stack([np.zeros(B, np.int64), 1 + np.arange(B)], 1).astype(np.int32)


def _attention(rng, k, A):
    gl = np.sqrt(2.0 / (A + k))
    return (rng.normal(0, gl, (k, A)).astype(F32), rng.normal(0, gl, A).astype(F32),
            rng.normal(0, 1, A).astype(F32))


def _scalars(y):
    g = (-y).astype(F32)
    return g, scalar_sum(g), loss_sum(0.5 * (y.astype(F64) ** 2))


@functools.lru_cache(maxsize=None)
def afm_table_known(B=3001, seed=KNOWN_SEED):
    """-> dict: X, y, par = (E, w, w0, W, b, pvec, P), the expected gradients
    ``grads`` in that order, the rows' contributions to dE[0] (``c0`` [B, k])
    with their two factors (``gP`` [B, k], ``e1`` [B, k]), and the loss."""
    k = A = 8
    rng = np.random.default_rng(seed)
    M = B + 1
    X = _hot_rows(B)
    E = np.zeros((M, k), F32)
    E[1:] = _small(rng, (B, k), -10, 0)
    P = _small_nz(rng, k, -4, 0)
    W, b, pvec = _attention(rng, k, A)
    y = _labels(rng, B)
    g, dw0, loss = _scalars(y)
    gP = (g[:, None] * P[None, :]).astype(F32)           # 4-bit × 4-bit
    c0 = (gP * E[1:]).astype(F32)                        # 8-bit × 4-bit
    dE = np.zeros((M, k), F32)
    dE[0] = ordered_sum(c0)
    dw = np.zeros(M, F32)
    dw[0] = ordered_sum(g)
    dw[1:] = g
    zero = lambda v: np.zeros_like(v)  # noqa: E731
    return dict(X=X, y=y, par=(E, np.zeros(M, F32), F32(0), W, b, pvec, P), g=g, gP=gP,
                e1=E[1:], c0=c0, loss=loss,
                grads=(dE, dw, dw0, zero(W), zero(b), zero(pvec), zero(P)))


@functools.lru_cache(maxsize=None)
def afm_head_known(B=1031, seed=KNOWN_SEED):
    """-> dict as afm_table_known; ``rowv`` [B, k] are the rows' values of dP
    with their factors ``g`` and ``pr`` = E[u_b] ⊙ E[v_b]."""
    k = A = 8
    rng = np.random.default_rng(seed)
    NU, NI = 37, 5
    M = NU + NI
    u = (np.arange(B) % NU).astype(np.int32)
    v = (NU + (np.arange(B) * 7) % NI).astype(np.int32)
    X = np.stack([u, v], 1).astype(np.int32)
    E = _small(rng, (M, k), -10, 0)
    W, b, pvec = _attention(rng, k, A)
    y = _labels(rng, B)
    g, dw0, loss = _scalars(y)
    pr = (E[u] * E[v]).astype(F32)                       # 4-bit × 4-bit
    rowv = (g[:, None] * pr).astype(F32)                 # 4-bit × 8-bit
    dw = segment_scatter(X.reshape(-1), np.repeat(g, 2), M)
    zero = lambda a: np.zeros_like(a)  # noqa: E731
    return dict(X=X, y=y, par=(E, np.zeros(M, F32), F32(0), W, b, pvec, np.zeros(k, F32)), g=g,
                pr=pr, rowv=rowv, loss=loss,
                grads=(zero(E), dw, dw0, zero(W), zero(b), zero(pvec), head_sum(rowv)))


DFM_LAYERS = (8, 4)


@functools.lru_cache(maxsize=None)
def dfm_table_known(B=3001, seed=KNOWN_SEED):
    """-> dict: X, y, par = (E, w, layers, biases, Wp, bp), the expected
    gradients of E, w and bp (``dE``, ``dw``, ``dbp``) — Wp[:F + k], the layer
    weights and biases get zero, the deep part of dWp is g·h_L and is not a
    known answer — ``c0`` [B, k] with its factors ``gW``, ``e1``, and the loss."""
    F, k = 2, 8
    rng = np.random.default_rng(seed)
    M = B + 1
    X = _hot_rows(B)
    E = np.zeros((M, k), F32)
    E[1:] = _small(rng, (B, k), -10, 0)
    Wp = np.zeros(F + k + DFM_LAYERS[-1], F32)
    Wp[:F + k] = _small_nz(rng, F + k, -4, 0)
    dims = (F * k,) + DFM_LAYERS
    layers = [rng.normal(0, np.sqrt(2.0 / (a + c)), (a, c)).astype(F32)
              for a, c in zip(dims, dims[1:])]
    biases = [rng.normal(0, 0.3, c).astype(F32) for c in DFM_LAYERS]
    y = _labels(rng, B)
    g, dbp, loss = _scalars(y)
    gW = (g[:, None] * Wp[None, F:F + k]).astype(F32)
    c0 = (gW * E[1:]).astype(F32)
    dE = np.zeros((M, k), F32)
    dE[0] = ordered_sum(c0)
    dw = np.zeros(M, F32)
    dw[0] = ordered_sum((g * Wp[0]).astype(F32))
    dw[1:] = (g * Wp[1]).astype(F32)
    return dict(X=X, y=y, par=(E, np.zeros(M, F32), layers, biases, Wp, F32(0)), g=g, gW=gW,
                e1=E[1:], c0=c0, loss=loss, dE=dE, dw=dw, dbp=dbp)


@functools.lru_cache(maxsize=None)
def dfm_head_known(B=1031, seed=KNOWN_SEED):
    """-> dict as dfm_table_known; dE = dw = 0, ``dWp`` is 0 but element 1, the
    scalar order of ``rowv`` = g_b·w[1 + b]."""
    F, k = 2, 8
    rng = np.random.default_rng(seed)
    M = B + 1
    X = _hot_rows(B)
    E = np.zeros((M, k), F32)
    E[1:] = _small(rng, (B, k), -10, 0)
    w = np.zeros(M, F32)
    w[1:] = _small_nz(rng, B, -10, 0)
    dims = (F * k,) + DFM_LAYERS
    layers = [np.zeros((a, c), F32) for a, c in zip(dims, dims[1:])]
    biases = [np.zeros(c, F32) for c in DFM_LAYERS]
    y = _labels(rng, B)
    g, dbp, loss = _scalars(y)
    rowv = (g * w[1:]).astype(F32)
    dWp = np.zeros(F + k + DFM_LAYERS[-1], F32)
    dWp[1] = scalar_sum(rowv)
    return dict(X=X, y=y, par=(E, w, layers, biases, np.zeros_like(dWp), F32(0)), g=g,
                rowv=rowv, loss=loss, dE=np.zeros_like(E), dw=np.zeros_like(w), dWp=dWp, dbp=dbp)
