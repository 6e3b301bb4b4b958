"""Training dropout — TEST INFRASTRUCTURE ONLY: the numpy restatement of the
mask hhfm_amd/csrc/dropout.h specifies, float64 references of the masked FM
and AFM gradients, and the seeded inputs of tests/test_gpu_dropout.py.

The mask (include/hhfm.h "Training dropout").  Philox4x32-10, multipliers
0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, key = the
64-bit per-step seed (low word, high word).  Element e of row r at site s
reads word (e >> 6) & 3 of the block with counter

    c0 = (e & 63) | ((e >> 8) << 6)    c1 = r & 0xffffffff    c2 = r >> 32    c3 = s

as u = float32(x >> 9) · 2^-23 (exact) and binary = floor(float32(keep) + u):
one float32 add and one floor.  Sites: 0 FM's FM_OUT (n = k), 1 AFM's
attention (n = F(F−1)/2 pairs, i < j order), 2 AFM's k-vector (n = k).

Dropout is tf.nn.dropout's (TF 1.x): y = x / keep · binary, keep the float32
the device holds; forward and backward share the mask.
"""
import numpy as np

from tests import train_ref as tr

F64 = np.float64
SITE_FM, SITE_AFM_ATT, SITE_AFM_VEC = 0, 1, 2
_M32 = np.uint64(0xffffffff)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (broadcastable) uint32 -> [..., 4] uint32."""
    ctr = np.asarray(ctr, np.uint64)
    key = np.asarray(key, np.uint64)
    c0, c1, c2, c3 = (ctr[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                      # 32 x 32 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def words(seed, site, rows, n):
    """The 32-bit word of every element: [rows, n] uint32."""
    seed = int(seed)
    r = np.arange(rows, dtype=np.uint64)[:, None]
    e = np.arange(n, dtype=np.uint64)[None, :]
    ctr = np.stack(np.broadcast_arrays((e & np.uint64(63)) | ((e >> np.uint64(8)) << np.uint64(6)),
                                       r & _M32, r >> np.uint64(32), np.uint64(site)), -1)
    x = philox4x32_10(ctr, np.array([seed & 0xffffffff, seed >> 32], np.uint64))
    w = ((e >> np.uint64(6)) & np.uint64(3)).astype(np.int64)
    return np.take_along_axis(x, np.broadcast_to(w, (rows, n))[..., None], -1)[..., 0]


def binary(seed, site, rows, n, keep):
    """The 0 / 1 decisions as float32 [rows, n]."""
    u = (words(seed, site, rows, n) >> np.uint32(9)).astype(np.float32) * np.float32(2.0 ** -23)
    return np.floor(np.float32(keep) + u).astype(np.float32)


def model_seed(random_seed, step):
    """The seed of a model's partial_fit number ``step`` (0-based)."""
    return (int(random_seed) & 0xffffffff) | (int(step) << 32)


def _mult(bin_, keep):
    return np.asarray(bin_, F64) / F64(np.float32(keep))


# ---------------------------------------------------------------------------
# FM
# ---------------------------------------------------------------------------
def fm_grad64_dropout(X, y, E, w, w0, bin_, keep):
    """tests/train_ref.fm_grad64 with FM_OUT dropped (FM.py:114): bin_ [B, k].
    The multiplier m = bin / keep enters S_b and every |factor| as it enters
    the score and the gradient.  -> loss, (dE, dw, dw0), (magE, magw, magw0)."""
    X = np.asarray(X, np.int64)
    y = np.asarray(y, F64).reshape(-1)
    E = np.asarray(E, F64)
    w = np.asarray(w, F64).reshape(-1)
    w0 = float(w0)
    m = _mult(bin_, keep)                                # [B, k]
    e = E[X]
    s = e.sum(1)
    q = (e * e).sum(1)
    wx = w[X]
    out = (0.5 * (s * s - q) * m).sum(1) + wx.sum(1) + w0
    S = (0.5 * (s * s + q) * m).sum(1) + np.abs(wx).sum(1) + abs(w0)
    g = out - y
    a = np.abs(g) + S
    ae = np.abs(e)
    sa = ae.sum(1)
    dE, mE = np.zeros_like(E), np.zeros_like(E)
    dw, mw = np.zeros_like(w), np.zeros_like(w)
    for f in range(X.shape[1]):
        np.add.at(dE, X[:, f], g[:, None] * m * (s - e[:, f]))
        np.add.at(mE, X[:, f], a[:, None] * m * (sa - ae[:, f]))
        np.add.at(dw, X[:, f], g)
        np.add.at(mw, X[:, f], a)
    return 0.5 * (g * g).sum(), (dE, dw, g.sum()), (mE, mw, a.sum())


def fm_step32_dropout(X, y, E, w, w0, bin_, keep):
    """A float32 restatement of the masked FM step (SGD, lr 1, λ 0; np.add.at
    like oracle.fm_oracle.fm_train_step) -> E, w, w0 after the step."""
    F32 = np.float32
    X = np.asarray(X, np.int64)
    y = np.asarray(y, F32).reshape(-1)
    E = np.asarray(E, F32)
    w = np.asarray(w, F32).reshape(-1)
    m = (np.asarray(bin_, F32) / F32(keep)).astype(F32)
    e = E[X]
    s = e.sum(1, dtype=F32)
    q = (e * e).sum(1, dtype=F32)
    out = (F32(0.5) * (s * s - q) * m).sum(1, dtype=F32) + w[X].sum(1, dtype=F32) + F32(w0)
    g = (out - y).astype(F32)
    dE, dw = np.zeros_like(E), np.zeros_like(w)
    for f in range(X.shape[1]):
        np.add.at(dE, X[:, f], (g[:, None] * m) * (s - e[:, f]))
        np.add.at(dw, X[:, f], g)
    return E - dE, w - dw, F32(F32(w0) - g.sum(dtype=F32))


# the existing cases and k = 260: elements 256.. take a second block index
FM_CASES = dict(tr.FM_CASES, k260=(260, 3, 5, 50, False, False))
FM_KEEPS = (0.5, 0.7, 0.9)
FM_SEED = 2016 | 7 << 32


def fm_case(name):
    """train_ref.fm_case, extended by k260."""
    if name in tr.FM_CASES:
        return tr.fm_case(name)
    k, F, B, M, _, _ = FM_CASES[name]
    rng = np.random.default_rng(360)
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    E = rng.normal(0, (k * F * F / 2.0) ** -0.25, (M, k)).astype(np.float32)
    w = rng.normal(0, 0.3, M).astype(np.float32)
    return X, rng.integers(0, 2, B).astype(np.float32), E, w, np.float32(0.02)


# ---------------------------------------------------------------------------
# AFM
# ---------------------------------------------------------------------------
def _pairs(e):
    F = e.shape[1]
    return np.stack([e[:, i] * e[:, j] for i in range(F) for j in range(i + 1, F)], 1)


def afm_relu_margin(X, E, W, b):
    """Per row, the least |z| / (Σ_c |pr_c W_ca| + |b_a|) over the row's
    (pair, a): how far the nearest pre-activation lies from relu's kink."""
    pr = _pairs(np.asarray(E, F64)[np.asarray(X, np.int64)])
    W, b = np.asarray(W, F64), np.asarray(b, F64).reshape(-1)
    z = pr @ W + b
    S = np.abs(pr) @ np.abs(W) + np.abs(b)
    return (np.abs(z) / S).min((1, 2))


def afm_grad64_dropout(X, y, params, bin1, bin2, keep):
    """AFM's loss Σ(y − out)²/2 and its gradient in float64 with the softmaxed
    attention dropped by bin1 [B, np] / keep[0] (AFM.py:126) and the k-vector
    by bin2 [B, k] / keep[1] (AFM.py:134).  params = (E, w, w0, W, b, pvec, P);
    -> loss, gradients in that order."""
    X = np.asarray(X, np.int64)
    y = np.asarray(y, F64).reshape(-1)
    E, w, w0, W, b, pvec, P = (np.asarray(v, F64) for v in params)
    w, b, pvec, P = w.reshape(-1), b.reshape(-1), pvec.reshape(-1), P.reshape(-1)
    B, F = X.shape
    m1, m2 = _mult(bin1, keep[0]), _mult(bin2, keep[1])
    e = E[X]
    pr = _pairs(e)                                       # [B, np, k]
    z = pr @ W + b                                       # [B, np, A]
    r = np.maximum(z, 0)
    logit = r @ pvec
    ex = np.exp(logit - logit.max(1, keepdims=True))
    a = ex / ex.sum(1, keepdims=True)
    at = a * m1                                          # the dropped attention
    afm = (at[:, :, None] * pr).sum(1)                   # [B, k]
    Pm = P[None, :] * m2                                 # [B, k]
    out = (afm * Pm).sum(1) + w[X].sum(1) + float(w0)
    g = out - y
    dP = (g[:, None] * m2 * afm).sum(0)
    s = (pr * Pm[:, None, :]).sum(2)                     # [B, np]
    da = m1 * g[:, None] * s
    dlogit = a * (da - (a * da).sum(1, keepdims=True))
    dpvec = (dlogit[:, :, None] * r).sum((0, 1))
    dz = dlogit[:, :, None] * pvec * (z > 0)
    db = dz.sum((0, 1))
    dW = np.einsum("bpc,bpa->ca", pr, dz)
    dpr = at[:, :, None] * (g[:, None] * Pm)[:, None, :] + dz @ W.T
    de = np.zeros_like(e)
    p = 0
    for i in range(F):
        for j in range(i + 1, F):
            de[:, i] += dpr[:, p] * e[:, j]
            de[:, j] += dpr[:, p] * e[:, i]
            p += 1
    dE, dw = np.zeros_like(E), np.zeros_like(w)
    for f in range(F):
        np.add.at(dE, X[:, f], de[:, f])
        np.add.at(dw, X[:, f], g)
    return 0.5 * (g * g).sum(), (dE, dw, g.sum(), dW, db, dpvec, dP)


# (F, k, A, B), all inside the step's envelope
AFM_SHAPES = [(3, 8, 8, 1), (5, 16, 16, 5), (16, 8, 8, 3), (5, 256, 8, 2), (5, 64, 64, 1030)]
AFM_KEEPS = [(0.5, 1.0), (1.0, 0.5), (0.7, 0.6)]
AFM_VOCAB = 10                    # ids per field; M = F · AFM_VOCAB


def afm_margin_needed(k):
    """fp32 evaluates z = Σ_c pr_c W_ca + b_a (k rounded products of rounded
    pair products, k additions) within (k + 2) · 2^-24 · (Σ|pr_c W_ca| + |b_a|)
    to first order, in any summation order; 4 × that keeps every
    pre-activation's sign — relu' — the same in fp32 and float64."""
    return 4 * (k + 2) * 2.0 ** -24


def afm_case(shape):
    """-> X [B, F] int32, y, (E, w, w0, W, b, pvec, P) float32.  Field f draws
    from its own AFM_VOCAB ids.  A row whose nearest pre-activation is closer to
    0 than afm_margin_needed(k) is drawn again (relu' is then the same in fp32
    and float64; asserted in tests/test_dropout_ref.py)."""
    F, k, A, B = shape
    rng = np.random.default_rng(AFM_SHAPES.index(tuple(shape)) + 500)
    M = F * AFM_VOCAB
    base = np.arange(F) * AFM_VOCAB
    E = rng.normal(0, min(0.3, 0.3 * (64.0 / k) ** 0.25), (M, k)).astype(np.float32)
    w = rng.normal(0, 0.1, M).astype(np.float32)
    gl = np.sqrt(2.0 / (A + k))
    W = rng.normal(0, gl, (k, A)).astype(np.float32)
    b = rng.normal(0, gl, A).astype(np.float32)
    pvec = rng.normal(0, 1, A).astype(np.float32)
    P = rng.normal(1, 0.2, k).astype(np.float32)
    X = (base + rng.integers(0, AFM_VOCAB, (B, F))).astype(np.int32)
    for _ in range(100):
        bad = afm_relu_margin(X, E, W, b) < afm_margin_needed(k)
        if not bad.any():
            break
        X[bad] = base + rng.integers(0, AFM_VOCAB, (int(bad.sum()), F))
    y = rng.choice([1.0, -1.0], B).astype(np.float32)
    return X, y, (E, w, np.float32(0.02), W, b, pvec, P)


def afm_masks(seed, shape, keep):
    F, k, _, B = shape
    return (binary(seed, SITE_AFM_ATT, B, F * (F - 1) // 2, keep[0]),
            binary(seed, SITE_AFM_VEC, B, k, keep[1]))
