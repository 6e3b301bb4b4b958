"""FM with batch_norm=1 — TEST INFRASTRUCTURE ONLY: the numpy restatement of
the layer include/hhfm.h specifies ("FM batch norm"), float64 and float32
forms of the training forward / backward, the float64 gradients with their
magnitudes, the exact inference score, and the designed known answer of
tests/test_gpu_fm_bn.py.

The layer (tf.contrib.layers.batch_norm on x = FM [B, 1, k], non-fused path):

    x_bc = ½(s_bc² − q_bc)        μ_c = Σ_b x_bc / B        v_c = Σ_b (x_bc − μ_c)² / B
    inv_c = 1/√(v_c + eps)        a_c = inv_c·γ_c            y_bc = x_bc·a_c + (β_c − μ_c·a_c)
    out_b = Σ_c y_bc·m_bc + Σ_f w + w0          m = bin / keep (1 without dropout)

    g_b = out_b − y_b    dy = g·m    x̂ = (x − μ)·inv    dβ = Σ_b dy    dγ = Σ_b dy·x̂
    dx = (a/B)·(B·dy − dβ − x̂·dγ)               dE[x_f] += dx·(s − e_f)

``fm_bn_grad64``'s magnitudes are built as tests/train_ref.fm_grad64 builds
``mag``: every product becomes the product of absolute values and every sum
the sum of absolute values.  |x| is ½(s² + q) as there, |μ| its batch mean,
S_b = Σ_c (|x|·|a| + |β| + |μ|·|a|)·m + Σ|w| + |w0| the forward's Σ|terms|
through the layer's form, g_b's own uncertainty |g_b| + S_b, |x̂| = (|x| + |μ|)·inv
and B·dy − dβ − x̂·dγ becomes B|dy| + Σ|dy| + |x̂|·Σ|dy·x̂|.
"""
import numpy as np

F64 = np.float64
F32 = np.float32
EPS = 0.001                      # contrib batch_norm's default epsilon
BN_UPDATE = float(1.0 - 0.9)     # 1 − decay, formed in double as TF forms it


def _mult(bin_, keep, shape, dt):
    if bin_ is None:
        return np.ones(shape, dt)
    return (np.asarray(bin_, dt) / dt(F32(keep))).astype(dt)


def fm_bn_step(X, y, E, w, w0, gamma, beta, eps=EPS, bin_=None, keep=1.0, dtype=F64):
    """The training forward and backward in ``dtype`` (float64, or float32 with
    every intermediate rounded to float32).  -> dict: loss (Σ(y − out)²/2, in
    float64 from ``dtype`` residuals), out, g, x, mu, v, and the gradients dE,
    dw, dw0, dgamma, dbeta."""
    dt = dtype
    X = np.asarray(X, np.int64)
    y = np.asarray(y, dt).reshape(-1)
    E = np.asarray(E, dt)
    w = np.asarray(w, dt).reshape(-1)
    gamma, beta = np.asarray(gamma, dt).reshape(-1), np.asarray(beta, dt).reshape(-1)
    B, F = X.shape
    e = E[X]
    s = e.sum(1, dtype=dt)
    q = (e * e).sum(1, dtype=dt)
    x = (dt(0.5) * (s * s - q)).astype(dt)
    mu = (x.sum(0, dtype=dt) / dt(B)).astype(dt)
    d = x - mu
    v = ((d * d).sum(0, dtype=dt) / dt(B)).astype(dt)
    inv = (dt(1) / np.sqrt(v + dt(eps), dtype=dt)).astype(dt)
    a = inv * gamma
    yv = x * a + (beta - mu * a)
    m = _mult(bin_, keep, x.shape, dt)
    out = ((yv * m).sum(1, dtype=dt) + w[X].sum(1, dtype=dt) + dt(w0)).astype(dt)
    g = (out - y).astype(dt)
    dy = g[:, None] * m
    xh = d * inv
    dbeta = dy.sum(0, dtype=dt)
    dgamma = (dy * xh).sum(0, dtype=dt)
    dx = (a / dt(B)) * (dt(B) * dy - dbeta - xh * dgamma)
    dE, dw = np.zeros_like(E), np.zeros_like(w)
    for f in range(F):
        np.add.at(dE, X[:, f], dx * (s - e[:, f]))
        np.add.at(dw, X[:, f], g)
    loss = 0.5 * (g.astype(F64) ** 2).sum()
    return dict(loss=loss, out=out, g=g, x=x, mu=mu, v=v, dE=dE, dw=dw, dw0=g.sum(dtype=dt),
                dgamma=dgamma, dbeta=dbeta)


def fm_bn_loss64(X, y, E, w, w0, gamma, beta, eps=EPS, bin_=None, keep=1.0):
    """The float64 data loss alone (what the finite differences differentiate)."""
    X = np.asarray(X, np.int64)
    E = np.asarray(E, F64)
    e = E[X]
    s = e.sum(1)
    x = 0.5 * (s * s - (e * e).sum(1))
    mu = x.mean(0)
    v = ((x - mu) ** 2).mean(0)
    a = np.asarray(gamma, F64) / np.sqrt(v + eps)
    yv = x * a + (np.asarray(beta, F64) - mu * a)
    out = (yv * _mult(bin_, keep, x.shape, F64)).sum(1) + np.asarray(w, F64).reshape(-1)[X].sum(1)
    r = np.asarray(y, F64).reshape(-1) - (out + float(w0))
    return 0.5 * (r * r).sum()


def fm_bn_grad64(X, y, E, w, w0, gamma, beta, eps=EPS, bin_=None, keep=1.0):
    """-> loss, (dE, dw, dw0, dγ, dβ), (magE, magw, magw0, magγ, magβ), stats
    (x, mu, v of the float64 forward)."""
    r = fm_bn_step(X, y, E, w, w0, gamma, beta, eps, bin_, keep, F64)
    X = np.asarray(X, np.int64)
    E = np.asarray(E, F64)
    w = np.asarray(w, F64).reshape(-1)
    gamma, beta = np.asarray(gamma, F64).reshape(-1), np.asarray(beta, F64).reshape(-1)
    B, F = X.shape
    e = E[X]
    s = e.sum(1)
    q = (e * e).sum(1)
    ae = np.abs(e)
    sa = ae.sum(1)
    xa = 0.5 * (s * s + q)                                # |x| as train_ref.fm_grad64's S
    mua = xa.mean(0)
    inv = 1.0 / np.sqrt(r["v"] + eps)
    aa = inv * np.abs(gamma)
    m = _mult(bin_, keep, xa.shape, F64)
    S = ((xa * aa + np.abs(beta) + mua * aa) * m).sum(1) + np.abs(w[X]).sum(1) + abs(float(w0))
    A = np.abs(r["g"]) + S                                # g_b's own uncertainty
    dya = A[:, None] * m
    xha = (xa + mua) * inv
    mbeta = dya.sum(0)
    mgamma = (dya * xha).sum(0)
    dxa = (aa / B) * (B * dya + mbeta + xha * mgamma)
    mE, mw = np.zeros_like(E), np.zeros_like(w)
    for f in range(F):
        np.add.at(mE, X[:, f], dxa * (sa - ae[:, f]))
        np.add.at(mw, X[:, f], A)
    return (r["loss"], (r["dE"], r["dw"], r["dw0"], r["dgamma"], r["dbeta"]),
            (mE, mw, A.sum(), mgamma, mbeta), dict(x=r["x"], mu=r["mu"], v=r["v"]))


def fm_bn_score64(X, E, w, w0, gamma, beta, mm, mv, eps=EPS):
    """The exact inference score (moving statistics, no dropout) and its
    Σ|terms| for tests/helpers.kappa_check:
    out_b = Σ_c a_c·x_bc + Σ_f w + w0 + Σ_c (β_c − mm_c·a_c), a = γ/√(mv + eps)."""
    X = np.asarray(X, np.int64)
    E = np.asarray(E, F64)
    w = np.asarray(w, F64).reshape(-1)
    gamma, beta, mm, mv = (np.asarray(t, F64).reshape(-1) for t in (gamma, beta, mm, mv))
    e = E[X]
    s = e.sum(1)
    q = (e * e).sum(1)
    a = gamma / np.sqrt(mv + eps)
    out = (a * 0.5 * (s * s - q)).sum(1) + w[X].sum(1) + float(w0) + (beta - mm * a).sum()
    mag = ((np.abs(a) * 0.5 * (s * s + q)).sum(1) + np.abs(w[X]).sum(1) + abs(float(w0))
           + (np.abs(beta) + np.abs(mm * a)).sum())
    return out, mag


def moving_update64(mm, mv, mu, v, u=BN_UPDATE):
    """assign_moving_average, zero_debias=False: m −= (m − value)·u."""
    mm, mv = np.asarray(mm, F64), np.asarray(mv, F64)
    return mm - (mm - mu) * u, mv - (mv - v) * u


# ---------------------------------------------------------------------------
# the known answer: every contribution and every sum exact in fp32, any order
# ---------------------------------------------------------------------------
KNOWN_EPS = 3.0      # v = 1, so inv = 1/√4 = ½ exactly


def known_answer():
    """B = 256, F = 2, k = 8.  Users 0 / 1 hold rows of +1 / −1, 16 items hold
    ±1 entries, row b = [b % 2, 2 + (b // 2) % 16]: x = ±1 with each item under
    both users equally often, so μ = 0, v = 1, inv = ½ (eps = 3).  γ_c = 2^(c % 3),
    β_c = c % 5 − 2, w = 0, w0 = 0.25, integer labels in [−3, 3].
    -> X, y, E, w, w0, gamma, beta."""
    B, k, NI = 256, 8, 16
    rng = np.random.default_rng(3)
    E = np.empty((2 + NI, k), F32)
    E[0], E[1] = 1.0, -1.0
    E[2:] = rng.choice(np.array([-1.0, 1.0], F32), (NI, k))
    b = np.arange(B)
    X = np.stack([b % 2, 2 + (b // 2) % NI], 1).astype(np.int32)
    y = rng.integers(-3, 4, B).astype(F32)
    c = np.arange(k)
    gamma = (2.0 ** (c % 3)).astype(F32)
    beta = (c % 5 - 2).astype(F32)
    return X, y, E, np.zeros(2 + NI, F32), F32(0.25), gamma, beta
