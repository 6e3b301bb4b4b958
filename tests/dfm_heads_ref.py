"""Restatement of the reference DeepFM's heads — TEST INFRASTRUCTURE ONLY.

``DeepFM(use_fm, use_deep, loss_type)`` (DFM.py:131-152, 199-204): the concat
projection sees [y1 | y2] (FM head), [h_L] (deep head) or [y1 | y2 | h_L]; with
loss_type "logloss" the output goes through a sigmoid and the loss is TF-1.x
``tf.losses.log_loss`` at its defaults:

    loss = (Σ_b l_b)/B,  l_b = −y·log(p + ε) − (1 − y)·log(1 − p + ε),  ε = 1e-7

``forward`` / ``loss32`` / ``train_step`` are float32 in the reference's op
order (built from oracle.fm_oracle's pieces; with head 3 they are
``orc.dfm_out`` and ``orc.dfm_train_step``, pinned in
tests/test_dfm_heads_ref.py).  ``grad64`` is the float64 gradient of the loss
at λ = 0 with a magnitude per element, in the way of tests/train_ref.py:

    mag = Σ_rows (|g_b| + c_b·S_b) · |factor|

S_b the row's Σ_j |concat_j·Wp_j| + |bp| (oracle.parity.dfm_magnitude's scale of
z over the head's columns), c_b = |∂g_b/∂z_b| (1 for mse; p(1 − p)/B for
logloss, since g_b = (p − y)/B up to ε), |factor| what multiplies g_b in that
element's gradient with every product taken in absolute values (through the
layers: |W|, relu' as in the forward).  A z off by the project's bar
(1e-5·S_b) moves g_b by c_b times as much, so 1e-5·mag is that bar propagated
to first order.  Where the factor is itself a computed forward quantity — a
concat entry in dWp, an activation h_i in dW_i — it enters by its own Σ|terms|
(y2_c: ½((Σe)² + Σe²); h_i: |h_{i-1}|·|W_{i-1}| + |b_{i-1}|; table rows and w:
their absolute values): fp32 computes such a sum to a fraction of its Σ|terms|,
not of its value, and a ReLU unit near zero is a cancelled sum — the same
convention as S itself.
"""
import numpy as np

from oracle import fm_oracle as orc

F32, F64 = np.float32, np.float64
HEAD_FM, HEAD_DEEP, HEAD_SIGMOID = 1, 2, 4
EPS = 1e-7
# the six heads of the fixtures: name -> (use_fm, use_deep, loss_type)
HEADS = {"fm_mse": (True, False, "mse"), "deep_mse": (False, True, "mse"),
         "both_mse": (True, True, "mse"), "fm_logloss": (True, False, "logloss"),
         "deep_logloss": (False, True, "logloss"), "both_logloss": (True, True, "logloss")}


def head_word(use_fm, use_deep, loss_type):
    return ((HEAD_FM if use_fm else 0) | (HEAD_DEEP if use_deep else 0)
            | (HEAD_SIGMOID if loss_type == "logloss" else 0))


def wp_size(head, F, k, layers):
    """concat_projection's rows (DFM.py:199-204)."""
    return (F + k if head & HEAD_FM else 0) + (layers[-1] if head & HEAD_DEEP else 0)


def _concat(X, E, w, layers, biases, head, dt):
    """-> cat [B, D], hs (the layers' activations, hs[0] the gathered rows), e, s,
    |cat| in float64, and the Σ|terms| of cat's entries and of every hs[i]
    (float64; ``grad64``'s factors)."""
    X = np.asarray(X, np.int64)
    E = np.asarray(E, dt)
    w = np.asarray(w, dt).reshape(-1)
    B, F = X.shape
    k = E.shape[1]
    e = E[X]                                                          # DFM.py:104
    s = e.sum(1, dtype=dt)
    parts, tm, hs = [], [], [e.reshape(B, F * k)]
    hm = [np.abs(hs[0]).astype(F64)]
    if head & HEAD_FM:
        parts += [w[X], dt(0.5) * (s * s - (e * e).sum(1, dtype=dt))]  # :109-122
        e64 = e.astype(F64)
        tm += [np.abs(w[X]).astype(F64), 0.5 * (e64.sum(1) ** 2 + (e64 * e64).sum(1))]
    if head & HEAD_DEEP:
        for W, b in zip(layers, biases):                              # :125-128
            W = np.asarray(W, dt)
            b = np.asarray(b, dt).reshape(-1)
            hm.append(np.abs(hs[-1]).astype(F64) @ np.abs(W).astype(F64) + np.abs(b).astype(F64))
            hs.append(np.maximum(np.matmul(hs[-1], W).astype(dt) + b, 0).astype(dt))
        parts.append(hs[-1])
        tm.append(hm[-1])
    cat = np.concatenate(parts, axis=1)
    return cat, hs, e, s, np.abs(cat).astype(F64), (np.concatenate(tm, axis=1), hm)


def forward(X, E, w, layers, biases, Wp, bp, head, dt=F32):
    """-> out [B] (z, or the sigmoid under SIGMOID), z [B], S [B] = Σ|terms| of z."""
    cat, _, _, _, cm, _ = _concat(X, E, w, layers, biases, head, dt)
    Wp = np.asarray(Wp, dt).reshape(-1)
    z = np.matmul(cat, Wp).astype(dt) + dt(bp)                        # :137
    S = cm @ np.abs(Wp).astype(F64) + abs(float(bp))
    out = (dt(1) / (dt(1) + np.exp(-z))).astype(dt) if head & HEAD_SIGMOID else z
    return out, z, S


def catalog_rows(A, n_user, n_item):
    return orc.dfm_catalog_rows(A, n_user, n_item)


def log_loss(y, p, dt=F32):
    """tf.losses.log_loss(labels, predictions) at its defaults."""
    y, p = np.asarray(y, dt).reshape(-1), np.asarray(p, dt).reshape(-1)
    if y.size == 0:
        return dt(0)
    l = -y * np.log(p + dt(EPS)) - (dt(1) - y) * np.log(dt(1) - p + dt(EPS))
    return dt(l.sum(dtype=dt) / dt(y.size))


def _l2(Wp, layers, head):
    reg = np.sum(np.asarray(Wp, F64) ** 2)
    if head & HEAD_DEEP:                                              # :149-152
        reg += sum(np.sum(np.asarray(W, F64) ** 2) for W in layers)
    return reg


def loss32(X, y, E, w, layers, biases, Wp, bp, head, lam):
    """The reference's ``self.loss`` (DFM.py:139-152)."""
    out, _, _ = forward(X, E, w, layers, biases, Wp, bp, head)
    y = np.asarray(y, F32).reshape(-1)
    if head & HEAD_SIGMOID:
        data = F64(log_loss(y, out))
    else:
        data = np.sum((y - out).astype(F64) ** 2) / 2
    return F32(data + (lam * _l2(Wp, layers, head) / 2 if lam > 0 else 0.0))


def _backward(X, y, E, w, layers, biases, Wp, bp, head, dt):
    """-> data loss, g [B], the gradients at λ = 0 (dict E, w, W0.., b0.., Wp,
    bp; None for a variable the head gives none), and what ``grad64`` needs for
    the magnitudes."""
    X = np.asarray(X, np.int64)
    y = np.asarray(y, dt).reshape(-1)
    layers = [np.asarray(W, dt) for W in layers]
    Wp = np.asarray(Wp, dt).reshape(-1)
    B, F = X.shape
    k = np.asarray(E).shape[1]
    fm, deep = bool(head & HEAD_FM), bool(head & HEAD_DEEP)
    cat, hs, e, s, cm, (tm, hm) = _concat(X, E, w, layers, biases, head, dt)
    z = np.matmul(cat, Wp).astype(dt) + dt(bp)
    if head & HEAD_SIGMOID:
        p = (dt(1) / (dt(1) + np.exp(-z))).astype(dt)
        data = F64(log_loss(y, p, dt))
        g = (((dt(1) - y) / (dt(1) - p + dt(EPS)) - y / (p + dt(EPS))) * p * (dt(1) - p)
             / dt(max(B, 1))).astype(dt)
        slope = (p * (dt(1) - p)).astype(F64) / max(B, 1)
    else:
        r = y - z
        data = np.sum(r.astype(F64) ** 2) / 2
        g = -r                                                        # d loss / d out
        slope = np.ones(B)
    gr = {"Wp": np.matmul(cat.T, g).astype(dt), "bp": dt(g.sum(dtype=F64)), "w": None}
    dcat = g[:, None] * Wp[None, :]
    nfm = F + k if fm else 0
    de = np.zeros((B, F, k), dt)
    L = len(layers)
    dzs = [None] * L
    if deep:
        dh = dcat[:, nfm:]
        for i in range(L - 1, -1, -1):
            dzs[i] = (dh * (hs[i + 1] > 0)).astype(dt)                # relu'
            gr[f"W{i}"] = np.matmul(hs[i].T, dzs[i]).astype(dt)
            gr[f"b{i}"] = dzs[i].sum(0, dtype=dt)
            dh = np.matmul(dzs[i], layers[i].T).astype(dt)
        de = de + dh.reshape(B, F, k)
    else:
        for i in range(L):
            gr[f"W{i}"] = gr[f"b{i}"] = None
    if fm:
        de = de + dcat[:, None, F:F + k] * (s[:, None, :] - e)
    dE = np.zeros_like(np.asarray(E, dt))
    for f in range(F):
        np.add.at(dE, X[:, f], de[:, f])
    gr["E"] = dE
    if fm:
        dw = np.zeros(np.asarray(w).size, dt)
        for f in range(F):
            np.add.at(dw, X[:, f], dcat[:, f])
        gr["w"] = dw
    return data, g, gr, dict(z=z, cat=cat, hs=hs, e=e, s=s, cm=cm, tm=tm, hm=hm, slope=slope,
                             nfm=nfm)


def grad64(X, y, E, w, layers, biases, Wp, bp, head):
    """-> loss, grads, mags (dicts keyed E, w, W0.., b0.., Wp, bp; None where
    the head gives no gradient), z: float64, λ = 0."""
    X = np.asarray(X, np.int64)
    data, g, gr, t = _backward(X, y, E, w, layers, biases, Wp, bp, head, F64)
    B, F = X.shape
    k = np.asarray(E).shape[1]
    Wp = np.abs(np.asarray(Wp, F64).reshape(-1))
    S = t["cm"] @ Wp + abs(float(bp))
    a = np.abs(g) + t["slope"] * S                                    # [B]
    mg = {"Wp": t["tm"].T @ a, "bp": a.sum(), "w": None}
    ae = np.abs(t["e"])
    me = np.zeros((B, F, k))
    L = len(layers)
    if head & HEAD_DEEP:
        hm = t["hm"]
        mdh = a[:, None] * Wp[None, t["nfm"]:]
        for i in range(L - 1, -1, -1):
            mdz = mdh * (t["hs"][i + 1] > 0)
            mg[f"W{i}"] = hm[i].T @ mdz
            mg[f"b{i}"] = mdz.sum(0)
            mdh = mdz @ np.abs(np.asarray(layers[i], F64)).T
        me = me + mdh.reshape(B, F, k)
    else:
        for i in range(L):
            mg[f"W{i}"] = mg[f"b{i}"] = None
    if head & HEAD_FM:
        me = me + a[:, None, None] * Wp[None, None, F:F + k] * (ae.sum(1)[:, None, :] - ae)
        mw = np.zeros(np.asarray(w).size)
        for f in range(F):
            np.add.at(mw, X[:, f], a * Wp[f])
        mg["w"] = mw
    mE = np.zeros_like(np.asarray(E, F64))
    for f in range(F):
        np.add.at(mE, X[:, f], me[:, f])
    mg["E"] = mE
    return data, gr, mg, t["z"]


def keys(L):
    return ["E", "w"] + [f"W{i}" for i in range(L)] + [f"b{i}" for i in range(L)] + ["Wp", "bp"]


def train_step(X, y, E, w, layers, biases, Wp, bp, acc, lr, lam, head, optimizer="adagrad",
               step=1):
    """One TF-1.x optimizer step of the head's loss (DFM.py:139-155): like
    ``orc.dfm_train_step``; a variable without a gradient, and its slot, come
    back as they went in (TF's minimize skips it).
    Returns (loss, E, w, layers, biases, Wp, bp, acc)."""
    X = np.asarray(X, np.int64)
    E = np.asarray(E, F32)
    w = np.asarray(w, F32).reshape(-1)
    layers = [np.asarray(W, F32) for W in layers]
    biases = [np.asarray(b, F32).reshape(-1) for b in biases]
    Wp = np.asarray(Wp, F32).reshape(-1)
    deep = bool(head & HEAD_DEEP)
    acc = {key: np.asarray(v, F32).copy() for key, v in acc.items()}
    if len(X) == 0:
        data = 0.0
        gr = {kk: None for kk in keys(len(layers))}
        gr.update(E=np.zeros_like(E), Wp=np.zeros_like(Wp), bp=F32(0))
        if head & HEAD_FM:
            gr["w"] = np.zeros_like(w)
        if deep:
            gr.update({f"W{i}": np.zeros_like(W) for i, W in enumerate(layers)})
            gr.update({f"b{i}": np.zeros_like(b) for i, b in enumerate(biases)})
    else:
        data, _, gr, _ = _backward(X, y, E, w, layers, biases, Wp, bp, head, F32)
    loss = F32(data + lam * _l2(Wp, layers, head) / 2)
    gr["Wp"] = gr["Wp"] + F32(lam) * Wp
    if deep:
        for i, W in enumerate(layers):
            gr[f"W{i}"] = gr[f"W{i}"] + F32(lam) * W

    def upd(var, key, rows=None):
        if gr[key] is None:
            return var
        var, acc[key] = orc.tf_apply(optimizer, var, gr[key], acc.get(key), lr, step, rows)
        return var

    E = upd(E, "E", X)
    w = upd(w, "w", X)
    layers = [upd(W, f"W{i}") for i, W in enumerate(layers)]
    biases = [upd(b, f"b{i}") for i, b in enumerate(biases)]
    Wp = upd(Wp, "Wp")
    bp = upd(np.float32(bp), "bp")
    return loss, E, w, layers, biases, Wp, F32(bp), acc
