"""H6 on the GPU: partial_fit steps vs the oracle's TF-semantics step
(hand-derived gradients pinned by finite differences in
tests/test_oracle_training.py), and the reference epoch loops end to end.
Gradients are summed with float atomics, so updates agree to ~1e-6
relative, not bitwise.  (The row kernels' raw gradients are held to float64
element by element in tests/test_gpu_train_grad.py.)"""
import argparse
import os

import numpy as np
import pytest
import torch

from oracle import fm_oracle as orc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _rows(rng, B, nu, ni, ctx, td=0):
    cols = [rng.integers(0, nu, B), rng.integers(nu, nu + ni, B)]
    o = nu + ni
    for c in ctx:
        cols.append(rng.integers(o, o + c, B))
        o += c
    for _ in range(td):
        cols.append(rng.integers(nu, nu + ni, B))
    return np.stack(cols, 1).astype(np.int64), o


def _close_update(got, ref, before):
    """Updated parameters agree to 1e-4 of the largest update (atomic
    summation order) and 1e-5 relative."""
    step = np.abs(ref - before).max()
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-4 * step + 1e-9)


OPTS = {"AdagradOptimizer": "adagrad", "GradientDescentOptimizer": "sgd",
        "MomentumOptimizer": "momentum", "AdamOptimizer": "adam"}


def _slot(o, v):
    """The oracle's initial slot for variable v (TF: Adagrad 0.1, Momentum 0,
    Adam m = v = 0 stacked flat)."""
    v = np.asarray(v, np.float32)
    return {"adagrad": np.full_like(v, 0.1), "momentum": np.zeros_like(v),
            "adam": np.zeros(2 * v.size, np.float32), "sgd": None}[o]


def _check_var(got, ref, before, o, grad):
    """_close_update, except under Adam: its early steps move an element by
    ≈ ±α whatever |g| is, so its update error is ≈ 3·α_t·δg/|g| for a
    gradient error δg (d(m̂/√v̂)/dg ≈ (1−β1)/√v̂, √v̂ ≥ √(1−β2)·|g|).  The
    float atomics' summation order gives δg up to ~1e-6 of the table row's
    largest |g| (a row's k elements sum over the same rows), so table
    elements with |g| ≥ 1e-2 of that are held to 1e-4 of the largest step (a
    1e-4 cut-off failed once among round 6's GPU runs); a vector's elements
    sum over different rows each (noise ∝ the element's own terms), so there
    the cut-off stays 1e-4 of the largest |g|.  The rest (~2 %) only to ≤ 2 ×
    the largest step."""
    got, ref, before = (np.asarray(x, np.float32) for x in (got, ref, before))
    if o != "adam":
        _close_update(got, ref, before)
        return
    g = np.abs(np.asarray(grad, np.float32).reshape(ref.shape))
    scale = g.max(axis=-1, keepdims=True) if g.ndim == 2 else g.max(initial=0.0)
    well = g >= (1e-2 if g.ndim == 2 else 1e-4) * scale
    step = np.abs(ref - before).max()
    off = well & ~np.isclose(got, ref, rtol=1e-5, atol=1e-4 * step + 1e-9)
    gs = g / np.maximum(scale, 1e-30)
    assert not off.any(), (f"{off.sum()} elements: |g|/row max {gs[off][:8]}, "
                           f"|got-ref| {np.abs(got - ref)[off][:8]}, step {step}")
    assert np.all(np.abs(got - ref) <= 2.01 * step + 1e-9)
    assert (well & (g > 0)).sum() >= 0.9 * (g > 0).sum()


def _check_slot(got, ref, o):
    if o == "sgd":
        return
    ref = np.asarray(ref, np.float32).reshape(-1)
    got = np.asarray(got, np.float32).reshape(-1)
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max() + 1e-12)


def _slots_of(m, names, o, cur):
    st = getattr(m, "_train_state", None)
    if st is None:
        return [_slot(o, v) for v in cur]
    return [None if o == "sgd" else st[n].cpu().numpy() for n in names]


FM_CASES = [("AdagradOptimizer", 0.1), ("GradientDescentOptimizer", 0.1),
            ("AdagradOptimizer", 0.0), ("MomentumOptimizer", 0.1), ("MomentumOptimizer", 0.0),
            ("AdamOptimizer", 0.1), ("AdamOptimizer", 0.0)]


FM_NAMES = ["feature_embeddings", "feature_bias", "bias"]


def _fm_model(rng, opt, lam, nu, ni, k, ctx=(7, 2, 3)):
    from hhfm_amd.FM import FM
    M = nu + ni + sum(ctx)
    m = FM(2 + len(ctx), M, nu, ni, k, 0.1, lam, 1, opt, 0, 0)
    E = rng.normal(0, 0.01, (M, k)).astype(np.float32)
    w = rng.normal(0, 0.01, M).astype(np.float32)
    m.set_weights(feature_embeddings=E, feature_bias=w[:, None], bias=np.float32(0.02))
    return m


def _fm_replay(m, Xb, y, o, lam, step):
    """One FM partial_fit, replayed by the oracle from the GPU's own pre-step
    parameters and slots (step: 1-based, Adam's t)."""
    Wg = m.get_weights()
    cur = [Wg["feature_embeddings"], Wg["feature_bias"][:, 0], np.float32(Wg["bias"])]
    sl = _slots_of(m, FM_NAMES, o, cur)
    loss = m.partial_fit({"X": Xb, "Y": y})
    rl, E1, w1, w01, aE, aw, a0 = orc.fm_train_step(Xb, y, *cur, *sl, 0.1, lam, o, step)
    _, Eg, wg, w0g, *_ = orc.fm_train_step(Xb, y, *cur, None, None, None, 1.0, lam, "sgd")
    assert np.isclose(loss, rl, rtol=1e-5)
    Wn = m.get_weights()
    _check_var(Wn["feature_embeddings"], E1, cur[0], o, cur[0] - Eg)
    _check_var(Wn["feature_bias"][:, 0], w1, cur[1], o, cur[1] - wg)
    _check_var(np.float32(Wn["bias"]).reshape(1), np.float32(w01).reshape(1),
               np.float32(cur[2]).reshape(1), o, np.float32(cur[2] - w0g).reshape(1))
    for n, r in zip(FM_NAMES, (aE, aw, a0)):
        if o != "sgd":
            _check_slot(m._train_state[n].cpu().numpy(), r, o)


@pytest.mark.parametrize("opt,lam", FM_CASES)
def test_fm_partial_fit_matches_oracle(opt, lam):
    """FM partial_fit (FM.py:123-136, 168-171) under each --optimizer, with
    the l2 term (E's gradient dense) and without it (E an IndexedSlices: the
    sparse Momentum / Adam rules).  Each step is replayed by the oracle from
    the GPU's own pre-step parameters and slots; Adam's β powers are the
    GPU's to carry (3 steps)."""
    rng = np.random.default_rng(0)
    nu, ni, k = 200, 500, 32
    X, M = _rows(rng, 5000, nu, ni, (7, 2, 3))
    m = _fm_model(rng, opt, lam, nu, ni, k)
    for step in range(3):
        Xb = X[step * 1500:(step + 1) * 1500]
        y = rng.integers(0, 2, len(Xb)).astype(np.float32)[:, None]
        _fm_replay(m, Xb, y, OPTS[opt], lam, step + 1)


ALL_OPT_LAM = [(o, lam) for o in OPTS for lam in (0.0, 0.1)]


@pytest.mark.parametrize("opt,lam", ALL_OPT_LAM)
def test_fm_partial_fit_k128(opt, lam):
    """The same at k = 128 (main.py's factor): each lane of `fm_train_rows`
    takes two columns of the row.  Every optimizer with and without the l2
    term, 3 steps of 200 rows."""
    rng = np.random.default_rng(10)
    nu, ni = 20, 50
    X, M = _rows(rng, 600, nu, ni, (7, 2, 3))
    m = _fm_model(rng, opt, lam, nu, ni, 128)
    for step in range(3):
        Xb = X[step * 200:(step + 1) * 200]
        y = rng.integers(0, 2, len(Xb)).astype(np.float32)[:, None]
        _fm_replay(m, Xb, y, OPTS[opt], lam, step + 1)


def _fm_adam_powers(m):
    """The FM train workspace's Adam scalars [β1^t, β2^t, started]
    (train.hip: scal = dE [M·k] + dw [M] floats in)."""
    M, k = m.weights["feature_embeddings"].shape
    o = M * k + M + 8
    return m._train_state["ws"].view(torch.float32)[o:o + 3]


def test_fm_adam_past_beta1_power_underflow():
    """β1^t = 0.9^t underflows to exactly 0 at t = 829 under TF's
    flush-to-zero and TF keeps using 0 (AdamOptimizer._finish multiplies the
    power each step), so a zero power must not read as "not started" (the
    round-4 kernels restarted the powers there: α jumped ~10×).  860 tiny
    Adam steps: the powers the GPU carries equal adam_powers(t + 1) bit for
    bit at every checked step, and each step from t = 822 on (across the
    underflow) is replayed by the oracle from the GPU's own pre-step
    parameters and slots."""
    from hhfm_amd.FM import FM
    rng = np.random.default_rng(5)
    nu, ni, k = 20, 30, 8
    X, M = _rows(rng, 64 * 860, nu, ni, (7, 2, 3))
    Y = rng.integers(0, 2, len(X)).astype(np.float32)[:, None]
    m = FM(5, M, nu, ni, k, 0.01, 0.1, 1, "AdamOptimizer", 0, 0)
    m.set_weights(feature_embeddings=rng.normal(0, 0.01, (M, k)).astype(np.float32),
                  feature_bias=rng.normal(0, 0.01, (M, 1)).astype(np.float32),
                  bias=np.float32(0.02))
    names = ["feature_embeddings", "feature_bias", "bias"]
    crossed = False
    for t in range(1, 861):
        Xb, yb = X[(t - 1) * 64:t * 64], Y[(t - 1) * 64:t * 64]
        if t < 822:
            m.partial_fit({"X": Xb, "Y": yb})
            if t % 97 == 0:
                b1, b2 = orc.adam_powers(t + 1)
                assert _fm_adam_powers(m).cpu().numpy().tolist() == [b1, b2, 1.0]
            continue
        Wg = m.get_weights()
        cur = [Wg["feature_embeddings"], Wg["feature_bias"][:, 0], np.float32(Wg["bias"])]
        sl = _slots_of(m, names, "adam", cur)
        loss = m.partial_fit({"X": Xb, "Y": yb})
        rl, E1, w1, w01, aE, aw, a0 = orc.fm_train_step(Xb, yb, *cur, *sl, 0.01, 0.1, "adam", t)
        _, Eg, wg, w0g, *_ = orc.fm_train_step(Xb, yb, *cur, None, None, None, 1.0, 0.1, "sgd")
        assert np.isclose(loss, rl, rtol=1e-5)
        Wn = m.get_weights()
        _check_var(Wn["feature_embeddings"], E1, cur[0], "adam", cur[0] - Eg)
        _check_var(Wn["feature_bias"][:, 0], w1, cur[1], "adam", cur[1] - wg)
        b1, b2 = orc.adam_powers(t + 1)
        assert _fm_adam_powers(m).cpu().numpy().tolist() == [b1, b2, 1.0]
        crossed |= b1 == 0.0
    assert crossed


HHFM_CASES = [("frappe", "AdagradOptimizer", 0.01), ("jiaju", "AdagradOptimizer", 0.01),
              ("frappe", "MomentumOptimizer", 0.0), ("jiaju", "MomentumOptimizer", 0.01),
              ("frappe", "AdamOptimizer", 0.0), ("jiaju", "AdamOptimizer", 0.01),
              ("frappe", "GradientDescentOptimizer", 0.0)]


@pytest.mark.parametrize("layout,opt,lam", HHFM_CASES)
def test_hhfm_partial_fit_matches_oracle(layout, opt, lam):
    """OUR partial_fit (OurModel7.py:171-193, 219-228) under each --optimizer;
    λ = 0 leaves the table's gradient an IndexedSlices over X and Neg."""
    _hhfm_steps(layout, opt, lam, np.random.default_rng(1), 300, 800, 32, 1500)


HHFM_LAYOUTS = {"frappe": ((7, 2, 3), 0), "jiaju": ((5, 4, 6, 3, 7), 3)}   # ctx values, time columns


def _hhfm_model(rng, layout, opt, lam, nu, ni, k):
    from hhfm_amd.OurModel7 import OUR
    ctx, td = HHFM_LAYOUTS[layout]
    M = nu + ni + sum(ctx)
    m = OUR(len(ctx), td, M, nu, ni, k, 0.1, lam, opt, True, td > 0)
    m.set_weights(feature_embeddings=rng.normal(0, 0.01, (M, k)).astype(np.float32))
    return m


def _hhfm_replay(m, Xb, Neg, o, lam, step):
    """One OUR partial_fit, replayed by the oracle from the GPU's own pre-step
    table and slot."""
    fd, td = m.feature_dimension, m.time_dimension if m.time else 0
    E = m.get_weights()["feature_embeddings"]
    (accE,) = _slots_of(m, ["feature_embeddings"], o, [E])
    data = {"X": Xb[:, :2], "Y": Neg, "F1": Xb[:, 2:2 + fd]}
    if td:
        data["F2"] = Xb[:, 2 + fd:]
    loss = m.partial_fit(data)
    rl, E1, acc1 = orc.hhfm_train_step(Xb, Neg, E, accE, 0.1, lam, fd, td, True, td > 0, o, step)
    _, Eg, _ = orc.hhfm_train_step(Xb, Neg, E, None, 1.0, lam, fd, td, True, td > 0, "sgd")
    assert np.isclose(loss, rl, rtol=1e-5)
    _check_var(m.get_weights()["feature_embeddings"], E1, E, o, E - Eg)
    if o != "sgd":
        _check_slot(m._train_state["feature_embeddings"].cpu().numpy(), acc1, o)


def _hhfm_steps(layout, opt, lam, rng, nu, ni, k, B):
    ctx, td = HHFM_LAYOUTS[layout]
    X, M = _rows(rng, 3 * B, nu, ni, ctx, td)
    m = _hhfm_model(rng, layout, opt, lam, nu, ni, k)
    for step in range(3):
        Xb = X[step * B:(step + 1) * B]
        Neg = rng.integers(nu, nu + ni, (len(Xb), 10))
        _hhfm_replay(m, Xb, Neg, OPTS[opt], lam, step + 1)


@pytest.mark.parametrize("opt,lam", ALL_OPT_LAM)
def test_hhfm_partial_fit_k128(opt, lam):
    """The same at k = 128 (two columns per lane in `hhfm_train_rows`), context
    + time columns: every optimizer with and without the l2 term, 3 steps of
    200 rows."""
    _hhfm_steps("jiaju", opt, lam, np.random.default_rng(11), 30, 80, 128, 200)


def _args(tmp_path, **kw):
    a = dict(path=G + "/", dataset="synth_frappe", epoch=3, batch_size=5000, hidden_factor=32,
             lamda=0.1, keep=1, lr=0.1, optimizer="AdagradOptimizer", verbose=1, batch_norm=0,
             TopK=10, Result=0, result_file=str(tmp_path / "result.txt"))
    a.update(kw)
    return argparse.Namespace(**a)


def test_fm_train_loop_end_to_end(tmp_path):
    from hhfm_amd.FM import Train
    np.random.seed(2016)
    t = Train(_args(tmp_path))
    losses = t.train()
    assert len(losses) == 2 and losses[1] < losses[0]
    log = open(tmp_path / "result.txt").read()
    assert "Init" in log and "FM Epoch 1" in log


def test_hhfm_train_loop_end_to_end(tmp_path):
    from hhfm_amd.OurModel7 import Train
    np.random.seed(2016)
    t = Train(_args(tmp_path, lamda=0.01, epoch=11))
    losses = t.train()
    assert len(losses) == 10 and losses[-1] < losses[0]
    assert "M7 Epoch 10" in open(tmp_path / "result.txt").read()


@pytest.mark.parametrize("k,layers,B", [
    (16, [24, 40, 24], 301),        # ragged batch, widths not multiples of 8
    (32, [150, 200, 150], 1000),    # the reference's MLP (DFM.py:256)
    (8, [12], 7),                   # one layer, tiny batch
    (8, [10, 7, 3], 9),             # widths that are no multiple of 4 or 8
    (8, [1], 9),                    # one hidden unit
    (8, [1011], 9),                 # concat width F + k + d_L = 1024: 16 columns per lane
])
def test_dfm_partial_fit_matches_oracle(k, layers, B):
    """DeepFM partial_fit (DFM.py:139-155): every variable after two Adagrad
    steps vs the oracle's TF-semantics step."""
    from hhfm_amd.DFM import DeepFM
    rng = np.random.default_rng(k + B)
    nu, ni = 60, 200
    X, M = _rows(rng, 2 * B, nu, ni, (7, 2, 3))
    m = DeepFM(nu, ni, M, 5, k, layers, None, 0.01, 0, 0.01)
    W = m.get_weights()
    L = len(layers)
    E, w = W["feature_embeddings"], W["feature_bias"][:, 0]
    Ls = [W[f"layer_{i}"] for i in range(L)]
    bs = [W[f"bias_{i}"][0] for i in range(L)]
    Wp, bp = W["concat_projection"][:, 0], np.float32(W["concat_bias"])
    keys = ["E", "w"] + [f"W{i}" for i in range(L)] + [f"b{i}" for i in range(L)] + ["Wp", "bp"]
    vals = [E, w] + Ls + bs + [Wp, bp]
    acc = {kk: np.full_like(np.asarray(v, np.float32), 0.1) for kk, v in zip(keys, vals)}
    for step in range(2):
        Xb = X[step * B:(step + 1) * B]
        y = rng.choice([1.0, -1.0], B).astype(np.float32)[:, None]
        loss = m.partial_fit({"X": Xb, "Y": y})
        rl, E1, w1, L1, b1, Wp1, bp1, acc = orc.dfm_train_step(Xb, y, E, w, Ls, bs, Wp, bp, acc,
                                                               0.01, 0.01)
        assert np.isclose(loss, rl, rtol=1e-5)
        G = m.get_weights()
        _close_update(G["feature_embeddings"], E1, E)
        _close_update(G["feature_bias"][:, 0], w1, w)
        for i in range(L):
            _close_update(G[f"layer_{i}"], L1[i], Ls[i])
            _close_update(G[f"bias_{i}"][0], b1[i], bs[i])
        _close_update(G["concat_projection"][:, 0], Wp1, Wp)
        assert np.isclose(float(G["concat_bias"]), bp1, rtol=1e-5, atol=1e-4 * abs(bp1 - bp))
        E, w, Ls, bs, Wp, bp = E1, w1, L1, b1, Wp1, bp1
    # the scoring path sees the updated weights: the oracle forward on the
    # GPU's own trained weights (the training comparison above carries the
    # float-atomics noise; the forward alone is held to 1e-5)
    G = m.get_weights()
    Xs = X[:50]
    ref = orc.dfm_out(Xs, G["feature_embeddings"], G["feature_bias"][:, 0],
                      [G[f"layer_{i}"] for i in range(L)], [G[f"bias_{i}"] for i in range(L)],
                      G["concat_projection"], np.float32(G["concat_bias"]))[:, 0]
    got = m.score_rows(Xs)[:, 0]
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def _dfm_names(L):
    return (["feature_embeddings", "feature_bias"] + [f"layer_{i}" for i in range(L)]
            + [f"bias_{i}" for i in range(L)] + ["concat_projection", "concat_bias"])


def _dfm_keys(L):
    return ["E", "w"] + [f"W{i}" for i in range(L)] + [f"b{i}" for i in range(L)] + ["Wp", "bp"]


class _DfmBinding:
    """hhfm_dfm_train_step on a DeepFM model's weights under any optimizer
    (DeepFM.partial_fit itself is the reference's Adagrad, DFM.py:155): the
    slots and the workspace are kept here, grown as training.dfm_partial_fit
    grows them."""

    def __init__(self, m, o, lr, lam):
        from hhfm_amd import training
        self.m, self.o, self.lr, self.lam = m, o, lr, lam
        self.opt = training._OPT[{v: n for n, v in OPTS.items()}[o]]
        self.names = _dfm_names(len(m.deep_layers))
        self.slots = {n: training._slots(self.opt, m.weights[n]) for n in self.names}
        self.ws, self.ws_rows = None, -1
        self.loss = torch.zeros(1, device=m.device)

    def workspace(self, B):
        from hhfm_amd import training
        from hhfm_amd._native import native
        m = self.m
        M, k = m.weights["feature_embeddings"].shape
        if self.ws_rows < B:
            n = native().dfm_train_workspace(B, m.field_size, k, M, m.deep_layers)
            self.ws = training._grow(self.ws, n, native().dfm_train_state_bytes(
                m.field_size, k, M, m.deep_layers), m.device)
            self.ws_rows = B
        return self.ws

    def step(self, Xb, y, ws_bytes=None):
        from hhfm_amd._native import native
        m, W = self.m, self.m.weights
        L = len(m.deep_layers)
        X = m._idx(Xb)
        yd = torch.as_tensor(np.asarray(y, np.float32).reshape(-1)).to(m.device)
        M, k = W["feature_embeddings"].shape
        ws = self.workspace(len(Xb))
        ptr = lambda n: W[n].data_ptr()  # noqa: E731
        native().dfm_train_step(
            X.data_ptr(), yd.data_ptr(), len(Xb), X.shape[1], ptr("feature_embeddings"),
            ptr("feature_bias"), M, k, m.deep_layers, [ptr(f"layer_{i}") for i in range(L)],
            [ptr(f"bias_{i}") for i in range(L)], ptr("concat_projection"), ptr("concat_bias"),
            self.lr, self.lam, self.opt,
            [self.slots[n].data_ptr() for n in self.names] if self.o != "sgd" else [],
            ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, self.loss.data_ptr(),
            torch.cuda.current_stream().cuda_stream)
        m._prep = None
        return float(self.loss.item())

    def slot(self, n):
        return None if self.o == "sgd" else self.slots[n].cpu().numpy()


def _dfm_vars(m):
    W = m.get_weights()
    L = len(m.deep_layers)
    return (W["feature_embeddings"], W["feature_bias"][:, 0], [W[f"layer_{i}"] for i in range(L)],
            [W[f"bias_{i}"][0] for i in range(L)], W["concat_projection"][:, 0],
            np.float32(W["concat_bias"]))


def _dfm_flat(E, w, Ls, bs, Wp, bp):
    return [E, w] + list(Ls) + list(bs) + [Wp, np.float32(bp).reshape(1)]


def _dfm_layer_mags(X, y, E, w, Ls, bs, Wp, bp):
    """Σ_b |h_bi · dz_bj| of every layer's dW = H_iᵀ·dZ_{i+1}, and last
    Σ_b |concat_bc · g_b| of dWp (float64): the magnitude an fp32 sum over the
    batch errs against."""
    X = np.asarray(X, np.int64)
    y = np.asarray(y, np.float64).reshape(-1)
    e = np.asarray(E, np.float64)[X]
    B, F, k = e.shape
    s = e.sum(1)
    hs = [e.reshape(B, F * k)]
    for W, b in zip(Ls, bs):
        hs.append(np.maximum(hs[-1] @ np.asarray(W, np.float64) + np.asarray(b, np.float64), 0))
    cat = np.concatenate([np.asarray(w, np.float64)[X], 0.5 * (s * s - (e * e).sum(1)), hs[-1]], 1)
    g = cat @ np.asarray(Wp, np.float64) + float(bp) - y
    dh = g[:, None] * np.asarray(Wp, np.float64)[None, F + k:]
    mags = [None] * len(Ls) + [np.abs(cat).T @ np.abs(g)]
    for i in range(len(Ls) - 1, -1, -1):
        dz = dh * (hs[i + 1] > 0)
        mags[i] = np.abs(hs[i]).T @ np.abs(dz)
        dh = dz @ np.asarray(Ls[i], np.float64).T
    return mags


def _check_layer_adam(got, ref, before, grad, mag):
    """_check_var's Adam rule for a layer's weight matrix or the concat
    projection.  Such a gradient is a dense sum over the batch, not a scatter
    into table rows: an element's noise is ∝ its own Σ_b |h_bi · dz_bj|
    (``mag``), and the elements of one variable span orders of magnitude
    (rarely active units; Wp's y1, y2 and h_L columns), so "well-conditioned"
    is taken per element: κ = mag / |g| <= 100 (oracle/parity.KAPPA_MAX).  Those are
    held to 1e-4 of the largest step (3·α·δg/|g| with δg ~ 1e-7 · mag), the
    rest to <= 2 × the largest step.  A sum of n random-sign terms has κ > 100
    with probability ≈ 0.008·√n (~10 % at n = 150 active rows), so at least
    three quarters of the moving elements must be the tightly held kind."""
    g = np.abs(grad)
    well = g * 100 >= mag
    step = np.abs(ref - before).max()
    off = well & ~np.isclose(got, ref, rtol=1e-5, atol=1e-4 * step + 1e-9)
    assert not off.any(), (f"{off.sum()} elements: κ {(mag / np.maximum(g, 1e-30))[off][:8]}, "
                           f"|got-ref| {np.abs(got - ref)[off][:8]}, step {step}")
    assert np.all(np.abs(got - ref) <= 2.01 * step + 1e-9)
    assert (well & (g > 0)).sum() >= 0.75 * (g > 0).sum()


def _dfm_replay(m, step_fn, slot_fn, Xb, y, o, lr, lam, step):
    """One DeepFM step (``step_fn``), replayed by the oracle from the GPU's
    own pre-step parameters and slots (``slot_fn(name)``)."""
    L = len(m.deep_layers)
    cur = _dfm_vars(m)
    acc = {kk: slot_fn(n) for kk, n in zip(_dfm_keys(L), _dfm_names(L)) if o != "sgd"}
    loss = step_fn(Xb, y)
    rl, *new, acc1 = orc.dfm_train_step(Xb, y, *cur, acc, lr, lam, optimizer=o, step=step)
    _, *gnew, _ = orc.dfm_train_step(Xb, y, *cur, {}, 1.0, lam, optimizer="sgd")
    assert np.isclose(loss, rl, rtol=1e-5), (loss, rl)
    got = _dfm_flat(*_dfm_vars(m))
    mags = _dfm_layer_mags(Xb, y, *cur) if o == "adam" else None
    for kk, n, g, v_new, v_old, v_g in zip(_dfm_keys(L), _dfm_names(L), got, _dfm_flat(*new),
                                           _dfm_flat(*cur), _dfm_flat(*gnew)):
        v_old, v_new = np.asarray(v_old, np.float32), np.asarray(v_new, np.float32)
        v_g = v_old - np.asarray(v_g, np.float32)
        if o == "adam" and kk[0] == "W":
            _check_layer_adam(g, v_new, v_old, v_g, mags[-1 if kk == "Wp" else int(kk[1:])])
        else:
            _check_var(g, v_new, v_old, o, v_g)
        if o != "sgd":
            _check_slot(slot_fn(n), acc1[kk], o)


@pytest.mark.parametrize("opt", ["GradientDescentOptimizer", "MomentumOptimizer", "AdamOptimizer"])
@pytest.mark.parametrize("k,layers,B", [(8, [12], 7), (16, [24, 40, 24], 301)])
def test_dfm_binding_other_optimizers(k, layers, B, opt):
    """hhfm_dfm_train_step takes all four optimizers although DeepFM.partial_fit
    only runs Adagrad: SGD, Momentum and Adam through the binding, two steps,
    every variable and slot against the oracle's step."""
    from hhfm_amd.DFM import DeepFM
    rng = np.random.default_rng(k + B)
    nu, ni = 60, 200
    X, M = _rows(rng, 2 * B, nu, ni, (7, 2, 3))
    m = DeepFM(nu, ni, M, 5, k, layers, None, 0.01, 0, 0.01)
    o = OPTS[opt]
    drv = _DfmBinding(m, o, 0.01, 0.01)
    for step in range(2):
        y = rng.choice([1.0, -1.0], B).astype(np.float32)[:, None]
        _dfm_replay(m, drv.step, drv.slot, X[step * B:(step + 1) * B], y, o, 0.01, 0.01, step + 1)


def test_dfm_train_loop_end_to_end(tmp_path):
    from hhfm_amd.DFM import Train
    np.random.seed(2016)
    t = Train(_args(tmp_path, lamda=0.01, lr=0.01, epoch=3, hidden_factor=16))
    losses = t.train()
    assert len(losses) == 2 and losses[1] < losses[0]
    assert "DFM Epoch 1" in open(tmp_path / "result.txt").read()


AFM_NAMES = ["feature_embeddings", "feature_bias", "bias", "attention_W", "attention_b",
             "attention_p", "prediction"]
AFM_KEYS = ["E", "w", "w0", "W", "b", "p", "P"]


def _afm_model(rng, k, A, M, F, opt, nu, ni, lr=0.1):
    from hhfm_amd.AFM import AFM
    m = AFM(nu, ni, M, 1, [A, k], None, lr, 100.0, [1, 1], opt, 0.999, F)
    W = m.get_weights()
    W["feature_bias"] = rng.normal(0, 0.01, (M, 1)).astype(np.float32)
    W["prediction"] = rng.normal(1, 0.2, (k, 1)).astype(np.float32)
    m.set_weights(feature_bias=W["feature_bias"], prediction=W["prediction"])
    if opt in ("MomentumOptimizer", "AdamOptimizer"):
        # at the 0.01 init every pair's pre-activation has the sign of its
        # bias, so d attention_b = p · Σ_pairs dlogit = 0 exactly and both
        # sides hold only summation noise in that slot: spread the pairs
        m.set_weights(feature_embeddings=rng.normal(0, 0.3, (M, k)).astype(np.float32))
    return m


def _afm_replay(m, Xb, y, o, step, lam=100.0):
    """One AFM partial_fit, replayed by the oracle from the GPU's own pre-step
    parameters and slots (lam: the model's lamda_attention; its learning rate
    is read off the model)."""
    lr = m.learning_rate
    G = m.get_weights()
    cur = [np.asarray(G[n], np.float32) for n in AFM_NAMES]
    cur[2] = cur[2].reshape(())
    acc = {kk: v for kk, v in zip(AFM_KEYS, _slots_of(m, AFM_NAMES, o, cur)) if v is not None}
    loss = m.partial_fit({"X": Xb, "Y": y})
    rl, *new, acc = orc.afm_train_step(Xb, y, *cur, acc, lr, lam, optimizer=o, step=step)
    _, *gnew, _ = orc.afm_train_step(Xb, y, *cur, {}, 1.0, lam, optimizer="sgd")
    assert np.isclose(loss, rl, rtol=1e-5), (loss, rl)
    G = m.get_weights()
    for n, kk, v_new, v_old, v_g in zip(AFM_NAMES, AFM_KEYS, new, cur, gnew):
        got = np.asarray(G[n], np.float32).reshape(np.shape(v_new))
        _check_var(got, np.asarray(v_new, np.float32), v_old, o,
                   np.asarray(v_old, np.float32) - np.asarray(v_g, np.float32).reshape(
                       np.shape(v_old)))
        if o != "sgd":
            _check_slot(m._train_state[n].cpu().numpy(), acc[kk], o)


@pytest.mark.parametrize("k,A,ctx,B,opt", [
    (64, 64, (7, 2, 3), 1000, "AdagradOptimizer"),       # Frappe F=5, the reference's k=A
    (16, 32, (5, 4, 6, 3, 7, 2, 2, 3, 4, 3), 301, "AdagradOptimizer"),   # F=12 (resturant/ml width), ragged
    (8, 4, (), 7, "GradientDescentOptimizer"),            # F=2: one pair, tiny batch
    (128, 128, (7, 2, 3), 600, "AdagradOptimizer"),       # main.py's factor 128
    (16, 32, (7, 2, 3), 301, "MomentumOptimizer"),        # AFM.py:157-158
    (32, 16, (5, 4, 6), 500, "AdamOptimizer"),            # AFM.py:151-152
    (16, 8, (7,), 1500, "AdagradOptimizer"),              # B > 1024: a wave of the head takes a 2nd row
    (8, 8, (3,) * 14, 40, "AdagradOptimizer"),            # F = 16: np = 120, the maximum
    (256, 256, (7,), 9, "AdagradOptimizer"),              # k = A = 256: all four chunks per lane
    (68, 12, (7, 2), 130, "AdagradOptimizer"),            # k = 68: a partial second chunk
    (4, 4, (), 1, "AdagradOptimizer"),                    # the smallest step
])
def test_afm_partial_fit_matches_oracle(k, A, ctx, B, opt):
    """AFM partial_fit (AFM.py:144-156, 205-207): every variable after two
    steps vs the oracle's TF-semantics step."""
    rng = np.random.default_rng(k + A + B)
    nu, ni = 60, 200
    X, M = _rows(rng, 2 * B, nu, ni, ctx)
    m = _afm_model(rng, k, A, M, X.shape[1], opt, nu, ni)
    for step in range(2):
        y = rng.choice([1.0, -1.0], B).astype(np.float32)[:, None]
        _afm_replay(m, X[step * B:(step + 1) * B], y, OPTS[opt], step + 1)
    # the scoring path sees the updated weights
    G = m.get_weights()
    cur = [np.asarray(G[n], np.float32) for n in AFM_NAMES]
    Xs = X[:50]
    ref = orc.afm_out(Xs, cur[0], cur[1], cur[2].reshape(()), cur[3], cur[4], cur[5],
                      cur[6])[:, 0]
    got = m.score_rows(Xs)[:, 0]
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def test_afm_train_loop_end_to_end(tmp_path):
    from hhfm_amd.AFM import Train
    np.random.seed(2016)
    t = Train(_args(tmp_path, hidden_factor="[16,16]", keep="[1,1]", lamda_attention=100.0,
                    attention=1, decay=0.999, activation="relu"))
    losses = t.train()
    assert len(losses) == 2 and losses[1] < losses[0]
    assert "AFM Epoch 1" in open(tmp_path / "result.txt").read()


def _plan_adam_powers(ws):
    """Adam's [β1^t, β2^t, started] in an AFM / DeepFM train workspace: the
    plans' off_scal (0) + 8 floats (train.hip afm_train_plan / dfm_train_plan)."""
    return ws.view(torch.float32)[8:11].cpu().numpy().tolist()


def _dfm_class_step(m):
    """(step_fn, slot_fn) of DeepFM.partial_fit for _dfm_replay."""
    def slot(n):
        st = getattr(m, "_train_state", None)
        return st[n].cpu().numpy() if st else _slot("adagrad", m.get_weights()[n])
    return (lambda Xb, y: m.partial_fit({"X": Xb, "Y": y})), slot


BATCHES = [301, 77, 301, 400, 5]


@pytest.mark.parametrize("model,opt", [("afm", "AdamOptimizer"), ("afm", "MomentumOptimizer"),
                                       ("dfm", "AdagradOptimizer"), ("fm", "AdamOptimizer")])
def test_varying_batch_matches_oracle(model, opt):
    """Batches of 301, 77, 301, 400 and 5 rows on one model: a smaller batch
    moves every per-batch offset of the AFM / DeepFM workspace and a larger
    one regrows it (training._grow copies the persistent prefix: gradient
    buffers, Adam's β powers, the touched mask).  Every step is replayed by
    the oracle from the GPU's own pre-step parameters and slots, and the β
    powers in the workspace equal TF's bit for bit after every step — a
    prefix one float short, or a gradient buffer left in the per-batch part,
    shows here."""
    rng = np.random.default_rng(7)
    nu, ni, o = 60, 200, OPTS[opt]
    X, M = _rows(rng, sum(BATCHES), nu, ni, (7, 2, 3))
    if model == "afm":
        # lr 0.01: Momentum(0.95) at 0.1 leaves the 0.3-spread table at 1e12 by
        # the fifth step, where two fp32 runs no longer compare.  attention_b
        # near 0: a unit whose relu is open on every pair of a row gets
        # p · Σ_pairs dlogit = 0 from it, and in a 5-row batch most units of
        # the default init would hold nothing but that summation noise
        m = _afm_model(rng, 16, 32, M, 5, opt, nu, ni, lr=0.01)
        m.set_weights(attention_b=rng.normal(0, 0.01, (1, 32)).astype(np.float32))
    elif model == "dfm":
        from hhfm_amd.DFM import DeepFM
        m = DeepFM(nu, ni, M, 5, 16, [24, 40, 24], None, 0.01, 0, 0.01)
        step_fn, slot_fn = _dfm_class_step(m)
    else:
        m = _fm_model(rng, opt, 0.1, nu, ni, 32)
    at = 0
    for t, B in enumerate(BATCHES, 1):
        Xb = X[at:at + B]
        at += B
        if model == "fm":
            _fm_replay(m, Xb, rng.integers(0, 2, B).astype(np.float32)[:, None], o, 0.1, t)
            powers = _fm_adam_powers(m).cpu().numpy().tolist()
        else:
            y = rng.choice([1.0, -1.0], B).astype(np.float32)[:, None]
            if model == "afm":
                _afm_replay(m, Xb, y, o, t)
            else:
                _dfm_replay(m, step_fn, slot_fn, Xb, y, o, 0.01, 0.01, t)
            powers = _plan_adam_powers(m._train_state["ws"])
        if o == "adam":
            b1, b2 = orc.adam_powers(t + 1)
            assert powers == [b1, b2, 1.0], (t, powers)
        else:
            assert powers == [0.0, 0.0, 0.0]


def _params(m):
    return {n: v.clone() for n, v in m.weights.items() if isinstance(v, torch.Tensor)}


def _same(a, b):
    return all(torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)) for n in a)


def _empty_batch_model(model, opt, lam, rng):
    """-> model, full rows X, step(Xb, t) (the step replayed by the oracle)
    and powers() (Adam's β powers in the workspace), for test_empty_batch_*.
    λ: FM / HHFM the table's, AFM attention_W's, DeepFM the layers' and the
    concat projection's."""
    nu, ni, o = 60, 200, OPTS[opt]
    if model == "hhfm":
        ctx, td = HHFM_LAYOUTS["jiaju"]
        X, M = _rows(rng, 50, nu, ni, ctx, td)
        m = _hhfm_model(rng, "jiaju", opt, lam, nu, ni, 16)
        return (m, X, lambda Xb, t: _hhfm_replay(
            m, Xb, rng.integers(nu, nu + ni, (len(Xb), 10)), o, lam, t),
            lambda: _fm_adam_powers(m).cpu().numpy().tolist())
    X, M = _rows(rng, 50, nu, ni, (7, 2, 3))
    if model == "fm":
        m = _fm_model(rng, opt, lam, nu, ni, 16)
        return (m, X, lambda Xb, t: _fm_replay(
            m, Xb, rng.integers(0, 2, len(Xb)).astype(np.float32)[:, None], o, lam, t),
            lambda: _fm_adam_powers(m).cpu().numpy().tolist())
    y = lambda Xb: rng.choice([1.0, -1.0], len(Xb)).astype(np.float32)[:, None]  # noqa: E731
    if model == "afm":
        from hhfm_amd.AFM import AFM
        m = AFM(nu, ni, M, 1, [8, 16], None, 0.1, lam, [1, 1], opt, 0.999, 5)
        m.set_weights(feature_embeddings=rng.normal(0, 0.3, (M, 16)).astype(np.float32))
        return (m, X, lambda Xb, t: _afm_replay(m, Xb, y(Xb), o, t, lam),
                lambda: _plan_adam_powers(m._train_state["ws"]))
    from hhfm_amd.DFM import DeepFM
    m = DeepFM(nu, ni, M, 5, 8, [12, 6], None, 0.01, 0, lam)
    drv = _DfmBinding(m, o, 0.01, lam)
    return (m, X, lambda Xb, t: _dfm_replay(m, drv.step, drv.slot, Xb, y(Xb), o, 0.01, lam, t),
            lambda: _plan_adam_powers(drv.ws))


@pytest.mark.parametrize("model", ["fm", "hhfm", "afm", "dfm"])
def test_empty_batch_with_l2_still_steps(model):
    """A B = 0 step under Adam with λ > 0, after one real step: the l2 term's
    variable (FM / HHFM: the table; AFM: attention_W; DeepFM: the layers and
    the concat projection) still decays, every variable moves as the oracle's
    empty-batch step moves it, and Adam's powers advance."""
    rng = np.random.default_rng(12)
    m, X, step, powers = _empty_batch_model(model, "AdamOptimizer", 0.1, rng)
    step(X, 1)
    before = _params(m)
    step(X[:0], 2)
    reg = {"fm": "feature_embeddings", "hhfm": "feature_embeddings", "afm": "attention_W",
           "dfm": "layer_0"}[model]
    assert not torch.equal(before[reg], m.weights[reg])
    b1, b2 = orc.adam_powers(3)
    assert powers() == [b1, b2, 1.0]


@pytest.mark.parametrize("opt", ["AdagradOptimizer", "MomentumOptimizer", "AdamOptimizer"])
@pytest.mark.parametrize("model", ["fm", "hhfm", "afm", "dfm"])
def test_empty_batch_without_l2_changes_nothing(model, opt):
    """A B = 0 first step with λ = 0: loss 0, every parameter bit for bit as
    it was (as the oracle's empty-batch step leaves it)."""
    rng = np.random.default_rng(13)
    m, X, step, _ = _empty_batch_model(model, opt, 0.0, rng)
    before = _params(m)
    step(X[:0], 1)
    assert _same(before, _params(m))


@pytest.mark.parametrize("entry", ["FM_main", "M7_main", "AFM_main", "DFM_main"])
def test_main_entry_points_through_argv(entry, tmp_path):
    """main.py's surface (Newcode/main.py:47-63 calls X_main(dataname, factor,
    TopK)): each entry point parses the reference's flags from argv, loads
    synth_frappe through LoadData, trains one epoch on the GPU (the loop
    whose batch stream test_epoch_stream.py pins) and appends the
    reference's result lines (Init + epoch 1 at --verbose 1; HHFM evaluates
    at init only before epoch 10, OurModel7.py:404) to --result_file."""
    import importlib
    mod = {"FM_main": "FM", "M7_main": "OurModel7", "AFM_main": "AFM", "DFM_main": "DFM"}[entry]
    fn = getattr(importlib.import_module(f"hhfm_amd.{mod}"), entry)
    out = tmp_path / "result.txt"
    argv = ["--path", G + "/", "--epoch", "2", "--batch_size", "4096",
            "--result_file", str(out)]
    if entry != "M7_main":
        argv += ["--verbose", "1"]
    np.random.seed(2016)
    session = fn("synth_frappe", 16, 5, argv)
    assert len(session.loss_epoch) == 1 and np.isfinite(session.loss_epoch[0])
    lines = out.read_text().splitlines()
    assert lines[0].startswith("Dataset=synth_frappe ") and "Init:" in lines[0]
    assert len(lines) == (1 if entry == "M7_main" else 2), lines
    for ln in lines:
        auc = float(ln.split("train=AUC:")[1].split(";")[0])
        hr = float(ln.split("HR:")[1].split(",")[0])
        assert 0.0 <= auc <= 1.0 and 0.0 <= hr <= 1.0, ln
