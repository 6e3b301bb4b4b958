"""The deterministic AFM / DeepFM training steps (include/hhfm.h "Deterministic
AFM and DeepFM steps"; ``deterministic=True`` of AFM / DeepFM) on the GPU.

1. Known answers: the four inputs of tests/train_det_heads_ref.py, whose
   contributions are exact in fp32 — one SGD step (lr 1, λ 0) moves every
   variable by the documented ordered sums, bit for bit, the loss included.
2. Repeatability: two runs from identical state, batches of 301 → 77 → 400
   rows — every parameter, slot, the workspace and every loss bit for bit.
3. The same arithmetic as the default steps: no id twice in the batch → E and
   w equal bit for bit; B = 1 and B = 0 → everything equal.
4. Parity at the bars of test_gpu_training.py and test_gpu_dropout.py.
5. Arguments: scratch short / NULL, keep = 0, the size functions, bad ids.
6. The model surface: ``--deterministic 1`` trains to the same bits twice.

Measured on an MI355X, largest figures of (4): see DESIGN.md §H6.
"""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import dropout_ref as dref
from tests import train_det_heads_ref as hr
from tests import test_gpu_training as tg

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
ADAGRAD, SGD, MOMENTUM, ADAM = 0, 1, 2, 3
F32 = np.float32
AFM_NAMES = tg.AFM_NAMES


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32).reshape(-1)).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _slot(opt, t):
    if opt == ADAGRAD:
        return torch.full_like(t, 0.1)
    if opt == MOMENTUM:
        return torch.zeros_like(t)
    if opt == ADAM:
        return torch.zeros(2 * t.numel(), device="cuda")
    return None


class _Run:
    """Device state of a run through the binding: parameters (flat float32),
    slots, the zero-filled workspace for ``rows`` rows, and (deterministic) a
    scratch filled with 0xA5 — it need not be zeroed."""

    def _setup(self, par, opt, ws_bytes, state_bytes, sc_bytes, deterministic):
        self.shapes = [np.shape(p) for p in par]
        self.par = [_dev(np.asarray(p, F32).reshape(-1)) for p in par]
        self.opt = opt
        self.acc = [_slot(opt, p) for p in self.par]
        self.ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        self.state_bytes = state_bytes
        self.det = deterministic
        self.sc = (torch.full((sc_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
                   if deterministic else None)
        self.loss = torch.zeros(1, device="cuda")
        self.losses = []

    def _slots(self):
        return [] if self.opt == SGD else [a.data_ptr() for a in self.acc]

    def _call(self, fn_det, fn_def, args, scratch):
        if self.det:
            sc = scratch if scratch is not None else (self.sc.data_ptr(), self.sc.numel())
            fn_det(*args, *sc, self.loss.data_ptr(), _stream())
        else:
            fn_def(*args, self.loss.data_ptr(), _stream())
        self.losses.append(F32(self.loss.item()))
        return self.losses[-1]

    def params(self):
        torch.cuda.synchronize()
        return [p.cpu().numpy().reshape(s) for p, s in zip(self.par, self.shapes)]

    def state(self, whole_ws=True):
        """Every parameter, every slot, the workspace (all of it, or its
        persistent prefix: zero but Adam's β powers) and the returned losses."""
        ws = self.ws.cpu().numpy()
        out = self.params() + [a.cpu().numpy() for a in self.acc if a is not None]
        out += [(ws if whole_ws else ws[:self.state_bytes]).view(np.uint32),
                np.asarray(self.losses, F32)]
        return out


class _Afm(_Run):
    """par = (E, w, w0, W, b, pvec, P)."""

    def __init__(self, par, opt, rows, F, deterministic=True):
        from hhfm_amd._native import native
        self.nat = native()
        (self.M, self.k), self.A, self.F = par[0].shape, par[3].shape[1], F
        dims = (F, self.k, self.A, self.M)
        self._setup(par, opt, self.nat.afm_train_workspace(rows, *dims),
                    self.nat.afm_train_state_bytes(*dims),
                    self.nat.afm_train_det_scratch(rows, *dims), deterministic)

    def step(self, X, y, lr, lam, keep=(1.0, 1.0), seed=0, scratch=None):
        B = len(X)
        Xd, yd = _dev(X.astype(np.int32)), _dev(np.asarray(y, F32).reshape(-1))
        p = [t.data_ptr() for t in self.par]
        args = (Xd.data_ptr() if B else 0, yd.data_ptr() if B else 0, B, self.F, *p[:3], self.M,
                self.k, self.A, *p[3:], lr, lam, self.opt, keep[0], keep[1], seed, self._slots(),
                self.ws.data_ptr(), self.ws.numel())
        return self._call(self.nat.afm_train_step_det, self.nat.afm_train_step_ex, args, scratch)


class _Dfm(_Run):
    """par = (E, w, layers, biases, Wp, bp), kept flat in the binding's slot
    order E, w, W_0.., b_0.., Wp, bp."""

    def __init__(self, par, opt, rows, F, deterministic=True):
        from hhfm_amd._native import native
        self.nat = native()
        E, w, layers, biases, Wp, bp = par
        self.L = len(layers)
        (self.M, self.k), self.F = E.shape, F
        self.dims = [int(W.shape[1]) for W in layers]
        dims = (F, self.k, self.M, self.dims)
        self._setup([E, w, *layers, *biases, Wp, bp], opt,
                    self.nat.dfm_train_workspace(rows, *dims),
                    self.nat.dfm_train_state_bytes(*dims),
                    self.nat.dfm_train_det_scratch(rows, *dims), deterministic)

    def step(self, X, y, lr, lam, scratch=None):
        B, L = len(X), self.L
        Xd, yd = _dev(X.astype(np.int32)), _dev(np.asarray(y, F32).reshape(-1))
        p = [t.data_ptr() for t in self.par]
        args = (Xd.data_ptr() if B else 0, yd.data_ptr() if B else 0, B, self.F, p[0], p[1],
                self.M, self.k, self.dims, p[2:2 + L], p[2 + L:2 + 2 * L], p[2 + 2 * L],
                p[3 + 2 * L], lr, lam, self.opt, self._slots(), self.ws.data_ptr(),
                self.ws.numel())
        return self._call(self.nat.dfm_train_step_det, self.nat.dfm_train_step, args, scratch)


def _equal_states(a, b):
    return len(a) == len(b) and all(
        x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
        for x, y in zip(a, b))


# ---------------------------------------------------------------------------
# 1. known answers: before − after is the gradient (lr 1, λ 0, SGD)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["table", "head"])
def test_afm_known_answer_bit_for_bit(case):
    """table: B = 3,001, id 0 in every row — its 3,001 occurrences cross the
    64-occurrence fetch and the 32-ahead groups many times.  head: B = 1,031 —
    the strided partials take 4 or 5 rows and the last ones are short."""
    d = hr.afm_table_known() if case == "table" else hr.afm_head_known()
    s = _Afm(d["par"], SGD, len(d["X"]), 2)
    loss = s.step(d["X"], d["y"], 1.0, 0.0)
    for n, old, new, g in zip(AFM_NAMES, d["par"], s.params(), d["grads"]):
        assert _same_bits(np.asarray(old, F32) - new, g), n
    assert _same_bits(loss, d["loss"]), (loss, d["loss"])


@pytest.mark.parametrize("case", ["table", "head"])
def test_dfm_known_answer_bit_for_bit(case):
    d = hr.dfm_table_known() if case == "table" else hr.dfm_head_known()
    E, w, layers, biases, Wp, bp = d["par"]
    F, k, L = 2, 8, len(layers)
    s = _Dfm(d["par"], SGD, len(d["X"]), F)
    loss = s.step(d["X"], d["y"], 1.0, 0.0)
    new = s.params()
    assert _same_bits(E - new[0], d["dE"])
    assert _same_bits(w - new[1], d["dw"])
    for old, got in zip(layers + biases, new[2:2 + 2 * L]):       # every layer delta is 0
        assert _same_bits(old, got)
    dWp = Wp - new[2 + 2 * L]
    if case == "table":                                  # the deep part is g·h_L: not known
        assert not dWp[:F + k].any()
    else:
        assert _same_bits(dWp, d["dWp"]) and dWp[1] != 0
    assert _same_bits(bp - new[3 + 2 * L], d["dbp"])
    assert _same_bits(loss, d["loss"]), (loss, d["loss"])


# ---------------------------------------------------------------------------
# 2. repeatability
# ---------------------------------------------------------------------------
BATCHES = (301, 77, 400)
VOCAB = 10                                               # ids per field: every id repeats


def _batches(rng, F, labels):
    base = np.arange(F) * VOCAB
    return [((base + rng.integers(0, VOCAB, (B, F))).astype(np.int32),
             rng.choice(labels, B).astype(F32)) for B in BATCHES]


def _afm_params(rng, F, k, A):
    M = F * VOCAB
    gl = np.sqrt(2.0 / (A + k))
    return (rng.normal(0, 0.3, (M, k)).astype(F32), rng.normal(0, 0.1, M).astype(F32), F32(0.02),
            rng.normal(0, gl, (k, A)).astype(F32), rng.normal(0, gl, A).astype(F32),
            rng.normal(0, 1, A).astype(F32), rng.normal(1, 0.2, k).astype(F32))


def _dfm_params(rng, F, k, layers):
    M = F * VOCAB
    dims = [F * k] + list(layers)
    Ls = [rng.normal(0, np.sqrt(2.0 / (a + c)), (a, c)).astype(F32)
          for a, c in zip(dims, dims[1:])]
    bs = [rng.normal(0, 0.1, c).astype(F32) for c in layers]
    D = F + k + layers[-1]
    return (rng.normal(0, 0.1, (M, k)).astype(F32), rng.uniform(0, 1, M).astype(F32), Ls, bs,
            rng.normal(0, np.sqrt(2.0 / (D + 1)), D).astype(F32), F32(0.01))


@pytest.mark.parametrize("keep", [(1.0, 1.0), (0.7, 0.6)])
@pytest.mark.parametrize("opt", [ADAGRAD, MOMENTUM, ADAM])
@pytest.mark.parametrize("F,k,A", [(5, 16, 16), (3, 64, 8)])
def test_afm_steps_repeat_bit_for_bit(F, k, A, opt, keep):
    """λ_att = 100 (the value _afm_replay uses): Σvar² is in the loss."""
    rng = np.random.default_rng(41)
    par = _afm_params(rng, F, k, A)
    batches = _batches(rng, F, [1.0, -1.0])
    runs = []
    for _ in range(2):
        s = _Afm(par, opt, max(BATCHES), F)
        for i, (X, y) in enumerate(batches):
            s.step(X, y, 0.01, 100.0, keep, 2016 | i << 32)
        runs.append(s.state())
    assert _equal_states(*runs)
    assert not _same_bits(runs[0][0], par[0]) and not _same_bits(runs[0][3], par[3])


@pytest.mark.parametrize("opt", [SGD, ADAM])
@pytest.mark.parametrize("F,k,layers", [(5, 16, [32, 16]), (3, 8, [150, 200, 150])])
def test_dfm_steps_repeat_bit_for_bit(F, k, layers, opt):
    """SGD and Adam through the binding, λ = 0.01."""
    rng = np.random.default_rng(43)
    par = _dfm_params(rng, F, k, layers)
    batches = _batches(rng, F, [1.0, -1.0])
    runs = []
    for _ in range(2):
        s = _Dfm(par, opt, max(BATCHES), F)
        for X, y in batches:
            s.step(X, y, 0.01, 0.01)
        runs.append(s.state())
    assert _equal_states(*runs)
    assert not _same_bits(runs[0][0], par[0]) and not _same_bits(runs[0][2], par[2][0])


@pytest.mark.parametrize("F,k,layers", [(5, 16, [32, 16]), (3, 8, [150, 200, 150])])
def test_dfm_class_steps_repeat_bit_for_bit(F, k, layers):
    """Adagrad through DeepFM.partial_fit (the scratch grows at the third batch)."""
    from hhfm_amd.DFM import DeepFM
    rng = np.random.default_rng(44)
    batches = _batches(rng, F, [1.0, -1.0])
    runs = []
    for _ in range(2):
        m = DeepFM(VOCAB, VOCAB, F * VOCAB, F, k, layers, None, 0.01, 0, 0.01, deterministic=True)
        assert m.deterministic
        losses = [m.partial_fit({"X": X.astype(np.int64), "Y": y[:, None]}) for X, y in batches]
        W = m.get_weights()
        st = m._train_state
        runs.append([np.asarray(losses, np.float64).view(np.uint64)]
                    + [_bits(W[n]) for n in sorted(W)]
                    + [_bits(st[n].cpu().numpy()) for n in sorted(W)])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


# ---------------------------------------------------------------------------
# 3. the same arithmetic as the default steps
# ---------------------------------------------------------------------------
def _pair(model, par, X, y, F, opt=SGD, lr=1.0, lam=0.0, steps=1):
    out = []
    for d in (True, False):
        s = (_Afm if model == "afm" else _Dfm)(par, opt, len(X), F, deterministic=d)
        for _ in range(steps):
            if model == "afm":
                s.step(X, y, lr, lam, (0.7, 0.6), 99)
            else:
                s.step(X, y, lr, lam)
        out.append(s.state(whole_ws=False))
    return out


def _distinct_case(model, B):
    rng = np.random.default_rng(5 + B)
    F, k, M = 5, 16, 400
    X = rng.permutation(M)[:B * F].reshape(B, F).astype(np.int32)
    y = rng.choice([1.0, -1.0], B).astype(F32)
    if model == "afm":
        par = list(_afm_params(rng, F, k, 16))
    else:
        par = list(_dfm_params(rng, F, k, [32, 16]))
    par[0] = rng.normal(0, 0.2, (M, k)).astype(F32)
    par[1] = rng.normal(0, 0.3, M).astype(F32)
    return par, X, y, F


@pytest.mark.parametrize("model", ["afm", "dfm"])
def test_contributions_equal_the_default_path(model):
    """B = 16, M >= B·F, no id twice: one contribution per element of E and w,
    so only the contribution arithmetic is compared (AFM under dropout)."""
    par, X, y, F = _distinct_case(model, 16)
    a, b = _pair(model, par, X, y, F)
    assert _same_bits(a[0], b[0]) and not _same_bits(a[0], par[0])
    assert _same_bits(a[1], b[1]) and not _same_bits(a[1], par[1])


@pytest.mark.parametrize("model", ["afm", "dfm"])
def test_one_row_equals_the_default_path(model):
    """B = 1: one row's value added to zero — every variable, the workspace's
    persistent part and the loss are equal."""
    par, X, y, F = _distinct_case(model, 1)
    a, b = _pair(model, par, X, y, F)
    assert _equal_states(a, b)
    third = par[2] if model == "afm" else par[2][0]      # w0, or layer_0
    assert not _same_bits(a[0], par[0]) and not _same_bits(a[2], third)


@pytest.mark.parametrize("model", ["afm", "dfm"])
def test_empty_batch_equals_the_default_path(model):
    """B = 0 under Adam with λ > 0, two steps: parameters, slots, the
    persistent workspace (Adam's β powers advance) and the loss.  Every
    λ-carrying variable fits one wave (attention_W [8][8]; layer_0 [24][2] and
    the 13-element concat projection), so Σvar² has at most two non-zero
    partials, whose float sum and rounded double sum are the same number."""
    rng = np.random.default_rng(9)
    F = 3
    par = _afm_params(rng, F, 8, 8) if model == "afm" else _dfm_params(rng, F, 8, [2])
    X, y = np.zeros((0, F), np.int32), np.zeros(0, F32)
    a, b = _pair(model, par, X, y, F, ADAM, 0.1, 0.1, steps=2)
    assert _equal_states(a, b)
    lam_var, before = (3, par[3]) if model == "afm" else (2, par[2][0])
    assert not _same_bits(a[lam_var], before)            # λ decayed it
    assert a[-1][0] > 0 and a[-2].any()                 # the l2 loss; β powers in the workspace


# ---------------------------------------------------------------------------
# 4. parity, at the existing bars
# ---------------------------------------------------------------------------
def test_afm_det_matches_oracle_replay():
    """test_afm_partial_fit_matches_oracle's Frappe shape through _afm_replay."""
    k, A, ctx, B, opt = 64, 64, (7, 2, 3), 1000, "AdagradOptimizer"
    rng = np.random.default_rng(k + A + B)
    nu, ni = 60, 200
    X, M = tg._rows(rng, 2 * B, nu, ni, ctx)
    m = tg._afm_model(rng, k, A, M, X.shape[1], opt, nu, ni)
    m.deterministic = True
    for step in range(2):
        y = rng.choice([1.0, -1.0], B).astype(F32)[:, None]
        tg._afm_replay(m, X[step * B:(step + 1) * B], y, tg.OPTS[opt], step + 1)
    assert m._train_state.get("det") is not None


@pytest.mark.parametrize("opt", ["AdagradOptimizer", "AdamOptimizer"])
def test_dfm_det_matches_oracle_replay(opt):
    """(k, layers, B) = (16, [24, 40, 24], 301) of test_gpu_training.py through
    _dfm_replay: Adagrad through the class, Adam through the binding."""
    from hhfm_amd.DFM import DeepFM
    k, layers, B = 16, [24, 40, 24], 301
    rng = np.random.default_rng(k + B)
    nu, ni = 60, 200
    X, M = tg._rows(rng, 2 * B, nu, ni, (7, 2, 3))
    m = DeepFM(nu, ni, M, 5, k, layers, None, 0.01, 0, 0.01, deterministic=True)
    o = tg.OPTS[opt]
    if o == "adagrad":
        step_fn, slot_fn = tg._dfm_class_step(m)
    else:
        drv = _DetDfmBinding(m, o, 0.01, 0.01)
        step_fn, slot_fn = drv.step, drv.slot
    for step in range(2):
        y = rng.choice([1.0, -1.0], B).astype(F32)[:, None]
        tg._dfm_replay(m, step_fn, slot_fn, X[step * B:(step + 1) * B], y, o, 0.01, 0.01, step + 1)


class _DetDfmBinding(tg._DfmBinding):
    """_DfmBinding on hhfm_dfm_train_step_det."""

    def step(self, Xb, y):
        from hhfm_amd._native import native
        m, W, nat = self.m, self.m.weights, native()
        L = len(m.deep_layers)
        X = m._idx(Xb)
        yd = torch.as_tensor(np.asarray(y, F32).reshape(-1)).to(m.device)
        M, k = W["feature_embeddings"].shape
        ws = self.workspace(len(Xb))
        sc = torch.empty(nat.dfm_train_det_scratch(len(Xb), X.shape[1], k, M, m.deep_layers),
                         dtype=torch.uint8, device=m.device)
        ptr = lambda n: W[n].data_ptr()  # noqa: E731
        nat.dfm_train_step_det(
            X.data_ptr(), yd.data_ptr(), len(Xb), X.shape[1], ptr("feature_embeddings"),
            ptr("feature_bias"), M, k, m.deep_layers, [ptr(f"layer_{i}") for i in range(L)],
            [ptr(f"bias_{i}") for i in range(L)], ptr("concat_projection"), ptr("concat_bias"),
            self.lr, self.lam, self.opt,
            [self.slots[n].data_ptr() for n in self.names] if self.o != "sgd" else [],
            ws.data_ptr(), ws.numel(), sc.data_ptr(), sc.numel(), self.loss.data_ptr(), _stream())
        m._prep = None
        return float(self.loss.item())


@pytest.mark.parametrize("shape", [(3, 8, 8, 1), (5, 16, 16, 5), (5, 64, 64, 1030)])
def test_afm_det_dropout_gradient_matches_float64(shape):
    """keep (0.7, 0.6) against dropout_ref.afm_grad64_dropout at the AFM step
    bar of test_gpu_dropout.py; AFM.partial_fit, first step, random_seed 2016.
    Rows from afm_case: the relu margin holds."""
    from hhfm_amd.AFM import AFM
    keep = (0.7, 0.6)
    F, k, A, B = shape
    X, y, par = dref.afm_case(shape)
    b1, b2 = dref.afm_masks(dref.model_seed(2016, 0), shape, keep)
    ref_loss, grads = dref.afm_grad64_dropout(X, y, par, b1, b2, keep)
    E, w, w0, W, b, pvec, P = par
    m = AFM(1, 1, E.shape[0], 1, [A, k], None, 1.0, 0.0, list(keep), "GradientDescentOptimizer",
            0.999, F, random_seed=2016, deterministic=True)
    assert m.deterministic
    m.set_weights(feature_embeddings=E, feature_bias=w[:, None], bias=w0, attention_W=W,
                  attention_b=b[None, :], attention_p=pvec, prediction=P[:, None])
    loss = m.partial_fit({"X": X.astype(np.int64), "Y": y[:, None]})
    G_ = m.get_weights()
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    for n, old, g in zip(AFM_NAMES, par, grads):
        got = np.asarray(G_[n], F32).reshape(np.shape(old))
        ref = np.asarray(old, np.float64) - np.asarray(g, np.float64).reshape(np.shape(old))
        step = np.abs(ref - old).max()
        atol = 1e-4 * step + 1e-9
        err = np.abs(got - ref) - 1e-5 * np.abs(ref)
        print(f"afm det {shape} keep {keep} {n}: worst err / atol = {float(err.max() / atol):.3g}")
        assert np.allclose(got, ref, rtol=1e-5, atol=atol), n


# ---------------------------------------------------------------------------
# 5. arguments
# ---------------------------------------------------------------------------
def _small_run(model, opt=ADAGRAD, B=8):
    rng = np.random.default_rng(12)
    F = 5
    par = _afm_params(rng, F, 8, 8) if model == "afm" else _dfm_params(rng, F, 8, [12])
    X = (np.arange(F) * VOCAB + rng.integers(0, VOCAB, (B, F))).astype(np.int32)
    s = (_Afm if model == "afm" else _Dfm)(par, opt, B, F)
    return s, par, X, np.ones(B, F32)


@pytest.mark.parametrize("model", ["afm", "dfm"])
def test_short_or_null_scratch_is_refused(model):
    """One byte short: HHFM_EWORKSPACE; NULL: HHFM_EINVAL; every parameter,
    slot and the workspace bit for bit as they were; the exact size is taken."""
    s, par, X, y = _small_run(model)
    before = s.state()
    n = s.sc.numel()
    for sc, msg in (((s.sc.data_ptr(), n - 1), "workspace too small"),
                    ((0, n), "invalid argument"), ((0, 0), "invalid argument")):
        with pytest.raises(ValueError, match=msg):
            s.step(X, y, 0.1, 0.1, scratch=sc)
        assert _equal_states(s.state()[:-1], before[:-1])
    s.step(X, y, 0.1, 0.1, scratch=(s.sc.data_ptr(), n))
    assert not _same_bits(s.state()[0], par[0])


@pytest.mark.parametrize("model", ["afm", "dfm"])
def test_empty_batch_needs_the_scratch_too(model):
    s, par, X, y = _small_run(model, B=0)
    with pytest.raises(ValueError, match="invalid argument"):
        s.step(X, y, 0.1, 0.1, scratch=(0, 0))
    with pytest.raises(ValueError, match="workspace too small"):
        s.step(X, y, 0.1, 0.1, scratch=(s.sc.data_ptr(), s.sc.numel() - 1))
    s.step(X, y, 0.1, 0.1)


def test_afm_keep_zero_is_refused_and_changes_nothing():
    s, par, X, y = _small_run("afm")
    before = s.state()
    for keep in ((0.0, 1.0), (1.0, 0.0), (1.5, 1.0)):
        with pytest.raises(ValueError, match="invalid argument"):
            s.step(X, y, 0.1, 0.0, keep, 1)
        assert _equal_states(s.state()[:-1], before[:-1])


def test_det_scratch_sizes():
    from hhfm_amd._native import native
    nat = native()
    rows = (0, 1, 7, 77, 2049, 5000, 32773)
    afm = [nat.afm_train_det_scratch(B, 5, 64, 64, 5382) for B in rows]
    dfm = [nat.dfm_train_det_scratch(B, 5, 64, 5382, [150, 200, 150]) for B in rows]
    for sizes in (afm, dfm):
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    bad = "invalid argument"
    with pytest.raises(ValueError, match=bad):
        nat.afm_train_det_scratch(8, 1, 64, 64, 5382)             # F < 2
    with pytest.raises(ValueError, match=bad):
        nat.afm_train_det_scratch(8, 5, 62, 64, 5382)             # k % 4
    with pytest.raises(ValueError, match=bad):
        nat.dfm_train_det_scratch(8, 5, 62, 5382, [150])          # k % 4
    with pytest.raises(ValueError, match=bad):
        nat.dfm_train_det_scratch(8, 5, 64, 5382, [])             # nlayers 0
    with pytest.raises(ValueError, match=bad):
        nat.dfm_train_det_scratch(2 ** 31 // 5 + 1, 5, 64, 5382, [8])   # B·F > INT_MAX
    # the FM / HHFM query keeps the values it had before these steps existed
    fm = [nat.train_det_scratch(B, 5, 64, 5382) for B in (0, 1, 4099, 32773)]
    assert fm == [22016, 287232, 3204608, 23620352], fm
    assert nat.train_det_scratch(2049, 17, 8, 90) == 1691136


@pytest.mark.parametrize("model", ["afm", "dfm"])
def test_out_of_range_ids_read_row_zero(model):
    """An id outside [0, M) is row 0: the step equals the step on the same
    batch with those ids written as 0."""
    rng = np.random.default_rng(10)
    B, F = 65, 4
    par = _afm_params(rng, F, 20, 8) if model == "afm" else _dfm_params(rng, F, 20, [12])
    M = F * VOCAB
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    bad = X.copy()
    X[3, 1] = X[7, 0] = X[64, 3] = 0
    bad[3, 1], bad[7, 0], bad[64, 3] = -1, M, 2 ** 31 - 1
    y = rng.choice([1.0, -1.0], B).astype(F32)
    runs = []
    for rows in (X, bad):
        s = (_Afm if model == "afm" else _Dfm)(par, ADAGRAD, B, F)
        s.step(rows, y, 0.1, 0.01)
        runs.append(s.state())
    assert _equal_states(*runs)
    assert not _same_bits(runs[0][0], par[0])


# ---------------------------------------------------------------------------
# 6. the model surface
# ---------------------------------------------------------------------------
def _args(tmp_path, **kw):
    a = dict(path=G + "/", dataset="synth_frappe", epoch=4, batch_size=5000, hidden_factor=16,
             lamda=0.01, keep=1, lr=0.01, optimizer="AdagradOptimizer", verbose=0, batch_norm=0,
             TopK=10, Result=1, result_file=str(tmp_path / "result.txt"), deterministic=1)
    a.update(kw)
    return argparse.Namespace(**a)


@pytest.mark.parametrize("model", ["afm", "afm_keep", "dfm"])
def test_train_loop_is_reproducible(model, tmp_path):
    """Train with --deterministic 1, three epochs, twice with numpy seeded the
    same: loss_epoch is equal as a list and every weight bit for bit."""
    runs = []
    for _ in range(2):
        np.random.seed(2016)
        if model == "dfm":
            from hhfm_amd.DFM import Train
            t = Train(_args(tmp_path))
        else:
            from hhfm_amd.AFM import Train
            t = Train(_args(tmp_path, hidden_factor="[16,16]", lr=0.1, lamda_attention=100.0,
                            keep="[0.8,0.5]" if model == "afm_keep" else "[1,1]", attention=1,
                            decay=0.999, activation="relu"))
        assert t.model.deterministic
        losses = t.train()
        assert len(losses) == 3 and np.all(np.isfinite(losses))
        W = t.model.get_weights()
        runs.append((list(losses), [_bits(W[n]) for n in sorted(W)]))
    assert runs[0][0] == runs[1][0]
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))


def test_parse_args_and_constructors_take_the_flag():
    from hhfm_amd import AFM, DFM
    assert AFM.parse_args("frappe", 64, 10, []).deterministic == 0
    assert AFM.parse_args("frappe", 64, 10, ["--deterministic", "1"]).deterministic == 1
    assert DFM.parse_args("frappe", 64, 10, []).deterministic == 0
    assert DFM.parse_args("frappe", 64, 10, ["--deterministic", "1"]).deterministic == 1
    a = AFM.AFM(1, 1, 10, 1, [8, 8], None, 0.1, 0.0, [1, 1], "AdagradOptimizer", 0.999, 3)
    d = DFM.DeepFM(1, 1, 10, 3, 8, [4])
    assert a.deterministic is False and d.deterministic is False
    a = AFM.AFM(1, 1, 10, 1, [8, 8], None, 0.1, 0.0, [1, 1], "AdagradOptimizer", 0.999, 3,
                deterministic=True)
    d = DFM.DeepFM(1, 1, 10, 3, 8, [4], deterministic=True)
    assert a.deterministic is True and d.deterministic is True
