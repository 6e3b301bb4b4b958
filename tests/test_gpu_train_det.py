"""The deterministic FM / HHFM training steps (include/hhfm.h "Deterministic
training steps"; ``deterministic=True`` of FM / OUR) on the GPU.

1. Known answers: inputs whose contributions are exact in fp32
   (tests/train_det_ref.py) — the update equals the documented ordered sums
   bit for bit.
2. Repeatability: two runs from identical state, three steps of changing
   batch size — every parameter, slot and loss bit for bit.
3. Float64 parity: the bound of tests/test_gpu_train_grad.py, unchanged, on
   its cases and on FM's k = 260 dropout cases.
4. The same contributions as the default steps: with no id twice in the
   batch every element has one contribution, so E and w are equal bit for bit.
5. Edges: B = 0, out-of-range ids, a short or NULL scratch, the scratch size.
6. The model surface: ``--deterministic 1`` trains to the same bits twice.

Measured on an MI355X, largest err / bound of (3): see DESIGN.md §H6.
"""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import dropout_ref as dref
from tests import train_det_ref as det
from tests import train_ref as tr

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
ADAGRAD, SGD, MOMENTUM, ADAM = 0, 1, 2, 3
F32 = np.float32


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


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class _Step:
    """Device state of a run through the binding: parameters, slots, the
    zero-filled workspace, and (deterministic) a scratch filled with 0xA5 —
    it need not be zeroed."""

    def __init__(self, params, opt, det_rows, occ, deterministic=True):
        from hhfm_amd._native import native
        self.nat = native()
        self.par = [_dev(np.asarray(p, F32).reshape(-1) if np.ndim(p) == 0 else p)
                    for p in params]
        self.opt = opt
        self.acc = [_slot(opt, p) for p in self.par]
        self.M, self.k = self.par[0].shape
        self.ws = torch.zeros(self.nat.train_workspace(self.M, self.k), dtype=torch.uint8,
                              device="cuda")
        self.det = deterministic
        self.sc = None
        if deterministic:
            n = self.nat.train_det_scratch(det_rows, occ, self.k, self.M)
            self.sc = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        self.loss = torch.zeros(1, device="cuda")
        self.losses = []

    def _finish(self):
        self.losses.append(F32(self.loss.item()))
        return self.losses[-1]

    def fm(self, X, y, lr, lam, keep=1.0, seed=0, scratch=None):
        E, w, w0 = self.par
        B, F = X.shape
        Xd, yd = _dev(X.astype(np.int32)), _dev(y.astype(F32))
        args = (_ptr(Xd) if B else 0, _ptr(yd) if B else 0, B, F, E.data_ptr(), w.data_ptr(),
                w0.data_ptr(), self.M, self.k, lr, lam, self.opt, keep, seed,
                _ptr(self.acc[0]), _ptr(self.acc[1]), _ptr(self.acc[2]), self.ws.data_ptr(),
                self.ws.numel())
        if self.det:
            sc = scratch if scratch is not None else (self.sc.data_ptr(), self.sc.numel())
            self.nat.fm_train_step_det(*args, *sc, self.loss.data_ptr(), _stream())
        else:
            self.nat.fm_train_step_ex(*args, self.loss.data_ptr(), _stream())
        return self._finish()

    def hhfm(self, X, Neg, ctx, tim, lr, lam, scratch=None):
        E, = self.par
        B, ncols = X.shape
        Xd, Nd = _dev(X.astype(np.int32)), _dev(Neg.astype(np.int32))
        args = (_ptr(Xd) if B else 0, _ptr(Nd) if B else 0, B, ncols, ctx[0], ctx[1], tim[0],
                tim[1], Neg.shape[1], E.data_ptr(), self.M, self.k, lr, lam, self.opt,
                _ptr(self.acc[0]), self.ws.data_ptr(), self.ws.numel())
        if self.det:
            sc = scratch if scratch is not None else (self.sc.data_ptr(), self.sc.numel())
            self.nat.hhfm_train_step_det(*args, *sc, self.loss.data_ptr(), _stream())
        else:
            self.nat.hhfm_train_step(*args, self.loss.data_ptr(), _stream())
        return self._finish()

    def state(self):
        """Every parameter, every slot, the workspace (zero but Adam's β
        powers) and the returned losses."""
        torch.cuda.synchronize()
        out = [p.cpu().numpy() for p in self.par]
        out += [a.cpu().numpy() for a in self.acc if a is not None]
        out += [self.ws.cpu().numpy().view(np.uint32), np.asarray(self.losses, F32)]
        return out


def _equal_states(a, b):
    return len(a) == len(b) and all(
        np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _occ(NG, ctx, tim):
    return 2 + NG + (ctx[1] - ctx[0]) + (tim[1] - tim[0])


# ---------------------------------------------------------------------------
# 1. known answers
# ---------------------------------------------------------------------------
def test_fm_known_answer_bit_for_bit():
    """One SGD step (lr 1, λ 0) from E[0] = 0, w = 0, w0 = 0: before − after is
    the gradient itself — dE[0], dw[0] the ordered sums over 3,001 rows, dw0
    the scalar-order sum — and the loss the float of Σ y²/2 within 1 ulp."""
    d = det.fm_known()
    B, M, k = len(d["X"]), d["M"], d["k"]
    w, w0 = np.zeros(M, F32), F32(0)
    s = _Step([d["E"], w, w0], SGD, B, 2)
    loss = s.fm(d["X"], d["y"], 1.0, 0.0)
    E1, w1, w01 = s.state()[:3]
    assert _same_bits(d["E"] - E1, d["dE"])
    assert _same_bits(w - w1, d["dw"])
    assert _same_bits(w0 - w01, d["dw0"])
    assert abs(np.float64(loss) - d["loss64"]) <= np.spacing(F32(d["loss64"])), (loss, d["loss"])


def test_hhfm_known_answer_bit_for_bit():
    """Layout "none", NG = 1, a hot item, pos = neg = 0: expf(−0) = 1 gives
    σ = ½ exactly (the result shows it: any other σ changes every bit), every
    contribution is exact, and the update is E − dE of the restatement."""
    d = det.hhfm_known()
    B = len(d["X"])
    s = _Step([d["E"]], SGD, B, 3)
    loss = s.hhfm(d["X"], d["Neg"], (0, 0), (0, 0), 1.0, 0.0)
    E1 = s.state()[0]
    want = (d["E"] - d["dE"]).astype(F32)               # var − lr·g, one rounding
    assert _same_bits(d["E"] - E1, d["E"] - want)
    assert abs(np.float64(loss) - d["loss64"]) <= np.spacing(F32(d["loss64"]))


# ---------------------------------------------------------------------------
# 2. repeatability
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [1.0, 0.7])
@pytest.mark.parametrize("opt", [ADAGRAD, MOMENTUM, ADAM])
def test_fm_steps_repeat_bit_for_bit(opt, keep):
    """B = 4,099 → 77 → 4,099, F = 5, k = 64, M = 300, a hot user, λ = 0.01."""
    rng = np.random.default_rng(41)
    M, F, k = 300, 5, 64
    E = rng.normal(0, 0.1, (M, k)).astype(F32)
    w = rng.normal(0, 0.1, M).astype(F32)
    batches = []
    for B in (4099, 77, 4099):
        X = rng.integers(0, M, (B, F)).astype(np.int32)
        X[:, 0] = 0
        batches.append((X, rng.integers(0, 2, B).astype(F32)))
    runs = []
    for _ in range(2):
        s = _Step([E, w, F32(0.02)], opt, 4099, F)
        for i, (X, y) in enumerate(batches):
            s.fm(X, y, 0.1, 0.01, keep, 2016 | i << 32)
        runs.append(s.state())
    assert _equal_states(*runs)
    assert not _same_bits(runs[0][0], E)


@pytest.mark.parametrize("opt", [ADAGRAD, ADAM])
@pytest.mark.parametrize("layout,NG,k", [("both", 10, 64), ("none", 16, 8)])
def test_hhfm_steps_repeat_bit_for_bit(layout, NG, k, opt):
    """B = 2,049 → 77 → 2,049, λ = 0.01; few items, so every negative list
    holds repeats and ties."""
    rng = np.random.default_rng(43)
    fd, td = tr.LAYOUTS[layout]
    nu, ni, nc = 30, 40, 4
    M = nu + ni + fd * nc
    ctx = (2, 2 + fd) if fd else (0, 0)
    tim = (2 + fd, 2 + fd + td) if td else (0, 0)
    E = rng.normal(0, 0.1, (M, k)).astype(F32)
    batches = []
    for B in (2049, 77, 2049):
        cols = [rng.integers(0, nu, B), rng.integers(nu, nu + ni, B)]
        cols += [rng.integers(nu + ni + f * nc, nu + ni + (f + 1) * nc, B) for f in range(fd)]
        cols += [rng.integers(nu, nu + ni, B) for _ in range(td)]
        X = np.stack(cols, 1).astype(np.int32)
        X[:, 1] = nu                                    # a hot item
        batches.append((X, rng.integers(nu, nu + ni, (B, NG)).astype(np.int32)))
    runs = []
    for _ in range(2):
        s = _Step([E], opt, 2049, _occ(NG, ctx, tim))
        for X, Neg in batches:
            s.hhfm(X, Neg, ctx, tim, 0.1, 0.01)
        runs.append(s.state())
    assert _equal_states(*runs)
    assert not _same_bits(runs[0][0], E)


# ---------------------------------------------------------------------------
# 3. float64 parity (the bound of test_gpu_train_grad.py, unchanged)
# ---------------------------------------------------------------------------
def _check(what, before, after, grad, mag):
    before, after = np.asarray(before, F32), np.asarray(after, F32)
    delta = before.astype(np.float64) - after.astype(np.float64)
    r = tr.ratio(delta, before, after, grad, mag)
    print(f"train_det_grad {what}: err / bound = {r:.3g}")
    assert r <= 1.0, (what, r)


def _fm_model_step(X, y, E, w, w0, keep=1, seed=2016):
    from hhfm_amd.FM import FM
    (B, F), (M, k) = X.shape, E.shape
    m = FM(F, M, 1, M - 1, k, 1.0, 0.0, keep, "GradientDescentOptimizer", 0, 0,
           random_seed=seed, deterministic=True)
    assert m.deterministic
    m.set_weights(feature_embeddings=E, feature_bias=w[:, None], bias=w0)
    loss = m.partial_fit({"X": X.astype(np.int64), "Y": y[:, None]})
    W = m.get_weights()
    return loss, W["feature_embeddings"], W["feature_bias"][:, 0], F32(W["bias"])


@pytest.mark.parametrize("name", sorted(tr.FM_CASES))
def test_fm_det_gradient_matches_float64(name):
    X, y, E, w, w0 = tr.fm_case(name)
    ref_loss, (dE, dw, dw0), (mE, mw, mw0) = tr.fm_grad64(X, y, E, w, w0)
    if name != "F65":
        loss, E1, w1, w01 = _fm_model_step(X, y, E, w, w0)
    else:                                               # wider than the class's layout
        s = _Step([E, w, w0], SGD, len(X), X.shape[1])
        loss = s.fm(X, y, 1.0, 0.0)
        E1, w1, w01 = s.state()[:3]
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    _check(f"fm {name} E", E, E1, dE, mE)
    _check(f"fm {name} w", w, w1, dw, mw)
    _check(f"fm {name} w0", w0, w01, dw0, mw0)


@pytest.mark.parametrize("keep", dref.FM_KEEPS)
def test_fm_det_dropout_gradient_matches_float64(keep):
    """k = 260: a lane's fifth column opens a second Philox block; the
    segment pass regenerates the row kernel's mask from (seed, b, c)."""
    name = "k260"
    X, y, E, w, w0 = dref.fm_case(name)
    bn = dref.binary(2016, dref.SITE_FM, len(X), E.shape[1], keep)
    ref_loss, (dE, dw, dw0), (mE, mw, mw0) = dref.fm_grad64_dropout(X, y, E, w, w0, bn, keep)
    loss, E1, w1, w01 = _fm_model_step(X, y, E, w, w0, keep)
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    _check(f"fm-dropout {name} keep {keep} E", E, E1, dE, mE)
    _check(f"fm-dropout {name} keep {keep} w", w, w1, dw, mw)
    _check(f"fm-dropout {name} keep {keep} w0", w0, w01, dw0, mw0)


@pytest.mark.parametrize("name", sorted(tr.HHFM_CASES))
def test_hhfm_det_gradient_matches_float64(name):
    layout = tr.HHFM_CASES[name][0]
    X, Neg, E, ctx, tim, ties = tr.hhfm_case(name)
    ref_loss, dE, mE, info = tr.hhfm_grad64(X, Neg, E, ctx, tim, ties)
    fd, td = tr.LAYOUTS[layout]
    if fd:
        from hhfm_amd.OurModel7 import OUR
        M, k = E.shape
        m = OUR(fd, td, M, tr.NU, tr.NI, k, 1.0, 0.0, "GradientDescentOptimizer", True, td > 0,
                deterministic=True)
        assert m.deterministic
        m.set_weights(feature_embeddings=E)
        data = {"X": X[:, :2].astype(np.int64), "Y": Neg.astype(np.int64),
                "F1": X[:, 2:2 + fd].astype(np.int64)}
        if td:
            data["F2"] = X[:, 2 + fd:].astype(np.int64)
        loss = m.partial_fit(data)
        E1 = m.get_weights()["feature_embeddings"]
    else:                                               # layouts the class does not take
        s = _Step([E], SGD, len(X), _occ(Neg.shape[1], ctx, tim))
        loss = s.hhfm(X, Neg, ctx, tim, 1.0, 0.0)
        E1 = s.state()[0]
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    _check(f"hhfm {name} E", E, E1, dE, mE)


# ---------------------------------------------------------------------------
# 4. the same contributions as the default steps
# ---------------------------------------------------------------------------
def _fm_pair(X, y, E, w, w0, keep=1.0):
    out = []
    for d in (True, False):
        s = _Step([E, w, w0], SGD, len(X), X.shape[1], deterministic=d)
        s.fm(X, y, 1.0, 0.0, keep, 99)
        out.append(s.state())
    return out


@pytest.mark.parametrize("keep", [1.0, 0.7])
def test_fm_contributions_equal_the_default_path(keep):
    """B = 64, F = 5, M = 400, k = 68, no id twice: one contribution per
    element, so only the contribution arithmetic is compared."""
    rng = np.random.default_rng(5)
    B, F, M, k = 64, 5, 400, 68
    X = rng.permutation(M)[:B * F].reshape(B, F).astype(np.int32)
    E = rng.normal(0, 0.2, (M, k)).astype(F32)
    w = rng.normal(0, 0.3, M).astype(F32)
    y = rng.integers(0, 2, B).astype(F32)
    a, b = _fm_pair(X, y, E, w, F32(0.02), keep)
    assert _same_bits(a[0], b[0]) and not _same_bits(a[0], E)
    assert _same_bits(a[1], b[1]) and not _same_bits(a[1], w)


@pytest.mark.parametrize("keep", [1.0, 0.7])
def test_fm_scalars_equal_the_default_path_at_one_row(keep):
    rng = np.random.default_rng(6)
    F, M, k = 5, 400, 68
    X = rng.permutation(M)[:F].reshape(1, F).astype(np.int32)
    E = rng.normal(0, 0.2, (M, k)).astype(F32)
    w = rng.normal(0, 0.3, M).astype(F32)
    a, b = _fm_pair(X, np.ones(1, F32), E, w, F32(0.02), keep)
    assert _equal_states(a, b)                          # E, w, w0, workspace, loss
    assert a[2] != F32(0.02)


def _hhfm_distinct(rng, B, NG, M):
    fd, td = tr.LAYOUTS["both"]
    ncols = 2 + fd + td
    ids = rng.permutation(M)[:B * (ncols + NG)].reshape(B, ncols + NG).astype(np.int32)
    return ids[:, :ncols], ids[:, ncols:], (2, 2 + fd), (2 + fd, ncols)


@pytest.mark.parametrize("B", [16, 1])
def test_hhfm_contributions_equal_the_default_path(B):
    """"both" layout, NG = 2, users, items, negatives, context and time ids
    all distinct; at B = 1 the loss is compared bit for bit as well."""
    rng = np.random.default_rng(8)
    NG, M, k = 2, 200, 68
    X, Neg, ctx, tim = _hhfm_distinct(rng, B, NG, M)
    E = rng.normal(0, 0.2, (M, k)).astype(F32)
    out = []
    for d in (True, False):
        s = _Step([E], SGD, B, _occ(NG, ctx, tim), deterministic=d)
        s.hhfm(X, Neg, ctx, tim, 1.0, 0.0)
        out.append(s.state())
    a, b = out
    assert _same_bits(a[0], b[0]) and not _same_bits(a[0], E)
    if B == 1:
        assert _equal_states(a, b)


# ---------------------------------------------------------------------------
# 5. edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["fm", "hhfm"])
def test_empty_batch_equals_the_default_path(model):
    """B = 0 under Adam with λ > 0, two steps: parameters, slots and the
    workspace (Adam's β powers advance) equal the default step's bit for bit.
    The table is one wave's worth (56 elements), so Σvar² has one partial and
    the loss is equal too."""
    rng = np.random.default_rng(9)
    M, k, F = 7, 8, 3
    E = rng.normal(0, 0.1, (M, k)).astype(F32)
    par = [E, rng.normal(0, 0.1, M).astype(F32), F32(0.02)] if model == "fm" else [E]
    out = []
    for d in (True, False):
        s = _Step(par, ADAM, 0, F if model == "fm" else 5, deterministic=d)
        for _ in range(2):
            if model == "fm":
                s.fm(np.zeros((0, F), np.int32), np.zeros(0, F32), 0.1, 0.1)
            else:
                s.hhfm(np.zeros((0, F), np.int32), np.zeros((0, 2), np.int32), (2, 3), (0, 0),
                       0.1, 0.1)
        out.append(s.state())
    a, b = out
    assert _equal_states(a, b)
    assert not _same_bits(a[0], E) and a[-1][0] > 0     # λ decayed the table; the l2 loss
    assert a[-2].any()                                  # β powers live in the workspace


def test_out_of_range_ids_read_row_zero():
    """As on the default path: an id outside [0, M) is row 0 — the step equals
    the step on the same batch with those ids written as 0."""
    rng = np.random.default_rng(10)
    B, F, M, k = 65, 4, 30, 20
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    bad = X.copy()
    X[3, 1] = X[7, 0] = X[64, 3] = 0
    bad[3, 1], bad[7, 0], bad[64, 3] = -1, M, 2 ** 31 - 1
    E = rng.normal(0, 0.2, (M, k)).astype(F32)
    w = rng.normal(0, 0.3, M).astype(F32)
    y = rng.integers(0, 2, B).astype(F32)
    runs = []
    for rows in (X, bad):
        s = _Step([E, w, F32(0.02)], ADAGRAD, B, F)
        s.fm(rows, y, 0.1, 0.01)
        runs.append(s.state())
    assert _equal_states(*runs)
    runs = []                                           # HHFM: [user, item, ctx | negative]
    for rows in (X, bad):
        s = _Step([E], ADAGRAD, B, _occ(1, (2, 3), (0, 0)))
        s.hhfm(rows[:, :3], rows[:, 3:], (2, 3), (0, 0), 0.1, 0.01)
        runs.append(s.state())
    assert _equal_states(*runs)


@pytest.mark.parametrize("model", ["fm", "hhfm"])
def test_short_or_null_scratch_is_refused(model):
    """One byte short, or NULL: the binding's error, every parameter and slot
    bit for bit as it was; the exact size is taken."""
    rng = np.random.default_rng(12)
    B, F, M, k = 8, 5, 40, 8
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    E = rng.normal(0, 0.1, (M, k)).astype(F32)
    if model == "fm":
        s = _Step([E, rng.normal(0, 0.1, M).astype(F32), F32(0.02)], ADAGRAD, B, F)
        call = lambda sc: s.fm(X, np.ones(B, F32), 0.1, 0.1, scratch=sc)  # noqa: E731
    else:
        s = _Step([E], ADAGRAD, B, _occ(2, (2, 3), (0, 0)))
        call = lambda sc: s.hhfm(X[:, :3], X[:, 3:], (2, 3), (0, 0), 0.1, 0.1,  # noqa: E731
                                 scratch=sc)
    before = s.state()
    for sc in ((s.sc.data_ptr(), s.sc.numel() - 1), (0, s.sc.numel()), (0, 0)):
        with pytest.raises(ValueError, match="invalid argument"):
            call(sc)
        assert _equal_states(s.state()[:-1], before[:-1])
    call((s.sc.data_ptr(), s.sc.numel()))
    assert not _same_bits(s.state()[0], E)


def test_det_scratch_size():
    from hhfm_amd._native import native
    nat = native()
    sizes = [nat.train_det_scratch(B, 5, 64, 5382) for B in (0, 1, 7, 77, 2049, 4099, 32773)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    with pytest.raises(ValueError, match="invalid argument"):
        nat.train_det_scratch(2 ** 31 // 5 + 1, 5, 64, 5382)    # B·occ_per_row > INT_MAX
    with pytest.raises(ValueError, match="invalid argument"):
        nat.train_det_scratch(8, 0, 64, 5382)


# ---------------------------------------------------------------------------
# 6. the model surface
# ---------------------------------------------------------------------------
def _args(tmp_path, **kw):
    a = dict(path=G + "/", dataset="synth_frappe", epoch=3, batch_size=5000, hidden_factor=32,
             lamda=0.1, keep=1, lr=0.1, optimizer="AdagradOptimizer", verbose=0, batch_norm=0,
             TopK=10, Result=1, result_file=str(tmp_path / "result.txt"), deterministic=1)
    a.update(kw)
    return argparse.Namespace(**a)


@pytest.mark.parametrize("model", ["fm", "fm_keep", "hhfm"])
def test_train_loop_is_reproducible(model, tmp_path):
    """Train with --deterministic 1, two epochs, twice with numpy seeded the
    same: loss_epoch and the final weights are identical bit for bit."""
    runs = []
    for _ in range(2):
        np.random.seed(2016)
        if model == "hhfm":
            from hhfm_amd.OurModel7 import Train
            t = Train(_args(tmp_path, lamda=0.01))
        else:
            from hhfm_amd.FM import Train
            t = Train(_args(tmp_path, keep=0.7 if model == "fm_keep" else 1))
        assert t.model.deterministic
        losses = t.train()
        assert len(losses) == 2 and losses[1] < losses[0]
        W = t.model.get_weights()
        runs.append([np.asarray(losses, np.float64).view(np.uint64)]
                    + [_bits(W[n]) for n in sorted(W)])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


def test_parse_args_take_the_flag():
    from hhfm_amd import FM, OurModel7
    assert FM.parse_args("frappe", 64, 10, []).deterministic == 0
    assert FM.parse_args("frappe", 64, 10, ["--deterministic", "1"]).deterministic == 1
    assert OurModel7.parse_args("frappe", 64, 10, ["--deterministic", "1"]).deterministic == 1
    assert OurModel7.parse_args("frappe", 64, 10, []).deterministic == 0
