"""H6 on the GPU, gradient by gradient: `fm_train_rows` / `hhfm_train_rows`
against the float64 references of tests/train_ref.py.

One step with GradientDescentOptimizer, lr = 1, λ = 0 leaves
``before − after`` equal to the raw gradient the row kernel scattered, so
every table / w / w0 element is held to

    |Δ − grad64| <= 1e-5 · mag + 2^-23 · max(|before|, |after|)

(mag: tests/train_ref.py — the 1e-5 score bar propagated to first order; the
second term is the rounding of the subtraction) and the loss to 1e-5
relative.  A contribution dropped from, or doubled into, one table row fails
this; the step-level checks of test_gpu_training.py (1e-4 of the largest
update) would not notice.

Inputs are kept where the fp32 oracle alone (float32, np.add.at) sits well
inside the bound — tests/test_train_ref.py asserts err / bound <= 0.25 for
every case on the CPU; measured there: FM 0.0016 – 0.014 (B32773 the
largest), HHFM 0.0021 – 0.15 (none_ng10_k128 the largest).  HHFM inputs keep
|pos − max neg| <= 4 (σ − 1 then loses <= ~3e-6 to cancellation) and every
untied negative more than 1e-5 · S below the maximum.

Measured on an MI355X, largest err / bound per model: FM 0.067 (w0 of
B32773: 32,773 atomics into one float; E 0.0073, w 0.0029 at most), HHFM
0.15 (none_ng10_k128, the same as the fp32 oracle's there; 0.034 next).  No
case passes 0.5.  With the `− e_f` term of `fm_train_rows` dropped every FM
case fails, with tied negatives given the unsplit gradient every HHFM case
that holds a tie does, and on the kernel as it was before this file F65
fails on `w`.

The second half checks the four train entry points' argument checks: the
binding's error and every parameter bit for bit as it was.
"""
import numpy as np
import pytest
import torch

from tests import train_ref as tr
from tests.helpers import log_parity

pytestmark = pytest.mark.gpu

def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _check(what, before, after, grad, mag):
    """The per-element bound; logs the case's largest err / bound.  The other
    fields are the ones the parity report (tests/conftest.py) prints for every
    record that is no top-K tie count, read elementwise: κ = mag / |grad64|,
    and the largest relative error among the elements with κ <= 100."""
    before, after = np.asarray(before, np.float32), np.asarray(after, np.float32)
    delta = before.astype(np.float64) - after.astype(np.float64)
    r = tr.ratio(delta, before, after, grad, mag)
    g = np.abs(np.asarray(grad, np.float64)).reshape(-1)
    err = np.abs(delta.reshape(-1) - np.asarray(grad, np.float64).reshape(-1))
    kappa = np.asarray(mag, np.float64).reshape(-1) / np.maximum(g, 1e-300)
    well = (g > 0) & (kappa <= 100)
    rel = err / np.maximum(g, 1e-300)
    log_parity("train_grad", rows=int(g.size), rows_kappa_gt_100=int(((g > 0) & ~well).sum()),
               max_rel_err_kappa_le_100=float(rel[well].max()) if well.any() else 0.0,
               max_rel_err_kappa_gt_100=0.0, oracle_max_rel_err_kappa_gt_100=0.0,
               max_err_over_bound=r)
    print(f"train_grad {what}: err / bound = {r:.3g}")
    assert r <= 1.0, (what, r)
    return r


def _fm_step(name, X, y, E, w, w0):
    """-> loss, E, w, w0 after one SGD step (lr 1, λ 0): FM.partial_fit, and
    the binding itself at F = 65 (wider than a wave: no model class needed)."""
    B, F = X.shape
    M, k = E.shape
    if name != "F65":
        from hhfm_amd.FM import FM
        m = FM(F, M, 1, M - 1, k, 1.0, 0.0, 1, "GradientDescentOptimizer", 0, 0)
        m.set_weights(feature_embeddings=E, feature_bias=w[:, None], bias=w0)
        loss = m.partial_fit({"X": X.astype(np.int64), "Y": y[:, None]})
        W = m.get_weights()
        return loss, W["feature_embeddings"], W["feature_bias"][:, 0], np.float32(W["bias"])
    from hhfm_amd._native import native
    Xd, yd, Ed, wd, w0d = _dev(X), _dev(y), _dev(E), _dev(w), _dev(np.float32([w0]))
    ws = torch.zeros(native().train_workspace(M, k), dtype=torch.uint8, device="cuda")
    loss = torch.zeros(1, device="cuda")
    native().fm_train_step(Xd.data_ptr(), yd.data_ptr(), B, F, Ed.data_ptr(), wd.data_ptr(),
                           w0d.data_ptr(), M, k, 1.0, 0.0, 1, 0, 0, 0, ws.data_ptr(), ws.numel(),
                           loss.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return float(loss.item()), Ed.cpu().numpy(), wd.cpu().numpy(), np.float32(w0d.item())


@pytest.mark.parametrize("name", sorted(tr.FM_CASES))
def test_fm_gradient_matches_float64(name):
    """k = 4 … 200 (one, two and partial strides of 64 lanes), F = 1 … 65
    (w's gradient of columns 64 and up), a hot user, repeated ids inside a
    row, and B > 32,768 (a wave takes a second row)."""
    X, y, E, w, w0 = tr.fm_case(name)
    ref_loss, (dE, dw, dw0), (mE, mw, mw0) = tr.fm_grad64(X, y, E, w, w0)
    loss, E1, w1, w01 = _fm_step(name, X, y, E, w, w0)
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    _check(f"fm {name} E", E, E1, dE, mE)
    _check(f"fm {name} w", w, w1, dw, mw)
    _check(f"fm {name} w0", w0, w01, dw0, mw0)


def _hhfm_step(layout, X, Neg, E, ctx, tim):
    """-> loss, E after one SGD step (lr 1, λ 0): OUR.partial_fit where the
    class takes the layout (context, context + time), else the binding."""
    fd, td = tr.LAYOUTS[layout]
    B, ncols = X.shape
    M, k = E.shape
    if fd:
        from hhfm_amd.OurModel7 import OUR
        m = OUR(fd, td, M, tr.NU, tr.NI, k, 1.0, 0.0, "GradientDescentOptimizer", True, td > 0)
        m.set_weights(feature_embeddings=E)
        data = {"X": X[:, :2].astype(np.int64), "Y": Neg.astype(np.int64),
                "F1": X[:, 2:2 + fd].astype(np.int64)}
        if td:
            data["F2"] = X[:, 2 + fd:].astype(np.int64)
        loss = m.partial_fit(data)
        return loss, m.get_weights()["feature_embeddings"]
    from hhfm_amd._native import native
    Xd, Nd, Ed = _dev(X), _dev(Neg), _dev(E)
    ws = torch.zeros(native().train_workspace(M, k), dtype=torch.uint8, device="cuda")
    loss = torch.zeros(1, device="cuda")
    native().hhfm_train_step(Xd.data_ptr(), Nd.data_ptr(), B, ncols, ctx[0], ctx[1], tim[0],
                             tim[1], Neg.shape[1], Ed.data_ptr(), M, k, 1.0, 0.0, 1, 0,
                             ws.data_ptr(), ws.numel(), loss.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    return float(loss.item()), Ed.cpu().numpy()


@pytest.mark.parametrize("name", sorted(tr.HHFM_CASES))
def test_hhfm_gradient_matches_float64(name):
    """Context only, time only, both, neither; NG = 1, 2, 10, 16; k = 8 … 128;
    B = 1 and 257 with the planted rows of train_ref.hhfm_case (a repeated
    maximum, NG equal negatives, negative = positive item, two ids with
    bit-identical rows, a context id equal to the user id)."""
    layout = tr.HHFM_CASES[name][0]
    X, Neg, E, ctx, tim, ties = tr.hhfm_case(name)
    ref_loss, dE, mE, info = tr.hhfm_grad64(X, Neg, E, ctx, tim, ties)
    assert np.abs(info["z"]).max() <= 4 and info["margin"] > 1e-5
    loss, E1 = _hhfm_step(layout, X, Neg, E, ctx, tim)
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    _check(f"hhfm {name} E", E, E1, dE, mE)


# ---------------------------------------------------------------------------
# argument checks of the four train entry points: the binding's error, and
# every parameter bit for bit as it was
# ---------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Args:
    """Device buffers for one refused call: int32 rows, labels, every
    parameter seeded non-zero, Adagrad slots at 0.1, loss and a workspace."""

    def __init__(self, B, F, M, k, extra=()):
        rng = np.random.default_rng(B + F + k)
        self.X = _dev(rng.integers(0, M, (B, F)).astype(np.int32))
        self.y = _dev(rng.integers(0, 2, B).astype(np.float32))
        shapes = [(M, k), (M,), (1,)] + [tuple(s) for s in extra]
        self.par = [_dev(rng.normal(0, 0.1, s).astype(np.float32)) for s in shapes]
        self.acc = [torch.full((2 * p.numel(),), 0.1, device="cuda") for p in self.par]
        self.before = [p.clone() for p in self.par]
        self.loss = torch.zeros(1, device="cuda")

    def ws(self, nbytes):
        self.w = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        return self.w

    def unchanged(self):
        torch.cuda.synchronize()
        return all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                   for a, b in zip(self.par, self.before))


def _fm_call(a, B, F, M, k, ws_bytes):
    from hhfm_amd._native import native
    E, w, w0 = a.par[:3]
    native().fm_train_step(a.X.data_ptr(), a.y.data_ptr(), B, F, E.data_ptr(), w.data_ptr(),
                           w0.data_ptr(), M, k, 0.1, 0.1, 0, a.acc[0].data_ptr(),
                           a.acc[1].data_ptr(), a.acc[2].data_ptr(), a.w.data_ptr(), ws_bytes,
                           a.loss.data_ptr(), _stream())


def _hhfm_call(a, Neg, B, F, M, k, ws_bytes):
    from hhfm_amd._native import native
    native().hhfm_train_step(a.X.data_ptr(), Neg.data_ptr(), B, F, 2, F, 0, 0, Neg.shape[1],
                             a.par[0].data_ptr(), M, k, 0.1, 0.1, 0, a.acc[0].data_ptr(),
                             a.w.data_ptr(), ws_bytes, a.loss.data_ptr(), _stream())


def _afm_call(a, B, F, M, k, A, ws_bytes):
    from hhfm_amd._native import native
    native().afm_train_step(a.X.data_ptr(), a.y.data_ptr(), B, F, a.par[0].data_ptr(),
                            a.par[1].data_ptr(), a.par[2].data_ptr(), M, k, A,
                            *[p.data_ptr() for p in a.par[3:7]], 0.1, 0.1, 0,
                            [s.data_ptr() for s in a.acc], a.w.data_ptr(), ws_bytes,
                            a.loss.data_ptr(), _stream())


def _afm_args(B, F, M, k, A):
    return _Args(B, F, M, k, [(k, A), (A,), (A,), (k,)])


def _dfm_call(a, B, F, M, k, dims, ws_bytes):
    from hhfm_amd._native import native
    L = len(dims)
    E, w, bp = a.par[:3]
    Ws, bs, Wp = a.par[3:3 + L], a.par[3 + L:3 + 2 * L], a.par[3 + 2 * L]
    acc = [a.acc[0], a.acc[1]] + a.acc[3:] + [a.acc[2]]       # E, w, W.., b.., Wp, bp
    native().dfm_train_step(a.X.data_ptr(), a.y.data_ptr(), B, F, E.data_ptr(), w.data_ptr(), M,
                            k, dims, [t.data_ptr() for t in Ws], [t.data_ptr() for t in bs],
                            Wp.data_ptr(), bp.data_ptr(), 0.1, 0.1, 0,
                            [t.data_ptr() for t in acc], a.w.data_ptr(), ws_bytes,
                            a.loss.data_ptr(), _stream())


def _dfm_args(B, F, M, k, dims):
    d = [F * k] + list(dims)
    return _Args(B, F, M, k, [(d[i], d[i + 1]) for i in range(len(dims))]
                 + [(n,) for n in dims] + [(F + k + dims[-1],)])


def test_hhfm_train_step_refuses_17_negatives():
    from hhfm_amd._native import native
    B, F, M, k = 8, 5, 40, 8
    a = _Args(B, F, M, k)
    a.ws(native().train_workspace(M, k))
    for NG, ok in ((17, False), (16, True)):
        Neg = _dev(np.random.default_rng(NG).integers(0, M, (B, NG)).astype(np.int32))
        if ok:
            _hhfm_call(a, Neg, B, F, M, k, a.w.numel())
            assert not a.unchanged()
        else:
            with pytest.raises(ValueError, match="unsupported"):
                _hhfm_call(a, Neg, B, F, M, k, a.w.numel())
            assert a.unchanged()


@pytest.mark.parametrize("F,k,A", [(17, 8, 8), (5, 6, 8), (5, 260, 8), (5, 8, 2)])
def test_afm_train_step_refuses_the_shape(F, k, A):
    B, M = 4, 40
    a = _afm_args(B, F, M, k, A)
    a.ws(1 << 22)
    with pytest.raises(ValueError, match="invalid argument"):
        _afm_call(a, B, F, M, k, A, a.w.numel())
    assert a.unchanged()


@pytest.mark.parametrize("F,k,dims", [(5, 8, [8, 8, 8, 8, 8]), (5, 8, [1012]), (5, 6, [12])])
def test_dfm_train_step_refuses_the_shape(F, k, dims):
    """Five layers, a concat width of F + k + d_L = 1025, k no multiple of 4."""
    B, M = 4, 40
    a = _dfm_args(B, F, M, k, dims)
    a.ws(1 << 22)
    with pytest.raises(ValueError, match="invalid argument"):
        _dfm_call(a, B, F, M, k, dims, a.w.numel())
    assert a.unchanged()


@pytest.mark.parametrize("model", ["fm", "hhfm", "afm", "dfm"])
def test_train_step_refuses_a_workspace_one_byte_short(model):
    """ws_bytes one short: the workspace error and untouched parameters; the
    exact size is taken (the same buffers, so the refusal was the size's)."""
    from hhfm_amd._native import native
    B, F, M, k, A, dims = 8, 5, 40, 8, 8, [12, 6]
    if model == "afm":
        a, need = _afm_args(B, F, M, k, A), native().afm_train_workspace(B, F, k, A, M)
        call = lambda n: _afm_call(a, B, F, M, k, A, n)  # noqa: E731
    elif model == "dfm":
        a, need = _dfm_args(B, F, M, k, dims), native().dfm_train_workspace(B, F, k, M, dims)
        call = lambda n: _dfm_call(a, B, F, M, k, dims, n)  # noqa: E731
    else:
        a, need = _Args(B, F, M, k), native().train_workspace(M, k)
        Neg = _dev(np.random.default_rng(3).integers(0, M, (B, 10)).astype(np.int32))
        call = ((lambda n: _fm_call(a, B, F, M, k, n)) if model == "fm"
                else (lambda n: _hhfm_call(a, Neg, B, F, M, k, n)))
    a.ws(need)
    with pytest.raises(ValueError, match="workspace too small"):
        call(need - 1)
    assert a.unchanged()
    call(need)
    assert not a.unchanged()
