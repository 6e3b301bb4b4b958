"""tests/train_ref.py on the CPU: the float64 gradient references against
central finite differences of a float64 loss, their magnitudes, and the input
condition of tests/test_gpu_train_grad.py — the fp32 oracle alone
(oracle/fm_oracle.py: float32, np.add.at) must sit well inside the bound the
GPU is held to, on every case."""
import numpy as np
import pytest

from oracle import fm_oracle as orc
from tests import train_ref as tr


def _fd(loss, arr, i, eps=1e-6):
    a = np.array(arr, np.float64)
    a[i] += eps
    lp = loss(a)
    a[i] -= 2 * eps
    return (lp - loss(a)) / (2 * eps)


def test_fm_grad64_matches_finite_differences():
    rng = np.random.default_rng(0)
    M, k, B, F = 30, 4, 20, 5
    X = rng.integers(0, M, (B, F))
    X[0, 3] = X[0, 2]                       # one id twice in a row
    X[1, :] = X[1, 0]                       # one id in every column
    y = rng.integers(0, 2, B).astype(np.float64)
    E, w, w0 = rng.normal(0, 0.3, (M, k)), rng.normal(0, 0.3, M), 0.05

    def loss(E, w, w0):
        e = E[X]
        s = e.sum(1)
        out = (0.5 * (s * s - (e * e).sum(1))).sum(1) + w[X].sum(1) + w0
        return ((y - out) ** 2).sum() / 2

    l0, (dE, dw, dw0), (mE, mw, mw0) = tr.fm_grad64(X, y, E, w, w0)
    assert np.isclose(l0, loss(E, w, w0), rtol=1e-13)
    free = int(np.setdiff1d(np.arange(M), X)[0])
    for i in [(X[0, 2], 1), (X[1, 0], 3), (X[3, 0], 0), (X[5, 4], 2), (free, 2)]:
        assert np.isclose(dE[i], _fd(lambda a: loss(a, w, w0), E, i), rtol=1e-7, atol=1e-8), i
    assert dE[free, 2] == 0 and mE[free, 2] == 0
    for i in [(X[0, 2],), (X[1, 0],), (X[7, 1],)]:
        assert np.isclose(dw[i], _fd(lambda a: loss(E, a, w0), w, i), rtol=1e-7, atol=1e-8), i
    assert np.isclose(dw0, _fd(lambda a: loss(E, w, a[0]), [w0], (0,)), rtol=1e-7)
    # the magnitude bounds the gradient (triangle inequality, S_b >= 0)
    assert np.all(mE >= np.abs(dE)) and np.all(mw >= np.abs(dw)) and mw0 >= abs(dw0)


@pytest.mark.parametrize("layout", sorted(tr.LAYOUTS))
def test_hhfm_grad64_matches_finite_differences(layout):
    """Every layout; a row whose maximum negative id appears twice (the split
    halves sum to the whole: still differentiable) and a context id equal to
    the user id."""
    rng = np.random.default_rng(1)
    fd_, td = tr.LAYOUTS[layout]
    k, B, NG = 4, 12, 5
    M = 40 + 5 * fd_
    X = np.stack([rng.integers(0, 10, B), rng.integers(10, 40, B)]
                 + [rng.integers(40 + 5 * f, 45 + 5 * f, B) for f in range(fd_)]
                 + [rng.integers(10, 40, B) for _ in range(td)], 1)
    Neg = rng.integers(10, 40, (B, NG))
    E = rng.normal(0, 0.5, (M, k))
    ctx = (2, 2 + fd_) if fd_ else (0, 0)
    tim = (2 + fd_, 2 + fd_ + td) if td else (0, 0)
    cols = [0] + tr._field_cols(ctx, tim)
    if len(cols) > 1:
        X[2, 2] = X[2, 0]

    def loss(Ev):
        h = Ev[X[:, cols]].sum(1)
        z = (h * Ev[X[:, 1]]).sum(1) - np.einsum("bc,bjc->bj", h, Ev[Neg]).max(1)
        return -np.log(1 / (1 + np.exp(-z))).sum()

    h = E[X[0, cols]].sum(0)
    j = (E[Neg[0]] @ h).argmax()
    Neg[0, (j + 1) % NG] = Neg[0, j]
    ties = np.einsum("bc,bjc->bj", E[X[:, cols]].sum(1), E[Neg])
    ties = ties == ties.max(1, keepdims=True)
    assert ties[0].sum() >= 2
    l0, dE, mE, info = tr.hhfm_grad64(X, Neg, E, ctx, tim, ties)
    assert np.isclose(l0, loss(E), rtol=1e-13) and info["margin"] > 1e-4
    ids = [(X[0, 0], 1), (X[1, 1], 2), (Neg[0, j], 3), (Neg[3, 1], 0), (X[2, 0], 2),
           (X[4, cols[-1]], 1)]
    for i in ids:
        assert np.isclose(dE[i], _fd(loss, E, i), rtol=1e-6, atol=1e-8), i
    assert np.all(mE >= np.abs(dE))


def test_hhfm_grad64_splits_between_equal_rows():
    """Two negative ids with bit-identical rows: each takes half of what the
    maximum would take alone (TF _MaxGrad), and dh uses their mean."""
    X, Neg, E, ctx, tim, ties = tr.hhfm_case("both_ng10_k100")
    a, b = Neg[3, 0], Neg[3, 1]
    assert a != b and np.array_equal(E[a], E[b]) and ties[3].tolist() == [True] * 2 + [False] * 8
    row = slice(3, 4)
    _, d2, m2, _ = tr.hhfm_grad64(X[row], Neg[row], E, ctx, tim, ties[row])
    one = ties[row].copy()
    one[0, 1] = False
    Neg1 = Neg[row].copy()
    Neg1[0, 1] = Neg1[0, 2]                  # the twin replaced by an untied negative
    _, d1, m1, _ = tr.hhfm_grad64(X[row], Neg1, E, ctx, tim, one)
    assert np.allclose(d2[a], 0.5 * d1[a], rtol=1e-12) and np.allclose(d2[b], d2[a], rtol=1e-12)
    assert np.allclose(m2[a] + m2[b], m1[a], rtol=1e-12)
    u = X[3, 0]
    assert np.allclose(d2[u], d1[u], rtol=1e-12)


def _oracle_fm(name):
    X, y, E, w, w0 = tr.fm_case(name)
    _, (dE, dw, dw0), (mE, mw, mw0) = tr.fm_grad64(X, y, E, w, w0)
    _, E1, w1, w01, *_ = orc.fm_train_step(X, y, E, w, w0, None, None, None, 1.0, 0.0, "sgd")
    return max(tr.ratio(E - E1, E, E1, dE, mE), tr.ratio(w - w1, w, w1, dw, mw),
               tr.ratio(w0 - w01, w0, w01, dw0, mw0))


@pytest.mark.parametrize("name", sorted(tr.FM_CASES))
def test_fm_inputs_keep_the_fp32_oracle_inside_the_bound(name):
    k, F, B, M, *_ = tr.FM_CASES[name]
    X = tr.fm_case(name)[0]
    assert np.bincount(X.reshape(-1)).max() <= 4200      # contributions per table row
    r = _oracle_fm(name)
    print(f"fm {name}: fp32 oracle err / bound = {r:.3g}")
    assert r <= 0.25


@pytest.mark.parametrize("name", sorted(tr.HHFM_CASES))
def test_hhfm_inputs_keep_the_fp32_oracle_inside_the_bound(name):
    layout, NG, k, B = tr.HHFM_CASES[name]
    fd_, td = tr.LAYOUTS[layout]
    X, Neg, E, ctx, tim, ties = tr.hhfm_case(name)
    _, dE, mE, info = tr.hhfm_grad64(X, Neg, E, ctx, tim, ties)
    assert np.abs(info["z"]).max() <= 4 and info["margin"] > 1e-5
    if B > 4:
        nt = info["nt"]
        assert nt[1] == NG and abs(info["z"][2]) < 1e-12
        assert NG < 2 or (nt[0] >= 2 and nt[3] == 2 and Neg[3, 0] != Neg[3, 1])
        assert not (fd_ + td) or X[4, 2] == X[4, 0]
    _, E1, _ = orc.hhfm_train_step(X, Neg, E, None, 1.0, 0.0, fd_, td, fd_ > 0, td > 0, "sgd")
    r = tr.ratio(E - E1, E, E1, dE, mE)
    print(f"hhfm {name}: fp32 oracle err / bound = {r:.3g}")
    assert r <= 0.25
