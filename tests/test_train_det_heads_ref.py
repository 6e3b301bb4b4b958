"""CPU checks of tests/train_det_heads_ref.py: ``head_sum`` is the scalar order
per column, the four known-answer inputs are exact in fp32 (asserted in
float64), the oracle's own step gives the same gradients to 1e-5 and leaves
the other variables alone, and every input has teeth — another summation order
changes the bits the GPU test compares."""
import numpy as np
import pytest

from oracle import fm_oracle as orc
from tests import train_det_heads_ref as hr
from tests import train_det_ref as dr

F32, F64 = np.float32, np.float64


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _orders(B):
    return [np.arange(B)[::-1], np.random.default_rng(1).permutation(B),
            np.random.default_rng(2).permutation(B)]


def _exact(prod32, a, b):
    """the float32 product equals the float64 one, elementwise"""
    return np.array_equal(np.asarray(prod32, F32).astype(F64),
                          np.asarray(a, F64) * np.asarray(b, F64))


def _close(got, want):
    want = np.asarray(want, F64)
    return np.allclose(got, want, rtol=1e-5, atol=1e-5 * max(np.abs(want).max(), 1e-30))


def test_head_sum_is_the_scalar_order_per_column():
    rng = np.random.default_rng(3)
    rows = (rng.normal(0, 1, (1031, 5)) * 2.0 ** rng.integers(-20, 20, (1031, 5))).astype(F32)
    want = np.array([dr.scalar_sum(rows[:, c]) for c in range(5)], F32)
    assert np.array_equal(_bits(hr.head_sum(rows)), _bits(want))
    # rows 0 and 256 meet in partial 0 before row 1 joins
    r = np.zeros((257, 1), F32)
    r[0], r[1], r[256] = 2.0 ** 24, 1.0, -2.0 ** 24
    assert hr.head_sum(r)[0] == 1.0 and dr.ordered_sum(r[:, 0]) == 0.0


def _afm_oracle_grads(d):
    par = d["par"]
    loss, *new, _ = orc.afm_train_step(d["X"], d["y"][:, None], *par, {}, 1.0, 0.0,
                                       optimizer="sgd")
    return loss, [np.asarray(o, F64).reshape(np.shape(n)) - np.asarray(n, F64)
                  for o, n in zip(par, new)]


@pytest.mark.parametrize("case", ["table", "head"])
def test_afm_known_answers_are_exact_and_match_the_oracle(case):
    d = hr.afm_table_known() if case == "table" else hr.afm_head_known()
    E, w, w0, W, b, pvec, P = d["par"]
    X = d["X"]
    assert np.array_equal(d["g"], -d["y"]) and not w.any() and w0 == 0
    if case == "table":
        assert X.shape == (3001, 2) and not E[0].any() and P.all()
        assert _exact(d["gP"], d["g"][:, None], P[None, :])
        assert _exact(d["c0"], d["gP"], d["e1"])
        assert np.array_equal(_bits(d["grads"][0][0]), _bits(dr.ordered_sum(d["c0"])))
    else:
        assert X.shape == (1031, 2) and not P.any()
        assert len(np.unique(X[:, 0])) == 37 and len(np.unique(X[:, 1])) == 5
        assert _exact(d["pr"], E[X[:, 0]], E[X[:, 1]])
        assert _exact(d["rowv"], d["g"][:, None], d["pr"])
        assert d["grads"][6].all()
    loss, got = _afm_oracle_grads(d)
    assert np.isclose(loss, d["loss"], rtol=1e-5)
    for n, g, want in zip("E w w0 W b pvec P".split(), got, d["grads"]):
        assert _close(g, want), n
        if not np.any(want):
            assert not np.any(g), n                      # the other variables are unchanged


def _dfm_oracle_grads(d):
    E, w, layers, biases, Wp, bp = d["par"]
    loss, E1, w1, L1, b1, Wp1, bp1, _ = orc.dfm_train_step(d["X"], d["y"][:, None], E, w, layers,
                                                           biases, Wp, bp, {}, 1.0, 0.0,
                                                           optimizer="sgd")
    sub = lambda o, n: np.asarray(o, F64) - np.asarray(n, F64).reshape(np.shape(o))  # noqa: E731
    return loss, dict(E=sub(E, E1), w=sub(w, w1), Wp=sub(Wp, Wp1), bp=sub(bp, bp1),
                      layers=[sub(o, n) for o, n in zip(layers, L1)],
                      biases=[sub(o, n) for o, n in zip(biases, b1)])


@pytest.mark.parametrize("case", ["table", "head"])
def test_dfm_known_answers_are_exact_and_match_the_oracle(case):
    d = hr.dfm_table_known() if case == "table" else hr.dfm_head_known()
    E, w, layers, biases, Wp, bp = d["par"]
    F, k = 2, 8
    assert np.array_equal(d["g"], -d["y"]) and bp == 0 and not E[0].any()
    loss, got = _dfm_oracle_grads(d)
    assert np.isclose(loss, d["loss"], rtol=1e-5)
    assert _close(got["E"], d["dE"]) and _close(got["w"], d["dw"]) and _close(got["bp"], d["dbp"])
    for g in got["layers"] + got["biases"]:
        assert not np.any(g)
    if case == "table":
        assert Wp[:F + k].all() and not Wp[F + k:].any() and not w.any()
        assert _exact(d["gW"], d["g"][:, None], Wp[None, F:F + k])
        assert _exact(d["c0"], d["gW"], d["e1"])
        assert _exact(d["dw"][1:], d["g"], Wp[1])
        assert not np.any(got["Wp"][:F + k])
    else:
        assert not Wp.any() and w[1:].all() and w[0] == 0
        assert _exact(d["rowv"], d["g"], w[1:])
        assert _close(got["Wp"], d["dWp"]) and d["dWp"][1] != 0
        assert not np.any(got["E"]) and not np.any(got["w"])


def test_known_answers_have_teeth():
    """Reversed and two seeded permutations of the rows change the bits of at
    least half the columns of each case's ordered sum."""
    t, h = hr.afm_table_known(), hr.afm_head_known()
    dt, dh = hr.dfm_table_known(), hr.dfm_head_known()
    for p in _orders(len(t["c0"])):
        for d, want in ((t, t["grads"][0][0]), (dt, dt["dE"][0])):
            changed = _bits(dr.ordered_sum(d["c0"][p])) != _bits(want)
            assert changed.sum() >= changed.size // 2, changed
    for p in _orders(len(h["rowv"])):
        changed = _bits(hr.head_sum(h["rowv"][p])) != _bits(h["grads"][6])
        assert changed.sum() >= changed.size // 2, changed
        assert _bits(dr.scalar_sum(dh["rowv"][p])) != _bits(dh["dWp"][1])
