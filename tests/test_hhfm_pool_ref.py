"""tests/hhfm_pool_ref.py on the CPU (no extension build needed): the numpy
restatement of HHFM with MAX / MEAN pooling against the reference's own
outputs (tests/golden/hhfm_pool.npz, hhfm_pool_losses.npz: the unmodified
OurModel7 graph with Pooling1C / 1T / 1F set to tf.reduce_max / reduce_mean),
against the sum-pooling oracle and references it must reduce to, and its
float64 gradient against central differences; and the input condition of
tests/test_gpu_hhfm_pool.py — the fp32 restatement alone sits well inside the
bound the GPU step is held to, on every case."""
import os

import numpy as np
import pytest

from oracle import fm_oracle as orc
from tests import hhfm_pool_ref as pr
from tests import train_ref as tr
from tests.helpers import kappa_check

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TRIPLES = [("max", "max", "max"), ("mean", "mean", "mean"), ("max", "max", "sum"),
           ("mean", "max", "sum")]
LAYOUTS = ["frappe", "jiaju", "resturant"]


def golden_layout(tag):
    """E, X, A, n_user, n_item, ctx, tim of a golden layout (A: the recorded
    re-drawn queries of hhfm_pool.npz where the committed ones held a near-tie)."""
    g = np.load(os.path.join(GOLD, f"hhfm_{tag}.npz"))
    p = np.load(os.path.join(GOLD, "hhfm_pool.npz"))
    fd, td = int(g["feature_dimension"]), int(g["time_dimension"])
    A = p[f"{tag}_A"] if int(p[f"{tag}_A_seed"]) >= 0 else g["A"]
    ctx = (2, 2 + fd)
    tim = (2 + fd, 2 + fd + td) if td else (0, 0)
    return g["E"], g["X"], A, int(g["n_user"]), int(g["n_item"]), ctx, tim


@pytest.mark.parametrize("triple", TRIPLES, ids="_".join)
@pytest.mark.parametrize("tag", LAYOUTS)
def test_restatement_equals_the_reference_outputs(tag, triple):
    E, X, A, nu, ni, ctx, tim = golden_layout(tag)
    p = np.load(os.path.join(GOLD, "hhfm_pool.npz"))
    key = f"{tag}_{'_'.join(triple)}"
    exact, mag = pr.exact_rows(X, E, ctx, tim, triple)
    kappa_check(f"pool_ref_out_{key}", pr.score_rows(X, E, ctx, tim, triple), p[key + "_out"],
                exact, mag)
    kappa_check(f"pool_golden_out_{key}", p[key + "_out"], None, exact, mag)
    sc = pr.catalog_scores(A, E, nu, ni, ctx, tim, triple)
    _, idx = orc.top_k(sc, 20)
    assert np.array_equal(idx, p[key + "_topk_idx"])
    top21 = -np.sort(-sc, axis=1)[:, :21]
    scale = np.abs(top21).max()
    assert np.abs(top21 - p[key + "_top21"]).max() <= 1e-5 * scale


@pytest.mark.parametrize("triple", TRIPLES, ids="_".join)
@pytest.mark.parametrize("tag", ["frappe", "jiaju"])
def test_restated_loss_equals_the_reference_loss(tag, triple):
    L = np.load(os.path.join(GOLD, "hhfm_pool_losses.npz"))
    fd, td = int(L[f"{tag}_feature_dimension"]), int(L[f"{tag}_time_dimension"])
    ctx, tim = (2, 2 + fd), ((2 + fd, 2 + fd + td) if td else (0, 0))
    assert (L[f"{tag}_Neg"][3, 4] == L[f"{tag}_Neg"][3, 7])            # the planted tie
    loss, _ = pr.train_step(L[f"{tag}_X"], L[f"{tag}_Neg"], L[f"{tag}_E"], None, 1.0,
                            float(L["lamda"]), ctx, tim, triple, grad_only=True)
    ref = float(L[f"{tag}_{'_'.join(triple)}_loss"])
    assert abs(loss - ref) <= 1e-5 * abs(ref), (loss, ref)


@pytest.mark.parametrize("name", sorted(tr.HHFM_CASES))
def test_sum_pooling_is_the_existing_reference(name):
    """(sum, sum, sum): hhfm_pool_grad64 is train_ref.hhfm_grad64 exactly and
    the forward is the oracle's bit for bit."""
    layout = tr.HHFM_CASES[name][0]
    fd, td = tr.LAYOUTS[layout]
    X, Neg, E, ctx, tim, ties = tr.hhfm_case(name)
    sss = ("sum", "sum", "sum")
    assert np.array_equal(pr.tie_mask(X, Neg, E, ctx, tim, sss), ties)
    a = tr.hhfm_grad64(X, Neg, E, ctx, tim, ties)
    b = pr.hhfm_pool_grad64(X, Neg, E, ctx, tim, ties, sss)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3]["z"], b[3]["z"]) and a[3]["margin"] == b[3]["margin"]
    if fd:      # the oracle's column split needs context columns
        ref = orc.hhfm_positive_feedback(X, E, fd, td, True, td > 0)[:, 0]
        got = pr.score_rows(X, E, ctx, tim, sss)
        assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))


def _fd(loss, arr, i, eps=1e-6):
    a = np.array(arr, np.float64)
    a[i] += eps
    lp = loss(a)
    a[i] -= 2 * eps
    return (lp - loss(a)) / (2 * eps)


ALL_TRIPLES = TRIPLES + [("sum", "max", "mean"), ("sum", "mean", "max"), ("max", "sum", "max")]


@pytest.mark.parametrize("triple", ALL_TRIPLES, ids="_".join)
@pytest.mark.parametrize("layout", sorted(tr.LAYOUTS))
def test_pool_grad64_matches_finite_differences(layout, triple):
    """Untied inputs (a continuous draw: every maximum is unique), every
    layout; the loss differentiated is the pooled graph itself in float64."""
    rng = np.random.default_rng(11)
    fd_, td = tr.LAYOUTS[layout]
    k, B, NG = 4, 12, 5
    M = 40 + 5 * fd_
    X = np.stack([rng.integers(0, 10, B), rng.integers(10, 40, B)]
                 + [rng.integers(40 + 5 * f, 45 + 5 * f, B) for f in range(fd_)]
                 + [rng.integers(10, 40, B) for _ in range(td)], 1)
    for r in range(B):       # distinct ids inside a row: no pool holds a tie
        while len(set(X[r, 2:])) < X.shape[1] - 2:
            X[r, 2 + fd_:] = rng.integers(10, 40, td)
    Neg = np.stack([rng.permutation(np.arange(10, 40))[:NG] for _ in range(B)])
    E = rng.normal(0, 0.5, (M, k)).astype(np.float32)
    ctx = (2, 2 + fd_) if fd_ else (0, 0)
    tim = (2 + fd_, 2 + fd_ + td) if td else (0, 0)
    ties = pr.tie_mask(X, Neg, E, ctx, tim, triple)
    assert (ties.sum(1) == 1).all()
    l0, dE, mE, info = pr.hhfm_pool_grad64(X, Neg, E, ctx, tim, ties, triple)
    E64 = E.astype(np.float64)
    loss = lambda Ev: pr.loss64(X, Neg, Ev, ctx, tim, triple)  # noqa: E731
    assert np.isclose(l0, loss(E64), rtol=1e-12) and info["margin"] > 1e-4
    ids = [(X[0, 0], 1), (X[1, 1], 2), (Neg[3, 1], 0), (X[2, 0], 2), (X[4, X.shape[1] - 1], 1),
           (X[5, 2 % X.shape[1]], 3), (X[6, X.shape[1] - 1], 0)]
    for i in ids:
        assert np.isclose(dE[i], _fd(loss, E64, i), rtol=1e-6, atol=1e-8), i
    assert np.all(mE >= np.abs(dE) * (1 - 1e-12))


def test_max_gradient_is_split_between_equal_values():
    """One context id twice in a row, two ids with equal rows, and a context
    id equal to the user id under final max: every holder of the maximum takes
    an equal share (TF _MinOrMaxGrad), and the shares sum to dh."""
    rng = np.random.default_rng(3)
    E = rng.normal(0, 0.5, (12, 4)).astype(np.float32)
    E[7] = E[6]
    E[5] = np.abs(E[5]) + 3                       # the largest row everywhere
    ctx, tim, mmm = (2, 5), (0, 0), ("max", "max", "max")
    for X, shares in ((np.array([[0, 1, 5, 5, 8]]), {5: 1.0}),                 # one id twice
                      (np.array([[0, 1, 6, 7, 8]]), None),                     # twin rows
                      (np.array([[5, 1, 5, 6, 8]]), {5: 1.0})):                # ctx id == user id
        cols, W = pr.pool_weights(X, E, ctx, tim, mmm)
        assert np.allclose(W.sum(1), 1.0)
        if shares:
            assert np.allclose(W[0, [j for j, c in enumerate(cols) if X[0, c] == 5]].sum(0), 1.0)
        else:
            assert np.array_equal(W[0, 1], W[0, 2])
    # context values all negative at an element: max is the largest of them, not 0
    En = -np.abs(E) - 1
    h = pr.hybrid(En, np.array([[0, 1, 2, 3, 4]]), ctx, tim, ("max", "max", "sum"))
    assert np.array_equal(h[0], En[0] + En[[2, 3, 4]].max(0))


@pytest.mark.parametrize("name", sorted(pr.POOL_CASES))
def test_pool_inputs_keep_the_fp32_restatement_inside_the_bound(name):
    """Per case: the planted rows are what they claim, the float64 forward with
    the fp32 selections is the pooled graph's own float64 value, few rows were
    redrawn, and one restated fp32 SGD step (lr 1, λ 0) sits within 0.25 of
    the bound of train_ref.ratio."""
    X, Neg, E, ctx, tim, ties, pooling, info = pr.hhfm_pool_case(name)
    B = len(X)
    assert info["redrawn"] <= 0.05 * B
    f = pr._cols(ctx) + pr._cols(tim)
    if B > 8 and len(f) >= 2:
        assert X[4, 2] == X[4, 0] and X[5, f[0]] == X[5, f[1]]
        assert X[6, f[0]] != X[6, f[1]] and np.array_equal(E[X[6, f[0]]], E[X[6, f[1]]])
        assert (E[X[7, f], 0] < 0).all()
    cols, W = pr.pool_weights(X, E, ctx, tim, pooling)
    E64 = E.astype(np.float64)
    h_sel = (W * E64[X[:, cols].astype(np.int64)]).sum(1)
    h_own = pr.hybrid(E64, X, ctx, tim, pooling, dtype=np.float64)
    assert np.allclose(h_sel, h_own, rtol=1e-12, atol=1e-15)
    _, dE, mE, gi = pr.hhfm_pool_grad64(X, Neg, E, ctx, tim, ties, pooling)
    assert np.abs(gi["z"]).max() <= 4 and gi["margin"] > 1e-5
    _, g32 = pr.train_step(X, Neg, E, None, 1.0, 0.0, ctx, tim, pooling, grad_only=True)
    E1 = (E - g32).astype(np.float32)
    r = tr.ratio(E.astype(np.float64) - E1, E, E1, dE, mE)
    print(f"hhfm pool {name}: redrawn {info['redrawn']}, fp32 restatement err / bound = {r:.3g}")
    assert r <= 0.25
