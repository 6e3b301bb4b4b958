"""tests/hhfm_two_way_ref.py on the CPU (no extension build needed): the numpy
restatement of the two-way HHFM model against the reference's own pair-product
tensors (tests/golden/hhfm_two_way.npz: the unmodified OurModel7 graph's
stack_features, mixdouble_features_context / _time and hybrid_feature2d), its
float64 gradient against central differences under the bars of
tests/test_hhfm_pool_ref.py, and the admissibility conditions of every case
tests/test_gpu_hhfm_two_way.py runs."""
import os

import numpy as np
import pytest

from tests import hhfm_pool_ref as pr
from tests import hhfm_two_way_ref as tw
from tests import train_ref as tr
from tests.test_hhfm_pool_ref import _fd

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LAYOUTS = ["frappe", "jiaju", "resturant"]


def _six(key):
    a, b = key.split("__")
    return tuple(a.split("_")), tuple(b.split("_"))


G2 = np.load(os.path.join(GOLD, "hhfm_two_way.npz"))
SEXTUPLES = [_six(str(k)) for k in G2["sextuples"]]
SIX_IDS = [str(k) for k in G2["sextuples"]]


def golden_layout2(tag):
    """E (the committed table times the recorded power of two), the 64 rows X,
    the recorded queries A, n_user, n_item, ctx, tim."""
    g = np.load(os.path.join(GOLD, f"hhfm_{tag}.npz"))
    fd, td = int(g["feature_dimension"]), int(g["time_dimension"])
    ctx = (2, 2 + fd)
    tim = (2 + fd, 2 + fd + td) if td else (0, 0)
    return (g["E"] * G2["scale"], g["X"][:int(G2["rows"])], G2[f"{tag}_A"], int(g["n_user"]),
            int(g["n_item"]), ctx, tim)


@pytest.mark.parametrize("n", range(len(SEXTUPLES)), ids=SIX_IDS)
@pytest.mark.parametrize("tag", LAYOUTS)
def test_restated_blocks_equal_the_reference_tensors(tag, n):
    """P1 (inside stack_features), P2 of both pools and H2 over the reference's
    one-way stack, bit for bit: the pair order and what Pooling2* reduces."""
    E, X, _, _, _, ctx, tim = golden_layout2(tag)
    p1, p2 = SEXTUPLES[n]
    Er = np.ascontiguousarray(E[:, :int(G2["kref"])])
    Xl = X.astype(np.int64)
    stack = G2[f"{tag}_stack_features"][n]
    mc, mt, mf = pr.modes_of(p1)
    mc2, mt2, mf2 = pr.modes_of(p2)
    P1c, P2c, _ = tw.mix(Er[Xl[:, pr._cols(ctx)]], mc, mc2)
    assert np.array_equal(stack[:, 0], Er[Xl[:, 0]])
    assert np.array_equal(stack[:, 1], P1c)
    assert np.array_equal(G2[f"{tag}_mixdouble_features_context"][n], P2c)
    if pr._cols(tim):
        P1t, P2t, _ = tw.mix(Er[Xl[:, pr._cols(tim)]], mt, mt2)
        assert np.array_equal(stack[:, 2], P1t)
        assert np.array_equal(G2[f"{tag}_mixdouble_features_time"][n], P2t)
    # the stack level, fed the reference's own one-way stack
    members = [stack[:, m] for m in range(stack.shape[1])]
    h1, h2 = tw.stack2(members, mf, mf2)
    assert np.array_equal(G2[f"{tag}_hybrid_feature2d"][n], h2)
    assert np.array_equal(h1, pr._final(members, mf))


@pytest.mark.parametrize("n", range(len(SEXTUPLES)), ids=SIX_IDS)
@pytest.mark.parametrize("tag", LAYOUTS)
def test_restated_entries_are_the_restatement_and_the_gap_holds(tag, n):
    E, X, A, nu, ni, ctx, tim = golden_layout2(tag)
    six = SEXTUPLES[n]
    assert np.array_equal(G2[f"{tag}_restated_out"][n], tw.score_rows2(X, E, ctx, tim, *six))
    exact = tw.exact_catalog2(A, E, nu, ctx, tim, *six)
    for b in range(len(A)):
        s, mag = exact(b, np.arange(ni))
        order = np.argsort(-s, kind="stable")[:21]
        assert np.min(-np.diff(s[order])) > 1e-5 * mag.max()
        assert np.array_equal(order[:20], G2[f"{tag}_restated_topk_idx"][n][b])
    assert tw.pair_share(X, E, ctx, tim, *six).min() >= 0.10


def test_known_answer_all_sum():
    """h = u + (a + b + ab) + u·(a + b + ab) on exact values."""
    E = np.array([[1, 2, -0.5, 4], [2, 1, 1, -1], [0.5, -2, 3, 1], [4, 0.25, -1, 2]], np.float32)
    X = np.array([[0, 1, 2, 3]])
    u, a, b = E[0], E[2], E[3]
    m = a + b + a * b
    h = tw.hybrid2(E, X, (2, 4), (0, 0), tw.SSS, tw.SSS)
    assert np.array_equal(h[0], u + m + u * m)


SIX_FD = SEXTUPLES + [(("sum", "max", "mean"), ("max", "mean", "sum")),
                      (("mean", "sum", "max"), ("sum", "max", "mean"))]


@pytest.mark.parametrize("six", SIX_FD, ids=lambda s: "_".join(s[0]) + "__" + "_".join(s[1]))
@pytest.mark.parametrize("layout", ["ctx", "time", "both"])
def test_grad64_matches_finite_differences(layout, six):
    """Untied inputs, every layout the contract admits; the loss differentiated
    is the two-way graph itself in float64 (test_hhfm_pool_ref's bars)."""
    rng = np.random.default_rng(12)
    fd_, td = tr.LAYOUTS[layout]
    k, B, NG = 4, 12, 5
    M = 40 + 5 * fd_
    X = np.stack([rng.integers(0, 10, B), rng.integers(10, 40, B)]
                 + [rng.integers(40 + 5 * f, 45 + 5 * f, B) for f in range(fd_)]
                 + [rng.integers(10, 40, B) for _ in range(td)], 1)
    for r in range(B):
        while len(set(X[r, 2:])) < X.shape[1] - 2:
            X[r, 2 + fd_:] = rng.integers(10, 40, td)
    Neg = np.stack([rng.permutation(np.arange(10, 40))[:NG] for _ in range(B)])
    E = rng.normal(0, 0.5, (M, k)).astype(np.float32)
    ctx = (2, 2 + fd_) if fd_ else (0, 0)
    tim = (2 + fd_, 2 + fd_ + td) if td else (0, 0)
    ties = tw.tie_mask2(X, Neg, E, ctx, tim, *six)
    assert (ties.sum(1) == 1).all()
    l0, dE, mE, info = tw.grad64(X, Neg, E, ctx, tim, ties, *six)
    E64 = E.astype(np.float64)
    loss = lambda Ev: tw.loss64(X, Neg, Ev, ctx, tim, *six)  # noqa: E731
    assert np.isclose(l0, loss(E64), rtol=1e-12) and info["margin"] > 1e-4
    ids = [(X[0, 0], 1), (X[1, 1], 2), (Neg[3, 1], 0), (X[2, 0], 2), (X[4, X.shape[1] - 1], 1),
           (X[5, 2], 3), (X[6, X.shape[1] - 1], 0), (X[7, 3], 2)]
    for i in ids:
        assert np.isclose(dE[i], _fd(loss, E64, i), rtol=1e-6, atol=1e-8), i
    assert np.all(mE >= np.abs(dE) * (1 - 1e-12))


@pytest.mark.parametrize("name", sorted(tw.TWO_WAY_CASES))
def test_cases_are_admissible(name):
    """Asserted, not assumed: the planted rows are what they claim; every max
    pool of either level selects alike in fp32 and float64; |z| <= 4; the BPR
    margin; every row is in the comparison; and the fp32 restatement alone
    sits inside the bound the GPU step is held to (its share is printed)."""
    X, Neg, E, ctx, tim, ties, p1, p2, info = tw.two_way_case(name)
    B = len(X)
    assert info["rows"] == B and info["redrawn"] <= max(1, 0.1 * B)
    f = pr._cols(ctx) + pr._cols(tim)
    if B > 8:
        assert X[4, f[0]] == X[4, 0] and X[5, f[0]] == X[5, f[1]]
        assert X[6, f[0]] != X[6, f[1]] and np.array_equal(E[X[6, f[0]]], E[X[6, f[1]]])
        assert (E[X[7, f], 0] < 0).all()
        if Neg.shape[1] >= 2:
            assert ties[3].sum() >= 2
    assert tw.admissible(X, E, ctx, tim, p1, p2).all()
    _, dE, mE, gi = tw.grad64(X, Neg, E, ctx, tim, ties, p1, p2)
    assert np.abs(gi["z"]).max() <= 4 and gi["margin"] > 1e-5
    assert tw.pair_share(X, E, ctx, tim, p1, p2).min() >= 0.10
    _, g32 = tw.train_step2(X, Neg, E, None, 1.0, 0.0, ctx, tim, p1, p2, grad_only=True)
    E1 = (E - g32).astype(np.float32)
    r = tr.ratio(E.astype(np.float64) - E1, E, E1, dE, mE)
    print(f"hhfm two-way {name}: redrawn {info['redrawn']}, fp32 restatement err / bound = {r:.3g}")
    assert r < 1.0
