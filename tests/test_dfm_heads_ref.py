"""tests/dfm_heads_ref.py pinned on the CPU: it equals the reference's own
numbers (tests/golden/dfm_heads.npz, written by make_golden_dfm_heads.py from
the unmodified DFM.py), with head 3 / mse it is oracle.fm_oracle's DeepFM, and
its float64 gradient is the finite difference of its float64 loss."""
import os

import numpy as np
import pytest

from oracle import fm_oracle as orc
from tests import dfm_heads_ref as hr

G = os.path.join(os.path.dirname(__file__), "golden")
HEADS = sorted(hr.HEADS)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "dfm_heads.npz")))


def weights(d, name):
    L = len(d["layer_dims"])
    return (d["E"], d["w"], [d[f"layer_{i}"] for i in range(L)],
            [d[f"bias_{i}"][0] for i in range(L)], d[f"{name}_concat_projection"][:, 0],
            np.float32(d[f"{name}_concat_bias"]))


@pytest.mark.parametrize("name", HEADS)
def test_restatement_equals_the_reference(gold, name):
    d = gold
    head = hr.head_word(*hr.HEADS[name])
    W = weights(d, name)
    assert len(W[4]) == hr.wp_size(head, 5, d["E"].shape[1], list(d["layer_dims"]))
    out, _, S = hr.forward(d["X"], *W, head)
    # the same float32 graph; only numpy's summation order inside matmul may differ
    assert np.all(np.abs(out - d[f"{name}_out"]) <= 1e-6 * S)
    nu, ni = int(d["n_user"]), int(d["n_item"])
    A = d[f"{name}_A"]
    sc, _, S = hr.forward(hr.catalog_rows(A, nu, ni), *W, head)
    sc, S = sc.reshape(len(A), ni), S.reshape(len(A), ni)
    assert np.all(np.abs(sc - d[f"{name}_topk_scores"]) <= 1e-6 * S)
    assert np.array_equal(orc.top_k(sc, 20)[1], d[f"{name}_topk_idx"])
    for tag in ("10", "1m"):
        loss = hr.loss32(d["X_loss"], d[f"Y_{tag}"], *W, head, float(d["l2"]))
        assert np.isclose(loss, d[f"{name}_loss_{tag}"], rtol=2e-6), (name, tag)


def test_fixture_rankings_are_separated(gold):
    """What make_golden_dfm_heads.py checked before it wrote the index lists:
    adjacent values of each query's 21 largest lie further apart than twice the
    tolerance of the ranking key — z (this code) and p (the reference's, under
    the sigmoid)."""
    d = gold
    nu, ni = int(d["n_user"]), int(d["n_item"])
    for name in HEADS:
        head = hr.head_word(*hr.HEADS[name])
        A = d[f"{name}_A"]
        out, z, S = hr.forward(hr.catalog_rows(A, nu, ni), *weights(d, name), head, dt=np.float64)
        keys = [(z, 1e-5 * S)]
        if head & hr.HEAD_SIGMOID:
            keys.append((out, 0.25e-5 * S + 4 * 2.0 ** -24))
        for v, tol in keys:
            v, tol = v.reshape(len(A), ni), tol.reshape(len(A), ni).max(1)
            for b in range(len(A)):
                top = np.sort(v[b])[::-1][:21]
                assert np.min(top[:-1] - top[1:]) > 2 * tol[b], name


def _case(rng, B, k, layers, nu=20, ni=40, scale=0.2):
    M = nu + ni + 12
    X = np.stack([rng.integers(0, nu, B), rng.integers(nu, nu + ni, B),
                  rng.integers(nu + ni, nu + ni + 7, B), rng.integers(nu + ni + 7, nu + ni + 9, B),
                  rng.integers(nu + ni + 9, M, B)], 1)
    E = rng.normal(0, scale, (M, k)).astype(np.float32)
    w = rng.uniform(0, 1, M).astype(np.float32)
    Ls, bs, fan = [], [], 5 * k
    for n in layers:
        g = np.sqrt(2.0 / (fan + n))
        Ls.append(rng.normal(0, g, (fan, n)).astype(np.float32))
        bs.append(rng.normal(0, g, n).astype(np.float32))
        fan = n
    return X, E, w, Ls, bs


def test_head3_mse_is_the_oracle():
    rng = np.random.default_rng(31)
    X, E, w, Ls, bs = _case(rng, 33, 8, [12, 10])
    Wp = rng.normal(0, 0.3, 5 + 8 + 10).astype(np.float32)
    bp = np.float32(0.01)
    y = rng.choice([1.0, -1.0], 33).astype(np.float32)
    out, z, _ = hr.forward(X, E, w, Ls, bs, Wp, bp, 3)
    assert np.array_equal(out, orc.dfm_out(X, E, w, Ls, bs, Wp[:, None], bp)[:, 0])
    acc = {kk: np.full_like(np.asarray(v, np.float32), 0.1)
           for kk, v in zip(hr.keys(2), [E, w] + Ls + bs + [Wp, bp])}
    for opt in ("adagrad", "adam"):
        slots = acc if opt == "adagrad" else {kk: np.zeros(2 * np.asarray(v).size, np.float32)
                                              for kk, v in acc.items()}
        mine = hr.train_step(X, y, E, w, Ls, bs, Wp, bp, slots, 0.05, 0.05, 3, opt)
        ref = orc.dfm_train_step(X, y, E, w, Ls, bs, Wp, bp, slots, 0.05, 0.05, optimizer=opt)
        assert mine[0] == ref[0]
        for a, b in zip(mine[1:3] + tuple(mine[3]) + tuple(mine[4]) + mine[5:7],
                        ref[1:3] + tuple(ref[3]) + tuple(ref[4]) + ref[5:7]):
            assert np.array_equal(a, b)
        for kk in ref[7]:
            assert np.array_equal(mine[7][kk], ref[7][kk])


@pytest.mark.parametrize("name", HEADS)
def test_variables_without_a_gradient_do_not_move(name):
    head = hr.head_word(*hr.HEADS[name])
    rng = np.random.default_rng(5)
    X, E, w, Ls, bs = _case(rng, 9, 4, [6, 5])
    Wp = rng.normal(0, 0.3, hr.wp_size(head, 5, 4, [6, 5])).astype(np.float32)
    acc = {kk: np.full_like(np.asarray(v, np.float32), 0.1)
           for kk, v in zip(hr.keys(2), [E, w] + Ls + bs + [Wp, np.float32(0)])}
    y = rng.choice([1.0, 0.0], 9).astype(np.float32)
    _, E1, w1, L1, b1, Wp1, bp1, acc1 = hr.train_step(X, y, E, w, Ls, bs, Wp, 0.0, acc, 0.1, 0.05,
                                                      head)
    assert not np.array_equal(E1, E) and not np.array_equal(Wp1, Wp)
    assert np.array_equal(w1, w) == (not head & hr.HEAD_FM)
    assert np.array_equal(acc1["w"], acc["w"]) == (not head & hr.HEAD_FM)
    for i in range(2):
        still = not head & hr.HEAD_DEEP
        assert np.array_equal(L1[i], Ls[i]) == still and np.array_equal(b1[i], bs[i]) == still
        assert np.array_equal(acc1[f"W{i}"], acc[f"W{i}"]) == still


@pytest.mark.parametrize("labels", ["10", "1m"])
@pytest.mark.parametrize("name", HEADS)
def test_gradient_matches_finite_differences(name, labels):
    """Central differences of the restated float64 loss (λ = 0) on a sample of
    every variable's elements; the log-loss rows keep ε in play (labels −1)."""
    head = hr.head_word(*hr.HEADS[name])
    rng = np.random.default_rng(17)
    X, E, w, Ls, bs = _case(rng, 12, 4, [6, 5])
    E, w = E.astype(np.float64), w.astype(np.float64)
    Ls, bs = [a.astype(np.float64) for a in Ls], [a.astype(np.float64) for a in bs]
    Wp = rng.normal(0, 0.4, hr.wp_size(head, 5, 4, [6, 5]))
    bp = 0.02
    y = rng.choice([1.0, 0.0 if labels == "10" else -1.0], 12)
    _, gr, mg, _ = hr.grad64(X, y, E, w, Ls, bs, Wp, bp, head)
    var = dict(zip(hr.keys(2), [E, w] + Ls + bs + [Wp, np.array([bp])]))

    def loss():
        return hr.grad64(X, y, var["E"], var["w"], [var["W0"], var["W1"]],
                         [var["b0"], var["b1"]], var["Wp"], float(var["bp"][0]), head)[0]

    for kk, v in var.items():
        if gr[kk] is None:
            # no gradient: the loss does not depend on the variable at all
            save, l0 = v.copy(), loss()
            v += 0.37
            assert loss() == l0, kk
            v[...] = save
            continue
        g = np.asarray(gr[kk], np.float64).reshape(-1)
        m = np.asarray(mg[kk], np.float64).reshape(-1)
        flat = v.reshape(-1)
        for j in rng.choice(flat.size, min(flat.size, 12), replace=False):
            h = 1e-5
            old = flat[j]
            flat[j] = old + h
            lp = loss()
            flat[j] = old - h
            lm = loss()
            flat[j] = old
            fd = (lp - lm) / (2 * h)
            assert abs(fd - g[j]) <= 1e-6 * max(abs(g).max(), 1e-3), (kk, j, fd, g[j])
            assert abs(g[j]) <= m[j] * (1 + 1e-12), (kk, j)   # the magnitude bounds the gradient
