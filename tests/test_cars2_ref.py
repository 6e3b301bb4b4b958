"""CARS2 on the CPU: tests/cars2_ref.py against the reference's own outputs
(tests/golden/cars2.npz, written by make_golden_cars2.py from the unmodified
Newcode/CARS2.py), its analytic gradients against central differences of its
float64 loss, the port's epoch loop against the reference's batch stream
(cars2_epoch_stream.json), and the fixture's and the GPU cases' tie conditions.

The batch stream pins ``feature_inject`` — an enumeration of a set of tuples,
whose iteration order is a property of the interpreter that generated it — so
it is a CPU test by nature."""
import argparse
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import parity
from tests import cars2_ref as cr

G = os.path.join(os.path.dirname(__file__), "golden")
GOLD = np.load(os.path.join(G, "cars2.npz"))
NU, NI, MC = int(GOLD["n_user"]), int(GOLD["n_item"]), int(GOLD["Mc"])


def golden(D):
    """-> weights, and the fixture's entries of that D without their prefix."""
    p = f"d{D}_"
    g = {k[len(p):]: GOLD[k] for k in GOLD.files if k.startswith(p)}
    return cr.weights(int(g["seed"]), NU + NI, MC, D), g


@pytest.mark.parametrize("D", [16, 64])
def test_ref_scores_equal_the_reference(D):
    """fp32 in the same op order: what differs is numpy's against tf1_numpy's
    summation inside a matmul / reduce_sum, so a few ulp of Σ|terms|."""
    Wt, g = golden(D)
    X = g["X"].astype(np.int64)
    exact, mag, share = cr.exact_rows(X, Wt)
    got = cr.score_rows(X, Wt)[:, 0]
    assert got.dtype == np.float32
    assert np.all(np.abs(got.astype(np.float64) - g["out"]) <= 4 * 2.0 ** -24 * mag)
    assert np.all(np.abs(g["out"] - exact) <= 1e-6 * mag)
    assert share.min() >= 0.1


@pytest.mark.parametrize("D", [16, 64])
def test_ref_topk_equals_the_reference(D):
    Wt, g = golden(D)
    q = g["q"].astype(np.int64)
    for dtype in (np.float32, np.float64):
        _, idx = cr.top_k(cr.catalog_scores(q, Wt, NU, NI, dtype), 20)
        assert np.array_equal(idx, g["topk_idx"])


@pytest.mark.parametrize("D", [16, 64])
def test_fixture_queries_have_no_near_ties(D):
    """The condition make_golden_cars2.py selected the query seed by."""
    Wt, g = golden(D)
    assert cr.min_top_gap(g["q"].astype(np.int64), Wt, NU, NI) > 1e-5
    r = np.random.default_rng(int(g["q_seed"]))
    q = np.stack([r.integers(0, NU, 8), r.integers(0, MC, 8)], 1)
    assert np.array_equal(q, g["q"])


@pytest.mark.parametrize("lam,tag", [(0.001, "1e-3"), (0.0, "0")])
@pytest.mark.parametrize("ng", [1, 3])
@pytest.mark.parametrize("D", [16, 64])
def test_ref_loss_equals_the_reference(D, ng, lam, tag):
    Wt, g = golden(D)
    X, Neg = g["X"].astype(np.int64), g[f"Neg{ng}"].astype(np.int64)
    if ng == 3:
        assert Neg[5, 2] == Neg[5, 0]
    want = float(g[f"loss_ng{ng}_lam{tag}"])
    got32 = float(cr.loss(X[:, :2], X[:, 2], Neg, Wt, lam))
    got64 = float(cr.loss(X[:, :2], X[:, 2], Neg, Wt, lam, np.float64))
    assert np.isclose(got32, want, rtol=2e-6), (got32, want)
    assert np.isclose(got64, want, rtol=1e-5), (got64, want)
    # the data loss of grad64 (the folded float64 form) is the same number
    assert np.isclose(cr.grad64(X[:, :2], X[:, 2], Neg, Wt)[0],
                      float(cr.loss(X[:, :2], X[:, 2], Neg, Wt, 0.0, np.float64)), rtol=1e-12)


@pytest.mark.parametrize("ng", [1, 3])
def test_analytic_gradients_match_central_differences(ng):
    """Every variable, a seeded sample of elements each; W and A: zero."""
    D = 16
    Wt, g = golden(D)
    Wt = {k: v.astype(np.float64) * (0.5 if k != "UI" else 1.0) for k, v in Wt.items()}
    X, Neg = g["X"].astype(np.int64), g[f"Neg{ng}"].astype(np.int64)
    args = (X[:, :2], X[:, 2], Neg)
    _, G, M, _ = cr.grad64(*args, Wt)
    rng = np.random.default_rng(5)
    h = 1e-6
    for name in cr.NAMES:
        flat = Wt[name].reshape(-1)
        for e in rng.choice(flat.size, size=min(flat.size, 12), replace=False):
            old = flat[e]
            flat[e] = old + h
            up = float(cr.loss(*args, Wt, 0.0, np.float64))
            flat[e] = old - h
            dn = float(cr.loss(*args, Wt, 0.0, np.float64))
            flat[e] = old
            fd = (up - dn) / (2 * h)
            an = G[name].reshape(-1)[e]
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)) + 1e-7, (name, e, fd, an)
            assert M[name].reshape(-1)[e] >= abs(an) * (1 - 1e-12)
    assert not G["W"].any() and not G["A"].any()


class _Recorder:
    def __init__(self):
        self.batches = []

    def partial_fit(self, data):
        h = hashlib.sha256()
        for key in sorted(data):
            a = np.ascontiguousarray(np.asarray(data[key], dtype=np.float64))
            h.update(key.encode())
            h.update(np.asarray(a.shape, np.int64).tobytes())
            h.update(a.tobytes())
        self.batches.append(h.hexdigest())
        return 1.0


def test_epoch_stream_matches_the_reference(capsys):
    """Train.__init__'s feature_inject, the in-place shuffle, NG = 1 and the
    host sampler's order: the batches the reference's own Train fed."""
    from hhfm_amd import CARS2
    from hhfm_amd.NewLoadData import LoadData
    ref = json.load(open(os.path.join(G, "cars2_epoch_stream.json")))
    np.random.seed(ref["loaddata_seed"])
    d = LoadData(G + "/", "synth_frappe")
    args = argparse.Namespace(Result=1, dataset="synth_frappe", result_file=None,
                              epoch=ref["epochs"] + 1, batch_size=ref["batch_size"], TopK=10,
                              hidden_factor=16, lr=0.01, lamda=0.001, keep=1,
                              optimizer="AdagradOptimizer", batch_norm=0)
    t = CARS2.Train(args, data=d, model=_Recorder())
    assert t.features_M == ref["features_M"]
    assert (t.eval_num, t.auc_first_chunk_only, t.auc_label_filter) == (300, True, False)
    np.random.seed(ref["seed"])
    t.train()
    assert len(t.model.batches) == len(ref["cars2"])
    assert t.model.batches == ref["cars2"]


def test_parse_args_defaults_are_the_references():
    from hhfm_amd.CARS2 import parse_args
    a = parse_args("frappe", 64, 10, [])
    assert (a.lamda, a.lr, a.epoch, a.batch_size, a.optimizer, a.hidden_factor, a.TopK) == \
        (0.001, 0.01, 60, 5000, "AdagradOptimizer", 64, 10)
    a = parse_args("frappe", 64, 10, ["--keep", "0.5", "--batch_norm", "1", "--deterministic", "1"])
    assert (a.keep, a.batch_norm, a.deterministic) == (0.5, 1, 1)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(cr.CATALOG_CASES))
def test_gpu_catalog_cases_keep_the_reference_within_the_tie_cap(name, dtype):
    """The seeds of the dense and streaming GPU cases: float32 in the
    reference's order against float64 differs in at most MAX_TIES positions of
    the top 64, each a verified tie, and the trilinear terms matter."""
    Wt, q, nu, ni = cr.catalog_case(name, dtype == "bf16")
    exact = cr.exact_catalog(q, Wt, nu)
    s64 = np.stack([exact(b, np.arange(ni))[0] for b in range(len(q))])
    _, r32 = cr.top_k(cr.catalog_reference(Wt, q, nu, ni), 64)
    _, r64 = cr.top_k(s64, 64)
    assert parity.topk_tie_swaps(r32, r64, exact) <= cr.MAX_TIES
    rows = np.stack([q[:, 0], nu + np.arange(len(q)) % ni, q[:, 1]], 1)
    assert cr.exact_rows(rows, Wt)[2].min() >= 0.1


def test_catalog_reference_is_catalog_scores():
    Wt, g = golden(16)
    q = g["q"].astype(np.int64)
    a, b = cr.catalog_scores(q, Wt, NU, NI), cr.catalog_reference(Wt, q, NU, NI)
    mag = cr.catalog_mag(Wt, q, NU, NI)
    assert np.all(np.abs(a.astype(np.float64) - b) <= 1e-6 * mag)
