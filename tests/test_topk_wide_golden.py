"""The CPU oracle against the reference's own ``topk(A, 100)`` lists
(tests/golden/topk_wide.npz, written by tests/golden/make_golden_topk_wide.py
from the reference's unmodified modules): FM, OUR in three layouts, AFM, DeepFM
and CARS2 at k = 16 on 320 items.

Positions must be array_equal; a differing position is allowed only as an fp32
tie confirmed in float64 (tests/helpers.topk_tie_swaps), at most 2 per case —
the project's existing cap.  The GPU models are held to the same file by the
same rule (tests/test_gpu_topk_wide_models.py).
"""
import os

import numpy as np
import pytest

from oracle import fm_oracle as orc
from oracle import parity
from tests.helpers import topk_tie_swaps

G = os.path.join(os.path.dirname(__file__), "golden", "topk_wide.npz")
MAX_TIES = 2
CASES = ("fm", "hhfm_frappe", "hhfm_jiaju", "hhfm_resturant", "afm", "dfm", "cars2")


def case(d, name):
    p = name + "_"
    return {k[len(p):]: v for k, v in d.items() if k.startswith(p)}


def _row_exact(A, n_user, rows_exact):
    """exact(b, ids) from a float64 row scorer: query b with item ids in column 1."""
    A = np.asarray(A, np.int64)

    def exact(b, ids):
        X = np.repeat(A[b:b + 1], len(ids), 0)
        X[:, 1] = n_user + np.asarray(ids, np.int64)
        return rows_exact(X)
    return exact


def oracle_lists(name, d, n_user, n_item, K=100):
    """(oracle top-K ids [B, K], exact) of one case of the fixture ``d``."""
    c = case(d, name)
    if name == "fm":
        sc = orc.fm_catalog_scores(c["A"], c["E"], c["w"], n_user, n_item)
        ex = parity.fm_exact(c["A"], c["E"], c["w"], n_user, ctx=(2, c["A"].shape[1]))
    elif name.startswith("hhfm"):
        fd, td = int(c["feature_dimension"]), int(c["time_dimension"])
        sc = orc.hhfm_catalog_scores(c["A"], c["E"], n_user, n_item, fd, td, True, td > 0)
        ex = parity.hhfm_exact(c["A"], c["E"], n_user, ctx=(2, 2 + fd),
                               time=(2 + fd, 2 + fd + td))
    elif name == "afm":
        args = (c["attention_W"], c["attention_b"], c["attention_p"], c["prediction"])
        sc = orc.afm_catalog_scores(c["A"], c["E"], c["w"], *args, n_user, n_item)
        ex = _row_exact(c["A"], n_user, lambda X: parity.afm_rows_exact(
            X, c["E"], c["w"], float(c["w0"]), *args))
    elif name == "dfm":
        n = sum(1 for k in c if k.startswith("layer_"))
        layers, biases = [c[f"layer_{i}"] for i in range(n)], [c[f"bias_{i}"] for i in range(n)]
        sc = orc.dfm_catalog_scores(c["A"], c["E"], c["w"], layers, biases,
                                    c["concat_projection"], c["concat_bias"], n_user, n_item)
        ex = _row_exact(c["A"], n_user, lambda X: parity.dfm_rows_exact(
            X, c["E"], c["w"], layers, biases, c["concat_projection"], c["concat_bias"]))
    else:
        from tests import cars2_ref as cr
        Wt = cr.weights(int(c["seed"]), n_user + n_item, int(d["cars2_Mc"]), 16)
        sc = cr.catalog_scores(c["q"], Wt, n_user, n_item)
        ex = cr.exact_catalog(c["q"], Wt, n_user)
    return orc.top_k(sc, K)[1], ex


def oracle_swaps(name, d, n_user, n_item):
    """Tie swaps between the oracle's list and the fixture's; None when a
    position differs that is no fp32 tie."""
    d = dict(d)
    d.setdefault("cars2_Mc", 11)
    ids, ex = oracle_lists(name, d, n_user, n_item)
    try:
        return topk_tie_swaps(ids, case(d, name)["topk_idx"].astype(np.int32), ex)
    except AssertionError:
        return None


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_the_reference_top_100(name):
    d = dict(np.load(G))
    nu, ni = int(d["n_user"]), int(d["n_item"])
    ref = case(d, name)["topk_idx"]
    assert ref.shape[1] == int(d["K"]) == 100 and ni >= 300
    ids, ex = oracle_lists(name, d, nu, ni)
    assert topk_tie_swaps(ids, ref.astype(np.int32), ex) <= MAX_TIES
