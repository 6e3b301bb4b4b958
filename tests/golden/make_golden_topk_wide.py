#!/usr/bin/env python3
"""Golden top-100 lists from the REFERENCE ITSELF, for wide K.

Runs where make_golden.py runs (the reference tree present, never on the GPU
box).  It imports make_golden — which installs tf1_numpy, the toolz chunker and
np.int and imports the reference's unmodified Newcode modules — and records, in
topk_wide.npz, the reference's own ``topk(A, 100)`` for FM, OUR in its three
layouts (frappe: 3 context columns; jiaju: 5 context + 3 time columns;
resturant: 7 context + 5 time columns), AFM, DeepFM and
CARS2, with the weights and the queries, at k = 16 on 320 items (prefix
``<case>_``).  The weights are N(0, 0.1) from a seeded generator (the model's
own draws for AFM's attention net and DeepFM's layers, which come from
np.random inside the reference's constructors, are stored as drawn).

The CPU test holds the oracle to these lists with array_equal, a differing
position being allowed only as a float64-confirmed fp32 tie, at most 2 per
case; the query seed of each case is the first from its base for which the
oracle alone meets that on the CPU (the generator checks it and records the
seed).
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_topk_wide.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs tf1_numpy, imports the reference)
import numpy as np  # noqa: E402
import tf1_numpy  # noqa: E402

import Newcode.CARS2 as RC2  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import cars2_ref as cr  # noqa: E402
from tests import topk_wide_ref as wr  # noqa: E402

K, KF, NU, NI, QUERIES, STD = 100, 16, 40, 320, 8, 0.1
LAYOUTS = {"frappe": ((7, 2, 3), 0), "jiaju": ((5, 4, 3, 6, 2), 3), "resturant": ((4, 3, 5, 2, 6, 3, 2), 5)}


def table(rng, M):
    return rng.normal(0, STD, (M, KF)).astype(np.float32)


def gen_fm(seed):
    rng = np.random.default_rng(seed)
    ctx = (7, 2, 3)
    M = mg.vocab(NU, NI, ctx)
    m = mg.RFM.FM(5, M, NU, NI, KF, 0.1, 0.1, 1, "AdagradOptimizer", 0, 0)
    E, w = table(rng, M), rng.normal(0, STD, (M, 1)).astype(np.float32)
    m.weights["feature_embeddings"].value = E
    m.weights["feature_bias"].value = w
    A = mg.rows(rng, QUERIES, NU, NI, ctx)
    return dict(E=E, w=w[:, 0], A=A, topk_idx=np.asarray(m.topk(A, K)).astype(np.int16))


def gen_hhfm(tag, seed):
    rng = np.random.default_rng(seed)
    ctx, td = LAYOUTS[tag]
    M = mg.vocab(NU, NI, ctx)
    fd = len(ctx)
    m = mg.RM7.OUR(fd, td, M, NU, NI, KF, 0.1, 0.01, "AdagradOptimizer", True, td > 0)
    E = table(rng, M)
    m.weights["feature_embeddings"].value = E
    A = mg.rows(rng, QUERIES, NU, NI, ctx, td)
    return dict(E=E, A=A, feature_dimension=np.int64(fd), time_dimension=np.int64(td),
                topk_idx=np.asarray(m.topk(A, K)).astype(np.int16))


def gen_afm(seed):
    rng = np.random.default_rng(seed)
    np.random.seed(seed)       # AFM draws its attention weights from np.random
    ctx = (7, 2, 3)
    M = mg.vocab(NU, NI, ctx)
    m = mg.RAFM.AFM(NU, NI, M, 1, [KF, KF], None, 0.1, 100.0, [1, 1], "AdagradOptimizer", 0.999, 5)
    E, w = table(rng, M), rng.normal(0, STD, (M, 1)).astype(np.float32)
    m.weights["feature_embeddings"].value = E
    m.weights["feature_bias"].value = w
    m.weights["bias"].value = np.float32(0.02)
    A = mg.rows(rng, QUERIES, NU, NI, ctx)
    W = m.weights
    return dict(E=E, w=w[:, 0], w0=np.float32(0.02), A=A,
                attention_W=W["attention_W"].value, attention_b=W["attention_b"].value,
                attention_p=W["attention_p"].value, prediction=W["prediction"].value,
                topk_idx=np.asarray(m.topk(A, K)).astype(np.int16))


DFM_LAYERS = [32, 24]


def gen_dfm(seed):
    rng = np.random.default_rng(seed)
    np.random.seed(seed)       # DeepFM draws its layer weights from np.random
    ctx = (7, 2, 3)
    M = mg.vocab(NU, NI, ctx)
    m = mg.RDFM.DeepFM(NU, NI, M, 5, KF, list(DFM_LAYERS), tf1_numpy.nn.relu, 0.01, 0, 0.01)
    E, w = table(rng, M), rng.uniform(0, 1, (M, 1)).astype(np.float32)
    m.weights["feature_embeddings"].value = E
    m.weights["feature_bias"].value = w
    A = mg.rows(rng, QUERIES, NU, NI, ctx)
    W = m.weights
    out = dict(E=E, w=w[:, 0], A=A, concat_projection=W["concat_projection"].value,
               concat_bias=np.float32(W["concat_bias"].value),
               topk_idx=np.asarray(m.topk(A, K)).astype(np.int16))
    for i in range(len(DFM_LAYERS)):
        out[f"layer_{i}"] = W[f"layer_{i}"].value
        out[f"bias_{i}"] = W[f"bias_{i}"].value
    return out


CARS2_MC = 11


def gen_cars2(seed):
    Wt = cr.weights(seed, NU + NI, CARS2_MC, KF)
    m = RC2.CARS2(CARS2_MC, NU, NI, KF, 0.01, 0.0, "AdagradOptimizer")
    for name in cr.NAMES:
        m.weights[name].value = Wt[name]
    r = np.random.default_rng(seed + 1)
    q = np.stack([r.integers(0, NU, QUERIES), r.integers(0, CARS2_MC, QUERIES)], 1).astype(np.int32)
    pred = m.topk({"X": q[:, 0], "F1": q[:, 1]}, K)
    return dict(seed=np.int64(seed), q=q, topk_idx=np.asarray(pred).astype(np.int16))


CASES = {"fm": (gen_fm, 7100), "hhfm_frappe": (lambda s: gen_hhfm("frappe", s), 7200),
         "hhfm_jiaju": (lambda s: gen_hhfm("jiaju", s), 7300),
         "hhfm_resturant": (lambda s: gen_hhfm("resturant", s), 7400),
         "afm": (gen_afm, 7500), "dfm": (gen_dfm, 7600), "cars2": (gen_cars2, 7700)}


def main():
    from tests.test_topk_wide_golden import MAX_TIES, oracle_swaps
    out = {"n_user": np.int64(NU), "n_item": np.int64(NI), "K": np.int64(K),
           "cars2_Mc": np.int64(CARS2_MC), "dfm_layers": np.asarray(DFM_LAYERS, np.int64)}
    for name, (gen, base) in CASES.items():
        for seed in range(base, base + 50):
            case = gen(seed)
            case["case_seed"] = np.int64(seed)
            swaps = oracle_swaps(name, {f"{name}_{k}": v for k, v in case.items()}, NU, NI)
            if swaps is not None and swaps <= MAX_TIES:
                break
        else:
            raise SystemExit(f"{name}: no seed at which the oracle meets the fixture")
        print(name, "seed", seed, "oracle tie swaps", swaps)
        out.update({f"{name}_{k}": v for k, v in case.items()})
    assert wr.MAX_K >= K
    mg.save("topk_wide.npz", **out)


if __name__ == "__main__":
    main()
