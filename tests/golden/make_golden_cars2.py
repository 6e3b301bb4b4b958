#!/usr/bin/env python3
"""Golden vectors of CARS2 from the REFERENCE ITSELF.

Runs where make_golden.py runs (the reference tree present, never on the GPU
box).  It imports make_golden — which installs tf1_numpy, the toolz chunker
and np.int — and then the reference's unmodified Newcode/CARS2.py.

cars2.npz, for D = 16 and D = 64 (prefix d16_ / d64_):
  weights   NOT stored: tests/cars2_ref.weights(seed, n_ui, Mc, D) draws them
            from a legacy RandomState (a frozen stream) at std 0.3 with
            non-zero A and B — at the reference's initial A = B = 0 the
            trilinear terms vanish; the seed and the sizes are recorded
  X, out    64 rows (user id, item id, context id) and their PositiveFeadback
  q, q_seed, topk_idx   8 queries (user id, context id) and CARS2.topk(·, 20).
            The lists are compared with array_equal, so the queries are drawn
            from seed 9000, 9001, ... until no two adjacent scores among a
            query's top 21 lie within 1e-5 of that query's Σ|terms| (float64,
            tests/cars2_ref.min_top_gap); the seed is recorded
  Neg1, Neg3            negatives [64, 1] and [64, 3]; row 5 of Neg3 repeats an id
  loss_ng{1,3}_lam{1e-3,0}   the reference's ``loss`` at λ = 0.001 and λ = 0
cars2_epoch_stream.json: per-batch sha256 of X / Y / F1 as the reference's own
Train (its __init__ builds feature_inject, its train() shuffles and samples)
feeds partial_fit over 2 epochs on synth_frappe, LoadData seeded 2016, the
loop seeded 47, batch 512, Result = 1.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cars2.py
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs tf1_numpy, imports the reference)
import numpy as np  # noqa: E402

import Newcode.CARS2 as RC2  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import cars2_ref as cr  # noqa: E402

NU, NI, MC = 30, 64, 11
ROWS, QUERIES, GAP = 64, 8, 1e-5
SEEDS = {16: 1601, 64: 6401}
STREAM_SEED = 47


def model(D, Wt, lam):
    m = RC2.CARS2(MC, NU, NI, D, 0.01, lam, "AdagradOptimizer")
    for k in cr.NAMES:
        assert m.weights[k].value.shape == Wt[k].shape, (k, m.weights[k].value.shape)
        m.weights[k].value = Wt[k]
    return m


def gen_model(D, out):
    p = f"d{D}_"
    Wt = cr.weights(SEEDS[D], NU + NI, MC, D)
    rng = np.random.default_rng(100 + D)
    X = np.stack([rng.integers(0, NU, ROWS), rng.integers(NU, NU + NI, ROWS),
                  rng.integers(0, MC, ROWS)], 1).astype(np.int32)
    m = model(D, Wt, 0.001)
    pf = m.sess.run(m.PositiveFeadback, feed_dict={m.Pos: X[:, :2], m.Fea: X[:, 2]})
    for seed in range(9000, 19000):
        r = np.random.default_rng(seed)
        q = np.stack([r.integers(0, NU, QUERIES), r.integers(0, MC, QUERIES)], 1).astype(np.int32)
        if cr.min_top_gap(q, Wt, NU, NI) > GAP:
            break
    else:
        raise SystemExit(f"D={D}: no gap-clean query set")
    pred = m.topk({"X": q[:, 0], "F1": q[:, 1]}, 20)
    Neg1 = rng.integers(NU, NU + NI, (ROWS, 1)).astype(np.int32)
    Neg3 = rng.integers(NU, NU + NI, (ROWS, 3)).astype(np.int32)
    Neg3[5, 2] = Neg3[5, 0]
    out.update({p + "seed": np.int64(SEEDS[D]), p + "X": X.astype(np.int16),
                p + "out": np.asarray(pf, np.float32)[:, 0], p + "q": q.astype(np.int16),
                p + "q_seed": np.int64(seed), p + "topk_idx": np.asarray(pred).astype(np.int16),
                p + "Neg1": Neg1.astype(np.int16), p + "Neg3": Neg3.astype(np.int16)})
    for lam, tag in ((0.001, "1e-3"), (0.0, "0")):
        ml = model(D, Wt, lam)
        for Neg, ng in ((Neg1, 1), (Neg3, 3)):
            loss = ml.sess.run(ml.loss, feed_dict={ml.Pos: X[:, :2], ml.Fea: X[:, 2], ml.Neg: Neg})
            out[f"{p}loss_ng{ng}_lam{tag}"] = np.float32(loss)
    print(f"D={D}: query seed {seed}, min top-21 gap / Σ|terms| =",
          cr.min_top_gap(q, Wt, NU, NI), "trilinear share >=",
          float(cr.exact_rows(X, Wt)[2].min()))


def gen_epoch_stream(epochs=2, batch=512):
    np.random.seed(2016)
    args = argparse.Namespace(path=HERE + "/", dataset="synth_frappe", epoch=epochs + 1,
                              batch_size=batch, hidden_factor=16, lamda=0.001, keep=1, lr=0.01,
                              optimizer="AdagradOptimizer", batch_norm=0, TopK=10, Result=1)
    t = RC2.Train(args)                  # the reference's own feature_inject
    t.model = mg._Recorder()
    np.random.seed(STREAM_SEED)
    t.train()
    res = {"cars2": t.model.batches, "epochs": epochs, "batch_size": batch, "seed": STREAM_SEED,
           "loaddata_seed": 2016, "features_M": int(t.features_M)}
    with open(os.path.join(HERE, "cars2_epoch_stream.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("cars2_epoch_stream", len(res["cars2"]), "batches, features_M", res["features_M"])


def main():
    out = {"n_user": np.int64(NU), "n_item": np.int64(NI), "Mc": np.int64(MC)}
    for D in (16, 64):
        gen_model(D, out)
    mg.save("cars2.npz", **out)
    gen_epoch_stream()


if __name__ == "__main__":
    main()
