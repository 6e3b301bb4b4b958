#!/usr/bin/env python3
"""Golden vectors of AFM with attention=0 from the REFERENCE ITSELF.

Runs where make_golden.py runs (the reference tree present, never on the GPU
box).  It imports make_golden — which installs tf1_numpy, the toolz chunker
and np.int — and then runs the reference's unmodified Newcode/AFM.py with
``attention=0``.

afm0.npz, for k = 16 and k = 64 (prefix k16_ / k64_):
  E, w, w0, P   tests/afm0_ref.weights(seed): E at std 0.3, w at std 0.1,
                w0 = 0.02 and P drawn N(1, 0.3) — not ones: at P ≡ 1 a kernel
                that drops P passes
  X, out        64 rows of 5 fields and the reference's ``out``
  Y, loss_lam100, loss_lam0   labels ±1 and the reference's ``loss`` at keep
                [1, 1] with lamda_attention 100 and 0: the two are asserted
                equal here (the model has no regulariser, AFM.py:148)
The model's variable names are asserted to be exactly feature_embeddings,
feature_bias, bias, prediction.  The reference's topk raises
KeyError('attention_W') on this model (asserted), so no ranking is stored:
the catalog score is the library's definition (include/hhfm.h).
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_afm0.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs tf1_numpy, imports the reference)
import numpy as np  # noqa: E402

import Newcode.AFM as RAFM  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import afm0_ref as ar  # noqa: E402

NU, NI, CTX, ROWS = 40, 150, (7, 2, 3), 64
SEEDS = {16: 1600, 64: 6400}


def model(M, k, Wt, lam):
    np.random.seed(303)
    m = RAFM.AFM(NU, NI, M, 0, [k, k], None, 0.1, lam, [1, 1], "AdagradOptimizer", 0.999, 5)
    assert sorted(m.weights) == ["bias", "feature_bias", "feature_embeddings", "prediction"], \
        sorted(m.weights)
    m.weights["feature_embeddings"].value = Wt["E"]
    m.weights["feature_bias"].value = Wt["w"][:, None]
    m.weights["bias"].value = np.float32(Wt["w0"])
    assert m.weights["prediction"].value.shape == (k, 1)
    m.weights["prediction"].value = Wt["P"][:, None]
    return m


def gen(k, out):
    p = f"k{k}_"
    M = mg.vocab(NU, NI, CTX)
    Wt = ar.weights(SEEDS[k], M, k)
    rng = np.random.default_rng(800 + k)
    X = mg.rows(rng, ROWS, NU, NI, CTX)
    Y = rng.choice([-1.0, 1.0], ROWS).astype(np.float32).reshape(-1, 1)
    losses = {}
    for lam in (100.0, 0.0):
        m = model(M, k, Wt, lam)
        feed = {m.train_features: X, m.train_labels: Y, m.dropout_keep: [1.0, 1.0],
                m.train_phase: True}
        o = m.sess.run(m.out, feed_dict=feed)
        losses[lam] = np.float32(m.sess.run(m.loss, feed_dict=feed))
    assert losses[100.0] == losses[0.0], losses           # no regulariser
    try:
        m.topk(X[:4], 5)
    except KeyError as e:
        assert "attention_W" in str(e), e
    else:
        raise SystemExit("the reference's topk ran with attention=0: store its ranking")
    o64, S = ar.out64(X, Wt["E"], Wt["w"], Wt["w0"], Wt["P"])
    print(f"k={k}: |out − float64| / Σ|terms| <=", float(np.abs(o[:, 0] - o64).max() / S.min()),
          "loss", losses[0.0], "float64", ar.loss64(X, Y, Wt["E"], Wt["w"], Wt["w0"], Wt["P"]))
    out.update({p + "E": Wt["E"], p + "w": Wt["w"], p + "w0": np.float32(Wt["w0"]),
                p + "P": Wt["P"], p + "X": X.astype(np.int16),
                p + "out": np.asarray(o, np.float32)[:, 0], p + "Y": Y[:, 0],
                p + "loss_lam100": losses[100.0], p + "loss_lam0": losses[0.0]})


def main():
    out = {"n_user": np.int64(NU), "n_item": np.int64(NI)}
    for k in (16, 64):
        gen(k, out)
    mg.save("afm0.npz", **out)


if __name__ == "__main__":
    main()
