#!/usr/bin/env python3
"""Golden vectors of DeepFM's FM-only, deep-only and logloss heads, from the
REFERENCE ITSELF.

Runs where make_golden.py runs (the reference tree present, never on the GPU
box).  It imports make_golden — the reference's unmodified DFM.py over
tf1_numpy — and installs on the stand-in's ``tf.losses`` the one node the
committed tf1_numpy.py leaves a no-op: TF-1.x ``log_loss`` at its defaults,

    losses = −y·log(p + ε) − (1 − y)·log(1 − p + ε),  ε = 1e-7   (float32)
    loss   = Σ losses / B        (Reduction.SUM_BY_NONZERO_WEIGHTS, weights 1)

Then ``DeepFM(use_fm, use_deep, loss_type)`` is constructed for the six heads
{FM, DEEP, both} × {mse, logloss}; with use_fm = use_deep = True, "mse" and
make_golden.gen_dfm's seeds the script first reproduces dfm.npz (a cross-check
of this route; nothing is stored for it).

  dfm_heads.npz   E, w, the layers (np.random seeded alike for every head, so
                  they are one set), and per head: concat_projection,
                  concat_bias, ``out`` of the 128 rows X, the queries A,
                  ``topk_idx`` = model.topk(A, 20), the score rows handed to
                  top_k, and ``self.loss`` (l2_reg = 0.05) on a 64-row batch
                  with labels {1, 0} and with labels {1, −1}

The index lists are compared with array_equal, so for every head the script
checks in float64 (tests/dfm_heads_ref) that adjacent values among each query's
21 largest are further apart than twice that head's comparison tolerance — z:
1e-5·S, S = Σ_j |concat_j·Wp_j| + |bp|; under the sigmoid also p:
0.25·1e-5·S + 4·2^-24 — and draws that head's queries from another seed until
they are; the seed is recorded.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dfm_heads.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs tf1_numpy, imports the reference)
import numpy as np  # noqa: E402
import tensorflow as tf  # noqa: E402  (tf1_numpy)

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import dfm_heads_ref as hr  # noqa: E402

RDFM = mg.RDFM
F32 = np.float32
NU, NI, CTX, K, LAYERS = 50, 300, (7, 2, 3), 16, [150, 200, 150]
NQ, TOP = 4, 20
L2 = 0.05


def _log_loss(labels, predictions):
    def fn(y, p):
        y, p = np.asarray(y, F32), np.asarray(p, F32)
        eps = F32(1e-7)
        losses = -y * np.log(p + eps) - (F32(1) - y) * np.log(F32(1) - p + eps)
        return F32(losses.sum(dtype=F32) / F32(losses.size))
    return tf.Node(fn, [labels, predictions])


tf.losses.log_loss = _log_loss


def build(use_fm, use_deep, loss_type, seed, l2, E, w):
    np.random.seed(seed)   # DeepFM draws layer weights from np.random (DFM.py:185-208)
    m = RDFM.DeepFM(NU, NI, E.shape[0], 5, K, LAYERS, tf.nn.relu, 0.01, 0, l2,
                    use_fm=use_fm, use_deep=use_deep, loss_type=loss_type)
    m.weights["feature_embeddings"].value = E
    m.weights["feature_bias"].value = w
    return m


def cross_check():
    """both / mse on gen_dfm's seeds is dfm.npz."""
    d = np.load(os.path.join(HERE, "dfm.npz"))
    rng = np.random.default_rng(404)
    M = mg.vocab(NU, NI, CTX)
    np.random.seed(404)
    m = RDFM.DeepFM(NU, NI, M, 5, K, LAYERS, tf.nn.relu, 0.01, 0, 0.01, use_fm=True,
                    use_deep=True, loss_type="mse")
    E = rng.normal(0, 0.01, (M, K)).astype(F32)
    w = rng.uniform(0, 1, (M, 1)).astype(F32)
    m.weights["feature_embeddings"].value = E
    m.weights["feature_bias"].value = w
    X = mg.rows(rng, 128, NU, NI, CTX)
    out = m.sess.run(m.out, feed_dict={m.feat_index: X, m.label: np.ones((128, 1))})
    A = mg.rows(rng, 8, NU, NI, CTX)
    assert np.array_equal(X, d["X"]) and np.array_equal(out[:, 0], d["out"])
    assert np.array_equal(m.topk(A, 20), d["topk_idx"])
    print("cross-check: both / mse reproduces dfm.npz")


def gap_ok(A, head, E, w, layers, biases, Wp, bp):
    """Adjacent values of each query's 21 largest, float64: the ranking key of
    this code (z) and of the reference (p under the sigmoid) both further
    apart than twice their tolerance.  -> ok, the least gap / (2·tol)."""
    rows = hr.catalog_rows(A, NU, NI)
    out, z, S = hr.forward(rows, E, w, layers, biases, Wp, bp, head, dt=np.float64)
    worst = np.inf
    for vals, tol in ((z, 1e-5 * S),) + (((out, 0.25e-5 * S + 4 * 2.0 ** -24),)
                                         if head & hr.HEAD_SIGMOID else ()):
        v = vals.reshape(len(A), NI)
        t = tol.reshape(len(A), NI).max(1)
        for b in range(len(A)):
            top = np.sort(v[b])[::-1][:TOP + 1]
            worst = min(worst, float(np.min(top[:-1] - top[1:]) / (2 * t[b])))
    return worst > 1.0, worst


def main():
    cross_check()
    rng = np.random.default_rng(2404)
    M = mg.vocab(NU, NI, CTX)
    E = rng.normal(0, 0.3, (M, K)).astype(F32)
    w = rng.uniform(0, 1, (M, 1)).astype(F32)
    X = mg.rows(rng, 128, NU, NI, CTX)
    Xl = mg.rows(rng, 64, NU, NI, CTX)
    Y10 = np.concatenate([np.ones(32), np.zeros(32)]).reshape(-1, 1).astype(F32)
    Y1m = np.concatenate([np.ones(32), -np.ones(32)]).reshape(-1, 1).astype(F32)
    out = dict(E=E, w=w[:, 0], X=X, X_loss=Xl, Y_10=Y10[:, 0], Y_1m=Y1m[:, 0],
               n_user=NU, n_item=NI, l2=F32(L2), layer_dims=np.array(LAYERS))
    for name, (use_fm, use_deep, loss_type) in hr.HEADS.items():
        head = hr.head_word(use_fm, use_deep, loss_type)
        m = build(use_fm, use_deep, loss_type, 2405, L2, E, w)
        W = m.weights
        layers = [W[f"layer_{i}"].value for i in range(3)]
        biases = [W[f"bias_{i}"].value for i in range(3)]
        for i in range(3):   # one set of layers for every head
            assert np.array_equal(out.setdefault(f"layer_{i}", layers[i]), layers[i])
            assert np.array_equal(out.setdefault(f"bias_{i}", biases[i]), biases[i])
        Wp, bp = W["concat_projection"].value, F32(W["concat_bias"].value)
        assert Wp.shape[0] == hr.wp_size(head, 5, K, LAYERS)
        o = m.sess.run(m.out, feed_dict={m.feat_index: X, m.label: np.ones((128, 1))})
        seed = 8000
        while True:
            A = mg.rows(np.random.default_rng(seed), NQ, NU, NI, CTX)
            ok, worst = gap_ok(A, head, E, w[:, 0], layers, biases, Wp, bp)
            if ok:
                break
            seed += 1
        mg.tf1_numpy.LAST_TOPK_INPUT.clear()
        pred = m.topk(A, TOP)
        out.update({f"{name}_concat_projection": Wp, f"{name}_concat_bias": bp,
                    f"{name}_out": o[:, 0], f"{name}_A": A, f"{name}_A_seed": np.int64(seed),
                    f"{name}_topk_idx": pred,
                    f"{name}_topk_scores": mg.tf1_numpy.LAST_TOPK_INPUT[-1]})
        for tag, Y in (("10", Y10), ("1m", Y1m)):
            loss = m.sess.run(m.loss, feed_dict={m.feat_index: Xl, m.label: Y})
            out[f"{name}_loss_{tag}"] = F32(loss)
        print(name, "A seed", seed, "least top-21 gap / (2·tol) =", worst,
              "losses", float(out[f"{name}_loss_10"]), float(out[f"{name}_loss_1m"]))
    mg.save("dfm_heads.npz", **out)


if __name__ == "__main__":
    main()
