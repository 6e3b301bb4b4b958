#!/usr/bin/env python3
"""Golden vectors of HHFM with MAX / MEAN pooling, from the REFERENCE ITSELF.

Runs where make_golden.py runs (the reference tree present, never on the GPU
box).  It imports make_golden — the reference's unmodified OurModel7 over
tf1_numpy — and sets the module constants the reference selects its pooling
by (OurModel7.py:14-19: Pooling1C, Pooling1T, Pooling1F) to tf.reduce_max /
tf.reduce_mean before constructing ``OUR``, as its authors did for the MAX and
MEAN sections of their result log.

  hhfm_pool.npz         per (layout, triple): ``out`` of the committed rows X,
                        ``topk_idx`` of the queries A and each query's 21
                        largest scores — E, X and (unless a seed is recorded)
                        A are those of hhfm_{frappe,jiaju,resturant}.npz
  hhfm_pool_losses.npz  ``self.loss`` under the same triples on a frappe- and a
                        jiaju-layout batch built like make_golden.gen_losses'
                        HHFM case (NG = 10, a planted reduce_max tie)

The index lists are compared with array_equal, so the script checks in float64
(tests/hhfm_pool_ref.exact_catalog) that no two adjacent scores among a query's
top 21 lie within 1e-5 of that query's Σ|terms|; if some do under any triple it
draws the layout's A from another seed and records A and the seed.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pooling.py
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
from tests import hhfm_pool_ref as pr  # noqa: E402

RM7 = mg.RM7
TF_POOL = {"sum": tf.reduce_sum, "max": tf.reduce_max, "mean": tf.reduce_mean}
TRIPLES = [("max", "max", "max"), ("mean", "mean", "mean"), ("max", "max", "sum"),
           ("mean", "max", "sum")]
# tag: (n_user, n_item, context cardinalities, time columns) of make_golden.main
LAYOUTS = {"frappe": (957, 4082, (7, 2, 3), 0), "jiaju": (200, 600, (5, 4, 6, 3, 7), 3),
           "resturant": (200, 600, (5, 4, 6, 3, 7), 5)}
GAP = 1e-5


def key(triple):
    return "_".join(triple)


def set_pooling(triple):
    RM7.Pooling1C, RM7.Pooling1T, RM7.Pooling1F = (TF_POOL[m] for m in triple)


def model(nu, ni, fd, td, E):
    m = RM7.OUR(fd, td, E.shape[0], nu, ni, E.shape[1], 0.1, 0.01, "AdagradOptimizer", True,
                td > 0)
    m.weights["feature_embeddings"].value = E
    return m


def feed(m, X, fd, td, Neg=None):
    f = {m.Pos: X[:, :2], m.Fea: X[:, 2:2 + fd]}
    if td:
        f[m.Tim] = X[:, 2 + fd:]
    if Neg is not None:
        f[m.Neg] = Neg
    return f


def ranges(fd, td):
    return (2, 2 + fd), ((2 + fd, 2 + fd + td) if td else (0, 0))


def min_gap(A, E, nu, ni, ctx, tim, triple):
    """Least float64 gap between adjacent scores of a query's top 21, in units
    of that query's largest Σ|terms|."""
    exact = pr.exact_catalog(A, E, nu, ctx, tim, triple)
    worst = np.inf
    for b in range(len(A)):
        s, mag = exact(b, np.arange(ni))
        top = np.sort(s)[::-1][:21]
        worst = min(worst, float(np.min(top[:-1] - top[1:]) / mag.max()))
    return worst


def gen_scores():
    out = {}
    for tag, (nu, ni, cards, td) in LAYOUTS.items():
        g = np.load(os.path.join(HERE, f"hhfm_{tag}.npz"))
        E, X, A = g["E"], g["X"], g["A"]
        fd = len(cards)
        ctx, tim = ranges(fd, td)
        seed = -1
        while min(min_gap(A, E, nu, ni, ctx, tim, t) for t in TRIPLES) <= GAP:
            seed += 1
            A = mg.rows(np.random.default_rng(7000 + seed), len(A), nu, ni, cards, td)
        out[f"{tag}_A_seed"] = np.int64(-1 if seed < 0 else 7000 + seed)
        if seed >= 0:
            out[f"{tag}_A"] = A
        for t in TRIPLES:
            set_pooling(t)
            m = model(nu, ni, fd, td, E)
            o = m.sess.run(m.PositiveFeadback, feed_dict=feed(m, X, fd, td))
            mg.tf1_numpy.LAST_TOPK_INPUT.clear()
            pred = m.topk(A, 20)
            sc = mg.tf1_numpy.LAST_TOPK_INPUT[-1]
            out[f"{tag}_{key(t)}_out"] = o[:, 0]
            out[f"{tag}_{key(t)}_topk_idx"] = pred
            out[f"{tag}_{key(t)}_top21"] = -np.sort(-sc, axis=1)[:, :21]
            print(tag, key(t), "min top-21 gap / Σ|terms| =",
                  min_gap(A, E, nu, ni, ctx, tim, t))
    set_pooling(("sum", "sum", "sum"))
    mg.save("hhfm_pool.npz", **out)


def gen_losses():
    out = {}
    k = 16
    for tag, nu, ni, cards, td, seed in (("frappe", 40, 150, (7, 2, 3), 0, 712),
                                         ("jiaju", 40, 150, (5, 4, 6, 3, 7), 3, 713)):
        rng = np.random.default_rng(seed)
        fd = len(cards)
        M = mg.vocab(nu, ni, cards)
        E = rng.normal(0, 0.3, (M, k)).astype(np.float32)
        X = mg.rows(rng, 80, nu, ni, cards, td)
        Neg = rng.integers(nu, nu + ni, (80, 10)).astype(np.int32)
        Neg[3, 4] = Neg[3, 7]                                   # a tie in reduce_max
        Neg[5, :] = Neg[5, 0]                                   # every negative the maximum
        out.update({f"{tag}_E": E, f"{tag}_X": X, f"{tag}_Neg": Neg,
                    f"{tag}_feature_dimension": fd, f"{tag}_time_dimension": td})
        for t in TRIPLES:
            set_pooling(t)
            m = model(nu, ni, fd, td, E)
            loss = m.sess.run(m.loss, feed_dict=feed(m, X, fd, td, Neg))
            out[f"{tag}_{key(t)}_loss"] = np.float32(loss)
    set_pooling(("sum", "sum", "sum"))
    out.update(n_user=40, n_item=150, lamda=np.float32(0.01))
    mg.save("hhfm_pool_losses.npz", **out)
    print({kk: float(v) for kk, v in out.items() if kk.endswith("_loss")})


if __name__ == "__main__":
    gen_scores()
    gen_losses()
