#!/usr/bin/env python3
"""Golden vectors of the two-way HHFM model: the pair-product tensors from the
REFERENCE ITSELF, and the composed model restated.

Runs where make_golden.py runs (the reference tree present, never on the GPU
box).  It imports make_golden — the reference's unmodified OurModel7 over
tf1_numpy — and sets the module constants Pooling1C / 1T / 1F and Pooling2C /
2T / 2F (OurModel7.py:14-19) before constructing ``OUR``.

The reference's committed text builds the pair products and pools them
(mixdouble_features_context :113-122, mixdouble_features_time :130-139,
hybrid_feature2d :157-166) but comments out the three additions that would use
them (:124, :141, :168).  So hhfm_two_way.npz holds two kinds of data:

  reference tensors   per (layout, sextuple) ``stack_features``,
                      ``mixdouble_features_context``, ``mixdouble_features_time``
                      (layouts with time fields) and ``hybrid_feature2d`` from
                      sess.run on the first 64 committed rows X of
                      hhfm_{frappe,jiaju,resturant}.npz.  They pin the pair order
                      and what Pooling2* reduces.  To keep the file small the
                      reference runs at hidden_factor 2, on the first two
                      columns of the table.
  restated_* entries  the composed model cannot be run from the reference's
                      text, so ``restated_out`` (the 64 rows' scores) and
                      ``restated_topk_idx`` (top-20 of the queries A) are
                      tests/hhfm_two_way_ref.py's, on the whole table.
Every entry of a layout stacks the sextuples of ``sextuples`` along axis 0.

The table is the layout's committed E times 64 (exact in fp32: std about 0.64,
at which the pair terms carry a large part of h; at the committed std of 0.01
they would vanish beside the one-way terms).  The index lists are compared
with array_equal, so no two adjacent scores among a query's top 21 may lie
within 1e-5 of that query's Σ|terms| under any sextuple (checked in float64).
At this std the scores cancel heavily against Σ|terms| and the committed 24
queries always hold such a pair, so each layout gets 8 queries A of its own,
drawn from seed 9000, 9001, ... until the check passes; A and the seed are
recorded.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_two_way.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs tf1_numpy, imports the reference)
import make_golden_pooling as mgp  # noqa: E402
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import fm_oracle as orc  # noqa: E402
from tests import hhfm_two_way_ref as tw  # noqa: E402

RM7 = mg.RM7
MMM, EEE, SSS = ("max",) * 3, ("mean",) * 3, ("sum",) * 3
SEXTUPLES = [(MMM, MMM), (EEE, EEE), (SSS, SSS),
             (("max", "mean", "sum"), ("mean", "sum", "max"))]
SCALE = np.float32(64.0)
ROWS, KREF, QUERIES = 64, 2, 8
GAP = 1e-5


def key(six):
    return "_".join(six[0]) + "__" + "_".join(six[1])


def set_pooling(six):
    mgp.set_pooling(six[0])
    RM7.Pooling2C, RM7.Pooling2T, RM7.Pooling2F = (mgp.TF_POOL[m] for m in six[1])


def min_gap(A, E, nu, ni, ctx, tim, six):
    exact = tw.exact_catalog2(A, E, nu, ctx, tim, *six)
    worst = np.inf
    for b in range(len(A)):
        s, mag = exact(b, np.arange(ni))
        top = np.sort(s)[::-1][:21]
        worst = min(worst, float(np.min(top[:-1] - top[1:]) / mag.max()))
    return worst


def main():
    out = {"scale": SCALE, "rows": np.int64(ROWS), "kref": np.int64(KREF),
           "sextuples": np.array([key(s) for s in SEXTUPLES])}
    for tag, (nu, ni, cards, td) in mgp.LAYOUTS.items():
        g = np.load(os.path.join(HERE, f"hhfm_{tag}.npz"))
        E, X = g["E"] * SCALE, g["X"][:ROWS]
        fd = len(cards)
        ctx, tim = mgp.ranges(fd, td)
        for seed in range(9000, 19000):
            A = mg.rows(np.random.default_rng(seed), QUERIES, nu, ni, cards, td)
            if min(min_gap(A, E, nu, ni, ctx, tim, s) for s in SEXTUPLES) > GAP:
                break
        else:
            raise SystemExit(f"{tag}: no gap-clean query set")
        out[f"{tag}_A_seed"] = np.int64(seed)
        out[f"{tag}_A"] = A
        Eref = np.ascontiguousarray(E[:, :KREF])
        per = {}
        for six in SEXTUPLES:
            set_pooling(six)
            m = mgp.model(nu, ni, fd, td, Eref)
            f = mgp.feed(m, X, fd, td)
            nodes = {"stack_features": m.stack_features,
                     "mixdouble_features_context": m.mixdouble_features_context,
                     "hybrid_feature2d": m.hybrid_feature2d}
            if td:
                nodes["mixdouble_features_time"] = m.mixdouble_features_time
            for name, node in nodes.items():
                per.setdefault(name, []).append(
                    np.asarray(m.sess.run(node, feed_dict=f), np.float32))
            per.setdefault("restated_out", []).append(tw.score_rows2(X, E, ctx, tim, *six))
            sc = tw.catalog_scores2(A, E, nu, ni, ctx, tim, *six)
            per.setdefault("restated_topk_idx", []).append(orc.top_k(sc, 20)[1].astype(np.int16))
            print(tag, key(six), "min top-21 gap / Σ|terms| =",
                  min_gap(A, E, nu, ni, ctx, tim, six), "pair share >=",
                  float(tw.pair_share(X, E, ctx, tim, *six).min()))
        out.update({f"{tag}_{name}": np.stack(v) for name, v in per.items()})
    set_pooling((SSS, SSS))
    mg.save("hhfm_two_way.npz", **out)


if __name__ == "__main__":
    main()
