"""HHFM (OurModel7) — drop-in for Newcode/OurModel7.py (OUR, Train, M7_main).

In the reference's committed text the pairwise-product branches are dead code
(the three additions that would use their Pooling2* results are commented out,
OurModel7.py:124 / :141 / :168), so with the committed sum pooling (:14-19)
  h = E[user] + Σ E[ctx] (+ Σ E[time]),   score = h · E[item]   (no bias).
The three live pools follow the module attributes ``Pooling1C`` (context rows),
``Pooling1T`` (time rows) and ``Pooling1F`` (the stack {user, context pool,
time pool}), read when an ``OUR`` is constructed: "sum", "max" or "mean" (or
``ops.POOL_*``), as the reference sets tf.reduce_sum / reduce_max /
reduce_mean there; ``OUR(..., pooling=(ctx, time, final))`` and ``--pooling``
override them.
``OUR(..., two_way=True)`` (``--two_way 1``) puts the three commented-out
additions back (include/hhfm.h "Two-way pooling"): each pool gains the pool of
its rows' pair products, the stack the pool of its member products, reduced by
``Pooling2C`` / ``Pooling2T`` / ``Pooling2F`` (read at construction like
``Pooling1*``; ``pooling2=(ctx, time, final)`` and ``--pooling2`` override
them, and ``--pooling2`` implies ``--two_way 1``).  All-sum ``pooling2`` is
still the two-way model.  It needs at least two context columns and, with time
fields, two time columns (ValueError otherwise), and has no deterministic step
(NotImplementedError).  With ``two_way=False`` ``Pooling2*`` are accepted and
ignored.
Scoring runs on the gfx950 kernels:
  * ``score_rows`` / ``sess.run(model.PositiveFeadback)`` -> hhfm_hybrid_score_rows
    (OurModel7.py:105-171)
  * ``topk(A, tp)`` -> hhfm_catalog_topk, HHFM_MODE_HHFM (OurModel7.py:229-307)
"""
from __future__ import annotations

import argparse

import numpy as np
import torch

from . import NewLoadData as DATA
from . import harness, ops
from ._model import Fetch, Placeholder, ScoringModel, rows_from

method = "M7"

# OurModel7.py:14-19.  Pooling2* reduce the pair products, which only the two-way
# model (OUR(two_way=True)) uses.
Pooling1C = "sum"
Pooling2C = "sum"
Pooling1T = "sum"
Pooling2T = "sum"
Pooling1F = "sum"
Pooling2F = "sum"


def parse_pooling(text, flag="--pooling"):
    """``--pooling`` / ``--pooling2``: "max" / "mean" / "sum" (all three pools)
    or "ctx,time,final" -> a (ctx, time, final) triple of mode names."""
    parts = [t.strip() for t in str(text).split(",")]
    if len(parts) == 1:
        parts = parts * 3
    if len(parts) != 3:
        raise ValueError(f"{flag} takes one mode or ctx,time,final, got {text!r}")
    for t in parts:
        ops.pool_mode(t)
    return tuple(parts)


def parse_args(dataname, factor, Topk, argv=None):
    """Same flags and defaults as the reference (OurModel7.py:23-49)."""
    p = argparse.ArgumentParser(description="Run .")
    p.add_argument("--path", nargs="?", default="../data/positive/")
    p.add_argument("--dataset", nargs="?", default=dataname)
    p.add_argument("--epoch", type=int, default=60)
    p.add_argument("--batch_size", type=int, default=5000)
    p.add_argument("--hidden_factor", type=int, default=factor)
    p.add_argument("--lamda", type=float, default=0.01)
    p.add_argument("--keep", type=float, default=1)
    p.add_argument("--lr", type=float, default=0.1)
    p.add_argument("--optimizer", nargs="?", default="AdagradOptimizer")
    p.add_argument("--batch_norm", type=int, default=0)
    p.add_argument("--TopK", type=int, default=Topk)
    p.add_argument("--Result", type=int, default=0)
    p.add_argument("--result_file", default="../result.txt")
    p.add_argument("--deterministic", type=int, default=0,
                   help="1: bit-reproducible training steps (row-ordered sums)")
    p.add_argument("--filter_seen", type=int, default=0, choices=(0, 1),
                   help="1: HR / NDCG / PRE over top-K lists without each key's train positives")
    p.add_argument("--pooling", default=None,
                   help="max | mean | sum, or ctx,time,final (default: the module's "
                        "Pooling1C / Pooling1T / Pooling1F)")
    p.add_argument("--two_way", type=int, default=0, choices=(0, 1),
                   help="1: the two-way model (pair products pooled by Pooling2*)")
    p.add_argument("--pooling2", default=None,
                   help="max | mean | sum, or ctx,time,final for the pair-product pools "
                        "(default: the module's Pooling2C / Pooling2T / Pooling2F); "
                        "implies --two_way 1")
    return p.parse_args(argv)


class OUR(ScoringModel):
    def __init__(self, feature_dimension, time_dimension, features_M, n_user, n_item,
                 hidden_factor, learning_rate, lamda_bilinear, optimizer_type, context, time,
                 random_seed=2016, device=None, table_dtype=torch.float32,
                 deterministic=False, pooling=None, two_way=False, pooling2=None):
        self.deterministic = bool(deterministic)
        self.two_way = bool(two_way)
        # None: the one-way entry points, exactly as before
        self.pooling2 = None
        if self.two_way:
            if pooling2 is None:
                pooling2 = (Pooling2C, Pooling2T, Pooling2F)
            elif isinstance(pooling2, str):
                pooling2 = parse_pooling(pooling2, "pooling2")
            ops.pooling_word(pooling2)
            self.pooling2 = tuple(pooling2)
            if context and feature_dimension < 2 or time and time_dimension < 2:
                raise ValueError("two_way=True needs at least two context columns and, with "
                                 "time fields, at least two time columns")
        if pooling is None:
            pooling = (Pooling1C, Pooling1T, Pooling1F)
        elif isinstance(pooling, str):
            pooling = parse_pooling(pooling)
        # None: the sum-pooling entry points, exactly as before
        self.pooling = tuple(pooling) if ops.pooling_word(pooling) != 0 else None
        self.feature_dimension = feature_dimension
        self.time_dimension = time_dimension
        self.n_user = n_user
        self.n_item = n_item
        self.learning_rate = learning_rate
        self.hidden_factor = hidden_factor
        self.features_M = features_M
        self.lamda_bilinear = lamda_bilinear
        self.optimizer_type = optimizer_type
        self.context = context
        self.time = time
        self.random_seed = random_seed
        if not context and time:
            # the reference never sets self.num on this branch (OurModel7.py:96-99)
            # and its graph construction fails at :159
            raise AttributeError("'OUR' object has no attribute 'num'")
        if not context and not time:
            raise UnboundLocalError("OUR needs context and/or time fields")
        self.num = 3 if (context and time) else 2
        self._setup_device(device, table_dtype)
        self._init_graph()

    def _init_graph(self):
        self.Pos = Placeholder("Pos")
        self.Fea = Placeholder("Fea") if self.context else None
        self.Tim = Placeholder("Tim") if self.time else None
        self.Neg = Placeholder("Neg")
        self.PositiveFeadback = Fetch("PositiveFeadback")
        self.weights = self._initialize_weights()

    def _initialize_weights(self):
        """OurModel7.py:207-216 (feature_bias/wgt are unused by the score)."""
        return {
            "feature_embeddings": self._normal((self.features_M, self.hidden_factor), 0.01,
                                               self.random_seed),
            "feature_bias": torch.zeros(self.features_M, 1, device=self.device),
        }

    def _ranges(self, ncols):
        """Column split of a full row (OurModel7.py:236-242, 374-385)."""
        td = self.time_dimension if self.time else 0
        ctx = (2, ncols - td) if self.context else (0, 0)
        tim = (ncols - td, ncols) if self.time else (0, 0)
        if ctx[1] <= ctx[0]:
            ctx = (0, 0)
        return ctx, tim

    def score_rows(self, X) -> np.ndarray:
        """PositiveFeadback for full rows [user, item, ctx..., time...] -> [B,1]."""
        idx = self._idx(X)
        ctx, tim = self._ranges(idx.shape[1])
        out = ops.hybrid_score_rows(idx, self.table, 0, 1, ctx, tim, pooling=self.pooling,
                                    pooling2=self.pooling2)
        return self._np_out(out)

    def catalog_topk(self, q, begin, count, K, exclude=None):
        """Top-K of items [begin, begin+count) by h·item (OurModel7.py:229-295)
        -> (scores, global item offsets) device tensors [B, K].  ``exclude``: an
        ops.ExclusionLists, or a positive_feedback-style dict key tuple -> set of
        table row ids (keys from ``q`` as harness.row_keys takes them): the top K
        of each query's other items; the two-way model has no such form."""
        extra = {}
        if exclude is not None:
            if self.two_way:
                raise NotImplementedError("OUR(two_way=True) has no catalog top-K with "
                                          "exclusion lists")
            extra["exclude"] = self._exclusion(q, exclude)
        ctx, tim = self._ranges(q.shape[1])
        return ops.catalog_topk(q, self.table, ops.MODE_HHFM, int(K), self.n_user + begin,
                                count, begin, None, 0, ctx, tim, pooling=self.pooling,
                                pooling2=self.pooling2, **extra)

    def topk(self, A, tp, exclude=None):
        if exclude is not None and self.two_way:   # before anything runs
            raise NotImplementedError("OUR(two_way=True) has no catalog top-K with "
                                      "exclusion lists")
        _, ids = self.catalog_topk(self._idx(A), 0, self.n_item, tp, exclude=exclude)
        return ids.cpu().numpy()

    def _run_fetch(self, fetch, feed):
        if fetch is self.PositiveFeadback:
            return self.score_rows(rows_from(feed, self.Pos, self.Fea, self.Tim))
        return super()._run_fetch(fetch, feed)

    def partial_fit(self, data):
        from .training import hhfm_partial_fit
        return hhfm_partial_fit(self, data)


class Train(harness.Train):
    method = "M7"
    auc_first_chunk_only = True      # OurModel7.py:461 (returns inside the loop)
    auc_label_filter = False         # OurModel7.py:431

    def __init__(self, args, data=None, model=None):
        data = data if data is not None else DATA.LoadData(args.path, args.dataset)
        super().__init__(args, data=data)
        self.features_M = self.data.features_M
        self.valid_dimension = self.data.Train_data.shape[1] - 1
        print("OurModel: dataset=%s, factors=%d, #epoch=%d, batch=%d, lr=%.4f, lambda=%.1e, "
              "keep=%.2f, optimizer=%s, batch_norm=%d"
              % (args.dataset, args.hidden_factor, args.epoch, args.batch_size, args.lr,
                 args.lamda, args.keep, args.optimizer, args.batch_norm))
        # dataset switch, OurModel7.py:326-346
        self.context, self.time, self.time_dimension = True, False, 0
        if args.dataset == "resturant":
            self.time, self.time_dimension = True, 5
        elif args.dataset == "jiaju":
            self.time, self.time_dimension = True, 3
        self.feature_dimension = self.valid_dimension - 2 - self.time_dimension
        self.model = model if model is not None else OUR(
            self.feature_dimension, self.time_dimension, self.features_M, self.n_user,
            self.n_item, args.hidden_factor, args.lr, args.lamda, args.optimizer,
            self.context, self.time, deterministic=bool(getattr(args, "deterministic", 0)),
            pooling=getattr(args, "pooling", None),
            two_way=bool(getattr(args, "two_way", 0)) or getattr(args, "pooling2", None) is not None,
            pooling2=getattr(args, "pooling2", None))

    def train(self):
        from .training import run_training_hhfm
        return run_training_hhfm(self)


def M7_main(dataname, factor, Topk, argv=None):
    args = parse_args(dataname, factor, Topk, argv)
    session = Train(args)
    session.train()
    return session
