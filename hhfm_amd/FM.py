"""FM — drop-in for Newcode/FM.py (model class, Train harness, FM_main).

Scoring runs on the gfx950 kernels:
  * ``score_rows`` / ``sess.run(model.out)`` -> hhfm_fm_score_rows (FM.py:99-120);
    with ``batch_norm=1`` hhfm_fm_score_rows_scaled on the moving statistics
  * ``topk(A, tp)`` -> hhfm_catalog_topk, HHFM_MODE_FM (FM.py:172-198); the
    reference's catalog score does not pass through the batch-norm layer
    (FM.py:181 is commented out)

``batch_norm=1`` (FM.py:111-112, :160-166; include/hhfm.h "FM batch norm") adds
the weights ``bn_gamma``, ``bn_beta``, ``bn_moving_mean``, ``bn_moving_variance``.
Two things the reference's graph does are deliberately not reproduced: it
builds both branches outside ``tf.cond``, so every ``sess.run(out)`` would also
move the moving averages with the fed batch — here scoring never writes a
weight; and batch statistics exist only inside ``partial_fit`` —
``train_phase: True`` through ``sess.run(model.out, …)`` raises.
"""
from __future__ import annotations

import argparse

import numpy as np
import torch

from . import NewLoadData as DATA
from . import harness, ops
from ._model import Fetch, Placeholder, ScoringModel

method = "FM"

# tf.contrib.layers.batch_norm(decay=0.9) and its default epsilon; the update
# factor is float(1.0 - decay), the complement formed in double as TF forms it
BN_DECAY, BN_EPS = 0.9, 0.001


def parse_args(dataname, factor, TopK, argv=None):
    """Same flags and defaults as the reference (FM.py:24-57)."""
    p = argparse.ArgumentParser(description="Run FM.")
    p.add_argument("--process", nargs="?", default="train")
    p.add_argument("--mla", type=int, default=0)
    p.add_argument("--path", nargs="?", default="../data/positive/")
    p.add_argument("--dataset", nargs="?", default=dataname)
    p.add_argument("--epoch", type=int, default=60)
    p.add_argument("--batch_size", type=int, default=5000)
    p.add_argument("--hidden_factor", type=int, default=factor)
    p.add_argument("--lamda", type=float, default=0.1)
    p.add_argument("--keep", type=float, default=1)
    p.add_argument("--lr", type=float, default=0.1)
    p.add_argument("--optimizer", nargs="?", default="AdagradOptimizer")
    p.add_argument("--verbose", type=int, default=10)
    p.add_argument("--batch_norm", type=int, default=0)
    p.add_argument("--TopK", type=int, default=TopK)
    p.add_argument("--Result", type=int, default=0)
    p.add_argument("--result_file", default="../result.txt")
    p.add_argument("--deterministic", type=int, default=0,
                   help="1: bit-reproducible training steps (row-ordered sums)")
    p.add_argument("--filter_seen", type=int, default=0, choices=(0, 1),
                   help="1: HR / NDCG / PRE over top-K lists without each key's train positives")
    return p.parse_args(argv)


class FM(ScoringModel):
    def __init__(self, valid_dimension, features_M, n_user, n_item, hidden_factor,
                 learning_rate, lamda_bilinear, keep, optimizer_type, batch_norm,
                 verbose, random_seed=2016, device=None, table_dtype=torch.float32,
                 deterministic=False):
        self.deterministic = bool(deterministic)
        self.valid_dimension = valid_dimension
        self.n_user = n_user
        self.n_item = n_item
        self.learning_rate = learning_rate
        self.hidden_factor = hidden_factor
        self.features_M = features_M
        self.lamda_bilinear = lamda_bilinear
        self.keep = keep
        self.random_seed = random_seed
        self.optimizer_type = optimizer_type
        self.batch_norm = batch_norm
        self.verbose = verbose
        self.train_rmse, self.valid_rmse, self.test_rmse = [], [], []
        self.bn_eps = BN_EPS
        self.bn_update = float(1.0 - BN_DECAY)
        if batch_norm and self.deterministic:
            raise NotImplementedError("deterministic=True has no batch_norm=1 step "
                                      "(hhfm_fm_train_step_bn adds its batch sums with atomics)")
        self._setup_device(device, table_dtype)
        self._init_graph()

    def _init_graph(self):
        # placeholders / fetches a reference caller may use (FM.py:89-120)
        self.train_features = Placeholder("train_features_fm")
        self.train_labels = Placeholder("train_labels_fm")
        self.dropout_keep = Placeholder("dropout_keep_fm")
        self.train_phase = Placeholder("train_phase_fm")
        self.out = Fetch("out")
        self.weights = self._initialize_weights()

    def _initialize_weights(self):
        """FM.py:150-158: E ~ N(0, 0.01), feature_bias = 0, bias = 0."""
        W = {
            "feature_embeddings": self._normal((self.features_M, self.hidden_factor), 0.01,
                                               self.random_seed),
            "feature_bias": torch.zeros(self.features_M, 1, device=self.device),
            "bias": torch.zeros((), device=self.device),
        }
        if self.batch_norm:   # contrib batch_norm's variables (beta, gamma, moving_*)
            k = self.hidden_factor
            W["bn_beta"] = torch.zeros(k, device=self.device)
            W["bn_gamma"] = torch.ones(k, device=self.device)
            W["bn_moving_mean"] = torch.zeros(k, device=self.device)
            W["bn_moving_variance"] = torch.ones(k, device=self.device)
        return W

    # -- scoring ------------------------------------------------------------------
    def score_rows(self, X) -> np.ndarray:
        """FM.out for full rows [user, item, ctx...] -> float32 [B, 1]."""
        idx = self._idx(X)
        W = self.weights
        w = W["feature_bias"].reshape(-1)
        if not self.batch_norm:
            return self._np_out(ops.fm_score_rows(idx, self.table, w, float(W["bias"])))
        # the layer on the moving statistics: a = γ/√(mv + eps) weights the
        # columns, Σ(β − mm·a) joins the bias
        a = (W["bn_gamma"] / torch.sqrt(W["bn_moving_variance"] + self.bn_eps)).contiguous()
        w0 = W["bias"] + (W["bn_beta"] - W["bn_moving_mean"] * a).sum()
        return self._np_out(ops.fm_score_rows(idx, self.table, w, float(w0), scale=a))

    def catalog_topk(self, q, begin, count, K, exclude=None):
        """Top-K of items [begin, begin+count) by (u+f)·(i+f) + w_i (FM.py:172-185)
        -> (scores, global item offsets) device tensors [B, K].  ``exclude``: an
        ops.ExclusionLists, or a positive_feedback-style dict key tuple -> set of
        table row ids (keys from ``q`` as harness.row_keys takes them): the top K
        of each query's other items."""
        ncols = q.shape[1]
        extra = {} if exclude is None else {"exclude": self._exclusion(q, exclude)}
        return ops.catalog_topk(q, self.table, ops.MODE_FM, int(K), self.n_user + begin, count,
                                begin, self.weights["feature_bias"].reshape(-1), 0,
                                (2, ncols) if ncols > 2 else (0, 0), (0, 0), **extra)

    def topk(self, A, tp, exclude=None):
        """Top-``tp`` item offsets in [0, n_item) by (u+f)·(i+f) + w_i; ``exclude``
        as in :meth:`catalog_topk`."""
        _, ids = self.catalog_topk(self._idx(A), 0, self.n_item, tp, exclude=exclude)
        return ids.cpu().numpy()

    def _run_fetch(self, fetch, feed):
        if fetch is self.out:
            if self.batch_norm and bool(np.any(feed.get(self.train_phase, False))):
                raise NotImplementedError("batch_norm=1: batch statistics exist only inside "
                                          "partial_fit; feed train_phase False to score")
            return self.score_rows(feed[self.train_features])
        return super()._run_fetch(fetch, feed)

    def partial_fit(self, data):
        from .training import fm_partial_fit
        return fm_partial_fit(self, data)


class Train(harness.Train):
    method = "FM"

    def __init__(self, args, data=None, model=None):
        data = data if data is not None else DATA.LoadData(args.path, args.dataset)
        super().__init__(args, data=data)
        self.valid_dimension = self.data.Train_data.shape[1] - 1
        if args.verbose > 0:
            print("FM: dataset=%s, factors=%d, #epoch=%d, batch=%d, lr=%.4f, lambda=%.1e, "
                  "keep=%.2f, optimizer=%s, batch_norm=%d"
                  % (args.dataset, args.hidden_factor, args.epoch, args.batch_size, args.lr,
                     args.lamda, args.keep, args.optimizer, args.batch_norm))
        self.model = model if model is not None else FM(
            self.valid_dimension, self.data.features_M, self.n_user, self.n_item,
            args.hidden_factor, args.lr, args.lamda, args.keep, args.optimizer,
            args.batch_norm, args.verbose,
            deterministic=bool(getattr(args, "deterministic", 0)))

    def train(self):
        from .training import run_training
        return run_training(self, negatives=2, neg_label=0)


def FM_main(dataname, factor, Topk, argv=None):
    args = parse_args(dataname, factor, Topk, argv)
    session = Train(args)
    session.train()
    return session
