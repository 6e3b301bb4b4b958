"""CARS2 — drop-in for Newcode/CARS2.py (CARS2, Train, CARS2_main): the
context-aware baseline the reference's driver runs beside FM, HHFM, AFM and
DeepFM (main.py:63).

Variables (CARS2.py:150-164): ``UI`` [n_user+n_item, D], ``Context``
[features_M, Dc], ``W`` [D, Dp, Dc], ``Z`` [D, Dq, Dc], ``A`` [Dp], ``B`` [Dq]
with D = hidden_factor, Dc = int(D/2.5), Dp = int(D/5), Dq = int(D/2.5)
(:53-56); ``features_M`` is the number of distinct context tuples and a row is
(user id, item id, context id).  With u = UI[user], i = UI[item],
c = Context[m] (:85-105)

    score = u·i + Σ_p (Σ_c (Σ_d u_d W[d,p,c]) c_c) A_p + Σ_q (Σ_c (Σ_d i_d Z[d,q,c]) c_c) B_q

which the device evaluates folded per context id (include/hhfm.h "CARS2"):
GA[m] = (W·A)·c_m and GB[m] = (Z·B)·c_m are prepared once per weight set and
cached; ``set_weights`` and ``partial_fit`` invalidate them.
  * ``score_rows`` / ``sess.run(model.PositiveFeadback)`` -> hhfm_cars2_score_rows
  * ``topk(feed, tp)`` / ``catalog_topk``                 -> hhfm_cars2_catalog_topk (:171-187)
  * ``partial_fit``                                       -> hhfm_cars2_train_step (:87, :103-136)
There is no deterministic step (NotImplementedError) and training runs on fp32
tables.
"""
from __future__ import annotations

import argparse

import numpy as np
import torch

from . import NewLoadData as DATA
from . import harness, ops
from ._model import Fetch, Placeholder, ScoringModel

method = "CARS2"


def parse_args(dataname, factor, Topk, argv=None):
    """Same flags and defaults as the reference (CARS2.py:18-44); ``--keep`` and
    ``--batch_norm`` are parsed and ignored, as there."""
    p = argparse.ArgumentParser(description="Run .")
    p.add_argument("--path", nargs="?", default="../data/positive/")
    p.add_argument("--dataset", nargs="?", default=dataname)
    p.add_argument("--epoch", type=int, default=60)
    p.add_argument("--batch_size", type=int, default=5000)
    p.add_argument("--hidden_factor", type=int, default=factor)
    p.add_argument("--lamda", type=float, default=0.001)
    p.add_argument("--keep", type=float, default=1)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--optimizer", nargs="?", default="AdagradOptimizer")
    p.add_argument("--batch_norm", type=int, default=0)
    p.add_argument("--TopK", type=int, default=Topk)
    p.add_argument("--Result", type=int, default=0)
    p.add_argument("--result_file", default="../result.txt")
    p.add_argument("--deterministic", type=int, default=0,
                   help="1: bit-reproducible training steps (not built for CARS2)")
    p.add_argument("--filter_seen", type=int, default=0, choices=(0, 1),
                   help="1: HR / NDCG / PRE over top-K lists without each key's train positives")
    return p.parse_args(argv)


class CARS2(ScoringModel):
    NAMES = ("UI", "Context", "W", "Z", "A", "B")

    def __init__(self, features_M, n_user, n_item, hidden_factor, learning_rate, lamda_bilinear,
                 optimizer_type, random_seed=2016, device=None, table_dtype=torch.float32,
                 deterministic=False):
        self.deterministic = bool(deterministic)
        self.n_user = n_user
        self.n_item = n_item
        self.learning_rate = learning_rate
        self.D = int(hidden_factor)
        self.D_c, self.D_p, self.D_q = ops.cars2_dims(self.D)      # CARS2.py:54-56
        if min(self.D_c, self.D_p, self.D_q) < 1:
            raise ValueError(f"hidden_factor {hidden_factor} leaves an empty factor "
                             f"(D_c, D_p, D_q = {self.D_c}, {self.D_p}, {self.D_q})")
        self.hidden_factor = self.D
        self.features_M = features_M
        self.lamda_bilinear = lamda_bilinear
        self.optimizer_type = optimizer_type
        self.random_seed = random_seed
        self._setup_device(device, table_dtype)
        self._init_graph()

    def _init_graph(self):
        self.Pos = Placeholder("Pos")
        self.Fea = Placeholder("Fea")
        self.Neg = Placeholder("Neg")
        self.PositiveFeadback = Fetch("PositiveFeadback")
        self.weights = self._initialize_weights()
        self._prep = None

    def _initialize_weights(self):
        """CARS2.py:150-164: N(0, 0.01) but A = B = 0."""
        s = self.random_seed
        D, Dc, Dp, Dq = self.D, self.D_c, self.D_p, self.D_q
        return {
            "UI": self._normal((self.n_user + self.n_item, D), 0.01, s),
            "Context": self._normal((self.features_M, Dc), 0.01, s + 1),
            "W": self._normal((D, Dp, Dc), 0.01, s + 2),
            "Z": self._normal((D, Dq, Dc), 0.01, s + 3),
            "A": torch.zeros(Dp, device=self.device),
            "B": torch.zeros(Dq, device=self.device),
        }

    def set_weights(self, **arrays):
        super().set_weights(**arrays)
        self._prep = None

    @property
    def table(self) -> torch.Tensor:
        """UI in its storage dtype (what the scoring kernels read)."""
        E = self.weights["UI"]
        if self.table_dtype == torch.float32:
            return E
        if getattr(self, "_table_cache_src", None) is not E or self._table_cache_ver != E._version:
            self._table_cache = E.to(self.table_dtype).contiguous()
            self._table_cache_src = E
            self._table_cache_ver = E._version
        return self._table_cache

    def _prepared(self) -> torch.Tensor:
        """The folded tables of hhfm_cars2_prepare for the current weights."""
        W = self.weights
        key = tuple((id(W[n]), W[n]._version) for n in self.NAMES[1:])
        if self._prep is None or self._prep[0] != key:
            self._prep = (key, ops.cars2_prepare(W["Context"], W["W"], W["Z"], W["A"], W["B"]))
        return self._prep[1]

    # -- conversions -----------------------------------------------------------
    def _idx(self, X, ctx_last=True) -> torch.Tensor:
        """Ids -> device int32 [rows, columns].  The columns have two ranges —
        UI rows, and context ids in the last column when ``ctx_last`` (rows
        and queries) — which the scoring kernels check themselves (the status
        word, raised by ``_check``); wider integers are range-checked before
        narrowing."""
        if isinstance(X, torch.Tensor):
            if X.dtype != torch.int32 and self.validate and X.numel():
                self._host_check(X.cpu().numpy(), ctx_last)
            t = X.to(device=self.device, dtype=torch.int32)
        else:
            a = np.asarray(X)
            if a.dtype != np.int32 and self.validate and a.size:
                self._host_check(a, ctx_last)
            t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
        if t.dim() != 2:
            raise ValueError("expected a 2-D index matrix [rows, columns]")
        return t.contiguous()

    def _host_check(self, a, ctx_last):
        a = np.asarray(a)
        n_ui = self.n_user + self.n_item
        for col, hi in zip(a.T, [n_ui] * (a.shape[1] - 1)
                           + [self.features_M if ctx_last else n_ui]):
            if col.size and (int(col.min()) < 0 or int(col.max()) >= hi):
                raise ValueError(f"indices must be in [0, {hi}), got "
                                 f"[{int(col.min())}, {int(col.max())}]")

    def _status(self):
        return ops.status_word(self.device) if self.validate else None

    def _check(self):
        if self.validate:
            ops.check_status(self.device, self.features_M)

    # -- scoring ---------------------------------------------------------------
    def score_rows(self, X) -> np.ndarray:
        """PositiveFeadback for rows [user id, item id, context id] -> [B, 1]."""
        idx = self._idx(X)
        out = ops.cars2_score_rows(idx, self.table, self._prepared(), self.features_M,
                                   status=self._status())
        self._check()
        return self._np_out(out)

    def _exclusion(self, q, exclude):
        """``exclude`` of a topk call as ops.ExclusionLists (or None): the lists
        themselves (rows of UI), or a dict (user id, context id) -> set of UI
        rows, looked up with the query rows ``q`` [B, 2]."""
        if exclude is None or isinstance(exclude, ops.ExclusionLists):
            return exclude
        if not isinstance(exclude, dict):
            raise TypeError("exclude must be an ops.ExclusionLists or a dict key -> set of ids")
        rows = q.cpu().numpy() if isinstance(q, torch.Tensor) else np.asarray(q)
        return ops.exclusion_lists([exclude.get(tuple(r), ()) for r in rows.tolist()],
                                   self.device)

    def catalog_topk(self, q, begin, count, K, exclude=None):
        """Top-K of items [begin, begin+count) for queries ``q`` [B, 2] = (user
        id, context id) (CARS2.py:171-187) -> (scores, global item offsets)
        device tensors [B, K].  ``exclude``: an ops.ExclusionLists of UI rows, or
        a dict (user id, context id) -> set of UI rows, that every query leaves
        out (include/hhfm.h "Exclusion lists")."""
        extra = {} if exclude is None else {"exclude": self._exclusion(q, exclude)}
        out = ops.cars2_catalog_topk(q, self.table, self._prepared(), self.features_M, int(K),
                                     self.n_user + begin, count, begin, status=self._status(),
                                     **extra)
        self._check()
        return out

    def topk(self, feed, tp, exclude=None):
        """``feed``: the reference's dict {'X': user ids [B], 'F1': context ids
        [B]} (CARS2.py:332) or an array [B, 2]; ``exclude`` as in catalog_topk."""
        if isinstance(feed, dict):
            feed = np.stack([np.asarray(feed["X"]).reshape(-1),
                             np.asarray(feed["F1"]).reshape(-1)], axis=1)
        _, ids = self.catalog_topk(self._idx(feed), 0, self.n_item, tp, exclude=exclude)
        return ids.cpu().numpy()

    def _run_fetch(self, fetch, feed):
        if fetch is self.PositiveFeadback:
            rows = np.concatenate([np.asarray(feed[self.Pos]).reshape(-1, 2),
                                   np.asarray(feed[self.Fea]).reshape(-1, 1)], axis=1)
            return self.score_rows(rows)
        return super()._run_fetch(fetch, feed)

    def partial_fit(self, data):
        from .training import cars2_partial_fit
        return cars2_partial_fit(self, data)


def _context_ids(feature_inject, rows):
    """feature_inject of the context columns of ``rows`` [B, 2 + contexts]
    (CARS2.py:249, :307-308, :331)."""
    return np.fromiter((feature_inject[tuple(r)] for r in np.asarray(rows)[:, 2:].tolist()),
                       dtype=np.int64, count=len(rows))


class _FullRows:
    """What the harness sees as its model: full rows [user, item, ctx...] in,
    (user, item, context id) to the CARS2 model (CARS2.py:307-311, :329-333)."""

    def __init__(self, model, feature_inject):
        self._m, self._fi = model, feature_inject
        self.device = getattr(model, "device", None)

    def _ctx(self, rows):
        return _context_ids(self._fi, rows)

    def score_rows(self, rows):
        rows = np.asarray(rows)
        return self._m.score_rows(np.column_stack([rows[:, 0], rows[:, 1], self._ctx(rows)]))

    def topk(self, rows, tp, exclude=None):
        """``exclude``: an ops.ExclusionLists, or a positive_feedback-style dict
        keyed by the full rows' columns but the item."""
        rows = np.asarray(rows)
        if isinstance(exclude, dict):
            exclude = ScoringModel._exclusion(self._m, rows, exclude)
        extra = {} if exclude is None else {"exclude": exclude}
        return self._m.topk({"X": rows[:, 0], "F1": self._ctx(rows)}, tp, **extra)


class Train(harness.Train):
    method = "CARS2"
    eval_num = 300                   # CARS2.py:327
    auc_first_chunk_only = True      # CARS2.py:320 (returns inside the loop)
    auc_label_filter = False         # CARS2.py:297

    def __init__(self, args, data=None, model=None):
        data = data if data is not None else DATA.LoadData(args.path, args.dataset)
        super().__init__(args, data=data)
        # CARS2.py:212-216, the same set-of-tuples iteration
        set1 = set()
        for line in self.data.Total_data.values[:, 3:]:
            set1.add(tuple(line))
        self.feature_inject = {f: i for i, f in enumerate(set1)}
        self.features_M = len(self.feature_inject.keys())
        print("OurModel: dataset=%s, factors=%d, #epoch=%d, batch=%d, lr=%.4f, lambda=%.1e, "
              "keep=%.2f, optimizer=%s, batch_norm=%d"
              % (args.dataset, args.hidden_factor, args.epoch, args.batch_size, args.lr,
                 args.lamda, args.keep, args.optimizer, args.batch_norm))
        self.model = model if model is not None else CARS2(
            self.features_M, self.n_user, self.n_item, args.hidden_factor, args.lr, args.lamda,
            args.optimizer, deterministic=bool(getattr(args, "deterministic", 0)))

    def _through_full_rows(self, fn, data1):
        real = self.model
        self.model = _FullRows(real, self.feature_inject)
        try:
            return fn(data1)
        finally:
            self.model = real

    def evaluate_AUC(self, data1):
        return self._through_full_rows(super().evaluate_AUC, data1)

    def evaluate_TopK(self, data1):
        return self._through_full_rows(super().evaluate_TopK, data1)

    def evaluate_TopK_filtered(self, data1):
        return self._through_full_rows(super().evaluate_TopK_filtered, data1)

    def context_ids(self, rows):
        return _context_ids(self.feature_inject, rows)

    def train(self):
        from .training import run_training_cars2
        return run_training_cars2(self)


def CARS2_main(dataname, factor, Topk, argv=None):
    args = parse_args(dataname, factor, Topk, argv)
    session = Train(args)
    session.train()
    return session
