"""Training surface (§8f "next" H6): ``partial_fit`` of FM, HHFM, DeepFM, AFM
and CARS2 on the gfx950 train-step kernels and the reference's epoch loops.

* FM / AFM / DFM loop — FM.py:221-282: each epoch NG=2 negatives per
  positive (label 0 for FM, -1 for AFM/DFM, FM.py:248 / AFM.py:317), shuffle,
  ``partial_fit`` over ``batch_size`` chunks, evaluation every ``verbose``
  epochs (or the loss-plateau rule when ``Result == 1``).
* HHFM loop — OurModel7.py:364-413: shuffle the train rows in place, NG=10
  negatives per row, BPR-max ``partial_fit``, evaluation every 10 epochs.
Result lines are printed and appended to ``args.result_file`` (the
reference's ``../result.txt``).
"""
from __future__ import annotations

from time import time

import numpy as np
import torch

from . import ops
from .harness import partition_all
from ._native import native

# --optimizer names (FM.py:129-136, AFM.py:151-158, OurModel7.py:186-193) -> the
# train kernels' optimizer codes (enum hhfm_optimizer, include/hhfm.h)
_OPT = {"AdagradOptimizer": 0, "GradientDescentOptimizer": 1, "MomentumOptimizer": 2,
        "AdamOptimizer": 3}
_ADAGRAD, _SGD, _MOMENTUM, _ADAM = _OPT.values()


def _opt_code(model):
    try:
        return _OPT[model.optimizer_type]
    except KeyError:
        raise NotImplementedError(f"optimizer {model.optimizer_type!r} (the reference accepts "
                                  f"{', '.join(_OPT)})") from None


def _slots(opt, t):
    """The optimizer's slot array for variable ``t``: Adagrad's accumulator
    (TF initial_accumulator_value 0.1), Momentum's zeroed accumulator, Adam's
    zeroed m then v (2 × numel); SGD keeps none (a 1-element placeholder)."""
    if opt == _ADAGRAD:
        return torch.full_like(t, 0.1)
    if opt == _MOMENTUM:
        return torch.zeros_like(t)
    if opt == _ADAM:
        return torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)
    return torch.zeros(1, dtype=t.dtype, device=t.device)


def _state(model, names, opt, fixed_ws=False):
    """The model's train state, created on first use: optimizer slots
    (``_slots``) per variable of ``names``, ``loss``, ``opt`` and the workspace
    ``ws`` — FM / HHFM's fixed one (``fixed_ws``; zeroed gradient buffers,
    Adam's β1^t, β2^t), or None for ``_ensure_ws`` to size by the batch."""
    st = getattr(model, "_train_state", None)
    if st is not None and st["opt"] != opt:
        raise ValueError("the optimizer changed after the first partial_fit")
    if st is None:
        if model.table_dtype != torch.float32:
            raise NotImplementedError("training runs on fp32 tables")
        st = {n: _slots(opt, model.weights[n]) for n in names}
        st["opt"] = opt
        st["loss"] = torch.zeros(1, dtype=torch.float32, device=model.device)
        st["ws"], st["ws_rows"] = None, 0
        st["step"] = 0   # partial_fit calls so far: the high word of the dropout seed
        if fixed_ws:
            M, k = model.weights["feature_embeddings"].shape
            st["ws"] = _grow(None, native().train_workspace(M, k), 0, model.device)
        model._train_state = st
    return st


def _grow(old, nbytes, state_bytes, dev):
    """A zero-filled train workspace of ``nbytes``; only the persistent prefix
    of the old one (``state_bytes``: include/hhfm.h hhfm_*_train_state_bytes —
    gradients, Adam's β powers, the touched mask) carried over, the per-batch
    scratch after it left zeroed."""
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    if old is not None:
        ws[:state_bytes].copy_(old[:state_bytes])
    return ws


def _ensure_ws(st, B, dev, size_fn, state_fn):
    """``st["ws"]`` large enough for a batch of ``B`` rows: ``size_fn(B)`` bytes,
    the first ``state_fn()`` of them kept when it has to grow (``_grow``)."""
    if st["ws"] is None or st["ws_rows"] < B:
        st["ws"] = _grow(st["ws"], size_fn(B), state_fn(), dev)
        st["ws_rows"] = B
    return st["ws"]


def _labels(model, data):
    return torch.as_tensor(np.asarray(data["Y"], np.float32).reshape(-1)).to(model.device)


def _keep(value, n):
    """``n`` dropout keep probabilities in (0, 1] (tf.nn.dropout raises
    ValueError outside it)."""
    keep = [float(x) for x in np.ravel(value)]
    if len(keep) != n or not all(0.0 < x <= 1.0 for x in keep):
        raise ValueError(f"keep must be {n} probabilit{'y' if n == 1 else 'ies'} in (0, 1], "
                         f"got {value!r}")
    return keep


def _next_seed(model, st):
    """The step's dropout seed (include/hhfm.h "Training dropout"): the model's
    random_seed in the low word, the count of its earlier partial_fit calls in
    the high word."""
    seed = (int(model.random_seed) & 0xffffffff) | ((st["step"] & 0xffffffff) << 32)
    st["step"] += 1
    return seed


def _det_scratch(model, st, B, occ_per_row=None, size_fn=None):
    """The deterministic steps' per-batch scratch (include/hhfm.h
    hhfm_train_det_scratch, or ``size_fn(B)`` bytes for AFM / DeepFM),
    reallocated when a larger batch comes: it carries no state, so there is
    nothing to copy or zero."""
    if st.get("det") is None or st["det_rows"] < B:
        M, k = model.weights["feature_embeddings"].shape
        nbytes = size_fn(B) if size_fn else native().train_det_scratch(B, occ_per_row, k, M)
        st["det"] = torch.empty(nbytes, dtype=torch.uint8, device=model.device)
        st["det_rows"] = B
    return st["det"]


def fm_partial_fit(model, data) -> float:
    """FM.partial_fit (FM.py:168-171): one optimizer step, returns the loss
    (of the dropped forward when keep < 1, FM.py:114)."""
    opt = _opt_code(model)
    keep, = _keep(model.keep, 1)
    if getattr(model, "batch_norm", 0):
        return _fm_bn_partial_fit(model, data, opt, keep)
    W = model.weights
    st = _state(model, ["feature_embeddings", "feature_bias", "bias"], opt, fixed_ws=True)
    X = model._idx(data["X"])
    y = _labels(model, data)
    B, F = X.shape
    M, k = W["feature_embeddings"].shape
    args = (X.data_ptr(), y.data_ptr(), B, F, W["feature_embeddings"].data_ptr(),
            W["feature_bias"].data_ptr(), W["bias"].data_ptr(), M, k, float(model.learning_rate),
            float(model.lamda_bilinear), opt, keep, _next_seed(model, st),
            st["feature_embeddings"].data_ptr(), st["feature_bias"].data_ptr(),
            st["bias"].data_ptr(), st["ws"].data_ptr(), st["ws"].numel())
    tail = (st["loss"].data_ptr(), ops._stream(model.device))
    if getattr(model, "deterministic", False):
        sc = _det_scratch(model, st, B, F)
        native().fm_train_step_det(*args, sc.data_ptr(), sc.numel(), *tail)
    else:
        native().fm_train_step_ex(*args, *tail)
    return float(st["loss"].item())


def _fm_bn_partial_fit(model, data, opt, keep) -> float:
    """FM.partial_fit with batch_norm=1 (FM.py:111-112, :160-166; include/hhfm.h
    "FM batch norm"): the step's optimizer also acts on bn_gamma / bn_beta, and
    the forward moves bn_moving_mean / bn_moving_variance."""
    W = model.weights
    names = ["feature_embeddings", "feature_bias", "bias", "bn_gamma", "bn_beta"]
    st = _state(model, names, opt)
    X = model._idx(data["X"])
    y = _labels(model, data)
    B, F = X.shape
    M, k = W["feature_embeddings"].shape
    nat = native()
    ws = _ensure_ws(st, B, model.device, lambda b: nat.fm_train_bn_workspace(b, M, k),
                    lambda: nat.fm_train_bn_state_bytes(M, k))
    ptr = lambda n: W[n].data_ptr()  # noqa: E731
    nat.fm_train_step_bn(
        X.data_ptr(), y.data_ptr(), B, F, ptr("feature_embeddings"), ptr("feature_bias"),
        ptr("bias"), M, k, float(model.learning_rate), float(model.lamda_bilinear), opt, keep,
        _next_seed(model, st), st["feature_embeddings"].data_ptr(),
        st["feature_bias"].data_ptr(), st["bias"].data_ptr(), ws.data_ptr(), ws.numel(),
        ptr("bn_gamma"), ptr("bn_beta"), ptr("bn_moving_mean"), ptr("bn_moving_variance"),
        float(model.bn_eps), float(model.bn_update), st["bn_gamma"].data_ptr(),
        st["bn_beta"].data_ptr(), st["loss"].data_ptr(), ops._stream(model.device))
    return float(st["loss"].item())


def hhfm_partial_fit(model, data) -> float:
    """OUR.partial_fit (OurModel7.py:219-228): data X [B,2], Y [B,NG] negatives,
    F1 ctx columns, F2 time columns."""
    pooling = getattr(model, "pooling", None)
    pooling2 = getattr(model, "pooling2", None)
    if pooling2 is not None and getattr(model, "deterministic", False):
        raise NotImplementedError("deterministic=True has no two-way step yet "
                                  "(hhfm_hhfm_train_step_det is one-way sum pooling only)")
    if pooling is not None and getattr(model, "deterministic", False):
        raise NotImplementedError("deterministic=True has no MAX / MEAN pooled step yet "
                                  "(hhfm_hhfm_train_step_det is sum pooling only)")
    opt = _opt_code(model)
    W = model.weights
    st = _state(model, ["feature_embeddings"], opt, fixed_ws=True)
    parts = [np.asarray(data["X"])]
    if model.context:
        parts.append(np.asarray(data["F1"]))
    if model.time:
        parts.append(np.asarray(data["F2"]))
    X = model._idx(np.concatenate(parts, axis=1))
    Neg = model._idx(np.asarray(data["Y"]))
    B, ncols = X.shape
    ctx, tim = model._ranges(ncols)
    M, k = W["feature_embeddings"].shape
    NG = Neg.shape[1]
    args = (X.data_ptr(), Neg.data_ptr(), B, ncols, ctx[0], ctx[1], tim[0], tim[1], NG,
            W["feature_embeddings"].data_ptr(), M, k, float(model.learning_rate),
            float(model.lamda_bilinear), opt, st["feature_embeddings"].data_ptr(),
            st["ws"].data_ptr(), st["ws"].numel())
    tail = (st["loss"].data_ptr(), ops._stream(model.device))
    if pooling2 is not None:
        native().hhfm_train_step_pool2(*args, ops.pooling_word(pooling),
                                       ops.pooling_word(pooling2), *tail)
    elif pooling is not None:
        native().hhfm_train_step_pool(*args, ops.pooling_word(pooling), *tail)
    elif getattr(model, "deterministic", False):
        occ = 2 + NG + (ctx[1] - ctx[0]) + (tim[1] - tim[0])   # item, negatives, user, fields
        sc = _det_scratch(model, st, B, occ)
        native().hhfm_train_step_det(*args, sc.data_ptr(), sc.numel(), *tail)
    else:
        native().hhfm_train_step(*args, *tail)
    return float(st["loss"].item())


def cars2_partial_fit(model, data) -> float:
    """CARS2.partial_fit (CARS2.py:167-170): data X [B,2] (user, item), Y [B,NG]
    negatives (summed, :87), F1 [B] context ids; one TF step on the six
    variables (include/hhfm.h "CARS2")."""
    if getattr(model, "deterministic", False):
        raise NotImplementedError("deterministic=True has no CARS2 step "
                                  "(hhfm_cars2_train_step sums with float atomics)")
    opt = _opt_code(model)
    W = model.weights
    names = list(model.NAMES)
    st = _state(model, names, opt)
    X = model._idx(np.asarray(data["X"]).reshape(-1, 2), ctx_last=False)
    Neg = model._idx(np.asarray(data["Y"]), ctx_last=False)
    Fea = model._idx(np.asarray(data["F1"]).reshape(-1, 1))
    B, NG = Neg.shape
    if X.shape[0] != B or Fea.shape[0] != B:
        raise ValueError("X, Y and F1 must have the same number of rows")
    if model.validate and B:
        n_ui = model.n_user + model.n_item
        ops.validate_ids(X, n_ui)
        ops.validate_ids(Neg, n_ui)
        ops.validate_ids(Fea, model.features_M)
    n_ui, D = W["UI"].shape
    Mc, Dc = W["Context"].shape
    Dp, Dq = W["W"].shape[1], W["Z"].shape[1]
    nat = native()
    ws = _ensure_ws(st, B, model.device,
                    lambda b: nat.cars2_train_workspace(b, n_ui, Mc, D, Dc, Dp, Dq),
                    lambda: nat.cars2_train_state_bytes(n_ui, Mc, D, Dc, Dp, Dq))
    ptr = lambda n: W[n].data_ptr()  # noqa: E731
    nat.cars2_train_step(X.data_ptr(), Fea.data_ptr(), Neg.data_ptr(), B, NG, ptr("UI"), n_ui,
                         ptr("Context"), Mc, ptr("W"), ptr("Z"), ptr("A"), ptr("B"), D, Dc, Dp,
                         Dq, float(model.learning_rate), float(model.lamda_bilinear), opt,
                         [st[n].data_ptr() for n in names] if opt != _SGD else [],
                         ws.data_ptr(), ws.numel(), st["loss"].data_ptr(),
                         ops._stream(model.device))
    model._prep = None   # the folded tables of the scoring path are stale
    return float(st["loss"].item())


def dfm_partial_fit(model, data) -> float:
    """DeepFM.partial_fit (DFM.py:214-217): one TF Adagrad step on every
    variable the model's head gives a gradient (DFM.py:155; without use_deep
    no layer moves, without use_fm not feature_bias), loss l2_loss(y − out) or
    log_loss(y, sigmoid(out)) + l2_reg on the concat projection and, with
    use_deep, the layer weights (DFM.py:139-152)."""
    W = model.weights
    L = len(model.deep_layers)
    names = (["feature_embeddings", "feature_bias"] + [f"layer_{i}" for i in range(L)]
             + [f"bias_{i}" for i in range(L)] + ["concat_projection", "concat_bias"])
    st = _state(model, names, _ADAGRAD)
    X = model._idx(data["X"])
    y = _labels(model, data)
    B, F = X.shape
    M, k = W["feature_embeddings"].shape
    dims = [int(d) for d in model.deep_layers]
    nat = native()
    ws = _ensure_ws(st, B, model.device, lambda b: nat.dfm_train_workspace(b, F, k, M, dims),
                    lambda: nat.dfm_train_state_bytes(F, k, M, dims))
    ptr = lambda n: W[n].data_ptr()  # noqa: E731
    args = (X.data_ptr(), y.data_ptr(), B, F, ptr("feature_embeddings"), ptr("feature_bias"), M,
            k, dims, [ptr(f"layer_{i}") for i in range(L)], [ptr(f"bias_{i}") for i in range(L)],
            ptr("concat_projection"), ptr("concat_bias"), float(model.learning_rate),
            float(model.l2_reg), _ADAGRAD, [st[n].data_ptr() for n in names], ws.data_ptr(),
            ws.numel())
    tail = (st["loss"].data_ptr(), ops._stream(model.device))
    head = getattr(model, "head", 3)
    head = () if head == 3 else (head,)   # the default model: the entry points without a head
    det = getattr(model, "deterministic", False)
    if det:
        sc = _det_scratch(model, st, B,
                          size_fn=lambda b: nat.dfm_train_det_scratch(b, F, k, M, dims))
        step = nat.dfm_train_step_head_det if head else nat.dfm_train_step_det
        step(*args, sc.data_ptr(), sc.numel(), *tail, *head)
    else:
        step = nat.dfm_train_step_head if head else nat.dfm_train_step
        step(*args, *tail, *head)
    model._prep = None   # the scoring path's prepared (transposed / bf16) weights are stale
    return float(st["loss"].item())


def afm_partial_fit(model, data) -> float:
    """AFM.partial_fit (AFM.py:205-207): one TF step on every variable, loss
    l2_loss(y − out) + l2_regularizer(λ)(attention_W) when λ > 0 (AFM.py:144-148);
    keep = [attention, AFM k-vector] (AFM.py:126, :134)."""
    opt = _opt_code(model)
    keep_att, keep_afm = _keep(model.keep, 2)
    W = model.weights
    names = ["feature_embeddings", "feature_bias", "bias", "attention_W", "attention_b",
             "attention_p", "prediction"]
    st = _state(model, names, opt)
    X = model._idx(data["X"])
    y = _labels(model, data)
    B, F = X.shape
    M, k = W["feature_embeddings"].shape
    A = W["attention_W"].shape[1]
    nat = native()
    ws = _ensure_ws(st, B, model.device, lambda b: nat.afm_train_workspace(b, F, k, A, M),
                    lambda: nat.afm_train_state_bytes(F, k, A, M))
    lam = float(model.lamda_attention) if model.lamda_attention > 0 else 0.0
    ptr = lambda n: W[n].data_ptr()  # noqa: E731
    args = (X.data_ptr(), y.data_ptr(), B, F, ptr("feature_embeddings"), ptr("feature_bias"),
            ptr("bias"), M, k, A, ptr("attention_W"), ptr("attention_b"), ptr("attention_p"),
            ptr("prediction"), float(model.learning_rate), lam, opt, keep_att, keep_afm,
            _next_seed(model, st), [st[n].data_ptr() for n in names] if opt != _SGD else [],
            ws.data_ptr(), ws.numel())
    tail = (st["loss"].data_ptr(), ops._stream(model.device))
    if getattr(model, "deterministic", False):
        sc = _det_scratch(model, st, B,
                          size_fn=lambda b: nat.afm_train_det_scratch(b, F, k, A, M))
        nat.afm_train_step_det(*args, sc.data_ptr(), sc.numel(), *tail)
    else:
        nat.afm_train_step_ex(*args, *tail)
    return float(st["loss"].item())


def afm_noatt_partial_fit(model, data) -> float:
    """AFM.partial_fit with attention=0 (AFM.py:103-148 with self.attention
    false; include/hhfm.h "AFM without attention"): one TF step on the four
    variables, loss l2_loss(y − out) without a regulariser; keep[0] is
    validated and has no site, keep[1] drops the k-vector (AFM.py:134)."""
    opt = _opt_code(model)
    _, keep_afm = _keep(model.keep, 2)
    W = model.weights
    names = ["feature_embeddings", "feature_bias", "bias", "prediction"]
    st = _state(model, names, opt)
    X = model._idx(data["X"])
    y = _labels(model, data)
    B, F = X.shape
    M, k = W["feature_embeddings"].shape
    nat = native()
    if st["ws"] is None:   # fixed: the layout does not depend on the batch
        st["ws"] = _grow(None, nat.afm_noatt_train_workspace(M, k), 0, model.device)
    ptr = lambda n: W[n].data_ptr()  # noqa: E731
    args = (X.data_ptr(), y.data_ptr(), B, F, ptr("feature_embeddings"), ptr("feature_bias"),
            ptr("bias"), ptr("prediction"), M, k, float(model.learning_rate), opt, keep_afm,
            _next_seed(model, st), [st[n].data_ptr() for n in names] if opt != _SGD else [],
            st["ws"].data_ptr(), st["ws"].numel())
    tail = (st["loss"].data_ptr(), ops._stream(model.device))
    if getattr(model, "deterministic", False):
        sc = _det_scratch(model, st, B,
                          size_fn=lambda b: nat.afm_noatt_train_det_scratch(b, F, k, M))
        nat.afm_noatt_train_step_det(*args, sc.data_ptr(), sc.numel(), *tail)
    else:
        nat.afm_noatt_train_step(*args, *tail)
    return float(st["loss"].item())


def _log(tr, line):
    print(line)
    path = getattr(tr.args, "result_file", None)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _evaluate(tr):
    # --filter_seen 1: the top-K lists leave out each key's train positives
    topk = tr.evaluate_TopK_filtered if getattr(tr.args, "filter_seen", 0) else tr.evaluate_TopK
    return (tr.evaluate_AUC(tr.data.Train_data), tr.evaluate_AUC(tr.data.Test_data),
            topk(tr.data.Test_data))


def _report_init(tr):
    """The evaluation of the untrained model both epoch loops log first (Result == 0)."""
    args = tr.args
    t0 = time()
    if args.Result == 0:
        a1, a2, tk = _evaluate(tr)
        _log(tr, "Dataset=%s %s Init: \t train=AUC:%.4f;test=AUC:%.4f,HR:%.4f,NDCG:%.4f,PRE:%.4f;"
             "[%.1f s]" % (args.dataset, tr.method, a1, a2, tk[0], tk[1], tk[2], time() - t0))


def _report(tr, head, t_epoch, t_eval0, res):
    a1, a2, tk = res
    _log(tr, "%s [%.1f s]\ttrain=AUC:%.4f;test=AUC:%.4f,HR:%.4f,NDCG:%.4f,PRE:%.4f;[%.1f s]"
         % (head, t_epoch, a1, a2, tk[0], tk[1], tk[2], time() - t_eval0))


def run_training(tr, negatives=2, neg_label=0, plateau=-0.0075, epoch_cap=100):
    """FM.py:221-282 (also AFM.py:290-351, DFM.py:259-320).  The loss-plateau
    stop (Result == 1) is ``plateau`` = −0.0075 with a 100-epoch cap in FM
    (FM.py:261-262), −0.0075 without a cap in DFM (DFM.py:299-300) and −0.01
    without a cap in AFM (AFM.py:330-331)."""
    args = tr.args
    _report_init(tr)
    tr.loss_epoch = []
    for epoch in range(1, tr.epoch):
        loss = 0.0
        t1 = time()
        pos = tr.data.Train_data.values
        rep = np.repeat(np.array(pos, copy=True)[:, None, :], negatives, axis=1)
        rep = rep.reshape(-1, rep.shape[2])
        negs = tr.sample_negative(pos[:, 1:], negatives)
        rep[:, 2] = negs.reshape(-1)
        rep[:, 0] = neg_label
        dat = np.append(pos, rep, axis=0)
        np.random.shuffle(dat)
        for chunk in partition_all(tr.batch_size, range(len(dat))):
            X = np.array(dat[chunk][:, 1:], dtype=np.int64)
            Y = np.expand_dims(dat[chunk][:, 0], axis=1)
            loss = loss + tr.model.partial_fit({"X": X, "Y": Y})
        tr.loss_epoch.append(loss)
        t2 = time()
        if args.Result == 1 and epoch > 30:
            n = 3
            le = np.array(tr.loss_epoch)
            cond = np.sum((le[-1 - n:-1] / le[-2 - n:-2] - 1) > plateau)
            if cond == n or (epoch_cap is not None and epoch > epoch_cap):
                _report(tr, "%s%s Epoch %d" % (args.dataset, tr.method, epoch), t2 - t1, t2,
                        _evaluate(tr))
                break
        if args.Result == 0 and tr.verbose > 0 and epoch % tr.verbose == 0:
            _report(tr, "%s Epoch %d" % (tr.method, epoch), t2 - t1, t2, _evaluate(tr))
    return tr.loss_epoch


def _hhfm_fields(tr, rows, batch):
    """The context / time columns of an HHFM batch (OurModel7.py:374-385)."""
    td = tr.time_dimension
    if tr.context and tr.time:
        batch["F1"] = np.array(rows[:, 2:-td], dtype=np.int64)
        batch["F2"] = np.array(rows[:, -td:], dtype=np.int64)
    elif tr.context:
        batch["F1"] = np.array(rows[:, 2:], dtype=np.int64)
    else:
        batch["F2"] = np.array(rows[:, 2:], dtype=np.int64)


def _cars2_fields(tr, rows, batch):
    """The context id of a CARS2 batch (CARS2.py:249)."""
    batch["F1"] = tr.context_ids(rows)


def run_training_hhfm(tr, NG=10, plateau_after=20, fields=_hhfm_fields):
    """OurModel7.py:349-413; CARS2.py:222-279 is the same loop with ``NG`` = 1,
    the plateau rule from epoch 11 and the context id as the only field
    (``run_training_cars2``)."""
    args = tr.args
    _report_init(tr)
    tr.loss_epoch = []
    for epoch in range(1, tr.epoch):
        loss = 0.0
        t1 = time()
        pos = tr.data.Train_data.values[:, 1:]
        np.random.shuffle(pos)            # in place, like the reference (:369-370)
        negs = tr.sample_negative(pos, NG)
        for chunk in partition_all(tr.batch_size, range(len(pos))):
            rows = pos[chunk]
            batch = {"X": np.array(rows[:, :2], dtype=np.int64),
                     "Y": np.array(negs[chunk], dtype=np.int64)}
            fields(tr, rows, batch)
            loss = loss + tr.model.partial_fit(batch)
        tr.loss_epoch.append(loss)
        t2 = time()
        if args.Result == 1 and epoch > plateau_after:
            n = 3
            le = np.array(tr.loss_epoch)
            cond = np.sum((le[-1 - n:-1] / le[-2 - n:-2] - 1) > -0.0075)
            if cond == n or epoch > 100:
                _report(tr, "%s%s Epoch %d" % (args.dataset, tr.method, epoch), t2 - t1, t2,
                        _evaluate(tr))
                break
        if args.Result == 0 and epoch % 10 == 0:
            _report(tr, "%s Epoch %d" % (tr.method, epoch), t2 - t1, t2, _evaluate(tr))
    return tr.loss_epoch


def run_training_cars2(tr):
    """CARS2.py:222-279: NG = 1, the plateau rule from epoch 11 (capped at 100)."""
    return run_training_hhfm(tr, NG=1, plateau_after=10, fields=_cars2_fields)
