"""Tensor-level entry points over the C ABI (include/hhfm.h).

PyTorch-ROCm is plumbing here: it owns device memory and streams.  Every
function launches a hand-written gfx950 kernel from ``libhhfm.so`` on
``torch.cuda.current_stream()``; there is no eager-PyTorch or CPU fallback.
"""
from __future__ import annotations

import numbers
from typing import Optional, Sequence, Tuple

import torch

from ._native import native

MODE_FM = 0
MODE_HHFM = 1

# Plan flags (include/hhfm.h, ABI v4): explicit per-call kernel choices; 0 is
# the default plan.  PLAN_EXACT_FP32 selects k-ordered fp32-MFMA arithmetic
# instead of split-bf16; the others force a fallback kernel on the same
# scores (tests compare both paths on one shape).
PLAN_EXACT_FP32 = 1 << 0
PLAN_NO_SEED = 1 << 1
PLAN_NO_RING = 1 << 2
PLAN_RING_ALT = 1 << 3
PLAN_GEMM = 1 << 4
PLAN_ROW_FM = 1 << 5
PLAN_UNSTAGED = 1 << 6
PLAN_UNGROUPED = 1 << 7
PLAN_NARROW = 1 << 8
PLAN_PER_FIELD = 1 << 9
PLAN_ONE_WAVE = 1 << 10
PLAN_WIDE_3X4 = 1 << 11   # DeepFM 256-row kernel shapes (test shape only)
PLAN_WIDE_2X4 = 2 << 11
PLAN_WIDE_1X4 = 3 << 11
PLAN_STORE = 1 << 13      # small catalog: score matrix + dense top-K (not the fused kernel)
PLAN_FUSED = 1 << 14      # small catalog: the fused score-and-select kernel at any query count


# HHFM pooling modes (include/hhfm.h enum hhfm_pool): how the context rows, the
# time rows and the stack {user, context pool, time pool} are reduced
POOL_SUM = 0
POOL_MAX = 1
POOL_MEAN = 2
_POOL_NAMES = {"sum": POOL_SUM, "max": POOL_MAX, "mean": POOL_MEAN}


def pool_mode(x) -> int:
    """One pooling mode: "sum" / "max" / "mean" or a POOL_* value."""
    if isinstance(x, str) and x in _POOL_NAMES:
        return _POOL_NAMES[x]
    if isinstance(x, numbers.Integral) and not isinstance(x, bool) and int(x) in _POOL_NAMES.values():
        return int(x)
    raise ValueError(f"pooling mode must be 'sum', 'max', 'mean' or a POOL_* value, got {x!r}")


def pooling_word(pooling) -> int:
    """HHFM_POOLING(ctx, time, final) of a (ctx, time, final) triple; None is
    (sum, sum, sum) = 0."""
    if pooling is None:
        return 0
    if isinstance(pooling, (str, numbers.Integral)) or len(pooling) != 3:
        raise ValueError(f"pooling must be a (ctx, time, final) triple, got {pooling!r}")
    c, t, f = (pool_mode(x) for x in pooling)
    return c | t << 4 | f << 8


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return 0
    if t.dtype == torch.bfloat16:
        return 1
    raise TypeError(f"embedding table must be float32 or bfloat16, got {t.dtype}")


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _need_cuda(*ts: Optional[torch.Tensor]) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError("hhfm_amd kernels take device (cuda/HIP) tensors")
        if not t.is_contiguous():
            raise ValueError("hhfm_amd kernels take contiguous tensors")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError("all tensors must be on the same device")
    return dev


def _idx(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.int32:
        raise TypeError(f"{name} must be int32 (the reference feeds int32 placeholders)")
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D [rows, cols]")
    return t


_STATUS = {}


def status_word(dev: torch.device) -> torch.Tensor:
    """This device's id status word (include/hhfm.h HHFM_STATUS_BAD_ID)."""
    t = _STATUS.get(dev.index)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=dev)
        _STATUS[dev.index] = t
    return t


def check_status(dev: torch.device, features_M: int) -> None:
    """Synchronise and raise like tf.nn.embedding_lookup (InvalidArgumentError,
    FM.py:99) if a kernel on this stream met an id outside [0, features_M)."""
    if native().status_read(status_word(dev).data_ptr(), _stream(dev)) != 0:
        raise ValueError(f"indices must be in [0, {features_M})")


def validate_ids(idx: torch.Tensor, features_M: int) -> None:
    """Raise like tf.nn.embedding_lookup does for ids outside [0, M): one
    hhfm_check_ids kernel + a 4-byte status read (the kernels themselves read
    such ids as row 0, so they can never fault)."""
    if idx.numel() == 0:
        return
    dev = _need_cuda(idx)
    native().check_ids(idx.data_ptr(), idx.numel(), int(features_M),
                       status_word(dev).data_ptr(), _stream(dev))
    check_status(dev, features_M)


def _status_ptr(status: Optional[torch.Tensor]) -> int:
    if status is None:
        return 0
    if status.dtype != torch.int32 or status.numel() < 1 or not status.is_cuda:
        raise TypeError("status must be a device int32 tensor")
    return status.data_ptr()


def fm_score_rows(idx: torch.Tensor, E: torch.Tensor, w: Optional[torch.Tensor],
                  w0: float = 0.0, out: Optional[torch.Tensor] = None,
                  status: Optional[torch.Tensor] = None, flags: int = 0,
                  scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FM.out (FM.py:99-120) for rows ``idx`` [B, F] -> float32 [B].
    ``status``: optional device int32 word the kernel flags bad ids in.
    ``flags``: HHFM_FLAG_* bits of include/hhfm.h, passed through (1 streams
    the table, 2 / 4 force / refuse the LDS-tail kernel; same bits out).
    ``scale``: float32 [k] column weights — hhfm_fm_score_rows_scaled, the
    batch-norm inference score Σ_c scale_c·½(s² − q) + Σw + w0; it takes no flags."""
    _idx(idx, "idx")
    dev = _need_cuda(idx, E, w, out, scale)
    B, F = idx.shape
    M, k = E.shape
    if w is not None and (w.dtype != torch.float32 or w.numel() != M):
        raise ValueError("w must be float32 with features_M entries")
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    if scale is not None:
        if scale.dtype != torch.float32 or scale.numel() != k or not scale.is_contiguous():
            raise ValueError("scale must be contiguous float32 with k entries")
        if flags:
            raise ValueError("the scaled row score takes no flags")
        native().fm_score_rows_scaled(idx.data_ptr(), B, F, E.data_ptr(), M, k, _dtype_code(E),
                                      0 if w is None else w.data_ptr(), float(w0),
                                      scale.data_ptr(), out.data_ptr(), _status_ptr(status),
                                      _stream(dev))
        return out
    native().fm_score_rows_ex(idx.data_ptr(), B, F, E.data_ptr(), M, k, _dtype_code(E),
                              0 if w is None else w.data_ptr(), float(w0),
                              out.data_ptr(), int(flags), _status_ptr(status), _stream(dev))
    return out


def hybrid_score_rows(idx: torch.Tensor, E: torch.Tensor, user_col: int = 0,
                      item_col: int = 1, ctx: Tuple[int, int] = (0, 0),
                      time: Tuple[int, int] = (0, 0),
                      out: Optional[torch.Tensor] = None,
                      status: Optional[torch.Tensor] = None,
                      pooling=None, pooling2=None) -> torch.Tensor:
    """OUR.PositiveFeadback (OurModel7.py:105-171) for rows ``idx`` -> [B].
    ``pooling``: (ctx, time, final) modes, "sum" / "max" / "mean" or POOL_*
    (OurModel7.py:14-19 Pooling1C / 1T / 1F); None is sum pooling.
    ``pooling2``: None is the one-way model; a (ctx, time, final) triple
    (Pooling2C / 2T / 2F) selects the two-way model (include/hhfm.h "Two-way
    pooling"), also when ``pooling`` is all-sum or None."""
    _idx(idx, "idx")
    dev = _need_cuda(idx, E, out)
    B, ncols = idx.shape
    M, k = E.shape
    word = pooling_word(pooling)
    word2 = pooling_word(pooling2)
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    if pooling2 is not None:
        native().hybrid_score_rows_pool2(idx.data_ptr(), B, ncols, user_col, item_col,
                                         ctx[0], ctx[1], time[0], time[1], E.data_ptr(), M, k,
                                         _dtype_code(E), out.data_ptr(), word, word2,
                                         _status_ptr(status), _stream(dev))
        return out
    if pooling is not None:
        native().hybrid_score_rows_pool(idx.data_ptr(), B, ncols, user_col, item_col,
                                        ctx[0], ctx[1], time[0], time[1], E.data_ptr(), M, k,
                                        _dtype_code(E), out.data_ptr(), word,
                                        _status_ptr(status), _stream(dev))
        return out
    native().hybrid_score_rows(idx.data_ptr(), B, ncols, user_col, item_col,
                               ctx[0], ctx[1], time[0], time[1], E.data_ptr(), M, k,
                               _dtype_code(E), out.data_ptr(), _status_ptr(status),
                               _stream(dev))
    return out


_WS = {}


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        _WS[key] = buf
    return buf


_CWS = {}


def _catalog_workspace(dev: torch.device, stream: int, nbytes: int) -> torch.Tensor:
    """hhfm_catalog_topk's own workspace per (device, stream): zero-filled when
    allocated, because its first HHFM_CATALOG_WS_ZERO bytes hold the
    small-catalog kernel's arrival counters (include/hhfm.h, ABI v6: zero
    before the first call, left zero by every call; no other op shares it)."""
    key = (dev.index, stream)
    buf = _CWS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.zeros(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
        _CWS[key] = buf
    return buf


TOPK_MAX_K = 1024       # HHFM_TOPK_MAX_K
_TOPK_NARROW_MAX_K = 64  # above it: the wide select (include/hhfm.h "Wide K")


def _check_topk_k(K: int) -> int:
    K = int(K)
    if K < 1 or K > TOPK_MAX_K:
        raise ValueError(f"K = {K}: top-K lists hold 1 to {TOPK_MAX_K} entries (TOPK_MAX_K)")
    return K


def _catalog_ws_bytes(nat, B: int, item_count: int, k: int, K: int) -> int:
    """The shared catalog workspace's size: the wide query above 64 entries."""
    if _check_topk_k(K) > _TOPK_NARROW_MAX_K:
        return nat.catalog_topk_wide_workspace(B, item_count, k, K)
    return nat.catalog_topk_workspace(B, item_count, k, K)


def _excl_args(exclude: "ExclusionLists", B: int, dev: torch.device) -> Tuple[int, int, int]:
    """(excl_ptr, excl_rows, max_excl) of a native *_excl call for B queries."""
    if exclude.ptr.numel() != B + 1:
        raise ValueError(f"exclude holds {exclude.ptr.numel() - 1} lists for {B} queries")
    if _need_cuda(exclude.ptr, exclude.rows) != dev:
        raise ValueError("exclude must live on the queries' device")
    return (exclude.ptr.data_ptr(), exclude.rows.data_ptr() if exclude.rows.numel() else 0,
            int(exclude.max_len))


def catalog_topk(qidx: torch.Tensor, E: torch.Tensor, mode: int, K: int,
                 item_row_begin: int, item_count: int, global_item_base: int = 0,
                 w: Optional[torch.Tensor] = None, user_col: int = 0,
                 ctx: Tuple[int, int] = (0, 0), time: Tuple[int, int] = (0, 0),
                 status: Optional[torch.Tensor] = None, plan: int = 0, pooling=None,
                 pooling2=None, exclude: Optional["ExclusionLists"] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Full-catalog score + top-K (FM.topk FM.py:172-198, OUR.topk
    OurModel7.py:229-307). Returns (scores float32 [B,K], ids int32 [B,K]).
    ``plan``: PLAN_* flags (PLAN_EXACT_FP32, _NO_SEED, _NO_RING, _RING_ALT,
    _GEMM, _ONE_WAVE).  ``pooling`` / ``pooling2``: as in
    :func:`hybrid_score_rows` (MODE_HHFM only; the two-way model never takes
    the small-catalog fused kernel).  ``exclude``: an :class:`ExclusionLists`
    of table rows per query — the top K of the other items
    (hhfm_catalog_topk_excl; not with ``pooling2``)."""
    _idx(qidx, "qidx")
    dev = _need_cuda(qidx, E, w)
    B, ncols = qidx.shape
    M, k = E.shape
    word = pooling_word(pooling)
    word2 = pooling_word(pooling2)
    nat = native()
    st = _stream(dev)
    ws = _catalog_workspace(dev, st, _catalog_ws_bytes(nat, B, item_count, k, K))
    top_s = torch.empty(B, K, dtype=torch.float32, device=dev)
    top_i = torch.empty(B, K, dtype=torch.int32, device=dev)
    if exclude is not None:
        if pooling2 is not None:
            raise NotImplementedError("exclusion lists have no two-way form")
        if exclude.ptr.numel() != B + 1:
            raise ValueError(f"exclude holds {exclude.ptr.numel() - 1} lists for {B} queries")
        _need_cuda(qidx, exclude.ptr, exclude.rows)
        nat.catalog_topk_excl(qidx.data_ptr(), B, ncols, mode, user_col, ctx[0], ctx[1],
                              time[0], time[1], E.data_ptr(), M, k, _dtype_code(E),
                              0 if w is None else w.data_ptr(), item_row_begin, item_count,
                              global_item_base, K, top_s.data_ptr(), top_i.data_ptr(),
                              ws.data_ptr(), ws.numel(), int(plan), word,
                              _status_ptr(status), st, exclude.ptr.data_ptr(),
                              exclude.rows.data_ptr() if exclude.rows.numel() else 0,
                              int(exclude.max_len))
        return top_s, top_i
    if pooling2 is not None:
        nat.catalog_topk_pool2(qidx.data_ptr(), B, ncols, mode, user_col, ctx[0], ctx[1],
                               time[0], time[1], E.data_ptr(), M, k, _dtype_code(E),
                               0 if w is None else w.data_ptr(), item_row_begin, item_count,
                               global_item_base, K, top_s.data_ptr(), top_i.data_ptr(),
                               ws.data_ptr(), ws.numel(), int(plan), word, word2,
                               _status_ptr(status), st)
        return top_s, top_i
    if pooling is not None:
        nat.catalog_topk_pool(qidx.data_ptr(), B, ncols, mode, user_col, ctx[0], ctx[1],
                              time[0], time[1], E.data_ptr(), M, k, _dtype_code(E),
                              0 if w is None else w.data_ptr(), item_row_begin, item_count,
                              global_item_base, K, top_s.data_ptr(), top_i.data_ptr(),
                              ws.data_ptr(), ws.numel(), int(plan), word,
                              _status_ptr(status), st)
        return top_s, top_i
    nat.catalog_topk(qidx.data_ptr(), B, ncols, mode, user_col, ctx[0], ctx[1],
                     time[0], time[1], E.data_ptr(), M, k, _dtype_code(E),
                     0 if w is None else w.data_ptr(), item_row_begin, item_count,
                     global_item_base, K, top_s.data_ptr(), top_i.data_ptr(),
                     ws.data_ptr(), ws.numel(), int(plan), _status_ptr(status), st)
    return top_s, top_i


# ---------------------------------------------------------------------------
# CARS2 (include/hhfm.h "CARS2")
# ---------------------------------------------------------------------------
def cars2_dims(hidden_factor: int) -> Tuple[int, int, int]:
    """(Dc, Dp, Dq) of CARS2.py:54-56."""
    D = int(hidden_factor)
    return int(D / 2.5), int(D / 5), int(D / 2.5)


def _cars2_f32(name, t, shape):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be float32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


def cars2_prepare(Context: torch.Tensor, W: torch.Tensor, Z: torch.Tensor, A: torch.Tensor,
                  B: torch.Tensor) -> torch.Tensor:
    """hhfm_cars2_prepare: the folded tables GA | GB | WA | ZB as one float32
    device tensor, to be passed with Mc = Context.shape[0] to
    :func:`cars2_score_rows` / :func:`cars2_catalog_topk`; stale once Context, W, Z, A or B change."""
    dev = _need_cuda(Context, W, Z, A, B)
    Mc, Dc = Context.shape
    D, Dp, _ = W.shape
    Dq = Z.shape[1]
    _cars2_f32("Context", Context, (Mc, Dc))
    _cars2_f32("W", W, (D, Dp, Dc))
    _cars2_f32("Z", Z, (D, Dq, Dc))
    _cars2_f32("A", A, (Dp,))
    _cars2_f32("B", B, (Dq,))
    nat = native()
    nbytes = nat.cars2_prepared_bytes(Mc, D, Dc)
    prepared = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    nat.cars2_prepare(Context.data_ptr(), Mc, W.data_ptr(), A.data_ptr(), Z.data_ptr(),
                      B.data_ptr(), D, Dc, Dp, Dq, prepared.data_ptr(), nbytes, _stream(dev))
    return prepared


def cars2_score_rows(idx: torch.Tensor, UI: torch.Tensor, prepared: torch.Tensor, Mc: int,
                     out: Optional[torch.Tensor] = None,
                     status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CARS2.PositiveFeadback (CARS2.py:85-105) for rows ``idx`` int32 [B, 3] =
    (user id, item id, context id) -> float32 [B]."""
    _idx(idx, "idx")
    if idx.shape[1] != 3:
        raise ValueError("idx must be [rows, 3]: user id, item id, context id")
    dev = _need_cuda(idx, UI, prepared, out)
    B = idx.shape[0]
    n_ui, D = UI.shape
    Mc = int(Mc)
    if prepared.dtype != torch.float32 or prepared.numel() < 2 * Mc * D:
        raise ValueError("prepared must be cars2_prepare's float32 tensor for this Mc and D")
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    native().cars2_score_rows(idx.data_ptr(), B, UI.data_ptr(), n_ui, D, _dtype_code(UI),
                              prepared.data_ptr(), Mc, out.data_ptr(), _status_ptr(status),
                              _stream(dev))
    return out


def cars2_catalog_topk(q: torch.Tensor, UI: torch.Tensor, prepared: torch.Tensor, Mc: int, K: int,
                       item_row_begin: int, item_count: int, global_item_base: int = 0,
                       status: Optional[torch.Tensor] = None, plan: int = 0,
                       exclude: Optional["ExclusionLists"] = None
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """CARS2.topk (CARS2.py:171-187) for queries ``q`` int32 [B, 2] = (user id,
    context id) over UI rows [item_row_begin, +item_count) -> (scores float32
    [B, K], ids int32 [B, K]); ``plan`` as in :func:`catalog_topk`.
    ``exclude``: :class:`ExclusionLists` of UI rows per query
    (hhfm_cars2_catalog_topk_excl)."""
    _idx(q, "q")
    if q.shape[1] != 2:
        raise ValueError("q must be [rows, 2]: user id, context id")
    dev = _need_cuda(q, UI, prepared)
    B = q.shape[0]
    n_ui, D = UI.shape
    Mc = int(Mc)
    if prepared.dtype != torch.float32 or prepared.numel() < 2 * Mc * D:
        raise ValueError("prepared must be cars2_prepare's float32 tensor for this Mc and D")
    nat = native()
    st = _stream(dev)
    ws = _catalog_workspace(dev, st, _catalog_ws_bytes(nat, B, item_count, D, K))
    top_s = torch.empty(B, K, dtype=torch.float32, device=dev)
    top_i = torch.empty(B, K, dtype=torch.int32, device=dev)
    args = (q.data_ptr(), B, UI.data_ptr(), n_ui, D, _dtype_code(UI), prepared.data_ptr(), Mc,
            item_row_begin, item_count, global_item_base, K, top_s.data_ptr(), top_i.data_ptr(),
            ws.data_ptr(), ws.numel(), int(plan), _status_ptr(status), st)
    if exclude is not None:
        nat.cars2_catalog_topk_excl(*args, *_excl_args(exclude, B, dev))
    else:
        nat.cars2_catalog_topk(*args)
    return top_s, top_i


def topk_merge(scores: torch.Tensor, ids: torch.Tensor
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge R sorted [B,K] lists (stacked [R,B,K], rank-major) into [B,K],
    K <= TOPK_MAX_K.  Device tensors use the HIP kernels (the wide merge above
    64 entries); host tensors the C++ host merge."""
    if scores.dim() != 3 or scores.shape != ids.shape:
        raise ValueError("expected scores/ids of shape [R, B, K]")
    if scores.dtype != torch.float32 or ids.dtype != torch.int32:
        raise TypeError("scores float32, ids int32")
    scores = scores.contiguous()
    ids = ids.contiguous()
    R, B, K = scores.shape
    out_s = torch.empty(B, K, dtype=torch.float32, device=scores.device)
    out_i = torch.empty(B, K, dtype=torch.int32, device=scores.device)
    nat = native()
    if scores.is_cuda:
        _need_cuda(scores, ids)
        _check_topk_k(K)
        nat.topk_merge(scores.data_ptr(), ids.data_ptr(), R, B, K, out_s.data_ptr(),
                       out_i.data_ptr(), _stream(scores.device))
    else:
        nat.topk_merge_host(scores.data_ptr(), ids.data_ptr(), R, B, K,
                            out_s.data_ptr(), out_i.data_ptr())
    return out_s, out_i


# ---------------------------------------------------------------------------
# DeepFM (K3) and dense top-K
# ---------------------------------------------------------------------------
def _pad8(x: int) -> int:
    return (x + 7) & ~7


def dfm_prepare_weights(layers, biases, mlp_dtype: torch.dtype, F: int, k: int):
    """Transpose (and pad K to a multiple of 8) the MLP weights into the
    [N][K] layout the GEMM kernel streams (include/hhfm.h, D1)."""
    Wt, bs, dims = [], [], []
    Kin = F * k
    for W, b in zip(layers, biases):
        W = torch.as_tensor(W)
        Kreal, N = W.shape
        t = torch.zeros(N, Kin, dtype=torch.float32, device=W.device)
        t[:, :Kreal] = W.t().float()
        Wt.append(t.to(mlp_dtype).contiguous())
        bs.append(torch.as_tensor(b).reshape(-1).float().contiguous())
        dims.append(N)
        Kin = _pad8(N)
    return Wt, bs, dims


# include/hhfm.h hhfm_dfm_proj: off / on / auto / context fields only / every
# field but the item
DFM_PROJ = {False: 0, True: 1, None: 2, "ctx": 3, "item": 4}


# DeepFM heads (include/hhfm.h HHFM_DFM_HEAD_*): which parts the concat
# projection sees, and the sigmoid output of loss_type "logloss"
DFM_HEAD_FM = 1
DFM_HEAD_DEEP = 2
DFM_HEAD_SIGMOID = 4


def dfm_head_word(use_fm: bool = True, use_deep: bool = True, loss_type: str = "mse") -> int:
    """The head word of the reference constructor's use_fm / use_deep /
    loss_type (DFM.py:131-144); 3 is the reference default."""
    if not (use_fm or use_deep):
        raise ValueError("a DeepFM head needs use_fm or use_deep")
    if loss_type not in ("mse", "logloss"):
        raise ValueError("loss_type can be either 'logloss' or 'mse'")
    return ((DFM_HEAD_FM if use_fm else 0) | (DFM_HEAD_DEEP if use_deep else 0)
            | (DFM_HEAD_SIGMOID if loss_type == "logloss" else 0))


def _head_ws_extra(head: int, F: int, k: int, dims) -> int:
    """HHFM_DFM_HEAD_WS_EXTRA: room after the plan for the deep head's
    zero-prefixed projection."""
    if head & DFM_HEAD_FM or not head & DFM_HEAD_DEEP:
        return 0
    return ((F + k + int(dims[-1])) * 4 + 255) & ~255


def _head_dims(head: int, dims):
    """The workspace queries' layer list: the model's, or one unit-wide layer
    for an FM head that carries none (its kernels touch no workspace)."""
    dims = [int(d) for d in dims]
    if not dims and not head & DFM_HEAD_DEEP:
        return [1]
    return dims


def dfm_forward(idx: torch.Tensor, E: torch.Tensor, w: torch.Tensor, Wt, bias, dims,
                mlp_dtype: torch.dtype, Wp: torch.Tensor, bp: float,
                out: Optional[torch.Tensor] = None,
                proj=None, plan: int = 0, head: Optional[int] = None) -> torch.Tensor:
    """DeepFM.out (DFM.py:104-137) for rows ``idx`` [B, F] -> float32 [B].

    ``proj``: projected layer 0 (include/hhfm.h, ABI v3) — None lets the
    library decide (include/hhfm.h HHFM_DFM_PROJ_AUTO), True / False force it
    on / off, "ctx" projects the context fields 2..F-1 only and "item" every
    field but the item (bf16 MLP).  ``plan``: PLAN_* flags (fp32 MLP:
    PLAN_EXACT_FP32, _ROW_FM, _UNSTAGED, _UNGROUPED; bf16 MLP: _NARROW).
    ``head``: a :func:`dfm_head_word` (include/hhfm.h "DeepFM heads") — ``Wp`` is
    then that head's projection, the layer lists may be empty without
    DFM_HEAD_DEEP, and DFM_HEAD_SIGMOID returns the sigmoid; None is the
    reference default on the entry point without a head word."""
    _idx(idx, "idx")
    dev = _need_cuda(idx, E, w, Wp, *Wt, *bias)
    B, F = idx.shape
    M, k = E.shape
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    nat = native()
    if head is not None:
        md = _dtype_code(Wt[0]) if len(Wt) else (1 if mlp_dtype == torch.bfloat16 else 0)
        nbytes = nat.dfm_forward_workspace_ex(B, F, k, M, _head_dims(head, dims), md,
                                              DFM_PROJ[proj])
        ws = _workspace(dev, nbytes + _head_ws_extra(head, F, k, dims))
        nat.dfm_forward_head(idx.data_ptr(), B, F, E.data_ptr(), M, k, _dtype_code(E),
                             w.data_ptr(), list(dims), [t.data_ptr() for t in Wt],
                             [t.data_ptr() for t in bias], md, Wp.data_ptr(), float(bp),
                             out.data_ptr(), DFM_PROJ[proj], int(plan), ws.data_ptr(),
                             ws.numel(), _stream(dev), int(head))
        return out
    md = _dtype_code(Wt[0])
    if mlp_dtype != Wt[0].dtype:
        raise TypeError("Wt dtype must equal mlp_dtype")
    nbytes = nat.dfm_forward_workspace_ex(B, F, k, M, list(dims), md, DFM_PROJ[proj])
    ws = _workspace(dev, nbytes)
    nat.dfm_forward(idx.data_ptr(), B, F, E.data_ptr(), M, k, _dtype_code(E), w.data_ptr(),
                    list(dims), [t.data_ptr() for t in Wt], [t.data_ptr() for t in bias], md,
                    Wp.data_ptr(), float(bp), out.data_ptr(), DFM_PROJ[proj], int(plan),
                    ws.data_ptr(), ws.numel(), _stream(dev))
    return out


def dfm_catalog_topk(qidx: torch.Tensor, E: torch.Tensor, w: torch.Tensor, Wt, bias, dims,
                     Wp: torch.Tensor, bp: float, item_col: int, item_row_begin: int,
                     item_count: int, K: int, global_item_base: int = 0,
                     chunk_rows: int = 1 << 20, proj=None, plan: int = 0,
                     head: Optional[int] = None,
                     exclude: Optional["ExclusionLists"] = None):
    """DeepFM.topk (DFM.py:219-231) -> (scores [B,K], ids [B,K]); ``proj``,
    ``plan`` and ``head`` as in :func:`dfm_forward` (rows = B x item_count).
    With a head the scores are the pre-sigmoid z whatever DFM_HEAD_SIGMOID says
    (the sigmoid is monotone: the same id lists).  ``exclude``:
    :class:`ExclusionLists` of table rows per query (hhfm_dfm_catalog_topk_excl;
    without a head it is the reference default's, fm + deep)."""
    _idx(qidx, "qidx")
    dev = _need_cuda(qidx, E, w, Wp, *Wt, *bias)
    B, F = qidx.shape
    M, k = E.shape
    K = _check_topk_k(K)
    nat = native()
    if exclude is not None and head is None:
        head = dfm_head_word()
    if head is not None:
        md = _dtype_code(Wt[0]) if len(Wt) else 0
        nbytes = nat.dfm_catalog_topk_workspace_ex(B, F, k, M, item_count,
                                                   _head_dims(head, dims), md, chunk_rows,
                                                   DFM_PROJ[proj])
        ws = _workspace(dev, nbytes + _head_ws_extra(head, F, k, dims))
        top_s = torch.empty(B, K, dtype=torch.float32, device=dev)
        top_i = torch.empty(B, K, dtype=torch.int32, device=dev)
        args = (qidx.data_ptr(), B, F, item_col, E.data_ptr(), M, k, _dtype_code(E),
                w.data_ptr(), list(dims), [t.data_ptr() for t in Wt],
                [t.data_ptr() for t in bias], md, Wp.data_ptr(), float(bp), item_row_begin,
                item_count, global_item_base, K, chunk_rows, top_s.data_ptr(),
                top_i.data_ptr(), DFM_PROJ[proj], int(plan), ws.data_ptr(), ws.numel(),
                _stream(dev), int(head))
        if exclude is not None:
            nat.dfm_catalog_topk_excl(*args, *_excl_args(exclude, B, dev))
        else:
            nat.dfm_catalog_topk_head(*args)
        return top_s, top_i
    md = _dtype_code(Wt[0])
    nbytes = nat.dfm_catalog_topk_workspace_ex(B, F, k, M, item_count, list(dims), md,
                                               chunk_rows, DFM_PROJ[proj])
    ws = _workspace(dev, nbytes)
    top_s = torch.empty(B, K, dtype=torch.float32, device=dev)
    top_i = torch.empty(B, K, dtype=torch.int32, device=dev)
    nat.dfm_catalog_topk(qidx.data_ptr(), B, F, item_col, E.data_ptr(), M, k, _dtype_code(E),
                         w.data_ptr(), list(dims), [t.data_ptr() for t in Wt],
                         [t.data_ptr() for t in bias], md, Wp.data_ptr(), float(bp),
                         item_row_begin, item_count, global_item_base, K, chunk_rows,
                         top_s.data_ptr(), top_i.data_ptr(), DFM_PROJ[proj], int(plan),
                         ws.data_ptr(), ws.numel(), _stream(dev))
    return top_s, top_i


def topk_dense(scores: torch.Tensor, K: int, global_item_base: int = 0, plan: int = 0,
               exclude: Optional["ExclusionLists"] = None, item_row_begin: int = 0):
    """tf.nn.top_k over a device score matrix [B, N] (K <= TOPK_MAX_K; above
    64 entries the wide select, which no plan bit changes); ``plan``
    PLAN_ONE_WAVE keeps one wave per query.  The rows may be a column slice of
    a wider matrix (unit column stride, leading dimension >= N).  ``exclude``:
    :class:`ExclusionLists` of table rows per matrix row, column i being table
    row ``item_row_begin + i`` — the top K of the other columns
    (hhfm_topk_dense_excl; the matrix is not written)."""
    if scores.dtype != torch.float32 or scores.dim() != 2:
        raise TypeError("scores must be float32 [B, N]")
    B, N = scores.shape
    K = _check_topk_k(K)
    if not scores.is_cuda:
        raise ValueError("hhfm_amd kernels take device (cuda/HIP) tensors")
    if N > 1 and scores.stride(1) != 1 or B > 1 and scores.stride(0) < N:
        raise ValueError("scores must have unit column stride and a leading dimension >= N")
    top_s = torch.empty(B, K, dtype=torch.float32, device=scores.device)
    top_i = torch.empty(B, K, dtype=torch.int32, device=scores.device)
    args = (scores.data_ptr(), B, N, scores.stride(0) if B > 1 else N, K, global_item_base,
            top_s.data_ptr(), top_i.data_ptr(), int(plan), _stream(scores.device))
    if exclude is not None:
        native().topk_dense_excl(*args, int(item_row_begin),
                                 *_excl_args(exclude, B, scores.device))
    else:
        native().topk_dense(*args)
    return top_s, top_i


# ---------------------------------------------------------------------------
# AFM (K4)
# ---------------------------------------------------------------------------
def afm_forward(idx: torch.Tensor, E: torch.Tensor, w: torch.Tensor, w0: float,
                Wt: torch.Tensor, att_b: torch.Tensor, att_p: torch.Tensor, P: torch.Tensor,
                out: Optional[torch.Tensor] = None, plan: int = 0) -> torch.Tensor:
    """AFM.out (AFM.py:103-142) for rows ``idx`` [B, F] -> float32 [B].
    ``Wt`` is attention_W transposed, [A, k] float32; ``plan`` PLAN_EXACT_FP32
    keeps the contraction on exact-fp32 MFMA."""
    _idx(idx, "idx")
    dev = _need_cuda(idx, E, w, Wt, att_b, att_p, P)
    B, F = idx.shape
    M, k = E.shape
    A = Wt.shape[0]
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    nat = native()
    ws = _workspace(dev, nat.afm_forward_workspace(B, F, A))
    nat.afm_forward(idx.data_ptr(), B, F, E.data_ptr(), M, k, _dtype_code(E), w.data_ptr(),
                    float(w0), Wt.data_ptr(), att_b.data_ptr(), att_p.data_ptr(), A, P.data_ptr(),
                    out.data_ptr(), int(plan), ws.data_ptr(), ws.numel(), _stream(dev))
    return out


def afm_catalog_topk(qidx: torch.Tensor, E: torch.Tensor, w: torch.Tensor, Wt: torch.Tensor,
                     att_b: torch.Tensor, att_p: torch.Tensor, P: torch.Tensor,
                     item_row_begin: int, item_count: int, K: int, global_item_base: int = 0,
                     max_cols: int = 1 << 17, plan: int = 0,
                     exclude: Optional["ExclusionLists"] = None):
    """AFM.topk (AFM.py:209-246) -> (scores [B,K], ids [B,K]); ``plan``:
    PLAN_EXACT_FP32, _PER_FIELD, _GEMM.  ``exclude``: :class:`ExclusionLists`
    of table rows per query (hhfm_afm_catalog_topk_excl)."""
    _idx(qidx, "qidx")
    dev = _need_cuda(qidx, E, w, Wt, att_b, att_p, P)
    B, F = qidx.shape
    M, k = E.shape
    A = Wt.shape[0]
    K = _check_topk_k(K)
    nat = native()
    ws = _workspace(dev, nat.afm_catalog_topk_workspace(B, F, k, A, item_count, max_cols,
                                                        int(plan)))
    top_s = torch.empty(B, K, dtype=torch.float32, device=dev)
    top_i = torch.empty(B, K, dtype=torch.int32, device=dev)
    args = (qidx.data_ptr(), B, F, E.data_ptr(), M, k, _dtype_code(E), w.data_ptr(),
            Wt.data_ptr(), att_b.data_ptr(), att_p.data_ptr(), A, P.data_ptr(), item_row_begin,
            item_count, global_item_base, K, max_cols, top_s.data_ptr(), top_i.data_ptr(),
            int(plan), ws.data_ptr(), ws.numel(), _stream(dev))
    if exclude is not None:
        nat.afm_catalog_topk_excl(*args, *_excl_args(exclude, B, dev))
    else:
        nat.afm_catalog_topk(*args)
    return top_s, top_i


def afm_noatt_catalog_topk(qidx: torch.Tensor, E: torch.Tensor, w: Optional[torch.Tensor],
                           w0: float, P: torch.Tensor, item_row_begin: int, item_count: int,
                           K: int, global_item_base: int = 0,
                           status: Optional[torch.Tensor] = None, plan: int = 0,
                           exclude: Optional["ExclusionLists"] = None):
    """AFM.topk with attention=0 (include/hhfm.h "AFM without attention") ->
    (scores [B,K], ids [B,K]): the score of item i is ``out`` of the query row
    with column 1 replaced by i — this library's definition, the reference's
    topk raises KeyError here.  ``plan`` as in :func:`catalog_topk`.
    ``exclude``: :class:`ExclusionLists` of table rows per query
    (hhfm_afm_noatt_catalog_topk_excl)."""
    _idx(qidx, "qidx")
    dev = _need_cuda(qidx, E, w, P)
    B, F = qidx.shape
    M, k = E.shape
    if P.dtype != torch.float32 or P.numel() != k:
        raise ValueError("P must be float32 with k entries")
    if w is not None and (w.dtype != torch.float32 or w.numel() != M):
        raise ValueError("w must be float32 with features_M entries")
    nat = native()
    st = _stream(dev)
    ws = _catalog_workspace(dev, st, _catalog_ws_bytes(nat, B, item_count, k, K))
    top_s = torch.empty(B, K, dtype=torch.float32, device=dev)
    top_i = torch.empty(B, K, dtype=torch.int32, device=dev)
    args = (qidx.data_ptr(), B, F, E.data_ptr(), M, k, _dtype_code(E),
            0 if w is None else w.data_ptr(), float(w0), P.data_ptr(), item_row_begin,
            item_count, global_item_base, K, top_s.data_ptr(), top_i.data_ptr(), ws.data_ptr(),
            ws.numel(), int(plan), _status_ptr(status), st)
    if exclude is not None:
        nat.afm_noatt_catalog_topk_excl(*args, *_excl_args(exclude, B, dev))
    else:
        nat.afm_noatt_catalog_topk(*args)
    return top_s, top_i


# ---- H5 / H3: harness membership test and metric walk ------------------------
def pf_contains(keys: torch.Tensor, codes: torch.Tensor, rows: torch.Tensor, item_col: int,
                cand: Optional[torch.Tensor] = None) -> torch.Tensor:
    """positive_feedback membership on the device (hhfm_pf_contains).

    keys int32 [nkeys, ncols-1] (sorted, distinct), codes int64 (sorted),
    rows int32 [B, ncols]; cand int32 [B, num] -> uint8 [B, num], or the
    rows' own items (cand None) -> uint8 [B]."""
    _need_cuda(keys, codes, rows, cand)
    if keys.dtype != torch.int32 or codes.dtype != torch.int64 or rows.dtype != torch.int32:
        raise TypeError("keys int32, codes int64, rows int32")
    B, ncols = rows.shape
    num = 1 if cand is None else cand.shape[1]
    if cand is not None and (cand.dtype != torch.int32 or cand.shape[0] != B):
        raise ValueError("cand must be int32 [B, num]")
    out = torch.empty(B, num, dtype=torch.uint8, device=rows.device)
    native().pf_contains(keys.data_ptr(), keys.shape[0], ncols - 1, codes.data_ptr(),
                         codes.numel(), rows.data_ptr(), B, ncols, item_col,
                         0 if cand is None else cand.data_ptr(), num, out.data_ptr(),
                         _stream(rows.device))
    return out if cand is not None else out[:, 0]


class ExclusionLists:
    """Per-query lists of table rows a catalog top-K leaves out (include/hhfm.h
    "Exclusion lists"): ``ptr`` int64 [B + 1] and ``rows`` int32 [ptr[B]]
    device tensors (ascending within a query), ``max_len`` the longest list."""

    def __init__(self, ptr: torch.Tensor, rows: torch.Tensor, max_len: int):
        if ptr.dtype != torch.int64 or rows.dtype != torch.int32:
            raise TypeError("ptr int64, rows int32")
        self.ptr = ptr
        self.rows = rows
        self.max_len = int(max_len)

    def __len__(self):
        return self.ptr.numel() - 1


def pf_exclusion_lists(keys: torch.Tensor, codes: torch.Tensor, rows: torch.Tensor,
                       item_col: int, keep_own: bool = False) -> ExclusionLists:
    """The positive_feedback items of every row's key as :class:`ExclusionLists`
    (hhfm_pf_exclusion_lists; keys / codes / rows as in :func:`pf_contains`).
    ``keep_own`` leaves a row's own item out of its list.  Two calls — sizes,
    then the lists; the read of ``ptr[B]`` in between synchronises."""
    dev = _need_cuda(keys, codes, rows)
    if keys.dtype != torch.int32 or codes.dtype != torch.int64 or rows.dtype != torch.int32:
        raise TypeError("keys int32, codes int64, rows int32")
    B, ncols = rows.shape
    nat = native()
    st = _stream(dev)
    ws = _workspace(dev, nat.pf_exclusion_lists_workspace(B))
    ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
    args = (keys.data_ptr() if keys.numel() else 0, keys.shape[0], ncols - 1,
            codes.data_ptr() if codes.numel() else 0, codes.numel(),
            rows.data_ptr() if B else 0, B, ncols, item_col, int(bool(keep_own)), ptr.data_ptr())
    nat.pf_exclusion_lists(*args, 0, 0, ws.data_ptr(), ws.numel(), st)
    host = ptr.cpu()
    total = int(host[B])
    out = torch.empty(total, dtype=torch.int32, device=dev)
    if total:
        nat.pf_exclusion_lists(*args, out.data_ptr(), total, ws.data_ptr(), ws.numel(), st)
    max_len = int((host[1:] - host[:-1]).max()) if B else 0
    return ExclusionLists(ptr, out, max_len)


def exclusion_lists(seqs: Sequence, device) -> ExclusionLists:
    """:class:`ExclusionLists` of B host sequences of table-row ids: each is
    sorted, freed of duplicates and uploaded."""
    import numpy as np
    lists = [np.unique(np.asarray(list(s), dtype=np.int64)) for s in seqs]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    if lists:
        np.cumsum([len(x) for x in lists], out=ptr[1:])
    flat = np.concatenate(lists) if lists else np.zeros(0, np.int64)
    if flat.size and (flat.min() < -2 ** 31 or flat.max() >= 2 ** 31):
        raise ValueError("exclusion ids must fit int32")
    dev = torch.device(device)
    return ExclusionLists(torch.from_numpy(ptr).to(dev),
                          torch.from_numpy(flat.astype(np.int32)).to(dev),
                          max((len(x) for x in lists), default=0))


def topk_walk(pred: torch.Tensor, target: torch.Tensor, positive: torch.Tensor,
              TopK: int) -> torch.Tensor:
    """evaluate_TopK's walk (hhfm_topk_walk): int32 [B] outcomes, n >= 0 hit
    at walk position n, -1 miss (zeros appended), -2 nothing appended."""
    _need_cuda(pred, target, positive)
    if pred.dtype != torch.int32 or target.dtype != torch.int32 or positive.dtype != torch.uint8:
        raise TypeError("pred/target int32, positive uint8")
    B, P = pred.shape
    out = torch.empty(B, dtype=torch.int32, device=pred.device)
    native().topk_walk(pred.data_ptr(), B, P, target.data_ptr(), positive.data_ptr(), TopK,
                       out.data_ptr(), _stream(pred.device))
    return out
