"""Wide K (include/hhfm.h "Wide K") without a GPU: the numpy restatement against
brute force, the host merge at wide K, the wide workspace query and the order
of the catalog entry points' return codes (every call below returns before the
first launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import topk_wide_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hhfm_amd", "lib", "libhhfm.so")
_vp, _i32, _i64, _f32, _sz = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float,
                              ctypes.c_size_t)
_D = 0x1000            # a non-null, 16-byte aligned pointer that is never dereferenced
OK, EINVAL, EUNSUPPORTED, EWORKSPACE = 0, -1, -2, -3


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def _brute(row, K):
    """Selection by repeated maximum: the first index of the largest remaining score."""
    row = np.asarray(row, np.float64).copy()
    out = []
    for _ in range(K):
        j = int(np.argmax(row))          # argmax returns the first of equal maxima
        out.append(j)
        row[j] = -np.inf
    return out


@pytest.mark.parametrize("kind", ["random", "ties", "all_equal", "ascending"])
def test_restatement_matches_brute_force(kind):
    rng = np.random.default_rng(3)
    B, N, K = 3, 700, 130
    if kind == "random":
        sc = rng.normal(size=(B, N)).astype(np.float32)
    elif kind == "ties":
        sc = rng.integers(0, 9, size=(B, N)).astype(np.float32)
    elif kind == "all_equal":
        sc = np.full((B, N), 2.5, np.float32)
    else:
        sc = np.tile(np.arange(N, dtype=np.float32), (B, 1))
    s, i = wr.topk(sc, K, base=11)
    for b in range(B):
        want = _brute(sc[b], K)
        assert i[b].tolist() == [11 + j for j in want]
        assert np.array_equal(s[b], sc[b][want])


@pytest.mark.parametrize("block", [64, 100, 699, 700, 5000])
def test_blockwise_equals_one_shot(block):
    rng = np.random.default_rng(4)
    sc = rng.integers(0, 40, size=(4, 700)).astype(np.float32)      # ties across block edges
    for K in (65, 130, 700):
        a = wr.topk(sc, K, base=5)
        b = wr.blockwise(sc, K, base=5, block=block)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])


def test_prefix_property():
    rng = np.random.default_rng(5)
    sc = rng.integers(0, 30, size=(3, 2000)).astype(np.float32)
    s, i = wr.topk(sc, 1024)
    for K in (1, 64, 65, 1000):
        s2, i2 = wr.topk(sc, K)
        assert np.array_equal(i2, i[:, :K]) and np.array_equal(s2, s[:, :K])


def test_admissible_restatement():
    sc = np.tile(np.arange(200, dtype=np.float32), (2, 1))
    s, i = wr.topk_admissible(sc, 70, [{199, 198, 0}, set()], base=3)
    assert i[0].tolist() == [3 + c for c in range(197, 127, -1)]
    assert i[1].tolist() == [3 + c for c in range(199, 129, -1)]


# ---------------------------------------------------------------------------
# hhfm_topk_merge_host at wide K
# ---------------------------------------------------------------------------
def sharded_lists(rng, R, B, K, levels=50, pad_from=None):
    """R sorted lists [R, B, K] with distinct ids and equal scores across lists;
    ``pad_from``: list R - 1 keeps that many entries, the rest (-inf, NO_IDX)."""
    sc = rng.integers(0, levels, size=(R, B, K)).astype(np.float32)
    ids = np.stack([rng.permutation(R * K * 3)[:R * K] for _ in range(B)])     # [B, R K]
    ids = ids.reshape(B, R, K).transpose(1, 0, 2).astype(np.int64)
    order = np.lexsort((ids, -sc.astype(np.float64)), axis=2)
    sc = np.take_along_axis(sc, order, 2)
    ids = np.take_along_axis(ids, order, 2)
    if pad_from is not None:
        sc[R - 1, :, pad_from:] = -np.inf
        ids[R - 1, :, pad_from:] = wr.NO_IDX
    return sc, ids.astype(np.int32)


@pytest.mark.parametrize("K", [65, 128, 1000, 1024])
@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_host_merge_wide(K, R):
    from hhfm_amd import ops
    rng = np.random.default_rng(100 * R + K)
    for pad in (None, K // 3):
        sc, ids = sharded_lists(rng, R, 3, K, pad_from=pad)
        s, i = ops.topk_merge(torch.from_numpy(sc), torch.from_numpy(ids))
        ws, wi = wr.merge(sc, ids)
        assert np.array_equal(i.numpy(), wi)
        assert np.array_equal(s.numpy().view(np.int32), ws.view(np.int32))


# ---------------------------------------------------------------------------
# hhfm_catalog_topk_wide_workspace (host only)
# ---------------------------------------------------------------------------
def _lib():
    lib = ctypes.CDLL(LIB)
    for n in ("hhfm_catalog_topk_wide_workspace", "hhfm_catalog_topk_workspace"):
        getattr(lib, n).argtypes = [_i64, _i32, _i32, _i32, ctypes.POINTER(_sz)]
    return lib


def _query(lib, name, B, N, k, K):
    ws = _sz(0)
    rc = getattr(lib, name)(B, N, k, K, ctypes.byref(ws))
    return rc, ws.value


SHAPES = [(1, 300), (300, 4082), (33, 16384), (33, 16385), (1024, 70000), (5000, 16000),
          (100000, 4082)]


def test_wide_workspace_argument_errors():
    lib = _lib()
    f = lib.hhfm_catalog_topk_wide_workspace
    ws = _sz(0)
    assert f(10, 100, 64, 65, None) == EINVAL
    for B, N, k, K in [(-1, 100, 64, 65), (10, 0, 64, 65), (10, 100, 0, 65), (10, 100, 64, 0),
                       (10, 100, 64, 1025), (10, 100, 64, -3)]:
        assert f(B, N, k, K, ctypes.byref(ws)) == EINVAL, (B, N, k, K)
    assert f(10, 100, 64, 1024, ctypes.byref(ws)) == OK and ws.value > 0
    assert f(0, 100, 64, 1024, ctypes.byref(ws)) == OK and ws.value == 0
    # the narrow query keeps refusing K > 64 (tests/test_capi.py pins it too)
    assert _query(lib, "hhfm_catalog_topk_workspace", 10, 100, 64, 65)[0] == EINVAL
    assert _query(lib, "hhfm_catalog_topk_workspace", 10, 100, 64, 64)[0] == OK


@pytest.mark.parametrize("B,N", SHAPES)
def test_wide_workspace_sizes(B, N):
    lib = _lib()
    for k in (16, 128):
        prev = 0
        for K in (1, 20, 32, 33, 64, 65, 100, 128, 129, 256, 1000, 1024):
            rc, wide = _query(lib, "hhfm_catalog_topk_wide_workspace", B, N, k, K)
            assert rc == OK
            if K <= 64:        # where both are defined: never less than the narrow query
                assert wide >= _query(lib, "hhfm_catalog_topk_workspace", B, N, k, K)[1]
            else:              # ... nor than the largest narrow one of these sizes
                assert wide >= _query(lib, "hhfm_catalog_topk_workspace", B, N, k, 64)[1]
            assert wide >= prev, (k, K)                    # monotone in K
            prev = wide


@pytest.mark.parametrize("B", [1, 7, 33, 129, 300, 1024, 5000, 100000])
def test_wide_workspace_covers_the_narrow_query_at_every_size(B):
    """The wide answer does not depend on item_count beyond 16,384 and must
    still cover the K = 64 narrow query there: a sweep over catalog sizes, the
    ones at which the split counts and the seed of the narrow plan change
    among them."""
    lib = _lib()
    rng = np.random.default_rng(B)
    sizes = [16385, 16416, 20000, 65535, 65536, 65537, 66048, 131072, 262144, 262145, 1 << 20,
             1_250_000, 10_000_000, (1 << 30), (1 << 31) - 1]
    sizes += [int(n) for n in rng.integers(16385, 3_000_000, 150)]
    for k in (8, 16, 128, 256):
        wide = _query(lib, "hhfm_catalog_topk_wide_workspace", B, 16385, k, 65)[1]
        for N in sizes:
            rc, narrow = _query(lib, "hhfm_catalog_topk_workspace", B, N, k, 64)
            assert rc == OK and wide >= narrow, (B, k, N, wide, narrow)


@pytest.mark.parametrize("B", [1, 33, 1024, 100000])
def test_wide_workspace_stops_growing_with_the_catalog(B):
    lib = _lib()
    for k in (16, 128):
        for K in (65, 100, 1024):
            sizes = {_query(lib, "hhfm_catalog_topk_wide_workspace", B, N, k, K)[1]
                     for N in (16385, 20000, 70000, 1_250_000, 50_000_000)}
            assert len(sizes) == 1, (B, k, K, sizes)


# ---------------------------------------------------------------------------
# return codes of the entry points, in order (no device: every call returns
# before its first launch)
# ---------------------------------------------------------------------------
_CAT = [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _i32,
        _i32, _i32, _i32, _vp, _vp, _vp, _sz]          # ... K, top_score, top_idx, ws, ws_bytes


def _catalog_calls(lib):
    """name -> f(B, N, k, K, ws_bytes) for every form of hhfm_catalog_topk."""
    def head(B, N, k, K, nbytes):
        return [_D, B, 4, 1, 0, 2, 4, 0, 0, _D, 7 + N + 5, k, 0, None, 7, N, 0, K, _D, _D, _D,
                nbytes]
    forms = {
        "hhfm_catalog_topk": ([_vp], lambda: [None]),
        "hhfm_catalog_topk_ex": ([_i32, _vp, _vp], lambda: [0, None, None]),
        "hhfm_catalog_topk_pool": ([_i32, _i32, _vp, _vp], lambda: [0, 0, None, None]),
        "hhfm_catalog_topk_pool2": ([_i32, _i32, _i32, _vp, _vp], lambda: [0, 0, 0, None, None]),
        "hhfm_catalog_topk_excl": ([_i32, _i32, _vp, _vp, _vp, _vp, _i64],
                                   lambda: [0, 0, None, None, _D, None, 0]),
    }
    out = {}
    for name, (types, tail) in forms.items():
        f = getattr(lib, name)
        f.argtypes = _CAT + types
        out[name] = (lambda f, tail: lambda B, N, k, K, nb: f(*head(B, N, k, K, nb), *tail()))(f, tail)
    c2 = lib.hhfm_cars2_catalog_topk
    c2.argtypes = [_vp, _i64, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp,
                   _vp, _sz, _i32, _vp, _vp]
    out["hhfm_cars2_catalog_topk"] = lambda B, N, k, K, nb: c2(
        _D, B, _D, 7 + N, k, 0, _D, 5, 7, N, 0, K, _D, _D, _D, nb, 0, None, None)
    na = lib.hhfm_afm_noatt_catalog_topk
    na.argtypes = [_vp, _i64, _i32, _vp, _i64, _i32, _i32, _vp, _f32, _vp, _i32, _i32, _i32, _i32,
                   _vp, _vp, _vp, _sz, _i32, _vp, _vp]
    out["hhfm_afm_noatt_catalog_topk"] = lambda B, N, k, K, nb: na(
        _D, B, 4, _D, 7 + N + 5, k, 0, _D, 0.0, _D, 7, N, 0, K, _D, _D, _D, nb, 0, None, None)
    return out


def test_catalog_return_code_order():
    lib = _lib()
    B, N, k = 33, 70000, 16
    narrow = _query(lib, "hhfm_catalog_topk_workspace", B, N, k, 64)[1]
    wide = _query(lib, "hhfm_catalog_topk_wide_workspace", B, N, k, 65)[1]
    assert wide > narrow                # at this size a narrow buffer cannot hold a score block
    for name, call in _catalog_calls(lib).items():
        assert call(B, N, k, 1025, 1 << 40) == EUNSUPPORTED, name      # above HHFM_TOPK_MAX_K
        assert call(B, 500, k, 501, 1 << 40) == EINVAL, name            # K > item_count
        assert call(B, 500, k, 1025, 1 << 40) == EINVAL, name           # ... is checked first
        assert call(B, N, k, 65, narrow) == EWORKSPACE, name            # a narrow-sized buffer
        assert call(B, N, k, 65, wide - 1) == EWORKSPACE, name
        assert call(0, N, k, 65, 0) == OK, name                         # no queries: nothing to do


def test_afm_and_dfm_return_code_order():
    """hhfm_afm_catalog_topk*, hhfm_dfm_catalog_topk* and _head: K > item_count
    is EINVAL before K > HHFM_TOPK_MAX_K is EUNSUPPORTED, and a wide K passes
    both checks (no queries: nothing to do)."""
    lib = _lib()
    N, k, M = 2000, 16, 7 + 2000 + 5
    afm_t = [_vp, _i64, _i32, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32,
             _i32, _i32, _i64, _vp, _vp]

    def afm_args(B, n, K):
        return [_D, B, 5, _D, M, k, 0, _D, _D, _D, _D, 16, _D, 7, n, 0, K, 1 << 17, _D, _D]
    a0, a1 = lib.hhfm_afm_catalog_topk, lib.hhfm_afm_catalog_topk_ex
    a0.argtypes = afm_t + [_vp, _sz, _vp]
    a1.argtypes = afm_t + [_i32, _vp, _sz, _vp]
    ax = lib.hhfm_afm_catalog_topk_excl
    ax.argtypes = afm_t + [_i32, _vp, _sz, _vp, _vp, _vp, _i64]
    dims = (_i32 * 2)(24, 40)
    two = (_vp * 2)(_D, _D)
    dfm_t = [_vp, _i64, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp,
             _f32, _i32, _i32, _i32, _i32, _i64, _vp, _vp]

    def dfm_args(B, n, K):
        return [_D, B, 5, 1, _D, M, k, 0, _D, 2, dims, two, two, 0, _D, 0.0, 7, n, 0, K, 1 << 20,
                _D, _D]
    d0, d1, dh = lib.hhfm_dfm_catalog_topk, lib.hhfm_dfm_catalog_topk_ex, lib.hhfm_dfm_catalog_topk_head
    d0.argtypes = dfm_t + [_vp, _sz, _vp]
    d1.argtypes = dfm_t + [_i32, _i32, _vp, _sz, _vp]
    dh.argtypes = dfm_t + [_i32, _i32, _vp, _sz, _vp, _i32]
    dx = lib.hhfm_dfm_catalog_topk_excl
    dx.argtypes = dfm_t + [_i32, _i32, _vp, _sz, _vp, _i32, _vp, _vp, _i64]
    big = 1 << 40
    calls = {
        "afm": lambda B, n, K: a0(*afm_args(B, n, K), _D, big, None),
        "afm_ex": lambda B, n, K: a1(*afm_args(B, n, K), 0, _D, big, None),
        "afm_excl": lambda B, n, K: ax(*afm_args(B, n, K), 0, _D, big, None, _D, None, 0),
        "dfm": lambda B, n, K: d0(*dfm_args(B, n, K), _D, big, None),
        "dfm_ex": lambda B, n, K: d1(*dfm_args(B, n, K), 0, 0, _D, big, None),
        "dfm_excl": lambda B, n, K: dx(*dfm_args(B, n, K), 0, 0, _D, big, None, 3, _D, None, 0),
    }
    for head in range(1, 8):
        if head & 3:            # HHFM_DFM_HEAD_FM | _DEEP | _SIGMOID: every head that scores
            calls[f"dfm_head{head}"] = (lambda h: lambda B, n, K: dh(
                *dfm_args(B, n, K), 0, 0, _D, big, None, h))(head)
    for name, call in calls.items():
        assert call(4, N, 1025) == EUNSUPPORTED, name
        assert call(4, 500, 501) == EINVAL, name
        assert call(4, 500, 1025) == EINVAL, name
        assert call(0, N, 1024) == OK, name
        assert call(0, N, 65) == OK, name


def test_dense_and_merge_return_codes():
    lib = _lib()
    d = lib.hhfm_topk_dense
    d.argtypes = [_vp, _i64, _i32, _i64, _i32, _i32, _vp, _vp, _vp]
    assert d(_D, 4, 2000, 2000, 1025, 0, _D, _D, None) == EUNSUPPORTED
    assert d(_D, 4, 100, 100, 101, 0, _D, _D, None) == EINVAL
    assert d(_D, 0, 2000, 2000, 1024, 0, _D, _D, None) == OK
    dx = lib.hhfm_topk_dense_ex
    dx.argtypes = [_vp, _i64, _i32, _i64, _i32, _i32, _vp, _vp, _i32, _vp]
    assert dx(_D, 4, 2000, 2000, 1025, 0, _D, _D, 0, None) == EUNSUPPORTED
    assert dx(_D, 0, 2000, 2000, 100, 0, _D, _D, 0, None) == OK
    de = lib.hhfm_topk_dense_excl
    de.argtypes = [_vp, _i64, _i32, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _i64]
    assert de(_D, 4, 2000, 2000, 1025, 0, _D, _D, 0, None, 0, _D, None, 0) == EUNSUPPORTED
    assert de(_D, 4, 2000, 2000, 1000, 0, _D, _D, 0, None, 0, _D, None, 1001) == EINVAL
    m = lib.hhfm_topk_merge
    m.argtypes = [_vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp]
    assert m(_D, _D, 8, 4, 1025, _D, _D, None) == EUNSUPPORTED
    assert m(_D, _D, 8, 0, 1024, _D, _D, None) == OK
    assert m(None, _D, 8, 4, 1024, _D, _D, None) == EINVAL


def test_python_refuses_k_above_the_maximum():
    from hhfm_amd import ops
    assert ops.TOPK_MAX_K == 1024
    with pytest.raises(ValueError, match="TOPK_MAX_K"):
        ops._check_topk_k(1025)
    with pytest.raises(ValueError, match="TOPK_MAX_K"):
        ops._check_topk_k(0)
    assert ops._check_topk_k(1024) == 1024
