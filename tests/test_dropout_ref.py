"""tests/dropout_ref.py on the CPU: the Philox generator against its known
answers, the mask's kept share, the masked float64 references against central
differences of an independently written float64 loss and (with masks of ones)
against the undropped references, the input conditions of
tests/test_gpu_dropout.py, and the new C-ABI entry points' argument checks
(every call returns before the first launch: no device needed).

fp32 restatement of the masked FM step, err / bound (tests/train_ref.ratio) on
train_ref.FM_CASES at keep 0.5 / 0.7 / 0.9, seed 2016 | 7 << 32: worst 0.044
(F2 at 0.5), every other case <= 0.017; the k = 260 case 0.054 – 0.061."""
import ctypes
import os

import numpy as np
import pytest

from oracle import fm_oracle as orc
from tests import dropout_ref as dr
from tests import train_ref as tr

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hhfm_amd", "lib",
                   "libhhfm.so")


# ---------------------------------------------------------------------------
# generator and mask
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, out):
    got = dr.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
    assert " ".join(f"{int(x):08x}" for x in got) == out


def test_counter_layout():
    """Element e reads word (e >> 6) & 3 of the block with counter
    ((e & 63) | ((e >> 8) << 6), row low, row high, site)."""
    seed, site, rows, n = 0x0123456789abcdef, 2, 3, 300
    w = dr.words(seed, site, rows, n)
    key = np.array([seed & 0xffffffff, seed >> 32], np.uint32)
    for r, e in [(0, 0), (1, 63), (2, 64), (0, 255), (1, 256), (2, 299)]:
        blk = dr.philox4x32_10(np.array([(e & 63) | ((e >> 8) << 6), r, 0, site], np.uint32), key)
        assert w[r, e] == blk[(e >> 6) & 3], (r, e)
    # lanes l, l + 64, l + 128, l + 192 share one block; element 256 starts the next
    assert len({(e & 63) | ((e >> 8) << 6) for e in (5, 69, 133, 197)}) == 1
    assert w[0, 0] != w[0, 256]


@pytest.mark.parametrize("keep", [0.3, 0.5, 0.9])
def test_binary_kept_share(keep):
    rows, n = 4000, 250                                  # 10^6 elements
    b = dr.binary(2016 | 3 << 32, dr.SITE_FM, rows, n, keep)
    assert b.dtype == np.float32 and np.isin(b, [0.0, 1.0]).all()
    sigma = np.sqrt(keep * (1 - keep) / b.size)
    assert abs(b.mean() - keep) <= 4 * sigma
    assert dr.binary(5, dr.SITE_FM, 4, 300, 1.0).min() == 1.0     # keep = 1 keeps everything
    # rows, sites and seeds are distinct streams
    a = dr.binary(1, 0, 2, 256, 0.5)
    assert not np.array_equal(a[0], a[1])
    assert not np.array_equal(a, dr.binary(1, 1, 2, 256, 0.5))
    assert not np.array_equal(a, dr.binary(1 | 1 << 32, 0, 2, 256, 0.5))


def test_model_seed():
    assert dr.model_seed(2016, 0) == 2016 and dr.model_seed(2016, 7) == dr.FM_SEED
    assert dr.model_seed(-1, 1) == 0xffffffff | 1 << 32


# ---------------------------------------------------------------------------
# the masked references
# ---------------------------------------------------------------------------
def _fd(loss, arr, i, eps=1e-6):
    a = np.array(arr, np.float64)
    a[i] += eps
    lp = loss(a)
    a[i] -= 2 * eps
    return (lp - loss(a)) / (2 * eps)


def test_fm_reference_with_ones_is_the_undropped_reference():
    X, y, E, w, w0 = tr.fm_case("k20")
    ones = np.ones((len(X), E.shape[1]), np.float32)
    l0, g0, m0 = tr.fm_grad64(X, y, E, w, w0)
    l1, g1, m1 = dr.fm_grad64_dropout(X, y, E, w, w0, ones, 1.0)
    assert l0 == l1
    for a, b in zip(g0 + m0, g1 + m1):
        assert np.array_equal(a, b)


def test_fm_reference_matches_finite_differences():
    rng = np.random.default_rng(0)
    M, k, B, F, keep = 30, 6, 20, 5, 0.7
    X = rng.integers(0, M, (B, F))
    X[0, 3] = X[0, 2]
    y = rng.integers(0, 2, B).astype(np.float64)
    E, w, w0 = rng.normal(0, 0.3, (M, k)), rng.normal(0, 0.3, M), 0.05
    bn = dr.binary(11, dr.SITE_FM, B, k, keep)
    assert 0 < bn.mean() < 1
    m = bn.astype(np.float64) / np.float64(np.float32(keep))

    def loss(E, w, w0):
        e = E[X]
        s = e.sum(1)
        out = (0.5 * (s * s - (e * e).sum(1)) * m).sum(1) + w[X].sum(1) + w0
        return ((y - out) ** 2).sum() / 2

    l0, (dE, dw, dw0), (mE, mw, mw0) = dr.fm_grad64_dropout(X, y, E, w, w0, bn, keep)
    assert np.isclose(l0, loss(E, w, w0), rtol=1e-13)
    for i in [(X[0, 2], 1), (X[1, 0], 3), (X[3, 0], 0), (X[5, 4], 5)]:
        assert np.isclose(dE[i], _fd(lambda a: loss(a, w, w0), E, i), rtol=1e-6, atol=1e-8), i
    assert np.isclose(dw[X[7, 1]], _fd(lambda a: loss(E, a, w0), w, (X[7, 1],)), rtol=1e-7)
    assert np.isclose(dw0, _fd(lambda a: loss(E, w, a[0]), [w0], (0,)), rtol=1e-7)
    # a column dropped in every row that holds the id has no gradient there
    dropped = bn[0] == 0
    only0 = np.setdiff1d(X[0], X[1:])
    assert dropped.any() and (len(only0) == 0 or np.all(dE[only0][:, dropped] == 0))
    assert np.all(mE >= np.abs(dE)) and np.all(mw >= np.abs(dw)) and mw0 >= abs(dw0)


def _afm_loss64(X, y, params, m1, m2):
    E, w, w0, W, b, pvec, P = params
    e = E[X]
    F = X.shape[1]
    out = np.zeros(len(X))
    for r in range(len(X)):
        prs = [e[r, i] * e[r, j] for i in range(F) for j in range(i + 1, F)]
        lg = np.array([np.maximum(p @ W + b, 0) @ pvec for p in prs])
        a = np.exp(lg - lg.max())
        a = a / a.sum() * m1[r]
        afm = sum(ai * p for ai, p in zip(a, prs)) * m2[r]
        out[r] = afm @ P + w[X[r]].sum() + w0
    return ((y - out) ** 2).sum() / 2


def test_afm_reference_matches_finite_differences():
    rng = np.random.default_rng(2)
    F, k, A, B, keep = 4, 6, 5, 6, (0.7, 0.6)
    M = 12
    X = rng.integers(0, M, (B, F))
    y = rng.choice([1.0, -1.0], B)
    par = [rng.normal(0, 0.5, (M, k)), rng.normal(0, 0.3, M), np.float64(0.05),
           rng.normal(0, 0.5, (k, A)), rng.normal(0, 0.3, A), rng.normal(0, 1, A),
           rng.normal(1, 0.2, k)]
    b1 = dr.binary(21, dr.SITE_AFM_ATT, B, F * (F - 1) // 2, keep[0])
    b2 = dr.binary(21, dr.SITE_AFM_VEC, B, k, keep[1])
    assert 0 < b1.mean() < 1 and 0 < b2.mean() < 1
    m1 = b1 / np.float64(np.float32(keep[0]))
    m2 = b2 / np.float64(np.float32(keep[1]))
    assert dr.afm_relu_margin(X, par[0], par[3], par[4]).min() > 1e-4     # no kink within h
    l0, grads = dr.afm_grad64_dropout(X, y, par, b1, b2, keep)

    def loss_with(n, a):
        q = list(par)
        q[n] = a.reshape(np.shape(par[n]))
        return _afm_loss64(X, y, q, m1, m2)

    assert np.isclose(l0, _afm_loss64(X, y, par, m1, m2), rtol=1e-13)
    picks = {0: [(X[0, 0], 1), (X[2, 3], 4), (X[5, 1], 0)], 1: [(X[1, 2],)], 2: [()],
             3: [(0, 0), (5, 4), (2, 3)], 4: [(0,), (4,)], 5: [(1,), (3,)], 6: [(0,), (5,)]}
    for n, idxs in picks.items():
        for i in idxs:
            fd = _fd(lambda a: loss_with(n, a), np.reshape(par[n], np.shape(grads[n])), i)
            assert np.isclose(np.asarray(grads[n])[i], fd, rtol=2e-5, atol=1e-8), (n, i)


@pytest.mark.parametrize("shape", [(3, 8, 8, 1), (5, 16, 16, 5), (16, 8, 8, 3)])
def test_afm_reference_with_ones_is_the_oracle_gradient(shape):
    """Masks of ones: the SGD step (lr 1, λ 0) of oracle.fm_oracle.afm_train_step
    moves every variable by the reference's gradient (fp32 against float64)."""
    F, k, A, B = shape
    X, y, par = dr.afm_case(shape)
    loss, grads = dr.afm_grad64_dropout(X, y, par, np.ones((B, F * (F - 1) // 2)),
                                        np.ones((B, k)), (1.0, 1.0))
    rl, *new, _ = orc.afm_train_step(X, y, *par, {}, 1.0, 0.0, optimizer="sgd")
    assert np.isclose(loss, rl, rtol=1e-5)
    for old, nv, g in zip(par, new, grads):
        d = np.asarray(old, np.float64) - np.asarray(nv, np.float64).reshape(np.shape(old))
        assert np.allclose(d, g, rtol=1e-4, atol=1e-5 * np.abs(g).max() + 1e-9)


@pytest.mark.parametrize("shape", dr.AFM_SHAPES)
def test_afm_inputs_keep_relu_decided(shape):
    """Every pre-activation of every seeded AFM case lies further from 0 than
    fp32 can move it (dropout_ref.afm_margin_needed), and both signs occur."""
    X, y, (E, w, w0, W, b, pvec, P) = dr.afm_case(shape)
    assert X.shape == (shape[3], shape[0]) and X.max() < E.shape[0]
    assert dr.afm_relu_margin(X, E, W, b).min() >= dr.afm_margin_needed(shape[1])
    z = dr._pairs(E.astype(np.float64)[X]) @ W.astype(np.float64) + b
    assert 0.1 < (z > 0).mean() < 0.9


# ---------------------------------------------------------------------------
# input condition of the GPU test: the fp32 restatement sits inside the bound
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("keep", dr.FM_KEEPS)
@pytest.mark.parametrize("name", sorted(dr.FM_CASES))
def test_fm_inputs_keep_the_fp32_step_inside_the_bound(name, keep):
    X, y, E, w, w0 = dr.fm_case(name)
    bn = dr.binary(dr.FM_SEED, dr.SITE_FM, len(X), E.shape[1], keep)
    _, (dE, dw, dw0), (mE, mw, mw0) = dr.fm_grad64_dropout(X, y, E, w, w0, bn, keep)
    E1, w1, w01 = dr.fm_step32_dropout(X, y, E, w, w0, bn, keep)
    r = max(tr.ratio(E - E1, E, E1, dE, mE), tr.ratio(w - w1, w, w1, dw, mw),
            tr.ratio(w0 - w01, w0, w01, dw0, mw0))
    print(f"fm {name} keep {keep}: fp32 err / bound = {r:.3g}")
    assert r <= 0.25


# ---------------------------------------------------------------------------
# C ABI without a device
# ---------------------------------------------------------------------------
_vp, _i32, _i64, _f32, _u64, _sz = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                    ctypes.c_float, ctypes.c_uint64, ctypes.c_size_t)
_D = 0x1000            # a non-null pointer that is never dereferenced
BAD_KEEPS = (0.0, 1.5, float("nan"), -0.5)


def _lib():
    lib = ctypes.CDLL(LIB)
    lib.hhfm_fm_train_step_ex.argtypes = [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _i32, _f32,
                                          _f32, _i32, _f32, _u64, _vp, _vp, _vp, _vp, _sz, _vp,
                                          _vp]
    lib.hhfm_afm_train_step_ex.argtypes = [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _i32, _i32,
                                           _vp, _vp, _vp, _vp, _f32, _f32, _i32, _f32, _f32, _u64,
                                           _vp, _vp, _sz, _vp, _vp]
    lib.hhfm_dropout_mask.argtypes = [_u64, _i32, _i64, _i32, _f32, _vp, _vp]
    lib.hhfm_train_workspace.restype = _sz
    lib.hhfm_train_workspace.argtypes = [_i64, _i32]
    lib.hhfm_afm_train_workspace.argtypes = [_i64, _i32, _i32, _i32, _i64, ctypes.POINTER(_sz)]
    return lib


def test_new_symbols_are_exported():
    lib = ctypes.CDLL(LIB)
    for n in ("hhfm_fm_train_step_ex", "hhfm_afm_train_step_ex", "hhfm_dropout_mask"):
        assert hasattr(lib, n), n


def test_keep_is_validated_before_anything_is_launched():
    """A keep that is 0, above 1, negative or NaN is HHFM_EINVAL; a valid keep
    below 1 passes every check (the workspace, one byte short, is what is
    refused then), and no call here reaches a launch."""
    lib = _lib()
    B, F, M, k, A = 7, 5, 40, 8, 12
    fm_ws = lib.hhfm_train_workspace(M, k)
    n = _sz(0)
    assert lib.hhfm_afm_train_workspace(B, F, k, A, M, ctypes.byref(n)) == 0
    slots = (_vp * 7)(*[_D] * 7)

    def fm(keep, ws_bytes=fm_ws):
        return lib.hhfm_fm_train_step_ex(_D, _D, B, F, _D, _D, _D, M, k, 0.1, 0.1, 0, keep, 5,
                                         _D, _D, _D, _D, ws_bytes, _D, None)

    def afm(k0, k1, ws_bytes=n.value):
        return lib.hhfm_afm_train_step_ex(_D, _D, B, F, _D, _D, _D, M, k, A, _D, _D, _D, _D,
                                          0.1, 0.1, 0, k0, k1, 5, slots, _D, ws_bytes, _D, None)

    for bad in BAD_KEEPS:
        assert fm(bad) == -1, bad
        assert afm(bad, 1.0) == -1 and afm(1.0, bad) == -1 and afm(0.5, bad) == -1, bad
        assert lib.hhfm_dropout_mask(1, 0, 3, 8, bad, _D, None) == -1, bad
    for good in (0.5, 1.0, 1e-3):
        assert fm(good, fm_ws - 1) == -3
        assert afm(good, 1.0, n.value - 1) == -3 and afm(1.0, good, n.value - 1) == -3


def test_dropout_mask_argument_checks():
    lib = _lib()
    assert lib.hhfm_dropout_mask(1, 0, 0, 8, 0.5, None, None) == 0       # no rows: a no-op
    assert lib.hhfm_dropout_mask(1, 0, 3, 8, 0.5, None, None) == -1      # no output
    assert lib.hhfm_dropout_mask(1, 0, -1, 8, 0.5, _D, None) == -1
    assert lib.hhfm_dropout_mask(1, 0, 3, 0, 0.5, _D, None) == -1
    assert lib.hhfm_dropout_mask(1, -1, 3, 8, 0.5, _D, None) == -1
