"""tests/fm_bn_ref.py on the CPU: the float64 gradients of the batch-norm FM
step against central differences of an independently written float64 loss,
the magnitudes against the fp32 restatement's own error, the designed known
answer's exactness, and the new C-ABI entry points as far as they go without a
device (exports, the workspace size, every argument check: all of them return
before the first launch).

fp32 restatement against float64, err / bound (tests/train_ref.ratio with the
magnitudes of fm_bn_grad64) at B = 257, F = 5, k = 20: E 0.00033, w 0.0009,
w0 0.000054, γ 0.00082, β 0.00041 — every sum of absolute values through the
layer makes the bound roomier than train_ref's (0.0016 – 0.014 there)."""
import ctypes
import os

import numpy as np
import pytest

from tests import dropout_ref as dr
from tests import fm_bn_ref as bn
from tests import train_ref as tr

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hhfm_amd", "lib",
                   "libhhfm.so")


def _case(B=37, F=5, k=6, M=30, seed=11):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    X[1, F - 1] = X[1, 0]                      # an id twice in one row
    E = rng.normal(0, 0.4, (M, k)).astype(np.float32)
    w = rng.normal(0, 0.3, M).astype(np.float32)
    y = rng.integers(0, 2, B).astype(np.float32)
    gamma = rng.normal(1, 0.2, k).astype(np.float32)
    beta = rng.normal(0, 0.2, k).astype(np.float32)
    return X, y, E, w, np.float32(0.02), gamma, beta


def _central(f, x0, h):
    return (f(x0 + h) - f(x0 - h)) / (2 * h)


@pytest.mark.parametrize("keep", [1.0, 0.7])
def test_grad64_matches_central_differences(keep):
    """E, γ and β elements (w and w0 enter the loss only through g): B = 37,
    F = 5, k = 6, with and without the dropout mask."""
    X, y, E, w, w0, gamma, beta = _case()
    bin_ = None if keep == 1.0 else dr.binary(dr.FM_SEED, dr.SITE_FM, X.shape[0], E.shape[1], keep)
    loss, (dE, dw, dw0, dg, db), _, _ = bn.fm_bn_grad64(X, y, E, w, w0, gamma, beta,
                                                        bin_=bin_, keep=keep)
    assert np.isclose(loss, bn.fm_bn_loss64(X, y, E, w, w0, gamma, beta, bin_=bin_, keep=keep),
                      rtol=1e-13)
    E64, g64, b64 = E.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64)
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(40):
        i, c = int(rng.integers(0, E.shape[0])), int(rng.integers(0, E.shape[1]))

        def f(t):
            Et = E64.copy()
            Et[i, c] = t
            return bn.fm_bn_loss64(X, y, Et, w, w0, g64, b64, bin_=bin_, keep=keep)
        fd = _central(f, E64[i, c], 1e-5)
        worst = max(worst, abs(fd - dE[i, c]))
    for c in range(E.shape[1]):
        def fg(t):
            gt = g64.copy()
            gt[c] = t
            return bn.fm_bn_loss64(X, y, E64, w, w0, gt, b64, bin_=bin_, keep=keep)

        def fb(t):
            bt = b64.copy()
            bt[c] = t
            return bn.fm_bn_loss64(X, y, E64, w, w0, g64, bt, bin_=bin_, keep=keep)
        worst = max(worst, abs(_central(fg, g64[c], 1e-5) - dg[c]),
                    abs(_central(fb, b64[c], 1e-5) - db[c]))
    print(f"fm_bn grad64 vs central differences (keep {keep}): {worst:.3g}")
    assert worst <= 1e-6
    # w and w0: dL/dw[i] = Σ over the occurrences of i of g, dL/dw0 = Σ g
    r = bn.fm_bn_step(X, y, E, w, w0, gamma, beta, bin_=bin_, keep=keep)
    ref_dw = np.zeros_like(dw)
    np.add.at(ref_dw, np.asarray(X, np.int64).reshape(-1), np.repeat(r["g"], X.shape[1]))
    assert np.allclose(dw, ref_dw, rtol=1e-13) and np.isclose(dw0, r["g"].sum(), rtol=1e-13)


def test_fp32_restatement_sits_inside_the_bound():
    """The magnitudes leave the float32 restatement (np.add.at, float32 sums)
    well inside 1e-5 · mag: err / bound <= 0.25 for every variable."""
    X, y, E, w, w0, gamma, beta = _case(B=257, k=20, M=50)
    _, grads, mags, _ = bn.fm_bn_grad64(X, y, E, w, w0, gamma, beta)
    r32 = bn.fm_bn_step(X, y, E, w, w0, gamma, beta, dtype=np.float32)
    befores = (E, w, w0, gamma, beta)
    for name, key, g64, mag, before in zip("E w w0 gamma beta".split(),
                                           "dE dw dw0 dgamma dbeta".split(), grads, mags, befores):
        g32 = np.asarray(r32[key], np.float32)
        after = np.asarray(before, np.float32) - g32
        ratio = tr.ratio(g32.astype(np.float64), before, after, g64, mag)
        print(f"fm_bn fp32 restatement {name}: err / bound = {ratio:.3g}")
        assert ratio <= 0.25, (name, ratio)


def test_masks_of_ones_are_the_undropped_step():
    X, y, E, w, w0, gamma, beta = _case()
    a = bn.fm_bn_step(X, y, E, w, w0, gamma, beta)
    b = bn.fm_bn_step(X, y, E, w, w0, gamma, beta, bin_=np.ones((X.shape[0], E.shape[1])), keep=1.0)
    for key in ("loss", "dE", "dw", "dw0", "dgamma", "dbeta"):
        assert np.array_equal(a[key], b[key]), key


def test_gamma_one_beta_zero_large_eps_tends_to_a_scaled_fm():
    """With v ≪ eps the layer is x ↦ (x − μ)/√eps: dE then follows the plain FM
    gradient of the centred score up to O(v/eps)."""
    X, y, E, w, w0, gamma, beta = _case()
    E = (E * 0.03).astype(np.float32)
    r = bn.fm_bn_step(X, y, E, w, w0, np.ones_like(gamma), np.zeros_like(beta), eps=1.0)
    assert r["v"].max() < 1e-6
    e = E.astype(np.float64)[np.asarray(X, np.int64)]
    s = e.sum(1)
    gc = r["g"][:, None] - r["g"].mean()
    dE = np.zeros((E.shape[0], E.shape[1]))
    for f in range(X.shape[1]):
        np.add.at(dE, X[:, f], gc * (s - e[:, f]))
    assert np.allclose(r["dE"], dE, rtol=1e-5, atol=1e-12)


def test_known_answer_is_exact():
    """x = ±1, μ = 0, v = 1, inv = ½: the float32 and the float64 restatements
    agree to the bit, and so do two seeded row permutations of each."""
    X, y, E, w, w0, gamma, beta = bn.known_answer()
    r64 = bn.fm_bn_step(X, y, E, w, w0, gamma, beta, eps=bn.KNOWN_EPS)
    r32 = bn.fm_bn_step(X, y, E, w, w0, gamma, beta, eps=bn.KNOWN_EPS, dtype=np.float32)
    assert np.all(np.abs(r64["x"]) == 1.0)
    assert np.all(r64["mu"] == 0.0) and np.all(r64["v"] == 1.0)
    keys = ("dE", "dw", "dw0", "dgamma", "dbeta")
    for key in keys:
        a = np.asarray(r64[key])
        assert np.array_equal(a, np.asarray(r32[key]).astype(np.float64)), key
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64)), key
    assert r64["loss"] == r32["loss"]
    assert np.count_nonzero(r64["dE"]) > 100 and np.abs(r64["dgamma"]).min() > 0
    for seed in (1, 2):
        p = np.random.default_rng(seed).permutation(len(y))
        for dt in (np.float64, np.float32):
            rp = bn.fm_bn_step(X[p], y[p], E, w, w0, gamma, beta, eps=bn.KNOWN_EPS, dtype=dt)
            for key in keys:
                assert np.array_equal(np.asarray(rp[key]).astype(np.float64), r64[key]), (key, dt)
            assert rp["loss"] == r64["loss"]
    # the figures of the design: 144 non-zero dE elements, max |dE| = 531.375, dβ_c = −695
    assert np.count_nonzero(r64["dE"]) == 144 and np.abs(r64["dE"]).max() == 531.375
    assert np.all(r64["dbeta"] == -695.0)


def test_exact_score_with_identity_statistics_is_fm_out():
    """γ = 1, β = 0, mm = 0, mv = 1 − eps: a ≡ 1 and the score is FM.out."""
    X, y, E, w, w0, gamma, beta = _case()
    k = E.shape[1]
    out, mag = bn.fm_bn_score64(X, E, w, w0, np.ones(k), np.zeros(k), np.zeros(k),
                                np.full(k, 1.0 - bn.EPS))
    e = E.astype(np.float64)[np.asarray(X, np.int64)]
    s = e.sum(1)
    ref = (0.5 * (s * s - (e * e).sum(1))).sum(1) + w.astype(np.float64)[X].sum(1) + float(w0)
    assert np.allclose(out, ref, rtol=1e-14) and np.all(mag >= np.abs(out))


# ---------------------------------------------------------------------------
# C ABI without a device
# ---------------------------------------------------------------------------
_vp, _i32, _i64, _f32, _u64, _sz = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                    ctypes.c_float, ctypes.c_uint64, ctypes.c_size_t)
_D = 0x1000            # a non-null, 8-byte aligned pointer that is never dereferenced
EINVAL, EWORKSPACE = -1, -3


def _lib():
    lib = ctypes.CDLL(LIB)
    lib.hhfm_fm_train_bn_workspace.argtypes = [_i64, _i64, _i32, ctypes.POINTER(_sz)]
    lib.hhfm_fm_train_bn_state_bytes.restype = _sz
    lib.hhfm_fm_train_bn_state_bytes.argtypes = [_i64, _i32]
    lib.hhfm_train_workspace.restype = _sz
    lib.hhfm_train_workspace.argtypes = [_i64, _i32]
    lib.hhfm_fm_train_step_bn.argtypes = (
        [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _i32, _f32, _f32, _i32, _f32, _u64, _vp, _vp,
         _vp, _vp, _sz] + [_vp] * 4 + [_f32, _f32, _vp, _vp, _vp, _vp])
    lib.hhfm_fm_score_rows_scaled.argtypes = [_vp, _i64, _i32, _vp, _i64, _i32, _i32, _vp, _f32,
                                              _vp, _vp, _vp, _vp]
    return lib


def test_new_symbols_are_exported_and_the_workspace_answers():
    """The CPU test that fails without the feature: the four symbols, and
    hhfm_fm_train_bn_workspace on the host — monotone in B, at least the
    persistent prefix plus x [B][k] and g [B], HHFM_EINVAL for B < 0."""
    lib = ctypes.CDLL(LIB)
    for n in ("hhfm_fm_score_rows_scaled", "hhfm_fm_train_step_bn", "hhfm_fm_train_bn_workspace",
              "hhfm_fm_train_bn_state_bytes"):
        assert hasattr(lib, n), n
    lib = _lib()
    M, k = 5051, 64
    state = lib.hhfm_fm_train_bn_state_bytes(M, k)
    assert state >= lib.hhfm_train_workspace(M, k) + 2 * k * 4
    last = 0
    for B in (0, 1, 2, 63, 64, 5000, 32773, 1 << 22):
        n = _sz(0)
        assert lib.hhfm_fm_train_bn_workspace(B, M, k, ctypes.byref(n)) == 0
        assert n.value >= state + B * k * 4 + B * 4 + (4 * k + 1) * 8 + 4 * k * 4
        assert n.value >= last and (B == 0 or n.value > last)
        last = n.value
    n = _sz(7)
    assert lib.hhfm_fm_train_bn_workspace(-1, M, k, ctypes.byref(n)) == EINVAL and n.value == 7
    assert lib.hhfm_fm_train_bn_workspace(8, 0, k, ctypes.byref(n)) == EINVAL
    assert lib.hhfm_fm_train_bn_workspace(8, M, 0, ctypes.byref(n)) == EINVAL
    assert lib.hhfm_fm_train_bn_workspace(8, M, k, None) == EINVAL
    assert lib.hhfm_fm_train_bn_state_bytes(0, k) == 0


def test_bn_step_checks_its_arguments_before_anything_is_launched():
    lib = _lib()
    B, F, M, k = 7, 5, 40, 8
    n = _sz(0)
    assert lib.hhfm_fm_train_bn_workspace(B, M, k, ctypes.byref(n)) == 0

    def step(B=B, keep=1.0, ws=_D, ws_bytes=n.value, gamma=_D, beta=_D, mm=_D, mv=_D, eps=1e-3,
             upd=0.1, ag=_D, ab=_D, opt=0):
        return lib.hhfm_fm_train_step_bn(_D, _D, B, F, _D, _D, _D, M, k, 0.1, 0.1, opt, keep, 5,
                                         _D, _D, _D, ws, ws_bytes, gamma, beta, mm, mv, eps, upd,
                                         ag, ab, _D, None)

    n0 = _sz(0)
    assert lib.hhfm_fm_train_bn_workspace(0, M, k, ctypes.byref(n0)) == 0
    assert step(B=0, ws_bytes=n0.value) == EINVAL
    for eps in (0.0, -1e-3, float("nan")):
        assert step(eps=eps) == EINVAL
    for upd in (1.5, -0.1, float("nan")):
        assert step(upd=upd) == EINVAL
    for name in ("gamma", "beta", "mm", "mv", "ag", "ab"):
        assert step(**{name: None}) == EINVAL, name
    assert step(ws=_D + 4) == EINVAL                    # the double sums need 8-byte alignment
    # the plain step's checks come first, in their order
    assert step(keep=0.0, eps=0.0) == EINVAL
    assert step(opt=9, eps=0.0) == -2                   # HHFM_EUNSUPPORTED before the layer's
    assert step(ws_bytes=n.value - 1, eps=0.0) == EWORKSPACE
    assert step(ws_bytes=n.value - 1) == EWORKSPACE


def test_scaled_rows_check_their_arguments():
    lib = _lib()

    def rows(B=4, F=5, k=8, dtype=0, scale=_D, out=_D):
        return lib.hhfm_fm_score_rows_scaled(_D, B, F, _D, 40, k, dtype, _D, 0.0, scale, out, None,
                                             None)
    assert rows(scale=None) == EINVAL
    assert rows(B=-1) == EINVAL and rows(F=65) == EINVAL and rows(dtype=7) == EINVAL
    assert rows(out=None) == EINVAL
    assert rows(B=0) == 0
