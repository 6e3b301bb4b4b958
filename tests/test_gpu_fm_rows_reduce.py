"""The in-register (DPP) group reductions of the FM and HHFM row kernels
(fm_rows_fast, fm_rows_fast_hot, hybrid_rows_fast), at every group width:
fp32 k = 16 .. 256 (4 .. 64 lanes per row) and bf16 k = 32, 128.

Exact cases: table entries are integers in [-4, 4], `w` entries multiples of
1/8 in [-2, 2], w0 = 0.25, so every partial sum is exact in fp32 in any order
and the kernel must return the float64 oracle's value bit for bit.  A lane
left out of, or counted twice in, a reduction changes that value; a store that
lands on the wrong row shows at B = 23 / 25 (24 rows per wave-iteration at
k = 64) and in the NaN-filled output.  `test_exact_reference_is_fp32` checks on
the CPU that the float64 values are fp32 numbers (largest |value| at k = 256,
F = 5).

Context-column layouts: "a" the table's last 12 rows (the LDS-tail loop of
fm_rows_fast_hot under flags 2), "d" uniform over the table (its general loop).

The same cases with N(0, 0.01) tables are held to the bound of
tests/test_gpu_fm_rows_hot.py: |got - float64| <= 1e-5 x Σ|terms| + 1e-12.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import fm_oracle as orc
from oracle import parity
from tests.helpers import bf16_round, table

gpu = pytest.mark.gpu
RTOL = 1e-5
W0_EXACT, W0_NORMAL = 0.25, 0.003
M = 600
BS = [1, 23, 24, 25, 63, 257]
BMAX = max(BS)
FS = [2, 5]
SHAPES = [(16, "f32"), (32, "f32"), (64, "f32"), (128, "f32"), (256, "f32"),
          (32, "bf16"), (128, "bf16")]
FLAGS = {2: (0, 4), 5: (0, 2, 4)}      # flags 2 (the LDS-tail kernel) needs F >= 3
LAYOUTS = "ad"
shape_cases = pytest.mark.parametrize("k,dtype", SHAPES, ids=[f"{d}-k{k}" for k, d in SHAPES])
field_cases = pytest.mark.parametrize("F", FS)


def _hhfm_split(F):
    """(ctx, time) column ranges and the oracle's (feature, time) dimensions"""
    return ((0, 0), (0, 0), 0, 0) if F == 2 else ((2, 4), (4, 5), 2, 1)


def _hhfm_terms(X, E):
    """Σ|terms| of the HHFM row score"""
    e = np.abs(E[X.astype(np.int64)].astype(np.float64))
    return (e[:, [0] + list(range(2, X.shape[1]))].sum(1) * e[:, 1]).sum(1)


@functools.lru_cache(maxsize=None)
def _case(F, k, dtype, layout, exact):
    """Host inputs and references of one case, computed once, never modified:
    X, E (as the GPU reads it), w, float64 FM rows with / without w and their
    Σ|terms|, the HHFM oracle's rows and their Σ|terms|."""
    rng = np.random.default_rng(9000 + 131 * F + k + 7 * ord(layout) + exact)
    X = rng.integers(0, M, size=(BMAX, F))
    if layout == "a":
        X[:, 2:] = rng.integers(M - 12, M, size=(BMAX, F - 2))
    X = X.astype(np.int32)
    if exact:
        E = rng.integers(-4, 5, size=(M, k)).astype(np.float32)
        w = (rng.integers(-16, 17, size=M) / 8.0).astype(np.float32)
        w0 = W0_EXACT
    else:
        E = table(rng, M, k)
        w = rng.normal(0, 0.01, size=M).astype(np.float32)
        w0 = W0_NORMAL
    if dtype == "bf16":
        E = bf16_round(E)
    fm = {True: parity.fm_rows_exact(X, E, w, w0), False: parity.fm_rows_exact(X, E, None, w0)}
    _, _, fd, td = _hhfm_split(F)
    hh = orc.hhfm_positive_feedback(X, E, fd, td, context=fd > 0, time=td > 0)[:, 0]
    hh_mag = _hhfm_terms(X, E)
    for a in (X, E, w, hh, hh_mag, *fm[True], *fm[False]):
        a.setflags(write=False)
    return X, E, w, w0, fm, hh, hh_mag


def _dev(a):
    return torch.tensor(a, device="cuda")


def _table_dev(E, dtype):
    return _dev(E).to(torch.bfloat16) if dtype == "bf16" else _dev(E)


def _fm(X, E, w, w0, k, dtype, flags):
    from hhfm_amd._native import native
    B, F = X.shape
    out = torch.full((B,), float("nan"), device="cuda")
    native().fm_score_rows_ex(X.data_ptr(), B, F, E.data_ptr(), M, k,
                              1 if dtype == "bf16" else 0, 0 if w is None else w.data_ptr(),
                              w0, out.data_ptr(), flags, 0,
                              torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


def _hhfm(X, E, F):
    from hhfm_amd import ops
    ctx, tim, _, _ = _hhfm_split(F)
    out = torch.full((X.shape[0],), float("nan"), device="cuda")
    return ops.hybrid_score_rows(X, E, 0, 1, ctx, tim, out=out).cpu().numpy()


@field_cases
@shape_cases
def test_exact_reference_is_fp32(k, dtype, F):
    """CPU: with the integer tables every reference value is an fp32 number,
    so bit equality with the float64 oracle is the right demand."""
    for layout in LAYOUTS:
        _, E, _, _, fm, hh, _ = _case(F, k, dtype, layout, True)
        if dtype == "bf16":
            assert np.array_equal(E, bf16_round(E.copy()))
        for has_w in (True, False):
            ref = fm[has_w][0]
            assert ref.dtype == np.float64
            assert np.array_equal(ref, ref.astype(np.float32).astype(np.float64))
        assert np.array_equal(hh.astype(np.float64), hh.astype(np.float32).astype(np.float64))


@gpu
@field_cases
@shape_cases
def test_fm_rows_exact(k, dtype, F):
    for layout in LAYOUTS:
        Xh, Eh, wh, w0, fm, _, _ = _case(F, k, dtype, layout, True)
        E, w, Xd = _table_dev(Eh, dtype), _dev(wh), _dev(Xh)
        for B in BS:
            X = Xd[:B].contiguous()
            for has_w in (True, False):
                ref = fm[has_w][0][:B]
                for flags in FLAGS[F]:
                    got = _fm(X, E, w if has_w else None, w0, k, dtype, flags)
                    assert np.array_equal(got.astype(np.float64), ref), \
                        (layout, B, has_w, flags, np.flatnonzero(got != ref)[:8])


@gpu
@field_cases
@shape_cases
def test_hybrid_rows_exact(k, dtype, F):
    for layout in LAYOUTS:
        Xh, Eh, _, _, _, hh, _ = _case(F, k, dtype, layout, True)
        E, Xd = _table_dev(Eh, dtype), _dev(Xh)
        for B in BS:
            got = _hhfm(Xd[:B].contiguous(), E, F)
            assert np.array_equal(got.astype(np.float64), hh[:B].astype(np.float64)), \
                (layout, B, np.flatnonzero(got != hh[:B])[:8])


@gpu
@field_cases
@shape_cases
def test_fm_rows_oracle_bound(k, dtype, F):
    worst = 0.0
    for layout in LAYOUTS:
        Xh, Eh, wh, w0, fm, _, _ = _case(F, k, dtype, layout, False)
        E, w, Xd = _table_dev(Eh, dtype), _dev(wh), _dev(Xh)
        for B in BS:
            X = Xd[:B].contiguous()
            for has_w in (True, False):
                ref, mag = fm[has_w][0][:B], fm[has_w][1][:B]
                for flags in FLAGS[F]:
                    got = _fm(X, E, w if has_w else None, w0, k, dtype, flags)
                    err = np.abs(got.astype(np.float64) - ref)
                    worst = max(worst, float((err / mag).max()))
                    assert np.all(err <= RTOL * mag + 1e-12), (layout, B, has_w, flags)
    print(f"max err / scale {worst:.3g}")


@gpu
@field_cases
@shape_cases
def test_hybrid_rows_oracle_bound(k, dtype, F):
    for layout in LAYOUTS:
        Xh, Eh, _, _, _, hh, mag = _case(F, k, dtype, layout, False)
        E, Xd = _table_dev(Eh, dtype), _dev(Xh)
        for B in BS:
            got = _hhfm(Xd[:B].contiguous(), E, F)
            err = np.abs(got.astype(np.float64) - hh[:B].astype(np.float64))
            assert np.all(err <= RTOL * mag[:B] + 1e-12), (layout, B)
