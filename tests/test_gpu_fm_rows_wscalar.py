"""The user / item `w` terms of the LDS-tail FM row kernel (HHFM_K1_W_SCALAR,
hhfm_amd/csrc/fm_rows.hip): for fp32 tables at F <= 5 and LPR >= 16 they are
fetched by wave-uniform scalar loads and written into lanes sub = 0, 1 of
each row's lane group; otherwise by the vector load.  Either way the forced
LDS-tail launch (flags 2) must give the bits of the default kernel (flags 4),
stay within the oracle bound of
tests/test_gpu_kernels.py::test_fm_score_rows_parity (RTOL x Σ|terms|) and
leave the status word 0.

Shapes (F, k, dtype): LPR 16 / 32 / 64 fp32 are on the scalar path; the two
bf16 shapes at LPR 16 / 32 were, until the path was kept to fp32 tables
(profiles/k1_w_scalar_ab.txt), and stay as cases of the vector load at those
widths beside the LPR 8 / 4 controls.

`w` is N(0, 1) with distinct entries against E ~ N(0, 0.01): a `w` delivered to
the wrong row, group or lane moves the result by ~1, five orders beyond the
bound.  Columns 2.. are drawn from the table's last 12 rows (inside the LDS
window), so every wave stays in the LDS-tail loop unless a case says otherwise.

B: 1, 3, 4, 5 (a slot of 4 rows at LPR 16, +-1), 23, 24, 25 (a wave-iteration
of 24 rows, +-1), 97, 4099 (a forced launch takes a quarter of the blocks, so
waves iterate); at LPR 32 / 64 the slot and iteration edges 2 / 12 and 1 / 6,
+-1, as well; at F = 8 (4 row slots) the 16-row iteration, +-1.

Not covered by these shapes: tables with features_M * 4 >= 2^32 bytes of `w`;
the kernel forms the 64-bit address of every scalar load, whatever M is.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import fm_oracle as orc
from tests.helpers import bf16_round, table

pytestmark = pytest.mark.gpu
RTOL = 1e-5
W0 = 0.003
M = 50000
BMAX = 4099
FLAG_HOT, FLAG_NO_HOT = 2, 4
STATUS_BAD_ID = 1
SENTINEL = 1.0e6

# LPR >= 16: fp32 on the scalar path, bf16 on the vector load; LPR < 16: vector load
WIDE = [(5, 64, "f32"), (3, 128, "f32"), (4, 256, "f32"), (8, 128, "bf16"), (5, 256, "bf16")]
NARROW = [(5, 32, "f32"), (5, 32, "bf16")]
B_BASE = [1, 3, 4, 5, 23, 24, 25, 97, 4099]


def _lpr(k, dtype):
    return k * (2 if dtype == "bf16" else 4) // 16


def _b_values(F, k, dtype):
    extra = {32: [2, 11, 12, 13], 64: [2, 6, 7]}.get(_lpr(k, dtype), [])
    if F > 6:                         # 4 row slots: 16 rows per wave-iteration at LPR 16
        extra = extra + [15, 16, 17]
    return sorted(set(B_BASE + extra))


CASES = [(F, k, dt, B) for F, k, dt in WIDE + NARROW for B in _b_values(F, k, dt)]


def _fm_scale(X, E, w, w0):
    e = E[X.astype(np.int64)].astype(np.float64)
    s = e.sum(1)
    q = (e * e).sum(1)
    scale = (0.5 * (s * s + q)).sum(1)
    if w is not None:
        scale += np.abs(w[X.astype(np.int64)]).sum(1)
    return scale + abs(w0)


def _reference(X, E, w, dtype, m):
    Eo = bf16_round(E) if dtype == "bf16" else E
    Xo = np.where((X < 0) | (X >= m), 0, X).astype(np.int32)   # bad ids read row 0
    return orc.fm_out(Xo, Eo, w, W0)[:, 0], _fm_scale(Xo, Eo, w, W0)


@functools.lru_cache(maxsize=None)
def _case(F, k, dtype, kind="plain"):
    """Host inputs and the oracle's rows of one (shape, kind), computed once,
    shared by every B and never modified.
      plain     columns 0, 1 uniform over the table, 2.. in the last 12 rows
      sentinel  as plain with w[0] = SENTINEL: what rows >= B and clamped ids
                read, visible at once if it reaches a row that did not ask for it
      bad       as plain with ids -1 and M in column 0, in column 1 and in a
                context column (that wave goes to the general loop)
      small     a 10-row table, every column uniform over it: user and item
                ids are window rows too
      now       as plain, without `w`
    """
    rng = np.random.default_rng(7100 + 37 * F + k + len(kind) + (dtype == "bf16"))
    m = 10 if kind == "small" else M
    X = rng.integers(0, m, size=(BMAX, F)).astype(np.int64)
    if kind != "small":
        X[:, 2:] = rng.integers(m - 12, m, size=(BMAX, F - 2))
    if kind == "bad":
        X[0, 0], X[1, 0] = -1, m
        X[2, 1], X[5, 1] = m, -1
        X[30, 2] = -1
        X[rng.integers(40, BMAX, 6), rng.integers(0, 2, 6)] = -1
    X = X.astype(np.int32)
    E = table(rng, m, k)
    # N(0, 1) with distinct fp32 entries: duplicates of a larger draw dropped
    w = rng.permutation(np.unique(rng.normal(0, 1, size=2 * m + 64).astype(np.float32)))[:m]
    w = np.ascontiguousarray(w)
    assert np.unique(w).size == m
    if kind == "sentinel":
        w[0] = SENTINEL
    ref, scale = _reference(X, E, None if kind == "now" else w, dtype, m)
    for a in (X, E, w, ref, scale):
        a.setflags(write=False)
    return X, E, w, m, ref, scale


def _dev(a):
    return torch.tensor(a, device="cuda")


def _run(X, E, w, m, k, dtype, flags):
    from hhfm_amd._native import native
    B, F = X.shape
    out = torch.full((B,), float("nan"), device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    native().fm_score_rows_ex(X.data_ptr(), B, F, E.data_ptr(), m, k,
                              1 if dtype == "bf16" else 0, 0 if w is None else w.data_ptr(),
                              W0, out.data_ptr(), flags, status.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    return out.cpu(), int(status.item())


def _check(F, k, dtype, B, kind, want_status=0):
    Xh, Eh, wh, m, ref, scale = _case(F, k, dtype, kind)
    X = _dev(Xh[:B])
    E = _dev(Eh)
    if dtype == "bf16":
        E = E.to(torch.bfloat16)
    w = None if kind == "now" else _dev(wh)
    hot, st_hot = _run(X, E, w, m, k, dtype, FLAG_HOT)
    fast, st_fast = _run(X, E, w, m, k, dtype, FLAG_NO_HOT)
    assert torch.equal(hot, fast)
    assert st_hot == want_status and st_fast == want_status
    err = np.abs(hot.numpy().astype(np.float64) - ref[:B])
    print(f"max err / scale {float((err / scale[:B]).max()):.3g}")
    assert np.all(err <= RTOL * scale[:B] + 1e-12)


@pytest.mark.parametrize("F,k,dtype,B", CASES)
def test_wscalar_bits_and_oracle(F, k, dtype, B):
    _check(F, k, dtype, B, "plain")


@pytest.mark.parametrize("B", [1, 5, 25, 4099])
@pytest.mark.parametrize("F,k,dtype", [(5, 64, "f32"), (4, 256, "f32"), (8, 128, "bf16"),
                                       (5, 32, "f32")])
def test_wscalar_row0_sentinel(F, k, dtype, B):
    """w[0] is what the loads of rows >= B read: it must reach no row."""
    _check(F, k, dtype, B, "sentinel")


@pytest.mark.parametrize("B", [3, 25, 97, 4099])
@pytest.mark.parametrize("F,k,dtype", [(5, 64, "f32"), (3, 128, "f32"), (5, 256, "bf16"),
                                       (5, 32, "bf16")])
def test_wscalar_bad_ids(F, k, dtype, B):
    _check(F, k, dtype, B, "bad", STATUS_BAD_ID)


@pytest.mark.parametrize("kind", ["small", "now"])
@pytest.mark.parametrize("B", [5, 25, 4099])
@pytest.mark.parametrize("F,k,dtype", WIDE + NARROW[:1])
def test_wscalar_small_table_and_no_w(F, k, dtype, B, kind):
    _check(F, k, dtype, B, kind)
