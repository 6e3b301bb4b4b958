"""The LDS-tail FM row kernel (HHFM_FLAG_HOT_TAIL, include/hhfm.h) against the
default kernel and the CPU oracle.

The two kernels add the same terms in the same order, so for every input the
forced LDS-tail launch (flags 2) must give the bits of the default kernel
(flags 4); the flags-2 output is also held to the oracle bound of
tests/test_gpu_kernels.py::test_fm_score_rows_parity (RTOL x Σ|terms|).

The window is the table's last T = 16 KiB / row_bytes rows.  Id layouts of
the columns 2.. (columns 0, 1 are uniform over the table):
  a  the last 12 rows (the loaders' context vocabulary)
  b  the last T rows, both boundary rows M-T and M-1 present
  c  as a, 1 % of the rows with one id just outside the window (M-T-1 or 0):
     waves leave the LDS loop part-way through their rows
  d  uniform over the table (nearly every wave-iteration misses)
  e  a 10-row table, all of it inside the window
  f  as a, with ids -1 and M: read as row 0, flagged in the status word
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
BMAX = 4099
FLAG_HOT, FLAG_NO_HOT = 2, 4
STATUS_BAD_ID = 1
SHAPES = [(5, 64, "f32"), (3, 16, "f32"), (8, 128, "bf16"), (5, 32, "bf16")]


def _fm_scale(X, E, w, w0):
    e = E[X.astype(np.int64)].astype(np.float64)
    s = e.sum(1)
    q = (e * e).sum(1)
    scale = (0.5 * (s * s + q)).sum(1)
    if w is not None:
        scale += np.abs(w[X.astype(np.int64)]).sum(1)
    return scale + abs(w0)


def _ids(rng, layout, F, M, T):
    """[BMAX, F] int32; the rows that make a layout what it is come first, so
    every prefix X[:B] keeps them."""
    X = rng.integers(0, M, size=(BMAX, F)).astype(np.int64)
    if layout in "acf":
        X[:, 2:] = rng.integers(max(M - 12, 0), M, size=(BMAX, F - 2))
    if layout == "b":
        X[:, 2:] = rng.integers(M - T, M, size=(BMAX, F - 2))
        X[0, 2] = X[1, 2] = M - T
        X[0, F - 1] = X[1, F - 1] = M - 1
        X[1, 2] = M - T
    if layout == "c":
        rows = np.unique(np.concatenate([[0], rng.integers(0, BMAX, BMAX // 100)]))
        cols = rng.integers(2, F, size=rows.size)
        X[rows, cols] = np.where(np.arange(rows.size) % 2 == 0, M - T - 1, 0)
    if layout == "f":
        X[0, 2] = -1
        X[1, 0] = M
        X[2, F - 1] = M
        X[rng.integers(3, BMAX, 5), rng.integers(0, F, 5)] = -1
    return X.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(F, k, dtype, layout):
    """Host inputs and the oracle's rows for one (shape, layout), computed once
    and shared by every B and by the w / no-w cases; never modified."""
    rng = np.random.default_rng(4000 + 31 * F + k + ord(layout))
    M = 10 if layout == "e" else 50000
    T = 16384 // (k * (2 if dtype == "bf16" else 4))
    X = _ids(rng, layout, F, M, T)
    E = table(rng, M, k)
    w = rng.normal(0, 0.01, size=M).astype(np.float32)
    Eo = bf16_round(E) if dtype == "bf16" else E
    Xo = np.where((X < 0) | (X >= M), 0, X).astype(np.int32)   # bad ids read row 0
    ref = {True: orc.fm_out(Xo, Eo, w, W0)[:, 0], False: orc.fm_out(Xo, Eo, None, W0)[:, 0]}
    scale = {True: _fm_scale(Xo, Eo, w, W0), False: _fm_scale(Xo, Eo, None, W0)}
    for a in (X, E, w, *ref.values(), *scale.values()):
        a.setflags(write=False)
    return X, E, w, M, ref, scale


def _dev(a):
    return torch.tensor(a, device="cuda")


def _run(X, E, w, M, k, dtype, flags):
    from hhfm_amd._native import native
    B, F = X.shape
    out = torch.full((B,), float("nan"), device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    native().fm_score_rows_ex(X.data_ptr(), B, F, E.data_ptr(), M, k,
                              1 if dtype == "bf16" else 0, 0 if w is None else w.data_ptr(),
                              W0, out.data_ptr(), flags, status.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    return out.cpu(), int(status.item())


@pytest.mark.parametrize("has_w", [True, False], ids=["w", "now"])
@pytest.mark.parametrize("layout", list("abcdef"))
@pytest.mark.parametrize("B", [1, 63, BMAX])
@pytest.mark.parametrize("F,k,dtype", SHAPES)
def test_hot_tail_bits_and_oracle(F, k, dtype, B, layout, has_w):
    Xh, Eh, wh, M, ref, scale = _case(F, k, dtype, layout)
    X = _dev(Xh[:B])
    E = _dev(Eh)
    if dtype == "bf16":
        E = E.to(torch.bfloat16)
    w = _dev(wh) if has_w else None
    hot, st_hot = _run(X, E, w, M, k, dtype, FLAG_HOT)
    fast, st_fast = _run(X, E, w, M, k, dtype, FLAG_NO_HOT)
    assert torch.equal(hot, fast)
    want = STATUS_BAD_ID if layout == "f" else 0
    assert st_hot == want and st_fast == want
    err = np.abs(hot.numpy().astype(np.float64) - ref[has_w][:B])
    print(f"max err / scale {float((err / scale[has_w][:B]).max()):.3g}")
    assert np.all(err <= RTOL * scale[has_w][:B] + 1e-12)


def test_hot_tail_automatic_threshold():
    """The smallest call the automatic rule gives to the LDS-tail kernel (its
    grid reaches the per-CU block cap: 64 blocks x 96 rows per CU at F=5, k=64
    fp32) and the largest it does not: the default kernel's bits either way,
    with rows that miss the window in both."""
    Xh, Eh, wh, M, _, _ = _case(5, 64, "f32", "c")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    edge = cus * 64 * 96
    E = _dev(Eh)
    w = _dev(wh)
    reps = -(-edge // BMAX)
    Xall = _dev(Xh).repeat(reps, 1)
    for B in (edge - 96, edge - 95):
        X = Xall[:B].contiguous()
        auto, _ = _run(X, E, w, M, 64, "f32", 0)
        fast, _ = _run(X, E, w, M, 64, "f32", FLAG_NO_HOT)
        assert torch.equal(auto, fast)


def test_hot_tail_flag_conflicts_rejected():
    """Force and refuse together, or force with the all-streaming plan, is
    HHFM_EINVAL (ValueError from the binding) before anything is launched;
    forcing a shape without such a kernel (F = 2) is HHFM_EUNSUPPORTED."""
    Xh, Eh, wh, M, _, _ = _case(5, 64, "f32", "a")
    X = _dev(Xh[:63])
    E = _dev(Eh)
    for flags in (FLAG_HOT | FLAG_NO_HOT, FLAG_HOT | 1, 8, 16):
        with pytest.raises(ValueError, match="invalid argument"):
            _run(X, E, None, M, 64, "f32", flags)
    with pytest.raises(ValueError, match="unsupported"):
        _run(X[:, :2].contiguous(), E, None, M, 64, "f32", FLAG_HOT)
