"""The validity-only front end and the packed chunk math of the LDS-tail FM row
kernel (HHFM_K1_LEAN_FRONT, HHFM_K1_PK_MATH; hhfm_amd/csrc/fm_rows.hip).

The LDS-tail loop takes full wave-iterations only and forms one verdict per
iteration from the raw ids; a bad id, an id outside the window and the partial
last iteration of a wave all go to the general loop, which clamps and raises
the status word.  So the forced LDS-tail launch (flags 2) must give the bits of
the default kernel (flags 4), stay within the oracle bound of
tests/test_gpu_kernels.py::test_fm_score_rows_parity (RTOL x Σ|terms|), and
report BAD_ID exactly when a row holds a bad id — wherever in a wave's walk the
hand-off to the general loop happens.

Geometry of the forced launch (try_fm_hot): LPR = row bytes / 16 lanes per
row, RPW = 64 / LPR rows per slot, U = 6 slots (4 at F > 6), RPI = RPW * U rows
per wave-iteration, a quarter of ceil(B / (4 * RPI)) blocks of 4 waves; wave v
takes the iterations at v * RPI + i * (waves * RPI).

Table M = 50,000; columns 2.. in the last 12 rows (inside the LDS window).
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

SHAPES = [(5, 64, "f32"), (3, 128, "f32"), (8, 128, "bf16"), (5, 32, "bf16")]


def _geom(F, k, dtype, B=BMAX):
    lpr = k * (2 if dtype == "bf16" else 4) // 16
    rpw = 64 // lpr
    U = 6 if F <= 6 else 4
    rpi = rpw * U
    blocks = -(-B // (4 * rpi))
    waves = 4 * max(1, blocks // 4)
    return dict(lpr=lpr, rpw=rpw, U=U, rpi=rpi, waves=waves, stride=waves * rpi,
                T=16384 // (lpr * 16))


def _fm_scale(X, E, w, w0):
    e = E[X.astype(np.int64)].astype(np.float64)
    s = e.sum(1)
    q = (e * e).sum(1)
    return (0.5 * (s * s + q)).sum(1) + np.abs(w[X.astype(np.int64)]).sum(1) + abs(w0)


def _reference(X, E, w, dtype):
    Eo = bf16_round(E) if dtype == "bf16" else E
    Xo = np.where((X < 0) | (X >= M), 0, X).astype(np.int32)   # bad ids read row 0
    return orc.fm_out(Xo, Eo, w, W0)[:, 0], _fm_scale(Xo, Eo, w, W0)


@functools.lru_cache(maxsize=None)
def _case(F, k, dtype, kind="plain"):
    """Host inputs, the oracle's rows and the device copies of the table and
    `w` of one (shape, kind); computed once, shared and never modified.
      plain  columns 0, 1 uniform over rows 1 .. M-1, 2.. in the last 12 rows
      row0   as plain, with batch row 0 wholly inside the window, E[0] = 1e3
             everywhere and w[0] = 1e6: table row 0 is what a clamped id reads,
             batch row 0 is what a load of a row past B reads
    """
    rng = np.random.default_rng(9300 + 41 * F + k + len(kind) + (dtype == "bf16"))
    X = rng.integers(1, M, size=(BMAX, F)).astype(np.int64)
    X[:, 2:] = rng.integers(M - 12, M, size=(BMAX, F - 2))
    E = table(rng, M, k)
    w = rng.permutation(np.unique(rng.normal(0, 1, size=2 * M + 64).astype(np.float32)))[:M]
    w = np.ascontiguousarray(w)
    if kind == "row0":
        X[0, :] = rng.integers(M - 12, M, size=F)
        E[0, :] = 1.0e3
        w[0] = 1.0e6
    X = X.astype(np.int32)
    ref, scale = _reference(X, E, w, dtype)
    for a in (X, E, w, ref, scale):
        a.setflags(write=False)
    Ed = torch.tensor(E, device="cuda")
    if dtype == "bf16":
        Ed = Ed.to(torch.bfloat16)
    return X, E, w, ref, scale, Ed, torch.tensor(w, device="cuda")


def _run(X, E, w, k, dtype, flags, w0=W0, m=M):
    from hhfm_amd._native import native
    B, F = X.shape
    out = torch.full((B,), float("nan"), device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    native().fm_score_rows_ex(X.data_ptr(), B, F, E.data_ptr(), m, k,
                              1 if dtype == "bf16" else 0, w.data_ptr(), w0, out.data_ptr(),
                              flags, status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out.cpu(), int(status.item())


def _check(F, k, dtype, Xh, Ed, wd, ref, scale, want_status=0):
    X = torch.tensor(Xh, device="cuda")
    hot, st_hot = _run(X, Ed, wd, k, dtype, FLAG_HOT)
    fast, st_fast = _run(X, Ed, wd, k, dtype, FLAG_NO_HOT)
    diff = torch.nonzero(~((hot == fast) | (hot.isnan() & fast.isnan()))).flatten()
    assert diff.numel() == 0, f"{diff.numel()} rows differ from flags 4, first {diff[:8].tolist()}"
    assert torch.equal(hot, fast)
    assert st_hot == want_status and st_fast == want_status
    err = np.abs(hot.numpy().astype(np.float64) - ref)
    print(f"max err / scale {float((err / scale).max()):.3g}")
    assert np.all(err <= RTOL * scale + 1e-12)


# --- where the hand-off to the general loop happens --------------------------
def _positions(F, k, dtype):
    """(name, row): wave 1's first, a middle and its last full iteration x slot
    0 / the last slot x group 0 / the last group"""
    g = _geom(F, k, dtype)
    v = 1
    last = (BMAX - g["rpi"] - v * g["rpi"]) // g["stride"]     # last full iteration of wave v
    assert last >= 2 and v * g["rpi"] + last * g["stride"] + g["rpi"] <= BMAX
    out = []
    for iname, i in (("first", 0), ("middle", last // 2 if last > 2 else 1), ("last", last)):
        for u in (0, g["U"] - 1):
            for grp in (0, g["rpw"] - 1):
                r = v * g["rpi"] + i * g["stride"] + u * g["rpw"] + grp
                out.append((f"{iname}-u{u}-g{grp}", r))
    return out


HANDOFF = [(F, k, dt, kind, name, r) for F, k, dt in SHAPES
           for kind in ("user-1", "itemM", "ctx-out")
           for name, r in _positions(F, k, dt)]


@pytest.mark.parametrize("F,k,dtype,kind,name,r", HANDOFF,
                         ids=[f"{F}-{k}-{dt}-{kind}-{name}" for F, k, dt, kind, name, r in HANDOFF])
def test_lean_handoff_position(F, k, dtype, kind, name, r):
    """One irregular row at row r: a bad user id (-1), a bad item id (M) or a
    valid context id just below the window (M - T - 1).  Every output row
    equals flags 4; the status word is BAD_ID exactly for the bad ids."""
    Xp, E, w, ref, scale, Ed, wd = _case(F, k, dtype)
    X = Xp.copy()
    if kind == "user-1":
        X[r, 0] = -1
    elif kind == "itemM":
        X[r, 1] = M
    else:
        X[r, F - 1] = M - _geom(F, k, dtype)["T"] - 1
    ref, scale = ref.copy(), scale.copy()
    ref[r:r + 1], scale[r:r + 1] = _reference(X[r:r + 1], E, w, dtype)
    _check(F, k, dtype, X, Ed, wd, ref, scale,
           0 if kind == "ctx-out" else STATUS_BAD_ID)


# --- edges of the full-iteration rule ----------------------------------------
def _b_values(F, k, dtype):
    g = _geom(F, k, dtype)
    rpw, rpi = g["rpw"], g["rpi"]
    own = [rpw - 1, rpw, rpw + 1, rpi - 1, rpi, rpi + 1, 2 * rpi - 1, 2 * rpi, 2 * rpi + 1]
    base = [1, 23, 24, 25, 47, 48, 49] + [960 + d for d in (0, 1, 23, 24, 25)]
    return sorted({b for b in base + own if b >= 1})


EDGES = [(F, k, dt, B) for F, k, dt in SHAPES for B in _b_values(F, k, dt)]


@pytest.mark.parametrize("F,k,dtype,B", EDGES)
def test_lean_full_iteration_edges(F, k, dtype, B):
    """B around a slot, a wave-iteration and two of them: the rows of a partial
    iteration are the general loop's."""
    X, E, w, ref, scale, Ed, wd = _case(F, k, dtype)
    _check(F, k, dtype, X[:B], Ed, wd, ref[:B], scale[:B])


@pytest.mark.parametrize("B", [25, 97, 4099])
@pytest.mark.parametrize("F,k,dtype", SHAPES)
def test_lean_row0_reaches_nobody(F, k, dtype, B):
    """E[0] = 1e3 and w[0] = 1e6, batch row 0 inside the window, B no multiple
    of the wave-iteration: what the loads of rows past B and of iterations the
    loop does not run bring in must reach no output row."""
    assert B % _geom(F, k, dtype)["rpi"] != 0
    X, E, w, ref, scale, Ed, wd = _case(F, k, dtype, "row0")
    assert X.min() >= 1
    _check(F, k, dtype, X[:B], Ed, wd, ref[:B], scale[:B])


# --- exact arithmetic: the packed chunk math ----------------------------------
EXACT_W0 = 0.25


def _exact_tables(rng, k):
    """entries in {-2 .. 2} x 2^-3 and `w` in multiples of 2^-6: every product
    and sum of the score is exact in fp32 (and the table in bf16), in any order"""
    E = rng.integers(-2, 3, size=(M, k)).astype(np.float32) / 8.0
    w = rng.integers(-64, 65, size=M).astype(np.float32) / 64.0
    return E, w


def _exact_f64(X, E, w):
    e = E[X.astype(np.int64)].astype(np.float64)
    s = e.sum(1)
    q = (e * e).sum(1)
    return (0.5 * (s * s - q)).sum(1) + w[X.astype(np.int64)].astype(np.float64).sum(1) + EXACT_W0


def _check_exact(F, k, dtype, X, E, w):
    want = _exact_f64(X, E, w)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    Xd = torch.tensor(X, device="cuda")
    Ed = torch.tensor(E, device="cuda")
    if dtype == "bf16":
        assert np.array_equal(bf16_round(E), E)
        Ed = Ed.to(torch.bfloat16)
    wd = torch.tensor(w, device="cuda")
    for flags in (FLAG_HOT, FLAG_NO_HOT):
        got, st = _run(Xd, Ed, wd, k, dtype, flags, w0=EXACT_W0)
        assert st == 0
        assert np.array_equal(got.numpy().astype(np.float64), want), f"flags {flags}"


@pytest.mark.parametrize("F,k,dtype", SHAPES)
def test_lean_exact_small_integers(F, k, dtype):
    rng = np.random.default_rng(9400 + F + k)
    E, w = _exact_tables(rng, k)
    X = rng.integers(0, M, size=(BMAX, F)).astype(np.int64)
    X[:, 2:] = rng.integers(M - 12, M, size=(BMAX, F - 2))
    _check_exact(F, k, dtype, X.astype(np.int32), E, w)


@pytest.mark.parametrize("F,k,dtype", SHAPES)
def test_lean_exact_one_hot_pairs(F, k, dtype):
    """User row 1 + j is one-hot at element j, item row 1 + k + j' at j', the
    context rows are zero: the interaction is 1 exactly when j = j', for every
    (j, j') — every element of a chunk in every lane of the row's group.  An
    element paired with the wrong partner turns a 0 into a 1 or back."""
    rng = np.random.default_rng(9500 + F + k)
    E, w = _exact_tables(rng, k)
    E[1:1 + 2 * k] = 0.0
    E[1 + np.arange(k), np.arange(k)] = 1.0
    E[1 + k + np.arange(k), np.arange(k)] = 1.0
    E[M - 12:] = 0.0
    j, jp = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    B = k * k
    X = np.empty((B, F), dtype=np.int64)
    X[:, 0] = 1 + j.ravel()
    X[:, 1] = 1 + k + jp.ravel()
    X[:, 2:] = rng.integers(M - 12, M, size=(B, F - 2))
    X = X.astype(np.int32)
    inter = _exact_f64(X, E, w) - w[X.astype(np.int64)].astype(np.float64).sum(1) - EXACT_W0
    assert np.array_equal(inter, (j.ravel() == jp.ravel()).astype(np.float64))
    _check_exact(F, k, dtype, X, E, w)
