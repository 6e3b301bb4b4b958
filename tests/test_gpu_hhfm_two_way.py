"""The two-way HHFM model on the GPU (include/hhfm.h "Two-way pooling"):
hybrid_rows_two_way and the TwoWayFeature instantiations of hybrid_rows_generic,
catalog_queries and hhfm_train_rows against the numpy restatement of
tests/hhfm_two_way_ref.py (pinned on the CPU against the reference's own
pair-product tensors and central differences: tests/test_hhfm_two_way_ref.py).

Bars: row scores the project's score bar (helpers.kappa_check, 1e-5); golden
top-20 lists array_equal (the fixture keeps adjacent scores more than 1e-5 of
Σ|terms| apart); the large catalog by helpers.topk_tie_swaps, at most 2
float64-verified ties per case; the raw gradient the per-element bound of
test_gpu_train_grad.py; optimizer steps the bars of test_gpu_training.py."""
import functools

import numpy as np
import pytest
import torch

from oracle import fm_oracle as orc
from tests import hhfm_pool_ref as pr
from tests import hhfm_two_way_ref as tw
from tests.helpers import bf16_round, kappa_check, topk_tie_swaps
from tests.test_gpu_hhfm_pool import ROW_LAYOUTS, STEP_LAYOUTS, _dev, _our, _rows, _stream, _table
from tests.test_gpu_train_grad import _check as check_grad
from tests.test_gpu_training import OPTS, _check_slot, _check_var, _slots_of
from tests.test_hhfm_two_way_ref import G2, GOLD, LAYOUTS, SEXTUPLES, SIX_IDS, golden_layout2

pytestmark = pytest.mark.gpu
MAX_TIES = 2
MMM, EEE, SSS = tw.MMM, tw.EEE, tw.SSS
MIXED = (("max", "mean", "sum"), ("mean", "sum", "max"))


def _six_id(s):
    return "_".join(s[0]) + "__" + "_".join(s[1])


# ---------------------------------------------------------------------------
# 1. known answer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_known_answer(dtype):
    """k = 4, F = 4 (two context rows), one row, small integers x powers of two
    (bf16-representable): under all-sum h = u + (a + b + ab) + u·(a + b + ab),
    every product and sum exact, the score compared with ==."""
    from hhfm_amd import ops
    E = np.array([[1, 2, -0.5, 4], [2, 1, 1, -1], [0.5, -2, 3, 1], [4, 0.25, -1, 2]], np.float32)
    assert np.array_equal(bf16_round(E), E)
    u, it, a, b = E
    m = a + b + a * b
    want = float(((u + m + u * m) * it).sum())
    Eg, _ = _table(E, dtype)
    X = _dev(np.array([[0, 1, 2, 3]], np.int32))
    got = ops.hybrid_score_rows(X, Eg, 0, 1, (2, 4), (0, 0), pooling2=SSS)
    assert float(got.item()) == want
    got = ops.hybrid_score_rows(X, Eg, 0, 1, (2, 4), (0, 0), pooling=SSS, pooling2=SSS)
    assert float(got.item()) == want
    # and it is not the one-way model
    one = ops.hybrid_score_rows(X, Eg, 0, 1, (2, 4), (0, 0))
    assert float(one.item()) == float(((u + a + b) * it).sum()) != want


# ---------------------------------------------------------------------------
# 2. row parity
# ---------------------------------------------------------------------------
ROW_LAYOUTS2 = {n: ROW_LAYOUTS[n] for n in ("F5", "F10", "F12", "F9_generic",
                                           "noncanonical_generic")}
WIDTHS = [(16, "f32"), (64, "f32"), (128, "f32"), (20, "f32"), (32, "bf16"), (128, "bf16")]
ROW_STD = 0.3      # the pair terms then carry well over 10 % of Σ|terms| of h (asserted)


@pytest.mark.parametrize("k,dtype", WIDTHS)
@pytest.mark.parametrize("layout", sorted(ROW_LAYOUTS2))
def test_hybrid_score_rows_two_way_parity(layout, k, dtype):
    """The three fast layouts at every LPR the widths reach, the generic kernel
    (F = 9, a non-canonical column order, 80-byte rows), a partial last
    wave-iteration (B = 4,099) and B = 1, under five sextuples."""
    from hhfm_amd import ops
    cards, td = ROW_LAYOUTS2[layout]
    rng = np.random.default_rng(len(layout) * 1000 + k + 7)
    X, M = _rows(rng, 4099, 300, 900, cards, td)
    fd = len(cards)
    ctx, tim = (2, 2 + fd), ((2 + fd, 2 + fd + td) if td else (0, 0))
    ucol, icol = 0, 1
    if layout.startswith("noncanonical"):
        X = np.ascontiguousarray(X[:, [1, 0] + list(range(2, X.shape[1]))])
        ucol, icol = 1, 0
    Eg, E = _table(rng.normal(0, ROW_STD, (M, k)).astype(np.float32), dtype)
    Xd = _dev(X)
    for p1, p2 in tw.SEXTUPLES:
        tag = f"two_way_rows_{layout}_k{k}_{dtype}_{_six_id((p1, p2))}"
        share = tw.pair_share(X, E, ctx, tim, p1, p2, ucol)
        print(tag, "pair share min", float(share.min()))
        assert share.min() >= 0.10
        got = ops.hybrid_score_rows(Xd, Eg, ucol, icol, ctx, tim, pooling=p1, pooling2=p2)
        got = got.cpu().numpy()
        exact, mag = tw.exact_rows2(X, E, ctx, tim, p1, p2, ucol, icol)
        ref = tw.score_rows2(X, E, ctx, tim, p1, p2, ucol, icol)
        kappa_check(tag, got, ref, exact, mag)
        one = ops.hybrid_score_rows(Xd[:1], Eg, ucol, icol, ctx, tim, pooling=p1, pooling2=p2)
        assert abs(float(one.item()) - exact[0]) <= 1e-5 * mag[0]


def test_bad_id_flags_and_reads_row_0():
    from hhfm_amd import ops
    rng = np.random.default_rng(9)
    X, M = _rows(rng, 700, 300, 900, (7, 2, 3), 0)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k in (64, 20):                                  # fast and generic
        E = rng.normal(0, 0.2, (M, k)).astype(np.float32)
        st.zero_()
        kw = dict(pooling=MMM, pooling2=MMM)
        ops.hybrid_score_rows(_dev(X), _dev(E), 0, 1, (2, 5), (0, 0), status=st, **kw)
        assert int(st.item()) == 0
        Xb = X.copy()
        Xb[5, 3], Xb[699, 0] = M + 7, -1
        got = ops.hybrid_score_rows(_dev(Xb), _dev(E), 0, 1, (2, 5), (0, 0), status=st, **kw)
        assert int(st.item()) & 1
        X0 = Xb.copy()
        X0[5, 3], X0[699, 0] = 0, 0
        ref = ops.hybrid_score_rows(_dev(X0), _dev(E), 0, 1, (2, 5), (0, 0), **kw)
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


# ---------------------------------------------------------------------------
# 3. rows, catalog and training agree on h
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("layout", ["F5", "F10", "F12"])
def test_generic_and_fast_row_kernels_give_the_same_bits(layout, dtype):
    """The item rows are one-hot (1.0 at one element), so a row's score is
    h at that element exactly in either kernel's summation order; the same
    rows in a non-canonical column order run the generic kernel."""
    from hhfm_amd import ops
    cards, td = ROW_LAYOUTS[layout]
    k = 16
    rng = np.random.default_rng(31)
    X, M = _rows(rng, 1024, 300, k, cards, td)          # items 300 .. 300 + k
    for c in range(2 + len(cards), X.shape[1]):         # time ids: any non-item row
        X[:, c] = rng.integers(0, 300, len(X))
    X[:, 1] = 300 + np.arange(len(X)) % k
    E = rng.normal(0, 0.3, (M, k)).astype(np.float32)
    E[300:300 + k] = np.eye(k, dtype=np.float32)
    Eg, Er = _table(E, dtype)
    fd = len(cards)
    ctx, tim = (2, 2 + fd), ((2 + fd, 2 + fd + td) if td else (0, 0))
    Xs = np.ascontiguousarray(X[:, [1, 0] + list(range(2, X.shape[1]))])
    for p1, p2 in tw.SEXTUPLES:
        fast = ops.hybrid_score_rows(_dev(X), Eg, 0, 1, ctx, tim, pooling=p1, pooling2=p2)
        gen = ops.hybrid_score_rows(_dev(Xs), Eg, 1, 0, ctx, tim, pooling=p1, pooling2=p2)
        assert torch.equal(fast.view(torch.int32), gen.view(torch.int32)), (p1, p2)
        h = tw.hybrid2(Er, X, ctx, tim, p1, p2)
        want = h[np.arange(len(X)), X[:, 1] - 300]
        assert np.array_equal(fast.cpu().numpy().view(np.uint32), want.view(np.uint32)), (p1, p2)


@pytest.mark.parametrize("tag", LAYOUTS)
def test_catalog_scores_are_the_row_scores(tag):
    """What catalog_topk returns for (query, item) is what score_rows gives the
    row [user, that item, ctx, time]: to 1e-5 of Σ|terms| on the split-bf16
    MFMA path (its documented bound), and both within that of the float64
    value under HHFM_PLAN_EXACT_FP32."""
    from hhfm_amd import ops
    E, _, A, nu, ni, ctx, tim = golden_layout2(tag)
    for p1, p2 in SEXTUPLES:
        for plan in (0, ops.PLAN_EXACT_FP32):
            s, i = ops.catalog_topk(_dev(A), _dev(E), ops.MODE_HHFM, 20, nu, ni, 0, None, 0, ctx,
                                    tim, plan=plan, pooling=p1, pooling2=p2)
            rows = np.repeat(A, 20, axis=0)
            rows[:, 1] = nu + i.cpu().numpy().reshape(-1)
            r = ops.hybrid_score_rows(_dev(rows), _dev(E), 0, 1, ctx, tim, pooling=p1, pooling2=p2)
            exact, mag = tw.exact_rows2(rows, E, ctx, tim, p1, p2)
            r, s = r.cpu().numpy().astype(np.float64), s.cpu().numpy().reshape(-1)
            assert np.all(np.abs(r - s) <= 1e-5 * mag)
            assert np.all(np.abs(s - exact) <= 1e-5 * mag)


# ---------------------------------------------------------------------------
# 4. catalog
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(len(SEXTUPLES)), ids=SIX_IDS)
@pytest.mark.parametrize("tag", LAYOUTS)
def test_catalog_topk_two_way_golden(tag, n):
    """The restated top-20 lists under every plan a small catalog can take;
    HHFM_PLAN_FUSED has no two-way kernel and runs what the default runs."""
    from hhfm_amd import ops
    E, _, A, nu, ni, ctx, tim = golden_layout2(tag)
    p1, p2 = SEXTUPLES[n]
    want = G2[f"{tag}_restated_topk_idx"][n].astype(np.int32)
    res = {}
    for name, plan in (("default", 0), ("store", ops.PLAN_STORE), ("fused", ops.PLAN_FUSED),
                       ("gemm", ops.PLAN_GEMM), ("exact", ops.PLAN_EXACT_FP32)):
        s, i = ops.catalog_topk(_dev(A), _dev(E), ops.MODE_HHFM, 20, nu, ni, 0, None, 0, ctx, tim,
                                plan=plan, pooling=p1, pooling2=p2)
        res[name] = s.cpu().numpy()
        assert np.array_equal(i.cpu().numpy(), want), name
    assert np.array_equal(res["default"].view(np.uint32), res["fused"].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _big_catalog(n_item, dtype):
    rng = np.random.default_rng(n_item + len(dtype) + 3)
    A, M = _rows(rng, 130, 300, n_item, (5, 4, 6, 3, 7), 3)
    E = rng.normal(0, ROW_STD, (M, 64)).astype(np.float32)
    Er = bf16_round(E) if dtype == "bf16" else E
    ctx, tim = (2, 7), (7, 10)
    ref = {}
    for six in (tw.SEXTUPLES[0], MIXED):
        h = tw.hybrid2(Er, A, ctx, tim, *six)
        sc = h @ Er[300:300 + n_item].T
        ah = tw._abs_hybrid2(Er.astype(np.float64), A, ctx, tim, *six)
        scale = (ah @ np.abs(Er[300:300 + n_item].astype(np.float64)).T).max(1, keepdims=True)
        ref[six] = (sc, scale, tw.exact_catalog2(A, Er, 300, ctx, tim, *six))
    return A, E, ctx, tim, ref


@pytest.mark.parametrize("plan", ["default", "no_seed"])
@pytest.mark.parametrize("K", [1, 20, 33])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_catalog_topk_two_way_streaming_20000(dtype, K, plan):
    from hhfm_amd import ops
    flag = {"default": 0, "no_seed": ops.PLAN_NO_SEED}[plan]
    A, E, ctx, tim, ref = _big_catalog(20000, dtype)
    Eg, _ = _table(E, dtype)
    for six, (sc, scale, exact) in ref.items():
        s, i = ops.catalog_topk(_dev(A), Eg, ops.MODE_HHFM, K, 300, 20000, 0, None, 0, ctx, tim,
                                plan=flag, pooling=six[0], pooling2=six[1])
        s, i = s.cpu().numpy(), i.cpu().numpy()
        _, ri = orc.top_k(sc, K)
        assert topk_tie_swaps(i, ri, exact) <= MAX_TIES
        picked = np.take_along_axis(sc, i.astype(np.int64), axis=1)
        assert np.all(np.abs(picked.astype(np.float64) - s) <= 1e-5 * scale)
        assert np.all(np.diff(s, axis=1) <= 0)


@pytest.mark.parametrize("six", [(MMM, MMM), MIXED], ids=_six_id)
def test_item_shards_merged_equal_model_topk(six):
    from hhfm_amd import ops
    E, _, A, nu, ni, ctx, tim = golden_layout2("jiaju")
    m = _our(ctx[1] - 2, tim[1] - tim[0], E.shape[0], nu, ni, E.shape[1], pooling=six[0],
             two_way=True, pooling2=six[1])
    m.set_weights(feature_embeddings=E)
    whole = m.topk(A, 20)
    q = m._idx(A)
    bounds = np.linspace(0, ni, 9).astype(int)
    parts = [m.catalog_topk(q, int(b0), int(b1 - b0), 20) for b0, b1 in zip(bounds, bounds[1:])]
    _, ids = ops.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert np.array_equal(ids.cpu().numpy(), whole)
    assert np.array_equal(whole, G2["jiaju_restated_topk_idx"][SEXTUPLES.index(six)])


def test_mode_fm_is_refused():
    from hhfm_amd import ops
    rng = np.random.default_rng(4)
    X, M = _rows(rng, 40, 30, 90, (7, 2, 3), 0)
    Ed = _dev(rng.normal(0, 0.01, (M, 16)).astype(np.float32))
    w = _dev(rng.normal(0, 0.01, M).astype(np.float32))
    with pytest.raises(ValueError, match="invalid argument"):
        ops.catalog_topk(_dev(X), Ed, ops.MODE_FM, 5, 30, 90, 0, w, 0, (2, 5), (0, 0),
                         pooling2=SSS)


# ---------------------------------------------------------------------------
# 5. word and shape validation
# ---------------------------------------------------------------------------
def test_words_and_shapes_are_validated():
    """Bad pooling2 words, bad spellings, nc == 1, nt == 1, no fields: refused
    with the output buffer untouched."""
    from hhfm_amd import ops
    from hhfm_amd._native import native
    rng = np.random.default_rng(5)
    X, M = _rows(rng, 64, 30, 90, (7, 2, 3), 2)           # [u, i, c, c, c, t, t]
    Xd, Ed = _dev(X), _dev(rng.normal(0, 0.1, (M, 16)).astype(np.float32))
    out = torch.full((64,), 7.0, device="cuda")
    nat = native()

    def rows(ctx, tim, w1, w2):
        nat.hybrid_score_rows_pool2(Xd.data_ptr(), 64, 7, 0, 1, ctx[0], ctx[1], tim[0], tim[1],
                                    Ed.data_ptr(), M, 16, 0, out.data_ptr(), w1, w2, 0, _stream())

    def topk(ctx, tim, w1, w2):
        ws = torch.zeros(nat.catalog_topk_workspace(64, 90, 16, 5), dtype=torch.uint8,
                         device="cuda")
        ts = torch.full((64, 5), 7.0, device="cuda")
        ti = torch.full((64, 5), 7, dtype=torch.int32, device="cuda")
        try:
            nat.catalog_topk_pool2(Xd.data_ptr(), 64, 7, ops.MODE_HHFM, 0, ctx[0], ctx[1], tim[0],
                                   tim[1], Ed.data_ptr(), M, 16, 0, 0, 30, 90, 0, 5, ts.data_ptr(),
                                   ti.data_ptr(), ws.data_ptr(), ws.numel(), 0, w1, w2, 0,
                                   _stream())
        finally:
            torch.cuda.synchronize()
            assert bool((ts == 7.0).all()) and bool((ti == 7).all())

    def step(ctx, tim, w1, w2):
        E0 = Ed.clone()
        ws = torch.zeros(nat.train_workspace(M, 16), dtype=torch.uint8, device="cuda")
        loss = torch.full((1,), 7.0, device="cuda")
        acc = torch.full((M * 16,), 0.1, device="cuda")
        Nd = _dev(rng.integers(30, 120, (64, 4)).astype(np.int32))
        try:
            nat.hhfm_train_step_pool2(Xd.data_ptr(), Nd.data_ptr(), 64, 7, ctx[0], ctx[1], tim[0],
                                      tim[1], 4, E0.data_ptr(), M, 16, 0.1, 0.0, 0, acc.data_ptr(),
                                      ws.data_ptr(), ws.numel(), w1, w2, loss.data_ptr(), _stream())
        finally:
            torch.cuda.synchronize()
            assert torch.equal(E0, Ed) and float(loss.item()) == 7.0

    good = ((2, 5), (5, 7), 0, 0)
    bad = [((2, 5), (5, 7), 0, 3), ((2, 5), (5, 7), 0, 1 << 12), ((2, 5), (5, 7), 0, 0x30),
           ((2, 5), (5, 7), 3 << 8, 0), ((2, 5), (5, 7), 0, -1),
           ((2, 3), (5, 7), 0, 0),      # nc == 1
           ((2, 5), (5, 6), 0, 0),      # nt == 1
           ((2, 3), (0, 0), 0, 0),      # nc == 1, no time
           ((0, 0), (0, 0), 0, 0)]      # no fields: a stack of one member
    for fn in (rows, topk, step):
        for args in bad:
            with pytest.raises(ValueError, match="invalid argument"):
                fn(*args)
            torch.cuda.synchronize()
            assert bool((out == 7.0).all()), args
    rows(*good)
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
    for spelling in ("max", ("max", "sum"), ("max", "sum", "avg"), ("max", "sum", "mean", "sum"),
                     (0, 1, 3), 5):
        with pytest.raises(ValueError):
            ops.hybrid_score_rows(Xd, Ed, 0, 1, (2, 5), (5, 7), pooling2=spelling)
        with pytest.raises(ValueError):
            ops.catalog_topk(Xd, Ed, ops.MODE_HHFM, 5, 30, 90, 0, None, 0, (2, 5), (5, 7),
                             pooling2=spelling)


# ---------------------------------------------------------------------------
# 6. gradient
# ---------------------------------------------------------------------------
def _step_binding(X, Neg, E, ctx, tim, p1, p2, lr=1.0, lam=0.0, opt=1):
    """One hhfm_hhfm_train_step_pool2 (default: SGD, lr 1, λ 0) -> loss, E after."""
    from hhfm_amd import ops
    from hhfm_amd._native import native
    B, ncols = X.shape
    M, k = E.shape
    Xd, Nd, Ed = _dev(X.astype(np.int32)), _dev(Neg.astype(np.int32)), _dev(E)
    ws = torch.zeros(native().train_workspace(M, k), dtype=torch.uint8, device="cuda")
    loss = torch.zeros(1, device="cuda")
    acc = torch.full((2 * M * k,), 0.1, device="cuda")
    native().hhfm_train_step_pool2(Xd.data_ptr() if B else 0, Nd.data_ptr() if B else 0, B, ncols,
                                   ctx[0], ctx[1], tim[0], tim[1], Neg.shape[1], Ed.data_ptr(), M,
                                   k, lr, lam, opt, acc.data_ptr(), ws.data_ptr(), ws.numel(),
                                   ops.pooling_word(p1), ops.pooling_word(p2), loss.data_ptr(),
                                   _stream())
    return float(loss.item()), Ed.cpu().numpy()


@pytest.mark.parametrize("name", sorted(tw.TWO_WAY_CASES))
def test_two_way_gradient_matches_float64(name):
    """hhfm_train_rows<TwoWayFeature>'s raw gradient, element by element: context
    only, time only, both; NG 1 .. 16; k = 4, 64, 128, 200; the planted rows of
    two_way_case (admissibility asserted in tests/test_hhfm_two_way_ref.py)."""
    X, Neg, E, ctx, tim, ties, p1, p2, _ = tw.two_way_case(name)
    ref_loss, dE, mE, info = tw.grad64(X, Neg, E, ctx, tim, ties, p1, p2)
    assert np.abs(info["z"]).max() <= 4 and info["margin"] > 1e-5
    loss, E1 = _step_binding(X, Neg, E, ctx, tim, p1, p2)
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    check_grad(f"hhfm two-way {name} E", E, E1, dE, mE)


# ---------------------------------------------------------------------------
# 7. loss and steps
# ---------------------------------------------------------------------------
def _data(Xb, Neg, fd, td):
    data = {"X": Xb[:, :2], "Y": Neg, "F1": Xb[:, 2:2 + fd]}
    if td:
        data["F2"] = Xb[:, 2 + fd:]
    return data


@pytest.mark.parametrize("six", [(MMM, MMM), MIXED], ids=_six_id)
@pytest.mark.parametrize("layout", ["frappe", "jiaju"])
def test_partial_fit_loss_is_loss64_plus_l2(layout, six):
    rng = np.random.default_rng(17)
    cards, td = STEP_LAYOUTS[layout]
    nu, ni, k, B, lam = 60, 200, 16, 300, 0.01
    fd = len(cards)
    ctx, tim = (2, 2 + fd), ((2 + fd, 2 + fd + td) if td else (0, 0))
    X, M = _rows(rng, B, nu, ni, cards, td)
    Neg = rng.integers(nu, nu + ni, (B, 10))
    E = rng.normal(0, 0.2, (M, k)).astype(np.float32)
    m = _our(fd, td, M, nu, ni, k, lam=lam, pooling=six[0], two_way=True, pooling2=six[1])
    m.set_weights(feature_embeddings=E)
    loss = m.partial_fit(_data(X.astype(np.int64), Neg, fd, td))
    want = tw.loss64(X, Neg, E, ctx, tim, *six) + lam * float((E.astype(np.float64) ** 2).sum()) / 2
    assert abs(loss - want) <= 1e-5 * abs(want), (loss, want)


REPLAY = [(ly, "AdagradOptimizer", 0.01, s) for ly in ("frappe", "jiaju")
          for s in ((MMM, MMM), MIXED)] + \
         [(ly, "AdamOptimizer", 0.0, s) for ly in ("frappe", "jiaju") for s in ((MMM, MMM), MIXED)]


@pytest.mark.parametrize("layout,opt,lam,six", REPLAY,
                         ids=lambda v: _six_id(v) if isinstance(v, tuple) else str(v))
def test_two_way_partial_fit_replayed(layout, opt, lam, six):
    """Three OUR.partial_fit steps, each replayed by the restated step from the
    GPU's own pre-step table and slot (test_pooled_partial_fit_replayed's bars)."""
    rng = np.random.default_rng(22)
    cards, td = STEP_LAYOUTS[layout]
    nu, ni, k, B = 300, 800, 32, 700
    fd = len(cards)
    ctx, tim = (2, 2 + fd), ((2 + fd, 2 + fd + td) if td else (0, 0))
    Xall, M = _rows(rng, 3 * B, nu, ni, cards, td)
    m = _our(fd, td, M, nu, ni, k, lam=lam, opt=opt, pooling=six[0], two_way=True,
             pooling2=six[1])
    m.set_weights(feature_embeddings=rng.normal(0, 0.2, (M, k)).astype(np.float32))
    o = OPTS[opt]
    for step in range(3):
        Xb = Xall[step * B:(step + 1) * B].astype(np.int64)
        Neg = rng.integers(nu, nu + ni, (B, 10))
        E = m.get_weights()["feature_embeddings"]
        (accE,) = _slots_of(m, ["feature_embeddings"], o, [E])
        loss = m.partial_fit(_data(Xb, Neg, fd, td))
        rl, E1, acc1 = tw.train_step2(Xb, Neg, E, accE, 0.1, lam, ctx, tim, *six, o, step + 1)
        _, Eg, _ = tw.train_step2(Xb, Neg, E, None, 1.0, lam, ctx, tim, *six, "sgd")
        assert np.isclose(loss, rl, rtol=1e-5)
        _check_var(m.get_weights()["feature_embeddings"], E1, E, o, E - Eg)
        _check_slot(m._train_state["feature_embeddings"].cpu().numpy(), acc1, o)


def test_two_way_empty_batch():
    """B = 0 behaves as the pooled empty step: with λ = 0 nothing moves and the
    loss is 0; with λ > 0 the table decays as hhfm_hhfm_train_step's does."""
    from hhfm_amd._native import native
    rng = np.random.default_rng(6)
    M, k = 60, 16
    E = rng.normal(0, 0.1, (M, k)).astype(np.float32)
    X0, N0 = np.zeros((0, 5), np.int32), np.zeros((0, 10), np.int32)
    loss, E1 = _step_binding(X0, N0, E, (2, 5), (0, 0), MMM, MMM, lr=0.1, lam=0.0, opt=0)
    assert loss == 0.0 and np.array_equal(E1.view(np.uint32), E.view(np.uint32))
    loss, E1 = _step_binding(X0, N0, E, (2, 5), (0, 0), MMM, MMM, lr=0.1, lam=0.5, opt=0)
    Ed = _dev(E)
    ws = torch.zeros(native().train_workspace(M, k), dtype=torch.uint8, device="cuda")
    l2 = torch.zeros(1, device="cuda")
    acc = torch.full((M * k,), 0.1, device="cuda")
    native().hhfm_train_step(0, 0, 0, 5, 2, 5, 0, 0, 10, Ed.data_ptr(), M, k, 0.1, 0.5, 0,
                             acc.data_ptr(), ws.data_ptr(), ws.numel(), l2.data_ptr(), _stream())
    assert np.array_equal(E1.view(np.uint32), Ed.cpu().numpy().view(np.uint32))
    want = 0.5 * 0.5 * float((E.astype(np.float64) ** 2).sum())
    assert np.isclose(loss, want, rtol=1e-5)


# ---------------------------------------------------------------------------
# 8. model surface
# ---------------------------------------------------------------------------
def test_module_attributes_take_effect_only_with_two_way(monkeypatch):
    from hhfm_amd import OurModel7 as M7
    rng = np.random.default_rng(10)
    X, M = _rows(rng, 300, 30, 90, (7, 2, 3), 0)
    E = rng.normal(0, 0.3, (M, 16)).astype(np.float32)

    def scores(**kw):
        m = M7.OUR(3, 0, M, 30, 90, 16, 0.1, 0.0, "AdagradOptimizer", True, False, **kw)
        m.set_weights(feature_embeddings=E)
        return m, m.score_rows(X)[:, 0]

    m0, base = scores()
    assert m0.pooling2 is None and not m0.two_way
    monkeypatch.setattr(M7, "Pooling2C", "max")
    monkeypatch.setattr(M7, "Pooling2F", "mean")
    assert np.array_equal(scores()[1], base)                       # ignored without two_way
    m1, got = scores(two_way=True)
    assert m1.pooling2 == ("max", "sum", "mean") and m1.pooling is None
    exact, mag = tw.exact_rows2(X, E, (2, 5), (0, 0), SSS, ("max", "sum", "mean"))
    kappa_check("two_way_module_attr", got, None, exact, mag)
    m2, over = scores(two_way=True, pooling2=SSS)                  # the keyword overrides
    assert m2.pooling2 == SSS
    exact, mag = tw.exact_rows2(X, E, (2, 5), (0, 0), SSS, SSS)
    kappa_check("two_way_keyword", over, None, exact, mag)
    assert not np.array_equal(over, base)                          # all-sum is still two-way
    assert np.array_equal(m1.score_rows(X)[:, 0], got)             # read at construction only
    assert np.array_equal(m1.sess.run(m1.PositiveFeadback,
                                      feed_dict={m1.Pos: X[:, :2], m1.Fea: X[:, 2:]})[:, 0], got)
    monkeypatch.setattr(M7, "Pooling2T", "median")
    with pytest.raises(ValueError):
        scores(two_way=True)
    scores()                                                       # still ignored
    for fd, td in ((1, 0), (3, 1)):
        with pytest.raises(ValueError):
            M7.OUR(fd, td, M, 30, 90, 16, 0.1, 0.0, "AdagradOptimizer", True, td > 0,
                   two_way=True, pooling2=SSS)


def test_train_loop_with_pooling2_end_to_end(tmp_path):
    """OurModel7.Train on synth_frappe with --pooling2 max (implies --two_way
    1), 2 epochs: the loss is finite and falling; afterwards score_rows is the
    restatement on the trained table, and is not the one-way model's."""
    from hhfm_amd import OurModel7 as M7
    argv = ["--path", GOLD + "/", "--epoch", "3", "--batch_size", "4096", "--pooling2", "max",
            "--Result", "1", "--result_file", str(tmp_path / "result.txt")]
    np.random.seed(2016)
    t = M7.M7_main("synth_frappe", 16, 5, argv)
    assert t.model.two_way and t.model.pooling2 == MMM and t.model.pooling is None
    assert len(t.loss_epoch) == 2 and np.all(np.isfinite(t.loss_epoch))
    assert t.loss_epoch[1] < t.loss_epoch[0]
    E = t.model.get_weights()["feature_embeddings"]
    X = t.data.Train_data.values[:2000, 1:].astype(np.int32)
    ctx, tim = t.model._ranges(X.shape[1])
    got = t.model.score_rows(X)[:, 0]
    exact, mag = tw.exact_rows2(X, E, ctx, tim, SSS, MMM)
    kappa_check("two_way_trained_rows", got, None, exact, mag)
    one, _ = pr.exact_rows(X, E, ctx, tim, SSS)
    print("two-way vs one-way on the trained table:",
          float(np.abs(exact - one).max() / mag.max()))
    assert np.abs(exact - one).max() > 1e-3 * mag.max()
    args = M7.parse_args("synth_frappe", 16, 5, ["--two_way", "1"])
    assert args.two_way == 1 and args.pooling2 is None
    for bad in ("min", "max,max", "max,sum,avg,sum"):
        with pytest.raises(ValueError):
            M7.parse_pooling(bad, "--pooling2")


def test_deterministic_two_way_raises_before_anything_runs():
    rng = np.random.default_rng(8)
    X, M = _rows(rng, 50, 30, 90, (7, 2, 3), 0)
    E = rng.normal(0, 0.1, (M, 16)).astype(np.float32)
    m = _our(3, 0, M, 30, 90, 16, deterministic=True, two_way=True)
    m.set_weights(feature_embeddings=E)
    data = {"X": X[:, :2].astype(np.int64), "F1": X[:, 2:].astype(np.int64),
            "Y": rng.integers(30, 120, (50, 10))}
    with pytest.raises(NotImplementedError):
        m.partial_fit(data)
    torch.cuda.synchronize()
    assert np.array_equal(m.get_weights()["feature_embeddings"].view(np.uint32), E.view(np.uint32))
    assert getattr(m, "_train_state", None) is None
