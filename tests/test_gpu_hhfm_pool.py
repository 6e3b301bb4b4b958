"""HHFM with MAX / MEAN pooling on the GPU (include/hhfm.h "Pooling"):
hybrid_rows_pool, the PoolFeature instantiations of hybrid_rows_generic and
catalog_queries, and hhfm_train_rows_pool against the numpy restatement of
tests/hhfm_pool_ref.py
(pinned on the CPU against the reference's own outputs and central
differences: tests/test_hhfm_pool_ref.py) and against the reference's outputs
themselves (tests/golden/hhfm_pool.npz, hhfm_pool_losses.npz).

Bars: row scores the project's score bar (1e-5 of Σ|terms|, and elementwise
where the condition number is at most 100: helpers.kappa_check); golden top-20
lists array_equal (the fixture keeps adjacent scores more than 1e-5 of Σ|terms|
apart); large catalogs by helpers.topk_tie_swaps, at most 2 float64-verified
ties per case; the raw gradient the per-element bound of
test_gpu_train_grad.py; optimizer steps the bars of test_gpu_training.py."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import fm_oracle as orc
from tests import hhfm_pool_ref as pr
from tests.helpers import bf16_round, kappa_check, topk_tie_swaps
from tests.test_gpu_train_grad import _check as check_grad
from tests.test_gpu_training import OPTS, _check_slot, _check_var, _slots_of
from tests.test_hhfm_pool_ref import GOLD, LAYOUTS, TRIPLES, golden_layout

pytestmark = pytest.mark.gpu
TRIPLES5 = TRIPLES + [("sum", "max", "mean")]
MAX_TIES = 2


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _table(E, dtype):
    """-> device table, and the values the kernel reads (bf16-rounded for bf16)."""
    if dtype == "bf16":
        return _dev(E).to(torch.bfloat16), bf16_round(E)
    return _dev(E), E


# ---------------------------------------------------------------------------
# row scores
# ---------------------------------------------------------------------------
# name: (context cardinalities, time columns); F = 2 + len(ctx) + time
ROW_LAYOUTS = {"F3": ((7,), 0), "F5": ((7, 2, 3), 0), "F10": ((5, 4, 6, 3, 7), 3),
               "F12": ((5, 4, 6, 3, 7), 5), "F9_generic": ((5, 4, 6, 3), 3),
               "noncanonical_generic": ((7, 2, 3), 0)}
WIDTHS = [(16, "f32"), (64, "f32"), (128, "f32"), (256, "f32"), (20, "f32"), (32, "bf16"),
          (128, "bf16")]


def _rows(rng, B, nu, ni, cards, td):
    cols = [rng.integers(0, nu, B), rng.integers(nu, nu + ni, B)]
    o = nu + ni
    for c in cards:
        cols.append(rng.integers(o, o + c, B))
        o += c
    for _ in range(td):
        cols.append(rng.integers(nu, nu + ni, B))
    return np.stack(cols, 1).astype(np.int32), o


@pytest.mark.parametrize("k,dtype", WIDTHS)
@pytest.mark.parametrize("layout", sorted(ROW_LAYOUTS))
def test_hybrid_score_rows_pool_parity(layout, k, dtype):
    """Every F x LPR path of hybrid_rows_pool the layouts and widths reach, the
    generic kernel (F = 9, a non-canonical column order, 80-byte rows), a
    partial last wave-iteration (B = 4,099) and B = 1, under five triples."""
    from hhfm_amd import ops
    cards, td = ROW_LAYOUTS[layout]
    rng = np.random.default_rng(len(layout) * 1000 + k)
    X, M = _rows(rng, 4099, 300, 900, cards, td)
    fd = len(cards)
    ctx, tim = (2, 2 + fd), ((2 + fd, 2 + fd + td) if td else (0, 0))
    ucol, icol = 0, 1
    if layout.startswith("noncanonical"):
        X = np.ascontiguousarray(X[:, [1, 0] + list(range(2, X.shape[1]))])
        ucol, icol = 1, 0
    Eg, E = _table(rng.normal(0, 0.01, (M, k)).astype(np.float32), dtype)
    Xd = _dev(X)
    for triple in TRIPLES5:
        got = ops.hybrid_score_rows(Xd, Eg, ucol, icol, ctx, tim, pooling=triple).cpu().numpy()
        exact, mag = pr.exact_rows(X, E, ctx, tim, triple, ucol, icol)
        ref = pr.score_rows(X, E, ctx, tim, triple, ucol, icol)
        kappa_check(f"pool_rows_{layout}_k{k}_{dtype}_{'_'.join(triple)}", got, ref, exact, mag)
        one = ops.hybrid_score_rows(Xd[:1], Eg, ucol, icol, ctx, tim, pooling=triple)
        assert abs(float(one.item()) - exact[0]) <= 1e-5 * mag[0]


@pytest.mark.parametrize("tag", LAYOUTS)
def test_hybrid_score_rows_pool_golden(tag):
    """The reference's own PositiveFeadback under the four golden triples."""
    from hhfm_amd import ops
    E, X, _, _, _, ctx, tim = golden_layout(tag)
    p = np.load(os.path.join(GOLD, "hhfm_pool.npz"))
    for triple in TRIPLES:
        got = ops.hybrid_score_rows(_dev(X), _dev(E), 0, 1, ctx, tim, pooling=triple)
        exact, mag = pr.exact_rows(X, E, ctx, tim, triple)
        ref = p[f"{tag}_{'_'.join(triple)}_out"]
        kappa_check(f"pool_rows_golden_{tag}_{'_'.join(triple)}", got.cpu().numpy(), ref, exact,
                    mag)


@pytest.mark.parametrize("k", [64, 20])
def test_hybrid_score_rows_pool_bad_id_flags_and_reads_row_0(k):
    from hhfm_amd import ops
    rng = np.random.default_rng(9)
    X, M = _rows(rng, 700, 300, 900, (7, 2, 3), 0)
    E = rng.normal(0, 0.01, (M, k)).astype(np.float32)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    mmm = ("max", "max", "max")
    ops.hybrid_score_rows(_dev(X), _dev(E), 0, 1, (2, 5), (0, 0), status=st, pooling=mmm)
    assert int(st.item()) == 0
    Xb = X.copy()
    Xb[5, 3], Xb[699, 0] = M + 7, -1
    got = ops.hybrid_score_rows(_dev(Xb), _dev(E), 0, 1, (2, 5), (0, 0), status=st, pooling=mmm)
    assert int(st.item()) & 1
    X0 = Xb.copy()
    X0[5, 3], X0[699, 0] = 0, 0
    ref = ops.hybrid_score_rows(_dev(X0), _dev(E), 0, 1, (2, 5), (0, 0), pooling=mmm)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_pooling_word_is_validated():
    """A mode value of 3, a bit above the three fields, and spellings the
    Python surface does not know."""
    from hhfm_amd import ops
    from hhfm_amd._native import native
    rng = np.random.default_rng(2)
    X, M = _rows(rng, 64, 30, 90, (7, 2, 3), 0)
    Xd, Ed = _dev(X), _dev(rng.normal(0, 0.01, (M, 16)).astype(np.float32))
    out = torch.full((64,), 7.0, device="cuda")
    for word in (3, 3 << 4, 3 << 8, 1 << 12, 1 | 1 << 30, -1):
        with pytest.raises(ValueError, match="invalid argument"):
            native().hybrid_score_rows_pool(Xd.data_ptr(), 64, 5, 0, 1, 2, 5, 0, 0, Ed.data_ptr(),
                                            M, 16, 0, out.data_ptr(), word, 0, _stream())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    for bad in (("max", "max"), ("max", "min", "sum"), "max", (1, 2, 3), (True, 0, 0)):
        with pytest.raises(ValueError):
            ops.hybrid_score_rows(Xd, Ed, 0, 1, (2, 5), (0, 0), pooling=bad)
    ok = ops.hybrid_score_rows(Xd, Ed, 0, 1, (2, 5), (0, 0),
                               pooling=(ops.POOL_MAX, ops.POOL_MEAN, ops.POOL_SUM))
    ref = ops.hybrid_score_rows(Xd, Ed, 0, 1, (2, 5), (0, 0), pooling=("max", "mean", "sum"))
    assert torch.equal(ok, ref)


@pytest.mark.parametrize("k,dtype", [(64, "f32"), (20, "f32"), (128, "bf16")])
def test_sum_pooling_through_the_new_entry_points_is_bit_identical(k, dtype):
    from hhfm_amd import ops
    rng = np.random.default_rng(k)
    X, M = _rows(rng, 4099, 300, 900, (5, 4, 6, 3, 7), 3)
    Eg, _ = _table(rng.normal(0, 0.01, (M, k)).astype(np.float32), dtype)
    sss = ("sum", "sum", "sum")
    a = ops.hybrid_score_rows(_dev(X), Eg, 0, 1, (2, 7), (7, 10))
    b = ops.hybrid_score_rows(_dev(X), Eg, 0, 1, (2, 7), (7, 10), pooling=sss)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if k % 8 == 0:
        ca = ops.catalog_topk(_dev(X[:70]), Eg, ops.MODE_HHFM, 20, 300, 900, 0, None, 0, (2, 7),
                              (7, 10))
        cb = ops.catalog_topk(_dev(X[:70]), Eg, ops.MODE_HHFM, 20, 300, 900, 0, None, 0, (2, 7),
                              (7, 10), pooling=sss)
        assert torch.equal(ca[1], cb[1]) and torch.equal(ca[0].view(torch.int32),
                                                         cb[0].view(torch.int32))


def test_sum_pooling_in_the_generic_pooled_kernel_is_bit_identical():
    """The all-sum word is 0 and is routed to the sum kernels, so the test above
    never runs hybrid_rows_generic over PoolFeature.  A layout without time
    columns with the word (sum, max, sum) does — the word is not 0, and the
    mode of the absent time pool changes nothing: h = (u + cv) + (-0) — at a
    width the register kernels decline (k = 72: 288-byte rows, 18 chunks).
    cv starts from -0 and the sum kernel's s from +0: the same bits unless the
    first context value is -0, which a normal table does not hold."""
    from hhfm_amd import ops
    rng = np.random.default_rng(72)
    X, M = _rows(rng, 64, 300, 900, (7, 2, 3), 0)
    Eg, _ = _table(rng.normal(0, 0.01, (M, 72)).astype(np.float32), "f32")
    a = ops.hybrid_score_rows(_dev(X), Eg, 0, 1, (2, 5), (0, 0))
    b = ops.hybrid_score_rows(_dev(X), Eg, 0, 1, (2, 5), (0, 0), pooling=("sum", "max", "sum"))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------
# catalog
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("triple", TRIPLES, ids="_".join)
@pytest.mark.parametrize("tag", LAYOUTS)
def test_catalog_topk_pool_golden(tag, triple):
    """The reference's own top-20 under every plan a small catalog can take;
    STORE and FUSED agree on the ids and on the score bits."""
    from hhfm_amd import ops
    E, _, A, nu, ni, ctx, tim = golden_layout(tag)
    p = np.load(os.path.join(GOLD, "hhfm_pool.npz"))
    key = f"{tag}_{'_'.join(triple)}"
    res = {}
    for name, plan in (("default", 0), ("store", ops.PLAN_STORE), ("fused", ops.PLAN_FUSED),
                       ("gemm", ops.PLAN_GEMM), ("exact", ops.PLAN_EXACT_FP32)):
        s, i = ops.catalog_topk(_dev(A), _dev(E), ops.MODE_HHFM, 20, nu, ni, 0, None, 0, ctx, tim,
                                plan=plan, pooling=triple)
        res[name] = (s.cpu().numpy(), i.cpu().numpy())
        assert np.array_equal(res[name][1], p[key + "_topk_idx"]), name
        ref = p[key + "_top21"][:, :20]
        assert np.abs(res[name][0] - ref).max() <= 1e-5 * np.abs(ref).max(), name
    assert np.array_equal(res["store"][1], res["fused"][1])
    assert np.array_equal(res["store"][0].view(np.uint32), res["fused"][0].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _big_catalog(n_item, dtype):
    """Seeded queries and table of a streaming-path catalog (k = 64, B = 130)
    with, per triple, the restated fp32 scores; built once per (size, dtype)."""
    rng = np.random.default_rng(n_item + len(dtype))
    A, M = _rows(rng, 130, 300, n_item, (5, 4, 6, 3, 7), 3)
    E = rng.normal(0, 0.01, (M, 64)).astype(np.float32)
    Er = bf16_round(E) if dtype == "bf16" else E
    ctx, tim = (2, 7), (7, 10)
    ref = {}
    for t in TRIPLES:
        h = pr.hybrid(Er, A, ctx, tim, t)
        sc = h @ Er[300:300 + n_item].T
        ah = pr._abs_hybrid(Er, A, ctx, tim, t)
        scale = (ah @ np.abs(Er[300:300 + n_item].astype(np.float64)).T).max(1, keepdims=True)
        ref[t] = (sc, scale, pr.exact_catalog(A, Er, 300, ctx, tim, t))
    return A, E, ctx, tim, ref


def _check_big(n_item, dtype, K, plan, triple):
    from hhfm_amd import ops
    A, E, ctx, tim, ref = _big_catalog(n_item, dtype)
    Eg, _ = _table(E, dtype)
    sc, scale, exact = ref[triple]
    s, i = ops.catalog_topk(_dev(A), Eg, ops.MODE_HHFM, K, 300, n_item, 0, None, 0, ctx, tim,
                            plan=plan, pooling=triple)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    _, ri = orc.top_k(sc, K)
    assert topk_tie_swaps(i, ri, exact) <= MAX_TIES
    picked = np.take_along_axis(sc, i.astype(np.int64), axis=1)
    assert np.all(np.abs(picked.astype(np.float64) - s) <= 1e-5 * scale)
    assert np.all(np.diff(s, axis=1) <= 0)


@pytest.mark.parametrize("plan", ["default", "no_seed", "no_ring"])
@pytest.mark.parametrize("K", [1, 20, 33])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_catalog_topk_pool_streaming_20000(dtype, K, plan):
    from hhfm_amd import ops
    flag = {"default": 0, "no_seed": ops.PLAN_NO_SEED, "no_ring": ops.PLAN_NO_RING}[plan]
    for triple in TRIPLES:
        _check_big(20000, dtype, K, flag, triple)


@pytest.mark.parametrize("plan", ["default", "no_seed", "no_ring"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_catalog_topk_pool_streaming_seed_and_ring(dtype, plan):
    """66,000 items: large enough for the threshold seed and the ring kernel
    (a 20,000-item catalog plans neither), so the pooled h feeds them too."""
    from hhfm_amd import ops
    flag = {"default": 0, "no_seed": ops.PLAN_NO_SEED, "no_ring": ops.PLAN_NO_RING}[plan]
    _check_big(66000, dtype, 20, flag, ("max", "max", "max"))
    _check_big(66000, dtype, 20, flag, ("mean", "max", "sum"))


@pytest.mark.parametrize("tag", LAYOUTS)
def test_catalog_scores_are_the_row_scores(tag):
    """What catalog_topk returns for (query, item) is what score_rows gives the
    row [user, that item, ctx, time], to 1e-5 of Σ|terms|."""
    from hhfm_amd import ops
    E, _, A, nu, ni, ctx, tim = golden_layout(tag)
    for triple in TRIPLES:
        s, i = ops.catalog_topk(_dev(A), _dev(E), ops.MODE_HHFM, 20, nu, ni, 0, None, 0, ctx, tim,
                                pooling=triple)
        rows = np.repeat(A, 20, axis=0)
        rows[:, 1] = nu + i.cpu().numpy().reshape(-1)
        r = ops.hybrid_score_rows(_dev(rows), _dev(E), 0, 1, ctx, tim, pooling=triple)
        _, mag = pr.exact_rows(rows, E, ctx, tim, triple)
        assert np.all(np.abs(r.cpu().numpy().astype(np.float64) - s.cpu().numpy().reshape(-1))
                      <= 1e-5 * mag)


def _our(fd, td, M, nu, ni, k, lr=0.1, lam=0.0, opt="AdagradOptimizer", **kw):
    from hhfm_amd.OurModel7 import OUR
    return OUR(fd, td, M, nu, ni, k, lr, lam, opt, True, td > 0, **kw)


@pytest.mark.parametrize("triple", [("max", "max", "max"), ("mean", "max", "sum")], ids="_".join)
def test_item_shards_merged_equal_model_topk(triple):
    """distributed.model_scorer's decomposition: 8 item shards through
    model.catalog_topk, merged by hhfm_topk_merge, against model.topk."""
    from hhfm_amd import ops
    E, _, A, nu, ni, ctx, tim = golden_layout("jiaju")
    m = _our(ctx[1] - 2, tim[1] - tim[0], E.shape[0], nu, ni, E.shape[1], pooling=triple)
    m.set_weights(feature_embeddings=E)
    whole = m.topk(A, 20)
    q = m._idx(A)
    bounds = np.linspace(0, ni, 9).astype(int)
    parts = [m.catalog_topk(q, int(b0), int(b1 - b0), 20) for b0, b1 in zip(bounds, bounds[1:])]
    _, ids = ops.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert np.array_equal(ids.cpu().numpy(), whole)
    p = np.load(os.path.join(GOLD, "hhfm_pool.npz"))
    assert np.array_equal(whole, p[f"jiaju_{'_'.join(triple)}_topk_idx"])


def test_mode_fm_with_pooling_is_refused():
    from hhfm_amd import ops
    rng = np.random.default_rng(4)
    X, M = _rows(rng, 40, 30, 90, (7, 2, 3), 0)
    Ed = _dev(rng.normal(0, 0.01, (M, 16)).astype(np.float32))
    w = _dev(rng.normal(0, 0.01, M).astype(np.float32))
    with pytest.raises(ValueError, match="invalid argument"):
        ops.catalog_topk(_dev(X), Ed, ops.MODE_FM, 5, 30, 90, 0, w, 0, (2, 5), (0, 0),
                         pooling=("max", "max", "max"))
    ops.catalog_topk(_dev(X), Ed, ops.MODE_FM, 5, 30, 90, 0, w, 0, (2, 5), (0, 0),
                     pooling=("sum", "sum", "sum"))


# ---------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------
def _step_binding(X, Neg, E, ctx, tim, pooling, lr=1.0, lam=0.0, opt=1):
    """One hhfm_hhfm_train_step_pool (default: SGD, lr 1, λ 0) -> loss, E after."""
    from hhfm_amd import ops
    from hhfm_amd._native import native
    B, ncols = X.shape
    M, k = E.shape
    Xd, Nd, Ed = _dev(X.astype(np.int32)), _dev(Neg.astype(np.int32)), _dev(E)
    ws = torch.zeros(native().train_workspace(M, k), dtype=torch.uint8, device="cuda")
    loss = torch.zeros(1, device="cuda")
    acc = torch.full((2 * M * k,), 0.1, device="cuda")
    native().hhfm_train_step_pool(Xd.data_ptr() if B else 0, Nd.data_ptr() if B else 0, B, ncols,
                                  ctx[0], ctx[1], tim[0], tim[1], Neg.shape[1], Ed.data_ptr(), M,
                                  k, lr, lam, opt, acc.data_ptr(), ws.data_ptr(), ws.numel(),
                                  ops.pooling_word(pooling), loss.data_ptr(), _stream())
    return float(loss.item()), Ed.cpu().numpy()


@pytest.mark.parametrize("name", sorted(pr.POOL_CASES))
def test_pooled_gradient_matches_float64(name):
    """hhfm_train_rows_pool's raw gradient, element by element: context only,
    time only, both, neither; NG 1 … 16; k = 4, 64, 128, 200; the planted rows
    of hhfm_pool_case (an id twice in a pool, twin rows, a field id equal to
    the user id, all-negative values) and of train_ref.hhfm_case."""
    X, Neg, E, ctx, tim, ties, pooling, _ = pr.hhfm_pool_case(name)
    ref_loss, dE, mE, info = pr.hhfm_pool_grad64(X, Neg, E, ctx, tim, ties, pooling)
    assert np.abs(info["z"]).max() <= 4 and info["margin"] > 1e-5
    loss, E1 = _step_binding(X, Neg, E, ctx, tim, pooling)
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    check_grad(f"hhfm pool {name} E", E, E1, dE, mE)


@pytest.mark.parametrize("triple", TRIPLES, ids="_".join)
@pytest.mark.parametrize("tag", ["frappe", "jiaju"])
def test_pooled_loss_equals_the_reference_loss(tag, triple):
    """OUR.partial_fit's returned loss against the reference graph's self.loss
    (the l2 term included), NG = 10 with a planted reduce_max tie."""
    L = np.load(os.path.join(GOLD, "hhfm_pool_losses.npz"))
    fd, td = int(L[f"{tag}_feature_dimension"]), int(L[f"{tag}_time_dimension"])
    E, X, Neg = L[f"{tag}_E"], L[f"{tag}_X"], L[f"{tag}_Neg"]
    m = _our(fd, td, E.shape[0], int(L["n_user"]), int(L["n_item"]), E.shape[1],
             lam=float(L["lamda"]), pooling=triple)
    m.set_weights(feature_embeddings=E)
    data = {"X": X[:, :2].astype(np.int64), "Y": Neg.astype(np.int64),
            "F1": X[:, 2:2 + fd].astype(np.int64)}
    if td:
        data["F2"] = X[:, 2 + fd:].astype(np.int64)
    loss = m.partial_fit(data)
    ref = float(L[f"{tag}_{'_'.join(triple)}_loss"])
    assert abs(loss - ref) <= 1e-5 * abs(ref), (loss, ref)


STEP_LAYOUTS = {"frappe": ((7, 2, 3), 0), "jiaju": ((5, 4, 6, 3, 7), 3)}


_T3 = [("max", "max", "max"), ("mean", "max", "sum"), ("sum", "mean", "max")]
REPLAY_CASES = ([(ly, "AdagradOptimizer", lam, t) for ly, lam in (("frappe", 0.01), ("jiaju", 0.0))
                 for t in _T3]
                + [(ly, "AdamOptimizer", 0.0, t) for ly in ("frappe", "jiaju") for t in _T3]
                + [("frappe", "AdamOptimizer", 0.01, ("mean", "max", "sum"))])


@pytest.mark.parametrize("layout,opt,lam,triple", REPLAY_CASES,
                         ids=lambda v: "_".join(v) if isinstance(v, tuple) else str(v))
def test_pooled_partial_fit_replayed(layout, opt, lam, triple):
    """Three OUR.partial_fit steps, each replayed by the restated step from the
    GPU's own pre-step table and slot (test_gpu_training._hhfm_replay's bars).
    Adam's bar also asks that at least 90 % of the non-zero gradient elements
    lie within 1e-2 of their table row's largest.  With λ > 0 an element a max
    pool did not select carries only λ·E, and the restated gradient alone
    gives 70 - 92 % there (85 %, 98 %, 92 % on frappe and 70 %, 92 %, 84 % on
    jiaju for the three triples; 98 % everywhere at λ = 0), so Adam runs at
    λ = 0 (the IndexedSlices rule) and with the dense l2 gradient under
    (mean, max, sum) on frappe; Adagrad covers the dense gradient under every
    triple."""
    rng = np.random.default_rng(21)
    cards, td = STEP_LAYOUTS[layout]
    nu, ni, k, B = 300, 800, 32, 700
    fd = len(cards)
    ctx, tim = (2, 2 + fd), ((2 + fd, 2 + fd + td) if td else (0, 0))
    Xall, M = _rows(rng, 3 * B, nu, ni, cards, td)
    m = _our(fd, td, M, nu, ni, k, lam=lam, opt=opt, pooling=triple)
    m.set_weights(feature_embeddings=rng.normal(0, 0.01, (M, k)).astype(np.float32))
    o = OPTS[opt]
    for step in range(3):
        Xb = Xall[step * B:(step + 1) * B].astype(np.int64)
        Neg = rng.integers(nu, nu + ni, (B, 10))
        E = m.get_weights()["feature_embeddings"]
        (accE,) = _slots_of(m, ["feature_embeddings"], o, [E])
        data = {"X": Xb[:, :2], "Y": Neg, "F1": Xb[:, 2:2 + fd]}
        if td:
            data["F2"] = Xb[:, 2 + fd:]
        loss = m.partial_fit(data)
        rl, E1, acc1 = pr.train_step(Xb, Neg, E, accE, 0.1, lam, ctx, tim, triple, o, step + 1)
        _, Eg, _ = pr.train_step(Xb, Neg, E, None, 1.0, lam, ctx, tim, triple, "sgd")
        assert np.isclose(loss, rl, rtol=1e-5)
        _check_var(m.get_weights()["feature_embeddings"], E1, E, o, E - Eg)
        _check_slot(m._train_state["feature_embeddings"].cpu().numpy(), acc1, o)


def test_pooled_empty_batch():
    """B = 0: with λ = 0 nothing moves and the loss is 0; with λ > 0 the table
    decays exactly as the unpooled entry point's empty step decays it."""
    from hhfm_amd._native import native
    rng = np.random.default_rng(6)
    M, k = 60, 16
    E = rng.normal(0, 0.1, (M, k)).astype(np.float32)
    X0, N0 = np.zeros((0, 5), np.int32), np.zeros((0, 10), np.int32)
    mmm = ("max", "max", "max")
    loss, E1 = _step_binding(X0, N0, E, (2, 5), (0, 0), mmm, lr=0.1, lam=0.0, opt=0)
    assert loss == 0.0 and np.array_equal(E1.view(np.uint32), E.view(np.uint32))
    loss, E1 = _step_binding(X0, N0, E, (2, 5), (0, 0), mmm, lr=0.1, lam=0.5, opt=0)
    Ed = _dev(E)
    ws = torch.zeros(native().train_workspace(M, k), dtype=torch.uint8, device="cuda")
    l2 = torch.zeros(1, device="cuda")
    acc = torch.full((M * k,), 0.1, device="cuda")
    native().hhfm_train_step(0, 0, 0, 5, 2, 5, 0, 0, 10, Ed.data_ptr(), M, k, 0.1, 0.5, 0,
                             acc.data_ptr(), ws.data_ptr(), ws.numel(), l2.data_ptr(), _stream())
    assert not np.array_equal(E1, E)
    assert np.array_equal(E1.view(np.uint32), Ed.cpu().numpy().view(np.uint32))
    # the l2 term alone (its Σ var² is a float-atomic sum: equal to rounding, not to the bit)
    want = 0.5 * 0.5 * float((E.astype(np.float64) ** 2).sum())
    assert np.isclose(loss, want, rtol=1e-5) and np.isclose(float(l2.item()), want, rtol=1e-5)


def test_train_loop_with_pooling_end_to_end(tmp_path):
    """OurModel7.Train on synth_frappe with --pooling max, 2 epochs; afterwards
    score_rows is the restatement on the trained table, and is not sum pooling's."""
    from hhfm_amd import OurModel7 as M7
    argv = ["--path", GOLD + "/", "--epoch", "3", "--batch_size", "4096", "--pooling", "max",
            "--Result", "1", "--result_file", str(tmp_path / "result.txt")]
    np.random.seed(2016)
    t = M7.M7_main("synth_frappe", 16, 5, argv)
    assert t.model.pooling == ("max", "max", "max")
    assert len(t.loss_epoch) == 2 and np.all(np.isfinite(t.loss_epoch))
    assert t.loss_epoch[1] < t.loss_epoch[0]
    E = t.model.get_weights()["feature_embeddings"]
    X = t.data.Train_data.values[:2000, 1:].astype(np.int32)
    ctx, tim = t.model._ranges(X.shape[1])
    got = t.model.score_rows(X)[:, 0]
    exact, mag = pr.exact_rows(X, E, ctx, tim, ("max", "max", "max"))
    kappa_check("pool_trained_rows", got, None, exact, mag)
    s_exact, _ = pr.exact_rows(X, E, ctx, tim, ("sum", "sum", "sum"))
    assert np.abs(exact - s_exact).max() > 1e-3 * mag.max()
    for bad in ("min", "max,max", "max,sum,avg,sum"):
        with pytest.raises(ValueError):
            M7.parse_pooling(bad)


def test_deterministic_with_pooling_raises_before_anything_runs():
    rng = np.random.default_rng(8)
    X, M = _rows(rng, 50, 30, 90, (7, 2, 3), 0)
    E = rng.normal(0, 0.1, (M, 16)).astype(np.float32)
    m = _our(3, 0, M, 30, 90, 16, deterministic=True, pooling=("max", "sum", "sum"))
    m.set_weights(feature_embeddings=E)
    data = {"X": X[:, :2].astype(np.int64), "F1": X[:, 2:].astype(np.int64),
            "Y": rng.integers(30, 120, (50, 10))}
    with pytest.raises(NotImplementedError):
        m.partial_fit(data)
    torch.cuda.synchronize()
    assert np.array_equal(m.get_weights()["feature_embeddings"].view(np.uint32), E.view(np.uint32))
    assert getattr(m, "_train_state", None) is None
    # sum pooling keeps its deterministic step
    d = _our(3, 0, M, 30, 90, 16, deterministic=True)
    d.set_weights(feature_embeddings=E)
    assert np.isfinite(d.partial_fit(data))


def test_module_attributes_select_the_pooling(monkeypatch):
    """OurModel7.Pooling1C / 1T / 1F are read when OUR is constructed, as the
    reference reads its module constants; Pooling2* are ignored; the keyword
    overrides them."""
    from hhfm_amd import OurModel7 as M7
    rng = np.random.default_rng(10)
    X, M = _rows(rng, 300, 30, 90, (7, 2, 3), 0)
    E = rng.normal(0, 0.1, (M, 16)).astype(np.float32)

    def scores(**kw):
        m = M7.OUR(3, 0, M, 30, 90, 16, 0.1, 0.0, "AdagradOptimizer", True, False, **kw)
        m.set_weights(feature_embeddings=E)
        return m, m.score_rows(X)[:, 0]

    m0, base = scores()
    assert m0.pooling is None
    monkeypatch.setattr(M7, "Pooling2C", "max")
    monkeypatch.setattr(M7, "Pooling2F", "mean")
    assert np.array_equal(scores()[1], base)
    monkeypatch.setattr(M7, "Pooling1C", "max")
    m1, got = scores()
    assert m1.pooling == ("max", "sum", "sum") and not np.array_equal(got, base)
    exact, mag = pr.exact_rows(X, E, (2, 5), (0, 0), ("max", "sum", "sum"))
    kappa_check("pool_module_attr", got, None, exact, mag)
    m2, over = scores(pooling=("sum", "sum", "sum"))
    assert m2.pooling is None and np.array_equal(over, base)
    assert np.array_equal(m0.score_rows(X)[:, 0], base)      # read at construction only
    monkeypatch.setattr(M7, "Pooling1F", "median")
    with pytest.raises(ValueError):
        scores()
