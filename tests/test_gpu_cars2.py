"""CARS2 on the GPU (include/hhfm.h "CARS2"): hhfm_cars2_prepare / _score_rows /
_catalog_topk / _train_step and the hhfm_amd.CARS2 surface against
tests/cars2_ref.py (the reference's op order in float32 and float64) and the
reference's own outputs in tests/golden/cars2.npz.

Bars: row and catalog scores at the project's score bar (helpers.kappa_check;
1e-5 of Σ|elementary products|), index lists array_equal on the gap-clean
fixture and within MAX_TIES float64-verified ties on the large catalogs
(helpers.topk_tie_swaps; tests/test_cars2_ref.py holds cars2_ref itself to the
same cap on the CPU), raw gradients under test_gpu_train_grad._check's
per-element bound, optimizer replays under test_gpu_training._check_var /
_check_slot, the loss to 1e-5 relative.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import cars2_ref as cr
from tests.helpers import bf16_round, kappa_check, topk_tie_swaps
from tests.test_gpu_train_grad import _check
from tests.test_gpu_training import OPTS, _check_slot, _check_var, _slot

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
GOLD = np.load(os.path.join(G, "cars2.npz"))
NU, NI, MC = int(GOLD["n_user"]), int(GOLD["n_item"]), int(GOLD["Mc"])


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _table(UI, dtype):
    """-> (device table in its storage dtype, the float32 values it holds)."""
    if dtype == "bf16":
        return _dev(UI).to(torch.bfloat16).contiguous(), bf16_round(UI)
    return _dev(UI), UI


def _prepare(Wt):
    from hhfm_amd import ops
    return ops.cars2_prepare(*(_dev(Wt[k]) for k in ("Context", "W", "Z", "A", "B")))


def _rows(rng, B, n_user, n_item, Mc):
    return np.stack([rng.integers(0, n_user, B), rng.integers(n_user, n_user + n_item, B),
                     rng.integers(0, Mc, B)], 1).astype(np.int32)


def golden(D):
    p = f"d{D}_"
    g = {k[len(p):]: GOLD[k] for k in GOLD.files if k.startswith(p)}
    return cr.weights(int(g["seed"]), NU + NI, MC, D), g


def _model(Wt, n_user, n_item, lam=0.0, opt="AdagradOptimizer", lr=0.01, **kw):
    from hhfm_amd.CARS2 import CARS2
    m = CARS2(Wt["Context"].shape[0], n_user, n_item, Wt["UI"].shape[1], lr, lam, opt, **kw)
    m.set_weights(**Wt)
    return m


# ---------------------------------------------------------------------------
# 1. known answer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_known_answer(dtype):
    """D = 8 (Dc 3, Dp 1, Dq 3), small integers x 1/2: every product and sum,
    in the folded association too, is exact in fp32 (|numerators| < 2^12 over
    2^4) and every UI value exact in bf16, so the scores are compared with ==."""
    from hhfm_amd import ops
    assert cr.dims(8) == (3, 1, 3)
    r = np.random.RandomState(8)
    ints = lambda *s: (r.randint(-3, 4, s) * 0.5).astype(np.float32)   # noqa: E731
    Wt = dict(UI=ints(5, 8), Context=ints(2, 3), W=ints(8, 1, 3), Z=ints(8, 3, 3), A=ints(1),
              B=ints(3))
    Wt["A"][:] = 1.5
    X = np.array([[0, 3, 1]], np.int32)
    want = cr.score_rows(X, Wt, np.float64)[0, 0]
    ui = (Wt["UI"][0].astype(np.float64) * Wt["UI"][3]).sum()
    assert want != ui and want == np.float32(want)
    UId, held = _table(Wt["UI"], dtype)
    assert np.array_equal(held, Wt["UI"])
    got = ops.cars2_score_rows(_dev(X), UId, _prepare(Wt), 2).cpu().numpy()
    assert got[0] == want
    zero = dict(Wt, A=np.zeros(1, np.float32), B=np.zeros(3, np.float32))
    got = ops.cars2_score_rows(_dev(X), UId, _prepare(zero), 2).cpu().numpy()
    assert got[0] == ui


# ---------------------------------------------------------------------------
# 2. row parity
# ---------------------------------------------------------------------------
WIDTHS = [(16, "f32"), (64, "f32"), (128, "f32"), (20, "f32"), (16, "bf16"), (128, "bf16")]


@pytest.mark.parametrize("Mc", [11, 3000])
@pytest.mark.parametrize("D,dtype", WIDTHS)
def test_score_rows_parity(D, dtype, Mc):
    """Every width the chunked kernel has (D = 20: Dc 8, Dp 4, the generic
    kernel), B = 4,099 (a partial last wave-iteration) and B = 1, GA / GB of 11
    rows and of 3,000; std 0.3 with non-zero A and B, where the trilinear terms
    carry well over 10 % of Σ|terms| (asserted)."""
    from hhfm_amd import ops
    nu, ni = 300, 900
    Wt = cr.weights(1000 + D + Mc, nu + ni, Mc, D)
    UId, held = _table(Wt["UI"], dtype)
    Wr = dict(Wt, UI=held)
    prepared = _prepare(Wt)
    rng = np.random.default_rng(D + Mc)
    for B in (4099, 1):
        X = _rows(rng, B, nu, ni, Mc)
        exact, mag, share = cr.exact_rows(X, Wr)
        assert share.min() >= 0.1
        got = ops.cars2_score_rows(_dev(X), UId, prepared, Mc).cpu().numpy()
        kappa_check(f"cars2_rows D{D} {dtype} Mc{Mc} B{B}", got, cr.score_rows(X, Wr)[:, 0],
                    exact, mag)


@pytest.mark.parametrize("D", [16, 20])
def test_bad_ids_flag_and_read_row_0(D):
    """A user, an item and a context id out of range (chunked and generic
    kernel): the status bit, and the bits of the same rows with those ids 0."""
    from hhfm_amd import ops
    nu, ni, Mc = 30, 60, 5
    Wt = cr.weights(77, nu + ni, Mc, D)
    X = _rows(np.random.default_rng(3), 300, nu, ni, Mc)
    bad = X.copy()
    bad[7, 0], bad[130, 1], bad[299, 2] = nu + ni, -1, Mc
    zeroed = bad.copy()
    zeroed[7, 0] = zeroed[130, 1] = zeroed[299, 2] = 0
    prepared, UId = _prepare(Wt), _dev(Wt["UI"])
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    clean = ops.cars2_score_rows(_dev(zeroed), UId, prepared, Mc, status=st)
    assert int(st.item()) == 0
    got = ops.cars2_score_rows(_dev(bad), UId, prepared, Mc, status=st)
    assert int(st.item()) == 1
    assert torch.equal(got.view(torch.int32), clean.view(torch.int32))
    for col in range(3):                                   # each range alone
        one = zeroed.copy()
        one[11, col] = bad[[7, 130, 299][col], col]
        st.zero_()
        ops.cars2_score_rows(_dev(one), UId, prepared, Mc, status=st)
        assert int(st.item()) == 1, col
    m = _model(Wt, nu, ni)
    with pytest.raises(ValueError):
        m.score_rows(bad)
    with pytest.raises(ValueError):
        m.score_rows(bad.astype(np.int64))
    with pytest.raises(ValueError):
        m.topk({"X": np.array([0, 1]), "F1": np.array([0, Mc])}, 5)


# ---------------------------------------------------------------------------
# 3. the reference's own outputs, through the class
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 64])
def test_golden_rows_and_topk(D):
    Wt, g = golden(D)
    m = _model(Wt, NU, NI)
    X = g["X"].astype(np.int64)
    got = m.sess.run(m.PositiveFeadback, feed_dict={m.Pos: X[:, :2], m.Fea: X[:, 2]})
    assert got.shape == (64, 1)
    exact, mag, _ = cr.exact_rows(X, Wt)
    kappa_check(f"cars2_golden_rows D{D}", got[:, 0], g["out"], exact, mag)
    assert np.all(np.abs(got[:, 0].astype(np.float64) - g["out"]) <= 1e-5 * mag)
    q = g["q"].astype(np.int64)
    assert np.array_equal(m.topk({"X": q[:, 0], "F1": q[:, 1]}, 20), g["topk_idx"])
    assert np.array_equal(m.topk(q, 20), g["topk_idx"])
    # set_weights invalidates the prepared tables
    m.set_weights(B=np.zeros_like(Wt["B"]), A=np.zeros_like(Wt["A"]))
    ui = (Wt["UI"][X[:, 0]].astype(np.float64) * Wt["UI"][X[:, 1]]).sum(1)
    assert np.allclose(m.score_rows(X)[:, 0], ui, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("plan", ["default", "exact", "gemm"])
@pytest.mark.parametrize("D", [16, 64])
def test_catalog_scores_are_the_row_scores(D, plan):
    """K = N: every (query, item) score of the catalog against the row kernel's
    score of that row and the float64 value, at the score bar."""
    from hhfm_amd import ops
    flag = {"default": 0, "exact": ops.PLAN_EXACT_FP32, "gemm": ops.PLAN_GEMM}[plan]
    Wt, g = golden(D)
    q = g["q"].astype(np.int32)
    prepared, UId = _prepare(Wt), _dev(Wt["UI"])
    s, i = ops.cars2_catalog_topk(_dev(q), UId, prepared, MC, NI, NU, NI, plan=flag)
    s, i = s.cpu().numpy().reshape(-1), i.cpu().numpy()
    assert all(sorted(r) == list(range(NI)) for r in i)
    rows = np.stack([np.repeat(q[:, 0], NI), NU + i.reshape(-1), np.repeat(q[:, 1], NI)], 1)
    r = ops.cars2_score_rows(_dev(rows.astype(np.int32)), UId, prepared, MC).cpu().numpy()
    exact, mag, _ = cr.exact_rows(rows, Wt)
    assert np.all(np.abs(r.astype(np.float64) - s) <= 1e-5 * mag)
    assert np.all(np.abs(s - exact) <= 1e-5 * mag)


# ---------------------------------------------------------------------------
# 4. large catalogs: dense (N = 4,082, B = 300) and streaming (N = 20,000, B = 130)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _catalog(name, dtype):
    Wt, q, nu, ni = cr.catalog_case(name, dtype == "bf16")
    return (Wt, q, nu, ni, cr.catalog_reference(Wt, q, nu, ni), cr.catalog_mag(Wt, q, nu, ni),
            cr.exact_catalog(q, Wt, nu))


@pytest.mark.parametrize("plan", ["default", "exact"])
@pytest.mark.parametrize("K", [20, 64])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["dense", "stream"])
def test_catalog_topk_large(name, dtype, K, plan):
    from hhfm_amd import ops
    flag = {"default": 0, "exact": ops.PLAN_EXACT_FP32}[plan]
    Wt, q, nu, ni, sc, mag, exact = _catalog(name, dtype)
    UId = _dev(Wt["UI"]).to(torch.bfloat16) if dtype == "bf16" else _dev(Wt["UI"])
    s, i = ops.cars2_catalog_topk(_dev(q), UId.contiguous(), _prepare(Wt), Wt["Context"].shape[0],
                                  K, nu, ni, plan=flag)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    _, ri = cr.top_k(sc, K)
    assert topk_tie_swaps(i, ri, exact) <= cr.MAX_TIES
    picked = np.take_along_axis(sc, i.astype(np.int64), axis=1)
    assert np.all(np.abs(picked.astype(np.float64) - s) <= 1e-5 * mag)
    assert np.all(np.diff(s, axis=1) <= 0)


def test_item_shards_merged_equal_model_topk():
    from hhfm_amd import ops
    Wt, g = golden(64)
    m = _model(Wt, NU, NI)
    q = g["q"].astype(np.int64)
    whole = m.topk(q, 20)
    qd = m._idx(q)
    parts = [m.catalog_topk(qd, b0, b1 - b0, 20) for b0, b1 in ((0, 30), (30, NI))]
    _, ids = ops.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert np.array_equal(ids.cpu().numpy(), whole)
    assert np.array_equal(whole, g["topk_idx"])


def test_unsupported_width_is_refused_like_the_hhfm_catalog():
    from hhfm_amd import ops
    nu, ni, Mc, D = 20, 50, 4, 20
    Wt = cr.weights(20, nu + ni, Mc, D)
    q = np.array([[0, 1], [3, 2]], np.int32)
    with pytest.raises(ValueError) as ours:
        ops.cars2_catalog_topk(_dev(q), _dev(Wt["UI"]), _prepare(Wt), Mc, 5, nu, ni)
    A = np.array([[0, nu, nu + 1]], np.int32)
    with pytest.raises(ValueError) as theirs:
        ops.catalog_topk(_dev(A), _dev(Wt["UI"]), ops.MODE_HHFM, 5, nu, ni, 0, None, 0, (2, 3))
    tail = lambda e: str(e.value).split(": ", 1)[1]   # noqa: E731
    assert tail(ours) == tail(theirs) and "unsupported" in tail(ours).lower()


# ---------------------------------------------------------------------------
# 5. training
# ---------------------------------------------------------------------------
GRAD_STD = 0.15      # |x| stays below 4: σ(x) − 1 then loses <= ~3e-6 to cancellation


def _grad_case(D, NG, B):
    nu, ni, Mc = 20, 40, 7
    Wt = cr.weights(7 * D + NG, nu + ni, Mc, D, GRAD_STD)
    r = np.random.RandomState(100 * NG + B)
    X = np.stack([r.randint(0, nu, B), r.randint(nu, nu + ni, B)], 1)
    Fea = r.randint(0, Mc, B)
    Neg = r.randint(nu, nu + ni, (B, NG))
    if NG > 1:
        Neg[0, 1] = Neg[0, 0]            # a repeated negative id
    Neg[B - 1, NG - 1] = X[B - 1, 1]     # a negative equal to the positive item
    return Wt, X, Fea, Neg, nu, ni


@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("NG", [1, 3, 16])
@pytest.mark.parametrize("D", [16, 64])
def test_gradient_matches_float64(D, NG, B):
    """One GradientDescentOptimizer step at lr 1, λ 0: before − after is the raw
    gradient the kernels formed."""
    Wt, X, Fea, Neg, nu, ni = _grad_case(D, NG, B)
    ref_loss, Gd, Mg, x = cr.grad64(X, Fea, Neg, Wt)
    assert np.abs(x).max() <= 4
    m = _model(Wt, nu, ni, lam=0.0, opt="GradientDescentOptimizer", lr=1.0)
    loss = m.partial_fit({"X": X, "Y": Neg, "F1": Fea})
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    after = m.get_weights()
    for name in ("UI", "Context", "Z", "B"):
        _check(f"cars2 D{D} NG{NG} B{B} {name}", Wt[name], after[name], Gd[name], Mg[name])
    for name in ("W", "A"):
        assert np.array_equal(after[name].view(np.uint32), Wt[name].view(np.uint32)), name


def test_reference_init_known_answer():
    """From A = B = 0 (CARS2.py:160-163) one SGD step at λ = 0 leaves W, A and
    Z bit-unchanged (dZ = B_q·T) and moves B."""
    nu, ni, Mc, D, B = 20, 40, 7, 16, 64
    Wt = cr.weights(5, nu + ni, Mc, D, 0.3, ab=False)
    r = np.random.RandomState(6)
    data = {"X": np.stack([r.randint(0, nu, B), r.randint(nu, nu + ni, B)], 1),
            "Y": r.randint(nu, nu + ni, (B, 1)), "F1": r.randint(0, Mc, B)}
    m = _model(Wt, nu, ni, lam=0.0, opt="GradientDescentOptimizer", lr=1.0)
    m.partial_fit(data)
    after = m.get_weights()
    for name in ("W", "A", "Z"):
        assert np.array_equal(after[name].view(np.uint32), Wt[name].view(np.uint32)), name
    assert np.all(after["B"] != 0)
    _, Gd, Mg, _ = cr.grad64(data["X"], data["F1"], data["Y"], Wt)
    _check("cars2 init B", Wt["B"], after["B"], Gd["B"], Mg["B"])


@pytest.mark.parametrize("lam,tag", [(0.001, "1e-3"), (0.0, "0")])
@pytest.mark.parametrize("ng", [1, 3])
@pytest.mark.parametrize("D", [16, 64])
def test_partial_fit_loss_is_the_references(D, ng, lam, tag):
    Wt, g = golden(D)
    X = g["X"].astype(np.int64)
    m = _model(Wt, NU, NI, lam=lam)
    loss = m.partial_fit({"X": X[:, :2], "Y": g[f"Neg{ng}"].astype(np.int64), "F1": X[:, 2]})
    want = float(g[f"loss_ng{ng}_lam{tag}"])
    assert abs(loss - want) <= 1e-5 * abs(want), (loss, want)


@pytest.mark.parametrize("lam", [0.0, 0.001])
@pytest.mark.parametrize("opt", sorted(OPTS))
def test_partial_fit_replayed(opt, lam):
    """Three steps, each replayed by cars2_ref.train_step from the GPU's own
    pre-step variables and slots: every variable and every slot."""
    nu, ni, Mc, D, B, NG, lr = 40, 90, 9, 16, 300, 2, 0.05
    o = OPTS[opt]
    m = _model(cr.weights(31, nu + ni, Mc, D, 0.2), nu, ni, lam=lam, opt=opt, lr=lr)
    r = np.random.RandomState(32)
    for step in range(3):
        X = np.stack([r.randint(0, nu, B), r.randint(nu, nu + ni, B)], 1)
        Fea, Neg = r.randint(0, Mc, B), r.randint(nu, nu + ni, (B, NG))
        cur = m.get_weights()
        st = getattr(m, "_train_state", None)
        slots = {n: (_slot(o, cur[n]) if st is None or o == "sgd" else st[n].cpu().numpy())
                 for n in cr.NAMES}
        loss = m.partial_fit({"X": X, "Y": Neg, "F1": Fea})
        rl, new, ns = cr.train_step(X, Fea, Neg, cur, slots, lr, lam, o, step + 1)
        _, sgd, _ = cr.train_step(X, Fea, Neg, cur, {n: None for n in cr.NAMES}, 1.0, lam, "sgd")
        assert np.isclose(loss, rl, rtol=1e-5), (loss, rl)
        got = m.get_weights()
        for n in cr.NAMES:
            if n in ("W", "A") and lam == 0:       # a zero gradient: nothing moves
                assert np.array_equal(got[n].view(np.uint32), cur[n].view(np.uint32)), n
                continue
            _check_var(got[n], new[n], cur[n], o, cur[n] - sgd[n])
            if o != "sgd":
                _check_slot(m._train_state[n].cpu().numpy(), ns[n], o)


def _adam_powers(m):
    from hhfm_amd._native import native
    W = m.weights
    n_ui, D = W["UI"].shape
    Mc, Dc = W["Context"].shape
    nbytes = native().cars2_train_state_bytes(n_ui, Mc, D, Dc, W["W"].shape[1], W["Z"].shape[1])
    ws = m._train_state["ws"][:nbytes].cpu().numpy().view(np.float32)
    # the scalar block is the 64-float region before the two touched masks
    off = nbytes // 4 - 64 * ((n_ui + 255) // 256) - 64 * ((Mc + 255) // 256) - 64
    return ws[off + 8:off + 11]


@pytest.mark.parametrize("opt", ["AdagradOptimizer", "AdamOptimizer"])
def test_empty_batch(opt):
    """B = 0: with λ > 0 all six variables decay as the replay says and Adam's
    powers advance; with λ = 0 nothing moves and the loss is 0."""
    nu, ni, Mc, D = 20, 40, 7, 16
    Wt = cr.weights(41, nu + ni, Mc, D, 0.2)
    empty = {"X": np.zeros((0, 2), np.int64), "Y": np.zeros((0, 1), np.int64),
             "F1": np.zeros(0, np.int64)}
    m = _model(Wt, nu, ni, lam=0.0, opt=opt)
    assert m.partial_fit(empty) == 0.0
    after = m.get_weights()
    for n in cr.NAMES:
        assert np.array_equal(after[n].view(np.uint32), Wt[n].view(np.uint32)), n
    lam, o = 0.5, OPTS[opt]
    m = _model(Wt, nu, ni, lam=lam, opt=opt, lr=0.05)
    loss = m.partial_fit(empty)
    slots = {n: _slot(o, Wt[n]) for n in cr.NAMES}
    rl, new, ns = cr.train_step(empty["X"], empty["F1"], empty["Y"], Wt, slots, 0.05, lam, o, 1)
    assert np.isclose(loss, rl, rtol=1e-5) and loss > 0
    after = m.get_weights()
    for n in cr.NAMES:
        assert not np.array_equal(after[n], Wt[n]), n
        assert np.allclose(after[n], new[n], rtol=1e-5, atol=1e-7), n
        _check_slot(m._train_state[n].cpu().numpy(), ns[n], o)
    if opt == "AdamOptimizer":
        b1, b2, started = _adam_powers(m)
        assert started == 1.0 and b1 == np.float32(0.9) * np.float32(0.9)
        assert b2 == np.float32(0.999) * np.float32(0.999)


class _Step:
    """The binding's arguments for one step on seeded device arrays."""

    def __init__(self, B=8, NG=1, D=16, opt=0):
        from hhfm_amd._native import native
        self.nat = native()
        self.nu, self.ni, self.Mc, self.D, self.B, self.NG, self.opt = 20, 40, 7, D, B, NG, opt
        self.Dc, self.Dp, self.Dq = cr.dims(D)
        self.Wt = cr.weights(51, 60, 7, D, 0.2)
        self.dev = {k: _dev(v) for k, v in self.Wt.items()}
        r = np.random.RandomState(52)
        self.X = _dev(np.stack([r.randint(0, 20, B), r.randint(20, 60, B)], 1).astype(np.int32))
        self.Fea = _dev(r.randint(0, 7, B).astype(np.int32))
        self.Neg = _dev(r.randint(20, 60, (B, NG)).astype(np.int32))
        self.acc = [torch.full((v.numel(),), 0.1, device="cuda") for v in self.dev.values()]
        self.loss = torch.full((1,), -7.0, device="cuda")
        n = self.nat.cars2_train_workspace(B, 60, 7, D, self.Dc, self.Dp, self.Dq)
        self.ws = torch.zeros(n, dtype=torch.uint8, device="cuda")

    def run(self, ws_bytes=None, null=None, NG=None):
        p = {k: (0 if k == null else v.data_ptr()) for k, v in self.dev.items()}
        self.nat.cars2_train_step(
            self.X.data_ptr(), self.Fea.data_ptr(), self.Neg.data_ptr(), self.B,
            self.NG if NG is None else NG, p["UI"], 60, p["Context"], 7, p["W"], p["Z"], p["A"],
            p["B"], self.D, self.Dc, self.Dp, self.Dq, 0.1, 0.01, self.opt,
            [a.data_ptr() for a in self.acc], self.ws.data_ptr(),
            self.ws.numel() if ws_bytes is None else ws_bytes, self.loss.data_ptr(), _stream())

    def untouched(self):
        torch.cuda.synchronize()
        ok = all(np.array_equal(self.dev[k].cpu().numpy().view(np.uint32),
                                self.Wt[k].view(np.uint32)) for k in cr.NAMES)
        return (ok and float(self.loss.item()) == -7.0 and not bool(self.ws.any())
                and all(bool((a == 0.1).all()) for a in self.acc))


def test_refusals_leave_everything_untouched():
    s = _Step(NG=16)
    with pytest.raises(ValueError, match="unsupported"):
        s.run(NG=17)
    assert s.untouched()
    s = _Step()
    with pytest.raises(ValueError, match="workspace"):
        s.run(ws_bytes=s.ws.numel() - 1)
    assert s.untouched()
    for name in cr.NAMES:
        with pytest.raises(ValueError, match="invalid"):
            s.run(null=name)
        assert s.untouched(), name
    s.run()                                         # the same arguments do step
    torch.cuda.synchronize()
    assert float(s.loss.item()) > 0 and not s.untouched()


def test_deterministic_and_bf16_training_are_refused():
    Wt, g = golden(16)
    X = g["X"].astype(np.int64)
    data = {"X": X[:, :2], "Y": g["Neg1"].astype(np.int64), "F1": X[:, 2]}
    for kw, err in ((dict(deterministic=True), NotImplementedError),
                    (dict(table_dtype=torch.bfloat16), NotImplementedError)):
        m = _model(Wt, NU, NI, **kw)
        with pytest.raises(err):
            m.partial_fit(data)
        after = m.get_weights()
        for n in cr.NAMES:
            assert np.array_equal(after[n].view(np.uint32), Wt[n].view(np.uint32)), n
        assert getattr(m, "_train_state", None) is None
    # scoring on the bf16 table still works
    exact, mag, _ = cr.exact_rows(X, dict(Wt, UI=bf16_round(Wt["UI"])))
    kappa_check("cars2_bf16_class_rows", m.score_rows(X)[:, 0], None, exact, mag)


# ---------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------
def test_main_end_to_end(tmp_path, monkeypatch):
    """CARS2_main on synth_frappe, 2 epochs: the Init line, a falling loss, and
    evaluate_TopK through the device walk."""
    from hhfm_amd import CARS2 as C2
    from hhfm_amd import harness
    walks = []
    real = harness.Train._device_walk
    monkeypatch.setattr(harness.Train, "_device_walk",
                        lambda self, *a: walks.append(1) or real(self, *a))
    out = tmp_path / "result.txt"
    argv = ["--path", G + "/", "--epoch", "3", "--batch_size", "2000", "--lr", "0.05",
            "--result_file", str(out)]
    np.random.seed(2016)
    t = C2.CARS2_main("synth_frappe", 16, 5, argv)
    assert isinstance(t.model, C2.CARS2) and t.model.features_M == len(t.feature_inject)
    assert len(t.loss_epoch) == 2 and np.all(np.isfinite(t.loss_epoch))
    assert t.loss_epoch[1] < t.loss_epoch[0]
    log = open(out).read()
    assert "Dataset=synth_frappe CARS2 Init:" in log
    assert walks
    # the trained model scores what the restatement scores
    Wt = t.model.get_weights()
    rows = t.data.Train_data.values[:500, 1:]
    X = np.column_stack([rows[:, :2], t.context_ids(rows)])
    exact, mag, _ = cr.exact_rows(X, Wt)
    kappa_check("cars2_trained_rows", t.model.score_rows(X)[:, 0], None, exact, mag)
