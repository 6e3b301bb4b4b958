"""AFM with attention=0 on the GPU (include/hhfm.h "AFM without attention"):
row scores (hhfm_fm_score_rows_scaled, scale = P), the catalog top-K
(hhfm_afm_noatt_catalog_topk), the training step (hhfm_afm_noatt_train_step)
and the model surface, against the float64 oracle of tests/afm0_ref.py and the
reference's own numbers (tests/golden/afm0.npz).

The catalog score is this library's definition (the reference's topk raises
KeyError there): ``out`` of the row with column 1 replaced by the item.  Its
query sets are gap-clean at 1e-5·Σ|terms| (tests/test_afm0_ref.py), so the id
lists are compared with array_equal.

Gradient parity, what each case catches (one SGD step, lr = 1, before − after
against grad64, |Δ − g64| <= 1e-5·mag + 2^-23·max(|before|, |after|)):
  F2_k4_B1            every element has one contribution: the `− e_f` term
                      dropped doubles dE; P missing from dE or x from dP shows
  F5_k64_B300_M30     300 rows over 30 ids (each table row ~50 contributions,
                      repeated ids inside rows 1 and 2): a lost or doubled
                      atomic, and dP's cross-workgroup sum (75 workgroups)
  F16_k256_B65        four columns per lane: the column ↔ Philox word / accP
                      slot mapping, and F = 16
  F5_k20_B4097        k no multiple of 64 (idle lanes in the workgroup sum),
                      B past the 2,048-workgroup cap (a wave takes three rows)
  *_keep              keep 0.5 with the mask read back from hhfm_dropout_mask
                      site 2: the mask missing from dP or dE, a wrong row or
                      column index of the mask, 1/keep applied once too often
Measured on an MI355X: largest err / bound 0.020 (E of F16_k256_B65; P 0.019,
w 0.0033, w0 0.0018 at most); the fp32 oracle alone sits at <= 0.024
(tests/test_afm0_ref.py).  On builds with one seeded bug each: the `− e_f` term
dropped, and P missing from dE, fail test_known_answer and all six cases; the
mask missing from dP fails both keep cases and no other.
"""
import os

import numpy as np
import pytest
import torch

from tests import afm0_ref as ar
from tests import dropout_ref as dref
from tests import train_ref as tr
from tests.helpers import bf16_round, kappa_check, log_parity

pytestmark = pytest.mark.gpu

SEED, case_mask = ar.SEED, ar.case_mask

G = os.path.join(os.path.dirname(__file__), "golden")
F32, F64 = np.float32, np.float64
ADAGRAD, SGD, MOMENTUM, ADAM = 0, 1, 2, 3
OPT_NAME = {ADAGRAD: "adagrad", SGD: "sgd", MOMENTUM: "momentum", ADAM: "adam"}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32).reshape(-1)).view(np.uint32)


def _model(Wt, n_user, n_item, F, opt="GradientDescentOptimizer", lr=1.0, keep=(1, 1), **kw):
    from hhfm_amd.AFM import AFM
    M, k = Wt["E"].shape
    m = AFM(n_user, n_item, M, 0, [k, k], None, lr, 100.0, list(keep), opt, 0.999, F, **kw)
    m.set_weights(feature_embeddings=Wt["E"], feature_bias=np.asarray(Wt["w"])[:, None],
                  bias=Wt["w0"], prediction=np.asarray(Wt["P"])[:, None])
    return m


def _weights_of(m):
    W = m.get_weights()
    return dict(E=W["feature_embeddings"], w=W["feature_bias"][:, 0], w0=F32(W["bias"]),
                P=W["prediction"][:, 0])


class _Step:
    """Device state of a run through the binding: the four parameters, their
    slots and the zero-filled workspace."""

    def __init__(self, Wt, opt, ws_bytes=None):
        from hhfm_amd._native import native
        self.nat = native()
        self.par = [_dev(np.asarray(Wt["E"], F32)), _dev(np.asarray(Wt["w"], F32)),
                    _dev(np.asarray([Wt["w0"]], F32)), _dev(np.asarray(Wt["P"], F32))]
        self.M, self.k = self.par[0].shape
        self.opt = opt
        self.acc = [None if opt == SGD else
                    torch.full_like(p, 0.1) if opt == ADAGRAD else
                    torch.zeros_like(p) if opt == MOMENTUM else
                    torch.zeros(2 * p.numel(), device="cuda") for p in self.par]
        n = self.nat.afm_noatt_train_workspace(self.M, self.k) if ws_bytes is None else ws_bytes
        self.ws = torch.zeros(n, dtype=torch.uint8, device="cuda")
        self.loss = torch.full((1,), 7.0, device="cuda")

    def args(self, X, y, lr, keep, seed, F=None, k=None, opt=None, acc=None, ws=None):
        B = len(X)
        Xd = _dev(np.asarray(X, np.int32)) if B else None
        yd = _dev(np.asarray(y, F32)) if B else None
        self._keep_alive = (Xd, yd)
        E, w, w0, P = self.par
        if acc is None:
            acc = [] if self.opt == SGD else [a.data_ptr() for a in self.acc]
        ws = (self.ws.data_ptr(), self.ws.numel()) if ws is None else ws
        return (Xd.data_ptr() if B else 0, yd.data_ptr() if B else 0, B,
                (X.shape[1] if F is None else F), E.data_ptr(), w.data_ptr(), w0.data_ptr(),
                P.data_ptr(), self.M, self.k if k is None else k, lr,
                self.opt if opt is None else opt, keep, seed, acc, *ws)

    def step(self, X, y, lr, keep=1.0, seed=0):
        self.nat.afm_noatt_train_step(*self.args(X, y, lr, keep, seed), self.loss.data_ptr(),
                                      _stream())
        return float(self.loss.item())

    def weights(self):
        E, w, w0, P = (p.cpu().numpy() for p in self.par)
        return dict(E=E, w=w, w0=F32(w0[0]), P=P)

    def slots(self):
        if self.opt == SGD:
            return {n: None for n in ar.NAMES}
        return {n: a.cpu().numpy() for n, a in zip(ar.NAMES, self.acc)}

    def state(self):
        torch.cuda.synchronize()
        out = [p.cpu().numpy() for p in self.par]
        out += [a.cpu().numpy() for a in self.acc if a is not None]
        return out + [self.ws.cpu().numpy().view(np.uint32)]


# ---------------------------------------------------------------------------
# 1. known answer
# ---------------------------------------------------------------------------
def test_known_answer():
    """F = 2, k = 4, one row [0, 1], every value dyadic: x = e_0 ⊙ e_1 =
    [2, −2, 2, −½], Σ x·P = 2 + 4 + 1 − 1.5 = 5.5, out = 5.5 − ¼ + ⅛ = 5.375,
    y = 1: g = 4.375, loss = g²/2 = 9.5703125, and one SGD step at lr 1 moves
    P by g·x, E[0] by g·P ⊙ e_1, E[1] by g·P ⊙ e_0, w and w0 by g."""
    Wt = dict(E=F32([[1, 2, 0.5, -1], [2, -1, 4, 0.5]]), w=F32([0.25, -0.5]), w0=F32(0.125),
              P=F32([1, -2, 0.5, 3]))
    X = np.array([[0, 1]], np.int32)
    m = _model(Wt, 1, 1, 2)
    assert sorted(m.weights) == ["bias", "feature_bias", "feature_embeddings", "prediction"]
    assert float(m.score_rows(X)[0, 0]) == 5.375
    loss = m.partial_fit({"X": X.astype(np.int64), "Y": np.array([[1.0]])})
    assert loss == 9.5703125
    W1 = _weights_of(m)
    g = 4.375
    assert np.array_equal(W1["P"], Wt["P"] - F32(g) * F32([2, -2, 2, -0.5]))
    assert np.array_equal(W1["E"][0], Wt["E"][0] - F32(g) * Wt["P"] * Wt["E"][1])
    assert np.array_equal(W1["E"][1], Wt["E"][1] - F32(g) * Wt["P"] * Wt["E"][0])
    assert np.array_equal(W1["w"], Wt["w"] - F32(g))
    assert W1["w0"] == F32(0.125 - g)


# ---------------------------------------------------------------------------
# 2. row scores
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("k", [4, 20, 64, 256])
@pytest.mark.parametrize("F", [2, 5, 16])
def test_row_parity(F, k, dtype):
    """``out`` against float64 with the rule of test_gpu_kernels._elementwise_vs_exact
    (helpers.kappa_check): rows with κ <= 100 within 1e-5 elementwise, the rest
    within 1e-5·Σ|terms|; bf16: the oracle runs on the rounded table."""
    from hhfm_amd import ops
    rng = np.random.default_rng(4000 + 31 * F + k)
    B, M = 1000, 777
    Wt = ar.weights(11 + k, M, k)
    Wt["E"] = (Wt["E"] * F32(min(1.0, (k * F * F / 2.0) ** -0.25 / 0.3))).astype(F32)
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    Eg = _dev(Wt["E"]) if dtype == "f32" else _dev(Wt["E"]).to(torch.bfloat16)
    E = Wt["E"] if dtype == "f32" else bf16_round(Wt["E"])
    got = ops.fm_score_rows(_dev(X), Eg, _dev(Wt["w"]), float(Wt["w0"]),
                            scale=_dev(Wt["P"])).cpu().numpy()
    ex, S = ar.out64(X, E, Wt["w"], Wt["w0"], Wt["P"])
    kappa_check("afm0_rows", got, None, ex, S)


def test_rows_through_the_class_match_the_reference():
    """The golden rows through score_rows and through sess.run(model.out), for
    fp32 tables; a bad id raises what FM.score_rows raises."""
    from hhfm_amd.FM import FM
    z = np.load(os.path.join(G, "afm0.npz"))
    nu, ni = int(z["n_user"]), int(z["n_item"])
    for k in (16, 64):
        p = f"k{k}_"
        Wt = dict(E=z[p + "E"], w=z[p + "w"], w0=z[p + "w0"], P=z[p + "P"])
        X = z[p + "X"].astype(np.int32)
        m = _model(Wt, nu, ni, X.shape[1])
        _, S = ar.out64(X, Wt["E"], Wt["w"], Wt["w0"], Wt["P"])
        a = m.score_rows(X)[:, 0]
        b = m.sess.run(m.out, feed_dict={m.train_features: X, m.dropout_keep: [1.0, 1.0],
                                         m.train_phase: False})[:, 0]
        assert np.array_equal(a, b)
        assert np.all(np.abs(a - z[p + "out"]) <= 1e-5 * S)
    M = Wt["E"].shape[0]
    bad = X.copy()
    bad[3, 2] = M
    fm = FM(X.shape[1], M, nu, ni, 64, 0.1, 0.0, 1, "AdagradOptimizer", 0, 0)
    for model in (fm, m):
        with pytest.raises(ValueError, match="indices must be in"):
            model.score_rows(bad)


# ---------------------------------------------------------------------------
# 3. catalog
# ---------------------------------------------------------------------------
_TABLES = {}


def _catalog(n_item, k, bf16=False, dup=False):
    """The case of tests/afm0_ref.catalog_case and its device tensors, uploaded once."""
    key = (n_item, k, bf16, dup)
    if key not in _TABLES:
        c = ar.catalog_case(n_item, k, bf16, dup)
        Wt = c["Wt"]
        E = _dev(Wt["E"])
        _TABLES[key] = (c, E.to(torch.bfloat16) if bf16 else E, _dev(Wt["w"]), _dev(Wt["P"]),
                        _dev(c["q"]))
    return _TABLES[key]


def _topk(n_item, k, B, bf16=False, dup=False, plan=0, q=None, begin=0, count=None, K=None):
    from hhfm_amd import ops
    c, E, w, P, qd = _catalog(n_item, k, bf16, dup)
    q = qd[:B].contiguous() if q is None else q
    count = n_item if count is None else count
    s, i = ops.afm_noatt_catalog_topk(q, E, w, float(c["Wt"]["w0"]), P, c["n_user"] + begin, count,
                                      c["K"] if K is None else K, begin, plan=plan)
    return c, s, i


def _check_catalog(c, s, i, B, E_dev, w_dev, P_dev):
    from hhfm_amd import ops
    K = c["K"]
    gs, gi = s.cpu().numpy(), i.cpu().numpy()
    assert np.array_equal(gi, c["ids"][:B])
    err = np.abs(gs.astype(F64) - c["score"][:B]) / c["mag"][:B]
    log_parity("afm0_catalog", rows=int(err.size), rows_kappa_gt_100=0,
               max_rel_err_kappa_le_100=float(err.max()), max_rel_err_kappa_gt_100=0.0,
               oracle_max_rel_err_kappa_gt_100=0.0)
    assert err.max() <= 1e-5, err.max()
    # the same rows through the row kernel: column 1 replaced by the item
    rows = np.repeat(c["q"][:B], K, axis=0)
    rows[:, 1] = c["n_user"] + gi.reshape(-1)
    r = ops.fm_score_rows(_dev(rows), E_dev, w_dev, float(c["Wt"]["w0"]), scale=P_dev)
    assert np.all(np.abs(r.cpu().numpy() - gs.reshape(-1)) <= 1e-5 * c["mag"][:B].reshape(-1))


@pytest.mark.parametrize("k", ar.CAT_K)
@pytest.mark.parametrize("B", ar.CAT_B)
@pytest.mark.parametrize("n_item", ar.CAT_ITEMS)
def test_catalog_matches_float64(n_item, B, k):
    """Ids equal to the float64 ranking; top_score within 1e-5·Σ|terms| of the
    float64 ``out`` and of score_rows of those rows (K = 20: all of a 20-item
    catalog; 64 / 65 items: one and two 64-item tiles … 70,000: streaming)."""
    c, s, i = _topk(n_item, k, B)
    _, E, w, P, _ = _catalog(n_item, k)
    _check_catalog(c, s, i, B, E, w, P)


@pytest.mark.parametrize("n_item,B,k", [(4100, 8, 64), (1025, 300, 16), (70000, 8, 64),
                                        (70000, 300, 16), (70000, 1, 128)])
def test_catalog_plans_agree(n_item, B, k):
    from hhfm_amd import ops
    _, _, base = _topk(n_item, k, B)
    for plan in (ops.PLAN_STORE, ops.PLAN_FUSED, ops.PLAN_NO_SEED, ops.PLAN_NO_RING,
                 ops.PLAN_EXACT_FP32):
        _, _, i = _topk(n_item, k, B, plan=plan)
        assert torch.equal(i, base), plan


@pytest.mark.parametrize("n_item,k", [(4100, 64), (70000, 16)])
def test_catalog_duplicated_items_come_out_index_ascending(n_item, k):
    """Three item rows with one table row and one w (the designed tie): equal
    score bits, and the lists hold them in ascending index, as tf.nn.top_k."""
    B = 8
    c, s, i = _topk(n_item, k, B, dup=True)
    gi, gs = i.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(gi, c["ids"][:B])
    assert np.array_equal(gi[:, :3], np.tile(ar.CAT_DUP, (B, 1)))
    assert np.array_equal(_bits(gs[:, 0]), _bits(gs[:, 1]))
    assert np.array_equal(_bits(gs[:, 0]), _bits(gs[:, 2]))


@pytest.mark.parametrize("n_item,k", [(4100, 64), (70000, 16)])
def test_catalog_shards_merge_to_the_whole(n_item, k):
    from hhfm_amd import ops
    B = 8
    c, s, i = _topk(n_item, k, B)
    cuts = [0, n_item // 3, n_item // 3 + n_item // 2, n_item]
    parts = [_topk(n_item, k, B, begin=a, count=b - a)[1:] for a, b in zip(cuts, cuts[1:])]
    ms, mi = ops.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(mi, i)
    assert torch.allclose(ms, s, rtol=1e-5, atol=0.0)


def test_catalog_ignores_column_1():
    c, s, i = _topk(4100, 64, 8)
    q = _catalog(4100, 64)[4][:8].clone()
    q[:, 1] = c["n_user"] + 7
    _, s2, i2 = _topk(4100, 64, 8, q=q.contiguous())
    assert torch.equal(i, i2) and torch.equal(s, s2)


@pytest.mark.parametrize("B", [8, 300])
def test_catalog_bf16_table(B):
    c, s, i = _topk(4100, 64, B, bf16=True)
    _, E, w, P, _ = _catalog(4100, 64, bf16=True)
    _check_catalog(c, s, i, B, E, w, P)


# ---------------------------------------------------------------------------
# 4. gradient parity
# ---------------------------------------------------------------------------
def _check(what, before, after, grad, mag):
    before, after = np.asarray(before, F32), np.asarray(after, F32)
    delta = before.astype(F64) - after.astype(F64)
    r = tr.ratio(delta, before, after, grad, mag)
    g = np.abs(np.asarray(grad, F64)).reshape(-1)
    err = np.abs(delta.reshape(-1) - np.asarray(grad, F64).reshape(-1))
    kappa = np.asarray(mag, F64).reshape(-1) / np.maximum(g, 1e-300)
    well = (g > 0) & (kappa <= 100)
    rel = err / np.maximum(g, 1e-300)
    log_parity("train_grad", rows=int(g.size), rows_kappa_gt_100=int(((g > 0) & ~well).sum()),
               max_rel_err_kappa_le_100=float(rel[well].max()) if well.any() else 0.0,
               max_rel_err_kappa_gt_100=0.0, oracle_max_rel_err_kappa_gt_100=0.0,
               max_err_over_bound=r)
    print(f"train_grad {what}: err / bound = {r:.3g}")
    assert r <= 1.0, (what, r)


@pytest.mark.parametrize("name", sorted(ar.GRAD_CASES))
def test_gradient_matches_float64(name):
    X, y, Wt = ar.grad_case(name)
    mask, keep = case_mask(name)
    s = _Step(Wt, SGD)
    if mask is not None:   # the mask the kernels draw, read back
        B, k = len(X), Wt["E"].shape[1]
        got = torch.empty(B, k, device="cuda")
        s.nat.dropout_mask(SEED, dref.SITE_AFM_VEC, B, k, keep, got.data_ptr(), _stream())
        mask = got.cpu().numpy()
        assert np.array_equal(mask, case_mask(name)[0])
        assert 0.3 < mask.mean() < 0.7
    ref_loss, Gd, Mg = ar.grad64(X, y, Wt["E"], Wt["w"], Wt["w0"], Wt["P"], mask, keep)
    loss = s.step(X, y, 1.0, keep, SEED)
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    W1 = s.weights()
    for n in ar.NAMES:
        _check(f"afm0 {name} {n}", Wt[n], W1[n], Gd[n], Mg[n])


# ---------------------------------------------------------------------------
# 5. optimizers
# ---------------------------------------------------------------------------
def _close_update(got, ref, before):
    step = np.abs(ref - before).max()
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-4 * step + 1e-9)


def _check_var(got, ref, before, o, grad):
    """tests/test_gpu_training._check_var's rule (restated: that module is a
    test file of its own)."""
    got, ref, before = (np.asarray(x, F32) for x in (got, ref, before))
    if o != "adam":
        _close_update(got, ref, before)
        return
    g = np.abs(np.asarray(grad, F32).reshape(ref.shape))
    scale = g.max(axis=-1, keepdims=True) if g.ndim == 2 else g.max(initial=0.0)
    well = g >= (1e-2 if g.ndim == 2 else 1e-4) * scale
    step = np.abs(ref - before).max()
    off = well & ~np.isclose(got, ref, rtol=1e-5, atol=1e-4 * step + 1e-9)
    assert not off.any(), (int(off.sum()), step)
    assert np.all(np.abs(got - ref) <= 2.01 * step + 1e-9)
    assert (well & (g > 0)).sum() >= 0.9 * (g > 0).sum()


@pytest.mark.parametrize("keep", [1.0, 0.5])
@pytest.mark.parametrize("opt", [ADAGRAD, SGD, MOMENTUM, ADAM])
def test_optimizer_steps_match_the_replay(opt, keep):
    """Three steps (B = 200, 0, 37: one workspace across batch sizes, an empty
    batch in the middle) replayed by the oracle from the GPU's own pre-step
    state.  Momentum leaves the rows no batch touched bit-identical; Adam
    decays m and v of every row, also at B = 0, where the loss is 0."""
    o = OPT_NAME[opt]
    rng = np.random.default_rng(60 + opt)
    M, F, k = 120, 5, 20
    Wt = ar.weights(5, M, k)
    Wt["E"] = (Wt["E"] * F32(0.5)).astype(F32)
    s = _Step(Wt, opt)
    W0 = s.weights()
    touched = np.zeros(M, bool)
    for t, B in enumerate((200, 0, 37), 1):
        X = rng.integers(0, M // 2, (B, F)).astype(np.int32)      # rows M/2.. are never touched
        y = rng.choice([-1.0, 1.0], B).astype(F32)
        touched[X.reshape(-1)] = True
        seed = 2016 | t << 32
        mask = dref.binary(seed, dref.SITE_AFM_VEC, B, k, keep) if keep < 1 and B else None
        cur, sl = s.weights(), s.slots()
        rl, W1, S1, Gr = ar.step(X, y, cur, sl, 0.05, o, t, mask, keep)
        loss = s.step(X, y, 0.05, keep, seed)
        assert np.isclose(loss, rl, rtol=1e-5, atol=0.0), (loss, rl)
        if B == 0:
            assert loss == 0.0
        got, gsl = s.weights(), s.slots()
        for n in ar.NAMES:
            _check_var(np.atleast_1d(got[n]), np.atleast_1d(W1[n]), np.atleast_1d(cur[n]), o,
                       np.atleast_1d(Gr[n]))
            if o != "sgd":
                ref = np.asarray(S1[n], F32).reshape(-1)
                assert np.allclose(gsl[n].reshape(-1), ref, rtol=1e-5,
                                   atol=1e-5 * np.abs(ref).max() + 1e-12), n
        if o == "adam" and B == 0:      # no gradient: m and v decay, every row
            m0, m1 = sl["E"][:M * k], gsl["E"][:M * k]
            assert np.allclose(m1, m0 * F32(0.9), rtol=1e-6) and np.abs(m0).max() > 0
            v0, v1 = sl["w"][M:], gsl["w"][M:]
            assert np.allclose(v1, v0 * F32(0.999), rtol=1e-6) and np.abs(v0).max() > 0
    W3 = s.weights()
    if o in ("momentum", "sgd", "adagrad"):
        assert np.array_equal(_bits(W3["E"][~touched]), _bits(W0["E"][~touched]))
        assert np.array_equal(_bits(W3["w"][~touched]), _bits(W0["w"][~touched]))
    assert not np.array_equal(_bits(W3["E"][touched]), _bits(W0["E"][touched]))
    ws = s.ws.cpu().numpy().view(np.uint32)
    if o != "adam":                     # left zeroed (Adam keeps its β powers there)
        assert not ws.any()


# ---------------------------------------------------------------------------
# 7. argument checks: the binding's error, every parameter bit for bit as it was
# ---------------------------------------------------------------------------
def _refused(s, call):
    before = s.state()
    with pytest.raises(ValueError):
        call()
    after = s.state()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32))
               for a, b in zip(before, after))
    assert float(s.loss.item()) == 7.0


def test_argument_checks_leave_everything_untouched():
    rng = np.random.default_rng(3)
    M, F, k, B = 40, 5, 16, 33
    Wt = ar.weights(9, M, k)
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    y = rng.choice([-1.0, 1.0], B).astype(F32)
    s = _Step(Wt, ADAGRAD)
    nat, L, st = s.nat, s.loss.data_ptr(), _stream()
    run = lambda a: nat.afm_noatt_train_step(*a, L, st)  # noqa: E731
    good = s.args(X, y, 0.1, 1.0, 0)
    for pos in (0, 1, 4, 5, 6, 7):                     # idx, y, E, w, w0, P NULL
        a = list(good)
        a[pos] = 0
        _refused(s, lambda a=a: run(a))
    _refused(s, lambda: nat.afm_noatt_train_step(*good, 0, st))              # loss NULL
    _refused(s, lambda: run(s.args(X, y, 0.1, 1.0, 0, ws=(0, s.ws.numel()))))  # workspace NULL
    for keep in (0.0, -0.5, 1.5, float("nan")):
        _refused(s, lambda keep=keep: run(s.args(X, y, 0.1, keep, 0)))
    _refused(s, lambda: run(s.args(X, y, 0.1, 1.0, 0, F=0)))
    _refused(s, lambda: run(s.args(X, y, 0.1, 1.0, 0, k=0)))
    _refused(s, lambda: run(s.args(X, y, 0.1, 1.0, 0, k=260)))
    _refused(s, lambda: run(s.args(X, y, 0.1, 1.0, 0, opt=4)))
    _refused(s, lambda: run(s.args(X, y, 0.1, 1.0, 0, ws=(s.ws.data_ptr(), s.ws.numel() - 1))))
    _refused(s, lambda: run(s.args(X, y, 0.1, 1.0, 0, acc=[])))                # missing slots
    a3 = [a.data_ptr() for a in s.acc]
    a3[3] = 0
    _refused(s, lambda: run(s.args(X, y, 0.1, 1.0, 0, acc=a3)))
    with pytest.raises(ValueError):
        nat.afm_noatt_train_workspace(M, 260)
    with pytest.raises(ValueError):
        nat.afm_noatt_train_workspace(0, k)
    s.step(X, y, 0.1)                                                          # and it still runs
    assert not np.array_equal(_bits(s.weights()["P"]), _bits(Wt["P"]))


def test_catalog_argument_checks():
    from hhfm_amd import ops
    c, E, w, P, q = _catalog(64, 16)
    with pytest.raises(ValueError):
        ops.afm_noatt_catalog_topk(q[:4, :1].contiguous(), E, w, 0.0, P, c["n_user"], 64, 5)
    with pytest.raises(ValueError):
        ops.afm_noatt_catalog_topk(q[:4].contiguous(), E, w, 0.0, P, c["n_user"], 64, 65)
    with pytest.raises(ValueError):
        ops.afm_noatt_catalog_topk(q[:4].contiguous(), E, w, 0.0, P[:8].contiguous(),
                                   c["n_user"], 64, 5)
    st = ops.status_word(E.device)
    bad = q[:4].clone()
    bad[2, 3] = E.shape[0]
    ops.afm_noatt_catalog_topk(bad.contiguous(), E, w, 0.0, P, c["n_user"], 64, 5, status=st)
    with pytest.raises(ValueError, match="indices must be in"):
        ops.check_status(E.device, E.shape[0])
    bad = q[:4].clone()
    bad[2, 1] = -5                                     # column 1 is not read
    ops.afm_noatt_catalog_topk(bad.contiguous(), E, w, 0.0, P, c["n_user"], 64, 5, status=st)
    ops.check_status(E.device, E.shape[0])


# ---------------------------------------------------------------------------
# 8. model level
# ---------------------------------------------------------------------------
def _main(tmp_path, *extra):
    from hhfm_amd.AFM import AFM_main
    np.random.seed(2016)
    return AFM_main("synth_frappe", 16, 5,
                    ["--path", G + "/", "--attention", "0", "--epoch", "3", "--batch_size", "4096",
                     "--verbose", "1", "--result_file", str(tmp_path / "result.txt"), *extra])


def test_main_trains_and_evaluates(tmp_path):
    """AFM_main --attention 0 end to end (the reference cannot: its
    evaluate_TopK hits KeyError('attention_W')): the second epoch's loss is
    below the first, evaluate_TopK returns, sharded_model_topk equals topk."""
    from hhfm_amd.distributed import sharded_model_topk
    t = _main(tmp_path)
    assert not t.model.attention and sorted(t.model.weights) == [
        "bias", "feature_bias", "feature_embeddings", "prediction"]
    assert len(t.loss_epoch) == 2 and t.loss_epoch[1] < t.loss_epoch[0]
    res = t.evaluate_TopK(t.data.Test_data)
    assert len(res) == 3 and all(0.0 <= float(x) <= 1.0 for x in res)
    log = (tmp_path / "result.txt").read_text()
    assert "Init" in log and "AFM Epoch 2" in log
    A = np.array(t.data.Test_data.values[:64, 1:], dtype=np.int64)
    assert np.array_equal(sharded_model_topk(t.model, A, 10), t.model.topk(A, 10))


def test_main_deterministic_runs_repeat(tmp_path):
    runs = []
    for _ in range(2):
        t = _main(tmp_path, "--deterministic", "1", "--keep", "[1,0.7]")
        assert t.model.deterministic
        W = t.model.get_weights()
        runs.append((list(t.loss_epoch), [_bits(W[n]) for n in sorted(W)]))
    assert runs[0][0] == runs[1][0]
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_bf16_model_scores_and_refuses_partial_fit():
    z = np.load(os.path.join(G, "afm0.npz"))
    nu, ni = int(z["n_user"]), int(z["n_item"])
    Wt = dict(E=z["k64_E"], w=z["k64_w"], w0=z["k64_w0"], P=z["k64_P"])
    X = z["k64_X"].astype(np.int32)
    m = _model(Wt, nu, ni, X.shape[1], table_dtype=torch.bfloat16)
    ex, S = ar.out64(X, bf16_round(Wt["E"]), Wt["w"], Wt["w0"], Wt["P"])
    assert np.all(np.abs(m.score_rows(X)[:, 0] - ex) <= 1e-5 * S)
    assert m.topk(X[:8], 10).shape == (8, 10)
    with pytest.raises(NotImplementedError, match="fp32"):
        m.partial_fit({"X": X.astype(np.int64), "Y": z["k64_Y"][:, None]})
