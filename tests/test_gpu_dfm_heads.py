"""DeepFM's FM-only, deep-only and logloss heads on the GPU (include/hhfm.h
"DeepFM heads"): scoring, catalog top-K and the train step against the
restatement of tests/dfm_heads_ref.py and the reference's own numbers
(tests/golden/dfm_heads.npz).

Score bars: tests/helpers.kappa_check for fp32 (1e-5 relative on κ <= 100 rows,
1e-5 of S = Σ_j |concat_j·Wp_j| + |bp| on the rest), 5e-3·S for a bf16 MLP, and
under the sigmoid |p − p64| <= 0.25·1e-5·S + 4·2^-24 (the z bar through the
sigmoid's slope of at most 1/4, plus the rounding of p).
"""
import os

import numpy as np
import pytest
import torch

from oracle import parity
from tests import dfm_heads_ref as hr
from tests.helpers import bf16_round, kappa_check
from tests.test_gpu_train_grad import _check
from tests.test_gpu_training import _args, _check_slot, _check_var

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
HEADS = sorted(hr.HEADS)
FM, DEEP, SIG = hr.HEAD_FM, hr.HEAD_DEEP, hr.HEAD_SIGMOID
F32 = np.float32


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rows(rng, B, nu, ni, F):
    """[user, item, F − 2 context columns of 5 values each]; -> X int32, M."""
    cols = [rng.integers(0, nu, B), rng.integers(nu, nu + ni, B)][:F]
    o = nu + ni
    for _ in range(F - 2):
        cols.append(rng.integers(o, o + 5, B))
        o += 5
    return np.stack(cols, 1).astype(np.int32), o


def _weights(rng, M, F, k, layers, head, scale):
    E = rng.normal(0, scale, (M, k)).astype(F32)
    w = rng.uniform(0, 1, M).astype(F32)
    Ls, bs, fan = [], [], F * k
    for n in layers:
        g = np.sqrt(2.0 / (fan + n))
        Ls.append(rng.normal(0, g, (fan, n)).astype(F32))
        bs.append(rng.normal(0, g, n).astype(F32))
        fan = n
    D = hr.wp_size(head, F, k, layers) if layers else F + k
    Wp = rng.normal(0, np.sqrt(2.0 / (D + 1)), D).astype(F32)
    return E, w, Ls, bs, Wp, F32(0.01)


def _forward(X, E, w, Ls, bs, Wp, bp, head, mlp=torch.float32, table=torch.float32, proj=None,
             plan=0):
    from hhfm_amd import ops
    F, k = X.shape[1], E.shape[1]
    Wt, bd, dims = ops.dfm_prepare_weights([_dev(W) for W in Ls], [_dev(b) for b in bs], mlp, F, k)
    out = ops.dfm_forward(_dev(X), _dev(E).to(table), _dev(w), Wt, bd, dims, mlp, _dev(Wp),
                          float(bp), proj=proj, plan=plan, head=head)
    return out.cpu().numpy()


def _p_bar(got, X, E, w, Ls, bs, Wp, bp, head):
    p64, _, S = hr.forward(X, E, w, Ls, bs, Wp, bp, head | SIG, dt=np.float64)
    err = np.abs(got.astype(np.float64) - p64)
    bound = 0.25e-5 * S + 4 * 2.0 ** -24
    assert np.all(err <= bound), float(np.max(err / bound))


# ---------------------------------------------------------------------------
# 1. FM head rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["f32", "bf16"])
@pytest.mark.parametrize("k", [16, 20, 64, 128])   # idle lanes of a 16-lane group, generic, KJ 1, KJ 2
@pytest.mark.parametrize("F", [2, 5, 13])
def test_fm_head_rows(F, k, table):
    rng = np.random.default_rng(100 * F + k)
    tdt = torch.float32 if table == "f32" else torch.bfloat16
    for B in (1, 257, 4099):   # one row, one past the 256-row staging block, ragged
        X, M = _rows(rng, B, 30, 60, F)
        E, w, _, _, Wp, bp = _weights(rng, M, F, k, [], FM, 0.3)
        Eq = bf16_round(E) if table == "bf16" else E
        got = _forward(X, E, w, [], [], Wp, bp, FM, table=tdt)
        ref32, _, _ = hr.forward(X, Eq, w, [], [], Wp, bp, FM)
        ex, _, S = hr.forward(X, Eq, w, [], [], Wp, bp, FM, dt=np.float64)
        kappa_check("dfm_fm_head_rows", got, ref32, ex, S)
        _p_bar(_forward(X, E, w, [], [], Wp, bp, FM | SIG, table=tdt), X, Eq, w, [], [], Wp, bp, FM)


@pytest.mark.parametrize("table", ["f32", "bf16"])
def test_fm_head_is_the_full_models_fm_part(table):
    """The full model with zero deep projection entries, on the forward whose
    `base` comes from the same row kernels (fp32 MLP, projected layer 0, FM
    part from the rows): the same bits."""
    from hhfm_amd import ops
    rng = np.random.default_rng(7)
    F, k, layers = 5, 64, [32, 24]
    tdt = torch.float32 if table == "f32" else torch.bfloat16
    for B in (257, 1000):
        X, M = _rows(rng, B, 30, 60, F)
        E, w, Ls, bs, Wp, bp = _weights(rng, M, F, k, layers, FM, 0.3)
        fm = _forward(X, E, w, [], [], Wp, bp, FM, table=tdt)
        full = np.concatenate([Wp, np.zeros(layers[-1], F32)])
        both = _forward(X, E, w, Ls, bs, full, bp, None, table=tdt, proj=True,
                        plan=ops.PLAN_ROW_FM)
        assert np.array_equal(fm, both)
        # the model's real layer list beside the head changes nothing
        assert np.array_equal(fm, _forward(X, E, w, Ls, bs, Wp, bp, FM, table=tdt))


def test_fm_head_bad_id_reads_row_0_and_is_flagged():
    from hhfm_amd import ops
    rng = np.random.default_rng(9)
    F, k = 5, 16
    X, M = _rows(rng, 40, 30, 60, F)
    E, w, _, _, Wp, bp = _weights(rng, M, F, k, [], FM, 0.3)
    bad, zero = X.copy(), X.copy()
    bad[3, 1], bad[17, 4] = M + 5, -1
    zero[3, 1] = zero[17, 4] = 0
    assert np.array_equal(_forward(bad, E, w, [], [], Wp, bp, FM),
                          _forward(zero, E, w, [], [], Wp, bp, FM))
    with pytest.raises(ValueError):
        ops.validate_ids(_dev(bad), M)
    ops.validate_ids(_dev(zero), M)


# ---------------------------------------------------------------------------
# 2. deep head rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("mlp", ["f32", "bf16"])
@pytest.mark.parametrize("layers", [[32, 24], [150, 200, 150]])
@pytest.mark.parametrize("k", [16, 64])
def test_deep_head_rows(k, layers, mlp, proj):
    """The table is drawn at the reference's own init scale (N(0, 0.01),
    DFM.py:176), as in tests/test_gpu_dfm.py: kappa_check's κ measures the
    projection's cancellation only, not the hidden layers', and without the FM
    part nothing else carries z.  At scale 0.3 the float32 restatement itself
    misses the elementwise bar on these shapes (1.3e-5 / 3.4e-5 / 0.8e-5 /
    1.3e-5 relative on κ <= 100 rows, measured on the CPU); at 0.01 it sits at
    0.6e-6 – 2.5e-6, asserted below at half the bar."""
    rng = np.random.default_rng(k + len(layers))
    F, B = 5, 1000
    mdt = torch.float32 if mlp == "f32" else torch.bfloat16
    X, M = _rows(rng, B, 30, 60, F)
    E, w, Ls, bs, Wp, bp = _weights(rng, M, F, k, layers, DEEP, 0.01)
    got = _forward(X, E, w, Ls, bs, Wp, bp, DEEP, mlp=mdt, proj=proj)
    full = np.concatenate([np.zeros(F + k, F32), Wp])
    assert np.array_equal(got, _forward(X, E, w, Ls, bs, full, bp, None, mlp=mdt, proj=proj))
    ex, _, S = hr.forward(X, E, w, Ls, bs, Wp, bp, DEEP, dt=np.float64)
    if mlp == "f32":
        ref32 = hr.forward(X, E, w, Ls, bs, Wp, bp, DEEP)[0]
        well = S <= 100 * np.abs(ex)
        assert np.max((np.abs(ref32 - ex) / np.abs(ex))[well]) <= 0.5e-5
        kappa_check("dfm_deep_head_rows", got, ref32, ex, S)
        _p_bar(_forward(X, E, w, Ls, bs, Wp, bp, DEEP | SIG, mlp=mdt, proj=proj), X, E, w, Ls, bs,
               Wp, bp, DEEP)
    else:
        ref = parity.dfm_bf16_out(X, E, w, Ls, bs, full, bp)
        assert np.all(np.abs(got - ref) <= 5e-3 * S), float(np.max(np.abs(got - ref) / S))
        p = _forward(X, E, w, Ls, bs, Wp, bp, DEEP | SIG, mlp=mdt, proj=proj)
        # the sigmoid pass alone: the rounding of p on the forward's own z
        assert np.all(np.abs(p - 1 / (1 + np.exp(-got.astype(np.float64)))) <= 4 * 2.0 ** -24)


# ---------------------------------------------------------------------------
# 3. the reference's own numbers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "dfm_heads.npz")))


def _gold_model(d, name, l2=0.0, **kw):
    from hhfm_amd.DFM import DeepFM
    use_fm, use_deep, loss_type = hr.HEADS[name]
    layers = [int(n) for n in d["layer_dims"]]
    M, k = d["E"].shape
    m = DeepFM(int(d["n_user"]), int(d["n_item"]), M, 5, k, layers, None, 0.01, 0, l2,
               use_fm=use_fm, use_deep=use_deep, loss_type=loss_type, **kw)
    assert m.weights["concat_projection"].shape == d[f"{name}_concat_projection"].shape
    m.set_weights(feature_embeddings=d["E"], feature_bias=d["w"][:, None],
                  concat_projection=d[f"{name}_concat_projection"],
                  concat_bias=d[f"{name}_concat_bias"],
                  **{f"layer_{i}": d[f"layer_{i}"] for i in range(len(layers))},
                  **{f"bias_{i}": d[f"bias_{i}"] for i in range(len(layers))})
    return m


def _gold_weights(d, name):
    L = len(d["layer_dims"])
    return (d["E"], d["w"], [d[f"layer_{i}"] for i in range(L)],
            [d[f"bias_{i}"][0] for i in range(L)], d[f"{name}_concat_projection"][:, 0],
            F32(d[f"{name}_concat_bias"]))


@pytest.mark.parametrize("name", HEADS)
def test_golden_out_and_topk(gold, name):
    from hhfm_amd import ops
    d = gold
    head = hr.head_word(*hr.HEADS[name])
    m = _gold_model(d, name)
    W = _gold_weights(d, name)
    out = m.score_rows(d["X"])[:, 0]
    assert np.array_equal(m.sess.run(m.out, feed_dict={m.feat_index: d["X"]})[:, 0], out)
    if head & SIG:
        _p_bar(out, d["X"], *W, head & ~SIG)
        assert np.all(np.abs(out - d[f"{name}_out"]) <= 0.5e-5 * hr.forward(d["X"], *W, head)[2]
                      + 8 * 2.0 ** -24)
    else:
        ex, _, S = hr.forward(d["X"], *W, head, dt=np.float64)
        kappa_check("dfm_heads_golden", out, d[f"{name}_out"], ex, S)
    A = d[f"{name}_A"]
    want = d[f"{name}_topk_idx"]
    assert np.array_equal(m.topk(A, 20), want)
    # chunk_rows = one query's rows: 4 passes
    Wt, bs, dims, Wp, bp = m._prepared()
    _, ids = ops.dfm_catalog_topk(m._idx(A), m.table, m.weights["feature_bias"].reshape(-1), Wt,
                                  bs, dims, Wp, bp, 1, m.n_user, m.n_item, 20, 0,
                                  chunk_rows=m.n_item, head=head)
    assert np.array_equal(ids.cpu().numpy(), want)


def test_golden_item_shards_merge_to_model_topk(gold):
    from hhfm_amd import ops
    name = "deep_logloss"
    m = _gold_model(gold, name)
    A = gold[f"{name}_A"]
    q = m._idx(A)
    bounds = np.linspace(0, m.n_item, 9).astype(int)
    parts = [m.catalog_topk(q, int(b0), int(b1 - b0), 20) for b0, b1 in zip(bounds, bounds[1:])]
    _, ids = ops.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert np.array_equal(ids.cpu().numpy(), m.topk(A, 20))
    assert np.array_equal(ids.cpu().numpy(), gold[f"{name}_topk_idx"])


# ---------------------------------------------------------------------------
# the train step through the binding
# ---------------------------------------------------------------------------
class _Step:
    """hhfm_dfm_train_step_head(_det) on device copies of a set of weights:
    slots, workspace and scratch kept here."""

    def __init__(self, E, w, Ls, bs, Wp, bp, head, opt="adagrad", det=False, ws_dims=None):
        from hhfm_amd import training
        self.head, self.det, self.o = head, det, opt
        self.opt = {"adagrad": 0, "sgd": 1}[opt]
        self.L = len(Ls)
        self.dims = [int(W.shape[1]) for W in Ls]
        self.ws_dims = self.dims if ws_dims is None else ws_dims   # the size queries' layer list
        self.par = ([_dev(E), _dev(w)] + [_dev(W) for W in Ls] + [_dev(b) for b in bs]
                    + [_dev(Wp), _dev(np.asarray(bp, F32).reshape(1))])
        self.slots = [training._slots(self.opt, p) for p in self.par]
        self.loss = torch.zeros(1, device="cuda")
        self.ws, self.ws_rows, self.sc = None, -1, None

    def get(self):
        return [p.cpu().numpy().copy() for p in self.par]

    def get_slots(self):
        return [s.cpu().numpy().copy() for s in self.slots]

    def step(self, X, y, lr, lam):
        from hhfm_amd._native import native
        nat = native()
        B, F = X.shape
        M, k = self.par[0].shape
        L = self.L
        if self.ws_rows < B:
            self.ws = torch.zeros(nat.dfm_train_workspace(B, F, k, M, self.ws_dims),
                                  dtype=torch.uint8, device="cuda")
            self.sc = torch.empty(nat.dfm_train_det_scratch(B, F, k, M, self.ws_dims),
                                  dtype=torch.uint8, device="cuda")
            self.ws_rows = B
        Xd, yd = _dev(np.asarray(X, np.int32)), _dev(np.asarray(y, F32).reshape(-1))
        ptr = [p.data_ptr() for p in self.par]
        acc = [s.data_ptr() for s in self.slots] if self.o != "sgd" else []
        args = (Xd.data_ptr(), yd.data_ptr(), B, F, ptr[0], ptr[1], M, k, self.dims,
                ptr[2:2 + L], ptr[2 + L:2 + 2 * L], ptr[2 + 2 * L], ptr[3 + 2 * L], float(lr),
                float(lam), self.opt, acc, self.ws.data_ptr(), self.ws.numel())
        tail = (self.loss.data_ptr(), _stream(), self.head)
        if self.det:
            nat.dfm_train_step_head_det(*args, self.sc.data_ptr(), self.sc.numel(), *tail)
        else:
            nat.dfm_train_step_head(*args, *tail)
        return float(self.loss.item())


def _train_case(rng, B, k, layers, head, F=5, scale=0.1, labels=(1.0, 0.0)):
    X, M = _rows(rng, max(B, 1), 30, 60, F)
    X = X[:B]
    E, w, Ls, bs, Wp, bp = _weights(rng, M, F, k, layers, head, scale)
    y = rng.choice(labels, B).astype(F32)
    return X, y, (E, w, Ls, bs, Wp, bp)


def _flat(E, w, Ls, bs, Wp, bp):
    return [E, w] + list(Ls) + list(bs) + [Wp, np.asarray(bp, F32).reshape(1)]


# 5. loss
@pytest.mark.parametrize("labels", ["10", "1m"])
@pytest.mark.parametrize("name", HEADS)
def test_partial_fit_loss_is_the_references(gold, name, labels):
    d = gold
    m = _gold_model(d, name, l2=float(d["l2"]))
    loss = m.partial_fit({"X": d["X_loss"], "Y": d[f"Y_{labels}"][:, None]})
    want = float(d[f"{name}_loss_{labels}"])
    print(f"{name} {labels}: loss {loss!r} reference {want!r}")
    assert abs(loss - want) <= 1e-5 * abs(want)


# 6. gradient
@pytest.mark.parametrize("B", [1, 700])
@pytest.mark.parametrize("k", [4, 64])
@pytest.mark.parametrize("name", HEADS)
def test_gradient_matches_float64(name, k, B):
    """One SGD step (lr 1, λ 0): before − after is the raw gradient, held to
    test_gpu_train_grad._check's bound with dfm_heads_ref.grad64's magnitudes."""
    head = hr.head_word(*hr.HEADS[name])
    rng = np.random.default_rng(1000 * k + B + head)
    layers = [12, 10]
    X, y, W = _train_case(rng, B, k, layers, head, labels=(1.0, 0.0) if head & SIG else (1.0, -1.0))
    loss64, gr, mg, z = hr.grad64(X, y, *W, head)
    assert np.abs(z).max() <= 4.0
    s = _Step(*W, head, opt="sgd")
    before = s.get()
    loss = s.step(X, y, 1.0, 0.0)
    after = s.get()
    assert abs(loss - loss64) <= 1e-5 * abs(loss64) + 1e-12
    for kk, b, a in zip(hr.keys(len(layers)), before, after):
        if gr[kk] is None:
            assert np.array_equal(b, a), kk
        else:
            _check(f"{name} k{k} B{B} {kk}", b, a, np.asarray(gr[kk]).reshape(b.shape),
                   np.asarray(mg[kk]).reshape(b.shape))


# 7. variables that must not move
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", ["fm_mse", "fm_logloss", "deep_mse", "deep_logloss"])
def test_variables_without_a_gradient_stay_bit_for_bit(name, det):
    head = hr.head_word(*hr.HEADS[name])
    rng = np.random.default_rng(head)
    layers = [12, 10]
    X, y, W = _train_case(rng, 3 * 50, 8, layers, head)
    s = _Step(*W, head, det=det)
    before, slots = s.get(), s.get_slots()
    for i in range(3):
        s.step(X[50 * i:50 * i + 50], y[50 * i:50 * i + 50], 0.1, 0.05)
    after, slots1 = s.get(), s.get_slots()
    keys = hr.keys(len(layers))
    still = [kk for kk in keys if (kk[0] in "Wb" and kk not in ("Wp", "bp") and not head & DEEP)
             or (kk == "w" and not head & FM)]
    assert still
    for kk, b, a, sb, sa in zip(keys, before, after, slots, slots1):
        same = np.array_equal(b.view(np.int32), a.view(np.int32))
        assert same == (kk in still), kk
        assert np.array_equal(sb.view(np.int32), sa.view(np.int32)) == (kk in still), kk


# 8. / 9. replay from the GPU's own pre-step state
def _replay(s, X, y, lr, lam, nsteps, B):
    L = s.L
    keys = hr.keys(L)
    for i in range(nsteps):
        Xb, yb = X[B * i:B * i + B], y[B * i:B * i + B]
        cur, slots = s.get(), s.get_slots()
        E, w, Ls, bs, Wp, bp = (cur[0], cur[1], cur[2:2 + L], cur[2 + L:2 + 2 * L], cur[2 + 2 * L],
                                cur[3 + 2 * L][0])
        acc = dict(zip(keys, slots))
        loss = s.step(Xb, yb, lr, lam)
        rl, *new, acc1 = hr.train_step(Xb, yb, E, w, Ls, bs, Wp, bp, acc, lr, lam, s.head)
        _, *gnew, _ = hr.train_step(Xb, yb, E, w, Ls, bs, Wp, bp, {}, 1.0, lam, s.head,
                                    optimizer="sgd")
        assert np.isclose(loss, rl, rtol=1e-5), (loss, rl)
        for kk, g, v_new, v_old, v_g, sl in zip(keys, s.get(), _flat(*new), cur, _flat(*gnew),
                                                s.get_slots()):
            v_new = np.asarray(v_new, F32).reshape(v_old.shape)
            _check_var(g, v_new, v_old, "adagrad", v_old - np.asarray(v_g, F32).reshape(v_old.shape))
            _check_slot(sl, acc1[kk], "adagrad")


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", ["fm_mse", "deep_mse", "fm_logloss", "deep_logloss",
                                  "both_logloss"])
def test_three_adagrad_steps_replayed(name, det):
    head = hr.head_word(*hr.HEADS[name])
    rng = np.random.default_rng(40 + head)
    B = 301
    X, y, W = _train_case(rng, 3 * B, 16, [24, 40, 24], head, labels=(1.0, -1.0))
    _replay(_Step(*W, head, det=det), X, y, 0.05, 0.05, 3, B)


@pytest.mark.parametrize("name", HEADS)
def test_deterministic_step_is_bit_reproducible(name):
    head = hr.head_word(*hr.HEADS[name])
    rng = np.random.default_rng(60 + head)
    B = 700
    X, y, W = _train_case(rng, 2 * B, 16, [24, 40, 24], head)
    X[:B, 1] = X[0, 1]   # one item in every row of the first batch: a long segment
    runs = []
    for _ in range(2):
        s = _Step(*W, head, det=True)
        losses = [s.step(X[B * i:B * i + B], y[B * i:B * i + B], 0.05, 0.05) for i in range(2)]
        runs.append((losses, s.get(), s.get_slots()))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("name", ["fm_logloss", "deep_mse"])
def test_deterministic_model_partial_fit(gold, name):
    """deterministic=True through the model: two models, the same batches, the same bits."""
    d = gold
    out = []
    for _ in range(2):
        m = _gold_model(d, name, l2=0.05, deterministic=True)
        losses = [m.partial_fit({"X": d["X_loss"], "Y": d["Y_10"][:, None]}) for _ in range(2)]
        out.append((losses, m.get_weights()))
    assert out[0][0] == out[1][0]
    for kk in out[0][1]:
        assert np.array_equal(out[0][1][kk], out[1][1][kk]), kk


# 10. empty batch
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", HEADS)
def test_empty_batch_moves_nothing(name, det):
    head = hr.head_word(*hr.HEADS[name])
    rng = np.random.default_rng(3)
    X, y, W = _train_case(rng, 8, 8, [12, 10], head)
    s = _Step(*W, head, det=det)
    s.step(X, y, 0.1, 0.0)
    before, slots = s.get(), s.get_slots()
    loss = s.step(X[:0], y[:0], 0.1, 0.0)
    assert loss == 0.0
    for b, a in zip(before + slots, s.get() + s.get_slots()):
        assert np.array_equal(b.view(np.int32), a.view(np.int32))


# ---------------------------------------------------------------------------
# 4. argument errors
# ---------------------------------------------------------------------------
def test_head_argument_errors():
    from hhfm_amd import ops
    from hhfm_amd._native import native
    nat = native()
    rng = np.random.default_rng(11)
    F, k, layers = 5, 16, [12, 10]
    X, M = _rows(rng, 20, 30, 60, F)
    E, w, Ls, bs, Wp, bp = _weights(rng, M, F, k, layers, FM | DEEP, 0.1)
    Xd, Ed, wd, Wpd = _dev(X), _dev(E), _dev(w), _dev(Wp)
    Wt, bd, dims = ops.dfm_prepare_weights([_dev(W) for W in Ls], [_dev(b) for b in bs],
                                           torch.float32, F, k)
    out = torch.empty(20, device="cuda")
    ws = torch.zeros(nat.dfm_forward_workspace_ex(20, F, k, M, dims, 0, 0) + 4096,
                     dtype=torch.uint8, device="cuda")

    def fwd(head, with_layers=True):
        nat.dfm_forward_head(Xd.data_ptr(), 20, F, Ed.data_ptr(), M, k, 0, wd.data_ptr(),
                             dims if with_layers else [],
                             [t.data_ptr() for t in Wt] if with_layers else [],
                             [t.data_ptr() for t in bd] if with_layers else [], 0, Wpd.data_ptr(),
                             float(bp), out.data_ptr(), 0, 0, ws.data_ptr(), ws.numel(), _stream(),
                             head)

    top_s = torch.empty(2, 5, device="cuda")
    top_i = torch.empty(2, 5, dtype=torch.int32, device="cuda")
    cws = torch.zeros(nat.dfm_catalog_topk_workspace_ex(2, F, k, M, 60, dims, 0, 1 << 20, 0) + 4096,
                      dtype=torch.uint8, device="cuda")

    def cat(head, with_layers=True):
        nat.dfm_catalog_topk_head(Xd.data_ptr(), 2, F, 1, Ed.data_ptr(), M, k, 0, wd.data_ptr(),
                                  dims if with_layers else [],
                                  [t.data_ptr() for t in Wt] if with_layers else [],
                                  [t.data_ptr() for t in bd] if with_layers else [], 0,
                                  Wpd.data_ptr(), float(bp), 30, 60, 0, 5, 1 << 20,
                                  top_s.data_ptr(), top_i.data_ptr(), 0, 0, cws.data_ptr(),
                                  cws.numel(), _stream(), head)

    y = rng.choice([1.0, 0.0], 20).astype(F32)

    def step(head, with_layers=True, det=False):
        s = _Step(E, w, Ls if with_layers else [], bs if with_layers else [], Wp, bp, head, det=det,
                  ws_dims=layers)
        before = s.get()
        try:
            s.step(X, y, 0.1, 0.0)
        except ValueError:
            assert all(np.array_equal(a, b) for a, b in zip(before, s.get()))
            raise

    for call in (fwd, cat, step, lambda h, wl=True: step(h, wl, det=True)):
        for head in (0, 8, SIG, FM | 8):
            with pytest.raises(ValueError, match="invalid argument"):
                call(head)
        for head in (DEEP, FM | DEEP, DEEP | SIG):   # NULL layers with DEEP
            with pytest.raises(ValueError, match="invalid argument"):
                call(head, False)
        call(FM, False)                              # NULL layers without DEEP
        call(FM | SIG, False)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 11. the reference's own route
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("use_fm,use_deep,loss_type", [(True, False, "mse"), (True, True, "logloss"),
                                                       (False, True, "logloss")])
def test_reference_route_trains(tmp_path, use_fm, use_deep, loss_type):
    from hhfm_amd import NewLoadData as DATA
    from hhfm_amd.DFM import DeepFM, Train
    np.random.seed(2016)
    args = _args(tmp_path, lamda=0.01, lr=0.01, epoch=3, hidden_factor=16)
    data = DATA.LoadData(args.path, args.dataset)
    m = DeepFM(data.n_user, data.n_item, data.features_M, data.Train_data.shape[1] - 1,
               args.hidden_factor, [150, 200, 150], None, args.lr, args.verbose, args.lamda,
               use_fm=use_fm, use_deep=use_deep, loss_type=loss_type)
    t = Train(args, data=data, model=m)
    losses = t.train()
    assert len(losses) == 2 and np.all(np.isfinite(losses))
    X = data.Train_data.values[:50, 1:]
    out = m.score_rows(X)
    assert np.all(np.isfinite(out))
    if loss_type == "logloss":
        assert np.all((out >= 0) & (out <= 1))
    assert m.topk(X[:3], 10).shape == (3, 10)
    assert "DFM Epoch 1" in open(tmp_path / "result.txt").read()
