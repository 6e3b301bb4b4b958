"""Training dropout (`--keep` < 1) of FM and AFM on the GPU.

The mask is this project's, specified bit for bit (include/hhfm.h "Training
dropout"; numpy restatement in tests/dropout_ref.py); the arithmetic and the
gradient are tf.nn.dropout's.  So: `dropout_mask` against the numpy mask bit
for bit, then one GradientDescentOptimizer step at lr = 1, λ = 0 — which
leaves ``before − after`` equal to the raw gradient — against the masked
float64 references of tests/dropout_ref.py:

* FM: every E / w / w0 element inside the bound of tests/test_gpu_train_grad.py,
  |Δ − grad64| <= 1e-5 · mag + 2^-23 · max(|before|, |after|), the loss to 1e-5
  relative;
* AFM: every variable at the bar tests/test_gpu_training.py holds AFM steps
  to — rtol 1e-5 and atol 1e-4 of that variable's largest update — the loss
  to 1e-5 relative;

and structural checks that a wrong or misaligned mask cannot pass (dropped
columns bit for bit unchanged; a row whose pairs are all dropped), the step
count in the seed, the argument checks, and the reference's epoch loops with
keep < 1 (scoring stays at keep = 1).

AFM rows are drawn so that every pre-activation lies further from relu's kink
than fp32 can move it (dropout_ref.afm_margin_needed, asserted on the CPU in
tests/test_dropout_ref.py), so float64 takes relu' as the device does.

Measured on an MI355X.  FM, largest err / bound: 0.33 (one table element of
k260 at keep 0.7 — a row [44, 33, 44] with g = 6.9 where the other fields'
values at that column are some 600 × smaller than the element's own, so the
fp32 rounding of s in s − e_f shows; 0.26 at keep 0.9, 0.071 at 0.5), every
other case <= 0.059 (w0 of B32773; E <= 0.02, w <= 0.012).  AFM, largest
error beyond the rtol term over atol: attention_p 2.1e-3, attention_W 1.3e-3,
prediction 1.2e-3, E 6.4e-4, w 2.7e-4, attention_b 6.2e-5, w0 0 (all at
B = 1030).  FM's loss at B32773: 4e-8 relative at the most, the same in 36
steps (the dropout step sums it in double; summed by float atomics it lay
between 6e-7 and 1.1e-5 from step to step and missed the 1e-5 check in
about a third of them).
"""
import argparse
import os

import numpy as np
import pytest
import torch

from oracle import fm_oracle as orc
from tests import dropout_ref as dr
from tests import train_ref as tr
from tests.helpers import log_parity

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
SGD = 1
AFM_NAMES = ["feature_embeddings", "feature_bias", "bias", "attention_W", "attention_b",
             "attention_p", "prediction"]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gpu_mask(seed, site, rows, n, keep):
    from hhfm_amd._native import native
    out = torch.full((rows, n), -1.0, device="cuda")
    native().dropout_mask(seed, site, rows, n, keep, out.data_ptr(), _stream())
    return out.cpu().numpy()


# ---------------------------------------------------------------------------
# the mask
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [3, 257])
@pytest.mark.parametrize("site", [0, 1, 2])
def test_dropout_mask_matches_numpy_bit_for_bit(site, rows):
    for seed in (2016, 0x9e3779b97f4a7c15):
        for keep in (0.3, 0.9):
            for n in (1, 4, 5, 64, 65, 120, 256, 260):
                got = _gpu_mask(seed, site, rows, n, keep)
                ref = dr.binary(seed, site, rows, n, keep)
                assert np.array_equal(_bits(got), _bits(ref)), (seed, keep, n)


# ---------------------------------------------------------------------------
# FM
# ---------------------------------------------------------------------------
def _fm_step(X, y, E, w, w0, keep, seed, via_model):
    """-> loss, E, w, w0 after one SGD step (lr 1, λ 0) at ``keep``:
    FM.partial_fit (seed = the model's random_seed, first step), or the
    binding with an explicit seed."""
    B, F = X.shape
    M, k = E.shape
    if via_model:
        from hhfm_amd.FM import FM
        m = FM(F, M, 1, M - 1, k, 1.0, 0.0, keep, "GradientDescentOptimizer", 0, 0,
               random_seed=seed)
        m.set_weights(feature_embeddings=E, feature_bias=w[:, None], bias=w0)
        loss = m.partial_fit({"X": X.astype(np.int64), "Y": y[:, None]})
        W = m.get_weights()
        return loss, W["feature_embeddings"], W["feature_bias"][:, 0], np.float32(W["bias"])
    from hhfm_amd._native import native
    Xd, yd, Ed, wd, w0d = _dev(X), _dev(y), _dev(E), _dev(w), _dev(np.float32([w0]))
    ws = torch.zeros(native().train_workspace(M, k), dtype=torch.uint8, device="cuda")
    loss = torch.zeros(1, device="cuda")
    native().fm_train_step_ex(Xd.data_ptr(), yd.data_ptr(), B, F, Ed.data_ptr(), wd.data_ptr(),
                              w0d.data_ptr(), M, k, 1.0, 0.0, SGD, keep, seed, 0, 0, 0,
                              ws.data_ptr(), ws.numel(), loss.data_ptr(), _stream())
    return float(loss.item()), Ed.cpu().numpy(), wd.cpu().numpy(), np.float32(w0d.item())


def _check(what, before, after, grad, mag):
    """The per-element bound of tests/test_gpu_train_grad.py; logs err / bound."""
    before, after = np.asarray(before, np.float32), np.asarray(after, np.float32)
    delta = before.astype(np.float64) - after.astype(np.float64)
    r = tr.ratio(delta, before, after, grad, mag)
    g = np.abs(np.asarray(grad, np.float64)).reshape(-1)
    err = np.abs(delta.reshape(-1) - np.asarray(grad, np.float64).reshape(-1))
    kappa = np.asarray(mag, np.float64).reshape(-1) / np.maximum(g, 1e-300)
    well = (g > 0) & (kappa <= 100)
    rel = err / np.maximum(g, 1e-300)
    log_parity("train_grad_dropout", rows=int(g.size),
               rows_kappa_gt_100=int(((g > 0) & ~well).sum()),
               max_rel_err_kappa_le_100=float(rel[well].max()) if well.any() else 0.0,
               max_rel_err_kappa_gt_100=0.0, oracle_max_rel_err_kappa_gt_100=0.0,
               max_err_over_bound=r)
    print(f"train_grad_dropout {what}: err / bound = {r:.3g}")
    assert r <= 1.0, (what, r)


@pytest.mark.parametrize("keep", dr.FM_KEEPS)
@pytest.mark.parametrize("name", sorted(dr.FM_CASES))
def test_fm_dropout_gradient_matches_float64(name, keep):
    """The cases of test_gpu_train_grad.py and k = 260 (a lane's fifth element
    opens a second Philox block), each at keep 0.5, 0.7, 0.9.  Through
    FM.partial_fit with random_seed 2016 (its first step: seed 2016), and
    through the binding at F = 65, which the class's id layout cannot take."""
    X, y, E, w, w0 = dr.fm_case(name)
    via_model = name != "F65"
    seed = 2016 if via_model else dr.FM_SEED
    bn = dr.binary(seed, dr.SITE_FM, len(X), E.shape[1], keep)
    ref_loss, (dE, dw, dw0), (mE, mw, mw0) = dr.fm_grad64_dropout(X, y, E, w, w0, bn, keep)
    loss, E1, w1, w01 = _fm_step(X, y, E, w, w0, keep, seed, via_model)
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    _check(f"fm {name} keep {keep} E", E, E1, dE, mE)
    _check(f"fm {name} keep {keep} w", w, w1, dw, mw)
    _check(f"fm {name} keep {keep} w0", w0, w01, dw0, mw0)


@pytest.mark.parametrize("k", [20, 200, 260])
def test_fm_dropped_columns_are_untouched(k):
    """B = 1, distinct ids: a dropped column of the row's table rows keeps its
    bits, a kept column of every one of them moves."""
    rng = np.random.default_rng(k)
    M, F, keep, seed = 30, 5, 0.5, 77 | 3 << 32
    X = rng.permutation(M)[:F].astype(np.int32)[None, :]
    E = rng.normal(0, 0.2, (M, k)).astype(np.float32)
    w = rng.normal(0, 0.3, M).astype(np.float32)
    y = np.float32([1.0])
    bn = dr.binary(seed, dr.SITE_FM, 1, k, keep)[0]
    assert 0 < bn.sum() < k
    _, E1, _, _ = _fm_step(X, y, E, w, np.float32(0.02), keep, seed, False)
    same = _bits(E1) == _bits(E)
    assert same[np.setdiff1d(np.arange(M), X[0])].all()
    assert same[X[0]][:, bn == 0].all()
    assert not same[X[0]][:, bn == 1].any()


# ---------------------------------------------------------------------------
# AFM
# ---------------------------------------------------------------------------
def _afm_step_model(shape, X, y, par, keep, seed):
    """-> loss, the seven variables after AFM.partial_fit (SGD, lr 1, λ 0)."""
    from hhfm_amd.AFM import AFM
    F, k, A, B = shape
    E, w, w0, W, b, pvec, P = par
    m = AFM(1, 1, E.shape[0], 1, [A, k], None, 1.0, 0.0, list(keep), "GradientDescentOptimizer",
            0.999, F, random_seed=seed)
    m.set_weights(feature_embeddings=E, feature_bias=w[:, None], bias=w0, attention_W=W,
                  attention_b=b[None, :], attention_p=pvec, prediction=P[:, None])
    loss = m.partial_fit({"X": X.astype(np.int64), "Y": y[:, None]})
    G_ = m.get_weights()
    return loss, [np.asarray(G_[n], np.float32).reshape(np.shape(v)) for n, v in
                  zip(AFM_NAMES, par)]


def _afm_step_binding(X, y, par, keep, seed, lr=1.0):
    from hhfm_amd._native import native
    nat = native()
    B, F = X.shape
    M, k = par[0].shape
    A = par[3].shape[1]
    dev = [_dev(np.asarray(v, np.float32).reshape(-1)) for v in par]
    Xd, yd = _dev(X), _dev(y)
    ws = torch.zeros(nat.afm_train_workspace(B, F, k, A, M), dtype=torch.uint8, device="cuda")
    loss = torch.zeros(1, device="cuda")
    nat.afm_train_step_ex(Xd.data_ptr(), yd.data_ptr(), B, F, *[t.data_ptr() for t in dev[:3]],
                          M, k, A, *[t.data_ptr() for t in dev[3:]], lr, 0.0, SGD, keep[0],
                          keep[1], seed, [], ws.data_ptr(), ws.numel(), loss.data_ptr(),
                          _stream())
    return float(loss.item()), [t.cpu().numpy().reshape(np.shape(v)) for t, v in zip(dev, par)]


@pytest.mark.parametrize("keep", dr.AFM_KEEPS)
@pytest.mark.parametrize("shape", dr.AFM_SHAPES)
def test_afm_dropout_gradient_matches_float64(shape, keep):
    """np = 3 … 120 (pairs past lane 63), k = 8 … 256 (all four words of a
    block), B = 1 … 1030 (a head wave's second row); attention only, k-vector
    only, both.  AFM.partial_fit, first step of a model with random_seed 2016."""
    X, y, par = dr.afm_case(shape)
    seed = dr.model_seed(2016, 0)
    b1, b2 = dr.afm_masks(seed, shape, keep)
    ref_loss, grads = dr.afm_grad64_dropout(X, y, par, b1, b2, keep)
    loss, new = _afm_step_model(shape, X, y, par, keep, 2016)
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    for n, old, got, g in zip(AFM_NAMES, par, new, grads):
        ref = np.asarray(old, np.float64) - np.asarray(g, np.float64).reshape(np.shape(old))
        step = np.abs(ref - old).max()
        atol = 1e-4 * step + 1e-9
        err = np.abs(got - ref) - 1e-5 * np.abs(ref)
        print(f"afm {shape} keep {keep} {n}: worst err / atol = {float(err.max() / atol):.3g}")
        log_parity("train_grad_dropout", rows=int(ref.size), rows_kappa_gt_100=0,
                   max_rel_err_kappa_le_100=0.0, max_rel_err_kappa_gt_100=0.0,
                   oracle_max_rel_err_kappa_gt_100=0.0,
                   max_err_over_bound=float(err.max() / atol))
        assert np.allclose(got, ref, rtol=1e-5, atol=atol), n


def test_afm_dropped_prediction_columns_are_untouched():
    """B = 1: `prediction` keeps its bits at every column site 2 drops and
    moves at every column it keeps."""
    shape = (5, 256, 8, 1)
    rng = np.random.default_rng(9)
    F, k, A, B = shape
    M = F * dr.AFM_VOCAB
    X = (np.arange(F) * dr.AFM_VOCAB + rng.integers(0, dr.AFM_VOCAB, (1, F))).astype(np.int32)
    _, _, par = dr.afm_case((5, 256, 8, 2))
    y, keep, seed = np.float32([1.0]), (1.0, 0.5), 123 | 9 << 32
    b2 = dr.binary(seed, dr.SITE_AFM_VEC, 1, k, keep[1])[0]
    assert 0 < b2.sum() < k and par[0].shape == (M, k)
    _, new = _afm_step_binding(X, y, par, keep, seed)
    same = _bits(new[6]) == _bits(par[6])
    assert same[b2 == 0].all() and not same[b2 == 1].any()


def test_afm_row_with_every_pair_dropped():
    """F = 3, keep0 = 0.3 and a seed for which site 1 drops all three pairs:
    the attention path carries nothing, so E, attention_W / b / p and
    prediction keep their bits, w moves by g alone and the loss is
    (Σw + w0 − y)²/2."""
    shape, keep = (3, 8, 8, 1), (0.3, 1.0)
    seed = next(s for s in range(1000)
                if not dr.binary(s | 4 << 32, dr.SITE_AFM_ATT, 1, 3, keep[0]).any()) | 4 << 32
    X, y, par = dr.afm_case(shape)
    E, w, w0 = par[:3]
    out = np.float64(w[X[0]].astype(np.float64).sum() + np.float64(w0))
    g = out - np.float64(y[0])
    loss, new = _afm_step_binding(X, y, par, keep, seed)
    assert np.isclose(loss, 0.5 * g * g, rtol=1e-6)
    for i in (0, 3, 4, 5, 6):
        assert np.array_equal(_bits(new[i]), _bits(par[i])), AFM_NAMES[i]
    dw = w.astype(np.float64) - new[1]
    hit = np.zeros(len(w), bool)
    hit[X[0]] = True
    assert np.allclose(dw[hit], g, rtol=1e-6) and np.all(dw[~hit] == 0)
    assert np.isclose(np.float64(w0) - np.float64(new[2]), g, rtol=1e-6)
    # the same row with a seed that keeps a pair does move the attention path
    seed2 = next(s for s in range(1000)
                 if dr.binary(s | 4 << 32, dr.SITE_AFM_ATT, 1, 3, keep[0]).any()) | 4 << 32
    _, new2 = _afm_step_binding(X, y, par, keep, seed2)
    assert not np.array_equal(_bits(new2[0]), _bits(E))


# ---------------------------------------------------------------------------
# step counting, argument checks
# ---------------------------------------------------------------------------
def test_partial_fit_counts_steps_in_the_seed():
    """Two models with one random_seed take identical first steps; a model's
    second step on the same batch uses the mask of seed | 1 << 32."""
    from hhfm_amd.FM import FM
    rng = np.random.default_rng(4)
    M, F, k, keep, rs = 30, 5, 64, 0.5, 4242
    X = rng.permutation(M)[:F].astype(np.int64)[None, :]
    E = rng.normal(0, 0.2, (M, k)).astype(np.float32)
    w = rng.normal(0, 0.3, M).astype(np.float32)
    data = {"X": X, "Y": np.float32([[1.0]])}

    def model():
        m = FM(F, M, 1, M - 1, k, 1.0, 0.0, keep, "GradientDescentOptimizer", 0, 0,
               random_seed=rs)
        m.set_weights(feature_embeddings=E, feature_bias=w[:, None], bias=np.float32(0.02))
        return m

    a, b = model(), model()
    la, lb = a.partial_fit(data), b.partial_fit(data)
    Ea, Eb = a.get_weights()["feature_embeddings"], b.get_weights()["feature_embeddings"]
    assert la == lb and np.array_equal(_bits(Ea), _bits(Eb))
    a.partial_fit(data)
    Ea2 = a.get_weights()["feature_embeddings"]
    masks = [_gpu_mask(dr.model_seed(rs, s), dr.SITE_FM, 1, k, keep)[0] for s in (0, 1)]
    assert not np.array_equal(masks[0], masks[1]) and 0 < masks[1].sum() < k
    for before, after, bn in ((E, Ea, masks[0]), (Ea, Ea2, masks[1])):
        same = _bits(after)[X[0]] == _bits(before)[X[0]]
        assert same[:, bn == 0].all() and not same[:, bn == 1].any()


@pytest.mark.parametrize("model", ["fm", "afm"])
def test_keep_zero_is_refused_and_changes_nothing(model):
    from hhfm_amd._native import native
    nat = native()
    rng = np.random.default_rng(3)
    B, F, M, k, A = 8, 5, 40, 8, 8
    shapes = [(M, k), (M,), (1,)] + ([(k, A), (A,), (A,), (k,)] if model == "afm" else [])
    par = [_dev(rng.normal(0, 0.1, s).astype(np.float32)) for s in shapes]
    before = [p.clone() for p in par]
    X = _dev(rng.integers(0, M, (B, F)).astype(np.int32))
    y = _dev(rng.integers(0, 2, B).astype(np.float32))
    loss = torch.zeros(1, device="cuda")
    nbytes = (nat.train_workspace(M, k) if model == "fm"
              else nat.afm_train_workspace(B, F, k, A, M))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

    def call(keep):
        p = [t.data_ptr() for t in par]
        if model == "fm":
            nat.fm_train_step_ex(X.data_ptr(), y.data_ptr(), B, F, *p, M, k, 0.1, 0.0, SGD, keep,
                                 1, 0, 0, 0, ws.data_ptr(), nbytes, loss.data_ptr(), _stream())
        else:
            nat.afm_train_step_ex(X.data_ptr(), y.data_ptr(), B, F, *p[:3], M, k, A, *p[3:], 0.1,
                                  0.0, SGD, keep, 1.0, 1, [], ws.data_ptr(), nbytes,
                                  loss.data_ptr(), _stream())

    with pytest.raises(ValueError, match="invalid argument"):
        call(0.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(par, before))
    call(0.5)
    torch.cuda.synchronize()
    assert not torch.equal(par[0], before[0])


def test_model_classes_refuse_a_bad_keep():
    from hhfm_amd.AFM import AFM
    from hhfm_amd.FM import FM
    data = {"X": np.array([[0, 1, 2]], np.int64), "Y": np.float32([[1.0]])}
    for keep in (0.0, 1.5, float("nan")):
        m = FM(3, 10, 1, 9, 8, 0.1, 0.0, keep, "AdagradOptimizer", 0, 0)
        with pytest.raises(ValueError):
            m.partial_fit(data)
    for keep in ([0.0, 1.0], [1.0, 1.5], [0.5]):
        m = AFM(1, 1, 10, 1, [8, 8], None, 0.1, 0.0, keep, "AdagradOptimizer", 0.999, 3)
        with pytest.raises(ValueError):
            m.partial_fit(data)


# ---------------------------------------------------------------------------
# the reference's epoch loops with keep < 1
# ---------------------------------------------------------------------------
def _args(tmp_path, **kw):
    a = dict(path=G + "/", dataset="synth_frappe", epoch=3, batch_size=5000, hidden_factor=32,
             lamda=0.1, keep=1, lr=0.1, optimizer="AdagradOptimizer", verbose=1, batch_norm=0,
             TopK=10, Result=0, result_file=str(tmp_path / "result.txt"))
    a.update(kw)
    return argparse.Namespace(**a)


def test_fm_train_loop_with_dropout(tmp_path):
    from hhfm_amd.FM import Train
    np.random.seed(2016)
    t = Train(_args(tmp_path, keep=0.7))
    W0 = t.model.get_weights()
    losses = t.train()
    assert len(losses) == 2 and np.all(np.isfinite(losses))
    W = t.model.get_weights()
    assert not np.array_equal(W["feature_embeddings"], W0["feature_embeddings"])
    assert not np.array_equal(W["feature_bias"], W0["feature_bias"])
    # scoring stays at keep = 1
    X = t.data.Test_data.values[:200, 1:].astype(np.int64)
    ref = orc.fm_out(X, W["feature_embeddings"], W["feature_bias"][:, 0], W["bias"])[:, 0]
    got = t.model.score_rows(X)[:, 0]
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def test_afm_train_loop_with_dropout(tmp_path):
    from hhfm_amd.AFM import Train
    np.random.seed(2016)
    t = Train(_args(tmp_path, hidden_factor="[16,16]", keep="[0.8,0.5]", lamda_attention=100.0,
                    attention=1, decay=0.999, activation="relu"))
    W0 = t.model.get_weights()
    losses = t.train()
    assert len(losses) == 2 and np.all(np.isfinite(losses))
    W = t.model.get_weights()
    for n in ("feature_embeddings", "attention_W", "prediction"):
        assert not np.array_equal(W[n], W0[n]), n
    X = t.data.Test_data.values[:200, 1:].astype(np.int64)
    cur = [np.asarray(W[n], np.float32) for n in AFM_NAMES]
    ref = orc.afm_out(X, cur[0], cur[1], cur[2].reshape(()), *cur[3:])[:, 0]
    got = t.model.score_rows(X)[:, 0]
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
