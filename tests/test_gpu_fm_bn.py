"""FM with batch_norm=1 on the GPU (include/hhfm.h "FM batch norm"):
hhfm_fm_train_step_bn and hhfm_fm_score_rows_scaled against the numpy
restatement of tests/fm_bn_ref.py.

* a designed known answer whose every contribution and sum is exact in fp32 in
  any order: one SGD step equals the restatement bit for bit;
* B = 1 (v = 0, x̂ = 0: no gradient reaches E or γ);
* every gradient against float64 with the project's bar, 1e-5 of the
  propagated magnitude (tests/train_ref.ratio <= 1), on the step shapes of
  tests/test_gpu_train_grad.py and the dropout keeps of tests/test_gpu_dropout.py;
* three partial_fit steps replayed from the GPU's own pre-step state, moving
  statistics included;
* the inference score with tests/helpers.kappa_check, and the scaled entry
  point's bits at scale ≡ 1;
* the argument rules and the command-line surface.

Measured on an MI355X, largest err / bound per variable over the gradient
cases: E 0.026 (k260 at keep 0.7; 0.00068 without dropout), w 0.0028
(B63_hot), w0 0.00059, γ 0.0010 (F12), β 0.00096 (k64 at the reference's
initialisation); B32773: E 0.00024, w 0.0019, w0 0.00022, γ 0.00013, β 0.00026.
No case passes 0.03.  Moving statistics: mean 0.0073 of its tolerance at most,
variance 0.52 (there the tolerance is the stored value's ulp).
"""
import os

import numpy as np
import pytest
import torch

from oracle import fm_oracle as orc
from tests import dropout_ref as dr
from tests import fm_bn_ref as bn
from tests import train_ref as tr
from tests.helpers import bf16_round, kappa_check, log_parity

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
SGD, ADAGRAD = 1, 0
BN_KEYS = ["bn_gamma", "bn_beta", "bn_moving_mean", "bn_moving_variance"]
ALL_KEYS = ["feature_embeddings", "feature_bias", "bias"] + BN_KEYS


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


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
    log_parity("train_grad_bn", rows=int(g.size), rows_kappa_gt_100=int(((g > 0) & ~well).sum()),
               max_rel_err_kappa_le_100=float(rel[well].max()) if well.any() else 0.0,
               max_rel_err_kappa_gt_100=0.0, oracle_max_rel_err_kappa_gt_100=0.0,
               max_err_over_bound=r)
    print(f"train_grad_bn {what}: err / bound = {r:.3g}")
    assert r <= 1.0, (what, r)


class _Step:
    """Device buffers of one hhfm_fm_train_step_bn call through the binding."""

    def __init__(self, X, y, E, w, w0, gamma, beta, mm=None, mv=None, opt=SGD):
        from hhfm_amd._native import native
        self.nat = native()
        self.B, self.F = X.shape
        self.M, self.k = E.shape
        k = self.k
        self.X, self.y = _dev(np.asarray(X, np.int32)), _dev(np.asarray(y, np.float32))
        host = [E, w, np.float32([w0]), gamma, beta,
                np.zeros(k, np.float32) if mm is None else mm,
                np.ones(k, np.float32) if mv is None else mv]
        self.par = [_dev(np.asarray(h, np.float32)) for h in host]
        self.acc = [torch.full((2 * p.numel(),), 0.1, device="cuda") for p in self.par[:5]]
        self.before = [p.clone() for p in self.par + self.acc]
        self.loss = torch.zeros(1, device="cuda")
        self.opt = opt
        self.ws = torch.zeros(self.nat.fm_train_bn_workspace(self.B, self.M, k),
                              dtype=torch.uint8, device="cuda")

    def run(self, lr=1.0, lam=0.0, keep=1.0, seed=0, eps=bn.EPS, upd=bn.BN_UPDATE, B=None,
            ws_bytes=None, null=()):
        E, w, w0, gamma, beta, mm, mv = (p.data_ptr() for p in self.par)
        ptr = dict(gamma=gamma, beta=beta, mm=mm, mv=mv)
        for n in null:
            ptr[n] = 0
        aE, aw, a0, ag, ab = (a.data_ptr() for a in self.acc)
        self.nat.fm_train_step_bn(
            self.X.data_ptr(), self.y.data_ptr(), self.B if B is None else B, self.F, E, w, w0,
            self.M, self.k, lr, lam, self.opt, keep, seed, aE, aw, a0, self.ws.data_ptr(),
            self.ws.numel() if ws_bytes is None else ws_bytes, ptr["gamma"], ptr["beta"],
            ptr["mm"], ptr["mv"], eps, upd, ag, ab, self.loss.data_ptr(), _stream())
        return float(self.loss.item())

    def host(self):
        return [p.cpu().numpy() for p in self.par]

    def unchanged(self):
        torch.cuda.synchronize()
        return all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                   for a, b in zip(self.par + self.acc, self.before))


# ---------------------------------------------------------------------------
# 1. the known answer, bit for bit
# ---------------------------------------------------------------------------
def test_known_answer_bit_for_bit():
    """B = 256, F = 2, k = 8, eps = 3 through the binding: x = ±1, μ = 0, v = 1,
    inv = ½; one SGD step (lr 1, λ 0) moves E, w, w0, γ, β by exactly the
    restatement's gradients, the loss is the float64 loss within 1 ulp, and
    the moving statistics (0 and 1) keep their bits."""
    X, y, E, w, w0, gamma, beta = bn.known_answer()
    ref = bn.fm_bn_step(X, y, E, w, w0, gamma, beta, eps=bn.KNOWN_EPS)
    s = _Step(X, y, E, w, w0, gamma, beta)
    loss = s.run(eps=bn.KNOWN_EPS)
    E1, w1, w01, g1, b1, mm, mv = s.host()
    for name, before, after, grad in (("E", E, E1, ref["dE"]), ("w", w, w1, ref["dw"]),
                                      ("w0", np.float32([w0]), w01, ref["dw0"]),
                                      ("gamma", gamma, g1, ref["dgamma"]),
                                      ("beta", beta, b1, ref["dbeta"])):
        delta = np.asarray(before, np.float32) - np.asarray(after, np.float32)
        assert _same_bits(delta.reshape(-1), np.asarray(grad, np.float32).reshape(-1)), name
    assert abs(np.float32(loss) - np.float32(ref["loss"])) <= np.spacing(np.float32(ref["loss"]))
    assert _same_bits(mm, np.zeros(8)) and _same_bits(mv, np.ones(8))
    assert np.count_nonzero(ref["dE"]) == 144


# ---------------------------------------------------------------------------
# 2. B = 1
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 100])
def test_single_row_batch(k):
    """v = 0 and x̂ = 0: dE and dγ are exactly zero, so E and γ keep their bits
    under SGD with λ = 0; β, w, w0 move by g; mv moves towards 0 by bn_update
    and mm towards x."""
    rng = np.random.default_rng(k)
    M, F = 30, 5
    X = rng.permutation(M)[:F].astype(np.int32)[None, :]
    E = rng.normal(0, 0.3, (M, k)).astype(np.float32)
    w = rng.normal(0, 0.3, M).astype(np.float32)
    gamma = rng.normal(1, 0.2, k).astype(np.float32)
    beta = rng.normal(0, 0.2, k).astype(np.float32)
    y, w0 = np.float32([-1.0]), np.float32(0.02)
    ref = bn.fm_bn_step(X, y, E, w, w0, gamma, beta)
    g = float(ref["g"][0])
    assert abs(g) > 0.5            # out − y does not cancel: g and the loss are well conditioned
    s = _Step(X, y, E, w, w0, gamma, beta)
    loss = s.run()
    E1, w1, w01, g1, b1, mm, mv = s.host()
    assert _same_bits(E1, E) and _same_bits(g1, gamma)
    assert np.isclose(loss, ref["loss"], rtol=1e-5)
    assert np.allclose(beta - b1, g, rtol=1e-5, atol=2.0 ** -23)
    assert np.allclose((w - w1)[X[0]], g, rtol=1e-5, atol=2.0 ** -23)
    assert np.isclose(w0 - w01[0], g, rtol=1e-5, atol=2.0 ** -23)
    untouched = np.setdiff1d(np.arange(M), X[0])
    assert _same_bits(w1[untouched], w[untouched])
    u = np.float32(bn.BN_UPDATE)
    assert _same_bits(mv, np.ones(k, np.float32) - (np.ones(k, np.float32) - np.float32(0)) * u)
    assert np.allclose(mm, ref["x"][0] * bn.BN_UPDATE, rtol=1e-5, atol=1e-9)


# ---------------------------------------------------------------------------
# 3. gradient parity against float64
# ---------------------------------------------------------------------------
def _model(F, M, k, lr, lam, keep, opt, seed=2016, **kw):
    from hhfm_amd.FM import FM
    return FM(F, M, 1, M - 1, k, lr, lam, keep, opt, 1, 0, random_seed=seed, **kw)


def _bn_params(name, k):
    rng = np.random.default_rng(sorted(dr.FM_CASES).index(name) + 700)
    return rng.normal(1, 0.2, k).astype(np.float32), rng.normal(0, 0.2, k).astype(np.float32)


def _grad_case(what, X, y, E, w, w0, gamma, beta, keep=1.0):
    """One SGD step (lr 1, λ 0) through FM.partial_fit (random_seed 2016, its
    first step) against fm_bn_grad64."""
    B, F = X.shape
    M, k = E.shape
    bin_ = None if keep == 1.0 else dr.binary(2016, dr.SITE_FM, B, k, keep)
    ref_loss, grads, mags, _ = bn.fm_bn_grad64(X, y, E, w, w0, gamma, beta, bin_=bin_, keep=keep)
    m = _model(F, M, k, 1.0, 0.0, keep, "GradientDescentOptimizer")
    m.set_weights(feature_embeddings=E, feature_bias=w[:, None], bias=w0, bn_gamma=gamma,
                  bn_beta=beta)
    loss = m.partial_fit({"X": X.astype(np.int64), "Y": y[:, None]})
    W = m.get_weights()
    print(f"train_grad_bn {what}: loss {loss!r} float64 {ref_loss!r}")
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    after = (W["feature_embeddings"], W["feature_bias"][:, 0], np.float32(W["bias"]),
             W["bn_gamma"], W["bn_beta"])
    for name, b, a, g, mg in zip("E w w0 gamma beta".split(), (E, w, w0, gamma, beta), after,
                                 grads, mags):
        _check(f"{what} {name}", b, a, g, mg)


GRAD_CASES = ["k4", "k64", "k68", "k200", "F1", "F2", "F12", "B63_hot", "B2049_hot", "B32773"]


@pytest.mark.parametrize("name", GRAD_CASES)
def test_bn_gradient_matches_float64(name):
    """k = 4 … 200 (one, two and partial column slabs), F = 1 (x ≡ 0, v = 0: no
    gradient passes the layer), F = 2, 12, a hot user, B = 2,049 (several
    workgroups' partials) and B = 32,773 (what the batch sums must survive);
    γ ~ N(1, 0.2), β ~ N(0, 0.2)."""
    X, y, E, w, w0 = tr.fm_case(name)
    gamma, beta = _bn_params(name, E.shape[1])
    _grad_case(f"fm_bn {name}", X, y, E, w, w0, gamma, beta)


def test_bn_gradient_at_the_reference_initialisation():
    """k64 with E ~ N(0, 0.01) (FM.py:152): v ≪ eps, the layer is all eps."""
    X, y, E, w, w0 = tr.fm_case("k64")
    E = np.random.default_rng(64).normal(0, 0.01, E.shape).astype(np.float32)
    gamma, beta = _bn_params("k64", E.shape[1])
    _grad_case("fm_bn k64_init", X, y, E, w, w0, gamma, beta)


@pytest.mark.parametrize("keep", dr.FM_KEEPS)
def test_bn_gradient_with_dropout(keep):
    """k = 260 (a lane's fifth column opens a second Philox block) at keep 0.5,
    0.7, 0.9: the mask of tests/dropout_ref.binary, applied after the layer."""
    X, y, E, w, w0 = dr.fm_case("k260")
    gamma, beta = _bn_params("k260", E.shape[1])
    _grad_case(f"fm_bn k260 keep {keep}", X, y, E, w, w0, gamma, beta, keep)


# ---------------------------------------------------------------------------
# 4. moving statistics and the step as a whole
# ---------------------------------------------------------------------------
NAMES = ["feature_embeddings", "feature_bias", "bias", "bn_gamma", "bn_beta"]


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)))


@pytest.mark.parametrize("opt,lam", [("AdagradOptimizer", 0.01), ("AdamOptimizer", 0.0)])
def test_partial_fit_replayed_step_by_step(opt, lam):
    """Three partial_fit steps (B = 700, k = 32, Frappe-shaped rows), each
    replayed from the GPU's own pre-step weights and slots: the float64
    gradients of the restatement through the oracle's TF optimizer rules, with
    the bars of tests/test_gpu_training.py for variables and slots; the moving
    statistics within 1e-5·bn_update·mean|x| (mean) and 1e-5·bn_update·mean
    (x−μ)² (variance) of the replay, plus 1 ulp of the stored value."""
    from tests.test_gpu_training import OPTS, _check_slot, _check_var, _rows, _slot
    o = OPTS[opt]
    rng = np.random.default_rng(4)
    nu, ni, k, B, lr = 200, 500, 32, 700, 0.1
    X, M = _rows(rng, 3 * B, nu, ni, (7, 2, 3))
    m = _model(5, M, k, lr, lam, 1, opt)
    m.set_weights(feature_embeddings=rng.normal(0, 0.1, (M, k)).astype(np.float32),
                  feature_bias=rng.normal(0, 0.01, M).astype(np.float32)[:, None],
                  bias=np.float32(0.02), bn_gamma=rng.normal(1, 0.2, k).astype(np.float32),
                  bn_beta=rng.normal(0, 0.2, k).astype(np.float32))
    u = m.bn_update
    for step in range(3):
        Xb = X[step * B:(step + 1) * B]
        y = rng.integers(0, 2, B).astype(np.float32)[:, None]
        Wg = m.get_weights()
        cur = [Wg["feature_embeddings"], Wg["feature_bias"][:, 0], np.float32(Wg["bias"]),
               Wg["bn_gamma"], Wg["bn_beta"]]
        st = getattr(m, "_train_state", None)
        sl = [_slot(o, v) if st is None else st[n].cpu().numpy() for n, v in zip(NAMES, cur)]
        loss = m.partial_fit({"X": Xb, "Y": y})
        r = bn.fm_bn_step(Xb, y, *cur)
        E64 = cur[0].astype(np.float64)
        ref_loss = r["loss"] + lam * (E64 ** 2).sum() / 2
        assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
        grads = [r["dE"] + lam * E64, r["dw"], r["dw0"], r["dgamma"], r["dbeta"]]
        rows = [Xb if lam == 0 else None, Xb, None, None, None]
        Wn = m.get_weights()
        got = [Wn["feature_embeddings"], Wn["feature_bias"][:, 0], np.float32(Wn["bias"]),
               Wn["bn_gamma"], Wn["bn_beta"]]
        for n, var, g, s0, rw, gv in zip(NAMES, cur, grads, sl, rows, got):
            var = np.asarray(var, np.float32)
            ref_var, ref_slot = orc.tf_apply(o, var, np.asarray(g, np.float32), s0, lr, step + 1,
                                             rw)
            shape = (1,) if var.ndim == 0 else var.shape
            _check_var(np.asarray(gv).reshape(shape), np.asarray(ref_var).reshape(shape),
                       var.reshape(shape), o, np.asarray(g, np.float32).reshape(shape))
            _check_slot(m._train_state[n].cpu().numpy(), ref_slot, o)
        mm_ref, mv_ref = bn.moving_update64(Wg["bn_moving_mean"], Wg["bn_moving_variance"],
                                            r["mu"], r["v"], u)
        tol_m = 1e-5 * u * np.abs(r["x"]).mean(0) + _ulp(Wn["bn_moving_mean"])
        tol_v = 1e-5 * u * ((r["x"] - r["mu"]) ** 2).mean(0) + _ulp(Wn["bn_moving_variance"])
        em = np.abs(Wn["bn_moving_mean"] - mm_ref)
        ev = np.abs(Wn["bn_moving_variance"] - mv_ref)
        print(f"fm_bn step {step} {opt}: moving mean err / tol {float((em / tol_m).max()):.3g}, "
              f"variance {float((ev / tol_v).max()):.3g}")
        assert np.all(em <= tol_m) and np.all(ev <= tol_v)
        assert not _same_bits(Wn["bn_moving_mean"], Wg["bn_moving_mean"])


# ---------------------------------------------------------------------------
# 5. inference
# ---------------------------------------------------------------------------
def _score_case(k, F, B, dtype, seed):
    rng = np.random.default_rng(seed)
    M = 60
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    std = min(0.3, (k * F * F / 2.0) ** -0.25)
    E = rng.normal(0, std, (M, k)).astype(np.float32)
    w = rng.normal(0, 0.3, M).astype(np.float32)
    stats = dict(bn_gamma=rng.normal(1, 0.3, k), bn_beta=rng.normal(0, 0.3, k) / k,
                 bn_moving_mean=rng.normal(0, 0.05, k), bn_moving_variance=rng.uniform(0.01, 2, k))
    stats = {n: v.astype(np.float32) for n, v in stats.items()}
    return X, E, w, np.float32(0.02), stats


SCORE_CASES = [(64, 5, 4099, torch.float32), (64, 3, 257, torch.float32),
               (128, 5, 63, torch.bfloat16), (6, 12, 1, torch.float32),
               (6, 12, 257, torch.float32), (64, 5, 1, torch.float32)]


@pytest.mark.parametrize("k,F,B,dtype", SCORE_CASES)
def test_inference_score_matches_exact(k, F, B, dtype):
    """score_rows and sess.run(model.out) on the moving statistics: the fast
    kernel (k = 64 fp32 at F = 5 and 3, k = 128 bf16) and the generic one
    (k = 6, F = 12), B = 1 … 4,099, non-trivial γ, β, mm, mv.  The oracle reads
    the bf16-rounded table, as elsewhere."""
    X, E, w, w0, stats = _score_case(k, F, B, dtype, 10 * k + F + B)
    m = _model(F, 60, k, 0.1, 0.0, 1, "AdagradOptimizer", table_dtype=dtype)
    m.set_weights(feature_embeddings=E, feature_bias=w[:, None], bias=w0, **stats)
    before = m.get_weights()
    got = m.score_rows(X)
    Et = bf16_round(E) if dtype == torch.bfloat16 else E
    exact, mag = bn.fm_bn_score64(X, Et, w, w0, stats["bn_gamma"], stats["bn_beta"],
                                  stats["bn_moving_mean"], stats["bn_moving_variance"])
    kappa_check("fm_bn_rows", got, None, exact, mag)
    via_sess = m.sess.run(m.out, feed_dict={m.train_features: X, m.train_phase: False})
    assert _same_bits(via_sess, got)
    after = m.get_weights()
    assert all(_same_bits(before[n], after[n]) for n in ALL_KEYS)


@pytest.mark.parametrize("k,F,B,dtype", SCORE_CASES)
def test_scale_of_ones_has_the_plain_kernels_bits(k, F, B, dtype):
    from hhfm_amd import ops
    X, E, w, w0, _ = _score_case(k, F, B, dtype, 10 * k + F + B)
    Xd, Ed, wd = _dev(X), _dev(E).to(dtype).contiguous(), _dev(w)
    plain = ops.fm_score_rows(Xd, Ed, wd, float(w0))
    scaled = ops.fm_score_rows(Xd, Ed, wd, float(w0), scale=torch.ones(k, device="cuda"))
    assert torch.equal(plain.view(torch.int32), scaled.view(torch.int32))
    now = ops.fm_score_rows(Xd, Ed, None, float(w0), scale=torch.ones(k, device="cuda"))
    assert torch.equal(ops.fm_score_rows(Xd, Ed, None, float(w0)).view(torch.int32),
                       now.view(torch.int32))


@pytest.mark.parametrize("k,F", [(64, 5), (6, 12)])
def test_scaled_rows_flag_a_bad_id_and_read_row_0(k, F):
    from hhfm_amd import ops
    X, E, w, w0, stats = _score_case(k, F, 257, torch.float32, k)
    scale = _dev(stats["bn_gamma"])
    Xbad = X.copy()
    Xbad[100, 1], Xbad[200, F - 1] = 60 + 5, -3
    Xfix = X.copy()
    Xfix[100, 1], Xfix[200, F - 1] = 0, 0
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ok = ops.fm_score_rows(_dev(Xfix), _dev(E), _dev(w), float(w0), status=status, scale=scale)
    assert int(status.item()) == 0
    bad = ops.fm_score_rows(_dev(Xbad), _dev(E), _dev(w), float(w0), status=status, scale=scale)
    assert int(status.item()) == 1
    assert torch.equal(ok.view(torch.int32), bad.view(torch.int32))
    with pytest.raises(ValueError, match="no flags"):
        ops.fm_score_rows(_dev(X), _dev(E), _dev(w), float(w0), flags=2, scale=scale)


def test_scoring_after_training_writes_no_weight():
    rng = np.random.default_rng(9)
    X, y, E, w, w0 = tr.fm_case("k64")
    m = _model(5, 50, 64, 0.1, 0.01, 0.7, "AdagradOptimizer")
    m.set_weights(feature_embeddings=E, feature_bias=w[:, None], bias=w0)
    for _ in range(2):
        m.partial_fit({"X": X.astype(np.int64), "Y": y[:, None]})
    before = m.get_weights()
    assert not _same_bits(before["bn_moving_mean"], np.zeros(64))
    got = m.score_rows(X[rng.permutation(len(X))[:100]])
    assert np.all(np.isfinite(got))
    after = m.get_weights()
    assert sorted(after) == sorted(ALL_KEYS)
    assert all(_same_bits(before[n], after[n]) for n in ALL_KEYS)


# ---------------------------------------------------------------------------
# 6. edges: the binding's error, every weight and slot bit for bit as it was
# ---------------------------------------------------------------------------
def _edge_step(opt=ADAGRAD):
    rng = np.random.default_rng(12)
    B, F, M, k = 8, 5, 40, 8
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    return _Step(X, rng.integers(0, 2, B).astype(np.float32),
                 rng.normal(0, 0.1, (M, k)).astype(np.float32),
                 rng.normal(0, 0.1, M).astype(np.float32), np.float32(0.02),
                 rng.normal(1, 0.2, k).astype(np.float32), rng.normal(0, 0.2, k).astype(np.float32),
                 rng.normal(0, 0.1, k).astype(np.float32),
                 rng.uniform(0.5, 2, k).astype(np.float32), opt=opt)


@pytest.mark.parametrize("kw", [dict(B=0), dict(eps=0.0), dict(eps=float("nan")),
                                dict(upd=1.5), dict(null=("gamma",)), dict(null=("mv",))],
                         ids=["B0", "eps0", "epsNaN", "update1.5", "null_gamma", "null_mv"])
def test_bn_step_refuses_bad_arguments(kw):
    s = _edge_step()
    with pytest.raises(ValueError, match="invalid argument"):
        s.run(lr=0.1, lam=0.1, **kw)
    assert s.unchanged()


def test_bn_step_refuses_a_workspace_one_byte_short():
    s = _edge_step()
    with pytest.raises(ValueError, match="workspace too small"):
        s.run(lr=0.1, lam=0.1, ws_bytes=s.ws.numel() - 1)
    assert s.unchanged()
    s.run(lr=0.1, lam=0.1)                       # the exact size is taken
    assert not s.unchanged()


def test_model_level_rules():
    from hhfm_amd.FM import FM
    with pytest.raises(NotImplementedError, match="deterministic"):
        FM(5, 40, 1, 39, 8, 0.1, 0.0, 1, "AdagradOptimizer", 1, 0, deterministic=True)
    m = _model(5, 40, 8, 0.1, 0.0, 1, "AdagradOptimizer")
    X = np.random.default_rng(1).integers(0, 40, (6, 5))
    with pytest.raises(NotImplementedError, match="train_phase"):
        m.sess.run(m.out, feed_dict={m.train_features: X, m.train_phase: True})
    assert sorted(m.weights) == sorted(ALL_KEYS)
    W = m.get_weights()
    assert np.all(W["bn_gamma"] == 1) and np.all(W["bn_beta"] == 0)
    assert np.all(W["bn_moving_mean"] == 0) and np.all(W["bn_moving_variance"] == 1)
    plain = FM(5, 40, 1, 39, 8, 0.1, 0.0, 1, "AdagradOptimizer", 0, 0)
    assert sorted(plain.weights) == ["bias", "feature_bias", "feature_embeddings"]
    # an empty batch is refused with every weight as it was
    before = m.get_weights()
    with pytest.raises(ValueError, match="invalid argument"):
        m.partial_fit({"X": np.zeros((0, 5), np.int64), "Y": np.zeros((0, 1), np.float32)})
    assert all(_same_bits(before[n], m.get_weights()[n]) for n in ALL_KEYS)
    # training refuses bf16 tables as the plain step does; scoring takes them
    b16 = _model(5, 40, 8, 0.1, 0.0, 1, "AdagradOptimizer", table_dtype=torch.bfloat16)
    assert np.all(np.isfinite(b16.score_rows(X)))
    with pytest.raises(NotImplementedError, match="fp32"):
        b16.partial_fit({"X": X, "Y": np.ones((6, 1), np.float32)})


def test_workspace_grows_with_the_batch_and_keeps_adams_powers():
    """Steps at B = 64, 300, 64: the larger batch reallocates the workspace and
    the persistent prefix is carried over — Adam's β powers (the scalar block
    of hhfm_train_workspace's layout) stand at β^4 after three steps, and the
    rest of the prefix (touched mask, dγ, dβ) is left zeroed."""
    rng = np.random.default_rng(2)
    M, k = 50, 16
    m = _model(5, M, k, 0.1, 0.0, 1, "AdamOptimizer")
    sizes = (64, 300, 64)
    for n in sizes:
        X = rng.integers(0, M, (n, 5))
        m.partial_fit({"X": X, "Y": rng.integers(0, 2, (n, 1)).astype(np.float32)})
    ws = m._train_state["ws"]
    from hhfm_amd._native import native
    assert ws.numel() == native().fm_train_bn_workspace(300, M, k)
    off = native().train_workspace(M, k)            # scal sits before the touched mask
    scal_end = (M * k + M + 16) * 4
    pw = ws[scal_end - 8 * 4:scal_end - 5 * 4].view(torch.float32).cpu().numpy()
    b1, b2 = orc.adam_powers(len(sizes) + 1)
    assert off >= scal_end and np.allclose(pw, [b1, b2, 1.0], rtol=1e-6)
    state = native().fm_train_bn_state_bytes(M, k)
    assert not ws[:state].view(torch.uint8)[scal_end:].any()      # left zeroed


# ---------------------------------------------------------------------------
# 7. surface
# ---------------------------------------------------------------------------
def test_fm_main_with_batch_norm(tmp_path):
    """FM_main … --batch_norm 1: the loss falls, score_rows equals the
    restatement on the trained weights, and topk is the topk of a
    batch_norm=0 model with the same E and w (the reference's catalog score
    does not pass through the layer)."""
    from hhfm_amd.FM import FM, FM_main
    np.random.seed(2016)
    session = FM_main("synth_frappe", 16, 5,
                      ["--path", G + "/", "--batch_norm", "1", "--epoch", "3", "--Result", "1",
                       "--batch_size", "4096", "--verbose", "0",
                       "--result_file", str(tmp_path / "result.txt")])
    losses = session.loss_epoch
    assert len(losses) == 2 and np.all(np.isfinite(losses)) and losses[1] < losses[0]
    m = session.model
    assert m.batch_norm == 1
    W = m.get_weights()
    assert sorted(W) == sorted(ALL_KEYS)
    assert not _same_bits(W["bn_moving_variance"], np.ones(16))
    rows = session.data.Test_data.values[:300, 1:].astype(np.int64)
    exact, mag = bn.fm_bn_score64(rows, W["feature_embeddings"], W["feature_bias"][:, 0],
                                  W["bias"], W["bn_gamma"], W["bn_beta"], W["bn_moving_mean"],
                                  W["bn_moving_variance"])
    kappa_check("fm_bn_rows", m.score_rows(rows), None, exact, mag)
    plain = FM(m.valid_dimension, m.features_M, m.n_user, m.n_item, 16, 0.1, 0.1, 1,
               "AdagradOptimizer", 0, 0)
    plain.set_weights(feature_embeddings=W["feature_embeddings"], feature_bias=W["feature_bias"],
                      bias=W["bias"])
    assert np.array_equal(m.topk(rows[:40], 5), plain.topk(rows[:40], 5))
