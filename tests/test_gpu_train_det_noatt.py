"""The deterministic attention=0 AFM step (hhfm_afm_noatt_train_step_det;
include/hhfm.h "AFM without attention") on the GPU, as tests/test_gpu_train_det.py
does for FM.

1. Known answer: on an input whose forward is exact in fp32
   (tests/train_det_noatt_ref.noatt_known) one SGD step at lr 1 equals the
   numpy restatement of the documented orders bit for bit — E, w, w0, P — at
   keep 1 and 0.5, from a scratch filled with 0xA5.
2. Repeatability: two fresh runs, three steps of changing batch size on one
   scratch sized for the largest — every parameter, slot, the workspace and
   the loss bit for bit, for the four optimizers at keep 1 and 0.5.
3. Float64 parity: the bound of tests/test_gpu_train_grad.py on the gradient
   cases of tests/afm0_ref.py.
4. Edges: B = 0, a short or NULL scratch (everything untouched), the size query.

Measured on an MI355X, largest err / bound of (3): 0.024 (P of
F16_k256_B65_keep; E 0.023, w 0.0078, w0 0.0018 at most).
"""
import numpy as np
import pytest
import torch

from tests import afm0_ref as ar
from tests import dropout_ref as dref
from tests import train_det_noatt_ref as dn
from tests import train_ref as tr
from tests.test_gpu_afm0 import ADAGRAD, ADAM, MOMENTUM, SGD, _bits, _Step, _stream

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


class _Det(_Step):
    """_Step plus the scratch, filled with 0xA5: it need not be zeroed."""

    def __init__(self, Wt, opt, det_rows, F):
        super().__init__(Wt, opt)
        n = self.nat.afm_noatt_train_det_scratch(det_rows, F, self.k, self.M)
        self.sc = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        self.losses = []

    def step(self, X, y, lr, keep=1.0, seed=0, scratch=None):
        sc = (self.sc.data_ptr(), self.sc.numel()) if scratch is None else scratch
        self.nat.afm_noatt_train_step_det(*self.args(X, y, lr, keep, seed), *sc,
                                          self.loss.data_ptr(), _stream())
        self.losses.append(F32(self.loss.item()))
        return float(self.losses[-1])

    def state(self):
        return super().state() + [np.asarray(self.losses, F32)]


def _equal_states(a, b):
    return len(a) == len(b) and all(
        np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("keep", [1.0, 0.5])
def test_known_answer_bit_for_bit(keep):
    d = dn.noatt_known()
    B, k = len(d["X"]), d["k"]
    seed = 2016 | 9 << 32
    mask = dref.binary(seed, dref.SITE_AFM_VEC, B, k, keep) if keep < 1 else None
    ref = dn.step_ref(d["X"], d["y"], d["E"], d["w"], d["w0"], d["P"], mask, keep)
    s = _Det(d, SGD, B, 2)
    loss = s.step(d["X"], d["y"], 1.0, keep, seed)
    W1 = s.weights()
    for n, key in zip(ar.NAMES, ("dE", "dw", "dw0", "dP")):
        want = (np.asarray(d[n], F32) - ref[key]).astype(F32)      # var − lr·g, one rounding
        assert np.array_equal(_bits(W1[n]), _bits(want)), n
    assert np.array_equal(_bits(loss), _bits(ref["loss"]))
    assert np.abs(ref["dP"]).min() > 0


@pytest.mark.parametrize("keep", [1.0, 0.5])
@pytest.mark.parametrize("opt", [ADAGRAD, SGD, MOMENTUM, ADAM])
def test_steps_repeat_bit_for_bit(opt, keep):
    """B = 1,031 → 77 → 0 → 1,031 on a scratch sized for 1,031, F = 5, k = 64,
    M = 300, a hot user."""
    rng = np.random.default_rng(41)
    M, F, k = 300, 5, 64
    Wt = ar.weights(3, M, k)
    Wt["E"] = (Wt["E"] * F32(0.3)).astype(F32)
    batches = []
    for B in (1031, 77, 0, 1031):
        X = rng.integers(0, M, (B, F)).astype(np.int32)
        X[:, 0] = 0
        batches.append((X, rng.choice([-1.0, 1.0], B).astype(F32)))
    runs = []
    for _ in range(2):
        s = _Det(Wt, opt, 1031, F)
        for i, (X, y) in enumerate(batches):
            s.step(X, y, 0.05, keep, 2016 | i << 32)
        runs.append(s.state())
    assert _equal_states(*runs)
    assert not np.array_equal(_bits(runs[0][0]), _bits(Wt["E"]))
    assert np.all(np.isfinite(runs[0][-1])) and runs[0][-1][2] == 0.0


@pytest.mark.parametrize("name", sorted(ar.GRAD_CASES))
def test_gradient_matches_float64(name):
    X, y, Wt = ar.grad_case(name)
    mask, keep = ar.case_mask(name)
    ref_loss, Gd, Mg = ar.grad64(X, y, Wt["E"], Wt["w"], Wt["w0"], Wt["P"], mask, keep)
    s = _Det(Wt, SGD, len(X), X.shape[1])
    loss = s.step(X, y, 1.0, keep, ar.SEED)
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    W1 = s.weights()
    for n in ar.NAMES:
        before, after = np.asarray(Wt[n], F32), np.asarray(W1[n], F32)
        r = tr.ratio(before.astype(F64) - after.astype(F64), before, after, Gd[n], Mg[n])
        print(f"train_grad det afm0 {name} {n}: err / bound = {r:.3g}")
        assert r <= 1.0, (name, n, r)


def test_refusals_leave_everything_untouched():
    rng = np.random.default_rng(8)
    M, F, k, B = 50, 5, 16, 64
    Wt = ar.weights(4, M, k)
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    y = rng.choice([-1.0, 1.0], B).astype(F32)
    s = _Det(Wt, ADAM, B, F)
    n = s.sc.numel()
    assert n == s.nat.afm_noatt_train_det_scratch(B, F, k, M)
    assert s.nat.afm_noatt_train_det_scratch(B // 2, F, k, M) < n
    with pytest.raises(ValueError):
        s.nat.afm_noatt_train_det_scratch(2 ** 31, F, k, M)       # B·F does not fit an int
    with pytest.raises(ValueError):
        s.nat.afm_noatt_train_det_scratch(B, F, 260, M)
    before = s.state()
    half = s.nat.afm_noatt_train_det_scratch(B // 2, F, k, M)
    for scratch in ((0, n), (s.sc.data_ptr(), n - 1), (s.sc.data_ptr(), half)):
        with pytest.raises(ValueError):
            s.step(X, y, 0.1, 1.0, 0, scratch=scratch)
    for scratch in ((0, n), (s.sc.data_ptr(), 1)):                 # also at B = 0
        with pytest.raises(ValueError):
            s.step(X[:0], y[:0], 0.1, 1.0, 0, scratch=scratch)
    with pytest.raises(ValueError):
        s.step(X, y, 0.1, 1.5, 0)                                  # the default step's checks
    assert _equal_states(before[:-1], s.state()[:-1])
    assert np.array_equal(s.sc.cpu().numpy(), np.full(n, 0xA5, np.uint8))
    s.step(X, y, 0.1)                                              # and it still runs
    assert not np.array_equal(_bits(s.weights()["P"]), _bits(Wt["P"]))
