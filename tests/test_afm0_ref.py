"""CPU checks of the attention=0 AFM oracles (tests/afm0_ref.py,
tests/train_det_noatt_ref.py) and of the inputs the GPU tests run on.

* the float64 oracle against the reference's own numbers (tests/golden/afm0.npz,
  written by make_golden_afm0.py from the unmodified Newcode/AFM.py): ``out``
  within 1e-5·Σ|terms|, the loss within 1e-5 relative, and the reference's
  loss the same at lamda_attention 100 and 0 (no regulariser);
* its analytic gradients against torch.autograd in float64, to 1e-12 relative
  (an independent derivation, not finite differences);
* for every GPU gradient case the fp32 oracle alone sits at err / bound <= 0.25
  (the rule of tests/test_train_ref.py), so the bound leaves the kernel room;
* every catalog query set is gap-clean at 1e-5·Σ|terms| among its top K + 1
  (the designed tie case: but for the exact zeros of the duplicated items);
* the deterministic orders against a plain float64 sum, to the fp32 bound;
* parse_args.
"""
import os

import numpy as np
import pytest
import torch

from tests import afm0_ref as ar
from tests import dropout_ref as dref
from tests import train_det_noatt_ref as dn
from tests import train_ref as tr

G = os.path.join(os.path.dirname(__file__), "golden")
F32, F64 = np.float32, np.float64
SEED = ar.SEED


def _golden(k):
    z = np.load(os.path.join(G, "afm0.npz"))
    p = f"k{k}_"
    return {n: z[p + n] for n in ("E", "w", "w0", "P", "X", "out", "Y", "loss_lam100",
                                   "loss_lam0")}


@pytest.mark.parametrize("k", [16, 64])
def test_oracle_matches_the_reference(k):
    g = _golden(k)
    assert not np.allclose(g["P"], 1.0)               # a kernel that drops P must fail
    out, S = ar.out64(g["X"], g["E"], g["w"], g["w0"], g["P"])
    assert np.all(np.abs(g["out"] - out) <= 1e-5 * S)
    assert g["loss_lam100"] == g["loss_lam0"]         # AFM.py:148: no regulariser
    loss = ar.loss64(g["X"], g["Y"], g["E"], g["w"], g["w0"], g["P"])
    assert np.isclose(g["loss_lam0"], loss, rtol=1e-5)


def _autograd(X, y, Wt, mask, keep):
    t = {n: torch.tensor(np.asarray(Wt[n], F64), requires_grad=True) for n in ar.NAMES}
    Xt = torch.as_tensor(np.asarray(X, np.int64))
    e = t["E"][Xt]                                    # [B, F, k]
    pairs = torch.zeros(e.shape[0], e.shape[2], dtype=torch.float64)
    for i in range(e.shape[1]):                       # Σ_{i<j} e_i ⊙ e_j, as AFM.py:107-115
        for j in range(i + 1, e.shape[1]):
            pairs = pairs + e[:, i] * e[:, j]
    if mask is not None:
        pairs = pairs / keep * torch.as_tensor(np.asarray(mask, F64))
    out = pairs @ t["P"] + t["w"][Xt].sum(1) + t["w0"]
    loss = 0.5 * ((torch.as_tensor(np.asarray(y, F64)) - out) ** 2).sum()
    loss.backward()
    return float(loss.detach()), {n: t[n].grad.numpy() for n in ar.NAMES}


@pytest.mark.parametrize("keep", [1.0, 0.5])
@pytest.mark.parametrize("F,k,B", [(3, 4, 5), (5, 16, 40)])
def test_analytic_gradients_match_autograd(F, k, B, keep):
    rng = np.random.default_rng(31 + F + k)
    M = 12
    Wt = ar.weights(77, M, k)
    X = rng.integers(0, M, (B, F))
    X[1, F - 1] = X[1, 0]
    y = rng.choice([-1.0, 1.0], B)
    mask = dref.binary(SEED, dref.SITE_AFM_VEC, B, k, keep) if keep < 1 else None
    loss, Gd, _ = ar.grad64(X, y, Wt["E"], Wt["w"], Wt["w0"], Wt["P"], mask, keep)
    la, Ga = _autograd(X, y, Wt, mask, keep)
    assert abs(loss - la) <= 1e-12 * abs(la)
    for n in ar.NAMES:
        a, b = np.asarray(Gd[n], F64), np.asarray(Ga[n], F64)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), n


@pytest.mark.parametrize("name", sorted(ar.GRAD_CASES))
def test_fp32_oracle_sits_inside_the_bound(name):
    X, y, Wt = ar.grad_case(name)
    mask, keep = ar.case_mask(name)
    loss, Gd, Mg = ar.grad64(X, y, Wt["E"], Wt["w"], Wt["w0"], Wt["P"], mask, keep)
    l32, G32 = ar.grad32(X, y, Wt["E"], Wt["w"], Wt["w0"], Wt["P"], mask, keep)
    assert np.isclose(l32, loss, rtol=1e-5)
    for n in ar.NAMES:
        before = np.asarray(Wt[n], F32)
        after = (before - np.asarray(G32[n], F32)).astype(F32)
        r = tr.ratio(np.asarray(G32[n], F64), before, after, Gd[n], Mg[n])
        print(f"afm0 fp32 oracle {name} {n}: err / bound = {r:.3g}")
        assert r <= 0.25, (name, n, r)


@pytest.mark.parametrize("k", ar.CAT_K)
@pytest.mark.parametrize("n_item", ar.CAT_ITEMS)
def test_catalog_queries_are_gap_clean(n_item, k):
    """The recorded seed search: ``rejected`` lists the pool positions left out."""
    c = ar.catalog_case(n_item, k)
    assert c["gap"] > ar.BAR and len(c["q"]) == max(ar.CAT_B)
    print(f"afm0 catalog n_item={n_item} k={k}: seed {c['seed']}, {len(c['rejected'])} of the "
          f"pool rejected, least gap / Σ|terms| = {c['gap']:.3g}")
    # B = 1 and 8 take the first rows: the same margin through min_top_gap
    assert ar.min_top_gap(c["q"][:8], c["Wt"], c["n_user"], n_item, c["K"]) > ar.BAR


@pytest.mark.parametrize("n_item,k,bf16,dup", [(4100, 64, True, False), (4100, 64, False, True),
                                               (70000, 16, False, True)])
def test_special_catalog_cases(n_item, k, bf16, dup):
    c = ar.catalog_case(n_item, k, bf16, dup)
    assert c["gap"] > ar.BAR
    if dup:   # the designed tie: the three duplicated items lead every list, index-ascending
        assert np.array_equal(c["ids"][:, :3], np.tile(ar.CAT_DUP, (len(c["ids"]), 1)))
        assert np.all(c["score"][:, 0] == c["score"][:, 2])


@pytest.mark.parametrize("keep", [1.0, 0.5])
def test_det_orders_match_a_float64_sum(keep):
    d = dn.noatt_known()
    B, k = len(d["X"]), d["k"]
    mask = dref.binary(SEED, dref.SITE_AFM_VEC, B, k, keep) if keep < 1 else None
    ref = dn.step_ref(d["X"], d["y"], d["E"], d["w"], d["w0"], d["P"], mask, keep)
    loss, Gd, Mg = ar.grad64(d["X"], d["y"], d["E"], d["w"], d["w0"], d["P"], mask, keep)
    assert abs(ref["loss64"] - loss) <= 1e-12 * loss
    assert abs(F64(ref["loss"]) - loss) <= np.spacing(F32(loss))
    for n, key in zip(ar.NAMES, ("dE", "dw", "dw0", "dP")):
        before = np.asarray(d[n], F32)
        after = (before - np.asarray(ref[key], F32)).astype(F32)
        r = tr.ratio(np.asarray(ref[key], F64), before, after, Gd[n], Mg[n])
        assert r <= 1.0, (n, r)
    assert np.abs(ref["dP"]).min() > 0 and np.abs(ref["dE"][0]).min() > 0


def test_parse_args():
    from hhfm_amd import AFM
    assert AFM.parse_args("frappe", 64, 10, []).attention == 1
    a = AFM.parse_args("frappe", 64, 10, ["--attention", "0", "--keep", "[1,0.5]"])
    assert a.attention == 0 and a.keep == "[1,0.5]" and a.lamda_attention == 100.0
