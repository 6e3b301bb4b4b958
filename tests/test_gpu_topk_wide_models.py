"""Wide K through the model classes: ``model.topk(A, 100)`` for FM, OUR (three
layouts), AFM, DeepFM and CARS2 on the weights and queries of the reference's
golden files, held to the CPU oracle's top-100 of the same catalog.

The reference only ever fetched 20, so the files hold its top-20: the first 20
entries of every wide list must be that list, position for position.  The rest
is compared with the oracle — positions array_equal; a differing position must
be an fp32 tie (confirmed in float64 by tests/helpers.topk_tie_swaps for FM,
OUR and CARS2, within 1e-5 of the query's score scale by the oracle's own
topk_swaps for AFM and DeepFM, the rule of their existing tests), at most 2 per
case.  Pooled and two-way OUR, AFM without attention and the six DeepFM heads
are held to their restatements (tests/hhfm_pool_ref.py, hhfm_two_way_ref.py,
afm0_ref.py, dfm_heads_ref.py) by the float64-confirmed rule, all seven model
cases to the reference's own top-100 (tests/golden/topk_wide.npz).  Exclusion
lists and an 8-way shard merge at K = 100 ride on the same models.
"""
import os

import numpy as np
import pytest
import torch

from oracle import fm_oracle as orc
from oracle import parity
from tests import topk_wide_ref as wr
from tests.helpers import topk_tie_swaps

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
K = 100
MAX_TIES = 2


def _load(name):
    return dict(np.load(os.path.join(G, name)))


def _fm():
    from hhfm_amd.FM import FM
    d = _load("fm.npz")
    nu, ni = int(d["n_user"]), int(d["n_item"])
    M, k = d["E"].shape
    m = FM(5, M, nu, ni, k, 0.1, 0.1, 1, "AdagradOptimizer", 0, 0)
    m.set_weights(feature_embeddings=d["E"], feature_bias=d["w"][:, None], bias=d["w0"])
    sc = orc.fm_catalog_scores(d["A"], d["E"], d["w"], nu, ni)
    return m, d, sc, parity.fm_exact(d["A"], d["E"], d["w"], nu, ctx=(2, d["A"].shape[1]))


def _hhfm(tag, **kw):
    from hhfm_amd.OurModel7 import OUR
    d = _load(f"hhfm_{tag}.npz")
    fd, td = int(d["feature_dimension"]), int(d["time_dimension"])
    nu, ni = int(d["n_user"]), int(d["n_item"])
    M, k = d["E"].shape
    m = OUR(fd, td, M, nu, ni, k, 0.1, 0.01, "AdagradOptimizer", True, td > 0, **kw)
    m.set_weights(feature_embeddings=d["E"])
    sc = orc.hhfm_catalog_scores(d["A"], d["E"], nu, ni, fd, td, True, td > 0)
    ex = parity.hhfm_exact(d["A"], d["E"], nu, ctx=(2, 2 + fd), time=(2 + fd, 2 + fd + td))
    return m, d, sc, ex


def _check(pred, d, sc, exact):
    assert pred.dtype == np.int32 and pred.shape == (len(d["A"]), K)
    assert np.array_equal(pred[:, :20], d["topk_idx"]), "the reference's own top-20 in front"
    ri = orc.top_k(sc, K)[1]
    assert np.array_equal(ri, wr.topk(sc, K)[1])            # the oracle's order is the restated one
    assert topk_tie_swaps(pred, ri, exact) <= MAX_TIES


def test_fm_topk_100():
    m, d, sc, ex = _fm()
    _check(m.topk(d["A"], K), d, sc, ex)


@pytest.mark.parametrize("tag", ["frappe", "jiaju", "resturant"])
def test_hhfm_topk_100(tag):
    m, d, sc, ex = _hhfm(tag)
    if sc.shape[1] < K:
        pytest.fail(f"hhfm_{tag}.npz holds {sc.shape[1]} items: no top-{K}")
    _check(m.topk(d["A"], K), d, sc, ex)


def _by_oracle_scores(pred, sc):
    ri = orc.top_k(sc, K)[1]
    bad, swaps = orc.topk_swaps(sc, ri, pred, 1e-5 * np.abs(sc).max(1, keepdims=True))
    assert bad == 0 and swaps <= MAX_TIES, (bad, swaps)


def test_afm_topk_100():
    from hhfm_amd.AFM import AFM
    d = _load("afm.npz")
    nu, ni = int(d["n_user"]), int(d["n_item"])
    M, k = d["E"].shape
    m = AFM(nu, ni, M, 1, [k, k], None, 0.1, 100.0, [1, 1], "AdagradOptimizer", 0.999, 5)
    m.set_weights(feature_embeddings=d["E"], feature_bias=d["w"][:, None], bias=d["w0"],
                  attention_W=d["attention_W"], attention_b=d["attention_b"],
                  attention_p=d["attention_p"], prediction=d["prediction"])
    pred = m.topk(d["A"], K)
    assert np.array_equal(pred[:, :20], d["topk_idx"])
    sc = orc.afm_catalog_scores(d["A"], d["E"], d["w"], d["attention_W"], d["attention_b"],
                                d["attention_p"], d["prediction"], nu, ni)
    _by_oracle_scores(pred, sc)
    # exclusion at K = 100: the restatement over admissible items, on the oracle's scores
    rng = np.random.default_rng(1)
    lists = [set(rng.permutation(ni)[:n].tolist()) for n in rng.integers(0, 200, len(d["A"]))]
    lists[0] = set(pred[0, :30].tolist())
    got = m.topk(d["A"], K, exclude=_lists(m, lists, nu))
    for b, s in enumerate(lists):
        assert not set(got[b].tolist()) & s
    want = wr.topk_admissible(sc, K, lists)[1]
    bad, swaps = orc.topk_swaps(sc, want, got, 1e-5 * np.abs(sc).max(1, keepdims=True))
    assert bad == 0 and swaps <= MAX_TIES


def _lists(model, lists, n_user):
    from hhfm_amd import ops
    return ops.exclusion_lists([[n_user + c for c in s] for s in lists], "cuda")


def test_dfm_topk_100():
    from hhfm_amd.DFM import DeepFM
    d = _load("dfm.npz")
    nu, ni = int(d["n_user"]), int(d["n_item"])
    M, k = d["E"].shape
    layers = [d[f"layer_{i}"] for i in range(3)]
    biases = [d[f"bias_{i}"] for i in range(3)]
    m = DeepFM(nu, ni, M, 5, k, [150, 200, 150], None, 0.01, 0, 0.01)
    m.set_weights(feature_embeddings=d["E"], feature_bias=d["w"][:, None],
                  concat_projection=d["concat_projection"], concat_bias=d["concat_bias"],
                  **{f"layer_{i}": layers[i] for i in range(3)},
                  **{f"bias_{i}": biases[i] for i in range(3)})
    pred = m.topk(d["A"], K)
    assert np.array_equal(pred[:, :20], d["topk_idx"])
    sc = orc.dfm_catalog_scores(d["A"], d["E"], d["w"], layers, biases, d["concat_projection"],
                                d["concat_bias"], nu, ni)
    _by_oracle_scores(pred, sc)
    lists = [set(pred[b, b:b + 40].tolist()) for b in range(len(d["A"]))]
    got = m.topk(d["A"], K, exclude=_lists(m, lists, nu))
    for b, s in enumerate(lists):
        assert not set(got[b].tolist()) & s
    want = wr.topk_admissible(sc, K, lists)[1]
    bad, swaps = orc.topk_swaps(sc, want, got, 1e-5 * np.abs(sc).max(1, keepdims=True))
    assert bad == 0 and swaps <= MAX_TIES


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["dense", "stream"])
def test_cars2_topk_100(name, dtype):
    from hhfm_amd import ops
    from tests import cars2_ref as cr
    from tests.test_gpu_cars2 import _dev, _prepare
    Wt, q, nu, ni = cr.catalog_case(name, dtype == "bf16")
    sc, exact = cr.catalog_reference(Wt, q, nu, ni), cr.exact_catalog(q, Wt, nu)
    UId = _dev(Wt["UI"]).to(torch.bfloat16) if dtype == "bf16" else _dev(Wt["UI"])
    args = (_dev(q), UId.contiguous(), _prepare(Wt), Wt["Context"].shape[0])
    s, i = ops.cars2_catalog_topk(*args, K, nu, ni)
    assert topk_tie_swaps(i.cpu().numpy(), cr.top_k(sc, K)[1], exact) <= cr.MAX_TIES
    n20 = ops.cars2_catalog_topk(*args, 20, nu, ni)
    assert torch.equal(i[:, :20], n20[1]) and torch.equal(s[:, :20], n20[0])
    lists = [set(i[b, :50].tolist()) for b in range(len(q))]
    got = ops.cars2_catalog_topk(*args, K, nu, ni, exclude=ops.exclusion_lists(
        [[nu + c for c in s_] for s_ in lists], "cuda"))[1].cpu().numpy()
    for b, s_ in enumerate(lists):
        assert not set(got[b].tolist()) & s_
    assert topk_tie_swaps(got, wr.topk_admissible(sc, K, lists)[1], exact) <= cr.MAX_TIES


# ---------------------------------------------------------------------------
# exclusion and shards on FM / OUR
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fm", "frappe", "jiaju"])
def test_exclusion_at_100(which):
    m, d, sc, ex = _fm() if which == "fm" else _hhfm(which)
    nu, ni = int(d["n_user"]), int(d["n_item"])
    plain = m.topk(d["A"], K)
    rng = np.random.default_rng(3)
    lists = [set(plain[b, :60].tolist()) | set(rng.permutation(ni)[:b * 7].tolist())
             for b in range(len(d["A"]))]
    got = m.topk(d["A"], K, exclude=_lists(m, lists, nu))
    for b, s in enumerate(lists):
        assert not set(got[b].tolist()) & s
    assert topk_tie_swaps(got, wr.topk_admissible(sc, K, lists)[1], ex) <= MAX_TIES
    long = [set(range(ni - K + 1))] + [set()] * (len(d["A"]) - 1)
    with pytest.raises(ValueError):               # K + max_excl > item_count
        m.topk(d["A"], K, exclude=_lists(m, long, nu))


@pytest.mark.parametrize("which", ["fm", "frappe"])
def test_eight_shards_merge_to_model_topk(which):
    from hhfm_amd import distributed as dist
    from hhfm_amd import ops
    m, d, _, _ = _fm() if which == "fm" else _hhfm(which)
    ni = int(d["n_item"])
    whole = m.topk(d["A"], K)
    q = m._idx(d["A"])
    edges = [ni * r // 8 + (r % 3) for r in range(8)] + [ni]      # ragged shards
    parts = []
    for b0, b1 in zip(edges[:-1], edges[1:]):
        s, i = m.catalog_topk(q, b0, b1 - b0, min(K, b1 - b0))
        parts.append(dist._pad(s, i, K))
    _, ids = ops.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert np.array_equal(ids.cpu().numpy(), whole)


# ---------------------------------------------------------------------------
# pooled and two-way OUR, AFM without attention, the six DeepFM heads: each held
# to its restatement at K = 100 by the same rule
# ---------------------------------------------------------------------------
def _layout(d):
    fd, td = int(d["feature_dimension"]), int(d["time_dimension"])
    return (2, 2 + fd), (2 + fd, 2 + fd + td)


@pytest.mark.parametrize("tag", ["frappe", "jiaju"])
@pytest.mark.parametrize("triple", [("max", "max", "max"), ("mean", "max", "sum")], ids="_".join)
def test_pooled_topk_100(triple, tag):
    from tests import hhfm_pool_ref as pr
    m, d, _, _ = _hhfm(tag, pooling=triple)
    nu, ni = int(d["n_user"]), int(d["n_item"])
    ctx, tim = _layout(d)
    h = pr.hybrid(d["E"], d["A"], ctx, tim, triple)
    sc = h @ d["E"][nu:nu + ni].T                       # the restated fp32 scores
    ex = pr.exact_catalog(d["A"], d["E"], nu, ctx, tim, triple)
    assert topk_tie_swaps(m.topk(d["A"], K), orc.top_k(sc, K)[1], ex) <= MAX_TIES


@pytest.mark.parametrize("tag", ["frappe", "jiaju"])
@pytest.mark.parametrize("n", [0, 3])
def test_two_way_topk_100(n, tag):
    from tests import hhfm_two_way_ref as tw
    p1, p2 = tw.SEXTUPLES[n]
    m, d, _, _ = _hhfm(tag, pooling=p1, two_way=True, pooling2=p2)
    nu, ni = int(d["n_user"]), int(d["n_item"])
    ctx, tim = _layout(d)
    h = tw.hybrid2(d["E"], d["A"], ctx, tim, p1, p2)
    sc = h @ d["E"][nu:nu + ni].T
    ex = tw.exact_catalog2(d["A"], d["E"], nu, ctx, tim, p1, p2)
    assert topk_tie_swaps(m.topk(d["A"], K), orc.top_k(sc, K)[1], ex) <= MAX_TIES


def test_afm_without_attention_topk_100():
    """AFM(attention=0) on afm.npz's table: the float64 catalog of
    tests/afm0_ref.py (out of the row with column 1 replaced by the item)."""
    from hhfm_amd.AFM import AFM
    from tests import afm0_ref as ar
    d = _load("afm.npz")
    nu, ni = int(d["n_user"]), int(d["n_item"])
    M, k = d["E"].shape
    m = AFM(nu, ni, M, 0, [k, k], None, 0.1, 100.0, [1, 1], "AdagradOptimizer", 0.999, 5)
    P = np.random.default_rng(5).normal(1.0, 0.3, (k, 1)).astype(np.float32)
    m.set_weights(feature_embeddings=d["E"], feature_bias=d["w"][:, None], bias=d["w0"],
                  prediction=P)
    score, mag, _ = ar.catalog64(d["A"], d["E"], d["w"], float(d["w0"]), P[:, 0], nu, ni)
    ref = wr.topk(score.astype(np.float32), K)[1]

    def exact(b, ids):
        ids = np.asarray(ids, np.int64)
        return score[b, ids], mag[b, ids]
    assert topk_tie_swaps(m.topk(d["A"], K), ref, exact) <= MAX_TIES


@pytest.mark.parametrize("name", ["fm_mse", "deep_mse", "both_mse", "fm_logloss", "deep_logloss",
                                  "both_logloss"])
def test_dfm_heads_topk_100(name):
    """The six heads on the reference's own weights (dfm_heads.npz): the list
    ranks by z, restated by tests/dfm_heads_ref.forward."""
    from tests import dfm_heads_ref as hr
    from tests.test_gpu_dfm_heads import _gold_model, _gold_weights
    d = _load("dfm_heads.npz")
    nu, ni = int(d["n_user"]), int(d["n_item"])
    head = hr.head_word(*hr.HEADS[name])
    m, W, A = _gold_model(d, name), _gold_weights(d, name), d[f"{name}_A"]
    rows = hr.catalog_rows(A, nu, ni)
    z32 = hr.forward(rows, *W, head)[1].reshape(len(A), ni)
    _, z64, S = hr.forward(rows, *W, head, dt=np.float64)
    z64, S = z64.reshape(len(A), ni), S.reshape(len(A), ni)

    def exact(b, ids):
        ids = np.asarray(ids, np.int64)
        return z64[b, ids], S[b, ids]
    pred = m.topk(A, K)
    assert np.array_equal(pred[:, :20], d[f"{name}_topk_idx"])      # the reference's own top-20
    assert topk_tie_swaps(pred, orc.top_k(z32, K)[1], exact) <= MAX_TIES


# ---------------------------------------------------------------------------
# the reference's own top-100 (tests/golden/topk_wide.npz)
# ---------------------------------------------------------------------------
def _fixture_model(name, c, nu, ni, d):
    """(model, queries) of one case of the fixture, weights set."""
    if name == "fm":
        from hhfm_amd.FM import FM
        M, k = c["E"].shape
        m = FM(5, M, nu, ni, k, 0.1, 0.1, 1, "AdagradOptimizer", 0, 0)
        m.set_weights(feature_embeddings=c["E"], feature_bias=c["w"][:, None])
        return m, c["A"]
    if name.startswith("hhfm"):
        from hhfm_amd.OurModel7 import OUR
        fd, td = int(c["feature_dimension"]), int(c["time_dimension"])
        M, k = c["E"].shape
        m = OUR(fd, td, M, nu, ni, k, 0.1, 0.01, "AdagradOptimizer", True, td > 0)
        m.set_weights(feature_embeddings=c["E"])
        return m, c["A"]
    if name == "afm":
        from hhfm_amd.AFM import AFM
        M, k = c["E"].shape
        m = AFM(nu, ni, M, 1, [k, k], None, 0.1, 100.0, [1, 1], "AdagradOptimizer", 0.999, 5)
        m.set_weights(feature_embeddings=c["E"], feature_bias=c["w"][:, None], bias=c["w0"],
                      attention_W=c["attention_W"], attention_b=c["attention_b"],
                      attention_p=c["attention_p"], prediction=c["prediction"])
        return m, c["A"]
    if name == "dfm":
        from hhfm_amd.DFM import DeepFM
        M, k = c["E"].shape
        dims = [int(x) for x in d["dfm_layers"]]
        m = DeepFM(nu, ni, M, 5, k, dims, None, 0.01, 0, 0.01)
        m.set_weights(feature_embeddings=c["E"], feature_bias=c["w"][:, None],
                      concat_projection=c["concat_projection"], concat_bias=c["concat_bias"],
                      **{f"layer_{i}": c[f"layer_{i}"] for i in range(len(dims))},
                      **{f"bias_{i}": c[f"bias_{i}"] for i in range(len(dims))})
        return m, c["A"]
    from tests import cars2_ref as cr
    from tests.test_gpu_cars2 import _model
    Wt = cr.weights(int(c["seed"]), nu + ni, int(d["cars2_Mc"]), 16)
    return _model(Wt, nu, ni), c["q"].astype(np.int64)


@pytest.mark.parametrize("name", ["fm", "hhfm_frappe", "hhfm_jiaju", "hhfm_resturant", "afm",
                                  "dfm", "cars2"])
def test_models_against_the_reference_top_100(name):
    from tests import test_topk_wide_golden as tg
    d = dict(np.load(tg.G))
    nu, ni = int(d["n_user"]), int(d["n_item"])
    c = tg.case(d, name)
    m, A = _fixture_model(name, c, nu, ni, d)
    pred = m.topk(A, K)
    _, ex = tg.oracle_lists(name, d, nu, ni)
    assert topk_tie_swaps(pred, c["topk_idx"].astype(np.int32), ex) <= MAX_TIES
