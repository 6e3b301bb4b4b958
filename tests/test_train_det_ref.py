"""CPU checks of tests/train_det_ref.py: the known-answer inputs are exact in
fp32 (asserted in float64), and the FM input has teeth — another summation
order changes the bits the GPU test compares."""
import numpy as np

from tests import train_det_ref as dr

F32, F64 = np.float32, np.float64


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_ordered_sum_and_scalar_sum_orders():
    v = np.array([2.0 ** 24, 1.0, 1.0, -2.0 ** 24], F32)
    assert dr.ordered_sum(v) == 0.0                    # ((2^24 + 1) + 1) − 2^24 in fp32
    assert dr.ordered_sum(v[::-1]) == 2.0                # ((−2^24 + 1) + 1) + 2^24
    assert dr.ordered_sum(np.array([1.0, 1.0, 2.0 ** 24, -2.0 ** 24], F32)) == 2.0
    # a −0 first contribution survives (the sum starts from it, not from +0)
    assert np.signbit(dr.ordered_sum(np.array([-0.0], F32)))
    # scalar order: rows 0 and 256 meet in partial 0 before row 1 joins
    rows = np.zeros(257, F32)
    rows[0], rows[1], rows[256] = 2.0 ** 24, 1.0, -2.0 ** 24
    assert dr.scalar_sum(rows) == 1.0                  # (2^24 − 2^24) + 1
    assert dr.ordered_sum(rows) == 0.0                 # plain ascending loses the 1
    ids = np.array([3, 1, 3, 1, 3])
    c = np.array([[1.0], [2.0 ** 24], [2.0 ** 24], [1.0], [-2.0 ** 24]], F32)
    out = dr.segment_scatter(ids, c, 5)
    assert out[3, 0] == 0.0 and out[1, 0] == 2.0 ** 24 and not out[[0, 2, 4]].any()


def test_fm_known_answer_is_exact_in_fp32():
    d = dr.fm_known()
    X, y, E = d["X"], d["y"], d["E"]
    assert X.shape == (3001, 2) and E.shape == (3002, 8)
    e = E[X]                                           # [B, 2, k]
    # the forward in fp32, in the kernel's order, equals the float64 one: out = 0
    s = (e[:, 0] + e[:, 1]).astype(F32)
    q = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]).astype(F32)
    assert np.array_equal(s.astype(F64), e.astype(F64).sum(1))
    assert np.array_equal(q.astype(F64), (e.astype(F64) ** 2).sum(1))
    assert not (F32(0.5) * (s * s - q)).any()
    assert not (0.5 * (s.astype(F64) ** 2 - q.astype(F64))).any()
    # g = −y; the contributions −y·E[1 + b] are 8-bit products, exact
    assert np.array_equal(d["g"], -y)
    c64 = -y.astype(F64)[:, None] * E[1:].astype(F64)
    assert np.array_equal(d["c0"].astype(F64), c64)
    # the contribution to dE[1 + b] is g·(s − e) = ±0
    assert not (d["g"][:, None] * (s - e[:, 1])).any()
    assert not d["dE"][1:].any() and np.array_equal(d["dw"][1:], d["g"])
    # the loss: float of the float64 sum, whatever its order, to 1 ulp
    assert abs(F64(d["loss"]) - d["loss64"]) <= np.spacing(F32(d["loss64"]))


def test_fm_known_answer_has_teeth():
    """Reversed and two seeded permutations of the rows: dw[0] changes and at
    least half of dE[0]'s columns change.  (The scalar order differs from the
    plain ascending one as well.)"""
    d = dr.fm_known()
    B, k = d["c0"].shape
    orders = [np.arange(B)[::-1], np.random.default_rng(1).permutation(B),
              np.random.default_rng(2).permutation(B)]
    for p in orders:
        assert _bits(dr.ordered_sum(d["g"][p])) != _bits(d["dw"][0])
        changed = _bits(dr.ordered_sum(d["c0"][p])) != _bits(d["dE"][0])
        assert changed.sum() >= k // 2, changed
    assert _bits(dr.ordered_sum(d["g"])) != _bits(d["dw0"])


def test_hhfm_known_answer_is_exact_in_fp32():
    d = dr.hhfm_known()
    X, Neg, E = d["X"], d["Neg"], d["E"]
    B = len(X)
    assert B == 1031 and Neg.shape == (B, 1) and E.shape[1] == 8
    E64 = E.astype(F64)
    h, it, ng = E64[X[:, 0]], E64[X[:, 1]], E64[Neg[:, 0]]
    assert not (h * it).any() and not (h * ng).any()   # every product of pos / neg is 0
    assert len(np.unique(X[:, 1])) == 1                # one hot item
    # σ(0) = ½ and g = −½ exactly; the contributions are exact
    g = -0.5
    ref = np.stack([g * h, -g * h, g * it - g * ng], 1).reshape(-1, 8)
    assert np.array_equal(d["contribs"].astype(F64), ref)
    # dE[item][0:4] is the ordered sum of −½·E[u_b]; columns 4–7 of it are 0
    item = d["item"]
    want = dr.ordered_sum((F32(-0.5) * E[X[:, 0]]).astype(F32))
    assert np.array_equal(_bits(d["dE"][item]), _bits(want))
    assert d["dE"][item, :4].any() and not d["dE"][item, 4:].any()
    # users and negatives repeat: their rows are ordered sums too
    assert len(np.unique(X[:, 0])) < B and len(np.unique(Neg)) < B
