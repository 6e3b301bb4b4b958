"""Wide K on the device (include/hhfm.h "Wide K"): 65 <= K <= 1,024.

Selection moves bits, so the select, the merge and the designed-score catalog
cases are held to np.array_equal on ids and on the scores' bit patterns against
tests/topk_wide_ref.py; there is no tolerance.  On random tables the wide list
is held to the narrow call: its first 64 entries are the K = 64 list bit for
bit, under every plan bit that chooses arithmetic.
"""
import numpy as np
import pytest
import torch

from tests import score_designs as sd
from tests import topk_wide_ref as wr

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _same(got, want, what=""):
    gs, gi = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in got)
    ws, wi = want
    if not np.array_equal(gi, wi):
        b, p = np.argwhere(gi != wi)[0]
        raise AssertionError(f"{what}: ids differ at {int((gi != wi).sum())} positions; first "
                             f"row {b} rank {p}: got {gi[b, p]} ({gs[b, p]}), "
                             f"expected {wi[b, p]} ({ws[b, p]})")
    assert np.array_equal(_bits(gs), _bits(ws)), f"{what}: score bits differ"


# ---------------------------------------------------------------------------
# 1. dense select
# ---------------------------------------------------------------------------
KS = (65, 100, 128, 129, 256, 1000, 1024)
KINDS = ("random", "ascending", "descending", "all_equal", "plateau")


def _rows(kind, B, N, K, rng):
    if kind == "random":
        return rng.normal(size=(B, N)).astype(np.float32)
    if kind == "ascending":
        return np.tile(np.arange(N, dtype=np.float32) - 7, (B, 1))
    if kind == "descending":
        return np.tile(-np.arange(N, dtype=np.float32) / 4, (B, 1))
    if kind == "all_equal":
        return np.full((B, N), -1.5, np.float32)
    sc = rng.integers(-50, 0, size=(B, N)).astype(np.float32)      # a plateau of K + 37 best
    for b in range(B):
        sc[b, rng.permutation(N)[:min(N, K + 37)]] = 3.0
    return sc


def _guarded(sc, pad):
    """sc on the device inside a NaN frame: NaN guard rows around the matrix,
    ld = N + pad with NaN in the padding.  Returns the [B, N] view."""
    B, N = sc.shape
    full = torch.full((B + 2, N + pad), NAN, dtype=torch.float32, device="cuda")
    view = full[1:B + 1, :N]
    view.copy_(torch.from_numpy(sc))
    return view


@pytest.mark.parametrize("K", KS)
def test_dense_select_exact(K):
    from hhfm_amd import ops
    rng = np.random.default_rng(K)
    for N in sorted({K, K + 1, 1023, 1025, 4099}):
        if N < K:
            continue
        for B in (1, 5):
            for kind in KINDS:
                sc = _rows(kind, B, N, K, rng)
                # ld = N + 3: rows start off a 16-byte boundary, every alignment in turn
                got = ops.topk_dense(_guarded(sc, 3), K, global_item_base=17)
                want = wr.topk(sc, K, base=17)
                _same(got, want, f"{kind} K={K} N={N} B={B}")
                if kind == "all_equal":
                    assert np.array_equal(want[1], np.tile(17 + np.arange(K), (B, 1)))
    sc = _rows("random", 3, 4099, K, rng)                      # ld a multiple of 4, ONE_WAVE ignored
    _same(ops.topk_dense(_guarded(sc, 1), K, plan=ops.PLAN_ONE_WAVE), wr.topk(sc, K), "aligned")


@pytest.mark.parametrize("K", [65, 1024])
def test_dense_prefix_is_the_narrow_list(K):
    from hhfm_amd import ops
    rng = np.random.default_rng(7)
    for kind in ("random", "plateau"):
        sc = _guarded(_rows(kind, 5, 4099, K, rng), 3)
        ws, wi = ops.topk_dense(sc, K)
        ns, ni = ops.topk_dense(sc, 64)
        assert torch.equal(wi[:, :64], ni)
        assert torch.equal(ws[:, :64].view(torch.int32), ns.view(torch.int32))


@pytest.mark.parametrize("K", [65, 100, 1024])
def test_signed_zeros_tie_by_index(K):
    """+0 and -0 are equal scores: a row that mixes them at the top (or at the
    K-th rank) orders them by index alone, as the narrow kernels' pair compare
    does, and every entry comes out with its own sign bit."""
    from hhfm_amd import ops
    rng = np.random.default_rng(K)
    B, N = 5, 4099
    sc = -np.abs(rng.normal(size=(B, N))).astype(np.float32) - 1
    for b in range(B):
        z = rng.permutation(N)[:K + 37 if b % 2 else K // 2]      # the zeros straddle / stay inside K
        sc[b, z] = np.where(rng.integers(0, 2, len(z)) == 1, np.float32(-0.0), np.float32(0.0))
    dev = _guarded(sc, 3)
    ws, wi = ops.topk_dense(dev, K)
    _same((ws, wi), wr.topk(sc, K), f"K={K}")
    assert np.signbit(ws.cpu().numpy()[:, :K // 2]).any() and not np.signbit(
        ws.cpu().numpy()[:, :K // 2]).all()
    ns, ni = ops.topk_dense(dev, 64)
    assert torch.equal(wi[:, :64], ni)
    assert torch.equal(ws[:, :64].view(torch.int32), ns.view(torch.int32))
    # and through the merge: two halves of the columns, merged
    halves = [ops.topk_dense(dev[:, :2048], K), ops.topk_dense(dev[:, 2048:], K, 2048)]
    ms, mi = ops.topk_merge(torch.stack([h[0] for h in halves]), torch.stack([h[1] for h in halves]))
    assert torch.equal(mi, wi) and torch.equal(ms.view(torch.int32), ws.view(torch.int32))


def test_dense_excl_wide():
    """hhfm_topk_dense_excl at wide K: the matrix is only read."""
    from hhfm_amd import ops
    rng = np.random.default_rng(8)
    B, N, irb = 5, 4099, 40
    sc = _rows("plateau", B, N, 100, rng)
    lists = [set(rng.permutation(N)[:n].tolist()) for n in (0, 1, 700, 3000, 64)]
    lists[1] = {int(np.argmax(sc[1]))}
    ex = ops.exclusion_lists([[irb + c for c in s] + [3, irb + N + 5] for s in lists], "cuda")
    dev = _guarded(sc, 3)
    before = dev.clone()
    for K in (100, 1024):
        got = ops.topk_dense(dev, K, 9, exclude=ex, item_row_begin=irb)
        _same(got, wr.topk_admissible(sc, K, lists, base=9), f"K={K}")
    assert torch.equal(dev, before)
    long = ops.exclusion_lists([[irb + c for c in range(3200)]] + [[]] * (B - 1), "cuda")
    with pytest.raises(ValueError):
        ops.topk_dense(dev, 1000, exclude=long, item_row_begin=irb)        # K + max_excl > N


# ---------------------------------------------------------------------------
# 3. merge
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [65, 128, 1000, 1024])
@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_merge_equals_host_merge(K, R):
    from hhfm_amd import ops
    from tests.test_topk_wide_ref import sharded_lists
    rng = np.random.default_rng(1000 * R + K)
    for B in (1, 5):
        for pad in (None, K // 3, 0):
            sc, ids = sharded_lists(rng, R, B, K, pad_from=pad)
            hs, hi = ops.topk_merge(torch.from_numpy(sc), torch.from_numpy(ids))
            ds, di = ops.topk_merge(torch.from_numpy(sc).cuda(), torch.from_numpy(ids).cuda())
            _same((ds, di), (hs.numpy(), hi.numpy()), f"R={R} K={K} B={B} pad={pad}")
            _same((ds, di), wr.merge(sc, ids), "restatement")


# ---------------------------------------------------------------------------
# 4. catalog, designed scores
# ---------------------------------------------------------------------------
SIZES = (300, 4082, 16385, 49153, 70000)
PLANTED = ((0, 12), (16383, 9), (16384, 9), (32767, 11), (32768, 10), (-1, 13))


class _Planted:
    """tests/score_designs.py's all_equal design (v = 1) with the best items
    planted on both sides of the 16,384-item block edges, at the first and the
    last column; 16,383 and 16,384 tie across the first edge."""

    def __init__(self, N, k, dtype, mode, B=33):
        d = sd.make("all_equal", N, k, dtype, mode, B=B)
        E = d.E.copy()
        for c, v in PLANTED:
            c = N - 1 if c < 0 else c
            if c < N:
                E[d.item_begin + c, c % (k - 2)] = v
        self.d, self.mode, self.N = d, mode, N
        self.scores = sd.expected_scores(d.A, E, d.w, d.item_begin, N, d.ctx, mode)
        self.A = torch.from_numpy(d.A).cuda()
        Ed = torch.from_numpy(E).cuda()
        self.E = Ed.to(torch.bfloat16) if dtype == "bf16" else Ed
        self.w = None if d.w is None else torch.from_numpy(d.w).cuda()

    def run(self, B, K, plan=0, lo=0, cnt=None, gbase=0, exclude=None):
        from hhfm_amd import ops
        d = self.d
        return ops.catalog_topk(self.A[:B].contiguous(), self.E,
                                ops.MODE_FM if self.mode == "fm" else ops.MODE_HHFM, K,
                                d.item_begin + lo, self.N - lo if cnt is None else cnt, gbase,
                                self.w, 0, d.ctx, (0, 0), plan=plan, exclude=exclude)


@pytest.mark.parametrize("mode", ["hhfm", "fm"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("N", SIZES)
def test_catalog_designed_scores(N, dtype, mode):
    t = _Planted(N, 16, dtype, mode)
    for K in (100, 1024):
        if K > N:
            continue
        want = wr.topk(t.scores, K)
        if N > wr.BLOCK_ITEMS:       # the blocked route restated: the same list
            blk = wr.blockwise(t.scores[:3], K)
            assert np.array_equal(blk[1], want[1][:3]) and np.array_equal(blk[0], want[0][:3])
        for B in (3, 33):
            _same(t.run(B, K), (want[0][:B], want[1][:B]), f"N={N} K={K} B={B}")
    # users 0, 1, 2 rank the planted items first, last, and not at all (a = 3, -2, 0)
    ids = wr.topk(t.scores[:3], 100)[1]
    assert ids[0, 0] == N - 1 and ids[0, 1] == 0
    if N > 32768:
        assert ids[0, 2:6].tolist() == [32767, 32768, 16383, 16384]
    assert ids[2].tolist() == list(range(100))


# ---------------------------------------------------------------------------
# 5. catalog prefix on random tables
# ---------------------------------------------------------------------------
class _Random:
    def __init__(self, N, k, dtype, seed=0, n_user=50, extra=40):
        rng = np.random.default_rng(seed + N)
        self.nu, self.N = n_user, N
        M = extra + n_user + N + 9                      # `extra` rows in front: a nonzero begin
        self.begin = extra + n_user
        E = torch.from_numpy(rng.normal(0, 0.1, (M, k)).astype(np.float32)).cuda()
        self.E = E.to(torch.bfloat16) if dtype == "bf16" else E
        self.w = torch.from_numpy(rng.normal(0, 0.1, M).astype(np.float32)).cuda()
        c0 = self.begin + N
        q = np.stack([extra + rng.integers(0, n_user, 33), np.full(33, self.begin),
                      c0 + rng.integers(0, 5, 33), c0 + 5 + rng.integers(0, 4, 33)], 1)
        self.q = torch.from_numpy(q.astype(np.int32)).cuda()

    def run(self, mode, B, K, plan=0, lo=0, cnt=None, gbase=0, exclude=None):
        from hhfm_amd import ops
        fm = mode == "fm"
        return ops.catalog_topk(self.q[:B].contiguous(), self.E,
                                ops.MODE_FM if fm else ops.MODE_HHFM, K, self.begin + lo,
                                self.N - lo if cnt is None else cnt, gbase,
                                self.w if fm else None, 0, (2, 4), (0, 0), plan=plan,
                                exclude=exclude)


def _plans(N):
    from hhfm_amd import ops
    p = {"default": 0, "exact": ops.PLAN_EXACT_FP32}
    if N <= 16384:                   # the narrow call takes the GEMM on the dense route only
        p["gemm"] = ops.PLAN_GEMM
        p["gemm+exact"] = ops.PLAN_GEMM | ops.PLAN_EXACT_FP32
    return p


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("N", SIZES)
def test_catalog_prefix_is_the_narrow_list(N, dtype):
    t = _Random(N, 16, dtype)
    for mode in ("hhfm", "fm"):
        for pname, plan in _plans(N).items():
            for B in (3, 33):
                for lo, gbase in ((0, 0), (37, 1000)):
                    ns, ni = t.run(mode, B, 64, plan, lo, None, gbase)
                    for K in (100, 1024):
                        if K > N - lo:
                            continue
                        s, i = t.run(mode, B, K, plan, lo, None, gbase)
                        what = f"{mode} {pname} B={B} K={K} lo={lo}"
                        assert torch.equal(i[:, :64], ni), what
                        assert torch.equal(s[:, :64].view(torch.int32), ns.view(torch.int32)), what
                        sn, idn = s.cpu().numpy(), i.cpu().numpy().astype(np.int64)
                        # the rest of the list: the same strict order, ids of the range
                        assert np.all((sn[:, 1:] < sn[:, :-1]) |
                                      ((sn[:, 1:] == sn[:, :-1]) & (idn[:, 1:] > idn[:, :-1]))), what
                        assert idn.min() >= gbase and idn.max() < gbase + N - lo, what


def test_many_queries_take_smaller_blocks():
    """5,000 queries x 16,000 items pass the dense route's matrix size, so the
    catalog, although below 16,384 items, goes in two blocks of fewer items."""
    from hhfm_amd import ops
    rng = np.random.default_rng(11)
    B, N, k, nu = 5000, 16000, 16, 50
    E = torch.from_numpy(rng.normal(0, 0.1, (nu + N + 9, k)).astype(np.float32)).cuda()
    q = np.stack([rng.integers(0, nu, B), np.full(B, nu), nu + N + rng.integers(0, 5, B),
                  nu + N + 5 + rng.integers(0, 4, B)], 1).astype(np.int32)
    q = torch.from_numpy(q).cuda()
    run = lambda K: ops.catalog_topk(q, E, ops.MODE_HHFM, K, nu, N, 0, None, 0, (2, 4), (0, 0))
    (ns, ni), (s, i) = run(64), run(100)
    assert torch.equal(i[:, :64], ni)
    assert torch.equal(s[:, :64].view(torch.int32), ns.view(torch.int32))
    # the whole list against the score matrix in float64 order (ties confirmed there)
    Ec = E.cpu().numpy().astype(np.float64)
    qc = q.cpu().numpy()[::250]
    h = Ec[qc[:, 0]] + Ec[qc[:, 2]] + Ec[qc[:, 3]]
    sc = h @ Ec[nu:nu + N].T
    ref = wr.topk(sc.astype(np.float32), 100)[1]
    got = i.cpu().numpy()[::250]
    for b, p in np.argwhere(got != ref):
        assert abs(sc[b, got[b, p]] - sc[b, ref[b, p]]) <= 1e-5 * np.abs(sc[b]).max()
    assert (got != ref).sum() <= 2


def test_selection_plan_bits_change_nothing():
    from hhfm_amd import ops
    t = _Random(16385, 16, "f32")
    ref = t.run("hhfm", 3, 100)
    for bit in (ops.PLAN_NO_SEED, ops.PLAN_NO_RING, ops.PLAN_RING_ALT, ops.PLAN_FUSED,
                ops.PLAN_STORE, ops.PLAN_ONE_WAVE):
        got = t.run("hhfm", 3, 100, bit)
        assert torch.equal(got[1], ref[1]) and torch.equal(got[0], ref[0])


# ---------------------------------------------------------------------------
# 7. exclusion (FM / HHFM here; the other models below)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4082, 49153])
def test_catalog_exclusion_designed(N):
    from hhfm_amd import ops
    t = _Planted(N, 16, "f32", "hhfm")
    B, K, begin = 5, 100, t.d.item_begin
    rng = np.random.default_rng(N)
    lists = [{N - 1, 0}, set(), set(rng.permutation(N)[:900].tolist()),
             {16383 % N, 16384 % N, 32767 % N}, set(range(0, 300))]
    ex = ops.exclusion_lists([[begin + c for c in s] for s in lists], "cuda")
    got = t.run(B, K, exclude=ex)
    want = wr.topk_admissible(t.scores[:B], K, lists)
    _same(got, want, f"N={N}")
    gi = got[1].cpu().numpy()
    for b, s in enumerate(lists):
        assert not set(gi[b].tolist()) & s
    long = ops.exclusion_lists([[begin + c for c in range(N - 50)]] + [[]] * (B - 1), "cuda")
    with pytest.raises(ValueError):          # K + max_excl > item_count
        t.run(B, K, exclude=long)


# ---------------------------------------------------------------------------
# 8. workspace
# ---------------------------------------------------------------------------
def _raw(nat, t, B, K, N, ws, plan=0):
    from hhfm_amd import ops
    s = torch.empty(B, K, dtype=torch.float32, device="cuda")
    i = torch.empty(B, K, dtype=torch.int32, device="cuda")
    q = t.q[:B].contiguous()
    M, k = t.E.shape
    nat.catalog_topk(q.data_ptr(), B, 4, ops.MODE_HHFM, 0, 2, 4, 0, 0, t.E.data_ptr(), M, k,
                     1 if t.E.dtype == torch.bfloat16 else 0, 0, t.begin, N, 0, K, s.data_ptr(),
                     i.data_ptr(), ws.data_ptr(), ws.numel(), plan, 0,
                     torch.cuda.current_stream().cuda_stream)
    return s, i


def test_workspace_contract_wide():
    from hhfm_amd._native import native
    nat = native()
    Z = nat.CATALOG_WS_ZERO
    t = _Random(49153, 16, "f32")
    B = 33
    calls = [(20, 49153), (100, 4082), (1024, 49153), (64, 16385), (100, 300)]
    need = max(nat.catalog_topk_wide_workspace(B, N, 16, K) for K, N in calls)
    alone = {}
    for K, N in calls:                         # each on a zero buffer of its own
        ws = torch.zeros(nat.catalog_topk_wide_workspace(B, N, 16, K), dtype=torch.uint8,
                         device="cuda")
        alone[(K, N)] = _raw(nat, t, B, K, N, ws)
        assert int(ws[:Z].max()) == 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")     # poisoned beyond the prefix
    ws[:Z] = 0
    for K, N in calls:                         # narrow, wide dense, wide blocked, narrow, wide dense
        s, i = _raw(nat, t, B, K, N, ws)
        assert torch.equal(i, alone[(K, N)][1]), (K, N)
        assert torch.equal(s.view(torch.int32), alone[(K, N)][0].view(torch.int32)), (K, N)
        assert int(ws[:Z].max()) == 0, (K, N)
    short = torch.zeros(nat.catalog_topk_wide_workspace(B, 49153, 16, 100) - 1, dtype=torch.uint8,
                        device="cuda")
    with pytest.raises(Exception):
        _raw(nat, t, B, 100, 49153, short)
