"""Catalog top-K with exclusion lists (include/hhfm.h "Exclusion lists") on the
device, held to two tolerance-free yardsticks:

* designed scores (tests/score_designs.py): the expected ids and score bits of
  the filtered list are exact (tests/topk_excl_ref.filtered_topk over the
  design's scores);
* the over-fetch identity against the existing entry points on random tables:
  the first K of (the plain call's top-64 minus the list) is the filtered
  top-K whenever at most 64 - K of a query's excluded items lie in its plain
  top-64 — which every test asserts for every query.

Every comparison is np.array_equal on int32 ids and on the float32 scores
viewed as int32.  Routes: the score matrix (STORE or the GEMM) with masked
entries, catalog_main's exclusion form without a seed, and behind a seed whose
tiles with excluded rows are taken out.
"""
import os

import numpy as np
import pytest
import torch

from tests import guard_tables as gt
from tests import score_designs as sd
from tests import topk_excl_ref as xr

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
BMAX = 130
KF = 64      # factors
POOL = ("max", "sum", "mean")


def _dev():
    return torch.device("cuda", 0)


def _same(got, want, what=""):
    gs, gi = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in got)
    ws, wi = want
    if not np.array_equal(gi, wi):
        b, p = np.argwhere(gi != wi)[0]
        raise AssertionError(f"{what}: ids differ at {int((gi != wi).sum())} positions; first "
                             f"query {b} rank {p}: got {gi[b, p]} ({gs[b, p]}), "
                             f"expected {wi[b, p]} ({ws[b, p]})")
    assert np.array_equal(sd.bits(gs), sd.bits(ws)), f"{what}: score bits differ"


# ---------------------------------------------------------------------------
# designed scores
# ---------------------------------------------------------------------------
_DESIGNS = {}


class _Design:
    def __init__(self, design, N, dtype, mode, K):
        self.d = d = sd.make(design, N, KF, dtype, mode, B=BMAX, K=K)
        self.mode = mode
        self.A = torch.from_numpy(d.A).cuda()
        E = torch.from_numpy(d.E).cuda()
        self.E = E.to(torch.bfloat16) if dtype == "bf16" else E
        self.w = None if d.w is None else torch.from_numpy(d.w).cuda()

    def lists(self, B, e, extra=None):
        """The designed top e items of the a = 3 queries for every query (the
        worst items of the a = -2 ones); the all-equal a = 0 queries also lose
        items 0, 2 and 5, so their answer is the lowest ids that are left."""
        d = self.d
        b3 = int(np.flatnonzero(d.A[:, 0] % 3 == 0)[0])
        top = np.argsort(-d.scores[b3], kind="stable")[:e] + d.item_begin
        out = []
        for b in range(B):
            rows = list(top)
            if d.A[b, 0] % 3 == 2:
                rows += [d.item_begin + i for i in (0, 2, 5)]
            if extra is not None:
                rows += list(extra(b))
            out.append(np.unique(np.asarray(rows, np.int64)))
        return out

    def run(self, B, K, plan, lists, lo=0, cnt=None, gbase=0, pooling=None):
        from hhfm_amd import ops
        d = self.d
        return ops.catalog_topk(self.A[:B].contiguous(), self.E,
                                ops.MODE_FM if self.mode == "fm" else ops.MODE_HHFM, K,
                                d.item_begin + lo, d.N - lo if cnt is None else cnt, gbase,
                                self.w, 0, d.ctx, (0, 0), plan=plan, pooling=pooling,
                                exclude=ops.exclusion_lists(lists, _dev()))

    def check(self, B, K, plan, lists, what=""):
        d = self.d
        want = xr.filtered_topk(d.scores[:B], K, lists, d.item_begin)
        _same(self.run(B, K, plan, lists), want, what)
        return want


def _design(design, N, dtype, mode, K=20):
    key = (design, N, dtype, mode, K if design == "plateau_spikes" else 0)
    if key not in _DESIGNS:
        _DESIGNS.clear()
        _DESIGNS[key] = _Design(design, N, dtype, mode, K)
    return _DESIGNS[key]


def _plan(name):
    from hhfm_amd import ops
    return {"default": 0, "gemm": ops.PLAN_GEMM, "exact": ops.PLAN_EXACT_FP32,
            "no_seed": ops.PLAN_NO_SEED, "one_wave": ops.PLAN_ONE_WAVE,
            # accepted without effect
            "fused": ops.PLAN_FUSED, "ring_alt": ops.PLAN_RING_ALT}[name]


def test_dense_exactly_k_items_left():
    """N = 33, K = 20 and 13 excluded items: K + max_excl = N, every query's
    list is all that is left, in order."""
    for dtype, mode in (("f32", "fm"), ("bf16", "hhfm")):
        t = _design("ascending", 33, dtype, mode)
        lists = t.lists(33, 13)
        lists = [x[:13] if len(x) > 13 else x for x in lists]
        assert max(len(x) for x in lists) == 13
        for plan in ("default", "gemm"):
            want = t.check(33, 20, _plan(plan), lists, f"{dtype} {mode} {plan}")
            full = [b for b, x in enumerate(lists) if len(x) == 13]
            assert all(len(set(want[1][b])) == 20 for b in full)


_TABLES = (("f32", "fm"), ("f32", "hhfm"), ("bf16", "fm"), ("bf16", "hhfm"))


def _dense_cases():
    """Every (route, design, e, table) cell: STORE and the GEMM x both designs
    x e in {1, K, 200} x the four (dtype, model) tables; B in {1, 33, 129}
    rotates through the cells and meets every route, design, e and table."""
    out = []
    for pi, plan in enumerate(("default", "gemm")):
        for di, design in enumerate(("ascending", "plateau_spikes")):
            for ei, e in enumerate((1, 20, 200)):
                for ti, (dtype, mode) in enumerate(_TABLES):
                    B = (1, 33, 129)[(pi + di + ei + ti) % 3]
                    out.append((design, dtype, mode, B, plan, e))
    return sorted(out, key=lambda c: (c[0], c[1], c[2]))      # cases that share tables side by side


@pytest.mark.parametrize("design,dtype,mode,B,plan,e", _dense_cases())
def test_dense_designed(design, dtype, mode, B, plan, e):
    """N = 4,082: the score matrix from STORE or the GEMM, masked, then the
    dense top-K (four waves per query at these sizes; one wave once)."""
    t = _design(design, 4082, dtype, mode)
    t.check(B, 20, _plan(plan), t.lists(B, e))
    if B == 33 and e == 20:
        t.check(B, 64, _plan(plan) | _plan("one_wave"), t.lists(B, e), "K=64 one wave")
        t.check(B, 20, _plan(plan) | _plan("fused"), t.lists(B, e), "PLAN_FUSED has no effect")


def _stream_cases():
    """Every (design, N, K, e) cell: both designs x N in {20,000, 20,011} x K in
    {20, 64} x e in {1, K, 200}; the four (dtype, model) tables rotate through
    the cells and meet every design, N, K and e.  HHFM_PLAN_EXACT_FP32 once
    per design."""
    out = []
    for di, design in enumerate(("ascending", "plateau_spikes")):
        for ni, N in enumerate((20000, 20011)):
            for ki, K in enumerate((20, 64)):
                for ei, e in enumerate((1, K, 200)):
                    dtype, mode = _TABLES[(di + 2 * ni + ki + ei) % 4]
                    out.append((design, N, dtype, mode, K, e, "default"))
    out.append(("ascending", 20011, "f32", "hhfm", 20, 20, "exact"))
    out.append(("plateau_spikes", 20011, "f32", "fm", 64, 64, "exact"))
    return sorted(out, key=lambda c: (c[0], c[1], c[2], c[3], c[4]))


@pytest.mark.parametrize("design,N,dtype,mode,K,e,plan", _stream_cases())
def test_streaming_unseeded_designed(design, N, dtype, mode, K, e, plan):
    """N = 20,000 / 20,011 (partial last tile), 130 queries: 39 splits of 17
    tiles, catalog_main's exclusion form from -inf, then the merge."""
    t = _design(design, N, dtype, mode, K)
    t.check(130, K, _plan(plan), t.lists(130, e))


@pytest.mark.parametrize("dtype,mode", [("f32", "hhfm"), ("bf16", "fm")])
def test_streaming_list_empties_a_split(dtype, mode):
    """Every second query excludes all 544 items of one split (and the last,
    partial one): that split's list stays empty and the merge skips it."""
    N, K = 20011, 20
    t = _design("ascending", N, dtype, mode)
    sp = sd.split_items(N, 130)
    assert sp == 544
    last = (N - 1) // sp

    def extra(b):
        if b % 2:
            return []
        s = last if b % 4 == 0 else 3
        return range(t.d.item_begin + s * sp, t.d.item_begin + min((s + 1) * sp, N))

    lists = t.lists(130, 1, extra)
    assert max(len(x) for x in lists) >= sp
    t.check(130, K, 0, lists)


@pytest.mark.parametrize("design,dtype,mode,e", [
    ("ascending", "f32", "hhfm", 1), ("ascending", "bf16", "hhfm", 20),
    ("ascending", "bf16", "fm", 200), ("plateau_spikes", "f32", "fm", 1),
    ("plateau_spikes", "bf16", "hhfm", 20), ("plateau_spikes", "f32", "fm", 200)])
def test_streaming_seeded_designed(design, dtype, mode, e):
    """N = 65,536: catalog_main's exclusion form behind the patched seed, the
    same lists without a seed, and PLAN_RING_ALT without effect."""
    t = _design(design, 65536, dtype, mode)
    lists = t.lists(32, e)
    want = t.check(32, 20, 0, lists, "seeded")
    _same(t.run(32, 20, _plan("no_seed"), lists), want, "no seed")
    _same(t.run(32, 20, _plan("ring_alt"), lists), want, "ring_alt")


# ---------------------------------------------------------------------------
# random tables: the over-fetch identity
# ---------------------------------------------------------------------------
class _Random:
    """Random Frappe-like table: 7 users, N items, 3 + 2 context values; the
    first `boost` items' rows scaled by 3 (their scores lead every query with
    a positive maximum there)."""

    def __init__(self, N, dtype, mode, B, seed, boost=0):
        rng = np.random.default_rng(seed)
        self.n_user, self.N, self.mode = 7, N, mode
        M = 7 + N + 5
        E = rng.normal(0, 0.1, (M, KF)).astype(np.float32)
        if boost:
            E[7:7 + boost] *= 3
        self.A = torch.from_numpy(np.stack(
            [rng.integers(0, 7, B), np.full(B, 7), 7 + N + rng.integers(0, 3, B),
             7 + N + 3 + rng.integers(0, 2, B)], 1).astype(np.int32)).cuda()
        E = torch.from_numpy(E).cuda()
        self.Ef = E
        self.E = E.to(torch.bfloat16) if dtype == "bf16" else E
        self.w = torch.from_numpy(rng.normal(0, 0.1, M).astype(np.float32)).cuda() \
            if mode == "fm" else None
        self.M, self.B = M, B
        self.rng = rng

    def call(self, K, plan=0, exclude=None, lo=0, cnt=None, gbase=0, pooling=None):
        from hhfm_amd import ops
        return ops.catalog_topk(self.A, self.E, ops.MODE_FM if self.mode == "fm" else ops.MODE_HHFM,
                                K, self.n_user + lo, self.N - lo if cnt is None else cnt, gbase,
                                self.w, 0, (2, 4), (0, 0), plan=plan, pooling=pooling,
                                exclude=exclude)


def _overfetch(t, K, plan, pooling=None, own=15, low=50, own_from=40):
    """Lists of `own` of each query's plain top-`own_from` plus `low` random
    items outside its plain top-64; -> (lists, expected) with the condition
    asserted for every query."""
    s64, i64 = (x.cpu().numpy() for x in t.call(64, plan, pooling=pooling))
    lists, ws, wi = [], [], []
    for b in range(t.B):
        mine = t.rng.choice(i64[b, :own_from], size=own, replace=False)
        rest = np.setdiff1d(np.arange(t.N), i64[b])
        other = t.rng.choice(rest, size=low, replace=False)
        lst = np.unique(np.concatenate([mine, other])) + t.n_user
        inside = np.isin(i64[b] + t.n_user, lst)
        assert inside.sum() <= 64 - K
        lists.append(lst)
        ws.append(s64[b][~inside][:K])
        wi.append(i64[b][~inside][:K])
    return lists, (np.stack(ws), np.stack(wi))


@pytest.mark.parametrize("route,N,B,plan", [
    ("dense", 4082, 33, "default"), ("dense_gemm", 4082, 33, "gemm"),
    ("stream", 20011, 130, "default"), ("seeded", 65536, 32, "default")])
@pytest.mark.parametrize("dtype,mode,pooling", [
    ("f32", "fm", None), ("bf16", "fm", None), ("f32", "hhfm", None), ("bf16", "hhfm", None),
    ("f32", "hhfm", POOL)])
def test_overfetch_identity(route, N, B, plan, dtype, mode, pooling):
    """The plain call runs under the same plan flags, so PLAN_GEMM's score
    matrix (the GEMM's own accumulation order) is compared with itself."""
    from hhfm_amd import ops
    t = _Random(N, dtype, mode, B, seed=N + B)
    K = 20
    lists, want = _overfetch(t, K, _plan(plan), pooling)
    got = t.call(K, _plan(plan), ops.exclusion_lists(lists, _dev()), pooling=pooling)
    _same(got, want, route)


def test_seed_tiles_with_excluded_rows_leave_the_seed():
    """N = 65,536, 32 queries, K = 20: every query's best 30 items lie in the
    first 4,096 (the seed's) and are excluded.  The K-th largest of the
    unpatched seed's tile maxima then lies above the filtered K-th score, so a
    filter at insertion alone returns short lists; with the tiles taken out of
    the seed the lists are the over-fetch's, and equal the unseeded call's."""
    from hhfm_amd import ops
    N, B, K, seed_n = 65536, 32, 20, 4096
    assert sd.seed_items(N) == seed_n
    for dtype, mode in (("f32", "hhfm"), ("bf16", "fm")):
        t = _Random(N, dtype, mode, B, seed=77, boost=seed_n)
        s64, i64 = (x.cpu().numpy() for x in t.call(64))
        assert (i64[:, :50] < seed_n).all()
        lists = [np.sort(i64[b, :30]) + t.n_user for b in range(B)]
        want = (s64[:, 30:30 + K], i64[:, 30:30 + K])
        # the unpatched threshold: K-th largest tile maximum of the seed.  The
        # best 30 items lie in >= K distinct tiles for the test to bite
        for b in range(B):
            tiles = np.unique(i64[b, :30] // 32)
            assert len(tiles) >= K
            kth_tile_max = np.sort([s64[b, :30][i64[b, :30] // 32 == x].max() for x in tiles])[-K]
            assert kth_tile_max > want[0][b, K - 1]
        x = ops.exclusion_lists(lists, _dev())
        got = t.call(K, 0, x)
        assert (got[1].cpu().numpy() != 0x7fffffff).all(), "short lists: seed not patched"
        _same(got, want, "seeded")
        _same(t.call(K, ops.PLAN_NO_SEED, x), want, "no seed")


def test_empty_lists_equal_the_plain_call():
    """Bit-equal to the plain call as such (plan 0: the fused kernel at N =
    4,082, the ring at N = 65,536) and to the plain call on the lists' route."""
    from hhfm_amd import ops
    for N, B, K in ((4082, 33, 20), (20011, 130, 64), (65536, 32, 20)):
        for dtype, mode, pooling in (("f32", "fm", None), ("bf16", "hhfm", POOL)):
            t = _Random(N, dtype, mode, B, seed=N)
            # the plain call on the route the lists take
            plan = ops.PLAN_STORE if N == 4082 else ops.PLAN_NO_RING
            plain = [x.cpu().numpy() for x in t.call(K, plan, pooling=pooling or (0, 0, 0))]
            empty = ops.exclusion_lists([[]] * B, _dev())
            assert empty.max_len == 0 and empty.rows.numel() == 0
            _same(t.call(K, 0, empty, pooling=pooling), plain, f"N={N} {dtype}")
            default = [x.cpu().numpy() for x in t.call(K, 0, pooling=pooling or (0, 0, 0))]
            _same(t.call(K, 0, empty, pooling=pooling), default, f"N={N} {dtype} default plan")
            # lists that hold nothing of the range
            outside = ops.exclusion_lists([[-5, 0, 3, t.n_user + N, t.M + 2]] * B, _dev())
            _same(t.call(K, 0, outside, pooling=pooling), plain, f"N={N} {dtype} outside")


@pytest.mark.parametrize("N,B", [(4082, 33), (20011, 130), (65536 + 20011, 32)])
def test_two_shards_merge_to_the_single_call(N, B):
    """The same lists (table rows: shard-independent) passed to both item
    shards; ops.topk_merge of the two equals the single call."""
    from hhfm_amd import ops
    K = 20
    t = _Random(N, "bf16", "fm", B, seed=B)
    lists, want = _overfetch(t, K, 0)
    x = ops.exclusion_lists(lists, _dev())
    single = [v.cpu().numpy() for v in t.call(K, 0, x, gbase=1000)]
    assert np.array_equal(single[1], want[1] + 1000)
    cut = N - 20011 if N > 65536 else N // 2 + 5
    a = t.call(K, 0, x, 0, cut, 1000)
    b = t.call(K, 0, x, cut, N - cut, 1000 + cut)
    _same(ops.topk_merge(torch.stack([a[0], b[0]]), torch.stack([a[1], b[1]])), single)


# ---------------------------------------------------------------------------
# guard bands: out-of-range rows and bad ids in the lists
# ---------------------------------------------------------------------------
def _raw_call(nat, t, K, ws, top_s, top_i, ptr, rows, max_excl, plan=0, pooling=0, mode=None,
              B=None, E=None, w=None, cnt=None):
    from hhfm_amd import ops
    E = t.E if E is None else E
    w = t.w if w is None else w
    mode = (ops.MODE_FM if t.mode == "fm" else ops.MODE_HHFM) if mode is None else mode
    B = t.B if B is None else B
    nat.catalog_topk_excl(t.A.data_ptr(), B, 4, mode, 0, 2, 4, 0, 0, E.data_ptr(), t.M, KF,
                          1 if E.dtype == torch.bfloat16 else 0,
                          0 if w is None else w.data_ptr(), t.n_user, t.N if cnt is None else cnt,
                          0, K, top_s.data_ptr(), top_i.data_ptr(), ws.data_ptr(), ws.numel(),
                          plan, pooling, 0, torch.cuda.current_stream().cuda_stream,
                          0 if ptr is None else ptr.data_ptr(),
                          0 if rows is None else rows.data_ptr(), max_excl)


@pytest.mark.parametrize("N,B,plan", [(4082, 33, "default"), (4082, 129, "gemm"),
                                      (20011, 130, "default"), (65536, 32, "default")])
@pytest.mark.parametrize("dtype,mode", [("f32", "fm"), ("bf16", "hhfm")])
def test_lists_with_out_of_range_rows_and_bad_ids(N, B, plan, dtype, mode):
    """Lists that straddle both ends of the item range and hold user rows,
    context rows, ids < 0 and ids >= M: those entries are ignored (compared,
    never used as an index).  The table, w and the workspace lie between guard
    bands that stay untouched (on the dense route the masked score matrix is
    the workspace's last region, on the seeded one the seed's tile maxima lie
    before its two small top-K lists); a write that strays inside the
    workspace — another query's row, H, cst, the hints — shows in the result,
    which is compared bit for bit with the over-fetch's."""
    from hhfm_amd import ops
    from hhfm_amd._native import native
    nat = native()
    K = 20
    t = _Random(N, dtype, mode, B, seed=3 * N + B)
    lists, want = _overfetch(t, K, _plan(plan), own=10, low=20)
    bad = np.concatenate([gt.near_miss_ids(t.M), [-2 ** 31, 2 ** 31 - 1],
                          np.arange(0, t.n_user), np.arange(t.n_user + N, t.M),
                          [t.n_user, t.n_user + N - 1]])
    for b in range(B):
        keep = bad if b % 3 else bad[:-2]          # some queries lose the range's two end items
        lists[b] = np.unique(np.concatenate([lists[b], keep]))
    want = _overfetch_apply(t, K, _plan(plan), lists)
    g = gt.Guards()
    E = g.table(t.E)
    w = None if t.w is None else g.table(t.w)
    ptr, rows, longest = xr.csr(lists)
    rows_d = torch.from_numpy(rows).cuda()
    ptr_d = torch.from_numpy(ptr).cuda()
    ws = g.workspace(nat.catalog_topk_workspace(B, N, KF, K), _dev())
    top_s = torch.empty(B, K, dtype=torch.float32, device=_dev())
    top_i = torch.empty(B, K, dtype=torch.int32, device=_dev())
    _raw_call(nat, t, K, ws, top_s, top_i, ptr_d, rows_d, longest, _plan(plan), E=E, w=w)
    g.assert_untouched()
    _same((top_s, top_i), want)


def _overfetch_apply(t, K, plan, lists):
    s64, i64 = (x.cpu().numpy() for x in t.call(64, plan))
    ws, wi = [], []
    for b in range(t.B):
        inside = np.isin(i64[b] + t.n_user, lists[b])
        assert inside.sum() <= 64 - K
        ws.append(s64[b][~inside][:K])
        wi.append(i64[b][~inside][:K])
    return np.stack(ws), np.stack(wi)


def test_argument_checks_leave_the_outputs_untouched():
    from hhfm_amd import ops
    from hhfm_amd._native import native
    nat = native()
    N, B, K = 4082, 5, 20
    t = _Random(N, "f32", "hhfm", B, seed=1)
    ws = torch.zeros(nat.catalog_topk_workspace(B, N, KF, K), dtype=torch.uint8, device=_dev())
    top_s = torch.full((B, K), 7.5, dtype=torch.float32, device=_dev())
    top_i = torch.full((B, K), -7, dtype=torch.int32, device=_dev())
    ptr = torch.zeros(B + 1, dtype=torch.int64, device=_dev())
    rows = torch.zeros(1, dtype=torch.int32, device=_dev())
    word = ops.pooling_word(POOL)
    with pytest.raises(ValueError):      # FM takes no pooling
        _raw_call(nat, t, K, ws, top_s, top_i, ptr, rows, 0, pooling=word, mode=ops.MODE_FM)
    with pytest.raises(ValueError):      # NULL lists with B > 0
        _raw_call(nat, t, K, ws, top_s, top_i, None, rows, 0)
    with pytest.raises(ValueError):      # K + max_excl > item_count
        _raw_call(nat, t, K, ws, top_s, top_i, ptr, rows, N - K + 1)
    with pytest.raises(ValueError):
        _raw_call(nat, t, K, ws, top_s, top_i, ptr, rows, 81, cnt=100)
    with pytest.raises(ValueError):
        _raw_call(nat, t, K, ws, top_s, top_i, ptr, rows, -1)
    torch.cuda.synchronize()
    assert (top_s == 7.5).all() and (top_i == -7).all()
    _raw_call(nat, t, K, ws, top_s, top_i, ptr, rows, N - K)      # the largest promise
    _same((top_s, top_i), [x.cpu().numpy() for x in t.call(K, ops.PLAN_STORE)])
    with pytest.raises(NotImplementedError):
        ops.catalog_topk(t.A, t.E, ops.MODE_HHFM, K, 7, N, ctx=(2, 4), pooling2=(0, 0, 0),
                         exclude=ops.exclusion_lists([[]] * B, _dev()))
    with pytest.raises(ValueError):      # lists for another number of queries
        t.call(K, 0, ops.exclusion_lists([[]] * (B + 1), _dev()))


# ---------------------------------------------------------------------------
# hhfm_pf_exclusion_lists
# ---------------------------------------------------------------------------
def _frappe_split(rng, rows_n=6000):
    """A Frappe-shaped split: 10 columns, few distinct keys so that a key
    gathers many items.  -> (positive_feedback, train rows)."""
    n_user, n_item = 20, 400
    cards = (3, 2, 2, 2, 3, 2, 2, 2)
    cols = [rng.integers(0, n_user, rows_n), rng.integers(n_user, n_user + n_item, rows_n)]
    off = n_user + n_item
    for n, c in enumerate(cards):      # one live context column: 60 keys in all
        cols.append(off + (rng.integers(0, c, rows_n) if n == 0 else np.zeros(rows_n, np.int64)))
        off += c
    X = np.stack(cols, 1).astype(np.int64)
    pf = {}
    for r in X:
        pf.setdefault(xr.row_key(r), set()).add(int(r[1]))
    return pf, X, off


@pytest.mark.parametrize("keep_own", [False, True])
def test_pf_exclusion_lists_match_the_dict(keep_own):
    from hhfm_amd import harness, ops
    rng = np.random.default_rng(9)
    pf, X, M = _frappe_split(rng)
    assert max(len(v) for v in pf.values()) > 64
    rows = X[rng.integers(0, len(X), 1500)].copy()
    rows[::7, 0] = M + 5                      # unknown keys
    rows[1::5, 1] = rng.integers(20, 420, len(rows[1::5]))      # own item mostly no positive
    dp = harness.DevicePairSet(pf, rows.shape[1] - 1, _dev())
    r = torch.from_numpy(rows.astype(np.int32)).cuda()
    got = ops.pf_exclusion_lists(dp.keys, dp.codes, r, 1, keep_own=keep_own)
    want = xr.lists_from_pf(pf, rows, 1, keep_own)
    ptr, flat, longest = xr.csr(want)
    assert np.array_equal(got.ptr.cpu().numpy(), ptr)
    assert np.array_equal(got.rows.cpu().numpy(), flat)
    assert got.max_len == longest and len(got) == len(rows)
    own = sum(int(x[1]) in pf.get(xr.row_key(x), ()) for x in rows)
    assert own > 500 and any(len(x) == 0 for x in want)
    # empty positive_feedback and B = 0
    empty = harness.DevicePairSet({}, rows.shape[1] - 1, _dev())
    e = ops.pf_exclusion_lists(empty.keys, empty.codes, r, 1, keep_own=keep_own)
    assert e.max_len == 0 and e.rows.numel() == 0 and not e.ptr.cpu().numpy().any()
    z = ops.pf_exclusion_lists(dp.keys, dp.codes, r[:0].contiguous(), 1, keep_own=keep_own)
    assert z.ptr.cpu().tolist() == [0] and z.rows.numel() == 0 and z.max_len == 0


def test_pf_exclusion_lists_capacity():
    """A fill call whose capacity is below excl_ptr[B] is HHFM_EWORKSPACE and
    writes nothing."""
    from hhfm_amd import harness, ops
    from hhfm_amd._native import native
    nat = native()
    rng = np.random.default_rng(10)
    pf, X, M = _frappe_split(rng, 2000)
    rows = torch.from_numpy(X[:200].astype(np.int32)).cuda()
    dp = harness.DevicePairSet(pf, X.shape[1] - 1, _dev())
    B = 200
    ws = torch.empty(nat.pf_exclusion_lists_workspace(B), dtype=torch.uint8, device=_dev())
    ptr = torch.empty(B + 1, dtype=torch.int64, device=_dev())
    st = torch.cuda.current_stream().cuda_stream
    args = (dp.keys.data_ptr(), dp.keys.shape[0], 9, dp.codes.data_ptr(), dp.codes.numel(),
            rows.data_ptr(), B, 10, 1, 0, ptr.data_ptr())
    nat.pf_exclusion_lists(*args, 0, 0, ws.data_ptr(), ws.numel(), st)
    total = int(ptr[B])
    assert total > B
    out = torch.full((total,), -9, dtype=torch.int32, device=_dev())
    with pytest.raises(ValueError):
        nat.pf_exclusion_lists(*args, out.data_ptr(), total - 1, ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    assert (out == -9).all()
    with pytest.raises(ValueError):      # the sizing call needs its workspace
        nat.pf_exclusion_lists(*args, 0, 0, ws.data_ptr(), 8, st)
    nat.pf_exclusion_lists(*args, out.data_ptr(), total, ws.data_ptr(), ws.numel(), st)
    want = xr.csr(xr.lists_from_pf(pf, X[:200], 1, False))
    assert np.array_equal(out.cpu().numpy(), want[1])


# ---------------------------------------------------------------------------
# models and the harness
# ---------------------------------------------------------------------------
def _model(kind, d, **kw):
    from hhfm_amd.FM import FM
    from hhfm_amd.OurModel7 import OUR
    M, k = d.E.shape
    if kind == "fm":
        m = FM(4, M, d.n_user, d.N, k, 0.1, 0.1, 1, "AdagradOptimizer", 0, 0)
        m.set_weights(feature_embeddings=d.E, feature_bias=d.w[:, None], bias=0.0)
    else:
        m = OUR(2, 0, M, d.n_user, d.N, k, 0.1, 0.01, "AdagradOptimizer", True, False, **kw)
        m.set_weights(feature_embeddings=d.E)
    return m


@pytest.mark.parametrize("kind", ["fm", "hhfm"])
def test_model_topk_with_a_positive_feedback_dict(kind):
    """FM.topk / OUR.topk(A, 20, exclude=pf) against the numpy reference over
    catalog scores taken from the model's own score_rows on a design."""
    N, B, K = 300, 12, 20
    d = sd.make("periodic", N, 16, "f32", kind, B=B)
    m = _model(kind, d)
    rng = np.random.default_rng(4)
    pf = {}
    for b in range(0, B, 2):      # every second query's key is known
        pf[xr.row_key(d.A[b])] = set(
            int(x) for x in d.item_begin + rng.choice(N, size=40 + b, replace=False))
    pf[(99, 98, 97)] = {d.item_begin}
    full = np.repeat(d.A[:, None, :], N, axis=1)
    full[:, :, 1] = d.item_begin + np.arange(N)
    scores = m.score_rows(full.reshape(-1, d.A.shape[1])).reshape(B, N)
    if kind == "hhfm":
        assert np.array_equal(scores, d.scores)
    lists = xr.lists_from_pf(pf, d.A)
    # (FM.out differs from the catalog score by a per-query constant: ids alone)
    got = m.topk(d.A, K, exclude=pf)
    assert np.array_equal(got, xr.filtered_topk(scores, K, lists, d.item_begin)[1])
    want = xr.filtered_topk(d.scores, K, lists, d.item_begin)
    assert np.array_equal(got, want[1])
    plain = m.topk(d.A, K)
    assert np.array_equal(m.topk(d.A, K, exclude={}), plain)
    assert not np.array_equal(got, plain)
    from hhfm_amd import ops
    x = ops.exclusion_lists(lists, m.device)
    s, i = m.catalog_topk(m._idx(d.A), 0, N, K, exclude=x)
    _same((s, i), want)


def test_two_way_model_refuses_exclusion_lists():
    d = sd.make("periodic", 300, 16, "f32", "hhfm", B=4)
    m = _model("hhfm", d, two_way=True)

    class Boom(dict):
        def get(self, *a):
            raise AssertionError("the lists were built")

    with pytest.raises(NotImplementedError):
        m.topk(np.full((4, 4), 10 ** 9), 20, exclude=Boom())      # bad ids: nothing may run
    with pytest.raises(NotImplementedError):
        m.catalog_topk(m._idx(d.A), 0, 300, 20, exclude={})
    assert m.topk(d.A, 20).shape == (4, 20)


def test_evaluate_topk_filtered_equals_a_python_walk():
    from hhfm_amd import harness, ops
    from hhfm_amd.FM import FM
    from hhfm_amd.NewLoadData import LoadData
    np.random.seed(2016)
    d = LoadData(G + "/", "synth_frappe")
    m = FM(d.Train_data.shape[1] - 1, d.features_M, d.n_user, d.n_item, 16, 0.1, 0.1, 1,
           "AdagradOptimizer", 0, 0)
    m.set_weights(feature_embeddings=np.random.default_rng(3).normal(
        0, 0.1, (d.features_M, 16)).astype(np.float32))
    t = harness.Train(data=d, model=m)
    t.TopK = 10
    np.random.seed(31)
    got = t.evaluate_TopK_filtered(d.Test_data)
    after = np.random.randint(0, 1 << 30)
    # the same batches, the lists from the dict on the host, a walk in plain Python
    np.random.seed(31)
    dat, pf = d.Test_data.values, d.positive_feedback
    hits, ndcg, pre = [], [], []
    for _ in range(int(min(3000, len(dat)) / t.eval_num)):
        feed = np.array(dat[:, 1:][np.random.randint(0, len(dat), t.eval_num)], dtype=np.int64)
        lists = xr.lists_from_pf(pf, feed, 1, keep_own=True)
        pred = m.topk(feed, 20, exclude=ops.exclusion_lists(lists, m.device)) + d.n_user
        for line, lst, p in zip(feed, lists, pred):
            assert not np.isin(p, lst).any()
            n = next((j for j, it in enumerate(p[:t.TopK]) if it == line[1]), None)
            hits.append(0 if n is None else 1)
            ndcg.append(0 if n is None else np.log(2) / np.log(n + 2))
            pre.append(0 if n is None else 1 / (n + 1))
    assert len(hits) >= 300 and len(hits) % t.eval_num == 0
    assert got == [np.average(hits), np.average(ndcg), np.average(pre)]
    assert after == np.random.randint(0, 1 << 30)      # the same np.random draws as the walk here
    # and the same draws as evaluate_TopK
    np.random.seed(31)
    t.evaluate_TopK(d.Test_data)
    assert after == np.random.randint(0, 1 << 30)


def test_filter_seen_parses():
    from hhfm_amd import FM, OurModel7
    for mod in (FM, OurModel7):
        assert mod.parse_args("frappe", 64, 10, []).filter_seen == 0
        assert mod.parse_args("frappe", 64, 10, ["--filter_seen", "1"]).filter_seen == 1
