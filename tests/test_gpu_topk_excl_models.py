"""Exclusion lists of the AFM, DeepFM and CARS2 catalogs and of the dense select
behind them (include/hhfm.h "Exclusion lists"), tolerance-free.

* The raw select, hhfm_topk_dense_excl, on designed score matrices against
  tests/topk_excl_ref.filtered_topk: equal ids and equal score bits, on the
  one-wave and the four-waves-per-query kernels, at the 2,048-score chunk edge
  and the split spans' edges, with lists that empty a chunk or a span, that
  leave exactly K columns, and that carry ids which must not matter.
* The models against their own PLAIN call, which this feature does not touch:
  with at most e = 44 listed items among a query's plain top-64, the filtered
  top-20 is the plain top-64 without the listed items, first 20 (the
  over-fetch identity, proved for the numpy reference in
  tests/test_topk_excl_models_ref.py).  The filtered call is never its own
  yardstick.

Every comparison is np.array_equal on int32 ids and on float32 scores viewed as
int32.
"""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import score_designs as sd
from tests import topk_excl_ref as xr
from tests.test_gpu_workspace_contract import _aa, _afm, _dev, _dfm, poison  # noqa: F401

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
CHUNK = 2048          # HHFM_TOPK_NV * 64 scores per fold
NOIDX = 0x7fffffff


def _cuda():
    return torch.device("cuda", 0)


def _same(got, want, what=""):
    gs, gi = (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in got)
    ws, wi = (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in want)
    if not np.array_equal(gi, wi):
        b, p = np.argwhere(gi != wi)[0]
        raise AssertionError(f"{what}: ids differ at {int((gi != wi).sum())} positions; first "
                             f"query {b} rank {p}: got {gi[b, p]} ({gs[b, p]}), "
                             f"expected {wi[b, p]} ({ws[b, p]})")
    assert np.array_equal(sd.bits(gs), sd.bits(ws)), f"{what}: score bits differ"


# ---------------------------------------------------------------------------
# the raw select on designed scores
# ---------------------------------------------------------------------------
DESIGNS = ("all_equal", "plateau_spikes", "periodic", "ascending")
SIZES = (65, 300, 2047, 2048, 2049, 4082)
KS = (1, 20, 33, 64)
KINDS = ("empty", "one", "63", "64", "65", "n_minus_k", "first_chunk", "span", "topk")


def _matrix(design, N, B):
    """float32 [B, N]: the design's values times 3 / -2 / 0 (the designed order,
    its reverse, all equal) plus the query number."""
    v = sd.values(design, N, m=21 if N >= 1024 else 5).astype(np.float32)   # (spikes at edges)
    a = np.asarray(sd.A_VALUES, np.float32)[np.arange(B) % 3]
    return (a[:, None] * v[None, :] + np.arange(B, dtype=np.float32)[:, None]).astype(np.float32)


def _span(N):
    return (((N + 3) // 4) + 63) // 64 * 64


def _columns(kind, row, N, K, b, rng):
    """The listed columns of one query (ascending, unique), at most N - K."""
    room = N - K
    if kind == "empty":
        cols = np.zeros(0, np.int64)
    elif kind == "one":
        cols = np.array([int(np.argmax(row))])          # the best column
    elif kind in ("63", "64", "65"):
        cols = rng.choice(N, size=min(int(kind), room), replace=False)
    elif kind == "n_minus_k":                           # exactly K columns left
        cols = rng.choice(N, size=room, replace=False)
    elif kind == "first_chunk":                         # the whole first chunk: the threshold seed
        cols = np.arange(min(CHUNK, N))
    elif kind == "span":                                # a whole split span: a wave with nothing
        sp, part = _span(N), b % 4
        cols = np.arange(min(part * sp, N), min((part + 1) * sp, N))
    else:                                               # exactly the plain top K
        cols = np.argsort(-row, kind="stable")[:K]
    cols = np.unique(cols)
    if len(cols) > room:                                # infeasible here: exactly K left instead
        cols = np.sort(rng.choice(N, size=room, replace=False))
    return cols.astype(np.int64)


def _raw_lists(S, K, irb, shift, rng):
    B, N = S.shape
    return [_columns(KINDS[(b + shift) % len(KINDS)], S[b], N, K, b, rng) + irb for b in range(B)]


def _select(S, K, lists, irb=0, base=0, plan=0):
    from hhfm_amd import ops
    x = ops.exclusion_lists(lists, _cuda())
    return ops.topk_dense(S, K, base, plan, exclude=x, item_row_begin=irb)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("design", DESIGNS)
def test_raw_select_designed(design, N):
    """B in {1, 5, 37} x K in {1, 20, 33, 64}; the list kinds rotate through
    the queries, so every (kind, K) pair is met at every size.  N < 1,024 runs
    the one-wave kernel, N >= 1,024 four waves per query (spans of 512 at
    2,047 / 2,048, 576 at 2,049, 1,024 at 4,082).  The matrix is read only."""
    from hhfm_amd import ops
    rng = np.random.default_rng(N)
    irb, base = 11, 1000
    for bi, B in enumerate((1, 5, 37)):
        Sh = _matrix(design, N, B)
        S = torch.from_numpy(Sh).cuda()
        before = S.clone()
        for ki, K in enumerate(KS):
            shifts = range(len(KINDS)) if B == 1 else (bi + ki,)
            for shift in shifts:
                lists = _raw_lists(Sh, K, irb, shift, rng)
                want = xr.filtered_topk(Sh, K, lists, irb, gbase=base)
                what = f"{design} N={N} B={B} K={K} shift={shift}"
                got = _select(S, K, lists, irb, base)
                _same(got, want, what)
                if B == 5 and N >= 1024:
                    _same(_select(S, K, lists, irb, base, ops.PLAN_ONE_WAVE), got,
                          what + " one wave == split")
        assert torch.equal(S.view(torch.int32), before.view(torch.int32)), "the matrix was written"


def test_raw_select_one_wave_route_at_many_queries():
    """B = 1,025 > 1,024 queries of 2,049 columns: one wave per query folds two
    chunks, the second of one score."""
    B, N, K = 1025, 2049, 20
    rng = np.random.default_rng(1)
    Sh = _matrix("periodic", N, B)
    Sh[:, -1] = 1e6                                     # the lone score of the second chunk leads
    lists = _raw_lists(Sh, K, 0, 0, rng)
    lists[3] = np.array([N - 1], np.int64)              # ... and is listed once
    S = torch.from_numpy(Sh).cuda()
    _same(_select(S, K, lists), xr.filtered_topk(Sh, K, lists, 0), "B=1025")


def test_raw_select_leading_dimension():
    """Rows that are a column slice of a wider matrix."""
    N, B, K = 2049, 5, 33
    rng = np.random.default_rng(2)
    wide = np.full((B, N + 37), 1e9, np.float32)
    wide[:, :N] = _matrix("plateau_spikes", N, B)
    W = torch.from_numpy(wide).cuda()
    lists = _raw_lists(wide[:, :N], K, 0, 4, rng)
    _same(_select(W[:, :N], K, lists), xr.filtered_topk(wide[:, :N], K, lists, 0), "ld > N")


@pytest.mark.parametrize("N,B", [(300, 5), (2049, 5), (4082, 37)])
def test_raw_select_ids_that_must_not_matter(N, B):
    """Negative ids, ids past the table and rows below / above the shard
    (item_row_begin > 0) inside valid ascending lists: the result equals the
    call without them, which equals the reference."""
    K, irb, M = 20, 500, 500 + N + 50
    rng = np.random.default_rng(N + B)
    Sh = _matrix("periodic", N, B)
    S = torch.from_numpy(Sh).cuda()
    kinds = ("one", "63", "topk", "empty", "65")
    clean = [_columns(kinds[b % 5], Sh[b], N, K, b, rng) + irb for b in range(B)]
    junk = np.array([-2 ** 31, -5, -1, 0, 3, irb - 1, irb + N, irb + N + 7, M, M + 9, 2 ** 31 - 1])
    dirty = [np.unique(np.concatenate([c, junk])) for c in clean]
    assert max(len(x) for x in dirty) + K <= N
    want = xr.filtered_topk(Sh, K, clean, irb)
    _same(_select(S, K, clean, irb), want, "clean")
    _same(_select(S, K, dirty, irb), want, "with ids outside the range")


def test_raw_select_empty_lists_equal_the_plain_select():
    from hhfm_amd import ops
    for N, B in ((300, 5), (2049, 37), (2049, 1025)):
        S = torch.from_numpy(_matrix("plateau_spikes", N, B)).cuda()
        for K in (1, 20, 64):
            for plan in (0, ops.PLAN_ONE_WAVE):
                plain = ops.topk_dense(S, K, 7, plan)
                empty = ops.exclusion_lists([[]] * B, _cuda())
                assert empty.rows.numel() == 0
                _same(ops.topk_dense(S, K, 7, plan, exclude=empty), plain, f"N={N} B={B} K={K}")
                # a rows array that no list points into
                full = ops.ExclusionLists(empty.ptr, torch.zeros(4, dtype=torch.int32,
                                                                 device=_cuda()), 0)
                _same(ops.topk_dense(S, K, 7, plan, exclude=full), plain, "unused rows")


def test_raw_select_argument_checks_leave_the_outputs_untouched():
    from hhfm_amd._native import native
    nat = native()
    B, N, K = 5, 300, 20
    S = torch.from_numpy(_matrix("ascending", N, B)).cuda()
    top_s = torch.full((B, K), 7.5, dtype=torch.float32, device=_cuda())
    top_i = torch.full((B, K), -7, dtype=torch.int32, device=_cuda())
    ptr = torch.zeros(B + 1, dtype=torch.int64, device=_cuda())
    rows = torch.zeros(1, dtype=torch.int32, device=_cuda())
    st = torch.cuda.current_stream().cuda_stream

    def call(p, r, max_excl, n=N, k=K):
        nat.topk_dense_excl(S.data_ptr(), B, n, N, k, 0, top_s.data_ptr(), top_i.data_ptr(), 0, st,
                            0, p, r, max_excl)

    for args in ((0, rows.data_ptr(), 0),                       # NULL excl_ptr with B > 0
                 (ptr.data_ptr(), rows.data_ptr(), -1),
                 (ptr.data_ptr(), rows.data_ptr(), N - K + 1),
                 (ptr.data_ptr(), 0, N - K + 1)):
        with pytest.raises(ValueError):
            call(*args)
    with pytest.raises(ValueError):
        call(ptr.data_ptr(), rows.data_ptr(), 81, n=100)        # K + max_excl > N = 100
    torch.cuda.synchronize()
    assert (top_s == 7.5).all() and (top_i == -7).all()
    call(ptr.data_ptr(), 0, N - K)                              # the largest promise, no rows
    _same((top_s, top_i), sd.expected_topk(S.cpu().numpy(), K), "after the refused calls")


# ---------------------------------------------------------------------------
# the models: cases as closures over ops-level calls
# ---------------------------------------------------------------------------
B_Q, K_M, E_MAX = 12, 20, 44


class _Case:
    """One model's catalog call: ``call(K, exclude, begin, count, gbase)`` over
    items [begin, begin + count) of N; ``n_user`` is the catalog's first table
    row; ``tables`` are the device tensors a tie block is written into (rows
    of the table, and w where the model has one)."""

    def __init__(self, name, N, n_user, call, tables):
        self.name, self.N, self.n_user, self._call, self.tables = name, N, n_user, call, tables

    def call(self, K, exclude=None, begin=0, count=None, gbase=0):
        count = self.N - begin if count is None else count
        return self._call(K, exclude, begin, count, gbase)


def _afm_case(N, plan_name, table):
    from hhfm_amd import ops
    plan = {"w": 0, "fused": ops.PLAN_PER_FIELD, "gemm": ops.PLAN_GEMM}[plan_name]
    F, k, A = 5, 32, 32
    m = _afm(F, k, A, nu=100, ni=N, table=table)
    q = m["X"][:B_Q].contiguous()
    max_cols = 5 * (F - 1) * A                          # query chunks of 5, 5, 2

    def call(K, exclude, begin, count, gbase):
        return ops.afm_catalog_topk(q, m["E"], m["w"], *m["att"], m["nu"] + begin, count, K, gbase,
                                    max_cols, plan=plan, exclude=exclude)
    return _Case(f"afm-{plan_name}-{table}", N, m["nu"], call, (m["E"], m["w"]))


def _noatt_case(N, table):
    from hhfm_amd import ops
    m = _afm(5, 32, 32, nu=100, ni=N, table=table)
    q = m["X"][:B_Q].contiguous()
    P = m["att"][3]

    def call(K, exclude, begin, count, gbase):
        return ops.afm_noatt_catalog_topk(q, m["E"], m["w"], 0.02, P, m["nu"] + begin, count, K,
                                          gbase, exclude=exclude)
    return _Case(f"afm0-{table}", N, m["nu"], call, (m["E"], m["w"]))


def _dfm_case(N, head_name, mlp, table):
    from hhfm_amd import ops
    F, k = 5, 32
    m = _dfm(50, N, F, k, [64, 48], mlp, table=table, deep_head=head_name == "deep")
    q = m["X"][:B_Q].contiguous()
    head = {"full": None, "deep": ops.DFM_HEAD_DEEP, "fm": ops.DFM_HEAD_FM}[head_name]
    Wp = m["Wp"][:F + k].contiguous() if head_name == "fm" else m["Wp"]

    def call(K, exclude, begin, count, gbase):
        return ops.dfm_catalog_topk(q, m["E"], m["w"], m["Wt"], m["bs"], m["dims"], Wp, m["bp"], 1,
                                    m["nu"] + begin, count, K, gbase, 5 * count, head=head,
                                    exclude=exclude)            # query chunks of 5, 5, 2
    return _Case(f"dfm-{head_name}-{mlp}-{table}", N, m["nu"], call, (m["E"], m["w"]))


def _cars2_case(N, table):
    from hhfm_amd import ops
    from tests import cars2_ref as cr
    D, Mc, nu = 64, 9, 300
    Wt = cr.weights(N, nu + N, Mc, D)
    prepared = ops.cars2_prepare(*(_dev(Wt[n]) for n in ("Context", "W", "Z", "A", "B")))
    rng = np.random.default_rng(N + 1)
    q = _dev(np.stack([rng.integers(0, nu, B_Q), rng.integers(0, Mc, B_Q)], 1).astype(np.int32))
    UI = _dev(Wt["UI"])
    if table == "bf16":
        UI = UI.to(torch.bfloat16)

    def call(K, exclude, begin, count, gbase):
        return ops.cars2_catalog_topk(q, UI, prepared, Mc, K, nu + begin, count, gbase,
                                      exclude=exclude)
    return _Case(f"cars2-{table}", N, nu, call, (UI,))


CASES = {
    "afm-w-f32": lambda N: _afm_case(N, "w", "f32"),
    "afm-w-bf16": lambda N: _afm_case(N, "w", "bf16"),
    "afm-fused-f32": lambda N: _afm_case(N, "fused", "f32"),
    "afm-gemm-f32": lambda N: _afm_case(N, "gemm", "f32"),
    "afm0-f32": lambda N: _noatt_case(N, "f32"),
    "afm0-bf16": lambda N: _noatt_case(N, "bf16"),
    "dfm-full-f32": lambda N: _dfm_case(N, "full", "f32", "f32"),
    "dfm-full-f32-bf16table": lambda N: _dfm_case(N, "full", "f32", "bf16"),
    "dfm-deep-f32": lambda N: _dfm_case(N, "deep", "f32", "f32"),
    "dfm-fm-f32": lambda N: _dfm_case(N, "fm", "f32", "f32"),
    "dfm-full-bf16mlp": lambda N: _dfm_case(N, "full", "bf16", "f32"),
    "cars2-f32": lambda N: _cars2_case(N, "f32"),
    "cars2-bf16": lambda N: _cars2_case(N, "bf16"),
}
ONE_PER_MODEL = ("afm-w-f32", "afm0-f32", "dfm-full-f32", "cars2-f32")


def _host(out):
    return tuple(x.cpu().numpy() for x in out)


def _from_plain64(c, lists, K=K_M, **kw):
    """The over-fetch identity's right-hand side: the plain top-64 without the
    listed items, first K — asserting that at most 44 of them are listed."""
    s64, i64 = _host(c.call(64, None, **kw))
    begin, gbase = kw.get("begin", 0), kw.get("gbase", 0)
    ws, wi = [], []
    for b in range(len(s64)):
        inside = np.isin(i64[b] - gbase + begin + c.n_user, lists[b])
        assert inside.sum() <= E_MAX
        ws.append(s64[b][~inside][:K])
        wi.append(i64[b][~inside][:K])
    return np.stack(ws), np.stack(wi)


def _biting_lists(c, rng, empty_every=4):
    """Per query up to 44 catalog rows, half of them from the query's plain
    top-30; every fourth query lists nothing."""
    _, i64 = _host(c.call(64))
    lists = []
    for b in range(len(i64)):
        if b % empty_every == empty_every - 1:
            lists.append(np.zeros(0, np.int64))
            continue
        n = (8, 30, E_MAX)[b % 3]
        top = rng.choice(i64[b, :30], size=n // 2, replace=False)
        rest = rng.choice(np.setdiff1d(np.arange(c.N), top), size=n - n // 2, replace=False)
        lists.append(np.unique(np.concatenate([top, rest])) + c.n_user)
    return lists


@pytest.mark.parametrize("N", [300, 4082])
@pytest.mark.parametrize("name", sorted(CASES))
def test_model_overfetch_identity(name, N):
    """B = 12 queries in query chunks of 5, 5 and 2 (AFM, DeepFM), so a list
    array that is not moved on with the chunk shows."""
    from hhfm_amd import ops
    c = CASES[name](N)
    rng = np.random.default_rng(N)
    lists = _biting_lists(c, rng)
    want = _from_plain64(c, lists)
    got = _host(c.call(K_M, ops.exclusion_lists(lists, _cuda())))
    _same(got, want, c.name)
    plain = _host(c.call(K_M))
    for b, lst in enumerate(lists):
        if len(lst):
            assert not np.array_equal(got[1][b], plain[1][b]), f"query {b}: the list did not bite"
            assert not np.isin(got[1][b] + c.n_user, lst).any()
        else:
            assert np.array_equal(got[1][b], plain[1][b])


@pytest.mark.parametrize("N", [300, 4082])
@pytest.mark.parametrize("name", sorted(CASES))
def test_model_exact_ties(name, N):
    """Query 0's best item copied into 70 consecutive catalog rows (across the
    2,048 chunk edge at N = 4,082): 70 bitwise equal scores that lead query 0.
    Every second one listed: the survivors come out in ascending id order,
    ahead of the rest, and every query equals the over-fetch identity."""
    from hhfm_amd import ops
    c = CASES[name](N)
    _, i1 = _host(c.call(1))
    src = int(i1[0, 0])
    lo = 100 if N == 300 else CHUNK - 28
    block = np.arange(lo, lo + 70)
    for t in c.tables:
        t[c.n_user + lo:c.n_user + lo + 70] = t[c.n_user + src]
    s64, i64 = _host(c.call(64))
    tied = np.union1d(block, [src])
    assert np.array_equal(i64[0], tied[:64]) and len(np.unique(sd.bits(s64[0]))) == 1
    listed = block[::2]
    lists = [listed + c.n_user] * B_Q
    want = _from_plain64(c, lists)
    got = _host(c.call(K_M, ops.exclusion_lists(lists, _cuda())))
    _same(got, want, c.name)
    survivors = np.setdiff1d(tied, listed)
    assert np.array_equal(got[1][0], survivors[:K_M])
    assert np.array_equal(sd.bits(got[0][0]), sd.bits(s64[0][:K_M]))
    # and as a matrix for the numpy reference: query 0's row from its plain top-64
    row = np.full((1, N), -np.inf, np.float32)
    row[0, i64[0]] = s64[0]
    ref = xr.filtered_topk(row, K_M, [lists[0]], c.n_user)
    _same((got[0][:1], got[1][:1]), ref, c.name + " filtered_topk")


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_empty_lists_equal_the_plain_call(name):
    from hhfm_amd import ops
    c = CASES[name](300)
    plain = _host(c.call(K_M))
    empty = ops.exclusion_lists([[]] * B_Q, _cuda())
    assert empty.rows.numel() == 0 and empty.max_len == 0
    _same(_host(c.call(K_M, empty)), plain, c.name)
    outside = ops.exclusion_lists([[-5, 0, 3, c.n_user + 300, c.n_user + 999]] * B_Q, _cuda())
    _same(_host(c.call(K_M, outside)), plain, c.name + " ids outside the range")
    with pytest.raises(ValueError):
        c.call(K_M, ops.exclusion_lists([[]] * (B_Q + 1), _cuda()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_two_shards_merge_to_the_single_call(name):
    from hhfm_amd import ops
    N = 4082
    c = CASES[name](N)
    lists = _biting_lists(c, np.random.default_rng(8))
    x = ops.exclusion_lists(lists, _cuda())
    single = c.call(K_M, x, gbase=1000)
    _same(_host(single), _from_plain64(c, lists, gbase=1000), c.name)
    cut = N // 2 + 5
    a = c.call(K_M, x, 0, cut, 1000)
    b = c.call(K_M, x, cut, N - cut, 1000 + cut)
    _same(ops.topk_merge(torch.stack([a[0], b[0]]), torch.stack([a[1], b[1]])), single, c.name)


@pytest.mark.parametrize("name", ONE_PER_MODEL + ("dfm-deep-f32", "afm-gemm-f32"))
def test_model_poisoned_scratch(poison, name):  # noqa: F811
    """Zero, 0xFF and 0x7F workspace bytes: the same bits, the guards
    untouched, the catalog workspace's zero prefix left zero."""
    from hhfm_amd import ops
    c = CASES[name](777)
    rng = np.random.default_rng(3)
    seqs = [sorted({c.n_user, c.n_user + 776} | set(rng.integers(c.n_user, c.n_user + 777,
                                                                  b * 3).tolist()))
            if b % 5 else [] for b in range(B_Q)]
    x = ops.exclusion_lists(seqs, _cuda())
    _aa(poison, lambda: c.call(K_M, x), c.name)


# ---------------------------------------------------------------------------
# the model classes and the harness
# ---------------------------------------------------------------------------
def _frappe():
    from hhfm_amd.NewLoadData import LoadData
    np.random.seed(2016)
    return LoadData(G + "/", "synth_frappe")


def _class_model(kind, d):
    from hhfm_amd.AFM import AFM
    from hhfm_amd.DFM import DeepFM
    F = d.Train_data.shape[1] - 1
    if kind == "afm":
        return AFM(d.n_user, d.n_item, d.features_M, 1, [16, 16], None, 0.1, 100.0, [1, 1],
                   "AdagradOptimizer", 0.999, F)
    if kind == "afm0":
        m = AFM(d.n_user, d.n_item, d.features_M, 0, [16, 16], None, 0.1, 100.0, [1, 1],
                "AdagradOptimizer", 0.999, F)
        m.set_weights(feature_bias=np.random.default_rng(1).normal(
            0, 0.1, (d.features_M, 1)).astype(np.float32))
        return m
    return DeepFM(d.n_user, d.n_item, d.features_M, F, 16, [24, 16], None, 0.01, 0, 0.01)


def _cars2_train(d):
    from hhfm_amd import CARS2
    args = argparse.Namespace(Result=1, dataset="synth_frappe", result_file=None, epoch=1,
                              batch_size=512, TopK=10, hidden_factor=16, lr=0.01, lamda=0.001,
                              keep=1, optimizer="AdagradOptimizer", batch_norm=0)
    return CARS2.Train(args, data=d)


@pytest.mark.parametrize("kind", ["afm", "afm0", "dfm", "cars2"])
def test_model_topk_with_a_positive_feedback_dict(kind):
    """model.topk(A, 20, exclude=pf_dict) equals exclude=ops.exclusion_lists(
    lists_from_pf(...)), leaves the listed items out, and equals the plain
    call for exclude={}.  CARS2: through the harness's full rows, and on its
    own (user, context id) queries with a dict keyed by those pairs."""
    from hhfm_amd import CARS2, ops
    d = _frappe()
    rows = np.array(d.Train_data.values[:40, 1:], dtype=np.int64)     # keys that pf knows
    pf = d.positive_feedback
    lists = xr.lists_from_pf(pf, rows)
    assert all(len(x) > 0 for x in lists)
    if kind == "cars2":
        t = _cars2_train(d)
        m = CARS2._FullRows(t.model, t.feature_inject)
    else:
        m = _class_model(kind, d)
    x = ops.exclusion_lists(lists, _cuda())
    got = m.topk(rows, 20, exclude=pf)
    assert np.array_equal(got, m.topk(rows, 20, exclude=x))
    plain = m.topk(rows, 20)
    assert np.array_equal(m.topk(rows, 20, exclude={}), plain)
    assert np.array_equal(m.topk(rows, 20, exclude=ops.exclusion_lists([[]] * len(rows), _cuda())),
                          plain)
    for b, lst in enumerate(lists):
        assert not np.isin(got[b] + d.n_user, lst).any()
        # the plain list without the listed items is a prefix of the filtered one
        keep = plain[b][~np.isin(plain[b] + d.n_user, lst)]
        assert np.array_equal(got[b][:len(keep)], keep)
    assert not np.array_equal(got, plain)
    if kind == "cars2":
        q = np.stack([rows[:, 0], t.context_ids(rows)], 1)
        pairs = {tuple(int(v) for v in q[b]): set(int(i) for i in lists[b]) for b in range(len(q))
                 if len(lists[b])}
        byq = [sorted(pairs.get(tuple(int(v) for v in r), ())) for r in q]
        assert np.array_equal(t.model.topk(q, 20, exclude=pairs),
                              t.model.topk(q, 20, exclude=ops.exclusion_lists(byq, _cuda())))


@pytest.mark.parametrize("kind", ["afm", "dfm", "cars2"])
def test_evaluate_topk_filtered_equals_a_python_walk(kind):
    from hhfm_amd import CARS2, harness, ops
    d = _frappe()
    if kind == "cars2":
        t = _cars2_train(d)
        m = CARS2._FullRows(t.model, t.feature_inject)
    else:
        m = _class_model(kind, d)
        t = harness.Train(data=d, model=m)
    t.TopK = 10
    np.random.seed(31)
    got = t.evaluate_TopK_filtered(d.Test_data)
    after = np.random.randint(0, 1 << 30)
    np.random.seed(31)
    dat, pf = d.Test_data.values, d.positive_feedback
    hits, ndcg, pre = [], [], []
    for _ in range(int(min(3000, len(dat)) / t.eval_num)):
        feed = np.array(dat[:, 1:][np.random.randint(0, len(dat), t.eval_num)], dtype=np.int64)
        lists = xr.lists_from_pf(pf, feed, 1, keep_own=True)
        pred = m.topk(feed, 20, exclude=ops.exclusion_lists(lists, _cuda())) + d.n_user
        for line, lst, p in zip(feed, lists, pred):
            assert not np.isin(p, lst).any()
            n = next((j for j, it in enumerate(p[:t.TopK]) if it == line[1]), None)
            hits.append(0 if n is None else 1)
            ndcg.append(0 if n is None else np.log(2) / np.log(n + 2))
            pre.append(0 if n is None else 1 / (n + 1))
    assert len(hits) >= 300 and len(hits) % t.eval_num == 0
    assert got == [np.average(hits), np.average(ndcg), np.average(pre)]
    assert after == np.random.randint(0, 1 << 30)
    np.random.seed(31)
    t.evaluate_TopK(d.Test_data)
    assert after == np.random.randint(0, 1 << 30)      # the same draws as evaluate_TopK


@pytest.mark.parametrize("entry", ["FM_main", "M7_main", "AFM_main", "DFM_main", "CARS2_main"])
def test_filter_seen_runs_end_to_end(entry, tmp_path, monkeypatch):
    """--filter_seen 1 through argv for every column of a result table: each
    entry point trains one epoch on synth_frappe and reports HR / NDCG / PRE
    from evaluate_TopK_filtered, never from evaluate_TopK."""
    import importlib
    from hhfm_amd import harness
    mod = {"FM_main": "FM", "M7_main": "OurModel7", "AFM_main": "AFM", "DFM_main": "DFM",
           "CARS2_main": "CARS2"}[entry]
    module = importlib.import_module(f"hhfm_amd.{mod}")
    calls = {"filtered": 0}
    real = harness.Train.evaluate_TopK_filtered

    def filtered(self, data1):
        calls["filtered"] += 1
        return real(self, data1)

    def plain(self, data1):
        raise AssertionError("evaluate_TopK ran under --filter_seen 1")

    monkeypatch.setattr(harness.Train, "evaluate_TopK_filtered", filtered)
    monkeypatch.setattr(harness.Train, "evaluate_TopK", plain)
    out = tmp_path / "result.txt"
    argv = ["--path", G + "/", "--epoch", "2", "--batch_size", "4096", "--filter_seen", "1",
            "--result_file", str(out)]
    if entry in ("FM_main", "AFM_main", "DFM_main"):
        argv += ["--verbose", "1"]
    np.random.seed(2016)
    session = getattr(module, entry)("synth_frappe", 16, 5, argv)
    assert session.args.filter_seen == 1 and calls["filtered"] >= 1
    lines = out.read_text().splitlines()
    assert lines and "Init:" in lines[0]
    for ln in lines:
        hr = float(ln.split("HR:")[1].split(",")[0])
        assert 0.0 <= hr <= 1.0, ln
