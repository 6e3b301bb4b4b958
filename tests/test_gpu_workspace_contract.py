"""The workspace contracts of include/hhfm.h on the device.

1. Scratch carries nothing in: every scoring and top-K entry point returns the
   same bits whatever its workspace held — here 0xFF bytes and 0x7F bytes
   (tests/guard_tables.py says what each stands for) — apart from the catalog
   workspace's first HHFM_CATALOG_WS_ZERO bytes, which the caller zeroes once.
2. That prefix is zero again after every call, on every path and plan.
3. One workspace serves any sequence of calls it is large enough for.

Every workspace is handed out by one fixture that replaces
``ops._workspace`` / ``ops._catalog_workspace``: a fresh buffer of exactly the
queried size between two 0xA5 guards, its interior poisoned.  The sampler's
buffer is pre-set on the harness object.  profiles/workspace_contract_map.txt
lists every region of every layout used here with its writer and first reader;
no region that holds ids, offsets or counts is read before the call wrote it,
so a poisoned region can change arithmetic only, never an address.

Comparisons are np.array_equal on ids and on scores viewed as int32.  The
expected output is the designed-score list of tests/score_designs.py where one
exists ("exact"), else the same call on a zero-filled workspace ("A/A": two
zero runs must agree bit for bit first; what the zero run returns is held to
its reference by the entry point's own test module).  Every entry point here
turned out bit-reproducible run to run, so no case falls back on a tolerance.
The fills are looped inside each case: both run for every case.
"""
import functools

import numpy as np
import pytest
import torch

from tests import guard_tables as gt
from tests import hhfm_pool_ref as pr
from tests import score_designs as sd
from tests import topk_excl_ref as xr
from tests.test_gpu_catalog_exact import _plans, _same, _tables

pytestmark = pytest.mark.gpu

FILLS = gt.POISONS
BS = (1, 32, 33, 130)            # one group, a full group, a ragged last group, five groups
KS = (1, 20, 32, 33, 64)
DESIGNS = ("all_equal", "plateau_Kp1", "one_per_split", "ascending")
CFGS = (("f32", 16), ("bf16", 64))
RING_CFGS = (("f32", 64), ("bf16", 128))     # the widths catalog_ring takes
MODES = ("fm", "hhfm")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


class _Poison(gt.Guards):
    """Hands out the workspaces of one test.  ``fill``: the byte a fresh
    workspace holds (0: a zero workspace, the A/A baseline); ``hold`` pins one
    buffer for a whole sequence of calls instead."""

    def __init__(self, zero):
        super().__init__()
        self.zero, self.fill, self.cat, self.held, self.sizes = zero, 0, [], {}, []

    def scratch(self, dev, n):
        self.sizes.append(n)
        if "scratch" in self.held:
            assert n <= self.held["scratch"].numel()
            return self.held["scratch"]
        return self.poisoned(max(n, 256), dev, self.fill)

    def catalog(self, dev, n):
        if "catalog" in self.held:
            assert n <= self.held["catalog"].numel()
            v = self.held["catalog"]
        else:
            v = self.poisoned(max(n, 256), dev, self.fill, self.zero)
        self.cat.append(v)
        return v

    def hold(self, kind, nbytes, fill):
        """One workspace for every later call of ``kind``: written here (the
        catalog one with its prefix zero) and never again by the test."""
        self.held[kind] = self.poisoned(nbytes, torch.device("cuda", 0), fill,
                                        self.zero if kind == "catalog" else 0)

    def check(self, what=""):
        """Guards untouched and, for the catalog workspaces handed out since
        the last check, the prefix all zero; then forget the fresh buffers."""
        self.assert_untouched()
        for v in self.cat:
            assert not bool(v[:self.zero].any()), f"{what}: the zero prefix was written"
        self.cat.clear()
        held = list(self.held.values())
        self.pairs[:] = [p for p in self.pairs if any(p[0] is h for h in held)]


@pytest.fixture
def poison(monkeypatch):
    from hhfm_amd import ops
    from hhfm_amd._native import native
    p = _Poison(int(native().CATALOG_WS_ZERO))
    monkeypatch.setattr(ops, "_workspace", p.scratch)
    monkeypatch.setattr(ops, "_catalog_workspace", lambda dev, st, n: p.catalog(dev, n))
    return p


def _snap(out):
    """An entry point's output as a tuple of host arrays, floats as their bits."""
    if isinstance(out, torch.Tensor):
        out = (out,)
    if hasattr(out, "ptr"):                              # ops.ExclusionLists
        out = (out.ptr, out.rows)
    res = []
    for t in out:
        a = t.cpu().numpy()
        res.append(a.view(np.int32) if a.dtype == np.float32 else a)
    return tuple(res)


def _equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _aa(poison, call, what):
    """A/A: ``call`` on two fresh zero-filled workspaces (bit-identical), then
    on a fresh workspace of each poison: the same bits, guards untouched,
    catalog prefix zero.  Returns the zero run's snapshot."""
    poison.fill = 0
    base = _snap(call())
    poison.check(f"{what} zero")
    again = _snap(call())
    poison.check(f"{what} zero")
    assert _equal(base, again), f"{what}: two runs on zero workspaces differ"
    for fill in FILLS:
        poison.fill = fill
        got = _snap(call())
        poison.check(f"{what} fill {fill:#x}")
        assert _equal(got, base), f"{what}: output depends on the workspace (fill {fill:#x})"
    poison.fill = 0
    return base


# ---------------------------------------------------------------------------
# a. poisoned scratch — catalog_topk, FM and HHFM, exact lists
# ---------------------------------------------------------------------------
def _combos(plans, Ks):
    """(K, plan) pairs: the fused kernel and catalog_ring take K <= 32."""
    narrow = ("fused", "ring", "ring_alt", "no_ring")
    return [(K, p) for K in Ks for p in plans if K <= 32 or p not in narrow]


def _flag(plan):
    return _plans()["default" if plan == "ring" else plan]


def _exact(poison, design, N, dtype, k, mode, plans, Ks=KS):
    """Every (K, plan) x B x fill of one table configuration against the
    designed list."""
    n = 0
    for K, plan in _combos(plans, Ks):
        t = _tables(design, N, K, dtype, k, mode)
        want = t.expected(K)
        for B in BS:
            for fill in FILLS:
                poison.fill = fill
                what = f"{design} N={N} K={K} {dtype} k={k} {mode} B={B} {plan} fill {fill:#x}"
                _same(t.run(B, K, _flag(plan)), want, B, what)
                poison.check(what)
                n += 1
    return n


# N -> the fused kernel's range count S (p.fS of make_plan; pinned on the host
# by tests/test_workspace_contract.py): S = 1, 2, 3-4, 5-15, 16.  At 1,025 and
# 4,097 the last range holds one item: its lists are all empty keys.
FUSED_N = {1024: 1, 1025: 2, 4096: 4, 4097: 5, 16384: 16}
DENSE_OTHER = ("store", "gemm", "store+one_wave")     # at N = 1,025 and 16,384


def _small_params():
    out = []
    for N in FUSED_N:
        for dtype, k in CFGS:
            for mode in MODES:
                for design in DESIGNS:
                    out.append(pytest.param(design, N, dtype, k, mode,
                                            id=f"{design}-N{N}-{dtype}-k{k}-{mode}"))
    return out


@pytest.mark.parametrize("design,N,dtype,k,mode", _small_params())
def test_small_catalog_poisoned(poison, design, N, dtype, k, mode):
    """The fused kernel (PLAN_FUSED: the range lists, their empty keys, the
    arrival counter) at every S, and the score-matrix plans at N = 1,025 and
    16,384 (STORE leaves the threshold hints unset; the matrix's pad columns
    are scratch)."""
    from hhfm_amd._native import native
    p = native().debug_catalog_plan(130, N, k, 20, 0, 1 if dtype == "bf16" else 0)
    assert p["dense"] == 1 and p["fS"] == FUSED_N[N]
    plans = ("fused",) + (DENSE_OTHER if N in (1025, 16384) else ())
    assert _exact(poison, design, N, dtype, k, mode, plans) == \
        len(BS) * len(FILLS) * (3 + (len(KS) * 3 if N in (1025, 16384) else 0))


# streaming: 16,385 is the smallest catalog past the dense limit (31 splits of
# 17 tiles, no seed possible below 65,536 items); 65,536 the smallest with a
# threshold seed (4,096 items), where f32 k = 16 / bf16 k = 64 run catalog_main
# behind the seed and f32 k = 64 / bf16 k = 128 catalog_ring
def _stream_params():
    out = []
    for N, cfgs, plans, Ks in (
            (16385, CFGS, ("no_seed", "default"), KS),
            (65536, CFGS, ("default", "no_seed"), KS),
            (65536, RING_CFGS, ("ring", "ring_alt", "no_ring", "no_seed"), (1, 20, 32))):
        for dtype, k in cfgs:
            for mode in MODES:
                for design in DESIGNS:
                    out.append(pytest.param(design, N, dtype, k, mode, plans, Ks,
                                            id=f"{design}-N{N}-{dtype}-k{k}-{mode}"))
    return out


@pytest.mark.parametrize("design,N,dtype,k,mode,plans,Ks", _stream_params())
def test_streaming_poisoned(poison, design, N, dtype, k, mode, plans, Ks):
    """More than one item split on every path, so the partial lists, the
    per-query threshold hints (0x80 fill or the seed's K-th maximum), the
    seed's tile maxima and its top-K lists all live in poisoned scratch."""
    from hhfm_amd._native import native
    for B in BS:
        p = native().debug_catalog_plan(B, N, k, 20, 0, 1 if dtype == "bf16" else 0)
        assert p["dense"] == 0 and p["S"] > 1 and p["rS0"] > 1 and p["rS1"] > 1
        assert p["seed_n"] == (4096 if N == 65536 else 0)
    _exact(poison, design, N, dtype, k, mode, plans, Ks)


@pytest.mark.parametrize("plan", ["default", "store"])
def test_pooled_max_poisoned(poison, plan):
    """test_gpu_catalog_exact.test_pooled_max_exact's smallest case (periodic,
    4,082 items, K = 20, f32 k = 64): the fused kernel's POOL form (the default
    at this size) and catalog_queries over PoolFeature + STORE."""
    pooling = ("max", "sum", "sum")
    N, K, B = 4082, 20, 37
    t = _tables("periodic", N, K, "f32", 64, "hhfm", ctx_on_items=True)
    d = t.d
    h = pr.hybrid(d.E, d.A, d.ctx, (0, 0), pooling)
    scores = sd.scores_from_queries(h, np.zeros(len(h)), d.E, None, d.item_begin, N)
    want = sd.expected_topk(scores[:B], K)
    for fill in FILLS:
        poison.fill = fill
        _same(t.run(B, K, _plans()[plan], pooling=pooling), want, B, f"{plan} fill {fill:#x}")
        poison.check(f"pooled {plan} fill {fill:#x}")


# ---------------------------------------------------------------------------
# a. poisoned scratch — the other catalog forms, A/A
# ---------------------------------------------------------------------------
DENSE_N, STREAM_N = 777, 16385


def _hhfm_inputs(N, dtype="f32", k=64, seed=0):
    """130 queries (user, item, five context columns, three time columns) over
    a random table: no exact ties, so every plan's list is unique."""
    from tests.test_gpu_hhfm_pool import _rows
    rng = np.random.default_rng(1000 + N + seed)
    A, M = _rows(rng, 130, 300, N, (5, 4, 6, 3, 7), 3)
    E = _dev(rng.normal(0, 0.2, (M, k)).astype(np.float32))
    w = _dev(rng.normal(0, 0.1, M).astype(np.float32))
    return _dev(A), (E.to(torch.bfloat16) if dtype == "bf16" else E), w, M


def _form_calls():
    """name -> (builder of call(N, plan), the plans it runs).  Dense size 777
    (ragged last tile), streaming size 16,385, both where the form has both."""
    from hhfm_amd import ops

    def two_way(N, plan):
        q, E, _, _ = _hhfm_inputs(N)
        return lambda: ops.catalog_topk(q, E, ops.MODE_HHFM, 20, 300, N, 0, None, 0, (2, 7), (7, 10),
                                        plan=plan, pooling=("max", "mean", "sum"),
                                        pooling2=("mean", "sum", "max"))

    def excl(N, plan):
        q, E, w, _ = _hhfm_inputs(N, "bf16")
        rng = np.random.default_rng(N)
        # per query up to 40 catalog rows, some queries none, rows at both ends
        seqs = [sorted({300, 300 + N - 1} | set(rng.integers(300, 300 + N, b % 41).tolist()))
                if b % 5 else [] for b in range(130)]
        lists = ops.exclusion_lists(seqs, "cuda")
        return lambda: ops.catalog_topk(q, E, ops.MODE_FM, 20, 300, N, 0, w, 0, (2, 7), (0, 0),
                                        plan=plan, exclude=lists)

    def cars2(N, plan):
        from tests import cars2_ref as cr
        D, Mc = 64, 9
        Wt = cr.weights(N, 300 + N, Mc, D)
        prepared = ops.cars2_prepare(*(_dev(Wt[n]) for n in ("Context", "W", "Z", "A", "B")))
        rng = np.random.default_rng(N + 1)
        q = _dev(np.stack([rng.integers(0, 300, 130), rng.integers(0, Mc, 130)], 1).astype(np.int32))
        UI = _dev(Wt["UI"])
        return lambda: ops.cars2_catalog_topk(q, UI, prepared, Mc, 20, 300, N, 0, plan=plan)

    def noatt(N, plan):
        q, E, w, _ = _hhfm_inputs(N, k=16)
        P = _dev(np.random.default_rng(N + 2).normal(1, 0.2, 16).astype(np.float32))
        q5 = q[:, :5].contiguous()
        return lambda: ops.afm_noatt_catalog_topk(q5, E, w, 0.02, P, 300, N, 20, 0, plan=plan)

    dense = {"store": ops.PLAN_STORE, "gemm": ops.PLAN_GEMM, "default": 0}
    stream = {"default": 0, "no_seed": ops.PLAN_NO_SEED}
    return {"two_way": (two_way, dense, stream), "exclusion": (excl, dense, stream),
            "cars2": (cars2, dense, stream), "afm_noatt": (noatt, dense, stream)}


@pytest.mark.parametrize("path", ["dense", "stream"])
@pytest.mark.parametrize("form", ["two_way", "exclusion", "cars2", "afm_noatt"])
def test_catalog_forms_poisoned(poison, form, path):
    build, dense, stream = _form_calls()[form]
    N, plans = (DENSE_N, dense) if path == "dense" else (STREAM_N, stream)
    for name, plan in plans.items():
        _aa(poison, build(N, plan), f"{form} {path} {name}")


# ---------------------------------------------------------------------------
# a. DeepFM and AFM (ops._workspace), A/A
# ---------------------------------------------------------------------------
def _dfm(nu, ni, F, k, layers, mlp, table="f32", seed=0, deep_head=False):
    from hhfm_amd import ops
    rng = np.random.default_rng(seed + nu + ni + k)
    M = nu + ni + 12
    mdt = torch.float32 if mlp == "f32" else torch.bfloat16
    E = _dev(rng.normal(0, 0.1, (M, k)).astype(np.float32))
    if table == "bf16":
        E = E.to(torch.bfloat16)
    w = _dev(rng.normal(0, 0.01, M).astype(np.float32))
    Ls, Bs, kin = [], [], F * k
    for n in layers:
        Ls.append(_dev(rng.normal(0, (2.0 / (kin + n)) ** 0.5, (kin, n)).astype(np.float32)))
        Bs.append(_dev(rng.normal(0, 0.01, n).astype(np.float32)))
        kin = n
    Wt, bs, dims = ops.dfm_prepare_weights(Ls, Bs, mdt, F, k)
    nproj = layers[-1] if deep_head else F + k + layers[-1]
    Wp = _dev(rng.normal(0, 0.1, nproj).astype(np.float32))
    cols = [rng.integers(0, nu, 6000), rng.integers(nu, nu + ni, 6000),
            rng.integers(nu + ni, nu + ni + 7, 6000), rng.integers(nu + ni + 7, nu + ni + 9, 6000),
            rng.integers(nu + ni + 9, M, 6000)]
    X = _dev(np.stack(cols[:F], 1).astype(np.int32))
    return dict(E=E, w=w, Wt=Wt, bs=bs, dims=dims, mdt=mdt, Wp=Wp, bp=0.3, X=X, nu=nu, ni=ni, M=M)


@pytest.mark.parametrize("proj", [False, True, "ctx", "item"], ids=str)
@pytest.mark.parametrize("mlp", ["f32", "bf16"])
def test_dfm_catalog_poisoned(poison, mlp, proj):
    """test_dfm_catalog_topk_chunked's shape (37 queries x 700 items, k = 32,
    layers 64-48): one pass and two query chunks (19 + 18 queries), so the row
    ids, the score block, the packed weights and P are rewritten per chunk."""
    from hhfm_amd import ops
    m = _dfm(50, 700, 5, 32, [64, 48], mlp)
    q = m["X"][:37].contiguous()
    for chunk in (1 << 20, 19 * 700):
        _aa(poison, lambda: ops.dfm_catalog_topk(q, m["E"], m["w"], m["Wt"], m["bs"], m["dims"],
                                                 m["Wp"], m["bp"], 1, 50, 700, 20, 0, chunk,
                                                 proj=proj),
            f"dfm_catalog {mlp} proj={proj} chunk={chunk}")


def _dfm_forward_cases():
    from hhfm_amd import ops
    # (id, model arguments, rows, proj, plan): bf16 MLP at test_dfm_item_grouping's
    # smallest table (M = 997; "item" groups the rows by user: counting sort,
    # order and field ranges in the workspace); fp32 MLP at M = 82, where 6,000
    # rows reach the grouped split kernel (rows >= 64 M), and the same ungrouped
    bf = dict(nu=40, ni=945, F=5, k=64, layers=[150, 200, 150], mlp="bf16", table="bf16")
    f32 = dict(nu=20, ni=50, F=5, k=32, layers=[64, 48], mlp="f32")
    out = [(f"bf16-{p}", bf, 6000, p, 0) for p in (False, True, "ctx", "item")]
    out += [("f32-False", f32, 6000, False, 0), ("f32-True-grouped", f32, 6000, True, 0),
            ("f32-True-ungrouped", f32, 6000, True, ops.PLAN_UNGROUPED),
            ("f32-True-997rows", f32, 997, True, 0)]
    return out


@pytest.mark.parametrize("n", range(8))
def test_dfm_forward_poisoned(poison, n):
    from hhfm_amd import ops
    name, kw, rows, proj, plan = _dfm_forward_cases()[n]
    m = _dfm(**kw)
    X = m["X"][:rows].contiguous()
    _aa(poison, lambda: ops.dfm_forward(X, m["E"], m["w"], m["Wt"], m["bs"], m["dims"], m["mdt"],
                                        m["Wp"], m["bp"], proj=proj, plan=plan),
        f"dfm_forward {name}")


@pytest.mark.parametrize("mlp", ["f32", "bf16"])
def test_dfm_deep_head_poisoned(poison, mlp):
    """The deep-only head: its zero-prefixed projection lives in
    _head_ws_extra bytes after the plan (rows and catalog)."""
    from hhfm_amd import ops
    head = ops.DFM_HEAD_DEEP
    m = _dfm(50, 700, 5, 32, [64, 48], mlp, deep_head=True)
    assert ops._head_ws_extra(head, 5, 32, m["dims"]) > 0
    X, q = m["X"][:997].contiguous(), m["X"][:37].contiguous()
    _aa(poison, lambda: ops.dfm_forward(X, m["E"], m["w"], m["Wt"], m["bs"], m["dims"], m["mdt"],
                                        m["Wp"], m["bp"], proj=None, head=head),
        f"dfm_forward deep head {mlp}")
    _aa(poison, lambda: ops.dfm_catalog_topk(q, m["E"], m["w"], m["Wt"], m["bs"], m["dims"],
                                             m["Wp"], m["bp"], 1, 50, 700, 20, 0, 19 * 700,
                                             proj=None, head=head),
        f"dfm_catalog deep head {mlp}")


def _afm(F, k, A, nu=100, ni=900, table="f32", seed=0):
    rng = np.random.default_rng(seed + F * 100 + k + A)
    M = nu + ni + 12
    E = _dev(rng.normal(0, 0.1, (M, k)).astype(np.float32))
    if table == "bf16":
        E = E.to(torch.bfloat16)
    w = _dev(rng.normal(0, 0.01, M).astype(np.float32))
    Wt = _dev(rng.normal(0, (2.0 / (k + A)) ** 0.5, (A, k)).astype(np.float32))
    b = _dev(rng.normal(0, 0.1, A).astype(np.float32))
    p = _dev(rng.normal(0, 0.5, A).astype(np.float32))
    P = _dev(rng.normal(1, 0.2, k).astype(np.float32))
    cols = [rng.integers(0, nu, 700), rng.integers(nu, nu + ni, 700)]
    cols += [rng.integers(nu + ni, M, 700) for _ in range(F - 2)]
    X = _dev(np.stack(cols, 1).astype(np.int32))
    return dict(E=E, w=w, att=(Wt, b, p, P), X=X, nu=nu, ni=ni)


def _afm_plans():
    from hhfm_amd import ops
    return {"default": 0, "exact": ops.PLAN_EXACT_FP32, "gemm": ops.PLAN_GEMM,
            "per_field": ops.PLAN_PER_FIELD}


@pytest.mark.parametrize("plan", ["default", "exact", "gemm", "per_field"])
@pytest.mark.parametrize("F,k,A", [(5, 32, 32), (9, 32, 32)], ids=["F5", "F9"])
def test_afm_catalog_poisoned(poison, F, k, A, plan):
    """test_afm_catalog_query_chunks's shape (33 queries x 900 items) in one
    pass and in two query chunks (17 + 16); F = 9 lies outside the fused
    envelope: W'', D and the logit partials go through the workspace under
    every plan."""
    from hhfm_amd import ops
    m = _afm(F, k, A)
    q = m["X"][:33].contiguous()
    for max_cols in (1 << 17, 17 * (F - 1) * A):
        _aa(poison, lambda: ops.afm_catalog_topk(q, m["E"], m["w"], *m["att"], m["nu"], m["ni"], 20,
                                                 0, max_cols, plan=_afm_plans()[plan]),
            f"afm_catalog F={F} {plan} max_cols={max_cols}")


@pytest.mark.parametrize("plan", ["default", "exact", "gemm", "per_field"])
@pytest.mark.parametrize("F,k,A,table", [(5, 32, 32, "f32"), (9, 32, 32, "f32"),
                                         (5, 20, 16, "f32"), (16, 32, 48, "bf16")],
                         ids=["F5-fused", "F9-gemm", "k20-gemm", "F16-bf16-gemm"])
def test_afm_forward_poisoned(poison, F, k, A, table, plan):
    """The fused row kernels touch no workspace; past their envelope (more
    than 32 pairs, or k % 8 != 0) the logit partials of the pair GEMM do."""
    from hhfm_amd import ops
    m = _afm(F, k, A, table=table)
    _aa(poison, lambda: ops.afm_forward(m["X"], m["E"], m["w"], 0.1, *m["att"],
                                        plan=_afm_plans()[plan]),
        f"afm_forward F={F} k={k} {plan}")


# ---------------------------------------------------------------------------
# a. pf_exclusion_lists and the device sampler
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("keep_own", [False, True])
def test_pf_exclusion_lists_poisoned(poison, keep_own):
    """test_gpu_topk_excl's split: A/A and the dict-built host lists."""
    from hhfm_amd import harness, ops
    from tests.test_gpu_topk_excl import _frappe_split
    rng = np.random.default_rng(9)
    pf, X, M = _frappe_split(rng)
    rows = X[rng.integers(0, len(X), 1500)].copy()
    rows[::7, 0] = M + 5
    dp = harness.DevicePairSet(pf, rows.shape[1] - 1, torch.device("cuda", 0))
    r = _dev(rows.astype(np.int32))
    ptr, flat = _aa(poison, lambda: ops.pf_exclusion_lists(dp.keys, dp.codes, r, 1,
                                                          keep_own=keep_own),
                    f"pf_exclusion_lists keep_own={keep_own}")
    wptr, wflat, _ = xr.csr(xr.lists_from_pf(pf, rows, 1, keep_own))
    assert np.array_equal(ptr, wptr) and np.array_equal(flat, wflat)


# (seed, negatives per row): 12,000 and 3,000 entries.  At 97 % cover ~11,600 of
# the 12,000 are rejected and take ~33 draws each: a dozen re-draw blocks of
# 1,024 entries and several generation rounds that slide the MT window.
SAMPLER_DRAWS = ((1, 4), (2, 1))


@functools.lru_cache(maxsize=None)
def _sampler_reference(n_item, cover):
    """The heavy-rejection split of tests/test_gpu_harness.py and, once for
    every user of it, the host harness's samples and generator state."""
    from hhfm_amd import harness
    from tests.test_gpu_harness import _PF
    rng = np.random.default_rng(n_item)
    n_user, ncols = 40, 4
    keys = [tuple(int(v) for v in rng.integers(0, 50, ncols - 1)) for _ in range(60)]
    pf = {}
    for key in keys:
        n_pos = min(int(cover * n_item), n_item - 1)
        pf[key] = set(int(n_user + i) for i in rng.choice(n_item, n_pos, replace=False))
    rows = []
    for _ in range(3000):
        key = keys[rng.integers(0, len(keys))] if rng.random() < 0.9 else (99, 99, 99)
        rows.append([key[0], n_user, key[1], key[2]])
    X = np.asarray(rows, dtype=np.int64)
    data = _PF(pf, n_user, n_item)
    host = harness.Train(data=data, model=None)
    want = {}
    for seed, num in SAMPLER_DRAWS:
        np.random.seed(seed)
        samples = host.sample_negative(X, num)
        want[seed, num] = (samples, np.random.get_state())
    return data, X, n_user, want


@pytest.mark.parametrize("bitmaps", [True, False])
@pytest.mark.parametrize("n_item,cover", [(65, 0.5), (1000, 0.97)])
def test_sample_negative_poisoned(poison, n_item, cover, bitmaps, monkeypatch):
    """test_sample_negative_on_device_heavy_rejection's catalogs of 2^k + 1
    items and of long re-draw chains with the sampler's own buffer poisoned:
    samples and generator state equal the host harness's, which is what
    tests/test_gpu_harness._both requires."""
    from hhfm_amd import harness
    from hhfm_amd._native import native
    from tests.test_gpu_harness import DeviceOracleModel, _state_eq
    monkeypatch.setattr(harness, "SAMPLER_BITMAPS", bitmaps)
    data, X, n_user, want = _sampler_reference(n_item, cover)
    devt = harness.Train(data=data, model=DeviceOracleModel(None, None, n_user, n_item))
    dev = devt._device()
    nkeys = devt._device_pairs(dev, X.shape[1] - 1).n
    nat = native()
    for fill in FILLS:
        for seed, num in SAMPLER_DRAWS:
            nbytes = (nat.sample_negative_workspace_ex(len(X), num, n_user, n_user + n_item, nkeys)
                      if bitmaps else nat.sample_negative_workspace(len(X), num))
            ws = poison.poisoned(nbytes, dev, fill)
            devt._sampler_bufs = {"dev": dev, "ws": ws,
                                  "state": torch.empty(625, dtype=torch.int32, pin_memory=True)}
            np.random.seed(seed)
            got = devt.sample_negative(X, num)
            state = np.random.get_state()
            assert devt._sampler_bufs["ws"] is ws                 # the poisoned one was used
            poison.check(f"sampler fill {fill:#x} num {num}")
            samples, host_state = want[seed, num]
            assert got.dtype == samples.dtype and got.shape == samples.shape
            assert np.array_equal(got, samples), int((got != samples).sum())
            assert _state_eq(host_state, state), (host_state[2], state[2])


# ---------------------------------------------------------------------------
# b. the prefix is never written by the plans that keep no counters there
# ---------------------------------------------------------------------------
def test_other_plans_leave_the_prefix_zero(poison):
    """STORE, GEMM, the streaming plans and the forms that never take the
    fused kernel, on zero workspaces: the prefix is still all zero.  (Every
    poisoned case above checks the same after its call; the host side,
    tests/test_workspace_contract.py, holds make_plan's offsets to it.)"""
    poison.fill = 0
    ran = 0
    for plan, N, dtype, k, K in (("store", 1025, "f32", 16, 20), ("gemm", 16384, "bf16", 64, 64),
                                 ("store+one_wave", 16384, "f32", 16, 33),
                                 ("no_seed", 16385, "bf16", 64, 20), ("default", 65536, "f32", 16, 64),
                                 ("default", 65536, "bf16", 128, 32), ("ring_alt", 65536, "f32", 64, 20),
                                 ("no_ring", 65536, "bf16", 128, 20)):
        for mode in MODES:
            t = _tables("ascending", N, K, dtype, k, mode)
            _same(t.run(130, K, _plans()[plan]), t.expected(K), 130, plan)
            assert len(poison.cat) == 1
            poison.check(f"{plan} N={N} {mode}")
            ran += 1
    for form, (build, dense, stream) in _form_calls().items():
        for N, plans in ((DENSE_N, dense), (STREAM_N, stream)):
            for name, plan in plans.items():
                build(N, plan)()
                assert len(poison.cat) == 1
                poison.check(f"{form} {name} N={N}")
                ran += 1
    assert ran == 16 + 4 * 5


# ---------------------------------------------------------------------------
# c. one workspace, many calls
# ---------------------------------------------------------------------------
# (design, N, K, dtype, k, mode, B, plan) in running order; the design changes
# between any two consecutive calls, so a stale list is a wrong answer
CATALOG_SEQUENCE = [
    # S shrinks 16 -> 5 -> 2 -> 1 at the same five query groups
    ("ascending", 16384, 32, "f32", 16, "hhfm", 130, "fused"),
    ("all_equal", 4097, 32, "f32", 16, "hhfm", 130, "fused"),
    ("plateau_Kp1", 1025, 32, "f32", 16, "hhfm", 130, "fused"),
    ("one_per_split", 1024, 32, "f32", 16, "hhfm", 130, "fused"),
    # B shrinks 130 -> 33 -> 1 at S = 5 (FM, bf16): stale groups behind it
    ("ascending", 4097, 20, "bf16", 64, "fm", 130, "fused"),
    ("all_equal", 4097, 20, "bf16", 64, "fm", 33, "fused"),
    ("plateau_Kp1", 4097, 20, "bf16", 64, "fm", 1, "fused"),
    # K changes
    ("one_per_split", 4096, 1, "bf16", 64, "hhfm", 33, "fused"),
    ("ascending", 4096, 32, "bf16", 64, "hhfm", 33, "fused"),
    # a fused call after STORE / GEMM: the score matrix lay over the list region
    ("all_equal", 16384, 64, "f32", 16, "fm", 130, "store"),
    ("plateau_Kp1", 16384, 20, "f32", 16, "fm", 130, "fused"),
    ("ascending", 16384, 33, "bf16", 64, "hhfm", 130, "gemm"),
    ("one_per_split", 16384, 20, "bf16", 64, "hhfm", 130, "fused"),
    ("all_equal", 1025, 20, "f32", 16, "hhfm", 32, "store+one_wave"),
    ("ascending", 1025, 20, "f32", 16, "hhfm", 32, "fused"),
    # a fused call after a streaming one (unseeded, ring, seeded catalog_main)
    ("plateau_Kp1", 16385, 20, "f32", 16, "fm", 130, "no_seed"),
    ("ascending", 4097, 20, "f32", 16, "fm", 130, "fused"),
    ("all_equal", 65536, 32, "bf16", 128, "hhfm", 130, "default"),
    ("one_per_split", 4097, 32, "bf16", 64, "hhfm", 130, "fused"),
    ("ascending", 65536, 20, "f32", 64, "fm", 33, "ring_alt"),
    ("plateau_Kp1", 16384, 20, "f32", 16, "fm", 33, "fused"),
    ("all_equal", 65536, 64, "bf16", 64, "fm", 130, "default"),
    ("ascending", 1025, 1, "bf16", 64, "fm", 130, "fused"),
    ("one_per_split", 65536, 20, "bf16", 128, "fm", 1, "no_ring"),
    ("plateau_Kp1", 4096, 20, "f32", 16, "hhfm", 1, "fused"),
    # streaming after fused, and back
    ("all_equal", 16385, 33, "bf16", 64, "hhfm", 33, "default"),
    ("ascending", 1024, 20, "f32", 16, "fm", 130, "fused"),
    ("one_per_split", 16384, 32, "f32", 16, "hhfm", 1, "fused"),
]


@pytest.mark.parametrize("first", [0, gt.POISON_FF, gt.POISON_7F], ids=["zero", "ff", "7f"])
def test_one_catalog_workspace_many_calls(poison, first):
    """One workspace sized for the largest call, written once (prefix zero, the
    rest zero or a poison) and never again: every call of the list returns its
    exact list and leaves the prefix zero."""
    from hhfm_amd._native import native
    seq = CATALOG_SEQUENCE
    assert len(seq) >= 24 and all(a[0] != b[0] for a, b in zip(seq, seq[1:]))
    nat = native()
    poison.hold("catalog", max(nat.catalog_topk_workspace(B, N, k, K)
                               for _, N, K, _, k, _, B, _ in seq), first)
    for n, (design, N, K, dtype, k, mode, B, plan) in enumerate(seq):
        t = _tables(design, N, K, dtype, k, mode)
        what = f"call {n}: {design} N={N} K={K} {dtype} k={k} {mode} B={B} {plan}"
        _same(t.run(B, K, _plans()[plan]), t.expected(K), B, what)
        assert poison.cat and poison.cat[-1] is poison.held["catalog"]
        poison.check(what)


@pytest.mark.parametrize("first", [0, gt.POISON_FF, gt.POISON_7F], ids=["zero", "ff", "7f"])
def test_one_scratch_workspace_many_calls(poison, first):
    """DeepFM, AFM and exclusion-list calls interleaved on one buffer: each
    equals its own result on a fresh zero workspace, whatever the call before
    it left behind."""
    from hhfm_amd import harness, ops
    from tests.test_gpu_topk_excl import _frappe_split
    d32 = _dfm(50, 700, 5, 32, [64, 48], "f32")
    dbf = _dfm(40, 945, 5, 64, [150, 200, 150], "bf16", table="bf16")
    a5, a9 = _afm(5, 32, 32), _afm(9, 32, 32)
    rng = np.random.default_rng(9)
    pf, X, _ = _frappe_split(rng)
    dp = harness.DevicePairSet(pf, X.shape[1] - 1, torch.device("cuda", 0))
    r = _dev(X[:1500].astype(np.int32))
    q32, qbf = d32["X"][:37].contiguous(), dbf["X"][:6000].contiguous()
    q5, q9 = a5["X"][:33].contiguous(), a9["X"][:33].contiguous()

    def dfm_cat(m, q, chunk, proj):
        return lambda: ops.dfm_catalog_topk(q, m["E"], m["w"], m["Wt"], m["bs"], m["dims"], m["Wp"],
                                            m["bp"], 1, m["nu"], m["ni"], 20, 0, chunk, proj=proj)

    def dfm_fwd(m, X_, proj):
        return lambda: ops.dfm_forward(X_, m["E"], m["w"], m["Wt"], m["bs"], m["dims"], m["mdt"],
                                       m["Wp"], m["bp"], proj=proj)

    def afm_cat(m, q, plan, max_cols=1 << 17):
        return lambda: ops.afm_catalog_topk(q, m["E"], m["w"], *m["att"], m["nu"], m["ni"], 20, 0,
                                            max_cols, plan=plan)

    calls = {
        "dfm_cat_f32_proj": dfm_cat(d32, q32, 1 << 20, True),
        "dfm_cat_f32_chunks": dfm_cat(d32, q32, 19 * 700, False),
        "dfm_fwd_bf16_item": dfm_fwd(dbf, qbf, "item"),
        "dfm_fwd_bf16_ctx": dfm_fwd(dbf, qbf, "ctx"),
        "dfm_fwd_f32": dfm_fwd(d32, d32["X"][:997].contiguous(), True),
        "afm_cat_fused": afm_cat(a5, q5, 0),
        "afm_cat_gemm": afm_cat(a5, q5, ops.PLAN_GEMM, 17 * 4 * 32),
        "afm_cat_F9": afm_cat(a9, q9, 0),
        "afm_fwd_F9": lambda: ops.afm_forward(a9["X"], a9["E"], a9["w"], 0.1, *a9["att"]),
        "pf_excl": lambda: ops.pf_exclusion_lists(dp.keys, dp.codes, r, 1),
    }
    order = ["dfm_fwd_bf16_item", "afm_cat_gemm", "dfm_cat_f32_proj", "pf_excl", "afm_fwd_F9",
             "dfm_cat_f32_chunks", "afm_cat_fused", "dfm_fwd_bf16_ctx", "pf_excl", "afm_cat_F9",
             "dfm_fwd_f32", "afm_cat_gemm", "dfm_fwd_bf16_item", "afm_fwd_F9", "dfm_cat_f32_proj",
             "afm_cat_F9", "dfm_cat_f32_chunks", "pf_excl", "dfm_fwd_f32", "afm_cat_fused",
             "dfm_fwd_bf16_ctx", "afm_cat_gemm", "dfm_cat_f32_proj", "dfm_fwd_bf16_item"]
    assert len(order) >= 24 and set(order) == set(calls)
    # each call's result, and the largest size any of them queries, on fresh zero workspaces
    poison.fill = 0
    want = {name: _snap(call()) for name, call in calls.items()}
    sizes = list(poison.sizes)
    poison.check("baselines")
    poison.hold("scratch", max(max(sizes), 256), first)
    for n, name in enumerate(order):
        got = _snap(calls[name]())
        poison.check(f"call {n}: {name}")
        assert _equal(got, want[name]), f"call {n} ({name}) depends on what ran before it"
