"""K2 top-K on designed scores: exact ids and exact score bits on every path.

tests/score_designs.py builds tables whose catalog scores are integers that
every arithmetic of the kernels reproduces bit for bit (proved for the
reference alone in tests/test_score_designs.py), so the expected list —
a stable argsort, tf.nn.top_k order — is unique.  Every assertion here is
np.array_equal on int32 ids and on the float32 scores viewed as int32; there
is no tolerance and no tie allowance.  Plans are not compared pairwise: each
one is held to the same expected list, so they agree bit for bit.

Case ids read  design-N-K-dtype-k-mode-B-plan.  The full product of the
parameters would be tens of thousands of launches; one primary configuration
per path runs every design x K x plan, the others a rotating share chosen by
index arithmetic (never by a result), so that every (configuration, plan),
(design, K) and (design, plan) pair runs at least once.
"""
import numpy as np
import pytest
import torch

from tests import hhfm_pool_ref as pr
from tests import score_designs as sd

pytestmark = pytest.mark.gpu

BMAX = 130
MODES = ("hhfm", "fm")
# name -> (design, spikes relative to K or None, in_w, outside_seed)
DESIGNS = {
    "all_equal": ("all_equal", None, False, False),
    "plateau_Km1": ("plateau_spikes", -1, False, False),
    "plateau_K": ("plateau_spikes", 0, False, False),
    "plateau_Kp1": ("plateau_spikes", 1, False, False),
    "plateau_3": ("plateau_spikes", "3", False, False),
    "plateau_Kp1_tail": ("plateau_spikes", 1, False, True),     # spikes outside the seed only
    "ascending": ("ascending", None, False, False),
    "periodic": ("periodic", None, False, False),
    "one_per_split": ("one_per_split", None, False, False),
    "w_only_plateau_Kp1": ("plateau_spikes", 1, True, False),   # FM: the pattern in w, v = 0
    "w_only_ascending": ("ascending", None, True, False),
}


def _designs(mode, seeded=False):
    return [n for n, d in DESIGNS.items()
            if (mode == "fm" or not d[2]) and (seeded or not d[3])]


def _plans():
    from hhfm_amd import ops
    return {"default": 0, "exact": ops.PLAN_EXACT_FP32, "fused": ops.PLAN_FUSED,
            "fused+exact": ops.PLAN_FUSED | ops.PLAN_EXACT_FP32, "store": ops.PLAN_STORE,
            "store+exact": ops.PLAN_STORE | ops.PLAN_EXACT_FP32, "gemm": ops.PLAN_GEMM,
            "gemm+exact": ops.PLAN_GEMM | ops.PLAN_EXACT_FP32,
            "store+one_wave": ops.PLAN_STORE | ops.PLAN_ONE_WAVE,
            "store+one_wave+exact": ops.PLAN_STORE | ops.PLAN_ONE_WAVE | ops.PLAN_EXACT_FP32,
            "ring_alt": ops.PLAN_RING_ALT, "no_ring": ops.PLAN_NO_RING,
            "no_seed": ops.PLAN_NO_SEED}


# ---------------------------------------------------------------------------
# tables: one design on the device at a time; B <= BMAX queries are the first
# rows of one 130-query design, expected lists are kept per (K, shard)
# ---------------------------------------------------------------------------
_CACHE = {}


class _Tables:
    def __init__(self, name, N, K, dtype, k, mode, sentinels=None, ctx_on_items=False, n_ctx=2):
        design, rel, in_w, tail = DESIGNS[name]
        m = None if rel is None else (3 if rel == "3" else K + rel)
        self.d = sd.make(design, N, k, dtype, mode, B=BMAX, K=K, m=m, in_w=in_w,
                         outside_seed=tail, sentinels=sentinels, ctx_on_items=ctx_on_items,
                         n_ctx=n_ctx)
        self.mode = mode
        self.A = torch.from_numpy(self.d.A).cuda()
        E = torch.from_numpy(self.d.E).cuda()
        self.E = E.to(torch.bfloat16) if dtype == "bf16" else E
        self.w = None if self.d.w is None else torch.from_numpy(self.d.w).cuda()
        self.scores = self.d.scores
        self.exp = {}

    def expected(self, K, lo=0, cnt=None, gbase=0):
        key = (K, lo, cnt, gbase)
        if key not in self.exp:
            self.exp[key] = sd.expected_topk(self.scores, K, lo, cnt, gbase)
        return self.exp[key]

    def run(self, B, K, plan, lo=0, cnt=None, gbase=0, pooling=None):
        from hhfm_amd import ops
        d = self.d
        s, i = ops.catalog_topk(self.A[:B].contiguous(), self.E,
                                ops.MODE_FM if self.mode == "fm" else ops.MODE_HHFM, K,
                                d.item_begin + lo, d.N - lo if cnt is None else cnt, gbase,
                                self.w, 0, d.ctx, (0, 0), plan=plan, pooling=pooling)
        return s, i


def _tables(name, N, K, dtype, k, mode, **kw):
    design, rel, _, _ = DESIGNS[name]
    kdep = rel not in (None, "3") or design == "one_per_split"
    key = (name, N, K if kdep else 0, dtype, k, mode, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = _Tables(name, N, K, dtype, k, mode, **kw)
    return _CACHE[key]


def _same(got, want, B, what=""):
    gs, gi = (x.cpu().numpy() for x in got)
    ws, wi = want[0][:B], want[1][:B]
    if not np.array_equal(gi, wi):
        b, p = np.argwhere(gi != wi)[0]
        raise AssertionError(f"{what}: ids differ at {int((gi != wi).sum())} positions; first "
                             f"query {b} rank {p}: got {gi[b, p]} ({gs[b, p]}), "
                             f"expected {wi[b, p]} ({ws[b, p]})")
    assert np.array_equal(sd.bits(gs), sd.bits(ws)), f"{what}: score bits differ"


def _cid(design, N, K, dtype, k, mode, B, plan):
    return f"{design}-N{N}-K{K}-{dtype}-k{k}-{mode}-B{B}-{plan}"


def _order(cases):
    """Cases that share tables side by side (one design lives on the device)."""
    return sorted(cases, key=lambda c: (c[1], c[3], c[4], c[5], c[0], c[2], c[6], c[7]))


def _params(cases):
    return [pytest.param(*c, id=_cid(*c)) for c in _order(cases)]


# ---------------------------------------------------------------------------
# small path: N <= 16,384 (fused kernel, STORE / GEMM score matrix + topk_dense)
# ---------------------------------------------------------------------------
def _small_cases():
    cfgs = [(N, dt, k, mode, B) for N in (4082, 16384)
            for dt, k in (("f32", 64), ("f32", 16), ("bf16", 16), ("bf16", 64))
            for mode in ("fm", "hhfm") for B in (37, 1)]
    plans = ["fused", "fused+exact", "store", "store+exact", "gemm", "gemm+exact",
             "store+one_wave", "store+one_wave+exact"]
    out = []
    for ci, (N, dt, k, mode, B) in enumerate(cfgs):
        for di, name in enumerate(_designs(mode)):
            if ci and (ci + di) % 4:
                continue
            for ki, K in enumerate((1, 20, 32, 33, 64)):
                for pi, plan in enumerate(plans):
                    if K > 32 and plan.startswith("fused"):
                        continue    # the fused kernel takes K <= 32
                    if ci and (ci + ki + pi) % 4:
                        continue
                    out.append((name, N, K, dt, k, mode, B, plan))
    return out


@pytest.mark.parametrize("design,N,K,dtype,k,mode,B,plan", _params(_small_cases()))
def test_small_catalog_exact(design, N, K, dtype, k, mode, B, plan):
    t = _tables(design, N, K, dtype, k, mode)
    _same(t.run(B, K, _plans()[plan]), t.expected(K), B)


# ---------------------------------------------------------------------------
# streaming, unseeded: N = 20,011 (catalog_main from -inf, 37 splits of 544
# items + merge; all_equal / periodic / plateau_Kp1 keep its dense
# sort-and-merge branch busy past the warm-up)
# ---------------------------------------------------------------------------
def _unseeded_cases():
    cfgs = [(dt, k, mode, B) for dt, k in (("f32", 64), ("f32", 16), ("f32", 128), ("bf16", 64),
                                           ("bf16", 128))
            for mode in ("fm", "hhfm") for B in (130, 37, 1)]
    out = []
    for ci, (dt, k, mode, B) in enumerate(cfgs):
        for di, name in enumerate(_designs(mode)):
            if ci and (ci + di) % 4:
                continue
            for ki, K in enumerate((1, 20, 32, 33, 64)):
                for pi, plan in enumerate(("default", "exact")):
                    if ci and (ci + ki + pi) % 2:
                        continue
                    out.append((name, 20011, K, dt, k, mode, B, plan))
    return out


@pytest.mark.parametrize("design,N,K,dtype,k,mode,B,plan", _params(_unseeded_cases()))
def test_streaming_unseeded_exact(design, N, K, dtype, k, mode, B, plan):
    t = _tables(design, N, K, dtype, k, mode)
    _same(t.run(B, K, _plans()[plan]), t.expected(K), B)


# ---------------------------------------------------------------------------
# streaming, seeded: N = 65,549 (seed over the first 4,096 items; ring kernel
# at both workgroup sizes, catalog_main behind the seed, no seed, fp32 MFMA)
# ---------------------------------------------------------------------------
def _seeded_cases():
    ring_plans = ("default", "ring_alt", "no_ring", "no_seed", "exact")
    cfgs = [(dt, k, mode, B) for dt, k in (("f32", 64), ("bf16", 128), ("bf16", 64))
            for mode in ("hhfm", "fm") for B in (130, 37)]
    out = []
    for ci, (dt, k, mode, B) in enumerate(cfgs):
        ring = (dt, k) != ("bf16", 64)
        for di, name in enumerate(_designs(mode, seeded=True)):
            if ci and (ci + di) % 3:
                continue
            # K = 64 (and bf16 k = 64 at every K): catalog_main behind the seed
            combos = [(K, p) for K in (1, 20, 32) for p in (ring_plans if ring else
                                                            ("default", "no_seed"))]
            combos += [(64, "default"), (64, "no_seed")]
            for xi, (K, plan) in enumerate(combos):
                if ci and (ci + xi) % 2:
                    continue
                out.append((name, 65549, K, dt, k, mode, B, plan))
    return out


@pytest.mark.parametrize("design,N,K,dtype,k,mode,B,plan", _params(_seeded_cases()))
def test_streaming_seeded_exact(design, N, K, dtype, k, mode, B, plan):
    t = _tables(design, N, K, dtype, k, mode)
    _same(t.run(B, K, _plans()[plan]), t.expected(K), B)


# ---------------------------------------------------------------------------
# shards and merge
# ---------------------------------------------------------------------------
_SHARD_CASES = [(name, N, K, dt, k, mode, 37, plan)
                for xi, (N, dt, k, plan) in enumerate([
                    (4082, "f32", 64, "default"), (16384, "bf16", 64, "store"),
                    (65549, "f32", 64, "default"), (65549, "bf16", 128, "default"),
                    (65549, "bf16", 128, "no_ring")])
                for mi, mode in enumerate(MODES)
                for di, (name, K) in enumerate([("periodic", 20), ("plateau_Kp1", 32),
                                                ("ascending", 20), ("all_equal", 1)])
                if (xi + mi + di) % 2 == 0 or N == 65549 and dt == "f32"]


@pytest.mark.parametrize("design,N,K,dtype,k,mode,B,plan", _params(_SHARD_CASES))
def test_ragged_shards_and_merge_exact(design, N, K, dtype, k, mode, B, plan):
    """R = 3 ragged shards (counts no multiples of 32, nonzero row and global
    bases) of an item range with the largest scores planted just outside it:
    every shard returns the expected list of its range — its neighbours' best
    items sit right at its edges —, and the device and host merges return the
    unsharded call's list, the expected one."""
    from hhfm_amd import ops
    lo0, total, G0 = 1021, N - 1021 - 777, 500_000
    t = _tables(design, N, K, dtype, k, mode, sentinels=(lo0, total))
    plan = _plans()[plan]
    parts_s, parts_i = [], []
    for lo, cnt in sd.ragged_shards(lo0, total):
        g = G0 + lo - lo0
        got = t.run(B, K, plan, lo, cnt, g)
        _same(got, t.expected(K, lo, cnt, g), B, f"shard [{lo}, {lo + cnt})")
        parts_s.append(got[0])
        parts_i.append(got[1])
    want = t.expected(K, lo0, total, G0)
    _same(t.run(B, K, plan, lo0, total, G0), want, B, "unsharded")
    S, I = torch.stack(parts_s), torch.stack(parts_i)
    _same(ops.topk_merge(S, I), want, B, "device merge")
    _same(ops.topk_merge(S.cpu(), I.cpu()), want, B, "host merge")


# ---------------------------------------------------------------------------
# pooled form: MAX context pooling (integer rows: exact; MEAN divides, left out)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("design,N,K,dtype,k,plan", [
    ("periodic", 4082, 20, "f32", 64, "default"), ("plateau_Kp1", 4082, 32, "bf16", 64, "store"),
    ("plateau_Kp1", 65549, 20, "f32", 64, "default"), ("periodic", 65549, 20, "bf16", 128, "default"),
    ("all_equal", 65549, 32, "bf16", 128, "no_ring"), ("periodic", 65549, 64, "bf16", 64, "default")],
    ids=lambda v: str(v))
def test_pooled_max_exact(design, N, K, dtype, k, plan):
    """hhfm_catalog_topk_pool with h = user + max(context rows): the context
    rows hold -1 / 0 / +1 on the item dimensions, so the maximum decides the
    ranking's direction per query; the reference scores come from the query
    vector of tests/hhfm_pool_ref.py."""
    pooling = ("max", "sum", "sum")
    t = _tables(design, N, K, dtype, k, "hhfm", ctx_on_items=True)
    d = t.d
    h = pr.hybrid(d.E, d.A, d.ctx, (0, 0), pooling)
    scores = sd.scores_from_queries(h, np.zeros(len(h)), d.E, None, d.item_begin, N)
    assert len({tuple(r) for r in np.sign(h[:, :3])}) >= 3      # both directions and zero
    B = 37
    _same(t.run(B, K, _plans()[plan], pooling=pooling), sd.expected_topk(scores[:B], K), B)
    lo, cnt, g = 1021, N - 2000 - 3, 77
    _same(t.run(B, K, _plans()[plan], lo, cnt, g, pooling=pooling),
          sd.expected_topk(scores[:B], K, lo, cnt, g), B, "shard")


# ---------------------------------------------------------------------------
# topk_dense on hand-made matrices
# ---------------------------------------------------------------------------
_FMAX = np.finfo(np.float32).max
_TINY = np.float32(1e-45)      # the smallest denormal


def _dense_rows(B, N):
    """Rows of special values, cycling through eight kinds."""
    rng = np.random.default_rng(N)
    S = np.empty((B, N), np.float32)
    specials = np.array([0.0, -0.0, -np.inf, _TINY, -_TINY, 1e-40, -1e-40, _FMAX, -_FMAX, 1.0,
                         -1.0], np.float32)
    i = np.arange(N)
    for b in range(B):
        kind = b % 8
        if kind == 0:       # everything at once, and one +inf
            S[b] = specials[rng.integers(0, len(specials), N)]
            S[b, rng.integers(0, N)] = np.inf
        elif kind == 1:     # the two zeros tie: ids decide, sign bits stay
            S[b] = np.where(rng.integers(0, 2, N) == 1, -0.0, 0.0)
        elif kind == 2:     # fewer finite scores than any K > 5: real -inf items fill the list
            S[b] = -np.inf
            S[b, rng.permutation(N)[:5]] = [3, -_FMAX, 0.0, -0.0, _TINY][:min(N, 5)]
        elif kind == 3:
            S[b] = 1.0
        elif kind == 4:
            S[b] = i
        elif kind == 5:
            S[b] = i % 7
        elif kind == 6:     # denormals and zeros only
            S[b] = specials[[0, 1, 3, 4, 5, 6]][rng.integers(0, 6, N)]
        else:               # descending: the first chunk holds the answer
            S[b] = -i.astype(np.float32)
    return S


@pytest.mark.parametrize("ld", ["tight", "padded"])
@pytest.mark.parametrize("B", [1, 5, 1030])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097])
def test_topk_dense_special_values_exact(N, B, ld):
    """hhfm_topk_dense, one wave and four waves per query (N >= 1,024 and B <=
    1,024 take four), on +-0, -inf, denormals, +-FLT_MAX and +inf, at the 64 /
    2,048-score chunk and four-wave span boundaries; "padded" reads a column
    slice of a wider matrix whose pad columns hold NaN and +inf."""
    from hhfm_amd import ops
    S = _dense_rows(B, N)
    if ld == "padded":
        wide = np.empty((B, N + 5), np.float32)
        wide[:, :N] = S
        wide[:, N:] = [np.nan, np.inf, np.nan, _FMAX, np.inf]
        Sd = torch.from_numpy(wide).cuda()[:, :N]
    else:
        Sd = torch.from_numpy(S).cuda()
    for K in sorted({1, min(N, 64)}):
        want = sd.expected_topk(S, K, gbase=11)
        for plan in (0, ops.PLAN_ONE_WAVE):
            _same(ops.topk_dense(Sd, K, 11, plan=plan), want, B, f"K={K} plan={plan}")
