"""The designed-score generator (tests/score_designs.py) on the CPU.

The GPU module compares with zero tolerance, which is sound only if the
reference's float32 scores do not depend on how they are summed.  That is
checked here for the reference alone, then the C oracle and the host merge
are held to the same expected lists.
"""
import numpy as np
import pytest
import torch

from oracle.parity import bf16_round
from tests import score_designs as sd

F32 = np.float32

# (design, kwargs of make) — every design of the GPU module, both table dtypes
# and modes, the hi/lo pair form (bf16 ascending) and the largest catalog
DESIGNS = [
    ("all_equal", dict(N=20011, k=16, dtype="f32", mode="hhfm")),
    ("all_equal", dict(N=4082, k=64, dtype="bf16", mode="fm")),
    ("plateau_spikes", dict(N=65549, k=64, dtype="f32", mode="hhfm", m=21)),
    ("plateau_spikes", dict(N=65549, k=128, dtype="bf16", mode="fm", m=19, outside_seed=True)),
    ("plateau_spikes", dict(N=20011, k=64, dtype="bf16", mode="hhfm", m=3)),
    ("ascending", dict(N=65549, k=64, dtype="f32", mode="hhfm")),
    ("ascending", dict(N=65549, k=128, dtype="bf16", mode="fm")),
    ("ascending", dict(N=20011, k=128, dtype="f32", mode="fm", in_w=True)),
    ("periodic", dict(N=20011, k=128, dtype="bf16", mode="hhfm", n_ctx=0)),
    ("periodic", dict(N=16384, k=16, dtype="f32", mode="fm", in_w=True)),
    ("one_per_split", dict(N=20011, k=64, dtype="f32", mode="fm", K=32)),
    ("one_per_split", dict(N=65549, k=64, dtype="bf16", mode="hhfm", K=20)),
    ("periodic", dict(N=65549, k=64, dtype="f32", mode="hhfm", sentinels=(4100, 50001))),
    ("plateau_spikes", dict(N=4082, k=64, dtype="f32", mode="hhfm", ctx_on_items=True)),
    # the sizes of tests/test_gpu_workspace_contract.py: the fused kernel's range
    # counts (1,024 .. 16,384), the smallest streaming (16,385) and seeded (65,536) catalogs
    ("plateau_spikes", dict(N=1024, k=16, dtype="f32", mode="fm", m=33)),
    ("plateau_spikes", dict(N=1025, k=64, dtype="bf16", mode="hhfm", m=65)),
    ("one_per_split", dict(N=1024, k=64, dtype="bf16", mode="fm", K=32)),
    ("one_per_split", dict(N=4097, k=16, dtype="f32", mode="hhfm", K=64)),
    ("ascending", dict(N=4096, k=64, dtype="bf16", mode="fm")),
    ("ascending", dict(N=16384, k=16, dtype="f32", mode="hhfm")),
    ("ascending", dict(N=16385, k=64, dtype="bf16", mode="hhfm")),
    ("one_per_split", dict(N=16385, k=16, dtype="f32", mode="fm", K=64)),
    ("ascending", dict(N=65536, k=16, dtype="f32", mode="fm")),
    ("plateau_spikes", dict(N=65536, k=128, dtype="bf16", mode="hhfm", m=65)),
]
IDS = [f"{d}-" + "-".join(f"{k}{v}" for k, v in kw.items()) for d, kw in DESIGNS]


def _split3(x):
    """x = x0 + x1 + x2 exactly, each piece a bf16 value."""
    x = np.asarray(x, F32)
    x0 = bf16_round(x)
    x1 = bf16_round(x - x0)
    x2 = bf16_round(x - x0 - x1)
    assert np.array_equal(x0 + x1 + x2, x)
    return x0, x1, x2


def _chain(q, items, order, start):
    """float32 accumulation of q[:, e] * items[:, e] over e in `order`."""
    s = start.astype(F32).copy()
    for e in order:
        s += q[:, e:e + 1] * items[None, :, e]
    return s


@pytest.mark.parametrize("design,kw", DESIGNS, ids=IDS)
def test_scores_are_exact_in_every_order(design, kw):
    d = sd.make(design, B=6, **kw)
    mode = kw["mode"]
    q64, c64 = sd.query_vectors(d.A, d.E, d.ctx, mode)
    q, const = q64.astype(F32), c64.astype(F32)
    assert np.array_equal(q.astype(np.float64), q64) and np.array_equal(const.astype(np.float64), c64)
    items = d.E[d.item_begin:d.item_begin + d.N]
    wi = d.w[d.item_begin:d.item_begin + d.N] if d.w is not None else np.zeros(d.N, F32)
    want = sd.bits(d.scores)
    # the design's closed form: a_u v_i (+ w_i) + h[k-1] + const
    a = np.asarray(sd.A_VALUES)[d.A[:, 0] % 3].astype(np.float64)
    v = d.values if not kw.get("in_w") else np.zeros(d.N)
    if not kw.get("ctx_on_items"):
        closed = a[:, None] * v[None, :] + wi[None, :] + (q64[:, d.k - 1] + c64)[:, None]
        assert np.array_equal(sd.bits(closed.astype(F32)), want)
    k = d.k
    zero = np.zeros((len(q), d.N), F32)
    tail = wi[None, :] + const[:, None]                     # FM epilogue terms (0 for HHFM)
    rng = np.random.default_rng(k + d.N)
    # epilogue last (the MFMA kernels) and first, k reversed and permuted
    assert np.array_equal(sd.bits(_chain(q, items, range(k), zero) + tail), want)
    assert np.array_equal(sd.bits(_chain(q, items, range(k - 1, -1, -1), zero + tail)), want)
    assert np.array_equal(sd.bits(_chain(q, items, rng.permutation(k), zero) + tail), want)
    # the nine products of the three bf16 pieces of each operand, small first
    s = zero.copy()
    qp, ip = _split3(q), _split3(items)
    for pq in (2, 1, 0):
        for pi in (2, 1, 0):
            if not qp[pq].any() or not ip[pi].any():
                continue
            s = _chain(qp[pq], ip[pi], range(k), s)
    assert np.array_equal(sd.bits(s + tail), want)
    if kw["dtype"] == "bf16":
        assert np.array_equal(bf16_round(d.E), d.E)
        assert not qp[1].any() and not qp[2].any() and not ip[1].any()


def test_edges_hold_the_planned_boundaries():
    """The numbers the docstring derives from make_plan / ring_splits."""
    assert sd.split_items(20000) == 544 and sd.split_items(20011, 130) == 544
    assert sd.split_items(65536) == 512 and sd.split_items(65549, 130) == 544
    assert sd.seed_items(65535) == 0 and sd.seed_items(65549) == 4096 and sd.seed_items(20011) == 0
    e = sd.edges(65549)
    for p in (0, 31, 32, 543, 544, 1023, 1024, 4095, 4096, 65535, 65536, 65548):
        assert p in e
    pos = sd.spike_positions(65549, 65, outside_seed=True)
    assert len(set(pos)) == 65 and min(pos) >= 4096 and 65548 in pos and 4096 in pos
    pos = sd.spike_positions(20011, 3)
    assert pos == [20010, 0, 20000]


_ORACLE_CASES = [(d, N, k, dt, mode) for d, N, k, dt in [
    ("all_equal", 20011, 16, "f32"), ("plateau_spikes", 65549, 64, "f32"),
    ("ascending", 65549, 128, "bf16"), ("periodic", 20011, 64, "bf16"),
    ("one_per_split", 20011, 64, "f32")] for mode in ("hhfm", "fm")] + [
    ("w_only", 20011, 64, "f32", "fm")]


@pytest.mark.parametrize("design,N,k,dtype,mode", _ORACLE_CASES)
def test_c_oracle_returns_the_expected_lists(design, N, k, dtype, mode):
    """oracle/cpu_oracle.c (k-ordered fp32 chain, insertion top-K) on the
    designs: whole catalog and a ragged shard with sentinels, K in {1, 20, 64}."""
    from oracle import cpu as ocpu
    extra = {}
    if design == "w_only":
        design, extra = "plateau_spikes", dict(in_w=True)
    lo, cnt = 4099, N - 4099 - 1001
    for K in (1, 20, 64):
        for shard in (None, (lo, cnt)):
            d = sd.make(design, N, k, dtype, mode, B=6, K=K, sentinels=shard, **extra)
            slo, scnt = shard or (0, N)
            rs, ri = ocpu.catalog_topk(d.A, d.E, 0 if mode == "fm" else 1, K, d.item_begin + slo,
                                       scnt, w=d.w, ctx=d.ctx, threads=4)
            es, ei = sd.expected_topk(d.scores, K, slo, scnt)
            assert np.array_equal(ri, ei), (K, shard)
            assert np.array_equal(sd.bits(rs), sd.bits(es)), (K, shard)


@pytest.mark.parametrize("R", [1, 2, 9, 17])
@pytest.mark.parametrize("K", [1, 20, 33, 64])
def test_host_merge_of_designed_partial_lists(R, K):
    """hhfm_topk_merge_host on the per-shard expected lists of designed rows:
    ragged shards, some shorter than K and padded with (-inf, 0x7fffffff)."""
    from hhfm_amd import ops
    N = 2111
    rows = [sd.make(dn, N, 16, B=6, K=K).scores
            for dn in ("all_equal", "plateau_spikes", "periodic", "ascending", "one_per_split")]
    scores = np.concatenate(rows, 0)
    cuts = np.linspace(0, N, R + 1).astype(int)
    if R > 2:                      # two short shards: 5 and 1 items
        cuts[1], cuts[R - 1] = 5, N - 1
        cuts = np.sort(cuts)
    ls = np.full((R, len(scores), K), sd.NEG_INF_PAD[0], F32)
    li = np.full((R, len(scores), K), sd.NEG_INF_PAD[1], np.int32)
    for r in range(R):
        lo, cnt = int(cuts[r]), int(cuts[r + 1] - cuts[r])
        kk = min(K, cnt)
        s, i = sd.expected_topk(scores, kk, lo, cnt, gbase=lo)
        ls[r, :, :kk], li[r, :, :kk] = s, i
    ms, mi = ops.topk_merge(torch.from_numpy(ls), torch.from_numpy(li))
    es, ei = sd.expected_topk(scores, K)
    assert np.array_equal(mi.numpy(), ei)
    assert np.array_equal(sd.bits(ms.numpy()), sd.bits(es))
