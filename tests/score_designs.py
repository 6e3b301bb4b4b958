"""Designed catalog scores — TEST INFRASTRUCTURE ONLY.

Tables whose catalog scores are exact in every arithmetic the K2 kernels use,
so the expected top-K is unique and a kernel can be held to equality of ids
and of score bits (tests/test_gpu_catalog_exact.py), with no tolerance.

Every table value is an integer that bf16 holds exactly (at most 8 significant
bits; ``|x| <= 255`` except the hi/lo pairs and the fp32 ``ascending`` design
below), and every partial sum of a score stays below 2^24.  ``h·item (+ w)``
is then the same float32 in any summation order, on split-bf16 MFMA (the low
pieces of the three-piece split are zero or multiply an exact factor), on
fp32 MFMA, in the GEMM and in float64.  tests/test_score_designs.py proves
that for the reference alone.

Layout of a design (``make``)::

    rows [0, n_user)               users
    rows [n_user, n_user + N)      the catalog; item i is row n_user + i
    rows [n_user + N, M)           context values, CTX_CARDS[j] per column

    dims [0, k - 2)   "item dims": item i holds v_i at dim i % (k - 2) — or,
                      where v_i > 255 on a bf16 table, (v_i // 256, v_i % 256)
                      at the dim pair 2 (i % ((k - 2) / 2)) — and 0 elsewhere;
                      user row u holds a_u in {+3, -2, 0} there (256 a_u on the
                      even dims of a pair design); context rows hold 0
    dim k - 2         items 0; users and context rows small integers
    dim k - 1         items 1; users and context rows small integers

A query (user u, context ids c_j) therefore scores item i

    HHFM   a_u v_i + h[k-1]                     h = E[u] + Σ E[c_j]
    FM     a_u v_i + w_i + q[k-1] + q·f         f = Σ E[c_j], q = E[u] + f

— the designed value times a_u plus a per-query constant that has to come out
of the last k chunk and (FM) of the ``+ w`` / ``(u+f)·f`` epilogue.  One
design gives three rankings per call: the designed order (a = 3), its reverse
with every score <= the constant (a = -2; lists seeded from 0 rather than
-inf would show) and all-equal scores (a = 0: ids lo .. lo + K - 1).

Designs (``values``): ``all_equal``, ``plateau_spikes`` (v = 1, v = 2 at m
edge positions), ``ascending`` (v_i = i), ``periodic`` (v_i = i % 7),
``one_per_split`` (v = 2 at one item of each of K + 1 stretches).  ``in_w``
moves the pattern into FM's w with v = 0; ``sentinels`` plants the largest
value just outside an item range.

Boundaries (``edges``), restated from ``make_plan`` / ``ring_splits`` /
``launch_store`` of csrc/catalog_topk.hip, ``kFusedTiles`` of catalog_fused.h
and ``topk_dense_split_kernel`` of topk_common.h (nothing is exported from the
library; if those change, the numbers here only stop being edges):

  * the MFMA tile: 32 items; the last partial tile starts at N - N % 32;
  * the fused small-catalog kernel's range: 8 waves x 4 tiles = 1,024 items;
  * the streaming item split: tiles_per_split = ceil(ntiles / S), S =
    min(ceil(512 / query_blocks), ntiles / 16).  N = 20,000 and 20,011 (625 /
    626 tiles, S = 39): 17 tiles = 544 items.  N = 65,536 (2,048 tiles, S =
    128): 16 tiles = 512 items; N = 65,549 (2,049 tiles): 17 tiles = 544
    items — the same for catalog_ring at both workgroup sizes up to 256
    queries;
  * the threshold seed: seed_n = (N / 16) & ~31 once that reaches 4,096, i.e.
    4,096 items for N in [65,536, 66,048), scored in seed splits of 16 tiles
    (512 items) on the ring and of single tiles on catalog_main;
  * topk_dense with four waves per query (N >= 1,024, B <= 1,024): spans of
    ceil(ceil(N / 4) / 64) * 64 items.
"""
from collections import namedtuple

import numpy as np

F32 = np.float32
A_VALUES = (3, -2, 0)
CTX_CARDS = (3, 2)          # context vocabulary sizes of the (up to two) context columns
N_USER = 7                  # users 0..6: a = A_VALUES[u % 3], two reserved-dim integers
W_CONST = -7                # FM's w where the pattern is not in w
W_SCALE = 8                 # w_i = W_SCALE * value for in_w designs (|w| < 2^20)
NEG_INF_PAD = (-np.inf, 0x7fffffff)

Design = namedtuple("Design", "A E w scores n_user item_begin N k ctx values")


# ---------------------------------------------------------------------------
# boundaries
# ---------------------------------------------------------------------------
def split_items(N, B=1):
    """Items per streaming split (catalog_main; equal to catalog_ring's at the
    sizes used here), from make_plan's formula."""
    ntiles = (N + 31) // 32
    nqb = (B + 127) // 128
    S = max(1, min((512 + nqb - 1) // nqb, max(ntiles // 16, 1)))
    return 32 * ((ntiles + S - 1) // S)


def seed_items(N):
    sn = (N // 16) & ~31
    return sn if sn >= 4096 and N > 16384 else 0


def edges(N):
    """Sorted item positions on both sides of every boundary that applies to a
    catalog of N items (see the module docstring)."""
    marks = {0, N}
    for unit in (32, 1024, split_items(N), 512 if seed_items(N) else 0):
        if unit:
            marks.update(range(unit, N, unit))
    marks.add(N - N % 32)
    if seed_items(N):
        marks.add(seed_items(N))
    span = (((N + 3) // 4) + 63) // 64 * 64
    marks.update(range(span, N, span))
    pos = set()
    for b in marks:
        pos.update(p for p in (b - 1, b) if 0 <= p < N)
    return sorted(pos)


def spike_positions(N, m, outside_seed=False):
    """m edge positions, the rarest boundaries first: last / first item, the
    last partial tile, the seed edge, then split, range and tile edges spread
    over the catalog."""
    sd, sp = seed_items(N), split_items(N)
    first = [N - 1, 0, N - N % 32, N - N % 32 - 1]
    if sd:
        first += [sd, sd - 1, sd + sp - sd % sp, sd + sp - sd % sp - 1]
    first += [sp, sp - 1, 1024, 1023, 32, 31]
    nsp = (N + sp - 1) // sp
    for j in range(1, nsp):   # one side of every split edge, far splits first
        s = nsp - j if j % 2 else j
        first.append(s * sp - (j % 2))
    first += edges(N)[::-1]
    out = []
    if m == 0:
        return out
    for p in first:
        if 0 <= p < N and p not in out and not (outside_seed and p < sd):
            out.append(p)
        if len(out) == m:
            return out
    raise ValueError(f"no {m} edge positions in {N} items")


# ---------------------------------------------------------------------------
# designs
# ---------------------------------------------------------------------------
def values(design, N, K=20, m=None, outside_seed=False):
    """int64 [N]: the designed value v_i of every item."""
    i = np.arange(N, dtype=np.int64)
    if design == "all_equal":
        return np.ones(N, np.int64)
    if design == "plateau_spikes":
        v = np.ones(N, np.int64)
        v[spike_positions(N, K + 1 if m is None else m, outside_seed)] = 2
        return v
    if design == "ascending":
        return i
    if design == "periodic":
        return i % 7
    if design == "one_per_split":
        # K + 1 equal stretches, one spike in each at a varying offset; the
        # stretches are >= a streaming split (544 items) while K + 1 <= N / 544
        v = np.ones(N, np.int64)
        stretch = N // (K + 1)
        j = np.arange(K + 1)
        v[j * stretch + (j * 37) % max(min(stretch, 31), 1)] = 2
        return v
    raise ValueError(design)


def with_sentinels(v, lo, cnt, width=2):
    """The largest value + 1 on `width` rows just outside [lo, lo + cnt) on
    both sides (where the catalog has them)."""
    v = v.copy()
    top = v.max() + 1
    for j in range(width):
        for p in (lo - 1 - j, lo + cnt + j):
            if 0 <= p < len(v):
                v[p] = top
    return v


def make(design, N, k, dtype="f32", mode="hhfm", B=37, K=20, m=None, n_ctx=2, in_w=False,
         sentinels=None, outside_seed=False, ctx_on_items=False):
    """Design(A, E, w, scores, ...) for a named design.

    A int32 [B, 2 + n_ctx] (user, unused item column, context ids); E float32
    [M, k] (every value exact in bf16 for dtype "bf16"); w float32 [M] (FM) or
    None; scores float32 [B, N], the expected score of every item.
    ``sentinels`` (lo, cnt): see with_sentinels.  ``ctx_on_items``: context
    rows hold -1 / 0 / +1 on the item dims (pooled-query tests)."""
    assert k >= 8 and k % 2 == 0 and mode in ("hhfm", "fm") and dtype in ("f32", "bf16")
    assert not (in_w and mode != "fm")
    v = values(design, N, K, m, outside_seed)
    if sentinels is not None:
        v = with_sentinels(v, *sentinels)
    ku = k - 2
    cards = CTX_CARDS[:n_ctx]
    item_begin = N_USER
    c0 = item_begin + N
    M = c0 + sum(cards)
    E = np.zeros((M, k), F32)
    w = None
    ev = np.zeros(N, np.int64) if in_w else v
    pair = dtype == "bf16" and ev.max() > 255
    assert not (pair and ctx_on_items)
    i = np.arange(N)
    items = E[item_begin:c0]
    if pair:
        d = 2 * (i % (ku // 2))
        items[i, d] = ev // 256
        items[i, d + 1] = ev % 256
    else:
        items[i, i % ku] = ev
    items[:, k - 1] = 1
    u = np.arange(N_USER)
    a = np.asarray(A_VALUES)[u % 3]
    E[:N_USER, :ku] = a[:, None]
    if pair:
        E[:N_USER, 0:ku:2] *= 256
    E[:N_USER, k - 2] = u % 5 - 2
    E[:N_USER, k - 1] = u % 4 + 1
    off = c0
    for card in cards:
        c = np.arange(card)
        E[off:off + card, k - 2] = c + 1
        E[off:off + card, k - 1] = 2 - c
        if ctx_on_items:
            E[off:off + card, :ku] = (c % 3 - 1)[:, None]
        off += card
    if mode == "fm":
        w = np.zeros(M, F32)
        w[:] = 3                                  # user / context entries: never read
        w[item_begin:c0] = W_SCALE * v if in_w else W_CONST
    if dtype == "bf16":
        bits = E.view(np.uint32)
        assert not np.any(bits & 0xffff), "design value not exact in bf16"
    b = np.arange(B)
    cols = [b % N_USER, np.full(B, item_begin)]
    off = c0
    for j, card in enumerate(cards):
        cols.append(off + (b + j) % card)
        off += card
    A = np.stack(cols, 1).astype(np.int32)
    ctx = (2, 2 + n_ctx) if n_ctx else (0, 0)
    scores = expected_scores(A, E, w, item_begin, N, ctx, mode)
    return Design(A, E, w, scores, N_USER, item_begin, N, k, ctx, v)


def query_vectors(A, E, ctx, mode):
    """(q float64 [B, k], const float64 [B]): the query vector and the
    item-independent term ((u+f)·f for FM, 0 for HHFM)."""
    E64 = np.asarray(E, np.float64)
    A = np.asarray(A, np.int64)
    f = E64[A[:, ctx[0]:ctx[1]]].sum(1) if ctx[1] > ctx[0] else np.zeros((len(A), E.shape[1]))
    q = E64[A[:, 0]] + f
    return q, ((q * f).sum(1) if mode == "fm" else np.zeros(len(A)))


def scores_from_queries(q, const, E, w, item_begin, N):
    """float32 [B, N] = float64 (q·item + w + const) rounded once."""
    s = np.asarray(q, np.float64) @ np.asarray(E[item_begin:item_begin + N], np.float64).T
    if w is not None:
        s = s + np.asarray(w[item_begin:item_begin + N], np.float64)[None, :]
    s = s + np.asarray(const, np.float64)[:, None]
    assert np.abs(s).max() < 2 ** 24
    return s.astype(F32)


def expected_scores(A, E, w, item_begin, N, ctx, mode):
    """float32 [B, N]; equal query rows are scored once."""
    uniq, inv = np.unique(np.asarray(A), axis=0, return_inverse=True)
    q, const = query_vectors(uniq, E, ctx, mode)
    return scores_from_queries(q, const, E, w, item_begin, N)[inv.reshape(-1)]


def expected_topk(scores, K, lo=0, cnt=None, gbase=0):
    """tf.nn.top_k order over the shard [lo, lo + cnt) of every score row: a
    stable argsort by descending score (equal scores, +0 and -0 among them,
    keep ascending ids).  Returns (scores float32 [B, K] — the picked
    elements' own bits —, ids int32 [B, K] = gbase + offset in the shard)."""
    scores = np.asarray(scores, F32)
    cnt = scores.shape[1] - lo if cnt is None else cnt
    sub = scores[:, lo:lo + cnt]
    out_s = np.empty((len(sub), K), F32)
    out_i = np.empty((len(sub), K), np.int32)
    seen = {}
    for b, row in enumerate(sub):
        key = row.tobytes()
        if key not in seen:
            seen[key] = np.argsort(-row, kind="stable")[:K]
        order = seen[key]
        out_s[b] = row[order]
        out_i[b] = order + gbase
    return out_s, out_i


def bits(x):
    """float32 array -> its bit patterns as int32."""
    return np.ascontiguousarray(x, F32).view(np.int32)


def ragged_shards(lo, total, R=3):
    """R contiguous shards (offset, count) of [lo, lo + total) whose counts are
    no multiples of 32."""
    base = total // R
    cnts = [base - 13 + 7 * r for r in range(R - 1)]
    cnts.append(total - sum(cnts))
    out, o = [], lo
    for c in cnts:
        assert c % 32 and c > 0
        out.append((o, c))
        o += c
    return out
