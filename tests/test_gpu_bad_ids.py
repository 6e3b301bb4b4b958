"""Bad ids read row 0 — on every id-reading path, with guard-banded tables.

include/hhfm.h promises that an id outside [0, features_M) is read as row 0 by
every kernel, and that entry points with a status word flag it.  Each case
here sends bad ids through one entry point on tables that sit between quiet-NaN
pads (tests/guard_tables.py) and runs it three times on the same buffers and
plan:

* ``zeroed``  the bad positions hold 0;
* ``bad``     they hold near-miss ids, {−8 … −1} ∪ {M … M + 7};
* ``moved``   they hold another in-range id, whose row differs from row 0.

Forward and catalog entry points: two ``zeroed`` runs are bitwise equal (so the
comparison means something), ``bad`` is bitwise equal to ``zeroed``, every
output is finite, ``moved`` differs from ``zeroed`` in exactly the rows (or
queries) that held a bad id, the status word is BAD_ID after ``bad`` and clear
after ``zeroed``, and no guard pad changed.  Train steps: the ``bad`` step
meets the model's existing oracle for the zeroed batch at the bar of the
model's own test file, row 0 of the table moved, and no pad of a table, a slot
array or the workspace changed.

Only near misses are used: with pads of 8 rows or more an unclamped access
lands in memory the test allocated and shows as a NaN, a changed output or a
changed pad.  Nothing in this file can fault the device, whether the code
under test is right or wrong; far values (INT_MIN, INT_MAX) go to
hhfm_check_ids alone, which looks nothing up.

The catalog-window cases put the item window flush against the last row of a
NaN-padded table (and against the first) with item counts one below, at and
one above the kernels' tile widths: a ragged last tile must not read past the
window.

Each parametrization's id names the kernel or plan it reaches, read off the
dispatchers (csrc/afm.hip, csrc/mlp_gemm.hip, csrc/dfm_fused.hip,
csrc/dfm_wide.hip, csrc/catalog_topk.hip) and confirmed with a kernel trace of
this file.
"""
import numpy as np
import pytest
import torch

from tests.guard_tables import Guards, near_miss_ids, plant

pytestmark = pytest.mark.gpu

BAD_ID = 1
EINVAL = -1
INT_MIN, INT_MAX = -2**31, 2**31 - 1


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _table(a, tdt):
    t = _dev(np.asarray(a, np.float32))
    return t.to(torch.bfloat16).contiguous() if tdt == "bf16" else t


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_ibits(x), _ibits(y)) for x, y in zip(a, b))


@pytest.fixture
def guards(monkeypatch):
    """The case's guard pads; every workspace hhfm_amd.ops hands to the library
    is a fresh one of exactly the queried size between two 0xA5 guards."""
    from hhfm_amd import ops
    g = Guards()
    monkeypatch.setattr(ops, "_workspace", lambda dev, n: g.workspace(max(n, 256), dev))
    monkeypatch.setattr(ops, "_catalog_workspace",
                        lambda dev, st, n: g.workspace(max(n, 256), dev))
    return g


def _positions(B, F, pair=(2, 3)):
    """Where the bad ids go in a [B, F] batch: the first row, the last row (in
    the ragged tail of the kernel's row block), field 0, field 1, the last
    field, one row with two bad ids that form a pair, one row made entirely of
    bad ids."""
    pos = [(0, 0), (B - 1, F - 1), (B // 3, 0), (B // 2, F - 1), (B // 3 + 1, 1),
           (B // 2 + 1, pair[0]), (B // 2 + 1, pair[1])]
    pos += [(B - 2, c) for c in range(F)]
    return sorted(set(pos))


def _three_runs(run, X, positions, M, guards, status=None, ignored=(), seed=0):
    """The zeroed / bad / moved protocol of the module docstring for a forward
    or catalog entry point.  ``run(ids)`` -> tuple of [rows, ...] tensors.
    ``ignored``: positions the entry point must not read (the item column of a
    catalog query): they hold a near-miss id in all three batches, must leave
    the outputs as they are with an in-range id there and must not be flagged."""
    rng = np.random.default_rng(seed)
    zeroed, bad, moved, rows = plant(X, positions, M, rng, M - 1)
    clean = zeroed.copy()
    nm = near_miss_ids(M)
    for n, (r, c) in enumerate(ignored):
        zeroed[r, c] = bad[r, c] = moved[r, c] = nm[(3 + 5 * n) % len(nm)]

    def go(ids):
        if status is not None:
            status.zero_()
        out = [o.clone() for o in run(_dev(ids))]
        torch.cuda.synchronize()
        return out, None if status is None else int(status.item())

    z1, st_zero = go(zeroed)
    z2, _ = go(zeroed)
    assert _same(z1, z2), "two runs on the same ids differ: the comparison below means nothing"
    got, st_bad = go(bad)
    for o in got:
        if o.is_floating_point():
            assert torch.isfinite(o).all(), "a bad id read outside the table (NaN pad)"
    assert _same(got, z1), "bad ids are not read as row 0"
    mv, _ = go(moved)
    B = len(X)
    changed = torch.zeros(B, dtype=torch.bool, device="cuda")
    for a, b in zip(mv, z1):
        changed |= (_ibits(a) != _ibits(b)).reshape(B, -1).any(1)
    assert changed.nonzero().reshape(-1).tolist() == rows, "the ids at the bad positions are not read"
    if ignored:
        cl, _ = go(clean)
        assert _same(cl, z1), "an ignored column changes the output"
    if status is not None:
        assert st_zero == 0 and st_bad == BAD_ID, (st_zero, st_bad)
    guards.assert_untouched()


# ---------------------------------------------------------------------------
# hhfm_check_ids
# ---------------------------------------------------------------------------
def _check(ids, M, st):
    from hhfm_amd._native import native
    native().check_ids(ids.data_ptr(), ids.numel(), M, st.data_ptr(), _stream())


def _read(st):
    from hhfm_amd._native import native
    return native().status_read(st.data_ptr(), _stream())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048 * 256 + 1])
def test_check_ids_edges(n):
    """check_ids_kernel: one block, a full block, one element into a second
    block, and 2048·256 + 1 elements — one more than the capped grid covers in
    a single grid-stride trip.  A bad element at the first, middle and last
    position with −1, INT_MIN, M and INT_MAX is reported; an all-good array
    holding 0 and M − 1 is not."""
    M = 1000
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    good = (torch.arange(n, dtype=torch.int64, device="cuda") % M).to(torch.int32)
    good[-1] = M - 1
    for edge in (0, M - 1):
        g = good.clone()
        g[0] = edge
        _check(g, M, st)
        assert _read(st) == 0, edge
    for pos in sorted({0, n // 2, n - 1}):
        for v in (-1, INT_MIN, M, INT_MAX):
            x = good.clone()
            x[pos] = v
            _check(x, M, st)
            assert int(st.item()) == BAD_ID, (pos, v)
            assert _read(st) == EINVAL, (pos, v)
            assert int(st.item()) == 0 and _read(st) == 0     # the read cleared the word


def test_check_ids_single_row_table():
    """M = 1: id 0 is the only good one."""
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    _check(torch.zeros(300, dtype=torch.int32, device="cuda"), 1, st)
    assert _read(st) == 0
    for v in (1, -1, INT_MIN, INT_MAX):
        x = torch.zeros(300, dtype=torch.int32, device="cuda")
        x[299] = v
        _check(x, 1, st)
        assert _read(st) == EINVAL, v


def test_check_ids_status_ors_across_calls():
    """The word ORs: a good array checked after a bad one leaves BAD_ID set;
    status_read reports it once and clears it."""
    from hhfm_amd import ops
    M = 50
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    bad = torch.arange(40, dtype=torch.int32, device="cuda")
    bad[17] = M
    good = torch.arange(40, dtype=torch.int32, device="cuda")
    _check(bad, M, st)
    _check(good, M, st)
    assert int(st.item()) == BAD_ID
    assert _read(st) == EINVAL
    assert _read(st) == 0
    _check(good, M, st)
    assert _read(st) == 0
    with pytest.raises(ValueError, match="indices must be in"):
        ops.validate_ids(bad, M)
    ops.validate_ids(good, M)                                 # the shared word was cleared


@pytest.mark.parametrize("plan", ["fused", "store"])
def test_catalog_query_id_check_reads_the_used_columns_only(plan, guards):
    """launch_check_query_ids through hhfm_catalog_topk_ex (the fused
    small-catalog kernel and catalog_queries + the STORE plan): a near-miss id
    in the user, a context or a time column is flagged; in the item column or
    in a column no range names it is not, and changes nothing."""
    from hhfm_amd import ops
    rng = np.random.default_rng(5)
    nu, ni, k, B = 20, 70, 16, 37
    M = nu + ni + 12
    E = guards.table(_dev(rng.normal(0, 0.3, (M, k)).astype(np.float32)))
    q = np.concatenate([rng.integers(0, nu, (B, 1)), rng.integers(nu, nu + ni, (B, 1)),
                        rng.integers(nu + ni, M, (B, 5))], 1).astype(np.int32)   # col 6 unused
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    flag = ops.PLAN_STORE if plan == "store" else 0

    def run(ids):
        return ops.catalog_topk(ids, E, ops.MODE_HHFM, 10, nu, ni, 0, None, 0, (2, 4), (4, 6),
                                status=st, plan=flag)

    pos = [(0, 0), (B - 1, 5), (B // 3, 2), (B // 2, 4), (B // 2 + 1, 2), (B // 2 + 1, 3)]
    pos += [(B - 2, c) for c in (0, 2, 3, 4, 5)]
    _three_runs(run, q, pos, M, guards, status=st, ignored=[(3, 1), (4, 6), (B - 2, 1)])
    nm = near_miss_ids(M)
    for col, want in ((0, BAD_ID), (2, BAD_ID), (3, BAD_ID), (4, BAD_ID), (5, BAD_ID), (1, 0),
                      (6, 0)):
        for v in (nm[0], nm[-1], -1, M):
            one = q.copy()
            one[B - 1, col] = v
            st.zero_()
            run(_dev(one))
            assert int(st.item()) == want, (col, v)


# ---------------------------------------------------------------------------
# AFM rows
# ---------------------------------------------------------------------------
def _afm_weights(rng, k, A):
    return (_dev(rng.normal(0, 0.3, (A, k)).astype(np.float32)),
            _dev(rng.normal(0, 0.1, A).astype(np.float32)),
            _dev(rng.normal(0, 0.5, A).astype(np.float32)),
            _dev(rng.normal(1, 0.2, k).astype(np.float32)))


AFM_ROW_CASES = {
    # id: (F, k, A, plan) -> kernel (csrc/afm.hip hhfm_afm_forward_ex)
    "afm_rows_pairs": (5, 32, 32, 0),
    "afm_rows_pairs-k64": (5, 64, 32, 0),
    "afm_rows_fused-split": (5, 32, 32, "PLAN_PER_FIELD"),
    "afm_rows_fused-exact": (5, 32, 32, "PLAN_EXACT_FP32"),
    "afm_rows_fused-k16": (3, 16, 8, 0),
    "afm_rows_finish-gemm": (9, 32, 32, 0),
    "afm_rows_finish-gemm-exact": (9, 32, 32, "PLAN_EXACT_FP32"),
}


@pytest.mark.parametrize("tdt", ["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(AFM_ROW_CASES))
def test_afm_rows_bad_ids(case, tdt, guards):
    """hhfm_afm_forward_ex: the pair-major kernel (afm_rows_pairs, split
    arithmetic at k = 32 / 64), the combo-packed one (afm_rows_fused: split under
    PLAN_PER_FIELD, exact under PLAN_EXACT_FP32, and k = 16), and the pair-gather
    GEMM + afm_rows_finish beyond 32 pairs (F = 9), fp32 and bf16 tables.
    B = 131: one row past a 128-row workgroup and past four 32-row wave tiles."""
    from hhfm_amd import ops
    F, k, A, plan = AFM_ROW_CASES[case]
    plan = getattr(ops, plan) if isinstance(plan, str) else plan
    rng = np.random.default_rng(F * 100 + k + A)
    M, B = 61, 131
    E = guards.table(_table(rng.normal(0, 0.3, (M, k)), tdt))
    w = guards.table(_dev(rng.normal(0, 0.1, M).astype(np.float32)))
    Wt, b, p, P = _afm_weights(rng, k, A)
    X = rng.integers(0, M, (B, F)).astype(np.int32)

    def run(ids):
        return (ops.afm_forward(ids, E, w, 0.02, Wt, b, p, P, plan=plan),)

    _three_runs(run, X, _positions(B, F, pair=(1, F - 1)), M, guards)


# ---------------------------------------------------------------------------
# AFM catalog, with and without attention
# ---------------------------------------------------------------------------
AFM_CAT_CASES = {
    # id: (plan names) -> kernels (csrc/afm.hip hhfm_afm_catalog_topk_ex)
    "afm_cat_qside+afm_cat_w": (),
    "afm_cat_qside+afm_cat_fused-split": ("PLAN_PER_FIELD",),
    "afm_cat_qside+afm_cat_fused-exact": ("PLAN_EXACT_FP32",),
    "afm_cat_prep+gemm+afm_cat_finish": ("PLAN_GEMM",),
}


def _plan(names):
    from hhfm_amd import ops
    word = 0
    for n in names:
        word |= getattr(ops, n)
    return word


def _afm_queries(rng, nq, nu, ni, M, F):
    return np.concatenate([rng.integers(0, nu, (nq, 1)), rng.integers(nu, nu + ni, (nq, 1)),
                           rng.integers(nu + ni, M, (nq, F - 2))], 1).astype(np.int32)


@pytest.mark.parametrize("tdt", ["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(AFM_CAT_CASES))
def test_afm_catalog_bad_ids(case, tdt, guards):
    """hhfm_afm_catalog_topk_ex: the query side (afm_cat_qside, or afm_cat_prep
    under PLAN_GEMM) and the item side (the per-query kernel afm_cat_w with the
    folded weights, afm_cat_fused under PLAN_PER_FIELD or PLAN_EXACT_FP32, the
    GEMM + afm_cat_finish).  9 queries, 70 items (a ragged third 32-item
    tile); the score reads columns 0, 2 … F − 1 and ignores column 1."""
    from hhfm_amd import ops
    plan = _plan(AFM_CAT_CASES[case])
    rng = np.random.default_rng(77)
    F, k, A, nq, nu, ni = 5, 32, 32, 9, 12, 70
    M = nu + ni + 9
    E = guards.table(_table(rng.normal(0, 0.3, (M, k)), tdt))
    w = guards.table(_dev(rng.normal(0, 0.1, M).astype(np.float32)))
    Wt, b, p, P = _afm_weights(rng, k, A)
    q = _afm_queries(rng, nq, nu, ni, M, F)

    def run(ids):
        return ops.afm_catalog_topk(ids, E, w, Wt, b, p, P, nu, ni, 10, 0, plan=plan)

    pos = [(0, 0), (nq - 1, F - 1), (2, 0), (3, 2), (4, 2), (4, 3)] + [(6, c) for c in (0, 2, 3, 4)]
    _three_runs(run, q, pos, M, guards, ignored=[(1, 1), (6, 1)])


@pytest.mark.parametrize("tdt", ["f32", "bf16"])
@pytest.mark.parametrize("plan", ["store", "gemm"])
def test_afm_noatt_catalog_bad_ids(plan, tdt, guards):
    """hhfm_afm_noatt_catalog_topk: afm_noatt_queries forms H and cst from
    every column but column 1 (table rows and w by id), then the score-matrix
    plans run; the status word flags those columns only."""
    from hhfm_amd import ops
    rng = np.random.default_rng(31)
    F, k, nq, nu, ni = 5, 16, 37, 12, 70
    M = nu + ni + 9
    E = guards.table(_table(rng.normal(0, 0.3, (M, k)), tdt))
    w = guards.table(_dev(rng.normal(0, 0.1, M).astype(np.float32)))
    P = _dev(rng.normal(1, 0.2, k).astype(np.float32))
    q = _afm_queries(rng, nq, nu, ni, M, F)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    flag = ops.PLAN_GEMM if plan == "gemm" else 0

    def run(ids):
        return ops.afm_noatt_catalog_topk(ids, E, w, 0.02, P, nu, ni, 10, 0, status=st, plan=flag)

    pos = [(0, 0), (nq - 1, F - 1), (12, 0), (18, 2), (19, 2), (19, 3)]
    pos += [(nq - 2, c) for c in (0, 2, 3, 4)]
    _three_runs(run, q, pos, M, guards, status=st, ignored=[(1, 1), (nq - 2, 1)])


# ---------------------------------------------------------------------------
# DeepFM forward
# ---------------------------------------------------------------------------
def _dfm_weights(rng, F, k, layers, mlp):
    from hhfm_amd import ops
    Ls, bs, kin = [], [], F * k
    for n in layers:
        Ls.append(_dev(rng.normal(0, np.sqrt(2.0 / (kin + n)), (kin, n)).astype(np.float32)))
        bs.append(_dev(rng.normal(0, 0.1, n).astype(np.float32)))
        kin = n
    mdt = torch.bfloat16 if mlp == "bf16" else torch.float32
    Wt, bias, dims = ops.dfm_prepare_weights(Ls, bs, mdt, F, k)
    Wp = _dev(rng.normal(0, 0.3, F + k + layers[-1]).astype(np.float32))
    return Wt, bias, dims, mdt, Wp, 0.05


# id: (k, layers, mlp, proj, plan names, M, B, users) -> kernels (csrc/mlp_gemm.hip dfm_plan /
# dfm_forward_impl, csrc/dfm_fused.hip dfm_fused_launch, csrc/dfm_wide.hip dfm_wide_launch).
# M = 40: a block's P rows of every projected field fit the LDS stage (plo / phi from the
# clamped ids); M = 997: they do not, the block reads P through the caches.  users: field 0
# is drawn from that many ids (grouped plans).
DFM_CASES = {
    "dfm_fused-bf16mlp": (16, [33, 20], "bf16", False, (), 40, 131, 0),
    "dfm_fused_f32": (16, [33, 20], "f32", False, (), 40, 131, 0),
    "dfm_fm_part+gather-gemm-f32mlp": (40, [33, 20], "f32", False, (), 40, 131, 0),
    "dfm_fm_part+gather-gemm-bf16mlp": (40, [33, 20], "bf16", False, (), 40, 131, 0),
    "dfm_fused-proj-on-staged": (16, [33, 20], "bf16", True, (), 40, 131, 0),
    "dfm_fused-proj-on-hbm": (16, [33, 20], "bf16", True, (), 997, 131, 0),
    "dfm_fused-proj-ctx-staged": (16, [33, 20], "bf16", "ctx", (), 40, 131, 0),
    "dfm_fused-proj-ctx-hbm": (16, [33, 20], "bf16", "ctx", (), 997, 131, 0),
    "dfm_fused-proj-item+dfm_group_hist+dfm_group_scatter": (16, [33, 20], "bf16", "item", (), 40,
                                                            131, 7),
    "dfm_fused-proj-item+dfm_order_keys+radix+dfm_gather_rows": (16, [33, 20], "bf16", "item", (), 8200, 131, 7),
    "dfm_fused_f32-proj-1layer": (16, [33], "f32", True, (), 40, 131, 0),
    "dfm_fused_f32-proj-exact": (16, [33, 20], "f32", True, ("PLAN_EXACT_FP32",), 40, 131, 0),
    "dfm_fused_f32s+dfm_fm_base": (16, [33, 20], "f32", True, (), 40, 131, 0),
    "dfm_fused_f32s+dfm_fm_base_st": (64, [33, 20], "f32", True, (), 40, 131, 0),
    "dfm_fused_f32s-unstaged+dfm_fm_base-k64": (64, [33, 20], "f32", True, ("PLAN_UNSTAGED",), 40,
                                                131, 0),
    "dfm_fused_f32s+dfm_fm_base_pairs": (16, [33, 20], "f32", True, (), 40, 643, 0),
    "dfm_fused_f32s+row_fm": (16, [33, 20], "f32", True, ("PLAN_ROW_FM",), 40, 643, 0),
    "dfm_fused_f32s-grouped+dfm_group_hist": (16, [33, 20], "f32", True, (), 40, 2563, 7),
    "dfm_fused_f32s-ungrouped": (16, [33, 20], "f32", True, ("PLAN_UNGROUPED",), 40, 2563, 7),
    "dfm_wide-one-ragged-block": (64, [150, 150, 150], "bf16", "item", (), 40, 131, 7),
    "dfm_wide-pairs": (64, [150, 150, 150], "bf16", "item", (), 40, 643, 7),
    "dfm_wide-overflow-blocks": (64, [150, 150, 150], "bf16", "item", (), 997, 300, 0),
    "dfm_fused-narrow-item": (64, [150, 150, 150], "bf16", "item", ("PLAN_NARROW",), 40, 131, 7),
}


# (the wide kernel is instantiated for bf16 tables only: with an fp32 table its
# cases would run dfm_fused again)
DFM_PARAMS = [(c, t) for c in sorted(DFM_CASES) for t in ("f32", "bf16")
              if t == "bf16" or not c.startswith("dfm_wide")]


@pytest.mark.parametrize("case,tdt", DFM_PARAMS, ids=["-".join(p) for p in DFM_PARAMS])
def test_dfm_forward_bad_ids(case, tdt, guards):
    """hhfm_dfm_forward_ex with ``proj`` and ``plan`` explicit, F = 5: the fused
    bf16 / fp32 kernels, the direct path outside their envelope (k % 16 != 0),
    projected layer 0 in its ON / CTX / ITEM modes with the P rows LDS-staged
    and not, the grouping front end on both sides of its 8192-key split, the
    split fp32 kernel with each FM-base kernel, and the wide ITEM kernel
    (dfm_fused_w, both of its launches: staged blocks and overflow blocks)."""
    from hhfm_amd import ops
    k, layers, mlp, proj, plans, M, B, users = DFM_CASES[case]
    F = 5
    rng = np.random.default_rng(len(case) * 131 + k)
    E = guards.table(_table(rng.normal(0, 0.3, (M, k)), tdt))
    w = guards.table(_dev(rng.normal(0, 0.1, M).astype(np.float32)))
    Wt, bias, dims, mdt, Wp, bp = _dfm_weights(rng, F, k, layers, mlp)
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    if users:
        X[:, 0] = rng.integers(1, users, B)
    plan = _plan(plans)

    def run(ids):
        return (ops.dfm_forward(ids, E, w, Wt, bias, dims, mdt, Wp, bp, proj=proj, plan=plan),)

    _three_runs(run, X, _positions(B, F), M, guards)


@pytest.mark.parametrize("tdt", ["f32", "bf16"])
@pytest.mark.parametrize("mlp,proj", [("f32", False), ("bf16", False), ("f32", True),
                                      ("bf16", "item"), ("bf16", "ctx")])
def test_dfm_catalog_bad_ids(mlp, proj, tdt, guards):
    """hhfm_dfm_catalog_topk_ex: dfm_build_rows copies the raw query ids into
    the tiled rows, which the forward kernels then clamp; 7 queries x 70 items
    in chunks of three queries.  Column 1 (item_col) is replaced by the items."""
    from hhfm_amd import ops
    rng = np.random.default_rng(13)
    F, k, nq, nu, ni = 5, 16, 7, 12, 70
    M = nu + ni + 9
    E = guards.table(_table(rng.normal(0, 0.3, (M, k)), tdt))
    w = guards.table(_dev(rng.normal(0, 0.1, M).astype(np.float32)))
    Wt, bias, dims, mdt, Wp, bp = _dfm_weights(rng, F, k, [33, 20], mlp)
    q = _afm_queries(rng, nq, nu, ni, M, F)

    def run(ids):
        return ops.dfm_catalog_topk(ids, E, w, Wt, bias, dims, Wp, bp, 1, nu, ni, 10, 0, 3 * ni,
                                    proj=proj)

    pos = [(0, 0), (nq - 1, F - 1), (2, 0), (3, 2), (3, 3)] + [(5, c) for c in (0, 2, 3, 4)]
    _three_runs(run, q, pos, M, guards, ignored=[(1, 1), (5, 1)])


# ---------------------------------------------------------------------------
# Train steps (the kernels that WRITE by id: table rows, w, optimizer slots,
# the touched-row lists of the workspace)
# ---------------------------------------------------------------------------
def _arm(m, guards, names, ws_bytes=None, rows=0, extra=()):
    """Put a model class's trainable tensors (``names``; ``extra``: tensors
    the step writes without a slot), their optimizer slots and its train
    workspace between guard pads, and stop the class from range-checking ids
    (the C callers' situation).  ``ws_bytes`` None: FM / HHFM's fixed
    workspace; else the size for this batch, of ``rows`` rows."""
    from hhfm_amd import training
    m.validate = False
    for n in list(names) + list(extra):
        m.weights[n] = guards.table(m.weights[n])
    st = training._state(m, list(names), training._opt_code(m), fixed_ws=ws_bytes is None)
    for n in names:
        st[n] = guards.table(st[n])
    nbytes = st["ws"].numel() if ws_bytes is None else ws_bytes
    st["ws"], st["ws_rows"] = guards.workspace(nbytes, m.device), rows
    return st


def _feed(m, **bad):
    """Every later ``m.partial_fit(data)`` runs on ``bad``'s arrays instead of
    ``data``'s: the replay helpers of the models' own test files then compare
    the step on the bad batch with their oracle on the batch they were given,
    the zeroed one, at their own bars."""
    real = m.partial_fit

    def fit(data):
        d = dict(data)
        d.update(bad)
        return real(d)

    m.partial_fit = fit


def _row0(m):
    return m.weights["feature_embeddings"][0].clone()


def _done(m, guards, before):
    """Row 0 received the bad ids' gradient; no pad changed."""
    assert not torch.equal(_ibits(_row0(m)), _ibits(before)), "row 0 of E did not move"
    guards.assert_untouched()


TRAIN_B = 131        # one row past 128; the bad last rows sit in a ragged tail


@pytest.mark.parametrize("opt,lam,k", [("AdagradOptimizer", 0.1, 32), ("AdamOptimizer", 0.0, 32),
                                       ("MomentumOptimizer", 0.1, 128)])
def test_fm_train_step_bad_ids(opt, lam, k, guards):
    """hhfm_fm_train_step(_ex at keep 1): fm_train_rows scatters into dE, dw and
    the touched-row list by id, the optimizer tail then walks those rows of E,
    w and the slots.  test_gpu_training._fm_replay's bars."""
    from tests.test_gpu_training import FM_NAMES, OPTS, _fm_model, _fm_replay, _rows
    rng = np.random.default_rng(3)
    nu, ni = 40, 90
    X, M = _rows(rng, TRAIN_B, nu, ni, (7, 2, 3))
    zeroed, bad, _, _ = plant(X, _positions(TRAIN_B, 5), M, rng, M - 1)
    m = _fm_model(rng, opt, lam, nu, ni, k)
    _arm(m, guards, FM_NAMES)
    _feed(m, X=bad)
    before = _row0(m)
    y = rng.integers(0, 2, TRAIN_B).astype(np.float32)[:, None]
    _fm_replay(m, zeroed.astype(np.int64), y, OPTS[opt], lam, 1)
    _done(m, guards, before)


@pytest.mark.parametrize("keep", [0.7])
def test_fm_train_step_dropout_bad_ids(keep, guards):
    """hhfm_fm_train_step_ex at keep < 1 through the binding: one SGD step at
    lr 1, λ 0 leaves before − after equal to the raw gradient, held to the
    masked float64 gradient of the zeroed batch by test_gpu_dropout._check."""
    from hhfm_amd._native import native
    from tests import dropout_ref as dr
    from tests.test_gpu_dropout import SGD, _check
    rng = np.random.default_rng(8)
    M, F, k, B, seed = 50, 5, 64, TRAIN_B, dr.FM_SEED
    X = rng.integers(0, M, (B, F)).astype(np.int32)
    zeroed, bad, _, _ = plant(X, _positions(B, F), M, rng, M - 1)
    E = rng.normal(0, 0.15, (M, k)).astype(np.float32)
    w = rng.normal(0, 0.3, M).astype(np.float32)
    w0 = np.float32(0.02)
    y = rng.integers(0, 2, B).astype(np.float32)
    bn = dr.binary(seed, dr.SITE_FM, B, k, keep)
    ref_loss, (dE, dw, dw0), (mE, mw, mw0) = dr.fm_grad64_dropout(zeroed, y, E, w, w0, bn, keep)
    Ed, wd, w0d = (guards.table(_dev(a)) for a in (E, w, np.float32([w0])))
    ws = guards.workspace(native().train_workspace(M, k), Ed.device)
    loss = torch.zeros(1, device="cuda")
    Xd, yd = _dev(bad), _dev(y)
    native().fm_train_step_ex(Xd.data_ptr(), yd.data_ptr(), B, F, Ed.data_ptr(), wd.data_ptr(),
                              w0d.data_ptr(), M, k, 1.0, 0.0, SGD, keep, seed, 0, 0, 0,
                              ws.data_ptr(), ws.numel(), loss.data_ptr(), _stream())
    assert np.isclose(float(loss.item()), ref_loss, rtol=1e-5)
    _check(f"fm bad ids keep {keep} E", E, Ed.cpu().numpy(), dE, mE)
    _check(f"fm bad ids keep {keep} w", w, wd.cpu().numpy(), dw, mw)
    _check(f"fm bad ids keep {keep} w0", w0, np.float32(w0d.item()), dw0, mw0)
    assert not np.array_equal(Ed[0].cpu().numpy(), E[0])
    guards.assert_untouched()


@pytest.mark.parametrize("opt,lam", [("AdagradOptimizer", 0.01), ("AdamOptimizer", 0.0)])
def test_fm_bn_train_step_bad_ids(opt, lam, guards):
    """hhfm_fm_train_step_bn: test_gpu_fm_bn.test_partial_fit_replayed_step_by_step's
    replay (float64 gradients of the restatement through the oracle's TF
    optimizer rules, test_gpu_training's bars for variables and slots, its own
    for the moving statistics) on the zeroed batch."""
    from hhfm_amd._native import native
    from oracle import fm_oracle as orc
    from tests import fm_bn_ref as bn
    from tests.test_gpu_fm_bn import NAMES, _model, _ulp
    from tests.test_gpu_training import OPTS, _check_slot, _check_var, _rows
    o = OPTS[opt]
    rng = np.random.default_rng(4)
    nu, ni, k, B, lr = 40, 90, 32, TRAIN_B, 0.1
    X, M = _rows(rng, B, nu, ni, (7, 2, 3))
    zeroed, bad, _, _ = plant(X, _positions(B, 5), M, rng, M - 1)
    m = _model(5, M, k, lr, lam, 1, opt)
    m.set_weights(feature_embeddings=rng.normal(0, 0.1, (M, k)).astype(np.float32),
                  feature_bias=rng.normal(0, 0.01, M).astype(np.float32)[:, None],
                  bias=np.float32(0.02), bn_gamma=rng.normal(1, 0.2, k).astype(np.float32),
                  bn_beta=rng.normal(0, 0.2, k).astype(np.float32))
    st = _arm(m, guards, NAMES, native().fm_train_bn_workspace(B, M, k), B,
              extra=["bn_moving_mean", "bn_moving_variance"])
    u = m.bn_update
    y = rng.integers(0, 2, B).astype(np.float32)[:, None]
    Wg = m.get_weights()
    cur = [Wg["feature_embeddings"], Wg["feature_bias"][:, 0], np.float32(Wg["bias"]),
           Wg["bn_gamma"], Wg["bn_beta"]]
    sl = [st[n].cpu().numpy() for n in NAMES]
    before = _row0(m)
    loss = m.partial_fit({"X": bad, "Y": y})
    Xz = zeroed.astype(np.int64)
    r = bn.fm_bn_step(Xz, y, *cur)
    E64 = cur[0].astype(np.float64)
    ref_loss = r["loss"] + lam * (E64 ** 2).sum() / 2
    assert np.isclose(loss, ref_loss, rtol=1e-5), (loss, ref_loss)
    grads = [r["dE"] + lam * E64, r["dw"], r["dw0"], r["dgamma"], r["dbeta"]]
    rows = [Xz if lam == 0 else None, Xz, None, None, None]
    Wn = m.get_weights()
    got = [Wn["feature_embeddings"], Wn["feature_bias"][:, 0], np.float32(Wn["bias"]),
           Wn["bn_gamma"], Wn["bn_beta"]]
    for n, var, g, s0, rw, gv in zip(NAMES, cur, grads, sl, rows, got):
        var = np.asarray(var, np.float32)
        ref_var, ref_slot = orc.tf_apply(o, var, np.asarray(g, np.float32), s0, lr, 1, rw)
        shape = (1,) if var.ndim == 0 else var.shape
        _check_var(np.asarray(gv).reshape(shape), np.asarray(ref_var).reshape(shape),
                   var.reshape(shape), o, np.asarray(g, np.float32).reshape(shape))
        _check_slot(st[n].cpu().numpy(), ref_slot, o)
    mm_ref, mv_ref = bn.moving_update64(Wg["bn_moving_mean"], Wg["bn_moving_variance"], r["mu"],
                                        r["v"], u)
    tol_m = 1e-5 * u * np.abs(r["x"]).mean(0) + _ulp(Wn["bn_moving_mean"])
    tol_v = 1e-5 * u * ((r["x"] - r["mu"]) ** 2).mean(0) + _ulp(Wn["bn_moving_variance"])
    assert np.all(np.abs(Wn["bn_moving_mean"] - mm_ref) <= tol_m)
    assert np.all(np.abs(Wn["bn_moving_variance"] - mv_ref) <= tol_v)
    _done(m, guards, before)


def _hhfm_batch(rng, layout, nu, ni):
    """-> zeroed and bad (X, Neg), fd, td, M: bad ids in the user, item, first
    and last field columns and in the negatives (first, last, a whole row)."""
    from tests.test_gpu_training import HHFM_LAYOUTS, _rows
    cards, td = HHFM_LAYOUTS[layout]
    B, NG = TRAIN_B, 10
    X, M = _rows(rng, B, nu, ni, cards, td)
    Neg = rng.integers(nu, nu + ni, (B, NG))
    Xz, Xb, _, _ = plant(X, _positions(B, X.shape[1]), M, rng, M - 1)
    npos = [(0, 0), (B - 1, NG - 1), (B // 2, 3), (B // 2, 4)] + [(B - 3, j) for j in range(NG)]
    Nz, Nb, _, _ = plant(Neg, npos, M, rng, M - 1)
    return (Xz, Nz), (Xb, Nb), len(cards), td, M


def _hhfm_data(X, Neg, fd, td):
    data = {"X": X[:, :2], "Y": Neg, "F1": X[:, 2:2 + fd]}
    if td:
        data["F2"] = X[:, 2 + fd:]
    return data


@pytest.mark.parametrize("layout,opt,lam", [("frappe", "AdagradOptimizer", 0.01),
                                            ("jiaju", "AdamOptimizer", 0.0),
                                            ("jiaju", "MomentumOptimizer", 0.01)])
def test_hhfm_train_step_bad_ids(layout, opt, lam, guards):
    """hhfm_hhfm_train_step (hhfm_train_rows: user, item, negatives, context
    and time rows all written by id).  test_gpu_training._hhfm_replay's bars."""
    from tests.test_gpu_training import OPTS, _hhfm_model, _hhfm_replay
    rng = np.random.default_rng(6)
    nu, ni, k = 40, 90, 32
    (Xz, Nz), (Xb, Nb), fd, td, M = _hhfm_batch(rng, layout, nu, ni)
    m = _hhfm_model(rng, layout, opt, lam, nu, ni, k)
    _arm(m, guards, ["feature_embeddings"])
    _feed(m, **_hhfm_data(Xb, Nb, fd, td))
    before = _row0(m)
    _hhfm_replay(m, Xz.astype(np.int64), Nz.astype(np.int64), OPTS[opt], lam, 1)
    _done(m, guards, before)


@pytest.mark.parametrize("two_way", [False, True], ids=["pool", "pool2"])
@pytest.mark.parametrize("layout,opt,lam", [("frappe", "AdagradOptimizer", 0.01),
                                            ("jiaju", "AdamOptimizer", 0.0)])
def test_hhfm_pooled_train_step_bad_ids(layout, opt, lam, two_way, guards):
    """hhfm_hhfm_train_step_pool / _pool2 under (mean, max, sum) (and (max, mean,
    sum) products): the replay of test_pooled_partial_fit_replayed /
    test_two_way_partial_fit_replayed, with their bars, on the zeroed batch."""
    from tests import hhfm_pool_ref as pr
    from tests import hhfm_two_way_ref as tw
    from tests.test_gpu_hhfm_pool import _our
    from tests.test_gpu_training import OPTS, _check_slot, _check_var, _slots_of
    rng = np.random.default_rng(21)
    nu, ni, k = 40, 90, 32
    (Xz, Nz), (Xb, Nb), fd, td, M = _hhfm_batch(rng, layout, nu, ni)
    ctx, tim = (2, 2 + fd), ((2 + fd, 2 + fd + td) if td else (0, 0))
    triple, triple2 = ("mean", "max", "sum"), ("max", "mean", "sum")
    kw = dict(pooling=triple, two_way=True, pooling2=triple2) if two_way else dict(pooling=triple)
    m = _our(fd, td, M, nu, ni, k, lam=lam, opt=opt, **kw)
    m.set_weights(feature_embeddings=rng.normal(0, 0.2 if two_way else 0.01,
                                                (M, k)).astype(np.float32))
    _arm(m, guards, ["feature_embeddings"])
    o = OPTS[opt]
    E = m.get_weights()["feature_embeddings"]
    (accE,) = _slots_of(m, ["feature_embeddings"], o, [E])
    before = _row0(m)
    loss = m.partial_fit(_hhfm_data(Xb, Nb, fd, td))
    Xz, Nz = Xz.astype(np.int64), Nz.astype(np.int64)
    if two_way:
        rl, E1, acc1 = tw.train_step2(Xz, Nz, E, accE, 0.1, lam, ctx, tim, triple, triple2, o, 1)
        _, Eg, _ = tw.train_step2(Xz, Nz, E, None, 1.0, lam, ctx, tim, triple, triple2, "sgd")
    else:
        rl, E1, acc1 = pr.train_step(Xz, Nz, E, accE, 0.1, lam, ctx, tim, triple, o, 1)
        _, Eg, _ = pr.train_step(Xz, Nz, E, None, 1.0, lam, ctx, tim, triple, "sgd")
    assert np.isclose(loss, rl, rtol=1e-5)
    _check_var(m.get_weights()["feature_embeddings"], E1, E, o, E - Eg)
    _check_slot(m._train_state["feature_embeddings"].cpu().numpy(), acc1, o)
    _done(m, guards, before)


@pytest.mark.parametrize("k,A,ctx,opt", [(32, 32, (7, 2, 3), "AdagradOptimizer"),
                                         (16, 32, (7, 2, 3), "MomentumOptimizer"),
                                         (16, 8, (5, 4, 6, 3, 7, 2, 2), "AdagradOptimizer")])
def test_afm_train_step_bad_ids(k, A, ctx, opt, guards):
    """hhfm_afm_train_step(_ex at keep 1, 1), λ_attention = 100: F = 5 and
    F = 9 (36 pairs).  test_gpu_training._afm_replay's bars."""
    from hhfm_amd._native import native
    from tests.test_gpu_training import AFM_NAMES, OPTS, _afm_model, _afm_replay, _rows
    rng = np.random.default_rng(k + A)
    nu, ni, B = 40, 90, TRAIN_B
    X, M = _rows(rng, B, nu, ni, ctx)
    F = X.shape[1]
    zeroed, bad, _, _ = plant(X, _positions(B, F), M, rng, M - 1)
    m = _afm_model(rng, k, A, M, F, opt, nu, ni)
    _arm(m, guards, AFM_NAMES, native().afm_train_workspace(B, F, k, A, M), B)
    _feed(m, X=bad)
    before = _row0(m)
    y = rng.choice([1.0, -1.0], B).astype(np.float32)[:, None]
    _afm_replay(m, zeroed.astype(np.int64), y, OPTS[opt], 1)
    _done(m, guards, before)


@pytest.mark.parametrize("keep", [(0.7, 0.6)])
def test_afm_train_step_dropout_bad_ids(keep, guards):
    """hhfm_afm_train_step_ex with both dropout sites live, through the binding:
    one SGD step at lr 1, λ 0 against dropout_ref.afm_grad64_dropout on the
    zeroed batch, at the bar of test_gpu_dropout's AFM gradient test (rtol 1e-5,
    atol 1e-4 of the variable's largest update; the loss 1e-5 relative).  The
    zeroed rows keep every pre-activation further from relu's kink than fp32
    can move it (asserted), as that test's rows do."""
    from hhfm_amd._native import native
    from tests import dropout_ref as dr
    from tests.test_gpu_dropout import AFM_NAMES, SGD
    nat = native()
    F, k, A, B, seed = 5, 16, 16, TRAIN_B, 2016 | 5 << 32
    rng = np.random.default_rng(501)
    M = F * dr.AFM_VOCAB
    base = np.arange(F) * dr.AFM_VOCAB
    gl = np.sqrt(2.0 / (A + k))
    par = (rng.normal(0, 0.3, (M, k)).astype(np.float32), rng.normal(0, 0.1, M).astype(np.float32),
           np.float32(0.02), rng.normal(0, gl, (k, A)).astype(np.float32),
           rng.normal(0, gl, A).astype(np.float32), rng.normal(0, 1, A).astype(np.float32),
           rng.normal(1, 0.2, k).astype(np.float32))
    X = (base + rng.integers(0, dr.AFM_VOCAB, (B, F))).astype(np.int32)
    pos = _positions(B, F)
    for _ in range(100):                      # dropout_ref.afm_case's redraw, on the zeroed rows
        zeroed, bad, _, held = plant(X, pos, M, np.random.default_rng(9), M - 1)
        close = dr.afm_relu_margin(zeroed, par[0], par[3], par[4]) < dr.afm_margin_needed(k)
        if not close.any():
            break
        assert not close[held].any(), "a row of bad ids sits on relu's kink: change the seed"
        X[close] = base + rng.integers(0, dr.AFM_VOCAB, (int(close.sum()), F))
    assert not close.any()
    y = rng.choice([1.0, -1.0], B).astype(np.float32)
    b1 = dr.binary(seed, dr.SITE_AFM_ATT, B, F * (F - 1) // 2, keep[0])
    b2 = dr.binary(seed, dr.SITE_AFM_VEC, B, k, keep[1])
    ref_loss, grads = dr.afm_grad64_dropout(zeroed, y, par, b1, b2, keep)
    dev = [guards.table(_dev(np.asarray(v, np.float32).reshape(-1))) for v in par]
    ws = guards.workspace(nat.afm_train_workspace(B, F, k, A, M), "cuda")
    loss = torch.zeros(1, device="cuda")
    Xd, yd = _dev(bad), _dev(y)
    nat.afm_train_step_ex(Xd.data_ptr(), yd.data_ptr(), B, F, *[t.data_ptr() for t in dev[:3]], M,
                          k, A, *[t.data_ptr() for t in dev[3:]], 1.0, 0.0, SGD, keep[0], keep[1],
                          seed, [], ws.data_ptr(), ws.numel(), loss.data_ptr(), _stream())
    assert np.isclose(float(loss.item()), ref_loss, rtol=1e-5), (float(loss.item()), ref_loss)
    for n, old, t, g in zip(AFM_NAMES, par, dev, grads):
        got = t.cpu().numpy().reshape(np.shape(old))
        ref = np.asarray(old, np.float64) - np.asarray(g, np.float64).reshape(np.shape(old))
        step = np.abs(ref - old).max()
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-4 * step + 1e-9), n
    assert not np.array_equal(dev[0].cpu().numpy()[:k], par[0][0])
    guards.assert_untouched()


@pytest.mark.parametrize("opt", [0, 3], ids=["adagrad", "adam"])
def test_afm_noatt_train_step_bad_ids(opt, guards):
    """hhfm_afm_noatt_train_step through the binding: the replay and the bars of
    test_gpu_afm0.test_optimizer_steps_match_the_replay on the zeroed batch."""
    from tests import afm0_ref as ar
    from tests.test_gpu_afm0 import OPT_NAME, _check_var, _Step
    o = OPT_NAME[opt]
    rng = np.random.default_rng(60 + opt)
    M, F, k, B = 120, 5, 20, TRAIN_B
    Wt = ar.weights(5, M, k)
    Wt["E"] = (Wt["E"] * np.float32(0.5)).astype(np.float32)
    s = _Step(Wt, opt)
    s.par = [guards.table(p) for p in s.par]
    s.acc = [guards.table(a) for a in s.acc]
    s.ws = guards.workspace(s.ws.numel(), s.ws.device)
    X = rng.integers(0, M // 2, (B, F)).astype(np.int32)
    zeroed, bad, _, _ = plant(X, _positions(B, F), M, rng, M - 1)
    y = rng.choice([-1.0, 1.0], B).astype(np.float32)
    cur, sl = s.weights(), s.slots()
    rl, W1, S1, Gr = ar.step(zeroed, y, cur, sl, 0.05, o, 1, None, 1.0)
    loss = s.step(bad, y, 0.05, 1.0, 2016 | 1 << 32)
    assert np.isclose(loss, rl, rtol=1e-5, atol=0.0), (loss, rl)
    got, gsl = s.weights(), s.slots()
    for n in ar.NAMES:
        _check_var(np.atleast_1d(got[n]), np.atleast_1d(W1[n]), np.atleast_1d(cur[n]), o,
                   np.atleast_1d(Gr[n]))
        ref = np.asarray(S1[n], np.float32).reshape(-1)
        assert np.allclose(gsl[n].reshape(-1), ref, rtol=1e-5,
                           atol=1e-5 * np.abs(ref).max() + 1e-12), n
    assert not np.array_equal(got["E"][0], cur["E"][0])
    guards.assert_untouched()


@pytest.mark.parametrize("opt", ["AdagradOptimizer", "AdamOptimizer"])
def test_dfm_train_step_bad_ids(opt, guards):
    """hhfm_dfm_train_step through test_gpu_training._DfmBinding (Adagrad is
    what DeepFM.partial_fit runs), l2_reg = 0.01.  _dfm_replay's bars."""
    from hhfm_amd._native import native
    from hhfm_amd.DFM import DeepFM
    from tests.test_gpu_training import OPTS, _DfmBinding, _dfm_replay, _rows
    rng = np.random.default_rng(16 + TRAIN_B)
    nu, ni, k, layers, B = 40, 90, 16, [24, 40, 24], TRAIN_B
    X, M = _rows(rng, B, nu, ni, (7, 2, 3))
    zeroed, bad, _, _ = plant(X, _positions(B, 5), M, rng, M - 1)
    m = DeepFM(nu, ni, M, 5, k, layers, None, 0.01, 0, 0.01)
    m.validate = False
    o = OPTS[opt]
    drv = _DfmBinding(m, o, 0.01, 0.01)
    for n in drv.names:
        m.weights[n] = guards.table(m.weights[n])
        drv.slots[n] = guards.table(drv.slots[n])
    drv.ws = guards.workspace(native().dfm_train_workspace(B, 5, k, M, layers), m.device)
    drv.ws_rows = B
    before = _row0(m)
    y = rng.choice([1.0, -1.0], B).astype(np.float32)[:, None]
    _dfm_replay(m, lambda Xb, yb: drv.step(bad, yb), drv.slot, zeroed.astype(np.int64), y, o,
                0.01, 0.01, 1)
    _done(m, guards, before)


@pytest.mark.parametrize("name", ["fm_mse", "deep_mse", "both_logloss"])
def test_dfm_head_train_step_bad_ids(name, guards):
    """hhfm_dfm_train_step_head: test_gpu_dfm_heads._Step and its _replay (one
    Adagrad step, λ = 0.05) with the bad batch fed to the step and the zeroed
    one to the oracle."""
    from hhfm_amd._native import native
    from tests import dfm_heads_ref as hr
    from tests.test_gpu_dfm_heads import _replay, _Step, _train_case
    head = hr.head_word(*hr.HEADS[name])
    rng = np.random.default_rng(40 + head)
    B, k, layers = TRAIN_B, 16, [24, 40, 24]
    X, y, W = _train_case(rng, B, k, layers, head, labels=(1.0, -1.0))
    M = W[0].shape[0]
    zeroed, bad, _, _ = plant(X, _positions(B, X.shape[1]), M, rng, M - 1)
    s = _Step(*W, head)
    s.par = [guards.table(p) for p in s.par]
    s.slots = [guards.table(a) for a in s.slots]
    s.ws = guards.workspace(native().dfm_train_workspace(B, X.shape[1], k, M, s.ws_dims), "cuda")
    s.sc, s.ws_rows = None, B
    real = s.step
    s.step = lambda Xb, yb, lr, lam: real(bad, yb, lr, lam)
    E0 = s.par[0][0].clone()
    _replay(s, zeroed, y, 0.05, 0.05, 1, B)
    assert not torch.equal(_ibits(s.par[0][0]), _ibits(E0))
    guards.assert_untouched()


# ---------------------------------------------------------------------------
# The catalog window flush against the end (and the start) of the table
# ---------------------------------------------------------------------------
SMALL = (31, 32, 33)                    # the 32-item MFMA tile (kTile; AFM's item tile)
RANGE = (1023, 1024, 1025)              # the fused small-catalog kernel's 8 x 4-tile range
GEMM = (63, 64, 65, 127, 128, 129)      # the 64-item finish wave and the 128-wide GEMM tile
STREAM = tuple(16384 + c for c in SMALL)     # past the dense limit: catalog_main streams
RING = tuple(65536 + c for c in SMALL)       # a seeded catalog: catalog_ring


def _hhfm_cat(mode, plans=(), **kw):
    def build(rng, k):
        from hhfm_amd import ops
        plan = _plan(plans)
        m = getattr(ops, mode)

        def score(q, E, w, begin, count):
            return ops.catalog_topk(q, E, m, min(5, count), begin, count, 0,
                                    w if mode == "MODE_FM" else None, 0, (2, 5), (0, 0),
                                    plan=plan, **kw)
        return score
    return build


def _noatt_cat(plans=()):
    def build(rng, k):
        from hhfm_amd import ops
        P = _dev(rng.normal(1, 0.2, k).astype(np.float32))
        plan = _plan(plans)
        return lambda q, E, w, begin, count: ops.afm_noatt_catalog_topk(
            q, E, w, 0.02, P, begin, count, min(5, count), 0, plan=plan)
    return build


def _afm_cat(plans=()):
    def build(rng, k):
        from hhfm_amd import ops
        Wt, b, p, P = _afm_weights(rng, k, 32)
        plan = _plan(plans)
        return lambda q, E, w, begin, count: ops.afm_catalog_topk(
            q, E, w, Wt, b, p, P, begin, count, min(5, count), 0, plan=plan)
    return build


def _dfm_cat(mlp, proj):
    def build(rng, k):
        from hhfm_amd import ops
        Wt, bias, dims, mdt, Wp, bp = _dfm_weights(rng, 5, k, [33, 20], mlp)
        return lambda q, E, w, begin, count: ops.dfm_catalog_topk(
            q, E, w, Wt, bias, dims, Wp, bp, 1, begin, count, min(5, count), 0, 1 << 20,
            proj=proj)
    return build


def _cars2_cat(plans=()):
    def build(rng, k):
        from hhfm_amd import ops
        from tests import cars2_ref as cr
        Wt = cr.weights(7, 8, 5, k)
        prepared = ops.cars2_prepare(*(_dev(Wt[n]) for n in ("Context", "W", "Z", "A", "B")))
        plan = _plan(plans)
        return lambda q, E, w, begin, count: ops.cars2_catalog_topk(
            torch.stack([q[:, 0], q[:, 2] % 5], 1).contiguous(), E, prepared, 5, min(5, count),
            begin, count, 0, plan=plan)
    return build


POOL1, POOL2 = ("max", "mean", "sum"), ("mean", "sum", "max")
# id: (builder, k, table dtypes, item counts)
WINDOW_CASES = {
    "hhfm-catalog_fused": (_hhfm_cat("MODE_HHFM"), 16, ("f32", "bf16"), SMALL + RANGE),
    "fm-catalog_fused": (_hhfm_cat("MODE_FM"), 16, ("f32", "bf16"), SMALL + RANGE),
    "hhfm-catalog_main-store": (_hhfm_cat("MODE_HHFM", ("PLAN_STORE",)), 16, ("f32", "bf16"), SMALL),
    "fm-catalog_main-store": (_hhfm_cat("MODE_FM", ("PLAN_STORE",)), 16, ("f32", "bf16"), SMALL),
    "fm-catalog_main-store-exact": (_hhfm_cat("MODE_FM", ("PLAN_STORE", "PLAN_EXACT_FP32")), 16,
                                    ("f32", "bf16"), SMALL),
    "hhfm-gemm": (_hhfm_cat("MODE_HHFM", ("PLAN_GEMM",)), 16, ("f32", "bf16"), GEMM),
    "fm-gemm": (_hhfm_cat("MODE_FM", ("PLAN_GEMM",)), 16, ("f32", "bf16"), GEMM),
    "hhfm-catalog_main-stream": (_hhfm_cat("MODE_HHFM"), 16, ("f32", "bf16"), STREAM),
    "fm-catalog_main-stream": (_hhfm_cat("MODE_FM"), 16, ("f32", "bf16"), STREAM),
    "hhfm-catalog_ring-f32": (_hhfm_cat("MODE_HHFM"), 64, ("f32",), RING),
    "fm-catalog_ring-bf16": (_hhfm_cat("MODE_FM"), 128, ("bf16",), RING),
    "fm-catalog_ring-alt": (_hhfm_cat("MODE_FM", ("PLAN_RING_ALT",)), 64, ("f32",), RING),
    "hhfm-catalog_main-seeded": (_hhfm_cat("MODE_HHFM", ("PLAN_NO_RING",)), 64, ("f32",), RING),
    "pooled-catalog_fused": (_hhfm_cat("MODE_HHFM", pooling=POOL1), 16, ("f32", "bf16"), SMALL),
    "pooled-store": (_hhfm_cat("MODE_HHFM", ("PLAN_STORE",), pooling=POOL1), 16, ("f32", "bf16"),
                     SMALL),
    "two-way-store": (_hhfm_cat("MODE_HHFM", pooling=POOL1, pooling2=POOL2), 16, ("f32", "bf16"),
                      SMALL),
    "two-way-stream": (_hhfm_cat("MODE_HHFM", pooling=POOL1, pooling2=POOL2), 16, ("f32",), STREAM),
    "afm_noatt-store": (_noatt_cat(), 16, ("f32", "bf16"), SMALL),
    "afm_noatt-gemm": (_noatt_cat(("PLAN_GEMM",)), 16, ("f32", "bf16"), GEMM),
    "afm_noatt-stream": (_noatt_cat(), 16, ("f32",), STREAM),
    "afm_cat_w": (_afm_cat(), 32, ("f32", "bf16"), SMALL),
    "afm_cat_fused": (_afm_cat(("PLAN_PER_FIELD",)), 32, ("f32", "bf16"), SMALL),
    "afm_cat_fused-exact": (_afm_cat(("PLAN_EXACT_FP32",)), 32, ("f32", "bf16"), SMALL),
    "afm_cat_finish-gemm": (_afm_cat(("PLAN_GEMM",)), 32, ("f32", "bf16"), GEMM),
    "dfm_catalog-fused-bf16mlp": (_dfm_cat("bf16", False), 16, ("f32", "bf16"), GEMM),
    "dfm_catalog-item": (_dfm_cat("bf16", "item"), 16, ("f32", "bf16"), GEMM),
    "dfm_catalog-fused_f32": (_dfm_cat("f32", False), 16, ("f32", "bf16"), GEMM),
    "dfm_catalog-f32s": (_dfm_cat("f32", True), 16, ("f32", "bf16"), GEMM),
    "cars2-store": (_cars2_cat(), 16, ("f32", "bf16"), SMALL),
    "cars2-gemm": (_cars2_cat(("PLAN_GEMM",)), 16, ("f32", "bf16"), GEMM),
    "cars2-stream": (_cars2_cat(), 16, ("f32",), STREAM),
}


@pytest.mark.parametrize("case", sorted(WINDOW_CASES))
def test_catalog_window_at_the_table_end(case, guards):
    """Every catalog kernel walks item_row_begin + item in tiles and guards a
    ragged last tile itself.  The window [M − count, M) ends at the table's
    last row, with quiet-NaN pads behind E and w: the outputs are finite and
    bitwise those of the same call on a table with 4 x 128 more real rows
    behind the window (the rows behind the window influence nothing).  Then the
    window [0, count) against the front pad: finite.  Item counts one below,
    at and one above the tile widths of the kernel the id names."""
    build, k, tdts, counts = WINDOW_CASES[case]
    rng = np.random.default_rng(len(case) + k)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(k + len(case))
    score = build(rng, k)
    nu, nq, tail = 8, 5, 4 * 128
    for tdt in tdts:
        dt = torch.bfloat16 if tdt == "bf16" else torch.float32
        for count in counts:
            M = nu + count
            full = (torch.randn(M + tail, k, generator=gen, device="cuda") * 0.3).to(dt)
            wfull = torch.randn(M + tail, generator=gen, device="cuda") * 0.1
            E, w = guards.table(full[:M]), guards.table(wfull[:M])
            Ebig, wbig = guards.table(full), guards.table(wfull)
            q = _dev(rng.integers(0, M, (nq, 5)).astype(np.int32))
            end = score(q, E, w, nu, count)
            big = score(q, Ebig, wbig, nu, count)
            front = score(q, E, w, 0, count)
            for s, i in (end, front):
                assert torch.isfinite(s).all(), (tdt, count, "a tile read past the window")
                assert int(i.min()) >= 0 and int(i.max()) < count, (tdt, count)
            assert _same(end, big), (tdt, count, "rows behind the window change the result")
            guards.assert_untouched()
            guards.pairs.clear()
