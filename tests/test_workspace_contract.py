"""The workspace contracts' host side (include/hhfm.h, the catalog workspace):
the poisoned-workspace helper of tests/guard_tables.py on a CPU tensor, and
make_plan's region offsets against the zero prefix that no plan may write
(hhfm_debug_catalog_plan; profiles/workspace_contract_map.txt is the map of
who writes and reads each region).  The device side is
tests/test_gpu_workspace_contract.py.
"""
import itertools

import pytest
import torch

from tests import guard_tables as gt

REGIONS = ("off_H", "off_cst", "off_thr", "off_ps", "off_pi", "off_sc", "off_seed_sc",
           "off_seed_s", "off_seed_i")


@pytest.mark.parametrize("fill", gt.POISONS, ids=["ff", "7f"])
@pytest.mark.parametrize("nbytes,prefix", [(1000, 0), (1000, 256), (300, 300), (100, 256), (1, 0)])
def test_poisoned_workspace_layout(nbytes, prefix, fill):
    """Guards of 0xA5 on both sides of exactly nbytes, the first `prefix` bytes
    (clipped to the view) zero, every other byte the fill; pads_untouched sees
    a write on either side and no write inside."""
    view, buf = gt.poisoned_workspace(nbytes, torch.device("cpu"), fill, prefix)
    assert view.dtype == torch.uint8 and view.numel() == nbytes
    assert buf.numel() == nbytes + 2 * gt.WS_GUARD
    assert view.data_ptr() - buf.data_ptr() == gt.WS_GUARD
    z = min(prefix, nbytes)
    assert not view[:z].any()
    assert bool((view[z:] == fill).all())
    assert bool((buf[:gt.WS_GUARD] == gt.WS_FILL).all())
    assert bool((buf[gt.WS_GUARD + nbytes:] == gt.WS_FILL).all())
    assert gt.pads_untouched(buf, view)
    view.fill_(0x11)                                   # the interior is the callee's
    assert gt.pads_untouched(buf, view)
    for at in (gt.WS_GUARD - 1, gt.WS_GUARD + nbytes):
        old = int(buf[at])
        buf[at] = 0
        assert not gt.pads_untouched(buf, view)
        buf[at] = old
    assert gt.pads_untouched(buf, view)


def test_poison_bytes_are_what_their_comment_says():
    import numpy as np
    ff = np.full(8, gt.POISON_FF, np.uint8)
    sf = np.full(8, gt.POISON_7F, np.uint8)
    assert np.isnan(ff.view(np.float32)).all() and ff.view(np.int32)[0] == -1
    assert ff.view(np.uint64)[0] == np.iinfo(np.uint64).max
    assert np.isnan((ff.view(np.uint16).astype(np.uint32) << 16).view(np.float32)).all()   # bf16
    x = sf.view(np.float32)[0]
    assert np.isfinite(x) and x > 3.3e38
    # the bitwise complement of the streaming path's 0x80 hint fill
    assert int(sf.view(np.uint32)[0]) == 0x80808080 ^ 0xffffffff


def test_guards_collects_poisoned_workspaces():
    g = gt.Guards()
    v = g.poisoned(512, torch.device("cpu"), gt.POISON_FF, 64)
    assert len(g.pairs) == 1 and g.pairs[0][0] is v
    assert gt.pads_untouched(g.pairs[0][1], v)


def _plan_grid():
    from hhfm_amd import ops
    plans = (0, ops.PLAN_EXACT_FP32, ops.PLAN_FUSED, ops.PLAN_STORE, ops.PLAN_GEMM,
             ops.PLAN_STORE | ops.PLAN_ONE_WAVE, ops.PLAN_NO_SEED, ops.PLAN_NO_RING,
             ops.PLAN_RING_ALT)
    Bs = (1, 32, 33, 128, 130, 4097, 100_000)
    Ns = (1, 32, 1024, 1025, 4096, 4097, 8193, 16384, 16385, 65535, 65536, 1_000_000)
    ks = (8, 16, 64, 128, 256)
    Ks = (1, 20, 32, 33, 64)
    return itertools.product(Bs, Ns, ks, Ks, plans, (0, 1))


def test_no_catalog_plan_region_lies_in_the_zero_prefix():
    """For a grid of (B, N, k, K, plan, dtype): every region offset make_plan
    reports is at or past HHFM_CATALOG_WS_ZERO, the regions are ordered and
    inside the plan's total, and the size query covers the plan (the fused
    kernel's arrival counters are the prefix's only tenant)."""
    from hhfm_amd._native import native
    nat = native()
    zero = nat.CATALOG_WS_ZERO
    assert zero > 0 and zero % 256 == 0
    n = 0
    for B, N, k, K, plan, dtype in _plan_grid():
        if K > N:
            continue
        p = nat.debug_catalog_plan(B, N, k, K, plan, dtype)
        offs = [p[r] for r in REGIONS]
        assert min(offs) >= zero, (B, N, k, K, plan, dtype, p)
        assert offs == sorted(offs) and offs[-1] <= p["total"], (B, N, k, K, plan, dtype, p)
        assert p["off_H"] == zero                      # nothing but the counters before H
        assert p["total"] <= nat.catalog_topk_workspace(B, N, k, K), (B, N, k, K, plan, dtype)
        n += 1
    assert n > 10_000


@pytest.mark.parametrize("N,fS", [(1024, 1), (1025, 2), (4096, 4), (4097, 5), (16384, 16)])
def test_the_fused_range_counts_the_gpu_tests_rely_on(N, fS):
    """tests/test_gpu_workspace_contract.py names its catalog sizes after the
    fused kernel's range count S = p.fS; the streaming sizes after the dense
    limit and the threshold seed."""
    from hhfm_amd._native import native
    nat = native()
    for B in (1, 32, 33, 130):
        for k, dtype in ((16, 0), (64, 1)):
            p = nat.debug_catalog_plan(B, N, k, 20, 0, dtype)
            assert p["dense"] == 1 and p["fS"] == fS
    for B in (1, 32, 33, 130):
        for k, dtype in ((16, 0), (64, 1), (64, 0), (128, 1)):
            p = nat.debug_catalog_plan(B, 16385, k, 20, 0, dtype)
            assert p["dense"] == 0 and p["seed_n"] == 0 and p["S"] > 1
            p = nat.debug_catalog_plan(B, 65536, k, 20, 0, dtype)
            assert p["dense"] == 0 and p["seed_n"] == 4096
            assert p["S"] > 1 and p["rS0"] > 1 and p["rS1"] > 1
            p = nat.debug_catalog_plan(B, 65535, k, 20, 0, dtype)
            assert p["seed_n"] == 0                    # 65,536 is the smallest seeded catalog
