"""Exclusion lists without a GPU: the numpy restatement (tests/topk_excl_ref.py)
against brute force, and the new entry points' host side — exported symbols,
the list builder's size query and the argument checks that come back before
anything touches a device."""
import ctypes
import os

import numpy as np

from tests import topk_excl_ref as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hhfm_amd", "lib", "libhhfm.so")
EINVAL = -1


def _pf(rng, n_keys=40, n_items=60, item_lo=100):
    """key (user, ctx) -> set of item ids; some keys hold an empty set."""
    pf = {}
    for n in range(n_keys):
        key = (int(rng.integers(0, 12)), int(rng.integers(200, 206)))
        size = 0 if n % 7 == 0 else int(rng.integers(1, 25))
        pf.setdefault(key, set()).update(
            int(x) for x in rng.integers(item_lo, item_lo + n_items, size))
    return pf


def test_lists_from_pf_match_brute_force():
    rng = np.random.default_rng(5)
    pf = _pf(rng)
    keys = list(pf)
    rows = []
    for n in range(200):
        if n % 5 == 0:      # a key positive_feedback does not know
            u, c = 50 + n, 300
        else:
            u, c = keys[int(rng.integers(0, len(keys)))]
        own = sorted(pf.get((u, c), ()))
        # the own item: a positive of the key on every third row where it has one
        item = own[n % len(own)] if own and n % 3 == 0 else int(rng.integers(100, 160))
        rows.append((u, item, c))
    rows = np.asarray(rows, np.int64)
    assert any(len(pf[k]) == 0 for k in keys)
    for keep_own in (False, True):
        got = xr.lists_from_pf(pf, rows, 1, keep_own)
        dropped = 0
        for row, lst in zip(rows, got):
            want = [it for it in range(100, 160) if it in pf.get((row[0], row[2]), ())
                    and not (keep_own and it == row[1])]
            assert lst.tolist() == want
            assert np.all(np.diff(lst) > 0)
            dropped += int(row[1]) in pf.get((row[0], row[2]), ())
        assert dropped > 10
        ptr, flat, longest = xr.csr(got)
        assert ptr[0] == 0 and ptr[-1] == len(flat) and longest == max(len(x) for x in got)
        assert all(a.tolist() == b.tolist() for a, b in zip(xr.uncsr(ptr, flat), got))


def test_filtered_topk_matches_full_sort():
    rng = np.random.default_rng(6)
    B, N, K, row_begin = 9, 300, 20, 1000
    scores = rng.integers(-4, 5, (B, N)).astype(np.float32)      # heavy ties
    lists = []
    for b in range(B):
        inside = rng.choice(N, size=int(rng.integers(0, 60)), replace=False) + row_begin
        outside = np.array([-3, 5, row_begin - 1, row_begin + N, 2 ** 31 - 1])
        lists.append(np.unique(np.concatenate([inside, outside])))
    for lo, cnt, g in ((0, None, 0), (37, 201, 500)):
        got_s, got_i = xr.filtered_topk(scores, K, lists, row_begin, lo, cnt, g)
        n = N - lo if cnt is None else cnt
        for b in range(B):
            pairs = sorted((-float(scores[b, lo + i]), i) for i in range(n)
                           if row_begin + lo + i not in set(lists[b].tolist()))[:K]
            assert got_i[b].tolist() == [g + i for _, i in pairs]
            assert got_s[b].tolist() == [-s for s, _ in pairs]
    # empty lists: the plain order
    s0, i0 = xr.filtered_topk(scores, K, [[]] * B, row_begin)
    assert np.array_equal(i0, np.argsort(-scores, axis=1, kind="stable")[:, :K])


def test_exclusion_entry_points_are_exported_and_sized():
    """Fails without the feature: the three symbols and the host size query."""
    lib = ctypes.CDLL(LIB)
    for n in ("hhfm_catalog_topk_excl", "hhfm_pf_exclusion_lists",
              "hhfm_pf_exclusion_lists_workspace"):
        assert hasattr(lib, n), n
    f = lib.hhfm_pf_exclusion_lists_workspace
    f.argtypes = [ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t)]
    small, large = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert f(0, ctypes.byref(small)) == 0 and small.value >= 8
    assert f(3000, ctypes.byref(large)) == 0 and large.value >= 3001 * 8
    assert f(-1, ctypes.byref(large)) == EINVAL
    assert f(10, None) == EINVAL
    from hhfm_amd._native import native
    m = native()
    assert m.pf_exclusion_lists_workspace(300) >= 301 * 8
    assert hasattr(m, "catalog_topk_excl") and hasattr(m, "pf_exclusion_lists")
    assert m.abi_version() == 6


def _excl(lib):
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    f = lib.hhfm_catalog_topk_excl
    f.argtypes = [vp, i64, i32, i32, i32, i32, i32, i32, i32, vp, i64, i32, i32, vp, i32, i32,
                  i32, i32, vp, vp, vp, ctypes.c_size_t, i32, i32, vp, vp, vp, vp, i64]
    return f


def test_exclusion_argument_checks_without_device():
    """K + max_excl > item_count, max_excl < 0 and NULL lists with B > 0 are
    HHFM_EINVAL from the host-side checks, before any pointer is read."""
    f = _excl(ctypes.CDLL(LIB))

    def call(B, K, max_excl, item_count=100, ptr=8, mode=1, pooling=0):
        p = 8 if B else None      # never read: every case returns from the host checks
        return f(p, B, 4, mode, 0, 2, 4, 0, 0, p, 1000, 64, 0, None, 10, item_count, 0, K,
                 p, p, p, 1 << 20, 0, pooling, None, None, ptr if B else None, p, max_excl)

    assert call(0, 20, 80) == 0                      # K + max_excl == item_count: fine
    assert call(0, 20, 81) == EINVAL
    assert call(0, 20, -1) == EINVAL
    assert call(0, 64, 37) == EINVAL
    assert call(0, 20, 2 ** 40) == EINVAL
    assert call(5, 20, 81) == EINVAL
    assert call(5, 20, 10, ptr=None) == EINVAL       # NULL excl_ptr with B > 0
    assert call(0, 20, 10, mode=0, pooling=1) == EINVAL     # FM takes no pooling
