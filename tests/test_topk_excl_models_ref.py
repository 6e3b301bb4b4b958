"""Exclusion lists for the AFM, DeepFM and CARS2 catalogs, the parts that need
no GPU: the new entry points are exported and bound, the ABI version stays 6,
``--filter_seen`` parses for the three models, and the numpy identity the GPU
tests (tests/test_gpu_topk_excl_models.py) lean on holds: the filtered top-K is
the plain top-(K + e) with the listed columns removed, first K, whenever every
list has at most e entries inside the range.
"""
import ctypes
import os

import numpy as np

from tests import score_designs as sd
from tests import topk_excl_ref as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hhfm_amd", "lib", "libhhfm.so")

SYMBOLS = ("hhfm_topk_dense_excl", "hhfm_afm_catalog_topk_excl", "hhfm_dfm_catalog_topk_excl",
           "hhfm_cars2_catalog_topk_excl", "hhfm_afm_noatt_catalog_topk_excl")


def test_the_five_entry_points_are_exported_and_bound():
    from hhfm_amd._native import native
    lib = ctypes.CDLL(LIB)
    m = native()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert hasattr(m, name[len("hhfm_"):]), name


def test_abi_version_stays_6():
    from hhfm_amd._native import native
    lib = ctypes.CDLL(LIB)
    lib.hhfm_abi_version.restype = ctypes.c_int
    assert lib.hhfm_abi_version() == 6
    assert native().abi_version() == 6


def test_filter_seen_parses_for_afm_dfm_and_cars2():
    from hhfm_amd import AFM, CARS2, DFM, FM
    fm_help = [a.help for a in _actions(FM) if a.dest == "filter_seen"]
    for mod in (AFM, DFM, CARS2):
        assert mod.parse_args("frappe", 64, 10, []).filter_seen == 0
        assert mod.parse_args("frappe", 64, 10, ["--filter_seen", "1"]).filter_seen == 1
        assert [a.help for a in _actions(mod) if a.dest == "filter_seen"] == fm_help


def _actions(mod):
    """The argparse actions of a model module's parse_args."""
    import argparse
    seen = []
    real = argparse.ArgumentParser.parse_args

    def spy(self, *a, **kw):
        seen.extend(self._actions)
        return real(self, *a, **kw)

    argparse.ArgumentParser.parse_args = spy
    try:
        mod.parse_args("frappe", 64, 10, [])
    finally:
        argparse.ArgumentParser.parse_args = real
    return seen


def test_raw_select_argument_rules_without_a_device():
    """hhfm_topk_dense_excl decides its argument errors before any launch."""
    lib = ctypes.CDLL(LIB)
    f = lib.hhfm_topk_dense_excl
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    f.argtypes = [vp, i64, i32, i64, i32, i32, vp, vp, i32, vp, i32, vp, vp, i64]
    one = ctypes.c_int64(0)
    p = ctypes.addressof(one)
    assert f(None, 0, 100, 100, 5, 0, None, None, 0, None, 0, None, None, 0) == 0     # B = 0
    assert f(None, 4, 100, 100, 5, 0, None, None, 0, None, 0, None, None, 0) == -1    # no excl_ptr
    assert f(None, 4, 100, 100, 5, 0, None, None, 0, None, 0, p, None, -1) == -1      # max_excl < 0
    assert f(None, 4, 100, 100, 5, 0, None, None, 0, None, 0, p, None, 96) == -1      # K + max > N
    assert f(None, 0, 100, 100, 5, 0, None, None, 0, None, 0, p, None, 95) == 0
    assert f(None, 4, 100, 100, 5, 0, None, None, 0, None, 0, p, None, 95) == -1      # no scores
    assert f(None, 4, 100, 100, 5, 0, None, None, 1 << 30, None, 0, p, None, 0) == -1  # plan


def test_overfetch_identity_of_the_numpy_reference():
    """filtered_topk(S, K, lists) == (plain top-(K + e) minus the listed
    columns)[:K] when every list has <= e entries inside the range, on
    matrices with many exact ties, with a shifted range and ids that lie
    outside it."""
    rng = np.random.default_rng(5)
    for trial in range(40):
        B = int(rng.integers(1, 6))
        N = int(rng.integers(30, 400))
        K = int(rng.integers(1, min(N // 3, 20) + 1))
        e = int(rng.integers(0, min(N - K, 44) + 1))
        row_begin = int(rng.integers(0, 50))
        S = rng.integers(0, 6, (B, N)).astype(np.float32)        # six values: ties everywhere
        if trial % 3 == 0:
            S[:] = 1.0
        lists = []
        for b in range(B):
            n_in = int(rng.integers(0, e + 1))
            top = np.argsort(-S[b], kind="stable")[:K + 5]
            pick = np.unique(np.concatenate([rng.choice(top, size=min(n_in, len(top)) // 2,
                                                        replace=False),
                                             rng.choice(N, size=n_in // 2, replace=False)]))[:e]
            outside = np.array([-7, row_begin - 1, row_begin + N, row_begin + N + 9])
            lists.append(np.unique(np.concatenate([pick + row_begin, outside])))
        ws, wi = xr.filtered_topk(S, K, lists, row_begin)
        ps, pi = sd.expected_topk(S, K + e)
        for b in range(B):
            keep = ~np.isin(pi[b] + row_begin, lists[b])
            assert keep.sum() >= K
            assert np.array_equal(wi[b], pi[b][keep][:K])
            assert np.array_equal(sd.bits(ws[b]), sd.bits(ps[b][keep][:K]))
