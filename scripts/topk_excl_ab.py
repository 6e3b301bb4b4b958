"""What the exclusion lists cost: hhfm_catalog_topk_excl against the plain call
on the same route, event-timed and alternating (A, B, A, B, ... windows in one
process), on an MI355X.

  dense      300 and 3,000 queries x the 4,076 distinct items of a Frappe-shape
             split (bench.frappe_shape_dataset draws from 4,082: no Frappe rows
             are shipped), the lists of its positive_feedback with keep_own,
             against the plain call under PLAN_STORE;
  streaming  1,024 queries x 65,536 items, 16 random items per list, against
             the plain call under PLAN_NO_RING (catalog_main behind the seed).

Usage: python scripts/topk_excl_ab.py [out.txt]"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from hhfm_amd import harness, ops  # noqa: E402
from hhfm_amd.NewLoadData import LoadData  # noqa: E402

K, KF, ROUNDS = 20, 64, 15


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps      # us per call


def ab(plain, excl, reps):
    for fn in (plain, excl):
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(window(plain, reps))
        tb.append(window(excl, reps))
    return np.array(ta), np.array(tb)


def line(name, ta, tb, extra=""):
    return ("%-34s plain %8.1f us (min %.1f max %.1f)   excl %8.1f us (min %.1f max %.1f)   "
            "+%.1f us = %+.1f %%  %s" % (name, np.median(ta), ta.min(), ta.max(), np.median(tb),
                                         tb.min(), tb.max(), np.median(tb) - np.median(ta),
                                         100 * (np.median(tb) / np.median(ta) - 1), extra))


def main():
    dev = torch.device("cuda", 0)
    out = ["# exclusion lists: cost against the plain call on the same route (K = %d, k = %d), "
           "medians of %d alternating windows" % (K, KF, ROUNDS),
           "# device (the name the runtime reports; run on an MI355X, gfx950): %s"
           % torch.cuda.get_device_name(dev)]
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as tmp:
        np.random.seed(2016)
        d = LoadData(bench.frappe_shape_dataset(tmp), "frappe_shape")
    ncols = d.Train_data.shape[1] - 1
    pairs = harness.DevicePairSet(d.positive_feedback, ncols - 1, dev)
    test = np.asarray(d.Test_data.values[:, 1:], dtype=np.int64)
    for dtype in (torch.float32, torch.bfloat16):
        E = torch.from_numpy(rng.normal(0, 0.1, (d.features_M, KF)).astype(np.float32)).to(dev)
        E = E.to(dtype)
        for B in (300, 3000):
            rows = torch.from_numpy(test[rng.integers(0, len(test), B)].astype(np.int32)).to(dev)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ops.pf_exclusion_lists(pairs.keys, pairs.codes, rows, 1, keep_own=True)
            t0.record()
            x = ops.pf_exclusion_lists(pairs.keys, pairs.codes, rows, 1, keep_own=True)
            t1.record()
            t1.synchronize()
            lens = (x.ptr[1:] - x.ptr[:-1]).cpu().numpy()
            call = lambda **kw: ops.catalog_topk(rows, E, ops.MODE_HHFM, K, d.n_user, d.n_item, 0,
                                                 None, 0, (2, ncols), (0, 0), **kw)
            ta, tb = ab(lambda: call(plan=ops.PLAN_STORE), lambda: call(exclude=x), 200)
            out.append(line("dense %s B=%d N=%d" % (str(dtype)[6:], B, d.n_item), ta, tb,
                            "lists mean %.1f max %d; building them %.0f us"
                            % (lens.mean(), lens.max(), t0.elapsed_time(t1) * 1e3)))
        N, B = 65536, 1024
        M = 7 + N + 5
        Es = torch.from_numpy(rng.normal(0, 0.1, (M, KF)).astype(np.float32)).to(dev).to(dtype)
        A = torch.from_numpy(np.stack([rng.integers(0, 7, B), np.full(B, 7),
                                       7 + N + rng.integers(0, 3, B),
                                       7 + N + 3 + rng.integers(0, 2, B)], 1).astype(np.int32)).to(dev)
        x = ops.exclusion_lists([7 + rng.choice(N, 16, replace=False) for _ in range(B)], dev)
        call = lambda **kw: ops.catalog_topk(A, Es, ops.MODE_HHFM, K, 7, N, 0, None, 0, (2, 4),
                                             (0, 0), **kw)
        ta, tb = ab(lambda: call(plan=ops.PLAN_NO_RING), lambda: call(exclude=x), 50)
        out.append(line("streaming %s B=%d N=%d" % (str(dtype)[6:], B, N), ta, tb,
                        "16-item lists"))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
