#!/usr/bin/env python3
"""A/B of K1's LDS-tail kernel (HHFM_FLAG_HOT_TAIL, include/hhfm.h) against
fm_rows_fast in one process, timed with HIP events after warm-up.

  hit    configs[1] as bench.py builds it (2^25 rows, 4.3 GB fp32 table, the
         three context columns in the table's last 12 rows): flags 4 (the
         default kernel) against flags 0 (the automatic rule)
  miss   the same table with all five columns uniform over [0, M): every
         wave leaves the LDS loop in its first iteration (the cliff guard)
  wprice the hit leg's table and rows under the automatic rule (flags 0), with
         `w` and with w=None: what the user / item `w` terms cost this kernel
  --shapes F:k:dtype,...  further Frappe-layout shapes (2^23 rows, 2 M users
         + 2 M items + 12 context ids), the same two flags

Prints one JSON line: median and min ms of `--reps` launches for each leg, and
whether the two kernels' outputs are bit-identical.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from hhfm_amd import ops  # noqa: E402  (a PYTHONPATH copy wins: appended path)

FLAG_NO_HOT = 4


def time_ms(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms))}


def ab(idx, E, w, reps):
    out = {}
    keep = {}
    for name, flags in (("fast_flags4", FLAG_NO_HOT), ("auto_flags0", 0)):
        o = torch.empty(idx.shape[0], dtype=torch.float32, device=idx.device)
        out[name] = time_ms(lambda: ops.fm_score_rows(idx, E, w, 0.0, out=o, flags=flags), reps)
        keep[name] = o
    out["bit_identical"] = bool(torch.equal(keep["fast_flags4"], keep["auto_flags0"]))
    out["auto_over_fast"] = out["auto_flags0"]["median_ms"] / out["fast_flags4"]["median_ms"]
    return out


def w_price(idx, E, w, reps):
    out = {}
    o = torch.empty(idx.shape[0], dtype=torch.float32, device=idx.device)
    for name, ww in (("with_w", w), ("without_w", None)):
        out[name] = time_ms(lambda: ops.fm_score_rows(idx, E, ww, 0.0, out=o, flags=0), reps)
    out["price_ms"] = out["with_w"]["median_ms"] - out["without_w"]["median_ms"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--rows", type=int, default=1 << 25)
    p.add_argument("--shapes", default="", help="extra legs, e.g. 3:16:f32,8:128:bf16")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    res = {}
    idx, E, w, M = bench.make_batch(a.rows, 8 << 20, 8 << 20, 64, 1, dev)
    res["hit"] = ab(idx, E, w, a.reps)
    res["wprice"] = w_price(idx, E, w, a.reps)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    idx = torch.randint(0, M, idx.shape, generator=g, device=dev, dtype=torch.int32)
    res["miss"] = ab(idx, E, w, a.reps)
    del idx, E, w
    torch.cuda.empty_cache()
    for spec in [s for s in a.shapes.split(",") if s]:
        F, k, dt = spec.split(":")
        F, k = int(F), int(k)
        rows, nu = 1 << 23, 2 << 20
        idx, E, w, M = bench.make_batch(rows, nu, nu, k, 1, dev)
        off = 2 * nu
        cols = [idx[:, 0], idx[:, 1]]
        for f in range(2, F):                    # context columns over the last 12 rows
            cols.append(torch.randint(off, M, (rows,), generator=g, device=dev,
                                      dtype=torch.int32))
        idx = torch.stack(cols, 1).contiguous()
        if dt == "bf16":
            E = E.to(torch.bfloat16)
        res[spec] = ab(idx, E, w, a.reps)
        del idx, E, w
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
