"""Event-times of HHFM scoring with MAX / MEAN pooling beside sum pooling, one
process, the modes alternated (sum, max, mean; four runs each):

  rows     ops.hybrid_score_rows at 2^23 Frappe-layout rows (F = 5), k = 64
           fp32 and k = 128 bf16; and at 2^22 rows of the F = 10 layout
           (5 context + 3 time columns, k = 64 fp32), where the pooled kernel
           holds 2 waves per SIMD against the sum kernel's 3
           (profiles/hhfm_pool_resources.txt)
  catalog  ops.catalog_topk, 300 and 3,000 queries over the Frappe catalog
           (4,082 items, k = 64 fp32, top-20): the fused small-catalog kernel

A run is the mean of `reps` back-to-back calls between two events, after a
warm-up.  Per case: each mode's four runs, the sum kernel's own spread
(max / min of its runs) and the pooled / sum ratio of the medians.
usage: python scripts/hhfm_pool_time.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hhfm_amd import ops  # noqa: E402

MODES = [("sum", None), ("max", ("max", "max", "max")), ("mean", ("mean", "mean", "mean"))]
RUNS = 4


def rows_of(rng, B, nu, ni, cards, td):
    cols = [rng.integers(0, nu, B), rng.integers(nu, nu + ni, B)]
    o = nu + ni
    for c in cards:
        cols.append(rng.integers(o, o + c, B))
        o += c
    for _ in range(td):
        cols.append(rng.integers(nu, nu + ni, B))
    return torch.from_numpy(np.stack(cols, 1).astype(np.int32)).cuda(), o


def run_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(make, reps, lines, title, unit=1.0, name="ms"):
    """make(pooling) -> a call; RUNS rounds over the modes in turn."""
    fns = {m: make(p) for m, p in MODES}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {m: [] for m, _ in MODES}
    for _ in range(RUNS):
        for m, _ in MODES:
            t[m].append(run_ms(fns[m], reps) * unit)
    med = {m: statistics.median(v) for m, v in t.items()}
    lines.append(title)
    for m, _ in MODES:
        lines.append(f"  {m:5s} {name}: " + "  ".join(f"{x:9.4f}" for x in t[m])
                     + f"   median {med[m]:.4f}")
    lines.append(f"  sum's own spread (max / min of its runs): {max(t['sum']) / min(t['sum']):.4f}")
    for m in ("max", "mean"):
        lines.append(f"  {m} / sum (medians): {med[m] / med['sum']:.4f}")
    lines.append("")


def main():
    rng = np.random.default_rng(0)
    lines = ["# scripts/hhfm_pool_time.py: pooled against sum, modes alternated in one process",
             f"# device: {torch.cuda.get_device_name(0)}", ""]
    nu, ni = 957, 4082
    for title, B, cards, td, k, dt in (
            ("rows, F = 5 (Frappe), k = 64 fp32, 2^23 rows", 1 << 23, (7, 2, 3), 0, 64, torch.float32),
            ("rows, F = 5 (Frappe), k = 128 bf16, 2^23 rows", 1 << 23, (7, 2, 3), 0, 128,
             torch.bfloat16),
            ("rows, F = 10 (5 ctx + 3 time), k = 64 fp32, 2^22 rows", 1 << 22, (5, 4, 6, 3, 7), 3,
             64, torch.float32)):
        X, M = rows_of(rng, B, nu, ni, cards, td)
        E = torch.from_numpy(rng.normal(0, 0.01, (M, k)).astype(np.float32)).cuda().to(dt)
        out = torch.empty(B, dtype=torch.float32, device="cuda")
        fd = len(cards)
        ctx, tim = (2, 2 + fd), ((2 + fd, 2 + fd + td) if td else (0, 0))
        alternate(lambda p: (lambda: ops.hybrid_score_rows(X, E, 0, 1, ctx, tim, out=out,
                                                           pooling=p)), 10, lines, title)
        del X, E, out
    X, M = rows_of(rng, 3000, nu, ni, (7, 2, 3), 0)
    E = torch.from_numpy(rng.normal(0, 0.01, (M, 64)).astype(np.float32)).cuda()
    for nq in (300, 3000):
        q = X[:nq].contiguous()
        alternate(lambda p: (lambda: ops.catalog_topk(q, E, ops.MODE_HHFM, 20, nu, ni, 0, None, 0,
                                                      (2, 5), (0, 0), pooling=p)), 200, lines,
                  f"catalog, {nq} queries x 4,082 items, k = 64 fp32, top-20", 1000.0, "us")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
