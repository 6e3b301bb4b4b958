"""Event-times of the two-way HHFM model beside the one-way pooled kernels with
the same level-1 modes, one process, the two alternated (four runs each), for
all-sum, all-max and all-mean modes:

  rows     ops.hybrid_score_rows at 2^23 Frappe-layout rows (F = 5), k = 64
           fp32 and k = 128 bf16; and at 2^22 rows of the F = 10 layout
           (5 context + 3 time columns, k = 64 fp32)
  catalog  ops.catalog_topk, 300 and 3,000 queries over the Frappe catalog
           (4,082 items, k = 64 fp32, top-20): one-way takes the fused
           small-catalog kernel, two-way the query kernel + score matrix +
           dense top-K, so this also shows what skipping the fused kernel costs
  step     one training step on the Frappe layout, B = 5,000, NG = 10, k = 64,
           Adagrad: hhfm_hhfm_train_step_pool2 against hhfm_hhfm_train_step_pool

The Frappe-size table is L2-resident, so the row shapes show the added VALU at
its worst.  A run is the mean of `reps` back-to-back calls between two events,
after a warm-up.  Per case: each side's four runs, the one-way side's own
spread (max / min of its runs) and the two-way / one-way ratio of the medians.
usage: python scripts/hhfm_two_way_time.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hhfm_amd import ops  # noqa: E402
from hhfm_amd._native import native  # noqa: E402
from scripts.hhfm_pool_time import rows_of, run_ms  # noqa: E402

MODES = ["sum", "max", "mean"]
RUNS = 4


def alternate(make, reps, lines, title, unit=1.0, name="ms"):
    """make(mode, two_way) -> a call; per mode RUNS rounds over (one-way, two-way)."""
    lines.append(title)
    for mode in MODES:
        fns = {"one-way": make(mode, False), "two-way": make(mode, True)}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {s: [] for s in fns}
        for _ in range(RUNS):
            for s, fn in fns.items():
                t[s].append(run_ms(fn, reps) * unit)
        med = {s: statistics.median(v) for s, v in t.items()}
        for s in fns:
            lines.append(f"  {mode:4s} {s} {name}: " + "  ".join(f"{x:9.4f}" for x in t[s])
                         + f"   median {med[s]:.4f}")
        lines.append(f"  {mode:4s} one-way's own spread (max / min of its runs): "
                     f"{max(t['one-way']) / min(t['one-way']):.4f}")
        lines.append(f"  {mode:4s} two-way / one-way (medians): "
                     f"{med['two-way'] / med['one-way']:.4f}")
    lines.append("")


def main():
    rng = np.random.default_rng(0)
    lines = ["# scripts/hhfm_two_way_time.py: two-way against the one-way pooled kernel with the "
             "same level-1 modes, alternated in one process",
             f"# device: {torch.cuda.get_device_name(0)}", ""]
    nu, ni = 957, 4082
    for title, B, cards, td, k, dt in (
            ("rows, F = 5 (Frappe), k = 64 fp32, 2^23 rows", 1 << 23, (7, 2, 3), 0, 64, torch.float32),
            ("rows, F = 5 (Frappe), k = 128 bf16, 2^23 rows", 1 << 23, (7, 2, 3), 0, 128,
             torch.bfloat16),
            ("rows, F = 10 (5 ctx + 3 time), k = 64 fp32, 2^22 rows", 1 << 22, (5, 4, 6, 3, 7), 3,
             64, torch.float32)):
        X, M = rows_of(rng, B, nu, ni, cards, td)
        E = torch.from_numpy(rng.normal(0, 0.1, (M, k)).astype(np.float32)).cuda().to(dt)
        out = torch.empty(B, dtype=torch.float32, device="cuda")
        fd = len(cards)
        ctx, tim = (2, 2 + fd), ((2 + fd, 2 + fd + td) if td else (0, 0))
        alternate(lambda m, two: (lambda: ops.hybrid_score_rows(
            X, E, 0, 1, ctx, tim, out=out, pooling=(m,) * 3, pooling2=(m,) * 3 if two else None)),
            10, lines, title)
        del X, E, out
    X, M = rows_of(rng, 5000, nu, ni, (7, 2, 3), 0)
    E = torch.from_numpy(rng.normal(0, 0.1, (M, 64)).astype(np.float32)).cuda()
    for nq in (300, 3000):
        q = X[:nq].contiguous()
        alternate(lambda m, two: (lambda: ops.catalog_topk(
            q, E, ops.MODE_HHFM, 20, nu, ni, 0, None, 0, (2, 5), (0, 0), pooling=(m,) * 3,
            pooling2=(m,) * 3 if two else None)), 200, lines,
            f"catalog, {nq} queries x 4,082 items, k = 64 fp32, top-20", 1000.0, "us")
    # one training step (Adagrad, lr 0.01 so that the table stays in range over the repeats)
    nat = native()
    B, NG, k = 5000, 10, 64
    Neg = torch.from_numpy(rng.integers(nu, nu + ni, (B, NG)).astype(np.int32)).cuda()
    Et = E.clone()
    acc = torch.full((M * k,), 0.1, device="cuda")
    ws = torch.zeros(nat.train_workspace(M, k), dtype=torch.uint8, device="cuda")
    loss = torch.zeros(1, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    args = (X.data_ptr(), Neg.data_ptr(), B, 5, 2, 5, 0, 0, NG, Et.data_ptr(), M, k, 0.01, 0.0, 0,
            acc.data_ptr(), ws.data_ptr(), ws.numel())

    def step(m, two):
        w = ops.pooling_word((m,) * 3)
        if two:
            return lambda: nat.hhfm_train_step_pool2(*args, w, w, loss.data_ptr(), st)
        return lambda: nat.hhfm_train_step_pool(*args, w, loss.data_ptr(), st)
    alternate(step, 50, lines, "training step, Frappe layout, B = 5,000, NG = 10, k = 64, Adagrad",
              1000.0, "us")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
