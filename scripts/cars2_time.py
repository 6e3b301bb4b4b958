"""Event-times of the CARS2 row kernel beside the HHFM row kernel, and of one
CARS2 train step, in one process:

  rows   ops.cars2_score_rows at B = 2^22, D = 128 fp32, Mc = 42, and
         ops.hybrid_score_rows at F = 5, k = 128 fp32 on the same user / item
         ids and the same table (its three context columns index the table's
         last rows), alternated, four runs each
  step   hhfm_cars2_train_step at the reference's batch (B = 5,000, NG = 1),
         D = 128, the Frappe vocabulary, Adagrad, λ = 0.001

A run is the mean of 200 (rows) or 500 (step) back-to-back calls between two
events, after a warm-up: windows of 70 ms and more.  Algorithmic bytes per
row: CARS2 2·D·4 (the UI rows) + 2·D·4 (the GA / GB rows) + 12 (ids) + 4
(out); HHFM F·k·4 + F·4 + 4.
usage: python scripts/cars2_time.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hhfm_amd import ops  # noqa: E402
from hhfm_amd._native import native  # noqa: E402

RUNS = 4


def run_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def main():
    rng = np.random.default_rng(0)
    lines = ["# scripts/cars2_time.py: the CARS2 row kernel beside the HHFM row kernel, alternated",
             f"# device: {torch.cuda.get_device_name(0)}", ""]
    nu, ni, cards, D, Mc, B = 957, 4082, (7, 2, 3), 128, 42, 1 << 22
    Dc, Dp, Dq = ops.cars2_dims(D)
    M = nu + ni + sum(cards)
    E = dev(rng.normal(0, 0.01, (M, D)).astype(np.float32))
    user, item = rng.integers(0, nu, B), rng.integers(nu, nu + ni, B)
    cols, o = [user, item], nu + ni
    for c in cards:
        cols.append(rng.integers(o, o + c, B))
        o += c
    Xh = dev(np.stack(cols, 1).astype(np.int32))
    Xc = dev(np.stack([user, item, rng.integers(0, Mc, B)], 1).astype(np.int32))
    n = lambda *s: dev(rng.normal(0, 0.01, s).astype(np.float32))   # noqa: E731
    Ctx, W, Z, A, Bv = n(Mc, Dc), n(D, Dp, Dc), n(D, Dq, Dc), n(Dp), n(Dq)
    prepared = ops.cars2_prepare(Ctx, W, Z, A, Bv)
    out = torch.empty(B, dtype=torch.float32, device="cuda")
    fns = {"cars2": lambda: ops.cars2_score_rows(Xc, E, prepared, Mc, out=out),
           "hhfm": lambda: ops.hybrid_score_rows(Xh, E, 0, 1, (2, 5), (0, 0), out=out)}
    nbytes = {"cars2": 2 * D * 4 + 2 * D * 4 + 12 + 4, "hhfm": 5 * D * 4 + 5 * 4 + 4}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(RUNS):
        for k, fn in fns.items():
            t[k].append(run_ms(fn, 200))
    med = {k: statistics.median(v) for k, v in t.items()}
    lines.append(f"rows, B = 2^22, D = k = {D} fp32, table of {M} rows, Mc = {Mc}")
    for k in fns:
        lines.append(f"  {k:5s} ms: " + "  ".join(f"{x:8.4f}" for x in t[k])
                     + f"   median {med[k]:.4f}   {nbytes[k]} algorithmic B/row"
                     f"   {nbytes[k] * B / med[k] / 1e9:.2f} TB/s algorithmic")
    lines.append(f"  cars2 / hhfm (medians): {med['cars2'] / med['hhfm']:.4f}"
                 f"   byte-count ratio: {nbytes['cars2'] / nbytes['hhfm']:.4f}")
    lines.append("")

    Bt, NG = 5000, 1
    n_ui = nu + ni
    UI = dev(rng.normal(0, 0.01, (n_ui, D)).astype(np.float32))
    X = dev(np.stack([rng.integers(0, nu, Bt), rng.integers(nu, n_ui, Bt)], 1).astype(np.int32))
    Fea = dev(rng.integers(0, Mc, Bt).astype(np.int32))
    Neg = dev(rng.integers(nu, n_ui, (Bt, NG)).astype(np.int32))
    var = [UI, Ctx, W, Z, A, Bv]
    acc = [torch.full((v.numel(),), 0.1, device="cuda") for v in var]
    nat = native()
    ws = torch.zeros(nat.cars2_train_workspace(Bt, n_ui, Mc, D, Dc, Dp, Dq), dtype=torch.uint8,
                     device="cuda")
    loss = torch.zeros(1, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def step():
        nat.cars2_train_step(X.data_ptr(), Fea.data_ptr(), Neg.data_ptr(), Bt, NG, UI.data_ptr(),
                             n_ui, Ctx.data_ptr(), Mc, W.data_ptr(), Z.data_ptr(), A.data_ptr(),
                             Bv.data_ptr(), D, Dc, Dp, Dq, 0.01, 0.001, 0,
                             [a.data_ptr() for a in acc], ws.data_ptr(), ws.numel(),
                             loss.data_ptr(), st)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ts = [run_ms(step, 500) * 1000 for _ in range(RUNS)]
    lines.append(f"train step, B = {Bt}, NG = {NG}, D = {D}, n_ui = {n_ui}, Mc = {Mc}, Adagrad, "
                 "lambda = 0.001")
    lines.append("  us: " + "  ".join(f"{x:8.1f}" for x in ts)
                 + f"   median {statistics.median(ts):.1f}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
