"""Event-times of the attention=0 AFM step and catalog call beside their
siblings, at the Frappe shape, in one process, alternated:

  step     B = 5,000, F = 10, k = 64 (A = 64 for the attention step), the Frappe
           vocabulary padded to ten fields, Adagrad, keep 1:
             noatt      hhfm_afm_noatt_train_step
             noatt_det  hhfm_afm_noatt_train_step_det
             afm        hhfm_afm_train_step_ex        (the attention step)
             fm         hhfm_fm_train_step_ex         (λ = 0: the nearest sibling)
  catalog  300 and 3,000 queries over 4,082 items, F = 10, k = 64, K = 20:
             noatt      hhfm_afm_noatt_catalog_topk
             afm        hhfm_afm_catalog_topk

A run is the mean of REPS back-to-back calls between two events after a
warm-up; RUNS runs per variant, interleaved (A B C D A B C D ...), medians and
the spread (max − min) / median reported.
usage: python scripts/afm0_time.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hhfm_amd import ops  # noqa: E402
from hhfm_amd._native import native  # noqa: E402

RUNS = 7


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


def interleaved(fns, reps):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(RUNS):
        for k, fn in fns.items():
            t[k].append(run_ms(fn, reps) * 1000)
    return t


def report(lines, t):
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, v in t.items():
        lines.append(f"  {k:10s} us: " + " ".join(f"{x:8.1f}" for x in v)
                     + f"   median {med[k]:8.1f}   spread {(max(v) - min(v)) / med[k]:.3f}")
    return med


def rows(rng, B, nu, ni, cards):
    cols, o = [rng.integers(0, nu, B), rng.integers(nu, nu + ni, B)], nu + ni
    for c in cards:
        cols.append(rng.integers(o, o + c, B))
        o += c
    return np.stack(cols, 1).astype(np.int32)


def main():
    rng = np.random.default_rng(0)
    nat = native()
    st = torch.cuda.current_stream().cuda_stream
    lines = ["# scripts/afm0_time.py: the attention=0 AFM step and catalog call beside their siblings",
             f"# device: {torch.cuda.get_device_name(0)}; {RUNS} interleaved runs per variant", ""]
    nu, ni, cards, k, A, B = 957, 4082, (7, 2, 3, 5, 4, 6, 9, 8), 64, 64, 5000
    F = 2 + len(cards)
    M = nu + ni + sum(cards)
    X = dev(rows(rng, B, nu, ni, cards))
    y = dev(rng.choice([-1.0, 1.0], B).astype(np.float32))
    n = lambda *s: dev(rng.normal(0, 0.01, s).astype(np.float32))   # noqa: E731
    loss = torch.zeros(1, device="cuda")
    zeros = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")   # noqa: E731
    acc = lambda vs: [torch.full((v.numel(),), 0.1, device="cuda") for v in vs]   # noqa: E731

    E0, w0v, b0, P0 = n(M, k), n(M), n(1), dev(np.ones(k, np.float32))
    v_na = [E0.clone(), w0v.clone(), b0.clone(), P0.clone()]
    a_na = acc(v_na)
    ws_na = zeros(nat.afm_noatt_train_workspace(M, k))
    v_nd = [t.clone() for t in v_na]
    a_nd = acc(v_nd)
    ws_nd = zeros(nat.afm_noatt_train_workspace(M, k))
    sc_nd = torch.empty(nat.afm_noatt_train_det_scratch(B, F, k, M), dtype=torch.uint8,
                        device="cuda")
    v_af = [E0.clone(), w0v.clone(), b0.clone(), n(k, A), n(A), n(A), P0.clone()]
    a_af = acc(v_af)
    ws_af = zeros(nat.afm_train_workspace(B, F, k, A, M))
    v_fm = [E0.clone(), w0v.clone(), b0.clone()]
    a_fm = acc(v_fm)
    ws_fm = zeros(nat.train_workspace(M, k))

    def noatt_args(v, a, ws):
        return (X.data_ptr(), y.data_ptr(), B, F, v[0].data_ptr(), v[1].data_ptr(),
                v[2].data_ptr(), v[3].data_ptr(), M, k, 0.01, 0, 1.0, 0,
                [t.data_ptr() for t in a], ws.data_ptr(), ws.numel())

    def noatt():
        nat.afm_noatt_train_step(*noatt_args(v_na, a_na, ws_na), loss.data_ptr(), st)

    def noatt_det():
        nat.afm_noatt_train_step_det(*noatt_args(v_nd, a_nd, ws_nd), sc_nd.data_ptr(),
                                     sc_nd.numel(), loss.data_ptr(), st)

    def afm():
        v = v_af
        nat.afm_train_step_ex(X.data_ptr(), y.data_ptr(), B, F, v[0].data_ptr(), v[1].data_ptr(),
                              v[2].data_ptr(), M, k, A, v[3].data_ptr(), v[4].data_ptr(),
                              v[5].data_ptr(), v[6].data_ptr(), 0.01, 0.0, 0, 1.0, 1.0, 0,
                              [t.data_ptr() for t in a_af], ws_af.data_ptr(), ws_af.numel(),
                              loss.data_ptr(), st)

    def fm():
        v = v_fm
        nat.fm_train_step_ex(X.data_ptr(), y.data_ptr(), B, F, v[0].data_ptr(), v[1].data_ptr(),
                             v[2].data_ptr(), M, k, 0.01, 0.0, 0, 1.0, 0, a_fm[0].data_ptr(),
                             a_fm[1].data_ptr(), a_fm[2].data_ptr(), ws_fm.data_ptr(),
                             ws_fm.numel(), loss.data_ptr(), st)

    t = interleaved({"noatt": noatt, "noatt_det": noatt_det, "afm": afm, "fm": fm}, 300)
    lines.append(f"train step, B = {B}, F = {F}, k = {k} (A = {A}), M = {M}, Adagrad, keep 1")
    med = report(lines, t)
    lines.append(f"  noatt / afm = {med['noatt'] / med['afm']:.4f}   noatt / fm = "
                 f"{med['noatt'] / med['fm']:.4f}   noatt_det / noatt = "
                 f"{med['noatt_det'] / med['noatt']:.4f}")
    lines.append("")

    E, w, P = n(M, k), n(M), dev(rng.normal(1, 0.3, k).astype(np.float32))
    Wt, ab, ap = n(A, k), n(A), n(A)
    for Bq in (300, 3000):
        q = dev(rows(rng, Bq, nu, ni, cards))
        fns = {"noatt": lambda q=q: ops.afm_noatt_catalog_topk(q, E, w, 0.02, P, nu, ni, 20),
               "afm": lambda q=q: ops.afm_catalog_topk(q, E, w, Wt, ab, ap, P, nu, ni, 20)}
        t = interleaved(fns, 50 if Bq == 300 else 10)
        lines.append(f"catalog top-20, {Bq} queries x {ni} items, F = {F}, k = {k} (A = {A})")
        med = report(lines, t)
        lines.append(f"  noatt / afm = {med['noatt'] / med['afm']:.4f}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
