"""What the exclusion lists cost on the AFM and DeepFM catalogs, event-timed in
alternating windows (A, B, C, A, B, C, ... in one process) on an MI355X.

Three things per shape, as whole calls and as the select alone on a score
matrix of the call's size:

  plain     the same build's plain call (hhfm_afm_catalog_topk_ex /
            hhfm_dfm_catalog_topk_ex; the select: hhfm_topk_dense_ex);
  filtered  the exclusion form (hhfm_*_catalog_topk_excl; the select:
            hhfm_topk_dense_excl), with the lists of a Frappe-shape split and
            with empty lists;
  mask      the alternative: excl_mask_kernel on the matrix, then the plain
            select (hhfm_debug_mask_then_select) — the select alone; as a whole
            call it is the plain call plus the difference measured there.

Shapes: AFM 300 queries, DeepFM 60 queries, over the distinct items of the
Frappe-shape split (bench.frappe_shape_dataset draws from 4,082; no Frappe rows
are shipped), K = 20, k = 64.  AFM selects with one wave per query, DeepFM by
the default routing (four waves per query here).

Usage: python scripts/topk_excl_models_ab.py [out.txt]"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from hhfm_amd import harness, ops  # noqa: E402
from hhfm_amd._native import native  # noqa: E402
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


def alternate(fns, reps):
    for fn in fns:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(ROUNDS):
        for n, fn in enumerate(fns):
            t[n].append(window(fn, reps))
    return [np.array(x) for x in t]


def line(name, labels, ts):
    parts = ["%s %8.1f us (min %.1f max %.1f)" % (lab, np.median(t), t.min(), t.max())
             for lab, t in zip(labels, ts)]
    return "%-26s %s" % (name, "   ".join(parts))


def main():
    dev = torch.device("cuda", 0)
    nat = native()
    out = ["# exclusion lists on the AFM / DeepFM catalogs (K = %d, k = %d): medians of %d "
           "alternating windows" % (K, KF, ROUNDS),
           "# device (the name the runtime reports; run on an MI355X, gfx950): %s"
           % torch.cuda.get_device_name(dev)]
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as tmp:
        np.random.seed(2016)
        d = LoadData(bench.frappe_shape_dataset(tmp), "frappe_shape")
    F = d.Train_data.shape[1] - 1
    M, N, nu = d.features_M, d.n_item, d.n_user
    pairs = harness.DevicePairSet(d.positive_feedback, F - 1, dev)
    test = np.asarray(d.Test_data.values[:, 1:], dtype=np.int64)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)  # noqa: E731
    E, w = t(rng.normal(0, 0.1, (M, KF))), t(rng.normal(0, 0.01, M))
    st = torch.cuda.current_stream(dev).cuda_stream

    def lists_for(B):
        rows = torch.from_numpy(test[rng.integers(0, len(test), B)].astype(np.int32)).to(dev)
        x = ops.pf_exclusion_lists(pairs.keys, pairs.codes, rows, 1, keep_own=True)
        lens = (x.ptr[1:] - x.ptr[:-1]).cpu().numpy()
        return rows, x, ops.exclusion_lists([[]] * B, dev), lens

    def select_rows(name, B, plan):
        rows, x, empty, lens = lists_for(B)
        S = t(rng.normal(0, 1, (B, N)))
        top_s = torch.empty(B, K, dtype=torch.float32, device=dev)
        top_i = torch.empty(B, K, dtype=torch.int32, device=dev)
        # the raw entry points on preallocated outputs: the same host work per call
        o = (top_s.data_ptr(), top_i.data_ptr(), plan, st)
        plain = lambda: nat.topk_dense(S.data_ptr(), B, N, N, K, 0, *o)  # noqa: E731
        excl = lambda v: (lambda: nat.topk_dense_excl(  # noqa: E731
            S.data_ptr(), B, N, N, K, 0, *o, nu, v.ptr.data_ptr(),
            v.rows.data_ptr() if v.rows.numel() else 0, v.max_len))
        mask = lambda: nat.debug_mask_then_select(  # noqa: E731
            S.data_ptr(), B, N, N, K, 0, *o, nu, x.ptr.data_ptr(), x.rows.data_ptr())
        ts = alternate([plain, excl(x), excl(empty), mask], 500)
        out.append(line("%s select B=%d N=%d" % (name, B, N),
                        ("plain", "filtered", "filtered(empty)", "mask+select"), ts)
                   + "   lists mean %.1f max %d" % (lens.mean(), lens.max()))

    # AFM: 300 queries, A = k = 64
    A = 64
    Wt = t(rng.normal(0, (2.0 / (KF + A)) ** 0.5, (A, KF)))
    att = (Wt, t(rng.normal(0, 0.1, A)), t(rng.normal(0, 0.5, A)), t(rng.normal(1, 0.2, KF)))
    rows, x, empty, lens = lists_for(300)
    afm = lambda **kw: ops.afm_catalog_topk(rows, E, w, *att, nu, N, K, 0, **kw)  # noqa: E731
    ts = alternate([afm, lambda: afm(exclude=x), lambda: afm(exclude=empty)], 50)
    out.append(line("AFM call B=300 N=%d" % N, ("plain", "filtered", "filtered(empty)"), ts)
               + "   lists mean %.1f max %d" % (lens.mean(), lens.max()))
    select_rows("AFM", 300, ops.PLAN_ONE_WAVE)

    # DeepFM: 60 queries, the harness's layers, fp32 MLP
    layers, kin, Ls, Bs = [150, 200, 150], F * KF, [], []
    for n in layers:
        Ls.append(t(rng.normal(0, (2.0 / (kin + n)) ** 0.5, (kin, n))))
        Bs.append(t(rng.normal(0, 0.01, n)))
        kin = n
    Wl, bl, dims = ops.dfm_prepare_weights(Ls, Bs, torch.float32, F, KF)
    Wp = t(rng.normal(0, 0.1, F + KF + layers[-1]))
    rows, x, empty, lens = lists_for(60)
    dfm = lambda **kw: ops.dfm_catalog_topk(rows, E, w, Wl, bl, dims, Wp, 0.3, 1, nu, N, K,  # noqa: E731
                                            0, **kw)
    ts = alternate([dfm, lambda: dfm(exclude=x), lambda: dfm(exclude=empty)], 20)
    out.append(line("DeepFM call B=60 N=%d" % N, ("plain", "filtered", "filtered(empty)"), ts)
               + "   lists mean %.1f max %d" % (lens.mean(), lens.max()))
    select_rows("DeepFM", 60, 0)

    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
