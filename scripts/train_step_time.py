"""Event-time of one FM and one AFM train step (the C ABI's step, all its
kernels) at the reference's default batch (5000 rows, Frappe shape, k = A = 64,
Adagrad), with the native extension loaded from a given folder, so that two
builds (say a commit's and its parent's) can be alternated, a fresh process
each.  Prints one JSON line: per case the sorted µs / step of 7 windows of 40
steps; --drop adds FM at keep 0.5 and AFM at keep [0.8, 0.5]; --det adds an HHFM
step (NG = 10) and the deterministic steps (FM at keep 1 and 0.5, HHFM) next
to their default ones, and FM at B = 32,773 with one id in every row (the
longest serial walk of the segment pass), default and deterministic; --dfm adds
the default DeepFM step (150/200/150), and --det, on a build that has them,
also the deterministic AFM (keep 1 and [0.8, 0.5]) and DeepFM steps; --pooling
adds the default HHFM step (NG = 10) and, on a build that has
hhfm_train_step_pool, the (max, max, max) and (mean, mean, mean) pooled steps
alternated with it (two rounds); --heads adds the default DeepFM step and
forward (fp32 MLP, 5000 and 2^20 rows) and, on a build that has the DeepFM
heads, the FM-head / deep-head / logloss steps, and at 2^22 rows the FM-head
forward with and without the sigmoid pass beside hhfm_fm_score_rows; --bn adds
the plain row score on bench.py's 4.3 GB table at 2^22 and 2^25 rows (the
automatic plan and HHFM_FLAG_NO_HOT_TAIL) and, on a build that has FM's batch
norm, hhfm_fm_score_rows_scaled beside them and the batch-norm FM step (keep 1
and 0.5) alternated with the plain one (two rounds).
usage: python scripts/train_step_time.py LIBDIR TAG [--drop] [--det] [--dfm] [--pooling]
       [--heads] [--bn]"""
import importlib.machinery
import importlib.util
import json
import os
import sys
import sysconfig

import numpy as np
import torch

libdir, tag = sys.argv[1], sys.argv[2]
drop = "--drop" in sys.argv
det = "--det" in sys.argv
ext = sysconfig.get_config_var("EXT_SUFFIX")
path = os.path.join(os.path.abspath(libdir), "_hhfm" + ext)
loader = importlib.machinery.ExtensionFileLoader("_hhfm", path)
spec = importlib.util.spec_from_file_location("_hhfm", path, loader=loader)
nat = importlib.util.module_from_spec(spec)
loader.exec_module(nat)

rng = np.random.default_rng(0)
nu, ni, ctx = 957, 4082, (7, 2, 3)
M = nu + ni + sum(ctx)
B, F, k, A = 5000, 5, 64, 64
cols = [rng.integers(0, nu, B), rng.integers(nu, nu + ni, B)]
o = nu + ni
for c in ctx:
    cols.append(rng.integers(o, o + c, B))
    o += c
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
X = dev(np.stack(cols, 1).astype(np.int32))
y = dev(rng.choice([1.0, -1.0], B).astype(np.float32))
st = torch.cuda.current_stream().cuda_stream
loss = torch.zeros(1, device="cuda")


def params(shapes, stds):
    par = [dev(rng.normal(0, s, sh).astype(np.float32)) for sh, s in zip(shapes, stds)]
    acc = [torch.full_like(p, 0.1) for p in par]
    return par, acc


def timed(fn, reps=7, n=40):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / n)
    return sorted(out)


par, acc = params([(M, k), (M,), (1,)], [0.01, 0.01, 0.01])
ws = torch.zeros(nat.train_workspace(M, k), dtype=torch.uint8, device="cuda")
p, a = [t.data_ptr() for t in par], [t.data_ptr() for t in acc]
step = [0]


def fm_plain():
    nat.fm_train_step(X.data_ptr(), y.data_ptr(), B, F, *p, M, k, 0.1, 0.1, 0, *a,
                      ws.data_ptr(), ws.numel(), loss.data_ptr(), st)


def fm_drop():
    step[0] += 1
    nat.fm_train_step_ex(X.data_ptr(), y.data_ptr(), B, F, *p, M, k, 0.1, 0.1, 0, 0.5,
                         2016 | step[0] << 32, *a, ws.data_ptr(), ws.numel(), loss.data_ptr(), st)


apar, aacc = params([(M, k), (M,), (1,), (k, A), (A,), (A,), (k,)],
                    [0.3, 0.01, 0.01, 0.125, 0.125, 1.0, 0.2])
aws = torch.zeros(nat.afm_train_workspace(B, F, k, A, M), dtype=torch.uint8, device="cuda")
ap, aa = [t.data_ptr() for t in apar], [t.data_ptr() for t in aacc]


def afm_plain():
    nat.afm_train_step(X.data_ptr(), y.data_ptr(), B, F, *ap[:3], M, k, A, *ap[3:], 0.1, 100.0, 0,
                       aa, aws.data_ptr(), aws.numel(), loss.data_ptr(), st)


def afm_drop():
    step[0] += 1
    nat.afm_train_step_ex(X.data_ptr(), y.data_ptr(), B, F, *ap[:3], M, k, A, *ap[3:], 0.1, 100.0,
                          0, 0.8, 0.5, 2016 | step[0] << 32, aa, aws.data_ptr(), aws.numel(),
                          loss.data_ptr(), st)


res = {"tag": tag, "fm_keep1_us": timed(fm_plain), "afm_keep1_us": timed(afm_plain)}
if drop:
    res["fm_keep0.5_us"] = timed(fm_drop)
    res["afm_keep0.8_0.5_us"] = timed(afm_drop)

if det:
    def scratch(rows, occ):
        return torch.empty(nat.train_det_scratch(rows, occ, k, M), dtype=torch.uint8,
                           device="cuda")

    def fm_step(Xt, yt, rows, keep, sc):
        """One FM step on Xt: the default path, or the deterministic one on scratch sc."""
        def fn():
            step[0] += 1
            args = (Xt.data_ptr(), yt.data_ptr(), rows, F, *p, M, k, 0.1, 0.1, 0, keep,
                    2016 | step[0] << 32, *a, ws.data_ptr(), ws.numel())
            if sc is None:
                nat.fm_train_step_ex(*args, loss.data_ptr(), st)
            else:
                nat.fm_train_step_det(*args, sc.data_ptr(), sc.numel(), loss.data_ptr(), st)
        return fn

    NG = 10
    Neg = dev(rng.integers(nu, nu + ni, (B, NG)).astype(np.int32))
    (hE,), (hacc,) = params([(M, k)], [0.1])
    hws = torch.zeros(nat.train_workspace(M, k), dtype=torch.uint8, device="cuda")

    def hhfm_step(sc):
        def fn():
            args = (X.data_ptr(), Neg.data_ptr(), B, F, 2, F, 0, 0, NG, hE.data_ptr(), M, k, 0.1,
                    0.01, 0, hacc.data_ptr(), hws.data_ptr(), hws.numel())
            if sc is None:
                nat.hhfm_train_step(*args, loss.data_ptr(), st)
            else:
                nat.hhfm_train_step_det(*args, sc.data_ptr(), sc.numel(), loss.data_ptr(), st)
        return fn

    sc = scratch(B, F)
    res["fm_det_keep1_us"] = timed(fm_step(X, y, B, 1.0, sc))
    res["fm_det_keep0.5_us"] = timed(fm_step(X, y, B, 0.5, sc))
    res["fm_keep0.5_us"] = timed(fm_step(X, y, B, 0.5, None))
    res["hhfm_ng10_us"] = timed(hhfm_step(None))
    res["hhfm_det_ng10_us"] = timed(hhfm_step(scratch(B, 2 + NG + F - 2)))
    # one id in every row: its 32,773 occurrences are one wave's serial walk
    Bh = 32773
    Xh = rng.integers(0, M, (Bh, F)).astype(np.int32)
    Xh[:, 0] = 0
    Xh, yh = dev(Xh), dev(rng.choice([1.0, -1.0], Bh).astype(np.float32))
    res["fm_hot32773_us"] = timed(fm_step(Xh, yh, Bh, 1.0, None), reps=3, n=10)
    res["fm_det_hot32773_us"] = timed(fm_step(Xh, yh, Bh, 1.0, scratch(Bh, F)), reps=3, n=10)

if "--pooling" in sys.argv:
    NGp = 10
    Negp = dev(np.random.default_rng(1).integers(nu, nu + ni, (B, NGp)).astype(np.int32))
    (pE,), (pacc,) = params([(M, k)], [0.1])
    pws = torch.zeros(nat.train_workspace(M, k), dtype=torch.uint8, device="cuda")

    def hhfm_pool_step(word):
        """The default HHFM step (word None) or the pooled one (HHFM_POOLING word)."""
        def fn():
            args = (X.data_ptr(), Negp.data_ptr(), B, F, 2, F, 0, 0, NGp, pE.data_ptr(), M, k, 0.1,
                    0.01, 0, pacc.data_ptr(), pws.data_ptr(), pws.numel())
            if word is None:
                nat.hhfm_train_step(*args, loss.data_ptr(), st)
            else:
                nat.hhfm_train_step_pool(*args, word, loss.data_ptr(), st)
        return fn

    cases = [("hhfm_sum_ng10_us", None)]
    if hasattr(nat, "hhfm_train_step_pool"):
        cases += [("hhfm_pool_max_ng10_us", 1 | 1 << 4 | 1 << 8),
                  ("hhfm_pool_mean_ng10_us", 2 | 2 << 4 | 2 << 8)]
    for rnd in (1, 2):
        for name, word in cases:
            res[f"{name}_round{rnd}"] = timed(hhfm_pool_step(word))

if det or "--dfm" in sys.argv:
    # DeepFM 150/200/150 (DFM.py:256), default step; with --det, on a build that
    # has them, the deterministic AFM (keep 1 and [0.8, 0.5]) and DeepFM steps
    layers = [150, 200, 150]
    dims = [F * k] + layers
    D = F + k + layers[-1]
    shapes = ([(M, k), (M,)] + [(i, o_) for i, o_ in zip(dims, dims[1:])] + [(o_,) for o_ in layers]
              + [(D,), (1,)])
    dpar, dacc = params(shapes, [0.01, 0.3] + [0.08] * 3 + [0.08] * 3 + [0.1, 0.01])
    dp, da = [t.data_ptr() for t in dpar], [t.data_ptr() for t in dacc]
    dws = torch.zeros(nat.dfm_train_workspace(B, F, k, M, layers), dtype=torch.uint8,
                      device="cuda")

    def dfm_step(sc):
        def fn():
            args = (X.data_ptr(), y.data_ptr(), B, F, dp[0], dp[1], M, k, layers, dp[2:5], dp[5:8],
                    dp[8], dp[9], 0.01, 0.01, 0, da, dws.data_ptr(), dws.numel())
            if sc is None:
                nat.dfm_train_step(*args, loss.data_ptr(), st)
            else:
                nat.dfm_train_step_det(*args, sc.data_ptr(), sc.numel(), loss.data_ptr(), st)
        return fn

    def afm_step(keep, sc):
        def fn():
            step[0] += 1
            args = (X.data_ptr(), y.data_ptr(), B, F, *ap[:3], M, k, A, *ap[3:], 0.1, 100.0, 0,
                    keep[0], keep[1], 2016 | step[0] << 32, aa, aws.data_ptr(), aws.numel())
            if sc is None:
                nat.afm_train_step_ex(*args, loss.data_ptr(), st)
            else:
                nat.afm_train_step_det(*args, sc.data_ptr(), sc.numel(), loss.data_ptr(), st)
        return fn

    res["dfm_us"] = timed(dfm_step(None))
    if det and hasattr(nat, "afm_train_step_det"):
        asc = torch.empty(nat.afm_train_det_scratch(B, F, k, A, M), dtype=torch.uint8,
                          device="cuda")
        dsc = torch.empty(nat.dfm_train_det_scratch(B, F, k, M, layers), dtype=torch.uint8,
                          device="cuda")
        res["afm_det_keep1_us"] = timed(afm_step((1.0, 1.0), asc))
        res["afm_keep0.8_0.5_us"] = timed(afm_step((0.8, 0.5), None))
        res["afm_det_keep0.8_0.5_us"] = timed(afm_step((0.8, 0.5), asc))
        res["dfm_det_us"] = timed(dfm_step(dsc))
if "--heads" in sys.argv:
    layers = [150, 200, 150]
    dims = [F * k] + layers
    D = F + k + layers[-1]
    shapes = ([(M, k), (M,)] + [(i, o_) for i, o_ in zip(dims, dims[1:])] + [(o_,) for o_ in layers]
              + [(D,), (1,)])
    hpar, hacc = params(shapes, [0.01, 0.3] + [0.08] * 3 + [0.08] * 3 + [0.1, 0.01])
    hp, ha = [t.data_ptr() for t in hpar], [t.data_ptr() for t in hacc]
    hws = torch.zeros(nat.dfm_train_workspace(B, F, k, M, layers), dtype=torch.uint8, device="cuda")
    # the forward's layout: layer weights transposed [N][K], K padded to 8
    Wt, kin = [], F * k
    for n_ in layers:
        Wt.append(dev(rng.normal(0, 0.08, (n_, kin)).astype(np.float32)))
        kin = (n_ + 7) & ~7

    def step_head(head):
        """The default step (head None: the entry point without a head word) or a head's."""
        def fn():
            args = (X.data_ptr(), y.data_ptr(), B, F, hp[0], hp[1], M, k, layers, hp[2:5], hp[5:8],
                    hp[8], hp[9], 0.01, 0.01, 0, ha, hws.data_ptr(), hws.numel(), loss.data_ptr(), st)
            if head is None:
                nat.dfm_train_step(*args)
            else:
                nat.dfm_train_step_head(*args, head)
        return fn

    def forward(rows, head, Xr, out, fws):
        def fn():
            args = (Xr.data_ptr(), rows, F, hp[0], M, k, 0, hp[1], layers,
                    [t.data_ptr() for t in Wt], hp[5:8], 0, hp[8], 0.01, out.data_ptr(), 2, 0,
                    fws.data_ptr(), fws.numel(), st)
            if head is None:
                nat.dfm_forward(*args)
            else:
                nat.dfm_forward_head(*args, head)
        return fn

    def rows_of(n):
        Xr = X[torch.randint(0, B, (n,), device="cuda", generator=torch.Generator("cuda")
                             .manual_seed(n))].contiguous()
        fws = torch.empty(nat.dfm_forward_workspace_ex(n, F, k, M, layers, 0, 2) + 4096,
                          dtype=torch.uint8, device="cuda")
        return Xr, torch.empty(n, device="cuda"), fws

    has = hasattr(nat, "dfm_train_step_head")
    for rnd in (1, 2):
        res[f"dfm_step_us_round{rnd}"] = timed(step_head(None))
        if has:
            res[f"dfm_step_head3_us_round{rnd}"] = timed(step_head(3))
    for n in (B, 1 << 20):
        Xr, out, fws = rows_of(n)
        reps = dict(reps=7, n=40) if n == B else dict(reps=5, n=5)
        for rnd in (1, 2):
            res[f"dfm_fwd_{n}_us_round{rnd}"] = timed(forward(n, None, Xr, out, fws), **reps)
            if has:
                res[f"dfm_fwd_head3_{n}_us_round{rnd}"] = timed(forward(n, 3, Xr, out, fws), **reps)
    if has:
        for name, head in (("fm", 1), ("deep", 2), ("fm_logloss", 5), ("both_logloss", 7)):
            res[f"dfm_step_{name}_us"] = timed(step_head(head))
        n = 1 << 22
        Xr, out, fws = rows_of(n)
        res["fm_head_fwd_4M_us"] = timed(forward(n, 1, Xr, out, fws), reps=5, n=5)
        res["fm_head_sigmoid_fwd_4M_us"] = timed(forward(n, 5, Xr, out, fws), reps=5, n=5)
        res["fm_score_rows_4M_us"] = timed(
            lambda: nat.fm_score_rows_ex(Xr.data_ptr(), n, F, hp[0], M, k, 0, hp[1], 0.01,
                                         out.data_ptr(), 0, 0, st), reps=5, n=5)
if "--bn" in sys.argv:
    # the row score on bench.py's table (8 M users + 8 M items + 12 context ids, k = 64 fp32,
    # 4.3 GB) at 2^22 and 2^25 rows: the plain entry point (its automatic plan: the LDS-tail
    # kernel) and with HHFM_FLAG_NO_HOT_TAIL (fm_rows_fast); on a build that has them, the scaled
    # entry point beside them (two rounds) and the batch-norm FM step beside the plain one
    has = hasattr(nat, "fm_train_step_bn")
    nub = nib = 8_000_000
    Mb = nub + nib + sum(ctx)
    g = torch.Generator("cuda").manual_seed(1)
    Eb = torch.empty(Mb, k, device="cuda").normal_(0, 0.01, generator=g)
    wb = torch.empty(Mb, device="cuda").normal_(0, 0.01, generator=g)
    nmax = 1 << 25
    bcols = [torch.randint(0, nub, (nmax,), generator=g, device="cuda", dtype=torch.int32),
             torch.randint(nub, nub + nib, (nmax,), generator=g, device="cuda", dtype=torch.int32)]
    o = nub + nib
    for c in ctx:
        bcols.append(torch.randint(o, o + c, (nmax,), generator=g, device="cuda",
                                   dtype=torch.int32))
        o += c
    Xb = torch.stack(bcols, 1).contiguous()
    outb = torch.empty(nmax, device="cuda")
    scale = torch.empty(k, device="cuda").normal_(1, 0.2, generator=g)

    def rows_plain(n, flags):
        return lambda: nat.fm_score_rows_ex(Xb.data_ptr(), n, F, Eb.data_ptr(), Mb, k, 0,
                                            wb.data_ptr(), 0.01, outb.data_ptr(), flags, 0, st)

    def rows_scaled(n):
        return lambda: nat.fm_score_rows_scaled(Xb.data_ptr(), n, F, Eb.data_ptr(), Mb, k, 0,
                                                wb.data_ptr(), 0.01, scale.data_ptr(),
                                                outb.data_ptr(), 0, st)

    for rnd in (1, 2):
        for n, tagn in ((1 << 22, "4M"), (1 << 25, "32M")):
            res[f"fm_rows_{tagn}_us_round{rnd}"] = timed(rows_plain(n, 0), reps=5, n=5)
            res[f"fm_rows_nohot_{tagn}_us_round{rnd}"] = timed(rows_plain(n, 4), reps=5, n=5)
            if has:
                res[f"fm_rows_scaled_{tagn}_us_round{rnd}"] = timed(rows_scaled(n), reps=5, n=5)
    del Eb, wb, Xb, outb
    if has:
        bpar, bacc = params([(M, k), (M,), (1,), (k,), (k,)], [0.01, 0.01, 0.01, 0.0, 0.0])
        bpar[3].fill_(1.0)
        mm, mv = torch.zeros(k, device="cuda"), torch.ones(k, device="cuda")
        bws = torch.zeros(nat.fm_train_bn_workspace(B, M, k), dtype=torch.uint8, device="cuda")
        bp, ba = [t.data_ptr() for t in bpar], [t.data_ptr() for t in bacc]

        def fm_bn(keep):
            def fn():
                step[0] += 1
                nat.fm_train_step_bn(X.data_ptr(), y.data_ptr(), B, F, *bp[:3], M, k, 0.1, 0.1, 0,
                                     keep, 2016 | step[0] << 32, *ba[:3], bws.data_ptr(),
                                     bws.numel(), bp[3], bp[4], mm.data_ptr(), mv.data_ptr(), 1e-3,
                                     float(1.0 - 0.9), ba[3], ba[4], loss.data_ptr(), st)
            return fn

        for rnd in (1, 2):
            res[f"fm_keep1_us_round{rnd}"] = timed(fm_plain)
            res[f"fm_bn_keep1_us_round{rnd}"] = timed(fm_bn(1.0))
        res["fm_bn_keep0.5_us"] = timed(fm_bn(0.5))
res = {k_: ([round(v, 2) for v in vs] if isinstance(vs, list) else vs) for k_, vs in res.items()}
print(json.dumps(res))
