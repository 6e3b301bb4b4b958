"""What a wide list costs: hhfm_catalog_topk at K in {100, 256, 1024} against
the K = 64 call (the existing narrow call, the yardstick), event-timed in one
process with the sides alternating (yardstick, K, yardstick, K, ...: four
windows per side), on an MI355X.

  dense     300 queries x 4,082 items              (score matrix + select)
  blocked   1,024 queries x a 1.25 M-item shard    (77 blocks of 16,384 items)
  select    topk_dense alone on a resident [1024][16384] matrix

all at k = 128, fp32 and bf16 tables, HHFM mode.  For the blocked route the
bytes of block matrix written and read back per call are printed beside the
ratio: the narrow streaming path materialises none of them.

Usage: python scripts/topk_wide_time.py [out.txt]   (default profiles/topk_wide_ab.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hhfm_amd import ops  # noqa: E402

KF, ROUNDS, BLOCK = 128, 4, 16384
KS = (100, 256, 1024)


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps      # us per call


def ab(narrow, wide, reps):
    for fn in (narrow, wide):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(window(narrow, reps))
        tb.append(window(wide, reps))
    return np.array(ta), np.array(tb)


def line(name, ta, tb, extra=""):
    return ("%-40s K=64 %9.1f us (min %.1f max %.1f)   wide %9.1f us (min %.1f max %.1f)   "
            "x%.2f  %s" % (name, np.median(ta), ta.min(), ta.max(), np.median(tb), tb.min(),
                           tb.max(), np.median(tb) / np.median(ta), extra))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "topk_wide_ab.txt")
    dev = torch.device("cuda", 0)
    out = ["# wide K against the K = 64 call (k = %d, HHFM mode), medians of %d alternating "
           "windows per side" % (KF, ROUNDS),
           "# device (the name the runtime reports; run on an MI355X, gfx950): %s"
           % torch.cuda.get_device_name(dev)]
    rng = np.random.default_rng(1)
    nu, nctx = 957, 12
    for B, N, reps in ((300, 4082, 50), (1024, 1_250_000, 3)):
        M = nu + N + nctx
        E32 = torch.from_numpy(rng.normal(0, 0.1, (M, KF)).astype(np.float32)).to(dev)
        q = np.stack([rng.integers(0, nu, B), np.full(B, nu), nu + N + rng.integers(0, 7, B),
                      nu + N + 7 + rng.integers(0, 5, B)], 1).astype(np.int32)
        q = torch.from_numpy(q).to(dev)
        for dtype in (torch.float32, torch.bfloat16):
            E = E32.to(dtype)

            def call(K):
                return lambda: ops.catalog_topk(q, E, ops.MODE_HHFM, K, nu, N, 0, None, 0, (2, 4),
                                                (0, 0))
            for K in KS:
                ta, tb = ab(call(64), call(K), reps)
                extra = ""
                if N > BLOCK:
                    extra = "block matrix: %.2f GiB written + read per call" % (B * N * 4 / 2 ** 30)
                out.append(line("%d x %d %s K=%d" % (B, N, str(dtype)[6:], K), ta, tb, extra))
                print(out[-1], flush=True)
        del E32, E
    S = torch.from_numpy(rng.normal(size=(1024, BLOCK)).astype(np.float32)).to(dev)
    for K in KS:
        ta, tb = ab(lambda: ops.topk_dense(S, 64), lambda: ops.topk_dense(S, K), 20)
        out.append(line("select alone [1024][16384] K=%d" % K, ta, tb))
        print(out[-1], flush=True)
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
