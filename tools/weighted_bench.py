#!/usr/bin/env python3
"""What row weights cost the single-sweep erm pass: one process, one on-device synthetic data set, two handles on the
same D - an unweighted owner and a borrower with sample weights c log-uniform on [1/2, 2] (rbl_set_row_weights) - stepped
in interleaved blocks, with HIP events around the fused pass of every step (rbl_kernel_time, KERNEL_SWEEP_ERM).

    python tools/weighted_bench.py [--n 6000000] [--d 1000] [--storage f32] [--warmup 10] [--steps 20] [--blocks 5]
                                   [--out profiles/weighted_bench.json]

Per block: `steps` steps of the unweighted handle, then `steps` of the weighted one (after `warmup` steps of each once, at
the start).  Reported: the mean pass time of every block of both handles, the medians, their ratio, and the spread of the
unweighted blocks among themselves ((max - min) / median) - the comparison is against the unweighted pass of the SAME
run, never against a remembered number.  The byte model: the weighted pass reads 8 more bytes per row (sigma_i) beside
ld * sizeof(T) of D and 16 + 16 (24 with the objective) bytes of row-wise state: + 0.2 % at d = 1000 in fp32.  A ratio
above 1 + spread + 1 % is a finding ("finding": true in the record)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6_000_000)
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--storage", default="f32")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import admm_for_rank_based_loss_amd as rbl
    L, S = rbl._lib, rbl._solver.Solver
    if L.device_count() < 1:
        raise SystemExit("weighted_bench: no HIP device (a pass time is measured on the GPU or not at all)")
    kw = dict(weight_function="erm", loss="binary_cross_entropy", reg=0.01, wstep=L.WSTEP_L1, storage=a.storage, tol=0.0,
              max_iter=10 ** 6)
    plain = S(a.n, a.d, **kw)
    plain.generate_synthetic(seed=17)
    plain.gram()
    weighted = S(a.n, a.d, share=plain, **kw)
    rng = np.random.default_rng(5)
    weighted.set_row_weights(np.exp(rng.uniform(np.log(0.5), np.log(2.0), size=a.n)))
    esz = {0: 4, 1: 8, 2: 2}[L.STORAGE[a.storage]]
    ld = plain.info()["ld"]
    handles = (("unweighted", plain), ("weighted", weighted))
    for _, s in handles:
        s.profile_kernels(1)
        for _ in range(a.warmup):
            st = s.step()
            assert st.fused == 1 or st.iter == 1, "the single-sweep pass did not run"
    ms = {name: [] for name, _ in handles}
    for _ in range(a.blocks):
        for name, s in handles:
            s.reset_kernel_times()
            for _ in range(a.steps):
                st = s.step()
                assert st.fused == 1, f"{name}: the single-sweep pass did not run"
            total, cnt = s.kernel_time(L.KERNEL_SWEEP_ERM)
            assert cnt == a.steps, (name, cnt)
            ms[name].append(total / cnt)
    mu, mw = statistics.median(ms["unweighted"]), statistics.median(ms["weighted"])
    spread = (max(ms["unweighted"]) - min(ms["unweighted"])) / mu
    ratio = mw / mu
    rec = dict(n=a.n, d=a.d, ld=ld, storage=a.storage, warmup=a.warmup, steps=a.steps, blocks=a.blocks,
               unweighted_pass_ms=ms["unweighted"], weighted_pass_ms=ms["weighted"], unweighted_median_ms=mu,
               weighted_median_ms=mw, ratio=ratio, unweighted_spread=spread, byte_model_ratio=1.0 + 8.0 / (ld * esz),
               D_bytes_per_s_unweighted=a.n * ld * esz / (mu * 1e-3), D_bytes_per_s_weighted=a.n * ld * esz / (mw * 1e-3),
               finding=bool(ratio > 1.0 + spread + 0.01))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    weighted.close()
    plain.close()


if __name__ == "__main__":
    main()
