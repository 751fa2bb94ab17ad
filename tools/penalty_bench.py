#!/usr/bin/env python3
"""What per-coordinate penalties cost per iteration: erm / binary_cross_entropy on on-device synthetic data, the single
sweep with the w-step enqueued ahead, one handle at a time per variant, the variants interleaved over `rounds` rounds in
one process.

    python tools/penalty_bench.py [--n 6000000] [--d 1000] [--storage f32] [--warmup 5] [--steps 20] [--ksteps 10]
                                  [--rounds 3] [--out profiles/penalty_bench.json]

Variants: `scalar` - l1_reg = 0.01 through cfg.reg, no rbl_set_penalty: the kernels of the scalar path, the yardstick;
`l1_vector` - the same problem as a uniform l1 vector (k_lasso_fs<true>, the weighted sums of the objective);
`elastic_net` - l1 = 0.01, l2 = 0.02.  Per round and variant: create -> generate -> Gram -> `warmup` + `steps` timed
rbl_step (each ends in a host wait) -> `ksteps` more with HIP events around the phases, whose ms_w is the w-step's own
time.  The tool fails if a step did not run the single-sweep pass or the active-set kernel (wstep_form 2): a fallback is
never recorded as the cost of a variant."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {"scalar": None, "l1_vector": (0.01, None), "elastic_net": (0.01, 0.02)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6_000_000)
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--storage", default="f32")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--ksteps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import admm_for_rank_based_loss_amd as rbl
    L = rbl._lib
    per = {v: dict(iter_ms=[], wstep_us=[]) for v in VARIANTS}
    for rnd in range(a.rounds):
        for name, pen in VARIANTS.items():
            s = rbl.Solver(a.n, a.d, "erm", "binary_cross_entropy", reg=0.01, wstep=L.WSTEP_L1, storage=a.storage, tol=0.0,
                           max_iter=10 ** 6)
            if pen is not None:
                s.set_penalty(pen[0], pen[1])
            s.generate_synthetic(seed=17)
            s.gram()
            for _ in range(a.warmup):
                s.step(False)
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                st = s.step(False)
                ts.append((time.perf_counter() - t0) * 1e3)
                if st.fused != 1 or st.wstep_form != 2:
                    sys.exit(f"{name}: fused={st.fused} wstep_form={st.wstep_form} - not the path this line times")
            s.profile_kernels(2)
            ws = []
            for _ in range(a.ksteps):
                ws.append(s.step(False).ms_w * 1e3)
            s.close()
            per[name]["iter_ms"].append(statistics.median(ts))
            per[name]["wstep_us"].append(statistics.median(ws))
            print(f"  round {rnd} {name}: {per[name]['iter_ms'][-1]:.3f} ms/iteration, w-step {per[name]['wstep_us'][-1]:.1f} us",
                  flush=True)
    record = dict(n=a.n, d=a.d, storage=a.storage, warmup=a.warmup, steps=a.steps, ksteps=a.ksteps, rounds=a.rounds, results=[])
    base = per["scalar"]["iter_ms"]
    for name, p in per.items():
        med = statistics.median(p["iter_ms"])
        line = dict(variant=name, iter_ms_median=med, it_per_s=1e3 / med, iter_ms_rounds=p["iter_ms"],
                    wstep_us_median=statistics.median(p["wstep_us"]), wstep_us_rounds=p["wstep_us"],
                    over_scalar_iter_ms_rounds=[x / b for x, b in zip(p["iter_ms"], base)])
        record["results"].append(line)
        print(f"{name:12s} {med:8.3f} ms/iteration  {line['it_per_s']:7.2f} it/s  w-step {line['wstep_us_median']:.1f} us  "
              f"/ scalar per round: " + ", ".join(f"{r:.4f}" for r in line["over_scalar_iter_ms_rounds"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(record, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
