#!/usr/bin/env python3
"""What the storage type of D costs per iteration: on-device synthetic data, one handle at a time per storage type,
the storage types interleaved over `rounds` rounds in one process.

    python tools/storage_bench.py [--n 6000000] [--d 1000] [--storages f32 fp16] [--families erm superquantile]
                                  [--warmup 5] [--steps 20] [--rounds 3] [--out profiles/storage_bench_C2.json]

Per family, round and storage type: create -> generate -> Gram -> `warmup` + `steps` timed rbl_step (each ends in a host
wait, so wall time is device time + launch gaps) -> `ksteps` more steps with HIP events around the sweep kernels
(rbl_kernel_time: the kernels' own mean time, from which the GB/s of D) -> destroy.  --family erm is the single sweep
(l1 w-step), superquantile the two passes with the sort-free z-step.  Reported per line: ms per iteration median
[min - max] over the rounds' medians, the sweep kernels' mean time, bytes of D, GB/s; and, when both are measured, the
ratio fp16 / f32 of every round."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILIES = {
    "erm": dict(weight_function="erm", wstep="l1", args=None, passes=1),
    "superquantile": dict(weight_function="superquantile", wstep="l2", args=[0.5], passes=2),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6_000_000)
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--storages", nargs="*", default=["f32", "fp16"])
    ap.add_argument("--families", "--family", nargs="*", default=["erm", "superquantile"], choices=sorted(FAMILIES))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--ksteps", type=int, default=10, help="further steps with events around the sweep kernels")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import admm_for_rank_based_loss_amd as rbl
    L = rbl._lib
    esz = {0: 4, 1: 8, 2: 2}
    record = dict(n=a.n, d=a.d, warmup=a.warmup, steps=a.steps, ksteps=a.ksteps, rounds=a.rounds, results=[])
    for fam in a.families:
        f = FAMILIES[fam]
        per = {s: dict(iter_ms=[], kernel_ms=[]) for s in a.storages}
        for rnd in range(a.rounds):
            for storage in a.storages:
                s = rbl.Solver(a.n, a.d, f["weight_function"], "binary_cross_entropy", reg=0.01,
                               wstep=L.WSTEP_L1 if f["wstep"] == "l1" else L.WSTEP_L2, args=f["args"], storage=storage, tol=0.0,
                               max_iter=10 ** 6)
                s.generate_synthetic(seed=17)
                s.gram()
                ld = s.info()["ld"]
                per[storage]["D_bytes"] = a.n * ld * esz[L.STORAGE[storage]]
                for _ in range(a.warmup):
                    s.step(False)
                ts = []
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    s.step(False)
                    ts.append((time.perf_counter() - t0) * 1e3)
                per[storage]["iter_ms"].append(statistics.median(ts))
                s.profile_kernels(1)
                s.reset_kernel_times()
                for _ in range(a.ksteps):
                    s.step(False)
                tot, cnt = 0.0, 0
                for which in (L.KERNEL_GEMV, L.KERNEL_GEMVT, L.KERNEL_SWEEP_ERM):
                    ms, c = s.kernel_time(which)
                    tot, cnt = tot + ms, cnt + c
                per[storage]["kernel_ms"].append(tot / cnt if cnt else float("nan"))
                per[storage]["launches_per_step"] = cnt / max(1, a.ksteps)
                s.close()
                print(f"  {fam} round {rnd} {storage}: {per[storage]['iter_ms'][-1]:.3f} ms/iteration, sweep kernel "
                      f"{per[storage]['kernel_ms'][-1]:.3f} ms x {per[storage]['launches_per_step']:.0f}", flush=True)
        for storage in a.storages:
            p = per[storage]
            km = statistics.median(p["kernel_ms"])
            line = dict(family=fam, storage=storage, iter_ms_median=statistics.median(p["iter_ms"]), iter_ms_min=min(p["iter_ms"]),
                        iter_ms_max=max(p["iter_ms"]), iter_ms_rounds=p["iter_ms"], sweep_kernel_ms=km, sweep_kernel_ms_rounds=p["kernel_ms"],
                        sweep_launches_per_step=p["launches_per_step"], D_bytes=p["D_bytes"], sweep_GBps=p["D_bytes"] / km / 1e6)
            record["results"].append(line)
            print(f"{fam:14s} {storage:5s} {line['iter_ms_median']:8.3f} ms/iteration [{line['iter_ms_min']:.3f} - {line['iter_ms_max']:.3f}]  "
                  f"sweep kernel {km:.3f} ms  D {p['D_bytes'] / 1e9:.2f} GB  {line['sweep_GBps']:.0f} GB/s", flush=True)
        if "f32" in per and "fp16" in per:
            ratios = [h / f32 for h, f32 in zip(per["fp16"]["iter_ms"], per["f32"]["iter_ms"])]
            record["results"].append(dict(family=fam, fp16_over_f32_iter_ms_rounds=ratios))
            print(f"{fam:14s} fp16 / f32 per round: " + ", ".join(f"{r:.3f}" for r in ratios), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(record, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
