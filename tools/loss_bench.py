#!/usr/bin/env python3
"""What the loss costs per iteration: on-device synthetic data, fp32 storage, one handle at a time per loss, the losses
interleaved over `rounds` rounds in one process.

    python tools/loss_bench.py [--n 6000000] [--d 1000] [--losses binary_cross_entropy hinge squared_hinge]
                               [--families erm superquantile] [--warmup 5] [--steps 20] [--rounds 3]
                               [--lib path/to/another/librbl.so] [--out profiles/loss_bench_C2.json]

Per family, round and loss: create -> generate -> Gram -> `warmup` + `steps` timed rbl_step (each ends in a host wait, so
wall time is device time + launch gaps) -> `ksteps` more steps with HIP events around the sweep kernels
(rbl_kernel_time: the kernels' own mean time, from which the GB/s of D) -> destroy.  Every line records the path its
steps took - how many of the timed steps ran the single-sweep erm kernel (`fused`) or the sort-free z-step (`zband`), and
the single-sweep kernel's launches among the `ksteps` - and the tool fails if a family did not take the path it is there
to time (erm: every step; superquantile: at least one, the count is recorded), so that a fallback is never recorded as the cost of a loss.  --family erm is the single sweep
(l1 w-step), superquantile the two passes with the sort-free z-step.  The pass moves the same bytes of D whatever the
loss, so the yardstick of a loss is the binary_cross_entropy line of the SAME run (ratio per round).  --lib times another
build of the library (the parent commit's, on the same box) with the same tool; a loss that build does not know is
reported as not measured."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILIES = {
    "erm": dict(weight_function="erm", wstep="l1", args=None),
    "superquantile": dict(weight_function="superquantile", wstep="l2", args=[0.5]),
}
LOSSES = ["binary_cross_entropy", "hinge", "squared_hinge"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6_000_000)
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--storage", default="f32")
    ap.add_argument("--losses", nargs="*", default=LOSSES, choices=LOSSES)
    ap.add_argument("--families", "--family", nargs="*", default=["erm", "superquantile"], choices=sorted(FAMILIES))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--ksteps", type=int, default=10, help="further steps with events around the sweep kernels")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another librbl.so to time instead of the package's own")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import admm_for_rank_based_loss_amd as rbl
    L = rbl._lib
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)      # read by _lib.load() on first use
    esz = {0: 4, 1: 8, 2: 2}
    record = dict(n=a.n, d=a.d, storage=a.storage, warmup=a.warmup, steps=a.steps, ksteps=a.ksteps, rounds=a.rounds,
                  lib=a.lib or "package", results=[])
    for fam in a.families:
        f = FAMILIES[fam]
        per = {l: dict(iter_ms=[], kernel_ms=[], fused_steps=[], zband_steps=[], sweep_erm_launches=[]) for l in a.losses}
        unknown = set()
        for rnd in range(a.rounds):
            for loss in a.losses:
                if loss in unknown:
                    continue
                try:
                    s = rbl.Solver(a.n, a.d, f["weight_function"], loss, reg=0.01,
                                   wstep=L.WSTEP_L1 if f["wstep"] == "l1" else L.WSTEP_L2, args=f["args"], storage=a.storage,
                                   tol=0.0, max_iter=10 ** 6)
                except ValueError as e:              # a library that does not know this loss (rbl_create rejects the id)
                    print(f"  {fam} {loss}: not measured ({e})", flush=True)
                    unknown.add(loss)
                    continue
                s.generate_synthetic(seed=17)
                s.gram()
                ld = s.info()["ld"]
                per[loss]["D_bytes"] = a.n * ld * esz[L.STORAGE[a.storage]]
                for _ in range(a.warmup):
                    s.step(False)
                ts, fused, zband = [], 0, 0
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    st = s.step(False)
                    ts.append((time.perf_counter() - t0) * 1e3)
                    fused += int(st.fused)
                    zband += int(st.zband)
                per[loss]["iter_ms"].append(statistics.median(ts))
                per[loss]["fused_steps"].append(fused)
                per[loss]["zband_steps"].append(zband)
                s.profile_kernels(1)
                s.reset_kernel_times()
                for _ in range(a.ksteps):
                    s.step(False)
                tot, cnt = 0.0, 0
                for which in (L.KERNEL_GEMV, L.KERNEL_GEMVT, L.KERNEL_SWEEP_ERM):
                    ms, c = s.kernel_time(which)
                    tot, cnt = tot + ms, cnt + c
                    if which == L.KERNEL_SWEEP_ERM:
                        per[loss]["sweep_erm_launches"].append(c)
                per[loss]["kernel_ms"].append(tot / cnt if cnt else float("nan"))
                per[loss]["launches_per_step"] = cnt / max(1, a.ksteps)
                s.close()
                print(f"  {fam} round {rnd} {loss}: {per[loss]['iter_ms'][-1]:.3f} ms/iteration, sweep kernel "
                      f"{per[loss]['kernel_ms'][-1]:.3f} ms x {per[loss]['launches_per_step']:.0f}; of {a.steps} timed steps "
                      f"fused {fused} zband {zband}; single-sweep launches in {a.ksteps} steps "
                      f"{per[loss]['sweep_erm_launches'][-1]}", flush=True)
                if fam == "erm" and (fused != a.steps or per[loss]["sweep_erm_launches"][-1] < a.ksteps):
                    sys.exit(f"{fam} {loss}: the single-sweep kernel did not run in every step - not the path this line times")
                if fam == "superquantile" and zband == 0:     # (a step whose band is not certified redoes its z-step sorted)
                    sys.exit(f"{fam} {loss}: the sort-free z-step ran in no step - not the path this line times")
        for loss in a.losses:
            p = per[loss]
            if loss in unknown or not p["iter_ms"]:
                record["results"].append(dict(family=fam, loss=loss, measured=False))
                continue
            km = statistics.median(p["kernel_ms"])
            line = dict(family=fam, loss=loss, measured=True, iter_ms_median=statistics.median(p["iter_ms"]),
                        iter_ms_min=min(p["iter_ms"]), iter_ms_max=max(p["iter_ms"]), iter_ms_rounds=p["iter_ms"], sweep_kernel_ms=km,
                        sweep_kernel_ms_rounds=p["kernel_ms"], sweep_launches_per_step=p["launches_per_step"], D_bytes=p["D_bytes"],
                        fused_steps_rounds=p["fused_steps"], zband_steps_rounds=p["zband_steps"],
                        sweep_erm_launches_rounds=p["sweep_erm_launches"],
                        sweep_GBps=p["D_bytes"] / km / 1e6)
            base = per.get("binary_cross_entropy")
            if loss != "binary_cross_entropy" and base and len(base["iter_ms"]) == len(p["iter_ms"]):
                line["over_bce_iter_ms_rounds"] = [x / b for x, b in zip(p["iter_ms"], base["iter_ms"])]
                line["over_bce_sweep_kernel_rounds"] = [x / b for x, b in zip(p["kernel_ms"], base["kernel_ms"])]
            record["results"].append(line)
            print(f"{fam:14s} {loss:21s} {line['iter_ms_median']:8.3f} ms/iteration [{line['iter_ms_min']:.3f} - {line['iter_ms_max']:.3f}]  "
                  f"sweep kernel {km:.3f} ms  D {p['D_bytes'] / 1e9:.2f} GB  {line['sweep_GBps']:.0f} GB/s"
                  + ("  / BCE per round: " + ", ".join(f"{r:.3f}" for r in line["over_bce_iter_ms_rounds"])
                     if "over_bce_iter_ms_rounds" in line else ""), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(record, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
