#!/usr/bin/env python3
"""Timings of the typed data path (include/rbl.h: rbl_set_data_from) -> one JSON document.

    python tools/upload_sources.py [--n 6000000] [--d 1000] [--out profiles/upload_sources.json]

Three measurements, each in a fresh child process under its own time limit, medians of 5 runs, variants interleaved:

  device   an n x d float32 device tensor -> fp32 storage: the forming pass (HIP events inside the library,
           rbl_kernel_time RBL_KERNEL_SRC_FORM) against torch.mul(X, -y[:, None]) on the same tensor (a stock kernel that
           moves the same bytes) and against a device-to-device copy of the tensor.
  fit      the same tensor with scaling="fit": statistics pass and forming pass separately.
  host     the same matrix as a float32 host array through set_data against the float64 route (a float64 host copy, then
           rbl_set_data): wall time of both, the conversion's share, peak host memory of each (its own process each).
"""
import argparse
import json
import os
import resource
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 5


def _med(v):
    return float(statistics.median(v))


def _labels(n):
    import numpy as np
    return np.where(np.random.default_rng(1).random(n) < 0.5, 1.0, -1.0)


def step_device(n, d, fit):
    import numpy as np
    import torch
    import admm_for_rank_based_loss_amd as rbl
    L = rbl._lib
    y = _labels(n)
    X = torch.empty((n, d), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, 500_000):
        X[r0:r0 + 500_000].normal_()
    yneg = torch.from_numpy(-y).to(device="cuda", dtype=torch.float32)[:, None]
    out = torch.empty_like(X)
    s = rbl.Solver(n, d, "erm", storage="f32", objective_only=True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    t = dict(form=[], stats=[], mul=[], copy=[], wall=[])
    for rep in range(REPS + 1):                          # (the first round warms every variant up)
        t0 = time.perf_counter()
        s.set_data(X, y, scaling="fit" if fit else "none")
        wall = (time.perf_counter() - t0) * 1e3
        form = s.kernel_time(L.KERNEL_SRC_FORM)[0]
        stats = s.kernel_time(L.KERNEL_SRC_STATS)[0]
        mul = timed(lambda: torch.mul(X, yneg, out=out))
        cp = timed(lambda: out.copy_(X))
        if rep:
            for k, v in (("form", form), ("stats", stats), ("mul", mul), ("copy", cp), ("wall", wall)):
                t[k].append(v)
    gb = n * d * 4 / 1e9
    res = dict(n=n, d=d, source="float32 device tensor", storage="f32", scaling="fit" if fit else "none", reps=REPS,
               form_ms=_med(t["form"]), form_GBs=2 * gb / (_med(t["form"]) / 1e3),
               torch_mul_ms=_med(t["mul"]), torch_mul_GBs=2 * gb / (_med(t["mul"]) / 1e3),
               device_copy_ms=_med(t["copy"]), device_copy_GBs=2 * gb / (_med(t["copy"]) / 1e3),
               form_over_torch_mul=_med(t["form"]) / _med(t["mul"]), set_data_wall_ms=_med(t["wall"]),
               form_ms_all=t["form"], torch_mul_ms_all=t["mul"])
    if fit:
        res.update(stats_ms=_med(t["stats"]), stats_GBs=gb / (_med(t["stats"]) / 1e3), stats_ms_all=t["stats"])
    s.close()
    return res


def step_host(n, d, route):
    """one route per process, so that ru_maxrss is that route's peak"""
    import numpy as np
    import admm_for_rank_based_loss_amd as rbl
    L = rbl._lib
    y = _labels(n)
    rng = np.random.default_rng(0)
    X = np.empty((n, d), dtype=np.float32)
    for r0 in range(0, n, 250_000):
        X[r0:r0 + 250_000] = rng.standard_normal((min(250_000, n - r0), d), dtype=np.float32)
    base_rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6
    s = rbl.Solver(n, d, "erm", storage="f32", objective_only=True)
    wall, conv, form = [], [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        if route == "float32":
            s.set_data(X, y)
            t1 = t0
        else:                                            # what the float64-only entry point asked of the caller
            X64 = np.ascontiguousarray(X, dtype=np.float64)
            t1 = time.perf_counter()
            s.set_data_f64(X64, y)
            del X64
        t2 = time.perf_counter()
        if rep:
            wall.append(t2 - t0)
            conv.append(t1 - t0)
            form.append(s.kernel_time(L.KERNEL_SRC_FORM)[0] / 1e3)
    res = dict(n=n, d=d, route=route, reps=REPS, wall_s=_med(wall), host_conversion_s=_med(conv),
               bytes_over_pcie_GB=n * d * (4 if route == "float32" else 8) / 1e9,
               GBs_of_source=n * d * (4 if route == "float32" else 8) / 1e9 / (_med(wall) - _med(conv)),
               peak_host_rss_GB=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6,
               host_rss_before_upload_GB=base_rss, wall_s_all=wall)
    if route == "float32":
        res["pipelined_pass_s"] = _med(form)
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6_000_000)
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upload_sources.json"))
    ap.add_argument("--step", default=None)
    ap.add_argument("--limit", type=int, default=420, help="time limit of one step in seconds")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--only-host", action="store_true", help="the host steps alone (e.g. at a smaller --n; results are merged into --out)")
    a = ap.parse_args()
    if a.step:
        if a.step == "device":
            r = step_device(a.n, a.d, False)
        elif a.step == "fit":
            r = step_device(a.n, a.d, True)
        else:
            r = step_host(a.n, a.d, a.step.split(":")[1])
        print("RESULT " + json.dumps(r))
        return 0
    steps = ([] if a.only_host else ["device", "fit"]) + ([] if a.skip_host else ["host:float32", "host:float64"])
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    for st in steps:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", st, "--n", str(a.n),
               "--d", str(a.d)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(f"step {st}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1                                     # nothing more is started after a step that failed
        doc[st] = json.loads(lines[-1][7:])
        print(st, json.dumps(doc[st]))
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
