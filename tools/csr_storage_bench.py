#!/usr/bin/env python3
"""What sparse storage of D (storage="csr") costs and saves: upload, Gram matrix, the two passes, the iteration and the
resident memory, against the same sparse matrix solved with storage="f32" (the dense path) where that fits.

    python tools/csr_storage_bench.py [--configs 1000000x1000@0.01 ...] [--families superquantile erm] [--rounds 5]
                                      [--segs 128 512 2048] [--lanes 4 8 16 32] [--out profiles/csr_storage.json]

One child process per (configuration, family), each under its own time limit (--limit seconds; a child that runs out is
recorded as such).  Inside a child the variants - "csr", "f32", and for the tuning tables "csr seg=T" (RBL_CSC_SEG) and
"csr lanes=L" (RBL_CSR_LANES), read at upload by a library built with RBL_HIPCC_FLAGS=-DRBL_CSR_TUNING_HOOKS and by no
other (with the library as it ships these variants all run the constants) - are interleaved: one warm-up round, then `rounds`
rounds, each of which creates every variant's handle in turn: upload (wall), Gram (wall), `warmup` + `steps` timed
iterations, `ksteps` more with HIP events around the passes (rbl_kernel_time 0 = v = D w, 1 = q = D^T c), destroy.
Medians over the rounds are reported; every round's figure is kept.  GB/s counts 12 bytes per entry and pass (a 4-byte
index and an 8-byte value).  The matrix: `k = round(density d)` entries per row, one per stride of d / k columns, N(0, 1)
float32 values, labels from a planted linear model with 5 % flips."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILIES = {
    "superquantile": dict(weight_function="superquantile", wstep="l2", args=[0.5]),
    "erm": dict(weight_function="erm", wstep="l1", args=None),
}
F32_LIMIT_BYTES = 64e9        # the dense yardstick is run where n ld 4 stays below this


def make_matrix(n, d, density, seed=17):
    import numpy as np
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    k = max(1, int(round(density * d)))
    stride = d // k
    cols = (np.arange(k, dtype=np.int32) * stride)[None, :] + rng.integers(0, stride, size=(n, k), dtype=np.int32)
    vals = rng.standard_normal(n * k, dtype=np.float32)
    A = sp.csr_matrix((vals, cols.reshape(-1), np.arange(n + 1, dtype=np.int64) * k), shape=(n, d))
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int64) if n * k >= 2 ** 31 else A.indptr.astype(np.int32)
    w = rng.standard_normal(d) / np.sqrt(k)
    y = np.where((A @ w + 0.1 * rng.standard_normal(n) > 0) ^ (rng.random(n) < 0.05), 1.0, -1.0)
    return A, y


def child(a):
    import numpy as np
    import torch
    import admm_for_rank_based_loss_amd as rbl
    L = rbl._lib
    n, d, density = a.n, a.d, a.density
    f = FAMILIES[a.family]
    A, y = make_matrix(n, d, density)
    nnz = int(A.nnz)
    variants = [("csr", {})]
    if n * L.storage_ld(d, "f32") * 4 <= F32_LIMIT_BYTES and not a.no_f32:
        variants.append(("f32", {}))
    variants += [(f"csr seg={t}", {"RBL_CSC_SEG": str(t)}) for t in a.segs]
    variants += [(f"csr lanes={l}", {"RBL_CSR_LANES": str(l)}) for l in a.lanes]
    runs = {name: [] for name, _ in variants}

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info(0)
        return total - free

    for rnd in range(a.rounds + 1):          # round 0 warms up
        for name, env in variants:
            os.environ.update(env)
            try:
                u0 = used()
                s = rbl.Solver(n, d, f["weight_function"], "binary_cross_entropy", reg=0.01,
                               wstep=L.WSTEP_L1 if f["wstep"] == "l1" else L.WSTEP_L2, args=f["args"], storage=name.split()[0],
                               tol=0.0, max_iter=10 ** 6)
                t0 = time.perf_counter()
                s.set_data(A, y)
                t1 = time.perf_counter()
                s.gram()
                t2 = time.perf_counter()
            finally:
                for k in env:
                    os.environ.pop(k, None)
            mem = used() - u0
            fused = 0
            for _ in range(a.warmup):
                s.step(False)
            ts = []
            for _ in range(a.steps):
                t = time.perf_counter()
                fused += s.step(False).fused
                ts.append((time.perf_counter() - t) * 1e3)
            s.profile_kernels(1)
            s.reset_kernel_times()
            for _ in range(a.ksteps):
                s.step(False)
            kt = {}
            for key, which in (("v", L.KERNEL_GEMV), ("q", L.KERNEL_GEMVT), ("erm", L.KERNEL_SWEEP_ERM)):
                ms, c = s.kernel_time(which)
                kt[key] = ms / c if c else None
            s.close()
            r = dict(round=rnd, upload_s=t1 - t0, gram_s=t2 - t1, iter_ms=statistics.median(ts), iter_per_s=1e3 / statistics.median(ts),
                     v_ms=kt["v"], q_ms=kt["q"], erm_sweep_ms=kt["erm"], fused_steps=fused, resident_bytes=mem)
            if rnd > 0:
                runs[name].append(r)
            print(f"  round {rnd} {name:14s} upload {r['upload_s']:.3f} s gram {r['gram_s']:.3f} s iter {r['iter_ms']:.3f} ms "
                  f"v {kt['v']} q {kt['q']} erm {kt['erm']} mem {mem / 1e6:.0f} MB", file=sys.stderr, flush=True)

    def med(name, key):
        xs = [r[key] for r in runs[name] if r[key] is not None]
        return statistics.median(xs) if xs else None

    out = dict(n=n, d=d, density=density, nnz=nnz, family=a.family, rounds=a.rounds, steps=a.steps, ksteps=a.ksteps, variants={})
    for name, _ in variants:
        m = {k: med(name, k) for k in ("upload_s", "gram_s", "iter_ms", "iter_per_s", "v_ms", "q_ms", "erm_sweep_ms", "resident_bytes")}
        if name.startswith("csr"):
            for p in ("v", "q"):
                m[p + "_GBps"] = 12.0 * nnz / m[p + "_ms"] / 1e6 if m[p + "_ms"] else None
            if m["v_ms"] and m["q_ms"]:
                m["outside_passes_ms"] = m["iter_ms"] - m["v_ms"] - m["q_ms"]
                m["outside_exceeds_passes"] = m["outside_passes_ms"] > m["v_ms"] + m["q_ms"]
        out["variants"][name] = dict(median=m, runs=runs[name])
    if "f32" in runs:
        out["csr_over_f32_iter_ms_rounds"] = [c["iter_ms"] / f32["iter_ms"] for c, f32 in zip(runs["csr"], runs["f32"])]
        out["csr_faster_than_f32"] = all(x < 1.0 for x in out["csr_over_f32_iter_ms_rounds"])
    else:
        out["f32"] = f"not run: dense f32 storage needs {n * L.storage_ld(d, 'f32') * 4 / 1e9:.0f} GB"
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["1000000x1000@0.001", "1000000x1000@0.01", "1000000x1000@0.1", "1000000x10000@0.01"])
    ap.add_argument("--families", nargs="*", default=["superquantile", "erm"], choices=sorted(FAMILIES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--ksteps", type=int, default=10)
    ap.add_argument("--segs", nargs="*", type=int, default=[])
    ap.add_argument("--lanes", nargs="*", type=int, default=[])
    ap.add_argument("--no-f32", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="seconds one child may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_storage.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int)
    ap.add_argument("--d", type=int)
    ap.add_argument("--density", type=float)
    ap.add_argument("--family")
    a = ap.parse_args()
    if a.child:
        return child(a)
    record = dict(rounds=a.rounds, warmup=a.warmup, steps=a.steps, ksteps=a.ksteps, results=[])
    if os.path.exists(a.out):                 # runs accumulate: a later call adds configurations
        with open(a.out) as fh:
            record["results"] = json.load(fh).get("results", [])
    for cfg in a.configs:
        shape, density = cfg.split("@")
        n, d = (int(v) for v in shape.split("x"))
        for fam in a.families:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--n", str(n), "--d", str(d), "--density", density, "--family", fam,
                   "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--steps", str(a.steps), "--ksteps", str(a.ksteps)]
            cmd += (["--segs"] + [str(t) for t in a.segs] if a.segs else []) + (["--lanes"] + [str(l) for l in a.lanes] if a.lanes else [])
            cmd += ["--no-f32"] if a.no_f32 else []
            print(f"{cfg} {fam}:", flush=True)
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
                if p.returncode != 0:
                    res = dict(n=n, d=d, density=float(density), family=fam, error=f"exit status {p.returncode}")
                else:
                    res = json.loads(p.stdout.strip().splitlines()[-1])
            except subprocess.TimeoutExpired:
                res = dict(n=n, d=d, density=float(density), family=fam, error=f"not finished within {a.limit} s")
            same = lambda r: (r.get("n"), r.get("d"), r.get("density"), r.get("family")) == (n, d, float(density), fam)
            record["results"] = [r for r in record["results"] if not same(r)] + [res]      # a re-run replaces its configuration
            for name, v in res.get("variants", {}).items():
                m = v["median"]
                print(f"  {name:14s} upload {m['upload_s']:.3f} s  gram {m['gram_s']:.3f} s  {m['iter_ms']:.3f} ms/iteration "
                      f"({m['iter_per_s']:.0f}/s)  v {m['v_ms']} ms  q {m['q_ms']} ms  {m['resident_bytes'] / 1e6:.0f} MB", flush=True)
            if "error" in res:
                print("  " + res["error"], flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(record, fh, indent=1)
            if "error" in res:                # nothing more is started on the device after a child that failed or hung
                print("stopping: the child did not finish cleanly", flush=True)
                return 1
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
