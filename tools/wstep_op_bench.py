#!/usr/bin/env python3
"""What the operator w-step (gram="none": no Gram matrix, csrc/wstep_op.hip) costs against the Gram route where both run,
and what an iteration costs where only it can run.

    python tools/wstep_op_bench.py [--both 1000000x10000@100] [--wide 1000000x200000@50] [--rounds 3]
                                   [--out profiles/wstep_op.json]

A configuration is NxD@K: K entries per row, one per stride of D / K columns, N(0, 1) float32 values, labels from a
planted linear model with 5 % flips (the generator of tools/csr_storage_bench.py: the library's own generator is refused
for storage "csr", and this one builds 10^8 entries in seconds where scipy.sparse.random takes minutes).  The matrix goes
through rbl_set_data_csr as a SciPy CSR matrix.

(a) --both: widths where the Gram route runs too (ld <= 16 384).  erm / l2.  gram="dense" and gram="none" interleaved in one
    process, one warm-up round and `rounds` rounds; per round and route: setup (set_data, gram: wall), `steps` iterations
    (wall, ms per iteration), the w-step alone (HIP events around the phase, rbl_profile_kernels level 2) and the inner
    iterations per w-step.
(b) --wide: widths past the Gram route.  erm / l2 and superquantile / elastic net (per-coordinate l1, l2), gram="none": ms
    per iteration, inner iterations, and the sparse passes' share of the w-step - (inner iterations + 1) operator
    applications, each one v pass and one q pass at the cost the iteration's own passes are timed at (rbl_kernel_time).

One child process per configuration and family under its own time limit; after a child that failed or ran out of time
nothing more is started.  Medians over the rounds are reported, every round's figures are kept."""
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
    "erm_l2": dict(weight_function="erm", args=None, enet=False),
    "superquantile_enet": dict(weight_function="superquantile", args=[0.5], enet=True),
}


def make_matrix(n, d, k, seed=17):
    import numpy as np
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
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
    import admm_for_rank_based_loss_amd as rbl
    L = rbl._lib
    n, d, k = a.n, a.d, a.k
    f = FAMILIES[a.family]
    A, y = make_matrix(n, d, k)
    routes = ["dense", "none"] if a.part == "both" else ["none"]
    runs = {r: [] for r in routes}
    rng = np.random.default_rng(3)
    # (the thresholds are l1_j / (2 rho) with rho starting at 1e-5: penalties of this size leave a support that is neither
    # empty nor full - the reported `support` says what it was)
    l1 = rng.uniform(0.5e-6, 2e-6, d) if f["enet"] else None
    l2 = rng.uniform(0.5e-3, 2e-3, d) if f["enet"] else None
    for rnd in range(a.rounds + 1):          # round 0 warms up
        for route in routes:
            s = rbl.Solver(n, d, f["weight_function"], "binary_cross_entropy", reg=0.01,
                           wstep=L.WSTEP_L1 if f["enet"] else L.WSTEP_L2, args=f["args"], storage="csr", tol=0.0,
                           max_iter=10 ** 6, gram=route)
            t0 = time.perf_counter()
            s.set_data(A, y)
            t1 = time.perf_counter()
            s.gram()
            t2 = time.perf_counter()
            if f["enet"]:
                s.set_penalty(l1, l2)
            for _ in range(a.warmup):
                s.step(False)
            ts, inner, forms = [], [], set()
            for _ in range(a.steps):
                t = time.perf_counter()
                st = s.step(False)
                ts.append((time.perf_counter() - t) * 1e3)
                inner.append(st.inner_iters)
                forms.add(int(st.wstep_form))
            s.profile_kernels(2)
            s.reset_kernel_times()
            ms_w = []
            for _ in range(a.ksteps):
                ms_w.append(s.step(False).ms_w)
            kt = {}
            for key, which in (("v", L.KERNEL_GEMV), ("q", L.KERNEL_GEMVT)):
                ms, c = s.kernel_time(which)
                kt[key] = ms / c if c else None
            support = int(np.count_nonzero(s.get_state(want_z=False, want_lam=False)["w"]))
            s.close()
            r = dict(round=rnd, support=support, upload_s=t1 - t0, gram_s=t2 - t1, iter_ms=statistics.median(ts), wstep_ms=statistics.median(ms_w),
                     inner_iters=statistics.mean(inner), wstep_forms=sorted(forms), v_ms=kt["v"], q_ms=kt["q"])
            if route == "none" and kt["v"] and kt["q"] and r["wstep_ms"] > 0:
                r["op_pass_share_of_wstep"] = (r["inner_iters"] + 1) * (kt["v"] + kt["q"]) / r["wstep_ms"]
            if rnd > 0:
                runs[route].append(r)
            print(f"  round {rnd} gram={route:5s} upload {r['upload_s']:.3f} s gram {r['gram_s']:.3f} s iter {r['iter_ms']:.3f} ms "
                  f"w-step {r['wstep_ms']:.3f} ms inner {r['inner_iters']:.1f} forms {r['wstep_forms']} support {support}", file=sys.stderr, flush=True)
    out = dict(part=a.part, n=n, d=d, per_row=k, nnz=int(A.nnz), family=a.family, rounds=a.rounds, steps=a.steps, ksteps=a.ksteps,
               routes={})
    for route in routes:
        keys = ("upload_s", "gram_s", "iter_ms", "wstep_ms", "inner_iters", "v_ms", "q_ms", "op_pass_share_of_wstep", "support")
        med = {}
        for key in keys:
            xs = [r[key] for r in runs[route] if r.get(key) is not None]
            med[key] = statistics.median(xs) if xs else None
        out["routes"][route] = dict(median=med, runs=runs[route])
    if a.part == "both":
        out["none_over_dense_iter_ms_rounds"] = [b["iter_ms"] / c["iter_ms"] for b, c in zip(runs["none"], runs["dense"])]
        out["none_over_dense_wstep_ms_rounds"] = [b["wstep_ms"] / c["wstep_ms"] for b, c in zip(runs["none"], runs["dense"])]
    print(json.dumps(out))


def parse(cfg):
    shape, k = cfg.split("@")
    n, d = (int(v) for v in shape.split("x"))
    return n, d, int(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--both", nargs="*", default=["1000000x10000@100"])
    ap.add_argument("--wide", nargs="*", default=["1000000x200000@50"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ksteps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds one child may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wstep_op.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--part")
    ap.add_argument("--n", type=int)
    ap.add_argument("--d", type=int)
    ap.add_argument("--k", type=int)
    ap.add_argument("--family")
    a = ap.parse_args()
    if a.child:
        return child(a)
    record = dict(rounds=a.rounds, warmup=a.warmup, steps=a.steps, ksteps=a.ksteps, results=[])
    if os.path.exists(a.out):                 # runs accumulate: a later call adds configurations
        with open(a.out) as fh:
            record["results"] = json.load(fh).get("results", [])
    jobs = [("both", cfg, "erm_l2") for cfg in a.both] + [("wide", cfg, fam) for cfg in a.wide for fam in sorted(FAMILIES)]
    for part, cfg, fam in jobs:
        n, d, k = parse(cfg)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--part", part, "--n", str(n), "--d", str(d), "--k", str(k),
               "--family", fam, "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--steps", str(a.steps), "--ksteps", str(a.ksteps)]
        print(f"{part} {cfg} {fam}:", flush=True)
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
            if p.returncode != 0:
                res = dict(part=part, n=n, d=d, per_row=k, family=fam, error=f"exit status {p.returncode}")
            else:
                res = json.loads(p.stdout.strip().splitlines()[-1])
        except subprocess.TimeoutExpired:
            res = dict(part=part, n=n, d=d, per_row=k, family=fam, error=f"not finished within {a.limit} s")
        same = lambda r: (r.get("part"), r.get("n"), r.get("d"), r.get("per_row"), r.get("family")) == (part, n, d, k, fam)
        record["results"] = [r for r in record["results"] if not same(r)] + [res]      # a re-run replaces its configuration
        for route, v in res.get("routes", {}).items():
            m = v["median"]
            print(f"  gram={route:5s} setup {m['upload_s']:.3f} + {m['gram_s']:.3f} s  {m['iter_ms']:.3f} ms/iteration  w-step "
                  f"{m['wstep_ms']:.3f} ms  {m['inner_iters']:.1f} inner iterations  passes' share {m['op_pass_share_of_wstep']}", flush=True)
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
