#!/usr/bin/env python3
"""What the working-set lasso (l1_solver="working_set": csrc/wstep_ws.hip) costs against FISTA on the operator where only
the gram="none" route runs, and against the Gram route's exact active-set kernel where both run.

    python tools/wstep_ws_bench.py [--wide 1000000x200000@50] [--both 1000000x10000@100] [--families erm_l1 ...]
                                   [--l1-reg 1e-3] [--rounds 3] [--out profiles/wstep_ws.json]

A configuration is NxD@K (the generator of tools/wstep_op_bench.py: K entries per row, N(0, 1) float32 values, labels from
a planted linear model with 5 % flips), uploaded through rbl_set_data_csr as a SciPy CSR matrix.

(a) --wide: gram="none".  superquantile / elastic net (the penalties of tools/wstep_op_bench.py) and erm / l1.
    l1_solver="working_set" and "fista" interleaved in one process, one warm-up round and `rounds` rounds; per round and
    solver: `warmup + steps` iterations from the same start - ms per iteration (wall) over the last `steps`, the w-step
    alone over `ksteps` more (HIP events around the phase), inner iterations, and for the working set the rounds, the
    D^T (D w) evaluations (pass pairs) and the rows of the sub-Gram matrix formed per w-step; then the objective of both
    after the same number of iterations.
(b) --both: widths where the Gram route runs too.  erm / l1: gram="dense" (the active-set kernel on G) against gram="none"
    with the working set, the same figures.

One child process per configuration and family under its own time limit; after a child that failed or ran out of time
nothing more is started.  Medians over the rounds are reported, every round's figures are kept; runs accumulate in the
output file, one record per configuration, family and --l1-reg (the erm / l1 family's penalty: it sets the support)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FAMILIES = {
    "superquantile_enet": dict(weight_function="superquantile", args=[0.5], enet=True),
    "erm_l1": dict(weight_function="erm", args=None, enet=False),
}


def child(a):
    import numpy as np
    import admm_for_rank_based_loss_amd as rbl
    from wstep_op_bench import make_matrix
    L = rbl._lib
    n, d, k = a.n, a.d, a.k
    f = FAMILIES[a.family]
    A, y = make_matrix(n, d, k)
    # (solver name, gram, l1_solver)
    variants = [("working_set", "none", "working_set"), ("fista", "none", "fista")] if a.part == "wide" else \
               [("working_set", "none", "working_set"), ("gram_route", "dense", "fista")]
    runs = {v[0]: [] for v in variants}
    rng = np.random.default_rng(3)
    l1 = rng.uniform(0.5e-6, 2e-6, d) if f["enet"] else None
    l2 = rng.uniform(0.5e-3, 2e-3, d) if f["enet"] else None
    for rnd in range(a.rounds + 1):          # round 0 warms up
        for name, gram, l1_solver in variants:
            s = rbl.Solver(n, d, f["weight_function"], "binary_cross_entropy", reg=a.l1_reg, wstep=L.WSTEP_L1, args=f["args"],
                           storage="csr", tol=0.0, max_iter=10 ** 6, gram=gram, l1_solver=l1_solver)
            s.set_data(A, y)
            s.gram()
            if f["enet"]:
                s.set_penalty(l1, l2)
            ws = l1_solver == "working_set"
            ts, inner, forms, rounds_, pairs, rows = [], [], set(), [], [], []
            for i in range(a.warmup + a.steps):
                t = time.perf_counter()
                st = s.step(False)
                dt = (time.perf_counter() - t) * 1e3
                info = s.wset_info() if ws else None
                if i >= a.warmup:
                    ts.append(dt)
                    inner.append(st.inner_iters)
                    forms.add(int(st.wstep_form))
                    if ws:
                        rounds_.append(info["rounds"])
                        pairs.append(info["pass_pairs"])
                        rows.append(info["rows_last"])
            w = s.get_state(want_z=False, want_lam=False)["w"]
            objective = float(s.objective(w))
            support = int(np.count_nonzero(w))
            info = s.wset_info() if ws else {}
            s.profile_kernels(2)
            ms_w = [s.step(False).ms_w for _ in range(a.ksteps)]
            s.close()
            r = dict(round=rnd, iter_ms=statistics.median(ts), wstep_ms=statistics.median(ms_w), inner_iters=statistics.mean(inner),
                     wstep_forms=sorted(forms), support=support, objective=objective,
                     rounds_per_wstep=statistics.mean(rounds_) if ws else None,
                     pass_pairs_per_wstep=statistics.mean(pairs) if ws else None,
                     gs_rows_per_iteration=statistics.mean(rows) if ws else None,
                     slots=info.get("slots"), gs_rows_total=info.get("rows_total"), evictions=info.get("evictions"))
            if rnd > 0:
                runs[name].append(r)
            print(f"  round {rnd} {name:11s} iter {r['iter_ms']:.3f} ms w-step {r['wstep_ms']:.3f} ms inner {r['inner_iters']:.1f} forms "
                  f"{r['wstep_forms']} support {support} objective {objective!r} rounds {r['rounds_per_wstep']} pairs "
                  f"{r['pass_pairs_per_wstep']} rows {r['gs_rows_per_iteration']} slots {r['slots']}", file=sys.stderr, flush=True)
    out = dict(part=a.part, n=n, d=d, per_row=k, nnz=int(A.nnz), family=a.family, l1_reg=a.l1_reg, rounds=a.rounds, warmup=a.warmup,
               steps=a.steps, ksteps=a.ksteps, solvers={})
    keys = ("iter_ms", "wstep_ms", "inner_iters", "support", "objective", "rounds_per_wstep", "pass_pairs_per_wstep",
            "gs_rows_per_iteration", "slots")
    for name, _, _ in variants:
        med = {}
        for key in keys:
            xs = [r[key] for r in runs[name] if r.get(key) is not None]
            med[key] = statistics.median(xs) if xs else None
        out["solvers"][name] = dict(median=med, runs=runs[name])
    other = variants[1][0]
    out[f"{other}_over_working_set_iter_ms_rounds"] = [b["iter_ms"] / c["iter_ms"] for b, c in zip(runs[other], runs["working_set"])]
    print(json.dumps(out))


def parse(cfg):
    shape, k = cfg.split("@")
    n, d = (int(v) for v in shape.split("x"))
    return n, d, int(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", nargs="*", default=["1000000x200000@50"])
    ap.add_argument("--both", nargs="*", default=["1000000x10000@100"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ksteps", type=int, default=5)
    ap.add_argument("--l1-reg", dest="l1_reg", type=float, default=1e-3, help="the scalar l1 penalty of the erm / l1 family")
    ap.add_argument("--families", nargs="*", default=sorted(FAMILIES), help="the families of --wide")
    ap.add_argument("--limit", type=int, default=400, help="seconds one child may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wstep_ws.json"))
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
    jobs = [("wide", cfg, fam) for cfg in a.wide for fam in a.families] + [("both", cfg, "erm_l1") for cfg in a.both]
    for part, cfg, fam in jobs:
        n, d, k = parse(cfg)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--part", part, "--n", str(n), "--d", str(d), "--k", str(k),
               "--family", fam, "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--steps", str(a.steps), "--ksteps", str(a.ksteps),
               "--l1-reg", repr(a.l1_reg)]
        print(f"{part} {cfg} {fam}:", flush=True)
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
            if p.returncode != 0:
                res = dict(part=part, n=n, d=d, per_row=k, family=fam, error=f"exit status {p.returncode}")
            else:
                res = json.loads(p.stdout.strip().splitlines()[-1])
        except subprocess.TimeoutExpired:
            res = dict(part=part, n=n, d=d, per_row=k, family=fam, error=f"not finished within {a.limit} s")
        res.setdefault("l1_reg", a.l1_reg)
        same = lambda r: (r.get("part"), r.get("n"), r.get("d"), r.get("per_row"), r.get("family"), r.get("l1_reg")) == (part, n, d, k, fam, a.l1_reg)
        record["results"] = [r for r in record["results"] if not same(r)] + [res]      # a re-run replaces its configuration
        for name, v in res.get("solvers", {}).items():
            m = v["median"]
            print(f"  {name:11s} {m['iter_ms']:.3f} ms/iteration  w-step {m['wstep_ms']:.3f} ms  {m['inner_iters']:.1f} inner iterations  "
                  f"support {m['support']}  objective {m['objective']!r}  rounds {m['rounds_per_wstep']}  pass pairs "
                  f"{m['pass_pairs_per_wstep']}  Gs rows / iteration {m['gs_rows_per_iteration']}", flush=True)
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
