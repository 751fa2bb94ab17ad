#!/usr/bin/env python3
"""What shared sparse passes (``share_sparse=True``, RBL_GROUP_SHARE_SPARSE) gain a group on storage="csr".

    python tools/csr_group_bench.py [--configs 1000000x1000@0.01 ...] [--families erm superquantile] [--ks 2 4 8]
                                    [--rounds 3] [--out profiles/csr_group.json]

One child process per (configuration, family), each under its own time limit (--limit seconds; a child that runs out is
recorded as such, and nothing more is started on the device after it).  A child uploads the matrix once (one owner
handle, everything else borrows its D and G) and, for every K, interleaves three variants - "shared" (a group with
share_sparse on), "unshared" (the same group with it off: every member's own passes, the behaviour without the flag) and
"standalone" (K solvers stepped in turn) - one warm-up round, then `rounds` rounds; in a round every variant is built,
runs `warmup` + `steps` wall-timed steps, then `ksteps` more with HIP events around the passes, and is destroyed.  The
members are K regularisation strengths of the family.  Recorded per K and variant, medians over the rounds with every
round kept: the step of all K members (ms), the v and q passes of such a step (shared: the events of rbl_group_profile
around the batches; unshared / standalone: the members' own rbl_kernel_time sums, K passes each) and, shared only, the
interleaving kernel of one batch.  The matrix and its float32 / int32 source are tools/csr_storage_bench.py's."""
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

from csr_storage_bench import FAMILIES, make_matrix  # noqa: E402

VARIANTS = ("shared", "unshared", "standalone")


def child(a):
    import admm_for_rank_based_loss_amd as rbl
    L = rbl._lib
    n, d = a.n, a.d
    f = FAMILIES[a.family]
    A, y = make_matrix(n, d, a.density)
    nnz = int(A.nnz)

    def solver(reg, share=None):
        return rbl.Solver(n, d, f["weight_function"], "binary_cross_entropy", reg=reg, wstep=L.WSTEP_L1 if f["wstep"] == "l1" else L.WSTEP_L2,
                          args=f["args"], storage="csr", tol=0.0, max_iter=10 ** 6, share=share)

    owner = solver(0.01)
    t0 = time.perf_counter()
    owner.set_data(A, y)
    owner.gram()
    print(f"  upload + gram {time.perf_counter() - t0:.1f} s, nnz {nnz}", file=sys.stderr, flush=True)
    out = dict(n=n, d=d, density=a.density, nnz=nnz, family=a.family, rounds=a.rounds, steps=a.steps, ksteps=a.ksteps, K={})
    for K in a.ks:
        runs = {v: [] for v in VARIANTS}
        for rnd in range(a.rounds + 1):      # round 0 warms up
            for variant in VARIANTS:
                members = [solver(0.01 * 2.0 ** -k, share=owner) for k in range(K)]
                g = rbl._solver.Group(members, share_sparse=variant == "shared") if variant != "standalone" else None

                def step():
                    if g is not None:
                        g.step(False)
                    else:
                        for s in members:
                            s.step(False)

                for _ in range(a.warmup):
                    step()
                ts = []
                for _ in range(a.steps):
                    t = time.perf_counter()
                    step()
                    ts.append((time.perf_counter() - t) * 1e3)
                pack = None
                if variant == "shared":
                    g.profile(True)
                    for _ in range(a.ksteps):
                        step()
                    pt = g.pass_times()
                    v_ms, q_ms, pack = pt["v"], pt["q"], pt["pack"]
                    cnt = g.counters()
                    assert pt["steps"] == a.ksteps and cnt["k_per_pass"] == 4 and cnt["shared_v"] == cnt["shared_q"] > 0, (pt, cnt)
                else:
                    for s in members:
                        s.profile_kernels(1)
                        s.reset_kernel_times()
                    for _ in range(a.ksteps):
                        step()
                    v_ms = sum(s.kernel_time(L.KERNEL_GEMV)[0] for s in members) / a.ksteps
                    q_ms = sum(s.kernel_time(L.KERNEL_GEMVT)[0] for s in members) / a.ksteps
                    if g is not None:
                        cnt = g.counters()
                        assert cnt["k_per_pass"] == 1 and cnt["shared_v"] == cnt["shared_q"] == 0, cnt
                if g is not None:
                    g.close()
                for s in members:
                    s.close()
                r = dict(round=rnd, step_ms=statistics.median(ts), v_ms=v_ms, q_ms=q_ms, pack_ms=pack)
                if rnd > 0:
                    runs[variant].append(r)
                print(f"  K={K} round {rnd} {variant:10s} step {r['step_ms']:.3f} ms  v {v_ms:.3f}  q {q_ms:.3f}  pack {pack}",
                      file=sys.stderr, flush=True)
        res = {}
        for variant in VARIANTS:
            med = {k: statistics.median(r[k] for r in runs[variant]) for k in ("step_ms", "v_ms", "q_ms")}
            if variant == "shared":
                med["pack_ms"] = statistics.median(r["pack_ms"] for r in runs[variant])
            res[variant] = dict(median=med, runs=runs[variant])
        sh, un = res["shared"]["median"], res["unshared"]["median"]
        res["shared_over_unshared"] = {k: sh[k] / un[k] for k in ("step_ms", "v_ms", "q_ms")}
        res["step_ratio_rounds"] = [s["step_ms"] / u["step_ms"] for s, u in zip(runs["shared"], runs["unshared"])]
        res["shared_faster_every_round"] = all(x < 1.0 for x in res["step_ratio_rounds"])
        out["K"][str(K)] = res
    owner.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["1000000x1000@0.01", "1000000x1000@0.1", "1000000x10000@0.01"])
    ap.add_argument("--families", nargs="*", default=["erm", "superquantile"], choices=sorted(FAMILIES))
    ap.add_argument("--ks", nargs="*", type=int, default=[2, 4, 8])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--ksteps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds one child may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_group.json"))
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
                   "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--steps", str(a.steps), "--ksteps", str(a.ksteps),
                   "--ks"] + [str(k) for k in a.ks]
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
            for K, v in res.get("K", {}).items():
                for variant in VARIANTS:
                    m = v[variant]["median"]
                    print(f"  K={K} {variant:10s} step {m['step_ms']:.3f} ms  v {m['v_ms']:.3f} ms  q {m['q_ms']:.3f} ms"
                          + (f"  pack {m['pack_ms']:.3f} ms" if "pack_ms" in m else ""), flush=True)
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
