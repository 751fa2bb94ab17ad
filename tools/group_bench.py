#!/usr/bin/env python3
"""K superquantile levels on one on-device synthetic data set: a group step (the two passes over D shared by up to
k_per_pass members) against the same K members stepped one after another through rbl_step, interleaved in one process.

    python tools/group_bench.py [--n 6000000] [--d 1000] [--storage f32] [--ks 1 2 4 8] [--warmup 5] [--steps 20]
                                [--rounds 3] [--labels] [--out profiles/group_bench_C2sq.json]

Per K and per round: `warmup` + `steps` group steps, then `warmup` + `steps` sequential sweeps over the members (both
end in a host wait, so wall time is device time + launch gaps).  Reported: median over rounds and the spread
(min..max) of the per-iteration time of both, problems x iterations / s, and the bytes/s of D the group's shared
passes sustain if the whole step were passes (a lower bound: the step also holds K z-steps and w-steps).

--labels adds a third set of members to every round: the same K problems, members 2..K with random +-1 label vectors
of their own (drawn on the host, rbl_set_labels) - the shape of a one-vs-rest job.  Its group step runs between the
equal-label group and the sequential sweep of every round (relabelled_ms beside group_ms)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6_000_000)
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--storage", default="f32")
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--labels", action="store_true", help="also time a group whose members 2..K carry random labels of their own")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import admm_for_rank_based_loss_amd as rbl
    S, G = rbl._solver.Solver, rbl._solver.Group
    levels = [0.5, 0.9, 0.3, 0.7, 0.2, 0.8, 0.4, 0.6, 0.1, 0.95, 0.25, 0.75, 0.35, 0.65, 0.45, 0.55]
    kw = dict(reg=0.01, wstep=rbl._lib.WSTEP_L2, storage=a.storage, tol=0.0, max_iter=10 ** 6)
    owner = S(a.n, a.d, "superquantile", args=[levels[0]], **kw)
    owner.generate_synthetic(seed=17)
    owner.gram()
    esz = {0: 4, 1: 8, 2: 2}[rbl._lib.STORAGE[a.storage]]
    ld = owner.info()["ld"]
    dbytes = a.n * ld * esz
    y0 = owner.labels() if a.labels else None
    record = dict(labels=bool(a.labels), n=a.n, d=a.d, storage=a.storage, warmup=a.warmup, steps=a.steps, rounds=a.rounds, D_bytes=dbytes, results=[])
    for K in a.ks:
        # two sets of members on the same D: one iterated as a group, one member by member
        grp_members = [S(a.n, a.d, "superquantile", args=[levels[k]], share=owner, **kw) for k in range(K)]
        seq_members = [S(a.n, a.d, "superquantile", args=[levels[k]], share=owner, **kw) for k in range(K)]
        g = G(grp_members)
        rel_members, gr = [], None
        if a.labels:
            import numpy as np
            rng = np.random.default_rng(1000 + K)
            rel_members = [S(a.n, a.d, "superquantile", args=[levels[k]], share=owner, **kw) for k in range(K)]
            for s in rel_members[1:]:
                s.set_labels(np.where(rng.random(a.n) < 0.5, -1.0, 1.0))
            gr = G(rel_members)
        tg, ts, tr = [], [], []
        for _ in range(a.rounds):
            for _ in range(a.warmup):
                g.step()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                g.step()
            tg.append((time.perf_counter() - t0) / a.steps)
            if gr is not None:
                for _ in range(a.warmup):
                    gr.step()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    gr.step()
                tr.append((time.perf_counter() - t0) / a.steps)
            for _ in range(a.warmup):
                for s in seq_members:
                    s.step()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                for s in seq_members:
                    s.step()
            ts.append((time.perf_counter() - t0) / a.steps)
        cnt = g.counters()
        kpp = cnt["k_per_pass"]
        passes = 2 * -(-K // kpp)
        mg, ms = statistics.median(tg), statistics.median(ts)
        res = dict(K=K, k_per_pass=kpp, group_ms=mg * 1e3, group_ms_range=[min(tg) * 1e3, max(tg) * 1e3],
                   sequential_ms=ms * 1e3, sequential_ms_range=[min(ts) * 1e3, max(ts) * 1e3], speedup=ms / mg,
                   group_problem_iters_per_s=K / mg, sequential_problem_iters_per_s=K / ms,
                   shared_passes_per_step=passes, D_bytes_per_s_lower_bound=passes * dbytes / mg,
                   shared_v=cnt["shared_v"], shared_q=cnt["shared_q"], single_passes=cnt["single_passes"])
        if gr is not None:
            cr = gr.counters()
            mr = statistics.median(tr)
            res.update(relabelled_ms=mr * 1e3, relabelled_ms_range=[min(tr) * 1e3, max(tr) * 1e3], relabelled_over_equal=mr / mg,
                       relabelled_shared_v=cr["shared_v"], relabelled_shared_q=cr["shared_q"],
                       relabelled_single_passes=cr["single_passes"])
        record["results"].append(res)
        print(json.dumps(res), flush=True)
        g.close()
        if gr is not None:
            gr.close()
        for s in grp_members + seq_members + rel_members:
            s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
