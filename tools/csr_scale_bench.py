#!/usr/bin/env python3
"""What scale-only standardisation (standardize="scale": rbl_set_centering(h, 0) + RBL_SCALE_FIT) costs on storage="csr".

    python tools/csr_scale_bench.py [--configs 1000000x1000@10 1000000x200000@50] [--rounds 3] [--blocks 5] [--steps 20]
                                    [--out profiles/csr_scale.json]

A configuration is NxD@K (the generator of tools/wstep_op_bench.py: K entries per row, float32 values, here multiplied by a
unit per column drawn from exp(N(0, 2)) so that the columns need the scaling), uploaded as a SciPy CSR matrix on one GPU.

Per configuration, in one process:
(a) the upload: rbl_set_data_csr with RBL_SCALE_FIT and centring off against the same call with RBL_SCALE_NONE (the path
    the feature leaves as it was: the yardstick), wall time of the call, interleaved over `rounds` rounds after one warm-up
    round; and from rbl_kernel_time the statistics launches (RBL_KERNEL_SRC_STATS) and the store pass plus the scaling
    launches (RBL_KERNEL_SRC_FORM; the unscaled upload's RBL_KERNEL_SRC_FORM is the store pass alone).
(b) the iteration: the scaled handle against a handle given the host-prescaled matrix A . diag(1.0 / scale) - identical
    kernels on identically structured data, bit-identical iterates - erm / l1, `blocks` interleaved blocks of `steps`
    iterations each after a warm-up block; the ratio scaled / prescaled per block, its median and its spread (min, max).
    The expected ratio is 1 within that spread; nothing is asserted.

One child process per configuration under its own time limit; after a child that failed or ran out of time nothing more is
started.  The output file holds one record per configuration (a rerun replaces it)."""
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


def child(a):
    import numpy as np
    import admm_for_rank_based_loss_amd as rbl
    from wstep_op_bench import make_matrix
    L = rbl._lib
    n, d, k = a.n, a.d, a.k
    A, y = make_matrix(n, d, k)
    units = np.exp(2.0 * np.random.default_rng(5).standard_normal(d)).astype(np.float32)
    A.data *= units[A.indices]
    kw = dict(reg=1e-3, wstep=L.WSTEP_L1, storage="csr", tol=0.0, max_iter=10 ** 6)

    def upload(scaled, src=A):
        s = rbl.Solver(n, d, "erm", "binary_cross_entropy", **kw)
        if scaled:
            s.set_centering(False)
        t = time.perf_counter()
        s.set_data(src, y, scaling="fit" if scaled else "none")
        ms = (time.perf_counter() - t) * 1e3
        return s, dict(upload_ms=ms, stats_ms=s.kernel_time(L.KERNEL_SRC_STATS)[0], form_ms=s.kernel_time(L.KERNEL_SRC_FORM)[0])

    ups = {"scale": [], "none": []}
    for rnd in range(a.rounds + 1):          # round 0 warms up
        for name in ("none", "scale"):
            s, r = upload(name == "scale")
            s.close()
            if rnd > 0:
                ups[name].append(r)
            print(f"  round {rnd} upload {name:5s} {r['upload_ms']:.2f} ms stats {r['stats_ms']:.3f} ms form {r['form_ms']:.3f} ms",
                  file=sys.stderr, flush=True)
    hs, _ = upload(True)
    scale = hs.get_scaling()[1]
    B = A.copy()
    B.data = A.data.astype(np.float64) * (1.0 / scale)[A.indices]          # the device's multiplication, on the host
    hp, _ = upload(False, B)
    for h in (hs, hp):
        h.gram()
    blocks = []
    for blk in range(a.blocks + 1):          # block 0 warms up
        ms = {}
        for name, h in (("scaled", hs), ("prescaled", hp)):
            t = time.perf_counter()
            for _ in range(a.steps):
                h.step(False)
            ms[name] = (time.perf_counter() - t) * 1e3 / a.steps
        if blk > 0:
            blocks.append(ms)
        print(f"  block {blk} scaled {ms['scaled']:.4f} ms prescaled {ms['prescaled']:.4f} ms per iteration", file=sys.stderr, flush=True)
    ws, wp = (h.get_state(want_z=False, want_lam=False)["w"] for h in (hs, hp))
    same = bool(np.array_equal(ws.view(np.uint64), wp.view(np.uint64)))
    gram_route = hs.gram_route
    hs.close()
    hp.close()
    med = {name: {key: statistics.median(r[key] for r in rs) for key in ("upload_ms", "stats_ms", "form_ms")} for name, rs in ups.items()}
    ratios = [b["scaled"] / b["prescaled"] for b in blocks]
    print(json.dumps(dict(
        n=n, d=d, per_row=k, nnz=int(A.nnz), rounds=a.rounds, blocks=a.blocks, steps=a.steps, gram_route=gram_route,
        upload=dict(median=med, runs=ups, scale_over_none_upload_ms=med["scale"]["upload_ms"] / med["none"]["upload_ms"],
                    statistics_launches_ms=med["scale"]["stats_ms"],
                    scaling_launches_ms=med["scale"]["form_ms"] - med["none"]["form_ms"]),
        iteration=dict(blocks=blocks, scaled_over_prescaled=ratios, ratio_median=statistics.median(ratios),
                       ratio_min=min(ratios), ratio_max=max(ratios), iterates_bit_identical=same))))


def parse(cfg):
    shape, k = cfg.split("@")
    n, d = (int(v) for v in shape.split("x"))
    return n, d, int(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["1000000x1000@10", "1000000x200000@50"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_scale.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        a.n, a.d, a.k = parse(a.child)
        return child(a)
    records = {}
    if os.path.exists(a.out):
        records = {r["config"]: r for r in json.load(open(a.out))["records"]}
    for cfg in a.configs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--rounds", str(a.rounds), "--blocks", str(a.blocks),
               "--steps", str(a.steps)]
        print(cfg, file=sys.stderr, flush=True)
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"{cfg}: no result within {a.timeout} s - stopping here", file=sys.stderr)
            break
        if r.returncode != 0:
            print(f"{cfg}: exit status {r.returncode} - stopping here", file=sys.stderr)
            break
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        rec["config"] = cfg
        records[cfg] = rec
        u, it = rec["upload"], rec["iteration"]
        print(f"{cfg}: upload scale {u['median']['scale']['upload_ms']:.1f} ms / none {u['median']['none']['upload_ms']:.1f} ms = "
              f"{u['scale_over_none_upload_ms']:.3f}; statistics {u['statistics_launches_ms']:.3f} ms, scaling "
              f"{u['scaling_launches_ms']:.3f} ms; iteration scaled / prescaled {it['ratio_median']:.4f} "
              f"[{it['ratio_min']:.4f}, {it['ratio_max']:.4f}] at {statistics.median(b['scaled'] for b in it['blocks']):.3f} ms, "
              f"iterates bit-identical: {it['iterates_bit_identical']}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/csr_scale_bench.py", records=list(records.values())), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
