#!/usr/bin/env python3
"""Timings of the sparse data path (include/rbl.h: rbl_set_data_csr) against the dense float32 host source -> one JSON
document.

    python tools/upload_csr.py [--n 1000000] [--d 1000] [--densities 0.01,0.1,0.5] [--out profiles/csr_upload.json]

One matrix per density (float32 values, int32 indices, fp32 storage), each density in a fresh child process under its
own time limit.  Three sources of the SAME matrix, interleaved, medians of 3 runs after one warm-up round:

  csr_host     the CSR arrays in host memory: only indptr, indices and values cross PCIe
  csr_device   the CSR arrays already on the GPU: nothing crosses but the 4 (n + 1) bytes of indptr the checks read
  dense_host   the dense float32 host array through rbl_set_data_from - the yardstick

For each, with scaling "none" and "fit": the wall time of set_data (pinning and synchronisation included), the passes as
the library times them (rbl_kernel_time RBL_KERNEL_SRC_STATS / RBL_KERNEL_SRC_FORM: events on the handle's stream, the
copies a host source waits for included) and the bytes that crossed PCIe, counted from the shapes.  The byte ratio
csr_host / dense_host is density * (4 + 4) / 4 (+ indptr)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 3


def _med(v):
    return float(statistics.median(v))


def _matrix(n, d, density, seed=0):
    """(indptr int32, indices int32, values float32, dense float32) of one random matrix, built in row blocks"""
    import numpy as np
    rng = np.random.default_rng(seed)
    dense = np.zeros((n, d), dtype=np.float32)
    counts = np.zeros(n + 1, dtype=np.int64)
    idx, val = [], []
    for r0 in range(0, n, 50_000):
        rows = min(50_000, n - r0)
        mask = rng.random((rows, d), dtype=np.float32) < density
        r, c = np.nonzero(mask)                          # row-major: sorted columns inside every row
        v = rng.standard_normal(r.shape[0], dtype=np.float32)
        v[v == 0.0] = 1.0
        dense[r0 + r, c] = v
        counts[r0 + 1:r0 + rows + 1] = mask.sum(axis=1)
        idx.append(c.astype(np.int32))
        val.append(v)
    indptr = np.cumsum(counts)
    assert indptr[-1] < 2 ** 31
    return indptr.astype(np.int32), np.concatenate(idx), np.concatenate(val), dense


def step(n, d, density):
    import numpy as np
    import torch
    import admm_for_rank_based_loss_amd as rbl
    L = rbl._lib
    indptr, indices, values, dense = _matrix(n, d, density)
    nnz = int(values.shape[0])
    y = np.where(np.random.default_rng(1).random(n) < 0.5, 1.0, -1.0)
    dev = [torch.from_numpy(a).cuda() for a in (indptr, indices, values)]
    torch.cuda.synchronize()

    def csr(mem, arrays):
        ptrs = [a.data_ptr() if mem == L.MEM_DEVICE else a.ctypes.data for a in arrays]
        return rbl._solver.CsrSource((n, d), L.DTYPE_F32, mem, L.INDEX_I32, nnz, ptrs[0], ptrs[1], ptrs[2], arrays)

    sources = dict(csr_host=csr(L.MEM_HOST, [indptr, indices, values]), csr_device=csr(L.MEM_DEVICE, dev), dense_host=dense)
    once = dict(csr_host=4 * (n + 1) + 8 * nnz, csr_device=0, dense_host=4 * n * d)       # bytes over PCIe per pass
    s = rbl.Solver(n, d, "erm", storage="f32", objective_only=True)
    res = dict(n=n, d=d, density=density, nnz=nnz, values="float32", indices="int32", storage="f32", reps=REPS,
               byte_ratio_csr_over_dense=once["csr_host"] / once["dense_host"])
    D_ref = {}
    for scaling in ("none", "fit"):
        t = {k: dict(wall=[], form=[], stats=[]) for k in sources}
        for rep in range(REPS + 1):                      # (the first round warms every variant up)
            for name, src in sources.items():
                s.set_scaling(None, None)
                t0 = time.perf_counter()
                s.set_data(src, y, scaling=scaling)      # (returns with the stream idle)
                wall = (time.perf_counter() - t0) * 1e3
                if rep:
                    t[name]["wall"].append(wall)
                    t[name]["form"].append(s.kernel_time(L.KERNEL_SRC_FORM)[0])
                    t[name]["stats"].append(s.kernel_time(L.KERNEL_SRC_STATS)[0])
                elif n * d <= 50_000_000:                # at small sizes: the three routes form the same matrix
                    D = s.get_D()
                    assert np.array_equal(D_ref.setdefault(scaling, D), D), (name, scaling)
        passes = 2 if scaling == "fit" else 1
        for name in sources:
            r = dict(set_data_wall_ms=_med(t[name]["wall"]), form_pass_ms=_med(t[name]["form"]),
                     bytes_over_pcie=passes * once[name] + (4 * (n + 1) if name == "csr_device" else 0),
                     set_data_wall_ms_all=t[name]["wall"])
            if scaling == "fit":
                r["stats_pass_ms"] = _med(t[name]["stats"])
            res.setdefault(name, {})[scaling] = r
        res.setdefault("csr_host_over_dense_host_wall", {})[scaling] = \
            res["csr_host"][scaling]["set_data_wall_ms"] / res["dense_host"][scaling]["set_data_wall_ms"]
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1000)
    ap.add_argument("--densities", default="0.01,0.1,0.5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_upload.json"))
    ap.add_argument("--step", type=float, default=None)
    ap.add_argument("--limit", type=int, default=420, help="time limit of one density in seconds")
    a = ap.parse_args()
    if a.step is not None:
        print("RESULT " + json.dumps(step(a.n, a.d, a.step)))
        return 0
    doc = {}
    for dens in a.densities.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", dens, "--n", str(a.n),
               "--d", str(a.d)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(f"density {dens}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1                                     # nothing more is started after a step that failed
        doc[f"density_{dens}"] = json.loads(lines[-1][7:])
        print(dens, json.dumps(doc[f"density_{dens}"]))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
