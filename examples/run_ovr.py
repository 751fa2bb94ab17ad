#!/usr/bin/env python3
"""A 3-class problem as three one-vs-rest rank-based problems on ONE feature matrix through ``OneVsRest``: member k
has the labels +1 for class k and -1 for the rest (superquantile / binary cross entropy / l2, the reference's
run_SRM.py:39-42 once per class).  X is uploaded once, D and DTD are formed once - the Gram matrix does not depend on
+-1 labels - and every ADMM iteration reads D once for all three classes in each of its two passes.  The class of a
test row is the arg-max of x . w_k, taken on the GPU.

One CSV row per class (class, rows of the class, iterations, final train loss, final test loss, one-vs-rest test
accuracy), then the multi-class test accuracy.

    python examples/run_ovr.py [--rows 9000] [--cols 400] [--iters 200] [--out rows.csv] [--sparse]

``--sparse``: the same problem on a SciPy CSR matrix (70 % of the entries dropped) with ``storage="csr",
share_sparse=True``: D stays sparse on the device and the three classes share its multi-column sparse passes - the entries
are read once per pass for all three, with the iterates of three separate sparse solves bit for bit.
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n, d, n_class, seed):
    """n_class Gaussian blobs around random centres, standardised columns, 1 % of the class labels reassigned"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, n_class, size=n)
    centres = 3.0 * rng.standard_normal((n_class, d)) / np.sqrt(d)
    X = rng.standard_normal((n, d)) + centres[labels]
    X = (X - X.mean(axis=0)) / X.std(axis=0)
    noisy = rng.random(n) < 0.01
    labels[noisy] = rng.integers(0, n_class, size=int(noisy.sum()))
    return X, labels


def main():
    fast = os.environ.get("RBL_EXAMPLE_FAST") == "1"
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=3000 if fast else 9000)
    ap.add_argument("--cols", type=int, default=200 if fast else 400)
    ap.add_argument("--iters", type=int, default=30 if fast else 200)
    ap.add_argument("--level", type=float, default=0.5, help="superquantile level")
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sparse", action="store_true", help='a SciPy CSR matrix with storage="csr", share_sparse=True')
    a = ap.parse_args()

    from admm_for_rank_based_loss_amd import OneVsRest

    X, labels = synthetic(a.rows, a.cols, 3, a.seed)
    ntr = int(0.6 * a.rows)
    X_train, l_train, X_test, l_test = X[:ntr], labels[:ntr], X[ntr:], labels[ntr:]

    extra = {}
    if a.sparse:
        import scipy.sparse as sp
        keep = np.random.default_rng(a.seed + 1).random(X.shape) < 0.3
        X_train, X_test = sp.csr_matrix(X_train * keep[:ntr]), sp.csr_matrix(X_test * keep[ntr:])
        extra = dict(storage="csr", share_sparse=True)
    ovr = OneVsRest(X_train, l_train, weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01,
                    args=[a.level], max_iter=a.iters, **extra)
    ovr.group.start_store(X_test, [np.where(l_test == c, 1.0, -1.0) for c in ovr.classes_])
    W = ovr.main_loop(verbose=False)
    cnt = ovr.group.counters()
    print(f"{len(ovr.classes_)} classes, {cnt['shared_q']} + {cnt['shared_v']} shared passes over D "
          f"({cnt['k_per_pass']} problems per pass), {sum(cnt['single_passes'])} passes by single members")
    rows = [["class", "rows", "iterations", "train_loss", "test_loss", "ovr_test_acc"]]
    for k, (c, it, (w, times, train, test)) in enumerate(zip(ovr.classes_, ovr.group.iterations, ovr.group.final_res())):
        s = ovr.group.solvers[k]
        acc = s.test_objective._s.accuracy(W[:, k])      # member k's own test labels: class k against the rest
        rows.append([c, int(np.sum(l_train == c)), it, train[-1], test[-1], acc])
    for r in rows:
        print(",".join(str(x) for x in r))
    print("multi-class test accuracy:", ovr.accuracy(X_test, l_test))
    if a.out:
        with open(a.out, "w", newline="") as f:
            csv.writer(f).writerows(rows)
        print("rows written to", a.out)
    ovr.close()
    return rows


if __name__ == "__main__":
    main()
