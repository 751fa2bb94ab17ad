#!/usr/bin/env python3
"""Families of problems on ONE data set through ``ADMMgroup``: a superquantile-level sweep and a regularisation path,
as the reference's tables are built (one ``ADMMmethod`` per row there: run_SRM.py:39-42 in a loop over the levels /
the regularisers).  The data is uploaded once, D = -y*X and DTD are formed once, and every ADMM iteration reads D once
for several problems in each of its two passes.

One CSV row per problem: family, weight function, args, regulariser, iterations, final train loss, final test loss,
test accuracy.

    python examples/run_group.py [--rows 10000] [--cols 1000] [--iters 200] [--out rows.csv]
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n, d, seed):
    """two Gaussian classes, standardised columns, labels +-1 with 1 % flipped"""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    mu = rng.standard_normal(d) / np.sqrt(d)
    X = rng.standard_normal((n, d)) + 1.5 * y[:, None] * mu[None, :]
    X = (X - X.mean(axis=0)) / X.std(axis=0)
    flip = rng.random(n) < 0.01
    y[flip] = -y[flip]
    return X, y.reshape(-1, 1)


def main():
    fast = os.environ.get("RBL_EXAMPLE_FAST") == "1"
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=3000 if fast else 10000)
    ap.add_argument("--cols", type=int, default=200 if fast else 1000)
    ap.add_argument("--iters", type=int, default=30 if fast else 200)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from admm_for_rank_based_loss_amd import ADMMgroup
    from admm_for_rank_based_loss_amd.src.util.calculate_acc import calculate_accuracy

    X, y = synthetic(a.rows, a.cols, a.seed)
    ntr = int(0.6 * a.rows)
    X_train, y_train, X_test, y_test = X[:ntr], y[:ntr], X[ntr:], y[ntr:]

    families = {
        "superquantile_levels": [dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[q])
                                 for q in (0.1, 0.3, 0.5, 0.7, 0.9)],
        "l1_path": [dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=r)
                    for r in (0.1, 0.03, 0.01, 0.003)] +
                   [dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01, smooth=True, t=1)],
    }
    rows = [["family", "weight_function", "args", "reg", "iterations", "train_loss", "test_loss", "test_acc"]]
    for name, problems in families.items():
        grp = ADMMgroup(X_train, y_train, problems, max_iter=a.iters)
        grp.start_store(X_test, y_test)
        grp.main_loop(verbose=False)
        cnt = grp.counters()
        print(f"{name}: {len(problems)} problems, {cnt['shared_q']} + {cnt['shared_v']} shared passes over D "
              f"({cnt['k_per_pass']} problems per pass), {sum(cnt['single_passes'])} passes by single members")
        for pr, it, (w, times, train, test) in zip(problems, grp.iterations, grp.final_res()):
            acc = calculate_accuracy(w.reshape(-1, 1), X_test, y_test, threshold=0.5, loss=pr["loss"])
            reg = pr.get("l1_reg") or pr.get("l2_reg")
            rows.append([name, pr["weight_function"] + ("/smooth" if pr.get("smooth") else ""),
                         " ".join(str(x) for x in pr.get("args") or []), reg, it, train[-1], test[-1], acc])
        grp.close()
    for r in rows:
        print(",".join(str(x) for x in r))
    if a.out:
        with open(a.out, "w", newline="") as f:
            csv.writer(f).writerows(rows)
        print("rows written to", a.out)
    return rows


if __name__ == "__main__":
    main()
