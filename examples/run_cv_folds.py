#!/usr/bin/env python3
"""K-fold cross-validation of a regularisation value on ONE upload: a fold is "the same rows with some of them switched
off", so the folds x values problems are members of one ``ADMMgroup`` with 0/1 ``sample_weight`` - one D = -y*X, one DTD,
and every ADMM iteration reads D once for several members in each of its two passes.  A held-out row (weight 0) leaves
the member's problem (its z follows m, its multiplier goes to 0); it is scored afterwards from the member's own
v = D w: the loss of row i is loss(v_i), and it is classified correctly when v_i < 0.

Held-out rows act as a proximal term on w while the ADMM runs, so a member needs somewhat more iterations than the same
problem on the training rows alone ("Row weights").

One CSV row per member (value, fold, iterations, held-out loss, held-out accuracy), then the mean per value and the
chosen one.

    python examples/run_cv_folds.py [--rows 6000] [--cols 500] [--folds 5] [--iters 200]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REGS = (0.1, 0.01, 0.001)


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
    ap.add_argument("--rows", type=int, default=600 if fast else 6000)
    ap.add_argument("--cols", type=int, default=150 if fast else 500)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40 if fast else 200)
    ap.add_argument("--seed", type=int, default=17)
    a = ap.parse_args()

    from admm_for_rank_based_loss_amd import ADMMgroup

    X, y = synthetic(a.rows, a.cols, a.seed)
    fold = np.random.default_rng(a.seed + 1).permutation(a.rows) % a.folds
    problems, tags = [], []
    for reg in REGS:
        for k in range(a.folds):
            problems.append(dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=reg,
                                 sample_weight=(fold != k).astype(np.float64)))
            tags.append((reg, k))
    grp = ADMMgroup(X, y, problems, max_iter=a.iters)
    ws = grp.main_loop(verbose=False)
    cnt = grp.counters()
    print(f"{len(problems)} members ({len(REGS)} values x {a.folds} folds), {cnt['shared_q']} + {cnt['shared_v']} shared "
          f"passes over D ({cnt['k_per_pass']} members per pass)")
    D = -y * X
    rows = [["l1_reg", "fold", "iterations", "heldout_loss", "heldout_acc"]]
    score = {reg: [] for reg in REGS}
    for (reg, k), it, w in zip(tags, grp.iterations, ws):
        v = (D @ np.asarray(w, dtype=np.float64).reshape(-1))[fold == k]       # the member's v on its held-out rows
        loss, acc = float(np.mean(np.logaddexp(0.0, v))), float(np.mean(v < 0.0))
        score[reg].append(loss)
        rows.append([reg, k, it, loss, acc])
    grp.close()
    for r in rows:
        print(",".join(str(x) for x in r))
    means = {reg: float(np.mean(v)) for reg, v in score.items()}
    best = min(means, key=means.get)
    for reg in REGS:
        print(f"mean,{reg},{means[reg]}")
    print(f"chosen,{best}")
    return rows, best


if __name__ == "__main__":
    main()
