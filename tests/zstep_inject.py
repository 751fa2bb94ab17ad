"""A prescribed m through a live z-step, and the exact answer to it (a helper, no tests; used by
test_zstep_inject_host.py on the CPU and test_gpu_zstep_inject.py on the device).

The injection.  For a rank-weighted handle with data, set_state(w = 0, lam = -rho * m0, rho, iter = k) followed by
phase_m gives v = D 0 = 0 (set_state clears the cached v) and m = v - lam / rho.  With rho a power of two the product
and the quotient are exact, so m has the values of m0 (a -0.0 in m0 comes out as +0.0: 0 - 0 = +0); `inject` reads m
back and the reference is built from what was read.  `iter` selects the path: iteration 0 always sorts 64-bit keys,
and the fast paths pause after a step they could not certify until `iter` passes their skip_until.

The reference.  Stable argsort of m, exact stack PAV on the sorted values (oracle/pav.py: pav_exact / ehrm_exact; the
squared hinge: tests/sqhinge_ref.py), scatter back.

The verdict.  What oracle/zband.py: z_step says about (family, loss, rho, m): OK (the banded structure holds: the
device's sort-free path is expected to certify), TIE (keys equal across a band edge - an exact integer property: the
device MUST redo with the sort), anything else (swallowed band, one-sided block, ...: no statement about the device).

The hub.  ShardedADMM (dist.py) with ranks as threads of one process and barrier-based collectives, for any engine: the
device synchronisation is a parameter, so the same driver runs librbl handles on one GPU and tests/_numpy_engine.py on
a CPU."""
import threading

import numpy as np

from oracle import admm, weights, zband

import sqhinge_ref

BAR = 1e-10                                   # test_gpu_kernels.py::test_pav_vs_oracle: "two exact algorithms"
RHOS = [2.0 ** -20, 2.0 ** -12, 2.0 ** -4, 1.0]
LOSSES = ["binary_cross_entropy", "hinge", "squared_hinge"]
NOT_CERTIFIED = -2                            # squared hinge: sqhinge_ref.zstep_banded gives no reason

# family -> (weight_function, args as a function of n, B)
FAMILIES = {
    "superq_0.5": ("superquantile", lambda n: [0.5], None),
    "superq_0.37": ("superquantile", lambda n: [0.37], None),
    "aorr_0.2_0.8": ("aorr", lambda n: [0.2, 0.8], None),
    "aorr_0.45_0.55": ("aorr", lambda n: [0.45, 0.55], None),
    "aorr_dc": ("aorr_dc", lambda n: [int(0.7 * n), int(0.1 * n)], None),
    "extremile": ("extremile", lambda n: [2.0], None),
    "esrm": ("esrm", lambda n: [1.0], None),
    "ehrm": ("ehrm", lambda n: None, -5.0),
}
BANDED = ["superq_0.5", "superq_0.37", "aorr_0.2_0.8", "aorr_0.45_0.55", "aorr_dc"]
SMOOTH = ["extremile", "esrm", "ehrm"]


def family(name, n):
    """-> (weight_function, args, B, sigma_a, sigma_b)"""
    wf, fa, B = FAMILIES[name]
    args = fa(n)
    sa, sb = weights.get_weights(wf, n, args)
    return wf, args, B, sa, sb


def losses_of(name):
    return ["binary_cross_entropy"] if name == "ehrm" else LOSSES


def edge_ranks(name, n):
    """(last rank of the first band, last rank of the last band but one); n // 2 for weights without bands"""
    sa = family(name, n)[3]
    starts, _ = zband.bands_of(sa)
    if name not in BANDED or starts.size < 3:
        return n // 2, n // 2
    return int(starts[1] - 1), int(starts[-2] - 1)


# ------------------------------------------------------------------------------------------------------- patterns
PATTERNS = ["gaussian", "sorted", "reversed", "wide", "all_equal", "two_values", "grid", "tight", "tie_1000", "tie_3000",
            "signed_zeros", "one_shard_large"]
BENIGN = ["gaussian", "sorted", "reversed", "wide"]
TIED = ["all_equal", "two_values", "grid", "tight"]


def pattern(name, n, seed=0, fam="superq_0.5", scale=1.0, shift=0.0):
    """the named n-vector; scale (a power of two) and shift are applied to the draws before ties are made, so tied
    entries stay tied"""
    rng = np.random.default_rng([seed, n, PATTERNS.index(name)])
    g = rng.standard_normal(n) * scale + shift
    if name == "gaussian":
        m = g
    elif name == "sorted":
        m = np.sort(g)
    elif name == "reversed":
        m = np.sort(g)[::-1]
    elif name == "wide":
        m = g * 10.0 ** rng.integers(-8, 8, n)
    elif name == "all_equal":
        m = np.full(n, 0.75 * scale + shift)
    elif name == "two_values":
        m = rng.choice(np.array([-0.5, 1.25]) * scale + shift, n)
    elif name == "grid":
        m = np.round(g, 2)
    elif name == "tight":
        m = (1.0 + 1e-13 * rng.standard_normal(n)) * scale + shift
    elif name in ("tie_1000", "tie_3000"):
        k = min(int(name[4:]), n)
        first, last = edge_ranks(fam, n)
        r = first if name == "tie_1000" else last
        order = np.argsort(g, kind="stable")
        lo = min(max(0, r - k // 2), n - k)
        m = g.copy()
        m[order[lo:lo + k]] = g[order[r]]          # k rows at the key of the band-edge rank r, ranks r and r + 1 among them
    elif name == "signed_zeros":
        m = np.zeros(n)
        m[1::2] = -0.0
    elif name == "one_shard_large":
        m = g.copy()
        m[(7 * n) // 8:] += 100.0 * scale           # the rows of the last shard (worlds 2, 3, 8) hold every large value
    else:
        raise KeyError(name)
    return np.ascontiguousarray(m, dtype=np.float64).copy()


def chunk_pattern(n, c, seed=0):
    """c rows drawn around -1.5 and n - c rows equal to 1.0, shuffled.  With c below n / world every splitter
    of the sample sort is 1.0, so the first c positions of the sorted order are the chunk of rank 0 and everything else
    lands on the last rank - c = 2047 / 2048 / 2049 puts the end of that chunk around the 2048-position tile of the
    chunk PAV"""
    rng = np.random.default_rng([seed, n, c])
    m = np.full(n, 1.0)
    m[:c] = -1.5 + 0.1 * rng.standard_normal(c)
    return rng.permutation(m)


# ------------------------------------------------------------------------------------------------------ reference
def exact_z(fam, loss, rho, m):
    m = np.ascontiguousarray(m, dtype=np.float64)
    wf, args, B, sa, sb = family(fam, m.size)
    if loss == "squared_hinge":
        return sqhinge_ref.z_step(wf, sa, rho, m)
    return admm.z_step_exact(wf, loss, sa, sb, B, rho, m)[0]


def value_error(z, zref):
    """max |z - z_exact| relative to max(1, max |z_exact|)"""
    return float(np.max(np.abs(z - zref), initial=0.0) / max(1.0, np.max(np.abs(zref), initial=0.0)))


def verdict(fam, loss, rho, m):
    """-> (status, z or None): zband.OK / zband.TIE / another status of oracle/zband.py (NOT_CERTIFIED for the squared
    hinge, whose restatement gives no reason)"""
    m = np.ascontiguousarray(m, dtype=np.float64)
    n = m.size
    wf, args, B, sa, sb = family(fam, n)
    if fam not in BANDED or n < 16:
        return zband.UNSUPPORTED, None
    if loss != "squared_hinge":
        z, st = zband.z_step(loss, sa, rho, m)
        return st, z
    starts, values = zband.bands_of(sa)
    if zband.clusters_of(starts, values) is None:
        return zband.UNSUPPORTED, None
    nb = values.size
    ranks = sorted({int(starts[j + 1] - 1) for j in range(nb - 1)} | {int(starts[j]) for j in range(1, nb)})
    part = np.partition(m, ranks)
    for r in ranks:
        if r + 1 in ranks and not part[r] < part[r + 1]:
            return zband.TIE, None
    order = np.argsort(m, kind="stable")
    out = sqhinge_ref.zstep_banded(sa, rho, m[order])
    if out is None:
        return NOT_CERTIFIED, None
    z = np.empty(n)
    z[order] = out[0]
    return zband.OK, z


# --------------------------------------------------------------------------------------------- single handle (GPU)
def make_problem(n, d=3, seed=1):
    rng = np.random.default_rng([seed, n, d])
    return rng.standard_normal((n, d)), np.where(rng.random(n) < 0.5, -1.0, 1.0)


def make_solver(R, fam, loss, n, d=3):
    """a single librbl handle with (any) data; the environment (RBL_NO_ZBAND, RBL_NO_SORT32, RBL_ZBAND_MIN_N) is read at
    its first z-step"""
    wf, args, B, _, _ = family(fam, n)
    X, y = make_problem(n, d)
    s = R.Solver(n, d, wf, loss, reg=0.01, wstep=2, args=args, B=B, tol=0.0, storage="f64")
    s.set_data(X, y)
    return s


def read_buffer(s, which):
    """a device buffer of the handle (Solver.buffer) on the host"""
    import torch
    from admm_for_rank_based_loss_amd.dist import _DevArray
    ptr, cnt = s.buffer(which)
    torch.cuda.synchronize()
    if cnt == 0:
        return np.zeros(0)
    return torch.as_tensor(_DevArray(ptr, cnt), device=torch.device("cuda", 0)).cpu().numpy().copy()


def inject(s, m0, rho, it, peek=False):
    """one iteration of the handle on the prescribed m -> dict(m read back, z after the iteration, zmid = z read right
    after the z-step if peek, mode = stats.zband, passes = stats.sort_passes, status = the banded path's status word,
    split = its pooled blocks whose value came from bracket-split sums)"""
    from admm_for_rank_based_loss_amd import _lib
    s.set_state(w=np.zeros(s.d), lam=-rho * m0, rho=rho, iter=it)
    s.phase_m()
    m = read_buffer(s, _lib.BUF_M)
    s.phase_z()
    zmid = s.get_state(want_lam=False)["z"].copy() if peek else None
    s.phase_q()
    s.phase_w()
    s.phase_dual(False)
    st = s.phase_finish()
    z = s.get_state(want_lam=False)["z"].copy()
    status, split = s.zband_status_split()
    return dict(m=m, z=z, zmid=zmid, mode=st.zband, passes=st.sort_passes, status=status, split=split)


# ----------------------------------------------------------------------------------------------- thread hub (any engine)
class Hub:
    def __init__(self, world):
        self.world = world
        self.bar = threading.Barrier(world)
        self.slot = [None] * world
        self.total = None


def make_thread_driver(ShardedADMM, hub, sync):
    """ShardedADMM with the collectives of `hub`; sync(): wait for the device (a no-op for a CPU engine).  The driver
    records which z-step ran (rec["banded"]: what _z_banded returned, None = not asked; rec["distributed"]) and the
    totals of the sample sort's count matrix (rec["totals"]: rows per chunk)."""
    import torch

    class ThreadSharded(ShardedADMM):
        rec = None

        def _exchange(self, item):
            hub.slot[self.rank] = item
            hub.bar.wait()
            items = list(hub.slot)
            hub.bar.wait()
            return items

        def _allreduce(self, t):
            if t.numel() == 0:
                return
            items = self._exchange(t)
            if self.rank == 0:
                tot = items[0].clone()
                for x in items[1:]:
                    tot += x               # fixed order: every rank gets the same bits
                hub.total = tot
            hub.bar.wait()
            t.copy_(hub.total)
            sync()
            hub.bar.wait()

        def _gather_small(self, t):
            out = torch.cat([x.reshape(-1) for x in self._exchange(t.clone())])
            sync()
            hub.bar.wait()
            return out

        def _gather_counts(self, counts_dev):
            sync()
            m = np.array([x.cpu().numpy() for x in self._exchange(counts_dev.clone())], dtype=np.int64)
            hub.bar.wait()
            m = m.reshape(self.world, self.world)
            if self.rec is not None and "totals" not in self.rec:
                self.rec["totals"] = m.sum(axis=0).tolist()
            return m

        def _alltoall(self, send, send_counts, recv, recv_counts):
            items = self._exchange((send, [int(c) for c in send_counts]))
            pos = 0
            for src, (buf, cnts) in enumerate(items):
                off = sum(cnts[: self.rank])
                c = cnts[self.rank]
                assert c == int(recv_counts[src])
                recv[pos:pos + c].copy_(buf[off:off + c])
                pos += c
            sync()
            hub.bar.wait()              # nobody overwrites a send buffer that is still being read

        def _allgather_rows(self, local):
            return torch.cat([x.reshape(-1) for x in self._exchange(local.clone())])

        def _z_banded(self):
            ok = super()._z_banded()
            self.rec["banded"] = bool(ok)
            return ok

        def _z_distributed(self):
            self.rec["distributed"] = True
            return super()._z_distributed()

    return ThreadSharded


class NumpyRank:
    """one rank of the CPU run: tests/_numpy_engine.py on its rows"""

    def __init__(self, fam, loss, n, world, rank, banded):
        from _numpy_engine import NumpyEngine
        from admm_for_rank_based_loss_amd.dist import shard_rows
        wf, args, B, _, _ = family(fam, n)
        X, y = make_problem(n)
        self.lo, self.cnt, _ = shard_rows(n, world, rank)
        sl = slice(self.lo, self.lo + self.cnt)
        self.engine = NumpyEngine(X[sl], y[sl], n, self.lo, wf, loss, 0.01, False, B=B, args=args, tol=0.0)
        self.sync = lambda: None

    def setup(self, drv):
        drv.setup_gram()

    def set(self, m0_local, rho, it):
        e = self.engine
        e.w, e.lam, e.rho, e.iter = np.zeros(e.d), -rho * m0_local, rho, it

    def z(self):
        return np.array(self.engine.z, dtype=np.float64).copy()

    def report(self, st, rec):
        pass


class GpuRank:
    """one rank of the device run: a librbl handle on its rows of a generated problem (all ranks on device 0)"""

    def __init__(self, fam, loss, n, world, rank, banded):
        import torch
        import admm_for_rank_based_loss_amd as rbl
        from admm_for_rank_based_loss_amd.dist import GpuEngine, shard_rows
        torch.cuda.set_device(0)
        wf, args, B, _, _ = family(fam, n)
        self.lo, self.cnt, _ = shard_rows(n, world, rank)
        self.s = rbl.Solver(self.cnt, 3, wf, loss, reg=0.01, wstep=2, B=B, args=args, n_total=n, row_offset=self.lo,
                            tol=0.0, storage="f64")
        self.engine = GpuEngine(self.s, 0)
        self.sync = torch.cuda.synchronize

    def setup(self, drv):
        drv.setup_synthetic(seed=12)
        drv.setup_gram()

    def set(self, m0_local, rho, it):
        self.s.set_state(w=np.zeros(3), lam=-rho * m0_local, rho=rho, iter=it)

    def z(self):
        return self.s.get_state(want_lam=False)["z"].copy()

    def report(self, st, rec):
        rec["mode"] = int(st.zband)
        rec["status"] = self.s.zband_status()


def run_ranks(rank_cls, fam, loss, n, world, banded, body, timeout=120, what="sharded z-step"):
    """`world` rank threads on the rows of one problem, each with its engine and a ShardedADMM on the hub's collectives
    (set up: data, Gram matrix); every thread runs body(rk, drv) -> [per rank: what body returned]"""
    from admm_for_rank_based_loss_amd.dist import ShardedADMM
    hub, out, errs = Hub(world), [None] * world, []

    def work(rank):
        try:
            rk = rank_cls(fam, loss, n, world, rank, banded)
            drv = make_thread_driver(ShardedADMM, hub, rk.sync)(rk.engine, world=world, rank=rank)
            drv.banded_z = bool(banded)
            rk.setup(drv)
            out[rank] = body(rk, drv)
        except BaseException as ex:              # a dead thread must not leave the others in a barrier forever
            errs.append((rank, repr(ex)))
            hub.bar.abort()

    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
    if any(t.is_alive() for t in ts):
        # ranks stuck in a collective or on the device keep their handles open: no further device work in this process
        import pytest
        pytest.exit(f"{what} hung: {fam} {loss} n={n} world={world} banded={banded} {errs}", returncode=1)
    real = [e for e in errs if "BrokenBarrierError" not in e[1]] or errs
    assert not errs, real
    assert all(o is not None for o in out)
    return out


def run_sharded(rank_cls, fam, loss, n, world, banded, injections, timeout=120):
    """injections: [(m0, rho, iter)].  Every rank thread runs all of them through ShardedADMM.step on its rows.
    -> [per injection: dict(m, z = concatenated, recs = [per rank: banded / distributed / totals / mode / status])]"""
    def body(rk, drv):
        e, res = rk.engine, []
        plain = e.phase_m
        seen = {}

        def phase_m():                       # m as the z-step is about to see it (the device path reuses the buffer)
            plain()
            rk.sync()
            seen["m"] = e.buf("m").cpu().numpy().copy()

        e.phase_m = phase_m
        for m0, rho, it in injections:
            rk.set(m0[rk.lo:rk.lo + rk.cnt], rho, it)
            drv.rec = dict(banded=None, distributed=False)
            st = drv.step(False)
            rk.report(st, drv.rec)
            res.append(dict(m=seen["m"], z=rk.z(), rec=drv.rec))
        return res

    out = run_ranks(rank_cls, fam, loss, n, world, banded, body, timeout)
    return [dict(m=np.concatenate([out[r][k]["m"] for r in range(world)]),
                 z=np.concatenate([out[r][k]["z"] for r in range(world)]),
                 recs=[out[r][k]["rec"] for r in range(world)]) for k in range(len(injections))]


def check_sharded(fam, loss, results, injections, banded, label=""):
    """value against the exact reference on the concatenated z, the same verdict / mode on every rank, TIE never
    certified.  -> [(oracle verdict, certified sort-free?)]"""
    out = []
    for (m0, rho, it), r in zip(injections, results):
        assert np.array_equal(r["m"], m0), (label, "m was not injected exactly")
        zref = exact_z(fam, loss, rho, r["m"])
        err = value_error(r["z"], zref)
        recs = r["recs"]
        first = {k: v for k, v in recs[0].items() if k != "totals"}
        for rec in recs[1:]:
            assert {k: v for k, v in rec.items() if k != "totals"} == first, (label, recs)
        st = verdict(fam, loss, rho, r["m"])[0] if banded else None
        print(f"{label} {fam} {loss[:6]} n={m0.size} rho=2^{int(np.log2(rho))} iter={it}: err={err:.2e} oracle={st} {first}"
              f" chunks={recs[0].get('totals')}")
        assert err <= BAR, (label, fam, loss, m0.size, rho, err, first)
        if not banded:
            assert first["banded"] is None and first["distributed"]
        elif first["banded"] is not None:
            assert first["distributed"] == (not first["banded"])
            if st == zband.TIE:
                assert first["banded"] is False, (label, "keys tied across a band edge were certified", first)
        out.append((st, first["banded"]))
    return out


# ------------------------------------------------------------------------------------------------------ case lists
def injections(fam, n, names, seed=0, it0=1000):
    """[(m0, rho, iter)]: names are pattern names or (name, rho, shift) triples; rho rotates over RHOS otherwise; iter
    advances by 100 per injection, past any pause (<= 64 iterations) an uncertified step leaves behind"""
    out = []
    for k, nm in enumerate(names):
        name, rho, shift = nm if isinstance(nm, tuple) else (nm, RHOS[(k + seed) % len(RHOS)], 0.0)
        if name.startswith("chunk_"):
            m0 = chunk_pattern(n, int(name[6:]), seed)
        else:
            m0 = pattern(name, n, seed, fam, shift=shift)
        out.append((m0, rho, it0 + 100 * k))
    return out


BCE, HINGE, SQ = LOSSES
CHUNK_N = 24000      # c <= 2049 rows are fewer than a rank's share at 8 ranks: they sit below the first splitter
EVERY = ["gaussian", "sorted", "reversed", "wide", "all_equal", "two_values", "grid", "tight", "tie_1000", "tie_3000",
         "signed_zeros", "one_shard_large"]
SMALL = ["gaussian", "sorted", "reversed", "wide", "two_values", "all_equal"]

# path 4 (sample sort, chunk PAV, seam searches): (family, loss, n, pattern names)
SHARDED_SORT = [
    ("extremile", BCE, 6000, EVERY[:4] + [("gaussian", 2.0 ** -20, 0.0)] + EVERY[4:]),    # gaussian at 2^-20: ONE block over all ranks
    ("ehrm", BCE, 4099, [("gaussian", 2.0 ** -12, 0.0), ("gaussian", 2.0 ** -4, -6.0), "two_values", "reversed"]),   # both branches
    ("superq_0.5", HINGE, CHUNK_N, ["chunk_2047", "chunk_2048", "chunk_2049", "all_equal", "gaussian"]),
    ("aorr_0.2_0.8", BCE, 1023, ["tie_1000", "gaussian", "two_values", "reversed"]),
    ("esrm", HINGE, 5, ["gaussian", "all_equal", "reversed"]),                                    # n < world at 8 ranks
    ("aorr_dc", SQ, 4096, ["gaussian", "reversed", "two_values", "grid"]),
]
# path 5 (sort-free, sharded): every size meets it
SHARDED_BANDED = [
    ("superq_0.5", BCE, 16, SMALL), ("superq_0.37", HINGE, 17, SMALL), ("aorr_0.2_0.8", BCE, 18, SMALL),
    ("aorr_dc", HINGE, 19, SMALL), ("aorr_0.45_0.55", BCE, 1023, SMALL + ["grid", "tight"]),
    ("superq_0.37", BCE, 4096, SMALL + ["tie_1000"]), ("aorr_0.2_0.8", HINGE, 4099, SMALL + ["tie_1000", "tie_3000"]),
    ("superq_0.5", HINGE, 6000, EVERY), ("aorr_dc", BCE, 70001, ["gaussian", "reversed", "tie_3000"]),
    ("aorr_0.2_0.8", SQ, 6000, EVERY),
]


def check_chunks(names, results, n, world):
    """what the sample sort did with the designed inputs (rows per chunk, rec["totals"])"""
    for nm, r in zip(names, results):
        tot = r["recs"][0].get("totals")
        if tot is None:
            continue
        assert sum(tot) == n
        if isinstance(nm, str) and nm.startswith("chunk_"):
            assert int(nm[6:]) in tot, (nm, tot)                       # that many rows landed on one rank
        if nm == "all_equal":
            assert sorted(tot)[:-1] == [0] * (world - 1), tot          # one chunk holds every row
        if nm == "two_values" and world == 8 and n >= 64:
            k = [i for i, t in enumerate(tot) if t]
            assert len(k) == 2 and k[1] - k[0] > 1, tot                # empty chunks between non-empty ones


# single handle.  Paths 1 and 2 (64-bit sort; 32-bit keys, fix-up, redo): every family, loss and pattern
SINGLE_SORT = [
    ("extremile", BCE, 6000, EVERY), ("esrm", HINGE, 4099, EVERY), ("aorr_0.2_0.8", SQ, 6000, EVERY),
    ("ehrm", BCE, 4099, [("gaussian", 2.0 ** -12, 0.0), ("gaussian", 2.0 ** -4, -6.0)] + TIED),
    ("superq_0.5", HINGE, 1023, SMALL), ("aorr_dc", BCE, 4096, SMALL), ("superq_0.37", SQ, 17, SMALL),
    ("aorr_0.45_0.55", HINGE, 70001, ["gaussian", "tie_3000"]), ("esrm", SQ, 1023, SMALL), ("extremile", HINGE, 19, SMALL),
]
# path 3 (sort-free): every banded family with every loss; every pattern at n = 6000; every size
SIZES_SMALL, SIZES_LARGE = [16, 17, 18, 19], [1023, 4096, 4099, 70001]
SINGLE_BANDED = []
for _i, _fam in enumerate(BANDED):
    for _j, _loss in enumerate(LOSSES):
        SINGLE_BANDED.append((_fam, _loss, 6000, EVERY))
        for _n in SIZES_SMALL:
            SINGLE_BANDED.append((_fam, _loss, _n, ["gaussian", "reversed", "two_values"]))
        for _k in range(2):
            _n = SIZES_LARGE[(_i + _j + 2 * _k) % 4]
            SINGLE_BANDED.append((_fam, _loss, _n, ["gaussian", "sorted", "wide", "tie_1000", "grid"]))
