"""Upper levels of the merge-tree PAV (csrc/pav.hip: the levels whose segments are longer than the 2048-position tile).

They run either in one persistent launch (k_pav_upper: device-wide barriers, a dirty-level mask, merging waves that
write pooled ranges of up to PU_DIRECT_FILL = 8192 positions themselves and a list of longer "long fills" that all
blocks write together) or in two launches per level (k_pav_seam_wave + k_pav_fill).  rbl_k_pav_seq runs both in one
process, keeps the workspace - seam hints, barrier parity, EHRM speculated branch - from one call to the next as a
solver handle does between z-steps, and returns the persistent kernel's counters, so every case here can say which
path and which fill schedule it exercised.

Every result is compared with the oracle's exact stack PAV (oracle.pav.pav_exact / ehrm_exact) or a closed form.
The piecewise-constant schedules below are built so that every block of the answer is known in advance; the tests
without the gpu mark check those claims on the CPU.
"""
import math

import numpy as np
import pytest

TILE = 2048          # PB_TILE: segments up to this size are solved inside k_pav_bottom
DIRECT = 8192        # PU_DIRECT_FILL: longer pooled ranges go to the long-fill list
OLD_CAP = 4096       # the long-fill list's fixed capacity before it was sized by n
PATHS = ("persist", "two_launch")
BCE, HINGE = "binary_cross_entropy", "hinge"
FAMILIES = [("superquantile", [0.5]), ("extremile", [2.0]), ("esrm", [1.0]), ("aorr", [0.2, 0.8]),
            ("aorr_dc", [80, 3]), ("erm", None)]
SIZES = [2049, 4097, 8193, 16385, 2 ** 17 + 1, 2 ** 20 + 3, 2 ** 22 + 12345, 6_250_000]


@pytest.fixture(scope="module")
def L():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    return rbl._lib


def _bar(ref):
    return 1e-9 * max(1.0, float(np.max(np.abs(ref))))


def _check_counters(path, cnt, ref):
    """status 0; the two-launch path leaves the persistent kernel's counters at 0; an answer with a block across a
    tile boundary (every multiple of 2048 is an upper seam) needs an upper level with a violating seam.  (Equal
    values are one block on tie-free m, except where the hinge prox clips at -1.)"""
    assert cnt[3] == 0
    if path == "two_launch":
        assert cnt[1] == 0 and cnt[2] == 0
    else:
        p = np.arange(TILE, ref.size, TILE)
        if np.any((ref[p - 1] == ref[p]) & (ref[p] != -1.0)):
            assert cnt[1] != 0


def _nlevels(n):
    lv, half = 0, TILE
    while half < n:
        lv, half = lv + 1, half * 2
    return lv


# ------------------------------------------------------------------ piecewise-constant schedules
# A schedule is a list of pieces (kind, length): "run" = constant m with sigma strictly increasing (the element values
# strictly decrease, so the run pools into ONE block), "free" = strictly increasing m with a constant sigma (every
# position its own block).  Piece j sits at level j * GAP and its values stay within (j GAP - 0.5, j GAP + 0.5) for
# rho = RHO (sigma <= 0.5), so no two pieces ever pool together, in the answer or in any segment of the tree.
GAP, RHO = 1.0, 1.0


def make_schedule(pieces):
    n = sum(ln for _, ln in pieces)
    sigma, m = np.empty(n), np.empty(n)
    starts, pooled = [], []
    o = 0
    for j, (kind, ln) in enumerate(pieces):
        c = j * GAP
        if kind == "run":
            m[o:o + ln] = c
            sigma[o:o + ln] = np.linspace(0.05, 0.5, ln) if ln > 1 else 0.05
        else:
            m[o:o + ln] = c + np.linspace(0.0, 0.45, ln)
            sigma[o:o + ln] = 0.05
        starts.append(o)
        pooled.append(kind == "run")
        o += ln
    return sigma, m, np.array(starts + [n], dtype=np.int64), np.array(pooled)


def expected_upper(n, starts, pooled):
    """What k_pav_upper does on a schedule, level by level.  The tree's state after level l is the isotonic solution
    of every segment, i.e. every piece cut to the segment; a seam violates iff a run straddles it, and then pools
    exactly that run cut to [L0, R1).  Returns (dirty mask, total long fills, per-level list of
    (violating seams, direct fills, long fills))."""
    mask, levels = 0, []
    for lv in range(_nlevels(n)):
        half = TILE << lv
        p = np.arange(half, n, 2 * half, dtype=np.int64)            # seams of this level
        jl = np.searchsorted(starts, p - 1, side="right") - 1       # piece of position p - 1
        jr = np.searchsorted(starts, p, side="right") - 1           # piece of position p
        viol = (jl == jr) & pooled[jr]
        p, j = p[viol], jr[viol]
        L0, R1 = p - half, np.minimum(p + half, n)
        s = np.maximum(starts[j], L0)
        e = np.minimum(starts[j + 1], R1) - 1
        long_ = (e - s + 1) > DIRECT
        if p.size:
            mask |= 1 << lv
        # a pooled range that reaches an end of its segment marks the level whose seam sits there
        for pos in np.concatenate((L0[(s == L0) & (L0 > 0)], R1[(e == R1 - 1) & (R1 < n)])):
            mask |= 1 << ((int(pos) // TILE) & -(int(pos) // TILE)).bit_length() - 1
        levels.append((int(p.size), int(np.count_nonzero(~long_)), int(np.count_nonzero(long_))))
    return mask, sum(lv[2] for lv in levels), levels


def simulate_upper(loss, sigma, rho, m):
    """The same prediction from the definition, for any input: before level l every segment of half positions holds its
    own isotonic solution (oracle stack PAV), after it every segment of 2 half; a seam violates iff the value drops
    across it before the level, and it pools the block of the merged segment's solution that contains it."""
    from oracle import pav

    def solved(size):
        out = np.empty_like(m)
        for a in range(0, n, size):
            out[a:a + size], _ = pav.pav_exact(loss, sigma[a:a + size], rho, m[a:a + size])
        return out

    n = m.size
    mask, levels = 0, []
    before = solved(TILE)
    for lv in range(_nlevels(n)):
        half = TILE << lv
        after = solved(2 * half)
        viol = direct = long_ = 0
        for p in range(half, n, 2 * half):
            if not before[p - 1] > before[p]:
                continue
            viol += 1
            mask |= 1 << lv
            L0, R1 = p - half, min(p + half, n)
            s = p
            while s > L0 and after[s - 1] == after[p]:
                s -= 1
            e = p
            while e < R1 - 1 and after[e + 1] == after[p]:
                e += 1
            if e - s + 1 > DIRECT:
                long_ += 1
            else:
                direct += 1
            for pos in ([L0] if s == L0 and L0 > 0 else []) + ([R1] if e == R1 - 1 and R1 < n else []):
                q = pos // TILE
                mask |= 1 << ((q & -q).bit_length() - 1)
        levels.append((viol, direct, long_))
        before = after
    return mask, sum(lv[2] for lv in levels), levels


def _periodic(period, layout, n_periods, tail=5):
    pieces = []
    for k in range(n_periods):
        for kind, ln in layout(k):
            if ln > 0:
                pieces.append((kind, ln))
    pieces.append(("free", tail))
    # merge neighbouring free pieces (one strictly increasing stretch)
    out = []
    for kind, ln in pieces:
        if out and kind == "free" and out[-1][0] == "free":
            out[-1] = ("free", out[-1][1] + ln)
        else:
            out.append((kind, ln))
    return out


def schedule(name):
    if name == "a_all_equal":
        # one run over everything: levels 0-1 pool 4096 / 8192 positions (direct fills), every higher level long ones
        return [("run", 2 ** 20 + 3)]
    if name == "b_skipped_level":
        # per 65536 positions one run [17384, 48152): level 2 pools the two halves (15384 positions each, long), the run
        # touches no level-3 seam and no pooled range ends on one (level 3 is skipped), level 4 pools the run (long)
        return _periodic(65536, lambda k: [("free", 17384), ("run", 30768), ("free", 65536 - 48152)], 4)
    if name == "c_mixed_level":
        # level-2 segments alternate: a run of 8000 around the seam (direct fill) / one of 16200 (long fill)
        def lay(k):
            if k % 2 == 0:
                return [("free", 4000), ("run", 8000), ("free", 4384)]
            return [("free", 100), ("run", 16200), ("free", 84)]
        return _periodic(16384, lay, 12)
    if name == "d_top_only":
        # n = 2^20 + 777: the top seam sits at 2^20; the only run straddling it is 8192 + 777 long, everything below
        # it pools at most 8192 positions
        top = 2 ** 20
        return [("free", top - 8192 - 3000), ("run", 3000), ("run", 8192 + 777)]
    if name == "e_straddle":
        # run lengths around 8192 and the segment sizes, placed across segment boundaries
        rng = np.random.default_rng(77)
        lens = [8191, 8192, 8193, 16383, 16384, 16385, 2047, 2049, 4095, 4097, 30001, 65537]
        pieces, n = [], 0
        while n < 2 ** 19:
            ln = int(lens[rng.integers(len(lens))])
            kind = "run" if rng.random() < 0.7 else "free"
            if pieces and kind == "free" and pieces[-1][0] == "free":
                kind = "run"
            pieces.append((kind, ln))
            n += ln
        return pieces
    raise KeyError(name)


SCHEDULES = ["a_all_equal", "b_skipped_level", "c_mixed_level", "d_top_only", "e_straddle"]


def _claims(name, n, levels, mask):
    """the property each schedule was built for"""
    nl = len(levels)
    if name == "a_all_equal":
        assert all(lv[2] == 0 and lv[0] > 0 for lv in levels[:2])
        assert all(lv[2] > 0 for lv in levels[2:])
        assert mask == (1 << nl) - 1
    elif name == "b_skipped_level":
        assert levels[2][2] > 0 and levels[3][0] == 0 and levels[4][2] > 0
        assert not (mask >> 3) & 1 and (mask >> 4) & 1
    elif name == "c_mixed_level":
        assert levels[2][1] > 0 and levels[2][2] > 0
    elif name == "d_top_only":
        assert levels[-1][2] == 1 and all(lv[2] == 0 for lv in levels[:-1])
        assert any(not (mask >> lv) & 1 for lv in range(nl))     # and some levels are skipped on the way
    elif name == "e_straddle":
        assert sum(lv[1] for lv in levels) > 0 and sum(lv[2] for lv in levels) > 0


@pytest.mark.parametrize("name", SCHEDULES)
def test_schedule_fixtures_are_what_they_claim(name):
    """CPU: the oracle's exact PAV pools every run into one block and nothing else, and the predicted upper-level
    schedule has the property the fixture was built for."""
    from oracle import pav
    sigma, m, starts, pooled = make_schedule(schedule(name))
    n = m.size
    for loss in (BCE, HINGE):
        u, nb = pav.pav_exact(loss, sigma, RHO, m)
        lens = np.diff(starts)
        assert nb == int(np.sum(np.where(pooled, 1, lens)))
        for j in np.flatnonzero(pooled):
            blk = u[starts[j]:starts[j + 1]]
            assert np.all(blk == blk[0])
            assert abs(blk[0] - j * GAP) < 0.5
        assert np.all(np.diff(u) >= 0)
    mask, nlong, levels = expected_upper(n, starts, pooled)
    _claims(name, n, levels, mask)
    # the shortcut prediction (runs cut to segments) is the tree's behaviour from its definition
    assert simulate_upper(HINGE, sigma, RHO, m) == (mask, nlong, levels)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCHEDULES)
def test_long_fill_schedules(L, name):
    """Both paths on the constructed schedules; the persistent kernel's dirty mask and long-fill count are the
    predicted ones, the two paths agree bit for bit, and both match the oracle."""
    from oracle import pav
    sigma, m, starts, pooled = make_schedule(schedule(name))
    n = m.size
    mask, nlong, levels = expected_upper(n, starts, pooled)
    for loss in (BCE, HINGE):
        ref, _ = pav.pav_exact(loss, sigma, RHO, m)
        u = {}
        for path in PATHS:
            out, _, cnt = L.k_pav_seq(loss, sigma, RHO, m[None, :], path)
            u[path] = out[0]
            assert np.max(np.abs(out[0] - ref)) <= _bar(ref), (name, loss, path)
            assert cnt[0, 3] == 0
            if path == "persist":
                assert int(cnt[0, 1]) == mask, (name, loss, bin(int(cnt[0, 1])), bin(mask))
                assert int(cnt[0, 2]) == nlong, (name, loss, int(cnt[0, 2]), nlong)
            else:
                assert cnt[0, 1] == 0 and cnt[0, 2] == 0
        assert np.array_equal(u["persist"], u["two_launch"]), name


# ------------------------------------------------------------------ both paths, many levels
def _tie_free_m(rng, n, scale, shift):
    m = np.sort(rng.standard_normal(n) * scale + shift)
    assert np.all(np.diff(m) > 0)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_both_paths_every_family(L, n):
    """Every family and both losses (EHRM: BCE, automatic branch) on both upper paths against the oracle; on these
    tie-free inputs the two paths agree bit for bit.  The two largest sizes give k_pav_upper one block per CU."""
    from oracle import pav, weights
    rng = np.random.default_rng(1000 + n)
    rhos = (2e-7, 1e-5, 1e-3)
    for fi, (fam, args) in enumerate(FAMILIES + [("ehrm", None)]):
        sa, sb = weights.get_weights(fam, n, args)
        for li, loss in enumerate((BCE, HINGE)):
            rho = rhos[(fi + li) % len(rhos)]
            m = _tie_free_m(rng, n, 2.0, -0.5)
            sg = sb if li else sa
            ref, _ = pav.pav_exact(loss, sg, rho, m)
            outs = []
            for path in PATHS:
                u, _, cnt = L.k_pav_seq(loss, sg, rho, m[None, :], path)
                _check_counters(path, cnt[0], ref)
                assert np.max(np.abs(u[0] - ref)) <= _bar(ref), (n, fam, loss, path)
                outs.append(u[0])
            assert np.array_equal(outs[0], outs[1]), (n, fam, loss)
        if fam == "ehrm":
            m = _tie_free_m(rng, n, 2.0, 0.0)
            zo, bo = pav.ehrm_exact(sa, sb, -5.0, 1e-4, m)
            outs = []
            for path in PATHS:
                z, br, cnt = L.k_pav_seq(BCE, sa, 1e-4, m[None, :], path, sigma_b=sb, B=-5.0)
                assert cnt[0, 3] == 0 and br[0] == (0 if bo == "a" else 1), (n, path)
                assert np.max(np.abs(z[0] - zo)) <= _bar(zo), (n, path)
                outs.append(z[0])
            assert np.array_equal(outs[0], outs[1]), n


# ------------------------------------------------------------------ warm hints
def _check_seq(L, loss, sigma, rho, ms, sigma_b=None, B=0.0, tie_free=True):
    """runs the sequence on both paths; every call against the oracle; returns the persistent path's outputs"""
    from oracle import pav
    refs = []
    for k in range(ms.shape[0]):
        if sigma_b is None:
            refs.append((pav.pav_exact(loss, sigma, rho, ms[k])[0], -1))
        else:
            ref, bo = pav.ehrm_exact(sigma, sigma_b, B, rho, ms[k])
            refs.append((ref, 0 if bo == "a" else 1))
    res = {}
    for path in PATHS:
        u, br, cnt = L.k_pav_seq(loss, sigma, rho, ms, path, sigma_b=sigma_b, B=B)
        for k, (ref, bref) in enumerate(refs):
            if sigma_b is None:
                _check_counters(path, cnt[k], ref)
            assert cnt[k, 3] == 0 and br[k] == bref, (path, k)
            assert np.max(np.abs(u[k] - ref)) <= _bar(ref), (path, k)
        res[path] = (u, br, cnt)
    if tie_free:
        # the same hints on both paths: the same searches, the same answer
        assert np.array_equal(res["persist"][0], res["two_launch"][0])
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("loss", [BCE, HINGE])
def test_warm_hints_perturbed_same_unrelated(L, loss):
    """m, then m + small noise (re-sorted: the solver's situation), then the same m again, then an unrelated m, then
    the first m again: each call on the workspace the previous ones left."""
    from oracle import weights
    rng = np.random.default_rng(5)
    for n, fam, args, rho in ((2 ** 20 + 3, "extremile", [2.0], 1e-5), (300_001, "superquantile", [0.5], 1e-4),
                              (2 ** 17 + 1, "esrm", [1.0], 2e-7)):
        sa, _ = weights.get_weights(fam, n, args)
        m0 = _tie_free_m(rng, n, 2.0, -0.5)
        m1 = np.sort(m0 + 1e-3 * rng.standard_normal(n))
        assert np.all(np.diff(m1) > 0)
        m3 = _tie_free_m(rng, n, 7.0, 3.0)           # unrelated: hints far off, values outside the old brackets
        ms = np.stack([m0, m1, m1, m3, m0])
        res = _check_seq(L, loss, sa, rho, ms)
        for path in PATHS:
            u, _, cnt = res[path]
            assert np.array_equal(u[2], u[1]), path   # warm (hints from the same m) == the call that set them
        # ... and == a cold call on a fresh workspace
        cold, _, _ = L.k_pav_seq(loss, sa, rho, m1[None, :], "persist")
        assert np.array_equal(res["persist"][0][2], cold[0])
        cold, _, _ = L.k_pav_seq(loss, sa, rho, m0[None, :], "two_launch")
        assert np.array_equal(res["two_launch"][0][4], cold[0])


def _banded_sigma(n, period, c):
    """zero weight on the first half of every period, c on the second: every zero -> c boundary pools a block that
    reaches back into the zero-weight positions (where the element value is m itself)"""
    s = np.zeros(n)
    pos = np.arange(n) % period
    s[pos >= period // 2] = c
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("loss", [BCE, HINGE])
def test_warm_hints_ties_at_previous_pooled_value(L, loss):
    """The second m has runs of values EXACTLY equal to the values the first call pooled, in the zero-weight
    positions where a block starts (there the element value is m itself): the searches of the next call start at a
    value (the hint) that the new data holds many times."""
    rng = np.random.default_rng(9)
    n, period = 2 ** 20 + 3, 16384
    sigma = _banded_sigma(n, period, 0.02)
    for rho in (1.0, 0.25):
        m0 = _tie_free_m(rng, n, 1.0, 0.0)
        u0, _, _ = L.k_pav_seq(loss, sigma, rho, m0[None, :], "persist")
        u0 = u0[0]
        # the pooled values (blocks of >= 2 positions) and the zero-weight positions whose m lies just below them
        starts = np.flatnonzero(np.concatenate(([True], u0[1:] != u0[:-1])))
        lens = np.diff(np.append(starts, n))
        vals = u0[starts[lens >= 2]]
        assert vals.size >= 20
        m1 = m0.copy()
        zero = sigma == 0.0
        for x in vals:
            i = int(np.searchsorted(m1, x))
            lo = max(0, i - 40)
            sel = np.arange(lo, min(n, i + 40))
            sel = sel[zero[sel]]
            m1[sel] = x
        m1 = np.maximum.accumulate(m1)   # (sorted again where a tie run overran its neighbours)
        assert np.count_nonzero(np.isin(m1, vals)) >= 10 * vals.size
        _check_seq(L, loss, sigma, rho, np.stack([m0, m1, m1, m0]), tie_free=False)


@pytest.mark.gpu
def test_warm_hints_ehrm_branch_flips(L):
    """EHRM sequences on one workspace: the branch speculated for each call is the previous call's, and it is wrong
    whenever the branch flips (b -> a -> a -> b -> a), so the fall-back tree runs on a warm workspace."""
    from oracle import pav, weights
    rng = np.random.default_rng(13)
    B = -5.0
    for n, rho in ((2 ** 20 + 3, 1e-4), (16385, 1e-3)):
        sa, sb = weights.get_weights("ehrm", n)
        ms = np.stack([_tie_free_m(rng, n, 2.0, sh) for sh in (0.0, -12.0, -11.0, 1.0, -12.0)])
        want = [pav.ehrm_branch_exact(sa, sb, B, rho, ms[k]) for k in range(ms.shape[0])]
        assert want == ["b", "a", "a", "b", "a"], want       # the sequence flips as intended
        res = _check_seq(L, BCE, sa, rho, ms, sigma_b=sb, B=B)
        assert list(res["persist"][1]) == [1, 0, 0, 1, 0]


# ------------------------------------------------------------------ capacity of the long-fill list
CAP_N = 2 ** 25 + 2 ** 20


@pytest.mark.gpu
@pytest.mark.parametrize("loss", [BCE, HINGE])
def test_long_fill_list_capacity(L, loss):
    """All m equal and sigma increasing - the first z-step of extremile / esrm from w = 0 - at 2^25 + 2^20 positions:
    every seam pools, and the levels from 2 up need more long fills than the list's old fixed 4096 entries.  The
    answer is one block, in closed form."""
    from oracle import pav
    n = CAP_N
    sigma = np.linspace(0.0, 1.0, n)
    m = np.full(n, 0.25)
    rho = 1.0
    x = pav.block_value(loss, math.fsum(sigma), math.fsum(m), n, rho)
    _, nlong, _ = expected_upper(n, np.array([0, n], dtype=np.int64), np.array([True]))
    assert nlong > OLD_CAP
    for path in PATHS:
        u, _, cnt = L.k_pav_seq(loss, sigma, rho, m[None, :], path)
        assert cnt[0, 3] == 0
        if path == "persist":
            assert int(cnt[0, 2]) == nlong and int(cnt[0, 2]) > OLD_CAP, int(cnt[0, 2])
        assert np.ptp(u[0]) == 0.0
        assert abs(u[0][0] - x) <= 1e-9 * max(1.0, abs(x)), (path, u[0][0], x)
        del u


@pytest.mark.gpu
def test_solver_capacity_all_rows_pool(L):
    """The same size through the solver: extremile with an all-zero single-feature D, so m is constant in every
    z-step and every z-step pools all rows into one block.  Two iterations; z against the isotonic KKT conditions
    (test_gpu_fullsize.check_isotonic_kkt) and the single-block value."""
    import admm_for_rank_based_loss_amd as rbl
    from oracle import pav, weights
    from test_gpu_fullsize import check_isotonic_kkt
    n, loss = CAP_N, BCE
    s = rbl.Solver(n, 1, "extremile", loss, reg=0.01, wstep=2, args=[2.0], tol=0.0, storage="f32")
    try:
        s.set_data(np.zeros((n, 1), dtype=np.float32), np.ones(n))
        s.gram()
        sigma, _ = weights.get_weights("extremile", n, [2.0])
        for it in range(2):
            st0 = s.get_state(want_z=False)
            m = -st0["lam"] / st0["rho"]                    # D = 0: m = D w - lambda / rho
            assert np.ptp(m) == 0.0
            s.phase_m()
            s.phase_z()
            z = s.get_state(want_lam=False)["z"]
            assert np.ptp(z) == 0.0, it
            x = pav.block_value(loss, math.fsum(sigma), float(m[0]) * n, n, st0["rho"])
            assert abs(z[0] - x) <= 1e-9 * max(1.0, abs(x)), (it, z[0], x)
            assert check_isotonic_kkt(loss, sigma, st0["rho"], m, z) == 1
            s.phase_q()
            s.phase_w()
            s.phase_dual(False)
            s.phase_finish()                                 # reports a kernel that did not complete
    finally:
        s.close()
