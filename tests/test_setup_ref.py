"""CPU suite: the set-up stage's reference (tests/setup_ref.py) against things it did not come from, and the conditions ("caps") of every
scene tests/test_setup_gpu.py registers -- checked here, where no GPU is needed."""
import numpy as np
import pytest

import estep_ref as R
import mstep_ref as MR
import setup_ref as S
import test_setup_gpu as TG

LD = np.longdouble
U = S.U


def test_threshold_is_the_first_double_whose_root_reaches_a_tenth():
    t = S.T_KEEP
    assert np.sqrt(t) >= 0.1 and np.sqrt(np.nextafter(t, 0.0)) < 0.1
    # on the 2^-26 m grid d2 = n 2^-52: the two integers either side
    assert TG.N_KEPT_MAX * 2.0 ** -52 < t <= TG.N_PRUNED_MIN * 2.0 ** -52 and TG.N_PRUNED_MIN == TG.N_KEPT_MAX + 1
    assert np.sqrt(TG.N_KEPT_MAX * 2.0 ** -52) < 0.1 <= np.sqrt(TG.N_PRUNED_MIN * 2.0 ** -52)


def test_grid_scene_realises_integers_next_to_the_threshold():
    """An integer 4^a (8 b + 7) is no sum of three squares: the scene takes the nearest representable ones; how far they are from the boundary."""
    sc = TG.scene_grid(8)
    kept_n, prun_n = sc["edge_n"]
    assert max(kept_n) <= TG.N_KEPT_MAX and min(prun_n) >= TG.N_PRUNED_MIN
    assert TG.N_KEPT_MAX - max(kept_n) <= 2 and min(prun_n) - TG.N_PRUNED_MIN <= 2, (kept_n, prun_n)
    assert TG.N_KEPT_MAX - min(kept_n) <= 16 and max(prun_n) - TG.N_PRUNED_MIN <= 16
    d = S.decide(sc["X"], sc["Y0"], exact=True)
    n = np.round(d["dmin"] * 2.0 ** 52)
    assert (n * 2.0 ** -52 == d["dmin"]).all()                 # every d2 is an integer number of 2^-52: the arithmetic is exact
    for v in kept_n:
        assert ((n == v) & d["kept"]).any()
    for v in prun_n:
        assert ((n == v) & ~d["kept"]).any()
    print(f"grid scene: largest kept d2 = {int(n[d['kept']].max())} 2^-52, smallest pruned = {int(n[~d['kept']].min())} 2^-52")


@pytest.mark.parametrize("label,build", TG.all_scenes(), ids=[l for l, _ in TG.all_scenes()])
def test_conditions_of_every_gpu_scene(label, build):
    sc = build()
    r = TG.reference(sc)
    TG.caps(sc, r)
    if sc["claim"] == "razor":
        assert sc["made"] >= 40


def test_screened_margins_equal_the_unscreened_ones():
    """decide() forms the longdouble margins only below an fp64 margin of 2^-30: the pinned set is that of the full evaluation."""
    for sc in (TG.scene_razor(), TG.scene_shell(3000, 45)):
        X, Y0 = sc["X"], sc["Y0"]
        d = S.decide(X, Y0)
        a = (Y0[None, :, :] - X[:, None, :]).astype(LD)
        d2 = (a * a).sum(axis=2)
        srt = np.sort(d2, axis=1)
        mt = np.abs(srt[:, 0] / LD(S.T_KEEP) - 1).astype(np.float64)
        mq = np.where(d["kept"], ((srt[:, 1] - srt[:, 0]) / srt[:, 1]).astype(np.float64), np.inf)
        assert np.array_equal((mt > S.PIN) & (mq > S.PIN), d["pinned"])


def test_prune_is_estep_refs_and_the_oracles(oracle):
    """n_kept: every committed golden case, and live oracle runs (one iteration) on the new edge scenes -- shell, grid, razor band (the oracle
    evaluates the fp64 formula without fused multiply-adds: decide()'s `kept` is that evaluation, unpinned points included), non-finite points."""
    from test_oracle_golden import load_cases
    for name, c in load_cases().items():
        d = S.decide(c["X"], c["Y0"])
        assert int(d["kept"].sum()) == int(c["n_kept"]), name
        assert np.array_equal(d["kept"], R.prune(c["X"], c["Y0"]))
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    kw = dict(beta=P["beta"], lambda_=P["lambda_"], lle_weight=P["lle_weight"], mu=P["mu"], max_iter=1, tol=0.0, include_lle=False, alpha=0.0, k_vis=0.0,
              visibility_threshold=P["visibility_threshold"])
    for sc in (TG.scene_shell(6000, 45), TG.scene_grid(7), TG.scene_grid(12), TG.scene_razor(), TG.scene_shell(5000, 45, cfg=950, off=(12.0, -7.0, 3.0))):
        d = S.decide(sc["X"], sc["Y0"], exact=sc["exact"])
        o = oracle.cpd_lle(sc["X"], sc["Y0"], 0.0, **kw)
        assert o["n_kept"] == int(d["kept"].sum()), (sc["claim"], o["n_kept"], int(d["kept"].sum()))


def test_sum_d2_around_the_centroid_is_the_direct_sum():
    for sc in (TG.scene_shell(3000, 45), TG.scene_shell(2000, 64, off=(12.0, -7.0, 3.0)), TG.scene_grid(9)):
        d = S.decide(sc["X"], sc["Y0"], exact=sc["exact"])
        a = TG.sum_d2_centred(sc["X"][d["kept"]], sc["Y0"]); b = R.sum_d2(sc["X"][d["kept"]], sc["Y0"])
        assert abs(float((a - b) / b)) <= 2.0 ** -58


def test_sorted_order_is_a_stable_counting_sort():
    sc = TG.scene_shell(3000, 45)
    d = S.decide(sc["X"], sc["Y0"])
    order, starts = S.sorted_order(d["kept"], d["nearest"], 45)
    assert len(order) == d["kept"].sum() and starts[0] == 0 and starts[-1] == len(order)
    nn = d["nearest"][order]
    assert (np.diff(nn) >= 0).all()
    for m in range(45):
        run = order[starts[m]:starts[m + 1]]
        assert (nn[starts[m]:starts[m + 1]] == m).all() and (np.diff(run) > 0).all()


GAPS = [1e-9, 1e-6, 1e-3, 0.02, 0.3, 3.0]


def to_mp(mp, v):
    """A longdouble as an mpf, exactly (mantissa in two fp64 pieces, exponent apart: the value may lie below fp64's range)."""
    m, e = np.frexp(LD(v))
    hi = float(m); lo = float(m - LD(hi))
    return mp.ldexp(mp.mpf(hi) + mp.mpf(lo), int(e))


@pytest.mark.parametrize("beta", TG.BETAS)
def test_links_against_mpmath(beta):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    hs = GAPS + [TG.gap_for(beta, t) for t in TG.X_TARGETS]
    for h in hs:
        v, _ = S.links(h, beta)
        b = mp.mpf(beta); hh = mp.mpf(float(h))
        s = mp.sqrt(2) / b; sf2 = 1 / (2 * mp.sqrt(2) * b); x = s * hh
        e = mp.exp(-x); e2 = mp.exp(-2 * x)
        want = [e * (1 + x), e * hh, -s * s * hh * e, e * (1 - x), sf2 * (1 - e2 * (1 + 2 * x + 2 * x * x)), 2 * sf2 * s ** 3 * hh * hh * e2,
                sf2 * s * s * (1 - e2 * (1 - 2 * x + 2 * x * x))]
        for k in range(7):
            got = to_mp(mp, v[k])
            tol = (mp.mpf(2) ** -58 + x * mp.mpf(2) ** -62) * abs(want[k]) + mp.mpf(10) ** -4900      # (exp's argument carries longdouble's 2^-64: x 2^-63 in e, twice in e2)
            if k == 3:
                tol += mp.mpf(2) ** -60 * e                     # (1 - x cancels: absolute in e)
            assert abs(got - want[k]) <= tol, (beta, h, k, got, want[k])
    r0 = S.row0(beta)
    b = mp.mpf(beta); s = mp.sqrt(2) / b; sf2 = 1 / (2 * mp.sqrt(2) * b)
    for got, want in zip(r0, [sf2, s * s * sf2, 1 / sf2, 1 / (s * s * sf2)]):
        assert abs(to_mp(mp, got) - want) <= mp.mpf(2) ** -60 * want


@pytest.mark.parametrize("beta", TG.BETAS)
def test_link_identities(beta):
    """Phi11(h) Pinf11 = G(h) (trackdlo.cpp:233, mstep_ref.kernel_G in longdouble); Q = Pinf - Phi Pinf Phi^T evaluated directly where that form
    does not cancel (x >= 1); the reference is continuous across x = 1 (it has no switch there)."""
    p = S.row0(beta)
    for h in GAPS + [TG.gap_for(beta, 2.0), TG.gap_for(beta, 20.0)]:
        v, q = S.links(h, beta)
        Y0 = np.array([[0.0, 0, 0], [h, 0, 0]])
        _, G = MR.kernel_G(Y0, beta, dtype=LD)
        assert abs(float((v[0] * p[0] - G[0, 1]) / G[0, 1])) <= 2.0 ** -58, (beta, h)
        if q["x"] >= 1:
            Phi = np.array([[v[0], v[1]], [v[2], v[3]]], dtype=LD); Pinf = np.diag(p[:2])
            Q = Pinf - Phi @ Pinf @ Phi.T
            for got, want in ((v[4], Q[0, 0]), (v[5], Q[0, 1]), (v[6], Q[1, 1])):
                assert abs(float((got - want) / want)) <= 2.0 ** -54, (beta, h)
            assert abs(float(Q[0, 1] - Q[1, 0])) <= 2.0 ** -60 * float(abs(Q[0, 1]))
    a, _ = S.links(TG.gap_for(beta, "1-"), beta); b, _ = S.links(TG.gap_for(beta, "1+"), beta)
    assert (np.abs(((a - b) / b).astype(np.float64)[[0, 1, 2, 4, 5, 6]]) <= 2.0 ** -48).all()


def test_link_gates_hold_an_fp64_restatement_and_see_a_short_series():
    """The gates are neither too tight for honest fp64 arithmetic -- the documented formulas evaluated in numpy fp64, series of 31 terms below
    x = 1 -- nor too loose to see the series cut at 10 terms."""
    for beta in TG.BETAS:
        for h in GAPS + [TG.gap_for(beta, t) for t in TG.X_TARGETS]:
            s = np.sqrt(2.0) / beta; sf2 = 1.0 / (2.0 * np.sqrt(2.0) * beta)
            x = s * h; e = np.exp(-x); e2 = e * e

            def entries(nmax):
                if x < 1.0:
                    tt = 2.0 * x; term = tt * tt * tt / 6.0; sm = term
                    for n in range(4, nmax):
                        term *= tt * (1.0 / n); sm += term
                    u11 = e2 * sm; u22 = e2 * (4.0 * x + sm)
                else:
                    u11 = 1.0 - e2 * (1.0 + 2.0 * x + 2.0 * x * x); u22 = 1.0 - e2 * (1.0 - 2.0 * x + 2.0 * x * x)
                return np.array([e * (1.0 + x), e * h, -s * s * h * e, e * (1.0 - x), sf2 * u11, 2.0 * sf2 * s * s * s * h * h * e2, sf2 * s * s * u22])
            v, g = S.link_gates(h, beta)
            err = np.abs((entries(34).astype(LD) - v).astype(np.float64))
            assert (err <= g).all(), (beta, h, err / g)
            if 0.25 <= x < 1.0:
                err = np.abs((entries(10).astype(LD) - v).astype(np.float64))
                assert err[4] > 10 * g[4], (beta, h, err[4] / g[4])


def test_hy0_reference_is_the_dense_product():
    rng = np.random.default_rng(3)
    M = 20
    H = rng.normal(size=(M, M)); H = H + H.T
    H[np.abs(np.subtract.outer(np.arange(M), np.arange(M))) > 6] = 0
    Y = rng.normal(size=(M, 3)) + 5
    got, mass = S.hy0(S.band_of(H), Y)
    want = H.astype(LD) @ Y.astype(LD)
    assert (np.abs((got - want).astype(np.float64)) <= 2.0 ** -60 * mass.astype(np.float64)).all()
