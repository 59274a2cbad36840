"""The extended-precision E-step reference (tests/estep_ref.py) against the oracle, on the CPU.

The reference's sums, run through an fp64 M-step with the oracle's extended-precision solve, must reproduce the oracle's
trajectory (oracle.cpd_lle with max_iter = k, tol = 0) for k = 1, 2, 3 -- on every committed case of
tests/golden/oracle_cases.npz (priors, visibility, the end-node gap quirk, the LLE term, ...) and on synth.scene draws --
and count the end-node gap quirk as the oracle does.  Only then may tests/test_estep_sums_gpu.py hold the kernels to it."""
import numpy as np
import pytest

import estep_ref as R
from conftest import case_kwargs, load_cases

TOL_Y = 1e-12


def _run(oracle, X, Y0, s2_in, kw, priors=None, vis=None, H=None, iters=3):
    Y = np.asarray(Y0, dtype=np.float64).copy(); s2 = float(s2_in)
    keep = R.prune(X, Y0)
    dq = None
    quirk = 0
    for k in range(1, iters + 1):
        if vis is not None and len(vis) and kw["k_vis"] != 0:
            dq = R.dmin_sq(np.asarray(X)[keep], Y)
        r = R.estep(X, Y0, Y, s2, mu=kw["mu"], k_vis=kw["k_vis"], visibility_threshold=kw["visibility_threshold"], visible_nodes=vis,
                    dmin_sq_global=dq, keep=keep)
        quirk += r["gap_quirk"]
        Y, s2 = R.mstep(r["sums"], Y0, Y, r["sigma2"], beta=kw["beta"], lambda_=kw["lambda_"], solve=oracle.solve_extended,
                        alpha=kw["alpha"], priors=priors, lle_weight=kw["lle_weight"], H=H if kw["include_lle"] else None)
        okw = dict(kw, max_iter=k, tol=0.0)
        o = oracle.cpd_lle(X, Y0, s2_in, priors=priors, visible_nodes=vis, H=H, **okw)
        dy = float(np.abs(Y - o["Y"]).max())
        assert o["iters"] == k and r["N"] == o["n_kept"]
        assert dy <= TOL_Y, (k, dy)
        assert abs(s2 - o["sigma2"]) <= 1e-9 * o["sigma2"], (k, s2, o["sigma2"])
        assert quirk == o["gap_quirk"], (k, quirk, o["gap_quirk"])
    return quirk


@pytest.mark.parametrize("name", sorted(load_cases()))
def test_reference_reproduces_the_oracle_on_the_committed_cases(oracle, name):
    c = load_cases()[name]
    kw = case_kwargs(c)
    H = c.get("H")
    if kw["include_lle"] and H is None:
        L = oracle.calc_lle_weights(c["Y0"], 6)
        H = (np.eye(len(L)) - L).T @ (np.eye(len(L)) - L)
    with oracle.extended_solver():
        q = _run(oracle, c["X"], c["Y0"], float(c["sigma2_in"]), kw, priors=c.get("priors"), vis=c.get("vis"), H=H)
    if name == "quirk":
        assert q > 0                                            # the fixture exists for this branch


@pytest.mark.parametrize("N,M,cfg,vis,s2", [(3000, 45, 1, False, 0.0), (2500, 64, 2, True, 0.0), (1999, 8, 3, False, 1e-4),
                                            (4000, 129, 4, False, 0.0), (1500, 30, 5, False, 1e-6)])
def test_reference_reproduces_the_oracle_on_synth_scenes(oracle, N, M, cfg, vis, s2):
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    X, Y0, v = synth.scene(N, M, config=cfg, occlude=(0.4, 0.6) if vis else None, outliers=5)
    vext = np.asarray(synth.extend_visible(v, M, synth.geodesic_coord(Y0)), dtype=np.int32) if vis else None
    kw = dict(beta=P["beta"], lambda_=P["lambda_"], lle_weight=P["lle_weight"], mu=P["mu"], include_lle=False, alpha=0.0,
              k_vis=P["k_vis"] if vis else 0.0, visibility_threshold=P["visibility_threshold"])
    with oracle.extended_solver():
        _run(oracle, X, Y0, s2, kw, vis=vext)


def test_reference_counts_the_end_node_gap_and_the_underflow_rows(oracle):
    """The chain's tips folded back (as tests/test_estep_wide_gpu.py builds it): the gap quirk's count equals the oracle's; and at a sigma2
    far below the data's every Euclidean membership of the outliers underflows in fp64 -- those points go to node 0 as in the oracle."""
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    N, M = 3000, 60
    X, Y0, _ = synth.scene(N, M, config=777, outliers=20)
    rng = np.random.default_rng(5)
    X = np.asarray(X).copy(); Y0 = np.asarray(Y0).copy()
    Y0[1] += (0.0, 0.0, 0.09); Y0[M - 2] += (0.0, 0.0, 0.09)
    X[:200] = Y0[0] + rng.normal(0, 0.004, (200, 3))
    X[200:400] = Y0[M - 1] + rng.normal(0, 0.004, (200, 3))
    X[400:460] = Y0[20:50:1].repeat(2, axis=0) + (0.0, 0.0, 0.06)        # 6 cm off the chain: beyond fp64's exp at sigma2 = 1e-6
    kw = dict(beta=P["beta"], lambda_=P["lambda_"], lle_weight=P["lle_weight"], mu=P["mu"], include_lle=False, alpha=0.0, k_vis=0.0,
              visibility_threshold=P["visibility_threshold"])
    with oracle.extended_solver():
        assert _run(oracle, X, Y0, 0.0, kw, iters=2) > 100
        _run(oracle, X, Y0, 1e-6, kw, iters=2)
    r = R.estep(X, Y0, Y0, 1e-6, mu=kw["mu"])
    assert r["n_underflow"] >= 60
