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


# ---- k_estep2: its gate (tests/test_estep_sums_gpu.py::gate2) is honest -----------------------------------------------------------------
# (The second and third E-steps of the GPU matrix start from the kernel's own M-steps; here they start from the reference's.)
# a. an fp32 restatement of the kernel's data flow (tests/estep2_numpy.py) lies inside the gate on every case of the GPU matrix, at both tile
#    heights;  b. the gate sees one point on every case;  c. each plausible mistake of the restatement leaves the gate by 10 x on a named case;
#    d. every scene has the property the GPU test runs it for, asserted on the reference's structure.
import estep2_numpy as E2
import test_estep_sums_gpu as S

_E2 = {}


def _e2(c):
    """(X, Y0, reference, gate, restatement inputs) of a case, once."""
    k = S.ckey(c)
    if k not in _E2:
        from trackdlo_amd import synth
        P = synth.LAUNCH_PARAMS
        X, Y0, vis = S.e2_scene(c)
        dq = None
        if vis is not None:
            dq = R.dmin_sq(X[R.prune(X, Y0)], Y0, fp32=True).astype(np.float64) * c["dq_scale"]
            if c.get("dq_step"):
                dq = S.stepped_dmin(len(Y0), c["dq_step"])
        _, _, _, r, g = S.e2_ref(c, dq=dq)
        Xs, kidx = S.sorted_cloud(X, Y0)
        s2 = r["sigma2"]
        mu = c.get("mu", P["mu"])
        cn = (2.0 * np.pi * s2) ** 1.5 * mu / (1.0 - mu)                                   # set_iter_consts
        cn = cn / r["N"] if r["vis_branch"] else cn * len(Y0) / r["N"]
        kw = dict(Xs=Xs, Y=Y0, coord=R.chain_coord(Y0), sigma2=s2, c_norm=cn, sh=S.shifts(c["N0"], Y0, 0, s2, True),
                  vis=dict(dq=dq, k_vis=P["k_vis"], thr=P["visibility_threshold"]) if r["vis_branch"] else None)
        _E2[k] = (X, Y0, r, g, kw, kidx)
    return _E2[k]


def _ratio(c, TR, variant=None):
    _, Y0, r, g, kw, _ = _e2(c)
    out, info = E2.estep2(TR=TR, variant=variant, **kw)
    M = len(Y0)
    q = np.abs(out - r["sums"][:4 * M + 1]).astype(np.float64) / g
    return float(q.max()), info


@pytest.mark.parametrize("c", S.e2_cases(), ids=S.cid)
def test_estep2_gate_contains_the_restatement_and_sees_one_point(c):
    _, _, r, g, _, _ = _e2(c)
    S.assert_gate_sees_one_point(r, g, S.cid(c))
    for TR in (8, 16):
        q, info = _ratio(c, TR)
        print(f"{S.cid(c)} rows {TR}: restatement {q:.3f} of gate2; candidates {min(info['cands'])}-{max(info['cands'])}, "
              f"windows {min(info['window'])}-{max(info['window'])}, forms {sorted(info['modes'])}")
        assert q <= 1.0, (S.cid(c), TR, q)


def _case(**kw):
    return next(c for c in S.e2_cases() if all(c.get(k) == v for k, v in kw.items()))


# variant -> (case, TR) on which it must leave the gate by 10 x
CAUGHT_ON = {
    "half_range": (dict(N0=321, M=64), 8),
    "gap_one_point": (dict(gap=True), 8),
    "mode2_in_gap": (dict(gap=True), 8),
    "no_node0_rule": (dict(off=64), 8),
    "no_lv_span": (dict(dq_step=(20, 0.5)), 8),
    "vis_one_point": (dict(dq_scale=0.81, s2=0.0), 8),
    "q_cross_dropped": (dict(N0=321, M=64), 8),
    "q_cross_sign": (dict(N0=321, M=64), 8),
    "tail_copies_weighted": (dict(N0=37), 8),
    "first_chunk_only": (dict(win=24), 8),
}


@pytest.mark.parametrize("variant", E2.VARIANTS)
def test_estep2_gate_sees_each_wrong_variant(variant):
    """Each plausible mistake of the restatement leaves gate2 by 10 x on the case named in CAUGHT_ON.  Measured (rows 8): half_range 209,
    gap_one_point 14.6, mode2_in_gap 4.2e3, no_node0_rule 1.1e5, vis_one_point 8.4e5, q_cross_dropped 1.1e4, q_cross_sign 2.3e4,
    tail_copies_weighted 3.7e6, first_chunk_only 1.6e5, no_lv_span 26.7.

    no_lv_span needs a scene built for it.  On the visibility scenes of the launch parameters it is invisible (0.015 of the gate with lv_span and
    without): a window without lv_span drops at most 2^(lv_span - 36) of the point's nearest membership, the outlier term c (2^-31 at these
    sizes) bounds the normaliser from below, the wave's window is the union over 128 points, and at the window's edge the geodesic exponent
    falls by 10 .. 27 bits per node.  The scene named in CAUGHT_ON removes each of the four (e2_cases says how)."""
    sel, TR = CAUGHT_ON[variant]
    c = _case(**sel)
    q, _ = _ratio(c, TR, variant)
    print(f"{variant} on {S.cid(c)} rows {TR}: {q:.3g} of gate2")
    assert q >= 10.0, (variant, S.cid(c), q)


def _batches(c):
    """Per 128-point batch of the sorted cloud: the reference's nearest nodes, pairs and underflow flags of its points."""
    _, _, r, _, _, kidx = _e2(c)
    return [(r["near"][kidx[b:b + 128]], r["lo"][kidx[b:b + 128]], r["hi"][kidx[b:b + 128]], r["under"][kidx[b:b + 128]]) for b in range(0, len(kidx), 128)]


@pytest.mark.parametrize("c", S.e2_cases(), ids=S.cid)
def test_estep2_scenes_have_the_property_they_are_run_for(c):
    bs = _batches(c)
    _, Y0, r, _, _, _ = _e2(c)
    span = max(int(a[~u].max() - a[~u].min()) + 1 for a, _, _, u in bs if not u.all())      # (an all-underflow column's node 0 is no nearest node)
    if c.get("far"):
        assert span >= 17, span                          # the plain search beyond 16 candidates
        assert max(_ratio(c, 8)[1]["cands"]) > 16
    else:
        assert span <= 16, span
        assert min(_ratio(c, 8)[1]["cands"]) <= 16       # ... and the search that drops four bits elsewhere
    if c.get("gap"):
        assert any(((hi - lo) == 2).any() and ((hi - lo) == 1).any() for _, lo, hi, _ in bs)
        assert r["gap_quirk"] > 100
    if c.get("off"):
        assert any(u.any() and not u.all() for _, _, _, u in bs)
        assert r["n_underflow"] >= c["off"]
    if c.get("win"):
        w = S.window_nodes(Y0, c["s2"], 0)
        assert c["win"] - 1 <= w <= c["win"] + 1, (c["win"], w)
    if c["s2"] == 0.5:
        assert min(_ratio(c, 8)[1]["window"]) == c["M"]  # the whole chain


@pytest.mark.parametrize("M", [45, 64])
def test_estep2_gate_contains_the_restatement_at_later_iterations(oracle, M):
    """The scenes of the GPU matrix's second and third E-steps, at the (Y_k, sigma2_k) the reference's own M-steps give."""
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    c = dict(N0=7000 + 65, M=M, cfg=540 + M, prec=0, s2=0.0)
    X, Y0, r, g, kw, _ = _e2(c)
    Y, s2 = Y0, r["sigma2"]
    for k in (1, 2):
        with oracle.extended_solver():
            Y, s2 = R.mstep(r["sums"], Y0, Y, s2, beta=P["beta"], lambda_=P["lambda_"], solve=oracle.solve_extended)
        _, _, _, r, g = S.e2_ref(c, Y=Y, s2=s2, key=("cpu", k))
        S.assert_gate_sees_one_point(r, g, f"{S.cid(c)}-it{k + 1}")
        cn = (2.0 * np.pi * s2) ** 1.5 * P["mu"] / (1.0 - P["mu"]) * M / r["N"]
        for TR in (8, 16):
            out, _ = E2.estep2(TR=TR, **dict(kw, Y=Y, sigma2=s2, c_norm=cn, sh=S.shifts(c["N0"], Y0, 0, s2, True)))
            q = float((np.abs(out - r["sums"][:4 * M + 1]).astype(np.float64) / g).max())
            print(f"{S.cid(c)} rows {TR} E-step {k + 1}: restatement {q:.3f} of gate2")
            assert q <= 1.0, (M, k, TR, q)
