"""The quad-precision M-step reference and its gate (tests/mstep_ref.py), on the CPU.

  * the reference, fed the extended-precision E-step's sums, reproduces the oracle's trajectory under its extended-precision solve;
  * lambda = 0 with every P1 > 0 has the closed form T = y + R / P1, and the quad solve lands on it;
  * fp64 restatements of every kernel family's algorithm -- partial-pivot LU of A W = B then V = G W (the dense eliminations),
    tests/chain_numpy.py (the chain smoother), tests/band_numpy.py (the banded L D L^T) -- sit inside the gate on every case of the
    GPU matrix (tests/test_mstep_sums_gpu.py): the gate is not tighter than honest fp64 arithmetic of the same algorithm;
  * on every case the gate is at most 1/10 of the change rounding the sums to fp32 makes in T: it would see one fp32 slip;
  * the short-beta cells of the dense eliminations (beta = k h, tests/test_mstep_sums_gpu.py: short_beta_cases) can see a wrong kernel: the
    restatement takes at most 1/10 of the gate, partial pivoting swaps rows, and T* moves by 100 gates and more without the LLE term, without
    the priors and at the launch file's beta;
  * the band's backward-error measure (mstep_ref.band_backward_error) can see a wrong kernel on every band cell: the fp64 restatements (the plain
    L D L^T, the kernel's tile data flow, both ends) take at most a quarter of the tolerance, the answer of the fp32-rounded sums stands at 10
    tolerances and more, the reference's dense system at 256 bits at a quarter at most, a missing term or a node's second-round data taken from
    the first round at 100 and more."""
import numpy as np
import pytest
import scipy.linalg as sla

import band_numpy as bn
import chain_numpy as cn
import estep_ref as R
import mstep_ref as MR
from conftest import case_kwargs, load_cases
from test_mstep_sums_gpu import CASES, DEC, HANDOVER_BAND, PE, _c, band_handover_case, build_case, by_backward_error, case_scene, cid, lle_H, params_of

LD = np.longdouble


def _no_vis(name):
    c = load_cases()[name]
    return not (case_kwargs(c)["k_vis"] != 0 and c.get("vis") is not None and len(c["vis"]) not in (0, len(c["Y0"])))


@pytest.mark.parametrize("name", [n for n in sorted(load_cases()) if _no_vis(n)])      # (visibility weighting: the E-step's dmin is not the M-step's)
def test_reference_reproduces_the_oracle(oracle, name):
    """Two consecutive M-steps (from the second on y != Y0 and the criterion's yp != y): T, sigma2 and the iteration count of oracle.cpd_lle
    (max_iter = k, tol = 0) under the extended-precision solve."""
    c = load_cases()[name]
    kw = case_kwargs(c)
    H = c.get("H")
    if kw["include_lle"] and H is None:
        L = oracle.calc_lle_weights(c["Y0"], 6)
        H = (np.eye(len(L)) - L).T @ (np.eye(len(L)) - L)
    X, Y0 = c["X"], c["Y0"]
    keep = R.prune(X, Y0)
    y = np.asarray(Y0, dtype=np.float64); yp = y; s2 = float(c["sigma2_in"])
    for k in (1, 2):
        r = R.estep(X, Y0, y, s2, mu=kw["mu"], keep=keep)
        case = MR.Case(r["sums"], Y0, y, r["sigma2"], beta=kw["beta"], lambda_=kw["lambda_"], alpha=kw["alpha"], priors=c.get("priors"),
                       lle_weight=kw["lle_weight"], H=H if kw["include_lle"] else None, yp=yp)
        T, s2L, crit = MR.reference(case)
        with oracle.extended_solver():
            o = oracle.cpd_lle(X, Y0, float(c["sigma2_in"]), priors=c.get("priors"), H=H, **dict(kw, max_iter=k, tol=0.0))
        assert o["iters"] == k
        assert float(np.abs(T.astype(np.float64) - o["Y"]).max()) <= 1e-12, (k, float(np.abs(T.astype(np.float64) - o["Y"]).max()))
        assert abs(float(s2L) - o["sigma2"]) <= 1e-9 * o["sigma2"]
        yp, y, s2 = y, T.astype(np.float64), float(s2L)
        assert crit > 0


@pytest.mark.parametrize("M", [8, 45, 129])
def test_closed_form_for_lambda_zero(M):
    from trackdlo_amd import synth
    X, Y0, _ = synth.scene(30 * M, M, config=900 + M)
    r = R.estep(X, Y0, Y0, 1e-3, mu=0.1)
    P1 = r["sums"][:M]
    assert (P1 > 0).all()
    c = MR.Case(r["sums"], Y0, Y0 + 1e-3, 1e-3, beta=0.35, lambda_=0.0)
    T, _, _ = MR.reference(c)
    Tc = MR.closed_form(c)
    scale = float(np.abs(Tc - c.y.astype(LD)).max())
    assert float(np.abs(T - Tc).max()) <= 1e-12 * max(scale, 1.0), float(np.abs(T - Tc).max())


# ---- fp64 restatements of the kernels' algorithms ------------------------------------------------------------------------------------------
def restated(c, kernel):
    """T from the same inputs, in fp64, by the kernel family's algorithm."""
    M = c.M
    G, D, g, H, cc, A, _ = MR.system(c)
    B = MR._W(c, G, np.eye(M))                    # (A = I: B itself, in fp64)
    if kernel == "dense":
        lu = sla.lu_factor(A)
        W = sla.lu_solve(lu, B)
        return c.Y0 + G @ W
    coord = R.chain_coord(c.Y0)
    if kernel == "chain":
        V = cn.chain_solve(coord, c.beta, cc, D, B)
    else:
        V, _ = bn.band_solve(coord, c.beta, cc, D, g, H, B)
    return c.Y0 + np.asarray(V)


_CPU = {}


def case_data(case):
    k = cid(case)
    if k not in _CPU:
        c = build_case(case)
        T, s2, crit = MR.reference(c)
        gT, gS, gC = MR.gate(c, case["family"], T)
        c32 = MR.Case(c.sums.astype(np.float32).astype(LD), c.Y0, c.y, c.s2, yp=c.yp, **c.kw())
        T32, _, _ = MR.reference(c32)
        _CPU[k] = (c, T, gT, float(np.abs(T32 - T).max()))
    return _CPU[k]


# (lambda = 0 with a zero row: no reference; the GPU test pins the refusal.  The band above 129 nodes: held by its backward error, further down)
CPU_CASES = [cs for cs in CASES if cs["route"] != "lambda0" and not by_backward_error(cs)]


@pytest.mark.parametrize("case", CPU_CASES, ids=cid)
def test_restatement_inside_the_gate(case):
    c, T, gT, _ = case_data(case)
    Tr = restated(c, case["family"])
    q = (np.abs(Tr - T.astype(np.float64)) / gT).max()
    assert q <= 1.0, (cid(case), float(q))


@pytest.mark.parametrize("case", CPU_CASES, ids=cid)
def test_gate_sees_an_fp32_slip(case):
    c, T, gT, slip = case_data(case)
    assert gT.max() <= 0.1 * slip, (cid(case), float(gT.max()), slip)


@pytest.mark.parametrize("regime", HANDOVER_BAND)
def test_band_hand_over_restatement_inside_the_dense_gate(regime):
    """The band's hand-over cases (tests/test_mstep_sums_gpu.py::test_band_hands_over_to_the_dense_kernels) take the dense pivoted kernels: their fp64
    restatement sits inside the dense gate there."""
    _, c, _, _, _ = band_handover_case(regime)
    T, _, _ = MR.reference(c)
    gT, _, _ = MR.gate(c, "dense", T)
    q = (np.abs(restated(c, "dense") - T.astype(np.float64)) / gT).max()
    assert q <= 1.0, (regime, float(q))


# ---- the short-beta cells of the dense eliminations (beta = k h): conditions on the reference alone, so that a cell can see a wrong kernel ----------
SHORT = [cs for cs in CPU_CASES if cs.get("beta_h")]
PIVOTING = [cs for cs in SHORT if (cs["route"] == "lle_dense" and cs["M"] <= 300) or cs["regime"] == "p1zero"]
TERMS = [(cs, "beta") for cs in SHORT] + [(cs, "lle") for cs in SHORT if cs["route"] == "lle_dense"] + [(cs, "priors") for cs in SHORT if cs["regime"] == "priors"]


@pytest.mark.parametrize("case", SHORT, ids=cid)
def test_short_beta_restatement_leaves_the_kernels_headroom(case):
    """The kernels eliminate in another order than LAPACK: the fp64 restatement takes at most a tenth of the gate."""
    c, T, gT, slip = case_data(case)
    q = float((np.abs(restated(c, "dense") - T.astype(np.float64)) / gT).max())
    print(f"{cid(case)}: beta {c.beta:.6g}, gate / slip {float(gT.max()) / slip:.3g}, restatement / gate {q:.3g}")
    assert q <= 0.1, (cid(case), q)


@pytest.mark.parametrize("case", PIVOTING, ids=cid)
def test_short_beta_cells_swap_rows(case):
    """Partial pivoting of A swaps at least one row: the cell exercises the kernels' pivot search."""
    c = case_data(case)[0]
    piv = sla.lu_factor(MR.system(c)[5])[1]
    n = int((piv != np.arange(c.M)).sum())
    print(f"{cid(case)}: {n} rows swapped")
    assert n >= 1, cid(case)


@pytest.mark.parametrize("case,term", TERMS, ids=[f"{cid(cs)}-{t}" for cs, t in TERMS])
def test_short_beta_every_term_reaches_the_answer(case, term):
    """T* moves by at least 100 gates (the largest move over the largest gate) when the LLE term or the priors are taken away or beta is the
    launch file's: a kernel that ignored H G, alpha J or the beta it was given would fail the GPU cell."""
    c, T, gT, _ = case_data(case)
    kw = {"lle": dict(H=None, lle_weight=0.0), "priors": dict(priors=None, alpha=0.0), "beta": dict(beta=params_of(dict(case, beta_h=None))["beta"])}[term]
    T2, _, _ = MR.reference(MR.Case(c.sums, c.Y0, c.y, c.s2, yp=c.yp, **dict(c.kw(), **kw)))
    q = float(np.abs(T2 - T).max()) / float(gT.max())
    print(f"{cid(case)} without {term}: T* moves by {q:.3g} gates")
    assert q >= 100.0, (cid(case), term, q)


@pytest.mark.parametrize("case", [cs for cs in DEC if cs.get("beta_h")], ids=cid)
def test_short_beta_crit_gate_pins_the_stopping_decision(case):
    """tests/test_mstep_sums_gpu.py::test_stopping_decision_and_refusals sets tol at crit (1 +- 1e-6): crit's gate is far below that."""
    c, T, _, _ = case_data(case)
    crit = MR.reference(c)[2]
    gC = MR.gate(c, "dense", T)[2]
    print(f"{cid(case)}: crit gate / crit {gC / float(crit):.3g}")
    assert gC < 1e-7 * float(crit), (cid(case), gC, float(crit))


def test_the_oracles_H_at_512_nodes_is_unbounded():
    """Why the LLE cells of 512 nodes and more take uniform_H: on the straight 0.02 m chain calc_lle_weights' local Gram matrices are singular to
    rounding and H = (I - L)^T (I - L) has entries above 1e12 -- the system's condition number is then 1e10 and more and no gate means anything.
    Should this stop holding, the cells can go back to the oracle's H."""
    case = next(cs for cs in SHORT if cs["route"] == "lle_dense" and cs["M"] == 512)
    hmax = float(np.abs(lle_H(case_scene(case)[3], "typical")).max())
    assert hmax > 1e12, hmax
    assert float(np.abs(build_case(case).H).max()) < 10.0


# ---- the band by its backward error (mstep_ref.band_backward_error): conditions on the CPU, so that a cell held by it can see a wrong kernel ---------
BAND = [cs for cs in CASES if cs["family"] == "band"]
BAND_NEW = [cs for cs in BAND if by_backward_error(cs)]           # held by the backward error alone
_BE = {}


def be_data(case):
    """(Case, fp64 restatement's T, its ratio) of a band cell, once."""
    k = cid(case)
    if k not in _BE:
        c = build_case(case)
        Tr = restated(c, "band")
        _BE[k] = (c, Tr, MR.band_backward_error(c, Tr))
    return _BE[k]


@pytest.mark.parametrize("M", [45, 257, 512])
def test_state_precision_series_against_mpmath(M):
    """K's entries in longdouble two ways -- the closed form at 256 bits (mpmath) and chain_link's positive series in longdouble -- agree to the
    series' own rounding: ~14 longdouble roundings (5.4e-20 each) per entry of Q, through det Q = q11 q22 - q12^2, which cancels 7-fold on these
    gaps: 5e-18, relative to the entry (the diagonal blocks' f-f' entries: relative to the two links' terms, which nearly cancel there)."""
    pytest.importorskip("mpmath")
    c = build_case(_c("band", "band", M, "typical"))
    (da, oa), (db, ob) = MR.state_precision_exact(c.Y0, c.beta, True), MR.state_precision_exact(c.Y0, c.beta, False)
    fp = np.abs(oa[:, 1]); fp[:-1] += np.abs(oa[1:, 1])
    w = max(float((np.abs(da[:, [0, 2]] - db[:, [0, 2]]) / np.abs(da[:, [0, 2]])).max()), float((np.abs(da[:, 1] - db[:, 1]) / fp).max()),
            float((np.abs(oa[1:] - ob[1:]) / np.abs(oa[1:])).max()))
    print(f"M {M}: state precision, series against mpmath {w:.3g}")
    assert w <= 5e-18, (M, w)


@pytest.mark.parametrize("case", BAND, ids=cid)
def test_band_restatement_leaves_the_kernel_headroom(case):
    """The kernel eliminates in another order (twisted plan, MFMA accumulation, contracted FMAs, rcp + correction): the fp64 restatement takes at
    most a quarter of the tolerance."""
    c, _, (q, where) = be_data(case)
    print(f"{cid(case)}: restatement / tolerance {q:.3g} at node {where[0]}")
    assert MR.band_system(c).chol is not None, cid(case)              # (the cell's own system has a Cholesky factor in fp64: the kernel's premise)
    assert q <= 0.25, (cid(case), q, where)


@pytest.mark.parametrize("M", [45, 257, PE[0], 512])
def test_band_data_flow_restatement_leaves_the_kernel_headroom(M):
    """The same for the kernel's own data flow: column records of (lambda K + gamma H), the system divided by sigma2, the circular window in a
    16 x 16 tile (band_numpy.build_records, tile_solve), and the elimination from both ends where the plan is two-ended (twisted_solve)."""
    c = build_case(_c("band", "band", M, "typical"))
    G, D, g, H, cc, _, _ = MR.system(c)
    B = MR._W(c, G, np.eye(M))
    coord = R.chain_coord(c.Y0)
    hb = bn.lle_band(H, M)
    x = bn.tile_solve(bn.build_records(coord, c.beta, c.lambda_, c.lle_weight, hb), D, B, c.s2, 2 * M)
    q, where = MR.band_backward_error(c, c.Y0 + x[0::2])
    msg = f"band M {M}: tile data flow / tolerance {q:.3g} at node {where[0]}"
    assert q <= 0.25, (M, q, where)
    bp = bn.band_plan(M)
    assert bp["tw"] == (0 if M == 512 else 1)
    if bp["tw"]:
        A, Rr = bn.assemble(coord, c.beta, cc, D, g, hb, B)
        q2, w2 = MR.band_backward_error(c, c.Y0 + bn.twisted_solve(A, Rr, bp["mT"])[0::2])
        msg += f", from both ends {q2:.3g} at node {w2[0]}"
        assert q2 <= 0.25, (M, q2, w2)
    print(msg)


def _c32(c):
    return MR.Case(c.sums.astype(np.float32).astype(LD), c.Y0, c.y, c.s2, yp=c.yp, **c.kw())


@pytest.mark.parametrize("case", BAND, ids=cid)
def test_band_backward_error_sees_an_fp32_slip(case):
    """The exact solution of the system whose sums were rounded to fp32 (a banded longdouble solve) stands at 10 tolerances and more."""
    c = be_data(case)[0]
    q, where = MR.band_backward_error(c, MR.band_exact(_c32(c)).astype(np.float64))
    print(f"{cid(case)}: fp32 slip / tolerance {q:.3g} at node {where[0]}")
    assert q >= 10.0, (cid(case), q)


@pytest.mark.parametrize("case", [cs for cs in BAND_NEW if cs["M"] <= 257] + [_c("band", "band", 512, "typical")], ids=cid)
def test_band_backward_error_follows_the_reference(case):
    """T* of the reference's dense system takes at most a quarter of the tolerance: the measure follows trackdlo.cpp's system, not only
    band_numpy's formulation of it.  T* is mstep_ref.reference_mp's: the dense system (c I + (D + g H) G) W = B, T = Y0 + G W at 256 bits, where the
    residual G W - V says to 40 digits and more that it IS that system's solution.  `reference`'s own T* (quad LU, G and A formed in longdouble) cannot
    make the statement for these cells: it carries its documented 1e-19 |G| |W| / |V|, 1e-16 m here and 1e-12 m under the oracle's H at 256 / 257
    nodes (|H| up to 9e10), which is 2.2 - 4.1 tolerances on six of these cells (0.7 - 0.9 at 45 - 129 nodes); its ratio and distance are printed beside."""
    pytest.importorskip("mpmath")
    c = be_data(case)[0]
    T, res = MR.reference_mp(c)
    q, where = MR.band_backward_error(c, T.astype(np.float64))
    msg = f"{cid(case)}: T* (256 bits; dense system's residual {res:.3g}) / tolerance {q:.3g} at node {where[0]}"
    if c.M <= 257:
        Tq = MR.reference(c)[0]
        msg += f"; the quad solve's T*: {MR.band_backward_error(c, Tq.astype(np.float64))[0]:.3g}, {float(np.abs(Tq - T).max()):.3g} m away"
    print(msg + f"; banded longdouble solve {float(np.abs(MR.band_exact(c) - T).max()):.3g} m away")
    assert res <= 1e-40, (cid(case), res)
    assert q <= 0.25, (cid(case), q, where)


BAND_TERMS = [(cs, t) for cs in BAND_NEW for t in ("lle", "beta") + (("priors",) if cs["regime"] == "priors" else ())]


@pytest.mark.parametrize("case,term", BAND_TERMS, ids=[f"{cid(cs)}-{t}" for cs, t in BAND_TERMS])
def test_band_every_term_reaches_the_answer(case, term):
    """T* of the case without the LLE term, without the priors, or at the launch file's beta stands at 100 tolerances and more against the true case
    (the quad solve up to 257 nodes, the banded longdouble solve beyond, the 256-bit one where that does not converge)."""
    from trackdlo_amd import synth
    c = be_data(case)[0]
    kw = {"lle": dict(H=None, lle_weight=0.0), "priors": dict(priors=None, alpha=0.0), "beta": dict(beta=synth.LAUNCH_PARAMS["beta"])}[term]
    assert term != "beta" or kw["beta"] != c.beta
    c2 = MR.Case(c.sums, c.Y0, c.y, c.s2, yp=c.yp, **dict(c.kw(), **kw))
    if c.M <= 257:
        T2 = MR.reference(c2)[0]
    else:
        try:
            T2 = MR.band_exact(c2)
        except MR.NotRefined:                  # (512 nodes, P1 zeroed, the launch file's beta under the oracle's H: beyond longdouble refinement)
            T2 = MR.reference_mp(c2)[0]
    q, _ = MR.band_backward_error(c, T2.astype(np.float64))
    print(f"{cid(case)} without {term}: {q:.3g} tolerances")
    assert q >= 100.0, (cid(case), term, q)


# The second round of the kernel's node loop (thread t serves node t and node t + 256): what it reads per node is P1 and R (the sums), alpha J and
# alpha (Y_ext - Y0) (the priors), H Y0.  A round that read node m - 256's value for node m is shown here on the restatement, one array at a time.
ROUND2 = [cs for cs in BAND_NEW if cs["M"] > 256]
ROUND2_ARRAYS = ("P1", "R", "priors", "H Y0")
_R2 = {}


def second_round(case):
    """{array: ratio of the restatement with that array's second round taken from the first, or None where the replacement changes no value by more
    than 1e-12 of itself}."""
    k = cid(case)
    if k not in _R2:
        c = be_data(case)[0]
        M = c.M
        a = {"P1": c.sums[:M].astype(np.float64), "R": c.sums[M:4 * M].reshape(3, M).T.astype(np.float64), "aJ": np.zeros(M), "aY": np.zeros((M, 3)),
             "H Y0": np.asarray(c.H) @ c.Y0}
        for r in (c.priors if c.priors is not None else ()):
            a["aJ"][int(r[0])] = c.alpha; a["aY"][int(r[0])] = c.alpha * (r[1:] - c.Y0[int(r[0])])
        g = c.s2 * c.lle_weight; cc = c.lambda_ * c.s2

        def solve(v):
            B = v["R"] + v["P1"][:, None] * (c.y - c.Y0) + v["aY"] - g * v["H Y0"]
            return c.Y0 + bn.band_solve(R.chain_coord(c.Y0), c.beta, cc, v["P1"] + v["aJ"], g, np.asarray(c.H), B)[0]

        assert MR.band_backward_error(c, solve(a))[0] <= 0.25
        out = {}
        for name in ROUND2_ARRAYS:
            v = dict(a)
            for key in (("aJ", "aY") if name == "priors" else (name,)):
                v[key] = a[key].copy(); v[key][256:] = a[key][:M - 256]
            same = all(np.allclose(v[key], a[key], rtol=1e-12, atol=0.0) for key in v)     # (1e-12: (Y0 + 0.003) - Y0 at two nodes differs by the rounding of the sum)
            out[name] = None if same else MR.band_backward_error(c, solve(v))[0]
        _R2[k] = out
    return _R2[k]


@pytest.mark.parametrize("case", ROUND2, ids=cid)
def test_band_second_round_of_the_node_loop_is_seen(case):
    """Every replacement that changes a value stands at 100 tolerances and more.  Where it changes none (257 nodes: node 256 alone is in the second
    round, and in the P1-zeroed and the priors cell it carries the same values as node 0: both are chain ends) a kernel with that mistake computes
    this cell right; test_band_second_round_every_array_is_seen_somewhere holds that another cell sees it."""
    for name, q in second_round(case).items():
        print(f"{cid(case)}, {name} of node m - 256 at node m: " + ("no value changes" if q is None else f"{q:.3g} tolerances"))
        assert q is None or q >= 100.0, (cid(case), name, q)


def test_band_second_round_every_array_is_seen_somewhere():
    for name in ROUND2_ARRAYS:
        seen = [cid(cs) for cs in ROUND2 if (second_round(cs)[name] or 0.0) >= 100.0]
        assert seen, name
        if name != "priors":
            assert any("-M257-" in s for s in seen) and any("-M512-" in s for s in seen), (name, seen)


@pytest.mark.parametrize("case", [_c("band", "band", 45, "typical"), _c("band", "band", 257, "priors")], ids=cid)
def test_held_at_T_is_the_references_sigma2_and_crit(case):
    """mstep_ref.held_at_T at the reference's own T* (rounded to fp64, as a kernel returns it) gives the reference's sigma2 and crit within its gates, and
    those gates are the part of mstep_ref.gate's that does not come from T's error: never wider."""
    c = be_data(case)[0]
    T, s2, crit = MR.reference(c)
    s2k, gS, critk, gC = MR.held_at_T(c, T.astype(np.float64))
    _, gS_full, gC_full = MR.gate(c, "band", T)
    assert abs(float(s2k - s2)) <= gS and abs(float(critk - crit)) <= gC
    assert 0 < gS <= gS_full and 0 < gC <= gC_full and gC < 1e-7 * float(crit)
