"""The quad-precision M-step reference and its gate (tests/mstep_ref.py), on the CPU.

  * the reference, fed the extended-precision E-step's sums, reproduces the oracle's trajectory under its extended-precision solve;
  * lambda = 0 with every P1 > 0 has the closed form T = y + R / P1, and the quad solve lands on it;
  * fp64 restatements of every kernel family's algorithm -- partial-pivot LU of A W = B then V = G W (the dense eliminations),
    tests/chain_numpy.py (the chain smoother), tests/band_numpy.py (the banded L D L^T) -- sit inside the gate on every case of the
    GPU matrix (tests/test_mstep_sums_gpu.py): the gate is not tighter than honest fp64 arithmetic of the same algorithm;
  * on every case the gate is at most 1/10 of the change rounding the sums to fp32 makes in T: it would see one fp32 slip;
  * the short-beta cells of the dense eliminations (beta = k h, tests/test_mstep_sums_gpu.py: short_beta_cases) can see a wrong kernel: the
    restatement takes at most 1/10 of the gate, partial pivoting swaps rows, and T* moves by 100 gates and more without the LLE term, without
    the priors and at the launch file's beta."""
import numpy as np
import pytest
import scipy.linalg as sla

import band_numpy as bn
import chain_numpy as cn
import estep_ref as R
import mstep_ref as MR
from conftest import case_kwargs, load_cases
from test_mstep_sums_gpu import CASES, DEC, HANDOVER_BAND, band_handover_case, build_case, case_scene, cid, lle_H, params_of

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


CPU_CASES = [cs for cs in CASES if cs["route"] != "lambda0"]      # (lambda = 0 with a zero row: no reference; the GPU test pins the refusal)


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
