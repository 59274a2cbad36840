"""Each M-step kernel from given sums against the quad-precision solve (tests/mstep_ref.py), node by node.

The N-split step API (trackdlo_amd.nsplit.HipShard on one context) runs begin -> set_global -> estep -> mstep(sums) -> end, and mstep copies any
sums [P1 | R | Q | N_kept] into the frame (from_sums = 1): that reaches every M-step kernel.  The sums are the extended-precision E-step's
(tests/estep_ref.py) of a synth scene, then edited: P1 (with R) zeroed at the chain's ends and at the smoother's junction nodes, a single observed
node, priors there, lambda sigma2 over eleven decades, an LLE regulariser whose rows do not sum to zero on a scene 12 m from the origin.  T and
sigma2 must lie within `mstep_ref.gate`, and done / iters / converged must be the reference's decisions exactly.  Every case names the kernel it
reached (Context.profile_iteration: mstep_kernel_name).  The dense eliminations from 129 nodes on and every dense LLE elimination are held at a
beta of the order of the node spacing (short_beta_cases; the comment above DROPPED says why and with which ratios).  The banded solve is held by its
backward error (mstep_ref.band_backward_error) at every chain length, above 129 nodes by that alone: 256 / 257 nodes (a thread's second node), both
sides of BandPlan's edge, 480 and 512 (one direction, more than 64 KB of LDS), with the stopping decision at the kernel's own crit.

After a successful M-step the next E-step must start from it: its sums match the E-step reference at the kernel's own (T, sigma2), and in fp64 mode
their resolution follows the new sigma2 (IterState::sh_boost, set_iter_consts) -- every R x 2^sR an integer, not all of them even."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import band_numpy as bn  # noqa: E402
import chain_numpy as cn  # noqa: E402
import estep_ref as R  # noqa: E402
import mstep_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu
LD = np.longdouble
SHIFT = np.array([10.0, -7.0, 3.0])


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------
def _direct_edge():
    """The chain lengths on both sides of nQ = kDirectMax = 21 steps per direction (ChainCarve): the backward pass walked step by step or in strides."""
    Ms = [M for M in range(40, 120) if cn.carve(M)[4] == 21]
    return Ms[-1], Ms[-1] + 1


def _plan_edge():
    """The longest chain whose elimination runs from both ends (BandPlan: both directions' records fit the LDS) and the next one, one direction again."""
    Ms = [M for M in range(19, 513) if bn.band_plan(M)["tw"]]
    return Ms[-1], Ms[-1] + 1


DE = _direct_edge()
PE = _plan_edge()
CHAIN_M = [4, 5, 7, 9, 13, 24, DE[0], DE[1], 255, 256, 257, 319, 320, 511, 512]
LONG_M = [513, 777, 1024]
BAND_M = [4, 5, 6, 7, 12, 13, 14, 19, 20, 26, 27, 45, 128, 129, 256, 257, PE[0], PE[1], 480, 512]
DENSE_M = [8, 45, 60, 61, 64, 65, 129, 300, 512, 513]
LLE_DENSE_M = [8, 45, 64, 65, 128, 129, 300, 512, 513]


def _c(family, route, M, regime, prec=1, **kw):
    return dict(family=family, route=route, M=M, regime=regime, prec=prec, **kw)


def cases():
    cs = []
    for M in CHAIN_M:
        cs.append(_c("chain", "chain", M, "typical"))
        if M >= 7:
            cs.append(_c("chain", "chain", M, "p1zero"))
            cs.append(_c("chain", "chain", M, "priors"))
    for M in (45, 256):
        cs.append(_c("chain", "chain", M, "single"))
        cs.append(_c("chain", "chain", M, "tiny_c"))
        cs.append(_c("chain", "chain", M, "big_c"))
        cs.append(_c("chain", "chain", M, "typical", prec=0))
        cs.append(_c("chain", "chain", M, "coincident"))
    for M in LONG_M:
        cs.append(_c("chain", "long", M, "typical"))          # (M >= 513: a quad solve of 10 - 20 s each on the CPU -- typical sums only, and one p1zero)
    cs.append(_c("chain", "long", 777, "p1zero"))
    for M in BAND_M:
        cs.append(_c("band", "band", M, "typical"))
        if M >= 12 and M not in PE:
            cs.append(_c("band", "band", M, "p1zero"))
    for M in (45, 257):
        cs.append(_c("band", "band", M, "shifted_h"))
        cs.append(_c("band", "band", M, "priors"))
        cs.append(_c("band", "band", M, "typical", prec=0))
    cs.append(_c("band", "band", 300, "priors"))             # (a prior on node 0 and none on node 256: the second round of the node loop has something to confuse)
    for M in DENSE_M:
        cs.append(_c("dense", "dense", M, "typical"))
        cs.append(_c("dense", "dense", M, "p1zero"))
    for M in (45, 129):
        cs.append(_c("dense", "dense", M, "priors"))
        cs.append(_c("dense", "dense", M, "dense_c"))
        cs.append(_c("dense", "dense", M, "typical", prec=0))
        cs.append(_c("dense", "lambda0", M, "lambda0"))
    for M in LLE_DENSE_M:
        cs.append(_c("dense", "lle_dense", M, "typical"))
    for M in (45, 129):
        cs.append(_c("dense", "lle_dense", M, "shifted_h"))
        cs.append(_c("dense", "lle_dense", M, "coincident"))
    return cs


def short_beta(M):
    """k of beta = k h for a short-beta cell of M nodes (h: the chain's mean node spacing, params_of)."""
    return 1.0 if M <= 300 else 0.7


def _s(route, M, regime, prec=1):
    return _c("dense", route, M, regime, prec, beta_h=short_beta(M))


def short_beta_cases():
    """The dense eliminations at beta = k h: the smallest and largest M of every kernel's range (see the comment above DROPPED)."""
    cs = []
    for M in (129, 300, 512, 513):
        cs.append(_s("dense", M, "typical"))
        cs.append(_s("dense", M, "p1zero"))
    cs.append(_s("dense", 129, "priors"))
    cs.append(_s("dense", 129, "dense_c"))
    cs.append(_s("dense", 129, "typical", prec=0))
    for M in LLE_DENSE_M:
        if M != 8:                                            # (8 nodes: no row is ever swapped, see the comment above DROPPED)
            cs.append(_s("lle_dense", M, "typical"))
    for M in (45, 129):
        cs.append(_s("lle_dense", M, "shifted_h"))
    cs.append(_s("lle_dense", 129, "typical", prec=0))
    return cs


# What is held where.  A cell is held when tests/test_mstep_ref.py shows on the CPU that its gate contains the fp64 restatement and is at most 1/10 of
# what rounding the sums to fp32 changes ("slip"); the ratios below are that run's.
#
# At the launch file's beta (0.35; pre-processing: 3) on chains whose nodes are 0.02 m apart G is nearly singular, |G| |W| / |V| reaches 1e5 - 1e9, and
# the dense gate, which carries that amplification, is wider than a slip.  DROPPED takes those cells out:
#   * (the band is no longer here.  Its FORWARD gate is wider than an fp32 slip from 256 nodes on -- gate / slip 1.3 at 257 nodes, 3e5 at 480, at any
#     beta -- because the forward error of the state system grows with the chain and with H's entries; part of what was read as the band's own error
#     was the quad reference's: under the oracle's H at 256 / 257 nodes (entries up to 9e10) mstep_ref.reference is 1e-12 - 2e-11 m from the system's
#     answer at 256 bits.  The band solves (c G^-1 + D + g H) V = B as an SPD banded L D L^T, and such a solve promises a small BACKWARD error at any
#     condition number: mstep_ref.band_backward_error, the longdouble residual of the state system at the returned T with f' rebuilt from f, against
#     EPS_BAND u |A2| |x| + EPS_B u |B|'s terms + the read-back u |T|, times SAFETY.  Band cells above 129 nodes (by_backward_error) are held by it alone,
#     sigma2 at the kernel's own T (mstep_ref.held_at_T); up to 129 nodes it is asserted beside the forward gate.  tests/test_mstep_ref.py, per cell --
#     fp64 restatement / tolerance (<= 0.25 asked), answer of the fp32-rounded sums / tolerance (>= 10 asked), T* at 256 bits / tolerance (<= 0.25):
#         256 typical 0.075, 2.2e4, 0.078   p1zero 0.083, 2.2e4, 0.066       257 typical 0.095, 1.5e4, 0.095   p1zero 0.072, 1.9e4, 0.069
#         257 shifted_h 0.092, 820, 0.092   priors 0.072, 1.5e4, 0.070       257 typical fp32 mode 0.084, 2.1e4, 0.084     300 priors 0.074, 2.0e4, -
#         474 typical 0.13, 1.7e4, -        475 typical 0.077, 1.9e4, -      480 typical 0.17, 2.5e4, -        p1zero 0.19, 1.3e4, -
#         512 typical 0.086, 2.5e4, 0.072   p1zero 0.17, 2.5e4, -            (T* at 256 bits: every cell up to 257 nodes and one of 512)
#     the kernel's own data flow (records, tile, both ends) 0.052 - 0.10 at 45 / 257 / 474 / 512; the 4 - 129 node cells 0.006 - 0.078 and 745 - 1.3e6.
#     T* without the LLE term stands at 3.5e8 - 1.1e12 tolerances, without the priors at 1.9e11 - 4.5e11, at the launch file's beta at 3.3e11 - 1.4e13;
#     node m - 256's P1, R, priors or H Y0 read at node m (the second round of the kernel's node loop) at 170 - 9e11 wherever it changes a value (at
#     257 nodes only node 256 is in that round, and it shares P1 = R = 0 with node 0 in the P1-zeroed cell and the prior's offset in the priors cell:
#     band-M300-priors is there for the priors).  All of them with the oracle's own H, made symmetric bit for bit (build_case); 474 / 475 are the two
#     sides of BandPlan's edge (both ends / one direction again: the records of two directions no longer fit the LDS).  Nothing of the band is left out.)
#   * dense eliminations without the LLE term from 129 nodes on (k_mstep_mcu at 129 / 300 / 512, k_mstep<1wg> at 513) and at lambda sigma2 = 1e-7: the
#     dense gate carries |G| |A^-1| |A| |W| and the fp64 chain coordinate's worst-case running-sum error through G W; it is 0.2 - 5 (129 - 513 nodes),
#     3e4 - 6e5 (lambda sigma2 = 1e-7) of an fp32 slip.  At that beta k_mstep_mcu is held at 61 - 65 nodes, k_mstep_fast<MFMA> up to 60.
#   * every dense LLE cell at beta = 3 (k_mstep_fast<pivoted>, k_mstep<LDS>, k_mstep_pivot_mcu, k_mstep<1wg> with the LLE term; the TDLO_MSTEP_LLE=1wg
#     comparator for the same reason): W is 1e5 - 1e9 times larger than V = G W, and the gate is 3e5 - 7e21 of an fp32 slip (7.8e6 at 45 nodes, 1.6e8
#     at 129).  Their routes are still asserted (the hand-over tests below) and the band's hand-over cases are held to the dense gate, which
#     contains their restatement.
#
# The same kernels are held at a short beta instead (short_beta_cases: the key beta_h = k, beta = k h, h = chain_coord(Y0)[-1] / (M - 1) in fp64, handed
# to the reference and to the library alike; k = 1.0 up to 300 nodes, 0.7 from 512 on -- at 1.0 the 512 / 513 cells stand at 0.18 - 0.27).  Scenes, sums
# and gate are those of the cells above; only G is well conditioned.  Smallest and largest M of every kernel's range; gate / slip, then the fp64
# restatement / gate, then the rows partial pivoting swaps:
#     dense (no LLE term)   k_mstep_mcu   129 typical 7.8e-3, 1.1e-4, -      p1zero 8.8e-3, 7.7e-3, 14    priors 8.9e-3, 3.1e-4    dense_c 8.8e-3, 2.3e-4
#                                         129 typical, fp32 mode 1.4e-2, 4.2e-4
#                                         300 typical 8.3e-2, 1.4e-4, -      p1zero 7.7e-2, 2.8e-4, 20
#                                         512 typical 6.1e-2, 3.6e-4, -      p1zero 5.3e-2, 9.6e-3, 12
#                           k_mstep<1wg>  513 typical 4.1e-2, 1.4e-4, -      p1zero 4.7e-2, 5.2e-3, 10
#     lle_dense   k_mstep_fast<pivoted>   45 typical 8.5e-4, 3.0e-4, 5       shifted_h 8.5e-4, < 1e-4, 5      64 typical 2.4e-3, 4.9e-4, 6
#                 k_mstep<LDS>            65 typical 3.0e-3, 9.8e-4, 2       128 typical 1.2e-2, 1.9e-4, 4
#                 k_mstep_pivot_mcu       129 typical 8.8e-3, 1.7e-4, 5      shifted_h 8.8e-3, 8.6e-4, 5      fp32 mode 1.6e-2, 3.5e-4, 8
#                                         300 typical 9.5e-2, 3.4e-4, 13     512 typical (uniform_H) 6.3e-2, 4.2e-4
#                 k_mstep<1wg>            513 typical (uniform_H) 4.1e-2, 7.3e-4
#   The CPU file also shows for each of them that T* moves by >= 100 gates without the LLE term (3.7e4 - 7.4e8), without the priors (1.3e9) and at the
#   launch file's beta (5e4 - 5.6e9).  The stopping decision is pinned on lle_dense 45 / 100 / 129 and dense 129 (DEC: crit's gate is 7e-11 - 2e-9 of
#   crit); k_mstep_big and the TDLO_MSTEP_LLE=1wg comparator are held at 129 and 300 nodes (CHILD).
#   From 512 nodes on the LLE cells take uniform_H: the oracle's H has entries up to 6.6e18 there (tests/test_mstep_ref.py asserts > 1e12).
#   Left out of the short-beta list: lle_dense M8 typical -- gate / slip 2.0e-4 / 6.1e-5 / 3.1e-5 and restatement / gate 5.7e-4 / 3.8e-3 / 5.6e-2 at
#   k = 1.0 / 0.7 / 0.5, but partial pivoting swaps 0 rows of its 8 x 8 system at every k, so it does not meet the CPU file's pivoting condition.
#   Still out at any beta: the LLE cells with P1 zeroed (condition number 1e6: the restatement sits at 0.12 - 1.16 of the gate, gate / slip up to 1.65)
#   and the coincident LLE cells (gate 1e4 slips).
DROPPED = {
    "dense-M129-typical-f64", "dense-M129-p1zero-f64", "dense-M300-typical-f64", "dense-M300-p1zero-f64", "dense-M512-typical-f64",
    "dense-M512-p1zero-f64", "dense-M513-typical-f64", "dense-M513-p1zero-f64", "dense-M45-dense_c-f64", "dense-M129-priors-f64",
    "dense-M129-dense_c-f64", "dense-M129-typical-f32",
    "lle_dense-M8-typical-f64", "lle_dense-M45-typical-f64", "lle_dense-M64-typical-f64", "lle_dense-M65-typical-f64", "lle_dense-M128-typical-f64",
    "lle_dense-M129-typical-f64", "lle_dense-M300-typical-f64", "lle_dense-M512-typical-f64", "lle_dense-M513-typical-f64",
    "lle_dense-M45-shifted_h-f64", "lle_dense-M45-coincident-f64", "lle_dense-M129-shifted_h-f64", "lle_dense-M129-coincident-f64",
}
ALL_CASES = cases()
CASES = [c for c in ALL_CASES if f"{c['route']}-M{c['M']}-{c['regime']}-{'f64' if c['prec'] else 'f32'}" not in DROPPED] + short_beta_cases()


def by_backward_error(case):
    """The band cells above 129 nodes: held by mstep_ref.band_backward_error alone (their forward gate is wider than an fp32 slip, see above)."""
    return case["family"] == "band" and case["M"] > 129


def cid(c):
    bh = f"-bh{c['beta_h']}" if c.get("beta_h") else ""
    return f"{c['route']}-M{c['M']}-{c['regime']}{bh}-{'f64' if c['prec'] else 'f32'}"


def expected_kernel(route, M):
    """mstep_kernel_name (tdlo_device.hip) for the route a case forces."""
    if route == "chain":
        return "k_mstep_chain"
    if route == "long":
        return "k_mstep_chain_long"
    if route == "band":
        return "k_mstep_band"
    if route in ("dense", "lambda0"):
        return "k_mstep_fast<MFMA>" if M <= 60 else ("k_mstep<1wg>" if M > 512 else "k_mstep_mcu")
    return "k_mstep_fast<pivoted>" if M <= 64 else ("k_mstep<LDS>" if M <= 128 else ("k_mstep<1wg>" if M > 512 else "k_mstep_pivot_mcu"))


# ---- scenes and sums ----------------------------------------------------------------------------------------------------------------------
def scene(M, cfg, scale=1.0, coincident=False):
    """synth.scene on a 2^-20 m grid with the nodes' centroid exactly 0 (fp32 mode reads the fp32 node copy: the centring and the coordinates are
    then exact in fp32 and the test does not measure their rounding).  scale stretches the chain (the resolution check wants >= 3 m)."""
    from trackdlo_amd import synth
    N0 = max(600, 16 * M)
    X, Y0, _ = synth.scene(N0, M, config=cfg)
    X = np.array(X, dtype=np.float64) * scale; Y0 = np.array(Y0, dtype=np.float64) * scale
    if coincident:
        Y0[M // 3 + 1] = Y0[M // 3]
    c = Y0.mean(axis=0)
    g = 2.0 ** 20
    Y0 = np.round((Y0 - c) * g) / g
    k = M // 2 if not coincident or M // 2 not in (M // 3, M // 3 + 1) else M - 1
    Y0[k] -= np.round(Y0.sum(axis=0) * g) / g
    assert (Y0.sum(axis=0) == 0).all() and (Y0.astype(np.float32) == Y0).all()
    X = np.asfortranarray((X - c).astype(np.float32).astype(np.float64))
    return X, Y0


_SCENES = {}


def case_scene(case):
    """(X, Y0) of a cell as the library and the reference get them (shifted_h: 12 m from the origin), then as the E-step reference gets them."""
    key = (case["M"], case["prec"], case["regime"] == "coincident", case["regime"] == "shifted_h")
    if key not in _SCENES:
        X, Y0 = scene(case["M"], 800 + case["M"] + (1000 if case["prec"] == 0 else 0), coincident=key[2])
        _SCENES[key] = (np.asfortranarray(X + SHIFT), Y0 + SHIFT, X, Y0) if key[3] else (X, Y0, X, Y0)      # (the sums are translation-invariant)
    return _SCENES[key]


def params_of(case):
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    lle = case["route"] in ("band", "lle_dense")
    lam = {"tiny_c": 1e-4, "dense_c": 0.1, "big_c": 5e4, "lambda0": 0.0}.get(case["regime"], P["lambda_pre_proc"] if lle else P["lambda_"])
    beta = P["beta_pre_proc"] if lle else P["beta"]
    if case.get("beta_h"):                                                                # beta = k h, h the mean node spacing of the Y0 both sides get
        beta = case["beta_h"] * float(R.chain_coord(case_scene(case)[1])[-1]) / (case["M"] - 1)
    s2 = {"tiny_c": 1e-6, "dense_c": 1e-6, "big_c": 2e-4}.get(case["regime"], 2e-5 if lle else 1e-4)
    return dict(beta=beta, lambda_=lam, alpha=P["alpha"], lle_weight=P["lle_weight"], mu=P["mu"], lle=lle, s2=s2)


def junctions(M):
    j1, j2, j3, _, _ = cn.carve(M)
    return sorted({0, j1, max(j2 - 1, 0), j2, j3, M - 1})


def lle_H(Y0, regime):
    from oracle import ref_cpu
    M = len(Y0)
    L = ref_cpu.calc_lle_weights(Y0, 6)
    H = (np.eye(M) - L).T @ (np.eye(M) - L)
    if regime == "shifted_h":
        H = H + 0.05 * np.eye(M) + 0.01 * (np.eye(M, k=1) + np.eye(M, k=-1))      # rows no longer sum to zero (still banded and symmetric)
    return H


def uniform_H(M, k=6):
    """(I - L)^T (I - L) with L giving each node's k nearest chain neighbours the weight 1 / k (a window of k + 1 nodes, shifted inwards at the ends):
    an LLE regulariser with bounded entries for the chains of 512 nodes and more, where calc_lle_weights on a straight chain does not give one
    (tests/test_mstep_ref.py: test_the_oracles_H_at_512_nodes_is_unbounded).  The M-step takes H as an input."""
    L = np.zeros((M, M))
    for i in range(M):
        lo = min(max(i - k // 2, 0), M - 1 - k)
        L[i, [j for j in range(lo, lo + k + 1) if j != i]] = 1.0 / k
    return (np.eye(M) - L).T @ (np.eye(M) - L)


_BUILT = {}
_ESTEP = {}


def build_case(case, with_scene=False):
    """(mstep_ref.Case, X, Y0 handed to the library, priors handed to the library)."""
    key = cid(case)
    if key not in _BUILT:
        M = case["M"]; p = params_of(case)
        Xl, Yl, X, Y0 = case_scene(case)
        ks = (M, case["prec"], case["regime"] == "coincident", p["mu"])                                                       # (the short-beta cells share the scenes, and so the sums)
        if ks not in _ESTEP:
            _ESTEP[ks] = R.estep(X, Y0, Y0, 1e-4, mu=p["mu"])["sums"]
        s = _ESTEP[ks].copy()
        P1 = s[:M]; Rm = s[M:4 * M].reshape(3, M).T.copy()
        reg = case["regime"]
        if reg == "p1zero":
            z = junctions(M)
            j2 = cn.carve(M)[1]
            if M >= 12:                                                                  # (shorter chains: the junctions alone leave few nodes observed)
                z += list(range(max(j2 - 2, 0), min(j2 + 3, M)))                        # a run of unobserved nodes across j2
            P1[z] = 0; Rm[z] = 0
        elif reg == "single":
            keep = M // 3
            m = np.ones(M, dtype=bool); m[keep] = False
            P1[m] = 0; Rm[m] = 0
        elif reg == "lambda0":
            P1[M // 2] = 0; Rm[M // 2] = 0                                               # one unobserved node: A's row is exactly zero
        if reg in ("typical", "p1zero", "priors") and M >= 8 and case["family"] == "chain" and M % 3 == 0:
            P1[: M // 4] *= LD(1e-10); Rm[: M // 4] *= LD(1e-10)                         # P1 over fourteen decades on one chain
        s[:M] = P1; s[M:4 * M] = Rm.T.reshape(-1)
        priors = None
        if reg == "priors":
            idx = junctions(M)
            rows = [[i, *(Y0[i] + 0.003)] for i in idx] + [[idx[1], *(Y0[idx[1]] - 0.002)]]      # two priors on one node: the last one wins
            priors = np.array(rows, dtype=np.float64)
            if M >= 7:
                P1[idx[1]] = 0; Rm[idx[1]] = 0                                         # a prior where no point is
                s[:M] = P1; s[M:4 * M] = Rm.T.reshape(-1)
        H = (uniform_H(M) if case.get("beta_h") and M >= 512 else lle_H(Y0, reg)) if p["lle"] else None
        if by_backward_error(case):
            # prepare_frame gives an H_override to the banded solve only if it is symmetric bit for bit; the product (I - L)^T (I - L) as BLAS forms it
            # is so on one machine and not on the next (entries up to 1e15 here): a + b == b + a makes it so everywhere, for both sides alike
            H = 0.5 * (H + H.T)
        c = MR.Case(s, Yl, Yl, p["s2"], beta=p["beta"], lambda_=p["lambda_"], alpha=p["alpha"] if priors is not None else 0.0, priors=None
                    if priors is None else np.column_stack([priors[:, 0], priors[:, 1:] + (SHIFT if reg == "shifted_h" else 0)]),
                    lle_weight=p["lle_weight"] if p["lle"] else 0.0, H=H)
        _BUILT[key] = (c, np.asfortranarray(Xl), Yl, c.priors)
    c, X, Y0, pr = _BUILT[key]
    return (c, X, Y0, pr) if with_scene else c


# ---- driving the kernels ----------------------------------------------------------------------------------------------------------------------
def make_params(case, max_iter=10, tol=0.0):
    from trackdlo_amd import binding as B
    p = params_of(case)
    return B.make_params(p["beta"], p["lambda_"], p["lle_weight"], p["mu"], max_iter, tol, p["lle"], p["alpha"], 0.0, 0.008, case["prec"])


def run_mstep(ctx, X, Y0, s2, prm, sums, priors=None, H=None, then_estep=False):
    """begin -> set_global -> estep -> mstep(sums) [-> estep] -> end: (rc, done flag, end() dict or None, next E-step's sums or None)."""
    from trackdlo_amd import binding as B, nsplit
    sh = nsplit.HipShard(ctx, X)
    init = sh.begin(Y0, s2, prm, priors, None, H)
    sh.set_global(init[0], init[1])
    sh.estep(None)
    done = sh.mstep(np.asarray(sums, dtype=np.float64))
    nxt = sh.estep(None) if then_estep and not done else None
    try:
        o = sh.end()
        return 0, done, o, nxt
    except B.TdloError as e:
        return e.code, done, None, nxt


def set_route(route):
    from trackdlo_amd import binding as B
    B.mstep_dense(route in ("dense",))
    B.mstep_lle_dense(route in ("lle_dense",))


@pytest.fixture(scope="module")
def ctx():
    from trackdlo_amd import binding as B
    c = B.Context(device=0, timing=False, max_points=16 * 1024, max_nodes=1024)
    yield c
    B.mstep_dense(False); B.mstep_lle_dense(False)
    c.close()


WORST = {}


def _report():
    for k, (qt, qs) in sorted(WORST.items()):
        what = "backward error / tolerance" if k.endswith(" backward") else "|dT| / gate"
        print(f"  {k}: worst {what} {qt:.3g}, |d sigma2| / gate {qs:.3g}")


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_mstep_from_sums_against_the_quad_solve(ctx, case):
    from trackdlo_amd import binding as B
    c, X, Y0, priors = build_case(case, with_scene=True)
    set_route(case["route"])
    rc, done, o, _ = run_mstep(ctx, X, Y0, c.s2, make_params(case, max_iter=1), c.sums, priors, c.H)
    name = ctx.profile_iteration(1)[3]
    assert name == expected_kernel(case["route"], case["M"]), (cid(case), name)
    if case["route"] == "lambda0":
        # one unobserved node with lambda = 0: A's row is exactly zero -- no fp64 answer; every dense kernel refuses
        assert rc == B.TDLO_E_NUMERIC, (cid(case), rc, name)
        return
    assert rc == 0 and done, (cid(case), rc, done)
    assert o["iters"] == 1 and o["converged"] is False                  # max_iter = 1: done, not converged
    Tk = np.asarray(o["Y"])
    k = f"{name} {'f64' if case['prec'] else 'f32'}"
    if case["family"] == "band":
        # the banded solve by its backward error, every chain length; sigma2 at the kernel's own T (the plan on both sides of its edge)
        if case["M"] in PE:
            assert bn.band_plan(case["M"])["tw"] == (1 if case["M"] == PE[0] else 0) and bn.band_plan(case["M"])["lds_bytes"] > 64 * 1024
        qb, where = MR.band_backward_error(c, Tk)
        s2k, gSk, _, _ = MR.held_at_T(c, Tk)
        qsk = abs(o["sigma2"] - float(s2k)) / gSk
        a, b = WORST.get(k + " backward", (0.0, 0.0)); WORST[k + " backward"] = (max(a, qb), max(b, qsk))
        print(f"{cid(case)} -> {name}: backward error / tolerance {qb:.3g} at node {where[0]} coordinate {where[1]}, |d sigma2| / gate at its own T {qsk:.3g}")
        assert qb <= 1.0, (cid(case), qb, where)
        assert qsk <= 1.0, (cid(case), qsk)
        if by_backward_error(case):
            return
    T, s2, _ = MR.reference(c)
    gT, gS, _ = MR.gate(c, case["family"], T)
    dT = np.abs(Tk - T.astype(np.float64))
    qt = float((dT / gT).max()); qs = abs(o["sigma2"] - float(s2)) / gS
    a, b = WORST.get(k, (0.0, 0.0)); WORST[k] = (max(a, qt), max(b, qs))
    print(f"{cid(case)} -> {name}: |dT| / gate {qt:.3g} (max |dT| {dT.max():.3g} m), |d sigma2| / gate {qs:.3g}")
    assert qt <= 1.0, (cid(case), qt)
    assert qs <= 1.0, (cid(case), qs)


# ---- decisions --------------------------------------------------------------------------------------------------------------------------------
DEC = [_c("chain", "chain", 45, "typical"), _c("chain", "long", 513, "typical"), _c("band", "band", 45, "typical"), _c("dense", "dense", 45, "typical")]
# (the dense LLE eliminations at the pre-processing beta are not here: their gate on crit is half of crit itself -- see DROPPED; at beta = h it is
# 1e-9 - 1e-11 of crit: k_mstep_fast<pivoted>, k_mstep<LDS>, k_mstep_pivot_mcu and k_mstep_mcu)
DEC += [_s("lle_dense", 45, "typical"), _s("lle_dense", 100, "typical"), _s("lle_dense", 129, "typical"), _s("dense", 129, "typical")]


@pytest.mark.parametrize("case", DEC, ids=cid)
def test_stopping_decision_and_refusals(ctx, case):
    """tol at crit* (1 +- 1e-6) -- far above crit's gate -- gives done exactly as the reference; an exact sigma2 < 0 (Q lowered) and N_p = 0 (every P1
    zero) end in TDLO_E_NUMERIC from end()."""
    from trackdlo_amd import binding as B
    c, X, Y0, priors = build_case(case, with_scene=True)
    set_route(case["route"])
    T, s2, crit = MR.reference(c)
    _, _, gC = MR.gate(c, case["family"], T)
    assert gC < 1e-7 * float(crit)
    for f, want in ((1 + 1e-6, True), (1 - 1e-6, False)):
        tol = float(crit) * f
        rc, done, o, _ = run_mstep(ctx, X, Y0, c.s2, make_params(case, max_iter=10, tol=tol), c.sums, priors, c.H)
        assert MR.decision(float(crit), 1, tol, 10) == (want, True)
        assert done == want, (cid(case), f, done)
        if want:
            assert rc == 0 and o["iters"] == 1 and o["converged"] is True
    # sigma2 < 0: Q below what the residual form subtracts
    M = c.M
    d = T - c.y.astype(LD)
    Rm = c.sums[M:4 * M].reshape(3, M).T; P1 = c.sums[:M]
    q0 = LD(2) * (d * Rm).sum() - (P1[:, None] * d * d).sum()                          # Q at which sigma2 = 0
    bad = c.sums.copy(); bad[4 * M] = q0 - LD(0.5) * abs(c.sums[4 * M] - q0)
    rc, _, _, _ = run_mstep(ctx, X, Y0, c.s2, make_params(case, max_iter=1), bad, priors, c.H)
    assert rc == B.TDLO_E_NUMERIC, (cid(case), "sigma2 < 0", rc)
    empty = c.sums.copy(); empty[:4 * M] = 0
    rc, _, _, _ = run_mstep(ctx, X, Y0, c.s2, make_params(case, max_iter=1), empty, priors, c.H)
    assert rc == B.TDLO_E_NUMERIC, (cid(case), "N_p = 0", rc)


@pytest.mark.parametrize("M", [257, 512])
def test_band_stopping_decision_at_its_own_T(ctx, M):
    """The band above 129 nodes has no forward gate on crit: one M-step with tol = 0 gives the kernel's T, crit follows from it in longdouble
    (mstep_ref.held_at_T; its own-rounding gate is far below 1e-6 crit), and tol at that crit (1 +- 1e-6) must give done / converged exactly as
    mstep_ref.decision.  257 nodes: an exact sigma2 < 0 and N_p = 0 end in TDLO_E_NUMERIC."""
    from trackdlo_amd import binding as B
    case = _c("band", "band", M, "typical")
    c, X, Y0, priors = build_case(case, with_scene=True)
    set_route("band")
    rc, done, o, _ = run_mstep(ctx, X, Y0, c.s2, make_params(case, max_iter=10, tol=0.0), c.sums, priors, c.H)
    assert rc == 0 and not done and ctx.profile_iteration(1)[3] == "k_mstep_band"
    Tk = np.asarray(o["Y"])
    _, _, crit, gC = MR.held_at_T(c, Tk)
    print(f"{cid(case)}: crit {float(crit):.6g}, its gate / crit {gC / float(crit):.3g}")
    assert gC < 1e-7 * float(crit)
    for f, want in ((1 + 1e-6, True), (1 - 1e-6, False)):
        tol = float(crit) * f
        rc, done, o2, _ = run_mstep(ctx, X, Y0, c.s2, make_params(case, max_iter=10, tol=tol), c.sums, priors, c.H)
        assert MR.decision(float(crit), 1, tol, 10) == (want, True)
        assert done == want, (cid(case), f, done)
        assert np.array_equal(np.asarray(o2["Y"]), Tk)                  # (the same M-step: crit is this T's)
        if want:
            assert rc == 0 and o2["iters"] == 1 and o2["converged"] is True
    if M != 257:
        return
    d = Tk.astype(LD) - c.y.astype(LD)
    Rm = c.sums[M:4 * M].reshape(3, M).T; P1 = c.sums[:M]
    q0 = LD(2) * (d * Rm).sum() - (P1[:, None] * d * d).sum()                          # Q at which sigma2 = 0 at this T
    bad = c.sums.copy(); bad[4 * M] = q0 - LD(0.5) * abs(c.sums[4 * M] - q0)
    rc, _, _, _ = run_mstep(ctx, X, Y0, c.s2, make_params(case, max_iter=1), bad, priors, c.H)
    assert rc == B.TDLO_E_NUMERIC, (cid(case), "sigma2 < 0", rc)
    empty = c.sums.copy(); empty[:4 * M] = 0
    rc, _, _, _ = run_mstep(ctx, X, Y0, c.s2, make_params(case, max_iter=1), empty, priors, c.H)
    assert rc == B.TDLO_E_NUMERIC, (cid(case), "N_p = 0", rc)


HANDOVER_BAND = ["big_s2", "close"]


def band_handover_case(regime):
    """(case, mstep_ref.Case, X, Y0, priors): the band's M = 45 scene with sigma2 = 50 m2 (above band_s2_max) or two nodes 10 um apart (below the gap bound)."""
    M = 45
    case = _c("dense", "band", M, "typical")
    c, X, Y0, priors = build_case(case, with_scene=True)
    if regime == "big_s2":
        c = MR.Case(c.sums, c.Y0, c.y, 50.0, **c.kw())
    else:
        Y0 = Y0.copy(); Y0[M // 2 + 1] = Y0[M // 2] + 1e-5
        c = MR.Case(c.sums, Y0, Y0, c.s2, **dict(c.kw(), H=lle_H(Y0, "typical")))
    return case, c, X, Y0, priors


@pytest.mark.parametrize("regime", HANDOVER_BAND)
def test_band_hands_over_to_the_dense_kernels(ctx, regime):
    """A registration whose sigma2 is above band_s2_max (prepare_frame, fp64) or whose nodes are closer than the gap bound takes the dense pivoted
    kernels -- and is held to the dense gate there (tests/test_mstep_ref.py: the restatement inside it; the dense LLE gate is not sharp, see DROPPED)."""
    case, c, X, Y0, priors = band_handover_case(regime)
    set_route("band")
    rc, done, o, _ = run_mstep(ctx, X, Y0, c.s2, make_params(case, max_iter=1), c.sums, priors, c.H)
    name = ctx.profile_iteration(1)[3]
    assert name == "k_mstep_fast<pivoted>", (regime, name)
    assert rc == 0
    T, s2, _ = MR.reference(c)
    gT, gS, _ = MR.gate(c, "dense", T)
    q = float((np.abs(np.asarray(o["Y"]) - T.astype(np.float64)) / gT).max())
    print(f"band {regime}: {name}, |dT| / gate {q:.3g}")
    assert q <= 1.0, (regime, q)


# ---- the hand-over to the next E-step, and its resolution (IterState::sh_boost) ----------------------------------------------------------------
HANDOVER = [("chain", 200, 1), ("chain", 300, 1), ("chain", 200, 0), ("long", 600, 1), ("band", 200, 1), ("band", 300, 1), ("band", 200, 0),
            ("dense", 200, 1), ("dense", 300, 0), ("lle_dense", 200, 1)]


@pytest.mark.parametrize("route,M,prec", HANDOVER, ids=[f"{r}-M{m}-{'f64' if p else 'f32'}" for r, m, p in HANDOVER])
def test_next_estep_starts_from_the_mstep(ctx, route, M, prec):
    """sigma2 = 1 m2 at the start on a chain of >= 3 m (the set-up grants no extra resolution), sums fabricated so that the M-step leaves sigma2 at 1e-4 m2:
    the next E-step's sums must match the reference at the kernel's own (T, sigma2) and, in fp64 mode, carry the resolution set_iter_consts grants at
    that sigma2 -- R x 2^sR integers, not all even (P1 is the control)."""
    import test_estep_sums_gpu as ES
    from trackdlo_amd import binding as B
    case = _c("band" if route in ("band", "lle_dense") else ("dense" if route == "dense" else "chain"), route, M, "typical", prec=prec)
    p = params_of(case)
    X, Y0 = scene(M, 1700 + M)
    assert R.chain_coord(Y0)[-1] >= 3.0
    N0 = len(X)
    r = R.estep(X, Y0, Y0, 1e-4, mu=p["mu"])
    H = lle_H(Y0, "typical") if p["lle"] else None
    c = MR.Case(r["sums"], Y0, Y0, 1.0, beta=p["beta"], lambda_=p["lambda_"], lle_weight=p["lle_weight"] if p["lle"] else 0.0, H=H)
    T, _, _ = MR.reference(c)
    d = T - c.y.astype(LD)
    P1 = c.sums[:M]; Rm = c.sums[M:4 * M].reshape(3, M).T
    s = c.sums.copy()
    s[4 * M] = LD(3) * P1.sum() * LD(1e-4) + LD(2) * (d * Rm).sum() - (P1[:, None] * d * d).sum()        # sigma2_new = 1e-4 (fabricated_move's identity)
    set_route(route)
    prm = make_params(case, max_iter=10)
    rc, done, o, _ = run_mstep(ctx, X, Y0, 1.0, prm, s, None, H)
    assert rc == 0 and not done
    name = ctx.profile_iteration(1)[3]
    assert name == expected_kernel(route, M), name          # (the band: sigma2 = 1 is below band_s2_max for these chains)
    Yk, s2k = np.asarray(o["Y"]), o["sigma2"]
    assert abs(s2k - 1e-4) < 1e-6
    _, _, _, nxt = run_mstep(ctx, X, Y0, 1.0, prm, s, None, H, then_estep=True)
    if prec == 1:       # the resolution sigma2 = 1e-4 is granted is finer than the set-up's at sigma2 = 1: a boost left at the set-up's value shows
        assert ES.shifts(N0, Y0, 1, s2k, False)[1] > ES.shifts(N0, Y0, 1, 1.0, False)[1]
    re = ES.reference(X, Y0, Yk, s2k, prec)
    g = ES.gate(re, prec, N0, Y0)
    w = ES.compare(nxt, re, g, f"{route}-M{M}")
    msg = f"{route} M {M} ({name}) prec {prec}: next E-step worst {w:.3f} of the gate"
    if prec == 1:
        sP, sR, _ = ES.shifts(N0, Y0, 1, s2k, False)
        for lab, v, sh in (("P1", nxt[:M], sP), ("R", nxt[M:4 * M], sR)):
            k = np.ldexp(v, sh)
            assert (k == np.round(k)).all(), (lab, "not integers at 2^-%d" % sh)
            nz = k[k != 0]
            odd = np.mod(nz, 2) != 0
            assert odd.any(), f"{msg}: every {lab} x 2^{sh} is even -- the sums are coarser than the resolution sigma2 = {s2k:.3g} is granted"
        msg += f", R resolved to 2^-{sR}"
    print(msg)


# ---- process-wide switches: in a child process ----------------------------------------------------------------------------------------------------
CHILD = {"big": ("TDLO_MSTEP_BIG", "1wg", [_c("dense", "dense", 61, "typical"), _c("dense", "dense", 129, "typical"), _s("dense", 129, "typical"),
                 _s("dense", 300, "typical")], "k_mstep_big"),
         "lle1wg": ("TDLO_MSTEP_LLE", "1wg", [_s("lle_dense", 129, "typical"), _s("lle_dense", 300, "typical")], "k_mstep<1wg>")}


def _child(which, out):
    from trackdlo_amd import binding as B
    ctx = B.Context(device=0, timing=False, max_points=16 * 1024, max_nodes=1024)
    res = {}
    try:
        for i, case in enumerate(CHILD[which][2]):
            c, X, Y0, priors = build_case(case, with_scene=True)
            set_route(case["route"])
            rc, done, o, _ = run_mstep(ctx, X, Y0, c.s2, make_params(case, max_iter=1), c.sums, priors, c.H)
            res[f"rc{i}"] = np.array([rc]); res[f"name{i}"] = np.array([ctx.profile_iteration(1)[3]])
            if rc == 0:
                res[f"Y{i}"] = np.asarray(o["Y"]); res[f"s{i}"] = np.array([o["sigma2"]])
    finally:
        ctx.close()
    np.savez(out, **res)


@pytest.mark.parametrize("which", sorted(CHILD))
def test_process_wide_switches(tmp_path, which):
    env_key, env_val, cs, kname = CHILD[which]
    out = str(tmp_path / "m.npz")
    e = dict(os.environ, **{env_key: env_val})
    code = f"import sys; sys.path[:0] = [{HERE!r}, {os.path.dirname(HERE)!r}]; import test_mstep_sums_gpu as t; t._child({which!r}, {out!r})"
    p = subprocess.run([sys.executable, "-c", code], env=e, cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    z = np.load(out)
    for i, case in enumerate(cs):
        assert int(z[f"rc{i}"][0]) == 0, (which, cid(case))
        assert str(z[f"name{i}"][0]) == kname, (which, cid(case), z[f"name{i}"][0])
        c = build_case(case)
        T, s2, _ = MR.reference(c)
        gT, gS, _ = MR.gate(c, "dense", T)
        q = float((np.abs(z[f"Y{i}"] - T.astype(np.float64)) / gT).max()); qs = abs(float(z[f"s{i}"][0]) - float(s2)) / gS
        print(f"{which} {cid(case)} ({z[f'name{i}'][0]}): |dT| / gate {q:.3g}, |d sigma2| / gate {qs:.3g}")
        k = f"{kname} ({env_key}={env_val}) {'f64' if case['prec'] else 'f32'}"
        a, b = WORST.get(k, (0.0, 0.0)); WORST[k] = (max(a, q), max(b, qs))
        assert q <= 1.0 and qs <= 1.0, (which, cid(case), q, qs)


def test_zz_worst_per_kernel():
    _report()
