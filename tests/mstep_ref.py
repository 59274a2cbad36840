"""One M-step of trackdlo::cpd_lle from given sums, solved in quad precision, and the gate its kernels are held to (tests only).

The sums are the N-split's layout [P1 | R = PX - P1 y (3 x M, column-major) | Q | N_kept] (tests/estep_ref.py).  `reference` runs
estep_ref.mstep with exact=True: the distances along the chain come from estep_ref.chain_gaps_exact (relative error ~1e-19 -- the fp64
running sum's absolute 1e-16 m would come back amplified by |G| |W| / |V|, up to 1e6 for the LLE systems), G, A = P1 G + lambda sigma2 I
(+ alpha J G + sigma2 w H G) and B = R + P1 (y - Y0) (+ alpha (Y_ext - Y0) - sigma2 w H Y0) are formed in longdouble from them and the fp64
inputs, and A W = B is solved by oracle.solve_extended (__float128 LU with refinement) followed by two more refinement steps whose residuals
are formed in longdouble.  T* = Y0 + G W then carries the longdouble forming of G and A amplified by the same |G| |W| / |V|: ~1e-19 x 1e6
relative to V at worst, three or more decades below the gates it is compared with (tests/test_mstep_ref.py shows the fp64 restatements
inside them).  sigma2 is the residual form in longdouble, crit = sum_m |T_m - y_prev,m| / M, and the decision is
trackdlo.cpp:424-437's.

`gate` is what the kernels' fp64 arithmetic can be off by, per node and coordinate (u = 2^-53), derived below term by term.  It is
checked on the CPU (tests/test_mstep_ref.py) to contain fp64 restatements of the same algorithms (partial-pivot LU for the dense
eliminations, tests/chain_numpy.py, tests/band_numpy.py) and to be at most 1/10 of what rounding the sums to fp32 would change:
neither too tight for honest fp64 arithmetic nor too loose to see one fp32 slip."""
import numpy as np

import estep_ref as R

LD = np.longdouble
U = 2.0 ** -53
SAFETY = 4.0              # the magnitudes |A^-1| below are evaluated in fp64 and the constants are first-order: a factor 4 over them
EPS_G = 8.0               # forming G (trackdlo.cpp:233) from a distance: one division, one exp, one product, one sum (the distance's own error: coord_error)
EPS_B = 8.0               # forming B: R + P1 (y - Y0) [+ alpha (Y_ext - Y0) - sigma2 w H Y0], a few roundings relative to the terms' magnitudes
EPS_CHAIN = 64.0          # chain smoother: per-step roundings of the filter (links Phi / Q / P_inf, a 2 x 2 solve, one smoothing step) -- bounded, they do not
                          # accumulate with M (tdlo_mstep_chain.hip): its backward error relative to c G^-1 + D is a constant number of ulp
EPS_BAND = 64.0           # banded L D L^T: records formed from the state precision K (tdlo_mstep_band.hip) and 13 diagonals of H: a constant number of ulp per entry


def kernel_G(Y0, beta, dtype=np.float64):
    coord = R.chain_coord(Y0)
    dd = np.abs(coord[:, None] - coord[None, :]).astype(dtype)
    b = dtype(beta); r2 = np.sqrt(dtype(2))
    return coord, 1 / (2 * b * 2 * b) * np.exp(-r2 * dd / b) * (2 * dd + r2 * b)


def coord_error(Y0):
    """First-order bound on |coord_i(fp64) - coord_i| for the fp64 running sum of the segment lengths (estep_ref.chain_coord, the kernels' and the
    oracle's chain coordinate): each segment length 4 u relative (difference, squares, sum, sqrt), each addition u relative to the partial sum."""
    coord = R.chain_coord(Y0)
    seg = np.diff(coord)
    return U * np.concatenate([[0.0], np.cumsum(coord[1:] + 4 * seg)])


def solve_quad(A, B):
    """A W = B for longdouble A, B: oracle.solve_extended on the fp64-rounded A, then two refinement steps with residuals in longdouble.  The
    corrections are solved by fp64 LU: a correction needs only a few digits of its own (each step multiplies the error by ~cond(A) u)."""
    import scipy.linalg as sla
    from oracle import ref_cpu
    A = np.asarray(A, dtype=LD); B = np.asarray(B, dtype=LD)
    A64 = A.astype(np.float64)
    W = ref_cpu.solve_extended(A64, B.astype(np.float64)).astype(LD)
    lu = sla.lu_factor(A64)
    for _ in range(2):
        r = B - A @ W
        W = W + sla.lu_solve(lu, r.astype(np.float64)).astype(LD)
    return W


class Case:
    """The inputs of one M-step: sums (longdouble, the kernels' layout), Y0, the current nodes y, the previous nodes yp (criterion), sigma2 and the
    parameters.  y and yp are Y0 for the first M-step of a registration."""

    def __init__(self, sums, Y0, y, s2, *, beta, lambda_, alpha=0.0, priors=None, lle_weight=0.0, H=None, yp=None):
        self.sums = np.asarray(sums, dtype=LD); self.Y0 = np.asarray(Y0, dtype=np.float64); self.y = np.asarray(y, dtype=np.float64)
        self.yp = self.y if yp is None else np.asarray(yp, dtype=np.float64)
        self.s2 = float(s2); self.beta = beta; self.lambda_ = lambda_; self.alpha = alpha
        self.priors = None if priors is None or not len(priors) else np.asarray(priors, dtype=np.float64).reshape(-1, 4)
        self.lle_weight = lle_weight; self.H = H

    @property
    def M(self):
        return len(self.Y0)

    def kw(self):
        return dict(beta=self.beta, lambda_=self.lambda_, alpha=self.alpha, priors=self.priors, lle_weight=self.lle_weight, H=self.H)


def reference(c, solve=solve_quad):
    """(T* longdouble M x 3, sigma2* longdouble, crit* longdouble)."""
    T, s2 = R.mstep(c.sums, c.Y0, c.y, c.s2, solve=solve, exact=True, **c.kw())
    crit = np.sqrt(((T - c.yp.astype(LD)) ** 2).sum(axis=1)).sum() / LD(c.M)
    return T, s2, crit


def closed_form(c):
    """lambda = 0, no priors, no LLE term, every P1 > 0: A = diag(P1) G, so G W = B / P1 and T = Y0 + (R + P1 (y - Y0)) / P1 = y + R / P1 -- no solve."""
    M = c.M
    P1 = c.sums[:M]; Rm = c.sums[M:4 * M].reshape(3, M).T
    assert c.lambda_ == 0 and c.priors is None and c.H is None and (P1 > 0).all()
    return c.y.astype(LD) + Rm / P1[:, None]


def decision(crit, it, tol, max_iter):
    """(done, converged) after M-step number `it` (1-based): trackdlo.cpp:424-437."""
    if crit < tol:
        return True, True
    if it >= max_iter:
        return True, False
    return False, True


def system(c):
    """The pieces the gate needs, in fp64: G, D = P1 + alpha J, the LLE term g H, c = lambda sigma2, A, B."""
    M = c.M
    _, G = kernel_G(c.Y0, c.beta)
    P1 = c.sums[:M].astype(np.float64)
    Rm = c.sums[M:4 * M].reshape(3, M).T.astype(np.float64)
    D = P1.copy()
    B = np.abs(Rm) + np.abs(P1[:, None] * (c.y - c.Y0))        # magnitudes of B's terms
    if c.priors is not None:
        Yext = c.Y0.copy(); J = np.zeros(M)
        for r in c.priors:
            J[int(r[0])] = 1.0; Yext[int(r[0])] = r[1:]
        D = D + c.alpha * J
        B = B + c.alpha * np.abs(Yext - c.Y0)
    g = c.s2 * c.lle_weight if c.H is not None else 0.0
    H = np.zeros((M, M)) if c.H is None else np.asarray(c.H, dtype=np.float64)
    if c.H is not None:
        B = B + g * np.abs(H) @ np.abs(c.Y0)
    cc = c.lambda_ * c.s2
    A = D[:, None] * G + cc * np.eye(M) + g * H @ G
    return G, D, g, H, cc, A, B


def gate(c, kernel, T=None):
    """(per-node-and-coordinate gate on T, gate on sigma2, gate on crit) for `kernel` in {"dense", "chain", "band"}.

    T = Y0 + V, V = G W, A W = B.  A perturbation dA, dB, dG moves V by G A^-1 (dB - dA W) + dG W (first order), i.e.

      dense eliminations (k_mstep_fast / k_mstep / k_mstep_mcu / k_mstep_pivot_mcu / k_mstep_big): the kernel forms G in fp64 from the fp64 chain
        coordinate -- |dG_ij| <= G_ij (2 s dd_ij + EPS_G u), s = sqrt2 / beta (|G'| / G <= 2 s), dd_ij = e_i + e_j + u |c_i - c_j| (coord_error) --, A and B
        in fp64, and solves A W = B by partial-pivot elimination -- backward error gamma_3M |A| per element (3 M u, growth assumed O(1): the safety
        factor) -- then V = G W in fp64 (M products: M u |G| |W|) and T = Y0 + V (u |T|):
          |dT| <= |G| |A^-1| (3M u (|D| |G| + c + g |H| |G|) |W| + (|D| + g |H|) |dG| |W| + EPS_B u |B|) + M u |G| |W| + |dG| |W| + u |T|
      structured solves (k_mstep_chain / k_mstep_chain_long: Kalman filter + RTS smoother; k_mstep_band: banded L D L^T in the chain's state) solve
        (c G^-1 + D + g H) V = B without ever forming W or G: a backward error of EPS u relative to each term -- c G^-1 V = c W, D V, g H V -- and to B:
          |dT| <= |G A^-1| (EPS u (c |W| + |D| |V| + g |H| |V|) + EPS_B u |B|) + u |T|
        (G A^-1 = (c G^-1 + D + g H)^-1).  The band adds the documented eps sigma2 K |x| / P1 term (K's entries ~ 3 beta^4 / h^3 are rounded
        when the records are formed and come back divided by the data term): EPS u lambda sigma2 |K| |V| through |G A^-1|, K the state precision's
        position block.
    sigma2 = (Q - 2 sum d.R + sum P1 |d|^2) / (3 Np), d = T - y:  |d sigma2| <= sum_m |2 (P1 d - R)| / (3 Np) |dT| plus the residual form's own
      rounding ((2 log2 M + 8) u over the magnitudes of its three terms: the kernels sum per thread, per wave, then four waves) plus fast_rcp
      (two Newton steps: 4 u relative).
    crit = sum |T - yp| / M:  |d crit| <= sum_m |dT_m|_2 / M + (log2 M + 8) u crit."""
    M = c.M
    G, D, g, H, cc, A, Bmag = system(c)
    if T is None:
        T = reference(c)[0]
    T64 = np.asarray(T, dtype=np.float64)
    V = T64 - c.Y0
    Ainv = np.linalg.inv(A)
    absT = np.abs(T64)
    if kernel == "dense":
        W = _W(c, G, A)
        aW = np.abs(W); aG = np.abs(G)
        coord = R.chain_coord(c.Y0); e = coord_error(c.Y0)
        dd = e[:, None] + e[None, :] + U * np.abs(coord[:, None] - coord[None, :])
        dG = aG * (2 * np.sqrt(2.0) / c.beta * dd + EPS_G * U)
        dGW = dG @ aW
        dA_W = 3 * M * U * (D[:, None] * (aG @ aW) + cc * aW + g * (np.abs(H) @ (aG @ aW))) + np.abs(D)[:, None] * dGW + g * (np.abs(H) @ dGW)
        gT = aG @ (np.abs(Ainv) @ (dA_W + EPS_B * U * Bmag)) + M * U * (aG @ aW) + dGW + U * absT
    else:
        eps = EPS_CHAIN if kernel == "chain" else EPS_BAND
        W = _W(c, G, A)
        K = np.abs(G @ Ainv)
        terms = cc * np.abs(W) + np.abs(D)[:, None] * np.abs(V) + g * (np.abs(H) @ np.abs(V))
        if kernel == "band":
            terms = terms + c.lambda_ * c.s2 * (_kpos(c) @ np.abs(V))
        gT = K @ (eps * U * terms + EPS_B * U * Bmag) + U * absT
    gT = SAFETY * gT
    # sigma2
    P1 = c.sums[:M].astype(np.float64); Rm = c.sums[M:4 * M].reshape(3, M).T.astype(np.float64); Q = float(c.sums[4 * M])
    d = T64 - c.y
    Np = P1.sum()
    ds_dT = np.abs(2 * (P1[:, None] * d - Rm)) / (3 * Np)
    mag = abs(Q) + 2 * np.abs(d * Rm).sum() + (P1[:, None] * d * d).sum()
    gS = (ds_dT * gT).sum() + (2 * np.log2(max(M, 2)) + 8) * U * mag / (3 * Np) + 4 * U * abs(mag) / (3 * Np)
    crit = np.sqrt(((T64 - c.yp) ** 2).sum(axis=1)).sum() / M
    gC = np.sqrt((gT ** 2).sum(axis=1)).sum() / M + (np.log2(max(M, 2)) + 8) * U * crit
    return gT, gS, gC


def _W(c, G, A):
    """W with A W = B in fp64 (the magnitudes only)."""
    M = c.M
    s = c.sums
    P1 = s[:M]; Rm = s[M:4 * M].reshape(3, M).T
    B = (Rm + P1[:, None] * (c.y.astype(LD) - c.Y0.astype(LD))).astype(np.float64)
    if c.priors is not None:
        Yext = c.Y0.copy()
        for r in c.priors:
            Yext[int(r[0])] = r[1:]
        B = B + c.alpha * (Yext - c.Y0)
    if c.H is not None:
        B = B - c.s2 * c.lle_weight * np.asarray(c.H) @ c.Y0
    return np.linalg.solve(A, B)


def _kpos(c):
    """|K| of the state precision, position-position entries (tests/band_numpy.py state_precision), as an M x M magnitude."""
    import band_numpy as bn
    coord = R.chain_coord(c.Y0)
    dg, off = bn.state_precision(coord, c.beta)
    M = c.M
    K = np.zeros((M, M))
    K[np.arange(M), np.arange(M)] = np.abs(dg[:, 0])
    for i in range(1, M):
        K[i, i - 1] = K[i - 1, i] = np.abs(off[i][0])
    return K
