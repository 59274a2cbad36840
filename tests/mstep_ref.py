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
neither too tight for honest fp64 arithmetic nor too loose to see one fp32 slip.  The banded solve above 129 nodes, where that forward gate is
wider than a slip, is held by `band_backward_error` instead (the residual of the state system at the returned T, in longdouble), with sigma2
and crit at the kernel's own T (`held_at_T`); `reference_mp` states at 256 bits that the state system is the reference's dense system."""
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
    ds_dT, sum_S, rcp_S, own_C = own_rounding(c, T64)
    gS = (ds_dT * gT).sum() + sum_S + rcp_S
    gC = np.sqrt((gT ** 2).sum(axis=1)).sum() / M + own_C
    return gT, gS, gC


def own_rounding(c, T64):
    """What sigma2 and crit carry apart from T's own error, at the fp64 T given: (|d sigma2 / d T| per node and coordinate, the residual form's summation
    rounding, fast_rcp's, crit's summation rounding) -- the terms `gate` documents, shared with `held_at_T`."""
    M = c.M
    P1 = c.sums[:M].astype(np.float64); Rm = c.sums[M:4 * M].reshape(3, M).T.astype(np.float64); Q = float(c.sums[4 * M])
    d = T64 - c.y
    Np = P1.sum()
    ds_dT = np.abs(2 * (P1[:, None] * d - Rm)) / (3 * Np)
    mag = abs(Q) + 2 * np.abs(d * Rm).sum() + (P1[:, None] * d * d).sum()
    crit = np.sqrt(((T64 - c.yp) ** 2).sum(axis=1)).sum() / M
    return ds_dT, (2 * np.log2(max(M, 2)) + 8) * U * mag / (3 * Np), 4 * U * abs(mag) / (3 * Np), (np.log2(max(M, 2)) + 8) * U * crit


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


# ---- the band held by its backward error ------------------------------------------------------------------------------------------------------
# k_mstep_band solves (c G^-1 + D + g H) V = B directly in V, as an SPD banded L D L^T of the state system
#     A2 x = E^T B,   A2 = lambda sigma2 K + E^T (diag(P1 + alpha J) + sigma2 w H) E,   x = (f_0, f'_0, f_1, ...),  V = E x
# (tests/band_numpy.py).  Its forward error grows with the chain and the condition number; its backward error does not.  So a returned T is
# held by the residual of that system in longdouble, with the unknowns the kernel does not return (f') taken as their exact function of f.
def _to_ld(x):
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def _state_precision_in(F, sqrt, exp, gaps, beta, series):
    """band_numpy.state_precision in the arithmetic F: (dg [M][3: ff, fp, pp], off [M][4]).  series: Q of a gap with sqrt2 h / beta < 1 from the
    positive series of chain_numpy.chain_link (the closed form Q = Pinf - Phi Pinf Phi^T cancels by (sqrt2 h / beta)^3)."""
    import chain_numpy as cn
    b = F(beta); r2 = sqrt(F(2)); s = r2 / b; sf2 = 1 / (2 * r2 * b)
    M = len(gaps) + 1
    dg = [[F(0)] * 3 for _ in range(M)]; off = [[F(0)] * 4 for _ in range(M)]
    dg[0][0] += 1 / sf2; dg[0][2] += 1 / (s * s * sf2)
    for i in range(1, M):
        h = gaps[i - 1]; x = s * h; e = exp(-x); e2 = e * e
        if series and x < 1:
            sm = cn._tail_series(2 * x)
            u11, u22 = e2 * sm, e2 * (4 * x + sm)
        else:
            u11, u22 = 1 - e2 * (1 + 2 * x + 2 * x * x), 1 - e2 * (1 - 2 * x + 2 * x * x)
        f11, f12, f21, f22 = e * (1 + x), e * h, -s * s * h * e, e * (1 - x)
        q11, q12, q22 = sf2 * u11, 2 * sf2 * s ** 3 * h * h * e2, sf2 * s * s * u22
        det = q11 * q22 - q12 * q12
        a, bb, d = q22 / det, -q12 / det, q11 / det
        dg[i][0] += a; dg[i][1] += bb; dg[i][2] += d
        t11, t12 = a * f11 + bb * f21, a * f12 + bb * f22
        t21, t22 = bb * f11 + d * f21, bb * f12 + d * f22
        dg[i - 1][0] += f11 * t11 + f21 * t21
        dg[i - 1][1] += f11 * t12 + f21 * t22
        dg[i - 1][2] += f12 * t12 + f22 * t22
        off[i] = [-t11, -t12, -t21, -t22]
    return dg, off


def state_precision_exact(Y0, beta, use_mpmath=None):
    """K of band_numpy.state_precision from estep_ref.chain_gaps_exact, in longdouble, entries right to ~1e-18: evaluated by mpmath at 256 bits
    (closed form; every sum in mpmath, so the diagonal blocks' f-f' entries, which nearly cancel between the two links of a node, are right relative
    to themselves) where mpmath imports, else by the positive series in longdouble (right relative to the summed terms).  tests/test_mstep_ref.py
    holds the two against each other."""
    gaps = np.diagonal(R.chain_gaps_exact(Y0), 1)
    if use_mpmath is None:
        try:
            import mpmath  # noqa: F401
            use_mpmath = True
        except ImportError:
            use_mpmath = False
    if use_mpmath:
        import mpmath
        with mpmath.workprec(256):
            mpf = mpmath.mpf
            gm = [mpf(float(h)) + mpf(float(h - LD(float(h)))) for h in gaps]
            dg, off = _state_precision_in(mpf, mpmath.sqrt, mpmath.exp, gm, float(beta), False)
            dg = [[_to_ld(v) for v in r] for r in dg]; off = [[_to_ld(v) for v in r] for r in off]
    else:
        dg, off = _state_precision_in(LD, np.sqrt, np.exp, gaps, float(beta), True)
    return np.array(dg, dtype=LD), np.array(off, dtype=LD)


class NotRefined(ArithmeticError):
    """BandSystem.solve: the fp64 factor is too far from A2 for the refinement to contract (condition number beyond 1 / u)."""


class BandSystem:
    """A2 (2M x 2M, longdouble, dense storage of a band of half-width 12), B (M x 3, longdouble, formed as `reference` forms it) and the fp64
    magnitudes and factors band_backward_error and band_exact need."""

    def __init__(self, c):
        import scipy.linalg as sla
        M = c.M; n = 2 * M
        dg, off = state_precision_exact(c.Y0, c.beta)
        cc = LD(c.lambda_) * LD(c.s2)
        A = np.zeros((n, n), dtype=LD)
        i = np.arange(M)
        A[2 * i, 2 * i] = cc * dg[:, 0]; A[2 * i, 2 * i + 1] = cc * dg[:, 1]; A[2 * i + 1, 2 * i] = cc * dg[:, 1]; A[2 * i + 1, 2 * i + 1] = cc * dg[:, 2]
        for k in range(1, M):
            blk = cc * off[k].reshape(2, 2)
            A[2 * k: 2 * k + 2, 2 * k - 2: 2 * k] = blk; A[2 * k - 2: 2 * k, 2 * k: 2 * k + 2] = blk.T
        P1 = c.sums[:M]; Rm = c.sums[M:4 * M].reshape(3, M).T
        Y0 = c.Y0.astype(LD)
        D = P1.copy()
        B = Rm + P1[:, None] * (c.y.astype(LD) - Y0)
        if c.H is not None:
            H = np.asarray(c.H, dtype=np.float64).astype(LD); g = LD(c.s2) * LD(c.lle_weight)
            A[0::2, 0::2] += g * H; B = B - g * H @ Y0
        if c.priors is not None:
            J = np.zeros(M, dtype=LD); Yext = Y0.copy()
            for r in c.priors:
                J[int(r[0])] = 1; Yext[int(r[0])] = r[1:]
            D = D + LD(c.alpha) * J; B = B + LD(c.alpha) * (Yext - Y0)
        A[2 * i, 2 * i] += D
        r, q = np.indices((n, n))
        assert not A[np.abs(r - q) > 12].any(), "H reaches beyond 6 nodes: not the band's system"
        self.M = M; self.A = A; self.B = B
        self.Bmag = system(c)[6]
        A64 = A.astype(np.float64)
        self.absA = np.abs(A64)
        self.App = A[1::2, 1::2]; self.Apf = A[1::2, 0::2]
        self.lu_pp = sla.lu_factor(A64[1::2, 1::2])
        self.Wm = np.abs(A64[0::2, 1::2]) @ np.abs(np.linalg.inv(A64[1::2, 1::2]))            # |A_fp| |A_pp^-1|
        self.Rb = np.abs(A64[0::2, 0::2]) + self.Wm @ np.abs(A64[1::2, 0::2])                 # |A_ff| + |A_fp| |A_pp^-1| |A_pf|
        self.scale = 1.0 / np.sqrt(np.diagonal(A64))                                          # (H's entries span 20 decades: the factor is of S A2 S)
        ab = np.zeros((13, n))
        for d in range(min(13, n)):                                                           # (4 - 6 nodes: fewer unknowns than the band is wide)
            ab[12 - d, d:] = np.diagonal(A64, d) * self.scale[d:] * self.scale[:n - d]
        try:
            self.chol = sla.cholesky_banded(ab)
        except np.linalg.LinAlgError:
            # not positive definite in fp64: never a cell's own system (SPD is the kernel's premise; tests/test_mstep_ref.py asserts it), but a case
            # altered to see a term missing may be -- the launch file's beta under the oracle's H at 512 nodes.  A banded L U with row exchanges then.
            self.chol = None
            self.full = np.zeros((25, n))
            for d in range(-min(12, n - 1), min(12, n - 1) + 1):
                self.full[12 - d, max(d, 0): n + min(d, 0)] = np.diagonal(A64, d) * self.scale[max(d, 0): n + min(d, 0)] * self.scale[max(-d, 0): n - max(d, 0)]

    def with_fprime(self, V):
        """x (2M x 3, longdouble) with the f rows V and f' = -A_pp^-1 A_pf V: fp64 LU, refined with longdouble residuals until the f' rows' residual is at
        the longdouble rounding of forming it (<= 1e-18 |A2| |x|); returns (x, that residual's worst ratio to |A2| |x|)."""
        import scipy.linalg as sla
        rhs = -(self.Apf @ V)
        fp = sla.lu_solve(self.lu_pp, rhs.astype(np.float64)).astype(LD)
        x = np.zeros((2 * self.M, V.shape[1]), dtype=LD); x[0::2] = V
        for _ in range(8):
            x[1::2] = fp
            res = rhs - self.App @ fp
            w = float((np.abs(res).astype(np.float64) / (self.absA @ np.abs(x).astype(np.float64))[1::2]).max())
            if w <= 1e-18:
                return x, w
            fp = fp + sla.lu_solve(self.lu_pp, res.astype(np.float64)).astype(LD)
        raise AssertionError(f"f' rows not solved: residual {w:.3g} |A2| |x|")

    def solve(self, B=None):
        """x with A2 x = E^T B: banded Cholesky of the fp64-rounded, equilibrated A2, refined with longdouble residuals to the rounding of forming them."""
        import scipy.linalg as sla
        b = np.zeros((2 * self.M, 3), dtype=LD); b[0::2] = self.B if B is None else B
        S = self.scale[:, None]
        fac = (lambda r: sla.cho_solve_banded((self.chol, False), r)) if self.chol is not None else (lambda r: sla.solve_banded((12, 12), self.full, r))
        inv = lambda r: (S * fac(S * r.astype(np.float64))).astype(LD)
        x = inv(b)
        for _ in range(12):
            res = b - self.A @ x
            w = float((np.abs(res).astype(np.float64) / (self.absA @ np.abs(x).astype(np.float64) + np.abs(b).astype(np.float64))).max())
            if w <= 1e-18:
                return x
            x = x + inv(res)
        raise NotRefined(f"state system not solved: residual {w:.3g} (|A2| |x| + |b|)")


def band_system(c):
    if getattr(c, "_band_system", None) is None:
        c._band_system = BandSystem(c)
    return c._band_system


def band_exact(c):
    """T (longdouble) of the state system of c at the cost of a banded solve: a point whose residual in that system is at longdouble rounding.  Its
    distance from T* is that times the condition number -- 1e-19 m with a bounded H, 1e-16 m under the oracle's H at 257 nodes, 1e-7 m at 512 (entries
    up to 7e18; reference_mp, tests/test_mstep_ref.py) -- so it stands for `the exact answer of this system` only in the backward sense, which is what
    the conditions on band_backward_error ask of it (the answer of a system with rounded sums, or without a term, seen from the true one)."""
    return c.Y0.astype(LD) + band_system(c).solve()[0::2]


def band_backward_error(c, T):
    """(worst ratio, (node, coordinate)) of the f rows' residual of the state system at a returned T (M x 3, fp64) to what a banded L D L^T in fp64
    may leave there.  V = T - Y0 in longdouble, f' its exact function of V (BandSystem.with_fprime), r = B - A_ff V - A_fp f' per node and
    coordinate, against SAFETY times
        EPS_BAND u ((|A2| |x|) on the f rows + |A_fp| |A_pp^-1| (|A2| |x|) on the f' rows)      the solve's backward error, a constant number of ulp per
                                                                                              term; the kernel's own f'-row residuals reach the f rows
                                                                                              through A_fp A_pp^-1 once f' is rebuilt
      + EPS_B u |B|'s terms (system(c))                                                       forming B
      + u (|A_ff| + |A_fp| |A_pp^-1| |A_pf|) |T|                                              T = Y0 + V is rounded once and V read back as T - Y0.
    A cell passes at <= 1.  u = 2^-53 in fp32 mode too: only `nodes` is float there, and the cells' nodes are exact fp32 values."""
    s = band_system(c)
    T64 = np.asarray(T, dtype=np.float64)
    x, _ = s.with_fprime(T64.astype(LD) - c.Y0.astype(LD))
    mag = s.absA @ np.abs(x).astype(np.float64)
    r = np.abs(s.B - s.A[0::2] @ x).astype(np.float64)
    tol = SAFETY * (EPS_BAND * U * (mag[0::2] + s.Wm @ mag[1::2]) + EPS_B * U * s.Bmag + U * (s.Rb @ np.abs(T64)))
    q = r / tol
    m, d = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[m, d]), (int(m), int(d))


def held_at_T(c, T):
    """(sigma2, its gate, crit, its gate) at a returned T (fp64): the residual form and the criterion in longdouble from that T and the given sums, and
    what the kernel's own evaluation may differ by -- own_rounding's terms, and u |T| per coordinate (the kernel forms them before T = Y0 + V is
    rounded) through |d sigma2 / d T| and crit's sum.  T's own error is held by band_backward_error, not here."""
    M = c.M
    T64 = np.asarray(T, dtype=np.float64); TL = T64.astype(LD)
    P1 = c.sums[:M]; Rm = c.sums[M:4 * M].reshape(3, M).T
    d = TL - c.y.astype(LD)
    s2 = (c.sums[4 * M] - LD(2) * (d * Rm).sum() + (P1[:, None] * d * d).sum()) / (P1.sum() * LD(3))
    crit = np.sqrt(((TL - c.yp.astype(LD)) ** 2).sum(axis=1)).sum() / LD(M)
    ds_dT, sum_S, rcp_S, own_C = own_rounding(c, T64)
    rb = U * np.abs(T64)
    return s2, (ds_dT * rb).sum() + sum_S + rcp_S, crit, np.sqrt((rb ** 2).sum(axis=1)).sum() / M + own_C


def reference_mp(c, prec=256):
    """(T* longdouble, residual): the solution of the state system at `prec` bits (mpmath: K's closed form, a banded L D L^T) and the residual it
    leaves in `reference`'s dense system, both formed at that precision from the same inputs: W = (B - (D + g H) V) / (lambda sigma2) must give
    G W = V, G of trackdlo.cpp:233 over the distances along the chain; returned as max |G W - V| / max |V|.  `reference`'s own T* carries its
    longdouble forming of G and A amplified by |G| |W| / |V| -- ~1e-16 m with the pre-processing parameters, the size of band_backward_error's
    tolerance -- so the statement that the state system IS the reference's dense system is made here, where neither side rounds visibly."""
    import mpmath
    with mpmath.workprec(prec):
        mpf = mpmath.mpf
        ld = lambda v: mpf(float(v)) + mpf(float(v - LD(float(v))))                        # a longdouble, exactly
        M = c.M; n = 2 * M
        gaps = [ld(h) for h in np.diagonal(R.chain_gaps_exact(c.Y0), 1)]
        dg, off = _state_precision_in(mpf, mpmath.sqrt, mpmath.exp, gaps, float(c.beta), False)
        cc = mpf(c.lambda_) * mpf(c.s2)
        assert cc != 0
        g = mpf(c.s2) * mpf(c.lle_weight) if c.H is not None else mpf(0)
        Hn = None if c.H is None else np.asarray(c.H, dtype=np.float64)
        H = lambda i, j: mpf(float(Hn[i, j])) if Hn is not None and 0 <= j < M else mpf(0)
        assert Hn is None or not Hn[np.abs(np.subtract.outer(np.arange(M), np.arange(M))) > 6].any()
        P1 = [ld(v) for v in c.sums[:M]]
        Rm = [[ld(v) for v in row] for row in c.sums[M:4 * M].reshape(3, M).T]
        Y0 = [[mpf(float(v)) for v in row] for row in c.Y0]; y = [[mpf(float(v)) for v in row] for row in c.y]
        D = list(P1)
        B = [[Rm[i][d] + P1[i] * (y[i][d] - Y0[i][d]) - g * sum(H(i, j) * Y0[j][d] for j in range(max(i - 6, 0), min(i + 7, M))) for d in range(3)] for i in range(M)]
        if c.priors is not None:
            a = mpf(c.alpha); J = [mpf(0)] * M; Yext = [list(r) for r in Y0]
            for r in c.priors:
                J[int(r[0])] = mpf(1); Yext[int(r[0])] = [mpf(float(v)) for v in r[1:]]
            for i in range(M):
                D[i] = D[i] + a * J[i]
                for d in range(3):
                    B[i][d] = B[i][d] + a * (Yext[i][d] - Y0[i][d])
        # the band: ab[r][12 + d] = A2[r, r + d], d = -12 .. 12 -- row 2i carries row i of H as given (a product (I - L)^T (I - L) formed in fp64
        # is symmetric only to rounding, and the dense system reads H by rows), so an L U without pivoting, not an L D L^T
        ab = [[mpf(0)] * 25 for _ in range(n)]
        for i in range(M):
            ab[2 * i][12] = cc * dg[i][0] + D[i]; ab[2 * i][13] = cc * dg[i][1]; ab[2 * i + 1][11] = cc * dg[i][1]; ab[2 * i + 1][12] = cc * dg[i][2]
            for j in range(max(i - 6, 0), min(i + 7, M)):
                ab[2 * i][12 + 2 * (j - i)] += g * H(i, j)
            if i > 0:
                for p in range(2):
                    for q in range(2):                                                  # K[2i + p, 2(i - 1) + q] = off[i][2p + q], and its transpose
                        ab[2 * i + p][12 - 2 - p + q] += cc * off[i][2 * p + q]
                        ab[2 * (i - 1) + q][12 + 2 + p - q] += cc * off[i][2 * p + q]
        Y = [[mpf(0)] * 3 for _ in range(n)]
        for i in range(M):
            Y[2 * i] = list(B[i])
        for k in range(n):
            w = min(12, n - 1 - k)
            for i in range(1, w + 1):
                m = ab[k + i][12 - i] / ab[k][12]
                for j in range(1, w + 1):
                    ab[k + i][12 - i + j] -= m * ab[k][12 + j]
                for d in range(3):
                    Y[k + i][d] -= m * Y[k][d]
        x = [[mpf(0)] * 3 for _ in range(n)]
        for k in range(n - 1, -1, -1):
            for d in range(3):
                x[k][d] = (Y[k][d] - sum(ab[k][12 + j] * x[k + j][d] for j in range(1, min(12, n - 1 - k) + 1))) / ab[k][12]
        V = x[0::2]
        W = [[(B[i][d] - D[i] * V[i][d] - g * sum(H(i, j) * V[j][d] for j in range(max(i - 6, 0), min(i + 7, M)))) / cc for d in range(3)] for i in range(M)]
        coord = [mpf(0)]
        for h in gaps:
            coord.append(coord[-1] + h)
        b = mpf(float(c.beta)); r2 = mpmath.sqrt(mpf(2)); k0 = 1 / (2 * b * 2 * b)
        GW = [[mpf(0)] * 3 for _ in range(M)]
        for i in range(M):
            for j in range(i, M):
                dd = coord[j] - coord[i]
                gij = k0 * mpmath.exp(-r2 * dd / b) * (2 * dd + r2 * b)
                for d in range(3):
                    GW[i][d] += gij * W[j][d]
                    if j != i:
                        GW[j][d] += gij * W[i][d]
        res = max(abs(GW[i][d] - V[i][d]) for i in range(M) for d in range(3)) / max(abs(V[i][d]) for i in range(M) for d in range(3))
        T = np.array([[_to_ld(Y0[i][d] + V[i][d]) for d in range(3)] for i in range(M)], dtype=LD)
        return T, float(res)
