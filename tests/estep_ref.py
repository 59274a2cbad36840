"""One E-step of trackdlo::cpd_lle restated in extended precision (tests only).

This is the oracle's E-step (oracle/ref_cpu.c, ref_cpd_lle: trackdlo.cpp:278-389) for a given state -- cloud X, the
registration's incoming nodes Y0, the current nodes Y, sigma2 -- returned in the layout of the library's N-split sums
(include/trackdlo_hip.h, tdlo_split_estep):

    P1[m] = sum_n P_mn,  R[m, d] = sum_n P_mn (x_nd - y_md),  Q = sum_mn P_mn |x_n - y_m|^2,  N_kept

The values are accumulated in np.longdouble (pairwise inside a chunk of points, compensated across chunks), so that the
kernels' fixed-point and floating-point sums can be compared element by element with gates derived from their own
arithmetic (tests/test_estep_sums_gpu.py).  Every branch the oracle takes on fp64 values is decided on fp64 values here:
the prune, the Euclidean argmax (an all-zero column in fp64 sends a point to node 0), the second node, and which
memberships are exact zeros in fp64 (exp underflow): the wider exponent of longdouble would not underflow and the
reference would take the other branch.

Besides the sums it returns what the gates need: each element's absolute mass (sum of |terms|, distances measured from
an origin up to `rho` away -- the kernels sum relative to a wave-local origin), the mass weighted by the exponent
argument of every term (`wmass`; `cmass`: the same with the cancellation of the normalisation, to first order), the bound on what a node
window of E bits may drop, the mass of points whose discrete decisions
are within rounding of a tie (fp32 mode), per-point contributions, and per kept point its nearest node, its pair (lo, hi) and whether
its whole column underflowed (`near`, `lo`, `hi`, `under`).
"""
import numpy as np

LD = np.longdouble
F64_EXP_ZERO = -745.2            # exp(t) is exactly 0.0 in fp64 below about this


def prune(X, Y0):
    """trackdlo.cpp:177-195: keep the points closer than 0.1 m to some incoming node (fp64, the oracle's formula)."""
    X = np.asarray(X, dtype=np.float64); Y0 = np.asarray(Y0, dtype=np.float64)
    keep = np.zeros(len(X), dtype=bool)
    for s in range(0, len(X), 4096):
        x = X[s:s + 4096]
        d2 = (Y0[None, :, 0] - x[:, 0:1]) ** 2 + (Y0[None, :, 1] - x[:, 1:2]) ** 2 + (Y0[None, :, 2] - x[:, 2:3]) ** 2
        keep[s:s + 4096] = np.sqrt(d2.min(axis=1)) < 0.1
    return keep


def chain_coord(Y0):
    """trackdlo.cpp:219-223: the running sum of the segment lengths, left to right, in fp64."""
    Y0 = np.asarray(Y0, dtype=np.float64)
    seg = np.sqrt(((Y0[1:] - Y0[:-1]) ** 2).sum(axis=1))
    c = np.zeros(len(Y0))
    cur = 0.0
    for i, s in enumerate(seg):
        cur += s
        c[i + 1] = cur
    return c


def chain_gaps_exact(Y0):
    """|coord_i - coord_j| for every pair, to a few longdouble ulp RELATIVE to the distance itself: the segment lengths in longdouble, their
    running sum carried as an unevaluated pair hi + lo (two-sum at every step), the difference of two entries formed from both parts.  The
    fp64 running sum of chain_coord is off by ~1e-16 m absolute, which the dense form G W amplifies by |G| |W| / |V| (up to 1e6 with the
    pre-processing parameters): tests/mstep_ref.py's reference must not carry that."""
    Y0 = np.asarray(Y0, dtype=np.float64).astype(LD)
    seg = np.sqrt(((Y0[1:] - Y0[:-1]) ** 2).sum(axis=1))
    hi = np.zeros(len(Y0), dtype=LD); lo = np.zeros(len(Y0), dtype=LD)
    h = LD(0); l = LD(0)
    for i, sg in enumerate(seg):
        t = h + sg
        l += (h - t) + sg if abs(h) >= abs(sg) else (sg - t) + h
        h = t
        hi[i + 1] = h; lo[i + 1] = l
    return np.abs((hi[:, None] - hi[None, :]) + (lo[:, None] - lo[None, :]))


def sum_d2(X, Y0):
    """The sigma2 initialisation's sum over kept points and nodes (trackdlo.cpp:263-273), in longdouble."""
    X = np.asarray(X, dtype=LD); Y0 = np.asarray(Y0, dtype=LD)
    tot = LD(0)
    for s in range(0, len(X), 4096):
        x = X[s:s + 4096]
        tot += (((x[:, None, :] - Y0[None, :, :]) ** 2).sum(axis=2)).sum()
    return tot


def dmin_sq(X, Y, fp32=False):
    """Per-node minimum squared distance to the kept points (trackdlo.cpp:278-296) with the oracle's fp64 formula
    (a*a + b*b + c*c); fp32=True: of the fp32-rounded coordinates, evaluated exactly."""
    X = np.asarray(X, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    if fp32:
        X = X.astype(np.float32).astype(LD); Y = Y.astype(np.float32).astype(LD)
    best = np.full(len(Y), np.inf, dtype=X.dtype)
    for s in range(0, len(X), 4096):
        x = X[s:s + 4096]
        a = Y[None, :, 0] - x[:, 0:1]; b = Y[None, :, 1] - x[:, 1:2]; c = Y[None, :, 2] - x[:, 2:3]
        best = np.minimum(best, (a * a + b * b + c * c).min(axis=0))
    return best


class _Acc:
    """Neumaier-compensated running sum of longdouble arrays (one term per chunk)."""

    def __init__(self, shape):
        self.s = np.zeros(shape, dtype=LD); self.c = np.zeros(shape, dtype=LD)

    def add(self, v):
        v = np.asarray(v, dtype=LD)
        t = self.s + v
        big = np.abs(self.s) >= np.abs(v)
        self.c += np.where(big, (self.s - t) + v, (v - t) + self.s)
        self.s = t

    def value(self):
        return self.s + self.c


def estep(X, Y0, Y, sigma2, *, mu, k_vis=0.0, visibility_threshold=0.008, visible_nodes=None, n_kept_global=None,
          sum_d2_global=None, dmin_sq_global=None, fp32=False, rho=0.25, win_e=None, tie_rel=None, chunk_elems=1 << 21,
          keep=None):
    """One E-step.  X: the cloud as handed to the library (before the prune); Y0: the registration's incoming nodes (prune,
    chain coordinate); Y: the current nodes; sigma2: the current sigma2 (0: initialised from the GLOBAL kept count and sum,
    trackdlo.cpp:263-273, defaulting to this cloud's own).  fp32=True restates the fp32 mode's inputs: the kernels compute
    on fp32-rounded coordinates and chain coordinate (centring offset 0: the caller's nodes have centroid 0 exactly).
    win_e: a node window of that many bits (memberships below 2^-E of the point's largest may be dropped) -- the bound on
    what it drops is returned as `win`.  tie_rel: relative margin within which a discrete decision counts as a tie (its
    point's terms go to `amb`)."""
    X = np.asarray(X, dtype=np.float64); Y0 = np.asarray(Y0, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    M = len(Y)
    if keep is None:
        keep = prune(X, Y0)
    Xk = X[keep]
    N = len(Xk)
    Ng = float(N if n_kept_global is None else n_kept_global)
    coord = chain_coord(Y0)
    if fp32:
        Xk = Xk.astype(np.float32).astype(np.float64); Yc = Y.astype(np.float32).astype(np.float64)
        coord = coord.astype(np.float32).astype(np.float64)
    else:
        Yc = Y
    s2 = float(sigma2)
    if s2 == 0:
        sd = sum_d2(X[keep], Y0) if sum_d2_global is None else LD(sum_d2_global)
        s2 = float(sd / LD(3 * M * Ng))
    s2L = LD(s2)
    vis_branch = visible_nodes is not None and len(visible_nodes) not in (0, M) and k_vis != 0
    # trackdlo.cpp:300 / :378 (pow(2 pi sigma2, 3/2) mu / (1 - mu) [* M] / N)
    cpre = (LD(2) * LD(np.pi) * s2L) ** LD(1.5) * LD(mu) / (LD(1) - LD(mu))
    lnv = np.zeros(M, dtype=LD)
    if vis_branch:
        dq = np.asarray(dmin_sq_global, dtype=np.float64)
        if fp32:
            dq = dq.astype(np.float32).astype(np.float64)
        d = np.sqrt(dq.astype(LD))
        d = np.where(d > 10000, LD(10000), d)
        d = np.where(d <= visibility_threshold, LD(0), d)
        w = np.exp(-LD(k_vis) * d)
        lnv = np.log(w / w.sum())                                   # :362-372, as a log weight (<= 0)
        c = cpre / LD(Ng)
    else:
        c = cpre * LD(M) / LD(Ng)
    YL = Yc.astype(LD)
    coordL = coord.astype(LD)
    acc_sum = _Acc(4 * M + 1); acc_mass = _Acc(4 * M + 1); acc_wmass = _Acc(4 * M + 1); acc_win = _Acc(4 * M + 1); acc_amb = _Acc(4 * M + 1)
    pmax = np.zeros(N); parg = np.zeros(N, dtype=np.int64); rmax = np.zeros(N); qn = np.zeros(N)
    acc_cmass = _Acc(4 * M + 1)
    near = np.zeros(N, dtype=np.int64); p_lo = np.zeros(N, dtype=np.int64); p_hi = np.zeros(N, dtype=np.int64); under = np.zeros(N, dtype=bool)
    gap = 0; n_under = 0; n_amb = 0
    B = max(1, chunk_elems // M)
    m_idx = np.arange(M)
    for s in range(0, N, B):
        x = Xk[s:s + B]; nb = len(x)
        rows = np.arange(nb)
        # ---- distances (fp64, the oracle's formula) and the Euclidean argmax with its first-max rule (:298-310)
        dx = Yc[None, :, 0] - x[:, 0:1]; dy = Yc[None, :, 1] - x[:, 1:2]; dz = Yc[None, :, 2] - x[:, 2:3]
        d2 = dx * dx + dy * dy + dz * dz                                       # nb x M
        col = np.exp(-0.5 * d2 / s2)
        allz = ~(col > 0).any(axis=1)
        a = np.where(allz, 0, col.argmax(axis=1))                              # (an all-zero column: its first index, node 0)
        n_under += int(allz.sum())
        # ---- the second node and the geodesic distances (:313-351)
        c1 = np.where(a - 1 == -1, 2, a - 1); c2 = np.where(a + 1 == M, M - 3, a + 1)
        s1 = np.sqrt(d2[rows, c1]); s2_ = np.sqrt(d2[rows, c2])
        b = np.where(s1 < s2_, c1, c2)
        lo = np.minimum(a, b); hi = np.maximum(a, b)
        gap += int((hi - lo == 2).sum())
        amb = np.zeros(nb, dtype=bool)
        if tie_rel is not None:
            srt = np.sort(d2, axis=1)
            if M > 1:
                amb |= (srt[:, 1] - srt[:, 0]) <= tie_rel * srt[:, 1]
            amb |= np.abs(s1 - s2_) <= tie_rel * np.maximum(s1, s2_)
            # the all-underflow decision: the nearest node's exponent within rounding of fp64's last value
            amb |= np.abs(-0.5 * srt[:, 0] / s2 - F64_EXP_ZERO) <= tie_rel * 0.5 * srt[:, 0] / s2 + 1.0
        n_amb += int(amb.sum())
        # extended precision from here on
        xL = x.astype(LD)
        ddx = xL[:, None, 0] - YL[None, :, 0]; ddy = xL[:, None, 1] - YL[None, :, 1]; ddz = xL[:, None, 2] - YL[None, :, 2]
        d2L = ddx * ddx + ddy * ddy + ddz * ddz
        dlo = np.sqrt(d2L[rows, lo]); dhi = np.sqrt(d2L[rows, hi])
        mm = m_idx[None, :]
        t = np.where(mm < lo[:, None], np.abs(coordL[None, :] - coordL[lo][:, None]) + dlo[:, None],
                     np.where(mm > hi[:, None], np.abs(coordL[None, :] - coordL[hi][:, None]) + dhi[:, None], LD(0)))
        geo = t * t
        geo[rows, lo] = d2L[rows, lo]; geo[rows, hi] = d2L[rows, hi]          # (:332-333; nodes strictly between keep the zero of :305)
        arg = LD(0.5) * geo / s2L
        # which memberships the oracle's fp64 exp leaves exactly zero (:375 / :381), decided in fp64
        e64 = np.exp(-0.5 * geo.astype(np.float64) / s2 + (lnv.astype(np.float64)[None, :] if vis_branch else 0.0))
        E = np.where(e64 > 0, np.exp(-arg + lnv[None, :]), LD(0))
        den = E.sum(axis=1) + c
        P = E / den[:, None]                                                   # :383
        # ---- the sums (:386-389), node-major so that the reductions over points are pairwise
        PT = P.T
        dist = np.sqrt(d2L)
        rel = arg - lnv[None, :]                                               # the exponent's size (the kernels' relative error grows with it)
        abar = (P * rel).sum(axis=1) / np.maximum(P.sum(axis=1), LD(1e-300))
        relw = rel + abar[:, None]
        dd = (ddx, ddy, ddz)
        terms = [PT]
        for k in range(3):
            terms.append((P * dd[k]).T)
        tq = (P * d2L).T
        vals = np.concatenate([tt.sum(axis=1) for tt in terms] + [tq.sum(axis=1).sum(keepdims=True)])
        acc_sum.add(vals)
        Pd = P * (dist + LD(rho))
        mP = PT.sum(axis=1)
        mR = Pd.T.sum(axis=1)
        mQ = (P * (dist + LD(rho)) ** 2).sum()
        acc_mass.add(np.concatenate([mP, mR, mR, mR, [mQ]]))
        wP = (P * relw).T.sum(axis=1); wR = (Pd * relw).T.sum(axis=1); wQ = (P * (dist + LD(rho)) ** 2 * relw).sum()
        acc_wmass.add(np.concatenate([wP, wR, wR, wR, [wQ]]))
        # the same to first order WITH the normalisation's cancellation: relative errors delta_k of a point's unnormalised memberships move
        # P_m by P_m (delta_m - sum_k P_k delta_k), at most P_m (|delta_m| (1 - P_m) + sum_{k != m} P_k |delta_k|); here |delta_k| = rel_k
        cw = P * (rel * (LD(1) - LD(2) * P) + (P * rel).sum(axis=1)[:, None])
        cR = (cw * (dist + LD(rho))).T.sum(axis=1)
        acc_cmass.add(np.concatenate([cw.T.sum(axis=1), cR, cR, cR, [(cw * (dist + LD(rho)) ** 2).sum()]]))
        near[s:s + nb] = a; p_lo[s:s + nb] = lo; p_hi[s:s + nb] = hi; under[s:s + nb] = allz
        if win_e is not None:
            pm = P.max(axis=1)
            small = P < pm[:, None] * LD(2.0) ** LD(-win_e)
            Ps = np.where(small, P, LD(0))
            # a dropped membership is missing from its own sum and from the point's normaliser (which scales all of its terms)
            frac = Ps.sum(axis=1) / np.maximum(P.sum(axis=1), LD(1e-300))
            wp = Ps + P * frac[:, None]
            wpd = wp * (dist + LD(rho))
            acc_win.add(np.concatenate([wp.T.sum(axis=1), wpd.T.sum(axis=1), wpd.T.sum(axis=1), wpd.T.sum(axis=1), [(wp * (dist + LD(rho)) ** 2).sum()]]))
        if amb.any():
            Pa = P[amb]; da_ = dist[amb] + LD(rho)
            acc_amb.add(np.concatenate([Pa.sum(axis=0), (Pa * da_).sum(axis=0), (Pa * da_).sum(axis=0), (Pa * da_).sum(axis=0), [(Pa * da_ ** 2).sum()]]))
        pmax[s:s + nb] = P.max(axis=1).astype(np.float64)
        parg[s:s + nb] = P.argmax(axis=1)
        rmax[s:s + nb] = np.max(np.abs(np.stack([P * q for q in dd])), axis=(0, 2)).astype(np.float64) if nb else 0
        qn[s:s + nb] = (P * d2L).sum(axis=1).astype(np.float64)
    v = acc_sum.value()
    out = dict(P1=v[:M], R=v[M:4 * M].reshape(3, M).T, Q=v[4 * M], N=N, sigma2=s2, coord=coord, vis_branch=vis_branch,
               mass=acc_mass.value(), wmass=acc_wmass.value(), win=acc_win.value(), amb=acc_amb.value(),
               cmass=acc_cmass.value(), near=near, lo=p_lo, hi=p_hi, under=under,
               pmax=pmax, parg=parg, rmax=rmax, qn=qn, gap_quirk=gap, n_underflow=n_under, n_amb=n_amb, keep=keep)
    out["sums"] = sums_vector(out)
    return out


def sums_vector(r):
    """[P1 | R (column-major M x 3) | Q | N_kept] as longdouble, the kernels' layout."""
    return np.concatenate([r["P1"], r["R"].T.reshape(-1), [r["Q"], LD(r["N"])]])


def mstep(sums, Y0, Y, sigma2, *, beta, lambda_, solve, alpha=0.0, priors=None, lle_weight=0.0, H=None, exact=False):
    """The M-step of trackdlo.cpp:392-422 from sums in the kernels' layout, as tests/numpy_shard.py builds it: R is converted
    back to PX = R + P1 y and the system is solved by `solve(A, B)` (oracle.solve_extended).  sigma2 in the residual form
    sum P |x - T|^2 = Q - 2 sum_m d_m . R_m + sum_m P1_m |d_m|^2, d = T - y, evaluated in longdouble.
    exact=True (tests/mstep_ref.py): the distances along the chain are those of chain_gaps_exact (relative error ~1e-19, not the fp64
    running sum's absolute 1e-16 m), G, A and B = R + P1 (y - Y0) are formed in longdouble from them and the fp64 inputs and handed to
    `solve` as longdouble, T = Y0 + G W stays in longdouble, and T and sigma2 are returned in longdouble."""
    Y0 = np.asarray(Y0, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    M = len(Y0)
    F = LD if exact else np.float64
    s = np.asarray(sums, dtype=LD)
    P1L = s[:M]; RL = s[M:4 * M].reshape(3, M).T; QL = s[4 * M]
    P1 = P1L.astype(F)
    if exact:
        dd = chain_gaps_exact(Y0)
    else:
        coord = chain_coord(Y0)
        dd = np.abs(coord[:, None] - coord[None, :])
    b = F(beta); r2 = np.sqrt(F(2))
    G = 1 / (2 * b * 2 * b) * np.exp(-r2 * dd / b) * (2 * dd + r2 * b)       # :233
    A = P1[:, None] * G + F(lambda_) * F(sigma2) * np.eye(M, dtype=F)
    if exact:
        Bm = RL + P1L[:, None] * (Y.astype(LD) - Y0.astype(LD))
    else:
        PX = (RL + P1L[:, None] * Y.astype(LD)).astype(np.float64)
        Bm = PX - P1[:, None] * Y0
    Y0F = Y0.astype(F)
    if H is not None:
        HF = np.asarray(H, dtype=np.float64).astype(F); g = F(sigma2) * F(lle_weight)
        A = A + g * HF @ G; Bm = Bm - g * HF @ Y0F
    if priors is not None and len(priors):
        J = np.zeros(M, dtype=F); Yext = Y0F.copy()
        for r in np.asarray(priors, dtype=np.float64).reshape(-1, 4):
            J[int(r[0])] = 1.0; Yext[int(r[0])] = r[1:]
        A = A + F(alpha) * J[:, None] * G; Bm = Bm + F(alpha) * (Yext - Y0F)
    W = solve(A, Bm)
    T = Y0F + G @ np.asarray(W, dtype=F)
    d = T.astype(LD) - Y.astype(LD)
    num = QL - LD(2) * (d * RL).sum() + (P1L[:, None] * d * d).sum()
    s2 = num / (P1L.sum() * LD(3))
    return (T, s2) if exact else (T, float(s2))
