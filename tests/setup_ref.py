"""The set-up stage of trackdlo::cpd_lle restated exactly (tests only): which points exist, in which order, around which origin
and in which precision they are stored, the sigma2 a registration starts from, the chain coordinate and the state-space links.

This is the stage the kernels k_prune_pass1 / k_setup / k_prune_scatter and their one-launch form k_prologue implement
(trackdlo.cpp:177-273, :214-233).  Nothing here is taken from them:

  * `decide`: the prune and the nearest node in the oracle's fp64 formula (a*a + b*b + c*c on the fp64 differences y - x, numpy: no
    contraction), and each decision's MARGIN from the same sum of squares in np.longdouble formed from the fp64 differences (y - x rounds
    the same way in every evaluation; only the products and sums depend on how they are evaluated).  A decision is PINNED when its margin
    exceeds 8 u (u = 2^-53): three products, two sums, with or without fused multiply-adds, move a d2 by less than 4 u relative, so two
    evaluations cannot disagree about a comparison whose operands are more than 8 u apart.  The longdouble margins are only formed for
    points whose fp64 margin is below 2^-30: above it the fp64 value's own 4 u already prove the margin.
  * `sorted_order`: kept points by (nearest node, original index) -- the stable counting sort -- and the per-node run starts.
  * `centroid`, `stored`: the centring offset in longdouble; the stored coordinates fl_T(fl64(x - ctr)) for the offset the device reports.
  * `sigma2_0`: sum of d2 over kept points and all nodes in longdouble (estep_ref.sum_d2) / (3 M N).
  * `links`, `row0`: Phi, Q of a gap h and Pinf as documented above chain_link (tdlo_devcommon.h) in longdouble, the positive series
    summed to convergence for EVERY x (no switch at x = 1); `hy0`: H Y0 from the 13 diagonals with the mass of every element.
"""
import numpy as np

import estep_ref as R

LD = np.longdouble
U = 2.0 ** -53
PIN = 8.0 * U                    # a margin above this pins a decision
SCREEN = 2.0 ** -30              # fp64 margins above this are not re-evaluated in longdouble (4 u << 2^-30)


def threshold():
    """The smallest fp64 t whose correctly rounded square root is >= 0.1: sqrt(d2) < 0.1 <=> d2 < t.  Bisection on the bit patterns
    (positive doubles are ordered like their bits)."""
    lo = np.array([0.009], dtype=np.float64).view(np.int64)[0]; hi = np.array([0.011], dtype=np.float64).view(np.int64)[0]
    assert np.sqrt(0.009) < 0.1 <= np.sqrt(0.011)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        v = np.array([mid], dtype=np.int64).view(np.float64)[0]
        if np.sqrt(v) >= 0.1:
            hi = mid
        else:
            lo = mid
    return float(np.array([hi], dtype=np.int64).view(np.float64)[0])


T_KEEP = threshold()


def decide(X, Y0, exact=False, chunk=4096):
    """Per point: kept, nearest (first index of the minimum; -1 where not kept), the margins and which decisions are pinned.
    exact=True: the caller vouches that every difference, product and sum is exact in fp64 (grid scenes): everything is pinned, ties
    included; `ties` then counts the points whose two smallest d2 are EQUAL."""
    X = np.asarray(X, dtype=np.float64); Y0 = np.asarray(Y0, dtype=np.float64)
    N, M = len(X), len(Y0)
    kept = np.zeros(N, dtype=bool); nearest = np.full(N, -1, dtype=np.int64)
    m_thr = np.full(N, np.inf); m_tie = np.full(N, np.inf); tie = np.zeros(N, dtype=bool); dmin = np.full(N, np.inf)
    t = T_KEEP; tL = LD(t)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, N, chunk):
            x = X[s:s + chunk]
            a = Y0[None, :, 0] - x[:, 0:1]; b = Y0[None, :, 1] - x[:, 1:2]; c = Y0[None, :, 2] - x[:, 2:3]
            d2 = a * a + b * b + c * c
            d2 = np.where(np.isnan(d2), np.inf, d2)               # a NaN never wins a strict comparison
            best = d2.min(axis=1); arg = d2.argmin(axis=1)
            k = np.sqrt(best) < 0.1
            dmin[s:s + chunk] = best
            kept[s:s + chunk] = k
            nearest[s:s + chunk] = np.where(k, arg, -1)
            mt = np.abs(best / t - 1.0)
            if M > 1:
                two = np.partition(d2, 1, axis=1)[:, :2]
                with np.errstate(divide="ignore"):
                    mq = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / np.where(two[:, 1] > 0, two[:, 1], 1.0), 0.0)
                tie[s:s + chunk] = k & (two[:, 1] == two[:, 0])
            else:
                mq = np.full(len(x), np.inf)
            mq = np.where(k, mq, np.inf)                          # the nearest node of a pruned point decides nothing
            mt = np.where(np.isfinite(best), mt, np.inf)
            close = np.nonzero((mt < SCREEN) | (mq < SCREEN))[0]
            if len(close) and not exact:
                aL = a[close].astype(LD); bL = b[close].astype(LD); cL = c[close].astype(LD)
                d2L = aL * aL + bL * bL + cL * cL
                srt = np.sort(d2L, axis=1)
                mt[close] = np.abs(srt[:, 0] / tL - LD(1)).astype(np.float64)
                if M > 1:
                    q = np.where(srt[:, 1] > 0, (srt[:, 1] - srt[:, 0]) / np.where(srt[:, 1] > 0, srt[:, 1], LD(1)), LD(0)).astype(np.float64)
                    mq[close] = np.where(k[close], q, np.inf)
            m_thr[s:s + chunk] = mt; m_tie[s:s + chunk] = mq
    if exact:
        pinned = np.ones(N, dtype=bool)
    else:
        pinned = (m_thr > PIN) & (m_tie > PIN)
    return dict(kept=kept, nearest=nearest, m_thr=m_thr, m_tie=m_tie, pinned=pinned, ties=tie, dmin=dmin)


def sorted_order(kept, nearest, M):
    """Original indices of the kept points in (nearest node, original index) order, and where each node's run starts (M + 1 entries)."""
    idx = np.nonzero(kept)[0]
    o = np.argsort(nearest[idx], kind="stable")
    order = idx[o]
    starts = np.searchsorted(nearest[order], np.arange(M + 1))
    return order, starts


def centroid(Y0):
    Y = np.asarray(Y0, dtype=np.float64).astype(LD)
    return Y.sum(axis=0) / LD(len(Y))


def stored(P, ctr, fp32):
    """fl_T(fl64(p - ctr)) for the fp64 offset the device reports: exact, no gate."""
    v = np.asarray(P, dtype=np.float64) - np.asarray(ctr, dtype=np.float64)[None, :]
    return v.astype(np.float32).astype(np.float64) if fp32 else v


def sigma2_0(X, Y0, kept):
    """(sum of d2 over kept points and all nodes, sigma2_0 = sum / (3 M N)) in longdouble (trackdlo.cpp:263-273)."""
    n = int(np.count_nonzero(kept))
    sd = R.sum_d2(np.asarray(X, dtype=np.float64)[kept], Y0) if n else LD(0)
    return sd, (sd / LD(3 * len(Y0) * n) if n else LD(0))


def chain_exact(Y0):
    """The chain coordinate to longdouble accuracy (the first row of estep_ref.chain_gaps_exact)."""
    return R.chain_gaps_exact(Y0)[0]


# ---- the links ---------------------------------------------------------------------------------------------------------------
def _tail3(tt):
    """sum_{n >= 3} tt^n / n!  (tt >= 0) in longdouble, summed until the terms no longer change the sum."""
    tt = LD(tt)
    term = tt * tt * tt / LD(6); tot = term
    n = 3
    while True:
        n += 1
        term = term * tt / LD(n)
        new = tot + term
        if new == tot:
            return tot
        tot = new


def links(h, beta):
    """{Phi11, Phi12, Phi21, Phi22, Q11, Q12, Q22} of the gap h >= 0 (fp64 value), longdouble:
         Phi = e^-x [[1 + x, h], [-s^2 h, 1 - x]],  x = s h,  s = sqrt2 / beta,  sf2 = 1 / (2 sqrt2 beta),
         Q11 = sf2 (1 - e^-2x (1 + 2x + 2x^2)) = sf2 e^-2x sum_{n >= 3} (2x)^n / n!,
         Q12 = 2 sf2 s^3 h^2 e^-2x,
         Q22 = sf2 s^2 (1 - e^-2x (1 - 2x + 2x^2)) = sf2 s^2 e^-2x (4x + sum_{n >= 3} (2x)^n / n!).
    The series form is used while 2x <= 40 (it has only positive terms and converges for every x; at 2x = 40 its largest term is 1e16 times
    the first and longdouble still leaves 2^-64 relative); beyond, e^-2x < 2^-57 and the closed form loses nothing."""
    h = LD(h); b = LD(beta)
    r2 = np.sqrt(LD(2))
    s = r2 / b; sf2 = LD(1) / (LD(2) * r2 * b)
    x = s * h
    e = np.exp(-x); e2 = np.exp(-LD(2) * x)
    if 2 * x <= 40:
        t3 = _tail3(LD(2) * x)
        u11 = e2 * t3; u22 = e2 * (LD(4) * x + t3)
    else:
        u11 = LD(1) - e2 * (LD(1) + LD(2) * x + LD(2) * x * x); u22 = LD(1) - e2 * (LD(1) - LD(2) * x + LD(2) * x * x)
    return np.array([e * (LD(1) + x), e * h, -s * s * h * e, e * (LD(1) - x), sf2 * u11, LD(2) * sf2 * s * s * s * h * h * e2, sf2 * s * s * u22],
                    dtype=LD), dict(x=x, e=e, e2=e2, s=s, sf2=sf2, u11=u11, u22=u22)


def row0(beta):
    """{Pinf11, Pinf22, 1 / Pinf11, 1 / Pinf22}: Pinf = sf2 diag(1, s^2)."""
    b = LD(beta); r2 = np.sqrt(LD(2))
    s = r2 / b; sf2 = LD(1) / (LD(2) * r2 * b)
    return np.array([sf2, s * s * sf2, LD(1) / sf2, LD(1) / (s * s * sf2)], dtype=LD)


def band_of(H):
    """Hb[i, u] = H[i, i - 6 + u] (zero outside the matrix): the 13 diagonals the banded M-step is given."""
    H = np.asarray(H, dtype=np.float64); M = len(H)
    Hb = np.zeros((M, 13))
    for i in range(M):
        for u in range(13):
            k = i - 6 + u
            if 0 <= k < M:
                Hb[i, u] = H[i, k]
    return Hb


def hy0(Hb, Y0):
    """(H Y0 [M x 3], its mass sum_k |H_ik y_kd|) from the 13 diagonals, longdouble; Y0: the nodes as handed in (NOT centred)."""
    Hb = np.asarray(Hb, dtype=np.float64).astype(LD); Y = np.asarray(Y0, dtype=np.float64).astype(LD)
    M = len(Y)
    out = np.zeros((M, 3), dtype=LD); mass = np.zeros((M, 3), dtype=LD)
    for i in range(M):
        for u in range(13):
            k = i - 6 + u
            if 0 <= k < M:
                out[i] += Hb[i, u] * Y[k]; mass[i] += np.abs(Hb[i, u] * Y[k])
    return out, mass


# ---- the gates of the links: counted from the expressions of chain_link (tdlo_devcommon.h) --------------------------------------
def link_gates(h, beta):
    """Absolute gates of the seven entries, u = 2^-53 per rounding (a fused multiply-add only removes roundings):
         s = sqrt(2) / beta: 2 u.  sf2 = 1 / (2 sqrt(2) beta): 3 u (sqrt, product, reciprocal; the factor 2 is exact).
         x = s h: 3 u.  e = exp(-x): the argument's 3 u x plus ocml's 1 ulp = 2 u -> (2 + 3x) u.  e2 = e e: (5 + 6x) u.
         Phi11 = e (1 + x): 1 + x 4 u, product 1 -> (7 + 3x) u.        Phi12 = e h: (3 + 3x) u.
         Phi21 = -s s h e: s s 5 u, h 6 u, e -> (9 + 3x) u.
         Phi22 = e (1 - x): 1 - x cancels -- its ABSOLUTE error is 3 u x + u |1 - x| -> u e (3x + |1 - x| (4 + 3x)).
         x < 1, series: tt = 2x 3 u; term_3 = tt tt tt / 6: 12 u; every further term 6 u more (tt (1 / n): 5 u, product 1), weighted by the
           terms' sizes (tt < 2) <= 5 u; 30 additions of positive terms <= 30 u: sum 47 u.
           u11 = e2 sum: (53 + 6x) u.  Q11 = sf2 u11: (57 + 6x) u.
           u22 = e2 (4x + sum): 4x 3 u, sum <= 48 u -> (54 + 6x) u.  Q22 = sf2 s s u22: sf2 s 6 u, s 9 u, product -> (64 + 6x) u.
         x >= 1, closed form: p = 1 + 2x + 2x x: 8 u; w = e2 p: (14 + 6x) u; u11 = 1 - w: ABSOLUTE w (14 + 6x) u + u u11.  Q11: 4 u more.
           p2 = 1 - 2x + 2x x: absolute u (6x + |1 - 2x| + 14 x^2 + p2); w2 = e2 p2: that over p2 plus (6 + 6x) u; u22 = 1 - w2: absolute
           w2 rel(w2) + u u22.  Q22 = sf2 s s u22: 10 u more.
         Q12 = 2 sf2 s s s h h e2: 3, 6, 9, 12, 13, 14 u, e2 -> (20 + 6x) u.
       Where e (e2) is subnormal or zero in fp64 its error is 2^-1074 absolute, carried through the products: + 2^-1074 (|coefficient| + 1)."""
    v, q = links(h, beta)
    x = float(q["x"]); hh = float(h); s = float(q["s"]); sf2 = float(q["sf2"])
    a = np.abs(v).astype(np.float64)
    e = float(q["e"]); e2 = float(q["e2"])
    g = np.zeros(7)
    g[0] = a[0] * (7 + 3 * x) * U; g[1] = a[1] * (3 + 3 * x) * U; g[2] = a[2] * (9 + 3 * x) * U
    g[3] = U * e * (3 * x + abs(1 - x) * (4 + 3 * x))
    x64 = (np.sqrt(2.0) / np.float64(beta)) * np.float64(h)      # which expression the fp64 code evaluates: its own x (one division, one product)
    if x64 < 1.0:
        g[4] = a[4] * (57 + 6 * x) * U; g[6] = a[6] * (64 + 6 * x) * U
    else:
        p = 1 + 2 * x + 2 * x * x; w = e2 * p; u11 = float(q["u11"])
        g[4] = sf2 * (w * (14 + 6 * x) * U + U * u11) + a[4] * 4 * U
        p2 = 1 - 2 * x + 2 * x * x; w2 = e2 * p2; u22 = float(q["u22"])
        rel2 = U * (6 * x + abs(1 - 2 * x) + 14 * x * x + p2) / p2 + (6 + 6 * x) * U
        g[6] = sf2 * s * s * (w2 * rel2 + U * u22) + a[6] * 10 * U
    g[5] = a[5] * (20 + 6 * x) * U
    tiny = 2.0 ** -1074
    if e < 2.0 ** -1021:
        g[0] += tiny * (1 + x + 1); g[1] += tiny * (hh + 1); g[2] += tiny * (s * s * hh + 1); g[3] += tiny * (abs(1 - x) + 1)
    if e2 < 2.0 ** -1021:
        g[5] += tiny * (2 * sf2 * s ** 3 * hh * hh + 1)
    return v, g


ROW0_GATE = np.array([3.0, 9.0, 4.0, 10.0]) * U      # sf2: 3 u; s s sf2: 5 + 3 + 1; the reciprocals one more each
