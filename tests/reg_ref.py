"""Extended-precision reference of `reg` (utils.cpp:21-82, tdlo_reg.hip), the gate its kernels are held to, and the cases.

`reg` is utils.cpp:21-82 in numpy.longdouble on the M x N arrays: the centroids start on the same doubles as tdlo_reg (0.1 / M * i on the y axis),
sigma2 = sum d2 / (3 M N), then max_iter times  P = exp(-d2 / 2 sigma2) / (colsum + c),  Y = (P X) ./ P1,  sigma2 = sum P d2 / (3 sum P)  with d2
from the OLD centroids; exp is taken in longdouble, 0 / 0 gives NaN.  Per iteration it hands the sums P1, PX and Q_m = sum_n P d2 with their absolute
masses (sum p |x|) and argument-weighted masses (sum p |f| (|a_nm| + A_n), a = d2 / 2 sigma2, A_n = sum_m p_nm |a_nm|: the size of the exponents a
membership depends on, its own and -- through the column sum -- its point's) to `move`, which may return what to add to them: the gate is carried
through the iterations that way, on the reference alone.

`gate` is the per-iteration bound of what k_reg_estep / k_reg_mstep may lose on each sum, counted from tdlo_reg.hip (u = 2^-53):
  * a membership's own roundings, relative: the distance (3 subtractions, 3 squares, 2 additions: <= 6), exp (<= 2), the column sum (M - 1
    additions of positive terms, + c, the reciprocal: <= M + 1), c itself (pow and four operations: <= 8, and c <= den + c), the products
    exp * rden and p * f (2), d2 again as the factor of Q (6): K0 = M + 25;
  * the exponent's relative rounding (the distance's 6, k2 = -0.5 / sigma2 and the product: <= 8) times the argument's size: K1 = 8 on the weighted mass;
  * summation, each addition at most u times the absolute mass: six butterfly steps of wsum, one addition per trip and wave (T = trips of the
    grid-stride loop), three additions over the four waves, nblk sequential additions in k_reg_mstep: 6 + T + 3 + nblk;
  * k_reg_mstep's scalars: num and np are M sequential additions and one division more: (M + 2) u of their value (`gate_scalar`);
  * the first sigma2: sum d2 per thread is M sequential additions of distances (M + 6), then the same summation, the division (3).
Nothing in it comes from what a kernel returned."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
RB = 256                   # k_reg_estep's workgroup
MAXBLK = 256               # tdlo_reg: min(ceil(N / 256), 256) workgroups
TRIP = RB * MAXBLK         # 65 536 points: beyond them the E-step's grid-stride loop takes a second trip


def geometry(N):
    nblk = max(1, min(-(-N // RB), MAXBLK))
    return nblk, -(-N // (nblk * RB))                  # workgroups, trips


def start_nodes(M):
    Y = np.zeros((M, 3))
    for i in range(M):
        Y[i, 1] = 0.1 / float(M) * float(i)            # utils.cpp:24-29, the doubles tdlo_reg starts from
    return Y


def _dist2(Y, X):
    dx = Y[:, 0][:, None] - X[:, 0][None, :]; dy = Y[:, 1][:, None] - X[:, 1][None, :]; dz = Y[:, 2][:, None] - X[:, 2][None, :]
    return dx * dx + dy * dy + dz * dz                 # M x N


def reg(X, M, mu=0.05, max_iter=50, move=None, keep=False):
    """Returns dict(Y [M x 3 longdouble], sigma2, iters=[per-iteration sums and masses] when keep).  move(it, s) -> {name: addend} or None; it = -1:
    the first sigma2's sum (s['S0']), it >= 0: s['P1'], s['PX'], s['Q'] and, after those were moved, in a second call, s['num'], s['np']."""
    X = np.asarray(X, dtype=np.float64).astype(LD); N = len(X)
    Y = start_nodes(M).astype(LD)
    log = []
    with np.errstate(all="ignore"):
        S0 = _dist2(Y, X).sum()
        s = dict(S0=S0)
        if move:
            S0 = S0 + LD((move(-1, s) or {}).get("S0", 0.0))
        sigma2 = S0 / (LD(3) * LD(M) * LD(N))
        for it in range(max_iter):
            d2 = _dist2(Y, X)
            a = d2 / (LD(2) * sigma2)
            e = np.exp(-a)
            c = (LD(2) * LD(np.pi) * sigma2) ** LD(1.5) * LD(mu) / (LD(1) - LD(mu)) * LD(M) / LD(N)
            P = e / (e.sum(axis=0) + c)[None, :]
            Pd = P * d2
            s = dict(P1=P.sum(axis=1), PX=P @ X, Q=Pd.sum(axis=1), sigma2=sigma2)
            if move or keep:
                aa = np.abs(a)
                w = aa + (P * aa).sum(axis=0)[None, :]   # a membership's exponent and its point's memberships' mean exponent
                Pw = P * w
                s.update(mP1=s["P1"], mPX=P @ np.abs(X), mQ=s["Q"], wP1=Pw.sum(axis=1), wPX=Pw @ np.abs(X), wQ=(Pd * w).sum(axis=1))
            if move:
                d = move(it, s) or {}
                for k in ("P1", "PX", "Q"):
                    if k in d:
                        s[k] = s[k] + np.asarray(d[k]).astype(LD)
            s["num"] = s["Q"].sum(); s["np"] = s["P1"].sum()
            if move:
                d = move(it, s) or {}
                for k in ("num", "np"):
                    if k in d:
                        s[k] = s[k] + LD(d[k])
            Y = s["PX"] / s["P1"][:, None]
            sigma2 = s["num"] / (s["np"] * LD(3))
            if keep:
                log.append(s)
    return dict(Y=Y, sigma2=sigma2, iters=log)


# ---- the gate -------------------------------------------------------------------------------------------------------------------------
def gate(s, N, M):
    """Per-element gates of one iteration's P1 [M], PX [M x 3], Q [M] (module docstring)."""
    nblk, T = geometry(N)
    k0 = (M + 25.0) + (6.0 + T + 3.0 + nblk); k1 = 8.0
    f = lambda m, w: U * (k0 * np.abs(np.asarray(m, dtype=np.float64)) + k1 * np.abs(np.asarray(w, dtype=np.float64)))
    return dict(P1=f(s["mP1"], s["wP1"]), PX=f(s["mPX"], s["wPX"]), Q=f(s["mQ"], s["wQ"]))


def gate_scalar(s, M):
    return dict(num=U * (M + 2.0) * abs(float(s["num"])), np=U * (M + 2.0) * abs(float(s["np"])))


def gate_first(s, N, M):
    nblk, T = geometry(N)
    return dict(S0=U * ((M + 6.0) + (6.0 + T + 3.0 + nblk) + 3.0) * abs(float(s["S0"])))


def _finite(d):
    return {k: np.where(np.isfinite(v), v, 0.0) for k, v in d.items()}


def propagated(X, M, mu, max_iter, draws=4, seed=7):
    """The longdouble reference, and its gates carried through the iterations: every iteration's sums moved by +- their gates (all +, then random
    signs), 4 x the largest change of Y and of sigma2 seen, floored at 4 u of the value.  Returns (Y, sigma2, gate of Y [M x 3], gate of sigma2)."""
    N = len(X)
    base = reg(X, M, mu, max_iter)
    Yb = base["Y"]; sb = base["sigma2"]
    rng = np.random.default_rng(seed)
    dy = ds = 0.0
    for k in range(draws):
        def move(it, s, k=k):
            if it < 0:
                g = gate_first(s, N, M)
            elif "num" in s:
                g = gate_scalar(s, M)
            else:
                g = gate(s, N, M)
            g = _finite(g)
            return {n: v * (1.0 if k == 0 else rng.choice([-1.0, 1.0], np.shape(v))) for n, v in g.items()}
        r = reg(X, M, mu, max_iter, move=move)
        with np.errstate(invalid="ignore"):
            a = np.abs(r["Y"] - Yb); a = a[np.isfinite(a)]
            dy = max(dy, float(a.max()) if a.size else 0.0)
            b = abs(r["sigma2"] - sb)
            ds = max(ds, float(b) if np.isfinite(b) else 0.0)
    Y = Yb.astype(np.float64); s2 = float(sb)
    with np.errstate(invalid="ignore"):
        gy = np.maximum(4.0 * dy, 4.0 * U * np.abs(Y)); gs = max(4.0 * ds, 4.0 * U * abs(s2))
    return Yb, sb, gy, gs


def ratio(Yg, sg, ref):
    """Worst |kernel - reference| over the gate, for Y and for sigma2; the NaN masks must be equal (asserted)."""
    Yb, sb, gy, gs = ref
    Yg = np.asarray(Yg, dtype=np.float64)
    nan = np.isnan(Yb.astype(np.float64))
    assert np.array_equal(np.isnan(Yg), nan) and np.isnan(sg) == bool(np.isnan(sb)), "NaN masks differ"
    ok = ~nan
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(Yg.astype(LD) - Yb).astype(np.float64)
        qy = float(np.max(np.where(e[ok] == 0, 0.0, e[ok] / gy[ok]))) if ok.any() else 0.0
        es = float(abs(LD(sg) - sb)) if not np.isnan(sg) else 0.0
        qs = 0.0 if es == 0 else es / gs
    return qy, qs


# ---- fp64 restatements ------------------------------------------------------------------------------------------------------------------
def _sum_kernel_order(t, N):
    """Rows of t [K x N] summed as the kernels do: wsum's butterfly per wave, one addition per trip, ((w0 + w1) + w2) + w3, the workgroups in order."""
    nblk, T = geometry(N)
    K = t.shape[0]
    v = np.zeros((K, T * nblk * RB)); v[:, :N] = t
    v = v.reshape(K, T, nblk, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    v = v[..., 0]                                      # K x T x nblk x 4
    my = np.zeros((K, nblk, 4))
    for tr in range(T):
        my = my + v[:, tr]
    part = ((my[..., 0] + my[..., 1]) + my[..., 2]) + my[..., 3]
    acc = np.zeros(K)
    for b in range(nblk):
        acc = acc + part[:, b]
    return acc


def reg_fp64(X, M, mu=0.05, max_iter=50, kernel_order=True):
    """tdlo_reg.hip restated in numpy fp64, operation by operation; kernel_order=False: every sum in numpy's own (pairwise) order."""
    X = np.asarray(X, dtype=np.float64); N = len(X)
    Y = start_nodes(M)
    sm = (lambda t: _sum_kernel_order(t, N)) if kernel_order else (lambda t: t.sum(axis=1))
    with np.errstate(all="ignore"):
        def dist2():
            return [(lambda dx, dy, dz: dx * dx + dy * dy + dz * dz)(Y[m, 0] - X[:, 0], Y[m, 1] - X[:, 1], Y[m, 2] - X[:, 2]) for m in range(M)]
        s = np.zeros(N)
        for q in dist2():
            s = s + q
        sigma2 = sm(s[None, :])[0] / (3.0 * float(M) * float(N))
        for _ in range(max_iter):
            c = np.power(2.0 * np.pi * sigma2, 1.5) * mu / (1.0 - mu) * float(M) / float(N)
            k2 = -0.5 / sigma2
            d2 = dist2()
            den = np.zeros(N)
            for q in d2:
                den = den + np.exp(k2 * q)
            rden = 1.0 / (den + c)
            S = np.zeros((5, M))
            for m, q in enumerate(d2):
                p = np.exp(k2 * q) * rden
                S[:, m] = sm(np.stack([p, p * X[:, 0], p * X[:, 1], p * X[:, 2], p * q]))
            num = npp = 0.0
            for m in range(M):
                num += S[4, m]; npp += S[0, m]
            sigma2 = num / (npp * 3.0)
            Y = (S[1:4] / S[0][None, :]).T.copy()
    return Y, float(sigma2)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def cloud(N, M, cfg=11):
    """synth.scene moved to the origin, as tests/test_parity_gpu.py::test_reg_matches_oracle takes it."""
    from trackdlo_amd import synth
    X, _, _ = synth.scene(N, max(M, 4), config=cfg, frame=N)
    return np.asfortranarray(X - np.array([0.0, 0.0, 0.6]))


NS = [1, 37, 64, 65, 255, 256, 257, 5000]
MS = [1, 2, 5, 8, 30]
ITERS = [0, 1, 2, 5]
MUS = [0.0, 0.05, 0.5, 0.99]


def small_cases():
    """Every (N, M) pair once, max_iter and mu cycled over them: every M meets at least three of the four values of each
    (tests/test_reg_ref.py::test_matrix_covers_what_it_names).  One point (N = 1) is run for 0 and 1 iterations: from the second on its sigma2 is the
    rounding residue of p x / p - x, which no gate can hold (NAN_CASE takes that route on purpose, with coordinates whose residue is exactly 0)."""
    cs = []
    for i, N in enumerate(NS):
        for j, M in enumerate(MS):
            it = ITERS[(i + j) % 4]; mu = MUS[(i + 2 * j + j // 2) % 4]
            if N == 1:
                it = (i + j) % 2
            cs.append(dict(N=N, M=M, mu=mu, it=it))
    return cs


def trip_cases():
    return [dict(N=N, M=5, mu=0.05, it=2) for N in (TRIP, TRIP + 1, TRIP + 321, 2 * TRIP + 65)]


def lds_cases():
    return [dict(N=2000, M=M, mu=0.05, it=2) for M in (356, 357, 890)]


LONG_CASE = dict(N=777, M=5, mu=0.05, it=50)           # the reference's own 50 iterations
NAN_CASE = dict(N=1, M=1, mu=0.05, it=3)


REUSE_CASES = [dict(N=257, M=5, mu=0.05, it=2), dict(N=37, M=5, mu=0.0, it=5)]     # the small steps of the one-context sequence


def cases():
    return small_cases() + trip_cases() + lds_cases() + [LONG_CASE] + REUSE_CASES


def cid(c):
    return f"N{c['N']}-M{c['M']}-mu{c['mu']}-it{c['it']}"


def nan_cloud():
    """One point whose coordinates are 0 or powers of two: p x / p is x in any precision, so the second iteration's d2 is exactly 0, sigma2 becomes 0
    and the third iteration's exponent is 0 * -inf = NaN -- by the reference's own arithmetic, in longdouble and in fp64 alike."""
    return np.asfortranarray(np.array([[0.25, 0.5, -0.125]]))


_REF = {}


def case_ref(c):
    """(X, (Y, sigma2, gate of Y, gate of sigma2)) of a case, computed once per process."""
    k = cid(c)
    if k not in _REF:
        X = cloud(c["N"], c["M"])
        _REF[k] = (X, propagated(X, c["M"], c["mu"], c["it"]))
    return _REF[k]
