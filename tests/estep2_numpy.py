"""Host-side restatement (numpy, fp32) of the data flow of csrc/tdlo_estep2.hip -- test infrastructure.

One wave takes a 128-point batch of the sorted cloud (column c of the batch: lane c's first point below 64, lane c - 64's second from 64 on).
Restated step by step, every operation rounded to fp32 where the kernel's is:

  * the batch's origin o = its first point; lanes of the cloud's last batch without a point take a copy of it and weight zero;
  * ONE candidate range of the nearest-node search for the 128 points; with at most 16 candidates the squared distance carries the
    candidate's offset in its four lowest mantissa bits and comes out without them, beyond 16 the plain first-index argmin;
  * the node-0 rule for all-underflow columns, looked at by the wave together;
  * the second node per point, then ONE window per batch from min lo / max hi / the largest nearest distance / "some pair has the gap";
  * the geodesic argument in its four forms (0: m <= min lo, 1: m >= max hi, 2: per point between them, 3: a gap pair in the wave);
  * exp2, the running sum over the window, the reciprocal, the weights relative to o;
  * the column sums in chunks of TR nodes, slices of 16 (or 32) points in the kernel's order of groups and folds, then the fp64 tail:
    R_k = s_k + (o_k - y_k) P1 and Q's node part d (s + R), each ONE fixed-point conversion; Q's point part Pt1 |x - o|^2 per lane.

It is not bit-exact (v_exp_f32, v_sqrt_f32 and v_rcp_f32 are replaced by the correctly rounded functions, a fused multiply-add by the fp64
product and sum rounded once) -- it is what tests/test_estep_ref.py holds the gate of tests/test_estep_sums_gpu.py to, and `variant` turns
one step into a plausible mistake that the gate must see."""
import numpy as np

F = np.float32
D = np.float64
LD = np.longdouble
LOG2E = 1.4426950408889634
VARIANTS = ("half_range", "gap_one_point", "mode2_in_gap", "no_node0_rule", "no_lv_span", "vis_one_point", "q_cross_dropped",
            "q_cross_sign", "tail_copies_weighted", "first_chunk_only")


def _fma(a, b, c):
    return (np.asarray(a, dtype=D) * np.asarray(b, dtype=D) + np.asarray(c, dtype=D)).astype(F)


def _d2_fma(P, q):
    """fma(dz, dz, fma(dy, dy, dx dx)) of points P [n, 3] against nodes q [w, 3] -> [n, w]."""
    dx = P[:, None, 0] - q[None, :, 0]; dy = P[:, None, 1] - q[None, :, 1]; dz = P[:, None, 2] - q[None, :, 2]
    return _fma(dz, dz, _fma(dy, dy, dx * dx))


def _d2_plain(P, q):
    dx = P[:, None, 0] - q[None, :, 0]; dy = P[:, None, 1] - q[None, :, 1]; dz = P[:, None, 2] - q[None, :, 2]
    return dx * dx + dy * dy + dz * dz


def _slice_groups(shift):
    """[slice, 4-point group] in the order a lane's `four` calls take them."""
    if shift == 3:
        return [[(((sl & 1) << 3) | (sl >> 1)) | ((i & 1) << 4) | ((i >> 1) << 2) for i in range(4)] for sl in range(8)]
    return [[sl * 8 + i for i in range(8)] for sl in range(4)]


def _column_sums(p, w, shift):
    """sum_c p[c, node] w[c] over the 128 columns: per slice two fp32 accumulators (even / odd columns of a group, fused), their sum, the folds."""
    groups = _slice_groups(shift)
    parts = []
    for gl in groups:
        ax = np.zeros(p.shape[1], dtype=F); ay = np.zeros(p.shape[1], dtype=F)
        for g4 in gl:
            c = 4 * g4
            ax = _fma(p[c], w[c], ax); ay = _fma(p[c + 1], w[c + 1], ay)
            ax = _fma(p[c + 2], w[c + 2], ax); ay = _fma(p[c + 3], w[c + 3], ay)
        parts.append(ax + ay)
    if shift == 3:
        f32 = [parts[i] + parts[i + 4] for i in range(4)]
        f16 = [f32[0] + f32[2], f32[1] + f32[3]]
    else:
        f16 = [parts[0] + parts[2], parts[1] + parts[3]]
    return f16[0] + f16[1]


def _fix(v, sh):
    return np.rint(np.asarray(v, dtype=D) * 2.0 ** sh).astype(np.int64)


def estep2(Xs, Y, coord, sigma2, c_norm, sh, TR, win_e=36.0, vis=None, variant=None):
    """Xs [N, 3]: the kept points in the kernel's order (fp32 values); Y [M, 3], coord [M]: the nodes and the chain coordinate (fp32 values);
    sh = (sP, sR, sQ): the fixed point's exponents; vis = dict(dq=per-node d_min^2, k_vis=, thr=) for the visibility branch.
    Returns ([P1 | R column-major | Q] as longdouble, info)."""
    assert variant is None or variant in VARIANTS
    Xs = np.asarray(Xs).astype(F); Y = np.asarray(Y).astype(F); cw_ = np.asarray(coord).astype(F)
    N, M = len(Xs), len(Y)
    k2 = F(-LOG2E / (2.0 * sigma2)); cn = F(c_norm)
    rwin = win_e * 1.3862943611198906 * sigma2
    lv = None; lv_span = 0.0
    if vis is not None:
        d = np.sqrt(np.asarray(vis["dq"]).astype(F).astype(D))
        d = np.where(d > 10000.0, 10000.0, d); d = np.where(d <= vis["thr"], 0.0, d)
        tot = np.exp(-vis["k_vis"] * d).sum()
        lv_span = max(vis["k_vis"] * (d.max() - d.min()) * LOG2E, 0.0)
        lv = (-vis["k_vis"] * d * LOG2E - np.log2(tot)).astype(F)
        if variant == "no_lv_span":
            lv_span = 0.0
    R2win = F(rwin * (1.0 + lv_span / win_e))
    under_thr = F(-1075.0) / k2
    sP, sR, sQ = sh
    accP = np.zeros(M, dtype=np.int64); accR = np.zeros((3, M), dtype=np.int64); accQ = 0
    info = dict(cands=[], window=[], modes=set(), chunks=[], underflow_batches=0, gap_batches=0)
    first64 = np.arange(128) < 64
    for b in range(-(-N // 128)):
        base = b * 128
        n = min(128, N - base)
        valid = np.arange(128) < n
        P = np.empty((128, 3), dtype=F); P[:n] = Xs[base:base + n]; P[n:] = Xs[base]
        o = P[0].copy()
        e = P - o[None, :]
        r2v = _fma(e[:, 2], e[:, 2], _fma(e[:, 1], e[:, 1], e[:, 0] * e[:, 0]))
        # ---- the candidate range
        rsel = first64 if variant == "half_range" else np.ones(128, dtype=bool)
        dd = Y - o[None, :]
        Dm = dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2]
        lim = (np.sqrt(Dm.min()) + F(2) * np.sqrt(r2v[rsel].max())) * F(1.0001) + F(1e-30)
        lim = lim * lim
        cand = np.nonzero(Dm <= lim)[0]
        plo, phi = (int(cand[0]), int(cand[-1])) if len(cand) else (0, M - 1)
        info["cands"].append(phi - plo + 1)
        d2 = _d2_fma(P, Y[plo:phi + 1])
        if phi - plo < 16:
            key = (d2.view(np.uint32) & np.uint32(0xfffffff0)) | np.arange(phi - plo + 1, dtype=np.uint32)[None, :]
            kmin = key.min(axis=1)
            a = plo + (kmin & np.uint32(15)).astype(np.int64)
            best = (kmin & np.uint32(0xfffffff0)).view(F)
        else:
            a = plo + d2.argmin(axis=1)
            best = d2.min(axis=1)
        # ---- all-underflow columns take node 0
        if variant != "no_node0_rule" and (best > under_thr).any():
            d0 = _d2_plain(P, Y[0:1])[:, 0]
            u_ = best * k2 < F(-1075.0)
            a = np.where(u_, 0, a); best = np.where(u_, d0, best)
            info["underflow_batches"] += 1
        # ---- the second node
        c1 = np.where(a == 0, 2, a - 1); c2 = np.where(a == M - 1, M - 3, a + 1)
        rows = np.arange(128)
        s1 = _d2_plain(P, Y)[rows, c1]; s2 = _d2_plain(P, Y)[rows, c2]
        first = s1 < s2
        eb = np.sqrt(np.where(first, s1, s2)); bb = np.where(first, c1, c2); cb = cw_[bb]
        ea = np.sqrt(best); ca = cw_[a]
        a_lo = a < bb
        lo = np.where(a_lo, a, bb); hi = np.where(a_lo, bb, a)
        DLO = np.where(a_lo, ea, eb); DHI = np.where(a_lo, eb, ea)
        CLO = np.where(a_lo, ca, cb); CHI = np.where(a_lo, cb, ca)
        # ---- the wave's window
        wsel = first64 if variant == "half_range" else np.ones(128, dtype=bool)
        min_lo = int(lo[wsel].min()); max_hi = int(hi[wsel].max()); bmx = best[wsel].max()
        gsel = first64 if variant == "gap_one_point" else np.ones(128, dtype=bool)
        adj = not bool((hi - lo != 1)[gsel].any())
        if not adj:
            info["gap_batches"] += 1
        if variant == "mode2_in_gap":
            adj = True
        Rwin = np.sqrt(F(bmx + R2win))
        inw = np.nonzero((cw_ > cw_[min_lo] - Rwin) & (cw_ < cw_[max_hi] + Rwin))[0]
        wlo, whi = (int(inw[0]), int(inw[-1])) if len(inw) else (0, M - 1)
        W = whi - wlo + 1
        info["window"].append(W)
        # ---- memberships [128, W] and their running sum
        p = np.empty((128, W), dtype=F)
        s = np.zeros(128, dtype=F)
        for m in range(wlo, whi + 1):
            qw = cw_[m]
            if not adj:
                tl = (CLO - qw) + DLO; th = (qw - CHI) + DHI
                t = np.where(m <= lo, tl, F(0)); t = np.where(m >= hi, th, t); mode = 3
            elif m <= min_lo:
                t = (CLO - qw) + DLO; mode = 0
            elif m >= max_hi:
                t = (qw - CHI) + DHI; mode = 1
            else:
                sl_ = m <= lo
                t = np.abs(qw - np.where(sl_, CLO, CHI)) + np.where(sl_, DLO, DHI); mode = 2
            info["modes"].add(mode)
            ex = (t * t) * k2
            if lv is not None:
                ex = np.where(first64, ex + lv[m], ex) if variant == "vis_one_point" else ex + lv[m]
            pm = np.exp2(ex.astype(D)).astype(F)
            s = s + pm
            p[:, m - wlo] = pm
        inv = (1.0 / (s + cn).astype(D)).astype(F)
        if variant != "tail_copies_weighted":
            inv = np.where(valid, inv, F(0))
        qvv = (inv * s) * r2v
        accQ += int(_fix((qvv[:64] + qvv[64:]).astype(D), sQ).sum())
        w = np.stack([inv, inv * e[:, 0], inv * e[:, 1], inv * e[:, 2]])          # [4, 128]
        # ---- column sums, the window in chunks of TR nodes
        nch = 0
        for c0 in range(0, W, TR):
            if variant == "first_chunk_only" and c0 > 0:
                break
            nch += 1
            Wn = min(TR, W - c0)
            shift = 3 if (TR <= 8 or Wn <= 8) else 4
            pc = p[:, c0:c0 + Wn]
            s0 = _column_sums(pc, w[0][:, None], shift).astype(D)
            nodes = np.arange(wlo + c0, wlo + c0 + Wn)
            accP[nodes] += _fix(s0, sP)
            for k in range(3):
                u = _column_sums(pc, w[1 + k][:, None], shift).astype(D)
                dk = D(o[k]) - Y[nodes, k].astype(D)
                val = dk * s0 + u
                accR[k, nodes] += _fix(val, sR)
                if variant == "q_cross_dropped":
                    dq = dk * (val - u)
                elif variant == "q_cross_sign":
                    dq = dk * (val - 3.0 * u)
                else:
                    dq = dk * (u + val)
                accQ += int(_fix(dq, sQ).sum())
        info["chunks"].append(nch)
    out = np.concatenate([accP.astype(LD) * LD(2.0) ** -sP, accR.reshape(-1).astype(LD) * LD(2.0) ** -sR, [LD(accQ) * LD(2.0) ** -sQ]])
    return out, info
