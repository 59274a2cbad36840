"""k_iter_fused_w0 -- the one-launch iteration of chains whose step slots all fit wave 0 (ChainCarve(M).nSl <= 64: up to 61 nodes; policy FUSE = 3 of
trackdlo_amd/csrc/tdlo_mstep_chain_body.h) -- against k_iter_fused (TDLO_FUSED_W0=0) and against the two-launch loop (TDLO_FUSED_ITER=0).

The new kernel takes the same arithmetic statements in the same order and changes only who holds which value when, so the comparison is for EQUALITY: Y, sigma2,
the iteration count, the kept-point count and the status, as arrays, across the three routes.  The switches are read when a context is made: one context per
route serves every case.  tdlo_debug_route_count(14) counts the registrations the one-launch loop ran, (24) those of them that ran k_iter_fused_w0.

Chain lengths: 8 (nQ = 3: the remainder loops only), 13 (nQ = 4: one unrolled trip), 50 (the headline's), 61 (nSl = 64: every lane of wave 0 a slot, its last
six look-ahead writers as well) on the new kernel; 62 and 64 (nSl = 68) stay on k_iter_fused whatever the switch says.  Cloud sizes: 200 points (a single
workgroup, which is also the writing one) and 5 000 (20 workgroups; not a multiple of 64: the last batch is ragged).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROUTE_FUSED, ROUTE_W0 = 14, 24
ROUTES = {"w0": ("1", None), "fused": ("1", "0"), "two-launch": ("0", None)}      # TDLO_FUSED_ITER, TDLO_FUSED_W0
NMAX = 5000


def _ctx(fused, w0, **kw):
    from trackdlo_amd import binding as B
    want = {"TDLO_FUSED_ITER": fused, "TDLO_FUSED_W0": w0}
    old = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return B.Context(device=0, timing=False, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    made = {}
    try:
        for name, (fused, w0) in ROUTES.items():
            made[name] = _ctx(fused, w0, max_points=NMAX, max_nodes=64)
        yield made
    finally:
        for c in made.values():
            c.close()


def _counts(ctx):
    return int(ctx.lib.tdlo_debug_route_count(ctx.h, ROUTE_FUSED)), int(ctx.lib.tdlo_debug_route_count(ctx.h, ROUTE_W0))


def _kw(**over):
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    kw = dict(beta=P["beta"], lambda_=P["lambda_"], lle_weight=P["lle_weight"], mu=P["mu"], max_iter=30, tol=0.0, include_lle=False, alpha=0.0, k_vis=0.0,
              visibility_threshold=P["visibility_threshold"])
    kw.update(over)
    return kw


def _params(kw):
    from trackdlo_amd import binding as B
    return B.make_params(kw["beta"], kw["lambda_"], kw["lle_weight"], kw["mu"], kw["max_iter"], kw["tol"], kw["include_lle"],
                         kw["alpha"], kw["k_vis"], kw["visibility_threshold"], 0)


def _same(a, b, label):
    assert a["rc"] == b["rc"] and a["status"] == b["status"], (label, a["rc"], b["rc"], a["status"], b["status"])
    assert a["iters"] == b["iters"] and a["n_kept"] == b["n_kept"] and a["converged"] == b["converged"], (label, a["iters"], b["iters"], a["n_kept"], b["n_kept"])
    if a["rc"] == 0:
        assert np.array_equal(np.asarray(a["sigma2"]), np.asarray(b["sigma2"])), (label, a["sigma2"], b["sigma2"])
        assert np.array_equal(a["Y"], b["Y"]), (label, float(np.abs(a["Y"] - b["Y"]).max()))


@pytest.mark.parametrize("N", [200, NMAX])
@pytest.mark.parametrize("M", [8, 13, 50, 61, 62, 64])
def test_three_routes_give_the_same_bits(ctxs, M, N):
    """A fixed iteration count and the launch file's tol (the loop ends early through the mailbox chunks: the same iteration count), each with and without
    correspondence priors.  Up to 61 nodes the default route is the new kernel; 62 and 64 nodes stay on k_iter_fused."""
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    X, Y0 = synth.scene(N, M, config=2)[:2]
    pri = np.array([[1, *(Y0[1] + [0.004, -0.003, 0.002])], [M - 3, *(Y0[M - 3] + [-0.002, 0.005, 0.001])], [M // 2, *Y0[M // 2]]])
    variants = [("fixed", _kw(), False), ("fixed+priors", _kw(alpha=P["alpha"]), True),
                ("early", _kw(max_iter=50, tol=P["tol"]), False), ("early+priors", _kw(max_iter=50, tol=P["tol"], alpha=P["alpha"]), True)]
    fits = M <= 61
    outs = {}
    for name, ctx in ctxs.items():
        before = _counts(ctx)
        outs[name] = [ctx.cpd_lle(X, Y0, 0.0, _params(kw), priors=pri if wp else None) for _, kw, wp in variants]
        took = tuple(a - b for a, b in zip(_counts(ctx), before))
        want = {"w0": (len(variants), len(variants) if fits else 0), "fused": (len(variants), 0), "two-launch": (0, 0)}[name]
        assert took == want, (name, M, N, took, want)
    for i, (vname, kw, _) in enumerate(variants):
        for other in ("fused", "two-launch"):
            _same(outs["w0"][i], outs[other][i], (vname, other, M, N))
        if kw["tol"] == 0.0:
            assert outs["w0"][i]["rc"] == 0 and outs["w0"][i]["iters"] == kw["max_iter"]
    print(f"M={M} N={N}: early-exit iteration counts {[outs['w0'][i]['iters'] for i in (2, 3)]}")


def test_a_registration_that_ends_in_a_numeric_error_ends_the_same_way(ctxs):
    """The scenario of tests/test_fused_iter_gpu.py's test of this name on the new kernel (12 and 30 nodes): inputs far outside the extent the fixed-point sums were
    scaled for.  Same return code, same status, same iteration on the three routes -- and where the call succeeds, the same bits.  At least one of the inputs
    must end in TDLO_E_NUMERIC, or this test checks nothing."""
    from trackdlo_amd import binding as B, synth
    cases = []
    M, N = 12, 600
    X, Y0, _ = synth.scene(N, M, config=811)
    for far, alpha in ((3e4, 1e12), (3e6, 1e12), (3e9, 1e12), (50.0, 3.0)):
        cases.append((f"prior {far:g} m away, alpha {alpha:g}", X, Y0, 0.0, _kw(lambda_=1.0, alpha=alpha, max_iter=8), np.array([[5, Y0[5, 0] + far, Y0[5, 1], Y0[5, 2]]])))
    M2, N2 = 30, 4000
    X2, Y2, _ = synth.scene(N2, M2, config=810)
    Yoff = np.asfortranarray(Y2 + np.array([0.0, 0.09, 0.0]))
    cases.append(("nodes free to fly", X2, Yoff, 0.0, _kw(lambda_=1.0, beta=0.1, max_iter=12), None))
    cases.append(("mu = 0 beside the cloud", X2, Yoff, 1e-6, _kw(mu=0.0, max_iter=12), None))
    outs = {}
    for name, ctx in ctxs.items():
        before = _counts(ctx)
        outs[name] = [ctx.cpd_lle(Xc, Yc, s2, _params(kw), priors=pri, check=False) for _, Xc, Yc, s2, kw, pri in cases]
        took = tuple(a - b for a, b in zip(_counts(ctx), before))
        assert took == {"w0": (len(cases), len(cases)), "fused": (len(cases), 0), "two-launch": (0, 0)}[name], (name, took)
        ok = ctx.cpd_lle(X2, Y2, 0.0, _params(_kw(max_iter=12)))          # the context stays usable
        assert ok["rc"] == 0 and ok["iters"] == 12
    errors = 0
    for i, (cname, *_) in enumerate(cases):
        a = outs["w0"][i]
        print(f"{cname}: rc {a['rc']} status {a['status']} after {a['iters']} iterations")
        for other in ("fused", "two-launch"):
            _same(a, outs[other][i], (cname, other))
        errors += a["rc"] == B.TDLO_E_NUMERIC
    assert errors >= 1
