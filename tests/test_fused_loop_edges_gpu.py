"""The one-launch EM loop (k_iter_fused, k_iter_fused_w0; trackdlo_amd/csrc/tdlo_iter_fused.hip) on hard scenes and at every edge of its loop, against the
two-launch loop it replaces.  tests/test_fused_iter_gpu.py and tests/test_fused_w0_gpu.py hold the arithmetic on a benign scene; this file holds what exists on
this route alone: the M-step prologue of policies FUSE 1 and 3, the no-op branch of a finished registration, and the rotation of state copies (k & 1),
accumulator buffers (k % 3) and error words on the host and the device.

The routes are those of test_fused_w0_gpu.py (one context each, made under TDLO_FUSED_ITER / TDLO_FUSED_W0), and every comparison across them is for EQUALITY:
return code, status, iterations, converged flag, kept points, sigma2 and Y as arrays.  Every test asserts the route it took with tdlo_debug_route_count(14) (the
registrations the one-launch loop ran) and (24) (those of them that launched k_iter_fused_w0: up to 61 nodes and at least two iterations enqueued -- a
registration of one iteration is k_estep and the closing k_mstep_chain).  The scenes and their claims: tests/fused_scenes.py, proved by
tests/test_fused_scenes_ref.py."""
import functools

import numpy as np
import pytest

import fused_scenes as FS
from test_fused_w0_gpu import ROUTES, _counts, _ctx, _params, _same
from test_parity_gpu import TOL

pytestmark = pytest.mark.gpu

NMAX = 65537
W0_MAX_NODES = 61


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


def _fresh(route, X, Y0, sigma2, kw, priors=None):
    """The registration on a context made for it alone."""
    fused, w0 = ROUTES[route]
    ctx = _ctx(fused, w0, max_points=max(len(X), 64), max_nodes=64)
    try:
        return ctx.cpd_lle(X, Y0, sigma2, _params(kw), priors=priors, check=False)
    finally:
        ctx.close()


def _want(route, M, calls, launched):
    """Route counter increments of `calls` registrations of the one-launch loop's kind, `launched` of which enqueued a one-launch iteration."""
    if route == "two-launch" or not 8 <= M <= 64:
        return (0, 0)
    return (calls, launched if route == "w0" and M <= W0_MAX_NODES else 0)


class _Routes:
    """with _Routes(ctx, route, M) as r: ...; r.expect(calls, launched) -- asserts the counters' increments when the block ends."""
    def __init__(self, ctx, route, M):
        self.ctx, self.route, self.M, self.calls, self.launched = ctx, route, M, 0, 0

    def __enter__(self):
        self.before = _counts(self.ctx)
        return self

    def expect(self, calls, launched):
        self.calls += calls; self.launched += launched

    def __exit__(self, et, ev, tb):
        if et is None:
            took = tuple(a - b for a, b in zip(_counts(self.ctx), self.before))
            assert took == _want(self.route, self.M, self.calls, self.launched), (self.route, self.M, took, _want(self.route, self.M, self.calls, self.launched))
        return False


@functools.lru_cache(maxsize=None)
def _oracle_end(name, M):
    from oracle import ref_cpu
    sc = FS.HARD[name](M)
    return ref_cpu.cpd_lle(sc["X"], sc["Y0"], sc["sigma2_in"], priors=sc["priors"], **dict(sc["kw"], max_iter=FS.ITERS[-1], tol=0.0))


# ---- hard scenes, the whole trajectory ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", FS.CHAINS)
@pytest.mark.parametrize("name", sorted(FS.HARD))
def test_hard_scenes_iteration_by_iteration(ctxs, name, M):
    """max_iter = 1 .. 8 with tol = 0 on the three routes: 1 is k_estep and the closing k_mstep_chain with no one-launch iteration, 2 is one of them, 3 rotates
    the buffers once, 4 .. 8 go through every residue of the rotation.  The two-launch result of max_iter = 8 is held to the oracle at the project's stated fp32
    gate (test_parity_gpu.TOL[0]: 1e-5 m, 1e-3 relative on sigma2, iterations and kept points exact), so that equal bits mean something on this scene."""
    sc = FS.HARD[name](M)
    outs = {}
    for route, ctx in ctxs.items():
        with _Routes(ctx, route, M) as r:
            outs[route] = [ctx.cpd_lle(sc["X"], sc["Y0"], sc["sigma2_in"], _params(dict(sc["kw"], max_iter=it, tol=0.0)), priors=sc["priors"], check=False)
                           for it in FS.ITERS]
            r.expect(len(FS.ITERS), sum(it >= 2 for it in FS.ITERS))
    for i, it in enumerate(FS.ITERS):
        a = outs["two-launch"][i]
        assert a["rc"] == 0 and a["iters"] == it and not a["converged"], (name, M, it, a["rc"], a["status"], a["iters"])
        for other in ("w0", "fused"):
            _same(outs[other][i], a, (name, M, it, other))
    g, o = outs["two-launch"][-1], _oracle_end(name, M)
    dy = float(np.abs(g["Y"] - o["Y"]).max()); ds = abs(g["sigma2"] - o["sigma2"]) / o["sigma2"]
    print(f"{name} M={M} N={len(sc['X'])}: two-launch against the oracle after {o['iters']} iterations: max |dY| {dy:.3g} m, |d sigma2| / sigma2 {ds:.3g}, "
          f"kept {g['n_kept']} / {o['n_kept']}")
    assert g["iters"] == o["iters"] and g["n_kept"] == o["n_kept"] and g["converged"] == o["converged"]
    assert dy <= TOL[0][0] and ds <= TOL[0][1], (name, M, dy, ds)


# ---- an early exit in every launch ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_priors", [False, True], ids=["plain", "priors"])
def test_an_early_exit_in_every_launch(ctxs, oracle, with_priors):
    """The ladder of tests/test_fused_scenes_ref.py (scene d at 13 nodes; once more with the priors of scene c): the run with tol_k and max_iter = 30 ends after
    the oracle's iteration count for it, k, with `converged` set and equal bits on the three routes -- six and more consecutive k: every residue of the state
    copies and of the accumulator buffers sees the exit, and the no-op launches behind it pass the result on through 1 .. 3 hand-overs and more.  After each
    early exit a second call on the same context and slot (tol = 0, three iterations, the sorted cloud reused) gives the bits of a context made for it: a
    stale state copy, or a done flag handed on through the no-op launches, would show here."""
    from test_fused_scenes_ref import ladder_scene
    sc, ladder, crit = ladder_scene(oracle, with_priors)
    assert len(ladder) >= FS.LADDER_RUNGS
    M = len(sc["Y0"])
    kw3 = dict(sc["kw"], max_iter=3, tol=0.0)
    fresh = {route: _fresh(route, sc["X"], sc["Y0"], sc["sigma2_in"], kw3, sc["priors"]) for route in ctxs}
    for route in ("w0", "fused"):
        _same(fresh[route], fresh["two-launch"], ("fresh", route))
    assert fresh["two-launch"]["rc"] == 0 and fresh["two-launch"]["iters"] == 3
    for k, tol in ladder:
        outs = {}
        for route, ctx in ctxs.items():
            with _Routes(ctx, route, M) as r:
                first = ctx.cpd_lle(sc["X"], sc["Y0"], sc["sigma2_in"], _params(dict(sc["kw"], max_iter=30, tol=tol)), priors=sc["priors"], check=False)
                again = ctx.cpd_lle_resident(0, sc["Y0"], sc["sigma2_in"], _params(kw3), priors=sc["priors"], check=False)
                r.expect(2, 2)
            outs[route] = (first, again)
            assert again["sort_reused"] == 1, (route, k, again["sort_reused"])
            _same(again, fresh[route], ("after the exit in iteration", k, route))
        a = outs["two-launch"][0]
        print(f"tol {tol:.4g}: the oracle ends after {k} iterations (crit {crit[k - 1]:.3g}), the two-launch loop after {a['iters']}, converged {a['converged']}")
        for route in ("w0", "fused", "two-launch"):
            b = outs[route][0]
            assert b["rc"] == 0 and b["iters"] == k and b["converged"], (route, k, b["rc"], b["iters"], b["converged"])
            _same(b, a, ("exit in iteration", k, route))


# ---- buffers and state copies left dirty by the call before, the sorted cloud reused -----------------------------------------------------------------------------
SEQUENCE = (1, 2, 3, 4, 5, 6, 7, 3, 1, 30, 2)
_FRESH_SEQ = {}


def _fresh_seq(route, N, X, Y0, it):
    if (route, N, it) not in _FRESH_SEQ:
        _FRESH_SEQ[(route, N, it)] = _fresh(route, X, Y0, 0.0, FS.base_kw(max_iter=it))
    return _FRESH_SEQ[(route, N, it)]


@pytest.mark.parametrize("between", [False, True], ids=["fused-only", "ineligible-between"])
@pytest.mark.parametrize("N", [700, 20000])
def test_dirty_buffers_with_the_sorted_cloud_reused(ctxs, N, between):
    """One resident slot, the same nodes every call, sort reuse at its default (on): max_iter = 1, 2, 3, 4, 5, 6, 7, 3, 1, 30, 2 -- every registration starts on
    the accumulator buffers, state copies and error words the one before left, after every residue of the rotation -- and each call equals the same max_iter on
    a context made for it.  between: a registration the one-launch loop does not take runs on the same slot before every call, alternately in fp64 mode and
    with the visibility term (they use the two-parity accumulators and the first state copy only; a call behind the fp64 one sorts again -- the sort is kept
    per precision -- every other call reuses the sort).  700 points take the one-kernel set-up, 20 000 the three-kernel one."""
    from trackdlo_amd import binding as B, synth
    M = 50
    X, Y0, _ = synth.scene(N, M, config=2)
    vis = np.array([m for m in range(M) if not 20 <= m < 25], dtype=np.int32)
    P = synth.LAUNCH_PARAMS
    for route, ctx in ctxs.items():
        assert ctx.set_sort_reuse(True) is True                 # (the default, left as it was)
        ctx.set_cloud(0, X)
        with _Routes(ctx, route, M) as r:
            for i, it in enumerate(SEQUENCE):
                expect_reuse = i > 0
                if between:
                    kw = FS.base_kw(max_iter=4 + i % 3)
                    if i % 2 == 0:
                        other = ctx.cpd_lle_resident(0, Y0, 0.0, B.make_params(kw["beta"], kw["lambda_"], kw["lle_weight"], kw["mu"], kw["max_iter"], 0.0, False, 0.0, 0.0,
                                                                                 kw["visibility_threshold"], B.PREC_F64))
                        expect_reuse = False
                    else:
                        other = ctx.cpd_lle_resident(0, Y0, 0.0, _params(dict(kw, k_vis=P["k_vis"])), visible_nodes=vis)
                        expect_reuse = True
                    assert other["rc"] == 0 and other["iters"] == kw["max_iter"]
                g = ctx.cpd_lle_resident(0, Y0, 0.0, _params(FS.base_kw(max_iter=it)), check=False)
                r.expect(1, 1 if it >= 2 else 0)
                assert g["sort_reused"] == (1 if expect_reuse else 0), (route, i, it, g["sort_reused"])
                assert g["rc"] == 0 and g["iters"] == it, (route, i, it, g["rc"], g["iters"])
                _same(g, _fresh_seq(route, N, X, Y0, it), (route, N, "call", i, "max_iter", it))
    for it in sorted(set(SEQUENCE)):
        for route in ("w0", "fused"):
            _same(_fresh_seq(route, N, X, Y0, it), _fresh_seq("two-launch", N, X, Y0, it), ("fresh", route, N, it))


# ---- small clouds, every chain length -----------------------------------------------------------------------------------------------------------------------------
def _three_routes(ctxs, sc, with_priors, max_iter=6):
    from trackdlo_amd import synth
    M, P = len(sc["Y0"]), synth.LAUNCH_PARAMS
    kw = dict(sc["kw"], max_iter=max_iter, tol=0.0, alpha=P["alpha"] if with_priors else 0.0)
    pri = FS.w0_priors(sc["Y0"]) if with_priors else None
    outs = {}
    for route, ctx in ctxs.items():
        with _Routes(ctx, route, M) as r:
            outs[route] = ctx.cpd_lle(sc["X"], sc["Y0"], sc["sigma2_in"], _params(kw), priors=pri, check=False)
            r.expect(1, 1)
    for route in ("w0", "fused"):
        _same(outs[route], outs["two-launch"], (sc["claim"], route, "priors" if with_priors else "plain"))
    return outs["two-launch"]


@pytest.mark.parametrize("with_priors", [False, True], ids=["plain", "priors"])
@pytest.mark.parametrize("M", FS.SMALL_M)
def test_small_clouds(ctxs, M, with_priors):
    """1 .. 257 points: fewer points than nodes, less than one wave, one workgroup exactly, one point into the second workgroup.  Six iterations, with and
    without the three priors of test_fused_w0_gpu.py.  A cloud the library refuses ends with the same return code on the three routes."""
    for N in FS.SMALL_N:
        a = _three_routes(ctxs, FS.small(M, N), with_priors)
        print(f"M={M} N={N}: rc {a['rc']} status {a['status']} iterations {a['iters']} kept {a['n_kept']}")
        if a["rc"] == 0:
            assert a["iters"] == 6 and a["n_kept"] == N and np.isfinite(a["Y"]).all()


_GROUPS = [FS.LENGTHS[i:i + 10] for i in range(0, len(FS.LENGTHS), 10)]


@pytest.mark.parametrize("with_priors", [False, True], ids=["plain", "priors"])
@pytest.mark.parametrize("Ms", _GROUPS, ids=[f"{g[0]}-{g[-1]}" for g in _GROUPS])
def test_every_chain_length(ctxs, Ms, with_priors):
    """8 .. 64 nodes on 700 points, six iterations: k_iter_fused_w0 up to 61 nodes, k_iter_fused for 62 .. 64 (asserted by the route counters)."""
    for M in Ms:
        a = _three_routes(ctxs, FS.length(M), with_priors)
        assert a["rc"] == 0 and a["iters"] == 6 and a["n_kept"] == 700, (M, a["rc"], a["iters"], a["n_kept"])


@pytest.mark.parametrize("with_priors", [False, True], ids=["plain", "priors"])
def test_seven_nodes_stay_off_the_one_launch_loop(ctxs, with_priors):
    """(_Routes expects no increment of either counter for a chain outside 8 .. 64 nodes, on any route.)"""
    a = _three_routes(ctxs, FS.length(FS.REFUSED_M), with_priors)
    assert a["rc"] == 0 and a["iters"] == 6


# ---- the eligibility edge -------------------------------------------------------------------------------------------------------------------------------------------
def test_the_eligibility_edge_at_65536_points(ctxs):
    """Default switches: 65 536 points take the one-launch loop, 65 537 do not; both equal the two-launch loop's bits."""
    from trackdlo_amd import synth
    M = 50
    kw = FS.base_kw(max_iter=4)
    ctx = _ctx(None, None, max_points=NMAX, max_nodes=64)
    try:
        for N, takes in ((65536, 1), (65537, 0)):
            X, Y0, _ = synth.scene(N, M, config=2)
            before = _counts(ctx)
            g = ctx.cpd_lle(X, Y0, 0.0, _params(kw), check=False)
            took = tuple(a - b for a, b in zip(_counts(ctx), before))
            assert took == (takes, takes), (N, took)
            with _Routes(ctxs["two-launch"], "two-launch", M):
                a = ctxs["two-launch"].cpd_lle(X, Y0, 0.0, _params(kw), check=False)
            assert a["rc"] == 0 and a["iters"] == 4 and a["n_kept"] == N
            _same(g, a, ("default switches", N))
    finally:
        ctx.close()


# ---- an error in a chosen launch ------------------------------------------------------------------------------------------------------------------------------------
def test_an_error_in_a_chosen_launch(ctxs):
    """The "nodes free to fly" and "mu = 0 beside the cloud" inputs of test_fused_iter_gpu.py with max_iter = 2 .. 7: wherever the two-launch loop ends in
    TDLO_E_NUMERIC the other two routes end with the same code after the same iteration, and a benign registration on the same context and slot then equals
    a fresh context's.  At least two different error iterations, one odd and one even, must occur on the two-launch route (both error words, both state
    copies), or this test checks nothing.
    Measured on an MI355X: within seven iterations the first input does not end in an error at all, and the second one ends in the first E-step (k_estep,
    iteration 0) whatever max_iter is -- between them no one-launch iteration ever meets an error.  So four inputs of the same kind are run beside them, on
    the same cloud: a prior on node 5 far outside the extent the fixed-point sums were scaled for, which the two-launch loop refuses in iteration 1, 2, 3
    and 4 (1e5 m with alpha 3 at the launch file's lambda; 3e6 m with alpha 1e12 at the launch file's lambda and at lambda 1; 1e5 m with alpha 3 at lambda
    1).  The condition is asked of the iterations from 1 on: the ones an E-step half of a one-launch iteration reports and the next launch, or the closing
    k_mstep_chain, reads."""
    from trackdlo_amd import binding as B, synth
    M, N = 30, 4000
    X, Y, _ = synth.scene(N, M, config=810)
    Yoff = np.asfortranarray(Y + np.array([0.0, 0.09, 0.0]))
    far = lambda d: np.array([[5, Y[5, 0] + d, Y[5, 1], Y[5, 2]]])
    cases = [("nodes free to fly", Yoff, 0.0, dict(lambda_=1.0, beta=0.1), None), ("mu = 0 beside the cloud", Yoff, 1e-6, dict(mu=0.0), None),
             ("prior 1e5 m away, alpha 3", Y, 0.0, dict(alpha=3.0), far(1e5)), ("prior 3e6 m away, alpha 1e12", Y, 0.0, dict(alpha=1e12), far(3e6)),
             ("prior 3e6 m away, alpha 1e12, lambda 1", Y, 0.0, dict(alpha=1e12, lambda_=1.0), far(3e6)),
             ("prior 1e5 m away, alpha 3, lambda 1", Y, 0.0, dict(alpha=3.0, lambda_=1.0), far(1e5))]
    benign = FS.base_kw(max_iter=5)
    fresh = {route: _fresh(route, X, Y, 0.0, benign) for route in ctxs}
    assert fresh["two-launch"]["rc"] == 0 and fresh["two-launch"]["iters"] == 5
    outs = {}
    for route, ctx in ctxs.items():
        ctx.set_cloud(0, X)
        res = []
        with _Routes(ctx, route, M) as r:
            for cname, Yc, s2, over, pri in cases:
                for it in range(2, 8):
                    g = ctx.cpd_lle_resident(0, Yc, s2, _params(FS.base_kw(max_iter=it, **over)), priors=pri, check=False)
                    ok = ctx.cpd_lle_resident(0, Y, 0.0, _params(benign), check=False)
                    r.expect(2, 2)
                    _same(ok, fresh[route], ("benign after", cname, it, route))
                    res.append((cname, it, g))
        outs[route] = res
    error_its = set()
    for i, (cname, it, a) in enumerate(outs["two-launch"]):
        print(f"{cname}, max_iter {it}: rc {a['rc']} status {a['status']} after {a['iters']} iterations")
        for route in ("w0", "fused"):
            _same(outs[route][i][2], a, (cname, it, route))
        if a["rc"] == B.TDLO_E_NUMERIC:
            error_its.add(a["iters"])
        else:
            assert a["rc"] == 0 and a["iters"] == it, (cname, it, a["rc"], a["iters"])
    print("error iterations on the two-launch route:", sorted(error_its))
    in_loop = {e for e in error_its if e >= 1}
    assert len(in_loop) >= 2 and {e % 2 for e in in_loop} == {0, 1}, sorted(error_its)
