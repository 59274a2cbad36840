"""The loop with one launch per EM iteration (trackdlo_amd/csrc/tdlo_iter_fused.hip: k_iter_fused = M-step (k) ; E-step (k + 1), every workgroup of the E-step's
grid running the M-step itself) against the two-launch loop it replaces (k_estep, k_mstep_chain).  The sums are integers and both halves are the statements of the
two-launch kernels, so the comparison is for EQUALITY: Y, sigma2, the iteration count, the kept-point count and the status, bit for bit.  TDLO_FUSED_ITER=1 / =0
select the loop (read when the context is made); tdlo_debug_route_count(14) counts the registrations the one-launch loop ran."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_FUSED = 14


def _ctx(mode, **kw):
    from trackdlo_amd import binding as B
    old = os.environ.get("TDLO_FUSED_ITER")
    if mode is None:
        os.environ.pop("TDLO_FUSED_ITER", None)
    else:
        os.environ["TDLO_FUSED_ITER"] = mode
    try:
        return B.Context(device=0, timing=False, **kw)
    finally:
        if old is None:
            os.environ.pop("TDLO_FUSED_ITER", None)
        else:
            os.environ["TDLO_FUSED_ITER"] = old


def _fused(ctx):
    return int(ctx.lib.tdlo_debug_route_count(ctx.h, ROUTE_FUSED))


def _kw(**over):
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    kw = dict(beta=P["beta"], lambda_=P["lambda_"], lle_weight=P["lle_weight"], mu=P["mu"], max_iter=30, tol=0.0, include_lle=False, alpha=0.0, k_vis=0.0,
              visibility_threshold=P["visibility_threshold"])
    kw.update(over)
    return kw


def _params(kw, prec=0):
    from trackdlo_amd import binding as B
    return B.make_params(kw["beta"], kw["lambda_"], kw["lle_weight"], kw["mu"], kw["max_iter"], kw["tol"], kw["include_lle"],
                         kw["alpha"], kw["k_vis"], kw["visibility_threshold"], prec)


def _same(a, b, label):
    assert a["rc"] == b["rc"] and a["status"] == b["status"], (label, a["rc"], b["rc"], a["status"], b["status"])
    assert a["iters"] == b["iters"] and a["n_kept"] == b["n_kept"] and a["converged"] == b["converged"], (label, a["iters"], b["iters"], a["n_kept"], b["n_kept"])
    if a["rc"] == 0:
        assert a["sigma2"] == b["sigma2"], (label, a["sigma2"], b["sigma2"])
        assert np.array_equal(a["Y"], b["Y"]), (label, float(np.abs(a["Y"] - b["Y"]).max()))


@pytest.mark.parametrize("N", [5000, 20000, 50000])
@pytest.mark.parametrize("M", [8, 45, 50, 64])
def test_one_launch_loop_gives_the_two_launch_loops_bits(M, N):
    """Two slots called alternately five times, with and without correspondence priors, with tol = 0 (fixed count) and with the launch file's tol (early exit
    through the polling chunks: the same iteration count).  None of the point counts is a multiple of 64: the last batch is ragged."""
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    pairs = [synth.scene(N, M, config=2, frame=f)[:2] for f in range(2)]
    pri = [np.array([[1, *(Y0[1] + [0.004, -0.003, 0.002])], [M - 3, *(Y0[M - 3] + [-0.002, 0.005, 0.001])], [M // 2, *Y0[M // 2]]]) for _, Y0 in pairs]
    variants = [("fixed", _kw(), False), ("fixed+priors", _kw(alpha=P["alpha"]), True),
                ("early", _kw(max_iter=50, tol=P["tol"]), False), ("early+priors", _kw(max_iter=50, tol=P["tol"], alpha=P["alpha"]), True)]
    outs = {}
    for mode in ("0", "1"):
        ctx = _ctx(mode, max_frames=2, max_points=N, max_nodes=64)
        try:
            ctx.set_sort_reuse(False)
            for k in (0, 1):
                ctx.set_cloud(k, pairs[k][0])
            res = []
            for name, kw, wp in variants:
                before = _fused(ctx)
                res.append([ctx.cpd_lle_resident(k, pairs[k][1], 0.0, _params(kw), priors=pri[k] if wp else None) for k in (0, 1, 0, 1, 0)])
                assert _fused(ctx) - before == (5 if mode == "1" else 0), (name, mode, _fused(ctx) - before)
            outs[mode] = res
        finally:
            ctx.close()
    for (name, kw, _), ra, rb in zip(variants, outs["0"], outs["1"]):
        for i, (a, b) in enumerate(zip(ra, rb)):
            _same(a, b, (name, M, N, i))
            if kw["tol"] == 0.0:
                assert a["iters"] == kw["max_iter"]
    early = [r["iters"] for r in outs["1"][2]]
    print(f"M={M} N={N}: early-exit iteration counts {early}")


def test_a_registration_that_ends_in_a_numeric_error_ends_the_same_way():
    """Inputs far outside the extent the fixed-point sums were scaled for (a prior tens of kilometres away with a huge weight; nodes free to fly; mu = 0 beside the
    cloud): the E-step refuses a contribution, or the M-step finds a sigma2 it cannot use, in some iteration.  Same return code, same status, same iteration --
    and where the call succeeds, the same bits.  At least one of the inputs must end in TDLO_E_NUMERIC, or this test checks nothing."""
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
    for mode in ("0", "1"):
        ctx = _ctx(mode, max_points=N2, max_nodes=64)
        try:
            outs[mode] = [ctx.cpd_lle(Xc, Yc, s2, _params(kw), priors=pri, check=False) for _, Xc, Yc, s2, kw, pri in cases]
            assert _fused(ctx) == (len(cases) if mode == "1" else 0)
            ok = ctx.cpd_lle(X2, Y2, 0.0, _params(_kw(max_iter=12)))          # the context stays usable
            assert ok["rc"] == 0 and ok["iters"] == 12
        finally:
            ctx.close()
    errors = 0
    for (name, *_), a, b in zip(cases, outs["0"], outs["1"]):
        print(f"{name}: rc {a['rc']} status {a['status']} after {a['iters']} iterations")
        _same(a, b, name)
        errors += a["rc"] == B.TDLO_E_NUMERIC
    assert errors >= 1


def test_calls_the_one_launch_loop_does_not_take():
    """fp64 mode, the LLE term, the visibility term, 65 nodes and a batch run as before, TDLO_FUSED_ITER=1 or not: the route counter stays where it is."""
    from trackdlo_amd import synth
    from oracle import ref_cpu
    N, M = 6000, 45
    X, Y0, vis = synth.scene(N, M, config=3, occlude=(0.4, 0.55))
    vext = synth.extend_visible(vis, M, synth.geodesic_coord(Y0))
    P = synth.LAUNCH_PARAMS
    L = ref_cpu.calc_lle_weights(Y0, 6)
    H = (np.eye(M) - L).T @ (np.eye(M) - L)
    X65, Y65, _ = synth.scene(N, 65, config=3)
    ctx = _ctx("1", max_frames=2, max_points=N, max_nodes=80)
    try:
        took = ctx.cpd_lle(X, Y0, 0.0, _params(_kw(max_iter=6)))
        assert took["rc"] == 0 and _fused(ctx) == 1                      # (the counter does count)
        assert ctx.cpd_lle(X, Y0, 0.0, _params(_kw(max_iter=6), 1))["rc"] == 0                                                   # fp64 mode
        assert ctx.cpd_lle(X, Y0, 2e-5, _params(_kw(max_iter=6, include_lle=True, beta=P["beta_pre_proc"], lambda_=P["lambda_pre_proc"])), H=H)["rc"] == 0      # the LLE term
        assert ctx.cpd_lle(X, Y0, 0.0, _params(_kw(max_iter=6, k_vis=P["k_vis"])), visible_nodes=vext)["rc"] == 0                # the visibility term
        assert ctx.cpd_lle(X65, Y65, 0.0, _params(_kw(max_iter=6)))["rc"] == 0                                                   # 65 nodes
        ctx.set_cloud(0, X); ctx.set_cloud(1, X)
        ctx.cpd_lle_batch([Y0, Y0], [0.0, 0.0], _params(_kw(max_iter=6)))                                                        # a batch
        assert _fused(ctx) == 1
    finally:
        ctx.close()


def test_default_is_by_eligibility():
    """Unset: the one-launch loop up to 65 536 points, the two-launch loop beyond (TDLO_FUSED_ITER=1 takes those as well, with the same bits)."""
    from trackdlo_amd import synth
    M = 50
    small = synth.scene(20000, M, config=5)[:2]
    big = synth.scene(70000, M, config=5)[:2]
    res = {}
    for mode in (None, "1", "0"):
        ctx = _ctx(mode, max_points=70000, max_nodes=64)
        try:
            a = ctx.cpd_lle(small[0], small[1], 0.0, _params(_kw(max_iter=10)))
            n1 = _fused(ctx)
            b = ctx.cpd_lle(big[0], big[1], 0.0, _params(_kw(max_iter=10)))
            res[mode] = (a, b, n1, _fused(ctx) - n1)
        finally:
            ctx.close()
    assert res[None][2:] == (1, 0) and res["1"][2:] == (1, 1) and res["0"][2:] == (0, 0), [r[2:] for r in res.values()]
    for mode in (None, "1"):
        _same(res["0"][0], res[mode][0], ("small", mode)); _same(res["0"][1], res[mode][1], ("big", mode))


def test_bench_outputs_are_the_two_launch_loops(tmp_path):
    """bench.py --dump-outputs with the one-launch loop and with the two-launch loop, same arguments: the .npy files are equal."""
    dirs = {}
    for mode in ("0", "1"):
        d = tmp_path / f"out{mode}"
        env = dict(os.environ, TDLO_FUSED_ITER=mode)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        dirs[mode] = d
    names = sorted(f for f in os.listdir(dirs["0"]) if f.endswith(".npy"))
    assert names and names == sorted(f for f in os.listdir(dirs["1"]) if f.endswith(".npy")), names
    for f in names:
        a, b = np.load(dirs["0"] / f), np.load(dirs["1"] / f)
        assert a.shape == b.shape and np.array_equal(a, b), f
