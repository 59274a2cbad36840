"""tdlo_cpd_lle_batch_each -- the batch with per-frame priors, visible sets and H, in caller-chosen slots -- against tdlo_cpd_lle_resident frame by frame.

Contexts are made under TDLO_ESTEP2=0, so both sides run k_estep: the E-step's sums are integers from the grain of one wave x one batch on, and every
frame of a batch must equal the same frame registered alone bit for bit -- nodes, sigma2, iterations, `converged`, `n_kept`."""
import numpy as np
import pytest

from test_prepass_gpu import make_ctx

pytestmark = pytest.mark.gpu
M, N = 30, 3000


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx({"TDLO_ESTEP2": 0}, max_frames=8, max_points=1 << 14, max_nodes=64)
    yield c
    c.close()


def params(include_lle=False, k_vis=None, max_iter=30, alpha=None):
    from trackdlo_amd import binding as B, synth
    P = synth.LAUNCH_PARAMS
    if include_lle:
        return B.make_params(P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"], P["mu"], max_iter, P["tol"], True, 0.0, 0.0, 0.01)
    return B.make_params(P["beta"], P["lambda_"], P["lle_weight"], P["mu"], max_iter, P["tol"], False, P["alpha"] if alpha is None else alpha,
                         P["k_vis"] if k_vis is None else k_vis, P["visibility_threshold"])


def frames(F, config=140):
    from trackdlo_amd import synth
    out = []
    for f in range(F):
        X, Y0, _ = synth.scene(N - 41 * f, M, config=config, frame=f)
        out.append((X, Y0))
    return out


def priors_for(Y0, K, seed):
    """K correspondence priors: node index and a target 2 .. 6 mm from the node."""
    rng = np.random.default_rng(900 + seed)
    idx = np.sort(rng.choice(M, K, replace=False))
    return np.column_stack([idx.astype(np.float64), Y0[idx] + rng.uniform(0.002, 0.006, (K, 3)) * rng.choice([-1.0, 1.0], (K, 3))])


def compare(ctx, slots, fr, s2s, pr, priors, vis, H, label):
    """The batch in `slots`, then every frame alone on its slot with its own arguments: equal bits."""
    F = len(fr)
    for s, (X, _) in zip(slots, fr):
        ctx.set_cloud(s, X)
    out = ctx.cpd_lle_batch_each(slots, [y for _, y in fr], s2s, pr, priors=priors, visible_nodes=vis, H=H)
    for f in range(F):
        one = ctx.cpd_lle_resident(slots[f], fr[f][1], s2s[f], pr, priors=None if priors is None else priors[f],
                                   visible_nodes=None if vis is None else vis[f], H=None if H is None else H[f])
        st = out["stats"][f]
        np.testing.assert_array_equal(out["Y"][f], one["Y"], err_msg=f"{label}: frame {f}")
        assert out["sigma2"][f] == one["sigma2"], (label, f, out["sigma2"][f], one["sigma2"])
        assert (st["iters"], bool(st["converged"]), st["n_kept"], st["status"]) == (one["iters"], one["converged"], one["n_kept"], 0), (label, f, st, one)
        assert one["iters"] > 0 and not np.array_equal(one["Y"], fr[f][1])
    return out


def three_kinds():
    """One frame with priors and a partial visible set, one with neither, one with a visible set only."""
    from trackdlo_amd import synth
    fr = frames(3)
    coord = synth.geodesic_coord(fr[0][1])
    v0 = synth.extend_visible(np.arange(4, 22), M, coord); v2 = synth.extend_visible(np.arange(0, 17), M, coord)
    assert 0 < len(v0) < M and 0 < len(v2) < M
    return fr, [priors_for(fr[0][1], 5, 0), None, None], [v0, None, v2]


@pytest.mark.parametrize("slots", [[0, 1, 2], [2, 0, 1]], ids=["slots-0-1-2", "slots-2-0-1"])
def test_three_frames_three_kinds_of_arguments(ctx, slots):
    """k_vis != 0: the frames with a partial visible set weigh by visibility, the one without does not -- two launches' worth of E-step kernels in one call."""
    fr, pri, vis = three_kinds()
    pr = params(alpha=1.0)
    assert pr.k_vis != 0
    out = compare(ctx, slots, fr, [0.0, 1e-4, 0.0], pr, pri, vis, None, f"slots {slots}")
    # the arguments mattered: the frame with priors differs from itself without
    plain = ctx.cpd_lle_resident(slots[0], fr[0][1], 0.0, pr, visible_nodes=vis[0])
    assert not np.array_equal(plain["Y"], out["Y"][0])


def test_eight_frames_another_K_in_each(ctx):
    """F = 8 forks the stream groups; K = 0, 1, .. 7 priors per frame, no visibility weighting: one batch."""
    fr = frames(8, config=141)
    pri = [None if k == 0 else priors_for(fr[k][1], k, 10 + k) for k in range(8)]
    compare(ctx, list(range(8)), fr, [0.0] * 8, params(k_vis=0.0, alpha=1.0), pri, None, None, "F8")


def test_lle_term_with_an_H_per_frame(ctx, oracle):
    """The pre-processing registration's form: LLE term, an H_override per frame; chains with nodes 2 cm apart take the banded solve in every frame."""
    from trackdlo_amd import synth
    fr = frames(3, config=142)
    H = []
    for f, (_, Y0) in enumerate(fr):
        assert np.linalg.norm(np.diff(Y0, axis=0), axis=1).min() > 0.015
        L = oracle.calc_lle_weights(Y0 + 1e-4 * f, 6)
        H.append((np.eye(M) - L).T @ (np.eye(M) - L))
    retries = ctx.band_retries()
    compare(ctx, [0, 1, 2], fr, [2e-5, 0.0, 1e-4], params(include_lle=True), None, None, H, "LLE")
    assert ctx.band_retries() == retries and ctx.profile_iteration(1)[3] == "k_mstep_band"


def test_shared_arguments_give_the_shared_batch(ctx):
    """Every frame handed the same priors and visible set: what tdlo_cpd_lle_batch gives."""
    from trackdlo_amd import synth
    fr = frames(4, config=143)
    coord = synth.geodesic_coord(fr[0][1])
    vis = synth.extend_visible(np.arange(3, 20), M, coord)
    pri = priors_for(fr[0][1], 4, 50)
    pr = params(alpha=1.0)
    for s, (X, _) in enumerate(fr):
        ctx.set_cloud(s, X)
    Ys = [y for _, y in fr]
    a = ctx.cpd_lle_batch(Ys, [0.0] * 4, pr, priors=pri, visible_nodes=vis)
    b = ctx.cpd_lle_batch_each(None, Ys, [0.0] * 4, pr, priors=[pri] * 4, visible_nodes=[vis] * 4)
    for f in range(4):
        np.testing.assert_array_equal(a["Y"][f], b["Y"][f])
        assert a["sigma2"][f] == b["sigma2"][f] and a["stats"][f]["iters"] == b["stats"][f]["iters"] and a["stats"][f]["n_kept"] == b["stats"][f]["n_kept"]


def test_refusals(ctx):
    from trackdlo_amd import binding as B
    fr = frames(2)
    Ys = [y for _, y in fr]
    for slots in ([0, 0], [0, 8], [-1, 0]):
        with pytest.raises(B.TdloError) as e:
            ctx.cpd_lle_batch_each(slots, Ys, [0.0, 0.0], params())
        assert e.value.code == B.TDLO_E_INVALID
