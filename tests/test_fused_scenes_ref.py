"""The claims of tests/fused_scenes.py, proved on the CPU with numpy and the project's own oracle (oracle.ref_cpu, trace=True) alone: what
tests/test_fused_loop_edges_gpu.py runs on the one-launch loop is what its scenes say it is.  For every scene of a .. e the oracle also completes the
iteration counts the GPU suite uses, with n_kept > 0."""
import numpy as np
import pytest

import fused_scenes as FS
from chain_numpy import carve, kernel_G
from trackdlo_amd import synth


def _run(oracle, sc, **over):
    kw = dict(sc["kw"], max_iter=FS.ITERS[-1], tol=0.0)
    kw.update(over)
    return oracle.cpd_lle(sc["X"], sc["Y0"], sc["sigma2_in"], priors=sc["priors"], trace=True, **kw)


@pytest.mark.parametrize("M", FS.CHAINS)
@pytest.mark.parametrize("name", sorted(FS.HARD))
def test_every_hard_scene_is_eligible_and_the_oracle_completes_it(oracle, name, M):
    sc = FS.HARD[name](M)
    kw = sc["kw"]
    assert not kw["include_lle"] and kw["k_vis"] == 0.0 and 8 <= len(sc["Y0"]) <= 64 and 0 < len(sc["X"]) <= 65536
    assert np.array_equal(sc["X"], sc["X"].astype(np.float32).astype(np.float64))          # (what the fp32 route and the oracle see is the same cloud)
    o = _run(oracle, sc)
    assert o["iters"] == FS.ITERS[-1] and o["n_kept"] > 0 and not o["converged"]
    assert np.isfinite(o["Y"]).all() and np.isfinite(o["trace"]["sigma2"]).all() and (o["trace"]["sigma2"] > 0).all()
    for it in FS.ITERS[:-1]:            # every count the GPU suite runs is a prefix of that trajectory
        p = _run(oracle, sc, max_iter=it)
        assert p["iters"] == it and p["n_kept"] == o["n_kept"] and np.array_equal(p["Y"], o["trace"]["Y"][it - 1])


@pytest.mark.parametrize("M", FS.CHAINS)
def test_a_dark_run_lies_across_the_middle_junction(oracle, M):
    """numpy alone, at the nodes and the sigma2 handed in: three or more consecutive dark nodes, j2 among them.  And in every one of the oracle's iterations
    (its nodes, its sigma2) j2 stays dark -- with a neighbour on one side at 13 nodes, in a run of five or more on the longer chains."""
    sc = FS.dark(M)
    j2 = carve(M)[1]
    assert (M - 1) // 2 == j2
    d0 = FS.dark_nodes(sc["X"], sc["Y0"], sc["sigma2_in"])
    assert FS.longest_run_through(d0, j2) >= 3, (M, d0)
    assert j2 - 1 in d0 and j2 + 1 in d0
    assert FS.DARK_BITS < FS.WINDOW_BITS - 20
    tr = _run(oracle, sc)["trace"]
    for k in range(FS.ITERS[-1] - 1):             # iteration k + 2's E-step sees the nodes and the sigma2 iteration k + 1 left
        dk = FS.dark_nodes(sc["X"], tr["Y"][k], tr["sigma2"][k])
        assert FS.longest_run_through(dk, j2) >= (2 if M == 13 else 5), (M, k, dk)


@pytest.mark.parametrize("M", FS.CHAINS)
def test_coincident_nodes_make_an_identity_link_and_a_singular_G(M):
    sc = FS.coincident(M)
    a = M // 3
    assert np.array_equal(sc["Y0"][a], sc["Y0"][a + 1])
    coord = synth.geodesic_coord(sc["Y0"])
    assert coord[a + 1] == coord[a] and np.all(np.diff(coord)[np.arange(M - 1) != a] > 0.01)
    G = kernel_G(coord, sc["kw"]["beta"])
    assert np.array_equal(G[a], G[a + 1]) and np.linalg.matrix_rank(G) < M
    assert a not in (0, M - 1) and a + 1 not in (0, M - 1)


@pytest.mark.parametrize("M", FS.CHAINS)
def test_priors_sit_on_the_junctions_twice_on_one_node_and_on_a_dark_node(oracle, M):
    sc = FS.priors(M)
    pn = FS.prior_nodes(M)
    j1, j2, j3 = carve(M)[:3]
    nodes = sc["priors"][:, 0].astype(int)
    assert pn["junctions"] == [0, j1, j2 - 1, j2, j3, M - 1] and set(pn["junctions"]) <= set(nodes)
    assert list(nodes).count(pn["twice"]) == 2 and pn["twice"] not in pn["junctions"] and len(nodes) == len(set(nodes)) + 1
    rows = np.nonzero(nodes == pn["twice"])[0]
    assert not np.array_equal(sc["priors"][rows[0]], sc["priors"][rows[1]])
    assert pn["dark"] in FS.dark_nodes(sc["X"], sc["Y0"], sc["sigma2_in"]) and pn["dark"] not in pn["junctions"]
    assert sc["kw"]["alpha"] == synth.LAUNCH_PARAMS["alpha"] > 0
    # the last of the two wins: without the first one the oracle gives the same bits, without the last one it does not
    o = _run(oracle, sc)
    wo_first = _run(oracle, dict(sc, priors=np.delete(sc["priors"], rows[0], axis=0)))
    wo_last = _run(oracle, dict(sc, priors=np.delete(sc["priors"], rows[1], axis=0)))
    assert np.array_equal(o["Y"], wo_first["Y"]) and o["sigma2"] == wo_first["sigma2"]
    assert np.abs(o["Y"] - wo_last["Y"]).max() > 1e-4
    # and the priors matter at all
    assert np.abs(o["Y"] - _run(oracle, dict(sc, priors=None), alpha=0.0)["Y"]).max() > 1e-4


@pytest.mark.parametrize("M", FS.CHAINS)
def test_the_displaced_start_takes_large_steps_with_the_whole_chain_in_the_window(oracle, M):
    sc = FS.start(M)
    assert sc["sigma2_in"] == 0.0
    assert np.allclose(sc["Y0"] - synth.nodes(M), [0.0, FS.START_SHIFT, 0.0], atol=1e-15)
    o = _run(oracle, sc)
    crit = FS.crits(sc["Y0"], o["trace"]["Y"])
    assert crit[0] > 10 * synth.LAUNCH_PARAMS["tol"]             # large: ten times what the launch file calls converged, in the first step alone
    # the set-up's sigma2 (the mean squared distance over all pairs / 3) is what iteration 1 runs with: no node is outside the window for any point
    d2 = ((sc["X"][:, None, :] - sc["Y0"][None, :, :]) ** 2).sum(axis=2)
    s2 = d2.sum() / (3.0 * d2.size)
    bits = -(d2 - d2.min(axis=1, keepdims=True)) / (2.0 * s2 * np.log(2.0))
    assert bits.min() > FS.WINDOW_BITS
    assert len(FS.dark_nodes(sc["X"], sc["Y0"], s2)) == 0


@pytest.mark.parametrize("M", FS.CHAINS)
def test_P1_spans_many_decades_on_one_chain(oracle, M):
    sc = FS.decades(M)
    near = ((sc["X"][:, None, :] - sc["Y0"][None, :, :]) ** 2).sum(axis=2).argmin(axis=1)
    q = M // 4
    assert 1 <= np.count_nonzero(near < q) <= 8 and np.count_nonzero(near >= q) >= 1000
    P1 = _run(oracle, sc)["trace"]["P1"]
    for k in range(P1.shape[0]):
        assert P1[k].min() >= 0.0
        pos = P1[k][P1[k] > 0]
        assert np.log10(pos.max()) - np.log10(pos.min()) >= 4.0, (M, k, pos.min(), pos.max())
        assert np.median(P1[k][:q]) < 1e-1 * np.median(P1[k][q:]), (M, k, P1[k][:q])
        # ... and not only because some nodes are dark: from the second iteration on (the first one runs with the sigma2 handed in, the later ones with the
        # M-step's) the sums that lie inside the E-step's window (a point gives a node no less than 2^-36 of a membership) alone span four decades
        seen = P1[k][P1[k] > 2.0 ** FS.WINDOW_BITS]
        assert k == 0 or np.log10(seen.max()) - np.log10(seen.min()) >= 4.0, (M, k, seen.min(), seen.max())


@pytest.mark.parametrize("M", FS.SMALL_M)
def test_small_clouds_cover_the_workgroup_edges(oracle, M):
    assert min(FS.SMALL_N) == 1 and any(n < M for n in FS.SMALL_N) and {63, 64, 65, 255, 256, 257} <= set(FS.SMALL_N)
    for N in FS.SMALL_N:
        sc = FS.small(M, N)
        assert sc["X"].shape == (N, 3) and sc["Y0"].shape == (M, 3)
        # every point lies within the prune's 0.1 m of a node: the oracle keeps the whole cloud
        o = _run(oracle, sc, max_iter=6)
        assert o["n_kept"] == N and o["iters"] == 6


def test_every_chain_length_and_the_one_below():
    assert FS.LENGTHS == tuple(range(8, 65)) and len(FS.LENGTHS) == 57 and FS.REFUSED_M == 7
    for M in FS.LENGTHS + (FS.REFUSED_M,):
        sc = FS.length(M)
        assert sc["X"].shape == (700, 3) and sc["Y0"].shape == (M, 3)


@pytest.mark.parametrize("with_priors", [False, True], ids=["plain", "priors"])
def test_the_early_exit_ladder_has_six_consecutive_rungs(oracle, with_priors):
    """Scene d at 13 nodes (and once more with the priors of scene c): tolerances between the oracle's consecutive mean displacements, each
    FS.LADDER_MARGIN = 4e-5 away from both -- twice what the stated fp32 tolerance on Y (1e-5 m, test_parity_gpu.TOL) can move a mean displacement between
    two iterates -- so that a route within that tolerance of the oracle ends in the same iteration.  Six consecutive iteration counts cover every residue of
    k mod 2 (the state copies, the error words) and k mod 3 (the accumulator buffers).  The oracle, run with each tol_k, does end after k iterations."""
    sc, ladder, crit = ladder_scene(oracle, with_priors)
    print("crit", ["%.3g" % c for c in crit], "ladder", [(k, "%.4g" % t) for k, t in ladder])
    assert len(ladder) >= FS.LADDER_RUNGS
    ks = [k for k, _ in ladder]
    assert ks == list(range(ks[0], ks[0] + len(ks)))
    assert {k % 2 for k in ks} == {0, 1} and {k % 3 for k in ks} == {0, 1, 2}
    for k, tol in ladder:
        assert all(c >= tol + FS.LADDER_MARGIN for c in crit[:k - 1]) and crit[k - 1] <= tol - FS.LADDER_MARGIN
        o = oracle.cpd_lle(sc["X"], sc["Y0"], sc["sigma2_in"], priors=sc["priors"], **dict(sc["kw"], max_iter=30, tol=tol))
        assert o["iters"] == k and o["converged"] and o["n_kept"] > 0


def ladder_scene(oracle, with_priors):
    """(scene, [(k, tol_k)], crit) of the early-exit ladder; shared with the GPU suite."""
    sc = FS.start(FS.LADDER_M)
    if with_priors:
        pc = FS.priors(FS.LADDER_M)
        sc = dict(sc, priors=pc["priors"], kw=dict(sc["kw"], alpha=pc["kw"]["alpha"]))
    o = oracle.cpd_lle(sc["X"], sc["Y0"], sc["sigma2_in"], priors=sc["priors"], trace=True, **dict(sc["kw"], max_iter=12, tol=0.0))
    crit = FS.crits(sc["Y0"], o["trace"]["Y"])
    return sc, FS.exit_ladder(crit), crit
