"""bench.py on the GPU: a plain run (no --full) prints the headline and, with --dump-outputs, writes what its last timed call returned --
the nodes of that call agree with the CPU oracle's registration of the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path, oracle):
    from trackdlo_amd import synth
    steps, warmup = 3, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.rstrip("\n").splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["dtype"] == "f32" and "roofline" not in line
    Y, s2, iters = (np.load(tmp_path / (n + ".npy")) for n in ("Y", "sigma2", "iters"))
    assert Y.shape == (50, 3) and Y.dtype == np.float64 and s2.shape == iters.shape == (1,) and int(iters[0]) == 50
    # C2 alternates between the (cloud, Y0) pairs of frames 0 and 1: the last timed call is call warmup + steps - 1
    X, Y0, _ = synth.scene(50000, 50, config=2, frame=(warmup + steps - 1) % 2)
    P = synth.LAUNCH_PARAMS
    o = oracle.cpd_lle(X, Y0, 0.0, beta=P["beta"], lambda_=P["lambda_"], lle_weight=P["lle_weight"], mu=P["mu"], max_iter=50, tol=0.0,
                       include_lle=False, alpha=0.0, k_vis=0.0, visibility_threshold=P["visibility_threshold"])
    assert float(np.abs(Y - o["Y"]).max()) <= 1e-5 and abs(float(s2[0]) - o["sigma2"]) / o["sigma2"] <= 1e-3
