"""GPU suite: the order in which the pipeline creates its helper contexts' streams (csrc/host/lane_plan.hpp) decides which lanes
share a hardware queue, never what the product writes.  The product CLI runs in fresh child processes -- placement is fixed per
process -- under the default plan, SFMX_LANE_PLAN=parent, one alternate and the default with eight hardware queues: same bytes,
and every child names the plan it was asked for.  tests/test_lane_plan_cpu.py checks the plans themselves."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from test_oracle_golden import check_e2e_against_reference

pytestmark = pytest.mark.gpu
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")
FILES = ("keyframes_camera_centers.csv", "posegraph_edges.csv", "templeRing_sparse_points.ply")
SWITCHES = ("SFMX_LANE_PLAN", "SFMX_LANE_ORDER", "SFMX_LANE_PLAN_PRINT", "SFMX_NO_ASYNC", "SFMX_NO_CTX_POOL")
PARENT_ORDER = "T- T+ B- B+ P- P+ C- C+ A- A+ E- E+"
AS8_ORDER = "T+ A+ C+ B+ P+ E2+ A2+ E+ P2+ T- C- B- P- A- A2- E- P2- E2-"
# (environment, queue count the child must report, first words of its plan line, creation order it must report).  The CLI sets
# eight queues only where the variable is unset, so the default plan is pinned to four here.
DEFAULT = ({"GPU_MAX_HW_QUEUES": "4"}, 4, "as8 (default)", AS8_ORDER)
PARENT = ({"GPU_MAX_HW_QUEUES": "4", "SFMX_LANE_PLAN": "parent"}, 4, "parent (override)", PARENT_ORDER)
B_ALONE_ORDER = "A+ A2+ T+ B+ P+ E+ T- B- P2+ E2+ C- A- C+ E- A2- E2- P- P2-"
ALTERNATE = ({"GPU_MAX_HW_QUEUES": "4", "SFMX_LANE_PLAN": "b_alone"}, 4, "b_alone (override)", B_ALONE_ORDER)
DEFAULT_AT_8 = ({"GPU_MAX_HW_QUEUES": "8"}, 8, "parent (default)", PARENT_ORDER)


def _run_all(root, variants):
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    runs = []
    for k, (extra, queues, head, order) in enumerate(variants):
        out = os.path.join(root, f"out{k}")
        p = subprocess.run([pipe.CLI_PATH, root, out, "--config", os.path.join(root, "cfg.json")], capture_output=True, text=True, cwd=root,
                           env={**base, **extra, "SFMX_LANE_PLAN_PRINT": "1"}, timeout=120)
        assert p.returncode == 0, (extra, p.stderr[:4000])
        lines = [l for l in p.stderr.splitlines() if l.startswith("sfmx lane plan: ")]
        assert len(lines) == 1, (extra, p.stderr[:4000])
        assert lines[0].startswith(f"sfmx lane plan: {head} queues={queues} order="), (extra, lines[0])
        if order:
            assert f" order={order} first_use=" in lines[0], (extra, lines[0])
        assert "rejected" not in p.stderr, (extra, p.stderr[:4000])
        runs.append((p.stdout, out))
    for (stdout, out), v in zip(runs[1:], variants[1:]):
        assert stdout.replace(out, "X") == runs[0][0].replace(runs[0][1], "X"), v[0]
        for fn in FILES:
            assert open(os.path.join(out, fn), "rb").read() == open(os.path.join(runs[0][1], fn), "rb").read(), (v[0], fn)
    return runs[0]


def test_e2e_loop_same_bytes_under_every_plan(tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_loop.npz"))
    root = str(tmp_path / "data")
    names = [str(s) for s in g["names"]]
    synth.write_dataset(root, dict(images=g["images"], K=g["K"], R=g["R"], t=g["t"], names=names, lat=g["lat"], lon=g["lon"]))
    with open(os.path.join(root, "cfg.json"), "w") as f:
        f.write(str(g["config"]))
    stdout, out = _run_all(root, (DEFAULT, PARENT, ALTERNATE, DEFAULT_AT_8))
    check_e2e_against_reference(g, stdout, out)


def test_six_frames_same_bytes_default_and_parent(tmp_path):
    """the six-frame 320x240 case of tests/test_gpu_gather_early.py: ba.max_points = 8, ba.window = 2, keyframes on every second frame"""
    seq = synth.make_sequence(6, 320, 240, 0.3, n_blobs=6000, seed=5)
    root = str(tmp_path / "data")
    synth.write_dataset(root, seq)
    cfg = {"common": {"system": {"frames": 6}, "klt": {"max_tracks": 600, "min_tracks": 400, "min_distance": 5},
                      "keyframe": {"min_inliers": 100000, "min_gap": 2}}, "cpp": {"ba": {"max_points": 8, "window": 2, "iters": 3}}}
    with open(os.path.join(root, "cfg.json"), "w") as f:
        json.dump(cfg, f)
    stdout, out = _run_all(root, (DEFAULT, PARENT))
    rows = [l for l in stdout.strip().splitlines() if l.startswith("frame 6/6")]
    assert rows and "keyframes=3" in rows[0] and int(rows[0].rsplit("map_points=", 1)[1]) > 16
