"""GPU suite: the product CLI writes the same bytes whether a keyframe block prepares its map entries and the next BA window
before the join with lane B (default) or after it (SFMX_GATHER_LATE=1), on the serial schedule, and with the keyframe->keyframe
edges on one lane or alternating over two (SFMX_EDGE_LANES).  tests/test_gather_early_cpu.py runs the same host code under
ThreadSanitizer on more inputs."""
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
VARIANTS = ({}, {"SFMX_GATHER_LATE": "1"}, {"SFMX_NO_ASYNC": "1", "SFMX_NO_PREFETCH": "1", "SFMX_GATHER_LATE": "1"},
            {"SFMX_EDGE_LANES": "1"}, {"SFMX_EDGE_LANES": "2"}, {"SFMX_EDGE_LANES": "2", "SFMX_GATHER_LATE": "1"})
SWITCHES = ("SFMX_GATHER_LATE", "SFMX_NO_ASYNC", "SFMX_NO_PREFETCH", "SFMX_EDGE_LANES", "SFMX_JOIN_C_EARLY", "SFMX_VERIFY_LATE")


def _run_all(root):
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    runs = []
    for k, extra in enumerate(VARIANTS):
        out = os.path.join(root, f"out{k}")
        p = subprocess.run([pipe.CLI_PATH, root, out, "--config", os.path.join(root, "cfg.json")], capture_output=True, text=True, cwd=root,
                           env={**base, **extra}, timeout=120)
        assert p.returncode == 0, (extra, p.stderr[:4000])
        runs.append((p.stdout, out))
    for (stdout, out), extra in zip(runs[1:], VARIANTS[1:]):
        assert stdout.replace(out, "X") == runs[0][0].replace(runs[0][1], "X"), extra
        for fn in FILES:
            assert open(os.path.join(out, fn)).read() == open(os.path.join(runs[0][1], fn)).read(), (extra, fn)
    return runs[0]


def test_e2e_loop_same_bytes_either_order_and_edge_lanes(tmp_path):
    g = np.load(os.path.join(H.GOLDEN, "e2e_loop.npz"))
    root = str(tmp_path / "data")
    names = [str(s) for s in g["names"]]
    synth.write_dataset(root, dict(images=g["images"], K=g["K"], R=g["R"], t=g["t"], names=names, lat=g["lat"], lon=g["lon"]))
    with open(os.path.join(root, "cfg.json"), "w") as f:
        f.write(str(g["config"]))
    stdout, out = _run_all(root)
    check_e2e_against_reference(g, stdout, out)


def test_six_frames_cutoff_among_new_points_same_bytes(tmp_path):
    """ba.max_points = 8 with hundreds of points per block: the window's cut-off falls among points whose positions the
    structural half still awaits; ba.window = 2; keyframes on every second frame."""
    seq = synth.make_sequence(6, 320, 240, 0.3, n_blobs=6000, seed=5)
    root = str(tmp_path / "data")
    synth.write_dataset(root, seq)
    cfg = {"common": {"system": {"frames": 6}, "klt": {"max_tracks": 600, "min_tracks": 400, "min_distance": 5},
                      "keyframe": {"min_inliers": 100000, "min_gap": 2}}, "cpp": {"ba": {"max_points": 8, "window": 2, "iters": 3}}}
    with open(os.path.join(root, "cfg.json"), "w") as f:
        json.dump(cfg, f)
    stdout, out = _run_all(root)
    last = stdout.strip().splitlines()
    rows = [l for l in last if l.startswith("frame 6/6")]
    assert rows and "keyframes=3" in rows[0] and int(rows[0].rsplit("map_points=", 1)[1]) > 16
