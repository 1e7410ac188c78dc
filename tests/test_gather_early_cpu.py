"""CPU suite: a keyframe block builds its map entries and the next BA window while the previous BA is still on lane B (the
default), or after the join (SFMX_GATHER_LATE=1, and every block with an accepted loop closure).  Both orders, and the fully
serial schedule, must write the same bytes.

Runs the stand-alone CLI of tests/fake_sfmx built with ThreadSanitizer (a program of its own, run directly): the host runtime is
the product's, the kernels are the oracle's.  Inputs:
 * e2e_small and e2e_loop (accepted loop closures: both orders of a block and the transitions between them), also checked
   against the reference CLI's golden output;
 * 6-frame 320x240 synthetic sequences with configs that put the gather's edge cases on the path:
   - ba.max_points = 8: the cut-off falls among the points a block has just inserted (their positions are still awaited),
   - ba.max_points = 1,
   - ba.window = 2,
   - keyframe.min_gap = 2: frames without a keyframe lie between a BA submit and its join,
   - frames = 2: one BA is still in flight when the frame loop ends.
Each case is asserted from the run's own stdout (keyframe and map point counts per frame)."""
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
from test_oracle_golden import check_e2e_against_reference

FAKE = os.path.join(H.ROOT, "tests", "fake_sfmx")
synth = importlib.import_module(H.PKG_NAME + ".synth")
FILES = ("keyframes_camera_centers.csv", "posegraph_edges.csv", "templeRing_sparse_points.ply")
VARIANTS = ({}, {"SFMX_GATHER_LATE": "1"}, {"SFMX_NO_ASYNC": "1", "SFMX_NO_PREFETCH": "1", "SFMX_GATHER_LATE": "1"})
SWITCHES = ("SFMX_GATHER_LATE", "SFMX_NO_ASYNC", "SFMX_NO_PREFETCH", "SFMX_EDGE_LANES", "SFMX_JOIN_C_EARLY", "SFMX_VERIFY_LATE")


@pytest.fixture(scope="module")
def exe():
    p = subprocess.run(["make", "-C", FAKE, "SAN=thread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    return os.path.join(FAKE, "_build", "thread", "templering_sfm")


def _cfg(frames, klt=None, keyframe=None, ba=None):
    return {"common": {"system": {"frames": frames}, "klt": klt or {}, "keyframe": keyframe or {}}, "cpp": {"ba": ba or {}}}


def _run_all(exe, root):
    """The three schedules on one dataset: identical stdout and files, no sanitizer report.  Returns (stdout, out dir) of the default."""
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    runs = []
    for k, extra in enumerate(VARIANTS):
        out = os.path.join(root, f"out{k}")
        env = {**base, "TSAN_OPTIONS": "halt_on_error=0 exitcode=66", "SFMX_HOST_THREADS": "4", **extra}
        p = subprocess.run([exe, root, out, "--config", os.path.join(root, "cfg.json")], capture_output=True, text=True, cwd=root, env=env,
                           timeout=600)
        assert p.returncode == 0, (extra, p.stderr[:4000])
        for needle in ("ThreadSanitizer", "AddressSanitizer", "LeakSanitizer", "runtime error"):
            assert needle not in p.stderr, (extra, p.stderr[:4000])
        runs.append((p.stdout, out))
    for stdout, out in runs[1:]:
        assert stdout.replace(out, "X") == runs[0][0].replace(runs[0][1], "X")
        for fn in FILES:
            assert open(os.path.join(out, fn)).read() == open(os.path.join(runs[0][1], fn)).read(), fn
    return runs[0]


def _counts(stdout):
    """[(keyframes, map_points)] per frame, from the CLI's progress lines."""
    rows = [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"^frame \d+/\d+ \| keyframes=(\d+) \| map_points=(\d+)$", stdout, re.M)]
    assert rows, stdout[:2000]
    return rows


def _blocks(rows):
    """Map points added by each keyframe block after the first keyframe."""
    return [b[1] - a[1] for a, b in zip(rows, rows[1:]) if b[0] == a[0] + 1]


@pytest.mark.parametrize("name", ["e2e_small", "e2e_loop"])
def test_goldens_same_bytes_either_order(exe, tmp_path, name):
    g = np.load(os.path.join(H.GOLDEN, name + ".npz"))
    root = str(tmp_path / name)
    names = [str(s) for s in g["names"]]
    synth.write_dataset(root, dict(images=g["images"], K=g["K"], R=g["R"], t=g["t"], names=names, lat=g["lat"], lon=g["lon"]))
    with open(os.path.join(root, "cfg.json"), "w") as f:
        f.write(str(g["config"]))
    stdout, out = _run_all(exe, root)
    check_e2e_against_reference(g, stdout, out)
    rows = _counts(stdout)
    assert rows[-1][0] >= 3 and rows[-1][1] > 0  # several keyframe blocks, a map
    if name == "e2e_loop":  # an accepted loop closure: a loop edge in the pose graph, so both orders of a block ran in the default
        edges = open(os.path.join(out, "posegraph_edges.csv")).read().splitlines()[1:]
        loops = [e for e in edges if e.split(",")[-1] == "1"]
        assert loops and len(loops) < rows[-1][0] - 1


@pytest.fixture(scope="module")
def sequences():
    return {seed: synth.make_sequence(6, 320, 240, 0.3, n_blobs=6000, seed=seed) for seed in (5, 11)}


# every frame that may be a keyframe is one (inliers < min_inliers, T:1700-1704)
KLT = {"max_tracks": 600, "min_tracks": 400, "min_distance": 5}
CASES = {
    "cutoff8_window2_gap2": (5, _cfg(6, KLT, {"min_inliers": 100000, "min_gap": 2}, {"max_points": 8, "window": 2, "iters": 3})),
    "one_point": (11, _cfg(6, KLT, {"min_inliers": 100000}, {"max_points": 1, "iters": 3})),
    "two_frames": (11, _cfg(2, KLT, {"min_inliers": 100000}, {"iters": 3})),
}


@pytest.mark.parametrize("case", list(CASES))
def test_synthetic_edge_cases_same_bytes_either_order(exe, sequences, tmp_path, case):
    seed, cfg = CASES[case]
    root = str(tmp_path / case)
    synth.write_dataset(root, sequences[seed])
    with open(os.path.join(root, "cfg.json"), "w") as f:
        json.dump(cfg, f)
    stdout, out = _run_all(exe, root)
    rows = _counts(stdout)
    added = _blocks(rows)
    print(case, "keyframes/map_points per frame:", rows, "points added per block:", added)
    if case == "cutoff8_window2_gap2":
        # keyframes on every second frame only: frames without a keyframe lie between a submit and its join
        assert len(rows) == 6 and [r[0] for r in rows] == [1, 1, 2, 2, 3, 3]
        # every block inserts more points than a window takes: the cut-off at 8 falls among points of the same block
        assert len(added) == 2 and min(added) > 8
    elif case == "one_point":
        assert len(rows) == 6 and rows[-1][0] == 6 and rows[-1][1] > 1 and len(added) == 5
    else:
        assert len(rows) == 2 and rows[-1][0] == 2 and rows[-1][1] > 0  # BA(1) is in flight when the loop ends
    ply = open(os.path.join(out, "templeRing_sparse_points.ply")).read().splitlines()
    assert len(ply) - (ply.index("end_header") + 1) == rows[-1][1]  # the export sees every point, with its final position
    assert not any("nan" in l or "inf" in l for l in ply)


def test_a_block_without_triangulation_jobs(exe, sequences, tmp_path):
    """No replenish between two keyframes (min_tracks = 1): the later block has no track that is new to the map, so its
    structural part inserts nothing and the window awaits no position."""
    root = str(tmp_path / "nojobs")
    synth.write_dataset(root, sequences[5])
    with open(os.path.join(root, "cfg.json"), "w") as f:
        json.dump(_cfg(6, {"max_tracks": 600, "min_tracks": 1, "min_distance": 5}, {"min_inliers": 100000}, {"iters": 3}), f)
    stdout, _ = _run_all(exe, root)
    rows = _counts(stdout)
    added = _blocks(rows)
    print("keyframes/map_points per frame:", rows, "points added per block:", added)
    assert rows[-1][0] == 6 and added[0] > 0 and 0 in added[1:]
