"""Fresh-process runner of the RANSAC range suite (tests/test_gpu_ransac_range.py): SFMX_RANSAC_MIN_COND is read once per process,
so every value of it gets a process of its own.

    python tests/ransac_child.py run <out.npz>    the cases of CHILD_CASES, raw outputs per case; the parent checks them
    python tests/ransac_child.py table            per scene class, the measured figures of the contract on stdout (default switches)

The parent puts SFMX_RANSAC_MIN_COND into the environment of `run`."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers as H  # noqa: E402
import ransac_inputs as R  # noqa: E402

CHILD_CLASSES = ("rot4", "dup", "general")
CHILD_H = (1, 5, 9, 17, 400)
CHILD_CASES = [(name, h) for name in CHILD_CLASSES for h in CHILD_H]
KEYS = ("counts", "lo", "hi", "flags", "cond", "E")


def run(out_path):
    capi = importlib.import_module(H.PKG_NAME + ".capi")
    ctx = capi.Context(0)
    out = {}
    for i, (name, h) in enumerate(CHILD_CASES):
        s, T = R.scene(name), R.tables(name)
        res = ctx.ransac_score_ex(s.xi, s.xj, T.idx8[:h], s.thr)
        for k in KEYS:
            out[f"{i}:{k}"] = res[k]
        out[f"{i}:best"] = np.array([res["best_iter"], res["best_count"]])
    np.savez(out_path, **out)
    ctx.close()
    print(f"ransac_child SFMX_RANSAC_MIN_COND={os.environ.get('SFMX_RANSAC_MIN_COND')}: {len(CHILD_CASES)} cases")


def load(z, i):
    res = {k: z[f"{i}:{k}"] for k in KEYS}
    res["best_iter"], res["best_count"] = (int(v) for v in z[f"{i}:best"])
    return res


def table():
    capi = importlib.import_module(H.PKG_NAME + ".capi")
    ctx = capi.Context(0)
    print(f"# sfmx_ransac_score_ex on the scene classes of tests/ransac_inputs.py: n = {R.N0}, H = {R.ITERS}, thr = {R.THR} (pixel: x {R.PIXEL_SCALE:g}^2)")
    print("# worst        largest max|E - E_ref| * cond over device-scored rows (contract: <= 1e-16), and the same up to a global sign of E")
    print("# repeated     share of rows with a repeated sample index (exact host hypothesis, first round)")
    print("# second       share of rows re-derived on the host in the second round (cond < 1e-13, nearly tied pivot, NaN)")
    print("# dev<1e-8     share of rows scored with the device hypothesis at cond < 1e-8")
    print("# lo<hi        share of rows with some point inside the band around thr")
    print("# verify       iterations ransac_local re-derives exactly: lo < hi and hi >= max(lo)")
    print(f"{'class':9s} {'worst':>10s} {'up to sign':>10s} {'repeated':>9s} {'second':>8s} {'dev<1e-8':>9s} {'lo<hi':>7s} {'verify':>7s}")
    for name in R.CLASSES:
        s, T = R.scene(name), R.tables(name)
        r = R.summary_row(name, ctx.ransac_score_ex(s.xi, s.xj, T.idx8, s.thr), T.E, T.idx8)
        print(f"{name:9s} {r['worst']:10.2e} {r['worst_up_to_sign']:10.2e} {r['repeated']:9.4f} {r['second_round']:8.4f} {r['dev_low']:9.4f} "
              f"{r['band']:7.4f} {r['verify']:7d}")
    ctx.close()


if __name__ == "__main__":
    if sys.argv[1] == "table":
        table()
    else:
        run(sys.argv[2])
