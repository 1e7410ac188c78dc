#!/usr/bin/env python3
"""Surface registration on the device: the 36-pair VGA ring (10k, 10k + 3 degrees, D = 128, ground-truth poses) fused into
[-0.13, 0.13]^3 at 128^3 and 256^3 grid points, cleaned and simplified (2 voxels); the simplified vertices, read in place on the
device, are registered to synth.shell_mesh(5) (20 480 faces) with d_max = 8 mm.  Prints one JSON line and writes it to
profiles/register_bench_line.json.

  eval_query_ms      HIP events around the sdist query of one evaluation at the identity (sfmx_register_last_query_us) ...
  eval_own_ms        ... and around k_rg_apply plus k_rg_system and the tree levels (sfmx_register_last_us); mean over `calls`
                     after one warm-up call
  n, n_used          source points and the samples that evaluation used
  run_*              one full run from a start 1 degree, 1 % and 2 mm off: evaluations, status, the device time of its
                     queries and of its own launches (mean over `calls`), how far the result is from the identity
  cond7, cond6       condition of A (with and without the scale row) at the identity.  The shell is one bumpy sphere: the
                     rotation block of A rests on its relief of about a seventh of the radius alone
  --check            at 128^3: the evaluation and the run compared bit for bit with tests/register_ref.py
Run on the GPU box."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "structure-from-motion-3d-reconstruction_amd"
D_MAX = 0.008


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    import register_ref as RG
    import sdist_ref as SR
    capi = importlib.import_module(PKG + ".capi")
    pipeline = importlib.import_module(PKG + ".pipeline")
    synth = importlib.import_module(PKG + ".synth")
    angles = [x for k in range(36) for x in (10.0 * k, 10.0 * k + 3.0)]
    seq = synth.make_sequence(len(angles), 640, 480, angles=angles)
    poses = [(seq["R"][i].T, -seq["R"][i].T @ seq["t"][i]) for i in range(len(angles))]
    ctx = capi.Context(0)
    st = ctx.stereo(640, 480)
    views = []
    for k in range(36):
        i, j = 2 * k, 2 * k + 1
        r = pipeline.stereo_rectify(seq["K"], poses[i], poses[j], 640, 480)
        il, ir = (seq["images"][j], seq["images"][i]) if r["swapped"] else (seq["images"][i], seq["images"][j])
        views.append((r, st.disparity(il, ir, r["H_l"], r["H_r"])))
    st.close()
    G = synth.shell_mesh(5)
    out = {"calls": a.calls, "pairs": 36, "target_faces": int(len(G[1])), "d_max": D_MAX}
    ok = True
    rg, cl, sp = ctx.register(), ctx.clean(), ctx.simplify()
    ctx.set_timing(True)
    rg.set_target(*G, D_MAX)
    out["set_target_ms"] = round((rg.last_us() + rg.last_query_us()) / 1e3, 4)
    start = RG.disturb(rg.pivot(), 1.0, 1.01, 0.002, np.random.default_rng(3))
    for n in (128, 256):
        vol = dict(origin=(-0.13, -0.13, -0.13), voxel=0.26 / (n - 1), dims=(n, n, n))
        fu = ctx.fusion(**vol)
        for r, d in views:
            fu.add_view(r, d)
        fu.extract()
        cl.fusion(fu)
        sp.clean(cl, cell=2.0 * vol["voxel"], origin=vol["origin"])
        nv, pv, _, _ = sp.device_mesh()
        rg.system(pv, n=nv)  # warm-up
        q, own = [], []
        for _ in range(a.calls):
            sums, used = rg.system(pv, n=nv)
            q.append(rg.last_query_us())
            own.append(rg.last_us())
        A = np.zeros((7, 7))
        for t, (i, j) in enumerate(RG.PAIRS):
            A[i, j] = A[j, i] = sums[t]
        rq, ro = [], []
        for _ in range(a.calls):
            res = rg.run(pv, init=start, n=nv)
            rq.append(rg.last_query_us())
            ro.append(rg.last_us())
        err = RG.transform_error(res["T"], RG.identity(), rg.pivot())
        r = dict(n=nv, n_used=used, eval_query_ms=round(float(np.mean(q)) / 1e3, 4), eval_own_ms=round(float(np.mean(own)) / 1e3, 4),
                 rms_plane=round(float(np.sqrt(sums[35] / used)), 6) if used else None,
                 cond7=float(f"{np.linalg.cond(A):.3g}") if used else None, cond6=float(f"{np.linalg.cond(A[:6, :6]):.3g}") if used else None,
                 run_evaluations=res["iterations"], run_status=capi.REGISTER_STATUS[res["status"]],
                 run_query_ms=round(float(np.mean(rq)) / 1e3, 4), run_own_ms=round(float(np.mean(ro)) / 1e3, 4),
                 start_error=[float(f"{v:.3g}") for v in RG.transform_error(start, RG.identity(), rg.pivot())],
                 final_error=[float(f"{v:.3g}") for v in err])
        if a.check and n == 128:
            X = sp.read()["verts"]
            rs, rn = RG.system(RG.identity(), X, *G, D_MAX, dist=SR.pruned)
            r["bit_equal"] = bool(rn == used and rs.tobytes() == sums.tobytes()
                                  and RG.same_result(res, RG.register(X, *G, D_MAX, init=start, dist=SR.pruned)))
            ok = ok and r["bit_equal"]
        out[f"n{n}"] = r
        fu.close()
    ctx.set_timing(False)
    for o in (rg, cl, sp):
        o.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "register_bench_line.json"), "w") as f:
        f.write(line + "\n")
    if a.check and not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
