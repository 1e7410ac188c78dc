#!/usr/bin/env python3
"""The photometric registration on the device: the 36-pair VGA ring (10k, 10k + 3 degrees, D = 128, ground-truth poses) fused into
[-0.13, 0.13]^3 at 128^3 and 256^3 grid points, the surface cleaned (default thresholds) and simplified at 2 voxels, textured from
the 36 left rectified cameras and images at 640 x 480 (depth_tol = 2 voxels, patch 8); view 0, one of the texture's own, is then
registered to the textured surface from its own pose (stride 2, margin 8, the defaults otherwise).
Prints one JSON line, writes it to profiles/palign_bench_line.json and prints the table row of DESIGN.md 29 per volume.

  eval_ms            HIP events around one evaluation (sfmx_palign_last_us of sfmx_palign_system), mean over `calls` after one
                     warm-up call; zbuffer_ms, mask_ms (the mask and its erosion: the rest) and system_ms (k_pa_system and the
                     tree's levels) split it
  loop               what sfmx_palign_view does from the view's own pose: status, evaluations, n, rms, how far the view moved
  --check            the 128^3 evaluation and loop compared bit for bit with tests/palign_ref.py (NumPy)
Run on the GPU box.  There is no time target: there is no earlier code to compare with."""
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
PATCH = 8
PARAMS = dict(stride=2, margin=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "palign_bench_line.json"))
    a = ap.parse_args()
    capi = importlib.import_module(PKG + ".capi")
    pipeline = importlib.import_module(PKG + ".pipeline")
    synth = importlib.import_module(PKG + ".synth")
    angles = [x for k in range(36) for x in (10.0 * k, 10.0 * k + 3.0)]
    seq = synth.make_sequence(len(angles), 640, 480, angles=angles)
    poses = [(seq["R"][i].T, -seq["R"][i].T @ seq["t"][i]) for i in range(len(angles))]
    ctx = capi.Context(0)
    st = ctx.stereo(640, 480)
    views, rects = [], []
    for k in range(36):
        i, j = 2 * k, 2 * k + 1
        r = pipeline.stereo_rectify(seq["K"], poses[i], poses[j], 640, 480)
        il, ir = (seq["images"][j], seq["images"][i]) if r["swapped"] else (seq["images"][i], seq["images"][j])
        d = st.disparity(il, ir, r["H_l"], r["H_r"], want_rect=True)
        views.append((r, d["disp16"]))
        rects.append(d["rect"][0].copy())
    st.close()
    cams = [dict(R_rw=r["R_rw"], c_left=r["c_left"], f=r["f"], cx=r["cx"], cy=r["cy"], B=r["B"], w=640, h=480) for r, _ in views]
    z_min = max(float(np.linalg.norm(poses[0][1])) - 0.23, 0.01)
    out = {"calls": a.calls, "pairs": 36, "views": 36, "patch": PATCH, "params": PARAMS, "view": 0}
    cl, sp, tx, pa = ctx.clean(), ctx.simplify(), ctx.texture(), ctx.palign()
    for cam, img in zip(cams, rects):
        tx.add_view(cam, img)
    pa.set_image(rects[0])
    ok, rows = True, []
    for n in (128, 256):
        vol = dict(origin=(-0.13, -0.13, -0.13), voxel=0.26 / (n - 1), dims=(n, n, n))
        fu = ctx.fusion(**vol)
        for r, d in views:
            fu.add_view(r, d)
        fu.extract()
        cl.fusion(fu)
        sp.clean(cl, cell=2.0 * vol["voxel"], origin=vol["origin"])
        mesh = sp.read()
        v, f, tol = mesh["verts"], mesh["faces"], 2.0 * vol["voxel"]
        cnt = tx.run(v, f, z_min, tol, read=False, patch=PATCH)
        used = v[np.unique(f.ravel())]
        lo, hi = used.min(0), used.max(0)
        pivot = [float(lo[k]) + 0.5 * (float(hi[k]) - float(lo[k])) for k in range(3)]
        eps_trans = 1e-5 * float(np.sqrt(sum((float(hi[k]) - float(lo[k])) ** 2 for k in range(3))))
        pa.set_model(tx, v, f)
        ctx.set_timing(True)
        pa.system(cams[0], z_min, pivot, **PARAMS)  # warm-up
        us, zus, sus = [], [], []
        for _ in range(a.calls):
            sums, nn = pa.system(cams[0], z_min, pivot, **PARAMS)
            us.append(pa.last_us())
            zus.append(pa.last_zbuffer_us())
            sus.append(pa.last_system_us())
        loop = pa.view(cams[0], z_min, pivot, eps_trans=eps_trans, **PARAMS)
        loop_us = pa.last_us()
        ctx.set_timing(False)
        t, tz, ts = float(np.mean(us)), float(np.mean(zus)), float(np.mean(sus))
        dR = np.asarray(loop["view"]["R_rw"]) @ np.asarray(cams[0]["R_rw"], np.float64).reshape(3, 3).T
        moved_deg = float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))))
        moved_m = float(np.linalg.norm(np.asarray(loop["view"]["c_left"]) - np.asarray(cams[0]["c_left"], np.float64)))
        n_last, e_last = loop["trace"][-1][0], loop["trace"][-1][1]
        row = dict(eval_ms=round(t / 1e3, 4), zbuffer_ms=round(tz / 1e3, 4), mask_ms=round((t - tz - ts) / 1e3, 4), system_ms=round(ts / 1e3, 4),
                   verts=len(v), faces=len(f), faces_textured=cnt["faces_textured"], n=nn, rms_start=float(np.sqrt(sums[27] / nn)) if nn else None,
                   loop=dict(status=capi.PALIGN_STATUS[loop["status"]], evaluations=loop["iterations"], n=n_last,
                             rms=float(np.sqrt(e_last / n_last)) if n_last else None, moved_deg=moved_deg, moved_m=moved_m,
                             ms=round(loop_us / 1e3, 4)))
        if a.check and n == 128:
            import palign_ref as PA
            import texture_ref as TR
            tex = TR.run(v, f, cams, rects, z_min, tol, patch=PATCH)
            M = PA.model(v, f, tex)
            ws, wn = PA.system(M, cams[0], rects[0], z_min, pivot, **PARAMS)
            want = PA.align(M, cams[0], rects[0], z_min, pivot, eps_trans=eps_trans, **PARAMS)
            row["bit_equal"] = bool(wn == nn and ws.tobytes() == sums.tobytes() and PA.same_result(loop, want))
            ok = ok and row["bit_equal"]
        out[f"n{n}_simplified"] = row
        rows.append("| %d³ | %s (%s) | %d | %.3f ms | %.3f ms | %.3f ms | %.3f ms | %s after %d, %.4f° / %.2e m |" % (
            n, f"{len(f):,}".replace(",", " "), f"{cnt['faces_textured']:,}".replace(",", " "), nn, t / 1e3, tz / 1e3, (t - tz - ts) / 1e3,
            ts / 1e3, row["loop"]["status"], loop["iterations"], moved_deg, moved_m))
        fu.close()
    for o in (cl, sp, tx, pa):
        o.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    print("| volume | faces (textured) | n | evaluation | z-buffer | mask + erosion | `k_pa_system` + tree | loop from the view's own pose |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(r)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
