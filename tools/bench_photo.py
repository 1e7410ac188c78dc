#!/usr/bin/env python3
"""The photometric re-rendering on the device: the 36-pair VGA ring (10k, 10k + 3 degrees, D = 128, ground-truth poses) fused into
[-0.13, 0.13]^3 at 128^3 and 256^3 grid points, the surface cleaned (default thresholds) and simplified at 2 voxels, textured from
the 36 left rectified cameras and images at 640 x 480 (depth_tol = 2 voxels, patch 8) and rendered back into those 36 views.
Prints one JSON line, writes it to profiles/photo_bench_line.json and prints the table row of DESIGN.md 27 per volume.

  photo_ms           HIP events from the first to the last launch of one sfmx_photo_run (sfmx_photo_last_us), mean over `calls`
                     after one warm-up call
  resolve_ms         the same for the k_ph_resolve launches alone (sfmx_photo_last_resolve_us)
  visib_ms           tools/bench_visib.py's run (sfmx_visib_run, the same cameras without images) on the same mesh in this process:
                     it builds the same z-buffers
  pixels_per_s, resolve_bytes, resolve_share_of_6300GBps
                     sum w h / resolve time, and the resolve's algorithmic bytes -- per pixel the key (8), the three stores (6) and
                     the image byte, per textured pixel four atlas bytes, per (view, visible face) 88 bytes of indices, projected
                     vertices, view and corners -- as a share of 6.3 TB/s
  own, cross         capi.photo_summary's pooled figures
  --check            the 128^3 run compared byte for byte with tests/photo_ref.py (NumPy)
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
PATCH = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_bench_line.json"))
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
    out = {"calls": a.calls, "pairs": 36, "views": 36, "patch": PATCH}
    cl, sp, vb, tx, ph = ctx.clean(), ctx.simplify(), ctx.visib(), ctx.texture(), ctx.photo()
    for cam, img in zip(cams, rects):
        vb.add_view(cam)
        tx.add_view(cam, img)
    ph.add_texture_views(tx)
    ok = True
    rows = []
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
        ctx.set_timing(True)
        ph.run(tx, v, f, z_min, read=False)  # warm-up
        us, res = [], []
        for _ in range(a.calls):
            ph.run(tx, v, f, z_min, read=False)
            us.append(ph.last_us())
            res.append(ph.last_resolve_us())
        vb.run(v, f, z_min, tol, read=False)  # warm-up
        vus = []
        for _ in range(a.calls):
            vb.run(v, f, z_min, tol, read=False)
            vus.append(vb.last_us())
        ctx.set_timing(False)
        got = ph.read()
        t, b, tv = float(np.mean(us)), float(np.mean(res)), float(np.mean(vus))
        px = int(got["offsets"][-1])
        faces_seen = sum(len(np.unique(ph.view_image(got, q, "face"))) - 1 for q in range(36))
        nbytes = 15 * px + 4 * int(got["classes"][:, 3:].sum()) + 88 * faces_seen
        s = capi.photo_summary(got["stats"], got["hist"])
        row = dict(photo_ms=round(t / 1e3, 4), resolve_ms=round(b / 1e3, 4), visib_ms=round(tv / 1e3, 4), photo_over_visib=round(t / tv, 3),
                   resolve_share_of_run=round(b / t, 3), batch=ph.last_batch(), verts=len(v), faces=len(f),
                   faces_textured=cnt["faces_textured"], atlas=[cnt["W"], cnt["H"]], pixels=px,
                   classes=[int(x) for x in got["classes"].sum(0)], pixels_per_s=round(px / (b * 1e-6), 0), resolve_bytes=nbytes,
                   resolve_share_of_6300GBps=round(nbytes / (b * 1e-6) / 6.3e12, 5),
                   own={k: s["own"][k] for k in ("count", "mae", "rmse", "psnr", "p90")},
                   cross={k: s["cross"][k] for k in ("count", "mae", "rmse", "psnr", "p90")})
        if a.check and n == 128:
            import photo_ref as PR
            import texture_ref as TR
            try:
                tex = TR.run(v, f, cams, rects, z_min, tol, patch=PATCH)
                PR.same(got, PR.run(v, f, cams, rects, list(range(36)), tex, z_min, patch=PATCH), "128^3")
                row["bit_equal"] = True
            except AssertionError as e:
                row["bit_equal"] = False
                row["difference"] = str(e)[:200]
                ok = False
        out[f"n{n}_simplified"] = row
        rows.append("| %d³ | %s (%s) | %.3f ms | %.3f ms | %.3f ms | %.2f | %.2e | %.1f %% | %.2f / %.2f |" % (
            n, f"{len(f):,}".replace(",", " "), f"{cnt['faces_textured']:,}".replace(",", " "), t / 1e3, b / 1e3, tv / 1e3, t / tv,
            px / (b * 1e-6), 100.0 * nbytes / (b * 1e-6) / 6.3e12, s["own"]["mae"] or 0.0, s["cross"]["mae"] or 0.0))
        fu.close()
    for o in (cl, sp, vb, tx, ph):
        o.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    print("| volume | faces (textured) | photo run | `k_ph_resolve` | visib run | photo / visib | pixels/s | share of 6.3 TB/s | own / cross MAE |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(r)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
