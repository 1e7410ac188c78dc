"""CPU suite: small-component removal of the fused surface -- properties of the NumPy restatement (tests/clean_ref.py), its
calibration on the sphere-26 and ring-6 surfaces of DESIGN.md 13 / 15 (fused by tests/fusion_ref.py, filtered by
tests/consist_ref.py), and parameter validation of the device stage (sfmx_clean_check_params needs no device).

Bounds: 1.25 x the value the restatement gives on the fixture, rounded up to the next integer (counts) or to half a percentage
point (shares, on the distance to 100 %); DESIGN.md 16 has the table.  Three rows are conditions and are stated exactly."""
import importlib
import inspect

import numpy as np
import pytest

import clean_ref as LR
import consist_ref as CR
import fusion_ref as FR
import helpers as H
import stereo_ref as SR

capi = importlib.import_module(H.PKG_NAME + ".capi")
pipe = importlib.import_module(H.PKG_NAME + ".pipeline")
synth = importlib.import_module(H.PKG_NAME + ".synth")

# measured -> bound, all at the default 10 permille
NOISY_OFF_SHELL = 85      # 68 vertices more than one voxel off the sphere after cleaning (10 461 before)
NOISY_ON_DROPPED = 40     # 32 vertices within one voxel of the sphere are dropped with their islands
RING_OFF_OFF_SHELL = 80   # ring-6, filter off: 64 vertices outside the shell after cleaning (158 before); they hang on the main part
RING_OFF_ON_DROPPED = 1025  # 820 vertices inside the shell are dropped
RING_OFF_OUTWARD = 0.87   # 89.83 % of the faces point outward after cleaning (88.63 % before)
RING_ON_ON_DROPPED = 310  # ring-6, filter on: 248 vertices inside the shell are dropped
RING_ON_OUTWARD = 0.97    # 97.90 % (97.69 % before)


@pytest.fixture(scope="module")
def soup():
    return LR.soup(3000, 800)  # near the threshold of the giant component: sizes 1, 2, 3, 4, 5, 9 and 631


# ---- properties ------------------------------------------------------------------------------------------------------------
def test_identity_at_zero_zero():
    """every component with a face is kept; with every vertex used the output is the input byte for byte"""
    v, f = LR.strip(300, "permuted")
    v2, f2 = LR._verts(150), np.arange(150, dtype=np.int32).reshape(50, 3)  # 50 components of one face
    for vv, ff in ((v, f), (v2, f2)):
        nrm = vv[::-1].copy()
        r = LR.clean(vv, ff, nrm, 0, 0)
        assert r["verts"].tobytes() == vv.tobytes() and r["faces"].tobytes() == ff.tobytes() and r["normals"].tobytes() == nrm.tobytes()
        assert (r["vert_src"] == np.arange(len(vv))).all() and (r["face_src"] == np.arange(len(ff))).all()


def test_idempotent(soup):
    v, f, nrm = soup
    for params in (dict(), dict(min_faces=2, min_permille=0), dict(min_permille=1000)):
        a = LR.clean(v, f, nrm, **params)
        b = LR.clean(a["verts"], a["faces"], a["normals"], **params)
        assert b["verts"].tobytes() == a["verts"].tobytes() and b["faces"].tobytes() == a["faces"].tobytes()
        assert b["normals"].tobytes() == a["normals"].tobytes() and b["n_verts"] == a["n_verts"] > 0


def test_kept_set_is_monotone_in_each_parameter(soup):
    v, f, _ = soup
    for key, values in (("min_faces", (0, 1, 2, 3, 5, 10, 100, 10000)), ("min_permille", (0, 1, 2, 5, 10, 100, 500, 999, 1000))):
        prev = None
        for x in values:
            r = LR.clean(v, f, **{"min_permille": 0, key: x})
            if prev is not None:
                assert set(r["face_src"].tolist()) <= set(prev["face_src"].tolist()), (key, x)
                assert set(r["vert_src"].tolist()) <= set(prev["vert_src"].tolist()), (key, x)
            prev = r
    sizes = np.unique(LR.clean(v, f)["comp_faces"])
    assert len(sizes) > 3, "the soup has components of several sizes, so the parameters bite"
    assert LR.clean(v, f, min_faces=10000)["n_faces"] == 0 and LR.clean(v, f, min_permille=1000)["n_faces"] == sizes.max()


def test_face_order_changes_neither_labels_nor_kept_set(soup):
    v, f, _ = soup
    perm = np.random.default_rng(11).permutation(len(f))
    for params in (dict(), dict(min_faces=2, min_permille=0), dict(min_permille=500)):
        a, b = LR.clean(v, f, **params), LR.clean(v, f[perm], **params)
        assert (a["label"] == b["label"]).all() and (a["comp_faces"] == b["comp_faces"]).all()
        assert (a["vert_src"] == b["vert_src"]).all() and a["verts"].tobytes() == b["verts"].tobytes()
        assert set(perm[b["face_src"]].tolist()) == set(a["face_src"].tolist())
        assert LR.counts(a) == LR.counts(b)


def test_labels_are_the_smallest_index(soup):
    v, f, _ = soup
    lab = LR.labels(len(v), f)
    assert (lab <= np.arange(len(v))).all() and (lab[lab] == lab).all()
    assert (lab[f[:, 0]] == lab[f[:, 1]]).all() and (lab[f[:, 0]] == lab[f[:, 2]]).all()
    for r in np.unique(lab)[:50]:
        assert np.nonzero(lab == r)[0].min() == r
    # the fallback union-find agrees with scipy's components
    import sys
    saved = {k: sys.modules.get(k) for k in ("scipy", "scipy.sparse", "scipy.sparse.csgraph")}
    try:
        for k in saved:
            sys.modules[k] = None  # import raises ImportError
        assert (LR.labels(len(v), f) == lab).all()
    finally:
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m
    for order in ("ascending", "descending", "permuted"):
        sv, sf = LR.strip(500, order)
        assert (LR.labels(len(sv), sf) == 0).all()


def test_two_equal_components_both_survive_1000_permille():
    v = LR._verts(7)
    f = np.array([[0, 1, 2], [4, 5, 6]], np.int32)
    r = LR.clean(v, f, min_permille=1000)
    assert r["n_faces"] == 2 and r["components"] == 2 and r["largest"] == 1 and list(r["vert_src"]) == [0, 1, 2, 4, 5, 6]
    assert list(r["label"]) == [0, 0, 0, 3, 4, 4, 4] and list(r["comp_faces"]) == [1, 1, 1, 0, 1, 1, 1]
    assert LR.clean(v, f, min_faces=2, min_permille=0)["n_faces"] == 0, "all kept or all dropped: there is no tie-break"


def test_an_unused_vertex_is_always_dropped(soup):
    v, f, _ = soup
    used = np.zeros(len(v), bool)
    used[f.ravel()] = True
    assert (~used).sum() > 10
    r = LR.clean(v, f, min_faces=0, min_permille=0)
    assert (r["vert_src"] == np.nonzero(used)[0]).all() and r["n_faces"] == len(f)
    assert (r["comp_faces"][~used] == 0).all() and (r["label"][~used] == np.nonzero(~used)[0]).all()
    e = LR.clean(np.zeros((5, 3)), np.zeros((0, 3), np.int32), min_permille=0)
    assert LR.counts(e) == dict(n_verts=0, n_faces=0, components=0, largest=0) and list(e["label"]) == [0, 1, 2, 3, 4]
    z = LR.clean(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    assert LR.counts(z) == dict(n_verts=0, n_faces=0, components=0, largest=0)
    for bad in (5, -1):
        with pytest.raises(ValueError):
            LR.clean(np.zeros((5, 3)), np.array([[0, 1, bad]], np.int32))


def test_repeated_indices_inside_a_face():
    v = LR._verts(6)
    f = np.array([[3, 3, 3], [0, 0, 1], [5, 4, 4]], np.int32)
    r = LR.clean(v, f, min_permille=0)
    assert list(r["label"]) == [0, 0, 2, 3, 4, 4] and list(r["comp_faces"]) == [1, 1, 0, 1, 1, 1]
    assert list(r["vert_src"]) == [0, 1, 3, 4, 5] and r["faces"].tolist() == [[2, 2, 2], [0, 0, 1], [4, 3, 3]]


# ---- calibration -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere26():
    noisy, _ = CR.sphere26(True)
    vol = CR.SPHERE26_VOL
    raw = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], noisy)
    filt = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], CR.filtered_views(noisy, CR.filter_views(noisy)))
    return {k: (m["verts"], m["faces"], LR.sphere_off_shell(m["verts"], vol["voxel"])) for k, m in (("raw", raw), ("filtered", filt))}


@pytest.fixture(scope="module")
def ring6():
    images, K, poses, pairs = CR.ring_frames(synth, CR.RING6_ANGLES, 320, 240)
    views = []
    for a, b in pairs:
        r = SR.rectify(K, poses[a][0], poses[a][1], poses[b][0], poses[b][1])
        il, ir = (images[b], images[a]) if r["swapped"] else (images[a], images[b])
        views.append((r, SR.disparity(il, ir, r["H_l"], r["H_r"], dict(num_disparities=64))))
    vol = CR.RING6_VOL
    out = {}
    for k, vs in (("off", views), ("on", CR.filtered_views(views, CR.filter_views(views)))):
        m = FR.fuse(vol["origin"], vol["voxel"], vol["dims"], vs)
        out[k] = (m["verts"], m["faces"], LR.ring_off_shell(m["verts"]))
    return out


def _row(name, surface, table, islands_at_1=True):
    v, f, off = surface
    fig = LR.figures(v, f, off)
    print("%s: %d components, %d faces, largest %d, next %d; off-shell %d -> %d, on-shell dropped %d, faces after %d"
          % (name, fig["components"], fig["faces"], fig["largest"], fig["second"], fig["off_before"], fig["off_after"],
             fig["on_dropped"], fig["faces_after"]))
    # the descriptive columns of DESIGN.md 16's table: the restatements are deterministic, so they are stated exactly
    assert (fig["components"], fig["faces"], fig["largest"], fig["second"]) == table, name
    assert fig["components"] > 1 and fig["second"] * 1000 < fig["largest"] * 5, "the next component is below 5 permille"
    assert (fig["second"] * 1000 >= fig["largest"]) == islands_at_1, "and at or above 1 permille where islands come back"
    # the default sits inside a plateau: 5 .. 1000 permille keep exactly the largest component; at 1 the first islands return
    # (not on the filtered sphere, whose next component has 12 faces)
    for pm in (5, 10, 100, 1000):
        assert LR.clean(v, f, min_permille=pm)["n_faces"] == fig["largest"], (name, pm)
    assert (LR.clean(v, f, min_permille=1)["n_faces"] > fig["largest"]) == islands_at_1, name
    return fig


def test_sphere26_calibration(sphere26):
    raw = _row("sphere-26, 5 % outliers, unfiltered", sphere26["raw"], (623, 59546, 45976, 224))
    assert raw["off_after"] <= NOISY_OFF_SHELL and raw["on_dropped"] <= NOISY_ON_DROPPED
    assert raw["off_before"] > 10 * raw["off_after"], "the unfiltered surface is not bad enough to show that cleaning acts"
    assert raw["off_before"] > 10 * NOISY_OFF_SHELL
    filt = _row("sphere-26, 5 % outliers, filtered", sphere26["filtered"], (9, 45632, 45580, 12), islands_at_1=False)
    assert filt["off_before"] > 0 and filt["off_after"] == 0 and filt["on_dropped"] == 0


def test_ring6_calibration(ring6):
    off = _row("ring-6, filter off", ring6["off"], (77, 34658, 33534, 98))
    assert off["off_after"] <= RING_OFF_OFF_SHELL and off["on_dropped"] <= RING_OFF_ON_DROPPED
    c = off["ref"]
    q0, q1 = CR.mesh_quality(*ring6["off"][:2]), CR.mesh_quality(c["verts"], c["faces"])
    print("filter off: outward %.4f -> %.4f" % (q0[0], q1[0]))
    assert q1[0] >= RING_OFF_OUTWARD and q1[0] > q0[0]
    on = _row("ring-6, filter on", ring6["on"], (26, 13622, 13378, 34))
    c = on["ref"]
    q0, q1 = CR.mesh_quality(*ring6["on"][:2]), CR.mesh_quality(c["verts"], c["faces"])
    print("filter on: outward %.4f -> %.4f" % (q0[0], q1[0]))
    assert on["off_after"] == 0 and q1[1] == 1.0, "every vertex in the shell"
    assert on["on_dropped"] <= RING_ON_ON_DROPPED and q1[0] >= RING_ON_OUTWARD and q1[0] > q0[0]


# ---- library and Python layer ----------------------------------------------------------------------------------------------
def test_check_params():
    assert capi.clean_default_params() == dict(min_faces=0, min_permille=10)
    assert capi.clean_default_params() == capi.CLEAN_DEFAULTS == LR.DEFAULTS
    assert capi.clean_check_params()
    assert capi.clean_check_params(min_faces=0, min_permille=0)
    assert capi.clean_check_params(min_faces=2 ** 31 - 1, min_permille=1000)
    for bad in (dict(min_faces=-1), dict(min_permille=-1), dict(min_permille=1001), dict(min_faces=-2 ** 31)):
        assert not capi.clean_check_params(**bad), bad
    lib = capi.load_library()
    assert lib.sfmx_clean_check_params(None) == capi.SFMX_ERR_INVALID
    lib.sfmx_clean_default_params(None)  # tolerated


def test_python_layer_rejects_unknown_keys():
    with pytest.raises(TypeError):
        capi.clean_params(min_area=1.0)
    assert set(pipe.CLEAN_KEYS) == set(capi.CLEAN_DEFAULTS)
    args = (None, np.zeros((2, 4, 4), np.uint8), np.eye(3), [np.zeros(12)] * 2, [(0, 1)], (0.0, 0.0, 0.0), 0.1, (2, 2, 2))
    for bad in (dict(min_area=1), dict(min_faces=1, permille=5)):
        with pytest.raises(TypeError):
            pipe.fuse(*args, clean=bad)
    assert inspect.signature(pipe.fuse).parameters["clean"].default is False
    assert hasattr(capi.Context, "clean") and hasattr(capi.Clean, "fusion")
    lib = pipe.load_host_library()
    assert hasattr(lib, "sfmx_host_fusion_mesh_cl")
