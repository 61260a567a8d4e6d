"""CPU: the renderer's host side.  The float64 reference the GPU tests compare with (tests/render_ref.py) against known answers; the ambiguity
cap of every parity case (asserted in f64 on the reference alone); the C entry mhe_render_mesh_f32 (csrc/render.hip) declared, exported, bound
and refusing bad arguments before any launch; the Python error paths, all raised on CPU tensors; ManoLayer's state_dict keys and its
render() without a vertex."""
import os
import re

import numpy as np
import pytest
import torch

import render_ref
from conftest import ROOT
from mhentropy_amd import _lib, criteria, ops, synth
from mhentropy_amd.ManoLayer import ManoLayer

NAME = "mhe_render_mesh_f32"


def _norm(X, G):
    """sample coordinate X (sample j sits at X = j) -> normalised image coordinate"""
    return (np.asarray(X, np.float64) + 0.5) * 2.0 / G - 1.0


def _one(verts_xyz, faces, size, aa, **kw):
    return render_ref.render64(np.asarray(verts_xyz, np.float64)[None], np.asarray(faces), [1.0], [[0.0, 0.0]], size=size, anti_aliasing=aa, **kw)


def test_right_triangle_covers_the_counted_samples():
    G = 8
    # legs on X = -0.5 and Y = -0.5, hypotenuse X + Y = 4.5: samples with X + Y <= 4, 5 + 4 + 3 + 2 + 1 of them
    v = [[_norm(-0.5, G), _norm(-0.5, G), 0.0], [_norm(5.0, G), _norm(-0.5, G), 0.0], [_norm(-0.5, G), _norm(5.0, G), 0.0]]
    ref = _one(v, [[0, 1, 2]], G, False)
    j, i = np.meshgrid(np.arange(G), np.arange(G))
    assert np.array_equal(ref["mask"][0], (i + j <= 4).astype(np.float64)) and ref["mask"].sum() == 15
    assert ref["n_ambiguous"][0] == 0 and np.isclose(ref["edge"][0, 0, 0], 0.5) and np.isclose(ref["edge"][0, 2, 2], 0.5 / np.sqrt(2.0))
    assert np.array_equal(ref["depth"][0] == 100.0, ref["mask"][0] == 0)


def test_quad_covers_a_known_pixel_block_with_quarter_steps():
    S, G = 8, 16
    # sample columns 3..9 and rows 3..7: pixel column 1 and pixel row 1 are half covered, columns 2..4 and rows 2..3 whole
    x0, x1, y0, y1 = _norm(2.5, G), _norm(9.5, G), _norm(2.5, G), _norm(7.5, G)
    ref = _one([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0]], [[0, 1, 2], [0, 2, 3]], S, True)
    want = np.zeros((S, S))
    want[1, 1], want[1, 2:5], want[2:4, 1], want[2:4, 2:5] = 0.25, 0.5, 0.5, 1.0
    assert np.array_equal(ref["mask"][0], want)
    # a diagonal cut gives the three-quarter pixels: under X + Y = 7.5 a pixel with row + column = 3 keeps its samples 6, 7, 7 and loses 8
    tri = _one([[_norm(-0.5, G), _norm(-0.5, G), 0], [_norm(8.0, G), _norm(-0.5, G), 0], [_norm(-0.5, G), _norm(8.0, G), 0]], [[0, 1, 2]], S, True)
    assert set(np.unique(tri["mask"])) == {0.0, 0.75, 1.0} and tri["mask"][0, 0, 3] == 0.75 and tri["mask"][0, 2, 1] == 0.75 and tri["mask"][0, 1, 1] == 1.0
    assert set(np.unique(ref["mask"])) | set(np.unique(tri["mask"])) == {0.0, 0.25, 0.5, 0.75, 1.0}


def test_depth_of_a_tilted_plane_is_the_plane_at_the_sample_centres():
    G = 12
    plane = lambda x, y: 0.3 * x + 0.2 * y + 0.1
    c = [(-0.83, -0.79), (0.81, -0.77), (0.85, 0.9), (-0.9, 0.8)]
    v = [[x, y, plane(x, y)] for x, y in c]
    for zs in (None, [250.0]):
        ref = _one(v, [[0, 1, 2], [0, 2, 3]], G, False, zscale=zs)
        x = _norm(np.arange(G), G)
        want = plane(x[None, :], x[:, None]) * (1.0 if zs is None else 0.25)
        hit = ref["mask"][0] == 1
        assert hit.sum() > 60 and np.abs(ref["depth"][0][hit] - want[hit]).max() < 1e-12 and (ref["depth"][0][~hit] == 100.0).all()
    # anti-aliased: the pixel holds the NEAREST of its covered samples
    ref = _one(v, [[0, 1, 2], [0, 2, 3]], G // 2, True)
    want = plane(x[None, :], x[:, None]).reshape(G // 2, 2, G // 2, 2).min((1, 3))
    full = ref["mask"][0] == 1
    assert full.sum() > 10 and np.abs(ref["depth"][0][full] - want[full]).max() < 1e-12


def test_either_winding_gives_the_same_image():
    v, f = render_ref.sheet(11, 6, 6)
    a = render_ref.render64(v[None], f, [0.9], [[0.05, -0.02]], [80.0], 16, True)
    b = render_ref.render64(v[None], f[:, ::-1], [-0.9], [[0.05, -0.02]], [80.0], 16, True)          # ... and the sign of the scale is ignored
    assert np.array_equal(a["mask"], b["mask"]) and np.allclose(a["depth"], b["depth"], rtol=0, atol=1e-15) and a["mask"].sum() > 100


def test_degenerate_and_out_of_range_faces_cover_nothing():
    v = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.0, 0.5, 0], [0.0, -0.5, 0]], np.float64)          # 0, 3, 1 are collinear
    good = _one(v, [[0, 1, 2]], 16, True)
    more = _one(v, [[0, 1, 2], [0, 0, 2], [0, 3, 1], [0, 1, 7], [-1, 1, 2]], 16, True)
    assert np.array_equal(good["mask"], more["mask"]) and np.array_equal(good["depth"], more["depth"])


@pytest.mark.parametrize("name", sorted(render_ref.CASES))
def test_parity_cases_stay_under_the_ambiguity_cap(name):
    operands, ref = render_ref.case(name)
    print(f"{name}: {ref['ambiguous_fraction']:.4%} of the samples within {render_ref.EDGE} of an edge, nearest {render_ref.skipped_edge_distance(ref):.2e}")
    assert ref["ambiguous_fraction"] <= render_ref.CAP
    assert 0.02 < ref["mask"].mean() < 0.98 and ref["ambiguous"].mean() < 0.05          # a case that checks nothing would pass the cap too
    build, R, S, aa = render_ref.CASES[name]
    assert operands["verts"].shape[0] == R and ref["mask"].shape == (R, S, S)
    if name == "crossing_64aa":
        assert operands["verts"].shape[1:] == (784, 3) and operands["faces"].shape == (1458, 3)
    if name == "smpl_64aa":
        assert operands["verts"].shape[1:] == (6890, 3) and operands["faces"].shape == (13776, 3) and operands["faces"].max() == 6889
    if name == "one_face":
        assert operands["verts"].shape[1:] == (3, 3) and operands["faces"].shape == (1, 3)


def test_symbol_declared_and_bound_with_matching_arity():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhe.h")).read(), flags=re.S)
    L = _lib.lib()
    m = re.search(rf"\b{NAME}\s*\(([^)]*)\)\s*;", src)
    assert m, f"{NAME} is not declared in include/mhe.h"
    assert NAME in _lib.SIGNATURES and hasattr(L, NAME)
    assert len(_lib.SIGNATURES[NAME][1]) == len(m.group(1).split(",")) == 17
    assert L.mhe_abi_version() == 4
    assert "render.hip" in __import__("mhentropy_amd.build", fromlist=["SOURCES"]).SOURCES
    assert callable(ops.render_mesh) and callable(criteria.silhouette_iou)


def test_entry_refuses_bad_arguments_before_any_launch():
    L, Z = _lib.lib(), None
    R, B, V, F, S = 4, 2, 5, 3, 16
    f = lambda *s: torch.zeros(*s)
    A = lambda t: Z if t is None else _lib.C.c_void_p(t.data_ptr())          # host addresses: every call below must return before a kernel could read them
    t = dict(verts=f(R, V, 3), faces=torch.zeros(F, 3, dtype=torch.int32), scale=f(R), trans=f(R, 2), zscale=f(R), target=f(B, S, S), mask=f(R, S, S),
             depth=f(R, S, S), iou=f(R, 2))

    def call(r=R, b=B, v=V, nf=F, s=S, far=100.0, **over):
        a = dict(t, **over)
        return L.mhe_render_mesh_f32(*(A(a[k]) for k in ("verts", "faces", "scale", "trans", "zscale", "target", "mask", "depth", "iou")), r, b, v, nf, s, 1, far, Z)
    bad = {"null verts": dict(verts=None), "null faces": dict(faces=None), "null scale": dict(scale=None), "null trans": dict(trans=None),
           "no output": dict(mask=None, depth=None, iou=None), "S = 7": dict(s=7), "S = 257": dict(s=257), "S = 0": dict(s=0),
           "iou_sums without target": dict(target=None), "R % B": dict(r=3), "B = 0": dict(b=0), "R = 0": dict(r=0), "V = 0": dict(v=0), "F = 0": dict(nf=0),
           "far is NaN": dict(far=float("nan")), "mask overlaps verts": dict(mask=t["verts"]), "depth is mask": dict(depth=t["mask"]),
           "iou_sums overlaps target": dict(iou=t["target"])}
    for what, kw in bad.items():
        assert call(**kw) == 1 and NAME.encode() in L.mhe_last_error(), what          # MHE_ERR_ARG
    assert call(s=257) == 1 and b"S in 8..256" in L.mhe_last_error()
    assert call(target=None) == 1 and b"iou_sums needs target" in L.mhe_last_error()
    assert call(r=3) == 1 and b"multiple of B" in L.mhe_last_error()
    assert call(mask=t["verts"]) == 1 and b"overlaps" in L.mhe_last_error()


def test_python_error_paths_on_cpu_tensors():
    R, V, S = 2, 5, 16
    v, fc, s, tr = torch.zeros(R, V, 3), torch.zeros(3, 3, dtype=torch.int32), torch.ones(R), torch.zeros(R, 2)
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        ops.render_mesh(v, fc, s, tr)
    with pytest.raises(_lib.MheError, match=r"\[R,V,3\]"):
        ops.render_mesh(v[0], fc, s, tr)
    with pytest.raises(_lib.MheError, match=r"\[F,3\]"):
        ops.render_mesh(v, fc[:, :2], s, tr)
    with pytest.raises(ValueError, match="want="):
        ops.render_mesh(v, fc, s, tr, want=("mask", "normals"))
    with pytest.raises(ValueError, match="needs target"):
        ops.render_mesh(v, fc, s, tr, want=("iou_sums",))
    for size in (7, 257):
        with pytest.raises(ValueError, match="size="):
            ops.render_mesh(v, fc, s, tr, size=size)
    lt, hm = torch.zeros(3, R, 3), torch.zeros(R, 64, 64, dtype=torch.bool)
    with pytest.raises(ValueError, match="verts must be"):
        criteria.silhouette_iou(torch.zeros(3, R, V, 2), lt, fc, hm, size=S)
    with pytest.raises(ValueError, match="logs_t must be"):
        criteria.silhouette_iou(torch.zeros(3, R, V * 3), lt[:2], fc, hm, size=S)
    with pytest.raises(ValueError, match="hand_mask must be"):
        criteria.silhouette_iou(torch.zeros(3, R, V * 3), lt, fc, hm[:1], size=S)
    with pytest.raises(ValueError, match="multiple of size"):
        criteria.silhouette_iou(torch.zeros(3, R, V * 3), lt, fc, torch.zeros(R, 40, 40), size=S)
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):          # valid shapes pass the checks and reach the device check
        criteria.silhouette_iou(torch.zeros(3, R, V * 3), lt, fc, hm, size=S)


def test_mano_layer_keeps_its_state_dict_keys_and_renders_nothing_without_a_vertex():
    layer = ManoLayer(skeidx="RHD", use_pca=True, ncomps=45, mask_sz=64, tables=synth.mano_tables(0))
    names = ("betas", "shapedirs", "posedirs", "v_template", "J_regressor", "weights", "faces", "hands_mean", "comps", "selected_comps")
    assert set(layer.state_dict()) == {"mano_layer.th_" + n for n in names}
    fi = layer.mano_layer.faces_i32
    assert fi.dtype == torch.int32 and fi.is_contiguous() and torch.equal(fi.long(), layer.mano_faces)
    assert layer.render(torch.ones(3, 1), torch.zeros(3, 2)) == {}
    assert layer.render(torch.ones(3, 1), torch.zeros(3, 2), vertex=None, norm=torch.ones(3), render=["mask", "depth"]) == {}
    with pytest.raises(ValueError, match="norm="):
        layer.render(torch.ones(3, 1), torch.zeros(3, 2), vertex=torch.zeros(3, 778, 3))
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        layer.render(torch.ones(3, 1), torch.zeros(3, 2), vertex=torch.zeros(3, 778, 3), norm=torch.ones(3), render=["mask", "depth"])
