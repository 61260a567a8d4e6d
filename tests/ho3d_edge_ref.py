"""Designed decoded HO3D samples for the edges of csrc/ho3d.hip, and a census of the edges a sample reaches.  A helper module
(numpy only), not a test; used by test_ho3d_edge_ref_host.py, test_gpu_ho3d_edges.py and oracle/gen_golden.py:gen_ho3d_edges.

Construction.  cam = [[512,0,320],[0,512,240],[0,0,1]], joints at z = -0.5 m and x, y multiples of 1/1024 m (or, for a few
joints, of 2^-18 m): x = k/1024 gives k*125/128 mm, times 512 = k*500, over z = 500 mm = k, so u = k + 320 and v = m + 240 with
every intermediate exact in float32 and in float64 (joints at z = -0.25 / -1 m: 2k and k/2).  An object with zero rotation and
translation (0, 0, -0.5) projects the same way.  Box extents, crop sizes, .5 ties and crop-space uv are therefore chosen, not drawn.

Keys.  A key is "<case>" or "<case>/<sub>": the case named before the slash is the designed sample that must hit it (one sample
of 21 joints decides 21 visibilities, so the per-joint keys of a visibility pass share one sample).  REQUIRED lists them.

Two edges a census of this kind could name are unreachable for any input the reference accepts, and are proved so instead
(test_ho3d_edge_ref_host.py checks both statements over a sweep):
  * an ODD crop width: centre c is an integer (int()), size s a float32; away from ties rint(c - s) = c - rint(s) and
    rint(c + s) = c + rint(s); at a tie both c - s and c + s are half-integers and both go to the even neighbour; either way
    x2 - x1 is even;
  * the clamp min(floor(X * cw / 256), cw - 1) TAKEN: cw / 256 and X * (cw / 256) are exact in float64, X <= 255, so
    floor(X cw / 256) <= cw - ceil(cw / 256) <= cw - 1 for cw >= 1; cw = 0 is an empty crop, on which the reference raises.
    What is reachable, and is a key, is the clamp's bound met with equality (output column 255 reads source column cw - 1)."""
import functools
import math

import numpy as np

from oracle import ho3d_ref as R

CAM = np.array([[512, 0, 320], [0, 512, 240], [0, 0, 1]], np.float32)
D_PASS, D_FAIL = 3681, 3680          # 16-bit depth values: 500 mm - v * 0.12498664727900177 mm is 39.92 / 40.05
IDENT = (1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0)
EPS = float(np.finfo(np.float64).eps)


# ---- building blocks ---------------------------------------------------------------------------------------------------------
def pt(u, v, z=-0.5):
    """the camera-space point (metres, OpenGL axes) that projects to pixel (u, v) exactly"""
    k = -z / 0.5
    return [(u - 320) / 1024 * k, -(v - 240) / 1024 * k, z]


def grid(u0, v0, du, dv):
    """21 joints on a 5-wide lattice from (u0, v0)"""
    return [(u0 + (i % 5) * du, v0 + (i // 5) * dv) for i in range(21)]


def box_points(mnx, mxx, mny, mxy, n):
    """n pixel positions inside [mnx, mxx] x [mny, mxy]; the two extreme corners come LAST (the highest lanes of the last pass
    of the kernel's 64-lane loop carry the extent)"""
    if n == 1:
        return [(mnx, mny)]
    w, h = max(int(mxx - mnx) - 2, 1), max(int(mxy - mny) - 2, 1)
    inner = [(mnx + 1 + (i * 37) % w, mny + 1 + (i * 61) % h) for i in range(n - 2)]
    return inner + [(mxx, mxy), (mnx, mny)]


@functools.lru_cache(maxsize=None)
def pattern_image():
    v, u, c = np.meshgrid(np.arange(480), np.arange(640), np.arange(3), indexing="ij")
    return ((u * 7 + v * 13 + c * 101 + (u * v) % 17) % 256).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pattern_depth16():
    v, u = np.meshgrid(np.arange(480), np.arange(640), indexing="ij")
    return ((u * 3 + v * 5) % 29 + 3670).astype(np.uint16)              # straddles the 40 mm test of a joint at 500 mm


@functools.lru_cache(maxsize=None)
def pattern_seg():
    a, b, c = np.meshgrid(np.arange(120), np.arange(160), np.arange(3), indexing="ij")
    return np.array([0, 200, 201, 255, 230], np.uint8)[(a * 3 + b * 5 + c * 2 + (a * b) % 3) % 5]


def depth_png(d16):
    out = np.full(d16.shape + (3,), 77, np.uint8)                       # channel 0 is never read
    out[:, :, 2], out[:, :, 1] = d16 & 255, d16 >> 8
    return out


def sample(joints_uv, obj_uv, rot=(0, 0, 0), image=None, d16=None, seg=None, joints_z=None):
    z = [-0.5] * 21 if joints_z is None else joints_z
    joints = np.array([pt(u, v, zz) for (u, v), zz in zip(joints_uv, z)], np.float32)
    off = np.array([[((i * 5) % 7 - 3) / 1024, ((i * 3) % 5 - 2) / 1024, ((i * 11) % 9 - 4) / 2048] for i in range(778)])
    mesh = (joints[np.arange(778) % 21].astype(np.float64) + off).astype(np.float32)
    verts = np.array([pt(u, v) for u, v in obj_uv], np.float32) - np.array([0, 0, -0.5], np.float32)
    return {"image": pattern_image().copy() if image is None else image, "depth_png": depth_png(pattern_depth16() if d16 is None else d16),
            "seg": pattern_seg().copy() if seg is None else seg, "joints3d": joints, "mesh": mesh, "cam": CAM.copy(),
            "obj_rot": np.array(rot, np.float32), "obj_trans": np.array([0, 0, -0.5], np.float32), "obj_verts": verts}


def generic(obj_box, hand=None, n=1000, **kw):
    """the object box decides the crop; the hand is a 16 x 16 pixel lattice inside it unless given"""
    mnx, mxx, mny, mxy = obj_box
    if hand is None:
        hand = grid(int((mnx + mxx) / 2) - 8, int((mny + mxy) / 2) - 8, 4, 4)
    return sample(hand, box_points(mnx, mxx, mny, mxy, n), **kw)


def _cells(seg, u0, v0, ch, val):
    """set channel ch of every seg cell the 9x9 window about (u0, v0) touches (inside the image)"""
    for v in range(max(v0 - 4, 0), min(v0 + 5, 480)):
        for u in range(max(u0 - 4, 0), min(u0 + 5, 640)):
            seg[v >> 2, u >> 2, ch] = val


VIS1_JOINTS = ["hand200", "hand201", "objchan_only", "depth_fail_by_a_step", "depth_pass_by_a_step", "depth_eq_40mm", "corner_mm",
               "corner_mp", "corner_pm", "corner_pp", "seg_cell_boundary", "cut_left", "cut_top", "cut_bottom", "u_neg_frac",
               "window_off_image"]
VIS1_EXPECT = [0, 1, 0, 0, 1, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0, 0, 0]


def vis1_sample():
    """one joint per decision of the first visibility pass (VIS1_JOINTS in joint order, with joint 12 between cut_left and cut_top,
    then four joints over bare background); seg and depth are zero except where a joint needs them.  Joint 12 at u = 638 passes
    the first pass and fails the second: x is clamped at 480, so with joints on the left no crop reaches u = 634; the right
    border has a sample of its own, vis1_right."""
    seg, d16 = np.zeros((120, 160, 3), np.uint8), np.zeros((480, 640), np.uint16)
    uv = [(100, 100), (140, 100), (180, 100), (220, 100), (260, 100), (320, 240), (100, 200), (140, 200), (180, 200), (220, 200), (262, 200),
          (2, 300), (638, 300), (300, 2), (340, 478), (-0.5, 400), (-100, 100), (400, 300), (440, 300), (400, 340), (440, 340)]
    z = [-0.5] * 21
    z[5] = -0.04                                                   # float32(0.04) * 1000 rounds to 40.0: d - 0 == 40 exactly
    win = lambda j, val: d16.__setitem__((slice(uv[j][1] - 4, uv[j][1] + 5), slice(uv[j][0] - 4, uv[j][0] + 5)), val)
    _cells(seg, 100, 100, 2, 200); win(0, 3700)
    _cells(seg, 140, 100, 2, 201); win(1, 3700)
    _cells(seg, 180, 100, 1, 255); win(2, 3700)
    _cells(seg, 220, 100, 2, 255); win(3, D_FAIL)
    _cells(seg, 260, 100, 2, 255); win(4, D_PASS)
    _cells(seg, 320, 240, 2, 255)                                  # depth stays 0
    for j, (su, sv) in zip((6, 7, 8, 9), ((-4, -4), (-4, 4), (4, -4), (4, 4))):
        _cells(seg, uv[j][0], uv[j][1], 2, 255)
        d16[uv[j][1] + sv, uv[j][0] + su] = 3700
    seg[50, 65, 2] = 255                                           # cell of u 260..263; the cell of u 256..259 stays clear
    d16[200, 259] = d16[200, 260] = 3700
    for j, (pu, pv) in zip((11, 12, 13, 14), ((0, 300), (639, 300), (300, 0), (340, 479))):
        _cells(seg, int(uv[j][0]), int(uv[j][1]), 2, 255)
        d16[pv, pu] = 3700
    seg[100, 1, 2] = 255                                           # u 4..7 at v 400: reached only if int() truncates -0.5 to 0
    d16[400, 4] = 3700
    return sample(uv, box_points(300, 340, 220, 260, 1000), d16=d16, seg=seg, joints_z=z)


def vis1_right_sample():
    """every joint at u >= 400, spread over the image height, so that the crop (x centre 410, size 285) reaches the right border:
    joint 0 at u = 638 has its window cut by u = 640 and its only qualifying pixel at u = 639"""
    seg, d16 = np.zeros((120, 160, 3), np.uint8), np.zeros((480, 640), np.uint16)
    uv = grid(400, 20, 40, 110)
    uv[0] = (638, 240)
    _cells(seg, 638, 240, 2, 255)
    d16[240, 639] = 3700
    return sample(uv, box_points(420, 460, 220, 260, 1000), d16=d16, seg=seg)


def vis2_sample(high):
    """crop size 128 (factor 1): joints at crop uv -4 and -4 - 2^-8 in x and in y (low), 259 and 259 + 2^-8 in x (high).  Hand
    mask and depth qualify everywhere, so the first pass leaves every joint with an in-image window pixel visible.  (uv_y > 259
    with the first pass true would need a joint below the fused box and inside the image: y is only clamped at 640.)"""
    seg, d16 = np.full((120, 160, 3), 255, np.uint8), np.full((480, 640), 3700, np.uint16)
    e = 1.0 / 256
    if high:
        uv = grid(300, 150, 20, 30)
        uv[0], uv[1], uv[2], uv[3] = (483, 200), (483 + e, 230), (482, 260), (479, 290)
        return sample(uv, box_points(224, 500, 100, 356, 1000), d16=d16, seg=seg)
    uv = grid(40, 40, 20, 20)
    uv[0], uv[1], uv[2], uv[3] = (-4, 100), (-4 - e, 120), (100, -4), (120, -4 - e)
    uv[6], uv[7] = (-3, 60), (60, -3)
    return sample(uv, box_points(0, 256, 0, 256, 1000), d16=d16, seg=seg)


def st_sample(kind):
    """compute_st: 'negdet' has u growing (360, 380, 420) where x falls (80, 60, 50 / 1024 m), because u - 320 = 512 x / z with
    z = 1, 0.5, 0.25 m, while v grows with y: a cross-covariance of negative determinant; 'collinear' has every joint on one
    image row, a cross-covariance of rank one"""
    if kind == "collinear":
        return sample([(200 + 7 * i, 240) for i in range(21)], box_points(150, 400, 140, 340, 1000))
    joints = [(320 + (40, 60, 100)[i // 7], 240 + (i % 7 - 3) * 12) for i in range(21)]
    return sample(joints, box_points(300, 560, 120, 360, 1000), joints_z=[(-1.0, -0.5, -0.25)[i // 7] for i in range(21)])


PADDED = (-50, 150, 150, 350)                # object box of the augmentation cases: the crop leaves the image on the left
TWO_PI_MINUS = float(np.nextafter(2 * math.pi, 0.0))

# name -> (builder, augmentation parameters (pn0 pn1 pn2 scale angle tx ty) or None)
CASES = {
    "win_inside": (lambda: generic((200, 400, 150, 350)), None),
    "win_left": (lambda: generic((-50, 150, 150, 350)), None),
    "win_top": (lambda: generic((200, 400, -50, 150)), None),
    "win_right": (lambda: generic((440, 470, 40, 440)), None),
    "win_bottom": (lambda: generic((200, 400, 300, 500)), None),
    "win_two_sides": (lambda: generic((440, 470, 140, 560)), None),
    "win_tie_floor_even": (lambda: generic((100, 201, 150, 240)), None),
    "win_tie_floor_odd": (lambda: generic((101, 202, 151, 241)), None),
    "fuse_x_upper_clamp_negative_extent": (lambda: generic((500, 600, 100, 300)), None),
    "fuse_hy_480_640": (lambda: generic((200, 300, 300, 560)), None),
    "fuse_lower_clamps": (lambda: generic((-50, 150, -50, 150)), None),
    "fuse_both_x_clamps_f64_size": (lambda: generic((-20, 520, 100, 300)), None),
    "fuse_object_dominates": (lambda: generic((180, 420, 130, 330)), None),
    "fuse_hand_dominates": (lambda: generic((290, 300, 230, 240), hand=grid(250, 190, 20, 20)), None),
    "obj_n1": (lambda: generic((300, 300, 240, 240), hand=grid(250, 190, 20, 20), n=1), None),
    "obj_n63": (lambda: generic((200, 400, 150, 350), n=63), None),
    "obj_n64": (lambda: generic((210, 400, 150, 350), n=64), None),
    "obj_n65": (lambda: generic((200, 410, 150, 350), n=65), None),
    "obj_n_not_multiple_of_64": (lambda: generic((200, 400, 160, 350), n=200), None),
    "obj_n_eq_nvmax": (lambda: generic((200, 400, 150, 340), n=1000), None),
    "obj_n_lt_nvmax": (lambda: generic((190, 400, 150, 350), n=130), None),
    "obj_rot_zero": (lambda: generic((220, 400, 150, 350), n=100, rot=(0, 0, 0)), None),
    "obj_rot_1e-20": (lambda: generic((200, 400, 170, 350), n=100, rot=(6e-21, 0, 8e-21)), None),
    "obj_rot_near_pi": (lambda: generic((250, 420, 200, 330), n=100, rot=(0, 0, 3.1412)), None),
    "vis1": (vis1_sample, None),
    "vis1_right": (vis1_right_sample, None),
    "resize_wide": (lambda: generic((440, 470, 60, 420)), None),
    "resize_narrow": (lambda: generic((300, 400, 200, 290)), None),
    "resize_tiny": (lambda: generic((318, 322, 238, 242), hand=grid(316, 236, 2, 2), n=5), None),
    "vis2_low": (lambda: vis2_sample(False), IDENT),
    "vis2_high": (lambda: vis2_sample(True), IDENT),
    "st_negative_det": (lambda: st_sample("negdet"), (1.0, 1.0, 1.0, 0.9, 0.7, 3.0, -2.0)),
    "st_collinear": (lambda: st_sample("collinear"), (1.0, 1.0, 1.0, 0.95, 2.1, -5.0, 4.0)),
    "aug_angle0_tx_half": (lambda: generic(PADDED), (1.0, 1.0, 1.0, 1.0, 0.0, 7.5, -3.5)),
    "aug_angle_half_pi": (lambda: generic(PADDED), (1.0, 1.0, 1.0, 1.0, math.pi / 2, 0.0, 0.0)),
    "aug_angle_pi": (lambda: generic(PADDED), (1.0, 1.0, 1.0, 0.9, math.pi, 3.25, -2.0)),
    "aug_angle_2pi_minus": (lambda: generic(PADDED), (1.0, 1.0, 1.0, 0.9, TWO_PI_MINUS, 0.0, 0.0)),
    "aug_scale08": (lambda: generic(PADDED), (1.0, 1.0, 1.0, 0.8, 1.0, 0.0, 0.0)),
    "aug_scale10": (lambda: generic(PADDED), (1.0, 1.0, 1.0, 1.0, 2.0, 0.0, 0.0)),
    "aug_t_plus40": (lambda: generic(PADDED), (1.0, 1.0, 1.0, 0.9, 0.3, 40.0, 40.0)),
    "aug_t_minus40": (lambda: generic(PADDED), (1.0, 1.0, 1.0, 0.9, 5.9, -40.0, -40.0)),
    "aug_colour06": (lambda: generic(PADDED), (0.6, 0.6, 0.6, 1.0, 0.0, 0.0, 0.0)),
    "aug_colour14": (lambda: generic(PADDED), (1.4, 1.4, 1.4, 1.0, 0.0, 0.0, 0.0)),
    "aug_pad127": (lambda: generic(PADDED), (0.6, 1.4, 1.1, 0.85, 4.0, 12.0, -9.0)),
}

# the pipeline calls of the GPU suite: the first two in evaluation mode, the third in evaluation and in augmented mode.
# NVmax of a batch is its largest object count: the second batch holds every count below it (padded rows).
BATCHES = [
    [n for n in CASES if n.startswith(("win_", "fuse_"))],
    [n for n in CASES if n.startswith(("obj_", "vis1", "resize_"))],
    [n for n in CASES if CASES[n][1] is not None],
]

# the designed cases whose targets the reference's own __getitem__ records (oracle/gen_golden.py:gen_ho3d_edges); all have >= 1000
# object vertices, which the reference's np.random.choice(n, 1000, replace=False) needs.  (name, augmented)
GOLDEN = [("fuse_x_upper_clamp_negative_extent", False), ("fuse_hy_480_640", False), ("fuse_lower_clamps", False),
          ("fuse_both_x_clamps_f64_size", False), ("win_tie_floor_even", False), ("vis1", False), ("vis2_low", False), ("vis2_high", True)]

REQUIRED = (
    ["win_inside", "win_left", "win_top", "win_right", "win_bottom", "win_two_sides", "win_tie_floor_even", "win_tie_floor_odd",
     "fuse_x_upper_clamp_negative_extent", "fuse_hy_480_640", "fuse_lower_clamps", "fuse_both_x_clamps_f64_size", "fuse_object_dominates",
     "fuse_hand_dominates", "obj_n1", "obj_n63", "obj_n64", "obj_n65", "obj_n_not_multiple_of_64", "obj_n_eq_nvmax", "obj_n_lt_nvmax",
     "obj_rot_zero", "obj_rot_1e-20", "obj_rot_near_pi"]
    + ["vis1/" + k for k in VIS1_JOINTS]
    + ["vis1_right/cut_right"]
    + ["vis2_low/eval_at_m4", "vis2_low/eval_below_m4", "vis2_low/aug_at_m4", "vis2_low/aug_below_m4",
       "vis2_high/eval_at_259", "vis2_high/eval_above_259", "vis2_high/aug_at_259", "vis2_high/aug_above_259",
       "resize_wide", "resize_narrow", "resize_tiny", "resize_narrow/last_column_is_cw_minus_1",
       "aug_angle0_tx_half", "aug_angle_half_pi", "aug_angle_pi", "aug_angle_2pi_minus", "aug_scale08", "aug_scale10", "aug_t_plus40",
       "aug_t_minus40", "aug_colour06", "aug_colour06/truncates", "aug_colour14", "aug_colour14/saturates", "aug_pad127",
       "st_negative_det", "st_collinear"])


def build(name):
    """(decoded sample, augmentation parameters [7] float64 or None)"""
    fn, aug = CASES[name]
    return fn(), (None if aug is None else np.array(aug, np.float64))


def aug_dict(a):
    return None if a is None else {"pn": np.asarray(a[:3], np.float64), "scale": float(a[3]), "angle": float(a[4]), "tx": float(a[5]), "ty": float(a[6])}


@functools.lru_cache(maxsize=None)
def _count(name):
    return CASES[name][0]()["obj_verts"].shape[0]


def nvmax_of(batch):
    return max(_count(n) for n in batch)


# ---- census ------------------------------------------------------------------------------------------------------------------
def intermediates(s):
    """the reference's intermediates of one sample, from the oracle's helpers"""
    J = s["joints3d"] * 1000.0
    obj = (np.matmul(s["obj_verts"], R.rodrigues(s["obj_rot"]).T) + s["obj_trans"]) * 1000.0
    J_uvd, obj_uvd = R.xyz2uvd(J, s["cam"]), R.xyz2uvd(obj, s["cam"])
    bh, bo = R.get_bbox_joints(J_uvd[:, :2], 1.5), R.get_bbox_joints(obj_uvd[:, :2], 1.0)
    center, scale = R.fuse_bbox(bh, bo, (480, 640, 3))
    return J_uvd, obj_uvd, bh, bo, center, scale, scale / 2


def _vis1_joint(seg, d16, J_uvd, i):
    """per joint: (u0, v0, d, in-image window pixels [(u, v, hand, obj, margin, d16)])"""
    u0, v0, d = int(J_uvd[i, 0]), int(J_uvd[i, 1]), J_uvd[i, 2]
    px = [(u, v, int(seg[v, u, 2]), int(seg[v, u, 1]), float(d - (d16[v, u] * R.DEPTH_SCALE) * 1000), int(d16[v, u]))
          for u in range(u0 - 4, u0 + 5) for v in range(v0 - 4, v0 + 5) if 0 <= u < 640 and 0 <= v < 480]
    return u0, v0, d, px


def census(s, aug=None, nvmax=None):
    """the set of edge keys (without the case prefix) that sample s (with augmentation aug [7] or None, in a batch padded to
    nvmax object vertices) reaches"""
    keys = set()
    J_uvd, obj_uvd, bh, bo, center, scale, size = intermediates(s)
    x1, y1, x2, y2 = R.crop_window(center, size)
    out = {"win_left": x1 < 0, "win_top": y1 < 0, "win_right": x2 > 640, "win_bottom": y2 > 480}
    keys |= {k for k, v in out.items() if v}
    if sum(out.values()) >= 2:
        keys.add("win_two_sides")
    if not any(out.values()):
        keys.add("win_inside")
    for val in (center[0] - size, center[1] - size, center[0] + size, center[1] + size):
        if float(val) - math.floor(val) == 0.5:
            keys.add("win_tie_floor_even" if math.floor(val) % 2 == 0 else "win_tie_floor_odd")
    # fuse_bbox
    bb = np.concatenate((bh.reshape(2, 2), bo.reshape(2, 2)), 0)
    (mn_x, mn_y), (mx_x, mx_y) = bb.min(0), bb.max(0)
    if mn_x > 480:
        keys.add("fuse_x_upper_clamp_negative_extent")
    if 480 < mx_y < 640:
        keys.add("fuse_hy_480_640")
    if mn_x < 0 and mn_y < 0:
        keys.add("fuse_lower_clamps")
    if mn_x < 0 and mx_x > 480 and 480 >= min(mx_y, 640) - max(0, mn_y) and isinstance(scale, float) and not isinstance(scale, np.floating):
        keys.add("fuse_both_x_clamps_f64_size")
    encloses = lambda a, b: a[0] <= b[0] and a[1] <= b[1] and a[2] >= b[2] and a[3] >= b[3] and not np.array_equal(a, b)
    if encloses(bo, bh):
        keys.add("fuse_object_dominates")
    if encloses(bh, bo):
        keys.add("fuse_hand_dominates")
    # object vertices
    n = s["obj_verts"].shape[0]
    keys |= {k for k, v in {"obj_n1": n == 1, "obj_n63": n == 63, "obj_n64": n == 64, "obj_n65": n == 65,
                            "obj_n_not_multiple_of_64": n > 65 and n % 64 != 0, "obj_n_eq_nvmax": nvmax is not None and n == nvmax,
                            "obj_n_lt_nvmax": nvmax is not None and n < nvmax}.items() if v}
    th = float(np.linalg.norm(np.asarray(s["obj_rot"], np.float64)))
    keys |= {k for k, v in {"obj_rot_zero": th == 0.0, "obj_rot_1e-20": 0.0 < th < EPS and 5e-21 < th < 2e-20,
                            "obj_rot_near_pi": abs(th - math.pi) < 1e-3}.items() if v}
    # first visibility pass
    seg = R.resize_nearest(s["seg"], (640, 480))
    d16 = s["depth_png"][:, :, 2].astype(np.int64) + s["depth_png"][:, :, 1].astype(np.int64) * 256
    for i in range(21):
        u0, v0, d, px = _vis1_joint(seg, d16, J_uvd, i)
        hand = [p for p in px if p[2] > 200]
        Q = [p for p in hand if p[4] < 40]
        okd = [p for p in px if p[4] < 40]
        if not px:
            keys.add("window_off_image")
            continue
        if not Q and okd and max(p[2] for p in okd) == 200:
            keys.add("hand200")
        if Q and max(p[2] for p in Q) == 201:
            keys.add("hand201")
        if not Q and any(p[3] > 200 and p[2] <= 200 for p in okd):
            keys.add("objchan_only")
        step = lambda p, k: float(d - ((p[5] + k) * R.DEPTH_SCALE) * 1000)
        if not Q and hand and any(step(p, 1) < 40 for p in hand):
            keys.add("depth_fail_by_a_step")
        if Q and all(step(p, -1) >= 40 for p in Q):
            keys.add("depth_pass_by_a_step")
        if not Q and any(p[4] == 40.0 for p in hand):
            keys.add("depth_eq_40mm")
        if len(Q) == 1:
            qu, qv = Q[0][0], Q[0][1]
            for nm, (su, sv) in {"corner_mm": (-4, -4), "corner_mp": (-4, 4), "corner_pm": (4, -4), "corner_pp": (4, 4)}.items():
                if (qu, qv) == (u0 + su, v0 + sv):
                    keys.add(nm)
            if qu % 4 == 0 and any(p[0] == qu - 1 and p[1] == qv and p[4] < 40 and p[2] <= 200 for p in px):
                keys.add("seg_cell_boundary")
            if -1 < J_uvd[i, 0] < 0 and qu == 4:
                keys.add("u_neg_frac")
        if Q:
            keys |= {k for k, v in {"cut_left": u0 - 4 < 0 <= u0 and J_uvd[i, 0] >= 0, "cut_right": u0 + 4 >= 640 > u0, "cut_top": v0 - 4 < 0 <= v0,
                                    "cut_bottom": v0 + 4 >= 480 > v0}.items() if v}
    # second visibility pass: crop uv as the reference forms it (float32 array; float64 after the augmentation's np.dot)
    if float(size) == 128.0:
        uv = J_uvd[:, :2].copy()
        uv[:, 0] = (uv[:, 0] - center[0] + size) * (256.0 / (size * 2))
        uv[:, 1] = (uv[:, 1] - center[1] + size) * (256.0 / (size * 2))
        mode = "eval"
        if aug is not None:
            a = aug_dict(aug)
            rot = R.get_rotation_matrix_2d((128, 128), -180.0 * a["angle"] / math.pi, a["scale"])
            rot[0, 2] += a["tx"]; rot[1, 2] += a["ty"]
            uv, mode = np.dot(rot, np.concatenate([uv, np.ones((21, 1))], 1).T).T, "aug"
        e = 2.0 ** -8
        for k, v in {"at_m4": (uv == -4).any(), "below_m4": ((uv < -4) & (uv >= -4 - e)).any(), "at_259": (uv == 259).any(),
                     "above_259": ((uv > 259) & (uv <= 259 + e)).any()}.items():
            if v:
                keys.add(mode + "_" + k)
    # resize
    cw = x2 - x1
    keys |= {k for k, v in {"resize_wide": cw > 256, "resize_narrow": 16 <= cw < 256, "resize_tiny": cw < 16,
                            "resize_odd": cw % 2 == 1, "last_column_is_cw_minus_1": math.floor(255 * (cw / 256)) == cw - 1,
                            "resize_clamp_taken": math.floor(255 * (cw / 256)) > cw - 1}.items() if v}
    # augmentation
    if aug is not None:
        a = aug_dict(aug)
        ang, sc, tx, ty, pn = a["angle"], a["scale"], a["tx"], a["ty"], a["pn"]
        rot = R.get_rotation_matrix_2d((128, 128), -180.0 * ang / math.pi, sc)
        rot[0, 2] += tx; rot[1, 2] += ty
        X, _ = R.warp_source_index(rot)
        half = ang == 0.0 and sc == 1.0 and tx % 1.0 == 0.5 and int(X[0, 100]) == 100 - math.floor(tx)      # source x - k - 0.5: a tie, up
        crop = R.imcrop(s["image"], center, size).astype(np.float64)
        pad = any(out.values())
        keys |= {k for k, v in {"aug_angle0_tx_half": half, "aug_angle_half_pi": ang == math.pi / 2, "aug_angle_pi": ang == math.pi,
                                "aug_angle_2pi_minus": ang == TWO_PI_MINUS, "aug_scale08": sc == 0.8, "aug_scale10": sc == 1.0 and ang != 0.0,
                                "aug_t_plus40": tx == 40.0 and ty == 40.0, "aug_t_minus40": tx == -40.0 and ty == -40.0,
                                "aug_colour06": (pn == 0.6).all(), "truncates": bool(((crop * pn) % 1.0 != 0).any()),
                                "aug_colour14": (pn == 1.4).all(), "saturates": bool(((crop * pn) > 255.0).any()),
                                "aug_pad127": pad and (pn != 1.0).all() and not (ang == 0.0 and sc == 1.0)}.items() if v}
    # compute_st: the 2x2 cross-covariance of centred uv and centred pose xy
    _, t = R.getitem(s, aug_dict(aug))
    a_, b_ = t["crop_uv"].reshape(21, 2).astype(np.float64), t["pose3d"].reshape(21, 3)[:, :2].astype(np.float64)
    a_, b_ = a_ - a_.mean(0), b_ - b_.mean(0)
    M = a_.T @ b_ / (np.linalg.norm(a_) * np.linalg.norm(b_))
    det = float(np.linalg.det(M))
    if det < -1e-3:
        keys.add("st_negative_det")
    if abs(det) < 1e-9:
        keys.add("st_collinear")
    return keys


def hits(name, batch=None):
    """full keys ("case" or "case/sub") the designed case reaches, over evaluation mode and (where it defines one) its augmentation"""
    s, aug = build(name)
    nv = None if batch is None else nvmax_of(batch)
    got = census(s, None, nv) | (census(s, aug, nv) if aug is not None else set())
    return {name if k == name else name + "/" + k for k in got}
