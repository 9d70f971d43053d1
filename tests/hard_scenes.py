"""A catalogue of constructed states at the poses the random image tests never reach (a plain helper of tests/test_hard_scenes.py and tests/test_gpu_hard_scenes.py): numpy and
the committed oracle only, no GPU, no RNG.  What is pinned with it is the culling of the frame kernels of gym_lowcostrobot_amd/csrc/lcr_render.hip -- build_prim's records
(screen bounding box, stadium, strip, the full-frame record of a primitive with a corner nearer than 0.02 m to the camera plane), the per-band tile intervals, the mask word, the
rule that the base belongs to the cached background, the staging of partial tile columns.

    catalogue(task, H, W) -> [(name, qpos (nq,), target (3,), claims), ...]       task: "stack" | "pick_place" | "push"

States are rounded to float32 (as tests/test_gpu_image_size._random_poses does) and come back as float64.  Poses are built from the cameras of oracle.render_oracle.camera by
unprojection: the point at axial depth t on the ray of the normalised image position (fx, fy) in [0, 1]^2 is  pos + t (sx X + sy Y - Z),  sx = (fx - 1/2)(W / H) 2 tan(fovy / 2),
sy = -(fy - 1/2) 2 tan(fovy / 2).  So a scene is at the same place of the IMAGE at every frame size (the world pose follows the aspect ratio W / H, and the two scenes that speak
of one pixel follow H as well), and its claims hold at every size.  Cubes "aligned" with a camera have the camera's axes, so their nearest corner lies at centre depth - 0.015.

Families (each for camera_front and camera_top unless the name says otherwise; the name's prefix is the family):
  border   cube centre on the four frame borders and corners; one cube whose projected bounding box ends half a pixel outside the left border; one outside by a cube width
  seam     cube centred on a tile corner of the 240 x 320 frame (column 176, row 100), 47 pixels wide there: 4 tile columns, 12 bands; a cube of 3 pixels inside one tile and
           a cube of less than a pixel (camera_front only, against the sky above the horizon: under camera_top nothing above the floor is further than 0.6 m = 15 pixels)
  near     nearest corner at 0.021 m (finite, large bounds), at 0.019 m (the full-frame record), the camera inside the cube, the cube behind the camera, a tilted cube off to
           the side that straddles the camera plane
  occl     second cube exactly / half behind the first (stack), a cube in front of and behind the base box, between the fingers, half-sunk in the floor (z = -0.010), under it
  marker   (push, pick_place) over the cube, over an arm link, over the base, cut by a border, hidden behind / inside an opaque box, nearer than 0.02 m to a camera, and
           Push's flat marker just above the floor
  arm      each joint at both ends of its range (oracle.orc.model_table()), the arm along +-x and +-y under camera_top (the flat and the zero-slope branch of the stadium), and
           link_3 / link_4 end-on to each camera: build_prim's own `len`, the distance of the means of the four projected corners of the two faces across the box's
           longest edge, is about 1e-5 pixels at every frame size used here, in fp64 and in a float32 emulation alike -- two orders below the 1e-3 of the fallback.  (What
           the kernel itself computes cannot be read back; its fp32 forward kinematics moves a corner by some 1e-7 m, about 1e-4 pixels.)
  wrist    (default mount of tests/wrist_ref.py) a cube a few centimetres in front of the camera, the camera inside the cube, the marker in front of it, a pose whose
           frame is sky and arm only (72 % sky at 36 x 52, 59 % in a square frame; all sky cannot be: the box of the mounting link is fixed in the camera's frame and crosses its near plane, so it covers
           the same pixels at every pose), a pose with the camera below the floor looking up

A claim is a tuple (kind, camera, ...) that check_claims() evaluates on segmentation planes -- the models' or the GPU's -- or, the kinds in GEOMETRIC, on the state alone (they
say that the scene reaches its regime: tests/test_hard_scenes.py checks them, a GPU frame cannot):
  ("none", cam, id)                 no pixel has that id               ("full", cam, id)                 every pixel has it
  ("some", cam, id)                 at least one pixel                 ("frac", cam, id, lo, hi)         share of the frame's pixels within [lo, hi]
  ("area", cam, id, E, lo, hi)      pixel count within [lo E - m, hi E + m], E the pixel count of the cube's uncut near face at this frame size, m = 2 sqrt(E) + 2 for the
                                    pixels along its outline
  ("touches", cam, id, sides)       the id's pixels reach every listed frame border ("l", "r", "t", "b")
  ("one_tile", cam, id)             the id's pixels lie in one 16 x 4 tile         ("long", cam, id, "h" | "v")   the id's pixels span more columns than rows / rows than columns
  ("marker_on", cam, ids)           the marker bit is set on at least one pixel whose id is in ids      ("marker_none", cam)   on no pixel
  ("marker_frac", cam, lo, hi)      share of pixels with the marker bit         ("marker_touches", cam, sides)
  ("corner_depth", cam, box, lo, hi)   GEOMETRIC: the least axial depth of the 8 corners of box `box` (index into oracle.render_oracle.scene's boxes) lies in [lo, hi]
  ("axis_px", cam, box, hi)         GEOMETRIC: build_prim's `len` of the box (kernel_axis_len), in pixels of the frame size in use, is below hi in fp64 and in float32
  ("cam_z", cam, lo, hi)            GEOMETRIC: the camera's height       ("joint", None, j, value)   GEOMETRIC: joint j of the state is float32(value)
Ids are those of tests/planes_ref.py: 0 sky, 1 floor, 2 .. 8 arm boxes, 9 cube, 10 second cube.
"""
import numpy as np

from oracle import orc, render_oracle
from tests import wrist_ref

FRONT, TOP, WRIST = "camera_front", "camera_top", "camera_wrist"
SCENE_CAMS = (FRONT, TOP)
TASKS = ("stack", "pick_place", "push")
GEOMETRIC = ("corner_depth", "axis_px", "cam_z", "joint")
HALF = 0.015                                   # cube half-size
K45 = 2.0 * np.tan(np.radians(45.0) / 2)       # frame height at depth 1 of the scene cameras
ID_FLOOR, ID_BASE, ID_CUBE, ID_CUBE2 = 1, 2, 9, 10
ARM_IDS = tuple(range(3, 9))                   # link_1 .. link_6
Q_HOME = np.zeros(6)                           # the arm upright, forearm along +y at z = 0.17: every constructed cube floats nearer to its camera than the arm is
PARK = (0.3, -0.3, -0.5)                       # where a cube or marker that a scene does not use waits: far under the floor, seen by no camera
D_BORDER = 0.2                                 # axial depth of the border / seam / occlusion cubes (47 pixels wide at 240 rows)

# Found by search, once (scipy's differential evolution over the six joints inside [-3.14, 3.14]^5 x [-2.45, 0.032] on the projected distance of the face centres, then
# Nelder-Mead on kernel_axis_len at 256 rows in fp64, on oracle.orc.link_frames): the arm states that minimise what build_prim calls `len` for the boxes of link_3 and link_4
# (boxes 3 and 4 of oracle.render_oracle.scene) under each scene camera, with every corner more than 0.1 m in front of the camera and the link within 80 pixels of the
# frame's centre -- the links seen end-on.  `len` of the float32 states, fp64 / float32 emulation, in pixels: below 1.1e-5 / 1.2e-5 at 240 and 256 rows, below 5e-6 at 120, 84
# and 36 rows.
END_ON = {
    # (link box, camera): six joint angles
    (3, "camera_front"): (0.09538363665342331, 2.186976194381714, -1.3036068677902222, 1.156045913696289, -0.8408671617507935, -2.194908857345581),
    (3, "camera_top"): (-0.00044642857392318547, -2.784914493560791, 2.0667669773101807, 0.6345236301422119, 1.6310582160949707, -0.04444938898086548),
    (4, "camera_front"): (-3.03952956199646, -3.025372266769409, 1.699397325515747, -1.8928565979003906, -1.4364886283874512, -0.7364428043365479),
    (4, "camera_top"): (-0.029915176331996918, 2.2201974391937256, 2.3832039833068848, -1.5821582078933716, 2.8470277786254883, -2.415311574935913),
}

# Found by search, once (3 000 states of numpy's default_rng(0) inside the joint ranges, fp64 reference of the wrist camera at 36 x 52): among the states whose wrist frame shows
# no floor pixel the one with the most sky (72 %; the rest is link_4, the mounting link_5 and link_6), and the first whose wrist camera lies more than 2 cm under the floor
# and looks upwards (its -Z has a positive world z).
Q_WRIST_SKY = (-0.7428449988365173, -0.6280933022499084, -2.7897627353668213, -1.2347339391708374, 2.5228872299194336, -0.0030391740147024393)
Q_WRIST_UNDER_FLOOR = (-1.8870429992675781, 2.776470422744751, -0.8471081256866455, -2.477489709854126, 0.8107991814613342, -0.14880239963531494)


def _unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def mat2quat(R):
    """(w, x, y, z) of a rotation matrix (columns = the body's axes), by the largest-diagonal branch"""
    R = np.asarray(R, float)
    t = np.trace(R)
    if t > 0:
        s = 2.0 * np.sqrt(1.0 + t); q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R))); j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s; q[1 + i] = 0.25 * s; q[1 + j] = (R[j, i] + R[i, j]) / s; q[1 + k] = (R[k, i] + R[i, k]) / s
    return _unit(q)


def rot(axis, angle):
    """rotation matrix about a unit axis (Rodrigues)"""
    k = _unit(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def camera_of(task, cam, qpos=None):
    """(pos, X, Y, Z, fovy in degrees) of a scene camera, or of the default wrist mount for the arm pose qpos[:6]"""
    if cam == WRIST:
        m = wrist_ref.default_mount()
        return wrist_ref.camera(m, qpos) + (m["fovy_deg"],)
    return render_oracle.camera(task, cam) + (45.0,)


def unproject(camera, fx, fy, t, aspect):
    """the point at axial depth t on the ray of the normalised image position (fx, fy)"""
    pos, X, Y, Z, fovy = camera
    k = 2.0 * np.tan(np.radians(fovy) / 2)
    return pos + t * ((fx - 0.5) * aspect * k * X - (fy - 0.5) * k * Y - Z)


def face_px(t, H, fovy=45.0):
    """pixel count of the uncut near face (axial depth t - 0.015) of a camera-aligned cube centred at depth t"""
    return (2 * HALF / ((t - HALF) * 2.0 * np.tan(np.radians(fovy) / 2) / H)) ** 2


def _state(task, arm=Q_HOME, cube=PARK, cube_R=None, cube2=PARK, cube2_R=None, target=PARK):
    nq = 20 if task == "stack" else 13
    q = np.zeros(nq)
    q[:6] = arm
    q[6:9] = cube; q[9:13] = mat2quat(np.eye(3) if cube_R is None else cube_R)
    if task == "stack":
        q[13:16] = cube2; q[16:20] = mat2quat(np.eye(3) if cube2_R is None else cube2_R)
    return q.astype(np.float32).astype(np.float64), np.asarray(target, np.float32).astype(np.float64)


def _axes(camera):
    return np.stack(camera[1:4], 1)     # columns X, Y, Z: a cube with the camera's axes


def catalogue(task, H=240, W=320):
    """the named scenes of a task for frames of H x W"""
    assert task in TASKS, task
    asp = W / H
    has_marker = task in ("push", "pick_place")
    out = []

    def add(name, claims, **kw):
        q, t = _state(task, **kw)
        out.append((name, q, t, [tuple(c) for c in claims]))

    for cam in SCENE_CAMS:
        C = camera_of(task, cam)
        R = _axes(C)
        c = cam.split("_")[1]
        E = face_px(D_BORDER, H)
        s = K45 / H
        # ---- border
        for tag, fx, fy, sides, lo, hi in (("left", 0.0, 0.5, "l", 0.35, 0.75), ("right", 1.0, 0.5, "r", 0.35, 0.75), ("top", 0.5, 0.0, "t", 0.35, 0.75),
                                           ("bottom", 0.5, 1.0, "b", 0.35, 0.75), ("top_left", 0.0, 0.0, "tl", 0.15, 0.45), ("top_right", 1.0, 0.0, "tr", 0.15, 0.45),
                                           ("bottom_left", 0.0, 1.0, "bl", 0.15, 0.45), ("bottom_right", 1.0, 1.0, "br", 0.15, 0.45)):
            add(f"border_{tag}_{c}", [("touches", cam, ID_CUBE, sides), ("area", cam, ID_CUBE, E, lo, hi)], cube=unproject(C, fx, fy, D_BORDER, asp), cube_R=R)
        # left of the frame, the right edge of its far face (depth D + 0.015: of the cube's right side it projects nearest to the frame) half a pixel outside the border: the
        # bounding box ends at x1 = -1 in pixel-centre units
        xc = (-0.5 - 0.5 * W) * s * (D_BORDER + HALF) - HALF
        add(f"border_just_outside_{c}", [("none", cam, ID_CUBE)], cube=C[0] + xc * C[1] - D_BORDER * C[3], cube_R=R)
        xc = -0.5 * W * s * (D_BORDER + HALF) - HALF - 2 * HALF
        add(f"border_far_outside_{c}", [("none", cam, ID_CUBE)], cube=C[0] + xc * C[1] - D_BORDER * C[3], cube_R=R)
        # ---- seams and sizes
        add(f"seam_tile_corner_{c}", [("area", cam, ID_CUBE, E, 0.9, 1.4)], cube=unproject(C, 176 / 320, 100 / 240, D_BORDER, asp), cube_R=R)
        if cam == FRONT:   # rows 8 .. 11 of 240 look above the horizon: sky behind the far cubes
            far = [("area", cam, ID_CUBE, face_px(2.9, H), 0.5, 1.6)] + ([("one_tile", cam, ID_CUBE), ("some", cam, ID_CUBE)] if (H, W) == (240, 320) else [])
            add(f"seam_few_pixels_{c}", far, cube=unproject(C, 168.5 / 320, 10.0 / 240, 2.9, asp), cube_R=R)
            add(f"seam_sub_pixel_{c}", [("frac", cam, ID_CUBE, 0.0, 1.5 / (H * W))], cube=unproject(C, 168.5 / 320, 10.0 / 240, 20.0, asp), cube_R=R)
        # ---- near plane
        fills = asp * np.tan(np.radians(22.5)) < HALF / 0.021 - 0.02    # the near face at 0.021 m spans |sx| < 0.714: wider frames see past it
        near_full = ("full", cam, ID_CUBE) if fills else ("frac", cam, ID_CUBE, 0.6, 1.0)
        add(f"near_021_{c}", [near_full, ("corner_depth", cam, 7, 0.0205, 0.0215)], cube=unproject(C, 0.5, 0.5, 0.021 + HALF, asp), cube_R=R)
        add(f"near_019_{c}", [near_full, ("corner_depth", cam, 7, 0.0185, 0.0195)], cube=unproject(C, 0.5, 0.5, 0.019 + HALF, asp), cube_R=R)
        add(f"near_inside_{c}", [("none", cam, ID_CUBE), ("corner_depth", cam, 7, -0.006, -0.004)], cube=unproject(C, 0.5, 0.5, 0.010, asp), cube_R=R)
        add(f"near_behind_{c}", [("none", cam, ID_CUBE), ("corner_depth", cam, 7, -0.066, -0.064)], cube=unproject(C, 0.5, 0.5, -0.050, asp), cube_R=R)
        # tilted, up and to the right of the axis, centre 0.03 m in front of the camera plane: its far corners reach into the frame's top right corner
        Rt = R @ rot([0, 1, 0], 0.6) @ rot([1, 0, 0], 0.4)
        add(f"near_straddle_{c}", [("touches", cam, ID_CUBE, "tr"), ("frac", cam, ID_CUBE, 0.002, 0.45), ("corner_depth", cam, 7, -0.02, 0.019)],
            cube=C[0] + 0.030 * C[1] + 0.024 * C[2] - 0.030 * C[3], cube_R=Rt)
        # ---- occlusion
        if task == "stack":
            p1 = unproject(C, 0.4, 0.4, D_BORDER, asp)
            E2 = face_px(D_BORDER + 0.06, H)
            add(f"occl_stack_behind_{c}", [("none", cam, ID_CUBE2), ("area", cam, ID_CUBE, E, 0.9, 1.4)], cube=p1, cube_R=R, cube2=unproject(C, 0.4, 0.4, D_BORDER + 0.06, asp),
                cube2_R=R)
            add(f"occl_stack_half_behind_{c}", [("area", cam, ID_CUBE2, E2, 0.2, 0.8), ("area", cam, ID_CUBE, E, 0.9, 1.4)], cube=p1, cube_R=R,
                cube2=unproject(C, 0.4, 0.4, D_BORDER + 0.06, asp) + HALF * (D_BORDER + 0.06) / D_BORDER * C[1], cube2_R=R)
    # the base box: centre (0.0118, -0.04, 0.0204), half (0.0409, 0.0801, 0.0213) along (y, -x, z) -- x in [-0.068, 0.092], y in [-0.081, 0.001], z in [-0.001, 0.042]
    base_c = np.array([0.0118, -0.04, 0.0204])
    CF, CT = camera_of(task, FRONT), camera_of(task, TOP)
    ray = _unit(base_c - CF[0])
    dist = np.linalg.norm(base_c - CF[0])
    add("occl_before_base_front", [("some", FRONT, ID_CUBE), ("area", FRONT, ID_CUBE, face_px((dist - 0.12) * -(ray @ CF[3]), H), 0.8, 2.2)], cube=CF[0] + (dist - 0.12) * ray,
        cube_R=_axes(CF))
    # behind the base as camera_front sees it, on the floor: only the arm's base (and link_1 above it) is in front of it
    add("occl_behind_base_front", [("none", FRONT, ID_CUBE), ("some", FRONT, ID_BASE)], cube=(0.012, -0.10, 0.015))
    # under camera_top: above the arm over the base (in front of everything), and inside the base box with one side sticking out of it
    add("occl_above_base_top", [("area", TOP, ID_CUBE, face_px(0.6 - 0.2, H), 0.9, 1.4)], cube=(0.012, -0.04, 0.2))
    add("occl_in_base_top", [("area", TOP, ID_CUBE, face_px(0.6 - 0.015, H), 0.2, 0.8), ("some", TOP, ID_BASE)], cube=(0.092, -0.06, 0.015))
    site = orc.fk(Q_HOME)[1]
    add("occl_between_fingers", [("some", TOP, ID_CUBE), ("frac", TOP, ID_CUBE, 0.0, 0.9 * face_px(0.6 - site[2], H) / (H * W))], cube=site)
    add("occl_half_sunk", [("area", TOP, ID_CUBE, face_px(0.6 + 0.010, H), 0.8, 1.3), ("some", FRONT, ID_CUBE)], cube=(0.1, 0.15, -0.010))
    add("occl_under_floor", [("none", TOP, ID_CUBE), ("none", FRONT, ID_CUBE)], cube=(0.1, 0.15, -0.05))
    # ---- marker
    if has_marker:
        add("marker_over_cube", [("marker_on", TOP, (ID_CUBE,)), ("marker_on", FRONT, (ID_CUBE,))], cube=(0.1, 0.15, 0.015), target=(0.1, 0.16, 0.05))
        add("marker_over_link", [("marker_on", TOP, ARM_IDS)], target=(0.0, 0.12, 0.22))            # above link_4 of the home pose
        add("marker_over_base_front", [("marker_on", FRONT, (ID_BASE,))], target=CF[0] + (dist - 0.15) * ray)
        for cam, C in ((FRONT, CF), (TOP, CT)):
            c = cam.split("_")[1]
            add(f"marker_cut_left_{c}", [("marker_touches", cam, "l"), ("marker_frac", cam, 0.001, 0.2)], target=unproject(C, 0.0, 0.5, D_BORDER, asp))
            near = 0.028 if cam == TOP else 0.035
            add(f"marker_near_{c}", [("marker_frac", cam, 0.3, 1.0), ("corner_depth", cam, 8, -0.03, 0.0199)], target=unproject(C, 0.5, 0.5, near, asp))
        # hidden: inside the base box (Push's flat marker is wider than a cube, the base is wider than the marker)
        add("marker_inside_base", [("marker_none", TOP), ("marker_none", FRONT)], target=(0.012, -0.04, 0.02))
        if task == "pick_place":   # ... and exactly behind the cube along a ray of each camera, a cube-sized marker
            for cam, C in ((FRONT, CF), (TOP, CT)):
                add(f"marker_behind_cube_{cam.split('_')[1]}", [("marker_none", cam), ("some", cam, ID_CUBE)], cube=unproject(C, 0.6, 0.4, D_BORDER, asp), cube_R=_axes(C),
                    target=unproject(C, 0.6, 0.4, D_BORDER + 0.05, asp))
        if task == "push":
            add("marker_flat_on_floor", [("marker_on", TOP, (ID_FLOOR,)), ("marker_on", FRONT, (ID_FLOOR,))], target=(0.1, 0.15, 0.011))
    # ---- arm
    ranges = [tuple(l["range"]) for l in orc.model_table()["links"]]
    for j, (lo, hi) in enumerate(ranges):
        for tag, v in (("lo", lo), ("hi", hi)):
            q = Q_HOME.copy(); q[j] = v
            add(f"arm_joint{j + 1}_{tag}", [("joint", None, j, v), ("some", TOP, ID_BASE)], arm=q, cube=(0.1, 0.15, 0.015))
    for tag, q0, d in (("py", 0.0, "v"), ("px", -np.pi / 2, "h"), ("ny", np.pi, "v"), ("nx", np.pi / 2, "h")):
        q = Q_HOME.copy(); q[0] = q0
        add(f"arm_along_{tag}_top", [("long", TOP, 5, d)], arm=q, cube=(0.1, 0.15, 0.015))      # id 5 = link_3, the forearm
    for (box, cam), q in END_ON.items():
        add(f"arm_end_on_link{box}_{cam.split('_')[1]}", [("axis_px", cam, box, 1e-4)], arm=np.asarray(q), cube=(0.1, 0.15, 0.015))
    # ---- wrist
    CW = camera_of(task, WRIST, Q_HOME)
    RW = _axes(CW)
    add("wrist_cube_in_front", [("some", WRIST, ID_CUBE), ("frac", WRIST, ID_CUBE, 0.05, 0.9)], cube=CW[0] - 0.06 * CW[3], cube_R=RW)
    add("wrist_near_019", [("frac", WRIST, ID_CUBE, 0.5, 1.0), ("corner_depth", WRIST, 7, 0.0185, 0.0195)], cube=CW[0] - (0.019 + HALF) * CW[3], cube_R=RW)
    add("wrist_inside_cube", [("none", WRIST, ID_CUBE), ("corner_depth", WRIST, 7, -0.012, -0.008)], cube=CW[0] - 0.005 * CW[3], cube_R=RW)
    if has_marker:
        add("wrist_marker_in_front", [("marker_frac", WRIST, 0.02, 1.0)], target=CW[0] - 0.06 * CW[3])
    # id 7 = link_5, the mounting link: in view at every pose
    add("wrist_sky", [("none", WRIST, ID_FLOOR), ("frac", WRIST, 0, 0.5, 1.0), ("some", WRIST, 7)], arm=np.asarray(Q_WRIST_SKY))
    add("wrist_under_floor", [("none", WRIST, ID_FLOOR), ("cam_z", WRIST, -1.0, -0.02)], arm=np.asarray(Q_WRIST_UNDER_FLOOR))
    assert len({s_[0] for s_ in out}) == len(out)
    return out


def kernel_axis_len(task, cam, qpos, target, box, H, dtype=np.float64):
    """what build_prim (gym_lowcostrobot_amd/csrc/lcr_render.hip) calls `len` for an arm box, restated: the 8 corners are projected to pixels (a depth below 0.02 m counts as
    0.02), the four of each face across the box's longest edge are averaged, and `len` is the distance of the two means -- under perspective not the distance of the projected
    face centres.  Below 1e-3 the kernel gives up the direction and takes the image's x axis.  `dtype` = np.float32 runs this arithmetic in float32 on the fp64 scene"""
    dt = np.dtype(dtype).type
    pos, X, Y, Z, fovy = camera_of(task, cam, qpos)
    pos, X, Y, Z = (np.asarray(a, dtype) for a in (pos, X, Y, Z))
    bc, R, bh = (np.asarray(a, dtype) for a in render_oracle.scene(task, qpos, target)[1][box][:3])
    ax = (0 if bh[0] >= bh[2] else 2) if bh[0] >= bh[1] else (1 if bh[1] >= bh[2] else 2)
    s = dt(2.0 * np.tan(np.radians(fovy) / 2) / H)
    mean = np.zeros((2, 2), dtype)
    for i in range(8):
        e = bc + R @ (bh * np.array([1 if i & 1 else -1, 1 if i & 2 else -1, 1 if i & 4 else -1], dtype)) - pos
        inv = dt(1.0) / (max(-(e @ Z), dt(0.02)) * s)
        mean[1 if i & (1 << ax) else 0] += dt(0.25) * np.array([(e @ X) * inv, -(e @ Y) * inv], dtype)
    d = mean[1] - mean[0]
    assert d.dtype == np.dtype(dtype)
    return float(np.sqrt(d[0] * d[0] + d[1] * d[1]))


def _mask_sides(mask, sides):
    edge = {"l": mask[:, 0], "r": mask[:, -1], "t": mask[0, :], "b": mask[-1, :]}
    return [sd for sd in sides if not edge[sd].any()]


def check_claims(task, scene, planes_of, H, W, geometric=True):
    """evaluate the claims of one scene.  planes_of(cam) -> the (H, W) uint8 segmentation plane of that camera, or None when this build does not draw that camera (its claims
    are then skipped).  Returns the list of claims that do not hold, each with what was found"""
    name, qpos, target, claims = scene
    bad = []
    for cl in claims:
        kind, cam = cl[0], cl[1]
        if kind in GEOMETRIC:
            if not geometric:
                continue
            if kind == "joint":
                v = qpos[cl[2]]
                if v != np.float32(cl[3]):
                    bad.append((name, cl, v))
                continue
            if kind == "axis_px":
                v = (kernel_axis_len(task, cam, qpos, target, cl[2], H), kernel_axis_len(task, cam, qpos, target, cl[2], H, np.float32))
                if not max(v) < cl[3]:
                    bad.append((name, cl, v))
                continue
            C = camera_of(task, cam, qpos)
            if kind == "cam_z":
                v = C[0][2]
                ok = cl[2] <= v <= cl[3]
            else:
                bc, R, bh = render_oracle.scene(task, qpos, target)[1][cl[2]][:3]
                corners = [bc + R @ (bh * np.array([sx, sy, sz])) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
                v = min(float(-(p - C[0]) @ C[3]) for p in corners)
                ok = cl[3] <= v <= cl[4]
            if not ok:
                bad.append((name, cl, v))
            continue
        seg = planes_of(cam)
        if seg is None:
            continue
        assert seg.shape == (H, W), (seg.shape, H, W)
        ids, mk = seg & 0x7F, (seg & 0x80) != 0
        if kind == "none":
            v = int((ids == cl[2]).sum()); ok = v == 0
        elif kind == "full":
            v = int((ids == cl[2]).sum()); ok = v == H * W
        elif kind == "some":
            v = int((ids == cl[2]).sum()); ok = v > 0
        elif kind == "frac":
            v = float((ids == cl[2]).mean()); ok = cl[3] <= v <= cl[4]
        elif kind == "area":
            E = cl[3]; m = 2.0 * np.sqrt(E) + 2.0
            v = int((ids == cl[2]).sum()); ok = cl[4] * E - m <= v <= cl[5] * E + m
        elif kind == "touches":
            v = _mask_sides(ids == cl[2], cl[3]); ok = not v
        elif kind == "one_tile":
            r, p = np.nonzero(ids == cl[2])
            v = sorted({(int(a) // 4, int(b) // 16) for a, b in zip(r, p)}); ok = len(v) <= 1
        elif kind == "long":
            r, p = np.nonzero(ids == cl[2])
            v = (int(np.ptp(r)) + 1, int(np.ptp(p)) + 1) if r.size else (0, 0)
            ok = r.size > 0 and (v[1] > v[0] if cl[3] == "h" else v[0] > v[1])
        elif kind == "marker_on":
            v = int((mk & np.isin(ids, cl[2])).sum()); ok = v > 0
        elif kind == "marker_none":
            v = int(mk.sum()); ok = v == 0
        elif kind == "marker_frac":
            v = float(mk.mean()); ok = cl[2] <= v <= cl[3]
        elif kind == "marker_touches":
            v = _mask_sides(mk, cl[2]); ok = not v
        else:
            raise ValueError(kind)
        if not ok:
            bad.append((name, cl, v))
    return bad


COLOUR_KINDS = ("none", "full", "some", "frac", "area", "touches", "one_tile")


def seg_from_rgb(rgb):
    """what a colour frame says about the cubes: id 9 where the pixel is pure red, 10 where it is pure blue (tests/planes_ref.rgb_class), 0 elsewhere.  A cube pixel under the
    translucent marker is neither, so only the claims of colour_claims() may be read off it"""
    from tests import planes_ref
    cls = planes_ref.rgb_class(rgb)
    return np.where(cls == 2, ID_CUBE, np.where(cls == 3, ID_CUBE2, 0)).astype(np.uint8)


def colour_claims(scene):
    """the scene with only those claims that a colour frame can decide: counts and places of the cubes' pixels, in scenes whose marker is parked or claimed hidden"""
    name, qpos, target, claims = scene
    marker_shows = any(c[0] in ("marker_on", "marker_frac", "marker_touches") for c in claims)
    keep = [c for c in claims if c[0] in COLOUR_KINDS and c[2] in (ID_CUBE, ID_CUBE2) and not marker_shows]
    return name, qpos, target, keep
