"""ctypes binding of libmod_sf.so (include/mod_sf.h).

The library is the product; there is no CPU fallback.  Loading fails loudly when the shared object has not been
built (``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C moving_object_detector_amd/csrc``).

torch is imported *before* the library on purpose: PyTorch-ROCm bundles its own ``libamdhip64.so`` (same soname as the
system one), and the dynamic loader then resolves our library's HIP dependency to that already-loaded runtime, so device
pointers and streams owned by torch are valid inside our kernels (one HIP runtime per process).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MOD_SF_LIB") or os.path.join(_HERE, "libmod_sf.so")   # MOD_SF_LIB: A/B builds during development

MOD_OK = 0
MOD_SKIP_NO_DISPARITY_NOW = 1
MOD_SKIP_NO_DISPARITY_PREV = 2
MOD_SKIP_NO_FLOW = 3
MOD_SKIP_NO_TRANSFORM = 4
MOD_ERR_INVALID_ARGUMENT = -1
MOD_ERR_NOT_CONFIGURED = -2
MOD_ERR_CAPACITY = -3
MOD_ERR_DEVICE = -4
MOD_ERR_NO_DEVICE = -5
MOD_STAGE_SCENE_FLOW, MOD_STAGE_CCL_TILE, MOD_STAGE_CCL_LINK, MOD_STAGE_CCL_MERGE = 0, 1, 2, 3
MOD_STAGE_FINAL, MOD_STAGE_MEDIAN, MOD_STAGE_CLUSTER_GROUP, MOD_STAGE_COUNT = 4, 5, 6, 7
MOD_PROFILE_ALL = 0x7F
MOD_PER_KERNEL_CLUSTER_STAGES = (1, 2, 3, 4, 5)
MOD_PIPELINE_DEPTH = 3
MOD_EGO_OK, MOD_EGO_FEW_POINTS, MOD_EGO_FEW_INLIERS, MOD_EGO_DIVERGED = 0, 1, 2, 3
MOD_EGO_MAX_HYPOTHESES = 4096
MOD_SGM_FRACTION_BITS = 4
MOD_FLOW_SEEDS = 5
MOD_TEXTURE_DISPARITY, MOD_TEXTURE_FLOW = 1, 2           # ModTextureFilter.apply: the estimators the texture threshold rejects in
MOD_DISPARITY_FILL_MIN, MOD_DISPARITY_FILL_SECOND, MOD_DISPARITY_FILL_MEDIAN = 0, 1, 2   # ModDisparityFill.mode: the rank taken of the found words
MOD_TEXTURE_MAX = 15 * 15 * 255                          # the largest texture sum (window 15, cap 255): it fits a uint16
MOD_CORNER_MAX = 15 * 15 * 255 * 255                     # 14630625: the largest min-eigenvalue (ModCornerFilter.threshold's upper end)
MOD_EYE_LEFT, MOD_EYE_RIGHT = 0, 1
MOD_DISTORTION_RATIONAL, MOD_DISTORTION_EQUIDISTANT = 0, 1   # how ModRectifyCamera.D is read (mod_set_distortion_model)
DISTORTION_MODELS = {"plumb_bob": MOD_DISTORTION_RATIONAL, "rational_polynomial": MOD_DISTORTION_RATIONAL,
                     "equidistant": MOD_DISTORTION_EQUIDISTANT}   # sensor_msgs/CameraInfo.distortion_model
MOD_MAX_WIDTH = 16384
MOD_BIN_MEAN, MOD_BIN_NEAREST = 0, 1                     # mod_set_image_binning: rounded box mean / the block's top-left pixel
BIN_MODES = {"mean": MOD_BIN_MEAN, "nearest": MOD_BIN_NEAREST}
MOD_DEPTH_16UC1, MOD_DEPTH_32FC1 = 0, 1                  # REP 118 depth images: uint16 millimetres / float32 metres
MOD_DEPTH_SPLAT_MAX = 8                                  # targets per axis a footprint of mod_set_depth_splat may paint
MOD_DEPTH_RAYS_CENTRES, MOD_DEPTH_RAYS_CORNERS = 0, 1    # mod_depth_rays_host: the ray table of the pixel centres / of the pixel corners
MOD_DEPTH_UNDISTORT_ITERS = 20                           # fixed-point iterations behind every ray of mod_set_depth_distortion
# mod_set_depth_decimation: the block's lower median / nearest / gated mean around the median / top-left word
MOD_DEPTH_DECIMATE_MEDIAN, MOD_DEPTH_DECIMATE_MIN, MOD_DEPTH_DECIMATE_MEAN, MOD_DEPTH_DECIMATE_NEAREST = 0, 1, 2, 3
DEPTH_DECIMATE_MODES = {"median": MOD_DEPTH_DECIMATE_MEDIAN, "min": MOD_DEPTH_DECIMATE_MIN, "mean": MOD_DEPTH_DECIMATE_MEAN,
                        "nearest": MOD_DEPTH_DECIMATE_NEAREST}
DEPTH_ENCODINGS = {"16UC1": MOD_DEPTH_16UC1, "32FC1": MOD_DEPTH_32FC1}
DEPTH_BYTES = {MOD_DEPTH_16UC1: 2, MOD_DEPTH_32FC1: 4}   # bytes per sample
MOD_ENCODING_MONO8, MOD_ENCODING_BGR8, MOD_ENCODING_RGB8, MOD_ENCODING_BGRA8, MOD_ENCODING_RGBA8 = 0, 1, 2, 3, 4
MOD_ENCODING_YUV422, MOD_ENCODING_YUV422_YUY2 = 5, 6   # packed 4:2:2: UYVY, YUYV (grey = Y)
ENCODINGS = {"mono8": MOD_ENCODING_MONO8, "bgr8": MOD_ENCODING_BGR8, "rgb8": MOD_ENCODING_RGB8, "bgra8": MOD_ENCODING_BGRA8,
             "rgba8": MOD_ENCODING_RGBA8, "yuv422": MOD_ENCODING_YUV422, "yuv422_yuy2": MOD_ENCODING_YUV422_YUY2}
# 8-bit Bayer mosaics, demosaiced straight to grey on the GPU (one byte per pixel; width, height >= 3)
MOD_ENCODING_BAYER_RGGB8, MOD_ENCODING_BAYER_BGGR8, MOD_ENCODING_BAYER_GBRG8, MOD_ENCODING_BAYER_GRBG8 = 16, 17, 18, 19
BAYER_ENCODINGS = {"bayer_rggb8": MOD_ENCODING_BAYER_RGGB8, "bayer_bggr8": MOD_ENCODING_BAYER_BGGR8,
                   "bayer_gbrg8": MOD_ENCODING_BAYER_GBRG8, "bayer_grbg8": MOD_ENCODING_BAYER_GRBG8}
BAYER_CHANNELS = {e: 1 for e in BAYER_ENCODINGS.values()}    # bytes per pixel (a dict of its own: CHANNELS' keys are ENCODINGS' values)
# bytes per pixel
CHANNELS = {MOD_ENCODING_MONO8: 1, MOD_ENCODING_BGR8: 3, MOD_ENCODING_RGB8: 3, MOD_ENCODING_BGRA8: 4, MOD_ENCODING_RGBA8: 4,
            MOD_ENCODING_YUV422: 2, MOD_ENCODING_YUV422_YUY2: 2}
STAGE_NAMES = ("k_scene_flow", "k_ccl_bits+k_ccl_tile_list", "k_ccl_link", "k_ccl_merge", "k_final", "k_median+k_median_ties",
               "cluster group (first launch to last)")

class ModConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_width", C.c_int32), ("max_height", C.c_int32), ("max_frames", C.c_int32),
                ("max_objects", C.c_int32), ("batch_chunks", C.c_int32), ("stream", C.c_void_p)]


class ModCamera(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("Tx", C.c_double), ("Ty", C.c_double), ("disp_f", C.c_float), ("disp_T", C.c_float),
                ("min_disparity", C.c_float), ("max_disparity", C.c_float)]


class ModParams(C.Structure):
    _fields_ = [("dynamic_flow_diff", C.c_int32), ("cluster_size", C.c_int32), ("neighbor_distance", C.c_int32),
                ("reserved", C.c_int32), ("depth_diff", C.c_double), ("dynamic_speed", C.c_double)]


class ModTransform(C.Structure):
    _fields_ = [("t", C.c_double * 3), ("q", C.c_double * 4)]


class ModObject(C.Structure):
    _fields_ = [("id", C.c_int32), ("n_points", C.c_int32), ("center", C.c_double * 3), ("orientation", C.c_double * 4),
                ("velocity", C.c_double * 3), ("bounding_box", C.c_double * 3)]


class ModFrameBatch(C.Structure):
    _fields_ = [("frames", C.c_int32), ("reserved", C.c_int32), ("disparity_now", C.c_void_p), ("disparity_prev", C.c_void_p),
                ("flow", C.c_void_p), ("transforms", C.POINTER(ModTransform)), ("dt", C.POINTER(C.c_double))]


class ModSceneFlowPlanes(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("vx", C.c_void_p), ("vy", C.c_void_p),
                ("vz", C.c_void_p), ("dynamic_mask", C.c_void_p), ("cloud_aos", C.c_void_p), ("depth", C.c_void_p),
                ("static_flow", C.c_void_p)]


class ModSgmParams(C.Structure):
    _fields_ = [("disparities", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("paths", C.c_int32), ("lr_check", C.c_int32),
                ("median", C.c_int32)]


class ModDisparityFilters(C.Structure):
    _fields_ = [("uniqueness_ratio", C.c_int32), ("speckle_size", C.c_int32), ("speckle_range", C.c_int32), ("reserved", C.c_int32)]


class ModDisparityFill(C.Structure):
    _fields_ = [("reach", C.c_int32), ("directions", C.c_int32), ("mode", C.c_int32), ("min_found", C.c_int32)]


_DISPARITY_FILL_MODES = {"min": MOD_DISPARITY_FILL_MIN, "second": MOD_DISPARITY_FILL_SECOND, "median": MOD_DISPARITY_FILL_MEDIAN}


def disparity_fill(reach: int, directions: int = 8, mode="min", min_found: int = 1) -> ModDisparityFill:
    """ModDisparityFill of include/mod_sf.h (reach 0 = off): an invalid disparity walks the first `directions` (2, 4 or 8) of the path
    directions for up to `reach` (0..256) steps each to the first valid word, and where at least `min_found` (1..directions) of them find
    one it becomes the lowest ("min", the background), the second lowest ("second") or the lower median ("median") of the found words;
    every other pixel stays.  `mode` is one of the three names or MOD_DISPARITY_FILL_*.  Raises ValueError where the library would
    refuse the value.  These defaults are placeholders, not tuned on any scene."""
    if isinstance(mode, str):
        if mode not in _DISPARITY_FILL_MODES:
            raise ValueError(f"disparity fill mode must be one of {sorted(_DISPARITY_FILL_MODES)}, not {mode!r}")
        mode = _DISPARITY_FILL_MODES[mode]
    reach, directions, mode, min_found = int(reach), int(directions), int(mode), int(min_found)
    if not 0 <= reach <= 256:
        raise ValueError("disparity fill reach must be in 0..256")
    if directions not in (2, 4, 8):
        raise ValueError("disparity fill directions must be 2, 4 or 8")
    if mode not in _DISPARITY_FILL_MODES.values():
        raise ValueError("disparity fill mode must be MOD_DISPARITY_FILL_MIN, _SECOND or _MEDIAN")
    if not 1 <= min_found <= directions:
        raise ValueError("disparity fill min_found must be in 1..directions")
    return ModDisparityFill(reach, directions, mode, min_found)


class ModDisparitySmooth(C.Structure):
    _fields_ = [("window", C.c_int32), ("min_members", C.c_int32), ("tol", C.c_float), ("reserved", C.c_int32)]


def disparity_smooth(window: int = 5, tol: float = 1.0, min_members: int = 1) -> ModDisparitySmooth:
    """ModDisparitySmooth of include/mod_sf.h: a valid disparity d becomes the mean, summed in row-major order, of the valid disparities
    of its `window` x `window` square (3, 5 or 7) that lie within `tol` px (finite, >= 0) of d, where at least `min_members`
    (1..window^2) do, itself included; every other pixel stays.  Raises ValueError where the library would refuse the value.  These
    defaults are placeholders, not tuned on camera data."""
    window, min_members, tol = int(window), int(min_members), float(tol)
    if window not in (3, 5, 7):
        raise ValueError("disparity smooth window must be 3, 5 or 7")
    if not 0.0 <= tol <= 3.4028234663852886e38:          # NaN fails both comparisons; the upper end is FLT_MAX
        raise ValueError("disparity smooth tol must be finite and >= 0")
    if not 1 <= min_members <= window * window:
        raise ValueError("disparity smooth min_members must be in 1..window^2")
    return ModDisparitySmooth(window, min_members, tol, 0)


class ModTextureFilter(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("window", C.c_int32), ("cap", C.c_int32), ("apply", C.c_int32)]


def texture_filter(threshold: int = 0, window: int = 9, cap: int = 31, apply: int = MOD_TEXTURE_DISPARITY | MOD_TEXTURE_FLOW) -> ModTextureFilter:
    """ModTextureFilter with the defaults of include/mod_sf.h (threshold 0 = off): T = the window x window sum of the horizontal central
    differences capped at `cap`; pixels with T < threshold are rejected in the estimators named by `apply`."""
    return ModTextureFilter(int(threshold), int(window), int(cap), int(apply))


class ModCornerFilter(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("window", C.c_int32), ("cap", C.c_int32), ("reserved", C.c_int32)]


def corner_filter(threshold: int = 0, window: int = 9, cap: int = 31) -> ModCornerFilter:
    """ModCornerFilter with the defaults of include/mod_sf.h (threshold 0 = off): E = the floor of the smaller eigenvalue of the window x
    window gradient structure tensor, gradients capped at +-`cap`; flow pixels with E < threshold are rejected."""
    return ModCornerFilter(int(threshold), int(window), int(cap), 0)


class ModFlowMedian(C.Structure):
    _fields_ = [("window", C.c_int32), ("min_valid", C.c_int32), ("reserved", C.c_int32 * 2)]


def flow_median(window: int = 5, min_valid: int = 0) -> ModFlowMedian:
    """ModFlowMedian of include/mod_sf.h (window 0 = off, 3 or 5): every valid flow pixel becomes the per-component lower median of the
    valid pixels of its window x window square, or (NaN, NaN) where fewer than `min_valid` of them are valid; invalid pixels stay."""
    return ModFlowMedian(int(window), int(min_valid), (0, 0))


class ModFlowFill(C.Structure):
    _fields_ = [("window", C.c_int32), ("min_valid", C.c_int32), ("tol_abs", C.c_float), ("tol_rel", C.c_float), ("reserved", C.c_int32 * 2)]


def flow_fill(window: int = 5, min_valid: int = 3, tol_abs: float = 1.0, tol_rel: float = 0.0) -> ModFlowFill:
    """ModFlowFill of include/mod_sf.h (window 0 = off, 3, 5 or 7): an invalid flow pixel with a valid disparity d becomes the
    per-component lower median of the valid flow pixels of its window x window square whose disparity lies within tol_abs + tol_rel * d
    of d, where at least `min_valid` of them do; every other pixel stays.  These defaults are placeholders, not tuned on any scene."""
    return ModFlowFill(int(window), int(min_valid), float(tol_abs), float(tol_rel), (0, 0))


class ModFlowParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("radius", C.c_int32), ("window", C.c_int32), ("subpixel", C.c_int32), ("fb_check", C.c_int32)]


def flow_params(levels: int = 4, radius: int = 4, window: int = 5, subpixel: bool = True, fb_check: int = 1) -> ModFlowParams:
    """ModFlowParams with the defaults of include/mod_sf.h (fb_check < 0 turns the forward-backward check off)."""
    return ModFlowParams(int(levels), int(radius), int(window), int(bool(subpixel)), int(fb_check))


def flow_max_displacement(p: ModFlowParams) -> int:
    """Largest displacement (px) the coarse-to-fine search can reach: radius * 2^(levels-1) + 2^(levels-1) - 1."""
    return p.radius * (1 << (p.levels - 1)) + (1 << (p.levels - 1)) - 1


class ModEgoParams(C.Structure):
    _fields_ = [("stride", C.c_int32), ("hypotheses", C.c_int32), ("iterations", C.c_int32), ("min_inliers", C.c_int32),
                ("inlier_threshold", C.c_float), ("min_disparity", C.c_float), ("seed", C.c_uint32), ("reserved", C.c_int32)]


class ModEgoResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("correspondences", C.c_int32), ("inliers", C.c_int32), ("iterations", C.c_int32),
                ("rms_px", C.c_double)]


def ego_params(stride: int = 4, hypotheses: int = 256, iterations: int = 10, min_inliers: int = 50, inlier_threshold: float = 2.0,
               min_disparity: float = 1.0, seed: int = 0) -> ModEgoParams:
    """ModEgoParams with the defaults of include/mod_sf.h."""
    return ModEgoParams(int(stride), int(hypotheses), int(iterations), int(min_inliers), float(inlier_threshold), float(min_disparity),
                        int(seed) & 0xFFFFFFFF, 0)


class ModImageLayout(C.Structure):
    _fields_ = [("encoding", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("step", C.c_int32), ("x0", C.c_int32),
                ("y0", C.c_int32)]


def image_layout(encoding, width: int, height: int, step=None, x0: int = 0, y0: int = 0) -> ModImageLayout:
    """ModImageLayout of a sensor_msgs/Image: `encoding` a MOD_ENCODING_* value or its ROS name ("bgr8", "bayer_rggb8", ...); step None = packed
    rows (width * channels); (x0, y0) = top-left of the camera-sized window taken from it.  For a side-by-side message (width = one
    eye's) pass the step of the whole row."""
    if isinstance(encoding, str):
        enc = ENCODINGS[encoding] if encoding in ENCODINGS else BAYER_ENCODINGS[encoding]
    else:
        enc = int(encoding)
    if step is None:
        step = int(width) * CHANNELS.get(enc, BAYER_CHANNELS.get(enc, 1))
    return ModImageLayout(enc, int(width), int(height), int(step), int(x0), int(y0))


class ModImageBinning(C.Structure):
    _fields_ = [("bx", C.c_int32), ("by", C.c_int32), ("mode", C.c_int32), ("reserved", C.c_int32)]


def image_binning(bx: int = 1, by: int = 1, mode=MOD_BIN_MEAN) -> ModImageBinning:
    """ModImageBinning (mod_set_image_binning): factors 1..4 and `mode` a MOD_BIN_* value or "mean" / "nearest"; bx = by = 1 is off."""
    return ModImageBinning(int(bx), int(by), BIN_MODES[mode] if isinstance(mode, str) else int(mode), 0)


def binned_camera(cam, binning: ModImageBinning, x0: int = 0, y0: int = 0):
    """The camera to give set_camera while `binning` is on, from the FULL-resolution camera `cam` (its P) and the layout's window
    origin: what image_geometry does with binning_x / binning_y, in float64.  fx, Tx and disp_f are divided by bx, fy and Ty by by; the
    principal point moves to the window and is divided likewise, MOD_BIN_MEAN taking the block's centre ((bx - 1) / 2 earlier), MOD_BIN_NEAREST
    its top-left pixel.  width and height become cam.width // bx, cam.height // by: state the window's size yourself when it is a crop.
    Returns a copy of the same type (dataclasses.replace)."""
    import dataclasses
    bx, by = int(binning.bx), int(binning.by)
    if bx < 1 or by < 1:
        raise ValueError("binning factors must be >= 1")
    ox, oy = ((bx - 1) / 2.0, (by - 1) / 2.0) if binning.mode == MOD_BIN_MEAN else (0.0, 0.0)
    return dataclasses.replace(cam, width=int(cam.width) // bx, height=int(cam.height) // by,
                               fx=float(cam.fx) / bx, fy=float(cam.fy) / by,
                               cx=(float(cam.cx) - x0 - ox) / bx, cy=(float(cam.cy) - y0 - oy) / by,
                               Tx=float(cam.Tx) / bx, Ty=float(cam.Ty) / by, disp_f=float(cam.disp_f) / bx)


def centred_window(msg_w: int, msg_h: int, W: int, H: int):
    """Origin (x0, y0) of the centred W x H window of a msg_w x msg_h image: image_crop.cpp:24-40's integer (msg - size) / 2."""
    if not (0 < W <= msg_w and 0 < H <= msg_h):
        raise ValueError("the window must fit inside the image")
    return (msg_w - W) // 2, (msg_h - H) // 2


class ModRectifyCamera(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("K", C.c_double * 9), ("D", C.c_double * 8), ("R", C.c_double * 9),
                ("P", C.c_double * 12)]


def rectify_camera(width: int, height: int, K, D, R, P) -> ModRectifyCamera:
    """ModRectifyCamera from the fields of the raw image's sensor_msgs/CameraInfo: K (9), R (9), P (12) row-major (flat or nested),
    D = k1 k2 p1 p2 [k3 [k4 k5 k6]] (plumb_bob: five, rational_polynomial: eight; shorter ones are padded with zeros)."""
    def flat(v, n, name):
        out = [float(x) for row in v for x in (row if hasattr(row, "__len__") else [row])]
        if len(out) != n:
            raise ValueError(f"{name} must have {n} entries")
        return out
    d = [float(x) for x in D]
    if len(d) > 8:
        raise ValueError("D has at most 8 coefficients (k1 k2 p1 p2 k3 k4 k5 k6)")
    d += [0.0] * (8 - len(d))
    return ModRectifyCamera(int(width), int(height), (C.c_double * 9)(*flat(K, 9, "K")), (C.c_double * 8)(*d),
                            (C.c_double * 9)(*flat(R, 9, "R")), (C.c_double * 12)(*flat(P, 12, "P")))


class ModDepthLayout(C.Structure):
    _fields_ = [("encoding", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("step", C.c_int32), ("x0", C.c_int32),
                ("y0", C.c_int32), ("unit", C.c_float)]


def depth_layout(encoding, width: int, height: int, step=None, x0: int = 0, y0: int = 0, unit: float = 0.0) -> ModDepthLayout:
    """ModDepthLayout of a depth sensor_msgs/Image: `encoding` a MOD_DEPTH_* value or its ROS name ("16UC1", "32FC1"); step None =
    packed rows; (x0, y0) = top-left of the camera-sized window taken from it (0, 0 with a registration); unit = metres per count,
    0 = the REP 118 default (0.001 for 16UC1, 1 for 32FC1)."""
    enc = DEPTH_ENCODINGS[encoding] if isinstance(encoding, str) else int(encoding)
    if step is None:
        step = int(width) * DEPTH_BYTES.get(enc, 2)
    return ModDepthLayout(enc, int(width), int(height), int(step), int(x0), int(y0), float(unit))


class ModDepthRegistration(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("R", C.c_double * 9),
                ("t", C.c_double * 3)]


def depth_registration(fx: float, fy: float, cx: float, cy: float, R=(1, 0, 0, 0, 1, 0, 0, 0, 1), t=(0, 0, 0)) -> ModDepthRegistration:
    """ModDepthRegistration: the depth camera's intrinsics (of the full depth message) and the transform depth optical frame -> image
    optical frame, P_img = R P_depth + t (R row-major, flat or nested)."""
    r = [float(x) for row in R for x in (row if hasattr(row, "__len__") else [row])]
    tt = [float(x) for x in t]
    if len(r) != 9 or len(tt) != 3:
        raise ValueError("R must have 9 entries and t 3")
    return ModDepthRegistration(float(fx), float(fy), float(cx), float(cy), (C.c_double * 9)(*r), (C.c_double * 3)(*tt))


class ModDepthDistortion(C.Structure):
    _fields_ = [("D", C.c_double * 8)]


def depth_distortion(D) -> ModDepthDistortion:
    """ModDepthDistortion from the D of the depth camera's sensor_msgs/CameraInfo: k1 k2 p1 p2 [k3 [k4 k5 k6]] (four, plumb_bob's five or
    rational_polynomial's eight coefficients; shorter ones are padded with zeros)."""
    d = [float(x) for x in D]
    if len(d) not in (4, 5, 8):
        raise ValueError("D must have 4, 5 or 8 coefficients (k1 k2 p1 p2 k3 k4 k5 k6)")
    return ModDepthDistortion((C.c_double * 8)(*(d + [0.0] * (8 - len(d)))))


class ModDepthFilter(C.Structure):
    _fields_ = [("z_min", C.c_float), ("z_max", C.c_float), ("window", C.c_int32), ("min_support", C.c_int32), ("tol_abs", C.c_float),
                ("tol_rel", C.c_float), ("reserved", C.c_int32 * 2)]


def depth_filter(z_min: float = 0.0, z_max: float = 0.0, window: int = 0, min_support: int = 3, tol_abs: float = 0.0,
                 tol_rel: float = 0.02) -> ModDepthFilter:
    """ModDepthFilter of mod_set_depth_filter: the range rule keeps z_min <= z <= z_max (metres; 0 = that bound is off); the support
    rule (window 3 or 5, 0 = off) keeps a sample that at least min_support of its window's other samples agree with to within
    tol_abs + tol_rel * z, which removes flying pixels at depth discontinuities.  The defaults are a convenience, NOT tuned on camera
    data: choose min_support and the tolerances for the sensor at hand.  All defaults together are the filter switched off."""
    return ModDepthFilter(float(z_min), float(z_max), int(window), int(min_support), float(tol_abs), float(tol_rel), (C.c_int32 * 2)(0, 0))


class ModDepthTemporal(C.Structure):
    _fields_ = [("alpha", C.c_float), ("delta_abs", C.c_float), ("delta_rel", C.c_float), ("hold", C.c_int32), ("reserved", C.c_int32 * 4)]


def depth_temporal(alpha: float = 0.4, delta_abs: float = 0.02, delta_rel: float = 0.0, hold: int = 0) -> ModDepthTemporal:
    """ModDepthTemporal of mod_set_depth_temporal: per pixel an exponential moving average over the frames, s += alpha * (x - s), while
    the new depth stays within delta_abs + delta_rel * z (metres) of the average, a restart at the new sample where it does not; a
    pixel without a reading repeats its average for at most `hold` frames (0: never, 254 at most).  alpha = 0 is the filter switched
    off; alpha = 1 with hold = 0 is the identity.  The defaults are a convenience, NOT tuned on camera data: choose alpha and the gate
    for the sensor's noise and the scene's motion."""
    return ModDepthTemporal(float(alpha), float(delta_abs), float(delta_rel), int(hold), (C.c_int32 * 4)(0, 0, 0, 0))


class ModDepthSpatial(C.Structure):
    _fields_ = [("window", C.c_int32), ("smooth", C.c_int32), ("fill_min", C.c_int32), ("tol_abs", C.c_float), ("tol_rel", C.c_float),
                ("reserved", C.c_int32 * 3)]


def depth_spatial(window: int = 5, smooth: bool = True, fill_min: int = 0, tol_abs: float = 0.0, tol_rel: float = 0.02) -> ModDepthSpatial:
    """ModDepthSpatial of mod_set_depth_spatial: with `smooth` a valid sample becomes the mean of the valid samples of its window (3, 5
    or 7; 0 = off) within tol_abs + tol_rel * z (metres) of it, so depth edges are not blurred; with fill_min > 0 a sample without a
    reading becomes the mean of its window's valid samples within that gate of the FARTHEST of them, where at least fill_min lie there
    (the background fills a hole, never the foreground).  One pass over the input: nothing cascades.  The defaults are a convenience,
    NOT tuned on camera data: choose the window, fill_min and the gate for the sensor's noise and its shadows."""
    return ModDepthSpatial(int(window), int(bool(smooth)), int(fill_min), float(tol_abs), float(tol_rel), (C.c_int32 * 3)(0, 0, 0))


class ModDepthDecimation(C.Structure):
    _fields_ = [("dx", C.c_int32), ("dy", C.c_int32), ("mode", C.c_int32), ("min_valid", C.c_int32), ("tol_abs", C.c_float), ("tol_rel", C.c_float),
                ("reserved", C.c_int32 * 2)]


def depth_decimation(dx: int = 2, dy: int = 2, mode="median", min_valid: int = 1, tol_abs: float = 0.0, tol_rel: float = 0.02) -> ModDepthDecimation:
    """ModDepthDecimation of mod_set_depth_decimation: every dx x dy block of the depth message (factors 1..4; dx = dy = 1 is off) becomes
    one sample, `mode` a MOD_DEPTH_DECIMATE_* value or "median" (the lower median of the block's valid samples, an input word), "min"
    (the nearest of them), "mean" (the mean of those within tol_abs + tol_rel * z, metres, of the median) or "nearest" (the block's
    top-left word, whatever it is); a block with fewer than max(min_valid, 1) valid samples has no reading.  The camera is the
    caller's: the first three go with MOD_BIN_MEAN's binned camera, "nearest" with MOD_BIN_NEAREST's (binned_camera)."""
    return ModDepthDecimation(int(dx), int(dy), int(DEPTH_DECIMATE_MODES.get(mode, mode)), int(min_valid), float(tol_abs), float(tol_rel),
                              (C.c_int32 * 2)(0, 0))


class ModClusterOut(C.Structure):
    _fields_ = [("labels", C.c_void_p), ("objects", C.c_void_p), ("n_objects", C.c_void_p), ("n_clusters", C.c_void_p)]


class ModClusterMembers(C.Structure):
    _fields_ = [("offsets", C.c_void_p), ("indices", C.c_void_p), ("points", C.c_void_p), ("reserved", C.c_int64)]


class ModClusterImage(C.Structure):
    _fields_ = [("image", C.c_void_p), ("host_image", C.c_void_p), ("palette_bgr", C.c_void_p), ("reserved", C.c_int64)]


MOD_OBJECT_BYTES = C.sizeof(ModObject)
assert C.sizeof(ModClusterImage) == 32
assert C.sizeof(ModClusterMembers) == 32
assert MOD_OBJECT_BYTES == 112
assert C.sizeof(ModRectifyCamera) == 312
assert C.sizeof(ModDepthLayout) == 28 and C.sizeof(ModDepthRegistration) == 128
assert C.sizeof(ModDepthFilter) == 32
assert C.sizeof(ModDepthTemporal) == 32
assert C.sizeof(ModDepthSpatial) == 32
assert C.sizeof(ModDepthDecimation) == 32
assert C.sizeof(ModImageBinning) == 16
assert C.sizeof(ModTextureFilter) == 16
assert C.sizeof(ModCornerFilter) == 16
assert C.sizeof(ModFlowMedian) == 16
assert C.sizeof(ModFlowFill) == 24
assert C.sizeof(ModDisparityFill) == 16
assert C.sizeof(ModDisparitySmooth) == 16


def distortion_model(model) -> int:
    """MOD_DISTORTION_* from the integer or from a CameraInfo's distortion_model string ("plumb_bob", "rational_polynomial",
    "equidistant").  An unknown string raises ValueError; an integer is passed on for the library to judge."""
    if isinstance(model, str):
        if model not in DISTORTION_MODELS:
            raise ValueError(f"unknown distortion model {model!r} (known: {', '.join(DISTORTION_MODELS)})")
        return DISTORTION_MODELS[model]
    return int(model)


class ModError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libmod_sf error {code}: {msg}")
        self.code = code


_vp, _i32 = C.c_void_p, C.c_int32
# Every symbol include/mod_sf.h declares, in the header's order of introduction, with its argtypes (None: not declared to ctypes).  The
# restype is c_int except where _RESTYPES says otherwise.  tests/test_abi.py compares the names with the header.
SIGNATURES = {
    "mod_abi_version": None,
    "mod_create": [C.POINTER(ModConfig), C.POINTER(_vp)],
    "mod_destroy": [_vp],
    "mod_last_error": [_vp],
    "mod_set_camera": [_vp, C.POINTER(ModCamera)],
    "mod_set_params": [_vp, C.POINTER(ModParams)],
    "mod_get_camera": [_vp, C.POINTER(ModCamera)],
    "mod_get_params": [_vp, C.POINTER(ModParams)],
    "mod_synchronize": [_vp],
    "mod_scene_flow_dev": [_vp, C.POINTER(ModFrameBatch), C.POINTER(ModSceneFlowPlanes)],
    "mod_dynamic_mask_dev": [_vp, _i32, _vp, _vp, _vp, _vp],
    "mod_cluster_dev": [_vp, _i32, C.POINTER(ModSceneFlowPlanes), C.POINTER(ModClusterOut)],
    "mod_process_dev": [_vp, C.POINTER(ModFrameBatch), C.POINTER(ModSceneFlowPlanes), C.POINTER(ModClusterOut)],
    "mod_pack_cloud_dev": [_vp, _i32, C.POINTER(ModSceneFlowPlanes), _vp],
    "mod_unpack_cloud_dev": [_vp, _i32, _vp, C.POINTER(ModSceneFlowPlanes)],
    "mod_process_frame_host": [_vp, _vp, _vp, _vp, C.POINTER(ModTransform), C.c_double, _vp, _vp, _vp, _i32, C.POINTER(_i32)],
    "mod_cluster_cloud_host": [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, C.POINTER(_i32)],
    "mod_submit_frame_host": [_vp, _vp, _vp, _vp, C.POINTER(ModTransform), C.c_double, _vp, _vp, _vp, _i32, C.POINTER(_i32)],
    "mod_submit_stereo_host": [_vp, _vp, _vp, C.POINTER(ModSgmParams), _vp, C.POINTER(ModTransform), C.c_double, _vp, _vp, _vp, _i32, _vp,
                               C.POINTER(_i32)],
    "mod_collect_frame_host": [_vp, _i32, C.POINTER(_i32)],
    "mod_forget_previous": [_vp],
    "mod_host_malloc": [_vp, C.c_uint64, C.POINTER(_vp)],
    "mod_host_free": [_vp, _vp],
    "mod_malloc": [_vp, C.c_uint64, C.POINTER(_vp)],
    "mod_free": [_vp, _vp],
    "mod_memcpy_h2d": [_vp, _vp, _vp, C.c_uint64],
    "mod_memcpy_d2h": [_vp, _vp, _vp, C.c_uint64],
    "mod_set_profiling": [_vp, _i32],
    "mod_get_stage_time": [_vp, _i32, C.POINTER(C.c_double), C.POINTER(C.c_int64)],
    "mod_reset_stage_times": [_vp],
    "mod_depth_image_dev": [_vp, _i32, _vp, _vp],
    "mod_depth_image_host": [_vp, _vp, _vp],
    "mod_static_flow_host": [_vp, _vp, C.POINTER(ModTransform), _vp],
    "mod_sgm_census_dev": [_vp, _i32, _vp, _vp],
    "mod_sgm_path_dev": [_vp, _i32, _vp, _vp, C.POINTER(ModSgmParams), _i32, _vp, _vp],
    "mod_sgm_compute_dev": [_vp, _i32, _vp, _vp, C.POINTER(ModSgmParams), _vp],
    "mod_sgm_compute_host": [_vp, _vp, _vp, C.POINTER(ModSgmParams), _vp],
    "mod_flow_compute_dev": [_vp, _i32, _vp, _vp, C.POINTER(ModFlowParams), _vp],
    "mod_flow_compute_host": [_vp, _vp, _vp, C.POINTER(ModFlowParams), _vp],
    "mod_submit_images_host": [_vp, _vp, _vp, C.POINTER(ModSgmParams), C.POINTER(ModFlowParams), C.POINTER(ModTransform), C.c_double, _vp,
                               _vp, _vp, _i32, _vp, _vp, C.POINTER(_i32)],
    "mod_egomotion_dev": [_vp, _i32, _vp, _vp, _vp, C.POINTER(ModEgoParams), _vp, _vp],
    "mod_egomotion_host": [_vp, _vp, _vp, _vp, C.POINTER(ModEgoParams), C.POINTER(ModTransform), C.POINTER(ModEgoResult)],
    "mod_submit_odometry_host": [_vp, _vp, _vp, C.POINTER(ModSgmParams), C.POINTER(ModFlowParams), C.POINTER(ModEgoParams), C.c_double,
                                 _vp, _vp, _vp, _i32, _vp, _vp, C.POINTER(ModTransform), C.POINTER(ModEgoResult), C.POINTER(_i32)],
    "mod_set_image_layout": [_vp, C.POINTER(ModImageLayout)],
    "mod_get_image_layout": [_vp, C.POINTER(ModImageLayout)],
    "mod_image_to_mono_dev": [_vp, _i32, _vp, C.POINTER(ModImageLayout), _vp],
    "mod_set_disparity_subpixel": [_vp, _i32],
    "mod_get_disparity_subpixel": [_vp, C.POINTER(_i32)],
    "mod_set_disparity_filters": [_vp, C.POINTER(ModDisparityFilters)],
    "mod_get_disparity_filters": [_vp, C.POINTER(ModDisparityFilters)],
    "mod_set_disparity_offset": [_vp, _i32],
    "mod_get_disparity_offset": [_vp, C.POINTER(_i32)],
    "mod_disparity_speckle_dev": [_vp, _i32, _vp, _i32, _i32],
    "mod_set_disparity_smooth": [_vp, C.POINTER(ModDisparitySmooth)],
    "mod_get_disparity_smooth": [_vp, C.POINTER(ModDisparitySmooth)],
    "mod_disparity_smooth_dev": [_vp, _i32, _vp, C.POINTER(ModDisparitySmooth), _vp],
    "mod_set_disparity_fill": [_vp, C.POINTER(ModDisparityFill)],
    "mod_get_disparity_fill": [_vp, C.POINTER(ModDisparityFill)],
    "mod_disparity_fill_dev": [_vp, _i32, _vp, C.POINTER(ModDisparityFill), _vp],
    "mod_set_flow_propagation": [_vp, _i32],
    "mod_get_flow_propagation": [_vp, C.POINTER(_i32)],
    "mod_set_texture_filter": [_vp, C.POINTER(ModTextureFilter)],
    "mod_get_texture_filter": [_vp, C.POINTER(ModTextureFilter)],
    "mod_texture_dev": [_vp, _i32, _vp, C.POINTER(ModTextureFilter), _vp],
    "mod_texture_reject_dev": [_vp, _i32, _vp, C.POINTER(ModTextureFilter), _vp, _vp],
    "mod_set_flow_corner_filter": [_vp, C.POINTER(ModCornerFilter)],
    "mod_get_flow_corner_filter": [_vp, C.POINTER(ModCornerFilter)],
    "mod_flow_corner_dev": [_vp, _i32, _vp, C.POINTER(ModCornerFilter), _vp],
    "mod_flow_corner_reject_dev": [_vp, _i32, _vp, C.POINTER(ModCornerFilter), _vp],
    "mod_set_flow_median": [_vp, C.POINTER(ModFlowMedian)],
    "mod_get_flow_median": [_vp, C.POINTER(ModFlowMedian)],
    "mod_flow_median_dev": [_vp, _i32, _vp, C.POINTER(ModFlowMedian), _vp],
    "mod_set_flow_fill": [_vp, C.POINTER(ModFlowFill)],
    "mod_get_flow_fill": [_vp, C.POINTER(ModFlowFill)],
    "mod_flow_fill_dev": [_vp, _i32, _vp, _vp, C.POINTER(ModFlowFill), _vp],
    "mod_set_rectification": [_vp, C.POINTER(ModRectifyCamera), C.POINTER(ModRectifyCamera)],
    "mod_get_rectification": [_vp, C.POINTER(ModRectifyCamera), C.POINTER(ModRectifyCamera), C.POINTER(_i32)],
    "mod_rectify_dev": [_vp, _i32, _vp, C.POINTER(ModImageLayout), _i32, _vp],
    "mod_rectify_map_host": [_vp, _i32, C.POINTER(ModImageLayout), _vp],
    "mod_set_distortion_model": [_vp, _i32],
    "mod_get_distortion_model": [_vp, C.POINTER(_i32)],
    "mod_set_side_by_side": [_vp, _i32],
    "mod_get_side_by_side": [_vp, C.POINTER(_i32)],
    "mod_set_image_binning": [_vp, C.POINTER(ModImageBinning)],
    "mod_get_image_binning": [_vp, C.POINTER(ModImageBinning)],
    "mod_set_depth_layout": [_vp, C.POINTER(ModDepthLayout)],
    "mod_get_depth_layout": [_vp, C.POINTER(ModDepthLayout)],
    "mod_set_depth_registration": [_vp, C.POINTER(ModDepthRegistration)],
    "mod_get_depth_registration": [_vp, C.POINTER(ModDepthRegistration), C.POINTER(_i32)],
    "mod_depth_to_disparity_dev": [_vp, _i32, _vp, C.POINTER(ModDepthLayout), _vp],
    "mod_submit_depth_host": [_vp, _vp, _vp, C.POINTER(ModFlowParams), C.POINTER(ModEgoParams), C.POINTER(ModTransform), C.c_double, _vp,
                              _vp, _vp, _i32, _vp, _vp, C.POINTER(ModTransform), C.POINTER(ModEgoResult), C.POINTER(_i32)],
    "mod_set_depth_splat": [_vp, _i32],
    "mod_get_depth_splat": [_vp, C.POINTER(_i32)],
    "mod_set_depth_distortion": [_vp, C.POINTER(ModDepthDistortion)],
    "mod_get_depth_distortion": [_vp, C.POINTER(ModDepthDistortion), C.POINTER(_i32)],
    "mod_depth_rays_host": [_vp, C.POINTER(ModDepthLayout), _i32, _vp],
    "mod_set_depth_filter": [_vp, C.POINTER(ModDepthFilter)],
    "mod_get_depth_filter": [_vp, C.POINTER(ModDepthFilter)],
    "mod_depth_filter_dev": [_vp, _i32, _vp, C.POINTER(ModDepthLayout), C.POINTER(ModDepthFilter), _vp],
    "mod_set_depth_spatial": [_vp, C.POINTER(ModDepthSpatial)],
    "mod_get_depth_spatial": [_vp, C.POINTER(ModDepthSpatial)],
    "mod_depth_spatial_dev": [_vp, _i32, _vp, C.POINTER(ModDepthLayout), C.POINTER(ModDepthSpatial), _vp],
    "mod_set_depth_decimation": [_vp, C.POINTER(ModDepthDecimation)],
    "mod_get_depth_decimation": [_vp, C.POINTER(ModDepthDecimation)],
    "mod_depth_decimate_dev": [_vp, _i32, _vp, C.POINTER(ModDepthLayout), C.POINTER(ModDepthDecimation), _vp],
    "mod_set_depth_temporal": [_vp, C.POINTER(ModDepthTemporal)],
    "mod_get_depth_temporal": [_vp, C.POINTER(ModDepthTemporal)],
    "mod_reset_depth_temporal": [_vp],
    "mod_depth_temporal_dev": [_vp, _i32, _vp, C.POINTER(ModDepthLayout), C.POINTER(ModDepthTemporal), _vp, _vp, _vp],
    "mod_set_cluster_members": [_vp, C.POINTER(ModClusterMembers)],
    "mod_get_cluster_members": [_vp, C.POINTER(ModClusterMembers), C.POINTER(_i32)],
    "mod_set_cluster_image": [_vp, C.POINTER(ModClusterImage)],
    "mod_get_cluster_image": [_vp, C.POINTER(ModClusterImage), C.POINTER(_i32)],
    "mod_cluster_image_dev": [_vp, _i32, _vp, _vp, _vp, _vp],
    "mod_cluster_color": [_i32, _i32, _vp, _vp],
    "mod_cluster_palette": [_vp],
    "mod_static_flow_dev": [_vp, _i32, _vp, _vp, _vp],
    "mod_flow_image_dev": [_vp, _i32, _vp, C.c_float, _vp],
    "mod_flow_residual_image_dev": [_vp, _i32, _vp, _vp, C.c_float, _vp],
    "mod_disparity_image_dev": [_vp, _i32, _vp, _vp],
    "mod_flow_color": [C.c_float, C.c_float, C.c_float, _vp],
}
_RESTYPES = {"mod_destroy": None, "mod_last_error": C.c_char_p}
EXPORTS = list(SIGNATURES)
# csrc/mod_sf_debug.h: only a build with the debug hooks compiled in exports these (the product does not)
DEBUG_SIGNATURES = {
    "mod_debug_read": [_vp, C.c_int, _vp, C.c_ulonglong],
    "mod_debug_counters": [_vp, C.POINTER(C.c_uint64)],
}


def declare(L, missing_ok: bool = False):
    """Give the functions of the loaded library `L` the argtypes and restypes of SIGNATURES, and those of DEBUG_SIGNATURES where `L`
    exports them.  A name of SIGNATURES that `L` lacks raises AttributeError naming it, or is left out with missing_ok (an older build)."""
    for table, optional in ((SIGNATURES, missing_ok), (DEBUG_SIGNATURES, True)):
        for name, argtypes in table.items():
            fn = getattr(L, name, None)
            if fn is None:
                if optional:
                    continue
                raise AttributeError(f"{getattr(L, '_name', L)} does not export {name}")
            if argtypes is not None:
                fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, C.c_int)
    return L


def bind(path: str, missing_ok: bool = False) -> C.CDLL:
    """Load the build of the library at `path` and declare its functions (declare()).  Import torch first when device pointers of
    torch's are to be handed to it (see the module docstring); load() does."""
    return declare(C.CDLL(path), missing_ok)


_lib = None


def load(require_torch_first: bool = True):
    """Load libmod_sf.so (once: the bound library is cached).  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: the HIP extension has not been built "
                          f"(run __graft_entry__.build() or `make -C moving_object_detector_amd/csrc`). "
                          f"There is no CPU fallback.")
    if require_torch_first:
        import torch  # noqa: F401  (see module docstring: one HIP runtime per process)
    _lib = bind(LIB_PATH)
    return _lib


def palette_bytes(palette):
    """A caller's colour table as the 768 bytes B, G, R the library takes (a (256, 3) uint8 array, or anything of 768 bytes), or None."""
    if palette is None:
        return None
    import numpy as np
    b = np.ascontiguousarray(np.asarray(palette, dtype=np.uint8)).reshape(-1)
    if b.size != 768:
        raise ValueError("a colour table is 256 x 3 bytes B, G, R")
    return (C.c_uint8 * 768).from_buffer_copy(b.tobytes())


def cluster_color(k: int, K: int, palette=None):
    """(b, g, r) of label k in a frame of K clusters (mod_cluster_color): entry (k * 255) // K of `palette`, or of the built-in table.
    Needs no GPU.  Raises ValueError unless 0 <= k < K."""
    out, pal = (C.c_uint8 * 3)(), palette_bytes(palette)
    if load().mod_cluster_color(int(k), int(K), pal, out) != MOD_OK:
        raise ValueError(f"cluster_color: need 0 <= k < K, got k={k}, K={K}")
    return tuple(out)


def cluster_palette():
    """The built-in colour table (mod_cluster_palette) as a (256, 3) uint8 array B, G, R.  Needs no GPU."""
    import numpy as np
    out = (C.c_uint8 * 768)()
    if load().mod_cluster_palette(out) != MOD_OK:
        raise RuntimeError("mod_cluster_palette failed")
    return np.frombuffer(bytes(out), dtype=np.uint8).reshape(256, 3).copy()


def flow_color(fx: float, fy: float, max_px: float):
    """(b, g, r) of the flow vector (fx, fy) at full strength max_px (mod_flow_color): the legend of Context.flow_image, by the
    renderer's own arithmetic.  Needs no GPU.  Raises ValueError unless max_px is finite and > 0."""
    out = (C.c_uint8 * 3)()
    if load().mod_flow_color(float(fx), float(fy), float(max_px), out) != MOD_OK:
        raise ValueError(f"flow_color: max_px must be finite and > 0, got {max_px}")
    return tuple(out)


def camera_struct(cam) -> ModCamera:
    return ModCamera(int(cam.width), int(cam.height), float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy),
                     float(cam.Tx), float(cam.Ty), float(cam.disp_f), float(cam.disp_T), float(cam.min_disparity),
                     float(cam.max_disparity))


def params_struct(prm) -> ModParams:
    return ModParams(int(prm.dynamic_flow_diff), int(prm.cluster_size), int(prm.neighbor_distance), 0,
                     float(prm.depth_diff), float(prm.dynamic_speed))


def transforms_array(ts, qs):
    n = len(ts)
    arr = (ModTransform * n)()
    for i in range(n):
        for k in range(3):
            arr[i].t[k] = float(ts[i][k])
        for k in range(4):
            arr[i].q[k] = float(qs[i][k])
    return arr
