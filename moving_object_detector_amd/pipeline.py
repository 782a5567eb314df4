"""Device-resident driver of the C ABI: owns a ModContext and the HBM buffers (torch tensors are used purely as
device memory + stream plumbing; every computation happens in libmod_sf.so)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import capi
from .host_calls import HostCalls

PLANES = ("x", "y", "z", "vx", "vy", "vz")

OBJECT_DTYPE = np.dtype([("id", "<i4"), ("n_points", "<i4"), ("center", "<f8", 3), ("orientation", "<f8", 4),
                         ("velocity", "<f8", 3), ("bounding_box", "<f8", 3)])
assert OBJECT_DTYPE.itemsize == capi.MOD_OBJECT_BYTES
EGO_RESULT_DTYPE = np.dtype([("status", "<i4"), ("correspondences", "<i4"), ("inliers", "<i4"), ("iterations", "<i4"), ("rms_px", "<f8")])
assert EGO_RESULT_DTYPE.itemsize == C.sizeof(capi.ModEgoResult)


# Planes of one call are carved from ONE block with their bases 1 MiB further apart than their size: at 512 x 1280 x 720 a plane is a
# multiple of 8 MiB, so back to back the nine streams of a scene-flow wave (3 in, 6 out) would carry the same low address bits — the
# same DRAM bank group at the same moment.  Measured inside one process (tools/ab_skew.py): -1 ... -3 % on the scene-flow kernel for
# 128 KiB ... 1 MiB of stagger (multiples of 2 MiB: nothing), depending on how (un)lucky the box's back-to-back placement is.
PLANE_STAGGER_BYTES = 1 << 20


def staggered(sizes, dtype, device, stagger_bytes: int = PLANE_STAGGER_BYTES):
    """1-D tensors of `sizes` elements each, carved from one allocation, consecutive bases `stagger_bytes` apart beyond their sizes."""
    skew = stagger_bytes // torch.empty((), dtype=dtype).element_size()
    flat = torch.empty(sum(sizes) + skew * (len(sizes) - 1), dtype=dtype, device=device)
    out, at = [], 0
    for n in sizes:
        out.append(flat[at:at + n])
        at += n + skew
    return out


class PinnedBuffer:
    """Page-locked host memory of a context (Context.pinned_copy)."""

    def __init__(self, ctx, ptr: int, nbytes: int):
        self._ctx, self.ptr, self.nbytes, self.array = ctx, ptr, nbytes, None

    def free(self) -> None:
        if self.ptr:
            self.array = None
            self._ctx._check(self._ctx.lib.mod_host_free(self._ctx.h, self.ptr))
            self._ctx._pinned.remove(self)
            self.ptr = None


class Context(HostCalls):
    """One context per GPU / stream (single caller), like one SceneFlowConstructor + one ClustererNodelet.  The synchronous host
    calls (disparity_host, process_frame_host, ...) are host_calls.HostCalls'."""

    def __init__(self, width: int, height: int, max_frames: int = 1, device: int = 0, max_objects: int = 0,
                 use_torch_stream: bool = True, batch_chunks: int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: the MI355X path has no CPU fallback")
        self.lib = capi.load()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.width, self.height, self.max_frames = width, height, max_frames
        stream = torch.cuda.current_stream(self.device).cuda_stream if use_torch_stream else None
        cfg = capi.ModConfig(device, width, height, max_frames, max_objects, batch_chunks, stream)
        h = C.c_void_p()
        rc = self.lib.mod_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise capi.ModError(rc, "mod_create failed")
        self.h = h
        self.max_objects = max_objects if max_objects > 0 else max(1, (width * height) // 100)
        self.mask_words = (width + 63) // 64
        self._ws = None
        self._members_ws = None
        self._image_keep = None
        self._pinned = []

    # ---- configuration ----------------------------------------------------------------------------------------
    def _done(self, rc: int, name: str) -> None:
        """_check for a call that has no skip to report: any code but 0 raises."""
        if self._check(rc) != 0:
            raise capi.ModError(rc, f"{name} skipped")

    def set_camera(self, cam) -> None:
        s = cam if isinstance(cam, capi.ModCamera) else capi.camera_struct(cam)
        self._check(self.lib.mod_set_camera(self.h, C.byref(s)))
        self.width, self.height = s.width, s.height
        self.mask_words = (s.width + 63) // 64

    def set_params(self, prm) -> None:
        s = prm if isinstance(prm, capi.ModParams) else capi.params_struct(prm)
        self._check(self.lib.mod_set_params(self.h, C.byref(s)))

    def get_camera(self) -> capi.ModCamera:
        s = capi.ModCamera()
        self._check(self.lib.mod_get_camera(self.h, C.byref(s)))
        return s

    def get_params(self) -> capi.ModParams:
        s = capi.ModParams()
        self._check(self.lib.mod_get_params(self.h, C.byref(s)))
        return s

    def set_image_layout(self, layout: Optional[capi.ModImageLayout]) -> None:
        """Layout of the host images the *_host image entry points read (mod_set_image_layout); None = mono8 packed at the camera size."""
        self._check(self.lib.mod_set_image_layout(self.h, C.byref(layout) if layout is not None else None))

    def get_image_layout(self) -> capi.ModImageLayout:
        s = capi.ModImageLayout()
        self._check(self.lib.mod_get_image_layout(self.h, C.byref(s)))
        return s

    def set_disparity_subpixel(self, on) -> None:
        """Sub-pixel mode of the on-GPU disparity estimator (mod_set_disparity_subpixel): False / 0 = whole disparities (the default),
        True / 4 = sixteenths of a pixel.  Read when a call or a submit enqueues its estimator."""
        bits = (capi.MOD_SGM_FRACTION_BITS if on else 0) if isinstance(on, (bool, np.bool_)) else int(on)   # any other number: as given
        self._check(self.lib.mod_set_disparity_subpixel(self.h, bits))

    def get_disparity_subpixel(self) -> int:
        bits = C.c_int32(-1)
        self._check(self.lib.mod_get_disparity_subpixel(self.h, C.byref(bits)))
        return bits.value

    def set_disparity_filters(self, uniqueness_ratio: int = 0, speckle_size: int = 0, speckle_range: int = 0) -> None:
        """Rejection filters of the on-GPU disparity estimator (mod_set_disparity_filters), all off by default: uniqueness_ratio in
        percent (StereoSGBM's rule), speckle_size / speckle_range as in stereo_image_proc (regions of at most speckle_size pixels whose
        neighbours differ by at most speckle_range go).  Read when a call or a submit enqueues its estimator."""
        f = capi.ModDisparityFilters(int(uniqueness_ratio), int(speckle_size), int(speckle_range), 0)
        self._check(self.lib.mod_set_disparity_filters(self.h, C.byref(f)))

    def get_disparity_filters(self) -> dict:
        f = capi.ModDisparityFilters(-1, -1, -1, -1)
        self._check(self.lib.mod_get_disparity_filters(self.h, C.byref(f)))
        return {"uniqueness_ratio": f.uniqueness_ratio, "speckle_size": f.speckle_size, "speckle_range": f.speckle_range}

    def set_disparity_fill(self, reach=None, directions: int = 8, mode="min", min_found: int = 1) -> None:
        """Occlusion hole fill of the on-GPU disparity estimator (mod_set_disparity_fill), off by default: the estimator's last stage,
        behind the speckle stage; an invalid disparity walks the first `directions` (2, 4 or 8) path directions for up to `reach`
        (1..256) steps each to the first valid word and becomes the lowest ("min"), second lowest ("second") or lower median ("median")
        of the found words where at least `min_found` directions found one.  No argument, None or 0 turns it off; a
        capi.ModDisparityFill is taken as it is.  Read when a call or a submit enqueues its estimator; the ego-motion estimator and the
        flow fill's gate see the filled disparity.  The defaults are not tuned."""
        if reach is None:
            self._check(self.lib.mod_set_disparity_fill(self.h, None))
            return
        f = reach if isinstance(reach, capi.ModDisparityFill) else capi.disparity_fill(reach, directions, mode, min_found)
        self._check(self.lib.mod_set_disparity_fill(self.h, C.byref(f)))

    def get_disparity_fill(self) -> capi.ModDisparityFill:
        f = capi.ModDisparityFill(-1, -1, -1, -1)
        self._check(self.lib.mod_get_disparity_fill(self.h, C.byref(f)))
        return f

    def set_disparity_smooth(self, window=None, tol: float = 1.0, min_members: int = 1) -> None:
        """Edge-preserving smoother of the on-GPU disparity estimator (mod_set_disparity_smooth), off by default: the estimator's stage
        behind the speckle stage and in front of the hole fill; a valid disparity d becomes the mean of the valid disparities of its
        `window` x `window` square (3, 5 or 7) within `tol` px of d, where at least `min_members` lie there; every other pixel stays.
        No argument or None turns it off; a capi.ModDisparitySmooth is taken as it is.  Read when a call or a submit enqueues its
        estimator; the ego-motion estimator and the flow fill's gate see the smoothed disparity.  The defaults are not tuned."""
        if window is None:
            self._check(self.lib.mod_set_disparity_smooth(self.h, None))
            return
        f = window if isinstance(window, capi.ModDisparitySmooth) else capi.disparity_smooth(window, tol, min_members)
        self._check(self.lib.mod_set_disparity_smooth(self.h, C.byref(f)))

    def get_disparity_smooth(self) -> capi.ModDisparitySmooth:
        f = capi.ModDisparitySmooth(-1, -1, -1.0, -1)
        self._check(self.lib.mod_get_disparity_smooth(self.h, C.byref(f)))
        return f

    def set_disparity_offset(self, d0: int = 0) -> None:
        """Minimum disparity of the on-GPU disparity estimator (mod_set_disparity_offset): the search window is [d0, d0 + disparities),
        0 <= d0 <= 128; 0 (the default) = the window starts at 0.  Invalid pixels stay -1.  Read when a call or a submit enqueues its
        estimator."""
        self._check(self.lib.mod_set_disparity_offset(self.h, int(d0)))

    def get_disparity_offset(self) -> int:
        d0 = C.c_int32(-1)
        self._check(self.lib.mod_get_disparity_offset(self.h, C.byref(d0)))
        return d0.value

    def set_texture_filter(self, threshold=None, window: int = 9, cap: int = 31,
                           apply: int = capi.MOD_TEXTURE_DISPARITY | capi.MOD_TEXTURE_FLOW) -> None:   # noqa: A002 (the header's name)
        """Texture threshold of the on-GPU disparity and flow estimators (mod_set_texture_filter), off by default: pixels whose texture
        sum T (Context.texture) is below `threshold` become -1 in the disparity / (NaN, NaN) in the flow of the estimators named by
        `apply`.  No argument or None turns it off; a capi.ModTextureFilter is taken as it is.  Read when a call or a submit enqueues
        its estimator."""
        if threshold is None:
            self._check(self.lib.mod_set_texture_filter(self.h, None))
            return
        f = threshold if isinstance(threshold, capi.ModTextureFilter) else capi.texture_filter(threshold, window, cap, apply)
        self._check(self.lib.mod_set_texture_filter(self.h, C.byref(f)))

    def get_texture_filter(self) -> capi.ModTextureFilter:
        f = capi.ModTextureFilter(-1, -1, -1, -1)
        self._check(self.lib.mod_get_texture_filter(self.h, C.byref(f)))
        return f

    def set_flow_corner_filter(self, threshold=None, window: int = 9, cap: int = 31) -> None:
        """Min-eigenvalue (aperture) threshold of the on-GPU flow estimator (mod_set_flow_corner_filter), off by default: pixels whose
        strength E (Context.flow_corner) of the now image is below `threshold` become (NaN, NaN) in the flow.  No argument or None turns
        it off; a capi.ModCornerFilter is taken as it is.  Read when a call or a submit enqueues the flow estimator."""
        if threshold is None:
            self._check(self.lib.mod_set_flow_corner_filter(self.h, None))
            return
        f = threshold if isinstance(threshold, capi.ModCornerFilter) else capi.corner_filter(threshold, window, cap)
        self._check(self.lib.mod_set_flow_corner_filter(self.h, C.byref(f)))

    def get_flow_corner_filter(self) -> capi.ModCornerFilter:
        f = capi.ModCornerFilter(-1, -1, -1, -1)
        self._check(self.lib.mod_get_flow_corner_filter(self.h, C.byref(f)))
        return f

    def set_flow_median(self, window=None, min_valid: int = 0) -> None:
        """NaN-aware median filter of the on-GPU flow estimator (mod_set_flow_median), off by default: behind every other step, each valid
        flow pixel becomes the per-component lower median of the valid pixels of its window x window square (window 3 or 5), or (NaN,
        NaN) where fewer than `min_valid` of them are valid; invalid pixels stay.  No argument or None turns it off; a
        capi.ModFlowMedian is taken as it is.  Read when a call or a submit enqueues the flow estimator."""
        if window is None:
            self._check(self.lib.mod_set_flow_median(self.h, None))
            return
        f = window if isinstance(window, capi.ModFlowMedian) else capi.flow_median(window, min_valid)
        self._check(self.lib.mod_set_flow_median(self.h, C.byref(f)))

    def get_flow_median(self) -> capi.ModFlowMedian:
        f = capi.ModFlowMedian(-1, -1, (-1, -1))
        self._check(self.lib.mod_get_flow_median(self.h, C.byref(f)))
        return f

    def set_flow_fill(self, window=None, min_valid: int = 3, tol_abs: float = 1.0, tol_rel: float = 0.0) -> None:
        """Disparity-gated hole fill of the flow in the submits that estimate it (mod_set_flow_fill), off by default: the last flow stage,
        behind the median and the ego-motion estimate and in front of the scene flow; an invalid flow pixel with a valid disparity d
        becomes the per-component lower median of the valid flow pixels of its window x window square (window 3, 5 or 7) whose disparity
        lies within tol_abs + tol_rel * d of d, where at least `min_valid` do.  No argument or None turns it off; a capi.ModFlowFill is
        taken as it is.  Read when a submit is made.  The defaults are not tuned."""
        if window is None:
            self._check(self.lib.mod_set_flow_fill(self.h, None))
            return
        f = window if isinstance(window, capi.ModFlowFill) else capi.flow_fill(window, min_valid, tol_abs, tol_rel)
        self._check(self.lib.mod_set_flow_fill(self.h, C.byref(f)))

    def get_flow_fill(self) -> capi.ModFlowFill:
        f = capi.ModFlowFill(-1, -1, -1.0, -1.0, (-1, -1))
        self._check(self.lib.mod_get_flow_fill(self.h, C.byref(f)))
        return f

    def set_cluster_members(self, ws: Optional[dict]) -> None:
        """Per-cluster member lists (mod_set_cluster_members), off by default: every later cluster() / process() and the synchronous
        host calls write offsets, indices (and points) into the tensors of `ws` (workspace(..., members=True)); None turns them off.
        The pipelined submits never write them.  The tensors must stay alive while the setting is on (the context keeps `ws`)."""
        if ws is None:
            self._check(self.lib.mod_set_cluster_members(self.h, None))
            self._members_ws = None
            return
        if ws.get("member_offsets") is None:
            raise ValueError("workspace(..., members=True) allocates the member-list tensors")
        pts = ws.get("member_points")
        m = capi.ModClusterMembers(ws["member_offsets"].data_ptr(), ws["member_indices"].data_ptr(), pts.data_ptr() if pts is not None else None, 0)
        self._check(self.lib.mod_set_cluster_members(self.h, C.byref(m)))
        self._members_ws = ws

    def get_cluster_members(self):
        """(ModClusterMembers in force, enabled)."""
        m, on = capi.ModClusterMembers(), C.c_int32(-1)
        self._check(self.lib.mod_get_cluster_members(self.h, C.byref(m), C.byref(on)))
        return m, bool(on.value)

    def set_cluster_image(self, ws: Optional[dict], host_image=None, palette=None) -> None:
        """The BGR8 cluster image (mod_set_cluster_image), off by default.  ws (workspace(..., image=True)): every later cluster() /
        process() draws all its frames into ws["image"].  host_image (a writable C-contiguous uint8 buffer of H * W * 3 bytes, e.g. a
        numpy array): the synchronous host calls and every submit write their frame there; a ticketed frame keeps the buffer and the
        table of its submit.  palette: a caller's (256, 3) B, G, R table, else the built-in one.  Both None: off.  The context keeps
        `ws` and `host_image` alive while the setting is on."""
        if ws is None and host_image is None:
            self._check(self.lib.mod_set_cluster_image(self.h, None))
            self._image_keep = None
            return
        if ws is not None and ws.get("image") is None:
            raise ValueError("workspace(..., image=True) allocates the image tensor")
        host = None
        if host_image is not None:
            view = memoryview(host_image)
            if view.readonly or not view.c_contiguous or view.nbytes < 3 * self.height * self.width:
                raise ValueError("host_image must be a writable C-contiguous buffer of H * W * 3 bytes")
            host = C.addressof((C.c_uint8 * view.nbytes).from_buffer(host_image))
        pal = capi.palette_bytes(palette)
        m = capi.ModClusterImage(ws["image"].data_ptr() if ws is not None else None, host, C.addressof(pal) if pal is not None else None, 0)
        self._check(self.lib.mod_set_cluster_image(self.h, C.byref(m)))
        self._image_keep = (ws, host_image)

    def get_cluster_image(self):
        """(ModClusterImage in force, enabled)."""
        m, on = capi.ModClusterImage(), C.c_int32(-1)
        self._check(self.lib.mod_get_cluster_image(self.h, C.byref(m), C.byref(on)))
        return m, bool(on.value)

    def render_clusters(self, labels: torch.Tensor, n_clusters: torch.Tensor, palette=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The renderer alone (mod_cluster_image_dev): device int32 labels (F, H, W) or (F, H * W) and int32 n_clusters (F,) ->
        (F, H, W, 3) uint8 B, G, R; labels outside [0, n_clusters[f]) are black.  Enqueued on the context's stream."""
        F = int(n_clusters.shape[0])
        if labels.dtype != torch.int32 or n_clusters.dtype != torch.int32 or labels.numel() != F * self.height * self.width:
            raise ValueError("render_clusters takes int32 labels of F * H * W elements and int32 n_clusters of F")
        labels, n_clusters = labels.contiguous(), n_clusters.contiguous()
        if out is None:
            out = torch.empty((F, self.height, self.width, 3), dtype=torch.uint8, device=labels.device)
        pal = capi.palette_bytes(palette)
        self._check(self.lib.mod_cluster_image_dev(self.h, F, labels.data_ptr(), n_clusters.data_ptr(), pal, out.data_ptr()))
        return out

    # ---- the constructor's views on device planes (mod_static_flow_dev, mod_flow_image_dev, ...) -----------------
    def _plane(self, t: torch.Tensor, per_pixel: int, what: str) -> int:
        """frames of a float32 device plane of per_pixel floats a pixel"""
        n = self.height * self.width * per_pixel
        if t.dtype != torch.float32 or t.numel() == 0 or t.numel() % n:
            raise ValueError(f"{what} takes float32 planes of F * H * W * {per_pixel} elements")
        return t.numel() // n

    def static_flow(self, disp_prev: torch.Tensor, transforms: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """calculateStaticOpticalFlow on device planes (mod_static_flow_dev): float32 disp_prev (F, H, W) and float64 device
        transforms (F, 7) (t[3] then q[4] x, y, z, w: ModTransform) -> (F, H, W, 2) float32, NaN where the reference leaves NaN."""
        F = self._plane(disp_prev, 1, "static_flow")
        if transforms.dtype != torch.float64 or transforms.numel() != 7 * F:
            raise ValueError("static_flow takes float64 transforms of F * 7 elements")
        disp_prev, transforms = disp_prev.contiguous(), transforms.contiguous()
        if out is None:
            out = torch.empty((F, self.height, self.width, 2), dtype=torch.float32, device=disp_prev.device)
        self._check(self.lib.mod_static_flow_dev(self.h, F, disp_prev.data_ptr(), transforms.data_ptr(), out.data_ptr()))
        return out

    def flow_image(self, flow: torch.Tensor, max_px: float, static: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The flow image (mod_flow_image_dev): float32 flow (F, H, W, 2) -> (F, H, W, 3) uint8 B, G, R; hue = direction, white at
        rest, full at max_px (capi.flow_color is its legend), black where a component is NaN or inf.  static (same shape) given: the
        image of flow - static (mod_flow_residual_image_dev).  Enqueued on the context's stream."""
        F = self._plane(flow, 2, "flow_image")
        if static is not None and (self._plane(static, 2, "flow_image") != F):
            raise ValueError("flow_image: flow and static differ in size")
        flow = flow.contiguous()
        if out is None:
            out = torch.empty((F, self.height, self.width, 3), dtype=torch.uint8, device=flow.device)
        if static is None:
            self._check(self.lib.mod_flow_image_dev(self.h, F, flow.data_ptr(), float(max_px), out.data_ptr()))
        else:
            static = static.contiguous()
            self._check(self.lib.mod_flow_residual_image_dev(self.h, F, flow.data_ptr(), static.data_ptr(), float(max_px), out.data_ptr()))
        return out

    def disparity_image(self, disp: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The disparity image (mod_disparity_image_dev): float32 disp (F, H, W) -> (F, H, W, 3) uint8 B, G, R over the camera's
        min_disparity .. max_disparity, black where getDisparity / getPoint3D reject the pixel."""
        F = self._plane(disp, 1, "disparity_image")
        disp = disp.contiguous()
        if out is None:
            out = torch.empty((F, self.height, self.width, 3), dtype=torch.uint8, device=disp.device)
        self._check(self.lib.mod_disparity_image_dev(self.h, F, disp.data_ptr(), out.data_ptr()))
        return out

    def set_flow_propagation(self, seeds: int = 1) -> None:
        """Neighbour-seed propagation of the on-GPU optical flow (mod_set_flow_propagation): 1 = off (the default), 5 = every finer
        level also tries the winners of the parent's four neighbours.  Takes effect for calls and submits made after it."""
        self._check(self.lib.mod_set_flow_propagation(self.h, int(seeds)))

    def get_flow_propagation(self) -> int:
        seeds = C.c_int32(-1)
        self._check(self.lib.mod_get_flow_propagation(self.h, C.byref(seeds)))
        return seeds.value

    def set_rectification(self, left: Optional[capi.ModRectifyCamera] = None, right: Optional[capi.ModRectifyCamera] = None) -> None:
        """Rectification of raw camera images on the GPU (mod_set_rectification): the calibrations of the two eyes
        (capi.rectify_camera), or neither = off (the default).  While set, the *_host image entry points take raw messages.  Refused
        while tickets are outstanding."""
        self._check(self.lib.mod_set_rectification(self.h, C.byref(left) if left is not None else None,
                                                   C.byref(right) if right is not None else None))

    def get_rectification(self):
        """(left, right) ModRectifyCamera of the rectification in force, or None while it is off."""
        l, r, on = capi.ModRectifyCamera(), capi.ModRectifyCamera(), C.c_int32(-1)
        self._check(self.lib.mod_get_rectification(self.h, C.byref(l), C.byref(r), C.byref(on)))
        return (l, r) if on.value else None

    def set_distortion_model(self, model) -> None:
        """How the rectification reads D (mod_set_distortion_model): capi.MOD_DISTORTION_RATIONAL (the default) or
        capi.MOD_DISTORTION_EQUIDISTANT, or a CameraInfo's string ("plumb_bob", "rational_polynomial", "equidistant").  Both eyes';
        refused while tickets are outstanding."""
        self._check(self.lib.mod_set_distortion_model(self.h, capi.distortion_model(model)))

    def get_distortion_model(self) -> int:
        model = C.c_int32(-1)
        self._check(self.lib.mod_get_distortion_model(self.h, C.byref(model)))
        return model.value

    def set_side_by_side(self, on) -> None:
        """Side-by-side stereo messages (mod_set_side_by_side): while on, one message holds both eyes, the layout's width is one eye's
        and its step the whole row's (>= 2 * width * channels); the stereo *_host entry points take it in `left`.  Off by default; read
        when a call or a submit is made."""
        self._check(self.lib.mod_set_side_by_side(self.h, int(bool(on)) if isinstance(on, (bool, np.bool_)) else int(on)))

    def get_side_by_side(self) -> bool:
        on = C.c_int32(-1)
        self._check(self.lib.mod_get_side_by_side(self.h, C.byref(on)))
        return bool(on.value)

    def set_image_binning(self, bx: int = 1, by: int = 1, mode=capi.MOD_BIN_MEAN) -> None:
        """Bin the camera images on the GPU at ingest (mod_set_image_binning, image_proc/crop_decimate's step): every image entry point
        takes a (bx W) x (by H) window of its messages and reduces it to the context's W x H, `mode` capi.MOD_BIN_MEAN ("mean", the
        rounded box mean) or capi.MOD_BIN_NEAREST ("nearest", the block's top-left pixel).  No arguments = off (the default).  The
        camera given to set_camera is the binned one (capi.binned_camera).  Read when a call or a submit is made."""
        b = capi.image_binning(bx, by, mode)
        self._check(self.lib.mod_set_image_binning(self.h, C.byref(b)))

    def get_image_binning(self) -> capi.ModImageBinning:
        b = capi.ModImageBinning()
        self._check(self.lib.mod_get_image_binning(self.h, C.byref(b)))
        return b

    def set_depth_layout(self, layout: Optional[capi.ModDepthLayout]) -> None:
        """Layout of the depth messages of an RGB-D camera (mod_set_depth_layout, capi.depth_layout); None = 16UC1 packed at the camera
        size.  Read when a call or a submit is made."""
        self._check(self.lib.mod_set_depth_layout(self.h, C.byref(layout) if layout is not None else None))

    def get_depth_layout(self) -> capi.ModDepthLayout:
        s = capi.ModDepthLayout()
        self._check(self.lib.mod_get_depth_layout(self.h, C.byref(s)))
        return s

    def set_depth_registration(self, registration: Optional[capi.ModDepthRegistration] = None) -> None:
        """Registration of the depth camera to the image camera on the GPU (mod_set_depth_registration, capi.depth_registration); None =
        off (the default: the depth image is aligned to the image already).  Set it before a depth layout of another size than the
        camera's."""
        self._check(self.lib.mod_set_depth_registration(self.h, C.byref(registration) if registration is not None else None))

    def get_depth_registration(self):
        """The ModDepthRegistration in force, or None while it is off."""
        r, on = capi.ModDepthRegistration(), C.c_int32(-1)
        self._check(self.lib.mod_get_depth_registration(self.h, C.byref(r), C.byref(on)))
        return r if on.value else None

    def set_depth_splat(self, on: bool = True) -> None:
        """Fill the holes a depth camera of fewer pixels than the image camera leaves in the registered path (mod_set_depth_splat):
        every depth sample paints the image pixels inside its projected footprint, at most capi.MOD_DEPTH_SPLAT_MAX per axis, not its
        centre alone.  Off by default; without a registration it has no effect.  Read when a call or a submit is made."""
        self._check(self.lib.mod_set_depth_splat(self.h, int(on)))

    def get_depth_splat(self) -> bool:
        on = C.c_int32(-1)
        self._check(self.lib.mod_get_depth_splat(self.h, C.byref(on)))
        return bool(on.value)

    def set_depth_distortion(self, d: Optional[capi.ModDepthDistortion] = None) -> None:
        """Lens model of the depth camera (mod_set_depth_distortion, capi.depth_distortion): the registered path back-projects every
        sample along its undistorted ray, from a table built on the GPU, instead of a pinhole's; None = off (the default).  Needs a
        registration (aligned cameras: identity pose and the depth intrinsics).  Refused while a distortion is set and tickets are
        outstanding."""
        self._check(self.lib.mod_set_depth_distortion(self.h, C.byref(d) if d is not None else None))

    def get_depth_distortion(self):
        """The ModDepthDistortion in force, or None while it is off."""
        d, on = capi.ModDepthDistortion(), C.c_int32(-1)
        self._check(self.lib.mod_get_depth_distortion(self.h, C.byref(d), C.byref(on)))
        return d if on.value else None

    def depth_rays(self, layout: Optional[capi.ModDepthLayout] = None, lattice: int = capi.MOD_DEPTH_RAYS_CENTRES) -> np.ndarray:
        """The ray table the registration kernels read (mod_depth_rays_host): (h, w, 2) float64 for the pixel centres of the layout's
        message (None = the context's), (h + 1, w + 1, 2) for capi.MOD_DEPTH_RAYS_CORNERS, entry [j][i] the ray of (i - 0.5, j - 0.5);
        NaN where the lens has no inverse.  Synchronises the context's stream."""
        lay = layout if layout is not None else self.get_depth_layout()
        k = 1 if int(lattice) == capi.MOD_DEPTH_RAYS_CORNERS else 0
        out = np.empty((lay.height + k, lay.width + k, 2), np.float64)
        self._check(self.lib.mod_depth_rays_host(self.h, C.byref(layout) if layout is not None else None, int(lattice), out.ctypes.data))
        return out

    def depth_to_disparity(self, dev: torch.Tensor, layout: Optional[capi.ModDepthLayout] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Disparity planes (F, H, W) float32 at the camera size from device depth messages (mod_depth_to_disparity_dev): `dev` holds F
        messages of layout.step * layout.height bytes each, back to back (any dtype and shape, contiguous); layout None = the context's.
        fT / depth where the depth is positive and finite, min_disparity - 1 elsewhere; with a registration set the messages are
        registered to the image camera first (set_depth_splat: with their footprints).  Enqueued on the context's stream."""
        lay = layout if layout is not None else self.get_depth_layout()
        F, out = self._whole_messages(dev, lay, out, torch.float32, "dev", "messages")
        self._done(self.lib.mod_depth_to_disparity_dev(self.h, F, dev.data_ptr(), C.byref(lay), out.data_ptr()), "mod_depth_to_disparity_dev")
        return out

    def set_depth_filter(self, filter: Optional[capi.ModDepthFilter] = None) -> None:   # noqa: A002 (the ABI's name)
        """Range and flying-pixel filter of the depth messages, on the depth camera's own lattice ahead of everything else
        (mod_set_depth_filter, capi.depth_filter); None = off (the default).  Read when a call or a submit is made; a ticket in
        flight keeps the filter of its submit."""
        self._check(self.lib.mod_set_depth_filter(self.h, C.byref(filter) if filter is not None else None))

    def get_depth_filter(self) -> capi.ModDepthFilter:
        """The ModDepthFilter in force; all zeros while it is off."""
        f = capi.ModDepthFilter()
        self._check(self.lib.mod_get_depth_filter(self.h, C.byref(f)))
        return f

    def depth_filter(self, dev_depth: torch.Tensor, layout: Optional[capi.ModDepthLayout] = None, filter: Optional[capi.ModDepthFilter] = None,  # noqa: A002
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The filter stage alone (mod_depth_filter_dev): `dev_depth` holds F whole messages of layout.step * layout.height bytes each,
        back to back (any dtype and shape, contiguous); the result has its dtype and shape, samples a rule removed set to "no reading"
        (0 for 16UC1, NaN for 32FC1), everything else bit for bit; bytes of a row beyond `width` samples are not defined.  layout None =
        the context's, filter None = the context's (off: a copy).  Not in place.  Enqueued on the context's stream."""
        lay = layout if layout is not None else self.get_depth_layout()
        if not dev_depth.is_contiguous() or dev_depth.device.type != "cuda":
            raise ValueError("dev_depth must be a contiguous device tensor")
        frame, nbytes = lay.step * lay.height, dev_depth.numel() * dev_depth.element_size()
        if frame <= 0 or nbytes % frame:
            raise ValueError("dev_depth must hold whole messages of step * height bytes")
        if out is None:
            out = torch.empty_like(dev_depth)
        elif out.shape != dev_depth.shape or out.dtype != dev_depth.dtype or not out.is_contiguous() or out.device != dev_depth.device:
            raise ValueError("out must be a contiguous device tensor of dev_depth's shape and dtype")
        self._done(self.lib.mod_depth_filter_dev(self.h, nbytes // frame, dev_depth.data_ptr(), C.byref(lay),
                                                 C.byref(filter) if filter is not None else None, out.data_ptr()), "mod_depth_filter_dev")
        return out

    def set_depth_spatial(self, spatial: Optional[capi.ModDepthSpatial] = None) -> None:
        """Edge-preserving smoother and hole fill of the depth messages, behind the depth filter and in front of the temporal filter
        (mod_set_depth_spatial, capi.depth_spatial); None or window = 0: off (the default).  Read when a call or a submit is made; a
        ticket in flight keeps the setting of its submit."""
        self._check(self.lib.mod_set_depth_spatial(self.h, C.byref(spatial) if spatial is not None else None))

    def get_depth_spatial(self) -> capi.ModDepthSpatial:
        """The ModDepthSpatial in force; all zeros while it is off."""
        s = capi.ModDepthSpatial()
        self._check(self.lib.mod_get_depth_spatial(self.h, C.byref(s)))
        return s

    def depth_spatial(self, dev_depth: torch.Tensor, layout: Optional[capi.ModDepthLayout] = None, spatial: Optional[capi.ModDepthSpatial] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The spatial stage alone (mod_depth_spatial_dev): `dev_depth` holds F whole messages of layout.step * layout.height bytes each,
        back to back (any dtype and shape, contiguous); the result has its dtype and shape: smoothed samples, filled holes, everything
        else bit for bit; bytes of a row beyond `width` samples are not defined.  layout None = the context's, spatial None = the
        context's (off: a copy).  Not in place.  Enqueued on the context's stream."""
        lay = layout if layout is not None else self.get_depth_layout()
        if not dev_depth.is_contiguous() or dev_depth.device.type != "cuda":
            raise ValueError("dev_depth must be a contiguous device tensor")
        frame, nbytes = lay.step * lay.height, dev_depth.numel() * dev_depth.element_size()
        if frame <= 0 or nbytes % frame:
            raise ValueError("dev_depth must hold whole messages of step * height bytes")
        if out is None:
            out = torch.empty_like(dev_depth)
        elif out.shape != dev_depth.shape or out.dtype != dev_depth.dtype or not out.is_contiguous() or out.device != dev_depth.device:
            raise ValueError("out must be a contiguous device tensor of dev_depth's shape and dtype")
        self._done(self.lib.mod_depth_spatial_dev(self.h, nbytes // frame, dev_depth.data_ptr(), C.byref(lay),
                                                  C.byref(spatial) if spatial is not None else None, out.data_ptr()), "mod_depth_spatial_dev")
        return out

    def set_depth_decimation(self, d: Optional[capi.ModDepthDecimation] = None) -> None:
        """Decimation of the depth messages by integer factors, the last stage in front of the conversion (mod_set_depth_decimation,
        capi.depth_decimation); None or dx = dy = 1: off (the default).  The window taken from a depth message is then (dx W) x (dy H).
        Read when a call or a submit is made; a ticket in flight keeps the setting of its submit.  Not with a registration."""
        self._check(self.lib.mod_set_depth_decimation(self.h, C.byref(d) if d is not None else None))

    def get_depth_decimation(self) -> capi.ModDepthDecimation:
        """The ModDepthDecimation in force; dx = dy = 1 while it is off."""
        d = capi.ModDepthDecimation()
        self._check(self.lib.mod_get_depth_decimation(self.h, C.byref(d)))
        return d

    def depth_decimate(self, dev_depth: torch.Tensor, layout: Optional[capi.ModDepthLayout] = None, decimation: Optional[capi.ModDepthDecimation] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The decimation stage alone (mod_depth_decimate_dev): `dev_depth` holds F whole messages of layout.step * layout.height bytes
        each, back to back (any dtype and shape, contiguous).  The blocks start at the layout's (x0, y0); the result is (F, out_h, out_w)
        packed samples, uint16 for 16UC1 and the words as uint32 for 32FC1 (`.view(torch.float32)` reads them), with
        out_w = (width - x0) // dx and out_h = (height - y0) // dy.  layout None = the context's, decimation None = the context's (off: a
        copy of the window).  Not in place.  Enqueued on the context's stream."""
        lay = layout if layout is not None else self.get_depth_layout()
        d = decimation if decimation is not None else self.get_depth_decimation()
        if not dev_depth.is_contiguous() or dev_depth.device.type != "cuda":
            raise ValueError("dev_depth must be a contiguous device tensor")
        frame, nbytes = lay.step * lay.height, dev_depth.numel() * dev_depth.element_size()
        if frame <= 0 or nbytes % frame:
            raise ValueError("dev_depth must hold whole messages of step * height bytes")
        F = nbytes // frame
        shape = (F, (lay.height - lay.y0) // max(d.dy, 1), (lay.width - lay.x0) // max(d.dx, 1))
        dtype = torch.uint16 if lay.encoding == capi.MOD_DEPTH_16UC1 else torch.uint32
        if out is None:
            out = torch.empty([max(n, 0) for n in shape], dtype=dtype, device=dev_depth.device)
        elif out.numel() * out.element_size() != shape[0] * shape[1] * shape[2] * capi.DEPTH_BYTES.get(lay.encoding, 0) or not out.is_contiguous() \
                or out.device != dev_depth.device:
            raise ValueError("out must be a contiguous device tensor of F * out_h * out_w samples")
        self._done(self.lib.mod_depth_decimate_dev(self.h, F, dev_depth.data_ptr(), C.byref(lay),
                                                   C.byref(decimation) if decimation is not None else None, out.data_ptr()), "mod_depth_decimate_dev")
        return out

    def set_depth_temporal(self, filter: Optional[capi.ModDepthTemporal] = None) -> None:   # noqa: A002 (the ABI's name)
        """Temporal filter with hold of the depth messages, behind the depth filter and ahead of everything else
        (mod_set_depth_temporal, capi.depth_temporal); None or alpha = 0: off (the default).  Every call empties the context's state.
        Read when a call or a submit is made; a ticket in flight keeps the parameters of its submit."""
        self._check(self.lib.mod_set_depth_temporal(self.h, C.byref(filter) if filter is not None else None))

    def get_depth_temporal(self) -> capi.ModDepthTemporal:
        """The ModDepthTemporal in force; all zeros while it is off."""
        f = capi.ModDepthTemporal()
        self._check(self.lib.mod_get_depth_temporal(self.h, C.byref(f)))
        return f

    def reset_depth_temporal(self) -> None:
        """Empties the temporal filter's state in the context (mod_reset_depth_temporal): the next frame starts every pixel anew."""
        self._check(self.lib.mod_reset_depth_temporal(self.h))

    def depth_temporal(self, dev_depth: torch.Tensor, layout: Optional[capi.ModDepthLayout] = None, filter: Optional[capi.ModDepthTemporal] = None,  # noqa: A002
                       state: Optional[tuple] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The temporal stage alone (mod_depth_temporal_dev): `dev_depth` holds F consecutive whole messages of layout.step *
        layout.height bytes each, oldest first (any dtype and shape, contiguous); the result has its dtype and shape; bytes of a row
        beyond `width` samples are not defined.  state = (s, age): contiguous device tensors of height * width float32 and uint8,
        updated in place (age filled with 255: empty); None = the context's state.  layout None = the context's, filter None = the
        context's (off: a copy).  out may be dev_depth itself.  Enqueued on the context's stream."""
        lay = layout if layout is not None else self.get_depth_layout()
        if not dev_depth.is_contiguous() or dev_depth.device.type != "cuda":
            raise ValueError("dev_depth must be a contiguous device tensor")
        frame, nbytes = lay.step * lay.height, dev_depth.numel() * dev_depth.element_size()
        if frame <= 0 or nbytes % frame:
            raise ValueError("dev_depth must hold whole messages of step * height bytes")
        if out is None:
            out = torch.empty_like(dev_depth)
        elif out.shape != dev_depth.shape or out.dtype != dev_depth.dtype or not out.is_contiguous() or out.device != dev_depth.device:
            raise ValueError("out must be a contiguous device tensor of dev_depth's shape and dtype")
        ps = pa = None
        if state is not None:
            s, age = state
            n = lay.width * lay.height
            for t, dt in ((s, torch.float32), (age, torch.uint8)):
                if t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != dev_depth.device:
                    raise ValueError("state must be (float32, uint8) contiguous device tensors of height * width elements")
            ps, pa = s.data_ptr(), age.data_ptr()
        self._done(self.lib.mod_depth_temporal_dev(self.h, nbytes // frame, dev_depth.data_ptr(), C.byref(lay),
                                                   C.byref(filter) if filter is not None else None, ps, pa, out.data_ptr()), "mod_depth_temporal_dev")
        return out

    def _whole_messages(self, t: torch.Tensor, lay, out: Optional[torch.Tensor], out_dtype, name: str, unit: str):
        """(F, out) for a contiguous device tensor `t` holding F whole messages of lay.step * lay.height bytes (uint8 where the output
        is; any dtype for depth) and the (F, H, W) tensor the call writes, `out` or a new one."""
        u8 = out_dtype == torch.uint8
        if (u8 and t.dtype != torch.uint8) or not t.is_contiguous() or t.device.type != "cuda":
            raise ValueError(f"{name} must be a contiguous {'uint8 ' if u8 else ''}device tensor")
        frame, nbytes = lay.step * lay.height, t.numel() * t.element_size()
        if frame <= 0 or nbytes % frame:
            raise ValueError(f"{name} must hold whole {unit} of step * height bytes")
        F = nbytes // frame
        if out is None:
            out = torch.empty((F, self.height, self.width), dtype=out_dtype, device=t.device)
        elif out.shape != (F, self.height, self.width) or out.dtype != out_dtype or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {str(out_dtype)[6:]} tensor (F, H, W)")
        return F, out

    def speckle_filter(self, dev_planes: torch.Tensor, size: int, range: int) -> torch.Tensor:   # noqa: A002 (stereo_image_proc's name)
        """The speckle stage alone, in place (mod_disparity_speckle_dev), on device float32 planes (F, H, W) or (H, W) of the camera's
        size: pixels take part when finite and >= the camera's min_disparity, removed ones become min_disparity - 1.  Enqueued on the
        context's stream; returns `dev_planes`."""
        p = dev_planes[None] if dev_planes.dim() == 2 else dev_planes
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device.type != "cuda" or p.shape[1:] != (self.height, self.width):
            raise ValueError("dev_planes must be a contiguous float32 device tensor (F, H, W) at the camera size")
        self._done(self.lib.mod_disparity_speckle_dev(self.h, p.shape[0], p.data_ptr(), int(size), int(range)), "mod_disparity_speckle_dev")
        return dev_planes

    def disparity_fill(self, planes: torch.Tensor, fill: Optional[capi.ModDisparityFill] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The occlusion hole fill alone (mod_disparity_fill_dev) on device float32 planes (F, H, W) or (H, W) of the camera's size, into
        `out` (another tensor of the planes' size; a new one when None) — returned as (F, H, W).  A word is valid when finite and >= the
        camera's min_disparity.  fill None = the context's; reach 0 is refused.  Enqueued on the context's stream."""
        p = planes[None] if planes.dim() == 2 else planes
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device.type != "cuda" or p.shape[1:] != (self.height, self.width):
            raise ValueError("planes must be a contiguous float32 device tensor (F, H, W) at the camera size")
        if out is None:
            out = torch.empty_like(p)
        elif out.numel() != p.numel() or out.shape[-2:] != p.shape[-2:] or out.dtype != torch.float32 or not out.is_contiguous() or out.device != p.device:
            raise ValueError("out must be a contiguous float32 tensor of the planes' size on their device")
        self._done(self.lib.mod_disparity_fill_dev(self.h, p.shape[0], p.data_ptr(), C.byref(fill) if fill is not None else None, out.data_ptr()),
                   "mod_disparity_fill_dev")
        return out.view(p.shape)

    def disparity_smooth(self, planes: torch.Tensor, smooth: Optional[capi.ModDisparitySmooth] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The edge-preserving smoother alone (mod_disparity_smooth_dev) on device float32 planes (F, H, W) or (H, W) of the camera's
        size, into `out` (another tensor of the planes' size; a new one when None) — returned as (F, H, W).  A word is valid when finite
        and >= the camera's min_disparity.  smooth None = the context's; with none set the call is refused.  Enqueued on the context's
        stream."""
        p = planes[None] if planes.dim() == 2 else planes
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device.type != "cuda" or p.shape[1:] != (self.height, self.width):
            raise ValueError("planes must be a contiguous float32 device tensor (F, H, W) at the camera size")
        if out is None:
            out = torch.empty_like(p)
        elif out.numel() != p.numel() or out.shape[-2:] != p.shape[-2:] or out.dtype != torch.float32 or not out.is_contiguous() or out.device != p.device:
            raise ValueError("out must be a contiguous float32 tensor of the planes' size on their device")
        self._done(self.lib.mod_disparity_smooth_dev(self.h, p.shape[0], p.data_ptr(), C.byref(smooth) if smooth is not None else None, out.data_ptr()),
                   "mod_disparity_smooth_dev")
        return out.view(p.shape)

    def _grey_planes(self, grey: torch.Tensor) -> torch.Tensor:
        g = grey[None] if grey.dim() == 2 else grey
        if g.dtype != torch.uint8 or not g.is_contiguous() or g.device.type != "cuda" or g.shape[1:] != (self.height, self.width):
            raise ValueError("grey must be a contiguous uint8 device tensor (F, H, W) at the camera size")
        return g

    def texture(self, grey: torch.Tensor, filter: Optional[capi.ModTextureFilter] = None,   # noqa: A002 (the header's name)
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The texture sum T of device grey planes (F, H, W) or (H, W) (mod_texture_dev) as uint16 of the same shape: what one looks at to
        choose a threshold.  filter None = the context's (only window and cap are used).  Enqueued on the context's stream."""
        g = self._grey_planes(grey)
        if out is None:
            out = torch.empty(g.shape, dtype=torch.uint16, device=g.device)
        elif out.shape not in (g.shape, grey.shape) or out.dtype != torch.uint16 or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint16 tensor of grey's shape")
        self._done(self.lib.mod_texture_dev(self.h, g.shape[0], g.data_ptr(), C.byref(filter) if filter is not None else None, out.data_ptr()),
                   "mod_texture_dev")
        return out[0] if grey.dim() == 2 and out.dim() == 3 else out

    def texture_reject(self, grey: Optional[torch.Tensor], disparity: Optional[torch.Tensor] = None, flow: Optional[torch.Tensor] = None,
                       filter: Optional[capi.ModTextureFilter] = None) -> int:   # noqa: A002
        """The texture rule alone, in place (mod_texture_reject_dev), on a caller's own device planes: where T of `grey` is below the
        threshold, `disparity` (F, H, W) float32 becomes the camera's min_disparity - 1 and `flow` (F, H, W, 2) float32 (NaN, NaN); either
        may be None.  filter None = the context's.  Returns the library's code: 0, or the skip code when there is no grey or no plane."""
        F = None
        if grey is not None:
            grey = self._grey_planes(grey)
            F = grey.shape[0]
        for name, t, tail in (("disparity", disparity, ()), ("flow", flow, (2,))):
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != "cuda" or t.shape[-len(tail) - 2:] != (self.height, self.width) + tail:
                raise ValueError(f"{name} must be a contiguous float32 device tensor (F, H, W{', 2' if tail else ''}) at the camera size")
            n = t.numel() // (self.height * self.width * (2 if tail else 1))
            if F is not None and n != F:
                raise ValueError(f"{name} must hold as many frames as grey")
            F = n if F is None else F
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        return self._check(self.lib.mod_texture_reject_dev(self.h, F or 1, ptr(grey), C.byref(filter) if filter is not None else None,
                                                           ptr(disparity), ptr(flow)))

    def flow_corner(self, grey: torch.Tensor, filter: Optional[capi.ModCornerFilter] = None,   # noqa: A002 (the header's name)
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The min-eigenvalue strength E of device grey planes (F, H, W) or (H, W) (mod_flow_corner_dev) as int32 of the same shape (E <=
        capi.MOD_CORNER_MAX, so the uint32 the library writes reads the same as int32; `out` may be int32 or uint32): what one looks at
        to choose a threshold.  filter None = the context's (only window and cap are used).  Enqueued on the context's stream."""
        g = self._grey_planes(grey)
        if out is None:
            out = torch.empty(g.shape, dtype=torch.int32, device=g.device)
        elif out.shape not in (g.shape, grey.shape) or out.dtype not in (torch.int32, torch.uint32) or not out.is_contiguous():
            raise ValueError("out must be a contiguous int32 or uint32 tensor of grey's shape")
        self._done(self.lib.mod_flow_corner_dev(self.h, g.shape[0], g.data_ptr(), C.byref(filter) if filter is not None else None,
                                                out.data_ptr()), "mod_flow_corner_dev")
        return out[0] if grey.dim() == 2 and out.dim() == 3 else out

    def flow_corner_reject(self, grey: Optional[torch.Tensor], flow: Optional[torch.Tensor],
                           filter: Optional[capi.ModCornerFilter] = None) -> int:   # noqa: A002
        """The min-eigenvalue rule alone, in place (mod_flow_corner_reject_dev), on a caller's own device flow (F, H, W, 2) float32: where
        E of `grey` is below the threshold the pixel becomes (NaN, NaN).  filter None = the context's.  Returns the library's code: 0,
        or the skip code when there is no grey or no flow."""
        F = None
        if grey is not None:
            grey = self._grey_planes(grey)
            F = grey.shape[0]
        if flow is not None:
            if flow.dtype != torch.float32 or not flow.is_contiguous() or flow.device.type != "cuda" or flow.shape[-3:] != (self.height, self.width, 2):
                raise ValueError("flow must be a contiguous float32 device tensor (F, H, W, 2) at the camera size")
            n = flow.numel() // (self.height * self.width * 2)
            if F is not None and n != F:
                raise ValueError("flow must hold as many frames as grey")
            F = n
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        return self._check(self.lib.mod_flow_corner_reject_dev(self.h, F or 1, ptr(grey), C.byref(filter) if filter is not None else None,
                                                               ptr(flow)))

    def flow_median(self, flow: torch.Tensor, filter: Optional[capi.ModFlowMedian] = None,   # noqa: A002 (the header's name)
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The NaN-aware median filter alone (mod_flow_median_dev) on a device flow (F, H, W, 2) or (H, W, 2) float32 at the camera size,
        into `out` (another tensor of the same size; a new one when None) — returned as (F, H, W, 2).  filter None = the context's;
        window 0 is refused.  Enqueued on the context's stream."""
        if flow.dtype != torch.float32 or not flow.is_contiguous() or flow.device.type != "cuda" or flow.shape[-3:] != (self.height, self.width, 2):
            raise ValueError("flow must be a contiguous float32 device tensor (F, H, W, 2) at the camera size")
        F = flow.numel() // (self.height * self.width * 2)
        if out is None:
            out = torch.empty((F, self.height, self.width, 2), dtype=torch.float32, device=flow.device)
        elif out.numel() != flow.numel() or out.shape[-3:] != flow.shape[-3:] or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor of flow's size")
        self._done(self.lib.mod_flow_median_dev(self.h, F, flow.data_ptr(), C.byref(filter) if filter is not None else None, out.data_ptr()),
                   "mod_flow_median_dev")
        return out.view(F, self.height, self.width, 2)

    def flow_fill(self, flow: torch.Tensor, disparity: torch.Tensor, fill: Optional[capi.ModFlowFill] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The disparity-gated hole fill alone (mod_flow_fill_dev) on a device flow (F, H, W, 2) or (H, W, 2) float32 and the disparity
        planes (F, H, W) or (H, W) float32 of the same frames, at the camera size, into `out` (another tensor of the flow's size; a new
        one when None) — returned as (F, H, W, 2).  fill None = the context's; window 0 is refused.  Enqueued on the context's stream."""
        if flow.dtype != torch.float32 or not flow.is_contiguous() or flow.device.type != "cuda" or flow.shape[-3:] != (self.height, self.width, 2):
            raise ValueError("flow must be a contiguous float32 device tensor (F, H, W, 2) at the camera size")
        F = flow.numel() // (self.height * self.width * 2)
        if (disparity.dtype != torch.float32 or not disparity.is_contiguous() or disparity.device != flow.device
                or disparity.shape[-2:] != (self.height, self.width) or disparity.numel() != F * self.height * self.width):
            raise ValueError("disparity must be a contiguous float32 tensor (F, H, W) on the flow's device, with the flow's frames")
        if out is None:
            out = torch.empty((F, self.height, self.width, 2), dtype=torch.float32, device=flow.device)
        elif out.numel() != flow.numel() or out.shape[-3:] != flow.shape[-3:] or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor of flow's size")
        self._done(self.lib.mod_flow_fill_dev(self.h, F, flow.data_ptr(), disparity.data_ptr(), C.byref(fill) if fill is not None else None,
                                              out.data_ptr()), "mod_flow_fill_dev")
        return out.view(F, self.height, self.width, 2)

    def pinned_copy(self, array) -> "PinnedBuffer":
        """A copy of `array` in page-locked host memory (mod_host_malloc): .ptr, .nbytes, .array (a numpy view of the copy); the submit
        methods of host_stream.HostStream take it where they take an array.  Freed by .free() or by close()."""
        a = np.ascontiguousarray(array)
        p = C.c_void_p()
        self._check(self.lib.mod_host_malloc(self.h, a.nbytes, C.byref(p)))
        buf = PinnedBuffer(self, p.value, a.nbytes)
        buf.array = np.frombuffer((C.c_uint8 * a.nbytes).from_address(p.value), dtype=a.dtype).reshape(a.shape)
        buf.array[...] = a
        self._pinned.append(buf)
        return buf

    def close(self) -> None:
        if getattr(self, "h", None):
            for buf in list(self._pinned):
                buf.free()
            self.lib.mod_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- buffers ----------------------------------------------------------------------------------------------
    def workspace(self, frames: int, aos: bool = False, extras: bool = False, labels: bool = True, xy: bool = True, members: bool = False,
                  points: bool = False, image: bool = False) -> dict:
        """Output buffers for `frames` frames, allocated once and reused.  labels=False: no cluster-label plane (the reference
        renders its cluster image only for subscribers, clusterer_nodelet.cpp:235-236).  xy=False: process() hands the library no x / y
        planes (nobody takes the cloud, scene_flow_constructor.cpp:141-142): the rows 0 and 1 of `planes` are then never written.
        members=True: the tensors of the per-cluster member lists (set_cluster_members(ws) turns them on), points=True: their x, y, z too.
        image=True: the (F, H, W, 3) uint8 tensor of the cluster image (set_cluster_image(ws) turns it on; it needs labels=True)."""
        members = members or points
        key = (frames, self.height, self.width, aos, extras, labels, xy, members, points, image)
        if self._ws is not None and self._ws["key"] == key:
            return self._ws
        H, W, dev = self.height, self.width, self.device
        ws = {"key": key, "xy": xy}
        per = frames * H * W                             # six planes from one block, bases staggered (see PLANE_STAGGER_BYTES)
        skew = PLANE_STAGGER_BYTES // 4
        ws["planes"] = torch.empty(6 * per + 5 * skew, dtype=torch.float32, device=dev).as_strided((6, frames, H, W), (per + skew, H * W, W, 1))
        ws["mask"] = torch.empty((frames, H, self.mask_words), dtype=torch.int64, device=dev)
        ws["labels"] = torch.empty((frames, H, W), dtype=torch.int32, device=dev) if labels else None
        ws["objects"] = torch.zeros((frames, self.max_objects, capi.MOD_OBJECT_BYTES), dtype=torch.uint8, device=dev)
        ws["n_objects"] = torch.zeros((frames,), dtype=torch.int32, device=dev)
        ws["n_clusters"] = torch.zeros((frames,), dtype=torch.int32, device=dev)
        ws["aos"] = torch.empty((frames, H, W, 8), dtype=torch.float32, device=dev) if aos else None
        ws["depth"] = torch.empty((frames, H, W), dtype=torch.float32, device=dev) if extras else None
        ws["static_flow"] = torch.empty((frames, H, W, 2), dtype=torch.float32, device=dev) if extras else None
        ws["member_offsets"] = torch.zeros((frames, self.max_objects + 1), dtype=torch.int32, device=dev) if members else None
        ws["member_indices"] = torch.empty((frames, H * W), dtype=torch.int32, device=dev) if members else None
        ws["member_points"] = torch.empty((frames, H * W, 3), dtype=torch.float32, device=dev) if points else None
        ws["image"] = torch.empty((frames, H, W, 3), dtype=torch.uint8, device=dev) if image else None
        self._ws = ws
        return ws

    def _planes_struct(self, ws, with_mask=True) -> capi.ModSceneFlowPlanes:
        p = ws["planes"]
        s = capi.ModSceneFlowPlanes()
        for i, k in enumerate(PLANES):
            setattr(s, k, p[i].data_ptr() if (ws.get("xy", True) or k not in ("x", "y")) else None)
        s.dynamic_mask = ws["mask"].data_ptr() if with_mask else None
        s.cloud_aos = ws["aos"].data_ptr() if ws.get("aos") is not None else None
        s.depth = ws["depth"].data_ptr() if ws.get("depth") is not None else None
        s.static_flow = ws["static_flow"].data_ptr() if ws.get("static_flow") is not None else None
        return s

    @staticmethod
    def _cluster_struct(ws) -> capi.ModClusterOut:
        return capi.ModClusterOut(ws["labels"].data_ptr() if ws["labels"] is not None else None, ws["objects"].data_ptr(), ws["n_objects"].data_ptr(),
                                  ws["n_clusters"].data_ptr())

    def make_batch(self, d_now: torch.Tensor, d_prev: Optional[torch.Tensor], flow: Optional[torch.Tensor], ts, qs, dts):
        """ModFrameBatch over device tensors (F,H,W), (F,H,W), (F,H,W,2) + host transforms.  Keeps references alive."""
        F = d_now.shape[0]
        b = capi.ModFrameBatch()
        b.frames = F
        b.disparity_now = d_now.data_ptr()
        b.disparity_prev = d_prev.data_ptr() if d_prev is not None else None
        b.flow = flow.data_ptr() if flow is not None else None
        tr = capi.transforms_array(ts, qs) if ts is not None else None
        dt = (C.c_double * F)(*[float(v) for v in dts]) if dts is not None else None
        b.transforms = tr
        b.dt = dt
        b._keep = (d_now, d_prev, flow, tr, dt)
        return b

    # ---- hot path ---------------------------------------------------------------------------------------------
    def scene_flow(self, batch, ws) -> int:
        return self._check(self.lib.mod_scene_flow_dev(self.h, C.byref(batch), C.byref(self._planes_struct(ws))))

    def cluster(self, frames: int, ws, mask_ready: bool) -> int:
        pl = self._planes_struct(ws, with_mask=mask_ready)
        return self._check(self.lib.mod_cluster_dev(self.h, frames, C.byref(pl), C.byref(self._cluster_struct(ws))))

    def process(self, batch, ws) -> int:
        return self._check(self.lib.mod_process_dev(self.h, C.byref(batch), C.byref(self._planes_struct(ws)),
                                                    C.byref(self._cluster_struct(ws))))

    def estimate_flow(self, prev: torch.Tensor, now: torch.Tensor, params: Optional[capi.ModFlowParams] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """On-GPU optical flow (mod_flow_compute_dev) from `prev` to `now`: device uint8 tensors (F,H,W) or (H,W) of the camera size.
        Returns (F,H,W,2) / (H,W,2) float32 indexed at the now pixel, prev = now - flow (NaN where the forward-backward check fails).
        Enqueued on the context's stream."""
        single = now.dim() == 2
        p4, n4 = (prev[None], now[None]) if single else (prev, now)
        if p4.shape != n4.shape or p4.dtype != torch.uint8 or n4.dtype != torch.uint8 or p4.shape[1:] != (self.height, self.width):
            raise ValueError("prev / now must be uint8 tensors of the same shape (F, H, W) at the camera size")
        if not (p4.is_contiguous() and n4.is_contiguous()):
            raise ValueError("prev / now must be contiguous")
        F = n4.shape[0]
        if out is None:
            out = torch.empty((F, self.height, self.width, 2), dtype=torch.float32, device=now.device)
        elif out.shape != (F, self.height, self.width, 2) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor (F, H, W, 2)")
        prm = params if params is not None else capi.flow_params()
        self._done(self.lib.mod_flow_compute_dev(self.h, F, p4.data_ptr(), n4.data_ptr(), C.byref(prm), out.data_ptr()), "mod_flow_compute_dev")
        return out[0] if single and out.dim() == 4 else out

    def estimate_disparity(self, left: torch.Tensor, right: torch.Tensor, params: capi.ModSgmParams,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """On-GPU semi-global matching (mod_sgm_compute_dev): device uint8 tensors (F,H,W) or (H,W) of the camera size -> (F,H,W) /
        (H,W) float32 disparity of the left image, min_disparity - 1 where rejected.  Enqueued on the context's stream."""
        single = left.dim() == 2
        l3, r3 = (left[None], right[None]) if single else (left, right)
        if l3.shape != r3.shape or l3.dtype != torch.uint8 or r3.dtype != torch.uint8 or l3.shape[1:] != (self.height, self.width):
            raise ValueError("left / right must be uint8 tensors of the same shape (F, H, W) at the camera size")
        if not (l3.is_contiguous() and r3.is_contiguous()):
            raise ValueError("left / right must be contiguous")
        F = l3.shape[0]
        if out is None:
            out = torch.empty((F, self.height, self.width), dtype=torch.float32, device=left.device)
        elif out.shape not in (l3.shape, l3.shape[1:])[:1 + (F == 1)] or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor (F, H, W) (one frame: or (H, W))")
        self._done(self.lib.mod_sgm_compute_dev(self.h, F, l3.data_ptr(), r3.data_ptr(), C.byref(params), out.data_ptr()), "mod_sgm_compute_dev")
        return out[0] if single and out.dim() == 3 else out

    def image_to_mono(self, src: torch.Tensor, layout: Optional[capi.ModImageLayout] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Grey planes (F, H, W) uint8 at the camera size from device 8-bit frames (mod_image_to_mono_dev): `src` holds F frames of
        layout.step * layout.height bytes each, back to back (any shape, contiguous uint8); layout None = the context's.  The camera-sized
        window at (x0, y0) is converted with OpenCV's 8-bit BGR2GRAY formula (packed YUV 4:2:2: grey = Y).  Enqueued on the context's
        stream."""
        lay = layout if layout is not None else self.get_image_layout()
        F, out = self._whole_messages(src, lay, out, torch.uint8, "src", "frames")
        self._done(self.lib.mod_image_to_mono_dev(self.h, F, src.data_ptr(), C.byref(lay), out.data_ptr()), "mod_image_to_mono_dev")
        return out

    def rectify(self, src: torch.Tensor, layout: Optional[capi.ModImageLayout] = None, eye: int = capi.MOD_EYE_LEFT,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Rectified grey planes (F, H, W) uint8 at the camera size from raw device 8-bit frames (mod_rectify_dev): `src` as for
        image_to_mono, `eye` selects the map (capi.MOD_EYE_LEFT / MOD_EYE_RIGHT) and, while side by side, the pane.  Enqueued on the
        context's stream."""
        lay = layout if layout is not None else self.get_image_layout()
        F, out = self._whole_messages(src, lay, out, torch.uint8, "src", "frames")
        self._done(self.lib.mod_rectify_dev(self.h, F, src.data_ptr(), C.byref(lay), int(eye), out.data_ptr()), "mod_rectify_dev")
        return out

    def rectification_map(self, eye: int = capi.MOD_EYE_LEFT, layout: Optional[capi.ModImageLayout] = None) -> np.ndarray:
        """The map k_rectify reads for `eye` and the window of `layout` (None = the context's), from the device
        (mod_rectify_map_host): (H, W, 2) int32, (qx, qy) in 1/32 pixel of the raw message; with a binning set the full window's map,
        (by H, bx W, 2)."""
        b = self.get_image_binning()
        out = np.empty((b.by * self.height, b.bx * self.width, 2), dtype=np.int32)
        self._check(self.lib.mod_rectify_map_host(self.h, int(eye), C.byref(layout) if layout is not None else None, out.ctypes.data))
        return out

    def estimate_egomotion(self, disp_prev: torch.Tensor, disp_now: torch.Tensor, flow: torch.Tensor,
                           params: Optional[capi.ModEgoParams] = None):
        """On-GPU stereo ego-motion (mod_egomotion_dev) of device float32 tensors (F,H,W), (F,H,W), (F,H,W,2) — or one frame without the
        F axis.  Returns (transforms (F,7) float64 [t xyz, q xyzw] prev -> now, NaN where the estimate failed; results: structured
        numpy array with status, correspondences, inliers, iterations, rms_px).  Synchronises the context's stream."""
        single = disp_now.dim() == 2
        dp, dn, fl = (disp_prev[None], disp_now[None], flow[None]) if single else (disp_prev, disp_now, flow)
        F = dn.shape[0]
        if dp.shape != dn.shape or dn.shape[1:] != (self.height, self.width) or fl.shape != (F, self.height, self.width, 2):
            raise ValueError("disp_prev / disp_now must be (F, H, W) and flow (F, H, W, 2) at the camera size")
        if any(t.dtype != torch.float32 or not t.is_contiguous() for t in (dp, dn, fl)):
            raise ValueError("disparities and flow must be contiguous float32 tensors")
        prm = params if params is not None else capi.ego_params()
        tf = torch.empty((F, 7), dtype=torch.float64, device=dn.device)
        res = torch.empty((F, C.sizeof(capi.ModEgoResult)), dtype=torch.uint8, device=dn.device)
        self._done(self.lib.mod_egomotion_dev(self.h, F, dp.data_ptr(), dn.data_ptr(), fl.data_ptr(), C.byref(prm), tf.data_ptr(),
                                                    res.data_ptr()), "mod_egomotion_dev")
        self.synchronize()
        return tf.cpu().numpy(), np.frombuffer(res.cpu().numpy().tobytes(), dtype=EGO_RESULT_DTYPE).copy()

    def synchronize(self) -> None:
        self._check(self.lib.mod_synchronize(self.h))

    # ---- measurement ------------------------------------------------------------------------------------------
    def set_profiling(self, on, stages=None) -> None:
        """Stage timers on/off; `stages` (iterable of MOD_STAGE_*) restricts them to those stages."""
        mask = 0
        if on:
            mask = capi.MOD_PROFILE_ALL if stages is None else sum(1 << int(s) for s in set(stages))
        self._check(self.lib.mod_set_profiling(self.h, mask))

    def reset_stage_times(self) -> None:
        self._check(self.lib.mod_reset_stage_times(self.h))

    def stage_time(self, stage: int):
        ms, calls = C.c_double(0), C.c_int64(0)
        self._check(self.lib.mod_get_stage_time(self.h, stage, C.byref(ms), C.byref(calls)))
        return ms.value, calls.value

    # ---- results to host --------------------------------------------------------------------------------------
    @staticmethod
    def objects_to_host(ws) -> list:
        """Per frame: structured numpy array of the accepted ModObject records."""
        n = ws["n_objects"].cpu().numpy()
        raw = ws["objects"].cpu().numpy()
        out = []
        for f in range(raw.shape[0]):
            k = min(int(n[f]), raw.shape[1])
            out.append(np.frombuffer(raw[f, :k].tobytes(), dtype=OBJECT_DTYPE).copy())
        return out

    def clusters_to_host(self, ws, frames: Optional[int] = None):
        """The member lists a call wrote (set_cluster_members).  Per frame a list of int32 arrays, cluster k's pixel indices v * W + u in
        the reference's order (u ascending, then v); with points also, second, per frame the list of (n, 3) float32 arrays of their
        x, y, z.  Copies the offsets first, then only the used prefix of indices / points."""
        off = ws["member_offsets"].cpu().numpy()
        K = ws["n_clusters"].cpu().numpy()
        pts_t = ws.get("member_points")
        F = off.shape[0] if frames is None else int(frames)
        lists, points = [], []
        for f in range(F):
            k, used = int(K[f]), int(off[f, int(K[f])])
            idx = ws["member_indices"][f, :used].cpu().numpy()
            lists.append([idx[off[f, j]:off[f, j + 1]].copy() for j in range(k)])
            if pts_t is not None:
                p = pts_t[f, :used].cpu().numpy()
                points.append([p[off[f, j]:off[f, j + 1]].copy() for j in range(k)])
        return (lists, points) if pts_t is not None else lists
