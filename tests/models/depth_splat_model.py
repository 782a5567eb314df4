"""numpy restatement of k_depth_register_splat (csrc/depth.hip; include/mod_sf.h, "The footprint"): the registered
path with mod_set_depth_splat on, bit for bit.  The scatter is depth_model.zbuffer (np.float64 in the header's operation order, one
operation at a time; np.minimum and np.maximum propagate a NaN, as the header says); this file names what it counts."""
import depth_model
from depth_model import count, zbuffer_to_disparity


def zbuffer(buf, lay, reg, cam, W, H, frames=1, order=None):
    """(z-buffer uint32 [frames * H * W], counts).  counts, over all frames: `capped` footprints wider or taller than SPLAT_MAX targets
    before clipping, `clipped_empty` footprints that hold no target after the clip (those that held none before it included),
    `corner_behind` footprints with a corner at Z <= 0 (or not finite), `painted` footprints that were painted, `empty` targets
    nothing reached.  `order`: a permutation of the valid samples, applied before the minima are taken (the result must not change)."""
    zbuf, s = depth_model.zbuffer(buf, lay, reg, cam, W, H, frames, splat=True, order=order)
    counts = {"capped": count(s["capped"]), "clipped_empty": count(s["clipped_empty"]), "corner_behind": count(s["front"], ~s["corners_front"]),
              "painted": count(s["painted"]), "empty": count(zbuf == depth_model.EMPTY)}
    return zbuf, counts


def register_splat(buf, lay, reg, cam, W, H, fT, min_disparity, frames=1, order=None):
    """the registered path with the mode on: ([frames][H][W] float32, counts of zbuffer())"""
    zbuf, counts = zbuffer(buf, lay, reg, cam, W, H, frames, order)
    return zbuffer_to_disparity(zbuf, W, H, fT, min_disparity, frames), counts
