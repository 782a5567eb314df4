"""CPU: tests/models/depth_splat_model.py, the numpy restatement of the footprint rule (include/mod_sf.h, "The footprint") that the GPU
tests compare k_depth_register_splat with bit for bit: against an independent scalar Python loop, and the properties the rule exists
for, on a 40 x 24 depth camera under an 80 x 48 image camera (tests/depth_splat_cases.py).  A flat wall that the point rule leaves
three quarters empty has no hole left, under a roll of 8 and of 180 degrees too; every target the point rule fills stays filled with a z
no larger; a foreground box owns what both layers cover; equal cameras, a downsampling pair and capped footprints give the point
rule's output; the order of the samples does not matter."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "models"))
import depth_model as dm  # noqa: E402
import depth_splat_cases as sc  # noqa: E402
import depth_splat_model as sm  # noqa: E402
from test_depth_model import _is_valid, _sample, _same  # noqa: E402

f32 = np.float32
FT = sc.fT(sc.CAM)


def _both(metres, reg, cam=sc.CAM, W=sc.W, H=sc.H, encoding="32FC1", nan=False):
    msg, lay = sc.message(metres, encoding)
    if encoding == "32FC1" and not nan:                  # sc.message's NaN sample would be a hole of the scene's own
        msg[:, lay.height // 2, 4 * (lay.width // 2):4 * (lay.width // 2) + 4] = np.frombuffer(f32(metres[0, lay.height // 2, lay.width // 2]).tobytes(), np.uint8)
    frames = metres.shape[0]
    point, pn = dm.register(msg, lay, reg, cam, W, H, FT, 0.0, frames)
    splat, sn = sm.register_splat(msg, lay, reg, cam, W, H, FT, 0.0, frames)
    return point, pn, splat, sn


def _scalar_splat(msg, lay, reg, cam, W, H, fT, dmin, frames):
    """Python floats are IEEE doubles and Python evaluates one operation at a time"""
    best = {}
    R, t = [float(v) for v in reg.R], [float(v) for v in reg.t]

    def chain(u, v, Z0):
        X0 = ((u - reg.cx) * Z0) / reg.fx
        Y0 = ((v - reg.cy) * Z0) / reg.fy
        return (((R[0] * X0 + R[1] * Y0) + R[2] * Z0) + t[0], ((R[3] * X0 + R[4] * Y0) + R[5] * Z0) + t[1], ((R[6] * X0 + R[7] * Y0) + R[8] * Z0) + t[2])

    def put(key, zf):
        if key not in best or zf < best[key]:
            best[key] = zf

    for f in range(frames):
        for V in range(lay.height):
            for U in range(lay.width):
                z = _sample(msg, lay, f, U, V)
                if not _is_valid(z):
                    continue
                Z0 = float(z)
                X, Y, Z = chain(float(U), float(V), Z0)
                if not (Z > 0 and math.isfinite(Z)):
                    continue
                zf = f32(Z)
                a = ((cam.fx * X + cam.Tx) / Z + cam.cx) + 0.5
                b = ((cam.fy * Y + cam.Ty) / Z + cam.cy) + 0.5
                if 0 <= a < W and 0 <= b < H:
                    put((f, math.floor(b), math.floor(a)), zf)
                corners = [chain(U + du, V + dv, Z0) for du in (-0.5, 0.5) for dv in (-0.5, 0.5)]
                if not all(c[2] > 0 and math.isfinite(c[2]) for c in corners):
                    continue
                p = [(cam.fx * c[0] + cam.Tx) / c[2] + cam.cx for c in corners]
                q = [(cam.fy * c[1] + cam.Ty) / c[2] + cam.cy for c in corners]
                if not all(math.isfinite(v) for v in p + q):
                    continue
                ulo, uhi = math.ceil(min(min(p[0], p[1]), min(p[2], p[3]))), math.ceil(max(max(p[0], p[1]), max(p[2], p[3]))) - 1
                vlo, vhi = math.ceil(min(min(q[0], q[1]), min(q[2], q[3]))), math.ceil(max(max(q[0], q[1]), max(q[2], q[3]))) - 1
                if uhi - ulo + 1 > 8 or vhi - vlo + 1 > 8:
                    continue
                for v in range(max(vlo, 0), min(vhi, H - 1) + 1):
                    for u in range(max(ulo, 0), min(uhi, W - 1) + 1):
                        put((f, v, u), zf)
    out = np.full((frames, H, W), f32(dmin) - f32(1.0), f32)
    with np.errstate(all="ignore"):
        for key, zf in best.items():
            out[key] = f32(fT) / zf
    return out


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
@pytest.mark.parametrize("name", ["wall + box", "roll 180", "under the cap", "registered_case"])
def test_model_matches_a_scalar_loop(name, encoding):
    msg, lay, reg, cam, W, H, frames = sc.rig(name, encoding)
    got, n = sm.register_splat(msg, lay, reg, cam, W, H, sc.fT(cam), cam.min_disparity, frames)
    assert _same(got, _scalar_splat(msg, lay, reg, cam, W, H, sc.fT(cam), cam.min_disparity, frames))
    if name == "registered_case":                         # the case holds what its name in depth_splat_cases says
        point, pn = dm.register(msg, lay, reg, cam, W, H, sc.fT(cam), cam.min_disparity, frames)
        assert pn["behind"] >= 1 and pn["outside"] >= 1 and n["clipped_empty"] >= 1 and n["painted"] >= 100 and n["empty"] >= 1, (pn, n)


def test_flat_wall_has_no_holes_left():
    point, pn, splat, sn = _both(sc.wall(), sc.REG)
    inner_p, inner_s = point[0, 6:-6, 8:-8], splat[0, 6:-6, 8:-8]
    assert inner_p.size == 2304
    assert (inner_p < 0).sum() >= 0.7 * inner_p.size, (inner_p < 0).sum()      # the point rule: three quarters empty (1722 of 2304)
    assert (inner_s < 0).sum() == 0
    assert sn["capped"] == 0 and sn["corner_behind"] == 0


def test_flat_wall_under_a_roll_of_8_degrees():
    point, pn, splat, sn = _both(sc.wall(), dm.Registration(R=sc.pose(8.0), t=sc.T, **sc.SMALL))
    assert (splat[0, 8:-8, 10:-10] < 0).sum() == 0
    assert (point[0, 8:-8, 10:-10] < 0).sum() > 0


def test_flat_wall_under_a_roll_of_180_degrees():
    """the minimum and the maximum of the corners swap roles"""
    point, pn, splat, sn = _both(sc.wall(), dm.Registration(R=sc.pose(180.0), t=sc.T, **sc.SMALL))
    assert (splat[0, 6:-6, 8:-8] < 0).sum() == 0
    assert (point[0, 6:-6, 8:-8] < 0).sum() >= 0.7 * 2304


@pytest.mark.parametrize("name", sc.RIGS)
def test_superset_of_the_point_rule(name):
    """every target the point rule fills is filled with a z no larger (a disparity no smaller), and most keep the point's own z"""
    msg, lay, reg, cam, W, H, frames = sc.rig(name, "32FC1")
    point, pn = dm.register(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    splat, sn = sm.register_splat(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    hit = point >= 0
    assert hit.any() and (splat[hit] >= point[hit]).all()
    assert sn["empty"] <= pn["empty"]
    # bit for bit where the point sample is the nearest: the z-buffer says which targets those are
    zbuf, _ = sm.zbuffer(msg, lay, reg, cam, W, H, frames)
    with np.errstate(all="ignore"):
        zp = np.where(hit, f32(sc.fT(cam)) / point, f32(np.inf)).reshape(-1)
    zs = zbuf.view(f32)
    nearest = hit.reshape(-1) & ~(zs < zp)
    assert nearest.sum() > hit.sum() // 2
    assert splat.reshape(-1)[nearest].tobytes() == point.reshape(-1)[nearest].tobytes()


@pytest.mark.parametrize("baseline,least", [(sc.T[0], 1), (0.1, 40)])
def test_foreground_wins(baseline, least):
    """a box at 0.8 m in front of the wall at 2 m: painted alone, each layer covers a region; where both do, the box's z stays.  The
    rig's 2 cm baseline moves the box by 0.6 targets against the wall, so few targets are shared; 10 cm moves it by 4"""
    reg = dm.Registration(R=sc.pose(), t=(baseline,) + sc.T[1:], **sc.SMALL)
    m = sc.wall()
    box = np.zeros_like(m, bool)
    box[0, 8:16, 12:24] = True
    only_box, only_wall, both = np.where(box, 0.8, 0.0), np.where(box, 0.0, 2.0), np.where(box, 0.8, 2.0)
    _, _, sb, _ = _both(only_box, reg)
    _, _, sw, _ = _both(only_wall, reg)
    _, _, s, _ = _both(both, reg)
    shared = (sb >= 0) & (sw >= 0)
    assert shared.sum() >= least, "the layers' footprints do not overlap enough: the check would be empty"
    assert s[shared].tobytes() == sb[shared].tobytes() and (sb[shared] > sw[shared]).all()
    assert s[(sb >= 0)].tobytes() == sb[sb >= 0].tobytes()                   # the box is whole
    assert s[(sb < 0)].tobytes() == sw[sb < 0].tobytes()                     # ... and the wall is what is left


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_identity_gives_the_point_rule(encoding):
    msg, lay, reg, cam, W, H, frames = sc.rig("identity", encoding)
    point, pn = dm.register(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    splat, sn = sm.register_splat(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    assert pn["empty"] >= 10 and pn["kept"] >= frames * W * H * 3 // 4 and pn["double_hits"] == 0
    assert sn["painted"] == pn["kept"] and sn["capped"] == 0 and sn["clipped_empty"] == 0
    assert _same(point, splat)


def test_downsampling_gives_the_point_rule():
    msg, lay, reg, cam, W, H, frames = sc.rig("downsampling", "16UC1")
    point, pn = dm.register(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    splat, sn = sm.register_splat(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    assert sn["clipped_empty"] >= 1000 and sn["capped"] == 0                  # half a target wide: most hold no centre
    assert _same(point, splat)


def test_cap():
    msg, lay, reg, cam, W, H, frames = sc.rig("cap", "16UC1")
    point, pn = dm.register(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    splat, sn = sm.register_splat(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    assert sn["painted"] == 0 and sn["clipped_empty"] == 0 and sn["capped"] == pn["kept"] + pn["outside"] >= 2000 and pn["kept"] >= 100, (sn, pn)
    assert _same(point, splat)
    msg, lay, reg, cam, W, H, frames = sc.rig("cap, posed", "16UC1")
    point, pn = dm.register(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    splat, sn = sm.register_splat(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    assert sn["painted"] == 0 and sn["capped"] >= 2000 and pn["kept"] >= 100, (sn, pn)
    assert _same(point, splat)
    msg, lay, reg, cam, W, H, frames = sc.rig("under the cap", "16UC1")      # a ratio just under 8: none capped, 7 or 8 targets per axis
    splat, sn = sm.register_splat(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    assert sn["capped"] == 0 and sn["painted"] >= 200, sn
    point, pn = dm.register(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    assert sn["empty"] < pn["empty"] // 4


@pytest.mark.parametrize("name", ["wall + box", "registered_case"])
def test_order_of_the_samples_does_not_matter(name):
    msg, lay, reg, cam, W, H, frames = sc.rig(name, "32FC1")
    want, _ = sm.register_splat(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames)
    n = int(dm.valid(dm.samples(msg, lay, frames)).sum())
    for seed in (0, 1):
        order = np.random.default_rng(seed).permutation(n)
        got, _ = sm.register_splat(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames, order=order)
        assert _same(got, want)
    got, _ = sm.register_splat(msg, lay, reg, cam, W, H, sc.fT(cam), 0.0, frames, order=np.arange(n)[::-1])
    assert _same(got, want)
