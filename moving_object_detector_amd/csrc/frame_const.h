// frame_const.h — the per-frame constants of the scene-flow kernel from a ModTransform, on the host (mod_sf.hip) and on the device
// (egomotion.hip writes the FrameConst of an estimated transform straight into HBM).  Plain operators, no library calls with
// implementation-defined rounding: with -ffp-contract=off both compilations give the same bits.
#pragma once
#include <math.h>

#include "../../include/mod_sf.h"
#include "exact_div.h"
#include "mod_device.h"

#pragma clang fp contract(off)

// Eigen::Quaterniond::toRotationMatrix operation order (tf2::transformToEigen, scene_flow_constructor.cpp:411);
// the quaternion is used as given, without normalisation.
ED_HD void transform_to_rows(const double t[3], const double q[4], double m[12]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  m[0] = 1.0 - (tyy + tzz); m[1] = txy - twz;         m[2] = txz + twy;          m[3] = t[0];
  m[4] = txy + twz;         m[5] = 1.0 - (txx + tzz); m[6] = tyz - twx;          m[7] = t[1];
  m[8] = txz - twy;         m[9] = tyz + twx;         m[10] = 1.0 - (txx + tyy); m[11] = t[2];
}

ED_HD void fill_frame_const(FrameConst &h, const double t[3], const double q[4], double dt) {
  transform_to_rows(t, q, h.m);
  h.dt = dt;
  // |t_i + (m_i0 x + (m_i1 y + m_i2 z))| <= tmax + 3 mmax B stays below FLT_MAX / 2 (so the F32 cast is finite, and no
  // intermediate can overflow or turn NaN) for every |x|,|y|,|z| <= B.  Non-finite transforms get B = 0: always compute.
  double mmax = 0.0, tmax = 0.0;
  bool finite = true;
  for (int i = 0; i < 12; i++) {
    const double v = fabs(h.m[i]);
    finite = finite && isfinite(v);
    if (i % 4 == 3) tmax = tmax < v ? v : tmax; else mmax = mmax < v ? v : mmax;
  }
  double B = 0.0;
  if (finite && tmax < 1e37) {
    const double den = 3.0 * (mmax < 1e-30 ? 1e-30 : mmax);
    const double b = (1.7e38 - tmax) / den;
    B = 1e30 < b ? 1e30 : b;
  }
  h.pad[0] = B;
  // velocity = difference / dt through the correctly rounded reciprocal (exact_div.h) when dt is an ordinary number
  const bool usable = exact_div::reciprocal_usable(h.dt);
  h.pad[1] = usable ? 1.0 / h.dt : 0.0;
  h.pad[2] = usable ? 1.0 : 0.0;
}
