// rectify_map.h — one entry of a rectification map: where pixel (U, V) of the RECTIFIED image lies in the raw
// message, in 1/32 pixel.  The ONE definition of that arithmetic: k_rectify_map (rectify.hip) evaluates it on the device, and a
// plain g++ build evaluates it on the host (tests/cpp/rectify_map_print.cpp), so a CPU test pins every bit before a GPU is involved.
// include/mod_sf.h states both formulas; tests/models/rectify_model.py and tests/models/fisheye_model.py restate them in numpy.
//
// Every operation is an IEEE f64 + - * / sqrt or rint, in the header's order; the build must not contract products and sums
// (-ffp-contract=off).  No libm / device-library transcendental is called: the fisheye model's arctangent is atan_m below.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdint.h>

#include "../../include/mod_sf.h"

#if defined(__HIPCC__)
#define RM_HD __host__ __device__ __forceinline__
#else
#define RM_HD inline
#endif

namespace rectify_map {

constexpr double kQMax = 16777216.0;   // 2^24: the map's clamp, so that ix + 1 and iy * step stay far from overflow
constexpr double kRMax = 1048576.0;    // 2^20: the largest tan(angle to the optical axis) the equidistant model evaluates

// 1/32 pixel, half to even (the default rounding mode); non-finite -> -2^24, else clamped to [-2^24, 2^24]
RM_HD int32_t quantise(double m) {
  const double q = rint(m * 32.0);
  if (!(fabs(q) <= 1.7976931348623157e308)) return (int32_t)-kQMax;   // NaN, +inf, -inf
  return (int32_t)(q < -kQMax ? -kQMax : q > kQMax ? kQMax : q);
}

// The library's own arctangent for r in [0, 2^20], from correctly rounded operations only, so that numpy, g++ and the GPU agree in
// every bit (libm's and the device library's atan are not correctly rounded and differ from each other).  Four half-angle steps
// t <- t / (1 + sqrt(1 + t t)) bring t below tan(pi / 32), where twelve terms of the series leave less than 2^-60; atan r = 16 atan t.
// Within 1.2e-15 absolute and 8.7e-16 relative of the true arctangent (tests/test_fisheye_model.py).
RM_HD double atan_m(double r) {
  double t = r;
  for (int i = 0; i < 4; i++) t = t / (1.0 + sqrt(1.0 + t * t));
  const double u = t * t;
  double s = -1.0 / 23.0;
  s = s * u + 1.0 / 21.0;
  s = s * u + -1.0 / 19.0;
  s = s * u + 1.0 / 17.0;
  s = s * u + -1.0 / 15.0;
  s = s * u + 1.0 / 13.0;
  s = s * u + -1.0 / 11.0;
  s = s * u + 1.0 / 9.0;
  s = s * u + -1.0 / 7.0;
  s = s * u + 1.0 / 5.0;
  s = s * u + -1.0 / 3.0;
  s = s * u + 1.0;
  return 16.0 * (t * s);
}

// Model: MOD_DISTORTION_RATIONAL or MOD_DISTORTION_EQUIDISTANT (a template parameter: neither instance carries the other's code)
template <int Model>
RM_HD void entry(const ModRectifyCamera &cam, double U, double V, int32_t &qx, int32_t &qy) {
  const double fx = cam.K[0], fy = cam.K[4], cx = cam.K[2], cy = cam.K[5];
  const double fxp = cam.P[0], fyp = cam.P[5], cxp = cam.P[2], cyp = cam.P[6];
  const double *R = cam.R;
  double x = (U - cxp) / fxp, y = (V - cyp) / fyp;
  const double X = R[0] * x + R[3] * y + R[6], Y = R[1] * x + R[4] * y + R[7], Wd = R[2] * x + R[5] * y + R[8];   // R transposed
  x = X / Wd; y = Y / Wd;
  double mx, my;
  if constexpr (Model == MOD_DISTORTION_EQUIDISTANT) {
    const double k1 = cam.D[0], k2 = cam.D[1], k3 = cam.D[2], k4 = cam.D[3];
    qx = qy = (int32_t)-kQMax;
    if (!(Wd > 0.0)) return;            // the ray is at or behind 90 degrees (cv::fisheye writes -inf there)
    const double r = sqrt(x * x + y * y);
    if (!(r <= kRMax)) return;          // (also NaN) such a pixel is never inside a real image
    const double th = atan_m(r), t2 = th * th;
    const double td = th * (1.0 + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2);
    const double sc = r == 0.0 ? 1.0 : td / r;
    mx = fx * (x * sc) + cx; my = fy * (y * sc) + cy;
  } else {
    static_assert(Model == MOD_DISTORTION_RATIONAL, "unknown distortion model");
    const double k1 = cam.D[0], k2 = cam.D[1], p1 = cam.D[2], p2 = cam.D[3], k3 = cam.D[4], k4 = cam.D[5], k5 = cam.D[6], k6 = cam.D[7];
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * x * y;
    const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
    const double xd = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * x2), yd = y * kr + p1 * (r2 + 2.0 * y2) + p2 * xy2;
    mx = fx * xd + cx; my = fy * yd + cy;
  }
  qx = quantise(mx); qy = quantise(my);
}

// the same, with the model chosen at run time (host callers)
inline void entry(int model, const ModRectifyCamera &cam, double U, double V, int32_t &qx, int32_t &qy) {
  if (model == MOD_DISTORTION_EQUIDISTANT) entry<MOD_DISTORTION_EQUIDISTANT>(cam, U, V, qx, qy);
  else entry<MOD_DISTORTION_RATIONAL>(cam, U, V, qx, qy);
}

}  // namespace rectify_map
