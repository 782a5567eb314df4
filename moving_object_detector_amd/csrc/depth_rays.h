// depth_rays.h — one entry of a depth camera's ray table (mod_set_depth_distortion): the undistorted ray (x, y) at
// z = 1 of lattice point (Uc, Vc) of the depth message, a pixel centre (U, V) or a pixel corner (U - 0.5, V - 0.5).  The ONE
// definition of that arithmetic: k_depth_rays (depth.hip) evaluates it on the device, and a plain g++ build can evaluate it on the
// host.  include/mod_sf.h states the formula; tests/models/depth_undistort_model.py restates it in numpy.
//
// The inverse of the rational model (plumb_bob / rational_polynomial) by cv::undistortPoints' fixed-point iteration, with a fixed
// count and a round-trip test through the forward model.  The forward lines restate those of rectify_map.h's rational branch (the
// same operations in the same order); rectify_map.h itself is not touched, so the rectifier's map kernel does not move.
//
// Every operation is an IEEE f64 + - * / or fabs, in the header's order; the build must not contract products and sums
// (-ffp-contract=off).  No libm / device-library function is called.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdint.h>

#include "../../include/mod_sf.h"

#if defined(__HIPCC__)
#define DR_HD __host__ __device__ __forceinline__
#else
#define DR_HD inline
#endif

namespace depth_rays {

// the depth camera of the whole message and its distortion: what a table is built from (and, with the message's size, its cache key)
struct Lens { double D[8], fx, fy, cx, cy; };

constexpr double kTol = 1.0 / 64;   // the round trip's bound, in pixels of the depth message

// the ray of lattice point (Uc, Vc); invalid (the round trip misses by more than kTol on an axis, or is not a number): x = y = NaN
DR_HD void entry(const Lens &c, double Uc, double Vc, double &x, double &y) {
  const double k1 = c.D[0], k2 = c.D[1], p1 = c.D[2], p2 = c.D[3], k3 = c.D[4], k4 = c.D[5], k5 = c.D[6], k6 = c.D[7];
  const double xd = (Uc - c.cx) / c.fx, yd = (Vc - c.cy) / c.fy;
  x = xd; y = yd;
#pragma unroll
  for (int i = 0; i < MOD_DEPTH_UNDISTORT_ITERS; i++) {
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * x * y;
    const double ic = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
    const double dx = p1 * xy2 + p2 * (r2 + 2.0 * x2), dy = p1 * (r2 + 2.0 * y2) + p2 * xy2;
    x = (xd - dx) * ic; y = (yd - dy) * ic;
  }
  // the check: the forward model at (x, y), the rectifier's lines x2 .. yd
  const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * x * y;
  const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
  const double xf = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * x2), yf = y * kr + p1 * (r2 + 2.0 * y2) + p2 * xy2;
  const bool ok = fabs(c.fx * (xf - xd)) <= kTol && fabs(c.fy * (yf - yd)) <= kTol;   // (a NaN fails)
  if (!ok) x = y = __builtin_nan("");
}

}  // namespace depth_rays
