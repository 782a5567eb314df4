// flow_color.h — the colour rule of the flow, residual-flow and disparity images (include/mod_sf.h "Flow and disparity images";
// DESIGN.md §3.2d).  One text for the kernels (flow_image.hip) and the host-only legend (mod_flow_color).  F32 throughout, every
// operation one correctly rounded IEEE operation (add, subtract, multiply, divide, sqrtf, compare, truncation of a non-negative
// value); no FMA (contraction is off), no atan2.  The palette is label_palette.h's hue wheel: no second table.
#pragma once
#include <math.h>

#include "label_palette.h"

#pragma clang fp contract(off)

namespace flow_color {

LP_HD bool is_finite(float v) { return v >= -3.4028234663852886e38f && v <= 3.4028234663852886e38f; }   // false for NaN and +-inf

// min(255, (int)v) for v >= 0, with the comparison made in F32 ahead of the conversion: defined for +inf and NaN too (both 255)
LP_HD uint32_t trunc255(float v) { return v < 255.0f ? (uint32_t)(int32_t)v : 255u; }

// white at s = 0, the palette's entry p (B | G << 8 | R << 16) at s = 255: per channel 255 - ((255 - p_c) s + 127) / 255
LP_HD uint32_t blend(uint32_t p, uint32_t s) {
  uint32_t out = 0;
  for (int ch = 0; ch < 3; ch++) {
    const uint32_t pc = (p >> (8 * ch)) & 255u;
    out |= (255u - ((255u - pc) * s + 127u) / 255u) << (8 * ch);
  }
  return out;
}

// The colour of the vector (fx, fy) at full strength max_px (> 0, finite), B | G << 8 | R << 16; pal(i): entry i of the table
template <class P> LP_HD uint32_t flow_bgr(float fx, float fy, float max_px, const P &pal) {
  if (!is_finite(fx) || !is_finite(fy)) return 0u;                  // invalid: black
  const float xx = fx * fx, yy = fy * fy;
  const float m = sqrtf(xx + yy);
  if (m == 0.0f) return 0x00ffffffu;                                // at rest (or too small to have a square): white
  const float r = m / max_px;
  const uint32_t s = trunc255(255.0f * r);
  const float A = fabsf(fx) + fabsf(fy);                            // > 0: m > 0
  const float t = fy / A;                                           // [-1, 1]
  const float q = fx < 0.0f ? 2.0f - t : (fy < 0.0f ? 4.0f + t : t);   // the diamond angle, [0, 4]
  return blend(pal(trunc255(q * 64.0f)), s);
}

// The colour of disparity d in the camera's range [dmin, dmax], dmin < dmax
template <class P> LP_HD uint32_t disparity_bgr(float d, float dmin, float dmax, const P &pal) {
  if (!is_finite(d) || d < dmin || d > dmax || d == 0.0f) return 0u;   // getDisparity's and getPoint3D's rejects: black
  const float r = (d - dmin) / (dmax - dmin);
  return pal(trunc255(255.0f * r));
}

struct Builtin { LP_HD uint32_t operator()(uint32_t i) const { return label_palette::builtin_bgr(i); } };

}  // namespace flow_color
