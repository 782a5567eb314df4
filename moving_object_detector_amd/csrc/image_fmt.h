// image_fmt.h — what the image kernels (ingest.hip, rectify.hip) share: the 8-bit encodings' channel layout and the grey conversion.
#pragma once
#include "mod_launch.h"

// OpenCV's 8-bit BGR2GRAY (BT.601 in 14-bit fixed point, what cv_bridge's MONO8 conversion calls).  The weights sum to 16384, so
// B = G = R = v gives (16384 v + 8192) >> 14 = v exactly: a grey image in colour converts back to itself.
__device__ __forceinline__ uint32_t grey(uint32_t b, uint32_t g, uint32_t r) {
  return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14;
}

// channels and the byte offsets of B, G, R within a pixel (alpha, when there is one, is never read)
template <int Enc> struct Fmt;
template <> struct Fmt<MOD_ENCODING_MONO8> { static constexpr int C = 1; };
template <> struct Fmt<MOD_ENCODING_BGR8>  { static constexpr int C = 3, b = 0, g = 1, r = 2; };
template <> struct Fmt<MOD_ENCODING_RGB8>  { static constexpr int C = 3, b = 2, g = 1, r = 0; };
template <> struct Fmt<MOD_ENCODING_BGRA8> { static constexpr int C = 4, b = 0, g = 1, r = 2; };
template <> struct Fmt<MOD_ENCODING_RGBA8> { static constexpr int C = 4, b = 2, g = 1, r = 0; };
