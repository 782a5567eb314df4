// image_fmt.h — what the image kernels (ingest.hip, rectify.hip) share: the 8-bit encodings' byte layout and the grey conversion.
#pragma once
#include "mod_launch.h"

// OpenCV's 8-bit BGR2GRAY (BT.601 in 14-bit fixed point, what cv_bridge's MONO8 conversion calls).  The weights sum to 16384, so
// B = G = R = v gives (16384 v + 8192) >> 14 = v exactly: a grey image in colour converts back to itself.
__device__ __forceinline__ uint32_t grey(uint32_t b, uint32_t g, uint32_t r) {
  return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14;
}

// A format: the pixel pitch C in bytes and either ONE grey channel at byte offset y of a pixel (mono: copied, never weighted) or
// the byte offsets of B, G, R (alpha, when there is one, is never read).  Packed YUV 4:2:2 is a one-channel format of pitch 2: the
// luma of pixel x is byte 2x + 1 (UYVY, "yuv422") or 2x (YUYV, "yuv422_yuy2"); the chroma bytes between are never used.
template <int Enc> struct Fmt;
template <> struct Fmt<MOD_ENCODING_MONO8>       { static constexpr bool mono = true;  static constexpr int C = 1, y = 0; };
template <> struct Fmt<MOD_ENCODING_BGR8>        { static constexpr bool mono = false; static constexpr int C = 3, b = 0, g = 1, r = 2; };
template <> struct Fmt<MOD_ENCODING_RGB8>        { static constexpr bool mono = false; static constexpr int C = 3, b = 2, g = 1, r = 0; };
template <> struct Fmt<MOD_ENCODING_BGRA8>       { static constexpr bool mono = false; static constexpr int C = 4, b = 0, g = 1, r = 2; };
template <> struct Fmt<MOD_ENCODING_RGBA8>       { static constexpr bool mono = false; static constexpr int C = 4, b = 2, g = 1, r = 0; };
template <> struct Fmt<MOD_ENCODING_YUV422>      { static constexpr bool mono = true;  static constexpr int C = 2, y = 1; };
template <> struct Fmt<MOD_ENCODING_YUV422_YUY2> { static constexpr bool mono = true;  static constexpr int C = 2, y = 0; };
