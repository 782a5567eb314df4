// label_palette.h — the colours of the cluster image and of the ~clusters markers: the built-in 256-entry table,
// the rule that picks a cluster's entry, and the table as the renderer takes it.  Plain C++: the kernel (label_image.hip), the host
// functions (mod_cluster_color, mod_cluster_palette) and tests/test_cluster_palette_cpp.py's program all read this text; no HIP
// include when g++ compiles it, like exact_div.h.
//
// The reference colours label k of a frame with K clusters with entry (k * 255) / K of cv::applyColorMap(COLORMAP_HSV)
// (color_set.cpp; clusterer_nodelet.cpp:269-322).  OpenCV's table is not restated here: the built-in one is this library's own hue
// wheel, and a caller who has OpenCV uploads COLORMAP_HSV instead (ModClusterImage.palette_bgr).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LP_HD __host__ __device__ __forceinline__
#else
#define LP_HD inline
#endif
#include <stdint.h>

namespace label_palette {

constexpr int kEntries = 256;

// Entry i of the built-in table as B | G << 8 | R << 16.  t = 6 i, sector s = t >> 8 (0 .. 5), f = t & 255, g = 255 - f:
//   s   0            1            2            3            4            5
//   RGB (255, f, 0)  (g, 255, 0)  (0, 255, f)  (0, g, 255)  (f, 0, 255)  (255, 0, g)
// Entry 0 is (0, 0, 255) B, G, R and entry 255 is (5, 0, 255).
LP_HD uint32_t builtin_bgr(uint32_t i) {
  const uint32_t t = 6u * i, s = t >> 8, f = t & 255u, g = 255u - f;
  uint32_t R, G, B;
  switch (s) {
    case 0: R = 255u; G = f; B = 0u; break;
    case 1: R = g; G = 255u; B = 0u; break;
    case 2: R = 0u; G = 255u; B = f; break;
    case 3: R = 0u; G = g; B = 255u; break;
    case 4: R = f; G = 0u; B = 255u; break;
    default: R = 255u; G = 0u; B = g; break;
  }
  return B | (G << 8) | (R << 16);
}

// The entry of label k in a frame of K clusters, 0 <= k < K: (k * 255) / K.  The product passes 2^32 above 16.8 M pixels: 64 bits.
LP_HD uint32_t palette_index(uint32_t k, uint32_t K) { return (uint32_t)(((uint64_t)k * 255u) / K); }

// The same entry without an integer division per pixel: rcp = palette_rcp(K), once per frame.  k * rcp is within 6.1e-5 of
// k * 255 / K (four F32 roundings of 2^-24 each on a value below 255), so its integer part is the quotient or one beside it; the
// remainder of that guess, exact in wrapping 32-bit arithmetic (it lies in (-K, 2 K) and K < 2^27), says which.
// Precondition: K < kRcpLimit = 2^27 (every K a context can produce: max_width * max_height < 2^27); the kernel divides outright above it.
constexpr uint32_t kRcpLimit = 1u << 27;
LP_HD float palette_rcp(uint32_t K) { return 255.0f / (float)K; }
LP_HD uint32_t palette_index_rcp(uint32_t k, uint32_t K, float rcp) {
  uint32_t q = (uint32_t)((float)k * rcp);
  const int32_t r = (int32_t)(k * 255u - q * K);
  q = r < 0 ? q - 1u : q;
  q = r >= (int32_t)K ? q + 1u : q;
  return q;
}

// A table as the renderer takes it: 768 bytes B, G, R, B, ... in 192 words (by value in the kernel's arguments)
struct Table { uint32_t w[3 * kEntries / 4]; };
inline void table_from_bytes(const uint8_t *bgr, Table *t) {
  for (int i = 0; i < 3 * kEntries / 4; i++)
    t->w[i] = (uint32_t)bgr[4 * i] | ((uint32_t)bgr[4 * i + 1] << 8) | ((uint32_t)bgr[4 * i + 2] << 16) | ((uint32_t)bgr[4 * i + 3] << 24);
}
inline void builtin_bytes(uint8_t *bgr) {
  for (int i = 0; i < kEntries; i++) {
    const uint32_t c = builtin_bgr((uint32_t)i);
    bgr[3 * i] = (uint8_t)c; bgr[3 * i + 1] = (uint8_t)(c >> 8); bgr[3 * i + 2] = (uint8_t)(c >> 16);
  }
}
// entry i of a table, B | G << 8 | R << 16
LP_HD uint32_t table_entry(const Table &t, uint32_t i) {
  const uint32_t b = 3u * i, lo = t.w[b >> 2], hi = t.w[(b >> 2) + 1 < 3u * kEntries / 4 ? (b >> 2) + 1 : b >> 2], sh = 8u * (b & 3u);
  return (sh ? (lo >> sh) | (hi << (32u - sh)) : lo) & 0x00ffffffu;
}

}  // namespace label_palette
