// label_image.hip — the cluster image: publishClustersImage's per-pixel pass (clusterer_nodelet.cpp:292-322) on the
// label plane where the cluster stage left it.
//
// k_cluster_image reads labels [frames][N] (int32) and n_clusters [frames] and writes image [frames][N][3] (B, G, R, packed): pixel i
// of frame f is black unless 0 <= label < K = n_clusters[f], else entry (label * 255) / K of the table (label_palette.h).  A label
// outside [0, K) never indexes the table, and K <= 0 never divides.
//
// Memory-bound: 4 B read and 3 B written per pixel.  The batch is one flat pixel array; a lane takes four consecutive pixels of the
// FLAT array's four-pixel grid — one 16-byte label load (the plane's base permitting, else four dwords) and 12 bytes stored as three
// whole dwords: the image's base is 4-byte aligned and four pixels are 12 bytes, so every group starts on a dword whatever N is.  K
// is per frame, so frames ride in blockIdx.y and a frame's lanes cover only the groups that lie wholly inside it: frame f starts
// (f N) mod 4 pixels into a group, and the up to three pixels in front of its first whole group and the up to three behind its last
// one — the halves of the groups that straddle two frames — are written byte-wise by one more lane of that frame.
// The table comes by value in the kernel's arguments (a frame in flight keeps the table of its submit for free) and is spread into
// LDS, one dword an entry; the quotient is label_palette::palette_index_rcp with the frame's reciprocal.
#include "label_palette.h"
#include "mod_launch.h"

namespace {

constexpr int kBlock = 256;
static_assert(kBlock == label_palette::kEntries, "one thread spreads one table entry");

__device__ __forceinline__ uint32_t colour_of(int32_t label, uint32_t K, float rcp, const uint32_t *lut) {
  const bool in = (uint32_t)label < K;       // K <= 0 arrives as 0: nothing is inside
  if (!in) return 0u;
  // a caller's count beyond what any context can hold (mod_cluster_image_dev takes it as it comes): the reciprocal form's remainder
  // is proven for K < 2^27 only, so such a frame divides outright (uniform: K is the frame's)
  const uint32_t q = K < label_palette::kRcpLimit ? label_palette::palette_index_rcp((uint32_t)label, K, rcp) : label_palette::palette_index((uint32_t)label, K);
  return lut[q];
}

template <bool ALIGNED16>
__global__ __launch_bounds__(kBlock) void k_cluster_image(uint32_t N, const int32_t *__restrict__ labels, const int32_t *__restrict__ n_clusters,
                                                          const label_palette::Table table, uint8_t *__restrict__ image) {
  __shared__ uint32_t lut[label_palette::kEntries];
  lut[threadIdx.x] = label_palette::table_entry(table, threadIdx.x);
  __syncthreads();
  const uint32_t f = blockIdx.y;
  const int32_t Ks = n_clusters[f];
  const uint32_t K = Ks > 0 ? (uint32_t)Ks : 0u;
  const float rcp = label_palette::palette_rcp(K ? K : 1u);
  const size_t start = (size_t)f * N;                                     // the frame's first pixel in the flat array
  const uint32_t head = min((uint32_t)((0 - start) & 3), N);               // pixels in front of the frame's first whole group
  const uint32_t groups = (N - head) >> 2;
  const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
  const int32_t *lab = labels + start;
  uint8_t *img = image + 3 * start;
  if (g < groups) {
    const size_t p = (size_t)head + 4 * (size_t)g;                         // (start + p) % 4 == 0
    int32_t l[4];
    if constexpr (ALIGNED16) {
      const int4 v = *reinterpret_cast<const int4 *>(__builtin_assume_aligned(lab + p, 16));
      l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) l[j] = lab[p + j];
    }
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; j++) c[j] = colour_of(l[j], K, rcp, lut);
    uint32_t *o = reinterpret_cast<uint32_t *>(__builtin_assume_aligned(img + 3 * p, 4));
    o[0] = c[0] | (c[1] << 24);
    o[1] = (c[1] >> 8) | (c[2] << 16);
    o[2] = (c[2] >> 16) | (c[3] << 8);
  } else if (g == groups) {                                                // the frame's edges, byte-wise: at most 3 + 3 pixels
    const uint32_t tail0 = head + 4 * groups;
    for (uint32_t k = 0; k < head + (N - tail0); k++) {
      const uint32_t p = k < head ? k : tail0 + (k - head);
      const uint32_t c = colour_of(lab[p], K, rcp, lut);
      img[3 * (size_t)p] = (uint8_t)c; img[3 * (size_t)p + 1] = (uint8_t)(c >> 8); img[3 * (size_t)p + 2] = (uint8_t)(c >> 16);
    }
  }
}

}  // namespace

void launch_cluster_image(int W, int H, int frames, const int32_t *labels, const int32_t *n_clusters, const label_palette::Table &table,
                          uint8_t *image, hipStream_t s) {
  const uint32_t N = (uint32_t)W * (uint32_t)H;
  const dim3 grid((N / 4 + 1 + kBlock - 1) / kBlock, (unsigned)frames);    // N / 4 bounds a frame's whole groups; + 1: its edge lane
  if (((uintptr_t)labels & 15) == 0)
    hipLaunchKernelGGL(k_cluster_image<true>, grid, dim3(kBlock), 0, s, N, labels, n_clusters, table, image);
  else
    hipLaunchKernelGGL(k_cluster_image<false>, grid, dim3(kBlock), 0, s, N, labels, n_clusters, table, image);
}
