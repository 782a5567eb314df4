// flow_image.hip — the constructor's per-pixel debug views on the GPU: ~optical_flow, ~synthetic_optical_flow and
// ~depth (scene_flow_constructor.cpp:45-48,100,118,145) colour-coded into BGR8 where the estimators left their planes, and the static
// flow on device planes.
//
// k_flow_image reads flow [frames][N][2] (F32; RESIDUAL: and a second such plane, subtracted per component) and writes image
// [frames][N][3] (B, G, R, packed) by flow_color::flow_bgr; k_disparity_image reads disparity [frames][N] and writes the same by
// flow_color::disparity_bgr.  Memory-bound: 8 (16) or 4 B read and 3 B written per pixel.  The frame walk is k_cluster_image's
// (label_image.hip): the batch is one flat pixel array, a lane takes four consecutive pixels of the FLAT array's four-pixel grid —
// two (four) or one 16-byte load, the planes' bases permitting, else dwords, and 12 bytes stored as three whole dwords: the image's base is
// 4-byte aligned and four pixels are 12 bytes, so every group starts on a dword whatever N is.  Frames ride in blockIdx.z; a
// frame's lanes cover the groups that lie wholly inside it, and the up to three pixels in front of its first whole group and behind its
// last one are written byte-wise by one more lane of that frame (a row whose W is no multiple of 4 needs no path of its own: rows are
// not units here).  The palette (label_palette.h's built-in table) is spread into LDS, one dword an entry.
//
// k_static_flow is calculateStaticOpticalFlow alone (scene_flow_constructor.cpp:65-89) from a device transform: one
// lane per pixel.  Its pixel body restates, operation by operation, the static-flow block of sceneflow.hip's sf_stage1 — the fused
// kernel itself stays as it is (moving the block into a shared header changed that kernel's register allocation and schedule) — and
// the isometry's rows come from frame_const.h's transform_to_rows, the very text the host runs for mod_static_flow_host.
#include "exact_div.h"
#include "flow_color.h"
#include "frame_const.h"
#include "mod_launch.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
static_assert(kBlock == label_palette::kEntries, "one thread spreads one table entry");

struct Lut { const uint32_t *e; __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return e[i]; } };

// K consecutive floats at p: 16-byte loads when the plane's base allows it (p is then 16-byte aligned: see the frame walk)
template <int K, bool ALIGNED16> __device__ __forceinline__ void load_run(const float *p, float v[K]) {
  if constexpr (ALIGNED16) {
#pragma unroll
    for (int j = 0; j < K / 4; j++) {
      const float4 q = reinterpret_cast<const float4 *>(__builtin_assume_aligned(p, 16))[j];
      v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < K; j++) v[j] = p[j];
  }
}

// the pixels of a frame as the walk sees them: colour of pixel p, colours of the four pixels from p
template <bool RESIDUAL, bool ALIGNED16> struct FlowSource {
  const float *flow, *still;   // the frame's planes; still: RESIDUAL only
  float max_px;
  __device__ __forceinline__ uint32_t one(uint32_t p, Lut lut) const {
    float fx = flow[2 * (size_t)p], fy = flow[2 * (size_t)p + 1];
    if constexpr (RESIDUAL) { fx = fx - still[2 * (size_t)p]; fy = fy - still[2 * (size_t)p + 1]; }
    return flow_color::flow_bgr(fx, fy, max_px, lut);
  }
  __device__ __forceinline__ void four(uint32_t p, Lut lut, uint32_t c[4]) const {
    float v[8];
    load_run<8, ALIGNED16>(flow + 2 * (size_t)p, v);
    if constexpr (RESIDUAL) {
      float w[8];
      load_run<8, ALIGNED16>(still + 2 * (size_t)p, w);
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = v[j] - w[j];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) c[j] = flow_color::flow_bgr(v[2 * j], v[2 * j + 1], max_px, lut);
  }
};
template <bool ALIGNED16> struct DisparitySource {
  const float *disparity;
  float dmin, dmax;
  __device__ __forceinline__ uint32_t one(uint32_t p, Lut lut) const { return flow_color::disparity_bgr(disparity[p], dmin, dmax, lut); }
  __device__ __forceinline__ void four(uint32_t p, Lut lut, uint32_t c[4]) const {
    float v[4];
    load_run<4, ALIGNED16>(disparity + p, v);
#pragma unroll
    for (int j = 0; j < 4; j++) c[j] = flow_color::disparity_bgr(v[j], dmin, dmax, lut);
  }
};

// One frame of N pixels that starts `start` pixels into the flat batch: src and img are the frame's own
template <class Source> __device__ __forceinline__ void render_frame(uint32_t N, size_t start, const Source &src, uint8_t *img) {
  __shared__ uint32_t table[label_palette::kEntries];
  table[threadIdx.x] = label_palette::builtin_bgr(threadIdx.x);
  __syncthreads();
  const Lut lut{table};
  const uint32_t head = min((uint32_t)((0 - start) & 3), N);               // pixels in front of the frame's first whole group
  const uint32_t groups = (N - head) >> 2;
  const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
  if (g < groups) {
    const uint32_t p = head + 4 * g;                                       // (start + p) % 4 == 0; p + 3 < N
    uint32_t c[4];
    src.four(p, lut, c);
    uint32_t *o = reinterpret_cast<uint32_t *>(__builtin_assume_aligned(img + 3 * (size_t)p, 4));
    o[0] = c[0] | (c[1] << 24);
    o[1] = (c[1] >> 8) | (c[2] << 16);
    o[2] = (c[2] >> 16) | (c[3] << 8);
  } else if (g == groups) {                                                // the frame's edges, byte-wise: at most 3 + 3 pixels
    const uint32_t tail0 = head + 4 * groups;
    for (uint32_t k = 0; k < head + (N - tail0); k++) {
      const uint32_t p = k < head ? k : tail0 + (k - head);
      const uint32_t c = src.one(p, lut);
      img[3 * (size_t)p] = (uint8_t)c; img[3 * (size_t)p + 1] = (uint8_t)(c >> 8); img[3 * (size_t)p + 2] = (uint8_t)(c >> 16);
    }
  }
}

template <bool RESIDUAL, bool ALIGNED16>
__global__ __launch_bounds__(kBlock) void k_flow_image(uint32_t N, const float *__restrict__ flow, const float *__restrict__ still, float max_px,
                                                       uint8_t *__restrict__ image) {
  const size_t start = (size_t)blockIdx.z * N;
  const FlowSource<RESIDUAL, ALIGNED16> src{flow + 2 * start, RESIDUAL ? still + 2 * start : nullptr, max_px};
  render_frame(N, start, src, image + 3 * start);
}

template <bool ALIGNED16>
__global__ __launch_bounds__(kBlock) void k_disparity_image(uint32_t N, const float *__restrict__ disparity, float dmin, float dmax,
                                                            uint8_t *__restrict__ image) {
  const size_t start = (size_t)blockIdx.z * N;
  const DisparitySource<ALIGNED16> src{disparity + start, dmin, dmax};
  render_frame(N, start, src, image + 3 * start);
}

dim3 image_grid(uint32_t N, int frames) { return dim3((N / 4 + 1 + kBlock - 1) / kBlock, 1, (unsigned)frames); }   // N / 4 bounds a frame's whole groups; + 1: its edge lane

// ---- the static flow ----
__device__ __forceinline__ bool disp_in_range(const DevCam &c, float d) {
  // getDisparity range gate (disparity_image_processor.cpp:25-28): a NaN passes both tests.
  return !(c.dmax < d) && !(c.dmin > d);
}

// Rigid transform, Eigen association t + (p0 + (p1 + p2)) per row (see oracle/oracle.cpp iso_apply), result cast to F32.
__device__ __forceinline__ void iso_apply(const double m[12], float X, float Y, float Z, float &ox, float &oy, float &oz) {
  const double x = (double)X, y = (double)Y, z = (double)Z;
  ox = (float)(m[3] + (m[0] * x + (m[1] * y + m[2] * z)));
  oy = (float)(m[7] + (m[4] * x + (m[5] * y + m[6] * z)));
  oz = (float)(m[11] + (m[8] * x + (m[9] * y + m[10] * z)));
}

// Block = 64 x 4 threads, one pixel a lane, frames in blockIdx.z; transforms [frames] in HBM (ModTransform: t[3], q[4])
__global__ __launch_bounds__(256) void k_static_flow(DevCam c, const float *__restrict__ dprev, const ModTransform *__restrict__ transforms,
                                                     float2 *__restrict__ sflow) {
  __shared__ double rows[12];
  const int f = blockIdx.z;
  if (threadIdx.x == 0 && threadIdx.y == 0) transform_to_rows(transforms[f].t, transforms[f].q, rows);
  __syncthreads();
  const int x = blockIdx.x * 64 + threadIdx.x;
  const int y = blockIdx.y * 4 + threadIdx.y;
  if (x >= c.W || y >= c.H) return;
  double m[12];
#pragma unroll
  for (int i = 0; i < 12; i++) m[i] = rows[i];
  const size_t i = ((size_t)f * c.H + y) * c.W + x;
  const float dpo = dprev[i];
  const double rx = c.rayx[x], ry = c.rayy[y];
  const float nan = __uint_as_float(0x7fc00000u);
  // ---- sf_stage1's static flow at the own pixel: reproject prev, transform, project ----
  const float z = c.fT / dpo;                             // F32
  const double zd = (double)z;
  const float X = (float)(rx * zd);                       // F64 product -> F32
  const float Y = (float)(ry * zd);
  float tx, ty, tz;
  iso_apply(m, X, Y, z, tx, ty, tz);
  // project3dToPixel, F64: (fx X + Tx) / Z + cx and (fy Y + Ty) / Z + cy share one refined reciprocal of Z (exact_div.h)
  const double A = c.fx * (double)tx + c.Tx, B = c.fy * (double)ty + c.Ty, D = (double)tz;
  // the reference skips NaN points before and after the transform; a NaN X makes tx NaN, so one test covers both
  const bool ok = disp_in_range(c, dpo) & !(dpo == 0.0f) & !isnan(tx);
  double qa, qb;
  const bool fast = exact_div::div2_shared(A, B, D, qa, qb);
  if (__any(ok & !fast)) {                                // operands outside the window: IEEE divisions (rare, wave-uniform)
    qa = fast ? qa : A / D;
    qb = fast ? qb : B / D;
  }
  const double u = qa + c.cx, v = qb + c.cy;
  sflow[i] = make_float2(ok ? (float)(u - (double)x) : nan, ok ? (float)(v - (double)y) : nan);
}

}  // namespace

void launch_flow_image(int W, int H, int frames, const float *flow, const float *still, float max_px, uint8_t *image, hipStream_t s) {
  const uint32_t N = (uint32_t)W * (uint32_t)H;
  const dim3 grid = image_grid(N, frames);
  const bool aligned = (((uintptr_t)flow | (uintptr_t)still) & 15) == 0;
  if (still) {
    if (aligned) hipLaunchKernelGGL((k_flow_image<true, true>), grid, dim3(kBlock), 0, s, N, flow, still, max_px, image);
    else hipLaunchKernelGGL((k_flow_image<true, false>), grid, dim3(kBlock), 0, s, N, flow, still, max_px, image);
  } else {
    if (aligned) hipLaunchKernelGGL((k_flow_image<false, true>), grid, dim3(kBlock), 0, s, N, flow, still, max_px, image);
    else hipLaunchKernelGGL((k_flow_image<false, false>), grid, dim3(kBlock), 0, s, N, flow, still, max_px, image);
  }
}

void launch_disparity_image(int W, int H, int frames, const float *disparity, float dmin, float dmax, uint8_t *image, hipStream_t s) {
  const uint32_t N = (uint32_t)W * (uint32_t)H;
  const dim3 grid = image_grid(N, frames);
  if (((uintptr_t)disparity & 15) == 0) hipLaunchKernelGGL(k_disparity_image<true>, grid, dim3(kBlock), 0, s, N, disparity, dmin, dmax, image);
  else hipLaunchKernelGGL(k_disparity_image<false>, grid, dim3(kBlock), 0, s, N, disparity, dmin, dmax, image);
}

void launch_static_flow(const DevCam &c, int frames, const float *dprev, const ModTransform *transforms, float *static_flow, hipStream_t s) {
  const dim3 block(64, 4, 1), grid((c.W + 63) / 64, (c.H + 3) / 4, frames);
  hipLaunchKernelGGL(k_static_flow, grid, block, 0, s, c, dprev, transforms, reinterpret_cast<float2 *>(static_flow));
}
