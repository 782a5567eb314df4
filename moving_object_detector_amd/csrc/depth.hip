// depth.hip — depth images to the disparity planes everything downstream reads.
//
// An RGB-D camera delivers one image and one depth image (REP 118: 16UC1 millimetres with 0 = no reading, 32FC1 metres with NaN = no
// reading).  The scene-flow, ego-motion and cluster kernels work from disparity alone, so the estimator stage of such a camera is a
// conversion: d = fT / z, with fT the F32 product disp_f * disp_T the scene-flow kernel divides by (DevCam.fT).
//
// k_depth_to_disparity (the plain path: the depth image is aligned to the image camera) reads the camera-sized window (W x H) at
// (x0, y0) of each depth message of a batch (row pitch `step`, frames stacked at step * message height bytes) and writes packed planes
// [frames][H][W] f32.  Memory-bound: 2 or 4 bytes in, 4 out per pixel.  Each lane makes one run of 8 consecutive pixels of one row,
// placed on the OUTPUT's 32-byte grid (two aligned 16-byte stores); the source of a run is loaded as 16-byte words where its address
// allows, as dwords where it is 4-byte aligned, and — a 16UC1 run that starts half-way into a dword (odd x0 + head) — as the dwords
// around it shifted into place with v_alignbyte.  Runs cut by a row end, and the half-way runs next to one, take the scalar path.
//
// k_depth_register + k_zbuffer_to_disparity (the registered path: the depth camera has its own intrinsics and pose) scatter every
// valid sample of the WHOLE message into a z-buffer of the camera's size, f64 in the operation order include/mod_sf.h states, and
// keep the nearest sample of every target with a 32-bit atomicMin on the bit pattern of (float)Z: positive floats order like their
// unsigned patterns and the all-ones word (no float a sample can produce) stands for "empty", so the minimum does not depend on the
// order the atomics arrive in.  Holes stay holes.  No LDS; frames in blockIdx.z.
//
// k_depth_register_splat (mod_set_depth_splat, opt-in) is k_depth_register for a depth camera of fewer pixels than the image camera:
// besides its point every sample paints its footprint, the target centres inside the bounding box of its four projected corners
// (at most MOD_DEPTH_SPLAT_MAX per axis), with the same atomicMin and the same (float)Z.  One lane per sample; the off path's kernel
// is untouched.
//
// k_depth_rays + k_depth_register_rays / k_depth_register_splat_rays (mod_set_depth_distortion, opt-in) are the registered path for a
// depth camera with a lens: k_depth_rays tabulates the undistorted ray of every pixel centre and pixel corner once per calibration
// (csrc/depth_rays.h holds the arithmetic), and the two kernels are the two above with X0 = x * Z0, Y0 = y * Z0 from those tables in
// the pinhole's place.  The host chooses them where it chooses the splat kernel; the kernels above are untouched.
#include "mod_launch.h"

namespace {

constexpr int kRun = 8;       // output pixels per lane
constexpr int kBlock = 256;
constexpr uint32_t kEmpty = 0xffffffffu;

template <int Enc> constexpr int kBytes = Enc == MOD_DEPTH_16UC1 ? 2 : 4;

// valid iff z > 0 and finite (0, -0.0, negatives, NaN, +-inf are not): d = fT / z, else `invalid` (min_disparity - 1)
__device__ __forceinline__ float to_disparity(float z, float fT, float invalid) {
  const bool ok = z > 0.0f && z < __builtin_inff();
  return ok ? fT / z : invalid;
}

template <int Enc>
__device__ __forceinline__ float sample_z(const uint8_t *p, float unit) {
  if constexpr (Enc == MOD_DEPTH_16UC1) return (float)*reinterpret_cast<const uint16_t *>(p) * unit;
  else return *reinterpret_cast<const float *>(p) * unit;
}

// sample k of a run held in dwords d[] (little-endian)
template <int Enc, int N>
__device__ __forceinline__ float run_z(const uint32_t (&d)[N], int k, float unit) {
  if constexpr (Enc == MOD_DEPTH_16UC1) return (float)((d[k >> 1] >> ((k & 1) * 16)) & 0xffffu) * unit;
  else return __uint_as_float(d[k]) * unit;
}

//   runs         runs per row: (W + 7) / 8 + 1 (run r covers x in [head + 8 (r - 1), head + 8 r), head = pixels of the row in front of
//                the output's first 32-byte boundary)
//   frame_bytes  step * message height
template <int Enc>
__global__ __launch_bounds__(kBlock) void k_depth_to_disparity(int W, int H, int runs, const uint8_t *__restrict__ src, size_t frame_bytes,
                                                               int step, int x0, int y0, float unit, float fT, float invalid,
                                                               float *__restrict__ dst) {
  constexpr int B = kBytes<Enc>, NW = kRun * B / 4;   // dwords of a run
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= runs * H) return;
  const int y = i / runs, r = i - y * runs;
  const int f = blockIdx.z;
  const uint8_t *row = src + (size_t)f * frame_bytes + (size_t)(y0 + y) * step + (size_t)x0 * B;   // the window's row
  float *out = dst + ((size_t)f * H + y) * W;
  const int head = (int)(((0u - (uint32_t)(uintptr_t)out) & 31u) >> 2);
  const int xs = head + (r - 1) * kRun;
  if (xs >= 0 && xs + kRun <= W) {
    const uint8_t *s = row + (ptrdiff_t)xs * B;
    const uint32_t a = (uint32_t)(uintptr_t)s;
    uint32_t d[NW];
    bool loaded = true;
    if ((a & 15u) == 0) {
      const uint4 *p = reinterpret_cast<const uint4 *>(s);
#pragma unroll
      for (int k = 0; k < NW / 4; k++) {
        const uint4 q = p[k];
        d[4 * k] = q.x; d[4 * k + 1] = q.y; d[4 * k + 2] = q.z; d[4 * k + 3] = q.w;
      }
    } else if ((a & 3u) == 0) {
      const uint32_t *p = reinterpret_cast<const uint32_t *>(s);
#pragma unroll
      for (int k = 0; k < NW; k++) d[k] = p[k];
    } else if (B == 2 && xs >= 1 && xs + kRun + 1 <= W) {   // half-way into a dword: the sample on either side is the window's too
      const uint32_t *p = reinterpret_cast<const uint32_t *>(s - 2);
      uint32_t w[NW + 1];
#pragma unroll
      for (int k = 0; k < NW + 1; k++) w[k] = p[k];
#pragma unroll
      for (int k = 0; k < NW; k++) d[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], 2);
    } else {
      loaded = false;
    }
    if (loaded) {
      float o[kRun];
#pragma unroll
      for (int k = 0; k < kRun; k++) o[k] = to_disparity(run_z<Enc>(d, k, unit), fT, invalid);
      float4 *q = reinterpret_cast<float4 *>(__builtin_assume_aligned(out + xs, 16));
      q[0] = make_float4(o[0], o[1], o[2], o[3]);
      q[1] = make_float4(o[4], o[5], o[6], o[7]);
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < kRun; k++) {
    const int x = xs + k;
    if (x >= 0 && x < W) out[x] = to_disparity(sample_z<Enc>(row + (size_t)x * B, unit), fT, invalid);
  }
}

// One lane per sample (U, V) of the whole width x height message; zbuf [frames][H][W] holds kEmpty on entry.
template <int Enc>
__global__ __launch_bounds__(kBlock) void k_depth_register(int width, const uint8_t *__restrict__ src, size_t frame_bytes, int step, float unit,
                                                           DepthRegArgs g, int W, int H, uint32_t *__restrict__ zbuf) {
  const int U = blockIdx.x * kBlock + threadIdx.x, V = blockIdx.y, f = blockIdx.z;
  if (U >= width) return;
  const float z = sample_z<Enc>(src + (size_t)f * frame_bytes + (size_t)V * step + (size_t)U * kBytes<Enc>, unit);
  if (!(z > 0.0f && z < __builtin_inff())) return;
  const double Z0 = (double)z;
  const double X0 = (((double)U - g.cxd) * Z0) / g.fxd, Y0 = (((double)V - g.cyd) * Z0) / g.fyd;
  const double X = ((g.R[0] * X0 + g.R[1] * Y0) + g.R[2] * Z0) + g.t[0];
  const double Y = ((g.R[3] * X0 + g.R[4] * Y0) + g.R[5] * Z0) + g.t[1];
  const double Z = ((g.R[6] * X0 + g.R[7] * Y0) + g.R[8] * Z0) + g.t[2];
  if (!(Z > 0.0 && Z < __builtin_inf())) return;
  const double a = ((g.fx * X + g.Tx) / Z + g.cx) + 0.5, b = ((g.fy * Y + g.Ty) / Z + g.cy) + 0.5;
  if (!(a >= 0.0 && a < (double)W && b >= 0.0 && b < (double)H)) return;   // as doubles, before any conversion (NaN fails)
  const int ui = (int)floor(a), vi = (int)floor(b);                        // 0 <= ui < W, 0 <= vi < H by the test above
  atomicMin(zbuf + ((size_t)f * H + vi) * W + ui, __float_as_uint((float)Z));
}

// the header's chain for message position (u, v) at depth Z0: the point in the image camera's frame
__device__ __forceinline__ void to_image_frame(const DepthRegArgs &g, double u, double v, double Z0, double &X, double &Y, double &Z) {
  const double X0 = ((u - g.cxd) * Z0) / g.fxd, Y0 = ((v - g.cyd) * Z0) / g.fyd;
  X = ((g.R[0] * X0 + g.R[1] * Y0) + g.R[2] * Z0) + g.t[0];
  Y = ((g.R[3] * X0 + g.R[4] * Y0) + g.R[5] * Z0) + g.t[1];
  Z = ((g.R[6] * X0 + g.R[7] * Y0) + g.R[8] * Z0) + g.t[2];
}

__device__ __forceinline__ bool positive_finite(double v) { return v > 0.0 && v < __builtin_inf(); }
__device__ __forceinline__ bool is_finite(double v) { return fabs(v) < __builtin_inf(); }   // NaN fails

// k_depth_register with the footprint of every sample (include/mod_sf.h, "the footprint").  One lane per sample: the four corners
// share the sample's Z0 and two values each of X0 and Y0, so the compiler keeps one copy of every product the corners have in common,
// and the lane then walks its own rectangle of at most kSplatMax x kSplatMax targets.  Neighbouring lanes paint neighbouring
// rectangles of the same rows, so iteration (dv, du) of a wave is one atomic instruction over one or two stretches of z-buffer rows.
constexpr int kSplatMax = MOD_DEPTH_SPLAT_MAX;

template <int Enc>
__global__ __launch_bounds__(kBlock) void k_depth_register_splat(int width, const uint8_t *__restrict__ src, size_t frame_bytes, int step, float unit,
                                                                 DepthRegArgs g, int W, int H, uint32_t *__restrict__ zbuf) {
  const int U = blockIdx.x * kBlock + threadIdx.x, V = blockIdx.y, f = blockIdx.z;
  if (U >= width) return;
  const float z = sample_z<Enc>(src + (size_t)f * frame_bytes + (size_t)V * step + (size_t)U * kBytes<Enc>, unit);
  if (!(z > 0.0f && z < __builtin_inff())) return;
  const double Z0 = (double)z;
  double X, Y, Z;
  to_image_frame(g, (double)U, (double)V, Z0, X, Y, Z);
  if (!positive_finite(Z)) return;                                          // no zf: neither point nor footprint
  const uint32_t zf = __float_as_uint((float)Z);
  uint32_t *const plane = zbuf + (size_t)f * H * W;
  // a. the point, as k_depth_register
  const double a = ((g.fx * X + g.Tx) / Z + g.cx) + 0.5, b = ((g.fy * Y + g.Ty) / Z + g.cy) + 0.5;
  if (a >= 0.0 && a < (double)W && b >= 0.0 && b < (double)H) atomicMin(plane + (size_t)(int)floor(b) * W + (int)floor(a), zf);
  // b. the footprint: corners (-,-), (-,+), (+,-), (+,+) of (U, V), all at Z0
  double p[4], q[4];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    double Xc, Yc, Zc;
    to_image_frame(g, (double)U + (k & 2 ? 0.5 : -0.5), (double)V + (k & 1 ? 0.5 : -0.5), Z0, Xc, Yc, Zc);
    ok &= positive_finite(Zc);
    p[k] = (g.fx * Xc + g.Tx) / Zc + g.cx;
    q[k] = (g.fy * Yc + g.Ty) / Zc + g.cy;
    ok &= is_finite(p[k]) & is_finite(q[k]);                                      // a non-finite corner makes a non-finite bound (NaN propagates)
  }
  if (!ok) return;
  double ulo = ceil(fmin(fmin(p[0], p[1]), fmin(p[2], p[3]))), uhi = ceil(fmax(fmax(p[0], p[1]), fmax(p[2], p[3]))) - 1.0;
  double vlo = ceil(fmin(fmin(q[0], q[1]), fmin(q[2], q[3]))), vhi = ceil(fmax(fmax(q[0], q[1]), fmax(q[2], q[3]))) - 1.0;
  if ((uhi - ulo) + 1.0 > (double)kSplatMax || (vhi - vlo) + 1.0 > (double)kSplatMax) return;   // before clipping: the point alone
  ulo = fmax(ulo, 0.0); uhi = fmin(uhi, (double)(W - 1));
  vlo = fmax(vlo, 0.0); vhi = fmin(vhi, (double)(H - 1));
  if (ulo > uhi || vlo > vhi) return;
  const int u0 = (int)ulo, u1 = (int)uhi, v0 = (int)vlo, v1 = (int)vhi;       // 0 <= u0 <= u1 < W, 0 <= v0 <= v1 < H, at most kSplatMax apart
  for (int v = v0; v <= v1; v++)
    for (int u = u0; u <= u1; u++) atomicMin(plane + (size_t)v * W + u, zf);
}

// ---- a depth camera with a lens (mod_set_depth_distortion): the ray tables and the kernels that read them --------------------------
// One lane per lattice entry (i, j) of a table [rows][cols]: depth_rays::entry at (i + offset, j + offset), straight-line f64 (the
// iteration is unrolled), one 16-byte store.  Launched once per lattice: offset 0 over width x height (pixel centres), offset -0.5
// over (width + 1) x (height + 1) (pixel corners).  Runs once per calibration and message size, not per frame.
__global__ __launch_bounds__(kBlock) void k_depth_rays(depth_rays::Lens lens, double offset, int cols, int rows, double2 *__restrict__ table) {
  const int i = blockIdx.x * kBlock + threadIdx.x, j = blockIdx.y;
  if (i >= cols || j >= rows) return;
  double x, y;
  depth_rays::entry(lens, (double)i + offset, (double)j + offset, x, y);
  table[(size_t)j * cols + i] = make_double2(x, y);
}

// the header's chain with the table's ray in the pinhole's place: X0 = x * Z0, Y0 = y * Z0 (an invalid ray is NaN, and so is its Z)
__device__ __forceinline__ void ray_to_image_frame(const DepthRegArgs &g, double2 r, double Z0, double &X, double &Y, double &Z) {
  const double X0 = r.x * Z0, Y0 = r.y * Z0;
  X = ((g.R[0] * X0 + g.R[1] * Y0) + g.R[2] * Z0) + g.t[0];
  Y = ((g.R[3] * X0 + g.R[4] * Y0) + g.R[5] * Z0) + g.t[1];
  Z = ((g.R[6] * X0 + g.R[7] * Y0) + g.R[8] * Z0) + g.t[2];
}

// k_depth_register with X0, Y0 from the centre table `rays` [height][width]: consecutive lanes are consecutive U of one row, so the
// ray is one coalesced 16-byte load per lane.  Everything behind X0, Y0 is k_depth_register's, word for word.
template <int Enc>
__global__ __launch_bounds__(kBlock) void k_depth_register_rays(int width, const uint8_t *__restrict__ src, size_t frame_bytes, int step, float unit,
                                                                DepthRegArgs g, const double2 *__restrict__ rays, int W, int H,
                                                                uint32_t *__restrict__ zbuf) {
  const int U = blockIdx.x * kBlock + threadIdx.x, V = blockIdx.y, f = blockIdx.z;
  if (U >= width) return;
  const float z = sample_z<Enc>(src + (size_t)f * frame_bytes + (size_t)V * step + (size_t)U * kBytes<Enc>, unit);
  if (!(z > 0.0f && z < __builtin_inff())) return;
  const double2 r = rays[(size_t)V * width + U];                            // one 16-byte load
  double X, Y, Z;
  ray_to_image_frame(g, r, (double)z, X, Y, Z);
  if (!(Z > 0.0 && Z < __builtin_inf())) return;                            // (an invalid ray has a NaN Z: the sample is dropped here)
  const double a = ((g.fx * X + g.Tx) / Z + g.cx) + 0.5, b = ((g.fy * Y + g.Ty) / Z + g.cy) + 0.5;
  if (!(a >= 0.0 && a < (double)W && b >= 0.0 && b < (double)H)) return;   // as doubles, before any conversion (NaN fails)
  const int ui = (int)floor(a), vi = (int)floor(b);                        // 0 <= ui < W, 0 <= vi < H by the test above
  atomicMin(zbuf + ((size_t)f * H + vi) * W + ui, __float_as_uint((float)Z));
}

// k_depth_register_splat with the point's ray from `rays` and the four corner rays from `corners` [height + 1][width + 1]: entries
// [V][U], [V + 1][U], [V][U + 1], [V + 1][U + 1] are the corners (-,-), (-,+), (+,-), (+,+) of (U, V).  A wave reads two row segments
// of the corner table, and each entry serves the two lanes on either side of it through the cache.  A footprint with an invalid
// corner ray is dropped (its Zc is NaN); its point stays.  Everything behind X0, Y0 is k_depth_register_splat's, word for word.
template <int Enc>
__global__ __launch_bounds__(kBlock) void k_depth_register_splat_rays(int width, const uint8_t *__restrict__ src, size_t frame_bytes, int step, float unit,
                                                                      DepthRegArgs g, const double2 *__restrict__ rays,
                                                                      const double2 *__restrict__ corners, int W, int H, uint32_t *__restrict__ zbuf) {
  const int U = blockIdx.x * kBlock + threadIdx.x, V = blockIdx.y, f = blockIdx.z;
  if (U >= width) return;
  const float z = sample_z<Enc>(src + (size_t)f * frame_bytes + (size_t)V * step + (size_t)U * kBytes<Enc>, unit);
  if (!(z > 0.0f && z < __builtin_inff())) return;
  const double Z0 = (double)z;
  const double2 r = rays[(size_t)V * width + U];                            // one 16-byte load
  double X, Y, Z;
  ray_to_image_frame(g, r, Z0, X, Y, Z);
  if (!positive_finite(Z)) return;                                          // no zf (an invalid ray has a NaN Z): neither point nor footprint
  const uint32_t zf = __float_as_uint((float)Z);
  uint32_t *const plane = zbuf + (size_t)f * H * W;
  // a. the point, as k_depth_register_rays
  const double a = ((g.fx * X + g.Tx) / Z + g.cx) + 0.5, b = ((g.fy * Y + g.Ty) / Z + g.cy) + 0.5;
  if (a >= 0.0 && a < (double)W && b >= 0.0 && b < (double)H) atomicMin(plane + (size_t)(int)floor(b) * W + (int)floor(a), zf);
  // b. the footprint: corners (-,-), (-,+), (+,-), (+,+) of (U, V), all at Z0
  const double2 *const c0 = corners + (size_t)V * (width + 1) + U, *const c1 = c0 + (width + 1);
  const double2 cr[4] = {c0[0], c1[0], c0[1], c1[1]};
  double p[4], q[4];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    double Xc, Yc, Zc;
    ray_to_image_frame(g, cr[k], Z0, Xc, Yc, Zc);
    ok &= positive_finite(Zc);                                                    // (an invalid corner ray fails here)
    p[k] = (g.fx * Xc + g.Tx) / Zc + g.cx;
    q[k] = (g.fy * Yc + g.Ty) / Zc + g.cy;
    ok &= is_finite(p[k]) & is_finite(q[k]);                                      // a non-finite corner makes a non-finite bound (NaN propagates)
  }
  if (!ok) return;
  double ulo = ceil(fmin(fmin(p[0], p[1]), fmin(p[2], p[3]))), uhi = ceil(fmax(fmax(p[0], p[1]), fmax(p[2], p[3]))) - 1.0;
  double vlo = ceil(fmin(fmin(q[0], q[1]), fmin(q[2], q[3]))), vhi = ceil(fmax(fmax(q[0], q[1]), fmax(q[2], q[3]))) - 1.0;
  if ((uhi - ulo) + 1.0 > (double)kSplatMax || (vhi - vlo) + 1.0 > (double)kSplatMax) return;   // before clipping: the point alone
  ulo = fmax(ulo, 0.0); uhi = fmin(uhi, (double)(W - 1));
  vlo = fmax(vlo, 0.0); vhi = fmin(vhi, (double)(H - 1));
  if (ulo > uhi || vlo > vhi) return;
  const int u0 = (int)ulo, u1 = (int)uhi, v0 = (int)vlo, v1 = (int)vhi;       // 0 <= u0 <= u1 < W, 0 <= v0 <= v1 < H, at most kSplatMax apart
  for (int v = v0; v <= v1; v++)
    for (int u = u0; u <= u1; u++) atomicMin(plane + (size_t)v * W + u, zf);
}

// n words of z-buffer -> n disparities, four per lane (16-byte accesses when dst allows; zbuf is the context's own allocation)
__global__ __launch_bounds__(kBlock) void k_zbuffer_to_disparity(size_t n, const uint32_t *__restrict__ zbuf, float fT, float invalid,
                                                                 float *__restrict__ dst) {
  const size_t i = 4 * ((size_t)blockIdx.x * kBlock + threadIdx.x);
  if (i >= n) return;
  if (i + 4 <= n && ((uintptr_t)dst & 15u) == 0) {
    const uint4 q = *reinterpret_cast<const uint4 *>(zbuf + i);
    *reinterpret_cast<float4 *>(dst + i) = make_float4(q.x == kEmpty ? invalid : fT / __uint_as_float(q.x), q.y == kEmpty ? invalid : fT / __uint_as_float(q.y),
                                                       q.z == kEmpty ? invalid : fT / __uint_as_float(q.z), q.w == kEmpty ? invalid : fT / __uint_as_float(q.w));
    return;
  }
  for (size_t k = i; k < n && k < i + 4; k++) {
    const uint32_t q = zbuf[k];
    dst[k] = q == kEmpty ? invalid : fT / __uint_as_float(q);
  }
}

template <int Enc>
void launch_plain(int W, int H, int frames, const void *src, size_t frame_bytes, int step, int x0, int y0, float unit, float fT, float invalid,
                  float *dst, hipStream_t s) {
  const int runs = (W + kRun - 1) / kRun + 1;
  const dim3 grid((unsigned)(((size_t)runs * H + kBlock - 1) / kBlock), 1, (unsigned)frames);
  hipLaunchKernelGGL(k_depth_to_disparity<Enc>, grid, dim3(kBlock), 0, s, W, H, runs, static_cast<const uint8_t *>(src), frame_bytes, step, x0, y0,
                     unit, fT, invalid, dst);
}

template <int Enc>
void launch_register(int W, int H, int frames, const void *src, int width, int height, int step, float unit, const DepthRegArgs &g, bool splat,
                     const DepthRayTables &rays, uint32_t *zbuf, hipStream_t s) {
  const dim3 grid((unsigned)((width + kBlock - 1) / kBlock), (unsigned)height, (unsigned)frames);
  const uint8_t *const msg = static_cast<const uint8_t *>(src);
  const size_t frame_bytes = (size_t)step * height;
  if (rays.centres && splat) {
    hipLaunchKernelGGL(k_depth_register_splat_rays<Enc>, grid, dim3(kBlock), 0, s, width, msg, frame_bytes, step, unit, g, rays.centres, rays.corners, W, H, zbuf);
  } else if (rays.centres) {
    hipLaunchKernelGGL(k_depth_register_rays<Enc>, grid, dim3(kBlock), 0, s, width, msg, frame_bytes, step, unit, g, rays.centres, W, H, zbuf);
  } else {
    const auto kernel = splat ? k_depth_register_splat<Enc> : k_depth_register<Enc>;
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, width, msg, frame_bytes, step, unit, g, W, H, zbuf);
  }
}

}  // namespace

int depth_bytes(int encoding) { return encoding == MOD_DEPTH_16UC1 ? 2 : encoding == MOD_DEPTH_32FC1 ? 4 : 0; }

void launch_depth_to_disparity(int encoding, int W, int H, int frames, const void *src, size_t frame_bytes, int step, int x0, int y0, float unit,
                               float fT, float invalid, float *dst, hipStream_t s) {
  if (encoding == MOD_DEPTH_16UC1) launch_plain<MOD_DEPTH_16UC1>(W, H, frames, src, frame_bytes, step, x0, y0, unit, fT, invalid, dst, s);
  else if (encoding == MOD_DEPTH_32FC1) launch_plain<MOD_DEPTH_32FC1>(W, H, frames, src, frame_bytes, step, x0, y0, unit, fT, invalid, dst, s);
}

hipError_t launch_depth_register(int encoding, int W, int H, int frames, const void *src, int width, int height, int step, float unit,
                                 const DepthRegArgs &g, bool splat, const DepthRayTables &rays, float fT, float invalid, uint32_t *zbuf,
                                 float *dst, hipStream_t s) {
  if (rays.centres && splat && !rays.corners) return hipErrorInvalidValue;   // (the caller builds both tables for the splat)
  const size_t n = (size_t)frames * W * H;
  const hipError_t e = hipMemsetAsync(zbuf, 0xff, 4 * n, s);
  if (e != hipSuccess) return e;
  if (encoding == MOD_DEPTH_16UC1) launch_register<MOD_DEPTH_16UC1>(W, H, frames, src, width, height, step, unit, g, splat, rays, zbuf, s);
  else if (encoding == MOD_DEPTH_32FC1) launch_register<MOD_DEPTH_32FC1>(W, H, frames, src, width, height, step, unit, g, splat, rays, zbuf, s);
  hipLaunchKernelGGL(k_zbuffer_to_disparity, dim3((unsigned)((n + 4 * kBlock - 1) / (4 * kBlock))), dim3(kBlock), 0, s, n, zbuf, fT, invalid, dst);
  return hipSuccess;
}

hipError_t launch_depth_rays(const depth_rays::Lens &lens, double offset, int cols, int rows, double2 *table, hipStream_t s) {
  hipLaunchKernelGGL(k_depth_rays, dim3((unsigned)((cols + kBlock - 1) / kBlock), (unsigned)rows), dim3(kBlock), 0, s, lens, offset, cols, rows, table);
  return hipGetLastError();
}
