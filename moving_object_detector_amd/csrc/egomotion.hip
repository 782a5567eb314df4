// egomotion.hip — on-GPU stereo ego-motion: RANSAC over dense correspondences, then Gauss-Newton.
//
// Stands in for libviso2 (VisualOdometryStereo::process + getMotion(), scene_flow_constructor.cpp:214-256), which the reference
// runs on the CPU over sparse features.  It is NOT a port of libviso2 and claims no parity with it: it keeps the model (RANSAC on
// minimal samples, then Gauss-Newton on the stereo reprojection error of previous-frame 3D points seen in the current pair) and the
// output convention (prev -> now, P_now = R P_prev + t), and takes its correspondences from the disparity pair and the flow that
// are already in HBM.  Every step is fixed so that tests/models/ego_model.py restates it bit for bit.
// Kernels: correspondence count + compaction (per-block counts, then a scan: raster order, no order-dependent atomics), minimal
// solver per hypothesis, scoring (hypotheses in registers, correspondences streamed through LDS), and one workgroup per frame for
// the selection, the refinement and the output (ModTransform, ModEgoResult and, for the odometry stream, the frame's FrameConst).
#include "frame_const.h"
#include "mod_launch.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;        // samples per block of the correspondence kernels, hypotheses per block of the scoring kernel
constexpr int kHypBlock = 64;      // hypotheses per block of the minimal solver
constexpr int kChunk = 128;        // correspondences per block of the scoring kernel
constexpr int kRefine = 1024;      // threads of the refinement workgroup (16 waves)
constexpr int kTerms = 28;         // 21 upper entries of J^T J, 6 of J^T r, r^T r
constexpr double kCollinear = 1e-4;
constexpr double kConverged = 1e-10;

__device__ __forceinline__ bool disp_ok(float d, float lo, float hi) { return isfinite(d) && d >= lo && d <= hi && d > 0.0f; }

// Correspondence of grid sample g of frame f: P, Q, O when kept.
__device__ __forceinline__ bool ego_sample(const EgoArgs &a, int f, int g, double r[9]) {
  if (g >= a.gw * a.gh) return false;
  const int gy = g / a.gw, x = (g - gy * a.gw) * a.stride, y = gy * a.stride;
  const size_t N = (size_t)a.W * a.H, at = (size_t)f * N + (size_t)y * a.W + x;
  const float dn = a.dnow[at];
  const float fx = a.flow[2 * at], fy = a.flow[2 * at + 1];
  if (!disp_ok(dn, a.dlo, a.dhi) || !isfinite(fx) || !isfinite(fy)) return false;
  const float rx = roundf((float)x - fx), ry = roundf((float)y - fy);      // the rounding rule of sceneflow.hip (A6)
  if (!(rx >= 0.0f && rx < (float)a.W && ry >= 0.0f && ry < (float)a.H)) return false;
  const float dp = a.dprev[(size_t)f * N + (size_t)(int)ry * a.W + (int)rx];
  if (!disp_ok(dp, a.dlo, a.dhi)) return false;
  const double xd = (double)x, yd = (double)y;
  const double ux = xd - (double)fx, uy = yd - (double)fy;
  const double zp = a.fT / (double)dp;
  r[0] = ((ux - a.cx) - a.Tx) / a.fx * zp;
  r[1] = ((uy - a.cy) - a.Ty) / a.fy * zp;
  r[2] = zp;
  const double zn = a.fT / (double)dn;
  r[3] = ((xd - a.cx) - a.Tx) / a.fx * zn;
  r[4] = ((yd - a.cy) - a.Ty) / a.fy * zn;
  r[5] = zn;
  r[6] = xd; r[7] = yd; r[8] = xd - (double)dn;
  return true;
}

__device__ __forceinline__ int block_count(bool keep, int *sh) {
  const uint64_t b = __ballot(keep);
  if (threadIdx.x == 0) *sh = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) atomicAdd(sh, (int)__popcll(b));
  __syncthreads();
  return *sh;
}

__global__ __launch_bounds__(kBlock) void k_ego_count(EgoArgs a) {
  __shared__ int cnt;
  const int f = blockIdx.y, g = blockIdx.x * kBlock + threadIdx.x;
  double r[9];
  const int c = block_count(ego_sample(a, f, g, r), &cnt);
  if (threadIdx.x == 0) a.blkcnt[(size_t)f * gridDim.x + blockIdx.x] = c;
}

// block b of frame f writes its kept samples, in raster order, after those of blocks 0 .. b-1
__global__ __launch_bounds__(kBlock) void k_ego_compact(EgoArgs a) {
  __shared__ int base, wcnt[kBlock / 64];
  const int f = blockIdx.y, b = blockIdx.x, g = b * kBlock + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  int part = 0;
  for (int k = threadIdx.x; k < b; k += kBlock) part += a.blkcnt[(size_t)f * gridDim.x + k];
  if (part) atomicAdd(&base, part);                       // an integer sum: any order gives the same value
  double r[9];
  const bool keep = ego_sample(a, f, g, r);
  const uint64_t bal = __ballot(keep);
  if (lane == 0) wcnt[wave] = (int)__popcll(bal);
  __syncthreads();
  int off = base;
  for (int w = 0; w < wave; w++) off += wcnt[w];
  off += (int)__popcll(bal & ((1ull << lane) - 1));
  if (keep) {
    double *dst = a.corr + (size_t)f * 9 * a.cap + off;
#pragma unroll
    for (int k = 0; k < 9; k++) dst[(size_t)k * a.cap] = r[k];
  }
  if (b == (int)gridDim.x - 1 && threadIdx.x == kBlock - 1) {
    int total = base;
    for (int w = 0; w < kBlock / 64; w++) total += wcnt[w];
    a.ncorr[f] = total;
  }
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t v) {
  uint64_t z = v + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// orthonormal triad (e1, e2, e3) of three points; false when near-collinear
__device__ __forceinline__ bool ego_frame(const double p1[3], const double p2[3], const double p3[3], double e[3][3]) {
  double av[3], bv[3];
  for (int i = 0; i < 3; i++) { av[i] = p2[i] - p1[i]; bv[i] = p3[i] - p1[i]; }
  const double c[3] = {av[1] * bv[2] - av[2] * bv[1], av[2] * bv[0] - av[0] * bv[2], av[0] * bv[1] - av[1] * bv[0]};
  const double aa = (av[0] * av[0] + av[1] * av[1]) + av[2] * av[2];
  const double bb = (bv[0] * bv[0] + bv[1] * bv[1]) + bv[2] * bv[2];
  const double cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
  if (!(cc > (kCollinear * aa) * bb)) return false;
  const double na = sqrt(aa), nc = sqrt(cc);
  for (int i = 0; i < 3; i++) { e[0][i] = av[i] / na; e[2][i] = c[i] / nc; }
  e[1][0] = e[2][1] * e[0][2] - e[2][2] * e[0][1];
  e[1][1] = e[2][2] * e[0][0] - e[2][0] * e[0][2];
  e[1][2] = e[2][0] * e[0][1] - e[2][1] * e[0][0];
  return true;
}

__global__ __launch_bounds__(kHypBlock) void k_ego_hyp(EgoArgs a) {
  const int f = blockIdx.y, h = blockIdx.x * kHypBlock + threadIdx.x;
  if (h >= a.hyps) return;
  const int n = a.ncorr[f];
  int32_t *cnt = a.hcnt + (size_t)f * a.hyps + h;
  if (n < 3) { *cnt = -1; return; }
  int idx[3];
  for (int k = 0; k < 3; k++)
    idx[k] = (int)__umul64hi(splitmix64(((uint64_t)a.seed << 32) | (uint64_t)(4 * h + k)), (uint64_t)n);
  if (idx[0] == idx[1] || idx[0] == idx[2] || idx[1] == idx[2]) { *cnt = -1; return; }
  const double *cr = a.corr + (size_t)f * 9 * a.cap;
  double P[3][3], Q[3][3];
  for (int k = 0; k < 3; k++)
    for (int i = 0; i < 3; i++) { P[k][i] = cr[(size_t)i * a.cap + idx[k]]; Q[k][i] = cr[(size_t)(3 + i) * a.cap + idx[k]]; }
  double fp[3][3], fq[3][3];
  if (!ego_frame(P[0], P[1], P[2], fp) || !ego_frame(Q[0], Q[1], Q[2], fq)) { *cnt = -1; return; }
  double M[12];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) M[4 * i + j] = (fq[0][i] * fp[0][j] + fq[1][i] * fp[1][j]) + fq[2][i] * fp[2][j];
  double cp[3], cq[3];
  for (int i = 0; i < 3; i++) {
    cp[i] = ((P[0][i] + P[1][i]) + P[2][i]) / 3.0;
    cq[i] = ((Q[0][i] + Q[1][i]) + Q[2][i]) / 3.0;
  }
  for (int i = 0; i < 3; i++) M[4 * i + 3] = cq[i] - ((M[4 * i] * cp[0] + M[4 * i + 1] * cp[1]) + M[4 * i + 2] * cp[2]);
  double *dst = a.hyp + ((size_t)f * a.hyps + h) * 12;
  for (int k = 0; k < 12; k++) dst[k] = M[k];
  *cnt = 0;
}

// Residuals of P under the row-major 3 x 4 motion M against O; returns X, Y, Z, a = fx X + Tx, b = fy Y + Ty in w[0..4]
__device__ __forceinline__ void ego_residuals(const EgoArgs &a, const double M[12], const double P[3], const double O[3], double w[5],
                                              double &ru, double &rv, double &rr) {
  const double X = ((M[0] * P[0] + M[1] * P[1]) + M[2] * P[2]) + M[3];
  const double Y = ((M[4] * P[0] + M[5] * P[1]) + M[6] * P[2]) + M[7];
  const double Z = ((M[8] * P[0] + M[9] * P[1]) + M[10] * P[2]) + M[11];
  const double A = a.fx * X + a.Tx, B = a.fy * Y + a.Ty;
  const double u = A / Z + a.cx, v = B / Z + a.cy, ur = u - a.fT / Z;      // project3dToPixel, u_r = u_l - fT / Z
  ru = u - O[0]; rv = v - O[1]; rr = ur - O[2];
  w[0] = X; w[1] = Y; w[2] = Z; w[3] = A; w[4] = B;
}

__device__ __forceinline__ bool ego_inlier(const EgoArgs &a, const double M[12], const double P[3], const double O[3]) {
  double w[5], ru, rv, rr;
  ego_residuals(a, M, P, O, w, ru, rv, rr);
  return w[2] > 0.0 && fabs(ru) < a.th && fabs(rv) < a.th && fabs(rr) < a.th;
}

// grid (correspondence chunks, hypothesis blocks, frames): thread = hypothesis, the chunk's correspondences in LDS
__global__ __launch_bounds__(kBlock) void k_ego_score(EgoArgs a) {
  __shared__ double sp[6][kChunk];
  const int f = blockIdx.z, h = blockIdx.y * kBlock + threadIdx.x, i0 = blockIdx.x * kChunk;
  const int n = a.ncorr[f];
  if (i0 >= n) return;                                   // block-uniform
  const int m = min(kChunk, n - i0);
  const double *cr = a.corr + (size_t)f * 9 * a.cap + i0;
  for (int k = threadIdx.x; k < 6 * kChunk; k += kBlock) {
    const int comp = k / kChunk, j = k - comp * kChunk;
    if (j < m) sp[comp][j] = cr[(size_t)(comp < 3 ? comp : comp + 3) * a.cap + j];     // P, then O
  }
  __syncthreads();
  if (h >= a.hyps) return;
  int32_t *cnt = a.hcnt + (size_t)f * a.hyps + h;
  if (*cnt < 0) return;                                  // invalid hypothesis (valid counts only grow from 0)
  double M[12];
  const double *src = a.hyp + ((size_t)f * a.hyps + h) * 12;
#pragma unroll
  for (int k = 0; k < 12; k++) M[k] = src[k];
  int c = 0;
  for (int j = 0; j < m; j++) {
    const double P[3] = {sp[0][j], sp[1][j], sp[2][j]}, O[3] = {sp[3][j], sp[4][j], sp[5][j]};
    c += ego_inlier(a, M, P, O) ? 1 : 0;
  }
  if (c) atomicAdd(cnt, c);                              // integer counts: any order gives the same value
}

// adds the correspondence's 28 terms to acc (each term is formed first, then added: the model's per-thread sum)
__device__ __forceinline__ void ego_add_terms(const EgoArgs &a, const double M[12], const double P[3], const double O[3], double t[kTerms]) {
  double w[5], ru, rv, rr;
  ego_residuals(a, M, P, O, w, ru, rv, rr);
  const double X = w[0], Y = w[1], Z = w[2];
  const double iz = 1.0 / Z;
  const double ux = a.fx * iz, vy = a.fy * iz;
  const double gu = -((w[3] * iz) * iz), gv = -((w[4] * iz) * iz);
  const double gr = gu + (a.fT * iz) * iz;
  const double Ju[6] = {gu * Y, ux * Z - gu * X, -(ux * Y), ux, 0.0, gu};
  const double Jv[6] = {gv * Y - vy * Z, -(gv * X), vy * X, 0.0, vy, gv};
  const double Jr[6] = {gr * Y, ux * Z - gr * X, -(ux * Y), ux, 0.0, gr};
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = i; j < 6; j++, k++) t[k] = t[k] + ((Ju[i] * Ju[j] + Jv[i] * Jv[j]) + Jr[i] * Jr[j]);
#pragma unroll
  for (int i = 0; i < 6; i++) t[21 + i] = t[21 + i] + ((Ju[i] * ru + Jv[i] * rv) + Jr[i] * rr);
  t[27] = t[27] + ((ru * ru + rv * rv) + rr * rr);
}

// Fixed-order sum of Q per-thread partials: a tree within each wave (offsets 32 .. 1), then over the 16 wave sums (8 .. 1).
template <int Q>
__device__ __forceinline__ void ego_reduce(const double (&v)[Q], double (&red)[kRefine / 64][kTerms], double *out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < Q; k++) {
    double x = v[k];
#pragma unroll
    for (int off = 32; off; off >>= 1) x = x + __shfl_down(x, off, 64);
    if (lane == 0) red[wave][k] = x;
  }
  __syncthreads();
  if (threadIdx.x < Q) {
    double w[kRefine / 64];
#pragma unroll
    for (int i = 0; i < kRefine / 64; i++) w[i] = red[i][threadIdx.x];
#pragma unroll
    for (int off = kRefine / 128; off; off >>= 1)
#pragma unroll
      for (int i = 0; i < off; i++) w[i] = w[i] + w[i + off];
    out[threadIdx.x] = w[0];
  }
  __syncthreads();
}

// A x = -g, A symmetric 6 x 6 from its 21 upper entries; false when not positive definite / not finite
__device__ bool ego_cholesky(const double *s, double x[6]) {
  double A[6][6], L[6][6] = {};
  int k = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) { A[i][j] = s[k]; A[j][i] = s[k]; k++; }
  for (int j = 0; j < 6; j++) {
    double d = A[j][j];
    for (int q = 0; q < j; q++) d = d - L[j][q] * L[j][q];
    if (!(d > 0.0) || !isfinite(d)) return false;
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < 6; i++) {
      double e = A[i][j];
      for (int q = 0; q < j; q++) e = e - L[i][q] * L[j][q];
      L[i][j] = e / L[j][j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; i++) {
    double e = -s[21 + i];
    for (int q = 0; q < i; q++) e = e - L[i][q] * y[q];
    y[i] = e / L[i][i];
  }
  for (int i = 5; i >= 0; i--) {
    double e = y[i];
    for (int q = i + 1; q < 6; q++) e = e - L[q][i] * x[q];
    x[i] = e / L[i][i];
  }
  bool fin = true;
  for (int i = 0; i < 6; i++) fin = fin && isfinite(x[i]);
  return fin;
}

// R <- dR R, t <- dR t + tau, dR of the unit quaternion (w / 2, 1) / |(w / 2, 1)|
__device__ void ego_update(double M[12], const double d[6]) {
  const double hx = d[0] * 0.5, hy = d[1] * 0.5, hz = d[2] * 0.5;
  const double nn = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
  const double q[4] = {hx / nn, hy / nn, hz / nn, 1.0 / nn}, z3[3] = {0.0, 0.0, 0.0};
  double D[12], N[12];
  transform_to_rows(z3, q, D);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 4; j++) N[4 * i + j] = (D[4 * i] * M[j] + D[4 * i + 1] * M[4 + j]) + D[4 * i + 2] * M[8 + j];
    N[4 * i + 3] = N[4 * i + 3] + d[3 + i];
  }
  for (int k = 0; k < 12; k++) M[k] = N[k];
}

// tf2::Matrix3x3::getRotation (host/messages.hpp transform_from_motion) -> x, y, z, w
__device__ void ego_get_rotation(const double M[12], double q[4]) {
  auto m = [&](int i, int j) { return M[4 * i + j]; };
  const double trace = (m(0, 0) + m(1, 1)) + m(2, 2);
  if (trace > 0.0) {
    double s = sqrt(trace + 1.0);
    q[3] = s * 0.5;
    s = 0.5 / s;
    q[0] = (m(2, 1) - m(1, 2)) * s;
    q[1] = (m(0, 2) - m(2, 0)) * s;
    q[2] = (m(1, 0) - m(0, 1)) * s;
  } else {
    const int i = m(0, 0) < m(1, 1) ? (m(1, 1) < m(2, 2) ? 2 : 1) : (m(0, 0) < m(2, 2) ? 2 : 0);
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    double s = sqrt(((m(i, i) - m(j, j)) - m(k, k)) + 1.0);
    q[i] = s * 0.5;
    s = 0.5 / s;
    q[3] = (m(k, j) - m(j, k)) * s;
    q[j] = (m(j, i) + m(i, j)) * s;
    q[k] = (m(k, i) + m(i, k)) * s;
  }
}

__global__ __launch_bounds__(kRefine) void k_ego_refine(EgoArgs a) {
  __shared__ double red[kRefine / 64][kTerms];
  __shared__ double sum[kTerms];
  __shared__ double M[12];
  __shared__ unsigned long long best_key;
  __shared__ int count, status, steps, stop;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = a.ncorr[f];
  const int32_t *hc = a.hcnt + (size_t)f * a.hyps;
  if (tid == 0) { best_key = 0; count = 0; status = MOD_EGO_OK; steps = 0; stop = 0; }
  __syncthreads();
  // best hypothesis: most inliers, ties to the lowest h (key = (count + 1) << 32 | ~h; invalid ones count -1)
  unsigned long long key = 0;
  for (int h = tid; h < a.hyps; h += kRefine) {
    const unsigned long long k = ((unsigned long long)(uint32_t)(hc[h] + 1) << 32) | (uint32_t)~(uint32_t)h;
    key = k > key ? k : key;
  }
  atomicMax(&best_key, key);
  __syncthreads();
  const int best = (int)~(uint32_t)(best_key & 0xffffffffu), best_cnt = (int)(best_key >> 32) - 1;
  const int need = a.min_inliers > 1 ? a.min_inliers : 1;
  int inl = 0;
  const double *cr = a.corr + (size_t)f * 9 * a.cap;
  uint8_t *flag = a.flag + (size_t)f * a.cap;
  auto load = [&](int i, double P[3], double O[3]) {
    for (int k = 0; k < 3; k++) { P[k] = cr[(size_t)k * a.cap + i]; O[k] = cr[(size_t)(6 + k) * a.cap + i]; }
  };
  // inlier flags and count under the motion in M
  auto select = [&]() -> int {
    if (tid == 0) count = 0;
    __syncthreads();
    double Ml[12];
    for (int k = 0; k < 12; k++) Ml[k] = M[k];
    int c = 0;
    for (int i = tid; i < n; i += kRefine) {
      double P[3], O[3];
      load(i, P, O);
      const bool in = ego_inlier(a, Ml, P, O);
      flag[i] = in ? 1 : 0;
      c += in ? 1 : 0;
    }
    if (c) atomicAdd(&count, c);
    __syncthreads();
    const int total = count;
    __syncthreads();                                     // before the next select() clears it
    return total;
  };
  if (n < (a.min_inliers > 3 ? a.min_inliers : 3)) {
    if (tid == 0) status = MOD_EGO_FEW_POINTS;
  } else if (best_cnt < need) {
    if (tid == 0) status = MOD_EGO_FEW_INLIERS;
    inl = best_cnt > 0 ? best_cnt : 0;
  } else {
    if (tid < 12) M[tid] = a.hyp[((size_t)f * a.hyps + best) * 12 + tid];
    __syncthreads();
    const int first = (a.iterations + 1) / 2;
    for (int phase = 0; phase < 2 && status == MOD_EGO_OK; phase++) {
      inl = select();
      if (inl < need) { if (tid == 0) status = MOD_EGO_FEW_INLIERS; break; }
      if (tid == 0) stop = 0;
      __syncthreads();
      const int budget = phase == 0 ? first : a.iterations - first;
      for (int s = 0; s < budget && !stop; s++) {
        double Ml[12];
        for (int k = 0; k < 12; k++) Ml[k] = M[k];
        double acc[kTerms];
        for (int k = 0; k < kTerms; k++) acc[k] = 0.0;
        for (int i = tid; i < n; i += kRefine) {
          if (!flag[i]) continue;
          double P[3], O[3];
          load(i, P, O);
          ego_add_terms(a, Ml, P, O, acc);
        }
        ego_reduce<kTerms>(acc, red, sum);
        if (tid == 0) {
          double d[6];
          steps++;
          if (!ego_cholesky(sum, d)) { status = MOD_EGO_DIVERGED; stop = 1; }
          else {
            double Mn[12];
            for (int k = 0; k < 12; k++) Mn[k] = M[k];
            ego_update(Mn, d);
            for (int k = 0; k < 12; k++) M[k] = Mn[k];
            double mx = 0.0;
            for (int k = 0; k < 6; k++) mx = fabs(d[k]) > mx ? fabs(d[k]) : mx;
            if (mx < kConverged) stop = 1;
          }
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();                                       // status
  double rms = __builtin_nan("");
  if (status == MOD_EGO_OK) {
    inl = select();
    if (inl < need) { if (tid == 0) status = MOD_EGO_FEW_INLIERS; }
    else {
      double Ml[12];
      for (int k = 0; k < 12; k++) Ml[k] = M[k];
      double acc[1] = {0.0};
      for (int i = tid; i < n; i += kRefine) {
        if (!flag[i]) continue;
        double P[3], O[3], w[5], ru, rv, rr;
        load(i, P, O);
        ego_residuals(a, Ml, P, O, w, ru, rv, rr);
        acc[0] = acc[0] + ((ru * ru + rv * rv) + rr * rr);
      }
      ego_reduce<1>(acc, red, sum);
      rms = sqrt(sum[0] / (3.0 * (double)inl));
    }
  }
  __syncthreads();
  if (tid != 0) return;
  double t[3], q[4];
  bool ok = status == MOD_EGO_OK;
  if (ok) {
    for (int k = 0; k < 12; k++) ok = ok && isfinite(M[k]);
    if (!ok) status = MOD_EGO_DIVERGED;
  }
  if (ok) {
    for (int i = 0; i < 3; i++) t[i] = M[4 * i + 3];
    ego_get_rotation(M, q);
  } else {
    for (int i = 0; i < 3; i++) t[i] = __builtin_nan("");
    for (int i = 0; i < 4; i++) q[i] = __builtin_nan("");
    rms = __builtin_nan("");
  }
  double *tf = a.tf + (size_t)f * 7;
  for (int i = 0; i < 3; i++) tf[i] = t[i];
  for (int i = 0; i < 4; i++) tf[3 + i] = q[i];
  ModEgoResult r;
  r.status = status; r.correspondences = n; r.inliers = inl; r.iterations = steps; r.rms_px = rms;
  a.res[f] = r;
  if (a.fc) fill_frame_const(a.fc[f], t, q, a.dt);     // the odometry stream: the scene-flow kernel reads this copy
}

}  // namespace

int ego_grid_blocks(int gw, int gh) { return (gw * gh + kBlock - 1) / kBlock; }

void launch_egomotion(const EgoArgs &a, hipStream_t s) {
  const int G = a.gw * a.gh, nblk = ego_grid_blocks(a.gw, a.gh);
  hipLaunchKernelGGL(k_ego_count, dim3(nblk, a.frames), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(k_ego_compact, dim3(nblk, a.frames), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(k_ego_hyp, dim3((a.hyps + kHypBlock - 1) / kHypBlock, a.frames), dim3(kHypBlock), 0, s, a);
  hipLaunchKernelGGL(k_ego_score, dim3((G + kChunk - 1) / kChunk, (a.hyps + kBlock - 1) / kBlock, a.frames), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(k_ego_refine, dim3(a.frames), dim3(kRefine), 0, s, a);
}
