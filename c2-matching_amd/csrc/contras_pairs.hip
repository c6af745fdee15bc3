// contras_pairs.hip -- the training pairs of C2-Matching's stage 1-2 extractor training, made on the device from a batch
// of uint8 crops (the reference builds them on the host, one sample at a time: mmsr/data/contras_dataset.py:13-92, 150-229).
//
//   c2m_warp_perspective_u8   cv2.warpPerspective(img, H_inverse) + the float64 grid of transformed coordinates
//                             (np.dot(H_inverse, coordinate) / its third row), one launch for the batch;
//   c2m_pil_bicubic_u8        one axis of PIL.Image.resize(..., BICUBIC) on 8-bit planes, in Pillow's integer arithmetic.
//
// The warp's rule (bilinear on a 1/32-pixel position grid, constant zero border) is stated at the kernel.  It is OpenCV's
// INTER_LINEAR as far as the authors know it; parity with OpenCV is unpinned (OpenCV is not available where this is built
// and tested).  What training needs holds by construction: image and coordinates describe the same map.
//
// Both kernels give each thread a run of four pixels along x: 4-byte stores of uint8, 16-byte stores of fp32 and of the
// float64 coordinates.  The vector forms need rows that start on a 4-pixel boundary (W % 4 == 0) and 16-byte-aligned
// bases; any other geometry takes the same arithmetic with scalar stores.  The gathers of the warp move by a few pixels
// from one destination pixel to the next and stay in L1 / L2.
#include "c2m_common.h"

namespace c2m {
namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kRun = 4;          // pixels per thread along x
constexpr int kThreadsCP = 256;
constexpr int kPosBits = 5;      // positions are rounded to 1/32 pixel
constexpr int kCoeffBits = 22;   // Pillow's PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ int sat_rint_i32(double v) {
  // round half to even, then saturate (a NaN takes the lower bound: fmax returns the other operand)
  const double r = fmin(fmax(rint(v), -2147483648.0), 2147483647.0);
  return (int)r;
}

__device__ __forceinline__ uint32_t pack_u8x4(const uint8_t* v) {
  return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
}

// ---- perspective warp + transformed coordinates ---------------------------------------------------------------------
// src [B][3][H][W] uint8, M / Mi [B][3][3] float64 (Mi = inv(M), inverted on the host).  For destination pixel (x, y):
//   (X, Y, Wd) = Mi . (x, y, 1) in float64;  sx = rint(32 X / Wd), sy = rint(32 Y / Wd) (half to even, saturated to int32;
//   0 if Wd == 0);  x0 = sx >> 5, a = (sx & 31) / 32, y0 = sy >> 5, b = (sy & 31) / 32;
//   dst = s00 (1-a)(1-b) + s01 a(1-b) + s10 (1-a) b + s11 a b in fp32, in that order, with s = u8 / 255 (fp32) and 0 for a
//   tap outside the image.  The four weights are multiples of 1/1024 and exact; dst_u8 = trunc(dst * 255.0f).
//   coords[b][y][x][:] = M . (x, y, 1) / its third component, float64.
template <bool VEC>
__global__ __launch_bounds__(kThreadsCP) void warp_perspective_kernel(const uint8_t* __restrict__ src,
                                                                      const double* __restrict__ M,
                                                                      const double* __restrict__ Mi, int B, int H, int W,
                                                                      int runs, float* __restrict__ dst_f32,
                                                                      uint8_t* __restrict__ dst_u8,
                                                                      double* __restrict__ coords) {
  const long long g = (long long)blockIdx.x * kThreadsCP + threadIdx.x;
  if (g >= (long long)B * H * runs) return;
  const int r = (int)(g % runs), y = (int)((g / runs) % H), b = (int)(g / ((long long)runs * H));
  const int xb = r * kRun;
  const double* m = M + (size_t)b * 9;
  const double* mi = Mi + (size_t)b * 9;
  const size_t plane = (size_t)H * W;
  const uint8_t* sp = src + (size_t)b * 3 * plane;
  const double yd = (double)y;
  float vf[3][kRun];
  uint8_t vu[3][kRun];
  double co[3 * kRun];
#pragma unroll
  for (int e = 0; e < kRun; ++e) {
    const double xd = (double)(xb + e);   // (lanes of a partial last run compute in-range arithmetic and store nothing)
    const double c0 = (m[0] * xd + m[1] * yd) + m[2];
    const double c1 = (m[3] * xd + m[4] * yd) + m[5];
    const double c2 = (m[6] * xd + m[7] * yd) + m[8];
    co[3 * e] = c0 / c2, co[3 * e + 1] = c1 / c2, co[3 * e + 2] = c2 / c2;
    const double X = (mi[0] * xd + mi[1] * yd) + mi[2];
    const double Y = (mi[3] * xd + mi[4] * yd) + mi[5];
    const double Wd = (mi[6] * xd + mi[7] * yd) + mi[8];
    int sx = 0, sy = 0;
    if (Wd != 0.0) sx = sat_rint_i32(32.0 * X / Wd), sy = sat_rint_i32(32.0 * Y / Wd);
    const int x0 = sx >> kPosBits, y0 = sy >> kPosBits;   // arithmetic shifts: floor
    const float a = (float)(sx & 31) * (1.f / 32.f), bb = (float)(sy & 31) * (1.f / 32.f);
    const float w00 = (1.f - a) * (1.f - bb), w01 = a * (1.f - bb), w10 = (1.f - a) * bb, w11 = a * bb;
    // |x0|, |y0| <= 2^26: x0 + 1 and y0 + 1 cannot overflow; every tap is bounds-checked
    const bool inx0 = x0 >= 0 && x0 < W, inx1 = x0 + 1 >= 0 && x0 + 1 < W;
    const bool iny0 = y0 >= 0 && y0 < H, iny1 = y0 + 1 >= 0 && y0 + 1 < H;
    const size_t o00 = (size_t)(iny0 ? y0 : 0) * W + (inx0 ? x0 : 0), o01 = (size_t)(iny0 ? y0 : 0) * W + (inx1 ? x0 + 1 : 0);
    const size_t o10 = (size_t)(iny1 ? y0 + 1 : 0) * W + (inx0 ? x0 : 0), o11 = (size_t)(iny1 ? y0 + 1 : 0) * W + (inx1 ? x0 + 1 : 0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint8_t* p = sp + c * plane;
      const float s00 = iny0 && inx0 ? (float)p[o00] / 255.f : 0.f, s01 = iny0 && inx1 ? (float)p[o01] / 255.f : 0.f;
      const float s10 = iny1 && inx0 ? (float)p[o10] / 255.f : 0.f, s11 = iny1 && inx1 ? (float)p[o11] / 255.f : 0.f;
      const float v = ((s00 * w00 + s01 * w01) + s10 * w10) + s11 * w11;
      vf[c][e] = v;
      vu[c][e] = (uint8_t)(int)(v * 255.0f);   // 0 <= v <= 1
    }
  }
  const size_t pix = (size_t)y * W + xb;
  if (VEC) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t o = ((size_t)b * 3 + c) * plane + pix;
      *reinterpret_cast<uint32_t*>(dst_u8 + o) = pack_u8x4(vu[c]);
      *reinterpret_cast<f32x4*>(dst_f32 + o) = f32x4{vf[c][0], vf[c][1], vf[c][2], vf[c][3]};
    }
    f64x2* cp = reinterpret_cast<f64x2*>(coords + ((size_t)b * plane + pix) * 3);
#pragma unroll
    for (int q = 0; q < 3 * kRun / 2; ++q) cp[q] = f64x2{co[2 * q], co[2 * q + 1]};
  } else {
    for (int e = 0; e < kRun && xb + e < W; ++e) {
      for (int c = 0; c < 3; ++c) {
        const size_t o = ((size_t)b * 3 + c) * plane + pix + e;
        dst_u8[o] = vu[c][e];
        dst_f32[o] = vf[c][e];
      }
      double* cp = coords + ((size_t)b * plane + pix + e) * 3;
      cp[0] = co[3 * e], cp[1] = co[3 * e + 1], cp[2] = co[3 * e + 2];
    }
  }
}

// ---- one axis of Pillow's 8-bit bicubic resampler ---------------------------------------------------------------------
// src [N][H][W] uint8 planes.  VERT = false: dst [N][H][out] resampled along x; VERT = true: dst [N][out][W] along y.
// Output index i reads `count[i]` source pixels from `start[i]` on with the int32 coefficients coeff[i][0 .. K) (22 fraction
// bits, rows padded with zeros): dst = clip8((2^21 + sum c p) >> 22), the shift arithmetic (floor) as in Pillow's Resample.c.
// dst_f32 (or NULL): the same pixels as fp32 p / 255.
template <bool VEC, bool VERT>
__global__ __launch_bounds__(kThreadsCP) void pil_resample_kernel(const uint8_t* __restrict__ src, int N, int H, int W,
                                                                  int out, const int* __restrict__ start,
                                                                  const int* __restrict__ count,
                                                                  const int* __restrict__ coeff, int K,
                                                                  uint8_t* __restrict__ dst_u8,
                                                                  float* __restrict__ dst_f32) {
  const int OH = VERT ? out : H, OW = VERT ? W : out;
  const int runs = (OW + kRun - 1) / kRun;
  const long long g = (long long)blockIdx.x * kThreadsCP + threadIdx.x;
  if (g >= (long long)N * OH * runs) return;
  const int r = (int)(g % runs), yo = (int)((g / runs) % OH), n = (int)(g / ((long long)runs * OH));
  const int xb = r * kRun;
  const uint8_t* sp = src + (size_t)n * H * W;
  const int in_size = VERT ? H : W;
  // Accumulator: Pillow's own bound.  A row of coefficients sums to 2^22 (to rounding) and the a = -0.5 bicubic kernel's
  // negative lobes keep sum |c| below 1.3 x 2^22 for every scale, so |sum c p| <= 255 x 1.3 x 2^22 < 1.4e9 < 2^31 with the
  // rounding constant 2^21 included: int32 never overflows (the host checks sum |c| of every table it builds).
  int acc[kRun];
#pragma unroll
  for (int e = 0; e < kRun; ++e) acc[e] = 1 << (kCoeffBits - 1);
  if (VERT) {
    const int s = max(start[yo], 0), cnt = min(count[yo], min(K, in_size - s));
    const int* cf = coeff + (size_t)yo * K;
    for (int k = 0; k < cnt; ++k) {
      const uint8_t* p = sp + (size_t)(s + k) * W + xb;
      const int c = cf[k];
      if (VEC) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int e = 0; e < kRun; ++e) acc[e] += c * (int)((q >> (8 * e)) & 255u);
      } else {
        for (int e = 0; e < kRun && xb + e < W; ++e) acc[e] += c * (int)p[e];
      }
    }
  } else {
    const uint8_t* row = sp + (size_t)yo * W;
#pragma unroll
    for (int e = 0; e < kRun; ++e) {
      const int xo = min(xb + e, out - 1);   // (clamped: lanes of a partial last run store nothing)
      const int s = max(start[xo], 0), cnt = min(count[xo], min(K, in_size - s));
      const int* cf = coeff + (size_t)xo * K;
      for (int k = 0; k < cnt; ++k) acc[e] += cf[k] * (int)row[s + k];
    }
  }
  uint8_t v[kRun];
#pragma unroll
  for (int e = 0; e < kRun; ++e) v[e] = (uint8_t)min(max(acc[e] >> kCoeffBits, 0), 255);
  const size_t o = ((size_t)n * OH + yo) * OW + xb;
  if (VEC) {
    *reinterpret_cast<uint32_t*>(dst_u8 + o) = pack_u8x4(v);
    if (dst_f32)
      *reinterpret_cast<f32x4*>(dst_f32 + o) =
          f32x4{(float)v[0] / 255.f, (float)v[1] / 255.f, (float)v[2] / 255.f, (float)v[3] / 255.f};
  } else {
    for (int e = 0; e < kRun && xb + e < OW; ++e) {
      dst_u8[o + e] = v[e];
      if (dst_f32) dst_f32[o + e] = (float)v[e] / 255.f;
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace
}  // namespace c2m

using namespace c2m;

extern "C" int c2m_warp_perspective_u8(c2m_stream_t stream, const uint8_t* src, const double* M, const double* M_inv, int B,
                                       int H, int W, float* dst_f32, uint8_t* dst_u8, double* coords) {
  if (!src || !M || !M_inv || !dst_f32 || !dst_u8 || !coords || B <= 0 || H <= 0 || W <= 0) return C2M_ERR_INVALID_ARG;
  if ((long long)B * 3 * H * W >= (1ll << 31)) return C2M_ERR_UNSUPPORTED;
  const int runs = ceil_div(W, kRun);
  const long long threads = (long long)B * H * runs;
  const unsigned blocks = (unsigned)((threads + kThreadsCP - 1) / kThreadsCP);
  hipStream_t s = as_stream(stream);
  if (W % kRun == 0 && aligned16(dst_f32) && aligned4(dst_u8) && aligned16(coords))
    warp_perspective_kernel<true><<<blocks, kThreadsCP, 0, s>>>(src, M, M_inv, B, H, W, runs, dst_f32, dst_u8, coords);
  else
    warp_perspective_kernel<false><<<blocks, kThreadsCP, 0, s>>>(src, M, M_inv, B, H, W, runs, dst_f32, dst_u8, coords);
  return check_launch();
}

extern "C" int c2m_pil_bicubic_u8(c2m_stream_t stream, const uint8_t* src, int N, int H, int W, int vertical, int out_size,
                                  const int* start, const int* count, const int* coeff, int K, uint8_t* dst_u8,
                                  float* dst_f32) {
  if (!src || !start || !count || !coeff || !dst_u8 || N <= 0 || H <= 0 || W <= 0 || out_size <= 0 || K <= 0)
    return C2M_ERR_INVALID_ARG;
  const long long OH = vertical ? out_size : H, OW = vertical ? W : out_size;
  if ((long long)N * H * W >= (1ll << 31) || (long long)N * OH * OW >= (1ll << 31) || (long long)out_size * K >= (1ll << 31))
    return C2M_ERR_UNSUPPORTED;
  const long long threads = (long long)N * OH * ((OW + kRun - 1) / kRun);
  const unsigned blocks = (unsigned)((threads + kThreadsCP - 1) / kThreadsCP);
  hipStream_t s = as_stream(stream);
  bool vec = OW % kRun == 0 && aligned4(dst_u8) && (!dst_f32 || aligned16(dst_f32));
  if (vertical) vec = vec && aligned4(src);   // (W % 4 == 0 already: the pass reads 4-byte groups of the source rows)
#define C2M_RESAMPLE(V, T) \
  pil_resample_kernel<V, T><<<blocks, kThreadsCP, 0, s>>>(src, N, H, W, out_size, start, count, coeff, K, dst_u8, dst_f32)
  if (vertical) {
    if (vec) C2M_RESAMPLE(true, true);
    else C2M_RESAMPLE(false, true);
  } else {
    if (vec) C2M_RESAMPLE(true, false);
    else C2M_RESAMPLE(false, false);
  }
#undef C2M_RESAMPLE
  return check_launch();
}
