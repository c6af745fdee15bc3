// ref_band.hip -- the padding band of a zero-padded Ref image (the dataset pads every Ref to the LR x 4 canvas at the bottom
// and right; a 500 x 500 Ref on a 640 x 640 canvas leaves 39 % of every Ref-side feature map as a band).
//
// Behind the live region plus the receptive radius of a layer, a feature map no longer depends on the image: its value at a
// pixel is a function of that pixel's distances to the four canvas edges only (zero padding outside the canvas against
// act(bias) propagated inside), and constant once all four exceed the radius.  The Ref-side towers therefore launch their
// convolutions on the top-left tiles only (roi_tiles_y / roi_tiles_x of the two convolution descriptors), run the same layers once on a
// small all-zero canvas (the TEMPLATE, B = 1), and copy the band from it:
//
//   c2m_ref_live_extent_f32   img [B][3][H][W] -> (live_h, live_w): 1 + the largest row / column index of a pixel that is not
//                             exactly 0.0 in all three channels, over the batch (0, 0 for an all-zero batch).
//   c2m_band_fill_f32         dst(b, c, y, x) = tmpl(c, sy(y), sx(x)) for every pixel outside [0, roi_h) x [0, roi_w), with the
//                             edge-distance clamp  s(v) = v            if v < margin            (same distance to the near edge)
//                                                       = T - (N - v)  if N - v <= margin       (same distance to the far edge)
//                                                       = margin       otherwise                (the template's interior)
//                             (N: dst extent, T: template extent; needs N, T >= 2 margin + 1).  One pass, 16-byte stores.
//
// Layouts of the fill (dst and template of one call share the kind; pitches in floats):
//   channel-vector (planar == 0): element (b, c, y, x) at b*img + (c / cpg)*plane + y*row + x*pix + c % cpg -- channels-last
//       tensors and views (cpg = C, plane = 0; zero-bordered tap buffers through their interior's pitches) and the 8-channel
//       group-major twin (cpg = 8, pix = 8);
//   planar (planar != 0): contiguous [B][C][H][W] / [C][Ht][Wt], W % 4 == 0 and roi_w % 4 == 0.
#include <algorithm>

#include "c2m_common.h"

namespace c2m {
namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) live_extent_kernel(const float* __restrict__ img, unsigned n, unsigned H, unsigned Wv,
                                                               int vec, int* __restrict__ out) {
  // n < 2^31: elements (vec == 1) or float4 groups (vec == 4; W % 4 == 0: a group never crosses a row); Wv = W / vec
  int my = 0, mx = 0;
  const unsigned stride = gridDim.x * kThreads;
  for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    int last = -1;   // highest non-zero element of the group
    if (vec == 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(img + 4 * (size_t)i);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (v[e] != 0.0f) last = e;
    } else if (img[i] != 0.0f) {
      last = 0;
    }
    if (last >= 0) {
      const unsigned row = i / Wv, xv = i - row * Wv;
      my = max(my, (int)(row % H) + 1);
      mx = max(mx, (int)xv * vec + last + 1);
    }
  }
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) {
    my = max(my, __shfl_xor(my, s, kWave));
    mx = max(mx, __shfl_xor(mx, s, kWave));
  }
  // one pair of atomics per workgroup at most, and none where the result already holds a value at least as large (it only grows:
  // a stale read can only cause a redundant atomic) -- tens of thousands of atomics on one address would serialise in L2
  __shared__ int wy[kThreads / kWave], wx[kThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) {
    wy[threadIdx.x / kWave] = my;
    wx[threadIdx.x / kWave] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kThreads / kWave; ++w) {
      my = max(my, wy[w]);
      mx = max(mx, wx[w]);
    }
    if (my > *(volatile int*)out) atomicMax(out, my);
    if (mx > *(volatile int*)(out + 1)) atomicMax(out + 1, mx);
  }
}

struct FillParams {
  float* dst;
  const float* tmpl;
  int B, C, H, W, Ht, Wt;
  int cpg;
  int d_pix, d_row;
  long long d_plane, d_img;
  int t_pix, t_row;
  long long t_plane;
  int roi_h, roi_w, margin_y, margin_x;
  long long n_a, n_band;   // band pixels (planar: 4-pixel groups) right of the ROI / in all
};

__device__ __forceinline__ int band_src(int v, int N, int T, int margin) {
  return v < margin ? v : (N - v <= margin ? T - (N - v) : margin);
}

// band element p -> (y, x): first the columns right of the ROI in rows [0, roi_h), then the whole rows below it
// (wq / rq: W and roi_w in pixels, or in 4-pixel groups for the planar kernel)
__device__ __forceinline__ void band_pixel(const FillParams& p, long long q, int wq, int rq, int& y, int& x) {
  if (q < p.n_a) {
    const int wa = wq - rq;
    y = (int)(q / wa);
    x = rq + (int)(q - (long long)y * wa);
  } else {
    q -= p.n_a;
    y = p.roi_h + (int)(q / wq);
    x = (int)(q - (long long)(y - p.roi_h) * wq);
  }
}

__global__ void __launch_bounds__(kThreads) band_fill_vec_kernel(FillParams p) {
  const int cv = p.C >> 2;
  const long long per_img = p.n_band * cv;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= per_img * p.B) return;
  const int b = (int)(i / per_img);
  const long long r = i - (long long)b * per_img;
  const long long q = r / cv;
  const int c = 4 * (int)(r - q * cv);
  int y, x;
  band_pixel(p, q, p.W, p.roi_w, y, x);
  const int sy = band_src(y, p.H, p.Ht, p.margin_y), sx = band_src(x, p.W, p.Wt, p.margin_x);
  const int plane = c / p.cpg, ci = c - plane * p.cpg;
  const f32x4 v = *reinterpret_cast<const f32x4*>(p.tmpl + (size_t)plane * p.t_plane + (size_t)sy * p.t_row + (size_t)sx * p.t_pix + ci);
  *reinterpret_cast<f32x4*>(p.dst + (size_t)b * p.d_img + (size_t)plane * p.d_plane + (size_t)y * p.d_row + (size_t)x * p.d_pix + ci) = v;
}

__global__ void __launch_bounds__(kThreads) band_fill_planar_kernel(FillParams p) {
  const long long per_img = p.n_band * p.C;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= per_img * p.B) return;
  const int b = (int)(i / per_img);
  const long long r = i - (long long)b * per_img;
  const int c = (int)(r / p.n_band);
  const long long q = r - (long long)c * p.n_band;
  int y, xq;
  band_pixel(p, q, p.W >> 2, p.roi_w >> 2, y, xq);
  const int sy = band_src(y, p.H, p.Ht, p.margin_y);
  const float* trow = p.tmpl + ((size_t)c * p.Ht + sy) * p.Wt;
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = trow[band_src(4 * xq + e, p.W, p.Wt, p.margin_x)];
  *reinterpret_cast<f32x4*>(p.dst + (((size_t)b * p.C + c) * p.H + y) * p.W + 4 * xq) = v;
}

}  // namespace
}  // namespace c2m

extern "C" int c2m_ref_live_extent_f32(c2m_stream_t stream, const float* img, int B, int H, int W, int* extent) {
  using namespace c2m;
  if (!img || !extent || B <= 0 || H <= 0 || W <= 0) return C2M_ERR_INVALID_ARG;
  const int vec = (W % 4 == 0 && ((uintptr_t)img & 15) == 0) ? 4 : 1;
  const long long n = 3LL * B * H * W / vec;
  if (n >= (1LL << 31)) return C2M_ERR_UNSUPPORTED;   // 32-bit group indices
  const unsigned grid = (unsigned)std::min<long long>((n + kThreads - 1) / kThreads, 2048);
  hipLaunchKernelGGL(live_extent_kernel, dim3(grid), dim3(kThreads), 0, as_stream(stream), img, (unsigned)n, (unsigned)H,
                     (unsigned)(W / vec), vec, extent);
  return check_launch();
}

extern "C" int c2m_band_fill_f32(c2m_stream_t stream, float* dst, int B, int C, int H, int W, int cpg, int d_pix_pitch,
                                 int d_row_pitch, long long d_plane_pitch, long long d_img_pitch, const float* tmpl, int Ht,
                                 int Wt, int t_pix_pitch, int t_row_pitch, long long t_plane_pitch, int roi_h, int roi_w,
                                 int margin_y, int margin_x, int planar) {
  using namespace c2m;
  if (!dst || !tmpl || B <= 0 || C <= 0 || H <= 0 || W <= 0 || Ht <= 0 || Wt <= 0 || roi_h < 0 || roi_w < 0 || roi_h > H ||
      roi_w > W || margin_y < 0 || margin_x < 0)
    return C2M_ERR_INVALID_ARG;
  // the three zones of the clamp must be disjoint in the destination and exist in the template
  if (H < 2 * margin_y + 1 || Ht < 2 * margin_y + 1 || W < 2 * margin_x + 1 || Wt < 2 * margin_x + 1) return C2M_ERR_INVALID_ARG;
  if (((uintptr_t)dst & 15) || ((uintptr_t)tmpl & 15)) return C2M_ERR_UNSUPPORTED;
  FillParams p;
  p.dst = dst; p.tmpl = tmpl; p.B = B; p.C = C; p.H = H; p.W = W; p.Ht = Ht; p.Wt = Wt;
  p.roi_h = roi_h; p.roi_w = roi_w; p.margin_y = margin_y; p.margin_x = margin_x;
  long long threads;
  if (planar) {
    if (W % 4 != 0 || roi_w % 4 != 0) return C2M_ERR_UNSUPPORTED;
    p.cpg = 1; p.d_pix = 1; p.d_row = W; p.d_plane = (long long)H * W; p.d_img = p.d_plane * C;
    p.t_pix = 1; p.t_row = Wt; p.t_plane = (long long)Ht * Wt;
    p.n_a = (long long)roi_h * ((W - roi_w) / 4);
    p.n_band = p.n_a + (long long)(H - roi_h) * (W / 4);
    threads = p.n_band * C * B;
  } else {
    if (cpg <= 0 || cpg % 4 != 0 || C % cpg != 0 || d_pix_pitch < cpg || t_pix_pitch < cpg || d_pix_pitch % 4 != 0 ||
        d_row_pitch % 4 != 0 || d_plane_pitch % 4 != 0 || d_img_pitch % 4 != 0 || t_pix_pitch % 4 != 0 || t_row_pitch % 4 != 0 ||
        t_plane_pitch % 4 != 0 || d_row_pitch < 0 || t_row_pitch < 0 || d_plane_pitch < 0 || t_plane_pitch < 0 || d_img_pitch < 0)
      return C2M_ERR_UNSUPPORTED;
    p.cpg = cpg; p.d_pix = d_pix_pitch; p.d_row = d_row_pitch; p.d_plane = d_plane_pitch; p.d_img = d_img_pitch;
    p.t_pix = t_pix_pitch; p.t_row = t_row_pitch; p.t_plane = t_plane_pitch;
    p.n_a = (long long)roi_h * (W - roi_w);
    p.n_band = p.n_a + (long long)(H - roi_h) * W;
    threads = p.n_band * (C / 4) * B;
  }
  if (threads == 0) return C2M_OK;
  const long long blocks = (threads + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffLL) return C2M_ERR_UNSUPPORTED;
  if (planar)
    hipLaunchKernelGGL(band_fill_planar_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, as_stream(stream), p);
  else
    hipLaunchKernelGGL(band_fill_vec_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, as_stream(stream), p);
  return check_launch();
}
