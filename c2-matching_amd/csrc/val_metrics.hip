// val_metrics.hip -- the end of validation in one pass over SR and GT (mmsr/utils/metrics.py here; the reference pulls both
// images to the host, tensor2img -> numpy, and evaluates mmsr/utils/metrics.py there: ref_restoration_model.py:295-351).
//
//   c2m_val_metrics_f32   per image: the uint8 image(s) a user saves, and the three sums nondist_validation reports
//                         (squared 8-bit difference, squared Y difference, SSIM_Y map), from fp32 [B,3,H,W] RGB tensors.
//
// Definitions (exactly those of metrics.validation_metrics):
//   v      = rint(clamp(x, 0, 1) * 255.0f) in fp32, half to even
//   sq     = sum over the border-cropped window and the 3 channels of (v_sr - v_gt)^2           (integers: exact)
//   Y      = ((24.966 B + 128.553 G + 65.481 R) / 255 + 16) / 255 * 255 in float64, B G R = (double)(v / 255.0f) * 255.0
//   sq_y   = float64 sum of (Y_sr - Y_gt)^2 over the cropped window
//   ssim   = float64 sum over the 'valid' positions of the SSIM map of the Y images: 11 x 11 Gaussian window (sigma 1.5),
//            five windowed means a, b, a^2, b^2, ab
//
// Tiling.  One workgroup of 256 threads makes kTileH x kTileW = 16 x 32 SSIM outputs of one image.  It holds Y of both images
// for the tile and its 10-pixel halo in LDS as float64 (2 x 26 x 42 x 8 = 17 472 bytes), runs the window separably -- the
// horizontal pass writes the five quantities for 26 rows x 32 columns (5 x 26 x 32 x 8 = 33 280 bytes), the vertical pass
// reads them back -- 50 752 bytes in all: three workgroups per CU.  A tile's Y window overlaps its neighbours' by the halo;
// every pixel of the valid window is OWNED by exactly one workgroup, which stores its uint8 values and adds its squared
// differences: the tile whose 16 x 32 outputs start at that pixel's cropped position, the last tile of a row / column also
// taking the trailing 10 pixels and the border band behind them, the first the border band in front.
// Lanes of a wave walk along x everywhere: global loads are coalesced and LDS reads of neighbouring doubles conflict-free.
//
// Determinism.  A thread adds its terms in a fixed order, the workgroup's 256 partial sums go through a fixed tree, the
// per-tile results go to the workspace, and a second launch (one workgroup per image) adds the tiles in a fixed order.  No
// atomics.  a*a, b*b and a*b are formed by the same instruction sequence, so SR == GT gives an SSIM map of exactly 1.0.
#include <cmath>

#include "c2m_common.h"

namespace c2m {
namespace {

constexpr int kTileH = C2M_VAL_TILE_H, kTileW = C2M_VAL_TILE_W;
constexpr int kWin = 11, kHalo = kWin - 1;
constexpr int kThreadsVM = 256;
constexpr int kYRows = kTileH + kHalo, kYCols = kTileW + kHalo;   // 26 x 42
static_assert(kTileW == 32 && kTileH * kTileW == 2 * kThreadsVM, "the thread -> output maps below are written for 16 x 32 tiles");

struct Window { double g[kWin]; };                   // the normalised 1-D Gaussian; the 2-D window is its outer product
struct Image { const float* p; long long row, plane, img; };   // element pitches; innermost stride 1

__device__ __forceinline__ float to_8bit(float x) { return __builtin_rintf(fminf(fmaxf(x, 0.f), 1.f) * 255.0f); }

__device__ __forceinline__ double y_of(float b, float g, float r) {
  const double B = (double)(b / 255.0f) * 255.0, G = (double)(g / 255.0f) * 255.0, R = (double)(r / 255.0f) * 255.0;
  return ((24.966 * B + 128.553 * G + 65.481 * R) / 255.0 + 16.0) / 255.0 * 255.0;
}

__device__ __forceinline__ void store_rgb8(uint8_t* dst, size_t pixel, const float v[3], int rgb) {
  uint8_t* d = dst + pixel * 3;
  d[0] = (uint8_t)(rgb ? v[0] : v[2]);
  d[1] = (uint8_t)v[1];
  d[2] = (uint8_t)(rgb ? v[2] : v[0]);
}

// sums of the 256 threads' values in a fixed tree; the result is valid in thread 0
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = kThreadsVM / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// partial [B][tiles][3] float64: sq, sq_y, ssim of one tile
__global__ __launch_bounds__(kThreadsVM) void val_metrics_kernel(Image sr, Image gt, int vh, int vw, int crop, int tiles_x,
                                                                 int tiles_y, int rgb, Window win,
                                                                 uint8_t* __restrict__ sr_u8, uint8_t* __restrict__ gt_u8,
                                                                 double* __restrict__ partial) {
  __shared__ double s_a[kYRows][kYCols], s_b[kYRows][kYCols];
  __shared__ double s_h[5][kYRows][kTileW];

  const int tid = threadIdx.x;
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int ty = t / tiles_x, tx = t % tiles_x;
  const int h = vh - 2 * crop, w = vw - 2 * crop;          // the cropped window; outputs (h - 10) x (w - 10)
  const int y0 = ty * kTileH, x0 = tx * kTileW;            // first output = first Y pixel of the tile, cropped coordinates
  const int th = min(kTileH, h - kHalo - y0), tw = min(kTileW, w - kHalo - x0);
  const int yr = th + kHalo, yc = tw + kHalo;              // the tile's Y window, <= 26 x 42
  const bool last_y = ty == tiles_y - 1, last_x = tx == tiles_x - 1;
  // owned pixels and the rectangle walked (owned + Y window), coordinates of the valid window
  const int oy0 = ty == 0 ? 0 : crop + y0, oy1 = last_y ? vh : crop + y0 + kTileH;
  const int ox0 = tx == 0 ? 0 : crop + x0, ox1 = last_x ? vw : crop + x0 + kTileW;
  const int uy1 = last_y ? vh : crop + y0 + yr, ux1 = last_x ? vw : crop + x0 + yc;
  const int ucols = ux1 - ox0, upix = (uy1 - oy0) * ucols;

  const float* ps = sr.p + (size_t)n * sr.img;
  const float* pg = gt.p + (size_t)n * gt.img;
  unsigned long long sq = 0;
  double sq_y = 0.0;
  for (int i = tid; i < upix; i += kThreadsVM) {
    const int vy = oy0 + i / ucols, vx = ox0 + i % ucols;
    const int ly = vy - crop - y0, lx = vx - crop - x0;
    const bool in_y = ly >= 0 && ly < yr && lx >= 0 && lx < yc;
    const bool owned = vy < oy1 && vx < ox1;
    if (!in_y && !owned) continue;
    float a[3], b[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a[c] = to_8bit(ps[(size_t)c * sr.plane + (size_t)vy * sr.row + vx]);
      b[c] = to_8bit(pg[(size_t)c * gt.plane + (size_t)vy * gt.row + vx]);
    }
    if (owned) {
      const size_t pixel = ((size_t)n * vh + vy) * vw + vx;
      if (sr_u8) store_rgb8(sr_u8, pixel, a, rgb);
      if (gt_u8) store_rgb8(gt_u8, pixel, b, rgb);
    }
    if (in_y) {
      const double ya = y_of(a[2], a[1], a[0]), yb = y_of(b[2], b[1], b[0]);
      s_a[ly][lx] = ya;
      s_b[ly][lx] = yb;
      if (owned) {   // an owned pixel of the Y window lies in the cropped window
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int d = (int)a[c] - (int)b[c];
          sq += (unsigned)(d * d);
        }
        const double dy = ya - yb;
        sq_y += dy * dy;
      }
    }
  }
  __syncthreads();

  // horizontal pass: the five quantities for every row of the Y window x the tile's output columns
  for (int i = tid; i < yr * kTileW; i += kThreadsVM) {
    const int r = i / kTileW, c = i % kTileW;
    if (c >= tw) continue;
    double ma = 0.0, mb = 0.0, maa = 0.0, mbb = 0.0, mab = 0.0;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const double a = s_a[r][c + k], b = s_b[r][c + k], g = win.g[k];
      ma += g * a;
      mb += g * b;
      maa += g * (a * a);
      mbb += g * (b * b);
      mab += g * (a * b);
    }
    s_h[0][r][c] = ma;
    s_h[1][r][c] = mb;
    s_h[2][r][c] = maa;
    s_h[3][r][c] = mbb;
    s_h[4][r][c] = mab;
  }
  __syncthreads();

  // vertical pass and the SSIM map: two outputs per thread
  const double c1 = (0.01 * 255) * (0.01 * 255), c2 = (0.03 * 255) * (0.03 * 255);
  double ssim = 0.0;
  for (int i = tid; i < kTileH * kTileW; i += kThreadsVM) {
    const int r = i / kTileW, c = i % kTileW;
    if (r >= th || c >= tw) continue;
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const double g = win.g[k];
#pragma unroll
      for (int q = 0; q < 5; ++q) m[q] += g * s_h[q][r + k][c];
    }
    const double mu1 = m[0], mu2 = m[1];
    const double s11 = m[2] - mu1 * mu1, s22 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
    ssim += ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2));
  }

  // s_h is free after the barrier inside block_sum
  double* red = &s_h[0][0][0];
  const unsigned long long sq_all = block_sum(sq, reinterpret_cast<unsigned long long*>(red), tid);
  const double sq_y_all = block_sum(sq_y, red, tid);
  const double ssim_all = block_sum(ssim, red, tid);
  if (tid == 0) {
    double* o = partial + (size_t)blockIdx.x * 3;
    o[0] = (double)sq_all;
    o[1] = sq_y_all;
    o[2] = ssim_all;
  }
}

// partial [B][tiles][3] -> sums [B][3]: thread t adds tiles t, t + 256, ... in that order, then the fixed tree
__global__ __launch_bounds__(kThreadsVM) void val_metrics_finish_kernel(const double* __restrict__ partial, int tiles,
                                                                        double* __restrict__ sums) {
  __shared__ double red[kThreadsVM];
  const int tid = threadIdx.x, n = blockIdx.x;
  const double* p = partial + (size_t)n * tiles * 3;
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < tiles; i += kThreadsVM)
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] += p[(size_t)i * 3 + q];
  for (int q = 0; q < 3; ++q) {
    const double s = block_sum(v[q], red, tid);
    if (tid == 0) sums[(size_t)n * 3 + q] = s;
  }
}

// the uint8 image alone (tensor2img of one batch): one thread per pixel
__global__ __launch_bounds__(kThreadsVM) void to_u8_kernel(Image src, int B, int vh, int vw, int rgb,
                                                           uint8_t* __restrict__ dst) {
  const size_t total = (size_t)B * vh * vw;
  const size_t i = (size_t)blockIdx.x * kThreadsVM + threadIdx.x;
  if (i >= total) return;
  const int vx = (int)(i % vw), vy = (int)((i / vw) % vh);
  const size_t n = i / ((size_t)vw * vh);
  const float* p = src.p + n * src.img + (size_t)vy * src.row + vx;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = to_8bit(p[(size_t)c * src.plane]);
  store_rgb8(dst, i, v, rgb);
}

inline long long tiles_of(int valid_h, int valid_w, int crop_border, int* tiles_x, int* tiles_y) {
  const int oh = valid_h - 2 * crop_border - kHalo, ow = valid_w - 2 * crop_border - kHalo;
  *tiles_x = ceil_div(ow, kTileW);
  *tiles_y = ceil_div(oh, kTileH);
  return (long long)*tiles_x * *tiles_y;
}

inline bool window_ok(int valid_h, int valid_w, int crop_border) {
  return crop_border >= 0 && crop_border < (1 << 28) && (long long)(valid_h < valid_w ? valid_h : valid_w) - 2ll * crop_border >= kWin;
}

inline bool pitches_ok(const c2m_image_src* s) {   // overlapping (expanded) tensors are fine, negative pitches are not
  return s->ptr && s->row_pitch >= 0 && s->plane_pitch >= 0 && s->img_pitch >= 0;
}

}  // namespace
}  // namespace c2m

using namespace c2m;

extern "C" int c2m_val_metrics_tile(int* tile_h, int* tile_w) {
  if (!tile_h || !tile_w) return C2M_ERR_INVALID_ARG;
  *tile_h = kTileH;
  *tile_w = kTileW;
  return C2M_OK;
}

extern "C" size_t c2m_val_metrics_workspace_bytes(int B, int valid_h, int valid_w, int crop_border) {
  if (B <= 0 || valid_h <= 0 || valid_w <= 0 || !window_ok(valid_h, valid_w, crop_border)) return 0;
  int tiles_x, tiles_y;
  return (size_t)B * (size_t)tiles_of(valid_h, valid_w, crop_border, &tiles_x, &tiles_y) * 3 * sizeof(double);
}

extern "C" int c2m_val_metrics_f32(c2m_stream_t stream, const c2m_image_src* sr, const c2m_image_src* gt, int B, int H, int W,
                                   int valid_h, int valid_w, int crop_border, int rgb_order, uint8_t* sr_u8, uint8_t* gt_u8,
                                   double* sums, void* workspace, size_t workspace_bytes) {
  if (!sr || B <= 0 || H <= 0 || W <= 0 || valid_h <= 0 || valid_w <= 0 || valid_h > H || valid_w > W || crop_border < 0 ||
      !pitches_ok(sr) || (gt && !pitches_ok(gt)))
    return C2M_ERR_INVALID_ARG;
  if (sr->pix_pitch != 1 || (gt && gt->pix_pitch != 1)) return C2M_ERR_UNSUPPORTED;
  if ((long long)valid_h * valid_w >= (1ll << 31)) return C2M_ERR_UNSUPPORTED;   // a tile walks its pixels with an int
  const Image s{sr->ptr, sr->row_pitch, sr->plane_pitch, sr->img_pitch};
  if (!gt) {   // the image alone
    if (!sr_u8 || gt_u8 || sums) return C2M_ERR_INVALID_ARG;
    const long long blocks = ((long long)B * valid_h * valid_w + kThreadsVM - 1) / kThreadsVM;
    if (blocks >= (1ll << 31)) return C2M_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(to_u8_kernel, dim3((unsigned)blocks), dim3(kThreadsVM), 0, as_stream(stream), s, B, valid_h, valid_w,
                       rgb_order != 0, sr_u8);
    return check_launch();
  }
  if (!sums) return C2M_ERR_INVALID_ARG;
  if (!window_ok(valid_h, valid_w, crop_border)) return C2M_ERR_UNSUPPORTED;   // fewer than 11 pixels: the SSIM map is empty
  int tiles_x, tiles_y;
  const long long tiles = tiles_of(valid_h, valid_w, crop_border, &tiles_x, &tiles_y);
  if ((long long)B * tiles >= (1ll << 31) || tiles >= (1ll << 31)) return C2M_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < (size_t)B * (size_t)tiles * 3 * sizeof(double)) return C2M_ERR_WORKSPACE;
  Window win;
  double total = 0.0;
  for (int k = 0; k < kWin; ++k) {
    const double x = (double)k - 5.0;
    win.g[k] = std::exp(-(x * x) / (2 * 1.5 * 1.5));
    total += win.g[k];
  }
  for (int k = 0; k < kWin; ++k) win.g[k] /= total;
  const Image g{gt->ptr, gt->row_pitch, gt->plane_pitch, gt->img_pitch};
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(val_metrics_kernel, dim3((unsigned)(B * tiles)), dim3(kThreadsVM), 0, as_stream(stream), s, g, valid_h,
                     valid_w, crop_border, tiles_x, tiles_y, rgb_order != 0, win, sr_u8, gt_u8, partial);
  if (int rc = check_launch()) return rc;
  hipLaunchKernelGGL(val_metrics_finish_kernel, dim3((unsigned)B), dim3(kThreadsVM), 0, as_stream(stream), partial, (int)tiles,
                     sums);
  return check_launch();
}
