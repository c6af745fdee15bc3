// ref_pairs.hip -- the resampler of the stage-3 batch maker (mmsr/data/ref_pairs.py; the reference builds the same images
// on the host with five PIL.Image.resize calls per sample: mmsr/data/ref_cufed_dataset.py).
//
//   c2m_pil_bicubic2d_u8   PIL.Image.resize(..., BICUBIC) on 8-bit planes, BOTH passes in one launch, with the sample's
//                          horizontal flip / vertical flip / transpose applied while the source is read.
//
// The arithmetic is that of c2m_pil_bicubic_u8 (contras_pairs.hip), pass by pass: int32 accumulation of 22-bit fixed-point
// coefficients, + 2^21, >> 22, clip to 0..255, the horizontal pass first and a uint8 image between the passes.  An axis
// whose size does not change is given the identity table (one coefficient 2^22 per row), which reproduces the pixel, so
// "Pillow skips that pass" and "the pass runs with the identity table" are the same bits.
//
// Tile and LDS budget.  One workgroup of 256 threads makes one 32 x 32 output tile of one plane from LDS alone:
//   the two tiles of the coefficient tables (row pitch K | 1 dwords: the 32 rows a pass reads at once start in 32 banks),
//   the oriented source window, uint8, [win_h][win_w rounded up to 4],
//   the horizontally resampled window, uint8, [win_h][40].
// 32 columns: a wave of the horizontal pass is two window rows x 32 output columns, ds_read_u8 is banked by dword within
// lanes 0-31 and 32-63, and the 32 lanes of one row read taps at most `ratio` bytes apart -- the same or neighbouring
// dwords for the x4 / :4 of the training data, no conflict.  The vertical pass gives a thread four neighbouring columns of
// one output row (one ds_read_b32 per tap, 4-byte / 16-byte stores), so a lane group holds four output rows; their
// windows start 4 rows apart at :4 and 0-1 rows apart at x4, and the pitch of 40 bytes = 10 dwords puts those rows 8 or 10
// banks apart: conflict-free for both (pitch 32 would be 4-way at :4).
// The source window grows with the down-scaling ratio (support = 2 x ratio per side): 134 x 134 at :4, 12 x 12 at x4.  The
// budget is 64 KiB of the CU's 160 KiB: two workgroups stay resident per CU at the largest window taken (about 216 x 216,
// ratio 6), five at :4.  A geometry over the budget is the caller's to run as two c2m_pil_bicubic_u8 passes.
#include "c2m_common.h"

namespace c2m {
namespace {

constexpr int kTile = C2M_PIL2D_TILE;
constexpr int kThreadsRP = 256;
constexpr int kMidPitch = 40;    // bytes per row of the horizontally resampled window
constexpr int kCoeffBits = 22;   // Pillow's PRECISION_BITS = 32 - 8 - 2
static_assert(kTile == 32 && kThreadsRP == 256, "the thread -> pixel maps below are written for 32 x 32 tiles and 256 threads");

__host__ __device__ inline int round_up4(int v) { return (v + 3) & ~3; }

inline size_t lds_bytes(int Kh, int Kv, int win_h, int win_w) {
  return sizeof(int) * ((size_t)4 * kTile + (size_t)kTile * (Kh | 1) + (size_t)kTile * (Kv | 1)) +
         (size_t)win_h * round_up4(win_w) + (size_t)win_h * kMidPitch;
}

// src [N][H][W] uint8 planes, plane n belongs to sample n / pps.  flags (or NULL) one byte per sample: bit 0 horizontal
// flip, bit 1 vertical flip, bit 2 transpose (H == W), applied in that order; O below is the oriented plane.
// Tables as for c2m_pil_bicubic_u8: h_* resample the x axis W -> OW, v_* the y axis H -> OH.  win_h / win_w: the largest
// source window of any tile (start of its first row .. end of its last).  Every tap is clamped to the plane and to the
// window: tables that do not fit the stated window give wrong pixels there, never an access outside LDS or the plane.
__global__ __launch_bounds__(kThreadsRP) void pil_bicubic2d_kernel(
    const uint8_t* __restrict__ src, const uint8_t* __restrict__ flags, int pps, int H, int W, int OH, int OW,
    const int* __restrict__ h_start, const int* __restrict__ h_count, const int* __restrict__ h_coeff, int Kh,
    const int* __restrict__ v_start, const int* __restrict__ v_count, const int* __restrict__ v_coeff, int Kv, int win_h,
    int win_w, int tiles_x, int tiles_y, int vec_out, int vec_orient, uint8_t* __restrict__ dst_u8,
    float* __restrict__ dst_f32, float* __restrict__ orient_f32) {
  extern __shared__ int lds_i[];
  const int Khp = Kh | 1, Kvp = Kv | 1, sp = round_up4(win_w);
  int* s_hs = lds_i;                    // [32] first source column of each output column of the tile
  int* s_hn = s_hs + kTile;             // [32] its tap count
  int* s_vs = s_hn + kTile;             // [32] first source row of each output row
  int* s_vn = s_vs + kTile;
  int* s_hc = s_vn + kTile;             // [32][Khp]
  int* s_vc = s_hc + kTile * Khp;       // [32][Kvp]
  uint8_t* s_src = reinterpret_cast<uint8_t*>(s_vc + kTile * Kvp);   // [win_h][sp]
  uint8_t* s_mid = s_src + (size_t)win_h * sp;                        // [win_h][kMidPitch]  (win_h * sp is a multiple of 4)

  const int tid = threadIdx.x;
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int tyi = t / tiles_x, txi = t % tiles_x;
  const int tx0 = txi * kTile, ty0 = tyi * kTile;
  const int tw = min(kTile, OW - tx0), th = min(kTile, OH - ty0);
  const int f = flags ? flags[n / pps] : 0;
  const bool fh = f & 1, fv = f & 2, ft = (f & 4) && H == W;
  const uint8_t* sp_n = src + (size_t)n * H * W;
  // O[y][x], 0 <= y < H, 0 <= x < W
  auto oriented = [&](int y, int x) -> uint8_t {
    const int a = ft ? x : y, b = ft ? y : x;
    return sp_n[(size_t)(fv ? H - 1 - a : a) * W + (fh ? W - 1 - b : b)];
  };

  if (tid < 2 * kTile) {
    const bool vert = tid >= kTile;
    const int i = tid & (kTile - 1);
    const int o = (vert ? ty0 : tx0) + i, out = vert ? OH : OW, in = vert ? H : W, K = vert ? Kv : Kh;
    int s = 0, c = 0;
    if (o < out) {
      s = min(max((vert ? v_start : h_start)[o], 0), in);
      c = min(max((vert ? v_count : h_count)[o], 0), min(K, in - s));
    }
    (vert ? s_vs : s_hs)[i] = s;
    (vert ? s_vn : s_hn)[i] = c;
  }
  for (int i = tid; i < kTile * Kh; i += kThreadsRP) {
    const int c = i / Kh, k = i - c * Kh;
    s_hc[c * Khp + k] = tx0 + c < OW ? h_coeff[(size_t)(tx0 + c) * Kh + k] : 0;
  }
  for (int i = tid; i < kTile * Kv; i += kThreadsRP) {
    const int c = i / Kv, k = i - c * Kv;
    s_vc[c * Kvp + k] = ty0 + c < OH ? v_coeff[(size_t)(ty0 + c) * Kv + k] : 0;
  }
  __syncthreads();

  // the tile's source window [wy0, wy0 + wh) x [wx0, wx0 + ww), never larger than the LDS arrays
  int wx0 = W, wx1 = 0, wy0 = H, wy1 = 0;
  for (int i = 0; i < tw; ++i) wx0 = min(wx0, s_hs[i]), wx1 = max(wx1, s_hs[i] + s_hn[i]);
  for (int i = 0; i < th; ++i) wy0 = min(wy0, s_vs[i]), wy1 = max(wy1, s_vs[i] + s_vn[i]);
  const int ww = min(max(wx1 - wx0, 0), win_w), wh = min(max(wy1 - wy0, 0), win_h);

  if (ft) {   // neighbouring lanes walk down a column of O: along a row of the source
    for (int i = tid; i < wh * ww; i += kThreadsRP) {
      const int b = i / wh, a = i - b * wh;
      s_src[a * sp + b] = oriented(wy0 + a, wx0 + b);
    }
  } else {
    for (int i = tid; i < wh * ww; i += kThreadsRP) {
      const int a = i / ww, b = i - a * ww;
      s_src[a * sp + b] = oriented(wy0 + a, wx0 + b);
    }
  }
  __syncthreads();

  {   // horizontal pass: window rows x the tile's columns -> s_mid
    const int c = tid & (kTile - 1);
    if (c < tw) {
      const int o = s_hs[c] - wx0, cnt = min(s_hn[c], ww - o);
      const int* cf = s_hc + c * Khp;
      for (int r = tid / kTile; r < wh; r += kThreadsRP / kTile) {
        const uint8_t* p = s_src + r * sp + o;
        int acc = 1 << (kCoeffBits - 1);
        for (int k = 0; k < cnt; ++k) acc += cf[k] * (int)p[k];
        s_mid[r * kMidPitch + c] = (uint8_t)min(max(acc >> kCoeffBits, 0), 255);
      }
    }
  }
  __syncthreads();

  {   // vertical pass: four neighbouring columns of one output row per thread
    const int q = tid & 7, r = tid >> 3;
    if (r < th && 4 * q < tw) {
      const int o = s_vs[r] - wy0, cnt = min(s_vn[r], wh - o);
      const int* cf = s_vc + r * Kvp;
      int acc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = 1 << (kCoeffBits - 1);
      for (int k = 0; k < cnt; ++k) {
        const uint32_t px = *reinterpret_cast<const uint32_t*>(s_mid + (o + k) * kMidPitch + 4 * q);
        const int c = cf[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += c * (int)((px >> (8 * e)) & 255u);
      }
      uint32_t v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (uint32_t)min(max(acc[e] >> kCoeffBits, 0), 255);
      const int x = tx0 + 4 * q;
      const size_t off = ((size_t)n * OH + ty0 + r) * OW + x;
      if (vec_out) {   // OW % 4 == 0: the run lies inside the row
        *reinterpret_cast<uint32_t*>(dst_u8 + off) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        if (dst_f32)
          *reinterpret_cast<f32x4*>(dst_f32 + off) =
              f32x4{(float)v[0] / 255.f, (float)v[1] / 255.f, (float)v[2] / 255.f, (float)v[3] / 255.f};
      } else {
        for (int e = 0; e < 4 && x + e < OW; ++e) {
          dst_u8[off + e] = (uint8_t)v[e];
          if (dst_f32) dst_f32[off + e] = (float)v[e] / 255.f;
        }
      }
    }
  }

  if (orient_f32) {   // O / 255: the tiles share the plane as a tiles_y x tiles_x grid of rectangles, 4-pixel runs along x
    const int rh = (H + tiles_y - 1) / tiles_y, rw = round_up4((W + tiles_x - 1) / tiles_x);
    const int y0 = tyi * rh, y1 = min(H, y0 + rh), x0 = txi * rw, x1 = min(W, x0 + rw);
    const int runs = x1 > x0 ? (x1 - x0 + 3) / 4 : 0;
    float* op = orient_f32 + (size_t)n * H * W;
    for (int i = tid; i < (y1 - y0) * runs; i += kThreadsRP) {
      const int y = y0 + i / runs, x = x0 + 4 * (i % runs);
      if (vec_orient) {   // W % 4 == 0
        *reinterpret_cast<f32x4*>(op + (size_t)y * W + x) =
            f32x4{(float)oriented(y, x) / 255.f, (float)oriented(y, x + 1) / 255.f, (float)oriented(y, x + 2) / 255.f,
                  (float)oriented(y, x + 3) / 255.f};
      } else {
        for (int e = 0; e < 4 && x + e < x1; ++e) op[(size_t)y * W + x + e] = (float)oriented(y, x + e) / 255.f;
      }
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace
}  // namespace c2m

using namespace c2m;

extern "C" size_t c2m_pil_bicubic2d_lds_bytes(int Kh, int Kv, int win_h, int win_w) {
  if (Kh <= 0 || Kv <= 0 || win_h <= 0 || win_w <= 0) return 0;
  return lds_bytes(Kh, Kv, win_h, win_w);
}

extern "C" int c2m_pil_bicubic2d_u8(c2m_stream_t stream, const uint8_t* src, const uint8_t* flags, int N,
                                    int planes_per_sample, int H, int W, int out_h, int out_w, const int* h_start,
                                    const int* h_count, const int* h_coeff, int Kh, const int* v_start, const int* v_count,
                                    const int* v_coeff, int Kv, int win_h, int win_w, uint8_t* dst_u8, float* dst_f32,
                                    float* orient_f32) {
  if (!src || !h_start || !h_count || !h_coeff || !v_start || !v_count || !v_coeff || !dst_u8 || N <= 0 ||
      planes_per_sample <= 0 || N % planes_per_sample || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || Kh <= 0 || Kv <= 0 ||
      win_h <= 0 || win_w <= 0 || win_h > H || win_w > W)
    return C2M_ERR_INVALID_ARG;
  if ((long long)Kh * out_w >= (1ll << 31) || (long long)Kv * out_h >= (1ll << 31) || (long long)N * H * W >= (1ll << 31) ||
      (long long)N * out_h * out_w >= (1ll << 31))
    return C2M_ERR_UNSUPPORTED;
  const size_t lds = lds_bytes(Kh, Kv, win_h, win_w);
  if (lds > C2M_PIL2D_LDS_BUDGET) return C2M_ERR_UNSUPPORTED;
  const int tiles_x = ceil_div(out_w, kTile), tiles_y = ceil_div(out_h, kTile);
  const long long blocks = (long long)N * tiles_x * tiles_y;
  if (blocks >= (1ll << 31)) return C2M_ERR_UNSUPPORTED;
  const int vec_out = out_w % 4 == 0 && aligned4(dst_u8) && (!dst_f32 || aligned16(dst_f32));
  const int vec_orient = W % 4 == 0 && aligned16(orient_f32);
  if (int rc = launch_dynamic_lds<pil_bicubic2d_kernel, kThreadsRP>(
          dim3((unsigned)blocks), lds, as_stream(stream), src, flags, planes_per_sample, H, W, out_h, out_w, h_start, h_count,
          h_coeff, Kh, v_start, v_count, v_coeff, Kv, win_h, win_w, tiles_x, tiles_y, vec_out, vec_orient, dst_u8, dst_f32,
          orient_f32))
    return rc;
  return check_launch();
}
