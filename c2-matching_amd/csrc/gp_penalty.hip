// gp_penalty.hip -- the WGAN-GP penalty of stage-3 GAN training on the critic's input gradient (reference:
// mmsr/models/losses.py:397-398; here mmsr/models/losses.py GradientPenaltyLoss, c2m_amd.ops.gradient_penalty).
//
//   c2m_gp_penalty_forward_f32    G fp32 [N, M] -> norms[n] = ||G[n, :]||_2, out[0] = mean_n (norms[n] - 1)^2
//   c2m_gp_penalty_backward_f32   dG[n, i] = gout * (2 / N) * (norms[n] - 1) / norms[n] * G[n, i]; 0 where norms[n] == 0
//
// The torch composition of the same expression is 13 element-wise / reduction / copy launches per forward + backward (kernel
// trace) over a tensor of ~1 MB at the training shape (N 4, M 3 * 160 * 160): the launches cost more than
// the bytes.  Here the forward is two launches and the backward one.
//
// Forward.  A sample is cut into P slices of `slice` elements (a multiple of 4 * kThreadsGP; P <= kMaxSlices).  Launch 1,
// grid (P, N): a block adds the squares of its slice.  The slice is walked in groups of 4 consecutive elements, thread t
// takes groups t, t + 256, ...: one 16-byte load per group where the sample's base is 16-byte aligned, four 4-byte loads
// otherwise, and per-element loads with a bound check in the one group that straddles the end of the sample -- the elements a
// thread adds, and their order, are the same in all three forms.  The 64 lanes of a wave are added by a shuffle tree, the
// block's 4 waves through LDS in wave order; the block writes one partial.  Launch 2, one block: thread n adds the P partials
// of sample n in index order (float64), takes the root, writes norms[n]; the (norms[n] - 1)^2 go through a fixed tree.
// No atomics anywhere: the same input gives the same bits on every call.
//
// Backward.  One launch, grid (ceil(M / 1024), N): one group of 4 per thread, the same three load / store forms.  The
// coefficient of sample n is formed from norms[n] and the device-resident gout by every thread; nothing goes to the host.
#include "c2m_common.h"
#include "../../include/c2m_gan_hip.h"

namespace c2m {
namespace {

constexpr int kThreadsGP = 256;
constexpr int kGroup = 4;                                  // elements per 16-byte access
constexpr long long kSliceQuantum = kGroup * kThreadsGP;   // 1024: every thread of a block gets whole groups
constexpr long long kMinSlice = 4 * kSliceQuantum;         // 4 groups per thread
constexpr int kMaxSlices = 256;                            // per sample: launch 2 adds them one after the other
constexpr int kMaxSamples = 65535;                         // grid.y

// slice length for samples of M elements and the number of slices
inline long long slice_of(long long M, int* slices) {
  long long slice = (M + kMaxSlices - 1) / kMaxSlices;
  slice = (slice + kSliceQuantum - 1) / kSliceQuantum * kSliceQuantum;
  if (slice < kMinSlice) slice = kMinSlice;
  *slices = (int)((M + slice - 1) / slice);
  return slice;
}

inline bool sizes_ok(int N, long long M) { return N > 0 && N <= kMaxSamples && M > 0 && M < (1ll << 40); }

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the 4 elements of the group that starts at element `e` of a sample of M elements; elements past the end read as 0
__device__ __forceinline__ f32x4 load_group(const float* __restrict__ row, long long e, long long M, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (e + kGroup <= M) {
    if (vec) {
      v = *reinterpret_cast<const f32x4*>(row + e);
    } else {
      v.x = row[e];
      v.y = row[e + 1];
      v.z = row[e + 2];
      v.w = row[e + 3];
    }
  } else {
    if (e < M) v.x = row[e];
    if (e + 1 < M) v.y = row[e + 1];
    if (e + 2 < M) v.z = row[e + 2];
  }
  return v;
}

// partial [N][P]: the sum of squares of slice blockIdx.x of sample blockIdx.y
__global__ __launch_bounds__(kThreadsGP) void gp_sumsq_kernel(const float* __restrict__ G, long long M, long long slice,
                                                              float* __restrict__ partial) {
  __shared__ float s_wave[kThreadsGP / kWave];
  const int tid = threadIdx.x;
  const int n = blockIdx.y, s = blockIdx.x;
  const float* row = G + (size_t)n * (size_t)M;
  const bool vec = aligned16(row);        // slice and group starts are multiples of 4 elements
  const long long e0 = (long long)s * slice;
  const long long e1 = e0 + slice < M ? e0 + slice : M;
  float acc = 0.f;
  for (long long e = e0 + (long long)tid * kGroup; e < e1; e += kSliceQuantum) {
    const f32x4 v = load_group(row, e, M, vec);
    acc = fmaf(v.x, v.x, acc);
    acc = fmaf(v.y, v.y, acc);
    acc = fmaf(v.z, v.z, acc);
    acc = fmaf(v.w, v.w, acc);
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) acc += __shfl_down(acc, d, kWave);
  if ((tid & (kWave - 1)) == 0) s_wave[tid / kWave] = acc;
  __syncthreads();
  if (tid == 0) {
    float t = s_wave[0];
#pragma unroll
    for (int w = 1; w < kThreadsGP / kWave; ++w) t += s_wave[w];
    partial[(size_t)n * gridDim.x + s] = t;
  }
}

// one block: norms[n] from the P partials of sample n added in index order, out[0] = mean_n (norms[n] - 1)^2
__global__ __launch_bounds__(kThreadsGP) void gp_finish_kernel(const float* __restrict__ partial, int N, int P,
                                                               float* __restrict__ norms, float* __restrict__ out) {
  __shared__ double red[kThreadsGP];
  const int tid = threadIdx.x;
  double terms = 0.0;
  for (int n = tid; n < N; n += kThreadsGP) {
    const float* p = partial + (size_t)n * P;
    double ss = 0.0;
    for (int i = 0; i < P; ++i) ss += (double)p[i];
    const float norm = (float)sqrt(ss);
    norms[n] = norm;
    const double d = (double)norm - 1.0;
    terms += d * d;
  }
  red[tid] = terms;
  __syncthreads();
  for (int s = kThreadsGP / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) out[0] = (float)(red[0] / (double)N);
}

__global__ __launch_bounds__(kThreadsGP) void gp_backward_kernel(const float* __restrict__ G, const float* __restrict__ norms,
                                                                 const float* __restrict__ gout, int N, long long M,
                                                                 float* __restrict__ dG) {
  const int n = blockIdx.y;
  const long long e = ((long long)blockIdx.x * kThreadsGP + threadIdx.x) * kGroup;
  if (e >= M) return;
  const float norm = norms[n];
  // (float64: one rounding for the whole coefficient; a handful of operations per thread next to a 16-byte load and store)
  const float c = norm == 0.f ? 0.f : (float)((double)gout[0] * (2.0 / (double)N) * (((double)norm - 1.0) / (double)norm));
  const float* row = G + (size_t)n * (size_t)M;
  float* drow = dG + (size_t)n * (size_t)M;
  const bool vec = aligned16(row) && aligned16(drow);
  f32x4 v = load_group(row, e, M, vec);
  v.x *= c;
  v.y *= c;
  v.z *= c;
  v.w *= c;
  if (e + kGroup <= M) {
    if (vec) {
      *reinterpret_cast<f32x4*>(drow + e) = v;
    } else {
      drow[e] = v.x;
      drow[e + 1] = v.y;
      drow[e + 2] = v.z;
      drow[e + 3] = v.w;
    }
  } else {
    drow[e] = v.x;                        // e < M
    if (e + 1 < M) drow[e + 1] = v.y;
    if (e + 2 < M) drow[e + 2] = v.z;
  }
}

}  // namespace
}  // namespace c2m

using namespace c2m;

extern "C" size_t c2m_gp_penalty_workspace_bytes(int N, long long M) {
  if (!sizes_ok(N, M)) return 0;
  int slices;
  slice_of(M, &slices);
  return (size_t)N * (size_t)slices * sizeof(float);
}

extern "C" int c2m_gp_penalty_forward_f32(c2m_stream_t stream, const float* grad, int N, long long M, float* norms, float* out,
                                          void* workspace, size_t workspace_bytes) {
  if (!grad || !norms || !out || N <= 0 || M <= 0) return C2M_ERR_INVALID_ARG;
  if (!sizes_ok(N, M)) return C2M_ERR_UNSUPPORTED;
  int slices;
  const long long slice = slice_of(M, &slices);
  if (!workspace || workspace_bytes < (size_t)N * (size_t)slices * sizeof(float)) return C2M_ERR_WORKSPACE;
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(gp_sumsq_kernel, dim3((unsigned)slices, (unsigned)N), dim3(kThreadsGP), 0, as_stream(stream), grad, M,
                     slice, partial);
  if (int rc = check_launch()) return rc;
  hipLaunchKernelGGL(gp_finish_kernel, dim3(1), dim3(kThreadsGP), 0, as_stream(stream), partial, N, slices, norms, out);
  return check_launch();
}

extern "C" int c2m_gp_penalty_backward_f32(c2m_stream_t stream, const float* grad, const float* norms, const float* gout, int N,
                                           long long M, float* dgrad) {
  if (!grad || !norms || !gout || !dgrad || N <= 0 || M <= 0) return C2M_ERR_INVALID_ARG;
  if (!sizes_ok(N, M)) return C2M_ERR_UNSUPPORTED;
  const long long blocks = (M + kSliceQuantum - 1) / kSliceQuantum;     // < 2^30 for M < 2^40
  hipLaunchKernelGGL(gp_backward_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(kThreadsGP), 0, as_stream(stream), grad,
                     norms, gout, N, M, dgrad);
  return check_launch();
}
