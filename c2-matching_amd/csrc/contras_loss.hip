// contras_loss.hip -- the contrastive correspondence loss of C2-Matching's stage-1 / stage-2 extractor training
// (TeacherContrasModel / StudentContrasDistillationModel.loss_function), fused for the whole batch.
//
// Per sample b with n valid correspondences (CSR offsets[b] .. offsets[b+1]):
//   D1 = normalize(F1) at all H1*W1 positions (channels-last copy), d1_i = D1[ids_i], d2_i = normalize(F2[:, pos2_i]),
//   pos_i  = 2 - 2<d1_i, d2_i>
//   neg2_i = min_j   (2 - 2<d1_i, d2_j> + 10 [cheb(pos2_i, pos2_j) <= r])     j over the n valid rows
//   neg1_i = min_k   (2 - 2<d2_i, D1_k> + 10 [cheb(grid(ids_i), grid(k)) <= r])  k over all H1*W1 positions
//   hinge  = mean_i relu(margin + pos_i - min(neg1_i, neg2_i))
//   KL     = mean_i sum_j p_ij (log p_ij - log q_ij),  p = softmax_j(<t1_i,t2_j>/tau), log q = log_softmax_j(<d1_i,d2_j>/tau)
//
// Structure: no [n x n] or [n x H1W1] matrix is ever stored.  The dense kernels compute 32x32 tiles of dot products
// with v_mfma_f32_32x32x2_f32 (an exact fp32 fma chain) in the TRANSPOSED orientation: the tile's columns (one per lane)
// are the loss rows i, its 16 registers walk the candidates j.  Every lane therefore owns exactly one loss row and
// keeps that row's running statistics (arg-min, online log-sum-exp of S and T, the running sum e^{t-m}(t-s) of the KL)
// in a handful of registers.  The four waves of a workgroup share a 32-row block and split the candidate tiles; their
// statistics are merged in a fixed order, so the forward is bitwise reproducible.
//
// Backward: G_ij = gk_b (q_ij - p_ij) / (n tau) is rebuilt tile by tile from the saved log-sum-exps and immediately
// consumed as the B operand of a second MFMA (grad d1 = G d2 in the rows pass, grad d2 = G^T d1 in the columns pass);
// the four waves' partial products are summed in LDS in a fixed order.  The hinge's sparse terms (pos, and the single
// arg-min each of neg1 / neg2 routes to), the normalisation backward (g - u(u.g)) / |x| and the scatter into NCHW
// grad F1 / grad F2 follow in one wave-per-row kernel that uses fp32 atomics (global_atomic_add_f32): neg1 arg-mins
// may hit any position of F1 and repeated pos2 (rounding collisions) hit the same pixel of F2, so the BACKWARD is not
// bitwise reproducible from run to run; the forward is.
#include "c2m_common.h"

namespace c2m {
namespace {

constexpr int kRows = 32;        // loss rows per workgroup = the lanes of one 32x32 tile
constexpr int kWavesCL = 4;      // waves per workgroup; they split the candidate tiles
constexpr int kThreadsCL = kWavesCL * kWave;
constexpr int kChanPass = 256;   // channels of the backward's output per pass (8 tiles of 32 -> 128 accumulator registers)
constexpr float kNormEps = 1e-12f;
constexpr float kPenalty = 10.f;

struct Ws {
  float* D1;     // [B*HW1][C]   normalised F1, channels-last
  float* n1;     // [B*HW1]      |F1| per position
  float* d2;     // [Ntot][C]    normalised F2 at pos2
  float* n2;     // [Ntot]
  float* t1;     // [Ntot][C]    normalised teacher F1 at ids (stage 2)
  float* t2;     // [Ntot][C]    normalised teacher F2 at pos2 (stage 2)
  float* pos;    // [Ntot]
  float* neg1v;  // [Ntot]
  int* neg1j;    // [Ntot]       arg-min over H1*W1 (position within the sample)
  float* neg2v;  // [Ntot]
  int* neg2j;    // [Ntot]       arg-min over the sample's rows (row within the sample)
  float* lseS;   // [Ntot]
  float* lseT;   // [Ntot]
  float* kl;     // [Ntot]
  float* gd1;    // [Ntot][C]    dense KL gradient wrt d1 (backward, stage 2)
  float* gd2;    // [Ntot][C]    dense KL gradient wrt d2
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Carve the workspace; returns the bytes needed (ws may be null to size only).
size_t carve(char* base, int B, int C, int HW1, int Ntot, bool teacher, Ws* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) -> char* {
    char* p = base ? base + off : nullptr;
    off += align256(bytes);
    return p;
  };
  const size_t P = (size_t)B * HW1, R = (size_t)Ntot, F = sizeof(float);
  Ws t;
  t.D1 = (float*)take(P * C * F);
  t.n1 = (float*)take(P * F);
  t.d2 = (float*)take(R * C * F);
  t.n2 = (float*)take(R * F);
  t.t1 = teacher ? (float*)take(R * C * F) : nullptr;
  t.t2 = teacher ? (float*)take(R * C * F) : nullptr;
  t.pos = (float*)take(R * F);
  t.neg1v = (float*)take(R * F);
  t.neg1j = (int*)take(R * sizeof(int));
  t.neg2v = (float*)take(R * F);
  t.neg2j = (int*)take(R * sizeof(int));
  t.lseS = (float*)take(R * F);
  t.lseT = (float*)take(R * F);
  t.kl = (float*)take(R * F);
  t.gd1 = teacher ? (float*)take(R * C * F) : nullptr;
  t.gd2 = teacher ? (float*)take(R * C * F) : nullptr;
  if (w) *w = t;
  return off;
}

struct Geo {
  int B, C, H1, W1, HW1, H2, W2, HW2, Ntot;
  float margin, radius, tau;
};

__device__ __forceinline__ int sample_of(const int* __restrict__ offsets, int B, int r) {
  int b = 0;
  while (b + 1 < B && offsets[b + 1] <= r) ++b;
  return b;
}

__device__ __forceinline__ float cheb_out(int ay, int ax, int by, int bx, float radius) {
  const int dy = ay > by ? ay - by : by - ay, dx = ax > bx ? ax - bx : bx - ax;
  return (float)(dy > dx ? dy : dx) > radius ? 0.f : kPenalty;   // penalty inside the safe radius, +0 outside
}

// ---- prep 1: normalise F1 at every position of every sample (one thread per position) ------------------------------
__global__ __launch_bounds__(256) void cl_normalize_all(const float* __restrict__ f, int C, int HW, long long total,
                                                        float* __restrict__ out, float* __restrict__ nrm) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const long long b = g / HW, p = g % HW;
  const float* x = f + b * C * HW + p;
  float ss = 0.f;
  for (int c = 0; c < C; ++c) {
    const float v = x[(size_t)c * HW];
    ss = fmaf(v, v, ss);
  }
  const float n = sqrtf(ss), d = fmaxf(n, kNormEps);
  float* o = out + g * C;
  for (int c = 0; c < C; ++c) o[c] = x[(size_t)c * HW] / d;
  nrm[g] = n;
}

// ---- prep 2: gather + normalise the per-row vectors: y = 0 d2 (F2 at pos2), 1 t1 (teacher F1 at ids), 2 t2 -----------
__global__ __launch_bounds__(256) void cl_gather_rows(const float* __restrict__ f2, const float* __restrict__ tf1,
                                                      const float* __restrict__ tf2, const int* __restrict__ ids,
                                                      const int* __restrict__ pos2, const int* __restrict__ offsets, Geo g,
                                                      float* __restrict__ d2, float* __restrict__ n2,
                                                      float* __restrict__ t1, float* __restrict__ t2) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= g.Ntot) return;
  const int which = blockIdx.y;
  const int b = sample_of(offsets, g.B, r);
  const float* src;
  int HW, p;
  float* dst;
  if (which == 1) {
    src = tf1, HW = g.HW1, dst = t1;
    p = min(max(ids[r], 0), g.HW1 - 1);
  } else {
    src = which == 0 ? f2 : tf2, HW = g.HW2, dst = which == 0 ? d2 : t2;
    const int y = min(max(pos2[2 * r], 0), g.H2 - 1), x = min(max(pos2[2 * r + 1], 0), g.W2 - 1);
    p = y * g.W2 + x;
  }
  const float* x = src + (size_t)b * g.C * HW + p;
  float ss = 0.f;
  for (int c = 0; c < g.C; ++c) {
    const float v = x[(size_t)c * HW];
    ss = fmaf(v, v, ss);
  }
  const float n = sqrtf(ss), d = fmaxf(n, kNormEps);
  float* o = dst + (size_t)r * g.C;
  for (int c = 0; c < g.C; ++c) o[c] = x[(size_t)c * HW] / d;
  if (which == 0) n2[r] = n;
}

// ---- the 32x32 dot-product tile: acc[r] = <col_{j(r)}, row_lane> over C, k = h*C/2 + s for lane half h ----------------
template <bool TWO>
__device__ __forceinline__ void dot_tile(const float* __restrict__ colp, const float* __restrict__ rowp,
                                         const float* __restrict__ tcolp, const float* __restrict__ trowp, int half,
                                         f32x16& accS, f32x16& accT) {
  for (int r = 0; r < 16; ++r) accS[r] = 0.f, accT[r] = 0.f;
  for (int q = 0; q < half; q += 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(colp + q);
    const f32x4 b = *reinterpret_cast<const f32x4*>(rowp + q);
    f32x4 ta, tb;
    if (TWO) {
      ta = *reinterpret_cast<const f32x4*>(tcolp + q);
      tb = *reinterpret_cast<const f32x4*>(trowp + q);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      accS = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], accS, 0, 0, 0);
      if (TWO) accT = __builtin_amdgcn_mfma_f32_32x32x2f32(ta[e], tb[e], accT, 0, 0, 0);
    }
  }
}

struct RowStat {
  float bv;   // best (minimum) value
  int bj;     // its index (lowest on ties)
  float mS, sS, mT, sT, A;   // online log-sum-exp of S and T; A = sum e^{t-mT} (t - s)
};

__device__ __forceinline__ void merge_min(RowStat& a, float v, int j) {
  if (v < a.bv || (v == a.bv && j < a.bj)) a.bv = v, a.bj = j;
}

__device__ __forceinline__ void merge_lse(float& m, float& s, float m2, float s2) {
  if (m2 == -INFINITY) return;
  if (m == -INFINITY) { m = m2, s = s2; return; }
  const float M = fmaxf(m, m2);
  s = s * __expf(m - M) + s2 * __expf(m2 - M);
  m = M;
}

__device__ __forceinline__ void merge(RowStat& a, const RowStat& o) {
  merge_min(a, o.bv, o.bj);
  merge_lse(a.mS, a.sS, o.mS, o.sS);
  // T and A share the running max
  if (o.mT != -INFINITY) {
    if (a.mT == -INFINITY) {
      a.mT = o.mT, a.sT = o.sT, a.A = o.A;
    } else {
      const float M = fmaxf(a.mT, o.mT), ea = __expf(a.mT - M), eo = __expf(o.mT - M);
      a.sT = a.sT * ea + o.sT * eo;
      a.A = a.A * ea + o.A * eo;
      a.mT = M;
    }
  }
}

__device__ __forceinline__ RowStat shfl_stat(const RowStat& s, int lane) {
  RowStat o;
  o.bv = __shfl(s.bv, lane);
  o.bj = __shfl(s.bj, lane);
  o.mS = __shfl(s.mS, lane);
  o.sS = __shfl(s.sS, lane);
  o.mT = __shfl(s.mT, lane);
  o.sT = __shfl(s.sT, lane);
  o.A = __shfl(s.A, lane);
  return o;
}

// ---- forward dense sweep.  blockIdx = (row block, sample, mode): mode 0 = neg2 (+ KL when KL), mode 1 = neg1 --------
template <bool KL>
__global__ __launch_bounds__(kThreadsCL) void cl_forward_dense(const int* __restrict__ ids, const int* __restrict__ pos2,
                                                               const int* __restrict__ offsets, Geo g, Ws w) {
  __shared__ RowStat lds[kWavesCL][kRows];
  const int b = blockIdx.y, mode = blockIdx.z;
  const int o = offsets[b], n = offsets[b + 1] - o;
  const int rb = blockIdx.x * kRows;
  if (rb >= n) return;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6, h = lane >> 5, li = lane & 31;
  const int C = g.C, half = C / 2;
  const int i = min(rb + li, n - 1);         // clamped: lanes past the end compute row n-1 and store nothing
  const int ri = o + i;
  const float* D1b = w.D1 + (size_t)b * g.HW1 * C;
  const bool kl = KL && mode == 0;
  const float *rowp, *trowp = nullptr;
  int ry, rx, ncols;
  const int idr = min(max(ids[ri], 0), g.HW1 - 1);   // (clamped: the host builds ids in range; a bad one reads in bounds)
  if (mode == 0) {
    rowp = D1b + (size_t)idr * C;
    if (KL) trowp = w.t1 + (size_t)ri * C;
    ry = pos2[2 * ri], rx = pos2[2 * ri + 1];
    ncols = n;
  } else {
    rowp = w.d2 + (size_t)ri * C;
    ry = idr / g.W1, rx = idr % g.W1;
    ncols = g.HW1;
  }
  rowp += h * half;
  if (trowp) trowp += h * half;

  RowStat st;
  st.bv = INFINITY, st.bj = 0x7fffffff;
  st.mS = st.mT = -INFINITY, st.sS = st.sT = st.A = 0.f;
  const int ntiles = (ncols + 31) / 32;
  for (int tile = wave; tile < ntiles; tile += kWavesCL) {
    const int cb = tile * 32;
    const int cj = min(cb + li, ncols - 1);   // this lane's A-operand column (clamped)
    const float* colp = (mode == 0 ? w.d2 + (size_t)(o + cj) * C : D1b + (size_t)cj * C) + h * half;
    const float* tcolp = kl ? w.t2 + (size_t)(o + cj) * C + h * half : nullptr;
    f32x16 accS, accT;
    if (kl)
      dot_tile<true>(colp, rowp, tcolp, trowp, half, accS, accT);
    else
      dot_tile<false>(colp, rowp, nullptr, nullptr, half, accS, accT);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = cb + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (j >= ncols) continue;
      int cy, cx;
      if (mode == 0) {
        cy = pos2[2 * (o + j)], cx = pos2[2 * (o + j) + 1];
      } else {
        cy = j / g.W1, cx = j % g.W1;
      }
      const float dot = accS[r];
      const float v = (2.f - 2.f * dot) + cheb_out(ry, rx, cy, cx, g.radius);
      if (v < st.bv) st.bv = v, st.bj = j;   // j ascends along the lane's walk: strict < keeps the lowest index
      if (kl) {
        const float s = dot / g.tau, t = accT[r] / g.tau;
        const float eS = __expf(-fabsf(s - st.mS));
        if (s > st.mS) st.sS = st.sS * eS + 1.f, st.mS = s;
        else st.sS += eS;
        const float eT = __expf(-fabsf(t - st.mT));
        if (t > st.mT) st.sT = st.sT * eT + 1.f, st.A = st.A * eT + (t - s), st.mT = t;
        else st.sT += eT, st.A = fmaf(eT, t - s, st.A);
      }
    }
  }
  // lanes l and l+32 hold the same row: fold the upper half into the lower, then the waves in order 0..3
  const RowStat up = shfl_stat(st, lane | 32);
  if (h == 0) {
    merge(st, up);
    lds[wave][li] = st;
  }
  __syncthreads();
  if (wave != 0 || h != 0 || rb + li >= n) return;
  RowStat a = lds[0][li];
  for (int v = 1; v < kWavesCL; ++v) merge(a, lds[v][li]);
  if (mode == 0) {
    w.neg2v[ri] = a.bv;
    w.neg2j[ri] = a.bj;
    // positive distance: plain dot of d1_i and d2_i
    const float* p1 = D1b + (size_t)idr * C;
    const float* p2 = w.d2 + (size_t)ri * C;
    float d = 0.f;
    for (int c = 0; c < C; ++c) d = fmaf(p1[c], p2[c], d);
    w.pos[ri] = 2.f - 2.f * d;
    if (KL) {
      const float lS = a.mS + __logf(a.sS), lT = a.mT + __logf(a.sT);
      w.lseS[ri] = lS;
      w.lseT[ri] = lT;
      w.kl[ri] = (a.A / a.sT - lT) + lS;
    }
  } else {
    w.neg1v[ri] = a.bv;
    w.neg1j[ri] = a.bj;
  }
}

// ---- per-sample means [B][4] = (hinge, pos, neg, kl), fixed-order tree: deterministic --------------------------------
__global__ __launch_bounds__(256) void cl_sample_reduce(const int* __restrict__ offsets, Geo g, Ws w, int has_kl,
                                                        float* __restrict__ out) {
  __shared__ float red[4][256];
  const int b = blockIdx.x, t = threadIdx.x;
  const int o = offsets[b], n = offsets[b + 1] - o;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = t; i < n; i += 256) {
    const int r = o + i;
    const float p = w.pos[r], ng = fminf(w.neg1v[r], w.neg2v[r]);
    s[0] += fmaxf(g.margin + (p - ng), 0.f);
    s[1] += p;
    s[2] += ng;
    if (has_kl) s[3] += w.kl[r];
  }
  for (int k = 0; k < 4; ++k) red[k][t] = s[k];
  __syncthreads();
  for (int stride = 128; stride > 0; stride >>= 1) {
    if (t < stride)
      for (int k = 0; k < 4; ++k) red[k][t] += red[k][t + stride];
    __syncthreads();
  }
  if (t < 4) out[b * 4 + t] = n > 0 ? red[t][0] / (float)n : 0.f;
}

// ---- backward dense KL passes.  blockIdx = (row block, sample, 2*pass + mode): mode 0 rows (grad d1), 1 columns ------
// Lane-side vectors ("rows" of this pass) L_i, streamed candidates M_j.  mode 0: L = d1/t1, M = d2/t2, G indexed [i][j].
// mode 1: L = d2/t2, M = d1/t1, G indexed [j][i] (the softmax rows are then the streamed index).
__global__ __launch_bounds__(kThreadsCL) void cl_backward_dense(const int* __restrict__ ids, const int* __restrict__ offsets,
                                                                const float* __restrict__ grad_terms, Geo g, Ws w) {
  __shared__ float red[kWavesCL][16 * kWave];
  const int b = blockIdx.y, mode = blockIdx.z & 1, pass = blockIdx.z >> 1;
  const int o = offsets[b], n = offsets[b + 1] - o;
  const int rb = blockIdx.x * kRows;
  const int C = g.C, half = C / 2, c0 = pass * kChanPass;
  if (rb >= n || c0 >= C) return;
  const float gk = grad_terms[2 * b + 1];
  const float scale = gk / ((float)n * g.tau);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6, h = lane >> 5, li = lane & 31;
  const int i = min(rb + li, n - 1), ri = o + i;
  const float* D1b = w.D1 + (size_t)b * g.HW1 * C;
  auto vecS = [&](int side, int r) -> const float* {   // side 0: d1 of row r, side 1: d2 of row r (r within sample)
    return side == 0 ? D1b + (size_t)min(max(ids[o + r], 0), g.HW1 - 1) * C : w.d2 + (size_t)(o + r) * C;
  };
  auto vecT = [&](int side, int r) -> const float* { return (side == 0 ? w.t1 : w.t2) + (size_t)(o + r) * C; };
  const int lside = mode == 0 ? 0 : 1, mside = 1 - lside;
  const float* rowp = vecS(lside, i) + h * half;
  const float* trowp = vecT(lside, i) + h * half;
  const float lS_lane = w.lseS[ri], lT_lane = w.lseT[ri];

  f32x16 Y[8];
#pragma unroll
  for (int t = 0; t < 8; ++t)
    for (int r = 0; r < 16; ++r) Y[t][r] = 0.f;
  const int cm = c0 + li * 8;   // this lane's 8 output channels (A operand of the second product)
  const bool cm_ok = cm < C;    // C % 16 == 0: a group of 8 is either whole or absent

  const int ntiles = (n + 31) / 32;
  for (int tile = wave; tile < ntiles; tile += kWavesCL) {
    const int cb = tile * 32;
    const int cj = min(cb + li, n - 1);
    f32x16 accS, accT;
    dot_tile<true>(vecS(mside, cj) + h * half, rowp, vecT(mside, cj) + h * half, trowp, half, accS, accT);
    float G[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = cb + (r & 3) + 8 * (r >> 2) + 4 * h;
      float lS = lS_lane, lT = lT_lane;
      if (mode == 1 && j < n) lS = w.lseS[o + j], lT = w.lseT[o + j];
      const float s = accS[r] / g.tau, t = accT[r] / g.tau;
      G[r] = j < n ? scale * (__expf(s - lS) - __expf(t - lT)) : 0.f;
    }
    // Y[t][m][lane vector] += sum_j M_j[channel(m, t)] G[j][lane]; k of step r for half h is j(r, h)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = min(cb + (r & 3) + 8 * (r >> 2) + 4 * h, n - 1);
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
      if (cm_ok) {
        const float* mp = vecS(mside, j) + cm;
        a0 = *reinterpret_cast<const f32x4*>(mp);
        a1 = *reinterpret_cast<const f32x4*>(mp + 4);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        Y[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[t], G[r], Y[t], 0, 0, 0);
        Y[t + 4] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[t], G[r], Y[t + 4], 0, 0, 0);
      }
    }
  }
  // Y[t] register rr at lane l: channel c0 + m*8 + t with m = (rr&3) + 8(rr>>2) + 4h, lane vector l&31.
  float* dst = mode == 0 ? w.gd1 : w.gd2;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    for (int rr = 0; rr < 16; ++rr) red[wave][rr * kWave + lane] = Y[t][rr];
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * kWave; e += kThreadsCL) {
      const int rr = e / kWave, l = e % kWave;
      const int m = (rr & 3) + 8 * (rr >> 2) + 4 * (l >> 5);
      const int c = c0 + m * 8 + t, row = rb + (l & 31);
      if (c < C && row < n) {
        float s = red[0][e];
        for (int v = 1; v < kWavesCL; ++v) s += red[v][e];
        dst[(size_t)(o + row) * C + c] = s;
      }
    }
    __syncthreads();
  }
}

// (g - u (u.g)) / |x| for one wave: u, g are this lane's `per` elements of the vector
__device__ __forceinline__ float wave_sum(float v) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// ---- backward: hinge terms + normalisation backward + scatter into NCHW grad F1 / grad F2 (one wave per row) ---------
__global__ __launch_bounds__(256) void cl_backward_scatter(const int* __restrict__ ids, const int* __restrict__ pos2,
                                                           const int* __restrict__ offsets,
                                                           const float* __restrict__ grad_terms, Geo g, Ws w, int has_kl,
                                                           float* __restrict__ gf1, float* __restrict__ gf2) {
  const int r = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6);
  if (r >= g.Ntot) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int b = sample_of(offsets, g.B, r);
  const int o = offsets[b], n = offsets[b + 1] - o;
  const int C = g.C;
  const int p1 = ids[r], y2 = pos2[2 * r], x2 = pos2[2 * r + 1];
  if (p1 < 0 || p1 >= g.HW1 || y2 < 0 || y2 >= g.H2 || x2 < 0 || x2 >= g.W2) return;   // (the host never builds these)
  const float gh = grad_terms[2 * b] / (float)n;
  const float pos = w.pos[r], v1 = w.neg1v[r], v2 = w.neg2v[r];
  const bool active = g.margin + (pos - fminf(v1, v2)) > 0.f;
  // torch.minimum's backward: the smaller operand takes the gradient, ties split it in halves
  const float w1 = v1 < v2 ? 1.f : (v1 == v2 ? 0.5f : 0.f), w2 = 1.f - w1;
  const float a = active ? gh : 0.f;
  const int k1 = w.neg1j[r], j2 = w.neg2j[r];
  const bool s1 = active && w1 > 0.f && k1 >= 0 && k1 < g.HW1;
  bool s2 = active && w2 > 0.f && j2 >= 0 && j2 < n;
  if (s2) {
    const int yq = pos2[2 * (o + j2)], xq = pos2[2 * (o + j2) + 1];
    s2 = yq >= 0 && yq < g.H2 && xq >= 0 && xq < g.W2;
  }

  const float* D1b = w.D1 + (size_t)b * g.HW1 * C;
  const float* u1 = D1b + (size_t)p1 * C;
  const float* u2 = w.d2 + (size_t)r * C;
  const float* uk = D1b + (size_t)(s1 ? k1 : 0) * C;
  const float* uj = w.d2 + (size_t)(o + (s2 ? j2 : 0)) * C;
  const float nr1 = w.n1[(size_t)b * g.HW1 + p1], nr2 = w.n2[r];
  const float nrk = w.n1[(size_t)b * g.HW1 + (s1 ? k1 : 0)], nrj = w.n2[o + (s2 ? j2 : 0)];
  const int yj = pos2[2 * (o + (s2 ? j2 : 0))], xj = pos2[2 * (o + (s2 ? j2 : 0)) + 1];
  float* F1b = gf1 + (size_t)b * C * g.HW1;
  float* F2b = gf2 + (size_t)b * C * g.HW2;
  const int q2 = y2 * g.W2 + x2, qj = yj * g.W2 + xj;

  // four contributions, each projected with its own vector's normalisation: 0 -> F1[ids_i], 1 -> F2[pos2_i],
  // 2 -> F1[k1] (neg1 arg-min), 3 -> F2[pos2_j2] (neg2 arg-min)
  float d[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = lane; c < C; c += kWave) {
    float g1 = a * (-2.f * u2[c] + (s2 ? 2.f * w2 * uj[c] : 0.f));
    float g2 = a * (-2.f * u1[c] + (s1 ? 2.f * w1 * uk[c] : 0.f));
    if (has_kl) g1 += w.gd1[(size_t)r * C + c], g2 += w.gd2[(size_t)r * C + c];
    const float g3 = 2.f * a * w1 * u2[c], g4 = 2.f * a * w2 * u1[c];
    d[0] = fmaf(u1[c], g1, d[0]);
    d[1] = fmaf(u2[c], g2, d[1]);
    d[2] = fmaf(uk[c], g3, d[2]);
    d[3] = fmaf(uj[c], g4, d[3]);
  }
  for (int k = 0; k < 4; ++k) d[k] = wave_sum(d[k]);
  auto proj = [](float gv, float u, float dot, float nr) {
    return nr > kNormEps ? (gv - u * dot) / nr : gv / kNormEps;
  };
  for (int c = lane; c < C; c += kWave) {
    float g1 = a * (-2.f * u2[c] + (s2 ? 2.f * w2 * uj[c] : 0.f));
    float g2 = a * (-2.f * u1[c] + (s1 ? 2.f * w1 * uk[c] : 0.f));
    if (has_kl) g1 += w.gd1[(size_t)r * C + c], g2 += w.gd2[(size_t)r * C + c];
    atomicAdd(F1b + (size_t)c * g.HW1 + p1, proj(g1, u1[c], d[0], nr1));
    atomicAdd(F2b + (size_t)c * g.HW2 + q2, proj(g2, u2[c], d[1], nr2));
    if (s1) atomicAdd(F1b + (size_t)c * g.HW1 + k1, proj(2.f * a * w1 * u2[c], uk[c], d[2], nrk));
    if (s2) atomicAdd(F2b + (size_t)c * g.HW2 + qj, proj(2.f * a * w2 * u1[c], uj[c], d[3], nrj));
  }
}

int validate(int B, int C, int H1, int W1, int H2, int W2, int Ntot, int max_n) {
  if (B <= 0 || C <= 0 || H1 <= 0 || W1 <= 0 || H2 <= 0 || W2 <= 0 || Ntot < 0 || max_n < 0 || max_n > Ntot)
    return C2M_ERR_INVALID_ARG;
  if (C % 16 != 0 || C > 512) return C2M_ERR_UNSUPPORTED;
  if ((long long)H1 * W1 > (1 << 20) || (long long)H2 * W2 > (1 << 20) || max_n > (long long)H1 * W1) return C2M_ERR_UNSUPPORTED;
  if ((long long)B * H1 * W1 * C >= (1ll << 40) || (long long)Ntot * C >= (1ll << 40)) return C2M_ERR_UNSUPPORTED;
  return C2M_OK;
}

}  // namespace
}  // namespace c2m

using namespace c2m;

extern "C" size_t c2m_contras_loss_workspace_bytes(int B, int C, int H1, int W1, int Ntot, int with_teacher) {
  if (B <= 0 || C <= 0 || H1 <= 0 || W1 <= 0 || Ntot < 0) return 0;
  return carve(nullptr, B, C, H1 * W1, Ntot, with_teacher != 0, nullptr);
}

extern "C" int c2m_contras_loss_forward_f32(c2m_stream_t stream, const float* f1, const float* f2, const float* tf1,
                                            const float* tf2, int B, int C, int H1, int W1, int H2, int W2,
                                            const int* ids, const int* pos2, const int* offsets, int Ntot, int max_n,
                                            float margin, float safe_radius, float temperature, float* out,
                                            void* workspace, size_t workspace_bytes) {
  int st = validate(B, C, H1, W1, H2, W2, Ntot, max_n);
  if (st != C2M_OK) return st;
  if (!f1 || !f2 || !offsets || !out || (Ntot > 0 && (!ids || !pos2))) return C2M_ERR_INVALID_ARG;
  if ((tf1 == nullptr) != (tf2 == nullptr)) return C2M_ERR_INVALID_ARG;
  const bool teacher = tf1 != nullptr;
  if (teacher && !(temperature > 0.f)) return C2M_ERR_INVALID_ARG;
  const size_t need = carve(nullptr, B, C, H1 * W1, Ntot, teacher, nullptr);
  if (!workspace || workspace_bytes < need) return C2M_ERR_WORKSPACE;
  Ws w;
  carve((char*)workspace, B, C, H1 * W1, Ntot, teacher, &w);
  Geo g{B, C, H1, W1, H1 * W1, H2, W2, H2 * W2, Ntot, margin, safe_radius, temperature};
  hipStream_t s = as_stream(stream);
  const long long P = (long long)B * g.HW1;
  cl_normalize_all<<<(unsigned)((P + 255) / 256), 256, 0, s>>>(f1, C, g.HW1, P, w.D1, w.n1);
  if (Ntot > 0) {
    dim3 gg((Ntot + 255) / 256, teacher ? 3 : 1);
    cl_gather_rows<<<gg, 256, 0, s>>>(f2, tf1, tf2, ids, pos2, offsets, g, w.d2, w.n2, w.t1, w.t2);
  }
  if (max_n > 0) {
    dim3 grid(ceil_div(max_n, kRows), B, 2);
    if (teacher)
      cl_forward_dense<true><<<grid, kThreadsCL, 0, s>>>(ids, pos2, offsets, g, w);
    else
      cl_forward_dense<false><<<grid, kThreadsCL, 0, s>>>(ids, pos2, offsets, g, w);
  }
  cl_sample_reduce<<<B, 256, 0, s>>>(offsets, g, w, teacher ? 1 : 0, out);
  return check_launch();
}

extern "C" int c2m_contras_loss_backward_f32(c2m_stream_t stream, int B, int C, int H1, int W1, int H2, int W2,
                                             const int* ids, const int* pos2, const int* offsets, int Ntot, int max_n,
                                             float margin, float safe_radius, float temperature, int with_teacher,
                                             const float* grad_terms, float* grad_f1, float* grad_f2, void* workspace,
                                             size_t workspace_bytes) {
  int st = validate(B, C, H1, W1, H2, W2, Ntot, max_n);
  if (st != C2M_OK) return st;
  if (!offsets || !grad_terms || !grad_f1 || !grad_f2 || (Ntot > 0 && (!ids || !pos2))) return C2M_ERR_INVALID_ARG;
  const bool teacher = with_teacher != 0;
  if (teacher && !(temperature > 0.f)) return C2M_ERR_INVALID_ARG;
  const size_t need = carve(nullptr, B, C, H1 * W1, Ntot, teacher, nullptr);
  if (!workspace || workspace_bytes < need) return C2M_ERR_WORKSPACE;
  Ws w;
  carve((char*)workspace, B, C, H1 * W1, Ntot, teacher, &w);
  Geo g{B, C, H1, W1, H1 * W1, H2, W2, H2 * W2, Ntot, margin, safe_radius, temperature};
  hipStream_t s = as_stream(stream);
  hipError_t e = hipMemsetAsync(grad_f1, 0, (size_t)B * C * g.HW1 * sizeof(float), s);
  if (e == hipSuccess) e = hipMemsetAsync(grad_f2, 0, (size_t)B * C * g.HW2 * sizeof(float), s);
  if (e != hipSuccess) {
    set_last_error(e);
    return C2M_ERR_LAUNCH;
  }
  if (Ntot == 0 || max_n == 0) return check_launch();
  if (teacher) {
    dim3 grid(ceil_div(max_n, kRows), B, 2 * ceil_div(C, kChanPass));
    cl_backward_dense<<<grid, kThreadsCL, 0, s>>>(ids, offsets, grad_terms, g, w);
  }
  const int rows_per_block = 256 / kWave;
  cl_backward_scatter<<<ceil_div(Ntot, rows_per_block), 256, 0, s>>>(ids, pos2, offsets, grad_terms, g, w,
                                                                     teacher ? 1 : 0, grad_f1, grad_f2);
  return check_launch();
}

extern "C" int c2m_contras_loss_rows_f32(c2m_stream_t stream, int B, int C, int H1, int W1, int Ntot, int with_teacher,
                                         const void* workspace, size_t workspace_bytes, float* pos, float* neg1,
                                         int* neg1_idx, float* neg2, int* neg2_idx) {
  if (B <= 0 || C <= 0 || H1 <= 0 || W1 <= 0 || Ntot < 0) return C2M_ERR_INVALID_ARG;
  if (!pos || !neg1 || !neg1_idx || !neg2 || !neg2_idx) return C2M_ERR_INVALID_ARG;
  const size_t need = carve(nullptr, B, C, H1 * W1, Ntot, with_teacher != 0, nullptr);
  if (!workspace || workspace_bytes < need) return C2M_ERR_WORKSPACE;
  Ws w;
  carve((char*)workspace, B, C, H1 * W1, Ntot, with_teacher != 0, &w);
  hipStream_t s = as_stream(stream);
  const size_t n = (size_t)Ntot * 4;
  hipError_t e = hipSuccess;
  if (n) {
    e = hipMemcpyAsync(pos, w.pos, n, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(neg1, w.neg1v, n, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(neg1_idx, w.neg1j, n, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(neg2, w.neg2v, n, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(neg2_idx, w.neg2j, n, hipMemcpyDeviceToDevice, s);
  }
  if (e != hipSuccess) {
    set_last_error(e);
    return C2M_ERR_LAUNCH;
  }
  return C2M_OK;
}
