// Spectral normalisation of the discriminator's weights: power iteration, normalised copy,
// gradient projection. Bandwidth-bound fp32 streaming (16-byte loads, wave + LDS reductions, no
// MFMA), built for every element type: the normalised copy of a conv kernel is written in elem_t
// into the mirror slice the conv GEMMs read, the head's stays fp32.
//
// Every weight is a matrix W [K, Cout], row-major (TF's reshape(w, [-1, Cout]); the head is
// [K, 1]); an SNTable of up to 8 of them rides in the kernel arguments and each block finds its
// matrix from the table's block counts. Dependencies between workgroups only cross launch
// boundaries; every final reduction reads its partials from a buffer in a fixed order (no float
// atomics), so two runs -- and two ranks -- produce the same bits.
//
// Power step (one iteration from the stored u), eps = 1e-12:
//   sn_wu      t = W u -> v (unnormalised), per-block partials of sum t^2
//   sn_wtv     v = t / max(|t|, eps); per-block column partials of W^T v
//   sn_colsum  s = sum of the column partials -> u (unnormalised), per-tile partials of sum s^2
//              (1024 threads: the partials of a column split over 4 row groups)
//   sn_apply   sigma = max(|s|, eps), u = s / sigma, normalised copy W * (1 / sigma)
//              (from_state: only the copy, from the stored sigma -- init / checkpoint load)
// An overflowed fp16 step (ls[1] != 0) skips all four, as it skips Adam.
// Projection of G = dL/d(W / sigma) to dL/dW = (G - <G, W> / sigma * v u^T) / sigma, in place:
//   sn_dot     per-block partials of <G, W>
//   sn_project the update
#include "common.h"
#include "kernels.h"

namespace dcg {

constexpr float SN_EPS = 1e-12f;

// sum over the 256 threads of a block, the same association in every block; red: 4 floats of LDS
__device__ __forceinline__ float sn_block_sum(float x, float* red) {
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  const float r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}

// the matrix of block `b` and b's index inside it, by the per-matrix block count `cnt`
#define SN_FIND(cnt)                                   \
  int mi = 0, lb = (int)blockIdx.x;                    \
  while (mi < tab.n - 1 && lb >= tab.m[mi].cnt) {      \
    lb -= tab.m[mi].cnt;                               \
    ++mi;                                              \
  }                                                    \
  const SNMat& M = tab.m[mi];                          \
  if (lb >= M.cnt) return;

__global__ __launch_bounds__(256) void sn_wu_kernel(const SNTable tab, const float* __restrict__ ls) {
  if (ls && ls[1] != 0.f) return;
  SN_FIND(nrb)
  __shared__ float red[4];
  const int K = M.K, C = M.Cout;
  const int r0 = lb * M.rpb, r1 = min(r0 + M.rpb, K);
  const int vw = (C & 3) ? 1 : 4, nslot = C / vw;
  int lpr = 1;  // lanes per row (a power of two <= 64: a row's lanes share a wave)
  while (lpr < nslot && lpr < 64) lpr <<= 1;
  const int gpb = 256 / lpr, g = threadIdx.x / lpr, l = threadIdx.x % lpr;
  const int iters = (r1 - r0 + gpb - 1) / gpb;
  float acc2 = 0.f;
  for (int it = 0; it < iters; ++it) {  // (uniform trip count: the shuffles below need every lane)
    const int r = r0 + g + it * gpb;
    const bool ok = r < r1;
    float a = 0.f;
    if (ok) {
      const float* row = M.W + (size_t)r * C;
      if (vw == 4) {
        for (int s = l; s < nslot; s += lpr) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(row + 4 * s);
          const f32x4 uu = *reinterpret_cast<const f32x4*>(M.u + 4 * s);
          a += (w[0] * uu[0] + w[1] * uu[1]) + (w[2] * uu[2] + w[3] * uu[3]);
        }
      } else {
        for (int s = l; s < nslot; s += lpr) a += row[s] * M.u[s];
      }
    }
    for (int o = lpr >> 1; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (ok && l == 0) {
      M.v[r] = a;
      acc2 += a * a;
    }
  }
  const float tot = sn_block_sum(acc2, red);
  if (threadIdx.x == 0) M.ws[SN_WS_TPART + lb] = tot;
}

__global__ __launch_bounds__(256) void sn_wtv_kernel(const SNTable tab, const float* __restrict__ ls) {
  if (ls && ls[1] != 0.f) return;
  SN_FIND(nrb)
  __shared__ float red[4];
  __shared__ float sv[SN_MAX_ROWS_PER_BLOCK];
  __shared__ f32x4 cred[256];
  const int K = M.K, C = M.Cout;
  const int r0 = lb * M.rpb, nrows = min(M.rpb, K - r0);
  const int tid = threadIdx.x;
  const float nt2 = sn_block_sum(tid < M.nrb ? M.ws[SN_WS_TPART + tid] : 0.f, red);
  const float nt = fmaxf(sqrtf(nt2), SN_EPS);
  for (int i = tid; i < nrows; i += 256) {
    const float x = M.v[r0 + i] / nt;
    sv[i] = x;
    M.v[r0 + i] = x;
  }
  __syncthreads();
  const int vw = (C & 3) ? 1 : 4, nslot = C / vw;
  int tc_n = 1;  // threads across the columns (a power of two), the rest across the rows
  while (tc_n < nslot && tc_n < 256) tc_n <<= 1;
  const int rg_n = 256 / tc_n, tc = tid % tc_n, rg = tid / tc_n;
  float* cpart = M.ws + SN_WS_CPART + (size_t)lb * C;
  for (int c0 = 0; c0 < nslot; c0 += tc_n) {
    const int slot = c0 + tc;
    const bool ok = slot < nslot;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (ok) {
      const float* col = M.W + (size_t)r0 * C + (size_t)slot * vw;
      if (vw == 4) {
        for (int r = rg; r < nrows; r += rg_n) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(col + (size_t)r * C);
          const float x = sv[r];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(w[j], x, acc[j]);
        }
      } else {
        for (int r = rg; r < nrows; r += rg_n) acc[0] = __builtin_fmaf(col[(size_t)r * C], sv[r], acc[0]);
      }
    }
    cred[tid] = acc;
    __syncthreads();
    if (ok && rg == 0) {
      f32x4 s = cred[tc];
      for (int q = 1; q < rg_n; ++q) s += cred[q * tc_n + tc];
      for (int j = 0; j < vw; ++j) cpart[slot * vw + j] = s[j];
    }
    __syncthreads();
  }
}

// 1024 threads: 256 columns x 4 row groups. Each thread adds every 4th row-block partial of its
// column (four independent chains, so the loads overlap), the groups meet in LDS in a fixed order.
__global__ __launch_bounds__(1024) void sn_colsum_kernel(const SNTable tab, const float* __restrict__ ls) {
  if (ls && ls[1] != 0.f) return;
  SN_FIND(nct)
  __shared__ float part[4][256];
  __shared__ float red[4];
  const int C = M.Cout, tc = (int)threadIdx.x & 255, rg = (int)threadIdx.x >> 8, c = lb * 256 + tc;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < C) {
    const float* cpart = M.ws + SN_WS_CPART + c;
    const int nrb = M.nrb;
    int j = rg;
    for (; j + 12 < nrb; j += 16) {
      s0 += cpart[(size_t)j * C];
      s1 += cpart[(size_t)(j + 4) * C];
      s2 += cpart[(size_t)(j + 8) * C];
      s3 += cpart[(size_t)(j + 12) * C];
    }
    for (; j < nrb; j += 4) s0 += cpart[(size_t)j * C];
  }
  part[rg][tc] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  float sq = 0.f;  // row group 0 (the first four waves) finishes its column
  if (rg == 0 && c < C) {
    const float s = (part[0][tc] + part[1][tc]) + (part[2][tc] + part[3][tc]);
    M.u[c] = s;
    sq = s * s;
  }
  sq = wave_sum(sq);
  if (rg == 0 && (tc & 63) == 0) red[tc >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) M.ws[SN_WS_SPART + lb] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void sn_apply_kernel(const SNTable tab, int from_state, const float* __restrict__ ls) {
  if (ls && ls[1] != 0.f) return;
  SN_FIND(ncb)
  const int tid = threadIdx.x;
  float sg;
  if (from_state) {
    sg = M.sigma[0];
  } else {
    float s2 = 0.f;
    for (int j = 0; j < M.nct; ++j) s2 += M.ws[SN_WS_SPART + j];
    sg = fmaxf(sqrtf(s2), SN_EPS);
    if (lb == 0) {  // (no other block of this launch reads u or sigma)
      for (int c = tid; c < M.Cout; c += 256) M.u[c] = M.u[c] / sg;
      if (tid == 0) M.sigma[0] = sg;
    }
  }
  const float inv = 1.f / sg;
  const size_t n = (size_t)M.K * M.Cout, n4 = n / 4, stride = (size_t)M.ncb * 256;
  const bool f32 = M.hat_f32 || sizeof(elem_t) == 4;
  for (size_t i = (size_t)lb * 256 + tid; i < n4; i += stride) {
    f32x4 w = reinterpret_cast<const f32x4*>(M.W)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] *= inv;
    if (f32) {
      reinterpret_cast<f32x4*>(M.hat)[i] = w;
    } else {
      const elem4 o = {(elem_t)w[0], (elem_t)w[1], (elem_t)w[2], (elem_t)w[3]};
      reinterpret_cast<elem4*>(M.hat)[i] = o;
    }
  }
  for (size_t i = n4 * 4 + (size_t)lb * 256 + tid; i < n; i += stride) {
    const float w = M.W[i] * inv;
    if (f32) reinterpret_cast<float*>(M.hat)[i] = w;
    else reinterpret_cast<elem_t*>(M.hat)[i] = (elem_t)w;
  }
}

__global__ __launch_bounds__(256) void sn_dot_kernel(const SNTable tab) {
  SN_FIND(ncb)
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const size_t n = (size_t)M.K * M.Cout, n4 = n / 4, stride = (size_t)M.ncb * 256;
  float acc = 0.f;
  for (size_t i = (size_t)lb * 256 + tid; i < n4; i += stride) {
    const f32x4 g = reinterpret_cast<const f32x4*>(M.grad)[i];
    const f32x4 w = reinterpret_cast<const f32x4*>(M.W)[i];
    acc += (g[0] * w[0] + g[1] * w[1]) + (g[2] * w[2] + g[3] * w[3]);
  }
  for (size_t i = n4 * 4 + (size_t)lb * 256 + tid; i < n; i += stride) acc += M.grad[i] * M.W[i];
  const float tot = sn_block_sum(acc, red);
  if (tid == 0) M.ws[SN_WS_DPART + lb] = tot;
}

__global__ __launch_bounds__(256) void sn_project_kernel(const SNTable tab) {
  SN_FIND(ncb)
  __shared__ float red[4];
  const int tid = threadIdx.x, C = M.Cout;
  float p = 0.f;
  for (int j = tid; j < M.ncb; j += 256) p += M.ws[SN_WS_DPART + j];
  const float dot = sn_block_sum(p, red);
  const float inv = 1.f / M.sigma[0];
  const float coef = dot * inv;  // <G, W / sigma>
  const size_t n = (size_t)M.K * C, stride = (size_t)M.ncb * 256;
  if ((C & 3) == 0) {
    const size_t n4 = n / 4;
    for (size_t i = (size_t)lb * 256 + tid; i < n4; i += stride) {
      const unsigned e = (unsigned)(i * 4), k = e / (unsigned)C, c = e % (unsigned)C;
      f32x4 g = reinterpret_cast<f32x4*>(M.grad)[i];
      const f32x4 uu = *reinterpret_cast<const f32x4*>(M.u + c);
      const float cv = coef * M.v[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = (g[j] - cv * uu[j]) * inv;
      reinterpret_cast<f32x4*>(M.grad)[i] = g;
    }
  } else {
    for (size_t i = (size_t)lb * 256 + tid; i < n; i += stride) {
      const unsigned k = (unsigned)i / (unsigned)C, c = (unsigned)i % (unsigned)C;
      M.grad[i] = (M.grad[i] - coef * M.v[k] * M.u[c]) * inv;
    }
  }
}

static unsigned sn_blocks(const SNTable* t, int which) {
  unsigned b = 0;
  for (int i = 0; i < t->n; ++i) b += (unsigned)(which == 0 ? t->m[i].nrb : which == 1 ? t->m[i].nct : t->m[i].ncb);
  return b;
}

}  // namespace dcg

using namespace dcg;

extern "C" int DCG_API(dcg_sn_wu)(const SNTable* t, const float* ls, hipStream_t s) {
  hipLaunchKernelGGL(sn_wu_kernel, dim3(sn_blocks(t, 0)), dim3(256), 0, s, *t, ls);
  return (int)hipGetLastError();
}

extern "C" int DCG_API(dcg_sn_wtv)(const SNTable* t, const float* ls, hipStream_t s) {
  hipLaunchKernelGGL(sn_wtv_kernel, dim3(sn_blocks(t, 0)), dim3(256), 0, s, *t, ls);
  return (int)hipGetLastError();
}

extern "C" int DCG_API(dcg_sn_colsum)(const SNTable* t, const float* ls, hipStream_t s) {
  hipLaunchKernelGGL(sn_colsum_kernel, dim3(sn_blocks(t, 1)), dim3(1024), 0, s, *t, ls);
  return (int)hipGetLastError();
}

extern "C" int DCG_API(dcg_sn_apply)(const SNTable* t, int from_state, const float* ls, hipStream_t s) {
  hipLaunchKernelGGL(sn_apply_kernel, dim3(sn_blocks(t, 2)), dim3(256), 0, s, *t, from_state, ls);
  return (int)hipGetLastError();
}

extern "C" int DCG_API(dcg_sn_dot)(const SNTable* t, hipStream_t s) {
  hipLaunchKernelGGL(sn_dot_kernel, dim3(sn_blocks(t, 2)), dim3(256), 0, s, *t);
  return (int)hipGetLastError();
}

extern "C" int DCG_API(dcg_sn_project)(const SNTable* t, hipStream_t s) {
  hipLaunchKernelGGL(sn_project_kernel, dim3(sn_blocks(t, 2)), dim3(256), 0, s, *t);
  return (int)hipGetLastError();
}
