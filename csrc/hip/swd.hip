// dcg-variants: bf16
// Sliced Wasserstein distance (Karras et al. 2018, section 5) between the Laplacian-pyramid patch
// descriptors of a real and a generated image set, per pyramid level. fp32 throughout, whatever the
// engine's element type (one build, swd.h). It runs beside the training step, never inside it.
//
// One set of n images x [n][S][S][C] (NHWC), P patches per image, N = n P descriptors of K = 49 C values:
//   swd_down       g_{k+1} = the 5x5 binomial filter of g_k at every second pixel. A workgroup stages a band
//                  of 11 image rows (4 output rows) in LDS, 16-byte accesses where s C % 8 == 0; the
//                  reflect-101 border is resolved there: rows by the source row, columns by a 2-pixel halo
//   swd_laplace    l_k = g_k - up(g_{k+1}), up as its polyphase filter -- even pixel (1, 6, 1) / 8, odd
//                  (1, 1) / 2 per axis -- over a staged band of 6 coarse rows with a 1-pixel halo: the
//                  upsampled image only ever exists in registers
//   swd_centres    the patch centres of a level, int32 [N][2], from Philox (stream 6)
//   swd_stats      per-channel mean / std of the sampled windows: fp64 sums per 256 descriptors, an LDS tree,
//                  then one thread per channel adds the blocks' partials in index order -- no atomics
//   swd_prepare    theta' = theta / |theta| / std_c, zero-padded in k, and bias = -sum_k mean_c theta'_k: the
//                  per-channel normalisation folded into the projection's operands
//   swd_project    proj [J][N] = D theta'^T + bias on v_mfma_f32_16x16x4_f32 (fp32 products: bf16's 2^-8 would
//                  be the size of the distances measured). A 64-descriptor x 128-direction tile per
//                  workgroup; the A tile is gathered as 7x7xC windows straight out of l_k into LDS (the
//                  descriptor matrix never exists in memory), theta' fragments are 16-byte loads of its
//                  k-contiguous rows, the output is direction-major so every column to sort is contiguous
//   swd_sort       one workgroup of 1024 threads per direction: the column through topk's monotone uint32
//                  key into LDS, a bitonic network there, the sorted column kept; N <= 16384: two columns at
//                  once. Then sum_i |a_i - b_i| against the second column or a stored sorted one, per-thread
//                  strided fp64 sums and an LDS tree: a fixed order. N <= 32768, what one workgroup's LDS holds
//   swd_sort_chunks, swd_merge, swd_tile_sum   N in (32768, 2^21]: runs of 16384 keys sorted by the same network
//                  (64 KB of LDS, two workgroups per CU), then log2(N / 16384) merge passes between two key
//                  buffers. A pass is split by merge path: a workgroup owns 4096 output keys of one pair of runs,
//                  two of its waves find the tile's co-ranks by binary search in memory, the 4096 input keys go
//                  to LDS, every thread finds its own co-rank there and merges 16 keys in registers (the left
//                  run first among equals), and the tile leaves through LDS in 16-byte words. The last pass
//                  stores floats (only if asked to) and sums |a - b| against the other sorted column: per
//                  thread in index order, an LDS tree per tile, the tiles' partials added in index order
//   swd_mean       1000 x the mean of the J partials, added in index order
#include "common.h"
#include "swd.h"

namespace dcg {

// ---------------------------------------------------------------- pyramid
constexpr int SWD_DOWN_ROWS = 4;   // output rows per workgroup -> 11 staged rows
constexpr int SWD_LAP_ROWS = 8;    // fine rows per workgroup -> 6 staged coarse rows

// rows [0, nrows) of the band: LDS row lr <- image row src(lr) of x [.][s][s C], at float `body`
template <bool VEC, class Src>
__device__ __forceinline__ void swd_stage_rows(float* lds, const float* __restrict__ img, int nrows, int sC, int LS,
                                               int body, Src src) {
  if (VEC) {
    const int q4 = sC >> 2;
    for (int v = threadIdx.x; v < nrows * q4; v += 256) {
      const int lr = v / q4, q = v - lr * q4;
      *reinterpret_cast<f32x4*>(lds + lr * LS + body + 4 * q) =
          *reinterpret_cast<const f32x4*>(img + (size_t)src(lr) * sC + 4 * q);
    }
  } else {
    for (int v = threadIdx.x; v < nrows * sC; v += 256) {
      const int lr = v / sC, q = v - lr * sC;
      lds[lr * LS + body + q] = img[(size_t)src(lr) * sC + q];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void swd_down_kernel(const float* __restrict__ g, float* __restrict__ out, int s,
                                                       int C, int LS) {
  extern __shared__ __attribute__((aligned(16))) float band[];
  const int so = s >> 1, sC = s * C, body = (2 * C + 3) & ~3;
  const int i0 = blockIdx.x * SWD_DOWN_ROWS, rows = min(SWD_DOWN_ROWS, so - i0), nst = 2 * rows + 3;
  const float* img = g + (size_t)blockIdx.y * s * sC;
  swd_stage_rows<VEC>(band, img, nst, sC, LS, body, [&](int lr) {
    const int y = 2 * i0 - 2 + lr;
    return y < 0 ? -y : (y > s - 1 ? 2 * (s - 1) - y : y);
  });
  __syncthreads();
  for (int v = threadIdx.x; v < nst * 4 * C; v += 256) {  // columns -2, -1, s, s + 1 <- 2, 1, s - 2, s - 3
    const int lr = v / (4 * C), h = (v / C) & 3, c = v % C;
    const int dst = h == 0 ? -2 : h == 1 ? -1 : h == 2 ? s : s + 1, from = h == 0 ? 2 : h == 1 ? 1 : h == 2 ? s - 2 : s - 3;
    band[lr * LS + body + dst * C + c] = band[lr * LS + body + from * C + c];
  }
  __syncthreads();
  const float w[5] = {1.f / 16, 4.f / 16, 6.f / 16, 4.f / 16, 1.f / 16};
  const int soC = so * C, cnt = rows * soC;
  float* dst = out + ((size_t)blockIdx.y * so + i0) * soC;  // the band's outputs are contiguous
  for (int o4 = threadIdx.x * 4; o4 < cnt; o4 += 1024) {
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int o = min(o4 + e, cnt - 1), li = o / soC, rem = o - li * soC, j = rem / C, c = rem - j * C;
      const float* p = band + (2 * li) * LS + body + (2 * j - 2) * C + c;
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 5; ++a) {
        float h = 0.f;
#pragma unroll
        for (int b = 0; b < 5; ++b) h = __builtin_fmaf(w[b], p[a * LS + b * C], h);
        acc = __builtin_fmaf(w[a], h, acc);
      }
      r[e] = acc;
    }
    if (VEC) {  // (s C % 8 == 0 here: cnt is a multiple of 4)
      *reinterpret_cast<f32x4*>(dst + o4) = (f32x4){r[0], r[1], r[2], r[3]};
    } else {
      for (int e = 0; e < 4 && o4 + e < cnt; ++e) dst[o4 + e] = r[e];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void swd_laplace_kernel(const float* __restrict__ g, const float* __restrict__ gn,
                                                          float* __restrict__ l, int s, int C, int LS) {
  extern __shared__ __attribute__((aligned(16))) float band[];
  const int sc = s >> 1, scC = sc * C, sC = s * C, body = (C + 3) & ~3;
  const int p0 = blockIdx.x * SWD_LAP_ROWS, rows = min(SWD_LAP_ROWS, s - p0), nst = rows / 2 + 2;
  const float* img = gn + (size_t)blockIdx.y * sc * scC;
  swd_stage_rows<VEC>(band, img, nst, scC, LS, body, [&](int lr) {  // (fine row 2 sc reflects to 2 sc - 2)
    const int i = p0 / 2 - 1 + lr;
    return i < 0 ? -i : (i > sc - 1 ? sc - 1 : i);
  });
  __syncthreads();
  for (int v = threadIdx.x; v < nst * 2 * C; v += 256) {  // columns -1, sc <- 1, sc - 1
    const int lr = v / (2 * C), h = (v / C) & 1, c = v % C;
    band[lr * LS + body + (h ? sc : -1) * C + c] = band[lr * LS + body + (h ? sc - 1 : 1) * C + c];
  }
  __syncthreads();
  const int cnt = rows * sC;
  const size_t base = ((size_t)blockIdx.y * s + p0) * sC;
  for (int o4 = threadIdx.x * 4; o4 < cnt; o4 += 1024) {
    float x[4];
    if (VEC) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(g + base + o4);
      x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
    } else {
      for (int e = 0; e < 4; ++e) x[e] = o4 + e < cnt ? g[base + o4 + e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int o = min(o4 + e, cnt - 1), pr = o / sC, rem = o - pr * sC, q = rem / C, c = rem - q * C;
      // taps over coarse offsets (-1, 0, 1): even pixel (1, 6, 1) / 8, odd pixel (0, 1, 1) / 2
      const float wy0 = (pr & 1) ? 0.f : 0.125f, wy1 = (pr & 1) ? 0.5f : 0.75f, wy2 = (pr & 1) ? 0.5f : 0.125f;
      const float wx0 = (q & 1) ? 0.f : 0.125f, wx1 = (q & 1) ? 0.5f : 0.75f, wx2 = (q & 1) ? 0.5f : 0.125f;
      const float* p = band + (pr >> 1) * LS + body + ((q >> 1) - 1) * C + c;  // (LDS row 0 = coarse row p0 / 2 - 1)
      const float h0 = wx0 * p[0] + wx1 * p[C] + wx2 * p[2 * C];
      const float h1 = wx0 * p[LS] + wx1 * p[LS + C] + wx2 * p[LS + 2 * C];
      const float h2 = wx0 * p[2 * LS] + wx1 * p[2 * LS + C] + wx2 * p[2 * LS + 2 * C];
      x[e] -= wy0 * h0 + wy1 * h1 + wy2 * h2;
    }
    if (VEC) {
      *reinterpret_cast<f32x4*>(l + base + o4) = (f32x4){x[0], x[1], x[2], x[3]};
    } else {
      for (int e = 0; e < 4 && o4 + e < cnt; ++e) l[base + o4 + e] = x[e];
    }
  }
}

// ---------------------------------------------------------------- patch centres
// Philox-4x32-10 (Random123), as misc.hip's generator of z: the block at counter (p, i, level, stream 6)
__device__ __forceinline__ void swd_philox(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0], hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

__global__ __launch_bounds__(256) void swd_centres_kernel(int* __restrict__ cen, int N, int P, int s, int level,
                                                          uint64_t seed) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  uint32_t c[4] = {(uint32_t)(r % P), (uint32_t)(r / P), (uint32_t)level, (uint32_t)SWD_STREAM};
  swd_philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  cen[2 * r] = 3 + (int)__umulhi(c[0], (uint32_t)(s - 6));
  cen[2 * r + 1] = 3 + (int)__umulhi(c[1], (uint32_t)(s - 6));
}

// float offset of the window of descriptor r (its corner), centres clamped into the image
__device__ __forceinline__ size_t swd_window(const int* __restrict__ cen, int r, int P, int s, int C) {
  const int cy = min(max(cen[2 * r], 3), s - 4), cx = min(max(cen[2 * r + 1], 3), s - 4);
  return (((size_t)(r / P) * s + (cy - 3)) * s + (cx - 3)) * C;
}

// ---------------------------------------------------------------- statistics
__global__ __launch_bounds__(256) void swd_stats_kernel(const float* __restrict__ l, const int* __restrict__ cen, int N,
                                                        int P, int s, int C, double* __restrict__ part) {
  __shared__ double red[256][2 * SWD_MAX_CH];
  const int tid = threadIdx.x, r = blockIdx.x * SWD_STAT_ROWS + tid;
  double acc[2 * SWD_MAX_CH];
#pragma unroll
  for (int c = 0; c < 2 * SWD_MAX_CH; ++c) acc[c] = 0.0;
  if (r < N) {
    const float* w = l + swd_window(cen, r, P, s, C);
    for (int dy = 0; dy < 7; ++dy)
      for (int dx = 0; dx < 7; ++dx)
#pragma unroll
        for (int c = 0; c < SWD_MAX_CH; ++c)
          if (c < C) {
            const double v = (double)w[(dy * s + dx) * C + c];
            acc[2 * c] += v;
            acc[2 * c + 1] += v * v;
          }
  }
#pragma unroll
  for (int c = 0; c < 2 * SWD_MAX_CH; ++c) red[tid][c] = acc[c];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h)
#pragma unroll
      for (int c = 0; c < 2 * SWD_MAX_CH; ++c) red[tid][c] += red[tid + h][c];
    __syncthreads();
  }
  if (tid < 2 * C) part[(size_t)blockIdx.x * 2 * C + tid] = red[0][tid];
}

// stats [2][C] = (mean, std) from the blocks' partials, added in index order
__global__ __launch_bounds__(64) void swd_stats_final_kernel(const double* __restrict__ part, int blocks, int C,
                                                             double count, float* __restrict__ stats) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < blocks; ++b) {
    s1 += part[(size_t)b * 2 * C + 2 * c];
    s2 += part[(size_t)b * 2 * C + 2 * c + 1];
  }
  const double mu = s1 / count;
  stats[c] = (float)mu;
  stats[C + c] = (float)sqrt(s2 / count - mu * mu);  // (0 for a constant channel: the level is then non-finite)
}

__device__ __forceinline__ double swd_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wave per direction
__global__ __launch_bounds__(64) void swd_prepare_kernel(const float* __restrict__ theta, const float* __restrict__ stats,
                                                         float* __restrict__ thetap, float* __restrict__ bias, int C,
                                                         int Kp) {
  const int j = blockIdx.x, lane = threadIdx.x, K = 49 * C;
  const float* t = theta + (size_t)j * K;
  double ss = 0.0;
  for (int k = lane; k < K; k += 64) ss += (double)t[k] * (double)t[k];
  const float nrm = (float)sqrt(swd_wave_sum(ss));
  double b = 0.0;
  for (int k = lane; k < Kp; k += 64) {
    float v = 0.f;
    if (k < K) {
      const int c = k % C;
      v = (t[k] / nrm) / stats[C + c];
      b -= (double)stats[c] * (double)v;
    }
    thetap[(size_t)j * Kp + k] = v;
  }
  b = swd_wave_sum(b);
  if (lane == 0) bias[j] = (float)b;
}

// ---------------------------------------------------------------- projection
constexpr int SWD_BM = 64, SWD_BN = 128;

__global__ __launch_bounds__(256) void swd_project_kernel(const float* __restrict__ l, const int* __restrict__ cen,
                                                          const float* __restrict__ thetap,
                                                          const float* __restrict__ bias, float* __restrict__ proj,
                                                          int N, int P, int s, int C, int Kp) {
  extern __shared__ __attribute__((aligned(16))) float at[];  // [64][Kp + 4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * SWD_BM, n0 = blockIdx.y * SWD_BN + wave * 32;
  const int K = 49 * C, LDA = Kp + 4, rowC = 7 * C, sC = s * C;
  {  // the A tile: thread (row, part) gathers k = part, part + 4, ... of its descriptor's window
    const int row = tid >> 2, part = tid & 3, r = m0 + row;
    const bool ok = r < N;
    const float* w = l + (ok ? swd_window(cen, r, P, s, C) : 0);
    for (int k = part; k < Kp; k += 4) {
      const int dy = k / rowC;
      at[row * LDA + k] = (ok && k < K) ? w[dy * sC + (k - dy * rowC)] : 0.f;
    }
  }
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn) acc[i][jn] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* b0 = thetap + (size_t)(n0 + fr) * Kp + 4 * fq;
  for (int kt = 0; kt < Kp; kt += 16) {  // lane group fq supplies k = kt + 4 fq + e to MFMA e, for A and B alike
    f32x4 a[4], b[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4*>(at + (i * 16 + fr) * LDA + kt + 4 * fq);
#pragma unroll
    for (int jn = 0; jn < 2; ++jn) b[jn] = *reinterpret_cast<const f32x4*>(b0 + (size_t)jn * 16 * Kp + kt);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jn = 0; jn < 2; ++jn)
          acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][e], b[jn][e], acc[i][jn], 0, 0, 0);
  }
#pragma unroll
  for (int jn = 0; jn < 2; ++jn) {  // C fragment: rows 4 fq .. + 3 of column fr -> 16 contiguous bytes of proj[col]
    const int col = n0 + jn * 16 + fr;
    const float bv = bias[col];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = m0 + i * 16 + 4 * fq;
      if (r < N) {
        f32x4 v = acc[i][jn];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] += bv;
        *reinterpret_cast<f32x4*>(proj + (size_t)col * N + r) = v;
      }
    }
  }
}

// ---------------------------------------------------------------- sort and distance
// topk's key (misc.hip topk_key): uint32, monotone in x, -0 < +0, NaNs by their bits; and its inverse
__device__ __forceinline__ uint32_t swd_key(float x) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float swd_unkey(uint32_t k) {
  return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// the bitonic network over keys [nset][N] in LDS, 1024 threads; the caller synchronises before it reads the keys
__device__ __forceinline__ void swd_bitonic(uint32_t* keys, int N, int nset, int tid) {
  const int half = N >> 1;
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int t = tid; t < nset * half; t += 1024) {
        const int set = t >= half, tt = t - set * half;
        const int i = 2 * tt - (tt & (j - 1)), lo = set * N + i, hi = lo + j;
        const uint32_t x = keys[lo], y = keys[hi];
        if ((x > y) == ((i & k) == 0)) {
          keys[lo] = y;
          keys[hi] = x;
        }
      }
    }
}

__global__ __launch_bounds__(1024) void swd_sort_kernel(const float* __restrict__ src0, float* __restrict__ dst0,
                                                        const float* __restrict__ src1, float* __restrict__ dst1,
                                                        const float* __restrict__ ref, double* __restrict__ partial,
                                                        int N) {
  extern __shared__ __attribute__((aligned(16))) uint32_t keys[];  // [1 or 2][N], then double red[1024]
  const int tid = threadIdx.x, nset = src1 ? 2 : 1;
  const size_t col = (size_t)blockIdx.x * N;
  double* red = reinterpret_cast<double*>(keys + nset * N);
  for (int i = tid; i < N; i += 1024) {
    keys[i] = swd_key(src0[col + i]);
    if (src1) keys[N + i] = swd_key(src1[col + i]);
  }
  swd_bitonic(keys, N, nset, tid);
  __syncthreads();
  double acc = 0.0;
  for (int i = tid; i < N; i += 1024) {
    const float a = swd_unkey(keys[i]);
    if (dst0) dst0[col + i] = a;
    float b = 0.f;
    if (src1) {
      b = swd_unkey(keys[N + i]);
      if (dst1) dst1[col + i] = b;
    } else if (ref) {
      b = ref[col + i];
    }
    acc += (double)fabsf(a - b);
  }
  if (!partial) return;
  red[tid] = acc;
  __syncthreads();
  for (int h = 512; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) partial[blockIdx.x] = red[0];
}

// ---------------------------------------------------------------- global merge sort (N > SWD_MAX_ROWS)
// runs: workgroup (c, j) sorts keys [c T, (c + 1) T) of column j in LDS and writes them as uint32 keys
__global__ __launch_bounds__(1024) void swd_sort_chunks_kernel(const float* __restrict__ src,
                                                               uint32_t* __restrict__ keys_out, int N, int T) {
  extern __shared__ __attribute__((aligned(16))) uint32_t keys[];  // [T]
  const int tid = threadIdx.x;
  const size_t off = (size_t)blockIdx.y * N + (size_t)blockIdx.x * T;
  for (int i = 4 * tid; i < T; i += 4096) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + off + i);
    *reinterpret_cast<u32x4*>(keys + i) = (u32x4){swd_key(v[0]), swd_key(v[1]), swd_key(v[2]), swd_key(v[3])};
  }
  swd_bitonic(keys, T, 1, tid);
  __syncthreads();
  for (int i = 4 * tid; i < T; i += 4096)
    *reinterpret_cast<u32x4*>(keys_out + off + i) = *reinterpret_cast<const u32x4*>(keys + i);
}

constexpr int SWD_MERGE_E = SWD_MERGE_TILE / 256;  // keys a thread merges serially
// LDS word of key i while threads merge: thread t walks its two runs from about 8 t words on (E / 2 of either run
// per thread on average), which alone would put a wave on 4 of the 32 banks; one pad word per 8 makes that
// 9 t -- every lane of a half-wave on a bank of its own when the runs interleave evenly
__device__ __forceinline__ int swd_pad_merge(int i) { return i + (i >> 3); }
// ... and while the merged tile goes out: thread t stores its 16 keys as four 16-byte words from word 20 t on (4 pad
// words per 16: eight lanes' 16-byte stores cover all 32 banks once), and reads 16-byte word v back at 4 v + 4 (v >> 2)
__device__ __forceinline__ int swd_pad_out(int i) { return i + ((i >> 4) << 2); }
constexpr int SWD_MERGE_LDS = SWD_MERGE_TILE + SWD_MERGE_TILE / 4;  // words: the larger of the two layouts

// merge path: how many of the first d keys of merge(A [na], B [nb]) come from A, A first among equal keys.
// Reads A[i] for i in [max(0, d - nb), min(d, na)) and B[d - 1 - i] only
template <class FA, class FB>
__device__ __forceinline__ int swd_corank(int d, int na, int nb, FA A, FB B) {
  int lo = max(0, d - nb), hi = min(d, na);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (A(mid) <= B(d - 1 - mid)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One pass: the sorted runs [2 q L, (2 q + 1) L) and [(2 q + 1) L, (2 q + 2) L) of column j of `in` merged; workgroup
// (t, j) makes output keys [t M, (t + 1) M), M = SWD_MERGE_TILE. LAST (2 L = N): the keys go out as floats to dst (if
// given) and, with `other`, tilepart[j][t] = sum |sorted - other| over the tile, per thread in index order, then a tree
template <bool LAST>
__global__ __launch_bounds__(256) void swd_merge_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                        float* __restrict__ dst, const float* __restrict__ other,
                                                        double* __restrict__ tilepart, int N, int L) {
  __shared__ __attribute__((aligned(16))) uint32_t buf[SWD_MERGE_LDS];
  __shared__ int split[2];
  constexpr int M = SWD_MERGE_TILE, E = SWD_MERGE_E;
  const int tid = threadIdx.x;
  const size_t col = (size_t)blockIdx.y * N;
  const int pos = blockIdx.x * M, base = pos & ~(2 * L - 1), d0 = pos - base;
  const uint32_t* __restrict__ A = in + col + base;
  const uint32_t* __restrict__ B = A + L;
  if (tid == 0 || tid == 64)  // the tile's two diagonals, each a chain of dependent global loads: one wave each
    split[tid >> 6] = swd_corank(d0 + (tid ? M : 0), L, L, [&](int i) { return A[i]; }, [&](int i) { return B[i]; });
  __syncthreads();
  const int a0 = split[0], na = split[1] - a0, b0 = d0 - a0, nb = M - na;
  for (int i = tid; i < M; i += 256) buf[swd_pad_merge(i)] = i < na ? A[a0 + i] : B[b0 + (i - na)];
  __syncthreads();
  auto la = [&](int i) { return buf[swd_pad_merge(i)]; };
  auto lb = [&](int i) { return buf[swd_pad_merge(na + i)]; };
  uint32_t r[E];
  {
    int i = swd_corank(tid * E, na, nb, la, lb), j = tid * E - i;
    uint32_t ka = i < na ? la(i) : 0u, kb = j < nb ? lb(j) : 0u;
#pragma unroll
    for (int e = 0; e < E; ++e) {  // (M - tid E >= E keys are left: the two runs never end together before e = E)
      const bool ta = j >= nb || (i < na && ka <= kb);
      r[e] = ta ? ka : kb;
      if (ta) {
        ++i;
        ka = i < na ? la(i) : 0u;
      } else {
        ++j;
        kb = j < nb ? lb(j) : 0u;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < E / 4; ++q)
    *reinterpret_cast<u32x4*>(buf + swd_pad_out(tid * E + 4 * q)) = (u32x4){r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]};
  __syncthreads();
  const size_t o = col + pos;
  double acc = 0.0;
#pragma unroll
  for (int w = 0; w < M / 1024; ++w) {
    const int v = 4 * (tid + 256 * w);
    const u32x4 k = *reinterpret_cast<const u32x4*>(buf + swd_pad_out(v));
    if (!LAST) {
      *reinterpret_cast<u32x4*>(out + o + v) = k;
    } else {
      const f32x4 a = (f32x4){swd_unkey(k[0]), swd_unkey(k[1]), swd_unkey(k[2]), swd_unkey(k[3])};
      if (dst) *reinterpret_cast<f32x4*>(dst + o + v) = a;
      if (other) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(other + o + v);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += (double)fabsf(a[q] - b[q]);
      }
    }
  }
  if (LAST && other) {
    __shared__ double red[256];
    red[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    if (tid == 0) tilepart[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
  }
}

// partial[j] = the column's tile partials, added in index order
__global__ __launch_bounds__(64) void swd_tile_sum_kernel(const double* __restrict__ tilepart, double* __restrict__ partial,
                                                          int tiles, int J) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= J) return;
  double s = 0.0;
  for (int t = 0; t < tiles; ++t) s += tilepart[(size_t)j * tiles + t];
  partial[j] = s;
}

__global__ __launch_bounds__(256) void swd_mean_kernel(const double* __restrict__ partial, double* __restrict__ out,
                                                       int J, double count) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int j = threadIdx.x; j < J; j += 256) acc += partial[j];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = 1000.0 * red[0] / count;
}

static bool swd_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// an image set the kernels index with 32 bits and whose row band fits the LDS budget
static bool swd_images_ok(int n, int s, int C, int halo, int rows) {
  if (n < 1 || s < 16 || C < 1 || C > SWD_MAX_CH || (double)n * s * s * C >= 2147483648.0) return false;
  return (size_t)rows * swd_row_floats(s, C, halo) * sizeof(float) <= (size_t)SWD_BAND_LDS;
}

static bool swd_rows_ok(int n, int P, int s, int C) {
  const long N = (long)n * P;
  return n >= 1 && P >= 1 && N >= SWD_MIN_ROWS && N <= SWD_GLOBAL_MAX_ROWS && (N & (N - 1)) == 0 && s >= 16 && C >= 1 &&
         C <= SWD_MAX_CH && (double)n * s * s * C < 2147483648.0;
}

}  // namespace dcg

using namespace dcg;

extern "C" int dcg_swd_down(const float* g, float* out, int n, int s, int C, hipStream_t st) {
  if (!g || !out || (s & 1) || !swd_images_ok(n, s, C, 2, 2 * SWD_DOWN_ROWS + 3)) return -2;
  const int LS = swd_row_floats(s, C, 2), so = s / 2;
  const size_t shm = (size_t)(2 * SWD_DOWN_ROWS + 3) * LS * sizeof(float);
  const dim3 grid((so + SWD_DOWN_ROWS - 1) / SWD_DOWN_ROWS, n);
  if ((s * C) % 8 == 0 && swd_al16(g) && swd_al16(out))  // (16-byte rows in and out)
    hipLaunchKernelGGL(swd_down_kernel<true>, grid, dim3(256), shm, st, g, out, s, C, LS);
  else
    hipLaunchKernelGGL(swd_down_kernel<false>, grid, dim3(256), shm, st, g, out, s, C, LS);
  return (int)hipGetLastError();
}

extern "C" int dcg_swd_laplace(const float* g, const float* gn, float* l, int n, int s, int C, hipStream_t st) {
  if (!g || !gn || !l || (s & 1) || !swd_images_ok(n, s / 2, C, 1, SWD_LAP_ROWS / 2 + 2)) return -2;
  const int LS = swd_row_floats(s / 2, C, 1);
  const size_t shm = (size_t)(SWD_LAP_ROWS / 2 + 2) * LS * sizeof(float);
  const dim3 grid((s + SWD_LAP_ROWS - 1) / SWD_LAP_ROWS, n);
  if ((s * C) % 8 == 0 && swd_al16(g) && swd_al16(gn) && swd_al16(l))
    hipLaunchKernelGGL(swd_laplace_kernel<true>, grid, dim3(256), shm, st, g, gn, l, s, C, LS);
  else
    hipLaunchKernelGGL(swd_laplace_kernel<false>, grid, dim3(256), shm, st, g, gn, l, s, C, LS);
  return (int)hipGetLastError();
}

extern "C" int dcg_swd_centres(int* cen, int n, int P, int s, int level, uint64_t seed, hipStream_t st) {
  if (!cen || !swd_rows_ok(n, P, s, 1) || level < 0) return -2;
  const int N = n * P;
  hipLaunchKernelGGL(swd_centres_kernel, dim3((N + 255) / 256), dim3(256), 0, st, cen, N, P, s, level, seed);
  return (int)hipGetLastError();
}

extern "C" int dcg_swd_stats(const float* l, const int* cen, int n, int P, int s, int C, double* part, float* stats,
                             hipStream_t st) {
  if (!l || !cen || !part || !stats || !swd_rows_ok(n, P, s, C)) return -2;
  const int N = n * P, blocks = (N + SWD_STAT_ROWS - 1) / SWD_STAT_ROWS;
  hipLaunchKernelGGL(swd_stats_kernel, dim3(blocks), dim3(256), 0, st, l, cen, N, P, s, C, part);
  hipLaunchKernelGGL(swd_stats_final_kernel, dim3(1), dim3(64), 0, st, part, blocks, C, (double)N * 49.0, stats);
  return (int)hipGetLastError();
}

extern "C" int dcg_swd_prepare(const float* theta, const float* stats, float* thetap, float* bias, int J, int C,
                               hipStream_t st) {
  if (!theta || !stats || !thetap || !bias || J < 1 || J > SWD_MAX_DIRS || C < 1 || C > SWD_MAX_CH) return -2;
  hipLaunchKernelGGL(swd_prepare_kernel, dim3(J), dim3(64), 0, st, theta, stats, thetap, bias, C, swd_kpad(C));
  return (int)hipGetLastError();
}

extern "C" int dcg_swd_project(const float* l, const int* cen, const float* thetap, const float* bias, float* proj,
                               int n, int P, int s, int C, int J, hipStream_t st) {
  if (!l || !cen || !thetap || !bias || !proj || !swd_rows_ok(n, P, s, C) || J < SWD_BN || J > SWD_MAX_DIRS ||
      J % SWD_BN || !swd_al16(thetap) || !swd_al16(proj))
    return -2;
  const int N = n * P, Kp = swd_kpad(C);
  const size_t shm = (size_t)SWD_BM * (Kp + 4) * sizeof(float);
  hipLaunchKernelGGL(swd_project_kernel, dim3((N + SWD_BM - 1) / SWD_BM, J / SWD_BN), dim3(256), shm, st, l, cen,
                     thetap, bias, proj, N, P, s, C, Kp);
  return (int)hipGetLastError();
}

extern "C" int dcg_swd_sort_distance(const float* src0, float* dst0, const float* src1, float* dst1, const float* ref,
                                     double* partial, int N, int J, hipStream_t st) {
  if (!src0 || J < 1 || J > SWD_MAX_DIRS || N < SWD_MIN_ROWS || N > SWD_MAX_ROWS || (N & (N - 1))) return -2;
  if (src1 && (N > SWD_FUSED_ROWS || ref)) return -2;
  if (partial && !src1 && !ref) return -2;
  static bool attr = false;
  if (!attr) {  // up to 128 KB of keys: the 160 KB of LDS narrow.hip asks for, too
    hipError_t e = hipFuncSetAttribute((const void*)swd_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  const size_t shm = (size_t)(src1 ? 2 : 1) * N * sizeof(uint32_t) + 1024 * sizeof(double);
  hipLaunchKernelGGL(swd_sort_kernel, dim3(J), dim3(1024), shm, st, src0, dst0, src1, dst1, ref, partial, N);
  return (int)hipGetLastError();
}

extern "C" int dcg_swd_sort_large(const float* src, float* dst, const float* other, uint32_t* keys0, uint32_t* keys1,
                                  double* tilepart, double* partial, int N, int J, hipStream_t st) {
  static_assert(SWD_MERGE_TILE % 1024 == 0 && SWD_MERGE_E % 4 == 0 && SWD_CHUNK_ROWS % 4096 == 0 &&
                SWD_CHUNK_ROWS >= SWD_MERGE_TILE && SWD_CHUNK_ROWS <= SWD_MAX_ROWS, "swd: tile sizes");
  if (!src || !keys0 || !keys1 || keys0 == keys1 || J < 1 || J > SWD_MAX_DIRS || N <= SWD_MAX_ROWS ||
      N > SWD_GLOBAL_MAX_ROWS || (N & (N - 1)))
    return -2;
  if (!swd_al16(src) || !swd_al16(dst) || !swd_al16(other) || !swd_al16(keys0) || !swd_al16(keys1)) return -2;
  if ((other != nullptr) != (partial != nullptr) || (other != nullptr) != (tilepart != nullptr) || (!dst && !other)) return -2;
  constexpr int T = SWD_CHUNK_ROWS, M = SWD_MERGE_TILE;
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void*)swd_sort_chunks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       T * (int)sizeof(uint32_t));
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  hipLaunchKernelGGL(swd_sort_chunks_kernel, dim3(N / T, J), dim3(1024), (size_t)T * sizeof(uint32_t), st, src, keys0, N, T);
  uint32_t *in = keys0, *out = keys1;
  const dim3 grid(N / M, J);
  for (int L = T; 2 * L < N; L <<= 1) {  // all passes but the last, between the two key buffers
    hipLaunchKernelGGL(swd_merge_kernel<false>, grid, dim3(256), 0, st, (const uint32_t*)in, out, (float*)nullptr,
                       (const float*)nullptr, (double*)nullptr, N, L);
    uint32_t* t = in;
    in = out;
    out = t;
  }
  hipLaunchKernelGGL(swd_merge_kernel<true>, grid, dim3(256), 0, st, (const uint32_t*)in, (uint32_t*)nullptr, dst, other,
                     tilepart, N, N / 2);
  if (other) hipLaunchKernelGGL(swd_tile_sum_kernel, dim3((J + 63) / 64), dim3(64), 0, st, (const double*)tilepart, partial, N / M, J);
  return (int)hipGetLastError();
}

extern "C" int dcg_swd_mean(const double* partial, double* out, int N, int J, hipStream_t st) {
  if (!partial || !out || N < 1 || J < 1) return -2;
  hipLaunchKernelGGL(swd_mean_kernel, dim3(1), dim3(256), 0, st, partial, out, J, (double)N * (double)J);
  return (int)hipGetLastError();
}
