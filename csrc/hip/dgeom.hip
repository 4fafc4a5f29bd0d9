// dcg-variants: bf16 f16 f32
// ADA's geometric augmentations on D's input for gfx950 (kernels.h GeomPolicy): x-flip, 90-degree turns,
// isotropic scaling and arbitrary rotation of x [N][S][S][C] as ONE bilinear resampling per sample, with
// reflected borders, and its exact transpose.
//
//   sample n : ONE Philox block w0..w3 at counter (n, t = *step, GEOM_STREAM) of the step's z seed
//   flip = w0 >> 31, k = (w0 >> 29) & 3, s = exp2(0.2 e), e = the even-lane Box-Muller normal of (w1, w2) as
//   instance noise draws it, theta = (float(w3 >> 8) 2^-24 - 0.5) 2 pi
//   M = F^flip Q^k (1 / s) R(theta), F = [[-1, 0], [0, 1]], Q = [[0, -1], [1, 0]], R = [[cos, -sin], [sin, cos]],
//   a factor whose policy is off (mask, or gate of GEOM_GATE_STREAM under adaptive augmentation) = identity
//   output (i, j): u = j - c, v = i - c, c = (S - 1) / 2; xs = m00 u + m01 v + c, ys = m10 u + m11 v + c
//   fold(x) = reflect-101 over any number of periods T = 2 (S - 1): m = x mod T, m > S - 1 -> T - m
//   x0 = floor(fold(xs)), fx = fold(xs) - x0, x1 = min(x0 + 1, S - 1), the same in y
//   y[n,i,j,:] = elem_t((1 - fy) ((1 - fx) x[y0,x0] + fx x[y0,x1]) + fy ((1 - fx) x[y1,x0] + fx x[y1,x1]))
//
// Work split, both kernels: one workgroup of 1024 threads per image, so the draw, the gate and the matrix are
// workgroup-uniform -- thread 0 computes and records them (params [n][8], gates [n]), the rest read them from
// LDS behind one barrier. The workgroup stages its image in LDS once (64x64x3 bf16: 24 KB, 128x128x3 bf16:
// 96 KB) and the four taps of a pixel become LDS reads: a rotated read pattern has no row locality for global
// loads to use. Images beyond the 160 KB the project asks of a CU (256x256, fp32 at 128) keep their taps in
// global memory and are split over several workgroups per image.
// LDS layout: rows of S * C elements at a pitch padded to an ODD number of dwords. A wave walks a line of
// the source whose direction is the sample's: along x consecutive dwords, along y one pitch per pixel -- with
// the unpadded pitch of 64x64x3 bf16 (96 dwords) a 90-degree turn would put a wave's 64 reads on 2 banks;
// an odd pitch is coprime to the bank count, so a walk along y spreads over all of them as one along x does.
// Stores are 16 bytes per thread over the row-flattened image where rows are a multiple of 16 bytes, else
// element stores. A sample whose matrix is the identity (effective policy 0) is a vector copy; one whose
// matrix is a signed permutation moves element bits from the one tap with weight 1 (the lerp would give the
// same bits for finite values; -0 and NaN payloads survive the move).
//
// The transpose (d_geom_bwd_kernel) is a gather with no atomics and no scatter: one thread owns one input
// pixel (p, q) and sums w * g over the output pixels whose taps land on it, in an enumeration order that
// depends on (S, C, the matrix) alone. It recomputes every candidate's taps with geom_taps, the forward's own
// function, so its weights are the forward's bit for bit; the function also returns, per axis, the reflection
// image (period, flipped or not) the candidate's source point lies in, and a candidate counts for the image
// being enumerated only: images of (p, q) that coincide or whose candidate boxes overlap share no term.
//   images per axis: q + k T and (k + 1) T - q for the periods k the sample's source box reaches. The source
//   box is c +- c (|m_a0| + |m_a1|): at the strongest zoom-out (1 / s = 2.227, a 45-degree turn) about -2.1 c
//   .. 4.1 c, 5 images per axis, 25 per pixel; at s = 1 mostly 1, near the borders 2 per axis.
//   candidates per image: the output pixels inside M^-1 of the open box of +-1 around the image, a box of
//   about (2 (|i_a0| + |i_a1|) + 1)^2 pixels, i = M^-1: 3x3 at the zoom-out above, 7x7 at the strongest
//   zoom-in (1 / s = 0.449), where there is one image.
#include <type_traits>

#include "kernels.h"

namespace dcg {

constexpr int GEOM_THREADS = 1024;
constexpr size_t GEOM_LDS_BYTES = 160 * 1024 - 256;  // of the staged image (the rest: the matrix)
constexpr unsigned GEOM_ITERS = 4;                   // 16-byte stores (pixels: transpose) per thread without LDS

// the block at counter (n, 0, lo32(t), hi32(t) ^ stream), key = seed: Philox-4x32-10 as misc.hip's philox_block
__device__ __forceinline__ void geom_philox(uint32_t n, uint64_t seed, uint64_t t, uint64_t stream, uint32_t (&c)[4]) {
  c[0] = n; c[1] = 0u; c[2] = (uint32_t)t; c[3] = (uint32_t)(t >> 32) ^ (uint32_t)stream;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the sample's map in the form every thread reads it: the matrix, the centre, S - 1, the period and 1 / period
struct GeomMap {
  float m00, m01, m10, m11, c, lim, T, invT;
};

// one axis of a source point: taps i0, i1 = min(i0 + 1, S - 1) with weights 1 - f, f, and the reflection
// image the point lies in as label = 2 * period + (1 if mirrored)
struct GeomAxis {
  int i0, i1, label;
  float f;
};

// fold(x) and its taps. Every product that feeds a sum is an explicit fma, so the forward and the transpose,
// which inline this into different loops, round alike. A non-finite or absurd x (a matrix handed to the probe)
// ends on pixel 0: the clamps order NaN away, no index leaves 0 .. S - 1. The period's rounding (x a hair off a
// multiple of T) moves m a hair outside [0, T); the clamp puts it on the border pixel, where fold is continuous.
__device__ __forceinline__ GeomAxis geom_fold(float x, const GeomMap& g) {
  float k = floorf(x * g.invT);
  k = fminf(fmaxf(k, -1048576.f), 1048576.f);
  const float m = __builtin_fmaf(-k, g.T, x);
  const bool mirrored = m > g.lim;
  float r = mirrored ? g.T - m : m;
  r = fminf(fmaxf(r, 0.f), g.lim);
  const float fl = floorf(r);
  GeomAxis a;
  a.i0 = (int)fl;
  a.i1 = min(a.i0 + 1, (int)g.lim);
  a.f = r - fl;
  a.label = 2 * (int)k + (int)mirrored;
  return a;
}

// THE tap function of output pixel (i, j): the forward samples with it, the transpose finds its terms with it
__device__ __forceinline__ void geom_taps(const GeomMap& g, int i, int j, GeomAxis& ax, GeomAxis& ay) {
  const float u = (float)j - g.c, v = (float)i - g.c;  // exact: S <= 2^14
  ax = geom_fold(__builtin_fmaf(g.m00, u, __builtin_fmaf(g.m01, v, g.c)), g);
  ay = geom_fold(__builtin_fmaf(g.m10, u, __builtin_fmaf(g.m11, v, g.c)), g);
}

enum GeomKind : int { GEOM_COPY = 0, GEOM_BLIT = 1, GEOM_WARP = 2 };

// what a matrix asks for: nothing (the identity, or a one-pixel image), a move of pixels (a signed
// permutation: every source point is a pixel centre, every weight 0 or 1), or the resampling
__device__ __forceinline__ int geom_kind(const float* m, int S) {
  if (S == 1 || (m[0] == 1.f && m[1] == 0.f && m[2] == 0.f && m[3] == 1.f)) return GEOM_COPY;
  const bool diag = fabsf(m[0]) == 1.f && m[1] == 0.f && m[2] == 0.f && fabsf(m[3]) == 1.f;
  const bool anti = m[0] == 0.f && fabsf(m[1]) == 1.f && fabsf(m[2]) == 1.f && m[3] == 0.f;
  return diag || anti ? GEOM_BLIT : GEOM_WARP;
}

__device__ __forceinline__ GeomMap geom_map(const float* m, int S) {
  GeomMap g;
  g.m00 = m[0]; g.m01 = m[1]; g.m10 = m[2]; g.m11 = m[3];
  g.c = 0.5f * (float)(S - 1);
  g.lim = (float)(S - 1);
  g.T = 2.f * g.lim;
  g.invT = S > 1 ? 1.f / g.T : 0.f;
  return g;
}

// elements [lo, hi) of one image, bit for bit: 16 bytes per thread where both are aligned (vcopy), else elements
template <typename E>
__device__ __forceinline__ void geom_copy(const E* __restrict__ xi, E* __restrict__ yi, unsigned lo, unsigned hi,
                                          int vcopy) {
  constexpr unsigned V = 16 / sizeof(E);
  if (vcopy) {  // lo and hi are multiples of V
    for (unsigned e = lo + threadIdx.x * V; e < hi; e += GEOM_THREADS * V)
      *reinterpret_cast<u32x4*>(yi + e) = *reinterpret_cast<const u32x4*>(xi + e);
  } else {
    typedef typename std::conditional<sizeof(E) == 2, uint16_t, uint32_t>::type U;
    for (unsigned e = lo + threadIdx.x; e < hi; e += GEOM_THREADS)
      reinterpret_cast<U*>(yi)[e] = reinterpret_cast<const U*>(xi)[e];
  }
}

// the image's S rows of RC elements into LDS at `pitch` elements per row (an odd number of dwords): 16-byte
// global loads split into four dword writes where rows are a multiple of 16 bytes (vstage), else elements
template <typename E>
__device__ __forceinline__ void geom_stage(const E* __restrict__ xi, E* lds, unsigned S, unsigned RC, unsigned pitch,
                                           int vstage) {
  constexpr unsigned V = 16 / sizeof(E);
  if (vstage) {
    const unsigned nq = S * RC / V;
    for (unsigned q = threadIdx.x; q < nq; q += GEOM_THREADS) {
      const u32x4 v = reinterpret_cast<const u32x4*>(xi)[q];
      const unsigned e = q * V, r = e / RC;
      uint32_t* d = reinterpret_cast<uint32_t*>(lds + r * pitch + (e - r * RC));
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
  } else {
    for (unsigned e = threadIdx.x; e < S * RC; e += GEOM_THREADS) {
      const unsigned r = e / RC;
      lds[r * pitch + (e - r * RC)] = xi[e];
    }
  }
  __syncthreads();
}

// flags of the launch, computed by the host from the shapes and the pointers' alignment
enum GeomFlags : int { GEOM_VSTORE = 1, GEOM_VSTAGE = 2, GEOM_VCOPY = 4 };

// MODE 0: draw, record, apply. MODE 1 (the probe): apply the matrix of params[n] as it is. GATED: the effective
// policy is policy & gate mask -- drawn from GEOM_GATE_STREAM against p24 = ada[0] and recorded in gates[n]
// (MODE 0), or read from gates[n] (MODE 1). An effective policy of 0 is the identity whatever params holds.
// bpi workgroups per image, each `chunk` elements of it (bpi = 1 whenever the image is staged: pitch > 0).
template <typename E, int MODE, bool GATED>
__global__ __launch_bounds__(GEOM_THREADS) void d_geom_kernel(const E* __restrict__ x, E* __restrict__ y,
                                                              float* __restrict__ params, int S, int C, int policy,
                                                              unsigned bpi, unsigned chunk, unsigned pitch, int flags,
                                                              uint64_t seed, const unsigned long long* __restrict__ step,
                                                              int* __restrict__ gates, const int* __restrict__ ada) {
  extern __shared__ __attribute__((aligned(16))) unsigned char geom_lds[];
  __shared__ float sm[4];
  const unsigned n = blockIdx.x / bpi, part = blockIdx.x - n * bpi;
  if (threadIdx.x == 0) {
    int eff = policy;
    float* row = params + (size_t)GEOM_PARAMS * n;
    float m[4] = {1.f, 0.f, 0.f, 1.f};
    if (MODE == 0) {
      const unsigned long long t = step[0];
      if (GATED) {
        uint32_t gw[4];
        geom_philox(n, seed, t, GEOM_GATE_STREAM, gw);
        const uint32_t p24 = (uint32_t)ada[0];
        int on = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) on |= (gw[b] >> 8) < p24 ? 1 << b : 0;
        eff &= on;
        if (part == 0) gates[n] = eff;
      }
      uint32_t w[4];
      geom_philox(n, seed, t, GEOM_STREAM, w);
      const int flip = (int)(w[0] >> 31), k = (int)((w[0] >> 29) & 3u);
      const float u0 = (float)((w[1] >> 8) + 1u) * (1.0f / 16777216.0f);
      const float u1 = (float)(w[2] >> 8) * (1.0f / 16777216.0f);
      float sn, cs;
      sincospif(2.f * u1, &sn, &cs);
      const float s = exp2f(GEOM_LOG2_SIGMA * (sqrtf(-2.f * logf(u0)) * cs));
      const float turn = (float)(w[3] >> 8) * (1.0f / 16777216.0f) - 0.5f;  // exact
      const float theta = turn * 6.2831855f;
      if (eff & GEOM_ROTATE) {
        sincospif(2.f * turn, &sn, &cs);  // of the exact angle, not of the rounded theta
        m[0] = cs; m[1] = -sn; m[2] = sn; m[3] = cs;
      }
      if (eff & GEOM_SCALE) {
        const float r = 1.f / s;
        m[0] *= r; m[1] *= r; m[2] *= r; m[3] *= r;
      }
      if (eff & GEOM_ROT90) {
        for (int q = 0; q < k; ++q) {  // Q A = [[-a10, -a11], [a00, a01]]
          const float a00 = m[0], a01 = m[1];
          m[0] = -m[2]; m[1] = -m[3]; m[2] = a00; m[3] = a01;
        }
      }
      if ((eff & GEOM_XFLIP) && flip) { m[0] = -m[0]; m[1] = -m[1]; }
      if (part == 0) {
        row[0] = m[0]; row[1] = m[1]; row[2] = m[2]; row[3] = m[3];
        row[4] = s; row[5] = theta; row[6] = (float)flip; row[7] = (float)k;
      }
    } else {
      if (GATED) eff &= gates[n];
      if (eff) { m[0] = row[0]; m[1] = row[1]; m[2] = row[2]; m[3] = row[3]; }
    }
    sm[0] = m[0]; sm[1] = m[1]; sm[2] = m[2]; sm[3] = m[3];
  }
  __syncthreads();
  const float m[4] = {sm[0], sm[1], sm[2], sm[3]};
  const int kind = geom_kind(m, S);
  const unsigned RC = (unsigned)(S * C), HWC = (unsigned)S * RC;
  const E* xi = x + (size_t)n * HWC;
  E* yi = y + (size_t)n * HWC;
  const unsigned lo = part * chunk, hi = min(HWC, lo + chunk);
  if (kind == GEOM_COPY) {
    geom_copy(xi, yi, lo, hi, flags & GEOM_VCOPY);
    return;
  }
  E* lds = reinterpret_cast<E*>(geom_lds);
  if (pitch) geom_stage(xi, lds, (unsigned)S, RC, pitch, flags & GEOM_VSTAGE);
  const GeomMap g = geom_map(m, S);
  const unsigned uc = (unsigned)C;
  auto ld = [&](int yy, int xx, unsigned ch) -> E {
    return pitch ? lds[(unsigned)yy * pitch + (unsigned)xx * uc + ch]
                 : xi[((unsigned)yy * (unsigned)S + (unsigned)xx) * uc + ch];
  };
  // element ch of output pixel (i, j) under its taps
  auto sample = [&](const GeomAxis& ax, const GeomAxis& ay, unsigned ch) -> E {
    if (kind == GEOM_BLIT) return ld(ay.i0, ax.i0, ch);
    const float gx = 1.f - ax.f, gy = 1.f - ay.f;
    const float top = __builtin_fmaf(ax.f, (float)ld(ay.i0, ax.i1, ch), gx * (float)ld(ay.i0, ax.i0, ch));
    const float bot = __builtin_fmaf(ax.f, (float)ld(ay.i1, ax.i1, ch), gx * (float)ld(ay.i1, ax.i0, ch));
    return (E)__builtin_fmaf(ay.f, bot, gy * top);
  };
  constexpr unsigned V = 16 / sizeof(E);
  if (flags & GEOM_VSTORE) {  // a thread's V elements share a row
    typedef E EV __attribute__((ext_vector_type(V)));
    for (unsigned e0 = lo + threadIdx.x * V; e0 < hi; e0 += GEOM_THREADS * V) {
      const unsigned i = e0 / RC, re = e0 - i * RC;
      unsigned j = re / uc, ch = re - j * uc;
      GeomAxis ax, ay;
      geom_taps(g, (int)i, (int)j, ax, ay);
      EV v;
#pragma unroll
      for (unsigned u = 0; u < V; ++u) {
        v[u] = sample(ax, ay, ch);
        if (++ch == uc) {
          ch = 0;
          ++j;
          if (u + 1 < V) geom_taps(g, (int)i, (int)j, ax, ay);
        }
      }
      *reinterpret_cast<u32x4*>(yi + e0) = __builtin_bit_cast(u32x4, v);
    }
  } else {
    for (unsigned e = lo + threadIdx.x; e < hi; e += GEOM_THREADS) {
      const unsigned i = e / RC, re = e - i * RC, j = re / uc;
      GeomAxis ax, ay;
      geom_taps(g, (int)i, (int)j, ax, ay);
      yi[e] = sample(ax, ay, re - j * uc);
    }
  }
}

// gx = W^T g over N images under the matrices of params (and, GATED, the recorded gate masks): see the head
// of the file. bpi workgroups per image, each `chunk` input pixels of it (bpi = 1 whenever g is staged).
template <typename E, bool GATED>
__global__ __launch_bounds__(GEOM_THREADS) void d_geom_bwd_kernel(const E* __restrict__ gy, E* __restrict__ gx,
                                                                  const float* __restrict__ params,
                                                                  const int* __restrict__ gates, int S, int C,
                                                                  int policy, unsigned bpi, unsigned chunk,
                                                                  unsigned pitch, int flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char geom_lds[];
  __shared__ float sm[4];
  const unsigned n = blockIdx.x / bpi, part = blockIdx.x - n * bpi;
  if (threadIdx.x == 0) {
    const float* row = params + (size_t)GEOM_PARAMS * n;
    const int eff = GATED ? policy & gates[n] : policy;
    sm[0] = eff ? row[0] : 1.f; sm[1] = eff ? row[1] : 0.f; sm[2] = eff ? row[2] : 0.f; sm[3] = eff ? row[3] : 1.f;
  }
  __syncthreads();
  const float m[4] = {sm[0], sm[1], sm[2], sm[3]};
  const unsigned RC = (unsigned)(S * C), HWC = (unsigned)S * RC, uc = (unsigned)C;
  const E* gi = gy + (size_t)n * HWC;
  E* oi = gx + (size_t)n * HWC;
  if (geom_kind(m, S) == GEOM_COPY) {
    geom_copy(gi, oi, part * chunk * uc, min(HWC, (part + 1) * chunk * uc), flags & GEOM_VCOPY);
    return;
  }
  E* lds = reinterpret_cast<E*>(geom_lds);
  if (pitch) geom_stage(gi, lds, (unsigned)S, RC, pitch, flags & GEOM_VSTAGE);
  const GeomMap g = geom_map(m, S);
  auto ld = [&](int yy, int xx, unsigned ch) -> float {
    return (float)(pitch ? lds[(unsigned)yy * pitch + (unsigned)xx * uc + ch]
                         : gi[((unsigned)yy * (unsigned)S + (unsigned)xx) * uc + ch]);
  };
  // M^-1, of any invertible matrix
  const float det = m[0] * m[3] - m[1] * m[2];
  const float i00 = m[3] / det, i01 = -m[1] / det, i10 = -m[2] / det, i11 = m[0] / det;
  // half-width of the box around an image, in source pixels: 1 (the taps' reach) plus what fp32 can lose on
  // coordinates of magnitude 3 S; and the output-pixel reach of that box along each axis
  const float h = 1.001f + 2e-5f * (float)S;
  const float eu = (fabsf(i00) + fabsf(i01)) * h, ev = (fabsf(i10) + fabsf(i11)) * h;
  // a matrix no draw gives (singular, non-finite, a zoom-in beyond 1 / 64) transposes to +0: its candidate
  // boxes would cover the image
  const bool sane = eu + ev < 128.f;
  // the sample's source box per axis, widened by h, and the periods it reaches
  const float rx = g.c * (fabsf(m[0]) + fabsf(m[1])), ry = g.c * (fabsf(m[2]) + fabsf(m[3]));
  const float xlo = g.c - rx - h, xhi = g.c + rx + h, ylo = g.c - ry - h, yhi = g.c + ry + h;
  const float P = (float)GEOM_MAX_PERIODS;
  const int kx0 = (int)fminf(fmaxf(floorf(xlo * g.invT), -P), P), kx1 = (int)fminf(fmaxf(floorf(xhi * g.invT), -P), P);
  const int ky0 = (int)fminf(fmaxf(floorf(ylo * g.invT), -P), P), ky1 = (int)fminf(fmaxf(floorf(yhi * g.invT), -P), P);
  const float top = g.lim;
  const unsigned plo = part * chunk, phi = min((unsigned)(S * S), plo + chunk);
  for (unsigned pix = plo + threadIdx.x; pix < phi; pix += GEOM_THREADS) {
    const int p = (int)(pix / (unsigned)S), q = (int)(pix - (unsigned)p * (unsigned)S);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ly = 2 * ky0; sane && ly <= 2 * ky1 + 1; ++ly) {  // images of row p: period ly >> 1, mirrored if odd
      const float Y = (ly & 1) ? (float)((ly >> 1) + 1) * g.T - (float)p : (float)(ly >> 1) * g.T + (float)p;
      if (!(Y >= ylo && Y <= yhi)) continue;
      for (int lx = 2 * kx0; lx <= 2 * kx1 + 1; ++lx) {
        const float X = (lx & 1) ? (float)((lx >> 1) + 1) * g.T - (float)q : (float)(lx >> 1) * g.T + (float)q;
        if (!(X >= xlo && X <= xhi)) continue;
        const float dx = X - g.c, dy = Y - g.c;
        const float uj = __builtin_fmaf(i00, dx, i01 * dy) + g.c, vi = __builtin_fmaf(i10, dx, i11 * dy) + g.c;
        const float jl = fmaxf(ceilf(uj - eu), 0.f), jh = fminf(floorf(uj + eu), top);
        const float il = fmaxf(ceilf(vi - ev), 0.f), ih = fminf(floorf(vi + ev), top);
        if (!(jl <= jh && il <= ih)) continue;
        const int j0 = (int)jl, j1 = (int)jh, i0 = (int)il, i1 = (int)ih;
        for (int i = i0; i <= i1; ++i) {
          for (int j = j0; j <= j1; ++j) {
            GeomAxis ax, ay;
            geom_taps(g, i, j, ax, ay);
            if (ax.label != lx || ay.label != ly) continue;
            const float wx = (ax.i0 == q ? 1.f - ax.f : 0.f) + (ax.i1 == q ? ax.f : 0.f);
            const float wy = (ay.i0 == p ? 1.f - ay.f : 0.f) + (ay.i1 == p ? ay.f : 0.f);
            const float w = wy * wx;
            if (w != 0.f) {
              for (unsigned ch = 0; ch < uc; ++ch) acc[ch] = __builtin_fmaf(w, ld(i, j, ch), acc[ch]);
            }
          }
        }
      }
    }
    for (unsigned ch = 0; ch < uc; ++ch) oi[pix * uc + ch] = (E)acc[ch];
  }
}

}  // namespace dcg

using namespace dcg;

namespace {

// how a launch lays an image out: staged in LDS at `pitch` elements per row by one workgroup, or (pitch 0)
// read from global memory by bpi workgroups of `chunk` units (elements forward, pixels transposed) each
struct GeomPlan {
  unsigned pitch, bpi, chunk;
  size_t lds;
  int flags;
};

GeomPlan geom_plan(const void* x, const void* y, int N, int S, int C, bool pixels) {
  GeomPlan p;
  const size_t es = sizeof(elem_t), rowb = (size_t)S * C * es, hwc = (size_t)S * S * C;
  const size_t pitch_dw = ((rowb + 3) / 4) | 1;  // an odd number of dwords
  const size_t units = pixels ? (size_t)S * S : hwc, V = pixels ? 1 : 16 / es;
  p.lds = pitch_dw * 4 * (size_t)S;
  if (p.lds <= GEOM_LDS_BYTES) {
    p.pitch = (unsigned)(pitch_dw * 4 / es);
    p.bpi = 1;
    p.chunk = (unsigned)units;
  } else {
    p.pitch = 0;
    p.lds = 0;
    p.chunk = (unsigned)(GEOM_THREADS * GEOM_ITERS * V);
    p.bpi = (unsigned)((units + p.chunk - 1) / p.chunk);
  }
  const bool ax = ((uintptr_t)x & 15) == 0, ay = ((uintptr_t)y & 15) == 0;
  p.flags = (rowb % 16 == 0 && ay ? GEOM_VSTORE : 0) | (rowb % 16 == 0 && ax ? GEOM_VSTAGE : 0) |
            ((hwc * es) % 16 == 0 && (p.chunk * (pixels ? (size_t)C : 1) * es) % 16 == 0 && ax && ay ? GEOM_VCOPY : 0);
  if ((size_t)p.bpi * (size_t)N > 0x7FFFFFFFull) p.bpi = 0;
  return p;
}

// more than 64 KB of dynamic LDS has to be asked for once per kernel instance (as swd.hip and narrow.hip do)
template <typename K>
int geom_lds_attr(K kernel, bool* done) {
  if (*done) return 0;
  const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)GEOM_LDS_BYTES);
  if (e != hipSuccess) return (int)e;
  *done = true;
  return 0;
}

template <int MODE, bool GATED>
int geom_launch(const elem_t* x, elem_t* y, float* params, int N, int S, int C, int policy, const GeomPlan& p,
                uint64_t seed, const unsigned long long* step, int* gates, const int* ada, hipStream_t s) {
  static bool attr = false;
  const auto kernel = d_geom_kernel<elem_t, MODE, GATED>;
  if (const int rc = geom_lds_attr(kernel, &attr)) return rc;
  hipLaunchKernelGGL(kernel, dim3(p.bpi * (unsigned)N), dim3(GEOM_THREADS), p.lds, s, x, y, params, S, C, policy,
                     p.bpi, p.chunk, p.pitch, p.flags, seed, step, gates, ada);
  return (int)hipGetLastError();
}

template <bool GATED>
int geom_bwd_launch(const elem_t* g, elem_t* gx, const float* params, const int* gates, int N, int S, int C,
                    int policy, const GeomPlan& p, hipStream_t s) {
  static bool attr = false;
  const auto kernel = d_geom_bwd_kernel<elem_t, GATED>;
  if (const int rc = geom_lds_attr(kernel, &attr)) return rc;
  hipLaunchKernelGGL(kernel, dim3(p.bpi * (unsigned)N), dim3(GEOM_THREADS), p.lds, s, g, gx, params, gates, S, C,
                     policy, p.bpi, p.chunk, p.pitch, p.flags);
  return (int)hipGetLastError();
}

// as misc.hip's d_stage_args_ok
bool geom_args_ok(const void* x, const void* y, const void* params, int N, int S, int C, int policy) {
  if (!x || !y || !params || x == y) return false;
  return !(N < 1 || S < 1 || S > AUG_MAX_SIZE || C < 1 || C > 4 || policy < 1 || policy > GEOM_ALL);
}

}  // namespace

extern "C" int DCG_API(dcg_d_geom_bwd)(const elem_t* g, elem_t* gx, const float* params, const int* gates, int N,
                                       int S, int C, int policy, hipStream_t s) {
  if (!geom_args_ok(g, gx, params, N, S, C, policy)) return -2;
  const GeomPlan p = geom_plan(g, gx, N, S, C, true);
  if (!p.bpi) return -2;
  return gates ? geom_bwd_launch<true>(g, gx, params, gates, N, S, C, policy, p, s)
               : geom_bwd_launch<false>(g, gx, params, gates, N, S, C, policy, p, s);
}

extern "C" int DCG_API(dcg_d_geom)(const elem_t* x, elem_t* y, float* params, int N, int S, int C, int policy,
                                   int mode, uint64_t seed, const unsigned long long* step, int* gates,
                                   const int* ada, hipStream_t s) {
  if (!geom_args_ok(x, y, params, N, S, C, policy) || mode < 0 || mode > 2 || (mode == 0 && !step)) return -2;
  if (gates ? (mode == 0 && !ada) : ada != nullptr) return -2;
  if (mode == 2) return DCG_API(dcg_d_geom_bwd)(x, y, params, gates, N, S, C, policy, s);
  const GeomPlan p = geom_plan(x, y, N, S, C, false);
  if (!p.bpi) return -2;
  if (mode == 0)
    return gates ? geom_launch<0, true>(x, y, params, N, S, C, policy, p, seed, step, gates, ada, s)
                 : geom_launch<0, false>(x, y, params, N, S, C, policy, p, seed, step, gates, ada, s);
  return gates ? geom_launch<1, true>(x, y, params, N, S, C, policy, p, seed, step, gates, ada, s)
               : geom_launch<1, false>(x, y, params, N, S, C, policy, p, seed, step, gates, ada, s);
}
