// dcg-variants: bf16
// Nearest-neighbour search between two sets of feature rows: the hot path of the leave-one-out 1-NN two-sample
// test (Lopez-Paz & Oquab 2017), of the nearest-training-image distance and of the k-NN manifold estimates
// (precision / recall, Kynkaanniemi et al. 2019; density / coverage, Naeem et al. 2020). fp32 throughout,
// whatever the engine's element type (one build, nn.h): bf16's 2^-8 is the size of the gaps being compared.
// It runs beside the training step, never inside it.
//
// X [Mx][K], Y [My][K] are pyramid levels (swd_down's output, or the images) flattened per image:
//   nn_features  F [M][Kp] = x - mu, zero-filled from K to Kp = K rounded up to 16, and norm [M] = |F_i|^2. mu is
//                the real set's per-feature mean, from fp64 partial sums per 64 rows added in index order (no
//                atomics). Centring changes no distance; it shrinks the norms and with them the cancellation
//                in d = |x|^2 + |y|^2 - 2 x.y. A workgroup owns 4 rows; a row's norm is summed by wave
//                shuffles, then through LDS in wave order: a fixed order
//   nn_top1      G = X Y^T on v_mfma_f32_16x16x4_f32 with the selection fused into its epilogue. A workgroup of
//                256 threads owns 128 rows of X and walks the 128-column tiles of its chunk of Y (grid.y
//                chunks, so that a small My still fills the GPU). Both operand tiles stream through LDS in k
//                steps of 32, double-buffered: the 16-byte global loads of step t + 1 are issued into
//                registers before the MFMAs of step t and stored to the other buffer after them, one barrier
//                per step. LDS rows sit 36 floats apart: the fragment read of lane (fr, fq) is the 16 bytes at
//                row fr, float 4 fq, and 36 fr mod 64 takes 16 distinct multiples of 4 -- the 16 lanes of a
//                quarter-wave cover all 64 banks once (and any 8 consecutive rows all of 32). Each wave owns
//                64 x 64 of the tile: 4 A and 4 B fragments feed 64 MFMAs per 16 k. Per tile the epilogue forms
//                d = nx_i + ny_j - 2 g, masks the diagonal (loo) and the columns past My, packs
//                (topk's monotone key of d) << 32 | j and folds it into the lane's running minimum of its 16
//                rows: one 64-bit min is "smallest d, then smallest j". At the end of the chunk the minima
//                are reduced across the 16 lanes of a column group by shuffles and across the two column
//                waves through LDS, and go to part [chunk][row]. No atomics, no dependence between workgroups
//   nn_merge     idx [Mx] = the column of the minimum of part over the chunks, in chunk order
//   nn_refine    the Gram form is only good enough to choose. The winner's distance is recomputed from the
//                uncentred rows, (x_k - y_k)^2 in fp32 summed in fp64: one wave per row, every lane its k in
//                index order, then a shuffle tree -- a fixed order; a bitwise duplicate reports exactly 0
//   nn_topk      the same GEMM (nn_gemm_tiles: one main loop for nn_topk and nn_count) with a k-smallest selection,
//                k <= 16, in its epilogue. The packed keys of one row are distinct, so "the k smallest keys of a
//                set" does not depend on the order they are met in. A row's list lies across the 16 lanes that
//                share the row (all fr of one fq): lane fr < k holds the fr-th smallest so far, in the registers
//                that hold nn_top1's minima; lane k - 1 holds the row's threshold. Per tile a lane tests its 4 new
//                keys of the row against the threshold (one broadcast shuffle); only if some lane of the wave has
//                one below it does the wave re-select: k rounds of "smallest key above the last one extracted"
//                over the group's 16 x (4 new + 1 listed) keys, each round a 4-step shuffle minimum, round p
//                landing in lane p. Once the lists have filled a row triggers about k ln(My) times in all. The
//                two column waves' lists meet once per chunk in LDS (the operand tiles' space) and merge by two
//                pointers into part [chunk][row][k], NN_NONE where the chunk has fewer than k columns
//   nn_merge_k   idx [Mx][k] = the columns of the k smallest keys of part over the chunks, ascending, -1 where
//                there is none: one wave per row, k rounds of the same extraction over the row's splits * k keys
//   nn_radius    nn_refine for all k candidates of a row, one wave per candidate, and rad = the fp32 value of
//                the largest: the squared radius of the row's k-NN ball
//   nn_count     the same GEMM with an integer epilogue: cnt [row] = #{col : nx + ny - 2 g <= rad [col]}, 16
//                counters per lane where nn_top1 holds its minima, summed across the 16 lanes by shuffles, across
//                the two column waves through LDS and across the chunks in chunk order. Integers only
//   nn_mmd_bw    the kernel MMD's bandwidth h = 2 / (n - 1) * sum_i norm_i of the centred reals, fp64 in a fixed order,
//                and c = log2(e) / (4 h), left on the device for nn_mmd
//   nn_mmd       the Gaussian-mixture kernel summed over the upper triangle of the Gram of Z = [X; Y]: one workgroup
//                per 128 x 128 tile (I, J), I <= J, in one launch, so the symmetric blocks cost half a rectangle's
//                MFMAs. The same main loop on one tile, every loader row from the matrix that holds it. Epilogue:
//                d = max(nx + ny - 2 g, 0), e1 = exp2(-d c), the other four Gaussians by squaring, three fp32
//                partials per lane by class (A, A), (A, B), (B, B) over row < col, then fp64: shuffles, the four
//                waves through LDS in order, part [pair][3]. No atomics; bitwise reproducible
//   nn_mmd_final the pairs' sums added in a fixed order, the three means and mmd2 = k_rr + k_ff - 2 k_rf
// The Frechet distance of the two sets' Gaussians, FD = |d|^2 + tr S_A + tr S_B - 2 tr (S_A S_B)^(1/2), through its dual
// (Mathiasen & Hvilshoj 2020): tr (S_A S_B)^(1/2) = ||C||_*, C = Xc Yc^T / (n - 1) [n][n], and ||C||_* = tr(U^T C) for the
// polar factor U of C, which the Newton-Schulz iteration X <- 1.5 X - 0.5 (X X^T) X reaches by GEMMs alone. Square
// matrices [n][ld], ld = n rounded up to 16, columns n..ld-1 zero, so that a row is a k range for the loaders above:
//   nn_fd_nt     out = scale A B^T, the main loop above with a store epilogue. As the cross-Gram C' = F_A F_B^T / (n - 1)
//                over all tiles; as P = X X^T over the tiles (I, J), I <= J, of the upper triangle (nn_mmd's pair
//                index), an off-diagonal tile also stored transposed: the four rows 4 fq + r of a C fragment are four
//                consecutive columns of the mirror image, one 16-byte store
//   nn_fd_rows .. nn_fd_x0  the scale. F_B is centred by the real mean, F_B = Yc + 1 d^T, and F_A's columns sum to zero,
//                so C = C' - rowmean(C'): per row the fp64 mean and the sum of |c - mean| (one wave per row, every lane
//                its columns in index order, a shuffle tree), per column the same sum through fp64 partials per 64
//                rows, alpha = sqrt(max row sum * max column sum) >= sigma_max (a maximum has no order), and one
//                pass that leaves C centred in place and X_0 = C / alpha: singular values in [0, 1]
//   nn_fd_step   X' = 1.5 X - 0.5 P X. P's rows are the row-major operand as above; X is the k-major one, element (k, j),
//                read from its rows with no transposed copy in memory: per stage of 32 k a thread takes 16-byte loads
//                along j and stores them as they are into a tile [32 k][TILE + 4]. The B fragment of lane (fr, fq) for
//                MFMA e is the float at row kk + 4 fq + e, column 16 j + fr: with a pitch of TILE + 4 = 132 (or 68)
//                floats, 4 fq pitch mod 64 = 16 fq, so the bank is 16 fq + fr + a constant -- the wave's 64 lanes read
//                64 different banks (and either half-wave 32 different ones mod 32). The 16-byte stores of 16
//                consecutive lanes cover 64 consecutive floats of one k row: every bank once. A transpose in the
//                stash would buy 16-byte fragment reads at the price of 4-way conflicts on every store; [k][col] with
//                this pitch has none on either side. The 1.5 X term comes from the output tile's own rows of X in the
//                epilogue. Two X buffers alternate, so the last two iterates are both there at the end
//   nn_fd_trace  part [4 rows] = sum X_ij C_ij in fp64: a wave per row in index order, the four waves in order
//   nn_fd_final  v = tr(X^T C) of the last two iterates from nn_fd_trace's parts in a fixed order, |d|^2 from the fp64
//                column sums of F_B (nn_fd_mean: nn_mean_part on F_B), tr S_B from its norms:
//                out = {fd, mean2, tr_a, tr_b, nuc = v_k, tail = v_k - v_{k-1}, alpha, iters}
// Tiles are 128 x 128 as above or, below 2048 rows, 64 x 64 (a wave owns 32 x 32): at n = 1024 that is 136 workgroups
// for P and 256 for the step instead of 36 and 64. No atomics; every dependency between workgroups is a launch boundary.
// Every index into a feature matrix is 64-bit: n Kp passes 2^31 at 128x128x3.
#include "common.h"
#include "nn.h"

namespace dcg {

// ---------------------------------------------------------------- mean and features
// thread k of row block b: the fp64 sum of x[r][k] over the block's rows, in index order
__global__ __launch_bounds__(256) void nn_mean_part_kernel(const float* __restrict__ x, int n, int K,
                                                           double* __restrict__ part) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const int r0 = blockIdx.y * NN_MEAN_ROWS, r1 = min(n, r0 + NN_MEAN_ROWS);
  double s = 0.0;
  for (int r = r0; r < r1; ++r) s += (double)x[(size_t)r * K + k];
  part[(size_t)blockIdx.y * K + k] = s;
}

__global__ __launch_bounds__(256) void nn_mean_final_kernel(const double* __restrict__ part, int blocks, int K,
                                                            double count, float* __restrict__ mu) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += part[(size_t)b * K + k];
  mu[k] = (float)(s / count);
}

__global__ __launch_bounds__(256) void nn_features_kernel(const float* __restrict__ x, const float* __restrict__ mu,
                                                          float* __restrict__ F, float* __restrict__ norm, int n, int K,
                                                          int Kp) {
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int q = 0; q < NN_FEAT_ROWS; ++q) {
    const int r = blockIdx.x * NN_FEAT_ROWS + q;
    if (r >= n) break;  // (the same for every thread of the workgroup)
    const float* src = x + (size_t)r * K;
    float* dst = F + (size_t)r * Kp;
    float s = 0.f;
    for (int k = tid; k < Kp; k += 256) {
      float v = 0.f;
      if (k < K) v = mu ? src[k] - mu[k] : src[k];
      dst[k] = v;
      s = __builtin_fmaf(v, v, s);
    }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0) norm[r] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
  }
}

// ---------------------------------------------------------------- the distance GEMM with its epilogues
// topk's key (misc.hip topk_key): uint32, monotone in x, -0 < +0
__device__ __forceinline__ uint32_t nn_key(float x) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
constexpr unsigned long long NN_NONE = ~0ull;  // no candidate: above every (key, column)
constexpr int NN_TILE_F = NN_TILE * NN_PITCH;  // floats of one operand tile in LDS
constexpr size_t NN_GEMM_LDS = (size_t)4 * NN_TILE_F * sizeof(float);
constexpr size_t NN_TOP1_LDS = NN_GEMM_LDS + (size_t)2 * NN_TILE * sizeof(unsigned long long);
constexpr int NN_LIST_PITCH = NN_MAX_KNN + 1;  // 64-bit words between two rows' lists in LDS: odd, so rows spread over banks
static_assert((size_t)2 * NN_TILE * NN_LIST_PITCH * sizeof(unsigned long long) <= NN_GEMM_LDS, "nn: lists fit the tiles");

__device__ __forceinline__ unsigned long long nn_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// nn_top1's main loop for nn_topk and nn_count (nn_top1_kernel keeps its own copy below: built on this function it
// takes 250 VGPRs for its 248): the workgroup's 128 rows from m0 against the column tiles [t0, t1) of Y. Whenever a tile's sums are complete, epi(first column of the wave's 64, acc) consumes and clears
// them: C fragment acc[i][j][r] = row wr * 64 + i * 16 + 4 fq + r, column j * 16 + fr. The last epilogue is followed
// by a barrier, after which the operand tiles in LDS are free
template <class Epi>
__device__ __forceinline__ void nn_gemm_tiles(const float* __restrict__ X, const float* __restrict__ Y, float* lds, int Mx,
                                              int My, int Kp, int m0, int t0, int t1, Epi epi) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int nk = (Kp + NN_BK - 1) / NN_BK, steps = (t1 - t0) * nk;
  const int lr = tid >> 3, lq = tid & 7;  // the loader's rows lr + 32 p, its 16-byte word lq of the 32 k
  const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 sx[4], sy[4];

  auto fetch = [&](int it) {  // rows past the ends and k past Kp read as zeros
    const int ct = t0 + it / nk, k0 = (it % nk) * NN_BK + 4 * lq;
    const bool kok = k0 < Kp;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int rx = m0 + lr + 32 * p, ry = ct * NN_TILE + lr + 32 * p;
      sx[p] = (kok && rx < Mx) ? *reinterpret_cast<const f32x4*>(X + (size_t)rx * Kp + k0) : zero;
      sy[p] = (kok && ry < My) ? *reinterpret_cast<const f32x4*>(Y + (size_t)ry * Kp + k0) : zero;
    }
  };
  auto stash = [&](int buf) {
    float* bx = lds + buf * 2 * NN_TILE_F + lr * NN_PITCH + 4 * lq;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      *reinterpret_cast<f32x4*>(bx + 32 * p * NN_PITCH) = sx[p];
      *reinterpret_cast<f32x4*>(bx + NN_TILE_F + 32 * p * NN_PITCH) = sy[p];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = zero;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int it = 0; it < steps; ++it) {
    const int buf = it & 1;
    const bool more = it + 1 < steps;
    if (more) fetch(it + 1);
    const float* bx = lds + buf * 2 * NN_TILE_F + (wr * 64 + fr) * NN_PITCH + 4 * fq;
    const float* by = lds + buf * 2 * NN_TILE_F + NN_TILE_F + (wc * 64 + fr) * NN_PITCH + 4 * fq;
#pragma unroll
    for (int kk = 0; kk < NN_BK; kk += 16) {  // lane group fq supplies k = kk + 4 fq + e to MFMA e, for A and B alike
      f32x4 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4*>(bx + i * 16 * NN_PITCH + kk);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const f32x4*>(by + j * 16 * NN_PITCH + kk);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
    }
    if (more) stash(buf ^ 1);  // (last read in step it - 1, before that step's barrier)
    if ((it + 1) % nk == 0) epi((t0 + it / nk) * NN_TILE + wc * 64, acc);  // the tile is complete
    __syncthreads();
  }
}

// two waves per SIMD (248 VGPRs, no scratch): two workgroups per CU, the second one's MFMAs cover this one's barrier
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void nn_top1_kernel(const float* __restrict__ X, const float* __restrict__ nx, const float* __restrict__ Y,
                    const float* __restrict__ ny, unsigned long long* __restrict__ part, int Mx, int My, int Kp, int loo,
                    int nct) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [2 buffers][X tile, Y tile][128][36], then red
  unsigned long long* red = reinterpret_cast<unsigned long long*>(lds + 4 * NN_TILE_F);  // [2 column waves][128]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int m0 = blockIdx.x * NN_TILE, chunk = blockIdx.y, splits = gridDim.y;
  const int t0 = (int)((long long)chunk * nct / splits), t1 = (int)((long long)(chunk + 1) * nct / splits);
  const int nk = (Kp + NN_BK - 1) / NN_BK, steps = (t1 - t0) * nk;
  const int lr = tid >> 3, lq = tid & 7;  // the loader's rows lr + 32 p, its 16-byte word lq of the 32 k
  const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 sx[4], sy[4];

  auto fetch = [&](int it) {  // rows past the ends and k past Kp read as zeros
    const int ct = t0 + it / nk, k0 = (it % nk) * NN_BK + 4 * lq;
    const bool kok = k0 < Kp;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int rx = m0 + lr + 32 * p, ry = ct * NN_TILE + lr + 32 * p;
      sx[p] = (kok && rx < Mx) ? *reinterpret_cast<const f32x4*>(X + (size_t)rx * Kp + k0) : zero;
      sy[p] = (kok && ry < My) ? *reinterpret_cast<const f32x4*>(Y + (size_t)ry * Kp + k0) : zero;
    }
  };
  auto stash = [&](int buf) {
    float* bx = lds + buf * 2 * NN_TILE_F + lr * NN_PITCH + 4 * lq;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      *reinterpret_cast<f32x4*>(bx + 32 * p * NN_PITCH) = sx[p];
      *reinterpret_cast<f32x4*>(bx + NN_TILE_F + 32 * p * NN_PITCH) = sy[p];
    }
  };

  float nxr[4][4];               // |x|^2 of the lane's rows: wr * 64 + i * 16 + 4 fq + r
  unsigned long long best[4][4];
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wr * 64 + i * 16 + 4 * fq + r;
      nxr[i][r] = row < Mx ? nx[row] : 0.f;
      best[i][r] = NN_NONE;
    }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = zero;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int it = 0; it < steps; ++it) {
    const int buf = it & 1;
    const bool more = it + 1 < steps;
    if (more) fetch(it + 1);
    const float* bx = lds + buf * 2 * NN_TILE_F + (wr * 64 + fr) * NN_PITCH + 4 * fq;
    const float* by = lds + buf * 2 * NN_TILE_F + NN_TILE_F + (wc * 64 + fr) * NN_PITCH + 4 * fq;
#pragma unroll
    for (int kk = 0; kk < NN_BK; kk += 16) {  // lane group fq supplies k = kk + 4 fq + e to MFMA e, for A and B alike
      f32x4 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4*>(bx + i * 16 * NN_PITCH + kk);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const f32x4*>(by + j * 16 * NN_PITCH + kk);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
    }
    if (more) stash(buf ^ 1);  // (last read in step it - 1, before that step's barrier)
    if ((it + 1) % nk == 0) {  // the tile is complete. C fragment: rows 4 fq + r of column fr
      const int cbase = (t0 + it / nk) * NN_TILE + wc * 64;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = cbase + j * 16 + fr;
        const bool cok = col < My;
        const float nyv = cok ? ny[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = m0 + wr * 64 + i * 16 + 4 * fq + r;
            const float d = __builtin_fmaf(-2.f, acc[i][j][r], nxr[i][r] + nyv);
            unsigned long long key = ((unsigned long long)nn_key(d) << 32) | (unsigned)col;
            if (!cok || (loo && col == row)) key = NN_NONE;
            best[i][r] = nn_min(best[i][r], key);
          }
        acc[0][j] = zero; acc[1][j] = zero; acc[2][j] = zero; acc[3][j] = zero;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      unsigned long long v = best[i][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) v = nn_min(v, __shfl_xor(v, o, 64));
      if (fr == 0) red[wc * NN_TILE + wr * 64 + i * 16 + 4 * fq + r] = v;
    }
  __syncthreads();
  if (tid < NN_TILE && m0 + tid < Mx) part[(size_t)chunk * Mx + m0 + tid] = nn_min(red[tid], red[NN_TILE + tid]);
}

__global__ __launch_bounds__(256) void nn_merge_kernel(const unsigned long long* __restrict__ part, int* __restrict__ idx,
                                                       int Mx, int splits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Mx) return;
  unsigned long long b = part[i];
  for (int c = 1; c < splits; ++c) b = nn_min(b, part[(size_t)c * Mx + i]);
  idx[i] = (int)(unsigned)b;  // (-1: no candidate)
}

// ---------------------------------------------------------------- the k smallest per row
// list[i][r] of lane (fr, fq): the fr-th smallest key so far of row wr * 64 + i * 16 + 4 fq + r (NN_NONE from lane k on)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void nn_topk_kernel(const float* __restrict__ X, const float* __restrict__ nx, const float* __restrict__ Y,
                    const float* __restrict__ ny, unsigned long long* __restrict__ part, int Mx, int My, int Kp, int loo,
                    int nct, int k) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [2 buffers][X tile, Y tile][128][36]; at the end the lists
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int m0 = blockIdx.x * NN_TILE, chunk = blockIdx.y, splits = gridDim.y;
  const int t0 = (int)((long long)chunk * nct / splits), t1 = (int)((long long)(chunk + 1) * nct / splits);
  const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};

  float nxr[4][4];
  unsigned long long list[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wr * 64 + i * 16 + 4 * fq + r;
      nxr[i][r] = row < Mx ? nx[row] : 0.f;
      list[i][r] = NN_NONE;
    }

  nn_gemm_tiles(X, Y, lds, Mx, My, Kp, m0, t0, t1, [&](int cbase, f32x4 (&acc)[4][4]) {
    float nyv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) nyv[j] = cbase + j * 16 + fr < My ? ny[cbase + j * 16 + fr] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wr * 64 + i * 16 + 4 * fq + r;
        unsigned long long c[4];  // the lane's new keys of this row
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int col = cbase + j * 16 + fr;
          const float d = __builtin_fmaf(-2.f, acc[i][j][r], nxr[i][r] + nyv[j]);
          c[j] = ((unsigned long long)nn_key(d) << 32) | (unsigned)col;
          if (col >= My || (loo && col == row)) c[j] = NN_NONE;
        }
        const unsigned long long thr = __shfl(list[i][r], k - 1, 16);
        const unsigned long long low = nn_min(nn_min(c[0], c[1]), nn_min(c[2], c[3]));
        if (__any(low < thr)) {  // (wave-uniform) some row of the wave's four groups gains a key
          unsigned long long prev = 0, mine = NN_NONE;
          for (int p = 0; p < k; ++p) {  // round p: the smallest key above round p - 1's, into lane p
            unsigned long long m = (p == 0 || list[i][r] > prev) ? list[i][r] : NN_NONE;
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (p == 0 || c[j] > prev) m = nn_min(m, c[j]);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) m = nn_min(m, __shfl_xor(m, o, 64));
            if (fr == p) mine = m;
            prev = m;  // (NN_NONE once the keys are used up: nothing lies above it)
          }
          list[i][r] = mine;
        }
      }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = zero;
  });

  unsigned long long* red = reinterpret_cast<unsigned long long*>(lds);  // [2 column waves][128][NN_LIST_PITCH]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      red[(size_t)(wc * NN_TILE + wr * 64 + i * 16 + 4 * fq + r) * NN_LIST_PITCH + fr] = list[i][r];
  __syncthreads();
  if (tid < NN_TILE && m0 + tid < Mx) {  // two ascending lists -> the k smallest of both
    const unsigned long long* a = red + (size_t)tid * NN_LIST_PITCH;
    const unsigned long long* b = red + (size_t)(NN_TILE + tid) * NN_LIST_PITCH;
    unsigned long long* dst = part + ((size_t)chunk * Mx + m0 + tid) * k;
    int ia = 0, ib = 0;
    for (int p = 0; p < k; ++p) {  // (ia + ib = p < k <= 16: inside the lists)
      const unsigned long long va = a[ia], vb = b[ib];
      const bool fa = va <= vb;
      dst[p] = fa ? va : vb;
      ia += fa ? 1 : 0;
      ib += fa ? 0 : 1;
    }
  }
}

// one wave per row: round p takes the smallest of the row's splits * k keys above round p - 1's
__global__ __launch_bounds__(256) void nn_merge_k_kernel(const unsigned long long* __restrict__ part, int* __restrict__ idx,
                                                         int Mx, int splits, int k) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Mx) return;
  unsigned long long prev = 0;
  for (int p = 0; p < k; ++p) {
    unsigned long long m = NN_NONE;
    for (int c = 0; c < splits; ++c) {
      const unsigned long long* src = part + ((size_t)c * Mx + row) * k;
      for (int q = lane; q < k; q += 64) {
        const unsigned long long e = src[q];
        if (p == 0 || e > prev) m = nn_min(m, e);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = nn_min(m, __shfl_xor(m, o, 64));
    if (lane == 0) idx[(size_t)row * k + p] = (int)(unsigned)m;  // (-1: no candidate)
    prev = m;
  }
}

// ---------------------------------------------------------------- the winner's distance, recomputed
// sum_k (x_k - y_k)^2 over the wave: fp32 differences and squares, every lane its k in index order in fp64, a shuffle tree
__device__ __forceinline__ double nn_wave_dist(const float* __restrict__ x, const float* __restrict__ y, int K, int lane) {
  double s = 0.0;
  for (int k = lane; k < K; k += 64) {
    const float df = x[k] - y[k];
    const float sq = df * df;
    s += (double)sq;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

__global__ __launch_bounds__(256) void nn_refine_kernel(const float* __restrict__ x0, const float* __restrict__ y0,
                                                        const int* __restrict__ idx, double* __restrict__ dist, int Mx,
                                                        int My, int K) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Mx) return;
  const int j = idx[row];
  double s = __builtin_inf();
  if (j >= 0 && j < My) s = nn_wave_dist(x0 + (size_t)row * K, y0 + (size_t)j * K, K, lane);
  if (lane == 0) dist[row] = s;
}

// a workgroup per row, a wave per candidate (p = wave, wave + 4, ...); rad = the largest of the row's k distances
__global__ __launch_bounds__(256) void nn_radius_kernel(const float* __restrict__ x0, const float* __restrict__ y0,
                                                        const int* __restrict__ idx, double* __restrict__ dist,
                                                        float* __restrict__ rad, int Mx, int My, int K, int k) {
  __shared__ double top[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = blockIdx.x;
  double most = 0.0;
  for (int p = wave; p < k; p += 4) {
    const int j = idx[(size_t)row * k + p];
    double s = __builtin_inf();
    if (j >= 0 && j < My) s = nn_wave_dist(x0 + (size_t)row * K, y0 + (size_t)j * K, K, lane);
    if (lane == 0) dist[(size_t)row * k + p] = s;
    most = s > most ? s : most;
  }
  if (lane == 0) top[wave] = most;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) most = top[w] > most ? top[w] : most;
    rad[row] = (float)most;
  }
}

// ---------------------------------------------------------------- the balls a row falls into
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void nn_count_kernel(const float* __restrict__ X, const float* __restrict__ nx, const float* __restrict__ Y,
                     const float* __restrict__ ny, const float* __restrict__ rad, int* __restrict__ part, int Mx, int My,
                     int Kp, int nct) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [2 buffers][X tile, Y tile][128][36]; at the end the counts
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int m0 = blockIdx.x * NN_TILE, chunk = blockIdx.y, splits = gridDim.y;
  const int t0 = (int)((long long)chunk * nct / splits), t1 = (int)((long long)(chunk + 1) * nct / splits);
  const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};

  float nxr[4][4];
  int cnt[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wr * 64 + i * 16 + 4 * fq + r;
      nxr[i][r] = row < Mx ? nx[row] : 0.f;
      cnt[i][r] = 0;
    }

  nn_gemm_tiles(X, Y, lds, Mx, My, Kp, m0, t0, t1, [&](int cbase, f32x4 (&acc)[4][4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = cbase + j * 16 + fr;
      const bool cok = col < My;
      const float nyv = cok ? ny[col] : 0.f, rv = cok ? rad[col] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d = __builtin_fmaf(-2.f, acc[i][j][r], nxr[i][r] + nyv);
          cnt[i][r] += (cok && d <= rv) ? 1 : 0;
        }
      acc[0][j] = zero; acc[1][j] = zero; acc[2][j] = zero; acc[3][j] = zero;
    }
  });

  int* red = reinterpret_cast<int*>(lds);  // [2 column waves][128]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int v = cnt[i][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
      if (fr == 0) red[wc * NN_TILE + wr * 64 + i * 16 + 4 * fq + r] = v;
    }
  __syncthreads();
  if (tid < NN_TILE && m0 + tid < Mx) part[(size_t)chunk * Mx + m0 + tid] = red[tid] + red[NN_TILE + tid];
}

__global__ __launch_bounds__(256) void nn_count_sum_kernel(const int* __restrict__ part, int* __restrict__ cnt, int Mx,
                                                           int splits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Mx) return;
  int s = part[i];
  for (int c = 1; c < splits; ++c) s += part[(size_t)c * Mx + i];
  cnt[i] = s;
}

// ---------------------------------------------------------------- kernel MMD over the upper triangle of one Gram
__device__ __forceinline__ double nn_wave_sum(double s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// h = 2 / (n - 1) * sum_i norm_i, c = log2(e) / (4 h): every thread its rows in index order in fp64, a shuffle tree,
// the four waves in order
__global__ __launch_bounds__(256) void nn_mmd_bw_kernel(const float* __restrict__ norm, int n, float* __restrict__ bw) {
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s = 0.0;
  for (int i = tid; i < n; i += 256) s += (double)norm[i];
  s = nn_wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) {
    const double h = 2.0 / (double)(n - 1) * (((red[0] + red[1]) + red[2]) + red[3]);
    bw[0] = (float)h;
    bw[1] = (float)(1.4426950408889634 / (4.0 * h));  // (h = 0: inf, and the sums come out non-finite)
  }
}

// One workgroup per 128 x 128 tile (I, J), I <= J, of the Gram of Z = [X; Y]: pair p = J (J + 1) / 2 + I, so that
// neighbours share the tile column J. nn_gemm_tiles does not serve: it addresses its operands as X + row * Kp and
// Y + row * Kp, while a tile of Z may straddle row Mx and takes every row from the matrix that holds it; and with
// exactly one tile per workgroup the epilogue leaves the loop, so the loader's registers are dead when it runs. The
// loop itself (staging, pitch, one barrier per step, MFMA order) is nn_gemm_tiles'. Rows past M are read from row
// M - 1: their sums only reach masked elements, and every load stays inside the matrices
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void nn_mmd_kernel(const float* __restrict__ X, const float* __restrict__ nx, const float* __restrict__ Y,
                   const float* __restrict__ ny, const float* __restrict__ bw, double* __restrict__ part, int Mx, int My,
                   int Kp, int p0, int skip_aa) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [2 buffers][I tile, J tile][128][36]; at the end the sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int M = Mx + My, p = p0 + (int)blockIdx.x;  // (at most 8192 tile rows: p < 2^26)
  int J = (int)((__builtin_sqrtf(8.f * (float)p + 1.f) - 1.f) * 0.5f);
  while (J * (J + 1) / 2 > p) --J;  // the float root is one step off at the most
  while ((J + 1) * (J + 2) / 2 <= p) ++J;
  const int I = p - J * (J + 1) / 2;
  const int nk = (Kp + NN_BK - 1) / NN_BK;
  const int lr = tid >> 3, lq = tid & 7;  // the loader's rows lr + 32 p, its 16-byte word lq of the 32 k
  const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* pi[4];
  const float* pj[4];
  f32x4 si[4], sj[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int zi = min(I * NN_TILE + lr + 32 * q, M - 1), zj = min(J * NN_TILE + lr + 32 * q, M - 1);
    pi[q] = (zi < Mx ? X + (size_t)zi * Kp : Y + (size_t)(zi - Mx) * Kp) + 4 * lq;
    pj[q] = (zj < Mx ? X + (size_t)zj * Kp : Y + (size_t)(zj - Mx) * Kp) + 4 * lq;
  }

  auto fetch = [&](int it) {  // k past Kp reads as zeros
    const int k0 = it * NN_BK;
    const bool kok = k0 + 4 * lq < Kp;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      si[q] = kok ? *reinterpret_cast<const f32x4*>(pi[q] + k0) : zero;
      sj[q] = kok ? *reinterpret_cast<const f32x4*>(pj[q] + k0) : zero;
    }
  };
  auto stash = [&](int buf) {
    float* bx = lds + buf * 2 * NN_TILE_F + lr * NN_PITCH + 4 * lq;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<f32x4*>(bx + 32 * q * NN_PITCH) = si[q];
      *reinterpret_cast<f32x4*>(bx + NN_TILE_F + 32 * q * NN_PITCH) = sj[q];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = zero;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int it = 0; it < nk; ++it) {
    const int buf = it & 1;
    const bool more = it + 1 < nk;
    if (more) fetch(it + 1);
    const float* bx = lds + buf * 2 * NN_TILE_F + (wr * 64 + fr) * NN_PITCH + 4 * fq;
    const float* by = lds + buf * 2 * NN_TILE_F + NN_TILE_F + (wc * 64 + fr) * NN_PITCH + 4 * fq;
#pragma unroll
    for (int kk = 0; kk < NN_BK; kk += 16) {  // lane group fq supplies k = kk + 4 fq + e to MFMA e, for A and B alike
      f32x4 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4*>(bx + i * 16 * NN_PITCH + kk);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const f32x4*>(by + j * 16 * NN_PITCH + kk);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
    }
    if (more) stash(buf ^ 1);  // (last read in step it - 1, before that step's barrier)
    __syncthreads();
  }

  // C fragment acc[i][j][r] = row I 128 + wr 64 + i 16 + 4 fq + r, column J 128 + wc 64 + j 16 + fr. One exp2 per
  // pair; the bandwidths lie a factor 2 apart, so the other four Gaussians are its repeated squares
  const float c = bw[1];
  const int r0 = I * NN_TILE + wr * 64 + 4 * fq, c0 = J * NN_TILE + wc * 64 + fr;
  float nr[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int z = min(r0 + i * 16 + r, M - 1);
      nr[i][r] = z < Mx ? nx[z] : ny[z - Mx];
    }
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;  // the lane's sums per class (row >= Mx) + (col >= Mx): AA, AB, BB
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = c0 + j * 16, z = min(col, M - 1);
    const float nc = z < Mx ? nx[z] : ny[z - Mx];
    const bool cok = col < M && !(skip_aa && col < Mx);  // (row < col: with col in X the pair is (A, A))
    const int cc = col >= Mx ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + i * 16 + r;
        const float d = fmaxf(__builtin_fmaf(-2.f, acc[i][j][r], nr[i][r] + nc), 0.f);
        const float e1 = __builtin_amdgcn_exp2f(-d * c), e2 = e1 * e1, e4 = e2 * e2, e8 = e4 * e4, e16 = e8 * e8;
        const float t = (((e1 + e2) + e4) + e8) + e16;
        const bool ok = cok && row < col;  // strictly above the diagonal
        const int cls = (row >= Mx ? 1 : 0) + cc;
        s0 += (ok && cls == 0) ? t : 0.f;
        s1 += (ok && cls == 1) ? t : 0.f;
        s2 += (ok && cls == 2) ? t : 0.f;
      }
  }
  double* red = reinterpret_cast<double*>(lds);  // [4 waves][3] (the tiles are free after the loop's last barrier)
  const double v0 = nn_wave_sum((double)s0), v1 = nn_wave_sum((double)s1), v2 = nn_wave_sum((double)s2);
  if (lane == 0) {
    red[wave * 3 + 0] = v0;
    red[wave * 3 + 1] = v1;
    red[wave * 3 + 2] = v2;
  }
  __syncthreads();
  if (tid < 3) part[(size_t)blockIdx.x * 3 + tid] = ((red[tid] + red[3 + tid]) + red[6 + tid]) + red[9 + tid];
}

// out = {S_AA, S_BB, S_AB, k_rr, k_ff, k_rf, mmd2, h}. A fixed order: thread t adds the pairs t, t + 256, ... in index
// order per class, then a shuffle tree and the four waves in order. With skip_aa, S_AA is the cached *saa (null: 0)
__global__ __launch_bounds__(256) void nn_mmd_final_kernel(const double* __restrict__ part, int pairs,
                                                           const double* __restrict__ saa, int skip_aa, int Mx, int My,
                                                           const float* __restrict__ bw, double* __restrict__ out) {
  __shared__ double red[12];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int p = tid; p < pairs; p += 256) {
    s0 += part[(size_t)p * 3 + 0];
    s1 += part[(size_t)p * 3 + 1];
    s2 += part[(size_t)p * 3 + 2];
  }
  s0 = nn_wave_sum(s0), s1 = nn_wave_sum(s1), s2 = nn_wave_sum(s2);
  if (lane == 0) {
    red[wave * 3 + 0] = s0;
    red[wave * 3 + 1] = s1;
    red[wave * 3 + 2] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    double raw[3];
    for (int q = 0; q < 3; ++q) raw[q] = (((red[q] + red[3 + q]) + red[6 + q]) + red[9 + q]) / 5.0;
    const double na = (double)Mx, nb = (double)My;
    const double saa_v = skip_aa ? (saa ? *saa : 0.0) : raw[0], sab = raw[1], sbb = raw[2];
    const double krr = Mx > 1 ? 2.0 * saa_v / (na * (na - 1.0)) : 0.0, kff = My > 1 ? 2.0 * sbb / (nb * (nb - 1.0)) : 0.0;
    const double krf = My > 0 ? sab / (na * nb) : 0.0;
    out[0] = saa_v, out[1] = sbb, out[2] = sab;
    out[3] = krr, out[4] = kff, out[5] = krf;
    out[6] = krr + kff - 2.0 * krf;
    out[7] = (double)bw[0];
  }
}

// ---------------------------------------------------------------- Frechet distance: the polar iteration on C [n][n]
// tile pair p -> (I, J), I <= J, p = J (J + 1) / 2 + I (nn_mmd's order)
__device__ __forceinline__ void nn_tri_pair(int p, int& I, int& J) {
  J = (int)((__builtin_sqrtf(8.f * (float)p + 1.f) - 1.f) * 0.5f);
  while (J * (J + 1) / 2 > p) --J;  // the float root is one step off at the most
  while ((J + 1) * (J + 2) / 2 <= p) ++J;
  I = p - J * (J + 1) / 2;
}

// out [M][ld] = scale A B^T, A and B [M][Kp] (Kp a multiple of 16): one workgroup per tile of 32 FR rows and columns,
// a wave 16 FR x 16 FR. SYM (A is B): blockIdx.x is a pair of the upper triangle, and an off-diagonal tile goes to both
// halves. Rows past M read as zeros, so the columns M..ld-1 of out are written as zeros
template <int FR, bool SYM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, FR == 4 ? 2 : 4)))
void nn_fd_nt_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ out, int M, int Kp,
                     int ld, float scale) {
  constexpr int TILE = 32 * FR, TF = TILE * NN_PITCH;
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [2 buffers][A tile, B tile][TILE][36]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  int I, J;
  if (SYM) nn_tri_pair((int)blockIdx.x, I, J); else I = (int)blockIdx.y, J = (int)blockIdx.x;
  const int nk = (Kp + NN_BK - 1) / NN_BK;
  const int lr = tid >> 3, lq = tid & 7;  // the loader's rows lr + 32 p, its 16-byte word lq of the 32 k
  const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 sa[FR], sb[FR];

  auto fetch = [&](int it) {
    const int k0 = it * NN_BK + 4 * lq;
    const bool kok = k0 < Kp;
#pragma unroll
    for (int p = 0; p < FR; ++p) {
      const int ra = I * TILE + lr + 32 * p, rb = J * TILE + lr + 32 * p;
      sa[p] = (kok && ra < M) ? *reinterpret_cast<const f32x4*>(A + (size_t)ra * Kp + k0) : zero;
      sb[p] = (kok && rb < M) ? *reinterpret_cast<const f32x4*>(B + (size_t)rb * Kp + k0) : zero;
    }
  };
  auto stash = [&](int buf) {
    float* bx = lds + buf * 2 * TF + lr * NN_PITCH + 4 * lq;
#pragma unroll
    for (int p = 0; p < FR; ++p) {
      *reinterpret_cast<f32x4*>(bx + 32 * p * NN_PITCH) = sa[p];
      *reinterpret_cast<f32x4*>(bx + TF + 32 * p * NN_PITCH) = sb[p];
    }
  };

  f32x4 acc[FR][FR];
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int j = 0; j < FR; ++j) acc[i][j] = zero;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int it = 0; it < nk; ++it) {
    const int buf = it & 1;
    const bool more = it + 1 < nk;
    if (more) fetch(it + 1);
    const float* bx = lds + buf * 2 * TF + (wr * 16 * FR + fr) * NN_PITCH + 4 * fq;
    const float* by = lds + buf * 2 * TF + TF + (wc * 16 * FR + fr) * NN_PITCH + 4 * fq;
#pragma unroll
    for (int kk = 0; kk < NN_BK; kk += 16) {  // lane group fq supplies k = kk + 4 fq + e to MFMA e, for A and B alike
      f32x4 a[FR], b[FR];
#pragma unroll
      for (int i = 0; i < FR; ++i) a[i] = *reinterpret_cast<const f32x4*>(bx + i * 16 * NN_PITCH + kk);
#pragma unroll
      for (int j = 0; j < FR; ++j) b[j] = *reinterpret_cast<const f32x4*>(by + j * 16 * NN_PITCH + kk);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < FR; ++i)
#pragma unroll
          for (int j = 0; j < FR; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
    }
    if (more) stash(buf ^ 1);  // (last read in step it - 1, before that step's barrier)
    __syncthreads();
  }

  // C fragment acc[i][j][r] = row I TILE + wr 16 FR + 16 i + 4 fq + r, column J TILE + wc 16 FR + 16 j + fr. In the
  // mirror image the four r are four consecutive columns from a multiple of 4: inside the row's ld, 16-byte aligned
  const bool mirror = SYM && I != J;
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int j = 0; j < FR; ++j) {
      const int row0 = I * TILE + wr * 16 * FR + 16 * i + 4 * fq, col = J * TILE + wc * 16 * FR + 16 * j + fr;
      f32x4 v = acc[i][j];
      v[0] *= scale, v[1] *= scale, v[2] *= scale, v[3] *= scale;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (row0 + r < M && col < ld) out[(size_t)(row0 + r) * ld + col] = v[r];
      if (mirror && col < M && row0 < ld) *reinterpret_cast<f32x4*>(out + (size_t)col * ld + row0) = v;
    }
}

// Xn = 1.5 X - 0.5 P X, all [M][ld]. P's rows are the row-major operand (nn_fd_nt's A); X is the k-major one
template <int FR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, FR == 4 ? 2 : 4)))
void nn_fd_step_kernel(const float* __restrict__ P, const float* __restrict__ X, float* __restrict__ Xn, int M, int ld) {
  constexpr int TILE = 32 * FR, TF = TILE * NN_PITCH, PB = TILE + 4, BF = NN_BK * PB;
  constexpr int CW = TILE / 4, KR = 256 / CW;  // 16-byte words per k row of the X tile; k rows per pass of the loader
  static_assert(KR * FR == NN_BK && (4 * PB) % 64 == 16, "nn_fd_step: the X tile's loader and pitch");
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [2 buffers][TILE][36] of P, then [2 buffers][32][PB] of X
  float* ldx = lds + 2 * TF;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int I = (int)blockIdx.y, J = (int)blockIdx.x;
  const int nk = (M + NN_BK - 1) / NN_BK;
  const int lr = tid >> 3, lq = tid & 7;     // P: rows lr + 32 p, 16-byte word lq of the 32 k
  const int lk = tid / CW, lc = tid % CW;    // X: k rows lk + KR p, 16-byte word lc of the TILE columns
  const int xc = J * TILE + 4 * lc;
  const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 sp[FR], sx[FR];

  auto fetch = [&](int it) {  // P: rows past M and k past ld read as zeros; X: k rows past M and columns past ld
    const int k0 = it * NN_BK + 4 * lq;
#pragma unroll
    for (int p = 0; p < FR; ++p) {
      const int rp = I * TILE + lr + 32 * p, kx = it * NN_BK + lk + KR * p;
      sp[p] = (k0 < ld && rp < M) ? *reinterpret_cast<const f32x4*>(P + (size_t)rp * ld + k0) : zero;
      sx[p] = (kx < M && xc < ld) ? *reinterpret_cast<const f32x4*>(X + (size_t)kx * ld + xc) : zero;
    }
  };
  auto stash = [&](int buf) {
    float* bp = lds + buf * TF + lr * NN_PITCH + 4 * lq;
    float* bx = ldx + buf * BF + lk * PB + 4 * lc;
#pragma unroll
    for (int p = 0; p < FR; ++p) {
      *reinterpret_cast<f32x4*>(bp + 32 * p * NN_PITCH) = sp[p];
      *reinterpret_cast<f32x4*>(bx + KR * p * PB) = sx[p];
    }
  };

  f32x4 acc[FR][FR];
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int j = 0; j < FR; ++j) acc[i][j] = zero;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int it = 0; it < nk; ++it) {
    const int buf = it & 1;
    const bool more = it + 1 < nk;
    if (more) fetch(it + 1);
    const float* bp = lds + buf * TF + (wr * 16 * FR + fr) * NN_PITCH + 4 * fq;
    const float* bx = ldx + buf * BF + 4 * fq * PB + wc * 16 * FR + fr;
#pragma unroll
    for (int kk = 0; kk < NN_BK; kk += 16) {  // lane group fq supplies k = kk + 4 fq + e to MFMA e, for P and X alike
      f32x4 a[FR];
      float b[FR][4];
#pragma unroll
      for (int i = 0; i < FR; ++i) a[i] = *reinterpret_cast<const f32x4*>(bp + i * 16 * NN_PITCH + kk);
#pragma unroll
      for (int j = 0; j < FR; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) b[j][e] = bx[(kk + e) * PB + 16 * j];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < FR; ++i)
#pragma unroll
          for (int j = 0; j < FR; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
    }
    if (more) stash(buf ^ 1);  // (last read in step it - 1, before that step's barrier)
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int j = 0; j < FR; ++j) {
      const int row0 = I * TILE + wr * 16 * FR + 16 * i + 4 * fq, col = J * TILE + wc * 16 * FR + 16 * j + fr;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (row0 + r < M && col < ld) {
          const size_t o = (size_t)(row0 + r) * ld + col;
          Xn[o] = __builtin_fmaf(-0.5f, acc[i][j][r], 1.5f * X[o]);
        }
    }
}

// the sum of a double over the workgroup's 256 threads in a fixed order: a shuffle tree, then the four waves in order
__device__ __forceinline__ double nn_block_sum(double s, double* red) {
  s = nn_wave_sum(s);
  __syncthreads();  // (red is free again)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double nn_block_max(double s, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = fmax(s, __shfl_xor(s, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// one wave per row: rmean = the row's mean over its n columns (0 without center), rabs = sum_j |c - rmean|
__global__ __launch_bounds__(256) void nn_fd_rows_kernel(const float* __restrict__ C, int n, int ld, int center,
                                                         double* __restrict__ rmean, double* __restrict__ rabs) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* c = C + (size_t)row * ld;
  double m = 0.0;
  if (center) {
    double s = 0.0;
    for (int j = lane; j < n; j += 64) s += (double)c[j];
    m = nn_wave_sum(s) / (double)n;
  }
  double a = 0.0;
  for (int j = lane; j < n; j += 64) a += fabs((double)c[j] - m);
  a = nn_wave_sum(a);
  if (lane == 0) rmean[row] = m, rabs[row] = a;
}

// thread j of row block b: sum_r |c[r][j] - rmean[r]| over the block's 64 rows in index order
__global__ __launch_bounds__(256) void nn_fd_cols_kernel(const float* __restrict__ C, int n, int ld,
                                                         const double* __restrict__ rmean, double* __restrict__ cpart) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int r0 = blockIdx.y * NN_MEAN_ROWS, r1 = min(n, r0 + NN_MEAN_ROWS);
  double s = 0.0;
  for (int r = r0; r < r1; ++r) s += fabs((double)C[(size_t)r * ld + j] - rmean[r]);
  cpart[(size_t)blockIdx.y * n + j] = s;
}

// al = {alpha, 1 / alpha (0 when alpha is 0: C = 0 has X = 0 and a nuclear norm of 0)}
__global__ __launch_bounds__(256) void nn_fd_alpha_kernel(const double* __restrict__ rabs, const double* __restrict__ cpart,
                                                          int n, int blocks, double* __restrict__ al) {
  __shared__ double red[4];
  double mr = 0.0, mc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    mr = fmax(mr, rabs[i]);
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += cpart[(size_t)b * n + i];
    mc = fmax(mc, s);
  }
  mr = nn_block_max(mr, red);
  mc = nn_block_max(mc, red);
  if (threadIdx.x == 0) {
    const double alpha = sqrt(mr * mc);
    al[0] = alpha;
    al[1] = alpha > 0.0 ? 1.0 / alpha : 0.0;
  }
}

// a workgroup per row: C <- C - rmean in place (columns n..ld-1: 0), X = C / alpha
__global__ __launch_bounds__(256) void nn_fd_x0_kernel(float* __restrict__ C, int n, int ld, const double* __restrict__ rmean,
                                                       const double* __restrict__ al, float* __restrict__ X) {
  const int row = blockIdx.x;
  const double m = rmean[row], alpha = al[0];
  for (int j = threadIdx.x; j < ld; j += 256) {
    const size_t o = (size_t)row * ld + j;
    const float c = j < n ? (float)((double)C[o] - m) : 0.f;
    C[o] = c;
    X[o] = alpha > 0.0 ? (float)((double)c / alpha) : 0.f;
  }
}

// part [workgroup] = sum_ij X_ij C_ij over the workgroup's 4 rows: a wave per row in index order, the waves in order
__global__ __launch_bounds__(256) void nn_fd_trace_kernel(const float* __restrict__ X, const float* __restrict__ C, int n,
                                                          int ld, double* __restrict__ part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  double s = 0.0;
  if (row < n)
    for (int j = lane; j < n; j += 64) s += (double)X[(size_t)row * ld + j] * (double)C[(size_t)row * ld + j];
  s = nn_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// out [0] = sum_i norm_i / (n - 1): the trace of the covariance of n rows centred by their own mean
__global__ __launch_bounds__(256) void nn_fd_tr_kernel(const float* __restrict__ norm, int n, double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)norm[i];
  s = nn_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s / (double)(n - 1);
}

// out = {fd, mean2, tr_a, tr_b, nuc, tail, alpha, iters}. tprev, tlast: nn_fd_trace's parts of the last two iterates.
// mpart [mblocks][Kp]: nn_mean_part's sums of F_B's rows, d = their mean; norm_b [n] = |F_B i|^2; tra: tr S_A. Without
// them (the probe on a bare C) the three terms are 0
__global__ __launch_bounds__(256) void nn_fd_final_kernel(const double* __restrict__ tprev, const double* __restrict__ tlast,
                                                          int nparts, const double* __restrict__ al,
                                                          const double* __restrict__ mpart, int mblocks, int Kp,
                                                          const float* __restrict__ norm_b, const double* __restrict__ tra,
                                                          int n, int iters, double* __restrict__ out) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  double v0 = 0.0, v1 = 0.0, m2 = 0.0, sb = 0.0;
  for (int p = tid; p < nparts; p += 256) v0 += tprev[p], v1 += tlast[p];
  if (mpart)
    for (int k = tid; k < Kp; k += 256) {
      double s = 0.0;
      for (int b = 0; b < mblocks; ++b) s += mpart[(size_t)b * Kp + k];
      s /= (double)n;
      m2 += s * s;
    }
  if (norm_b)
    for (int i = tid; i < n; i += 256) sb += (double)norm_b[i];
  v0 = nn_block_sum(v0, red), v1 = nn_block_sum(v1, red), m2 = nn_block_sum(m2, red), sb = nn_block_sum(sb, red);
  if (tid == 0) {
    const double alpha = al[0], nuc = v1;
    const double tr_a = tra ? tra[0] : 0.0, tr_b = norm_b ? (sb - (double)n * m2) / (double)(n - 1) : 0.0;
    out[0] = m2 + tr_a + tr_b - 2.0 * nuc;
    out[1] = m2, out[2] = tr_a, out[3] = tr_b;
    out[4] = nuc;
    out[5] = v1 - v0;
    out[6] = alpha;
    out[7] = (double)iters;
  }
}

static inline bool nn_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool nn_shape_ok(int M, int K) { return M >= 1 && M <= NN_MAX_ROWS && K >= 1 && K <= NN_MAX_K; }
// the operands and the chunking of one distance GEMM
static inline bool nn_gemm_ok(const float* X, const float* nx, const float* Y, const float* ny, int Mx, int My, int Kp,
                              int splits) {
  return X && nx && Y && ny && nn_shape_ok(Mx, Kp) && nn_shape_ok(My, Kp) && Kp % 16 == 0 && nn_al16(X) && nn_al16(Y) &&
         splits >= 1 && splits <= nn_col_tiles(My) && splits <= 65535;
}
// more than 64 KB of dynamic LDS has to be asked for, once per kernel
template <class Kernel>
static inline hipError_t nn_big_lds(Kernel kernel, size_t bytes, bool* done) {
  if (*done) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  *done = e == hipSuccess;
  return e;
}

}  // namespace dcg

using namespace dcg;

extern "C" int dcg_nn_features(const float* x, int n, int K, float* mu, double* part, int compute_mu, float* F,
                               float* norm, hipStream_t st) {
  if (!x || !F || !norm || !nn_shape_ok(n, K) || (compute_mu && (!mu || !part))) return -2;
  if (compute_mu) {
    const int blocks = (n + NN_MEAN_ROWS - 1) / NN_MEAN_ROWS;
    hipLaunchKernelGGL(nn_mean_part_kernel, dim3((K + 255) / 256, blocks), dim3(256), 0, st, x, n, K, part);
    hipLaunchKernelGGL(nn_mean_final_kernel, dim3((K + 255) / 256), dim3(256), 0, st, (const double*)part, blocks, K,
                       (double)n, mu);
  }
  hipLaunchKernelGGL(nn_features_kernel, dim3((n + NN_FEAT_ROWS - 1) / NN_FEAT_ROWS), dim3(256), 0, st, x,
                     (const float*)mu, F, norm, n, K, nn_kpad(K));
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_top1(const float* X, const float* nx, const float* Y, const float* ny, uint64_t* part, int Mx,
                           int My, int Kp, int loo, int splits, hipStream_t st) {
  static_assert(NN_BK % 16 == 0 && NN_PITCH % 4 == 0 && NN_TILE == 128, "nn: tile sizes");
  if (!X || !nx || !Y || !ny || !part || !nn_shape_ok(Mx, Kp) || !nn_shape_ok(My, Kp) || Kp % 16 || !nn_al16(X) ||
      !nn_al16(Y))
    return -2;
  const int nct = nn_col_tiles(My);
  if (splits < 1 || splits > nct || splits > 65535 || (loo && (Mx != My || My < 2))) return -2;
  static bool attr = false;
  if (!attr) {  // 74 KB: two workgroups per CU
    hipError_t e = hipFuncSetAttribute((const void*)nn_top1_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)NN_TOP1_LDS);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  hipLaunchKernelGGL(nn_top1_kernel, dim3((Mx + NN_TILE - 1) / NN_TILE, splits), dim3(256), NN_TOP1_LDS, st, X, nx, Y, ny,
                     reinterpret_cast<unsigned long long*>(part), Mx, My, Kp, loo ? 1 : 0, nct);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_merge(const uint64_t* part, int* idx, int Mx, int splits, hipStream_t st) {
  if (!part || !idx || Mx < 1 || Mx > NN_MAX_ROWS || splits < 1) return -2;
  hipLaunchKernelGGL(nn_merge_kernel, dim3((Mx + 255) / 256), dim3(256), 0, st,
                     reinterpret_cast<const unsigned long long*>(part), idx, Mx, splits);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_refine(const float* x0, const float* y0, const int* idx, double* dist, int Mx, int My, int K,
                             hipStream_t st) {
  if (!x0 || !y0 || !idx || !dist || !nn_shape_ok(Mx, K) || !nn_shape_ok(My, K)) return -2;
  hipLaunchKernelGGL(nn_refine_kernel, dim3((Mx + 3) / 4), dim3(256), 0, st, x0, y0, idx, dist, Mx, My, K);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_topk(const float* X, const float* nx, const float* Y, const float* ny, uint64_t* part, int Mx,
                           int My, int Kp, int loo, int splits, int k, hipStream_t st) {
  if (!part || !nn_gemm_ok(X, nx, Y, ny, Mx, My, Kp, splits) || (loo && Mx != My) || k < 1 || k > NN_MAX_KNN ||
      k > My - (loo ? 1 : 0))
    return -2;
  static bool attr = false;
  const hipError_t e = nn_big_lds(nn_topk_kernel, NN_GEMM_LDS, &attr);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(nn_topk_kernel, dim3((Mx + NN_TILE - 1) / NN_TILE, splits), dim3(256), NN_GEMM_LDS, st, X, nx, Y, ny,
                     reinterpret_cast<unsigned long long*>(part), Mx, My, Kp, loo ? 1 : 0, nn_col_tiles(My), k);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_merge_k(const uint64_t* part, int* idx, int Mx, int splits, int k, hipStream_t st) {
  if (!part || !idx || Mx < 1 || Mx > NN_MAX_ROWS || splits < 1 || k < 1 || k > NN_MAX_KNN) return -2;
  hipLaunchKernelGGL(nn_merge_k_kernel, dim3((Mx + 3) / 4), dim3(256), 0, st,
                     reinterpret_cast<const unsigned long long*>(part), idx, Mx, splits, k);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_radius(const float* x0, const float* y0, const int* idx, double* dist, float* rad, int Mx, int My,
                             int K, int k, hipStream_t st) {
  if (!x0 || !y0 || !idx || !dist || !rad || !nn_shape_ok(Mx, K) || !nn_shape_ok(My, K) || k < 1 || k > NN_MAX_KNN)
    return -2;
  hipLaunchKernelGGL(nn_radius_kernel, dim3(Mx), dim3(256), 0, st, x0, y0, idx, dist, rad, Mx, My, K, k);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_count(const float* X, const float* nx, const float* Y, const float* ny, const float* rad, int* part,
                            int* cnt, int Mx, int My, int Kp, int splits, hipStream_t st) {
  if (!rad || !part || !cnt || !nn_gemm_ok(X, nx, Y, ny, Mx, My, Kp, splits)) return -2;
  static bool attr = false;
  const hipError_t e = nn_big_lds(nn_count_kernel, NN_GEMM_LDS, &attr);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(nn_count_kernel, dim3((Mx + NN_TILE - 1) / NN_TILE, splits), dim3(256), NN_GEMM_LDS, st, X, nx, Y, ny,
                     rad, part, Mx, My, Kp, nn_col_tiles(My));
  hipLaunchKernelGGL(nn_count_sum_kernel, dim3((Mx + 255) / 256), dim3(256), 0, st, (const int*)part, cnt, Mx, splits);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_mmd_bw(const float* norm, int n, float* bw, hipStream_t st) {
  if (!norm || !bw || n < 2 || n > NN_MAX_ROWS) return -2;
  hipLaunchKernelGGL(nn_mmd_bw_kernel, dim3(1), dim3(256), 0, st, norm, n, bw);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_mmd(const float* X, const float* nx, const float* Y, const float* ny, const float* bw, double* part,
                          int Mx, int My, int Kp, int skip_aa, hipStream_t st) {
  if (!X || !nx || !bw || !part || !nn_shape_ok(Mx, Kp) || My < 0 || My > NN_MAX_ROWS - Mx || Kp % 16 || !nn_al16(X) ||
      (My > 0 && (!Y || !ny || !nn_al16(Y))) || (skip_aa && My < 1))
    return -2;
  const int pairs = nn_mmd_pairs(Mx, My, skip_aa);
  static bool attr = false;
  const hipError_t e = nn_big_lds(nn_mmd_kernel, NN_GEMM_LDS, &attr);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(nn_mmd_kernel, dim3(pairs), dim3(256), NN_GEMM_LDS, st, X, nx, Y, ny, bw, part, Mx, My, Kp,
                     nn_mmd_pairs(Mx, My, 0) - pairs, skip_aa ? 1 : 0);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_mmd_final(const double* part, int pairs, const double* saa, int skip_aa, int Mx, int My,
                                const float* bw, double* out, hipStream_t st) {
  if (!part || !bw || !out || Mx < 1 || My < 0 || Mx > NN_MAX_ROWS || My > NN_MAX_ROWS - Mx || (skip_aa && My < 1) ||
      pairs != nn_mmd_pairs(Mx, My, skip_aa))
    return -2;
  hipLaunchKernelGGL(nn_mmd_final_kernel, dim3(1), dim3(256), 0, st, part, pairs, saa, skip_aa ? 1 : 0, Mx, My, bw, out);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- Frechet distance: launchers
static inline bool nn_fd_ok(int n) { return n >= 2 && n <= NN_FD_MAX_ROWS; }

template <int FR, bool SYM>
static int nn_fd_nt_launch(const float* A, const float* B, float* out, int M, int Kp, int ld, float scale, hipStream_t st) {
  constexpr int TILE = 32 * FR;
  constexpr size_t bytes = (size_t)4 * TILE * NN_PITCH * sizeof(float);
  static bool attr = false;
  const hipError_t e = nn_big_lds(nn_fd_nt_kernel<FR, SYM>, bytes, &attr);
  if (e != hipSuccess) return (int)e;
  const int T = (M + TILE - 1) / TILE;
  hipLaunchKernelGGL((nn_fd_nt_kernel<FR, SYM>), SYM ? dim3(T * (T + 1) / 2) : dim3(T, T), dim3(256), bytes, st, A, B, out, M,
                     Kp, ld, scale);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_fd_gram(const float* FA, const float* FB, float* C, int n, int Kp, hipStream_t st) {
  if (!FA || !FB || !C || !nn_fd_ok(n) || Kp < 16 || Kp > NN_MAX_K || Kp % 16 || !nn_al16(FA) || !nn_al16(FB) || !nn_al16(C))
    return -2;
  const float scale = 1.f / (float)(n - 1);
  return nn_fd_tile(n) == 64 ? nn_fd_nt_launch<2, false>(FA, FB, C, n, Kp, nn_fd_ld(n), scale, st)
                             : nn_fd_nt_launch<4, false>(FA, FB, C, n, Kp, nn_fd_ld(n), scale, st);
}

extern "C" int dcg_nn_fd_scale(float* C, int n, int center, double* rmean, double* rabs, double* cpart, double* al, float* X,
                               hipStream_t st) {
  if (!C || !rmean || !rabs || !cpart || !al || !X || !nn_fd_ok(n) || !nn_al16(C) || !nn_al16(X)) return -2;
  const int ld = nn_fd_ld(n), blocks = (n + NN_MEAN_ROWS - 1) / NN_MEAN_ROWS;
  hipLaunchKernelGGL(nn_fd_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, st, (const float*)C, n, ld, center ? 1 : 0, rmean, rabs);
  hipLaunchKernelGGL(nn_fd_cols_kernel, dim3((n + 255) / 256, blocks), dim3(256), 0, st, (const float*)C, n, ld,
                     (const double*)rmean, cpart);
  hipLaunchKernelGGL(nn_fd_alpha_kernel, dim3(1), dim3(256), 0, st, (const double*)rabs, (const double*)cpart, n, blocks, al);
  hipLaunchKernelGGL(nn_fd_x0_kernel, dim3(n), dim3(256), 0, st, C, n, ld, (const double*)rmean, (const double*)al, X);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_fd_ppt(const float* X, float* P, int n, hipStream_t st) {
  if (!X || !P || X == P || !nn_fd_ok(n) || !nn_al16(X) || !nn_al16(P)) return -2;
  const int ld = nn_fd_ld(n);
  return nn_fd_tile(n) == 64 ? nn_fd_nt_launch<2, true>(X, X, P, n, ld, ld, 1.f, st)
                             : nn_fd_nt_launch<4, true>(X, X, P, n, ld, ld, 1.f, st);
}

template <int FR>
static int nn_fd_step_launch(const float* P, const float* X, float* Xn, int n, hipStream_t st) {
  constexpr int TILE = 32 * FR;
  constexpr size_t bytes = (size_t)2 * (TILE * NN_PITCH + NN_BK * (TILE + 4)) * sizeof(float);
  static bool attr = false;
  const hipError_t e = nn_big_lds(nn_fd_step_kernel<FR>, bytes, &attr);
  if (e != hipSuccess) return (int)e;
  const int T = (n + TILE - 1) / TILE;
  hipLaunchKernelGGL((nn_fd_step_kernel<FR>), dim3(T, T), dim3(256), bytes, st, P, X, Xn, n, nn_fd_ld(n));
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_fd_step(const float* P, const float* X, float* Xn, int n, hipStream_t st) {
  if (!P || !X || !Xn || X == Xn || P == Xn || !nn_fd_ok(n) || !nn_al16(P) || !nn_al16(X) || !nn_al16(Xn)) return -2;
  return nn_fd_tile(n) == 64 ? nn_fd_step_launch<2>(P, X, Xn, n, st) : nn_fd_step_launch<4>(P, X, Xn, n, st);
}

extern "C" int dcg_nn_fd_trace(const float* X, const float* C, int n, double* part, hipStream_t st) {
  if (!X || !C || !part || !nn_fd_ok(n)) return -2;
  hipLaunchKernelGGL(nn_fd_trace_kernel, dim3(nn_fd_parts(n)), dim3(256), 0, st, X, C, n, nn_fd_ld(n), part);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_fd_tr(const float* norm, int n, double* out, hipStream_t st) {
  if (!norm || !out || !nn_fd_ok(n)) return -2;
  hipLaunchKernelGGL(nn_fd_tr_kernel, dim3(1), dim3(256), 0, st, norm, n, out);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_fd_mean(const float* FB, int n, int Kp, double* mpart, hipStream_t st) {
  if (!FB || !mpart || !nn_fd_ok(n) || Kp < 1 || Kp > NN_MAX_K) return -2;
  hipLaunchKernelGGL(nn_mean_part_kernel, dim3((Kp + 255) / 256, (n + NN_MEAN_ROWS - 1) / NN_MEAN_ROWS), dim3(256), 0, st, FB, n,
                     Kp, mpart);
  return (int)hipGetLastError();
}

extern "C" int dcg_nn_fd_final(const double* tprev, const double* tlast, const double* al, const double* mpart, int Kp,
                               const float* norm_b, const double* tra, int n, int iters, double* out, hipStream_t st) {
  if (!tprev || !tlast || !al || !out || !nn_fd_ok(n) || iters < 1 || iters > NN_FD_MAX_ITERS || (mpart && Kp < 1)) return -2;
  hipLaunchKernelGGL(nn_fd_final_kernel, dim3(1), dim3(256), 0, st, tprev, tlast, nn_fd_parts(n), al, mpart,
                     (n + NN_MEAN_ROWS - 1) / NN_MEAN_ROWS, Kp, norm_b, tra, n, iters, out);
  return (int)hipGetLastError();
}
