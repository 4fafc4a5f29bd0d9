// Sliced Wasserstein distance between Laplacian-pyramid patch descriptors (swd.hip): limits and host
// launchers. Everything is fp32 whatever the engine's element type, so the file is built once and its
// launchers carry no element-type suffix.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr unsigned long long SWD_STREAM = 6;      // Philox stream of the patch centres (0..5 are taken)
constexpr int SWD_MIN_ROWS = 16, SWD_MAX_ROWS = 32768;  // N: descriptors per set and level (a power of two)
constexpr int SWD_FUSED_ROWS = 16384;             // up to here two columns share the sort's LDS
constexpr int SWD_GLOBAL_MAX_ROWS = 1 << 21;      // N of the global merge sort: above SWD_MAX_ROWS, a power of two
constexpr int SWD_CHUNK_ROWS = 16384;             // its LDS-sorted runs: 64 KB, two workgroups per CU
constexpr int SWD_MERGE_TILE = 4096;              // output keys per workgroup of a merge pass (256 threads x 16)
constexpr int SWD_MAX_CH = 4;                     // channels
constexpr int SWD_MAX_DIRS = 1024;                // J = repeats * dirs (a multiple of 128)
constexpr int SWD_STAT_ROWS = 256;                // descriptors per block of the statistics' first pass
constexpr int SWD_BAND_LDS = 64 * 1024;           // the pyramid kernels' row band in LDS (bytes)

// floats of one staged image row of the pyramid kernels: the row's s * C values from a 16-byte boundary,
// `halo` pixels in front of it and behind; 0: the band does not fit
static inline int swd_row_floats(int s, int C, int halo) {
  const int body = (halo * C + 3) & ~3;
  return (body + (s + halo) * C + 3) & ~3;
}
// K = 49 C padded with zeros to the k depth of four 16x16x4 MFMAs
static inline int swd_kpad(int C) { return (49 * C + 15) & ~15; }

extern "C" {
// Every launcher: -2 = an argument out of range (null pointer, size, alignment)
// g [n][s][s][C] -> out [n][s/2][s/2][C]: 5x5 binomial filter at every second pixel, reflect-101 borders
int dcg_swd_down(const float* g, float* out, int n, int s, int C, hipStream_t st);
// l = g - up(gn): g, l [n][s][s][C], gn [n][s/2][s/2][C]; the upsampled image stays in registers
int dcg_swd_laplace(const float* g, const float* gn, float* l, int n, int s, int C, hipStream_t st);
// cen int32 [n * P][2] = (cy, cx) of level `level` at size s
int dcg_swd_centres(int* cen, int n, int P, int s, int level, uint64_t seed, hipStream_t st);
// per-channel (mean, std) of the sampled 7x7 windows of l: part double [ceil(N / 256)][C][2], stats float [2][C]
int dcg_swd_stats(const float* l, const int* cen, int n, int P, int s, int C, double* part, float* stats,
                  hipStream_t st);
// theta [J][K] (any length) -> thetap [J][Kp] = theta / |theta| / std_c(k), zeros from K on; bias [J]
int dcg_swd_prepare(const float* theta, const float* stats, float* thetap, float* bias, int J, int C, hipStream_t st);
// proj [J][N] = windows of l x thetap^T + bias
int dcg_swd_project(const float* l, const int* cen, const float* thetap, const float* bias, float* proj, int n, int P,
                    int s, int C, int J, hipStream_t st);
// per direction j: sort src0[j] -> dst0[j] (dst0 may be null); with src1 (N <= 16384) also src1[j] -> dst1[j];
// partial[j] = sum_i |sorted0[i] - other[i]|, other = sorted1, else the sorted column ref[j] (partial may be null)
int dcg_swd_sort_distance(const float* src0, float* dst0, const float* src1, float* dst1, const float* ref,
                          double* partial, int N, int J, hipStream_t st);
// The same for N in (32768, 2^21]: runs of SWD_CHUNK_ROWS sorted in LDS, then log2(N / SWD_CHUNK_ROWS) merge-path
// passes between the key buffers keys0, keys1 uint32 [J][N]. src[j] sorted -> dst[j] (dst may be null); with the
// sorted columns `other` [J][N]: partial[j] = sum_i |sorted[i] - other[j][i]| through tilepart double
// [J][N / SWD_MERGE_TILE] (other, tilepart and partial are given together or not at all). Buffers 16-byte aligned
int dcg_swd_sort_large(const float* src, float* dst, const float* other, uint32_t* keys0, uint32_t* keys1,
                       double* tilepart, double* partial, int N, int J, hipStream_t st);
// out[0] = 1000 * sum_j partial[j] / (J * N), the partials added in index order
int dcg_swd_mean(const double* partial, double* out, int N, int J, hipStream_t st);
}
