// 1- and k-nearest-neighbour search between two sets of feature rows (nn.hip): limits and host launchers. Everything
// is fp32 whatever the engine's element type, so the file is built once and its launchers carry no suffix.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int NN_TILE = 128;        // rows and columns of G = X Y^T that one workgroup owns at a time
constexpr int NN_BK = 32;           // k depth of one LDS stage
constexpr int NN_PITCH = NN_BK + 4; // floats between LDS rows: 36 r mod 64 is distinct for 16 rows (see nn.hip)
constexpr int NN_MEAN_ROWS = 64;    // rows per fp64 partial sum of the mean
constexpr int NN_FEAT_ROWS = 4;     // rows per workgroup of nn_features
constexpr int NN_MAX_ROWS = 1 << 20;
constexpr int NN_MAX_K = 1 << 20;
constexpr int NN_MAX_KNN = 16;      // neighbours per row of nn_topk: one per lane of the 16 that share a row

// K padded with zeros to the k depth of four 16x16x4 MFMAs
static inline int nn_kpad(int K) { return (K + 15) & ~15; }
static inline int nn_col_tiles(int My) { return (My + NN_TILE - 1) / NN_TILE; }
// workgroups of nn_mmd: the 128 x 128 tiles (I, J), I <= J, of the upper triangle of the Gram of Mx + My stacked rows,
// with skip_aa from the first tile column that holds a row past Mx (at least one: My >= 1 then)
static inline int nn_mmd_pairs(int Mx, int My, int skip_aa) {
  const int T = nn_col_tiles(Mx + My), J0 = skip_aa ? Mx / NN_TILE : 0;
  return T * (T + 1) / 2 - J0 * (J0 + 1) / 2;
}
// The Frechet distance's square matrices [n][nn_fd_ld(n)]: a row is padded with zeros to a multiple of 16 columns, so
// that it serves as the k range of a GEMM. Below NN_FD_SMALL rows the tiles are 64 x 64, so that a launch fills the device
constexpr int NN_FD_MAX_ROWS = 8192;
constexpr int NN_FD_MAX_ITERS = 256;
constexpr int NN_FD_SMALL = 2048;
static inline int nn_fd_ld(int n) { return (n + 15) & ~15; }
static inline int nn_fd_tile(int n) { return n < NN_FD_SMALL ? 64 : NN_TILE; }
static inline int nn_fd_parts(int n) { return (n + 3) / 4; }  // fp64 partials of nn_fd_trace: one per 4 rows
// workgroups of P = X X^T (the tiles of the upper triangle) and of the step X' = 1.5 X - 0.5 P X
static inline int nn_fd_ppt_groups(int n) { const int T = (n + nn_fd_tile(n) - 1) / nn_fd_tile(n); return T * (T + 1) / 2; }
static inline int nn_fd_step_groups(int n) { const int T = (n + nn_fd_tile(n) - 1) / nn_fd_tile(n); return T * T; }
// fp64 partials of the mean: [ceil(n / NN_MEAN_ROWS)][K]
static inline size_t nn_mean_part_bytes(int n, int K) {
  return (size_t)((n + NN_MEAN_ROWS - 1) / NN_MEAN_ROWS) * (size_t)K * sizeof(double);
}

extern "C" {
// Every launcher: -2 = an argument out of range (null pointer, size, alignment)
// x [n][K] -> F [n][Kp] = x - mu (zeros from K on), norm [n] = |F_i|^2. mu [K] may be null (no centring). With
// compute_mu, mu is first set to the mean over the n rows: fp64 partials `part` per 64 rows, added in index order
int dcg_nn_features(const float* x, int n, int K, float* mu, double* part, int compute_mu, float* F, float* norm,
                    hipStream_t st);
// part [splits][Mx] = per row i of X and column chunk c the smallest (key(d) << 32 | j), d = nx_i + ny_j - 2 x_i.y_j
// over the columns j of the chunk (j != i with loo). X [Mx][Kp], Y [My][Kp], Kp a multiple of 16, 16-byte aligned
int dcg_nn_top1(const float* X, const float* nx, const float* Y, const float* ny, uint64_t* part, int Mx, int My, int Kp,
                int loo, int splits, hipStream_t st);
// idx [Mx] = the column of the smallest of part [splits][Mx] over the chunks, in chunk order
int dcg_nn_merge(const uint64_t* part, int* idx, int Mx, int splits, hipStream_t st);
// dist [Mx] = sum_k (x0[i][k] - y0[idx[i]][k])^2 from the uncentred rows: fp32 differences and squares, fp64 sums
int dcg_nn_refine(const float* x0, const float* y0, const int* idx, double* dist, int Mx, int My, int K, hipStream_t st);
// part [splits][Mx][k] = per row and column chunk the k smallest keys of dcg_nn_top1's kind, ascending, ~0 where the
// chunk has fewer than k columns. 1 <= k <= NN_MAX_KNN, k <= My (My - 1 with loo); bitwise independent of splits
int dcg_nn_topk(const float* X, const float* nx, const float* Y, const float* ny, uint64_t* part, int Mx, int My, int Kp,
                int loo, int splits, int k, hipStream_t st);
// idx [Mx][k] = the columns of the k smallest of part [splits][Mx][k] over the chunks, ascending by key; -1: none
int dcg_nn_merge_k(const uint64_t* part, int* idx, int Mx, int splits, int k, hipStream_t st);
// dist [Mx][k] = dcg_nn_refine's distance of every candidate idx [Mx][k]; rad [Mx] = the fp32 value of the row's largest
int dcg_nn_radius(const float* x0, const float* y0, const int* idx, double* dist, float* rad, int Mx, int My, int K, int k,
                  hipStream_t st);
// cnt [Mx] = #{j < My : nx_i + ny_j - 2 x_i.y_j <= rad_j}, through the chunks' counts part int [splits][Mx] in chunk order
int dcg_nn_count(const float* X, const float* nx, const float* Y, const float* ny, const float* rad, int* part, int* cnt,
                 int Mx, int My, int Kp, int splits, hipStream_t st);
// The kernel MMD (a mixture of 5 Gaussians, 2 sigma^2 = 4h .. h/4). bw float [2] = {h, c}: h = 2 / (n - 1) * sum_i
// norm_i, the mean squared distance between two of the n centred rows whose squared norms are norm; c = log2(e) / (4 h)
int dcg_nn_mmd_bw(const float* norm, int n, float* bw, hipStream_t st);
// part double [nn_mmd_pairs(Mx, My, skip_aa)][3]: per tile pair of the upper triangle of the Gram of Z = [X; Y] and
// per class (row >= Mx) + (col >= Mx) the sum over row < col of sum_m exp2(-2^m d c), m = 0..4, c = bw [1]. My = 0:
// X alone (Y, ny may be null). skip_aa: no pair of two rows of X, and no tile that holds only such pairs
int dcg_nn_mmd(const float* X, const float* nx, const float* Y, const float* ny, const float* bw, double* part, int Mx,
               int My, int Kp, int skip_aa, hipStream_t st);
// out double [8] = {S_AA, S_BB, S_AB, k_rr, k_ff, k_rf, mmd2, h} from part in a fixed order, the sums with the
// mixture's 1/5. With skip_aa, S_AA is *saa (null: 0); a mean over no pair is 0
int dcg_nn_mmd_final(const double* part, int pairs, const double* saa, int skip_aa, int Mx, int My, const float* bw,
                     double* out, hipStream_t st);
// The Frechet distance through the polar iteration (nn.hip). 2 <= n <= NN_FD_MAX_ROWS; C, X, Xn, P are [n][nn_fd_ld(n)]
// C = FA FB^T / (n - 1), FA and FB [n][Kp]
int dcg_nn_fd_gram(const float* FA, const float* FB, float* C, int n, int Kp, hipStream_t st);
// center: C <- C - rowmean(C) in place. al double [2] = {alpha, 1 / alpha}, alpha = sqrt(max_i sum_j |c_ij| * max_j
// sum_i |c_ij|); X = C / alpha. Workspaces: rmean, rabs double [n], cpart double [ceil(n / NN_MEAN_ROWS)][n]
int dcg_nn_fd_scale(float* C, int n, int center, double* rmean, double* rabs, double* cpart, double* al, float* X,
                    hipStream_t st);
// P = X X^T, over the tiles of the upper triangle, each stored to both halves
int dcg_nn_fd_ppt(const float* X, float* P, int n, hipStream_t st);
// Xn = 1.5 X - 0.5 P X; Xn is neither X nor P
int dcg_nn_fd_step(const float* P, const float* X, float* Xn, int n, hipStream_t st);
// part double [nn_fd_parts(n)]: sum_ij X_ij C_ij per 4 rows
int dcg_nn_fd_trace(const float* X, const float* C, int n, double* part, hipStream_t st);
// out double [1] = sum_i norm_i / (n - 1)
int dcg_nn_fd_tr(const float* norm, int n, double* out, hipStream_t st);
// mpart double [ceil(n / NN_MEAN_ROWS)][Kp]: the column sums of FB per 64 rows
int dcg_nn_fd_mean(const float* FB, int n, int Kp, double* mpart, hipStream_t st);
// out double [8] = {fd, mean2, tr_a, tr_b, nuc, tail, alpha, iters} from the traces of the last two iterates; mpart,
// norm_b and tra may be null (their terms are then 0: the nuclear norm of a bare C)
int dcg_nn_fd_final(const double* tprev, const double* tlast, const double* al, const double* mpart, int Kp,
                    const float* norm_b, const double* tra, int n, int iters, double* out, hipStream_t st);
}
