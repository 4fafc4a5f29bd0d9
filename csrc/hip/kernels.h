// Argument structs and host launchers of the gfx950 kernel library (csrc/hip/*.hip).
#pragma once
#include "common.h"

namespace dcg {

struct IGemmPhase {
  int Hq, Wq, M;            // row grid of this phase: m -> (b, qy, qx)
  int iy0_off, ix0_off;     // source pixel base: iy0 = qy * sstride + iy0_off
  int oy_off, ox_off;       // output pixel:      y   = qy * ostride + oy_off
  int ntaps;
  FastDiv fd_hw, fd_w;      // division by Hq*Wq and by Wq
  signed char dy[25], dx[25];
  short wtap[25];
  short pad_;
  int tap[25];              // packed (dy & 0xff) | (dx & 0xff) << 8 | wtap << 16 (igemm3: staged in LDS)
};

// Compact per-phase table passed BY VALUE in the kernel arguments (igemm3): uniform reads of it
// are scalar loads from the kernarg segment, instead of dependent vector loads from a device
// table (which cost ~1-2k cycles each in a workgroup's prologue / epilogue).
struct IGemmPhaseK {
  int Hq, Wq, M, iy0_off, ix0_off, oy_off, ox_off, ntaps;
  FastDiv fd_hw, fd_w;
  int tap[25];              // packed (dy & 0xff) | (dx & 0xff) << 8 | wtap << 16
};

struct IGemmArgs {
  const elem_t* A; int Bn, H, W, Kc, sstride, plain;
  const elem_t* Bw; int N;
  void* C; int out_f32, outH, outW, ldc, ostride, cofs;
  const float* bias; int act; float leak;
  float* stats;             // [mtiles * nphases][2][N] or nullptr
  int nphases, mtiles;
  uint32_t a_bytes, b_bytes;
  const IGemmPhase* ph;     // device table [nphases]
  // igemm3 only
  int kb_valid;             // B rows (k) that exist; larger k reads zeros (im2col'd K padding)
  int splits;               // split-K over workgroups (k tiles split evenly per phase)
  float* ws;                // [tiles][splits][BM*BN] fp32 slabs (splits > 1)
  unsigned* counters;       // [tiles] arrival counters, zero between launches
  int ablate;               // timing-only builds: bit0 drops A loads, bit1 drops B loads (0 = normal)
  unsigned long long* stamps;  // diagnostics: per-workgroup s_memtime at 4 points (nullptr = off)
  IGemmPhaseK phk[4];       // igemm3: the phase table by value
  // fused BN-backward statistics (epilogue of the data-gradient GEMM that produces dL/da for a
  // BN + activation layer): stats become (sum g, sum g*xhat), g = da * act'(y), xhat = (x-mean)*rstd,
  // instead of (sum v, sum v^2). x / y share C's layout. Tile group = tile row0 / bnb_rpg.
  const elem_t* bnb_x;
  const elem_t* bnb_y;
  const float* bnb_mean;    // [groups][N]
  const float* bnb_rstd;
  int bnb_rpg, bnb_act;
  float bnb_leak;
  // activation-only backward (layer without BN): store g = dL/da * act'(y) instead of dL/da and
  // emit (sum g, 0) per channel -- the bias gradient partials. bnb_x aliases y, mean/rstd unused.
  int bnb_store_g;
  // igemm3: longest phase first (mode 1: phases host-sorted by decreasing tap count, dispatched
  // phase by phase, each phase's tiles XCD-contiguous) instead of the phases interleaved
  int lpt;
  // igemm3: tile order with N slowest (each XCD's contiguous run of tiles shares weight columns)
  // instead of M slowest (shares activation rows); the host picks the smaller per-XCD footprint
  int nmajor;
};


struct WGradArgs {
  const elem_t* G; int Hg, Wg, Mc;     // gathered operand [B][Hg][Wg][Mc] (plain: [K][Mc])
  const elem_t* Dm; int Nc;            // direct operand [K][Nc]
  int K, plain, pl, ntaps;
  float* out;                        // [splits][ntaps][Mc][Nc]
  int kt_per_split;
  uint32_t g_bytes, d_bytes;
  FastDiv fd_hw, fd_w;               // of Hd*Wd, Wd (pixel decode of k)
  int Hd, Wd;
};

struct WGrad3Args {                 // wgrad3.hip: 25-tap gather GEMM, in-kernel split-K
  const elem_t* G; int Hg, Wg, Mc;     // gathered operand [B][Hg][Wg][Mc]
  const elem_t* Dm; int Nc;            // direct operand [K][Nc]
  int K, pl, splits, kt_per_split;
  uint32_t g_bytes, d_bytes;
  FastDiv fd_hw, fd_w;                 // of Hd*Wd, Wd (pixel decode of k)
  int Hd, Wd;
  float* out;                          // final fp32 gradient [25][Mc][Nc] (TF layout), scaled
  float scale;
  float* ws;                           // [tiles][splits][BM*BN] fp32 slabs (splits > 1)
  unsigned* counters;                  // [tiles] arrival counters, zero between launches
  int lhw, lw;                         // log2(Hd*Wd), log2(Wd) when both are powers of two, else -1
};

// grid cap of the streaming generator-EMA kernel (misc.hip ema_kernel): 256 CUs x 8 resident
// workgroups; larger buffers grid-stride
constexpr unsigned EMA_MAX_BLOCKS = 2048;

// grid cap of the D sub-step's one-launch update (misc.hip adam1_kernel): as adam2_kernel's ~512
// blocks, since every block bumps one arrival counter; larger buffers grid-stride
constexpr unsigned ADAM1_MAX_BLOCKS = 512;

// Learning-rate schedule of the Adam kernels (misc.hip dcg::lr_factor), by value in the kernel
// arguments: the factor f(t) of the DEVICE step counter t that multiplies lr (one fp32 multiply)
// ahead of the bias correction, so graph replays follow the live counter.
//   k = t <= start ? 0 : min(t - start, steps),  p = float(k) / float(steps)
//   linear 1 - (1 - end) p | cosine 1 - (1 - end) (1 - cos(pi p)) / 2 | exponential end^p
//   k == 0 -> 1 and k == steps -> end by selection;  t < warmup: f *= float(t + 1) / float(warmup)
// LR_NONE with warmup == 0 is "off": the counter is never read and lr is used as it is.
enum LrKind : int { LR_NONE = 0, LR_LINEAR = 1, LR_COSINE = 2, LR_EXPONENTIAL = 3 };
constexpr unsigned LR_MAX_STEPS = 1u << 24;  // steps and warmup: exact as fp32

struct LrSched {
  int kind;
  unsigned steps, warmup;
  float end;
  unsigned long long start;
};

__host__ __device__ static inline bool lr_sched_on(const LrSched& s) { return s.kind != LR_NONE || s.warmup != 0; }

// Instance noise on D's input (misc.hip instance_noise_kernel), by value in the kernel arguments:
// sigma(t) of the DEVICE step counter t, so graph replays follow the live counter.
//   sigma(t) = s1 if s0 == s1 or t >= steps, else fma(s1 - s0, float(t) / float(steps), s0)
// The noise draws from Philox stream NOISE_STREAM of the step's z seed (z itself from stream 0).
constexpr unsigned NOISE_MAX_STEPS = 1u << 24;  // exact as fp32
constexpr float NOISE_MAX_SIGMA = 2.f;
constexpr unsigned NOISE_MAX_BLOCKS = 2048;     // grid cap (256 CUs x 8 resident workgroups); grid-stride beyond
constexpr unsigned long long NOISE_STREAM = 1;

struct NoiseSched {
  float s0, s1;
  unsigned steps;
};

// DiffAugment on D's input (misc.hip d_augment_kernel): a policy bitmask over the two geometric
// transforms. Sample n draws the 4 words of ONE Philox block, counter (n, step, AUG_STREAM), of the
// step's z seed: (ty, tx, oy, ox), always all four; the mask selects which of them apply.
enum AugPolicy : int { AUG_TRANSLATION = 1, AUG_CUTOUT = 2, AUG_ALL = 3 };
constexpr unsigned long long AUG_STREAM = 2;
constexpr int AUG_MAX_SIZE = 1 << 14;  // S: keeps every index of one image inside 32 bits

// DiffAugment's color policy on D's input (misc.hip d_color_kernel): a bitmask of its own over the three
// pointwise transforms, applied in this order ahead of AugPolicy's. Sample n draws words w0..w2 of
// ONE Philox block, counter (n, step, COLOR_STREAM), of the step's z seed: (b, s, c), always all three.
enum ColorPolicy : int { COLOR_BRIGHTNESS = 1, COLOR_SATURATION = 2, COLOR_CONTRAST = 4, COLOR_ALL = 7 };
constexpr unsigned long long COLOR_STREAM = 3;

// Adaptive augmentation probability (ADA, Karras et al. 2020) for the two policies above: each selected
// transform applies to a sample with probability p = p24 * 2^-24, p24 an integer in [0, 2^24] that lives
// in word 0 of a device state int32 [8] = (p24, acc, cnt, r_acc, windows, 0, 0, 0). The gated kernel
// instances draw one more Philox block per sample -- AUG_GATE_STREAM: w0 translation, w1 cutout;
// COLOR_GATE_STREAM: w0 brightness, w1 saturation, w2 contrast -- and policy bit i is on iff (w_i >> 8)
// < p24; they record the effective policy per sample for the transposes. misc.hip ada_update_kernel
// steers p24 once per step from the real logits x_0..x_{B-1}:
//   acc += sum_i ((x_i > thr) - (x_i < thr));  cnt += 1
//   cnt == interval:  p24 = clamp(p24 + ((acc > Tn) - (acc < Tn)) * delta24, 0, 2^24);
//                     r_acc = acc; windows += 1; acc = cnt = 0
constexpr unsigned long long AUG_GATE_STREAM = 4;
constexpr unsigned long long COLOR_GATE_STREAM = 5;
constexpr int ADA_ONE = 1 << 24;
constexpr int ADA_MAX_INTERVAL = 1 << 16;
constexpr int ADA_STATE_WORDS = 8;

// GAN objectives of the loss / head kernels (misc.hip gan_loss_block). The first three are the
// ids of the launchers and bindings; GAN_BCE_T is the kernel instance of bce with a smoothed
// real target, which the launchers pick themselves (real_target != 1).
enum GanObjective : int { GAN_BCE = 0, GAN_LSGAN = 1, GAN_HINGE = 2, GAN_BCE_T = 3 };

// Top-k generator updates (misc.hip g_topk_kernel), by value in the kernel arguments: G's seed keeps
// the k(t) highest-scored of the B fakes, k annealed from B to kmin over the DEVICE step counter t, so
// graph replays follow the live counter.
//   k(t) = B - ((B - kmin) * min(t, steps)) / steps      (integer arithmetic: exact, stateless)
constexpr int TOPK_MAX_B = 4096;               // the keys of one batch in LDS: 16 KB
constexpr unsigned TOPK_MAX_STEPS = 1u << 24;

struct TopkSched {
  unsigned kmin, steps;
};

// ---- spectral normalisation of D's weights (specnorm.hip). One descriptor per normalised
// weight, viewed as W [K, Cout] row-major (TF's reshape(w, [-1, Cout]); the head is [K, 1]); a table
// of up to SN_MAX_MATS of them rides in the kernel arguments so one grid covers them all.
constexpr int SN_MAX_MATS = 8;
constexpr int SN_MAX_ROW_BLOCKS = 256;        // row blocks per matrix (power step, launches 1 and 2)
constexpr int SN_MAX_ROWS_PER_BLOCK = 1024;   // v rows a block stages in LDS -> K <= 262144
constexpr int SN_MAX_STREAM_BLOCKS = 512;     // streaming blocks per matrix (copy write, dot, project)
constexpr int SN_MAX_COL_TILES = 64;          // 256-column tiles -> Cout <= 16384
// workspace layout (floats): [tpart 256 | spart 64 | dpart 512 | cpart nrb * Cout]
constexpr int SN_WS_TPART = 0, SN_WS_SPART = 256, SN_WS_DPART = 320, SN_WS_CPART = 832;

struct SNMat {
  const float* W;   // fp32 master [K, Cout]
  float* u;         // [Cout]
  float* v;         // [K]
  float* sigma;     // [1]
  float* ws;        // workspace, sn_plan().ws_floats floats
  void* hat;        // normalised copy W / sigma: elem_t [K * Cout] (mirror slice), or float (hat_f32)
  float* grad;      // dL/d(W / sigma) -> dL/dW in place (projection only)
  int K, Cout;
  int nrb, rpb;     // row blocks, rows per block
  int nct;          // 256-column tiles
  int ncb;          // streaming blocks
  int hat_f32;
};

struct SNTable {
  int n;
  SNMat m[SN_MAX_MATS];
};

struct SNPlan {
  int nrb, rpb, nct, ncb;
  size_t ws_floats;
};

// block counts and workspace size of a [K, Cout] matrix; nrb = 0: shape out of range
static inline SNPlan sn_plan(long K, long Cout) {
  SNPlan p = {0, 0, 0, 0, 0};
  if (K <= 0 || Cout <= 0 || Cout > 256L * SN_MAX_COL_TILES ||
      K > (long)SN_MAX_ROW_BLOCKS * SN_MAX_ROWS_PER_BLOCK || K * Cout >= (1L << 31))
    return p;
  long nrb = (K + 7) / 8;
  if (nrb > SN_MAX_ROW_BLOCKS) nrb = SN_MAX_ROW_BLOCKS;
  p.rpb = (int)((K + nrb - 1) / nrb);
  p.nrb = (int)((K + p.rpb - 1) / p.rpb);
  p.nct = (int)((Cout + 255) / 256);
  long ncb = (K * Cout + 4095) / 4096;  // 4 float4 per thread
  p.ncb = (int)(ncb < 1 ? 1 : ncb > SN_MAX_STREAM_BLOCKS ? SN_MAX_STREAM_BLOCKS : ncb);
  p.ws_floats = (size_t)SN_WS_CPART + (size_t)p.nrb * (size_t)Cout;
  return p;
}

}  // namespace dcg

extern "C" {
#include "launchers.inc"
}
