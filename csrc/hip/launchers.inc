// C launchers of the kernel library; DCG_API(name) = name (bf16 build), name##_f16 (fp16 build)
// or name##_f32 (fp32 build). Included by kernels.h, and again by bindings.cpp for the _f16 and
// _f32 sets.
int DCG_API(dcg_igemm_tile)(int cfg, int* bm, int* bn);
int DCG_API(dcg_igemm_launch)(const dcg::IGemmArgs* a, int cfg, int mtiles, int ntiles, hipStream_t s);
int DCG_API(dcg_igemm3_tile)(int cfg, int* bm, int* bn, int* ns);
int DCG_API(dcg_igemm3_launch)(const dcg::IGemmArgs* a, int cfg, int bkn, unsigned blocks, hipStream_t s);
int DCG_API(dcg_igemm3_threads)(int cfg);
int DCG_API(dcg_wgrad_tile)(int cfg, int* bm, int* bn);
int DCG_API(dcg_wgrad_launch)(const dcg::WGradArgs* a, int cfg, int splits, hipStream_t s);
int DCG_API(dcg_wgrad3_tile)(int cfg, int* bm, int* bn, int* ns);
int DCG_API(dcg_wgrad3_launch)(const dcg::WGrad3Args* a, int cfg, hipStream_t s);
int DCG_API(dcg_splitk_reduce)(const float* src, int splits, size_t n, float* dst, float scale, hipStream_t s);

int DCG_API(dcg_colstats)(int mode, const elem_t* x, const elem_t* dy, const elem_t* y, const float* mean, const float* rstd,
                 int act, float leak, int R, int C, int rows_per_block, int rows_per_group, float* part,
                 hipStream_t s);
int DCG_API(dcg_bn_finalize)(const float* part, int ppg, int groups, int C, double count, const float* gamma,
                    const float* beta, float eps, float* mean, float* rstd, float* scale, float* shift,
                    float* ema_mean, float* ema_var, float decay, hipStream_t s);
int DCG_API(dcg_bn_coef_eval)(int C, const float* gamma, const float* beta, float eps, const float* mean, const float* var,
                     float debias, const float* debias_ptr, float* scale, float* shift, hipStream_t s);
int DCG_API(dcg_bn_apply_act)(const elem_t* x, elem_t* y, const float* scale, const float* shift, int R, int C,
                     int rows_per_group, int act, float leak, hipStream_t s);
int DCG_API(dcg_bn_bwd_finalize)(const float* part, int ppg, int groups, int C, float count, const float* gamma,
                        const float* mean, const float* rstd, float* dgamma, float* dbeta, float* coef,
                        hipStream_t s);
int DCG_API(dcg_bn_bwd_apply)(const elem_t* dy, const elem_t* y, const elem_t* x, const float* coef, elem_t* dx, int R, int C,
                     int rows_per_group, int act, float leak, hipStream_t s);
int DCG_API(dcg_act_bwd)(const elem_t* dy, const elem_t* y, elem_t* dx, size_t n, int act, float leak, hipStream_t s);
int DCG_API(dcg_sum_partials)(const float* part, int P, int stride, int C, float* dst, hipStream_t s);
int DCG_API(dcg_act_bwd_dbias)(const elem_t* dy, const elem_t* y, elem_t* dx, int R, int C, int act, float leak,
                               float* part, int max_blocks, unsigned* counter, float* db, hipStream_t s);
int DCG_API(dcg_head_bwd)(const elem_t* x, const float* dl, const float* w, elem_t* dx, float* dW, float* db, int R,
                          int K, const elem_t* bx, const elem_t* by, const float* mean, const float* rstd, int C,
                          int rpg, int act, float leak, float* part, hipStream_t s);
int DCG_API(dcg_colsum_small)(const elem_t* x, int R, int C, float* part, int blocks, hipStream_t s);

// objective = GAN_BCE | GAN_LSGAN | GAN_HINGE, real_target = 1 - label_smooth (1 for hinge); -2 otherwise
int DCG_API(dcg_gan_loss)(const float* logits, int B, float* out, float* dl_d, float* dl_g, float* prob,
                          const float* ls, int objective, float real_target, hipStream_t s);
// top-k generator updates over the fake half of the logits x[B] and the all-sample seed dl_g[B]: dl_g_k[B],
// sel int32[B], info float[4] = (g_loss_topk, threshold, B / k, k), k = k(*step) of `sched`; its probe: k at
// each of n step values. -2: a null pointer, B outside 1..TOPK_MAX_B, kmin outside 1..B, steps outside
// 1..2^24, an objective other than GAN_BCE | GAN_LSGAN | GAN_HINGE
int DCG_API(dcg_g_topk)(const float* x, const float* dl_g, float* dl_g_k, int* sel, float* info, int B,
                        const dcg::TopkSched* sched, const unsigned long long* step, int objective, hipStream_t s);
int DCG_API(dcg_topk_k)(const unsigned long long* steps, int* out, size_t n, int B, const dcg::TopkSched* sched,
                        hipStream_t s);
int DCG_API(dcg_linear_fwd)(float* z, const float* W, const float* b, elem_t* out, int B, int K, int N, float* stats,
                            int C, const unsigned long long* gen_step, uint64_t gen_seed, hipStream_t s);
int DCG_API(dcg_linear_wgrad)(const float* z, const elem_t* dh, float* dW, float* db, int B, int K, int N, hipStream_t s);
int DCG_API(dcg_gemv_head)(const elem_t* x, const float* w, const float* b, float* out, int R, int K, unsigned* counter,
                           float* loss_out, float* dl_d, float* dl_g, float* prob, const float* ls, int objective,
                           float real_target, hipStream_t s);
int DCG_API(dcg_head_dgrad)(const float* dl, const float* w, elem_t* dx, int R, int K, hipStream_t s);
int DCG_API(dcg_head_wgrad)(const elem_t* x, const float* dl, float* part, int R, int K, int splits, hipStream_t s);
int DCG_API(dcg_sum_vec)(const float* v, int n, float* out, hipStream_t s);
int DCG_API(dcg_adam)(float* w, elem_t* wbf, const float* g, float* m, float* v, const float* powers, size_t n,
                      float lr, float b1, float b2, float eps, float gscale, const float* ls,
                     const void* g_bf16, const dcg::LrSched* sched, const unsigned long long* step, hipStream_t s);
int DCG_API(dcg_step_end)(float* pd, float* pg, float b1d, float b2d, float b1g, float b2g,
                          unsigned long long* step, float* ls, int growth_interval, hipStream_t s);
// the D-only sub-step's update: one-launch Adam + mirror + powers of one set
int DCG_API(dcg_adam1)(float* w, elem_t* wbf, const float* g, float* m, float* v, float* powers, size_t n, float lr,
                       float b1, float b2, float eps, float gscale, unsigned* counter, const dcg::LrSched* sched,
                       const unsigned long long* step, hipStream_t s);
int DCG_API(dcg_ema)(float* s, elem_t* sbf, const float* w, size_t n, float decay, const unsigned long long* step,
                     int step_bias, const float* ls, hipStream_t st);
// spectral normalisation (specnorm.hip): power step = wu, wtv, colsum, apply(from_state = 0);
// apply(from_state = 1) rewrites the normalised copies from the stored sigma; projection = dot, project
int DCG_API(dcg_sn_wu)(const dcg::SNTable* t, const float* ls, hipStream_t s);
int DCG_API(dcg_sn_wtv)(const dcg::SNTable* t, const float* ls, hipStream_t s);
int DCG_API(dcg_sn_colsum)(const dcg::SNTable* t, const float* ls, hipStream_t s);
int DCG_API(dcg_sn_apply)(const dcg::SNTable* t, int from_state, const float* ls, hipStream_t s);
int DCG_API(dcg_sn_dot)(const dcg::SNTable* t, hipStream_t s);
int DCG_API(dcg_sn_project)(const dcg::SNTable* t, hipStream_t s);
int DCG_API(dcg_nonfinite_check)(const float* g, size_t n, float* ls, hipStream_t s);
int DCG_API(dcg_pack)(const float* src, int T, int A, int Bd, elem_t* nat, elem_t* tr, int st, int sb, int sa, hipStream_t s);
int DCG_API(dcg_philox_uniform)(float* out, size_t n, uint64_t seed, const unsigned long long* step, uint64_t stream_id,
                       float lo, float hi, hipStream_t s);
// instance noise: y = x + sigma(*step) * eps over n elements (eps: Box-Muller normals of the Philox
// stream (seed, *step, stream_id)); its probes: the fp32 normals, sigma at each of n step values.
// -2: a null pointer
int DCG_API(dcg_instance_noise)(const elem_t* x, elem_t* y, size_t n, uint64_t seed, const unsigned long long* step,
                                uint64_t stream_id, const dcg::NoiseSched* sched, hipStream_t s);
int DCG_API(dcg_philox_normal)(float* out, size_t n, uint64_t seed, const unsigned long long* step, uint64_t stream_id,
                               hipStream_t s);
int DCG_API(dcg_noise_sigma)(const unsigned long long* steps, float* out, size_t n, const dcg::NoiseSched* sched,
                             hipStream_t s);
// DiffAugment (translation / cutout, kernels.h AugPolicy) of x [N][S][S][C] into y, params int32 [N][4]
// = (ty, tx, oy, ox). mode 0: drawn from the Philox stream (seed, *step, AUG_STREAM) and written to
// params; 1: read from params; 2: the transposed gather (backward) of the rows in params.
// DiffAugment's color policy (brightness / saturation / contrast, kernels.h ColorPolicy) of x [N][S][S][C]
// into y, params float [N][4] = (b, s, c, Mx). mode 0: (b, s, c) drawn from the Philox stream (seed, *step,
// COLOR_STREAM), all four written; 1: (b, s, c) read from params, Mx written; 2: the transpose (backward)
// under (s, c) of params, which it only reads.
// Both with adaptive gates (kernels.h ADA): gates int32 [N], the effective policy per sample, written in mode
// 0 from the Philox gate streams and p24 = ada[0], read in modes 1 and 2 (ada unused). gates == nullptr: the
// ungated kernels.
// -2: a null pointer, x == y, N < 1, S outside 1..2^14, C outside 1..4, an empty or unknown policy / mode,
// gates in mode 0 without ada, ada without gates
int DCG_API(dcg_d_augment)(const elem_t* x, elem_t* y, int* params, int N, int S, int C, int policy, int mode,
                           uint64_t seed, const unsigned long long* step, int* gates, const int* ada, hipStream_t s);
int DCG_API(dcg_d_color)(const elem_t* x, elem_t* y, float* params, int N, int S, int C, int policy, int mode,
                         uint64_t seed, const unsigned long long* step, int* gates, const int* ada, hipStream_t s);
// one step of the ADA controller on state int32 [8] from the B real logits (fp32). -2: a null pointer, B < 1,
// interval outside 1..2^16, B * interval >= 2^31, delta24 outside 1..2^24, |target_n| > B * interval, thr NaN
int DCG_API(dcg_ada_update)(const float* logits, int B, int* state, float thr, int target_n, int delta24,
                            int interval, hipStream_t s);
int DCG_API(dcg_im2col_s2)(const elem_t* src, elem_t* dst, int B, int H, int W, int C, int Ho, int Wo, int pl_y, int pl_x,
                  int Kpad, hipStream_t s);
int DCG_API(dcg_cast_to_bf16)(const void* src, int src_dtype, elem_t* dst, size_t n, float scale, float shift, hipStream_t s);
int DCG_API(dcg_cast_bf16_f32)(const elem_t* src, float* dst, size_t n, hipStream_t s);
int DCG_API(dcg_narrow_deconv)(const elem_t* x, const elem_t* w, const float* bias, elem_t* y, int B, int Hi, int Wi,
                              int C, int Ho, int Wo, int N, int pad, int act, float leak, hipStream_t s);
int DCG_API(dcg_bn_finalize_split)(const float* part, int ppg, int groups, int C, double count, const float* gamma,
                                  const float* beta, float eps, float* mean, float* rstd, float* scale, float* shift,
                                  float* ema_mean, float* ema_var, float decay, double* ws, unsigned* counters, int PS,
                                  hipStream_t s);
int DCG_API(dcg_bn_bwd_finalize_split)(const float* part, int ppg, int groups, int C, float count, const float* gamma,
                                      const float* mean, const float* rstd, float* dgamma, float* dbeta, float* coef,
                                      double* ws, unsigned* counters, int PS, hipStream_t s);
int DCG_API(dcg_sum_partials_split)(const float* part, int P, int stride, int C, float* dst, float* ws,
                                    unsigned* counters, int PS, hipStream_t s);
int DCG_API(dcg_adam2)(float* wA, elem_t* wbfA, const float* gA, float* mA, float* vA, float* pA, size_t nA, float lrA,
                       float b1A, float b2A, float epsA, float* wD, elem_t* wbfD, const float* gD, float* mD,
                       float* vD, float* pD, size_t nD, float lrD, float b1D, float b2D, float epsD, float gscale,
                       unsigned long long* step, unsigned* counter, const dcg::LrSched* sched, hipStream_t s);
// the schedule's factor at each of n step values (the device function the Adam kernels call);
// sched == nullptr = off; -2: an active schedule with a null step pointer (all four launchers)
int DCG_API(dcg_lr_factor)(const unsigned long long* steps, float* out, size_t n, const dcg::LrSched* sched,
                           hipStream_t s);
int DCG_API(dcg_tensor_summary)(const void* x, int x_dtype, size_t n, const double* edges, int nbins, double* out,
                                double* part, unsigned* counter, int blocks, hipStream_t s);
