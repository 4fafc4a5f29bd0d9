// C launchers of narrow2.hip (the 3-channel image layers without column matrices); included by
// bindings.cpp once per element-type suffix, like launchers.inc.
int DCG_API(dcg_nconv)(const elem_t* x, const elem_t* w, const float* bias, elem_t* y, int B, int H, int W, int Cin,
                       int Ho, int Wo, int pad_y, int pad_x, int act, float leak, int grid, const elem_t* bx,
                       const elem_t* by, const float* mean, const float* rstd, int bact, float bleak, float* part,
                       hipStream_t s);
int DCG_API(dcg_nconv_tiles)(int B, int Ho, int Wo);
int DCG_API(dcg_nwgrad_plan)(int H, int W, int Hd, int Wd, int* tyc, int* wrows, int* wcols);
int DCG_API(dcg_nwgrad)(const elem_t* x, int B, int H, int W, int Cin, const elem_t* d, int Hd, int Wd, int pl,
                        int chunks_per_wg, float* part, hipStream_t s);
// narrow.hip: the image gradient with the activation backward fused (+ per-workgroup column sums)
int DCG_API(dcg_narrow_deconv_dact)(const elem_t* x, const elem_t* w, elem_t* y, const elem_t* ya, int B, int Hi,
                                    int Wi, int C, int Ho, int Wo, int N, int pad, int act, float leak, float* part,
                                    hipStream_t s);
int DCG_API(dcg_narrow_deconv_tiles)(int B, int Ho, int Wo);
// wgrad3.hip: taps per tile of a wgrad3 cfg (2 for the two-tap tiles 320..339)
int DCG_API(dcg_wgrad3_taps_per_tile)(int cfg);
// misc.hip: the D head GEMV (+ the fused 3 losses of the objective) with the top BN layer's apply + activation fused
int DCG_API(dcg_gemv_head_bn)(const elem_t* x, const float* w, const float* b, float* out, int R, int K,
                              unsigned* counter, float* loss_out, float* dl_d, float* dl_g, float* prob,
                              const float* ls, const float* scale, const float* shift, int C, int rpg, int act,
                              float leak, elem_t* y, int objective, float real_target, hipStream_t s);
// narrow.hip: G's RGB layer forward with the lower layer's BN apply + activation fused into its staging
int DCG_API(dcg_narrow_deconv_bnin)(const elem_t* x, const elem_t* w, const float* bias, elem_t* y, int B, int Hi,
                                    int Wi, int C, int Ho, int Wo, int N, int pad, int act, float leak,
                                    const float* scale, const float* shift, int bn_act, float bn_leak, elem_t* a_out,
                                    hipStream_t s);
// bnfin.hip: one-level BN finalizes (forward + EMA, backward coefficients + dgamma / dbeta)
int DCG_API(dcg_bnfin_fwd)(const float* part, int ppg, int groups, int C, double count, const float* gamma,
                           const float* beta, float eps, float* mean, float* rstd, float* scale, float* shift,
                           float* ema_mean, float* ema_var, float decay, hipStream_t s);
int DCG_API(dcg_bnfin_bwd)(const float* part, int ppg, int groups, int C, float count, const float* gamma,
                           const float* mean, const float* rstd, float* dgamma, float* dbeta, float* coef,
                           hipStream_t s);
// misc.hip: the D head backward with row splits (more workgroups for the same bytes)
int DCG_API(dcg_head_bwd_rs)(const elem_t* x, const float* dl, const float* w, elem_t* dx, float* dW, float* db, int R,
                             int K, const elem_t* bx, const elem_t* by, const float* mean, const float* rstd, int C,
                             int rpg, int act, float leak, float* part, int RS, float* dw_ws, unsigned* dw_ctr,
                             hipStream_t s);
// wgrad5.hip: halo-row weight gradient (one kernel row of taps per workgroup, staged input window)
int DCG_API(dcg_wgrad5_tile)(int cfg, int* mc, int* bn, int* wd, int* ns);
int DCG_API(dcg_wgrad5_launch)(const dcg::WGrad3Args* a, int cfg, hipStream_t s);
