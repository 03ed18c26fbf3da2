/*
 * include/rwkv7_hip.h -- C ABI of librwkv7_hip.so: the MI355X (gfx950) RWKV-7 time-mix hot path.
 *
 * This is the drop-in boundary.  Every entry point takes plain device pointers, sizes and a HIP
 * stream; nothing here knows about torch.  The caller owns ALL memory including outputs and scratch
 * (as in the reference: y/s/sa/grads are torch.empty_like'd by the Python wrapper,
 * model/llm/rwkv_s2s_single_ffn.py:22-24,33) and the ops mutate in place and return an int:
 *      0   success
 *     <0   argument error (RWKV7_E*)          -- nothing was launched
 *     >0   hipError_t from the launch          -- hipGetLastError() after the launch
 * Kernels are stream-ordered, re-entrant and keep no global state, so they may be called from
 * several host threads on different streams (service/tts_service.py:42-60 runs one thread per engine).
 *
 * Tensor conventions (reference: model/llm/cuda/wkv7_cuda.cu:18, rwkv7_state_fwd_fp16.cu:16,27):
 *   w,q,k,v,a,b,y,dy,d*  [B,T,H,64] contiguous  == [B,T,C] with C = H*64
 *   w is the PRE-activation: the decay used is exp(-exp(w))            (wkv7_cuda.cu:21)
 *   s   fp32 [B,H,T/16,64,64], checkpoint of the state after every 16th step, stored TRANSPOSED
 *       (s[..., j, i] = S[i][j], wkv7_cuda.cu:45-48)
 *   sa  fp32 [B,T,H,64],  sa[i] = sum_j a[j] * S_{t-1}[i][j]             (wkv7_cuda.cu:27-32)
 *   state fp32 [B,H,64,64], row = value index, col = key index          (rwkv7_state_fwd_fp16.cu:16)
 * The *_bf16 functions take bf16 tensors (the reference's only dtype); the *_f32 twins take fp32
 * tensors and exist for the fp32 logit-parity path.
 */
#ifndef RWKV7_HIP_H
#define RWKV7_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RWKV7_OK 0
#define RWKV7_EINVAL (-1)   /* null pointer / non-positive size */
#define RWKV7_ECHUNK (-2)   /* T % 16 != 0   (assert, wkv7_cuda.cu:136; rwkv_s2s_single_ffn.py:19) */
#define RWKV7_EHEAD  (-3)   /* H*64 != C     (assert, rwkv7_state_fwd_fp16.cu:61) */
#define RWKV7_ESHAPE (-4)   /* unsupported size for a fused elementwise op */

#define RWKV7_HEAD_SIZE 64
#define RWKV7_CHUNK_LEN 16

typedef void *rwkv7_stream_t; /* hipStream_t */

/* library identification: "rwkv7_hip <version> gfx950" */
const char *rwkv7_version(void);

/* ---- WKV7 training forward: torch.ops.wind_backstepping.forward (model/llm/cuda/wkv7_op.cpp:21-22,
 *      kernel wkv7_cuda.cu:10-52).  Zero initial state.  s and sa may both be NULL (inference). ---- */
int rwkv7_wkv_fwd_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                       const void *a, const void *b, void *y, float *s, float *sa, rwkv7_stream_t stream);
int rwkv7_wkv_fwd_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                      const void *a, const void *b, void *y, float *s, float *sa, rwkv7_stream_t stream);

/* ---- WKV7 training backward: torch.ops.wind_backstepping.backward (wkv7_op.cpp:23-24,
 *      kernel wkv7_cuda.cu:54-130).  Output order dw,dq,dk,dv,da,db == reference dw,dq,dk,dv,dz,da. ---- */
int rwkv7_wkv_bwd_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                       const void *a, const void *b, const void *dy, const float *s, const float *sa,
                       void *dw, void *dq, void *dk, void *dv, void *da, void *db, rwkv7_stream_t stream);
int rwkv7_wkv_bwd_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                      const void *a, const void *b, const void *dy, const float *s, const float *sa,
                      void *dw, void *dq, void *dk, void *dv, void *da, void *db, rwkv7_stream_t stream);

/* ---- The same pair on the matrix cores ("fast" twins; bf16, T % 32 == 0): what torch.ops.wind_backstepping.forward / .backward
 *      launch for bf16 tensors whose T is a multiple of 32 (rwkvtts_amd/ops.py), i.e. what a maintainer who binds the reference's op
 *      (wkv7_op.cpp:21-29) gets.  Same schema, same caller-allocated tensors, same y / sa / gradients (sa in the reference's
 *      layout, fp32 [B,T,H,64]).  `s` -- in the reference a private forward -> backward scratch of state checkpoints (its content is
 *      read by nothing but the backward kernel, rwkv_s2s_single_ffn.py:22-35) -- is used as an opaque arena of the SAME size:
 *      per 32-step chunk and head 9216 B of state checkpoint (q15 record, see rwkv7_wkv_chunk_fwd_bf16) + 4096 B of
 *      T = (I - A_ab)^-1 + 9216 B of adjoint state and 8192 B of Z written by the backward = 30 720 of the 32 768 B the
 *      reference's layout has there.  Launches: chunk_prep + chunk_fwd (forward); chunk_bseq + chunk_bwd_out_z (backward).  RWKV7_ECHUNK when T % 32 != 0:
 *      fall back to rwkv7_wkv_fwd_bf16 / rwkv7_wkv_bwd_bf16 (T % 16 == 0), whose `s` holds the reference's checkpoints. ---- */
int rwkv7_wkv_fwd_fast_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                            const void *a, const void *b, void *y, float *s, float *sa, rwkv7_stream_t stream);
int rwkv7_wkv_bwd_fast_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                            const void *a, const void *b, const void *dy, float *s, const float *sa,
                            void *dw, void *dq, void *dk, void *dv, void *da, void *db, rwkv7_stream_t stream);

/* Sizes of the two caller-allocated scratch tensors of the training forward/backward pair (the reference allocates
 * them in Python, rwkv_s2s_single_ffn.py:22-24): s = fp32 [B,H,T/16,64,64] state checkpoints, sa = fp32 [B,T,H,64]. */
int rwkv7_wkv_workspace_bytes(int B, int T, int H, size_t *s_bytes, size_t *sa_bytes);

/* Measurement / cross-check variants.  The library keeps NO process-global state: every entry point is re-entrant and safe
 * from several host threads on different streams (threading row); which kernel shape runs is an explicit
 * argument of these `_variant` twins, never a hidden switch that changes what the plain entry points above launch.
 *   cols_per_lane : state columns per lane of the scalar forward kernel -- 0 automatic by B*H (what the plain entry does), 4, 8
 *   wide          : row-split backward -- 0 = 256 threads, 2 state rows per lane tile (plain entry); 1 = 512 threads, 1 row
 *   (The chunked bf16 forward has one shipped kernel, csrc/wkv7_chunk_fwd9.hip; the bf16 instantiation of the 4-wave kernel that fp32
 *   tensors run is a lab-build entry, include/rwkv7_hip_lab.h.) */
int rwkv7_wkv_fwd_variant_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                               const void *a, const void *b, void *y, float *s, float *sa, int cols_per_lane, rwkv7_stream_t stream);
int rwkv7_wkv_fwd_variant_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                              const void *a, const void *b, void *y, float *s, float *sa, int cols_per_lane, rwkv7_stream_t stream);
int rwkv7_wkv_state_fwd_variant_bf16(int B, int T, int C, int H, float *state, const void *r, const void *w,
                                     const void *k, const void *v, const void *a, const void *b, void *y, int cols_per_lane,
                                     rwkv7_stream_t stream);
int rwkv7_wkv_bwd_split_variant_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                                     const void *a, const void *b, const void *dy, const float *s, const float *sa,
                                     void *const *dw, void *const *dq, void *const *dk, void *dv, void *const *da,
                                     void *const *db, int wide, rwkv7_stream_t stream);

/* ---- same backward with each head split over two workgroups (32 state rows each) so that 256 CUs are busy at
 *      B*H = 128.  dv is complete; dw,dq,dk,da,db are HOST arrays of 2 device pointers receiving the two partial
 *      column sums (final gradient = [0] + [1]); rwkv7_tmix_prepare_bwd_* can consume the pairs directly. ---- */
int rwkv7_wkv_bwd_split_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                             const void *a, const void *b, const void *dy, const float *s, const float *sa,
                             void *const *dw, void *const *dq, void *const *dk, void *dv, void *const *da,
                             void *const *db, rwkv7_stream_t stream);
int rwkv7_wkv_bwd_split_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                            const void *a, const void *b, const void *dy, const float *s, const float *sa,
                            void *const *dw, void *const *dq, void *const *dk, void *dv, void *const *da,
                            void *const *db, rwkv7_stream_t stream);

/* ---- state-carrying forward: torch.ops.rwkv7_state_fwd_fp16.forward (rwkv7_state_fwd_fp16.cpp:8-14,
 *      kernel rwkv7_state_fwd_fp16.cu:9-57) and its B=1 twin torch.ops.wkv7s.forward
 *      (wkv7s_op.cpp:9-15).  state is read at entry and overwritten at exit; any T >= 1. ---- */
int rwkv7_wkv_state_fwd_bf16(int B, int T, int C, int H, float *state, const void *r, const void *w,
                             const void *k, const void *v, const void *a, const void *b, void *y,
                             rwkv7_stream_t stream);
int rwkv7_wkv_state_fwd_f32(int B, int T, int C, int H, float *state, const void *r, const void *w,
                            const void *k, const void *v, const void *a, const void *b, void *y,
                            rwkv7_stream_t stream);

/* =====================================================================================================
 * Fused elementwise stages of the time-mix / channel-mix blocks.  Activations are [rows = B*T, D]
 * row-major, same dtype as the parameters (bf16 or fp32); `mask` is [rows] of that dtype or NULL;
 * D % 64 == 0 and D <= 8192.  `nblocks` = number of workgroups walking the rows; backward kernels
 * write per-workgroup fp32 partials of the parameter gradients, dparams_partial[nblocks][P][D], which
 * the caller sums over the first axis.
 * ===================================================================================================== */

/* token shift + nmix lerps (nmix = 6: x_r,x_w,x_k,x_v,x_a,x_g -- rwkv_s2s_single_ffn.py:160-169; nmix = 3: x_r,x_k,x_v when the
 * low-rank branches take their inputs through the lerp, fused.mix_lora;
 * nmix = 1: channel-mix x_k -- :224-227):  xm = x*mask ; out[i] = xm + (shift(xm) - xm) * params[i].
 * x_prev [B,D] (carried token-shift state, rwkv_asr_cuda_whisper.py:185) or NULL = zeros.
 * out is [nmix][rows][D]. */
int rwkv7_mix_fwd_bf16(int B, int T, int D, int nmix, const void *x, const void *x_prev, const void *mask,
                       const void *params, void *out, int nblocks, rwkv7_stream_t stream);
int rwkv7_mix_fwd_f32(int B, int T, int D, int nmix, const void *x, const void *x_prev, const void *mask,
                      const void *params, void *out, int nblocks, rwkv7_stream_t stream);
/* grad_outs: HOST array of nmix device pointers, one [rows][D] gradient per output of the forward.
 * Workgroup b walks the runs of run_len consecutive rows number b, b + nblocks, b + 2 nblocks, ...;
 * dparams_partial is [nblocks][nmix][D] fp32 (summed by the caller). */
int rwkv7_mix_bwd_bf16(int B, int T, int D, int nmix, const void *const *grad_outs, const void *x, const void *x_prev,
                       const void *mask, const void *params, void *dx, float *dparams_partial, int nblocks,
                       int run_len, rwkv7_stream_t stream);
int rwkv7_mix_bwd_f32(int B, int T, int D, int nmix, const void *const *grad_outs, const void *x, const void *x_prev,
                      const void *mask, const void *params, void *dx, float *dparams_partial, int nblocks,
                      int run_len, rwkv7_stream_t stream);

/* everything between the projections and the scan (rwkv_s2s_single_ffn.py:172-190):
 *   w = (-softplus(-w_pre) - 0.5)*mask ; k,v *= mask ; v += (v_first - v)*sigmoid(v_pre) (v_pre != NULL)
 *   a = sigmoid(a_pre) ; kk = l2norm_head(k*k_k)*mask ; k2 = k*(1 + (a-1)*k_a) ; v2 = v*mask
 * outputs w, k2, v2, ain = -kk, bin = kk*a (the scan's w,k,v,a,b).  v_pre/v_first NULL for layer 0.
 * backward partials: P = 5 (dk_k, dk_a, and the column sums of d_wpre, d_apre, d_vpre -- the bias gradients of the
 * low-rank branches that produced w_pre, a_pre, v_pre; the last is zero when v_pre is NULL). */
int rwkv7_tmix_prepare_fwd_bf16(long rows, int D, const void *w_pre, const void *k, const void *v, const void *a_pre,
                                const void *v_pre, const void *v_first, const void *mask, const void *k_k,
                                const void *k_a, void *w, void *k2, void *v2, void *ain, void *bin, int nblocks,
                                rwkv7_stream_t stream);
int rwkv7_tmix_prepare_fwd_f32(long rows, int D, const void *w_pre, const void *k, const void *v, const void *a_pre,
                               const void *v_pre, const void *v_first, const void *mask, const void *k_k,
                               const void *k_a, void *w, void *k2, void *v2, void *ain, void *bin, int nblocks,
                               rwkv7_stream_t stream);
int rwkv7_tmix_prepare_bwd_bf16(long rows, int D, const void *w_pre, const void *k, const void *v, const void *a_pre,
                                const void *v_pre, const void *v_first, const void *mask, const void *k_k,
                                const void *k_a, const void *d_w, const void *d_k2, const void *d_v2,
                                const void *d_ain, const void *d_bin, void *d_wpre, void *d_k, void *d_v,
                                void *d_apre, void *d_vpre, void *d_vfirst, float *dparams_partial, int nblocks,
                                rwkv7_stream_t stream);
int rwkv7_tmix_prepare_bwd_f32(long rows, int D, const void *w_pre, const void *k, const void *v, const void *a_pre,
                               const void *v_pre, const void *v_first, const void *mask, const void *k_k,
                               const void *k_a, const void *d_w, const void *d_k2, const void *d_v2,
                               const void *d_ain, const void *d_bin, void *d_wpre, void *d_k, void *d_v,
                               void *d_apre, void *d_vpre, void *d_vfirst, float *dparams_partial, int nblocks,
                               rwkv7_stream_t stream);

/* Same backward with the incoming gradients given as sums, added in fp32 on load (no separate add kernels): gsum is a
 * HOST array of 15 device pointers {d_w a,b; d_k2 a,b,c; d_v2 a,b; d_ain a,b; d_bin a,b; d_r a,b,c; d_vfirst_in}, and
 * d_r = d_r a+b+c is written as well.  Consumes the two partial sets of rwkv7_wkv_bwd_split_* plus tmix_post's
 * contributions to k2, v2 and r.  The second partials (d_w b, d_k2 b, d_ain b, d_bin b, d_r b) may be NULL: complete
 * gradients, as the chunked backward produces them.  d_vfirst_in (may be NULL): the gradient of v_first collected by the
 * layers after this one (v_first of layer 0 feeds every later layer, rwkv_s2s_single_ffn.py:179-182); d_vfirst = own + d_vfirst_in,
 * so the sum over the layers is formed layer by layer inside this kernel instead of by one [rows, D] add pass per layer. */
int rwkv7_tmix_prepare_bwd_sum_bf16(long rows, int D, const void *w_pre, const void *k, const void *v,
                                    const void *a_pre, const void *v_pre, const void *v_first, const void *mask,
                                    const void *k_k, const void *k_a, const void *const *gsum, void *d_wpre, void *d_k,
                                    void *d_v, void *d_apre, void *d_vpre, void *d_vfirst, void *d_r,
                                    float *dparams_partial, int nblocks, rwkv7_stream_t stream);
int rwkv7_tmix_prepare_bwd_sum_f32(long rows, int D, const void *w_pre, const void *k, const void *v,
                                   const void *a_pre, const void *v_pre, const void *v_first, const void *mask,
                                   const void *k_k, const void *k_a, const void *const *gsum, void *d_wpre, void *d_k,
                                   void *d_v, void *d_apre, void *d_vpre, void *d_vfirst, void *d_r,
                                   float *dparams_partial, int nblocks, rwkv7_stream_t stream);
/* The same with the COMPACT hand-off from rwkv7_tmix_post_bwd_compact_* (what bf16 training runs since round 4): the bonus term of
 * tmix_post contributes rank-1 per head -- d_v2 += dt * dot_h, d_k2 += ds_h r r_k, d_r += ds_h k2 r_k -- so the post backward writes
 * one tensor and two scalars per (row, head) instead of three tensors, and this kernel rebuilds them (k2 recomputed from k, a_pre,
 * k_a as the forward did).  gsum: HOST array of 19 device pointers = the 15 above (entries 4, 6, 13 -- the post tensors -- unused,
 * may be NULL) + {dt [rows,D], r [rows,D], r_k [D], hscal fp32 [rows][D/64][2] = (dot_h, ds_h)}. */
int rwkv7_tmix_prepare_bwd_sum_compact_bf16(long rows, int D, const void *w_pre, const void *k, const void *v,
                                            const void *a_pre, const void *v_pre, const void *v_first, const void *mask,
                                            const void *k_k, const void *k_a, const void *const *gsum, void *d_wpre, void *d_k,
                                            void *d_v, void *d_apre, void *d_vpre, void *d_vfirst, void *d_r,
                                            float *dparams_partial, int nblocks, rwkv7_stream_t stream);
int rwkv7_tmix_prepare_bwd_sum_compact_f32(long rows, int D, const void *w_pre, const void *k, const void *v,
                                           const void *a_pre, const void *v_pre, const void *v_first, const void *mask,
                                           const void *k_k, const void *k_a, const void *const *gsum, void *d_wpre, void *d_k,
                                           void *d_v, void *d_apre, void *d_vpre, void *d_vfirst, void *d_r,
                                           float *dparams_partial, int nblocks, rwkv7_stream_t stream);

/* ---- residual add + LayerNorm (block wiring of rwkv_s2s_single_ffn.py:262-276: x = x + att(ln1(x)); x = x + ffn(ln2(x));
 *      rwkvfla RWKV7Block attn_norm / ffn_norm / pre_norm, model-level norm) ----
 *   fwd: x_out = x + branch (rounded to the tensor type) ; h = LayerNorm(x_out; gamma, beta, eps) ; mean/rstd [rows] fp32.
 *        branch NULL: plain LayerNorm of x (x_out unused).  beta NULL: no bias.
 *   bwd: dx = d_resid + dLayerNorm(dh)   (d_resid NULL = 0) ; dparams_partial [nblocks][2][D] fp32 = dgamma, dbeta */
int rwkv7_add_ln_fwd_bf16(long rows, int D, const void *x, const void *branch, const void *gamma, const void *beta,
                          float eps, void *x_out, void *h, float *mean, float *rstd, int nblocks,
                          rwkv7_stream_t stream);
int rwkv7_add_ln_fwd_f32(long rows, int D, const void *x, const void *branch, const void *gamma, const void *beta,
                         float eps, void *x_out, void *h, float *mean, float *rstd, int nblocks,
                         rwkv7_stream_t stream);
int rwkv7_add_ln_bwd_bf16(long rows, int D, const void *dh, const void *d_resid, const void *x1, const float *mean,
                          const float *rstd, const void *gamma, void *dx, float *dparams_partial, int nblocks,
                          rwkv7_stream_t stream);
int rwkv7_add_ln_bwd_f32(long rows, int D, const void *dh, const void *d_resid, const void *x1, const float *mean,
                         const float *rstd, const void *gamma, void *dx, float *dparams_partial, int nblocks,
                         rwkv7_stream_t stream);
/* ---- the two stages above in one pass each (training path without carried state): residual add + LayerNorm + token-shift
 *      lerps, i.e. everything between a block's branch output and the inputs of the next projections
 *      (rwkv_s2s_single_ffn.py:251-259 with :160-169 / :223-226).
 *   fwd: x_out = x + branch ; h = LayerNorm(x_out) rounded to the tensor type ; hm = h*mask ;
 *        out[i] = hm + (shift(hm) - hm) * params[i], out [nmix][rows][D] ; mean/rstd [rows].  branch NULL: x_out unused.
 *   bwd: from the nmix output gradients (HOST array of device pointers) and the gradient d_resid arriving at x_out:
 *        dx (= gradient of x and of branch) ; dparams_partial [nblocks][nmix + 2][D] fp32 = dparams[0..nmix), dgamma, dbeta.
 *   Workgroup b walks the runs of run_len consecutive rows number b, b + nblocks, ... ---- */
int rwkv7_add_ln_mix_fwd_bf16(int B, int T, int D, int nmix, const void *x, const void *branch, const void *gamma,
                              const void *beta, float eps, const void *mask, const void *params, void *x_out, void *out,
                              float *mean, float *rstd, int nblocks, int run_len, rwkv7_stream_t stream);
int rwkv7_add_ln_mix_fwd_f32(int B, int T, int D, int nmix, const void *x, const void *branch, const void *gamma,
                             const void *beta, float eps, const void *mask, const void *params, void *x_out, void *out,
                             float *mean, float *rstd, int nblocks, int run_len, rwkv7_stream_t stream);
/*   fwd_h: the same forward that ALSO stores h [rows][D] (unmasked), for callers whose backward runs as the two separate kernels
 *        rwkv7_mix_bwd_* + rwkv7_add_ln_bwd_* (the six-lerp side: its one-pass backward carries 6 x 3 x 8 values per thread and
 *        spills; the one-pass forward is 18 us per layer ahead of the two stages even with the extra store). */
int rwkv7_add_ln_mix_fwd_h_bf16(int B, int T, int D, int nmix, const void *x, const void *branch, const void *gamma,
                                const void *beta, float eps, const void *mask, const void *params, void *x_out, void *out, void *h,
                                float *mean, float *rstd, int nblocks, int run_len, rwkv7_stream_t stream);
int rwkv7_add_ln_mix_fwd_h_f32(int B, int T, int D, int nmix, const void *x, const void *branch, const void *gamma,
                               const void *beta, float eps, const void *mask, const void *params, void *x_out, void *out, void *h,
                               float *mean, float *rstd, int nblocks, int run_len, rwkv7_stream_t stream);
int rwkv7_mix_add_ln_bwd_bf16(int B, int T, int D, int nmix, const void *const *grad_outs, const void *d_resid, const void *x1,
                              const float *mean, const float *rstd, const void *gamma, const void *beta, const void *mask,
                              const void *params, void *dx, float *dparams_partial, int nblocks, int run_len,
                              rwkv7_stream_t stream);
int rwkv7_mix_add_ln_bwd_f32(int B, int T, int D, int nmix, const void *const *grad_outs, const void *d_resid, const void *x1,
                             const float *mean, const float *rstd, const void *gamma, const void *beta, const void *mask,
                             const void *params, void *dx, float *dparams_partial, int nblocks, int run_len,
                             rwkv7_stream_t stream);

/* after the scan (rwkv_s2s_single_ffn.py:192-195): out = (GroupNorm_H(y; gn_w, gn_b, eps) + (sum_head r*k*r_k) v) * g.
 * r_k is [H*64] flattened.  backward partials: P = 3 (d gn_w, d gn_b, d r_k). */
int rwkv7_tmix_post_fwd_bf16(long rows, int D, const void *y, const void *r, const void *k, const void *v,
                             const void *g, const void *gn_w, const void *gn_b, const void *r_k, float eps, void *out,
                             int nblocks, rwkv7_stream_t stream);
int rwkv7_tmix_post_fwd_f32(long rows, int D, const void *y, const void *r, const void *k, const void *v,
                            const void *g, const void *gn_w, const void *gn_b, const void *r_k, float eps, void *out,
                            int nblocks, rwkv7_stream_t stream);
int rwkv7_tmix_post_bwd_bf16(long rows, int D, const void *dout, const void *y, const void *r, const void *k,
                             const void *v, const void *g, const void *gn_w, const void *gn_b, const void *r_k,
                             float eps, void *d_y, void *d_r, void *d_k, void *d_v, void *d_g, float *dparams_partial,
                             int nblocks, rwkv7_stream_t stream);
int rwkv7_tmix_post_bwd_f32(long rows, int D, const void *dout, const void *y, const void *r, const void *k,
                            const void *v, const void *g, const void *gn_w, const void *gn_b, const void *r_k,
                            float eps, void *d_y, void *d_r, void *d_k, void *d_v, void *d_g, float *dparams_partial,
                            int nblocks, rwkv7_stream_t stream);
/* compact form: d_y, d_g as above; dt = dL/d(GroupNorm(y) + bonus) [rows,D] and hscal fp32 [rows][D/64][2] = (sum_head r k r_k,
 * sum_head dt v) instead of d_r, d_k, d_v (rebuilt by rwkv7_tmix_prepare_bwd_sum_compact_*) */
int rwkv7_tmix_post_bwd_compact_bf16(long rows, int D, const void *dout, const void *y, const void *r, const void *k,
                                     const void *v, const void *g, const void *gn_w, const void *gn_b, const void *r_k,
                                     float eps, void *d_y, void *dt, void *d_g, float *hscal, float *dparams_partial,
                                     int nblocks, rwkv7_stream_t stream);
int rwkv7_tmix_post_bwd_compact_f32(long rows, int D, const void *dout, const void *y, const void *r, const void *k,
                                    const void *v, const void *g, const void *gn_w, const void *gn_b, const void *r_k,
                                    float eps, void *d_y, void *dt, void *d_g, float *hscal, float *dparams_partial,
                                    int nblocks, rwkv7_stream_t stream);

/* channel-mix activation relu(x)^2 (rwkv_s2s_single_ffn.py:228) and dx = 2 relu(x) dy; n % 8 == 0 */
int rwkv7_relusq_fwd_bf16(long n, const void *x, void *y, rwkv7_stream_t stream);
int rwkv7_relusq_fwd_f32(long n, const void *x, void *y, rwkv7_stream_t stream);
int rwkv7_relusq_bwd_bf16(long n, const void *x, const void *dy, void *dx, rwkv7_stream_t stream);
int rwkv7_relusq_bwd_f32(long n, const void *x, const void *dy, void *dx, rwkv7_stream_t stream);
/* the same backward from the OUTPUT s = relu(x)^2 (dx = 2 sqrt(s) dy): rwkv7_gemm_nt_bf16 with the activation as its epilogue never
 * writes x */
int rwkv7_relusq_bwd_s_bf16(long n, const void *s, const void *dy, void *dx, rwkv7_stream_t stream);
int rwkv7_relusq_bwd_s_f32(long n, const void *s, const void *dy, void *dx, rwkv7_stream_t stream);

/* =====================================================================================================
 * Chunked (MFMA) WKV7 -- the training fast path.  Same operator as rwkv7_wkv_fwd/bwd (reference
 * wkv7_cuda.cu:10-130), evaluated 32 steps at a time on the matrix cores (algebra: csrc/chunk_common.h).
 * Requires T % 32 == 0 and exp(w) <= ~2 per step (the model's soft-clamped decay satisfies it:
 * w <= -0.5, rwkv_s2s_single_ffn.py:172).  Scratch / saved tensors, all caller-allocated fp32:
 *   tinv [B,H,T/32,32,32]   (I - A_ab)^-1 per chunk, written by _prep, read by _fwd and _bwd
 *   sa   [B,T,H,64]         u_t = S_{t-1} a_t (same meaning as the scalar op's `sa`)
 *   hs   [B,H,T/32,64,64]   state at the START of each chunk, bf16, [value][key]: the backward's checkpoint (the forward itself
 *                           carries the state in fp32; the checkpoint is its bf16 rounding, 8 KB per chunk and head)
 * sa and hs may both be NULL in _fwd (inference).
 * ===================================================================================================== */
#define RWKV7_CHUNK_T 32
/* One 64x64 fp32 matrix handed between the chunk kernels (hs, e_vk, np) as a "q15" record: 4096 int16 mantissas in MFMA
 * accumulator order [tile][lane][16] followed by 256 fp32 scales [tile][lane] (x = mantissa * scale of its lane); see
 * csrc/chunk_common.h.  Sizes of hs / e_vk / np buffers: RWKV7_Q15_REC uint16 per (batch, head, chunk). */
#define RWKV7_Q15_REC (64 * 64 + 2 * 256)
int rwkv7_wkv_chunk_prep_bf16(int B, int T, int H, const void *w, const void *a, const void *b, float *tinv,
                              rwkv7_stream_t stream);
int rwkv7_wkv_chunk_prep_f32(int B, int T, int H, const void *w, const void *a, const void *b, float *tinv,
                             rwkv7_stream_t stream);
int rwkv7_wkv_chunk_fwd_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                             const void *a, const void *b, const float *tinv, void *y, float *sa, void *hs,
                             rwkv7_stream_t stream);
int rwkv7_wkv_chunk_fwd_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                            const void *a, const void *b, const float *tinv, void *y, float *sa, void *hs,
                            rwkv7_stream_t stream);
/* Packed variable-length rows (fla chunk_rwkv7's `cu_seqlens`; the reference passes it for its packed Spark batches,
 * train_spark_rwkv7speech.py:238-239, data/utils/spark_dataset.py:111-162): the caller lays the sequences out 32-aligned
 * and passes seq_chunk_off, int32 [nseq + 1] on the device: sequence s owns the 32-step chunks seq_chunk_off[s] ..
 * seq_chunk_off[s+1] - 1, counted over the whole [B][T/32] chunk space (a sequence does not span rows).  Every sequence
 * starts from the zero state and gets its own workgroups, so the sequences of a row run in parallel; chunks that belong to
 * no sequence are left untouched.  seq_chunk_off == NULL: the plain ops above (one sequence per row). */
int rwkv7_wkv_chunk_fwd_seq_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                                 const void *a, const void *b, const float *tinv, void *y, float *sa, void *hs,
                                 const int *seq_chunk_off, int nseq, rwkv7_stream_t stream);
int rwkv7_wkv_chunk_fwd_seq_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                                const void *a, const void *b, const float *tinv, void *y, float *sa, void *hs,
                                const int *seq_chunk_off, int nseq, rwkv7_stream_t stream);
/* ---- chunked backward, bf16 (csrc/wkv7_chunk_bseq.hip, wkv7_chunk_bwd10.hip; reference wkv7_cuda.cu:54-130).  With H = S^T and the
 *      chunk quantities above, the adjoint state obeys E_c = M_c^T E_{c+1} + N'_c.  T % 32 == 0.
 *   bseq    : sequential over chunks (reverse), one workgroup per (head, half of the value columns): the recurrence in factored
 *             form, E_c = E' + A~^T Z + Q~^T dY with Z = (T^T B^) E' + (T^T A_qb^T) dY, E' = g_C E_{c+1} -- M_c^T and N'_c are
 *             never formed and never reach HBM.  e_vk[b,h,c] = E_{c+1}, what chunk c receives from its future, one q15 record
 *             per chunk (int16 [4 tiles][64 lanes][16] + fp32 scale [4][64]; RWKV7_Q15_REC uint16 units; the recurrence itself
 *             carries ~16 mantissa bits, the per-chunk kernel reads this rounded copy once); seq_chunk_off / nseq as in
 *             rwkv7_wkv_chunk_fwd_seq_bf16 (NULL / 0 for plain rows). ---- */
int rwkv7_wkv_chunk_bseq_bf16(int B, int T, int H, const void *w, const void *q, const void *a, const void *b, const void *dy,
                              const float *tinv, void *e_vk, float *z, const int *seq_chunk_off, int nseq, rwkv7_stream_t stream);
/*             z (may be NULL): fp32 [B,T,H,64], Z_t = dL/du_t (u = sa), which the recurrence forms anyway.  With it the per-chunk
 *             gradient kernel needs neither T^-1 nor an A_qb -> G1 -> Z chain of its own.
 *   bwd_out_z : parallel over chunks: the six gradients (the contract of wind_backstepping::backward) from what the chunked
 *             forward saved (hs, sa) and e_vk, z of `bseq`; two matrix phases per chunk (csrc/wkv7_chunk_bwd10.hip: raw rows by
 *             LDS-DMA, unpadded XOR-swizzled planes, state prologue and phase A in one barrier interval). */
int rwkv7_wkv_chunk_bwd_out_z_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                                   const void *a, const void *b, const void *dy, const void *hs, const float *sa,
                                   const float *z, const void *e_vk, void *dw, void *dq, void *dk, void *dv,
                                   void *da, void *db, rwkv7_stream_t stream);
/* ---- the two sequential chunked kernels with a carried state (bf16, plain rows, T % 32 == 0): training through a recurrent state.
 *   fwd_state  : rwkv7_wkv_chunk_fwd_seq_bf16 (seq_chunk_off = NULL) starting from h0 instead of zero; hs of chunk 0 then holds h0;
 *                hT receives the state after the last chunk (fp32, from the recurrence's own accumulators).
 *   bseq_state : rwkv7_wkv_chunk_bseq_bf16 (seq_chunk_off = NULL) with dhT = dL/d(final state) as the adjoint after the last chunk
 *                (it flows into e_vk[last] and on); dh0 receives dL/dh0.
 *   h0, hT, dhT, dh0: fp32 [B,H,64,64], row = value, column = key (the layout of rwkv7_wkv_state_fwd_*'s state).  Each may be NULL
 *   (a zero input / no output); with all of them NULL the results are bit-identical to the stateless entries.  y, hT, e_vk, z and
 *   dh0 are correct for any row.
 *   THE SIX GRADIENTS NEED A FRAMED ROW.  rwkv7_wkv_chunk_bwd_out_z_bf16 (the per-chunk gradients on top of these two) assumes that
 *   every row starts from the zero state and has no future: a workgroup hands the end state of one chunk on as the start state of
 *   the next and zeroes it across a row boundary, and the decay gradient of a row's last chunk drops its rowsum(E * H_C) term.  With
 *   a non-zero h0 or dhT its dw, dq, dk, dv, da, db are therefore valid only if the row starts AND ends with one whole identity
 *   chunk -- 32 steps with w = -1e4 (exp(w) underflows to 0: decay exactly 1) and q = k = v = a = b = 0 -- whose gradients the
 *   caller drops (the identity chunks pass h0 and dhT through bit for bit).  rwkvtts_amd/ops.py, _WkvStateChunked (with the framing
 *   wkv7_state_chunked chooses), does this.  Both entries are the packed ones below with seq_chunk_off = NULL, nseq = 0. ---- */
int rwkv7_wkv_chunk_fwd_state_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                                   const void *a, const void *b, const float *tinv, void *y, float *sa, void *hs,
                                   const float *h0, float *hT, rwkv7_stream_t stream);
int rwkv7_wkv_chunk_bseq_state_bf16(int B, int T, int H, const void *w, const void *q, const void *a, const void *b,
                                    const void *dy, const float *tinv, void *e_vk, float *z,
                                    const float *dhT, float *dh0, rwkv7_stream_t stream);
/* ---- the same two kernels on packed rows (seq_chunk_off / nseq as rwkv7_wkv_chunk_fwd_seq_bf16; NULL / 0: plain rows, as above):
 *   one carried state per SEQUENCE.  h0, hT, dhT, dh0: fp32 [nseq,H,64,64] (entry s * H + h: sequence s, head h), each may be NULL;
 *   with all of them NULL the results are bit-identical to rwkv7_wkv_chunk_fwd_seq_bf16 / rwkv7_wkv_chunk_bseq_bf16 with the same
 *   seq_chunk_off.  A sequence with an empty chunk range writes hT = h0 and dh0 = dhT (zeros for a NULL input).  y, hT, e_vk, z and
 *   dh0 are correct for any packed row; seq_chunk_off must cover every chunk the per-chunk gradients read (as for the stateless op).
 *   FRAMING FOR THE SIX GRADIENTS ON A PACKED ROW (B = 1).  rwkv7_wkv_chunk_bwd_out_z_bf16 reads the end state H_C of chunk c from
 *   hs[c + 1], the next chunk's start record: for a sequence's last chunk that is the NEXT sequence's h0 (or zero at the row's end),
 *   and with a non-zero dhT its decay term rowsum(E * H_C) is then wrong.  Each sequence therefore needs ONE TRAILING identity chunk
 *   (32 steps with w = -1e4 and q = k = v = a = b = 0, inside its chunk range, gradients dropped) whenever dhT is non-zero.  Inside
 *   the row no sequence needs a leading one: the start state of a sequence's first chunk is hs[c0] = h0 whether the gradient
 *   workgroup loads it directly or takes it as the H_C of the chunk before (hs[c0] again).  But the ROW needs one leading identity
 *   chunk when its first sequence has a non-zero h0: that kernel's workgroups walk the [H][T/32] chunk space across head
 *   boundaries and hand a zero state into each head's first chunk (measured: without it dq of the row's first sequence was wrong on
 *   every head but head 0).  tests/test_varlen_state_gpu.py checks the six gradients and dh0 against fp64 autograd and bit for bit
 *   against the framed plain op.  rwkvtts_amd/ops.py, packed_state_layout / wkv7_state_chunked_varlen, lay rows out this way. ---- */
int rwkv7_wkv_chunk_fwd_state_seq_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                                       const void *a, const void *b, const float *tinv, void *y, float *sa, void *hs,
                                       const int *seq_chunk_off, int nseq, const float *h0, float *hT, rwkv7_stream_t stream);
int rwkv7_wkv_chunk_bseq_state_seq_bf16(int B, int T, int H, const void *w, const void *q, const void *a, const void *b,
                                        const void *dy, const float *tinv, void *e_vk, float *z, const int *seq_chunk_off, int nseq,
                                        const float *dhT, float *dh0, rwkv7_stream_t stream);
/* ---- stateful packed PREFILL into chosen rows of a cache (rwkvtts_amd/prefill.py, PackedPrefill): bf16, forward only, no tape.  Every
 *      index below is a device pointer read at run time, so one captured launch serves every pack of the same shapes.
 *   rwkv7_wkv_chunk_fwd_state_rows_bf16: rwkv7_wkv_chunk_fwd_state_seq_bf16 (B = 1, no sa / hs) on indexed rows of a cache field, IN
 *      PLACE.  state fp32 [S,H,64,64]; state_row int32 [nseq]: sequence s loads its start state from state[state_row[s]] and stores
 *      its end state there.  state_row[s] < 0: the sequence is inactive, its workgroups return and write nothing (y of its chunks
 *      included: give it an empty chunk range).  Bit 30 (RWKV7_STATE_ROW_ZERO) set: start from zero instead of loading.  The row
 *      index (state_row[s] without bit 30) MUST lie in [0, S) and the active rows must be distinct: they live on the device and are
 *      NOT checked here -- the caller guarantees both (PackedPrefill.plan validates on the host before it copies).  Each of the two
 *      workgroups of a (sequence, head) owns its own 32 value rows of the entry, which makes the in-place update safe.  The grid is
 *      sized by nseq, the capacity, not by the live count.  y and the end states are bit-identical to the _state_seq entry run on
 *      the gathered rows (h0 = zeros for bit 30).  RWKV7_EINVAL: NULL pointer, T / H / nseq < 1; RWKV7_ESHAPE: T % 32 != 0. */
#define RWKV7_STATE_ROW_ZERO (1 << 30)
int rwkv7_wkv_chunk_fwd_state_rows_bf16(int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a,
                                        const void *b, const float *tinv, void *y, const int *seq_chunk_off, int nseq, float *state,
                                        const int *state_row, rwkv7_stream_t stream);
/*   rwkv7_add_ln_mix_rows_fwd_bf16: rwkv7_add_ln_mix_fwd_bf16 (B = 1, nmix = 6 or 1, branch may be NULL, mask per row or NULL, no
 *      mean / rstd) on a packed row of T rows whose token-shift predecessors may be carried, with two int32 maps of length T:
 *        prev_src[t]  -1: ordinary, the predecessor is the masked h of row t - 1 (0 for t = 0); -2: the predecessor is zero (the first
 *                     token of a fresh sequence); r >= 0: the predecessor is row r of the cache field x_prev [S,D]
 *        last_dst[t]  -1: nothing; r >= 0: this row's hm (h rounded to bf16 and masked, exactly what the lerp reads) -> x_prev[r]
 *      The lerp on a carried row is the kernel's own hm + (x_prev - hm) * mu in fp32 with one rounding.  x_out and every ordinary
 *      row are bit-identical to rwkv7_add_ln_mix_fwd_bf16 (one LayerNorm device routine, csrc/ln_row.h).
 *      x_prev_rd: where carried predecessors are READ; NULL = x_prev itself.  A row that reads and writes the same r (a one-token
 *      piece) reads first, inside the thread that owns the channels.  A piece of SEVERAL rows whose first row reads r while its
 *      last row writes r is two different workgroups and a race on x_prev: pass a snapshot of the field as x_prev_rd then (what
 *      PackedPrefill does).  Rows r are not range-checked (device data; caller's guarantee, as above); each r at most once per map.
 *      RWKV7_EINVAL: NULL x / gamma / params / out / prev_src / last_dst / x_prev, branch without x_out, T, nblocks or run_len < 1;
 *      RWKV7_ESHAPE: T % 32 != 0, nmix not in {1, 6}, D % 64 != 0 or D > 4096. ---- */
int rwkv7_add_ln_mix_rows_fwd_bf16(int T, int D, int nmix, const void *x, const void *branch, const void *gamma, const void *beta,
                                   float eps, const void *mask, const void *params, const int *prev_src, const int *last_dst,
                                   const void *x_prev_rd, void *x_prev, void *x_out, void *out, int nblocks, int run_len,
                                   rwkv7_stream_t stream);
/*   rwkv7_cache_rows_commit_bf16: copy whole rows of one cache into chosen rows of another, every field of every layer, in one
 *      launch (csrc/cache_rows.hip).  ContinuousDecoder(admission="overlap") prefills admitted prompts into a small staging cache on a
 *      side stream and commits the finished rows into the slots' rows with this entry on the decode stream.
 *        src_tbl / dst_tbl  DEVICE tables of 3 * layers pointers, per layer in the order att_x_prev (bf16 [S,D]), att_kv (fp32
 *                           [S,H,64,64]), ffn_x_prev (bf16 [S,D]); every field contiguous and 16-byte aligned.  The two caches may
 *                           have different row counts S.
 *        src_row / dst_row  DEVICE int32 [n]: entry i copies row src_row[i] of the source to row dst_row[i] of the destination.  An
 *                           entry with dst_row[i] < 0 (or src_row[i] < 0) is skipped.  Rows not named keep every bit; the copy
 *                           preserves bits (NaN payloads included).
 *      The row indices and the tables live on the device and are NOT checked here: the caller guarantees rows inside the caches and
 *      distinct destination rows among the active entries (the Python wrapper validates on the host before it copies them over).
 *      src_tbl and dst_tbl may name the SAME cache, provided no row is both read and written in one call (no active dst_row[i]
 *      equals an active src_row[j]); a source row may be repeated, which fans it out (ContinuousDecoder.submit_n copies a prompt's
 *      row to its sibling candidates' rows this way).
 *      n = 0 returns RWKV7_OK without a launch.  RWKV7_EINVAL: NULL table, NULL index array with n > 0, n < 0, layers < 1, n or
 *      layers > 65535, D or H < 1; RWKV7_ESHAPE: D % 8 != 0 or D > 4096; RWKV7_EHEAD: D != 64 * H.  Nothing is launched then. */
int rwkv7_cache_rows_commit_bf16(int layers, int n, const void *const *src_tbl, void *const *dst_tbl, const int *src_row,
                                 const int *dst_row, int D, int H, rwkv7_stream_t stream);
/*   rwkv7_cache_rows_seed_bf16: the same launch (one kernel body, csrc/cache_rows.hip) for an admission that starts some requests
 *      from STORED states and the others from zero (rwkvtts_amd/state_store.py; ContinuousDecoder(..., state_store=...)): what 3 L
 *      index_fill_ plus 3 L index_copy_ calls do, and the choice between the two is device data.  Tables, shapes and error codes as
 *      for rwkv7_cache_rows_commit_bf16.  Entry i, with s = src_row[i] and d = dst_row[i]:
 *        d < 0                        skipped
 *        s >= 0                       row s of the source -> row d of the destination, all three fields of all layers, bits preserved
 *        s == RWKV7_SEED_ZERO (-1)    zeros -> row d of the destination, all three fields of all layers; the source is not read
 *        s < -1                       skipped
 *      Rows are NOT range-checked (device data): the caller guarantees source rows inside the source cache, destination rows inside
 *      the destination cache, and DISTINCT destination rows among the active entries (copy and zero entries alike).  With one
 *      cache as source and destination no active destination may equal an active source.  Rows not named keep every bit.
 *      n = 0 returns RWKV7_OK without a launch.  RWKV7_EINVAL: NULL table, NULL index array with n > 0, n < 0, layers < 1, n or
 *      layers > 65535, D or H < 1; RWKV7_ESHAPE: D % 8 != 0 or D > 4096; RWKV7_EHEAD: D != 64 * H.  Nothing is launched then. */
#define RWKV7_SEED_ZERO (-1)
int rwkv7_cache_rows_seed_bf16(int layers, int n, const void *const *src_tbl, void *const *dst_tbl, const int *src_row,
                               const int *dst_row, int D, int H, rwkv7_stream_t stream);
/*   rwkv7_cache_rows_retain_bf16: the same copy body (csrc/cache_rows.hip) as the last launch of a continuous-batching step
 *      (ContinuousDecoder(..., state_store=..., retain=True)): the state a request leaves behind goes to a row of a StateStore in the
 *      very step in which the request ends, before a later step runs the dead slot's row through stale inputs.  Tables, field order,
 *      alignment and error codes as for rwkv7_cache_rows_commit_bf16; the source cache has at least `slots` rows.
 *        live        DEVICE uint8 [slots]  the engine's live flags (rwkv7_slot_state.live), read only
 *        armed       DEVICE uint8 [slots]  != 0: the slot's request is to be retained; cleared by the launch that copies the slot
 *        retain_row  DEVICE int32 [slots]  the destination row of slot s, or a negative value (no row), read only
 *        ticket      DEVICE int32 [slots]  zero between launches; workspace of the launch
 *      Slot s is copied -- row s of the source -> row retain_row[s] of the destination, all three fields of all layers, bits
 *      preserved -- when armed[s] != 0, live[s] == 0 and retain_row[s] >= 0, and then armed[s] is 0 when the launch completes, so the
 *      copy happens once.  In every other case nothing of slot s is read or written beyond the flags.  Many workgroups serve one
 *      slot; each reads the flags, copies its piece and draws a ticket with a device-scope atomic add on ticket[s], and the one
 *      that draws the last ticket clears armed[s] and ticket[s]: no workgroup sees armed[s] cleared within its own launch.
 *      retain_row is NOT range-checked (device data): the caller guarantees rows inside the destination cache, distinct among the
 *      non-negative entries (the Python wrapper validates on the host), and a destination that is not the source cache.
 *      slots = 0 returns RWKV7_OK without a launch.  RWKV7_EINVAL: NULL table, NULL live / armed / retain_row / ticket (whatever
 *      slots is), slots < 0, layers < 1, slots or layers > 65535, D or H < 1; RWKV7_ESHAPE: D % 8 != 0 or D > 4096; RWKV7_EHEAD:
 *      D != 64 * H.  Nothing is launched then. */
int rwkv7_cache_rows_retain_bf16(int layers, int slots, const void *const *src_tbl, void *const *dst_tbl, const unsigned char *live,
                                 unsigned char *armed, const int *retain_row, int *ticket, int D, int H, rwkv7_stream_t stream);
/* ---- state tuning (rwkvtts_amd/state_tune.py, csrc/state_tune.hip): every weight frozen, the initial states of named voices are
 *      the trained tensors.  The MASTER state of voice v is fp32, per layer att_x_prev [V,D], att_kv [V,H,64,64], ffn_x_prev [V,D];
 *      its AdamW moments m and v are fp32 of the same shapes.  Every table below is a DEVICE table of 3 * layers pointers in the
 *      order of rwkv7_cache_rows_seed_bf16 (per layer att_x_prev, att_kv, ffn_x_prev; every field contiguous, 16-byte aligned).
 *   rwkv7_state_rows_expand_f32: the forward hand-over, one launch for all layers and fields.  dst_tbl names an n-row bf16 cache
 *      (att_x_prev / ffn_x_prev bf16 [n,D], att_kv fp32 [n,H,64,64]); voice is DEVICE int32 [n].  Entry i, with v = voice[i]:
 *        v >= 0     master row v -> row i of the cache: att_kv bits copied, the two shift rows rounded ONCE to bf16
 *                   (round-to-nearest-even; a NaN stays a quiet NaN)
 *        v == -1    zeros -> row i, all three fields of all layers; no source is read
 *        v < -1     skipped: row i keeps every bit
 *      voice[i] is NOT range-checked against the master's rows (device data; the caller's guarantee).
 *      n = 0 returns RWKV7_OK without a launch.  Error codes as for rwkv7_cache_rows_seed_bf16: RWKV7_EINVAL: NULL table, NULL voice
 *      with n > 0, n < 0, layers < 1, n or layers > 65535, D or H < 1; RWKV7_ESHAPE: D % 8 != 0 or D > 4096; RWKV7_EHEAD:
 *      D != 64 * H.  Nothing is launched then. */
int rwkv7_state_rows_expand_f32(int layers, int n, const void *const *master_tbl, void *const *dst_tbl, const int *voice, int D, int H,
                                rwkv7_stream_t stream);
/*   rwkv7_state_rows_adamw_f32: the optimizer step of the voices of one batch, one launch for all layers, fields and active voices.
 *        grad_tbl     the leaf gradients of the n-row cache the forward started from: fp32 [n,H,64,64] for att_kv, bf16 [n,D] for
 *                     the shift rows.  A NULL entry: that field is not tuned -- its master, moments and store row are left alone
 *                     (the m_tbl / v_tbl entries of such a field are not read and may be NULL too)
 *        master_tbl, m_tbl, v_tbl   the fp32 master states and moments, updated in place
 *        store_tbl    the serving cache (a StateStore's: bf16 shift rows, fp32 att_kv) that receives the new states
 *        seg_start    DEVICE int32 [A + 1], a CSR over seg_rows: active voice a owns seg_rows[seg_start[a] .. seg_start[a + 1])
 *        seg_rows     DEVICE int32 [seg_start[A]]: rows of the gradient cache, grouped by voice
 *        seg_info     DEVICE int32 [A][3] = {the voice's row in the master, its row in the store or -1 (no row is written), its
 *                     step count t >= 1 (1 for its first update)}
 *        skip_flag    DEVICE float or NULL; != 0 runs the step on a ZERO gradient, as rwkv7_adamw_groups_bf16 does (the gradients
 *                     are still read; a NaN in them reaches nothing)
 *      Per element of a tuned field of an active voice: g = grad_scale * (the gradients of the voice's rows added in fp32, one after
 *      the other in the listed order, starting from 0), then the update rule of rwkv7_adamw_bf16 (torch.optim.AdamW, decoupled
 *      weight decay) with the bias corrections 1 - beta^t of THAT voice's t, formed on the device in double from the float betas;
 *      then the new state is written to the voice's store row: the fp32 value for att_kv, one round-to-nearest-even to bf16 for the
 *      shift rows.  No atomics: an element is owned by one thread, which walks the voice's rows itself, so a voice's result does not
 *      depend on the grid, on the other voices of the launch or on their order, and two identical calls give the same bits.  Voices
 *      not named keep every bit of master, moments and store row.  A voice may be listed ONCE, store rows must be distinct, and the
 *      gradient cache must not overlap the store.  No row is range-checked (device data; the caller validates on the host).
 *      n = 0 or A = 0 returns RWKV7_OK without a launch.  RWKV7_EINVAL: a NULL table, a NULL seg_* array with n > 0 and A > 0, n or
 *      A < 0 or > 65535, layers < 1 or > 21845 (3 * layers is a grid dimension), D or H < 1; RWKV7_ESHAPE: D % 8 != 0 or D > 4096;
 *      RWKV7_EHEAD: D != 64 * H.  Nothing is launched then. */
int rwkv7_state_rows_adamw_f32(int layers, int n, int A, const void *const *grad_tbl, void *const *master_tbl, void *const *m_tbl,
                               void *const *v_tbl, void *const *store_tbl, const int *seg_start, const int *seg_rows, const int *seg_info,
                               const float *skip_flag, float lr, float beta1, float beta2, float eps, float weight_decay,
                               float grad_scale, int D, int H, rwkv7_stream_t stream);
/*      (The round-3/4 per-chunk gradient kernel, csrc/lab/wkv7_chunk_bwd9.hip, is an A/B twin with its own entry point in the lab build:
 *      include/rwkv7_hip_lab.h.  There are no process-wide switches in this library.) */
/* ---- head loss: softmax cross-entropy of a chunk of bf16 logits [rows,V], forward and backward in one pass
 *      (spark_llm.py:146-160, FusedLinearCrossEntropyLoss).  labels int64 [rows]; rows with label == ignore_index give 0.
 *      loss_rows[rows] = logsumexp - logit[label]; logits are REPLACED by (softmax - onehot) * scale. ---- */
int rwkv7_ce_fwd_bwd_bf16(long rows, int V, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
                          rwkv7_stream_t stream);
/*      The same with label smoothing (torch.nn.CrossEntropyLoss(label_smoothing = ls), the XY heads: xy_llm.py:233-240):
 *      loss_rows = (1 - ls)(logsumexp - logit[label]) + ls (logsumexp - mean logit); logits REPLACED by
 *      (softmax - ls / V - (1 - ls) onehot) * scale.  0 <= ls < 1; ls = 0 is the entry above. */
int rwkv7_ce_fwd_bwd_ls_bf16(long rows, int V, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
                             float label_smoothing, rwkv7_stream_t stream);
/*      The same on logits with a leading dimension ld >= V elements (rows of a buffer padded to aligned rows; columns V .. ld - 1 are
 *      neither read nor written). */
int rwkv7_ce_fwd_bwd_ld_bf16(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
                             float label_smoothing, rwkv7_stream_t stream);
/*      The same with two regularisers of the logits' scale added to the GRADIENT (losses.fused_linear_cross_entropy(z_loss, max_logit);
 *      DESIGN.md section 6.8).  For a valid row with p = softmax, lse = logsumexp, m = max_j x_j (all fp32 from the bf16 logits), a the
 *      LOWEST index with x_a = m and t the (smoothed) target, element j is REPLACED by
 *        (p_j (1 + 2 z_coef lse) - t_j + [j == a] max_coef m) * scale      (formed in fp32, rounded to bf16 once)
 *      -- the gradient of CE + z_coef lse^2 + 0.5 max_coef m^2.  loss_rows stays the PLAIN cross-entropy of the row, bit for bit what
 *      rwkv7_ce_fwd_bwd_ld_bf16 writes; lse_rows[row] = lse and max_rows[row] = m (fp32 [rows], each may be NULL; m is exact).  Rows
 *      with label == ignore_index are replaced by zeros and give 0 in all three outputs.  With z_coef = max_coef = 0 the logits are
 *      replaced by the bits rwkv7_ce_fwd_bwd_ld_bf16 writes.  Columns V .. ld - 1 are neither read nor written.  No LDS, no atomics,
 *      nothing shared between rows.  RWKV7_EINVAL, before any launch: a NULL logits / labels / loss_rows, rows <= 0, V <= 0, ld < V,
 *      label_smoothing outside [0, 1), z_coef or max_coef negative, infinite or a NaN. */
int rwkv7_ce_reg_fwd_bwd_bf16(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
                              float label_smoothing, float z_coef, float max_coef, float *lse_rows, float *max_rows,
                              rwkv7_stream_t stream);
/*      The backward of a per-SEQUENCE sum of log-probabilities (losses.fused_linear_seq_logprob): the plain cross-entropy gradient
 *      (label smoothing 0) of a chunk of logits [rows, ld] whose scale is looked up per row.  Row r of the chunk is row row0 + r of the
 *      batch; its sequence is the largest s < n_seq with seq_start[s] <= row0 + r, provided row0 + r < seq_start[n_seq] (seq_start:
 *      int64 [n_seq + 1] on the DEVICE, non-decreasing; equal neighbours are empty sequences).  The row is REPLACED by
 *      (softmax - onehot) * seq_scale[s] (seq_scale: fp32 [n_seq] on the DEVICE; the product is formed in fp32 and rounded to bf16
 *      once): bit for bit what rwkv7_ce_fwd_bwd_ld_bf16 writes with scale = seq_scale[s] and label_smoothing = 0.  Rows with
 *      label == ignore_index, rows in front of seq_start[0] and rows at or behind seq_start[n_seq] are replaced by zeros (finite
 *      logits).  loss_rows may be NULL; otherwise it receives what rwkv7_ce_fwd_bwd_ld_bf16 writes, for every row of the chunk
 *      whatever its sequence.  Columns V .. ld - 1 are neither read nor written.  seq_start is NOT range-checked beyond that.  No
 *      atomics, nothing shared between rows.  RWKV7_EINVAL, before any launch: a NULL logits / labels / seq_start / seq_scale,
 *      rows <= 0, V <= 0, ld < V, row0 < 0, n_seq <= 0. */
int rwkv7_ce_seq_bwd_bf16(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, long row0, long n_seq,
                          const long *seq_start, const float *seq_scale, float *loss_rows, rwkv7_stream_t stream);
/*      The token-level clipped policy objective (PPO-clip / GRPO; losses.fused_linear_policy) of a chunk of logits [rows, ld], loss
 *      terms and d loss / d logits in one pass: the same kernel with the scale computed per ROW.  Rows, sequences, row0 and seq_start
 *      as in rwkv7_ce_seq_bwd_bf16.  adv, seq_w: fp32 [n_seq] on the DEVICE (a sequence's advantage A and the weight w of each of its
 *      rows); old_lp, ref_lp: fp32 on the DEVICE, indexed by the BATCH row row0 + r (at least seq_start[n_seq] entries; read only for
 *      rows that count); ref_lp may be NULL (no KL term, whatever beta says).  For a row that counts -- label != ignore_index, inside
 *      [seq_start[0], seq_start[n_seq]) -- with lp = logit[label] - logsumexp in fp32 and the rest in double from it:
 *        rho = exp(lp - old_lp);  s1 = rho A;  s2 = clamp(rho, 1 - eps_lo, 1 + eps_hi) A;  active = s1 <= s2 (ties are active; a NaN
 *        takes the s1 branch and stays a NaN);  l = -min(s1, s2);  coef = active ? s1 : 0
 *        with ref_lp:  d = ref_lp - lp;  kl = exp(d) - d - 1 (the k3 estimator);  l += beta kl;  coef -= beta (1 - exp(d))
 *      The row is REPLACED by (softmax - onehot) * (float)(w coef): the product formed in fp32 and rounded to bf16 once.  Without
 *      ref_lp and at rho = 1 that is bit for bit what rwkv7_ce_seq_bwd_bf16 writes with seq_scale = the fp32 product w A.  Per-row
 *      outputs, fp32 [rows] indexed by the CHUNK row r, each may be NULL: lp_rows = lp, loss_rows = l (unweighted), kl_rows = kl (0
 *      without ref_lp), clip_rows = 1.0 where not active, else 0.0.  Every other row is replaced by zeros and gets zeros in the four
 *      outputs.  Columns V .. ld - 1 are neither read nor written.  Labels and seq_start are NOT range-checked on the device.  No LDS,
 *      no atomics, nothing shared between rows, no host read.  RWKV7_EINVAL, before any launch: a NULL logits / labels / seq_start /
 *      adv / seq_w / old_lp, rows <= 0, V <= 0, ld < V, row0 < 0, n_seq <= 0, eps_lo outside [0, 1), eps_hi < 0 (or either a NaN). */
int rwkv7_ce_policy_fwd_bwd_bf16(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, long row0, long n_seq,
                                 const long *seq_start, const float *adv, const float *seq_w, const float *old_lp, const float *ref_lp,
                                 float eps_lo, float eps_hi, float beta, float *lp_rows, float *loss_rows, float *kl_rows,
                                 float *clip_rows, rwkv7_stream_t stream);
/* ---- Cosy head loss: label-smoothing KL loss (cosyvoice/transformer/label_smoothing_loss.py:68-96), its gradient and the accuracy
 *      flag (cosyvoice/utils/common.py:76-95) of a chunk of bf16 logits [rows, ld] in one pass.  Columns V .. ld - 1 are neither read
 *      nor written.  dlogits (bf16 [rows, ld]) MAY be the same pointer as logits (in place); otherwise the logits are left intact.
 *      Target distribution of a row with label y: t_y = 1 - s, t_j = s / (V - 1) for j != y, s = smoothing in [0, 1).  With lse the
 *      log-sum-exp of the row's V logits:
 *        loss_rows[row]    = C - (1 - s)(x_y - lse) - s/(V-1) ((sum_j x_j - x_y) - (V-1) lse),
 *                            C = (1-s) ln(1-s) + s ln(s/(V-1)) with 0 ln 0 = 0, computed by this entry on the HOST in double and handed
 *                            to the kernel as a float
 *        dlogits[row][j]   = (softmax_j - t_j) * scale, rounded to bf16 once from the fp32 value
 *        correct_rows[row] = 1 if the LOWEST index among the row's maxima equals y, else 0 (torch.argmax's rule on the CPU; exact ties
 *                            are common in bf16 logits)
 *      Rows with label == ignore_index give loss_rows = 0, correct_rows = 0 and dlogits = 0.  Reductions run in fp32 from the bf16
 *      logits with the running maximum subtracted before exp.  Labels must be ignore_index or lie in [0, V): they are NOT checked on the
 *      device (the kernel indexes x[label]).  RWKV7_EINVAL, before any launch: a NULL pointer, rows <= 0, V < 2, ld < V, smoothing
 *      outside [0, 1).  Fastest when logits and dlogits agree modulo 16 bytes (always true in place) and V <= 8192 (the row stays in
 *      registers: one read, one write); any V, ld >= V and alignment is correct. ---- */
int rwkv7_kl_acc_fwd_bwd_bf16(long rows, int V, long ld, const void *logits, void *dlogits, const long *labels, long ignore_index,
                              float smoothing, float scale, float *loss_rows, int *correct_rows, rwkv7_stream_t stream);
/* ---- head metrics for held-out evaluation: ONE read-only pass over a chunk of bf16 head logits [rows, ld].  Nothing is written to
 *      the logits; columns V .. ld - 1 are never read.  No gradient is formed.
 *        kind = 0 : cross-entropy with label smoothing, the formula of rwkv7_ce_fwd_bwd_ls_bf16 (smoothing = 0: plain CE)
 *        kind = 1 : the Cosy label-smoothing KL, the formula of rwkv7_kl_acc_fwd_bwd_bf16; its constant C is computed by this entry on
 *                   the HOST in double and handed to the kernel as a float, as that entry does
 *        loss_rows[row]    = the row's loss; BIT-IDENTICAL to what rwkv7_ce_fwd_bwd_ld_bf16 (kind 0) / rwkv7_kl_acc_fwd_bwd_bf16
 *                            (kind 1, in place) write for the same logits at the same address modulo 16 bytes, labels and smoothing:
 *                            the fp32 row reduction runs in the training kernel's order
 *        correct_rows[row] = 1 if the LOWEST index among the row's maxima equals the label, else 0 (the KL entry's rule)
 *        argmax_rows[row]  = that lowest index; may be NULL; written for ignored rows too
 *      Rows with label == ignore_index give loss_rows = 0 and correct_rows = 0.  Reductions run in fp32 from the bf16 logits with the
 *      running maximum subtracted before exp.  Labels must be ignore_index or lie in [0, V): they are NOT checked on the device (the
 *      kernel indexes x[label]).  RWKV7_EINVAL, before any launch: a NULL logits / labels / loss_rows / correct_rows, rows <= 0, V < 2,
 *      ld < V, kind outside {0, 1}, smoothing outside [0, 1).  A wave per row; fastest on 16-byte aligned rows (16-byte loads, one
 *      trip through HBM); any V >= 2, ld >= V and 2-byte alignment of the base pointer is correct. ---- */
int rwkv7_head_eval_bf16(long rows, int V, long ld, const void *logits, const long *labels, long ignore_index, int kind, float smoothing,
                         float *loss_rows, int *correct_rows, int *argmax_rows, rwkv7_stream_t stream);
/* ---- per-sequence scores from the per-row outputs of rwkv7_head_eval_bf16: ONE launch after the last chunk of a batch, over the
 *      full-length loss_rows / correct_rows / labels (16 bytes per row; the logits are never kept).  Sequence s owns rows
 *      seq_start[s] .. seq_start[s + 1] - 1 (seq_start: int64 [n_seq + 1] on the DEVICE, non-decreasing); over its rows with
 *      label != ignore_index:
 *        loss_sum[s]   = the sum of loss_rows, accumulated in fp64
 *        tokens[s]     = the number of such rows;   correct[s] = the sum of correct_rows over them
 *        worst_loss[s] = the maximum of loss_rows (a NaN counts as the largest, as torch.max / torch.argmax take it)
 *        worst_row[s]  = the LOWEST row index, relative to seq_start[s], that attains worst_loss
 *      A sequence with no such row (an empty range included) gives 0, 0, 0, 0.0f, -1.
 *      FIXED summation order, a function of the sequence's length alone -- not of the grid, of n_seq, of which workgroup takes the
 *      sequence or of how the rows were chunked upstream: one 256-thread workgroup per sequence; thread t adds rows t, t + 256, ... in
 *      ascending order into one fp64 partial; an xor butterfly (32 .. 1) combines a wave; waves 0, 1, 2, 3 are added in that order
 *      through LDS.  No atomics, nothing shared between workgroups; the results are stored by one thread.
 *      seq_start is device data and is NOT range-checked: every row in [seq_start[s], seq_start[s + 1]) is read (a decreasing pair is
 *      an empty sequence).  RWKV7_EINVAL, before any launch: a NULL pointer, n_seq <= 0 or n_seq >= 2^31. ---- */
int rwkv7_seq_scores_f32(long n_seq, const long *seq_start, const float *loss_rows, const int *correct_rows, const long *labels,
                         long ignore_index, double *loss_sum, long *tokens, long *correct, float *worst_loss, long *worst_row,
                         rwkv7_stream_t stream);

/* ---- optimizer step (train_spark_rwkv7speech.py:178-197; torch.optim.AdamW update rule, decoupled weight decay) on a
 *      flat parameter buffer: fp32 master weights p32 and moments m, v updated in place from bf16 gradients g16; the
 *      bf16 working copy p16 is rewritten in the same pass.  n % 4 == 0; step = 1 for the first update. ---- */
int rwkv7_adamw_bf16(long n, float *p32, const void *g16, float *m, float *v, void *p16, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, rwkv7_stream_t stream);
/*      Parameter groups (train_scripts/train_cosy_rwkv7speech_multiple_dataset.py:162-202: `lr_2x` for
 *      'attn.w_lora.lora.2.bias', a weight-decay group for >= 2-D non-LoRA `.weight`, `my_lr_scale`): slab_group[n / 128]
 *      (uint8, one entry per 128 consecutive elements -- the host aligns every parameter to 128 elements) indexes
 *      group_tab[ngroups][2] = {lr scale, weight decay}, both in device memory; both NULL = one group {1, 0}.
 *      skip_flag: device float or NULL; != 0 makes the step run on a zero gradient (the reference's NaN-loss step,
 *      train_spark_rwkv7speech.py:664-687) without the host ever reading the flag.  n % 128 == 0 with groups. ---- */
int rwkv7_adamw_groups_bf16(long n, float *p32, const void *g16, float *m, float *v, void *p16, const unsigned char *slab_group,
                            const float *group_tab, int ngroups, const float *skip_flag, float lr, float beta1, float beta2,
                            float eps, int step, rwkv7_stream_t stream);
/*      The same step with gradient clipping by global norm (the reference hands `gradient_clipping` to DeepSpeed,
 *      train_scripts/train_rwkv_tts.py:133,405; third_party/cosyvoice/utils/train_utils.py:283-291 calls clip_grad_norm_):
 *      coef = min(1, max_norm / (sqrt(*sumsq) + 1e-6)), computed per launch from the DEVICE scalar sumsq (the sum of squares of
 *      the whole gradient, rwkv7_grad_sumsq_bf16 -- not only of the n elements of this call); the gradient is multiplied by coef
 *      in fp32 right after the bf16 load, and only when coef < 1: with coef == 1 the arithmetic is that of
 *      rwkv7_adamw_groups_bf16.  A non-finite *sumsq acts like skip_flag != 0 (zero-gradient step, nothing becomes NaN).
 *      max_norm >= 0; +inf = measure only.  The host reads neither sumsq nor skip_flag. */
int rwkv7_adamw_groups_clip_bf16(long n, float *p32, const void *g16, float *m, float *v, void *p16, const unsigned char *slab_group,
                                 const float *group_tab, int ngroups, const float *skip_flag, const float *sumsq, float max_norm,
                                 float lr, float beta1, float beta2, float eps, int step, rwkv7_stream_t stream);

/* ---- passes over a flat bf16 gradient buffer (n % 128 == 0, pointers 16-byte aligned; the trainer's slices are 256-byte
 *      aligned).  No atomics anywhere: two calls on the same data give the same bits.
 *      rwkv7_grad_sumsq_bf16: out[0] = (accumulate ? out[0] : 0) + sum g16[i]^2.  Two launches: one workgroup per FIXED tile of
 *      8192 elements (fp32, one partial per tile into `partials`, rwkv7_grad_sumsq_workspace_bytes(n) bytes), then one
 *      workgroup that adds the partials in double in a fixed order.  A NaN or Inf in g16 gives a non-finite out[0]. */
long rwkv7_grad_sumsq_workspace_bytes(long n);
int rwkv7_grad_sumsq_bf16(long n, const void *g16, float *partials, float *out, int accumulate, rwkv7_stream_t stream);
/*      Micro-batch accumulation in fp32 (`accum_grad`, train_utils.py:87-89; DeepSpeed's bf16 engine accumulates in fp32):
 *      rwkv7_grad_accum_bf16: acc32 = (first ? 0 : acc32) + float(g16)   (first: acc32 is not read, float(g16) is stored as it is);
 *      rwkv7_grad_fold_bf16:  g16 = bf16_rne((acc32 + float(g16)) * inv_count) in place -- the last micro-batch's gradient joins
 *      the sum here, and the only rounding to bf16 is this one. */
int rwkv7_grad_accum_bf16(long n, float *acc32, const void *g16, int first, rwkv7_stream_t stream);
int rwkv7_grad_fold_bf16(long n, const float *acc32, void *g16, float inv_count, rwkv7_stream_t stream);

/* ---- position-sensitive 64-bit digest of a device buffer of n_words 32-bit words whose first word has the GLOBAL index
 *      first_index (trainer checkpoints: the buffers in memory after a load are the buffers that were saved; replica check):
 *          x_i  = (uint64)w[i] + (first_index + i + 1) * 0x9E3779B97F4A7C15
 *          x_i ^= x_i >> 30;  x_i *= 0xBF58476D1CE4E5B9;  x_i ^= x_i >> 27;  x_i *= 0x94D049BB133111EB;  x_i ^= x_i >> 31
 *          out[0] = (accumulate ? out[0] : 0) + sum_i x_i                               (all of it mod 2^64)
 *      Exact integer arithmetic: the same 64 bits on every call and in a numpy uint64 restatement.  Additive over disjoint index
 *      ranges: the digest of a buffer is the wrapping sum of the digests of its slabs, each with its own first_index.  The digest
 *      of all-zero words is not zero, and exchanging two unequal words changes it.  Two launches, no atomics: one workgroup per
 *      FIXED tile of 8192 words (16-byte loads, one uint64 partial per tile into `partials`, the workspace query's byte count),
 *      then one workgroup that adds the partials.  buf is only read.  n_words % 4 == 0, buf 16-byte aligned (RWKV7_ESHAPE
 *      otherwise, nothing launched); n_words == 0 is allowed (buf and partials may then be NULL).  64-bit indices throughout. ---- */
long rwkv7_buf_digest_workspace_bytes(long n_words);
int rwkv7_buf_digest_u32(long n_words, long first_index, const void *buf, unsigned long long *partials, unsigned long long *out,
                         int accumulate, rwkv7_stream_t stream);
/*      Snapshot and digest in one pass (the trainer's non-blocking checkpoints: a consistent copy of a state buffer that the next
 *      step will overwrite, and the proof of what was copied): dst[0..n_words) = src[0..n_words) bit for bit, and out[0] is exactly
 *      the word rwkv7_buf_digest_u32(n_words, first_index, src, ...) gives, `accumulate` included.  Same two launches, same tiles
 *      and the same workspace (rwkv7_buf_digest_workspace_bytes) as that entry; each 16-byte piece is stored to dst with a plain
 *      vector store from the registers it is then mixed from, so the digest is of the words that were written.  Words of dst at
 *      and behind n_words are never written, src is only read.  Bytes moved: one read and one write of the buffer (a copy followed
 *      by the digest entry reads it twice and writes it once).  Checked here, nothing launched otherwise: n_words % 4 == 0, src and
 *      dst 16-byte aligned (RWKV7_ESHAPE); src, dst, partials non-NULL when n_words > 0, out non-NULL, nothing negative, and
 *      [src, src + 4 n_words) must not overlap [dst, dst + 4 n_words) (RWKV7_EINVAL).  n_words == 0 stores nothing and sets out[0]
 *      as the digest entry does.  The caller keeps both buffers alive and orders other writers of dst by the stream. */
int rwkv7_buf_snapshot_digest_u32(long n_words, long first_index, const void *src, void *dst, unsigned long long *partials,
                                  unsigned long long *out, int accumulate, rwkv7_stream_t stream);

/* ---- last step of a split weight gradient (the dW of nn.Linear under autograd, e.g. rwkv_s2s_single_ffn.py:171-174,195,
 *      228-229, reduced over B*T in S row slabs with fp32 partials): out[n] (bf16) = (accumulate ? out[n] : 0) +
 *      sum_s parts[s][n].  out may be the parameter's slice of the flat gradient buffer.  n % 4 == 0. ---- */
int rwkv7_sum_slabs_bf16(long n, int S, const float *parts, void *out, int accumulate, rwkv7_stream_t stream);
/*   out[C][R] = in[R][C]^T, 16-bit elements, R % 64 == 0 and C % 64 == 0: the NT operand W_value^T of the channel-mix backward's
 *   input-gradient GEMM (rwkv7_gemm_nt_relusq_bwd_s_bf16; autograd of rwkv_s2s_single_ffn.py:229). */
int rwkv7_transpose_bf16(int R, int C, const void *in, void *out, rwkv7_stream_t stream);
/*   out[r][0..D) = idx[r] >= 0 ? src[idx[r]][0..D) : 0 for r < n_out -- 16-bit rows, D % 8 == 0, idx int32 on the device.  The re-layout
 *   of a packed `cu_seqlens` row (train_spark_rwkv7speech.py:238-239, data/utils/spark_dataset.py:111-162) into the 32-aligned row the
 *   chunked WKV7 kernels walk, and back: the maps are injective, so forward and backward of both directions are this one gather. */
int rwkv7_gather_rows_bf16(long n_out, int D, const void *src, const int *idx, void *out, rwkv7_stream_t stream);
/*   Weight gradient of a low-rank projection (rwkv_s2s_single_ffn.py:172-184, autograd of x @ w1 / h @ w2): for y = x W^T,
 *   parts[s][N][K] (fp32) = dy[slab s][N]^T x[slab s][K], slab = M / S consecutive rows (a multiple of 128); one of N, K is the
 *   rank (32, 64 or 128), the other a multiple of 256.  bf16 operands, fp32 accumulation on MFMA; finish with
 *   rwkv7_sum_slabs_bf16(N * K, S, parts, dW, 0). */
int rwkv7_wgrad_skinny_bf16(long M, int N, int K, int S, const void *dy, const void *x, float *parts, rwkv7_stream_t stream);
/*   wgrad_mid: the same partials for the [W_a ; W_b] gradient of the through-the-lerp projections (dy = dG [M][N], N = 2 R in {512, 576};
 *   K a multiple of 256; rows per slab a multiple of 64): neither side is skinny, a workgroup holds a [N / 2][256] fp32 tile. */
int rwkv7_wgrad_mid_bf16(long M, int N, int K, int S, const void *dy, const void *x, float *parts, rwkv7_stream_t stream);
/*   wgrad_tn: the same partials for the dense projections (r / k / v / o and the channel-mix key / value, autograd of
 *   rwkv_s2s_single_ffn.py:171-174, 195, 228-229): N and K multiples of 256, rows per slab a multiple of 128 (RWKV7_ESHAPE otherwise,
 *   nothing is launched); a workgroup holds a 256 x 256 fp32 tile and reads both operands token-major (csrc/wgrad_tn.hip). */
int rwkv7_wgrad_tn_bf16(long M, int N, int K, int S, const void *dy, const void *x, float *parts, rwkv7_stream_t stream);

/* ---- C[M][N] = epi(A[M][K] . W[N][K]^T), bf16, fp32 accumulation: the channel-mix key projection with its activation as
 *      the epilogue (epilogue 1: relu(.)^2, rwkv_s2s_single_ffn.py:228; 0: none).  Hand-written persistent MFMA kernel fed by
 *      LDS-DMA (csrc/gemm_nt4.hip); M, N multiples of 256, K of 1024 (RWKV7_ESHAPE otherwise); bit-identical to the library
 *      GEMM + rwkv7_relusq_fwd pair. ---- */
int rwkv7_gemm_nt_bf16(int M, int N, int K, const void *A, const void *W, void *C, int epilogue, rwkv7_stream_t stream);
/*      the backward of the activation as the epilogue of the value projection's input-gradient GEMM (round 4):
 *      C[M][N] = bf16(A[M][K] . W[N][K]^T) * 2 relu(aux[M][N]) -- A = dy, W = value.weight^T (contiguous [N = F][K = D]), aux = the key
 *      projection's output h: dh without ds ever reaching HBM and without rwkv7_relusq_bwd_*. */
int rwkv7_gemm_nt_relusq_bwd_bf16(int M, int N, int K, const void *A, const void *W, const void *aux, void *C, rwkv7_stream_t stream);
/*      the same from the activation's OUTPUT: C[M][N] = bf16(A . W^T) * 2 sqrt(s[M][N]), s = relu(h)^2 as written by rwkv7_gemm_nt_bf16 with
 *      epilogue 1 (what the library GEMM + rwkv7_relusq_bwd_s_* produce, bit for bit): with it the channel mix never materialises h or
 *      ds (fused.channel_mix).  csrc/gemm_nt4.hip only: K % 1024 == 0. */
int rwkv7_gemm_nt_relusq_bwd_s_bf16(int M, int N, int K, const void *A, const void *W, const void *s, void *C, rwkv7_stream_t stream);
/*      a projection with the residual add that follows it as the epilogue: C[M][N] = bf16(bf16(A . W^T) + resid[M][N]) -- the block wiring
 *      x = x + att(...) of rwkv_s2s_single_ffn.py:262-276 for the output projection (fused.linear_add); what nn.Linear followed by the
 *      add of the two bf16 tensors produces, bit for bit.  csrc/gemm_nt4.hip only: K % 1024 == 0.  C must not alias resid. */
int rwkv7_gemm_nt_add_bf16(int M, int N, int K, const void *A, const void *W, const void *resid, void *C, rwkv7_stream_t stream);
/*      All four entries run csrc/gemm_nt4.hip (four waves, quadrant phases, ring of eight half-tile LDS slots): M, N multiples of 256,
 *      K a multiple of 1024, RWKV7_ESHAPE otherwise.  The first-generation kernel (csrc/lab/gemm_relusq.hip, K % 64 == 0) lives in the lab
 *      build under its own entry points (include/rwkv7_hip_lab.h). */

/* ---- the low-rank branches of the time-mix block taken THROUGH the token-shift lerp (fused.mix_lora; rwkv_s2s_single_ffn.py:160-190):
 *      (xm (1 - mu) + shift(xm) mu) W1^T = xm (W1 * (1 - mu))^T + shift(xm) (W1 * mu)^T, so one GEMM G = x [W_a ; W_b]^T on the LayerNorm
 *      output ([M, D] x [D, 2 R]) replaces the mixed inputs x_w, x_a, x_v, x_g and their four Linear(D, r_i).  nb <= 4 branches with ranks
 *      r_i (multiples of 8, R = sum r_i), HOST arrays of device pointers, bf16.
 *   wcat_fwd:     wcat [2 R][D]: rows off_i .. = W1_i * (1 - mu_i), rows R + off_i .. = W1_i * mu_i           (W1_i [r_i][D], mu_i [D])
 *   wcat_bwd:     dW1_i = dW_a (1 - mu_i) + dW_b mu_i ;  dmu_i[c] = sum_rows W1_i (dW_b - dW_a)                from dwcat [2 R][D]
 *   combine_fwd:  out_i[t] = act_i(bf16(m_t G[t][off_i ..] + m_{t-1} G[t - 1][R + off_i ..])), nothing from t - 1 at the first step of a
 *                 sequence (rows are [B][T]); acts: 0 none, 1 tanh, 2 sigmoid; mask [M] or NULL; out_i [M][r_i]
 *   combine_bwd:  dG [M][2 R] from the activation OUTPUTS y_i and their gradients dy_i ---- */
int rwkv7_mix_lora_wcat_fwd_bf16(int nb, const int *ranks, const void *const *w1, const void *const *mu, int D, void *wcat,
                                 rwkv7_stream_t stream);
int rwkv7_mix_lora_wcat_bwd_bf16(int nb, const int *ranks, const void *const *w1, const void *const *mu, int D, const void *dwcat,
                                 void *const *dw1, void *const *dmu, rwkv7_stream_t stream);
int rwkv7_mix_lora_combine_fwd_bf16(int nb, const int *ranks, const int *acts, long M, int T, const void *G, const void *mask,
                                    void *const *out, rwkv7_stream_t stream);
int rwkv7_mix_lora_combine_bwd_bf16(int nb, const int *ranks, const int *acts, long M, int T, const void *mask, const void *const *y,
                                    const void *const *dy, void *dG, rwkv7_stream_t stream);

/* ---- the same low-rank branches' down projections with the lerp as the GEMM's A prologue (csrc/lora_down.hip; rwkv_s2s_single_ffn.py:160-190):
 *      out_i[t] = act_i(bf16( bf16(xm[t] + (xm[t - 1] - xm[t]) mu_i) W1_i^T )), xm = x * mask, nothing from t - 1 at the first step of a
 *      sequence (rows are [B][T]) -- the reference's own rounding points; one kernel streams x [M][D] once and writes every branch's
 *      [M][r_i].  nb <= 4 branches, ranks multiples of 32 with sum <= 512, D a multiple of 128 (<= 4096), M a multiple of 128 and of T.
 *   pack:  W1_i [r_i][D] -> packed [sum r_i][D] in MFMA fragment order (same bytes, one coalesced 1 KB wave load per fragment); once
 *          per weight update
 *   fwd:   acts: 0 none, 1 tanh, 2 sigmoid; mask [M] or NULL; mu / out: HOST arrays of device pointers (mu_i [D], out_i [M][r_i]).
 *      The gradient is the one of the through-the-lerp form above (combine_bwd, wcat_*). ---- */
int rwkv7_lora_down_pack_bf16(int nb, const int *ranks, const void *const *w1, int D, void *packed, rwkv7_stream_t stream);
int rwkv7_lora_down_fwd_bf16(int nb, const int *ranks, const int *acts, long M, int T, int D, const void *x, const void *mask,
                             const void *const *mu, const void *packed, void *const *out, rwkv7_stream_t stream);

/* ---- decode-step linear layers: y[M,N] = x[M,K] @ w[N,K]^T (+ bias[N]), bf16, M <= 32 rows (one token per sequence and
 *      step), K % 64 == 0.  Replaces the nn.Linear calls of the per-token path (rwkv_s2s_single_ffn.py:482-506,545-549)
 *      for the decode batch; weight-streaming on MFMA, see csrc/gemv32.hip.  bias may be NULL. ---- */
int rwkv7_gemv32_bf16(int M, int N, int K, const void *x, const void *w, const void *bias, void *y, rwkv7_stream_t stream);

/* ---- one whole decode step (T = 1, B <= 32 sequences, bf16 weights) in ONE persistent kernel: replaces the per-token loop
 *      body RWKV_x070.forward_one (model/llm/rwkv_s2s_single_ffn.py:417-445; TMix_one :482-506, CMix_one :545-549) /
 *      forward_batch at T = 1 (model/llm/rwkv_asr_cuda_whisper.py:438-472) including the final norm and the head
 *      projection.  See csrc/decode_step.hip.
 *
 *      layer_tbl: DEVICE array [L][RWKV7_DEC_COUNT] of device pointers in the order below (bf16 unless noted; entries a
 *      layer does not have -- LN0 outside layer 0, the v branch in layer 0 -- may be NULL).  Weights are torch/rwkvfla
 *      layouts: Linear [out,in], low-rank lora.0.weight [R,D] ("1"), lora.2.weight [D,R] ("2"), lora.2.bias [D] ("0").
 *      State tensors are updated in place: att_x_prev/ffn_x_prev bf16 [B,D], att_kv fp32 [B,H,64,64] (row = value index).
 *      x_in bf16 [B,D] = embeddings of the current tokens; logits fp32 [B,V] (head_b may be NULL).
 *      workspace: rwkv7_decode_workspace_bytes() bytes, 256-byte aligned, owned by the caller, reused step after step;
 *      its first 8 bytes are the barrier words {arrivals, timeout flag}: flag != 0 after a step means a grid barrier was not
 *      met within ~0.1 s (the kernel then exits instead of hanging; the step's results are invalid).
 *      persistent = 0: ordinary launches, one kernel per phase (a stream-ordered kernel boundary costs ~1.5 us).  persistent = 1
 *      (ONE launch, the same phase bodies separated by device-scope barriers; measured 7.4 us per barrier on MI355X -- 3.9 us of
 *      arrivals/polling on one counter plus 1.8 us L2 write-back and 1.6 us invalidate, the XCD L2s not being coherent -- 2.4 ms per
 *      step) exists in the lab build only (python -m rwkvtts_amd.build --lab): the shipped library answers RWKV7_ESHAPE.
 *      Errors: RWKV7_ESHAPE unless B in [1,32], D = 64 H <= 4096, F % 64 == 0, every rank a multiple of 32 and <= 256, ranks sum <= 512. */
enum {
    RWKV7_DEC_LN0_W, RWKV7_DEC_LN0_B, RWKV7_DEC_LN1_W, RWKV7_DEC_LN1_B, RWKV7_DEC_LN2_W, RWKV7_DEC_LN2_B,
    RWKV7_DEC_XR, RWKV7_DEC_XW, RWKV7_DEC_XK, RWKV7_DEC_XV, RWKV7_DEC_XA, RWKV7_DEC_XG,
    RWKV7_DEC_WR, RWKV7_DEC_WK, RWKV7_DEC_WV, RWKV7_DEC_WO,
    RWKV7_DEC_W1, RWKV7_DEC_W2, RWKV7_DEC_W0, RWKV7_DEC_A1, RWKV7_DEC_A2, RWKV7_DEC_A0,
    RWKV7_DEC_V1, RWKV7_DEC_V2, RWKV7_DEC_V0, RWKV7_DEC_G1, RWKV7_DEC_G2,
    RWKV7_DEC_KK, RWKV7_DEC_KA, RWKV7_DEC_RK, RWKV7_DEC_GNW, RWKV7_DEC_GNB,
    RWKV7_DEC_FXK, RWKV7_DEC_WKEY, RWKV7_DEC_WVAL,
    RWKV7_DEC_ATT_XPREV, RWKV7_DEC_ATT_KV /* fp32 */, RWKV7_DEC_FFN_XPREV,
    RWKV7_DEC_COUNT
};
typedef struct rwkv7_decode_dims {
    int B, D, H, L, F, V;      /* sequences, hidden, heads, layers, channel-mix width, head rows */
    int Rw, Ra, Rv, Rg;        /* low-rank sizes of the decay / a / value-residual / gate branches */
    float ln_eps, gn_eps;      /* LayerNorm eps; GroupNorm eps (64e-5, rwkv_s2s_single_ffn.py:504) */
} rwkv7_decode_dims;
int rwkv7_decode_layer_ptrs(void);   /* == RWKV7_DEC_COUNT of the library that was loaded */
size_t rwkv7_decode_workspace_bytes(const rwkv7_decode_dims *dims);   /* 0: unsupported shape */
int rwkv7_decode_step_bf16(const rwkv7_decode_dims *dims, const void *const *layer_tbl, const void *x_in, const void *norm_w,
                           const void *norm_b, const void *head_w, const void *head_b, float *logits, void *workspace,
                           int persistent, rwkv7_stream_t stream);
/* the same step for a caller that also holds the table in HOST memory (layer_tbl_host: the same [L][RWKV7_DEC_COUNT] addresses,
 * read during the call only): with persistent = 0 every phase kernel then receives its 1-13 pointers as kernel arguments instead of
 * fetching its table row first -- one dependent load less at the head of each of the 7 L + 2 launches (0.3-0.4 us each, measured).
 * Results are bit-identical to rwkv7_decode_step_bf16. */
int rwkv7_decode_step_tbl_bf16(const rwkv7_decode_dims *dims, const void *const *layer_tbl, const void *const *layer_tbl_host,
                               const void *x_in, const void *norm_w, const void *norm_b, const void *head_w, const void *head_b,
                               float *logits, void *workspace, int persistent, rwkv7_stream_t stream);
/* the same step for B = 33 .. 128 sequences (csrc/decode_step_wide.hip): RT = ceil(B / 32) row tiles of 32, one launch per phase, and
 * every weight is streamed ONCE per step -- a GEMV item loads its weight fragments once per k-step and multiplies them against the RT
 * activation tiles in registers.  Same layer_tbl, tensors and in-place state as above with B rows; layer_tbl_host may be NULL (the
 * phase kernels then read their row of the device table).  Rows 32 g .. 32 g + 31 get bit for bit what rwkv7_decode_step_bf16 gives a
 * batch made of those rows; rows >= B of logits and state are never written.  workspace: rwkv7_decode_wide_workspace_bytes() bytes
 * (the same for every B of one row tile; 0 for B <= 32, B > 128 or an uncovered shape), 256-byte aligned, owned by the caller.  There
 * is no persistent variant.  Errors: as above with B in [33,128]; the arguments are checked before the first launch. */
size_t rwkv7_decode_wide_workspace_bytes(const rwkv7_decode_dims *dims);
int rwkv7_decode_step_wide_bf16(const rwkv7_decode_dims *dims, const void *const *layer_tbl, const void *const *layer_tbl_host,
                                const void *x_in, const void *norm_w, const void *norm_b, const void *head_w, const void *head_b,
                                float *logits, void *workspace, rwkv7_stream_t stream);

/* ---- token draws of the generation loops, one launch each (csrc/sampling.hip).
 *
 * rwkv7_sample_rows_f32: for every row r < rows and segment s < nseg one id from logits[r * ld + seg_off[s] .. + seg_len[s])
 *      (fp32), restricted to the ids [allow_lo[s], allow_hi[s]) of the segment (NULL: the whole segment) and never one of
 *      `suppress` (segment-relative ids, nsuppress <= 256).  do_sample = 0: argmax (first maximum).  do_sample = 1: the warper
 *      chain the reference's generate() runs (HF temperature -> top-k -> top-p -> softmax -> multinomial; utils/utilities.py:101-117,
 *      model/llm/xy_llm.py:88-101 for the eight channels of a frame): top_k in [1, 64] with any top_p in (0, 1], or top_k = 0 with
 *      top_p = 1 (plain multinomial); temperature > 0.  seg_off / seg_len / allow_* / suppress are DEVICE int arrays; max_domain =
 *      the largest allow_hi - allow_lo (or seg_len), <= 15360.  out: [rows][nseg] int64 ids (segment-relative).
 *      Randomness: Philox4x32-10 keyed by `seed`, counter (*step, workgroup): `step` is a DEVICE int64 the caller advances between
 *      calls (the position counter of the decode loop), so a captured launch draws fresh ids on every replay and (seed, *step)
 *      fixes them.  RWKV7_ESHAPE for parameter combinations outside the above (the Python host then runs the torch chain).  At most
 *      128 candidates survive top-k: a row with more than 128 ids tied at the k-th value keeps the 128 smallest of them.
 * rwkv7_ras_step_f32: one token of CosyVoice's streaming loop (B = 1): ras_sampling (third_party/cosyvoice/utils/common.py:109-137:
 *      nucleus top_p / top_k, and random_sampling when the candidate already occurs >= win_size * tau_r times in `recent`) with the
 *      EOS rejection of sampling_ids (model/llm/llm.py:160-176) while *step_i < n_ignore, followed by the loop's bookkeeping:
 *      *tok = id; if id != eos: recent[*ptr] = id, *ptr = (*ptr + 1) % win_size; *step_i += 1.  logits fp32 [V] (any shift of the
 *      log-probabilities), V <= 15360, top_k <= 128, win_size <= 128; tok / recent [win_size] / ptr / step_i DEVICE int64. */
int rwkv7_sample_rows_f32(int rows, int nseg, const float *logits, long ld, const int *seg_off, const int *seg_len, const int *allow_lo,
                          const int *allow_hi, const int *suppress, int nsuppress, int max_domain, int do_sample, int top_k, float top_p,
                          float temperature, unsigned long long seed, const long *step, long *out, rwkv7_stream_t stream);
/* the one-segment draw followed by what the decode loop does with the id (decode.GraphDecoder._step; the reference's generate():
 * finished sequences emit `pad`, `eos` ends a sequence, the id is stored in the output row at column *step and is the next input):
 * unfinished [rows] bytes or NULL (no EOS handling), ids [rows] (required), seq [rows][seq_ld] or NULL, emb bf16 [V][D] + x bf16
 * [rows][D] or NULL: the embedding row of the id is copied to x, where the next decode step reads its input.  tail may be NULL
 * (the draw alone).  min_eos_id >= 0: that id cannot be drawn while *step < min_eos_until (min_new_tokens of the reference's
 * generate(): utils/utilities.py:106). */
typedef struct rwkv7_sample_tail {
    unsigned char *unfinished;
    long eos, pad;
    long *ids;
    long *seq;
    long seq_ld;
    const void *emb;
    void *x;
    int D;
} rwkv7_sample_tail;
int rwkv7_sample_rows_tail_f32(int rows, const float *logits, long ld, const int *seg_off, const int *seg_len, const int *allow_lo,
                               const int *allow_hi, const int *suppress, int nsuppress, int max_domain, int do_sample, int top_k, float top_p,
                               float temperature, unsigned long long seed, const long *step, long *out, const rwkv7_sample_tail *tail,
                               int min_eos_id, long min_eos_until, rwkv7_stream_t stream);
/* rwkv7_sample_slots_f32: the one-segment draw + decode-loop bookkeeping per SLOT of a continuous-batching engine
 * (rwkvtts_amd/continuous.py), where every slot runs its own request.  Logits row r belongs to slot s = row_slot[r] (row_slot NULL:
 * s = r; rows with s outside [0, slots) are skipped).  A slot with live[s] == 0 is left untouched (x[s] keeps its row).  A live
 * slot draws one id with its own do_sample / inv_temp / top_k / top_p, EOS barred while step[s] < min_until[s], from the ids
 * [allow_lo[0], allow_hi[0]) of the row (NULL: the first max_domain columns) minus `suppress`; Philox key seed[s], counter
 * (step[s], 0): the id is bit-identical to a ONE-row rwkv7_sample_rows_tail_f32 call with *step = step[s] and the same key,
 * parameters (temperature = 1 / inv_temp) and logits.  Then seq[s][step[s]] = id (if step[s] < seq_ld), ids[s] = id,
 * x[s] = emb[id] (emb NULL: no copy), step[s] += 1, live[s] = id != eos && step[s] < limit[s].  All per-slot fields are DEVICE
 * arrays of `slots` entries; eos < 0: no EOS.  top_k_max (host): the largest top_k[] value, in [0, 64]; a slot's top_k is
 * clamped to it.  A sampled slot with top_k = 0 draws from the whole distribution (top_p is ignored there).  Errors:
 * RWKV7_EINVAL for rows <= 0, a null st / logits / per-slot array, seq_ld <= 0, slots <= 0, emb without x; RWKV7_ESHAPE for
 * max_domain > 15360, nsuppress > 256, top_k_max outside [0, 64], D % 8 != 0. */
typedef struct rwkv7_slot_state {
    long *step;                 /* ids emitted so far = output column of the next id */
    long *limit;                /* max_new_tokens of the slot's request */
    long *min_until;            /* EOS barred while step < min_until (0: none) */
    unsigned long long *seed;   /* the request's Philox key */
    float *inv_temp;
    int *top_k;
    float *top_p;
    unsigned char *do_sample;
    unsigned char *live;        /* 1 while the slot's request runs */
    long *ids;                  /* next input id */
    long *seq;                  /* [slots][seq_ld] generated ids */
    long seq_ld;
    const void *emb;            /* bf16 [V][D] embedding table, or NULL */
    void *x;                    /* bf16 [slots][D]: the next decode step's input */
    int D;
    int slots;
    int top_k_max;
    long eos;
} rwkv7_slot_state;
int rwkv7_sample_slots_f32(int rows, const float *logits, long ld, const int *row_slot, const int *allow_lo, const int *allow_hi,
                           const int *suppress, int nsuppress, int max_domain, const rwkv7_slot_state *st, rwkv7_stream_t stream);
/* rwkv7_sample_slots_lp_f32: rwkv7_sample_slots_f32 that also reports the log-probability of every id it draws
 * (ContinuousDecoder(logprobs=True): ranking n candidates of one text without a second, teacher-forced pass).  For a live slot
 * every field of `st` is written bit for bit as rwkv7_sample_slots_f32 writes it, and in addition
 *   tok_lp[s][step[s]] = x[id] - max - log sum_j exp(x[j] - max)     (if step[s] < seq_ld; row stride seq_ld, like seq)
 *   cum_lp[s]         += (double)tok_lp[s][step[s]]                  (plain read, add, store: one workgroup owns a slot)
 * with x the RAW fp32 logits -- temperature 1, before top-k / top-p -- and j over the ids the draw could have produced at this
 * step: the allowed range minus `suppress`, minus EOS while step[s] < min_until[s].  If no id is allowed (the draw falls back to
 * the first id of the range) the value is -INFINITY.  A slot that is not live, and a row whose slot is outside [0, slots), leave
 * tok_lp and cum_lp untouched.  The reductions run thread -> wave -> workgroup in a fixed order: the same logits row gives the same
 * bits whatever row, slot or grid it is drawn in.  Errors: those of rwkv7_sample_slots_f32, and RWKV7_EINVAL for a null lp,
 * lp->tok_lp or lp->cum_lp; nothing is launched then.
 * (Declared as a struct plus a typedef, which a C compiler reads like the one-piece typedefs above; its Python mirror,
 * continuous.SlotLogprob, is checked against the compiler's layout in tests/test_best_of_abi.py.) */
struct rwkv7_slot_logprob {
    float *tok_lp;              /* [slots][seq_ld] log-probability of every drawn id */
    double *cum_lp;             /* [slots] running sum of the slot's tok_lp, in step order */
};
typedef struct rwkv7_slot_logprob rwkv7_slot_logprob;
int rwkv7_sample_slots_lp_f32(int rows, const float *logits, long ld, const int *row_slot, const int *allow_lo, const int *allow_hi,
                              const int *suppress, int nsuppress, int max_domain, const rwkv7_slot_state *st,
                              const rwkv7_slot_logprob *lp, rwkv7_stream_t stream);
int rwkv7_ras_step_f32(int V, const float *logits, long *tok, long *recent, long *ptr, long *step_i, long n_ignore, int eos, float top_p,
                       int top_k, int win_size, float tau_r, unsigned long long seed, rwkv7_stream_t stream);

/* ---- one frame of the XY generation loop (model/llm/xy_llm.py:39-146, CustomGenerationMixin._sample) after the eight draws:
 * rwkv7_xy_frame_step: flush countdown, EOS / pad substitution, append of the row, stopping criteria and the `all finished` flag for
 *      B <= 64 sequences of C channels, on DEVICE int64 state (out [B][rows][C], row [B][C] = the row just written, pos / n_rows
 *      scalars, unfinished / needs [B], all_done one byte), from the drawn ids nt [B][C] (channel 0 in vocabulary ids).  eos0 < 0:
 *      no EOS id; total < 0: no length bound; eos_list: n_eos DEVICE ids for the stopping criterion; reference_termination = 1
 *      reproduces lines :139-140 literally.  The torch form of the same rules is rwkvtts_amd/xy_llm.py _XYFrameState.step.
 * rwkv7_xy_embed_bf16: x[b] = sum_c table_c[row[b][c]] (bf16 rows of D, added in channel order with bf16 rounding after every
 *      addition, like the module's chain of tensor additions; xy_llm.py:189-200); tables_host: HOST array of C <= 16 DEVICE pointers. */
int rwkv7_xy_frame_step(int B, int C, int rows, long text_shift, long speech_vocab, long pad, long eos0, long total, const long *eos_list,
                        int n_eos, int reference_termination, const long *nt, long *out, long *row, long *pos, long *unfinished, long *needs,
                        unsigned char *all_done, long *n_rows, rwkv7_stream_t stream);
int rwkv7_xy_embed_bf16(int B, int C, int D, const void *const *tables_host, const long *row, void *x, rwkv7_stream_t stream);

/* ---- one XY frame per SLOT of a continuous-batching engine (csrc/xy_slots.hip; rwkvtts_amd/continuous_xy.py), where every slot runs
 * its own request.  Logits row r belongs to slot s = row_slot[r] (row_slot NULL: s = r; rows with s outside [0, slots) are skipped;
 * the named slots must be distinct).  A slot with live[s] == 0 is left completely untouched by both entries: nt, x, row, needs,
 * step and seq keep their contents.  A frame is the two calls in this order on one stream:
 * rwkv7_xy_slots_draw_f32: for every live slot and channel c < C one id from logits[r * ld + seg_off[c] .. + seg_len[c]) restricted
 *      to the ids [allow_lo[c], allow_hi[c]) of the segment (NULL: whole segments), with the slot's own do_sample / inv_temp / top_k /
 *      top_p; seg_off may be negative when the row holds only the allowed part of a segment (channel 0: the audio range of the text
 *      head), so that ids keep their vocabulary values.  Philox key seed[s], counter (step[s], c): the C ids are bit-identical to a
 *      ONE-row rwkv7_sample_rows_f32(rows = 1, nseg = C, *step = step[s], seed = seed[s]) call with the slot's parameters
 *      (temperature = 1 / inv_temp), the same max_domain and the same logits.  Writes nt[s][0..C) and nothing else.  seg_off / seg_len /
 *      allow_* are DEVICE int arrays of C entries; max_domain = the largest allow_hi - allow_lo (or seg_len), <= 15360.  One workgroup
 *      per (row, channel).
 * rwkv7_xy_slots_frame_bf16: for every live slot the rules of rwkv7_xy_frame_step for a batch of one with pos = step[s],
 *      total = limit[s], all_done = 0, on nt[s]: a non-audio id on channel 0 starts the flush countdown (needs = C - 1 .. -1), channel 0
 *      carries eos0 while flushing (eos0 < 0: keeps its id), channel i pads once needs < C - i; stop on step[s] + 1 >= limit[s] or on an
 *      eos_list hit on channel 0 while not flushing; the slot also ends when the countdown reaches -1 (reference_termination = 1:
 *      rwkv7_xy_frame_step's literal form).  Then seq[s][step[s]][0..C) = row[s][0..C) = the frame (row index clamped to seq_ld - 1),
 *      x[s] = sum_c tables[c][row[s][c]] as rwkv7_xy_embed_bf16 forms it (0 ulp), step[s] += 1, needs[s] updated, live[s] = still
 *      unfinished.  Every id of the frame (eos0 and pad included) must be a row of its channel's table.  One workgroup per row.
 * All per-slot fields are DEVICE arrays of `slots` entries.  top_k_max (host): the largest top_k[] value, in [0, 64]; a slot's top_k
 * is clamped to it; a sampled slot with top_k = 0 draws from the whole distribution (top_p is ignored there).  Errors: RWKV7_EINVAL
 * for rows / slots / C / D / seq_ld / max_domain <= 0, a null st / logits / segment array / per-slot array / table, one of allow_lo /
 * allow_hi without the other, n_eos > 0 without eos_list; RWKV7_ESHAPE for max_domain > 15360, top_k_max outside [0, 64], C > 16,
 * D % 8 != 0. */
typedef struct rwkv7_xy_slot_state {
    long *step;                 /* frames emitted so far = output row of the next frame */
    long *limit;                /* the request's frame budget */
    unsigned long long *seed;   /* the request's Philox key */
    float *inv_temp;
    int *top_k;
    float *top_p;
    unsigned char *do_sample;
    unsigned char *live;        /* 1 while the slot's request runs */
    long *needs;                /* flush countdown, -1: not flushing */
    long *nt;                   /* [slots][C] the drawn ids of the current frame */
    long *row;                  /* [slots][C] the frame written last */
    long *seq;                  /* [slots][seq_ld][C] generated frames */
    long seq_ld;
    const void *tables[16];     /* bf16 [V_c][D] embedding tables, C of them */
    void *x;                    /* bf16 [slots][D]: the next decode step's input */
    int D, C, slots, top_k_max;
    long text_shift, speech_vocab, pad, eos0;
    const long *eos_list;       /* n_eos DEVICE ids for the stopping criterion, or NULL */
    int n_eos, reference_termination;
} rwkv7_xy_slot_state;
int rwkv7_xy_slots_draw_f32(int rows, const float *logits, long ld, const int *row_slot, const int *seg_off, const int *seg_len,
                            const int *allow_lo, const int *allow_hi, int max_domain, const rwkv7_xy_slot_state *st, rwkv7_stream_t stream);
int rwkv7_xy_slots_frame_bf16(int rows, const int *row_slot, const rwkv7_xy_slot_state *st, rwkv7_stream_t stream);
/* rwkv7_xy_slots_draw_lp_f32 / rwkv7_xy_slots_frame_lp_bf16: the two entries above, which also report the log-probability of what a
 * frame drew (ContinuousXYDecoder(logprobs=True): ranking n candidates of one prompt without a second pass).  A frame is the two LP
 * calls in this order on one stream, with the same st and lp.  For a live slot every field of `st` -- nt; seq, row, x, step, needs,
 * live -- is written bit for bit as the plain entries write it.
 * rwkv7_xy_slots_draw_lp_f32 writes in addition, for every channel c it draws,
 *   ch_lp[s][c] = (x[id] - m) - log sum_j exp(x[j] - m)        (m = the maximum over j)
 * with x the RAW fp32 logits of channel c -- temperature 1, before top-k / top-p -- and j over the ids [allow_lo[c], allow_hi[c]).  A
 * channel whose allowed logits are all -INFINITY gives -INFINITY, not NaN.  Where the plain entry writes no nt[s][c] (slot not live,
 * row without a slot, empty range), ch_lp[s][c] is left as it is.  The reductions run thread -> wave -> workgroup in a fixed order:
 * the same logits and slot parameters give the same bits whatever row, slot or grid they are drawn in.
 * rwkv7_xy_slots_frame_lp_bf16 decides which of the C draws COUNT -- the frame rules may replace a drawn id by a forced one -- from the
 * slot's state alone, never by comparing ids (a drawn id that happens to equal the pad id is not misjudged):
 *   channel 0 counts iff needs[s] < 0 on entry: the flush had not started before this frame, so the drawn id was the model's free
 *             choice -- also on the frame that starts the flush, where eos0 is written in its place;
 *   channel i >= 1 counts iff the frame keeps its drawn id: not (flushing and needs < C - i), with `needs` as the frame rule sees it
 *             (after a flush start set it to C - 1, before the decrement).
 * With pw = the row of seq the frame is written to (step[s] on entry, clamped to [0, seq_ld - 1]):
 *   frame_lp[s][pw][c] = ch_lp[s][c] for a counted channel, +0.0f for a forced one
 *   cum_lp[s]         += the counted values in channel order 0 .. C-1, each converted to double and added on its own (plain read,
 *                        add, store: one workgroup owns a slot)
 *   n_lp[s]           += the number of counted channels (the length for a per-draw mean)
 * A slot that is not live, and a row whose slot is outside [0, slots), leave all four arrays untouched.  Errors: those of the plain
 * entries, and RWKV7_EINVAL for a null lp or a null member of it (one struct serves both calls: either entry wants all four);
 * nothing is launched then.  (A struct plus a typedef, like rwkv7_slot_logprob; the Python mirror is continuous_xy.XYSlotLogprob.) */
struct rwkv7_xy_slot_logprob {
    float *ch_lp;               /* [slots][C]: log-probability of every channel's drawn id of the current frame (draw -> frame) */
    float *frame_lp;            /* [slots][seq_ld][C]: per emitted frame, the counted channels' values; +0 where the id was forced */
    double *cum_lp;             /* [slots]: running fp64 sum of the counted values, in (frame, channel) order */
    long *n_lp;                 /* [slots]: number of counted values so far */
};
typedef struct rwkv7_xy_slot_logprob rwkv7_xy_slot_logprob;
int rwkv7_xy_slots_draw_lp_f32(int rows, const float *logits, long ld, const int *row_slot, const int *seg_off, const int *seg_len,
                               const int *allow_lo, const int *allow_hi, int max_domain, const rwkv7_xy_slot_state *st,
                               const rwkv7_xy_slot_logprob *lp, rwkv7_stream_t stream);
int rwkv7_xy_slots_frame_lp_bf16(int rows, const int *row_slot, const rwkv7_xy_slot_state *st, const rwkv7_xy_slot_logprob *lp,
                                 rwkv7_stream_t stream);

/* ---- CosyVoice's repetition-aware draw per SLOT of a continuous-batching engine (csrc/ras_slots.hip; rwkvtts_amd/continuous_cosy.py),
 * where every slot runs its own utterance.  Logits row r (fp32, V ids, row stride ld) belongs to slot s = row_slot[r] (row_slot NULL:
 * s = r; rows with s outside [0, slots) are skipped).  Two rows that name the same slot are a caller error: the slot's state would
 * be written by two workgroups.  A slot with live[s] == 0 is left completely untouched, its x row included.
 * rwkv7_ras_slots_f32: a live slot draws one id as rwkv7_ras_step_f32 does: nucleus over the softmax probabilities with top_p[s] /
 *      top_k[s] (clamped to [1, top_k_max]), EOS removed per stage while step[s] < n_ignore[s], and the draw from the full
 *      distribution when the candidate already occurs >= win_size * tau_r[s] times in the slot's ring.  Philox key seed[s], counter
 *      (step[s] lo, step[s] hi, 0, 0x7a5).  Contract: the id, the ring, ptr[s] and step[s] after the call are bit-identical to ONE
 *      rwkv7_ras_step_f32 call with the slot's logits row, ring, pointer, step, n_ignore, parameters and seed.  Then the streaming
 *      loop's bookkeeping: ids[s] = id; if id != eos: seq[s][n_out[s]] = id (when n_out[s] < seq_ld), recent[s][ptr[s]] = id,
 *      ptr[s] = (ptr[s] + 1) % win_size, n_out[s] += 1, x[s] = emb[id] (emb NULL: no copy); step[s] += 1;
 *      live[s] = id != eos && step[s] < limit[s].  One workgroup per row.
 * All per-slot fields are DEVICE arrays of `slots` entries.  Errors (nothing is launched): RWKV7_EINVAL for rows / V / slots /
 * seq_ld <= 0, a null st / logits / per-slot array, emb without x (or with D <= 0); RWKV7_ESHAPE for V > 15360, win_size outside
 * [1, min(128, win_ld)], top_k_max outside [1, 128], D % 8 != 0. */
typedef struct rwkv7_ras_slot_state {
    long *step;                 /* loop index of the utterance: draws made so far */
    long *limit;                /* max_len: the slot ends when step reaches it */
    long *n_ignore;             /* EOS is rejected while step < n_ignore */
    unsigned long long *seed;   /* the request's Philox key */
    int *top_k;
    float *top_p;
    float *tau_r;
    unsigned char *live;        /* 1 while the slot's request runs */
    long *recent;               /* [slots][win_ld] ring of the last win_size emitted ids, -1 = empty */
    long win_ld;
    long *ptr;                  /* write position in the ring */
    long *ids;                  /* last drawn id, EOS included */
    long *n_out;                /* emitted (non-EOS) ids so far */
    long *seq;                  /* [slots][seq_ld] emitted ids */
    long seq_ld;
    const void *emb;            /* bf16 [V][D] speech embedding table, or NULL */
    void *x;                    /* bf16 [slots][D]: the next decode step's input */
    int D;
    int slots;
    int win_size;               /* <= 128, <= win_ld */
    int top_k_max;              /* the largest top_k[] value, in [1, 128] */
    long eos;
} rwkv7_ras_slot_state;
int rwkv7_ras_slots_f32(int rows, int V, const float *logits, long ld, const int *row_slot, const rwkv7_ras_slot_state *st,
                        rwkv7_stream_t stream);
/* rwkv7_ras_slots_lp_f32: rwkv7_ras_slots_f32 that also reports the log-probability of every id it draws
 * (ContinuousCosyDecoder(logprobs=True): ranking n candidates of one utterance without a second, teacher-forced pass).  For a live
 * slot every field of `st` -- id, ring, ptr, n_out, seq, step, live, x -- is written bit for bit as rwkv7_ras_slots_f32 writes it.
 * The value is
 *   lp = x[id] - m - log sum_j exp(x[j] - m)        (m = the row's maximum)
 * with x the RAW fp32 logits of the row -- temperature 1, before top-k, top-p and the repetition test; the reference's
 * logits.log_softmax(-1) entry -- and j over the ids the draw could have produced: all V ids, minus EOS while
 * step[s] < n_ignore[s] (the reference redraws until it gets another id).  The EOS-free sum is formed from its own terms, not by
 * subtracting EOS's from the full sum.  When the repetition test replaces the nucleus candidate by the draw from the full
 * distribution, lp is that id's value under the same formula.  With n = n_out[s] before the call:
 *   id != eos (emitted):  tok_lp[s][n] = lp (if 0 <= n < seq_ld; row stride seq_ld, column = the id's index in seq),
 *                         cum_lp[s] += (double)lp (plain read, add, store: one workgroup owns a slot); end_lp[s] is untouched
 *   id == eos:            end_lp[s] = lp; tok_lp, cum_lp (and n_out) are untouched
 * A row without a finite logit (or, next to a barred EOS, without any other id of non-zero weight) gives -INFINITY, not NaN.  A
 * slot that is not live, and a row whose slot is outside [0, slots), leave all three arrays untouched.  The reductions run
 * thread -> wave -> workgroup in a fixed order: the same logits row and slot state give the same bits whatever row, slot or grid
 * they are drawn in.  Errors: those of rwkv7_ras_slots_f32, and RWKV7_EINVAL for a null lp, lp->tok_lp, lp->cum_lp or lp->end_lp;
 * nothing is launched then.  (A struct plus a typedef, like rwkv7_slot_logprob; the Python mirror is continuous_cosy.RasSlotLogprob.) */
struct rwkv7_ras_slot_logprob {
    float *tok_lp;              /* [slots][seq_ld]: log-probability of every EMITTED id, column = its index in seq */
    double *cum_lp;             /* [slots]: running fp64 sum of the slot's tok_lp, in emission order */
    float *end_lp;              /* [slots]: log-probability of the EOS draw that ended the utterance (written only then) */
};
typedef struct rwkv7_ras_slot_logprob rwkv7_ras_slot_logprob;
int rwkv7_ras_slots_lp_f32(int rows, int V, const float *logits, long ld, const int *row_slot, const rwkv7_ras_slot_state *st,
                           const rwkv7_ras_slot_logprob *lp, rwkv7_stream_t stream);

/* the low-rank pair of the decode step in one launch: y[M,N] = act(x[M,K] @ w1[R,K]^T) @ w2[N,R]^T (+ bias); M <= 32,
 * K % 64 == 0, R in {32,64,128}, act 0 none / 1 tanh / 2 sigmoid (rwkv_s2s_single_ffn.py:497-500: w, a, v, g branches) */
int rwkv7_lora32_bf16(int M, int N, int K, int R, int act, const void *x, const void *w1, const void *w2, const void *bias,
                      void *y, rwkv7_stream_t stream);

/* probe of ds_read_b64_tr_b16 (LDS transpose read): in = 4096 u16 copied to LDS, addr[64] = element index each lane
 * points at, out[64][4] = what each lane receives */
int rwkv7_debug_tr16(const void *in, const int *addr, void *out, rwkv7_stream_t stream);
/* unit-test hook for the MFMA fragment layouts: D[32][32] = X[32][64] Y[32][64]^T (fp32 in, bf16-split MFMA),
 * DT = the same tile after the transposed LDS write-back (hi+lo planes re-joined). */
int rwkv7_debug_mma32(const float *X, const float *Y, float *D, float *DT, rwkv7_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RWKV7_HIP_H */
