// rwkvtts_amd/csrc/launchers.h -- every host launcher that one csrc file defines and another calls, declared once (internal, not
// installed).  capi.hip and lab/capi_lab.hip call through these declarations and every defining .hip file includes them, so a
// definition is compiled against the declaration its callers see.  The exception is the scan kernels whose source hashes
// profiles/pmc_wkv7.json records (wkv7_fwd / wkv7_bwd / wkv7_chunk_fwd / wkv7_chunk_fwd9 / wkv7_chunk_bseq / wkv7_chunk_bwd10 .hip):
// they are declared here and left untouched; a parameter that drifts there is an undefined symbol at link time.
// The launchers check nothing unless a comment says so: the extern "C" entries refuse bad arguments first (include/rwkv7_hip.h).
// The fused row stages (mix, add_ln, tmix_prepare, tmix_post, relusq) are not here: their entries sit beside their kernels in
// elementwise.hip and nothing else calls them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

namespace rwkv7 {

// the entries' first check
inline bool any_null(std::initializer_list<const void *> ps) {
    for (const void *p : ps)
        if (!p) return true;
    return false;
}

// ---- WKV7 scan, one step per iteration (wkv7_fwd.hip, wkv7_bwd.hip).  s, sa: the checkpoints the backward reads, both NULL for
//      inference; state: fp32 [B,H,64,64] carried in place, or NULL.  force_cw: columns per lane 4 / 8, 0 = the kernel's choice
int wkv_fwd_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b, void *y,
                 float *s, float *sa, float *state, int force_cw, hipStream_t stream);
int wkv_fwd_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b, void *y,
                float *s, float *sa, float *state, int force_cw, hipStream_t stream);
int wkv_bwd_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b,
                 const void *dy, const float *s, const float *sa, void *dw, void *dq, void *dk, void *dv, void *da, void *db,
                 hipStream_t stream);
int wkv_bwd_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b,
                const void *dy, const float *s, const float *sa, void *dw, void *dq, void *dk, void *dv, void *da, void *db,
                hipStream_t stream);
// dw, dq, dk, da, db: HOST arrays of two device pointers (the partial sets of the row-split backward); dv is one tensor
int wkv_bwd_split_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b,
                       const void *dy, const float *s, const float *sa, void *const *dw, void *const *dq, void *const *dk, void *dv,
                       void *const *da, void *const *db, int wide, hipStream_t stream);
int wkv_bwd_split_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b,
                      const void *dy, const float *s, const float *sa, void *const *dw, void *const *dq, void *const *dk, void *dv,
                      void *const *da, void *const *db, int wide, hipStream_t stream);

// ---- chunked (MFMA) WKV7 (wkv7_chunk_fwd.hip, wkv7_chunk_fwd9.hip, wkv7_chunk_bseq.hip, wkv7_chunk_bwd10.hip).  tinv: the chunk
//      inverses of chunk_prep; sa / hs: the backward's tape, both NULL or both set; seq_chunk_off / nseq: packed rows, NULL / 0 for plain
//      ones; h0 / hT (dhT / dh0): carried state in / out (its gradient in / out), fp32 [nseq or B,H,64,64], each may be NULL
int chunk_prep_bf16(int B, int T, int H, const void *w, const void *a, const void *b, float *tinv, hipStream_t stream);
int chunk_prep_f32(int B, int T, int H, const void *w, const void *a, const void *b, float *tinv, hipStream_t stream);
int chunk_fwd_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b,
                   const float *tinv, void *y, float *sa, void *hs, const int *seq_chunk_off, int nseq, hipStream_t stream);
int chunk_fwd_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b,
                  const float *tinv, void *y, float *sa, void *hs, const int *seq_chunk_off, int nseq, hipStream_t stream);
int chunk_fwd9_state_seq_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a,
                              const void *b, const float *tinv, void *y, float *sa, void *hs, const int *seq_chunk_off, int nseq,
                              const float *h0, float *hT, hipStream_t stream);
// state: the cache field [rows,H,64,64], sequence i reads and writes row state_row[i] (device data, not range-checked)
int chunk_fwd9_state_rows_bf16(int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b,
                               const float *tinv, void *y, const int *seq_chunk_off, int nseq, float *state, const int *state_row,
                               hipStream_t stream);
int chunk_bseq_bf16(int B, int T, int H, const void *w, const void *q, const void *a, const void *b, const void *dy, const float *tinv,
                    void *e_vk, float *z, const int *seq_chunk_off, int nseq, hipStream_t stream);
int chunk_bseq_state_seq_bf16(int B, int T, int H, const void *w, const void *q, const void *a, const void *b, const void *dy,
                              const float *tinv, void *e_vk, float *z, const int *seq_chunk_off, int nseq, const float *dhT, float *dh0,
                              hipStream_t stream);
int chunk_bwd_out10_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b,
                         const void *dy, const void *hs, const float *sa, const float *z, const void *e_vk, void *dw, void *dq, void *dk,
                         void *dv, void *da, void *db, hipStream_t stream);
int chunk_debug_mma(const float *X, const float *Y, float *D, float *DT, hipStream_t stream);
int chunk_debug_tr16(const uint16_t *in, const int *addr, uint16_t *out, hipStream_t stream);

// ---- GEMMs and GEMVs (gemm_nt4.hip, gemv32.hip, wgrad_skinny.hip).  gemm_nt4: aux is the second operand of epilogues 2..4 (x, s or
//      the residual), NULL for 0 and 1; bias may be NULL
int gemm_nt4_bf16(int M, int N, int K, const void *A, const void *W, void *C, const void *aux, int epilogue, hipStream_t stream);
int gemv32_bf16(int M, int N, int K, const void *x, const void *w, const void *bias, void *y, hipStream_t stream);
int lora32_bf16(int M, int N, int K, int R, int act, const void *x, const void *w1, const void *w2, const void *bias, void *y,
                hipStream_t stream);
int wgrad_skinny_bf16(long M, int N, int K, int S, const void *dy, const void *x, float *parts, hipStream_t stream);
int wgrad_mid_bf16(long M, int N, int K, int S, const void *dy, const void *x, float *parts, hipStream_t stream);
int wgrad_tn_bf16(long M, int N, int K, int S, const void *dy, const void *x, float *parts, hipStream_t stream);   // wgrad_tn.hip

// ---- low-rank branches through the token-shift lerp (mix_lora.hip).  Passed by value into the kernels
struct MixLoraDesc {
    int nb;               // branches (3 in layer 0: w, a, g; else 4: w, a, v, g)
    int r[4], off[4];     // rank and first column of each branch inside R
    int act[4];           // 0 none, 1 tanh, 2 sigmoid
    const void *w1[4];    // Linear(D, r_i).weight  [r_i][D]
    const void *mu[4];    // lerp coefficient [D]
    void *out[4];         // fwd: activation outputs [M][r_i];  wcat_bwd: dW1_i [r_i][D]
    void *out2[4];        // wcat_bwd: dmu_i [D];  combine_bwd: the incoming gradients d a_i [M][r_i]
};
int mix_lora_wcat_fwd(const MixLoraDesc &d, int R, int D, void *wcat, hipStream_t stream);
int mix_lora_wcat_bwd(const MixLoraDesc &d, int R, int D, const void *dwcat, hipStream_t stream);
int mix_lora_combine_fwd(const MixLoraDesc &d, long M, int T, int R, const void *G, const void *mask, hipStream_t stream);   // mask may be NULL
int mix_lora_combine_bwd(const MixLoraDesc &d, long M, int T, int R, const void *mask, void *dG, hipStream_t stream);

// ---- their down projections with the lerp as the GEMM's prologue (lora_down.hip).  Passed by value into the kernels
struct LoraDownDesc {
    int nb;               // branches
    int r[4], off[4];     // rank and first output column of each branch inside R
    int act[4];           // 0 none, 1 tanh, 2 sigmoid
    const void *w1[4];    // pack: Linear(D, r_i).weight [r_i][D]
    const void *mu[4];    // lerp coefficient [D]
    void *out[4];         // [M][r_i]
    int tile0[5];         // column group g owns the 32-column tiles tile0[g] .. tile0[g + 1] - 1
};
int lora_down_pack(const LoraDownDesc &d, int R, int D, void *packed, hipStream_t stream);
// fills d.tile0; RWKV7_ESHAPE unless the 2..10 column tiles cut into two halves of at most 5 tiles and two branches each.  mask may be NULL
int lora_down_fwd(LoraDownDesc &d, int R, long M, int T, int D, const void *x, const void *mask, const void *packed, hipStream_t stream);

// ---- plain row and buffer kernels of elementwise.hip
int sum_slabs_bf16(long n, int S, const float *parts, void *out, int accumulate, hipStream_t stream);
int transpose_bf16(int R, int C, const void *in, void *out, hipStream_t stream);
int gather_rows16(long n_out, int D, const void *src, const int *idx, void *out, hipStream_t stream);   // idx[r] < 0: a zero row

// ---- packed prefill into chosen cache rows (prefill_rows.hip, cache_rows.hip).  RWKV7_ESHAPE for an nmix outside {1, 6}; branch,
//      beta, mask and x_out (without branch) may be NULL; x_prev_rd is never NULL (the entry passes x_prev for it)
int add_ln_mix_rows_fwd_bf16(int T, int D, int nmix, const void *x, const void *branch, const void *gamma, const void *beta, float eps,
                             const void *mask, const void *params, const int *prev_src, const int *last_dst, const void *x_prev_rd,
                             void *x_prev, void *x_out, void *out, int nblocks, int run_len, hipStream_t stream);
int cache_rows_commit_bf16(int layers, int n, const void *const *src_tbl, void *const *dst_tbl, const int *src_row, const int *dst_row,
                           int D, int H, hipStream_t stream);
int cache_rows_seed_bf16(int layers, int n, const void *const *src_tbl, void *const *dst_tbl, const int *src_row, const int *dst_row,
                         int D, int H, hipStream_t stream);   // src_row == RWKV7_SEED_ZERO: zeros instead of a copy
int cache_rows_retain_bf16(int layers, int slots, const void *const *src_tbl, void *const *dst_tbl, const unsigned char *live,
                           unsigned char *armed, const int *retain_row, int *ticket, int D, int H, hipStream_t stream);   // slots >= 1

// ---- state tuning (state_tune.hip): fp32 master states of named voices -> rows of a bf16 cache, and their AdamW step from the
//      cache's leaf gradients straight into the serving cache's rows.  skip_flag may be NULL; A >= 1, n >= 1
int state_rows_expand_f32(int layers, int n, const void *const *master_tbl, void *const *dst_tbl, const int *voice, int D, int H,
                          hipStream_t stream);
int state_rows_adamw_f32(int layers, int A, const void *const *grad_tbl, void *const *master_tbl, void *const *m_tbl, void *const *v_tbl,
                         void *const *store_tbl, const int *seg_start, const int *seg_rows, const int *seg_info, const float *skip_flag,
                         float lr, float beta1, float beta2, float eps, float wd, float grad_scale, int D, int H, hipStream_t stream);

// ---- loss heads and per-sequence scores (head_loss.hip, seq_scores.hip).  C: the entropy constant of the smoothed target
//      distribution; argmax_rows, and ce_seq_bwd's loss_rows, may be NULL
int ce_fwd_bwd(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
               float label_smoothing, hipStream_t stream);
//      lse_rows and max_rows may be NULL
int ce_reg_fwd_bwd(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
                   float label_smoothing, float z_coef, float max_coef, float *lse_rows, float *max_rows, hipStream_t stream);
int ce_seq_bwd(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, long row0, long n_seq,
               const long *seq_start, const float *seq_scale, float *loss_rows, hipStream_t stream);
//      ref_lp and each of the four per-row outputs may be NULL
int ce_policy_fwd_bwd(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, long row0, long n_seq,
                      const long *seq_start, const float *adv, const float *seq_w, const float *old_lp, const float *ref_lp, float eps_lo,
                      float eps_hi, float beta, float *lp_rows, float *loss_rows, float *kl_rows, float *clip_rows, hipStream_t stream);
int kl_acc_fwd_bwd(long rows, int V, long ld, const void *logits, void *dlogits, const long *labels, long ignore_index, float smoothing,
                   float C, float scale, float *loss_rows, int *correct_rows, hipStream_t stream);
int head_eval(long rows, int V, long ld, const void *logits, const long *labels, long ignore_index, int kind, float smoothing, float C,
              float *loss_rows, int *correct_rows, int *argmax_rows, hipStream_t stream);
int seq_scores(long n_seq, const long *seq_start, const float *loss_rows, const int *correct_rows, const long *labels, long ignore_index,
               double *loss_sum, long *tokens, long *correct, float *worst_loss, long *worst_row, hipStream_t stream);

// ---- optimizer and gradient buffers (elementwise.hip: adamw_step; grad_ops.hip; buf_digest.hip).  slab_group / group_tab: both NULL
//      or both set; skip_flag may be NULL; inv_bc1, inv_sqrt_bc2: the bias corrections 1 / (1 - beta1^step), 1 / sqrt(1 - beta2^step)
int adamw_step(long n, float *p32, const void *g16, float *m, float *v, void *p16, const uint8_t *slab_group, const float *group_tab,
               const float *skip_flag, float lr, float beta1, float beta2, float eps, float wd, float inv_bc1, float inv_sqrt_bc2,
               hipStream_t stream);
int adamw_clip_step(long n, float *p32, const void *g16, float *m, float *v, void *p16, const uint8_t *slab_group, const float *group_tab,
                    const float *skip_flag, const float *sumsq, float max_norm, float lr, float beta1, float beta2, float eps, float wd,
                    float inv_bc1, float inv_sqrt_bc2, hipStream_t stream);
int grad_sumsq_bf16(long n, const void *g16, float *partials, float *out, int accumulate, hipStream_t stream);
int grad_accum_bf16(long n, float *acc32, const void *g16, int first, hipStream_t stream);
int grad_fold_bf16(long n, const float *acc32, void *g16, float inv_count, hipStream_t stream);
long buf_digest_tiles(long n_words);
// dst NULL: digest only; otherwise dst[0..n_words) = buf[0..n_words) as well
int buf_digest_u32(long n_words, long first_index, const void *buf, void *dst, unsigned long long *partials, unsigned long long *out,
                   int accumulate, hipStream_t stream);

// ---- sampling (sampling.hip, xy_slots.hip, ras_slots.hip).  tail, st: the header's rwkv7_sample_tail / rwkv7_slot_state /
//      rwkv7_xy_slot_state / rwkv7_ras_slot_state, copied by the launcher; these launchers return RWKV7_ESHAPE for sizes past
//      their kernels' limits.  allow_lo / allow_hi, suppress, row_slot and tail may be NULL
int sample_rows_f32(int rows, int nseg, const float *logits, long ld, const int *seg_off, const int *seg_len, const int *allow_lo,
                    const int *allow_hi, const int *suppress, int nsuppress, int max_domain, int do_sample, int top_k, float top_p,
                    float temperature, unsigned long long seed, const long *step, long *out, const void *tail, int min_id, long min_until,
                    hipStream_t stream);
int sample_slots_f32(int rows, const float *logits, long ld, const int *row_slot, const int *allow_lo, const int *allow_hi,
                     const int *suppress, int nsuppress, int max_domain, const void *st, hipStream_t stream);
int sample_slots_lp_f32(int rows, const float *logits, long ld, const int *row_slot, const int *allow_lo, const int *allow_hi,
                        const int *suppress, int nsuppress, int max_domain, const void *st, float *tok_lp, double *cum_lp,
                        hipStream_t stream);
int ras_step_f32(int V, const float *logits, long *tok, long *recent, long *ptr, long *step_i, long n_ignore, int eos, float top_p,
                 int top_k, int win_size, float tau_r, unsigned long long seed, hipStream_t stream);
int xy_frame_step(int B, int C, int rows, long text_shift, long speech_vocab, long pad, long eos0, long total, const long *eos_list,
                  int n_eos, int reference_termination, const long *nt, long *out, long *row, long *pos, long *unfinished, long *needs,
                  unsigned char *all_done, long *n_rows, hipStream_t stream);
int xy_embed_bf16(int B, int C, int D, const void *const *tables_host, const long *row, void *x, hipStream_t stream);
int xy_slots_draw_f32(int rows, const float *logits, long ld, const int *row_slot, const int *seg_off, const int *seg_len,
                      const int *allow_lo, const int *allow_hi, int max_domain, const void *st, hipStream_t stream);
int xy_slots_frame_bf16(int rows, const int *row_slot, const void *st, hipStream_t stream);
// lp: the header's rwkv7_xy_slot_logprob, copied by the launcher like st
int xy_slots_draw_lp_f32(int rows, const float *logits, long ld, const int *row_slot, const int *seg_off, const int *seg_len,
                         const int *allow_lo, const int *allow_hi, int max_domain, const void *st, const void *lp, hipStream_t stream);
int xy_slots_frame_lp_bf16(int rows, const int *row_slot, const void *st, const void *lp, hipStream_t stream);
int ras_slots_f32(int rows, int V, const float *logits, long ld, const int *row_slot, const void *st, hipStream_t stream);
int ras_slots_lp_f32(int rows, int V, const float *logits, long ld, const int *row_slot, const void *st, float *tok_lp, double *cum_lp,
                     float *end_lp, hipStream_t stream);

// ---- decode step (decode_step.hip: B <= 32; decode_step_wide.hip: 32 < B <= 128).  layer_tbl: device table of decode_layer_ptrs()
//      pointers per layer, layer_tbl_host its host copy or NULL; head_b may be NULL.  RWKV7_ESHAPE (workspace size 0) for shapes
//      outside the kernels' limits
int decode_layer_ptrs();
size_t decode_workspace_bytes(int B, int D, int H, int F, int V, int Rw, int Ra, int Rv, int Rg);
int decode_step_bf16(int B, int D, int H, int L, int F, int V, int Rw, int Ra, int Rv, int Rg, float ln_eps, float gn_eps,
                     const void *const *layer_tbl, const void *const *layer_tbl_host, const void *x_in, const void *norm_w,
                     const void *norm_b, const void *head_w, const void *head_b, float *logits, void *workspace, int persistent,
                     hipStream_t stream);
size_t decode_wide_workspace_bytes(int B, int D, int H, int F, int V, int Rw, int Ra, int Rv, int Rg);
int decode_step_wide_bf16(int B, int D, int H, int L, int F, int V, int Rw, int Ra, int Rv, int Rg, float ln_eps, float gn_eps,
                          const void *const *layer_tbl, const void *const *layer_tbl_host, const void *x_in, const void *norm_w,
                          const void *norm_b, const void *head_w, const void *head_b, float *logits, void *workspace, hipStream_t stream);

#ifdef RWKV7_LAB
// ---- lab build only (lab/capi_lab.hip): the superseded twins in lab/wkv7_chunk_bwd9.hip, lab/gemm_relusq.hip and the 4-wave bf16
//      forward of wkv7_chunk_fwd.hip
int chunk_bwd_out9_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b,
                        const void *dy, const void *hs, const float *sa, const float *z, const void *e_vk, void *dw, void *dq, void *dk,
                        void *dv, void *da, void *db, hipStream_t stream);
int chunk_fwd4_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a, const void *b,
                    const float *tinv, void *y, float *sa, void *hs, const int *seq_chunk_off, int nseq, hipStream_t stream);
int gemm_nt_bf16_variant(int M, int N, int K, const void *A, const void *W, void *C, int epilogue, int variant, hipStream_t stream);
int gemm_nt_relusq_bwd_bf16(int M, int N, int K, const void *A, const void *W, const void *aux, void *C, hipStream_t stream);
#endif

}  // namespace rwkv7
