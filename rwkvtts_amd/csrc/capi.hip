// rwkvtts_amd/csrc/capi.hip -- extern "C" surface of librwkv7_hip.so (declared in include/rwkv7_hip.h).
// Argument checking mirrors the reference's asserts (wkv7_cuda.cu:136, rwkv7_state_fwd_fp16.cu:61,
// rwkv_s2s_single_ffn.py:19-21) but reports through the return code instead of aborting the process.
// The launchers it calls are declared in launchers.h.  The entries of the fused row stages (rwkv7_mix_*, rwkv7_add_ln_*,
// rwkv7_tmix_*, rwkv7_relusq_*) are not here: each is one checked launcher beside its kernel, at the end of elementwise.hip.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/rwkv7_hip.h"
#include "launchers.h"
#include "ln_row.h"   // row_width_ok

using rwkv7::any_null;

extern "C" {

const char *rwkv7_version(void) { return "rwkv7_hip 0.1.0 gfx950"; }

#define FWD_BODY(IMPL, CW)                                                                   \
    if (B <= 0 || T <= 0 || H <= 0 || any_null({w, q, k, v, a, b, y})) return RWKV7_EINVAL; \
    if ((s == nullptr) != (sa == nullptr)) return RWKV7_EINVAL;                              \
    if (T % RWKV7_CHUNK_LEN != 0) return RWKV7_ECHUNK;                                       \
    if ((CW) != 0 && (CW) != 4 && (CW) != 8) return RWKV7_ESHAPE;                            \
    return rwkv7::IMPL(B, T, H, w, q, k, v, a, b, y, s, sa, nullptr, CW, (hipStream_t)stream);

int rwkv7_wkv_fwd_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                       const void *a, const void *b, void *y, float *s, float *sa, rwkv7_stream_t stream) {
    FWD_BODY(wkv_fwd_bf16, 0)
}
int rwkv7_wkv_fwd_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                      const void *a, const void *b, void *y, float *s, float *sa, rwkv7_stream_t stream) {
    FWD_BODY(wkv_fwd_f32, 0)
}
int rwkv7_wkv_fwd_variant_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                               const void *a, const void *b, void *y, float *s, float *sa, int cols_per_lane, rwkv7_stream_t stream) {
    FWD_BODY(wkv_fwd_bf16, cols_per_lane)
}
int rwkv7_wkv_fwd_variant_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                              const void *a, const void *b, void *y, float *s, float *sa, int cols_per_lane, rwkv7_stream_t stream) {
    FWD_BODY(wkv_fwd_f32, cols_per_lane)
}

#define BWD_BODY(IMPL)                                                                                          \
    if (B <= 0 || T <= 0 || H <= 0 || any_null({w, q, k, v, a, b, dy, s, sa, dw, dq, dk, dv, da, db}))         \
        return RWKV7_EINVAL;                                                                                    \
    if (T % RWKV7_CHUNK_LEN != 0) return RWKV7_ECHUNK;                                                          \
    return rwkv7::IMPL(B, T, H, w, q, k, v, a, b, dy, s, sa, dw, dq, dk, dv, da, db, (hipStream_t)stream);

int rwkv7_wkv_bwd_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                       const void *a, const void *b, const void *dy, const float *s, const float *sa, void *dw,
                       void *dq, void *dk, void *dv, void *da, void *db, rwkv7_stream_t stream) {
    BWD_BODY(wkv_bwd_bf16)
}
int rwkv7_wkv_bwd_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                      const void *a, const void *b, const void *dy, const float *s, const float *sa, void *dw,
                      void *dq, void *dk, void *dv, void *da, void *db, rwkv7_stream_t stream) {
    BWD_BODY(wkv_bwd_f32)
}

// the reference-schema pair on the chunked (MFMA) kernels: `s` as an arena [hs | T^-1 | e_vk] (include/rwkv7_hip.h)
namespace {
constexpr size_t kArenaRec = (size_t)RWKV7_Q15_REC * 2, kArenaTinv = 32 * 32 * sizeof(float);
}
int rwkv7_wkv_fwd_fast_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                            const void *a, const void *b, void *y, float *s, float *sa, rwkv7_stream_t stream) {
    if (B <= 0 || T <= 0 || H <= 0 || any_null({w, q, k, v, a, b, y, s, sa})) return RWKV7_EINVAL;
    if (T % RWKV7_CHUNK_T != 0) return RWKV7_ECHUNK;
    const size_t n = (size_t)B * H * (T / RWKV7_CHUNK_T);
    char *base = reinterpret_cast<char *>(s);
    float *tinv = reinterpret_cast<float *>(base + n * kArenaRec);
    const int rc = rwkv7::chunk_prep_bf16(B, T, H, w, a, b, tinv, (hipStream_t)stream);
    if (rc != 0) return rc;
    return rwkv7::chunk_fwd_bf16(B, T, H, w, q, k, v, a, b, tinv, y, sa, base, nullptr, 0, (hipStream_t)stream);
}
int rwkv7_wkv_bwd_fast_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                            const void *a, const void *b, const void *dy, float *s, const float *sa, void *dw,
                            void *dq, void *dk, void *dv, void *da, void *db, rwkv7_stream_t stream) {
    if (B <= 0 || T <= 0 || H <= 0 || any_null({w, q, k, v, a, b, dy, s, sa, dw, dq, dk, dv, da, db})) return RWKV7_EINVAL;
    if (T % RWKV7_CHUNK_T != 0) return RWKV7_ECHUNK;
    const size_t n = (size_t)B * H * (T / RWKV7_CHUNK_T);
    char *base = reinterpret_cast<char *>(s);
    const float *tinv = reinterpret_cast<const float *>(base + n * kArenaRec);
    void *e_vk = base + n * (kArenaRec + kArenaTinv);
    float *z = reinterpret_cast<float *>(base + n * (2 * kArenaRec + kArenaTinv));   // fp32 [B,T,H,64]: 8192 B per chunk and head
    const int rc = rwkv7::chunk_bseq_bf16(B, T, H, w, q, a, b, dy, tinv, e_vk, z, nullptr, 0, (hipStream_t)stream);
    if (rc != 0) return rc;
    return rwkv7::chunk_bwd_out10_bf16(B, T, H, w, q, k, v, a, b, dy, base, sa, z, e_vk, dw, dq, dk, dv, da, db, (hipStream_t)stream);
}

#define BWD2_BODY(IMPL, WIDE)                                                                                 \
    if (B <= 0 || T <= 0 || H <= 0 || any_null({w, q, k, v, a, b, dy, s, sa, dw, dq, dk, dv, da, db}))   \
        return RWKV7_EINVAL;                                                                               \
    for (int i = 0; i < 2; i++)                                                                            \
        if (!dw[i] || !dq[i] || !dk[i] || !da[i] || !db[i]) return RWKV7_EINVAL;                           \
    if (T % RWKV7_CHUNK_LEN != 0) return RWKV7_ECHUNK;                                                     \
    return rwkv7::IMPL(B, T, H, w, q, k, v, a, b, dy, s, sa, dw, dq, dk, dv, da, db, (WIDE) ? 1 : 0, (hipStream_t)stream);

int rwkv7_wkv_bwd_split_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                             const void *a, const void *b, const void *dy, const float *s, const float *sa,
                             void *const *dw, void *const *dq, void *const *dk, void *dv, void *const *da,
                             void *const *db, rwkv7_stream_t stream) {
    BWD2_BODY(wkv_bwd_split_bf16, 0)
}
int rwkv7_wkv_bwd_split_f32(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                            const void *a, const void *b, const void *dy, const float *s, const float *sa,
                            void *const *dw, void *const *dq, void *const *dk, void *dv, void *const *da,
                            void *const *db, rwkv7_stream_t stream) {
    BWD2_BODY(wkv_bwd_split_f32, 0)
}
int rwkv7_wkv_bwd_split_variant_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                                     const void *a, const void *b, const void *dy, const float *s, const float *sa,
                                     void *const *dw, void *const *dq, void *const *dk, void *dv, void *const *da,
                                     void *const *db, int wide, rwkv7_stream_t stream) {
    BWD2_BODY(wkv_bwd_split_bf16, wide)
}

int rwkv7_wkv_workspace_bytes(int B, int T, int H, size_t *s_bytes, size_t *sa_bytes) {
    if (B <= 0 || T <= 0 || H <= 0 || !s_bytes || !sa_bytes) return RWKV7_EINVAL;
    if (T % RWKV7_CHUNK_LEN != 0) return RWKV7_ECHUNK;
    *s_bytes = (size_t)B * H * (T / RWKV7_CHUNK_LEN) * RWKV7_HEAD_SIZE * RWKV7_HEAD_SIZE * sizeof(float);
    *sa_bytes = (size_t)B * T * H * RWKV7_HEAD_SIZE * sizeof(float);
    return 0;
}

#define STATE_BODY(IMPL, CW)                                                                          \
    if (B <= 0 || T <= 0 || H <= 0 || any_null({state, r, w, k, v, a, b, y})) return RWKV7_EINVAL;   \
    if (H * RWKV7_HEAD_SIZE != C) return RWKV7_EHEAD;                                                 \
    if ((CW) != 0 && (CW) != 4 && (CW) != 8) return RWKV7_ESHAPE;                                     \
    return rwkv7::IMPL(B, T, H, w, r, k, v, a, b, y, nullptr, nullptr, state, CW, (hipStream_t)stream);

int rwkv7_wkv_state_fwd_bf16(int B, int T, int C, int H, float *state, const void *r, const void *w,
                             const void *k, const void *v, const void *a, const void *b, void *y,
                             rwkv7_stream_t stream) {
    STATE_BODY(wkv_fwd_bf16, 0)
}
int rwkv7_wkv_state_fwd_f32(int B, int T, int C, int H, float *state, const void *r, const void *w,
                            const void *k, const void *v, const void *a, const void *b, void *y,
                            rwkv7_stream_t stream) {
    STATE_BODY(wkv_fwd_f32, 0)
}
int rwkv7_wkv_state_fwd_variant_bf16(int B, int T, int C, int H, float *state, const void *r, const void *w,
                                     const void *k, const void *v, const void *a, const void *b, void *y, int cols_per_lane,
                                     rwkv7_stream_t stream) {
    STATE_BODY(wkv_fwd_bf16, cols_per_lane)
}


// ---- chunked (MFMA) WKV7 -----------------------------------------------------------------------------------------
#define CHUNK_DEFINE(SFX)                                                                                          \
    int rwkv7_wkv_chunk_prep_##SFX(int B, int T, int H, const void *w, const void *a, const void *b, float *tinv,   \
                                   rwkv7_stream_t stream) {                                                         \
        if (B <= 0 || T <= 0 || H <= 0 || any_null({w, a, b, tinv})) return RWKV7_EINVAL;                           \
        if (T % RWKV7_CHUNK_T != 0) return RWKV7_ECHUNK;                                                            \
        return rwkv7::chunk_prep_##SFX(B, T, H, w, a, b, tinv, (hipStream_t)stream);                                \
    }                                                                                                               \
    int rwkv7_wkv_chunk_fwd_##SFX(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,  \
                                  const void *a, const void *b, const float *tinv, void *y, float *sa, void *hs,   \
                                  rwkv7_stream_t stream) {                                                          \
        if (B <= 0 || T <= 0 || H <= 0 || any_null({w, q, k, v, a, b, tinv, y})) return RWKV7_EINVAL;               \
        if ((sa == nullptr) != (hs == nullptr)) return RWKV7_EINVAL;                                                \
        if (T % RWKV7_CHUNK_T != 0) return RWKV7_ECHUNK;                                                            \
        return rwkv7::chunk_fwd_##SFX(B, T, H, w, q, k, v, a, b, tinv, y, sa, hs, nullptr, 0, (hipStream_t)stream); \
    }                                                                                                               \
    int rwkv7_wkv_chunk_fwd_seq_##SFX(int B, int T, int H, const void *w, const void *q, const void *k, const void *v, \
                                      const void *a, const void *b, const float *tinv, void *y, float *sa, void *hs, \
                                      const int *seq_chunk_off, int nseq, rwkv7_stream_t stream) {                  \
        if (B <= 0 || T <= 0 || H <= 0 || any_null({w, q, k, v, a, b, tinv, y})) return RWKV7_EINVAL;               \
        if ((sa == nullptr) != (hs == nullptr) || (seq_chunk_off != nullptr && nseq <= 0)) return RWKV7_EINVAL;    \
        if (T % RWKV7_CHUNK_T != 0) return RWKV7_ECHUNK;                                                            \
        return rwkv7::chunk_fwd_##SFX(B, T, H, w, q, k, v, a, b, tinv, y, sa, hs, seq_chunk_off, nseq, (hipStream_t)stream); \
    }
CHUNK_DEFINE(bf16)
CHUNK_DEFINE(f32)
// chunked backward (bf16): csrc/wkv7_chunk_bseq.hip (adjoint recurrence, writes E and Z) + csrc/wkv7_chunk_bwd10.hip (per-chunk gradients)
int rwkv7_wkv_chunk_bseq_bf16(int B, int T, int H, const void *w, const void *q, const void *a, const void *b, const void *dy,
                              const float *tinv, void *e_vk, float *z, const int *seq_chunk_off, int nseq, rwkv7_stream_t stream) {
    if (B <= 0 || T <= 0 || H <= 0 || any_null({w, q, a, b, dy, (const void *)tinv, (const void *)e_vk})) return RWKV7_EINVAL;
    if (seq_chunk_off != nullptr && nseq <= 0) return RWKV7_EINVAL;
    if (T % 32 != 0) return RWKV7_ECHUNK;
    return rwkv7::chunk_bseq_bf16(B, T, H, w, q, a, b, dy, tinv, e_vk, z, seq_chunk_off, nseq, (hipStream_t)stream);
}
// the two sequential kernels with a carried state, one per sequence of a packed row (seq_chunk_off / nseq as
// rwkv7_wkv_chunk_fwd_seq_bf16): h0 / hT / dhT / dh0 fp32 [nseq,H,64,64], each may be NULL
int rwkv7_wkv_chunk_fwd_state_seq_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                                       const void *a, const void *b, const float *tinv, void *y, float *sa, void *hs,
                                       const int *seq_chunk_off, int nseq, const float *h0, float *hT, rwkv7_stream_t stream) {
    if (B <= 0 || T <= 0 || H <= 0 || any_null({w, q, k, v, a, b, (const void *)tinv, y})) return RWKV7_EINVAL;
    if ((sa == nullptr) != (hs == nullptr)) return RWKV7_EINVAL;
    if ((seq_chunk_off == nullptr) != (nseq <= 0)) return RWKV7_EINVAL;
    if (T % 32 != 0) return RWKV7_ECHUNK;
    return rwkv7::chunk_fwd9_state_seq_bf16(B, T, H, w, q, k, v, a, b, tinv, y, sa, hs, seq_chunk_off, nseq, h0, hT, (hipStream_t)stream);
}
int rwkv7_wkv_chunk_bseq_state_seq_bf16(int B, int T, int H, const void *w, const void *q, const void *a, const void *b,
                                        const void *dy, const float *tinv, void *e_vk, float *z, const int *seq_chunk_off, int nseq,
                                        const float *dhT, float *dh0, rwkv7_stream_t stream) {
    if (B <= 0 || T <= 0 || H <= 0 || any_null({w, q, a, b, dy, (const void *)tinv, (const void *)e_vk})) return RWKV7_EINVAL;
    if ((seq_chunk_off == nullptr) != (nseq <= 0)) return RWKV7_EINVAL;
    if (T % 32 != 0) return RWKV7_ECHUNK;
    return rwkv7::chunk_bseq_state_seq_bf16(B, T, H, w, q, a, b, dy, tinv, e_vk, z, seq_chunk_off, nseq, dhT, dh0, (hipStream_t)stream);
}
// stateful packed prefill into chosen cache rows (rwkvtts_amd/prefill.py): every index is device data read by the kernels
int rwkv7_wkv_chunk_fwd_state_rows_bf16(int T, int H, const void *w, const void *q, const void *k, const void *v, const void *a,
                                        const void *b, const float *tinv, void *y, const int *seq_chunk_off, int nseq, float *state,
                                        const int *state_row, rwkv7_stream_t stream) {
    if (T <= 0 || H <= 0 || nseq < 1 ||
        any_null({w, q, k, v, a, b, (const void *)tinv, y, (const void *)seq_chunk_off, (const void *)state, (const void *)state_row}))
        return RWKV7_EINVAL;
    if (T % 32 != 0) return RWKV7_ESHAPE;
    return rwkv7::chunk_fwd9_state_rows_bf16(T, H, w, q, k, v, a, b, tinv, y, seq_chunk_off, nseq, state, state_row, (hipStream_t)stream);
}
int rwkv7_add_ln_mix_rows_fwd_bf16(int T, int D, int nmix, const void *x, const void *branch, const void *gamma, const void *beta,
                                   float eps, const void *mask, const void *params, const int *prev_src, const int *last_dst,
                                   const void *x_prev_rd, void *x_prev, void *x_out, void *out, int nblocks, int run_len,
                                   rwkv7_stream_t stream) {
    if (T <= 0 || nblocks <= 0 || run_len <= 0 ||
        any_null({x, gamma, params, out, (const void *)prev_src, (const void *)last_dst, (const void *)x_prev}))
        return RWKV7_EINVAL;
    if (branch && !x_out) return RWKV7_EINVAL;
    if (!rwkv7::row_width_ok(D) || T % 32 != 0) return RWKV7_ESHAPE;   // and for an nmix outside {1, 6}, from the launcher
    return rwkv7::add_ln_mix_rows_fwd_bf16(T, D, nmix, x, branch, gamma, beta, eps, mask, params, prev_src, last_dst,
                                           x_prev_rd ? x_prev_rd : x_prev, x_prev, x_out, out, nblocks, run_len, (hipStream_t)stream);
}
// staged cache rows -> slot rows in one launch (rwkvtts_amd/continuous.py, admission="overlap"): tables and row indices are device data.
// The checks of the two row entries; 1: checked, but nothing to do (n = 0)
static int cache_rows_check(int layers, int n, const void *const *src_tbl, void *const *dst_tbl, const int *src_row, const int *dst_row,
                            int D, int H) {
    if (layers < 1 || layers > 65535 || n < 0 || n > 65535 || D <= 0 || H <= 0 || !src_tbl || !dst_tbl) return RWKV7_EINVAL;
    if (D % 8 != 0 || D > 4096) return RWKV7_ESHAPE;
    if (D != 64 * H) return RWKV7_EHEAD;
    if (n == 0) return 1;
    if (!src_row || !dst_row) return RWKV7_EINVAL;
    return RWKV7_OK;
}
int rwkv7_cache_rows_commit_bf16(int layers, int n, const void *const *src_tbl, void *const *dst_tbl, const int *src_row,
                                 const int *dst_row, int D, int H, rwkv7_stream_t stream) {
    const int rc = cache_rows_check(layers, n, src_tbl, dst_tbl, src_row, dst_row, D, H);
    if (rc) return rc < 0 ? rc : RWKV7_OK;   // an argument error, or nothing to commit: no launch
    return rwkv7::cache_rows_commit_bf16(layers, n, src_tbl, dst_tbl, src_row, dst_row, D, H, (hipStream_t)stream);
}
// stored or zero rows -> slot (or staging) rows in one launch (rwkvtts_amd/state_store.py): copy or zero is device data too
int rwkv7_cache_rows_seed_bf16(int layers, int n, const void *const *src_tbl, void *const *dst_tbl, const int *src_row,
                               const int *dst_row, int D, int H, rwkv7_stream_t stream) {
    const int rc = cache_rows_check(layers, n, src_tbl, dst_tbl, src_row, dst_row, D, H);
    if (rc) return rc < 0 ? rc : RWKV7_OK;
    return rwkv7::cache_rows_seed_bf16(layers, n, src_tbl, dst_tbl, src_row, dst_row, D, H, (hipStream_t)stream);
}
// slot rows -> stored rows inside the captured step (rwkvtts_amd/continuous.py, retain=True): which slots are copied is device data
int rwkv7_cache_rows_retain_bf16(int layers, int slots, const void *const *src_tbl, void *const *dst_tbl, const unsigned char *live,
                                 unsigned char *armed, const int *retain_row, int *ticket, int D, int H, rwkv7_stream_t stream) {
    const int rc = cache_rows_check(layers, slots, src_tbl, dst_tbl, retain_row, ticket, D, H);
    if (rc < 0) return rc;
    if (!live || !armed || !retain_row || !ticket) return RWKV7_EINVAL;
    if (rc) return RWKV7_OK;
    return rwkv7::cache_rows_retain_bf16(layers, slots, src_tbl, dst_tbl, live, armed, retain_row, ticket, D, H, (hipStream_t)stream);
}
// state tuning (rwkvtts_amd/state_tune.py): master rows -> training cache rows, and the AdamW step of the voices of a batch.  The
// shape checks are cache_rows_check's (a table stands in for the index arrays it also wants).
int rwkv7_state_rows_expand_f32(int layers, int n, const void *const *master_tbl, void *const *dst_tbl, const int *voice, int D, int H,
                                rwkv7_stream_t stream) {
    const int rc = cache_rows_check(layers, n, master_tbl, dst_tbl, voice, voice, D, H);
    if (rc) return rc < 0 ? rc : RWKV7_OK;
    return rwkv7::state_rows_expand_f32(layers, n, master_tbl, dst_tbl, voice, D, H, (hipStream_t)stream);
}
int rwkv7_state_rows_adamw_f32(int layers, int n, int A, const void *const *grad_tbl, void *const *master_tbl, void *const *m_tbl,
                               void *const *v_tbl, void *const *store_tbl, const int *seg_start, const int *seg_rows, const int *seg_info,
                               const float *skip_flag, float lr, float beta1, float beta2, float eps, float weight_decay,
                               float grad_scale, int D, int H, rwkv7_stream_t stream) {
    if (A < 0 || A > 65535 || n < 0 || n > 65535 || layers > 21845 || !m_tbl || !v_tbl || !store_tbl)   // 3 * layers is a grid dimension
        return RWKV7_EINVAL;
    const int rc = cache_rows_check(layers, A ? n : 0, grad_tbl, master_tbl, seg_start, seg_rows, D, H);   // no voice: as no row
    if (rc) return rc < 0 ? rc : RWKV7_OK;
    if (!seg_info) return RWKV7_EINVAL;
    return rwkv7::state_rows_adamw_f32(layers, A, grad_tbl, master_tbl, m_tbl, v_tbl, store_tbl, seg_start, seg_rows, seg_info, skip_flag,
                                       lr, beta1, beta2, eps, weight_decay, grad_scale, D, H, (hipStream_t)stream);
}
// plain rows (one state per row, [B,H,64,64]): the packed entries with seq_chunk_off = NULL, nseq = 0
int rwkv7_wkv_chunk_fwd_state_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                                   const void *a, const void *b, const float *tinv, void *y, float *sa, void *hs,
                                   const float *h0, float *hT, rwkv7_stream_t stream) {
    return rwkv7_wkv_chunk_fwd_state_seq_bf16(B, T, H, w, q, k, v, a, b, tinv, y, sa, hs, nullptr, 0, h0, hT, stream);
}
int rwkv7_wkv_chunk_bseq_state_bf16(int B, int T, int H, const void *w, const void *q, const void *a, const void *b,
                                    const void *dy, const float *tinv, void *e_vk, float *z,
                                    const float *dhT, float *dh0, rwkv7_stream_t stream) {
    return rwkv7_wkv_chunk_bseq_state_seq_bf16(B, T, H, w, q, a, b, dy, tinv, e_vk, z, nullptr, 0, dhT, dh0, stream);
}
int rwkv7_wkv_chunk_bwd_out_z_bf16(int B, int T, int H, const void *w, const void *q, const void *k, const void *v,
                                   const void *a, const void *b, const void *dy, const void *hs, const float *sa,
                                   const float *z, const void *e_vk, void *dw, void *dq, void *dk, void *dv,
                                   void *da, void *db, rwkv7_stream_t stream) {
    if (B <= 0 || T <= 0 || H <= 0 ||
        any_null({w, q, k, v, a, b, dy, hs, (const void *)sa, (const void *)z, e_vk, dw, dq, dk, dv, da, db}))
        return RWKV7_EINVAL;
    if (T % 32 != 0) return RWKV7_ECHUNK;
    return rwkv7::chunk_bwd_out10_bf16(B, T, H, w, q, k, v, a, b, dy, hs, sa, z, e_vk, dw, dq, dk, dv, da, db, (hipStream_t)stream);
}
int rwkv7_gemm_nt_bf16(int M, int N, int K, const void *A, const void *W, void *C, int epilogue, rwkv7_stream_t stream) {
    if (any_null({A, W, (const void *)C})) return RWKV7_EINVAL;
    if (M <= 0 || N <= 0 || K <= 0 || M % 256 != 0 || N % 256 != 0 || K % 1024 != 0 || epilogue < 0 || epilogue > 1) return RWKV7_ESHAPE;
    return rwkv7::gemm_nt4_bf16(M, N, K, A, W, C, nullptr, epilogue, (hipStream_t)stream);
}
int rwkv7_gemm_nt_relusq_bwd_bf16(int M, int N, int K, const void *A, const void *W, const void *aux, void *C, rwkv7_stream_t stream) {
    if (any_null({A, W, aux, (const void *)C})) return RWKV7_EINVAL;
    if (M <= 0 || N <= 0 || K <= 0 || M % 256 != 0 || N % 256 != 0 || K % 1024 != 0) return RWKV7_ESHAPE;
    return rwkv7::gemm_nt4_bf16(M, N, K, A, W, C, aux, 2, (hipStream_t)stream);
}
int rwkv7_gemm_nt_relusq_bwd_s_bf16(int M, int N, int K, const void *A, const void *W, const void *s, void *C, rwkv7_stream_t stream) {
    if (any_null({A, W, s, (const void *)C})) return RWKV7_EINVAL;
    if (M <= 0 || N <= 0 || K <= 0 || M % 256 != 0 || N % 256 != 0 || K % 1024 != 0) return RWKV7_ESHAPE;
    return rwkv7::gemm_nt4_bf16(M, N, K, A, W, C, s, 3, (hipStream_t)stream);
}
int rwkv7_gemm_nt_add_bf16(int M, int N, int K, const void *A, const void *W, const void *resid, void *C, rwkv7_stream_t stream) {
    if (any_null({A, W, resid, (const void *)C})) return RWKV7_EINVAL;
    if (M <= 0 || N <= 0 || K <= 0 || M % 256 != 0 || N % 256 != 0 || K % 1024 != 0) return RWKV7_ESHAPE;
    return rwkv7::gemm_nt4_bf16(M, N, K, A, W, C, resid, 4, (hipStream_t)stream);
}
namespace {
// ranks: multiples of 8, 1 <= nb <= 4; fills nb, r, off; returns R or a negative error
int mix_lora_desc(rwkv7::MixLoraDesc &d, int nb, const int *ranks) {
    if (nb < 1 || nb > 4 || ranks == nullptr) return RWKV7_EINVAL;
    d.nb = nb;
    int R = 0;
    for (int i = 0; i < 4; i++) {
        d.r[i] = i < nb ? ranks[i] : 0;
        d.off[i] = R;
        d.act[i] = 0;
        d.w1[i] = d.mu[i] = nullptr;
        d.out[i] = d.out2[i] = nullptr;
        if (i < nb) {
            if (ranks[i] <= 0 || ranks[i] % 8 != 0) return RWKV7_ESHAPE;
            R += ranks[i];
        }
    }
    return R;
}
}  // namespace
int rwkv7_mix_lora_wcat_fwd_bf16(int nb, const int *ranks, const void *const *w1, const void *const *mu, int D, void *wcat, rwkv7_stream_t stream) {
    rwkv7::MixLoraDesc d;
    const int R = mix_lora_desc(d, nb, ranks);
    if (R < 0) return R;
    if (w1 == nullptr || mu == nullptr || wcat == nullptr) return RWKV7_EINVAL;
    if (D <= 0) return RWKV7_ESHAPE;
    for (int i = 0; i < nb; i++) {
        if (w1[i] == nullptr || mu[i] == nullptr) return RWKV7_EINVAL;
        d.w1[i] = w1[i];
        d.mu[i] = mu[i];
    }
    return rwkv7::mix_lora_wcat_fwd(d, R, D, wcat, (hipStream_t)stream);
}
int rwkv7_mix_lora_wcat_bwd_bf16(int nb, const int *ranks, const void *const *w1, const void *const *mu, int D, const void *dwcat,
                                 void *const *dw1, void *const *dmu, rwkv7_stream_t stream) {
    rwkv7::MixLoraDesc d;
    const int R = mix_lora_desc(d, nb, ranks);
    if (R < 0) return R;
    if (w1 == nullptr || mu == nullptr || dwcat == nullptr || dw1 == nullptr || dmu == nullptr) return RWKV7_EINVAL;
    if (D <= 0) return RWKV7_ESHAPE;
    for (int i = 0; i < nb; i++) {
        if (w1[i] == nullptr || mu[i] == nullptr || dw1[i] == nullptr || dmu[i] == nullptr) return RWKV7_EINVAL;
        d.w1[i] = w1[i];
        d.mu[i] = mu[i];
        d.out[i] = dw1[i];
        d.out2[i] = dmu[i];
    }
    return rwkv7::mix_lora_wcat_bwd(d, R, D, dwcat, (hipStream_t)stream);
}
int rwkv7_mix_lora_combine_fwd_bf16(int nb, const int *ranks, const int *acts, long M, int T, const void *G, const void *mask,
                                    void *const *out, rwkv7_stream_t stream) {
    rwkv7::MixLoraDesc d;
    const int R = mix_lora_desc(d, nb, ranks);
    if (R < 0) return R;
    if (acts == nullptr || G == nullptr || out == nullptr) return RWKV7_EINVAL;
    if (M <= 0 || T <= 0 || M % T != 0) return RWKV7_ESHAPE;
    for (int i = 0; i < nb; i++) {
        if (out[i] == nullptr || acts[i] < 0 || acts[i] > 2) return RWKV7_EINVAL;
        d.act[i] = acts[i];
        d.out[i] = out[i];
    }
    return rwkv7::mix_lora_combine_fwd(d, M, T, R, G, mask, (hipStream_t)stream);
}
int rwkv7_mix_lora_combine_bwd_bf16(int nb, const int *ranks, const int *acts, long M, int T, const void *mask, const void *const *y,
                                    const void *const *dy, void *dG, rwkv7_stream_t stream) {
    rwkv7::MixLoraDesc d;
    const int R = mix_lora_desc(d, nb, ranks);
    if (R < 0) return R;
    if (acts == nullptr || y == nullptr || dy == nullptr || dG == nullptr) return RWKV7_EINVAL;
    if (M <= 0 || T <= 0 || M % T != 0) return RWKV7_ESHAPE;
    for (int i = 0; i < nb; i++) {
        if (y[i] == nullptr || dy[i] == nullptr || acts[i] < 0 || acts[i] > 2) return RWKV7_EINVAL;
        d.act[i] = acts[i];
        d.out[i] = const_cast<void *>(y[i]);
        d.out2[i] = const_cast<void *>(dy[i]);
    }
    return rwkv7::mix_lora_combine_bwd(d, M, T, R, mask, dG, (hipStream_t)stream);
}
namespace {
// ranks: multiples of 32, 1 <= nb <= 4, at most 16 column tiles; fills nb, r, off; returns R or a negative error
int lora_down_desc(rwkv7::LoraDownDesc &d, int nb, const int *ranks) {
    if (nb < 1 || nb > 4 || ranks == nullptr) return RWKV7_EINVAL;
    d.nb = nb;
    int R = 0;
    for (int i = 0; i < 4; i++) {
        d.r[i] = i < nb ? ranks[i] : 0;
        d.off[i] = R;
        d.act[i] = 0;
        d.w1[i] = d.mu[i] = nullptr;
        d.out[i] = nullptr;
        if (i < nb) {
            if (ranks[i] <= 0 || ranks[i] % 32 != 0) return RWKV7_ESHAPE;
            R += ranks[i];
        }
    }
    for (int i = 0; i < 5; i++) d.tile0[i] = 0;
    return R <= 512 ? R : RWKV7_ESHAPE;
}
}  // namespace
int rwkv7_lora_down_pack_bf16(int nb, const int *ranks, const void *const *w1, int D, void *packed, rwkv7_stream_t stream) {
    rwkv7::LoraDownDesc d;
    const int R = lora_down_desc(d, nb, ranks);
    if (R < 0) return R;
    if (w1 == nullptr || packed == nullptr) return RWKV7_EINVAL;
    if (D <= 0 || D % 128 != 0) return RWKV7_ESHAPE;
    for (int i = 0; i < nb; i++) {
        if (w1[i] == nullptr) return RWKV7_EINVAL;
        d.w1[i] = w1[i];
    }
    return rwkv7::lora_down_pack(d, R, D, packed, (hipStream_t)stream);
}
int rwkv7_lora_down_fwd_bf16(int nb, const int *ranks, const int *acts, long M, int T, int D, const void *x, const void *mask,
                             const void *const *mu, const void *packed, void *const *out, rwkv7_stream_t stream) {
    rwkv7::LoraDownDesc d;
    const int R = lora_down_desc(d, nb, ranks);
    if (R < 0) return R;
    if (acts == nullptr || x == nullptr || mu == nullptr || packed == nullptr || out == nullptr) return RWKV7_EINVAL;
    if (M <= 0 || T <= 0 || M % T != 0 || M % 128 != 0 || D <= 0 || D % 128 != 0 || D > 4096) return RWKV7_ESHAPE;
    for (int i = 0; i < nb; i++) {
        if (mu[i] == nullptr || out[i] == nullptr || acts[i] < 0 || acts[i] > 2) return RWKV7_EINVAL;
        d.act[i] = acts[i];
        d.mu[i] = mu[i];
        d.out[i] = out[i];
    }
    return rwkv7::lora_down_fwd(d, R, M, T, D, x, mask, packed, (hipStream_t)stream);
}
int rwkv7_gemv32_bf16(int M, int N, int K, const void *x, const void *w, const void *bias, void *y, rwkv7_stream_t stream) {
    if (any_null({x, w, y})) return RWKV7_EINVAL;
    if (M <= 0 || M > 32 || N <= 0 || K <= 0 || K % 64 != 0) return RWKV7_ESHAPE;
    return rwkv7::gemv32_bf16(M, N, K, x, w, bias, y, (hipStream_t)stream);
}
int rwkv7_lora32_bf16(int M, int N, int K, int R, int act, const void *x, const void *w1, const void *w2, const void *bias,
                      void *y, rwkv7_stream_t stream) {
    if (any_null({x, w1, w2, y})) return RWKV7_EINVAL;
    if (M <= 0 || M > 32 || N <= 0 || K <= 0 || K % 64 != 0 || (R != 32 && R != 64 && R != 128) || act < 0 || act > 2)
        return RWKV7_ESHAPE;
    return rwkv7::lora32_bf16(M, N, K, R, act, x, w1, w2, bias, y, (hipStream_t)stream);
}
int rwkv7_adamw_groups_bf16(long n, float *p32, const void *g16, float *m, float *v, void *p16, const unsigned char *slab_group,
                            const float *group_tab, int ngroups, const float *skip_flag, float lr, float beta1, float beta2, float eps,
                            int step, rwkv7_stream_t stream) {
    if (n <= 0 || step <= 0 || any_null({(const void *)p32, g16, (const void *)m, (const void *)v, p16})) return RWKV7_EINVAL;
    if ((slab_group == nullptr) != (group_tab == nullptr) || (slab_group && (ngroups <= 0 || ngroups > 256))) return RWKV7_EINVAL;
    if (n % 4 != 0 || (slab_group && n % 128 != 0)) return RWKV7_ESHAPE;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    return rwkv7::adamw_step(n, p32, g16, m, v, p16, slab_group, group_tab, skip_flag, lr, beta1, beta2, eps, 0.f, (float)(1.0 / bc1),
                             (float)(1.0 / sqrt(bc2)), (hipStream_t)stream);
}
int rwkv7_adamw_groups_clip_bf16(long n, float *p32, const void *g16, float *m, float *v, void *p16, const unsigned char *slab_group,
                                 const float *group_tab, int ngroups, const float *skip_flag, const float *sumsq, float max_norm,
                                 float lr, float beta1, float beta2, float eps, int step, rwkv7_stream_t stream) {
    if (n <= 0 || step <= 0 || any_null({(const void *)p32, g16, (const void *)m, (const void *)v, p16, (const void *)sumsq}))
        return RWKV7_EINVAL;
    if ((slab_group == nullptr) != (group_tab == nullptr) || (slab_group && (ngroups <= 0 || ngroups > 256))) return RWKV7_EINVAL;
    if (!(max_norm >= 0.f)) return RWKV7_EINVAL;   // NaN or negative; +inf = measure only
    if (n % 4 != 0 || (slab_group && n % 128 != 0)) return RWKV7_ESHAPE;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    return rwkv7::adamw_clip_step(n, p32, g16, m, v, p16, slab_group, group_tab, skip_flag, sumsq, max_norm, lr, beta1, beta2, eps, 0.f,
                                  (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)), (hipStream_t)stream);
}
long rwkv7_grad_sumsq_workspace_bytes(long n) { return n <= 0 ? 0 : (n + 8191) / 8192 * (long)sizeof(float); }
int rwkv7_grad_sumsq_bf16(long n, const void *g16, float *partials, float *out, int accumulate, rwkv7_stream_t stream) {
    if (n <= 0 || any_null({g16, (const void *)partials, (const void *)out})) return RWKV7_EINVAL;
    if (n % 128 != 0 || ((uintptr_t)g16 & 15) != 0) return RWKV7_ESHAPE;
    return rwkv7::grad_sumsq_bf16(n, g16, partials, out, accumulate != 0, (hipStream_t)stream);
}
int rwkv7_grad_accum_bf16(long n, float *acc32, const void *g16, int first, rwkv7_stream_t stream) {
    if (n <= 0 || any_null({(const void *)acc32, g16})) return RWKV7_EINVAL;
    if (n % 128 != 0 || (((uintptr_t)g16 | (uintptr_t)acc32) & 15) != 0) return RWKV7_ESHAPE;
    return rwkv7::grad_accum_bf16(n, acc32, g16, first != 0, (hipStream_t)stream);
}
int rwkv7_grad_fold_bf16(long n, const float *acc32, void *g16, float inv_count, rwkv7_stream_t stream) {
    if (n <= 0 || any_null({(const void *)acc32, (const void *)g16})) return RWKV7_EINVAL;
    if (n % 128 != 0 || (((uintptr_t)g16 | (uintptr_t)acc32) & 15) != 0) return RWKV7_ESHAPE;
    return rwkv7::grad_fold_bf16(n, acc32, g16, inv_count, (hipStream_t)stream);
}
long rwkv7_buf_digest_workspace_bytes(long n_words) {
    return n_words <= 0 ? 0 : rwkv7::buf_digest_tiles(n_words) * (long)sizeof(unsigned long long);
}
int rwkv7_buf_digest_u32(long n_words, long first_index, const void *buf, unsigned long long *partials, unsigned long long *out,
                         int accumulate, rwkv7_stream_t stream) {
    if (n_words < 0 || first_index < 0 || out == nullptr) return RWKV7_EINVAL;
    if (n_words > 0 && any_null({buf, (const void *)partials})) return RWKV7_EINVAL;
    if (n_words % 4 != 0 || ((uintptr_t)buf & 15) != 0 || (((uintptr_t)partials | (uintptr_t)out) & 7) != 0) return RWKV7_ESHAPE;
    if (rwkv7::buf_digest_tiles(n_words) > 0x7fffffffL) return RWKV7_ESHAPE;   // one workgroup per tile: 2^44 words
    return rwkv7::buf_digest_u32(n_words, first_index, buf, nullptr, partials, out, accumulate != 0, (hipStream_t)stream);
}
int rwkv7_buf_snapshot_digest_u32(long n_words, long first_index, const void *src, void *dst, unsigned long long *partials,
                                  unsigned long long *out, int accumulate, rwkv7_stream_t stream) {
    if (n_words < 0 || first_index < 0 || out == nullptr) return RWKV7_EINVAL;
    if (n_words > 0 && any_null({src, (const void *)dst, (const void *)partials})) return RWKV7_EINVAL;
    if (n_words % 4 != 0 || (((uintptr_t)src | (uintptr_t)dst) & 15) != 0 || (((uintptr_t)partials | (uintptr_t)out) & 7) != 0)
        return RWKV7_ESHAPE;
    if (rwkv7::buf_digest_tiles(n_words) > 0x7fffffffL) return RWKV7_ESHAPE;
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst, nbytes = (uintptr_t)n_words * 4;
    if (n_words > 0 && s < d + nbytes && d < s + nbytes) return RWKV7_EINVAL;   // [src, src + 4n) and [dst, dst + 4n) overlap
    if (n_words == 0) dst = nullptr;   // nothing to store: the digest entry's empty case (out[0] = accumulate ? out[0] : 0)
    return rwkv7::buf_digest_u32(n_words, first_index, src, dst, partials, out, accumulate != 0, (hipStream_t)stream);
}
int rwkv7_adamw_bf16(long n, float *p32, const void *g16, float *m, float *v, void *p16, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, rwkv7_stream_t stream) {
    if (n <= 0 || step <= 0 || any_null({(const void *)p32, g16, (const void *)m, (const void *)v, p16})) return RWKV7_EINVAL;
    if (n % 4 != 0) return RWKV7_ESHAPE;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    return rwkv7::adamw_step(n, p32, g16, m, v, p16, nullptr, nullptr, nullptr, lr, beta1, beta2, eps, weight_decay,
                             (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)), (hipStream_t)stream);
}
int rwkv7_ce_fwd_bwd_bf16(long rows, int V, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
                          rwkv7_stream_t stream) {
    if (rows <= 0 || V <= 0 || any_null({(const void *)logits, (const void *)labels, (const void *)loss_rows})) return RWKV7_EINVAL;
    return rwkv7::ce_fwd_bwd(rows, V, V, logits, labels, ignore_index, scale, loss_rows, 0.f, (hipStream_t)stream);
}
int rwkv7_ce_fwd_bwd_ls_bf16(long rows, int V, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
                             float label_smoothing,
                          rwkv7_stream_t stream) {
    if (rows <= 0 || V <= 0 || any_null({(const void *)logits, (const void *)labels, (const void *)loss_rows})) return RWKV7_EINVAL;
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return RWKV7_EINVAL;
    return rwkv7::ce_fwd_bwd(rows, V, V, logits, labels, ignore_index, scale, loss_rows, label_smoothing, (hipStream_t)stream);
}
int rwkv7_ce_fwd_bwd_ld_bf16(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
                             float label_smoothing, rwkv7_stream_t stream) {
    if (rows <= 0 || V <= 0 || ld < V || any_null({(const void *)logits, (const void *)labels, (const void *)loss_rows})) return RWKV7_EINVAL;
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return RWKV7_EINVAL;
    return rwkv7::ce_fwd_bwd(rows, V, ld, logits, labels, ignore_index, scale, loss_rows, label_smoothing, (hipStream_t)stream);
}
int rwkv7_ce_reg_fwd_bwd_bf16(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
                              float label_smoothing, float z_coef, float max_coef, float *lse_rows, float *max_rows,
                              rwkv7_stream_t stream) {
    if (rows <= 0 || V <= 0 || ld < V || any_null({(const void *)logits, (const void *)labels, (const void *)loss_rows})) return RWKV7_EINVAL;
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return RWKV7_EINVAL;
    if (!(z_coef >= 0.f && z_coef < INFINITY && max_coef >= 0.f && max_coef < INFINITY)) return RWKV7_EINVAL;
    return rwkv7::ce_reg_fwd_bwd(rows, V, ld, logits, labels, ignore_index, scale, loss_rows, label_smoothing, z_coef, max_coef, lse_rows,
                                 max_rows, (hipStream_t)stream);
}
int rwkv7_ce_seq_bwd_bf16(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, long row0, long n_seq,
                          const long *seq_start, const float *seq_scale, float *loss_rows, rwkv7_stream_t stream) {
    if (rows <= 0 || V <= 0 || ld < V || row0 < 0 || n_seq <= 0 ||
        any_null({(const void *)logits, (const void *)labels, (const void *)seq_start, (const void *)seq_scale}))
        return RWKV7_EINVAL;
    return rwkv7::ce_seq_bwd(rows, V, ld, logits, labels, ignore_index, row0, n_seq, seq_start, seq_scale, loss_rows, (hipStream_t)stream);
}
int rwkv7_ce_policy_fwd_bwd_bf16(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, long row0, long n_seq,
                                 const long *seq_start, const float *adv, const float *seq_w, const float *old_lp, const float *ref_lp,
                                 float eps_lo, float eps_hi, float beta, float *lp_rows, float *loss_rows, float *kl_rows,
                                 float *clip_rows, rwkv7_stream_t stream) {
    if (rows <= 0 || V <= 0 || ld < V || row0 < 0 || n_seq <= 0 ||
        any_null({(const void *)logits, (const void *)labels, (const void *)seq_start, (const void *)adv, (const void *)seq_w,
                  (const void *)old_lp}))
        return RWKV7_EINVAL;
    if (!(eps_lo >= 0.f && eps_lo < 1.f && eps_hi >= 0.f)) return RWKV7_EINVAL;
    return rwkv7::ce_policy_fwd_bwd(rows, V, ld, logits, labels, ignore_index, row0, n_seq, seq_start, adv, seq_w, old_lp, ref_lp, eps_lo,
                                    eps_hi, beta, lp_rows, loss_rows, kl_rows, clip_rows, (hipStream_t)stream);
}
// the entropy constant of the label-smoothing KL's target distribution (1 - s on the label, s / (V - 1) elsewhere), sum_j t_j ln t_j
// with 0 ln 0 = 0 (what F.kl_div gives for a zero target)
static float kl_entropy_const(float smoothing, int V) {
    const double s = (double)smoothing;
    return (float)((1.0 - s) * log(1.0 - s) + (s > 0.0 ? s * log(s / (double)(V - 1)) : 0.0));
}
int rwkv7_kl_acc_fwd_bwd_bf16(long rows, int V, long ld, const void *logits, void *dlogits, const long *labels, long ignore_index,
                              float smoothing, float scale, float *loss_rows, int *correct_rows, rwkv7_stream_t stream) {
    if (rows <= 0 || V < 2 || ld < V ||
        any_null({logits, (const void *)dlogits, (const void *)labels, (const void *)loss_rows, (const void *)correct_rows}))
        return RWKV7_EINVAL;
    if (!(smoothing >= 0.f && smoothing < 1.f)) return RWKV7_EINVAL;
    return rwkv7::kl_acc_fwd_bwd(rows, V, ld, logits, dlogits, labels, ignore_index, smoothing, kl_entropy_const(smoothing, V), scale,
                                 loss_rows, correct_rows, (hipStream_t)stream);
}
int rwkv7_head_eval_bf16(long rows, int V, long ld, const void *logits, const long *labels, long ignore_index, int kind, float smoothing,
                         float *loss_rows, int *correct_rows, int *argmax_rows, rwkv7_stream_t stream) {
    if (rows <= 0 || V < 2 || ld < V || (kind != 0 && kind != 1) ||
        any_null({logits, (const void *)labels, (const void *)loss_rows, (const void *)correct_rows}))
        return RWKV7_EINVAL;
    if (!(smoothing >= 0.f && smoothing < 1.f)) return RWKV7_EINVAL;
    const float C = kind == 1 ? kl_entropy_const(smoothing, V) : 0.f;
    return rwkv7::head_eval(rows, V, ld, logits, labels, ignore_index, kind, smoothing, C, loss_rows, correct_rows, argmax_rows,
                            (hipStream_t)stream);
}
int rwkv7_seq_scores_f32(long n_seq, const long *seq_start, const float *loss_rows, const int *correct_rows, const long *labels,
                         long ignore_index, double *loss_sum, long *tokens, long *correct, float *worst_loss, long *worst_row,
                         rwkv7_stream_t stream) {
    if (n_seq <= 0 || n_seq > 0x7fffffffL ||   // one workgroup per sequence: the grid's x extent
        any_null({(const void *)seq_start, (const void *)loss_rows, (const void *)correct_rows, (const void *)labels,
                  (const void *)loss_sum, (const void *)tokens, (const void *)correct, (const void *)worst_loss, (const void *)worst_row}))
        return RWKV7_EINVAL;
    return rwkv7::seq_scores(n_seq, seq_start, loss_rows, correct_rows, labels, ignore_index, loss_sum, tokens, correct, worst_loss,
                             worst_row, (hipStream_t)stream);
}
int rwkv7_wgrad_skinny_bf16(long M, int N, int K, int S, const void *dy, const void *x, float *parts, rwkv7_stream_t stream) {
    if (any_null({dy, x, parts})) return RWKV7_EINVAL;
    const int rank = N > K ? K : N, wide = N > K ? N : K;
    if (M <= 0 || S <= 0 || M % S != 0 || (M / S) % 128 != 0 || wide % 256 != 0 || (rank != 32 && rank != 64 && rank != 128))
        return RWKV7_ESHAPE;
    return rwkv7::wgrad_skinny_bf16(M, N, K, S, dy, x, parts, (hipStream_t)stream);
}
int rwkv7_wgrad_mid_bf16(long M, int N, int K, int S, const void *dy, const void *x, float *parts, rwkv7_stream_t stream) {
    if (any_null({dy, x, parts})) return RWKV7_EINVAL;
    if (M <= 0 || S <= 0 || M % S != 0 || (M / S) % 64 != 0 || K <= 0 || K % 256 != 0 || (N != 512 && N != 576)) return RWKV7_ESHAPE;
    return rwkv7::wgrad_mid_bf16(M, N, K, S, dy, x, parts, (hipStream_t)stream);
}
int rwkv7_wgrad_tn_bf16(long M, int N, int K, int S, const void *dy, const void *x, float *parts, rwkv7_stream_t stream) {
    if (any_null({dy, x, parts})) return RWKV7_EINVAL;
    if (M <= 0 || S <= 0 || N <= 0 || K <= 0) return RWKV7_EINVAL;
    if (M % S != 0 || M / S > 0x7fffffffL || (M / S) % 128 != 0 || N % 256 != 0 || K % 256 != 0) return RWKV7_ESHAPE;
    return rwkv7::wgrad_tn_bf16(M, N, K, S, dy, x, parts, (hipStream_t)stream);
}
int rwkv7_sum_slabs_bf16(long n, int S, const float *parts, void *out, int accumulate, rwkv7_stream_t stream) {
    if (n <= 0 || S <= 0 || any_null({(const void *)parts, (const void *)out})) return RWKV7_EINVAL;
    if (n % 4 != 0) return RWKV7_ESHAPE;
    return rwkv7::sum_slabs_bf16(n, S, parts, out, accumulate, (hipStream_t)stream);
}
int rwkv7_gather_rows_bf16(long n_out, int D, const void *src, const int *idx, void *out, rwkv7_stream_t stream) {
    if (n_out <= 0 || D <= 0 || any_null({src, (const void *)idx, (const void *)out})) return RWKV7_EINVAL;
    if (D % 8 != 0) return RWKV7_ESHAPE;
    return rwkv7::gather_rows16(n_out, D, src, idx, out, (hipStream_t)stream);
}
int rwkv7_transpose_bf16(int R, int C, const void *in, void *out, rwkv7_stream_t stream) {
    if (R <= 0 || C <= 0 || any_null({in, (const void *)out})) return RWKV7_EINVAL;
    if (R % 64 != 0 || C % 64 != 0) return RWKV7_ESHAPE;
    return rwkv7::transpose_bf16(R, C, in, out, (hipStream_t)stream);
}
int rwkv7_decode_layer_ptrs(void) { return rwkv7::decode_layer_ptrs(); }
size_t rwkv7_decode_workspace_bytes(const rwkv7_decode_dims *dm) {
    if (!dm) return 0;
    return rwkv7::decode_workspace_bytes(dm->B, dm->D, dm->H, dm->F, dm->V, dm->Rw, dm->Ra, dm->Rv, dm->Rg);
}
int rwkv7_decode_step_bf16(const rwkv7_decode_dims *dm, const void *const *layer_tbl, const void *x_in, const void *norm_w,
                           const void *norm_b, const void *head_w, const void *head_b, float *logits, void *workspace,
                           int persistent, rwkv7_stream_t stream) {
    if (!dm || any_null({(const void *)layer_tbl, x_in, norm_w, norm_b, head_w, (const void *)logits, (const void *)workspace}))
        return RWKV7_EINVAL;
    if (dm->H * RWKV7_HEAD_SIZE != dm->D) return RWKV7_EHEAD;
    return rwkv7::decode_step_bf16(dm->B, dm->D, dm->H, dm->L, dm->F, dm->V, dm->Rw, dm->Ra, dm->Rv, dm->Rg, dm->ln_eps, dm->gn_eps,
                                   layer_tbl, nullptr, x_in, norm_w, norm_b, head_w, head_b, logits, workspace, persistent,
                                   (hipStream_t)stream);
}
int rwkv7_decode_step_tbl_bf16(const rwkv7_decode_dims *dm, const void *const *layer_tbl, const void *const *layer_tbl_host,
                               const void *x_in, const void *norm_w, const void *norm_b, const void *head_w, const void *head_b,
                               float *logits, void *workspace, int persistent, rwkv7_stream_t stream) {
    if (!dm || any_null({(const void *)layer_tbl, (const void *)layer_tbl_host, x_in, norm_w, norm_b, head_w, (const void *)logits,
                         (const void *)workspace}))
        return RWKV7_EINVAL;
    if (dm->H * RWKV7_HEAD_SIZE != dm->D) return RWKV7_EHEAD;
    return rwkv7::decode_step_bf16(dm->B, dm->D, dm->H, dm->L, dm->F, dm->V, dm->Rw, dm->Ra, dm->Rv, dm->Rg, dm->ln_eps, dm->gn_eps,
                                   layer_tbl, layer_tbl_host, x_in, norm_w, norm_b, head_w, head_b, logits, workspace, persistent,
                                   (hipStream_t)stream);
}
size_t rwkv7_decode_wide_workspace_bytes(const rwkv7_decode_dims *dm) {
    if (!dm || dm->H * RWKV7_HEAD_SIZE != dm->D) return 0;
    return rwkv7::decode_wide_workspace_bytes(dm->B, dm->D, dm->H, dm->F, dm->V, dm->Rw, dm->Ra, dm->Rv, dm->Rg);
}
int rwkv7_decode_step_wide_bf16(const rwkv7_decode_dims *dm, const void *const *layer_tbl, const void *const *layer_tbl_host,
                                const void *x_in, const void *norm_w, const void *norm_b, const void *head_w, const void *head_b,
                                float *logits, void *workspace, rwkv7_stream_t stream) {
    if (!dm || any_null({(const void *)layer_tbl, x_in, norm_w, norm_b, head_w, (const void *)logits, (const void *)workspace}))
        return RWKV7_EINVAL;
    if (dm->H * RWKV7_HEAD_SIZE != dm->D) return RWKV7_EHEAD;
    return rwkv7::decode_step_wide_bf16(dm->B, dm->D, dm->H, dm->L, dm->F, dm->V, dm->Rw, dm->Ra, dm->Rv, dm->Rg, dm->ln_eps, dm->gn_eps,
                                        layer_tbl, layer_tbl_host, x_in, norm_w, norm_b, head_w, head_b, logits, workspace,
                                        (hipStream_t)stream);
}
int rwkv7_sample_rows_f32(int rows, int nseg, const float *logits, long ld, const int *seg_off, const int *seg_len, const int *allow_lo,
                          const int *allow_hi, const int *suppress, int nsuppress, int max_domain, int do_sample, int top_k, float top_p,
                          float temperature, unsigned long long seed, const long *step, long *out, rwkv7_stream_t stream) {
    if (rows <= 0 || nseg <= 0 || max_domain <= 0 || nsuppress < 0 ||
        any_null({(const void *)logits, (const void *)seg_off, (const void *)seg_len, (const void *)step, (const void *)out}) ||
        (nsuppress > 0 && !suppress))
        return RWKV7_EINVAL;
    return rwkv7::sample_rows_f32(rows, nseg, logits, ld, seg_off, seg_len, allow_lo, allow_hi, suppress, nsuppress, max_domain, do_sample,
                                  top_k, top_p, temperature, seed, step, out, nullptr, -1, 0, (hipStream_t)stream);
}
int rwkv7_sample_rows_tail_f32(int rows, const float *logits, long ld, const int *seg_off, const int *seg_len, const int *allow_lo,
                               const int *allow_hi, const int *suppress, int nsuppress, int max_domain, int do_sample, int top_k, float top_p,
                               float temperature, unsigned long long seed, const long *step, long *out, const rwkv7_sample_tail *tail,
                               int min_eos_id, long min_eos_until, rwkv7_stream_t stream) {
    if (rows <= 0 || max_domain <= 0 || nsuppress < 0 ||
        any_null({(const void *)logits, (const void *)seg_off, (const void *)seg_len, (const void *)step, (const void *)out}) ||
        (nsuppress > 0 && !suppress))
        return RWKV7_EINVAL;
    return rwkv7::sample_rows_f32(rows, 1, logits, ld, seg_off, seg_len, allow_lo, allow_hi, suppress, nsuppress, max_domain, do_sample, top_k,
                                  top_p, temperature, seed, step, out, tail, min_eos_id, min_eos_until, (hipStream_t)stream);
}
// what rwkv7_sample_slots_f32 and rwkv7_sample_slots_lp_f32 both refuse before a launch
static bool sample_slots_args_ok(int rows, const float *logits, const int *allow_lo, const int *allow_hi, const int *suppress, int nsuppress,
                                 int max_domain, const rwkv7_slot_state *st) {
    if (rows <= 0 || !st || !logits || max_domain <= 0 || nsuppress < 0 || (nsuppress > 0 && !suppress) || (!allow_lo != !allow_hi))
        return false;
    return !(any_null({(const void *)st->step, (const void *)st->limit, (const void *)st->min_until, (const void *)st->seed,
                       (const void *)st->inv_temp, (const void *)st->top_k, (const void *)st->top_p, (const void *)st->do_sample,
                       (const void *)st->live, (const void *)st->ids, (const void *)st->seq}) ||
             st->seq_ld <= 0 || st->slots <= 0 || (st->emb && (!st->x || st->D <= 0)));
}
int rwkv7_sample_slots_f32(int rows, const float *logits, long ld, const int *row_slot, const int *allow_lo, const int *allow_hi,
                           const int *suppress, int nsuppress, int max_domain, const rwkv7_slot_state *st, rwkv7_stream_t stream) {
    if (!sample_slots_args_ok(rows, logits, allow_lo, allow_hi, suppress, nsuppress, max_domain, st)) return RWKV7_EINVAL;
    return rwkv7::sample_slots_f32(rows, logits, ld, row_slot, allow_lo, allow_hi, suppress, nsuppress, max_domain, st, (hipStream_t)stream);
}
int rwkv7_sample_slots_lp_f32(int rows, const float *logits, long ld, const int *row_slot, const int *allow_lo, const int *allow_hi,
                              const int *suppress, int nsuppress, int max_domain, const rwkv7_slot_state *st, const rwkv7_slot_logprob *lp,
                              rwkv7_stream_t stream) {
    if (!sample_slots_args_ok(rows, logits, allow_lo, allow_hi, suppress, nsuppress, max_domain, st)) return RWKV7_EINVAL;
    if (!lp || !lp->tok_lp || !lp->cum_lp) return RWKV7_EINVAL;
    return rwkv7::sample_slots_lp_f32(rows, logits, ld, row_slot, allow_lo, allow_hi, suppress, nsuppress, max_domain, st, lp->tok_lp,
                                      lp->cum_lp, (hipStream_t)stream);
}
int rwkv7_ras_step_f32(int V, const float *logits, long *tok, long *recent, long *ptr, long *step_i, long n_ignore, int eos, float top_p,
                       int top_k, int win_size, float tau_r, unsigned long long seed, rwkv7_stream_t stream) {
    if (V <= 0 || any_null({(const void *)logits, (const void *)tok, (const void *)recent, (const void *)ptr, (const void *)step_i}))
        return RWKV7_EINVAL;
    return rwkv7::ras_step_f32(V, logits, tok, recent, ptr, step_i, n_ignore, eos, top_p, top_k, win_size, tau_r, seed, (hipStream_t)stream);
}
int rwkv7_xy_frame_step(int B, int C, int rows, long text_shift, long speech_vocab, long pad, long eos0, long total, const long *eos_list,
                        int n_eos, int reference_termination, const long *nt, long *out, long *row, long *pos, long *unfinished, long *needs,
                        unsigned char *all_done, long *n_rows, rwkv7_stream_t stream) {
    if (B <= 0 || n_eos < 0 || (n_eos > 0 && !eos_list) ||
        any_null({(const void *)nt, (const void *)out, (const void *)row, (const void *)pos, (const void *)unfinished, (const void *)needs,
                  (const void *)all_done, (const void *)n_rows}))
        return RWKV7_EINVAL;
    return rwkv7::xy_frame_step(B, C, rows, text_shift, speech_vocab, pad, eos0, total, eos_list, n_eos, reference_termination, nt, out, row,
                                pos, unfinished, needs, all_done, n_rows, (hipStream_t)stream);
}
int rwkv7_xy_embed_bf16(int B, int C, int D, const void *const *tables_host, const long *row, void *x, rwkv7_stream_t stream) {
    if (B <= 0 || D <= 0 || any_null({(const void *)tables_host, (const void *)row, (const void *)x})) return RWKV7_EINVAL;
    for (int c = 0; c < C && c < 16; c++)
        if (!tables_host[c]) return RWKV7_EINVAL;
    return rwkv7::xy_embed_bf16(B, C, D, tables_host, row, x, (hipStream_t)stream);
}
static bool xy_slot_state_ok(const rwkv7_xy_slot_state *st) {
    if (!st || st->slots <= 0 || st->C <= 0 || st->D <= 0 || st->seq_ld <= 0 || st->n_eos < 0 || (st->n_eos > 0 && !st->eos_list)) return false;
    if (any_null({(const void *)st->step, (const void *)st->limit, (const void *)st->seed, (const void *)st->inv_temp,
                  (const void *)st->top_k, (const void *)st->top_p, (const void *)st->do_sample, (const void *)st->live,
                  (const void *)st->needs, (const void *)st->nt, (const void *)st->row, (const void *)st->seq, (const void *)st->x}))
        return false;
    for (int c = 0; c < st->C && c < 16; c++)
        if (!st->tables[c]) return false;
    return true;
}
// what rwkv7_xy_slots_draw_f32 and rwkv7_xy_slots_draw_lp_f32 both refuse before a launch
static bool xy_slots_draw_args_ok(int rows, const float *logits, const int *seg_off, const int *seg_len, const int *allow_lo,
                                  const int *allow_hi, int max_domain, const rwkv7_xy_slot_state *st) {
    return !(rows <= 0 || max_domain <= 0 || !xy_slot_state_ok(st) || (!allow_lo != !allow_hi) ||
             any_null({(const void *)logits, (const void *)seg_off, (const void *)seg_len}));
}
int rwkv7_xy_slots_draw_f32(int rows, const float *logits, long ld, const int *row_slot, const int *seg_off, const int *seg_len,
                            const int *allow_lo, const int *allow_hi, int max_domain, const rwkv7_xy_slot_state *st, rwkv7_stream_t stream) {
    if (!xy_slots_draw_args_ok(rows, logits, seg_off, seg_len, allow_lo, allow_hi, max_domain, st)) return RWKV7_EINVAL;
    return rwkv7::xy_slots_draw_f32(rows, logits, ld, row_slot, seg_off, seg_len, allow_lo, allow_hi, max_domain, st, (hipStream_t)stream);
}
int rwkv7_xy_slots_frame_bf16(int rows, const int *row_slot, const rwkv7_xy_slot_state *st, rwkv7_stream_t stream) {
    if (rows <= 0 || !xy_slot_state_ok(st)) return RWKV7_EINVAL;
    return rwkv7::xy_slots_frame_bf16(rows, row_slot, st, (hipStream_t)stream);
}
// one struct serves the two calls of a frame: both entries want all of it
static bool xy_slot_logprob_ok(const rwkv7_xy_slot_logprob *lp) { return lp && lp->ch_lp && lp->frame_lp && lp->cum_lp && lp->n_lp; }
int rwkv7_xy_slots_draw_lp_f32(int rows, const float *logits, long ld, const int *row_slot, const int *seg_off, const int *seg_len,
                               const int *allow_lo, const int *allow_hi, int max_domain, const rwkv7_xy_slot_state *st,
                               const rwkv7_xy_slot_logprob *lp, rwkv7_stream_t stream) {
    if (!xy_slots_draw_args_ok(rows, logits, seg_off, seg_len, allow_lo, allow_hi, max_domain, st)) return RWKV7_EINVAL;
    if (!xy_slot_logprob_ok(lp)) return RWKV7_EINVAL;
    return rwkv7::xy_slots_draw_lp_f32(rows, logits, ld, row_slot, seg_off, seg_len, allow_lo, allow_hi, max_domain, st, lp,
                                       (hipStream_t)stream);
}
int rwkv7_xy_slots_frame_lp_bf16(int rows, const int *row_slot, const rwkv7_xy_slot_state *st, const rwkv7_xy_slot_logprob *lp,
                                 rwkv7_stream_t stream) {
    if (rows <= 0 || !xy_slot_state_ok(st)) return RWKV7_EINVAL;
    if (!xy_slot_logprob_ok(lp)) return RWKV7_EINVAL;
    return rwkv7::xy_slots_frame_lp_bf16(rows, row_slot, st, lp, (hipStream_t)stream);
}
// what rwkv7_ras_slots_f32 and rwkv7_ras_slots_lp_f32 both refuse before a launch
static bool ras_slots_args_ok(int rows, int V, const float *logits, const rwkv7_ras_slot_state *st) {
    if (rows <= 0 || V <= 0 || !st || !logits) return false;
    return !(any_null({(const void *)st->step, (const void *)st->limit, (const void *)st->n_ignore, (const void *)st->seed,
                       (const void *)st->top_k, (const void *)st->top_p, (const void *)st->tau_r, (const void *)st->live,
                       (const void *)st->recent, (const void *)st->ptr, (const void *)st->ids, (const void *)st->n_out,
                       (const void *)st->seq}) ||
             st->slots <= 0 || st->seq_ld <= 0 || (st->emb && (!st->x || st->D <= 0)));
}
int rwkv7_ras_slots_f32(int rows, int V, const float *logits, long ld, const int *row_slot, const rwkv7_ras_slot_state *st,
                        rwkv7_stream_t stream) {
    if (!ras_slots_args_ok(rows, V, logits, st)) return RWKV7_EINVAL;
    return rwkv7::ras_slots_f32(rows, V, logits, ld, row_slot, st, (hipStream_t)stream);
}
int rwkv7_ras_slots_lp_f32(int rows, int V, const float *logits, long ld, const int *row_slot, const rwkv7_ras_slot_state *st,
                           const rwkv7_ras_slot_logprob *lp, rwkv7_stream_t stream) {
    if (!ras_slots_args_ok(rows, V, logits, st)) return RWKV7_EINVAL;
    if (!lp || !lp->tok_lp || !lp->cum_lp || !lp->end_lp) return RWKV7_EINVAL;
    return rwkv7::ras_slots_lp_f32(rows, V, logits, ld, row_slot, st, lp->tok_lp, lp->cum_lp, lp->end_lp, (hipStream_t)stream);
}
int rwkv7_debug_tr16(const void *in, const int *addr, void *out, rwkv7_stream_t stream) {
    if (!in || !addr || !out) return RWKV7_EINVAL;
    return rwkv7::chunk_debug_tr16((const uint16_t *)in, addr, (uint16_t *)out, (hipStream_t)stream);
}
int rwkv7_debug_mma32(const float *X, const float *Y, float *D, float *DT, rwkv7_stream_t stream) {
    if (any_null({X, Y, D, DT})) return RWKV7_EINVAL;
    return rwkv7::chunk_debug_mma(X, Y, D, DT, (hipStream_t)stream);
}

}  // extern "C"
