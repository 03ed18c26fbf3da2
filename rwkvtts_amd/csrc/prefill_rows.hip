// rwkvtts_amd/csrc/prefill_rows.hip -- the row stage of the stateful packed prefill (rwkvtts_amd/prefill.py, PackedPrefill), bf16,
// forward only, no tape:
//   x1 = x + branch ; h = LN(x1) ; hm = h * mask ; out_i[t] = hm[t] + (pred[t] - hm[t]) p_i
// on a packed row [T, D] whose sequences carry their token-shift predecessor in and out of chosen rows of a cache field
// x_prev [S, D].  It is add_ln_mix_fwd_kernel (elementwise.hip: same runs of rows, same row routine add_ln_row of ln_row.h, so x1 and
// every ordinary row come out with the same bits) with two per-row int32 maps that live on the DEVICE and are read here:
//   prev_src[t]  -1: pred = hm[t-1] (0 for t = 0)   -2: pred = 0 (first token of a fresh sequence)   r >= 0: pred = x_prev_rd[r]
//   last_dst[t]  -1: nothing                        r >= 0: hm[t] -> x_prev[r]
// Nothing about a particular pack reaches the launch, so one captured launch per shape serves every pack.  In one launch it does what
// add_layer_norm + token_shift_mix6/1 + the carried first rows + the stored last rows take on the eager path (6 + 6 + 2 gather /
// scatter groups per layer there).  The scan's twin, on indexed state rows, is an instantiation of wkv7_chunk_fwd9.hip's kernel
// (chunk_fwd9_state_rows_bf16 there).
//
// x_prev_rd and x_prev may be the same field: a row that reads and writes the same r reads first, inside the thread that owns the
// channels.  Two DIFFERENT rows of one launch that read and write the same r (the first and the last row of a longer piece) race
// unless x_prev_rd is a snapshot.  r is not range-checked: device data, the caller's guarantee (include/rwkv7_hip.h).
#include "launchers.h"
#include "ln_row.h"

namespace rwkv7 {

template <int NMIX>
__global__ __launch_bounds__(kEwMaxThreads) void add_ln_mix_rows_kernel(int T_, int D, int run_len, const bf16_t *__restrict__ x,
                                                                        const bf16_t *__restrict__ branch, const bf16_t *__restrict__ gamma,
                                                                        const bf16_t *__restrict__ beta, float eps,
                                                                        const bf16_t *__restrict__ mask, const bf16_t *__restrict__ params,
                                                                        const int *__restrict__ prev_src, const int *__restrict__ last_dst,
                                                                        const bf16_t *x_prev_rd, bf16_t *x_prev, bf16_t *__restrict__ x_out,
                                                                        bf16_t *__restrict__ out) {
    using T = bf16_t;
    __shared__ __attribute__((aligned(16))) float red[4][kEwMaxThreads / 8];
    red_init<4>(red);
    const int c = threadIdx.x * 8, ng = D / 64;
    const long rows = T_;
    const float inv_d = 1.0f / (float)D;
    float gm[8], bt[8], p[NMIX][8];
    V8<T>::ld(gamma + c, gm);
    if (beta) {
        V8<T>::ld(beta + c, bt);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) bt[j] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < NMIX; i++) V8<T>::ld(params + (long)i * D + c, p[i]);
    int ph = 0;
    // unconditional loads issued one row ahead, as in add_ln_mix_fwd_kernel; the two map entries ride with them
    const bool has_branch = branch != nullptr, has_mask = mask != nullptr;
    const T *const brq = has_branch ? branch : x;
    const T *const maskq = has_mask ? mask : gamma;
    struct Pre {
        RowPre<T> r;
        int ps, ld;
    };
    auto fetch = [&](long row) {
        Pre f;
        f.r.xv.load(x + row * D + c);
        f.r.bv.load(brq + row * D + c);
        f.r.m = V8<T>::ld1(maskq + (has_mask ? row : 0));
        f.ps = prev_src[row];
        f.ld = last_dst[row];
        return f;
    };
    for (long r_lo = (long)blockIdx.x * run_len; r_lo < rows; r_lo += (long)gridDim.x * run_len) {
        const long r_hi = r_lo + run_len < rows ? r_lo + run_len : rows;
        const long first = r_lo != 0 ? r_lo - 1 : r_lo;    // the neighbour row is re-normalised at the start of a run
        float hp[8];
#pragma unroll
        for (int j = 0; j < 8; j++) hp[j] = 0.f;
        Pre A = fetch(first);
        for (long row = first; row < r_hi; row++) {
            const Pre Bn = fetch(row + 1 < r_hi ? row + 1 : row);
            __builtin_amdgcn_sched_barrier(0);
            const bool write = row >= r_lo;
            float hc[8], mu, rs;
            add_ln_row<T>(A.r, row * D + c, has_branch, has_mask, write, x_out, (T *)nullptr, gm, bt, inv_d, eps, ng, red, ph, mu, rs, hc);
            if (write) {
                const int ps = A.ps, ld = A.ld;
                const float keep = (row != 0 && ps == -1) ? 1.f : 0.f;   // row 0 and a fresh sequence's first token: shift(x) = 0
#pragma unroll
                for (int j = 0; j < 8; j++) hp[j] *= keep;
                if (ps >= 0) V8<T>::ld(x_prev_rd + (long)ps * D + c, hp);   // the carried predecessor (rare rows: behind its branch)
#pragma unroll
                for (int i = 0; i < NMIX; i++) {
                    float o[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) o[j] = fmaf(hp[j] - hc[j], p[i][j], hc[j]);
                    V8<T>::st(out + ((long)i * rows + row) * D + c, o);
                }
                if (ld >= 0) {
                    // read before write when this row's ps names the same cache row: the load above has returned before the store leaves
                    if (ps >= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    V8<T>::st(x_prev + (long)ld * D + c, hc);   // hc is already rounded to bf16: the store is exact
                }
            }
#pragma unroll
            for (int j = 0; j < 8; j++) hp[j] = hc[j];
            A = Bn;
        }
    }
}

int add_ln_mix_rows_fwd_bf16(int T_, int D, int nmix, const void *x, const void *branch, const void *gamma, const void *beta, float eps,
                             const void *mask, const void *params, const int *prev_src, const int *last_dst, const void *x_prev_rd,
                             void *x_prev, void *x_out, void *out, int nblocks, int run_len, hipStream_t st) {
    using T = bf16_t;
    return for_nmix<1, 6>(nmix, [&](auto n) {
        return launch_rows(add_ln_mix_rows_kernel<decltype(n)::value>, nblocks, D, st, T_, D, run_len, (const T *)x, (const T *)branch,
                           (const T *)gamma, (const T *)beta, eps, (const T *)mask, (const T *)params, prev_src, last_dst,
                           (const T *)x_prev_rd, (T *)x_prev, (T *)x_out, (T *)out);
    });
}

}  // namespace rwkv7
