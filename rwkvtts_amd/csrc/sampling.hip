// rwkvtts_amd/csrc/sampling.hip -- the token draws of the generation loops as ONE launch each (sampling / generation
// control on the device).
//
// Reference semantics:
//   * sample_rows: HF's warper chain that the reference's generate() runs (utils/utilities.py:101-117 -> transformers
//     TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> softmax -> multinomial), model/llm/xy_llm.py:88-101 for the
//     eight channels of an XY frame, or argmax.  As torch operations that chain is ~15 launches per call (topk, sort, softmax,
//     cumsum, scatter, multinomial ...): 0.45 ms per Spark step at B = 32 and 1.8 ms per XY frame (8 calls) on MI355X, against a
//     decode step of 0.98 ms.  Here: one workgroup per (row, channel), the segment's logits in registers (5 / 33 / 60 per thread),
//     the k largest by repeated block-wide maxima of (value, index) keys -- DPP inside the rows of 16, one barrier per round, the
//     owning thread drops its element and rescans its registers -- the nucleus and the draw on one thread.
//   * ras_step: CosyVoice's repetition-aware sampler (third_party/cosyvoice/utils/common.py:109-137: nucleus_sampling + the
//     win_size / tau_r fallback to random_sampling) with the EOS rejection of sampling_ids (model/llm/llm.py:160-176) and the
//     bookkeeping of the streaming loop (previous id, ring of recent ids, step index) in the same launch.
// The draws use a counter-based generator (Philox4x32-10; key = seed, counter = step index, workgroup, draw): the same (seed,
// step) gives the same id in eager runs and in hipGraph replays -- the step index lives in device memory and is advanced by the
// loop itself.  Same distributions as the torch chains (tests/test_sampling_gpu.py), not the same consumption of torch's stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "launchers.h"
#include "sampling_common.h"

namespace rwkv7 {
namespace {

// Optional tail of a one-segment draw: what the decode loop does with the id before the next step (decode.GraphDecoder._step:
// finished sequences emit the pad id, EOS ends a sequence, the id goes into the output row at column *step and becomes the next
// input -- whose embedding row is copied here, so the next step's first kernel finds its input in place).
struct SmpTail {
    unsigned char *unfinished;   // [rows] bool, or null (no EOS handling)
    long eos, pad;
    long *ids;                   // [rows] the ids as the loop keeps them, or null: no tail at all
    long *seq;                   // [rows][seq_ld] generated ids, or null
    long seq_ld;
    const uint16_t *emb;         // [V][D] bf16, or null
    uint16_t *x;                 // [rows][D]
    int D;
};

// ---- one workgroup per (row, segment) ----------------------------------------------------------------------------------------------
template <int EPT>
__global__ __launch_bounds__(kSmpThreads) void sample_rows_kernel(int nseg, const float *__restrict__ logits, long ld,
                                                                  const int *__restrict__ seg_off, const int *__restrict__ seg_len,
                                                                  const int *__restrict__ allow_lo, const int *__restrict__ allow_hi,
                                                                  const int *__restrict__ suppress, int nsuppress, int do_sample, int top_k,
                                                                  float top_p, float inv_temp, uint2 key, const long *__restrict__ step,
                                                                  long *__restrict__ out, SmpTail tail, int min_id, long min_until) {
    __shared__ SmpShared sm;
    const int seg = blockIdx.x % nseg, row = blockIdx.x / nseg, tid = threadIdx.x;
    const float *xg = logits + (long)row * ld + seg_off[seg];
    const int n = seg_len[seg];
    const int lo = allow_lo ? max(allow_lo[seg], 0) : 0, hi = allow_hi ? min(allow_hi[seg], n) : n;
    const int m = hi - lo;
    Vals<EPT> x;
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const int j = tid + kSmpThreads * e;
        const float t = xg[lo + min(j, m - 1)];   // unconditional (clamped): a guarded load is waited for behind its issue
        x.v[e] = j < m ? t * inv_temp : -INFINITY;
    }
    for (int t = 0; t < nsuppress; t++) {   // a handful of ids
        const int sidx = suppress[t] - lo;
        if (sidx >= 0 && sidx < m && (sidx & (kSmpThreads - 1)) == tid) x.drop(sidx);
    }
    if (min_id >= 0 && *step < min_until) {   // min_new_tokens: no EOS before that many draws (HF MinNewTokensLengthLogitsProcessor)
        const int sidx = min_id - lo;
        if (sidx >= 0 && sidx < m && (sidx & (kSmpThreads - 1)) == tid) x.drop(sidx);
    }
    int choice = warper_draw(x, sm, m, do_sample, top_k, top_p, key, do_sample ? *step : 0L, blockIdx.x);
    choice = min(max(choice, 0), m - 1);   // an id outside [lo, lo + m) never reaches the output or the embedding lookup below
    if (tid == 0) out[(long)row * nseg + seg] = lo + choice;
    if (tail.ids) {   // nseg == 1
        __syncthreads();
        if (tid == 0) {
            long id = lo + choice;
            if (tail.unfinished) {
                const bool u = tail.unfinished[row] != 0;
                id = u ? id : tail.pad;
                tail.unfinished[row] = u && id != tail.eos;
            }
            tail.ids[row] = id;
            const long col = *step;
            if (tail.seq && col < tail.seq_ld) tail.seq[(long)row * tail.seq_ld + col] = id;
            sm.sel[0] = (unsigned)id;
        }
        __syncthreads();
        if (tail.emb) copy_emb_row(tail.emb + (long)sm.sel[0] * tail.D, tail.x + (long)row * tail.D, tail.D);
    }
}

// ---- continuous batching: one draw per decode SLOT, each slot with its own request ------------------------------------------------
// = rwkv7_slot_state (include/rwkv7_hip.h).  Every per-slot field is a DEVICE array of `slots` entries.
struct SlotState {
    long *step, *limit, *min_until;
    unsigned long long *seed;
    float *inv_temp;
    int *top_k;
    float *top_p;
    unsigned char *do_sample, *live;
    long *ids, *seq;
    long seq_ld;
    const uint16_t *emb;
    uint16_t *x;
    int D, slots, top_k_max;
    long eos;
};

// Row r of `logits` belongs to slot s = row_slot[r] (row_slot NULL: s = r).  The draw is the one of sample_rows_kernel for a ONE-row
// launch (workgroup 0) with the slot's key, step counter, parameters and min-EOS bound, so a request's ids do not depend on the slot
// it occupies or on when it was admitted; then the slot's bookkeeping (output column, next id, its embedding row, step, live flag).
// Both kernels call the one draw body, warper_draw (csrc/sampling_common.h); this one passes counter word 0 and the slot's key.
//
// LP (rwkv7_sample_slots_lp_f32): the log-probability of the drawn id as well.  Everything under `if constexpr (LP)` is extra; with
// LP = false the body is the draw as it always was.  The probability is the one of the RAW logits (temperature 1, no top-k / top-p)
// over the ids the draw could produce at this step -- the allowed range minus `suppress`, minus EOS while it is barred -- so a second
// copy of the row stays unscaled in registers until its maximum and its exp-sum are known (raw_logprob_stats), which is before
// select_bins needs the registers for its bins: the value depends on the row's contents and the thread layout only, never on the
// row, the slot or the grid.
struct SlotStateLp : SlotState {
    float *tok_lp;    // [slots][seq_ld]
    double *cum_lp;   // [slots]
};
template <int EPT, bool LP>
__global__ __launch_bounds__(kSmpThreads) void sample_slots_kernel(const float *__restrict__ logits, long ld, const int *__restrict__ row_slot,
                                                                   const int *__restrict__ allow_lo, const int *__restrict__ allow_hi,
                                                                   const int *__restrict__ suppress, int nsuppress, int max_domain,
                                                                   typename std::conditional<LP, SlotStateLp, SlotState>::type st) {
    __shared__ SmpShared sm;
    const int row = blockIdx.x, tid = threadIdx.x;
    const int s = row_slot ? row_slot[row] : row;
    if (s < 0 || s >= st.slots || !st.live[s]) return;   // uniform over the workgroup; a slot that is not live is left untouched
    const long step = st.step[s];
    const int do_sample = st.do_sample[s] != 0;
    const float inv_temp = do_sample ? st.inv_temp[s] : 1.f;
    const int top_k = min(max(st.top_k[s], 0), st.top_k_max);
    const float top_p = st.top_p[s];
    const float *xg = logits + (long)row * ld;
    const int lo = allow_lo ? max(allow_lo[0], 0) : 0, hi = allow_hi ? min(allow_hi[0], lo + max_domain) : max_domain;
    const int m = hi - lo;
    Vals<EPT> x;
    Vals<LP ? EPT : 1> raw;   // LP: the same elements at temperature 1
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const int j = tid + kSmpThreads * e;
        const float t = xg[lo + min(j, m - 1)];
        x.v[e] = j < m ? t * inv_temp : -INFINITY;
        if constexpr (LP) raw.v[e] = j < m ? t : -INFINITY;
    }
    for (int t = 0; t < nsuppress; t++) {
        const int sidx = suppress[t] - lo;
        if (sidx >= 0 && sidx < m && (sidx & (kSmpThreads - 1)) == tid) {
            x.drop(sidx);
            if constexpr (LP) raw.drop(sidx);
        }
    }
    if (st.eos >= 0 && step < st.min_until[s]) {
        const long sidx = st.eos - lo;
        if (sidx >= 0 && sidx < m && (sidx & (kSmpThreads - 1)) == tid) {
            x.drop((int)sidx);
            if constexpr (LP) raw.drop((int)sidx);
        }
    }
    float lp_max = 0.f, lp_logz = 0.f;   // LP: max and log sum exp(. - max) over the ids that were not dropped
    if constexpr (LP) raw_logprob_stats(raw, sm, lp_max, lp_logz);
    const uint2 key = make_uint2((uint32_t)st.seed[s], (uint32_t)(st.seed[s] >> 32));
    const int choice = warper_draw(x, sm, m, do_sample, top_k, top_p, key, step, 0u);
    // every thread holds the same choice (it came out of LDS after a barrier), and every read of the slot's state lies before that barrier
    const long id = lo + min(max(choice, 0), m - 1);
    if (tid == 0) {
        if (step >= 0 && step < st.seq_ld) st.seq[(long)s * st.seq_ld + step] = id;
        st.ids[s] = id;
        st.step[s] = step + 1;
        st.live[s] = id != st.eos && step + 1 < st.limit[s];
        if constexpr (LP) {
            // nothing allowed (every id dropped or -inf; the id is the fall-back): -inf, not the NaN of (-inf) - (-inf)
            const float lp = lp_max == -INFINITY ? -INFINITY : (xg[id] - lp_max) - lp_logz;
            if (step >= 0 && step < st.seq_ld) st.tok_lp[(long)s * st.seq_ld + step] = lp;
            st.cum_lp[s] += (double)lp;   // one workgroup owns the slot: a plain read, add, store
        }
    }
    if (st.emb) copy_emb_row(st.emb + id * st.D, st.x + (long)s * st.D, st.D);
}

// ---- CosyVoice streaming step: draw + bookkeeping --------------------------------------------------------------------------------
template <int EPT>
__global__ __launch_bounds__(kSmpThreads) void ras_step_kernel(int V, const float *__restrict__ logits, long *__restrict__ tok,
                                                               long *__restrict__ recent, long *__restrict__ ptr, long *__restrict__ step_i,
                                                               long n_ignore, int eos, float top_p, int top_k, int win_size, float tau_r,
                                                               uint2 key) {
    __shared__ SmpShared sm;
    const int tid = threadIdx.x;
    Vals<EPT> x;
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const int j = tid + kSmpThreads * e;
        const float t = logits[min(j, V - 1)];
        x.v[e] = j < V ? t : -INFINITY;
    }
    const long st = *step_i;
    long rc[2];   // the ring of recent ids, one entry per lane of wave 0 (win_size <= 128)
    rc[0] = recent[min(tid, win_size - 1)];
    rc[1] = recent[min(64 + tid, win_size - 1)];
    const bool ignore_eos = st < n_ignore;
    const uint4 r = philox(make_uint4((uint32_t)st, (uint32_t)((uint64_t)st >> 32), 0u, 0x7a5u), key);
    float mx, z;
    int imx;
    ras_row_stats(x, sm, mx, imx, z);
    const int pick = ras_pick(x, sm, V, mx, imx, z, ignore_eos, eos, top_p, top_k, win_size, tau_r, r, rc);
    if (tid == 0) {   // lane 0 of wave 0, which knows the id
        const long id = pick;
        *tok = id;
        if (id != (long)eos) {   // the reference appends emitted ids only
            const long p = *ptr;
            recent[p] = id;
            *ptr = (p + 1) % win_size;
        }
        *step_i = st + 1;
    }
}

// ---- XY frame: the bookkeeping of CustomGenerationMixin._sample (model/llm/xy_llm.py:104-146) for one frame --------------------------
// One wave, lane = sequence (B <= 64).  The torch form of this (xy_llm._XYFrameState.step) is ~45 launches per frame.  Semantics
// (identical to that function, which stays as the reference path and is compared id for id in tests/test_heads_gpu.py):
//   a non-audio id on channel 0 starts a countdown of C - 1 further rows (needs = C - 1 .. -1); while it runs channel 0 carries EOS
//   (if configured) and channel i keeps its drawn ids for i more rows, then the pad id; finished sequences emit EOS / pad; the row
//   is appended at `pos` while the reference's loop would still be running (`all_done` not yet set); stop = length bound | EOS hit
//   (flushing sequences excepted unless reference_termination); unfinished &= ~stop & ~(needs == -1 [& flushing]).
struct XYFrameArgs {
    int B, C, rows;                 // out is [B][rows][C]
    long text_shift, speech_vocab, pad, eos0, total;   // eos0 < 0: no EOS id; total < 0: no length bound
    int n_eos, reference_termination;
};
__global__ __launch_bounds__(64) void xy_frame_kernel(XYFrameArgs a, const long *__restrict__ nt, const long *__restrict__ eos_list,
                                                      long *__restrict__ out, long *__restrict__ row, long *__restrict__ pos,
                                                      long *__restrict__ unfinished, long *__restrict__ needs_, unsigned char *__restrict__ all_done,
                                                      long *__restrict__ n_rows) {
    const int b = threadIdx.x, C = a.C;
    const bool live = b < a.B;
    const bool running = *all_done == 0;
    const long p0 = *pos;
    const long pw = min(p0, (long)a.rows - 1);                 // where the row goes (clamped like the torch form)
    const long p1 = p0 + (running ? 1 : 0);
    long u = 1, needs = -1;
    if (live) {
        u = unfinished[b];
        needs = needs_[b];
        const long *t = nt + (long)b * C;
        const long t0 = t[0];
        const bool is_audio = t0 >= a.text_shift && t0 < a.text_shift + a.speech_vocab;
        if (!is_audio && needs < 0) needs = C - 1;
        const bool flushing = needs >= 0;
        const long pddp_text = a.eos0 >= 0 ? a.eos0 : 0;
        long c0 = (a.eos0 >= 0 && flushing) ? a.eos0 : t0;
        c0 = u ? c0 : pddp_text;
        long *ob = out + ((long)b * a.rows + pw) * C, *rb = row + (long)b * C;
        if (running) ob[0] = c0;
        rb[0] = c0;
        for (int i = 1; i < C; i++) {
            long ci = (flushing && needs < C - i) ? a.pad : t[i];
            ci = u ? ci : a.pad;
            if (running) ob[i] = ci;
            rb[i] = ci;
        }
        if (flushing) needs -= 1;
        bool stop = a.total >= 0 && p1 >= a.total;
        bool hit = false;
        for (int e = 0; e < a.n_eos; e++) hit |= c0 == eos_list[e];
        stop |= a.reference_termination ? hit : (hit && !flushing);
        const bool gone = a.reference_termination ? needs == -1 : (needs == -1 && flushing);
        const long un = (u && !stop && !gone) ? 1 : 0;
        if (running) {
            unfinished[b] = un;
            needs_[b] = needs;
            u = un;
        }
    }
    const bool any = __ballot(live && u != 0) != 0;            // u: the value `unfinished` holds after this frame
    if (b == 0) {
        *pos = p1;
        *n_rows += running ? 1 : 0;
        if (!any) *all_done = 1;
    }
}

// the next frame's input: x[b] = emb_0[row[b][0]] + emb_1[row[b][1]] + ... in bf16 (xy_embed_sum, csrc/sampling_common.h)
struct XYTables {
    const uint16_t *t[kXYMaxC];
};
__global__ __launch_bounds__(256) void xy_embed_kernel(int C, int D, XYTables tb, const long *__restrict__ row, uint16_t *__restrict__ x) {
    const int b = blockIdx.x;
    xy_embed_sum(C, D, tb.t, row + (long)b * C, x + (long)b * D);
}

}  // namespace

int sample_rows_f32(int rows, int nseg, const float *logits, long ld, const int *seg_off, const int *seg_len, const int *allow_lo,
                    const int *allow_hi, const int *suppress, int nsuppress, int max_domain, int do_sample, int top_k, float top_p,
                    float temperature, unsigned long long seed, const long *step, long *out, const void *tail_, int min_id, long min_until,
                    hipStream_t st) {
    SmpTail tail = {};
    if (tail_) {
        tail = *(const SmpTail *)tail_;
        if (nseg != 1 || !tail.ids || (tail.emb && (tail.D % 8 != 0 || !tail.x))) return -4;
    }
    if (max_domain > kSmpMaxN || nsuppress > 256) return -4;                      // RWKV7_ESHAPE
    if (do_sample && (top_k < 0 || top_k > 64 || (top_k == 0 && top_p < 1.f) || !(temperature > 0.f))) return -4;
    (void)hipGetLastError();
    const float it = do_sample ? 1.f / temperature : 1.f;
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    const dim3 grid(rows * nseg), block(kSmpThreads);
    for_ept(max_domain, [&](auto ept) {
        sample_rows_kernel<decltype(ept)::value><<<grid, block, 0, st>>>(nseg, logits, ld, seg_off, seg_len, allow_lo, allow_hi, suppress, nsuppress,
                                                                         do_sample, top_k, top_p, it, key, step, out, tail, min_id, min_until);
    });
    return (int)hipGetLastError();
}

template <bool LP, typename State>
static int launch_sample_slots(int rows, const float *logits, long ld, const int *row_slot, const int *allow_lo, const int *allow_hi,
                               const int *suppress, int nsuppress, int max_domain, const State &st, hipStream_t stream) {
    if (max_domain > kSmpMaxN || nsuppress > 256 || st.top_k_max < 0 || st.top_k_max > 64 || (st.emb && st.D % 8 != 0)) return -4;
    (void)hipGetLastError();
    const dim3 grid(rows), block(kSmpThreads);
    for_ept(max_domain, [&](auto ept) {
        sample_slots_kernel<decltype(ept)::value, LP><<<grid, block, 0, stream>>>(logits, ld, row_slot, allow_lo, allow_hi, suppress, nsuppress,
                                                                                  max_domain, st);
    });
    return (int)hipGetLastError();
}

int sample_slots_f32(int rows, const float *logits, long ld, const int *row_slot, const int *allow_lo, const int *allow_hi,
                     const int *suppress, int nsuppress, int max_domain, const void *st_, hipStream_t stream) {
    return launch_sample_slots<false>(rows, logits, ld, row_slot, allow_lo, allow_hi, suppress, nsuppress, max_domain, *(const SlotState *)st_, stream);
}

int sample_slots_lp_f32(int rows, const float *logits, long ld, const int *row_slot, const int *allow_lo, const int *allow_hi,
                        const int *suppress, int nsuppress, int max_domain, const void *st_, float *tok_lp, double *cum_lp, hipStream_t stream) {
    SlotStateLp st;
    static_cast<SlotState &>(st) = *(const SlotState *)st_;
    st.tok_lp = tok_lp;
    st.cum_lp = cum_lp;
    return launch_sample_slots<true>(rows, logits, ld, row_slot, allow_lo, allow_hi, suppress, nsuppress, max_domain, st, stream);
}

int ras_step_f32(int V, const float *logits, long *tok, long *recent, long *ptr, long *step_i, long n_ignore, int eos, float top_p,
                 int top_k, int win_size, float tau_r, unsigned long long seed, hipStream_t st) {
    if (V > kSmpMaxN || top_k < 1 || top_k > kSmpMaxCand || win_size < 1 || win_size > 128) return -4;
    (void)hipGetLastError();
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    for_ept(V, [&](auto ept) {
        ras_step_kernel<decltype(ept)::value><<<dim3(1), dim3(kSmpThreads), 0, st>>>(V, logits, tok, recent, ptr, step_i, n_ignore, eos, top_p, top_k,
                                                                                     win_size, tau_r, key);
    });
    return (int)hipGetLastError();
}

int xy_frame_step(int B, int C, int rows, long text_shift, long speech_vocab, long pad, long eos0, long total, const long *eos_list, int n_eos,
                  int reference_termination, const long *nt, long *out, long *row, long *pos, long *unfinished, long *needs,
                  unsigned char *all_done, long *n_rows, hipStream_t st) {
    if (B > 64 || C < 1 || rows < 1) return -4;
    XYFrameArgs a;
    a.B = B; a.C = C; a.rows = rows;
    a.text_shift = text_shift; a.speech_vocab = speech_vocab; a.pad = pad; a.eos0 = eos0; a.total = total;
    a.n_eos = n_eos; a.reference_termination = reference_termination;
    (void)hipGetLastError();
    xy_frame_kernel<<<dim3(1), dim3(64), 0, st>>>(a, nt, eos_list, out, row, pos, unfinished, needs, all_done, n_rows);
    return (int)hipGetLastError();
}

int xy_embed_bf16(int B, int C, int D, const void *const *tables_host, const long *row, void *x, hipStream_t st) {
    if (C < 1 || C > kXYMaxC || D % 8 != 0) return -4;
    XYTables tb;
    for (int c = 0; c < kXYMaxC; c++) tb.t[c] = (const uint16_t *)tables_host[c < C ? c : 0];
    (void)hipGetLastError();
    xy_embed_kernel<<<dim3(B), dim3(256), 0, st>>>(C, D, tb, row, (uint16_t *)x);
    return (int)hipGetLastError();
}

}  // namespace rwkv7
