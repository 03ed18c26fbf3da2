// rwkvtts_amd/csrc/xy_slots.hip -- one XY frame per decode SLOT of a continuous-batching engine (rwkvtts_amd/continuous_xy.py), where
// every slot runs its own request: its own Philox key, frame counter, frame budget, sampling parameters, flush countdown and live
// flag, all in device memory.  Two launches per frame (the closed-batch loop of xy_llm.RWKV7XYLM.generate takes three: draw, frame
// rules, embedding sum):
//   1. xy_slot_draw_kernel: one workgroup per (logits row, channel) -- the C draws of a slot run side by side, not one after the other
//      inside a workgroup (a block-wide selection costs about as much as a launch boundary).  The draw is sample_rows_kernel's for a
//      ONE-row launch of C segments: workgroup index = channel, key = seed[s], counter = (step[s], channel).  Writes nt[s][c].
//   2. xy_slot_frame_kernel: one workgroup per logits row.  Lane 0 applies the frame rules of xy_frame_kernel for a batch of one
//      (pos = step[s], total = limit[s], still running) and leaves the row in LDS; after the barrier every lane adds the C embedding
//      rows like xy_embed_kernel (bf16 rounding after each addition, channel order) with 16-byte loads.
// A slot with live[s] == 0, and a row whose row_slot entry lies outside [0, slots), is left completely untouched by both launches.
//
// LP (rwkv7_xy_slots_draw_lp_f32 / rwkv7_xy_slots_frame_lp_bf16; ContinuousXYDecoder(logprobs=True)): the log-probability of what a
// frame drew as well.  The draw writes every channel's value (ch_lp); which of them COUNT is only known once the frame rules have
// decided which drawn ids the frame keeps, so the frame kernel does the accounting (frame_lp, cum_lp, n_lp).  Everything new sits
// under `if constexpr (LP)`; with LP = false both bodies are what they always were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "launchers.h"
#include "sampling_common.h"

namespace rwkv7 {
namespace {

// = rwkv7_xy_slot_state (include/rwkv7_hip.h).  Every per-slot field is a DEVICE array of `slots` entries.
struct XYSlotState {
    long *step, *limit;
    unsigned long long *seed;
    float *inv_temp;
    int *top_k;
    float *top_p;
    unsigned char *do_sample, *live;
    long *needs;
    long *nt, *row, *seq;
    long seq_ld;
    const uint16_t *tables[kXYMaxC];
    uint16_t *x;
    int D, C, slots, top_k_max;
    long text_shift, speech_vocab, pad, eos0;
    const long *eos_list;
    int n_eos, reference_termination;
};

// = rwkv7_xy_slot_state followed by the members of rwkv7_xy_slot_logprob: what the LP instantiations get
struct XYSlotStateLp : XYSlotState {
    float *ch_lp;      // [slots][C]
    float *frame_lp;   // [slots][seq_ld][C]
    double *cum_lp;    // [slots]
    long *n_lp;        // [slots]
};
template <bool LP>
using XYState = typename std::conditional<LP, XYSlotStateLp, XYSlotState>::type;

// The draw is the body sample_rows_kernel (csrc/sampling.hip) calls too, warper_draw (csrc/sampling_common.h), with the slot's
// parameters in place of the launch's: same loads, counter word 2 = channel, key = seed[s], so the id equals that kernel's bit for bit.
//
// LP: ch_lp[s][c] = the drawn id's log-probability under the RAW logits (temperature 1, no top-k / top-p) over the channel's allowed
// range.  A second copy of the range stays unscaled in registers until its maximum and its exp-sum are known (raw_logprob_stats), which
// is before select_bins needs the registers for its bins: the value depends on the range's contents and the thread layout only, never
// on the row, the slot or the grid.
template <int EPT, bool LP>
__global__ __launch_bounds__(kSmpThreads) void xy_slot_draw_kernel(const float *__restrict__ logits, long ld, const int *__restrict__ row_slot,
                                                                   const int *__restrict__ seg_off, const int *__restrict__ seg_len,
                                                                   const int *__restrict__ allow_lo, const int *__restrict__ allow_hi,
                                                                   XYState<LP> st) {
    __shared__ SmpShared sm;
    const int C = st.C;
    const int seg = blockIdx.x % C, row = blockIdx.x / C, tid = threadIdx.x;
    const int s = row_slot ? row_slot[row] : row;
    if (s < 0 || s >= st.slots || !st.live[s]) return;   // uniform over the workgroup
    const long step = st.step[s];
    const int do_sample = st.do_sample[s] != 0;
    const float inv_temp = do_sample ? st.inv_temp[s] : 1.f;
    const int top_k = min(max(st.top_k[s], 0), st.top_k_max);
    const float top_p = st.top_p[s];
    const float *xg = logits + (long)row * ld + seg_off[seg];
    const int n = seg_len[seg];
    const int lo = allow_lo ? max(allow_lo[seg], 0) : 0, hi = allow_hi ? min(allow_hi[seg], n) : n;
    const int m = hi - lo;
    if (m < 1) return;   // an empty allowed range: nothing is read (uniform)
    Vals<EPT> x;
    Vals<LP ? EPT : 1> raw;   // LP: the same elements at temperature 1
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const int j = tid + kSmpThreads * e;
        const float t = xg[lo + min(j, m - 1)];
        x.v[e] = j < m ? t * inv_temp : -INFINITY;
        if constexpr (LP) raw.v[e] = j < m ? t : -INFINITY;
    }
    float lp_max = 0.f, lp_logz = 0.f;   // LP: max and log sum exp(. - max) over the allowed range
    if constexpr (LP) raw_logprob_stats(raw, sm, lp_max, lp_logz);
    const uint2 key = make_uint2((uint32_t)st.seed[s], (uint32_t)(st.seed[s] >> 32));
    int choice = warper_draw(x, sm, m, do_sample, top_k, top_p, key, step, (uint32_t)seg);
    choice = min(max(choice, 0), m - 1);
    if (tid == 0) {
        st.nt[(long)s * C + seg] = lo + choice;
        // no finite logit in the range (the id is the fall-back): -inf, not the NaN of (-inf) - (-inf)
        if constexpr (LP) st.ch_lp[(long)s * C + seg] = lp_max == -INFINITY ? -INFINITY : (xg[lo + choice] - lp_max) - lp_logz;
    }
}

// Frame rules (xy_frame_kernel for B = 1, pos = step[s], total = limit[s], all_done = 0) + the next input (xy_embed_kernel).
//
// LP: which of the C draws COUNT is a function of the slot's state alone (ids are never compared: a drawn id that happens to equal the
// pad id is not misjudged).  Channel 0 counts iff the flush had not started before this frame (needs < 0 at entry): its id was the
// model's free choice, even when eos0 is written in its place.  Channel i >= 1 counts iff the rule below keeps its drawn id.  Lane 0
// writes frame_lp (the counted channels' ch_lp, +0 for a forced one) at the frame's row of seq, adds the counted values to cum_lp in
// channel order in fp64 (one workgroup owns the slot: a plain read, add, store) and their number to n_lp.
template <bool LP>
__global__ __launch_bounds__(256) void xy_slot_frame_kernel(const int *__restrict__ row_slot, XYState<LP> st) {
    __shared__ long frame[kXYMaxC];
    __shared__ long next[3];   // needs, step, live after this frame
    const int C = st.C, D = st.D, tid = threadIdx.x;
    const int s = row_slot ? row_slot[blockIdx.x] : (int)blockIdx.x;
    if (s < 0 || s >= st.slots || !st.live[s]) return;   // uniform: every lane reads live[s] before the barrier, lane 0 writes it after
    if (tid == 0) {
        const long p0 = st.step[s];
        long needs = st.needs[s];
        [[maybe_unused]] const long needs_in = needs;   // LP: the countdown as this frame found it
        const long *t = st.nt + (long)s * C;
        const long t0 = t[0];
        const bool is_audio = t0 >= st.text_shift && t0 < st.text_shift + st.speech_vocab;
        if (!is_audio && needs < 0) needs = C - 1;
        const bool flushing = needs >= 0;
        const long c0 = (st.eos0 >= 0 && flushing) ? st.eos0 : t0;
        frame[0] = c0;
        for (int i = 1; i < C; i++) frame[i] = (flushing && needs < C - i) ? st.pad : t[i];
        if constexpr (LP) {
            const long pw = min(max(p0, 0L), st.seq_ld - 1);   // the row seq gets below
            float *fl = st.frame_lp + ((long)s * st.seq_ld + pw) * C;
            const float *cl = st.ch_lp + (long)s * C;
            double cum = st.cum_lp[s];
            long counted = 0;
            for (int i = 0; i < C; i++) {
                const bool counts = i == 0 ? needs_in < 0 : !(flushing && needs < C - i);
                const float v = counts ? cl[i] : 0.f;
                fl[i] = v;
                if (counts) {
                    cum += (double)v;
                    counted++;
                }
            }
            st.cum_lp[s] = cum;
            st.n_lp[s] += counted;
        }
        if (flushing) needs -= 1;
        const long p1 = p0 + 1;
        const long total = st.limit[s];
        bool stop = total >= 0 && p1 >= total;
        bool hit = false;
        for (int e = 0; e < st.n_eos; e++) hit |= c0 == st.eos_list[e];
        stop |= st.reference_termination ? hit : (hit && !flushing);
        const bool gone = st.reference_termination ? needs == -1 : (needs == -1 && flushing);
        next[0] = needs;
        next[1] = p1;
        next[2] = (!stop && !gone) ? 1 : 0;
    }
    __syncthreads();
    if (tid < C) {
        const long p0 = next[1] - 1;
        const long pw = min(max(p0, 0L), st.seq_ld - 1);   // clamped like xy_frame_kernel
        st.seq[((long)s * st.seq_ld + pw) * C + tid] = frame[tid];
        st.row[(long)s * C + tid] = frame[tid];
    }
    if (tid == 0) {
        st.needs[s] = next[0];
        st.step[s] = next[1];
        st.live[s] = (unsigned char)next[2];
    }
    xy_embed_sum(C, D, st.tables, frame, st.x + (long)s * D);
}

}  // namespace

template <bool LP>
static int launch_xy_draw(int rows, const float *logits, long ld, const int *row_slot, const int *seg_off, const int *seg_len,
                          const int *allow_lo, const int *allow_hi, int max_domain, const XYState<LP> &st, hipStream_t stream) {
    if (max_domain > kSmpMaxN || st.top_k_max < 0 || st.top_k_max > 64 || st.C > kXYMaxC || st.D % 8 != 0) return -4;   // RWKV7_ESHAPE
    (void)hipGetLastError();
    const dim3 grid(rows * st.C), block(kSmpThreads);
    for_ept(max_domain, [&](auto ept) {
        xy_slot_draw_kernel<decltype(ept)::value, LP><<<grid, block, 0, stream>>>(logits, ld, row_slot, seg_off, seg_len, allow_lo, allow_hi, st);
    });
    return (int)hipGetLastError();
}

template <bool LP>
static int launch_xy_frame(int rows, const int *row_slot, const XYState<LP> &st, hipStream_t stream) {
    if (st.C > kXYMaxC || st.D % 8 != 0) return -4;
    (void)hipGetLastError();
    xy_slot_frame_kernel<LP><<<dim3(rows), dim3(256), 0, stream>>>(row_slot, st);
    return (int)hipGetLastError();
}

// st + lp (the header's rwkv7_xy_slot_logprob: four pointers in the order of XYSlotStateLp's own members)
static XYSlotStateLp with_lp(const void *st_, const void *lp_) {
    struct Lp {
        float *ch_lp, *frame_lp;
        double *cum_lp;
        long *n_lp;
    };
    const Lp lp = *(const Lp *)lp_;
    XYSlotStateLp st;
    static_cast<XYSlotState &>(st) = *(const XYSlotState *)st_;
    st.ch_lp = lp.ch_lp;
    st.frame_lp = lp.frame_lp;
    st.cum_lp = lp.cum_lp;
    st.n_lp = lp.n_lp;
    return st;
}

int xy_slots_draw_f32(int rows, const float *logits, long ld, const int *row_slot, const int *seg_off, const int *seg_len,
                      const int *allow_lo, const int *allow_hi, int max_domain, const void *st_, hipStream_t stream) {
    return launch_xy_draw<false>(rows, logits, ld, row_slot, seg_off, seg_len, allow_lo, allow_hi, max_domain, *(const XYSlotState *)st_, stream);
}

int xy_slots_draw_lp_f32(int rows, const float *logits, long ld, const int *row_slot, const int *seg_off, const int *seg_len,
                         const int *allow_lo, const int *allow_hi, int max_domain, const void *st_, const void *lp_, hipStream_t stream) {
    return launch_xy_draw<true>(rows, logits, ld, row_slot, seg_off, seg_len, allow_lo, allow_hi, max_domain, with_lp(st_, lp_), stream);
}

int xy_slots_frame_bf16(int rows, const int *row_slot, const void *st_, hipStream_t stream) {
    return launch_xy_frame<false>(rows, row_slot, *(const XYSlotState *)st_, stream);
}

int xy_slots_frame_lp_bf16(int rows, const int *row_slot, const void *st_, const void *lp_, hipStream_t stream) {
    return launch_xy_frame<true>(rows, row_slot, with_lp(st_, lp_), stream);
}

}  // namespace rwkv7
