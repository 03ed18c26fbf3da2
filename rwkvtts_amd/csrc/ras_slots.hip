// rwkvtts_amd/csrc/ras_slots.hip -- CosyVoice's repetition-aware draw per decode SLOT of a continuous-batching engine
// (rwkvtts_amd/continuous_cosy.py), where every slot runs its own utterance: its own Philox key, loop index, EOS bar (n_ignore),
// length bound, top_k / top_p / tau_r, ring of recent ids and live flag, all in device memory.  One launch per captured step:
// one workgroup per logits row draws the slot's id as ras_step_kernel (csrc/sampling.hip) does for B = 1 and then does what the
// streaming loop of RWKV7CosyLM.inference does with it (ring, emitted ids, next input embedding, loop index, end of utterance).
// A slot with live[s] == 0, and a row whose row_slot entry lies outside [0, slots), is left completely untouched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "launchers.h"
#include "sampling_common.h"

namespace rwkv7 {
namespace {

// = rwkv7_ras_slot_state (include/rwkv7_hip.h).  Every per-slot field is a DEVICE array of `slots` entries.
struct RasSlotState {
    long *step, *limit, *n_ignore;
    unsigned long long *seed;
    int *top_k;
    float *top_p, *tau_r;
    unsigned char *live;
    long *recent;
    long win_ld;
    long *ptr, *ids, *n_out, *seq;
    long seq_ld;
    const uint16_t *emb;
    uint16_t *x;
    int D, slots, win_size, top_k_max;
    long eos;
};

// = rwkv7_ras_slot_state followed by the members of rwkv7_ras_slot_logprob: what the LP instantiation gets
struct RasSlotStateLp : RasSlotState {
    float *tok_lp;    // [slots][seq_ld]
    double *cum_lp;   // [slots]
    float *end_lp;    // [slots]
};

// The draw is the one body that ras_step_kernel calls too (ras_row_stats + ras_pick, csrc/sampling_common.h), with the slot's fields
// in place of the launch's arguments, so the id equals that kernel's bit for bit.  Every lane reads live[s], step[s] and the
// ring before the first barrier; lane 0 writes them after the last one, so the early exit is uniform over the workgroup.
//
// LP (rwkv7_ras_slots_lp_f32): the log-probability of the drawn id as well.  Everything under `if constexpr (LP)` is extra; with
// LP = false the body is the draw as it always was.  The probability is the one of the RAW logits (temperature 1, before top-k /
// top-p and the repetition test): the draw already holds the row's maximum mx and z = sum exp(x - mx) in registers.  While EOS is
// barred it cannot be drawn, so it is left out of the sum: the masked terms are added up on their own (per thread, wave butterfly,
// the four waves in fixed order, as z is), never as z - exp(x[eos] - mx), which cancels when EOS holds the row's mass.
template <int EPT, bool LP>
__global__ __launch_bounds__(kSmpThreads) void ras_slots_kernel(int V, const float *__restrict__ logits_, long ld,
                                                                const int *__restrict__ row_slot,
                                                                typename std::conditional<LP, RasSlotStateLp, RasSlotState>::type a) {
    __shared__ SmpShared sm;
    const int tid = threadIdx.x;
    const int s = row_slot ? row_slot[blockIdx.x] : (int)blockIdx.x;
    if (s < 0 || s >= a.slots || !a.live[s]) return;
    const float *logits = logits_ + (long)blockIdx.x * ld;
    Vals<EPT> x;
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const int j = tid + kSmpThreads * e;
        const float t = logits[min(j, V - 1)];
        x.v[e] = j < V ? t : -INFINITY;
    }
    const long st = a.step[s];
    const int win_size = a.win_size, eos = (int)a.eos;
    long *recent = a.recent + (long)s * a.win_ld;
    long rc[2];   // the ring of recent ids, one entry per lane of wave 0 (win_size <= 128)
    rc[0] = recent[min(tid, win_size - 1)];
    rc[1] = recent[min(64 + tid, win_size - 1)];
    const float top_p = a.top_p[s], tau_r = a.tau_r[s];
    const int top_k = min(max(a.top_k[s], 1), a.top_k_max);
    const bool ignore_eos = st < a.n_ignore[s];
    const uint2 key = make_uint2((uint32_t)a.seed[s], (uint32_t)(a.seed[s] >> 32));
    const uint4 r = philox(make_uint4((uint32_t)st, (uint32_t)((uint64_t)st >> 32), 0u, 0x7a5u), key);
    float mx, z;
    int imx;
    ras_row_stats(x, sm, mx, imx, z);
    float lp_z = z;   // LP: the exp-sum over the ids this draw can produce
    if constexpr (LP) {
        if (ignore_eos) {   // uniform over the workgroup
            float ws = 0.f;
#pragma unroll
            for (int e = 0; e < EPT; e++) ws += tid + kSmpThreads * e == eos ? 0.f : __expf(x.v[e] - mx);
            lp_z = block_sum(ws, sm);
        }
    }
    const int pick = ras_pick(x, sm, V, mx, imx, z, ignore_eos, eos, top_p, top_k, win_size, tau_r, r, rc);
    if (tid == 0) sm.sel[3] = (unsigned)pick;   // lane 0 of wave 0, which knows the id
    __syncthreads();
    // every thread holds the same id (it came out of LDS after a barrier); all reads of the slot's state that other lanes make lie
    // before that barrier
    const long id = min(max((int)sm.sel[3], 0), V - 1);
    const bool emit = id != (long)eos;   // the reference appends emitted ids only
    if (tid == 0) {
        a.ids[s] = id;
        if (emit) {
            const long n = a.n_out[s], p = a.ptr[s];
            if (n >= 0 && n < a.seq_ld) a.seq[(long)s * a.seq_ld + n] = id;
            if (p >= 0 && p < win_size) recent[p] = id;
            a.ptr[s] = (p + 1) % win_size;
            a.n_out[s] = n + 1;
        }
        a.step[s] = st + 1;
        a.live[s] = emit && st + 1 < a.limit[s];
        if constexpr (LP) {
            // no finite logit in the row, or none with any mass next to a barred EOS (the id is a fall-back): -inf, not a NaN
            const float lp = mx == -INFINITY || !(lp_z > 0.f) ? -INFINITY : (logits[id] - mx) - __logf(lp_z);
            if (emit) {
                const long n = a.n_out[s] - 1;   // the column seq got above
                if (n >= 0 && n < a.seq_ld) a.tok_lp[(long)s * a.seq_ld + n] = lp;
                a.cum_lp[s] += (double)lp;   // one workgroup owns the slot: a plain read, add, store
            } else {
                a.end_lp[s] = lp;
            }
        }
    }
    if (emit && a.emb) copy_emb_row(a.emb + id * a.D, a.x + (long)s * a.D, a.D);
}

}  // namespace

template <bool LP, typename State>
static int launch_ras_slots(int rows, int V, const float *logits, long ld, const int *row_slot, const State &st, hipStream_t stream) {
    if (V > kSmpMaxN || st.win_size < 1 || st.win_size > 128 || st.win_size > st.win_ld || st.top_k_max < 1 || st.top_k_max > kSmpMaxCand ||
        (st.emb && st.D % 8 != 0))
        return -4;   // RWKV7_ESHAPE
    (void)hipGetLastError();
    const dim3 grid(rows), block(kSmpThreads);
    for_ept(V, [&](auto ept) { ras_slots_kernel<decltype(ept)::value, LP><<<grid, block, 0, stream>>>(V, logits, ld, row_slot, st); });
    return (int)hipGetLastError();
}

int ras_slots_f32(int rows, int V, const float *logits, long ld, const int *row_slot, const void *st_, hipStream_t stream) {
    return launch_ras_slots<false>(rows, V, logits, ld, row_slot, *(const RasSlotState *)st_, stream);
}

int ras_slots_lp_f32(int rows, int V, const float *logits, long ld, const int *row_slot, const void *st_, float *tok_lp, double *cum_lp,
                     float *end_lp, hipStream_t stream) {
    RasSlotStateLp st;
    static_cast<RasSlotState &>(st) = *(const RasSlotState *)st_;
    st.tok_lp = tok_lp;
    st.cum_lp = cum_lp;
    st.end_lp = end_lp;
    return launch_ras_slots<true>(rows, V, logits, ld, row_slot, st, stream);
}

}  // namespace rwkv7
