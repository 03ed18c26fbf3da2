// rwkvtts_amd/csrc/decode_step.hip -- one greedy-decode step (T = 1, B <= 32 sequences) of the whole RWKV-7 stack on gfx950
// (BASELINE.json configs[4]: "persistent-state decode kernel").
//
// Reference: the per-token path RWKV_x070.forward_one (model/llm/rwkv_s2s_single_ffn.py:417-445) with
// RWKV_x070_TMix_one (:482-506) and RWKV_x070_CMix_one (:545-549); batched form forward_batch at T = 1
// (model/llm/rwkv_asr_cuda_whisper.py:438-472).  Module by module a step is ~18 launches per layer; even replayed from a
// hipGraph that is 430 launches and 4.0 ms for a step whose HBM traffic (0.65 GB of weights + 0.4 GB of state) would take
// 0.13 ms.
//
// Here the step is 7 grid-wide phases per layer:
//   P0 row    x += previous channel-mix output (K-split partials); h = LayerNorm1(x); six token-shift lerps -> bf16 rows;
//             att_x_prev <- h                                                      (rwkv_s2s_single_ffn.py:486-487)
//   P1 gemv   r, k, v projections and the four low-rank down projections in one sweep: [32 x K] . W^T on MFMA, the batch
//             rows are the 32-wide B operand, K split over waves and workgroups -> fp32 partials   (:489-491,497-500)
//   P2 head   per (head, 2 sequences): low-rank up projections (+ tanh / sigmoid), decay, value residual, kk
//             normalisation, the 64x64 fp32 state update in place, y, GroupNorm, bonus, gate -> bf16 rows   (:493-505)
//   P3 gemv   output projection -> partials                                                                  (:506)
//   P4 row    x += attention output; h = LayerNorm2(x); channel-mix lerp; ffn_x_prev <- h                    (:546-547)
//   P5 gemv   key projection, relu(.)^2 -> bf16 rows (no K split: the activation needs the whole sum)        (:548)
//   P6 gemv   value projection -> partials                                                                   (:548-549)
// and a final row phase (last residual add + model norm) and the head projection -> fp32 logits.  GEMV phases write fp32
// K-split partials [KS][32][N] that the consumer sums when it loads them, so no phase waits for a reduction.  A phase is a
// chain of load latencies, so every phase requests whatever does not depend on the previous phase (state rows, parameter
// vectors, up-projection rows) before it reads the activations, and sums partials with all loads of a round in flight.
//
// Two ways to run the phases (same bodies, bit-identical results, tests/test_decode_step_gpu.py):
//   persistent = 0  one launch per phase (7 L + 2), one kernel per phase, each sized to its item count.  Measured at configs[4]
//                   (0.4B, B = 32, tools/decode_phase_profile.py): row phases 3.1-3.6 us at best, GEMV phases 3.5-6.6 us, head
//                   phase 7.4-8.5 us (round 2: 13 us -- see head_phase), 1.05 ms per step in the replayed graph = 30.5 k
//                   tokens/s (module path: 4.0 ms, 8 k tokens/s).
//   persistent = 1  ONE launch of 256 resident workgroups that meet at a device-scope barrier between phases.  Measured:
//                   7.4 us per barrier -- 3.9 us for 256 arrivals + polling on one counter, 1.8 us for the agent-scope
//                   release (L2 write-back) and 1.6 us for the acquire (invalidate); the XCDs' L2s are not coherent with
//                   each other, so both are needed -- against ~1.5 us for a stream-ordered kernel boundary: 2.4 ms per step.
//                   Kept as an option (and as a cross-check of the phase bodies); the Python host uses persistent = 0.
//
// The phase bodies, the per-phase kernels and the workspace layout live in decode_step_phases.h, templated on the number of 32-row
// tiles RT: this file instantiates RT = 1 (and holds the lab build's persistent kernel); decode_step_wide.hip runs B = 33 .. 128
// through RT = 2, 3, 4.
#include "launchers.h"
#include "decode_step_phases.h"

namespace rwkv7 {

namespace {

#ifdef RWKV7_LAB   // the one-launch variant lost (2.4 ms against 0.93 ms per step): lab build only (python -m rwkvtts_amd.build --lab)
// mode 1: the step; mode 2 (debug): the barriers alone
template <int V>
__global__ __launch_bounds__(kDecThreads) void decode_persistent_kernel(DecodeDesc d, int mode) {
    using W = Variant<V>;
    __shared__ DecSmem<1> sm;
    unsigned target = 0;
    const int nphase = 7 * d.L + 2;
    for (int idx = 0; idx < nphase; idx++) {   // one call site per phase body
        const int l = idx / 7, ph = idx - 7 * l + (l == d.L ? 7 : 0);
        if (mode == 1) {
            const TblRow lp{d.tbl + (long)(l < d.L ? l : 0) * DP_COUNT};
            switch (ph) {
            case 0: run_phase<1, 0, W::NG, 0>(d, sm, l, lp); break;
            case 1: run_phase<1, 1, 0, 0>(d, sm, l, lp); break;
            case 2: run_phase<1, 2, W::NF1, W::NF2>(d, sm, l, lp); break;
            case 3: run_phase<1, 3, 0, 0>(d, sm, l, lp); break;
            case 4: run_phase<1, 4, W::NG, 0>(d, sm, l, lp); break;
            case 5: run_phase<1, 5, 16, 0>(d, sm, l, lp); break;
            case 6: run_phase<1, 6, 0, 0>(d, sm, l, lp); break;
            case 7: run_phase<1, 7, W::NG, 0>(d, sm, l, lp); break;
            default: run_phase<1, 8, 0, 0>(d, sm, l, lp); break;
            }
        }
        if (idx + 1 < nphase) grid_barrier(d.bar, target, gridDim.x, mode);
    }
}
#endif

}  // namespace

int decode_layer_ptrs() { return DP_COUNT; }

size_t decode_workspace_bytes(int B, int D, int H, int F, int V, int Rw, int Ra, int Rv, int Rg) {
    WsLayout w;
    if (!shape_ok<1>(B, D, H, F, V, Rw, Ra, Rv, Rg) || !ws_layout<1>(D, F, Rw, Ra, Rv, Rg, w)) return 0;
    return w.total;
}

int decode_step_bf16(int B, int D, int H, int L, int F, int V, int Rw, int Ra, int Rv, int Rg, float ln_eps, float gn_eps,
                     const void *const *layer_tbl, const void *const *layer_tbl_host, const void *x_in, const void *norm_w,
                     const void *norm_b, const void *head_w, const void *head_b, float *logits, void *workspace, int persistent,
                     hipStream_t st) {
    WsLayout w;
    if (!shape_ok<1>(B, D, H, F, V, Rw, Ra, Rv, Rg) || L < 1 || !ws_layout<1>(D, F, Rw, Ra, Rv, Rg, w)) return -4;  // RWKV7_ESHAPE
    const DecodeDesc d = make_desc({B, D, H, L, F, V, Rw, Ra, Rv, Rg, ln_eps, gn_eps, layer_tbl, x_in, norm_w, norm_b, head_w, head_b,
                                    logits, workspace}, w);
    (void)hipGetLastError();
#ifdef RWKV7_LAB
    if (persistent) {
        const int variant = pick_variant(D, Rw, Ra, Rv, Rg);
        int dev = 0, cus = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return (int)e;
        // every workgroup must be resident at once: one per CU (14 KB of LDS; 4 waves of <= 512 VGPRs fit any CU)
        const int grid = cus < kGrid ? cus : kGrid;
        e = hipMemsetAsync(d.bar, 0, 8, st);
        if (e != hipSuccess) return (int)e;
        if (variant == 0) decode_persistent_kernel<0><<<dim3(grid), dim3(kDecThreads), 0, st>>>(d, persistent);
        else if (variant == 1) decode_persistent_kernel<1><<<dim3(grid), dim3(kDecThreads), 0, st>>>(d, persistent);
        else decode_persistent_kernel<2><<<dim3(grid), dim3(kDecThreads), 0, st>>>(d, persistent);
    } else
#else
    if (persistent) return -4;   // RWKV7_ESHAPE: the persistent variant exists in the lab build only
#endif
        launch_step<1>(d, w, layer_tbl_host, st);
    return (int)hipGetLastError();
}

}  // namespace rwkv7
