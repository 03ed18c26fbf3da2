// rwkvtts_amd/csrc/decode_step_wide.hip -- the decode step of decode_step.hip for B = 33 .. 128 sequences: RT = 2, 3 or 4 row tiles
// of 32, one launch per phase, every weight streamed ONCE per step.
//
// The 32-row step is a chain of ~170 launch-latency-bound kernels; a GEMV item pays one launch and one weight-fetch latency whatever
// the batch.  Here an item is still (32-column weight tile, K split), each wave loads its weight fragments once per k-step and issues
// one MFMA per row tile against that tile's activation rows, into RT accumulators (decode_step_phases.h: gemv_steps): the reuse is
// in registers, not in a cache.  The row phases and the head phase scale by grid (B workgroups; H ceil(B / 2) items), and every
// scratch plane's row stride is the padded capacity 32 RT.
//
// Bit-identity with the 32-row kernel (tests/test_decode_wide_gpu.py): a row's values depend on its own MFMA column only, and the K
// split (pick_ks does not see B), the head phase's pairing (2p, 2p + 1) and every summation order are the one-tile kernel's, so
// rows 32 g .. 32 g + 31 get exactly what rwkv7_decode_step_bf16 gives a batch of those rows.
//
// Rounds of loads: 8 k-steps in flight (one tile: 16).  Registers / LDS per instantiation: DESIGN.md 7.2.  There is no persistent
// variant.
#include "launchers.h"
#include "decode_step_phases.h"

namespace rwkv7 {

namespace {

template <int RT>
size_t wide_bytes(int B, int D, int H, int F, int V, int Rw, int Ra, int Rv, int Rg) {
    WsLayout w;
    if (!shape_ok<RT>(B, D, H, F, V, Rw, Ra, Rv, Rg) || !ws_layout<RT>(D, F, Rw, Ra, Rv, Rg, w)) return 0;
    return w.total;
}

template <int RT>
int wide_step(const StepArgs &a, const void *const *layer_tbl_host, hipStream_t st) {
    WsLayout w;
    if (!shape_ok<RT>(a.B, a.D, a.H, a.F, a.V, a.Rw, a.Ra, a.Rv, a.Rg) || a.L < 1 || !ws_layout<RT>(a.D, a.F, a.Rw, a.Ra, a.Rv, a.Rg, w))
        return -4;  // RWKV7_ESHAPE
    const DecodeDesc d = make_desc(a, w);
    (void)hipGetLastError();
    launch_step<RT>(d, w, layer_tbl_host, st);
    return (int)hipGetLastError();
}

}  // namespace

size_t decode_wide_workspace_bytes(int B, int D, int H, int F, int V, int Rw, int Ra, int Rv, int Rg) {
    if (B <= 32 || B > 128) return 0;
    const int rt = (B + 31) / 32;
    return rt == 2 ? wide_bytes<2>(B, D, H, F, V, Rw, Ra, Rv, Rg)
                   : rt == 3 ? wide_bytes<3>(B, D, H, F, V, Rw, Ra, Rv, Rg) : wide_bytes<4>(B, D, H, F, V, Rw, Ra, Rv, Rg);
}

int decode_step_wide_bf16(int B, int D, int H, int L, int F, int V, int Rw, int Ra, int Rv, int Rg, float ln_eps, float gn_eps,
                          const void *const *layer_tbl, const void *const *layer_tbl_host, const void *x_in, const void *norm_w,
                          const void *norm_b, const void *head_w, const void *head_b, float *logits, void *workspace, hipStream_t st) {
    if (B <= 32 || B > 128) return -4;  // RWKV7_ESHAPE
    const StepArgs a{B, D, H, L, F, V, Rw, Ra, Rv, Rg, ln_eps, gn_eps, layer_tbl, x_in, norm_w, norm_b, head_w, head_b, logits, workspace};
    const int rt = (B + 31) / 32;
    return rt == 2 ? wide_step<2>(a, layer_tbl_host, st) : rt == 3 ? wide_step<3>(a, layer_tbl_host, st) : wide_step<4>(a, layer_tbl_host, st);
}

}  // namespace rwkv7
