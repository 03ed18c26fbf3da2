// rwkvtts_amd/csrc/wgrad_tn.hip -- weight gradients of the dense projections, bf16, gfx950.
//
// Reference arithmetic: autograd of nn.Linear (model/llm/rwkv_s2s_single_ffn.py:171-174, 195, 228-229): for y = x W^T the weight
// gradient is dW[N][K] = sum_t dy[t][N] x[t][K] with t over the B*T rows.  Both operands are token-major, so the contraction index is
// the ROW of both ("TN" for a BLAS); the library's kernels for that layout run at 0.86-1.04 PF/s where its NT kernels reach 1.2-1.45.
//
// Here, in the family of wgrad_mid_kernel (wgrad_skinny.hip): grid = (N / 256) x (K / 256) output tiles x S row slabs; a workgroup of
// four waves keeps its 256 x 256 fp32 tile in MFMA accumulators (wave = 128 dy columns x 128 x columns, 4 x 4 tiles of 32 x 32: 32
// transposing fragment reads per 32 MFMAs) and streams its [rows][256] pieces of dy and x as they are stored through LDS in 32-token
// steps.  Fragments come from the LDS transpose read (frag_tr); plane rows are 288 elements = 16 (mod 64) dwords apart, so the four
// token rows one transpose read touches fall into disjoint bank windows.  The planes are double-buffered (ONE barrier per step: the
// next step is written while this one is read) and registers hold kTnPF further steps in flight: a step is ~0.45 us of MFMA time,
// a load from HBM under load takes three times that.  Partials [S][N][K] fp32 are summed by rwkv7_sum_slabs_bf16 as before.
#include "launchers.h"
#include "chunk_common.h"
#include "launch_attr.h"

namespace rwkv7 {

namespace {
constexpr int kTnTile = 256;            // edge of the output tile: dy columns x x columns per workgroup
constexpr int kTnStep = 32;             // rows (tokens) per step
constexpr int kTnLd = kTnTile + 32;     // 288 elements = 144 dwords = 16 (mod 64)
constexpr int kTnPF = 4;                // steps in flight in registers (the loop body names four register sets)
constexpr int kTnPlane = kTnStep * kTnLd;                      // elements of one [32][288] plane
constexpr size_t kTnLds = 4 * kTnPlane * sizeof(uint16_t);     // dy and x planes, two buffers each: 72 KB

__global__ __launch_bounds__(256) void wgrad_tn_kernel(int N, int K, int rows_per_slab, const bf16_t *__restrict__ dy_, const bf16_t *__restrict__ x_,
                                                       float *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) uint16_t s_tn[];   // [buffer][dy plane, x plane]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
    const int ntk = K / kTnTile, tiles = (N / kTnTile) * ntk;
    // block id -> (slab, tile): ids b, b + 8, ... share an XCD (one L2); each XCD takes a run of consecutive (slab, tile) pairs, so the
    // workgroups that re-read the same dy / x rows sit behind the same L2
    int lin = blockIdx.x;
    if ((gridDim.x & 7) == 0) lin = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const int slab = lin / tiles, tile = lin - slab * tiles;
    const int n0 = (tile / ntk) * kTnTile, k0 = (tile % ntk) * kTnTile;
    const long row0 = (long)slab * rows_per_slab;
    const uint16_t *ga = reinterpret_cast<const uint16_t *>(dy_) + row0 * N + n0;
    const uint16_t *gb = reinterpret_cast<const uint16_t *>(x_) + row0 * K + k0;
    // per-thread pieces of a step: 32 x 32 chunks of 16 bytes per plane = 4 + 4 per thread; chunk tid + 256 i = row (tid >> 5) + 8 i
    const int crow = tid >> 5, ccol = (tid & 31) * 8;
    const int nsteps = rows_per_slab / kTnStep;
    struct Regs { uint4 a0, a1, a2, a3, b0, b1, b2, b3; };   // scalar fields (see wgrad_skinny_kernel)
    auto fetch = [&](int step) {
        Regs r;
        step = step < nsteps ? step : nsteps - 1;   // unconditional (clamped): the last steps are requested again and never read
        const uint16_t *a = ga + ((long)step * kTnStep + crow) * N + ccol, *b = gb + ((long)step * kTnStep + crow) * K + ccol;
        r.a0 = *reinterpret_cast<const uint4 *>(a);
        r.a1 = *reinterpret_cast<const uint4 *>(a + 8L * N);
        r.a2 = *reinterpret_cast<const uint4 *>(a + 16L * N);
        r.a3 = *reinterpret_cast<const uint4 *>(a + 24L * N);
        r.b0 = *reinterpret_cast<const uint4 *>(b);
        r.b1 = *reinterpret_cast<const uint4 *>(b + 8L * K);
        r.b2 = *reinterpret_cast<const uint4 *>(b + 16L * K);
        r.b3 = *reinterpret_cast<const uint4 *>(b + 24L * K);
        return r;
    };
    auto stage = [&](int buf, const Regs r) {
        uint16_t *sa = s_tn + buf * 2 * kTnPlane + crow * kTnLd + ccol, *sb = sa + kTnPlane;
        *reinterpret_cast<uint4 *>(sa) = r.a0;
        *reinterpret_cast<uint4 *>(sa + 8 * kTnLd) = r.a1;
        *reinterpret_cast<uint4 *>(sa + 16 * kTnLd) = r.a2;
        *reinterpret_cast<uint4 *>(sa + 24 * kTnLd) = r.a3;
        *reinterpret_cast<uint4 *>(sb) = r.b0;
        *reinterpret_cast<uint4 *>(sb + 8 * kTnLd) = r.b1;
        *reinterpret_cast<uint4 *>(sb + 16 * kTnLd) = r.b2;
        *reinterpret_cast<uint4 *>(sb + 24 * kTnLd) = r.b3;
    };
    f32x16 acc[4][4];   // [32 dy columns][32 x columns] tiles of the wave's 128 x 128
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = zero16();
    // every fragment of a 16-token k step is fetched once: 8 transposing reads (16 ds_read_b64_tr_b16) per 16 MFMAs
    struct Frags { bf16x8 a[4], b[4]; };
    auto read_frags = [&](Frags &F, int buf, int ks) {
        const uint16_t *sa = s_tn + buf * 2 * kTnPlane, *sb = sa + kTnPlane;
#pragma unroll
        for (int i = 0; i < 4; i++) F.a[i] = frag_tr(sa, kTnLd, 16 * ks, wm * 128 + i * 32, lane);
#pragma unroll
        for (int j = 0; j < 4; j++) F.b[j] = frag_tr(sb, kTnLd, 16 * ks, wn * 128 + j * 32, lane);
    };
    auto mfma16 = [&](const Frags &F) {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.a[i], F.b[j], acc[i][j], 0, 0, 0);   // m = dy column, n = x column
    };
    // four named register sets (see wgrad_skinny_kernel).  Step s is read from buffer s & 1 while step s + 1 (already in registers) is
    // written into the other one, which everybody left at the barrier that ended step s - 1.  The two 16-token halves of a step are
    // skewed across the barrier so that no fragment read is waited for with the matrix cores idle: the first half's fragments are read
    // right behind the barrier under the previous step's second-half MFMAs, the second half's (and the plane writes) under the first
    // half's MFMAs.  (First cut, reads and MFMAs of a step in program order: 250 us for the 4096 x 1024 class, every read exposed.)
    Regs r0 = fetch(0), r1 = fetch(1), r2 = fetch(2), r3 = fetch(3);
    stage(0, r0);
    r0 = fetch(kTnPF);
    lds_barrier();
    Frags F0, F1;
    read_frags(F0, 0, 0);
#define WGT_STEP(R_, U_)                                                                                                  \
    read_frags(F1, (U_) & 1, 1);                                                                                          \
    stage(((U_) + 1) & 1, R_);                                                                                            \
    mfma16(F0);                                                                                                           \
    _Pragma("unroll") for (int q = 0; q < 8; q++) {  /* MFMA, two fragment reads */                                       \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                                \
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                                                \
    }                                                                                                                     \
    _Pragma("unroll") for (int q = 0; q < 8; q++) {  /* MFMA, one plane write */                                          \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                                \
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                                                                \
    }                                                                                                                     \
    lds_barrier();                                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    R_ = fetch(step + (U_) + 1 + kTnPF);                                                                                  \
    read_frags(F0, ((U_) + 1) & 1, 0);                                                                                    \
    mfma16(F1);                                                                                                           \
    _Pragma("unroll") for (int q = 0; q < 8; q++) {  /* MFMA, a load, two fragment reads */                               \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                                \
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                                                \
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                                                \
    }                                                                                                                     \
    __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);                                                                    \
    __builtin_amdgcn_sched_barrier(0);
    for (int step = 0; step < nsteps; step += kTnPF) {   // nsteps is a multiple of kTnPF (entry check)
        WGT_STEP(r1, 0)
        WGT_STEP(r2, 1)
        WGT_STEP(r3, 2)
        WGT_STEP(r0, 3)
    }
#undef WGT_STEP
    // the tile leaves once: a store instruction writes two full 128-byte lines (32 consecutive floats per half wave)
    float *p = part + (long)slab * N * K;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int nb = n0 + wm * 128 + i * 32, kb = k0 + wn * 128 + j * 32;
#pragma unroll
            for (int r = 0; r < 16; r++) p[(long)(nb + d_row(r, lane)) * K + kb + (lane & 31)] = acc[i][j][r];
        }
}
}  // namespace

// part[s][N][K] (fp32) = dy[rows of slab s][N]^T x[rows of slab s][K]; N, K multiples of 256, rows per slab a multiple of 128
// (kTnPF steps of 32 rows)
int wgrad_tn_bf16(long M, int N, int K, int S, const void *dy, const void *x, float *part, hipStream_t st) {
    static DynLdsOnce lds_once;
    if (N % kTnTile || K % kTnTile || M % S || (M / S) % (kTnStep * kTnPF)) return -4;
    if (hipError_t e = lds_once.ensure(reinterpret_cast<const void *>(&wgrad_tn_kernel), (int)kTnLds); e != hipSuccess) return (int)e;
    (void)hipGetLastError();
    const int grid = (N / kTnTile) * (K / kTnTile) * S;
    wgrad_tn_kernel<<<dim3(grid), dim3(256), kTnLds, st>>>(N, K, (int)(M / S), (const bf16_t *)dy, (const bf16_t *)x, part);
    return (int)hipGetLastError();
}

}  // namespace rwkv7
