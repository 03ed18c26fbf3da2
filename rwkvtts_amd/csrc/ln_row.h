// rwkvtts_amd/csrc/ln_row.h -- what the row-stream kernels that LayerNorm a row share (elementwise.hip, prefill_rows.hip): 8-channel
// vector I/O, the workgroup sums with a pinned summation order, and the residual add + LayerNorm of one row (add_ln_row), so that
// every kernel built on it gives the same bits for the same row; and, on the host, the one launch shape they all have.
#pragma once
#include <type_traits>

#include "../../include/rwkv7_hip.h"
#include "wkv7_common.h"

namespace rwkv7 {

// One thread per 8 columns of a row: D <= 4096.  Declaring the bound lets the register allocator use 256 VGPRs
// (the default assumes 1024-thread blocks = 128 VGPRs, which made mix_bwd<6> spill 392 bytes of scratch per lane
// and serialised its loads: 1.1 TB/s).
constexpr int kEwMaxThreads = 512;

// two fp32 -> packed bf16 pair (low half = a), round-to-nearest-even in ONE v_cvt_pk_bf16_f32 (gfx950) instead of the ~14 integer
// instructions of two f2bf(): the row-stream kernels below round 8-24 values per thread and row
typedef __bf16 pkbf2_t __attribute__((ext_vector_type(2)));
typedef float pkf2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
    const pkf2_t v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, pkbf2_t));
}

template <typename T>
struct V8;
template <>
struct V8<bf16_t> {
    static __device__ __forceinline__ void ld(const bf16_t *p, float (&f)[8]) {
        const uint4 r = *reinterpret_cast<const uint4 *>(p);
        f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
        f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
        f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
        f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
    }
    static __device__ __forceinline__ void st(bf16_t *p, const float (&f)[8]) {
        uint4 r;
        r.x = pk_bf16(f[0], f[1]);
        r.y = pk_bf16(f[2], f[3]);
        r.z = pk_bf16(f[4], f[5]);
        r.w = pk_bf16(f[6], f[7]);
        *reinterpret_cast<uint4 *>(p) = r;
    }
    static __device__ __forceinline__ float ld1(const bf16_t *p) { return bf2f(p->x); }
};
template <>
struct V8<float> {
    static __device__ __forceinline__ void ld(const float *p, float (&f)[8]) {
        const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    }
    static __device__ __forceinline__ void st(float *p, const float (&f)[8]) {
        *reinterpret_cast<float4 *>(p) = make_float4(f[0], f[1], f[2], f[3]);
        *reinterpret_cast<float4 *>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
    }
    static __device__ __forceinline__ float ld1(const float *p) { return *p; }
};

// the 16 (bf16) / 32 (fp32) bytes of 8 consecutive channels as they come from memory: loaded early, converted at the use
template <typename T>
struct Raw8;
template <>
struct Raw8<bf16_t> {
    uint4 r;
    __device__ __forceinline__ void load(const bf16_t *p) { r = *reinterpret_cast<const uint4 *>(p); }
    __device__ __forceinline__ void get(float (&f)[8]) const {
        f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
        f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
        f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
        f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
    }
};
template <>
struct Raw8<float> {
    float4 a, b;
    __device__ __forceinline__ void load(const float *p) {
        a = *reinterpret_cast<const float4 *>(p);
        b = *reinterpret_cast<const float4 *>(p + 4);
    }
    __device__ __forceinline__ void get(float (&f)[8]) const {
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    }
};

template <typename T>
__device__ __forceinline__ float round_to(float v);
template <>
__device__ __forceinline__ float round_to<bf16_t>(float v) { return __uint_as_float(pk_bf16(v, v) & 0xffff0000u); }
template <>
__device__ __forceinline__ float round_to<float>(float v) { return v; }

// a + b that -ffast-math cannot reassociate: the LayerNorm sums of the one-pass kernels and of the separate stages must come out
// bit for bit the same (tests/test_fused_gpu.py compares the two routes with torch.equal), whatever shape the compiler gives each loop
__device__ __forceinline__ float add_pinned(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// red[0 .. ngroups) summed in index order (slots past ngroups hold zeros, red_init: whole float4 groups are read)
__device__ __forceinline__ float sum_slots(const float *red, int ngroups) {
    float t = 0.f;
    for (int i = 0; i < ngroups; i += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(red + i);
        t = add_pinned(add_pinned(add_pinned(add_pinned(t, v.x), v.y), v.z), v.w);
    }
    return t;
}
// every reduction slot zero before the first block_sum / block_sum2 (they read whole float4 groups)
template <int ROWS>
__device__ __forceinline__ void red_init(float (*red)[kEwMaxThreads / 8]) {   // red[ROWS][kEwMaxThreads / 8]
    for (int i = threadIdx.x; i < ROWS * (kEwMaxThreads / 8); i += blockDim.x) (&red[0][0])[i] = 0.f;
    __syncthreads();
}

// two sums over the D/8 threads of the workgroup with ONE barrier; slots alternate (ph = 0 / 2) between consecutive calls so that
// a fast wave cannot overwrite a slot a slow wave is still reading
__device__ __forceinline__ void block_sum2(float &a, float &b, float (*red)[kEwMaxThreads / 8], int ph, int ngroups) {
    a = sum8(a);
    b = sum8(b);
    if ((threadIdx.x & 7) == 0) {
        red[ph][threadIdx.x >> 3] = a;
        red[ph + 1][threadIdx.x >> 3] = b;
    }
    __syncthreads();
    const float ta = sum_slots(red[ph], ngroups), tb = sum_slots(red[ph + 1], ngroups);
    a = ta;
    b = tb;
}

// what one row of add_ln_row needs from memory, loaded early (a row ahead) and converted at the use
template <typename T>
struct RowPre {
    Raw8<T> xv, bv;
    float m;
};

// One row of residual add + LayerNorm, thread = 8 channels from c, all D/8 threads of the workgroup together (two barriers: the mean,
// then the centred squares, as add_ln_fwd_kernel): x1 = x + branch rounded to T (has_branch; stored to x_out at element offset o
// when `write`), h = LN(x1) gamma + beta rounded to T (stored to h_out when `write` and h_out), hm = h * mask.  mu / rs: the row's
// statistics.  red: four zeroed reduction rows (red_init<4>), ph: the slot phase, advanced here.
template <typename T>
__device__ __forceinline__ void add_ln_row(const RowPre<T> &f, long o, bool has_branch, bool has_mask, bool write, T *x_out, T *h_out,
                                           const float (&gm)[8], const float (&bt)[8], float inv_d, float eps, int ng,
                                           float (*red)[kEwMaxThreads / 8], int &ph, float &mu, float &rs, float (&hm)[8]) {
    float v[8];
    f.xv.get(v);
    if (has_branch) {
        float b[8];
        f.bv.get(b);
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = round_to<T>(v[j] + b[j]);
        if (write) V8<T>::st(x_out + o, v);
    }
    float s = 0.f, dummy = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) s += v[j];
    block_sum2(s, dummy, red, ph, ng);
    ph ^= 2;
    mu = s * inv_d;
    float q = 0.f;
    dummy = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        v[j] -= mu;
        q = fmaf(v[j], v[j], q);
    }
    block_sum2(q, dummy, red, ph, ng);
    ph ^= 2;
    rs = rsqrtf(q * inv_d + eps);
    const float m = has_mask ? f.m : 1.f;
#pragma unroll
    for (int j = 0; j < 8; j++) hm[j] = round_to<T>(fmaf(v[j] * rs, gm[j], bt[j]));
    if (write && h_out) V8<T>::st(h_out + o, hm);
#pragma unroll
    for (int j = 0; j < 8; j++) hm[j] *= m;
}

// ---- host side: how every row-stream kernel is launched ---------------------------------------------------------------------------
// a row of D channels on D/8 threads, whole heads (64 channels) only
inline bool row_width_ok(int D) { return D > 0 && D % 64 == 0 && D <= kEwMaxThreads * 8; }

// nblocks workgroups of D/8 threads; returns the launch's error
template <typename... P, typename... A>
int launch_rows(void (*kernel)(P...), int nblocks, int D, hipStream_t st, A... args) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(D / 8), 0, st, args...);
    return (int)hipGetLastError();
}

// launch(std::integral_constant<int, N>) for the N of NS... that equals nmix: NS is the list of lerp counts a stage instantiates its
// kernel for, and an nmix outside it is RWKV7_ESHAPE
template <int... NS, typename F>
int for_nmix(int nmix, F launch) {
    int rc = RWKV7_ESHAPE;
    (void)((nmix == NS && ((rc = launch(std::integral_constant<int, NS>{})), true)) || ...);
    return rc;
}

}  // namespace rwkv7
