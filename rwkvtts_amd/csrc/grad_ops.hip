// rwkvtts_amd/csrc/grad_ops.hip -- passes over the trainer's flat bf16 gradient buffer (rwkvtts_amd/trainer.py):
//   * the sum of squares behind gradient clipping by global norm (the reference hands `gradient_clipping` to DeepSpeed,
//     train_scripts/train_rwkv_tts.py:133,405; third_party/cosyvoice/utils/train_utils.py:283-291 calls clip_grad_norm_),
//   * fp32 accumulation of micro-batch gradients and the fold of the sum into the bf16 buffer (`accum_grad` /
//     `gradient_accumulation_steps`, train_utils.py:87-89; DeepSpeed's bf16 engine accumulates in fp32),
//   * AdamW with the clip factor taken from device memory.
// Bytes per element: 2 for the norm, 6 for the first accumulate of a window (10 for the later ones, which also read the
// fp32 sum), 8 for the fold, against AdamW's 28.
#include "launchers.h"
#include "adamw_body.h"

namespace rwkv7 {

constexpr int kSumsqTile = 8192;   // elements per workgroup of stage 1: FIXED, so the partials do not depend on the grid

__device__ __forceinline__ void sq8(float &s, const uint4 &r) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float lo = __uint_as_float(w[k] << 16), hi = __uint_as_float(w[k] & 0xffff0000u);
        s = fmaf(lo, lo, s);
        s = fmaf(hi, hi, s);
    }
}

// Stage 1: workgroup b sums the squares of elements [b * 8192, min(n, (b + 1) * 8192)).  Thread t takes the 16-byte pieces
// t, t + 256, t + 512, t + 768 of the tile (a wave reads 1 KiB contiguous per load), all four loads in flight before the
// first multiply; 32 sequential fp32 adds per thread, 6 levels across the wave, 2 across the 4 waves.  n % 8 == 0, so a
// piece is inside the buffer or outside it as a whole; pieces outside count as zeros.
__global__ __launch_bounds__(256) void grad_sumsq_tiles_kernel(long n, const bf16_t *__restrict__ g16, float *__restrict__ partials) {
    __shared__ float sh[4];
    const long base = (long)blockIdx.x * kSumsqTile;
    uint4 r[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const long e = base + (long)(j * 256 + (int)threadIdx.x) * 8;
        r[j] = e < n ? *reinterpret_cast<const uint4 *>(g16 + e) : make_uint4(0u, 0u, 0u, 0u);
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) sq8(s, r[j]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// Stage 2, one workgroup: thread t adds partials t, t + 256, ... in double, then a fixed tree over the 256 threads.  A
// double holds the sum of 2^29 fp32 values exactly enough that the order would not show in the fp32 result; the order is
// fixed all the same.
__global__ __launch_bounds__(256) void grad_sumsq_final_kernel(long ntiles, const float *__restrict__ partials, float *__restrict__ out,
                                                               int accumulate) {
    __shared__ double sh[256];
    double s = 0.0;
    for (long i = threadIdx.x; i < ntiles; i += 256) s += (double)partials[i];
    sh[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float tot = (float)sh[0];
        out[0] = accumulate ? out[0] + tot : tot;
    }
}

int grad_sumsq_bf16(long n, const void *g16, float *partials, float *out, int accumulate, hipStream_t st) {
    (void)hipGetLastError();
    const long ntiles = (n + kSumsqTile - 1) / kSumsqTile;
    hipLaunchKernelGGL(grad_sumsq_tiles_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, n, (const bf16_t *)g16, partials);
    hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(256), 0, st, ntiles, (const float *)partials, out, accumulate);
    return (int)hipGetLastError();
}

// acc32 = (first ? 0 : acc32) + float(g16): 8 elements per thread and iteration (one 16-byte bf16 load, two 16-byte fp32
// loads and stores), 2 + 4 bytes read (2 when first) and 4 written per element.  One exact fp32 add per element.
template <bool FIRST>
__global__ __launch_bounds__(256) void grad_accum_kernel(long n8, float *__restrict__ acc32, const bf16_t *__restrict__ g16) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        const uint4 r = *reinterpret_cast<const uint4 *>(g16 + 8 * i);
        float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
        if (!FIRST) {
            a0 = reinterpret_cast<const float4 *>(acc32)[2 * i];
            a1 = reinterpret_cast<const float4 *>(acc32)[2 * i + 1];
        }
        a0.x += __uint_as_float(r.x << 16); a0.y += __uint_as_float(r.x & 0xffff0000u);
        a0.z += __uint_as_float(r.y << 16); a0.w += __uint_as_float(r.y & 0xffff0000u);
        a1.x += __uint_as_float(r.z << 16); a1.y += __uint_as_float(r.z & 0xffff0000u);
        a1.z += __uint_as_float(r.w << 16); a1.w += __uint_as_float(r.w & 0xffff0000u);
        reinterpret_cast<float4 *>(acc32)[2 * i] = a0;
        reinterpret_cast<float4 *>(acc32)[2 * i + 1] = a1;
    }
}

// g16 = bf16_rne((acc32 + float(g16)) * inv_count) in place: the last micro-batch's gradient never visits the fp32 buffer,
// and the only rounding to bf16 is the one at the end.  4 + 2 bytes read, 2 written per element.
__global__ __launch_bounds__(256) void grad_fold_kernel(long n8, const float *__restrict__ acc32, bf16_t *__restrict__ g16, float inv_count) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        const uint4 r = *reinterpret_cast<const uint4 *>(g16 + 8 * i);
        const float4 a0 = reinterpret_cast<const float4 *>(acc32)[2 * i], a1 = reinterpret_cast<const float4 *>(acc32)[2 * i + 1];
        auto pair = [&](float a_lo, float a_hi, uint32_t w) {   // two bf16 in one word: low half first
            const float lo = (a_lo + __uint_as_float(w << 16)) * inv_count, hi = (a_hi + __uint_as_float(w & 0xffff0000u)) * inv_count;
            return (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
        };
        uint4 o;
        o.x = pair(a0.x, a0.y, r.x);
        o.y = pair(a0.z, a0.w, r.y);
        o.z = pair(a1.x, a1.y, r.z);
        o.w = pair(a1.z, a1.w, r.w);
        *reinterpret_cast<uint4 *>(g16 + 8 * i) = o;
    }
}

static int stream_grid(long n8) { return (int)((n8 + 255) / 256 < 16384 ? (n8 + 255) / 256 : 16384); }

int grad_accum_bf16(long n, float *acc32, const void *g16, int first, hipStream_t st) {
    (void)hipGetLastError();
    const long n8 = n / 8;
    if (first)
        hipLaunchKernelGGL(grad_accum_kernel<true>, dim3(stream_grid(n8)), dim3(256), 0, st, n8, acc32, (const bf16_t *)g16);
    else
        hipLaunchKernelGGL(grad_accum_kernel<false>, dim3(stream_grid(n8)), dim3(256), 0, st, n8, acc32, (const bf16_t *)g16);
    return (int)hipGetLastError();
}

int grad_fold_bf16(long n, const float *acc32, void *g16, float inv_count, hipStream_t st) {
    (void)hipGetLastError();
    const long n8 = n / 8;
    hipLaunchKernelGGL(grad_fold_kernel, dim3(stream_grid(n8)), dim3(256), 0, st, n8, acc32, (bf16_t *)g16, inv_count);
    return (int)hipGetLastError();
}

// AdamW with the clip factor of torch.nn.utils.clip_grad_norm_ computed per launch from the device scalar *sumsq:
// coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)).  A non-finite sumsq (a NaN or Inf anywhere in the gradient) acts like
// skip_flag != 0: the step runs on a zero gradient.  The host never reads either value.
template <bool GROUPS>
__global__ __launch_bounds__(256) void adamw_clip_kernel(long n4, float *__restrict__ p32, const bf16_t *__restrict__ g16,
                                                         float *__restrict__ m, float *__restrict__ v, bf16_t *__restrict__ p16,
                                                         const uint8_t *__restrict__ slab_group, const float2 *__restrict__ group_tab,
                                                         const float *__restrict__ skip_flag, const float *__restrict__ sumsq,
                                                         float max_norm, float lr, float beta1, float beta2, float eps, float wd,
                                                         float inv_bc1, float inv_sqrt_bc2) {
    const float ss = *sumsq;
    const bool finite = (__float_as_uint(ss) & 0x7f800000u) != 0x7f800000u;
    const bool skip = (skip_flag != nullptr && *skip_flag != 0.f) || !finite;
    const float coef = finite ? fminf(1.f, max_norm / (sqrtf(ss) + 1e-6f)) : 1.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
        adamw_body<GROUPS, true>(i, p32, g16, m, v, p16, slab_group, group_tab, skip, coef, lr, beta1, beta2, eps, wd, inv_bc1,
                             inv_sqrt_bc2);
}

int adamw_clip_step(long n, float *p32, const void *g16, float *m, float *v, void *p16, const uint8_t *slab_group,
                    const float *group_tab, const float *skip_flag, const float *sumsq, float max_norm, float lr, float beta1,
                    float beta2, float eps, float wd, float inv_bc1, float inv_sqrt_bc2, hipStream_t st) {
    (void)hipGetLastError();
    const long n4 = n / 4;
    const int grid = (int)((n4 + 255) / 256 < 16384 ? (n4 + 255) / 256 : 16384);
    if (slab_group)
        hipLaunchKernelGGL(adamw_clip_kernel<true>, dim3(grid), dim3(256), 0, st, n4, p32, (const bf16_t *)g16, m, v, (bf16_t *)p16,
                           slab_group, reinterpret_cast<const float2 *>(group_tab), skip_flag, sumsq, max_norm, lr, beta1, beta2, eps,
                           wd, inv_bc1, inv_sqrt_bc2);
    else
        hipLaunchKernelGGL(adamw_clip_kernel<false>, dim3(grid), dim3(256), 0, st, n4, p32, (const bf16_t *)g16, m, v, (bf16_t *)p16,
                           slab_group, reinterpret_cast<const float2 *>(group_tab), skip_flag, sumsq, max_norm, lr, beta1, beta2, eps,
                           wd, inv_bc1, inv_sqrt_bc2);
    return (int)hipGetLastError();
}

}  // namespace rwkv7
