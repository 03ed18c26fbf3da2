// rwkvtts_amd/csrc/state_tune.hip -- state tuning (rwkvtts_amd/state_tune.py): the initial states of named voices are the ONLY trained
// tensors.  A voice's master state is fp32 -- per layer att_x_prev [V,D], att_kv [V,H,64,64], ffn_x_prev [V,D] -- with fp32 AdamW
// moments of the same shapes.  Two entries, both ONE launch for all layers and fields, every table a DEVICE table of 3 * layers
// pointers in the order of the cache_rows entries (att_x_prev, att_kv, ffn_x_prev):
//   expand  master rows -> the rows of the bf16 cache a training forward starts from: entry i writes master row voice[i] to row i
//           (att_kv: bits copied; the two shift rows: one round-to-nearest-even to bf16); voice[i] == -1 writes zeros and reads no
//           source, voice[i] < -1 skips the entry.
//   adamw   the optimizer step from the leaf gradients of that cache (fp32 [n,H,64,64] and bf16 [n,D]).  A device CSR groups the
//           batch rows by voice; per element g = grad_scale * (the rows' gradients added in fp32, one after the other in the listed
//           order), then the update rule of adamw_body.h with the bias corrections of THAT voice's step count, then the new state
//           goes to the voice's row of the serving cache (fp32 for att_kv, one RNE rounding for the shift rows).
// No atomics, no LDS: an element is owned by one thread, which walks its voice's rows itself, so a voice's result depends neither on
// the grid nor on the other voices of the launch nor on their order.  16-byte loads and stores throughout: a unit of work is 4 fp32
// elements of att_kv or 8 elements of a shift row (8 bf16 = one 16-byte vector of the gradient and of the cache row).
//
// No row (voice, batch row, store row) is range-checked: device data, the caller's guarantee (include/rwkv7_hip.h).
#include <hip/hip_runtime.h>

#include "../../include/rwkv7_hip.h"
#include "launchers.h"
#include "wkv7_common.h"

namespace rwkv7 {

constexpr int kTuneThreads = 256, kTuneVecs = 4;

__device__ __forceinline__ uint4 pack8_bf16(float4 a, float4 b) {
    return make_uint4((uint32_t)f2bf(a.x) | ((uint32_t)f2bf(a.y) << 16), (uint32_t)f2bf(a.z) | ((uint32_t)f2bf(a.w) << 16),
                      (uint32_t)f2bf(b.x) | ((uint32_t)f2bf(b.y) << 16), (uint32_t)f2bf(b.z) | ((uint32_t)f2bf(b.w) << 16));
}

// ---- expand.  A row of the three fields of one layer is one virtual array of 16-byte DESTINATION vectors, D/8 | 1024 H | D/8, as in
// cache_rows.hip; grid (piece of that array, entry, layer), kTuneVecs vectors per thread, all loads issued before the first store.
__global__ __launch_bounds__(kTuneThreads) void state_rows_expand_kernel(const float4 *const *__restrict__ master_tbl,
                                                                         uint4 *const *__restrict__ dst_tbl,
                                                                         const int *__restrict__ voice, int xv, int kvv) {
    const int e = blockIdx.y, l = blockIdx.z;
    const long vr = voice[e];
    if (vr < -1) return;   // uniform over the workgroup
    const bool zero = vr == -1;
    const float4 *const s0 = master_tbl[3 * l], *const s1 = master_tbl[3 * l + 1], *const s2 = master_tbl[3 * l + 2];
    uint4 *const d0 = dst_tbl[3 * l], *const d1 = dst_tbl[3 * l + 1], *const d2 = dst_tbl[3 * l + 2];
    const int nv = 2 * xv + kvv;
    const int base = blockIdx.x * (kTuneThreads * kTuneVecs) + threadIdx.x;
    uint4 v[kTuneVecs];
    uint4 *to[kTuneVecs];
#pragma unroll
    for (int j = 0; j < kTuneVecs; j++) {
        const int i = base + j * kTuneThreads;
        to[j] = nullptr;
        v[j] = make_uint4(0, 0, 0, 0);
        if (i < nv) {
            if (i >= xv && i < xv + kvv) {   // att_kv: fp32 -> fp32, the bits as they are
                const int c = i - xv;
                to[j] = d1 + (long)e * kvv + c;
                if (!zero) {
                    const float4 f = s1[vr * kvv + c];
                    v[j] = make_uint4(__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w));
                }
            } else {                          // a shift row: 8 fp32 of the master -> 8 bf16
                const bool att = i < xv;
                const int c = att ? i : i - xv - kvv;
                to[j] = (att ? d0 : d2) + (long)e * xv + c;
                if (!zero) {
                    const float4 *const from = (att ? s0 : s2) + (vr * xv + c) * 2;
                    v[j] = pack8_bf16(from[0], from[1]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kTuneVecs; j++)
        if (to[j]) *to[j] = v[j];
}

int state_rows_expand_f32(int layers, int n, const void *const *master_tbl, void *const *dst_tbl, const int *voice, int D, int H,
                          hipStream_t st) {
    (void)hipGetLastError();
    const int xv = D / 8, kvv = H * 1024, nv = 2 * xv + kvv;
    const int per = kTuneThreads * kTuneVecs;
    const dim3 grid((nv + per - 1) / per, n, layers), block(kTuneThreads);
    hipLaunchKernelGGL(state_rows_expand_kernel, grid, block, 0, st, (const float4 *const *)master_tbl, (uint4 *const *)dst_tbl, voice, xv,
                       kvv);
    return (int)hipGetLastError();
}

// ---- step
struct TuneHyper {
    float lr, beta1, beta2, eps, wd, grad_scale;
};

// beta^t in double by repeated squaring (t >= 1): the bias corrections 1 - beta^t of a voice's own step count, which is device data
__device__ __forceinline__ double powi(double b, int t) {
    double r = 1.0;
    for (; t > 0; t >>= 1, b *= b)
        if (t & 1) r *= b;
    return r;
}

// The update rule of adamw_body.h (torch.optim.AdamW, decoupled decay), statement for statement.
struct TuneRule {
    float decay, step, beta1, beta2, eps, inv_sqrt_bc2;
    __device__ __forceinline__ void operator()(float &pp, float &m1, float &v1, float gg) const {
        pp *= decay;
        m1 = fmaf(beta1, m1, (1.f - beta1) * gg);
        v1 = fmaf(beta2, v1, (1.f - beta2) * gg * gg);
        pp -= step * m1 / (sqrtf(v1) * inv_sqrt_bc2 + eps);
    }
    __device__ __forceinline__ void operator()(float4 &p, float4 &m, float4 &v, float4 g) const {
        (*this)(p.x, m.x, v.x, g.x); (*this)(p.y, m.y, v.y, g.y); (*this)(p.z, m.z, v.z, g.z); (*this)(p.w, m.w, v.w, g.w);
    }
};

__device__ __forceinline__ void add4(float4 &a, float4 g) { a.x += g.x; a.y += g.y; a.z += g.z; a.w += g.w; }
__device__ __forceinline__ float4 scale_or_zero(float4 a, float s, bool skip) {
    return skip ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(a.x * s, a.y * s, a.z * s, a.w * s);
}

// Grid (tile of the row, field 3 l + f, active voice).  A shift row has D/8 units of 8 elements, att_kv 1024 H units of 4: the
// workgroups of a shift field beyond its few tiles leave at once.  A NULL gradient pointer: the field is not tuned, nothing is touched.
__global__ __launch_bounds__(kTuneThreads) void state_rows_adamw_kernel(const void *const *__restrict__ grad_tbl,
                                                                        float4 *const *__restrict__ master_tbl,
                                                                        float4 *const *__restrict__ m_tbl, float4 *const *__restrict__ v_tbl,
                                                                        void *const *__restrict__ store_tbl,
                                                                        const int *__restrict__ seg_start, const int *__restrict__ seg_rows,
                                                                        const int *__restrict__ seg_info,
                                                                        const float *__restrict__ skip_flag, TuneHyper hp, int xv, int kvv) {
    const int fl = blockIdx.y, a = blockIdx.z;
    const bool kv = fl % 3 == 1;
    const int units = kv ? kvv : xv;
    const int base = (int)blockIdx.x * (kTuneThreads * kTuneVecs) + (int)threadIdx.x;
    if ((int)blockIdx.x * (kTuneThreads * kTuneVecs) >= units) return;   // uniform
    const void *const grad = grad_tbl[fl];
    if (!grad) return;                                              // uniform
    const long vr = seg_info[3 * a], sr = seg_info[3 * a + 1];
    const int t = seg_info[3 * a + 2], r0 = seg_start[a], r1 = seg_start[a + 1];
    const bool skip = skip_flag && *skip_flag != 0.f;
    const double bc1 = 1.0 - powi((double)hp.beta1, t), bc2 = 1.0 - powi((double)hp.beta2, t);
    const TuneRule rule{1.f - hp.lr * hp.wd, hp.lr * (float)(1.0 / bc1), hp.beta1, hp.beta2, hp.eps, (float)(1.0 / sqrt(bc2))};
    if (kv) {
        float4 *const p = master_tbl[fl] + vr * kvv, *const m = m_tbl[fl] + vr * kvv, *const v = v_tbl[fl] + vr * kvv;
        float4 *const out = sr >= 0 ? (float4 *)store_tbl[fl] + sr * kvv : nullptr;
        const float4 *const g4 = (const float4 *)grad;
        float4 pp[kTuneVecs], mm[kTuneVecs], vv[kTuneVecs], acc[kTuneVecs];
#pragma unroll
        for (int j = 0; j < kTuneVecs; j++) {
            const int i = base + j * kTuneThreads;
            acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < units) pp[j] = p[i], mm[j] = m[i], vv[j] = v[i];
        }
        for (int r = r0; r < r1; r++) {
            const float4 *const row = g4 + (long)seg_rows[r] * kvv;
#pragma unroll
            for (int j = 0; j < kTuneVecs; j++) {
                const int i = base + j * kTuneThreads;
                if (i < units) add4(acc[j], row[i]);
            }
        }
#pragma unroll
        for (int j = 0; j < kTuneVecs; j++) {
            const int i = base + j * kTuneThreads;
            if (i < units) {
                rule(pp[j], mm[j], vv[j], scale_or_zero(acc[j], hp.grad_scale, skip));
                p[i] = pp[j], m[i] = mm[j], v[i] = vv[j];
                if (out) out[i] = pp[j];
            }
        }
    } else {
        // 8 elements per unit: two float4 of master and moments, one 16-byte vector of the bf16 gradient and of the cache row
        float4 *const p = master_tbl[fl] + vr * xv * 2, *const m = m_tbl[fl] + vr * xv * 2, *const v = v_tbl[fl] + vr * xv * 2;
        uint4 *const out = sr >= 0 ? (uint4 *)store_tbl[fl] + sr * xv : nullptr;
        const uint4 *const g8 = (const uint4 *)grad;
        // D <= 4096: at most 512 units, fewer than one tile -- this is workgroup 0 of the field, two trips at the most
        for (int u = threadIdx.x; u < units; u += kTuneThreads) {
            float4 p0 = p[2 * u], p1 = p[2 * u + 1], m0 = m[2 * u], m1 = m[2 * u + 1], v0 = v[2 * u], v1 = v[2 * u + 1];
            float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
            for (int r = r0; r < r1; r++) {
                const uint4 g = g8[(long)seg_rows[r] * xv + u];
                add4(a0, make_float4(__uint_as_float(g.x << 16), __uint_as_float(g.x & 0xffff0000u), __uint_as_float(g.y << 16),
                                     __uint_as_float(g.y & 0xffff0000u)));
                add4(a1, make_float4(__uint_as_float(g.z << 16), __uint_as_float(g.z & 0xffff0000u), __uint_as_float(g.w << 16),
                                     __uint_as_float(g.w & 0xffff0000u)));
            }
            rule(p0, m0, v0, scale_or_zero(a0, hp.grad_scale, skip));
            rule(p1, m1, v1, scale_or_zero(a1, hp.grad_scale, skip));
            p[2 * u] = p0, p[2 * u + 1] = p1, m[2 * u] = m0, m[2 * u + 1] = m1, v[2 * u] = v0, v[2 * u + 1] = v1;
            if (out) out[u] = pack8_bf16(p0, p1);
        }
    }
}

int state_rows_adamw_f32(int layers, int A, const void *const *grad_tbl, void *const *master_tbl, void *const *m_tbl, void *const *v_tbl,
                         void *const *store_tbl, const int *seg_start, const int *seg_rows, const int *seg_info, const float *skip_flag,
                         float lr, float beta1, float beta2, float eps, float wd, float grad_scale, int D, int H, hipStream_t st) {
    (void)hipGetLastError();
    const int xv = D / 8, kvv = H * 1024;
    const int per = kTuneThreads * kTuneVecs;
    const dim3 grid((kvv + per - 1) / per, 3 * layers, A), block(kTuneThreads);
    hipLaunchKernelGGL(state_rows_adamw_kernel, grid, block, 0, st, grad_tbl, (float4 *const *)master_tbl, (float4 *const *)m_tbl,
                       (float4 *const *)v_tbl, store_tbl, seg_start, seg_rows, seg_info, skip_flag,
                       TuneHyper{lr, beta1, beta2, eps, wd, grad_scale}, xv, kvv);
    return (int)hipGetLastError();
}

}  // namespace rwkv7
