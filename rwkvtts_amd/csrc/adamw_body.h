// rwkvtts_amd/csrc/adamw_body.h -- the loop body of the AdamW kernels, shared by adamw_kernel (elementwise.hip) and
// adamw_clip_kernel (grad_ops.hip) so that the update rule exists once.
#pragma once
#include "wkv7_common.h"

namespace rwkv7 {

// Update rule = torch.optim.AdamW (decoupled weight decay):
//   p *= 1 - lr wd ;  m = b1 m + (1-b1) g ;  v = b2 v + (1-b2) g^2 ;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
// 4 floats per thread and iteration: 2 + 3*4 bytes read, 3*4 + 2 written per parameter (28 B) -- nothing else touches HBM.
// GROUPS: slab_group[e / 128] indexes group_tab[g] = {lr scale, weight decay}.  skip: the step runs on a ZERO gradient.
// CLIP: the gradient is scaled by coef (<= 1, uniform over the launch) right after the load, and only when coef < 1; with
// CLIP false, or coef == 1, the statements executed are those of the plain kernel.  One call = one float4 (index i) of the
// kernel's grid-stride loop; the loop itself stays in the kernel.
template <bool GROUPS, bool CLIP>
__device__ __forceinline__ void adamw_body(long i, float *__restrict__ p32, const bf16_t *__restrict__ g16, float *__restrict__ m,
                                           float *__restrict__ v, bf16_t *__restrict__ p16, const uint8_t *__restrict__ slab_group,
                                           const float2 *__restrict__ group_tab, bool skip, float coef, float lr, float beta1,
                                           float beta2, float eps, float wd, float inv_bc1, float inv_sqrt_bc2) {
    {
        float lr_i = lr, wd_i = wd;
        if (GROUPS) {
            const float2 g = group_tab[slab_group[i >> 5]];
            lr_i = lr * g.x;
            wd_i = g.y;
        }
        const float decay = 1.f - lr_i * wd_i, step = lr_i * inv_bc1;
        float4 p = reinterpret_cast<float4 *>(p32)[i], mm = reinterpret_cast<float4 *>(m)[i], vv = reinterpret_cast<float4 *>(v)[i];
        float4 g = cvt4(ld4<bf16_t>(g16 + 4 * i, true));
        if (CLIP && coef < 1.f) g = make_float4(g.x * coef, g.y * coef, g.z * coef, g.w * coef);
        if (skip) g = make_float4(0.f, 0.f, 0.f, 0.f);
        auto upd = [&](float &pp, float &m1, float &v1, float gg) {
            pp *= decay;
            m1 = fmaf(beta1, m1, (1.f - beta1) * gg);
            v1 = fmaf(beta2, v1, (1.f - beta2) * gg * gg);
            pp -= step * m1 / (sqrtf(v1) * inv_sqrt_bc2 + eps);
        };
        upd(p.x, mm.x, vv.x, g.x); upd(p.y, mm.y, vv.y, g.y); upd(p.z, mm.z, vv.z, g.z); upd(p.w, mm.w, vv.w, g.w);
        reinterpret_cast<float4 *>(p32)[i] = p;
        reinterpret_cast<float4 *>(m)[i] = mm;
        reinterpret_cast<float4 *>(v)[i] = vv;
        st4(p16 + 4 * i, p);
    }
}

}  // namespace rwkv7
