// rwkvtts_amd/csrc/head_eval.hip -- forward-only head metrics of one chunk of bf16 head logits [rows, ld] (held-out evaluation:
// losses.fused_linear_eval, the heads' eval_metrics, DataParallelTrainer.evaluate).
//
// ONE read-only pass: per row the loss of the head's training kernel, the flag "the lowest index among the row's maxima is the label"
// and, optionally, that index.  Nothing is written to the logits and columns V .. ld - 1 are never read.  A wave per row, four rows per
// 256-thread workgroup; a row is walked as [0, head) single elements, nv 16-byte pieces, [tail0, V) single elements (head: the elements
// in front of the first 16-byte boundary, 0 for the padded aligned rows the callers use), exactly as the two training kernels walk it.
//
// loss_rows is BIT-IDENTICAL to what the training kernels of elementwise.hip write for the same logits, labels and smoothing, because
// the fp32 reduction of a row is restated here in their order:
//   KIND 0 (ce_fwd_bwd_kernel, a wave per row): element j of the row belongs to lane j % 64 of its region; one (m, ssum, xsum) per lane,
//           singles first (head, then tail), then the pieces i = lane, lane + 64, ...; xor butterfly 32 .. 1; loss in fp32.
//   KIND 1 (kl_acc_fwd_bwd_kernel, a 256-thread workgroup per row): the same with 256 threads.  The wave here plays all four of that
//           kernel's waves: lane l carries the accumulators of threads l, l + 64, l + 128, l + 192 (acc[0 .. 3]), each is reduced by
//           the butterfly, then 1, 2, 3 are merged into 0 in that order -- what the workgroup does through LDS; loss in double on one lane.
// The maximum's index needs no order: the lowest index among the maxima is the same however the row is split.
// Only loads differ from the training kernels: up to four 16-byte loads are in flight per lane before the first is consumed.
// Labels are NOT checked on the device (the kernel indexes x[label] for rows whose label is not ignore_index).
#include "wkv7_common.h"

namespace rwkv7 {

namespace {

struct RowAcc {
    float m, ssum, xsum;
    int best;   // lowest index at which the running maximum m was seen
};

__device__ __forceinline__ void acc_init(RowAcc &a) {
    a.m = -INFINITY;
    a.ssum = 0.f;
    a.xsum = 0.f;
    a.best = 0x7fffffff;
}

__device__ __forceinline__ void acc_one(RowAcc &a, float v, int j) {
    a.best = (v > a.m || (v == a.m && j < a.best)) ? j : a.best;
    const float mn = fmaxf(a.m, v);
    a.ssum = a.ssum * __expf(a.m - mn) + __expf(v - mn);
    a.m = mn;
    a.xsum += v;
}

// one 16-byte piece (8 logits starting at element `base` of the row): one running-max rescale per piece
__device__ __forceinline__ void acc_piece(RowAcc &a, const uint4 r, int base) {
    float f[8];
    f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
    f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
    f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
    f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
    float mx = fmaxf(fmaxf(fmaxf(f[0], f[1]), fmaxf(f[2], f[3])), fmaxf(fmaxf(f[4], f[5]), fmaxf(f[6], f[7])));
    if (mx > a.m || (mx == a.m && base < a.best)) {
#pragma unroll
        for (int j = 7; j >= 0; j--) a.best = f[j] == mx ? base + j : a.best;
    }
    const float mn = fmaxf(a.m, mx);
    float e = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        e += __expf(f[j] - mn);
        a.xsum += f[j];
    }
    a.ssum = a.ssum * __expf(a.m - mn) + e;
    a.m = mn;
}

// a lane that saw no element carries (m, ssum) = (-inf, 0): exp(-inf - mn) = 0 keeps it out, and two such lanes must not form exp(nan) * 0
__device__ __forceinline__ void acc_merge(RowAcc &a, float mo, float so, float xo, int bo) {
    a.best = (mo > a.m || (mo == a.m && bo < a.best)) ? bo : a.best;
    const float mn = fmaxf(a.m, mo);
    a.ssum = (a.m == mn ? a.ssum : a.ssum * __expf(a.m - mn)) + (mo == mn ? so : so * __expf(mo - mn));
    a.m = mn;
    a.xsum += xo;
}

__device__ __forceinline__ void acc_butterfly(RowAcc &a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float mo = __shfl_xor(a.m, off), so = __shfl_xor(a.ssum, off), xo = __shfl_xor(a.xsum, off);
        const int bo = __shfl_xor(a.best, off);
        acc_merge(a, mo, so, xo, bo);
    }
}

}  // namespace

// KIND 0: s = label smoothing of the cross-entropy, C unused.  KIND 1: s = smoothing of the KL target distribution, C its entropy constant.
template <int KIND>
__global__ __launch_bounds__(256) void head_eval_kernel(long rows, int V, long ld, const uint16_t *__restrict__ logits,
                                                        const long *__restrict__ labels, long ignore_index, float s, float C,
                                                        float *__restrict__ loss_rows, int *__restrict__ correct_rows,
                                                        int *__restrict__ argmax_rows) {
    constexpr int NA = KIND == 0 ? 1 : 4;   // accumulators per lane: the threads of the training kernel this lane stands for
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint16_t *x = logits + row * ld;
    const long lab = labels[row];
    const bool valid = lab != ignore_index;
    // [0, head) singles, [head, head + 8 nv) aligned pieces, [head + 8 nv, V) singles
    int head = (int)(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) >> 1);
    head = head < V ? head : V;
    const int nv = (V - head) >> 3, tail0 = head + 8 * nv;
    const uint4 *xv = reinterpret_cast<const uint4 *>(x + head);
    RowAcc acc[NA];
#pragma unroll
    for (int w = 0; w < NA; w++) acc_init(acc[w]);
    // at most 7 singles on each side: they all belong to threads 0 .. 6 of the training kernel, i.e. to acc[0]
    if (lane < head) acc_one(acc[0], bf2f(x[lane]), lane);
    if (tail0 + lane < V) acc_one(acc[0], bf2f(x[tail0 + lane]), tail0 + lane);
    // piece i belongs to thread i % (64 NA); a thread takes its pieces in ascending order.  Four loads per lane and round either way.
    for (int i0 = lane; i0 < nv; i0 += 256) {
        uint4 r[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i0 + 64 * k < nv) r[k] = xv[i0 + 64 * k];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i0 + 64 * k < nv) acc_piece(acc[KIND == 0 ? 0 : k], r[k], head + 8 * (i0 + 64 * k));
    }
#pragma unroll
    for (int w = 0; w < NA; w++) acc_butterfly(acc[w]);
#pragma unroll
    for (int w = 1; w < NA; w++) acc_merge(acc[0], acc[w].m, acc[w].ssum, acc[w].xsum, acc[w].best);
    if (lane != 0) return;
    const float m = acc[0].m, ssum = acc[0].ssum, xsum = acc[0].xsum;
    const int best = acc[0].best;
    if (argmax_rows) argmax_rows[row] = best;
    correct_rows[row] = (valid && best == (int)lab) ? 1 : 0;
    if (!valid) {
        loss_rows[row] = 0.f;
        return;
    }
    if (KIND == 0) {
        const float ls = s;
        const float lse = m + __logf(ssum);
        const float nll = lse - bf2f(x[lab < 0 ? 0 : lab]);
        loss_rows[row] = valid ? (ls > 0.f ? (1.f - ls) * nll + ls * (lse - xsum / (float)V) : nll) : 0.f;
    } else {
        const float xy = bf2f(x[lab]);
        const double L = (double)m + log((double)ssum), dxy = (double)xy, ds = (double)s, vm1 = (double)(V - 1);
        double loss = -(1.0 - ds) * (dxy - L);
        if (s > 0.f) loss += (double)C - ds / vm1 * (((double)xsum - dxy) - vm1 * L);
        loss_rows[row] = (float)loss;
    }
}

int head_eval(long rows, int V, long ld, const void *logits, const long *labels, long ignore_index, int kind, float smoothing, float C,
              float *loss_rows, int *correct_rows, int *argmax_rows, hipStream_t st) {
    (void)hipGetLastError();
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    if (kind == 0)
        hipLaunchKernelGGL(head_eval_kernel<0>, grid, block, 0, st, rows, V, ld, (const uint16_t *)logits, labels, ignore_index, smoothing,
                           C, loss_rows, correct_rows, argmax_rows);
    else
        hipLaunchKernelGGL(head_eval_kernel<1>, grid, block, 0, st, rows, V, ld, (const uint16_t *)logits, labels, ignore_index, smoothing,
                           C, loss_rows, correct_rows, argmax_rows);
    return (int)hipGetLastError();
}

}  // namespace rwkv7
