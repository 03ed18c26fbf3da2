// rwkvtts_amd/csrc/seq_scores.hip -- per-sequence scores from the per-row outputs of rwkv7_head_eval_bf16 (losses.fused_linear_score,
// the heads' score, DataParallelTrainer.score).
//
// Sequence s owns rows seq_start[s] .. seq_start[s + 1] - 1 of loss_rows / correct_rows / labels.  Over its rows with
// label != ignore_index it gets
//     loss_sum   fp64   the sum of loss_rows, accumulated in fp64
//     tokens     int64  the number of such rows
//     correct    int64  the sum of correct_rows
//     worst_loss fp32   the maximum of loss_rows (a NaN counts as larger than every number, as torch.max / torch.argmax take it)
//     worst_row  int64  the lowest row index, relative to seq_start[s], that attains worst_loss
// and 0, 0, 0, 0.0f, -1 when it has no such row (an empty range included).
//
// ONE 256-thread workgroup per sequence, no atomics, nothing shared between workgroups.  The summation order of a sequence depends on
// its length and on nothing else -- not on the grid, on n_seq, on which workgroup took it or on how the rows were chunked upstream:
//   1. thread t adds the rows t, t + 256, t + 512, ... of the sequence, in ascending order, into ONE fp64 partial;
//   2. an xor butterfly (32, 16, ..., 1) combines the 64 partials of a wave; a + b is commutative, so every lane ends with the same bits;
//   3. lane 0 of each wave writes its partial to LDS and thread 0 adds waves 0, 1, 2, 3 in that order.
// The counts are integers and the (maximum, lowest index) pair is a total order, so they are the same in any order.
// An fp64 shuffle is two 32-bit moves (__shfl_xor on a double); the five results are stored by thread 0 with plain vector stores.
// seq_start is device data and is NOT range-checked: every row index in [seq_start[s], seq_start[s + 1]) is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.h"

// the library is built with -ffast-math: the order stated above is a contract, so no reassociation of the fp64 adds in this file
#pragma clang fp reassociate(off)

namespace rwkv7 {

namespace {

struct SeqAcc {
    double sum;
    long tokens, correct;
    float worst;
    long row;   // -1: no valid row seen
};

// is (v, i) in front of (w, j) in the order "larger loss first, NaN largest, then lower row"?  i, j >= 0
__device__ __forceinline__ bool seq_before(float v, long i, float w, long j) {
    const bool vn = v != v, wn = w != w;
    if (vn != wn) return vn;
    if (!vn && v != w) return v > w;
    return i < j;
}

__device__ __forceinline__ void seq_merge(SeqAcc &a, double sum, long tokens, long correct, float worst, long row) {
    a.sum += sum;
    a.tokens += tokens;
    a.correct += correct;
    if (row >= 0 && (a.row < 0 || seq_before(worst, row, a.worst, a.row))) {
        a.worst = worst;
        a.row = row;
    }
}

__device__ __forceinline__ long shfl_xor_long(long v, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(uint64_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), d, 64);
    return (long)(((uint64_t)hi << 32) | lo);
}

}  // namespace

__global__ __launch_bounds__(256) void seq_scores_kernel(const long *__restrict__ seq_start, const float *__restrict__ loss_rows,
                                                         const int *__restrict__ correct_rows, const long *__restrict__ labels,
                                                         long ignore_index, double *__restrict__ loss_sum, long *__restrict__ tokens,
                                                         long *__restrict__ correct, float *__restrict__ worst_loss,
                                                         long *__restrict__ worst_row) {
    __shared__ double sh_sum[4];
    __shared__ long sh_tokens[4], sh_correct[4], sh_row[4];
    __shared__ float sh_worst[4];
    const long s = blockIdx.x;
    const long lo = seq_start[s], hi = seq_start[s + 1];
    SeqAcc a = {0.0, 0, 0, 0.f, -1};
    // step 1: ascending rows, one accumulator per thread (the loads of later rows may be issued early, the adds stay in order)
#pragma unroll 4
    for (long r = lo + threadIdx.x; r < hi; r += 256) {
        const long lab = labels[r];
        const float v = loss_rows[r];
        const int c = correct_rows[r];
        if (lab != ignore_index) seq_merge(a, (double)v, 1, (long)c, v, r - lo);
    }
    // step 2: the wave's butterfly
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double os = __shfl_xor(a.sum, d, 64);
        const long ot = shfl_xor_long(a.tokens, d), oc = shfl_xor_long(a.correct, d), orow = shfl_xor_long(a.row, d);
        const float ow = __shfl_xor(a.worst, d, 64);
        seq_merge(a, os, ot, oc, ow, orow);
    }
    // step 3: the four waves in wave-index order
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh_sum[wave] = a.sum;
        sh_tokens[wave] = a.tokens;
        sh_correct[wave] = a.correct;
        sh_worst[wave] = a.worst;
        sh_row[wave] = a.row;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 1; w < 4; w++) seq_merge(a, sh_sum[w], sh_tokens[w], sh_correct[w], sh_worst[w], sh_row[w]);
    loss_sum[s] = a.sum;
    tokens[s] = a.tokens;
    correct[s] = a.correct;
    worst_loss[s] = a.row < 0 ? 0.f : a.worst;
    worst_row[s] = a.row;
}

int seq_scores(long n_seq, const long *seq_start, const float *loss_rows, const int *correct_rows, const long *labels, long ignore_index,
               double *loss_sum, long *tokens, long *correct, float *worst_loss, long *worst_row, hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(seq_scores_kernel, dim3((unsigned)n_seq), dim3(256), 0, st, seq_start, loss_rows, correct_rows, labels,
                       ignore_index, loss_sum, tokens, correct, worst_loss, worst_row);
    return (int)hipGetLastError();
}

}  // namespace rwkv7
