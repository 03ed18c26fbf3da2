// rwkvtts_amd/csrc/head_loss.hip -- the three kernels that walk a row of bf16 head logits [rows, ld]: the two training heads (loss and
// d loss / d logits in one pass; the cross-entropy one also with a scale per SEQUENCE, rwkv7_ce_seq_bwd_bf16, and with the clipped
// policy-gradient coefficient per ROW, rwkv7_ce_policy_fwd_bwd_bf16, and with the z-loss / max-logit regularisers,
// rwkv7_ce_reg_fwd_bwd_bf16) and the forward-only
// metrics of held-out evaluation.  They share ONE row body (the anonymous namespace
// below): how a row is split, how a thread folds elements into (m, ssum, xsum[, best]), how two such partials merge, the two closing
// loss formulas and the gradient of an element.  A kernel adds only its structure: which thread owns which element and in which order
// the partials meet.  So head_eval_kernel's loss_rows / correct_rows are bit-identical to the training kernels' by construction.
// Labels are NOT checked on the device (the kernels index x[label] for rows whose label is not ignore_index); columns V .. ld - 1 are
// neither read nor written.
#include "launchers.h"
#include "ln_row.h"

namespace rwkv7 {

namespace {

// A row is walked as [0, head) single elements, nv 16-byte pieces (8 logits each), [tail0, V) single elements.  head: the elements in
// front of the first 16-byte boundary (V is odd for the Spark head -- 8 193 -- so an unpadded row starts on any 2-byte boundary; 0 for the
// padded aligned rows), at most 7 on each side.  singles: no pieces at all, head = V.
struct RowSplit {
    int head, nv, tail0;
};

__device__ __forceinline__ RowSplit row_split(const uint16_t *x, int V, bool singles = false) {
    RowSplit sp;
    sp.head = singles ? V : (int)(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) >> 1);
    sp.head = sp.head < V ? sp.head : V;
    sp.nv = (V - sp.head) >> 3;
    sp.tail0 = sp.head + 8 * sp.nv;
    return sp;
}

__device__ __forceinline__ void unpack8(const uint4 r, float (&f)[8]) {
    f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
    f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
    f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
    f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
}

// online max / sum-of-exp of the elements a thread has seen, all fp32 from the bf16 logits (running maximum subtracted before exp)
template <bool ARGMAX>
struct RowAcc {
    float m, ssum, xsum;   // xsum: sum of the logits (the smoothing term)
    int best;              // ARGMAX: lowest index at which the running maximum m was seen; otherwise never touched
};

template <bool ARGMAX>
__device__ __forceinline__ void acc_init(RowAcc<ARGMAX> &a) {
    a.m = -INFINITY;
    a.ssum = 0.f;
    a.xsum = 0.f;
    if constexpr (ARGMAX) a.best = 0x7fffffff;
}

template <bool ARGMAX>
__device__ __forceinline__ void acc_one(RowAcc<ARGMAX> &a, float v, int j) {
    if constexpr (ARGMAX) a.best = (v > a.m || (v == a.m && j < a.best)) ? j : a.best;
    const float mn = fmaxf(a.m, v);
    a.ssum = a.ssum * __expf(a.m - mn) + __expf(v - mn);
    a.m = mn;
    a.xsum += v;
}

// one 16-byte piece (8 logits starting at element `base` of the row): one running-max rescale per piece instead of one per element
// (9 exponentials per 8 logits instead of 16)
template <bool ARGMAX>
__device__ __forceinline__ void acc_piece(RowAcc<ARGMAX> &a, const uint4 r, int base) {
    float f[8];
    unpack8(r, f);
    const float mx = fmaxf(fmaxf(fmaxf(f[0], f[1]), fmaxf(f[2], f[3])), fmaxf(fmaxf(f[4], f[5]), fmaxf(f[6], f[7])));
    if constexpr (ARGMAX) {
        if (mx > a.m || (mx == a.m && base < a.best)) {
#pragma unroll
            for (int j = 7; j >= 0; j--) a.best = f[j] == mx ? base + j : a.best;
        }
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

// a thread that saw no element carries (m, ssum, xsum, best) = (-inf, 0, 0, INT_MAX): exp(-inf - mn) = 0 keeps it out, and two such
// threads must not form exp(nan) * 0
template <bool ARGMAX>
__device__ __forceinline__ void acc_merge(RowAcc<ARGMAX> &a, float mo, float so, float xo, int bo) {
    if constexpr (ARGMAX) a.best = (mo > a.m || (mo == a.m && bo < a.best)) ? bo : a.best;
    const float mn = fmaxf(a.m, mo);
    a.ssum = (a.m == mn ? a.ssum : a.ssum * __expf(a.m - mn)) + (mo == mn ? so : so * __expf(mo - mn));
    a.m = mn;
    a.xsum += xo;
}

// xor butterfly 32 .. 1 over the wave: every lane ends with the wave's partial
template <bool ARGMAX>
__device__ __forceinline__ void acc_butterfly(RowAcc<ARGMAX> &a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float mo = __shfl_xor(a.m, off), so = __shfl_xor(a.ssum, off), xo = __shfl_xor(a.xsum, off);
        int bo = 0;
        if constexpr (ARGMAX) bo = __shfl_xor(a.best, off);
        acc_merge(a, mo, so, xo, bo);
    }
}

template <bool ARGMAX>
__device__ __forceinline__ float acc_lse(const RowAcc<ARGMAX> &a) {
    return a.m + __logf(a.ssum);
}

// cross-entropy with label smoothing ls (torch.nn.CrossEntropyLoss(label_smoothing), xy_llm.py:233-240) of a valid row, fp32:
// (1 - ls)(lse - x[label]) + ls (lse - mean x); ls = 0 is the plain form, bit for bit what it was before smoothing existed
__device__ __forceinline__ float ce_row_loss(float lse, float xsum, float xlab, int V, float ls) {
    const float nll = lse - xlab;
    return ls > 0.f ? (1.f - ls) * nll + ls * (lse - xsum / (float)V) : nll;
}

// label-smoothing KL of a valid row, in double on one thread: C - (1 - s)(x_y - lse) - s/(V-1) ((sum_j x_j - x_y) - (V-1) lse)
__device__ __forceinline__ float kl_row_loss(float m, float ssum, float xsum, float xy, int V, float s, float C) {
    const double L = (double)m + log((double)ssum), dxy = (double)xy, ds = (double)s, vm1 = (double)(V - 1);
    double loss = -(1.0 - ds) * (dxy - L);
    if (s > 0.f) loss += (double)C - ds / vm1 * (((double)xsum - dxy) - vm1 * L);
    return (float)loss;
}

// d loss / d logits of element j: (softmax_j - target_j) * sc, one bf16 rounding of the fp32 value.  minus_target(p, j) takes the
// softmax value p to p - target_j in the caller's own expression:  CE  p - ls / V - (1 - ls) [j == label];
// KL  p - (j == label ? 1 - s : s / (V - 1)).
template <typename F>
__device__ __forceinline__ uint16_t grad_one(float v, int j, float lse, float sc, F minus_target) {
    return (uint16_t)pk_bf16(minus_target(__expf(v - lse), j) * sc, 0.f);
}

// ... of the piece whose first element is `base`: the gradients leave as one 16-byte store through v_cvt_pk_bf16_f32
template <typename F>
__device__ __forceinline__ uint4 grad_piece(const uint4 r, int base, float lse, float sc, F minus_target) {
    float f[8];
    unpack8(r, f);
#pragma unroll
    for (int j = 0; j < 8; j++) f[j] = minus_target(__expf(f[j] - lse), base + j) * sc;
    return make_uint4(pk_bf16(f[0], f[1]), pk_bf16(f[2], f[3]), pk_bf16(f[4], f[5]), pk_bf16(f[6], f[7]));
}

}  // namespace

// ------------------------------------------------------------------------------------------------------
// softmax cross-entropy of one chunk of head logits, forward and backward in one kernel
// (model/llm/spark_llm.py:146-160 uses rwkvfla's FusedLinearCrossEntropyLoss; the chunking over tokens lives in
// rwkvtts_amd/losses.py).  One wave per row, four rows per workgroup: online max / sum-of-exp over the row (bf16 logits as the GEMM
// wrote them, no fp32 copy), then the row is rewritten IN PLACE with d loss / d logits = (softmax - onehot(label)) * scale, or 0
// for ignored rows; loss_rows[row] = (logsumexp - logit[label]) * valid.  Two reads (the second from L2) + one write.
// Lane l folds its singles first (head, then tail), then the pieces l, l + 64, ...; xor butterfly; loss in fp32.
// ------------------------------------------------------------------------------------------------------
// Round 4: the row is walked in 16-byte pieces (8 logits per lane and load).  The first form read and wrote 2 bytes per lane and
// instruction: 98 us per 4 096 x 8 193 chunk.
// label smoothing ls: d loss / d x_j = softmax_j - ls / V - (1 - ls) [j == label].
// ld: elements between rows (>= V; round 6: the Spark head's logits live in a buffer padded to a multiple of 256 columns, so rows are 16-byte
// aligned and the head GEMMs see aligned leading dimensions)
// Where a row's scale comes from is the kernel's first parameter (Scale, the three structs below): one value for the whole chunk
// (rwkv7_ce_fwd_bwd*_bf16: loss_rows is never NULL there), the value of the row's SEQUENCE (rwkv7_ce_seq_bwd_bf16, the backward of
// losses.fused_linear_seq_logprob: the upstream gradient of a per-sequence sum of log-probabilities differs from sequence to sequence,
// so it cannot be applied to the finished gradient afterwards as one scalar; loss_rows may be NULL), or the clipped policy-gradient
// coefficient of the row (rwkv7_ce_policy_fwd_bwd_bf16: PolicyScale, which also writes the row's statistics; loss_rows is NULL).
// Everything else is one text.
// Every source is called as scale_of(row, valid, lp, lane) by all 64 lanes of the row's wave with the same arguments but `lane`: valid --
// the label is not ignore_index; lp = x[label] - lse, the row's fp32 log-probability of its label (meaningless when !valid).  The first
// two ignore lp and lane.
struct UniformScale {
    float scale;
    __device__ __forceinline__ float operator()(long, bool valid, float, int) const { return valid ? scale : 0.f; }
};

// Row r of the chunk is row row0 + r of the batch; its sequence is the largest s < n_seq with seq_start[s] <= row0 + r, provided
// row0 + r < seq_start[n_seq] (seq_start: n_seq + 1 non-decreasing offsets; equal neighbours are empty sequences, which own no row).
// A row in front of seq_start[0] or at / behind seq_start[n_seq] has no sequence (-1).  The search is the same for the
// 64 lanes of a row's wave: the row index goes through readfirstlane, so the offsets arrive by scalar loads and no lane diverges.
struct SeqOfRow {
    long row0, n_seq;
    const long *seq_start;
    __device__ __forceinline__ long operator()(long row) const {
        const long g = row0 + row;
        const long gu = ((long)__builtin_amdgcn_readfirstlane((int)(g >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)g);
        if (gu >= seq_start[n_seq]) return -1;
        long lo = 0, hi = n_seq;   // lo ends as the number of s < n_seq with seq_start[s] <= gu
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (seq_start[mid] <= gu) lo = mid + 1; else hi = mid;
        }
        return lo - 1;
    }
};

// A row without a sequence gets scale 0, like an ignored row.
struct SeqScale {
    SeqOfRow seq_of;
    const float *seq_scale;
    __device__ __forceinline__ float operator()(long row, bool valid, float, int) const {
        if (!valid) return 0.f;
        const long s = seq_of(row);
        return s >= 0 ? seq_scale[s] : 0.f;
    }
};

// The token-level clipped policy objective (PPO-clip / GRPO; rwkv7_ce_policy_fwd_bwd_bf16, losses.fused_linear_policy): the row's loss
// term and its coefficient on (softmax - onehot) follow from the row's own lp and from data known before the launch -- old_lp / ref_lp of
// batch row row0 + r, adv / seq_w of its sequence.  The closing arithmetic of a row runs in double (kl_row_loss's precedent), from the
// fp32 lp, and it runs REPLICATED on all 64 lanes of the row's wave on purpose -- two exponentials, a clamp and the loads of old_lp /
// ref_lp from one shared address per row, next to V / 64 exponentials per lane in each pass over the row: one lane computing and a
// broadcast of sc would save nothing measurable and add a cross-lane step in front of the gradient pass.
//   rho = exp(lp - old_lp);  s1 = rho A;  s2 = clamp(rho, lo, hi) A;  the unclipped branch s1 is taken unless s1 > s2 (ties are active, as
//   the gradient of torch.minimum / clamp has it; a NaN stays a NaN);  l = -min(s1, s2);  coef = s1 where taken, else 0
//   with ref_lp:  d = ref_lp - lp;  kl = exp(d) - d - 1 (the k3 estimator);  l += beta kl;  coef -= beta (1 - exp(d))
//   sc = (float)(w coef)
// Without ref_lp the KL lines are not executed at all: coef is s1 or 0 and sc the correctly rounded product w (rho A) -- at rho = 1 the
// fp32 product w A, which is how the row then equals rwkv7_ce_seq_bwd_bf16's with seq_scale = w A bit for bit.
// Lane 0 writes the row's statistics (each array may be NULL); ignored rows and rows without a sequence give sc = 0 and zero statistics.
struct PolicyScale {
    SeqOfRow seq_of;
    const float *adv, *seq_w, *old_lp, *ref_lp;
    double lo, hi, beta;   // 1 - eps_lo, 1 + eps_hi
    float *lp_rows, *loss_rows, *kl_rows, *clip_rows;
    __device__ __forceinline__ float operator()(long row, bool valid, float lp, int lane) const {
        const long s = valid ? seq_of(row) : -1;
        float sc = 0.f, lp_o = 0.f, l_o = 0.f, kl_o = 0.f, clip_o = 0.f;
        if (s >= 0) {
            const long g = seq_of.row0 + row;
            const double A = (double)adv[s], rho = exp((double)lp - (double)old_lp[g]);
            const double s1 = rho * A, s2 = fmin(fmax(rho, lo), hi) * A;
            const bool take1 = !(s1 > s2);
            double l = -(take1 ? s1 : s2), coef = take1 ? s1 : 0.0;
            if (ref_lp != nullptr) {
                const double d = (double)ref_lp[g] - (double)lp, e = exp(d), kl = e - d - 1.0;
                l += beta * kl;
                coef -= beta * (1.0 - e);
                kl_o = (float)kl;
            }
            sc = (float)((double)seq_w[s] * coef);
            lp_o = lp;
            l_o = (float)l;
            clip_o = take1 ? 0.f : 1.f;
        }
        if (lane == 0) {
            if (lp_rows) lp_rows[row] = lp_o;
            if (loss_rows) loss_rows[row] = l_o;
            if (kl_rows) kl_rows[row] = kl_o;
            if (clip_rows) clip_rows[row] = clip_o;
        }
        return sc;
    }
};

// What is added to a row's gradient beside the cross-entropy is the kernel's second parameter (Reg).  reg.row(...) is called by all 64
// lanes of the row's wave once the row's partials have met (acc is the whole row's on every lane) and returns the row's map of a softmax
// value p_j to what takes its place in front of "- target_j":
//   NoReg    : p_j itself, from RowAcc<false> -- the code of the three cross-entropy entries as it always was.
//   LogitReg : p_j k + [j == a] c m  (rwkv7_ce_reg_fwd_bwd_bf16), k = 1 + 2 z lse the derivative of lse + z lse^2
//              by lse, c m the derivative of 0.5 c m^2 by the row's maximum m, which lands on a, the LOWEST index among the row's maxima
//              (RowAcc<true>: head_eval_kernel's arg-max fold, which changes no bit of m, ssum or xsum).  Lane 0 writes the row's lse and
//              m (0 for an ignored row; each array may be NULL).  At z = c = 0: k = 1 and the bump 0 exactly, the row is NoReg's.
struct NoReg {
    static constexpr bool ARGMAX = false;
    struct Row {
        __device__ __forceinline__ float operator()(float p, int) const { return p; }
    };
    __device__ __forceinline__ Row row(long, bool, float, const RowAcc<false> &, int) const { return Row{}; }
};

struct LogitReg {
    static constexpr bool ARGMAX = true;
    float z, c;
    float *lse_rows, *max_rows;
    struct Row {
        float k, cm;
        int a;
        __device__ __forceinline__ float operator()(float p, int j) const {
            const float q = p * k;
            return j == a ? q + cm : q;
        }
    };
    __device__ __forceinline__ Row row(long row, bool valid, float lse, const RowAcc<true> &acc, int lane) const {
        if (lane == 0) {
            if (lse_rows) lse_rows[row] = valid ? lse : 0.f;
            if (max_rows) max_rows[row] = valid ? acc.m : 0.f;
        }
        return Row{1.f + 2.f * z * lse, c * acc.m, acc.best};
    }
};

template <typename Scale, typename Reg>
__global__ __launch_bounds__(256) void ce_fwd_bwd_kernel(long rows, int V, long ld, bf16_t *__restrict__ logits, const long *__restrict__ labels,
                                                         long ignore_index, Scale scale_of, Reg reg, float *__restrict__ loss_rows, float ls) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    uint16_t *x = reinterpret_cast<uint16_t *>(logits) + row * ld;
    const long lab = labels[row];
    const bool valid = lab != ignore_index;
    const RowSplit sp = row_split(x, V);
    const uint4 *xv = reinterpret_cast<const uint4 *>(x + sp.head);
    RowAcc<Reg::ARGMAX> acc;
    acc_init(acc);
    if (lane < sp.head) acc_one(acc, bf2f(x[lane]), lane);
    if (sp.tail0 + lane < V) acc_one(acc, bf2f(x[sp.tail0 + lane]), sp.tail0 + lane);
    for (int i = lane; i < sp.nv; i += 64) acc_piece(acc, xv[i], sp.head + 8 * i);
    acc_butterfly(acc);
    const float lse = acc_lse(acc);
    // before any store of this row.  An ignored row reads its own first element, never x[ignore_index]; a valid row reads what it always read
    const float xlab = bf2f(x[(valid && lab > 0) ? lab : 0]);
    if (lane == 0 && loss_rows) loss_rows[row] = valid ? ce_row_loss(lse, acc.xsum, xlab, V, ls) : 0.f;
    const float sc = scale_of(row, valid, xlab - lse, lane), hit = 1.f - ls, off_all = ls / (float)V;
    const int labi = (int)lab;   // an ignored row's gradient is 0 whatever this matches
    const auto reg_row = reg.row(row, valid, lse, acc, lane);
    auto minus_target = [&](float p, int j) { return reg_row(p, j) - off_all - (j == labi ? hit : 0.f); };
    if (lane < sp.head) x[lane] = grad_one(bf2f(x[lane]), lane, lse, sc, minus_target);
    if (sp.tail0 + lane < V) x[sp.tail0 + lane] = grad_one(bf2f(x[sp.tail0 + lane]), sp.tail0 + lane, lse, sc, minus_target);
    uint4 *xw = reinterpret_cast<uint4 *>(x + sp.head);
    for (int i = lane; i < sp.nv; i += 64) xw[i] = grad_piece(xv[i], sp.head + 8 * i, lse, sc, minus_target);
}

int ce_fwd_bwd(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
               float label_smoothing, hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((ce_fwd_bwd_kernel<UniformScale, NoReg>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, rows, V, ld,
                       (bf16_t *)logits, labels, ignore_index, UniformScale{scale}, NoReg{}, loss_rows, label_smoothing);
    return (int)hipGetLastError();
}

int ce_reg_fwd_bwd(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, float scale, float *loss_rows,
                   float label_smoothing, float z_coef, float max_coef, float *lse_rows, float *max_rows, hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((ce_fwd_bwd_kernel<UniformScale, LogitReg>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, rows, V, ld,
                       (bf16_t *)logits, labels, ignore_index, UniformScale{scale}, LogitReg{z_coef, max_coef, lse_rows, max_rows}, loss_rows,
                       label_smoothing);
    return (int)hipGetLastError();
}

int ce_seq_bwd(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, long row0, long n_seq,
               const long *seq_start, const float *seq_scale, float *loss_rows, hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((ce_fwd_bwd_kernel<SeqScale, NoReg>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, rows, V, ld, (bf16_t *)logits,
                       labels, ignore_index, SeqScale{{row0, n_seq, seq_start}, seq_scale}, NoReg{}, loss_rows, 0.f);
    return (int)hipGetLastError();
}

int ce_policy_fwd_bwd(long rows, int V, long ld, void *logits, const long *labels, long ignore_index, long row0, long n_seq,
                      const long *seq_start, const float *adv, const float *seq_w, const float *old_lp, const float *ref_lp, float eps_lo,
                      float eps_hi, float beta, float *lp_rows, float *loss_rows, float *kl_rows, float *clip_rows, hipStream_t st) {
    (void)hipGetLastError();
    const PolicyScale ps{{row0, n_seq, seq_start}, adv, seq_w, old_lp, ref_lp, 1.0 - (double)eps_lo, 1.0 + (double)eps_hi, (double)beta,
                         lp_rows, loss_rows, kl_rows, clip_rows};
    hipLaunchKernelGGL((ce_fwd_bwd_kernel<PolicyScale, NoReg>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, rows, V, ld, (bf16_t *)logits,
                       labels, ignore_index, ps, NoReg{}, nullptr, 0.f);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------
// label-smoothing KL loss + accuracy of one chunk of Cosy head logits, forward and backward in one kernel
// (third_party/cosyvoice/transformer/label_smoothing_loss.py:68-96 + utils/common.py:76-95; the chunking over tokens lives in
// rwkvtts_amd/losses.py).  Target distribution t: 1 - s on the label, s / (V - 1) elsewhere.  Per valid row
//   loss = C - (1 - s)(x_y - lse) - s/(V-1) ((sum_j x_j - x_y) - (V-1) lse),  C = (1-s) ln(1-s) + s ln(s/(V-1))  (host, double -> float)
//   dx_j = (exp(x_j - lse) - t_j) * scale        (one bf16 rounding of the fp32 value)
//   correct = [lowest index among the row's maxima == y]                       (torch.argmax's tie rule on the CPU)
// ignored rows: 0 everywhere.  ONE 256-thread workgroup per row (V = 6562: 820 16-byte pieces, 3.2 per thread).  REG: V <= 8192 and
// the row is kept in registers between the reduction and the gradient (one read, one write); otherwise the second pass reads the row again
// (from L2: a 16 KB+ row a workgroup has just walked).  Every thread reads in the second pass exactly the elements it then writes, and the
// label's logit is read before the block-wide reduction, so dx may be x (in place).
// Rows of an unpadded V = 6562 buffer start on 4-byte boundaries.  vec = 0 (x and dx differ modulo 16 bytes): everything goes through
// the 2-byte loops.  Thread t folds its singles first (head, then tail), then the pieces t, t + 256, ...; xor butterfly per wave, then
// the four waves through LDS in wave order; the closing arithmetic of the row's loss runs in double on one thread.
// ------------------------------------------------------------------------------------------------------
template <bool REG>
__global__ __launch_bounds__(256) void kl_acc_fwd_bwd_kernel(long rows, int V, long ld, const uint16_t *logits, uint16_t *dlogits,
                                                             const long *__restrict__ labels, long ignore_index, float s, float C, float scale,
                                                             float *__restrict__ loss_rows, int *__restrict__ correct_rows, int vec) {
    __shared__ float red_m[4], red_s[4], red_x[4];
    __shared__ int red_i[4];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint16_t *x = logits + row * ld;
        uint16_t *dx = dlogits + row * ld;
        const long lab = labels[row];
        const RowSplit sp = row_split(x, V, !vec);
        const uint4 *xv = reinterpret_cast<const uint4 *>(x + sp.head);
        uint4 *dv = reinterpret_cast<uint4 *>(dx + sp.head);
        if (lab == ignore_index) {   // the whole workgroup takes this branch: no barrier is skipped by a part of it
            for (int j = tid; j < sp.head; j += 256) dx[j] = 0;
            for (int j = sp.tail0 + tid; j < V; j += 256) dx[j] = 0;
            for (int i = tid; i < sp.nv; i += 256) dv[i] = make_uint4(0u, 0u, 0u, 0u);
            if (tid == 0) {
                loss_rows[row] = 0.f;
                correct_rows[row] = 0;
            }
            continue;
        }
        const float xy = bf2f(x[lab]);   // before any store of this row
        RowAcc<true> acc;
        acc_init(acc);
        for (int j = tid; j < sp.head; j += 256) acc_one(acc, bf2f(x[j]), j);
        for (int j = sp.tail0 + tid; j < V; j += 256) acc_one(acc, bf2f(x[j]), j);
        uint4 r[4];
        if (REG) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (tid + 256 * k < sp.nv) r[k] = xv[tid + 256 * k];
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (tid + 256 * k < sp.nv) acc_piece(acc, r[k], sp.head + 8 * (tid + 256 * k));
        } else {
            for (int i = tid; i < sp.nv; i += 256) acc_piece(acc, xv[i], sp.head + 8 * i);
        }
        acc_butterfly(acc);
        if ((tid & 63) == 0) {
            red_m[wave] = acc.m; red_s[wave] = acc.ssum; red_x[wave] = acc.xsum; red_i[wave] = acc.best;
        }
        __syncthreads();
        acc.m = red_m[0]; acc.ssum = red_s[0]; acc.xsum = red_x[0]; acc.best = red_i[0];
#pragma unroll
        for (int w = 1; w < 4; w++) acc_merge(acc, red_m[w], red_s[w], red_x[w], red_i[w]);
        __syncthreads();   // red_* are free for the next row
        const float lse = acc_lse(acc);
        if (tid == 0) {
            loss_rows[row] = kl_row_loss(acc.m, acc.ssum, acc.xsum, xy, V, s, C);
            correct_rows[row] = acc.best == (int)lab ? 1 : 0;
        }
        const float hit = 1.f - s, off_t = s / (float)(V - 1);
        const int labi = (int)lab;
        auto minus_target = [&](float p, int j) { return p - (j == labi ? hit : off_t); };
        for (int j = tid; j < sp.head; j += 256) dx[j] = grad_one(bf2f(x[j]), j, lse, scale, minus_target);
        for (int j = sp.tail0 + tid; j < V; j += 256) dx[j] = grad_one(bf2f(x[j]), j, lse, scale, minus_target);
        if (REG) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (tid + 256 * k < sp.nv) dv[tid + 256 * k] = grad_piece(r[k], sp.head + 8 * (tid + 256 * k), lse, scale, minus_target);
        } else {
            for (int i = tid; i < sp.nv; i += 256) dv[i] = grad_piece(xv[i], sp.head + 8 * i, lse, scale, minus_target);
        }
    }
}

int kl_acc_fwd_bwd(long rows, int V, long ld, const void *logits, void *dlogits, const long *labels, long ignore_index, float smoothing,
                   float C, float scale, float *loss_rows, int *correct_rows, hipStream_t st) {
    (void)hipGetLastError();
    // 16-byte pieces need x and dx rows that agree modulo 16 bytes (same ld: the two base pointers decide it for every row)
    const int vec = ((reinterpret_cast<uintptr_t>(logits) ^ reinterpret_cast<uintptr_t>(dlogits)) & 15) == 0;
    const unsigned grid = (unsigned)(rows < (1L << 20) ? rows : (1L << 20));
    if (vec && V <= 8192)
        hipLaunchKernelGGL(kl_acc_fwd_bwd_kernel<true>, dim3(grid), dim3(256), 0, st, rows, V, ld, (const uint16_t *)logits,
                           (uint16_t *)dlogits, labels, ignore_index, smoothing, C, scale, loss_rows, correct_rows, vec);
    else
        hipLaunchKernelGGL(kl_acc_fwd_bwd_kernel<false>, dim3(grid), dim3(256), 0, st, rows, V, ld, (const uint16_t *)logits,
                           (uint16_t *)dlogits, labels, ignore_index, smoothing, C, scale, loss_rows, correct_rows, vec);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------
// forward-only head metrics of one chunk of head logits (held-out evaluation: losses.fused_linear_eval, the heads' eval_metrics,
// DataParallelTrainer.evaluate).  ONE read-only pass: per row the loss of the head's training kernel, the flag
// "the lowest index among the row's maxima is the label" and, optionally, that index.  Nothing is written to the logits.
// A wave per row, four rows per workgroup.  The arithmetic and its order inside a thread are the shared row body above; what this
// kernel has to keep by itself is the mapping of its lanes to the training kernel's threads, since a partial is the fold of ONE such
// thread's elements in ascending order and the partials merge in that kernel's order:
//   KIND 0 (ce_fwd_bwd_kernel, also a wave per row): lane l is that kernel's lane l -- one accumulator, the same loops.
//   KIND 1 (kl_acc_fwd_bwd_kernel, a 256-thread workgroup per row): lane l carries the accumulators of threads l, l + 64, l + 128,
//           l + 192 (acc[0 .. 3] = that kernel's four waves): piece i goes to acc[(i >> 6) & 3], the at most 7 singles on each side
//           belong to threads 0 .. 6, i.e. to acc[0]; each accumulator takes the butterfly, then 1, 2, 3 are merged into 0 in that
//           order -- what the workgroup does through LDS.
// The maximum's index needs no order: the lowest index among the maxima is the same however the row is split.
// Only loads differ from the training kernels: up to four 16-byte loads are in flight per lane before the first is consumed.
// KIND 0: s = label smoothing of the cross-entropy, C unused.  KIND 1: s = smoothing of the KL target distribution, C its entropy constant.
// ------------------------------------------------------------------------------------------------------
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
    const RowSplit sp = row_split(x, V);
    const uint4 *xv = reinterpret_cast<const uint4 *>(x + sp.head);
    RowAcc<true> acc[NA];
#pragma unroll
    for (int w = 0; w < NA; w++) acc_init(acc[w]);
    if (lane < sp.head) acc_one(acc[0], bf2f(x[lane]), lane);
    if (sp.tail0 + lane < V) acc_one(acc[0], bf2f(x[sp.tail0 + lane]), sp.tail0 + lane);
    // a thread takes its pieces in ascending order.  Four loads per lane and round either way.
    for (int i0 = lane; i0 < sp.nv; i0 += 256) {
        uint4 r[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i0 + 64 * k < sp.nv) r[k] = xv[i0 + 64 * k];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i0 + 64 * k < sp.nv) acc_piece(acc[KIND == 0 ? 0 : k], r[k], sp.head + 8 * (i0 + 64 * k));
    }
#pragma unroll
    for (int w = 0; w < NA; w++) acc_butterfly(acc[w]);
#pragma unroll
    for (int w = 1; w < NA; w++) acc_merge(acc[0], acc[w].m, acc[w].ssum, acc[w].xsum, acc[w].best);
    if (lane != 0) return;
    if (argmax_rows) argmax_rows[row] = acc[0].best;
    correct_rows[row] = (valid && acc[0].best == (int)lab) ? 1 : 0;
    if (!valid)
        loss_rows[row] = 0.f;
    else if (KIND == 0)
        loss_rows[row] = ce_row_loss(acc_lse(acc[0]), acc[0].xsum, bf2f(x[lab < 0 ? 0 : lab]), V, s);
    else
        loss_rows[row] = kl_row_loss(acc[0].m, acc[0].ssum, acc[0].xsum, bf2f(x[lab]), V, s, C);
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
