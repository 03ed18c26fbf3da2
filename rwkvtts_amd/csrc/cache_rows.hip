// rwkvtts_amd/csrc/cache_rows.hip -- whole cache rows in ONE launch, all three fields (att_x_prev bf16 [S,D], att_kv fp32 [S,H,64,64],
// ffn_x_prev bf16 [S,D]) of all layers: what 3 L index_copy_ (and index_fill_) calls do.  Three entries over one copy body:
//   commit (rwkvtts_amd/continuous.py, admission="overlap" and submit_n): for every entry i with src_row[i] >= 0 and dst_row[i] >= 0,
//          row src_row[i] of a source cache is copied to row dst_row[i] of a destination cache;
//   seed   (rwkvtts_amd/state_store.py, admission from a stored state): the same, and an entry with src_row[i] == RWKV7_SEED_ZERO (-1)
//          writes zeros to row dst_row[i] instead (a fresh request next to seeded ones); src_row[i] < -1 skips the entry;
//   retain (rwkvtts_amd/continuous.py, retain=True; inside the captured step): row s of the engine's cache -> row retain_row[s] of a
//          StateStore's cache in the launch in which slot s is found armed and dead; that launch disarms the slot (below).
//
// A row of the three fields of one layer is one virtual array of 16-byte vectors: D/8 | 1024 H | D/8 (D = 64 H, so 1040 H in all).
// Grid (piece of that array, entry, layer); a thread moves kCommitVecs vectors, all loads issued before the first store.  The field
// pointers come from two device tables, the rows from two device index arrays, so nothing about a particular admission reaches the
// launch -- the choice between copy and zero included.  Plain 16-byte vector loads and stores, no LDS, bits preserved whatever they
// encode; no atomics but the retain entry's ticket, one per copying workgroup.
//
// Neither row index is range-checked against the caches' row counts (device data; the caller's guarantee, include/rwkv7_hip.h); a
// negative destination skips the entry, and so does a negative source other than the seed entry's zero mark.  Destination rows must
// be distinct among the active entries.
#include <hip/hip_runtime.h>

#include "../../include/rwkv7_hip.h"
#include "launchers.h"

namespace rwkv7 {

constexpr int kCommitThreads = 256, kCommitVecs = 4;

// The copy body of every entry: this workgroup's piece (blockIdx.x) of row sr of layer l of the source -> row dr of the destination, or
// zeros (`zero`: nothing is read).  The caller has decided, uniformly over the workgroup, that the row is to be written.
__device__ __forceinline__ void copy_piece(const uint4 *const *__restrict__ src_tbl, uint4 *const *__restrict__ dst_tbl, int l, long sr,
                                           long dr, bool zero, int xv, int kvv) {
    const uint4 *const s0 = src_tbl[3 * l], *const s1 = src_tbl[3 * l + 1], *const s2 = src_tbl[3 * l + 2];
    uint4 *const d0 = dst_tbl[3 * l], *const d1 = dst_tbl[3 * l + 1], *const d2 = dst_tbl[3 * l + 2];
    const int nv = 2 * xv + kvv;
    const int base = blockIdx.x * (kCommitThreads * kCommitVecs) + threadIdx.x;
    uint4 v[kCommitVecs];
    uint4 *to[kCommitVecs];
#pragma unroll
    for (int j = 0; j < kCommitVecs; j++) {
        const int i = base + j * kCommitThreads;
        to[j] = nullptr;
        if (i < nv) {
            const uint4 *from;
            if (i < xv) {
                from = s0 + sr * xv + i;
                to[j] = d0 + dr * xv + i;
            } else if (i < xv + kvv) {
                from = s1 + sr * kvv + (i - xv);
                to[j] = d1 + dr * kvv + (i - xv);
            } else {
                from = s2 + sr * xv + (i - xv - kvv);
                to[j] = d2 + dr * xv + (i - xv - kvv);
            }
            v[j] = zero ? make_uint4(0, 0, 0, 0) : *from;   // a zero entry reads nothing: `from` is never dereferenced
        }
    }
#pragma unroll
    for (int j = 0; j < kCommitVecs; j++)
        if (to[j]) *to[j] = v[j];
}

// kZero: a source row of RWKV7_SEED_ZERO means "write zeros" (the seed entry); without it every negative source row skips (commit)
template <bool kZero>
__global__ __launch_bounds__(kCommitThreads) void cache_rows_kernel(const uint4 *const *__restrict__ src_tbl,
                                                                    uint4 *const *__restrict__ dst_tbl,
                                                                    const int *__restrict__ src_row,
                                                                    const int *__restrict__ dst_row, int xv, int kvv) {
    const int e = blockIdx.y, l = blockIdx.z;
    const long sr = src_row[e], dr = dst_row[e];
    const bool zero = kZero && sr == RWKV7_SEED_ZERO;
    if ((sr < 0 && !zero) || dr < 0) return;   // uniform over the workgroup
    copy_piece(src_tbl, dst_tbl, l, sr, dr, zero, xv, kvv);
}

// retain: slot s (blockIdx.y) is copied when it is armed, dead and has a row to go to.  gridDim.x * gridDim.z workgroups serve one
// slot and each decides for itself, so none of them may see armed[s] cleared by another: every workgroup reads the flags, copies its
// piece and only then draws a ticket (device-scope atomicAdd); the one that draws the last ticket knows that every other workgroup of
// the slot has read the flags, and clears armed[s] and the ticket word.  A slot that is not copied returns on the three flag loads.
__global__ __launch_bounds__(kCommitThreads) void cache_rows_retain_kernel(const uint4 *const *__restrict__ src_tbl,
                                                                           uint4 *const *__restrict__ dst_tbl,
                                                                           const unsigned char *__restrict__ live, unsigned char *armed,
                                                                           const int *__restrict__ retain_row, int *ticket, int xv,
                                                                           int kvv) {
    const int s = blockIdx.y, l = blockIdx.z;
    if (!armed[s] || live[s]) return;   // uniform over the workgroup, and over the slot's workgroups: armed[s] is cleared only
    const long dr = retain_row[s];      // after all of them have passed the barrier below
    if (dr < 0) return;
    copy_piece(src_tbl, dst_tbl, l, s, dr, false, xv, kvv);
    __syncthreads();   // every wave of this workgroup has read its flags
    if (threadIdx.x == 0) {
        const int last = (int)(gridDim.x * gridDim.z) - 1;
        if (__hip_atomic_fetch_add(&ticket[s], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == last) {
            __hip_atomic_store(&armed[s], (unsigned char)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ticket[s], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // zero between launches
        }
    }
}

template <bool kZero>
static int cache_rows_launch(int layers, int n, const void *const *src_tbl, void *const *dst_tbl, const int *src_row, const int *dst_row,
                             int D, int H, hipStream_t st) {
    (void)hipGetLastError();
    const int xv = D / 8, kvv = H * 1024, nv = 2 * xv + kvv;
    const int per = kCommitThreads * kCommitVecs;
    const dim3 grid((nv + per - 1) / per, n, layers), block(kCommitThreads);
    hipLaunchKernelGGL(cache_rows_kernel<kZero>, grid, block, 0, st, (const uint4 *const *)src_tbl, (uint4 *const *)dst_tbl, src_row,
                       dst_row, xv, kvv);
    return (int)hipGetLastError();
}

int cache_rows_commit_bf16(int layers, int n, const void *const *src_tbl, void *const *dst_tbl, const int *src_row, const int *dst_row,
                           int D, int H, hipStream_t st) {
    return cache_rows_launch<false>(layers, n, src_tbl, dst_tbl, src_row, dst_row, D, H, st);
}

int cache_rows_seed_bf16(int layers, int n, const void *const *src_tbl, void *const *dst_tbl, const int *src_row, const int *dst_row,
                         int D, int H, hipStream_t st) {
    return cache_rows_launch<true>(layers, n, src_tbl, dst_tbl, src_row, dst_row, D, H, st);
}

int cache_rows_retain_bf16(int layers, int slots, const void *const *src_tbl, void *const *dst_tbl, const unsigned char *live,
                           unsigned char *armed, const int *retain_row, int *ticket, int D, int H, hipStream_t st) {
    (void)hipGetLastError();
    const int xv = D / 8, kvv = H * 1024, nv = 2 * xv + kvv;
    const int per = kCommitThreads * kCommitVecs;
    const dim3 grid((nv + per - 1) / per, slots, layers), block(kCommitThreads);
    hipLaunchKernelGGL(cache_rows_retain_kernel, grid, block, 0, st, (const uint4 *const *)src_tbl, (uint4 *const *)dst_tbl, live, armed,
                       retain_row, ticket, xv, kvv);
    return (int)hipGetLastError();
}

}  // namespace rwkv7
