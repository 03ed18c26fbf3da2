// rwkvtts_amd/csrc/buf_digest.hip -- position-sensitive 64-bit digest of a device buffer of 32-bit words, in exact integer
// arithmetic (rwkvtts_amd/trainer.py: checkpoints that can prove after loading that what is in HBM is what was in HBM at save
// time, the replica-divergence check, bit-identity tests).  For a buffer w[0..n) whose first word has GLOBAL index `first`:
//     x_i  = (uint64)w[i] + (first + i + 1) * 0x9E3779B97F4A7C15
//     x_i ^= x_i >> 30;  x_i *= 0xBF58476D1CE4E5B9;  x_i ^= x_i >> 27;  x_i *= 0x94D049BB133111EB;  x_i ^= x_i >> 31
//     digest = sum_i x_i                                                            (everything mod 2^64)
// i.e. the splitmix64 finaliser of every word keyed by its global position, under a wrapping sum: the digest of a buffer is the
// wrapping sum of the digests of its slabs, each taken with its own `first` (sharded checkpoints, the cross-rank check).
// The buffer is only read.  4 bytes read per word against two 64-bit multiplies and three shift-xors: about as much integer VALU
// work as the load delivers bytes for (DESIGN.md section 6.2 has the measured rate).
// The snapshot form (rwkv7_buf_snapshot_digest_u32, the non-blocking checkpoints) is the same pass with one more instruction per
// piece: the 16 bytes a thread holds are stored to a second buffer before they are mixed, so the copy and the digest of the copy
// cost one read and one write of the data, and the digest is of the words that were written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.h"

namespace rwkv7 {

constexpr int kDigestTile = 8192;   // words per workgroup of stage 1: FIXED, as in grad_ops.hip (rwkv7_buf_digest_workspace_bytes)
constexpr int kDigestPieces = kDigestTile / (256 * 4);   // 16-byte pieces per thread: 8

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// Stage 1: workgroup b digests words [b * 8192, min(n, (b + 1) * 8192)).  Thread t takes the 16-byte pieces t, t + 256, ...,
// t + 7 * 256 of the tile (a wave reads 1 KiB contiguous per load), all eight loads in flight before the first multiply.
// n % 4 == 0, so a piece is inside the buffer or outside it as a whole; a piece outside contributes NOTHING (the digest of a
// zero word is not zero).  The key of a piece's first word costs one 64-bit multiply, the next three are one add each.
// kSnapshot: every piece inside the buffer is also stored to dst + (its offset in w), from the registers it is mixed from; a
// piece outside is not stored, so dst is never written at or behind word n.  dst does not overlap w (checked by the C entry).
template <bool kSnapshot>
__global__ __launch_bounds__(256) void buf_digest_tiles_kernel(long n, uint64_t first, const uint32_t *__restrict__ w,
                                                               uint32_t *__restrict__ dst, uint64_t *__restrict__ partials) {
    __shared__ uint64_t sh[4];
    constexpr uint64_t G = 0x9E3779B97F4A7C15ull;
    const long base = (long)blockIdx.x * kDigestTile;
    uint4 r[kDigestPieces];
#pragma unroll
    for (int j = 0; j < kDigestPieces; j++) {
        const long e = base + (long)(j * 256 + (int)threadIdx.x) * 4;
        r[j] = e < n ? *reinterpret_cast<const uint4 *>(w + e) : make_uint4(0u, 0u, 0u, 0u);
    }
    uint64_t s = 0;
#pragma unroll
    for (int j = 0; j < kDigestPieces; j++) {
        const long e = base + (long)(j * 256 + (int)threadIdx.x) * 4;
        if (e < n) {
            if constexpr (kSnapshot) *reinterpret_cast<uint4 *>(dst + e) = r[j];
            const uint64_t k0 = (first + (uint64_t)e + 1ull) * G;
            s += mix64((uint64_t)r[j].x + k0);
            s += mix64((uint64_t)r[j].y + (k0 + G));
            s += mix64((uint64_t)r[j].z + (k0 + 2ull * G));
            s += mix64((uint64_t)r[j].w + (k0 + 3ull * G));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {   // wrapping adds commute: any order gives the same word
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)s, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(s >> 32), d, 64);
        s += ((uint64_t)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// Stage 2, one workgroup: thread t adds partials t, t + 256, ..., then a tree over the 256 threads.  ntiles == 0 (an empty
// buffer) leaves out[0] as it is when accumulating and stores 0 otherwise.
__global__ __launch_bounds__(256) void buf_digest_final_kernel(long ntiles, const uint64_t *__restrict__ partials, uint64_t *__restrict__ out,
                                                               int accumulate) {
    __shared__ uint64_t sh[256];
    uint64_t s = 0;
    for (long i = threadIdx.x; i < ntiles; i += 256) s += partials[i];
    sh[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = accumulate ? out[0] + sh[0] : sh[0];
}

long buf_digest_tiles(long n_words) { return (n_words + kDigestTile - 1) / kDigestTile; }

// dst == nullptr: digest only; otherwise dst[0..n_words) = buf[0..n_words) as well.  Same grid, same partials, same stage 2.
int buf_digest_u32(long n_words, long first_index, const void *buf, void *dst, unsigned long long *partials, unsigned long long *out,
                   int accumulate, hipStream_t st) {
    (void)hipGetLastError();
    const long ntiles = buf_digest_tiles(n_words);
    if (ntiles > 0) {
        if (dst != nullptr)
            hipLaunchKernelGGL(buf_digest_tiles_kernel<true>, dim3((unsigned)ntiles), dim3(256), 0, st, n_words, (uint64_t)first_index,
                               (const uint32_t *)buf, (uint32_t *)dst, (uint64_t *)partials);
        else
            hipLaunchKernelGGL(buf_digest_tiles_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, st, n_words, (uint64_t)first_index,
                               (const uint32_t *)buf, (uint32_t *)nullptr, (uint64_t *)partials);
    }
    hipLaunchKernelGGL(buf_digest_final_kernel, dim3(1), dim3(256), 0, st, ntiles, (const uint64_t *)partials, (uint64_t *)out, accumulate);
    return (int)hipGetLastError();
}

}  // namespace rwkv7
