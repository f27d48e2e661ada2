// fg_rows_scan.h -- the 64-bit offsets of packed rows: what fg_key_dict_rows (fg_keydict.hip) and
// fg_key_dict_project (fg_keyproj.hip) share. Rows are taken in blocks of kScanThreads; a lengths
// kernel of the caller's writes every row's length and each block's padded bytes (sums), then
// k_rows_scan_sums (one workgroup: the exclusive scan of the block sums, the total) and
// k_rows_offsets (offsets[0..n)) give the offsets. The host reads RowsCtr once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fg {

constexpr int kScanThreads = 256;   // rows per scan block = threads per workgroup

struct RowsCtr {
    unsigned long long total;      // padded bytes of every row = offsets[n]
    unsigned long long bad;        // rows the lengths kernel refused
    unsigned long long bad_first;  // lowest index of such a row (~0: none)
};

__host__ __device__ __forceinline__ uint64_t padded8(int32_t len) { return ((uint64_t)(uint32_t)len + 7) & ~7ull; }

// exclusive scan of v over the workgroup (s_wave: kScanThreads / 64 words, reusable on return)
__device__ __forceinline__ uint64_t block_exclusive_scan_u64(uint64_t v, uint64_t* s_wave, uint64_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t x = v;   // inclusive scan over the wave
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    uint64_t base = 0, t = 0;
#pragma unroll
    for (int k = 0; k < kScanThreads / 64; k++) {
        const uint64_t w = s_wave[k];
        if (k < wave) base += w;
        t += w;
    }
    __syncthreads();
    *total = t;
    return base + x - v;
}

// one workgroup: sums[0..nb) -> their exclusive scan, the total to rc->total and off_out[n]
static __global__ __launch_bounds__(kScanThreads) void k_rows_scan_sums(uint64_t* sums, int64_t nb, RowsCtr* rc,
                                                                        int64_t* off_out, int64_t n) {
    __shared__ uint64_t s_wave[kScanThreads / 64];
    uint64_t carry = 0;   // (the same in every thread)
    for (int64_t b0 = 0; b0 < nb; b0 += kScanThreads) {
        const int64_t b = b0 + threadIdx.x;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan_u64(b < nb ? sums[b] : 0ull, s_wave, &total);
        if (b < nb) sums[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        rc->total = carry;
        off_out[n] = (int64_t)carry;
    }
}

static __global__ __launch_bounds__(kScanThreads) void k_rows_offsets(int64_t n, const int32_t* len_in, const uint64_t* sums,
                                                                      int64_t* off_out) {
    __shared__ uint64_t s_wave[kScanThreads / 64];
    const int64_t i = (int64_t)blockIdx.x * kScanThreads + threadIdx.x;
    const int32_t len = i < n ? len_in[i] : 0;
    uint64_t total;
    const uint64_t ex = block_exclusive_scan_u64(len > 0 ? padded8(len) : 0ull, s_wave, &total);
    if (i < n) off_out[i] = (int64_t)(sums[blockIdx.x] + ex);
}

}  // namespace fg
