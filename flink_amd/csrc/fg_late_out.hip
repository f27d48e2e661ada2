// fg_late_out.hip -- DataStream WindowedStream.sideOutputLateData on the GPU.
//
// WindowOperator.processElement (:448-456): an element skipped by all of its windows and late
// itself goes to the side output when a lateDataOutputTag is set, and only otherwise counts in
// numLateRecordsDropped. The ingest kernels implement the count alone (classify returns -1); with
// fg_set_late_output on, this pass runs ahead of them on the same device columns and appends
// the elements they will discard -- ds_dropped (fg_late.h), the decision classify and
// k_late_split take -- to the handle's late-record columns, in arrival order. The batch itself
// is left untouched.
//
// A stable stream compaction in three launches on the handle's stream, with no wait between
// workgroups and no host read:
//   k_late_out_count    one workgroup per chunk of kLateOutChunk elements: reads the rowtimes,
//                       writes the chunk's count;
//   k_late_out_scan     one workgroup: exclusive prefix of the chunk counts on top of the
//                       device-resident total of records not yet collected, total written back;
//   k_late_out_scatter  one workgroup per chunk; returns at once when its count is 0 (the common
//                       case: nothing late), else takes the predicate again, ranks with wave
//                       ballots + the waves' counts in LDS and stores key / rowtime / value /
//                       NULL flag at base + rank.
#include <hip/hip_runtime.h>

#include "fg_late.h"

namespace fg {

namespace {

constexpr int kLateOutThreads = 256;
constexpr int kLateOutWaves = kLateOutThreads / 64;
constexpr int kLateOutIters = kLateOutChunk / kLateOutThreads;
constexpr int kLateOutScanThreads = 1024;
static_assert((kLateOutChunk & (kLateOutChunk - 1)) == 0 && kLateOutChunk <= 16384, "chunk: a power of two <= 16,384");
static_assert(kLateOutChunk % kLateOutThreads == 0, "whole iterations per chunk");

__device__ __forceinline__ bool late_out_pred(const LateOut& p, int64_t i) {
    return i < p.n && ds_dropped(p.w, p.ts[i], p.progress, p.late_wm, p.lateness, p.purging != 0);
}

}  // namespace

__global__ __launch_bounds__(kLateOutThreads) void k_late_out_count(LateOut p) {
    __shared__ uint32_t s_wave[kLateOutWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * kLateOutChunk;
    uint32_t cnt = 0;   // wave-uniform
    for (int it = 0; it < kLateOutIters; it++) {
        const int64_t i = c0 + (int64_t)it * kLateOutThreads + threadIdx.x;
        cnt += (uint32_t)__popcll(__ballot(late_out_pred(p, i)));
    }
    if (lane == 0) s_wave[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kLateOutWaves; w++) t += s_wave[w];
        p.chunk_cnt[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kLateOutScanThreads) void k_late_out_scan(LateOut p) {
    __shared__ unsigned long long s_wave[kLateOutScanThreads / 64];
    __shared__ unsigned long long s_run;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_run = p.total[0];
    __syncthreads();
    for (int c0 = 0; c0 < p.n_chunks; c0 += kLateOutScanThreads) {
        const int c = c0 + (int)threadIdx.x;
        const unsigned long long v = c < p.n_chunks ? p.chunk_cnt[c] : 0ull;
        unsigned long long x = v;
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        unsigned long long base = s_run;
        for (int w = 0; w < wave; w++) base += s_wave[w];
        if (c < p.n_chunks) p.chunk_base[c] = base + x - v;
        __syncthreads();
        if (threadIdx.x == kLateOutScanThreads - 1) s_run = base + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) p.total[0] = s_run;
}

__global__ __launch_bounds__(kLateOutThreads) void k_late_out_scatter(LateOut p) {
    if (p.chunk_cnt[blockIdx.x] == 0) return;   // (uniform over the workgroup: before any barrier)
    __shared__ uint32_t s_wave[kLateOutWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * kLateOutChunk;
    unsigned long long at0 = p.chunk_base[blockIdx.x];   // position of the iteration's first late record
    for (int it = 0; it < kLateOutIters; it++) {
        const int64_t i = c0 + (int64_t)it * kLateOutThreads + threadIdx.x;
        const bool late = late_out_pred(p, i);
        const unsigned long long m = __ballot(late);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int w = 0; w < kLateOutWaves; w++) {
            const uint32_t t = s_wave[w];
            before += w < wave ? t : 0u;
            all += t;
        }
        if (late) {
            const unsigned long long at = at0 + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (at < (unsigned long long)p.cap) {
                p.o_key[at] = p.key[i];
                p.o_ts[at] = p.ts[i];
                if (p.o_val) p.o_val[at] = p.val[i];
                p.o_null[at] = p.vnull ? p.vnull[i] : (uint8_t)0;
            } else {
                atomicAdd(&p.total[1], 1ull);   // (the host sizes the columns for every element: never)
            }
        }
        at0 += all;
        __syncthreads();
    }
}

hipError_t launch_late_out(const LateOut& p, hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    fg_launch(k_late_out_count, dim3((unsigned)p.n_chunks), dim3(kLateOutThreads), 0, s, p);
    fg_launch(k_late_out_scan, dim3(1), dim3(kLateOutScanThreads), 0, s, p);
    fg_launch(k_late_out_scatter, dim3((unsigned)p.n_chunks), dim3(kLateOutThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace fg
