// fg_pack.hip -- the fired rows as packed BinaryRowData rows (fg_fired_packed).
//
// The output half of fg_add_rows: rows [first, first + n) of the columns a call handed back,
// transposed into the fixed-length parts of BinaryRowData rows (BinaryRowData.java:68-76, the
// layout of fg_row_batch) -- word 0 the bit set (RowKind INSERT in byte 0, bit 8 + f: field f is
// NULL; at most 11 fields, so always 8 bytes), then 8 bytes per field:
//   [key,] agg[0] .. agg[num_aggs - 1], window_start, window_end.
// One launch per call. A row is W = arity + 1 words; one lane per 8-byte OUTPUT word over the flat
// word index, so the lanes of a wave store 512 consecutive bytes whatever W is (a lane per row
// would store with a stride of 8 W bytes). Every column is read in runs of contiguous elements:
// the 64 / W rows a wave covers, the neighbouring waves' rows next to them. A workgroup takes
// whole 256-word blocks, grid-strided; the block's first row and word come from one uniform 64-bit
// division, the lanes divide a 32-bit offset (< 256 + W) by the constant W.
// A NULL aggregate stores eight zero bytes (BinaryRowWriter.setNullAt): whatever the column holds
// there does not reach the row. In run mode (fg_set_fired_runs) the columns window_start /
// window_end do not exist: a window lane finds its row's run by a binary search over the call's
// run directory (run_first, uploaded once per call) -- the lanes of a wave almost always share a
// run, so the search reads the same few words.
#include <hip/hip_runtime.h>

#include "fg_kernels.h"

namespace fg {

namespace {

constexpr int kPackThreads = 256;
constexpr int kPackMaxGrid = 2048;   // workgroups; the rest is grid-strided

// the run of fired row `row`: the last r with run_first[r] <= row (run_first[0] <= row)
__device__ __forceinline__ int pack_run_of(const int64_t* run_first, int n_runs, int64_t row) {
    int lo = 0, hi = n_runs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (run_first[mid] <= row) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// W: words per row; KEY: the key is field 0
template <int W, int KEY>
__global__ __launch_bounds__(kPackThreads) void k_pack_rows(PackRows p) {
    constexpr int kAggs = W - 3 - KEY;
    static_assert(kAggs >= 0 && kAggs <= kMaxAggs, "fields: [key,] aggregates, window_start, window_end");
    const unsigned long long total = (unsigned long long)p.n * W;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kPackThreads; base < total;
         base += (unsigned long long)gridDim.x * kPackThreads) {
        const unsigned long long row0 = base / W;               // (uniform)
        const uint32_t t = (uint32_t)(base - row0 * W) + threadIdx.x;
        const uint32_t dr = t / W, w = t - dr * W;
        const unsigned long long idx = base + threadIdx.x;
        if (idx >= total) break;                                 // (only in the last block)
        const long long row = p.first + (long long)(row0 + dr);  // < first + n <= the call's rows
        const unsigned long long nm = p.null_mask[row];
        unsigned long long v;
        if (w == 0) {
            v = nm << (8 + KEY);
        } else if (w >= (uint32_t)(1 + KEY + kAggs)) {           // window_start, window_end
            const bool end = w == (uint32_t)(2 + KEY + kAggs);
            if (p.n_runs > 0) {
                const int r = pack_run_of(p.run_first, p.n_runs, row);
                v = (unsigned long long)(end ? p.run_we[r] : p.run_ws[r]);
            } else {
                v = (unsigned long long)(end ? p.we[row] : p.ws[row]);
            }
        } else {
            const int64_t* col = KEY ? p.key : p.agg[0];
            bool isnull = KEY ? false : (nm & 1ull) != 0;
#pragma unroll
            for (int a = KEY ? 0 : 1; a < kAggs; a++) {
                if (w == (uint32_t)(1 + KEY + a)) {
                    col = p.agg[a];
                    isnull = ((nm >> a) & 1ull) != 0;
                }
            }
            const unsigned long long x = (unsigned long long)col[row];
            v = isnull ? 0ull : x;
        }
        p.rows[idx] = v;
    }
}

template <int W>
void pack_launch(const PackRows& p, dim3 grid, hipStream_t s) {
    if (p.key_field) {
        if constexpr (W >= 4) fg_launch(k_pack_rows<W, 1>, grid, dim3(kPackThreads), 0, s, p);
    } else {
        if constexpr (W <= 3 + kMaxAggs) fg_launch(k_pack_rows<W, 0>, grid, dim3(kPackThreads), 0, s, p);
    }
}

}  // namespace

hipError_t launch_pack_rows(const PackRows& p, hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    const int W = p.num_aggs + 3 + (p.key_field ? 1 : 0);
    if (p.num_aggs < 0 || p.num_aggs > kMaxAggs) return hipErrorInvalidValue;
    const unsigned long long blocks = ((unsigned long long)p.n * W + kPackThreads - 1) / kPackThreads;
    const dim3 grid((unsigned)(blocks < (unsigned long long)kPackMaxGrid ? blocks : kPackMaxGrid));
    switch (W) {
        case 3: pack_launch<3>(p, grid, s); break;
        case 4: pack_launch<4>(p, grid, s); break;
        case 5: pack_launch<5>(p, grid, s); break;
        case 6: pack_launch<6>(p, grid, s); break;
        case 7: pack_launch<7>(p, grid, s); break;
        case 8: pack_launch<8>(p, grid, s); break;
        case 9: pack_launch<9>(p, grid, s); break;
        case 10: pack_launch<10>(p, grid, s); break;
        case 11: pack_launch<11>(p, grid, s); break;
        case 12: pack_launch<12>(p, grid, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace fg
