// fg_topn.hip -- Window Top-N over the fired rows (fg_set_fired_topn).
//
// ROW_NUMBER() OVER (PARTITION BY window_start, window_end ORDER BY agg DESC) <= n directly above a
// window aggregate (the reference's WindowRankOperator): of the rows a call hands back, every window
// keeps the n that rank first. A post-pass over the output columns of the fires, on the handle's
// stream, in three launches whatever the number of windows:
//   k_topn_cand    one workgroup per chunk of at most kTopnChunk rows of ONE window (the host cuts
//                  the chunks from the run directory): streams the order column, its null_mask byte
//                  and the key -- 17 B per row, nothing else of a losing row is read -- and writes the
//                  chunk's best <= n rows as (composite, row index) candidates;
//   k_topn_merge   one workgroup per group of at most kTopnGroup candidate lists of one window: the
//                  same selection over the lists, one list of <= n candidates out;
//   k_topn_final   one workgroup per window: selects over the window's group lists, sorts, and
//                  gathers every output column of the winners into the second column set at the
//                  window's offset (a host prefix over min(n, rows of the window): no counter is
//                  shared between windows, positions are deterministic).
// The selection (topn_select) is the same code in all three: a workgroup keeps its candidates in an
// LDS buffer of kTopnBuf entries, appended by wave ballots; when a round's candidates do not fit (or
// early, to get a threshold) it sorts the buffer (bitonic, on the composite), keeps the first n and
// takes the n-th as the threshold: from then on an item that does not rank before the threshold is
// rejected by one compare.
//
// The composite is a total order in which "smaller ranks first": (NULL side, value, key, row). The
// value word is the aggregate mapped to an ascending unsigned (BIGINT: sign flipped; DOUBLE:
// Double.compare's order on doubleToLongBits -- -0.0 below +0.0, every NaN the canonical NaN above
// +inf), complemented for a descending order; a NULL aggregate is the smallest value (last when
// descending, first when ascending: the flag in bit 31 of the row word); ties go to the smaller
// signed key. A window holds a key once, so no two rows of a window compare equal.
#include <hip/hip_runtime.h>

#include "fg_kernels.h"

namespace fg {

namespace {

constexpr int kTopnThreads = 256;
constexpr int kTopnWaves = kTopnThreads / 64;
constexpr int kTopnU = 4;                              // items per thread per round
constexpr int kTopnStep = kTopnU * kTopnThreads;       // items per round
constexpr int kTopnBuf = 2048;                         // LDS candidates: 2048 x 20 B = 40 KiB
static_assert(kTopnBuf - kTopnStep >= kTopnMax, "a trimmed buffer takes one more round");
static_assert((kTopnBuf & (kTopnBuf - 1)) == 0, "bitonic sort: a power of two");
static_assert(kTopnChunk % kTopnStep == 0, "whole rounds per full chunk");

constexpr unsigned long long kSign = 1ull << 63;

struct Ent {
    unsigned long long hi, lo;
    uint32_t ix;   // bit 31: the NULL side (0 ranks first), bits 0-30: the row
};

__device__ __forceinline__ bool ent_less(const Ent& a, const Ent& b) {
    const uint32_t fa = a.ix >> 31, fb = b.ix >> 31;
    if (fa != fb) return fa < fb;
    if (a.hi != b.hi) return a.hi < b.hi;
    if (a.lo != b.lo) return a.lo < b.lo;
    return a.ix < b.ix;
}

struct SelLds {
    unsigned long long hi[kTopnBuf];
    unsigned long long lo[kTopnBuf];
    uint32_t ix[kTopnBuf];
    uint32_t wave[1][kTopnWaves];
};

__device__ __forceinline__ Ent lds_get(const SelLds& s, int i) { return Ent{s.hi[i], s.lo[i], s.ix[i]}; }
__device__ __forceinline__ void lds_put(SelLds& s, int i, const Ent& e) {
    s.hi[i] = e.hi;
    s.lo[i] = e.lo;
    s.ix[i] = e.ix;
}

// sorts the buffer's first cnt entries (all waves have stored them: a barrier precedes the call's
// reads) and returns min(cnt, n): the entries that stay, in rank order. Ends with a barrier.
__device__ int topn_trim(SelLds& s, int cnt, int n) {
    int P = 2;
    while (P < cnt) P <<= 1;
    for (int i = cnt + (int)threadIdx.x; i < P; i += kTopnThreads) lds_put(s, i, Ent{~0ull, ~0ull, ~0u});
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += kTopnThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const bool up = (i & k) == 0;
                const Ent a = lds_get(s, i), b = lds_get(s, l);
                if (ent_less(b, a) == up) {
                    lds_put(s, i, b);
                    lds_put(s, l, a);
                }
            }
            __syncthreads();
        }
    }
    return cnt < n ? cnt : n;
}

// The selection over items [0, total): fetch(v, e) says whether item v exists and fills its entry.
// Returns the number of entries kept (<= n), sorted, in s[0 ..). All threads of the workgroup call it.
// A round takes kTopnStep items into registers, tests them against the threshold and appends the
// ones that pass. The buffer is trimmed (sorted, cut to n, the n-th entry the new threshold) when a
// round's candidates would not fit -- they are then tested again, against the new threshold, so they
// fit -- and early, once it holds kTopnEarly(n) entries: a small sort that buys a threshold (or a
// tighter one) for the rows still to come.
__device__ __forceinline__ int topn_early(int n) { return 4 * n > 512 ? 4 * n : 512; }
template <class Fetch>
__device__ int topn_select(SelLds& s, long long total, int n, Fetch fetch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int early = topn_early(n);
    int cnt = 0;          // uniform over the workgroup
    bool have = false;    // a threshold is known: the n-th best so far
    Ent thr{};
    for (long long v0 = 0; v0 < total; v0 += kTopnStep) {
        Ent e[kTopnU];
        bool ok[kTopnU];
        unsigned long long m[kTopnU];
#pragma unroll
        for (int u = 0; u < kTopnU; u++) {
            const long long v = v0 + u * kTopnThreads + (long long)threadIdx.x;
            ok[u] = v < total && fetch(v, e[u]);
        }
        uint32_t at = 0, all = 0;
        for (int pass = 0; pass < 2; pass++) {   // (the second pass only after a trim for room)
            uint32_t mine = 0;
#pragma unroll
            for (int u = 0; u < kTopnU; u++) {
                m[u] = __ballot(ok[u] && (!have || ent_less(e[u], thr)));
                mine += (uint32_t)__popcll(m[u]);
            }
            if (lane == 0) s.wave[0][wave] = mine;
            __syncthreads();   // (also: the stores of the round before are complete)
            at = (uint32_t)cnt;
            all = 0;
            for (int w = 0; w < kTopnWaves; w++) {
                const uint32_t t = s.wave[0][w];
                at += w < wave ? t : 0u;
                all += t;
            }
            if (cnt + (int)all <= kTopnBuf) break;
            // no room: cnt > kTopnBuf - kTopnStep >= n, so the trim leaves n entries and a threshold
            __syncthreads();   // (every wave has read the counts before they are written again)
            cnt = topn_trim(s, cnt, n);
            thr = lds_get(s, n - 1);
            have = true;
        }
#pragma unroll
        for (int u = 0; u < kTopnU; u++) {
            if ((m[u] >> lane) & 1ull) lds_put(s, (int)(at + (uint32_t)__popcll(m[u] & ((1ull << lane) - 1ull))), e[u]);
            at += (uint32_t)__popcll(m[u]);
        }
        cnt += (int)all;
        __syncthreads();   // (the counts are read, the entries stored)
        if (cnt >= early && cnt > n) {
            cnt = topn_trim(s, cnt, n);
            thr = lds_get(s, n - 1);   // (the next stores go to s[n ..])
            have = true;
        }
    }
    return topn_trim(s, cnt, n);
}

__device__ __forceinline__ Ent make_ent(const Topn& p, long long row) {
    const bool isnull = (p.null_mask[row] >> p.agg_index) & 1;
    const long long raw = p.ord[row];
    long long b = raw;
    if (p.f64) {   // Double.compare: doubleToLongBits, then the sign-magnitude order
        b = (b & 0x7FFFFFFFFFFFFFFFll) > 0x7FF0000000000000ll ? 0x7FF8000000000000ll : b;
        b = b >= 0 ? b : b ^ 0x7FFFFFFFFFFFFFFFll;
    }
    const unsigned long long asc = (unsigned long long)b ^ kSign;
    Ent e;
    e.hi = isnull ? 0ull : (p.descending ? ~asc : asc);
    e.lo = (unsigned long long)p.key[row] ^ kSign;
    const uint32_t side = p.descending ? (isnull ? 1u : 0u) : (isnull ? 0u : 1u);
    e.ix = (uint32_t)row | (side << 31);
    return e;
}

__device__ __forceinline__ void list_store(const TopnLists& l, long long list, int n, int cnt, const SelLds& s) {
    for (int j = threadIdx.x; j < cnt; j += kTopnThreads) {
        const long long o = list * n + j;
        l.hi[o] = s.hi[j];
        l.lo[o] = s.lo[j];
        l.ix[o] = s.ix[j];
    }
    if (threadIdx.x == 0) l.cnt[list] = (uint32_t)cnt;
}

// item v of the lists [l0, ..): entry v % n of list l0 + v / n, if the list holds that many
struct ListFetch {
    TopnLists l;
    long long l0;
    int n;
    __device__ __forceinline__ bool operator()(long long v, Ent& e) const {
        const uint32_t q = (uint32_t)v / (uint32_t)n;   // (v < lists x n <= 2^17 x 2^10)
        const long long list = l0 + q;
        const uint32_t j = (uint32_t)v - q * (uint32_t)n;
        if (j >= l.cnt[list]) return false;
        const long long o = list * n + j;
        e = Ent{l.hi[o], l.lo[o], l.ix[o]};
        return true;
    }
};

}  // namespace

__global__ __launch_bounds__(kTopnThreads) void k_topn_cand(Topn p) {
    __shared__ SelLds s;
    const TopnSeg seg = p.seg[blockIdx.x];
    const int cnt = topn_select(s, (long long)seg.rows, p.n, [&](long long v, Ent& e) {
        e = make_ent(p, seg.first + v);
        return true;
    });
    list_store(p.cand, blockIdx.x, p.n, cnt, s);
}

__global__ __launch_bounds__(kTopnThreads) void k_topn_merge(Topn p) {
    __shared__ SelLds s;
    const TopnRange g = p.group[blockIdx.x];   // the group's chunk lists
    const int cnt = topn_select(s, (long long)(g.end - g.begin) * p.n, p.n, ListFetch{p.cand, g.begin, p.n});
    list_store(p.merged, blockIdx.x, p.n, cnt, s);
}

__global__ __launch_bounds__(kTopnThreads) void k_topn_final(Topn p) {
    __shared__ SelLds s;
    const TopnWin w = p.win[blockIdx.x];       // the window's group lists, its rows in the output
    int cnt = topn_select(s, (long long)(w.end - w.begin) * p.n, p.n, ListFetch{p.merged, w.begin, p.n});
    if (cnt != w.out_rows) {   // (the host's min(n, rows of the window); never)
        if (threadIdx.x == 0) p.err[0] = 1ull;
        cnt = cnt < w.out_rows ? cnt : w.out_rows;
    }
    for (int j = threadIdx.x; j < cnt; j += kTopnThreads) {
        const long long r = (long long)(s.ix[j] & 0x7FFFFFFFu), o = w.out_first + j;
        p.o_key[o] = p.key[r];
        p.o_null[o] = p.null_mask[r];
#pragma unroll
        for (int a = 0; a < kMaxAggs; a++)
            if (a < p.num_aggs) p.o_agg[a][o] = p.agg[a][r];
        if (p.o_ws) p.o_ws[o] = p.ws[r];
        if (p.o_we) p.o_we[o] = p.we[r];
        if (p.o_rt) p.o_rt[o] = p.rt[r];
    }
}

hipError_t launch_topn(const Topn& p, hipStream_t s) {
    if (p.n_chunks <= 0) return hipSuccess;
    fg_launch(k_topn_cand, dim3((unsigned)p.n_chunks), dim3(kTopnThreads), 0, s, p);
    fg_launch(k_topn_merge, dim3((unsigned)p.n_groups), dim3(kTopnThreads), 0, s, p);
    fg_launch(k_topn_final, dim3((unsigned)p.n_windows), dim3(kTopnThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace fg
