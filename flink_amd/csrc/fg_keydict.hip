// fg_keydict.hip -- grouping keys of any type: a GPU-resident dictionary of serialized key
// rows (BinaryRowData bytes), for the C-ABI fg_key_dict_* of include/flinkgpu.h.
//
// The reference groups by the key row the BinaryRowDataKeySelector projects
// (TR/keyselector/BinaryRowDataKeySelector.java:43-50): key identity is byte equality of the
// row (BinarySection.equals, TC/data/binary/BinarySection.java:62-73) and its hash is
// MurmurHashUtils.hashBytesByWords over the row's bytes, seed 42 (BinarySection.java:76-78 ->
// BinarySegmentUtils.hash -> MurmurHashUtils.java:92-96,131-170), which KeyGroupStreamPartitioner
// turns into a key group (KeyGroupRangeAssignment.java:63-77). The window engine aggregates
// 64-bit keys; this dictionary interns each distinct key row once and hands out an id
// (ordinal << kg_bits | key group): equal rows get equal ids, distinct rows distinct ids, so the
// aggregation by id is the aggregation by key row, and the id carries the row's key group
// (FG_KEYHASH_DICT_ID routes by it).
//
// Layout in HBM: an open-addressing table of `cap` 64-B slots -- one memory line -- {tag u64
// (a 64-bit hash of the row, 0 = empty), loc u64 (where the row's arena entry lives, and its
// length), id i64, the row's first 40 bytes}; the arena holds one entry per id, [id i64][row
// bytes padded to 8]. A steady-state lookup is one random access: the slot holds the tag, the
// id and the bytes to compare (rows of up to 40 bytes -- BinaryRowData key rows of a short
// string and a fixed field or two). One intern call: k_dict_lookup over every row (both hashes
// in one pass over its words, the slot of its tag, the byte comparison, the id; rows whose tag
// is not in the table go to a miss list -- none in a steady state), then over the misses only,
// in chunks the table has room for: k_dict_probe (the slot of its tag or a CAS claiming an
// empty one), k_dict_assign (the first claimer of a new slot allocates the id and writes the
// slot and the entry) and k_dict_verify (the byte comparison of the rows whose slot is new).
// Reservations (miss and pending lists, ids, arena bytes) take one atomic per wave. A 64-bit
// tag shared by distinct rows fails the comparison and is resolved on the host, so ids stay
// exact whatever the hash. The way out is fg_key_dict_rows: the packed key rows of ids, gathered
// by k_rows_* (lengths and a 64-bit scan for the offsets, one host read, then a copy balanced by
// bytes) -- fired rows, checkpoints and a rescale's re-intern copy those rows, never an arena range.
// The keyed two-phase edge uses both ends: fg_partition_keyed_by_owner groups rows keyed by ids by
// owner and gathers their key rows in the grouped order (the same k_rows_* pipeline on the caller's
// stream, k_owner_byte_counts for the bytes per owner), and keydict_intern_packed (fg_keydict.h)
// checks and scans the lengths an owner received (k_recv_lengths) and interns the rows.
// The key rows themselves can be made on the GPU: fg_key_dict_project / fg_key_dict_intern_fields
// project them from packed BinaryRowData records (the key selector; kernels in fg_keyproj.hip, the
// offsets by the same scan, fg_rows_scan.h) and intern them from the dictionary's scratch.
// An entry lasts until fg_key_dict_retain retires it: the caller lists the ids that still hold
// state, every other entry leaves the table and the arena (k_retain_*), and k_dict_assign hands
// the retired ordinals out again before it issues a fresh one -- the dictionary is bounded by the
// keys alive at once, not by the keys ever seen.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/flinkgpu.h"
#include "fg_kernels.h"
#include "fg_keydict.h"
#include "fg_keyproj.h"
#include "fg_rows_scan.h"
#include "fg_window.h"

using namespace fg;

namespace {

constexpr int kDictThreads = 256;
#ifndef FG_DICT_GROW
#define FG_DICT_GROW 4   // table rebuilt at FG_DICT_GROW x (ids + 1M) slots (>= 2: room for a chunk)
#endif
static_assert(FG_DICT_GROW >= 2, "FG_DICT_GROW: the table must stay at most half full after a rebuild");
#ifndef FG_DICT_INIT
#define FG_DICT_INIT 2   // slots at open: FG_DICT_INIT x expected keys, rounded up to a power of two
#endif
// id = ordinal << kg_bits | key group, kg_bits = dict_kg_bits(max parallelism) (7 at Flink's
// default 128): ids stay below 2^31 for 16.7M keys, so the window engine stages them as narrow
// 32-bit keys (fg_window.h key_group_of reads the key group back from the low bits)

__host__ __device__ __forceinline__ uint32_t load_u32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// MurmurHashUtils.hashBytesByWords(segment, offset, len) (MurmurHashUtils.java:92-96,131-141,
// 143-161): little-endian 4-byte words (MemorySegment.getInt is native order), seed 42
__host__ __device__ __forceinline__ int32_t binaryrow_hash_bytes(const uint8_t* p, int32_t len) {
    uint32_t h1 = 42u;
    for (int32_t i = 0; i < len; i += 4) h1 = mix_h1(h1, mix_k1(load_u32(p + i)));
    return (int32_t)fmix32(h1 ^ (uint32_t)len);
}

constexpr uint64_t kNoLoc = ~0ull;   // a slot whose entry is not written yet

// Table slot (one 64-B line): the row's 64-bit tag, where its entry lives in the arena (entry
// offset << 24 | row length), its id and its first kSlotWords 4-byte words (zero padded). An
// arena entry is [id i64][row bytes, padded to 8].
constexpr int kSlotWords = 10;
struct alignas(64) Slot {
    unsigned long long tag;   // 0: empty
    unsigned long long loc;   // kNoLoc until the entry (and id, row words) are written
    long long id;
    uint32_t row[kSlotWords];
};
static_assert(sizeof(Slot) == 64, "one slot per 64-B line");
__host__ __device__ __forceinline__ uint64_t loc_of(uint64_t entry, int32_t len) { return entry << 24 | (uint32_t)len; }

struct DictDev {
    Slot* slots;         // [cap]
    uint32_t* slot_row;  // [cap] first claimer of a new slot in this call
    int64_t* ent_off;    // [ids] arena offset of the id's row bytes (its entry + 8)
    int32_t* ent_len;    // [ids]
    uint64_t* ent_tag;   // [ids] tag (0: resolved on the host, not in the table)
    uint8_t* arena;
    unsigned long long* counters;   // [0] ordinals issued, [1] arena bytes, [2] collisions, [3] bad rows, [4] pending
                                    // rows, [5] entry bytes of the lookup's misses, [6] lookup misses, [7] free ordinals taken
    const int64_t* free_ord;   // [nfree] ordinals a retain retired, ascending: reused before a fresh one is issued
    uint64_t nfree;      // (0: every new key takes a fresh ordinal)
    uint64_t mask;       // cap - 1
    int32_t kg_bits;     // id = ordinal << kg_bits | key group
};

// one atomic per wave: lane-exclusive offsets of `amount` (0 for a lane that takes nothing)
// reserved from *ctr; every lane of the wave must call it (inactive lanes count as 0)
__device__ __forceinline__ unsigned long long wave_reserve(unsigned long long* ctr, uint32_t amount) {
    const int lane = threadIdx.x & 63;
    uint32_t x = amount;   // inclusive scan over the wave
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    const uint32_t total = __shfl(x, 63);
    unsigned long long base = 0;
    if (lane == 63 && total) base = atomicAdd(ctr, (unsigned long long)total);
    base = __shfl(base, 63);
    return base + x - amount;
}

struct RowsIn {
    const uint8_t* bytes;   // 4-byte aligned; every row at a multiple of 4, of 4-byte words
    const int64_t* off;
    const int32_t* len;
    const uint32_t* idx;    // rows idx[0..n) of off / len (the miss list), or null: rows 0..n
    int64_t n;
    int64_t nbytes;
    int32_t max_p;
    int32_t tag_bits;
    int32_t check;          // device rows: k_dict_lookup checks them (bad rows -> counters[3])
};

// arena bytes an entry of a row of `len` bytes takes: [id i64][row bytes, padded to 8]
__host__ __device__ __forceinline__ uint64_t entry_bytes(int32_t len) { return 8 + (((uint64_t)len + 7) & ~7ull); }

// Both hashes of a row in one pass over its 4-byte words: the Flink hash (hashBytesByWords,
// seed 42) and the table's own 64-bit tag (independent of it: equal Flink hashes are common at
// 10M keys; equal tags are ~1e-5 there, and resolved exactly anyway).
__device__ __forceinline__ void row_hashes(const uint32_t* w, int32_t len, int tag_bits, uint64_t* tag, int32_t* fh) {
    uint32_t h1 = 42u;
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)(uint32_t)len * 0xff51afd7ed558ccdull;
    const int32_t nw = len >> 2;
    int32_t k = 0;
    for (; k + 2 <= nw; k += 2) {
        const uint32_t a = w[k], b = w[k + 1];
        h1 = mix_h1(mix_h1(h1, mix_k1(a)), mix_k1(b));
        h = fmix64(h ^ ((uint64_t)a | (uint64_t)b << 32)) + 0x632BE59BD9B4E019ull;
    }
    if (k < nw) {
        const uint32_t a = w[k];
        h1 = mix_h1(h1, mix_k1(a));
        h = fmix64(h ^ (uint64_t)a ^ 0xA0761D6478BD642Full);
    }
    h = fmix64(h);
    if (tag_bits < 64) h &= (1ull << tag_bits) - 1;   // diagnostic: force collisions (tests)
    *tag = h ? h : 1;
    *fh = (int32_t)fmix32(h1 ^ (uint32_t)len);
}

// the id of the entry at `loc` if its row equals the row at w, else -1
__device__ __forceinline__ int64_t entry_id_if_equal(const DictDev& d, uint64_t loc, const uint32_t* w, int32_t len) {
    if ((int32_t)(loc & 0xFFFFFF) != len) return -1;
    const uint8_t* e = d.arena + (loc >> 24);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(e + 8);
    bool eq = true;
    for (int32_t k = 0; eq && k < (len >> 2); k++) eq = w[k] == q[k];
    return eq ? *reinterpret_cast<const int64_t*>(e) : -1;
}

// Rows of up to kRegWords words (BinaryRowData key rows of one or two fixed fields and a short
// string: 16-32 bytes) are read once into registers -- 8-byte loads when the row is 8-byte
// aligned -- and hashed and compared from there; longer rows take the word loops above.
constexpr int kRegWords = 8;
__device__ __forceinline__ void row_words(const uint8_t* p, int32_t len, uint32_t (&r)[kRegWords]) {
    const int32_t nw = len >> 2;
    if (((uintptr_t)p & 15) == 0 && nw == kRegWords) {   // the common 32-B row, 16-B aligned
        const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 16);
        r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
        r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
        return;
    }
    const bool a8 = ((uintptr_t)p & 7) == 0;
#pragma unroll
    for (int k = 0; k < kRegWords; k += 2) {
        r[k] = r[k + 1] = 0;
        if (a8 && k + 2 <= nw) {
            const uint2 v = *reinterpret_cast<const uint2*>(p + 4 * k);
            r[k] = v.x;
            r[k + 1] = v.y;
        } else {
            if (k < nw) r[k] = *reinterpret_cast<const uint32_t*>(p + 4 * k);
            if (k + 1 < nw) r[k + 1] = *reinterpret_cast<const uint32_t*>(p + 4 * k + 4);
        }
    }
}
// row_hashes over register words (the same arithmetic, unrolled)
__device__ __forceinline__ void row_hashes_reg(const uint32_t (&r)[kRegWords], int32_t len, int tag_bits, uint64_t* tag,
                                               int32_t* fh) {
    uint32_t h1 = 42u;
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)(uint32_t)len * 0xff51afd7ed558ccdull;
    const int32_t nw = len >> 2;
#pragma unroll
    for (int k = 0; k < kRegWords; k += 2) {
        if (k + 2 <= nw) {
            h1 = mix_h1(mix_h1(h1, mix_k1(r[k])), mix_k1(r[k + 1]));
            h = fmix64(h ^ ((uint64_t)r[k] | (uint64_t)r[k + 1] << 32)) + 0x632BE59BD9B4E019ull;
        } else if (k < nw) {
            h1 = mix_h1(h1, mix_k1(r[k]));
            h = fmix64(h ^ (uint64_t)r[k] ^ 0xA0761D6478BD642Full);
        }
    }
    h = fmix64(h);
    if (tag_bits < 64) h &= (1ull << tag_bits) - 1;
    *tag = h ? h : 1;
    *fh = (int32_t)fmix32(h1 ^ (uint32_t)len);
}
// The id of a written slot if its row equals the row (register words r when `small`, else the
// words at w): the slot's words first, an entry's bytes past them only for rows longer than the
// slot holds; -1 for a distinct row with an equal tag.
__device__ __forceinline__ int64_t slot_id_if_equal(const DictDev& d, const Slot& sl, const uint32_t (&r)[kRegWords],
                                                    const uint32_t* w, bool small, int32_t len) {
    if ((int32_t)(sl.loc & 0xFFFFFF) != len) return -1;
    const int32_t nw = len >> 2;
    uint32_t diff = 0;
    if (small) {
        static_assert(kRegWords <= kSlotWords, "register rows fit the slot");
#pragma unroll
        for (int k = 0; k < kRegWords; k++)
            if (k < nw) diff |= r[k] ^ sl.row[k];
    } else {
        for (int k = 0; k < nw && k < kSlotWords; k++) diff |= w[k] ^ sl.row[k];
        if (diff == 0 && nw > kSlotWords) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(d.arena + (sl.loc >> 24) + 8);
            for (int k = kSlotWords; k < nw; k++) diff |= w[k] ^ q[k];
        }
    }
    return diff == 0 ? (int64_t)sl.id : -1;
}

// a slot as four 16-B loads issued together (the line is fetched once)
__device__ __forceinline__ Slot load_slot(const Slot* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1], c = q[2], e = q[3];
    Slot sl;
    sl.tag = (unsigned long long)a.x | (unsigned long long)a.y << 32;
    sl.loc = (unsigned long long)a.z | (unsigned long long)a.w << 32;
    sl.id = (long long)((unsigned long long)b.x | (unsigned long long)b.y << 32);
    sl.row[0] = b.z; sl.row[1] = b.w;
    sl.row[2] = c.x; sl.row[3] = c.y; sl.row[4] = c.z; sl.row[5] = c.w;
    sl.row[6] = e.x; sl.row[7] = e.y; sl.row[8] = e.z; sl.row[9] = e.w;
    return sl;
}

// Lookup of every row of the call (no claims): both hashes, the slot of its tag (one 64-B line
// holds tag, length, id and the row's first 40 bytes), the byte comparison, the id. A row whose
// tag is not in the table joins the miss list (counters[6]); a distinct row with an equal tag
// gets -1 (counters[2], resolved on the host). kg_out (optional) takes every row's key group.
// Each thread takes kLookupRows rows (a block's rows in kLookupRows coalesced strides) and issues
// all their slot loads before resolving any.
#ifndef FG_DICT_ROWS
#define FG_DICT_ROWS 1   // rows per thread (A/B in DESIGN.md)
#endif
constexpr int kLookupRows = FG_DICT_ROWS;
__global__ __launch_bounds__(kDictThreads) void k_dict_lookup(DictDev d, RowsIn in, int32_t* kg_out, int64_t* id_out,
                                                              uint32_t* miss) {
    constexpr int R = kLookupRows;
    const int64_t b0 = (int64_t)blockIdx.x * kDictThreads * R + threadIdx.x;
    int64_t ii[R];
    bool valid[R], small[R];
    int32_t len[R], fh[R];
    const uint8_t* rp[R];
    uint32_t r[R][kRegWords];
    uint64_t t[R], s[R];
    uint32_t nbad = 0;
#pragma unroll
    for (int u = 0; u < R; u++) {   // (every lane stays for the wave-wide reservations below)
        const int64_t i0 = b0 + (int64_t)u * kDictThreads;
        valid[u] = i0 < in.n;
        ii[u] = valid[u] ? i0 : 0;
        len[u] = in.len[ii[u]];
        const int64_t off = in.off[ii[u]];
        if (in.check && valid[u]) {   // device rows: inside the buffer, 4-byte words (BinaryRowData)
            const bool bad = len[u] < 0 || len[u] >= (1 << 24) || (len[u] & 3) != 0 || off < 0 || (off & 3) != 0 ||
                             off + len[u] > in.nbytes;
            if (bad) {
                nbad++;
                valid[u] = false;   // (not looked up; the call fails before anything is inserted)
                len[u] = 0;
            }
        }
        rp[u] = in.bytes + (valid[u] ? off : 0);
    }
    if (in.check) {
        uint32_t b = nbad;
        for (int o = 32; o > 0; o >>= 1) b += __shfl_xor(b, o);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(&d.counters[3], (unsigned long long)b);
    }
#pragma unroll
    for (int u = 0; u < R; u++) {
        small[u] = len[u] <= 4 * kRegWords;
        if (small[u]) {
            row_words(rp[u], len[u], r[u]);
            row_hashes_reg(r[u], len[u], in.tag_bits, &t[u], &fh[u]);
        } else {
#pragma unroll
            for (int k = 0; k < kRegWords; k++) r[u][k] = 0;
            row_hashes(reinterpret_cast<const uint32_t*>(rp[u]), len[u], in.tag_bits, &t[u], &fh[u]);
        }
        s[u] = fmix64(t[u]) & d.mask;
    }
    Slot sl[R];
#pragma unroll
    for (int u = 0; u < R; u++) sl[u] = load_slot(&d.slots[s[u]]);   // every row's line in flight
#pragma unroll
    for (int u = 0; u < R; u++) {
        bool found = false;
        int64_t id = -1;
        if (valid[u]) {
            Slot cur = sl[u];
            uint64_t at = s[u];
            for (;;) {   // (the home slot resolves almost every row; probing past it is rare)
                if (cur.tag == t[u]) {   // (every slot is written: no claims run beside the lookup)
                    found = true;
                    id = slot_id_if_equal(d, cur, r[u], reinterpret_cast<const uint32_t*>(rp[u]), small[u], len[u]);
                    break;
                }
                if (cur.tag == 0) break;
                at = (at + 1) & d.mask;
                cur = load_slot(&d.slots[at]);
            }
            if (kg_out) kg_out[ii[u]] = murmur_hash(fh[u]) % in.max_p;
            if (found) {
                if (id < 0) atomicAdd(&d.counters[2], 1ull);
                id_out[ii[u]] = id;
            }
        }
        const bool m = valid[u] && !found;
        const unsigned long long w = wave_reserve(&d.counters[6], m ? 1u : 0u);
        if (m) miss[w] = (uint32_t)ii[u];
        // the arena bytes the misses may take as new entries (counters[5], one atomic per wave)
        uint64_t eb = m ? entry_bytes(len[u]) : 0;
        for (int o = 32; o > 0; o >>= 1) eb += __shfl_xor(eb, o);
        if ((threadIdx.x & 63) == 0 && eb) atomicAdd(&d.counters[5], (unsigned long long)eb);
    }
}

// Pending rows (their slot is new in this call): row index, slot and key group, for
// k_dict_assign / k_dict_verify.
struct Pending {
    uint32_t* row;
    uint64_t* slot;
    int32_t* kg;
};

// One pass per row: both hashes, the slot holding the row's tag or an empty one claimed with a
// CAS (one 16-B load reads a slot's tag and entry location together), and -- when the slot's
// entry was written by an earlier call -- the byte comparison with that entry (its id, or -1: a
// distinct row with an equal tag, left to the host). Rows whose slot is new in this call (claimed
// by them or by an equal-tagged row) join the pending list (none in a steady state). kg_out
// (optional) takes every row's key group.
__global__ __launch_bounds__(kDictThreads) void k_dict_probe(DictDev d, RowsIn in, int64_t* id_out, Pending pend_out) {
    const int64_t j0 = (int64_t)blockIdx.x * kDictThreads + threadIdx.x;
    const bool valid = j0 < in.n;   // (every lane stays for the wave-wide reservation below)
    const int64_t i = in.idx ? (int64_t)in.idx[valid ? j0 : 0] : (valid ? j0 : 0);
    const int32_t len = in.len[i];
    const uint8_t* rp = in.bytes + in.off[i];
    const bool small = len <= 4 * kRegWords;
    uint32_t r[kRegWords];
    uint64_t t;
    int32_t fh;
    if (small) {
        row_words(rp, len, r);
        row_hashes_reg(r, len, in.tag_bits, &t, &fh);
    } else {
#pragma unroll
        for (int k = 0; k < kRegWords; k++) r[k] = 0;
        row_hashes(reinterpret_cast<const uint32_t*>(rp), len, in.tag_bits, &t, &fh);
    }
    uint64_t s = fmix64(t) & d.mask;
    uint64_t loc = kNoLoc;
    int64_t sid = -1;
    for (; valid;) {
        // the whole line in four 16-B loads: a written slot holds the row's first kSlotWords
        // words and its id, so a row of up to 40 bytes is compared and resolved from the slot
        // alone -- no second random access into the arena (the 32-B key rows of a STRING key)
        const Slot cur = load_slot(&d.slots[s]);
        if (cur.tag == t) {   // (a slot claimed earlier in this call still has no entry: kNoLoc)
            loc = cur.loc;
            if (loc != kNoLoc) sid = slot_id_if_equal(d, cur, r, reinterpret_cast<const uint32_t*>(rp), small, len);
            break;
        }
        if (cur.tag == 0) {
            const unsigned long long old = atomicCAS(&d.slots[s].tag, 0ull, (unsigned long long)t);
            if (old == 0) {   // claimed: this row owns the new slot (no other row can claim it)
                d.slot_row[s] = (uint32_t)i;
                break;
            }
            if (old == t) break;   // claimed in this call by an equal-tagged row
        }
        s = (s + 1) & d.mask;
    }
    const int32_t kg = murmur_hash(fh) % in.max_p;
    if (valid) {
        if (loc != kNoLoc) {   // written by an earlier call, or an earlier chunk of this one
            if (sid < 0) atomicAdd(&d.counters[2], 1ull);
            id_out[i] = sid;
        }
    }
    const bool pend = valid && loc == kNoLoc;
    const unsigned long long at = wave_reserve(&d.counters[4], pend ? 1u : 0u);
    if (pend) {
        pend_out.row[at] = (uint32_t)i;
        pend_out.slot[at] = s;
        pend_out.kg[at] = kg;
    }
}

// pending rows: the claimer of a new slot allocates its id and writes its entry
__global__ __launch_bounds__(kDictThreads) void k_dict_assign(DictDev d, RowsIn in, Pending pend) {
    const uint64_t np = d.counters[4];
    const int lane = threadIdx.x & 63;
    // wave-uniform trip count (the reservations are wave-wide)
    for (uint64_t wb = (uint64_t)blockIdx.x * kDictThreads + (threadIdx.x & ~63u); wb < np;
         wb += (uint64_t)gridDim.x * kDictThreads) {
        const uint64_t j = wb + lane;
        const int64_t i = j < np ? pend.row[j] : 0;
        const uint64_t s = j < np ? pend.slot[j] : 0;
        const bool own = j < np && d.slot_row[s] == (uint32_t)i;
        const int32_t len = own ? in.len[i] : 0;
        // its ordinal: the next of the free list while one is left (counters[7] runs past nfree once
        // the list is spent), else a fresh one -- one reservation per wave per counter
        const unsigned long long fp = d.nfree ? wave_reserve(&d.counters[7], own ? 1u : 0u) : 0ull;
        const bool reuse = own && fp < d.nfree;
        const unsigned long long fresh = wave_reserve(&d.counters[0], own && !reuse ? 1u : 0u);
        const unsigned long long ord = reuse ? (unsigned long long)d.free_ord[fp] : fresh;
        const unsigned long long at = wave_reserve(&d.counters[1], own ? (uint32_t)(8 + ((len + 7) & ~7)) : 0u);
        if (!own) continue;
        const int64_t id = (int64_t)(ord << d.kg_bits | (uint64_t)pend.kg[j]);
        *reinterpret_cast<int64_t*>(d.arena + at) = id;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(in.bytes + in.off[i]);
        uint32_t* dst = reinterpret_cast<uint32_t*>(d.arena + at + 8);
        for (int32_t k = 0; k < (len >> 2); k++) dst[k] = src[k];
        if (len & 4) dst[len >> 2] = 0;   // (zero padding to 8 bytes)
        d.ent_off[ord] = (int64_t)at + 8;
        d.ent_len[ord] = len;
        d.ent_tag[ord] = d.slots[s].tag;
        Slot& sl = d.slots[s];
        sl.id = id;
        for (int k = 0; k < kSlotWords; k++) sl.row[k] = k < (len >> 2) ? src[k] : 0u;
        __threadfence();   // the slot's id and words before its loc (read by later chunks' probes)
        sl.loc = loc_of(at, len);
    }
}

// pending rows compare their bytes with their slot's (new) entry; a mismatch is left to the host
__global__ __launch_bounds__(kDictThreads) void k_dict_verify(DictDev d, RowsIn in, Pending pend, int64_t* id_out) {
    const uint64_t np = d.counters[4];
    for (uint64_t j = (uint64_t)blockIdx.x * kDictThreads + threadIdx.x; j < np; j += (uint64_t)gridDim.x * kDictThreads) {
        const int64_t i = pend.row[j];
        const int64_t id = entry_id_if_equal(d, d.slots[pend.slot[j]].loc,
                                             reinterpret_cast<const uint32_t*>(in.bytes + in.off[i]), in.len[i]);
        if (id < 0) atomicAdd(&d.counters[2], 1ull);
        id_out[i] = id;
    }
}

// rebuild the table at a larger capacity from the entries (ids keep their values)
__global__ __launch_bounds__(kDictThreads) void k_dict_rehash(DictDev d, int64_t nids) {
    const int64_t o = (int64_t)blockIdx.x * kDictThreads + threadIdx.x;
    if (o >= nids) return;
    const uint64_t t = d.ent_tag[o];
    if (t == 0) return;   // a host-resolved row: not in the table
    uint64_t s = fmix64(t) & d.mask;
    for (;;) {
        const unsigned long long old = atomicCAS(&d.slots[s].tag, 0ull, (unsigned long long)t);
        if (old == 0) break;
        s = (s + 1) & d.mask;
    }
    const int32_t len = d.ent_len[o];
    const uint8_t* e = d.arena + d.ent_off[o] - 8;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(e + 8);
    Slot& sl = d.slots[s];
    sl.id = *reinterpret_cast<const long long*>(e);
    for (int k = 0; k < kSlotWords; k++) sl.row[k] = k < (len >> 2) ? w[k] : 0u;
    sl.loc = loc_of((uint64_t)(d.ent_off[o] - 8), len);
}

__global__ __launch_bounds__(kDictThreads) void k_dict_gather(DictDev d, int64_t n, const int64_t* ids, int64_t nids,
                                                              int64_t* off_out, int32_t* len_out) {
    const int64_t i = (int64_t)blockIdx.x * kDictThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t ord = (uint64_t)ids[i] >> d.kg_bits;
    const int32_t len = ids[i] >= 0 && (int64_t)ord < nids ? d.ent_len[ord] : -1;   // (< 0: a retired ordinal)
    off_out[i] = len >= 0 ? d.ent_off[ord] : -1;
    len_out[i] = len >= 0 ? len : -1;
}

// ---- fg_key_dict_rows: the packed key rows of ids (the layout fg_key_dict_intern reads) ----
//
// Ids are taken in blocks of kRowsBlock. Lengths and offsets: k_rows_lengths (the ordinal check,
// out_lengths, each block's padded bytes), k_rows_scan_sums (one workgroup: the exclusive scan of
// the block sums, the total) and k_rows_offsets (out_offsets[0..n)); 64-bit throughout. The host
// reads RowsCtr once, checks the capacity and the bad ids, and only then launches k_rows_copy.
// (RowsCtr, padded8, the block scan, k_rows_scan_sums and k_rows_offsets: fg_rows_scan.h, shared with
// fg_keyproj.hip; RowsCtr's bad rows are here the ids that are negative or past the dictionary's size)
constexpr int kRowsBlock = kDictThreads;   // ids per scan block = rows per copy workgroup
static_assert(kRowsBlock == kScanThreads, "fg_rows_scan.h scans blocks of kScanThreads rows");

__global__ __launch_bounds__(kDictThreads) void k_rows_lengths(DictDev d, int64_t nids, int64_t n, const int64_t* ids,
                                                               int32_t* len_out, uint64_t* sums, RowsCtr* rc) {
    __shared__ uint64_t s_wave[kDictThreads / 64];
    const int64_t i = (int64_t)blockIdx.x * kRowsBlock + threadIdx.x;
    const bool valid = i < n;
    const int64_t id = valid ? ids[i] : 0;
    const uint64_t ord = (uint64_t)id >> d.kg_bits;
    const int32_t elen = valid && id >= 0 && (int64_t)ord < nids ? d.ent_len[ord] : -1;
    const bool ok = elen >= 0;   // (a retired ordinal's length is -1: unknown, like one never issued)
    const int32_t len = ok ? elen : 0;
    if (valid) len_out[i] = ok ? len : -1;
    const unsigned long long badm = __ballot(valid && !ok);   // (one atomic pair per wave holding a bad id)
    if (badm && (threadIdx.x & 63) == 0) {
        atomicAdd(&rc->bad, (unsigned long long)__popcll(badm));
        atomicMin(&rc->bad_first, (unsigned long long)(i + __ffsll((long long)badm) - 1));
    }
    uint64_t total;
    (void)block_exclusive_scan_u64(padded8(len), s_wave, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// The copy, balanced by bytes: a workgroup owns kRowsBlock consecutive rows, whose output span
// [off[r0], off[r0 + m]) is contiguous; its threads stride over the span's 8-byte words, so the
// stores are coalesced and no lane idles because its row is short. A word finds its row by a
// binary search over the run's offsets in LDS (the last row starting at or before it: empty rows
// share their successor's offset and are never picked) and loads the word at the same distance
// into that row's arena entry -- rows are 8-byte aligned and zero-padded to 8 in the arena, so
// whole words, pad included, are right. Launched only after the host has seen every id good and
// the total within the caller's capacity; an ordinal is still checked against nids (zero words).
__global__ __launch_bounds__(kDictThreads) void k_rows_copy(DictDev d, int64_t nids, int64_t n, const int64_t* ids,
                                                            const int64_t* off, uint64_t* out, int64_t out_words) {
    __shared__ int64_t s_off[kRowsBlock + 1];
    __shared__ int64_t s_src[kRowsBlock];
    const int64_t r0 = (int64_t)blockIdx.x * kRowsBlock;
    const int m = (int)(n - r0 < kRowsBlock ? n - r0 : kRowsBlock);
    if ((int)threadIdx.x < m) {
        const int64_t id = ids[r0 + threadIdx.x];
        const uint64_t ord = (uint64_t)id >> d.kg_bits;
        s_off[threadIdx.x] = off[r0 + threadIdx.x];
        s_src[threadIdx.x] = (id >= 0 && (int64_t)ord < nids) ? d.ent_off[ord] : -1;
    }
    if (threadIdx.x == 0) s_off[m] = off[r0 + m];
    __syncthreads();
    const int64_t w1 = s_off[m] >> 3 < out_words ? s_off[m] >> 3 : out_words;
    for (int64_t w = (s_off[0] >> 3) + threadIdx.x; w < w1; w += kDictThreads) {
        const int64_t b = w << 3;
        int lo = 0, hi = m;   // s_off[lo] <= b < s_off[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= b) lo = mid; else hi = mid;
        }
        const int64_t src = s_src[lo];
        out[w] = src >= 0 ? *reinterpret_cast<const uint64_t*>(d.arena + src + (b - s_off[lo])) : 0ull;
    }
}

// ---- the keyed edge (fg_partition_keyed_by_owner, keydict_intern_packed) ----
//
// Sender: the rows are grouped by owner (counts[par]) and their key rows packed in the grouped
// order, so owner p's key bytes are the offsets at its run's two boundaries: off[end_p] -
// off[begin_p], the boundaries being the exclusive scan of counts. One workgroup.
__global__ __launch_bounds__(kDictThreads) void k_owner_byte_counts(const int64_t* counts, int32_t par, const int64_t* off,
                                                                    int64_t n, int64_t* byte_counts) {
    __shared__ uint64_t s_wave[kDictThreads / 64];
    uint64_t carry = 0;   // (the same in every thread)
    for (int32_t p0 = 0; p0 < par; p0 += kDictThreads) {
        const int32_t p = p0 + (int32_t)threadIdx.x;
        const uint64_t c = p < par && counts[p] > 0 ? (uint64_t)counts[p] : 0ull;
        uint64_t total;
        const uint64_t b = carry + block_exclusive_scan_u64(c, s_wave, &total);
        carry += total;
        if (p < par) {   // (clamped: counts that do not add up to n never index past off[n])
            const uint64_t lo = b < (uint64_t)n ? b : (uint64_t)n;
            const uint64_t hi = b + c < (uint64_t)n ? b + c : (uint64_t)n;
            byte_counts[p] = off[hi] - off[lo];
        }
    }
}

// Receiver: the lengths as they came off the wire. A length that is negative, not a multiple of 4
// or >= 2^24 is counted (rc->bad, rc->bad_first) and taken as 0; each block's padded bytes go to
// sums (k_rows_scan_sums and k_rows_offsets then give the offsets). No key byte is read here.
__global__ __launch_bounds__(kDictThreads) void k_recv_lengths(int64_t n, const int32_t* len_in, uint64_t* sums,
                                                               RowsCtr* rc) {
    __shared__ uint64_t s_wave[kDictThreads / 64];
    const int64_t i = (int64_t)blockIdx.x * kRowsBlock + threadIdx.x;
    const bool valid = i < n;
    const int32_t len = valid ? len_in[i] : 0;
    const bool ok = len >= 0 && len < (1 << 24) && (len & 3) == 0;
    const unsigned long long badm = __ballot(valid && !ok);
    if (badm && (threadIdx.x & 63) == 0) {
        atomicAdd(&rc->bad, (unsigned long long)__popcll(badm));
        atomicMin(&rc->bad_first, (unsigned long long)(i - (threadIdx.x & 63) + __ffsll((long long)badm) - 1));
    }
    uint64_t total;
    (void)block_exclusive_scan_u64(ok ? padded8(len) : 0ull, s_wave, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kDictThreads) void k_slots_clear(Slot* p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kDictThreads + threadIdx.x;
    if (i < n) {
        uint4* q = reinterpret_cast<uint4*>(p + i);
        q[0] = make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu);   // tag 0, loc kNoLoc
        q[1] = q[2] = q[3] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// ---- fg_key_dict_retain: keep the listed ids, retire every other entry, compact, reuse ----
//
// Mark (k_retain_mark, one launch per set of ids: every id checked, a byte per kept ordinal), plan
// (k_retain_sums + k_retain_scan_sums: per block of kRowsBlock ordinals the arena bytes of its kept
// entries and the number of its dead ordinals, their exclusive scans and totals; 64-bit), one host
// read of RetCtr -- nothing of the dictionary has been written up to here -- then k_retain_compact
// (kept entries copied into a fresh arena, balanced by bytes like k_rows_copy; ent_off rewritten;
// dead ordinals marked ent_len -1 / ent_tag 0 and listed ascending as the free list), the table
// rebuilt by k_slots_clear + k_dict_rehash, and k_retain_side for the surviving host-resolved rows.
struct RetCtr {
    unsigned long long bad;        // listed ids that name no live entry
    unsigned long long bad_first;  // lowest (set << 32 | index) of such an id (~0: none)
    unsigned long long bytes;      // arena bytes of the kept entries
    unsigned long long dead;       // ordinals below `issued` that are not kept
};

// An id is good if it is not negative, its ordinal was issued and is not retired, and the id its
// arena entry stores is this id (a stale id whose ordinal was reused under another key group is
// not). Racing writers of a mark byte all store 1; bad ids take one atomic pair per wave.
__global__ __launch_bounds__(kDictThreads) void k_retain_mark(DictDev d, int64_t issued, int64_t n, const int64_t* ids,
                                                              int32_t set, uint8_t* mark, RetCtr* rc) {
    const int64_t i = (int64_t)blockIdx.x * kDictThreads + threadIdx.x;
    const bool valid = i < n;
    const int64_t id = valid ? ids[i] : 0;
    const uint64_t ord = (uint64_t)id >> d.kg_bits;
    bool ok = valid && id >= 0 && (int64_t)ord < issued;
    if (ok) ok = d.ent_len[ord] >= 0;
    if (ok) ok = *reinterpret_cast<const int64_t*>(d.arena + d.ent_off[ord] - 8) == id;
    if (ok) mark[ord] = 1;
    const unsigned long long badm = __ballot(valid && !ok);
    if (badm && (threadIdx.x & 63) == 0) {
        atomicAdd(&rc->bad, (unsigned long long)__popcll(badm));
        atomicMin(&rc->bad_first, (unsigned long long)set << 32 | (unsigned long long)(i + __ffsll((long long)badm) - 1));
    }
}

// per block of ordinals: sums[b] = arena bytes of its kept entries, sums[nb + b] = its dead ordinals
__global__ __launch_bounds__(kDictThreads) void k_retain_sums(DictDev d, int64_t issued, const uint8_t* mark, uint64_t* sums,
                                                              int64_t nb) {
    __shared__ uint64_t s_wave[kDictThreads / 64];
    const int64_t o = (int64_t)blockIdx.x * kRowsBlock + threadIdx.x;
    const bool in = o < issued, keep = in && mark[o];
    uint64_t bytes, dead;
    (void)block_exclusive_scan_u64(keep ? entry_bytes(d.ent_len[o]) : 0ull, s_wave, &bytes);
    (void)block_exclusive_scan_u64(in && !keep ? 1ull : 0ull, s_wave, &dead);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = bytes;
        sums[nb + blockIdx.x] = dead;
    }
}

// one workgroup: both halves of sums -> their exclusive scans, the totals to rc
__global__ __launch_bounds__(kDictThreads) void k_retain_scan_sums(uint64_t* sums, int64_t nb, RetCtr* rc) {
    __shared__ uint64_t s_wave[kDictThreads / 64];
    for (int h = 0; h < 2; h++) {
        uint64_t* v = sums + h * nb;
        uint64_t carry = 0;   // (the same in every thread)
        for (int64_t b0 = 0; b0 < nb; b0 += kDictThreads) {
            const int64_t b = b0 + threadIdx.x;
            uint64_t total;
            const uint64_t ex = block_exclusive_scan_u64(b < nb ? v[b] : 0ull, s_wave, &total);
            if (b < nb) v[b] = carry + ex;
            carry += total;
        }
        if (threadIdx.x == 0) (h ? rc->dead : rc->bytes) = carry;
    }
}

// A workgroup owns kRowsBlock consecutive ordinals. Its kept entries [id][row, padded to 8] land
// back to back at sums[block] in the new arena, so its output span is contiguous and its threads
// stride over the span's 8-byte words (k_rows_copy's balance: one very long row does not serialize
// its neighbours' lanes). Each thread first reads its own ordinal's old entry into LDS, then --
// no other workgroup reads that ordinal -- rewrites it: ent_off into the new arena, or ent_off -1,
// ent_len -1, ent_tag 0 and a place in the free list for a dead one.
__global__ __launch_bounds__(kDictThreads) void k_retain_compact(DictDev d, int64_t issued, const uint8_t* mark,
                                                                 const uint64_t* sums, int64_t nb, uint64_t* narena,
                                                                 int64_t* free_out) {
    __shared__ uint64_t s_wave[kDictThreads / 64];
    __shared__ int64_t s_off[kRowsBlock + 1];
    __shared__ int64_t s_src[kRowsBlock];
    const int64_t o = (int64_t)blockIdx.x * kRowsBlock + threadIdx.x;
    const bool in = o < issued, keep = in && mark[o];
    uint64_t bytes, dead;
    const uint64_t at = sums[blockIdx.x] + block_exclusive_scan_u64(keep ? entry_bytes(d.ent_len[o]) : 0ull, s_wave, &bytes);
    const uint64_t fp = sums[nb + blockIdx.x] + block_exclusive_scan_u64(in && !keep ? 1ull : 0ull, s_wave, &dead);
    s_off[threadIdx.x] = (int64_t)at;
    s_src[threadIdx.x] = keep ? d.ent_off[o] - 8 : -1;
    if (threadIdx.x == 0) s_off[kRowsBlock] = (int64_t)(sums[blockIdx.x] + bytes);
    __syncthreads();
    if (keep) {
        d.ent_off[o] = (int64_t)at + 8;
    } else if (in) {
        d.ent_off[o] = -1;
        d.ent_len[o] = -1;
        d.ent_tag[o] = 0;
        free_out[fp] = o;
    }
    const int64_t w1 = s_off[kRowsBlock] >> 3;
    for (int64_t w = (s_off[0] >> 3) + threadIdx.x; w < w1; w += kDictThreads) {
        const int64_t b = w << 3;
        int lo = 0, hi = kRowsBlock;   // s_off[lo] <= b < s_off[hi]; entries of no bytes are never picked
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= b) lo = mid; else hi = mid;
        }
        narena[w] = *reinterpret_cast<const uint64_t*>(d.arena + s_src[lo] + (b - s_off[lo]));
    }
}

// Surviving host-resolved rows (ent_tag 0: outside the table, found only through the slot of the
// row that held their tag) after the table was rebuilt: each is tagged again from its arena bytes
// and takes the slot of its tag if no live row holds it -- one wins per tag, the rest stay with
// the host. state: 0 retired, 1 still resolved on the host, 2 now in the table.
__global__ __launch_bounds__(kDictThreads) void k_retain_side(DictDev d, int tag_bits, int64_t n, const int64_t* ords,
                                                              int32_t* state) {
    const int64_t i = (int64_t)blockIdx.x * kDictThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t o = ords[i];
    const int32_t len = d.ent_len[o];
    if (len < 0) {
        state[i] = 0;
        return;
    }
    const uint8_t* e = d.arena + d.ent_off[o] - 8;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(e + 8);
    uint64_t t;
    int32_t fh;
    row_hashes(w, len, tag_bits, &t, &fh);
    uint64_t s = fmix64(t) & d.mask;
    for (;;) {
        const unsigned long long old = atomicCAS(&d.slots[s].tag, 0ull, (unsigned long long)t);
        if (old == 0) break;
        if (old == t) {
            state[i] = 1;
            return;
        }
        s = (s + 1) & d.mask;
    }
    Slot& sl = d.slots[s];
    sl.id = *reinterpret_cast<const long long*>(e);
    for (int k = 0; k < kSlotWords; k++) sl.row[k] = k < (len >> 2) ? w[k] : 0u;
    sl.loc = loc_of((uint64_t)(d.ent_off[o] - 8), len);
    d.ent_tag[o] = t;
    state[i] = 2;
}

inline unsigned grid_of(int64_t n) { return (unsigned)((n + kDictThreads - 1) / kDictThreads); }

struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() {
        if (p) (void)hipFree(p);
    }
    // grow to `need` bytes, keeping the first `keep` bytes
    hipError_t ensure(size_t need, hipStream_t s, size_t keep = 0) {
        if (need <= bytes) return hipSuccess;
        const size_t nb = std::max(need, bytes + bytes / 2);
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, nb);
        if (e != hipSuccess) return e;
        if (keep && p) {
            e = hipMemcpyAsync(q, p, std::min(keep, bytes), hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) {
                (void)hipFree(q);
                return e;
            }
        }
        if (p) (void)hipFree(p);
        p = q;
        bytes = nb;
        return hipSuccess;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

}  // namespace

struct fg_key_dict {
    int device = 0;
    int32_t max_p = 128;
    int tag_bits = 64;
    hipStream_t stream = nullptr;
    uint64_t cap = 0;   // table slots (power of two)
    uint64_t cap0 = 0;  // ... at open: a retain never shrinks the table below it
    int64_t nids = 0;   // ordinals issued (host mirror of counters[0]): every valid ordinal is below it
    int64_t arena_used = 0;
    // ordinals a retain retired, ascending (free_ord[nfree]); free_taken of them are in use again
    // (host mirror of counters[7], capped at nfree). The live entries are live().
    int64_t nfree = 0, free_taken = 0, retired_total = 0;
    Buf slots, slot_row, ent_off, ent_len, ent_tag, arena, counters, free_ord;
    Buf ret_mark, ret_ctr, ret_side;   // fg_key_dict_retain: mark bytes, RetCtr, the side rows' ordinals and states
    Buf in_bytes, in_off, in_len, row_tag, row_kg, row_slot, row_pkg, row_id, miss;   // per-call scratch
    // fg_key_dict_rows: its counters (RowsCtr), the block sums, and for FG_HOST callers the device
    // ids, lengths, offsets and packed bytes; grown on demand and reused across calls
    Buf rows_ctr, rows_sums, rows_ids, rows_len, rows_off, rows_bytes;
    Buf part_scratch;                // fg_partition_keyed_by_owner: the owner partition's histogram and offsets
    // fg_key_dict_project / _intern_fields: for FG_HOST callers the device records, columns and null
    // bytes; the key rows' offsets, lengths and bytes (intern_fields, and FG_HOST project) and the
    // ids and key groups of FG_HOST intern_fields; grown to the largest call
    Buf pj_bytes, pj_off, pj_len, pj_cols, pj_null, pj_koff, pj_klen, pj_kbytes, pj_ids, pj_kg;
    bool projected = false;          // a projection's length pass has run: kernel_stats lists "dict_project"
    hipEvent_t ev_order = nullptr;   // ... and the event that orders a caller's stream after the dictionary's
    std::unordered_map<std::string, int64_t> side;   // rows whose tag another row holds
    std::string err;
    // kernel timing (fg_key_dict_set_timing): HIP events around each chunk's probe and its
    // assign + verify, and around the two kernel stages of fg_key_dict_rows (ev[3..6]), on the
    // dictionary's stream; summed into the three classes below
    bool timing = false;
    // ([7..10]: the two kernel stages of fg_key_dict_retain, "dict_retain"; [11..12]: a table rebuild --
    // k_slots_clear + k_dict_rehash, when the table grows and inside a retain -- "dict_rebuild";
    // [13..16]: the two kernel stages of a projection, "dict_project")
    hipEvent_t ev[17] = {};
    fg_kernel_stat kstat[6] = {};
    // fg_key_dict_intern_async: the lookup launched, the rest of the call taken by _wait
    struct Pending {
        bool active = false, host = false;
        int64_t n = 0, nbytes = 0;
        RowsIn in{};
        int64_t* ids = nullptr;
        int32_t* kg_dev = nullptr;
        const uint8_t* bytes = nullptr;
        const int64_t* offsets = nullptr;
        const int32_t* lengths = nullptr;
        int64_t* out_id = nullptr;
        int32_t* out_kg = nullptr;
        uint64_t entry_need = 0;   // host rows: every row as a new entry
    } pend;

    int fail(int rc, const std::string& m) {
        err = m;
        return rc;
    }
    int64_t live() const { return nids - (nfree - free_taken); }
    // one table rebuild bracketed by ev[11], ev[12] (complete): records = the ordinals rehashed, rows = the slots
    hipError_t rebuilt() {
        float ms = 0.f;
        const hipError_t e = hipEventElapsedTime(&ms, ev[11], ev[12]);
        kstat[4].launches++;
        kstat[4].total_ms += ms;
        kstat[4].records += nids;
        kstat[4].rows += (int64_t)cap;
        return e;
    }
    // the counters as intern_finish read them: ordinals issued, arena bytes, free ordinals taken
    void mirror(const unsigned long long* cnt) {
        nids = (int64_t)cnt[0];
        arena_used = (int64_t)cnt[1];
        if (nfree) free_taken = std::min<int64_t>((int64_t)cnt[7], nfree);
        if (free_taken == nfree) nfree = free_taken = 0;   // spent: k_dict_assign leaves counters[7] alone again
    }
    DictDev dev() const {
        DictDev d;
        d.slots = slots.as<Slot>();
        d.slot_row = slot_row.as<uint32_t>();
        d.ent_off = ent_off.as<int64_t>();
        d.ent_len = ent_len.as<int32_t>();
        d.ent_tag = ent_tag.as<uint64_t>();
        d.arena = arena.as<uint8_t>();
        d.counters = counters.as<unsigned long long>();
        d.free_ord = free_ord.as<int64_t>();
        d.nfree = (uint64_t)nfree;
        d.mask = cap - 1;
        d.kg_bits = dict_kg_bits(max_p);
        return d;
    }
};

#define DCHK(d, x)                                                                     \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) return (d)->fail(FG_EDEVICE, std::string(#x " failed: ") + hipGetErrorString(e_)); \
    } while (0)

namespace {

// table at `ncap` slots (power of two) holding every entry
int rebuild(fg_key_dict* d, uint64_t ncap) {
    hipStream_t s = d->stream;
    Buf nslots, nrow;
    DCHK(d, nslots.ensure(sizeof(Slot) * ncap, s));
    DCHK(d, nrow.ensure(4 * ncap, s));
    if (d->timing) DCHK(d, hipEventRecord(d->ev[11], s));
    hipLaunchKernelGGL(k_slots_clear, dim3(grid_of((int64_t)ncap)), dim3(kDictThreads), 0, s, nslots.as<Slot>(),
                       (int64_t)ncap);
    DCHK(d, hipGetLastError());
    std::swap(d->slots.p, nslots.p);
    std::swap(d->slots.bytes, nslots.bytes);
    std::swap(d->slot_row.p, nrow.p);
    std::swap(d->slot_row.bytes, nrow.bytes);
    d->cap = ncap;
    if (d->nids)
        hipLaunchKernelGGL(k_dict_rehash, dim3(grid_of(d->nids)), dim3(kDictThreads), 0, s, d->dev(), d->nids);
    if (d->timing) DCHK(d, hipEventRecord(d->ev[12], s));
    DCHK(d, hipGetLastError());
    DCHK(d, hipStreamSynchronize(s));
    if (d->timing) DCHK(d, d->rebuilt());
    return FG_OK;
}

// Rows of one chunk whose 64-bit tag another row holds (ids -1): exact ids from the host-side
// map, new rows appended to the arena (ent_tag 0: never rehashed into the table). `bytes`,
// `offsets`, `lengths` are the caller's (host or device) arrays for the chunk's rows.
int resolve_collisions(fg_key_dict* d, bool host, int64_t n, const uint8_t* bytes, int64_t nbytes,
                       const int64_t* offsets, const int32_t* lengths, int64_t* ids) {
    hipStream_t s = d->stream;
    std::vector<int64_t> hid(n);
    DCHK(d, hipMemcpy(hid.data(), ids, 8 * (size_t)n, hipMemcpyDeviceToHost));
    // device rows: one copy of the buffer and the chunk's offsets / lengths, not one per row
    std::vector<uint8_t> hbytes;
    std::vector<int64_t> hoff;
    std::vector<int32_t> hlen;
    if (!host) {
        hbytes.resize((size_t)nbytes);
        hoff.resize(n);
        hlen.resize(n);
        if (nbytes) DCHK(d, hipMemcpy(hbytes.data(), bytes, (size_t)nbytes, hipMemcpyDeviceToHost));
        DCHK(d, hipMemcpy(hoff.data(), offsets, 8 * (size_t)n, hipMemcpyDeviceToHost));
        DCHK(d, hipMemcpy(hlen.data(), lengths, 4 * (size_t)n, hipMemcpyDeviceToHost));
    }
    const uint8_t* rb = host ? bytes : hbytes.data();
    const int64_t* ro = host ? offsets : hoff.data();
    const int32_t* rl = host ? lengths : hlen.data();
    for (int64_t i = 0; i < n; i++) {
        if (hid[i] >= 0) continue;
        const int32_t l = rl[i];
        const uint8_t* row = rb + ro[i];
        std::string k(row, row + l);
        auto it = d->side.find(k);
        int64_t id;
        if (it != d->side.end()) {
            id = it->second;
        } else {
            // its entry ([id][row bytes, padded]) appended to the arena, out of the table
            const int64_t ord = d->nids++;
            const int64_t at = d->arena_used;
            d->arena_used += 8 + ((l + 7) & ~7);
            DCHK(d, d->ent_off.ensure(8 * (size_t)d->nids, s, 8 * (size_t)ord));
            DCHK(d, d->ent_len.ensure(4 * (size_t)d->nids, s, 4 * (size_t)ord));
            DCHK(d, d->ent_tag.ensure(8 * (size_t)d->nids, s, 8 * (size_t)ord));
            DCHK(d, d->arena.ensure((size_t)d->arena_used, s, (size_t)at));
            const int32_t kg = murmur_hash(binaryrow_hash_bytes(row, l)) % d->max_p;
            id = (int64_t)((uint64_t)ord << dict_kg_bits(d->max_p) | (uint64_t)kg);
            std::vector<uint8_t> entry(8 + ((l + 7) & ~7), 0);
            std::memcpy(entry.data(), &id, 8);
            std::memcpy(entry.data() + 8, row, (size_t)l);
            const uint64_t zero = 0;
            const int64_t row_off = at + 8;
            DCHK(d, hipMemcpy(d->arena.as<uint8_t>() + at, entry.data(), entry.size(), hipMemcpyHostToDevice));
            DCHK(d, hipMemcpy(d->ent_off.as<int64_t>() + ord, &row_off, 8, hipMemcpyHostToDevice));
            DCHK(d, hipMemcpy(d->ent_len.as<int32_t>() + ord, &l, 4, hipMemcpyHostToDevice));
            DCHK(d, hipMemcpy(d->ent_tag.as<uint64_t>() + ord, &zero, 8, hipMemcpyHostToDevice));
            d->side.emplace(std::move(k), id);
        }
        hid[i] = id;
    }
    DCHK(d, hipMemcpy(ids, hid.data(), 8 * (size_t)n, hipMemcpyHostToDevice));
    const unsigned long long c2[3] = {(unsigned long long)d->nids, (unsigned long long)d->arena_used, 0ull};
    DCHK(d, hipMemcpy(d->counters.p, c2, sizeof c2, hipMemcpyHostToDevice));
    return FG_OK;
}

// The rows pipeline of fg_key_dict_rows and fg_partition_keyed_by_owner, on stream s (the
// dictionary's, or a caller's ordered after it) over device ids. Stage 1: lengths[n] (-1 for an
// unknown id), offsets[n + 1] and the call's RowsCtr (d->rows_ctr, for the one host read).
int rows_lengths_offsets(fg_key_dict* d, hipStream_t s, int64_t n, const int64_t* ids, int32_t* len_out,
                         int64_t* off_out) {
    const int64_t nb = (n + kRowsBlock - 1) / kRowsBlock;
    DCHK(d, d->rows_ctr.ensure(sizeof(RowsCtr), s));
    DCHK(d, d->rows_sums.ensure(8 * (size_t)nb, s));
    RowsCtr* rc = d->rows_ctr.as<RowsCtr>();
    uint64_t* sums = d->rows_sums.as<uint64_t>();
    DCHK(d, hipMemsetAsync(rc, 0, offsetof(RowsCtr, bad_first), s));
    DCHK(d, hipMemsetAsync(&rc->bad_first, 0xff, 8, s));
    if (d->timing) DCHK(d, hipEventRecord(d->ev[3], s));
    hipLaunchKernelGGL(k_rows_lengths, dim3((unsigned)nb), dim3(kDictThreads), 0, s, d->dev(), d->nids, n, ids, len_out,
                       sums, rc);
    hipLaunchKernelGGL(k_rows_scan_sums, dim3(1), dim3(kDictThreads), 0, s, sums, nb, rc, off_out, n);
    hipLaunchKernelGGL(k_rows_offsets, dim3((unsigned)nb), dim3(kDictThreads), 0, s, n, len_out, sums, off_out);
    if (d->timing) DCHK(d, hipEventRecord(d->ev[4], s));
    DCHK(d, hipGetLastError());
    return FG_OK;
}

// Stage 2, the copy: only after the host has seen every id good and `total` within the buffer.
int rows_copy(fg_key_dict* d, hipStream_t s, int64_t n, const int64_t* ids, const int64_t* off, uint8_t* out,
              int64_t total) {
    const int64_t nb = (n + kRowsBlock - 1) / kRowsBlock;
    if (d->timing) DCHK(d, hipEventRecord(d->ev[5], s));
    hipLaunchKernelGGL(k_rows_copy, dim3((unsigned)nb), dim3(kDictThreads), 0, s, d->dev(), d->nids, n, ids, off,
                       reinterpret_cast<uint64_t*>(out), total >> 3);
    if (d->timing) DCHK(d, hipEventRecord(d->ev[6], s));
    DCHK(d, hipGetLastError());
    return FG_OK;
}

uint64_t pow2_at_least(uint64_t x) {
    uint64_t c = 1024;
    while (c < x) c <<= 1;
    return c;
}

}  // namespace

extern "C" {

int fg_key_dict_open(int32_t device_id, int32_t max_parallelism, int64_t expected_keys, fg_key_dict** out) {
    if (!out || max_parallelism <= 0 || max_parallelism > (1 << 15)) return FG_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) return FG_EDEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return FG_EDEVICE;
    std::unique_ptr<fg_key_dict> d(new fg_key_dict());
    d->device = device_id;
    d->max_p = max_parallelism;
    if (const char* e = getenv("FG_DICT_TAG_BITS")) d->tag_bits = std::max(1, std::min(64, std::atoi(e)));   // tests
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) return FG_EDEVICE;
    if (d->counters.ensure(64, d->stream) != hipSuccess) return FG_EDEVICE;
    if (hipMemsetAsync(d->counters.p, 0, 64, d->stream) != hipSuccess) return FG_EDEVICE;
    if (rebuild(d.get(), pow2_at_least(FG_DICT_INIT * (uint64_t)std::max<int64_t>(expected_keys, 1)))) return FG_EDEVICE;
    d->cap0 = d->cap;
    *out = d.release();
    return FG_OK;
}

// The first half of an intern call: arguments checked, scratch sized, the lookup of every row
// launched (device rows are checked by the lookup itself: a bad row is counted, not looked up,
// and the call fails in intern_finish before anything is inserted). No host synchronization.
static int intern_begin(fg_key_dict* d, int32_t location, int64_t n, const uint8_t* bytes, int64_t nbytes,
                        const int64_t* offsets, const int32_t* lengths, int64_t* out_id, int32_t* out_kg) {
    if (!d) return FG_EINVAL;
    if (d->pend.active) return d->fail(FG_ESTATE, "fg_key_dict_intern: an async intern is pending (fg_key_dict_intern_wait)");
    if (n < 0 || n > 0x7fffffff || !bytes || nbytes < 0 || !offsets || !lengths || !out_id)
        return d->fail(FG_EINVAL, "fg_key_dict_intern: invalid arguments");
    if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
    hipStream_t s = d->stream;
    const bool host = location == FG_HOST;
    if (!host && (uintptr_t)bytes % 4 != 0)
        return d->fail(FG_EINVAL, "fg_key_dict_intern: the row buffer must be 4-byte aligned");
    uint64_t entry_need = 0;   // host rows: arena bytes if every row is new
    if (host) {   // validate on the host: every row inside the buffer, 4-byte words
        for (int64_t i = 0; i < n; i++) {
            if (lengths[i] < 0 || lengths[i] >= (1 << 24) || (lengths[i] & 3) || (offsets[i] & 3) || offsets[i] < 0 ||
                offsets[i] + lengths[i] > nbytes)
                return d->fail(FG_EINVAL, "key row " + std::to_string(i) +
                                              ": offset/length outside the buffer or not a multiple of 4 bytes");
            entry_need += entry_bytes(lengths[i]);
        }
    }
    const size_t ents = (size_t)(d->nids + n);
    DCHK(d, d->ent_off.ensure(8 * ents, s, 8 * (size_t)d->nids));
    DCHK(d, d->ent_len.ensure(4 * ents, s, 4 * (size_t)d->nids));
    DCHK(d, d->ent_tag.ensure(8 * ents, s, 8 * (size_t)d->nids));
    RowsIn in{};
    in.n = n;
    in.nbytes = nbytes;
    in.max_p = d->max_p;
    in.tag_bits = d->tag_bits;
    in.check = host ? 0 : 1;
    if (host) {
        DCHK(d, d->in_bytes.ensure((size_t)nbytes + 8, s));
        DCHK(d, d->in_off.ensure(8 * (size_t)n, s));
        DCHK(d, d->in_len.ensure(4 * (size_t)n, s));
        DCHK(d, hipMemcpyAsync(d->in_bytes.p, bytes, (size_t)nbytes, hipMemcpyHostToDevice, s));
        DCHK(d, hipMemcpyAsync(d->in_off.p, offsets, 8 * (size_t)n, hipMemcpyHostToDevice, s));
        DCHK(d, hipMemcpyAsync(d->in_len.p, lengths, 4 * (size_t)n, hipMemcpyHostToDevice, s));
        in.bytes = d->in_bytes.as<uint8_t>();
        in.off = d->in_off.as<int64_t>();
        in.len = d->in_len.as<int32_t>();
    } else {
        in.bytes = bytes;
        in.off = offsets;
        in.len = lengths;
    }
    int64_t* ids = out_id;
    if (host) {
        DCHK(d, d->row_id.ensure(8 * (size_t)n, s));
        ids = d->row_id.as<int64_t>();
    }
    int32_t* kg_dev = nullptr;   // every row's key group, when asked for
    if (out_kg) {
        if (host) {
            DCHK(d, d->row_kg.ensure(4 * (size_t)n, s));
            kg_dev = d->row_kg.as<int32_t>();
        } else {
            kg_dev = out_kg;
        }
    }
    // 1) lookup of every row: one random 64-B slot per row; the misses are listed, their arena
    // bytes summed (counters[5]), bad device rows counted (counters[3])
    DCHK(d, d->miss.ensure(4 * (size_t)std::max<int64_t>(n, 1), s));
    unsigned long long* ctr = d->counters.as<unsigned long long>();
    DCHK(d, hipMemsetAsync(ctr + 5, 0, 16, s));   // [5] miss entry bytes, [6] misses
    if (n > 0) {
        if (d->timing) DCHK(d, hipEventRecord(d->ev[0], s));
        hipLaunchKernelGGL(k_dict_lookup, dim3((unsigned)((n + (int64_t)kDictThreads * kLookupRows - 1) /
                                                    ((int64_t)kDictThreads * kLookupRows))),
                           dim3(kDictThreads), 0, s, d->dev(), in, kg_dev, ids, d->miss.as<uint32_t>());
        if (d->timing) DCHK(d, hipEventRecord(d->ev[1], s));
        DCHK(d, hipGetLastError());
    }
    auto& pc = d->pend;
    pc.active = true;
    pc.host = host;
    pc.n = n;
    pc.nbytes = nbytes;
    pc.in = in;
    pc.ids = ids;
    pc.kg_dev = kg_dev;
    pc.bytes = bytes;
    pc.offsets = offsets;
    pc.lengths = lengths;
    pc.out_id = out_id;
    pc.out_kg = out_kg;
    pc.entry_need = entry_need;
    return FG_OK;
}

// The second half: the lookup's counters (one synchronization), then the misses -- none in a
// steady state -- in chunks, and the collisions.
static int intern_finish(fg_key_dict* d) {
    if (!d) return FG_EINVAL;
    if (!d->pend.active) return FG_OK;
    auto pc = d->pend;
    d->pend.active = false;
    hipStream_t s = d->stream;
    const int64_t n = pc.n;
    RowsIn in = pc.in;
    int64_t* ids = pc.ids;
    unsigned long long* ctr = d->counters.as<unsigned long long>();
    unsigned long long cnt[8];
    DCHK(d, hipMemcpyAsync(cnt, ctr, sizeof cnt, hipMemcpyDeviceToHost, s));
    DCHK(d, hipStreamSynchronize(s));
    if (n == 0) return FG_OK;
    if (cnt[3]) {   // bad device rows: nothing was inserted
        DCHK(d, hipMemsetAsync(ctr + 3, 0, 8, s));
        DCHK(d, hipStreamSynchronize(s));
        return d->fail(FG_EINVAL, "fg_key_dict_intern: " + std::to_string(cnt[3]) +
                                      " key rows outside the buffer or not a multiple of 4 bytes");
    }
    if (d->timing) {
        float ms = 0.f;
        DCHK(d, hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
        d->kstat[0].launches++;
        d->kstat[0].total_ms += ms;
        d->kstat[0].records += n;
    }
    uint64_t collisions = cnt[2];
    const int64_t nmiss = (int64_t)cnt[6];
    if (nmiss > 0) {
        // k_dict_assign writes a new row's entry at a reserved arena offset without a bound check:
        // the arena holds every missed row of the call as a new entry
        const uint64_t need = pc.host ? pc.entry_need : cnt[5];
        DCHK(d, d->arena.ensure((size_t)d->arena_used + (size_t)need + 16, s, (size_t)d->arena_used));
    }
    // 2) the misses, in chunks the table has room for: it stays at most half full even if every
    // row of a chunk is new. It grows when that room falls under an eighth of the live entries (and
    // 1M rows): to FG_DICT_GROW x (live + 1M) slots rounded up -- sized by the distinct live keys.
    for (int64_t pos = 0; pos < nmiss;) {
        const int64_t live = d->live();
        const int64_t room = (int64_t)(d->cap / 2) - live;
        if (room < std::max<int64_t>(1 << 20, live / 8))
            if (int rc = rebuild(d, pow2_at_least(FG_DICT_GROW * (uint64_t)(live + (1 << 20))))) return rc;
        const int64_t m = std::min<int64_t>(nmiss - pos, (int64_t)(d->cap / 2) - live);
        DCHK(d, d->row_tag.ensure(4 * (size_t)m, s));   // the pending list
        DCHK(d, d->row_slot.ensure(8 * (size_t)m, s));
        DCHK(d, d->row_pkg.ensure(4 * (size_t)m, s));
        RowsIn c = in;
        c.idx = d->miss.as<uint32_t>() + pos;
        c.n = m;
        const Pending pend{d->row_tag.as<uint32_t>(), d->row_slot.as<uint64_t>(), d->row_pkg.as<int32_t>()};
        const DictDev dv = d->dev();
        const unsigned gm = grid_of(m);
        DCHK(d, hipMemsetAsync(dv.counters + 4, 0, 8, s));
        if (d->timing) DCHK(d, hipEventRecord(d->ev[1], s));
        hipLaunchKernelGGL(k_dict_probe, dim3(gm), dim3(kDictThreads), 0, s, dv, c, ids, pend);
        const unsigned gp = std::min(gm, 1024u);
        hipLaunchKernelGGL(k_dict_assign, dim3(gp), dim3(kDictThreads), 0, s, dv, c, pend);
        hipLaunchKernelGGL(k_dict_verify, dim3(gp), dim3(kDictThreads), 0, s, dv, c, pend, ids);
        if (d->timing) DCHK(d, hipEventRecord(d->ev[2], s));
        DCHK(d, hipGetLastError());
        DCHK(d, hipMemcpyAsync(cnt, ctr, sizeof cnt, hipMemcpyDeviceToHost, s));
        DCHK(d, hipStreamSynchronize(s));
        if (d->timing) {
            float ms = 0.f;
            DCHK(d, hipEventElapsedTime(&ms, d->ev[1], d->ev[2]));
            d->kstat[1].launches++;
            d->kstat[1].total_ms += ms;
            d->kstat[1].records += m;
        }
        d->mirror(cnt);
        pos += m;
    }
    collisions = cnt[2];
    if (collisions) {   // rows whose tag another row holds: exact ids from the host-side map
        DCHK(d, hipMemsetAsync(ctr + 2, 0, 8, s));
        if (int rc = resolve_collisions(d, pc.host, n, pc.bytes, pc.nbytes, pc.offsets, pc.lengths, ids)) return rc;
    }
    if (pc.host) DCHK(d, hipMemcpy(pc.out_id, ids, 8 * (size_t)n, hipMemcpyDeviceToHost));
    if (pc.out_kg && pc.host) DCHK(d, hipMemcpy(pc.out_kg, pc.kg_dev, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return FG_OK;
}

int fg_key_dict_intern(fg_key_dict* d, int32_t location, int64_t n, const uint8_t* bytes, int64_t nbytes,
                       const int64_t* offsets, const int32_t* lengths, int64_t* out_id, int32_t* out_kg) {
    if (!d) return FG_EINVAL;
    if (n == 0 && !d->pend.active) return FG_OK;
    if (int rc = intern_begin(d, location, n, bytes, nbytes, offsets, lengths, out_id, out_kg)) return rc;
    return intern_finish(d);
}

int fg_key_dict_intern_async(fg_key_dict* d, int64_t n, const uint8_t* bytes, int64_t nbytes, const int64_t* offsets,
                             const int32_t* lengths, int64_t* out_id, int32_t* out_kg) {
    if (!d) return FG_EINVAL;
    return intern_begin(d, FG_DEVICE, n, bytes, nbytes, offsets, lengths, out_id, out_kg);
}

int fg_key_dict_intern_wait(fg_key_dict* d) {
    if (!d) return FG_EINVAL;
    if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
    return intern_finish(d);
}

int fg_key_dict_lookup(fg_key_dict* d, int32_t location, int64_t n, const int64_t* ids, int64_t* out_offsets,
                       int32_t* out_lengths) {
    if (!d) return FG_EINVAL;
    if (n == 0) return FG_OK;
    if (d->pend.active) return d->fail(FG_ESTATE, "fg_key_dict_lookup: an async intern is pending (fg_key_dict_intern_wait)");
    if (n < 0 || !ids || !out_offsets || !out_lengths) return d->fail(FG_EINVAL, "fg_key_dict_lookup: invalid arguments");
    if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
    hipStream_t s = d->stream;
    const bool host = location == FG_HOST;
    const int64_t* di = ids;
    int64_t* doff = out_offsets;
    int32_t* dlen = out_lengths;
    Buf bi, bo, bl;
    if (host) {
        DCHK(d, bi.ensure(8 * (size_t)n, s));
        DCHK(d, bo.ensure(8 * (size_t)n, s));
        DCHK(d, bl.ensure(4 * (size_t)n, s));
        DCHK(d, hipMemcpyAsync(bi.p, ids, 8 * (size_t)n, hipMemcpyHostToDevice, s));
        di = bi.as<int64_t>();
        doff = bo.as<int64_t>();
        dlen = bl.as<int32_t>();
    }
    hipLaunchKernelGGL(k_dict_gather, dim3(grid_of(n)), dim3(kDictThreads), 0, s, d->dev(), n, di, d->nids, doff, dlen);
    DCHK(d, hipGetLastError());
    if (host) {
        DCHK(d, hipMemcpyAsync(out_offsets, doff, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
        DCHK(d, hipMemcpyAsync(out_lengths, dlen, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    }
    DCHK(d, hipStreamSynchronize(s));
    return FG_OK;
}

int fg_key_dict_rows(fg_key_dict* d, int32_t location, int64_t n, const int64_t* ids, uint8_t* out_bytes,
                     int64_t cap_bytes, int64_t* out_offsets, int32_t* out_lengths, int64_t* out_nbytes) {
    if (!d) return FG_EINVAL;
    if (location != FG_HOST && location != FG_DEVICE) return d->fail(FG_EINVAL, "fg_key_dict_rows: unknown location");
    if (n < 0 || n > 0x7fffffff || cap_bytes < 0 || (cap_bytes > 0 && !out_bytes) ||
        (n > 0 && (!ids || !out_offsets || !out_lengths || !out_nbytes)))
        return d->fail(FG_EINVAL, "fg_key_dict_rows: invalid arguments");
    const bool host = location == FG_HOST;
    if (!host && (uintptr_t)out_bytes % 8 != 0)
        return d->fail(FG_EINVAL, "fg_key_dict_rows: a device out_bytes must be 8-byte aligned");
    if (d->pend.active) return d->fail(FG_ESTATE, "fg_key_dict_rows: an async intern is pending (fg_key_dict_intern_wait)");
    if (n == 0) {
        if (out_nbytes) *out_nbytes = 0;
        if (out_offsets && host) out_offsets[0] = 0;
        if (out_offsets && !host) {   // (a device word: the only device work of an empty call)
            if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
            DCHK(d, hipMemsetAsync(out_offsets, 0, 8, d->stream));
            DCHK(d, hipStreamSynchronize(d->stream));
        }
        return FG_OK;
    }
    if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
    hipStream_t s = d->stream;
    const int64_t* di = ids;
    int64_t* doff = out_offsets;
    int32_t* dlen = out_lengths;
    if (host) {
        DCHK(d, d->rows_ids.ensure(8 * (size_t)n, s));
        DCHK(d, d->rows_off.ensure(8 * (size_t)(n + 1), s));
        DCHK(d, d->rows_len.ensure(4 * (size_t)n, s));
        DCHK(d, hipMemcpyAsync(d->rows_ids.p, ids, 8 * (size_t)n, hipMemcpyHostToDevice, s));
        di = d->rows_ids.as<int64_t>();
        doff = d->rows_off.as<int64_t>();
        dlen = d->rows_len.as<int32_t>();
    }
    // 1) lengths and offsets; then the one host read of the call: {total, bad ids, lowest bad index}
    if (int rc1 = rows_lengths_offsets(d, s, n, di, dlen, doff)) return rc1;
    RowsCtr* rc = d->rows_ctr.as<RowsCtr>();   // (allocated by the stage above)
    RowsCtr hc;
    DCHK(d, hipMemcpyAsync(&hc, rc, sizeof hc, hipMemcpyDeviceToHost, s));
    DCHK(d, hipStreamSynchronize(s));
    float ms = 0.f;
    if (d->timing) DCHK(d, hipEventElapsedTime(&ms, d->ev[3], d->ev[4]));
    auto timed = [&](float t) {
        if (!d->timing) return;
        d->kstat[2].launches++;
        d->kstat[2].total_ms += t;
        d->kstat[2].records += n;
    };
    if (hc.bad) {
        timed(ms);
        return d->fail(FG_EINVAL, "fg_key_dict_rows: " + std::to_string(hc.bad) +
                                      " unknown ids (negative, or not below the dictionary's size); the first at index " +
                                      std::to_string(hc.bad_first));
    }
    const int64_t total = (int64_t)hc.total;
    *out_nbytes = total;
    if (host) {   // straight into the caller's memory (pinned or pageable): no staging of our own
        DCHK(d, hipMemcpyAsync(out_offsets, doff, 8 * (size_t)(n + 1), hipMemcpyDeviceToHost, s));
        DCHK(d, hipMemcpyAsync(out_lengths, dlen, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    }
    if (total > cap_bytes) {
        if (host) DCHK(d, hipStreamSynchronize(s));
        timed(ms);
        return d->fail(FG_EFULL, "fg_key_dict_rows: the rows take " + std::to_string(total) + " bytes, out_bytes holds " +
                                     std::to_string(cap_bytes));
    }
    // 2) the copy: total <= cap_bytes and every id is good
    if (total > 0) {
        uint8_t* dbytes = out_bytes;
        if (host) {
            DCHK(d, d->rows_bytes.ensure((size_t)total, s));
            dbytes = d->rows_bytes.as<uint8_t>();
        }
        if (int rc2 = rows_copy(d, s, n, di, doff, dbytes, total)) return rc2;
        if (host) DCHK(d, hipMemcpyAsync(out_bytes, dbytes, (size_t)total, hipMemcpyDeviceToHost, s));
    }
    DCHK(d, hipStreamSynchronize(s));
    if (d->timing && total > 0) {
        float ms2 = 0.f;
        DCHK(d, hipEventElapsedTime(&ms2, d->ev[5], d->ev[6]));
        ms += ms2;
    }
    timed(ms);
    return FG_OK;
}

// fg_key_dict_project (intern false) and fg_key_dict_intern_fields (intern true): the arguments
// checked, FG_HOST inputs staged, the length pass (fg_keyproj.hip), the one host read, then the key
// rows written -- into the caller's buffer, or into the dictionary's scratch and interned from there.
static int project_impl(fg_key_dict* d, bool intern, int32_t location, int64_t n, const uint8_t* bytes, int64_t nbytes,
                        const int64_t* offsets, const int32_t* lengths, const fg_row_projection* proj, uint8_t* out_key_bytes,
                        int64_t cap_bytes, int64_t* out_key_offsets, int32_t* out_key_lengths, int64_t* const* out_cols,
                        uint8_t* const* out_col_null, int64_t* out_nbytes, int64_t* out_id, int32_t* out_kg) {
    if (!d) return FG_EINVAL;
    const std::string who = intern ? "fg_key_dict_intern_fields" : "fg_key_dict_project";
    if (!proj) return d->fail(FG_EINVAL, who + ": a NULL projection");
    if (location != FG_HOST && location != FG_DEVICE) return d->fail(FG_EINVAL, who + ": unknown location");
    const bool host = location == FG_HOST;
    if (n < 0 || n > 0x7fffffff || nbytes < 0 ||
        (n > 0 && (!bytes || !offsets || !lengths ||
                   (intern ? !out_id : (!out_key_offsets || !out_key_lengths || !out_nbytes)))))
        return d->fail(FG_EINVAL, who + ": invalid arguments");
    if (proj->arity < 1 || proj->arity > 32767 || proj->n_key_fields < 1 || proj->n_key_fields > FG_PROJ_MAX_KEY_FIELDS ||
        proj->n_cols < 0 || proj->n_cols > FG_PROJ_MAX_COLS)
        return d->fail(FG_EINVAL, who + ": arity in [1, 32767], 1..8 key fields and 0..4 columns expected");
    ProjArgs a{};
    a.n = n;
    a.nbytes = nbytes;
    a.in_bits = ((proj->arity + 63 + 8) / 64) * 8;
    a.in_fixed = a.in_bits + 8 * proj->arity;
    a.k = proj->n_key_fields;
    a.n_cols = proj->n_cols;
    for (int f = 0; f < a.k; f++) {
        const int32_t kind = proj->key_kind[f];
        if (proj->key_field[f] < 0 || proj->key_field[f] >= proj->arity)
            return d->fail(FG_EINVAL, who + ": key field " + std::to_string(f) + " names no field of the input row");
        if (kind != FG_FIELD_FIX1 && kind != FG_FIELD_FIX2 && kind != FG_FIELD_FIX4 && kind != FG_FIELD_FIX8 &&
            kind != FG_FIELD_VAR)
            return d->fail(FG_EINVAL, who + ": key field " + std::to_string(f) + " has an unknown kind");
        a.key_field[f] = proj->key_field[f];
        a.key_kind[f] = kind;
    }
    if (n > 0 && a.n_cols > 0 && !out_cols) return d->fail(FG_EINVAL, who + ": a NULL out_cols");
    for (int c = 0; c < a.n_cols; c++) {
        if (proj->col_field[c] < 0 || proj->col_field[c] >= proj->arity)
            return d->fail(FG_EINVAL, who + ": column " + std::to_string(c) + " names no field of the input row");
        if (n > 0 && !out_cols[c]) return d->fail(FG_EINVAL, who + ": a NULL column in out_cols");   // (columns of no row may be NULL)
        a.col_field[c] = proj->col_field[c];
    }
    if (!intern && (cap_bytes < 0 || (cap_bytes > 0 && !out_key_bytes)))
        return d->fail(FG_EINVAL, who + ": invalid arguments");
    if (!host && ((uintptr_t)bytes % 8 != 0 || (!intern && (uintptr_t)out_key_bytes % 8 != 0)))
        return d->fail(FG_EINVAL, who + ": device records and a device out_key_bytes must be 8-byte aligned");
    if (d->pend.active) return d->fail(FG_ESTATE, who + ": an async intern is pending (fg_key_dict_intern_wait)");
    if (n == 0) {
        if (intern) return FG_OK;
        if (out_nbytes) *out_nbytes = 0;
        if (out_key_offsets && host) out_key_offsets[0] = 0;
        if (out_key_offsets && !host) {   // (a device word: the only device work of an empty call)
            if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
            DCHK(d, hipMemsetAsync(out_key_offsets, 0, 8, d->stream));
            DCHK(d, hipStreamSynchronize(d->stream));
        }
        return FG_OK;
    }
    if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
    hipStream_t s = d->stream;
    const int64_t nb = (n + kRowsBlock - 1) / kRowsBlock;
    DCHK(d, d->rows_ctr.ensure(sizeof(RowsCtr), s));
    DCHK(d, d->rows_sums.ensure(8 * (size_t)nb, s));
    if (host) {
        DCHK(d, d->pj_bytes.ensure((size_t)nbytes + 8, s));
        DCHK(d, d->pj_off.ensure(8 * (size_t)n, s));
        DCHK(d, d->pj_len.ensure(4 * (size_t)n, s));
        if (nbytes) DCHK(d, hipMemcpyAsync(d->pj_bytes.p, bytes, (size_t)nbytes, hipMemcpyHostToDevice, s));
        DCHK(d, hipMemcpyAsync(d->pj_off.p, offsets, 8 * (size_t)n, hipMemcpyHostToDevice, s));
        DCHK(d, hipMemcpyAsync(d->pj_len.p, lengths, 4 * (size_t)n, hipMemcpyHostToDevice, s));
        a.bytes = d->pj_bytes.as<uint8_t>();
        a.off = d->pj_off.as<int64_t>();
        a.len = d->pj_len.as<int32_t>();
        if (a.n_cols) {
            DCHK(d, d->pj_cols.ensure(8 * (size_t)n * a.n_cols, s));
            DCHK(d, d->pj_null.ensure((size_t)n * a.n_cols, s));
        }
    } else {
        a.bytes = bytes;
        a.off = offsets;
        a.len = lengths;
    }
    for (int c = 0; c < a.n_cols; c++) {
        uint8_t* cn = out_col_null ? out_col_null[c] : nullptr;
        a.out_col[c] = host ? d->pj_cols.as<int64_t>() + (size_t)c * n : out_cols[c];
        a.out_null[c] = !cn ? nullptr : host ? d->pj_null.as<uint8_t>() + (size_t)c * n : cn;
    }
    int64_t* koff = out_key_offsets;
    int32_t* klen = out_key_lengths;
    if (host || intern) {
        DCHK(d, d->pj_koff.ensure(8 * (size_t)(n + 1), s));
        DCHK(d, d->pj_klen.ensure(4 * (size_t)n, s));
        koff = d->pj_koff.as<int64_t>();
        klen = d->pj_klen.as<int32_t>();
    }
    // 1) the length pass; then the one host read of the call: {total, bad rows, lowest bad index}
    RowsCtr* rc = d->rows_ctr.as<RowsCtr>();
    DCHK(d, hipMemsetAsync(rc, 0, offsetof(RowsCtr, bad_first), s));
    DCHK(d, hipMemsetAsync(&rc->bad_first, 0xff, 8, s));
    if (d->timing) DCHK(d, hipEventRecord(d->ev[13], s));
    DCHK(d, keyproj_lengths_offsets(s, a, klen, koff, d->rows_sums.as<uint64_t>(), rc));
    if (d->timing) DCHK(d, hipEventRecord(d->ev[14], s));
    d->projected = true;
    RowsCtr hc;
    DCHK(d, hipMemcpyAsync(&hc, rc, sizeof hc, hipMemcpyDeviceToHost, s));
    DCHK(d, hipStreamSynchronize(s));
    float ms = 0.f;
    if (d->timing) DCHK(d, hipEventElapsedTime(&ms, d->ev[13], d->ev[14]));
    auto timed = [&](float t, int64_t written) {
        if (!d->timing) return;
        d->kstat[5].launches++;
        d->kstat[5].total_ms += t;
        d->kstat[5].records += n;
        d->kstat[5].rows += written;
    };
    if (hc.bad) {
        timed(ms, 0);
        return d->fail(FG_EINVAL, who + ": " + std::to_string(hc.bad) +
                                      " bad rows (an offset or length outside the buffer or not a multiple of 8, a row "
                                      "shorter than its fixed-length part, a variable-length key field outside its row, a "
                                      "key row above 2^24 - 4 bytes, or a NULL column without null bytes); the first at index " +
                                      std::to_string(hc.bad_first));
    }
    const int64_t total = (int64_t)hc.total;
    if (host) {   // straight into the caller's memory
        for (int c = 0; c < a.n_cols; c++) {
            DCHK(d, hipMemcpyAsync(out_cols[c], a.out_col[c], 8 * (size_t)n, hipMemcpyDeviceToHost, s));
            if (a.out_null[c]) DCHK(d, hipMemcpyAsync(out_col_null[c], a.out_null[c], (size_t)n, hipMemcpyDeviceToHost, s));
        }
        if (!intern) {
            DCHK(d, hipMemcpyAsync(out_key_offsets, koff, 8 * (size_t)(n + 1), hipMemcpyDeviceToHost, s));
            DCHK(d, hipMemcpyAsync(out_key_lengths, klen, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
        }
    }
    if (!intern) {
        *out_nbytes = total;
        if (total > cap_bytes) {
            if (host) DCHK(d, hipStreamSynchronize(s));
            timed(ms, 0);
            return d->fail(FG_EFULL, who + ": the key rows take " + std::to_string(total) + " bytes, out_key_bytes holds " +
                                         std::to_string(cap_bytes));
        }
    }
    // 2) the key rows: every row is good and the buffer holds `total` bytes (a key row has at least 16)
    uint8_t* kbytes = out_key_bytes;
    if (host || intern) {
        DCHK(d, d->pj_kbytes.ensure((size_t)total, s));
        kbytes = d->pj_kbytes.as<uint8_t>();
    }
    if (d->timing) DCHK(d, hipEventRecord(d->ev[15], s));
    DCHK(d, keyproj_write(s, a, koff, reinterpret_cast<uint64_t*>(kbytes), total >> 3));
    if (d->timing) DCHK(d, hipEventRecord(d->ev[16], s));
    if (host && !intern) DCHK(d, hipMemcpyAsync(out_key_bytes, kbytes, (size_t)total, hipMemcpyDeviceToHost, s));
    DCHK(d, hipStreamSynchronize(s));
    if (d->timing) {
        float ms2 = 0.f;
        DCHK(d, hipEventElapsedTime(&ms2, d->ev[15], d->ev[16]));
        ms += ms2;
    }
    timed(ms, total);
    if (!intern) return FG_OK;
    // 3) the key rows interned where they lie
    int64_t* ids = out_id;
    int32_t* kg = out_kg;
    if (host) {
        DCHK(d, d->pj_ids.ensure(8 * (size_t)n, s));
        ids = d->pj_ids.as<int64_t>();
        if (out_kg) {
            DCHK(d, d->pj_kg.ensure(4 * (size_t)n, s));
            kg = d->pj_kg.as<int32_t>();
        }
    }
    if (int rc1 = intern_begin(d, FG_DEVICE, n, kbytes, total, koff, klen, ids, kg)) return rc1;
    if (int rc2 = intern_finish(d)) return rc2;
    if (host) {
        DCHK(d, hipMemcpy(out_id, ids, 8 * (size_t)n, hipMemcpyDeviceToHost));
        if (out_kg) DCHK(d, hipMemcpy(out_kg, kg, 4 * (size_t)n, hipMemcpyDeviceToHost));
    }
    return FG_OK;
}

int fg_key_dict_project(fg_key_dict* d, int32_t location, int64_t n, const uint8_t* bytes, int64_t nbytes,
                        const int64_t* offsets, const int32_t* lengths, const fg_row_projection* proj, uint8_t* out_key_bytes,
                        int64_t cap_bytes, int64_t* out_key_offsets, int32_t* out_key_lengths, int64_t* const* out_cols,
                        uint8_t* const* out_col_null, int64_t* out_nbytes) {
    return project_impl(d, false, location, n, bytes, nbytes, offsets, lengths, proj, out_key_bytes, cap_bytes,
                        out_key_offsets, out_key_lengths, out_cols, out_col_null, out_nbytes, nullptr, nullptr);
}

int fg_key_dict_intern_fields(fg_key_dict* d, int32_t location, int64_t n, const uint8_t* bytes, int64_t nbytes,
                              const int64_t* offsets, const int32_t* lengths, const fg_row_projection* proj, int64_t* out_id,
                              int32_t* out_kg, int64_t* const* out_cols, uint8_t* const* out_col_null) {
    return project_impl(d, true, location, n, bytes, nbytes, offsets, lengths, proj, nullptr, 0, nullptr, nullptr, out_cols,
                        out_col_null, nullptr, out_id, out_kg);
}

int fg_key_dict_get_stats(fg_key_dict* d, fg_key_dict_stats* out) {
    if (!d || !out) return FG_EINVAL;
    out->live = d->live();
    out->issued = d->nids;
    out->free_ordinals = d->nfree - d->free_taken;
    out->arena_bytes = d->arena_used;
    out->table_slots = (int64_t)d->cap;
    out->side_rows = (int64_t)d->side.size();
    out->retired_total = d->retired_total;
    out->reserved0 = 0;
    return FG_OK;
}

int fg_key_dict_retain(fg_key_dict* d, int32_t location, int32_t n_sets, const int64_t* const* ids, const int64_t* counts,
                       fg_key_dict_stats* out) {
    if (!d) return FG_EINVAL;
    if (location != FG_HOST && location != FG_DEVICE) return d->fail(FG_EINVAL, "fg_key_dict_retain: unknown location");
    if (n_sets < 0 || n_sets > 16 || (n_sets > 0 && (!ids || !counts)))
        return d->fail(FG_EINVAL, "fg_key_dict_retain: 0..16 sets of ids expected");
    int64_t n = 0;
    for (int k = 0; k < n_sets; k++) {
        if (counts[k] < 0 || counts[k] > 0x7fffffff || (counts[k] > 0 && !ids[k]))
            return d->fail(FG_EINVAL,
                           "fg_key_dict_retain: set " + std::to_string(k) + ": a count in [0, 2^31) and its ids expected");
        n += counts[k];
    }
    if (d->pend.active) return d->fail(FG_ESTATE, "fg_key_dict_retain: an async intern is pending (fg_key_dict_intern_wait)");
    if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
    hipStream_t s = d->stream;
    const bool host = location == FG_HOST;
    const int64_t issued = d->nids;
    const int64_t nb = (issued + kRowsBlock - 1) / kRowsBlock;
    // 1) mark and plan: scratch only -- the dictionary is read, not written
    DCHK(d, d->ret_mark.ensure((size_t)std::max<int64_t>(issued, 1), s));
    DCHK(d, d->ret_ctr.ensure(sizeof(RetCtr), s));
    DCHK(d, d->rows_sums.ensure(16 * (size_t)std::max<int64_t>(nb, 1), s));
    if (host && n) DCHK(d, d->rows_ids.ensure(8 * (size_t)n, s));
    uint8_t* mark = d->ret_mark.as<uint8_t>();
    RetCtr* rc = d->ret_ctr.as<RetCtr>();
    uint64_t* sums = d->rows_sums.as<uint64_t>();
    DCHK(d, hipMemsetAsync(mark, 0, (size_t)std::max<int64_t>(issued, 1), s));
    DCHK(d, hipMemsetAsync(rc, 0, sizeof(RetCtr), s));
    DCHK(d, hipMemsetAsync(&rc->bad_first, 0xff, 8, s));
    if (d->timing) DCHK(d, hipEventRecord(d->ev[7], s));
    int64_t at = 0;
    for (int k = 0; k < n_sets; k++) {
        if (!counts[k]) continue;
        const int64_t* di = ids[k];
        if (host) {
            DCHK(d, hipMemcpyAsync(d->rows_ids.as<int64_t>() + at, ids[k], 8 * (size_t)counts[k], hipMemcpyHostToDevice, s));
            di = d->rows_ids.as<int64_t>() + at;
            at += counts[k];
        }
        hipLaunchKernelGGL(k_retain_mark, dim3(grid_of(counts[k])), dim3(kDictThreads), 0, s, d->dev(), issued, counts[k], di,
                           (int32_t)k, mark, rc);
    }
    if (nb) {
        hipLaunchKernelGGL(k_retain_sums, dim3((unsigned)nb), dim3(kDictThreads), 0, s, d->dev(), issued, (const uint8_t*)mark,
                           sums, nb);
        hipLaunchKernelGGL(k_retain_scan_sums, dim3(1), dim3(kDictThreads), 0, s, sums, nb, rc);
    }
    if (d->timing) DCHK(d, hipEventRecord(d->ev[8], s));
    DCHK(d, hipGetLastError());
    RetCtr hc;   // the one host read: bad ids, the new arena's size, the dead ordinals
    DCHK(d, hipMemcpyAsync(&hc, rc, sizeof hc, hipMemcpyDeviceToHost, s));
    DCHK(d, hipStreamSynchronize(s));
    float ms = 0.f;
    if (d->timing) DCHK(d, hipEventElapsedTime(&ms, d->ev[7], d->ev[8]));
    auto timed = [&](float t, int64_t kept) {
        if (!d->timing) return;
        d->kstat[3].launches++;
        d->kstat[3].total_ms += t;
        d->kstat[3].records += issued;
        d->kstat[3].rows += kept;
    };
    if (hc.bad) {
        timed(ms, 0);
        return d->fail(FG_EINVAL, "fg_key_dict_retain: " + std::to_string(hc.bad) +
                                      " ids name no live entry (negative, never issued, retired, or stale); the first at set " +
                                      std::to_string(hc.bad_first >> 32) + " index " +
                                      std::to_string(hc.bad_first & 0xffffffffull) + "; the dictionary is unchanged");
    }
    const int64_t dead = (int64_t)hc.dead, kept = issued - dead;
    const int64_t before = d->live();
    // 2) everything the new state needs is allocated before anything is modified
    const uint64_t ncap =
        std::min<uint64_t>(d->cap, std::max<uint64_t>(d->cap0, pow2_at_least(FG_DICT_GROW * (uint64_t)(kept + (1 << 20)))));
    std::vector<int64_t> side_ord;
    std::vector<std::unordered_map<std::string, int64_t>::iterator> side_it;
    for (auto it = d->side.begin(); it != d->side.end(); ++it) {
        side_ord.push_back((int64_t)((uint64_t)it->second >> dict_kg_bits(d->max_p)));
        side_it.push_back(it);
    }
    const int64_t nside = (int64_t)side_ord.size();
    Buf narena, nslots, nrow, nfree;
    DCHK(d, narena.ensure((size_t)hc.bytes + 16, s));
    DCHK(d, nslots.ensure(sizeof(Slot) * ncap, s));
    DCHK(d, nrow.ensure(4 * ncap, s));
    DCHK(d, nfree.ensure(8 * (size_t)std::max<int64_t>(dead, 1), s));
    if (nside) DCHK(d, d->ret_side.ensure(12 * (size_t)nside, s));
    // 3) compact, rebuild, side rows
    if (d->timing) DCHK(d, hipEventRecord(d->ev[9], s));
    if (nb)
        hipLaunchKernelGGL(k_retain_compact, dim3((unsigned)nb), dim3(kDictThreads), 0, s, d->dev(), issued, (const uint8_t*)mark,
                           (const uint64_t*)sums, nb, narena.as<uint64_t>(), nfree.as<int64_t>());
    if (d->timing) DCHK(d, hipEventRecord(d->ev[11], s));
    hipLaunchKernelGGL(k_slots_clear, dim3(grid_of((int64_t)ncap)), dim3(kDictThreads), 0, s, nslots.as<Slot>(), (int64_t)ncap);
    auto swap = [](Buf& a, Buf& b) {
        std::swap(a.p, b.p);
        std::swap(a.bytes, b.bytes);
    };
    swap(d->arena, narena);   // (the old ones are freed on return: the stream is idle by then)
    swap(d->slots, nslots);
    swap(d->slot_row, nrow);
    swap(d->free_ord, nfree);
    d->cap = ncap;
    d->arena_used = (int64_t)hc.bytes;
    d->nfree = dead;
    d->free_taken = 0;
    d->retired_total += before - kept;
    if (issued) hipLaunchKernelGGL(k_dict_rehash, dim3(grid_of(issued)), dim3(kDictThreads), 0, s, d->dev(), issued);
    if (d->timing) DCHK(d, hipEventRecord(d->ev[12], s));
    int64_t* side_dev = d->ret_side.as<int64_t>();
    int32_t* state_dev = reinterpret_cast<int32_t*>(side_dev + nside);
    if (nside) {
        DCHK(d, hipMemcpyAsync(side_dev, side_ord.data(), 8 * (size_t)nside, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_retain_side, dim3(grid_of(nside)), dim3(kDictThreads), 0, s, d->dev(), d->tag_bits, nside,
                           (const int64_t*)side_dev, state_dev);
    }
    if (d->timing) DCHK(d, hipEventRecord(d->ev[10], s));
    DCHK(d, hipGetLastError());
    const unsigned long long c2[2] = {(unsigned long long)issued, hc.bytes}, zero = 0;
    unsigned long long* ctr = d->counters.as<unsigned long long>();
    DCHK(d, hipMemcpyAsync(ctr, c2, sizeof c2, hipMemcpyHostToDevice, s));
    DCHK(d, hipMemcpyAsync(ctr + 7, &zero, 8, hipMemcpyHostToDevice, s));
    std::vector<int32_t> state((size_t)nside);
    if (nside) DCHK(d, hipMemcpyAsync(state.data(), state_dev, 4 * (size_t)nside, hipMemcpyDeviceToHost, s));
    DCHK(d, hipStreamSynchronize(s));
    for (int64_t i = 0; i < nside; i++)   // retired side rows leave the map, and those the table holds now
        if (state[i] != 1) d->side.erase(side_it[i]);
    if (d->timing) {
        float ms2 = 0.f;
        DCHK(d, hipEventElapsedTime(&ms2, d->ev[9], d->ev[10]));
        ms += ms2;
        DCHK(d, d->rebuilt());
    }
    timed(ms, kept);
    if (out) return fg_key_dict_get_stats(d, out);
    return FG_OK;
}

int fg_partition_keyed_by_owner(fg_key_dict* d, void* stream, int64_t n, int32_t ncols, const int64_t* const* cols,
                                int32_t parallelism, int64_t* const* out_cols, int64_t* counts, int32_t* out_key_lengths,
                                uint8_t* out_key_bytes, int64_t cap_bytes, int64_t* out_byte_counts, int64_t* out_nbytes) {
    if (!d) return FG_EINVAL;
    if (cap_bytes < 0 || (cap_bytes > 0 && !out_key_bytes))
        return d->fail(FG_EINVAL, "fg_partition_keyed_by_owner: invalid arguments");
    if ((uintptr_t)out_key_bytes % 8 != 0)
        return d->fail(FG_EINVAL, "fg_partition_keyed_by_owner: out_key_bytes must be 8-byte aligned");
    struct Fixed {
        uint8_t* p;
        int64_t cap;
    } fixed{out_key_bytes, cap_bytes};
    auto take = [](void* ctx, int64_t nbytes) -> uint8_t* {
        const Fixed* f = static_cast<const Fixed*>(ctx);
        return nbytes <= f->cap ? f->p : nullptr;
    };
    return keydict_partition_keyed(d, static_cast<hipStream_t>(stream), n, ncols, cols, parallelism, out_cols, counts,
                                   out_key_lengths, take, &fixed, out_byte_counts, out_nbytes);
}

int fg_key_dict_arena(fg_key_dict* d, const uint8_t** dev_bytes, int64_t* size) {
    if (!d || !dev_bytes || !size) return FG_EINVAL;
    *dev_bytes = d->arena.as<uint8_t>();
    *size = d->arena_used;
    return FG_OK;
}

int fg_key_dict_copy_arena(fg_key_dict* d, int64_t begin, int64_t nbytes, uint8_t* host) {
    if (d && d->pend.active)
        return d->fail(FG_ESTATE, "fg_key_dict_copy_arena: an async intern is pending (fg_key_dict_intern_wait)");
    if (!d || begin < 0 || nbytes < 0 || begin + nbytes > d->arena_used || (nbytes && !host))
        return d ? d->fail(FG_EINVAL, "fg_key_dict_copy_arena: range outside the arena") : FG_EINVAL;
    if (!nbytes) return FG_OK;
    if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
    DCHK(d, hipMemcpy(host, d->arena.as<uint8_t>() + begin, (size_t)nbytes, hipMemcpyDeviceToHost));
    return FG_OK;
}

int64_t fg_key_dict_size(fg_key_dict* d) { return d ? d->live() : -1; }

void* fg_key_dict_stream(fg_key_dict* d) { return d ? (void*)d->stream : nullptr; }

int fg_key_dict_set_timing(fg_key_dict* d, int32_t on) {
    if (!d) return FG_EINVAL;
    if (on && !d->ev[0]) {
        if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
        for (auto& e : d->ev) DCHK(d, hipEventCreate(&e));
        std::snprintf(d->kstat[0].name, sizeof d->kstat[0].name, "dict_probe");
        std::snprintf(d->kstat[1].name, sizeof d->kstat[1].name, "dict_assign");
        std::snprintf(d->kstat[2].name, sizeof d->kstat[2].name, "dict_rows");
        std::snprintf(d->kstat[3].name, sizeof d->kstat[3].name, "dict_retain");
        std::snprintf(d->kstat[4].name, sizeof d->kstat[4].name, "dict_rebuild");
        std::snprintf(d->kstat[5].name, sizeof d->kstat[5].name, "dict_project");
    }
    d->timing = on != 0;
    return FG_OK;
}

int fg_key_dict_kernel_stats(fg_key_dict* d, fg_kernel_stat* out, int32_t max, int32_t* count) {
    if (!d || !count || (max > 0 && !out)) return FG_EINVAL;
    *count = d->ev[0] ? (d->projected ? 6 : 5) : 0;   // ("dict_project" only once the dictionary has projected)
    for (int i = 0; i < *count && i < max; i++) out[i] = d->kstat[i];
    return FG_OK;
}

const char* fg_key_dict_last_error(fg_key_dict* d) { return d ? d->err.c_str() : "null dictionary"; }

void fg_key_dict_close(fg_key_dict* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    hipStream_t s = d->stream;
    if (s) (void)hipStreamSynchronize(s);
    for (auto e : d->ev)
        if (e) (void)hipEventDestroy(e);
    if (d->ev_order) (void)hipEventDestroy(d->ev_order);
    delete d;
    if (s) (void)hipStreamDestroy(s);
}

int32_t fg_binaryrow_hash(const uint8_t* row, int32_t len) {
    if (!row || len < 0 || (len & 3)) return 0;
    return binaryrow_hash_bytes(row, len);
}

}  // extern "C"

namespace fg {

int32_t keydict_max_parallelism(const fg_key_dict* d) { return d ? d->max_p : 0; }
int32_t keydict_device(const fg_key_dict* d) { return d ? d->device : -1; }

int keydict_partition_keyed(fg_key_dict* d, hipStream_t s, int64_t n, int32_t ncols, const int64_t* const* cols,
                            int32_t parallelism, int64_t* const* out_cols, int64_t* counts, int32_t* out_key_lengths,
                            keydict_bytes_fn key_bytes, void* ctx, int64_t* out_byte_counts, int64_t* out_nbytes) {
    if (!d) return FG_EINVAL;
    if (n < 0 || n > 0x7fffffff || ncols < 1 || ncols > kMaxOwnerCols || parallelism < 1 ||
        parallelism > std::min(1024, d->max_p) || !key_bytes)
        return d->fail(FG_EINVAL, "fg_partition_keyed_by_owner: n in [0, 2^31), 1..8 columns and a parallelism in "
                                  "[1, min(1024, the dictionary's max parallelism)] expected");
    bool null_arg = n > 0 && (!cols || !out_cols || !counts || !out_key_lengths || !out_byte_counts || !out_nbytes);
    for (int j = 0; !null_arg && n > 0 && j < ncols; j++) null_arg = !cols[j] || !out_cols[j];
    if (null_arg) return d->fail(FG_EINVAL, "fg_partition_keyed_by_owner: a NULL column or output");
    if (d->pend.active)
        return d->fail(FG_ESTATE, "fg_partition_keyed_by_owner: an async intern is pending (fg_key_dict_intern_wait)");
    if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
    if (n == 0) {
        if (out_nbytes) *out_nbytes = 0;
        if (counts) DCHK(d, hipMemsetAsync(counts, 0, 8 * (size_t)parallelism, s));
        if (out_byte_counts) DCHK(d, hipMemsetAsync(out_byte_counts, 0, 8 * (size_t)parallelism, s));
        DCHK(d, hipStreamSynchronize(s));
        return FG_OK;
    }
    // after everything queued on the dictionary's stream (an intern's writes to the arena)
    if (s != d->stream) {
        if (!d->ev_order) DCHK(d, hipEventCreateWithFlags(&d->ev_order, hipEventDisableTiming));
        DCHK(d, hipEventRecord(d->ev_order, d->stream));
        DCHK(d, hipStreamWaitEvent(s, d->ev_order, 0));
    }
    // 1) the owner partition of the columns (an id carries its key group: FG_KEYHASH_DICT_ID)
    const size_t words = partition_scratch_words(n, parallelism);
    DCHK(d, d->part_scratch.ensure(4 * words, s));
    DCHK(d, d->rows_off.ensure(8 * (size_t)(n + 1), s));
    OwnerCols oc{};
    oc.ncols = ncols;
    for (int j = 0; j < ncols; j++) {
        oc.in[j] = cols[j];
        oc.out[j] = out_cols[j];
    }
    DCHK(d, launch_partition_cols_by_owner(oc, n, FG_KEYHASH_DICT_ID, d->max_p, parallelism, counts,
                                           d->part_scratch.as<uint32_t>(), words, s));
    // 2) the key rows of the grouped ids: lengths, offsets, the bytes per owner; one host read
    int64_t* off = d->rows_off.as<int64_t>();
    if (int rc = rows_lengths_offsets(d, s, n, out_cols[0], out_key_lengths, off)) return rc;
    hipLaunchKernelGGL(k_owner_byte_counts, dim3(1), dim3(kDictThreads), 0, s, (const int64_t*)counts, parallelism,
                       (const int64_t*)off, n, out_byte_counts);
    DCHK(d, hipGetLastError());
    RowsCtr hc;
    DCHK(d, hipMemcpyAsync(&hc, d->rows_ctr.p, sizeof hc, hipMemcpyDeviceToHost, s));
    DCHK(d, hipStreamSynchronize(s));
    float ms = 0.f;
    if (d->timing) DCHK(d, hipEventElapsedTime(&ms, d->ev[3], d->ev[4]));
    auto timed = [&](float t) {
        if (!d->timing) return;
        d->kstat[2].launches++;
        d->kstat[2].total_ms += t;
        d->kstat[2].records += n;
    };
    if (hc.bad) {
        timed(ms);
        return d->fail(FG_EINVAL, "fg_partition_keyed_by_owner: " + std::to_string(hc.bad) +
                                      " unknown ids (negative, or not below the dictionary's size); the first at "
                                      "grouped index " + std::to_string(hc.bad_first));
    }
    const int64_t total = (int64_t)hc.total;
    *out_nbytes = total;
    if (total > 0) {
        uint8_t* out = key_bytes(ctx, total);
        if (!out) {
            timed(ms);
            return d->fail(FG_EFULL, "fg_partition_keyed_by_owner: the key rows take " + std::to_string(total) +
                                         " bytes, more than out_key_bytes holds");
        }
        // 3) the copy: every id is good and the buffer holds `total` bytes
        if (int rc = rows_copy(d, s, n, out_cols[0], off, out, total)) return rc;
        DCHK(d, hipStreamSynchronize(s));
        if (d->timing) {
            float ms2 = 0.f;
            DCHK(d, hipEventElapsedTime(&ms2, d->ev[5], d->ev[6]));
            ms += ms2;
        }
    }
    timed(ms);
    return FG_OK;
}

int keydict_intern_packed(fg_key_dict* d, hipEvent_t ready, int64_t n, const int32_t* lengths, const uint8_t* bytes,
                          int64_t nbytes, int64_t* out_ids) {
    if (!d) return FG_EINVAL;
    if (n < 0 || n > 0x7fffffff || nbytes < 0 || (n > 0 && (!lengths || !out_ids)) || (nbytes > 0 && !bytes) ||
        (uintptr_t)bytes % 8 != 0)
        return d->fail(FG_EINVAL, "key rows received: invalid arguments");
    if (d->pend.active) return d->fail(FG_ESTATE, "key rows received: an async intern is pending (fg_key_dict_intern_wait)");
    if (n == 0)
        return nbytes == 0 ? FG_OK : d->fail(FG_EDEVICE, "key rows received: " + std::to_string(nbytes) + " bytes for no row");
    if (hipSetDevice(d->device) != hipSuccess) return d->fail(FG_EDEVICE, "hipSetDevice failed");
    hipStream_t s = d->stream;
    if (ready) DCHK(d, hipStreamWaitEvent(s, ready, 0));
    const int64_t nb = (n + kRowsBlock - 1) / kRowsBlock;
    DCHK(d, d->rows_ctr.ensure(sizeof(RowsCtr), s));
    DCHK(d, d->rows_sums.ensure(8 * (size_t)nb, s));
    DCHK(d, d->rows_off.ensure(8 * (size_t)(n + 1), s));
    RowsCtr* rc = d->rows_ctr.as<RowsCtr>();
    uint64_t* sums = d->rows_sums.as<uint64_t>();
    int64_t* off = d->rows_off.as<int64_t>();
    DCHK(d, hipMemsetAsync(rc, 0, offsetof(RowsCtr, bad_first), s));
    DCHK(d, hipMemsetAsync(&rc->bad_first, 0xff, 8, s));
    hipLaunchKernelGGL(k_recv_lengths, dim3((unsigned)nb), dim3(kDictThreads), 0, s, n, lengths, sums, rc);
    hipLaunchKernelGGL(k_rows_scan_sums, dim3(1), dim3(kDictThreads), 0, s, sums, nb, rc, off, n);
    hipLaunchKernelGGL(k_rows_offsets, dim3((unsigned)nb), dim3(kDictThreads), 0, s, n, lengths, (const uint64_t*)sums, off);
    DCHK(d, hipGetLastError());
    RowsCtr hc;
    DCHK(d, hipMemcpyAsync(&hc, rc, sizeof hc, hipMemcpyDeviceToHost, s));
    DCHK(d, hipStreamSynchronize(s));
    if (hc.bad)
        return d->fail(FG_EDEVICE, "key rows received: " + std::to_string(hc.bad) +
                                       " lengths negative, not a multiple of 4 or >= 2^24; the first at row " +
                                       std::to_string(hc.bad_first));
    if ((int64_t)hc.total != nbytes)
        return d->fail(FG_EDEVICE, "key rows received: the lengths add up to " + std::to_string(hc.total) + " bytes, " +
                                       std::to_string(nbytes) + " were received");
    if (!bytes) {   // (only empty rows: the intern still wants a buffer to point at)
        DCHK(d, d->rows_bytes.ensure(8, s));
        bytes = d->rows_bytes.as<uint8_t>();
    }
    if (int rc2 = intern_begin(d, FG_DEVICE, n, bytes, nbytes, off, lengths, out_ids, nullptr)) return rc2;
    return intern_finish(d);
}

}  // namespace fg
