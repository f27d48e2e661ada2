// fg_keyproj.hip -- the key selector on the GPU: the key rows of packed BinaryRowData records, for
// fg_key_dict_project / fg_key_dict_intern_fields of include/flinkgpu.h (their host side lives with
// the dictionary, fg_keydict.hip).
//
// The reference's BinaryRowDataKeySelector.getKey (TR/keyselector/BinaryRowDataKeySelector.java:43-50)
// runs a generated projection that writes the key fields of a record through BinaryRowWriter into a
// fresh row; fg_key_dict_intern groups by that row's bytes. Here the projection runs over a whole
// batch of serialized records: k_proj_lengths validates every record and sizes its key row (and
// copies the 8-byte columns out: rowtime, value), the scan of fg_rows_scan.h turns the lengths into
// offsets, the host reads {total, bad rows} once, and k_proj_write writes the key rows -- byte for
// byte what BinaryRowWriter writes (writer/BinaryRowWriter.java, AbstractBinaryWriter.java:81-105,
// 280-330): RowKind INSERT, a null bit and a zero slot per NULL field, fixed-length fields narrowed
// to their width, a CHAR/VARCHAR/BINARY field of up to 7 bytes inline in its slot (0x80 | len in the
// top byte) and a longer one in the variable part, zero-padded to 8, the slot holding
// offset << 32 | len.
#include <hip/hip_runtime.h>

#include "fg_keyproj.h"

namespace fg {
namespace {

constexpr int kProjBlock = kScanThreads;   // rows per scan block = rows per write workgroup
constexpr uint64_t kMaxKeyRow = (1u << 24) - 4;   // the intern's limit on a row's length

__device__ __forceinline__ uint64_t load_u64(const uint8_t* p) { return *reinterpret_cast<const uint64_t*>(p); }
__device__ __forceinline__ uint64_t low_bytes(uint64_t v, uint32_t nbytes) {   // nbytes 0..7
    return v & ((1ull << (8 * nbytes)) - 1);
}
__device__ __forceinline__ uint64_t pad8(uint32_t len) { return ((uint64_t)len + 7) & ~7ull; }

// is field `field` of the row at `row` NULL (bit 8 + field of the bit set; byte 0 is the RowKind)
__device__ __forceinline__ bool field_is_null(const uint8_t* row, int32_t field) {
    const uint32_t b = 8u + (uint32_t)field;
    return load_u64(row + 8 * (b >> 6)) >> (b & 63) & 1;
}

// A variable-length field's slot: inline (top bit set: len in bits 56..62, data in the low bytes)
// or offset << 32 | len, the offset from the row's start. src 0: inline.
struct VarField {
    uint32_t len, src;
    bool bad;
};
__device__ __forceinline__ VarField decode_var(uint64_t slot, int32_t row_len, int32_t in_fixed) {
    VarField v;
    if (slot >> 63) {
        v.len = (uint32_t)(slot >> 56) & 0x7f;
        v.src = 0;
        v.bad = v.len > 7;
    } else {
        v.len = (uint32_t)slot;
        v.src = (uint32_t)(slot >> 32);
        v.bad = (v.src & 7) != 0 || v.src < (uint32_t)in_fixed || (uint64_t)v.src + v.len > (uint64_t)row_len;
    }
    return v;
}

// One lane per input row: the row validated (inside the buffer, multiples of 8, at least the
// fixed-length part; every non-NULL variable-length key field inside the row), the length of its
// key row, the columns. Nothing is read through an offset before it is checked. Bad rows take one
// atomic pair per wave; each block's padded bytes go to sums.
__global__ __launch_bounds__(kScanThreads) void k_proj_lengths(ProjArgs a, int32_t* key_len, uint64_t* sums, RowsCtr* rc) {
    __shared__ uint64_t s_wave[kScanThreads / 64];
    const int64_t i = (int64_t)blockIdx.x * kProjBlock + threadIdx.x;
    const bool valid = i < a.n;
    const int64_t off = valid ? a.off[i] : 0;
    const int32_t len = valid ? a.len[i] : 0;
    // the row's fixed-length part can be read: the bit set and every slot lie inside the buffer
    const bool readable = valid && off >= 0 && (off & 7) == 0 && (len & 7) == 0 && len >= a.in_fixed && off <= a.nbytes &&
                          (int64_t)len <= a.nbytes - off;
    bool ok = readable;
    const uint8_t* row = a.bytes + (readable ? off : 0);
    uint64_t klen = 8ull * (uint32_t)(a.k + 1);
    if (readable) {
        for (int f = 0; f < a.k; f++) {
            if (a.key_kind[f] != FG_FIELD_VAR || field_is_null(row, a.key_field[f])) continue;
            const VarField v = decode_var(load_u64(row + a.in_bits + 8 * a.key_field[f]), len, a.in_fixed);
            if (v.bad) ok = false;
            else if (v.len > 7) klen += pad8(v.len);
        }
        if (klen > kMaxKeyRow) ok = false;
    }
    for (int c = 0; c < a.n_cols; c++) {
        uint64_t v = 0;
        bool null = false;
        if (readable) {
            null = field_is_null(row, a.col_field[c]);
            if (!null) v = load_u64(row + a.in_bits + 8 * a.col_field[c]);
            if (null && !a.out_null[c]) ok = false;
        }
        if (valid) {
            a.out_col[c][i] = (int64_t)v;
            if (a.out_null[c]) a.out_null[c][i] = null ? 1 : 0;
        }
    }
    if (valid) key_len[i] = ok ? (int32_t)klen : -1;
    const unsigned long long badm = __ballot(valid && !ok);
    if (badm && (threadIdx.x & 63) == 0) {
        atomicAdd(&rc->bad, (unsigned long long)__popcll(badm));
        atomicMin(&rc->bad_first, (unsigned long long)(i + __ffsll((long long)badm) - 1));
    }
    uint64_t total;
    (void)block_exclusive_scan_u64(ok ? klen : 0ull, s_wave, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// The write, balanced by bytes like k_rows_copy: a workgroup owns kProjBlock consecutive rows, whose
// key rows [key_off[r0], key_off[r0 + m]) are contiguous. Each thread first stages its own row in
// LDS, field-major so that consecutive lanes touch consecutive words: the header word, per key field
// the finished slot word (a NULL's zero, the narrowed fixed-length value, the inline string, or
// offset << 32 | len into the key row's variable part) and, for a field that goes to the variable
// part, where its bytes start in the input row. The threads then stride over the span's 8-byte
// words: a word finds its row by binary search over the run's offsets and is the header word, a slot
// word, or a word of one field's variable part -- loaded whole from the input (8-byte aligned: the
// length pass checked it) and masked by the field's length where it is the last one. The stores are
// coalesced, and a 70,000-byte string is copied by the whole workgroup. Launched only after the host
// has seen every row good and the total within the buffer.
__global__ __launch_bounds__(kScanThreads) void k_proj_write(ProjArgs a, const int64_t* key_off, uint64_t* out,
                                                             int64_t out_words) {
    __shared__ int64_t s_off[kProjBlock + 1];
    __shared__ int64_t s_in[kProjBlock];
    __shared__ uint64_t s_hdr[kProjBlock];
    __shared__ uint64_t s_slot[FG_PROJ_MAX_KEY_FIELDS * kProjBlock];
    __shared__ uint32_t s_vsrc[FG_PROJ_MAX_KEY_FIELDS * kProjBlock];
    const int64_t r0 = (int64_t)blockIdx.x * kProjBlock;
    const int m = (int)(a.n - r0 < kProjBlock ? a.n - r0 : kProjBlock);
    const int t = (int)threadIdx.x;
    if (t < m) {
        const int64_t off = a.off[r0 + t];
        const uint8_t* row = a.bytes + off;
        s_off[t] = key_off[r0 + t];
        s_in[t] = off;
        uint64_t hdr = 0;                           // byte 0: RowKind INSERT
        uint64_t cursor = 8ull * (uint32_t)(a.k + 1);   // where the next variable-length field goes
        for (int f = 0; f < a.k; f++) {
            const int32_t field = a.key_field[f], kind = a.key_kind[f];
            uint64_t slot = 0;
            uint32_t vsrc = 0;
            if (field_is_null(row, field)) {
                hdr |= 1ull << (8 + f);
            } else {
                const uint64_t in = load_u64(row + a.in_bits + 8 * field);
                if (kind != FG_FIELD_VAR) {
                    slot = kind == FG_FIELD_FIX8 ? in : low_bytes(in, (uint32_t)kind);
                } else {
                    const VarField v = decode_var(in, 0x7fffffff, 0);
                    if (v.len <= 7) {   // inline, wherever the input kept it
                        const uint64_t data = v.src == 0 ? in : (v.len ? load_u64(row + v.src) : 0ull);
                        slot = (uint64_t)(0x80u | v.len) << 56 | low_bytes(data, v.len);
                    } else {
                        slot = cursor << 32 | v.len;
                        vsrc = v.src;
                        cursor += pad8(v.len);
                    }
                }
            }
            s_slot[f * kProjBlock + t] = slot;
            s_vsrc[f * kProjBlock + t] = vsrc;
        }
        s_hdr[t] = hdr;
    }
    if (t == 0) s_off[m] = key_off[r0 + m];
    __syncthreads();
    const int64_t w1 = s_off[m] >> 3 < out_words ? s_off[m] >> 3 : out_words;
    const uint32_t fixed_words = (uint32_t)a.k + 1;
    for (int64_t w = (s_off[0] >> 3) + t; w < w1; w += kScanThreads) {
        const int64_t b = w << 3;
        int lo = 0, hi = m;   // s_off[lo] <= b < s_off[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= b) lo = mid; else hi = mid;
        }
        const uint32_t rel = (uint32_t)(b - s_off[lo]);   // byte of the key row (< 2^24)
        uint64_t v = 0;
        if (rel == 0) {
            v = s_hdr[lo];
        } else if ((rel >> 3) < fixed_words) {
            v = s_slot[((rel >> 3) - 1) * kProjBlock + lo];
        } else {
            for (int f = 0; f < a.k; f++) {
                const uint32_t vsrc = s_vsrc[f * kProjBlock + lo];
                if (!vsrc) continue;
                const uint64_t slot = s_slot[f * kProjBlock + lo];
                const uint32_t vo = (uint32_t)(slot >> 32), vl = (uint32_t)slot;
                if (rel >= vo + pad8(vl)) continue;   // (fields follow each other: the first that ends past rel)
                const uint32_t at = rel - vo;
                v = load_u64(a.bytes + s_in[lo] + vsrc + at);
                if (vl - at < 8) v = low_bytes(v, vl - at);
                break;
            }
        }
        out[w] = v;
    }
}

}  // namespace

hipError_t keyproj_lengths_offsets(hipStream_t s, const ProjArgs& a, int32_t* key_len, int64_t* key_off, uint64_t* sums,
                                   RowsCtr* rc) {
    const int64_t nb = (a.n + kProjBlock - 1) / kProjBlock;
    hipLaunchKernelGGL(k_proj_lengths, dim3((unsigned)nb), dim3(kScanThreads), 0, s, a, key_len, sums, rc);
    hipLaunchKernelGGL(k_rows_scan_sums, dim3(1), dim3(kScanThreads), 0, s, sums, nb, rc, key_off, a.n);
    hipLaunchKernelGGL(k_rows_offsets, dim3((unsigned)nb), dim3(kScanThreads), 0, s, a.n, (const int32_t*)key_len,
                       (const uint64_t*)sums, key_off);
    return hipGetLastError();
}

hipError_t keyproj_write(hipStream_t s, const ProjArgs& a, const int64_t* key_off, uint64_t* out, int64_t out_words) {
    const int64_t nb = (a.n + kProjBlock - 1) / kProjBlock;
    hipLaunchKernelGGL(k_proj_write, dim3((unsigned)nb), dim3(kScanThreads), 0, s, a, key_off, out, out_words);
    return hipGetLastError();
}

}  // namespace fg
