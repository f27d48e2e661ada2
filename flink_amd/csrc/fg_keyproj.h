// fg_keyproj.h -- the key selector's kernels (fg_keyproj.hip) as fg_keydict.hip launches them for
// fg_key_dict_project / fg_key_dict_intern_fields.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/flinkgpu.h"
#include "fg_rows_scan.h"

namespace fg {

// One projection call on the device: the input records, the checked projection and the outputs of
// the length pass. Every pointer is device memory; bytes is 8-byte aligned.
struct ProjArgs {
    const uint8_t* bytes;   // input records: row i = bytes[off[i], off[i] + len[i])
    int64_t nbytes;
    const int64_t* off;
    const int32_t* len;
    int64_t n;
    int32_t in_bits;        // bytes of an input row's bit set: ((arity + 71) / 64) * 8
    int32_t in_fixed;       // ... and of its fixed-length part: in_bits + 8 * arity
    int32_t k;              // key fields
    int32_t n_cols;
    int32_t key_field[FG_PROJ_MAX_KEY_FIELDS];
    int32_t key_kind[FG_PROJ_MAX_KEY_FIELDS];
    int32_t col_field[FG_PROJ_MAX_COLS];
    int64_t* out_col[FG_PROJ_MAX_COLS];
    uint8_t* out_null[FG_PROJ_MAX_COLS];   // an entry may be null: a NULL field is then a bad row
};

// The length pass on stream s: every row validated, key_len[n] (-1 for a bad row), the columns and
// their null bytes, key_off[n + 1] and *rc = {total, bad rows, lowest bad index} (sums: one word
// per block of kScanThreads rows). No byte is read through an unchecked offset.
hipError_t keyproj_lengths_offsets(hipStream_t s, const ProjArgs& a, int32_t* key_len, int64_t* key_off, uint64_t* sums,
                                   RowsCtr* rc);
// The write pass: only after the host has seen rc->bad == 0 and the total within the buffer
// (out: 8-byte aligned, out_words 8-byte words).
hipError_t keyproj_write(hipStream_t s, const ProjArgs& a, const int64_t* key_off, uint64_t* out, int64_t out_words);

}  // namespace fg
