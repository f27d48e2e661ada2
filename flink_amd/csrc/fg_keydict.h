// fg_keydict.h -- what the keyed edge (fg_comm.cpp) uses of the key dictionary beyond the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/flinkgpu.h"

namespace fg {

int32_t keydict_max_parallelism(const fg_key_dict* d);
int32_t keydict_device(const fg_key_dict* d);

// fg_partition_keyed_by_owner with the key byte buffer provided after the one host read:
// key_bytes(ctx, nbytes) returns a device buffer of nbytes (8-byte aligned), or NULL (FG_EFULL:
// everything but the key bytes is complete).
typedef uint8_t* (*keydict_bytes_fn)(void* ctx, int64_t nbytes);
int keydict_partition_keyed(fg_key_dict* d, hipStream_t stream, int64_t n, int32_t ncols, const int64_t* const* cols,
                            int32_t parallelism, int64_t* const* out_cols, int64_t* counts, int32_t* out_key_lengths,
                            keydict_bytes_fn key_bytes, void* ctx, int64_t* out_byte_counts, int64_t* out_nbytes);

// The receiving side of key rows: n rows of lengths[n] bytes packed back to back in bytes[nbytes),
// each zero-padded to 8 (device memory, produced before `ready` -- an event the dictionary's stream
// waits for, or NULL), interned into d: out_ids[n] (device) complete on return. The input is
// checked on the device before a byte is read: a length that is negative, not a multiple of 4 or
// >= 2^24, or padded lengths that do not add up to nbytes, give FG_EDEVICE and nothing is interned.
int keydict_intern_packed(fg_key_dict* d, hipEvent_t ready, int64_t n, const int32_t* lengths, const uint8_t* bytes,
                          int64_t nbytes, int64_t* out_ids);

}  // namespace fg
