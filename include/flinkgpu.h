/*
 * flinkgpu.h -- C-ABI of the MI355X keyed window-aggregation engine (libflinkgpu.so).
 *
 * Drop-in boundary for Flink's window aggregation hot path.  A JNI / Panama stub on
 * the Java side binds these entry points one-for-one to the reference
 * SPI methods they replace:
 *
 *   reference (Java)                                                   C-ABI
 *   ---------------------------------------------------------------   ----------------------
 *   WindowBuffer.Factory.create(...)                                    fg_open
 *     TR/operators/aggregate/window/buffers/WindowBuffer.java:105-118
 *     + SlicingWindowAggOperatorBuilder.build  .../SlicingWindowAggOperatorBuilder.java:127-170
 *   SlicingWindowOperator.processElement -> WindowProcessor.processElement
 *     TR/operators/window/slicing/SlicingWindowOperator.java:196-204     fg_add_batch
 *     (packed BinaryRowData rows, TC/data/binary/BinaryRowData.java:68-76) fg_add_rows
 *     TR/operators/aggregate/window/processors/AbstractWindowAggProcessor.java:135-165
 *     (+ RecordsWindowBuffer.addElement  .../buffers/RecordsWindowBuffer.java:81-97)
 *   SlicingWindowOperator.processWatermark + onEventTime/onTimer
 *     SlicingWindowOperator.java:207-237                                  fg_advance_progress
 *     AbstractWindowAggProcessor.advanceProgress :178-192, fireWindow/clearWindow
 *     (SliceUnsharedWindowAggProcessor.java:46-54, SliceSharedWindowAggProcessor.java:64-118)
 *   SlicingWindowOperator.prepareSnapshotPreBarrier :240-242           fg_flush
 *     -> AbstractWindowAggProcessor.prepareCheckpoint :195-197 -> RecordsWindowBuffer.flush :108-119
 *   StreamOperatorStateHandler.snapshotState (window-aggs state + timers)   fg_snapshot_state
 *     SJ/api/operators/StreamOperatorStateHandler.java:185-241
 *   AbstractStreamOperator.initializeState (keyed state restore)         fg_restore
 *   AbstractStreamOperator.initializeState after a rescale: KeyGroupRangeAssignment /
 *     StateAssignmentOperation (each new subtask takes its key-group range out of every
 *     old subtask's state)                                                fg_restore_range
 *   HeapSnapshotStrategy / KeyGroupRangeOffsets (a keyed snapshot written in key-group order
 *     with an offset per key group)                  fg_set_snapshot_grouping, fg_snapshot_key_groups
 *   SlicingWindowOperator.getNumLateRecordsDropped :300-303            fg_late_dropped
 *   WindowedStream.sideOutputLateData -> WindowOperator.processElement :448-456
 *     (sideOutput(element) instead of numLateRecordsDropped.inc())      fg_set_late_output, fg_collect_late
 *   WindowRankOperator above the window aggregate (Window Top-N: ROW_NUMBER() OVER (PARTITION BY
 *     window_start, window_end ORDER BY agg) <= N), its local rank                 fg_set_fired_topn
 *   two-phase: LocalAggCombiner.combine (local operator output)        fg_config.flags |= FG_FLAG_LOCAL_PARTIALS
 *     GlobalAggCombiner.combine  .../combines/GlobalAggCombiner.java:77-110  fg_add_partials
 *   WindowBuffer.close / SlicingWindowOperator.close :178-183           fg_close
 *   DataStream WindowOperator.processElement / processWatermark / onEventTime
 *     SJ/runtime/operators/windowing/WindowOperator.java:300-503          same entry points,
 *                                                                        fg_config.mode = FG_MODE_DATASTREAM
 *   KeyGroupRangeAssignment.assignToKeyGroup  RT/state/KeyGroupRangeAssignment.java:63-77
 *     + KeyGroupStreamPartitioner.selectChannel SJ/runtime/partitioner/KeyGroupStreamPartitioner.java:55-65
 *                                                                        fg_key_groups
 *   BinaryRowDataKeySelector.getKey (any key type: STRING, several columns)
 *     TR/keyselector/BinaryRowDataKeySelector.java:43-50, key identity BinarySection.equals /
 *     hashCode TC/data/binary/BinarySection.java:62-78                   fg_key_dict_intern
 *
 * Conventions
 *  - Return 0 (FG_OK) on success, a positive FG_E* code otherwise; fg_last_error()
 *    holds the message (for FG_EINVAL: the reference's IllegalArgumentException text).
 *  - FG_EFULL mirrors the EOFException "buffer full, flush and retry" signal of
 *    RecordsWindowBuffer (:91-96); the engine handles it internally, it is returned only
 *    if a single batch exceeds the configured buffer capacity.
 *  - Input buffers are owned by the caller and must stay valid for the call only.
 *    Output buffers (fg_rows, fg_state_rows) are owned by the library and stay valid
 *    until the next call on the same handle.
 *  - A handle is single-threaded (Flink's mailbox model, MailboxProcessor.java:44-48);
 *    distinct handles are independent and may be used from different threads.
 *  - Times are epoch milliseconds (Java long). All integer arithmetic wraps like Java.
 */
#ifndef FLINKGPU_H
#define FLINKGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FG_ABI_VERSION 16

enum fg_status {
    FG_OK = 0,
    FG_EINVAL = 1,     /* invalid argument / window spec (IllegalArgumentException) */
    FG_EFULL = 2,      /* batch larger than the configured buffer (EOFException analogue) */
    FG_EDEVICE = 3,    /* HIP runtime error or no usable MI355X device */
    FG_ECAPACITY = 4,  /* more distinct keys in one slice than 2^13 state regions hold (~29M):
                        * raise the parallelism. Below that a region that overflows splits
                        * (BytesMap growth, BytesMap.java:229-290) and the call succeeds. */
    FG_ESTATE = 5      /* API used out of order */
};

enum fg_mode { FG_MODE_SQL = 0, FG_MODE_DATASTREAM = 1 };
enum fg_window_kind { FG_TUMBLE = 0, FG_HOP = 1, FG_CUMULATE = 2 };   /* DataStream: TUMBLE, HOP=sliding */
enum fg_val_type { FG_VAL_NONE = 0, FG_VAL_I64 = 1, FG_VAL_F64 = 2 };
/* Aggregates over the single value column (SumAggFunction, Count1AggFunction,
 * CountAggFunction, AvgAggFunction, Sum0AggFunction of TP/functions/aggfunctions/).
 * SUM0 (Sum0AggFunction.java:60-63,75-76,97-98,136-137,162-163): 0-initialised, never NULL;
 * its value is the AVG accumulator's sum. */
/* MIN / MAX (MinAggFunction.java:56-90, MaxAggFunction.java:56-96, TP/functions/aggfunctions/):
 * NULL-initialised; a non-null operand replaces the accumulator iff operand < min (> max),
 * Java primitive comparison; NULL when the window holds no non-null value. An aggregate list
 * may mix SUM / AVG / SUM0, MIN and MAX over the value column: the operator then keeps all three
 * value accumulators per (key, slice), as the reference's generated accumulator row does
 * (AggsHandlerCodeGenerator.scala:578-700), staging each record once; the two-phase operators'
 * partial rows then carry the three value accumulators too (FG_FLAG_LOCAL_PARTIALS, fg_partials). */
enum fg_agg { FG_AGG_COUNT_STAR = 0, FG_AGG_COUNT = 1, FG_AGG_SUM = 2, FG_AGG_AVG = 3, FG_AGG_SUM0 = 4,
              FG_AGG_MIN = 5, FG_AGG_MAX = 6 };
/* FG_DEVICE columns are read on the handle's stream (fg_stream): the caller orders their
 * producer before it (complete, or an event the stream waits on). fg_add_partials and
 * fg_add_rows have read them when they return; fg_add_batch's columns stay in use until the
 * work queued on the handle's stream by the NEXT call on the handle has completed (the engine
 * finishes a batch's staging in that call, so that its two partition passes run back to back
 * on the GPU): a caller that frees or reuses them orders that after the handle's stream (an
 * event recorded on fg_stream after the next call, or fg_synchronize, which releases them).
 * FG_HOST buffers (pageable or pinned) have been read completely when the call returns: the
 * caller may overwrite them at once (the H2D copy is complete; the batch's kernels may still
 * be running on the handle's stream). */
enum fg_location { FG_HOST = 0, FG_DEVICE = 1 };
/* FG_KEYHASH_DICT_ID: the key is an id of an fg_key_dict (any key type); its key group, computed
 * from the key row's bytes when it was interned, is carried in the id's low ceil(log2(max_parallelism))
 * bits. */
enum fg_key_hash { FG_KEYHASH_BINARYROW_BIGINT = 0, FG_KEYHASH_JAVA_LONG = 1, FG_KEYHASH_DICT_ID = 2 };
enum fg_flags {
    FG_FLAG_KERNEL_TIMING = 1,    /* HIP-event timing of every launch (fg_kernel_stats) */
    /* Local phase of the two-phase window aggregation (LocalSlicingWindowAggOperator +
     * LocalAggCombiner, TR/operators/aggregate/window/LocalSlicingWindowAggOperator.java:113-139,
     * combines/LocalAggCombiner.java:69-106): records are assigned to their own slice with no
     * late handling, and fg_advance_progress emits, for every slice the watermark fires, one
     * partial accumulator row per key instead of window rows: window_start/window_end = the
     * slice, agg[0] = COUNT(*), agg[1] = COUNT(v), agg[2] = SUM bits (0 when COUNT(v) = 0).
     * fg_config.aggs is ignored (the global operator's list applies), except that a MIN or
     * MAX in it makes agg[2] the partial MIN / MAX instead of the SUM; a list mixing the SUM
     * family, MIN and MAX makes the partial row carry all three value accumulators: agg[2] =
     * SUM, agg[3] = MIN, agg[4] = MAX (fg_partials.min / max of the global operator). */
    FG_FLAG_LOCAL_PARTIALS = 2,
    /* SQL processing-time windows (SliceAssigner.isEventTime() == false,
     * AbstractWindowAggProcessor.java:137-140): `rowtime` carries each record's processing
     * time, nothing is late, fg_advance_progress takes the current processing time. Records
     * are expected at or after the last progress (as processing time is). */
    FG_FLAG_PROCTIME = 4,
    /* Input rows already carry their window (SliceAssigners.windowed / WindowedSliceAssigner,
     * TR/operators/window/slicing/SliceAssigners.java:386-435, after a window TVF): `rowtime`
     * carries each row's window_end; every window is its own slice (unshared, fired and
     * expired alone, a late row is dropped once its window fired); window_start =
     * the kind's getWindowStart(window_end). The window kind/size/slide/offset describe the
     * inner assigner. window_end values must lie on the inner assigner's slice grid (as a
     * window TVF emits them), else fg_add_batch fails with FG_EINVAL. SQL event time only,
     * not the local phase. With zone rules the window_end values are local (UTC-shifted)
     * times and are taken as is. */
    FG_FLAG_WINDOWED = 8,
    /* DataStream: PurgingTrigger.of(EventTimeTrigger) -- a firing window's state is cleared
     * (FIRE_AND_PURGE), so an element of a fired, not yet cleaned window (allowed lateness)
     * fires it with itself alone (WindowOperatorTest.testLateness :1805-1886). */
    FG_FLAG_PURGING_TRIGGER = 16
};

#define FG_MAX_AGGS 8

typedef struct fg_config {
    int32_t mode;                 /* fg_mode */
    int32_t window_kind;          /* fg_window_kind */
    int64_t size_ms;              /* TUMBLE size / HOP size / CUMULATE max size */
    int64_t slide_ms;             /* HOP slide / CUMULATE step; ignored for TUMBLE */
    int64_t offset_ms;            /* window offset */
    int64_t shift_tz_offset_ms;   /* fixed-offset shift time zone (TIMESTAMP_LTZ); 0 = UTC */
    int32_t val_type;             /* fg_val_type of the aggregated column */
    int32_t num_aggs;             /* output aggregate columns, in order */
    int32_t aggs[FG_MAX_AGGS];    /* fg_agg */
    int32_t max_parallelism;      /* number of key groups (KeyGroupRangeAssignment) */
    int32_t key_group_start;      /* key-group range owned by this subtask (inclusive) */
    int32_t key_group_end;
    int32_t device_id;            /* HIP device ordinal */
    int32_t flags;                /* FG_FLAG_* */
    int64_t expected_keys;        /* distinct keys per slice on this subtask: sizes the state regions
                                   * (speed, not correctness: regions split on overflow, up to 2^13);
                                   * <= 0: unknown, 2^10 regions (117 MB per slice table), grown on demand */
    int64_t buffer_records;       /* staged records before an implicit flush (managed-memory analogue) */
    /* Shift time zone with transitions (daylight saving): the ZoneRules of the ZoneId as data
     * (ZoneRules.getTransitions() on the Java side). n_tz_transitions > 0 replaces
     * shift_tz_offset_ms: toUtcTimestampMills / toEpochMillsForTimer / getNextTriggerWatermark
     * follow TimeWindowUtil.java:53-61,70-140,187-210 with these rules. SQL mode only (incl. the
     * two-phase operators, whose partial rows carry local slice ends). Copied at fg_open. */
    const int64_t* tz_transition_ms;   /* n_tz_transitions instants, epoch ms, ascending */
    const int64_t* tz_offset_ms;       /* n_tz_transitions + 1 offsets (ms): [i] in force before transition i */
    int32_t n_tz_transitions;
    int32_t tz_use_daylight;           /* TimeZone.getTimeZone(zone).useDaylightTime() */
    /* DataStream WindowOperator.allowedLateness (WindowedStream.allowedLateness, WindowOperator.java:
     * 608-622,630-681): a window's state is kept until cleanupTime = maxTimestamp + lateness
     * (Long.MAX_VALUE on overflow); an element of a fired window not yet cleaned re-fires it
     * (EventTimeTrigger.onElement :37-46). 0 for SQL operators. */
    int64_t allowed_lateness_ms;
} fg_config;

/* fg_batch.format bits -- narrow FG_HOST columns, so a batch moves fewer bytes over PCIe (the
 * link, not the kernels, bounds a host-fed operator): a shim whose keys fit 32 bits (INT keys,
 * dictionary ordinals, most BIGINT ids) and whose micro-batch spans < 2^32 ms hands 4-byte
 * columns; the engine widens them on the device. 24 -> 16 B per record for a DOUBLE value, 12 B
 * for a BIGINT value that fits 32 bits. */
enum fg_batch_format {
    FG_BATCH_KEY32 = 1,       /* key: int32_t[n], sign-extended */
    FG_BATCH_ROWTIME32 = 2,   /* rowtime: uint32_t[n], each rowtime_base + the offset */
    FG_BATCH_VAL32 = 4        /* BIGINT val: int32_t[n], sign-extended (FG_VAL_I64 only) */
};

typedef struct fg_batch {
    int64_t n;
    int32_t location;             /* fg_location of the column pointers */
    int32_t format;               /* fg_batch_format bits; 0: 8-byte columns. Non-zero: FG_HOST only */
    const int64_t* key;           /* BIGINT grouping key (FG_BATCH_KEY32: int32_t[]) */
    const int64_t* rowtime;       /* event time, epoch ms (TIMESTAMP(3) compact form; FG_BATCH_ROWTIME32: uint32_t[]) */
    const void* val;              /* int64_t[] or double[] per fg_config.val_type; may be NULL for FG_VAL_NONE */
    const uint8_t* val_null;      /* optional: 1 = value is NULL */
    int64_t rowtime_base;         /* FG_BATCH_ROWTIME32: rowtime[i] = rowtime_base + offset[i] */
} fg_batch;

typedef struct fg_rows {
    int64_t n;
    int32_t location;             /* where the column pointers live */
    int32_t num_aggs;
    const int64_t* key;
    const int64_t* window_start;       /* window_start, window_end: NULL in run mode (fg_set_fired_runs) */
    const int64_t* window_end;
    const int64_t* agg[FG_MAX_AGGS];   /* 8-byte columns: BIGINT, or the bits of a DOUBLE */
    const uint8_t* null_mask;          /* bit i set: agg[i] is NULL in that row */
    const int64_t* rowtime;            /* DataStream: window.maxTimestamp() (end - 1); SQL, run mode: NULL */
} fg_rows;

/* Packed BinaryRowData input: the records as Flink holds them (BinaryRowData.java:68-76): row i
 * is the fixed-length part of a BinaryRowData of `arity` fields at rows + i * stride -- a
 * header byte (RowKind) and the null bits (bit 8 + f of the little-endian bit set marks field f
 * NULL, :155-157) in calculateBitSetWidthInBytes(arity) = ((arity + 71) / 64) * 8 bytes, then
 * 8 bytes per field (:119-121): BIGINT / DOUBLE as is (:306-320), TIMESTAMP(3) as its compact
 * epoch millis (:347-352). A shim hands a MemorySegment of such rows (e.g. the serialized
 * records of a network buffer or the RecordsWindowBuffer's pages) without building columns.
 * A NULL value field is a NULL value; a NULL key or rowtime is FG_EINVAL (the columnar boundary
 * has no NULL key either: the shim maps a nullable key to a BIGINT id). */
typedef struct fg_row_batch {
    int64_t n;
    int32_t location;             /* fg_location of `rows` */
    int32_t stride;               /* bytes between rows: >= the fixed-length part, a multiple of 8 */
    const uint8_t* rows;
    int32_t arity;                /* fields per row */
    int32_t key_field;            /* BIGINT grouping key */
    int32_t rowtime_field;        /* TIMESTAMP(3) event time */
    int32_t val_field;            /* BIGINT or DOUBLE per fg_config.val_type; -1: none (FG_VAL_NONE) */
} fg_row_batch;

/* Partial accumulator rows entering the global phase (GlobalAggCombiner.combine,
 * combines/GlobalAggCombiner.java:77-110, fed through the `sliced` assigner,
 * SliceAssigners.java:494-533): the rows of a FG_FLAG_LOCAL_PARTIALS operator after the
 * key-group exchange. */
typedef struct fg_partials {
    int64_t n;
    int32_t location;             /* fg_location of the column pointers */
    int32_t reserved0;
    const int64_t* key;
    const int64_t* slice_end;     /* the partial's slice (window_end of the local row) */
    const int64_t* cnt_star;
    const int64_t* cnt_val;
    const int64_t* sum;           /* i64 or f64 bits per fg_config.val_type */
    /* a global operator whose list mixes the SUM family, MIN and MAX (several value
     * accumulators): the partial MIN and MAX (the local phase's agg[3] / agg[4]); else NULL */
    const int64_t* min;
    const int64_t* max;
} fg_partials;

/* Checkpoint image of the GPU-resident keyed state: one entry per (key, slice) accumulator,
 * the content of WindowValueState "window-aggs" (AbstractWindowAggProcessor.java:103-109). */
typedef struct fg_state_rows {
    int64_t n;
    const int64_t* key;
    const int64_t* slice_end;     /* namespace of WindowValueState */
    const int64_t* cnt_star;      /* COUNT(*) accumulator */
    const int64_t* cnt_val;       /* COUNT(v) accumulator */
    const int64_t* sum;           /* SUM/AVG sum accumulator (i64 or f64 bits); a MIN- or MAX-only
                                   * operator: its MIN / MAX accumulator */
    const int64_t* min;           /* an operator with several value accumulators (SUM family, MIN,
                                   * MAX in one aggregate list): the MIN and MAX accumulators (the
                                   * identity where absent); NULL for other operators */
    const int64_t* max;
} fg_state_rows;

typedef struct fg_stats {
    int64_t records_in;
    int64_t records_staged;
    int64_t late_dropped;
    int64_t rows_fired;
    int64_t flushes;
    int64_t live_slices;
    int64_t state_regions;        /* P */
    int64_t region_capacity;      /* entries per region in HBM */
} fg_stats;

/* Per-kernel accounting (filled when FG_FLAG_KERNEL_TIMING is set): launches, summed
 * HIP-event duration on the handle's stream, records consumed and rows emitted. A restore
 * (fg_restore as well as fg_restore_range) records the classes restore_filter (slice dictionary,
 * row counts), restore_scatter (grouping) and restore (the merges). */
typedef struct fg_kernel_stat {
    char name[32];
    int64_t launches;
    double total_ms;
    int64_t records;
    int64_t rows;
} fg_kernel_stat;

typedef struct fg_handle fg_handle;

int  fg_open(const fg_config* cfg, fg_handle** out);
int  fg_add_batch(fg_handle* h, const fg_batch* batch);
/* fg_add_batch for packed BinaryRowData rows (same semantics, same processElement per row). */
int  fg_add_rows(fg_handle* h, const fg_row_batch* rows);
/* Global phase: merge partial accumulators (late rules of the global operator apply to
 * the partial's slice). */
int  fg_add_partials(fg_handle* h, const fg_partials* partials);
int  fg_advance_progress(fg_handle* h, int64_t watermark, int32_t out_location, fg_rows* fired);
/* Asynchronous fg_advance_progress (ABI 11; the same processWatermark, device output): the
 * windows the watermark fires are queued on the handle's stream and the call returns without
 * waiting for them. A shim that forwards the watermark only after the fired rows (Flink emits a
 * window's rows before the watermark, SlicingWindowOperator.java:207-237 / WindowOperator
 * onEventTime) takes them with fg_collect_fired, which waits; until then the host is free to
 * deliver the next watermarks and batches. The fires' completion -- row count, region retries,
 * overflow check -- is taken by the next call that needs it: a watermark that fires again, any
 * batch, flush, snapshot or restore. Errors of a fire are reported by that call. The rows of an
 * async advance stay valid until the next call that fires windows. */
int  fg_advance_progress_async(fg_handle* h, int64_t watermark);
/* fg_advance_progress_async of n watermarks in order, as n calls would (ABI 13): the
 * watermarks a shim received since its last batch -- with no element between them -- in one
 * call instead of one JNI / C call each (configs[0]: 100 watermarks per 1M-record batch; each
 * one that fires nothing only moves the progress). Stops at the first error. */
int  fg_advance_progress_async_n(fg_handle* h, const int64_t* watermarks, int64_t n);
/* Waits for the fires of the last fg_advance_progress_async call and returns their rows (device
 * pointers, as fg_advance_progress with FG_DEVICE); n = 0 when it fired nothing. A synchronous
 * fg_advance_progress called while async rows are uncollected returns them ahead of its own rows
 * (none is dropped). */
int  fg_collect_fired(fg_handle* h, fg_rows* fired);
/* fg_collect_fired with the rows at out_location (ABI 12): FG_HOST copies them into library-owned
 * host memory (as fg_advance_progress with FG_HOST) -- what a JVM shim wraps in direct buffers;
 * FG_DEVICE is fg_collect_fired. */
int  fg_collect_fired_to(fg_handle* h, int32_t out_location, fg_rows* fired);
int  fg_flush(fg_handle* h);
/* Local phase only (FG_FLAG_LOCAL_PARTIALS; ABI 12): every buffered slice emits its partial
 * accumulator rows now, as fg_advance_progress does for the slices a watermark fires --
 * LocalSlicingWindowAggOperator.prepareSnapshotPreBarrier -> WindowBuffer.flush
 * (LocalSlicingWindowAggOperator.java:142-144, RecordsWindowBuffer.java:108-119 with
 * LocalAggCombiner.java:69-106): the local operator holds no state across a checkpoint. The
 * progress does not move. Rows as fg_advance_progress at out_location. */
int  fg_flush_partials(fg_handle* h, int32_t out_location, fg_rows* fired);
int  fg_snapshot_state(fg_handle* h, fg_state_rows* out, int64_t* timer_watermark);
/* snapshotState in two parts (ABI 15; StreamOperatorStateHandler.snapshotState's synchronous
 * part and the AsyncSnapshotCallable of a heap state backend, SnapshotStrategyRunner.snapshot):
 * _async flushes the staged records and exports every resident slice into a device image (the
 * state as of this call) and queues its copy into the pinned host image on a stream of its own;
 * the operator takes batches, watermarks and partials meanwhile. _wait returns that image (the
 * fg_snapshot_state layout, valid until the next snapshot call) once the copy has completed.
 * One snapshot at a time: fg_snapshot_state[_async] fails with FG_ESTATE while one is not
 * collected. fg_snapshot_state is _async + _wait. An image of an operator that never saw a NULL
 * value may return the same column for cnt_star and cnt_val (they are equal).
 * A full image is fg_snapshot_plan + fg_snapshot_state_select_async with every slice selected (one
 * export launch) and shares the select's limits: at most 65,535 resident slices and fewer than 2^32
 * rows (over 130 GB of image columns). Beyond either the call returns FG_EINVAL after the staged
 * records are flushed and before a row is exported or copied; the handle stays usable. A caller's
 * earlier fg_snapshot_plan is invalid from the call on, and no plan is valid after it.
 * fg_kernel_stats: a full image counts under "export" (one launch per image with rows, records =
 * the image's rows), a selective one under "export_select". */
int  fg_snapshot_state_async(fg_handle* h);
int  fg_snapshot_state_wait(fg_handle* h, fg_state_rows* out, int64_t* timer_watermark);
/* The slices of the image the last fg_snapshot_state / fg_snapshot_state_wait returned (ABI 16):
 * the image's rows are grouped by slice, ascending; `changed` tells whether the slice's state was
 * written since the previous image of this handle (a new slice, a flush or fold into it, a late
 * record; every slice of a handle's first image; a table restored into an empty handle by fg_restore
 * counts as unchanged -- the backend holds it). A shim keeps its keyed state between checkpoints and
 * rewrites only the changed slices' entries, clearing the namespaces of slices no longer in the image
 * (AbstractWindowAggProcessor.prepareCheckpoint :195-197 flushes only the buffer; AggCombiner.combine
 * :76-115 touches only the (key, slice) pairs a flush saw). Valid until the next snapshot call. */
typedef struct fg_image_slices {
    int64_t n;
    const int64_t* slice_end;   /* [n] */
    const int64_t* first_row;   /* [n] the slice's rows are image rows [first_row, first_row + rows) */
    const int64_t* rows;        /* [n] */
    const uint8_t* changed;     /* [n] 1 / 0 */
} fg_image_slices;
int  fg_snapshot_slices(fg_handle* h, fg_image_slices* out);
/* Key-grouped images (ABI 16, added; Flink writes a keyed snapshot in key-group order with an offset
 * per key group -- KeyGroupRangeOffsets, HeapSnapshotStrategy -- so that a restore after a rescale
 * reads only the ranges it owns). From the next snapshot on, the rows of every slice of an image are
 * ordered by key group (key_group(key, key_hash, fg_config.max_parallelism)), ascending; key_hash < 0
 * turns the grouping off (the default).
 *  - A grouped image is a valid fg_snapshot_state image in every respect: the same multiset of rows,
 *    the same slice grouping and the same fg_snapshot_slices answer. Only the order of the rows inside
 *    a slice differs; the order inside one (slice, key group) run is unspecified.
 *  - Works with fg_snapshot_state and with _async / _wait (the image is the state as of the _async
 *    call). The partition runs as kernels on the handle's stream between the export and the image's
 *    device-to-host copy; the host reads no row. A cnt_val column that aliases cnt_star (see
 *    fg_snapshot_state_async) is neither moved nor copied.
 *  - FG_EINVAL: a key_hash >= 0 that is no fg_key_hash; a handle whose max_parallelism is not in
 *    1 .. 32768; an asynchronous snapshot not collected yet. The call does no device work, and the
 *    handle stays usable after an error.
 *  - Extra device memory while the grouping is on: one more set of the moved image columns, 8 B x
 *    (3 .. 6: key, cnt_star, sum, and cnt_val / min / max where the image has them; slice_end stays in
 *    place) per row, and 8 B x max_parallelism x slices for the (slice, key group) counters and their
 *    offsets.
 * fg_snapshot_key_groups: the index of the image the last fg_snapshot_state / _wait returned, valid
 * as long as fg_snapshot_slices' answer. FG_ESTATE if no image was returned since the last snapshot
 * call, or if that image was taken with the grouping off. An image without slices: n_slices == 0 and
 * first_row == {0}. first_row[s * max_parallelism] == fg_image_slices.first_row[s], and the last
 * entry is the image's row count. */
int  fg_set_snapshot_grouping(fg_handle* h, int32_t key_hash);
typedef struct fg_image_key_groups {
    int64_t n_slices;            /* = fg_image_slices.n of the same image, same order */
    int32_t max_parallelism;     /* key groups per slice */
    const int64_t* first_row;    /* [n_slices * max_parallelism + 1]: key group g of slice s holds image
                                  * rows [first_row[s*maxp+g], first_row[s*maxp+g+1]) */
} fg_image_key_groups;
int  fg_snapshot_key_groups(fg_handle* h, fg_image_key_groups* out);
/* Fired rows as runs (ABI 16, added): every row of one fire carries the same window_start, window_end
 * and (DataStream) rowtime = end - 1. A handle in run mode returns its fired rows without these
 * columns and says once per run which window a range of rows belongs to.
 * fg_set_fired_runs(h, on != 0) turns run mode on, 0 turns it off (the default). Idempotent.
 *  - FG_EINVAL (turning on): a FG_FLAG_LOCAL_PARTIALS handle -- its rows feed fg_comm_* and
 *    fg_partition_*, which read window_end per row; a handle with allowed_lateness_ms > 0 -- late
 *    elements fire rows whose window differs per row.
 *  - FG_ESTATE: fired rows are not collected yet, or a fire is pending (after
 *    fg_advance_progress_async: fg_collect_fired first).
 *    fg_last_error names the reason. The handle stays usable after an error.
 * In run mode every call that returns fg_rows -- fg_advance_progress, fg_collect_fired,
 * fg_collect_fired_to -- fills key, agg[], null_mask, n and num_aggs as always and leaves
 * window_start, window_end and rowtime NULL, for FG_DEVICE and FG_HOST alike. The handle holds no
 * device or host memory for the three columns (16 of 8 x (3 + aggs) + 1 bytes per SQL row, 24 per
 * DataStream row), the kernels do not store them and no copy moves them.
 * fg_fired_runs: the runs of the rows the last such call returned, in library-owned host memory,
 * valid until the next call that fires windows (or fg_reset, fg_restore, fg_set_fired_runs); n = 0
 * when that call returned no rows. FG_ESTATE when run mode is off. Run i covers rows
 * [first_row[i], first_row[i] + rows[i]):
 *  - first_row[0] = 0, first_row[i + 1] = first_row[i] + rows[i], every rows[i] > 0, and the rows sum
 *    to fg_rows.n;
 *  - rowtime[i] = window_end[i] - 1 (Java subtraction; also filled for a SQL handle);
 *  - adjacent runs never share a window_end, but a window may appear in more than one run: the rows
 *    a state region re-emits after it overflowed and was split follow the rows of the windows fired
 *    after it. A consumer must not assume one run per window;
 *  - rows of fg_advance_progress_async calls not yet collected that lead a synchronous advance's
 *    rows keep their runs, in order. */
typedef struct fg_row_runs {
    int64_t n;
    const int64_t* window_start;   /* [n] */
    const int64_t* window_end;     /* [n] */
    const int64_t* rowtime;        /* [n] window_end - 1 */
    const int64_t* first_row;      /* [n] */
    const int64_t* rows;           /* [n] */
} fg_row_runs;
int  fg_set_fired_runs(fg_handle* h, int32_t on);
int  fg_fired_runs(fg_handle* h, fg_row_runs* out);
/* Late elements as a side output (ABI 16, added; WindowedStream.sideOutputLateData): in
 * WindowOperator.processElement (:448-456) an element whose windows are all late and which is late
 * itself is emitted to the side output when a lateDataOutputTag is set, and only otherwise counted in
 * numLateRecordsDropped. fg_set_late_output(h, on != 0) selects the first branch, 0 the second (the
 * default). Idempotent.
 *  - FG_EINVAL (turning on): a handle that is not FG_MODE_DATASTREAM, or one with FG_FLAG_LOCAL_PARTIALS,
 *    FG_FLAG_PROCTIME or FG_FLAG_WINDOWED -- SQL window operators have no side output.
 *  - FG_ESTATE (turning off): late records are not collected yet.
 *    fg_last_error names the reason. The handle stays usable after either error.
 * While on, every element that the same handle with the mode off would add to fg_late_dropped is kept
 * as a record instead, through fg_add_batch (every fg_batch_format) and fg_add_rows alike, and
 * fg_late_dropped does not move (the reference increments the counter only in the else branch). Fired
 * rows, state, snapshots, records_in and every other statistic are what they are with the mode off.
 * The records are copied out on the device by a pass of their own ahead of the ingest
 * (fg_kernel_stats class "late_out": records = the batches' elements, rows = the late records; the
 * class follows every other class but "topn" (fg_set_fired_topn), and fg_kernel_stats lists it for a
 * handle once the mode was turned on); the host reads nothing during fg_add_batch.
 * fg_collect_late: the late records of all batches since the previous collect (or since fg_open,
 * fg_reset, fg_restore*), in arrival order -- batch by batch, inside a batch by index, as the reference
 * emits them one by one in processElement. rowtime is the element's timestamp as it was handed in
 * (widened to 8 bytes), val its value bits. FG_HOST copies the columns into library-owned host memory;
 * FG_DEVICE returns device columns, complete in stream order on fg_stream. The call drains the list: a
 * second call returns n = 0. The columns stay valid until the next fg_add_batch / fg_add_rows /
 * fg_collect_late / fg_reset / fg_restore* / fg_close on the handle.
 *  - FG_ESTATE: the mode is off; or "internal: late output and ingest disagree" -- the number of
 *    records kept differs from the ingest's own drop count (the list is drained, nothing is returned).
 * Late records are not operator state (the reference has emitted them when processElement returns):
 * snapshots do not contain them, fg_reset and fg_restore* discard uncollected ones. A shim therefore
 * collects after each batch, and in any case before it forwards a watermark or takes a checkpoint
 * barrier. The columns grow with the uncollected records: 24 B + 1 B per element of the largest
 * uncollected run of batches, as a worst case. */
typedef struct fg_late_records {
    int64_t n;
    int32_t location;          /* fg_location of the columns */
    int32_t reserved0;
    const int64_t* key;
    const int64_t* rowtime;    /* the element's timestamp as it was handed in (8-byte, widened) */
    const void*    val;        /* int64_t[] / double[] bits; NULL for FG_VAL_NONE */
    const uint8_t* val_null;   /* NULL when no batch since the last collect carried val_null */
} fg_late_records;
int  fg_set_late_output(fg_handle* h, int32_t on);
int  fg_collect_late(fg_handle* h, int32_t out_location, fg_late_records* out);
/* Top-N rows per fired window (ABI 16, added): Flink's Window Top-N directly above the window
 * aggregate, ROW_NUMBER() OVER (PARTITION BY window_start, window_end ORDER BY agg [DESC]) <= n, selected
 * where the fired rows sit instead of after their copy to the host. At parallelism P the P x n rows
 * the handles return are a superset of the global top n (the local rank of the reference's plan); the
 * global rank over them stays with the caller.
 * fg_set_fired_topn(h, n, agg_index, descending): n = 0 turns the selection off (the default;
 * agg_index and descending are then ignored; idempotent). n in 1 .. FG_TOPN_MAX: every call that
 * returns fg_rows -- fg_advance_progress, fg_collect_fired, fg_collect_fired_to -- returns, per fired
 * window, only the n rows that rank first by agg[agg_index].
 *  - Rank order, a total order (results are deterministic). Primary: agg[agg_index] compared as the
 *    column's SQL type -- BIGINT (COUNT(*), COUNT, and SUM / AVG / SUM0 / MIN / MAX of a BIGINT value)
 *    as signed 64-bit; DOUBLE (SUM / AVG / SUM0 / MIN / MAX of a DOUBLE value) in Double.compare's
 *    order: -0.0 below +0.0, NaN (every NaN alike) above +inf. descending != 0: the largest first. A
 *    NULL aggregate (its null_mask bit) is the smallest value: last when descending, first when
 *    ascending (Flink's default null collation, NULLs low). Ties: the smaller key (signed) ranks
 *    first -- the engine's choice; ROW_NUMBER in the reference breaks ties by arrival order at the
 *    rank operator, which a keyBy leaves unspecified.
 *  - The selection is per window, not per run: it is applied to the complete set of rows the call
 *    hands back, grouped by window_end -- the rows of uncollected fg_advance_progress_async calls
 *    that lead a synchronous advance included, and a window whose rows sit in several runs
 *    (fg_fired_runs) is selected once. Without allowed lateness all rows a watermark fires for a
 *    window, the rows a split region re-emits included, are complete before any call returns them,
 *    so a window's rows never straddle two returning calls. (After fg_restore* a HOP / CUMULATE
 *    window that fired before the checkpoint may fire again for the keys of later records: those
 *    rows are a set of their own, selected as the call returns them.)
 *  - Output order: windows by ascending window_end; inside a window by rank -- row i of a window is
 *    ROW_NUMBER = i + 1. A window with fewer than n rows returns all of them, ranked.
 *  - fg_rows.n is the selected count; key, agg[], null_mask and, when run mode is off, window_start,
 *    window_end and rowtime are gathered for the selected rows, for FG_DEVICE and FG_HOST alike. With
 *    FG_HOST only the selected rows are copied to the host. The FG_DEVICE columns are complete when
 *    the call returns.
 *  - Run mode (fg_set_fired_runs) composes: fg_fired_runs describes the selected rows, exactly
 *    one run per window, and its invariants hold (first_row[0] = 0, contiguous runs, every
 *    rows[i] > 0, the rows sum to fg_rows.n).
 *  - fg_stats.rows_fired, fg_late_dropped, state, snapshots and restore are what they are with the
 *    selection off. fg_kernel_stats class "topn": records = rows in, rows = rows out; listed for a
 *    handle once the selection was turned on, after "late_out" when both are listed
 *    (fg_set_kernel_timing's bit i is entry i of the list as fg_kernel_stats returns it).
 *  - FG_EINVAL (fg_last_error names the reason; the handle stays usable): n < 0 or n > FG_TOPN_MAX;
 *    and turning on: agg_index outside 0 .. num_aggs - 1; a FG_FLAG_LOCAL_PARTIALS handle -- its rows
 *    are partial accumulators, not results; allowed_lateness_ms > 0 -- late elements re-fire single
 *    rows, and an update row is not a rank input. A returning call with 2^31 or more fired rows
 *    fails with FG_EINVAL while the selection is on.
 *  - FG_ESTATE: fired rows are not collected yet, or a fire is pending (after
 *    fg_advance_progress_async: fg_collect_fired first) -- the rule of fg_set_fired_runs.
 *  - The pass runs as three kernel launches per returning call (whatever the number of windows) on the
 *    handle's stream, after the fires have completed and before the row copy; per fired row it reads
 *    the order column, its null_mask byte and the key (17 B), and every column of the selected rows
 *    only. While the selection is on the engine keeps the run marks of fg_fired_runs also with run mode
 *    off (one small launch per window change), so that the host knows a call's windows without
 *    reading a row.
 *  - Extra device memory, allocated by the first selecting call and kept until fg_close: candidate
 *    buffers of 20 B x n per 16,384 fired rows (plus 1/32 of that for the merged lists), and a second
 *    set of the output columns sized by n x (windows per call), not by the fired rows. */
#define FG_TOPN_MAX 1024
int  fg_set_fired_topn(fg_handle* h, int32_t n, int32_t agg_index, int32_t descending);
/* Fired rows as packed BinaryRowData rows (ABI 16, added): the output half of fg_add_rows. The rows
 * the last returning call -- fg_advance_progress, fg_collect_fired or fg_collect_fired_to -- handed
 * back, transposed on the device into the fixed-length parts of BinaryRowData rows, which a shim
 * views with BinaryRowData.pointTo instead of building one GenericRowData per row on the host. The
 * intended use: take the fired rows with FG_DEVICE (nothing is copied), then pull them packed.
 * fg_fired_packed(h, first_row, max_rows, flags, out_location, out) packs rows
 * [first_row, min(first_row + max_rows, N)), N = that call's fg_rows.n. The range is there because a
 * JVM direct buffer holds less than 2 GiB: a shim pulls a large fire in chunks, each call on its own.
 *  - Row layout, byte-exact, the layout of fg_row_batch: little endian; a bit set of
 *    ((arity + 71) / 64) * 8 bytes (8 for every arity here) whose byte 0 is RowKind INSERT = 0 and
 *    whose bit 8 + f marks field f NULL; then 8 bytes per field. Fields:
 *    [key,] agg[0] .. agg[num_aggs - 1], window_start, window_end -- arity = num_aggs + 2, one more
 *    with FG_PACK_KEY_FIELD; stride = calculateFixPartSizeInBytes(arity) = 8 * (arity + 1). An
 *    aggregate is the 8 bytes of fg_rows.agg[] (BIGINT, or the bits of a DOUBLE), the window fields
 *    are TIMESTAMP(3) compact epoch milliseconds, the values fg_rows.window_start / window_end hold
 *    (or would hold). A NULL aggregate (its null_mask bit) sets its field's bit and stores eight
 *    zero bytes (BinaryRowWriter.setNullAt): whatever the column holds there does not reach the row.
 *  - key: the rows' key column (for the ids of a key dictionary: the ids; the key rows come from
 *    fg_key_dict_rows), at the location of `rows`; NULL with FG_PACK_KEY_FIELD, where the key (or
 *    id) is field 0, a BIGINT.
 *  - Run mode (fg_set_fired_runs): the window columns do not exist; the window of a row is its
 *    run's, looked up on the device in the run directory fg_fired_runs describes (uploaded once per
 *    call; one launch covers every run).
 *  - Top-N (fg_set_fired_topn): the packed rows are the selected rows, in their order.
 *  - FG_HOST: rows (and key) are library-owned pinned host memory, complete when the call returns.
 *    FG_DEVICE: device memory, complete in stream order on fg_stream. Both stay valid until the
 *    next fg_fired_packed or the next call that invalidates the fired rows (below). The buffers are
 *    reused and grow to the largest range asked for.
 *  - FG_EINVAL, before any device work (fg_last_error names the reason; the handle stays usable):
 *    NULL h or out, an unknown location; flag bits other than FG_PACK_KEY_FIELD; first_row < 0,
 *    first_row > N or max_rows < 0; n * stride >= 2^31 with FG_HOST (ask for a smaller range); an
 *    FG_MODE_DATASTREAM handle, whose elements are tuples, not RowData; an FG_FLAG_LOCAL_PARTIALS
 *    handle, whose rows are accumulator rows of another layout.
 *  - FG_ESTATE unless the fired rows are still the ones the last returning call handed back: no
 *    returning call yet; any call on the handle since then other than fg_fired_runs,
 *    fg_fired_packed, fg_get_stats, fg_late_dropped, fg_kernel_stats, fg_set_kernel_timing,
 *    fg_synchronize, fg_stream, fg_last_error and fg_snapshot_plan (the calls a valid
 *    fg_snapshot_plan survives, and fg_fired_runs); a pending fg_advance_progress_async fire or
 *    uncollected async rows. A returning call that fired nothing is valid and gives n = 0, as do
 *    first_row == N and max_rows == 0.
 *  - One kernel launch per call with rows, on the handle's stream, one lane per 8-byte word of the
 *    output; per row it reads 8 * arity + 1 bytes (8 * (arity - 2) + 1 in run mode) and writes
 *    8 * (arity + 1). fg_kernel_stats class "pack_rows": records = rows = rows packed; listed for a
 *    handle once it has packed rows, after every other class, "late_out" and "topn" included (a
 *    handle that never packs lists what it listed before the class existed). */
enum fg_pack_flags { FG_PACK_KEY_FIELD = 1 };
typedef struct fg_packed_rows {
    int64_t n;             /* rows packed */
    int32_t location;      /* fg_location of rows / key */
    int32_t arity;         /* fields per row */
    int32_t stride;        /* bytes per row = calculateFixPartSizeInBytes(arity) */
    int32_t flags;         /* as passed */
    const uint8_t* rows;   /* n * stride bytes */
    const int64_t* key;    /* the rows' key column (dictionary handles: the ids); NULL with FG_PACK_KEY_FIELD */
} fg_packed_rows;
int  fg_fired_packed(fg_handle* h, int64_t first_row, int64_t max_rows, int32_t flags,
                     int32_t out_location, fg_packed_rows* out);
/* Selective images (ABI 16, added): a checkpoint that exports and copies only the slices its caller
 * needs. The engine says what is resident and what changed (plan), the caller answers with a mask
 * (a shim's policy needs more than the changed slices: a CUMULATE namespace is rebuilt from all its
 * contributing slices), the engine exports exactly the masked slices (select).
 * fg_snapshot_plan: the front half of fg_snapshot_state -- pending fires settled, the staged records
 * flushed, a pending restore re-fire finished, the region counts read -- without exporting or copying a
 * row. `out` lists every resident slice, ascending: rows, first_row = the position the slice would have
 * in a full fg_snapshot_state image taken now (the exclusive prefix of rows), changed as
 * fg_snapshot_slices would report it; *timer_watermark (may be NULL) is what fg_snapshot_state would
 * return. No changed flag is cleared, two plans in a row give the same answer. The arrays are valid
 * until the next call on the handle. FG_ESTATE while an asynchronous snapshot is uncollected.
 * fg_snapshot_state_select_async: exports the slices i with want[i] != 0 (indexed as in the plan) in
 * one kernel launch and queues the image's copy as fg_snapshot_state_async does;
 * fg_snapshot_state_wait collects it (one snapshot at a time, shared with fg_snapshot_state[_async]).
 *  - FG_ESTATE unless the plan is still valid: fg_snapshot_plan, fg_get_stats, fg_late_dropped,
 *    fg_kernel_stats, fg_set_kernel_timing, fg_synchronize, fg_stream and fg_last_error keep it valid,
 *    every other call on the handle invalidates it, and a select consumes it. The image is therefore
 *    the state as of the plan.
 *  - FG_EINVAL before any device work (the handle stays usable, the plan stays valid): n differs from
 *    the plan's n; want is NULL with n > 0; 2^32 or more selected rows; more than 65,535 selected
 *    slices.
 *  - The image holds exactly the rows a full image holds for the selected slices (per slice the same
 *    multiset), grouped by slice, ascending, compact from row 0. After the wait fg_snapshot_slices
 *    describes that image: only the selected slices, first_row the compact prefix, changed as planned.
 *    With fg_set_snapshot_grouping on each selected slice's rows are ordered by key group and
 *    fg_snapshot_key_groups indexes the compact image (n_slices = the selected slices).
 *  - changed is cleared only for the selected slices: a changed slice left out is reported changed
 *    again by the next plan.
 *  - An all-zero mask, or a handle without slices (n == 0, want may be NULL), gives a valid image with
 *    n == 0. cnt_val may alias cnt_star as for fg_snapshot_state_async.
 * fg_snapshot_state_select is _select_async + _wait. */
int  fg_snapshot_plan(fg_handle* h, fg_image_slices* out, int64_t* timer_watermark);
int  fg_snapshot_state_select_async(fg_handle* h, const uint8_t* want, int64_t n);
int  fg_snapshot_state_select(fg_handle* h, const uint8_t* want, int64_t n, fg_state_rows* out,
                              int64_t* timer_watermark);
/* The device self-check (ABI 16): the DPP wave scans and the tile walk the fire runs, as this
 * library's code object compiled them, on inputs whose answers the host knows (msg: "ok" or what is
 * wrong). fg_open runs it once per process and device and fails with FG_EDEVICE (its message in
 * fg_last_error(NULL)) if it does not pass: a miscompiled build fails loudly instead of firing wrong
 * rows. */
int  fg_selftest(int32_t device_id, char* msg, int32_t cap);
/* Restore (initializeState): the rows of one host image (an fg_snapshot_state image, or the
 * `window-aggs` entries a shim read from the keyed state backend) merged into the handle's state,
 * and the handle left as open() + initializeState() leave the operator: progress at
 * Long.MIN_VALUE, the timer watermark as DESIGN.md section 3 tells. Every row is kept --
 * fg_config's key-group range and max parallelism are not read. fg_restore and fg_restore_range
 * are two entry points of one pipeline: the image is uploaded whole, the grouping by slice and
 * state region and the scatter run as kernels on the handle's stream, then one merge per slice; the
 * host never reads a row. What fg_restore_range says below about row order and duplicates, the
 * limits (at most 4096 distinct slice ends and fewer than 2^32 rows per call, else FG_EINVAL), the
 * empty image (n == 0) and the device memory during the call holds here too.
 *  - FG_EINVAL, before any device work: n < 0; n > 0 and a NULL key, slice_end, cnt_star, cnt_val or
 *    sum; a NULL min or max for an operator with several value accumulators. The handle stays usable. */
int  fg_restore(fg_handle* h, const fg_state_rows* in, int64_t timer_watermark);
/* Rescale restore (ABI 16, added): fg_restore of the concatenation of images[0 .. n_images),
 * restricted to the rows whose key group lies in the handle's range,
 *   fg_config.key_group_start <= key_group(key, key_hash, fg_config.max_parallelism) <= key_group_end
 * (KeyGroupRangeAssignment; a restart at another parallelism hands every new subtask the images of
 * all old subtasks). The state after the call is what fg_restore leaves for that filtered image:
 * the filter is one more test in the kernels fg_restore runs.
 *  - timer_watermark: the minimum over the images' timer watermarks.
 *  - location FG_HOST: pageable or pinned columns, copied up on the handle's stream and read when the
 *    call returns. FG_DEVICE: device columns read in place on the handle's stream (the ordering rule
 *    of fg_location applies); they must not change during the call.
 *  - Rows may come in any order and a slice may occur in several images; duplicate (key, slice)
 *    rows merge (counts and sums added, MIN of MIN, MAX of MAX). With three or more DOUBLE duplicates of one (key, slice)
 *    the summation order is unspecified. Rows listed slice by slice (as fg_snapshot_state writes
 *    them) are the fast case: the grouping walks a run of rows once per distinct slice end in it.
 *  - At most 4096 distinct slice ends among the rows of all images (foreign rows included) and fewer
 *    than 2^32 rows per call, else FG_EINVAL.
 *  - FG_EINVAL, before any device work: n_images < 0; an image with n > 0 and a NULL key, slice_end,
 *    cnt_star, cnt_val or sum; a NULL min or max for an operator with several value accumulators; an
 *    unknown key_hash or location; a handle whose range is not 0 <= start <= end < max_parallelism
 *    (fg_open does not check the range). The handle stays usable.
 *  - No image (n_images == 0) or only foreign rows: a valid restore of an empty image.
 *  - Device memory during the call, freed on return: 8 B x columns (5, or 7 with min / max) per input
 *    row for FG_HOST images (they are uploaded whole), 8 B x (4, or 6) per kept row for the grouped
 *    batch, and 32 KiB + 12 B x state regions per distinct slice end for the histograms. */
typedef struct fg_restore_info {
    int64_t rows_in;        /* rows of all images */
    int64_t rows_kept;      /* rows whose key group lies in the handle's range */
    int64_t slices;         /* distinct slice ends among the kept rows */
    int64_t state_regions;  /* regions per slice table after the restore (fg_stats.state_regions) */
} fg_restore_info;
int  fg_restore_range(fg_handle* h, const fg_state_rows* images, int32_t n_images, int32_t location,
                      int32_t key_hash, int64_t timer_watermark, fg_restore_info* info /* may be NULL */);
int  fg_late_dropped(fg_handle* h, int64_t* out);
int  fg_get_stats(fg_handle* h, fg_stats* out);
int  fg_synchronize(fg_handle* h);
/* Drop all resident state and staged records, keep device allocations: a fresh operator
 * after open() + initializeState() from an empty snapshot. */
int  fg_reset(fg_handle* h);
/* Copies up to `max` kernel statistics into out; *count receives the number available. */
int  fg_kernel_stats(fg_handle* h, fg_kernel_stat* out, int32_t max, int32_t* count);
/* With FG_FLAG_KERNEL_TIMING: bracket only the kernel classes whose bit is set (bit i = entry
 * i of fg_kernel_stats' list); each bracket costs two events on the stream, so a measurement
 * times the kernel it reports and leaves the others unperturbed. Default: all classes. */
int  fg_set_kernel_timing(fg_handle* h, uint32_t class_mask);
/* Device stream of the handle (hipStream_t), for callers that overlap their own work. */
void* fg_stream(fg_handle* h);
const char* fg_last_error(fg_handle* h);   /* h may be NULL: last error of fg_open */
void fg_close(fg_handle* h);

/* Key-group routing (keyBy partitioner) on the device of `device_id`:
 * out_kg[i] = murmurHash(hash(key[i])) % max_parallelism, hash per fg_key_hash.
 * Pointers are device pointers when location == FG_DEVICE. */
int  fg_key_groups(int32_t device_id, int32_t location, int64_t n, const int64_t* key,
                   int32_t key_hash, int32_t max_parallelism, int32_t* out_kg);

/* Pack a batch for the key-group exchange: records are reordered by destination
 * subtask (kg * parallelism / max_parallelism) into the caller-provided device buffers,
 * counts[parallelism] receives per-destination record counts. Device pointers only. */
int  fg_partition_by_owner(int32_t device_id, void* stream, int64_t n, const int64_t* key,
                           const int64_t* rowtime, const int64_t* val, int32_t key_hash,
                           int32_t max_parallelism, int32_t parallelism, int64_t* out_key,
                           int64_t* out_rowtime, int64_t* out_val, int64_t* counts);

/* The same for `ncols` int64 columns moved together (cols[0] = the key), e.g. the partial
 * accumulator rows (key, slice_end, cnt_star, cnt_val, sum) of the two-phase exchange.
 * ncols <= 8. Device pointers only. */
int  fg_partition_columns_by_owner(int32_t device_id, void* stream, int64_t n, int32_t ncols,
                                   const int64_t* const* cols, int32_t key_hash, int32_t max_parallelism,
                                   int32_t parallelism, int64_t* const* out_cols, int64_t* counts);

/* The keyBy edge of the two-phase plan over RCCL (ABI 14; libflinkgpu.so links librccl): replaces,
 * between co-located subtasks, KeyGroupStreamPartitioner.selectChannel
 * (SJ/runtime/partitioner/KeyGroupStreamPartitioner.java:55-65) + RecordWriter.emit
 * (RT/io/network/api/writer/RecordWriter.java:101-128) on the edge LocalSlicingWindowAggOperator ->
 * GlobalSlicingWindowAggOperator, and StatusWatermarkValve's min over the input channels
 * (SJ/runtime/watermarkstatus/StatusWatermarkValve.java). One communicator per subtask (one process
 * per GPU): a coordinator (the JobManager) makes the id once with fg_comm_unique_id and ships its
 * bytes with the deployment; every subtask calls fg_comm_open(device, parallelism, its index, id),
 * which blocks until all have joined. Owner of a row = computeOperatorIndexForKeyGroup(key group)
 * (KeyGroupRangeAssignment.java:124-127) with fg_key_hash routing. Per exchange: the rows grouped by
 * owner on the device, ONE all-to-all of (row count, this rank's watermark) per peer, ONE host read
 * of them, grouped send / receive of each column's runs. Collective: every rank calls the same
 * exchanges in the same order (a rank with no rows still calls). Keys that are ids of per-rank
 * dictionaries (FG_KEYHASH_DICT_ID) cross as key rows once fg_comm_set_key_dicts (below, after the
 * key dictionary) has attached the subtask's dictionaries; without it ids move as they are. */
#define FG_COMM_ID_BYTES 128
typedef struct fg_comm fg_comm;
typedef struct fg_exchanged {
    int64_t n;                        /* rows received (this rank's key groups) */
    int32_t ncols;
    int32_t reserved0;
    const int64_t* cols[8];           /* device columns, communicator-owned, valid until the next exchange;
                                       * complete in stream order on fg_comm_stream */
    int64_t min_watermark;            /* min over the ranks of the watermarks passed in (StatusWatermarkValve) */
    int64_t bytes_sent;               /* to other ranks */
} fg_exchanged;
int  fg_comm_unique_id(uint8_t* id /* FG_COMM_ID_BYTES */);
int  fg_comm_open(int32_t device_id, int32_t world, int32_t rank, const uint8_t* id, fg_comm** out);
/* ncols <= 8 int64 device columns (cols[0] = key) produced on `stream` (hipStream_t; the
 * communicator's stream waits for it), grouped by owner and exchanged. */
int  fg_comm_exchange_columns(fg_comm* c, void* stream, int64_t n, int32_t ncols, const int64_t* const* cols,
                              int32_t key_hash, int32_t max_parallelism, int64_t watermark, fg_exchanged* out);
/* The local operator's partial rows (FG_DEVICE rows of a FG_FLAG_LOCAL_PARTIALS handle: key,
 * window_end = slice end, agg[0..2] or [0..4]) exchanged and merged into this rank's global operator
 * (fg_add_partials on `global`, ordered after the collective on its stream). *min_watermark receives
 * the combined watermark the caller then advances `global` to. */
int  fg_comm_exchange_partials(fg_comm* c, fg_handle* local, const fg_rows* rows, int32_t key_hash,
                               int32_t max_parallelism, int64_t watermark, fg_handle* global, int64_t* min_watermark);
/* fg_comm_exchange_partials of the rows fg_collect_fired(local) returns (the local fires of the
 * async advances since the last collect) -- a shim's per-batch call: LocalSlicingWindowAggOperator
 * .processWatermark's output edge. */
int  fg_comm_exchange_fired(fg_comm* c, fg_handle* local, int32_t key_hash, int32_t max_parallelism,
                            int64_t watermark, fg_handle* global, int64_t* min_watermark);
/* ... of fg_flush_partials(local) (LocalSlicingWindowAggOperator.prepareSnapshotPreBarrier :142-144:
 * the local buffer crosses the edge before the barrier). */
int  fg_comm_exchange_flushed(fg_comm* c, fg_handle* local, int32_t key_hash, int32_t max_parallelism,
                              int64_t watermark, fg_handle* global, int64_t* min_watermark);
/* The exchange as a round of three calls (ABI 16), for a subtask whose edge runs on a thread of its
 * own: the operators are touched only in _begin (the local rows collected or flushed and grouped by
 * owner) and _end (the received rows merged into `global`), never while _exchange waits for the
 * peers. Every rank runs the same sequence of rounds: a rank with nothing to send still begins an
 * FG_ROUND_IDLE round. The meta words of a round carry each rank's watermark and epoch (the id of
 * the last checkpoint whose pre-barrier flush it has sent) and a failure flag: a rank whose _begin
 * failed still takes part, sending no rows, and _exchange then fails on EVERY rank with FG_EDEVICE
 * (fg_round.failed_rank) instead of leaving the peers blocked in the data collective. After a
 * _begin -- whatever it returned -- the caller calls _exchange; _end after an _exchange that
 * returned FG_OK. */
#define FG_ROUND_FIRED 0     /* the local handle's uncollected async fires (fg_collect_fired) */
#define FG_ROUND_FLUSHED 1   /* the local buffer (fg_flush_partials: before a checkpoint barrier) */
#define FG_ROUND_IDLE 2      /* nothing to send (local may be NULL) */
typedef struct fg_round {
    int64_t min_watermark;   /* min over the ranks of the watermarks passed to _begin (StatusWatermarkValve) */
    int64_t min_epoch;       /* min over the ranks of the epochs passed to _begin */
    int64_t rows_sent;       /* this rank's rows (to every rank, itself included) */
    int64_t rows_received;
    int64_t bytes_sent;      /* to other ranks */
    int32_t failed_rank;     /* -1, or the lowest rank whose round failed (world: column counts disagree) */
    int32_t reserved0;
} fg_round;
int  fg_comm_round_begin(fg_comm* c, fg_handle* local, int32_t mode, int32_t key_hash, int32_t max_parallelism,
                         int64_t watermark, int64_t epoch);
int  fg_comm_round_exchange(fg_comm* c, fg_round* out);
int  fg_comm_round_end(fg_comm* c, fg_handle* global);
void* fg_comm_stream(fg_comm* c);
int64_t fg_comm_bytes_sent(fg_comm* c);      /* bytes sent to other ranks by every exchange so far */
const char* fg_comm_last_error(fg_comm* c);   /* c may be NULL: last error of fg_comm_open / _unique_id */
void fg_comm_close(fg_comm* c);

/* Grouping keys of any type (STRING, several key columns ...): a GPU-resident dictionary of the
 * serialized key rows. The reference groups by the BinaryRowData key row the key selector
 * projects (BinaryRowDataKeySelector.java:43-50); two keys are equal iff their rows' bytes are
 * (BinarySection.equals, BinarySection.java:62-73), and the key group comes from
 * MurmurHashUtils.hashBytesByWords over those bytes, seed 42 (BinarySection.hashCode :76-78,
 * MurmurHashUtils.java:92-96,131-170) -> KeyGroupRangeAssignment. fg_key_dict_intern maps each row
 * to a 64-bit id: equal rows -> equal ids, distinct rows -> distinct ids (exact: a hash collision
 * is resolved by comparing the bytes), id = ordinal << ceil(log2(max_parallelism)) | key group (below
 * 2^31 for 16.7M keys at max parallelism 128, so the window engine stages them as 32-bit keys). The ids are the BIGINT key
 * column of fg_add_batch / the key field of fg_add_rows; FG_KEYHASH_DICT_ID routes them by the
 * carried key group; fired rows' ids map back to their rows with fg_key_dict_rows. A handle is
 * single-threaded like fg_handle; an id is stable until fg_key_dict_retain retires it -- for the
 * dictionary's life if that is never called (a restored operator re-interns the key rows of its
 * state image first). */
typedef struct fg_key_dict fg_key_dict;
int  fg_key_dict_open(int32_t device_id, int32_t max_parallelism, int64_t expected_keys, fg_key_dict** out);
/* n key rows: row i = bytes[offsets[i], offsets[i] + lengths[i]) (nbytes = the buffer's size),
 * each length and offset a multiple of 4 (BinaryRowData rows are multiples of 8; rows may
 * overlap). out_id[n] receives the ids, out_kg[n] (optional) the rows' key groups under the
 * dictionary's max parallelism. All pointers FG_HOST or all FG_DEVICE (location). FG_DEVICE
 * inputs are read on the dictionary's stream (fg_key_dict_stream): the caller orders their
 * producer before it; the outputs are complete when the call returns. */
int  fg_key_dict_intern(fg_key_dict* d, int32_t location, int64_t n, const uint8_t* bytes, int64_t nbytes,
                        const int64_t* offsets, const int32_t* lengths, int64_t* out_id, int32_t* out_kg);
/* fg_key_dict_intern of device rows in two halves (ABI 13): _async launches the lookup of every
 * row on the dictionary's stream (fg_key_dict_stream) and returns at once; _wait synchronizes,
 * interns the rows the table did not hold yet and resolves tag collisions -- out_id / out_kg are
 * complete when it returns. A key selector interns the next micro-batch's rows while the engine
 * aggregates the current one. One call pending per dictionary (FG_ESTATE otherwise); bad rows are
 * reported by _wait, before anything is inserted. */
int  fg_key_dict_intern_async(fg_key_dict* d, int64_t n, const uint8_t* bytes, int64_t nbytes, const int64_t* offsets,
                              const int32_t* lengths, int64_t* out_id, int32_t* out_kg);
int  fg_key_dict_intern_wait(fg_key_dict* d);
/* For each id: its row's offset and length in the dictionary's arena (-1 / -1 for an unknown id). */
int  fg_key_dict_lookup(fg_key_dict* d, int32_t location, int64_t n, const int64_t* ids, int64_t* out_offsets,
                        int32_t* out_lengths);
/* The key rows of n ids, packed, in the order of the ids (ABI 16, added): the way out of the
 * dictionary, one gather on the device instead of fg_key_dict_lookup + a copy of the arena range
 * the ids span. The layout is the one fg_key_dict_intern reads, so the output of one dictionary
 * is valid input to the intern of another (rescale: a new subtask re-interns the key rows of
 * every old image):
 *   row i = out_bytes[out_offsets[i], out_offsets[i] + out_lengths[i]);
 *   out_offsets has n + 1 entries: out_offsets[0] = 0, out_offsets[i + 1] = out_offsets[i] +
 *   ((out_lengths[i] + 7) & ~7), out_offsets[n] = *out_nbytes; the pad bytes are zero (zero
 *   padding to 8); a repeated id gets a copy of its row per occurrence.
 * location is FG_HOST (ids and the three outputs are host memory, pageable or pinned: the packed
 * bytes, the offsets and the lengths are copied straight into them -- 8 + 12 n + *out_nbytes
 * bytes and one 24-byte read of the call's counters cross to the host, no arena range) or
 * FG_DEVICE (all four are device pointers, read and written on the dictionary's stream under
 * the ordering rule of fg_key_dict_intern; out_bytes 8-byte aligned). out_nbytes is always a
 * host pointer. The outputs are complete when the call returns. Returns
 *   FG_EFULL   *out_nbytes > cap_bytes: out_offsets, out_lengths and *out_nbytes are complete,
 *              out_bytes is untouched; call again with a larger buffer. out_bytes NULL with
 *              cap_bytes 0 is the sizing call;
 *   FG_EINVAL  before any device work: a NULL dictionary, n < 0 or n > 2^31 - 1, n > 0 with a
 *              NULL ids / out_offsets / out_lengths / out_nbytes, cap_bytes < 0, cap_bytes > 0
 *              with a NULL out_bytes, an unknown location, a misaligned device out_bytes;
 *   FG_EINVAL  after the length pass: an id that is negative or whose ordinal is not below
 *              fg_key_dict_size -- the message gives how many and the lowest such index;
 *              nothing is written to out_bytes;
 *   FG_ESTATE  while an async intern is pending, as fg_key_dict_lookup.
 * n == 0: FG_OK, *out_nbytes = 0, out_offsets[0] = 0 if out_offsets is non-NULL (no kernel runs;
 * a device out_offsets takes one 8-byte memset). The dictionary is not modified and stays usable
 * after every error. Rows of any length up to the intern's limit (2^24 - 4 bytes) come out
 * right; one very long row is copied by a single workgroup. */
int  fg_key_dict_rows(fg_key_dict* d, int32_t location, int64_t n, const int64_t* ids,
                      uint8_t* out_bytes, int64_t cap_bytes,
                      int64_t* out_offsets /* [n + 1] */, int32_t* out_lengths /* [n] */,
                      int64_t* out_nbytes /* always a host pointer */);
/* The key selector on the GPU (ABI 16, added): the key rows of n packed BinaryRowData records,
 * projected the way the reference's BinaryRowDataKeySelector.getKey does (the generated projection
 * writing through BinaryRowWriter, BinaryRowDataKeySelector.java:43-50), plus up to
 * FG_PROJ_MAX_COLS 8-byte fields copied out as columns (rowtime, value) -- the way into the
 * dictionary for a GROUP BY on a STRING column, several key columns or a nullable key, with no
 * per-record host work. Input records are whole rows, fixed-length part and variable-length part:
 *   row i = bytes[offsets[i], offsets[i] + lengths[i]) (nbytes = the buffer's size) -- the layout
 *   fg_key_dict_intern reads, except that every offset and length is a multiple of 8 (a
 *   BinaryRowData's size always is); proj->arity is the rows' field count.
 * location is FG_HOST or FG_DEVICE and covers every pointer except proj, the two pointer arrays
 * out_cols / out_col_null (host arrays of pointers at `location`) and out_nbytes (always a host
 * pointer). FG_HOST inputs (pageable or pinned) are copied up on the dictionary's stream and the
 * host outputs are complete when the call returns; FG_DEVICE pointers are read and written on the
 * dictionary's stream (fg_key_dict_stream) under the ordering rule of fg_key_dict_intern, complete
 * when the call returns; device bytes and out_key_bytes are 8-byte aligned. The dictionary lends
 * its stream, scratch, timing and error text: fg_key_dict_project does not modify it.
 * The key row of an input row is byte-exact (little endian, k = n_key_fields):
 *   header     8 bytes of bit set (((k + 71) / 64) * 8): byte 0 is RowKind INSERT = 0 whatever the
 *              input row's RowKind; bit 8 + f is set iff input field key_field[f] is NULL, and its
 *              slot is then eight zero bytes (BinaryRowWriter.setNullAt);
 *   slots      8 bytes per key field. FG_FIELD_FIXw copies the low w bytes of the input slot and
 *              zeroes the rest (canonical whatever the input slot holds there);
 *   FG_FIELD_VAR  is decoded from the input slot either way -- top bit set: inline, len = bits
 *              56..62, data in the low bytes; otherwise offset << 32 | len, the offset from the
 *              row's start -- and re-encoded as BinaryRowWriter.writeString / writeBytes does
 *              (AbstractBinaryWriter.java:81-105,280-330): len <= 7 inline (0x80 | len in the top
 *              byte, unused bytes zero), also when the input kept it in its variable part; a longer
 *              one in the key row's variable part, the fields in key-field order, each zero-padded
 *              to 8 (its last word masked by its length, not trusted from the input), the slot
 *              holding key_row_offset << 32 | len, the first offset being 8 * (k + 1).
 *   out_key_lengths[i] is the row's length (a multiple of 8); out_key_offsets has n + 1 entries,
 *   the prefix of the lengths: [0] = 0, [n] = *out_nbytes; rows are packed back to back. The
 *   output is valid input to fg_key_dict_intern, on the device or on the host.
 * Columns: out_cols[c][i] = the 8 bytes of field col_field[c], 0 when it is NULL; out_col_null[c][i]
 * = 1 for NULL, 0 otherwise, where that pointer is non-NULL (out_col_null itself may be NULL).
 * A row is bad if its offset or length is negative or not a multiple of 8, offsets[i] + lengths[i] >
 * nbytes, lengths[i] is smaller than the fixed-length part of `arity` fields, a non-NULL
 * FG_FIELD_VAR key field is inline with a length above 7, lies in the variable part at an offset
 * that is not a multiple of 8 or is below the fixed-length part, or has offset + len beyond the
 * row's length, its key row would exceed the intern's limit of 2^24 - 4 bytes, or a column field
 * is NULL while its out_col_null[c] is NULL (the fg_add_rows rule: a NULL key or rowtime is
 * FG_EINVAL). Bad rows are found in the length pass; no byte is read through an unchecked offset.
 * Returns
 *   FG_EFULL   (_project) *out_nbytes > cap_bytes: out_key_offsets, out_key_lengths, the columns
 *              and *out_nbytes are complete, out_key_bytes is untouched. out_key_bytes NULL with
 *              cap_bytes 0 is the sizing call;
 *   FG_EINVAL  before any device work: a NULL d or proj; an unknown location; n < 0 or n > 2^31 - 1;
 *              nbytes < 0; n > 0 with a NULL bytes / offsets / lengths / out_key_offsets /
 *              out_key_lengths / out_nbytes (_project) or a NULL out_id (_intern_fields); arity
 *              outside 1..32767, n_key_fields outside 1..FG_PROJ_MAX_KEY_FIELDS, n_cols outside
 *              0..FG_PROJ_MAX_COLS; a field index outside 0..arity - 1; an unknown kind; n > 0 and
 *              n_cols > 0 with a NULL out_cols or a NULL entry; cap_bytes < 0, or cap_bytes > 0 with a NULL
 *              out_key_bytes; misaligned device bytes or out_key_bytes;
 *   FG_EINVAL  after the length pass (one host read of {total, bad rows, lowest bad index}, as
 *              fg_key_dict_rows): any bad row -- the message gives how many and the lowest index; no
 *              key byte is written and nothing is interned;
 *   FG_ESTATE  while an async intern is pending.
 * n == 0: FG_OK, *out_nbytes = 0, out_key_offsets[0] = 0 where non-NULL, no kernel runs. The
 * dictionary stays usable after every error. A long string is copied by a whole workgroup.
 * fg_key_dict_set_timing class "dict_project": all of a projection's kernels, records = the input
 * rows, rows = the key bytes written; listed only once the dictionary has projected. */
enum fg_field_kind { FG_FIELD_FIX1 = 1,   /* BOOLEAN, TINYINT */
                     FG_FIELD_FIX2 = 2,   /* SMALLINT */
                     FG_FIELD_FIX4 = 4,   /* INT, DATE, TIME, FLOAT */
                     FG_FIELD_FIX8 = 8,   /* BIGINT, DOUBLE, TIMESTAMP(<=3) compact */
                     FG_FIELD_VAR  = 16 };/* CHAR / VARCHAR / STRING / BINARY / VARBINARY */
#define FG_PROJ_MAX_KEY_FIELDS 8
#define FG_PROJ_MAX_COLS 4
typedef struct fg_row_projection {
    int32_t arity;                                /* fields of an input row, 1 .. 32767 */
    int32_t n_key_fields;                         /* 1 .. FG_PROJ_MAX_KEY_FIELDS */
    int32_t key_field[FG_PROJ_MAX_KEY_FIELDS];    /* input field of key field f (any order, repeats allowed) */
    int32_t key_kind[FG_PROJ_MAX_KEY_FIELDS];     /* fg_field_kind */
    int32_t n_cols;                               /* 0 .. FG_PROJ_MAX_COLS */
    int32_t col_field[FG_PROJ_MAX_COLS];          /* 8-byte input fields copied out as columns (rowtime, value) */
} fg_row_projection;
int  fg_key_dict_project(fg_key_dict* d, int32_t location, int64_t n,
                         const uint8_t* bytes, int64_t nbytes, const int64_t* offsets, const int32_t* lengths,
                         const fg_row_projection* proj,
                         uint8_t* out_key_bytes, int64_t cap_bytes,
                         int64_t* out_key_offsets /* [n + 1] */, int32_t* out_key_lengths /* [n] */,
                         int64_t* const* out_cols /* [n_cols] columns of n, may be NULL when n_cols == 0 */,
                         uint8_t* const* out_col_null /* [n_cols], each entry may be NULL */,
                         int64_t* out_nbytes /* always a host pointer */);
/* fg_key_dict_project into dictionary-owned device scratch, then fg_key_dict_intern of those rows:
 * records in, ids (and columns) out. out_id[n] are the ids fg_key_dict_intern returns for the same
 * key rows (equal keys give equal ids; a key first seen through either entry point is found by the
 * other), out_kg[n] (optional) their key groups. Arguments, bad rows and errors as above; the
 * scratch grows to the largest call and is freed at fg_key_dict_close. There is no async form. */
int  fg_key_dict_intern_fields(fg_key_dict* d, int32_t location, int64_t n,
                               const uint8_t* bytes, int64_t nbytes, const int64_t* offsets, const int32_t* lengths,
                               const fg_row_projection* proj,
                               int64_t* out_id, int32_t* out_kg /* optional */,
                               int64_t* const* out_cols, uint8_t* const* out_col_null);
/* fg_partition_columns_by_owner for rows keyed by ids of dictionary d (cols[0] = ids; owner from the key
 * group an id carries, FG_KEYHASH_DICT_ID, under d's max parallelism), plus what the owner needs to know
 * the keys: the key rows of the grouped ids, packed back to back in the grouped order, each zero-padded
 * to 8 bytes (the fg_key_dict_rows layout without its offsets), their lengths, and the key bytes per owner
 * (ABI 16, added): the sender half of the keyed two-phase edge, at any `parallelism` on one device.
 * All pointers except out_nbytes are device pointers. The work is queued on `stream` (hipStream_t)
 * after everything queued on the dictionary's stream, and everything is complete when the call
 * returns: it reads {total, bad ids} back once, as fg_key_dict_rows does. Row i of the grouped
 * output has its key row at the exclusive prefix of the padded lengths ((len + 7) & ~7) of rows
 * 0 .. i-1, and that key row is the row of out_cols[0][i]; the order inside an owner's run is
 * unspecified (the partition is an atomic counting sort), but the columns, the lengths and the
 * bytes agree with each other position by position. Returns
 *   FG_EFULL   *out_nbytes > cap_bytes: out_cols, counts, out_key_lengths, out_byte_counts and
 *              *out_nbytes are complete, out_key_bytes is untouched. out_key_bytes NULL with
 *              cap_bytes 0 is the sizing call;
 *   FG_EINVAL  before any device work: a NULL d; n < 0 or n > 2^31 - 1; ncols outside 1..8;
 *              parallelism outside 1..min(1024, d's max parallelism); n > 0 with a NULL column or
 *              output; cap_bytes < 0, or > 0 with a NULL out_key_bytes; a misaligned out_key_bytes;
 *   FG_EINVAL  after the length pass: an id that is negative or whose ordinal is not below
 *              fg_key_dict_size -- the message gives how many and the lowest grouped index; no key
 *              byte is written;
 *   FG_ESTATE  while an async intern is pending.
 * n == 0: counts and out_byte_counts are zeroed (where non-NULL) and *out_nbytes = 0. The
 * dictionary is not modified and stays usable after every error. */
int  fg_partition_keyed_by_owner(fg_key_dict* d, void* stream, int64_t n, int32_t ncols,
        const int64_t* const* cols, int32_t parallelism, int64_t* const* out_cols,
        int64_t* counts            /* device [parallelism] */,
        int32_t* out_key_lengths   /* device [n], grouped order */,
        uint8_t* out_key_bytes, int64_t cap_bytes /* device, 8-byte aligned */,
        int64_t* out_byte_counts   /* device [parallelism]: sum of padded lengths per owner */,
        int64_t* out_nbytes        /* host */);
/* The dictionaries of a subtask whose grouping keys are dictionary ids: from now on every exchange
 * with key_hash == FG_KEYHASH_DICT_ID ships each row's key row and the receiver's key column holds ids
 * of global_keys. Both NULL detaches. FG_EINVAL: only one NULL, different max parallelism, a device
 * other than the communicator's. Every rank of a job attaches, or none does (ranks that disagree
 * fail their round together, fg_round.failed_rank = world).
 * With dictionaries attached, fg_comm_round_* and fg_comm_exchange_partials / _fired / _flushed
 * (fg_comm_exchange_columns stays unkeyed): _begin groups the local rows with
 * fg_partition_keyed_by_owner over local_keys at `world` owners -- max_parallelism must be the
 * dictionaries'; the gather of the key rows has completed when _begin returns; an unknown id, a
 * pending async intern or a device error there is this rank's failed round, reported through the
 * meta words like any other; _exchange moves, with the columns, 4 bytes of length per row and the
 * key bytes (every row carries its key: the round is stateless, a failed one needs no repair) and
 * counts them in bytes_sent; _end checks what it received (FG_EDEVICE, nothing interned, for a
 * length that is negative, not a multiple of 4 or >= 2^24, or lengths that do not add up to the
 * bytes received), interns it into global_keys and merges the rows under those ids.
 * A dictionary handle is single-threaded: fg_comm uses local_keys only inside _begin and
 * global_keys only inside _end (the one-call forms use both), so the lock under which the caller
 * makes those calls (its operator lock) must also cover its own use of the two dictionaries. */
int  fg_comm_set_key_dicts(fg_comm* c, fg_key_dict* local_keys, fg_key_dict* global_keys);
/* Retire keys without state and reuse their ids (ABI 16, added). The reference clears the keyed
 * state of a (key, window) when the window expires; a dictionary that only grows keeps a slot, an
 * arena entry and an ordinal for every key ever seen. fg_key_dict_retain keeps exactly the listed
 * ids (the key column of a state image), retires every other entry, compacts the arena, rebuilds the
 * table and hands the retired ordinals out again; fg_key_dict_get_stats reports the sizes. A
 * dictionary that never calls retain behaves as before.
 *   ids[0 .. n_sets) and counts are host arrays (n_sets 0..16: one image per handle or slice, no
 *   concatenation); the arrays ids[k] point to hold counts[k] ids each (0 .. 2^31 - 1) and are all
 *   FG_HOST or all FG_DEVICE (location); device arrays are read on the dictionary's stream under the
 *   ordering rule of fg_key_dict_intern. Duplicates are allowed. The call is synchronous: everything
 *   below is complete when it returns. `out` (optional) receives the stats after the call.
 * Every listed id is validated before anything changes: it is invalid if it is negative, its ordinal
 * is >= issued, its entry is retired, or the id stored in its arena entry differs (a stale id whose
 * ordinal was reused under another key group). Returns
 *   FG_EINVAL  a NULL d, an unknown location, n_sets outside 0..16, a NULL ids / counts with
 *              n_sets > 0, a count outside [0, 2^31), a NULL set with a count > 0; or, after one
 *              host read of the call's counters (as fg_key_dict_rows), an invalid id -- the message
 *              gives how many and the lowest (set, index); the dictionary is unchanged;
 *   FG_ESTATE  while an async intern is pending; the dictionary is unchanged;
 *   FG_EDEVICE a device error; the new arena, table and free list are allocated before anything is
 *              modified, so a failed allocation leaves the dictionary unchanged.
 * Kept ids keep their id and their row: fg_key_dict_rows, fg_key_dict_lookup, fg_key_dict_intern of
 * the row and fg_partition_keyed_by_owner answer as before. Every other entry is retired: its row is
 * no longer in the table (a later intern of the same bytes is a new key), its arena bytes are gone,
 * fg_key_dict_rows and fg_partition_keyed_by_owner report its id as unknown (as an id past the size)
 * and fg_key_dict_lookup gives -1 / -1 -- until its ordinal is reused, after which the id may be
 * another key's. The contract: after retain the caller holds no id outside the live sets.
 * n_sets == 0, or all counts 0, is legal and empties the dictionary. Later interns take the lowest
 * free ordinals first and fresh ones only when none is free, so `issued` is the largest number of
 * keys ever alive at once (up to rows resolved on the host after a tag collision, which take fresh
 * ordinals), not the number ever seen -- ids stay below 2^31 on a bounded live set. After the call
 * arena_bytes is exactly the sum of 8 + ((len + 7) & ~7) over the live rows, and the table has
 * min(current, max(slots at open, pow2 >= FG_DICT_GROW x (live + 2^20))) slots. */
typedef struct fg_key_dict_stats {
    int64_t live;            /* = fg_key_dict_size */
    int64_t issued;          /* ordinals ever handed out: every id is below issued << kg_bits */
    int64_t free_ordinals;   /* retired ordinals not yet reused */
    int64_t arena_bytes;     /* arena bytes in use */
    int64_t table_slots;
    int64_t side_rows;       /* rows resolved on the host (tag collisions) */
    int64_t retired_total;   /* entries retired by all retain calls */
    int64_t reserved0;
} fg_key_dict_stats;
int  fg_key_dict_get_stats(fg_key_dict* d, fg_key_dict_stats* out);
int  fg_key_dict_retain(fg_key_dict* d, int32_t location, int32_t n_sets,
                        const int64_t* const* ids, const int64_t* counts,
                        fg_key_dict_stats* out /* optional */);
/* The arena (device memory, rows padded to 8 bytes) and its used size; valid until the next intern
 * or retain. */
int  fg_key_dict_arena(fg_key_dict* d, const uint8_t** dev_bytes, int64_t* size);
int  fg_key_dict_copy_arena(fg_key_dict* d, int64_t begin, int64_t nbytes, uint8_t* host);
int64_t fg_key_dict_size(fg_key_dict* d);   /* distinct key rows interned and not retired (live) */
void* fg_key_dict_stream(fg_key_dict* d);   /* the dictionary's device stream (hipStream_t) */
/* HIP-event timing of the dictionary's kernels (per chunk: "dict_probe", then "dict_assign" =
 * assign + verify of the rows new in the chunk; per fg_key_dict_rows call: "dict_rows" = all of
 * the call's kernels, records = its ids; per fg_key_dict_retain call: "dict_retain" = all of the
 * call's kernels, records = the ordinals issued, rows = the entries kept; per table rebuild, when
 * the table grows and inside every retain: "dict_rebuild" = the clear and the rehash, records = the
 * ordinals, rows = the slots); fg_key_dict_kernel_stats copies them. */
int  fg_key_dict_set_timing(fg_key_dict* d, int32_t on);
int  fg_key_dict_kernel_stats(fg_key_dict* d, fg_kernel_stat* out, int32_t max, int32_t* count);
const char* fg_key_dict_last_error(fg_key_dict* d);
void fg_key_dict_close(fg_key_dict* d);
/* BinarySection.hashCode of one row (MurmurHashUtils.hashBytesByWords, seed 42); len % 4 == 0. */
int32_t fg_binaryrow_hash(const uint8_t* row, int32_t len);

/* Page-lock a caller range for FG_HOST input (hipHostRegister): Flink's managed memory is
 * off-heap MemorySegments (MemorySegmentFactory.allocateOffHeapUnsafeMemory,
 * CO/core/memory/MemorySegmentFactory.java:130-167; address MemorySegment.getAddress :288)
 * that live for the operator's life, so a shim registers each segment it hands batches from
 * once, at open, and unregisters it at close. Batches read from a registered range are DMA'd
 * directly; pageable ranges are staged by the runtime at a lower rate. Not per handle: the
 * registration serves every handle on the device. Errors: fg_last_error(NULL). */
int  fg_host_register(int32_t device_id, void* p, int64_t bytes);
int  fg_host_unregister(int32_t device_id, void* p);

int  fg_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLINKGPU_H */
