/*
 * Natives of libflinkgpu_jni.so (jni/flink_gpu_jni.c), one per C-ABI entry point of
 * include/flinkgpu.h. Every ByteBuffer is a direct buffer in native byte order (a wrapped
 * off-heap MemorySegment, MemorySegment.java:288,307, or ByteBuffer.allocateDirect).
 */
package org.apache.flink.table.runtime.operators.window.gpu;

import java.nio.ByteBuffer;

/** JNI entry points of the MI355X window-aggregation engine. */
public final class FlinkGpu {

    static {
        System.loadLibrary("flinkgpu_jni");
    }

    private FlinkGpu() {}

    /** fg_open: config is an fg_config image (FgConfig); zone rules as arrays (may be null). */
    public static native long open(ByteBuffer config, long[] tzTransitions, long[] tzOffsets);

    /** fg_add_batch (FG_HOST): the buffers may be refilled as soon as the call returns. */
    public static native void addBatch(
            long h, ByteBuffer key, ByteBuffer rowtime, ByteBuffer val, ByteBuffer valNull, int n);

    /**
     * fg_add_batch with fg_batch.format: FORMAT_KEY32 (int keys), FORMAT_ROWTIME32 (rowtime as
     * unsigned int offsets from rowtimeBase), FORMAT_VAL32 (int BIGINT values) -- 16 instead of
     * 24 bytes per record over PCIe for a DOUBLE value.
     */
    public static native void addBatchNarrow(
            long h,
            int format,
            ByteBuffer key,
            ByteBuffer rowtime,
            long rowtimeBase,
            ByteBuffer val,
            ByteBuffer valNull,
            int n);

    public static final int FORMAT_KEY32 = 1;
    public static final int FORMAT_ROWTIME32 = 2;
    public static final int FORMAT_VAL32 = 4;

    /** fg_add_rows: n packed BinaryRowData fixed-length parts, stride bytes apart. */
    public static native void addRows(
            long h,
            ByteBuffer rows,
            int n,
            int stride,
            int arity,
            int keyField,
            int rowtimeField,
            int valField);

    /** fg_add_partials (GlobalAggCombiner.combine); min / max null unless several accumulators. */
    public static native void addPartials(
            long h,
            int n,
            ByteBuffer key,
            ByteBuffer sliceEnd,
            ByteBuffer cntStar,
            ByteBuffer cntVal,
            ByteBuffer sum,
            ByteBuffer min,
            ByteBuffer max);

    /**
     * fg_advance_progress: fills cols with key, window_start, window_end, agg[0..numAggs),
     * null_mask, rowtime (library-owned, valid until the next call); returns the row count. In run
     * mode ({@link #setFiredRuns}) the window_start, window_end and rowtime entries stay null.
     */
    public static native long advanceProgress(long h, long watermark, ByteBuffer[] cols);

    /**
     * fg_advance_progress_async: the watermark's fires are queued and the call returns at once; the
     * caller holds the watermark until {@link #collectFired} has returned the fired rows.
     */
    public static native void advanceProgressAsync(long h, long watermark);

    /** fg_advance_progress_async_n: watermarks[0..n) in order, as n advanceProgressAsync calls. */
    public static native void advanceProgressAsyncN(long h, long[] watermarks, int n);

    /**
     * fg_collect_fired_to(FG_HOST): waits for the fires of every async advance since the last
     * collect; fills cols as {@link #advanceProgress} (host memory); returns the row count.
     */
    public static native long collectFired(long h, ByteBuffer[] cols);

    /**
     * fg_set_fired_runs (ABI 16): run mode -- advanceProgress and collectFired leave the
     * window_start, window_end and rowtime entries of cols null (the engine neither stores nor
     * copies these per-fire constants) and {@link #firedRuns} says which rows belong to which
     * window. Refused for FG_FLAG_LOCAL_PARTIALS handles and with allowed lateness
     * (IllegalArgumentException), and while fired rows are uncollected.
     */
    public static native void setFiredRuns(long h, boolean on);

    /**
     * fg_fired_runs: the runs of the rows the last advanceProgress / collectFired returned, as
     * [n, windowStart[n], windowEnd[n], firstRow[n], rows[n]]: run i covers rows [firstRow[i],
     * firstRow[i] + rows[i]); their rowtime is windowEnd[i] - 1. A window may appear in more than
     * one run.
     */
    public static native long[] firedRuns(long h);

    /**
     * fg_set_fired_topn (ABI 16): Window Top-N on the GPU -- advanceProgress and collectFired
     * return, per fired window, only the n rows ranking first by agg[aggIndex] (windows by ascending
     * end, rows in rank order; NULL smallest, ties to the smaller key); n = 0 turns it off. Refused
     * for FG_FLAG_LOCAL_PARTIALS handles and with allowed lateness (IllegalArgumentException), and
     * while fired rows are uncollected.
     */
    public static native void setFiredTopN(long h, int n, int aggIndex, boolean descending);

    /** fg_advance_progress(FG_DEVICE): the fired rows stay on the device (nothing is copied); their count. */
    public static native long advanceProgressDevice(long h, long watermark);

    /** fg_collect_fired: as {@link #collectFired}, the rows left on the device; their count. */
    public static native long collectFiredDevice(long h);

    /** fg_pack_flags: the key (or dictionary id) is field 0 of the packed rows */
    public static final int PACK_KEY_FIELD = 1;

    /**
     * fg_fired_packed(FG_HOST) (ABI 16): rows [firstRow, firstRow + maxRows) of the rows the last
     * advanceProgress* / collectFired* returned, packed on the GPU into the fixed-length parts of
     * BinaryRowData rows of the fields [key,] agg[0..), window_start, window_end (BinaryRowData.pointTo
     * views them). out[0]: the rows (n * stride bytes), out[1]: their key column (null with
     * PACK_KEY_FIELD) -- library-owned host memory, valid until the next firedPacked or the next call
     * that changes the fired rows. shape: {arity, stride}. Returns n. IllegalArgumentException for a
     * range outside the rows and for DataStream / FG_FLAG_LOCAL_PARTIALS handles.
     */
    public static native long firedPacked(long h, long firstRow, long maxRows, int flags, ByteBuffer[] out, long[] shape);

    /**
     * fg_set_late_output (ABI 16): WindowedStream.sideOutputLateData -- every element the handle
     * would count in {@link #lateDropped} is kept instead and returned by {@link #collectLate}; the
     * counter does not move. DataStream handles only (IllegalArgumentException otherwise); turning
     * it off with uncollected records is refused.
     */
    public static native void setLateOutput(long h, boolean on);

    /**
     * fg_collect_late: the late elements of the batches since the last collect, in arrival order,
     * as [n, key[n], rowtime[n], valBits[n], null[n]]: valBits the value's long or the double's
     * bits (0 without a value column), null 1 for a NULL value. Drains the list. Called after each
     * batch, and in any case before a watermark is forwarded or a barrier taken.
     */
    public static native long[] collectLate(long h);

    /** fg_flush (prepareSnapshotPreBarrier). */
    public static native void flush(long h);

    /**
     * fg_flush_partials (FG_FLAG_LOCAL_PARTIALS handles): every buffered slice's partial rows, in
     * host memory; cols (length >= 10) as {@link #advanceProgress}; returns the row count.
     */
    public static native long flushPartials(long h, ByteBuffer[] cols);

    /**
     * fg_snapshot_state: cols (length 7) receives key, slice_end, cnt_star, cnt_val, sum, min, max;
     * timerWatermark[0] the timer watermark; returns the entry count.
     */
    public static native long snapshotState(long h, ByteBuffer[] cols, long[] timerWatermark);

    /**
     * fg_snapshot_state_async (ABI 15): the staged records flushed, the resident state exported on
     * the GPU and its copy into the host image queued; the handle takes further calls meanwhile.
     */
    public static native void snapshotStateAsync(long h);

    /** fg_snapshot_state_wait: the image of the last snapshotStateAsync, as snapshotState. */
    public static native long snapshotStateWait(long h, ByteBuffer[] cols, long[] timerWatermark);

    /**
     * fg_snapshot_slices (ABI 16): the slices of the image the last snapshotState / snapshotStateWait
     * returned, as [n, sliceEnd[n], firstRow[n], rows[n], changed[n] (1 / 0)].
     */
    public static native long[] snapshotSlices(long h);

    /**
     * fg_snapshot_plan (ABI 16): every resident slice, laid out as snapshotSlices returns an image's
     * slices ([n, sliceEnd[n], firstRow[n], rows[n], changed[n]]; firstRow: the slice's place in a full
     * image taken now), without exporting or copying a row; timerWatermark[0] as snapshotState returns
     * it. Valid for snapshotSelectAsync until any other call that may change the handle's state.
     */
    public static native long[] snapshotPlan(long h, long[] timerWatermark);

    /**
     * fg_snapshot_state_select_async: the planned slices i with want[i] != 0 (one long per planned
     * slice) exported (one kernel launch) and their copy to the host image queued; snapshotStateWait collects the image, and
     * snapshotSlices then lists the selected slices with compact firstRow.
     */
    public static native void snapshotSelectAsync(long h, long[] want);

    /**
     * fg_set_snapshot_grouping: from the next snapshot on, the rows of every slice of an image are
     * ordered by key group (keyHash, the handle's max parallelism), partitioned on the GPU before
     * the image leaves it; keyHash &lt; 0 turns the grouping off.
     */
    public static native void snapshotGrouping(long h, int keyHash);

    /**
     * fg_snapshot_key_groups: the index of the grouped image the last snapshotState /
     * snapshotStateWait returned, as [nSlices, maxP, firstRow[nSlices * maxP + 1]]: key group g of
     * slice s holds the image rows [firstRow[s * maxP + g], firstRow[s * maxP + g + 1]).
     */
    public static native long[] snapshotKeyGroups(long h);

    /** fg_restore. */
    public static native void restore(
            long h,
            int n,
            ByteBuffer key,
            ByteBuffer sliceEnd,
            ByteBuffer cntStar,
            ByteBuffer cntVal,
            ByteBuffer sum,
            ByteBuffer min,
            ByteBuffer max,
            long timerWatermark);

    /**
     * fg_restore_range over one host image: restore of the rows whose key group (keyHash, the
     * handle's max parallelism) lies in the handle's key-group range, filtered and grouped on the
     * GPU; returns the rows kept. What a subtask calls with every old subtask's image after a
     * restart at another parallelism.
     */
    public static native long restoreRange(
            long h,
            int n,
            ByteBuffer key,
            ByteBuffer sliceEnd,
            ByteBuffer cntStar,
            ByteBuffer cntVal,
            ByteBuffer sum,
            ByteBuffer min,
            ByteBuffer max,
            int keyHash,
            long timerWatermark);

    /** fg_late_dropped (numLateRecordsDropped). */
    public static native long lateDropped(long h);

    /** fg_close. */
    public static native void close(long h);

    /** fg_key_dict_open. */
    public static native long dictOpen(int device, int maxParallelism, long expectedKeys);

    /** fg_key_dict_intern (FG_HOST); outKeyGroups may be null. */
    public static native void dictIntern(
            long d,
            ByteBuffer rows,
            long nbytes,
            ByteBuffer offsets,
            ByteBuffer lengths,
            int n,
            ByteBuffer outIds,
            ByteBuffer outKeyGroups);

    /** fg_key_dict_lookup (FG_HOST). */
    public static native void dictLookup(
            long d, ByteBuffer ids, int n, ByteBuffer outOffsets, ByteBuffer outLengths);

    /**
     * fg_key_dict_rows (FG_HOST): the key rows of ids[0 .. n), packed in their order into
     * outBytes (row i at outOffsets[i], outLengths[i] bytes, padded with zeros to 8; outOffsets
     * holds n + 1 longs). Returns the bytes the rows take. A result above capBytes means outBytes
     * was too small and is untouched (outOffsets and outLengths are complete): grow it and call
     * again. outBytes may be null with capBytes 0.
     */
    public static native long dictRows(
            long d,
            ByteBuffer ids,
            int n,
            ByteBuffer outBytes,
            long capBytes,
            ByteBuffer outOffsets,
            ByteBuffer outLengths);

    /** fg_field_kind: how a key field is stored in its 8-byte slot (the bytes copied; VAR: CHAR / VARCHAR / BINARY). */
    public static final int FIELD_FIX1 = 1, FIELD_FIX2 = 2, FIELD_FIX4 = 4, FIELD_FIX8 = 8, FIELD_VAR = 16;

    /**
     * fg_key_dict_project (FG_HOST): the key rows of n serialized records (whole BinaryRowData rows:
     * record i at offsets[i], lengths[i] bytes, both multiples of 8), projected on the GPU the way
     * BinaryRowDataKeySelector.getKey projects them. projection = {arity, nKeyFields, nCols,
     * keyField[0], keyKind[0], ..., colField[0], ...}; outCols holds nCols columns of n longs back to
     * back (the 8 bytes of each column field, 0 for NULL), outColNull (may be null) nCols columns of
     * n bytes. The key rows come out as dictIntern reads them (outKeyOffsets holds n + 1 longs).
     * Returns the bytes they take; a result above capBytes means outKeyBytes was too small and is
     * untouched: grow it and call again.
     */
    public static native long dictProject(
            long d,
            ByteBuffer rows,
            long nbytes,
            ByteBuffer offsets,
            ByteBuffer lengths,
            int n,
            long[] projection,
            ByteBuffer outKeyBytes,
            long capBytes,
            ByteBuffer outKeyOffsets,
            ByteBuffer outKeyLengths,
            ByteBuffer outCols,
            ByteBuffer outColNull);

    /**
     * fg_key_dict_intern_fields (FG_HOST): dictProject into the dictionary's device scratch and
     * dictIntern of those key rows in one call -- serialized records in, ids (and columns) out;
     * outKeyGroups and outColNull may be null.
     */
    public static native void dictInternFields(
            long d,
            ByteBuffer rows,
            long nbytes,
            ByteBuffer offsets,
            ByteBuffer lengths,
            int n,
            long[] projection,
            ByteBuffer outIds,
            ByteBuffer outKeyGroups,
            ByteBuffer outCols,
            ByteBuffer outColNull);

    /**
     * fg_key_dict_retain (one FG_HOST set): keep exactly ids[0 .. n), retire every other entry and
     * reuse its ordinal for later interns; n == 0 empties the dictionary. Returns the 8 words of
     * fg_key_dict_stats after the call: [live, issued, freeOrdinals, arenaBytes, tableSlots,
     * sideRows, retiredTotal, 0]. After it the caller must hold no id outside ids.
     */
    public static native long[] dictRetain(long d, ByteBuffer ids, int n);

    /** fg_key_dict_get_stats: the 8 words as dictRetain returns them. */
    public static native long[] dictStats(long d);

    /** fg_key_dict_copy_arena. */
    public static native void dictCopyArena(long d, long begin, long nbytes, ByteBuffer out);

    /** fg_key_dict_close. */
    public static native void dictClose(long d);

    /**
     * fg_host_register: page-lock a whole direct buffer (an off-heap managed-memory segment,
     * MemorySegment.wrap) once, so batches handed from it are DMA'd without staging.
     */
    public static native void hostRegister(int device, ByteBuffer segment);

    /** fg_host_unregister (at close, before the segment is released to the MemoryManager). */
    public static native void hostUnregister(int device, ByteBuffer segment);

    // ---- the keyBy edge local -> global over RCCL (fg_comm; INTEGRATION.md section 7) ----

    /** fg_key_hash: a BIGINT key hashed as its BinaryRowData key row (FG_KEYHASH_BINARYROW_BIGINT). */
    public static final int KEYHASH_BINARYROW_BIGINT = 0;

    /** fg_key_hash: an id of a key dictionary, routed by the key group it carries (FG_KEYHASH_DICT_ID). */
    public static final int KEYHASH_DICT_ID = 2;

    /** Bytes of a communicator id (FG_COMM_ID_BYTES). */
    public static final int COMM_ID_BYTES = 128;

    /** fg_comm_unique_id: a new id into a direct buffer of COMM_ID_BYTES (the coordinator's). */
    public static native void commUniqueId(ByteBuffer id);

    /** fg_comm_open: this subtask's communicator (blocks until all `world` ranks joined). */
    public static native long commOpen(int device, int world, int rank, ByteBuffer id);

    /**
     * fg_comm_exchange_fired: the local handle's collected fires exchanged by key-group owner and
     * merged into the global handle; returns the combined watermark to advance the global to.
     */
    public static native long commExchangeFired(
            long comm, long local, int keyHash, int maxParallelism, long watermark, long global);

    /** fg_comm_exchange_flushed: the same for the local flush before a checkpoint barrier. */
    public static native long commExchangeFlushed(
            long comm, long local, int keyHash, int maxParallelism, long watermark, long global);

    /** fg_comm_round_begin modes (FG_ROUND_*). */
    public static final int ROUND_FIRED = 0;

    public static final int ROUND_FLUSHED = 1;
    public static final int ROUND_IDLE = 2;

    /**
     * fg_comm_round_begin (ABI 16): the local rows of the round grouped by owner (the operators are
     * touched here and in {@link #commRoundEnd}, never while {@link #commRoundExchange} waits). A
     * failed begin still takes part: call commRoundExchange after it whatever it threw.
     */
    public static native void commRoundBegin(
            long comm, long local, int mode, int keyHash, int maxParallelism, long watermark, long epoch);

    /**
     * fg_comm_round_exchange: the round's collectives; out[0..4] = min watermark, min epoch, rows
     * sent, rows received, bytes sent. Throws on every rank when one rank's round failed.
     */
    public static native void commRoundExchange(long comm, long[] out);

    /** fg_comm_round_end: the received partial rows merged into the global handle. */
    public static native void commRoundEnd(long comm, long global);

    /**
     * fg_comm_set_key_dicts: the subtask's key dictionaries (dictOpen handles; 0, 0 detaches). From
     * now on rounds and exchanges with KEYHASH_DICT_ID ship each partial row's key row and merge
     * under ids of globalDict. Every subtask of a job attaches, or none. The lock that covers
     * commRoundBegin / commRoundEnd must also cover the caller's own use of the two dictionaries.
     */
    public static native void commSetKeyDicts(long comm, long localDict, long globalDict);

    /** fg_comm_bytes_sent. */
    public static native long commBytesSent(long comm);

    /** fg_comm_close. */
    public static native void commClose(long comm);
}
