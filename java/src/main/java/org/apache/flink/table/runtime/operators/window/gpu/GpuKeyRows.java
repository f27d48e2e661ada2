/*
 * Grouping keys of a GPU window operator: one BIGINT key column as it is, any other key row
 * (BinaryRowDataKeySelector output, BinaryRowDataKeySelector.java:43-50 -- a STRING key, several
 * columns, a NULL key) through the engine's key dictionary (fg_key_dict: equal rows -> equal ids,
 * BinarySection.equals / hashCode, BinarySection.java:62-78).
 *
 * Per micro-batch the key rows are gathered into one direct buffer and interned by ONE
 * dictIntern call; per advance the fired rows' ids become key rows through ONE dictRows call:
 * the GPU gathers exactly those rows, packed in the ids' order, and only they cross to the host
 * (a second call when the reused buffer has to grow) -- never a JNI round trip per row, and no
 * copy of the arena range the ids span.
 *
 * The fused two-phase operator holds two of these: the local one (records -> ids of the local
 * handle) and a dictionary-only one for its global handle, whose ids the keyed RCCL edge hands out
 * (FlinkGpu.commSetKeyDicts); checkpoint chunks carry the packed key rows of their ids (packed) and
 * a restore interns them again (internPacked).
 */
package org.apache.flink.table.runtime.operators.window.gpu;

import org.apache.flink.core.memory.MemorySegment;
import org.apache.flink.core.memory.MemorySegmentFactory;
import org.apache.flink.table.data.RowData;
import org.apache.flink.table.data.binary.BinaryRowData;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

/** Key rows <-> 64-bit engine keys for one operator. */
final class GpuKeyRows implements AutoCloseable {
    private final boolean bigint;
    private final int arity;
    private final int batch;
    private long dict;
    private ByteBuffer rows, offsets, lengths;   // the current micro-batch's key rows
    private int n;
    private int bytes;
    private ByteBuffer outBytes, outOff, outLen; // dictRows scratch (reused, grown on demand)

    GpuKeyRows(GpuWindowAggSpec spec, int maxParallelism) {
        this(spec, maxParallelism, true);
    }

    /** batchBuffers false: the dictionary only (ids come from elsewhere; rows / packed / internPacked) */
    GpuKeyRows(GpuWindowAggSpec spec, int maxParallelism, boolean batchBuffers) {
        this.bigint = spec.bigintKey;
        this.arity = spec.keyArity;
        this.batch = spec.batchRecords;
        if (!bigint) {
            dict = FlinkGpu.dictOpen(spec.device, maxParallelism, spec.expectedKeys);
            if (batchBuffers) {
                rows = direct(64L * batch);
                offsets = direct(8L * batch);
                lengths = direct(4L * batch);
            }
        }
    }

    /** the fg_key_dict handle (0 for a BIGINT key) */
    long dict() {
        return dict;
    }

    static ByteBuffer direct(long bytes) {
        return ByteBuffer.allocateDirect((int) Math.max(bytes, 8)).order(ByteOrder.nativeOrder());
    }

    boolean bigint() {
        return bigint;
    }

    /** room for one more key row of `len` bytes in the batch's row buffer */
    boolean fits(RowData key) {
        return bigint || bytes + ((BinaryRowData) key).getSizeInBytes() <= rows.capacity();
    }

    /** record i of the micro-batch has key `key`: BIGINT into keys[i], else its row gathered */
    void add(RowData key, int i, ByteBuffer keys) {
        if (bigint) {
            keys.putLong(8 * i, key.getLong(0));
            return;
        }
        BinaryRowData row = (BinaryRowData) key;
        int len = row.getSizeInBytes();
        rows.position(bytes);
        MemorySegment[] segs = row.getSegments();
        if (segs.length == 1) {
            segs[0].get(row.getOffset(), rows, len);
        } else {   // (a key row spanning segments: copied through a heap array)
            byte[] b = new byte[len];
            org.apache.flink.table.data.binary.BinarySegmentUtils.copyToBytes(segs, row.getOffset(), b, 0, len);
            rows.put(b);
        }
        offsets.putLong(8 * n, bytes);
        lengths.putInt(4 * n, len);
        bytes += (len + 7) & ~7;
        n++;
    }

    /** the batch's key rows -> ids in keys[0 .. count) (one dictIntern) */
    void intern(int count, ByteBuffer keys) {
        if (bigint || count == 0) {
            return;
        }
        FlinkGpu.dictIntern(dict, rows, bytes, offsets, lengths, count, keys, null);
        n = 0;
        bytes = 0;
    }

    /**
     * The key selector on the GPU: count serialized records (whole BinaryRowData rows packed in rows[0 ..
     * nbytes), record i at recOffsets[i] with recLengths[i] bytes) -> their ids in keys[0 .. count) and the
     * projection's 8-byte columns (rowtime, value) in outCols / outColNull, by ONE dictInternFields call: the
     * GPU projects the key rows (what keySelector.getKey + add would build one record at a time) and interns
     * them. projection as FlinkGpu.dictProject takes it. Not for a BIGINT key (fg_add_rows reads those rows).
     */
    void internFields(
            ByteBuffer rows,
            long nbytes,
            ByteBuffer recOffsets,
            ByteBuffer recLengths,
            int count,
            long[] projection,
            ByteBuffer keys,
            ByteBuffer outCols,
            ByteBuffer outColNull) {
        if (bigint) {
            throw new IllegalStateException("internFields: a BIGINT key needs no dictionary");
        }
        if (count == 0) {
            return;
        }
        FlinkGpu.dictInternFields(dict, rows, nbytes, recOffsets, recLengths, count, projection, keys, null, outCols, outColNull);
    }

    /** the key rows of ids keys[0 .. count) (one dictRows into the reused buffers) */
    RowData[] rows(ByteBuffer keys, int count) {
        RowData[] out = new RowData[count];
        if (bigint) {
            // BinaryRowData of arity 1 (8-byte header + the long), as BinaryRowDataKeySelector
            // builds them: hashCode / equals -- and so key groups and state keys -- are the
            // selector's own (a GenericRowData would hash differently)
            MemorySegment seg = MemorySegmentFactory.wrap(new byte[16 * Math.max(count, 1)]);
            for (int i = 0; i < count; i++) {
                seg.putLong(16 * i + 8, keys.getLong(8 * i));
                BinaryRowData r = new BinaryRowData(1);
                r.pointTo(seg, 16 * i, 16);
                out[i] = r;
            }
            return out;
        }
        if (count == 0) {
            return out;
        }
        if (outOff == null || outOff.capacity() < 8L * (count + 1)) {
            outOff = direct(8L * (count + 1));
            outLen = direct(4L * count);
        }
        if (outBytes == null) {
            outBytes = direct(32L * count);
        }
        long nbytes = FlinkGpu.dictRows(dict, keys, count, outBytes, outBytes.capacity(), outOff, outLen);
        if (nbytes > outBytes.capacity()) {   // too small (nothing was written): grow, once
            if (nbytes > Integer.MAX_VALUE - 8) {
                throw new IllegalStateException(
                        "the key rows of one fired batch take " + nbytes + " bytes: more than a ByteBuffer holds");
            }
            outBytes = direct(Math.min(Math.max(nbytes, 2L * outBytes.capacity()), Integer.MAX_VALUE - 8));
            nbytes = FlinkGpu.dictRows(dict, keys, count, outBytes, outBytes.capacity(), outOff, outLen);
        }
        byte[] all = new byte[(int) nbytes];   // (the rows outlive the reused buffer)
        outBytes.position(0);
        outBytes.get(all);
        MemorySegment seg = MemorySegmentFactory.wrap(all);
        for (int i = 0; i < count; i++) {
            BinaryRowData r = new BinaryRowData(arity);
            r.pointTo(seg, (int) outOff.getLong(8 * i), outLen.getInt(4 * i));
            out[i] = r;
        }
        return out;
    }

    /**
     * the key rows of ids keys[0 .. count) as a checkpoint chunk stores them: count int32 lengths,
     * then the rows packed back to back, each zero-padded to 8 (one dictRows, a second if the
     * scratch has to grow)
     */
    byte[] packed(ByteBuffer keys, int count) {
        if (bigint || count == 0) {
            return new byte[0];
        }
        if (outOff == null || outOff.capacity() < 8L * (count + 1)) {
            outOff = direct(8L * (count + 1));
            outLen = direct(4L * count);
        }
        if (outBytes == null) {
            outBytes = direct(32L * count);
        }
        long nbytes = FlinkGpu.dictRows(dict, keys, count, outBytes, outBytes.capacity(), outOff, outLen);
        if (nbytes > outBytes.capacity()) {
            outBytes = direct(Math.min(Math.max(nbytes, 2L * outBytes.capacity()), Integer.MAX_VALUE - 8));
            nbytes = FlinkGpu.dictRows(dict, keys, count, outBytes, outBytes.capacity(), outOff, outLen);
        }
        byte[] out = new byte[4 * count + (int) nbytes];
        outLen.position(0);
        outLen.get(out, 0, 4 * count);
        outBytes.position(0);
        outBytes.get(out, 4 * count, (int) nbytes);
        return out;
    }

    /**
     * packed()'s layout back into ids: count key rows of lengths[0 .. count) (int32) packed back to
     * back in rows[0 .. nbytes), each padded to 8, interned into this dictionary; their ids go to
     * keys[0 .. count)
     */
    void internPacked(ByteBuffer rows, long nbytes, ByteBuffer lengths, int count, ByteBuffer keys) {
        if (bigint || count == 0) {
            return;
        }
        ByteBuffer off = direct(8L * count);
        long at = 0;
        for (int i = 0; i < count; i++) {
            off.putLong(8 * i, at);
            at += (lengths.getInt(4 * i) + 7) & ~7;
        }
        if (at != nbytes) {
            throw new IllegalStateException("a restored chunk's key rows take " + at + " bytes, it holds " + nbytes);
        }
        FlinkGpu.dictIntern(dict, rows, nbytes, off, lengths, count, keys, null);
    }

    /** the key rows of the given ids (a restore re-interns the image's rows first) */
    void internRows(byte[][] keyRows, ByteBuffer keys) {
        if (bigint) {
            return;
        }
        long total = 0;
        for (byte[] b : keyRows) {
            total += (b.length + 7) & ~7;
        }
        ByteBuffer all = direct(total);
        ByteBuffer off = direct(8L * keyRows.length);
        ByteBuffer len = direct(4L * keyRows.length);
        int at = 0;
        for (int i = 0; i < keyRows.length; i++) {
            all.position(at);
            all.put(keyRows[i]);
            off.putLong(8 * i, at);
            len.putInt(4 * i, keyRows[i].length);
            at += (keyRows[i].length + 7) & ~7;
        }
        FlinkGpu.dictIntern(dict, all, at, off, len, keyRows.length, keys, null);
    }

    /** the dictionary's live keys (fg_key_dict_stats.live); 0 for a BIGINT key */
    long liveKeys() {
        return bigint ? 0 : FlinkGpu.dictStats(dict)[0];
    }

    /**
     * keep exactly the ids keys[0 .. count) -- the key column of a full state image, every id the
     * operator holds -- and retire every other key of the dictionary (one dictRetain); a no-op for
     * a BIGINT key. Ids outside keys must not be used afterwards.
     */
    void retain(ByteBuffer keys, int count) {
        if (bigint) {
            return;
        }
        FlinkGpu.dictRetain(dict, keys, count);
    }

    @Override
    public void close() {
        if (dict != 0) {
            FlinkGpu.dictClose(dict);
            dict = 0;
        }
    }
}
