"""The fused two-phase subtask: local phase, keyBy edge and global phase in one operator, the edge
on a thread of its own (the Python mirror of java/.../gpu/GpuTwoPhaseWindowAggOperator.java).

The reference's two-phase plan (TwoStageOptimizedWindowAggregateRule.java:81-104) runs
LocalSlicingWindowAggOperator, a keyBy network edge (KeyGroupStreamPartitioner.selectChannel,
KeyGroupStreamPartitioner.java:55-65) and GlobalSlicingWindowAggOperator. On one node of GPUs the
edge is an RCCL all-to-all between the subtasks' GPUs (fg_comm), so one subtask holds the local and
the global operator of its GPU and the exchange is a collective every subtask must take part in --
the SAME number of times. Watermarks do not arrive in step at the subtasks (each source emits its
own), so the collective cannot be driven by them. Instead every subtask runs an edge thread that
exchanges in ROUNDS, forever, until every subtask has reached the end of its input:

  round (edge thread)     begin    [under the operator lock] the local operator's rows of the round --
                                   its uncollected async fires (FIRED), its whole buffer before a
                                   checkpoint barrier (FLUSHED), or nothing (IDLE) -- grouped by
                                   key-group owner, with this subtask's watermark and epoch
                          exchange [no lock: waits for the peers] one collective of (count, watermark,
                                   epoch, failure) per peer, then the rows
                          end      [under the lock] the received partial rows merged into the global
                                   operator (GlobalAggCombiner), the global advanced to the minimum
                                   watermark (StatusWatermarkValve) -- its fires are queued, and the
                                   task thread emits their rows (drain) before it forwards that
                                   watermark downstream

Checkpoints are aligned across the edge the way the reference aligns barriers on the global
operator's input channels: at its barrier a subtask flushes its local buffer into the next round
(LocalSlicingWindowAggOperator.prepareSnapshotPreBarrier :142-144) and advertises the checkpoint id as
its epoch; its task thread then waits until a round's minimum epoch reaches the id -- every subtask
has sent its pre-barrier rows -- and snapshots the global operator before the edge merges another
round. A subtask blocked at its barrier processes no post-barrier record, so no post-barrier row
reaches any image (the fast channels of an aligned checkpoint are blocked likewise).

Backends of a round: `CapiRounds` (fg_comm_round_begin / _exchange / _end, RCCL through the C-ABI) and
`TorchRounds` (torch.distributed: RCCL, or gloo through host memory for tests and rehearsals). The
subtask's operators are reached through a `pair` object (GpuPair for the HIP operators; tests plug
the oracle in the same way).

Keys of any type (STRING, composite, NULL): the operators aggregate ids of a key dictionary, and an
id of the sender's dictionary means nothing on the owner, so in a KEYED round every partial row
travels with its key row (as LocalAggCombiner ships the key BinaryRowData, LocalAggCombiner.java:
100-106) and the owner interns it into its own dictionary: `GpuPair(..., key_dicts=(local, owner))`
with `TorchRounds`, or `Communicator.set_key_dicts(local, owner)` with
`CapiRounds(comm, key_hash=KEYHASH_DICT_ID)`. The round is stateless: a failed one needs no repair.
"""
from __future__ import annotations

import ctypes as C
import threading
import time

import numpy as np

from . import _lib as L

JMIN, JMAX = -(1 << 63), (1 << 63) - 1
FIRED, FLUSHED, IDLE = L.ROUND_FIRED, L.ROUND_FLUSHED, L.ROUND_IDLE


class RoundFailed(RuntimeError):
    """a round failed on some subtask: every subtask's edge stops with this error"""


class Round:
    __slots__ = ("min_watermark", "min_epoch", "rows_sent", "rows_received", "bytes_sent")

    def __init__(self, min_watermark, min_epoch, rows_sent, rows_received, bytes_sent):
        self.min_watermark, self.min_epoch = int(min_watermark), int(min_epoch)
        self.rows_sent, self.rows_received, self.bytes_sent = int(rows_sent), int(rows_received), int(bytes_sent)


class GpuPair:
    """The HIP local (FG_FLAG_LOCAL_PARTIALS) and global operators of one subtask."""

    def __init__(self, local, glob, device=None, key_dicts=None):
        """key_dicts = (local, owner) KeyDictionary pair when the grouping keys are dictionary ids:
        the local operator's keys are ids of `local`, the global operator's ids of `owner`."""
        import torch
        self.local, self.glob = local, glob
        self.device = device if device is not None else torch.device("cuda", 0)
        self.key_dicts = key_dicts

    def local_batch(self, key, ts, val):
        """with key dictionaries `key` may be the records' packed key rows (bytes u8, offsets i64,
        lengths i32 device tensors): they are interned into the local dictionary here, under the
        subtask's lock -- the edge thread's rounds use the same dictionary"""
        if self.key_dicts is not None and isinstance(key, tuple):
            key = self.key_dicts[0].intern_rows(*key)
        self.local.process_batch(key, ts, val)

    def local_watermark(self, wm: int):
        self.local.process_watermarks([int(wm)])

    def local_rows(self, mode, world, max_parallelism, key_hash):
        """the round's local partial rows grouped by owner: (int64 device columns, counts[world]);
        with key dictionaries a third value, the grouped rows' key rows (key_lengths int32[n],
        key_bytes uint8[], byte_counts[world]) of fg_partition_keyed_by_owner (None when idle)"""
        import torch

        from .exchange import device_columns, partition_columns_by_owner, partition_keyed_by_owner
        keyed = self.key_dicts is not None
        if mode == IDLE:
            none = (None, torch.zeros(world, dtype=torch.int64))
            return none + (None,) if keyed else none
        r = self.local.collect_fired() if mode == FIRED else self.local.flush_partials(device_output=True)
        cols = device_columns(r, aggs=tuple(range(int(r.num_aggs))), device=self.device)
        if keyed:
            kd = self.key_dicts[0]
            if max_parallelism != kd.max_parallelism:
                raise ValueError(f"max_parallelism {max_parallelism} is not the key dictionaries' {kd.max_parallelism}")
            # (complete on return: the local operator may fire again, the dictionary intern again)
            outs, counts, klen, kbytes, bcounts = partition_keyed_by_owner(cols, kd, world)
            return outs, counts, (klen, kbytes, bcounts)
        outs, counts = partition_columns_by_owner(cols, world, max_parallelism, key_hash)
        torch.cuda.current_stream(self.device).synchronize()   # (the local's rows are read: it may fire again)
        return outs, counts

    def global_add(self, cols, key_rows=None):
        """the received partial rows merged into the global operator; key_rows = (lengths int32[n],
        bytes uint8[]) of a keyed round: the rows' key rows, packed back to back and padded to 8,
        interned into the owner dictionary -- their ids are the key column of the merge"""
        if cols is None or not cols[0].numel():
            return
        if self.key_dicts is not None:
            import torch
            if key_rows is None:
                raise RoundFailed("rows without their key rows reached a subtask with key dictionaries")
            ln, data = key_rows
            padded = (ln.to(torch.int64) + 7) & ~7
            off = torch.cumsum(padded, 0) - padded
            if int(padded.sum()) != data.numel() or bool(((ln < 0) | (ln % 4 != 0)).any()):
                raise RoundFailed("the key rows received do not match their lengths")
            if data.numel() == 0:   # (only empty rows: the intern still wants a buffer to point at)
                data = data.new_zeros(8)
            cols = [self.key_dicts[1].intern_rows(data, off, ln)] + list(cols[1:])
        self.glob.process_partials(*cols)

    def global_advance(self, wm: int):
        self.glob.process_watermark(int(wm), device_output=True, wait=False)
        self._pending = True

    _pending = False

    def global_collect(self):
        """the rows of the global fires queued since the last collect (host), or None"""
        if not self._pending:
            return None
        self._pending = False
        return self.glob.collect_fired(host=True)

    def global_snapshot(self):
        """(image, timer watermark); with key dictionaries a third value, the image's key rows
        (image_key_rows: the owner ids mean nothing to a restarted subtask's dictionary)"""
        self.glob.prepare_snapshot_pre_barrier()
        image, twm = self.glob.snapshot_state(copy=True)
        if self.key_dicts is None:
            return image, twm
        return image, twm, image_key_rows(image, self.key_dicts[1])


class TorchRounds:
    """A round over torch.distributed (fg_comm_round semantics): ONE all-to-all of (count,
    watermark, epoch, columns << 1 | failed, key bytes, keyed) per peer, one host read, ONE
    all-to-all of the rows packed [n, c]. via_cpu stages through host memory (gloo).

    A pair with key dictionaries (pair.key_dicts) makes the round keyed, as fg_comm_set_key_dicts
    does on the C side: the rows' key row lengths travel as one more column, their bytes in one more
    all-to-all (per-peer runs, sized by the meta's key bytes), and the owner interns them
    (pair.global_add). Every subtask sees every peer's keyed flag, so all decide alike; subtasks
    that disagree fail the round together."""

    def __init__(self, group=None, via_cpu=False, max_parallelism=128, key_hash=L.KEYHASH_BINARYROW_BIGINT):
        import torch.distributed as dist
        self.group, self.via_cpu = group, via_cpu
        self.maxp, self.key_hash = max_parallelism, key_hash
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self._out = None
        self._recv = None
        self._kbytes = None
        self._recv_keys = None
        self.bytes_sent = 0

    def begin(self, pair, mode, watermark, epoch):
        import torch
        self._err = None
        keyed = getattr(pair, "key_dicts", None) is not None
        krows = None
        try:
            res = pair.local_rows(mode, self.world, self.maxp, L.KEYHASH_DICT_ID if keyed else self.key_hash)
            outs, counts = res[0], res[1]
            if keyed and outs:
                klen, self._kbytes, bcounts = krows = res[2]
                outs = list(outs) + [klen.to(torch.int64)]
        except Exception as e:   # (still takes part in the round: the peers learn of it)
            self._err = e
            outs, counts = None, torch.zeros(self.world, dtype=torch.int64)
        ncols = len(outs) if outs else 0
        n = int(outs[0].numel()) if outs else 0
        if outs and int(counts.sum()) != n:
            self._err, outs, counts = RoundFailed("owner partition lost rows"), None, torch.zeros(self.world, dtype=torch.int64)
        fail = 1 if self._err is not None else 0
        meta = torch.zeros((self.world, 6), dtype=torch.int64)
        meta[:, 0] = counts.cpu() if not fail else 0
        meta[:, 1] = int(watermark)
        meta[:, 2] = int(epoch)
        meta[:, 3] = ncols << 1 | fail
        if krows is not None and not fail and outs:
            meta[:, 4] = krows[2].cpu()
        meta[:, 5] = 1 if keyed else 0   # (the same word to every peer)
        if fail or not outs:
            self._kbytes = None
        self._meta = meta if self.via_cpu else meta.to(counts.device)
        self._out = None if fail or not outs else torch.stack(outs, dim=1).contiguous()

    def exchange(self) -> Round:
        import torch
        import torch.distributed as dist
        rmeta = torch.empty_like(self._meta)
        dist.all_to_all_single(rmeta, self._meta, group=self.group)
        ms, mr = self._meta.cpu(), rmeta.cpu()
        failed = [p for p in range(self.world) if int(mr[p, 3]) & 1]
        if failed:
            if self._err is not None:
                raise RoundFailed(f"this subtask's round failed: {self._err!r}")
            raise RoundFailed(f"subtask {failed[0]} failed its round (no rows moved on any subtask)")
        cols = {int(mr[p, 3]) >> 1 for p in range(self.world) if int(mr[p, 0]) > 0}
        if len(cols) > 1:
            raise RoundFailed("subtasks sent rows of different column counts")
        if len({int(mr[p, 5]) for p in range(self.world)}) > 1:
            raise RoundFailed("subtasks disagree about shipping key rows (key dictionaries on all, or on none)")
        keyed = bool(int(mr[0, 5]))
        send, recv = ms[:, 0].tolist(), mr[:, 0].tolist()
        nc = cols.pop() if cols else 0
        self._recv = None
        if nc:
            packed = self._out if self._out is not None else torch.zeros((0, nc), dtype=torch.int64)
            if self.via_cpu:
                packed = packed.cpu()
            elif self._out is None:
                packed = packed.to(self._meta.device)
            out = torch.empty((sum(recv), nc), dtype=torch.int64, device=packed.device)
            dist.all_to_all_single(out, packed, output_split_sizes=recv, input_split_sizes=send, group=self.group)
            self._recv = out
        sent = 8 * nc * (sum(send) - send[self.rank])
        self._recv_keys = None
        if keyed and nc:
            # the key bytes (padded to 8: whole words) as per-peer runs, in the rows' order
            ksend, krecv = (ms[:, 4] // 8).tolist(), (mr[:, 4] // 8).tolist()
            kb = self._kbytes if self._kbytes is not None else torch.zeros(0, dtype=torch.uint8)
            if self.via_cpu:
                kb = kb.cpu()
            elif self._kbytes is None:
                kb = kb.to(self._meta.device)
            words = kb.contiguous().view(torch.int64) if kb.numel() else torch.zeros(0, dtype=torch.int64, device=kb.device)
            rwords = torch.empty(sum(krecv), dtype=torch.int64, device=words.device)
            dist.all_to_all_single(rwords, words, output_split_sizes=krecv, input_split_sizes=ksend, group=self.group)
            self._recv_keys = rwords.view(torch.uint8) if rwords.numel() else torch.zeros(0, dtype=torch.uint8, device=rwords.device)
            sent += 8 * (sum(ksend) - ksend[self.rank])
        self.bytes_sent += sent
        return Round(int(mr[:, 1].min()), int(mr[:, 2].min()), sum(send), sum(recv), sent)

    def end(self, pair, device=None):
        import torch
        if self._recv is None or self._recv.shape[0] == 0:
            return
        r = self._recv
        if device is not None and r.device != device:
            r = r.to(device)
        cols = [c.contiguous() for c in r.unbind(1)]
        if self._recv_keys is None:
            pair.global_add(cols)
            return
        kb = self._recv_keys
        if device is not None and kb.device != device:
            kb = kb.to(device)
        pair.global_add(cols[:-1], (cols[-1].to(torch.int32), kb))


class CapiRounds:
    """A round through the C-ABI (fg_comm_round_begin / _exchange / _end over RCCL): the pair's
    operators are HIP handles (GpuPair). Keyed simply by key_hash=KEYHASH_DICT_ID after
    comm.set_key_dicts(local, owner): the library ships and interns the key rows itself."""

    def __init__(self, comm, max_parallelism=128, key_hash=L.KEYHASH_BINARYROW_BIGINT):
        self.comm, self.maxp, self.key_hash = comm, max_parallelism, key_hash
        self._lib = L.load()

    @property
    def bytes_sent(self):
        return self.comm.bytes_sent

    def begin(self, pair, mode, watermark, epoch):
        h = None if mode == IDLE else pair.local._h
        # (its failure is reported by exchange, on every rank)
        self._rc = self._lib.fg_comm_round_begin(self.comm._h, h, mode, self.key_hash, self.maxp, int(watermark),
                                                 int(epoch))

    def exchange(self) -> Round:
        r = L.FgRound()
        rc = self._lib.fg_comm_round_exchange(self.comm._h, C.byref(r))
        if rc:
            raise RoundFailed(self._lib.fg_comm_last_error(self.comm._h).decode(errors="replace"))
        return Round(r.min_watermark, r.min_epoch, r.rows_sent, r.rows_received, r.bytes_sent)

    def end(self, pair, device=None):
        rc = self._lib.fg_comm_round_end(self.comm._h, pair.glob._h)
        if rc:
            raise RoundFailed(self._lib.fg_comm_last_error(self.comm._h).decode(errors="replace"))


class TwoPhaseSubtask:
    """One subtask of the fused operator: the task thread's calls (records, watermarks, barriers,
    end of input, drain) and the edge thread's rounds, under one lock."""

    def __init__(self, pair, rounds, idle_sleep_s: float = 0.001, device=None):
        self.pair, self.rounds = pair, rounds
        self.idle_sleep_s, self.device = idle_sleep_s, device
        self.cv = threading.Condition()
        self.wm_local = JMIN       # the last watermark handed to the local operator
        self.dirty = False         # local fires since the last round
        self.flush_req = 0         # checkpoint id whose pre-barrier flush is requested
        self.sent_epoch = 0        # ... and the last one sent
        self.aligned = 0           # the last epoch every subtask has sent (a round's minimum)
        self.snap_done = 0         # the last aligned epoch this subtask has snapshotted
        self.glob_wm = JMIN        # the global operator's (combined) watermark
        self.forwarded = JMIN      # the watermark drain() last forwarded
        self.error = None
        self.rounds_run = 0
        self.output = []           # ("rows", numpy rows) and ("watermark", wm) in emission order
        self._thread = threading.Thread(target=self._edge, name="fg-edge", daemon=True)
        self._thread.start()

    # -- the task thread ---------------------------------------------------------------------------
    def _check(self):
        if self.error is not None:
            raise self.error

    def process_batch(self, key, ts, val):
        with self.cv:
            self._check()
            self.pair.local_batch(key, ts, val)

    def process_watermark(self, wm: int):
        with self.cv:
            self._check()
            if wm <= self.wm_local:
                return
            self.pair.local_watermark(wm)
            self.wm_local = int(wm)
            self.dirty = True

    def drain(self):
        """the mailbox action the edge posts: the global fires' rows emitted, then the combined
        watermark forwarded (rows always precede the watermark that fired them)"""
        with self.cv:
            self._check()
            self._drain_locked()

    def _drain_locked(self):
        rows = self.pair.global_collect()
        if rows is not None and len(rows):
            self.output.append(("rows", rows))
        if self.glob_wm > self.forwarded:
            self.forwarded = self.glob_wm
            self.output.append(("watermark", self.glob_wm))

    def prepare_snapshot_pre_barrier(self, checkpoint_id: int, timeout_s: float = 300.0):
        """the barrier of checkpoint `checkpoint_id` (ids increase): the local buffer goes out with
        the next round; once every subtask has sent its pre-barrier rows the global operator's rows
        are emitted and its image taken; returns (image, timer watermark)"""
        with self.cv:
            self._check()
            self.flush_req = int(checkpoint_id)
            self.cv.notify_all()
            if not self.cv.wait_for(lambda: self.aligned >= checkpoint_id or self.error is not None, timeout_s):
                raise TimeoutError(f"checkpoint {checkpoint_id} not aligned in {timeout_s} s")
            self._check()
            self._drain_locked()
            image = self.pair.global_snapshot()
            self.snap_done = int(checkpoint_id)
            self.cv.notify_all()
            return image

    def end_input(self, timeout_s: float = 300.0):
        """Long.MAX_VALUE: the edge runs until every subtask has ended; the last rows drained"""
        self.process_watermark(JMAX)
        self._thread.join(timeout_s)
        if self._thread.is_alive():
            raise TimeoutError("the edge did not finish")
        with self.cv:
            self._check()
            self._drain_locked()

    def close(self):
        with self.cv:
            if self.error is None and self._thread.is_alive():
                self.error = RuntimeError("closed")
            self.cv.notify_all()

    # -- the edge thread -----------------------------------------------------------------------------
    def _edge(self):
        try:
            while True:
                with self.cv:
                    if self.dirty:   # (fires before a flush: a barrier's flush follows in the next round)
                        mode, epoch = FIRED, self.sent_epoch
                    elif self.flush_req > self.sent_epoch:
                        mode, epoch = FLUSHED, self.flush_req
                    else:
                        mode, epoch = IDLE, self.sent_epoch
                    self.dirty = False
                    wm = self.wm_local
                    self.rounds.begin(self.pair, mode, wm, epoch)
                    if mode == FLUSHED:
                        self.sent_epoch = epoch
                r = self.rounds.exchange()   # (no lock: the task thread goes on meanwhile)
                with self.cv:
                    self.rounds_run += 1
                    self.rounds.end(self.pair, self.device)
                    if r.min_watermark > self.glob_wm:
                        self.pair.global_advance(r.min_watermark)
                        self.glob_wm = r.min_watermark
                    if r.min_epoch > self.aligned:
                        # every subtask has sent its pre-barrier rows: this subtask snapshots before
                        # another round merges (its task thread waits at the barrier)
                        self.aligned = r.min_epoch
                        self.cv.notify_all()
                        self.cv.wait_for(lambda: self.snap_done >= self.aligned or self.error is not None)
                        if self.error is not None:
                            return
                if r.min_watermark == JMAX:
                    return   # (every subtask has ended: the same round on all of them)
                if mode == IDLE and r.rows_received == 0:
                    time.sleep(self.idle_sleep_s)
        except BaseException as e:   # noqa: BLE001 (the task thread re-raises it)
            with self.cv:
                self.error = e if isinstance(e, Exception) else RuntimeError(repr(e))
                self.cv.notify_all()


def union_image_for(images, key_group_range, max_parallelism=128, key_groups=None):
    """Restore after a failover (or a rescale): the fused operator is not keyed, so its global
    images are union operator state -- every subtask reads all of them and keeps the entries of its
    own key groups (KeyGroupRangeAssignment). `key_groups(keys)` -> key groups (default: the device
    hash of BIGINT keys)."""
    cat = {c: np.concatenate([np.asarray(im[c]) for im, _ in images]) for c in images[0][0]}
    if key_groups is None:
        from .window_agg import key_groups as kg_dev
        kg = kg_dev(cat["key"], max_parallelism)
    else:
        kg = key_groups(cat["key"])
    lo, hi = key_group_range
    keep = (kg >= lo) & (kg <= hi)
    twm = min(w for _, w in images)
    return {c: v[keep] for c, v in cat.items()}, twm


def restore_union(glob, images, key_hash=None):
    """union_image_for followed by restore_state, with the key-group filter on the GPU: the global
    operator `glob` (a WindowAggOperator opened with this subtask's key_group_range) takes the
    (image, timer watermark) pairs of every subtask's global image as they are and keeps the
    entries of its own key groups (fg_restore_range). Returns the restore's info dict."""
    from . import _lib as L
    return glob.restore_state_range(images, None, L.KEYHASH_BINARYROW_BIGINT if key_hash is None else key_hash)


def image_key_rows(image, owner_dict):
    """At a checkpoint: the key rows of a global image whose key column holds ids of `owner_dict`
    (KeyDictionary.rows: bytes, offsets[n + 1], lengths) -- stored with the image, since the ids
    mean nothing to the dictionary of a restarted subtask."""
    return owner_dict.rows(np.ascontiguousarray(image["key"], dtype=np.int64))


def restore_union_dict_ids(glob, sources, owner_dict):
    """restore_union for images keyed by dictionary ids: sources = [(image, timer watermark, key
    rows), ...] of every old subtask, the key rows as image_key_rows took them. Each image's key
    rows are interned into `owner_dict` (the restarted subtask's fresh owner dictionary), the ids
    it hands out replace the key column, and `glob` keeps the entries of its own key groups
    (restore_state_range with KEYHASH_DICT_ID: an id carries its key row's key group, the same in
    every dictionary). Returns the restore's info dict."""
    from . import _lib as L
    images = []
    for img, wm, (buf, off, ln) in sources:
        if len(buf) == 0:   # (only empty rows, or none: the intern still wants a buffer to point at)
            buf = np.zeros(8, dtype=np.uint8)
        ids, _ = owner_dict.intern(packed=(buf, off[:-1], ln), key_groups=False)
        images.append((dict(img, key=ids), wm))
    return glob.restore_state_range(images, None, L.KEYHASH_DICT_ID)


def keyed_runs(image, index, key_group_range):
    """The rows of a key-grouped image (WindowAggOperator.set_snapshot_grouping) whose key group
    lies in key_group_range = (lo, hi): one contiguous run of rows per slice, found from `index`
    (snapshot_key_groups) alone -- no key group is computed here, and no row outside the range is
    touched (KeyGroupRangeOffsets: a restore reads the ranges it owns). Returns the non-empty runs
    as image dicts of views into `image` (nothing is copied)."""
    maxp, first = int(index["max_parallelism"]), index["first_row"]
    lo, hi = max(int(key_group_range[0]), 0), min(int(key_group_range[1]), maxp - 1)
    if lo > hi:
        return []
    runs = [(int(first[s * maxp + lo]), int(first[s * maxp + hi + 1])) for s in range(int(index["n_slices"]))]
    return [{c: v[a:b] for c, v in image.items()} for a, b in runs if b > a]


def keyed_part(image, index, key_group_range):
    """keyed_runs as one image dict: the rows of the range, slice by slice (a copy when the range
    has rows in several slices)."""
    runs = keyed_runs(image, index, key_group_range)
    if len(runs) == 1:
        return runs[0]
    return {c: (np.concatenate([r[c] for r in runs]) if runs else v[:0]) for c, v in image.items()}


def restore_keyed(glob, sources):
    """restore_union for key-grouped images: sources = [(image, timer watermark, index), ...] of
    every old subtask. The global operator `glob` takes, out of every image, only the runs of its
    own key-group range (keyed_runs; they are handed over as they lie, one image per run) and
    restores them with the minimum watermark (restore_state_range: rows_in == rows_kept when the
    images were grouped with its hash). Returns the restore's info dict."""
    rng = (glob.cfg.key_group_start, glob.cfg.key_group_end)
    parts = [run for img, _, idx in sources for run in keyed_runs(img, idx, rng)]
    return glob.restore_state_range(parts, min(int(wm) for _, wm, _ in sources))
