"""The keyed two-phase edge on the HIP engine: STRING keys cross the edge as key rows.

The operators aggregate ids of GPU key dictionaries; an id of the sender's dictionary means
nothing on the owner, so every partial row travels with its key row and the owner interns it.
The owner dictionaries are pre-warmed in another first-seen order than the local ones, so ids
passed through as they are would name other keys and the rows would differ from the oracle's.

1. the C-ABI (fg_comm_round_* after fg_comm_set_key_dicts, RCCL at world size 1) under the fused
   subtask, 5- and 7-column rows, one checkpoint; and the one-call form on the same data;
2. a keyed begin that fails (an async intern pending on the local dictionary) ends the round;
3. two processes over gloo with real dictionaries of different orders;
4. the same with a checkpoint, a failover into fresh dictionaries and a replay: exactly once.

No record is late (jitter < delay), so the rows do not depend on the rounds' timing and the
reference is the single-phase oracle over the whole input, keyed by the key index.
"""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAXP = 128
DELAY, JITTER = 400, 300
CHILD_WAIT_S = 240
KINDS = {"tumble": ("tumble", 1000, 0, ("count_star", "count", "sum", "avg")),
         "cumulate": ("cumulate", 4000, 1000, ("count_star", "sum", "min", "max"))}
# world size 1 over the C-ABI / two ranks over gloo
N1, KEYS1, BATCH1, RATE1 = 60_000, 4_000, 10_000, 10
N2, KEYS2, BATCH2, RATE2, WORLD, CKPT_AFTER = 100_000, 8_000, 20_000, 20, 2, 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _stream(n, keys, rate, seed):
    from tests.streams import make_stream
    return make_stream(n, keys, "f64", seed=seed, jitter_ms=JITTER, rate_per_ms=rate)[:3]


def _packed(key, dev):
    """the records' 32-B STRING key rows (bench.string_key_rows) packed for the intern, on the device"""
    import torch

    import bench
    k = torch.as_tensor(key).to(dev)
    rows = bench.string_key_rows(k).view(torch.uint8).reshape(-1)
    n = k.numel()
    return rows, torch.arange(n, dtype=torch.int64, device=dev) * 32, torch.full((n,), 32, dtype=torch.int32, device=dev)


def _warm(d, order, dev):
    """first-seen order of a dictionary: the keys of `order` interned one batch after the other"""
    import torch
    d.intern(packed=_packed(torch.from_numpy(np.ascontiguousarray(order, dtype=np.int64)), dev), key_groups=False)


def _decode(rows, ko, nkeys):
    """the fired rows with their owner ids replaced by the key index their key row spells"""
    import torch

    import bench
    names = bench.string_key_rows(torch.arange(nkeys, dtype=torch.int64)).numpy().view(np.uint8).reshape(nkeys, 32)
    index = {names[i].tobytes(): i for i in range(nkeys)}
    ids, inv = np.unique(rows["key"], return_inverse=True)
    uniq = ko.lookup(ids)
    out = rows.copy()
    out["key"] = np.array([index[r] for r in uniq], dtype=np.int64)[inv]
    return out, uniq


def _window(F, kind):
    k_, size, slide, aggs = KINDS[kind]
    return (F.tumbling(size) if k_ == "tumble" else F.cumulative(size, slide)), aggs


def _pack(r):
    return None if r is None else (r.tobytes(), r.dtype.descr)


def _unpack(p):
    b, descr = p
    return np.frombuffer(b, dtype=np.dtype([tuple(x) for x in descr]))


def _oracle(O, kind, streams):
    k_, size, slide, _ = KINDS[kind]
    op = O.OracleOperator(kind={"tumble": O.TUMBLE, "cumulate": O.CUMULATE}[k_], size=size, slide=slide,
                          val_type=O.VAL_F64)
    for k, t, v in streams:
        op.process_batch(k, t, v)
    op.process_watermark((1 << 63) - 1)
    e = op.take_rows()
    assert op.late_dropped == 0
    op.close()
    return e


def _compare(g, e, kind):
    g = g[np.lexsort((g["key"], g["window_end"]))]
    e = e[np.lexsort((e["key"], e["window_end"]))]
    assert len(g) == len(e) > 0, (len(g), len(e))
    aggs = KINDS[kind][3]
    exact = [("key", "key"), ("window_start", "window_start"), ("window_end", "window_end"), ("count_star", "cnt_star")]
    exact += [("count", "cnt_val")] if "count" in aggs else []
    exact += [("min", "min_d"), ("max", "max_d")] if "min" in aggs else []
    for f, fe in exact:
        assert np.array_equal(g[f], e[fe]), f
    for f, fe in [("sum", "sum_d")] + ([("avg", "avg_d")] if "avg" in aggs else []):
        a, b = g[f], e[fe]   # DOUBLE sums: the project's 1e-9 relative
        assert (np.abs(a - b) <= 1e-9 * np.maximum(np.abs(a), np.abs(b))).all(), f


def _spawn(target, nproc, *args):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r,) + args + (q,)) for r in range(nproc)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(nproc):
            res.append(q.get(timeout=CHILD_WAIT_S))
            assert not res[-1][-1], res[-1][-1]
    finally:
        for p in procs:
            p.join(timeout=5 if len(res) < nproc else 60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return sorted(res, key=lambda r: r[0])


# ---- 1. the C-ABI at world size 1 ------------------------------------------------------------------

def _capi_child(rank, q):
    try:
        import torch

        import flink_amd as F
        from flink_amd import _lib as L
        from flink_amd.comm import Communicator, unique_id
        from flink_amd.keys import KeyDictionary
        from flink_amd.two_phase import CapiRounds, GpuPair, TwoPhaseSubtask
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        comm = Communicator(0, 1, 0, unique_id())
        key, ts, val = _stream(N1, KEYS1, RATE1, 8100)
        out = {}
        for kind in ("tumble", "cumulate"):
            kd, ko = KeyDictionary(MAXP, KEYS1), KeyDictionary(MAXP, KEYS1)
            _warm(ko, np.arange(KEYS1)[::-1], dev)   # the owner's first-seen order is not the sender's
            comm.set_key_dicts(kd, ko)
            w, aggs = _window(F, kind)
            local = F.WindowAggOperator(w, aggs=aggs, expected_keys=KEYS1, local_partials=True)
            glob = F.WindowAggOperator(w, aggs=aggs, expected_keys=KEYS1)
            sub = TwoPhaseSubtask(GpuPair(local, glob, dev, key_dicts=(kd, ko)),
                                  CapiRounds(comm, MAXP, key_hash=L.KEYHASH_DICT_ID), device=dev)
            mx, snap = -(1 << 63), None
            for bi, lo in enumerate(range(0, N1, BATCH1)):
                hi = lo + BATCH1
                sub.process_batch(_packed(key[lo:hi], dev), torch.from_numpy(ts[lo:hi]).to(dev),
                                  torch.from_numpy(val[lo:hi]).to(dev))
                mx = max(mx, int(ts[lo:hi].max()))
                sub.process_watermark(mx - DELAY - 1)
                sub.drain()
                if bi == 1:
                    snap = sub.prepare_snapshot_pre_barrier(1)
            sub.end_input()
            image, _, (kbytes, koff, klen) = snap
            assert len(image["key"]) > 0 and len(klen) == len(image["key"]) and (klen == 32).all()
            assert sub.rounds_run > 2 and comm.bytes_sent == 0   # (world size 1: nothing leaves the rank)
            assert len(kd) == len(ko) == KEYS1 and not torch.equal(
                kd.intern(packed=_packed(np.arange(64), dev), key_groups=False)[0],
                ko.intern(packed=_packed(np.arange(64), dev), key_groups=False)[0])
            rows, _ = _decode(np.concatenate([r for k, r in sub.output if k == "rows"]), ko, KEYS1)
            out[kind] = _pack(rows)
            if kind == "tumble":
                # the one-call form on the same data, fresh operators and dictionaries
                kd2, ko2 = KeyDictionary(MAXP, KEYS1), KeyDictionary(MAXP, KEYS1)
                _warm(ko2, np.arange(KEYS1)[::-1], dev)
                comm.set_key_dicts(kd2, ko2)
                l2 = F.WindowAggOperator(w, aggs=aggs, expected_keys=KEYS1, local_partials=True)
                g2 = F.WindowAggOperator(w, aggs=aggs, expected_keys=KEYS1)
                got, mx = [], -(1 << 63)
                for lo in range(0, N1, BATCH1):
                    hi = lo + BATCH1
                    ids = kd2.intern_rows(*_packed(key[lo:hi], dev))
                    l2.process_batch(ids, torch.from_numpy(ts[lo:hi]).to(dev), torch.from_numpy(val[lo:hi]).to(dev))
                    mx = max(mx, int(ts[lo:hi].max()))
                    for wm in (mx - DELAY - 1,) + (((1 << 63) - 1,) if hi == N1 else ()):
                        l2.process_watermarks([wm])
                        gwm = comm.exchange_fired(l2, g2, wm, key_hash=L.KEYHASH_DICT_ID, max_parallelism=MAXP)
                        assert gwm == wm
                        got.append(g2.process_watermark(gwm))
                rows2, _ = _decode(np.concatenate([r for r in got if len(r)]), ko2, KEYS1)
                out["one_call"] = _pack(rows2)
                for op in (l2, g2):
                    op.close()
                comm.set_key_dicts(None, None)
                kd2.close()
                ko2.close()
            comm.set_key_dicts(None, None)
            for x in (local, glob, kd, ko):
                x.close()
        comm.close()
        q.put((rank, out, None))
    except Exception as e:   # reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc() + repr(e)))


def test_capi_keyed_rounds_world1_match_the_oracle(oracle_mod):
    (_, out, _), = _spawn(_capi_child, 1)
    streams = [_stream(N1, KEYS1, RATE1, 8100)]
    for kind in ("tumble", "cumulate"):
        _compare(_unpack(out[kind]), _oracle(oracle_mod, kind, streams), kind)
    _compare(_unpack(out["one_call"]), _oracle(oracle_mod, "tumble", streams), "tumble")


# ---- 2. a failed keyed begin ---------------------------------------------------------------------------

def _failed_begin_child(rank, q):
    try:
        import torch

        import flink_amd as F
        from flink_amd import _lib as L
        from flink_amd.comm import Communicator, unique_id
        from flink_amd.keys import KeyDictionary
        from flink_amd.two_phase import FIRED, CapiRounds, GpuPair, RoundFailed
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        comm = Communicator(0, 1, 0, unique_id())
        kd, ko = KeyDictionary(MAXP, 1000), KeyDictionary(MAXP, 1000)
        comm.set_key_dicts(kd, ko)
        w, aggs = _window(F, "tumble")
        local = F.WindowAggOperator(w, aggs=aggs, expected_keys=1000, local_partials=True)
        glob = F.WindowAggOperator(w, aggs=aggs, expected_keys=1000)
        pair, rounds = GpuPair(local, glob, dev, key_dicts=(kd, ko)), CapiRounds(comm, MAXP, key_hash=L.KEYHASH_DICT_ID)
        key, ts, val = _stream(4000, 1000, 1, 8200)

        def feed(lo, hi):
            pair.local_batch(_packed(key[lo:hi], dev), torch.from_numpy(ts[lo:hi]).to(dev),
                             torch.from_numpy(val[lo:hi]).to(dev))
            pair.local_watermark(int(ts[lo:hi].max()) - DELAY - 1)
            return int(ts[lo:hi].max()) - DELAY - 1

        wm = feed(0, 2000)
        pending = _packed(key[2000:2100], dev)
        kd.intern_async(pending)                 # the local dictionary is busy: the keyed begin fails
        rounds.begin(pair, FIRED, wm, 0)
        try:
            rounds.exchange()
            raise AssertionError("the round did not fail")
        except RoundFailed as e:
            assert "async intern is pending" in str(e), str(e)
        glob.prepare_snapshot_pre_barrier()
        assert len(glob.snapshot_state()[0]["key"]) == 0 and len(ko) == 0   # nothing reached the global side
        kd.intern_wait()
        assert len(kd.lookup(kd.intern(packed=_packed(key[:8], dev), key_groups=False)[0].cpu().numpy())) == 8
        wm = feed(2000, 4000)                    # the dictionary and the edge are usable: a round goes through
        rounds.begin(pair, FIRED, wm, 0)
        r = rounds.exchange()
        rounds.end(pair, dev)
        assert r.rows_received == r.rows_sent > 0 and len(ko) > 0
        glob.prepare_snapshot_pre_barrier()
        assert 0 < len(glob.snapshot_state()[0]["key"]) <= r.rows_received
        comm.set_key_dicts(None, None)
        for x in (local, glob, kd, ko, comm):
            x.close()
        q.put((rank, None, None))
    except Exception as e:   # reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc() + repr(e)))


def test_a_failed_keyed_begin_ends_the_round_cleanly():
    _spawn(_failed_begin_child, 1)


# ---- 3. and 4. two processes over gloo, real dictionaries ----------------------------------------------

def _gloo_rank(rank, port, ckpt, q):
    import faulthandler
    import sys
    faulthandler.enable(file=sys.stderr)
    faulthandler.dump_traceback_later(CHILD_WAIT_S - 20, exit=True, file=sys.stderr)
    try:
        import datetime

        import torch
        import torch.distributed as dist

        import flink_amd as F
        from flink_amd import _lib as L
        from flink_amd.keys import KeyDictionary
        from flink_amd.two_phase import GpuPair, TorchRounds, TwoPhaseSubtask, restore_union_dict_ids
        from oracle import oracle as O
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=120))
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        w, aggs = _window(F, "tumble")
        kg = ((rank * MAXP + WORLD - 1) // WORLD, ((rank + 1) * MAXP - 1) // WORLD)
        key, ts, val = _stream(N2, KEYS2, RATE2, 8300 + rank)
        perm = np.random.default_rng(40 + rank).permutation(KEYS2)   # the ranks' dictionary orders differ

        def subtask():
            kd, ko = KeyDictionary(MAXP, KEYS2), KeyDictionary(MAXP, KEYS2)
            _warm(kd, perm, dev)
            _warm(ko, perm[::-1], dev)
            local = F.WindowAggOperator(w, aggs=aggs, expected_keys=KEYS2, buffer_records=1 << 20, local_partials=True)
            glob = F.WindowAggOperator(w, aggs=aggs, expected_keys=KEYS2 // WORLD + 1, buffer_records=1 << 20,
                                       key_group_range=kg)
            return TwoPhaseSubtask(GpuPair(local, glob, dev, key_dicts=(kd, ko)),
                                   TorchRounds(via_cpu=True, max_parallelism=MAXP, key_hash=L.KEYHASH_DICT_ID), device=dev)

        def feed(sub, b0, b1, snap_at=None):
            """batches [b0, b1); rank 0 forwards a watermark after every batch, rank 1 after every
            other one; returns the decoded rows, the barrier's snapshot and the rows before it"""
            mx, snap, before = -(1 << 63), None, None
            every = 1 if rank == 0 else 2
            for bi in range(b0, b1):
                lo, hi = bi * BATCH2, (bi + 1) * BATCH2
                sub.process_batch(_packed(key[lo:hi], dev), torch.from_numpy(ts[lo:hi]).to(dev),
                                  torch.from_numpy(val[lo:hi]).to(dev))
                mx = max(mx, int(ts[:hi].max()))
                if bi % every == every - 1:
                    sub.process_watermark(mx - DELAY - 1)
                sub.drain()
                if bi == snap_at:
                    snap = sub.prepare_snapshot_pre_barrier(1)
                    before = sum(len(r) for kk, r in sub.output if kk == "rows")
            sub.end_input()
            rows = [r for kk, r in sub.output if kk == "rows"]
            if not rows:
                return None, snap, before
            rows, uniq = _decode(np.concatenate(rows), sub.pair.key_dicts[1], KEYS2)
            # every decoded key's owner is the rank that fired it
            assert all(O.key_group_of_row(r, MAXP) * WORLD // MAXP == rank for r in uniq)
            return rows, snap, before

        def close(sub):
            for x in (sub.pair.local, sub.pair.glob) + tuple(sub.pair.key_dicts):
                x.close()

        nb = N2 // BATCH2
        sub = subtask()
        rows, snap, before = feed(sub, 0, nb, CKPT_AFTER if ckpt else None)
        rounds, sent = sub.rounds_run, sub.rounds.bytes_sent
        close(sub)
        after = None
        if ckpt:
            # failover: the images and their key rows of every subtask; fresh operators and fresh
            # dictionaries re-intern the key rows and restore their key-group range; the sources replay
            snaps = [None] * WORLD
            dist.all_gather_object(snaps, snap)
            sub2 = subtask()
            info = restore_union_dict_ids(sub2.pair.glob, snaps, sub2.pair.key_dicts[1])
            assert info["rows_in"] == sum(len(s[0]["key"]) for s in snaps) and 0 < info["rows_kept"] < info["rows_in"]
            after, _, _ = feed(sub2, CKPT_AFTER + 1, nb)
            close(sub2)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, _pack(rows), before, _pack(after), rounds, sent, None))
    except Exception as e:   # reported to the parent
        import traceback
        q.put((rank, None, None, None, 0, 0, traceback.format_exc() + repr(e)))


def _oracle2(O):
    return _oracle(O, "tumble", [_stream(N2, KEYS2, RATE2, 8300 + r) for r in range(WORLD)])


def test_two_ranks_with_different_dictionaries_match_the_oracle(oracle_mod):
    res = _spawn(_gloo_rank, WORLD, _free_port(), False)
    assert all(r[4] > 1 and r[5] > 0 for r in res)
    _compare(np.concatenate([_unpack(r[1]) for r in res if r[1] is not None]), _oracle2(oracle_mod), "tumble")


def test_failover_with_dictionary_keys_is_exactly_once(oracle_mod):
    res = _spawn(_gloo_rank, WORLD, _free_port(), True)
    e = _oracle2(oracle_mod)
    _compare(np.concatenate([_unpack(r[1]) for r in res if r[1] is not None]), e, "tumble")   # without the failover
    # the committed output of the failover run: each subtask's rows before its barrier, then the
    # restored subtasks' rows
    parts = [_unpack(r[1])[:r[2]] for r in res] + [_unpack(r[3]) for r in res if r[3] is not None]
    _compare(np.concatenate(parts), e, "tumble")
