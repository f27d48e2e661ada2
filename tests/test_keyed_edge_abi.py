"""The keyed two-phase edge (dictionary keys cross the edge as key rows) without a GPU: the two
entry points as the header, the export map, the built library, the ctypes binding and the Java
shim declare them; their argument checks, which run before any device call; and the keyed
TorchRounds protocol on two gloo ranks whose "dictionaries" are plain Python dicts handing out
ids in DIFFERENT orders -- the ids a rank receives must decode to the keys that were sent, and
the rows must be those the unkeyed protocol delivers for the same data."""
import ctypes as C
import os
import re
import socket
import subprocess

import numpy as np

from flink_amd import _lib as L
from flink_amd import keys as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flinkgpu.h")
JAVA = os.path.join(ROOT, "java", "src", "main", "java", "org", "apache", "flink", "table", "runtime", "operators",
                    "window", "gpu")

WORLD, MAXP = 2, 128
N, KEYS, BATCH, DELAY, RATE = 24_000, 1500, 4_000, 400, 10


def test_header_declares_both_functions():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"int\s+fg_partition_keyed_by_owner\s*\(([^)]*)\)\s*;", src)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["fg_key_dict* d", "void* stream", "int64_t n", "int32_t ncols", "const int64_t* const* cols",
                    "int32_t parallelism", "int64_t* const* out_cols", "int64_t* counts", "int32_t* out_key_lengths",
                    "uint8_t* out_key_bytes", "int64_t cap_bytes", "int64_t* out_byte_counts", "int64_t* out_nbytes"]
    m = re.search(r"int\s+fg_comm_set_key_dicts\s*\(([^)]*)\)\s*;", src)
    assert m
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ["fg_comm* c", "fg_key_dict* local_keys",
                                                                    "fg_key_dict* global_keys"]
    assert "Not for per-rank dictionary ids" not in open(HEADER).read()


def test_symbols_are_exported_and_bound():
    names = ("fg_partition_keyed_by_owner", "fg_comm_set_key_dicts")
    vmap = open(os.path.join(ROOT, "flink_amd", "csrc", "libflinkgpu.map")).read()
    assert re.search(r"global:\s*fg_\*;", vmap)   # (the C-ABI prefix is what the map exports)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert n in L.EXPORTS, n
        assert re.search(rf"\bT {n}$", nm, re.M), n
    lib = L.load()
    P = C.c_void_p
    assert lib.fg_partition_keyed_by_owner.argtypes == [P, P, C.c_int64, C.c_int32, P, C.c_int32, P, P, P, P, C.c_int64,
                                                        P, C.POINTER(C.c_int64)]
    assert lib.fg_comm_set_key_dicts.argtypes == [P, P, P]
    assert lib.fg_partition_keyed_by_owner.restype is C.c_int and lib.fg_comm_set_key_dicts.restype is C.c_int
    assert lib.fg_abi_version() == 16


def test_java_and_jni_agree_on_comm_set_key_dicts():
    gpu = open(os.path.join(JAVA, "FlinkGpu.java")).read()
    m = re.search(r"public static native void commSetKeyDicts\(([^)]*)\);", gpu, re.S)
    assert m, "FlinkGpu.java declares no commSetKeyDicts"
    assert [a.split()[0] for a in m.group(1).split(",")] == ["long", "long", "long"]
    jni = open(os.path.join(ROOT, "jni", "flink_gpu_jni.c")).read()
    m = re.search(r"JNIEXPORT void JNICALL FN\(commSetKeyDicts\)\(([^)]*)\)", jni, re.S)
    assert m and len(m.group(1).split(",")) == 2 + 3
    assert "fg_comm_set_key_dicts(" in jni


def test_null_handles_are_einval_without_a_device():
    lib = L.load()
    nbytes = C.c_int64(-1)
    assert lib.fg_partition_keyed_by_owner(None, None, 0, 1, None, 1, None, None, None, None, 0, None,
                                           C.byref(nbytes)) == L.FG_EINVAL
    col = (C.c_void_p * 1)(0)
    assert lib.fg_partition_keyed_by_owner(None, None, 1, 1, col, 2, col, None, None, None, 0, None,
                                           C.byref(nbytes)) == L.FG_EINVAL
    assert nbytes.value == -1
    assert lib.fg_comm_set_key_dicts(None, None, None) == L.FG_EINVAL


def test_python_mirror_exists():
    from flink_amd import comm, exchange, two_phase
    assert callable(exchange.partition_keyed_by_owner)
    assert callable(comm.Communicator.set_key_dicts)
    assert callable(two_phase.image_key_rows) and callable(two_phase.restore_union_dict_ids)
    import inspect
    assert "key_dicts" in inspect.signature(two_phase.GpuPair.__init__).parameters


# ---- the keyed TorchRounds protocol on two gloo ranks ------------------------------------------------

def _key_row(k):
    """a STRING key row: short names inline (16 bytes), long ones in the variable part (32 bytes)"""
    return K.key_row((f"u{k}" if k % 3 == 0 else f"user{k:08x}",), ("string",))


class PyDict:
    """key rows -> ids with the layout of the GPU dictionary's (ordinal << 7 | key group), on the host"""

    def __init__(self, O):
        self.O, self.ids, self.rows = O, {}, []

    def intern(self, row):
        i = self.ids.get(row)
        if i is None:
            i = self.ids[row] = len(self.rows) << 7 | self.O.key_group_of_row(row, MAXP)
            self.rows.append(row)
        return i

    def row(self, i):
        return self.rows[i >> 7]


class OraclePair:
    """the oracle's local / global operators behind the pair interface; keyed=True: the operators
    aggregate ids of two PyDicts and the rounds carry the key rows (test only)"""

    def __init__(self, O, rank, keyed):
        self.O, self.keyed = O, keyed
        self.local = O.OracleOperator(kind=O.TUMBLE, size=500, phase=O.PHASE_LOCAL)
        self.glob = O.OracleOperator(kind=O.TUMBLE, size=500, phase=O.PHASE_GLOBAL)
        self.fired, self.grows = [], []
        if keyed:
            self.key_dicts = (PyDict(O), PyDict(O))
            order = range(KEYS) if rank == 0 else range(KEYS - 1, -1, -1)   # the ranks' id orders differ
            for k in order:
                self.key_dicts[0].intern(_key_row(k))
            for k in (range(0, KEYS, 2) if rank == 0 else range(1, KEYS, 2)):   # ... and the owners' again
                self.key_dicts[1].intern(_key_row(k))

    def local_batch(self, key, ts, val):
        if self.keyed:
            key = np.array([self.key_dicts[0].intern(_key_row(int(k))) for k in key], dtype=np.int64)
        self.local.process_batch(key, ts, val)

    def local_watermark(self, wm):
        self.local.process_watermark(wm)
        self.fired.append(self.local.take_rows())

    def local_rows(self, mode, world, maxp, key_hash):
        import torch
        if mode == 2:
            none = (None, torch.zeros(world, dtype=torch.int64))
            return none + (None,) if self.keyed else none
        if mode == 1:
            self.local.prepare_snapshot()
            self.fired.append(self.local.take_rows())
        part = np.concatenate(self.fired) if self.fired else np.zeros(0, dtype=self.O.ROW_DTYPE)
        self.fired = []
        if self.keyed:
            assert key_hash == L.KEYHASH_DICT_ID
            kg = K.key_group_of_id(part["key"], maxp).astype(np.int64)
        else:
            kg = self.O.key_groups_binaryrow(part["key"], maxp).astype(np.int64)
        owner = kg * world // maxp
        part = part[np.argsort(owner, kind="stable")]
        owner = np.sort(owner)
        words = part.view(np.int64).reshape(len(part), self.O.ROW_DTYPE.itemsize // 8)
        cols = [torch.from_numpy(np.ascontiguousarray(words[:, j])) for j in range(words.shape[1])]
        counts = torch.from_numpy(np.bincount(owner, minlength=world).astype(np.int64))
        if not self.keyed:
            return cols, counts
        rows = [self.key_dicts[0].row(int(i)) for i in part["key"]]
        buf, _, lens = K.pack_key_rows(rows) if rows else (np.zeros(0, np.uint8), None, np.zeros(0, np.int32))
        padded = (lens.astype(np.int64) + 7) & ~7
        bcounts = np.bincount(owner, weights=padded, minlength=world).astype(np.int64)
        return cols, counts, (torch.from_numpy(lens.copy()), torch.from_numpy(buf[:int(padded.sum())].copy()),
                              torch.from_numpy(bcounts))

    def global_add(self, cols, key_rows=None):
        import torch
        cols = list(cols)
        if self.keyed:
            lens, data = key_rows[0].numpy().astype(np.int64), key_rows[1].numpy().tobytes()
            padded = (lens + 7) & ~7
            assert int(padded.sum()) == len(data)
            off = np.cumsum(padded) - padded
            ids = [self.key_dicts[1].intern(data[o:o + n]) for o, n in zip(off.tolist(), lens.tolist())]
            cols[0] = torch.tensor(ids, dtype=torch.int64)
        else:
            assert key_rows is None
        rows = np.ascontiguousarray(torch.stack(cols, dim=1).numpy()).view(self.O.ROW_DTYPE).reshape(-1)
        self.glob.process_partials(rows)

    def global_advance(self, wm):
        self.glob.process_watermark(wm)
        self.grows.append(self.glob.take_rows())

    def global_collect(self):
        if not self.grows:
            return None
        r, self.grows = np.concatenate(self.grows), []
        return r


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, port, q):
    import torch.distributed as dist

    from flink_amd.two_phase import TorchRounds, TwoPhaseSubtask
    from oracle import oracle as O
    from tests.streams import make_stream
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    key, ts, val, _ = make_stream(N, KEYS, "f64", seed=5100 + rank, jitter_ms=300, rate_per_ms=RATE)
    out = []
    try:
        for keyed in (True, False):
            pair = OraclePair(O, rank, keyed)
            sub = TwoPhaseSubtask(pair, TorchRounds(via_cpu=True))
            every, mx = (1 if rank == 0 else 3), -(1 << 63)
            for bi, lo in enumerate(range(0, N, BATCH)):
                hi = lo + BATCH
                sub.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
                mx = max(mx, int(ts[lo:hi].max()))
                if bi % every == every - 1:
                    sub.process_watermark(mx - DELAY)
                sub.drain()
            sub.end_input()
            rows = [r for k, r in sub.output if k == "rows"]
            rows = np.concatenate(rows) if rows else np.zeros(0, O.ROW_DTYPE)
            sent = sub.rounds.bytes_sent
            if keyed:   # the received ids decode, through the owner's dictionary, to key rows
                names = [pair.key_dicts[1].row(int(i)) for i in rows["key"]]
                owners = [O.key_group_of_row(r, MAXP) * WORLD // MAXP for r in names]
                assert all(o == rank for o in owners), "a key fired on a rank that does not own it"
                out.append((rows.tobytes(), names, sent))
            else:
                out.append((rows.tobytes(), None, sent))
        q.put((rank, out, None))
    except Exception as e:   # reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc() + repr(e)))
    dist.destroy_process_group()


def test_keyed_torch_rounds_ship_key_rows_between_two_gloo_ranks(oracle_mod):
    import torch.multiprocessing as mp
    O = oracle_mod
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in range(WORLD))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(err is None for *_, err in res), [err for *_, err in res]
    index = {_key_row(k): k for k in range(KEYS)}
    keyed, plain = [], []
    for _, (kd, un), _ in res:
        rows = np.frombuffer(kd[0], dtype=O.ROW_DTYPE).copy()
        rows["key"] = [index[r] for r in kd[1]]   # the sent keys, not ids of either dictionary
        keyed.append(rows)
        plain.append(np.frombuffer(un[0], dtype=O.ROW_DTYPE))
        assert kd[2] > un[2] > 0   # (the key rows are counted in bytes_sent)
    srt = lambda a: a[np.lexsort((a["key"], a["window_end"]))]
    g, e = srt(np.concatenate(keyed)), srt(np.concatenate(plain))
    assert len(g) == len(e) > 0
    for f in ("key", "window_start", "window_end", "cnt_star", "cnt_val"):
        assert np.array_equal(g[f], e[f]), f
    # (the two ranks' partial sums of a slice merge in arrival order: the project's 1e-9 relative)
    assert np.allclose(g["sum_d"], e["sum_d"], rtol=1e-9, atol=0)
