"""GPU tests of fg_key_dict_rows / KeyDictionary.rows / keys.reintern: the packed key rows of ids,
gathered on the GPU in the layout fg_key_dict_intern reads.

The reference everywhere is the list of row bytes the test itself packed and interned (the ids the
intern returned, in the test's own id -> row record) -- never KeyDictionary.lookup, which is built
on the code under test."""
import collections
import ctypes as C
import re

import numpy as np
import pytest

import flink_amd as F
from flink_amd import _lib as L
from flink_amd import keys as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MAXP = 128
TYPES = ["string", "bigint"]
SCAN_BLOCK = 256      # ids per scan block and per copy workgroup (kRowsBlock in fg_keydict.hip)
SENTINEL = 0xA5
SHORT_LENGTHS = (0, 4, 8, 12, 16, 44, 64)   # 4, 12 and 44 end in a 4-byte pad
LONG_LENGTHS = (4_100, 70_000)              # the second: 35 strides of one workgroup over one row


def raw_rows(rng, lengths, count):
    """`count` distinct rows of random bytes, their lengths drawn from `lengths`"""
    out = {}
    while len(out) < count:
        n = int(rng.choice(lengths))
        out[rng.integers(0, 256, n, dtype=np.uint8).tobytes()] = None
    return list(out)


def padded(row):
    return row + b"\0" * (-len(row) % 8)


def assert_packed(buf, off, ln, exp_rows, ctx=""):
    """lengths, all n + 1 offsets against the padded prefix sum, nbytes, every row's bytes and pad"""
    lens = np.array([len(r) for r in exp_rows], dtype=np.int32)
    exp_off = np.zeros(len(exp_rows) + 1, dtype=np.int64)
    exp_off[1:] = np.cumsum((lens.astype(np.int64) + 7) & ~7)
    assert np.array_equal(np.asarray(ln), lens), ctx
    assert np.asarray(off).dtype == np.int64 and np.array_equal(np.asarray(off), exp_off), ctx
    assert len(buf) == exp_off[-1], ctx
    assert np.asarray(buf).tobytes() == b"".join(padded(r) for r in exp_rows), ctx


def to_host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def dev_ids(ids):
    import torch
    return torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(torch.device("cuda", 0))


def call_rows(d, ids, cap, device=False, null_buf=False, room=0):
    """fg_key_dict_rows itself, into sentinel-filled outputs: (rc, nbytes, bytes[cap + room], offsets,
    lengths) as numpy arrays"""
    lib = d._lib
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    n = len(ids)
    nbytes = C.c_int64(-1)
    if device:
        import torch
        dev = torch.device("cuda", 0)
        t_ids = torch.from_numpy(ids).to(dev)
        buf = torch.full((max(cap + room, 8),), SENTINEL, dtype=torch.uint8, device=dev)
        off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
        ln = torch.full((n,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()   # the fills before the dictionary's stream writes
        ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    else:
        t_ids = ids
        buf = np.full(max(cap + room, 8), SENTINEL, dtype=np.uint8)
        off = np.full(n + 1, -7, dtype=np.int64)
        ln = np.full(n, -7, dtype=np.int32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    rc = lib.fg_key_dict_rows(d._h, L.DEVICE if device else L.HOST, n, ptr(t_ids), None if null_buf else ptr(buf), cap,
                              ptr(off), ptr(ln), C.byref(nbytes))
    return rc, int(nbytes.value), to_host(buf), to_host(off), to_host(ln)


def last_error(d):
    return d._lib.fg_key_dict_last_error(d._h).decode()


@pytest.fixture(scope="module")
def shapes():
    """one dictionary of short rows of every pad shape and two long ones, interned once:
    (dictionary, {id: row bytes}, ids of the short rows, ids of the long rows); never modified"""
    rng = np.random.default_rng(17)
    rows = raw_rows(rng, SHORT_LENGTHS, 400) + raw_rows(rng, LONG_LENGTHS[:1], 1) + raw_rows(rng, LONG_LENGTHS[1:], 1)
    assert {len(r) for r in rows} == set(SHORT_LENGTHS) | set(LONG_LENGTHS)
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=1000)
    ids, _ = d.intern(rows)
    assert len(d) == len(rows) == len(set(ids.tolist()))
    row_of = dict(zip(ids.tolist(), rows))
    yield d, row_of, ids[:-2].copy(), ids[-2:].copy()
    d.close()


def pick_ids(rng, short, long_, n):
    """n ids in random order with repeats; from 63 ids on both long rows are among them, twice"""
    ids = short[rng.integers(0, len(short), n)]
    if n >= 63:
        ids[rng.choice(n, 4, replace=False)] = [long_[0], long_[1], long_[1], long_[0]]
    return ids


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 3 * SCAN_BLOCK + 1])
def test_rows_of_every_shape(shapes, n):
    d, row_of, short, long_ = shapes
    rng = np.random.default_rng(100 + n)
    ids = pick_ids(rng, short, long_, n)
    if n == 1:
        ids[0] = long_[1]   # the 70,000-B row alone
    exp = [row_of[i] for i in ids.tolist()]
    buf, off, ln = d.rows(ids)
    assert isinstance(buf, np.ndarray) and buf.dtype == np.uint8 and ln.dtype == np.int32
    assert_packed(buf, off, ln, exp, f"host n={n}")
    tb, to, tl = d.rows(dev_ids(ids))
    assert tb.is_cuda and to.is_cuda and tl.is_cuda
    assert_packed(to_host(tb), to_host(to), to_host(tl), exp, f"device n={n}")


@pytest.mark.parametrize("which", ["pad4", "empty", "long"])
def test_one_id_repeated(shapes, which):
    """HOP windows repeat keys: a repeated id gets a copy of its row per occurrence"""
    d, row_of, short, long_ = shapes
    want = {"pad4": 44, "empty": 0, "long": LONG_LENGTHS[0]}[which]
    one = next(i for i in list(short) + list(long_) if len(row_of[int(i)]) == want)
    n = SCAN_BLOCK + 1
    ids = np.full(n, one, dtype=np.int64)
    for src in (ids, dev_ids(ids)):
        buf, off, ln = d.rows(src)
        assert_packed(to_host(buf), to_host(off), to_host(ln), [row_of[int(one)]] * n, which)


def test_host_and_device_agree(shapes):
    d, row_of, short, long_ = shapes
    ids = pick_ids(np.random.default_rng(5), short, long_, 2 * SCAN_BLOCK + 77)
    h = d.rows(ids)
    t = d.rows(dev_ids(ids))
    for a, b in zip(h, t):
        assert a.dtype == to_host(b).dtype and np.array_equal(a, to_host(b))
    assert int(h[1][-1]) == len(h[0])   # nbytes == offsets[n]
    e = d.rows(np.zeros(0, dtype=np.int64))
    assert len(e[0]) == 0 and e[1].tolist() == [0] and len(e[2]) == 0
    te = d.rows(dev_ids(np.zeros(0, dtype=np.int64)))
    assert te[0].numel() == 0 and to_host(te[1]).tolist() == [0] and te[2].numel() == 0


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_capacity(shapes, device):
    d, row_of, short, long_ = shapes
    ids = pick_ids(np.random.default_rng(8), short, long_, SCAN_BLOCK + 44)
    exp = [row_of[i] for i in ids.tolist()]
    lens = np.array([len(r) for r in exp], dtype=np.int32)
    exp_off = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 7) & ~7)])
    total = int(exp_off[-1])
    for cap, null_buf in ((total - 8, False), (0, True)):   # too small by one word; the sizing call
        rc, nbytes, buf, off, ln = call_rows(d, ids, cap, device, null_buf)
        assert rc == L.FG_EFULL, (cap, rc, last_error(d))
        assert nbytes == total and np.array_equal(off, exp_off) and np.array_equal(ln, lens)
        assert (buf == SENTINEL).all(), "FG_EFULL wrote to out_bytes"
    rc, nbytes, buf, off, ln = call_rows(d, ids, total, device, room=64)   # the exact capacity
    assert rc == L.FG_OK, last_error(d)
    assert nbytes == total
    assert_packed(buf[:total], off, ln, exp)
    assert (buf[total:] == SENTINEL).all(), "bytes past cap_bytes were written"


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_bad_ids(shapes, device):
    d, row_of, short, long_ = shapes
    good = pick_ids(np.random.default_rng(9), short, long_, SCAN_BLOCK + 9)
    past = np.int64(len(d) << K.dict_kg_bits(MAXP))   # the first ordinal the dictionary has not handed out
    n_before = len(d)
    for bad_at, count, first in (({SCAN_BLOCK + 3: -1}, 1, SCAN_BLOCK + 3), ({70: past}, 1, 70),
                                 ({SCAN_BLOCK + 3: -1, 70: past, 200: -5}, 3, 70)):
        ids = good.copy()
        for at, v in bad_at.items():
            ids[at] = v
        rc, nbytes, buf, off, ln = call_rows(d, ids, 1 << 20, device)
        assert rc == L.FG_EINVAL
        msg = last_error(d)
        assert re.search(rf"\b{count} unknown ids\b", msg), msg
        assert re.search(rf"index {first}\b", msg), msg
        assert (buf == SENTINEL).all(), "a call with bad ids wrote to out_bytes"
        with pytest.raises(KeyError, match=rf"index {first}\b"):
            d.rows(dev_ids(ids) if device else ids)
    assert len(d) == n_before
    rc, nbytes, buf, off, ln = call_rows(d, good, 1 << 20, device)   # the dictionary stays usable
    assert rc == L.FG_OK, last_error(d)
    assert_packed(buf[:nbytes], off, ln, [row_of[i] for i in good.tolist()])


def test_argument_errors_on_an_open_dictionary(shapes):
    d, row_of, short, long_ = shapes
    lib, h = d._lib, d._h
    ids = np.ascontiguousarray(short[:4])
    off, ln, buf = np.zeros(5, dtype=np.int64), np.zeros(4, dtype=np.int32), np.zeros(512, dtype=np.uint8)
    nb = C.c_int64(-1)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    bad_calls = [
        (L.HOST, -1, p(ids), p(buf), 512, p(off), p(ln), C.byref(nb)),
        (L.HOST, 1 << 31, p(ids), p(buf), 512, p(off), p(ln), C.byref(nb)),
        (L.HOST, 4, None, p(buf), 512, p(off), p(ln), C.byref(nb)),
        (L.HOST, 4, p(ids), p(buf), 512, None, p(ln), C.byref(nb)),
        (L.HOST, 4, p(ids), p(buf), 512, p(off), None, C.byref(nb)),
        (L.HOST, 4, p(ids), p(buf), 512, p(off), p(ln), None),
        (L.HOST, 4, p(ids), p(buf), -1, p(off), p(ln), C.byref(nb)),
        (L.HOST, 4, p(ids), None, 512, p(off), p(ln), C.byref(nb)),
        (7, 4, p(ids), p(buf), 512, p(off), p(ln), C.byref(nb)),
        (L.DEVICE, 4, p(ids), C.c_void_p(buf.ctypes.data | 4), 512, p(off), p(ln), C.byref(nb)),   # refused unread
    ]
    for args in bad_calls:
        assert lib.fg_key_dict_rows(h, *args) == L.FG_EINVAL, args[:2]
    off[0] = -1
    assert lib.fg_key_dict_rows(h, L.HOST, 0, None, None, 0, p(off), None, C.byref(nb)) == L.FG_OK
    assert nb.value == 0 and off[0] == 0
    assert lib.fg_key_dict_rows(h, L.HOST, 0, None, None, 0, None, None, None) == L.FG_OK
    buf2, off2, ln2 = d.rows(ids)
    assert_packed(buf2, off2, ln2, [row_of[i] for i in ids.tolist()])


def test_state_async_intern_growth_and_rebuild():
    """FG_ESTATE between intern_async and intern_wait; afterwards, and after further interns that
    reallocate the arena and rebuild the table, earlier ids still give their rows. The table is
    rebuilt when its free half falls under 2^20 slots: the first miss takes it to 2^22 slots, and
    with more than 2^20 ids in it the next call that misses rebuilds it again."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23)
    rows = raw_rows(rng, SHORT_LENGTHS + (LONG_LENGTHS[0],), 300)
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=16)
    try:
        ids, _ = d.intern(rows[:200])
        buf, off, ln = K.pack_key_rows(rows[200:])
        p = (torch.from_numpy(buf.copy()).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(ln).to(dev))
        ids2, _ = d.intern_async(p)
        with pytest.raises(F.FlinkGpuError) as ei:
            d.rows(ids)
        assert ei.value.code == L.FG_ESTATE
        with pytest.raises(F.FlinkGpuError) as ei:
            d.rows(dev_ids(ids))
        assert ei.value.code == L.FG_ESTATE
        d.intern_wait()
        all_ids = np.concatenate([ids, ids2.cpu().numpy()])
        assert_packed(*d.rows(all_ids), rows, "after the wait")

        def bigint_rows(lo, n):   # n distinct 16-B rows (a BIGINT key row: null bits, value)
            r = np.zeros((n, 2), dtype=np.int64)
            r[:, 1] = np.arange(lo, lo + n)
            return (torch.from_numpy(r.view(np.uint8).reshape(-1)).to(dev),
                    torch.arange(n, dtype=torch.int64, device=dev) * 16,
                    torch.full((n,), 16, dtype=torch.int32, device=dev))
        n_big = (1 << 20) + 5000
        big_ids, _ = d.intern(packed=bigint_rows(1 << 40, n_big), key_groups=False)
        assert len(d) == len(rows) + n_big
        more_ids, _ = d.intern(packed=bigint_rows(1 << 41, 3000), key_groups=False)   # misses: the table is rebuilt
        assert len(d) == len(rows) + n_big + 3000
        perm = rng.permutation(len(all_ids))
        assert_packed(*d.rows(all_ids[perm]), [rows[i] for i in perm], "after growth and a rebuild")
        tail = big_ids[-3:].cpu().numpy().tolist() + more_ids[:2].cpu().numpy().tolist()
        vals = [(1 << 40) + n_big - 3 + k for k in range(3)] + [(1 << 41) + k for k in range(2)]
        assert_packed(*d.rows(np.array(tail, dtype=np.int64)),
                      [np.array([0, v], dtype=np.int64).tobytes() for v in vals], "the new rows")
    finally:
        d.close()


def test_host_resolved_entries(monkeypatch):
    """a 6-bit table tag: nearly every row collides with another's tag and is appended to the arena
    by the host (out of the table); such rows come back exactly as well"""
    monkeypatch.setenv("FG_DICT_TAG_BITS", "6")
    rng = np.random.default_rng(29)
    rows = raw_rows(rng, SHORT_LENGTHS + (LONG_LENGTHS[0],), 1500)
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=16)
    try:
        ids, _ = d.intern(rows)
        assert len(d) == len(rows) > 64   # (at most 64 tags: the rest were resolved on the host)
        pick = rng.integers(0, len(rows), 2 * SCAN_BLOCK + 5)
        exp = [rows[i] for i in pick]
        assert_packed(*d.rows(ids[pick]), exp, "host")
        assert_packed(*(to_host(x) for x in d.rows(dev_ids(ids[pick]))), exp, "device")
    finally:
        d.close()


def string_key_rows(rng, n):
    out = {}
    while len(out) < n:
        s = "".join(chr(c) for c in rng.integers(0x20, 0x7f, int(rng.integers(0, 41))))
        out[K.key_row([s if rng.random() > 0.02 else None, int(rng.integers(-5, 5))], TYPES)] = None
    return list(out)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_round_trip_into_another_dictionary(device):
    """the output of one dictionary is valid input to the intern of another"""
    rng = np.random.default_rng(31)
    rows = string_key_rows(rng, 2000)
    src = F.KeyDictionary(max_parallelism=MAXP)
    dst = F.KeyDictionary(max_parallelism=MAXP)
    try:
        ids_all, _ = src.intern(rows)
        pick = rng.integers(0, len(rows), 3 * SCAN_BLOCK + 1)
        ids = ids_all[pick]
        exp = [rows[i] for i in pick]
        src_ids = dev_ids(ids) if device else ids
        buf, off, ln = src.rows(src_ids)
        new_ids, kg = dst.intern(packed=(buf, off[:-1], ln))
        exp_kg = np.array([O.key_group_of_row(r, MAXP) for r in exp], dtype=np.int32)
        assert np.array_equal(to_host(kg), exp_kg)
        assert np.array_equal(K.key_group_of_id(to_host(new_ids), MAXP), exp_kg)
        assert len(dst) == len(set(exp))
        back = dst.rows(new_ids)
        for a, b in zip(back, (buf, off, ln)):
            assert np.array_equal(to_host(a), to_host(b))
        assert_packed(*(to_host(x) for x in back), exp)
        again = K.reintern(src_ids, src, dst)   # the same step as one call: the same ids
        assert np.array_equal(to_host(again), to_host(new_ids))
        assert hasattr(again, "is_cuda") == device
    finally:
        src.close()
        dst.close()


@pytest.mark.parametrize("kind", ["tumble", "hop"])
def test_rescale_with_string_keys(kind):
    """Rescale 2 -> 2 at other key-group ranges, STRING keys, end to end: two old subtasks (key
    groups 0..63 and 64..127), each with its own dictionary, snapshot mid-stream; two new subtasks
    (0..42 and 43..127) with fresh dictionaries reintern the key column of BOTH old images and
    restore their range out of them by the ids' key groups. Each new subtask's state, its keys
    turned back into bytes by its own dictionary, is the union of the old images' rows whose key
    row falls in its range (the oracle's key group of the row bytes, the bytes from the test's own
    id -> row record). BIGINT values: sums are exact. One new subtask restores from host images,
    the other from device tensors."""
    import torch
    from tests.test_gpu_restore_range import mk
    spec = dict(kind=kind, size=3000 if kind == "hop" else 1000, slide=1000 if kind == "hop" else 0, vt="i64")
    rng = np.random.default_rng(37)
    rows_all = string_key_rows(rng, 3000)
    kg_all = np.array([O.key_group_of_row(r, MAXP) for r in rows_all])
    cols = ("slice_end", "cnt_star", "cnt_val", "sum")
    old, opened = [], []
    try:
        for lo, hi in ((0, 63), (64, 127)):
            mine = np.flatnonzero((kg_all >= lo) & (kg_all <= hi))
            n = 30_000
            pick = mine[rng.integers(0, len(mine), n)]
            ts = (1_000_000 + np.arange(n) // 10 + rng.integers(0, 300, n)).astype(np.int64)
            val = rng.integers(-1000, 1000, n).astype(np.int64)
            d = F.KeyDictionary(max_parallelism=MAXP)
            op = mk(spec, (lo, hi))
            opened += [d, op]
            row_of = {}
            for a in range(0, n, 10_000):
                b = a + 10_000
                rows = [rows_all[i] for i in pick[a:b]]
                ids, _ = d.intern(rows)
                row_of.update(zip(ids.tolist(), rows))
                op.process_batch(ids, ts[a:b], val[a:b])
                op.process_watermark(int(ts[b - 1]) - 1500)
            op.prepare_snapshot_pre_barrier()
            img, twm = op.snapshot_state()
            assert len(np.unique(img["slice_end"])) >= 2 and len(img["key"]) > 1000
            old.append((d, img, twm, row_of))
        total_rows = sum(len(img["key"]) for _, img, _, _ in old)
        kept = 0
        for (lo, hi), device in (((0, 42), False), ((43, 127), True)):
            nd = F.KeyDictionary(max_parallelism=MAXP)
            op = mk(spec, (lo, hi))
            opened += [nd, op]
            images, expected = [], collections.Counter()
            for d, img, twm, row_of in old:
                mapped = {c: np.asarray(v) for c, v in img.items()}
                if device:
                    mapped = {c: torch.from_numpy(np.array(v)).cuda() for c, v in mapped.items()}
                mapped["key"] = K.reintern(mapped["key"], d, nd)
                images.append((mapped, twm))
                for k, *rest in zip(img["key"].tolist(), *(img[c].tolist() for c in cols)):
                    row = row_of[k]
                    if lo <= O.key_group_of_row(row, MAXP) <= hi:
                        expected[(row, *rest)] += 1
            info = op.restore_state_range(images, key_hash=L.KEYHASH_DICT_ID)
            assert info["rows_in"] == total_rows
            assert info["rows_kept"] == sum(expected.values())
            kept += info["rows_kept"]
            got_img, _ = op.snapshot_state()
            buf, off, ln = nd.rows(got_img["key"])
            raw = buf.tobytes()
            got_rows = [raw[o:o + n_] for o, n_ in zip(off[:-1].tolist(), ln.tolist())]
            got = collections.Counter(zip(got_rows, *(got_img[c].tolist() for c in cols)))
            assert got == expected, f"{kind} range {lo}..{hi}"
        assert kept == total_rows
    finally:
        for x in reversed(opened):
            x.close()


def test_timing_class(shapes):
    d, row_of, short, long_ = shapes
    d.set_timing(True)
    try:
        before = d.kernel_stats().get("dict_rows", dict(launches=0, records=0))
        ids = pick_ids(np.random.default_rng(41), short, long_, 300)
        assert call_rows(d, ids, 1 << 20)[0] == L.FG_OK   # (one C call each: no retry at a larger size)
        assert call_rows(d, ids[:100], 1 << 20, device=True)[0] == L.FG_OK
        after = d.kernel_stats()["dict_rows"]
        assert after["launches"] - before["launches"] == 2
        assert after["records"] - before["records"] == 400
        assert after["total_ms"] > 0
    finally:
        d.set_timing(False)
