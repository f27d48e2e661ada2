"""GPU tests of fg_key_dict_project / fg_key_dict_intern_fields (KeyDictionary.project /
intern_fields): the key selector on the GPU -- key rows projected from packed BinaryRowData records.

The reference everywhere is keys.key_row / keys.project_key_row applied to rows the test itself
built, never a dictionary lookup of ids the code under test produced."""
import ctypes as C
import re

import numpy as np
import pytest

import flink_amd as F
from flink_amd import _lib as L
from flink_amd import keys as K
from flink_amd.rows import bit_set_width

pytestmark = pytest.mark.gpu

MAXP = 128
SENTINEL = 0xA5
# input rows: STRING a, BIGINT, INT, DOUBLE, STRING b, BOOLEAN -- a non-key STRING and a value column
# sit between the key fields
T6 = ["string", "bigint", "int", "double", "string", "boolean"]
A, BIG, INT, DBL, B, BOOL = range(6)
STRING_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 44)
LONG_LENGTHS = (4_100, 70_000)
PROJECTIONS = {
    "a": ([A], ["string"]),
    "b_a": ([B, A], ["string", "string"]),          # key order differs from input order
    "a_int_bool": ([A, INT, BOOL], ["string", "int", "boolean"]),
    "bigint": ([BIG], ["bigint"]),
    "a_a": ([A, A], ["string", "string"]),
}
COLS = (BIG, DBL)   # copied out as columns, with their NULL bytes


def proj_of(name, cols=COLS):
    fields, kinds = PROJECTIONS[name]
    return K.RowProjection(6, fields, kinds, col_fields=cols)


def random_record(rng, null_p=0.1, lengths=STRING_LENGTHS):
    def s():
        return bytes(rng.integers(1, 256, int(rng.choice(lengths)), dtype=np.uint8))
    rec = [s(), int(rng.integers(-2**62, 2**62)), int(rng.integers(-2**31, 2**31)), float(rng.integers(0, 4000)) / 4,
           s(), bool(rng.integers(0, 2))]
    return [None if rng.random() < null_p else v for v in rec]


def pack(rows):
    """(bytes u8[], offsets i64[n], lengths i32[n]) of whole input rows, packed back to back"""
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    assert not (lens % 8).any()
    off = np.zeros(len(rows), dtype=np.int64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.int64)
    return np.frombuffer(b"".join(rows) or b"\0" * 8, dtype=np.uint8).copy(), off, lens


def to_host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def last_error(d):
    return d._lib.fg_key_dict_last_error(d._h).decode()


def call_project(d, packed, proj, cap, device=False, null_buf=False, room=64, null_arrays=True):
    """fg_key_dict_project itself, into sentinel-filled outputs: (rc, nbytes, key bytes[cap + room],
    offsets, lengths, cols, col nulls) as numpy arrays"""
    buf, off, ln = packed
    n = len(ln)
    nc = len(proj.col_fields)
    total = C.c_int64(-1)
    if device:
        import torch
        dev = torch.device("cuda", 0)
        src = [torch.from_numpy(x).to(dev) for x in (buf, off, ln)]
        kbuf = torch.full((max(cap + room, 8),), SENTINEL, dtype=torch.uint8, device=dev)
        koff = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
        klen = torch.full((n,), -7, dtype=torch.int32, device=dev)
        cols = [torch.full((n,), -7, dtype=torch.int64, device=dev) for _ in range(nc)]
        nulls = [torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev) for _ in range(nc)]
        torch.cuda.synchronize()   # the fills before the dictionary's stream writes
        ptr = lambda t: t.data_ptr()   # noqa: E731
    else:
        src = [buf, off, ln]
        kbuf = np.full(max(cap + room, 8), SENTINEL, dtype=np.uint8)
        koff = np.full(n + 1, -7, dtype=np.int64)
        klen = np.full(n, -7, dtype=np.int32)
        cols = [np.full(n, -7, dtype=np.int64) for _ in range(nc)]
        nulls = [np.full(n, SENTINEL, dtype=np.uint8) for _ in range(nc)]
        ptr = lambda a: a.ctypes.data   # noqa: E731
    pc = (C.c_void_p * max(nc, 1))(*[ptr(c) for c in cols])
    pn = (C.c_void_p * max(nc, 1))(*[ptr(c) if null_arrays else None for c in nulls])
    ps = proj.struct()
    rc = d._lib.fg_key_dict_project(d._h, L.DEVICE if device else L.HOST, n, ptr(src[0]), len(buf), ptr(src[1]),
                                    ptr(src[2]), C.byref(ps), None if null_buf else ptr(kbuf), cap, ptr(koff), ptr(klen),
                                    pc, pn, C.byref(total))
    return (rc, int(total.value), to_host(kbuf), to_host(koff), to_host(klen), [to_host(c) for c in cols],
            [to_host(c) for c in nulls])


def assert_projected(res, exp_rows, recs, proj, ctx):
    """the lengths, all n + 1 offsets, nbytes, every byte (pads included), nothing past nbytes, the
    columns and their NULL bytes"""
    rc, nbytes, kbuf, koff, klen, cols, nulls = res
    assert rc == L.FG_OK, ctx
    lens = np.array([len(r) for r in exp_rows], dtype=np.int32)
    exp_off = np.zeros(len(exp_rows) + 1, dtype=np.int64)
    exp_off[1:] = np.cumsum(lens.astype(np.int64))
    assert np.array_equal(klen, lens), ctx
    assert koff.dtype == np.int64 and np.array_equal(koff, exp_off), ctx
    assert nbytes == exp_off[-1], ctx
    assert kbuf[:nbytes].tobytes() == b"".join(exp_rows), ctx
    assert (kbuf[nbytes:] == SENTINEL).all(), ctx
    for c, field in enumerate(proj.col_fields):
        isnull = np.array([r[field] is None for r in recs])
        raw = [0 if r[field] is None else r[field] for r in recs]
        want = np.array(raw, dtype=np.float64).view(np.int64) if T6[field] == "double" else np.array(raw, dtype=np.int64)
        assert np.array_equal(cols[c], want), ctx
        assert np.array_equal(nulls[c], isnull.astype(np.uint8)), ctx


@pytest.fixture(scope="module")
def pool():
    """1,000 records with ~10 % NULLs per field, their input rows (RowKinds 0..3) and, per projection,
    their reference key rows; never modified"""
    rng = np.random.default_rng(7)
    recs = [random_record(rng) for _ in range(1000)]
    rows = [K.key_row(r, T6, row_kind=i & 3) for i, r in enumerate(recs)]
    ref = {name: [K.project_key_row(row, proj_of(name)) for row in rows] for name in PROJECTIONS}
    for name, (fields, kinds) in PROJECTIONS.items():   # the reference is key_row of the fields themselves
        assert ref[name][:50] == [K.key_row([r[f] for f in fields], kinds) for r in recs[:50]]
    return recs, rows, ref


@pytest.fixture(scope="module")
def dictionary():
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=1000)
    yield d
    d.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 65_536 + 3])   # the last: a second pass over the block sums
def test_byte_exact_key_rows(pool, dictionary, n, device):
    recs, rows, ref = pool
    rng = np.random.default_rng(n)
    pick = rng.integers(0, len(rows), n)
    packed = pack([rows[i] for i in pick])
    picked = [recs[i] for i in pick]
    for name in PROJECTIONS:
        proj = proj_of(name)
        exp = [ref[name][i] for i in pick]
        cap = sum(len(r) for r in exp)
        res = call_project(dictionary, packed, proj, cap, device=device)
        assert_projected(res, exp, picked, proj, f"{name} n={n} device={device}")


def test_python_interface_numpy_and_tensors(pool, dictionary):
    import torch
    recs, rows, ref = pool
    packed = pack(rows[:300])
    proj = proj_of("b_a")
    exp = b"".join(ref["b_a"][:300])
    buf, off, ln, cols, nulls = dictionary.project(packed, proj)
    assert isinstance(buf, np.ndarray) and buf.tobytes() == exp and len(off) == 301 and off[-1] == len(exp)
    assert len(cols) == len(nulls) == 2 and cols[0].dtype == np.int64 and nulls[0].dtype == np.uint8
    dev = torch.device("cuda", 0)
    tb, to, tl, tc, tn = dictionary.project(tuple(torch.from_numpy(x).to(dev) for x in packed), proj)
    assert tb.is_cuda and to.is_cuda and tl.is_cuda and tc[0].is_cuda and tn[0].is_cuda
    assert to_host(tb).tobytes() == exp and np.array_equal(to_host(tl), ln) and np.array_equal(to_host(tc[1]), cols[1])
    e = dictionary.project((np.zeros(8, dtype=np.uint8), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)), proj)
    assert len(e[0]) == 0 and e[1].tolist() == [0] and len(e[2]) == 0


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_long_strings(dictionary, where, device):
    """a 4,100-byte and a 70,000-byte string among short ones: the write kernel's workgroup strides
    over one row many times"""
    rng = np.random.default_rng(3)
    recs = [random_record(rng, null_p=0.05) for _ in range(300)]
    at = {"first": 0, "middle": 150, "last": 298}[where]
    for j, n_ in enumerate(LONG_LENGTHS):
        recs[at + j][A] = bytes(rng.integers(1, 256, n_, dtype=np.uint8))
    recs[at][B] = bytes(rng.integers(1, 256, LONG_LENGTHS[0] + 3, dtype=np.uint8))
    rows = [K.key_row(r, T6) for r in recs]
    packed = pack(rows)
    for name in ("a", "b_a", "a_a"):
        proj = proj_of(name)
        exp = [K.project_key_row(r, proj) for r in rows]
        res = call_project(dictionary, packed, proj, sum(len(r) for r in exp), device=device)
        assert_projected(res, exp, recs, proj, f"{name} long {where} device={device}")


# rows of [STRING s, INT, SMALLINT, TINYINT, STRING p] for the canonical form
T5 = ["string", "int", "smallint", "tinyint", "string"]


def canonical_variants():
    fields = [b"hello", -7, 300, -3, b"ninebytes"]
    base = K.key_row(fields, T5)
    w = bit_set_width(5)
    out = {"base": base}
    v = bytearray(base)
    v[0] = 3   # RowKind DELETE
    out["rowkind"] = bytes(v)
    v = bytearray(base)
    v[w + 8 + 4: w + 16] = b"\xff" * 4      # upper bytes of the INT slot
    v[w + 16 + 2: w + 24] = b"\xee" * 6     # ... of the SMALLINT slot
    v[w + 24 + 1: w + 32] = b"\xdd" * 7     # ... of the TINYINT slot
    out["upper"] = bytes(v)
    v = bytearray(base)
    assert v[-7:] == b"\0" * 7
    v[-7:] = b"\xcc" * 7                    # the pad after the 9-byte string
    out["pad"] = bytes(v)
    v = bytearray(base)                     # the 5-byte string kept in the variable part, its pad dirty
    v[w: w + 8] = (len(base) << 32 | 5).to_bytes(8, "little")
    out["varpart"] = bytes(v) + b"hello\xbb\xbb\xbb"
    return fields, out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_canonical_form(device):
    fields, variants = canonical_variants()
    proj = K.RowProjection(5, [0, 1, 2, 3, 4], T5)
    want = K.key_row(fields, T5)
    for name, row in variants.items():
        assert K.project_key_row(row, proj) == want, name
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=100)
    rows = list(variants.values())
    packed = pack(rows)
    res = call_project(d, packed, proj, len(want) * len(rows), device=device)
    assert res[0] == L.FG_OK
    assert res[2][:res[1]].tobytes() == want * len(rows)
    if device:
        import torch
        packed = tuple(torch.from_numpy(x).to(torch.device("cuda", 0)) for x in packed)
    ids, kg, _, _ = d.intern_fields(packed, proj)
    assert len(set(to_host(ids).tolist())) == 1 and len(d) == 1
    ids2, _ = d.intern([want])
    assert ids2[0] == to_host(ids)[0] and len(d) == 1
    d.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_sizing_and_efull(pool, dictionary, device):
    recs, rows, ref = pool
    packed = pack(rows[:500])
    proj = proj_of("a_int_bool")
    exp = ref["a_int_bool"][:500]
    size = sum(len(r) for r in exp)
    rc, nbytes, kbuf, koff, klen, cols, nulls = call_project(dictionary, packed, proj, 0, device=device, null_buf=True)
    assert rc == L.FG_EFULL and nbytes == size
    assert koff[-1] == size and np.array_equal(klen, [len(r) for r in exp]) and (kbuf == SENTINEL).all()
    assert np.array_equal(nulls[0], [r[BIG] is None for r in recs[:500]])   # the columns are complete
    rc, nbytes, kbuf, koff, klen, _, _ = call_project(dictionary, packed, proj, size - 8, device=device)
    assert rc == L.FG_EFULL and nbytes == size and (kbuf == SENTINEL).all()
    assert str(size) in last_error(dictionary) and str(size - 8) in last_error(dictionary)
    assert_projected(call_project(dictionary, packed, proj, size, device=device), exp, recs[:500], proj, "cap = size")
    rc, nbytes, _, koff, _, _, _ = call_project(dictionary, (packed[0], packed[1][:0], packed[2][:0]), proj, 0, device=device)
    assert rc == L.FG_OK and nbytes == 0 and koff.tolist() == [0]


def bad_batches():
    """{kind: (packed, projection, null arrays?, indices of the bad rows)}: ten good rows with a
    bad row at 3 and 7. A bad offset points outside its row but inside the batch buffer, with other
    rows after it: a kernel that missed the check would read valid memory and give wrong bytes."""
    rng = np.random.default_rng(11)
    recs = [random_record(rng, null_p=0.0, lengths=(9, 16, 44)) for _ in range(10)]
    rows = [K.key_row(r, T6) for r in recs]
    w = bit_set_width(6)
    fixed = w + 8 * 6
    proj = proj_of("a")
    out = {}

    def tweak(fn):
        buf, off, ln = pack(rows)
        for i in (3, 7):
            fn(buf, off, ln, i)
        return buf, off, ln

    def set_slot(buf, off, i, field, word):
        at = int(off[i]) + w + 8 * field
        buf[at:at + 8] = np.frombuffer(int(word).to_bytes(8, "little"), dtype=np.uint8)

    def offset_of(buf, off, i, field):
        at = int(off[i]) + w + 8 * field
        return int.from_bytes(buf[at:at + 8].tobytes(), "little") >> 32

    def f_negoff(buf, off, ln, i): off[i] = -8
    def f_oddoff(buf, off, ln, i): off[i] += 4
    def f_neglen(buf, off, ln, i): ln[i] = -8
    def f_oddlen(buf, off, ln, i): ln[i] -= 4
    def f_past(buf, off, ln, i): ln[i] = len(buf) - off[i] + 8
    def f_short(buf, off, ln, i): ln[i] = fixed - 8
    def f_inline(buf, off, ln, i): set_slot(buf, off, i, A, 0x88 << 56 | 0x41414141414141)
    def f_varodd(buf, off, ln, i): set_slot(buf, off, i, A, (offset_of(buf, off, i, A) + 4) << 32 | 4)
    def f_varlow(buf, off, ln, i): set_slot(buf, off, i, A, (fixed - 8) << 32 | 8)
    def f_varpast(buf, off, ln, i): set_slot(buf, off, i, A, offset_of(buf, off, i, A) << 32 | (int(ln[i]) + 8))
    for name, fn in (("negative offset", f_negoff), ("offset not a multiple of 8", f_oddoff), ("negative length", f_neglen),
                     ("length not a multiple of 8", f_oddlen), ("row past the buffer", f_past),
                     ("shorter than the fixed part", f_short), ("inline longer than 7", f_inline),
                     ("variable offset not a multiple of 8", f_varodd), ("variable offset below the fixed part", f_varlow),
                     ("variable field past its row", f_varpast)):
        out[name] = (tweak(fn), proj, True, (3, 7))
    # a NULL column field without its NULL bytes
    nrows = list(rows)
    for i in (3, 7):
        rec = list(recs[i])
        rec[DBL] = None
        nrows[i] = K.key_row(rec, T6)
    out["NULL column without null bytes"] = (pack(nrows), proj, False, (3, 7))
    # a key row above the intern's limit: [a, a] of a string whose key row alone would fit
    big = list(recs[3])
    big[A] = b"x" * (1 << 23)
    brows = list(rows)
    brows[3] = K.key_row(big, T6)
    assert 16 + (1 << 23) <= (1 << 24) - 4 < 24 + (1 << 24)
    out["key row above 2^24 - 4"] = (pack(brows), proj_of("a_a"), True, (3,))
    return out


BAD = bad_batches()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", list(BAD))
def test_bad_rows(pool, kind, device):
    packed, proj, null_arrays, where = BAD[kind]
    recs, rows, ref = pool
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=100)
    d.intern(ref["a"][:20])
    size0 = len(d)
    rc, nbytes, kbuf, _, _, _, _ = call_project(d, packed, proj, 1 << 12, device=device, null_arrays=null_arrays)
    assert rc == L.FG_EINVAL, kind
    m = re.search(r"(\d+) bad rows.*index (\d+)", last_error(d))
    assert m and (int(m.group(1)), int(m.group(2))) == (len(where), where[0]), last_error(d)
    assert (kbuf == SENTINEL).all(), kind   # no key byte written
    if null_arrays:
        src = packed
        if device:
            import torch
            src = tuple(torch.from_numpy(x).to(torch.device("cuda", 0)) for x in packed)
        with pytest.raises(F.WindowSpecError, match=r"bad rows"):
            d.intern_fields(src, proj)
    assert len(d) == size0   # nothing interned
    good = pack(rows[:40])   # and the dictionary works afterwards
    res = call_project(d, good, proj_of("a"), sum(len(r) for r in ref["a"][:40]), device=device)
    assert_projected(res, ref["a"][:40], recs[:40], proj_of("a"), kind)
    ids, _, _, _ = d.intern_fields(good, proj_of("a"))
    assert len(set(ids.tolist())) == len(set(ref["a"][:40]))
    d.close()


@pytest.mark.parametrize("fields_first", [True, False], ids=["fields_first", "rows_first"])
def test_intern_agreement(pool, fields_first):
    """intern_fields(records) and intern(host-built key rows) hand out the same ids, whichever sees
    the keys first; repeated keys map to one id; out_kg is the id's key group"""
    import torch
    recs, rows, ref = pool
    rng = np.random.default_rng(5)
    pick = rng.integers(0, len(rows), 5000)
    packed = pack([rows[i] for i in pick])
    key_rows = [ref["a_int_bool"][i] for i in pick]
    proj = proj_of("a_int_bool")
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=1000)
    if fields_first:
        ids_f, kg_f, cols, nulls = d.intern_fields(packed, proj)
        ids_r, kg_r = d.intern(key_rows)
    else:
        ids_r, kg_r = d.intern(key_rows)
        ids_f, kg_f, cols, nulls = d.intern_fields(packed, proj)
    assert np.array_equal(ids_f, ids_r) and np.array_equal(kg_f, kg_r)
    assert np.array_equal(kg_f, K.key_group_of_id(ids_f, MAXP))
    first = {}
    for r, i in zip(key_rows, ids_f.tolist()):
        assert first.setdefault(r, i) == i   # equal keys, one id
    assert len(set(first.values())) == len(first) == len(d)   # distinct keys, distinct ids
    assert np.array_equal(nulls[1], [recs[i][DBL] is None for i in pick])
    dev = torch.device("cuda", 0)
    tp = tuple(torch.from_numpy(x).to(dev) for x in packed)
    ids_d, kg_d, _, _ = d.intern_fields(tp, proj)
    assert ids_d.is_cuda and np.array_equal(to_host(ids_d), ids_f) and np.array_equal(to_host(kg_d), kg_f)
    # FG_ESTATE while an async intern is pending
    kp = tuple(torch.from_numpy(x.copy()).to(dev) for x in K.pack_key_rows(key_rows[:100]))
    d.intern_async(kp)
    for call in (lambda: d.intern_fields(tp, proj), lambda: d.project(tp, proj)):
        with pytest.raises(F.FlinkGpuError) as e:
            call()
        assert e.value.code == L.FG_ESTATE
    d.intern_wait()
    assert np.array_equal(to_host(d.intern_fields(tp, proj)[0]), ids_f)
    d.close()


def test_through_the_operator():
    """20,000 records over 500 distinct (STRING, INT) keys, TUMBLE 1 s, COUNT(*) / SUM / AVG of a
    DOUBLE with NULLs: records -> intern_fields -> device columns -> process_batch fires what
    host-built key rows + intern + the original columns fire"""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    n, nkeys, batch = 20_000, 500, 5_000
    keys = [(bytes(rng.integers(65, 91, int(rng.choice(STRING_LENGTHS)), dtype=np.uint8)), int(rng.integers(-50, 50)))
            for _ in range(nkeys)]
    keys = list(dict.fromkeys(keys))
    which = rng.integers(0, len(keys), n)
    ts = (1_000_000 + np.arange(n) // 4 + rng.integers(0, 1500, n)).astype(np.int64)
    val = rng.integers(0, 4000, n) / 4.0          # quarters: sums are exact in any order
    isnull = rng.random(n) < 0.1
    rows = [K.key_row([keys[k][0], int(t), keys[k][1], None if nl else float(v), b"filler-string", True], T6)
            for k, t, v, nl in zip(which, ts, val, isnull)]
    key_rows = [K.key_row(list(keys[k]), ["string", "int"]) for k in which]
    proj = K.RowProjection(6, [A, INT], ["string", "int"], col_fields=(BIG, DBL))

    def run(fields):
        d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=nkeys)
        op = F.WindowAggOperator(F.tumbling(1000), aggs=("count_star", "sum", "avg"), val_type="f64", expected_keys=nkeys)
        fired = []

        def take(r):
            if len(r):
                kr = d.lookup(r["key"])
                fired.extend((k, x.tobytes()[8:]) for k, x in zip(kr, r))
        for lo in range(0, n, batch):
            hi = lo + batch
            if fields:
                p = tuple(torch.from_numpy(x).to(dev) for x in pack(rows[lo:hi]))
                ids, _, cols, nulls = d.intern_fields(p, proj, key_groups=False)
                op.process_batch(ids, cols[0], cols[1].view(torch.float64), nulls[1])
            else:
                ids, _ = d.intern(key_rows[lo:hi])
                op.process_batch(ids, ts[lo:hi], np.where(isnull[lo:hi], 0.0, val[lo:hi]), isnull[lo:hi].astype(np.uint8))
            take(op.process_watermark(int(ts[hi - 1]) - 200))
        late = op.num_late_records_dropped
        take(op.process_watermark((1 << 63) - 1))
        op.close()
        d.close()
        return sorted(fired), late

    fired_a, late_a = run(True)
    fired_b, late_b = run(False)
    assert len(fired_b) > nkeys and late_b > 0   # the stream fires many windows and drops late records
    assert late_a == late_b
    assert fired_a == fired_b
    assert {k for k, _ in fired_b} <= set(key_rows)


def test_kernel_stats(pool):
    recs, rows, ref = pool
    parent = ["dict_probe", "dict_assign", "dict_rows", "dict_retain", "dict_rebuild"]   # the classes before dict_project
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=100)
    assert d.kernel_stats() == {}
    d.set_timing(True)
    ids, _ = d.intern(ref["a"][:100])
    d.rows(ids)
    assert list(d.kernel_stats()) == parent   # a dictionary that never projects
    packed = pack(rows[:700])
    d.project(packed, proj_of("b_a"))         # (a guess of 32 bytes per row and the retry at the exact size)
    st = d.kernel_stats()
    assert list(st) == parent + ["dict_project"]
    size = sum(len(r) for r in ref["b_a"][:700])
    assert size > 32 * 700                    # (so the call above was two projections)
    assert st["dict_project"]["launches"] == 2 and st["dict_project"]["records"] == 1400
    assert st["dict_project"]["rows"] == size and st["dict_project"]["total_ms"] > 0
    d.intern_fields(packed, proj_of("b_a"))
    st = d.kernel_stats()["dict_project"]
    assert (st["launches"], st["records"], st["rows"]) == (3, 2100, 2 * size)
    d.close()
