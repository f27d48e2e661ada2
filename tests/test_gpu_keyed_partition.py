"""fg_partition_keyed_by_owner against numpy: the sender half of the keyed two-phase edge. Rows
keyed by dictionary ids are grouped by owner (the key group an id carries, times parallelism over
max parallelism) and travel with their key rows: the reference for the owner is
key_group_of_id(id) * parallelism // max_parallelism, for the key rows KeyDictionary.lookup."""
import ctypes as C
import re
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCOLS = 7


def _rows(seed, n):
    """distinct key rows of mixed lengths: 0, 12 (padded to 16), 16, 32 and 48 bytes, one of 4 096"""
    from flink_amd.keys import key_row
    out = [b"", key_row(("x" * 4080,), ("string",))]
    assert len(out[1]) == 4096
    for i in range(n - 2):
        t = (seed + i) % 4
        if t == 0:
            out.append(struct.pack("<iii", seed, i, -i))                                   # 12
        elif t == 1:
            out.append(key_row((f"k{i:05d}",), ("string",)))                               # 16 (inline)
        elif t == 2:
            out.append(key_row((f"user{seed:04x}{i:04x}",), ("string",)))                  # 32
        else:
            out.append(key_row((f"a-rather-longer-key-{seed:04x}{i:05d}",), ("string",)))  # 48
    assert {len(r) for r in out} == {0, 12, 16, 32, 48, 4096}
    return out


class Dict:
    def __init__(self, maxp, seed, nkeys):
        from flink_amd.keys import KeyDictionary
        self.maxp = maxp
        self.kd = KeyDictionary(max_parallelism=maxp, expected_keys=nkeys)
        ids, _ = self.kd.intern(_rows(seed, nkeys))
        self.ids = np.asarray(ids, dtype=np.int64)
        self.row = dict(zip(self.ids.tolist(), self.kd.lookup(self.ids)))   # the reference, computed once


@pytest.fixture(scope="module")
def d128():
    d = Dict(128, 11, 300)
    yield d
    d.kd.close()


@pytest.fixture(scope="module")
def d120():
    d = Dict(120, 23, 300)
    yield d
    d.kd.close()


def _cols(ids, seed):
    """7 columns: the ids, then values that identify a row"""
    rng = np.random.default_rng(seed)
    n = len(ids)
    return [ids] + [rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64) for _ in range(NCOLS - 2)] + \
        [np.arange(n, dtype=np.int64)]


def _call(kd, cols, par, cap=None, fill=0xAB):
    """the C call on device copies of `cols`; cap=None: exactly what the rows take (a sizing call
    first); returns rc and the outputs as numpy arrays"""
    import torch

    from flink_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda", 0)
    n = len(cols[0])
    ins = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cols]
    outs = [torch.full((n,), -7, dtype=torch.int64, device=dev) for _ in cols]
    counts = torch.full((par,), -1, dtype=torch.int64, device=dev)
    bcounts = torch.full((par,), -1, dtype=torch.int64, device=dev)
    lens = torch.full((n,), -9, dtype=torch.int32, device=dev)
    pi = (C.c_void_p * len(cols))(*[t.data_ptr() for t in ins])
    po = (C.c_void_p * len(cols))(*[t.data_ptr() for t in outs])
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nbytes = C.c_int64(-1)

    def run(buf, cap_):
        return lib.fg_partition_keyed_by_owner(kd._h, s, n, len(cols), pi, par, po, C.c_void_p(counts.data_ptr()),
                                               C.c_void_p(lens.data_ptr()),
                                               C.c_void_p(buf.data_ptr() if buf is not None else None), cap_,
                                               C.c_void_p(bcounts.data_ptr()), C.byref(nbytes))
    if cap is None:
        rc = run(None, 0)   # the sizing call
        assert rc in (L.FG_OK, L.FG_EFULL), (rc, kd._lib.fg_key_dict_last_error(kd._h))
        assert (rc == L.FG_EFULL) == (nbytes.value > 0)
        cap = nbytes.value
    buf = torch.full((max(cap, 8),), fill, dtype=torch.uint8, device=dev)
    rc = run(buf, cap)
    torch.cuda.synchronize()
    return dict(rc=rc, msg=kd._lib.fg_key_dict_last_error(kd._h).decode(), outs=[t.cpu().numpy() for t in outs],
                counts=counts.cpu().numpy(), bcounts=bcounts.cpu().numpy(), lens=lens.cpu().numpy(),
                buf=buf.cpu().numpy(), nbytes=nbytes.value, cap=cap)


def _check(d, cols, par, r, bytes_written=True):
    from flink_amd.keys import key_group_of_id
    n = len(cols[0])
    owner = key_group_of_id(cols[0], d.maxp).astype(np.int64) * par // d.maxp
    rowlen = np.array([len(d.row[i]) for i in cols[0].tolist()], dtype=np.int64)
    padded = (rowlen + 7) & ~7
    assert np.array_equal(r["counts"], np.bincount(owner, minlength=par))
    assert np.array_equal(r["bcounts"], np.bincount(owner, weights=padded, minlength=par).astype(np.int64))
    assert r["nbytes"] == int(padded.sum())
    out = r["outs"]
    # position by position: the lengths and the bytes are those of the id at that position
    glen = np.array([len(d.row[i]) for i in out[0].tolist()], dtype=np.int64)
    assert np.array_equal(r["lens"], glen)
    gpad = (glen + 7) & ~7
    pref = np.cumsum(gpad) - gpad
    if bytes_written:
        raw = r["buf"][:r["nbytes"]].tobytes()
        for i, (o, ln, pd) in enumerate(zip(pref.tolist(), glen.tolist(), gpad.tolist())):
            assert raw[o:o + ln] == d.row[int(out[0][i])], i
            assert raw[o + ln:o + pd] == b"\0" * (pd - ln), i
    # per owner: its run holds exactly its rows (columns and key row), in any order
    ends = np.cumsum(r["counts"])
    tuples = lambda cs, idx: sorted(tuple(int(c[i]) for c in cs) for i in idx)
    for p in range(par):
        a, b = int(ends[p] - r["counts"][p]), int(ends[p])
        assert tuples(out, range(a, b)) == tuples(cols, np.nonzero(owner == p)[0].tolist()), p
    assert int(ends[-1]) == n


@pytest.mark.parametrize("par", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 257, 20_000])
def test_partition_matches_numpy_at_max_parallelism_128(d128, par, n):
    from flink_amd import _lib as L
    rng = np.random.default_rng(1000 * par + n)
    ids = d128.ids[rng.integers(0, len(d128.ids), n)] if n != 1 else d128.ids[1:2]   # (n = 1: the 4 096-byte row)
    cols = _cols(ids, n + par)
    r = _call(d128.kd, cols, par)
    assert r["rc"] == L.FG_OK, r["msg"]
    if n == 0:
        assert r["nbytes"] == 0 and not r["counts"].any() and not r["bcounts"].any()
        return
    if n == 20_000:
        assert len(np.unique(ids)) < n   # repeated ids: a key in several rows
    _check(d128, cols, par, r)


def test_partition_at_max_parallelism_120(d120):
    from flink_amd import _lib as L
    ids = d120.ids[np.random.default_rng(5).integers(0, len(d120.ids), 5000)]
    cols = _cols(ids, 6)
    r = _call(d120.kd, cols, 3)
    assert r["rc"] == L.FG_OK, r["msg"]
    _check(d120, cols, 3, r)


def test_an_owner_without_rows(d128):
    from flink_amd import _lib as L
    ids = d128.ids[2:7][np.random.default_rng(9).integers(0, 5, 700)]   # 5 keys, 8 owners
    cols = _cols(ids, 10)
    r = _call(d128.kd, cols, 8)
    assert r["rc"] == L.FG_OK, r["msg"]
    assert (r["counts"] == 0).any() and (r["bcounts"][r["counts"] == 0] == 0).all()
    _check(d128, cols, 8, r)


def test_python_wrapper_retries_once_on_efull(d128):
    import torch

    from flink_amd.exchange import partition_keyed_by_owner
    ids = np.concatenate([d128.ids[1:2], d128.ids[:40]])   # the 4 096-byte row: more than 32 B per row
    cols = _cols(ids, 12)
    dev = torch.device("cuda", 0)
    outs, counts, lens, buf, bcounts = partition_keyed_by_owner([torch.from_numpy(c).to(dev) for c in cols], d128.kd, 3)
    r = dict(outs=[o.cpu().numpy() for o in outs], counts=counts.cpu().numpy(), lens=lens.cpu().numpy(),
             buf=buf.cpu().numpy(), bcounts=bcounts.cpu().numpy(), nbytes=buf.numel())
    assert buf.numel() > 32 * len(ids)
    _check(d128, cols, 3, r)


def test_efull_leaves_the_bytes_untouched_and_the_rest_complete(d128):
    from flink_amd import _lib as L
    ids = d128.ids[np.random.default_rng(3).integers(0, len(d128.ids), 257)]
    cols = _cols(ids, 4)
    full = _call(d128.kd, cols, 3)
    assert full["rc"] == L.FG_OK
    r = _call(d128.kd, cols, 3, cap=full["nbytes"] - 8, fill=0xCD)
    assert r["rc"] == L.FG_EFULL, (r["rc"], r["msg"])
    assert (r["buf"] == 0xCD).all()
    _check(d128, cols, 3, r, bytes_written=False)
    again = _call(d128.kd, cols, 3, cap=r["nbytes"])   # a retry at *out_nbytes succeeds
    assert again["rc"] == L.FG_OK
    _check(d128, cols, 3, again)


def test_unknown_and_negative_ids_are_einval_and_the_dictionary_stays_usable(d128):
    from flink_amd import _lib as L
    size = len(d128.kd)
    ids = d128.ids[np.random.default_rng(4).integers(0, len(d128.ids), 1000)].copy()
    ids[[17, 400]] = ((size + 5) << 7) | 3      # an ordinal past fg_key_dict_size
    ids[900] = -12                              # a negative id
    cols = _cols(ids, 5)
    r = _call(d128.kd, cols, 2, cap=1 << 20, fill=0xEE)
    assert r["rc"] == L.FG_EINVAL, (r["rc"], r["msg"])
    m = re.search(r"(\d+) unknown ids.*grouped index (\d+)", r["msg"])
    assert m, r["msg"]
    known = np.isin(r["outs"][0], d128.ids)
    assert int(m.group(1)) == 3 == int((~known).sum())
    assert int(m.group(2)) == int(np.nonzero(~known)[0][0])
    assert (r["buf"] == 0xEE).all()             # no key byte is written
    assert len(d128.kd) == size
    good = _cols(d128.ids[:100].copy(), 6)
    r2 = _call(d128.kd, good, 2)
    assert r2["rc"] == L.FG_OK
    _check(d128, good, 2, r2)


def test_a_pending_async_intern_is_estate(d128):
    import torch

    from flink_amd import _lib as L
    from flink_amd.keys import pack_key_rows
    dev = torch.device("cuda", 0)
    packed = tuple(torch.from_numpy(np.array(a)).to(dev) for a in pack_key_rows(_rows(11, 50)))
    size = len(d128.kd)
    d128.kd.intern_async(packed)
    try:
        r = _call(d128.kd, _cols(d128.ids[:10].copy(), 1), 2, cap=1 << 16)
        assert r["rc"] == L.FG_ESTATE, (r["rc"], r["msg"])
    finally:
        d128.kd.intern_wait()
    assert len(d128.kd) == size   # (rows it already held)
    cols = _cols(d128.ids[:10].copy(), 1)
    r = _call(d128.kd, cols, 2)
    assert r["rc"] == L.FG_OK
    _check(d128, cols, 2, r)


def test_argument_checks_come_before_device_work(d128):
    from flink_amd import _lib as L
    cols = _cols(d128.ids[:4].copy(), 2)
    assert _call(d128.kd, cols, 129, cap=64)["rc"] == L.FG_EINVAL    # parallelism above the max parallelism
    assert _call(d128.kd, cols, 0, cap=64)["rc"] == L.FG_EINVAL
    assert _call(d128.kd, cols + cols[:2], 2, cap=64)["rc"] == L.FG_EINVAL   # 9 columns
