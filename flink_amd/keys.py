"""Grouping keys of any type: the GPU key dictionary (fg_key_dict_* of include/flinkgpu.h).

The reference aggregates by the BinaryRowData key row its key selector projects
(TR/keyselector/BinaryRowDataKeySelector.java:43-50): a STRING key, or several key columns,
is one serialized row, equal keys are byte-equal rows (BinarySection.equals,
TC/data/binary/BinarySection.java:62-73) and the key group is
murmurHash(hashBytesByWords(row)) % maxParallelism (BinarySection.hashCode :76-78,
KeyGroupRangeAssignment.java:63-77). `KeyDictionary.intern` maps such rows to 64-bit ids on the
GPU (equal rows -> equal ids, exact), which the window operators aggregate as BIGINT keys;
`retain` keeps the ids that still hold state and retires the rest (their ordinals are reused);
`rows` gathers the packed key rows of ids on the GPU (fired rows, checkpoints; `lookup` is its
list-of-bytes form) and `reintern` carries ids from one dictionary into another (rescale).
`project` / `intern_fields` are the key selector itself on the GPU: packed BinaryRowData records
in, their key rows (or ids) and the rowtime / value columns out (`RowProjection` says which fields;
`project_key_row` is the pure-Python reference of one row).
`key_row` / `decode_key_row` write and read key rows the way BinaryRowWriter does (writer/BinaryRowWriter.java, AbstractBinaryWriter.java:
81-105,280-330: STRING of <= 7 bytes inline in its 8-byte slot as 0x80|len in the top byte,
longer ones in the variable part, 8-byte aligned, the slot holding offset << 32 | length).
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import _lib as L
from .rows import HEADER_SIZE_IN_BITS, bit_set_width

def dict_kg_bits(max_parallelism: int) -> int:
    """Bits of the key group in a dictionary id: ceil(log2(max parallelism)) (fg_window.h)."""
    b = 0
    while b < 31 and (1 << b) < max_parallelism:
        b += 1
    return b


def key_row(fields, types, row_kind: int = 0) -> bytes:
    """One BinaryRowData key row. types[i] in {"string", "bigint", "int", "double", "boolean", "float",
    "smallint", "tinyint"}; a None field is NULL (null bit set, slot zero: BinaryRowWriter.setNullAt)."""
    arity = len(fields)
    w = bit_set_width(arity)
    fixed = bytearray(w + 8 * arity)
    fixed[0] = row_kind
    var = bytearray()
    for f, (v, t) in enumerate(zip(fields, types)):
        slot = w + 8 * f
        if v is None:
            b = HEADER_SIZE_IN_BITS + f
            fixed[b >> 3] |= 1 << (b & 7)
            continue
        if t == "string":
            data = v.encode("utf-8") if isinstance(v, str) else bytes(v)
            if len(data) <= 7:   # writeBytesToFixLenPart: 0x80 | len in the top byte, data LE
                word = (0x80 | len(data)) << 56 | int.from_bytes(data, "little")
                fixed[slot:slot + 8] = word.to_bytes(8, "little")
            else:                # writeBytesToVarLenPart: offset << 32 | len, padded to 8 bytes
                off = len(fixed) + len(var)
                fixed[slot:slot + 8] = (off << 32 | len(data)).to_bytes(8, "little")
                var += data + b"\0" * (-len(data) % 8)
        elif t == "bigint":
            fixed[slot:slot + 8] = struct.pack("<q", int(v))
        elif t == "int":
            fixed[slot:slot + 4] = struct.pack("<i", int(v))
        elif t == "double":
            fixed[slot:slot + 8] = struct.pack("<d", float(v))
        elif t == "boolean":
            fixed[slot] = 1 if v else 0
        elif t == "float":
            fixed[slot:slot + 4] = struct.pack("<f", float(v))
        elif t == "smallint":
            fixed[slot:slot + 2] = struct.pack("<h", int(v))
        elif t == "tinyint":
            fixed[slot:slot + 1] = struct.pack("<b", int(v))
        else:
            raise ValueError(f"unsupported key field type {t!r}")
    return bytes(fixed + var)


def decode_key_row(row: bytes, types):
    """Fields of a key row written by key_row (None for NULL)."""
    arity = len(types)
    w = bit_set_width(arity)
    out = []
    for f, t in enumerate(types):
        b = HEADER_SIZE_IN_BITS + f
        if row[b >> 3] >> (b & 7) & 1:
            out.append(None)
            continue
        slot = row[w + 8 * f: w + 8 * f + 8]
        word = int.from_bytes(slot, "little")
        if t == "string":
            if word >> 63:
                n = (word >> 56) & 0x7F
                out.append(slot[:n].decode("utf-8"))
            else:
                off, n = word >> 32, word & 0xFFFFFFFF
                out.append(row[off:off + n].decode("utf-8"))
        elif t == "bigint":
            out.append(struct.unpack("<q", slot)[0])
        elif t == "int":
            out.append(struct.unpack("<i", slot[:4])[0])
        elif t == "double":
            out.append(struct.unpack("<d", slot)[0])
        elif t == "boolean":
            out.append(bool(slot[0]))
        elif t == "float":
            out.append(struct.unpack("<f", slot[:4])[0])
        elif t == "smallint":
            out.append(struct.unpack("<h", slot[:2])[0])
        elif t == "tinyint":
            out.append(struct.unpack("<b", slot[:1])[0])
    return tuple(out)


_KIND_OF_TYPE = {"string": L.FIELD_VAR, "bigint": L.FIELD_FIX8, "double": L.FIELD_FIX8, "int": L.FIELD_FIX4,
                 "float": L.FIELD_FIX4, "smallint": L.FIELD_FIX2, "tinyint": L.FIELD_FIX1, "boolean": L.FIELD_FIX1}
_TYPE_OF_KIND = {L.FIELD_VAR: "string", L.FIELD_FIX8: "bigint", L.FIELD_FIX4: "int", L.FIELD_FIX2: "smallint",
                 L.FIELD_FIX1: "tinyint"}


class RowProjection:
    """fg_row_projection: which fields of an input row of `arity` fields make its key row
    (key_fields, in key order; key_kinds their fg_field_kind -- L.FIELD_* or a key_row type name)
    and which 8-byte fields come out as columns (col_fields: rowtime, value)."""

    def __init__(self, arity, key_fields, key_kinds, col_fields=()):
        self.arity = int(arity)
        self.key_fields = tuple(int(f) for f in key_fields)
        self.key_kinds = tuple(_KIND_OF_TYPE[k] if isinstance(k, str) else int(k) for k in key_kinds)
        self.col_fields = tuple(int(f) for f in col_fields)
        if len(self.key_fields) != len(self.key_kinds):
            raise ValueError("one kind per key field expected")
        if len(self.key_fields) > L.PROJ_MAX_KEY_FIELDS or len(self.col_fields) > L.PROJ_MAX_COLS:
            raise ValueError(f"at most {L.PROJ_MAX_KEY_FIELDS} key fields and {L.PROJ_MAX_COLS} columns")

    def struct(self) -> "L.FgRowProjection":
        p = L.FgRowProjection()
        p.arity = self.arity
        p.n_key_fields = len(self.key_fields)
        p.n_cols = len(self.col_fields)
        for f, (field, kind) in enumerate(zip(self.key_fields, self.key_kinds)):
            p.key_field[f] = field
            p.key_kind[f] = kind
        for c, field in enumerate(self.col_fields):
            p.col_field[c] = field
        return p


def project_key_row(row: bytes, proj: RowProjection) -> bytes:
    """The key row fg_key_dict_project writes for one input row (a pure-Python reference): the key
    fields decoded by the rules of include/flinkgpu.h and written with key_row. A bad row raises
    ValueError."""
    w = bit_set_width(proj.arity)
    fixed = w + 8 * proj.arity
    if len(row) % 8 or len(row) < fixed:
        raise ValueError("a row shorter than its fixed-length part, or not a multiple of 8 bytes")
    fields, types = [], []
    for field, kind in zip(proj.key_fields, proj.key_kinds):
        types.append(_TYPE_OF_KIND[kind])
        b = HEADER_SIZE_IN_BITS + field
        if row[b >> 3] >> (b & 7) & 1:
            fields.append(None)
            continue
        slot = row[w + 8 * field: w + 8 * field + 8]
        word = int.from_bytes(slot, "little")
        if kind != L.FIELD_VAR:
            fields.append(int.from_bytes(slot[:kind], "little", signed=True))
        elif word >> 63:
            n = (word >> 56) & 0x7F
            if n > 7:
                raise ValueError("an inline field longer than 7 bytes")
            fields.append(slot[:n])
        else:
            off, n = word >> 32, word & 0xFFFFFFFF
            if off % 8 or off < fixed or off + n > len(row):
                raise ValueError("a variable-length field outside its row")
            fields.append(row[off:off + n])
    out = key_row(fields, types)
    if len(out) > (1 << 24) - 4:
        raise ValueError("a key row above 2^24 - 4 bytes")
    return out


def pack_key_rows(rows):
    """(bytes uint8[], offsets int64[], lengths int32[]) of a list of key rows (8-byte aligned)."""
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    pad = (-lens) % 8
    offs = np.zeros(len(rows), dtype=np.int64)
    if len(rows) > 1:
        offs[1:] = np.cumsum((lens + pad)[:-1], dtype=np.int64)
    buf = bytearray()
    for r, p in zip(rows, pad):
        buf += r + b"\0" * int(p)
    return np.frombuffer(bytes(buf) or b"\0" * 8, dtype=np.uint8), offs, lens


def key_group_of_id(ids, max_parallelism: int = 128):
    """Key group carried by a dictionary id (FG_KEYHASH_DICT_ID)."""
    mask = np.uint64((1 << dict_kg_bits(max_parallelism)) - 1)   # id = ordinal << kg_bits | key group
    return (np.asarray(ids, dtype=np.int64).view(np.uint64) & mask).astype(np.int32) % max_parallelism


def binaryrow_hash(row: bytes) -> int:
    """BinarySection.hashCode of one row, computed by the library (no device needed)."""
    lib = L.load()
    buf = (C.c_uint8 * max(len(row), 1)).from_buffer_copy(row or b"\0")
    return int(lib.fg_binaryrow_hash(buf, len(row)))


class KeyDictionary:
    """GPU-resident dictionary of key rows -> 64-bit ids (fg_key_dict)."""

    def __init__(self, max_parallelism: int = 128, expected_keys: int = 0, device: int = 0):
        lib = L.load()
        self._lib = lib
        self.max_parallelism = max_parallelism
        h = C.c_void_p()
        rc = lib.fg_key_dict_open(device, max_parallelism, expected_keys, C.byref(h))
        if rc != L.FG_OK:
            raise L.FlinkGpuError(rc, "fg_key_dict_open failed (no usable device?)")
        self._h = h

    def _check(self, rc):
        if rc == L.FG_OK:
            return
        msg = self._lib.fg_key_dict_last_error(self._h).decode(errors="replace")
        if rc == L.FG_EINVAL:
            raise L.WindowSpecError(msg)
        raise L.FlinkGpuError(rc, msg)

    def intern_async(self, packed, key_groups=False):
        """fg_key_dict_intern_async of device rows packed=(bytes u8, offsets i64, lengths i32
        tensors): the lookup is launched on the dictionary's stream and (ids, key_groups) tensors
        are returned at once -- complete after intern_wait(). The packed tensors must stay alive
        until then."""
        import torch
        buf, off, ln = packed
        n = len(off)
        ext = self.__dict__.get("_ext_stream")
        if ext is None or ext.device != buf.device:
            ext = self._ext_stream = torch.cuda.ExternalStream(self._lib.fg_key_dict_stream(self._h), device=buf.device)
        ext.wait_stream(torch.cuda.current_stream(buf.device))
        ids = torch.empty(n, dtype=torch.int64, device=buf.device)
        kg = torch.empty(n, dtype=torch.int32, device=buf.device) if key_groups else None
        self._pending = (buf, off, ln, ids, kg)
        self._check(self._lib.fg_key_dict_intern_async(self._h, n, C.c_void_p(buf.data_ptr()), buf.numel(),
                                                       C.c_void_p(off.data_ptr()), C.c_void_p(ln.data_ptr()),
                                                       C.c_void_p(ids.data_ptr()),
                                                       C.c_void_p(kg.data_ptr() if key_groups else None)))
        return ids, kg

    def intern_wait(self):
        """fg_key_dict_intern_wait: the pending intern_async's ids (and key groups) complete"""
        rc = self._lib.fg_key_dict_intern_wait(self._h)
        self._pending = None
        self._check(rc)

    def intern(self, rows=None, packed=None, key_groups=True):
        """rows: list of key-row bytes, or packed=(bytes u8[], offsets i64[], lengths i32[]) on the
        host (numpy) or the device (torch tensors). Returns (ids, key_groups) of the same kind
        (key_groups None when not asked for: an id carries its key group, FG_KEYHASH_DICT_ID)."""
        if packed is None:
            packed = pack_key_rows(rows)
        buf, off, ln = packed
        n = len(off)
        if hasattr(buf, "data_ptr"):   # torch device tensors
            import torch
            # the dictionary reads them on its own stream: order it after their producers
            ext = self.__dict__.get("_ext_stream")
            if ext is None or ext.device != buf.device:
                ext = self._ext_stream = torch.cuda.ExternalStream(self._lib.fg_key_dict_stream(self._h),
                                                                   device=buf.device)
            ext.wait_stream(torch.cuda.current_stream(buf.device))
            ids = torch.empty(n, dtype=torch.int64, device=buf.device)
            kg = torch.empty(n, dtype=torch.int32, device=buf.device) if key_groups else None
            self._check(self._lib.fg_key_dict_intern(self._h, L.DEVICE, n, C.c_void_p(buf.data_ptr()), buf.numel(),
                                                     C.c_void_p(off.data_ptr()), C.c_void_p(ln.data_ptr()),
                                                     C.c_void_p(ids.data_ptr()),
                                                     C.c_void_p(kg.data_ptr() if key_groups else None)))
            return ids, kg
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        ln = np.ascontiguousarray(ln, dtype=np.int32)
        ids = np.empty(n, dtype=np.int64)
        kg = np.empty(n, dtype=np.int32) if key_groups else None
        self._check(self._lib.fg_key_dict_intern(self._h, L.HOST, n, buf.ctypes.data, buf.size, off.ctypes.data,
                                                 ln.ctypes.data, ids.ctypes.data,
                                                 C.c_void_p(kg.ctypes.data if key_groups else None)))
        return ids, kg

    def intern_rows(self, data, offsets, lengths):
        """ids (device int64 tensor) of the key rows in device tensors: data uint8, offsets
        int64, lengths int32 (flink_amd.exchange's receiving side of key rows)."""
        ids, _ = self.intern(packed=(data, offsets, lengths), key_groups=False)
        return ids

    def locate(self, ids):
        """Where the key rows of device ids live: (word offsets int64, words int64, arena) with
        arena an int32 device tensor view of the dictionary's arena (valid until the next
        intern on this dictionary); row i = arena[woff[i] : woff[i] + nw[i]]."""
        import torch
        n = ids.numel()
        off = torch.empty(n, dtype=torch.int64, device=ids.device)
        ln = torch.empty(n, dtype=torch.int32, device=ids.device)
        if n:
            ext = self.__dict__.get("_ext_stream")
            if ext is None or ext.device != ids.device:
                ext = self._ext_stream = torch.cuda.ExternalStream(self._lib.fg_key_dict_stream(self._h),
                                                                   device=ids.device)
            ext.wait_stream(torch.cuda.current_stream(ids.device))
            self._check(self._lib.fg_key_dict_lookup(self._h, L.DEVICE, n, C.c_void_p(ids.data_ptr()),
                                                     C.c_void_p(off.data_ptr()), C.c_void_p(ln.data_ptr())))
            if bool((ln < 0).any()):
                raise KeyError("unknown dictionary id in locate()")
        p = C.c_void_p()
        size = C.c_int64()
        self._check(self._lib.fg_key_dict_arena(self._h, C.byref(p), C.byref(size)))

        class _Arena:   # zero-copy view for torch.as_tensor
            __cuda_array_interface__ = {"shape": (max(int(size.value) // 4, 1),), "typestr": "<i4",
                                        "data": (int(p.value or 0), False), "version": 2}
        arena = torch.as_tensor(_Arena(), device=ids.device)
        return off // 4, (ln // 4).to(torch.int64), arena

    def rows(self, ids):
        """fg_key_dict_rows: the key rows of the ids, packed in their order the way pack_key_rows
        packs them: (bytes u8[nbytes], offsets i64[n + 1], lengths i32[n]); row i is
        bytes[offsets[i] : offsets[i] + lengths[i]], padded with zeros to 8 bytes. Numpy ids give
        numpy arrays; a torch device tensor gives device tensors (no key byte touches the host).
        At most two C calls: a guess of 32 bytes per row, one retry at the exact size if the rows
        take more. Unknown ids raise KeyError."""
        dev = hasattr(ids, "data_ptr")
        if dev:
            import torch
            ids = ids.to(torch.int64).contiguous()
            n = ids.numel()
            ext = self.__dict__.get("_ext_stream")
            if ext is None or ext.device != ids.device:
                ext = self._ext_stream = torch.cuda.ExternalStream(self._lib.fg_key_dict_stream(self._h),
                                                                   device=ids.device)
            ext.wait_stream(torch.cuda.current_stream(ids.device))   # the ids' producer first
            off = torch.empty(n + 1, dtype=torch.int64, device=ids.device)
            ln = torch.empty(n, dtype=torch.int32, device=ids.device)
            alloc = lambda cap: torch.empty(cap, dtype=torch.uint8, device=ids.device)   # noqa: E731
            ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
            if n == 0:
                off.zero_()
        else:
            ids = np.ascontiguousarray(ids, dtype=np.int64)
            n = len(ids)
            off = np.zeros(n + 1, dtype=np.int64)
            ln = np.empty(n, dtype=np.int32)
            alloc = lambda cap: np.empty(cap, dtype=np.uint8)   # noqa: E731
            ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        if n == 0:
            return alloc(0), off, ln
        nbytes = C.c_int64()
        cap = 32 * n
        for _ in range(2):
            buf = alloc(max(cap, 8))
            rc = self._lib.fg_key_dict_rows(self._h, L.DEVICE if dev else L.HOST, n, ptr(ids), ptr(buf), cap, ptr(off),
                                            ptr(ln), C.byref(nbytes))
            if rc != L.FG_EFULL:
                break
            cap = int(nbytes.value)
        if rc == L.FG_EINVAL:   # (the arguments above are well formed: an unknown id)
            raise KeyError(self._lib.fg_key_dict_last_error(self._h).decode(errors="replace"))
        self._check(rc)
        return buf[:int(nbytes.value)], off, ln

    def _records(self, packed_rows, proj):
        """the inputs of project / intern_fields: (device?, n, records, struct, ptr, alloc, out_cols,
        out_nulls, their pointer arrays); device records order the dictionary's stream after their
        producer"""
        buf, off, ln = packed_rows
        dev = hasattr(buf, "data_ptr")
        if dev:
            import torch
            buf, off, ln = buf.contiguous(), off.to(torch.int64).contiguous(), ln.to(torch.int32).contiguous()
            ext = self.__dict__.get("_ext_stream")
            if ext is None or ext.device != buf.device:
                ext = self._ext_stream = torch.cuda.ExternalStream(self._lib.fg_key_dict_stream(self._h),
                                                                   device=buf.device)
            ext.wait_stream(torch.cuda.current_stream(buf.device))
            kinds = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}
            alloc = lambda m, kind: torch.empty(m, dtype=kinds[kind], device=buf.device)   # noqa: E731
            ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
            nbytes = buf.numel()
        else:
            buf = np.ascontiguousarray(buf, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.int64)
            ln = np.ascontiguousarray(ln, dtype=np.int32)
            kinds = {"u8": np.uint8, "i32": np.int32, "i64": np.int64}
            alloc = lambda m, kind: np.empty(m, dtype=kinds[kind])   # noqa: E731
            ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
            nbytes = buf.size
        n = len(ln)
        cols = [alloc(n, "i64") for _ in proj.col_fields]
        nulls = [alloc(n, "u8") for _ in proj.col_fields]
        k = max(len(cols), 1)
        pc = (C.c_void_p * k)(*[ptr(c) for c in cols])
        pn = (C.c_void_p * k)(*[ptr(c) for c in nulls])
        return dev, n, (buf, nbytes, off, ln), proj.struct(), ptr, alloc, cols, nulls, pc, pn

    def project(self, packed_rows, proj: RowProjection):
        """fg_key_dict_project: the key rows of packed BinaryRowData records packed_rows=(bytes u8[],
        offsets i64[n], lengths i32[n]), projected on the GPU: (bytes u8[nbytes], offsets i64[n + 1],
        lengths i32[n], cols, col_nulls) -- the key rows in the layout intern() reads, and per
        proj.col_fields an int64 column and its uint8 NULL column. Numpy in gives numpy out; device
        tensors in give device tensors out (no byte touches the host). At most two C calls: a guess
        of 32 bytes per key row, one retry at the exact size. A bad row raises WindowSpecError."""
        dev, n, (buf, nbytes, off, ln), ps, ptr, alloc, cols, nulls, pc, pn = self._records(packed_rows, proj)
        koff = alloc(n + 1, "i64")
        klen = alloc(n, "i32")
        if n == 0:
            koff[:] = 0
            return alloc(0, "u8"), koff, klen, cols, nulls
        total = C.c_int64()
        cap = 32 * n
        for _ in range(2):
            kbuf = alloc(max(cap, 8), "u8")
            rc = self._lib.fg_key_dict_project(self._h, L.DEVICE if dev else L.HOST, n, ptr(buf), nbytes, ptr(off), ptr(ln),
                                               C.byref(ps), ptr(kbuf), cap, ptr(koff), ptr(klen), pc, pn, C.byref(total))
            if rc != L.FG_EFULL:
                break
            cap = int(total.value)
        self._check(rc)
        return kbuf[:int(total.value)], koff, klen, cols, nulls

    def intern_fields(self, packed_rows, proj: RowProjection, key_groups=True):
        """fg_key_dict_intern_fields: records in, ids out -- project() into the dictionary's device
        scratch and intern() of those key rows in one call: (ids i64[n], key_groups i32[n] or None,
        cols, col_nulls), numpy or device tensors like the input."""
        dev, n, (buf, nbytes, off, ln), ps, ptr, alloc, cols, nulls, pc, pn = self._records(packed_rows, proj)
        ids = alloc(n, "i64")
        kg = alloc(n, "i32") if key_groups else None
        self._check(self._lib.fg_key_dict_intern_fields(self._h, L.DEVICE if dev else L.HOST, n, ptr(buf), nbytes, ptr(off),
                                                        ptr(ln), C.byref(ps), ptr(ids),
                                                        ptr(kg) if key_groups else None, pc, pn))
        return ids, kg, cols, nulls

    def lookup(self, ids):
        """Key rows (bytes) of the ids (host)."""
        buf, off, ln = self.rows(np.ascontiguousarray(ids, dtype=np.int64))
        raw = buf.tobytes()
        return [raw[o:o + n_] for o, n_ in zip(off[:-1].tolist(), ln.tolist())]

    @staticmethod
    def _stats_dict(st) -> dict:
        return {f: int(getattr(st, f)) for f, _ in L.FgKeyDictStats._fields_ if f != "reserved0"}

    def stats(self) -> dict:
        """fg_key_dict_get_stats: live, issued, free_ordinals, arena_bytes, table_slots, side_rows,
        retired_total."""
        st = L.FgKeyDictStats()
        self._check(self._lib.fg_key_dict_get_stats(self._h, C.byref(st)))
        return self._stats_dict(st)

    def retain(self, *id_arrays) -> dict:
        """fg_key_dict_retain: keep exactly the ids of the given arrays (numpy arrays, or torch
        tensors on the device -- one kind per call; up to 16, e.g. the key column of every handle's
        state image), retire every other entry and reuse its ordinal for later interns. No array
        empties the dictionary. Returns the stats after the call. After it the caller must hold no
        id outside the arrays; an id that names no live entry raises (the dictionary unchanged)."""
        dev = any(hasattr(a, "data_ptr") for a in id_arrays)
        if dev:
            import torch
            if not all(hasattr(a, "data_ptr") for a in id_arrays):
                raise TypeError("retain: numpy arrays or device tensors, not both")
            arrs = [a.to(torch.int64).contiguous() for a in id_arrays]
            for a in arrs:
                if a.numel():
                    ext = self.__dict__.get("_ext_stream")
                    if ext is None or ext.device != a.device:
                        ext = self._ext_stream = torch.cuda.ExternalStream(self._lib.fg_key_dict_stream(self._h),
                                                                           device=a.device)
                    ext.wait_stream(torch.cuda.current_stream(a.device))   # the ids' producer first
            ptrs = [a.data_ptr() for a in arrs]
            counts = [a.numel() for a in arrs]
        else:
            arrs = [np.ascontiguousarray(a, dtype=np.int64).reshape(-1) for a in id_arrays]
            ptrs = [a.ctypes.data for a in arrs]
            counts = [a.size for a in arrs]
        k = len(arrs)
        pa = (C.c_void_p * max(k, 1))(*ptrs)
        ca = (C.c_int64 * max(k, 1))(*counts)
        st = L.FgKeyDictStats()
        self._check(self._lib.fg_key_dict_retain(self._h, L.DEVICE if dev else L.HOST, k, pa, ca, C.byref(st)))
        return self._stats_dict(st)

    def set_timing(self, on: bool = True):
        """HIP-event timing of the dictionary's kernels (kernel_stats)."""
        self._check(self._lib.fg_key_dict_set_timing(self._h, 1 if on else 0))

    def kernel_stats(self) -> dict:
        """{"dict_probe" | "dict_assign" | "dict_rows" | "dict_retain" | "dict_rebuild": dict(launches,
        total_ms, records, rows)}, and "dict_project" once the dictionary has projected."""
        arr = (L.FgKernelStat * 8)()
        n = C.c_int32()
        self._check(self._lib.fg_key_dict_kernel_stats(self._h, arr, 8, C.byref(n)))
        return {arr[i].name.decode(): dict(launches=arr[i].launches, total_ms=arr[i].total_ms,
                                           records=arr[i].records, rows=arr[i].rows) for i in range(n.value)}

    def __len__(self):
        return int(self._lib.fg_key_dict_size(self._h))

    def close(self):
        if self._h:
            self._lib.fg_key_dict_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def reintern(ids, src: KeyDictionary, dst: KeyDictionary):
    """The ids in `dst` of the key rows that `ids` name in `src`: src.rows(ids) interned by dst,
    device to device when `ids` is a device tensor. Ids of one subtask's dictionary mean nothing
    to another's, so a rescaled subtask maps the key column of every old subtask's image into its
    own dictionary before restore_state_range(..., key_hash=KEYHASH_DICT_ID)."""
    buf, off, ln = src.rows(ids)
    if len(buf) == 0:   # (only empty rows, or none: the intern still wants a buffer to point at)
        buf = buf.new_zeros(8) if hasattr(buf, "data_ptr") else np.zeros(8, dtype=np.uint8)
    new_ids, _ = dst.intern(packed=(buf, off[:-1], ln), key_groups=False)
    return new_ids
