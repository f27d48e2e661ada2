"""CPU-side checks of selective snapshot images (fg_snapshot_plan, fg_snapshot_state_select[_async]):
the C-ABI is exported, bound and documented with ABI 16 unchanged, and the shim's policy
(keyed_state.wanted_slices / write_delta) leaves the backend as write_image leaves it when fed the
full image -- on a pure-numpy model of the engine's resident slices, no GPU."""
import ctypes as C

import numpy as np
import pytest

from flink_amd import _lib as L
from flink_amd.keyed_state import CUMULATE, HOP, TUMBLE, SliceSpec, WindowAggsState
from tests.test_abi import HEADER, declared_symbols

NEW = ("fg_snapshot_plan", "fg_snapshot_state_select_async", "fg_snapshot_state_select")


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for s in NEW:
        assert s in L.EXPORTS and s in declared_symbols(), s
        assert hasattr(lib, s), s
        assert getattr(lib, s).restype is C.c_int, s
    assert list(lib.fg_snapshot_plan.argtypes) == [C.c_void_p, C.POINTER(L.FgImageSlices), C.POINTER(C.c_int64)]
    assert list(lib.fg_snapshot_state_select_async.argtypes) == [C.c_void_p, C.c_void_p, C.c_int64]
    assert list(lib.fg_snapshot_state_select.argtypes) == [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(L.FgStateRows),
                                                           C.POINTER(C.c_int64)]
    assert lib.fg_abi_version() == 16


def test_null_handles_are_refused():
    lib = L.load()
    assert lib.fg_snapshot_plan(None, C.byref(L.FgImageSlices()), None) == L.FG_EINVAL
    assert lib.fg_snapshot_state_select_async(None, None, 0) == L.FG_EINVAL
    assert lib.fg_snapshot_state_select(None, None, 0, C.byref(L.FgStateRows()), None) == L.FG_EINVAL


def test_header_documents_them():
    src = open(HEADER).read()
    doc = src[src.index("Selective images (ABI 16, added)"):src.index("int  fg_snapshot_plan")]
    for word in NEW + ("FG_ESTATE", "FG_EINVAL", "fg_get_stats", "consumes", "2^32", "cnt_val", "all-zero mask",
                       "fg_snapshot_key_groups", "left out"):
        assert word in doc, word
    assert "#define FG_ABI_VERSION 16" in src


def test_operator_methods_exist():
    from flink_amd import WindowAggOperator
    for m in ("snapshot_plan", "snapshot_state_select", "snapshot_state_select_async"):
        assert callable(getattr(WindowAggOperator, m)), m


# ---- the policy on synthetic images ---------------------------------------------------------------

class Engine:
    """numpy model of the engine's resident state: slice -> {key: acc}, a changed flag per slice"""

    def __init__(self):
        self.slices: dict[int, dict[int, list]] = {}
        self.changed: dict[int, bool] = {}

    def add(self, slice_end, keys, v=1):
        t = self.slices.setdefault(slice_end, {})
        for k in keys:
            a = t.setdefault(int(k), [0, 0, 0, (1 << 63) - 1, -(1 << 63)])
            a[0] += 1
            a[1] += 1
            a[2] += v
            a[3], a[4] = min(a[3], v), max(a[4], v)
        self.changed[slice_end] = True

    def drop(self, slice_end):
        self.slices.pop(slice_end, None)
        self.changed.pop(slice_end, None)

    def plan(self):
        se = sorted(self.slices)
        rows = np.array([len(self.slices[s]) for s in se], dtype=np.int64)
        first = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64) if se else np.zeros(0, dtype=np.int64)
        return dict(slice_end=np.array(se, dtype=np.int64), first_row=first, rows=rows,
                    changed=np.array([self.changed[s] for s in se], dtype=bool))

    def image(self, want=None):
        """(image, its slices) of the planned slices with want != 0 (all if None); clears their flags"""
        p = self.plan()
        want = np.ones(len(p["slice_end"]), dtype=np.uint8) if want is None else np.asarray(want)
        assert len(want) == len(p["slice_end"])
        cols = {c: [] for c in ("key", "slice_end", "cnt_star", "cnt_val", "sum", "min", "max")}
        sel = want != 0
        for se in p["slice_end"][sel].tolist():
            for k, a in sorted(self.slices[se].items(), key=lambda kv: -kv[0]):   # (any order inside a slice)
                for c, x in zip(cols, (k, se, *a)):
                    cols[c].append(x)
            self.changed[se] = False
        rows = p["rows"][sel]
        sl = dict(slice_end=p["slice_end"][sel], rows=rows, changed=p["changed"][sel],
                  first_row=(np.cumsum(rows) - rows).astype(np.int64))
        return {c: np.array(v, dtype=np.int64) for c, v in cols.items()}, sl


def drive(spec, barriers):
    """barriers: (writes [(slice_end, keys)], slices dropped (fired and expired), progress) per
    checkpoint. Two engines in the same state: one selects, one exports everything."""
    sel, ref = Engine(), Engine()
    delta, inc = WindowAggsState(spec, f64=False), WindowAggsState(spec, f64=False)
    left_out = 0
    for i, (writes, drops, progress) in enumerate(barriers):
        for e in (sel, ref):
            for se, keys in writes:
                e.add(se, keys, v=i + 1)
            for se in drops:
                e.drop(se)
        plan = sel.plan()
        for b in (delta, inc):
            b.advance_watermark(progress)
        want = delta.wanted_slices(plan, progress)
        assert want.dtype == np.uint8 and len(want) == len(plan["slice_end"])
        assert want[plan["changed"]].all(), f"barrier {i}: a changed slice is not selected"
        left_out += int((want == 0).sum())
        img, img_sl = sel.image(want)
        assert len(img["key"]) == int(plan["rows"][want != 0].sum())
        delta.write_delta(img, img_sl, plan, progress)
        full_img, full_sl = ref.image()
        for c in ("slice_end", "first_row", "rows", "changed"):
            assert np.array_equal(full_sl[c], plan[c]), (i, c)
        inc.write_image(full_img, full_sl, progress)
        assert delta.entries == inc.entries, f"barrier {i}: entries differ"
        assert delta.timers == inc.timers, f"barrier {i}: timers differ"
        assert delta.namespaces == inc.namespaces and delta.contrib == inc.contrib, i
    return left_out, delta


K = np.arange


def test_policy_tumble():
    spec = SliceSpec(TUMBLE, 1000)
    left_out, _ = drive(spec, [
        ([(1000, K(0, 40)), (2000, K(10, 30))], [], 500),
        ([(2000, K(25, 50))], [1000], 1200),
        ([(3000, K(0, 5))], [], 1300),              # slice 2000 untouched
        ([(3000, K(3, 9)), (4000, K(7, 8))], [2000], 2500),
        ([], [], 2600),                             # nothing written at all
    ])
    assert left_out >= 2


def test_policy_hop_leaves_untouched_slices_out():
    spec = SliceSpec(HOP, 3000, 1000)
    left_out, delta = drive(spec, [
        ([(1000, K(0, 30)), (2000, K(5, 40)), (3000, K(20, 60))], [], 100),
        ([(3000, K(55, 70))], [], 200),                     # one micro-batch later: 1000 and 2000 untouched
        ([(4000, K(0, 10))], [], 1100),                     # slice 1000 fired (window 1000), kept for 2000 / 3000
        ([(4000, K(5, 15)), (5000, K(90, 95))], [1000], 2300),   # the next window end moved; 2000 fired, unselected
        ([(5000, K(1, 3))], [2000], 3050),
    ])
    assert left_out >= 4
    assert delta.ops["scan"] > 0   # the keys of unselected fired slices came from the backend


def test_policy_cumulate_rebuilds_a_namespace_from_all_its_slices():
    spec = SliceSpec(CUMULATE, 4000, 1000)
    left_out, _ = drive(spec, [
        ([(1000, K(0, 30)), (2000, K(10, 50))], [], 100),
        ([(2000, K(45, 60)), (3000, K(0, 4))], [], 1100),   # slice 1000 fired: namespace 1000 = {1000}
        ([(3000, K(2, 9))], [], 2200),                      # slice 2000 fired into namespace 1000: rebuilt
        ([(4000, K(70, 75))], [], 2300),                    # namespace 1000 = {1000, 2000} untouched
        ([(5000, K(0, 3))], [1000, 2000, 3000, 4000], 4100),
    ])
    assert left_out >= 2


def test_write_delta_refuses_an_image_that_lacks_a_needed_slice():
    spec = SliceSpec(HOP, 3000, 1000)
    e = Engine()
    e.add(1000, K(0, 5))
    e.add(2000, K(0, 5))
    b = WindowAggsState(spec, f64=False)
    plan = e.plan()
    img, sl = e.image([1, 0])
    with pytest.raises(ValueError):
        b.write_delta(img, sl, plan, 0)
