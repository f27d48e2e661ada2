"""CPU differential test of fg_window.h, the window / slice arithmetic every kernel and the
host engine share: the header is compiled for the host (tests/window_arith_shim.cpp, built at
run time into a temporary directory) and compared bit for bit with the oracle's assigner
functions -- at window offsets of both signs, fixed zone offsets, times below 0, |t| >= 2^52
(the floor_div_fast fallback), Long.MIN_VALUE / MAX_VALUE and their neighbours, slices of
1 ms and of more than 2^32 ms. No GPU is involved."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JMIN, JMAX = -(1 << 63), (1 << 63) - 1
H8 = 8 * 3600 * 1000
TUMBLE, HOP, CUMULATE = 0, 1, 2
LA = "America/Los_Angeles"

# (kind, size, slide)
WINDOWS = [
    (TUMBLE, 1000, 0), (TUMBLE, 1, 0), (TUMBLE, 7, 0), (TUMBLE, 86_400_000, 0), (TUMBLE, (1 << 32) + 5, 0),
    (HOP, 3000, 1000),
    (CUMULATE, 5000, 1000), (CUMULATE, 86_400_000, 3_600_000),
]
TZS = (0, H8, -H8)


def slice_of(kind, size, slide):
    return size if kind == TUMBLE else (int(np.gcd(size, slide)) if kind == HOP else slide)


def offsets_of(slice_):
    """0, a small positive offset, slice - 1, -(slice - 1), -(slice / 3) -- those the slice admits
    (|offset| < slice: SliceAssigners.java:149-158)."""
    out = []
    for o in (0, min(3, slice_ - 1), slice_ - 1, -(slice_ - 1), -(slice_ // 3)):
        if o not in out:
            out.append(o)
    return out


CONFIGS = [(k, size, slide, off, tz) for k, size, slide in WINDOWS for off in offsets_of(slice_of(k, size, slide))
           for tz in TZS]


def wrap(x):
    """Java long wrap of a Python integer."""
    return ((int(x) - JMIN) % (1 << 64)) + JMIN


def times_for(size, seed):
    """The adversarial times, plus seeded random ones per range: around 0, epoch-scale of both
    signs, both sides of +-2^52, and the whole 64-bit range."""
    adv = [0, 1, -1, size, -size, size - 1, -size + 1, size + 1, -size - 1, 2 * size, -2 * size]
    for p in (1 << 52, -(1 << 52)):
        adv += [p - 1, p, p + 1]
    adv += [JMIN, JMIN + 1, JMIN + 2, JMIN + size, JMAX, JMAX - 1, JMAX - 2, JMAX - size]
    adv += [1 << 30, (1 << 30) - 1, 1 << 32, -(1 << 32), 1 << 33, 1_600_000_000_000, -1_600_000_000_000, H8, -H8,
            H8 - 1, -H8 - 1]
    rng = np.random.default_rng(seed)
    n = 150
    rnd = np.concatenate([
        rng.integers(-10 * size, 10 * size + 1, n),
        rng.integers(-(1 << 41), 1 << 41, n),
        (1 << 52) + rng.integers(-(1 << 33), 1 << 33, n),
        -(1 << 52) + rng.integers(-(1 << 33), 1 << 33, n),
        rng.integers(JMIN, JMAX, n, endpoint=True),
    ])
    return np.unique(np.concatenate([np.array([wrap(a) for a in adv], dtype=np.int64), rnd.astype(np.int64)]))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("window_arith") / "libwindow_arith.so")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "hip", "--cuda-host-only",
                    "-I", os.path.join(ROOT, "flink_amd", "csrc"), os.path.join(HERE, "window_arith_shim.cpp"),
                    "-o", out], check=True)
    L = C.CDLL(out)
    P = C.c_void_p
    L.wa_spec.restype = P
    L.wa_spec.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, P, P, C.c_int32, C.c_int32]
    L.wa_free.argtypes = [P]
    L.wa_slice.restype = C.c_int64
    L.wa_slice.argtypes = [P]
    for fn in ("wa_assign_slice_end", "wa_window_start", "wa_last_window_end", "wa_merge_target", "wa_to_utc",
               "wa_to_epoch_for_timer", "wa_pseudo_rowtime", "wa_next_trigger_zone"):
        getattr(L, fn).argtypes = [P, C.c_int64, P, P]
    L.wa_is_window_fired.argtypes = [P, C.c_int64, P, C.c_int64, P]
    L.wa_target_slice.argtypes = [P, C.c_int64, P, C.c_int64, P, P]
    for fn in ("wa_next_trigger_watermark", "wa_floor_div_fast", "wa_jrem_fast"):
        getattr(L, fn).argtypes = [C.c_int64, P, C.c_int64, P]
    return L


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as mod
    mod.build()
    return mod


class Spec:
    """A WindowSpec of the shim; map(fn, times) applies one fg_window.h function to an array."""

    def __init__(self, L, kind, size, slide, offset, tz, zone=None, local_input=False):
        self.L = L
        self._keep = None
        tz_n, tr, of, dst = 0, None, None, 0
        if zone:
            from flink_amd.tz import zone_rules
            t, o, d = zone_rules(zone)
            self._keep = (np.ascontiguousarray(t), np.ascontiguousarray(o))
            tz_n, tr, of, dst = len(t), self._keep[0].ctypes.data, self._keep[1].ctypes.data, int(d)
        self.w = L.wa_spec(kind, size, slide, offset, tz, tz_n, tr, of, dst, int(local_input))
        self.slice = L.wa_slice(self.w)

    def map(self, fn, t):
        t = np.ascontiguousarray(t, dtype=np.int64)
        out = np.empty_like(t)
        getattr(self.L, "wa_" + fn)(self.w, len(t), t.ctypes.data, out.ctypes.data)
        return out

    def fired(self, ends, progress):
        ends = np.ascontiguousarray(ends, dtype=np.int64)
        out = np.empty_like(ends)
        self.L.wa_is_window_fired(self.w, len(ends), ends.ctypes.data, progress, out.ctypes.data)
        return out.astype(bool)

    def target_slice(self, ts, progress):
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        ok, tgt = np.empty_like(ts), np.empty_like(ts)
        self.L.wa_target_slice(self.w, len(ts), ts.ctypes.data, progress, ok.ctypes.data, tgt.ctypes.data)
        return ok.astype(bool), tgt

    def close(self):
        self.L.wa_free(self.w)


def omap(fn, h, t):
    """One of the oracle's scalar functions over an array of times."""
    return np.array([fn(h, x) for x in t.tolist()], dtype=np.int64)


def jsub(a, b):
    with np.errstate(over="ignore"):
        return (np.asarray(a, dtype=np.int64).view(np.uint64) - np.uint64(b % (1 << 64))).view(np.int64)


def oracle_of(O, kind, size, slide, offset, tz, zone=None):
    return O.OracleOperator(kind=kind, size=size, slide=slide, offset=offset, tz_offset_ms=tz, val_type=O.VAL_I64,
                            zone=zone)


def oracle_merge_target(O, o, ends):
    """sliceStateMergeTarget: the merge result of mergeSlices (cumulate), else the slice itself."""
    if o.cfg.kind != O.CUMULATE:
        return ends.copy()
    L, mr, tmp = O.lib(), C.c_int64(), (C.c_int64 * 1)()
    out = np.empty_like(ends)
    for i, e in enumerate(ends.tolist()):
        L.or_merge_slices(o._h, e, C.byref(mr), tmp, 1)
        out[i] = mr.value
    return out


def oracle_fired(O, o, ends, progress):
    """TimeWindowUtil.isWindowFired from the oracle's toEpochMillsForTimer."""
    trig = omap(O.lib().or_to_epoch_for_timer, o._h, jsub(ends, 1))
    return (ends != JMAX) & (progress >= trig)


def oracle_target_slice(O, o, ts, progress):
    """AbstractWindowAggProcessor.processElement :135-165 from the oracle's primitives: a record
    of a fired slice is dropped when the slice's last window has fired too, else it goes to
    the slice's merge target; a record of an unfired slice goes to its slice."""
    s = omap(O.lib().or_assign_slice_end, o._h, ts)
    fired = oracle_fired(O, o, s, progress)
    last_fired = oracle_fired(O, o, omap(O.lib().or_get_last_window_end, o._h, s), progress)
    ok = ~(fired & last_fired)
    return ok, np.where(fired, oracle_merge_target(O, o, s), s)


def same(a, b, what, t):
    bad = np.nonzero(np.asarray(a) != np.asarray(b))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} differ, first at t={t[bad[:4]]}: {np.asarray(a)[bad[:4]]} vs {np.asarray(b)[bad[:4]]}"


def test_direct_functions_match_the_oracle(shim, O):
    """assign_slice_end, window_start, last_window_end, merge_target, to_utc, to_epoch_for_timer,
    is_window_fired and target_slice, bit for bit, over every configuration and time."""
    L = O.lib()
    tuples = 0
    for ci, (kind, size, slide, off, tz) in enumerate(CONFIGS):
        ctx = f"kind {kind} size {size} slide {slide} offset {off} tz {tz}"
        t = times_for(size, 1000 + ci)
        s, o = Spec(shim, kind, size, slide, off, tz), oracle_of(O, kind, size, slide, off, tz)
        ends = omap(L.or_assign_slice_end, o._h, t)
        same(s.map("assign_slice_end", t), ends, ctx + " assign_slice_end", t)
        same(s.map("to_utc", t), omap(L.or_to_utc, o._h, t), ctx + " to_utc", t)
        same(s.map("to_epoch_for_timer", t), omap(L.or_to_epoch_for_timer, o._h, t), ctx + " to_epoch_for_timer", t)
        # window functions take grid ends (what the operators hand them) and, as times, anything
        for x, tag in ((ends, "grid ends"), (t, "times")):
            same(s.map("window_start", x), omap(L.or_get_window_start, o._h, x), f"{ctx} window_start of {tag}", x)
            same(s.map("last_window_end", x), omap(L.or_get_last_window_end, o._h, x),
                 f"{ctx} last_window_end of {tag}", x)
        same(s.map("merge_target", ends), oracle_merge_target(O, o, ends), ctx + " merge_target", ends)
        # progress: unset, both sides of zero, inside the times' ranges, the end of time
        for progress in (JMIN, -size - 1, -1, 0, size, 1 << 40, -(1 << 52), (1 << 52) + 7, JMAX - 1, JMAX):
            same(s.fired(ends, progress), oracle_fired(O, o, ends, progress), f"{ctx} is_window_fired at {progress}", ends)
            ok, tgt = s.target_slice(t, progress)
            eok, etgt = oracle_target_slice(O, o, t, progress)
            same(ok, eok, f"{ctx} target_slice dropped at {progress}", t)
            same(tgt[eok], etgt[eok], f"{ctx} target_slice at {progress}", t[eok])
        tuples += len(t)
        s.close()
        o.close()
    assert tuples > 50_000


def test_sliced_input_round_trip(shim, O):
    """A partial or windowed row carries its slice end e and is classified under the rowtime
    pseudo_rowtime(e); the reference's `sliced` / `windowed` assigners take e as it is
    (SliceAssigners.java:402-412, :494-533), so assign_slice_end(pseudo_rowtime(e)) must be e
    for every grid end: negative ends, every offset, fixed zone offsets. Excluded: Long.MAX_VALUE
    (no slice) and ends whose epoch form e - tz lies within one slice of Long.MIN_VALUE, whose
    slice start wraps."""
    L = O.lib()
    checked = negative = 0
    for ci, (kind, size, slide, off, tz) in enumerate(CONFIGS):
        t = times_for(size, 1000 + ci)
        s, o = Spec(shim, kind, size, slide, off, tz), oracle_of(O, kind, size, slide, off, tz)
        ends = np.unique(omap(L.or_assign_slice_end, o._h, t))
        keep = np.array([e != JMAX and e - tz >= JMIN + s.slice for e in ends.tolist()])
        ends = ends[keep]
        back = s.map("assign_slice_end", s.map("pseudo_rowtime", ends))
        same(back, ends, f"kind {kind} size {size} slide {slide} offset {off} tz {tz} round trip", ends)
        # on the slice grid in local time, as the 32-bit fast path and seed_anchor need
        local = s.map("to_utc", s.map("pseudo_rowtime", ends))
        same(local, jsub(ends, s.slice), "pseudo rowtime is the slice start", ends)
        checked += len(ends)
        negative += int((ends < 0).sum())
        s.close()
        o.close()
    assert checked > 40_000 and negative > 15_000, (checked, negative)


def test_zone_rules_match_the_oracle(shim, O):
    """America/Los_Angeles: to_utc, to_epoch_for_timer, is_window_fired and the daylight-saving
    trigger watermark against the oracle around the 2021 gap and overlap and over 1970-2037; the
    local_input round trip of partial rows' local slice ends."""
    L = O.lib()
    size = 3600_000
    spring, fall = 1615708800000, 1636268400000
    rng = np.random.default_rng(7)
    t = np.unique(np.concatenate([
        np.array([0, 1, -1, size, -size, spring, fall], dtype=np.int64),
        spring + rng.integers(-2 * 86_400_000, 2 * 86_400_000, 400),
        fall + rng.integers(-2 * 86_400_000, 2 * 86_400_000, 400),
        rng.integers(0, 2_114_380_800_000, 400),
        np.arange(spring + 8 * 3600_000, spring + 13 * 3600_000, 600_000),
        np.arange(fall + 6 * 3600_000, fall + 12 * 3600_000, 600_000),
    ]).astype(np.int64))
    for kind, sz, slide in ((TUMBLE, size, 0), (HOP, 4 * size, size), (CUMULATE, 3 * size, size)):
        s, o = Spec(shim, kind, sz, slide, 0, 0, zone=LA), oracle_of(O, kind, sz, slide, 0, 0, zone=LA)
        same(s.map("to_utc", t), omap(L.or_to_utc, o._h, t), "zone to_utc", t)
        same(s.map("to_epoch_for_timer", t), omap(L.or_to_epoch_for_timer, o._h, t), "zone to_epoch_for_timer", t)
        same(s.map("next_trigger_zone", t), omap(L.or_next_trigger, o._h, t), "zone next trigger watermark", t)
        ends = omap(L.or_assign_slice_end, o._h, t)
        same(s.map("assign_slice_end", t), ends, "zone assign_slice_end", t)
        for progress in (JMIN, spring + 9 * 3600_000, spring + 10 * 3600_000 - 1, fall + 8 * 3600_000,
                         fall + 9 * 3600_000, fall + 10 * 3600_000 - 1, JMAX):
            same(s.fired(ends, progress), oracle_fired(O, o, ends, progress), f"zone is_window_fired at {progress}", ends)
            ok, tgt = s.target_slice(t, progress)
            eok, etgt = oracle_target_slice(O, o, t, progress)
            same(ok, eok, f"zone target_slice dropped at {progress}", t)
            same(tgt[eok], etgt[eok], f"zone target_slice at {progress}", t[eok])
        # partial rows carry local slice ends (local_input): taken as they are, below zero too
        sl = Spec(shim, kind, sz, slide, 0, 0, zone=LA, local_input=True)
        local_ends = np.unique(np.concatenate([ends, ends - 600_000 * size]))   # 1970-2037 and 68 years below
        same(sl.map("assign_slice_end", sl.map("pseudo_rowtime", local_ends)), local_ends, "local_input round trip",
             local_ends)
        assert (local_ends < 0).sum() > 100
        for x in (s, sl):
            x.close()
        o.close()


def test_next_trigger_watermark_matches_the_oracle(shim, O):
    L = O.lib()
    for interval in (1, 7, 1000, 3_600_000, 86_400_000, (1 << 32) + 5):
        wm = times_for(interval, 5)
        wm = wm[wm > JMIN + 2 * interval]   # below: the watermark's own start wraps
        out = np.empty_like(wm)
        shim.wa_next_trigger_watermark(len(wm), wm.ctypes.data, interval, out.ctypes.data)
        exp = np.array([L.or_next_trigger_watermark(x, interval) for x in wm.tolist()], dtype=np.int64)
        same(out, exp, f"next_trigger_watermark interval {interval}", wm)


def test_fast_division_matches_integer_arithmetic(shim):
    """floor_div_fast / jrem_fast (one f64 multiply and corrections; integer division from
    |a| >= 2^52) against Python's integers: floor division, and Java's truncated remainder."""
    for b in (1, 2, 3, 7, 1000, 999_983, 3_600_000, 86_400_000, (1 << 31) - 1, 1 << 32, (1 << 32) + 5, (1 << 40) + 1,
              (1 << 52) - 1, 1 << 53):
        a = times_for(b, 11)
        a = a[a > JMIN + b]   # floor(a / b) * b stays a long
        q, r = np.empty_like(a), np.empty_like(a)
        shim.wa_floor_div_fast(len(a), a.ctypes.data, b, q.ctypes.data)
        shim.wa_jrem_fast(len(a), a.ctypes.data, b, r.ctypes.data)
        al = a.tolist()
        same(q, np.array([x // b for x in al], dtype=np.int64), f"floor_div_fast by {b}", a)
        jrem = [x % b if x >= 0 else -((-x) % b) for x in al]
        same(r, np.array(jrem, dtype=np.int64), f"jrem_fast by {b}", a)
