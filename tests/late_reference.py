"""Which elements of a batch the DataStream WindowOperator side-outputs (or, without a
lateDataOutputTag, counts in numLateRecordsDropped), in numpy with Java's wrapping long arithmetic.

Written from WindowOperator.java (flink-streaming-java), not from the engine:
  processElement :448-456   if (isSkippedElement && isElementLate(element)) sideOutput / inc()
    isSkippedElement: every window the assigner gave the element was skipped by
    `if (isWindowLate(window)) continue;` (:425-428 of the non-merging branch)
  isWindowLate  :608-611    cleanupTime(window) <= internalTimerService.currentWatermark()
  isElementLate :620-622    element.getTimestamp() + allowedLateness <= currentWatermark()
  cleanupTime   :669-673    maxTimestamp() + allowedLateness, Long.MAX_VALUE when that overflows
and the assigners TumblingEventTimeWindows / SlidingEventTimeWindows.assignWindows over
TimeWindow.getWindowStartWithOffset (timestamp - (timestamp - offset + size) % size, Java %).
"""
from __future__ import annotations

import numpy as np

JMIN = np.iinfo(np.int64).min
JMAX = np.iinfo(np.int64).max


def _jrem(a, b):
    """Java a % b (the sign of the dividend) for b > 0."""
    return np.fmod(a, np.int64(b))


def _window_start(ts, offset, size):
    with np.errstate(over="ignore"):
        return ts - _jrem(ts - np.int64(offset) + np.int64(size), size)


def cleanup_time(end, lateness):
    with np.errstate(over="ignore"):
        max_ts = end - np.int64(1)
        c = max_ts + np.int64(lateness)
    return np.where(c >= max_ts, c, JMAX)


def dropped_mask(ts, progress, window, lateness=0, purging=False, late_wm=None):
    """Boolean mask over `ts` (int64 epoch millis): the element is skipped by all of its windows
    and late itself under the timer service's watermark `progress`.

    window: ("tumble", size[, offset]) or ("hop", size, slide[, offset]). `purging` and `late_wm`
    do not enter the reference's decision: a PurgingTrigger changes what a window's firing emits,
    not which windows are late, and the only watermark processElement reads is the timer
    service's (Long.MIN_VALUE after a restore, whatever the checkpoint's was) -- they are taken so
    that callers pass the whole configuration of the operator under test."""
    del purging, late_wm
    ts = np.asarray(ts, dtype=np.int64)
    progress = np.int64(progress)
    kind, size = window[0], int(window[1])
    if kind == "tumble":
        slide, offset = size, int(window[2]) if len(window) > 2 else 0
    else:
        slide, offset = int(window[2]), int(window[3]) if len(window) > 3 else 0
    skipped = np.ones(len(ts), dtype=bool)
    with np.errstate(over="ignore"):
        last_start = _window_start(ts, offset, slide)
        # SlidingEventTimeWindows: for (start = lastStart; start > timestamp - size; start -= slide)
        for k in range(-(-size // slide)):
            start = last_start - np.int64(k * slide)
            assigned = start > ts - np.int64(size) if kind != "tumble" else np.ones(len(ts), dtype=bool)
            end = start + np.int64(size)
            window_late = cleanup_time(end, lateness) <= progress
            skipped &= ~assigned | window_late
        element_late = ts + np.int64(lateness) <= progress
    return skipped & element_late
