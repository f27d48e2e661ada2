// Host build of fg_window.h for tests/test_window_arith.py: extern "C" wrappers over the
// window / slice arithmetic that the kernels and the engine share, and nothing else. A
// WindowSpec is filled the way fg_open fills it; every function maps an array of times.
#include <cstdint>

#include "fg_window.h"

using namespace fg;

namespace {
int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}
}  // namespace

extern "C" {

// tz_trans / tz_offs: zone rules (tz_n transitions, tz_n + 1 offsets), owned by the caller
void* wa_spec(int32_t kind, int64_t size, int64_t slide, int64_t offset, int64_t tz, int32_t tz_n,
              const int64_t* tz_trans, const int64_t* tz_offs, int32_t tz_dst, int32_t local_input) {
    WindowSpec* w = new WindowSpec{};
    w->kind = kind;
    w->mode = 0;
    w->size = size;
    w->slide = kind == TUMBLE ? size : slide;
    w->offset = offset;
    w->tz = tz_n > 0 ? 0 : tz;
    w->slice = kind == HOP ? gcd64(w->size, w->slide) : w->slide;
    w->nslices = w->size / w->slice;
    w->rslice = 1.0 / (double)w->slice;
    w->rsize = 1.0 / (double)w->size;
    w->tz_n = tz_n;
    w->tz_dst = tz_dst;
    w->tz_trans_h = w->tz_trans_d = tz_trans;
    w->tz_offs_h = w->tz_offs_d = tz_offs;
    w->local_input = local_input;
    return w;
}
void wa_free(void* w) { delete static_cast<WindowSpec*>(w); }
int64_t wa_slice(const void* w) { return static_cast<const WindowSpec*>(w)->slice; }

#define WA_MAP(name, expr)                                                          \
    void name(const void* wp, int64_t n, const int64_t* in, int64_t* out) {        \
        const WindowSpec& w = *static_cast<const WindowSpec*>(wp);                  \
        for (int64_t i = 0; i < n; i++) {                                           \
            const int64_t t = in[i];                                                \
            out[i] = (expr);                                                        \
        }                                                                           \
    }
WA_MAP(wa_assign_slice_end, assign_slice_end(w, t))
WA_MAP(wa_window_start, window_start(w, t))
WA_MAP(wa_last_window_end, last_window_end(w, t))
WA_MAP(wa_merge_target, merge_target(w, t))
WA_MAP(wa_to_utc, to_utc(w, t))
WA_MAP(wa_to_epoch_for_timer, to_epoch_for_timer(w, t))
WA_MAP(wa_pseudo_rowtime, pseudo_rowtime(w, t))
WA_MAP(wa_next_trigger_zone, next_trigger_watermark(w, t, w.slice))
#undef WA_MAP

// is_window_fired(w, end[i], progress)
void wa_is_window_fired(const void* wp, int64_t n, const int64_t* end, int64_t progress, int64_t* out) {
    const WindowSpec& w = *static_cast<const WindowSpec*>(wp);
    for (int64_t i = 0; i < n; i++) out[i] = is_window_fired(w, end[i], progress) ? 1 : 0;
}
// target_slice(w, ts[i], progress): ok[i] = 0 when dropped, else target[i] is the slice
void wa_target_slice(const void* wp, int64_t n, const int64_t* ts, int64_t progress, int64_t* ok, int64_t* target) {
    const WindowSpec& w = *static_cast<const WindowSpec*>(wp);
    for (int64_t i = 0; i < n; i++) {
        int64_t t = 0;
        ok[i] = target_slice(w, ts[i], progress, &t) ? 1 : 0;
        target[i] = t;
    }
}
void wa_next_trigger_watermark(int64_t n, const int64_t* wm, int64_t interval, int64_t* out) {
    for (int64_t i = 0; i < n; i++) out[i] = next_trigger_watermark(wm[i], interval);
}
void wa_floor_div_fast(int64_t n, const int64_t* a, int64_t b, int64_t* out) {
    const double rb = 1.0 / (double)b;
    for (int64_t i = 0; i < n; i++) out[i] = floor_div_fast(a[i], b, rb);
}
void wa_jrem_fast(int64_t n, const int64_t* a, int64_t b, int64_t* out) {
    const double rb = 1.0 / (double)b;
    for (int64_t i = 0; i < n; i++) out[i] = jrem_fast(a[i], b, rb);
}

}  // extern "C"
