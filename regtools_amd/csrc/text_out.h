// text_out.h -- the one two-pass text writer of the cohort formatters: a body writes through a TextOut once to size the text and, when it fits, a
// second time into the caller's buffer.  Standard headers only.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <charconv>

struct TextOut {
    char *dst; size_t need = 0;                                         // dst: null while sizing
    void put(const char *s, size_t k) { if (dst) memcpy(dst + need, s, k); need += k; }
    void put(const char *s) { put(s, strlen(s)); }
    // bounded fields only (numbers, a strand word): what does not fit the buffer is cut, never overrun
    __attribute__((format(printf, 2, 3))) void fmt(const char *f, ...) {
        char b[256];
        va_list ap; va_start(ap, f);
        const int k = vsnprintf(b, sizeof b, f, ap);
        va_end(ap);
        put(b, k < 0 ? 0 : (size_t)k < sizeof b ? (size_t)k : sizeof b - 1);
    }
    // %.17g and `end`; every NaN as "nan", whatever its sign
    void g17(double x, char end) { if (x != x) fmt("nan%c", end); else fmt("%.17g%c", x, end); }
    void u(uint64_t v) { char b[24]; put(b, (size_t)(std::to_chars(b, b + sizeof b, v).ptr - b)); }
};

// body(TextOut &) once to size the text, a second time into buf only when it fits: nothing is written into a buffer that is too small.  Returns
// the bytes needed.
template <class F> size_t format_twice(char *buf, size_t cap, F body) {
    TextOut size{nullptr};
    body(size);
    if (buf && size.need <= cap) { TextOut out{buf}; body(out); }
    return size.need;
}
