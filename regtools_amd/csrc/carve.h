// carve.h -- how a device workspace is cut into its arrays.  Plain C++, nothing from HIP: the CPU tests drive it over host memory (tests/hostemu).
#pragma once
#include <stddef.h>
#include <stdint.h>

// Hands out a buffer's bytes array by array and remembers whether it was asked for more than the buffer holds: CARVE_TRY, behind the last array and in
// front of the first launch, fails the call instead of letting a kernel write past the end.  An array that does not fit sets `over`, gets the current
// position and moves nothing; no padding between arrays.
struct Carve {
    uint8_t *at; size_t left; bool over = false;
    Carve(void *base, size_t cap) : at((uint8_t *)base), left(cap) {}
    template <class T> T *take(size_t n) {
        if (n > left / sizeof(T)) { over = true; n = 0; }
        T *r = (T *)at; at += n * sizeof(T); left -= n * sizeof(T);
        return r;
    }
    uint8_t *u8(size_t n) { return take<uint8_t>(n); }
    uint32_t *u32(size_t n) { return take<uint32_t>(n); }
    uint64_t *u64(size_t n) { return take<uint64_t>(n); }
};
// (inside a function with the entry points' `err`, `errlen` and api_internal.h's fail())
#define CARVE_TRY(w, what) \
    do { if ((w).over) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: the %s buffer is smaller than its arrays\n", what); } while (0)
