// carve.h -- how a device workspace is cut into its arrays.  Plain C++, nothing from HIP: the CPU tests drive it over host memory (tests/hostemu).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>

// What a Carve writes down when a log is attached: per array that fitted its offset from the buffer's start, its byte length and its kind, and where
// the last array ends.  The fill mode of the cohort runs (cohort_internal.h) reads it.  Fixed capacity, no allocation: an array beyond kCap sets
// `full` (the reader fails its call) and still moves `end`.  A take of no elements is no array.
enum class CarveKind : uint8_t { fp = 0, int1 = 1, int2 = 2, int4 = 4, int8 = 8 };              // (an integer kind's value is its width)
struct CarveLog {
    static constexpr uint32_t kCap = 48;
    struct Array { size_t off, bytes; CarveKind kind; };
    Array a[kCap]; uint32_t n = 0; size_t end = 0; bool full = false;
    void note(size_t off, size_t bytes, CarveKind kind) {
        if (!bytes) return;
        end = off + bytes;
        if (n < kCap) a[n++] = Array{off, bytes, kind}; else full = true;
    }
};
template <class T> constexpr CarveKind carve_kind() {
    static_assert(std::is_floating_point<T>::value || (std::is_integral<T>::value && (sizeof(T) == 1 || sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8)),
                  "a workspace array is of doubles, floats or integers of 1, 2, 4 or 8 bytes");
    return std::is_floating_point<T>::value ? CarveKind::fp : (CarveKind)sizeof(T);
}

// Hands out a buffer's bytes array by array and remembers whether it was asked for more than the buffer holds: CARVE_TRY, behind the last array and in
// front of the first launch, fails the call instead of letting a kernel write past the end.  An array that does not fit sets `over`, gets the current
// position, moves nothing and is not logged; no padding between arrays.
struct Carve {
    uint8_t *at; size_t left; bool over = false;
    uint8_t *base; CarveLog *log;
    Carve(void *base_, size_t cap, CarveLog *log_ = nullptr) : at((uint8_t *)base_), left(cap), base((uint8_t *)base_), log(log_) {
        if (log) { log->n = 0; log->end = 0; log->full = false; }
    }
    template <class T> T *take(size_t n) {
        if (n > left / sizeof(T)) { over = true; n = 0; }
        T *r = (T *)at; at += n * sizeof(T); left -= n * sizeof(T);
        if (log) log->note((size_t)((uint8_t *)r - base), n * sizeof(T), carve_kind<T>());
        return r;
    }
    uint8_t *u8(size_t n) { return take<uint8_t>(n); }
    uint32_t *u32(size_t n) { return take<uint32_t>(n); }
    uint64_t *u64(size_t n) { return take<uint64_t>(n); }
};
// (inside a function with the entry points' `err`, `errlen` and api_internal.h's fail())
#define CARVE_TRY(w, what) \
    do { if ((w).over) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: the %s buffer is smaller than its arrays\n", what); } while (0)

// The guard bytes of the fill mode: everything behind a workspace's last array is set to kCarveGuardByte in front of the call's launches, and the
// first kCarveGuardWindow bytes of that come back with the results.  carve_guard_check: true when window[0 .. n) still holds the guard byte; else
// false, and msg says which workspace (the name CARVE_TRY calls it by) and which byte changed.
constexpr uint8_t kCarveGuardByte = 0xA5;
constexpr size_t kCarveGuardWindow = 256;
inline bool carve_guard_check(const uint8_t *window, size_t n, const char *what, char *msg, size_t msglen) {
    for (size_t i = 0; i < n; ++i) if (window[i] != kCarveGuardByte) {
        if (msg && msglen) snprintf(msg, msglen, "regtools_amd: a kernel wrote behind the arrays of the %s buffer: byte %zu behind the last array is 0x%02x, not 0x%02x\n",
                                    what, i, window[i], kCarveGuardByte);
        return false;
    }
    return true;
}
