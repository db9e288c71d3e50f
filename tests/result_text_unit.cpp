// The smallest cases of result_block.h and text_out.h that can go wrong, as a plain host program (tests/test_result_text_unit.py builds it with
// the address and undefined-behaviour sanitizers and runs it).  The block cache is malloc / free here.
#include "result_block.h"
#include "text_out.h"

#include <math.h>

#include <vector>

static int g_taken = 0, g_given = 0, g_failed = 0;
void *block_take(size_t need, size_t &cap, bool) { ++g_taken; cap = need; return malloc(need); }
void block_give(void *p, size_t, bool) { ++g_given; free(p); }

#define CHECK(cond) do { if (!(cond)) { ++g_failed; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

// arrays of 0, 1 and 3 elements of 1-, 4- and 8-byte types, interleaved
struct Mixed { uint8_t *a0, *a1, *a3; uint32_t *b0, *b1, *b3; uint64_t *c0, *c1, *c3; };
static void mixed_arrays(Mixed &r, BlockTake &take) {
    take(r.a0, 0); take(r.b1, 1); take(r.c3, 3); take(r.a1, 1); take(r.b0, 0); take(r.c1, 1); take(r.a3, 3); take(r.b3, 3); take(r.c0, 0);
}
struct Range { uint8_t *p; size_t bytes; };

static void test_result_alloc() {
    Mixed *m = result_alloc<Mixed>(false, mixed_arrays);
    CHECK(m != nullptr);
    if (!m) return;
    const ResultBox<Mixed> *box = (const ResultBox<Mixed> *)m;
    // the sizing pass and the pointer pass agree, with each other and with the block
    Mixed again{};
    BlockTake size{nullptr}, take{(uint8_t *)box->block};
    mixed_arrays(again, size); mixed_arrays(again, take);
    CHECK(size.o == take.o);
    CHECK(size.o == box->block_cap);
    CHECK(size.o == 5 * 16 + 32);                                       // (five arrays of at most 16 bytes and one of 24; the empty ones take none)
    CHECK(again.b1 == m->b1 && again.c3 == m->c3 && again.a1 == m->a1 && again.c1 == m->c1 && again.a3 == m->a3 && again.b3 == m->b3);
    const Range r[] = {{(uint8_t *)m->b1, 4}, {(uint8_t *)m->c3, 24}, {m->a1, 1}, {(uint8_t *)m->c1, 8}, {m->a3, 3}, {(uint8_t *)m->b3, 12}};
    uint8_t *lo = (uint8_t *)box->block, *hi = lo + box->block_cap;
    for (const Range &x : r) {
        CHECK((uintptr_t)x.p % 16 == 0);
        CHECK(x.p >= lo && x.p + x.bytes <= hi);
        for (const Range &y : r) CHECK(&x == &y || x.p + x.bytes <= y.p || y.p + y.bytes <= x.p);
        memset(x.p, 0x5a, x.bytes);                                     // (the sanitizer sees a write past the block)
    }
    result_free(m);
    result_free((Mixed *)nullptr);

    // nothing but empty arrays: still a result, still a block
    Mixed *e = result_alloc<Mixed>(true, [](Mixed &q, BlockTake &t) { t(q.a0, 0); t(q.b0, 0); t(q.c0, 0); });
    CHECK(e != nullptr);
    if (e) CHECK(((const ResultBox<Mixed> *)e)->block != nullptr);
    result_free(e);

    // a payload beside the result
    Mixed *x = result_alloc<Mixed, uint64_t>(false, mixed_arrays);
    CHECK(x != nullptr);
    if (x) {
        CHECK(result_extra<uint64_t>(x) == 0);
        result_extra<uint64_t>(x) = 0x0123456789abcdefull;
        m = result_alloc<Mixed>(false, mixed_arrays);
        CHECK(result_extra<uint64_t>(x) == 0x0123456789abcdefull && x->c3 != nullptr);
        result_free(m);
    }
    result_free<Mixed, uint64_t>(x);
    CHECK(g_taken == g_given);
}

// The principal components' block: gram, col_sum and the flag's slot are ONE array of S * S + S + 1 doubles (the device copies it back in one
// piece), so col_sum and the flag are derived from gram and no padding comes between them, odd S included.
struct Pcs { double *gram, *col_sum, *variance, *component; };
static void test_pcs_piece(uint32_t S, uint32_t n_pcs) {
    Pcs *p = result_alloc<Pcs>(false, [&](Pcs &r, BlockTake &take) {
        take(r.gram, (size_t)S * S + S + 1); take(r.variance, S); take(r.component, (size_t)n_pcs * S);
    });
    CHECK(p != nullptr);
    if (!p) return;
    p->col_sum = p->gram + (size_t)S * S;
    double *flag = p->col_sum + S;
    CHECK(p->col_sum == p->gram + (size_t)S * S);
    CHECK((uint8_t *)flag == (uint8_t *)p->gram + ((size_t)S * S + S) * 8);
    CHECK((uint8_t *)(flag + 1) <= (uint8_t *)p->variance);
    CHECK((uintptr_t)p->gram % 16 == 0 && (uintptr_t)p->variance % 16 == 0 && (uintptr_t)p->component % 16 == 0);
    for (size_t i = 0; i < (size_t)S * S + S + 1; ++i) p->gram[i] = 1.0;   // the one copy's bytes
    for (uint32_t i = 0; i < S; ++i) p->variance[i] = 2.0;
    for (size_t i = 0; i < (size_t)n_pcs * S; ++i) p->component[i] = 3.0;
    *flag = 0.0;
    CHECK(p->gram[(size_t)S * S + S] == 0.0 && p->variance[0] == 2.0);
    result_free(p);
}

static void test_format_twice() {
    auto body = [](TextOut &o) { o.put("ab", 2); o.put("cd"); o.u(42u); o.fmt("%c%u\n", ':', 7u); };
    const char want[] = "abcd42:7\n";
    const size_t need = sizeof want - 1;
    CHECK(format_twice(nullptr, 1000, body) == need);
    std::vector<char> buf(need + 1);
    // it fits exactly: written, and not a byte more
    memset(buf.data(), 0x7e, buf.size());
    CHECK(format_twice(buf.data(), need, body) == need);
    CHECK(memcmp(buf.data(), want, need) == 0 && buf[need] == 0x7e);
    // one byte short: the size alone, the buffer untouched
    memset(buf.data(), 0x7e, buf.size());
    CHECK(format_twice(buf.data(), need - 1, body) == need);
    for (char c : buf) CHECK(c == 0x7e);
    CHECK(format_twice(buf.data(), 0, [](TextOut &) {}) == 0);
}

static void test_numbers() {
    char buf[64], want[64];
    auto g17 = [&](double x) { return format_twice(buf, sizeof buf, [&](TextOut &o) { o.g17(x, '\t'); }); };
    const double values[] = {-0.0, 0x1p-1074, 0.1, -1.0 / 3.0, 1e300};
    for (double x : values) {
        const size_t k = (size_t)snprintf(want, sizeof want, "%.17g\t", x);
        CHECK(g17(x) == k && memcmp(buf, want, k) == 0);
    }
    CHECK(g17(-0.0) == 3 && memcmp(buf, "-0\t", 3) == 0);
    CHECK(g17(NAN) == 4 && memcmp(buf, "nan\t", 4) == 0);
    CHECK(g17(-NAN) == 4 && memcmp(buf, "nan\t", 4) == 0);              // (snprintf writes -nan: the text does not)
    auto u = [&](uint64_t v) { return format_twice(buf, sizeof buf, [&](TextOut &o) { o.u(v); }); };
    CHECK(u(0) == 1 && buf[0] == '0');
    CHECK(u(UINT64_MAX) == 20 && memcmp(buf, "18446744073709551615", 20) == 0);
    CHECK(u((uint32_t)0xffffffffu) == 10 && memcmp(buf, "4294967295", 10) == 0);
}

int main() {
    test_result_alloc();
    test_pcs_piece(1, 1);
    test_pcs_piece(3, 2);
    test_format_twice();
    test_numbers();
    CHECK(g_taken == g_given);
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("result_text_unit ok\n");
    return 0;
}
