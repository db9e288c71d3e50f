// result_block.h -- the one owner of a result's block: every result the cohort calls hand out (matrix, clusters, phenotype table, principal
// components, the three sQTL results) is a ResultBox, its arrays in ONE block from the block cache (api_ctx.cpp).  Standard headers only: a plain
// host program that defines block_take / block_give can include it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

// api_ctx.cpp: a block of at least `need` bytes (cap: what it really holds), page-locked when asked for; null: none to be had
void *block_take(size_t need, size_t &cap, bool pinned);
void block_give(void *p, size_t cap, bool pinned);

// A result and the one block its arrays live in, with what else the library keeps beside it (the matrix: its serial).  arrays(q, take) names every
// array once with its length; it runs twice, to size the block (a running offset, every array 16-byte aligned) and to hand out the pointers.
// Page-locked when asked for and possible.  The box starts zeroed and is never constructed: X is plain data.
struct NoExtra {};
template <class R, class X = NoExtra> struct ResultBox { R q; void *block; size_t block_cap; bool pinned; X extra; };
struct BlockTake {
    uint8_t *base; size_t o = 0;
    template <class T> void operator()(T *&p, size_t n) { if (base) p = (T *)(base + o); o += (n * sizeof(T) + 15) & ~(size_t)15; }
};
template <class R, class X = NoExtra, class F> R *result_alloc(bool pinned, F arrays) {
    ResultBox<R, X> *box = (ResultBox<R, X> *)calloc(1, sizeof *box);
    if (!box) return nullptr;
    BlockTake size{nullptr};
    arrays(box->q, size);
    const size_t need = size.o ? size.o : 16;                           // (a result without entries still owns a block)
    box->pinned = pinned;
    box->block = block_take(need, box->block_cap, pinned);
    if (!box->block && pinned) { box->pinned = false; box->block = block_take(need, box->block_cap, false); }
    if (!box->block) { free(box); return nullptr; }
    BlockTake take{(uint8_t *)box->block};
    arrays(box->q, take);
    return &box->q;
}
template <class X, class R> X &result_extra(R *q) { return ((ResultBox<R, X> *)q)->extra; }                // q is the first member
template <class R, class X = NoExtra> void result_free(R *q) {
    if (!q) return;
    ResultBox<R, X> *box = (ResultBox<R, X> *)q;
    block_give(box->block, box->block_cap, box->pinned);
    free(box);
}
