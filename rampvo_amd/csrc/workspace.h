// The one way a caller-owned workspace is laid out (host code).  Each workspace has one xxx_carve(ws, <dims>, &w): it walks
// the buffer once with a WsCarver and fills a struct of pointers; with ws == nullptr the same walk only measures, and that
// is what the exported ramp_*_workspace_bytes returns.  Sizes and pointers cannot disagree: they come from the same takes.
#pragma once
#include <stddef.h>

static inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct WsCarver {
  char *base;                            // nullptr: measure only, every take returns nullptr
  size_t off;                            // (a carve that extends another one's layout starts at the bytes that one returned)
  explicit WsCarver(void *ws, size_t at = 0) : base((char *)ws), off(at) {}
  // `count` elements of T at the running offset; the block's end is rounded up to `pad` (1: packed, the next block is adjacent,
  // which is how a layout says that one memset clears both: its length is the difference of the carved pointers)
  template <class T> T *take(size_t count, size_t pad) {
    T *p = base ? (T *)(base + off) : nullptr;
    off = round_up(off + count * sizeof(T), pad);
    return p;
  }
  size_t bytes() const { return off; }
};
// the bytes between two carved blocks: what a memset over adjacent blocks clears
static inline size_t ws_span(const void *first, const void *next) { return (size_t)((const char *)next - (const char *)first); }
