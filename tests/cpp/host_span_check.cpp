// host_span_check.cpp — exhaustive CPU check of oneccl_amd/csrc/host_span.hpp,
// the address arithmetic under every staged copy of mi_reduce.hip: the
// aligned hull, the head / interior / tail split, the span a copy hands the
// runtime, and the staging chunk.  No GPU, no library: the header is plain
// C++.  Addresses are numbers only; nothing is dereferenced.
//
// Over every address offset 0..4111 within a page pair (every `& 15`, both
// sides of a page boundary) and lengths 0..80, 4095, 4096, 4097, kChunkBytes
// and kChunkBytes + 15:
//   * head + interior + tail == bytes; head, tail < 16; interior % 16 == 0;
//     a non-empty interior starts on a 16-byte boundary;
//   * the hull is aligned and contains the span; hi - lo <= bytes +
//     kStageSlack - 2; shift + bytes <= hi - lo;
//   * the hull touches no page the span does not touch;
//   * the runtime span is the hull, or else the interior;
//   * hull, split, runtime span and staging offset equal the formulas of
//     h2d_stage, d2h_pageable, copy_geometry and reduce_issue as they stood
//     before the header held them, written out below.
// Over every offset and element sizes 1, 2, 4, 8: a staging buffer
// (stage_buf_bytes) holds the hull of a whole chunk at its shift, and chunks
// are multiples of 16 elements of at most kChunkBytes.
// Prints "cases N failures F"; exits non-zero on any failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../oneccl_amd/csrc/host_span.hpp"

namespace {

// ---- the formulas before host_span.hpp -------------------------------------
constexpr uintptr_t kAlign = 16;
uintptr_t dn(uintptr_t a) { return a & ~(kAlign - 1); }
uintptr_t up(uintptr_t a) { return (a + kAlign - 1) & ~(kAlign - 1); }

// h2d_stage: the span copied and *shift
void before_h2d_stage(uintptr_t a, size_t bytes, uintptr_t* lo, uintptr_t* hi, size_t* shift) {
    *lo = dn(a), *hi = up(a + bytes);
    *shift = a - *lo;
}
// d2h_pageable (and its hand-written mirror in mi_copy_sync)
void before_d2h_pageable(uintptr_t a, size_t bytes, size_t* head, size_t* interior, size_t* tail) {
    *head = std::min(bytes, (size_t)(up(a) - a));
    *interior = (bytes - *head) & ~(size_t)(kAlign - 1);
    *tail = bytes - *head - *interior;
}
// copy_geometry: the runtime span of an error text
void before_copy_geometry(uintptr_t a, size_t bytes, bool hull, uintptr_t* lo, uintptr_t* hi) {
    *lo = hull ? dn(a) : std::min(up(a), a + bytes);
    *hi = hull ? up(a + bytes) : std::max(*lo, dn(a + bytes));
}
// reduce_issue: an operand's offset in its staging buffers (mi_convert_sync's
// destination offset was the same expression)
size_t before_stage_shift(uintptr_t host_ptr) { return host_ptr & (kAlign - 1); }

long g_cases = 0, g_failures = 0;

void fail(const char* what, uintptr_t a, size_t bytes) {
    if (g_failures++ < 20) fprintf(stderr, "%s: addr & 8191 = %zu, %zu bytes\n", what, (size_t)(a & 8191), bytes);
}

void check(uintptr_t a, size_t bytes) {
    g_cases++;
    const mi::HostSplit s = mi::host_split(a, bytes);
    if (s.head + s.interior + s.tail != bytes) fail("split does not add up", a, bytes);
    if (s.head >= 16 || s.tail >= 16) fail("head or tail of 16 bytes or more", a, bytes);
    if (s.interior % 16) fail("interior is no multiple of 16", a, bytes);
    if (s.interior && ((a + s.head) & 15u)) fail("interior off the 16-byte grid", a, bytes);

    const mi::HostHull h = mi::host_hull(a, bytes);
    if ((h.lo & 15u) || (h.hi & 15u)) fail("hull not aligned", a, bytes);
    if (h.lo > a || h.hi < a + bytes) fail("hull does not contain the span", a, bytes);
    if (h.hi - h.lo > bytes + mi::kStageSlack - 2) fail("hull longer than the span and the slack", a, bytes);
    if (h.shift != a - h.lo || h.shift + bytes > h.hi - h.lo) fail("span at its shift leaves the hull", a, bytes);
    if (h.hi > h.lo) {  // an empty span touches the page of its address
        const uintptr_t first = a >> 12, last = (bytes ? a + bytes - 1 : a) >> 12;
        if ((h.lo >> 12) < first || ((h.hi - 1) >> 12) > last) fail("hull touches another page", a, bytes);
    }

    const mi::HostSpan rh = mi::runtime_span(a, bytes, true), ri = mi::runtime_span(a, bytes, false);
    if (rh.lo != h.lo || rh.bytes != h.hi - h.lo) fail("runtime span of a hull copy is not the hull", a, bytes);
    if (ri.lo != a + s.head || ri.bytes != s.interior) fail("runtime span of an interior copy is not the interior", a, bytes);

    uintptr_t lo, hi;
    size_t shift, head, interior, tail;
    before_h2d_stage(a, bytes, &lo, &hi, &shift);
    if (h.lo != lo || h.hi != hi || h.shift != shift) fail("hull differs from h2d_stage's", a, bytes);
    if (h.shift != before_stage_shift(a)) fail("shift differs from reduce_issue's", a, bytes);
    before_d2h_pageable(a, bytes, &head, &interior, &tail);
    if (s.head != head || s.interior != interior || s.tail != tail) fail("split differs from d2h_pageable's", a, bytes);
    before_copy_geometry(a, bytes, true, &lo, &hi);
    if (rh.lo != lo || rh.bytes != hi - lo) fail("runtime span differs from copy_geometry's (hull)", a, bytes);
    before_copy_geometry(a, bytes, false, &lo, &hi);
    if (ri.lo != lo || ri.bytes != hi - lo) fail("runtime span differs from copy_geometry's (interior)", a, bytes);
}

void check_chunk(uintptr_t a, size_t es) {
    g_cases++;
    const size_t n = mi::stage_chunk_elems(es), before = mi::kChunkBytes / es - (mi::kChunkBytes / es) % 16;
    if (n != before || n % 16 || n == 0 || n * es > mi::kChunkBytes) fail("chunk length", a, es);
    if (mi::stage_buf_bytes(es) != before * es + mi::kStageSlack) fail("staging buffer size differs", a, es);
    const mi::HostHull h = mi::host_hull(a, n * es);
    if (h.hi - h.lo > mi::stage_buf_bytes(es) || h.shift + n * es > mi::stage_buf_bytes(es))
        fail("a chunk's hull does not fit its staging buffer", a, es);
    // the next chunk keeps the operand's shift
    if (mi::host_hull(a + n * es, n * es).shift != h.shift) fail("shift changes from chunk to chunk", a, es);
}

}  // namespace

int main() {
    const uintptr_t base = 0x7f0000010000ull;  // the first of two pages
    const size_t more[] = {4095, 4096, 4097, mi::kChunkBytes, mi::kChunkBytes + 15};
    for (uintptr_t off = 0; off <= 4111; off++) {
        for (size_t bytes = 0; bytes <= 80; bytes++) check(base + off, bytes);
        for (size_t bytes : more) check(base + off, bytes);
        for (size_t es : {1, 2, 4, 8}) check_chunk(base + off, es);
    }
    printf("cases %ld failures %ld\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
