// host_span.hpp — the byte ranges of a host operand that the runtime's copies
// are handed, and the staging chunk.  Plain C++ with no HIP header, so a CPU
// program can include it (tests/cpp/host_span_check.cpp checks every formula
// here over every address offset within a page pair).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mi {

// The runtime's copies between pageable host memory and the device get
// 16-byte-aligned host addresses and 16-byte multiples only (mi_reduce.hip,
// "the runtime's copies of pageable memory").
constexpr uintptr_t kHostAlign = 16;
constexpr size_t kStageSlack = 2 * kHostAlign;  // a staging buffer holds a chunk and its alignment
constexpr size_t kChunkBytes = 32ull << 20;     // staging chunk per operand

inline uintptr_t host_align_dn(uintptr_t a) { return a & ~(kHostAlign - 1); }
inline uintptr_t host_align_up(uintptr_t a) { return (a + kHostAlign - 1) & ~(kHostAlign - 1); }

// The aligned hull [lo, hi) of [a, a + bytes): what an H2D into a staging
// buffer copies.  The operand then lies `shift` bytes into that buffer.
// Aligning by < 16 bytes never leaves the pages the operand touches.
struct HostHull {
    uintptr_t lo, hi;
    size_t shift;  // a - lo
};
inline HostHull host_hull(uintptr_t a, size_t bytes) {
    const uintptr_t lo = host_align_dn(a);
    return {lo, host_align_up(a + bytes), (size_t)(a - lo)};
}

// [a, a + bytes) = head + interior + tail: the interior starts and ends on a
// 16-byte boundary and goes to the runtime; head and tail (< 16 bytes each)
// go through pinned scratch.  A span that reaches no boundary is all head.
struct HostSplit {
    size_t head, interior, tail;
};
inline HostSplit host_split(uintptr_t a, size_t bytes) {
    const size_t to_boundary = (size_t)(host_align_up(a) - a);
    const size_t head = bytes < to_boundary ? bytes : to_boundary;
    const size_t interior = (bytes - head) & ~(size_t)(kHostAlign - 1);
    return {head, interior, bytes - head - interior};
}

// Pinned scratch for the two ends of one copy: the head at 0, the tail at kEdgeTail.
constexpr size_t kEdgeTail = kHostAlign, kEdgeSlot = 2 * kHostAlign;

// The host range one copy hands the runtime: the operand's hull, or else its
// interior (possibly empty).
struct HostSpan {
    uintptr_t lo;
    size_t bytes;
};
inline HostSpan runtime_span(uintptr_t a, size_t bytes, bool hull) {
    if (hull) {
        const HostHull h = host_hull(a, bytes);
        return {h.lo, (size_t)(h.hi - h.lo)};
    }
    const HostSplit s = host_split(a, bytes);
    return {a + s.head, s.interior};
}

// Elements of a staging chunk when the largest operand element has `es`
// bytes.  A multiple of 16: chunk starts are then 16-byte multiples apart, so
// an operand keeps its `shift` from chunk to chunk, and they are multiples of
// 16 elements, so the VCVTNEPS2BF16 tail split (elements from
// (count / 16) * 16 on are truncated), which is defined on the whole array,
// falls into the last chunk only and at the same place as a per-chunk split.
inline size_t stage_chunk_elems(size_t es) {
    const size_t n = kChunkBytes / es;
    return n - n % 16;
}
// A staging buffer: holds the hull of any chunk of such elements.
inline size_t stage_buf_bytes(size_t es) { return stage_chunk_elems(es) * es + kStageSlack; }

}  // namespace mi
