// vec_grid.hpp — the vector-grid plan of an element-wise launch.  Plain C++
// with no HIP header, so a CPU program can include it
// (tests/cpp/vec_grid_check.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mi {

// Elements of `es` bytes before the first 16-byte boundary at or after
// address `a` (itself a multiple of es), at most `count`.
inline size_t grid_head(uintptr_t a, size_t es, size_t count) {
    const size_t h = ((16 - (a & 15u)) & 15u) / es;
    return h < count ? h : count;
}

// count = head + nvec * (16 / es) + tail: a scalar head up to the first
// 16-byte boundary of the output, a body of 16-byte vectors, a scalar tail.
// !vec: no vector grid (all zero), the element loop takes the whole count.
struct VecGrid {
    bool vec;
    size_t head;
    uint64_t nvec;
    size_t tail;
};

// The vector grid is the outputs' 16-byte grid, so the outputs must share
// one misalignment.  Inputs need only be aligned to their element size:
// gfx950 serves a 16-byte load from any byte address
// (profiles/round1_unaligned_probe.jsonl: right bytes at every offset; 98-99 %
// of the aligned stream rate at 4-byte offsets, 89 % at 1- and 2-byte
// offsets), so ring chunks at arbitrary element offsets still stream as
// 16-byte vectors; with `unaligned_ok` off (mi_set_unaligned_vectors(0)) they
// must sit at the outputs' misalignment too.  Operands that are not aligned
// to their element size have no vector grid.
inline VecGrid plan_vec_grid(size_t es, size_t count, const void* const* outs, int m, const void* const* ins, int k,
                             bool unaligned_ok) {
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(outs[0]), mis = o0 & 15u;
    bool elem = (mis % es) == 0, same_out = true, same_in = true;
    for (int i = 1; i < m; i++) same_out = same_out && (reinterpret_cast<uintptr_t>(outs[i]) & 15u) == mis;
    for (int i = 0; i < k; i++) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(ins[i]);
        elem = elem && (p % es) == 0;
        same_in = same_in && (p & 15u) == mis;
    }
    VecGrid g = {same_out && elem && (same_in || unaligned_ok), 0, 0, 0};
    if (g.vec) {
        g.head = grid_head(o0, es, count);
        g.nvec = (count - g.head) / (16 / es);
        g.tail = count - g.head - (size_t)g.nvec * (16 / es);
    }
    return g;
}

// The plan of a launch whose inputs and outputs differ in element size
// (mi_reduce_bcast_mixed; es_in, es_out = 2, 4 or 4, 2): launch_convert's.
// count = head + 8 * ngroups + tail: a scalar head up to the outputs' first
// 16-byte boundary (< 16 / es_out elements), a body of groups of 8 elements
// (16 bytes on the 16-bit side, 32 on the fp32 side), a scalar tail (< 8).
// The body's stores, 4 elements wide, are aligned to their width at every
// group.  !vec: the element loop takes the whole count.
struct MixedGrid {
    bool vec;
    size_t head;
    uint64_t ngroups;
    size_t tail;
};

// The element loop is taken when the outputs sit at differing misalignments
// mod 16, when an operand is not aligned to its element size (`acc`, fp32 or
// null, included), or, with `unaligned_ok` off, when an input or `acc` is off
// the grid: its element `head` is not on a 16-byte boundary.  Otherwise inputs
// may sit at any element-aligned offset, read with unaligned loads.
inline MixedGrid plan_mixed_grid(size_t es_in, size_t es_out, size_t count, const void* const* outs, int m,
                                 const void* const* ins, int k, const void* acc, bool unaligned_ok) {
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(outs[0]), mis = o0 & 15u;
    bool elem = (mis % es_out) == 0, same_out = true;
    for (int i = 1; i < m; i++) same_out = same_out && (reinterpret_cast<uintptr_t>(outs[i]) & 15u) == mis;
    MixedGrid g = {false, 0, 0, 0};
    if (!same_out || !elem) return g;
    const size_t head = grid_head(o0, es_out, count);
    bool on_grid = true;
    for (int i = 0; i < k; i++) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(ins[i]);
        elem = elem && (p % es_in) == 0;
        on_grid = on_grid && ((p + head * es_in) & 15u) == 0;
    }
    if (acc) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(acc);
        elem = elem && (p % 4) == 0;
        on_grid = on_grid && ((p + head * 4) & 15u) == 0;
    }
    if (!elem || !(on_grid || unaligned_ok)) return g;
    g.vec = true;
    g.head = head;
    g.ngroups = (count - head) / 8;
    g.tail = count - head - (size_t)g.ngroups * 8;
    return g;
}

}  // namespace mi
