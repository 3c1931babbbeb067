// mixed_grid_check.cpp — exhaustive CPU check of plan_mixed_grid
// (oneccl_amd/csrc/vec_grid.hpp), the head / body / tail split of
// mi_reduce_bcast_mixed.  No GPU, no library: the header is plain C++.
// Addresses are numbers only; nothing is dereferenced.
//
// Over both element-size pairs (2 -> 4, 4 -> 2); every misalignment 0..15 of
// the first output and of an input; a second output at the same misalignment,
// one element further and one byte further; a second input on the outputs'
// grid; an accumulator (widening only) absent, equal to the first output, and
// at every 4th misalignment plus an odd one; counts 0..600; unaligned vectors
// on and off:
//   * with a vector grid, head + 8 * ngroups + tail == count, head <
//     16 / es_out and tail < 8; without one all three are 0 (the element loop
//     takes the whole count);
//   * every body store (4 elements wide: 16 bytes of fp32, 8 of a 16-bit type)
//     of every output is aligned to its width, and every group starts on a
//     16-byte boundary of the output;
//   * the route is the element loop exactly when the outputs' misalignments
//     differ, or an operand (acc included) is not aligned to its element size,
//     or, with unaligned vectors off, an input's or acc's element `head` is not
//     on a 16-byte boundary.
// Prints "cases N failures F"; exits non-zero on any failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../oneccl_amd/csrc/vec_grid.hpp"

namespace {

long g_cases = 0, g_failures = 0;

struct Case {
    size_t es_in, es_out, count;
    uintptr_t outs[2];
    int m;
    uintptr_t ins[2];
    int k;
    uintptr_t acc;  // 0 = none
    bool unaligned;
};

void fail(const char* what, const Case& c, const mi::MixedGrid& g) {
    if (g_failures++ < 20)
        fprintf(stderr,
                "%s: es %zu -> %zu count %zu outs %#zx %#zx (m %d) ins %#zx %#zx (k %d) acc %#zx unaligned %d -> vec %d "
                "head %zu ngroups %llu tail %zu\n",
                what, c.es_in, c.es_out, c.count, (size_t)c.outs[0], (size_t)c.outs[1], c.m, (size_t)c.ins[0],
                (size_t)c.ins[1], c.k, (size_t)c.acc, (int)c.unaligned, (int)g.vec, g.head,
                (unsigned long long)g.ngroups, g.tail);
}

void check(const Case& c) {
    g_cases++;
    const void* po[2] = {reinterpret_cast<const void*>(c.outs[0]), reinterpret_cast<const void*>(c.outs[1])};
    const void* pi[2] = {reinterpret_cast<const void*>(c.ins[0]), reinterpret_cast<const void*>(c.ins[1])};
    const mi::MixedGrid g = mi::plan_mixed_grid(c.es_in, c.es_out, c.count, po, c.m, pi, c.k,
                                                reinterpret_cast<const void*>(c.acc), c.unaligned);

    if (g.vec ? g.head + 8 * g.ngroups + g.tail != c.count : (g.head || g.ngroups || g.tail))
        fail("split does not add up", c, g);
    if (g.head >= 16 / c.es_out || g.tail >= 8) fail("head or tail too long", c, g);

    if (g.vec) {
        const size_t width = 4 * c.es_out;  // bytes of one body store
        const uint64_t nstores = 2 * g.ngroups;
        for (int i = 0; i < c.m; i++)
            for (uint64_t p = 0; p < nstores; p++) {
                if (p >= 4 && p + 2 < nstores && c.count > 48) continue;  // the first four and the last two runs
                const uintptr_t a = c.outs[i] + (g.head + 4 * p) * c.es_out;
                if (a % width) fail("body store not aligned to its width", c, g);
                if (p % 2 == 0 && (a & 15u)) fail("group not on the output's 16-byte grid", c, g);
            }
    }

    // the documented conditions, restated independently
    const size_t head_cap = ((16 - (c.outs[0] & 15u)) & 15u) / c.es_out;
    const size_t head = std::min(head_cap, c.count);
    bool off_elem = false, outs_differ = false, off_grid = false;
    for (int i = 0; i < c.m; i++) {
        off_elem = off_elem || c.outs[i] % c.es_out;
        outs_differ = outs_differ || ((c.outs[i] ^ c.outs[0]) & 15u);
    }
    for (int i = 0; i < c.k; i++) {
        off_elem = off_elem || c.ins[i] % c.es_in;
        off_grid = off_grid || ((c.ins[i] + head * c.es_in) & 15u);
    }
    if (c.acc) {
        off_elem = off_elem || c.acc % 4;
        off_grid = off_grid || ((c.acc + head * 4) & 15u);
    }
    const bool loop = outs_differ || off_elem || (off_grid && !c.unaligned);
    if (g.vec == loop) fail("route", c, g);
    if (g.vec && g.head != head) fail("head is not the outputs' distance to their 16-byte boundary", c, g);
}

}  // namespace

int main() {
    const uintptr_t base_out = 0x7f0000010000ull, base_out2 = 0x7f0000250000ull, base_in = 0x7f0000480000ull,
                    base_in2 = 0x7f0000690000ull, base_acc = 0x7f00008a0000ull;
    const size_t pairs[2][2] = {{2, 4}, {4, 2}};
    for (const auto& pr : pairs) {
        const size_t es_in = pr[0], es_out = pr[1];
        for (unsigned omis = 0; omis < 16; omis++)
            for (unsigned imis = 0; imis < 16; imis++)
                for (size_t count = 0; count <= 600; count++)
                    for (int unaligned = 0; unaligned < 2; unaligned++) {
                        Case c = {es_in, es_out, count, {base_out + omis, 0}, 1, {base_in + imis, 0}, 1, 0, unaligned != 0};
                        check(c);
                        // a second input on the outputs' grid: its element `head` on a 16-byte boundary
                        const size_t head = mi::grid_head(c.outs[0], es_out, count);
                        c.ins[1] = base_in2 + ((16 - (head * es_in) % 16) & 15u);
                        c.k = 2;
                        check(c);
                        // a second output: same misalignment, one element further, one byte further
                        c.m = 2;
                        for (unsigned d : {0u, (unsigned)es_out, 1u}) {
                            c.outs[1] = base_out2 + ((omis + d) & 15u);
                            check(c);
                        }
                        c.m = 1;
                        if (es_out == 4) {  // widening: an accumulator
                            c.acc = c.outs[0];  // in place
                            check(c);
                            for (unsigned amis : {0u, 4u, 8u, 12u, 3u}) {
                                c.acc = base_acc + amis;
                                check(c);
                            }
                        }
                    }
    }
    printf("cases %ld failures %ld\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
