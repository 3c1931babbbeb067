// vec_grid_check.cpp — exhaustive CPU check of plan_vec_grid
// (oneccl_amd/csrc/vec_grid.hpp), the one head / body / tail split behind
// mi_reduce*, mi_reduce_bcast and mi_reduce_batch.  No GPU, no library: the
// header is plain C++.  Addresses are numbers only; nothing is dereferenced.
//
// Over element sizes 1, 2, 4, 8; every misalignment 0..15 of the first
// output, of a second output and of an input; counts 0..70; one and two
// outputs; unaligned vectors on and off:
//   * with a vector grid, head + nvec * (16 / es) + tail == count; without
//     one all three are 0 (the element loop takes the whole count);
//   * head * es < 16 and tail * es < 16;
//   * with a vector grid, every output + head * es is 16-byte aligned, or
//     nvec == 0;
//   * there is no vector grid exactly when some operand is not element-aligned,
//     or the outputs' misalignments differ, or an input's differs from theirs
//     with unaligned vectors off;
//   * the plan equals the formulas of launch_reduce / launch_reduce_bcast as
//     they stood before the plan was shared, written out below.
// Prints "cases N failures F"; exits non-zero on any failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../oneccl_amd/csrc/vec_grid.hpp"

namespace {

struct Want {
    bool vec;
    size_t head;
    uint64_t nvec;
    size_t tail;
};

// launch_reduce_bcast's decision before vec_grid.hpp (launch_reduce's is its
// m = 1 case; launch_reduce_batch's the m = 1, k = 1 case)
Want before(size_t es, size_t count, const uintptr_t* outs, int m, const uintptr_t* ins, int k, bool unaligned) {
    const uintptr_t mis = outs[0] & 15u;
    bool elem = (mis % es) == 0;
    bool same_out = true, same_in = true;
    for (int i = 1; i < m; i++) same_out = same_out && (outs[i] & 15u) == mis;
    for (int i = 0; i < k; i++) {
        elem = elem && (ins[i] % es) == 0;
        same_in = same_in && (ins[i] & 15u) == mis;
    }
    const bool vec = same_out && ((elem && same_in) || (elem && unaligned));
    const size_t n_per_vec = 16 / es;
    const size_t head = vec && mis ? std::min<size_t>((16 - mis) / es, count) : 0;
    const uint64_t nvec = vec ? (count - head) / n_per_vec : 0;
    const size_t tail = vec ? count - head - nvec * n_per_vec : 0;
    return {vec, head, nvec, tail};
}

long g_cases = 0, g_failures = 0;

void fail(const char* what, size_t es, size_t count, const uintptr_t* outs, int m, const uintptr_t* ins, bool unaligned,
          const mi::VecGrid& g) {
    if (g_failures++ < 20)
        fprintf(stderr, "%s: es %zu count %zu outs %#zx %#zx (m %d) ins %#zx %#zx unaligned %d -> vec %d head %zu nvec %llu tail %zu\n",
                what, es, count, (size_t)outs[0], (size_t)outs[1], m, (size_t)ins[0], (size_t)ins[1], (int)unaligned,
                (int)g.vec, g.head, (unsigned long long)g.nvec, g.tail);
}

void check(size_t es, size_t count, const uintptr_t* outs, int m, const uintptr_t* ins, int k, bool unaligned) {
    g_cases++;
    const void* po[2] = {reinterpret_cast<const void*>(outs[0]), reinterpret_cast<const void*>(outs[1])};
    const void* pi[2] = {reinterpret_cast<const void*>(ins[0]), reinterpret_cast<const void*>(ins[1])};
    const mi::VecGrid g = mi::plan_vec_grid(es, count, po, m, pi, k, unaligned);
    const size_t per = 16 / es;

    if (g.vec ? g.head + g.nvec * per + g.tail != count : (g.head || g.nvec || g.tail))
        fail("split does not add up", es, count, outs, m, ins, unaligned, g);
    if (g.head * es >= 16 || g.tail * es >= 16) fail("head or tail of a vector or more", es, count, outs, m, ins, unaligned, g);
    if (g.vec && g.nvec)
        for (int i = 0; i < m; i++)
            if ((outs[i] + g.head * es) & 15u) fail("body not on the output's grid", es, count, outs, m, ins, unaligned, g);

    bool off_elem = false, outs_differ = false, in_differs = false;
    for (int i = 0; i < m; i++) {
        off_elem = off_elem || outs[i] % es;
        outs_differ = outs_differ || ((outs[i] ^ outs[0]) & 15u);
    }
    for (int i = 0; i < k; i++) {
        off_elem = off_elem || ins[i] % es;
        in_differs = in_differs || ((ins[i] ^ outs[0]) & 15u);
    }
    if (g.vec == (off_elem || outs_differ || (in_differs && !unaligned)))
        fail("vector-grid decision", es, count, outs, m, ins, unaligned, g);

    const Want w = before(es, count, outs, m, ins, k, unaligned);
    if (g.vec != w.vec || g.head != w.head || g.nvec != w.nvec || g.tail != w.tail)
        fail("differs from the formulas it replaced", es, count, outs, m, ins, unaligned, g);
}

}  // namespace

int main() {
    const uintptr_t base_out = 0x7f0000010000ull, base_out2 = 0x7f0000250000ull, base_in = 0x7f0000480000ull;
    for (size_t es : {1, 2, 4, 8})
        for (unsigned omis = 0; omis < 16; omis++)
            for (unsigned imis = 0; imis < 16; imis++)
                for (size_t count = 0; count <= 70; count++)
                    for (int unaligned = 0; unaligned < 2; unaligned++) {
                        // inputs: one at imis, and (in place) the first output
                        uintptr_t outs[2] = {base_out + omis, 0};
                        const uintptr_t ins[2] = {base_in + imis, outs[0]};
                        check(es, count, outs, 1, ins, 2, unaligned != 0);
                        check(es, count, outs, 1, ins, 1, unaligned != 0);  // the batch descriptor's shape
                        for (unsigned omis2 = 0; omis2 < 16; omis2++) {
                            outs[1] = base_out2 + omis2;
                            check(es, count, outs, 2, ins, 2, unaligned != 0);
                        }
                    }
    // grid_head alone: convert's and copy's destination grid
    for (size_t es : {1, 2, 4})
        for (unsigned mis = 0; mis < 16; mis += (unsigned)es)
            for (size_t count = 0; count <= 70; count++) {
                g_cases++;
                const size_t want = std::min<size_t>(((16 - mis) & 15u) / es, count);
                if (mi::grid_head(base_out + mis, es, count) != want) {
                    g_failures++;
                    fprintf(stderr, "grid_head: es %zu mis %u count %zu\n", es, mis, count);
                }
            }
    printf("cases %ld failures %ld\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
