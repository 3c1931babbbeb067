// variant_check.cpp — exhaustive CPU check of oneccl_amd/csrc/variant.hpp, the
// variant rule of the host fold (host_reduce.cpp), against copies of the text
// mi_reduce.hip still holds for the kernels (canon_flags, valid_v) and of the
// host fold's former canon.  No GPU, no library: the header is plain C++.  Built
// twice, as gnu++11 (the in-tree build's standard) and as c++17 (the
// libraries'), where the functions must also be constant expressions.
//
// Over every dtype -1..12, op -1..4, flag word 0..255 and k in {1, 2, 3, 16}:
//   * canon_flags equals the two formulas beside it, mi_reduce.hip's
//     canon_flags and host_reduce.cpp's former canon, written out below;
//   * it is idempotent, its result is below 32 and valid_variant accepts it.
// Over every dtype, op and v in 0..31:
//   * valid_variant(v) equals "some (flags, k) canonicalises to v", and for a
//     real dtype and op the conditions of mi_reduce.hip's valid_v,
//     written out below.
// The number of variants per (dtype, op): integers 1; fp32 / fp64 1 for sum /
// prod and 2 for min / max; fp16 2 and 8; bf16 5 and 10; 94 in all.
// dtype_size over -1..12 and tail_trunc_from at 0, 1, 15, 16, 17, 2^63 + 17.
// Prints "cases N failures F"; exits non-zero on any failure.
#include <cstdint>
#include <cstdio>

#include "../../oneccl_amd/csrc/variant.hpp"

#if __cplusplus >= 201402L
static_assert(mi::valid_variant(MI_BFLOAT16, MI_OP_SUM, 14u) && !mi::valid_variant(MI_BFLOAT16, MI_OP_SUM, 8u) &&
                  mi::canon_flags(MI_FLOAT16, MI_OP_MAX, 255u, 2) == 17u && mi::dtype_size(MI_FLOAT64) == 8 &&
                  mi::tail_trunc_from(33) == 32,
              "the rule is usable at compile time");
#endif

namespace {

// ---- the formulas beside variant.hpp ---------------------------------------
// mi_reduce.hip canon_flags, over reduce_kernels.hpp's V_* bits
const unsigned kInoutFirst = 1u, kBf16Rne = 2u, kAccFp32 = 4u, kTailTrunc = 8u, kFp16Native = 16u;
unsigned before_device(int dt, int op, unsigned f, int k) {
    const bool mm = (op == 2 || op == 3);
    switch (dt) {
        case 9:
        case 10: return mm ? (f & kInoutFirst) : 0u;
        case 8: {
            unsigned v = (mm ? (f & (kInoutFirst | kFp16Native)) : 0u) | (f & kAccFp32);
            if (k == 2 && mm) v &= ~kAccFp32;
            return v;
        }
        case 11: {
            unsigned v = (mm ? (f & kInoutFirst) : 0u) | (f & (kBf16Rne | kAccFp32 | kTailTrunc));
            if (!((v & kAccFp32) && (v & kBf16Rne))) v &= ~kTailTrunc;
            if (k == 2 && mm && !(v & kTailTrunc)) v &= ~kAccFp32;
            return v;
        }
        default: return 0u;
    }
}
// host_reduce.cpp canon, over include/mi_reduce.h's MI_F_* bits
unsigned before_host(int dt, int op, unsigned f, int k) {
    const bool mm = op == MI_OP_MIN || op == MI_OP_MAX;
    switch (dt) {
        case MI_FLOAT32:
        case MI_FLOAT64: return mm ? (f & MI_F_MINMAX_INOUT_FIRST) : 0u;
        case MI_FLOAT16: {
            unsigned v = (mm ? (f & (MI_F_MINMAX_INOUT_FIRST | MI_F_FP16_NATIVE_MINMAX)) : 0u) | (f & MI_F_ACC_FP32);
            if (k == 2 && mm) v &= ~MI_F_ACC_FP32;
            return v;
        }
        case MI_BFLOAT16: {
            unsigned v = (mm ? (f & MI_F_MINMAX_INOUT_FIRST) : 0u) |
                         (f & (MI_F_BF16_RNE | MI_F_ACC_FP32 | MI_F_BF16_TAIL_TRUNC16));
            if (!((v & MI_F_ACC_FP32) && (v & MI_F_BF16_RNE))) v &= ~MI_F_BF16_TAIL_TRUNC16;
            if (k == 2 && mm && !(v & MI_F_BF16_TAIL_TRUNC16)) v &= ~MI_F_ACC_FP32;
            return v;
        }
        default: return 0u;
    }
}
// mi_reduce.hip valid_v<Tag, OP, V>(), the tag's traits spelled by dtype id (0..11), op 0..3
bool before_valid_v(int dt, int op, unsigned v) {
    const bool mm = (op == 2 || op == 3);
    const bool fp = dt >= 8, fp16 = dt == 8, lp = dt == 8 || dt == 11;
    if (!fp) return v == 0;
    if (!lp) return v == 0 || (mm && v == kInoutFirst);
    if ((v & kInoutFirst) && !mm) return false;
    if ((v & kFp16Native) && !(fp16 && mm)) return false;
    if (fp16) return (v & (kBf16Rne | kTailTrunc)) == 0;
    if ((v & kTailTrunc) && !((v & kAccFp32) && (v & kBf16Rne))) return false;
    return true;
}

long g_cases = 0, g_failures = 0;

void fail(const char* what, int dt, int op, unsigned f, int k) {
    if (g_failures++ < 20) fprintf(stderr, "%s: dtype %d, op %d, flags %u, k %d\n", what, dt, op, f, k);
}

const int kKs[] = {1, 2, 3, 16};

void check_canon(int dt, int op, unsigned f, int k) {
    g_cases++;
    const unsigned v = mi::canon_flags(dt, op, f, k);
    if (v != before_device(dt, op, f, k)) fail("differs from mi_reduce.hip's canon_flags", dt, op, f, k);
    if (v != before_host(dt, op, f, k)) fail("differs from host_reduce.cpp's canon", dt, op, f, k);
    if (mi::canon_flags(dt, op, v, k) != v) fail("not idempotent", dt, op, f, k);
    if (v >= 32) fail("a canonical variant of 32 or more", dt, op, f, k);
    if (!mi::valid_variant(dt, op, v)) fail("valid_variant refuses a canonical variant", dt, op, f, k);
}

void check_valid(int dt, int op, unsigned v) {
    g_cases++;
    bool reached = false;
    for (unsigned f = 0; f < 256; f++)
        for (int k : kKs) reached = reached || mi::canon_flags(dt, op, f, k) == v;
    if (mi::valid_variant(dt, op, v) != reached) fail("valid_variant is not the image of canon_flags", dt, op, v, 0);
    if (dt >= 0 && dt <= 11 && op >= 0 && op <= 3 && mi::valid_variant(dt, op, v) != before_valid_v(dt, op, v))
        fail("valid_variant differs from mi_reduce.hip's valid_v", dt, op, v, 0);
}

// variants of (dtype, op): counted over every value a flag word can take
int variants(int dt, int op) {
    int n = 0;
    for (unsigned v = 0; v < 256; v++) n += mi::valid_variant(dt, op, v) ? 1 : 0;
    return n;
}

}  // namespace

int main() {
    for (int dt = -1; dt <= 12; dt++)
        for (int op = -1; op <= 4; op++) {
            for (unsigned f = 0; f < 256; f++)
                for (int k : kKs) check_canon(dt, op, f, k);
            for (unsigned v = 0; v < 32; v++) check_valid(dt, op, v);
        }

    int total = 0;
    for (int dt = 0; dt <= 11; dt++)
        for (int op = 0; op <= 3; op++) {
            g_cases++;
            const bool mm = op >= 2;
            const int want = dt < 8 ? 1 : (dt == 9 || dt == 10) ? (mm ? 2 : 1) : dt == 8 ? (mm ? 8 : 2) : (mm ? 10 : 5);
            const int n = variants(dt, op);
            total += n;
            if (n != want) fail("number of variants", dt, op, (unsigned)n, 0);
        }
    g_cases++;
    if (total != 94) fail("variants in all", 0, 0, (unsigned)total, 0);

    const size_t sizes[] = {0, 1, 1, 2, 2, 4, 4, 8, 8, 2, 4, 8, 2, 0};  // dtypes -1..12
    for (int dt = -1; dt <= 12; dt++) {
        g_cases++;
        if (mi::dtype_size(dt) != sizes[dt + 1]) fail("dtype_size", dt, 0, 0, 0);
    }
    const uint64_t big = (1ull << 63) + 17;
    const uint64_t counts[][2] = {{0, 0}, {1, 0}, {15, 0}, {16, 16}, {17, 16}, {big, big - 1}};
    for (const auto& c : counts) {
        g_cases++;
        if (mi::tail_trunc_from(c[0]) != c[1]) fail("tail_trunc_from", 0, 0, (unsigned)c[0], 0);
    }
    printf("cases %ld failures %ld\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
