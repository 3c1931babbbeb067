// variant.hpp — which bits a call produces: the variant bits, the op ids, the
// element sizes, a call's canonical variant and the keep-precision tail
// threshold, written so that both libraries can hold them once.  The host
// fold (host_reduce.cpp, host_lp.hpp) takes them from here.  The kernels'
// host code (mi_reduce.hip, reduce_kernels.hpp) still has its own canon_flags,
// dtype_size, valid_v and V_* / OP_*, in the same text: do not include this
// header beside reduce_kernels.hpp until they are gone.  Plain C++, no HIP
// and no x86 headers.  tests/cpp/variant_check.cpp checks it exhaustively on
// the CPU, against both libraries' formulas.
#pragma once

#include "../../include/mi_reduce.h"

// C++11 in oneCCL's tree (host_reduce.cpp); constexpr from C++14 on, where
// valid_variant decides at compile time which kernels exist.  Internal
// linkage: neither library exports the rule.
#if __cplusplus >= 201402L
#define MI_VARIANT_FN static constexpr
#else
#define MI_VARIANT_FN static inline
#endif

namespace mi {

enum : int { OP_SUM = 0, OP_PROD = 1, OP_MIN = 2, OP_MAX = 3 };

// Semantic variant bits (the MI_F_* of include/mi_reduce.h, asserted below).
enum : unsigned {
    V_INOUT_FIRST = 1u,  // min/max: MINPS/MAXPS(in, inout) order -> inout on NaN/tie
    V_BF16_RNE = 2u,     // bf16 rounding: VCVTNEPS2BF16 (else truncate)
    V_ACC_FP32 = 4u,     // lp fan-in accumulates in fp32, one rounding at the end
    V_TAIL_TRUNC = 8u,   // with ACC|RNE: elements >= trunc_from truncate at the end
    V_FP16_NATIVE = 16u, // fp16 min/max as VMINPH/VMAXPH (avx512fp16): a NaN accumulator as stored
};

static_assert(V_INOUT_FIRST == MI_F_MINMAX_INOUT_FIRST && V_BF16_RNE == MI_F_BF16_RNE && V_ACC_FP32 == MI_F_ACC_FP32 &&
                  V_TAIL_TRUNC == MI_F_BF16_TAIL_TRUNC16 && V_FP16_NATIVE == MI_F_FP16_NATIVE_MINMAX,
              "every V_* is its MI_F_*");
static_assert(OP_SUM == (int)MI_OP_SUM && OP_PROD == (int)MI_OP_PROD && OP_MIN == (int)MI_OP_MIN &&
                  OP_MAX == (int)MI_OP_MAX,
              "every OP_* is its MI_OP_*");

MI_VARIANT_FN size_t dtype_size(int dt) {
    switch (dt) {
        case MI_INT8: case MI_UINT8: return 1;
        case MI_INT16: case MI_UINT16: case MI_FLOAT16: case MI_BFLOAT16: return 2;
        case MI_INT32: case MI_UINT32: case MI_FLOAT32: return 4;
        case MI_INT64: case MI_UINT64: case MI_FLOAT64: return 8;
        default: return 0;
    }
}

// Keep only the variant bits that change results for (dtype, op, k).
MI_VARIANT_FN unsigned canon_flags(int dt, int op, unsigned f, int k) {
    const bool mm = (op == MI_OP_MIN || op == MI_OP_MAX);
    switch (dt) {
        case MI_FLOAT32:
        case MI_FLOAT64: return mm ? (f & V_INOUT_FIRST) : 0u;
        case MI_FLOAT16: {
            unsigned v = (mm ? (f & (V_INOUT_FIRST | V_FP16_NATIVE)) : 0u) | (f & V_ACC_FP32);
            // One step rounds once either way, but a sum/prod step with fp32
            // accumulation takes the accumulator's NaN first (CCL_REDUCE(float)
            // order), a storage-precision step `in`'s: only min/max may drop the
            // bit.  k = 1 keeps it: no step runs, but the widening to the fp32
            // accumulator (VCVTPH2PS) quiets a signalling NaN, which a copy of
            // the bytes would leave signalling.
            if (k == 2 && mm) v &= ~V_ACC_FP32;
            return v;
        }
        case MI_BFLOAT16: {
            unsigned v = (mm ? (f & V_INOUT_FIRST) : 0u) | (f & (V_BF16_RNE | V_ACC_FP32 | V_TAIL_TRUNC));
            if (!((v & V_ACC_FP32) && (v & V_BF16_RNE))) v &= ~V_TAIL_TRUNC;
            if (k == 2 && mm && !(v & V_TAIL_TRUNC)) v &= ~V_ACC_FP32;  // see fp16 above
            return v;
        }
        default: return 0u;  // integers: no variants
    }
}

// Whether v is in the image of canon_flags, which is what it leaves alone at
// k = 3 (no k drops less): the variants a kernel exists for.
MI_VARIANT_FN bool valid_variant(int dt, int op, unsigned v) { return canon_flags(dt, op, v, 3) == v; }

// V_TAIL_TRUNC threshold: the count % 16 tail that keep-precision truncates starts here.
MI_VARIANT_FN uint64_t tail_trunc_from(uint64_t count) { return (count / 16) * 16; }

}  // namespace mi
