// reduce_kernels.hpp — CDNA4 (gfx950) element-wise reduction kernels.
//
// Device half of the MI355X-native replacement for oneCCL's local reduction:
//   src/comp/comp.cpp:31-58      CCL_REDUCE (int / fp32 / fp64)
//   src/comp/bf16/*              bf16 reduce (scalar / avx512f / avx512bf)
//   src/comp/fp16/*              fp16 reduce (f16c / avx512f / avx512fp16)
//   src/comp/comp.cpp:202-249    ccl_comp_batch_reduce (K-input fan-in,
//                                optional fp32 keep-precision accumulate)
//   src/kernels/kernels.cl:219-421  device in-place / out-of-place / fan-in
//   src/kernels/kernels.cl:190-217, 424-560  allreduce into two buffers; the
//                                fan-in's result written to every peer
//
// Design: the op is a pure HBM stream with zero data reuse,
// so there is no LDS and no MFMA.  Every lane moves 16-byte vectors
// (global_load_dwordx4: one wave-instruction = 1 KiB, fully coalesced into
// 128-byte lines), U independent vectors per input per lane so that
// K*U*16 bytes per lane are in flight before the first use, non-temporal
// stores for the output (written once, never re-read by this op).  bf16 /
// fp16 are widened to fp32 in registers (a shift for bf16, v_cvt for fp16),
// combined, and rounded back once per step (storage-precision chain) or
// once at the end (fp32 accumulate).
//
// One place for each shared piece: fold_elem (the scalar fold of one
// element), Tile / tile_of (a tile's descriptor geometry), head_tail (block
// 0's scalar duty) and fan_fold (the one-wave tile fold of fan_kernel and
// bcast_kernel).  Every kernel here is reachable from a library entry point;
// kernels that only the measurement tools launch are in
// tools/probe_kernels.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace mi {

enum : int { OP_SUM = 0, OP_PROD = 1, OP_MIN = 2, OP_MAX = 3 };

// Semantic variant bits (same values as MI_F_* in include/mi_reduce.h).
enum : unsigned {
    V_INOUT_FIRST = 1u,  // min/max: MINPS/MAXPS(in, inout) order -> inout on NaN/tie
    V_BF16_RNE = 2u,     // bf16 rounding: VCVTNEPS2BF16 (else truncate)
    V_ACC_FP32 = 4u,     // lp fan-in accumulates in fp32, one rounding at the end
    V_TAIL_TRUNC = 8u,   // with ACC|RNE: elements >= trunc_from truncate at the end
    V_FP16_NATIVE = 16u, // fp16 min/max as VMINPH/VMAXPH (avx512fp16): a NaN accumulator as stored
};

constexpr int kMaxInputs = 16;
constexpr int kBlock = 256;  // 4 waves of 64

// storage tags for the two 16-bit float formats
struct bf16_tag {};
struct fp16_tag {};

template <typename Tag>
struct Tr {  // integers, float, double: storage == compute type
    using S = Tag;
    using C = Tag;
    static constexpr bool lp = false;
    static constexpr bool fp = std::is_floating_point<Tag>::value;
};
template <>
struct Tr<bf16_tag> {
    using S = uint16_t;
    using C = float;
    static constexpr bool lp = true;
    static constexpr bool fp = true;
};
template <>
struct Tr<fp16_tag> {
    using S = uint16_t;
    using C = float;
    static constexpr bool lp = true;
    static constexpr bool fp = true;
};

// Kernel arguments (passed by value in the kernarg segment).
struct KArgs {
    const void* in[kMaxInputs];  // in[0] = accumulator start (the `inout` role)
    void* out;
    uint64_t nvec;        // 16-byte vectors in the aligned body
    uint64_t head;        // leading scalar elements (common misalignment)
    uint64_t tail;        // trailing scalar elements
    uint64_t count;       // total elements
    uint64_t trunc_from;  // V_TAIL_TRUNC threshold (element index)
    int k;                // number of inputs (runtime form)
    int scalar_only;      // operands misaligned differently: element loop only
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// conversions (bit-exact restatements of the x86 instructions the reference
// uses; see oracle/comp_oracle.c and oracle/ISA_CHECK.json)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float bf16_to_f32(uint32_t v) { return __uint_as_float(v << 16); }

__device__ __forceinline__ uint32_t f32_to_bf16_trunc(float f) { return __float_as_uint(f) >> 16; }

// VCVTNEPS2BF16 (Intel SDM convert_fp32_to_bfloat16): zero/denormal ->
// signed zero, NaN -> quiet NaN, otherwise round to nearest even.
// Integer formulation, bit-exact including the NaN payload (~12 VALU ops).
__device__ __forceinline__ uint32_t f32_to_bf16_rne_int(float f) {
    const uint32_t u = __float_as_uint(f);
    uint32_t r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    r = ((u & 0x7FFFFFFFu) > 0x7F800000u) ? ((u >> 16) | 0x40u) : r;
    r = ((u & 0x7F800000u) == 0u) ? ((u >> 16) & 0x8000u) : r;
    return r;
}

__device__ __forceinline__ bool nan_bits(uint32_t u) { return (u & 0x7FFFFFFFu) > 0x7F800000u; }

// Same result via gfx950's v_cvt_pk_bf16_f32 (round to nearest even): flush
// denormals to signed zero first, in the integer domain so the compiler
// cannot fold the flush into the conversion.  Two conversions pack into one
// instruction; ~4 VALU ops per element.  X (exact NaN): a NaN takes
// VCVTNEPS2BF16's quieted upper half explicitly — the hardware's NaN payload
// is its own; the kernels run X only on rows holding an Inf or NaN
// (fold_vec_x86).  Checked against the oracle over all 2^32 fp32 inputs, NaN
// payloads included (tests/test_gpu_convert.py).
template <bool X = true>
__device__ __forceinline__ uint32_t f32_to_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    const uint32_t q = (u >> 16) | 0x40u;
    u = (u & 0x7F800000u) ? u : (u & 0x80000000u);
    const uint32_t r = (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)__uint_as_float(u));
    if constexpr (X) return nan_bits(u) ? q : r;
    return r;
}

// VCVTPH2PS: exact widening (v_cvt_f32_f16; fp16 denormals are on by
// default).  A signalling NaN may stay signalling here; every path that
// stores the value quiets it the way x86 does (x86_nan_first, the narrowing
// below, convert_elem), so stored bits match.
__device__ __forceinline__ float fp16_to_f32(uint32_t h) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
}
// VCVTPS2PH imm8=0: round to nearest even (v_cvt_f16_f32, default RNE mode);
// X: a NaN keeps its sign and top 10 payload bits, quieted (Intel SDM
// VCVTPS2PH).
template <bool X = true>
__device__ __forceinline__ uint32_t f32_to_fp16_rne(float f) {
    const uint32_t u = __float_as_uint(f);
    const uint32_t q = ((u >> 16) & 0x8000u) | 0x7E00u | ((u >> 13) & 0x3FFu);
    const uint32_t r = (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
    if constexpr (X) return nan_bits(u) ? q : r;
    return r;
}

// x86 NaN propagation of ADDPS/MULPS(first, second) (Intel SDM vol. 1
// §4.8.3.5): a NaN operand comes back quieted, the first source's when both
// are; an invalid operation on numbers (inf - inf, 0 * inf) gives the default
// NaN 0xFFC00000.  CDNA's ALUs choose their own NaN, so the low-precision
// paths — whose reference is explicit AVX-512 code, _mm512_add_ps(in, inout)
// (src/comp/bf16/bf16_intrisics.cpp:20-26, fp16_intrisics.hpp:58-63) — fix the
// result up to those bits (oracle/comp_oracle.c x86_nan_first) on the rows
// that need it (fold_vec_x86).
__device__ __forceinline__ float x86_nan_first(float r, float first, float second) {
    const uint32_t a = __float_as_uint(first), b = __float_as_uint(second);
    uint32_t u = __float_as_uint(r);
    u = nan_bits(u) ? 0xFFC00000u : u;
    u = nan_bits(b) ? (b | 0x400000u) : u;
    u = nan_bits(a) ? (a | 0x400000u) : u;
    return __uint_as_float(u);
}
// The same rule for fp64 (default NaN 0xFFF8000000000000).
__device__ __forceinline__ bool nan_bits64(uint64_t u) { return (u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }
__device__ __forceinline__ double x86_nan_first(double r, double first, double second) {
    const uint64_t a = __double_as_longlong(first), b = __double_as_longlong(second);
    uint64_t u = __double_as_longlong(r);
    u = nan_bits64(u) ? 0xFFF8000000000000ull : u;
    u = nan_bits64(b) ? (b | 0x8000000000000ull) : u;
    u = nan_bits64(a) ? (a | 0x8000000000000ull) : u;
    return __longlong_as_double(u);
}

template <typename Tag>
__device__ __forceinline__ typename Tr<Tag>::C widen(typename Tr<Tag>::S s) {
    if constexpr (std::is_same<Tag, bf16_tag>::value)
        return bf16_to_f32(s);
    else if constexpr (std::is_same<Tag, fp16_tag>::value)
        return fp16_to_f32(s);
    else
        return s;
}

// round a compute value to storage: per-step / final rounding
template <typename Tag, unsigned V, bool X = true>
__device__ __forceinline__ typename Tr<Tag>::S narrow(typename Tr<Tag>::C c) {
    // Keep the fp32 value: left alone, the compiler turns
    // fptrunc(fmul(fpext a, fpext b)) into a native v_pk_mul_f16 (likewise
    // adds), whose zero signs differed from VCVTPS2PH of the fp32 product on
    // the GPU (fp16 prod chains gave +0 for -0; profiles/round2_nan/).  The
    // kernels compute in fp32 and round with the restated conversions only;
    // tests/test_kernel_resources.py checks the built code has no f16 math.
    if constexpr (Tr<Tag>::lp) asm volatile("" : "+v"(c));
    if constexpr (std::is_same<Tag, bf16_tag>::value) {
        if constexpr (V & V_BF16_RNE)
            return (uint16_t)f32_to_bf16_rne<X>(c);
        else
            return (uint16_t)f32_to_bf16_trunc(c);
    } else if constexpr (std::is_same<Tag, fp16_tag>::value) {
        return (uint16_t)f32_to_fp16_rne<X>(c);
    } else {
        return c;
    }
}

// ---------------------------------------------------------------------------
// the reduction operator: acc' = op(in, acc)   (`in` role first, as in
// CCL_REDUCE's std::min(in_buf[i], inout_buf[i]))
// ---------------------------------------------------------------------------
template <int OP, bool INOUT_FIRST, typename C>
__device__ __forceinline__ C apply(C in, C acc) {
    if constexpr (std::is_integral<C>::value) {
        // wrap-around integer arithmetic (defined via unsigned)
        using U = typename std::make_unsigned<C>::type;
        using W = typename std::conditional<(sizeof(C) <= 4), uint32_t, uint64_t>::type;
        if constexpr (OP == OP_SUM) return (C)(U)((W)(U)acc + (W)(U)in);
        if constexpr (OP == OP_PROD) return (C)(U)((W)(U)acc * (W)(U)in);
        if constexpr (OP == OP_MIN) return (acc < in) ? acc : in;
        if constexpr (OP == OP_MAX) return (in < acc) ? acc : in;
    } else {
        if constexpr (OP == OP_SUM) return acc + in;
        if constexpr (OP == OP_PROD) return acc * in;
        if constexpr (OP == OP_MIN) {
            if constexpr (INOUT_FIRST)
                return (in < acc) ? in : acc;  // MINPS(in, inout)
            else
                return (acc < in) ? acc : in;  // std::min(in, inout)
        }
        if constexpr (OP == OP_MAX) {
            if constexpr (INOUT_FIRST)
                return (in > acc) ? in : acc;  // MAXPS(in, inout)
            else
                return (in < acc) ? acc : in;  // std::max(in, inout)
        }
    }
}

// one fold step in the variant's precision (X: x86 NaN bits, see above).
// Which operand is the first source: a bf16/fp16 step in storage precision
// is _mm512_add_ps(in, inout) -> `in`; CCL_REDUCE's `inout op= in` on
// float/double, and the fp32 accumulation of keep-precision (CCL_REDUCE(float),
// comp.cpp:223-229), compile to ADDPS/MULPS with `inout` first -> the
// accumulator (pinned by the reference's compiled comp.cpp,
// tests/golden/ref_comp_vectors.npz).
template <typename Tag, int OP, unsigned V, bool X = true>
__device__ __forceinline__ typename Tr<Tag>::C step(typename Tr<Tag>::C x, typename Tr<Tag>::C acc) {
    auto c = apply<OP, (V & V_INOUT_FIRST) != 0>(x, acc);
    if constexpr (X && Tr<Tag>::fp && (OP == OP_SUM || OP == OP_PROD)) {
        if constexpr (Tr<Tag>::lp && !(V & V_ACC_FP32)) c = x86_nan_first(c, x, acc);
        else c = x86_nan_first(c, acc, x);
    }
    if constexpr (Tr<Tag>::lp && !(V & V_ACC_FP32)) c = widen<Tag>(narrow<Tag, V, X>(c));
    return c;
}

// final rounding of the accumulator for element `idx`
template <typename Tag, unsigned V, bool X = true>
__device__ __forceinline__ typename Tr<Tag>::S finish(typename Tr<Tag>::C acc, uint64_t idx,
                                                      uint64_t trunc_from) {
    if constexpr (std::is_same<Tag, bf16_tag>::value && (V & V_TAIL_TRUNC)) {
        return (idx >= trunc_from) ? (uint16_t)f32_to_bf16_trunc(acc)
                                   : (uint16_t)f32_to_bf16_rne<X>(acc);
    } else {
        return narrow<Tag, V, X>(acc);
    }
}

// final store of a fold's accumulator.  In storage precision (bf16 without
// V_ACC_FP32) every step has already rounded, so the accumulator holds a
// bf16 value exactly and its upper half is the result: no second rounding
// (it cost ~8 VALU ops per element pair on the C3 path).
template <typename Tag, unsigned V, bool X = true>
__device__ __forceinline__ typename Tr<Tag>::S finish_fold(typename Tr<Tag>::C acc, uint64_t idx,
                                                           uint64_t trunc_from) {
    if constexpr (std::is_same<Tag, bf16_tag>::value && !(V & V_ACC_FP32))
        return (uint16_t)f32_to_bf16_trunc(acc);
    else
        return finish<Tag, V, X>(acc, idx, trunc_from);
}

// mi_reduce_bcast_scaled: the accumulator times a multiplier before its final
// rounding.  The multiplier is a kernel argument of its own (BCArgs stays what
// mi_reduce_bcast passes): f = (float)d is the compute type's value for fp32,
// bf16 and fp16, d for fp64.  NoScale, the default of every fold below, is the
// unscaled finish.
struct NoScale {};
struct ScaleArg {
    double d;
    float f;
    template <typename C>
    __device__ __forceinline__ C as() const {
        if constexpr (std::is_same<C, double>::value) return d;
        else return f;
    }
};

// finish_fold under a multiplier: one multiply in the compute type, then the
// variant's final conversion (finish, not finish_fold: the product of a
// storage-precision accumulator needs its rounding).  A NaN accumulator is
// stored as the unscaled fold stores it and never reaches the multiplier,
// whose NaN choice is the hardware's.  X = false leaves the select out with
// the other NaN fix-ups: a NaN accumulator makes a NaN row, and every such row
// is refolded with X (x86_refold's screens: a sum is NaN only from a NaN or
// Inf input, and the multiplier is finite and not zero).
template <typename Tag, unsigned V, bool X, typename SC>
__device__ __forceinline__ typename Tr<Tag>::S finish_scaled(typename Tr<Tag>::C acc, uint64_t idx,
                                                             uint64_t trunc_from, const SC& sc) {
    if constexpr (std::is_same<SC, NoScale>::value) {
        return finish_fold<Tag, V, X>(acc, idx, trunc_from);
    } else {
        using C = typename Tr<Tag>::C;
        const auto r = finish<Tag, V, X>(acc * sc.template as<C>(), idx, trunc_from);
        if constexpr (X) return (acc != acc) ? finish_fold<Tag, V, X>(acc, idx, trunc_from) : r;
        else return r;
    }
}


// The avx512fp16 impl's VMINPH/VMAXPH(in, inout) return the selected operand
// as stored; the fp32 route's widening (VCVTPH2PS) has quieted it.  They
// differ only for a signalling NaN, and only the accumulator's start can be
// the NaN a fold returns (a min/max step takes `in` only when in < acc,
// ordered), so the result is that start, as stored, whenever it is a NaN
// (oracle/fp16_native_check.c proves this over all 2^32 operand pairs).
template <typename Tag, int OP, unsigned V>
__device__ __forceinline__ typename Tr<Tag>::S native_minmax(typename Tr<Tag>::S r, typename Tr<Tag>::S acc0) {
    if constexpr (std::is_same<Tag, fp16_tag>::value && (V & V_FP16_NATIVE) && (OP == OP_MIN || OP == OP_MAX)) {
        if (((uint32_t)acc0 & 0x7C00u) == 0x7C00u && ((uint32_t)acc0 & 0x03FFu)) return acc0;
    }
    return r;
}

template <int MEM>
__device__ __forceinline__ u32x4 vload(const u32x4* p) {
    if constexpr (MEM & 1)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}
template <int MEM>
__device__ __forceinline__ void vstore(u32x4* p, u32x4 v) {
    if constexpr (MEM & 2)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// Buffer addressing (cdna_hip_programming.md T8/T20): one SGPR descriptor per
// tile, built from kernel arguments and blockIdx only (wave-uniform), whose
// range is the tile's valid bytes, so out-of-range lanes read zeros and their
// stores are dropped.
constexpr int kAuxNT = 2;      // buffer op aux bit 1: non-temporal (gfx950)
constexpr int kAuxSC1NT = 18;  // sc1 + nt: the store drops the line from L2 instead of keeping it

__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void* base, uint64_t byte0, uint32_t nbytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(base) + byte0), (short)0,
                                             (int)nbytes, 0x00020000);
}

template <typename S>
struct alignas(16) Pack {
    S e[16 / sizeof(S)];
};

// ---------------------------------------------------------------------------
// Fold of one 16-byte vector position across inputs x[0..k) (acc = x[0];
// acc = op(x[i], acc); one final rounding) into the output vector.
// fold_vec_x86 runs it without the NaN fix-ups, then screens the inputs for
// an all-ones exponent (Inf or NaN) — 3 integer ops per dword, on the packed
// words — and refolds the row with them only when one is present.  A
// low-precision sum or product is NaN only from a NaN or Inf operand, except
// a product chain whose partial product overflows to Inf and meets a zero
// (K >= 3), which the screen of the result catches.  The fix-ups cost ~10
// VALU ops per element; on every row they made C3 VALU-bound (28 % slower,
// profiles/round2_nan/).
// ---------------------------------------------------------------------------
template <typename Tag>
__device__ __forceinline__ uint32_t inf_nan_word(uint32_t w) {
    // per 16-bit half (bf16, fp16), per word (fp32) or per high word (fp64):
    // exponent field + one ulp of it carries into the top bit exactly when
    // the field is all ones
    if constexpr (std::is_same<Tag, bf16_tag>::value) return (w & 0x7F807F80u) + 0x00800080u;
    else if constexpr (std::is_same<Tag, fp16_tag>::value) return (w & 0x7C007C00u) + 0x04000400u;
    else if constexpr (std::is_same<Tag, double>::value) return (w & 0x7FF00000u) + 0x00100000u;
    else return (w & 0x7F800000u) + 0x00800000u;
}
template <typename Tag>
__device__ __forceinline__ uint32_t inf_nan_bits(u32x4 v) {
    if constexpr (std::is_same<Tag, double>::value) return inf_nan_word<Tag>(v.y) | inf_nan_word<Tag>(v.w);
    return inf_nan_word<Tag>(v.x) | inf_nan_word<Tag>(v.y) | inf_nan_word<Tag>(v.z) | inf_nan_word<Tag>(v.w);
}
template <typename Tag>
__device__ __forceinline__ bool inf_nan_hit(uint32_t bits) {
    return (bits & (sizeof(typename Tr<Tag>::S) == 2 ? 0x80008000u : 0x80000000u)) != 0u;
}

template <typename Tag, int OP, unsigned V, bool X, int KMAX, typename SC = NoScale>
__device__ __forceinline__ u32x4 fold_vec(const u32x4 (&x)[KMAX], int k, uint64_t e0, uint64_t trunc_from,
                                          const SC& sc = SC()) {
    using S = typename Tr<Tag>::S;
    using C = typename Tr<Tag>::C;
    constexpr int N = 16 / sizeof(S);
    C acc[N];
    const Pack<S> p0 = __builtin_bit_cast(Pack<S>, x[0]);
#pragma unroll
    for (int e = 0; e < N; e++) acc[e] = widen<Tag>(p0.e[e]);
#pragma unroll
    for (int i = 1; i < KMAX; i++) {
        if (i < k) {
            const Pack<S> pi = __builtin_bit_cast(Pack<S>, x[i]);
#pragma unroll
            for (int e = 0; e < N; e++) acc[e] = step<Tag, OP, V, X>(widen<Tag>(pi.e[e]), acc[e]);
        }
    }
    Pack<S> pr;
#pragma unroll
    for (int e = 0; e < N; e++) {
        pr.e[e] = finish_scaled<Tag, V, X>(acc[e], e0 + e, trunc_from, sc);
        if constexpr (X) pr.e[e] = native_minmax<Tag, OP, V>(pr.e[e], p0.e[e]);  // NaN rows take X
    }
    return __builtin_bit_cast(u32x4, pr);
}

// r = the fast fold of x; refold with the fix-ups when the screen hits.
// Low precision: screen the inputs (and a K-input product's result).
// float / double sum and prod: a NaN operand or an invalid operation makes
// the result NaN, and a NaN stays NaN along the fold, so the result's own
// screen finds every row to fix: one unordered compare per element (an
// integer exponent screen cost C2 ~3 %, profiles/round3_run2).  Other types
// and ops: a no-op.
template <typename Tag, int OP, unsigned V, int KMAX, typename SC = NoScale>
__device__ __forceinline__ u32x4 x86_refold(u32x4 r, const u32x4 (&x)[KMAX], int k, uint64_t e0,
                                            uint64_t trunc_from, const SC& sc = SC()) {
    if constexpr (Tr<Tag>::lp) {
        uint32_t bits = inf_nan_bits<Tag>(x[0]);
#pragma unroll
        for (int i = 1; i < KMAX; i++)
            if (i < k) bits |= inf_nan_bits<Tag>(x[i]);
        if constexpr (OP == OP_PROD && KMAX > 2) bits |= inf_nan_bits<Tag>(r);
        if (__builtin_expect(inf_nan_hit<Tag>(bits), 0)) r = fold_vec<Tag, OP, V, true, KMAX>(x, k, e0, trunc_from, sc);
    } else if constexpr (Tr<Tag>::fp && (OP == OP_SUM || OP == OP_PROD)) {
        // unordered self-compares: one v_cmp_u per element pair into a lane mask
        const Pack<Tag> p = __builtin_bit_cast(Pack<Tag>, r);
        bool nan = false;
#pragma unroll
        for (int e = 0; e < 16 / (int)sizeof(Tag); e++) nan |= (p.e[e] != p.e[e]);
        if (__builtin_expect(nan, 0)) r = fold_vec<Tag, OP, V, true, KMAX>(x, k, e0, trunc_from, sc);
    }
    return r;
}

template <typename Tag, int OP, unsigned V, int KMAX>
__device__ __forceinline__ u32x4 fold_vec_x86(const u32x4 (&x)[KMAX], int k, uint64_t e0, uint64_t trunc_from) {
    return x86_refold<Tag, OP, V, KMAX>(fold_vec<Tag, OP, V, false, KMAX>(x, k, e0, trunc_from), x, k, e0,
                                        trunc_from);
}

template <typename Tag>
__device__ __forceinline__ bool row_has_nan(u32x4 r) {
    const Pack<Tag> p = __builtin_bit_cast(Pack<Tag>, r);
    bool nan = false;
#pragma unroll
    for (int e = 0; e < 16 / (int)sizeof(Tag); e++) nan |= (p.e[e] != p.e[e]);
    return nan;
}

// fold_vec_x86 for the lean kernels.  float / double sum and prod: the rare
// NaN row re-reads its inputs (`reload(y)`) instead of keeping x live past the
// fold; kept live, they made the compiler split the guarded load / add / store
// row into three exec-masked blocks and cost the C2 kernel ~3 %
// (profiles/round3_run2).  The compiler barrier stops the re-read from being
// folded into the first read.  Other types: fold_vec_x86.
template <typename Tag, int OP, unsigned V, int KMAX, typename Reload>
__device__ __forceinline__ u32x4 fold_row(const u32x4 (&x)[KMAX], int k, uint64_t e0, uint64_t trunc_from,
                                          Reload&& reload) {
    if constexpr (!Tr<Tag>::lp && Tr<Tag>::fp && (OP == OP_SUM || OP == OP_PROD)) {
        u32x4 r = fold_vec<Tag, OP, V, false, KMAX>(x, k, e0, trunc_from);
        if (__builtin_expect(row_has_nan<Tag>(r), 0)) {
            asm volatile("" ::: "memory");
            u32x4 y[KMAX];
            reload(y);
            r = fold_vec<Tag, OP, V, true, KMAX>(y, k, e0, trunc_from);
        }
        return r;
    } else {
        return fold_vec_x86<Tag, OP, V, KMAX>(x, k, e0, trunc_from);
    }
}

// ---------------------------------------------------------------------------
// Packed 8- and 16-bit integer ops on whole dwords: acc' = op(in, acc) per
// byte / half, with CCL_REDUCE's wrap-around sum and prod.  Unpacking 16 bytes
// of each of up to 16 inputs cost the fan-in 258 VGPRs, one wave per SIMD and
// 1.7 TB/s (profiles/round1_misalign.jsonl).  Packed, the fold stays in the 4
// dwords of the loaded vector.  16-bit lanes map to gfx950's v_pk_*_{i,u}16;
// bytes run as even/odd halves of those, and sum uses the carry-free SWAR add.
// min/max of integers have no tie or NaN cases, so operand order is moot.
// ---------------------------------------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

template <typename V2>
__device__ __forceinline__ V2 as2(uint32_t x) { return __builtin_bit_cast(V2, x); }
template <typename V2>
__device__ __forceinline__ uint32_t as1(V2 x) { return __builtin_bit_cast(uint32_t, x); }

template <int OP, bool SIGNED>
__device__ __forceinline__ uint32_t pk16_op(uint32_t in, uint32_t acc) {
    if constexpr (OP == OP_SUM) return as1(as2<u16x2>(acc) + as2<u16x2>(in));
    if constexpr (OP == OP_PROD) return as1(as2<u16x2>(acc) * as2<u16x2>(in));
    if constexpr (SIGNED) {
        if constexpr (OP == OP_MIN) return as1(__builtin_elementwise_min(as2<i16x2>(acc), as2<i16x2>(in)));
        if constexpr (OP == OP_MAX) return as1(__builtin_elementwise_max(as2<i16x2>(acc), as2<i16x2>(in)));
    } else {
        if constexpr (OP == OP_MIN) return as1(__builtin_elementwise_min(as2<u16x2>(acc), as2<u16x2>(in)));
        if constexpr (OP == OP_MAX) return as1(__builtin_elementwise_max(as2<u16x2>(acc), as2<u16x2>(in)));
    }
}

template <int OP, bool SIGNED>
__device__ __forceinline__ uint32_t pk8_op(uint32_t in, uint32_t acc) {
    constexpr uint32_t lo7 = 0x7F7F7F7Fu, hi1 = 0x80808080u, evn = 0x00FF00FFu;
    if constexpr (OP == OP_SUM) return ((acc & lo7) + (in & lo7)) ^ ((acc ^ in) & hi1);
    if constexpr (OP == OP_PROD) {  // low byte of each 16-bit product
        const uint32_t pe = as1(as2<u16x2>(acc & evn) * as2<u16x2>(in & evn));
        const uint32_t po = as1(as2<u16x2>((acc >> 8) & evn) * as2<u16x2>((in >> 8) & evn));
        return (pe & evn) | ((po & evn) << 8);
    }
    if constexpr (SIGNED) {  // sign-extend even / odd bytes into 16-bit lanes
        const i16x2 ae = as2<i16x2>(acc << 8) >> 8, ie = as2<i16x2>(in << 8) >> 8;
        const i16x2 ao = as2<i16x2>(acc) >> 8, io = as2<i16x2>(in) >> 8;
        i16x2 re, ro;
        if constexpr (OP == OP_MIN) {
            re = __builtin_elementwise_min(ae, ie);
            ro = __builtin_elementwise_min(ao, io);
        } else {
            re = __builtin_elementwise_max(ae, ie);
            ro = __builtin_elementwise_max(ao, io);
        }
        return (as1(re) & evn) | ((as1(ro) & evn) << 8);
    } else {
        const u16x2 ae = as2<u16x2>(acc & evn), ie = as2<u16x2>(in & evn);
        const u16x2 ao = as2<u16x2>((acc >> 8) & evn), io = as2<u16x2>((in >> 8) & evn);
        u16x2 re, ro;
        if constexpr (OP == OP_MIN) {
            re = __builtin_elementwise_min(ae, ie);
            ro = __builtin_elementwise_min(ao, io);
        } else {
            re = __builtin_elementwise_max(ae, ie);
            ro = __builtin_elementwise_max(ao, io);
        }
        return as1(re) | (as1(ro) << 8);
    }
}

// 8/16-bit integer storage: the fold runs packed on dwords
template <typename Tag>
constexpr bool packed_int() {
    return std::is_integral<Tag>::value && sizeof(Tag) <= 2;
}

template <typename Tag, int OP>
__device__ __forceinline__ u32x4 pk_op4(u32x4 in, u32x4 acc) {
    constexpr bool sg = std::is_signed<Tag>::value;
    u32x4 r;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        if constexpr (sizeof(Tag) == 1)
            r[d] = pk8_op<OP, sg>(in[d], acc[d]);
        else
            r[d] = pk16_op<OP, sg>(in[d], acc[d]);
    }
    return r;
}

// ---------------------------------------------------------------------------
// What every kernel below shares: the scalar fold of one element, the
// geometry of one tile, and the head / tail duty of block 0.
// ---------------------------------------------------------------------------

// The scalar path (head, tail, element loop): element `idx` of the fold of
// in[0..k), as stored.
template <typename Tag, int OP, unsigned V, typename SC = NoScale>
__device__ __forceinline__ typename Tr<Tag>::S fold_elem(const void* const* in, int k, uint64_t idx,
                                                         uint64_t trunc_from, const SC& sc = SC()) {
    using S = typename Tr<Tag>::S;
    using C = typename Tr<Tag>::C;
    const S s0 = static_cast<const S*>(in[0])[idx];
    C acc = widen<Tag>(s0);
    for (int i = 1; i < k; i++) acc = step<Tag, OP, V>(widen<Tag>(static_cast<const S*>(in[i])[idx]), acc);
    return native_minmax<Tag, OP, V>(finish_scaled<Tag, V, true>(acc, idx, trunc_from, sc), s0);
}

template <typename Tag, int OP, unsigned V>
__device__ __forceinline__ void reduce_elem(const KArgs& a, int k, uint64_t idx) {
    static_cast<typename Tr<Tag>::S*>(a.out)[idx] = fold_elem<Tag, OP, V>(a.in, k, idx, a.trunc_from);
}

// Tile `tile` of VECS 16-byte vectors in a body of `nvec` vectors that starts
// `head_bytes` into every operand.  Each stream gets one buffer descriptor
// tile_rsrc(base, byte0, bytes) per tile, so lanes past the end read zeros
// and their stores are dropped: no guard branches.
struct Tile {
    uint64_t t0;     // the tile's first vector
    uint64_t byte0;  // its byte offset from the operands' bases
    uint32_t bytes;  // its valid bytes (0 for a tile past the end)
    uint32_t off;    // this lane's byte offset in the tile (its first vector)
};
template <int VECS>
__device__ __forceinline__ Tile tile_of(uint64_t tile, uint64_t nvec, uint64_t head_bytes) {
    Tile t;
    t.t0 = tile * VECS;
    const uint64_t left = nvec > t.t0 ? nvec - t.t0 : 0;
    t.bytes = (uint32_t)(left < (uint64_t)VECS ? left : (uint64_t)VECS) * 16u;
    t.byte0 = head_bytes + t.t0 * 16;
    t.off = threadIdx.x * 16u;
    return t;
}

// The first lanes of block 0 do the scalar head [0, head) and tail
// [tail0, tail0 + tail), fewer than 16 elements (bytes, for a copy) each.
template <typename H, typename F>
__device__ __forceinline__ void head_tail(uint32_t blk, H head, H tail, uint64_t tail0, F&& elem) {
    if (blk == 0) {
        if (threadIdx.x < head) elem(threadIdx.x);
        if (threadIdx.x < tail) elem(tail0 + threadIdx.x);
    }
}

// One tile row: U vectors per lane at v0, v0+B, ...  GUARD = last tile.
template <typename Tag, int OP, unsigned V, int KT, int U, int MEM, bool GUARD, int B>
__device__ __forceinline__ void reduce_tile(const KArgs& a, int k, uint64_t v0) {
    using S = typename Tr<Tag>::S;
    using C = typename Tr<Tag>::C;
    constexpr int N = 16 / sizeof(S);
    const uint64_t hb = a.head * sizeof(S);

    C acc[U][N];
    u32x4 cur[U];
    constexpr bool kNative = std::is_same<Tag, fp16_tag>::value && (V & V_FP16_NATIVE) && (OP == OP_MIN || OP == OP_MAX);
    u32x4 raw0[kNative ? U : 1];  // the accumulator's start as stored (native_minmax)

    const u32x4* p0 = reinterpret_cast<const u32x4*>(static_cast<const char*>(a.in[0]) + hb);
    const u32x4* p1 =
        reinterpret_cast<const u32x4*>(static_cast<const char*>(a.in[(KT == 2 || k >= 2) ? 1 : 0]) + hb);
    // issue input 0 and input 1 loads back to back (2*U*16 B in flight per lane)
#pragma unroll
    for (int j = 0; j < U; j++) {
        const uint64_t v = v0 + (uint64_t)j * B;
        if (!GUARD || v < a.nvec) {
            u32x4 r = vload<MEM>(p0 + v);
            if constexpr (kNative) raw0[j] = r;
            Pack<S> p = __builtin_bit_cast(Pack<S>, r);
#pragma unroll
            for (int e = 0; e < N; e++) acc[j][e] = widen<Tag>(p.e[e]);
        }
    }
    if (KT == 2 || k >= 2) {
#pragma unroll
        for (int j = 0; j < U; j++) {
            const uint64_t v = v0 + (uint64_t)j * B;
            cur[j] = u32x4{0u, 0u, 0u, 0u};
            if (!GUARD || v < a.nvec) cur[j] = vload<MEM>(p1 + v);
        }
    }

    if constexpr (KT == 2) {
#pragma unroll
        for (int j = 0; j < U; j++) {
            Pack<S> p = __builtin_bit_cast(Pack<S>, cur[j]);
#pragma unroll
            for (int e = 0; e < N; e++) acc[j][e] = step<Tag, OP, V>(widen<Tag>(p.e[e]), acc[j][e]);
        }
    } else {
        for (int i = 1; i < k; i++) {
            // prefetch input i+1 while combining input i
            u32x4 nxt[U];
            if (i + 1 < k) {
                const u32x4* pn =
                    reinterpret_cast<const u32x4*>(static_cast<const char*>(a.in[i + 1]) + hb);
#pragma unroll
                for (int j = 0; j < U; j++) {
                    const uint64_t v = v0 + (uint64_t)j * B;
                    nxt[j] = u32x4{0u, 0u, 0u, 0u};
                    if (!GUARD || v < a.nvec) nxt[j] = vload<MEM>(pn + v);
                }
            }
#pragma unroll
            for (int j = 0; j < U; j++) {
                Pack<S> p = __builtin_bit_cast(Pack<S>, cur[j]);
#pragma unroll
                for (int e = 0; e < N; e++) acc[j][e] = step<Tag, OP, V>(widen<Tag>(p.e[e]), acc[j][e]);
            }
            if (i + 1 < k) {
#pragma unroll
                for (int j = 0; j < U; j++) cur[j] = nxt[j];
            }
        }
    }

    u32x4* po = reinterpret_cast<u32x4*>(static_cast<char*>(a.out) + hb);
#pragma unroll
    for (int j = 0; j < U; j++) {
        const uint64_t v = v0 + (uint64_t)j * B;
        if (!GUARD || v < a.nvec) {
            Pack<S> p;
#pragma unroll
            for (int e = 0; e < N; e++)
                p.e[e] = finish_fold<Tag, V>(acc[j][e], a.head + v * N + e, a.trunc_from);
            if constexpr (kNative) {
                const Pack<S> s0 = __builtin_bit_cast(Pack<S>, raw0[j]);
#pragma unroll
                for (int e = 0; e < N; e++) p.e[e] = native_minmax<Tag, OP, V>(p.e[e], s0.e[e]);
            }
            vstore<MEM>(po + v, __builtin_bit_cast(u32x4, p));
        }
    }
}

// Grid-stride over tiles of B*U vectors (B threads per block).  Block 0 also does the
// scalar head/tail (< 16 elements each).  `scalar_only` = operands with
// different misalignments: plain element loop.
// MAP 1: blocks b, b+8, b+16, ... (one XCD under the observed round-robin
// dispatch, MI355X_MICROARCH.md §Workgroup dispatch) take one contiguous
// 1/8 of the tiles (grid must be a multiple of 8; speed only, never
// correctness: every tile is still covered exactly once).
template <typename Tag, int OP, unsigned V, int KT, int U, int MEM, int MAP = 0, int B = kBlock>
__global__ __launch_bounds__(B) void reduce_kernel(KArgs a) {
    const int k = (KT > 0) ? KT : a.k;
    if (a.scalar_only) {
        for (uint64_t i = (uint64_t)blockIdx.x * B + threadIdx.x; i < a.count;
             i += (uint64_t)gridDim.x * B)
            reduce_elem<Tag, OP, V>(a, k, i);
        return;
    }
    using S = typename Tr<Tag>::S;
    constexpr int N = 16 / sizeof(S);
    head_tail(blockIdx.x, a.head, a.tail, a.head + a.nvec * N, [&](uint64_t i) { reduce_elem<Tag, OP, V>(a, k, i); });
    const uint64_t tile = (uint64_t)B * U;
    const uint64_t stride = (uint64_t)gridDim.x * tile;
    uint64_t b = blockIdx.x;
    if constexpr (MAP == 1) b = (uint64_t)(blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;
    for (uint64_t base = b * tile; base < a.nvec; base += stride) {
        if (base + tile <= a.nvec)
            reduce_tile<Tag, OP, V, KT, U, MEM, false, B>(a, k, base + threadIdx.x);
        else
            reduce_tile<Tag, OP, V, KT, U, MEM, true, B>(a, k, base + threadIdx.x);
    }
}

// ---------------------------------------------------------------------------
// Lean 2-input kernel (the ccl_comp_reduce case): one tile of B*U vectors per
// block, three pointers, no grid-stride loop.  Per-thread work is a handful
// of address ops around the loads — with 1-vector-per-lane tiles the general
// kernel's argument block and loop structure cost 10-15 % of HBM rate
// (profiles/round1_sweep5_block.jsonl).  Block 0 also does the scalar head
// and tail.  Same element semantics as reduce_kernel (step / finish).
// ---------------------------------------------------------------------------
struct R2Args {
    const void* acc;  // the `inout` role (accumulator start)
    const void* in;   // the `in` role
    void* out;
    uint64_t nvec;        // 16-byte vectors in the aligned body
    uint32_t head, tail;  // scalar elements before / after the body
    uint64_t trunc_from;  // V_TAIL_TRUNC threshold (element index)
};

template <typename Tag, int OP, unsigned V>
__device__ __forceinline__ void reduce2_elem(const R2Args& a, uint64_t idx) {
    const void* const in[2] = {a.acc, a.in};
    static_cast<typename Tr<Tag>::S*>(a.out)[idx] = fold_elem<Tag, OP, V>(in, 2, idx, a.trunc_from);
}

// One tile (block `blk` of the operand set `a`): the body of reduce2_kernel,
// shared with the descriptor-batched form below.
template <typename Tag, int OP, unsigned V, int U, int B>
__device__ __forceinline__ void reduce2_tile(const R2Args& a, uint32_t blk) {
    using S = typename Tr<Tag>::S;
    constexpr int N = 16 / sizeof(S);
    // Head / tail and the tile's geometry are written out here, not through
    // head_tail and tile_of: with them the bf16 RNE form took one VGPR more
    // (40 -> 41), int64 three (9 -> 12), and the 256 MiB bf16 sum ran at
    // 1.0007 and 1.0024 of this form's time where the same build against
    // itself gave 0.9997 and 1.0001 (tools/ab_c2.py, profiles/fold_refactor/).
    if (blk == 0) {
        if (threadIdx.x < a.head) reduce2_elem<Tag, OP, V>(a, threadIdx.x);
        if (threadIdx.x < a.tail) reduce2_elem<Tag, OP, V>(a, a.head + a.nvec * N + threadIdx.x);
    }
    const size_t hb = (size_t)a.head * sizeof(S);
    // Every operand through a buffer descriptor per tile (base = the tile's
    // first vector, range = its valid bytes; lanes past the end read zeros
    // and their stores are dropped).  Loads nt: against the global nt loads
    // of rounds 1-5 the same fold ran 0.3-0.5 % faster at the median and in
    // each of 16 fresh placements per layout (tools/r2_load_ab.py), and the
    // library built this way 0.2-0.5 % faster than the round-5 build over 10
    // fresh placements per config, C3 bf16 within noise (tools/ab_c2.py
    // --trials; both in profiles/round6_run6/).  Stores sc1 + nt drop each line from L2 as it
    // is written; nt alone keeps it there, and the 2-input stream then ran
    // 2.3-3.1 % slower (tools/occupancy_sweep.hip policy,
    // profiles/round3_occupancy/).  The fan-in keeps nt (sc1 did not pay there).
    const uint64_t t0 = (uint64_t)blk * (B * U);
    const uint64_t tleft = a.nvec > t0 ? a.nvec - t0 : 0;
    const uint32_t tbytes = (uint32_t)(tleft < (uint64_t)B * U ? tleft : (uint64_t)B * U) * 16u;
    const uint64_t tb = hb + t0 * 16;
    const __amdgpu_buffer_rsrc_t arsrc = tile_rsrc(a.acc, tb, tbytes);
    const __amdgpu_buffer_rsrc_t irsrc = tile_rsrc(a.in, tb, tbytes);
    const __amdgpu_buffer_rsrc_t orsrc = tile_rsrc(a.out, tb, tbytes);
    const uint64_t v0 = t0 + threadIdx.x;
    u32x4 x[U], y[U];
#pragma unroll
    for (int j = 0; j < U; j++)
        x[j] = __builtin_amdgcn_raw_buffer_load_b128(arsrc, (uint32_t)(j * B + threadIdx.x) * 16u, 0, kAuxNT);
#pragma unroll
    for (int j = 0; j < U; j++)
        y[j] = __builtin_amdgcn_raw_buffer_load_b128(irsrc, (uint32_t)(j * B + threadIdx.x) * 16u, 0, kAuxNT);
#pragma unroll
    for (int j = 0; j < U; j++) {
        const uint64_t v = v0 + (uint64_t)j * B;
        if (v < a.nvec) {
            const uint32_t off = (uint32_t)(v - t0) * 16u;
            const u32x4 xs[2] = {x[j], y[j]};
            __builtin_amdgcn_raw_buffer_store_b128(
                fold_row<Tag, OP, V, 2>(xs, 2, a.head + v * N, a.trunc_from, [&](u32x4 (&r)[2]) {
                    r[0] = __builtin_amdgcn_raw_buffer_load_b128(arsrc, off, 0, kAuxNT);
                    r[1] = __builtin_amdgcn_raw_buffer_load_b128(irsrc, off, 0, kAuxNT);
                }),
                orsrc, off, 0, kAuxSC1NT);
        }
    }
}

template <typename Tag, int OP, unsigned V, int U, int B>
__global__ __launch_bounds__(B) void reduce2_kernel(R2Args a) {
    reduce2_tile<Tag, OP, V, U, B>(a, blockIdx.x);
}

// ---------------------------------------------------------------------------
// Descriptor-batched 2-input reduce: up to kBatchMax independent
// (acc, in, out) operand sets in one launch, each cut into reduce2_kernel's
// tiles.  Block b works on descriptor d = the last one with block0[d] <= b
// (a uniform binary search over the kernarg table), tile b - block0[d].  For
// schedules with many small chunks in one phase: one dispatch instead of one
// per chunk (sub-MiB reduces are dispatch-bound).
// ---------------------------------------------------------------------------
constexpr int kBatchMax = 64;

struct BArgs {
    const void* acc[kBatchMax];
    const void* in[kBatchMax];
    void* out[kBatchMax];
    uint64_t nvec[kBatchMax];
    uint64_t trunc_from[kBatchMax];
    uint8_t head[kBatchMax], tail[kBatchMax];  // < 16 elements each
    uint32_t block0[kBatchMax + 1];             // first block of each descriptor; [n] = grid size
    int n;
};

template <typename Tag, int OP, unsigned V, int U, int B>
__global__ __launch_bounds__(B) void reduce2_batch_kernel(BArgs a) {
    const uint32_t b = blockIdx.x;
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.block0[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    R2Args r;
    r.acc = a.acc[lo];
    r.in = a.in[lo];
    r.out = a.out[lo];
    r.nvec = a.nvec[lo];
    r.head = a.head[lo];
    r.tail = a.tail[lo];
    r.trunc_from = a.trunc_from[lo];
    reduce2_tile<Tag, OP, V, U, B>(r, b - a.block0[lo]);
}

// ---------------------------------------------------------------------------
// One-wave fan kernels (cdna_hip_programming.md T8/T20).  Each block owns one
// tile of B vectors.  Every stream gets one SGPR descriptor per tile, built
// from kernel arguments and blockIdx only (wave-uniform, so no waterfall).
// Lanes carry only a 32-bit byte offset.
// ---------------------------------------------------------------------------

// The fold of one tile, shared by fan_kernel and bcast_kernel: all k
// (2..KMAX; bcast also 1) loads are issued before the first combine (uniform
// branches on k only), then the left fold in the reference's order
// (acc = in[0]; acc = op(in[j], acc)).  Returns the lane's result vector;
// x0 = its vector of in[0] as loaded (bcast's k = 1 rule).  `ain` is the
// kernel argument's pointer list.
template <typename Tag, int OP, unsigned V, int KMAX, typename SC = NoScale>
__device__ __forceinline__ u32x4 fan_fold(const void* const (&ain)[kMaxInputs], int k, const Tile& t,
                                          uint64_t head, uint64_t trunc_from, u32x4& x0, const SC& sc = SC()) {
    using S = typename Tr<Tag>::S;
    constexpr int N = 16 / sizeof(S);
    // Materialise every input pointer before the first branch: left alone, the
    // compiler sinks each kernarg load into its `i < k` block and every buffer
    // load then waits on its own scalar load.
    const void* in[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; i++) {
        in[i] = ain[i];
        asm volatile("" ::"s"(in[i]));
    }
    u32x4 x[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; i++)
        if (i < k) x[i] = __builtin_amdgcn_raw_buffer_load_b128(tile_rsrc(in[i], t.byte0, t.bytes), t.off, 0, kAuxNT);
    x0 = x[0];
    if constexpr (packed_int<Tag>()) {
        u32x4 r = x[0];
#pragma unroll
        for (int i = 1; i < KMAX; i++)
            if (i < k) r = pk_op4<Tag, OP>(x[i], r);
        return r;
    } else {
        // The fast fold is written out here rather than through fold_vec: with
        // the runtime-k loop in a callee, the compiler kept the fp32 8-input
        // form's x[] as an aggregate and spilled it to scratch (33 ms instead of
        // 1.6 ms per GiB; tests/test_kernel_resources.py guards every kernel).
        using C = typename Tr<Tag>::C;
        C acc[N];
        const Pack<S> p0 = __builtin_bit_cast(Pack<S>, x[0]);
#pragma unroll
        for (int e = 0; e < N; e++) acc[e] = widen<Tag>(p0.e[e]);
#pragma unroll
        for (int i = 1; i < KMAX; i++) {
            if (i < k) {
                const Pack<S> pi = __builtin_bit_cast(Pack<S>, x[i]);
#pragma unroll
                for (int e = 0; e < N; e++) acc[e] = step<Tag, OP, V, false>(widen<Tag>(pi.e[e]), acc[e]);
            }
        }
        Pack<S> pr;
        const uint64_t e0 = head + (t.t0 + threadIdx.x) * N;
#pragma unroll
        for (int e = 0; e < N; e++) pr.e[e] = finish_scaled<Tag, V, false>(acc[e], e0 + e, trunc_from, sc);
        return x86_refold<Tag, OP, V, KMAX>(__builtin_bit_cast(u32x4, pr), x, k, e0, trunc_from, sc);
    }
}

// Fan-in with a runtime K (2..kMaxInputs).  Common alignment required;
// head/tail by block 0 through the scalar element path.
template <typename Tag, int OP, unsigned V, int B, int KMAX = kMaxInputs>
__global__ __launch_bounds__(B) void fan_kernel(KArgs a) {
    constexpr int N = 16 / sizeof(typename Tr<Tag>::S);
    const int k = a.k;
    head_tail(blockIdx.x, a.head, a.tail, a.head + a.nvec * N, [&](uint64_t i) { reduce_elem<Tag, OP, V>(a, k, i); });
    const Tile t = tile_of<B>(blockIdx.x, a.nvec, a.head * sizeof(typename Tr<Tag>::S));
    if (t.t0 >= a.nvec) return;
    if constexpr (std::is_same<Tag, fp16_tag>::value) {
        // fp16 keeps fan_fold's text written out in the kernel.  Through the
        // callee its forms took 6-9 VGPRs more (46 -> 53, 48 -> 57, 78 -> 85,
        // 81 -> 89) and the 8-input 256 MiB sum ran at 1.0035 of this form's
        // time, every one of 12 placements at or above 1.0000, where the same
        // build against itself gave 0.9986 (tools/ab_c2.py,
        // profiles/fold_refactor/).  Not the cause, each tried alone: the
        // element index, head_tail, Tile, the returned x[0], reference or value
        // parameters, the store passed in as a functor.
        using S = uint16_t;
        const void* in[KMAX];
#pragma unroll
        for (int i = 0; i < KMAX; i++) {
            in[i] = a.in[i];
            asm volatile("" ::"s"(in[i]));
        }
        u32x4 x[KMAX];
#pragma unroll
        for (int i = 0; i < KMAX; i++)
            if (i < k) x[i] = __builtin_amdgcn_raw_buffer_load_b128(tile_rsrc(in[i], t.byte0, t.bytes), t.off, 0, kAuxNT);
        float acc[N];
        const Pack<S> p0 = __builtin_bit_cast(Pack<S>, x[0]);
#pragma unroll
        for (int e = 0; e < N; e++) acc[e] = widen<Tag>(p0.e[e]);
#pragma unroll
        for (int i = 1; i < KMAX; i++) {
            if (i < k) {
                const Pack<S> pi = __builtin_bit_cast(Pack<S>, x[i]);
#pragma unroll
                for (int e = 0; e < N; e++) acc[e] = step<Tag, OP, V, false>(widen<Tag>(pi.e[e]), acc[e]);
            }
        }
        Pack<S> pr;
        const uint64_t e0 = a.head + (t.t0 + threadIdx.x) * N;
#pragma unroll
        for (int e = 0; e < N; e++) pr.e[e] = finish_fold<Tag, V, false>(acc[e], e0 + e, a.trunc_from);
        __builtin_amdgcn_raw_buffer_store_b128(
            x86_refold<Tag, OP, V, KMAX>(__builtin_bit_cast(u32x4, pr), x, k, e0, a.trunc_from),
            tile_rsrc(a.out, t.byte0, t.bytes), t.off, 0, kAuxNT);
    } else {
        u32x4 x0;
        const u32x4 r = fan_fold<Tag, OP, V, KMAX>(a.in, k, t, a.head, a.trunc_from, x0);
        __builtin_amdgcn_raw_buffer_store_b128(r, tile_rsrc(a.out, t.byte0, t.bytes), t.off, 0, kAuxNT);
    }
}

// ---------------------------------------------------------------------------
// Fold K inputs once, write the result to M outputs (mi_reduce_bcast): the
// step that completes an allreduce on the GPU.  The reference does it as
// allreduce_kernel_* (out = peer_out = op(in, peer_in),
// src/kernels/kernels.cl:190-217) and as reduce_monolithic_kernel_N followed
// by write_monolithic_kernel_N (kernels.cl:269-421, 424-560).  The fold is
// fan_fold, the one fan_kernel runs; the vector grid is the outputs' common 16-byte
// grid.  An output may be exactly one of the inputs (in place): such an input
// has the outputs' misalignment, so a lane loads exactly the bytes it later
// stores, and every lane has all k loads back (the refold keeps them in
// registers: no re-load) before its first store.
//   mi_reduce_bcast_scaled runs the same bodies with a multiplier in the
// finish step (finish_scaled), selected at compile time by the SC parameter:
// kernels of their own, sum on the floating types only, for every (k, m).
// The multiply sits after the last combine, so the order of loads and stores,
// and with it the in-place argument above, is unchanged.
// ---------------------------------------------------------------------------
struct BCArgs {
    const void* in[kMaxInputs];  // in[0] = accumulator start
    void* out[kMaxInputs];       // m destinations, all at one misalignment on the vector path
    uint64_t nvec;        // 16-byte vectors in the aligned body
    uint64_t head;        // leading scalar elements (the outputs' misalignment)
    uint64_t tail;        // trailing scalar elements
    uint64_t count;       // total elements
    uint64_t trunc_from;  // V_TAIL_TRUNC threshold (element index)
    int k;                // inputs
    int m;                // outputs
    int scalar_only;      // outputs misaligned differently / operands not element-aligned: element loop
    int store_sc1;        // stores sc1 + nt instead of nt (tuning knob, mi_set_bcast_store)
};

// k = 1 in storage precision folds nothing: mi_reduce_multi copies the bytes,
// so the fan-out does too (a rounding step would quiet a signalling fp16 NaN).
template <typename Tag, unsigned V>
constexpr bool bcast_copies_k1() {
    return Tr<Tag>::lp && !(V & V_ACC_FP32);
}

// The k = 1 rule on a lane's result vector `r`, x0 = its vector of in[0] as
// loaded.  Unscaled: x0.  Scaled: the unscaled store is in[0]'s bytes, so a
// NaN goes out as loaded (the rounding in `r` has quieted a signalling fp16
// NaN); every other element is the scaled one.
template <typename Tag, typename SC>
__device__ __forceinline__ u32x4 bcast_k1(u32x4 r, u32x4 x0) {
    if constexpr (std::is_same<SC, NoScale>::value) {
        return x0;
    } else {
        using S = typename Tr<Tag>::S;
        Pack<S> pr = __builtin_bit_cast(Pack<S>, r);
        const Pack<S> p0 = __builtin_bit_cast(Pack<S>, x0);
#pragma unroll
        for (int e = 0; e < 16 / (int)sizeof(S); e++) {
            const typename Tr<Tag>::C w = widen<Tag>(p0.e[e]);
            pr.e[e] = (w != w) ? p0.e[e] : pr.e[e];
        }
        return __builtin_bit_cast(u32x4, pr);
    }
}

template <typename Tag, int OP, unsigned V, typename SC = NoScale>
__device__ __forceinline__ void bcast_elem(const BCArgs& a, int k, int m, uint64_t idx, const SC& sc = SC()) {
    using S = typename Tr<Tag>::S;
    S r = fold_elem<Tag, OP, V>(a.in, k, idx, a.trunc_from, sc);
    if constexpr (bcast_copies_k1<Tag, V>()) {
        if constexpr (std::is_same<SC, NoScale>::value) {
            r = (k == 1) ? static_cast<const S*>(a.in[0])[idx] : r;
        } else if (k == 1) {  // bcast_k1's rule
            const S s0 = static_cast<const S*>(a.in[0])[idx];
            const typename Tr<Tag>::C w = widen<Tag>(s0);
            r = (w != w) ? s0 : r;
        }
    }
    for (int o = 0; o < m; o++) static_cast<S*>(a.out[o])[idx] = r;
}

// Shared tail of the two kernels below: the m stores of a lane's result, a
// wave-uniform loop over the output pointers (one descriptor per iteration,
// read from the kernel arguments by a uniform index: no per-lane array).
__device__ __forceinline__ void bcast_store(const BCArgs& a, int m, u32x4 r, const Tile& t) {
    if (a.store_sc1) {
#pragma nounroll
        for (int o = 0; o < m; o++)
            __builtin_amdgcn_raw_buffer_store_b128(r, tile_rsrc(a.out[o], t.byte0, t.bytes), t.off, 0, kAuxSC1NT);
    } else {
#pragma nounroll
        for (int o = 0; o < m; o++)
            __builtin_amdgcn_raw_buffer_store_b128(r, tile_rsrc(a.out[o], t.byte0, t.bytes), t.off, 0, kAuxNT);
    }
}

// One tile of B vectors per block: fan_fold (all k loads before the first
// combine), then the m stores.  bcast_kernel and bcast_scaled_kernel are this
// body without and with a multiplier.
template <typename Tag, int OP, unsigned V, int B, int KMAX, typename SC>
__device__ __forceinline__ void bcast_tile(const BCArgs& a, const SC& sc) {
    constexpr int N = 16 / sizeof(typename Tr<Tag>::S);
    const int k = a.k, m = a.m;
    head_tail(blockIdx.x, a.head, a.tail, a.head + a.nvec * N,
              [&](uint64_t i) { bcast_elem<Tag, OP, V>(a, k, m, i, sc); });
    const Tile t = tile_of<B>(blockIdx.x, a.nvec, a.head * sizeof(typename Tr<Tag>::S));
    if (t.t0 >= a.nvec) return;
    u32x4 x0;
    u32x4 r = fan_fold<Tag, OP, V, KMAX>(a.in, k, t, a.head, a.trunc_from, x0, sc);
    if constexpr (bcast_copies_k1<Tag, V>()) r = (k == 1) ? bcast_k1<Tag, SC>(r, x0) : r;
    bcast_store(a, m, r, t);
}

template <typename Tag, int OP, unsigned V, int B, int KMAX>
__global__ __launch_bounds__(B) void bcast_kernel(BCArgs a) {
    bcast_tile<Tag, OP, V, B, KMAX>(a, NoScale());
}

template <typename Tag, int OP, unsigned V, int B, int KMAX>
__global__ __launch_bounds__(B) void bcast_scaled_kernel(BCArgs a, ScaleArg sc) {
    bcast_tile<Tag, OP, V, B, KMAX>(a, sc);
}

// The grid-stride form, for launches under mi_set_max_blocks and for the
// element loop (`scalar_only`: outputs at differing misalignments, or operands
// off the vector path).  The blocks stride over tiles of B vectors addressed
// as above; the fold is reduce_kernel's (a runtime loop over the inputs, the
// next input's load in flight while one is combined, every step with the x86
// NaN bits), so a lane still has all k loads back before its first store.
// Same bits as bcast_kernel.
template <typename Tag, int OP, unsigned V, int B>
__global__ __launch_bounds__(B) void bcast_stride_kernel(BCArgs a) {
    using S = typename Tr<Tag>::S;
    constexpr int N = 16 / sizeof(S);
    const int k = a.k, m = a.m;
    if (a.scalar_only) {
        for (uint64_t i = (uint64_t)blockIdx.x * B + threadIdx.x; i < a.count; i += (uint64_t)gridDim.x * B)
            bcast_elem<Tag, OP, V>(a, k, m, i);
        return;
    }
    head_tail(blockIdx.x, a.head, a.tail, a.head + a.nvec * N, [&](uint64_t i) { bcast_elem<Tag, OP, V>(a, k, m, i); });
    for (uint64_t tile = blockIdx.x; tile * B < a.nvec; tile += gridDim.x) {
        const Tile t = tile_of<B>(tile, a.nvec, a.head * sizeof(S));
        const auto load = [&](int i) {
            return __builtin_amdgcn_raw_buffer_load_b128(tile_rsrc(a.in[i], t.byte0, t.bytes), t.off, 0, kAuxNT);
        };
        const u32x4 x0 = load(0);
        u32x4 cur = x0, r = x0;
        if (k >= 2) cur = load(1);
        using C = typename Tr<Tag>::C;
        C acc[N];
        const Pack<S> p0 = __builtin_bit_cast(Pack<S>, x0);
        if constexpr (!packed_int<Tag>()) {
#pragma unroll
            for (int e = 0; e < N; e++) acc[e] = widen<Tag>(p0.e[e]);
        }
        for (int i = 1; i < k; i++) {
            u32x4 nxt = cur;
            if (i + 1 < k) nxt = load(i + 1);
            if constexpr (packed_int<Tag>()) {
                r = pk_op4<Tag, OP>(cur, r);
            } else {
                const Pack<S> pi = __builtin_bit_cast(Pack<S>, cur);
#pragma unroll
                for (int e = 0; e < N; e++) acc[e] = step<Tag, OP, V>(widen<Tag>(pi.e[e]), acc[e]);
            }
            cur = nxt;
        }
        if constexpr (!packed_int<Tag>()) {
            Pack<S> pr;
            const uint64_t e0 = a.head + (t.t0 + threadIdx.x) * N;
#pragma unroll
            for (int e = 0; e < N; e++)
                pr.e[e] = native_minmax<Tag, OP, V>(finish_fold<Tag, V>(acc[e], e0 + e, a.trunc_from), p0.e[e]);
            r = __builtin_bit_cast(u32x4, pr);
            if constexpr (bcast_copies_k1<Tag, V>()) r = (k == 1) ? x0 : r;
        }
        bcast_store(a, m, r, t);
    }
}

// bcast_stride_kernel under a multiplier, for a floating type.  A kernel text
// of its own: with one body shared through a callee, bcast_stride_kernel's
// registers moved (its arguments by reference: the fp16 min / max forms with
// fp32 accumulation 21 -> 23 and 30 -> 32 VGPRs; by value: most forms, either
// way).
template <typename Tag, int OP, unsigned V, int B>
__global__ __launch_bounds__(B) void bcast_scaled_stride_kernel(BCArgs a, ScaleArg sc) {
    using S = typename Tr<Tag>::S;
    constexpr int N = 16 / sizeof(S);
    const int k = a.k, m = a.m;
    if (a.scalar_only) {
        for (uint64_t i = (uint64_t)blockIdx.x * B + threadIdx.x; i < a.count; i += (uint64_t)gridDim.x * B)
            bcast_elem<Tag, OP, V>(a, k, m, i, sc);
        return;
    }
    head_tail(blockIdx.x, a.head, a.tail, a.head + a.nvec * N,
              [&](uint64_t i) { bcast_elem<Tag, OP, V>(a, k, m, i, sc); });
    for (uint64_t tile = blockIdx.x; tile * B < a.nvec; tile += gridDim.x) {
        const Tile t = tile_of<B>(tile, a.nvec, a.head * sizeof(S));
        const auto load = [&](int i) {
            return __builtin_amdgcn_raw_buffer_load_b128(tile_rsrc(a.in[i], t.byte0, t.bytes), t.off, 0, kAuxNT);
        };
        const u32x4 x0 = load(0);
        u32x4 cur = x0;
        if (k >= 2) cur = load(1);
        typename Tr<Tag>::C acc[N];
        const Pack<S> p0 = __builtin_bit_cast(Pack<S>, x0);
#pragma unroll
        for (int e = 0; e < N; e++) acc[e] = widen<Tag>(p0.e[e]);
        for (int i = 1; i < k; i++) {
            u32x4 nxt = cur;
            if (i + 1 < k) nxt = load(i + 1);
            const Pack<S> pi = __builtin_bit_cast(Pack<S>, cur);
#pragma unroll
            for (int e = 0; e < N; e++) acc[e] = step<Tag, OP, V>(widen<Tag>(pi.e[e]), acc[e]);
            cur = nxt;
        }
        Pack<S> pr;
        const uint64_t e0 = a.head + (t.t0 + threadIdx.x) * N;
#pragma unroll
        for (int e = 0; e < N; e++) pr.e[e] = finish_scaled<Tag, V, true>(acc[e], e0 + e, a.trunc_from, sc);
        u32x4 r = __builtin_bit_cast(u32x4, pr);
        if constexpr (bcast_copies_k1<Tag, V>()) r = (k == 1) ? bcast_k1<Tag, ScaleArg>(r, x0) : r;
        bcast_store(a, m, r, t);
    }
}

// ---------------------------------------------------------------------------
// element conversions fp32 <-> bf16 / fp16 (ccl_convert_*_arrays,
// src/comp/bf16/bf16.cpp:113-169, src/comp/fp16/fp16.cpp:55-61)
// ---------------------------------------------------------------------------
struct CArgs {
    const void* src;
    void* dst;
    uint64_t count;       // elements
    uint64_t head;        // elements before dst's first 16-byte boundary (vector path)
    uint64_t ngroups;     // groups of 8 elements on the vector path
    uint64_t trunc_from;  // V_TAIL_TRUNC: elements >= trunc_from truncate
    int scalar_only;
};

// X: the reference's NaN bits (the vector body runs X only on groups whose
// source holds an Inf or NaN, as fold_vec_x86 does)
template <typename ST, typename DT, unsigned V, bool X = true>
__device__ __forceinline__ typename Tr<DT>::S convert_elem(typename Tr<ST>::S s, uint64_t idx, uint64_t trunc_from) {
    float f = widen<ST>(s);
    if constexpr (X && std::is_same<ST, fp16_tag>::value)  // VCVTPH2PS quiets a signalling NaN
        f = nan_bits(__float_as_uint(f)) ? __uint_as_float(__float_as_uint(f) | 0x400000u) : f;
    if constexpr (std::is_same<DT, float>::value)
        return f;
    else
        return finish<DT, V, X>(f, idx, trunc_from);
}

template <typename ST, typename DT, unsigned V, bool X, int SV, int DV>
__device__ __forceinline__ void convert_group(const Pack<typename Tr<ST>::S> (&sp)[SV],
                                              Pack<typename Tr<DT>::S> (&dp)[DV], uint64_t e0, uint64_t trunc_from) {
    constexpr int SN = 16 / sizeof(typename Tr<ST>::S), DN = 16 / sizeof(typename Tr<DT>::S);
#pragma unroll
    for (int e = 0; e < 8; e++)
        dp[e / DN].e[e % DN] = convert_elem<ST, DT, V, X>(sp[e / SN].e[e % SN], e0 + e, trunc_from);
}

// The same 8 elements taken as two runs of 4: elements 0-3 have indices
// ea..ea+3, elements 4-7 eb..eb+3.
template <typename ST, typename DT, unsigned V, bool X, int SV, int DV>
__device__ __forceinline__ void convert_runs(const Pack<typename Tr<ST>::S> (&sp)[SV],
                                             Pack<typename Tr<DT>::S> (&dp)[DV], uint64_t ea, uint64_t eb,
                                             uint64_t trunc_from) {
    constexpr int SN = 16 / sizeof(typename Tr<ST>::S), DN = 16 / sizeof(typename Tr<DT>::S);
#pragma unroll
    for (int e = 0; e < 8; e++)
        dp[e / DN].e[e % DN] =
            convert_elem<ST, DT, V, X>(sp[e / SN].e[e % SN], e < 4 ? ea + e : eb + (e - 4), trunc_from);
}

// 8 elements per lane per group: fp32 side 2 x 16 B, 16-bit side 16 B.
// SC1: the vector body's stores go through one buffer descriptor per wave
// chunk with sc1 + nt (the line leaves L2 as it is written, as reduce2_kernel
// stores) instead of global nt stores.
template <typename ST, typename DT, unsigned V, int B = kBlock, bool SC1 = false>
__global__ __launch_bounds__(B) void convert_kernel(CArgs a) {
    using SS = typename Tr<ST>::S;
    using DS = typename Tr<DT>::S;
    const uint64_t stride = (uint64_t)gridDim.x * B;
    uint64_t i = (uint64_t)blockIdx.x * B + threadIdx.x;
    if (a.scalar_only) {
        for (; i < a.count; i += stride)
            static_cast<DS*>(a.dst)[i] = convert_elem<ST, DT, V>(static_cast<const SS*>(a.src)[i], i, a.trunc_from);
        return;
    }
    // vector body on dst's 16-byte grid from element `head` on; the source
    // vectors may be unaligned (element-aligned loads of 16 bytes)
    constexpr int SV = 8 * sizeof(SS) / 16;  // 16-byte source vectors per group
    constexpr int DV = 8 * sizeof(DS) / 16;
    const u32x4* src = reinterpret_cast<const u32x4*>(static_cast<const SS*>(a.src) + a.head);
    u32x4* dst = reinterpret_cast<u32x4*>(static_cast<DS*>(a.dst) + a.head);
    if constexpr (sizeof(SS) != sizeof(DS)) {
        // A lane's 8 elements as two runs of 4, so that every load and store
        // instruction covers one contiguous span across the wave (8 bytes per
        // lane on the 16-bit side, 16 on the fp32 side).  A wave whose 64
        // groups all lie in range (wave-uniform: `stride` and the block size
        // are multiples of 64) takes its 512 elements as the runs [4L, 4L+4)
        // and [256+4L, 256+4L+4) for lane L.  With eight contiguous elements
        // per lane (the loop below) every fp32-side instruction touched every
        // other 16 bytes: widening ran at ~4.1 TB/s, narrowing at ~6.2.
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        for (; (i | 63u) < a.ngroups; i += stride) {
            const uint64_t w = i & ~(uint64_t)63, lane = i & 63u;  // wave chunk: groups [w, w + 64)
            const uint64_t p0 = w * 2 + lane, p1 = p0 + 64;         // the two 4-element runs
            Pack<SS> sp[SV];
            if constexpr (sizeof(SS) < sizeof(DS)) {
                const u32x2* s2 = reinterpret_cast<const u32x2*>(src);
                const u32x2 x0 = __builtin_nontemporal_load(s2 + p0), x1 = __builtin_nontemporal_load(s2 + p1);
                sp[0] = __builtin_bit_cast(Pack<SS>, u32x4{x0.x, x0.y, x1.x, x1.y});
            } else {
                sp[0] = __builtin_bit_cast(Pack<SS>, vload<3>(src + p0));
                sp[1] = __builtin_bit_cast(Pack<SS>, vload<3>(src + p1));
            }
            const uint64_t ea = a.head + 4 * p0, eb = a.head + 4 * p1;  // element indices (V_TAIL_TRUNC)
            Pack<DS> dp[DV];
            convert_runs<ST, DT, V, false>(sp, dp, ea, eb, a.trunc_from);
            if constexpr (!std::is_same<ST, bf16_tag>::value) {  // bf16 -> fp32 is a shift: bits exact as is
                uint32_t bits = 0;
#pragma unroll
                for (int v = 0; v < SV; v++) bits |= inf_nan_bits<ST>(__builtin_bit_cast(u32x4, sp[v]));
                if (__builtin_expect(inf_nan_hit<ST>(bits), 0)) convert_runs<ST, DT, V, true>(sp, dp, ea, eb, a.trunc_from);
            }
            if constexpr (SC1) {
                // the wave chunk's destination: 128 consecutive stores of 16 B
                // (widening) or 8 B (narrowing), the whole chunk in range
                constexpr uint32_t SB = sizeof(SS) < sizeof(DS) ? 16u : 8u;
                const __amdgpu_buffer_rsrc_t o = tile_rsrc(dst, w * 2 * SB, 128u * SB);
                const uint32_t o0 = (uint32_t)lane * SB, o1 = o0 + 64u * SB;
                if constexpr (sizeof(SS) < sizeof(DS)) {
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, dp[0]), o, o0, 0, kAuxSC1NT);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, dp[1]), o, o1, 0, kAuxSC1NT);
                } else {
                    const u32x4 d = __builtin_bit_cast(u32x4, dp[0]);
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2{d.x, d.y}, o, o0, 0, kAuxSC1NT);
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2{d.z, d.w}, o, o1, 0, kAuxSC1NT);
                }
            } else if constexpr (sizeof(SS) < sizeof(DS)) {
                vstore<3>(dst + p0, __builtin_bit_cast(u32x4, dp[0]));
                vstore<3>(dst + p1, __builtin_bit_cast(u32x4, dp[1]));
            } else {
                const u32x4 d = __builtin_bit_cast(u32x4, dp[0]);
                u32x2* d2 = reinterpret_cast<u32x2*>(dst);
                __builtin_nontemporal_store(u32x2{d.x, d.y}, d2 + p0);
                __builtin_nontemporal_store(u32x2{d.z, d.w}, d2 + p1);
            }
        }
    }
    for (; i < a.ngroups; i += stride) {
        Pack<SS> sp[SV];
#pragma unroll
        for (int v = 0; v < SV; v++) sp[v] = __builtin_bit_cast(Pack<SS>, vload<3>(src + i * SV + v));
        Pack<DS> dp[DV];
        convert_group<ST, DT, V, false>(sp, dp, a.head + i * 8, a.trunc_from);
        if constexpr (!std::is_same<ST, bf16_tag>::value) {  // bf16 -> fp32 is a shift: bits exact as is
            uint32_t bits = 0;
#pragma unroll
            for (int v = 0; v < SV; v++) bits |= inf_nan_bits<ST>(__builtin_bit_cast(u32x4, sp[v]));
            if (__builtin_expect(inf_nan_hit<ST>(bits), 0)) convert_group<ST, DT, V, true>(sp, dp, a.head + i * 8, a.trunc_from);
        }
#pragma unroll
        for (int v = 0; v < DV; v++) vstore<3>(dst + i * DV + v, __builtin_bit_cast(u32x4, dp[v]));
    }
    // head (< 16 bytes of dst) and tail (< 8 elements) by the first lanes of block 0
    if (blockIdx.x == 0) {
        if (threadIdx.x < a.head)
            static_cast<DS*>(a.dst)[threadIdx.x] =
                convert_elem<ST, DT, V>(static_cast<const SS*>(a.src)[threadIdx.x], threadIdx.x, a.trunc_from);
        if (threadIdx.x < a.count - a.head - a.ngroups * 8) {
            const uint64_t j = a.head + a.ngroups * 8 + threadIdx.x;
            static_cast<DS*>(a.dst)[j] = convert_elem<ST, DT, V>(static_cast<const SS*>(a.src)[j], j, a.trunc_from);
        }
    }
}

// ---------------------------------------------------------------------------
// mi_reduce_bcast_mixed: fold K inputs of one precision in fp32 and write the
// result in the other, to M outputs, in one pass.  Widening (bf16 / fp16 in,
// fp32 out, optionally on top of an fp32 accumulator `acc`) is the fp32
// scratch fold of the reference's keep-precision batch reduce
// (src/comp/comp.cpp:214-234) without the rounding that ends it; narrowing
// (fp32 in, bf16 / fp16 out) is the fp32 fan-in followed by the array
// conversion.  The pieces are the ones above: convert_elem (the fp16
// signalling-NaN quieting included), step<float, OP_SUM> with the accumulator
// as first source, finish<DT, V> with the element-indexed trunc_from, per-tile
// buffer descriptors, the wave-uniform store loop.
//   Geometry: launch_convert's plan (plan_mixed_grid, vec_grid.hpp).  The body
// is groups of 8 elements from the outputs' first 16-byte boundary on.  A
// one-wave block owns a tile of 64 * RUNS runs of 4 elements; lane L takes
// run r * 64 + L for r < RUNS, so every load and store instruction covers one
// contiguous span across the wave (8 bytes per lane on the 16-bit side, 16 on
// the fp32 side), as convert_kernel's wave chunks do.  RUNS = 2 is that
// kernel's layout (512 elements per wave, 8 per lane) and the one built;
// RUNS = 1 would be 4 elements per lane (256 per wave).  A tile's valid elements
// are a multiple of 8, so a run is wholly inside its descriptors or wholly
// outside (loads zeros, stores dropped).
//   Every lane has all k loads (and acc's) issued before its first combine and
// back before its first store; `acc` may be exactly one output (both fp32, so
// it sits on the outputs' grid and a lane loads exactly the bytes it later
// stores): mi_reduce_bcast's in-place argument.
//   mi_reduce_bcast_mixed_scaled runs the same bodies with a multiplier (the SC
// parameter, as the scaled fan-out): kernels of their own, MXArgs unchanged.
// The inputs are folded alone, their sum is scaled once and acc is added last
// (mx_scaled, mx_scaled_onto); the multiply sits after the last combine of the
// inputs and acc's load is issued with theirs, so the order of loads and
// stores, and with it the in-place argument, is unchanged.
// ---------------------------------------------------------------------------
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct MXArgs {
    const void* in[kMaxInputs];
    void* out[kMaxInputs];  // m destinations, all at one misalignment on the vector path
    const void* acc;        // widening: the fp32 accumulator's start, or null
    uint64_t ngroups;       // groups of 8 elements in the body
    uint64_t head;          // leading scalar elements (the outputs' misalignment)
    uint64_t tail;          // trailing scalar elements (< 8)
    uint64_t count;         // total elements
    uint64_t trunc_from;    // V_TAIL_TRUNC threshold (element index)
    int k;                  // inputs (acc not counted)
    int m;                  // outputs
    int scalar_only;        // element loop only
    int store_sc1;          // stores sc1 + nt instead of nt (mi_set_bcast_store)
};

constexpr int kMixedBlock = 64;  // one wave
template <int RUNS>
constexpr uint32_t mixed_tile_elems() {
    return 4u * kMixedBlock * RUNS;
}

// One run of 4 elements as loaded: 8 bytes of a 16-bit type, 16 of fp32.
template <typename T>
struct MxRun {
    using type = typename std::conditional<sizeof(typename Tr<T>::S) == 2, u32x2, u32x4>::type;
};

template <typename T>
__device__ __forceinline__ typename MxRun<T>::type mx_load(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
    if constexpr (sizeof(typename Tr<T>::S) == 2)
        return __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, kAuxNT);
    else
        return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, kAuxNT);
}

// The run's 4 values in fp32: what mi_convert(T -> fp32) writes (X: with the
// fp16 signalling-NaN quieting), or the words themselves.
template <typename T, bool X>
__device__ __forceinline__ void mx_widen(const typename MxRun<T>::type& x, float (&f)[4]) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
        if constexpr (sizeof(typename Tr<T>::S) == 2)
            f[e] = convert_elem<T, float, 0u, X>((uint16_t)(x[e >> 1] >> (16 * (e & 1))), 0, 0);
        else
            f[e] = __uint_as_float(x[e]);
    }
}

// inf_nan_bits of one run (all-ones exponent: Inf or NaN)
template <typename T>
__device__ __forceinline__ bool mx_inf_nan(const typename MxRun<T>::type& x) {
    if constexpr (sizeof(typename Tr<T>::S) == 2)
        return inf_nan_hit<T>(inf_nan_word<T>(x.x) | inf_nan_word<T>(x.y));
    else
        return inf_nan_hit<float>(inf_nan_word<float>(x.x) | inf_nan_word<float>(x.y) | inf_nan_word<float>(x.z) |
                                  inf_nan_word<float>(x.w));
}

// mi_reduce_bcast_mixed_scaled: the fp32 sum of the inputs alone times the
// multiplier, one IEEE multiply rounded to fp32 (finish_scaled's rule: a NaN
// sum is kept as it is and never reaches the multiplier, whose NaN choice is
// the hardware's; X = false leaves the select out, the caller refolds every
// row its Inf/NaN screen hits).
template <bool X>
__device__ __forceinline__ float mx_scaled(float sum, float s) {
#pragma clang fp contract(off)
    const float p = sum * s;
    if constexpr (X) return (sum != sum) ? sum : p;
    else return p;
}
// That product added to the accumulator: acc + (float)(sum * s), one x86-rule
// add with acc as first source (mi_reduce_multi({acc, P}, fp32, sum)).  The
// product is rounded before the add: with contraction on (the build's default)
// the compiler makes the pair one v_fmac_f32, which rounds once and differs in
// the last bit (in 2630 of 12259 finite elements of the bf16 test inputs at
// scale 1/3), so both operations stand in this one body with contraction off.
template <bool X>
__device__ __forceinline__ float mx_scaled_onto(float sum, float s, float acc) {
#pragma clang fp contract(off)
    const float p = mx_scaled<X>(sum, s);
    const float r = acc + p;
    if constexpr (X) return x86_nan_first(r, acc, p);
    else return r;
}

// The fold of one run of 4 elements across the loaded inputs (and acc), and
// its final conversion.  e0: the run's first element index.  Under a
// multiplier (SC = ScaleArg) the inputs are folded alone, the sum is scaled
// and acc is added last (mx_scaled_onto): acc + s * sum, not s * (acc + sum).
//   The X = false form under a multiplier is still exact on every run the
// callers' screen (an all-ones exponent in an input or in acc as loaded) does
// not hit: s is finite and not zero, so the product of a finite sum is finite
// or, on overflow, an Inf; a sum of finite inputs is finite or an Inf of one
// sign (no Inf - Inf without an Inf input); and acc is finite there, so the
// last add has at most one Inf operand.  No NaN can arise, and without a NaN
// the fix-ups change nothing.
template <typename ST, typename DT, unsigned V, bool X, int KMAX, typename SC = NoScale>
__device__ __forceinline__ typename MxRun<DT>::type mx_fold(const typename MxRun<ST>::type (&x)[KMAX], int k,
                                                            bool has_acc, u32x4 xa, uint64_t e0,
                                                            uint64_t trunc_from, const SC& sc = SC()) {
    constexpr bool SCALED = !std::is_same<SC, NoScale>::value;
    const bool from_acc = SCALED ? false : has_acc;  // the unscaled fold starts from acc
    float s[4], c[4];
    if (from_acc) {
#pragma unroll
        for (int e = 0; e < 4; e++) s[e] = __uint_as_float(xa[e]);
    }
#pragma unroll
    for (int i = 0; i < KMAX; i++) {
        if (i < k) {
            mx_widen<ST, X>(x[i], c);
            if (i == 0 && !from_acc) {
#pragma unroll
                for (int e = 0; e < 4; e++) s[e] = c[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) s[e] = step<float, OP_SUM, 0u, X>(c[e], s[e]);
            }
        }
    }
    if constexpr (SCALED) {
        const float f = sc.template as<float>();
        if (has_acc) {
#pragma unroll
            for (int e = 0; e < 4; e++) s[e] = mx_scaled_onto<X>(s[e], f, __uint_as_float(xa[e]));
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) s[e] = mx_scaled<X>(s[e], f);
        }
    }
    typename MxRun<DT>::type r;
    if constexpr (std::is_same<DT, float>::value) {
#pragma unroll
        for (int e = 0; e < 4; e++) r[e] = __float_as_uint(s[e]);
    } else {
        uint32_t h[4];
#pragma unroll
        for (int e = 0; e < 4; e++) h[e] = finish<DT, V, X>(s[e], e0 + e, trunc_from);
        r.x = h[0] | (h[1] << 16);
        r.y = h[2] | (h[3] << 16);
    }
    return r;
}

// Element `idx` on the scalar path (head, tail, element loop), stored to every
// output.
template <typename ST, typename DT, unsigned V, typename SC = NoScale>
__device__ __forceinline__ void mixed_elem(const MXArgs& a, uint64_t idx, const SC& sc = SC()) {
    using SS = typename Tr<ST>::S;
    using DS = typename Tr<DT>::S;
    constexpr bool SCALED = !std::is_same<SC, NoScale>::value;
    const auto c = [&](int j) -> float {
        if constexpr (sizeof(SS) == 2)
            return convert_elem<ST, float, 0u, true>(static_cast<const SS*>(a.in[j])[idx], 0, 0);
        else
            return static_cast<const float*>(a.in[j])[idx];
    };
    float s;
    int j = 0;
    if (!SCALED && a.acc) s = static_cast<const float*>(a.acc)[idx];
    else s = c(j++);
    for (; j < a.k; j++) s = step<float, OP_SUM, 0u, true>(c(j), s);
    if constexpr (SCALED) {  // the inputs' sum alone, scaled, then onto acc (mx_fold)
        const float f = sc.template as<float>();
        s = a.acc ? mx_scaled_onto<true>(s, f, static_cast<const float*>(a.acc)[idx]) : mx_scaled<true>(s, f);
    }
    DS r;
    if constexpr (std::is_same<DT, float>::value) r = s;
    else r = finish<DT, V, true>(s, idx, a.trunc_from);
    for (int o = 0; o < a.m; o++) static_cast<DS*>(a.out[o])[idx] = r;
}

// A tile's geometry: its first element and its valid elements (a multiple of
// 8; 0 for a tile past the end).
template <int RUNS>
__device__ __forceinline__ void mx_tile_of(const MXArgs& a, uint64_t tile, uint64_t& first, uint32_t& ne) {
    constexpr uint32_t TE = mixed_tile_elems<RUNS>();
    const uint64_t t0 = tile * TE, nbody = a.ngroups * 8;
    const uint64_t left = nbody > t0 ? nbody - t0 : 0;
    ne = (uint32_t)(left < (uint64_t)TE ? left : (uint64_t)TE);
    first = a.head + t0;
}

// This lane's byte offset of run r in a tile of elements of `es` bytes.
__device__ __forceinline__ uint32_t mx_off(int r, uint32_t es) {
    return (uint32_t)(r * kMixedBlock + threadIdx.x) * 4u * es;
}

// The m stores of a lane's results: bcast_store's wave-uniform loop over the
// output pointers, one descriptor per output.
template <typename DT, int RUNS>
__device__ __forceinline__ void mx_store(const MXArgs& a, int m, const typename MxRun<DT>::type (&res)[RUNS],
                                         uint64_t first, uint32_t ne) {
    using DS = typename Tr<DT>::S;
    const auto store = [&](auto aux) {
#pragma nounroll
        for (int o = 0; o < m; o++) {
            const __amdgpu_buffer_rsrc_t rs = tile_rsrc(a.out[o], first * sizeof(DS), ne * (uint32_t)sizeof(DS));
#pragma unroll
            for (int r = 0; r < RUNS; r++) {
                if constexpr (sizeof(DS) == 2)
                    __builtin_amdgcn_raw_buffer_store_b64(res[r], rs, mx_off(r, 2), 0, decltype(aux)::value);
                else
                    __builtin_amdgcn_raw_buffer_store_b128(res[r], rs, mx_off(r, 4), 0, decltype(aux)::value);
            }
        }
    };
    if (a.store_sc1) store(std::integral_constant<int, kAuxSC1NT>());
    else store(std::integral_constant<int, kAuxNT>());
}

// One tile per one-wave block; block 0 also does the scalar head and tail.
// All k loads (and acc's) are issued before the first combine (uniform
// branches on k only); the fast fold without the NaN fix-ups, then the screen
// on the inputs as loaded and the x86 refold of the runs that hold an Inf or
// NaN.  mx_fold is force-inlined and x[] is indexed by constants only: with
// the fold's runtime-k branches in a callee the compiler may keep x[] as an
// aggregate in scratch (fan_fold's note; tests/test_kernel_resources.py).
template <typename ST, typename DT, unsigned V, int RUNS, int KMAX, typename SC>
__device__ __forceinline__ void mixed_tile(const MXArgs& a, const SC& sc) {
    using SS = typename Tr<ST>::S;
    constexpr bool WIDE = std::is_same<DT, float>::value;
    head_tail(blockIdx.x, a.head, a.tail, a.head + a.ngroups * 8, [&](uint64_t i) { mixed_elem<ST, DT, V>(a, i, sc); });
    uint64_t first;
    uint32_t ne;
    mx_tile_of<RUNS>(a, blockIdx.x, first, ne);
    if (ne == 0) return;
    const int k = a.k;
    const bool has_acc = WIDE && a.acc != nullptr;

    const void* in[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; i++) {
        in[i] = a.in[i];
        asm volatile("" ::"s"(in[i]));
    }
    typename MxRun<ST>::type x[RUNS][KMAX] = {};  // defined in every slot: the fold's k is opaque (below)
#pragma unroll
    for (int i = 0; i < KMAX; i++) {
        if (i < k) {
            const __amdgpu_buffer_rsrc_t rs = tile_rsrc(in[i], first * sizeof(SS), ne * (uint32_t)sizeof(SS));
#pragma unroll
            for (int r = 0; r < RUNS; r++) x[r][i] = mx_load<ST>(rs, mx_off(r, sizeof(SS)));
        }
    }
    u32x4 xa[RUNS];
#pragma unroll
    for (int r = 0; r < RUNS; r++) xa[r] = u32x4{0u, 0u, 0u, 0u};
    if constexpr (WIDE) {
        if (has_acc) {
            const __amdgpu_buffer_rsrc_t rs = tile_rsrc(a.acc, first * 4, ne * 4u);
#pragma unroll
            for (int r = 0; r < RUNS; r++) xa[r] = __builtin_amdgcn_raw_buffer_load_b128(rs, mx_off(r, 4), 0, kAuxNT);
        }
    }
    // The fold's branches test a copy of k the compiler cannot relate to the
    // loads' k, and x[] is defined in every slot: the branches of the loads
    // cannot be threaded through those of the fold (one path per k, all of x[]
    // merged where the paths meet), so every load is issued before the first
    // combine whatever the compiler makes of the fold.  Written against the
    // one-run layout's registers (238 to 492 VGPRs, each load next to its use),
    // which it did not cure; with two runs it costs at most one VGPR.
    int kf = k;
    asm volatile("" : "+s"(kf));

    typename MxRun<DT>::type res[RUNS];
#pragma unroll
    for (int r = 0; r < RUNS; r++) {
        const uint64_t e0 = first + (uint64_t)(r * kMixedBlock + threadIdx.x) * 4u;
        res[r] = mx_fold<ST, DT, V, false, KMAX>(x[r], kf, has_acc, xa[r], e0, a.trunc_from, sc);
        bool hit = WIDE && mx_inf_nan<float>(xa[r]);
#pragma unroll
        for (int i = 0; i < KMAX; i++)
            if (i < kf) hit |= mx_inf_nan<ST>(x[r][i]);
        if (__builtin_expect(hit, 0))
            res[r] = mx_fold<ST, DT, V, true, KMAX>(x[r], kf, has_acc, xa[r], e0, a.trunc_from, sc);
    }
    mx_store<DT, RUNS>(a, a.m, res, first, ne);
}

template <typename ST, typename DT, unsigned V, int RUNS, int KMAX>
__global__ __launch_bounds__(kMixedBlock) void mixed_kernel(MXArgs a) {
    mixed_tile<ST, DT, V, RUNS, KMAX>(a, NoScale());
}

// The same tile under a multiplier (mi_reduce_bcast_mixed_scaled): a kernel of
// its own, MXArgs as the unscaled call passes it.
template <typename ST, typename DT, unsigned V, int RUNS, int KMAX>
__global__ __launch_bounds__(kMixedBlock) void mixed_scaled_kernel(MXArgs a, ScaleArg sc) {
    mixed_tile<ST, DT, V, RUNS, KMAX>(a, sc);
}

// The grid-stride form (launches under mi_set_max_blocks) and the element
// loop (`scalar_only`).  The blocks stride over the same tiles, addressed as
// above; the fold is a runtime loop over the inputs, acc's load first, the
// next input's load in flight while one is combined, every step with the x86
// NaN bits (bcast_stride_kernel's shape), so a lane still has every load back
// before its first store.  Same bits as mixed_kernel.
template <typename ST, typename DT, unsigned V, int RUNS, typename SC>
__device__ __forceinline__ void mixed_stride(const MXArgs& a, const SC& sc) {
    using SS = typename Tr<ST>::S;
    constexpr bool WIDE = std::is_same<DT, float>::value;
    constexpr bool SCALED = !std::is_same<SC, NoScale>::value;
    if (a.scalar_only) {
        for (uint64_t i = (uint64_t)blockIdx.x * kMixedBlock + threadIdx.x; i < a.count;
             i += (uint64_t)gridDim.x * kMixedBlock)
            mixed_elem<ST, DT, V>(a, i, sc);
        return;
    }
    head_tail(blockIdx.x, a.head, a.tail, a.head + a.ngroups * 8, [&](uint64_t i) { mixed_elem<ST, DT, V>(a, i, sc); });
    const int k = a.k;
    const bool has_acc = WIDE && a.acc != nullptr;
    for (uint64_t tile = blockIdx.x; tile * mixed_tile_elems<RUNS>() < a.ngroups * 8; tile += gridDim.x) {
        uint64_t first;
        uint32_t ne;
        mx_tile_of<RUNS>(a, tile, first, ne);
        typename MxRun<ST>::type cur[RUNS], nxt[RUNS];
        const auto load = [&](int i, typename MxRun<ST>::type (&x)[RUNS]) {
            const __amdgpu_buffer_rsrc_t rs = tile_rsrc(a.in[i], first * sizeof(SS), ne * (uint32_t)sizeof(SS));
#pragma unroll
            for (int r = 0; r < RUNS; r++) x[r] = mx_load<ST>(rs, mx_off(r, sizeof(SS)));
        };
        // acc's values: the fold's start, or under a multiplier its last operand (mx_fold)
        float s[RUNS][4], c[4], sa[SCALED ? RUNS : 1][4];
        if constexpr (WIDE) {
            if (has_acc) {
                const __amdgpu_buffer_rsrc_t rs = tile_rsrc(a.acc, first * 4, ne * 4u);
#pragma unroll
                for (int r = 0; r < RUNS; r++) {
                    const u32x4 xa = __builtin_amdgcn_raw_buffer_load_b128(rs, mx_off(r, 4), 0, kAuxNT);
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        if constexpr (SCALED) sa[r][e] = __uint_as_float(xa[e]);
                        else s[r][e] = __uint_as_float(xa[e]);
                    }
                }
            }
        }
        const bool from_acc = SCALED ? false : has_acc;
        load(0, cur);
        for (int i = 0; i < k; i++) {
#pragma unroll
            for (int r = 0; r < RUNS; r++) nxt[r] = cur[r];
            if (i + 1 < k) load(i + 1, nxt);
#pragma unroll
            for (int r = 0; r < RUNS; r++) {
                mx_widen<ST, true>(cur[r], c);
#pragma unroll
                for (int e = 0; e < 4; e++) s[r][e] = (i == 0 && !from_acc) ? c[e] : step<float, OP_SUM, 0u, true>(c[e], s[r][e]);
                cur[r] = nxt[r];
            }
        }
        if constexpr (SCALED) {
            const float f = sc.template as<float>();
#pragma unroll
            for (int r = 0; r < RUNS; r++) {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    s[r][e] = has_acc ? mx_scaled_onto<true>(s[r][e], f, sa[r][e]) : mx_scaled<true>(s[r][e], f);
            }
        }
        typename MxRun<DT>::type res[RUNS];
#pragma unroll
        for (int r = 0; r < RUNS; r++) {
            if constexpr (WIDE) {
#pragma unroll
                for (int e = 0; e < 4; e++) res[r][e] = __float_as_uint(s[r][e]);
            } else {
                const uint64_t e0 = first + (uint64_t)(r * kMixedBlock + threadIdx.x) * 4u;
                uint32_t h[4];
#pragma unroll
                for (int e = 0; e < 4; e++) h[e] = finish<DT, V, true>(s[r][e], e0 + e, a.trunc_from);
                res[r].x = h[0] | (h[1] << 16);
                res[r].y = h[2] | (h[3] << 16);
            }
        }
        mx_store<DT, RUNS>(a, a.m, res, first, ne);
    }
}

template <typename ST, typename DT, unsigned V, int RUNS>
__global__ __launch_bounds__(kMixedBlock) void mixed_stride_kernel(MXArgs a) {
    mixed_stride<ST, DT, V, RUNS>(a, NoScale());
}

template <typename ST, typename DT, unsigned V, int RUNS>
__global__ __launch_bounds__(kMixedBlock) void mixed_scaled_stride_kernel(MXArgs a, ScaleArg sc) {
    mixed_stride<ST, DT, V, RUNS>(a, sc);
}

// Byte copy with optional non-temporal stores (ccl_comp_copy), on the
// destination's 16-byte grid: block 0 copies the < 16-byte head and tail byte
// by byte, the body moves 16-byte vectors.  The source may sit at any byte
// offset from that grid (unaligned 16-byte loads, as in the reduce kernels).
template <int MEM>
__global__ __launch_bounds__(kBlock) void copy_kernel(const char* __restrict__ src8, char* __restrict__ dst8,
                                                      uint32_t head, uint64_t nvec, uint32_t tail) {
    head_tail(blockIdx.x, head, tail, head + nvec * 16, [&](uint64_t o) { dst8[o] = src8[o]; });
    const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(src8 + head);
    u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(dst8 + head);
    constexpr int U = 4;
    const uint64_t tile = (uint64_t)kBlock * U;
    for (uint64_t base = (uint64_t)blockIdx.x * tile + threadIdx.x; base < nvec;
         base += (uint64_t)gridDim.x * tile) {
        u32x4 r[U];
#pragma unroll
        for (int j = 0; j < U; j++)
            if (base + (uint64_t)j * kBlock < nvec) r[j] = vload<MEM & 1>(src + base + (uint64_t)j * kBlock);
#pragma unroll
        for (int j = 0; j < U; j++)
            if (base + (uint64_t)j * kBlock < nvec) vstore<MEM & 2>(dst + base + (uint64_t)j * kBlock, r[j]);
    }
}

// The same copy as one tile per block, one 16-byte vector per lane, no loop
// (reduce2_kernel's shape); the default grid.  One-wave (64-lane) tiles with
// no residency cap: 1 GiB in 0.320 ms against 0.336 at round 2's 512 lanes
// (-5 %; the 1-read/1-write stream keeps only 1 KiB per wave in flight, so
// unlike the reduce kernels it wants every wave slot; tools/occupancy_sweep.hip
// copyu / copyconv, profiles/round3_occupancy/).  Round 2's sweep
// (tools/copy_sweep.hip) had 512 lanes at 6.44 TB/s against 5.78 for
// copy_kernel<2>, which stays for a capped grid (mi_set_max_blocks).
// MEM bit 0: nt loads; bit 1: nt stores; bit 2: stores through a per-tile
// buffer descriptor with sc1 + nt (each line leaves L2 as it is written, as
// reduce2_kernel stores), for streaming copies far larger than the caches.
constexpr int kCopyBlock = 64;
template <int MEM, int B = kCopyBlock>
__global__ __launch_bounds__(B) void copy_lean_kernel(const char* __restrict__ src8, char* __restrict__ dst8,
                                                      uint32_t head, uint64_t nvec, uint32_t tail) {
    head_tail(blockIdx.x, head, tail, head + nvec * 16, [&](uint64_t o) { dst8[o] = src8[o]; });
    const uint64_t v = (uint64_t)blockIdx.x * B + threadIdx.x;
    if (MEM & 4) {
        // global nt loads: buffer loads here ran 0.4-0.7 % slower in every
        // one of 20 fresh placements (tools/ab_c2.py --config copy,
        // profiles/round6_run8/), unlike the 2-input reduce's
        const Tile t = tile_of<B>(blockIdx.x, nvec, head);
        if (v < nvec)
            __builtin_amdgcn_raw_buffer_store_b128(vload<MEM & 1>(reinterpret_cast<const u32x4*>(src8 + head) + v),
                                                   tile_rsrc(dst8, t.byte0, t.bytes), t.off, 0, kAuxSC1NT);
    } else if (v < nvec) {
        vstore<MEM & 2>(reinterpret_cast<u32x4*>(dst8 + head) + v,
                        vload<MEM & 1>(reinterpret_cast<const u32x4*>(src8 + head) + v));
    }
}

}  // namespace mi
