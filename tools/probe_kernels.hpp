// probe_kernels.hpp — kernels that only the measurement tools launch
// (reduce_sweep, fan_sweep, burst_sweep, lds_stage_sweep): earlier shapes of
// the product's kernels, kept to measure against.  No library entry point
// reaches them, and nothing here is compiled into libmi_reduce.so.
#pragma once

#include "../oneccl_amd/csrc/reduce_kernels.hpp"

namespace mi {

// ---------------------------------------------------------------------------
// Lean K-input fan-in (compile-time K): one tile of B*U vectors per block,
// every input's loads issued before the first combine, left fold in the
// reference's order (acc = in[0]; acc = op(in[j], acc)).  Requires a common
// alignment; head/tail by block 0.
// ---------------------------------------------------------------------------
struct RKArgs {
    const void* in[kMaxInputs];
    void* out;
    uint64_t nvec;
    uint32_t head, tail;
    uint64_t trunc_from;
};

template <typename Tag, int OP, unsigned V, int K>
__device__ __forceinline__ void reducek_elem(const RKArgs& a, uint64_t idx) {
    static_cast<typename Tr<Tag>::S*>(a.out)[idx] = fold_elem<Tag, OP, V>(a.in, K, idx, a.trunc_from);
}

template <typename Tag, int OP, unsigned V, int K, int U, int B>
__global__ __launch_bounds__(B) void reducek_kernel(RKArgs a) {
    using S = typename Tr<Tag>::S;
    constexpr int N = 16 / sizeof(S);
    head_tail(blockIdx.x, a.head, a.tail, a.head + a.nvec * N, [&](uint64_t i) { reducek_elem<Tag, OP, V, K>(a, i); });
    const size_t hb = (size_t)a.head * sizeof(S);
    const uint64_t v0 = (uint64_t)blockIdx.x * (B * U) + threadIdx.x;
    const bool full = v0 + (uint64_t)(U - 1) * B < a.nvec;
    u32x4 x[K][U];
#pragma unroll
    for (int i = 0; i < K; i++) {
        const u32x4* p = reinterpret_cast<const u32x4*>(static_cast<const char*>(a.in[i]) + hb);
#pragma unroll
        for (int j = 0; j < U; j++)
            if (full || v0 + (uint64_t)j * B < a.nvec) x[i][j] = vload<3>(p + v0 + (uint64_t)j * B);
    }
    u32x4* po = reinterpret_cast<u32x4*>(static_cast<char*>(a.out) + hb);
#pragma unroll
    for (int j = 0; j < U; j++) {
        const uint64_t v = v0 + (uint64_t)j * B;
        if (full || v < a.nvec) {
            u32x4 xs[K];
#pragma unroll
            for (int i = 0; i < K; i++) xs[i] = x[i][j];
            vstore<3>(po + v, fold_row<Tag, OP, V, K>(xs, K, a.head + v * N, a.trunc_from, [&](u32x4 (&r)[K]) {
#pragma unroll
                          for (int i = 0; i < K; i++)
                              r[i] = vload<3>(reinterpret_cast<const u32x4*>(static_cast<const char*>(a.in[i]) + hb) + v);
                      }));
        }
    }
}

// The 2-input fold through one buffer descriptor per tile of B vectors, with
// nt stores (R2Args: acc, in -> out): reduce2_kernel before its sc1 stores.
template <typename Tag, int OP, unsigned V, int B>
__global__ __launch_bounds__(B) void reduce2b_kernel(R2Args a) {
    using S = typename Tr<Tag>::S;
    constexpr int N = 16 / sizeof(S);
    head_tail(blockIdx.x, a.head, a.tail, a.head + a.nvec * N, [&](uint64_t i) { reduce2_elem<Tag, OP, V>(a, i); });
    const Tile t = tile_of<B>(blockIdx.x, a.nvec, (uint64_t)a.head * sizeof(S));
    if (t.t0 >= a.nvec) return;
    const auto load = [&](const void* p) {
        return __builtin_amdgcn_raw_buffer_load_b128(tile_rsrc(p, t.byte0, t.bytes), t.off, 0, kAuxNT);
    };
    const u32x4 xs[2] = {load(a.acc), load(a.in)};
    __builtin_amdgcn_raw_buffer_store_b128(
        fold_row<Tag, OP, V, 2>(xs, 2, a.head + (t.t0 + threadIdx.x) * N, a.trunc_from,
                                [&](u32x4 (&r)[2]) {
                                    r[0] = load(a.acc);
                                    r[1] = load(a.in);
                                }),
        tile_rsrc(a.out, t.byte0, t.bytes), t.off, 0, kAuxNT);
}

}  // namespace mi
