"""Guarded placement of operands: proof that a call writes nothing outside
its output.

oneCCL hands the library sub-buffers of larger buckets (reduce-scatter
chunks, ring chunks, tmp_buf slices), so the bytes on either side of an
output are another rank's live data.  An `Arena` is one allocation (device,
pinned host or pageable host memory) filled with seeded random bytes in
1..254.  Operands are carved out of it at chosen misalignments with at least
`GUARD` bytes of arena on each side; after the call, `check()` compares the
whole arena with the snapshot taken before it and requires every byte
outside the declared outputs to be unchanged.  One comparison covers both
guards of every operand, every gap, and every input.

A random byte canary alone misses two kinds of spill:
  * a lane past the end that loads zeros and stores op(0, 0) = 0 would be
    invisible over zero padding (hence no zero byte anywhere in an arena);
  * in place, a spilling lane does load-op-store on its neighbour, which for
    min/max is often the identity.
`guard_elems` therefore draws the guards beside a reduce's operands as
elements of the dtype such that, at every position, the output-side guard
differs from the fold of the operands' guards, from the fold of zeros and
from zero.

Who guards what (kernels of reduce_kernels.hpp, host-writing paths of
mi_reduce.hip and host_reduce*.cpp; knob = how the test routes to it):

  reduce2_kernel           test_gpu_bounds::test_lean_two_input_kernel (mi_reduce, mi_reduce_out; default knobs)
  reduce2_batch_kernel     test_gpu_bounds::test_batch_kernel (mi_reduce_batch, 3 / 64 / 65 descriptors);
                           test_gpu_batch (pool compared byte for byte)
  fan_kernel<.., 8 / 16>   test_gpu_bounds::test_fan_kernel, test_fan_kernel_fp32_accumulate
                           (mi_reduce_multi, k = 1, 3, 8 | 9, 16)
  reduce_kernel, tiles     test_gpu_bounds::test_general_kernel_under_grid_cap (mi_set_max_blocks(1), (3))
  reduce_kernel, elements  test_gpu_bounds::test_element_loop (mi_set_unaligned_vectors(0), differing
                           misalignments), test_element_loop_byte_misaligned_fp32 (odd byte offsets)
  unaligned vector loads   test_gpu_bounds::test_unaligned_vector_loads (mi_set_unaligned_vectors(1), k = 2, 5)
  convert_kernel           test_gpu_bounds::test_convert_kernel (default, mi_set_max_blocks(1), element loop)
  convert_kernel, SC1      test_gpu_convert::test_streaming_narrowing_conversions (sources of 64 MiB and more)
  copy_lean_kernel<1 / 3>  test_gpu_bounds::test_copy_kernels (mi_copy, ccl_comp_copy; nontemporal 0 / 1)
  copy_kernel<1 / 3>       test_gpu_bounds::test_copy_kernels (mi_set_max_blocks(3))
  copy_lean_kernel<5>      test_gpu_shim::test_comp_copy_streaming_sizes (copies of 64 MiB and more)
  bcast_kernel<.., 8 / 16> test_gpu_bcast_bounds::test_tile_kernel, _in_place, _fp32_accumulate (mi_reduce_bcast;
                           fan_fold, the fold fan_kernel runs)
  bcast_stride_kernel      test_gpu_bcast_bounds::test_stride_kernel_under_grid_cap, test_element_loop_*
  reducek_kernel,          tools/probe_kernels.hpp, launched by tools/reduce_sweep.hip only: not in the
  reduce2b_kernel          product header, no library entry point reaches them
  bucket / tmp_buf layouts test_gpu_bounds::test_contiguous_ragged_chunks_in_one_bucket, test_packed_tmp_buf
  zero-copy (pinned)       test_gpu_host_bounds::test_zero_copy_pinned (mi_reduce_sync, mi_reduce_multi_sync)
  bounce buffers           test_gpu_host_bounds::test_bounce_buffers (pageable, at most 1 MiB)
  staged pipeline, Edges   test_gpu_host_bounds::test_staged_pipeline_one_chunk, _two_chunks (pageable, above 1 MiB)
  mi_copy_sync / convert   test_gpu_host_bounds::test_copy_sync_into_host, test_convert_sync_into_host,
                           test_convert_sync_two_chunks (d2h_pageable; staged_pipeline's second chunk)
  mi_reduce_start, split   test_gpu_host_bounds::test_start_wait, test_split_start
  drop-in on host buffers  test_gpu_host_bounds::test_dropin_*_on_host_buffers (CCL_COMP_HOST_MAX_BYTES=0, default)
  CPU host path            test_host_bounds (mi_host_reduce, mi_host_convert, mi_host_copy, the drop-in's
                           CPU path; again under MI_HOST_ISA=avx2 / avx512)
  any path, random shapes  test_gpu_fuzz, test_gpu_dispatch_fuzz (every operand's pads are random non-zero
                           bytes, checked)
"""
from __future__ import annotations

import functools

import numpy as np

import oracle
from tests.util import ALL_DTYPES, BF16, DT_NAME, FP16, FP32, FP64, OP_NAME, OPS, rand_array

# 16 KiB is the largest tile any kernel owns (the general kernel's
# kBlock * kUnroll = 1024 vectors of 16 bytes); the lean, batch, fan and copy
# tiles are 64 vectors = 1 KiB.  256 B more for a stray cache line or two.
GUARD = 16 * 1024 + 256

F_MINMAX_INOUT_FIRST, F_BF16_RNE, F_ACC_FP32 = 0x1, 0x2, 0x4


# ---- what the bounds tests share: dtypes, flags, tile-edge shapes ------------------

T_LEAN, T_GENERAL = 64, 1024  # 16-byte vectors per tile: lean / batch / fan / lean copy; general / grid-stride copy

# all 12 dtypes with the op rotating, then fp32, bf16, int8 and fp64 over the other ops
ROT = [(dt, i % 4) for i, dt in enumerate(ALL_DTYPES)]
DT_OP = ROT + [(dt, op) for dt in (FP32, BF16, 0, FP64) for op in OPS if (dt, op) not in ROT]
DT_OP_IDS = [f"{DT_NAME[d]}-{OP_NAME[o]}" for d, o in DT_OP]
ROT_IDS = DT_OP_IDS[:len(ROT)]


def es_of(dt):
    return np.dtype(oracle.NP_DTYPE[dt]).itemsize


def ref_flags(dt):
    """The flags under which the library reproduces ccl_comp_reduce: bf16 as
    the avx512bf impl, fp16 as avx512f."""
    return F_MINMAX_INOUT_FIRST | F_BF16_RNE if dt == BF16 else (F_MINMAX_INOUT_FIRST if dt == FP16 else 0)


def tile_shapes(es, T):
    """(count, output misalignment in bytes): bodies of 0, 1, T-1, T, T+1 and
    2T+1 vectors x scalar heads x scalar tails of 0, 1 and 16/es - 1
    elements, and one element at misalignment es (count < head)."""
    per = 16 // es
    edge = sorted({0, 1, per - 1})
    out = [(h + b * per + t, (16 - h * es) % 16) for b in (0, 1, T - 1, T, T + 1, 2 * T + 1) for h in edge
           for t in edge]
    return out + [(1, es % 16)]


def oracle_fold(ins, dt, op, flags, fp16_impl=oracle.FP16_AVX512F):
    """The oracle's left fold of `ins` under the semantic variant `flags`
    (include/mi_reduce.h) selects.  fp16_impl = oracle.FP16_AVX512FP16 is
    MI_F_FP16_NATIVE_MINMAX's min / max in storage precision."""
    if flags & F_ACC_FP32:
        return oracle.lp_fanin_acc_fp32(ins, dt, op, dt == FP16 or bool(flags & F_BF16_RNE),
                                        bool(flags & F_MINMAX_INOUT_FIRST))
    bimpl = oracle.BF16_AVX512BF if flags & F_BF16_RNE else (
        oracle.BF16_AVX512F if flags & F_MINMAX_INOUT_FIRST else oracle.BF16_SCALAR)
    return oracle.fanin(ins, dt, op, bimpl, fp16_impl)


def _bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize])


def guard_conditions(in_guards, out_guard, dt, op, flags, inplace):
    """Per position: True where the output-side guard fails to differ from
    (a) the fold of the operands' guards, (b) the fold of zeros, (c) zero."""
    k = len(in_guards)
    ob = _bits(out_guard)
    bad = ob == 0  # (c)
    zeros = [np.zeros_like(out_guard) for _ in range(k)]
    bad |= ob == _bits(oracle_fold(zeros, dt, op, flags))  # (b)
    if not (inplace and k == 1):  # x = fold(x) is the identity: nothing is launched for it
        bad |= ob == _bits(oracle_fold(list(in_guards), dt, op, flags))  # (a)
    return bad


def guard_elems(dt, op, k, n, flags=0, inplace=False, seed=0, max_rounds=64):
    """Guard contents for a k-input reduce: `n` elements beside each input
    and beside the output.  Returns (in_guards, out_guard); in place the
    output's guard is the accumulator's, in_guards[0].  Positions are redrawn
    until guard_conditions() holds nowhere."""
    draw = lambda j, r: rand_array(dt, n, seed=(seed * 131 + j) * 97 + r + 1, op=op, specials=False)  # noqa: E731
    ing = [draw(j, 0) for j in range(k)]
    out = ing[0] if inplace else draw(k, 0)
    for r in range(1, max_rounds + 1):
        bad = guard_conditions(ing, out, dt, op, flags, inplace)
        if not bad.any():
            return ing, out
        for j in range(k):
            ing[j][bad] = draw(j, r)[bad]
        if not inplace:
            out[bad] = draw(k, r)[bad]
    raise AssertionError(f"guard_elems did not converge: dtype {dt} op {op} k {k} flags {flags:#x}")


@functools.lru_cache(maxsize=32)
def reduce_guards(dt, op, k, n, flags, inplace):
    """guard_elems for the span before and the span after each operand, drawn
    once per kind of reduce (the arrays are copied into arenas, never
    changed)."""
    return guard_elems(dt, op, k, n, flags, inplace, seed=1), guard_elems(dt, op, k, n, flags, inplace, seed=2)


class Op:
    """One operand placed in an arena."""

    def __init__(self, arena, name, role, off, array):
        self.arena, self.name, self.role, self.off = arena, name, role, off
        self.dtype, self.count, self.nbytes = array.dtype, array.size, array.nbytes
        self.ptr = arena.base + off

    @property
    def end(self):
        return self.off + self.nbytes


class Arena:
    """kind: "device" (torch uint8 CUDA tensor), "pinned" (torch pinned host
    memory) or "pageable" (numpy).  Contents are built on the host and reach
    a device arena in one copy at snapshot()."""

    def __init__(self, nbytes, kind, seed=0):
        self.kind = kind
        nbytes = int(nbytes) + 512
        fill = np.random.default_rng(seed).integers(1, 255, nbytes, dtype=np.uint8)  # 1..254
        if kind == "device":
            import torch
            self.t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            self.mem = fill  # staged; uploaded by snapshot()
            raw = self.t.data_ptr()
        elif kind == "pinned":
            import torch
            self.t = torch.from_numpy(fill).pin_memory()
            self.mem = self.t.numpy()  # the pinned memory itself
            raw = self.t.data_ptr()
        elif kind == "pageable":
            self.mem = fill
            raw = fill.ctypes.data
        else:
            raise ValueError(kind)
        skip = -raw % 256
        self.mem = self.mem[skip:]
        self.base = raw + skip  # 256-byte aligned: `mis` below is the true misalignment
        self.size = self.mem.size
        self.cursor = 0
        self.ops = []
        self.outputs = []  # (off, nbytes) that the call may write
        self.snap = None
        self.cur = None

    # ---- carving ---------------------------------------------------------
    def place(self, array, mis=0, role="in", name=None, guards=None):
        """Carve `array` at byte misalignment `mis` (mod 16) with GUARD bytes
        of arena on each side.  role "out" / "inout" declares its range
        writable.  guards = (before, after): element arrays written right
        before and right after the operand (from guard_elems)."""
        assert self.snap is None, "place() after snapshot()"
        array = np.ascontiguousarray(array)
        off = (self.cursor + GUARD + 15) // 16 * 16 + mis % 16
        end = off + array.nbytes
        assert end + GUARD <= self.size, "arena too small"
        self.mem[off:end] = array.view(np.uint8).reshape(-1)
        if guards is not None:
            before, after = (np.ascontiguousarray(g).view(np.uint8).reshape(-1) for g in guards)
            assert before.size <= GUARD and after.size <= GUARD
            self.mem[off - before.size:off] = before
            self.mem[end:end + after.size] = after
        self.cursor = end + GUARD
        op = Op(self, name or f"op{len(self.ops)}", role, off, array)
        self.ops.append(op)
        if role in ("out", "inout"):
            self.outputs.append((off, array.nbytes))
        return op

    def sub(self, parent, elem_off, count, role="in", name=None):
        """A sub-range of a placed operand (a chunk of a bucket) as an operand
        of its own; role "out" / "inout" declares it writable."""
        es = parent.dtype.itemsize
        view = np.empty(count, parent.dtype)
        op = Op(self, name or f"{parent.name}[{elem_off}:{elem_off + count}]", role, parent.off + elem_off * es, view)
        if role in ("out", "inout"):
            self.outputs.append((op.off, op.nbytes))
        return op

    def place_reduce(self, ins, dt, op, flags, mis, inplace, out_mis=0, tag=""):
        """The operands of one reduce, each between guards from guard_elems
        (so that a read-modify-write or zero-fill spill changes bits).
        mis[j]: byte misalignment of input j.  Returns (inputs, out)."""
        k = len(ins)
        es = ins[0].itemsize
        n = GUARD // es
        (gb_in, gb_out), (ga_in, ga_out) = reduce_guards(dt, op, k, n, flags, inplace)
        placed = []
        for j, x in enumerate(ins):
            role = "inout" if inplace and j == 0 else "in"
            placed.append(self.place(x, mis[j], role, f"{tag}in{j}", (gb_in[j], ga_in[j])))
        if inplace:
            return placed, placed[0]
        # the output starts as non-zero noise of the dtype, never as zeros
        noise = rand_array(dt, ins[0].size, seed=len(self.ops) + 7, op=op, specials=False)
        return placed, self.place(noise, out_mis, "out", f"{tag}out", (gb_out, ga_out))

    # ---- before / after ---------------------------------------------------
    def snapshot(self):
        """Call after every operand is placed and before the call under test."""
        if self.kind == "device":
            import torch
            skip = self.base - self.t.data_ptr()
            self.t[skip:].copy_(torch.from_numpy(self.mem))
            torch.cuda.synchronize()
        self.snap = self.mem.copy()

    def fetch(self):
        if self.kind == "device":
            skip = self.base - self.t.data_ptr()
            self.cur = self.t[skip:].cpu().numpy()
        else:
            self.cur = self.mem.copy()
        return self.cur

    def check(self, outputs=None, what=""):
        """Fetch the arena and require every byte outside the writable ranges
        (`outputs`: operands, default those placed as "out" / "inout") to
        equal the snapshot.  read() then returns operands as the call left
        them."""
        assert self.snap is not None, "check() without snapshot()"
        cur = self.fetch()
        ranges = self.outputs if outputs is None else [(o.off, o.nbytes) for o in outputs]
        changed = cur != self.snap
        for off, nb in ranges:
            changed[off:off + nb] = False
        bad = np.flatnonzero(changed)
        if bad.size:
            raise AssertionError(f"{what + ': ' if what else ''}{bad.size} bytes outside the output changed "
                                 f"({self.kind} arena): " + "; ".join(self.describe(int(b)) for b in bad[:4])
                                 + f"; last at {int(bad[-1])}")

    def describe(self, b):
        """Where byte offset `b` lies relative to the nearest operand."""
        best = None
        for o in self.ops:
            if o.off <= b < o.end:
                d, txt = 0, f"byte {b - o.off} inside {o.role} operand {o.name}"
            elif b < o.off:
                d, txt = o.off - b, f"{o.off - b} bytes before {o.role} operand {o.name}"
            else:
                d, txt = b - o.end + 1, f"{b - o.end} bytes after the end of {o.role} operand {o.name}"
            if best is None or d < best[0]:
                best = (d, txt)
        where = best[1] if best else "no operand placed"
        return f"offset {b} ({where}): {int(self.snap[b]):#04x} -> {int(self.cur[b]):#04x}"

    def read(self, op, fresh=False):
        if fresh or self.cur is None:
            self.fetch()
        return self.cur[op.off:op.off + op.nbytes].view(op.dtype).copy()

    def original(self, op):
        return self.snap[op.off:op.off + op.nbytes].view(op.dtype).copy()


def arena_bytes(operand_nbytes, n_operands):
    """Arena size for operands of the given total size."""
    return int(operand_nbytes) + n_operands * (2 * GUARD + 32) + GUARD
