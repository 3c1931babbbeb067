"""Inputs whose NaN and Inf bits tell the kernels' NaN paths apart, for the
entry points added after mi_reduce and mi_reduce_multi (mi_reduce_batch,
mi_reduce_bcast, mi_reduce_bcast_scaled).  CPU only: tests/test_nanvec.py
checks what is built here, tests/test_gpu_nan_paths.py runs it.

Three sources:

  golden   the reference's own vectors (tests/golden/*.npz through
           tests.refvec and tests.refcomp), re-addressed as fold inputs: the
           reference's inout is inputs[0], its in inputs[1]; a batch or
           keep-precision case is inout followed by the chunks at their
           offsets.  Expected values are the reference's; no oracle.
  table    special_table(): every ordered pair of 16 special values (quiet,
           signalling and payload NaNs of both signs, +-inf, +-0, +-max,
           +-1, the smallest denormal and normal) between inputs[0] and each
           other input in turn, the rest 1.0, with pairs in the scalar head,
           the scalar tail, the first tile and the last, partial tile.
           Expected values from fold() (tests.guard.oracle_fold).
  sparse   tests.test_gpu_nan._inputs: about 1 % of elements special, so most
           lanes of a wave stay on the fast path and a few refold; for a
           product of three or more inputs, finite rows whose partial product
           overflows and then meets a zero.  Expected values from fold().

rand_array (tests.util) narrows its float32 specials, so the bf16 / fp16
arrays it makes hold no payload and no signalling NaN, and two of its
specials practically never meet at one index."""
from __future__ import annotations

import functools

import numpy as np

import oracle
from tests import refcomp, refvec
from tests.guard import oracle_fold
from tests.test_gpu_nan import BF16_SPECIAL, FP16_SPECIAL
from tests.test_gpu_nan import _inputs as sparse_inputs  # noqa: F401  (re-exported)
from tests.test_gpu_ref_comp_vectors import _keep_flags
from tests.test_gpu_ref_vectors import BF16_FLAGS, FP16_FLAGS
from tests.util import BF16, FP16, FP32, FP64

F_ACC_FP32, F_TAIL, F_NATIVE = 0x4, 0x8, 0x10
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
T = 64  # 16-byte vectors per tile of the batch, fan and fan-out kernels

# name, dtype, flags: every semantic variant that has a reference
# (include/mi_reduce.h).  bf16: scalar, avx512f, avx512bf, keep-precision
# under avx512f, fp32 accumulation with RNE and the MINPS order; fp16:
# f16c / avx512f, avx512fp16, fp32 accumulation.
VARIANTS = [("bf16-0x0", BF16, 0x0), ("bf16-0x1", BF16, 0x1), ("bf16-0x3", BF16, 0x3), ("bf16-0x4", BF16, 0x4),
            ("bf16-0x7", BF16, 0x7), ("fp16-0x1", FP16, 0x1), ("fp16-0x11", FP16, 0x11), ("fp16-0x5", FP16, 0x5),
            ("fp32", FP32, 0), ("fp64", FP64, 0)]
# keep-precision under avx512bf (MI_F_BF16_TAIL_TRUNC16): the oracle does not
# model the truncated tail, so only the reference's `keep` vectors pin it
KEEP_TAIL = ("bf16-keep-tail", BF16, _keep_flags(2))
assert KEEP_TAIL[2] & F_TAIL and _keep_flags(1) == 0x4

# quiet NaN +-, signalling NaN +-, payload NaN + (signalling) and - (quiet), +-inf, +-0, +-max, +-1,
# the smallest denormal, the smallest normal.  The first eleven of bf16 and fp16 are test_gpu_nan's.
SPECIALS = {
    BF16: np.array(BF16_SPECIAL[:5] + [0xFFE3] + BF16_SPECIAL[5:] + [0x3F80, 0xBF80, 0x0001, 0x0080], np.uint16),
    FP16: np.array(FP16_SPECIAL[:5] + [0xFF23] + FP16_SPECIAL[5:] + [0x3C00, 0xBC00, 0x0001, 0x0400], np.uint16),
    FP32: np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FA00123, 0xFFC00456, 0x7F800000, 0xFF800000,
                    0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000, 0xBF800000, 0x00000001, 0x00800000],
                   np.uint32),
    FP64: np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001,
                    0x7FF4000000000123, 0xFFF8000000000456, 0x7FF0000000000000, 0xFFF0000000000000,
                    0x0000000000000000, 0x8000000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,
                    0x3FF0000000000000, 0xBFF0000000000000, 0x0000000000000001, 0x0010000000000000], np.uint64),
}
assert all(s.size == 16 and np.unique(s).size == 16 for s in SPECIALS.values())
I_QNAN, I_SNAN, I_PAYLOAD, I_PINF, I_NINF, I_ONE = 0, 2, 4, 6, 7, 12
# exponent mask, mantissa mask, quiet bit
FIELDS = {BF16: (0x7F80, 0x007F, 0x0040), FP16: (0x7C00, 0x03FF, 0x0200), FP32: (0x7F800000, 0x007FFFFF, 0x00400000),
          FP64: (0x7FF0000000000000, 0x000FFFFFFFFFFFFF, 0x0008000000000000)}
DEFAULT_NAN = {FP32: 0xFFC00000, FP64: 0xFFF8000000000000}  # x86's, of an invalid operation


def per_vec(dt):
    return 16 // np.dtype(oracle.NP_DTYPE[dt]).itemsize


def bits(a):
    return a.view(UINT[a.itemsize])


def nan_mask(a, dt):
    e, m, _ = FIELDS[dt]
    b = bits(a)
    return ((b & e) == e) & ((b & m) != 0)


def signalling_mask(a, dt):
    return nan_mask(a, dt) & ((bits(a) & FIELDS[dt][2]) == 0)


def head_tail(dt):
    """The scalar head and tail every table of `dt` is built with: both
    non-empty, the head the longest there is."""
    per = per_vec(dt)
    return per - 1, per // 2


def fold(ins, dt, op, flags):
    """oracle_fold, with MI_F_FP16_NATIVE_MINMAX selecting the avx512fp16 impl."""
    return oracle_fold(ins, dt, op, flags & ~F_NATIVE,
                       fp16_impl=oracle.FP16_AVX512FP16 if flags & F_NATIVE else oracle.FP16_AVX512F)


# ---- b. the dense table -------------------------------------------------------------------

def pair_blocks(dt, k):
    """One block of 256 per j in 1..k-1: inputs[0] = repeat(S, 16), inputs[j]
    = tile(S, 16), every other input 1.0; for k = 1 repeat(S, 16) alone.
    The block of the last input comes first: a min or max that drops a NaN
    operand (the scalar bf16 impl, MINPS against a later 1.0) still ends in a
    NaN where the last input and the accumulator's start are both NaN, and
    the head, the tail and the partial tile are cut from this block."""
    S = SPECIALS[dt]
    one = S[I_ONE]
    rows = [[] for _ in range(k)]
    for j in range(max(k, 2) - 1, 0, -1):
        for i in range(k):
            rows[i].append(np.repeat(S, 16) if i == 0 else np.tile(S, 16) if i == j else np.full(256, one, S.dtype))
    return [np.concatenate(r) for r in rows]


def table_layout(dt, k):
    """(repeats, extra vectors) of special_table's body: the blocks repeated
    until they span two tiles, then the first vectors of the blocks again as
    the last, partial tile."""
    per = per_vec(dt)
    n = 256 * max(k - 1, 1)
    reps = -(-2 * T * per // n)
    extra = 17
    while (reps * n // per + extra) % T == 0:
        extra += 1
    return reps, extra


@functools.lru_cache(maxsize=None)
def _special_table(dt, k, head, tail):
    per = per_vec(dt)
    assert 0 <= head < per and 0 <= tail < per
    blocks = pair_blocks(dt, k)
    reps, extra = table_layout(dt, k)
    # the head starts at the pairs (signalling NaN, S), the tail at (payload NaN, S)
    h0, t0 = 16 * I_SNAN, 16 * I_PAYLOAD
    out = []
    for b in blocks:
        x = np.concatenate([b[h0:h0 + head]] + [b] * reps + [b[:extra * per], b[t0:t0 + tail]])
        x.setflags(write=False)
        out.append(x.view(oracle.NP_DTYPE[dt]))
    return tuple(out)


def special_table(dt, k, head, tail):
    """k read-only arrays: `head` leading elements, a body of whole 16-byte
    vectors (at least two tiles of 64 and a partial one), `tail` trailing
    elements, all cut from pair_blocks."""
    return list(_special_table(dt, k, head, tail))


def table_regions(dt, k, head, tail):
    """Element index ranges (lo, hi) of the scalar head, the first tile, the
    last (partial) tile and the scalar tail of special_table's arrays."""
    per = per_vec(dt)
    n = special_table(dt, k, head, tail)[0].size
    nvec = (n - head - tail) // per
    assert nvec > 2 * T and nvec % T and head + nvec * per + tail == n
    last = head + (nvec // T) * T * per
    return {"head": (0, head), "first tile": (head, head + T * per), "last tile": (last, head + nvec * per),
            "tail": (n - tail, n)}


@functools.lru_cache(maxsize=None)
def table_case(dt, flags, op, k):
    """(inputs, expected) of the table of `dt` at head_tail(dt), computed once
    and shared; all read-only."""
    ins = special_table(dt, k, *head_tail(dt))
    exp = fold(ins, dt, op, flags)
    exp.setflags(write=False)
    return ins, exp


@functools.lru_cache(maxsize=None)
def sparse_case(dt, flags, op, k, n):
    """(inputs, expected) of test_gpu_nan's sparse inputs; read-only."""
    ins = sparse_inputs(dt, k, n, op, seed=4000 + 100 * k + 10 * op + n % 89)
    exp = fold(ins, dt, op, flags)
    for x in ins + [exp]:
        x.setflags(write=False)
    return ins, exp


# ---- a. the reference's vectors, re-addressed ------------------------------------------------

def _case(key, dt, flags, op, ins, exp):
    ins = [np.ascontiguousarray(x) for x in ins]
    assert all(x.size == exp.size and x.dtype == exp.dtype for x in ins)
    return {"key": key, "dtype": dt, "flags": flags, "op": op, "ins": ins, "expected": exp}


@functools.lru_cache(maxsize=None)
def golden_two_input():
    """Every 2-input vector of a floating type: ins = [inout, in] cut to the
    case's count.  reduce1 (256 one-element calls of the reference's scalar
    path) is kept as one case of 256 elements, marked "calls"."""
    out = []
    for c in refvec.reduce_cases():
        n = c["count"]
        flags = (BF16_FLAGS if c["dtype"] == BF16 else FP16_FLAGS)[c["impl"]]
        out.append(_case(c["key"], c["dtype"], flags, c["op"], [c["b"][:n], c["a"][:n]], c["expected"][:n]))
    for kind in ("reduce", "reduce1", "bf16s"):
        for c in refcomp.cases(kind):
            if c["dtype"] in (FP32, FP64, BF16):
                d = _case(c["key"], c["dtype"], 0, c["op"], [c["b"], c["a"]], c["expected"])
                d["calls"] = c.get("calls", 0)
                out.append(d)
    return out


@functools.lru_cache(maxsize=None)
def golden_fans():
    """The chained 8-input fan-ins (bf16 and fp16, sum and max)."""
    return [_case(c["key"], c["dtype"], (BF16_FLAGS if c["dtype"] == BF16 else FP16_FLAGS)[c["impl"]], c["op"],
                  list(c["inputs"]), c["expected"]) for c in refvec.fan_cases()]


@functools.lru_cache(maxsize=None)
def golden_chunks():
    """ccl_comp_batch_reduce's vectors, k = 5: the storage-precision chain
    (fp32, fp64) and keep-precision mode (bf16 under _keep_flags)."""
    out = []
    for kind in ("batch", "keep"):
        for c in refcomp.cases(kind):
            if c["dtype"] not in (FP32, FP64, BF16):
                continue
            n = c["count"]
            ins = [c["b"]] + [c["buf"][o:o + n] for o in c["offsets"][1:]]
            out.append(_case(c["key"], c["dtype"], _keep_flags(c["impl"]) if kind == "keep" else 0, c["op"], ins,
                             c["expected"]))
    return out


def golden(cases, dt, flags, op=None):
    return [c for c in cases if c["dtype"] == dt and c["flags"] == flags and op in (None, c["op"])]
