"""Shared helpers for the parity tests: seeded inputs (with the special
values the reference's semantics distinguish, NaNs with payloads of both
signs among them), numpy<->device transfer and the comparison rule
(bit-exact, NaN payloads included for every type: the kernels and the host
path restate x86's NaN rules for the reference's AVX-512 paths and for its
compiled CCL_REDUCE, tests/golden/ref_comp_vectors.npz)."""
from __future__ import annotations

import numpy as np

import oracle

# ccl::datatype ids
INT_DTYPES = [0, 1, 2, 3, 4, 5, 6, 7]
FP16, FP32, FP64, BF16 = 8, 9, 10, 11
ALL_DTYPES = INT_DTYPES + [FP16, FP32, FP64, BF16]
OPS = [0, 1, 2, 3]
DT_NAME = {0: "int8", 1: "uint8", 2: "int16", 3: "uint16", 4: "int32", 5: "uint32", 6: "int64", 7: "uint64",
           8: "float16", 9: "float32", 10: "float64", 11: "bfloat16"}
OP_NAME = {0: "sum", 1: "prod", 2: "min", 3: "max"}

F32_SPECIALS = np.concatenate([
    np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, -np.nan, 1e-40, -1e-40, 1e-45,
              3.4e38, -3.4e38, 1.17549435e-38, 65504.0, 6.1e-5, 5.96e-8, 2.0 ** -126], dtype=np.float32),
    # quiet NaNs with payloads of both signs and a signalling NaN
    np.array([0x7FC00123, 0xFFC00456, 0x7F800005], dtype=np.uint32).view(np.float32)])


def rand_array(dtype: int, n: int, seed: int, op: int = 0, specials: bool = True) -> np.ndarray:
    """Seeded input of ccl datatype `dtype` (storage dtype as in oracle.NP_DTYPE)."""
    rng = np.random.default_rng(seed)
    st = oracle.NP_DTYPE[dtype]
    if dtype in INT_DTYPES:
        info = np.iinfo(st)
        if op == 1:  # keep products from being all-zero quickly; wraps still exercised
            a = rng.integers(-3, 4, size=n).astype(np.int64)
            if info.min == 0:
                a = np.abs(a)
            a = a.astype(st)
        else:
            a = rng.integers(info.min, info.max, size=n, endpoint=True, dtype=st)
        if specials and n > 8:
            idx = rng.choice(n, size=min(n, 8), replace=False)
            a[idx[:4]] = info.min
            a[idx[4:]] = info.max
        return a
    if dtype == FP64:
        a = rng.standard_normal(n) * (10.0 ** rng.integers(-3, 4, size=n))
        if specials and n > 40:
            idx = rng.choice(n, size=len(F32_SPECIALS) + 3, replace=False)
            with np.errstate(invalid="ignore"):  # the signalling NaN quiets on widening
                a[idx[:len(F32_SPECIALS)]] = F32_SPECIALS.astype(np.float64)
            a[idx[0]] = 1e-310  # fp64 denormal
            a.view(np.uint64)[idx[len(F32_SPECIALS):]] = np.array(  # fp64 NaN payloads, both signs, signalling
                [0x7FF8000000000123, 0xFFF8000000000456, 0x7FF0000000000007], np.uint64)
        return a
    f = (rng.standard_normal(n) * (2.0 ** rng.integers(-8, 9, size=n))).astype(np.float32)
    if specials and n > 40:
        idx = rng.choice(n, size=len(F32_SPECIALS), replace=False)
        f[idx] = F32_SPECIALS
    if dtype == FP32:
        return f
    if dtype == BF16:
        b = oracle.f32_to_bf16(f, rne=True)
        if specials and n > 40:  # bf16 denormals and tiny values
            idx = rng.choice(n, size=6, replace=False)
            b[idx] = np.array([0x0001, 0x8001, 0x007F, 0x0080, 0x7F7F, 0xFF7F], np.uint16)
        return b
    # fp16
    h = oracle.f32_to_fp16(np.clip(f, -60000, 60000))
    if specials and n > 40:
        idx = rng.choice(n, size=8, replace=False)
        h[idx] = np.array([0x0001, 0x8001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0x7E00], np.uint16)
    return h


def is_nan_bits(a: np.ndarray, dtype: int) -> np.ndarray:
    if dtype == BF16:
        return ((a & 0x7F80) == 0x7F80) & ((a & 0x007F) != 0)
    if dtype == FP16:
        return ((a & 0x7C00) == 0x7C00) & ((a & 0x03FF) != 0)
    if dtype in (FP32, FP64):
        return np.isnan(a)
    return np.zeros(a.shape, bool)


# NaN payloads count for every type.  Round 2 left the both-NaN choice of
# float/double CCL_REDUCE and of keep-precision's fp32 scratch fold unpinned
# (a compiler-vectorized `inout op= in`); the reference's own compiled
# comp.cpp now pins it (tests/golden/ref_comp_vectors.npz: inout's NaN wins,
# inf - inf gives 0xFFC00000), and the kernels, the host path and the oracle
# restate that rule.  nan_payload=False remains for callers that compare
# against something that does not model payloads (e.g. numpy).


def assert_same(got: np.ndarray, exp: np.ndarray, dtype: int, what: str = "", nan_payload=True) -> None:
    """Bit-exact comparison, NaN payloads included (nan_payload=False: two
    NaNs compare equal)."""
    assert got.shape == exp.shape and got.itemsize == exp.itemsize
    iv = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.itemsize]
    cand = np.flatnonzero(got.view(iv) != exp.view(iv))
    if cand.size and not nan_payload:
        both_nan = is_nan_bits(got[cand], dtype) & is_nan_bits(exp[cand], dtype)
        cand = cand[~both_nan]
    if cand.size:
        i = cand
        raise AssertionError(f"{what}: {len(i)} of {got.size} elements differ; first at {i[:5].tolist()}: "
                             f"got {got[i[:5]].tolist()} expected {exp[i[:5]].tolist()}")


# ---- device transfer (torch is plumbing only) ----------------------------
_SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def guard_fill(nbytes: int, guard_seed: int) -> np.ndarray:
    """Seeded random bytes in 1..254: a canary with no zero byte, so that a
    stray store of zeros (a lane past the end that loaded zeros) shows."""
    return np.random.default_rng(guard_seed).integers(1, 255, nbytes, dtype=np.uint8)


def padded(a: np.ndarray, pad_elems: int = 0, offset_elems: int = 0, guard_seed=None) -> np.ndarray:
    """`a` with `offset_elems` elements in front and `pad_elems` behind:
    zeros, or guard_fill(guard_seed) bytes."""
    raw = np.zeros(a.size + pad_elems + offset_elems, a.dtype)
    raw[offset_elems:offset_elems + a.size] = a
    if guard_seed is not None:
        front, back = _guard_regions(a.itemsize, pad_elems, offset_elems, guard_seed)
        raw[:offset_elems] = front.view(a.dtype)
        raw[offset_elems + a.size:] = back.view(a.dtype)
    return raw


def _guard_regions(es: int, pad_elems: int, offset_elems: int, guard_seed: int):
    fill = guard_fill((offset_elems + pad_elems) * es, guard_seed)
    return fill[:offset_elems * es], fill[offset_elems * es:]


def to_dev(a: np.ndarray, pad_elems: int = 0, offset_elems: int = 0, guard_seed=None):
    """Copy to a fresh device buffer; returns (tensor_holder, device_ptr).
    `offset_elems` shifts the data inside the buffer to test misaligned
    pointers.  With `guard_seed` the pad and offset regions hold seeded random
    non-zero bytes instead of zeros; guards_intact() checks them afterwards."""
    import torch
    es = a.itemsize
    raw = padded(a, pad_elems, offset_elems, guard_seed)
    t = torch.from_numpy(raw.view(_SIGNED[es])).cuda()
    return t, t.data_ptr() + offset_elems * es


def from_dev(t, like: np.ndarray, offset_elems: int = 0) -> np.ndarray:
    host = t.cpu().numpy().view(like.dtype)
    return host[offset_elems:offset_elems + like.size].copy()


def guards_intact(t, like: np.ndarray, offset_elems: int, guard_seed: int, what: str = "") -> None:
    """The offset and pad regions of a buffer made by to_dev(like, ...,
    guard_seed=guard_seed) (or its host counterpart from padded(): a numpy
    array or a pinned tensor) still hold their fill."""
    total = t.size if isinstance(t, np.ndarray) else t.numel()
    esz = t.itemsize if isinstance(t, np.ndarray) else t.element_size()
    n_lo, n_hi = offset_elems * like.itemsize // esz, (offset_elems + like.size) * like.itemsize // esz
    flat = t.reshape(-1)

    def region(a, b):  # only the guards travel back from the device
        part = flat[a:b]
        return (part if isinstance(part, np.ndarray) else part.cpu().numpy()).view(np.uint8)

    pad_elems = (total * esz) // like.itemsize - offset_elems - like.size
    front, back = _guard_regions(like.itemsize, pad_elems, offset_elems, guard_seed)
    for got, fill, side in ((region(0, n_lo), front, "before the operand"), (region(n_hi, total), back, "after its end")):
        bad = np.flatnonzero(got != fill)
        if bad.size:
            b = int(bad[0])
            d = got.size - b if side.startswith("before") else b
            raise AssertionError(f"{what}: {bad.size} guard bytes {side} changed; first {d} bytes {side}: "
                                 f"{int(fill[b]):#04x} -> {int(got[b]):#04x}")


def convert_expected(src: np.ndarray, sdt: int, ddt: int, flags: int) -> np.ndarray:
    """The oracle's fp32 <-> bf16 / fp16 array conversion under mi_convert's
    flags (0x2 RNE, 0x8 the truncated count % 16 tail)."""
    n = src.size
    if sdt == FP32 and ddt == BF16:
        rne, tail = bool(flags & 0x2), bool(flags & 0x8)
        lim = (n // 16) * 16 if (rne and tail) else (n if rne else 0)
        return np.concatenate([oracle.f32_to_bf16(src[:lim], True), oracle.f32_to_bf16(src[lim:], False)])
    if sdt == FP32:
        return oracle.f32_to_fp16(src)
    return oracle.bf16_to_f32(src) if sdt == BF16 else oracle.fp16_to_f32(src)


def wait_os_threads_gone(native_ids, timeout=60.0):
    """Wait until the OS threads `native_ids` (threading.get_native_id() of
    each) have exited.  Python's Thread.join() returns when the thread's
    Python function ends, before the OS thread runs its thread_local
    destructors -- for the library, each thread's HIP context teardown
    (streams, staging buffers) -- so a GPU test that starts workers lets
    those teardowns finish here rather than overlap the next test."""
    import os
    import time
    t0 = time.monotonic()
    pending = set(native_ids)
    while pending and time.monotonic() - t0 < timeout:
        pending = {t for t in pending if os.path.exists(f"/proc/self/task/{t}")}
        if pending:
            time.sleep(0.005)
    return not pending
