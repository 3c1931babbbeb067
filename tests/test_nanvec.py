"""tests/nanvec.py makes what tests/test_gpu_nan_paths.py needs it to make:
the dense table and its oracle fold hold the signalling NaNs, the distinct
NaN bit patterns, the native-variant survivors, x86's default NaN and the
placements that tell the kernels' NaN paths apart, and the fold that gives
the table's expected values reproduces the reference's own vectors."""
from __future__ import annotations

import numpy as np
import pytest

from tests import nanvec as nv
from tests.nanvec import F_ACC_FP32, F_NATIVE, F_TAIL
from tests.util import BF16, FP16, FP32, FP64, assert_same

KS = [1, 2, 3, 9, 16]  # what the GPU file folds the table at
V_IDS = [v[0] for v in nv.VARIANTS]


def test_specials_are_what_they_are_called():
    for dt, S in nv.SPECIALS.items():
        nan, sig = nv.nan_mask(S, dt), nv.signalling_mask(S, dt)
        assert nan.tolist() == [True] * 6 + [False] * 10
        assert sig.tolist() == [False, False, True, True, True, False] + [False] * 10
        f = S.view({2: np.uint16, 4: np.float32, 8: np.float64}[S.itemsize])
        if dt in (FP32, FP64):
            assert f[6] == np.inf and f[7] == -np.inf and f[12] == 1 and f[13] == -1
            assert f[10] == np.finfo(f.dtype).max and f[15] == np.finfo(f.dtype).tiny and 0 < f[14] < f[15]
            assert np.signbit(f[9]) and f[9] == 0 and not np.signbit(f[8])
        else:
            import oracle
            w = (oracle.bf16_to_f32 if dt == BF16 else oracle.fp16_to_f32)(S)
            assert w[6] == np.inf and w[7] == -np.inf and w[12] == 1 and w[13] == -1 and w[10] == -w[11]
            assert 0 < w[14] < w[15] and np.signbit(w[9]) and w[9] == 0
            assert S[10] + 1 == S[6] and S[14] == 1 and S[15] == (0x0080 if dt == BF16 else 0x0400)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dt", [FP16, BF16, FP32, FP64], ids=["fp16", "bf16", "fp32", "fp64"])
def test_table_shape(dt, k):
    """Every ordered pair of specials between inputs[0] and each other input,
    the rest 1.0; a head, a body of two tiles and a partial one, a tail."""
    S, per = nv.SPECIALS[dt], nv.per_vec(dt)
    head, tail = nv.head_tail(dt)
    assert 0 < head < per and 0 < tail < per
    ins = nv.special_table(dt, k, head, tail)
    assert len(ins) == k and len({x.size for x in ins}) == 1
    regions = nv.table_regions(dt, k, head, tail)  # asserts two tiles and a partial one
    assert regions["last tile"][1] - regions["last tile"][0] < nv.T * per
    body = [nv.bits(x)[head:head + 256 * max(k - 1, 1)] for x in ins]
    for j in range(1, k):
        blk = slice(256 * (k - 1 - j), 256 * (k - j))  # the last input's block first
        pairs = set(zip(body[0][blk].tolist(), body[j][blk].tolist()))
        assert pairs == {(a, b) for a in S.tolist() for b in S.tolist()}
        for i in range(1, k):
            if i != j:
                assert (body[i][blk] == S[nv.I_ONE]).all()
    if k == 1:
        assert set(body[0].tolist()) == set(S.tolist())
    assert nv.signalling_mask(ins[0], dt).any()  # signalling inputs
    for x in ins:
        assert not x.flags.writeable


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("op", [0, 1, 2, 3])
@pytest.mark.parametrize("name,dt,flags", nv.VARIANTS, ids=V_IDS)
def test_table_fold_has_the_signal(name, dt, flags, op, k):
    ins, exp = nv.table_case(dt, flags, op, k)
    head, tail = nv.head_tail(dt)
    nan = nv.nan_mask(exp, dt)
    # signalling inputs, in every input that carries specials
    for j in range(k):
        assert nv.signalling_mask(ins[j], dt).any()
    # placement: a NaN-producing position in each region
    for where, (lo, hi) in nv.table_regions(dt, k, head, tail).items():
        assert hi > lo and nan[lo:hi].any(), where
    # distinct NaN patterns of a low-precision sum or product
    if dt in (BF16, FP16) and op in (0, 1):
        assert np.unique(nv.bits(exp)[nan]).size >= 4
    # the native variant keeps a signalling accumulator as stored
    if flags & F_NATIVE and op in (2, 3):
        assert nv.signalling_mask(exp, dt).any()
    if dt == FP16 and flags == 0x1 and op in (2, 3) and k > 1:
        assert not nv.signalling_mask(exp, dt).any()  # the fp32 route has quieted it
    # x86's default NaN at the inf - inf positions
    if dt in (FP32, FP64) and op == 0 and k > 1:
        b0 = nv.bits(ins[0])
        S = nv.SPECIALS[dt]
        hits = 0
        for j in range(1, k):
            bj = nv.bits(ins[j])
            for a, b in ((nv.I_PINF, nv.I_NINF), (nv.I_NINF, nv.I_PINF)):
                pos = (b0 == S[a]) & (bj == S[b])
                assert (nv.bits(exp)[pos] == nv.DEFAULT_NAN[dt]).all()
                hits += int(pos.sum())
        assert hits >= 2 * (k - 1)
    # k = 1: quieted under fp32 accumulation, the input's bytes without.  (bf16 widens by a shift, so it is
    # the RNE narrowing, VCVTNEPS2BF16, that quiets: truncated, 0x4, the bytes pass through as well.)
    if k == 1:
        if flags & F_ACC_FP32 and (dt == FP16 or flags & 0x2):
            assert nv.signalling_mask(ins[0], dt).any() and not nv.signalling_mask(exp, dt).any()
            sig = nv.signalling_mask(ins[0], dt)
            assert (nv.bits(exp)[sig] == nv.bits(ins[0])[sig] | nv.FIELDS[dt][2]).all()
        else:
            assert np.array_equal(nv.bits(exp), nv.bits(ins[0]))


@pytest.mark.parametrize("name,dt,flags", [v for v in nv.VARIANTS if v[1] in (BF16, FP16)],
                         ids=[v[0] for v in nv.VARIANTS if v[1] in (BF16, FP16)])
def test_sparse_inputs_refold_a_few_rows(name, dt, flags):
    """About 1 % special, and for a product of 3 the overflow-then-zero rows:
    x86's default NaN (narrowed) from finite inputs."""
    for op in (0, 1):
        ins, exp = nv.sparse_case(dt, flags, op, 3, 4096 + 13)
        rows = np.logical_or.reduce([nv.nan_mask(x, dt) | (nv.bits(x) & nv.FIELDS[dt][0] == nv.FIELDS[dt][0])
                                     for x in ins])
        assert 0 < rows.mean() < 0.05
        if op == 1:
            born = nv.nan_mask(exp, dt) & ~rows
            if dt == FP16 and flags & F_ACC_FP32:
                assert not born.any()  # 65504 ** 2 does not overflow the fp32 accumulator
            else:
                assert born.sum() >= 4
                assert (nv.bits(exp)[born] == (0xFFC0 if dt == BF16 else 0xFE00)).all()


# ---- the generator of the expected values against the reference's own vectors -------------------

def _modelled(c):
    return not c["flags"] & F_TAIL


def test_golden_cases_cover_every_variant():
    two = nv.golden_two_input()
    for name, dt, flags in nv.VARIANTS:
        if (dt, flags) in ((BF16, 0x4), (BF16, 0x7), (FP16, 0x5)):  # fp32 accumulation: k = 5 or the table only
            continue
        for op in range(4):
            assert nv.golden(two, dt, flags, op), (name, op)
    fans = nv.golden_fans()
    assert {(c["dtype"], c["flags"]) for c in fans} == {(BF16, 0x1), (BF16, 0x3), (FP16, 0x1), (FP16, 0x11)}
    assert all(len(c["ins"]) == 8 for c in fans)
    chunks = nv.golden_chunks()
    assert {(c["dtype"], c["flags"]) for c in chunks} == {(FP32, 0), (FP64, 0), (BF16, 0x4), nv.KEEP_TAIL[1:]}
    assert all(len(c["ins"]) == 5 for c in chunks)
    assert sum(c.get("calls", 0) == 256 for c in two) == 8  # reduce1: fp32 and fp64, four ops


@pytest.mark.parametrize("c", nv.golden_two_input() + nv.golden_fans() + [c for c in nv.golden_chunks() if _modelled(c)],
                         ids=lambda c: c["key"])
def test_fold_reproduces_the_reference(c):
    """nanvec.fold (oracle_fold with the fp16 impl chosen by the flags) on
    the golden inputs gives the golden expected arrays."""
    assert_same(nv.fold(c["ins"], c["dtype"], c["op"], c["flags"]), c["expected"], c["dtype"], c["key"])


@pytest.mark.parametrize("name,dt,flags", nv.VARIANTS, ids=V_IDS)
def test_host_path_folds_the_table(name, dt, flags):
    """The dispatcher's CPU side (mi_host_reduce) on the table, every op and
    k: the bits the device kernels are held to.  k = 1 under fp32 accumulation
    runs the conversions (a signalling fp16 NaN is quieted), it is no copy."""
    from oneccl_amd import _lib
    if not _lib.shim().mi_host_supported():
        pytest.skip("no AVX2/F16C: the dispatcher sends every bucket to the GPU")
    for op in range(4):
        for k in KS:
            ins, exp = nv.table_case(dt, flags, op, k)
            out = np.zeros_like(exp)
            arr = _lib.void_ptr_array([x.ctypes.data for x in ins])
            assert _lib.shim().mi_host_reduce(arr, k, out.ctypes.data, out.size, dt, op, flags) == 0
            assert_same(out, exp, dt, f"{name} op={op} k={k}")


def test_oracle_fold_default_is_unchanged():
    """Without fp16_impl, fp16 min / max go the fp32 route (avx512f)."""
    import oracle
    from tests.guard import oracle_fold
    ins = nv.special_table(FP16, 2, *nv.head_tail(FP16))
    for op in range(4):
        assert_same(oracle_fold(ins, FP16, op, 0x1), oracle.fanin(ins, FP16, op, oracle.BF16_AVX512BF,
                                                                  oracle.FP16_AVX512F), FP16)
    assert not np.array_equal(oracle_fold(ins, FP16, 2, 0x1), oracle_fold(ins, FP16, 2, 0x1, oracle.FP16_AVX512FP16))
