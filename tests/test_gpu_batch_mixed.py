"""mi_reduce_batch_mixed on the GPU: one batch call per case, every destination
bit for bit tests.mixed_scaled.expected_mixed_scaled for that descriptor alone
(acc = the destination before the call when widening).  Both sides are carved
from one sentinel-filled byte arena each, and the whole destination arena is
compared with the one built on the CPU: every gap is a bounds check.  The batch
(tile = 512 elements, group = 8, bf16 tail group = 16): counts from scalar-only
to three tiles at destination misalignments 0 and one element, sources on and
off the destination's grid; 65 in the table (two launches); in mid-batch one
source not aligned to its element size (its own element-loop launch)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from oneccl_amd import _lib
from tests.mixed import PAIR_IDS, PAIRS, knobs
from tests.mixed_scaled import expected_mixed_scaled
from tests.util import BF16, FP16, FP32, rand_array

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 7, 8, 9, 17, 33, 511, 512, 513, 1031]
SENTINEL, PAD, GAP = 0x5A, 4096, 32
NP = {BF16: np.uint16, FP16: np.uint16, FP32: np.uint32}
# +Inf, -Inf, a quiet NaN and a signalling NaN with payloads, among finite values of mixed sign
SPECIALS = {BF16: [0x7F80, 0xFF80, 0x7FC1, 0x7F85], FP16: [0x7C00, 0xFC00, 0x7E01, 0x7D05],
            FP32: [0x7F800000, 0xFF800000, 0x7FC00123, 0x7F800005]}
# position in a descriptor of >= 9 elements: which special, in the source and in the destination
PLANT_SRC, PLANT_DST = {0: 0, 2: 0, 3: 2, 4: 3, -1: 3, -3: 1}, {1: 1, 2: 1, 3: 3, -1: 2, -2: 0, -3: 1}


@functools.lru_cache(maxsize=None)
def _batch(idt, odt):
    """The two arenas as built on the host and each descriptor's (source offset, destination offset, count)."""
    esi, eso = NP[idt]().itemsize, NP[odt]().itemsize
    lay = []  # (count, destination misalignment, source misalignment), bytes mod 16, in batch order
    for dmis in (0, eso):
        on = -((16 - dmis) % 16 // eso) * esi % 16  # the source's body starts on a 16-byte boundary too
        lay += [(c, dmis, smis) for smis in (on, (on + esi) % 16) for c in COUNTS]
    lay += [(c, eso, 0) for c in (COUNTS[1:] * 3)[:65 - 40]]  # 4 * 10 non-empty so far: 65 in the table
    lay.insert(len(lay) // 2, (777, 0, esi // 2))              # not aligned to its element size
    src, dst = (np.full(2 * PAD + sum(c * es + GAP + 64 for c, _, _ in lay), SENTINEL, np.uint8) for es in (esi, eso))
    cs, cd, descs = PAD, PAD, []
    for i, (c, dmis, smis) in enumerate(lay):
        so, do = (cs + 15) // 16 * 16 + GAP + smis, (cd + 15) // 16 * 16 + GAP + dmis
        cs, cd = so + c * esi, do + c * eso
        descs.append((so, do, c))
        if c:
            x = rand_array(idt, c, seed=9100 + i, specials=False).view(NP[idt])
            y = rand_array(odt, c, seed=9500 + i, specials=False).view(NP[odt])
            for a, plant, dt in ((x, PLANT_SRC, idt), (y, PLANT_DST, odt)) if c >= 9 else []:
                a[list(plant)] = [SPECIALS[dt][k] for k in plant.values()]
            src[so:cs], dst[do:cd] = x.view(np.uint8), y.view(np.uint8)
    return src, dst, descs


@functools.lru_cache(maxsize=None)
def _expected(idt, odt, flags, scale):
    src, dst, descs = _batch(idt, odt)
    exp = dst.copy()
    for so, do, c in descs:
        if c:
            x = src[so:so + c * NP[idt]().itemsize].copy().view(np.float32 if idt == FP32 else np.uint16)
            acc = dst[do:do + c * 4].copy().view(np.float32) if odt == FP32 else None
            exp[do:do + c * NP[odt]().itemsize] = expected_mixed_scaled([x], idt, odt, flags, scale, acc).view(np.uint8)
    return exp


def _run(idt, odt, flags, scale, cap):
    import torch
    src, dst, descs = _batch(idt, odt)

    def upload(a):
        t = torch.empty(a.size + 256, dtype=torch.uint8, device="cuda")
        t = t[-t.data_ptr() % 256:][:a.size]  # 256-byte aligned: the offsets are the true misalignments
        return t.copy_(torch.from_numpy(a.copy()))

    ts, td = upload(src), upload(dst)
    arr = _lib.desc_array([(ts.data_ptr() + so, td.data_ptr() + do, c) for so, do, c in descs])
    with knobs(max_blocks=cap):
        _lib.check(_lib.mi().mi_reduce_batch_mixed(arr, len(descs), idt, odt, 0, flags, scale,
                                                   torch.cuda.current_stream().cuda_stream), "mi_reduce_batch_mixed")
    torch.cuda.synchronize()
    got, exp = td.cpu().numpy(), _expected(idt, odt, flags, scale)
    bad = np.flatnonzero(got != exp)
    assert not bad.size, (f"grid cap {cap}: {bad.size} bytes differ, first at {bad[0]}; descriptors at or before it "
                          f"(source offset, destination offset, count): {[x for x in descs if x[1] <= bad[0]][-2:]}")
    assert np.array_equal(ts.cpu().numpy(), src), "a source changed"


@pytest.mark.parametrize("scale", [1.0, 1 / 3], ids=["one", "third"])
@pytest.mark.parametrize("idt,odt,flags", PAIRS, ids=PAIR_IDS)
def test_batch(idt, odt, flags, scale):
    """At scale 1/3 the same batch again under mi_set_max_blocks(4), on fresh arenas: every descriptor then gets a
    launch of its own (the existing call's)."""
    _run(idt, odt, flags, scale, 0)
    if scale != 1.0:
        _run(idt, odt, flags, scale, 4)
