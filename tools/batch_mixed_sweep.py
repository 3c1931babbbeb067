#!/usr/bin/env python3
"""mi_reduce_batch_mixed against the sequence it replaces, in one process:

  batch     one mi_reduce_batch_mixed call of 64 descriptors
  sequence  the 64 mi_reduce_bcast_mixed_scaled calls (k = 1, m = 1; widening
            with acc = the destination) that write the same bytes

for bf16 -> fp32 and fp32 -> bf16 at 4 KiB, 64 KiB, 1 MiB and 16 MiB of
destination per descriptor.  Warm, event-timed: a trial is `reps` back-to-back
runs between two events (reps sized so a trial lasts about 50 ms), the two
variants alternate, and the median, minimum and maximum over the trials are
printed, one JSON line per (direction, size, variant).  Times include the
host's enqueue through ctypes, with every argument array built beforehand."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from oneccl_amd import _lib  # noqa: E402

FP32, BF16, SUM, N_DESC, SCALE = 9, 11, 0, 64, 1e-3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4 << 10, 64 << 10, 1 << 20, 16 << 20])
    args = ap.parse_args()
    mi, stream = _lib.mi(), torch.cuda.current_stream().cuda_stream
    tdt = {FP32: torch.float32, BF16: torch.bfloat16}
    for idt, odt in ((BF16, FP32), (FP32, BF16)):
        for nbytes in args.sizes:
            n = nbytes // (4 if odt == FP32 else 2)
            src = [torch.randn(n, device="cuda").to(tdt[idt]) for _ in range(N_DESC)]
            dst = [torch.zeros(n, dtype=tdt[odt], device="cuda") for _ in range(N_DESC)]
            descs = _lib.desc_array([(s.data_ptr(), d.data_ptr(), n) for s, d in zip(src, dst)])
            seq = [(_lib.void_ptr_array([s.data_ptr()]), d.data_ptr() if odt == FP32 else None,
                    _lib.void_ptr_array([d.data_ptr()])) for s, d in zip(src, dst)]

            def batch():
                _lib.check(mi.mi_reduce_batch_mixed(descs, N_DESC, idt, odt, SUM, 0x2, SCALE, stream))

            def sequence():
                for pin, acc, pout in seq:
                    _lib.check(mi.mi_reduce_bcast_mixed_scaled(pin, 1, idt, acc, pout, 1, odt, n, SUM, 0x2, SCALE, stream))

            def timed(fn, reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) / reps  # ms per run

            variants = {"batch": batch, "sequence": sequence}
            reps = {}
            for name, fn in variants.items():  # warm up, then size a trial to about 50 ms
                timed(fn, 3)
                reps[name] = max(5, min(500, int(50.0 / max(timed(fn, 5), 1e-3))))
            times = {name: [] for name in variants}
            for _ in range(args.trials):
                for name, fn in variants.items():
                    times[name].append(timed(fn, reps[name]))
            for name, t in times.items():
                print(json.dumps(dict(pair=f"{idt}->{odt}", dst_bytes=nbytes, descriptors=N_DESC, variant=name,
                                      reps=reps[name], trials=len(t), median_ms=round(statistics.median(t), 5),
                                      min_ms=round(min(t), 5), max_ms=round(max(t), 5))), flush=True)


if __name__ == "__main__":
    main()
