#!/usr/bin/env python3
"""mi_reduce_bcast_mixed_scaled against the unscaled call of the same shape and
against the sequence it replaces, in one process on the same seeded buffers:

  fused       one mi_reduce_bcast_mixed_scaled at scale 1 / k (the mean)
  unscaled    mi_reduce_bcast_mixed of the same k, m, acc and dtypes: the same
              streams without the multiply.  Timed in two slots of every round
              (A and B): A over B is that call's own spread, the range the
              fused call's time is held to.
  sequence    built only from calls that exist without the fused one.
              Widening: the unscaled call, then one in-place scaling pass per
              output (mi_reduce_bcast_scaled, k = m = 1, fp32).  Widening with
              acc: the unscaled call (no acc) into an fp32 scratch buffer, one
              in-place scaling pass over it, then an fp32 mi_reduce_bcast of
              {acc, scratch} into the outputs.  Narrowing:
              mi_reduce_bcast_scaled in fp32 into a scratch buffer, then m
              mi_convert calls.

  python tools/mixed_scaled_sweep.py [--points bf16-fp32-2x1-1g,...] [--trials 3] [--rounds 4]

Points: bf16 -> fp32 and fp32 -> bf16 at (k, m) = (2, 1), (8, 1), (8, 1) with
an accumulator in place (widening only: acc == outs[0]), (2, 2), (8, 8), at
1 GiB of the fp32 side per buffer and at 256 KiB.

Per point and trial, as tools/mixed_sweep.py: fresh allocations after a random
pad, seeded fills, every fused output checked bit for bit at the timed size
against the sequence's, a warm-up of every variant, then rounds that alternate
the variants (the order reversed every other round); each timing is a
device-event pair around a window of back-to-back launches that ends in a
synchronise.

One JSON line per point (the columns: profiles/reduce_mixed_scaled/README.md).
Measurement tool only (not product, not a test).  Needs a GPU: exits 2 without
one."""
from __future__ import annotations

import argparse
import json
import random
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FP32, BF16, SUM = 9, 11, 0
SIZES = {"1g": (1 << 30, 5), "256k": (256 << 10, 200)}  # bytes of an fp32 buffer, launches per timed window
SHAPES = (("2x1", 2, 1, False), ("8x1", 8, 1, False), ("8x1acc", 8, 1, True), ("2x2", 2, 2, False), ("8x8", 8, 8, False))
# name: (in dtype, out dtype, k, m, acc, elements, launches per timed window)
POINTS = {f"{dn}-{sn}-{zn}": (idt, odt, k, m, acc, nbytes // 4, launches)
          for zn, (nbytes, launches) in SIZES.items()
          for dn, idt, odt in (("bf16-fp32", BF16, FP32), ("fp32-bf16", FP32, BF16))
          for sn, k, m, acc in SHAPES if not (acc and odt != FP32)}
NAMES = ["fused", "unscaled_a", "unscaled_b", "seq"]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--points", default=",".join(POINTS))
    p.add_argument("--trials", type=int, default=3)
    p.add_argument("--rounds", type=int, default=4)
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("mixed_scaled_sweep: no GPU found (this tool never falls back to the CPU)", file=sys.stderr)
        return 2
    from oneccl_amd import _lib
    from oneccl_amd.comp import reference_flags
    mi = _lib.mi()
    rng = random.Random(37)
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    tdt = {FP32: torch.float32, BF16: torch.bfloat16}
    ptrs = lambda ts: _lib.void_ptr_array([t.data_ptr() for t in ts])  # noqa: E731

    for name in a.points.split(","):
        idt, odt, k, m, with_acc, n, launches = POINTS[name]
        widening = odt == FP32
        flags = reference_flags(BF16)  # the 16-bit side's: round to nearest even
        scale = 1.0 / k
        ms = {v: [] for v in NAMES}
        for trial in range(a.trials):
            torch.cuda.empty_cache()
            pad_mib = 2 * rng.randrange(0, 1536) if a.trials > 1 else 0
            pad = torch.empty(pad_mib << 18, dtype=torch.float32, device="cuda") if pad_mib else None
            ins = [torch.empty(n, dtype=tdt[idt], device="cuda") for _ in range(k)]
            outs = [torch.empty(n, dtype=tdt[odt], device="cuda") for _ in range(m)]
            seq_outs = [torch.empty(n, dtype=tdt[odt], device="cuda") for _ in range(m)]
            scratch = torch.empty(n, dtype=torch.float32, device="cuda")
            for j, t in enumerate(ins):
                g = torch.Generator(device="cuda")
                g.manual_seed(0xAB + j)
                t.uniform_(-1.0, 1.0, generator=g)
            pin, pout, pseq, pscr = ptrs(ins), ptrs(outs), ptrs(seq_outs), ptrs([scratch])
            pone = [ptrs([o]) for o in seq_outs]
            pacc_scr = ptrs([seq_outs[0], scratch])  # the sequence's fp32 fan-out reads {acc, scratch}

            def fill_acc():
                if with_acc:  # acc == outs[0], in place; the sequence's copy likewise
                    g = torch.Generator(device="cuda")
                    g.manual_seed(0xCD)
                    outs[0].uniform_(-1.0, 1.0, generator=g)
                    seq_outs[0].copy_(outs[0])

            def run_fused():
                _lib.check(mi.mi_reduce_bcast_mixed_scaled(pin, k, idt, outs[0].data_ptr() if with_acc else None, pout,
                                                           m, odt, n, SUM, flags, scale, sh),
                           "mi_reduce_bcast_mixed_scaled")

            def run_unscaled():
                _lib.check(mi.mi_reduce_bcast_mixed(pin, k, idt, outs[0].data_ptr() if with_acc else None, pout, m,
                                                    odt, n, SUM, flags, sh), "mi_reduce_bcast_mixed")

            def run_seq():
                if widening and not with_acc:
                    _lib.check(mi.mi_reduce_bcast_mixed(pin, k, idt, None, pseq, m, odt, n, SUM, flags, sh),
                               "mi_reduce_bcast_mixed")
                    for po in pone:
                        _lib.check(mi.mi_reduce_bcast_scaled(po, 1, po, 1, n, FP32, SUM, 0, scale, sh),
                                   "mi_reduce_bcast_scaled")
                elif widening:
                    _lib.check(mi.mi_reduce_bcast_mixed(pin, k, idt, None, pscr, 1, FP32, n, SUM, flags, sh),
                               "mi_reduce_bcast_mixed")
                    _lib.check(mi.mi_reduce_bcast_scaled(pscr, 1, pscr, 1, n, FP32, SUM, 0, scale, sh),
                               "mi_reduce_bcast_scaled")
                    _lib.check(mi.mi_reduce_bcast(pacc_scr, 2, pseq, m, n, FP32, SUM, 0, sh), "mi_reduce_bcast")
                else:
                    _lib.check(mi.mi_reduce_bcast_scaled(pin, k, pscr, 1, n, FP32, SUM, 0, scale, sh),
                               "mi_reduce_bcast_scaled")
                    for o in seq_outs:
                        _lib.check(mi.mi_convert(scratch.data_ptr(), FP32, o.data_ptr(), odt, n, flags, sh),
                                   "mi_convert")

            fns = {"fused": run_fused, "unscaled_a": run_unscaled, "unscaled_b": run_unscaled, "seq": run_seq}

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(launches):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / launches

            # the fused outputs against the sequence's, bit for bit, at the timed size
            for t in outs + seq_outs:
                t.zero_()
            fill_acc()
            run_fused()
            run_seq()
            torch.cuda.synchronize()
            it = torch.int32 if odt == FP32 else torch.int16
            for o in range(m):
                if not torch.equal(outs[o].view(it), seq_outs[o].view(it)):
                    print(f"mixed_scaled_sweep: {name}: output {o} differs from the sequence's", file=sys.stderr)
                    return 1
            fill_acc()
            for fn in fns.values():  # warm-up of every variant
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            per = {v: [] for v in NAMES}
            for r in range(a.rounds):
                order = list(NAMES)
                if r % 2:
                    order.reverse()
                for v in order:
                    fill_acc()  # an accumulator in place grows with every launch: start each window alike
                    per[v].append(timed(fns[v]))
            for v in NAMES:
                ms[v].append(statistics.mean(per[v]))
            del ins, outs, seq_outs, scratch, pad

        def spread(xs):
            return {"mean": round(statistics.mean(xs), 5), "min": round(min(xs), 5), "max": round(max(xs), 5)}

        def ratios(num, den):
            r = [x / y for x, y in zip(num, den)]
            return {"median": round(statistics.median(r), 4), "min": round(min(r), 4), "max": round(max(r), 4)}

        unscaled = [(x + y) / 2 for x, y in zip(ms["unscaled_a"], ms["unscaled_b"])]
        acc_b = 4 if with_acc else 0
        fused_bytes = (2 * k + 4 * m + acc_b) if widening else (4 * k + 2 * m)
        if not widening:
            seq_bytes, seq_disp = 4 * k + 4 + 6 * m, 1 + m
        elif with_acc:
            seq_bytes, seq_disp = 2 * k + 20 + 4 * m, 3
        else:
            seq_bytes, seq_disp = 2 * k + 12 * m, 1 + m
        fm = statistics.mean(ms["fused"])
        line = {
            "point": name, "in_dtype": "bf16" if idt == BF16 else "fp32", "out_dtype": "bf16" if odt == BF16 else "fp32",
            "k": k, "m": m, "acc_in_place": with_acc, "elements": n, "flags": flags, "scale": scale,
            "trials": a.trials, "rounds": a.rounds, "launches_per_window": launches,
            "ms": {v: spread(ms[v]) for v in NAMES},
            "unscaled_a_over_b_per_trial": ratios(ms["unscaled_a"], ms["unscaled_b"]),
            "fused_over_unscaled_per_trial": ratios(ms["fused"], unscaled),
            "fused_over_seq_per_trial": ratios(ms["fused"], ms["seq"]),
            "fused_bytes_per_element": fused_bytes, "sequence_bytes_per_element": seq_bytes,
            "bytes_ratio": round(fused_bytes / seq_bytes, 4),
            "fused_dispatches": 1, "sequence_dispatches": seq_disp,
            "fused_frac_of_8TBps": round(fused_bytes * n / (fm / 1e3) / 8e12, 4),
            "verified_bit_exact": True}
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
