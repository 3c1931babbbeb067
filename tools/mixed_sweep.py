#!/usr/bin/env python3
"""mi_reduce_bcast_mixed against the sequence it replaces, in one process on
the same buffers:

  fused     one mi_reduce_bcast_mixed of k inputs (and acc) into m outputs
  sequence  built only from calls that exist without it.  Widening: k
            mi_convert calls into k fp32 scratch buffers, then an fp32
            mi_reduce_bcast of (acc and) the scratch buffers into the m
            outputs.  Narrowing: mi_reduce_multi into an fp32 scratch buffer,
            then m mi_convert calls.  Timed in two slots of every round (A and
            B): A over B is the spread of the sequence against itself, the
            margin a difference has to exceed.

  python tools/mixed_sweep.py [--points bf16-fp32-2x1-1g,...] [--trials 3] [--rounds 4] [--residency 0,9,16]

Points: bf16 -> fp32 and fp32 -> bf16 at (k, m) = (2, 1), (8, 1), (8, 1) with
an accumulator in place (widening only: acc == outs[0]), (2, 2), (8, 8), at
1 GiB of the fp32 side per buffer and at 256 KiB.

Per point and trial: fresh allocations after a random pad (a placement per
trial, as tools/scaled_sweep.py), seeded fills, the fused outputs checked bit
for bit at the timed size against the sequence's own outputs, a warm-up of
every variant, then rounds that alternate the variants (the order reversed
every other round); each timing is a device-event pair around a window of
back-to-back launches that ends in a synchronise.  --residency adds fused
variants under mi_set_residency of the launch's streams, min(k + acc + m - 1,
16) (waves per CU; 0 = the library's plan, always measured as `fused`); the
override is taken back after each such launch.

One JSON line per point: each variant's time (mean over trials of the
per-trial means, with the spread over trials), the per-trial ratios sequence A
/ sequence B and fused / sequence, and the bytes per element and dispatches of
the fused call and of the sequence.  Measurement tool only (not product, not
a test).  Needs a GPU: exits 2 without one."""
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--points", default=",".join(POINTS))
    p.add_argument("--trials", type=int, default=3)
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--residency", default="0", help="comma list of waves per CU for the fused call; 0 = the plan")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("mixed_sweep: no GPU found (this tool never falls back to the CPU)", file=sys.stderr)
        return 2
    from oneccl_amd import _lib
    from oneccl_amd.comp import reference_flags
    mi = _lib.mi()
    rng = random.Random(31)
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    waves = [w for w in dict.fromkeys(int(x) for x in a.residency.split(",")) if w]  # 0, the plan, is `fused`
    names = ["fused", "seq_a", "seq_b"] + [f"fused_w{w}" for w in waves]
    tdt = {FP32: torch.float32, BF16: torch.bfloat16}
    ptrs = lambda ts: _lib.void_ptr_array([t.data_ptr() for t in ts])  # noqa: E731

    for name in a.points.split(","):
        idt, odt, k, m, with_acc, n, launches = POINTS[name]
        widening = odt == FP32
        flags = reference_flags(BF16)  # the 16-bit side's: round to nearest even
        key = min(k + (1 if with_acc else 0) + m - 1, 16)
        ms = {v: [] for v in names}
        for trial in range(a.trials):
            torch.cuda.empty_cache()
            pad_mib = 2 * rng.randrange(0, 1536) if a.trials > 1 else 0
            pad = torch.empty(pad_mib << 18, dtype=torch.float32, device="cuda") if pad_mib else None
            ins = [torch.empty(n, dtype=tdt[idt], device="cuda") for _ in range(k)]
            outs = [torch.empty(n, dtype=tdt[odt], device="cuda") for _ in range(m)]
            seq_outs = [torch.empty(n, dtype=tdt[odt], device="cuda") for _ in range(m)]
            scratch = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(k if widening else 1)]
            for j, t in enumerate(ins):
                g = torch.Generator(device="cuda")
                g.manual_seed(0xAB + j)
                t.uniform_(-1.0, 1.0, generator=g)
            pin, pout, pseq = ptrs(ins), ptrs(outs), ptrs(seq_outs)

            lst = ([seq_outs[0]] if with_acc else []) + scratch  # the sequence's fp32 fan-out reads these
            plst, nlst = ptrs(lst), len(lst)

            def fill_acc():
                if with_acc:  # acc == outs[0], in place; the sequence's copy likewise
                    g = torch.Generator(device="cuda")
                    g.manual_seed(0xCD)
                    outs[0].uniform_(-1.0, 1.0, generator=g)
                    seq_outs[0].copy_(outs[0])

            def run_fused():
                _lib.check(mi.mi_reduce_bcast_mixed(pin, k, idt, outs[0].data_ptr() if with_acc else None, pout, m,
                                                    odt, n, SUM, flags, sh), "mi_reduce_bcast_mixed")

            def run_fused_at(w):  # two more host calls per launch: compare these variants with each other
                mi.mi_set_residency(key, w)
                try:
                    run_fused()
                finally:
                    mi.mi_set_residency(key, 0)

            def run_seq():
                if widening:
                    for x, c in zip(ins, scratch):
                        _lib.check(mi.mi_convert(x.data_ptr(), idt, c.data_ptr(), FP32, n, 0, sh), "mi_convert")
                    _lib.check(mi.mi_reduce_bcast(plst, nlst, pseq, m, n, FP32, SUM, 0, sh),
                               "mi_reduce_bcast")
                else:
                    _lib.check(mi.mi_reduce_multi(pin, k, scratch[0].data_ptr(), n, FP32, SUM, 0, sh), "mi_reduce_multi")
                    for o in seq_outs:
                        _lib.check(mi.mi_convert(scratch[0].data_ptr(), FP32, o.data_ptr(), odt, n, flags, sh),
                                   "mi_convert")

            fns = {"fused": run_fused, "seq_a": run_seq, "seq_b": run_seq}
            fns.update({f"fused_w{w}": (lambda w=w: run_fused_at(w)) for w in waves})

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
                    print(f"mixed_sweep: {name}: output {o} differs from the sequence's", file=sys.stderr)
                    return 1
            fill_acc()
            for fn in fns.values():  # warm-up of every variant
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            per = {v: [] for v in names}
            for r in range(a.rounds):
                order = list(names)
                if r % 2:
                    order.reverse()
                for v in order:
                    fill_acc()  # an accumulator in place grows with every launch: start each window alike
                    per[v].append(timed(fns[v]))
            for v in names:
                ms[v].append(statistics.mean(per[v]))
            del ins, outs, seq_outs, scratch, pad

        def spread(xs):
            return {"mean": round(statistics.mean(xs), 5), "min": round(min(xs), 5), "max": round(max(xs), 5)}

        def ratios(num, den):
            r = [x / y for x, y in zip(num, den)]
            return {"median": round(statistics.median(r), 4), "min": round(min(r), 4), "max": round(max(r), 4)}

        seq = [(x + y) / 2 for x, y in zip(ms["seq_a"], ms["seq_b"])]
        acc_b = 4 if with_acc else 0
        fused_bytes = (2 * k + 4 * m + acc_b) if widening else (4 * k + 2 * m)
        seq_bytes = (10 * k + 4 * m + acc_b) if widening else (4 * k + 4 + 6 * m)
        fm = statistics.mean(ms["fused"])
        line = {
            "point": name, "in_dtype": "bf16" if idt == BF16 else "fp32", "out_dtype": "bf16" if odt == BF16 else "fp32",
            "k": k, "m": m, "acc_in_place": with_acc, "elements": n, "flags": flags, "trials": a.trials,
            "rounds": a.rounds, "launches_per_window": launches,
            "ms": {v: spread(ms[v]) for v in names},
            "seq_a_over_b_per_trial": ratios(ms["seq_a"], ms["seq_b"]),
            "fused_over_seq_per_trial": ratios(ms["fused"], seq),
            "fused_bytes_per_element": fused_bytes, "sequence_bytes_per_element": seq_bytes,
            "bytes_ratio": round(fused_bytes / seq_bytes, 4),
            "fused_dispatches": 1, "sequence_dispatches": (k + 1) if widening else (1 + m),
            "fused_frac_of_8TBps": round(fused_bytes * n / (fm / 1e3) / 8e12, 4),
            "verified_bit_exact": True}
        for w in waves:
            line[f"fused_w{w}_over_fused_per_trial"] = ratios(ms[f"fused_w{w}"], ms["fused"])
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
