#!/usr/bin/env python3
"""mi_reduce_bcast_scaled against the unscaled call and against the sequence
it replaces, in one process on the same buffers:

  fused     one mi_reduce_bcast_scaled of k inputs into m outputs, scale 1 / k
  unscaled  (a) mi_reduce_bcast of the same (k, m), timed in two slots of every
            round (A and B): A over B is the spread of that call against
            itself, the margin the fused call is held to
  sequence  (b) mi_reduce_bcast, then one in-place scaling pass per output, as
            a caller without the fused entry does it: `torch` = Tensor.mul_
            on the same stream, `lib` = the library's own k = m = 1 in-place
            scaled call

  python tools/scaled_sweep.py [--points fp32-2x1-1g,...] [--trials 3] [--rounds 4] [--residency 0,16,21]

Per point and trial: fresh allocations after a random pad (a placement per
trial, as tools/bcast_sweep.py), seeded fills, the fused outputs checked bit
for bit at the timed size against the same fold and multiply done with torch
ops, a warm-up of every variant, then rounds that alternate the variants (the
order reversed every other round); each timing is a device-event pair around
a window of back-to-back launches that ends in a synchronise.  --residency
adds fused variants under mi_set_residency of the launch's min(k + m - 1, 16)
streams (waves per CU; 0 = the library's plan, always measured as `fused`);
the override is taken back after each such launch, since for two streams it is
the 2-input kernel's too.

One JSON line per point: each variant's time (mean over trials of the
per-trial means, with the spread over trials), the per-trial ratios unscaled A
/ unscaled B, fused / unscaled and fused / sequence, and the buffer-sized
streams and dispatches of the fused call and of the sequence (k + m and 1
against k + 3m and 1 + m).  Measurement tool only (not product, not a test).
Needs a GPU: exits 2 without one."""
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
MIB = 1 << 20
SIZES = {"1g": (1024 * MIB, 10), "256k": (256 << 10, 200)}  # bytes per buffer, launches per timed window
# name: (dtype, element size, k, m, bytes per buffer, launches per timed window)
POINTS = {f"{dn}-{k}x{m}-{sn}": (dt, es, k, m, nbytes, launches)
          for sn, (nbytes, launches) in SIZES.items()
          for dn, dt, es in (("fp32", FP32, 4), ("bf16", BF16, 2))
          for k, m in ((2, 1), (8, 1), (2, 2), (8, 8))}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--points", default=",".join(POINTS))
    p.add_argument("--trials", type=int, default=3)
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--residency", default="0", help="comma list of waves per CU for the fused call; 0 = the plan")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("scaled_sweep: no GPU found (this tool never falls back to the CPU)", file=sys.stderr)
        return 2
    from oneccl_amd import _lib
    from oneccl_amd.comp import reference_flags
    mi = _lib.mi()
    rng = random.Random(29)
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    waves = [w for w in dict.fromkeys(int(x) for x in a.residency.split(",")) if w]  # 0, the plan, is `fused`
    names = ["fused", "unscaled_a", "unscaled_b", "seq_torch", "seq_lib"] + [f"fused_w{w}" for w in waves]

    for name in a.points.split(","):
        dt, es, k, m, nbytes, launches = POINTS[name]
        n = nbytes // es
        flags = reference_flags(dt)
        tdt = torch.float32 if dt == FP32 else torch.bfloat16
        scale = 1.0 / k
        key = min(k + m - 1, 16)
        ms = {v: [] for v in names}
        for trial in range(a.trials):
            torch.cuda.empty_cache()
            pad_mib = 2 * rng.randrange(0, 1536) if a.trials > 1 else 0
            pad = torch.empty(pad_mib << 18, dtype=torch.float32, device="cuda") if pad_mib else None
            ins = [torch.empty(n, dtype=tdt, device="cuda") for _ in range(k)]
            outs = [torch.empty(n, dtype=tdt, device="cuda") for _ in range(m)]
            for j, t in enumerate(ins):
                g = torch.Generator(device="cuda")
                g.manual_seed(0xAB + j)
                t.uniform_(-1.0, 1.0, generator=g)
            pin = _lib.void_ptr_array([t.data_ptr() for t in ins])
            pout = _lib.void_ptr_array([t.data_ptr() for t in outs])
            pone = [_lib.void_ptr_array([t.data_ptr()]) for t in outs]

            def run_fused():
                _lib.check(mi.mi_reduce_bcast_scaled(pin, k, pout, m, n, dt, SUM, flags, scale, sh),
                           "mi_reduce_bcast_scaled")

            def run_fused_at(w):  # two more host calls per launch: compare these variants with each other
                mi.mi_set_residency(key, w)
                try:
                    run_fused()
                finally:
                    mi.mi_set_residency(key, 0)

            def run_unscaled():
                _lib.check(mi.mi_reduce_bcast(pin, k, pout, m, n, dt, SUM, flags, sh), "mi_reduce_bcast")

            def run_seq_torch():
                run_unscaled()
                for t in outs:
                    t.mul_(scale)

            def run_seq_lib():
                run_unscaled()
                for q in pone:
                    _lib.check(mi.mi_reduce_bcast_scaled(q, 1, q, 1, n, dt, SUM, flags, scale, sh), "scaling pass")

            fns = {"fused": run_fused, "unscaled_a": run_unscaled, "unscaled_b": run_unscaled,
                   "seq_torch": run_seq_torch, "seq_lib": run_seq_lib}
            fns.update({f"fused_w{w}": (lambda w=w: run_fused_at(w)) for w in waves})

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(launches):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / launches

            # the fused outputs against the same left fold and one multiply in torch ops (fp32: plain IEEE adds;
            # bf16 under the reference's flags: every step rounded to bf16, nearest even), bit for bit
            for t in outs:
                t.zero_()
            run_fused()
            torch.cuda.synchronize()
            acc = ins[0].clone()
            for t in ins[1:]:
                acc = (acc.float() + t.float()).to(tdt)
            exp = (acc.float() * torch.tensor(scale, dtype=torch.float32, device="cuda")).to(tdt)
            del acc
            it = torch.int32 if es == 4 else torch.int16
            for o in range(m):
                if not torch.equal(outs[o].view(it), exp.view(it)):
                    print(f"scaled_sweep: {name}: output {o} differs from the torch fold and multiply", file=sys.stderr)
                    return 1
            del exp
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
                    per[v].append(timed(fns[v]))
            for v in names:
                ms[v].append(statistics.mean(per[v]))
            del ins, outs, pad

        def spread(xs):
            return {"mean": round(statistics.mean(xs), 5), "min": round(min(xs), 5), "max": round(max(xs), 5)}

        def ratios(num, den):
            r = [x / y for x, y in zip(num, den)]
            return {"median": round(statistics.median(r), 4), "min": round(min(r), 4), "max": round(max(r), 4)}

        unscaled = [(x + y) / 2 for x, y in zip(ms["unscaled_a"], ms["unscaled_b"])]
        fm = statistics.mean(ms["fused"])
        print(json.dumps({
            "point": name, "dtype": "fp32" if dt == FP32 else "bf16", "k": k, "m": m, "bytes_per_buffer": nbytes,
            "scale": scale, "trials": a.trials, "rounds": a.rounds, "launches_per_window": launches,
            "ms": {v: spread(ms[v]) for v in names},
            "unscaled_a_over_b_per_trial": ratios(ms["unscaled_a"], ms["unscaled_b"]),
            "fused_over_unscaled_per_trial": ratios(ms["fused"], unscaled),
            "fused_over_seq_torch_per_trial": ratios(ms["fused"], ms["seq_torch"]),
            "fused_over_seq_lib_per_trial": ratios(ms["fused"], ms["seq_lib"]),
            "fused_streams": k + m, "sequence_streams": k + 3 * m, "fused_dispatches": 1,
            "sequence_dispatches": 1 + m, "streams_ratio": round((k + m) / (k + 3 * m), 4),
            "fused_frac_of_8TBps": round((k + m) * nbytes / (fm / 1e3) / 8e12, 4),
            "verified_bit_exact": True}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
