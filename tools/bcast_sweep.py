#!/usr/bin/env python3
"""mi_reduce_bcast against the sequence it replaces, in one process on the
same buffers: (a) one mi_reduce_bcast of k inputs into m outputs; (b)
mi_reduce_multi into outs[0], then m - 1 mi_copy calls from it.

  python tools/bcast_sweep.py [--points fp32-2x2-1g,...] [--trials 4] [--rounds 6]
                              [--store nt,sc1nt] [--residency 0,5,8,...]

Per point and trial: fresh allocations after a random pad (a placement per
trial, as tools/ab_c2.py --trials), seeded fills, (a) checked against (b) bit
for bit at the timed size, a warm-up of every variant, then rounds that
alternate the variants; each timing is a device-event pair around a window of
back-to-back launches that ends in a synchronise.  --store and --residency
add fused variants: the store policy (mi_set_bcast_store) and the waves per CU
(mi_set_residency of the launch's min(k + m - 1, 16) streams; 0 = the
library's plan).

One JSON line per point and fused variant: both times (mean over trials of
the per-trial means) and their spread over trials, the per-trial time ratio
fused / sequence, the algorithmic bytes of each ((k + m) n against
(k + 2m - 1) n) and the fused rate as a fraction of the 8 TB/s spec.
Measurement tool only (not product, not a test).  Needs a GPU: exits 2
without one."""
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
# name: (dtype, element size, k, m, bytes per buffer, launches per timed window)
POINTS = {
    "fp32-2x2-1g": (FP32, 4, 2, 2, 1024 * MIB, 10),
    "fp32-8x8-256m": (FP32, 4, 8, 8, 256 * MIB, 10),
    "fp32-4x4-256m": (FP32, 4, 4, 4, 256 * MIB, 10),
    "bf16-8x8-256m": (BF16, 2, 8, 8, 256 * MIB, 10),
    "fp32-8x8-256k": (FP32, 4, 8, 8, 256 << 10, 200),
}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--points", default=",".join(POINTS))
    p.add_argument("--trials", type=int, default=4)
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--store", default="", help="comma list of nt / sc1nt; empty = the library's default")
    p.add_argument("--residency", default="0", help="comma list of waves per CU; 0 = the library's plan")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bcast_sweep: no GPU found (this tool never falls back to the CPU)", file=sys.stderr)
        return 2
    from oneccl_amd import _lib
    from oneccl_amd.comp import reference_flags
    mi = _lib.mi()
    default_store = mi.mi_set_bcast_store(0)
    mi.mi_set_bcast_store(default_store)
    stores = [{"nt": 0, "sc1nt": 1}[s] for s in a.store.split(",") if s] or [default_store]
    waves = [int(w) for w in a.residency.split(",")]
    variants = [(s, w) for s in stores for w in waves]
    rng = random.Random(17)
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream

    for name in a.points.split(","):
        dt, es, k, m, nbytes, launches = POINTS[name]
        n = nbytes // es
        flags = reference_flags(dt)
        tdt = torch.float32 if dt == FP32 else torch.bfloat16
        key = min(k + m - 1, 16)
        seq_ms, fused_ms = [], {v: [] for v in variants}
        for trial in range(a.trials):
            torch.cuda.empty_cache()
            pad_mib = 2 * rng.randrange(0, 1536) if a.trials > 1 else 0
            pad = torch.empty(pad_mib << 18, dtype=torch.float32, device="cuda") if pad_mib else None
            ins = [torch.empty(n, dtype=tdt, device="cuda") for _ in range(k)]
            fused = [torch.empty(n, dtype=tdt, device="cuda") for _ in range(m)]
            seq = [torch.empty(n, dtype=tdt, device="cuda") for _ in range(m)]
            for j, t in enumerate(ins):
                g = torch.Generator(device="cuda")
                g.manual_seed(0xAB + j)
                t.uniform_(-1.0, 1.0, generator=g)
            pin = _lib.void_ptr_array([t.data_ptr() for t in ins])
            pfused = _lib.void_ptr_array([t.data_ptr() for t in fused])

            def run_fused(v):
                mi.mi_set_bcast_store(v[0])
                mi.mi_set_residency(key, v[1])
                _lib.check(mi.mi_reduce_bcast(pin, k, pfused, m, n, dt, SUM, flags, sh), "mi_reduce_bcast")

            def run_seq(_=None):
                _lib.check(mi.mi_reduce_multi(pin, k, seq[0].data_ptr(), n, dt, SUM, flags, sh), "mi_reduce_multi")
                for t in seq[1:]:
                    _lib.check(mi.mi_copy(seq[0].data_ptr(), t.data_ptr(), nbytes, 1, sh), "mi_copy")

            def timed(fn, v):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(launches):
                    fn(v)
                e1.record(stream)
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / launches

            try:
                # (a) == (b), bit for bit, at the timed size, for every variant; this is the warm-up too
                run_seq()
                for v in variants:
                    for t in fused:
                        t.zero_()
                    for _ in range(3):
                        run_fused(v)
                    torch.cuda.synchronize()
                    for o in range(m):
                        if not torch.equal(fused[o].view(torch.int16), seq[o].view(torch.int16)):
                            print(f"bcast_sweep: {name} variant {v}: output {o} differs from the sequence's",
                                  file=sys.stderr)
                            return 1
                for _ in range(2):
                    run_seq()
                torch.cuda.synchronize()
                per = {v: [] for v in variants}
                per_seq = []
                for r in range(a.rounds):
                    order = [("seq", None)] + [("fused", v) for v in variants]
                    if r % 2:
                        order.reverse()
                    for what, v in order:
                        if what == "seq":
                            per_seq.append(timed(run_seq, None))
                        else:
                            per[v].append(timed(run_fused, v))
            finally:
                mi.mi_set_bcast_store(default_store)
                mi.mi_set_residency(key, 0)
            seq_ms.append(statistics.mean(per_seq))
            for v in variants:
                fused_ms[v].append(statistics.mean(per[v]))
            del ins, fused, seq, pad

        def spread(xs):
            return {"mean": round(statistics.mean(xs), 5), "min": round(min(xs), 5), "max": round(max(xs), 5)}

        for v in variants:
            ratios = [f / s for f, s in zip(fused_ms[v], seq_ms)]
            fm = statistics.mean(fused_ms[v])
            print(json.dumps({
                "point": name, "dtype": "fp32" if dt == FP32 else "bf16", "k": k, "m": m, "bytes_per_buffer": nbytes,
                "store": "sc1nt" if v[0] else "nt", "waves_per_cu": v[1] or "plan", "trials": a.trials,
                "rounds": a.rounds, "launches_per_window": launches,
                "fused_ms": spread(fused_ms[v]), "sequence_ms": spread(seq_ms),
                "fused_over_sequence_per_trial": {"median": round(statistics.median(ratios), 4),
                                                  "min": round(min(ratios), 4), "max": round(max(ratios), 4)},
                "fused_algorithmic_bytes": (k + m) * nbytes, "sequence_algorithmic_bytes": (k + 2 * m - 1) * nbytes,
                "bytes_ratio": round((k + m) / (k + 2 * m - 1), 4),
                "fused_frac_of_8TBps": round((k + m) * nbytes / (fm / 1e3) / 8e12, 4),
                "verified_bit_exact": True}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
