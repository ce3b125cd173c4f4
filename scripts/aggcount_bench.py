"""Time per 1M-packet batch of the AggregateCounter post-pass (k_aggcount behind
k_rx, fcgpu_aggcount_configure) at three key shapes: one flow, 64k flows and
all-distinct flows; 60-B UDP/IPv4 frames in 64-B slots, checksum, FLOWID hash,
tile partition, 8 rotating device copies of the batch.

    python scripts/aggcount_bench.py [--steps 64] [--repeat 3] [--n 1048576] [--tag lds]

Per shape one JSON line: off_us = device time per fcgpu_process call with the
counter disabled, on_us = with it (events around `steps` calls: k_rx + post-pass
+ launch gaps; the table is warm, every key has its node), k_rx_us = k_rx alone
(every 8th launch, fcgpu_set_timing), agg_us = on_us - off_us, cold_us = the
first batch after fcgpu_aggcount_reset (every key is inserted). The rounds of
off and on alternate; *_all has every round. --tag names the library measured.

The naive variant (one global probe and atomic per packet, no LDS stage) is a
bench-only build: compile fcgpu_aggcount_api.hip with -DFCGPU_AGGCOUNT_NAIVE,
link it with the other units' objects into a second libfcgpu.so and run this
script with FCGPU_LIB=<that file> --tag naive. It is not a test."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402
from fastclick_amd import synth, _native as N  # noqa: E402
from fastclick_amd.device import DeviceBatch, DeviceOutputs  # noqa: E402

NPORTS = 16


def batch_for(n, flows, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(1 << 24, 2**32, flows, dtype=np.uint64)
    sport = rng.integers(0, 65536, flows)
    f = rng.integers(0, flows, n) if flows < n else np.arange(n)
    hdr = synth.build_headers(n, src=src[f], dst=synth.ip4(10, 0, 0, 2), sport=sport[f], dport=5678, frame_len=60, width=64)
    return synth.pack(hdr, 60)


def time_shape(name, b, steps, repeat, capacity, tag):
    n = b.n
    cfg = N.make_cfg(offset=14, checksum=True, hash_mode=N.HASH_FLOWID, classify=N.CLS_LB_HASH, nports=NPORTS)
    ctx = N.Context(0, n, cfg)
    db = DeviceBatch.upload(b, device="cuda:0")
    bufs = [(db.arena, db.desc)] + [(db.arena.clone(), db.desc.clone()) for _ in range(7)]
    outs = DeviceOutputs(n, NPORTS, device="cuda:0", tile_perm=True, partition=N.PART_TILE)
    s = torch.cuda.current_stream().cuda_stream

    def rounds(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for j in range(k):
            a, d = bufs[j % len(bufs)]
            ctx.process(a.data_ptr(), d.data_ptr(), n, stream=s, **outs.ptrs())
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / k

    off, on, krx, cold = [], [], [], []
    for rep in range(repeat + 1):                      # the first round warms up
        ctx.aggcount_configure(0)
        ctx.set_timing(8)
        t_off = rounds(steps)
        ms, cnt = ctx.read_timing()
        ctx.aggcount_configure(capacity)
        t_cold = rounds(1)
        t_on = rounds(steps)
        ctx.read_timing()                              # drop the on rounds' samples
        if rep:
            off.append(t_off)
            on.append(t_on)
            cold.append(t_cold)
            krx.append(1e3 * ms[0] / max(cnt[0], 1))
    st = ctx.aggcount_stats()
    ctx.close()
    med = statistics.median
    print(json.dumps(dict(row=name, tag=tag, packets=n, steps=steps, off_us=round(med(off), 2), on_us=round(med(on), 2),
                          agg_us=round(med(on) - med(off), 2), k_rx_us=round(med(krx), 2), cold_us=round(med(cold), 2),
                          off_all=[round(x, 2) for x in off], on_all=[round(x, 2) for x in on],
                          cold_all=[round(x, 2) for x in cold], nagg=st["nagg"], seen=st["seen"],
                          uncounted=st["uncounted"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--tag", default="lds")
    args = ap.parse_args()
    for name, flows in (("one-flow", 1), ("64k-flows", 1 << 16), ("distinct", args.n)):
        time_shape(name, batch_for(args.n, min(flows, args.n), seed=flows & 0xffff), args.steps, args.repeat,
                   min(2 * args.n, N.AGGCOUNT_MAX_CAPACITY), args.tag)


if __name__ == "__main__":
    main()
