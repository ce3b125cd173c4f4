"""Time per batch of FCGPU_CLS_STRING (the k_acmatch pre-pass + k_rx) beside
CLS_NONE and the L4-checksum configuration (the other whole-payload reader) on
the same batches: UDP/IPv4 frames with a seeded random payload, 64-B frames in
a 1M-packet batch and 1500-B frames in a batch of the same arena size,
checksum, FLOWID hash, tile partition, 8 rotating device copies.

    python scripts/strmatch_bench.py [--steps 80] [--repeat 3] [--only none|l4|string]

Per row one JSON line: step_us = device time per fcgpu_process call (events
around `steps` calls: pre-pass + k_rx + launch gaps), k_rx_us = k_rx alone
(every 8th launch, fcgpu_set_timing); for CLS_STRING their difference is the
pre-pass, and text_gbps = frame bytes scanned per second of it. Pattern sets:
`lds` (24 words of 4..12 letters: transitions in LDS) and `global` (40 random
200-byte strings: a 2.5-MB image read from global memory); the payload bytes are
drawn from the patterns' alphabet, so the automaton leaves the root. The
package is taken from the current directory: --only none / l4 run from a
checkout of another commit too."""
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

NPORTS = 64


def pattern_sets():
    rng = np.random.default_rng(9)
    words = [bytes(rng.integers(0x61, 0x71, int(rng.integers(4, 13)), dtype=np.uint8)) for _ in range(24)]
    big = [bytes(rng.integers(0x61, 0x100, 200, dtype=np.uint8)) for _ in range(40)]
    return {"lds": list(dict.fromkeys(words)), "global": big}


def batch_for(n, frame_len, seed):
    rng = np.random.default_rng(seed)
    hdr = synth.build_headers(n, src=rng.integers(1 << 24, 2**32, n, dtype=np.uint64), dst=synth.ip4(10, 0, 0, 2),
                              sport=rng.integers(0, 65536, n), dport=53, frame_len=frame_len, width=64)
    b = synth.pack(hdr, frame_len)
    slot = int(b.desc[1, 0] - b.desc[0, 0])
    rows = b.arena[:n * slot].reshape(n, slot)
    rows[:, 42:frame_len] = rng.integers(0x61, 0x80, (n, frame_len - 42), dtype=np.uint8)
    return synth.set_udp_checksums(b)


def time_row(name, b, steps, repeat, classify=N.CLS_NONE, patterns=None, l4=False):
    n = b.n
    cfg = N.make_cfg(offset=14, checksum=True, hash_mode=N.HASH_FLOWID, classify=classify, nports=NPORTS)
    if l4:
        cfg.l4_mode, cfg.l4_checksum = N.L4_UDP, 1
    ctx = N.Context(0, n, cfg)
    if patterns is not None:
        ctx.set_patterns(patterns)
    db = DeviceBatch.upload(b, device="cuda:0")
    bufs = [(db.arena, db.desc)] + [(db.arena.clone(), db.desc.clone()) for _ in range(7)]
    outs = DeviceOutputs(n, NPORTS, device="cuda:0", tile_perm=True, partition=N.PART_TILE)
    s = torch.cuda.current_stream().cuda_stream
    krx, step = [], []
    for rep in range(repeat + 1):                      # the first round warms up
        ctx.set_timing(8)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(steps):
            a, d = bufs[k % len(bufs)]
            ctx.process(a.data_ptr(), d.data_ptr(), n, stream=s, **outs.ptrs())
        e1.record()
        torch.cuda.synchronize()
        ms, cnt = ctx.read_timing()
        if rep:
            krx.append(1e3 * ms[0] / max(cnt[0], 1))
            step.append(1e3 * e0.elapsed_time(e1) / steps)
    v = outs.numpy()
    ctx.close()
    row = dict(row=name, packets=n, frame=int(b.desc[0, 1]), steps=steps, step_us=round(statistics.median(step), 2),
               k_rx_us=round(statistics.median(krx), 2), step_us_all=[round(x, 2) for x in step],
               valid=int((v["reason"] == N.R_OK).sum()), matched=int(((v["reason"] == N.R_OK) & (v["port"] < len(patterns or ()))).sum()))
    if patterns is not None:
        pre = row["step_us"] - row["k_rx_us"]
        row.update(prepass_us=round(pre, 2), text_gbps=round(float(b.desc[:, 1].sum()) / pre / 1e3, 1),
                   stats=N.patterns_stats(patterns))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--only", choices=["none", "l4", "string"], default=None)
    args = ap.parse_args()
    sets = pattern_sets()
    for frame_len in (64, 1500):
        n = args.n if frame_len == 64 else max(args.n * 64 // 1536, 1)      # the same arena
        b = batch_for(n, frame_len, seed=frame_len)
        if args.only in (None, "none"):
            time_row(f"none/{frame_len}", b, args.steps, args.repeat)
        if args.only in (None, "l4"):
            time_row(f"l4udp/{frame_len}", b, args.steps, args.repeat, l4=True)
        for sname, pats in sets.items():
            if args.only in (None, "string"):
                time_row(f"string-{sname}/{frame_len}", b, args.steps, args.repeat, classify=N.CLS_STRING, patterns=pats)


if __name__ == "__main__":
    main()
