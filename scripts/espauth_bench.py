"""Time per batch of the ESP authentication post-pass (k_espauth behind k_rx,
fcgpu_espauth_set_sas) on ESP/IPv4 frames with a seeded random payload and a
right digest: 1,048,576 x 64-B frames (two compressions per packet), 43,690 x
1500-B frames (24 + 1) and a C3-style IMIX (64/570/1500 B at 7:4:1), four SAs,
checksum, FLOWID hash, tile partition, 8 rotating device copies.

    python scripts/espauth_bench.py [--steps 64] [--repeat 3] [--n 1048576]

Per row one JSON line: step_us = device time per fcgpu_process call (events
around `steps` calls), k_rx_us = k_rx alone (every 8th launch,
fcgpu_set_timing). Rows per batch: `off` (no SAs), `on` (tiles ordered by block
count) and `arrival` (FCGPU_ESPAUTH_ORDER=0); for the last two post_us = step -
k_rx, mcomp_s = millions of SHA-1 compressions per second of it, auth_gbps =
authenticated bytes per second of it. For scale `l4udp`: the UDP checksum,
which reads the same bytes, on the same frames marked UDP."""
import argparse
import hashlib
import hmac
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
SAS = [(0x2000 + k, bytes((11 * k + j) & 0xFF for j in range(16))) for k in range(4)]


def batch_for(flen, seed, proto=50):
    """Frames of the given lengths: SPI, random payload; a right digest in the
    first 2048 (the status mix of the rest does not change the work)."""
    n = len(flen)
    rng = np.random.default_rng(seed)
    hdr = synth.build_headers(n, src=rng.integers(1 << 24, 2**32, n, dtype=np.uint64), dst=synth.ip4(10, 0, 0, 2),
                              sport=rng.integers(0, 65536, n), dport=53, proto=proto, frame_len=flen, width=64)
    b = synth.pack(hdr, flen)
    body = rng.integers(0, 256, b.arena.size, dtype=np.uint8)
    spi = synth._be32(np.asarray([s for s, _ in SAS])[np.arange(n) % 4])
    for L in np.unique(flen):
        sel = np.nonzero(flen == L)[0]
        idx = b.desc[sel, 0].astype(np.int64)[:, None] + np.arange(34, L)[None, :]
        b.arena[idx] = body[idx]
        b.arena[idx[:, :4]] = spi[sel]
    for i in range(min(n, 2048)):
        o, L = int(b.desc[i, 0]), int(flen[i])
        b.arena[o + L - 12:o + L] = np.frombuffer(
            hmac.new(SAS[i % 4][1], bytes(b.arena[o + 34:o + L - 12]), hashlib.sha1).digest()[:12], np.uint8)
    return synth.set_udp_checksums(b) if proto == 17 else b


def time_row(name, b, steps, repeat, sas=None, l4=False):
    n = b.n
    cfg = N.make_cfg(offset=14, checksum=True, hash_mode=N.HASH_FLOWID, nports=NPORTS)
    if l4:
        cfg.l4_mode, cfg.l4_checksum = N.L4_UDP, 1
    ctx = N.Context(0, n, cfg)
    if sas:
        ctx.espauth_set_sas(sas)
    db = DeviceBatch.upload(b, device="cuda:0")
    bufs = [(db.arena, db.desc)] + [(db.arena.clone(), db.desc.clone()) for _ in range(7)]
    outs = DeviceOutputs(n, NPORTS, device="cuda:0", anno=True, tile_perm=True, partition=N.PART_TILE)
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
    row = dict(row=name, packets=n, steps=steps, step_us=round(statistics.median(step), 2),
               k_rx_us=round(statistics.median(krx), 2), step_us_all=[round(x, 2) for x in step],
               valid=int((outs.numpy()["reason"] == N.R_OK).sum()))
    if sas:
        st = ctx.espauth_stats()
        rec = ctx.espauth_records(min(n, 2048))
        L = b.desc[:, 1].astype(np.int64) - 34 - 12          # authenticated bytes per packet
        post = row["step_us"] - row["k_rx_us"]
        row.update(post_us=round(post, 2), mcomp_s=round(float(((L + 9 + 63) // 64 + 1).sum()) / post, 1),
                   auth_gbps=round(float(L.sum()) / post / 1e3, 2), first_ok=int((rec["status"] == N.ESP_OK).sum()),
                   considered=int(st["ok"] + st["bad"]) // ((repeat + 1) * steps))
    ctx.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 20)
    args = ap.parse_args()
    rng = np.random.default_rng(3)
    shapes = {"64": np.full(args.n, 64), "1500": np.full(max(args.n * 64 // 1536, 1), 1500),
              "imix": (synth.IMIX_LEN + 4)[rng.choice(3, args.n // 4, p=synth.IMIX_W)]}
    for name, flen in shapes.items():
        b = batch_for(flen, seed=len(name))
        time_row(f"off/{name}", b, args.steps, args.repeat)
        for tag, order in (("on", "1"), ("arrival", "0")):
            os.environ["FCGPU_ESPAUTH_ORDER"] = order
            time_row(f"{tag}/{name}", b, args.steps, args.repeat, sas=SAS)
        time_row(f"l4udp/{name}", batch_for(flen, seed=len(name), proto=17), args.steps, args.repeat, l4=True)


if __name__ == "__main__":
    main()
