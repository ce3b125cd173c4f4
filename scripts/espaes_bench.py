"""Time per batch of the ESP decryption post-pass (k_espaes behind k_rx,
fcgpu_espaes_set_sas) on ESP/IPv4 frames with a seeded random payload:
1,048,576 x 64-B frames (elen 28: no block, the per-packet cost), 43,690 x
1500-B frames (90 blocks each) and a C3-style IMIX (64/570/1500 B at 7:4:1; 0,
32 and 90 blocks), four SAs, checksum, FLOWID hash, tile partition, 8 rotating
device copies. Every frame's IP length is cut so that plen % 8 == 0.

    python scripts/espaes_bench.py [--steps 64] [--repeat 3] [--n 1048576] [--ab] [--mode decrypt|encrypt]

Per row one JSON line: step_us = device time per fcgpu_process call (events
around `steps` calls, median of `repeat` rounds), k_rx_us = k_rx alone (every
8th launch, fcgpu_set_timing). Rows per batch: `off` (no SAs), `aes` (this
stage), `auth` (k_espauth alone, the yardstick of the same session) and
`both`; post_us = step - k_rx, mblk_s = millions of 16-byte blocks per second
of it, gbps = decrypted bytes per second of it. --ab adds, for the 1500-B
batch, one row per table layout: t<tables>r<replicas> (FCGPU_ESPAES_TABLES,
FCGPU_ESPAES_REPLICAS). The stage decrypts the rotating copies in place again
and again: the work does not depend on the bytes.

--mode encrypt takes the outbound rows on the same batches:
`enc` (k_espenc, fcgpu_espaes_configure(ENCRYPT)), `seal` (k_espauth in
FCGPU_ESP_SEAL), `both` (SEAL then ENCRYPT in one call) and `aes` (k_espaes,
decryption, the yardstick of the same session). --ab then adds, for the IMIX
batch, k_espenc sorted by block count against arrival order
(FCGPU_ESPENC_ORDER), two alternating rounds."""
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
SAS = [(0x2000 + k, bytes((11 * k + j) & 0xFF for j in range(16))) for k in range(4)]


def batch_for(flen, seed):
    """Frames of the given lengths: SPI, random payload, elen = 28 + 8 k."""
    n = len(flen)
    rng = np.random.default_rng(seed)
    iplen = 34 + 28 + (flen - 62) // 8 * 8
    hdr = synth.build_headers(n, src=rng.integers(1 << 24, 2**32, n, dtype=np.uint64), dst=synth.ip4(10, 0, 0, 2),
                              sport=rng.integers(0, 65536, n), dport=53, proto=50, frame_len=iplen, width=64)
    b = synth.pack(hdr, flen)
    body = rng.integers(0, 256, b.arena.size, dtype=np.uint8)
    spi = synth._be32(np.asarray([s for s, _ in SAS])[np.arange(n) % 4])
    for L in np.unique(flen):
        sel = np.nonzero(flen == L)[0]
        idx = b.desc[sel, 0].astype(np.int64)[:, None] + np.arange(34, L)[None, :]
        b.arena[idx] = body[idx]
        b.arena[idx[:, :4]] = spi[sel]
    return b, int((((flen - 62) // 8 * 8 + 8) // 16).sum())


def time_row(name, b, blocks, steps, repeat, aes=False, auth=False, outbound=False):
    n = b.n
    ctx = N.Context(0, n, N.make_cfg(offset=14, checksum=True, hash_mode=N.HASH_FLOWID, nports=NPORTS))
    if aes:
        ctx.espaes_set_sas(SAS)
        ctx.espaes_configure(N.ESPAES_ENCRYPT if outbound else N.ESPAES_DECRYPT)
    if auth:
        ctx.espauth_set_sas(SAS)
        ctx.espauth_configure(N.ESP_SEAL if outbound else N.ESP_VERIFY)
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
    if aes or auth:
        row["post_us"] = post = round(row["step_us"] - row["k_rx_us"], 2)
    if aes:
        st = ctx.espaes_stats()
        row.update(mblk_s=round(blocks / post, 1), gbps=round(16e-3 * blocks / post, 2), ok=int(st["ok"]) // ((repeat + 1) * steps),
                   blocks=int(st["blocks"]) // ((repeat + 1) * steps))
    ctx.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--mode", choices=["decrypt", "encrypt"], default="decrypt")
    args = ap.parse_args()
    rng = np.random.default_rng(3)
    shapes = {"64": np.full(args.n, 64), "1500": np.full(max(args.n * 64 // 1536, 1), 1500),
              "imix": (synth.IMIX_LEN + 4)[rng.choice(3, args.n // 4, p=synth.IMIX_W)]}
    for name, flen in shapes.items():
        b, blocks = batch_for(flen, seed=len(name))
        time_row(f"off/{name}", b, blocks, args.steps, args.repeat)
        if args.mode == "encrypt":
            time_row(f"enc/{name}", b, blocks, args.steps, args.repeat, aes=True, outbound=True)
            time_row(f"seal/{name}", b, blocks, args.steps, args.repeat, auth=True, outbound=True)
            time_row(f"both/{name}", b, blocks, args.steps, args.repeat, aes=True, auth=True, outbound=True)
            time_row(f"aes/{name}", b, blocks, args.steps, args.repeat, aes=True)
            if args.ab and name == "imix":
                for rnd in range(2):
                    for o in "10":
                        os.environ["FCGPU_ESPENC_ORDER"] = o
                        time_row(f"order{o}.{rnd}/{name}", b, blocks, args.steps, args.repeat, aes=True, outbound=True)
                del os.environ["FCGPU_ESPENC_ORDER"]
            continue
        time_row(f"aes/{name}", b, blocks, args.steps, args.repeat, aes=True)
        time_row(f"auth/{name}", b, blocks, args.steps, args.repeat, auth=True)
        time_row(f"both/{name}", b, blocks, args.steps, args.repeat, aes=True, auth=True)
        if args.ab and name == "1500":
            for rnd in range(2):                       # twice, alternating: the spread beside the difference
                for t in "14":
                    for r in "124":
                        os.environ["FCGPU_ESPAES_TABLES"], os.environ["FCGPU_ESPAES_REPLICAS"] = t, r
                        time_row(f"t{t}r{r}.{rnd}/{name}", b, blocks, args.steps, args.repeat, aes=True)
            del os.environ["FCGPU_ESPAES_TABLES"], os.environ["FCGPU_ESPAES_REPLICAS"]


if __name__ == "__main__":
    main()
