"""k_rx time per 1M-packet batch with a route table (CLS_ROUTE) beside the
"one extra table read per packet" path that existed before it (CLS_LB_TABLE
with a 65536-bucket ring): C2-shaped batches (60-B frames in 64-B slots,
checksum, FLOWID hash, tile partition, 16 outputs), 8 rotating device copies,
every 8th launch timed (fcgpu_set_timing). Destinations are drawn from the
table's prefixes, so every packet has a route; the LB_TABLE rows run on the
same batches.

    python scripts/route_bench.py [--steps 200] [--repeat 3] [--only lbtable|route|route6|lbhash6]

Tables: `iplookups02` (tests/golden/iplookups.json, 1527 routes, /32 hosts
among /8../24) and `synth500k` (8192 /16 blocks with 61 /24s each, a /8 and a
/16 over them, 64 next hops: a 4.3-MB trie, more than the 4-MB L2). The
package is taken from the current directory, so the LB_TABLE row can be run
from a checkout of another commit (--only lbtable). One JSON line per row.

IPv6 (CLS_ROUTE6, --only route6): all-IPv6 64-B frames in 64-B slots under
CHECK_AUTO, tables `v6default` (::/0 alone), `v6-1.5k` (4 /32 allocations, each
with 30 /48s of 12 /64s) and `v6-200k` (512 such allocations over 64 top-16-bit
values: 200,192 routes). The yardstick row is CHECK_AUTO + CLS_LB_HASH on the
same batches (--only lbhash6, which uses nothing newer than CLS_LB_HASH and so
runs from a checkout of the parent commit too)."""
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

HERE = os.path.dirname(os.path.abspath(__file__))
NPORTS = 16


def table_iplookups02():
    f = json.load(open(os.path.join(HERE, "..", "tests", "golden", "iplookups.json")))["iplookups-02"]
    rows = []
    for pfx, out in f["configured"] + f["added"]:
        a, l = pfx.split("/")
        rows.append((int.from_bytes(bytes(int(x) for x in a.split(".")), "big"), int(l), 0, out % NPORTS))
    return rows


def table_synth500k():
    rows = [(20 << 24, 8, 1, 0)]
    for blk in range(8192):
        hi = (20 << 24) + (blk << 16)
        if blk % 64 == 0:
            rows.append((hi, 16, 2, 1))
        rows += [(hi + (k * 4 << 8), 24, 3 + (blk + k) % 62, (3 + (blk + k) % 62) % NPORTS) for k in range(61)]
    return rows


def as_routes(rows):
    r = np.zeros(len(rows), N.route_dtype())
    a = np.array([x[0] for x in rows], np.uint32)
    r["addr"] = a.byteswap()
    r["gw"] = np.array([x[2] for x in rows], np.uint32)       # any distinct words serve as gateways
    r["plen"] = [x[1] for x in rows]
    r["port"] = [x[3] for x in rows]
    return r


def batch_for(rows, n, seed):
    """C2's frames with each destination inside a route drawn at random."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(rows), n)
    base = np.array([x[0] for x in rows], np.uint64)[pick]
    span = np.array([32 - x[1] for x in rows], np.uint64)[pick]
    dst = base + (rng.integers(0, 2**32, n, dtype=np.uint64) & ((np.uint64(1) << span) - np.uint64(1)))
    hdr = synth.build_headers(n, src=synth.ip4(10, 0, 0, 1), dst=dst, sport=1234, dport=5678, frame_len=60, width=64)
    return synth.pack(hdr, 60)


def table6(nblk):
    """(addr, plen, gw, port) on Python ints: nblk /32 allocations, 8 per top-16-bit value."""
    rows = []
    for blk in range(nblk):
        a32 = (0x2400 + (blk >> 3) * 0x10 << 112) | ((0x0100 + (blk & 7) * 0x1111) << 96)
        rows.append((a32, 32, 0, blk % NPORTS))
        for s in range(30):
            a48 = a32 | s << 80
            rows.append((a48, 48, 1 + (blk + s) % 60, (blk + s) % NPORTS))
            rows += [(a48 | k << 64, 64, 1 + (blk + s + k) % 60, (s + k) % NPORTS) for k in range(12)]
    return rows or [(0, 0, 0, 3)]


def as_routes6(rows):
    r = np.zeros(len(rows), N.route6_dtype())
    r["addr"] = np.frombuffer(b"".join(x[0].to_bytes(16, "big") for x in rows), np.uint8).reshape(-1, 16)
    r["gw"][:, 0], r["gw"][:, 15] = [0xfe if x[2] else 0 for x in rows], [x[2] for x in rows]
    r["plen"] = [x[1] for x in rows]
    r["port"] = [x[3] for x in rows]
    return r


def batch6_for(rows, n, seed):
    """All-IPv6 64-B frames, each destination inside a route drawn at random."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(rows), n)
    dst = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    base = np.frombuffer(b"".join(x[0].to_bytes(16, "big") for x in rows), np.uint8).reshape(-1, 16)[pick]
    plen = np.array([x[1] for x in rows])[pick]
    keep = np.clip(plen[:, None] - 8 * np.arange(16)[None, :], 0, 8)          # prefix bits per byte
    m = (0xff00 >> keep).astype(np.uint8)
    dst = (base & m) | (dst & ~m)
    hdr = synth.build_headers(n, src=0, dst=0, sport=rng.integers(0, 65536, n), dport=rng.integers(0, 65536, n),
                              frame_len=64, width=64,
                              ip6=dict(mask=np.ones(n, bool), src=rng.integers(0, 256, (n, 16), dtype=np.uint8), dst=dst))
    return synth.pack(hdr, 64)


def time_row(name, classify, b, steps, repeat, routes=None, ring=None, routes6=None):
    n = b.n
    cfg = N.make_cfg(offset=14, checksum=True, hash_mode=N.HASH_FLOWID, classify=classify, nports=NPORTS)
    if routes6 is not None or classify == N.CLS_LB_HASH:       # the IPv6 rows: CHECK_AUTO from the Ethernet header
        cfg = N.make_cfg(check_mode=N.CHECK_AUTO, offset=0, checksum=True, hash_mode=N.HASH_FLOWID, classify=classify,
                         nports=NPORTS)
    ctx = N.Context(0, n, cfg)
    if routes is not None:
        ctx.set_routes(routes)
    if routes6 is not None:
        ctx.set_routes6(routes6)
    if ring is not None:
        ctx.set_lb_table(ring)
    db = DeviceBatch.upload(b, device="cuda:0")
    bufs = [(db.arena, db.desc)] + [(db.arena.clone(), db.desc.clone()) for _ in range(7)]
    outs = DeviceOutputs(n, NPORTS, device="cuda:0", tile_perm=True, partition=N.PART_TILE)
    s = torch.cuda.current_stream().cuda_stream
    us = []
    for rep in range(repeat + 1):                      # the first round warms up
        ctx.set_timing(8)
        for k in range(steps):
            a, d = bufs[k % len(bufs)]
            ctx.process(a.data_ptr(), d.data_ptr(), n, stream=s, **outs.ptrs())
        torch.cuda.synchronize()
        ms, cnt = ctx.read_timing()
        if rep:
            us.append(1e3 * ms[0] / max(cnt[0], 1))
    v = outs.numpy()
    ctx.close()
    print(json.dumps(dict(row=name, k_rx_us_median=round(statistics.median(us), 3),
                          k_rx_us=[round(x, 3) for x in us], packets=n, steps=steps,
                          valid=int((v["reason"] == N.R_OK).sum()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--only", choices=["lbtable", "route", "route6", "lbhash6"], default=None)
    args = ap.parse_args()
    for tname, nblk in (("v6default", 0), ("v6-1.5k", 4), ("v6-200k", 512)):
        if args.only not in ("route6", "lbhash6"):
            break
        rows = table6(nblk)
        b = batch6_for(rows, args.n, seed=len(rows))
        if args.only == "lbhash6":
            time_row(f"auto-lbhash/{tname}-batch", N.CLS_LB_HASH, b, args.steps, args.repeat)
        else:
            r6 = as_routes6(rows)
            chunks, loads = N.route6_stats(r6)
            print(json.dumps(dict(table=tname, routes=len(rows), chunks=chunks, max_loads=loads,
                                  trie_bytes=262144 + 1040 * chunks)), flush=True)
            time_row(f"route6/{tname}", N.CLS_ROUTE6, b, args.steps, args.repeat, routes6=r6)
    if args.only in ("route6", "lbhash6"):
        return
    for tname, mk in (("iplookups02", table_iplookups02), ("synth500k", table_synth500k)):
        rows = mk()
        b = batch_for(rows, args.n, seed=len(rows))
        if args.only != "route":
            ring = N.lb_hash_ring(NPORTS, 65536)
            time_row(f"lbtable65536/{tname}-batch", N.CLS_LB_TABLE, b, args.steps, args.repeat, ring=ring)
        if args.only != "lbtable":
            time_row(f"route/{tname}", N.CLS_ROUTE, b, args.steps, args.repeat, routes=as_routes(rows))


if __name__ == "__main__":
    main()
