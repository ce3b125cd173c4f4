"""FCGPU_CLS_ROUTE: IPRouteTable::process (elements/ip/iproutetable.cc:152-169)
over the 16-8-8 trie of csrc/host/route_table.hh. The reference everywhere is
a numpy linear scan (mask, compare, keep the longest match); the reference's
own iplookups-01 / -02 expectations (tests/golden/iplookups.json) pin the host
walk. Everything but the port and DST_IP comes from the oracle with CLS_NONE."""
import json
import os

import numpy as np
import pytest

from fastclick_amd import synth
from fastclick_amd import _native as N

FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "iplookups.json")))


def _host(dotted):
    a, b, c, d = (int(x) for x in dotted.split("."))
    return (a << 24) | (b << 16) | (c << 8) | d


def _routes(rows):
    """[ADDR/LEN, [GW,] OUT] rows -> (addr, plen, gw, port) with dotted strings."""
    out = []
    for r in rows:
        addr, plen = r[0].split("/")
        out.append((addr, int(plen), r[1] if len(r) == 3 else 0, r[-1]))
    return out


def _scan(routes, dst):
    """Linear-scan longest-prefix match of host-order dst: (port or -1, raw gw)."""
    port = np.full(len(dst), -1, np.int64)
    gw = np.zeros(len(dst), np.uint32)
    best = np.full(len(dst), -1, np.int64)
    for addr, plen, g, p in routes:
        mask = (0xFFFFFFFF << (32 - plen)) & 0xFFFFFFFF
        hit = ((dst & mask) == (_host(addr) & mask)) & (plen > best)
        port[hit], best[hit] = p, plen
        gw[hit] = N.raw_addr(g) if g else 0
    return port, gw


def _unparse(raw):
    return ".".join(str((raw >> (8 * k)) & 255) for k in range(4))


def _dotted(host):
    return ".".join(str((host >> s) & 255) for s in (24, 16, 8, 0))

@pytest.mark.parametrize("state", FIX["iplookups-01"]["states"], ids=lambda s: f"line{s['line']}")
def test_iplookups_01(state):
    f = FIX["iplookups-01"]
    routes = _routes(state["routes"])
    port, gw = N.route_lookup(routes, f["lookup"], f["nports"])
    assert (f"{port} {_unparse(gw)}" if port >= 0 else "-1") == state["expect"]
    if "refused" in state:     # "conflict with existing route": the table stays as it was
        with pytest.raises(ValueError, match="conflict with existing route '18.16.0.0/12'"):
            N.route_lookup(routes + _routes([state["refused"]]), f["lookup"], f["nports"])


def _table_02():
    f = FIX["iplookups-02"]
    return _routes(f["configured"] + f["added"])


def test_iplookups_02():
    f = FIX["iplookups-02"]
    routes = _table_02()
    assert len(routes) == 8 + 1 + 1518
    assert N.route_lookup(routes, f["lookup"], f["nports"]) == (int(f["expect"]), 0)
    rng = np.random.default_rng(2002)
    dst = rng.integers(0, 2**32, 2000, dtype=np.uint64).astype(np.int64)
    dst[:len(routes)] = [_host(r[0]) for r in routes]            # every prefix's first address
    want, _ = _scan(routes, dst)
    arr = N.routes_array(routes)
    got = [N.route_lookup(arr, _dotted(int(d)))[0] for d in dst]
    assert got == want.tolist()


@pytest.mark.parametrize("routes,nports,msg", [
    ([("10.0.0.0", 8, 0, 0), ("10.1.2.3", 8, "1.1.1.1", 1)], 2, "conflict"),    # equal after addr &= mask
    ([("10.0.0.0", 8, 0, 2)], 2, "OUTPUT"),
    ([("10.0.0.0", 33, 0, 0)], 2, "prefix length"),
    ([(f"{k >> 8}.{k & 255}.1.0", 24, 0, 0) for k in range(32768)], 1, "chunks"),     # one chunk per /16
])
def test_route_table_errors(routes, nports, msg):
    with pytest.raises(ValueError, match=msg):
        N.route_lookup(routes, "10.0.0.1", nports)

NESTED = "77.141.203.85"     # every byte odd and distinct: each prefix length ends inside a chunk


def _nested(lo):
    h = _host(NESTED)
    return [(_dotted(h >> (32 - p) << (32 - p)), p, f"9.9.{p}.1", p % 7) for p in range(lo, 33)]


TABLES = {
    "iplookups02": (_table_02, 17),
    "nested": (lambda: _nested(0), 7),
    "nested-nodefault": (lambda: _nested(1), 7),
    # 600 next hops: more than the 512 that are staged in LDS
    "hops600": (lambda: [(f"10.{k >> 8}.{k & 255}.0", 24, f"172.16.{k >> 8}.{k & 255}", k % 5) for k in range(600)], 5),
    "nogw": (lambda: [("10.0.0.0", 8, 0, 0), ("10.128.0.0", 9, 0, 1), ("10.128.7.0", 24, "1.2.3.4", 2),
                      ("10.128.7.128", 25, 0, 3)], 4),
}
N_PKT = 4096 + 37


def _batch(routes, seed, ttl=64):
    """Destinations: every route's edges and the addresses just outside, then
    seeded random ones; a few percent header errors and IP options."""
    rng = np.random.default_rng(seed)
    edge = []
    for addr, plen, _, _ in routes:
        lo = _host(addr) & ((0xFFFFFFFF << (32 - plen)) & 0xFFFFFFFF)
        hi = lo + (1 << (32 - plen)) - 1
        edge += [lo, hi, (lo - 1) & 0xFFFFFFFF, (hi + 1) & 0xFFFFFFFF]
    dst = rng.integers(0, 2**32, N_PKT, dtype=np.uint64)
    # half of the random ones near the table, so they do not all miss
    near = rng.integers(0, len(routes), N_PKT)
    base = np.array([_host(r[0]) for r in routes], np.uint64)[near]
    dst = np.where(rng.random(N_PKT) < 0.5, base ^ (np.uint64(1) << rng.integers(0, 12, N_PKT).astype(np.uint64)), dst)
    edge = np.array(edge[:N_PKT], np.uint64)
    dst[rng.permutation(N_PKT)[:len(edge)]] = edge
    hdr = synth.build_headers(N_PKT, src=rng.integers(1 << 24, 2**32, N_PKT, dtype=np.uint64), dst=dst,
                              sport=rng.integers(0, 65536, N_PKT), dport=rng.integers(0, 65536, N_PKT),
                              frame_len=60, width=64, ttl=ttl)
    b = synth.pack(hdr, 60)
    synth.add_ip_options(b, 0.03, seed=seed + 1)
    synth.inject_errors(b, 0.01, seed=seed + 2)
    return b


def _expect(oracle, cfg, b, routes):
    """The oracle's CLS_NONE result with the scan's ports and gateways put in."""
    n, nports = b.n, cfg.nports
    c0 = N.make_cfg(check_mode=cfg.check_mode, offset=cfg.offset, checksum=bool(cfg.checksum), nports=nports)
    c0.hash_mode = cfg.hash_mode
    chk = oracle.process_batch(c0, b)                     # the checks alone
    c0.rewrite = cfg.rewrite
    e = oracle.process_batch(c0, b)                       # ... and the rewrite of what port 0 let through
    valid = chk["reason"] == N.R_OK
    # the key: the header's ip_dst word (GetIPAddress(16); CheckIPHeader's annotation)
    at = b.desc[:, 0].astype(np.int64)[:, None] + cfg.offset + 16 + np.arange(4)
    dst_raw = np.ascontiguousarray(b.arena[at]).view("<u4").ravel()
    port, gw = _scan(routes, dst_raw.byteswap().astype(np.int64))
    noroute = valid & (port < 0)
    reason = np.where(noroute, N.R_NO_MATCH, e["reason"]).astype(np.uint8)
    eport = np.where(reason == N.R_OK, port, nports).astype(np.uint8)
    out = dict(reason=reason, port=eport, hash=e["hash"], ip_rw=np.where(noroute, 0, e["ip_rw"]).astype(np.uint32),
               dst_ip=np.where(valid & (port >= 0) & (gw != 0), gw, dst_raw), anno=e["anno"])
    out["perm"] = np.argsort(eport, kind="stable").astype(np.uint32)
    cnt = np.bincount(eport, minlength=nports + 1)
    out["port_start"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    tiles = [eport[t:t + N.TILE] for t in range(0, n, N.TILE)]
    out["perm_tile"] = np.concatenate([t0 + np.argsort(t, kind="stable")
                                       for t0, t in zip(range(0, n, N.TILE), tiles)]).astype(np.uint32)
    out["tile_count"] = np.concatenate([np.bincount(t, minlength=nports + 1) for t in tiles]).astype(np.uint16)
    ctr = np.zeros(N.NCOUNTERS, np.uint64)
    ctr[N.CTR_PORT:N.CTR_PORT + nports + 1] = cnt
    for r in np.unique(reason[reason != N.R_OK]):
        ctr[N.CTR_REASON + N.reason_slot(int(r))] = int((reason == r).sum())
    ctr[N.CTR_DROPS] = ctr[N.CTR_REASON:N.CTR_REASON + N.reason_slot(N.R_NO_MATCH)].sum()
    ctr[N.CTR_COUNT] = n - ctr[N.CTR_DROPS]
    out["counters"] = ctr
    return out


def _check(got, exp, part, what=""):
    for k in ("reason", "port", "hash"):
        assert np.array_equal(got[k], exp[k]), f"{what}{k}"
    seen = np.isin(exp["reason"], (N.R_OK, N.R_NO_MATCH))
    assert np.array_equal(got["anno"]["dst_ip"][seen], exp["dst_ip"][seen]), f"{what}dst_ip"
    ok = exp["reason"] == N.R_OK
    for f in ("length", "nh", "th"):
        assert np.array_equal(got["anno"][f][ok], exp["anno"][f][ok]), f"{what}anno.{f}"
    keys = ("perm_tile", "tile_count") if part == N.PART_TILE else ("perm", "port_start")
    for k in keys + ("counters",) + (("ip_rw",) if "ip_rw" in got else ()):
        assert np.array_equal(got[k], exp[k]), f"{what}{k}"


def _cases():
    for name in TABLES:
        for part in (N.PART_TILE, N.PART_GLOBAL):
            for mode in (N.CHECK_IP4, N.MARK_IP4):
                yield pytest.param(name, part, mode, 0, id=f"{name}-{'tile' if part else 'global'}-"
                                                           f"{'mark' if mode else 'check'}")
    yield pytest.param("nested-nodefault", N.PART_TILE, N.CHECK_IP4, N.RW_DECTTL | N.RW_SETCKSUM, id="rewrite")


@pytest.mark.gpu
@pytest.mark.parametrize("name,part,mode,rewrite", _cases())
def test_gpu_route_matches_scan(oracle, name, part, mode, rewrite):
    from fastclick_amd import device as D
    mk, nports = TABLES[name]
    routes = mk()
    b = _batch(routes, seed=len(name) + 31 * part + mode, ttl=np.where(np.arange(N_PKT) % 5, 64, 1) if rewrite else 64)
    cfg = N.make_cfg(check_mode=mode, offset=14, checksum=True, classify=N.CLS_ROUTE, nports=nports,
                     hash_mode=N.HASH_FLOWID, rewrite=rewrite)
    exp = _expect(oracle, cfg, b, routes)
    assert (exp["reason"] == N.R_NO_MATCH).any() == (name not in ("iplookups02", "nested"))
    got = D.process_batch(b, cfg, partition=part, routes=routes)
    _check(got, exp, part)


@pytest.mark.gpu
def test_gpu_route_replace_table_and_errors(oracle):
    """One context, three tables in turn; no table, an output >= nports and
    CLS_ROUTE outside the IPv4 check modes are refused."""
    import torch
    from fastclick_amd import device as D
    cfg = N.make_cfg(offset=14, checksum=True, classify=N.CLS_ROUTE, nports=7)
    ctx = N.Context(0, N_PKT, cfg)
    try:
        db0 = D.DeviceBatch.upload(synth.c4(300, seed=1))
        with pytest.raises(RuntimeError, match="fcgpu_set_routes"):
            D.run_device(ctx, db0, D.DeviceOutputs(300, 7))
        with pytest.raises(RuntimeError, match="OUTPUT"):
            ctx.set_routes([("10.0.0.0", 8, 0, 7)])
        for k, routes in enumerate((_nested(1), TABLES["hops600"][0](), [])):
            ctx.set_routes(routes)
            ctx.reset_counters()
            b = _batch(routes or _nested(1), seed=70 + k)
            outs = D.DeviceOutputs(b.n, 7, anno=True, perm=True, port_start=True)
            D.run_device(ctx, D.DeviceBatch.upload(b), outs)
            torch.cuda.synchronize()
            got = dict(outs.numpy(), counters=ctx.counters())
            _check(got, _expect(oracle, cfg, b, routes), N.PART_GLOBAL, f"table {k}: ")
        for mode in (N.CHECK_AUTO, N.MARK_IP6):
            with pytest.raises(RuntimeError, match="IPv4 check modes"):
                ctx.configure(N.make_cfg(check_mode=mode, classify=N.CLS_ROUTE, nports=7))
    finally:
        ctx.close()

EL_ROUTES = "10.0.0.0/8 0, 10.128/9 - 1, 10.128.7.0/24 1.2.3.4 2, 10.128.7.128/255.255.255.128 3"


def test_element_routes_config():
    """ROUTES implies CLS_ROUTE, N defaults to the largest OUT + 1."""
    from fastclick_amd import click as K
    c = K.element_cfg(f'GPUIPCheckClassify(OFFSET 14, ROUTES "{EL_ROUTES}")')
    assert (c.classify, c.nports) == (N.CLS_ROUTE, 4)
    assert K.element_cfg(f'GPUIPCheckClassify(OFFSET 14, N 9, ROUTES "{EL_ROUTES}")').nports == 9
    for bad, msg in ((f'ROUTES "{EL_ROUTES}", LB_MODE hash', "conflicts"), (f'ROUTES "{EL_ROUTES}", N 3', "OUTPUT"),
                     ('ROUTES "10.0.0.0/8 0, 10.9.9.9/8 1"', "conflict with existing route"),
                     (f'ROUTES "{EL_ROUTES}", MODE AUTO', "MODE CHECK or MARK"), ('ROUTES "10.0.0.0/8 x 0"', "GATEWAY")):
        with pytest.raises(K.ConfigError, match=msg):
            K.check_config(f"GPUIPCheckClassify(OFFSET 14, {bad})")


@pytest.mark.gpu
def test_element_routes(oracle):
    """Through the element, whose block submissions take FCGPU_OUT_ANNO8
    annotations for IPv4 chains: per-output packets, the gateway in the DST_IP
    annotation, no-route packets killed, and the `table` handler."""
    from fastclick_amd import click as K
    routes = TABLES["nogw"][0]()
    b = _batch(routes, seed=95)
    exp = _expect(oracle, N.make_cfg(offset=14, checksum=True, classify=N.CLS_ROUTE, nports=4), b, routes)
    r = K.run_element(f'GPUIPCheckClassify(OFFSET 14, CHECKSUM true, ROUTES "{EL_ROUTES}")', b, nsinks=5)
    want = np.where(exp["reason"] == N.R_NO_MATCH, 0xFFFFFFFF, exp["port"].astype(np.uint32)).astype(np.uint32)
    assert np.array_equal(r["port"], want)
    ok = exp["reason"] == N.R_OK
    assert np.array_equal(r["dst"][ok], exp["dst_ip"][ok])
    assert r["handlers"]["port_counts"] == " ".join(str(int(c)) for c in exp["counters"][N.CTR_PORT:N.CTR_PORT + 5])
    assert r["handlers"]["table"].rstrip("\n") == ("10.0.0.0/8\t\t-\t\t0\n10.128.0.0/9\t\t-\t\t1\n"
                                      "10.128.7.0/24\t\t1.2.3.4\t\t2\n10.128.7.128/25\t\t-\t\t3")
