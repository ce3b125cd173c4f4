"""FCGPU_CLS_ROUTE6: LookupIP6Route behind GetIP6Address(24) over the
path-compressed trie of csrc/host/route6_table.hh. The reference everywhere is
an exact linear scan over the route list on Python ints (longest match, the
last of equal addr/plen wins, gateway ids by first appearance); everything but
the port, dst_ip and the no-route reason comes from the oracle with CLS_NONE."""
import functools

import numpy as np
import pytest

from fastclick_amd import synth
from fastclick_amd import _native as N
from tests.test_route import _check

N_PKT = 4096 + 37
A = int.from_bytes(bytes.fromhex("20010db885a317425b8e03707334c96f"), "big")   # 16 distinct non-zero bytes
DB8 = 0x20010db8 << 96
A4 = (77 << 24) | (141 << 16) | (203 << 8) | 85


def _mask(x, plen, w=128):
    return x >> (w - plen) << (w - plen)


def _nested(lo):
    return [(_mask(A, p), p, (0xfe80 << 112) | p if p % 3 == 0 else 0, p % 7) for p in range(lo, 129)]


def _sparse():
    rng = np.random.default_rng(48)
    rnd = [int.from_bytes(rng.bytes(12), "big") for _ in range(40)]
    return [(DB8, 32, 0, 0)] + [(_mask(DB8 | r, p), p, (0xfe80 << 112) | (k % 9) if k % 2 else 0, 1 + k % 4)
                                for k, (r, p) in enumerate(zip(rnd, [48, 64, 96, 128] * 10))]


TABLES = {   # name -> (routes as (addr, plen, gw, port) ints, nports)
    "nested": (lambda: _nested(0), 7),
    "nested-nodefault": (lambda: _nested(1), 7),
    "sparse": (_sparse, 5),
    "hops600": (lambda: [(DB8 | k << 64, 64, (0xfe80 << 112) | (1000 + k), k % 5) for k in range(600)], 5),
    "dup": (lambda: [(0, 0, 0, 3), (DB8, 32, 1, 0), (DB8 | 7 << 80, 48, 0, 1), (DB8 | 0xffff, 32, 2, 2),
                     (0, 0, 1, 1), (DB8 | 7 << 80, 48, 2, 0), (A, 128, 0, 3), (A, 128, 0, 2)], 4),
}
NO_DEFAULT = ("nested-nodefault", "sparse", "hops600")


def _native(routes, w=128):
    if w == 32:      # raw network-order words
        return [(int.from_bytes(a.to_bytes(4, "big"), "little"), p, int.from_bytes(g.to_bytes(4, "big"), "little"), o)
                for a, p, g, o in routes]
    return [(a.to_bytes(16, "big"), p, g.to_bytes(16, "big") if g else 0, o) for a, p, g, o in routes]


def _scan(routes, keys, w=128):
    """Index of the winning route per key (-1: none), and each route's gateway id."""
    ids = {}
    for _, _, g, _ in routes:
        if g:
            ids.setdefault(g, len(ids) + 1)
    pre = [(a >> (w - p), w - p, p) for a, p, _, _ in routes]
    win = []
    for k in keys:
        best, bi = -1, -1
        for i, (pf, sh, p) in enumerate(pre):
            if p >= best and (k >> sh) == pf:
                best, bi = p, i
        win.append(bi)
    return np.array(win), np.array([ids.get(g, 0) for _, _, g, _ in routes] + [0])


def _dests(routes, n, seed, w=128):
    """First and last address of every route, then (sampled to fit) the two
    addresses outside, every byte below the root replaced, bit flips inside the
    prefix; seeded random addresses, half of them near a route, for the rest."""
    rng = np.random.default_rng(seed)
    full, must, more = (1 << w) - 1, [], []
    for a, p, _, _ in routes:
        hi = a | (full >> p)
        must += [a, hi]
        more += [(a - 1) & full, (hi + 1) & full]
        more += [a ^ (int(rng.integers(1, 256)) << (8 * (w // 8 - 1 - j))) for j in range(2, w // 8)]
        more += [a ^ (1 << (w - 1 - int(b))) for b in rng.integers(0, p, 4)] if p else []
    room = n * 7 // 8 - len(must)
    more = [more[i] for i in rng.permutation(len(more))[:room]]
    rest = n - len(must) - len(more)
    near = [routes[i][0] ^ int.from_bytes(rng.bytes(w // 16), "big") for i in rng.integers(0, len(routes), rest // 2)]
    rand = [int.from_bytes(rng.bytes(w // 8), "big") for _ in range(rest - len(near))]
    return must + more + near + rand


def _bytes16(keys):
    return np.frombuffer(b"".join(k.to_bytes(16, "big") for k in keys), np.uint8).reshape(-1, 16)


def _headers(name, routes):
    rng = np.random.default_rng(len(name))
    dst = _bytes16(_dests(routes, N_PKT, seed=len(name) + 1))
    return synth.build_headers(N_PKT, src=0, dst=0, sport=rng.integers(0, 65536, N_PKT),
                               dport=rng.integers(0, 65536, N_PKT), frame_len=78,
                               ip6=dict(mask=np.ones(N_PKT, bool), src=rng.integers(0, 256, (N_PKT, 16)), dst=dst))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(routes, nports, all-IPv6 batch) of a table; shared by its cases."""
    mk, nports = TABLES[name]
    routes = mk()
    b = synth.pack(_headers(name, routes), 78)
    synth.inject_errors(b, 0.01, seed=len(name) + 2)
    return routes, nports, b


def _key(b, off, width):
    at = b.desc[:, 0].astype(np.int64)[:, None] + off[:, None] + np.arange(width)
    return [int.from_bytes(bytes(r), "big") for r in b.arena[at]]


def _expect(oracle, cfg, b, routes6, routes4=()):
    """The oracle's CLS_NONE result with the scans' ports and dst_ip put in."""
    n, nports = b.n, cfg.nports
    c0 = N.make_cfg(check_mode=cfg.check_mode, offset=cfg.offset, checksum=bool(cfg.checksum), nports=nports)
    e = oracle.process_batch(c0, b)
    valid, v6 = e["reason"] == N.R_OK, e["anno"]["ipver"] == 6
    nh = np.where(valid, e["anno"]["nh"], 0).astype(np.int64)
    w6, gid6 = _scan(routes6, _key(b, nh + 24, 16))
    w4, _ = _scan(routes4, _key(b, nh + 16, 4), 32)
    port6 = np.array([r[3] for r in routes6] + [-1])[w6]
    port4 = np.array([r[3] for r in routes4] + [-1])[w4]
    gw4 = np.array([int.from_bytes(r[2].to_bytes(4, "big"), "little") for r in routes4] + [0], np.uint32)[w4]
    port = np.where(v6, port6, port4)
    noroute = valid & (port < 0)
    reason = np.where(noroute, N.R_NO_MATCH, e["reason"]).astype(np.uint8)
    eport = np.where(reason == N.R_OK, port, nports).astype(np.uint8)
    dst4 = np.where((port4 >= 0) & (gw4 != 0), gw4, e["anno"]["dst_ip"])
    out = dict(reason=reason, port=eport, hash=e["hash"], anno=e["anno"], won6=set(w6[valid & v6]),
               dst_ip=np.where(v6, np.where(port6 >= 0, gid6[w6], 0), dst4).astype(np.uint32))
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


def _returnable(routes):
    """The routes the scan can return at all: a route wins somewhere iff it
    wins at its own first address or just past the end of a longer route
    inside it (the points where the winner can change within its range)."""
    full = (1 << 128) - 1
    pts = [a for a, _, _, _ in routes]
    for a, p, _, _ in routes:
        ends = [(b | full >> q) + 1 for b, q, _, _ in routes if q > p and b >> (128 - p) == a >> (128 - p)]
        pts += [x for x in ends if x <= full and x >> (128 - p) == a >> (128 - p)]
    return set(_scan(routes, pts)[0]) - {-1}


def _conditions(exp, routes6, name):
    """What a batch must contain for its comparison to mean something."""
    assert (exp["reason"] != N.R_OK).sum() - (exp["reason"] == N.R_NO_MATCH).sum() <= 0.1 * len(exp["reason"])
    assert _returnable(routes6) <= exp["won6"], "a route no valid packet is routed by"
    assert (exp["reason"] == N.R_NO_MATCH).any() == (name in NO_DEFAULT)


@pytest.mark.parametrize("name", TABLES)
def test_batches_meet_conditions_by_scan_alone(name):
    """The seeds, checked without oracle or GPU: at most 2 % of the frames
    differ from what synth built (inject_errors at 1 %), so counting every
    changed frame as invalid, the untouched ones alone hit every returnable
    route, and a no-route one exists exactly without a /0."""
    routes, _, b = _case(name)
    keys = _dests(routes, N_PKT, seed=len(name) + 1)
    clean = np.array(_key(b, np.full(b.n, 38), 16), object) == np.array(keys, object)
    at = b.desc[:, 0].astype(np.int64)[:, None] + np.arange(78)
    ref = synth.pack(_headers(name, routes), 78)
    clean &= (b.arena[at] == ref.arena[at]).all(axis=1) & (b.desc[:, 1] == ref.desc[:, 1])
    assert clean.sum() >= 0.9 * b.n
    win = _scan(routes, [k for k, c in zip(keys, clean) if c])[0]
    assert _returnable(routes) <= set(win)
    assert (-1 in win) == (name in NO_DEFAULT)


@pytest.mark.gpu
@pytest.mark.parametrize("name,part,mode", [(t, p, N.CHECK_AUTO) for t in TABLES for p in (N.PART_TILE, N.PART_GLOBAL)]
                         + [("nested", N.PART_TILE, N.MARK_IP6)])
def test_gpu_route6_matches_scan(oracle, name, part, mode):
    from fastclick_amd import device as D
    routes, nports, b = _case(name)
    cfg = N.make_cfg(check_mode=mode, offset=0 if mode == N.CHECK_AUTO else 14, checksum=True, classify=N.CLS_ROUTE6,
                     nports=nports, hash_mode=N.HASH_FLOWID)
    exp = _expect(oracle, cfg, b, routes)
    _conditions(exp, routes, name)
    got = D.process_batch(b, cfg, partition=part, routes6=_native(routes))
    _check(got, exp, part)


@pytest.mark.gpu
def test_gpu_route6_dual_stack(oracle):
    """C5's shape: half the frames VLAN-tagged, about 40 % IPv6; the IPv4 half
    is routed by fcgpu_set_routes' table with CLS_ROUTE's meaning of dst_ip."""
    from fastclick_amd import device as D
    routes6 = _sparse()
    routes4 = [(_mask(A4, p, 32), p, (9 << 24) | (9 << 16) | (p << 8) | 1, p % 5) for p in range(1, 33)]
    rng = np.random.default_rng(64)
    is6, tagged = rng.random(N_PKT) < 0.4, rng.random(N_PKT) < 0.5
    flen = np.where(is6, 80, 60) + np.where(tagged, 4, 0)
    hdr = synth.build_headers(N_PKT, src=rng.integers(1 << 24, 2**32, N_PKT, dtype=np.uint64),
                              dst=np.array(_dests(routes4, N_PKT, 65, 32), np.uint64)[rng.permutation(N_PKT)],
                              sport=rng.integers(0, 65536, N_PKT), dport=rng.integers(0, 65536, N_PKT), frame_len=flen,
                              vlan_tci=np.where(tagged, rng.integers(0, 4096, N_PKT), -1),
                              ip6=dict(mask=is6, src=rng.integers(0, 256, (N_PKT, 16)),
                                       dst=_bytes16(_dests(routes6, N_PKT, 66))[rng.permutation(N_PKT)]))
    b = synth.pack(hdr, flen)
    synth.inject_errors(b, 0.01, seed=67)
    cfg = N.make_cfg(check_mode=N.CHECK_AUTO, checksum=True, classify=N.CLS_ROUTE6, nports=5)
    exp = _expect(oracle, cfg, b, routes6, routes4)
    v = np.isin(exp["reason"], (N.R_OK, N.R_NO_MATCH))
    assert (exp["reason"] == N.R_NO_MATCH).any() and {4, 6} <= set(exp["anno"]["ipver"][exp["reason"] == N.R_OK])
    got = D.process_batch(b, cfg, partition=N.PART_TILE, routes=_native(routes4, 32), routes6=_native(routes6))
    _check(got, exp, N.PART_TILE)
    assert np.array_equal(got["anno"]["ipver"][v], exp["anno"]["ipver"][v])


@pytest.mark.gpu
def test_gpu_route6_replace_table_and_errors(oracle):
    """One context, three tables in turn (the empty one included); no IPv6
    table, an output >= nports and CLS_ROUTE6 under CHECK_IP4 are refused."""
    import torch
    from fastclick_amd import device as D
    cfg = N.make_cfg(check_mode=N.CHECK_AUTO, checksum=True, classify=N.CLS_ROUTE6, nports=7)
    ctx = N.Context(0, N_PKT, cfg)
    try:
        with pytest.raises(RuntimeError, match="fcgpu_set_routes6"):
            D.run_device(ctx, D.DeviceBatch.upload(synth.c5(300, seed=1)), D.DeviceOutputs(300, 7))
        with pytest.raises(RuntimeError, match="OUTPUT"):
            ctx.set_routes6(_native([(DB8, 32, 0, 7)]))
        for k, name in enumerate(("nested-nodefault", "hops600", None)):
            routes = _case(name)[0] if name else []
            ctx.set_routes6(_native(routes))
            ctx.reset_counters()
            b = _case(name or "sparse")[2]
            outs = D.DeviceOutputs(b.n, 7, anno=True, perm=True, port_start=True)
            D.run_device(ctx, D.DeviceBatch.upload(b), outs)
            torch.cuda.synchronize()
            got = dict(outs.numpy(), counters=ctx.counters())
            _check(got, _expect(oracle, cfg, b, routes), N.PART_GLOBAL, f"table {k}: ")
        with pytest.raises(RuntimeError, match="CHECK_AUTO and MARK_IP6 only"):
            ctx.configure(N.make_cfg(check_mode=N.CHECK_IP4, classify=N.CLS_ROUTE6, nports=7))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", TABLES)
def test_route6_lookup_matches_scan(name):
    routes, nports, _ = _case(name)
    keys = _dests(routes, N_PKT, seed=len(name) + 1)[::5]
    win, gid = _scan(routes, keys)
    arr = N.routes6_array(_native(routes))
    got = [N.route6_lookup(arr, k.to_bytes(16, "big"), nports) for k in keys]
    assert got == [(routes[i][3], int(gid[i])) if i >= 0 else (-1, 0) for i in win]
    if name in NO_DEFAULT:
        assert -1 in win


def test_route6_strings_and_stats():
    r = [("::", 0, None, 0), ("2001:db8::1", 128, "fe80::1", 1)]
    assert N.route6_lookup(r, "2001:db8::1") == (1, 1) and N.route6_lookup(r, "2001:db8::2") == (0, 0)
    assert N.route6_stats(r) == (1, 2)                    # one compressed chunk under the default
    assert N.route6_stats(_native(_nested(0)))[1] == 15   # a route ending at every byte: root + 14 chunks
    sparse = _sparse()
    assert N.route6_stats(_native(sparse))[0] < 2 * len(sparse)   # path compression: not a chunk per byte


def test_route6_table_errors():
    for routes, nports, msg in (([("::", 129, 0, 0)], 2, "prefix length"), ([("::", 0, 0, 2)], 2, "OUTPUT")):
        with pytest.raises(ValueError, match=msg):
            N.route6_lookup(routes, "::1", nports)
    many = np.zeros(32768, N.route6_dtype())
    many["plen"], many["addr"][:, 0], many["addr"][:, 1] = 16, np.arange(32768) >> 8, np.arange(32768) & 255
    many["gw"][:, 0], many["gw"][:, 14:] = 0xfe, many["addr"][:, :2]     # 32768 distinct gateways
    with pytest.raises(ValueError, match="32767 next hops"):
        N.route6_lookup(many, "::1")


EL6 = "2001:db8::/32 0, 2001:db8:7::/48 fe80::1 1, 2001:db8:7:9::/64 - 2, 2001:db8::1:2/32 fe80::2 3, ::/0 fe80::1 0"
EL6_ROUTES = [(DB8, 32, 0, 0), (DB8 | 7 << 80, 48, (0xfe80 << 112) | 1, 1), (DB8 | 7 << 80 | 9 << 64, 64, 0, 2),
              (DB8, 32, (0xfe80 << 112) | 2, 3), (0, 0, (0xfe80 << 112) | 1, 0)]
EL4 = "77.0.0.0/8 9.9.9.1 4, 77.141.0.0/16 1"
EL4_ROUTES = [(77 << 24, 8, (9 << 24) | (9 << 16) | (9 << 8) | 1, 4), ((77 << 24) | (141 << 16), 16, 0, 1)]


def test_element_routes6_config():
    """ROUTES6 implies CLS_ROUTE6; N defaults to the largest OUT + 1 over both lists."""
    from fastclick_amd import click as K
    c = K.element_cfg(f'GPUIPCheckClassify(MODE AUTO, ROUTES6 "{EL6}")')
    assert (c.classify, c.nports, c.check_mode) == (N.CLS_ROUTE6, 4, N.CHECK_AUTO)
    assert K.element_cfg(f'GPUIPCheckClassify(MODE AUTO, ROUTES "{EL4}", ROUTES6 "{EL6}")').nports == 5
    assert K.element_cfg(f'GPUIPCheckClassify(MODE MARK6, OFFSET 14, N 9, ROUTES6 "{EL6}")').nports == 9
    for bad, msg in ((f'MODE AUTO, ROUTES6 "{EL6}", LB_MODE hash', "conflicts"), (f'MODE AUTO, ROUTES6 "{EL6}", N 3', "OUTPUT"),
                     (f'OFFSET 14, ROUTES6 "{EL6}"', "MODE AUTO or MARK6"), ('MODE AUTO, ROUTES6 "2001:db8::/129 0"', "0..128"),
                     (f'MODE MARK6, ROUTES "{EL4}", ROUTES6 "{EL6}"', "dual stack"), ('MODE AUTO, ROUTES6 "::/0 x 0"', "GATEWAY"),
                     (f'MODE AUTO, ROUTES "{EL4}"', "MODE CHECK or MARK")):
        with pytest.raises(K.ConfigError, match=msg):
            K.check_config(f"GPUIPCheckClassify({bad})")


@pytest.mark.gpu
def test_element_routes6_dual_stack(oracle):
    """ROUTES + ROUTES6 through the element: per-output packets, the 16-byte
    DST_IP6 annotation (the gateway, else the packet's ip6_dst), DST_IP for
    the IPv4 half, no-route packets killed, and the `table6` handler."""
    from fastclick_amd import click as K
    rng = np.random.default_rng(96)
    is6 = rng.random(N_PKT) < 0.5
    d6 = _bytes16(_dests(EL6_ROUTES[:4], N_PKT, 97))[rng.permutation(N_PKT)]
    hdr = synth.build_headers(N_PKT, src=rng.integers(1 << 24, 2**32, N_PKT, dtype=np.uint64),
                              dst=np.array(_dests(EL4_ROUTES, N_PKT, 98, 32), np.uint64)[rng.permutation(N_PKT)],
                              sport=rng.integers(0, 65536, N_PKT), dport=rng.integers(0, 65536, N_PKT),
                              frame_len=np.where(is6, 80, 60),
                              ip6=dict(mask=is6, src=rng.integers(0, 256, (N_PKT, 16)), dst=d6))
    b = synth.pack(hdr, np.where(is6, 80, 60))
    synth.inject_errors(b, 0.01, seed=99)
    cfg = N.make_cfg(check_mode=N.CHECK_AUTO, checksum=True, classify=N.CLS_ROUTE6, nports=5)
    exp = _expect(oracle, cfg, b, EL6_ROUTES, EL4_ROUTES)
    r = K.run_element(f'GPUIPCheckClassify(MODE AUTO, CHECKSUM true, ROUTES "{EL4}", ROUTES6 "{EL6}")', b, nsinks=6)
    want = np.where(exp["reason"] == N.R_NO_MATCH, 0xFFFFFFFF, exp["port"].astype(np.uint32)).astype(np.uint32)
    assert (exp["reason"] == N.R_NO_MATCH).any() and np.array_equal(r["port"], want)
    ok, v6 = exp["reason"] == N.R_OK, exp["anno"]["ipver"] == 6
    gws = _bytes16([0, (0xfe80 << 112) | 1, (0xfe80 << 112) | 2])
    dst6 = np.where((exp["dst_ip"] > 0)[:, None], gws[np.where(v6, exp["dst_ip"], 0)], d6)
    assert set(exp["dst_ip"][ok & v6]) == {0, 1, 2}
    assert np.array_equal(r["dst6"][ok & v6], dst6[ok & v6])
    assert np.array_equal(r["dst"][ok & ~v6], exp["dst_ip"][ok & ~v6])
    assert r["handlers"]["table6"].rstrip("\n") == ("# Active routes\n2001:db8::/32\tfe80::2\t3\n2001:db8:7::/48\tfe80::1\t1\n"
                                                     "2001:db8:7:9::/64\t::\t2\n::/0\tfe80::1\t0")
