"""AggregateCounter on the device (fcgpu_aggcount_*, k_aggcount behind k_rx)
against a dictionary filled from the oracle's own outputs for the same batch:
a packet counts iff the oracle's reason is R_OK, under key hash & mask, by 1,
anno.length or anno.length - anno.nh. No second table implementation here.

Zero counts: with bytes the amount is a frame's trimmed length, with ip_bytes
an IP datagram's length; neither is 0 for a packet that passed the checker, so
no case here yields a zero count and read()'s omission of them is not
exercised on the device (nnz == nagg in every case)."""
from collections import Counter

import numpy as np
import pytest

from fastclick_amd import synth
from fastclick_amd import _native as N

LENGTHS = (60, 64, 65, 257, 1500)
NOMATCH = -2147483647
# IPClassifier(udp && dst port even): odd destination ports match no output
PROG = (N.PROG_IPFILTER, [(256 + 8, 17 << 8, 0xff00, 1, NOMATCH, 0), (512, 0, 0x01000000, -1, NOMATCH, 0)], -1)


def _frames(n, flows, *, lens=(60,), first=0, v6=False):
    """n UDP frames over `flows` 5-tuples (numbered from `first`), interleaved,
    lengths cycling through lens; every 5th frame has 6 bytes of padding past
    ip_len, every 13th a bad IP version, every 17th an odd destination port
    (no match under PROG). v6: every 3rd frame IPv6, every other one tagged,
    no odd ports (CLS_NONE would count them as aggregates of their own)."""
    i = np.arange(n)
    f = first + i % flows
    L = np.asarray(lens)[i % len(lens)] + (30 if v6 else 0)
    tci = np.where(i % 2 == 1, 100 + f % 7, -1) if v6 else None
    a6 = np.zeros((2, n, 16), np.uint8)
    a6[:, :, 15], a6[:, :, 14], a6[1, :, 0] = f & 0xff, f >> 8, 0x20
    hdr = synth.build_headers(n, src=0x0A000000 + f, dst=0x0A800002, sport=1000 + f,
                              dport=2 * f + ((i % 17 == 16) & (not v6)), frame_len=L - 6 * (i % 5 == 4), vlan_tci=tci,
                              width=128 if v6 else 64, ip6=dict(mask=i % 3 == 2, src=a6[0], dst=a6[1]) if v6 else None)
    b = synth.pack(hdr, L)
    bad = (i % 13 == 12) & (i % 2 == 0 if v6 else True)
    b.arena[b.desc[bad, 0] + 14] = 0x55
    return b


def _expect(e, mask=0xFFFFFFFF, mode=0):
    """{aggregate: count} and the number of R_OK packets, from oracle outputs."""
    ok = e["reason"] == N.R_OK
    an = e["anno"]
    amt = [np.ones(len(ok), np.int64), an["length"].astype(np.int64), an["length"].astype(np.int64) - an["nh"]][mode]
    d = {}
    for k, a in zip((e["hash"][ok] & np.uint32(mask)).tolist(), amt[ok].tolist()):
        d[k] = d.get(k, 0) + a
    return d, int(ok.sum())


def _read(ctx):
    aggs, counts = ctx.aggcount_read()
    assert np.all(np.diff(aggs.astype(np.int64)) > 0) and np.all(counts > 0)
    return dict(zip(aggs.tolist(), counts.tolist()))


def _run(ctx, b, *, null=False, anno=True):
    import torch
    from fastclick_amd import device as D
    db = D.DeviceBatch.upload(b)
    outs = D.DeviceOutputs(b.n, ctx.cfg.nports, verdict=not null, hash=not null, anno=anno and not null)
    D.run_device(ctx, db, outs)
    torch.cuda.synchronize()


def _cfg(classify=N.CLS_PROGRAM, check_mode=N.CHECK_IP4, **kw):
    return N.make_cfg(check_mode=check_mode, offset=0 if check_mode == N.CHECK_AUTO else 14, checksum=True, classify=classify,
                      nports=2 if classify == N.CLS_PROGRAM else 1, **kw)


def _oracle(oracle, cfg, b):
    prog = PROG if cfg.classify == N.CLS_PROGRAM else None
    if prog:
        oracle.set_program(*prog)
    return oracle.process_batch(cfg, b, program=prog)


def _ctx(cfg, capacity, **kw):
    ctx = N.Context(0, 1024, cfg)
    if cfg.classify == N.CLS_PROGRAM:
        ctx.set_program(*PROG)
    ctx.aggcount_configure(capacity, **kw)
    return ctx


SHAPES = {"one": (1, 64, 0xFFFFFFFF), "distinct": (1 << 20, 1024, 0xFFFFFFFF), "eight": (8, 64, 0xFFFFFFFF),
          "chain": (1 << 20, 8, 0x7)}    # flows (capped at n), capacity, mask
CASES = [pytest.param(n, s, 0, False, False, id=f"{s}-n{n}") for s in SHAPES for n in (1, 255, 256, 257, 3 * 256 + 5)] + \
        [pytest.param(773, "eight", 1, False, False, id="bytes"), pytest.param(773, "distinct", 2, False, False, id="ip_bytes"),
         pytest.param(773, "eight", 2, True, False, id="ip_bytes-auto6"), pytest.param(773, "eight", 0, False, True, id="null-outputs"),
         pytest.param(773, "distinct", 2, False, True, id="null-outputs-ip_bytes")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape,mode,v6,null", CASES)
def test_gpu_aggcount_matches_dictionary(oracle, n, shape, mode, v6, null):
    flows, cap, mask = SHAPES[shape]
    b = _frames(n, min(flows, n), lens=LENGTHS if mode else (60,), v6=v6)
    cfg = _cfg(N.CLS_NONE, N.CHECK_AUTO) if v6 else _cfg()
    e = _oracle(oracle, cfg, b)
    exp, seen = _expect(e, mask, mode)
    if n > 256:     # the batch has what it is meant to have
        assert (e["reason"] == N.R_BAD_VERSION).any() and (v6 or (e["reason"] == N.R_NO_MATCH).any())
        assert len(exp) == {"one": 1, "eight": 16 if v6 else 8, "chain": 8}.get(shape, len(exp))     # v6: 8 IPv4 + 8 IPv6
        assert shape != "distinct" or len(exp) == seen
        assert not mode or (e["anno"]["length"] != b.desc[:, 1])[e["reason"] == N.R_OK].any()
        assert not v6 or {14, 18} <= set(e["anno"]["nh"][e["reason"] == N.R_OK].tolist())
        assert shape != "chain" or 0 in exp
    ctx = _ctx(cfg, cap, bytes=mode > 0, ip_bytes=mode == 2, mask=mask)
    try:
        _run(ctx, b, null=null)
        st = ctx.aggcount_stats()
        assert _read(ctx) == exp
        assert (st["nagg"], st["nnz"], st["seen"], st["uncounted"], st["count"], st["capacity"], st["frozen"]) == \
               (len(exp), len(exp), seen, 0, sum(exp.values()), cap, 0)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_aggcount_accumulates_freezes_resets(oracle):
    """Two batches accumulate; a frozen counter only grows the aggregates it
    has and reports the rest uncounted; reset forgets everything; two jobs of
    one fcgpu_process_jobs call count like two fcgpu_process calls."""
    import torch
    from fastclick_amd import device as D
    cfg = _cfg()
    A, B = _frames(700, 12), _frames(900, 20, first=6)      # B: flows 6..25, 6..11 old
    ea, eb = (_expect(_oracle(oracle, cfg, x)) for x in (A, B))
    ctx = _ctx(cfg, 64)
    try:
        _run(ctx, A)
        _run(ctx, B)
        assert _read(ctx) == dict(Counter(ea[0]) + Counter(eb[0])) and ctx.aggcount_stats()["nagg"] == 26
        ctx.aggcount_reset()
        st = ctx.aggcount_stats()
        assert _read(ctx) == {} and (st["nagg"], st["nnz"], st["count"], st["seen"]) == (0, 0, 0, 0)
        _run(ctx, A)
        ctx.aggcount_freeze(True)
        _run(ctx, B)
        old = {k: v for k, v in eb[0].items() if k in ea[0]}
        st = ctx.aggcount_stats()
        assert len(old) == 6 and _read(ctx) == dict(Counter(ea[0]) + Counter(old))
        assert (st["frozen"], st["nagg"], st["seen"]) == (1, 12, ea[1] + eb[1])
        assert st["uncounted"] == eb[1] - sum(old.values())
        ctx.aggcount_freeze(False)
        ctx.aggcount_reset()
        dbs = [D.DeviceBatch.upload(x) for x in (A, B)]
        outs = [D.DeviceOutputs(x.n, cfg.nports) for x in (A, B)]
        s = torch.cuda.current_stream().cuda_stream
        ctx.run_jobs(ctx.jobs([(d.arena.data_ptr(), d.desc.data_ptr(), d.n, s, o.ptrs()) for d, o in zip(dbs, outs)]))
        assert _read(ctx) == dict(Counter(ea[0]) + Counter(eb[0]))
        assert np.array_equal(outs[1].numpy()["hash"], _oracle(oracle, cfg, B)["hash"])
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flows", [8, 20])
def test_gpu_aggcount_capacity(oracle, flows):
    """capacity 8: with 8 aggregates nothing is refused; with 20 (several
    packets each, over four tiles) which 8 get a node depends on scheduling,
    but each is counted whole or not at all and the totals agree."""
    cfg = _cfg()
    b = _frames(3 * 256 + 5, flows)
    exp, seen = _expect(_oracle(oracle, cfg, b))
    ctx = _ctx(cfg, 8)
    try:
        _run(ctx, b)
        got, st = _read(ctx), ctx.aggcount_stats()
        assert len(exp) == flows and st["nagg"] == 8 and len(got) == 8
        assert all(exp[k] == v for k, v in got.items())
        assert sum(got.values()) == st["count"] and st["seen"] == seen
        assert st["seen"] - st["uncounted"] == sum(exp[k] for k in got)
        if flows == 8:
            assert st["uncounted"] == 0 and got == exp
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_aggcount_refusals():
    """HASH_NONE with the counter enabled, a capacity above the limit and the
    submission paths that do not serve the counter are refused; disabling it
    serves them again."""
    import torch
    from fastclick_amd import device as D
    b = _frames(300, 4)
    ctx = N.Context(0, 1024, _cfg(N.CLS_NONE))
    try:
        with pytest.raises(RuntimeError, match="capacity"):
            ctx.aggcount_configure(N.AGGCOUNT_MAX_CAPACITY + 1)
        with pytest.raises(RuntimeError, match="not enabled"):
            ctx.aggcount_freeze(True)
        ctx.aggcount_configure(16)
        db, o = D.DeviceBatch.upload(b), D.DeviceOutputs(b.n, 1, partition=N.PART_TILE)
        lens = np.ascontiguousarray(b.desc[:, 1])
        cnt = torch.tensor([4], dtype=torch.int32, device="cuda")
        refused = [
            lambda: ctx.process_counted(db.arena.data_ptr(), db.desc.data_ptr(), db.n, cnt.data_ptr(), **o.ptrs()),
            lambda: ctx.process_host((N.C.c_void_p * db.n)(), lens.ctypes.data, db.n, verdict=1),
            lambda: ctx.process_mbufs(lens.ctypes.data, db.n, verdict=1),
            lambda: ctx.span_submit(0, b.arena.ctypes.data, b.arena.size, b.desc.ctypes.data, db.n, verdict=1),
            lambda: ctx._chk(ctx.lib.fcgpu_span_submit_block(ctx.h, 0, b.arena.ctypes.data, b.arena.size, 0, 0, db.n,
                                                             b.arena.ctypes.data, 1, 0), "block"),
        ]
        for call in refused:
            with pytest.raises(RuntimeError, match="aggregate counter"):
                call()
        ctx.configure(_cfg(N.CLS_NONE, hash_mode=N.HASH_NONE))
        with pytest.raises(RuntimeError, match="HASH_NONE"):
            D.run_device(ctx, db, o)
        ctx.aggcount_configure(0)
        D.run_device(ctx, db, o)
        torch.cuda.synchronize()
        assert ctx.aggcount_stats()["capacity"] == 0 and len(ctx.aggcount_read()[0]) == 0
    finally:
        ctx.close()
