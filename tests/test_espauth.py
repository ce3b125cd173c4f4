"""ESP authentication on the device (fcgpu_espauth_*, k_espauth behind k_rx)
against Python's own hmac.new(key, data, hashlib.sha1).digest()[:12], applied
to bytes sliced from the same arena by the rule of include/fastclick_gpu.h
with e0 and end from the oracle's annotations for the batch. No second SHA-1
is written here.

Padding boundaries: L = 4 and 5 stay in the list of authenticated lengths,
but elen = L + 12 < 28 makes them SHORT packets by the stage's semantics (no
digest); 16 and 17 are the shortest that hash."""
import hashlib
import hmac

import numpy as np
import pytest

from fastclick_amd import synth
from fastclick_amd import _native as N

pytestmark = pytest.mark.gpu
KEYS = [bytes((7 * k + j) & 0xFF for j in range(16)) for k in range(4)]
SAS = [(0x1000 + 0x101 * k, KEYS[k]) for k in range(4)]


def _batch(elens, *, spi=SAS[0][0], proto=50, pad=0, seed=1):
    """ESP-in-IPv4 frames: 14 B Ethernet, 20 B IP, then elen bytes: the SPI,
    seeded random payload and 12 bytes for the digest (_sign fills them)."""
    elens = np.asarray(elens)
    n = len(elens)
    flen = 34 + elens
    hdr = synth.build_headers(n, src=0x0A000001, dst=0x0A000002, sport=0, dport=0, proto=proto, frame_len=flen, width=64)
    b = synth.pack(hdr, flen + pad)
    rng = np.random.default_rng(seed)
    spi = np.broadcast_to(np.asarray(spi, np.uint64), (n,))
    for i in range(n):
        o = int(b.desc[i, 0]) + 34
        b.arena[o:o + elens[i] + pad] = rng.integers(0, 256, elens[i] + pad, dtype=np.uint8)
        b.arena[o:o + 4] = synth._be32(spi[i:i + 1])[0][:min(4, elens[i])]
    return b


def _expect(b, e, sas, mode):
    """(status, icv) per packet from the oracle's outputs and hmac."""
    keys = dict(sas)
    st, icv = np.zeros(b.n, np.uint8), np.zeros((b.n, 12), np.uint8)
    for i in range(b.n):
        off, an = int(b.desc[i, 0]), e["anno"][i]
        nh, end = int(an["nh"]), int(an["length"])
        if e["reason"][i] != N.R_OK or an["ipver"] != 4 or b.arena[off + nh + 9] != 50:
            continue
        e0 = nh + 4 * (int(b.arena[off + nh]) & 15)
        key = keys.get(int.from_bytes(bytes(b.arena[off + e0:off + e0 + 4]), "big"))
        if end - e0 < 28:
            st[i] = N.ESP_SHORT
        elif key is None:
            st[i] = N.ESP_NO_SA
        else:
            stop = end if mode == N.ESP_COMPUTE else end - 12
            d = hmac.new(key, bytes(b.arena[off + e0:off + stop]), hashlib.sha1).digest()[:12]
            icv[i] = np.frombuffer(d, np.uint8)
            st[i] = N.ESP_OK if mode == N.ESP_COMPUTE or bytes(b.arena[off + stop:off + end]) == d else N.ESP_BAD
    return st, icv


def _sign(b, e, sas):
    """Write the right digest into every frame that has an SA (VERIFY)."""
    st, icv = _expect(b, e, sas, N.ESP_VERIFY)
    for i in np.nonzero(st >= N.ESP_OK)[0]:
        if st[i] in (N.ESP_OK, N.ESP_BAD):
            end = int(b.desc[i, 0]) + int(e["anno"][i]["length"])
            b.arena[end - 12:end] = icv[i]


CFG = dict(check_mode=N.CHECK_IP4, offset=14, checksum=False)


def _run(ctx, b, *, null=False):
    import torch
    from fastclick_amd import device as D
    db = D.DeviceBatch.upload(b)
    D.run_device(ctx, db, D.DeviceOutputs(b.n, 1, verdict=not null, hash=True, anno=not null))
    torch.cuda.synchronize()
    return ctx.espauth_records(b.n)


def _check(oracle, b, sas=SAS, mode=N.ESP_VERIFY, *, sign=True, null=False, ctx=None):
    cfg = N.make_cfg(**CFG)
    e = oracle.process_batch(cfg, b)
    if sign:
        _sign(b, e, sas)
    st, icv = _expect(b, e, sas, mode)
    own = ctx is None
    if own:
        ctx = N.Context(0, 1024, cfg)
        ctx.espauth_set_sas(sas)
        ctx.espauth_configure(mode)
    try:
        rec = _run(ctx, b, null=null)
    finally:
        if own:
            ctx.close()
    assert rec["status"].tolist() == st.tolist()
    assert np.array_equal(rec["icv"], icv) and not rec["pad"].any()
    return st


LS = [4, 5, 16, 17, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 128] + list(range(144, 1455, 16)) + [1454]


def test_gpu_espauth_padding_boundaries(oracle):
    """Every authenticated length around the one- and two-block paddings, up
    to a 1500-B frame, in one batch (the lanes of a wave then end at
    different steps)."""
    st = _check(oracle, _batch(np.asarray(LS) + 12), SAS[:1])
    assert st.tolist() == [N.ESP_SHORT] * 2 + [N.ESP_OK] * (len(LS) - 2)


@pytest.mark.parametrize("ihl", [5, 6])
def test_gpu_espauth_alignment(oracle, ihl):
    """One 3-block frame at all 16 arena alignments, without and with IP options."""
    one = _batch([150 + 12])
    f = bytearray(one.frame(0))
    if ihl == 6:
        f[14] = 0x46
        f[34:34] = b"\x01" * 4
        f[16:18] = (len(f) - 14).to_bytes(2, "big")
    arena = np.zeros(16 * 512 + synth.ARENA_PAD, np.uint8)
    desc = np.array([[512 * a + 64 + a, len(f)] for a in range(16)], np.uint32)
    for o in desc[:, 0]:
        arena[o:o + len(f)] = np.frombuffer(bytes(f), np.uint8)
    st = _check(oracle, synth.Batch(arena=arena, desc=desc), SAS[:1])
    assert (st == N.ESP_OK).all()


FLIPS = [0, 149, 40, 100] + list(range(150, 162))      # first, last, one per 64-B block, each digest byte


def test_gpu_espauth_tampering(oracle):
    """One flipped bit anywhere in the message or the digest is BAD; the
    untouched frame, whose 12 digest bytes are the first 12 of the 20-byte
    HMAC, is OK (truncation). The first message byte is the SPI's: the
    flipped SPI names a second SA with the same key, so the digest decides."""
    sas = [SAS[0], (SAS[0][0] ^ 0x01000000, KEYS[0])]
    b = _batch([150 + 12] * (len(FLIPS) + 1))
    _sign(b, oracle.process_batch(N.make_cfg(**CFG), b), sas)
    for i, at in enumerate(FLIPS):
        b.arena[int(b.desc[i, 0]) + 34 + at] ^= 1 << (i % 8)
    st = _check(oracle, b, sas, sign=False)
    assert st.tolist() == [N.ESP_BAD] * len(FLIPS) + [N.ESP_OK]


def _mixed(n, seed=3):
    i = np.arange(n)
    elens = np.asarray((60, 64, 65, 257, 1500))[i % 5] - 34
    if n > 100:
        elens[100] = 27
    spi = np.where(i % 7 == 6, 0xDEAD0000 + i, np.asarray([s for s, _ in SAS])[i % 4])
    b = _batch(elens - 6 * (i % 5 == 4), spi=spi, proto=np.where(i % 11 == 10, 17, 50), pad=6, seed=seed)
    b.desc[:, 1] -= (6 * (i % 5 != 4)).astype(np.uint32)          # every 5th keeps 6 bytes of padding past ip_len
    b.arena[b.desc[i % 13 == 12, 0] + 14] = 0x55
    return b


@pytest.mark.parametrize("order", ["1", "0"])
@pytest.mark.parametrize("n,mode", [(1, 0), (255, 0), (256, 0), (257, 0), (773, 0), (773, 1)])
def test_gpu_espauth_mixed_tile(oracle, n, mode, order, monkeypatch):
    """Mixed lengths, four SAs, unknown SPIs, UDP, bad versions, trimmed
    padding and one short packet, with the tiles ordered by block count and in
    arrival order; VERIFY and COMPUTE; the statistics count every packet."""
    monkeypatch.setenv("FCGPU_ESPAUTH_ORDER", order)
    st = _check(oracle, _mixed(n), mode=mode)
    if n == 773:
        assert set(st.tolist()) == {N.ESP_NOT_ESP, N.ESP_OK, N.ESP_NO_SA, N.ESP_SHORT}


@pytest.mark.parametrize("nsa", [1, 300, 2000])
def test_gpu_espauth_sa_tables(oracle, nsa):
    """One SA, the LDS image (300 x 48 B) and the global one (2,000): the
    first, a middle and the last SPI of the sorted table, and a miss."""
    sas = [(5 + 3 * k, hashlib.sha1(bytes([k & 255, k >> 8])).digest()[:16]) for k in range(nsa)][::-1]
    hit = [5, 5 + 3 * (nsa // 2), 5 + 3 * (nsa - 1), 6]
    st = _check(oracle, _batch([100] * 4, spi=hit), sas)
    assert st.tolist() == [N.ESP_OK] * 3 + [N.ESP_NO_SA]


def test_gpu_espauth_replacement_stats_null_outputs(oracle):
    """The table is replaced between batches; statistics accumulate over
    batches and reset; verdict / anno NULL outputs use context scratch."""
    cfg = N.make_cfg(**CFG)
    ctx = N.Context(0, 1024, cfg)
    try:
        ctx.espauth_set_sas(SAS)
        a = _check(oracle, _mixed(300), ctx=ctx)
        b = _check(oracle, _mixed(257, seed=4), ctx=ctx, null=True)
        both = np.bincount(np.concatenate([a, b]), minlength=5)
        assert ctx.espauth_stats() == dict(not_esp=both[0], ok=both[1], bad=both[2], no_sa=both[3], too_short=both[4])
        ctx.espauth_reset()
        assert not any(ctx.espauth_stats().values())
        ctx.espauth_set_sas(SAS[2:])
        c = _check(oracle, _mixed(300), SAS[2:], ctx=ctx)
        assert (c == N.ESP_NO_SA).sum() > (a == N.ESP_NO_SA).sum() and ctx.espauth_stats()["ok"] == (c == N.ESP_OK).sum()
    finally:
        ctx.close()


def test_gpu_espauth_refusals():
    """set_sas refuses SPI 0, duplicates and more than 65,536 SAs and keeps
    the installed table; fcgpu_process_jobs and the span path refuse while
    SAs are installed and work again after set_sas([])."""
    import torch
    from fastclick_amd import device as D
    b = _batch([100] * 8)
    ctx = N.Context(0, 1024, N.make_cfg(**CFG))
    try:
        ctx.espauth_set_sas(SAS)
        for bad, msg in ([(0, KEYS[0])], "SPI 0"), (SAS + SAS[1:2], "duplicate"), ([(1, KEYS[0])] * 65537, "65536"):
            with pytest.raises(RuntimeError, match=msg):
                ctx.espauth_set_sas(bad)
        assert ctx.espauth_records_ptr()
        db, o = D.DeviceBatch.upload(b), D.DeviceOutputs(b.n, 1)
        jobs = ctx.jobs([(db.arena.data_ptr(), db.desc.data_ptr(), db.n, 0, o.ptrs())])
        pin = [torch.from_numpy(x).pin_memory() for x in (b.arena, b.desc.view(np.int32), np.zeros(b.n, np.int16))]
        span = lambda: ctx.span_submit(0, pin[0].data_ptr(), b.arena.size, pin[1].data_ptr(), b.n,  # noqa: E731
                                       verdict=pin[2].data_ptr())
        for call in (lambda: ctx.run_jobs(jobs), span):
            with pytest.raises(RuntimeError, match="ESP authentication"):
                call()
        ctx.espauth_set_sas([])
        ctx.run_jobs(jobs)
        torch.cuda.synchronize()
        span()
        ctx.span_wait(0)
        assert (pin[2].numpy().view(np.uint16) & 0xFF == N.R_OK).all() and not ctx.espauth_records_ptr()
    finally:
        ctx.close()
