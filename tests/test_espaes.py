"""k_espaes (fcgpu_espaes_*) against a pure-Python AES-128 from FIPS 197 under the element's 8-byte-IV
chaining, applied to a copy of the arena with e0 / end from the oracle's annotations; the whole arena is
compared. The SA image is in LDS up to 16 KB = 85 records: 1 and 80 SAs take that branch, 2,000 the global one."""
import hashlib
import hmac

import numpy as np
import pytest

from fastclick_amd import synth
from fastclick_amd import _native as N

pytestmark = pytest.mark.gpu


def _xt(a):
    return (a << 1) ^ 0x11b if a & 0x80 else a << 1


def _mul(a, b):
    p = 0
    while b:
        p, a, b = p ^ (a if b & 1 else 0), _xt(a), b >> 1
    return p


_rl = lambda v, r: ((v << r) | (v >> (8 - r))) & 0xFF   # noqa: E731
_INV = [0] + [next(b for b in range(1, 256) if _mul(a, b) == 1) for a in range(1, 256)]
SBOX = [v ^ _rl(v, 1) ^ _rl(v, 2) ^ _rl(v, 3) ^ _rl(v, 4) ^ 0x63 for v in _INV]
ISBOX = [SBOX.index(v) for v in range(256)]
MUL = {k: [_mul(x, k) for x in range(256)] for k in (1, 2, 3, 9, 11, 13, 14)}


def expand(key):
    w, rcon = list(key), 1
    for i in range(4, 44):
        t = w[-4:]
        if i % 4 == 0:
            t, rcon = [SBOX[t[1]] ^ rcon, SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]], _xt(rcon)
        w += [w[-16 + b] ^ t[b] for b in range(4)]
    return w


def _mix(s, co):                                 # state byte (row q, column c) at s[4c + q]
    m = [MUL[k] for k in co]
    return [m[0][s[c + q]] ^ m[1][s[c + (q + 1) % 4]] ^ m[2][s[c + (q + 2) % 4]] ^ m[3][s[c + (q + 3) % 4]]
            for c in (0, 4, 8, 12) for q in range(4)]


def encrypt(w, blk):
    s = [a ^ b for a, b in zip(blk, w[:16])]
    for r in range(1, 11):
        s = [SBOX[s[4 * ((c + q) % 4) + q]] for c in range(4) for q in range(4)]
        s = [a ^ b for a, b in zip(_mix(s, (2, 3, 1, 1)) if r < 10 else s, w[16 * r:16 * r + 16])]
    return bytes(s)


def decrypt(w, blk):
    s = [a ^ b for a, b in zip(blk, w[160:])]
    for r in range(9, -1, -1):
        s = [ISBOX[s[4 * ((c - q) % 4) + q]] ^ w[16 * r + 4 * c + q] for c in range(4) for q in range(4)]
        s = _mix(s, (14, 11, 13, 9)) if r else s
    return bytes(s)


_C1 = [bytes.fromhex(h) for h in ("000102030405060708090a0b0c0d0e0f", "00112233445566778899aabbccddeeff",
                                   "69c4e0d86a7b0430d8cdb78070b4c55a")]
assert encrypt(expand(_C1[0]), _C1[1]) == _C1[2] and decrypt(expand(_C1[0]), _C1[2]) == _C1[1]   # FIPS 197 C.1

KEYS = [bytes((13 * k + 3 * j + 1) & 0xFF for j in range(16)) for k in range(4)]
AKEYS = [bytes((7 * k + j) & 0xFF for j in range(16)) for k in range(4)]
SAS = [(0x1000 + 0x101 * k, KEYS[k]) for k in range(4)]
CFG = dict(check_mode=N.CHECK_IP4, offset=14, checksum=False)


def _chain(arena, o, nblk, w, fn):
    """The element's chaining (first 8 bytes only) over nblk blocks from arena offset o, in place."""
    prev = bytes(arena[o - 8:o])
    for a in range(o, o + 16 * nblk, 16):
        c = bytes(arena[a:a + 16])
        if fn is decrypt:
            p = bytearray(decrypt(w, c))
            p[:8], prev = bytes(x ^ y for x, y in zip(p[:8], prev)), c[:8]
        else:
            p = encrypt(w, bytes(x ^ y for x, y in zip(c[:8], prev)) + c[8:])
            prev = p[:8]
        arena[a:a + 16] = np.frombuffer(bytes(p), np.uint8)


def _expect(b, e, sas, fn=decrypt):
    """(status per packet, blocks, the arena after the stage) by the rule of include/fastclick_gpu.h."""
    ws = {spi: expand(k) for spi, k in sas}
    st, arena, blocks = np.zeros(b.n, np.uint8), b.arena.copy(), 0
    for i in range(b.n):
        off, an = int(b.desc[i, 0]), e["anno"][i]
        nh, end = int(an["nh"]), int(an["length"])
        if e["reason"][i] != N.R_OK or an["ipver"] != 4 or b.arena[off + nh + 9] != 50:
            continue
        e0 = nh + 4 * (int(b.arena[off + nh]) & 15)
        w, plen = ws.get(int.from_bytes(bytes(b.arena[off + e0:off + e0 + 4]), "big")), end - e0 - 28
        st[i] = N.ESP_SHORT if plen < 0 else N.ESP_NO_SA if w is None else N.ESP_UNALIGNED if plen % 8 else N.ESP_OK
        if st[i] == N.ESP_OK:
            _chain(arena, off + e0 + 16, (plen + 8) // 16, w, fn)
            blocks += (plen + 8) // 16
    return st, blocks, arena


def _batch(elens, *, spi=SAS[0][0], proto=50, pad=0, seed=1):
    """ESP-in-IPv4 frames: 14 B Ethernet, 20 B IP, then elen seeded random bytes behind the SPI, pad bytes past ip_len."""
    elens = np.asarray(elens)
    n, flen = len(elens), 34 + elens
    hdr = synth.build_headers(n, src=0x0A000001, dst=0x0A000002, sport=0, dport=0, proto=proto, frame_len=flen, width=64)
    b = synth.pack(hdr, flen + pad)
    rng = np.random.default_rng(seed)
    spi = np.broadcast_to(np.asarray(spi, np.uint64), (n,))
    for i in range(n):
        o = int(b.desc[i, 0]) + 34
        b.arena[o:o + elens[i] + pad] = rng.integers(0, 256, elens[i] + pad, dtype=np.uint8)
        b.arena[o:o + 4] = synth._be32(spi[i:i + 1])[0]
    return b


def _run(ctx, b, *, null=False):
    import torch
    from fastclick_amd import device as D
    db = D.DeviceBatch.upload(b)
    D.run_device(ctx, db, D.DeviceOutputs(b.n, 1, verdict=not null, hash=True, anno=not null))
    torch.cuda.synchronize()
    return db.arena.cpu().numpy()


def _check(oracle, b, sas=SAS, *, null=False, ctx=None):
    cfg = N.make_cfg(**CFG)
    st, blocks, arena = _expect(b, oracle.process_batch(cfg, b), sas)
    own = ctx is None
    if own:
        ctx = N.Context(0, 1024, cfg)
        ctx.espaes_set_sas(sas)
    try:
        got = _run(ctx, b, null=null)
        assert ctx.espaes_status(b.n).tolist() == st.tolist()
        assert np.array_equal(got, arena), np.nonzero(got != arena)[0][:8]
        if own:
            c = np.bincount(st, minlength=6)
            assert ctx.espaes_stats() == dict(ok=c[1], no_sa=c[3], too_short=c[4], unaligned=c[5], not_esp=c[0], blocks=blocks)
    finally:
        if own:
            ctx.close()
    return st, blocks


def test_gpu_espaes_lengths(oracle):
    """SHORT, 0 blocks, 1 block over 8 digest bytes, 1-3 blocks, UNALIGNED, a 1500-B frame at plen % 16 = 8, 0."""
    st, _ = _check(oracle, _batch([27, 28, 36, 44, 52, 60, 76, 29, 33, 1460, 1452]), SAS[:1])
    assert st.tolist() == [N.ESP_SHORT] + [N.ESP_OK] * 6 + [N.ESP_UNALIGNED] * 2 + [N.ESP_OK] * 2


@pytest.mark.parametrize("ihl,tables,replicas", [(5, "1", "1"), (6, "1", "1"), (5, "4", "4"), (6, "1", "2")])
def test_gpu_espaes_alignment(oracle, ihl, tables, replicas, monkeypatch):
    """One 5-block frame back to back with no gap, 18 times: an odd length walks all 16 alignments, every
    neighbour is an OK packet, the odd byte past ip_len is nobody's. Default and other table layouts."""
    monkeypatch.setenv("FCGPU_ESPAES_TABLES", tables)
    monkeypatch.setenv("FCGPU_ESPAES_REPLICAS", replicas)
    f = bytearray(_batch([100], pad=1).frame(0))
    if ihl == 6:
        f[14] = 0x46
        f[34:34] = b"\x01" * 4
        f[16:18] = (len(f) - 15).to_bytes(2, "big")
    arena = np.zeros(16 + 18 * len(f) + synth.ARENA_PAD, np.uint8)
    desc = np.array([[16 + k * len(f), len(f)] for k in range(18)], np.uint32)
    assert len(f) % 2 == 1 and len(set((desc[:, 0] % 16).tolist())) == 16
    for o in desc[:, 0]:
        arena[o:o + len(f)] = np.frombuffer(bytes(f), np.uint8)
    st, blocks = _check(oracle, synth.Batch(arena=arena, desc=desc), SAS[:1])
    assert (st == N.ESP_OK).all() and blocks == 18 * 5


def _mixed(n, seed=3):
    """nblk over {0, 1, 2, 5, 91} (odd packets 8 mod 16), four SAs, unknown SPIs, UDP, bad versions, 6 bytes of
    padding past ip_len that anno.length trims."""
    i = np.arange(n)
    nblk = np.asarray((0, 1, 2, 5, 91))[i % 5]
    elens = 28 + 16 * nblk - 8 * ((i % 2 == 1) & (nblk > 0))
    spi = np.where(i % 7 == 6, 0xDEAD0000 + i, np.asarray([s for s, _ in SAS])[i % 4])
    b = _batch(elens, spi=spi, proto=np.where(i % 11 == 10, 17, 50), pad=6, seed=seed)
    b.desc[:, 1] -= (6 * (i % 5 != 4)).astype(np.uint32)
    b.arena[b.desc[i % 13 == 12, 0] + 14] = 0x55
    return b


@pytest.mark.parametrize("tile", ["256", "32"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 773])
def test_gpu_espaes_mixed_tile(oracle, n, tile, monkeypatch):
    """Chains across pass, wave and tile boundaries (some 20 passes a 256-packet tile, 91-block packets straddle
    them); 256-packet tiles and the 32 a small batch gets by default."""
    monkeypatch.setenv("FCGPU_ESPAES_TILE", tile)
    st, _ = _check(oracle, _mixed(n))
    if n == 773:
        assert set(st.tolist()) == {N.ESP_NOT_ESP, N.ESP_OK, N.ESP_NO_SA}


@pytest.mark.parametrize("nsa", [1, 80, 2000])
def test_gpu_espaes_sa_tables(oracle, nsa):
    """LDS images (1, 80 x 192 B) and the global one (2,000): first, middle and last SPI, and a miss."""
    sas = [(5 + 3 * k, hashlib.sha1(bytes([k & 255, k >> 8])).digest()[:16]) for k in range(nsa)][::-1]
    hit = [5, 5 + 3 * (nsa // 2), 5 + 3 * (nsa - 1), 6]
    st, _ = _check(oracle, _batch([108] * 4, spi=hit), sas)
    assert st.tolist() == [N.ESP_OK] * 3 + [N.ESP_NO_SA]


def test_gpu_espaes_chain_with_espauth(oracle):
    """Outbound-style packets (HMAC over plaintext [e0, end - 12), then the element's encryption) verify with both
    stages; one flipped ciphertext bit is BAD; with espauth alone every packet is BAD."""
    asas = [(s, AKEYS[k]) for k, (s, _) in enumerate(SAS)]
    n = 40
    b = _batch(36 + 8 * (np.arange(n) % 11), spi=np.asarray([s for s, _ in SAS])[np.arange(n) % 4])
    e = oracle.process_batch(N.make_cfg(**CFG), b)
    want = np.zeros((n, 12), np.uint8)
    for i in range(n):
        o, end = int(b.desc[i, 0]), int(b.desc[i, 0]) + int(e["anno"][i]["length"])
        want[i] = np.frombuffer(hmac.new(AKEYS[i % 4], bytes(b.arena[o + 34:end - 12]), hashlib.sha1).digest()[:12], np.uint8)
        b.arena[end - 12:end] = want[i]
    plain = b.arena.copy()
    b.arena = _expect(b, e, SAS, encrypt)[2]
    b.arena[int(b.desc[n - 1, 0]) + 34 + 16 + 3] ^= 0x10          # the last packet: one ciphertext bit
    ctx = N.Context(0, 1024, N.make_cfg(**CFG))
    try:
        ctx.espauth_set_sas(asas)
        _run(ctx, b)
        assert (ctx.espauth_records(n)["status"] == N.ESP_BAD).all()
        ctx.espaes_set_sas(SAS)
        got = _run(ctx, b)
        rec = ctx.espauth_records(n)
        assert rec["status"].tolist() == [N.ESP_OK] * (n - 1) + [N.ESP_BAD]
        lo = int(b.desc[n - 1, 0])
        assert np.array_equal(got[:lo], plain[:lo]) and np.array_equal(rec["icv"][:n - 1], want[:n - 1])
    finally:
        ctx.close()


def test_gpu_espaes_replacement_stats_null_outputs_refusals(oracle):
    """Table replacement, statistics over two batches and reset, NULL verdict / anno outputs, set_sas and
    entry-point refusals; after set_sas([]) the other paths work and the arena is not written."""
    import torch
    from fastclick_amd import device as D
    ctx = N.Context(0, 1024, N.make_cfg(**CFG))
    try:
        ctx.espaes_set_sas(SAS)
        (a, ba), (b, bb) = _check(oracle, _mixed(100), ctx=ctx), _check(oracle, _mixed(65, seed=4), ctx=ctx, null=True)
        c = np.bincount(np.concatenate([a, b]), minlength=6)
        assert ctx.espaes_stats() == dict(ok=c[1], no_sa=c[3], too_short=c[4], unaligned=c[5], not_esp=c[0], blocks=ba + bb)
        ctx.espaes_reset()
        assert not any(ctx.espaes_stats().values())
        for bad, msg in ([(0, KEYS[0])], "SPI 0"), (SAS + SAS[1:2], "duplicate"), ([(1, KEYS[0])] * 65537, "65536"):
            with pytest.raises(RuntimeError, match=msg):
                ctx.espaes_set_sas(bad)
        ctx.espaes_set_sas(SAS[2:])
        st, _ = _check(oracle, _mixed(100), SAS[2:], ctx=ctx)
        assert (st == N.ESP_NO_SA).sum() > (a == N.ESP_NO_SA).sum() and ctx.espaes_stats()["ok"] == (st == N.ESP_OK).sum()
        s = _batch([108] * 8)
        db, o = D.DeviceBatch.upload(s), D.DeviceOutputs(s.n, 1)
        jobs = ctx.jobs([(db.arena.data_ptr(), db.desc.data_ptr(), db.n, 0, o.ptrs())])
        pin = [torch.from_numpy(x).pin_memory() for x in (s.arena, s.desc.view(np.int32), np.zeros(s.n, np.int16))]
        span = lambda: ctx.span_submit(0, pin[0].data_ptr(), s.arena.size, pin[1].data_ptr(), s.n,  # noqa: E731
                                       verdict=pin[2].data_ptr())
        for call in (lambda: ctx.run_jobs(jobs), span):
            with pytest.raises(RuntimeError, match="ESP decryption"):
                call()
        ctx.espaes_set_sas([])
        ctx.run_jobs(jobs)
        torch.cuda.synchronize()
        span()
        ctx.span_wait(0)
        assert (pin[2].numpy().view(np.uint16) & 0xFF == N.R_OK).all() and not ctx.espaes_status_ptr()
        assert np.array_equal(db.arena.cpu().numpy(), s.arena)        # stage off: the arena is not written
    finally:
        ctx.close()
