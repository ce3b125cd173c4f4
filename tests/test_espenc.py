"""k_espenc (fcgpu_espaes_configure(ENCRYPT)) and FCGPU_ESP_SEAL against tests/test_espaes.py's pure-Python AES-128 and
hmac/hashlib on a copy of the arena: whole arena, statuses, records, statistics. A wave serves 16 packets, a tile 64 or 256."""
import hashlib
import hmac

import numpy as np
import pytest

from fastclick_amd import synth
from fastclick_amd import _native as N
from tests.test_espaes import AKEYS, CFG, SAS, _batch, _expect, _mixed, _run, encrypt

pytestmark = pytest.mark.gpu
ASAS = [(s, AKEYS[k]) for k, (s, _) in enumerate(SAS)]
_REF = {}                                        # expectations of the mixed batches, computed once


def _seal(b, e, asas):
    """FCGPU_ESP_SEAL by the rule of include/fastclick_gpu.h: (status, icv per packet, the arena after it)."""
    keys, arena = dict(asas), b.arena.copy()
    st, icv = np.zeros(b.n, np.uint8), np.zeros((b.n, 12), np.uint8)
    for i in range(b.n):
        off, an = int(b.desc[i, 0]), e["anno"][i]
        nh, end = int(an["nh"]), int(an["length"])
        if e["reason"][i] != N.R_OK or an["ipver"] != 4 or b.arena[off + nh + 9] != 50:
            continue
        e0 = nh + 4 * (int(b.arena[off + nh]) & 15)
        key = keys.get(int.from_bytes(bytes(b.arena[off + e0:off + e0 + 4]), "big"))
        st[i] = N.ESP_SHORT if end - e0 < 28 else N.ESP_NO_SA if key is None else N.ESP_OK
        if st[i] == N.ESP_OK:
            icv[i] = np.frombuffer(hmac.new(key, bytes(b.arena[off + e0:off + end - 12]), hashlib.sha1).digest()[:12], np.uint8)
            arena[off + end - 12:off + end] = icv[i]
    return st, icv, arena


def _want(oracle, b, sas, asas):
    """What one fcgpu_process call leaves: SEAL (asas) first, then ENCRYPT (sas); either may be None."""
    e = oracle.process_batch(N.make_cfg(**CFG), b)
    w = dict(arena=b.arena.copy())
    if asas:
        w["ast"], w["icv"], w["arena"] = _seal(b, e, asas)
    if sas:
        w["st"], w["blocks"], w["arena"] = _expect(synth.Batch(arena=w["arena"], desc=b.desc), e, sas, encrypt)
    return w


def _check(oracle, b, sas=SAS, asas=None, want=None):
    w = want or _want(oracle, b, sas, asas)
    ctx = N.Context(0, 1024, N.make_cfg(**CFG))
    try:
        if asas:
            ctx.espauth_set_sas(asas)
            ctx.espauth_configure(N.ESP_SEAL)
        if sas:
            ctx.espaes_configure(N.ESPAES_ENCRYPT)   # before the table: the mode survives set_sas
            ctx.espaes_set_sas(sas)
        got = _run(ctx, b)
        assert np.array_equal(got, w["arena"]), np.nonzero(got != w["arena"])[0][:8]
        if sas:
            c = np.bincount(w["st"], minlength=6)
            assert ctx.espaes_status(b.n).tolist() == w["st"].tolist()
            assert ctx.espaes_stats() == dict(ok=c[1], no_sa=c[3], too_short=c[4], unaligned=c[5], not_esp=c[0],
                                              blocks=w["blocks"])
        if asas:
            rec, c = ctx.espauth_records(b.n), np.bincount(w["ast"], minlength=5)
            assert rec["status"].tolist() == w["ast"].tolist() and np.array_equal(rec["icv"], w["icv"])
            assert ctx.espauth_stats() == dict(ok=c[1], bad=0, no_sa=c[3], too_short=c[4], not_esp=c[0])
    finally:
        ctx.close()
    return w


@pytest.mark.parametrize("sas,asas", [(SAS[:1], None), (None, ASAS[:1])], ids=["encrypt", "seal"])
def test_gpu_espenc_lengths(oracle, sas, asas):
    """SHORT, 0 blocks, 1 block over 8 digest bytes, 1-3 blocks, UNALIGNED (sealed all the same), 1500-B frames of 90 and 89 blocks."""
    w = _check(oracle, _batch([27, 28, 36, 44, 52, 60, 76, 29, 33, 1460, 1452]), sas, asas)
    want = [N.ESP_SHORT] + [N.ESP_OK] * 6 + ([N.ESP_UNALIGNED] * 2 if sas else [N.ESP_OK] * 2) + [N.ESP_OK] * 2
    assert w["st" if sas else "ast"].tolist() == want and (not sas or w["blocks"] == 188)   # sum of (plen + 8) // 16


@pytest.mark.parametrize("sas,asas", [(SAS[:1], None), (None, ASAS[:1])], ids=["encrypt", "seal"])
@pytest.mark.parametrize("ihl", [5, 6])
def test_gpu_espenc_alignment(oracle, ihl, sas, asas):
    """One 5-block frame back to back, 18 times at all 16 alignments: every store shape, every neighbour untouched."""
    f = bytearray(_batch([100], pad=1).frame(0))
    if ihl == 6:
        f[14] = 0x46
        f[34:34] = b"\x01" * 4
        f[16:18] = (len(f) - 15).to_bytes(2, "big")
    arena = np.zeros(16 + 18 * len(f) + synth.ARENA_PAD, np.uint8)
    desc = np.array([[16 + k * len(f), len(f)] for k in range(18)], np.uint32)
    for o in desc[:, 0]:
        arena[o:o + len(f)] = np.frombuffer(bytes(f), np.uint8)
    w = _check(oracle, synth.Batch(arena=arena, desc=desc), sas, asas)
    assert (w["st" if sas else "ast"] == N.ESP_OK).all() and (not sas or w["blocks"] == 18 * 5)


@pytest.mark.parametrize("n,tile,order", [(n, t, "1") for t in ("", "256") for n in (1, 15, 16, 17, 255, 256, 257, 773)] +
                         [(773, "", "0"), (773, "256", "0")])
def test_gpu_espenc_mixed_tile(oracle, n, tile, order, monkeypatch):
    """nblk over {0, 1, 2, 5, 91}: quad-group, wave and tile edges, sorted and in arrival order, 64- and 256-packet tiles."""
    if tile:
        monkeypatch.setenv("FCGPU_ESPAES_TILE", tile)
    monkeypatch.setenv("FCGPU_ESPENC_ORDER", order)
    b = _mixed(n)
    w = _REF[n] = _REF.get(n) or _want(oracle, b, SAS, None)
    _check(oracle, b, want=w)
    assert n != 773 or set(w["st"].tolist()) == {N.ESP_NOT_ESP, N.ESP_OK, N.ESP_NO_SA}


@pytest.mark.parametrize("nsa", [1, 80, 2000])
def test_gpu_espenc_sa_tables(oracle, nsa):
    """LDS images (1, 80 x 192 B) and the global one (2,000): first, middle and last SPI, and a miss."""
    sas = [(5 + 3 * k, hashlib.sha1(bytes([k & 255, k >> 8])).digest()[:16]) for k in range(nsa)][::-1]
    hit = [5, 5 + 3 * (nsa // 2), 5 + 3 * (nsa - 1), 6]
    w = _check(oracle, _batch([108] * 4, spi=hit), sas)
    assert w["st"].tolist() == [N.ESP_OK] * 3 + [N.ESP_NO_SA]


def test_gpu_espenc_outbound_chain_and_back(oracle):
    """SEAL + ENCRYPT in one call; DECRYPT + VERIFY on a second context undo it; one flipped bit is BAD for its packet."""
    n = 40
    b = _batch(36 + 8 * (np.arange(n) % 11), spi=np.asarray([s for s, _ in SAS])[np.arange(n) % 4])
    w = _check(oracle, b, SAS, ASAS)
    assert (w["ast"] == N.ESP_OK).all() and (w["st"] == N.ESP_OK).all()
    sealed = _seal(b, oracle.process_batch(N.make_cfg(**CFG), b), ASAS)[2]
    wire = synth.Batch(arena=w["arena"].copy(), desc=b.desc)
    wire.arena[int(b.desc[n - 1, 0]) + 34 + 16 + 3] ^= 0x10           # the last packet: one ciphertext bit
    ctx = N.Context(0, 1024, N.make_cfg(**CFG))
    try:
        ctx.espauth_set_sas(ASAS)
        ctx.espaes_set_sas(SAS)
        got, rec, lo = _run(ctx, wire), ctx.espauth_records(n), int(b.desc[n - 1, 0])
        assert rec["status"].tolist() == [N.ESP_OK] * (n - 1) + [N.ESP_BAD]
        assert np.array_equal(got[:lo], sealed[:lo]) and np.array_equal(rec["icv"][:n - 1], w["icv"][:n - 1])
    finally:
        ctx.close()


def test_gpu_espenc_configure_modes_stats(oracle):
    """Refused modes, the mode across set_sas, encrypt then decrypt on one context, statistics, reset."""
    ctx = N.Context(0, 1024, N.make_cfg(**CFG))
    try:
        for call, mode in (ctx.espaes_configure, 2), (ctx.espauth_configure, 3):
            with pytest.raises(RuntimeError, match="configure: bad mode"):
                call(mode)
        ctx.espaes_set_sas(SAS[:2])
        ctx.espaes_configure(N.ESPAES_ENCRYPT)
        ctx.espaes_set_sas(SAS)                                       # the mode stays
        b1, b2 = _mixed(100), _mixed(65, seed=4)
        w1, w2 = _want(oracle, b1, SAS, None), _want(oracle, b2, SAS, None)
        g1, g2 = _run(ctx, b1), _run(ctx, b2)
        assert np.array_equal(g1, w1["arena"]) and np.array_equal(g2, w2["arena"])
        c = np.bincount(np.concatenate([w1["st"], w2["st"]]), minlength=6)
        assert ctx.espaes_stats() == dict(ok=c[1], no_sa=c[3], too_short=c[4], unaligned=c[5], not_esp=c[0],
                                          blocks=w1["blocks"] + w2["blocks"])
        ctx.espaes_reset()
        assert not any(ctx.espaes_stats().values())
        ctx.espaes_configure(N.ESPAES_DECRYPT)
        back = _run(ctx, synth.Batch(arena=g1, desc=b1.desc))
        assert np.array_equal(back, b1.arena) and ctx.espaes_stats()["blocks"] == w1["blocks"]
    finally:
        ctx.close()
