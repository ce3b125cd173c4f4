"""FCGPU_CLS_STRING: StringClassifier's AhoCorasick::match_first (earliest match
end; of the patterns ending there the longest) by the host walk and by the
k_acmatch pre-pass + k_rx. The reference is a plain search: each pattern's
first occurrence gives its earliest end, the least of those is the match end,
and the longest pattern that ends there wins. No automaton here. Everything
but the port comes from the oracle with CLS_NONE.

The chunk size S follows the set's longest pattern (32 for <= 32 bytes, else
the next power of two), so no set has patterns longer than its S: the lengths
S+1 and 2S+3 are taken against the base chunk of 32 (33 and 67, in the set
whose S is 128), S-1 and S in the set whose S is 32."""
import numpy as np
import pytest

from fastclick_amd import synth
from fastclick_amd import _native as N


def brute(pats, text):
    ends = [(text.find(p) + len(p), -len(p), k) for k, p in enumerate(pats) if p in text]
    if not ends:
        return -1, 0
    e = min(ends)[0]
    return max((len(p), k) for k, p in enumerate(pats) if text[:e].endswith(p))[1], e


def _rand_sets():
    for seed in range(6):
        rng = np.random.default_rng(seed)
        pats = list({bytes(rng.choice(list(b"acgt"), rng.integers(1, 7)).tolist()) for _ in range(12)})
        yield pats, [bytes(rng.choice(list(b"acgtn"), rng.integers(0, 60)).tolist()) for _ in range(200)]


CPU_SETS = [
    ([b"he", b"she", b"his", b"hers"], [b"ushers", b"his", b"xhex", b""]),
    ([b"abcd", b"bcd", b"d", b"ab", b"abcde"], [b"xabcdex", b"zzabz", b"bcd", b"abcx"]),        # suffixes and prefixes
    ([b"\x00", b"\xff", b"\x00\xff\x00"], [b"ab\xff\x00", b"a\x00\xff\x00", b"abc"]),
    ([b"q" * 1024, b"qz"], [b"q" * 1023 + b"z", b"q" * 1500, b"q" * 1023]),
] + list(_rand_sets())


@pytest.mark.parametrize("pats,texts", CPU_SETS, ids=lambda v: None)
def test_host_walk_matches_search(pats, texts):
    for t in texts:
        assert N.patterns_match(pats, t) == brute(pats, t), t
    assert N.patterns_match(CPU_SETS[0][0], b"ushers") == (1, 4)    # "she": same end as "he", longer


@pytest.mark.parametrize("pats,nports,msg", [([b"a", b""], 0, "empty"), ([b"x" * 1025], 0, "1024"),
                                             ([b"ab", b"c", b"ab"], 0, "duplicate"), ([b"a", b"b", b"c"], 2, "nports")])
def test_patterns_refused(pats, nports, msg):
    with pytest.raises(ValueError, match=msg):
        N.patterns_match(pats, b"abc", nports)


# ---- device ------------------------------------------------------------------
def _sets():
    rng = np.random.default_rng(40)
    s32 = [b"\xa1", b"\xa2\xa3", bytes(range(0xb0, 0xb0 + 31)), b"\xa4" + bytes(range(0xb0, 0xb0 + 31))]
    s128 = s32[:2] + [bytes(rng.integers(0xb0, 0xc0, k, dtype=np.uint8)) for k in (31, 32, 33, 67)]
    big = [bytes(rng.integers(0x90, 0x100, 200, dtype=np.uint8)) for _ in range(40)]
    # pattern 1 lies inside pattern 0: it starts later and ends first; pattern 2 is the
    # first four bytes of the 257-byte frames' IP header (header bytes are text)
    order = [bytes(range(0xc0, 0xe0)), b"\xc5\xc6", b"\x45\x00\x00\xf3"]
    return {"lds32": (s32, 32, True), "lds128": (s128, 128, True), "order": (order, 32, True),
            "global": (big, 256, False)}


SETS = _sets()
LENGTHS = (60, 64, 65, 257, 1500)


def _frames(pats, S, mark, seed):
    """UDP/IPv4 frames of LENGTHS with a zero payload: per pattern (the set's
    last eight at most) one frame for every end offset kS-1, kS, kS+1 and the
    last byte, where the pattern fits behind the headers (anywhere under
    MARK_IP4, which checks nothing), and one with no plant; a pattern only in
    padding past ip_len; a header error."""
    rng = np.random.default_rng(seed)
    out = []
    for L in LENGTHS:
        hdr = synth.build_headers(1, src=0x0A000001, dst=0x0A000002, sport=7, dport=9, frame_len=L, width=64)[0]
        base = bytearray(bytes(hdr[:min(L, 64)]) + bytes(max(L - 64, 0)))
        out.append(bytes(base))
        lo = 0 if mark else 42
        for p in pats[-8:]:
            ends = {L} | {k * S + d for k in range(1, L // S + 1) for d in (-1, 0, 1)}
            for e in sorted(e for e in ends if lo + len(p) <= e <= L):
                f = bytearray(base)
                f[e - len(p):e] = p
                out.append(bytes(f))
        out.append(bytes(base) + bytes(6) + pats[1] + bytes(3))          # padding past ip_len
        bad = bytearray(base)
        bad[14] = 0x55
        out.append(bytes(bad) if not mark else bytes(base))
    order = rng.permutation(len(out))
    return [out[k] for k in order]


def _batch(frames, seed):
    from helpers import repack
    return repack(synth.from_frames(frames), misalign_seed=seed)


def _expect(oracle, cfg, b, pats):
    c0 = N.make_cfg(check_mode=cfg.check_mode, offset=14, checksum=True, nports=cfg.nports)
    e = oracle.process_batch(c0, b)
    reason, port = e["reason"].copy(), np.full(b.n, cfg.nports, np.uint8)
    for i in np.nonzero(reason == N.R_OK)[0]:
        pid, _ = brute(pats, b.frame(i)[:int(e["anno"]["length"][i])])
        port[i] = pid if pid >= 0 else min(len(pats), cfg.nports)
        if port[i] == cfg.nports:
            reason[i] = N.R_NO_MATCH
    cnt = np.bincount(port, minlength=cfg.nports + 1)
    tiles = [port[t:t + N.TILE] for t in range(0, b.n, N.TILE)]
    ctr = np.zeros(N.NCOUNTERS, np.uint64)
    ctr[N.CTR_PORT:N.CTR_PORT + cfg.nports + 1] = cnt
    for r in np.unique(reason[reason != N.R_OK]):
        ctr[N.CTR_REASON + N.reason_slot(int(r))] = int((reason == r).sum())
    ctr[N.CTR_DROPS] = ctr[N.CTR_REASON:N.CTR_REASON + N.reason_slot(N.R_NO_MATCH)].sum()
    ctr[N.CTR_COUNT] = b.n - ctr[N.CTR_DROPS]
    return dict(reason=reason, port=port, hash=e["hash"], anno=e["anno"], counters=ctr,
                perm=np.argsort(port, kind="stable").astype(np.uint32),
                port_start=np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32),
                perm_tile=np.concatenate([t0 + np.argsort(t, kind="stable") for t0, t in
                                          zip(range(0, b.n, N.TILE), tiles)]).astype(np.uint32),
                tile_count=np.concatenate([np.bincount(t, minlength=cfg.nports + 1) for t in tiles]).astype(np.uint16))


def _check(got, exp):
    from helpers import compare
    compare(got, exp)
    assert np.array_equal(got["counters"], exp["counters"])


def _cases():
    for name in SETS:
        for mark in (0, 1):
            for part in (N.PART_TILE, N.PART_GLOBAL):
                for spare in (1, 0):       # a no-match output, or none: R_NO_MATCH
                    if (part == N.PART_TILE) == (spare == 1) or name == "lds32":
                        yield pytest.param(name, mark, part, spare, 0,
                                           id=f"{name}-{'mark' if mark else 'check'}-{'tile' if part else 'global'}-{spare}")
    for n in (1, 255, 1000):
        yield pytest.param("lds32", 0, N.PART_TILE, 1, n, id=f"n{n}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,mark,part,spare,n", _cases())
def test_gpu_string_matches_search(oracle, name, mark, part, spare, n):
    from fastclick_amd import device as D
    pats, S, in_lds = SETS[name]
    st = N.patterns_stats(pats)
    assert st["in_lds"] == in_lds and max(32, 1 << (st["lmax"] - 1).bit_length()) == S
    frames = _frames(pats, S, mark, seed=len(name) + mark)
    b = _batch((frames * (n // len(frames) + 1))[:n] if n else frames, seed=7 + part)
    cfg = N.make_cfg(check_mode=N.MARK_IP4 if mark else N.CHECK_IP4, offset=14, checksum=True, classify=N.CLS_STRING,
                     nports=len(pats) + spare)
    exp = _expect(oracle, cfg, b, pats)
    if not n:
        hit = exp["port"] < len(pats)
        assert hit.sum() > 20 and (~hit).any() and (mark or (exp["reason"] == N.R_BAD_VERSION).any())
        assert (exp["reason"] == N.R_NO_MATCH).any() == (spare == 0)
        winners = {"order": {1, 2}, "global": set(range(32, 40)) | ({1} if mark else set())}.get(name, set(range(len(pats))))
        assert set(exp["port"][hit].tolist()) == winners
    _check(D.process_batch(b, cfg, partition=part, patterns=pats), exp)


@pytest.mark.gpu
def test_gpu_string_jobs_and_refused_paths(oracle):
    """Three jobs in one fcgpu_process_jobs call equal three fcgpu_process
    calls; the other submission paths, a context without patterns, more
    patterns than outputs and the non-IPv4 check modes are refused."""
    import torch
    from fastclick_amd import device as D
    pats, S, _ = SETS["lds128"]
    cfg = N.make_cfg(offset=14, checksum=True, classify=N.CLS_STRING, nports=len(pats) + 1)
    ctx = N.Context(0, 4096, cfg)
    try:
        bs = [_batch(_frames(pats, S, 0, seed=k)[:300 + 50 * k], seed=k) for k in range(3)]
        dbs = [D.DeviceBatch.upload(b) for b in bs]
        with pytest.raises(RuntimeError, match="fcgpu_set_patterns"):
            D.run_device(ctx, dbs[0], D.DeviceOutputs(bs[0].n, cfg.nports))
        with pytest.raises(RuntimeError, match="nports"):
            ctx.set_patterns(pats + [b"one", b"two"])
        ctx.set_patterns(pats)
        outs = [[D.DeviceOutputs(b.n, cfg.nports, anno=True, perm=True, partition=N.PART_TILE) for b in bs]
                for _ in range(2)]
        for db, o in zip(dbs, outs[0]):
            D.run_device(ctx, db, o)
        s = torch.cuda.current_stream().cuda_stream
        ctx.run_jobs(ctx.jobs([(db.arena.data_ptr(), db.desc.data_ptr(), db.n, s, o.ptrs())
                               for db, o in zip(dbs, outs[1])]))
        torch.cuda.synchronize()
        for b, o1, o2 in zip(bs, outs[0], outs[1]):
            exp = _expect(oracle, cfg, b, pats)
            for o in (o1, o2):
                got = o.numpy()
                assert np.array_equal(got["port"], exp["port"]) and np.array_equal(got["reason"], exp["reason"])
                assert np.array_equal(got["perm_tile"], exp["perm_tile"])
        db, o = dbs[0], outs[0][0]
        lens = np.ascontiguousarray(bs[0].desc[:, 1])
        cnt = torch.tensor([4], dtype=torch.int32, device="cuda")
        refused = [
            lambda: ctx.process_counted(db.arena.data_ptr(), db.desc.data_ptr(), db.n, cnt.data_ptr(), **o.ptrs()),
            lambda: ctx.process_host((N.C.c_void_p * db.n)(), lens.ctypes.data, db.n, verdict=1),
            lambda: ctx.process_mbufs(lens.ctypes.data, db.n, verdict=1),
            lambda: ctx.span_submit(0, bs[0].arena.ctypes.data, bs[0].arena.size, bs[0].desc.ctypes.data, db.n, verdict=1),
            lambda: ctx._chk(ctx.lib.fcgpu_span_submit_block(ctx.h, 0, bs[0].arena.ctypes.data, bs[0].arena.size, 0, 0,
                                                             db.n, bs[0].arena.ctypes.data, 1, 0), "block"),
        ]
        for call in refused:
            with pytest.raises(RuntimeError, match="CLS_STRING"):
                call()
        for mode in (N.CHECK_AUTO, N.MARK_IP6):
            with pytest.raises(RuntimeError, match="IPv4 check modes"):
                ctx.configure(N.make_cfg(check_mode=mode, classify=N.CLS_STRING, nports=9))
    finally:
        ctx.close()
