"""ctypes binding of the C ABI in include/fastclick_gpu.h (libfcgpu.so).

The shared library is built in-tree by ``fastclick_amd.build`` (hipcc, gfx950)
into ``fastclick_amd/lib/``. Loading fails loudly when it is missing: there is
no CPU fallback for the product path.
"""
from __future__ import annotations

import ctypes as C
import os

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
# FCGPU_LIB: another build of the library (same-box A/B measurements only)
LIBFCGPU = os.environ.get("FCGPU_LIB") or os.path.join(LIB_DIR, "libfcgpu.so")
LIBFCCLICK = os.path.join(LIB_DIR, "libfcclick.so")

# ---- constants mirrored from include/fastclick_gpu.h -----------------------
ABI_VERSION = 32
SPAN_SLOTS = 3
SPAN_COPY = 0
SPAN_ZEROCOPY = 1
SPAN_AUTO = 2
OK, EINVAL, ENODEV, ENOMEM, ERUNTIME = 0, -1, -2, -3, -4
R_MINISCULE, R_BAD_VERSION, R_BAD_HLEN, R_BAD_IP_LEN, R_BAD_CKSUM, R_BAD_SADDR, R_OK, \
    R_BAD_IP6, R_VLAN_REJECT, R_NO_MATCH, R_L4_PROTO, R_L4_LENGTH, R_L4_CKSUM, \
    R_TTL_EXPIRED, R_SETCKSUM_BAD = range(15)
NREASON_SLOTS = 14
RW_DECTTL, RW_SETCKSUM, RW_INPLACE = 1, 2, 4
L4_NONE, L4_UDP, L4_TCP = 0, 1, 2


def reason_slot(r: int) -> int:
    """Counter slot of reason r (reasons 0-5, 7-14; 6 = valid has none)."""
    return r if r < 6 else r - 1
CHECK_IP4, MARK_IP4, CHECK_AUTO, MARK_IP6 = 0, 1, 2, 3
HASH_NONE, HASH_FLOWID, HASH_FLOW5ID = 0, 1, 2
CLS_NONE, CLS_LB_HASH, CLS_HASH_IP, CLS_HASHSWITCH, CLS_PROGRAM, CLS_LB_CRC, CLS_LB_TABLE, CLS_ROUTE = range(8)
CLS_ROUTE6 = 8
CLS_STRING = 9
AC_LDS_TABLE = 36 * 1024   # fcgpu_match.hh kAcLdsTable: class map + transitions staged in LDS up to this
PROG_IPFILTER, PROG_CLASSIFIER = 0, 1
STEP_SHORT_YES = 1
MAX_STEPS = 8192
MAX_PORTS = 64
LB_TABLE_MAX = 1 << 24
MAX_ADDRS = 16
CTR_COUNT, CTR_DROPS, CTR_REASON, CTR_PORT = 0, 1, 2, 16
NCOUNTERS = CTR_PORT + MAX_PORTS + 1
CTR_SHARDS = 64
PART_GLOBAL, PART_TILE = 0, 1
OUT_VERDICT, OUT_HASH, OUT_ANNO, OUT_PERM, OUT_PORT_START, OUT_TILE_COUNT, OUT_TILE_PERM, OUT_FLOWID, \
    OUT_IP_RW, OUT_ANNO8 = (1 << k for k in range(10))
SUBMIT_COPY = 1 << 31
SUBMIT_DESC32 = 1 << 30
FAULT_SUBMIT, FAULT_WAIT, FAULT_LAUNCH, FAULT_ALLOC = 0, 1, 2, 3
OUT_ABSENT = (1 << 64) - 1
TILE = 256

REASON_TEXTS = ["tiny packet", "bad IPv4 version", "bad IPv4 header length",
                "bad IPv4 length", "bad IPv4 checksum", "bad source address"]


class fcgpu_cfg(C.Structure):
    _fields_ = [
        ("size", C.c_uint32),
        ("check_mode", C.c_uint32),
        ("offset", C.c_int32),
        ("checksum", C.c_uint32),
        ("hash_mode", C.c_uint32),
        ("classify", C.c_uint32),
        ("nports", C.c_uint32),
        ("hs_offset", C.c_int32),
        ("hs_length", C.c_int32),
        ("native_vlan", C.c_int32),
        ("nbadsrc", C.c_uint32),
        ("ngooddst", C.c_uint32),
        ("badsrc", C.c_uint32 * MAX_ADDRS),
        ("gooddst", C.c_uint32 * MAX_ADDRS),
        ("nbad6", C.c_uint32),
        ("bad6", (C.c_uint8 * 16) * MAX_ADDRS),
        ("process_eh", C.c_uint32),
        ("l4_mode", C.c_uint32),
        ("l4_checksum", C.c_uint32),
        ("rewrite", C.c_uint32),
        ("ttl_multicast", C.c_uint32),
        ("vlan_ethertype", C.c_uint32),
    ]


class fcgpu_anno(C.Structure):
    _fields_ = [
        ("dst_ip", C.c_uint32),
        ("length", C.c_uint16),
        ("vlan_tci", C.c_uint16),
        ("nh", C.c_uint16),
        ("th", C.c_uint16),
        ("ip6_nxt", C.c_uint8),
        ("ipver", C.c_uint8),
        ("reserved", C.c_uint16),
    ]


class fcgpu_anno8(C.Structure):
    _fields_ = [("dst_ip", C.c_uint32), ("length", C.c_uint16), ("nh", C.c_uint8), ("thl", C.c_uint8)]


class fcgpu_xmeta(C.Structure):
    _fields_ = [("off", C.c_uint32), ("length", C.c_uint32), ("src_index", C.c_uint32), ("src_rank", C.c_uint32)]


ANNO_DTYPE = None   # numpy structured dtype, set lazily (numpy import is optional here)


def anno_dtype():
    global ANNO_DTYPE
    if ANNO_DTYPE is None:
        import numpy as np
        ANNO_DTYPE = np.dtype([("dst_ip", "<u4"), ("length", "<u2"), ("vlan_tci", "<u2"),
                               ("nh", "<u2"), ("th", "<u2"), ("ip6_nxt", "u1"), ("ipver", "u1"),
                               ("reserved", "<u2")])
        assert ANNO_DTYPE.itemsize == C.sizeof(fcgpu_anno) == 16
    return ANNO_DTYPE


FLOW_NONE = 0xFFFFFFFF
FLOW_FULL = 0xFFFFFFFE
FLOW_MAX_BATCH = 64 * ((1 << 14) + 64)   # FCGPU_FLOW_MAX_BATCH
MAX_FLOWS = 1 << 23
FLOW_MGR_HMP = 0
FLOW_MGR_IMP = 1


class fcgpu_flow_config(C.Structure):
    _fields_ = [("manager", C.c_uint32), ("capacity", C.c_uint32), ("timeout_s", C.c_uint32),
                ("recycle_ms", C.c_uint32)]


class fcgpu_flow_stat(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("manager", "capacity", "count", "free_ids", "pending", "epochs")]


AGGCOUNT_MAX_CAPACITY = 1 << 24


class fcgpu_aggcount_config(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("capacity", "bytes", "ip_bytes", "mask")]


class fcgpu_aggcount_stat(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("capacity", "nagg", "nnz", "frozen")] + \
               [(k, C.c_uint64) for k in ("count", "seen", "uncounted")]


class fcgpu_aggcount_rec(C.Structure):
    _fields_ = [("agg", C.c_uint32), ("reserved", C.c_uint32), ("count", C.c_uint64)]


ESP_VERIFY, ESP_COMPUTE, ESP_SEAL = 0, 1, 2
ESP_NOT_ESP, ESP_OK, ESP_BAD, ESP_NO_SA, ESP_SHORT = range(5)
ESPAUTH_MAX_SAS = 65536


class fcgpu_esp_sa(C.Structure):
    _fields_ = [("spi", C.c_uint32), ("auth_key", C.c_uint8 * 16)]


class fcgpu_espauth_config(C.Structure):
    _fields_ = [("mode", C.c_uint32)]


class fcgpu_esp_rec(C.Structure):
    _fields_ = [("status", C.c_uint8), ("pad", C.c_uint8 * 3), ("icv", C.c_uint8 * 12)]


class fcgpu_espauth_stat(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("ok", "bad", "no_sa", "too_short", "not_esp")]


ESP_UNALIGNED = 5
ESPAES_MAX_SAS = 65536
ESPAES_DECRYPT, ESPAES_ENCRYPT = 0, 1


class fcgpu_espaes_sa(C.Structure):
    _fields_ = [("spi", C.c_uint32), ("enc_key", C.c_uint8 * 16)]


class fcgpu_espaes_config(C.Structure):
    _fields_ = [("mode", C.c_uint32)]


class fcgpu_espaes_stat(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("ok", "no_sa", "too_short", "unaligned", "not_esp", "blocks")]


class fcgpu_out(C.Structure):
    _fields_ = [
        ("verdict", C.c_void_p),
        ("hash", C.c_void_p),
        ("anno", C.c_void_p),
        ("perm", C.c_void_p),
        ("port_start", C.c_void_p),
        ("tile_count", C.c_void_p),
        ("partition", C.c_uint32),
        ("reserved", C.c_uint32),
        ("tile_perm", C.c_void_p),
        ("flowid", C.c_void_p),
        ("ip_rw", C.c_void_p),
    ]


class fcgpu_job(C.Structure):
    _fields_ = [
        ("arena", C.c_void_p),
        ("desc", C.c_void_p),
        ("n", C.c_uint32),
        ("reserved", C.c_uint32),
        ("stream", C.c_void_p),
        ("out", fcgpu_out),
    ]


class fcgpu_block_layout(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("verdict", "hash", "anno", "perm", "port_start", "tile_count",
                                          "tile_perm", "flowid", "ip_rw", "bytes")]


class fcgpu_mbuf_layout(C.Structure):
    _fields_ = [("buf_addr", C.c_uint32), ("data_off", C.c_uint32), ("data_len", C.c_uint32),
                ("header_bytes", C.c_uint32)]


MBUF_LAYOUT_DPDK = (0, 16, 40, 64)      # FCGPU_MBUF_LAYOUT_DPDK (rte_mbuf, DPDK >= 20.11)


class fcgpu_step(C.Structure):
    _fields_ = [
        ("offset", C.c_int32),
        ("value", C.c_uint32),
        ("mask", C.c_uint32),
        ("yes", C.c_int32),
        ("no", C.c_int32),
        ("flags", C.c_uint32),
    ]


# Every symbol include/fastclick_gpu.h declares (checked by tests/test_abi.py).
FCGPU_SYMBOLS = {
    "fcgpu_abi_version": (C.c_int, []),
    "fcgpu_device_count": (C.c_int, []),
    "fcgpu_default_cfg": (None, [C.POINTER(fcgpu_cfg)]),
    "fcgpu_open": (C.c_int, [C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]),
    "fcgpu_configure": (C.c_int, [C.c_void_p, C.POINTER(fcgpu_cfg)]),
    "fcgpu_close": (None, [C.c_void_p]),
    "fcgpu_process": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                C.POINTER(fcgpu_out), C.c_void_p]),
    "fcgpu_process_jobs": (C.c_int, [C.c_void_p, C.POINTER(fcgpu_job), C.c_uint32, C.c_void_p]),
    "fcgpu_process_host": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32,
                                     C.POINTER(fcgpu_out)]),
    "fcgpu_set_program": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(fcgpu_step), C.c_uint32,
                                    C.c_int32]),
    "fcgpu_set_lb_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "fcgpu_lb_hash_ring": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p]),
    "fcgpu_set_routes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "fcgpu_route_lookup": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fcgpu_set_routes6": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "fcgpu_route6_lookup": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32)]),
    "fcgpu_route6_stats": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fcgpu_set_patterns": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint32]),
    "fcgpu_patterns_match": (C.c_int, [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32,
                                       C.POINTER(C.c_uint32)]),
    "fcgpu_patterns_stats": (C.c_int, [C.c_char_p, C.c_void_p, C.c_uint32] + [C.POINTER(C.c_uint32)] * 4),
    "fcgpu_set_host_threads": (C.c_int, [C.c_void_p, C.c_uint32]),
    "fcgpu_span_submit": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32,
                                    C.POINTER(fcgpu_out)]),
    "fcgpu_span_wait": (C.c_int, [C.c_void_p, C.c_uint32]),
    "fcgpu_span_poll": (C.c_int, [C.c_void_p, C.c_uint32]),
    "fcgpu_span_mode": (C.c_int, [C.c_void_p, C.c_uint32]),
    "fcgpu_span_reserve": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32]),
    "fcgpu_span_zerocopy_active": (C.c_int, [C.c_void_p]),
    "fcgpu_inject_fault": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "fcgpu_launch_guard_selftest": (C.c_int, []),
    "fcgpu_block_layout_for": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "fcgpu_span_submit_block": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                          C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]),
    "fcgpu_flow_enable": (C.c_int, [C.c_void_p, C.c_uint32]),
    "fcgpu_flow_reset": (C.c_int, [C.c_void_p]),
    "fcgpu_flow_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "fcgpu_flow_configure": (C.c_int, [C.c_void_p, C.POINTER(fcgpu_flow_config)]),
    "fcgpu_program_jit": (C.c_int, [C.c_void_p, C.c_int]),
    "fcgpu_program_jit_active": (C.c_int, [C.c_void_p]),
    "fcgpu_flow_set_time": (C.c_int, [C.c_void_p, C.c_uint32]),
    "fcgpu_flow_maintain": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "fcgpu_flow_stats": (C.c_int, [C.c_void_p, C.POINTER(fcgpu_flow_stat)]),
    "fcgpu_aggcount_configure": (C.c_int, [C.c_void_p, C.POINTER(fcgpu_aggcount_config)]),
    "fcgpu_aggcount_freeze": (C.c_int, [C.c_void_p, C.c_int]),
    "fcgpu_aggcount_reset": (C.c_int, [C.c_void_p]),
    "fcgpu_aggcount_stats": (C.c_int, [C.c_void_p, C.POINTER(fcgpu_aggcount_stat)]),
    "fcgpu_aggcount_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fcgpu_espauth_set_sas": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "fcgpu_espauth_configure": (C.c_int, [C.c_void_p, C.POINTER(fcgpu_espauth_config)]),
    "fcgpu_espauth_records": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "fcgpu_espauth_stats": (C.c_int, [C.c_void_p, C.POINTER(fcgpu_espauth_stat)]),
    "fcgpu_espauth_reset": (C.c_int, [C.c_void_p]),
    "fcgpu_espaes_set_sas": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "fcgpu_espaes_configure": (C.c_int, [C.c_void_p, C.POINTER(fcgpu_espaes_config)]),
    "fcgpu_espaes_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "fcgpu_espaes_stats": (C.c_int, [C.c_void_p, C.POINTER(fcgpu_espaes_stat)]),
    "fcgpu_espaes_reset": (C.c_int, [C.c_void_p]),
    "fcgpu_host_alloc": (C.c_void_p, [C.c_size_t]),
    "fcgpu_host_free": (None, [C.c_void_p]),
    "fcgpu_pool_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "fcgpu_process_mbufs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(fcgpu_mbuf_layout),
                                      C.POINTER(fcgpu_out), C.c_void_p]),
    "fcgpu_host_register": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int]),
    "fcgpu_host_unregister": (C.c_int, [C.c_void_p]),
    "fcgpu_read_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "fcgpu_counters_derive": (None, [C.c_void_p]),
    "fcgpu_reset_counters": (C.c_int, [C.c_void_p]),
    "fcgpu_counters_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "fcgpu_use_counters": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fcgpu_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "fcgpu_read_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                    C.c_int]),
    "fcgpu_exchange_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fcgpu_exchange_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]),
    "fcgpu_exchange_unpack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32,
                                        C.c_void_p, C.c_void_p]),
    "fcgpu_exchange_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.c_void_p]),
    "fcgpu_exchange_build_fixed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "fcgpu_exchange_unpack_fixed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                              C.c_void_p]),
    "fcgpu_process_counted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                        C.POINTER(fcgpu_out), C.c_void_p]),
    "fcgpu_last_error": (C.c_char_p, [C.c_void_p]),
}

_lib = None


class NativeMissing(RuntimeError):
    pass


def load(path: str = LIBFCGPU):
    """Load libfcgpu.so (after torch, so one HIP runtime serves both)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NativeMissing(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    try:
        import torch  # noqa: F401  (share torch's HIP runtime: same soname)
    except Exception:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in FCGPU_SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.fcgpu_abi_version() != ABI_VERSION:
        raise NativeMissing("libfcgpu.so ABI version mismatch")
    _lib = lib
    return lib


def lb_hash_ring(nsel: int, size: int | None = None):
    """The constant_hash_agg ring (fcgpu_lb_hash_ring: LoadBalancer::
    build_hash_ring over [0, nsel), size CST_BUCKETS or 100 per output) as a
    uint8 array, the table Context.set_lb_table takes. Host-only."""
    import numpy as np
    size = 100 * nsel if size is None else size
    out = np.zeros(size, np.uint8)
    rc = load().fcgpu_lb_hash_ring(nsel, size, out.ctypes.data)
    if rc != OK:
        raise ValueError(f"fcgpu_lb_hash_ring({nsel}, {size}) failed ({rc})")
    return out


def route_dtype():
    """numpy dtype of fcgpu_route."""
    import numpy as np
    return np.dtype([("addr", "<u4"), ("gw", "<u4"), ("plen", "u1"), ("port", "u1"), ("reserved", "<u2")])


def routes_array(routes):
    """fcgpu_route records (a numpy structured array) from a sequence of
    (addr, plen, gw, port): addr and gw dotted quads or raw network-order
    words (raw_addr), gw 0 / None = no gateway. An array of that dtype passes
    through."""
    import numpy as np
    dt = route_dtype()
    if isinstance(routes, np.ndarray) and routes.dtype == dt:
        return np.ascontiguousarray(routes)
    out = np.zeros(len(routes), dt)
    for k, (addr, plen, gw, port) in enumerate(routes):
        if not (0 <= int(plen) <= 255 and 0 <= int(port) <= 255):
            raise ValueError(f"route {k}: prefix length or output out of range")
        out[k] = (raw_addr(addr) if isinstance(addr, str) else addr,
                  raw_addr(gw) if isinstance(gw, str) else (gw or 0), plen, port, 0)
    return out


def route_lookup(routes, addr, nports: int = 0):
    """fcgpu_route_lookup: (port, gw) of addr's longest matching prefix in
    `routes` (routes_array's forms), port -1 and gw 0 without a route; gw is a
    raw network-order word. The trie is built and walked as on the device.
    Host-only. Raises ValueError for a route list fcgpu_set_routes refuses."""
    r = routes_array(routes)
    gw = C.c_uint32(0)
    lib = load()
    port = lib.fcgpu_route_lookup(r.ctypes.data, len(r), nports, raw_addr(addr) if isinstance(addr, str) else addr,
                                  C.byref(gw))
    if port < -1:
        raise ValueError((lib.fcgpu_last_error(None) or b"").decode())
    return port, gw.value


def route6_dtype():
    """numpy dtype of fcgpu_route6."""
    import numpy as np
    return np.dtype([("addr", "u1", 16), ("gw", "u1", 16), ("plen", "u1"), ("port", "u1"), ("reserved", "<u2")])


def addr6(a) -> bytes:
    """The 16 network-order bytes of an IPv6 address: a string (inet_pton),
    16 bytes, or 0 / None for ::."""
    import socket
    if not a:
        return bytes(16)
    if isinstance(a, str):
        return socket.inet_pton(socket.AF_INET6, a)
    a = bytes(a)
    if len(a) != 16:
        raise ValueError("an IPv6 address is 16 bytes")
    return a


def routes6_array(routes):
    """fcgpu_route6 records (a numpy structured array) from a sequence of
    (addr, plen, gw, port): addr and gw strings or 16 bytes (addr6's forms),
    gw 0 / None = no gateway. An array of that dtype passes through."""
    import numpy as np
    dt = route6_dtype()
    if isinstance(routes, np.ndarray) and routes.dtype == dt:
        return np.ascontiguousarray(routes)
    out = np.zeros(len(routes), dt)
    for k, (addr, plen, gw, port) in enumerate(routes):
        if not (0 <= int(plen) <= 255 and 0 <= int(port) <= 255):
            raise ValueError(f"route {k}: prefix length or output out of range")
        out[k] = (np.frombuffer(addr6(addr), np.uint8), np.frombuffer(addr6(gw), np.uint8), plen, port, 0)
    return out


def route6_lookup(routes, addr, nports: int = 0):
    """fcgpu_route6_lookup: (port, gateway id) of addr's longest matching
    prefix in `routes` (routes6_array's forms), port -1 and id 0 without a
    route. The trie is built and walked as on the device. Host-only. Raises
    ValueError for a route list fcgpu_set_routes6 refuses."""
    r = routes6_array(routes)
    gw = C.c_uint32(0)
    lib = load()
    port = lib.fcgpu_route6_lookup(r.ctypes.data, len(r), nports, addr6(addr), C.byref(gw))
    if port < -1:
        raise ValueError((lib.fcgpu_last_error(None) or b"").decode())
    return port, gw.value


def route6_stats(routes):
    """fcgpu_route6_stats: (surviving chunks, longest walk in dependent loads)
    of the trie built from `routes`."""
    r = routes6_array(routes)
    chunks, loads = C.c_uint32(0), C.c_uint32(0)
    lib = load()
    if lib.fcgpu_route6_stats(r.ctypes.data, len(r), C.byref(chunks), C.byref(loads)) != OK:
        raise ValueError((lib.fcgpu_last_error(None) or b"").decode())
    return chunks.value, loads.value


def _patterns(patterns):
    """(concatenated bytes, uint32 lengths array, n) of a sequence of byte strings."""
    pats = [bytes(p) for p in patterns]
    lens = (C.c_uint32 * max(len(pats), 1))(*[len(p) for p in pats])
    return b"".join(pats), lens, len(pats)


def patterns_match(patterns, text, nports: int = 0):
    """fcgpu_patterns_match: (id, end) of AhoCorasick::match_first over `text`
    -- the pattern whose match ends earliest, the longest of those ending
    there; end = the bytes of text up to and including the match -- or (-1, 0).
    The automaton is built and walked as on the device. Host-only. Raises
    ValueError for a pattern list fcgpu_set_patterns refuses."""
    blob, lens, n = _patterns(patterns)
    text = bytes(text)
    end = C.c_uint32(0)
    lib = load()
    pid = lib.fcgpu_patterns_match(blob, lens, n, nports, text, len(text), C.byref(end))
    if pid < -1:
        raise ValueError((lib.fcgpu_last_error(None) or b"").decode())
    return pid, end.value


def patterns_stats(patterns):
    """fcgpu_patterns_stats: dict(states, classes, image_bytes, lmax, in_lds)
    of the automaton built from `patterns`; in_lds: its transitions are staged
    in LDS by the pre-pass (else read from global memory)."""
    blob, lens, n = _patterns(patterns)
    v = [C.c_uint32(0) for _ in range(4)]
    lib = load()
    if lib.fcgpu_patterns_stats(blob, lens, n, *[C.byref(x) for x in v]) != OK:
        raise ValueError((lib.fcgpu_last_error(None) or b"").decode())
    states, classes, image, lmax = (x.value for x in v)
    return dict(states=states, classes=classes, image_bytes=image, lmax=lmax,
                in_lds=(256 + 2 * states * classes + 15) // 16 * 16 <= AC_LDS_TABLE)


def default_cfg() -> fcgpu_cfg:
    cfg = fcgpu_cfg()
    lib = _lib
    if lib is not None:
        lib.fcgpu_default_cfg(C.byref(cfg))
    else:
        # same values as fcgpu_default_cfg (fcgpu_context.hip)
        cfg.size = C.sizeof(fcgpu_cfg)
        cfg.check_mode = CHECK_IP4
        cfg.hash_mode = HASH_FLOWID
        cfg.classify = CLS_NONE
        cfg.nports = 1
        cfg.hs_length = 1
        cfg.nbad6 = 1
        cfg.l4_checksum = 1
        for j in range(16):
            cfg.bad6[0][j] = 0xFF
    return cfg


def make_cfg(*, check_mode=CHECK_IP4, offset=0, checksum=False, hash_mode=HASH_FLOWID,
             classify=CLS_NONE, nports=1, hs_offset=0, hs_length=1, native_vlan=0,
             badsrc=(), gooddst=(), bad6=None, process_eh=False, l4_mode=L4_NONE,
             l4_checksum=True, rewrite=0, ttl_multicast=True, vlan_ethertype=0) -> fcgpu_cfg:
    """Build an fcgpu_cfg. Addresses are raw network-order words (bytes a.b.c.d
    -> little-endian u32 of those bytes), as IPAddress stores them."""
    cfg = default_cfg()
    cfg.check_mode = check_mode
    cfg.offset = offset
    cfg.checksum = 1 if checksum else 0
    cfg.hash_mode = hash_mode
    cfg.classify = classify
    cfg.nports = nports
    cfg.hs_offset = hs_offset
    cfg.hs_length = hs_length
    cfg.native_vlan = native_vlan
    cfg.nbadsrc = len(badsrc)
    for j, a in enumerate(badsrc):
        cfg.badsrc[j] = a
    cfg.ngooddst = len(gooddst)
    for j, a in enumerate(gooddst):
        cfg.gooddst[j] = a
    cfg.process_eh = 1 if process_eh else 0
    cfg.l4_mode = l4_mode
    cfg.l4_checksum = 1 if l4_checksum else 0
    cfg.rewrite = rewrite
    cfg.ttl_multicast = 1 if ttl_multicast else 0
    cfg.vlan_ethertype = vlan_ethertype
    if bad6 is not None:
        cfg.nbad6 = len(bad6)
        for j, a in enumerate(bad6):
            for k in range(16):
                cfg.bad6[j][k] = a[k]
    return cfg


def derive_counters(vec):
    """fcgpu_counters_derive on a summed counter vector (numpy / list of
    NCOUNTERS): drops = checker reason slots, count = all packets - drops."""
    import numpy as np
    v = np.array(vec, dtype=np.uint64).copy()
    drops = int(v[CTR_REASON:CTR_REASON + reason_slot(R_NO_MATCH)].sum())
    total = int(v[CTR_PORT:CTR_PORT + MAX_PORTS + 1].sum())
    v[CTR_DROPS] = drops
    v[CTR_COUNT] = total - drops
    return v


def raw_addr(dotted: str) -> int:
    """'a.b.c.d' -> raw s_addr word as read little-endian from packet bytes."""
    b = bytes(int(x) for x in dotted.split("."))
    return int.from_bytes(b, "little")


class Context:
    """Owning wrapper over an fcgpu_ctx (one per thread x stream)."""

    def __init__(self, device: int = 0, max_batch: int = 1 << 20, cfg: fcgpu_cfg | None = None):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.fcgpu_open(device, max_batch, C.byref(h))
        if rc != OK:
            raise RuntimeError(f"fcgpu_open failed ({rc}): {self.lib.fcgpu_last_error(None).decode()}")
        self.h = h
        self.max_batch = max_batch
        self.cfg = None
        if cfg is not None:
            self.configure(cfg)

    def _chk(self, rc, what):
        if rc != OK:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.fcgpu_last_error(self.h).decode()}")

    def configure(self, cfg: fcgpu_cfg):
        self._chk(self.lib.fcgpu_configure(self.h, C.byref(cfg)), "fcgpu_configure")
        self.cfg = cfg

    def process(self, arena_ptr, desc_ptr, n, *, verdict=0, hash=0, anno=0, perm=0,
                port_start=0, tile_count=0, partition=PART_GLOBAL, tile_perm=0, flowid=0, ip_rw=0,
                stream=0):
        out = fcgpu_out(verdict or None, hash or None, anno or None, perm or None,
                        port_start or None, tile_count or None, partition, 0, tile_perm or None,
                        flowid or None, ip_rw or None)
        self._chk(self.lib.fcgpu_process(self.h, arena_ptr, desc_ptr, n, C.byref(out),
                                         stream or None), "fcgpu_process")

    def process_counted(self, arena_ptr, desc_ptr, n_max, count_ptr, base=0, *, verdict=0, hash=0, anno=0,
                        perm=0, port_start=0, tile_count=0, partition=PART_TILE, tile_perm=0, flowid=0, ip_rw=0,
                        stream=0):
        """fcgpu_process_counted: the first *count_ptr - base packets (a device word) of
        at most n_max; the launch covers n_max, nothing is read back to the host."""
        out = fcgpu_out(verdict or None, hash or None, anno or None, perm or None, port_start or None,
                        tile_count or None,
                        partition, 0, tile_perm or None, flowid or None, ip_rw or None)
        self._chk(self.lib.fcgpu_process_counted(self.h, arena_ptr, desc_ptr, n_max, count_ptr, base,
                                                 C.byref(out), stream or None), "fcgpu_process_counted")

    def jobs(self, specs):
        """Prepare an fcgpu_job array from (arena_ptr, desc_ptr, n, stream, outputs-dict)
        tuples; run it with run_jobs (no per-job Python work on the launch path)."""
        arr = (fcgpu_job * max(len(specs), 1))()
        for k, (arena, desc, n, stream, o) in enumerate(specs):
            arr[k].arena = arena
            arr[k].desc = desc
            arr[k].n = n
            arr[k].stream = stream or None
            arr[k].out = fcgpu_out(o.get("verdict") or None, o.get("hash") or None, o.get("anno") or None,
                                   o.get("perm") or None, o.get("port_start") or None,
                                   o.get("tile_count") or None, o.get("partition", PART_GLOBAL), 0,
                                   o.get("tile_perm") or None, o.get("flowid") or None, o.get("ip_rw") or None)
        return arr, len(specs)

    def run_jobs(self, prepared, stream=0):
        arr, n = prepared
        self._chk(self.lib.fcgpu_process_jobs(self.h, arr, n, stream or None), "fcgpu_process_jobs")

    def pool_register(self, base: int, nbytes: int):
        """Register a packet-buffer pool (mbuf headers + data rooms) for fcgpu_process_mbufs."""
        self._chk(self.lib.fcgpu_pool_register(self.h, base, nbytes), "fcgpu_pool_register")

    def process_mbufs(self, ptrs_addr: int, n: int, layout=MBUF_LAYOUT_DPDK, stream=0, **outs):
        """ptrs_addr: host array of n mbuf pointers (uint64) inside the registered pool."""
        lay = fcgpu_mbuf_layout(*layout)
        o = fcgpu_out(outs.get("verdict") or None, outs.get("hash") or None, outs.get("anno") or None,
                      outs.get("perm") or None, outs.get("port_start") or None, outs.get("tile_count") or None,
                      outs.get("partition", PART_GLOBAL), 0, outs.get("tile_perm") or None,
                      outs.get("flowid") or None, outs.get("ip_rw") or None)
        self._chk(self.lib.fcgpu_process_mbufs(self.h, ptrs_addr, n, C.byref(lay), C.byref(o), stream or None),
                  "fcgpu_process_mbufs")

    def process_host(self, frames, lens_ptr, n, *, verdict=0, hash=0, anno=0, perm=0,
                     port_start=0, tile_count=0, partition=PART_GLOBAL, tile_perm=0, flowid=0, ip_rw=0):
        out = fcgpu_out(verdict or None, hash or None, anno or None, perm or None,
                        port_start or None, tile_count or None, partition, 0, tile_perm or None,
                        flowid or None, ip_rw or None)
        self._chk(self.lib.fcgpu_process_host(self.h, frames, lens_ptr, n, C.byref(out)),
                  "fcgpu_process_host")

    def span_submit(self, slot, span_ptr, span_bytes, desc_ptr, n, *, verdict=0, hash=0, anno=0, perm=0,
                    port_start=0, tile_count=0, partition=PART_GLOBAL, tile_perm=0, flowid=0, ip_rw=0):
        """Asynchronous: frames already contiguous in host memory (pinned for DMA)."""
        out = fcgpu_out(verdict or None, hash or None, anno or None, perm or None,
                        port_start or None, tile_count or None, partition, 0, tile_perm or None,
                        flowid or None, ip_rw or None)
        self._chk(self.lib.fcgpu_span_submit(self.h, slot, span_ptr, span_bytes, desc_ptr, n, C.byref(out)),
                  "fcgpu_span_submit")

    def span_wait(self, slot):
        self._chk(self.lib.fcgpu_span_wait(self.h, slot), "fcgpu_span_wait")

    def set_program(self, kind, steps, output_everything=-1):
        """steps: sequence of (offset, value, mask, yes, no, flags) or fcgpu_step."""
        arr = (fcgpu_step * max(len(steps), 1))()
        for i, st in enumerate(steps):
            arr[i] = st if isinstance(st, fcgpu_step) else fcgpu_step(*[int(x) for x in st])
        self._chk(self.lib.fcgpu_set_program(self.h, kind, arr, len(steps), output_everything),
                  "fcgpu_set_program")

    def set_routes(self, routes):
        """The route table of CLS_ROUTE (routes_array's forms); replaces the
        previous one."""
        r = routes_array(routes)
        self._chk(self.lib.fcgpu_set_routes(self.h, r.ctypes.data, len(r)), "fcgpu_set_routes")

    def set_routes6(self, routes):
        """The IPv6 route table of CLS_ROUTE6 (routes6_array's forms);
        replaces the previous one."""
        r = routes6_array(routes)
        self._chk(self.lib.fcgpu_set_routes6(self.h, r.ctypes.data, len(r)), "fcgpu_set_routes6")

    def set_patterns(self, patterns):
        """The patterns of CLS_STRING (a sequence of byte strings, pattern k
        -> output k); replaces the previous ones."""
        blob, lens, n = _patterns(patterns)
        self._chk(self.lib.fcgpu_set_patterns(self.h, blob, lens, n), "fcgpu_set_patterns")

    def set_lb_table(self, table):
        """The bucket -> output table of CLS_LB_TABLE (uint8 sequence)."""
        import numpy as np
        t = np.ascontiguousarray(table, dtype=np.uint8)
        self._chk(self.lib.fcgpu_set_lb_table(self.h, t.ctypes.data, len(t)), "fcgpu_set_lb_table")

    def program_jit(self, enable=True):
        """Compile the installed (and later) decision programs to code (hiprtc)."""
        self._chk(self.lib.fcgpu_program_jit(self.h, int(enable)), "fcgpu_program_jit")

    def program_jit_active(self) -> bool:
        return bool(self.lib.fcgpu_program_jit_active(self.h))

    def flow_enable(self, max_flows: int):
        """Device flow table (FlowIPManagerHMP semantics); 0 disables it."""
        self._chk(self.lib.fcgpu_flow_enable(self.h, max_flows), "fcgpu_flow_enable")

    def flow_configure(self, manager=FLOW_MGR_IMP, capacity=65536, timeout_s=0, recycle_ms=1000):
        """Flow manager: FLOW_MGR_HMP (IDs 0, 1, ...) or FLOW_MGR_IMP (free-ID
        stack, timeouts on a timer wheel); capacity 0 disables the table."""
        fc = fcgpu_flow_config(manager, capacity, timeout_s, recycle_ms)
        self._chk(self.lib.fcgpu_flow_configure(self.h, C.byref(fc)), "fcgpu_flow_configure")

    def flow_set_time(self, now_ms: int):
        self._chk(self.lib.fcgpu_flow_set_time(self.h, now_ms & 0xFFFFFFFF), "fcgpu_flow_set_time")

    def flow_maintain(self, now_ms: int, stream=None):
        self._chk(self.lib.fcgpu_flow_maintain(self.h, now_ms & 0xFFFFFFFF, stream), "fcgpu_flow_maintain")

    def flow_stats(self) -> dict:
        st = fcgpu_flow_stat()
        self._chk(self.lib.fcgpu_flow_stats(self.h, C.byref(st)), "fcgpu_flow_stats")
        return {k: getattr(st, k) for k, _ in fcgpu_flow_stat._fields_}

    def flow_reset(self):
        self._chk(self.lib.fcgpu_flow_reset(self.h), "fcgpu_flow_reset")

    def flow_count(self) -> int:
        v = C.c_uint32()
        self._chk(self.lib.fcgpu_flow_count(self.h, C.byref(v)), "fcgpu_flow_count")
        return v.value

    def aggcount_configure(self, capacity, bytes=False, ip_bytes=False, mask=0xFFFFFFFF):
        """AggregateCounter behind the classifier (fcgpu_aggcount_configure):
        one count per distinct hash & mask of the packets that leave with R_OK,
        at most `capacity` of them; packets, or with bytes their trimmed
        length (ip_bytes: from the network header on). 0 disables it."""
        ac = fcgpu_aggcount_config(capacity, int(bytes), int(ip_bytes), mask)
        self._chk(self.lib.fcgpu_aggcount_configure(self.h, C.byref(ac)), "fcgpu_aggcount_configure")

    def aggcount_freeze(self, frozen=True):
        self._chk(self.lib.fcgpu_aggcount_freeze(self.h, int(frozen)), "fcgpu_aggcount_freeze")

    def aggcount_reset(self):
        self._chk(self.lib.fcgpu_aggcount_reset(self.h), "fcgpu_aggcount_reset")

    def aggcount_stats(self) -> dict:
        st = fcgpu_aggcount_stat()
        self._chk(self.lib.fcgpu_aggcount_stats(self.h, C.byref(st)), "fcgpu_aggcount_stats")
        return {k: getattr(st, k) for k, _ in fcgpu_aggcount_stat._fields_}

    def aggcount_read(self):
        """(aggregates uint32, counts uint64): the non-zero counts, sorted by
        aggregate (AggregateCounter's write_file order)."""
        import numpy as np
        n = C.c_uint32()
        self._chk(self.lib.fcgpu_aggcount_read(self.h, None, 0, C.byref(n)), "fcgpu_aggcount_read")
        rec = np.zeros(n.value, dtype=[("agg", "<u4"), ("reserved", "<u4"), ("count", "<u8")])
        self._chk(self.lib.fcgpu_aggcount_read(self.h, rec.ctypes.data, n.value, C.byref(n)), "fcgpu_aggcount_read")
        return rec["agg"][:n.value].copy(), rec["count"][:n.value].copy()

    def espauth_set_sas(self, sas):
        """ESP authentication behind the classifier (fcgpu_espauth_set_sas):
        sas is a sequence of (spi, 16-byte key); every later process() batch
        gets one record per packet (espauth_records). Empty: disabled."""
        import numpy as np
        arr = np.zeros(len(sas), dtype=[("spi", "<u4"), ("key", "u1", 16)])
        for k, (spi, key) in enumerate(sas):
            arr[k] = (spi, np.frombuffer(bytes(key), np.uint8))
        self._chk(self.lib.fcgpu_espauth_set_sas(self.h, arr.ctypes.data, len(sas)), "fcgpu_espauth_set_sas")

    def espauth_configure(self, mode=ESP_VERIFY):
        ec = fcgpu_espauth_config(mode)
        self._chk(self.lib.fcgpu_espauth_configure(self.h, C.byref(ec)), "fcgpu_espauth_configure")

    def espauth_records_ptr(self) -> int:
        p = C.c_void_p()
        self._chk(self.lib.fcgpu_espauth_records(self.h, C.byref(p)), "fcgpu_espauth_records")
        return p.value or 0

    def espauth_records(self, n: int):
        """The first n records of the last process() batch as a numpy
        structured array (status u1, icv 12 x u1); synchronises the device."""
        import numpy as np
        import torch
        dt = np.dtype([("status", "u1"), ("pad", "u1", 3), ("icv", "u1", 12)])
        ptr = self.espauth_records_ptr()
        if not ptr:
            raise RuntimeError("espauth_records: the stage is not enabled (espauth_set_sas)")
        if not n:
            return np.zeros(0, dt)

        class _Dev:     # the context's array, seen by torch without a copy
            __cuda_array_interface__ = {"shape": (n * dt.itemsize,), "typestr": "|u1", "data": (ptr, False),
                                        "version": 2}
        torch.cuda.synchronize()
        return torch.as_tensor(_Dev(), device="cuda").cpu().numpy().view(dt).copy()

    def espauth_stats(self) -> dict:
        st = fcgpu_espauth_stat()
        self._chk(self.lib.fcgpu_espauth_stats(self.h, C.byref(st)), "fcgpu_espauth_stats")
        return {k: getattr(st, k) for k, _ in fcgpu_espauth_stat._fields_}

    def espauth_reset(self):
        self._chk(self.lib.fcgpu_espauth_reset(self.h), "fcgpu_espauth_reset")

    def espaes_set_sas(self, sas):
        """ESP decryption in front of the authentication stage
        (fcgpu_espaes_set_sas): sas is a sequence of (spi, 16-byte AES key);
        every later process() batch is decrypted IN PLACE in its arena and
        gets one status byte per packet (espaes_status). Empty: disabled."""
        import numpy as np
        arr = np.zeros(len(sas), dtype=[("spi", "<u4"), ("key", "u1", 16)])
        for k, (spi, key) in enumerate(sas):
            arr[k] = (spi, np.frombuffer(bytes(key), np.uint8))
        self._chk(self.lib.fcgpu_espaes_set_sas(self.h, arr.ctypes.data, len(sas)), "fcgpu_espaes_set_sas")

    def espaes_configure(self, mode=ESPAES_DECRYPT):
        """ESPAES_DECRYPT (k_espaes in front of the authentication stage) or
        ESPAES_ENCRYPT (k_espenc behind it: with espauth_configure(ESP_SEAL)
        one process() call seals and encrypts) for the batches that follow."""
        ec = fcgpu_espaes_config(mode)
        self._chk(self.lib.fcgpu_espaes_configure(self.h, C.byref(ec)), "fcgpu_espaes_configure")

    def espaes_status_ptr(self) -> int:
        p = C.c_void_p()
        self._chk(self.lib.fcgpu_espaes_status(self.h, C.byref(p)), "fcgpu_espaes_status")
        return p.value or 0

    def espaes_status(self, n: int):
        """The first n status bytes (ESP_*) of the last process() batch as a
        numpy array; synchronises the device."""
        import numpy as np
        import torch
        ptr = self.espaes_status_ptr()
        if not ptr:
            raise RuntimeError("espaes_status: the stage is not enabled (espaes_set_sas)")
        if not n:
            return np.zeros(0, np.uint8)

        class _Dev:     # the context's array, seen by torch without a copy
            __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}
        torch.cuda.synchronize()
        return torch.as_tensor(_Dev(), device="cuda").cpu().numpy().copy()

    def espaes_stats(self) -> dict:
        st = fcgpu_espaes_stat()
        self._chk(self.lib.fcgpu_espaes_stats(self.h, C.byref(st)), "fcgpu_espaes_stats")
        return {k: getattr(st, k) for k, _ in fcgpu_espaes_stat._fields_}

    def espaes_reset(self):
        self._chk(self.lib.fcgpu_espaes_reset(self.h), "fcgpu_espaes_reset")

    def set_host_threads(self, n: int):
        self._chk(self.lib.fcgpu_set_host_threads(self.h, n), "fcgpu_set_host_threads")

    def counters(self, n=NCOUNTERS):
        buf = (C.c_uint64 * n)()
        self._chk(self.lib.fcgpu_read_counters(self.h, buf, n), "fcgpu_read_counters")
        return list(buf)

    def reset_counters(self):
        self._chk(self.lib.fcgpu_reset_counters(self.h), "fcgpu_reset_counters")

    def counters_device_ptr(self) -> int:
        p = C.c_void_p()
        self._chk(self.lib.fcgpu_counters_device(self.h, C.byref(p)), "fcgpu_counters_device")
        return p.value

    def use_counters(self, dptr: int):
        self._chk(self.lib.fcgpu_use_counters(self.h, dptr or None), "fcgpu_use_counters")

    def set_timing(self, every):
        """every: bracket every k-th launch with events (True = 1, False/0 = off)."""
        self._chk(self.lib.fcgpu_set_timing(self.h, int(every)), "fcgpu_set_timing")

    def read_timing(self):
        ms = (C.c_double * 3)()
        cnt = (C.c_uint32 * 3)()
        self._chk(self.lib.fcgpu_read_timing(self.h, ms, cnt, 3), "fcgpu_read_timing")
        return list(ms), list(cnt)

    def exchange_plan(self, desc, perm, port_start, n, world, rank, meta, seg_bytes, stream=0):
        """fcgpu_exchange_plan on device pointers (flow re-shard, one record per leaving packet)."""
        self._chk(self.lib.fcgpu_exchange_plan(self.h, desc, perm, port_start, n, world, rank, meta, seg_bytes,
                                               stream or None), "fcgpu_exchange_plan")

    def exchange_pack(self, arena, port_start, meta, seg_bytes, n, world, send, send_cap, stream=0):
        """fcgpu_exchange_pack: the leaving frames into their owners' segments of send
        (after exchange_plan of the same batch on this context)."""
        self._chk(self.lib.fcgpu_exchange_pack(self.h, arena, port_start, meta, seg_bytes, n, world,
                                               send or None, send_cap, stream or None), "fcgpu_exchange_pack")

    def exchange_build(self, arena, desc, verdict, n, world, rank, meta, seg_n, seg_bytes, send, send_cap,
                       stream=0):
        """fcgpu_exchange_build on device pointers: records and send buffer from the owner pass's verdicts."""
        self._chk(self.lib.fcgpu_exchange_build(self.h, arena, desc, verdict, n, world, rank, meta, seg_n,
                                                seg_bytes, send or None, send_cap, stream or None),
                  "fcgpu_exchange_build")

    def exchange_build_fixed(self, arena, desc, verdict, n, world, rank, seg_recs, seg_bytes, meta, send,
                             stream=0):
        """fcgpu_exchange_build_fixed on device pointers: every owner's segment at its
        fixed place (header + seg_recs records; seg_bytes frame bytes)."""
        self._chk(self.lib.fcgpu_exchange_build_fixed(self.h, arena, desc, verdict, n, world, rank, seg_recs,
                                                      seg_bytes, meta, send, stream or None),
                  "fcgpu_exchange_build_fixed")

    def exchange_unpack_fixed(self, rmeta, world, seg_recs, seg_bytes, desc, count, stall, step, total=0,
                              stream=0):
        """fcgpu_exchange_unpack_fixed: received fixed segments -> descriptors, *count, *stall
        (and *total += count when total is given)."""
        self._chk(self.lib.fcgpu_exchange_unpack_fixed(self.h, rmeta, world, seg_recs, seg_bytes, desc, count,
                                                       stall, total or None, step, stream or None),
                  "fcgpu_exchange_unpack_fixed")

    def exchange_unpack(self, meta, n, src_displ, desc, stream=0):
        """fcgpu_exchange_unpack: received records -> descriptors (src_displ: per-source segment starts)."""
        arr = (C.c_uint64 * max(len(src_displ), 1))(*[int(x) for x in src_displ])
        self._chk(self.lib.fcgpu_exchange_unpack(self.h, meta, n, arr, len(src_displ), desc, stream or None),
                  "fcgpu_exchange_unpack")

    def close(self):
        if getattr(self, "h", None):
            self.lib.fcgpu_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
