/*
 * fastclick_gpu.h -- C ABI of the MI355X receive-path element library
 * (libfcgpu.so, HIP for gfx950).
 *
 * One call processes one batch of packets through the fused chain
 *
 *     [StripEtherVLANHeader] -> CheckIPHeader | CheckIP6Header | MarkIPHeader
 *         -> AggregateHash (IPFlowID / IPFlow5ID / IP6FlowID low-32 hash)
 *         -> per-port classify (FlowSwitch LB hash, LB hash_ip, HashSwitch)
 *         -> stable per-port partition (CLASSIFY_EACH_PACKET)
 *
 * and replaces, for a FastClick BatchElement, the per-packet loops
 *   - CheckIPHeader::valid            elements/ip/checkipheader.cc:163-226
 *   - click_in_cksum                  lib/in_cksum.c:20-51
 *   - IPFlowID::hashcode              include/click/ipflowid.hh:153-164
 *   - IPFlow5ID::hashcode             include/click/ipflowid.hh:242-251
 *   - AggregateHash::simple_action    elements/analysis/aggregatehash.cc:49-55
 *   - LoadBalancer::pick_server       include/click/loadbalancer.hh:553-584
 *   - HashSwitch::process             elements/standard/hashswitch.cc:50-66
 *   - StripEtherVLANHeader::simple_action elements/ethernet/stripethervlanheader.cc:48-61
 *   - CheckIP6Header::simple_action   elements/ip6/checkip6header.cc:105-168
 *   - IP6FlowID::hashcode             include/click/ip6flowid.hh:220-230
 *   - CLASSIFY_EACH_PACKET            include/click/packetbatch.hh:259-307
 * (SURVEY.md section 8(a) rows A1-A15). The FastClick-side caller is the
 * GPUIPCheckClassify element (fastclick_amd/csrc/host/), which keeps the
 * Element::push_batch API (include/click/element.hh:53-54) and calls this ABI.
 *
 * Batch layout ("arena + descriptor"):
 *   arena : bytes; packet i's frame starts at arena + desc[2i] and is
 *           desc[2i+1] bytes long. The arena must stay readable for 128 bytes
 *           past every frame start and 16 bytes past every frame end
 *           (header-window over-read; bytes outside the frame never decide a
 *           verdict).
 *   desc  : uint32 pairs (offset, length), 8 bytes per packet.
 * Results are per-packet structure-of-arrays; every output pointer may be NULL
 * (that output is then not produced).
 *
 * Errors: every int-returning entry point returns FCGPU_OK (0) or a negative
 * FCGPU_E* code; fcgpu_last_error() gives the message. There is no silent
 * fallback: a missing device or a failed launch is an error return.
 */
#ifndef FASTCLICK_GPU_H
#define FASTCLICK_GPU_H

#ifndef __HIPCC_RTC__   /* hiprtc (fcgpu_set_program's compiled programs) has its own */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FCGPU_ABI_VERSION 32

#define FCGPU_OK          0
#define FCGPU_EINVAL     -1   /* bad argument / configuration            */
#define FCGPU_ENODEV     -2   /* no HIP device / device not usable       */
#define FCGPU_ENOMEM     -3   /* allocation failed / batch > max_batch   */
#define FCGPU_ERUNTIME   -4   /* HIP runtime or kernel launch failure    */

/* Verdict reason codes. 0..6 are CheckIPHeader::Reason
 * (elements/ip/checkipheader.hh:139-147); 6 = NREASONS = valid. */
#define FCGPU_R_MINISCULE   0
#define FCGPU_R_BAD_VERSION 1
#define FCGPU_R_BAD_HLEN    2
#define FCGPU_R_BAD_IP_LEN  3
#define FCGPU_R_BAD_CKSUM   4
#define FCGPU_R_BAD_SADDR   5
#define FCGPU_R_OK          6
#define FCGPU_R_BAD_IP6     7   /* CheckIP6Header's single drop reason      */
#define FCGPU_R_VLAN_REJECT 8   /* StripEtherVLANHeader output 1 (untagged, NATIVE_VLAN < 0) */
#define FCGPU_R_NO_MATCH    9   /* valid, but the classifier program matched no output:
                                   CLASSIFY_EACH_PACKET kills it (packetbatch.hh:268)  */
/* CheckUDPHeader / CheckTCPHeader::Reason (elements/tcpudp/checkudpheader.hh:83-87,
 * checktcpheader.hh:83-87) for IPv4-valid packets, when l4_mode is set: */
#define FCGPU_R_L4_PROTO    10  /* NOT_UDP / NOT_TCP                         */
#define FCGPU_R_L4_LENGTH   11  /* BAD_LENGTH                                */
#define FCGPU_R_L4_CKSUM    12  /* BAD_CHECKSUM (pseudo-header checksum)     */
/* Header rewrite stage (cfg.rewrite), after the classifier, on packets it let through: */
#define FCGPU_R_TTL_EXPIRED 13  /* DecIPTTL output 1: ip_ttl <= 1 (decipttl.cc:62-65)          */
#define FCGPU_R_SETCKSUM_BAD 14 /* SetIPChecksum "bad input packet": kill (setipchecksum.cc:44-56) */
#define FCGPU_NREASON_SLOTS 14  /* counters for reasons 0-5, 7-14            */
/* Reasons >= FCGPU_R_NO_MATCH are decided after CheckIPHeader accepted the
 * packet: they count in "count", not in "drops". */

/* check_mode */
#define FCGPU_CHECK_IP4   0   /* CheckIPHeader(OFFSET o[, CHECKSUM c, BADSRC, GOODDST]) */
#define FCGPU_MARK_IP4    1   /* MarkIPHeader(o): no validation                         */
#define FCGPU_CHECK_AUTO  2   /* StripEtherVLANHeader(NATIVE_VLAN) at o, then by IP version
                                 nibble: 6 -> CheckIP6Header, else -> CheckIPHeader.
                                 With vlan_ethertype: VLANDecap(ETHERTYPE) + Strip(14)
                                 (elements/ethernet/vlandecap.cc:49-70): same offsets,
                                 untagged -> tci 0 (native_vlan 0)                     */
#define FCGPU_MARK_IP6    3   /* MarkIP6Header(o) (elements/ip6/markip6header.cc:43-48): no
                                 validation, nh = o, th = o + 40; IP6FlowID hash        */
/* hash_mode (written to the AGGREGATE annotation output) */
#define FCGPU_HASH_NONE     0
#define FCGPU_HASH_FLOWID   1   /* IPFlowID(p).hashcode() low 32 (AggregateHash); v6: IP6FlowID */
#define FCGPU_HASH_FLOW5ID  2   /* IPFlow5ID(p).hashcode() low 32 (adds ip_p)               */
/* classify */
#define FCGPU_CLS_NONE       0  /* every valid packet -> port 0                          */
#define FCGPU_CLS_LB_HASH    1  /* LoadBalancer direct_hash / direct_hash_agg:
                                   ((H>>16) ^ (H&0xffff)) % nports                       */
#define FCGPU_CLS_HASH_IP    2  /* LoadBalancer direct_hash_ip (frame bytes 26..33)      */
#define FCGPU_CLS_HASHSWITCH 3  /* HashSwitch(hs_offset, hs_length), nports = MAX        */
#define FCGPU_CLS_PROGRAM    4  /* decision program set by fcgpu_set_program: IPFilter /
                                   IPClassifier or Classifier                          */
#define FCGPU_CLS_LB_CRC     5  /* LoadBalancer direct_hash_crc (DPDK builds,
                                   include/click/loadbalancer.hh:563-569): c = CRC32-C of
                                   the IPFlow5ID words proto, saddr, daddr, ports from 0
                                   (ipv4_hash_crc, include/click/dpdk_glue.hh:13-27, via
                                   rte_hash_crc_4byte = the SSE4.2 crc32 instruction), port =
                                   ((c>>16) ^ (c&0xffff)) % nports. IPv4 check modes only */
#define FCGPU_CLS_LB_TABLE   6  /* LoadBalancer constant_hash_agg (include/click/
                                   loadbalancer.hh:585-589): port = table[((H>>16) ^
                                   (H&0xffff)) % buckets], H the hash_mode hash; the table
                                   (the reference's consistent-hash ring, :170-189) is set
                                   by fcgpu_set_lb_table */
#define FCGPU_CLS_ROUTE      7  /* IPRouteTable::process (elements/ip/iproutetable.cc:152-169):
                                   longest-prefix lookup of the DST_IP annotation in the
                                   table set by fcgpu_set_routes; the route's output, its
                                   gateway (if any) into the annotation; no route ->
                                   FCGPU_R_NO_MATCH. The annotation is the header's ip_dst
                                   word, as after GetIPAddress(16) (MARK_IP4, which sets
                                   none itself, gets it too). IPv4 check modes only */
#define FCGPU_CLS_ROUTE6     8  /* LookupIP6Route behind GetIP6Address(24) (elements/ip6/
                                   lookupip6route.cc:98-149): longest-prefix lookup of the
                                   header's ip6_dst in the table set by fcgpu_set_routes6;
                                   the route's output, its gateway *id* into anno.dst_ip
                                   (0: no gateway, and for a packet without a route); no
                                   route -> FCGPU_R_NO_MATCH. CHECK_AUTO and MARK_IP6 only.
                                   MARK_IP6 checks no length, as GetIP6Address does not: a
                                   frame shorter than nh + 40 is looked up on whatever bytes
                                   follow it (inside the arena's slack), whatever hash_mode.
                                   Under CHECK_AUTO an IPv4 packet is looked up as
                                   FCGPU_CLS_ROUTE does in the table of fcgpu_set_routes
                                   (none set: no route); anno.ipver tells which meaning
                                   dst_ip has */
#define FCGPU_CLS_STRING     9  /* StringClassifier (elements/ids/stringclassifier.cc:94-101)
                                   over the patterns set by fcgpu_set_patterns: the packet
                                   goes to the output of AhoCorasick::match_first's pattern
                                   (ahocorasickplus.hh:113-123, ahocorasick.c:177-243,
                                   node.c:425-442) -- the one whose match ends earliest, of
                                   several ending there the longest; output = its index in
                                   the list. No match -> output npatterns, and where that
                                   output does not exist (npatterns == nports)
                                   FCGPU_R_NO_MATCH, as checked_output_push kills it. The
                                   text is the frame from its descriptor offset (byte 0,
                                   link header included) up to anno.length, i.e. after
                                   CheckIPHeader's trim to ip_len (MARK_IP4: the whole
                                   frame): a pattern found only in padding past ip_len is no
                                   match. IPv4 check modes only; served by fcgpu_process and
                                   fcgpu_process_jobs */

/* l4_mode: a CheckUDPHeader / CheckTCPHeader after the IPv4 check (CHECK_IP4 or
 * MARK_IP4 only). The checksum covers the whole L4 segment, so with
 * l4_checksum the device reads every byte of the packet, not only the header
 * window. */
#define FCGPU_L4_NONE 0
#define FCGPU_L4_UDP  1
#define FCGPU_L4_TCP  2

/* rewrite flags: header rewrites after the classifier on IPv4 packets it sent
 * to an output. The rewritten bytes 8..11 of the IP header
 * (ttl, protocol, checksum) come back in fcgpu_out.ip_rw; with
 * FCGPU_RW_INPLACE they are also stored into the arena (device path). */
#define FCGPU_RW_DECTTL   1u  /* DecIPTTL: ttl <= 1 -> FCGPU_R_TTL_EXPIRED, else ttl-1 and the
                                 RFC 1624 incremental checksum (elements/ip/decipttl.cc:52-78) */
#define FCGPU_RW_SETCKSUM 2u  /* SetIPChecksum: full header checksum (elements/ip/setipchecksum.cc:38-58),
                                 after DecIPTTL when both are set                          */
#define FCGPU_RW_INPLACE  4u

#define FCGPU_MAX_PORTS   64
#define FCGPU_MAX_ADDRS   16

typedef struct fcgpu_cfg {
    uint32_t size;            /* = sizeof(fcgpu_cfg)                                     */
    uint32_t check_mode;      /* FCGPU_CHECK_*                                           */
    int32_t  offset;          /* OFFSET: frame start -> IP header (CHECK_IP4/MARK_IP4),
                                 or frame start -> Ethernet header (CHECK_AUTO)          */
    uint32_t checksum;        /* CHECKSUM; the reference default is FALSE
                                 (elements/ip/checkipheader.cc:110)          */
    uint32_t hash_mode;       /* FCGPU_HASH_*                                            */
    uint32_t classify;        /* FCGPU_CLS_*                                             */
    uint32_t nports;          /* classify outputs N (1..FCGPU_MAX_PORTS)                 */
    int32_t  hs_offset;       /* HashSwitch OFFSET (frame-relative)                      */
    int32_t  hs_length;       /* HashSwitch LENGTH (> 0)                                 */
    int32_t  native_vlan;     /* StripEtherVLANHeader NATIVE_VLAN (default 0; <0 reject) */
    uint32_t nbadsrc;         /* BADSRC list (raw network-order s_addr words)            */
    uint32_t ngooddst;        /* GOODDST list                                             */
    uint32_t badsrc[FCGPU_MAX_ADDRS];
    uint32_t gooddst[FCGPU_MAX_ADDRS];
    uint32_t nbad6;           /* CheckIP6Header bad source list; default = {ff..ff}      */
    uint8_t  bad6[FCGPU_MAX_ADDRS][16];
    uint32_t process_eh;      /* CheckIP6Header PROCESS_EH: follow hop-by-hop, routing,
                                 fragment and AH extension headers (ip6_follow_eh,
                                 include/click/ip6address.hh:417-448)                    */
    uint32_t l4_mode;         /* FCGPU_L4_*                                               */
    uint32_t l4_checksum;     /* CheckUDPHeader/CheckTCPHeader CHECKSUM (reference default
                                 TRUE: checkudpheader.cc:54, checktcpheader.cc)          */
    uint32_t rewrite;         /* FCGPU_RW_* (IPv4 check modes)                            */
    uint32_t ttl_multicast;   /* DecIPTTL MULTICAST (default true: decrement multicast too) */
    uint32_t vlan_ethertype;  /* CHECK_AUTO tag protocol: 0x8100 (StripEtherVLANHeader, and
                                 VLANDecap's default) or VLANDecap ETHERTYPE (e.g. 0x88a8) */
} fcgpu_cfg;

/* Optional per-packet annotations (16 B), mirroring what the reference
 * elements leave on a valid packet. Offsets are relative to the frame start the
 * element received (the descriptor offset). */
typedef struct fcgpu_anno {
    uint32_t dst_ip;          /* DST_IP_ANNO (IPv4 valid) = raw ip_dst word             */
    uint16_t length;          /* packet length after Packet::take() trimming            */
    uint16_t vlan_tci;        /* VLAN_TCI_ANNO, raw network order (CHECK_AUTO)          */
    uint16_t nh;              /* network header offset (set_ip_header / set_ip6_header) */
    uint16_t th;              /* transport header offset (IPv6: after the extension
                                 headers when process_eh)                              */
    uint8_t  ip6_nxt;         /* IP6_NXT_ANNO (IPv6 valid)                              */
    uint8_t  ipver;           /* 4 or 6 for packets that reached a checker, else 0      */
    uint16_t reserved;
} fcgpu_anno;

/* Stable per-output partition (CLASSIFY_EACH_PACKET, packetbatch.hh:259-307),
 * selected by fcgpu_out.partition:
 *   FCGPU_PART_GLOBAL: the whole batch is one PacketBatch. perm[n] lists packet
 *       indices grouped by output in input order; output b occupies
 *       perm[port_start[b] .. port_start[b+1]). Three launches.
 *   FCGPU_PART_TILE: the batch is a sequence of FCGPU_TILE-packet PacketBatches
 *       (the element's input batches), each partitioned on its own, exactly as
 *       a ClassifyElement partitions every batch it receives. Tile t's entries
 *       are perm[t*FCGPU_TILE ...] (packet index) and/or tile_perm[t*FCGPU_TILE
 *       ...] (index within the tile, 1 byte), grouped by output;
 *       tile_count[t*(nports+1)+b] is the size of output b's run in tile t.
 *       One fused launch.                                                   */
#define FCGPU_PART_GLOBAL 0
#define FCGPU_PART_TILE   1
#define FCGPU_TILE        256

typedef struct fcgpu_out {
    uint16_t   *verdict;      /* [n] reason | (output port << 8); invalid -> port nports */
    uint32_t   *hash;         /* [n] AGGREGATE annotation (0 unless valid)               */
    fcgpu_anno *anno;         /* [n] optional annotations                                */
    uint32_t   *perm;         /* [n] packet indices grouped by output, input order kept  */
    uint32_t   *port_start;   /* GLOBAL: [nports+2] start of each output's run in perm   */
    uint16_t   *tile_count;   /* TILE: [ceil(n/FCGPU_TILE)][nports+1] run sizes          */
    uint32_t    partition;    /* FCGPU_PART_GLOBAL or FCGPU_PART_TILE                    */
    uint32_t    reserved;
    uint8_t    *tile_perm;    /* TILE: [n] index within the tile, grouped by output      */
    uint32_t   *flowid;       /* [n] flow ID from the context's flow table (fcgpu_flow_enable);
                                 FCGPU_FLOW_NONE for packets that reach no flow manager */
    uint32_t   *ip_rw;        /* [n] with cfg.rewrite: IP header bytes 8..11 after the rewrite
                                 (little-endian load: ttl | proto << 8 | checksum bytes << 16);
                                 for every packet that leaves with FCGPU_R_OK, rewritten
                                 or not (a rewritten word may be 0: compare it with the
                                 packet's bytes to see a change); 0 for the rest        */
} fcgpu_out;

typedef struct fcgpu_ctx fcgpu_ctx;

/* Counter vector layout returned by fcgpu_read_counters (uint64):
 *   [0] count (valid packets)         CheckIPHeader "count"
 *   [1] drops                         CheckIPHeader "drops"
 *   [2 .. 2+14) reason slots for reasons 0-5, 7, 8 ("drop_details") and
 *               9-14 (no classifier match, L4 checks, DecIPTTL / SetIPChecksum;
 *               not drops of the checker)
 *   [16 .. 16+nports+1) per-output packet counts, last = invalid list       */
#define FCGPU_CTR_COUNT   0
#define FCGPU_CTR_DROPS   1
#define FCGPU_CTR_REASON  2
#define FCGPU_CTR_PORT    16
#define FCGPU_NCOUNTERS   (FCGPU_CTR_PORT + FCGPU_MAX_PORTS + 1)
/* On the device the vector is kept in FCGPU_CTR_SHARDS replicas (tiles add to
 * replica tile % FCGPU_CTR_SHARDS) and summed on read, like per_thread<>
 * counters summed by PER_THREAD_SUM (include/click/sync.hh:56,384). */
#define FCGPU_CTR_SHARDS  64

int  fcgpu_abi_version(void);
int  fcgpu_device_count(void);
void fcgpu_default_cfg(fcgpu_cfg *cfg);

/* Open a context on HIP device `device` for batches of up to max_batch packets.
 * One context per (Click thread x stream); a context is not thread-safe. */
int  fcgpu_open(int device, uint32_t max_batch, fcgpu_ctx **out);
int  fcgpu_configure(fcgpu_ctx *ctx, const fcgpu_cfg *cfg);
void fcgpu_close(fcgpu_ctx *ctx);

/* Device-resident batch: arena, desc and every output pointer are device
 * memory. Asynchronous on `stream` (a hipStream_t; NULL = the HIP null stream,
 * as everywhere in HIP). Completion: synchronise that stream. */
int  fcgpu_process(fcgpu_ctx *ctx, const uint8_t *d_arena, const uint32_t *d_desc,
                   uint32_t n, const fcgpu_out *d_out, void *stream);

/* fcgpu_process for a batch whose size is known only on the device: the
 * first *d_count - base packets (at most n_max) of d_desc are processed, the
 * launch covers n_max. No host sync: what a received re-shard batch goes
 * through (fcgpu_exchange_unpack_fixed writes *d_count), in chunks of
 * max_batch (base = the chunk's first packet). Outputs are those of
 * fcgpu_process for the processed packets (per-tile counts of the tiles past
 * them are 0); a whole-batch partition (FCGPU_PART_GLOBAL with perm or
 * port_start) is refused. */
int  fcgpu_process_counted(fcgpu_ctx *ctx, const uint8_t *d_arena, const uint32_t *d_desc, uint32_t n_max,
                           const uint32_t *d_count, uint32_t base, const fcgpu_out *d_out, void *stream);

/* Several independent device-resident batches in one call -- e.g. the
 * batches of several rx queues, or a ring of batches a NIC filled: job k is
 * processed exactly as fcgpu_process(ctx, jobs[k].arena, jobs[k].desc,
 * jobs[k].n, &jobs[k].out, jobs[k].stream ? jobs[k].stream : stream), in
 * order, with one argument check and one device switch for the set. Jobs on
 * different streams run concurrently (their outputs must not overlap); that
 * is rejected when the context has a flow table or a job asks for a
 * whole-batch partition (both use context scratch). Every job is checked
 * before the first is launched.
 * Consecutive jobs of one stream whose outputs do not overlap share one
 * receive-kernel launch (up to 24 batches: the grid is their tiles end to
 * end; 8 with a flow table, whose new-flow passes follow in batch order; a
 * whole-batch partition adds one scan and one scatter launch for them all),
 * unless the context rewrites headers in place (FCGPU_RW_INPLACE: jobs may
 * share an arena) or a whole-batch partition comes without the caller's
 * verdicts or with a flow table; results are the same as one launch per job.
 * Sampled timing (fcgpu_set_timing) then counts batches: a fused launch is
 * timed when it covers a multiple of `every`, and fcgpu_read_timing reports
 * its batches as launches (time per batch = ms / launches). */
typedef struct fcgpu_job {
    const uint8_t  *arena;
    const uint32_t *desc;
    uint32_t        n;
    uint32_t        reserved;
    void           *stream;   /* hipStream_t or NULL (the call's stream)            */
    fcgpu_out       out;
} fcgpu_job;
int  fcgpu_process_jobs(fcgpu_ctx *ctx, const fcgpu_job *jobs, uint32_t njobs, void *stream);

/* Host-resident batch: frames[i] points at packet i's data (length lens[i]).
 * The first min(len, 128) bytes of every frame are gathered into pinned
 * staging, copied H2D, processed, and the requested outputs copied D2H into the
 * host pointers of h_out. Synchronous. Unless a whole-batch partition is asked
 * for (FCGPU_PART_GLOBAL with perm/port_start), the batch is pipelined in
 * chunks of 131,072 packets over three streams, so the gather of one chunk
 * overlaps the copies and kernel of the previous ones; results are identical
 * to one launch over the batch (chunks are whole 256-packet tiles). Outputs
 * are DMA'd straight into h_out arrays that are pinned (fcgpu_host_alloc),
 * otherwise through pinned staging. */
int  fcgpu_process_host(fcgpu_ctx *ctx, const uint8_t *const *frames,
                        const uint32_t *lens, uint32_t n, const fcgpu_out *h_out);

/* Host-resident batch whose frames already lie in one contiguous buffer
 * (e.g. pcap records read straight into pinned memory, include/fcpcap.h):
 * the span and the descriptors go to the device as two H2D copies -- no
 * per-packet gather -- then the kernels run and the requested outputs are
 * copied into the host pointers of h_out. Asynchronous: up to
 * FCGPU_SPAN_SLOTS submissions are in flight, each on its own stream (one
 * stream for all when a flow table is enabled, which needs batch order);
 * h_span, h_desc and h_out must stay valid until fcgpu_span_wait(slot).
 * Pinned buffers (fcgpu_host_alloc) make the copies true DMA. Every frame
 * starts inside the span (desc offsets < span_bytes: the descriptors are the
 * caller's and not checked per packet, as for fcgpu_process's arena) and the
 * span must be readable 128 bytes past every frame start (the context pads
 * its device copy; bytes past the span are never part of a verdict). */
#define FCGPU_SPAN_SLOTS 3
int  fcgpu_span_submit(fcgpu_ctx *ctx, uint32_t slot, const uint8_t *h_span, size_t span_bytes,
                       const uint32_t *h_desc, uint32_t n, const fcgpu_out *h_out);
int  fcgpu_span_wait(fcgpu_ctx *ctx, uint32_t slot);
/* Non-blocking: 1 if the slot's submission has completed (or none is in
 * flight), 0 if it is still running, < 0 on error. */
int  fcgpu_span_poll(fcgpu_ctx *ctx, uint32_t slot);

/* Block submissions: one H2D copy in, one D2H copy out per batch (instead of
 * one per array), for callers that stage into one pinned buffer -- the
 * GPUIPCheckClassify element. h_in holds the descriptors at desc_off and the
 * frames at frames_off (descriptor offsets are relative to frames_off); the
 * first in_bytes of h_in are copied, and the device copy is padded for the
 * header-window over-read. The requested outputs (FCGPU_OUT_* mask) come back
 * in h_out at the offsets fcgpu_block_layout_for() gives for (n, outputs,
 * partition) -- each array 256-B aligned, in the order of the mask bits.
 * Completion, slots and streams as fcgpu_span_submit. */
#define FCGPU_OUT_VERDICT    (1u << 0)
#define FCGPU_OUT_HASH       (1u << 1)
#define FCGPU_OUT_ANNO       (1u << 2)
#define FCGPU_OUT_PERM       (1u << 3)   /* GLOBAL: with port_start; TILE: packet indices */
#define FCGPU_OUT_PORT_START (1u << 4)   /* GLOBAL                                       */
#define FCGPU_OUT_TILE_COUNT (1u << 5)   /* TILE                                         */
#define FCGPU_OUT_TILE_PERM  (1u << 6)   /* TILE                                         */
#define FCGPU_OUT_FLOWID     (1u << 7)
#define FCGPU_OUT_IP_RW      (1u << 8)
/* Instead of FCGPU_OUT_ANNO, for the IPv4 check modes (CHECK_IP4 / MARK_IP4,
 * OFFSET < 256): 8-B annotations (fcgpu_anno8) at the layout's `anno`
 * offset -- half the bytes written back per packet. ipver is 4, vlan_tci and
 * ip6_nxt 0 for these modes; th = nh + thl. */
#define FCGPU_OUT_ANNO8      (1u << 9)
typedef struct fcgpu_anno8 {
    uint32_t dst_ip;          /* as fcgpu_anno                                            */
    uint16_t length;          /* as fcgpu_anno                                            */
    uint8_t  nh;              /* as fcgpu_anno (< 256)                                    */
    uint8_t  thl;             /* th - nh                                                  */
} fcgpu_anno8;
/* Not an output: this one submission goes through copies (H2D of h_in, D2H
 * of the results) whatever the span mode -- never zero-copy, never the shared
 * queue. What an element re-submits a failed batch with (SURVEY 8(b) Errors). */
#define FCGPU_SUBMIT_COPY    (1u << 31)
/* Not an output either: the block's descriptors are one uint32 per packet
 * (n x 4 B at a 4-B aligned desc_off) -- bits 0-15 the frame's offset from
 * frames_off in 8-B units (frames start on 8-B boundaries below 512 KiB),
 * bits 16-31 its length (< 65536) -- half the bytes a zero-copy batch reads
 * for them over PCIe. */
#define FCGPU_SUBMIT_DESC32  (1u << 30)
#define FCGPU_OUT_ABSENT     ((size_t)-1)
typedef struct fcgpu_block_layout {
    size_t verdict, hash, anno, perm, port_start, tile_count, tile_perm, flowid, ip_rw;  /* byte offsets */
    size_t bytes;                                                                       /* block size   */
} fcgpu_block_layout;
int  fcgpu_block_layout_for(const fcgpu_ctx *ctx, uint32_t n, uint32_t outputs, uint32_t partition,
                        fcgpu_block_layout *out);
int  fcgpu_span_submit_block(fcgpu_ctx *ctx, uint32_t slot, const void *h_in, size_t in_bytes,
                             size_t desc_off, size_t frames_off, uint32_t n, void *h_out, uint32_t outputs,
                             uint32_t partition);
/* Reserve every slot's device blocks (an in_bytes input block, a result block
 * for max_batch packets with these outputs) and streams now, on the calling
 * thread, instead of on the first submissions that need them. After it,
 * fcgpu_span_submit_block never allocates, frees or synchronises the device
 * -- not on its copy path, not for an FCGPU_SUBMIT_COPY re-submission while
 * other contexts' batches run on the device's shared queue -- and a block
 * larger than in_bytes is refused (FCGPU_ENOMEM). Without it the first
 * submission through copies sizes the blocks. Call it with no slot in flight
 * (FCGPU_EINVAL otherwise); again to grow the reservation. (Round 6: an
 * element's many threads must not grow device blocks while the shared queue
 * runs) */
int  fcgpu_span_reserve(fcgpu_ctx *ctx, size_t in_bytes, uint32_t outputs, uint32_t partition);

/* How span and block submissions reach the device (per context, default COPY):
 *   FCGPU_SPAN_COPY     -- one H2D copy of h_in and one D2H copy of the
 *                          results per batch, through the copy engine (the
 *                          device copy is padded for the header-window reads);
 *   FCGPU_SPAN_ZEROCOPY -- no copies: the kernels read the descriptors and
 *                          frames from h_in (fcgpu_span_submit: h_span,
 *                          h_desc) and write the results into h_out (the
 *                          h_out arrays) over PCIe, where they lie. All must
 *                          be page-locked (fcgpu_host_alloc, or
 *                          fcgpu_host_register / hipHostRegister), and the
 *                          frames readable 256 bytes past in_bytes /
 *                          span_bytes (the header-window over-read; those
 *                          bytes are never part of a verdict). The context
 *                          remembers each buffer address's device translation
 *                          until the next fcgpu_span_mode call, so a buffer
 *                          freed and replaced at the same address must be
 *                          page-locked as well. Many contexts
 *                          submitting small batches share one copy engine;
 *                          zero-copy batches only queue kernels.
 *   FCGPU_SPAN_AUTO     -- ZEROCOPY while at least 4 contexts of the process
 *                          are in AUTO mode on this device (one per element
 *                          thread), else COPY; decided at each submission.
 *                          Zero-copy block submissions of AUTO contexts then
 *                          share one queue per device: the 4th pending one, or
 *                          a wait/poll on one still pending, launches the
 *                          pending batches together (one kernel launch carries
 *                          several contexts' batches of one configuration, each
 *                          counted in its own context). Flow tables, whole-batch
 *                          partitions and in-place rewrites keep their own
 *                          launches. fcgpu_span_wait / fcgpu_span_poll of a slot
 *                          is how its batch is guaranteed to start.
 * Results are identical in every mode. Returns FCGPU_EINVAL for another mode
 * or while a slot is in flight. */
#define FCGPU_SPAN_COPY     0u
#define FCGPU_SPAN_ZEROCOPY 1u
#define FCGPU_SPAN_AUTO     2u
int  fcgpu_span_mode(fcgpu_ctx *ctx, uint32_t mode);
/* Fault injection (tests of the callers' error paths; process-wide, every
 * context): after `skip` events of kind `where` pass, the next `count` fail
 * as a HIP failure would, with FCGPU_ERUNTIME and a message:
 *   FCGPU_FAULT_SUBMIT -- fcgpu_span_submit / fcgpu_span_submit_block return
 *                         the error; nothing was queued, the slot stays free;
 *   FCGPU_FAULT_WAIT   -- fcgpu_span_submit / fcgpu_span_submit_block accept
 *                         the batch but nothing runs (an asynchronous launch
 *                         failure): its fcgpu_span_wait / fcgpu_span_poll
 *                         returns the error and frees the slot;
 *   FCGPU_FAULT_LAUNCH -- the next shared-queue launch (FCGPU_SPAN_AUTO) fails:
 *                         every batch it carried reports the error through its
 *                         owner's wait or poll;
 *   FCGPU_FAULT_ALLOC  -- a device or pinned allocation made after fcgpu_open
 *                         (scratch made on first use, span and staging blocks,
 *                         flow tables, programs) fails as out of memory: the
 *                         call returns FCGPU_ENOMEM or FCGPU_ERUNTIME and
 *                         leaves no partial state -- a group of buffers is made
 *                         whole or not at all, a flow table or program being
 *                         replaced is absent / the previous one -- so the next
 *                         call retries.
 * Events: submissions for SUBMIT and WAIT (an element's re-submission is
 * one), shared launches for LAUNCH, allocations for ALLOC. count 0 clears
 * the kind. Returns FCGPU_EINVAL for another kind. */
#define FCGPU_FAULT_SUBMIT 0u
#define FCGPU_FAULT_WAIT   1u
#define FCGPU_FAULT_LAUNCH 2u
#define FCGPU_FAULT_ALLOC  3u
int  fcgpu_inject_fault(uint32_t where, uint32_t skip, uint32_t count);

/* Host-only self-test of the launch guard every kernel launch passes (no
 * device needed): a set of malformed launches -- a partition output the
 * kernel stores through left null (tile_count under a tile partition, the
 * per-tile counts under a whole-batch one), null frames, descriptors or
 * counters, more workgroups than tiles, fused batches not end to end or too
 * many -- must all be refused. Returns how many were accepted (0 = all
 * refused), or -1 if a well-formed launch was refused. */
int  fcgpu_launch_guard_selftest(void);

/* 1 if the context's next block submission would be zero-copy (ZEROCOPY, or
 * AUTO with enough contexts), else 0 -- e.g. for an element that stages
 * smaller batches when its batches share the PCIe-read path with others. */
int  fcgpu_span_zerocopy_active(const fcgpu_ctx *ctx);

/* Decision programs. A program is the step list the
 * reference's own compiler produces and prints through the `program` handler
 * (IPFilter/IPClassifier: elements/ip/ipfilter.cc; Classifier:
 * elements/standard/classification.cc:978-991 and :1104-1140): each step loads
 * the 32-bit word at `offset`, masks it, compares with `value` and jumps to
 * `yes`/`no`; a jump > 0 is a step index, <= 0 is output -jump. A step whose
 * word is not entirely inside the packet takes `yes` if FCGPU_STEP_SHORT_YES
 * else `no` (length_checked_match, ipfilter.cc:1415-1474,
 * classification.cc:1146-1176).
 *   FCGPU_PROG_IPFILTER: offsets >= 512 address the transport header,
 *     >= 256 the network header, else the MAC header - 2 (ipfilter.hh:393-481).
 *   FCGPU_PROG_CLASSIFIER: offsets address the frame start
 *     (Classification::Wordwise::Program::match, classification.hh:372-392). */
#define FCGPU_PROG_IPFILTER   0
#define FCGPU_PROG_CLASSIFIER 1
#define FCGPU_STEP_SHORT_YES  1u
#define FCGPU_MAX_STEPS       8192

typedef struct fcgpu_step {
    int32_t  offset;
    uint32_t value;           /* bytes in packet order, read as a little-endian word */
    uint32_t mask;
    int32_t  yes;
    int32_t  no;
    uint32_t flags;           /* FCGPU_STEP_SHORT_YES */
} fcgpu_step;

/* Install a program for FCGPU_CLS_PROGRAM. output_everything >= 0 means the
 * program is empty and every packet goes to that output ("all->[N]"). */
int  fcgpu_set_program(fcgpu_ctx *ctx, uint32_t kind, const fcgpu_step *steps, uint32_t nsteps,
                       int32_t output_everything);
/* Programs compiled to code (enable != 0): the installed program, and every
 * program installed later, is also emitted as straight-line HIP (one block
 * per step with its offset, mask and value as immediates; a jump table as
 * compares over its runs) and compiled with hiprtc into the receive kernels
 * the context launches (~1-5 s per program and configuration, at this call /
 * fcgpu_set_program, or at the first launch of another configuration).
 * Results are identical to the interpreter's. A program with a cycle stays
 * interpreted (FCGPU_EINVAL here; fcgpu_set_program keeps it interpreted
 * silently). enable 0: back to the interpreter. */
int  fcgpu_program_jit(fcgpu_ctx *ctx, int enable);
/* 1 when the installed program runs as compiled code. */
int  fcgpu_program_jit_active(fcgpu_ctx *ctx);

/* The bucket -> output table of FCGPU_CLS_LB_TABLE: nbuckets entries, each
 * < the configured nports (checked here and at every submission). The folded
 * hash is < 65536, so a longer table's entries past 65535 are never read; they
 * are not kept. Synchronises the device before replacing a table. */
#define FCGPU_LB_TABLE_MAX (1u << 24)
int  fcgpu_set_lb_table(fcgpu_ctx *ctx, const uint8_t *table, uint32_t nbuckets);
/* LoadBalancer::build_hash_ring (include/click/loadbalancer.hh:170-189) over
 * the selector [0, nsel) (nsel <= FCGPU_MAX_PORTS): out[size] = the
 * constant_hash_agg ring, the table fcgpu_set_lb_table takes. Host-only (no
 * device, no context). */
int  fcgpu_lb_hash_ring(uint32_t nsel, uint32_t size, uint8_t *out);

/* The route table of FCGPU_CLS_ROUTE (StaticIPLookup's "ADDR/MASK [GW] OUT"
 * routes): addr and gw are raw network-order words (gw 0 = no gateway: the
 * packet keeps its DST_IP annotation), plen the prefix length (addr &= mask is
 * applied, iproutetable.cc:41), port the output. fcgpu_set_routes replaces the
 * context's table (n 0: an empty table, every packet has no route); a second
 * route for one addr/plen ("conflict with existing route"), plen > 32, a port
 * >= the configured nports (checked here and at every submission), more than
 * 32767 distinct (gw, port) next hops, or a table that needs more than 32767
 * 256-entry trie chunks is FCGPU_EINVAL and keeps the previous table, as an
 * allocation failure does. On the device the table is a 16-8-8 multibit trie
 * of 16-bit entries: 128 KiB + 512 B per chunk + 8 B per next
 * hop. Synchronises the device before replacing a table. */
typedef struct fcgpu_route {
    uint32_t addr, gw;        /* raw network order                                        */
    uint8_t  plen;            /* 0..32                                                    */
    uint8_t  port;            /* output                                                   */
    uint16_t reserved;
} fcgpu_route;
int  fcgpu_set_routes(fcgpu_ctx *ctx, const fcgpu_route *routes, uint32_t n);
/* IPRouteTable::lookup_route over the same trie, walked as the device walks
 * it: the output port of addr's longest matching prefix, or -1 (no route);
 * *gw (may be NULL) = its gateway, 0 if none. nports 0: outputs unbounded.
 * -2 for a route list fcgpu_set_routes would refuse (-1 is "no route";
 * fcgpu_last_error(NULL) has the message). Host-only (no device, no context). */
int  fcgpu_route_lookup(const fcgpu_route *routes, uint32_t n, uint32_t nports, uint32_t addr, uint32_t *gw);

/* The route table of FCGPU_CLS_ROUTE6 (LookupIP6Route's "ADDR/PLEN [GW] OUT"
 * routes): addr and gw are the 16 address bytes in network order (gw all zero
 * = no gateway), plen the prefix length 0..128 (addr &= mask is applied; only
 * contiguous masks exist here), port the output. A second route for one
 * addr/plen replaces the first, as IP6Table::add does (lib/ip6table.cc:52-73).
 * fcgpu_anno has no room for a 16-byte gateway, so a routed IPv6 packet's
 * anno.dst_ip is a gateway id: 0 for a route without gateway, else 1 + the
 * position of the route's gateway among the distinct non-zero gateways in
 * order of first appearance in `routes` -- the caller can number them itself.
 * fcgpu_set_routes6 replaces the context's table (n 0: an empty table); plen >
 * 128, a port >= the configured nports (checked here and at every submission,
 * for the IPv4 table of a dual-stack context too), more than 32767 distinct
 * (gateway id, port) next hops, or a device image above 256 MiB is
 * FCGPU_EINVAL and keeps the previous table, as an allocation failure does. On
 * the device the table is a path-compressed 16-8-...-8 trie of 32-bit entries
 * (DESIGN.md 3.7): 256 KiB + 1040 B per surviving chunk + 8 B per next hop.
 * Synchronises the device before replacing a table. */
typedef struct fcgpu_route6 {
    uint8_t  addr[16], gw[16];
    uint8_t  plen;            /* 0..128                                                   */
    uint8_t  port;            /* output                                                   */
    uint16_t reserved;
} fcgpu_route6;
int  fcgpu_set_routes6(fcgpu_ctx *ctx, const fcgpu_route6 *routes, uint32_t n);
/* The same trie walked as the device walks it: the output port of addr's
 * longest matching prefix, or -1 (no route); *gw_id (may be NULL) = its gateway
 * id. nports 0: outputs unbounded. -2 for a route list fcgpu_set_routes6 would
 * refuse (fcgpu_last_error(NULL) has the message). Host-only. */
int  fcgpu_route6_lookup(const fcgpu_route6 *routes, uint32_t n, uint32_t nports, const uint8_t addr[16],
                         uint32_t *gw_id);
/* The trie's shape: the chunks that survive path compression, and the longest
 * walk in dependent loads (the root load + one per chunk; the next hop is not
 * counted). FCGPU_EINVAL for a refused list. Host-only. */
int  fcgpu_route6_stats(const fcgpu_route6 *routes, uint32_t n, uint32_t *chunks, uint32_t *max_loads);

/* The patterns of FCGPU_CLS_STRING: n byte strings concatenated in `bytes`,
 * lens[k] the length of pattern k (1..1024, AC_PATTRN_MAX_LENGTH,
 * actypes.h:165); pattern k's output is k. fcgpu_set_patterns replaces the
 * context's automaton (n 0: nothing matches). An empty or over-long pattern,
 * a duplicate (the reference drops a duplicate with a warning and then counts
 * its no-match output one too high; here it is refused), more patterns than
 * the configured nports (checked here and at every submission), more than
 * 65535 automaton states or a device image above 32 MiB is FCGPU_EINVAL and
 * keeps the previous automaton, as an allocation failure does (the automaton
 * and the per-packet scratch of the payload pre-pass, max_batch words made
 * with the first table, are allocated as one group). On the device the
 * automaton is a byte-class map and a dense uint16 DFA, which
 * a pre-pass kernel runs over every frame before k_rx. Refused while a span
 * submission is queued; synchronises the device before replacing a table.
 * A CLS_STRING context's jobs (fcgpu_process_jobs) share one stream and are
 * not fused; fcgpu_process_host, fcgpu_process_counted, fcgpu_process_mbufs,
 * fcgpu_span_submit and fcgpu_span_submit_block return FCGPU_EINVAL. */
int  fcgpu_set_patterns(fcgpu_ctx *ctx, const uint8_t *bytes, const uint32_t *lens, uint32_t n);
/* The same automaton walked on the host: the id of match_first's pattern in
 * text[0, len), or -1 (no match); *end (may be NULL) = the match's end
 * position (1..len; 0 without a match). nports 0: ids unbounded. -2 for a list
 * fcgpu_set_patterns would refuse (fcgpu_last_error(NULL) has the message).
 * Host-only. */
int  fcgpu_patterns_match(const uint8_t *bytes, const uint32_t *lens, uint32_t n, uint32_t nports, const uint8_t *text,
                          uint32_t len, uint32_t *end);
/* The automaton's shape: states, byte classes ("other" included), the device
 * image in bytes and the longest pattern. The class map and transitions go to
 * LDS when image_bytes minus the output table (2 B per final state) is at
 * most 36 KiB, else the transitions are read from global memory.
 * FCGPU_EINVAL for a refused list. Host-only. */
int  fcgpu_patterns_stats(const uint8_t *bytes, const uint32_t *lens, uint32_t n, uint32_t *states, uint32_t *classes,
                          uint32_t *image_bytes, uint32_t *lmax);

/* Flow table: the IPFlow5ID flow classification of
 * FlowIPManagerHMP (elements/research/flowipmanagerhmp.cc:96-126; the
 * VirtualFlowManager family, include/click/flow/virtualflowmanager.hh) placed
 * after the IPv4 check (and the L4 check, if configured) and before the
 * classifier: every packet that passed the checks gets the ID of its
 * (saddr, daddr, sport, dport, proto) flow; a flow seen for the first time gets
 * the next ID (0, 1, 2, ... in packet order, persistent across batches: the
 * `_current.fetch_and_add(1)` of flowipmanagerhmp.cc:99-102 on one thread).
 * Non-first fragments key on ip_p alone: IPFlowID(p) returns before
 * assign() for them (lib/ipflowid.cc:34-38), so their addresses stay 0 and
 * their ports unset (defined as 0 here). IPv4 check modes only.
 *   max_flows: IDs 0 .. max_flows-1 (the table holds 2x that many slots, up to
 *     2^23 flows); a packet of a new flow beyond that gets FCGPU_FLOW_FULL (the
 *     manager kills it, virtualflowmanager.hh:262-266). 0 disables the table.
 * Batches are assigned IDs in the order the context receives them; a
 * fcgpu_process on a caller's stream is ordered after (and before) the
 * context's own span submissions, so mixing the two entry points is safe.
 * Each fcgpu_process with flow enabled adds a pass over the batch's new flows
 * after the receive kernel (one launch, three after a batch with many new
 * flows); fcgpu_process_host processes the batch in order on one stream.
 * The context's max_batch must be at most FCGPU_FLOW_MAX_BATCH. */
#define FCGPU_FLOW_NONE 0xffffffffu
#define FCGPU_FLOW_FULL 0xfffffffeu
#define FCGPU_MAX_FLOWS (1u << 23)
#define FCGPU_FLOW_MAX_BATCH (64u * ((1u << 14) + 64))
int  fcgpu_flow_enable(fcgpu_ctx *ctx, uint32_t max_flows);
/* Forget every flow (IDs restart at 0). */
int  fcgpu_flow_reset(fcgpu_ctx *ctx);
/* HMP: flow IDs assigned so far; IMP: flows in the table (the managers'
 * "count" handler, virtualflowmanager.hh:387-388). Synchronises the context's
 * device work. */
int  fcgpu_flow_count(fcgpu_ctx *ctx, uint32_t *count);

/* Flow managers (the VirtualFlowManager family). One table per
 * context, as the reference keeps one per thread (per_thread_oread<State>,
 * virtualflowmanager.hh:410); fcgpu_flow_enable(ctx, n) is the HMP manager.
 *   FCGPU_FLOW_MGR_HMP: FlowIPManagerHMP, IDs 0, 1, 2, ... (above); no timeout.
 *   FCGPU_FLOW_MGR_IMP: VirtualFlowManagerIMP over FlowManagerIMPState, the
 *     manager of FlowIPManager_CuckooPP / FlowIPManagerIMP
 *     (elements/flow/flowipmanager_cuckoopp.cc:57-121):
 *     - capacity is rounded up to a power of two (virtualflowmanager.hh:85);
 *       IDs come from a free-ID stack filled with 0 .. cap-1 (:113-115), popped
 *       from the top: cap-1, cap-2, ... A popped 0 means "full" (:264-268): a
 *       new flow when only 0 is left gets FCGPU_FLOW_FULL (the element kills
 *       it). (The reference then reads below its stack on the next pop; here
 *       the table stays full until IDs come back.)
 *     - timeout_s > 0 (TIMEOUT) with recycle_ms (RECYCLE_INTERVAL, 1 ..
 *       65535 ms): every flow with a packet in a batch is stamped with the
 *       batch's time (fcgpu_flow_set_time before the batch; :236-239,311-313);
 *       a new flow is scheduled on a timer wheel timeout_s * eps epochs ahead
 *       (eps = max(1, 1000 / recycle_ms); :72-74,293-296). Each
 *       fcgpu_flow_maintain is one maintainer run (:151-223): the IDs the
 *       previous run released go back onto the stack, then the wheel's current
 *       bucket is walked: a flow idle for old ms with old + recycle_ms >=
 *       timeout_s * 1000 is removed from the table and its ID released; others
 *       are rescheduled. The caller runs it every recycle_ms (the reference's
 *       maintain timer, :118-124,134-144), on the same clock.
 *       Memory: next_pow2(TE + 2) * cap * 4 B of wheel (TE = timeout epochs,
 *       at most 16382) and (cap / 1024) * (TE + 1) * 4 B of maintainer counts
 *       (at most 2^26 words); a second slot array the run rebuilds into.
 *   Times are ms on any clock that the caller uses consistently (32-bit,
 *   differences below 2^31 ms). */
#define FCGPU_FLOW_MGR_HMP 0u
#define FCGPU_FLOW_MGR_IMP 1u
typedef struct fcgpu_flow_config {
    uint32_t manager;       /* FCGPU_FLOW_MGR_* */
    uint32_t capacity;      /* HMP: max flows; IMP: CAPACITY (0 disables the table) */
    uint32_t timeout_s;     /* IMP: TIMEOUT in seconds, 0 = flows never expire */
    uint32_t recycle_ms;    /* IMP with timeout: RECYCLE_INTERVAL in ms (reference default 1000) */
} fcgpu_flow_config;
int  fcgpu_flow_configure(fcgpu_ctx *ctx, const fcgpu_flow_config *cfg);
/* The time stamp of the batches submitted after this call
 * (Timestamp::recent_steady() of push_batch, :227-230). */
int  fcgpu_flow_set_time(fcgpu_ctx *ctx, uint32_t now_ms);
/* One maintainer run at time now_ms, queued after the batches submitted
 * before it (on the context's own stream when it has one -- span submissions
 * -- else on `stream`, NULL = the null stream). No-op without timeouts. */
int  fcgpu_flow_maintain(fcgpu_ctx *ctx, uint32_t now_ms, void *stream);
typedef struct fcgpu_flow_stat {
    uint32_t manager, capacity;
    uint32_t count;         /* flows in the table ("count" handler) */
    uint32_t free_ids;      /* IDs the stack can still give ("count_fids", :390-391) */
    uint32_t pending;       /* IDs released by the last run, back on the stack at the next */
    uint32_t epochs;        /* maintainer runs so far (the wheel index) */
} fcgpu_flow_stat;
/* Synchronises the context's device work. */
int  fcgpu_flow_stats(fcgpu_ctx *ctx, fcgpu_flow_stat *st);

/* AggregateCounter (elements/analysis/aggcounter.{hh,cc}) behind the
 * classifier: one 64-bit packet or byte count per distinct value of the
 * AGGREGATE annotation, kept on the device across the context's batches until
 * fcgpu_aggcount_reset. Per packet it is AggregateCounterBase<T>::update
 * (aggcounter.cc:282-322), the path push_batch takes:
 *   - the counter sits where the classifier's outputs rejoin: it sees a packet
 *     iff its verdict reason is FCGPU_R_OK;
 *   - agg = hash & mask, hash = the value fcgpu_out.hash carries; 0 and
 *     0xffffffff are ordinary aggregates. cfg.hash_mode FCGPU_HASH_NONE with
 *     the counter enabled is FCGPU_EINVAL at submission;
 *   - amount: bytes 0: 1; bytes 1: anno.length (after the checker's trim);
 *     bytes 1 and ip_bytes: anno.length - anno.nh. The EXTRA_PACKETS and
 *     EXTRA_LENGTH annotations do not exist here and count as 0;
 *   - frozen (the "freeze" handler, set between batches): only aggregates that
 *     already have a node are updated, a packet of an unseen one is not
 *     counted;
 *   - capacity: at most `capacity` distinct aggregates get a node. An
 *     aggregate that arrives when the table is full is refused, and from then
 *     on every packet of it is, never a part of them; with at most `capacity`
 *     distinct aggregates nothing is refused. The limit is this library's: the
 *     reference grows until memory runs out;
 *   - the reference's 32-bit Node::count is the low word of a count; nnz is
 *     _num_nonzero.
 * Out of scope: the keywords AGGREGATE_FREEZE, AGGREGATE_STOP, AGGREGATE_CALL
 * and COUNT_* (they depend on the packet order inside a batch), the second,
 * always-frozen input, write_ip_file, counts_pdf and banners.
 * The counter is a post-pass kernel behind k_rx on the batch's stream
 * (DESIGN.md 3.9); where the caller leaves fcgpu_out.verdict, hash or anno
 * NULL, k_rx writes context scratch instead (max_batch entries, allocated with
 * the table as one group: an allocation failure leaves the previous state).
 * Served by fcgpu_process and fcgpu_process_jobs, with every check and
 * classify mode; an enabled context's jobs share one stream and are not fused,
 * and its fcgpu_process calls must all be on one stream too (the scratch is one
 * set per context and nothing orders two streams that use it);
 * fcgpu_process_host, fcgpu_process_counted, fcgpu_process_mbufs,
 * fcgpu_span_submit and fcgpu_span_submit_block return FCGPU_EINVAL.
 * configure and reset are refused while a span submission is queued and
 * synchronise the device. */
#define FCGPU_AGGCOUNT_MAX_CAPACITY (1u << 24)
typedef struct fcgpu_aggcount_config {
    uint32_t capacity;      /* distinct aggregates; 0 disables and frees. At most
                               FCGPU_AGGCOUNT_MAX_CAPACITY */
    uint32_t bytes, ip_bytes;
    uint32_t mask;          /* 0 is taken as 0xffffffff */
} fcgpu_aggcount_config;
/* Replaces the counter (its counts are forgotten, it is not frozen). */
int  fcgpu_aggcount_configure(fcgpu_ctx *ctx, const fcgpu_aggcount_config *cfg);
int  fcgpu_aggcount_freeze(fcgpu_ctx *ctx, int frozen);
/* "clear": forget every aggregate and the totals; frozen stays. */
int  fcgpu_aggcount_reset(fcgpu_ctx *ctx);
typedef struct fcgpu_aggcount_stat {
    uint32_t capacity, nagg, nnz, frozen;   /* nagg: aggregates with a node */
    uint64_t count;         /* sum of the amounts counted */
    uint64_t seen;          /* packets with FCGPU_R_OK */
    uint64_t uncounted;     /* packets refused or unseen-while-frozen */
} fcgpu_aggcount_stat;
/* stats and read synchronise the context's device work. */
int  fcgpu_aggcount_stats(fcgpu_ctx *ctx, fcgpu_aggcount_stat *st);
/* write_file order: records sorted by aggregate ascending, zero counts left
 * out. Up to max records are written (h_out may be NULL with max 0); *n gets
 * the number available. */
typedef struct fcgpu_aggcount_rec {
    uint32_t agg, reserved;
    uint64_t count;
} fcgpu_aggcount_rec;
int  fcgpu_aggcount_read(fcgpu_ctx *ctx, fcgpu_aggcount_rec *h_out, uint32_t max, uint32_t *n);

/* ESP authentication, IPsecAuthHMACSHA1 (elements/ipsec/hmacsha1.cc:61-96)
 * behind the classifier: HMAC-SHA1 with the SA's 16-byte key (hmac.cc:147-159,
 * plain HMAC), truncated to 96 bits, in both of the element's modes. It is
 * the authentication stage of the inbound chain of conf/router/
 * ipsec-router.click, rt[0] -> StripIPHeader -> IPsecAES(0) ->
 * IPsecAuthHMACSHA1(1) -> IPsecESPUnencap; the stage authenticates whatever
 * bytes the frame holds, exactly as the element does (the reference chain
 * decrypts first). Per packet:
 *   - it is considered iff its verdict reason is FCGPU_R_OK, anno.ipver == 4
 *     and the IP protocol byte (frame byte nh + 9) is 50, the ESP case of
 *     IPsecRouteTable::push (ipsecroutetable.cc:217-237); any other packet is
 *     left alone, status FCGPU_ESP_NOT_ESP;
 *   - e0 = nh + 4 * ihl (the bytes StripIPHeader removes), end = anno.length
 *     (after CheckIPHeader's trim), elen = end - e0;
 *   - elen < 16 + 12, the esp_new header (esp.hh:26-30) plus the digest:
 *     FCGPU_ESP_SHORT. (The reference would hand HMAC length() - 12 < 0; this
 *     library defines the case as a status);
 *   - the SA is found by the SPI, the big-endian word at e0 (IPsecESPEncap
 *     wrote it from the SA the annotation names); none: FCGPU_ESP_NO_SA, the
 *     reference's "Invalid SPI, Dropping packet";
 *   - FCGPU_ESP_VERIFY: the digest is HMAC-SHA1(auth_key, frame[e0, end - 12));
 *     its first 12 bytes are compared with frame[end - 12, end): FCGPU_ESP_OK
 *     or FCGPU_ESP_BAD; the record's icv holds the computed 12 bytes;
 *   - FCGPU_ESP_COMPUTE: icv = the first 12 bytes of HMAC-SHA1(auth_key,
 *     frame[e0, end)), the bytes put(12) would append; FCGPU_ESP_OK.
 *   - FCGPU_ESP_SEAL: the outbound IPsecAuthHMACSHA1(0) for a frame that
 *     already holds room for the digest. Selection and statuses are VERIFY's
 *     (elen < 28: FCGPU_ESP_SHORT); the digest is HMAC-SHA1(auth_key,
 *     frame[e0, end - 12)); its first 12 bytes are WRITTEN to frame[end - 12,
 *     end) and the record holds FCGPU_ESP_OK and the same 12 bytes. Those 12
 *     bytes of OK packets are written and no other byte, by naturally aligned
 *     byte, short or dword stores chosen by the address's low bits (no
 *     read-modify-write of a shared word); nothing past `end` is read beyond
 *     the 16-byte slack. While SEAL is configured fcgpu_process writes
 *     d_arena.
 * VERIFY and COMPUTE never write frames; verdict, hash, the partition and the
 * counters are untouched. Out of scope: IPsecESPUnencap, anti-replay and the element
 * keyword. With the decryption stage below installed as well, k_espaes runs
 * in front of this stage on the same stream, so the digest is taken over the
 * decrypted bytes, as in the reference's chain; with that stage in its
 * encryption mode this stage runs first (authenticate, then encrypt).
 * The stage is a post-pass kernel behind k_rx on the batch's stream (DESIGN.md
 * 3.10). Its records are one context-owned array of max_batch entries holding
 * the last fcgpu_process batch; where the caller leaves fcgpu_out.verdict or
 * anno NULL, k_rx writes context scratch instead (allocated with the table and
 * the records as one group: a failed fcgpu_espauth_set_sas leaves the
 * installed table in place). Served by fcgpu_process, on one stream per
 * context; while SAs are installed fcgpu_process_jobs, fcgpu_process_host,
 * fcgpu_process_counted, fcgpu_process_mbufs, fcgpu_span_submit and
 * fcgpu_span_submit_block return FCGPU_EINVAL. */
#define FCGPU_ESP_VERIFY  0u
#define FCGPU_ESP_COMPUTE 1u
#define FCGPU_ESP_SEAL    2u
#define FCGPU_ESP_NOT_ESP 0
#define FCGPU_ESP_OK      1
#define FCGPU_ESP_BAD     2
#define FCGPU_ESP_NO_SA   3
#define FCGPU_ESP_SHORT   4
#define FCGPU_ESPAUTH_MAX_SAS 65536u
typedef struct fcgpu_esp_sa {
    uint32_t spi;           /* host order; never 0 */
    uint8_t auth_key[16];
} fcgpu_esp_sa;
typedef struct fcgpu_espauth_config {
    uint32_t mode;          /* FCGPU_ESP_VERIFY | FCGPU_ESP_COMPUTE | FCGPU_ESP_SEAL */
} fcgpu_espauth_config;
typedef struct fcgpu_esp_rec {
    uint8_t status;         /* FCGPU_ESP_* */
    uint8_t pad[3];
    uint8_t icv[12];        /* FCGPU_ESP_OK / _BAD: the computed digest; else 0 */
} fcgpu_esp_rec;
typedef struct fcgpu_espauth_stat {
    uint64_t ok, bad, no_sa, too_short, not_esp;
} fcgpu_espauth_stat;
/* Replaces the SA table (the statistics restart, the mode stays); n == 0
 * disables the stage and frees it. FCGPU_EINVAL: SPI 0, a duplicate SPI, more
 * than FCGPU_ESPAUTH_MAX_SAS. Synchronises the device. */
int  fcgpu_espauth_set_sas(fcgpu_ctx *ctx, const fcgpu_esp_sa *sas, uint32_t n);
/* The mode of the batches submitted after this call (default VERIFY).
 * FCGPU_EINVAL: a mode above FCGPU_ESP_SEAL. */
int  fcgpu_espauth_configure(fcgpu_ctx *ctx, const fcgpu_espauth_config *cfg);
/* Device pointer to the records, [max_batch]: entry i is packet i of the last
 * fcgpu_process batch, ordered behind it on its stream. NULL while disabled. */
int  fcgpu_espauth_records(fcgpu_ctx *ctx, const fcgpu_esp_rec **d_rec);
/* Packets per status since set_sas / reset. Synchronises the device. */
int  fcgpu_espauth_stats(fcgpu_ctx *ctx, fcgpu_espauth_stat *st);
int  fcgpu_espauth_reset(fcgpu_ctx *ctx);

/* ESP decryption, IPsecAES(0) (elements/ipsec/aes.cc:69-138, decrypt branch)
 * behind the classifier and in front of the authentication stage above:
 * AES-128 (FIPS 197) with the SA's 16-byte key in the element's 8-byte-IV
 * chaining, in place in the arena. Per packet:
 *   - it is considered by the rule of the authentication stage: verdict
 *     reason FCGPU_R_OK, anno.ipver == 4 and frame byte nh + 9 == 50; any
 *     other packet: FCGPU_ESP_NOT_ESP, no byte touched;
 *   - e0 = nh + 4 * ihl, end = anno.length, elen = end - e0; elen < 28:
 *     FCGPU_ESP_SHORT; the SA is found by the big-endian SPI at e0, none:
 *     FCGPU_ESP_NO_SA;
 *   - plen = elen - 16 - 12 (esp_new and the element's _ignore = 12);
 *     plen % 8 != 0: FCGPU_ESP_UNALIGNED, no byte touched (the reference's
 *     loop would run past the packet's end; this library defines the case);
 *   - plen % 16 == 8: plen += 8 -- the reference encrypts the first 8 digest
 *     bytes rather than pad, so the region still ends inside the frame;
 *   - nblk = plen / 16 (may be 0); block i is C_i = frame[e0 + 16 + 16 i,
 *     + 16); it becomes P_i = AES128-decrypt(enc_key, C_i) with its FIRST 8
 *     BYTES ONLY XORed with IV = frame[e0 + 8, e0 + 16) for i = 0 and with
 *     the first 8 bytes of the ciphertext C_{i-1} otherwise; bytes 8..15 are
 *     the raw block decryption. This is the element's chaining, not RFC 3602
 *     CBC. The IV field is unchanged (the reference restores it);
 *     FCGPU_ESP_OK.
 * The stage writes exactly the 16 * nblk bytes of every OK packet: no header,
 * IV or untouched digest byte, no byte of another packet, no slack byte
 * between frames. WHILE A TABLE IS INSTALLED fcgpu_process WRITES d_arena
 * (the element decrypts in place after uniqueify()); the parameter stays
 * const in the signature. Loads may over-read within the 16-byte slack.
 * One status byte per packet in a context-owned device array of max_batch
 * entries holding the last fcgpu_process batch. The table, the status array,
 * the statistics and the scratch k_rx writes where fcgpu_out.verdict or anno
 * is NULL are one allocation group: a failed fcgpu_espaes_set_sas leaves the
 * installed table in place. Launch order on the batch's stream: k_rx, the
 * aggregate counter, k_espaes, k_espauth, the flow pass.
 * Served by fcgpu_process; while SAs are installed fcgpu_process_jobs,
 * fcgpu_process_host, fcgpu_process_counted, fcgpu_process_mbufs,
 * fcgpu_span_submit and fcgpu_span_submit_block return FCGPU_EINVAL.
 *
 * FCGPU_ESPAES_ENCRYPT (fcgpu_espaes_configure) is IPsecAES(1), the encrypt
 * branch of the same element (aes.cc:115-133), the last transform of the
 * outbound chain rt[1] -> IPsecESPEncap -> IPsecAuthHMACSHA1(0) -> IPsecAES(1)
 * -> IPsecEncap(50). Packet selection, e0, end, elen, plen, the statuses, the
 * region rule (plen % 16 == 8 extends the region over the first 8 digest
 * bytes) and nblk are exactly the rules above. Block i is P_i = frame[e0 + 16
 * + 16 i, + 16); it becomes C_i = AES128-encrypt(enc_key, P_i') where P_i' is
 * P_i with its FIRST 8 BYTES ONLY XORed with IV = frame[e0 + 8, e0 + 16) for
 * i = 0 and with C_{i-1}[0, 8) otherwise. In place: exactly the 16 * nblk
 * bytes of every OK packet are written and nothing else; the IV is read and
 * never written; fcgpu_espaes_stat.blocks counts blocks encrypted. The status
 * array, the statistics, the NULL-output scratch and the refusals of the
 * other entry points are those of decryption. A packet is a serial chain of
 * nblk dependent block encryptions (k_espenc).
 * Launch order with the encryption mode: k_rx, the aggregate counter,
 * k_espauth, k_espenc, the flow pass -- the reference's
 * authenticate-then-encrypt order, so one fcgpu_process call with
 * FCGPU_ESP_SEAL and FCGPU_ESPAES_ENCRYPT turns an IPsecESPEncap-shaped frame
 * (SPI, sequence number, IV, padded payload, 12 bytes of room) into the wire
 * packet's ESP part. Either stage alone keeps working.
 * Out of scope: IPsecESPEncap itself (frame growth, random IVs, the replay
 * counter), IPsecEncap(50), IPsecESPUnencap, anti-replay, the element
 * keyword. */
#define FCGPU_ESP_UNALIGNED 5
#define FCGPU_ESPAES_MAX_SAS 65536u
#define FCGPU_ESPAES_DECRYPT 0u
#define FCGPU_ESPAES_ENCRYPT 1u
typedef struct fcgpu_espaes_sa {
    uint32_t spi;           /* host order; never 0 */
    uint8_t enc_key[16];
} fcgpu_espaes_sa;
typedef struct fcgpu_espaes_config {
    uint32_t mode;          /* FCGPU_ESPAES_DECRYPT | FCGPU_ESPAES_ENCRYPT */
} fcgpu_espaes_config;
typedef struct fcgpu_espaes_stat {
    uint64_t ok, no_sa, too_short, unaligned, not_esp, blocks;   /* blocks: 16-byte blocks decrypted / encrypted */
} fcgpu_espaes_stat;
/* Replaces the SA table (the statistics restart, the mode stays); n == 0
 * disables the stage and frees it. FCGPU_EINVAL: SPI 0, a duplicate SPI, more than
 * FCGPU_ESPAES_MAX_SAS. Synchronises the device. */
int  fcgpu_espaes_set_sas(fcgpu_ctx *ctx, const fcgpu_espaes_sa *sas, uint32_t n);
/* The mode of the batches submitted after this call (default DECRYPT); it may
 * be called with no table installed. FCGPU_EINVAL: any other mode. */
int  fcgpu_espaes_configure(fcgpu_ctx *ctx, const fcgpu_espaes_config *cfg);
/* Device pointer to the status bytes (FCGPU_ESP_*), [max_batch]: entry i is
 * packet i of the last fcgpu_process batch. NULL while disabled. */
int  fcgpu_espaes_status(fcgpu_ctx *ctx, const uint8_t **d_status);
/* Packets per status and blocks since set_sas / reset. Synchronises the device. */
int  fcgpu_espaes_stats(fcgpu_ctx *ctx, fcgpu_espaes_stat *st);
int  fcgpu_espaes_reset(fcgpu_ctx *ctx);

/* Host threads the context may use for the gather / copy-out loops of
 * fcgpu_process_host (the caller's thread included; default 1). */
int  fcgpu_set_host_threads(fcgpu_ctx *ctx, uint32_t nthreads);
/* Pinned host memory for fcgpu_process_host outputs (NULL on failure). */
void *fcgpu_host_alloc(size_t bytes);
void fcgpu_host_free(void *p);
/* Page-lock existing host memory for DMA (hipHostRegister; read-only mappings
 * such as an mmapped pcap are registered read-only). */
int  fcgpu_host_register(void *p, size_t bytes, int read_only);
int  fcgpu_host_unregister(void *p);

/* mbuf ingress: the batch FromDPDKDevice::_run_task gets
 * from rte_eth_rx_burst (elements/userlevel/fromdpdkdevice.cc:374-456) goes to
 * the GPU as the array of mbuf pointers itself -- no Packet objects, no host
 * copy of the frames. The packet-buffer pool (a DPDK mempool's memory: mbuf
 * headers and data rooms, < 4 GiB) is registered once per context (contexts
 * of other threads registering the same pool share one pinning, released
 * with the last of them); each call copies the
 * n pointers H2D, a kernel reads every mbuf's buf_addr / data_off / data_len
 * straight from host memory and builds the batch's descriptors, and k_rx
 * reads the frames' header windows from the pool over PCIe (zero copy).
 * Outputs go to device memory (d_out), as fcgpu_process. A pointer (or a
 * frame) outside the registered pool is never dereferenced: that packet is
 * processed as an empty frame (FCGPU_R_MINISCULE / not checked). Field
 * offsets are the caller's mbuf layout; FCGPU_MBUF_LAYOUT_DPDK is rte_mbuf's
 * (DPDK >= 20.11: buf_addr @0, data_off @16, data_len @40). Asynchronous on
 * `stream`; mbufs[] may be reused when the call returns. */
typedef struct fcgpu_mbuf_layout {
    uint32_t buf_addr;        /* offset of the void *buf_addr field          */
    uint32_t data_off;        /* offset of the uint16_t data_off field       */
    uint32_t data_len;        /* offset of the uint16_t data_len field       */
    uint32_t header_bytes;    /* bytes of the mbuf header read (>= every field end, <= 64) */
} fcgpu_mbuf_layout;
#define FCGPU_MBUF_LAYOUT_DPDK {0u, 16u, 40u, 64u}
int  fcgpu_pool_register(fcgpu_ctx *ctx, void *base, size_t bytes);
int  fcgpu_process_mbufs(fcgpu_ctx *ctx, void *const *mbufs, uint32_t n, const fcgpu_mbuf_layout *layout,
                         const fcgpu_out *d_out, void *stream);

int  fcgpu_read_counters(fcgpu_ctx *ctx, uint64_t *out, int n);
/* The device keeps the per-reason and per-output bins only; "count" and
 * "drops" are derived: drops = the reason slots of reasons 0-5, 7, 8 (the
 * checker's drops), count = all packets (sum of the output bins, invalid list
 * included) - drops. fcgpu_read_counters applies this; callers summing the
 * raw device replicas themselves (e.g. after an all-reduce) call this on the
 * summed FCGPU_NCOUNTERS vector. */
void fcgpu_counters_derive(uint64_t *vec);
int  fcgpu_reset_counters(fcgpu_ctx *ctx);
/* Device address of the context's uint64 counter replicas
 * (FCGPU_CTR_SHARDS x FCGPU_NCOUNTERS), for a cross-GPU all-reduce. */
int  fcgpu_counters_device(fcgpu_ctx *ctx, uint64_t **d_counters);
/* Make the context accumulate into caller-owned device memory
 * (FCGPU_CTR_SHARDS x FCGPU_NCOUNTERS uint64, initialised by the caller), e.g. a
 * tensor that is all-reduced over RCCL. NULL reverts to the context's own. */
int  fcgpu_use_counters(fcgpu_ctx *ctx, uint64_t *d_counters);

/* Per-kernel timing with HIP events on the launch stream (off by default).
 * fcgpu_set_timing(ctx, k): k > 0 brackets the k-th, 2k-th, ... launch of the
 * context after this call (1 = every launch) with start/stop events: the
 * event pair of hipExtLaunchKernelGGL for a one-batch launch, two stream
 * markers (hipEventRecord) around a fused launch of several batches (cheaper
 * on an idle queue; the interval adds the launch's dispatch latency). A fused
 * launch counts as its number of batches. The events are created by this
 * call, not on the launch path. 0 = off. (Each recorded event idles the queue for a few us,
 * so sparse sampling keeps the measured region representative.)
 * fcgpu_read_timing returns, per stage (0 = fused check/hash/classify,
 * 1 = count scan, 2 = partition scatter), the summed milliseconds and launches
 * since the last read, and resets them. Synchronises the context stream. */
int  fcgpu_set_timing(fcgpu_ctx *ctx, int every);
int  fcgpu_read_timing(fcgpu_ctx *ctx, double *ms, uint32_t *launches, int nstages);

/* Flow re-shard across GPUs (SURVEY 8(f) #1 over 8(e)). FastClick keeps one
 * flow table per core and relies on the NIC's RSS hash to send every packet
 * of a flow to one core (VirtualFlowManagerIMP::process,
 * include/click/flow/virtualflowmanager.hh:249-330; FlowIPManagerHMP,
 * elements/flow/flowipmanagerhmp.cc:101-117). When packets reach the GPUs
 * unsharded, each rank's device pass (fcgpu_process with FCGPU_CLS_LB_HASH
 * over nports = world outputs and FCGPU_PART_GLOBAL: perm + port_start) names
 * every packet's owner rank, and these calls build and read the buffers of
 * one all-to-all (RCCL over xGMI) that moves each packet to its owner:
 *
 *   fcgpu_exchange_plan   perm[0 .. port_start[world]) -- the packets that
 *       leave (output `world`, the invalid list, stays) -- gets one
 *       fcgpu_xmeta record each, in perm order; d_seg_bytes[d] = the bytes of
 *       owner d's segment of the send buffer. Each frame takes a 16-B aligned
 *       slot of (length + 15) & ~15 bytes (ABI 22; 4-B slots before), so every
 *       slot is written in whole aligned 16-B stores. Segments follow in owner
 *       order.
 *   fcgpu_exchange_pack   the frames into d_send (at least the sum of
 *       d_seg_bytes; nothing is written past send_cap; an owner whose
 *       d_seg_bytes exceeds 0xffffffff -- its records' 32-bit offsets cannot
 *       address it -- is not packed, so check the plan's sizes first): owner d's segment
 *       holds its packets in input order; slot bytes past a frame's length
 *       are zero. It reads the frames' arena offsets the plan left in the
 *       context: call it after fcgpu_exchange_plan of the same batch on the
 *       same context and stream, before the next plan.
 *   (the caller's all-to-all: records and segments; a receiver concatenates
 *    the segments it gets in source-rank order)
 *   fcgpu_exchange_unpack the received records -> descriptors into the
 *       received buffer: desc[2j] = src_displ[record.src_rank] + record.off,
 *       desc[2j+1] = record.length, where src_displ[r] is where source r's
 *       segment starts in that buffer (host array of `world` values). The
 *       offsets must fit in 32 bits; the receiver keeps the ABI's over-read
 *       slack (128 B past every frame start, 16 B past every frame end)
 *       readable after its buffer.
 * The frames keep their bytes and lengths exactly; the records carry each
 * packet's source (rank, index), so the receiver's order is (source rank,
 * source index). world <= FCGPU_MAX_PORTS; n <= the context's max_batch for
 * the plan. Asynchronous on `stream` (plan needs the context's scratch: one
 * plan at a time per context). */
typedef struct fcgpu_xmeta {
    uint32_t off;             /* the frame's slot within its owner's segment             */
    uint32_t length;          /* frame length                                            */
    uint32_t src_index;       /* index in the source rank's batch                        */
    uint32_t src_rank;        /* source rank (bytes 8..15 = src_rank << 32 | src_index)  */
} fcgpu_xmeta;
int  fcgpu_exchange_plan(fcgpu_ctx *ctx, const uint32_t *d_desc, const uint32_t *d_perm,
                         const uint32_t *d_port_start, uint32_t n, uint32_t world, uint32_t rank,
                         fcgpu_xmeta *d_meta, uint64_t *d_seg_bytes, void *stream);
int  fcgpu_exchange_pack(fcgpu_ctx *ctx, const uint8_t *d_arena, const uint32_t *d_port_start,
                         const fcgpu_xmeta *d_meta, const uint64_t *d_seg_bytes, uint32_t n, uint32_t world,
                         uint8_t *d_send, uint64_t send_cap, void *stream);
int  fcgpu_exchange_unpack(fcgpu_ctx *ctx, const fcgpu_xmeta *d_meta, uint32_t n, const uint64_t *src_displ,
                           uint32_t world, uint32_t *d_desc, void *stream);

/* The send side in one call, from the owner pass's verdicts instead of its
 * whole-batch partition: packet i leaves to owner d = d_verdict[i] >> 8 when
 * d < world (a k_rx pass with LB_MODE hash over `world` outputs; the invalid
 * list, port `world`, stays). Writes exactly what fcgpu_exchange_plan +
 * fcgpu_exchange_pack write for the stable partition of those owners (records
 * in owner order, input order within an owner; owner d's segment; slot
 * padding zero), plus d_seg_n[d], the packets of owner d. send_cap bounds the
 * send buffer as for fcgpu_exchange_pack (the sum of the leaving frames'
 * slots fits in send_cap whenever it is at least the arena's frame bytes +
 * 15 per packet), so no host sync is needed before the call. Every per-packet
 * load is in input order (three launches: per-tile owner counts and bytes,
 * their scan per owner, the records and frames per tile). The per-tile
 * counts are one scratch per context: builds on one context must be
 * serialised on one stream (as plan -> pack are). */
int  fcgpu_exchange_build(fcgpu_ctx *ctx, const uint8_t *d_arena, const uint32_t *d_desc,
                          const uint16_t *d_verdict, uint32_t n, uint32_t world, uint32_t rank,
                          fcgpu_xmeta *d_meta, uint32_t *d_seg_n, uint64_t *d_seg_bytes, uint8_t *d_send,
                          uint64_t send_cap, void *stream);

/* The fixed-capacity exchange: no host sync anywhere in a re-shard step.
 * Owner d's segment has room for seg_recs packets and seg_bytes frame bytes
 * (16-B slots): d_meta holds world x (seg_recs + 1) records -- segment d at
 * d (seg_recs + 1): a header (fcgpu_xseg) then its records, as
 * fcgpu_exchange_build writes them -- and d_send world x seg_bytes bytes,
 * segment d at d x seg_bytes (record offsets relative to it). Both go through
 * all-to-alls with equal splits (the split sizes never leave the device). An
 * owner whose packets do not fit gets its header alone, flags bit 0 set:
 * the receivers then process nothing for that step and the caller falls
 * back to the counted exchange (fcgpu_exchange_build) for it
 * (fastclick_amd.dist). world x seg_bytes must stay below 4 GiB. */
typedef struct fcgpu_xseg {
    uint32_t packets;         /* the owner's packets this step                          */
    uint32_t bytes_lo;        /* their slot bytes                                         */
    uint32_t bytes_hi;
    uint32_t flags;           /* bit 0: overflow -- more than the capacity, none sent     */
} fcgpu_xseg;
int  fcgpu_exchange_build_fixed(fcgpu_ctx *ctx, const uint8_t *d_arena, const uint32_t *d_desc,
                                const uint16_t *d_verdict, uint32_t n, uint32_t world, uint32_t rank,
                                uint32_t seg_recs, uint64_t seg_bytes, fcgpu_xmeta *d_meta, uint8_t *d_send,
                                void *stream);
/* The receive side after the equal-split all-to-alls: d_rmeta / the received
 * frames in the layout above, source s's segment at s. Writes the received
 * packets' descriptors (in source-rank order, then source order, as
 * fcgpu_exchange_unpack) into d_desc (room for world x seg_recs) and their
 * number into *d_count. If any segment overflowed, or *d_stall is already
 * non-zero (an earlier step stalled and is not repaired yet), *d_count = 0
 * and *d_stall = step when it was 0: the flow pass of this step and of every
 * later one processes nothing until the caller has replayed them, in order,
 * through the counted exchange and cleared *d_stall. step must be non-zero.
 * d_total (may be NULL): *d_total += the count, a running total of the
 * packets received that needs no host read per step. */
int  fcgpu_exchange_unpack_fixed(fcgpu_ctx *ctx, const fcgpu_xmeta *d_rmeta, uint32_t world, uint32_t seg_recs,
                                 uint64_t seg_bytes, uint32_t *d_desc, uint32_t *d_count, uint32_t *d_stall,
                                 uint64_t *d_total, uint32_t step, void *stream);

const char *fcgpu_last_error(fcgpu_ctx *ctx);   /* ctx may be NULL (open errors) */

#ifdef __cplusplus
}
#endif
#endif /* FASTCLICK_GPU_H */
