/*
 * fcclick.h -- C ABI of the Click-shaped host harness (libfcclick.so).
 *
 * Drives the GPUIPCheckClassify BatchElement (fastclick_amd/csrc/host/
 * gpu_element.hh) the way FastClick drives an element behind FromDPDKDevice:
 * a source pushes PacketBatches of BURST packets (FromDPDKDevice BURST 32,
 * elements/userlevel/fromdpdkdevice.cc:124) into Element::push_batch
 * (include/click/element.hh:53-54); every output port feeds a sink that
 * records what left on it, in order. This is how the element is tested and
 * how the end-to-end host-resident rate is measured.
 */
#ifndef FCCLICK_H
#define FCCLICK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Parse/validate an element configuration such as
 *   "GPUIPCheckClassify(OFFSET 14, CHECKSUM true, N 16, LB_MODE hash)"
 * without touching a GPU. Returns 0, or -1 with the message in err. */
int fcclick_check_config(const char *conf, char *err, size_t errcap);

/* The device configuration (fcgpu_cfg) a GPUIPCheckClassify configuration
 * string produces -- its keywords mapped as the element maps them, e.g.
 * INTERFACES to the BADSRC / GOODDST lists -- without touching a GPU.
 * Returns 0, or -1 with the message in err. */
struct fcgpu_cfg;
int fcclick_element_cfg(const char *conf, struct fcgpu_cfg *cfg, char *err, size_t errcap);

/* Parse a decision program in the text form the reference's IPFilter /
 * IPClassifier / Classifier `program` read handler prints
 * (elements/standard/classification.cc:978-991, :1104-1140) into fcgpu_step
 * entries for fcgpu_set_program. Lines may be separated by '\n' or '|'.
 * *nsteps receives the step count (<= cap), *output_everything the "all->[N]"
 * output or -1. Returns 0, or -1 with the message in err. */
struct fcgpu_step;
int fcclick_parse_program(const char *text, struct fcgpu_step *steps, uint32_t cap, uint32_t *nsteps,
                          int32_t *output_everything, char *err, size_t errcap);

/* The element's compact staging (COMPACT true, fastclick_amd/csrc/capture.hh)
 * of n frames for a configuration: each frame's record holds only the bytes
 * the chain reads, in records packed 8 B apart from out_arena + 256; out_desc[i] = (record
 * offset - the chain's first byte, length), so frame byte b of packet i is at
 * out_arena + out_desc[2i] + b for every byte the chain reads. For tests (the
 * oracle on the compact layout must agree with the oracle on the frames).
 * Returns 0, -2 when the chain stages whole captures, -1 on error. */
int fcclick_stage_compact(const char *conf, const uint8_t *arena, const uint32_t *desc, uint32_t n,
                          uint8_t *out_arena, size_t out_cap, uint32_t *out_desc, size_t *out_bytes,
                          char *err, size_t errcap);

typedef struct fcclick_result {
    uint32_t *out_port;     /* [n] output the packet left on; 0xffffffff = killed        */
    uint32_t *out_seq;      /* [n] global departure order (0..), 0xffffffff = killed     */
    uint32_t *out_agg;      /* [n] AGGREGATE_ANNO (anno u32 @20) on departure            */
    uint32_t *out_dst;      /* [n] DST_IP_ANNO (anno u32 @0)                              */
    uint32_t *out_len;      /* [n] packet length on departure                            */
    int32_t  *out_nh;       /* [n] network header offset from data() (-1 unset)          */
    uint32_t *out_batches;  /* [1] number of PacketBatches the sinks received             */
    char     *handlers;     /* "name=value\n" for count, drops, drop_details, port_counts,
                               flow_count, flow_count_fids, flow_drops, gpu_errors,
                               gpu_retries, error                                          */
    size_t    handlers_cap;
    uint8_t  *out_paint;    /* [n] PAINT_ANNO (anno u8 @17) on departure (may be NULL)     */
    uint32_t *out_flow;     /* [n] anno u32 @28 (FLOWID_ANNO default) on departure (may be NULL) */
    uint32_t *out_ip8;      /* [n] network header bytes 8..11 (ttl, proto, checksum) on
                               departure, little-endian (may be NULL)                  */
    uint32_t *out_parked;   /* [1] FCCLICK_TIMER_FLUSH: packets the element still held when
                               the source stopped (may be NULL)                          */
    uint32_t *out_batch;    /* [n] index of the PacketBatch the packet arrived in at its
                               sink, in arrival order over all sinks (may be NULL)    */
    uint8_t  *out_dst6;     /* [n][16] DST_IP6_ANNO (anno bytes 0..15) on departure (may be NULL) */
} fcclick_result;

/* burst value for a non-batch upstream: the source calls the element's
 * per-packet push(0, p) (Element::push, lib/element.cc:3141-3147) instead of
 * push_batch. */
#define FCCLICK_PER_PACKET 0xffffffffu

/* Run a graph  Source(frames, BURST) -> conf => [0 .. nsinks-1] Sink  over n
 * frames (arena + (offset, length) descriptors, host memory), then flush.
 * burst 0 means 32; FCCLICK_PER_PACKET pushes the frames one at a time.
 * Returns 0 on success, -1 on configuration/initialisation error (message in
 * err), -2 when the element reported a GPU runtime error. */
int fcclick_run(const char *conf, const uint8_t *arena, const uint32_t *desc, uint32_t n,
                uint32_t burst, uint32_t nsinks, fcclick_result *res, char *err, size_t errcap);

/* fcclick_run with flags: FCCLICK_TIMER_FLUSH ends the run by firing the
 * element's timer (run_timer at the current time, repeated while it asks to
 * be rescheduled) instead of calling flush(): what a graph whose source has
 * gone quiet relies on to release the last partial batch. */
#define FCCLICK_TIMER_FLUSH 1u
int fcclick_run_ex(const char *conf, const uint8_t *arena, const uint32_t *desc, uint32_t n,
                   uint32_t burst, uint32_t nsinks, uint32_t flags, fcclick_result *res, char *err,
                   size_t errcap);

/* fcclick_run on a virtual clock: before burst b is pushed the element's clock
 * (what it reads as Timestamp::recent_steady) is set to burst_ns[b]
 * (ceil(n / burst) entries), so time-driven behaviour -- the flow managers'
 * timeouts and maintainer runs -- is reproducible. Ends with flush(). */
int fcclick_run_clocked(const char *conf, const uint8_t *arena, const uint32_t *desc, uint32_t n,
                        uint32_t burst, uint32_t nsinks, const uint64_t *burst_ns, fcclick_result *res,
                        char *err, size_t errcap);

/* A scripted run on a virtual clock: events in order, each at its own time
 * t_ns (0 keeps the clock where it is) --
 *   FCCLICK_EV_BURST: the next `count` packets (in descriptor order) as one
 *     PacketBatch, as a source whose bursts vary in size (FromIPSummaryDump
 *     with TIMING and BURST, elements/analysis/fromipsumdump.cc:759-795);
 *   FCCLICK_EV_READ: the element's Timer fires at t_ns (a partial batch due,
 *     the flow maintainer's runs due), then every handler is read, as a
 *     DriverManager `read` at that time would (the texts of all reads go to
 *     `reads`, each read as "name=value" lines ended by a "--" line).
 * The bursts must cover the n packets exactly. Ends with flush(); the final
 * handler values are in res->handlers as for fcclick_run. */
#define FCCLICK_EV_BURST 0u
#define FCCLICK_EV_READ  1u
typedef struct fcclick_event {
    uint64_t t_ns;
    uint32_t kind;
    uint32_t count;
} fcclick_event;
int fcclick_run_events(const char *conf, const uint8_t *arena, const uint32_t *desc, uint32_t n,
                       uint32_t nsinks, const fcclick_event *ev, uint32_t nev, fcclick_result *res,
                       char *reads, size_t reads_cap, char *err, size_t errcap);

/* Host-resident rate: repeat the same run `reps` times (packets recycled
 * LIFO into a mempool sized to what the element can hold, sinks discard), return packets per second through the element
 * including gather, PCIe copies, kernels and relinking. */
int fcclick_bench(const char *conf, const uint8_t *arena, const uint32_t *desc, uint32_t n,
                  uint32_t burst, uint32_t reps, double *pps, char *err, size_t errcap);

/* The same with `threads` element instances, one per thread (each with its
 * own GPU context and packet pool, as Click threads with their own rx queue
 * would be), their timed loops started together after every thread's set-up;
 * *pps = all threads' packets over the union of their timed windows. */
int fcclick_bench_threads(const char *conf, const uint8_t *arena, const uint32_t *desc, uint32_t n,
                          uint32_t burst, uint32_t reps, uint32_t threads, double *pps, char *err,
                          size_t errcap);

/* `threads` element instances (one GPU context each, as Click threads),
 * set up first, then each pushing the trace `reps` times in BURST-packet
 * PacketBatches and flushing, all at once. port_pkts[t * nsinks + k]: the
 * packets thread t's output k received; handlers: every thread's handler
 * dump (the fcclick_run format), each followed by a "--" line. What a
 * multi-threaded run of the element must account for exactly (packets in =
 * packets out + killed), e.g. with GPU faults injected mid-run. */
int fcclick_run_threads(const char *conf, const uint8_t *arena, const uint32_t *desc, uint32_t n,
                        uint32_t burst, uint32_t reps, uint32_t threads, uint32_t nsinks, uint64_t *port_pkts,
                        char *handlers, size_t handlers_cap, char *err, size_t errcap);

/* `threads` element instances pushing whole passes over the trace for
 * `seconds` (a source that keeps pushing, as the CPU baseline's threads do:
 * no thread's tail of a fixed packet count stretches the window): *pps = all
 * threads' packets over the union of their windows, each ending at its first
 * pass boundary after the stop plus its final flush. */
int fcclick_bench_timed(const char *conf, const uint8_t *arena, const uint32_t *desc, uint32_t n,
                        uint32_t burst, double seconds, uint32_t threads, double *pps, char *err,
                        size_t errcap);

#ifdef __cplusplus
}
#endif
#endif
