/*
 * xeng.h -- C ABI of the MI355X-native LWA-352 X-engine library (libxeng.so).
 *
 * This is the drop-in boundary for the hot path of realtimeradio/caltech-bifrost-dsp:
 * the functions below are what the reference's Python blocks reach through
 * `from bifrost.libbifrost import _bf` (ctypes).  Every entry point cites the
 * reference call site it replaces (paths relative to
 * /root/reference/pipeline/lwa352_pipeline/blocks unless stated).
 *
 * Conventions (same as the reference's BFstatus convention, corr_block.py:254):
 *   - every function returns int, 0 (XENG_STATUS_SUCCESS) on success, non-zero
 *     on error; nothing throws across the ABI; xengGetLastError() returns a
 *     thread-local message for the last failure.
 *   - the caller owns every data buffer; the library owns contexts and scratch.
 *   - contexts are process-global singletons like the reference's (one xGPU
 *     context: corr_block.py:249-256; one beamformer context shared by Beamform
 *     and BeamformSumBeams: beamform_sum_beams_block.py:186-187).
 *   - plain pointers and sizes only; "dev" pointers are HIP device pointers,
 *     "host" pointers are ordinary (ideally pinned) host memory.
 *
 * Two layers are exported:
 *   xeng*   raw-pointer functions (sizes are runtime arguments of Configure /
 *           Initialize; xGPU's were compile-time, install_xgpu.sh:5), and
 *   bf*     adapters with bifrost's names and BFarray* argument shapes, so a
 *           bifrost build could bind them 1:1.
 */
#ifndef XENG_H_
#define XENG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XENG_STATUS_SUCCESS            0
#define XENG_STATUS_INVALID_ARGUMENT   1
#define XENG_STATUS_INVALID_STATE      2
#define XENG_STATUS_DEVICE_ERROR       3
#define XENG_STATUS_UNSUPPORTED        4
#define XENG_STATUS_MEM_ALLOC_FAILED   5
#define XENG_STATUS_WOULD_BLOCK        6   /* a call that was asked not to wait would have had to */
#define XENG_STATUS_END_OF_DATA        7   /* ring readers: no more sequences / no more data in this sequence */

/* memory spaces, numbered as bifrost's BFspace [from memory of bifrost/src/bifrost/memory.h] */
#define XENG_SPACE_AUTO       0
#define XENG_SPACE_SYSTEM     1
#define XENG_SPACE_CUDA       2   /* device memory (HIP) -- keeps bifrost's name for the space */
#define XENG_SPACE_CUDA_HOST  3   /* pinned host memory */

/* mirrors bifrost's BFarray (bifrost/src/bifrost/array.h) [struct layout from memory, unverifiable here] */
#define XENG_MAX_DIMS 8
typedef struct XENGarray_ {
    void *data;
    int   space;
    int   dtype;
    int   ndim;
    long  shape[XENG_MAX_DIMS];
    long  strides[XENG_MAX_DIMS];
    int   immutable;
    int   big_endian;
    int   conjugated;
} XENGarray;

const char *xengGetLastError(void);
const char *xengVersion(void);

/* ---------------------------------------------------------------- device / memory plumbing
 * replaces bifrost.device.set_device / stream_synchronize and BFArray(space='cuda'|'cuda_host')
 * + copy_array (corr_acc_block.py:315-317, beamform_block.py:433, copy_block.py:146). */
int xengGetDeviceCount(int *count);
int xengSetDevice(int gpu);
int xengGetDevice(int *gpu);
int xengDeviceSynchronize(void);
int xengGetDeviceInfo(int gpu, int *num_cu, int *clock_khz, size_t *total_mem, char *name, int name_len);
/* "dddd:bb:dd.f" of a device: /sys/bus/pci/devices/<id>/{numa_node,local_cpulist} name the host cores next to it (the
 * reference pins every block thread, corr_block.py:336; sharding.pin_rank pins a rank to its GPU's NUMA node) */
int xengGetDevicePciBusId(int gpu, char *bus_id, int len);
int xengMalloc(void **ptr, size_t nbytes, int space);          /* XENG_SPACE_CUDA or XENG_SPACE_CUDA_HOST */
int xengFree(void *ptr, int space);
int xengMemcpy(void *dst, const void *src, size_t nbytes);     /* any direction, synchronous on return */
int xengMemcpyAsync(void *dst, const void *src, size_t nbytes);/* on the library's copy stream */
int xengMemset(void *dst, int value, size_t nbytes);
int xengStreamSynchronize(void);                               /* all library streams of the current device */

/* ---------------------------------------------------------------- stamps: what has been enqueued so far
 * A stamp names everything the library has enqueued on its streams of the current device up to now, by any thread -- including
 * gulps handed to xengXgpuKernelAsync whose contraction has not been enqueued yet.  It is complete when all of that has run.
 * Taking one enqueues nothing and costs a few loads; asking about one records an event only on a stream that is still
 * busy.  The span rings below stamp every allocation at the moment its last user lets go and reissue or free it only once the
 * stamp is complete: GPU memory lifetime does not rest on who dropped which Python reference when.
 * No reference counterpart: a bifrost ring is one circular buffer that is never freed while the pipeline runs. */
typedef struct xengStamp_ { unsigned long long w[16]; } xengStamp;
/* stream classes a stamp waits for (bits 32..36 of w[0]; xengStampNow sets all): the X-engine (staging stream, contractions,
 * registered gulps), the CorrAcc map stream, the beamformer stream, the copy stream, the span consumers' stream */
#define XENG_STREAMS_XGPU      1u
#define XENG_STREAMS_MAP       2u
#define XENG_STREAMS_BEAM      4u
#define XENG_STREAMS_COPY      8u
#define XENG_STREAMS_CONSUMER 16u
#define XENG_STREAMS_ALL      31u
/* a buffer that contractions only WRITE (a visibility span, a long accumulator; never handed over as a gulp): its stamp names
 * the last launch enqueued into that very buffer instead of every launch enqueued so far */
#define XENG_STREAMS_XGPU_OUT 32u
int xengStampNow(xengStamp *stamp);
int xengStampNowFor(xengStamp *stamp, const void *buf, unsigned classes);   /* the stamp of one buffer whose users are `classes` (0: all) */
/* non-blocking: *done = 1 when Wait would not wait; *waitable (may be NULL) = 0 when the stamp waits for an X-engine launch
 * that nobody has enqueued yet (only the owner of those gulps can end that: a dump, or xengXgpuReset) */
int xengStampDone(const xengStamp *stamp, int *done, int *waitable);
int xengStampWait(const xengStamp *stamp);

/* ---------------------------------------------------------------- span rings
 * The bookkeeping of the ring the blocks sit on -- bifrost.ring.Ring in the reference (lwa352-pipeline.py:147-155; protocol
 * used by the hot-path blocks: corr_block.py:342-350,388,433-452; corr_acc_block.py:313-318; beamform_block.py:440-450) --
 * for pipelines that run without bifrost: committed spans, reader cursors, back-pressure and the free list of span
 * allocations, native.  caltech-bifrost-dsp_amd/ring.py wraps these calls in the reference's Python protocol.
 * Every span is its own reference-counted allocation in `space` (system / device / pinned): a reader that keeps its span
 * handle may go on reading the bytes after the ring has moved on.  Calls that can wait take `may_block`: 0 returns
 * XENG_STATUS_WOULD_BLOCK instead of waiting (a caller that holds an interpreter lock asks first and gives the lock up only
 * for a call that has to sleep). */
typedef struct xengRing_ xengRing;
int xengRingCreate(xengRing **ring, const char *name, int space);
int xengRingDestroy(xengRing *ring);     /* wakes every waiter; spans still referenced stay valid until released */
int xengRingResize(xengRing *ring, size_t contig_bytes, size_t total_span);        /* ring.resize(): capacity in bytes (0: 4 x contig) */
/* Which of the library's streams touch this ring's spans (XENG_STREAMS_*; calls accumulate).  Every USER of a ring -- its
 * writer and each of its readers -- calls this exactly once (classes may be 0: a user that enqueues nothing on the spans, e.g.
 * a host reader whose copies are complete when it lets go).  A released span waits for the declared union -- the beamformer's
 * rings XENG_STREAMS_BEAM, Corr's XENG_STREAMS_XGPU ... -- so that a beam span is not held back by the 200 us contraction that
 * happened to be enqueued before its release; but ONLY while every user has declared: the ring counts the readers it has ever
 * opened plus its writer, and as long as there are more of those than declarations (a block that does not know the call, a
 * test reader with kernels of its own) every stamp waits for everything the library had enqueued, as on an undeclared ring. */
int xengRingDeclareStreams(xengRing *ring, unsigned classes);
/* the classes a span released now would wait for (XENG_STREAMS_* union, or all of them), declarations made, users seen */
int xengRingGetStampClasses(xengRing *ring, unsigned *classes, unsigned *declared, unsigned *users);
/* system-space rings hand out fresh zero-filled memory per span by default; on != 0 recycles released spans as the device /
 * pinned rings always do (contents: whatever the last user left, as in a circular bifrost ring) */
int xengRingSetRecycle(xengRing *ring, int on);
/* counters: allocations made, really freed, reissued from the free list, waits for a stamp at reissue, bytes skipped by readers */
int xengRingGetInfo(xengRing *ring, size_t *capacity, size_t *live_bytes, size_t *pool_bytes, int *nreaders, long long *nseq,
                    unsigned long long counters[5]);
/* writer: one at a time.  BeginSequence ends the sequence that was open. */
int xengRingBeginSequence(xengRing *ring, long long time_tag, const void *header, size_t header_len, int nringlet, long long *seq);
int xengRingEndSequence(xengRing *ring, long long seq);
int xengRingEndWriting(xengRing *ring);
/* WriteSpan(ring, nbytes, nonblocking) (corr_block.py:435): waits until the ring has room (guaranteed readers apply
 * back-pressure; without one the oldest span is overwritten, as in bifrost), then hands out span memory -- a released
 * allocation whose stamp is complete, or a fresh zero-filled one.  nonblocking: XENG_STATUS_WOULD_BLOCK + message when full. */
int xengRingReserve(xengRing *ring, long long seq, size_t nbytes, int nonblocking, int may_block, void **data, long long *span);
int xengRingCommit(xengRing *ring, long long seq, long long span, size_t nbytes);       /* the first nbytes of the span become readable */
/* publish the caller's own memory as the next span without a copy (a replay source: dummy_source_block.py:207-222 re-sends
 * the same gulps); the caller keeps it valid and unchanged while readers may hold it */
int xengRingCommitExternal(xengRing *ring, long long seq, void *data, size_t nbytes, int may_block);
/* readers.  A reader registered late starts at the oldest sequence still in the ring; data overwritten before a reader got
 * to it is skipped by whole gulps (*skipped bytes), as a bifrost reader skips frames. */
int xengRingOpenReader(xengRing *ring, int guarantee, int *reader);
int xengRingCloseReader(xengRing *ring, int reader);
/* XENG_STATUS_END_OF_DATA once writing has ended and every sequence has been seen; *header stays valid until the next call */
int xengRingNextSequence(xengRing *ring, int reader, int may_block, long long *seq, long long *time_tag, int *nringlet,
                         const void **header, size_t *header_len);
/* iseq.read(gulp_nbytes): first moves the reader `advance` bytes on (the previous gulp), then waits for the next gulp.
 * *nbytes < gulp_nbytes only for the short tail of an ended sequence; XENG_STATUS_END_OF_DATA when the sequence is over.
 * *span holds a reference on the memory: xengRingSpanRelease when done with it. */
int xengRingAcquire(xengRing *ring, int reader, size_t advance, size_t gulp_nbytes, int may_block, void **data, size_t *nbytes,
                    long long *span, size_t *skipped);
/* The same, but a gulp that lies in TWO committed spans comes back as two windows (*nparts = 2: data / nbytes / span of each,
 * in order) instead of a gathered copy -- for a consumer that can take its gulp in two parts (xengBeamformRunParts). */
int xengRingAcquireParts(xengRing *ring, int reader, size_t advance, size_t gulp_nbytes, int may_block, void *data[2], size_t nbytes[2],
                         long long span[2], int *nparts, size_t *skipped);
int xengRingSpanRelease(long long span);      /* a span handle from Reserve or Acquire: the last release stamps the allocation */
/* tests: tickets of a fake backend instead of the library's stream clocks (and a free list for system-space rings) */
typedef void (*xengRingStampNowFn)(void *user, unsigned long long stamp[2]);
typedef int (*xengRingStampDoneFn)(void *user, const unsigned long long stamp[2]);
typedef void (*xengRingStampWaitFn)(void *user, const unsigned long long stamp[2]);
int xengRingSetStampHooks(xengRing *ring, xengRingStampNowFn now, xengRingStampDoneFn done, xengRingStampWaitFn wait, void *user);

/* ---------------------------------------------------------------- X-engine (Corr)
 * replaces _bf.bfXgpuInitialize / bfXgpuKernel / bfXgpuCorrelate / bfXgpuGetOrder /
 * bfXgpuSubSelect / bfXgpuReorder. */

/* Sizes the next xengXgpuInitialize will use (xGPU compile-time NSTATION/NFREQUENCY/NTIME,
 * install_xgpu.sh:5; block args corr_block.py:221-231).  max_gulps_per_flush bounds how many
 * gulps are held back (kept in HBM and contracted in one launch at dump time; more gulps than
 * that are flushed early and accumulated in out_dev); 0 picks a default.  Defaults before any call: 352, 2, 96, 480. */
int xengXgpuConfigure(int nstand, int npol, int nchan, int ntime_gulp, int max_gulps_per_flush);

/* corr_block.py:251-256, xgpu_test.py:76.  Creates (or re-creates) the process-global context on `gpu`. */
int xengXgpuInitialize(int gpu);
int xengXgpuDestroy(void);

/* corr_block.py:445, xgpu_test.py:81-83.  in_dev: uint8[ntime_gulp][nchan][nstand][npol] 4+4 bit
 * (hi nibble real, lo nibble imag).  out_dev: int32[2][nchan][per_chan] planar re|im in xGPU
 * register-tile order (corr_block.py:27-58).  Gulps accumulate until a call with doDump=1, after
 * which out_dev holds the sum over all gulps since the previous dump and the accumulation restarts.
 * The same out_dev must be passed for every gulp of one integration (as Corr.main does: one
 * WriteSpan per integration, corr_block.py:433-435).  Synchronous: on return the input has been
 * consumed and, if doDump, the output is complete. */
int xengXgpuKernel(const void *in_dev, void *out_dev, int doDump);

/* Same, but enqueue only: the caller must keep in_dev valid AND UNCHANGED until the dump that consumes
 * it has completed (xengXgpuSync, or xengXgpuSyncLag covering that dump) before reading out_dev or
 * recycling in_dev.  On the default path the contraction kernel reads the gulps in place at dump time
 * (corner turn fused into its LDS staging): no copy of the gulp is made, in_dev must be 16-byte
 * aligned.  (No reference counterpart; this is how a ring-resident pipeline streams gulps.) */
int xengXgpuKernelAsync(const void *in_dev, void *out_dev, int doDump);
/* The same with CorrAcc's long accumulation (corr_acc_block.py:298-306, "a = b" / "a += b") fused into the dump: when
 * doDump is set and acc_dev is not NULL, every visibility the dump stores to out_dev is also assigned (acc_mode 1) or added
 * (acc_mode 2) to acc_dev, a planar int32 buffer of the same size and layout -- one pass over the accumulator in the
 * contraction's epilogue instead of a separate xengMapAssignI32 / xengMapAddI32 over both buffers (382 MB less HBM
 * traffic per config-2 dump).  Dumps that name the same accumulator are ordered; consecutive dumps overlap only when the
 * caller alternates between two accumulators (and adds them at the end of the long integration).  Readers of acc_dev:
 * xengXgpuSync / xengXgpuSyncLag as for out_dev.  XENG_STATUS_UNSUPPORTED on the non-default contraction paths. */
int xengXgpuKernelAsyncAcc(const void *in_dev, void *out_dev, int doDump, void *acc_dev, int acc_mode);
/* The two enqueue-only calls above wait when the caller is 256 launches ahead of the GPU (every launch owns one of 256
 * completion events).  This form never waits: XENG_STATUS_WOULD_BLOCK then, nothing enqueued; xengXgpuWaitLaunchSlot blocks
 * until a launch may be enqueued again.  (A caller that holds an interpreter lock tries, and gives the lock up to wait.) */
int xengXgpuTryKernelAsyncAcc(const void *in_dev, void *out_dev, int doDump, void *acc_dev, int acc_mode);
int xengXgpuWaitLaunchSlot(void);
/* A gulp handed over as the SLAB OF PACKETS it arrived in (round 4; layout: "Ingest" below; the gulp's window starts at seq0,
 * channel 0 of the pipeline is chan0_pipeline).  Enqueue-only like xengXgpuKernelAsync[Acc], same rules for out_dev / acc_dev /
 * doDump, and the slab must stay valid and unchanged until the dump that consumes it has completed.  On the device, without a host
 * round trip (round 5): every packet of the deployed geometry (one packet per sample and 64-input block, all channels) is entered
 * into an index -- the last packet that carries a (sample, block) wins, as in xengSnap2Unpack -- and the contraction kernel reads the
 * voltages out of the packets WHERE THEY LIE, through a table of their offsets: in order, shifted by lost packets, reordered,
 * duplicated, mixed with foreign or out-of-window packets, any packet count -- no scatter pass, no copy of the gulp at all;
 * samples nobody carries read as zero.  Only a slab that holds valid packets of ANOTHER geometry (several channel blocks per sample,
 * fewer inputs per packet), or one the table cannot describe (stride not a multiple of 16, unaligned, >= 2 GiB), goes through
 * zero-fill + scatter into the library's staging area, with the rules of xengSnap2Unpack.  The results are those of unpack +
 * correlate either way.  Slabs and plain gulps cannot be mixed inside one integration.  xengXgpuGetSlabFallbacks: gulps that took
 * the scatter since it was last called; xengXgpuGetSlabStats: those, and the gulps read in place whose packets were not all in
 * place (both wait for the staging stream).  No reference counterpart: bifrost's capture scatters on the CPU. */
int xengXgpuKernelAsyncSlab(const void *packets_dev, int npkt, size_t pkt_stride, uint64_t seq0, int chan0_pipeline, void *out_dev,
                            int doDump, void *acc_dev, int acc_mode);
int xengXgpuTryKernelAsyncSlab(const void *packets_dev, int npkt, size_t pkt_stride, uint64_t seq0, int chan0_pipeline, void *out_dev,
                               int doDump, void *acc_dev, int acc_mode);      /* never waits: see xengXgpuTryKernelAsyncAcc */
int xengXgpuGetSlabFallbacks(int *nfallback);
int xengXgpuGetSlabStats(int *nscattered, int *nirregular);
int xengXgpuSync(void);
/* Wait until all but the last `lag` (0..3) dumps are complete -- lag 1 lets a streaming caller enqueue
 * integration n+1 (into a different out_dev) before it waits for integration n, so the contraction of
 * n+1 fills the CUs that the contraction of n vacates.  lag 0 waits for the latest dump. */
int xengXgpuSyncLag(int lag);
/* The non-blocking form: *done = 1 when xengXgpuSyncLag(lag) would return without waiting.  (A caller that shares an
 * interpreter lock with other threads asks first and only gives the lock up for a call that really has to wait.) */
int xengXgpuDumpDone(int lag, int *done);

/* Drop the gulps staged and the partial sums accumulated since the last dump (an integration that
 * is abandoned, e.g. when a new start_time command interrupts it: corr_block.py:392-404 resets
 * `start` mid-integration).  No reference counterpart: xGPU would silently carry the partial sums
 * into the next integration. */
int xengXgpuReset(void);

/* xgpu_test.py:86-89: host-buffer variant (H2D, kernel, D2H on dump). */
int xengXgpuCorrelate(const void *in_host, void *out_host, int doDump);

/* corr_block.py:317-333.  Host arrays: antpol_to_input int32[nstand][npol];
 * antpol_to_bl, is_conj int32[nstand][nstand][npol][npol] indexed [s0][s1][p0][p1]
 * (corr_subsel_block.py:248-250).  is_conj=1: negate the stored imaginary part to obtain
 * x[s0,p0]*conj(x[s1,p1]) (corr_output_full_block.py:582-591). */
int xengXgpuGetOrder(const int32_t *antpol_to_input, int32_t *antpol_to_bl, int32_t *is_conj);

/* corr_subsel_block.py:298.  in_dev: planar xGPU buffer; out_dev: int32[nchan/nchan_sum][nvis][2];
 * vismap_dev/conj_dev: int32[nvis] device arrays. */
int xengXgpuSubSelect(const void *in_dev, void *out_dev, const int32_t *vismap_dev,
                      const int32_t *conj_dev, int nvis, int nchan_sum);

/* corr_output_full_block.py:669 + :461-467 / :512-519 done on the device: planar xGPU buffer -> the packet
 * payloads CorrOutputFull sends, one per dual-pol baseline s0 <= s1 in sending order
 * (k = s0*nstand - s0(s0-1)/2 + s1 - s0): out_dev int32[nstand(nstand+1)/2][npol][npol][nchan][2] (fmt 0,
 * send_packets_py) or [..][nchan][npol][npol][2] (fmt 1, COR).  Maps: device copies of the GetOrder
 * arrays.  The caller must have synchronised the contraction that produced in_dev.  Synchronous. */
int xengXgpuPacketize(const void *in_dev, void *out_dev, const int32_t *antpol_to_bl_dev,
                      const int32_t *is_conj_dev, int fmt);

/* corr_output_full_block.py:669.  Host: planar xGPU buffer -> int32[nstand][nstand][npol][npol][nchan][2]. */
int xengXgpuReorder(const void *in_host, void *out_host, const int32_t *antpol_to_bl, const int32_t *is_conj);

/* sizes of the current context */
int xengXgpuGetInfo(int *nstand, int *npol, int *nchan, int *ntime_gulp, int64_t *matlen, int *max_gulps);

/* which contraction path the current context runs: fused_corner_turn = 1 when gulps are read in place
 * (ninput % 16 == 0, ntime_gulp % 96 == 0, not disabled with XENG_RAW=0), else the two-pass path
 * (corner turn into a fragment-major staging area); fp6 is always 0 (the FP6 route was removed). */
int xengXgpuGetPath(int *fused_corner_turn, int *fp6);
/* the contraction kernel plain and slab launches of the current context take: 4 waves per work-group on v_mfma_i32_32x32x32_i8
 * (mfma_k 32: the default, the two-pass path, and always for dumps that feed a long accumulator) or, with XENG_KLOOP=16, 8 waves
 * on v_mfma_i32_16x16x64_i8 (xcorr_fused16.h; mfma_k 64) */
int xengXgpuGetKernel(int *waves_per_group, int *mfma_k);

/* profiling: HIP events around each kernel on the context's stream.  GetTimes returns and clears
 * the totals (ms) and launch counts since the last call: [0]=corner turn (two-pass path) or raw
 * gulp copy (synchronous calls on the fused path), [1]=MFMA contraction. */
int xengXgpuSetProfiling(int enable);
int xengXgpuGetTimes(double ms[2], int count[2]);

/* ---------------------------------------------------------------- Ingest (SNAP2 F-engine packets)
 * Scatter received packets into a gulp on the device.  In the reference this scatter happens on the CPU inside
 * bifrost's UDP capture, which capture_block.py:296-305 only configures; the packet format is pinned by the
 * reference's transmitters (test_tx_vectors.py:38-48,103-108; test_tx_mt.c:39-49): 32-byte big-endian header
 * `>QLHHHHLLL` = seq, sync_time, npol, npol_tot, nchan, nchan_tot, chan_block_id, chan0, pol0, then
 * u8[nchan][npol] 4+4-bit samples.  packets_dev: npkt packets, pkt_stride bytes apart (any order, duplicates
 * allowed).  out_dev: u8[ntime][nchan_tot][npol_tot]; row c of a packet lands at
 * [seq - seq0][chan0 - chan0_pipeline + c][pol0 ..].  Packets outside the window [seq0, seq0+ntime) or outside
 * the gulp geometry are dropped and counted.  clear != 0: samples that no packet covers read as 0 (blanked) -- a slab
 * that covers the whole gulp is scattered without any zero-fill, otherwise the gulp is zero-filled and scattered again.
 * Synchronous; the counters may be NULL. */
int xengSnap2Unpack(const void *packets_dev, int npkt, size_t pkt_stride, void *out_dev, uint64_t seq0, int ntime,
                    int chan0_pipeline, int nchan_tot, int npol_tot, int clear, int *nplaced, int *ndropped);
/* Same, enqueue only, on the X-engine's staging stream: a gulp unpacked this way and then passed to
 * xengXgpuKernelAsync is complete before the contraction of its dump reads it.  No counters are returned. */
int xengSnap2UnpackAsync(const void *packets_dev, int npkt, size_t pkt_stride, void *out_dev, uint64_t seq0, int ntime,
                         int chan0_pipeline, int nchan_tot, int npol_tot, int clear);
/* Packets the enqueue-only calls have dropped (out of window / foreign / malformed) since this was last called; waits for
 * the staging stream and clears the count.  The synchronous call reports its own drops in *ndropped. */
int xengSnap2GetAsyncDrops(int *ndropped);

/* ---------------------------------------------------------------- test / bench harness (no pipeline calls these)
 * Emulator side of the F-engine link: a receiver reuses its slab buffers; this re-stamps the sequence numbers of a device-resident
 * slab for its next window -- packet p gets seq0 + p / pkts_per_seq (big-endian, header bytes 0..7), nothing else changes.  Complete
 * on return.  (The Python side of the harness lives in the extension's `_xfast.bench` sub-module: a source and sinks that are not
 * Python threads.) */
int xengSnap2StampSeq(void *packets_dev, int npkt, size_t pkt_stride, uint64_t seq0, int pkts_per_seq);

/* ---------------------------------------------------------------- CorrAcc
 * replaces bifrost.map "a = b" / "a += b" on int32 (corr_acc_block.py:304,306).  Device pointers;
 * enqueued on the library's map stream; xengStreamSynchronize() (corr_acc_block.py:317) completes it. */
int xengMapAssignI32(void *a_dev, const void *b_dev, size_t nwords);
int xengMapAddI32(void *a_dev, const void *b_dev, size_t nwords);
/* a = (add ? a : 0) + srcs[0] + ... + srcs[nsrc - 1] in one pass (srcs: HOST array of nsrc device pointers, 1 <= nsrc <=
 * XENG_MAP_SUM_MAX).  The reference adds every dump as it arrives (corr_acc_block.py:298-306: 574 MB of traffic per config-2
 * dump); int32 addition wraps, so any grouping gives the same words, and with 288 GB of HBM CorrAcc keeps the spans of a
 * group of dumps and sums them together: 191 + 382 / nsrc MB per dump.  Map stream, like the two calls above. */
#define XENG_MAP_SUM_MAX 16
int xengMapSumI32(void *a_dev, const void *const *srcs_dev, int nsrc, size_t nwords, int add);
int xengMapSync(void);   /* wait for the map stream only */

/* ---------------------------------------------------------------- Beamformer
 * replaces _bf.bfBeamformInitialize / Run / Integrate / IntegrateSingleBeam. */

/* beamform_block.py:251-253.  ntime_blocks==0: voltage mode.  >0: "integrated power" mode the reference
 * marks experimental (beamform_block.py:108-110) -- implemented as Run then Integrate (parity unpinned). */
int xengBeamformInitialize(int gpu, int ninput, int nchan, int ntime, int nbeam, int ntime_blocks);
int xengBeamformDestroy(void);

/* beamform_block.py:446-449.  in_dev uint8[ntime][nchan][ninput] 4+4 bit; weights_dev
 * cf32[nchan][nbeam][ninput] interleaved; out_dev cf32[nchan][nbeam][ntime]:
 * out[c,b,t] = sum_i w[c,b,i]*x[t,c,i] (beamformer_test.py:76-84).  Asynchronous on the beamformer
 * stream; xengBeamformSync()/xengStreamSynchronize() is the BFSync() of beamform_block.py:450. */
int xengBeamformRun(const void *in_dev, void *out_dev, const void *weights_dev);
/* Same, for callers that know when the weights change: the library re-splits the fp32 weights into the
 * bf16 terms its MFMA kernel uses only when (weights_dev, weights_version) differs from the last call
 * (version 0 = always re-split, which is what xengBeamformRun / bfBeamformRun do). */
int xengBeamformRunVersioned(const void *in_dev, void *out_dev, const void *weights_dev, long long weights_version);
/* Run* is enqueue-only except in the integrated-power mode right after a weight upload, where it waits once for the routing
 * answer of the new weights.  This form never waits: XENG_STATUS_WOULD_BLOCK then (the weights are prepared and remembered;
 * call xengBeamformRunVersioned with the same arguments to wait and run). */
int xengBeamformTryRunVersioned(const void *in_dev, void *out_dev, const void *weights_dev, long long weights_version);
/* The gulp in two parts: samples [0, ntime0) at in0_dev, samples [ntime0, ntime) at in1_dev -- two consecutive spans of the
 * input ring taken as ONE beamformer gulp, one launch, no gathered copy.  The reference's Beamform reads GPU_NGULP = 2 capture
 * gulps per call (lwa352-pipeline.py:172,279-282: ntime_gulp = 2 x 480) out of bifrost's circular buffer, where two gulps
 * are contiguous; on a ring of separate spans this call gives the same.  RunVersioned semantics otherwise; the Try form never
 * waits (see xengBeamformTryRunVersioned). */
int xengBeamformRunParts(const void *in0_dev, int ntime0, const void *in1_dev, void *out_dev, const void *weights_dev, long long weights_version);
int xengBeamformTryRunParts(const void *in0_dev, int ntime0, const void *in1_dev, void *out_dev, const void *weights_dev, long long weights_version);
/* The gulp as the SLABS OF PACKETS it arrived in (round 4; cf. xengXgpuKernelAsyncSlab, layout: "Ingest" below): one slab
 * (packets1_dev NULL) or two consecutive ones -- samples [0, ntime0) from seq0 on, samples [ntime0, ntime) from seq0 + ntime0 on;
 * ntime0 a multiple of 16, inputs a multiple of 16.  Each slab is verified on the beam stream; a regular one is read by the
 * beamformer kernels where it lies, any other is scattered into the context's scratch gulp first (xengSnap2Unpack's rules), so
 * the beams are those of unpack + Run either way -- bit for bit, the same kernels do the arithmetic.  RunVersioned semantics
 * otherwise; the slabs must stay valid and unchanged until the call's kernels have completed (xengBeamformMark).
 * xengBeamformGetSlabFallbacks: parts that took the scatter since it was last called (waits for the beam stream). */
int xengBeamformRunSlabs(const void *packets0_dev, int npkt0, int ntime0, const void *packets1_dev, int npkt1, size_t pkt_stride,
                         uint64_t seq0, int chan0_pipeline, void *out_dev, const void *weights_dev, long long weights_version);
int xengBeamformTryRunSlabs(const void *packets0_dev, int npkt0, int ntime0, const void *packets1_dev, int npkt1, size_t pkt_stride,
                            uint64_t seq0, int chan0_pipeline, void *out_dev, const void *weights_dev, long long weights_version);   /* never waits: see xengBeamformTryRunVersioned */
int xengBeamformGetSlabFallbacks(int *nfallback);
/* (round 5) On a lossy link -- more than a quarter of the parts of the last eight calls not regular -- the beamformer reads the parts
 * where they lie as well, through a packet index built by the verify launch (lost, shifted, reordered, duplicated packets; samples
 * nobody carries read as zero; the int8 and bf16 kernels, not the fp32 one); XENG_SLAB_TABLES=1 / 0 pins that on / off.
 * xengBeamformGetSlabStats: parts scattered, and parts read through an index that was not regular, since the last call. */
int xengBeamformGetSlabStats(int *nscattered, int *nirregular);

/* beamform_sum_beams_block.py:243-246.  in_dev cf32[nchan][nbeam][ntime];
 * out_dev f32[nbeam/2][ntime/ntime_sum][nchan][4] = [XX, YY, Re XY*, Im XY*]. */
int xengBeamformIntegrate(const void *in_dev, void *out_dev, int ntime_sum);

/* beamform_sum_single_beam_block.py:114: one dual-pol beam -> f32[ntime/ntime_sum][nchan][4]. */
int xengBeamformIntegrateSingleBeam(const void *in_dev, void *out_dev, int ntime_sum, int beam_id);
/* beamform_vlbi_output_block.py:258-276 (BeamformVlbiOutput): the voltage beams of one gulp -> ntime "ibeam" packets, built on
 * the beamformer's stream (xengBeamformMark / Wait / TicketDone cover it; a live context is required, INVALID_STATE otherwise,
 * but every size comes from the arguments).  in_dev cf32[nchan][nbeam][ntime] (the Beamform output span, 8-byte aligned; never
 * written).  Packet t lives in slot t at out_dev + t*pkt_stride (out_dev 16-byte aligned, pkt_stride a multiple of 16 and at
 * least 16 + 8*nchan*nbeam_pkt) and is the byte range [1, 16 + 8*nchan*nbeam_pkt) of its slot:
 *   bytes [1,16)  header, the packed 15-byte `struct ibeam` of the reference docstring (:141-149):
 *                 u8 server, gbe, nchan, nbeam (= nbeam_hdr), nserver; u16 chan0; u64 seq = seq0 + t; multi-byte fields big-endian
 *   bytes [16,..) payload cf32[nchan][nbeam_pkt] = beams [beam0, beam0+nbeam_pkt) at sample t, bits copied unchanged, native
 *                 byte order (bifrost sends the numpy payload as it lies)
 * so a sender passes slot[1 : 16 + payload] as one contiguous buffer.  Byte 0 and the bytes after the packet are left as they were.
 * The layout is UNPINNED: the docstring also says "32 byte header" (:137) and a uint32 chan0 (:174), and bifrost's ibeam writer
 * is an empty submodule in the reference tree; this follows its struct.  Rejected without a launch: null or misaligned
 * pointers, beams outside [0, nbeam), nchan / nbeam_hdr / nserver / server / gbe above 255, chan0 above 65535, a stride too
 * small for header and payload. */
int xengBeamformPacketizeVoltages(const void *in_dev, void *out_dev, int nchan, int nbeam, int ntime, int beam0, int nbeam_pkt,
                                  size_t pkt_stride, int server, int gbe, int nbeam_hdr, int nserver, int chan0, uint64_t seq0);
int xengBeamformSync(void);
/* Completion tickets on the beamformer's stream: Mark returns a ticket for everything enqueued so far (Run, Integrate,
 * by any thread), Wait blocks until that point has been reached.  They let the Beamform / BeamformSumBeams blocks keep
 * several gulps in flight and commit each output span when its own kernels are done (no reference counterpart: the
 * reference waits for the whole stream after every gulp, beamform_block.py:450). */
int xengBeamformMark(unsigned long long *ticket);
int xengBeamformWait(unsigned long long ticket);
int xengBeamformTicketDone(unsigned long long ticket, int *done);   /* non-blocking: *done = 1 when Wait would not wait */
int xengBeamformSetProfiling(int enable);
int xengBeamformGetTimes(double ms[2], int count[2]);   /* [0]=Run, [1]=Integrate */
/* How the last weight upload was routed (waits for the beam stream): (channel, beam tile) pairs in all, pairs that run on
 * the bf16x3 kernel because their fixed-point image would not hold the 1e-5 bar, and outlier inputs that the int8x3
 * kernel adds in fp32 (summed over tiles).  Zeros for the bf16x3 / f32 modes.  No reference counterpart: the
 * reference's cuBLAS CF32 GEMM (bf_src/cublas_beamform.cu:248-276) has one route. */
int xengBeamformGetRouteInfo(int *tiles_total, int *tiles_bf16, int *outlier_inputs);

/* ---------------------------------------------------------------- Upchannelising beamformer
 * UpchanBeamform (lwa352-upchan-bf.py:94-113 with beamform_offline_block.py:211-245): a context of its own, independent of the
 * Beamform context (either may live without the other), whose kernel runs on the beamformer's stream -- rings declared 'beam'
 * cover it, and xengBeamformSync waits for it too.  One kernel per gulp (csrc/upchan_kernels.h):
 *   in       u8[ntime][nchan][ninput], 4+4 bit as Beamform reads it; never written
 *   frames   frame f = samples [f*N, f*N + N) of the gulp (N = nupchan in {8, 16, 32, 64}); with the PFB front end of
 *            xengUpchanSetPfb (below) it also reads the (P-1)*N samples before it, otherwise frames never cross gulps
 *   FFT      X[f,c,i,k] = sum_n x[f*N+n, c, i] exp(-2 pi i k n / N), forward, no normalisation; fine channel j = (k + N/2) mod N,
 *            so j ascends in frequency: centre sfreq + c*bw/nchan + (j - N/2)*bw/(nchan*N)
 *   weights  cf32[nchan][N][nbeam][ninput], indexed by j; read as they are (16-byte aligned)
 *   nframe_sum 0 (voltage):  out cf32[ntime/N][nbeam][nchan][N], v[f,b,c,j] = sum_i w[c,j,b,i] X[f,c,i,j]
 *   nframe_sum > 0 (power):  out f32[ntime/N/nframe_sum][nbeam][nchan][N], sum of |v|^2 over nframe_sum consecutive frames
 * (out 16-byte aligned; nothing past it is written).  fp32 throughout, the sum over inputs in a fixed order: bit-identical from
 * run to run.  Rejected at Initialize: ninput not a positive multiple of 4, nupchan outside the set, ntime % nupchan,
 * nframe_sum not dividing ntime/nupchan, nbeam*nupchan above 1024.  Rejected at Run without a launch: null or misaligned
 * pointers; RunParts: parts that are not positive multiples of nupchan. */
int xengUpchanInitialize(int gpu, int ninput, int nchan, int ntime, int nupchan, int nbeam, int nframe_sum);
/* The same context in dual-pol mode (replaces any live one, as Initialize does; either call replaces it again).  Beams 2p / 2p+1
 * are the X / Y pols of pair p, and Run / RunParts (same input and weight contracts) write their 2x2 products instead of |v|^2,
 * as BeamformSumBeams does for the coarse-channel beams (beamformer_sum_test.py:64-77):
 *   out f32[ntime/N/nframe_sum][nbeam/2][nchan][N][4] = [XX, YY, Re(XY*), Im(XY*)], X = v[f,2p,c,j], Y = v[f,2p+1,c,j],
 *            XX = sum |X|^2, YY = sum |Y|^2, XY* = sum X conj(Y), each sum over the nframe_sum frames of a window
 * Each 4-float group is 16-byte aligned (one vector store); nothing past the output is written.  XX / YY of pair p are bit-identical
 * to the power mode's outputs of beams 2p / 2p+1 under the same input and weights; the cross terms are a fixed-order fp32 chain of
 * their own: bit-identical from run to run.  Rejected at Initialize, before any device is touched: everything Initialize rejects,
 * an odd nbeam, nframe_sum = 0. */
int xengUpchanInitializeDualPol(int gpu, int ninput, int nchan, int ntime, int nupchan, int nbeam, int nframe_sum);
/* weights_version as xengBeamformRunVersioned's; the kernel reads the fp32 weights directly, so it is accepted and ignored */
int xengUpchanRun(const void *in_dev, void *out_dev, const void *weights_dev, long long weights_version);
/* one gulp in two spans: samples [0, ntime0) at in0_dev, [ntime0, ntime) at in1_dev */
int xengUpchanRunParts(const void *in0_dev, int ntime0, const void *in1_dev, void *out_dev, const void *weights_dev,
                       long long weights_version);
/* Polyphase filter bank front end (no reference counterpart: its offline chain is the plain FFT).  P = ntap taps, h = coeffs,
 * P*N fp32 values on the host, x[t] = the decoded samples of one (coarse channel, input), t counting samples of the continuous
 * stream.  Output frame f of a gulp reads its own frame and the P-1 frames before it:
 *   y[f, n] = sum_{k=0}^{P-1} h[k*N + n] x[(f - P + 1 + k)*N + n],  n = 0..N-1, a fixed-order fp32 fmaf chain (k ascending)
 *   X[f, c, i, k'] = sum_n y[f, n] exp(-2 pi i k' n / N); everything after X (fine channel order, weights, beams, power,
 *   dual-pol) is unchanged.  Output frame f is still labelled by gulp frame f: the group delay of (P-1)*N/2 samples is not
 *   compensated.  Samples before the first one the context has seen since SetPfb / Reset count as zero.
 * The context keeps the last (P-1)*N samples u8[(P-1)*N][nchan][ninput] in a history on the device, refreshed from each gulp's
 * tail by D2D copies on the beamformer's stream behind its launch.  ntap = 1 with coeffs = NULL: the plain FFT (the state after
 * Initialize / InitializeDualPol); ntap = 1 with coefficients: a windowed FFT.  Waits for the context's work in flight, then
 * uploads the coefficients and clears the history.  Rejected before anything is touched: ntap outside 1..8, NULL coeffs with
 * ntap > 1, a non-finite coefficient, ntime < (P-1)*N; without a context XENG_STATUS_INVALID_STATE. */
int xengUpchanSetPfb(int ntap, const float *coeffs);
/* the next Run sees zeros before its gulp (a gap, a new sequence): host state only, nothing is launched */
int xengUpchanReset(void);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengBeamformMark / Wait / TicketDone */
int xengUpchanMark(unsigned long long *ticket);
int xengUpchanWait(unsigned long long ticket);
int xengUpchanTicketDone(unsigned long long ticket, int *done);
int xengUpchanSync(void);
int xengUpchanDestroy(void);

/* ---------------------------------------------------------------- Upchannelised correlator
 * UpchanCorr (lwa352-upchan-imag.py:95-106: fft over fine_time, merge_axes, FrequencySelectBlock, blocks.correlate): a context
 * of its own, independent of the Upchan and Beamform contexts, whose kernels run on the beamformer's stream -- rings declared
 * 'beam' cover them, and xengBeamformSync waits for them too.  Three kernels (csrc/upchan_corr_kernels.h):
 *   in       u8[ntime][nchan][ninput], 4+4 bit as Beamform reads it; never written
 *   frames   frame f = samples [f*N, f*N + N) of the gulp (N = nupchan in {1, 2, 4, 8, 16, 32, 64}); with the PFB front end of
 *            xengUpchanCorrSetPfb (below) it also reads the (P-1)*N samples before it, otherwise frames never cross gulps
 *   FFT      X[f,c,i,k] = sum_n x[f*N+n, c, i] exp(-2 pi i k n / N), forward, no normalisation; fine channel j = (k + N/2) mod N
 *            (ascending in frequency), merged index c*N + j; the fine channels [fine_lo, fine_hi) of that axis are kept, as
 *            c' = c*N + j - fine_lo (the others are never correlated).  The twiddles 1 and -i are applied exactly, so N <= 4 is
 *            exact on integer data.
 *   out      cf32[nfine][ninput][ninput], nfine = fine_hi - fine_lo, V[c', i, j] = sum_f X[f, c', i] conj(X[f, c', j]) over every
 *            frame accumulated since the last Dump / Reset (oracle golden_corr's convention; the X-engine's xgpu_lookup gives
 *            the conjugate).  The full Hermitian matrix is written, so which triangle a convention keeps does not matter:
 *            the lower triangle (i >= j) as accumulated, the upper as its exact conjugate, diagonal imaginary parts exactly 0.
 *            16-byte aligned; nothing past it is written.
 * Numerics: fp32.  Re += Xr_i Xr_j + Xi_i Xi_j and Im += Xi_i Xr_j - Xr_i Xi_j on f32-input MFMAs, frames in order, two per
 * instruction (a gulp with an odd frame count is padded with a zero frame), one fmaf chain per gulp, the gulps' sums added
 * in order: each element is one fixed sum over the integration, the same whatever nstage, however the gulps came in (whole
 * or in parts), from run to run.  Within 1e-6 of sum_f |X_i||X_j| of the exact value; exact on integer data below 2^24
 * (N <= 4).  No atomics.
 * Accumulate stages a gulp's fine channels; every nstage gulps (0: a default of up to 8 within 4 GiB of staging) and at Dump
 * the staged frames are contracted into an fp32 accumulator of nfine * ceil(ninput/32)*(ceil(ninput/32)+1)/2 * 8 KiB.
 * ninput is padded internally to a multiple of 32 with zero inputs: any positive ninput is accepted.
 * Rejected at Initialize: a non-positive size, nupchan outside the set, ntime % nupchan, an empty or out-of-range
 * [fine_lo, fine_hi), nstage < 0.  Rejected without a launch: null or misaligned pointers; AccumulateParts: parts that are not
 * positive multiples of nupchan.  Without a context: XENG_STATUS_INVALID_STATE. */
int xengUpchanCorrInitialize(int gpu, int ninput, int nchan, int ntime, int nupchan, int fine_lo, int fine_hi, int nstage);
/* the live context's nfine and staging depth (nstage as resolved) */
int xengUpchanCorrGetInfo(int *nfine, int *nstage);
/* enqueue only: one gulp, or one gulp in two spans (samples [0, ntime0) at in0_dev, [ntime0, ntime) at in1_dev) */
int xengUpchanCorrAccumulate(const void *in_dev);
int xengUpchanCorrAccumulateParts(const void *in0_dev, int ntime0, const void *in1_dev);
/* enqueue only: contract what is staged, write the integration to out_dev, start the next one from zero */
int xengUpchanCorrDump(void *out_dev);
/* drop the integration in progress and invalidate the PFB history (nothing is launched) */
int xengUpchanCorrReset(void);
/* The PFB front end of xengUpchanSetPfb for this context: the same definition, history, rules and checks (CorrInitialize
 * returns the context to ntap = 1 without coefficients).  Dump leaves the history alone: contiguous integrations continue the
 * filter. */
int xengUpchanCorrSetPfb(int ntap, const float *coeffs);
/* enqueue only: the history from this gulp's tail (one part, or two as AccumulateParts takes them), nothing accumulated --
 * for a reader that waits for an integration boundary; nothing to do without a history (ntap = 1) */
int xengUpchanCorrPrime(const void *in_dev);
int xengUpchanCorrPrimeParts(const void *in0_dev, int ntime0, const void *in1_dev);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengUpchanCorrMark(unsigned long long *ticket);
int xengUpchanCorrWait(unsigned long long ticket);
int xengUpchanCorrTicketDone(unsigned long long ticket, int *done);
int xengUpchanCorrSync(void);
int xengUpchanCorrDestroy(void);

/* ---------------------------------------------------------------- Fine-channel power beams from live beams
 * UpchanSumBeams (no reference counterpart: the reference's fine-channel beams are offline only): a context of its own,
 * independent of the Beamform, Upchan and UpchanCorr contexts, whose kernels run on the beamformer's stream -- rings declared
 * 'beam' cover them, and xengBeamformSync waits for them too.  One kernel per gulp (csrc/upchan_beams_kernels.h):
 *   in       cf32[nchan][nbeam][ntime], the output of xengBeamformRun in voltage mode, 16-byte aligned; never written
 *   pairs    p in [pair0, pair0 + npair): X = beam 2p, Y = beam 2p+1 (BeamformSumBeams' convention)
 *   frames   frame f = samples [f*N, f*N + N) of the gulp (N = nupchan in {8, 16, 32, 64}); with the PFB front end of
 *            xengUpchanSumBeamsSetPfb (below) it also reads the (P-1)*N samples before it, otherwise frames never cross gulps
 *   FFT      V[f,c,b,k] = sum_n v[c,b,f*N+n] exp(-2 pi i k n / N), forward, no normalisation; fine channel j = (k + N/2) mod N,
 *            so j ascends in frequency: centre sfreq + c*bw/nchan + (j - N/2)*bw/(nchan*N)
 *   products per pair, fine channel and frame, X = V[f,c,2p,j], Y = V[f,c,2p+1,j]: XX = |X|^2, YY = |Y|^2,
 *            Re XY* = xr*yr + xi*yi, Im XY* = xi*yr - xr*yi
 *   windows  W = nframe_sum frames, F = ntime/N frames per gulp.  W | F: F/W windows per gulp.  F | W: one window per G = W/F
 *            gulps, carried in a device accumulator of the context; each gulp's partial sum is a fixed-order chain over its
 *            frames and the partial sums of a window's gulps are added in order.  Any other W is rejected.
 *   out      f32[nwin][npair][nchan][N][4] = [XX, YY, Re XY*, Im XY*], nwin = F/W (W | F) or 1 (F | W): the layout of
 *            xengUpchanInitializeDualPol's output.  16-byte aligned; nothing past it is written.
 * Numerics: fp32, every sum a fixed-order chain, no atomics: bit-identical from run to run, whatever else runs on the GPU.
 * In exact arithmetic the output equals xengUpchanInitializeDualPol's on the beamformer's input with the coarse weights copied
 * to every fine channel (the beamformer, the PFB and the FFT are linear).
 * Rejected at Initialize, before any device is touched: a non-positive size (pair0 < 0), nupchan outside the set,
 * ntime % nupchan, W neither dividing nor a multiple of F, pairs outside [0, nbeam/2).  Rejected at Run / Prime without a
 * launch: null (Run: where the gulp completes a window) or misaligned pointers.  Without a context: XENG_STATUS_INVALID_STATE. */
int xengUpchanSumBeamsInitialize(int gpu, int nchan, int nbeam, int ntime, int nupchan, int pair0, int npair, int nframe_sum);
/* the live context's gulps per window (G, 1 when W | F), windows per gulp (F/W, 1 when F | W), and how many gulps of the window
 * in progress Run has taken (0 .. G-1; the next Run writes out_dev when it is G-1) */
int xengUpchanSumBeamsGetInfo(int *gulps_per_window, int *windows_per_gulp, int *pos);
/* enqueue only: one gulp.  out_dev is written by a gulp that completes a window; with G > 1 it may be NULL on the others. */
int xengUpchanSumBeamsRun(const void *in_dev, void *out_dev);
/* The PFB front end of xengUpchanSetPfb applied to the complex beam samples: y[f,n] = sum_k h[k*N + n] v[(f-P+1+k)*N + n], a
 * fixed-order fp32 fmaf chain (k ascending), then the FFT.  The same rules and checks (Initialize returns the context to ntap = 1
 * without coefficients): waits for the context's work in flight, uploads the coefficients, clears the history; rejects ntap
 * outside 1..8, NULL coeffs with ntap > 1, a non-finite coefficient, ntime < (P-1)*N.  The history of the last (P-1)*N samples
 * of every selected (channel, beam) row lives on the device in two halves: the kernel reads one and writes the other. */
int xengUpchanSumBeamsSetPfb(int ntap, const float *coeffs);
/* enqueue only: the history from this gulp's tail, nothing summed and the window position unchanged -- for a reader that
 * waits for a window boundary; nothing to do without a history (ntap = 1) */
int xengUpchanSumBeamsPrime(const void *in_dev);
/* drop the window in progress and invalidate the PFB history (host state only, nothing is launched) */
int xengUpchanSumBeamsReset(void);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengUpchanSumBeamsMark(unsigned long long *ticket);
int xengUpchanSumBeamsWait(unsigned long long ticket);
int xengUpchanSumBeamsTicketDone(unsigned long long ticket, int *done);
int xengUpchanSumBeamsSync(void);
int xengUpchanSumBeamsDestroy(void);

/* ---------------------------------------------------------------- Per-input fine-channel spectra
 * UpchanSpectra (no reference counterpart: the reference has no per-input fine-channel product and no interference
 * statistic): per input and fine channel, the power and the squared power summed over a window of frames -- the fine-resolution
 * bandpass of every input and, from the two together, the spectral-kurtosis estimator (blocks/spectral_kurtosis.py).  A context
 * of its own, independent of the Beamform, Upchan, UpchanCorr and UpchanSumBeams contexts, whose kernel runs on the
 * beamformer's stream -- rings declared 'beam' cover it, and xengBeamformSync waits for it too.  One kernel per gulp
 * (csrc/upchan_spectra_kernels.h); the channelised data never reaches memory:
 *   in       u8[ntime][nchan][ninput], 4+4 bit as Beamform reads it; never written
 *   frames   frame f = samples [f*N, f*N + N) of the gulp (N = nupchan in {1, 2, 4, 8, 16, 32, 64}); with the PFB front end of
 *            xengUpchanSpectraSetPfb (below) it also reads the (P-1)*N samples before it, otherwise frames never cross gulps
 *   FFT      X[f,c,i,k] = sum_n x[f*N+n, c, i] exp(-2 pi i k n / N), forward, no normalisation; fine channel j = (k + N/2) mod N
 *            (ascending in frequency, as UpchanBeamform and UpchanCorr order them).  The twiddles 1 and -i are applied exactly,
 *            so N <= 4 is exact on integer data.
 *   moments  p[f,c,j,i] = fmaf(re X, re X, im X * im X) in fp32 (|X|^2: the product of the imaginary part rounded, then one
 *            fused multiply-add);  S1[w,c,j,i] = sum_f p,  S2[w,c,j,i] = sum_f p * p (the same fp32 p squared), over the
 *            W = nframe_sum frames of window w
 *   windows  F = ntime/N frames per gulp.  W | F: F/W windows per gulp.  F | W: one window per G = W/F gulps, carried in a
 *            device accumulator of the context: gulp 0 of a window assigns it, the following ones add to it in order, the last
 *            writes accumulator + its own sum to out (no clearing pass; out is not touched by the other gulps).  Any other W
 *            is rejected.
 *   out      f32[nwin][2][nchan][N][ninput], plane 0 = S1, plane 1 = S2; nwin = F/W (W | F) or 1 (F | W).  16-byte aligned;
 *            nothing past it is written.
 * Numerics: fp32.  The frames f0, f0 + 1, ... of a window (or of a gulp's part of it) are dealt to s = min(4, W, F) slots,
 * frame f0 + m to slot m mod s; each slot sums its frames in ascending order (S1 += p; S2 = fmaf(p, p, S2), from zero) and the
 * slots are added in slot order, ((s0 + s1) + s2) + s3; the sums of a window's gulps are added in gulp order.  Every output is
 * one fixed sum that depends on the data and the configuration only: no atomics, bit-identical from run to run, for whole and
 * two-part gulps, whatever else runs on the GPU.  Exact on integer data while S2 stays below 2^24 (N <= 4).
 * Rejected at Initialize, before any device is touched: a non-positive size, nupchan outside the set, ntime % nupchan, W neither
 * dividing nor a multiple of F, nchan * ninput above 2^24.  Rejected at Run / Prime without a launch: null (out: where the gulp
 * completes a window) or misaligned pointers; RunParts / PrimeParts: parts that are not positive multiples of nupchan.
 * Without a context: XENG_STATUS_INVALID_STATE. */
int xengUpchanSpectraInitialize(int gpu, int ninput, int nchan, int ntime, int nupchan, int nframe_sum);
/* the live context's gulps per window (G, 1 when W | F), windows per gulp (F/W, 1 when F | W), and how many gulps of the window
 * in progress Run has taken (0 .. G-1; the next Run writes out_dev when it is G-1) */
int xengUpchanSpectraGetInfo(int *gulps_per_window, int *windows_per_gulp, int *pos);
/* enqueue only: one gulp, or one gulp in two spans (samples [0, ntime0) at in0_dev, [ntime0, ntime) at in1_dev).  out_dev is
 * written by a gulp that completes a window; with G > 1 it may be NULL on the others. */
int xengUpchanSpectraRun(const void *in_dev, void *out_dev);
int xengUpchanSpectraRunParts(const void *in0_dev, int ntime0, const void *in1_dev, void *out_dev);
/* The PFB front end of xengUpchanSetPfb for this context: the same definition, history (u8[(P-1)*N][nchan][ninput] on the
 * device, refreshed from each gulp's tail behind its launch), rules and checks (Initialize returns the context to ntap = 1
 * without coefficients). */
int xengUpchanSpectraSetPfb(int ntap, const float *coeffs);
/* enqueue only: the history from this gulp's tail (one part, or two as RunParts takes them), nothing summed and the window
 * position unchanged -- for a reader that waits for a window boundary; nothing to do without a history (ntap = 1) */
int xengUpchanSpectraPrime(const void *in_dev);
int xengUpchanSpectraPrimeParts(const void *in0_dev, int ntime0, const void *in1_dev);
/* drop the window in progress and invalidate the PFB history (host state only, nothing is launched) */
int xengUpchanSpectraReset(void);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengUpchanSpectraMark(unsigned long long *ticket);
int xengUpchanSpectraWait(unsigned long long ticket);
int xengUpchanSpectraTicketDone(unsigned long long ticket, int *done);
int xengUpchanSpectraSync(void);
int xengUpchanSpectraDestroy(void);

/* ---------------------------------------------------------------- Incoherent dedispersion of fine-channel power beams
 * BeamDedisperse (no reference counterpart: the reference has no dedisperser): a direct (brute-force) incoherent dedisperser
 * over a caller-supplied grid of DM trials, streaming across calls through a history ring on the device.  A context of its own,
 * independent of all others, whose kernels run on the beamformer's stream -- rings declared 'beam' cover them, and
 * xengBeamformSync waits for them too.  Two kernels per call (csrc/dedisp_kernels.h):
 *   in       f32[nwin_call][npair][nfine][4] = [XX, YY, Re XY*, Im XY*], the output span of xengUpchanSumBeamsRun or of
 *            xengUpchanInitializeDualPol unchanged: nfine = nchan*nupchan, q = c*N + j ascending in frequency, the centre of
 *            channel q at fine_sfreq + q*fine_bw_hz.  16-byte aligned; never written.  1 <= nwin_call <= nwin.
 *   products nprod = 1: I = XX + YY (one f32 add, at ingest); nprod = 4: the four words, each dedispersed by itself
 *   delays   s[d][q], int32[ndm][nfine] on the host, 0 <= s <= max_delay, in windows (xengDedispSetDelays; the library knows
 *            nothing of the dispersion constant).  S = max s; the back-delay is b[d][q] = S - s[d][q].
 *   weights  w[q], f32[nfine] on the host, finite; NULL or never set: all ones (xengDedispSetWeights).  A channel whose weight is
 *            exactly 0 is left out, not multiplied: a NaN or Inf in it never reaches an output.
 *   out      f32[nwin_call][npair][ndm][nprod], 16-byte aligned; nothing past it is written.  With n counting windows since the
 *            last reset (xengDedispReset, xengDedispSetDelays, Initialize):
 *              y[n][p][d] = sum_q w[q] * x[n - b[d][q]][p][q],   terms with n - b[d][q] < 0 count as zero
 *            All trials share one time axis: output n is the pulse that reached the top channel (delay 0) at window n - S; the
 *            first S outputs after a reset are partial sums.
 *   state    a device ring of L = max_delay + nwin windows, f32[npair][nfine][nprod][L] (time the fastest axis, window n at slot
 *            n mod L), holding I or the four words UNWEIGHTED: new weights apply to every later output, old windows included.
 * Numerics: fp32, no atomics; every output is one fixed-order sum.  The channels are cut into 4 segments of Q = ceil(nfine / 4)
 * consecutive channels, segment k = [k*Q, min((k+1)*Q, nfine)); a segment's partial sum P_k starts from +0 and takes its channels
 * in ascending q, one fmaf(w[q], x, sum) each (a term that counts as zero or is left out enters as fmaf(w[q], +0, sum)); the
 * output is ((P_0 + P_1) + P_2) + P_3.  The order depends on nfine alone: not on nwin_call, on how a run of windows is split
 * over calls, on the ring's wrap position, or on what else runs on the GPU -- bit-identical in all of these.  Exact on integer
 * data while every sum stays below 2^24.
 * Rejected at Initialize, before any device is touched: a non-positive size, nprod outside {1, 4}, max_delay < 0, a history
 * above XENG_DEDISP_MAX_HISTORY_BYTES, npair > 65535, ndm*nfine > 2^28, ndm*nwin > 2^30.  Rejected by the setters and Run without
 * a launch: a NULL (SetDelays, Run) or misaligned pointer, nwin_call outside 1..nwin, a negative delay or one above max_delay, a
 * non-finite weight; Run before SetDelays and every call without a context: XENG_STATUS_INVALID_STATE. */
#define XENG_DEDISP_MAX_HISTORY_BYTES (1LL << 32)
int xengDedispInitialize(int gpu, int npair, int nfine, int nwin, int ndm, int max_delay, int nprod);
/* Both setters wait for the context's work in flight (as xengUpchanSetPfb does) and upload from the host.  SetDelays clears the
 * history and the window count, because S moves the time axis; SetWeights clears neither. */
int xengDedispSetDelays(const int *delays);
int xengDedispSetWeights(const float *weights);
/* enqueue only: nwin_call windows in, nwin_call out */
int xengDedispRun(const void *in_dev, int nwin_call, void *out_dev);
/* host state only, nothing is launched: the next input counts as window 0 of an empty history */
int xengDedispReset(void);
/* S of the table in use (-1 before SetDelays) and the windows taken since the last reset */
int xengDedispGetInfo(int *max_delay_in_use, long long *nwindows_since_reset);
/* The history is allocated between two guard bands of 64 KiB: waits for the context's work, reads them back and reports
 * whether both still hold their pattern (*intact = 1) -- for tests and for chasing a stray write; not a per-call function. */
int xengDedispCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengDedispMark(unsigned long long *ticket);
int xengDedispWait(unsigned long long ticket);
int xengDedispTicketDone(unsigned long long ticket, int *done);
int xengDedispSync(void);
int xengDedispDestroy(void);

/* ---------------------------------------------------------------- Boxcar single-pulse search of the dedispersed beams
 * BeamPulseSearch (no reference counterpart: the reference has no detection stage): per series a running baseline, a bank of
 * boxcar matched filters of widths 1, 2, 4 ... 2^(nwidth-1) windows and the peak per call, streaming across calls with its state
 * on the device.  A context of its own, independent of all others, whose kernel runs on the beamformer's stream -- rings
 * declared 'beam' cover it, and xengBeamformSync waits for it too.  One kernel per call (csrc/pulse_kernels.h).
 *   in       f32[nwin_call][npair][ndm][nprod], the output span of xengDedispRun unchanged; 16-byte aligned; never written.
 *            1 <= nwin_call <= nwin.  A series is one (p, d).  nprod = 1: z[n] = in[n][p][d][0]; nprod = 4:
 *            z[n] = fl(in[n][p][d][0] + in[n][p][d][1]), I = XX + YY.  n counts windows since the last reset (xengPulseReset,
 *            Initialize).
 * Everything below is fp32 and fl() is one rounding to fp32; no product is contracted into a sum except where fmaf is written.
 *   baseline   Block k is the windows [k*nstat, (k+1)*nstat).  At its first window c_k = z[k*nstat] and a = q = +0.  Then for
 *            every window of the block in ascending n, the first included: delta = fl(z[n] - c_k), a = fl(a + delta),
 *            q = fmaf(delta, delta, q).  After its last window m_k = fl(a*r) with r = 1.0f/(float)nstat formed on the host, and
 *            v_k = fmaf(-m_k, m_k, fl(q*r)).  The block is VALID iff 0 < v_k < +inf; then g_k = 1/sqrt(v_k) (evaluated as
 *            fl(1.0f / fl(sqrt(v_k))) with correctly rounded fp32 sqrt and divide; deterministic, but the library's choice and not
 *            part of the word-for-word contract).  The pivot c_k keeps the one-pass variance well conditioned: a series of summed
 *            powers has mean/sigma of 55-100, and without a pivot fp32 loses three digits of sigma.
 *   series   A window n in a block k >= 1 whose block k-1 is valid has y[n] = fl(fl(z[n] - c_{k-1}) - m_{k-1}).  Every other
 *            window has no y.
 *   boxcars  Widths w = 2^iw, iw = 0..nwidth-1.  B_1[n] = y[n]; B_{2w}[n] = fl(B_w[n] + B_w[n-w]): a pairwise tree, the newer
 *            half first, so the order is a function of w alone.
 *   score    snr_w[n] = fl(fl(B_w[n] * g_{k-1}) * rho_iw), k the block of n and rho_iw = (float)2^(-iw/2) from the host.
 *            (n, iw) is SCORED iff n - w + 1 >= nstat, every window of the boxcar has a y, and the score is not NaN.
 *   out      [npair][ndm] records of four 32-bit words {f32 snr, i32 n_call, i32 iw, f32 B}, 16-byte aligned: of the scored
 *            (n, iw) with n in this call the one with the largest snr, among equal scores the smallest n, then the smallest iw;
 *            n_call is the window's index within the call and B = B_w[n].  A series with nothing scored in the call gets
 *            {+0.0f, -1, -1, +0.0f}.  Each record is one 16-byte store; nothing outside npair*ndm*16 bytes is written.
 *   state    per series c, m, v, g of the last complete block and c, a, q of the running one, and a ring of the last
 *            2^(nwidth-1) - 1 + nwin values of y (series the fastest axis), all between two guard bands of 64 KiB.
 * A run gives the same records bit for bit however it is split over calls (merge the calls' records: strictly greater replaces,
 * in call order), whatever else runs on the GPU.  Exact on integer data while the sums stay below 2^24.
 * Rejected at Initialize, before any device is touched: a non-positive size, nprod outside {1, 4}, nwidth outside 1..8, nstat
 * outside 2..2^20, 2^(nwidth-1) > nstat, npair*ndm > 2^24, 2^(nwidth-1) - 1 + 2*nwin > 256 (what one work-group's LDS holds).
 * Rejected by Run without a launch: a NULL or misaligned pointer, nwin_call outside 1..nwin.  Every call without a context, and
 * GetBaseline before a block has completed: XENG_STATUS_INVALID_STATE. */
int xengPulseInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int nwidth, int nstat);
/* enqueue only: nwin_call windows in, one record per series out */
int xengPulseRun(const void *in_dev, int nwin_call, void *out_dev);
/* host state only, nothing is launched and nothing cleared: the next input counts as window 0.  The kernel decides by index
 * what lies before window 0 or before nstat and never looks at what the buffers still hold. */
int xengPulseReset(void);
/* windows taken since the last reset, and how many baseline blocks of them are complete */
int xengPulseGetInfo(long long *nwindows_since_reset, long long *nblocks_complete);
/* c, m and v of the last complete block into host f32[npair][ndm] each; waits for the context's work in flight */
int xengPulseGetBaseline(float *c, float *m, float *var);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengPulseCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengPulseMark(unsigned long long *ticket);
int xengPulseWait(unsigned long long ticket);
int xengPulseTicketDone(unsigned long long ticket, int *done);
int xengPulseSync(void);
int xengPulseDestroy(void);

/* ---------------------------------------------------------------- Phase-folded profiles of the fine-channel power beams
 * BeamFold (no reference counterpart: the reference ships its power beams to external pulsar backends): every window of every
 * pair, fine channel and product is added into the bin of a pulse profile that an integer phase oscillator names; a dump rotates
 * the channels against each other (dispersion, inside a fold, is a rotation of each channel's profile), weights and sums them.
 * A context of its own, independent of all others, whose kernels run on the beamformer's stream -- rings declared 'beam' cover
 * them, and xengBeamformSync waits for them too.  One kernel per call (csrc/fold_kernels.h).  The library knows nothing of
 * pulsars, of time or of the dispersion constant: the caller supplies oscillators and rotations as integers.
 *   in       f32[nwin_call][npair][nfine][4] = [XX, YY, Re XY*, Im XY*], as xengDedispRun takes it; 16-byte aligned; never
 *            written.  1 <= nwin_call <= nwin.
 *   products nprod = 1 folds I = fl(XX + YY); nprod = 4 folds the four words, each by itself.
 *   phase    n counts windows since the last reset (xengFoldReset, Initialize).  xengFoldSetPhase(phi0, dphi, ddphi, active, n_ref)
 *            takes host arrays of npair entries (uint64 phi0, uint64 dphi, int64 ddphi, uint8 active) and 0 <= n_ref <= the
 *            windows taken so far.  With m = n - n_ref the phase of pair p at window n, in turns * 2^64 and in wrapping 64-bit
 *            arithmetic, is
 *              Phi_p(n) = phi0 + dphi*m + ddphi*(m(m-1)/2)          (m(m-1)/2 formed exactly; Run refuses a call whose last m
 *                                                                     would reach 2^31)
 *              bin_p(n) = ((Phi_p(n) >> 32) * nbin) >> 32
 *            A pair with active = 0 is left out.  A new SetPhase acts from the next Run on and clears nothing: a caller
 *            re-tunes at a sub-integration boundary with n_ref = the current count.
 *   state    prof[p][b][q][k], f32[npair][nbin][nfine][nprod], +0 after Initialize, Reset or a clearing dump.  xengFoldRun, for
 *            every window of the call in ascending n:   prof[p][bin_p(n)][q][k] = fl(prof[p][bin_p(n)][q][k] + x[n][p][q][k]).
 *            Each word is ONE strictly sequential chain of fp32 adds over the windows that fall in its bin: no atomics, no
 *            partial sums added later.  So the result does not depend on nwin_call, on how a run is split over calls, or on
 *            what else runs on the GPU; a NaN in one channel never reaches another channel; the result is exact on integer
 *            data below 2^24; and any float32 restatement that adds in window order reproduces it bit for bit.
 *   hits     hits[p][b]: the windows folded into bin b of pair p since the last clear -- exact integers from the phase model,
 *            kept on the host side of the library (nothing on the device is needed to count them).
 *   dump     xengFoldDump(out_dev, hits_host, nfscr, normalise, clear): out is f32[npair][nprod][nfine/nfscr][nbin], the bin the
 *            fastest axis, 16-byte aligned; nothing past it is written.  nfscr divides nfine (1: the full cube; nfine: the
 *            dedispersed profile).  With rotations rot[p][q] in [0, nbin) (xengFoldSetRotations) and weights w[q]
 *            (xengFoldSetWeights):
 *              out[p][k][g][b] = sum over q = g*nfscr .. (g+1)*nfscr - 1, ascending, of w[q] * prof[p][(b + rot[p][q]) mod nbin][q][k]
 *            one chain from +0 of fmaf(w[q], x, sum).  A channel of weight exactly 0 is left out (a select, not a multiply:
 *            a NaN there never arrives).  normalise = 1 divides each term's prof word by (float)hits[p][(b + rot[p][q]) mod nbin]
 *            (correctly rounded fp32 division) before the fmaf; a bin with 0 hits then contributes +0.  An inactive pair's
 *            plane is +0.  hits_host, uint32[npair][nbin] on the host, unrotated, may be NULL; it is filled on return.
 *            clear = 1 zeroes the profile and the hits as part of the same launch: each profile word is read by exactly one
 *            thread, which then writes it.  A dump may wait for the context's work in flight the way the setters do (a
 *            normalising one does, to upload the hits): it runs once per sub-integration.
 * Rejected at Initialize, before any device is touched: a non-positive size, nprod outside {1, 4}, nbin > 65536, npair > 65535,
 * a profile above XENG_FOLD_MAX_PROFILE_BYTES (the live shape, 16 x 3072 x 4 at 1024 bins, is 805 MB).  Rejected by the setters,
 * Run and Dump without a launch: a NULL (Run, Dump's output, SetPhase) or misaligned pointer, nwin_call outside 1..nwin, a
 * rotation outside [0, nbin), a non-finite weight, nfscr not dividing nfine, n_ref out of range.  Run before SetPhase, Dump
 * before SetRotations and every call without a context: XENG_STATUS_INVALID_STATE. */
#define XENG_FOLD_MAX_PROFILE_BYTES (1LL << 32)
int xengFoldInitialize(int gpu, int npair, int nfine, int nwin, int nbin, int nprod);
/* The three setters wait for the context's work in flight (as xengDedispSetWeights does) and upload from the host; none of them
 * clears anything.  SetRotations: int32[npair][nfine], NULL means all zeros.  SetWeights: f32[nfine], finite; NULL or never
 * set means all ones.  Rotations and weights act on dumps only. */
int xengFoldSetPhase(const unsigned long long *phi0, const unsigned long long *dphi, const long long *ddphi, const unsigned char *active,
                     long long n_ref);
int xengFoldSetRotations(const int *rot);
int xengFoldSetWeights(const float *weights);
/* enqueue only: nwin_call windows folded into the profile */
int xengFoldRun(const void *in_dev, int nwin_call);
int xengFoldDump(void *out_dev, unsigned int *hits_host, int nfscr, int normalise, int clear);
/* enqueue only: the count back to 0, the hits cleared, the profile cleared by one clearing launch on the stream.  The
 * oscillators stay and their reference moves with the count: the next window has m = 0. */
int xengFoldReset(void);
/* windows taken since the last reset, and windows folded since the last clear (Reset, a clearing dump, Initialize) */
int xengFoldGetInfo(long long *nwindows_since_reset, long long *nwindows_folded);
/* The profile is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengFoldCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengFoldMark(unsigned long long *ticket);
int xengFoldWait(unsigned long long ticket);
int xengFoldTicketDone(unsigned long long ticket, int *done);
int xengFoldSync(void);
int xengFoldDestroy(void);

/* ---------------------------------------------------------------- FFT periodicity search of the dedispersed beams
 * BeamPeriodSearch (no reference counterpart: the reference has no detection stage): per series a long real FFT per segment of
 * NT windows, the power spectrum whitened by block means, nstack such spectra stacked incoherently, harmonic sums of the stack and
 * one peak record per series and harmonic level.  A context of its own, independent of all others, whose kernels run on the
 * beamformer's stream -- rings declared 'beam' cover them, and xengBeamformSync waits for them too.  An ingest kernel per call
 * and a spectrum kernel per completed segment (csrc/period_kernels.h).
 *   in       f32[nwin_call][npair][ndm][nprod], the output span of xengDedispRun unchanged; 16-byte aligned; never written.
 *            1 <= nwin_call <= nwin <= NT, so that a call completes at most one segment.  A series is one (p, d), nser =
 *            npair*ndm.  nprod = 1: z[n] = in[n][p][d][0]; nprod = 4: z[n] = fl(in[n][p][d][0] + in[n][p][d][1]), I = XX + YY.
 *            n counts windows since the last reset (xengPeriodReset, Initialize).
 *   sizes    NT = nt, the segment length: a power of two, 2^8 <= NT <= 2^14 (the FFT's NT/2 complex points are at most 64 KiB of
 *            LDS).  nstack >= 1 segments per stack.  nlevel = 1..5 harmonic levels, h = 1, 2, 4, 8, 16.  nwhite = B, the
 *            whitening block: a power of two, 8 <= B <= NT/2.  kmin, the lowest fundamental bin: 1 <= kmin < NT/32.
 *   segment  Segment s of a stack is the NT windows [(s0 + s)*NT, (s0 + s + 1)*NT).  The call that brings its last window
 *            transforms it, per series:
 *              1. x = z - mean(z).  The summation order is the library's: everything up to A is held to a tolerance.
 *              2. the NT-point real DFT  X[k] = sum_n x[n] * exp(-2 pi i n k / NT).
 *              3. P[k] = |X[k]|^2 for 1 <= k < NT/2.  DC and Nyquist are dropped.
 *              4. whitening.  Block b is the bins [b*B, (b+1)*B).  mu_b is the mean of P over the block's bins with k >= 1 and
 *                 keep[k] != 0.  If the block has no such bin, or mu_b is not finite and positive, S[k] = 1.0f for the whole
 *                 block (a dead series, all zeros, comes out as pure expectation); otherwise S[k] = P[k] / mu_b.
 *              5. the mask: a zapped bin (keep[k] = 0) gets S[k] = 1.0f; S[0] = +0.
 *              6. a segment whose mean(z) is not finite -- it held a NaN or an Inf sample -- has no spectrum: S[k] = NaN for
 *                 every k >= 1, zapped bins included, so that the series stays NaN in A to the end of its stack.
 *   stack    A[k] = ((S_1 + S_2) + S_3) + ... in segment order, fp32, one owner per word and no atomics.  The first segment of
 *            a stack STORES, so nothing is ever cleared.  A is f32[npair][ndm][NT/2] on the device.
 *   sums     When segment nstack of a stack completes: for h = 2^l, l < nlevel, and h*kmin <= k < NT/2
 *              H_h[k] = sum_{j=1..h} A[(j*k + h/2) div h]
 *            j ascending, plain fp32 adds starting from A of j = 1, no contraction.  k indexes the TOP harmonic: the
 *            fundamental is k/h bins, k / (h * NT * tsamp) Hz.  The index arithmetic is integer: which words are summed is
 *            exact, and any float32 restatement that adds in this order reproduces H bit for bit from the same A.
 *   out      [npair][ndm][nlevel] records of two 32-bit words {f32 H, i32 k}, each one 8-byte store, out_dev 16-byte aligned;
 *            nothing past npair*ndm*nlevel*8 bytes is written.  The record is the largest H_h[k], among equal sums the smallest
 *            k.  A NaN is never a maximum; if nothing qualifies the record is {+0.0f, -1}.  A series that held a non-finite
 *            sample anywhere in the stack therefore reads {+0.0f, -1} at every level, and disturbs no neighbour.
 *   state    between two guard bands of 64 KiB: the time buffer f32[nser][NT] (time the fastest axis, window n at slot
 *            n mod NT), A, the mask with the counts of its blocks, and the twiddle tables exp(-2 pi i k / NT) (float64 on the
 *            host, rounded once).  xengPeriodReset moves only the host's counts: the partial segment and the partial stack are
 *            dropped by index, and nothing is cleared.
 * A and the records are a fixed function of the series and the mask: bit-identical however a run is split over calls, whatever
 * nwin_call, after a Reset as in a fresh context, and whatever else runs on the GPU.  The sums are exact on integer-valued A
 * below 2^24.
 * Rejected at Initialize, before any device is touched: a non-positive size, nprod outside {1, 4}, nt not a power of two in
 * 2^8..2^14, nstack < 1, nlevel outside 1..5, nwhite not a power of two in 8..nt/2, kmin outside 1..nt/32 - 1, nwin > nt,
 * npair*ndm > 2^24, a state above XENG_PERIOD_MAX_STATE_BYTES.  Rejected by Run without a launch: a NULL input or result, a
 * misaligned pointer, nwin_call outside 1..nwin, a NULL output on the call that completes a stack.  Every call without a context,
 * and GetSpectrum before a segment has completed: XENG_STATUS_INVALID_STATE. */
#define XENG_PERIOD_MAX_STATE_BYTES (1LL << 32)
int xengPeriodInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int nt, int nstack, int nlevel, int nwhite, int kmin);
/* keep: u8[nt/2] on the host, 0 = zapped; NULL: all kept (as after Initialize).  Waits for the context's work in flight (as
 * xengDedispSetWeights does); holds from the next segment to complete. */
int xengPeriodSetMask(const unsigned char *keep);
/* enqueue only.  out_dev is written only by a call that completes a stack (*completed = 1); the host's window count decides that
 * before anything is enqueued.  Such a call with out_dev NULL is INVALID_ARGUMENT and enqueues nothing; on every other call
 * out_dev may be NULL and is not touched. */
int xengPeriodRun(const void *in_dev, int nwin_call, void *out_dev, int *completed);
/* host state only, nothing is launched and nothing cleared: the next input counts as window 0 of segment 0 of a new stack */
int xengPeriodReset(void);
/* windows taken since the last reset, complete segments of the stack in progress, stacks completed since the last reset */
int xengPeriodGetInfo(long long *nwindows_since_reset, int *nseg_in_stack, long long *nstacks_complete);
/* waits for the context's work in flight; the stack as it stands into host f32[npair][ndm][nt/2] and the segments it holds
 * (nstack after the call that completed a stack): the diagnostic plot, and what the exact test of the records reads */
int xengPeriodGetSpectrum(float *A_host, int *nseg);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengPeriodCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengPeriodMark(unsigned long long *ticket);
int xengPeriodWait(unsigned long long ticket);
int xengPeriodTicketDone(unsigned long long ticket, int *done);
int xengPeriodSync(void);
int xengPeriodDestroy(void);

/* ---------------------------------------------------------------- FFT periodicity search with long segments
 * BeamPeriodSearchLong (no reference counterpart): xengPeriod* for segments of 2^15 to 2^20 windows, which no work-group's LDS
 * holds -- the transform goes through a scratch buffer in HBM as a four-step FFT -- and with one peak record per series, harmonic
 * level and BAND of fundamental frequency, since one peak among half a million bins is too few.  A context of its own,
 * independent of all others (xengPeriod* included), whose kernels run on the beamformer's stream -- rings declared 'beam' cover
 * them, and xengBeamformSync waits for them too.  An ingest kernel per call; per completed segment a mean kernel and, per batch
 * of series, two FFT passes, an untangle and a whitening kernel; per completed stack and batch a sums and a reduce kernel
 * (csrc/plong_kernels.h).
 *   in       f32[nwin_call][npair][ndm][nprod], the output span of xengDedispRun unchanged; 16-byte aligned; never written.
 *            1 <= nwin_call <= nwin <= NT, so that a call completes at most one segment.  A series is one (p, d), nser =
 *            npair*ndm.  nprod = 1: z[n] = in[n][p][d][0]; nprod = 4: z[n] = fl(in[n][p][d][0] + in[n][p][d][1]), I = XX + YY.
 *            n counts windows since the last reset (xengPlongReset, Initialize).
 *   sizes    NT = nt, the segment length: a power of two, 2^15 <= NT <= 2^20 (2^14 and below are xengPeriod*'s).  nstack >= 1
 *            segments per stack.  nlevel = 1..5 harmonic levels, h = 1, 2, 4, 8, 16.  nwhite = B, the whitening block: a power
 *            of two, 8 <= B <= 2^13, so that a block never spans two work-groups' runs of bins.
 *   segment  Segment s of a stack is the NT windows [(s0 + s)*NT, (s0 + s + 1)*NT).  The call that brings its last window
 *            transforms it, per series:
 *              1. x = z - mean(z).  The mean is formed when the segment completes, in a fixed tree over the whole segment: it is
 *                 a function of the segment and not of how the calls cut it.  The summation order is the library's: everything
 *                 up to A is held to a tolerance.
 *              2. the NT-point real DFT  X[k] = sum_n x[n] * exp(-2 pi i n k / NT).
 *              3. P[k] = |X[k]|^2 for 1 <= k < NT/2.  DC and Nyquist are dropped.
 *              4. whitening.  Block b is the bins [b*B, (b+1)*B).  mu_b is the mean of P over the block's bins with k >= 1 and
 *                 keep[k] != 0.  If the block has no such bin, or mu_b is not finite and positive, S[k] = 1.0f for the whole
 *                 block (a dead series, all zeros, comes out as pure expectation); otherwise S[k] = P[k] / mu_b.
 *              5. the mask: a zapped bin (keep[k] = 0) gets S[k] = 1.0f; S[0] = +0.
 *              6. a segment whose mean(z) is not finite -- it held a NaN or an Inf sample -- has no spectrum: S[k] = NaN for
 *                 every k >= 1, zapped bins included, so that the series stays NaN in A to the end of its stack.
 *   stack    A[k] = ((S_1 + S_2) + S_3) + ... in segment order, fp32, one owner per word and no atomics.  The first segment of
 *            a stack STORES, so nothing is ever cleared.  A is f32[npair][ndm][NT/2] on the device, natural k order.
 *   bands    kedge[nband + 1], 1 <= nband <= 32: integers with 1 <= kedge[0] < kedge[1] < ... < kedge[nband] <= NT/2 and
 *            kedge[0] < NT/32.  Band b of level h = 2^l is the set of top-harmonic bins h*kedge[b] <= k < min(h*kedge[b+1],
 *            NT/2): it holds the fundamentals from kedge[b] to kedge[b+1].  At a high level an upper band may be empty.
 *   sums     When segment nstack of a stack completes: for h = 2^l, l < nlevel,
 *              H_h[k] = sum_{j=1..h} A[(j*k + h/2) div h]
 *            j ascending, plain fp32 adds starting from A of j = 1, no contraction.  k indexes the TOP harmonic: the
 *            fundamental is k/h bins, k / (h * NT * tsamp) Hz.  The index arithmetic is integer: which words are summed is
 *            exact, and any float32 restatement that adds in this order reproduces H bit for bit from the same A.  With
 *            nband = 1 and kedge = {kmin, NT/2} this is xengPeriod*'s rule.
 *   out      [npair][ndm][nlevel][nband] records of two 32-bit words {f32 H, i32 k}, each one 8-byte store, out_dev 16-byte
 *            aligned; nothing past npair*ndm*nlevel*nband*8 bytes is written.  A record is the largest H_h[k] of its band, among
 *            equal sums the smallest k.  A NaN is never a maximum; an empty or all-NaN band reads {+0.0f, -1}.  A series that
 *            held a non-finite sample anywhere in the stack therefore reads {+0.0f, -1} everywhere, and disturbs no neighbour.
 *   state    between two guard bands of 64 KiB: the time buffer f32[nser][NT] (time the fastest axis, window n at slot
 *            n mod NT); A; per series the mean and validity word of the last segment; one scratch for a batch of SB <= nser
 *            series -- cf32[SB][NT/2] between the FFT passes, the power spectrum f32[SB][NT/2] and the partial records of the
 *            sums -- with SB chosen at Initialize so that this scratch stays at or below 2 GiB, the per-segment launches looping
 *            over the batches; the mask with the counts of its blocks, the edges, and the twiddle tables (float64 on the host,
 *            rounded once).  4096 series at 2^20 are 24 GiB plus the scratch; 16384 series fit up to 2^18.  xengPlongReset moves
 *            only the host's counts: the partial segment and the partial stack are dropped by index, and nothing is cleared.
 * A and the records are a fixed function of the series, the mask and the edges: bit-identical however a run is split over calls,
 * whatever nwin_call, after a Reset as in a fresh context, whatever else runs on the GPU, and whatever SB is.  The records are
 * exact given A, and the sums exact on integer-valued A below 2^24.
 * Rejected at Initialize, before any device is touched: a non-positive size, nprod outside {1, 4}, nt not a power of two in
 * 2^15..2^20, nstack < 1, nlevel outside 1..5, nwhite not a power of two in 8..2^13, nband outside 1..32, NULL edges, edges not
 * strictly ascending or outside 1..nt/2, kedge[0] >= nt/32, nwin > nt, npair*ndm > 2^24, a state above
 * XENG_PLONG_MAX_STATE_BYTES; once the device is known, an LDS need above what a work-group may take (64 KiB at most).  Rejected
 * by Run without a launch: a NULL input or result, a misaligned pointer, nwin_call outside 1..nwin, a NULL output on the call
 * that completes a stack.  Every call without a context, and GetSpectrum before a segment has completed:
 * XENG_STATUS_INVALID_STATE. */
#define XENG_PLONG_MAX_STATE_BYTES (1LL << 36)
int xengPlongInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int nt, int nstack, int nlevel, int nwhite, int nband, const int *kedge);
/* keep: u8[nt/2] on the host, 0 = zapped; NULL: all kept (as after Initialize).  Waits for the context's work in flight; holds
 * from the next segment to complete. */
int xengPlongSetMask(const unsigned char *keep);
/* enqueue only.  out_dev is written only by a call that completes a stack (*completed = 1); the host's window count decides that
 * before anything is enqueued.  Such a call with out_dev NULL is INVALID_ARGUMENT and enqueues nothing; on every other call
 * out_dev may be NULL and is not touched. */
int xengPlongRun(const void *in_dev, int nwin_call, void *out_dev, int *completed);
/* host state only, nothing is launched and nothing cleared: the next input counts as window 0 of segment 0 of a new stack */
int xengPlongReset(void);
/* windows taken since the last reset, complete segments of the stack in progress, stacks completed since the last reset */
int xengPlongGetInfo(long long *nwindows_since_reset, int *nseg_in_stack, long long *nstacks_complete);
/* waits for the context's work in flight; series [series0, series0 + nser) of the stack as it stands into host f32[nser][nt/2],
 * natural k order, and the segments it holds (nstack after the call that completed a stack).  A range outside [0, npair*ndm) is
 * INVALID_ARGUMENT. */
int xengPlongGetSpectrum(int series0, int nser, float *A_host, int *nseg);
/* The series per batch: SB as Initialize chose it (nser_batch_max, what the scratch holds) and as the launches take it.
 * SetBatch lowers it to 1 <= nser_batch <= nser_batch_max from the next call on (0: back to nser_batch_max); host state only.
 * Results do not depend on it: it is there for the test of exactly that. */
int xengPlongSetBatch(int nser_batch);
int xengPlongGetBatch(int *nser_batch, int *nser_batch_max);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengPlongCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengPlongMark(unsigned long long *ticket);
int xengPlongWait(unsigned long long ticket);
int xengPlongTicketDone(unsigned long long ticket, int *done);
int xengPlongSync(void);
int xengPlongDestroy(void);

/* ---------------------------------------------------------------- Acceleration search of the long-segment spectra
 * BeamAccelSearch (no reference counterpart): the search of xengPlong* repeated per trial acceleration.  Over a segment of minutes
 * a pulsar in a binary drifts across z = a T^2 f / c Fourier bins and its harmonics smear; trial a reads the segment through a
 * quadratic index map that undoes a constant acceleration (time-domain resampling, nearest sample) and searches the result as
 * xengPlong* searches a segment.  A context of its own, independent of all others (xengPlong* included), whose kernels run on the
 * beamformer's stream.  An ingest kernel per call; per completed segment, per batch of series and per trial a gathered mean and
 * columns pass and xengPlong*'s rows pass, untangle, whitening, sums and reduce; then one kernel that takes the best over the
 * trials (csrc/accel_kernels.h).
 *   in       exactly xengPlong*'s: f32[nwin_call][npair][ndm][nprod], 16-byte aligned, never written; nprod 1 or 4;
 *            1 <= nwin_call <= nwin <= NT; NT = nt a power of two, 2^15 <= NT <= 2^20; the time buffer f32[nser][NT].  There is
 *            no stack: every completed segment yields one plane.
 *   trials   1 <= ntrial <= 256, alpha f64[ntrial] given at Initialize.  Trial a searches the series
 *              z_a[n] = z[n + s_a(n)],   s_a(n) = (long long) rint(alpha[a] * (double)(n * (n - NT))),   n = 0 .. NT-1
 *            the integer product formed exactly (it is below 2^40 in size, exact as a float64), ONE float64 multiply, rounding to
 *            nearest even.  Every term is an IEEE operation: any float64 restatement gives the same indices.  s_a(0) = 0 and
 *            s_a(NT-1) = 0 (|alpha| (NT-1) < 0.5): the segment's ends stay where they are and its middle moves by alpha NT^2 / 4
 *            windows.  Initialize refuses a non-finite alpha and |alpha| * NT > 0.5; under that limit the map is non-decreasing
 *            and stays inside [0, NT-1], so there is no clamp.  (alpha = a tsamp / 2c for an acceleration a along the line of
 *            sight: the limit is |a| <= c / T, far beyond any binary.)  izero is the first trial with alpha == 0.0, -1 without.
 *   trial a  computes everything xengPlong* computes for one segment with nstack = 1, applied to z_a: the segment mean in that
 *            engine's tree -- over z_a, not over z -- the transform, P, the block-mean whitening under the mask, and the banded
 *            harmonic sums (nlevel <= 5, nband <= 32, kedge as there).  The records of trial a are BIT FOR BIT the records
 *            xengPlongRun writes when fed z_a as its input, whatever the batch size and however the calls cut the segment.
 *   records  {f32 H, i32 k}[ntrial][npair*ndm][nlevel][nband] of the segment that completed last are kept in the state:
 *            xengAccelGetTrialRecords.
 *   out      written only by the call that completes a segment (*completed = 1): [npair][ndm][nlevel][nband] records of four
 *            32-bit words {f32 H, i32 k, i32 ia, f32 H0}, each one 16-byte store; nothing past npair*ndm*nlevel*nband*16 bytes
 *            is written.  (H, k, ia) is the best over the trials taken in ascending order: the larger H, then the smaller ia,
 *            then (within a trial already) the smaller k.  A NaN never enters.  A record that is empty in every trial reads
 *            {+0, -1, -1, H0}.  H0 is the H of trial izero for that record: what the unaccelerated search finds; +0 when
 *            izero < 0 or that record is empty.
 *   state    between two guard bands of 64 KiB: the time buffer, the trial records, one scratch for a batch of SB <= nser series
 *            (cf32[SB][NT/2] between the passes, the power spectrum and the whitened spectrum f32[SB][NT/2] each, the partial
 *            records of the sums, mean and validity of SB series), SB chosen at Initialize so that the scratch stays at or below
 *            2 GiB and SB <= 32768; the mask with its block counts, the edges and the twiddle tables.  Nothing of size
 *            [ntrial][NT] exists: the resampled series is never stored.  xengAccelReset moves only the host's counts.
 * Rejected at Initialize, before any device is touched: what xengPlongInitialize rejects (it has no nstack), ntrial outside
 * 1..256, a NULL or non-finite alpha, |alpha| * nt > 0.5, a state above XENG_ACCEL_MAX_STATE_BYTES; once the device is known, an
 * LDS need above what a work-group may take.  Rejected by Run without a launch: a NULL input or result, a misaligned pointer,
 * nwin_call outside 1..nwin, a NULL output on the call that completes a segment.  Every call without a context, and
 * GetTrialRecords before a segment has completed: XENG_STATUS_INVALID_STATE. */
#define XENG_ACCEL_MAX_STATE_BYTES (1LL << 36)
int xengAccelInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int nt, int nlevel, int nwhite, int nband, const int *kedge, int ntrial,
                        const double *alpha);
/* keep: u8[nt/2] on the host, 0 = zapped; NULL: all kept.  Waits for the context's work in flight; holds from the next segment. */
int xengAccelSetMask(const unsigned char *keep);
/* enqueue only.  out_dev is written only by a call that completes a segment (*completed = 1); such a call with out_dev NULL is
 * INVALID_ARGUMENT and enqueues nothing; on every other call out_dev may be NULL and is not touched. */
int xengAccelRun(const void *in_dev, int nwin_call, void *out_dev, int *completed);
/* host state only: the next input counts as window 0 of a new segment */
int xengAccelReset(void);
/* windows taken and segments completed since the last reset */
int xengAccelGetInfo(long long *nwindows_since_reset, long long *nsegments_complete);
/* waits for the context's work in flight; the trial records of series [series0, series0 + nser) of the segment that completed
 * last into host {f32 H, i32 k}[ntrial][nser][nlevel][nband].  A range outside [0, npair*ndm) is INVALID_ARGUMENT. */
int xengAccelGetTrialRecords(int series0, int nser, void *records_host);
/* the series per batch, as xengPlongSetBatch / GetBatch: results do not depend on it */
int xengAccelSetBatch(int nser_batch);
int xengAccelGetBatch(int *nser_batch, int *nser_batch_max);
int xengAccelCheckGuards(int *intact);
int xengAccelMark(unsigned long long *ticket);
int xengAccelWait(unsigned long long ticket);
int xengAccelTicketDone(unsigned long long ticket, int *done);
int xengAccelSync(void);
int xengAccelDestroy(void);

/* ---------------------------------------------------------------- Fast-folding search of the dedispersed beams
 * BeamFfaSearch (no reference counterpart: the reference has no detection stage): the fast folding algorithm (Staelin 1969) for
 * the long periods and small duty cycles the FFT search above is blind to.  Per series a segment of NT downsampled samples is
 * folded at every integer base period and at the fractional periods between, in octaves of the time resolution; a circular boxcar
 * matched filter runs over every folded profile; one peak record per series, octave and width comes out.  A context of its own,
 * independent of all others, whose kernels run on the beamformer's stream -- rings declared 'beam' cover them, and
 * xengBeamformSync waits for them too.  An ingest kernel per call; per completed segment a prepare kernel, a fold kernel per
 * octave and a reduce kernel (csrc/ffa_kernels.h).
 * Everything below is fp32 and fl() is one rounding to fp32; no product is contracted into a sum except where fmaf is written.
 *   in       f32[nwin_call][npair][ndm][nprod], the output span of xengDedispRun unchanged; 16-byte aligned; never written.
 *            1 <= nwin_call <= nwin.  A series is one (p, d), nser = npair*ndm.  z[n] as xengPeriodRun takes it: nprod = 1 the
 *            word, nprod = 4 fl(XX + YY).  n counts windows since the last reset (xengFfaReset, Initialize).
 *   downsample  u_0[k] = ((z[k*nds] + z[k*nds+1]) + ...) + z[k*nds+nds-1], one sequential chain of fp32 adds over nds windows,
 *            1 <= nds <= XENG_FFA_MAX_NDS.  The running sum of a sample whose windows a call cuts is kept per series on the
 *            device and taken up by the next call: a sample may straddle calls.
 *   segment  NT = nt samples of u_0, 2^8 <= NT <= 2^14, a multiple of 2^(noct-1) and not necessarily a power of two.
 *            nwin <= NT*nds, so that a call completes at most one segment.  Window n goes to slot (n div nds) mod NT of a time
 *            buffer f32[nser][NT], filled by index.
 *   octaves  o = 0 .. noct-1, 1 <= noct <= 6: u_o[k] = fl(u_{o-1}[2k] + u_{o-1}[2k+1]), of length N_o = NT >> o.
 *   statistics  per (series, octave), the pivoted one-pass form of xengPulse*, the pivot c = u_o[0]: a = sum of fl(u_o[k] - c),
 *            q = sum of its squares, m = fl(a*r), v = fmaf(-m, m, fl(q*r)) with r = (float)(1/N_o) from the host,
 *            g = fl(1 / fl(sqrt(v))).  The summation order of a and q is the library's: they are held to a tolerance.  The
 *            (series, octave) is VALID iff m is finite and 0 < v < +inf.  x_o[k] = fl(fl(u_o[k] - c) - m).
 *   fold     for every integer base period p, pmin <= p <= pmax, 16 <= pmin <= pmax, 2*pmax <= N_{noct-1}: M is the largest
 *            power of two with M*p <= N_o (M >= 2).  Row r is x_o[r*p .. r*p+p); samples past M*p are not read.  Stages
 *            L = 2, 4 .. M: in every block of L rows, A its first L/2 rows and B its last, for i < L and j < p
 *              out[i][j] = fl(A[i>>1][j] + B[i>>1][(j + ((i+1)>>1)) mod p])
 *            After the last stage profile i of M is the fold at a period of p + i/(M-1) samples.  Every word is one add of two
 *            fixed words: the bits do not depend on the schedule.
 *   boxcars  circular, widths w = 2^iw, iw < nwidth, 1 <= nwidth <= 8, 2^(nwidth-1) <= pmin/2: B_1 = the profile,
 *            B_{2w}[j] = fl(B_w[j] + B_w[(j+w) mod p]).
 *   score    S = fl(fl(B_w[j] * g) * rho), rho = (float)(1/sqrt(w*M)) from a host table indexed [iw][log2 M].
 *   out      [npair][ndm][noct][nwidth] records {f32 snr, i32 p, i32 i, i32 j}, each one 16-byte store, out_dev 16-byte
 *            aligned, written only by the call that completes a segment (*completed = 1); nothing past
 *            npair*ndm*noct*nwidth*16 bytes is written.  The record is the largest S over (p, i, j); among equals the
 *            smallest p, then i, then j.  A NaN is never a maximum.  An invalid (series, octave) reads {+0.0f, -1, -1, -1} at
 *            every width and disturbs no neighbour.
 *   state    between two guard bands of 64 KiB: the time buffer, the carried partial sums, x_o of every octave (fewer than
 *            2*NT words a series), the statistics {c, m, v, g}, the score table and one record per (series, octave, base period,
 *            width).  xengFfaReset moves only the host's counts: the partial segment and the partial sample are dropped by
 *            index, and nothing is cleared.
 * The records are a fixed function of the segment and of {c, m, g}: bit-identical however a run is split over calls, whatever
 * nwin_call (one that cuts a downsample group included), after a Reset as in a fresh context, and whatever else runs on the GPU.
 * Rejected at Initialize, before any device is touched: every size outside the ranges above, nprod outside {1, 4},
 * npair*ndm > 2^24, a state above XENG_FFA_MAX_STATE_BYTES.  Rejected by Run without a launch: a NULL input or result, a
 * misaligned pointer, nwin_call outside 1..nwin, a NULL output on the call that completes a segment.  Every call without a
 * context, and GetStats before a segment has completed: XENG_STATUS_INVALID_STATE.
 * Not built: general M (the head / tail FFA; up to half a segment is unread where N_o/p is just under a power of two), red-noise
 * detrending, more than one peak per (series, octave, width), segments above 2^14 samples. */
#define XENG_FFA_MAX_STATE_BYTES (1LL << 32)
#define XENG_FFA_MAX_NDS 65536
int xengFfaInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int nds, int nt, int noct, int pmin, int pmax, int nwidth);
/* enqueue only.  out_dev is written only by a call that completes a segment (*completed = 1); the host's window count decides
 * that before anything is enqueued.  Such a call with out_dev NULL is INVALID_ARGUMENT and enqueues nothing; on every other call
 * out_dev may be NULL and is not touched. */
int xengFfaRun(const void *in_dev, int nwin_call, void *out_dev, int *completed);
/* host state only, nothing is launched and nothing cleared: the next input counts as window 0 of a new segment */
int xengFfaReset(void);
/* windows taken and segments completed since the last reset */
int xengFfaGetInfo(long long *nwindows_since_reset, long long *nsegments_complete);
/* waits for the context's work in flight; {c, m, v, g} of the last completed segment into host f32[npair][ndm][noct][4]: what
 * the exact test of the records reads */
int xengFfaGetStats(float *stats_host);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengFfaCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengFfaMark(unsigned long long *ticket);
int xengFfaWait(unsigned long long ticket);
int xengFfaTicketDone(unsigned long long ticket, int *done);
int xengFfaSync(void);
int xengFfaDestroy(void);

/* ---------------------------------------------------------------- Folding of search candidates
 * BeamCandFold (no reference counterpart: the reference has no detection stage): what prepfold / pdmp do after a search.  Up to
 * ncand_max candidates are folded at once, each from its own (pair, trial) series of the dedispersed beams, into nsub
 * sub-integrations x nbin phase bins; at the end of each segment a table of period / period-derivative offsets is searched per
 * candidate on the folded cube, and one record and one best profile per candidate come out.  A context of its own, independent of
 * all others, whose kernels run on the beamformer's stream -- rings declared 'beam' cover them, and xengBeamformSync waits for
 * them too.  A fold kernel per call; per completed segment a refine kernel and a clearing launch (csrc/candfold_kernels.h).  The
 * library knows integers only: nothing of pulsars, time or c.
 * Everything below is fp32 and fl() is one rounding to fp32; no product is contracted into a sum anywhere.
 *   in       f32[nwin_call][npair][ndm][nprod], the output span of xengDedispRun unchanged; 16-byte aligned; never written.
 *            1 <= nwin_call <= nwin.  A series is one (p, d), series = p*ndm + d.  z[n] as xengPeriodRun / xengFfaRun take it:
 *            nprod = 1 the word, nprod = 4 fl(XX + YY).  n counts windows since the last reset (xengCandfoldReset, Initialize).
 *   sizes    nbin a power of two, 16 .. 256; 2 <= nsub <= 64 (odd values too), nsub*nbin <= 8192; nsubwin >= 1 windows a
 *            sub-integration; a segment is NT = nsub*nsubwin windows, NT < 2^31, nwin <= NT (a call completes at most one segment);
 *            1 <= ncand_max <= XENG_CANDFOLD_MAX_CAND; 1 <= nwidth, 2^(nwidth-1) <= nbin/2; 1 <= ntrial <= XENG_CANDFOLD_MAX_TRIAL
 *            trials (d1[t], d2[t]), int32, |d| <= 2^20, in sixteenths of a bin; g = f32[nwidth], finite and positive, from the host
 *            ((float)(1/sqrt(w(1 - w/nbin))), w = 2^iw).
 *   candidates  xengCandfoldSetCandidates: per candidate {series, u64 phi0, u64 dphi, i64 ddphi, active}.  The oscillator is
 *            xengFoldSetPhase's word for word: with m = n - n_ref, in wrapping 64-bit arithmetic
 *            Phi(m) = phi0 + dphi*m + ddphi*(m(m-1)/2) and bin = ((Phi >> 32) * nbin) >> 32.  A set takes effect at the next
 *            segment boundary, or at once when the count stands on one (after Initialize or Reset, or exactly between two
 *            segments); n_ref is the window at which it took effect, and m keeps running across segments.  Run refuses a call
 *            whose last m would reach 2^31.  Two candidates may name the same series.  Slots from ncand on are unset.
 *   fold     every call, s = (n mod NT) div nsubwin, b = bin_c(n): cube[c][s][b] = fl(cube[c][s][b] + z_c[n]) in ascending n, one
 *            strictly sequential chain of fp32 adds per word from +0; hits[c][s][b] += 1 (u32).  No atomics and no partial sums:
 *            the cube does not depend on nwin_call, on how calls cut sub-integrations, or on what else runs.  A NaN stays in its
 *            cell.  A call may straddle the end of a segment: it completes that segment (refine, outputs, one clearing launch) and
 *            its remaining windows fold into the next.
 *   refine   on the call that completes a segment, per active candidate.  u_s = 2s + 1 - nsub;
 *            r_t(s) = floor((2N + D) / (2D)), N = d1[t]*u_s*nsub + 2*d2[t]*u_s^2, D = 32*nsub^2, in 64-bit integers with floor
 *            division: d1*(t/T) + d2*(2t/T)^2 sixteenths of a bin about mid-segment, rounded half up to bins.  Per trial t
 *              P_t[b] = sum over s ascending of cube[c][s][(b - r_t(s)) mod nbin], plain adds from +0; H_t[b] the same over hits;
 *              p_t[b] = P_t[b] / (float)H_t[b], a correctly rounded division, +0 where H_t[b] = 0;
 *              circular boxcars B_1 = p_t, B_2w[j] = fl(B_w[j] + B_w[(j + w) mod nbin]);
 *              total_c = ((p_z[0] + p_z[1]) + ...) over the bins of the all-zero-shift profile p_z, whatever the table holds;
 *              base_w = fl(total_c * w/nbin) (w/nbin exact); the score C = fl(fl(B_w[j] - base_w) * g[iw]).
 *            The record is the largest C over (t, iw, j); among equals (+0 and -0 are equal) the smallest t, then iw, then j.  A
 *            NaN is never a maximum.
 *   out      written only by the completing call (*completed = 1): ncand_max records {f32 S, f32 S0, i16 it, i16 iw, i16 j,
 *            i16 pad = 0}, one 16-byte store each, then the best profiles f32[ncand_max][nbin], p_t at the winning trial;
 *            nothing past ncand_max*(16 + 4*nbin) bytes is written.  S0 is the best score, by the same rule, of the first trial
 *            with d1 = d2 = 0 (+0 without one, or when it has no score that is not NaN).  An inactive or unset slot reads
 *            {+0, +0, -1, -1, -1, 0}, a candidate without a score {+0, S0, -1, -1, -1, 0}; their profiles read +0.
 *   state    between two guard bands of 64 KiB: two cubes with their hits (the one that folds; the last completed one, kept for
 *            xengCandfoldGetCube until the next segment completes), two candidate tables, the shifts r_t(s) mod nbin, the gains.
 *            xengCandfoldReset moves the host's counts and enqueues one clearing launch: the partial segment is dropped, the
 *            candidates stay (a set that waited takes effect), the next window is n = 0 with m = 0.
 * Cube, hits, records and profiles are a fixed function of the windows and the candidates: bit-identical however a run is split
 * over calls, after a Reset as in a fresh context, and whatever else runs on the GPU.
 * Rejected at Initialize, before any device is touched: every size outside the ranges above, nprod outside {1, 4},
 * npair*ndm > 2^24, a null or misaligned table, a trial outside +-2^20, a gain that is not finite and positive, a state above
 * XENG_CANDFOLD_MAX_STATE_BYTES.  Rejected by SetCandidates: a null or misaligned array, ncand outside 1..ncand_max, a series
 * outside 0..npair*ndm-1.  Rejected by Run without a launch: a NULL input or result, a misaligned pointer, nwin_call outside
 * 1..nwin, a last m of 2^31 or more, a NULL output on the call that completes a segment.  Every call without a context, Run
 * before the first SetCandidates and GetCube before a segment has completed: XENG_STATUS_INVALID_STATE.
 * Not built: DM refinement (it needs the channelised data, which xengFold* has), interpolated (sub-bin) shifts, a chi^2 statistic,
 * plots or archive output, a second derivative of the period (jerk). */
#define XENG_CANDFOLD_MAX_STATE_BYTES (1LL << 28)
#define XENG_CANDFOLD_MAX_CAND 4096
#define XENG_CANDFOLD_MAX_TRIAL 4096
int xengCandfoldInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int ncand_max, int nbin, int nsub, int nsubwin, int nwidth, int ntrial,
                           const int *d1, const int *d2, const float *g);
/* host arrays of ncand entries.  Waits for the context's work in flight (as xengFoldSetPhase); the set is in force from the next
 * segment boundary, or at once when the window count stands on one */
int xengCandfoldSetCandidates(int ncand, const int *series, const unsigned long long *phi0, const unsigned long long *dphi, const long long *ddphi,
                              const unsigned char *active);
/* enqueue only.  out_dev is written only by a call that completes a segment (*completed = 1); the host's window count decides
 * that before anything is enqueued.  Such a call with out_dev NULL is INVALID_ARGUMENT and enqueues nothing; on every other call
 * out_dev may be NULL and is not touched. */
int xengCandfoldRun(const void *in_dev, int nwin_call, void *out_dev, int *completed);
/* enqueue only: the host's counts, and one clearing launch on the stream */
int xengCandfoldReset(void);
/* windows taken and segments completed since the last reset */
int xengCandfoldGetInfo(long long *nwindows_since_reset, long long *nsegments_complete);
/* waits for the context's work in flight; cube f32 and hits u32 [ncand_max][nsub][nbin] of the last completed segment: what the
 * exact tests read */
int xengCandfoldGetCube(float *cube_host, unsigned int *hits_host);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengCandfoldCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengCandfoldMark(unsigned long long *ticket);
int xengCandfoldWait(unsigned long long ticket);
int xengCandfoldTicketDone(unsigned long long ticket, int *done);
int xengCandfoldSync(void);
int xengCandfoldDestroy(void);

/* ---------------------------------------------------------------- Cleaning of the fine-channel power beams
 * BeamRfiClean (no reference counterpart): the power beams of UpchanSumBeams / UpchanBeamform(dual_pol) are normalised by a
 * bandpass measured per block of nstat windows, channels whose statistics stand out are dropped for that block, single samples
 * and whole windows that stand out are zeroed, and the mean over the channels (the zero-DM series) is taken off every window.  The
 * output has the input's format and is nstat windows late, so xengDedispRun and xengFoldRun read it unchanged.
 * Everything is fp32; fl() is one rounding, and nothing is contracted into an fma.
 *   in       f32[nwin_call][npair][nfine][4] = [XX, YY, Re XY*, Im XY*], as xengDedispRun takes it; 16-byte aligned, never written
 *   out      the same shape and format; stats i32[nwin_call][npair][4], 16-byte aligned
 *   n        counts windows since the last reset.  out[i] of a call that starts at window n0 is the cleaned window n0 + i - nstat;
 *            for n0 + i < nstat the four words of every channel are +0 and stats = {0, 0, 4, 0}.
 *   sizes    1 <= npair <= 65535, 4 <= nfine <= 8192, 2 <= nstat <= 2^20, 1 <= nwin <= nstat, 1 <= nwin_call <= nwin, and the
 *            history of nstat + nwin windows below XENG_RFI_MAX_HISTORY_BYTES.
 *   control  k_chan (channel threshold, in units of the median absolute deviation; the host folds in 1.4826), t_clip (sample
 *            threshold on z; the host folds in sqrt 2), t_broad (the host folds in sqrt 2), all finite and > 0; min_count in
 *            0..nfine; zerodm 0 or 1.  mask u8[nfine]: non-zero leaves the channel out.  Controls and mask hold from the next
 *            block to be decided: a block is decided by the call that takes its last window, with what stands at that call.
 *   baseline of block k = windows [k nstat, (k+1) nstat), per (pair, channel, word w): at the block's first window c_w = x_w,
 *            a_w = +0, and for w in {0, 1} s_w = +0.  For every window of the block in ascending n, the first included:
 *              d = fl(x_w - c_w);  a_w = fl(a_w + d);  s_w = fl(s_w + fl(d d)) for w in {0, 1}.
 *            At the block's end, with r = 1.0f / (float)nstat formed on the host: m_w = fl(a_w r),
 *            v_w = fl(fl(s_w r) - fl(m_w m_w)) for w in {0, 1}.
 *   decision per (pair, block): mu = fl(fl(c_0 + m_0) + fl(c_1 + m_1)), V = fl(v_0 + v_1), R = fl(V / fl(mu mu)): the variance
 *            of the total power over its squared mean, flat across a clean band whatever the bandpass.  A channel is live iff
 *            its mask byte is 0, the four m_w are finite, 0 < v_0, v_1 < +inf, mu > 0 and R is finite.  med is the median of R
 *            over the live channels: ranked by a sortable key of fl(R + 0) (-0 as +0), ties by index; the value of rank n/2 for
 *            odd n, 0.5f (lo + hi) of ranks (n-1)/2 and n/2 for even n, +0 for n = 0.  dev = |fl(R - med)|, mad the median of dev
 *            by the same rule.  A live channel is an outlier iff dev > fl(k_chan mad).  Flag byte: bit 0 the mask, bit 1 one of
 *            the other conditions of "live" fails (whether or not the channel is masked), bit 2 outlier.  A channel is kept iff
 *            its byte is 0.  Gains of a kept channel: g_0 = fl(1 / fl(sqrt v_0)), g_1 from v_1, g_2 = g_3 = fl(sqrt fl(g_0 g_1))
 *            -- power gains per hand and their geometric mean on the cross words, what a voltage gain per hand does; the gains of
 *            every other channel read +0.  Division and square root are correctly rounded.
 *   apply    per window n of a decided block and per pair, with the block's tables and the controls it was decided under:
 *            on kept channels y_w = fl(fl(fl(x_w - c_w) - m_w) g_w), z = fl(y_0 + y_1); the sample is clipped iff some y_w is
 *            not finite or !(|z| <= t_clip).  K = the kept, unclipped channels, count = |K|.  Sums over K per word in a fixed
 *            order: chain t in [0, 256) starts from +0 and takes channels q = t (mod 256) ascending (a channel outside K enters
 *            as +0); then P_t = fl(P_t + P_{t+h}) for t < h, h = 128, 64, .. 1; Z_w = P_0.  zm_w = fl(Z_w / (float)count), +0 at
 *            count = 0.  The window has code 1 iff count < min_count; otherwise code 2 iff
 *            |fl(Z_0 + Z_1)| > fl(t_broad fl(sqrt (float)count)); otherwise 0.  A window with a code writes +0 everywhere.
 *            Otherwise a channel in K writes fl(y_w - zm_w) with zerodm, y_w without, and every other channel four +0.
 *            stats = {count, clipped samples among kept channels, code, channels not kept in the block}.
 *            A +0 is the mean of a normalised channel: excised data is zero, not NaN, and the dedisperser's sums need no weights.
 *   state    between two guard bands of 64 KiB: a ring of nstat + nwin windows in the input's layout, the running {c, a, s},
 *            and two halves of block tables {c, m, v, g, flag, mu, V, R} that change places block by block (a call applies at
 *            most two blocks, and the newer one completes inside that call), the mask.
 * xengRfiReset moves the host's counts; it launches and clears nothing: the kernels decide by index what lies before window 0.
 * Everything is a fixed function of the window stream, the mask and the controls: bit-identical however a run is split over calls,
 * after a Reset as in a fresh context, and whatever else runs on the GPU.
 * Rejected at Initialize, before any device is touched: every size outside the ranges above, a history of
 * XENG_RFI_MAX_HISTORY_BYTES or more.  Rejected by SetControl: a float that is not finite and > 0, zerodm outside {0, 1},
 * min_count outside 0..nfine.  Rejected by Run without a launch: a NULL or misaligned pointer, nwin_call outside 1..nwin.  Every
 * call without a context, Run before the first SetControl, GetBlock before a block is decided: XENG_STATUS_INVALID_STATE.
 * Not built: statistics re-estimated after clipping (a burst inflates its own block's v; the test on R then drops the channel for
 * that block), a test along time between blocks, a smooth-bandpass test on mu, a flush of the last nstat windows, a mask ring. */
#define XENG_RFI_MAX_HISTORY_BYTES (1LL << 32)
int xengRfiInitialize(int gpu, int npair, int nfine, int nwin, int nstat);
int xengRfiSetControl(float k_chan, float t_clip, float t_broad, int min_count, int zerodm);
/* host array u8[nfine], or NULL for no channel left out.  Waits for the context's work in flight */
int xengRfiSetMask(const unsigned char *mask);
/* enqueue only: the three launches (the decision only on a call that takes a block's last window: *completed = 1) */
int xengRfiRun(const void *in_dev, int nwin_call, void *out_dev, void *stats_dev, int *completed);
/* the host's counts only */
int xengRfiReset(void);
/* windows taken and blocks decided since the last reset */
int xengRfiGetInfo(long long *nwindows_since_reset, long long *nblocks_decided);
/* waits for the context's work in flight; the newest decided block's tables: flags u8[npair][nfine], mu, var (V) and r
 * f32[npair][nfine], gains f32[npair][nfine][4] */
int xengRfiGetBlock(unsigned char *flags, float *mu, float *var, float *r, float *gains);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengRfiCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengRfiMark(unsigned long long *ticket);
int xengRfiWait(unsigned long long ticket);
int xengRfiTicketDone(unsigned long long ticket, int *done);
int xengRfiSync(void);
int xengRfiDestroy(void);

/* ---------------------------------------------------------------- Baseline removal of the dedispersed beams
 * BeamDetrend (no reference counterpart): under every (pair, DM trial) series of xengDedispRun's output lies a slowly varying
 * baseline that the searches behind assume away.  Per block of nblk windows and per series a knot is measured, the median and the
 * median absolute deviation; every window then loses the straight line between the two knots around it and, with `normalise`, is
 * scaled by the line between the knots' reciprocal scales.  The output is one word per series and 3 nblk / 2 windows late, in the
 * format xengPulseRun, xengPeriodRun, xengPlongRun, xengAccelRun, xengFfaRun and xengCandfoldRun take at nprod = 1.
 * Everything is fp32; fl() is one rounding, and nothing is contracted into an fma.
 *   in       f32[nwin_call][npair][ndm][nprod], xengDedispRun's output, 16-byte aligned, never written.  z = in[..][0] at
 *            nprod = 1, z = fl(XX + YY) at nprod = 4.  A series is one (pair, trial); nser = npair ndm <= 2^24.
 *   out      f32[nwin_call][npair][ndm], 16-byte aligned: always one word per series.
 *   sizes    nblk even, 4 <= nblk <= 8192; h = nblk/2, D = 3h; 1 <= nwin <= nblk, 1 <= nwin_call <= nwin; nprod 1 or 4; the
 *            history of D + nwin windows of nser floats below XENG_DETREND_MAX_HISTORY_BYTES.  Given to Initialize beside the
 *            sizes: normalise in {0, 1}; k_mad, finite and > 0 (the host folds in 1.4826); the library forms
 *            r = 1.0f / (float)(2 nblk) on the host.  There are no run-time controls.
 *   n        counts windows since the last reset.
 *   knots    block k is the windows [k nblk, (k+1) nblk); its knot is decided by the call that takes its last window.  Per
 *            series: M_k is the median of the block's z, A_k the median of |fl(z - M_k)|.  Both by one rule: the values are
 *            ranked by a sortable key of fl(v + 0) (-0 as +0), lo and hi are the values fl(v + 0) of ranks nblk/2 - 1 and
 *            nblk/2 (equal keys are equal values: ties need no rule), and the median is fl(0.5f fl(lo + hi)).
 *            The knot is valid iff all nblk values z are finite and, with normalise, s = fl(k_mad A_k) satisfies 0 < s < +inf;
 *            then G_k = fl(1.0f / s), correctly rounded.  A block with a z that is not finite has M_k = A_k = +0; G_k = +0
 *            wherever the knot is not valid or nothing is normalised.
 *   apply    out[i] of a call that starts at window n0 is the detrended window m = n0 + i - D; for m < 0 it is +0.  For m < h,
 *            k = -1 and t = m + h; otherwise k = (m - h) div nblk and t = m - (k nblk + h).  The two knots are a = max(k, 0)
 *            and b = k + 1; both are complete by the time window m + D has been taken: the latency is a constant.  If exactly
 *            one of them is not valid the other stands for both; if neither is, the output is +0.  With
 *            u = fl((float)(2t + 1) r):
 *              base = fl(M_a + fl(u fl(M_b - M_a)));  y = fl(z - base);
 *              with normalise, g = fl(G_a + fl(u fl(G_b - G_a))) and y = fl(y g).
 *            A y that is not finite is written as +0: excised data is zero, as in the cleaner.
 *   state    between two guard bands of 64 KiB: a ring of D + nwin windows per series, time the fastest axis, and four slots of
 *            knot tables {M, A, G, valid} that blocks take in turn (a call reads the knots of at most three blocks, the newest
 *            decided inside that call).
 * xengDetrendReset moves the host's counts; it launches and clears nothing: the kernels decide by index what lies before window 0.
 * Everything is a fixed function of the window stream: bit-identical however a run is split over calls, after a Reset as in a
 * fresh context, and whatever else runs on the GPU.
 * Rejected at Initialize, before any device is touched: every size outside the ranges above, normalise outside {0, 1}, a k_mad
 * that is not finite and > 0, a history of XENG_DETREND_MAX_HISTORY_BYTES or more.  Rejected by Run without a launch: a NULL or
 * misaligned pointer, nwin_call outside 1..nwin.  Every call without a context, GetKnots before a block is decided:
 * XENG_STATUS_INVALID_STATE.
 * Not built: a running median per sample instead of per-block knots, knots re-estimated after detected pulses are masked (a
 * pulse shorter than nblk/2 windows cannot move the median; a longer one is baseline), a flush of the last D windows, spectral
 * median whitening inside xengPlongRun. */
#define XENG_DETREND_MAX_HISTORY_BYTES (1LL << 32)
int xengDetrendInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int nblk, int normalise, float k_mad);
/* enqueue only: the three launches (the decision only on a call that takes a block's last window: *completed = 1) */
int xengDetrendRun(const void *in_dev, int nwin_call, void *out_dev, int *completed);
/* the host's counts only */
int xengDetrendReset(void);
/* windows taken and blocks decided since the last reset */
int xengDetrendGetInfo(long long *nwindows_since_reset, long long *nblocks_decided);
/* waits for the context's work in flight; the newest decided block's knots: M and A f32[npair][ndm], valid u8[npair][ndm] */
int xengDetrendGetKnots(float *M, float *A, unsigned char *valid);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengDetrendCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengDetrendMark(unsigned long long *ticket);
int xengDetrendWait(unsigned long long ticket);
int xengDetrendTicketDone(unsigned long long ticket, int *done);
int xengDetrendSync(void);
int xengDetrendDestroy(void);

/* ---------------------------------------------------------------- Dedispersed cut-outs and DM refinement of single pulses
 * BeamPulseCutout (no reference counterpart): the follow-up stage of a single-pulse candidate, as xengCandfold* is that of a
 * periodic one.  The engine keeps a history of the channelised power beams of its own and, on request, cuts out of it the
 * dedispersed dynamic spectrum of one pulse (the waterfall), its DM-time plane over a fine DM grid (the "bow tie"), and the best
 * boxcar score over that plane: a DM finer than the search grid, a width and a time.  The library knows integers only: nothing of
 * the dispersion constant, of time or of DM (blocks/pulse_cutout.py).
 * Everything is fp32; fl() is one rounding; no product is contracted into a sum except where fmaf is written.
 *   in       f32[nwin_call][npair][nfine][4] = [XX, YY, Re XY*, Im XY*], what xengDedispRun and xengFoldRun take; 16-byte
 *            aligned, never written.  x = fl(XX + YY).  n counts windows since the last reset.
 *   history  f32[npair][nfine][L], L = nhist + nwin, time the fastest axis: window n at slot n mod L, stored unweighted.  After a
 *            call that ends at count n the windows [max(0, n - nhist), n) are held.  xengCutoutReset moves the host's counts and
 *            drops the pending requests; it launches and clears nothing: by index, nothing from before window 0 is read.
 *   tables   SetDelays: i32[ndmf][nfine], the forward delays s[d][q] >= 0 of a fine DM grid (blocks/dedisp.py dm_delays' output
 *            as it is); refused if a delay is negative or max s + ntu > nhist; it clears the count and the pending requests.
 *            SetWeights: f32[nfine], finite (NULL: all 1); a weight of 0 leaves a channel out; it acts on the history held.
 *   sizes    at Initialize: 1 <= npair <= 65535; nfine >= 1; 1 <= nwin; 1 <= ndmf, ndmf nfine <= 2^28; nband in 1..256 divides
 *            nfine, band g = channels [g nfine/nband, (g+1) nfine/nband); tscr a power of two in 1..64; nt even in 16..1024,
 *            ntu = nt tscr; ndmc in 1..256, centre row c = ndmc div 2; nwidth >= 1 with 2^(nwidth-1) <= nt/2; nreq_max in 1..64;
 *            nhist >= ntu; k_mad finite and > 0 (the host folds in 1.4826); the history below XENG_CUTOUT_MAX_HISTORY_BYTES.
 *   request  xengCutoutReq {i32 id, i32 pair, i64 n_c, i32 ic, i32 dstep}: n_c is the window at which the pulse stands in the
 *            zero-delay channel.  Row i of the cut-out is fine trial d_i = ic + (i - c) dstep, dstep >= 1; a row with d_i outside
 *            0..ndmf-1 is ABSENT.  Column m of 0..ntu-1 is window a(m) = n_c - ntu/2 + m at the zero-delay channel.  The request
 *            needs the windows from first = a(0) to last = a(ntu-1) + max over present rows of max_q s[d_i][q].  Refused, and
 *            then none of the call's requests is taken: a pair or an ic out of range, n_c < 0 or >= 2^62, dstep outside 1..2^20,
 *            more than XENG_CUTOUT_MAX_PENDING waiting.
 *   serving  The host's counts decide, before anything is enqueued.  After the ingest of a call that ends at count n the pending
 *            requests are taken in the order given: first < n - nhist: EXPIRED, reported and never served; otherwise last < n:
 *            SERVED, in slot 0, 1, .. of this call, at most nreq_max per call (one that is due beyond that waits); otherwise
 *            it waits.  Run returns the ids served, in slot order, and the ids expired.  A request given before its last window
 *            comes is served for certain if nhist >= ntu + S + nwin - 1 (S its largest delay: the call that brings the last
 *            window may bring nwin - 1 more), and nwin more for every call it may have to wait for a free slot.
 *   partials for a present row i, band g and column m: D_i[g][m] starts from +0 and takes the band's channels in ascending q, one
 *            fmaf(w[q], v, sum) each, v = x[a(m) + s[d_i][q]][pair][q], and v = +0 where w[q] = 0 or the window lies before 0 (a
 *            select, as in xengDedispRun: a NaN in a left-out channel never arrives).
 *   waterfall W[g][j] = sum over u = 0..tscr-1 ascending of D_c[g][j tscr + u], plain adds from +0 (all +0 if row c is absent:
 *            it cannot be, 0 <= ic < ndmf).
 *   plane    B_i[m] = sum over g ascending of D_i[g][m], plain adds from +0; P[i][j] = sum over u ascending of B_i[j tscr + u],
 *            plain adds from +0.  An absent row is +0.
 *   refine   per present row: M_i and A_i are the median and the median absolute deviation of P[i][0..nt) by xengDetrend's knot
 *            rule: ranked by a sortable key of fl(v + 0), lo and hi the values of ranks nt/2 - 1 and nt/2, the median
 *            fl(0.5f fl(lo + hi)); A_i the same of |fl(fl(v + 0) - M_i)|.  The row is VALID iff all nt values are finite and
 *            0 < fl(k_mad A_i) < +inf; then G_i = fl(1.0f / fl(k_mad A_i)), correctly rounded.  y[j] = fl(P[i][j] - M_i).
 *            Boxcars as xengPulseRun's tree: B_1 = y, B_2w[j] = fl(B_w[j] + B_w[j - w]) for j >= 2w - 1.  The score
 *            C = fl(fl(B_w[j] G_i) rho_iw), w = 2^iw, rho_iw = (float)2^(-iw/2) formed on the host.
 *   record   the largest C over valid rows, iw < nwidth and j >= w - 1; among equals (+0 and -0 are equal) the smallest i, then
 *            iw, then j.  A NaN is never a maximum.  S0 is the best score of the centre row by the same rule, +0 without one.
 *   out      A call that serves nothing launches the ingest only and touches no output (out_dev may be NULL then).  A call that
 *            serves r >= 1 writes: nreq_max records of 32 bytes {i32 id, i32 status, f32 S, f32 S0, i16 i, i16 iw, i16 j, i16 0,
 *            f32 M, f32 A} (M and A of row i); slots from r on read {-1, 0, +0, +0, -1, -1, -1, 0, +0, +0}; a served request
 *            without a score {id, 1, +0, S0 = +0, -1, -1, -1, 0, +0, +0}.  Then per slot W f32[nband][nt] (slot z at byte
 *            32 nreq_max + 4 z nband nt), then per slot P f32[ndmc][nt] (slot z at 32 nreq_max + 4 nreq_max nband nt +
 *            4 z ndmc nt).  Only the areas of slots < r are written, and nothing past nreq_max (32 + 4 nt (nband + ndmc)) bytes.
 *   state    between two guard bands of 64 KiB: the history, the two tables, the row records of the last serving call.
 * A served cut-out is a fixed function of the window stream, the tables and the request: bit-identical however the run is split
 * over calls and whichever call serves it, after a Reset as in a fresh context, and whatever else runs on the GPU.  Exact on
 * integer data while the sums stay below 2^24.
 * Rejected at Initialize, before any device is touched: every size outside the ranges above.  Rejected by Run without a launch: a
 * NULL or misaligned input, a NULL result, nwin_call outside 1..nwin, a NULL or misaligned output on a serving call (the pending
 * requests stay as they were).  Every call without a context, and Run or Request before SetDelays: XENG_STATUS_INVALID_STATE.
 * Not built: the four Stokes words (I only), sharing xengDedisp's ring instead of a second history, sub-window delays, a
 * scattering fit, a file or trigger writer. */
#define XENG_CUTOUT_MAX_HISTORY_BYTES (1LL << 32)
#define XENG_CUTOUT_MAX_PENDING 1024
typedef struct xengCutoutReq {
    int id, pair;
    long long n_c;
    int ic, dstep;
} xengCutoutReq;
int xengCutoutInitialize(int gpu, int npair, int nfine, int nwin, int ndmf, int nhist, int nband, int nt, int tscr, int ndmc, int nwidth, int nreq_max,
                         float k_mad);
/* host array i32[ndmf][nfine].  Waits for the context's work in flight; clears the count and the pending requests */
int xengCutoutSetDelays(const int *delays);
/* host array f32[nfine], or NULL for all 1.  Waits for the context's work in flight */
int xengCutoutSetWeights(const float *weights);
/* host array of nreq requests, appended to the pending ones in the order given: all of them or, on a refusal, none */
int xengCutoutRequest(int nreq, const xengCutoutReq *reqs);
/* enqueue only.  served_ids i32[nreq_max] and expired_ids i32[XENG_CUTOUT_MAX_PENDING] are host arrays; out_dev is written only
 * when *nserved >= 1 */
int xengCutoutRun(const void *in_dev, int nwin_call, void *out_dev, int *nserved, int *served_ids, int *nexpired, int *expired_ids);
/* the host's counts and the pending requests only */
int xengCutoutReset(void);
/* windows taken since the last reset, requests waiting, and the bytes of a serving call's output */
int xengCutoutGetInfo(long long *nwindows_since_reset, int *npending, long long *out_bytes);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengCutoutCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengCutoutMark(unsigned long long *ticket);
int xengCutoutWait(unsigned long long ticket);
int xengCutoutTicketDone(unsigned long long ticket, int *done);
int xengCutoutSync(void);
int xengCutoutDestroy(void);

/* ---------------------------------------------------------------- Faraday rotation-measure synthesis of folded profiles
 * BeamRmSynth (no reference counterpart): the follow-up stage of the folded dual-pol cube xengFoldDump writes at nprod = 4.  Per
 * beam pair: the Faraday spectrum over a grid of nphi depths, the depth of its peak, and the band-summed I, Q, U, V profile
 * de-rotated at that depth.  The library takes numbers and knows nothing of Faraday rotation, wavelengths or depths: the host
 * gives, per channel group g and depth k, the two words of a rotation (blocks/rm_synth.py rm_table).
 * Everything is fp32; fl() is one rounding; no product is contracted into a sum except where fmaf is written.
 *   in       X f32[npair][4][nchg][nbin], bin the fastest; 16-byte aligned, never written.
 *   tables   SetTable: T f32[nchg][nphi][2] = (Tc, Ts), w f32[nchg] (NULL: all 1), use u8[nchg] (NULL: all 1); w finite, T finite
 *            in the used channels.  A channel with use = 0 is never read, in X or in T: a NaN there is harmless.
 *            SetMasks: off, on u8[npair][nbin], the off-pulse and on-pulse bins (NULL: every bin); n_off and n_on count them.
 *            SetActive: u8[npair] (NULL: all).  The setters wait for the context's work in flight.
 *   sizes    at Initialize: 1 <= npair <= 65535; 1 <= nchg <= 65536; 1 <= nbin <= 65536; 1 <= nphi <= 4096; nchg nphi 8 bytes
 *            <= 1 GiB; feeds 0 (linear) or 1 (circular); the output and the run partials below 4 GiB each.
 *   stokes   per (p, g, b), X0..X3 the four words:  linear   i = fl(X0+X1), q = fl(X0-X1), u = fl(X2+X2), v = fl(X3+X3)
 *                                                   circular i = fl(X0+X1), q = fl(X2+X2), u = fl(X3+X3), v = fl(X0-X1)
 *   baseline one value per (p, g) and word s of i, q, u, v: 64 partial chains from +0, chain j over the bins with b mod 64 = j and
 *            off[p][b] != 0 in ascending b, plain adds; the 64 partials summed from +0 in ascending j; divided by (float)n_off,
 *            correctly rounded; +0 if n_off = 0.  y_s = fl(s - base_s).
 *   faraday  per (p, b, k): (re, im) from (+0, +0) over the used g in ascending order, four steps a channel in this order:
 *            re = fmaf(y_q, Tc[g][k], re); re = fmaf(y_u, Ts[g][k], re); im = fmaf(y_u, Tc[g][k], im); im = fmaf(-y_q, Ts[g][k], im);
 *            then pw = fmaf(im, im, fl(re re)).
 *   spectrum per (p, k): per run r of 64 consecutive bins (b div 64 = r) a chain from +0 of plain adds of pw in ascending b over
 *            on[p][b] != 0; spec[p][k] a chain from +0 of plain adds of the runs in ascending r.
 *   record   per pair {i32 k, f32 peak, i32 n_on, i32 n_off}: k the depth of the largest spec[p][k], the smallest k among
 *            equals (+0 and -0 are equal); a NaN is never chosen.  k = -1 and peak = +0 if n_on = 0 or no word is comparable.
 *   profile  f32[npair][4][nbin]: words 0 and 3 chains from +0 of fmaf(w[g], y_i, .) and fmaf(w[g], y_v, .) over the used g in
 *            ascending order; words 1 and 2 re and im of the Faraday word at the record's k, +0 if k = -1.
 *   inactive nothing of X is read; the record is {-1, +0, 0, 0} and every word of spec and of the profile +0.
 *   out      npair records of 16 bytes, then spec f32[npair][nphi] at byte 16 npair, then the profile at byte 16 npair +
 *            4 npair nphi (xengRmsynthGetInfo gives both offsets and the size); nothing past it is written.
 *   state    between two guard bands of 64 KiB: T, w, use, the list of used channels, the masks and their counts, the active
 *            list, the baselines, the per-run partials, spec and the picked depths.
 * Every output word is one chain in a fixed order: a call is a fixed function of X and the tables, bit-identical on a second call,
 * after a Reset as in a fresh context, whatever the tile sizes and whatever else runs on the GPU; spec on a sub-list of the depths
 * equals those words of the full spectrum bit for bit (a word of spec reads one column of T).  Which words are NaN is part of
 * that; a NaN's sign and payload are not.  Exact on integer data while the sums stay below 2^24 (with a table of integers).
 * xengRmsynthReset clears the call count; it launches and clears nothing.
 * Rejected at Initialize, before any device is touched: every size outside the ranges above.  Rejected by Run without a launch: a
 * NULL or misaligned input or output.  Every call without a context, and Run before SetTable: XENG_STATUS_INVALID_STATE.
 * Not built: leakage and X-Y phase calibration, an ionospheric model, spectra summed over sub-integrations (additive: on the
 * host), RM-CLEAN, a depth grid per pair, single-pulse RM from the cut-outs, a contraction on MFMAs. */
#define XENG_RMSYNTH_MAX_NPHI 4096
#define XENG_RMSYNTH_MAX_NBIN 65536
#define XENG_RMSYNTH_MAX_NCHG 65536
#define XENG_RMSYNTH_MAX_TABLE_BYTES (1LL << 30)
int xengRmsynthInitialize(int gpu, int npair, int nchg, int nbin, int nphi, int feeds);
/* host arrays f32[nchg][nphi][2], f32[nchg] or NULL, u8[nchg] or NULL.  Waits for the context's work in flight */
int xengRmsynthSetTable(const float *T, const float *w, const unsigned char *use);
/* host arrays u8[npair][nbin], either may be NULL (every bin).  Waits for the context's work in flight */
int xengRmsynthSetMasks(const unsigned char *off, const unsigned char *on);
/* host array u8[npair], or NULL for all.  Waits for the context's work in flight */
int xengRmsynthSetActive(const unsigned char *active);
/* enqueue only: four launches on the beamformer's stream */
int xengRmsynthRun(const void *in_dev, void *out_dev);
/* the host's call count only */
int xengRmsynthReset(void);
/* calls since the last reset, the used channels (-1 before SetTable), the byte offsets of spec and of the profile, the output's bytes */
int xengRmsynthGetInfo(long long *ncalls_since_reset, int *nused, long long *spec_offset, long long *prof_offset, long long *out_bytes);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengRmsynthCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengRmsynthMark(unsigned long long *ticket);
int xengRmsynthWait(unsigned long long ticket);
int xengRmsynthTicketDone(unsigned long long ticket, int *done);
int xengRmsynthSync(void);
int xengRmsynthDestroy(void);

/* ---------------------------------------------------------------- Template-matched arrival phases of folded profiles
 * BeamToa (no reference counterpart): the stage between the folded cube xengFoldDump writes (nprod = 1 or 4) and a timing program.
 * Per beam pair and per row -- the nsub sub-bands r = 0 .. nsub-1 and the whole band r = nsub -- the weighted profile, its baseline
 * and noise over the off-pulse bins, its harmonics 1 .. nharm, and its correlation with a template on a grid of nlag lags with the
 * lag of the peak.  The library takes numbers and knows nothing of frequencies, pulsars or time: the host gives every sine and
 * cosine as a table (blocks/toa.py toa_tables) and the templates' harmonics (toa_template), and does the sub-lag refinement, the DM
 * fit and the conversion to a time in float64 from this output (toa_refine, toa_dm_fit, toa_epoch).
 * Everything is fp32; fl() is one rounding; no product is contracted into a sum except where fmaf is written.  k = 1 .. nharm
 * throughout; a table's index [k] is k - 1.
 *   in       X f32[npair][nprod][nchg][nbin], bin the fastest; 16-byte aligned, never written.
 *   tables   SetBands: edges i32[nsub+1], 0 <= edges[0] <= ... <= edges[nsub] <= nchg, sub-band r is the groups [edges[r], edges[r+1]);
 *            w f32[nchg] (NULL: all 1), finite.  A group is used if it lies in a sub-band and w[g] != 0; a group that is not used is
 *            never read: a NaN there is harmless.
 *            SetTables: D f32[nbin][nharm][2] = (cos, -sin)(2 pi k b / nbin), L f32[nharm][nlag][2] = (cos, -sin)(2 pi k l / nlag).
 *            SetTemplate: S f32[npair][nsub+1][nharm][2] = (sr, si).  D, L and S finite.
 *            SetMask: off u8[npair][nbin], the off-pulse bins (NULL: every bin); n_off counts them.
 *            SetActive: u8[npair] (NULL: all).  The setters wait for the context's work in flight.
 *   sizes    at Initialize: 1 <= npair <= 65535; nprod 1 or 4; 1 <= nchg <= 65536; 1 <= nbin <= 16384; 1 <= nsub <= 256;
 *            1 <= nharm <= min(4096, (nbin-1)/2); 1 <= nlag <= 65536; each of D, L, S at most 1 GiB; the output below 4 GiB.
 *   x        per (p, g, b): X[p][0][g][b] at nprod = 1; fl(X[p][0][g][b] + X[p][1][g][b]) at nprod = 4.
 *   P        P[p][r][b], r < nsub: a chain from +0 of acc = fmaf(w[g], x, acc) over the used groups of sub-band r in ascending g
 *            (+0 if it has none).  P[p][nsub][b]: a chain from +0 of plain adds of P[p][r][b] over r = 0 .. nsub-1 ascending.
 *   base     per (p, r): 64 partial chains from +0, chain j over the bins with b mod 64 = j and off[p][b] != 0 in ascending b, plain
 *            adds of P; the 64 partials summed from +0 in ascending j; divided by (float)n_off, correctly rounded; +0 if n_off = 0.
 *   var      the same scheme over fl(d d), d = fl(P - base); +0 if n_off = 0.
 *   PH       PH[p][r][k] = (re, im): chains from +0 over all b ascending, re = fmaf(d_b, D[b][k][0], re), im = fmaf(d_b, D[b][k][1], im).
 *   cross    cr = fmaf(re, sr, fl(im si)); ci = fmaf(im, sr, -fl(re si)), (sr, si) = S[p][r][k].
 *   ccf      ccf[p][r][l]: a chain from +0 over k ascending, two steps a harmonic in this order:
 *            acc = fmaf(cr, L[k][l][0], acc); acc = fmaf(ci, L[k][l][1], acc).  It peaks where l / nlag is the profile's delay behind
 *            the template in turns.
 *   record   per (p, r) {i32 l, f32 peak, f32 base, f32 var}: l the lag of the largest ccf[p][r][l], the smallest l among equals
 *            (+0 and -0 are equal); a NaN is never chosen.  l = -1 and peak = +0 if no word is comparable or the row has no used
 *            group (the band row: no sub-band has one); base and var are the words above either way.
 *   inactive nothing of X is read; every record is {-1, +0, +0, +0} and every word of P, PH and ccf +0.
 *   out      records [npair][nsub+1] of 16 bytes, then P f32[npair][nsub+1][nbin], then PH f32[npair][nsub+1][nharm][2], then
 *            ccf f32[npair][nsub+1][nlag], with no gaps (xengToaGetInfo gives the three offsets and the size); nothing past it is
 *            written.
 *   state    between two guard bands of 64 KiB: D, L, S, w, the lists of used groups, the mask and its counts, the active list,
 *            base and var.
 * Every output word is one chain in a fixed order: a call is a fixed function of X and the tables, bit-identical on a second call,
 * after a Reset as in a fresh context, whatever the tile sizes and whatever else runs on the GPU.  Which words are NaN is part of
 * that; a NaN's sign and payload are not.  P is exact on integer data while the sums stay below 2^24.
 * xengToaReset clears the call count; it launches and clears nothing.
 * Rejected at Initialize, before any device is touched: every size outside the ranges above.  Rejected by the setters: a NULL or
 * misaligned table, edges that descend or leave the groups, a word that is not finite.  Rejected by Run without a launch: a NULL or
 * misaligned input or output.  Every call without a context, and Run before SetBands, SetTables and SetTemplate:
 * XENG_STATUS_INVALID_STATE.
 * Not built: barycentring, a par-file or polyco reader, a .tim or archive writer, template generation from data,
 * profile-evolution (2-D template) fits, scattering fits. */
#define XENG_TOA_MAX_NBIN 16384
#define XENG_TOA_MAX_NHARM 4096
#define XENG_TOA_MAX_NLAG 65536
#define XENG_TOA_MAX_NSUB 256
#define XENG_TOA_MAX_NCHG 65536
#define XENG_TOA_MAX_TABLE_BYTES (1LL << 30)
int xengToaInitialize(int gpu, int npair, int nprod, int nchg, int nbin, int nsub, int nharm, int nlag);
/* host arrays i32[nsub+1] and f32[nchg] or NULL.  Waits for the context's work in flight */
int xengToaSetBands(const int *edges, const float *w);
/* host arrays f32[nbin][nharm][2] and f32[nharm][nlag][2].  Waits for the context's work in flight */
int xengToaSetTables(const float *D, const float *L);
/* host array f32[npair][nsub+1][nharm][2].  Waits for the context's work in flight */
int xengToaSetTemplate(const float *S);
/* host array u8[npair][nbin], or NULL for every bin.  Waits for the context's work in flight */
int xengToaSetMask(const unsigned char *off);
/* host array u8[npair], or NULL for all.  Waits for the context's work in flight */
int xengToaSetActive(const unsigned char *active);
/* enqueue only: six launches on the beamformer's stream */
int xengToaRun(const void *in_dev, void *out_dev);
/* the host's call count only */
int xengToaReset(void);
/* calls since the last reset, the used groups of each sub-band (i32[nsub], -1 before SetBands), the byte offsets of P, PH and ccf,
 * the output's bytes */
int xengToaGetInfo(long long *ncalls_since_reset, int *nused, long long *prof_offset, long long *harm_offset, long long *ccf_offset, long long *out_bytes);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengToaCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengToaMark(unsigned long long *ticket);
int xengToaWait(unsigned long long ticket);
int xengToaTicketDone(unsigned long long ticket, int *done);
int xengToaSync(void);
int xengToaDestroy(void);

/* ---------------------------------------------------------------- Coherent dedispersion of the voltage beams
 * BeamCoherentDedisperse (no reference counterpart): every (coarse channel, selected beam) row of the voltage beams is filtered by
 * overlap-save with a table given in the frequency domain, and comes out in the format it came in.  The library knows nothing of
 * the dispersion constant: blocks/coherent_dedisp.py builds the table.  A context of its own, independent of all others, whose
 * kernels run on the beamformer's stream -- rings declared 'beam' cover them, and xengBeamformSync waits for them too.  An ingest
 * kernel per call (one more where a call straddles a block boundary) and a filter kernel per completed block
 * (csrc/cdedisp_kernels.h).
 *   in       cf32[nchan][nbeam][ntime], the output of xengBeamformRun unchanged; 16-byte aligned; never written.  ntime is fixed
 *            per context.  The selected beams are 2*pair0 .. 2*(pair0 + npair) - 1; a row is one (c, selected beam b),
 *            nrow = nchan * 2*npair.  Samples are counted from the last reset (xengCdedispReset, Initialize).
 *   sizes    NFFT = nfft, a power of two, 2^8 <= NFFT <= 2^13 (64 KiB of LDS at 2^13).  M = overlap: even, 0 <= M <= NFFT/2.
 *            L = NFFT - M, the step.
 *   block    Block j covers the input samples [j*L, j*L + NFFT) and runs in the call that brings its last sample.  Per row:
 *              X[k] = sum_n x[n] * exp(-2 pi i k n / NFFT),  Y[k] = X[k] * T[p][c][k],  y[n] = sum_k Y[k] * exp(+2 pi i k n / NFFT)
 *            with p = b div 2 (both beams of a pair share a filter) and nothing else scaled: the table carries the 1/NFFT.  The
 *            block's output is y[M/2 .. M/2 + L): output sample i of the stream is input sample i + M/2, and the blocks tile the
 *            time axis without a gap.  fp32, held to a tolerance; no atomics, one owner per word.
 *   out      cf32[nblk][nchan][2*npair][L], one unit per block the call completes, 16-byte aligned; nothing past nblk units is
 *            written.  A call completes at most ceil(ntime / L) blocks (xengCdedispGetInfo).
 *   table    cf32[npair][nchan][NFFT] on the host in natural DFT order: bin k is the offset k*D/NFFT from the channel's centre for
 *            k < NFFT/2 and (k - NFFT)*D/NFFT above, D the channel width.  After Initialize it is 1/NFFT everywhere: a pure latency
 *            of M/2 samples.
 *   state    between two guard bands of 64 KiB: the time buffer cf32[nrow][NFFT], the table (in the kernel's order) and the
 *            twiddles exp(-2 pi i k / NFFT) (float64 on the host, rounded once).  xengCdedispReset moves only the host's counts.
 * The output is a fixed function of the sample stream and the table: bit-identical whatever ntime, however the stream falls on
 * calls, after a Reset as in a fresh context, and whatever else runs on the GPU.  A non-finite input sample makes the blocks of
 * its own row that contain it non-finite and changes no other word.
 * Rejected at Initialize, before any device is touched: a non-positive size, pairs outside [0, nbeam/2), nfft not a power of two
 * in 2^8..2^13, overlap odd, negative or above nfft/2, nchan*2*npair > 65535, an input or a state above
 * XENG_CDEDISP_MAX_STATE_BYTES; after the device is known, an LDS need above what a work-group may take.  Rejected by SetChirp: a
 * NULL table, a non-finite word.  Rejected by Run without a launch: a NULL input or result, a misaligned pointer, a NULL output on
 * a call that completes a block.  Every call without a context: XENG_STATUS_INVALID_STATE. */
#define XENG_CDEDISP_MAX_STATE_BYTES (1LL << 32)
int xengCdedispInitialize(int gpu, int nchan, int nbeam, int ntime, int pair0, int npair, int nfft, int overlap);
/* table: cf32[npair][nchan][nfft] on the host (see above).  Waits for the context's work in flight, uploads the table and does not
 * touch the time buffer: it holds from the next block to complete. */
int xengCdedispSetChirp(const float *table);
/* enqueue only.  *nblocks is the number of blocks the call completes; the host's sample count decides it before anything is
 * enqueued, and out_dev is written for those blocks only.  out_dev may be NULL on a call that completes none. */
int xengCdedispRun(const void *in_dev, void *out_dev, int *nblocks);
/* host state only, nothing is launched and nothing cleared: the next input sample counts as sample 0 */
int xengCdedispReset(void);
/* the step L, the most blocks one call completes, samples taken and blocks completed since the last reset */
int xengCdedispGetInfo(int *step, int *max_blocks_per_call, long long *nsamples_since_reset, long long *nblocks_since_reset);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengCdedispCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengCdedispMark(unsigned long long *ticket);
int xengCdedispWait(unsigned long long ticket);
int xengCdedispTicketDone(unsigned long long ticket, int *done);
int xengCdedispSync(void);
int xengCdedispDestroy(void);

/* ---------------------------------------------------------------- Coherent dedispersion with long transforms
 * BeamCoherentDedisperseLong (no reference counterpart): xengCdedisp* for transforms of 2^14 to 2^20 points, which no work-group's
 * LDS holds -- the sweeps of the band below about 47 MHz at the DMs of known pulsars.  A second engine beside xengCdedisp*, which
 * stays what it is; a context of its own, independent of all others, whose kernels run on the beamformer's stream -- rings
 * declared 'beam' cover them, and xengBeamformSync waits for them too.  An ingest kernel per call (one more where a call straddles
 * a block boundary) and, per completed block, a four-step FFT through a scratch buffer in device memory: column transforms, the
 * overlap copy, row transforms with the table between them, column transforms (csrc/cdlong_kernels.h).
 *   in       cf32[nchan][nbeam][ntime], the output of xengBeamformRun unchanged; 16-byte aligned; never written.  ntime is fixed
 *            per context.  The selected beams are 2*pair0 .. 2*(pair0 + npair) - 1; a row is one (c, selected beam b),
 *            nrow = nchan * 2*npair.  Samples are counted from the last reset (xengCdlongReset, Initialize).
 *   sizes    NFFT = nfft, a power of two, 2^14 <= NFFT <= 2^20.  M = overlap: even, 0 <= M <= NFFT/2.  L = NFFT - M, the step.
 *   block    Block j covers the input samples [j*L, j*L + NFFT) and runs in the call that brings its last sample.  Per row:
 *              X[k] = sum_n x[n] * exp(-2 pi i k n / NFFT),  Y[k] = X[k] * T[p][c][k],  y[n] = sum_k Y[k] * exp(+2 pi i k n / NFFT)
 *            with p = b div 2 (both beams of a pair share a filter) and nothing else scaled: the table carries the 1/NFFT.  The
 *            block's output is y[M/2 .. M/2 + L): output sample i of the stream is input sample i + M/2, and the blocks tile the
 *            time axis without a gap.  fp32, held to a tolerance; no atomics, one owner per word.
 *   out      cf32[nblk][nchan][2*npair][L], one unit per block the call completes, 16-byte aligned; nothing past nblk units is
 *            written.  A call completes at most ceil(ntime / L) blocks (xengCdlongGetInfo).
 *   table    per pair, cf32[nchan][NFFT] on the host in natural DFT order: bin k is the offset k*D/NFFT from the channel's centre
 *            for k < NFFT/2 and (k - NFFT)*D/NFFT above, D the channel width.  The upload is pair by pair: the whole table of 96
 *            channels x 16 pairs at 2^17 points is 1.6 GB, and twice that in the float64 it is built from.  After Initialize it is
 *            1/NFFT everywhere: a pure latency of M/2 samples.
 *   state    between two guard bands of 64 KiB: the time buffer cf32[nrow][NFFT], the scratch buffer cf32[nrow][NFFT], the table
 *            cf32[npair][nchan][NFFT] (in the kernels' order) and the twiddles exp(-2 pi i k / n) for n = NFFT and its two factors
 *            (float64 on the host, rounded once).  xengCdlongReset moves only the host's counts.
 * The output is a fixed function of the sample stream and the table: bit-identical whatever ntime, however the stream falls on
 * calls, after a Reset as in a fresh context, and whatever else runs on the GPU.  A non-finite input sample makes the blocks of
 * its own row that contain it non-finite and changes no other word.
 * Rejected at Initialize, before any device is touched: a non-positive size, pairs outside [0, nbeam/2), nfft not a power of two
 * in 2^14..2^20 (2^13 and 2^21 among them), overlap odd, negative or above nfft/2, nchan*2*npair > 65535, an input or a state
 * above XENG_CDLONG_MAX_STATE_BYTES; after the device is known, an LDS need (64 KiB at most) above what a work-group may take.
 * Rejected by SetChirp: a NULL table, a pair outside [0, npair), a non-finite word.  Rejected by Run without a launch: a NULL input
 * or result, a misaligned pointer, a NULL output on a call that completes a block.  Every call without a context:
 * XENG_STATUS_INVALID_STATE. */
#define XENG_CDLONG_MAX_STATE_BYTES (1LL << 35)
int xengCdlongInitialize(int gpu, int nchan, int nbeam, int ntime, int pair0, int npair, int nfft, int overlap);
/* table: cf32[nchan][nfft] on the host, the filter of pair `pair` (0 <= pair < npair; see above).  Waits for the context's work in
 * flight, uploads the pair's table and does not touch the time buffer: it holds from the next block to complete. */
int xengCdlongSetChirp(int pair, const float *table);
/* enqueue only.  *nblocks is the number of blocks the call completes; the host's sample count decides it before anything is
 * enqueued, and out_dev is written for those blocks only.  out_dev may be NULL on a call that completes none. */
int xengCdlongRun(const void *in_dev, void *out_dev, int *nblocks);
/* host state only, nothing is launched and nothing cleared: the next input sample counts as sample 0 */
int xengCdlongReset(void);
/* the step L, the most blocks one call completes, samples taken and blocks completed since the last reset */
int xengCdlongGetInfo(int *step, int *max_blocks_per_call, long long *nsamples_since_reset, long long *nblocks_since_reset);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengCdlongCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengCdlongMark(unsigned long long *ticket);
int xengCdlongWait(unsigned long long ticket);
int xengCdlongTicketDone(unsigned long long ticket, int *done);
int xengCdlongSync(void);
int xengCdlongDestroy(void);

/* ---------------------------------------------------------------- Dirty images of the fine-channel visibilities
 * UpchanImage (no reference counterpart: the reference writes its visibilities to disk): the direct Fourier sum of UpchanCorr's
 * matrix over a list of directions -- the matrix beamformed onto every pixel, exact for a non-coplanar array, no grid and no FFT.
 * The library knows nothing of the array or the sky: blocks/imaging.py builds the delays.  A context of its own, independent of
 * all others, whose kernel runs on the beamformer's stream -- rings declared 'beam' cover it, and xengBeamformSync waits for it
 * too.  One kernel per call (csrc/image_kernels.h).
 *   vis      cf32[nfine][nstand][2][nstand][2], the output of xengUpchanCorrDump unchanged (the full Hermitian matrix, two
 *            polarisations per stand), V[c][s p][t q]; 16-byte aligned; never written
 *   freq     f64[nfine], Hz;  tau f64[npix][nstand], seconds;  w f32[nstand], finite and >= 0 (after Initialize: all 1);  autos
 *            (after Initialize: 0);  nfavg, which divides nfine: channel group g is the channels [g*nfavg, (g+1)*nfavg)
 *   out      f32[nfine/nfavg][4][npix], the words [XX, YY, Re(XY), Im(XY)] (the four-word convention of the power beams);
 *            16-byte aligned; nothing past it is written
 *              I_pq[g][x] = norm * sum_{c in group g, ascending} sum_{s,t} conj(b_s(c,x)) * V[c][s p][t q] * b_t(c,x)
 *              b_s(c,x)   = w_s * exp(-2 pi i * frac(freq[c] * tau[x][s]))
 *            XX = Re I_00, YY = Re I_11 (their imaginary parts are rounding noise and are dropped), XY = I_01.
 *   phase    freq*tau and its reduction to a fraction of a turn in [-1/2, 1/2] (the product rounded, minus its nearest integer)
 *            are fp64 on the device; the sine and cosine of the fraction and everything after them are fp32.
 *   autos    with autos = 0 the 2x2 blocks s = t read as zero: an exact omission, not a subtraction.
 *   flags    a stand with w_s = 0 is NOT READ: its rows and columns count as zero even where they hold NaN or Inf (a select on
 *            the load, not a multiply).
 *   norm     1 / (nfavg * sum_{s,t} w_s w_t), over s != t with autos = 0: float64 on the host, rounded once and applied as one
 *            final multiply.  A unit point source at a pixel (V = a a^H, a_s = exp(-2 pi i freq tau[x0][s]), both
 *            polarisations) reads 1 there.
 * Every output word is a fixed function of vis and the tables: no atomics, one owner per word, one summation order (the stands s
 * in ascending order on f32-input MFMAs, two per instruction; the stands t in tiles of 32, a wave's tiles in ascending order,
 * the channels of the group in ascending order; one fixed tree over the 32 columns of a tile; the four waves in order).  It
 * does not depend on what else runs on the GPU, nor on which other pixels are in the list: the image of a sub-list equals the
 * corresponding words of the full image bit for bit.  A NaN in the visibilities of a stand that is read stays within its channel
 * group.
 * The state (freq, tau, w) sits between two guard bands of 64 KiB.  SetGeometry and SetWeights wait for the context's work in
 * flight: a call between two Runs applies to the later one only.
 * Rejected at Initialize, before any device is touched: a non-positive size, nfavg not dividing nfine, nstand >
 * XENG_IMAGE_MAX_NSTAND (the steering tile of 32 pixels lives in LDS), more than 65535 channel groups, npix > 2^24, a delay table
 * above XENG_IMAGE_MAX_STATE_BYTES.  Rejected by SetGeometry: NULL, a non-finite word.  Rejected by SetWeights: NULL, a negative
 * or non-finite weight, weights that leave no pair (all zero; with autos = 0, fewer than two stands).  Rejected by Run without a
 * launch: NULL or misaligned pointers (INVALID_ARGUMENT); no geometry yet, or a single stand with the initial autos = 0
 * (INVALID_STATE).  Every call without a context: XENG_STATUS_INVALID_STATE. */
#define XENG_IMAGE_MAX_NSTAND 512
#define XENG_IMAGE_MAX_STATE_BYTES (1LL << 31)
int xengImageInitialize(int gpu, int nstand, int nfine, int nfavg, int npix);
/* the live context's number of channel groups, the pixels per work-group, the LDS bytes of a work-group and norm (float64) */
int xengImageGetInfo(int *ngroup, int *pixel_tile, int *lds_bytes, double *norm);
/* tau: f64[npix][nstand] seconds, freq: f64[nfine] Hz, on the host.  Waits for the context's work in flight, uploads both. */
int xengImageSetGeometry(const double *tau, const double *freq);
/* w: f32[nstand] on the host.  Waits for the context's work in flight; holds from the next Run. */
int xengImageSetWeights(const float *w, int autos);
/* enqueue only: one integration */
int xengImageRun(const void *vis_dev, void *out_dev);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengImageCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengImageMark(unsigned long long *ticket);
int xengImageWait(unsigned long long ticket);
int xengImageTicketDone(unsigned long long ticket, int *done);
int xengImageSync(void);
int xengImageDestroy(void);

/* ---------------------------------------------------------------- Per-stand gains from the fine-channel visibilities
 * UpchanGainCal (no reference counterpart: the reference leaves calibration to offline packages that read its visibility files):
 * one complex gain per (fine channel, polarisation, stand) from UpchanCorr's matrix and a point-source sky model, by StEFCal
 * (Salvini & Wijnholds 2014).  The library knows nothing of the array or the sky: blocks/imaging.py builds the delays of the
 * sources' directions.  A context of its own, independent of all others, whose kernel runs on the beamformer's stream -- rings
 * declared 'beam' cover it, and xengBeamformSync waits for it too.  One kernel per call, the whole iteration inside it
 * (csrc/gaincal_kernels.h).
 *   vis      cf32[nfine][nstand][2][nstand][2], the output of xengUpchanCorrDump unchanged; 16-byte aligned; never written.  Per
 *            fine channel c and polarisation p only the pp block is used, and it is read along its rows:
 *              X[s][t] = conj(vis[c][t p][s p]),   which is V[c][s p][t p] of a Hermitian matrix (UpchanCorr's is, bit for bit)
 *            under the conjugation convention by which a unit point source (V = a a^H) images to 1 with xengImage*.
 *   model    tau f64[nsrc][nstand] seconds, freq f64[nfine] Hz, flux F f32[nfine][nsrc], finite and >= 0:
 *              M_c[s][t] = sum_k F[c][k] * a_ks * conj(a_kt),   a_ks = exp(-2 pi i * frac(freq[c] * tau[k][s]))
 *            freq*tau and its reduction to a fraction of a turn in [-1/2, 1/2] are fp64 on the device; sincospif of the fraction and
 *            everything after it are fp32.  The matrix M is never formed.
 *   weights  w f32[nstand], finite and >= 0.  A stand with w_s = 0 is NOT READ (a select on the load: it may hold NaN or Inf) and
 *            its gain is written as 0 + 0i.  The autos s = t are never read.
 *   solver   from g = 1 at every stand of weight > 0 (or the warm start below), for i = 1 .. niter:
 *              N_s = sum_k F_k conj(a_ks) * sum_{t != s} X[s][t] * (w_t g_t a_kt)
 *              D_s = sum_{t != s} w_t |g_t|^2 |M_c[s][t]|^2,  by the Gram route (the one route, in this summation order):
 *                    G[k][k'] = sum_t w_t |g_t|^2 conj(a_kt) a_k't                      over all t in ascending order
 *                    D_s = sum_k Re( z_k * sum_k' G[k][k'] conj(z_k') ) - w_s |g_s|^2 (sum_k F_k)^2,    z_k = F_k a_ks,
 *                    k and k' ascending, the t = s term removed by one final subtraction
 *              g_s <- N_s / D_s, and g_s = 0 where D_s is not > 0.
 *            On even i, delta = ||g_i - g_(i-1)|| / ||g_i|| over the stands of weight > 0.  With tol > 0 and delta <= tol the loop
 *            stops there (converged); otherwise g_i <- (g_i + g_(i-1)) / 2.  With tol = 0 exactly niter iterations run.
 *   phase    after the loop every gain of the (channel, pol) is multiplied by conj(g_ref) / |g_ref| of the reference stand refant
 *            (left as they are where |g_ref| is not > 0).
 *   gains    cf32[nfine][2][nstand]; 8-byte aligned
 *   stats    f32[nfine][2][4] = {iterations run, the last delta (-1: none was formed), stands solved (weight > 0 and a gain that is
 *            not 0), converged 0/1}
 *   warm     the context keeps, per (channel, pol), the last solution before its phase reference and whether it was converged and
 *            finite.  Run(.., warm = 1) starts from it where it was, else from 1.  A Run with niter = 0 returns its start, phase
 *            referenced, and leaves the kept solution alone.  SetModel, SetWeights and Initialize forget it.
 * Every output word is a fixed function of its own channel's block of vis, the model and the weights: no atomics, one owner per
 * word, one summation order (N: the stands t in ascending order on f32-input MFMAs, two per instruction, then the sources in
 * ascending order per half of the tile's rows, the halves added; delta: a thread's stands, one fixed tree over the wave, the four
 * waves in order).  It does not depend on what else runs on the GPU nor on which other channels are in the call.  A NaN in the
 * visibilities of a stand that is read stays within its (channel, pol).
 * The state sits between two guard bands of 64 KiB.  SetModel and SetWeights wait for the context's work in flight: a call
 * between two Runs applies to the later one only; SetSolver sets the arguments of the Runs after it.
 * Rejected with INVALID_ARGUMENT at the call that sees it: a non-positive size, nsrc > XENG_GAINCAL_MAX_NSRC, nstand >
 * XENG_GAINCAL_MAX_NSTAND, more than 65535 channels (Initialize); NULL, a non-finite word, a negative flux (SetModel); NULL, a
 * negative or non-finite weight, refant out of range or of weight 0 (SetWeights); niter outside [0, XENG_GAINCAL_MAX_NITER], a
 * negative or non-finite tol (SetSolver); NULL or misaligned pointers (Run).  Run before SetModel or before SetWeights, and every
 * call without a context: XENG_STATUS_INVALID_STATE. */
#define XENG_GAINCAL_MAX_NSRC 32
#define XENG_GAINCAL_MAX_NSTAND 512
#define XENG_GAINCAL_MAX_NITER 1024
#define XENG_GAINCAL_DEFAULT_NITER 60
#define XENG_GAINCAL_DEFAULT_TOL 1e-5
int xengGaincalInitialize(int gpu, int nstand, int nfine, int nsrc);
/* the LDS bytes of a work-group, the solver's niter and tol, the reference stand */
int xengGaincalGetInfo(int *lds_bytes, int *niter, double *tol, int *refant);
/* tau: f64[nsrc][nstand] seconds, freq: f64[nfine] Hz, flux: f32[nfine][nsrc], on the host.  Waits for the context's work in flight. */
int xengGaincalSetModel(const double *tau, const double *freq, const float *flux);
/* w: f32[nstand] on the host.  Waits for the context's work in flight; holds from the next Run. */
int xengGaincalSetWeights(const float *w, int refant);
/* after Initialize: XENG_GAINCAL_DEFAULT_NITER, XENG_GAINCAL_DEFAULT_TOL */
int xengGaincalSetSolver(int niter, double tol);
/* enqueue only: one integration */
int xengGaincalRun(const void *vis_dev, void *gains_dev, void *stats_dev, int warm);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengGaincalCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengGaincalMark(unsigned long long *ticket);
int xengGaincalWait(unsigned long long ticket);
int xengGaincalTicketDone(unsigned long long ticket, int *done);
int xengGaincalSync(void);
int xengGaincalDestroy(void);

/* ---------------------------------------------------------------- Calibrated, source-subtracted visibilities
 * UpchanCalApply (no reference counterpart: the reference leaves calibration and source subtraction to offline packages): UpchanCorr's
 * matrix with a gain solution applied and a point-source model taken out, written as a matrix of the same format, so that
 * xengImage* and a second xengGaincal* (a residual solve) read it unchanged.  The library knows nothing of the array or the sky:
 * blocks/imaging.py builds the delays, blocks/calibration.py (inverse_gains) the factors.  A context of its own, independent of
 * all others, whose kernels run on the beamformer's stream -- rings declared 'beam' cover it, and xengBeamformSync waits for it
 * too.  One kernel per Run (csrc/calapply_kernels.h), one more per SetModel.
 *   vis      cf32[nfine][nstand][2][nstand][2], the output of xengUpchanCorrDump unchanged, V[c][s p][t q]; 16-byte aligned; never
 *            written.  With row i = 2 s + p and column j = 2 t + q only the words i >= j are read: the upper triangle may hold
 *            anything.
 *   model    tau f64[nsrc][nstand] seconds, freq f64[nfine] Hz, flux F f32[nfine][nsrc], finite and >= 0, 0 <= nsrc <=
 *            XENG_CALAPPLY_MAX_NSRC:
 *              M_c[s][t] = sum_k F[c][k] * a_ks * conj(a_kt),   a_ks = exp(-2 pi i * frac(freq[c] * tau[k][s]))
 *            freq*tau and its reduction to a fraction of a turn in [-1/2, 1/2] are fp64 on the device; sincospif of the fraction and
 *            everything after it are fp32 (the convention of xengImage* and xengGaincal*).  The factors a are formed once per
 *            SetModel, not once per Run: the same words.  z_ks = F_k * a_ks is one fp32 multiply per part; per word of M and per part
 *            one chain of fused multiply-adds on f32-input MFMAs, the sources two per instruction in ascending order: of each pair
 *            first Re z Re a (k even, k odd), then Im z Im a (k even, k odd) for the real part; Im z Re a, then -Re z Im a for the
 *            imaginary part.  With nsrc = 0 there is no model (calibration only): tau and flux may be NULL and Run needs no SetModel.
 *   factors  h cf32[nfine][2][nstand], finite; after Initialize every factor is 1.  h_i of input i = 2 s + p is h[c][p][s].  h = 0
 *            marks a (stand, polarisation) that is left out.  The device divides nothing: the host forms h = 1 / g in float64
 *            (blocks/calibration.py inverse_gains) and rounds once.
 *   out      cf32 in vis's layout; 16-byte aligned; nothing past it is written.
 *              i > j:  out[c][i][j] = (h_i * conj(h_j)) * V[c][i][j] - delta_pq * M_c[s][t]
 *                      w = h_i conj(h_j):  Re w = fma(Re h_i, Re h_j, Im h_i Im h_j),  Im w = fma(Im h_i, Re h_j, -(Re h_i Im h_j))
 *                      y = w V          :  Re y = fma(Re w, Re V, -(Im w Im V)),       Im y = fma(Re w, Im V, Im w Re V)
 *                      then M is subtracted, part by part, where p = q.  No other contraction is taken.
 *              i = j:  the real part of the same expression; the imaginary part is written as +0.
 *              i < j:  the conjugate of out[c][j][i]: the same word with the sign of its imaginary part turned, not computed again
 *                      (xengUpchanCorrDump's convention), so the output is Hermitian bit for bit.
 *            With unit factors and nsrc = 0 the lower triangle is the input bit for bit (up to the sign of a zero).
 *   flags    a word whose h_i or h_j is 0 is NOT READ (a select on the load: it may hold NaN or Inf) and is written as +0 + 0i,
 *            in both triangles.  A NaN in a word that is read stays in that word and its mirror.
 * Every output word is a fixed function of its own input word, the two factors and the model: one owner per Hermitian pair, no
 * atomics, one summation order.  It does not depend on nstand, on which other channels are in the call nor on what else runs on
 * the GPU.
 * The state (freq, tau, a, h, flux) sits between two guard bands of 64 KiB.  SetModel and SetFactors wait for the context's work in
 * flight: a call between two Runs applies to the later one only.
 * Rejected with INVALID_ARGUMENT at the call that sees it: a non-positive nstand or nfine, a negative nsrc, nsrc >
 * XENG_CALAPPLY_MAX_NSRC, nstand > XENG_CALAPPLY_MAX_NSTAND, more than 65535 channels (Initialize); NULL frequencies, with nsrc > 0
 * NULL delays or fluxes, a non-finite word, a negative flux (SetModel); NULL, a non-finite word (SetFactors); NULL or misaligned
 * pointers (Run).  Run before SetModel with nsrc > 0, and every call without a context: XENG_STATUS_INVALID_STATE. */
#define XENG_CALAPPLY_MAX_NSRC 32
#define XENG_CALAPPLY_MAX_NSTAND 512
int xengCalapplyInitialize(int gpu, int nstand, int nfine, int nsrc);
/* the tiles of 32 stands per side, the work-groups of a Run, the LDS bytes of a work-group, the bytes of a span (input = output) */
int xengCalapplyGetInfo(int *ntile, int *ngroup, int *lds_bytes, long long *span_bytes);
/* tau: f64[nsrc][nstand] seconds, freq: f64[nfine] Hz, flux: f32[nfine][nsrc], on the host.  Waits for the context's work in flight. */
int xengCalapplySetModel(const double *tau, const double *freq, const float *flux);
/* h: cf32[nfine][2][nstand] on the host.  Waits for the context's work in flight; holds from the next Run. */
int xengCalapplySetFactors(const void *h);
/* enqueue only: one integration */
int xengCalapplyRun(const void *vis_dev, void *out_dev);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengCalapplyCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengCalapplyMark(unsigned long long *ticket);
int xengCalapplyWait(unsigned long long ticket);
int xengCalapplyTicketDone(unsigned long long ticket, int *done);
int xengCalapplySync(void);
int xengCalapplyDestroy(void);

/* ---------------------------------------------------------------- Direction-dependent gains and peeling
 * UpchanPeel (no reference counterpart: the reference leaves calibration and source subtraction to offline packages): one complex
 * gain per (fine channel, polarisation, direction, stand) for ndir <= XENG_PEEL_MAX_NDIR bright point sources, solved per
 * integration, and each source taken out of the matrix with its own gains; the result is a matrix of the same format, so that
 * xengImage*, xengGaincal* and a further xengCalapply* read it unchanged.  The input is normally xengCalapply*'s output: the
 * iteration below converges from gains near 1 (amplitude 1 +- 0.2, phases of half a radian) and diverges from gains of arbitrary
 * phase, so uncalibrated data are not its input.  The library knows nothing of the array or the sky: blocks/imaging.py builds the
 * delays.  A context of its own, independent of all others, whose kernels run on the beamformer's stream -- rings declared 'beam'
 * cover it, and xengBeamformSync waits for it too.  Two kernels per Run (csrc/peel_kernels.h), one more per SetModel.
 * The conventions are those of xengGaincal*:
 *   vis      cf32[nfine][nstand][2][nstand][2], 16-byte aligned, never written.  The solve uses, per fine channel c and polarisation p,
 *            only the pp block, read along its rows: X[s][t] = conj(vis[c][t p][s p]).  The subtraction reads the words i >= j (row i
 *            = 2 s + p, column j = 2 t + q).
 *   model    tau f64[ndir][nstand] seconds, freq f64[nfine] Hz, flux F f32[nfine][ndir], finite and >= 0:
 *              a_ds = exp(-2 pi i * frac(freq[c] * tau[d][s]))
 *            freq*tau and its reduction to a fraction of a turn in [-1/2, 1/2] are fp64 on the device; sincospif of the fraction and
 *            everything after it are fp32.  The factors are formed once per SetModel.  A direction with F_d = 0 is off: its gains
 *            are 0 and it takes no part.  The directions are solved in the order given (the brightest first); nothing is sorted.
 *   weights  w f32[nstand], finite and >= 0.  A stand with w_s = 0 is NOT LOADED by the solve (a select on the load: it may hold NaN
 *            or Inf) and all its gains are written as 0 + 0i.  The autos s = t never enter the solve.
 *   solver   V[s][t] ~ sum_d F_d u_ds conj(u_dt), u_ds = g_ds a_ds.  From g = 1 at every live (direction, stand) (or the warm start
 *            below), for i = 1 .. niter one sweep:
 *              1. for all directions at once, from the gains at the start of the sweep: Y[d][s] = sum_{t != s} X[s][t] * w_t u_dt,
 *                 the only pass over V in a sweep;
 *              2. for d ascending (Gauss-Seidel over the directions), with u~_e the new u_e for e < d and the sweep's old u_e for e > d:
 *                   G_e = sum_t w_t conj(u~_et) u_dt over all t,  P = sum_t w_t |u_dt|^2
 *                   N_s = Y[d][s] - sum_{e != d} F_e u~_es (G_e - w_s conj(u~_es) u_ds),  e ascending
 *                   g'_ds = conj(a_ds) N_s / (F_d (P - w_s |u_ds|^2)),  and 0 where the denominator is not > 0 or w_s = 0
 *                 which is the StEFCal step of direction d on V - sum_{e != d} F_e u~_e u~_e^H, that matrix never formed;
 *              3. on odd i, g <- g'.  On even i, delta = ||g' - g|| / ||g'|| over all live (direction, stand); with tol > 0 and
 *                 delta <= tol the loop stops with g <- g' (converged); otherwise g <- (g' + g) / 2.
 *            The simultaneous (Jacobi) update of all directions diverges from 4 directions on; this order converged in every case tried.
 *   phase    after the loop every direction's gains are multiplied by conj(g_d,ref) / |g_d,ref| of the reference stand refant (left
 *            as they are where |g_d,ref| is not > 0).  The subtraction does not depend on it.
 *   gains    cf32[nfine][2][ndir][nstand]; 8-byte aligned
 *   stats    f32[nfine][2][4] = {sweeps run, the last delta (-1: none was formed), stands solved (weight > 0 and a gain that is not 0
 *            in every direction that is on), converged 0/1}
 *   out      cf32 in vis's layout; 16-byte aligned; not the input; nothing past it is written.  From the gains just written:
 *              i > j:  out[c][s p][t q] = V[c][s p][t q] - delta_pq * sum_d (F_d u_ds) conj(u_dt); a word of a cross hand is the
 *                      input's, bit for bit
 *              i = j:  the real part of the same expression; the imaginary part is written as +0
 *              i < j:  the conjugate of out[c][j][i], not computed again: the output is Hermitian bit for bit.
 *            The rows and columns of a stand of weight 0 have u = 0: they pass through unchanged.
 *   warm     the context keeps, per (channel, pol), the last solution before its phase reference and whether it was converged and
 *            finite.  Run(.., warm = 1) starts from it where it was, else from 1.  A Run with niter = 0 returns its start, phase
 *            referenced, and leaves the kept solution alone.  SetModel, SetWeights and Initialize forget it.
 * Every word is a fixed sum: no atomics, one owner per word, one summation order.  A solution depends on its own (channel, pol) block
 * of vis, the model and the weights only; it does not depend on what else runs on the GPU nor on which other channels are in the
 * call.  A NaN in the visibilities of a stand that is read stays within its (channel, pol), which ends unconverged.
 * The state sits between two guard bands of 64 KiB.  SetModel and SetWeights wait for the context's work in flight: a call between
 * two Runs applies to the later one only; SetSolver sets the arguments of the Runs after it.
 * Rejected with INVALID_ARGUMENT at the call that sees it: a non-positive size, ndir > XENG_PEEL_MAX_NDIR, nstand >
 * XENG_PEEL_MAX_NSTAND, more than 65535 channels (Initialize); NULL, a non-finite word, a negative flux (SetModel); NULL, a negative
 * or non-finite weight, refant out of range or of weight 0 (SetWeights); niter outside [0, XENG_PEEL_MAX_NITER], a negative or
 * non-finite tol (SetSolver); NULL or misaligned pointers, out = vis (Run).  Run before SetModel or before SetWeights, and every call
 * without a context: XENG_STATUS_INVALID_STATE. */
#define XENG_PEEL_MAX_NDIR 8
#define XENG_PEEL_MAX_NSTAND 512
#define XENG_PEEL_MAX_NITER 1024
#define XENG_PEEL_DEFAULT_NITER 60
#define XENG_PEEL_DEFAULT_TOL 1e-5
int xengPeelInitialize(int gpu, int nstand, int nfine, int ndir);
/* the LDS bytes of a work-group of the solve, the solver's niter and tol, the reference stand, the bytes of a span (input = output) */
int xengPeelGetInfo(int *lds_bytes, int *niter, double *tol, int *refant, long long *span_bytes);
/* tau: f64[ndir][nstand] seconds, freq: f64[nfine] Hz, flux: f32[nfine][ndir], on the host.  Waits for the context's work in flight. */
int xengPeelSetModel(const double *tau, const double *freq, const float *flux);
/* w: f32[nstand] on the host.  Waits for the context's work in flight; holds from the next Run. */
int xengPeelSetWeights(const float *w, int refant);
/* after Initialize: XENG_PEEL_DEFAULT_NITER, XENG_PEEL_DEFAULT_TOL */
int xengPeelSetSolver(int niter, double tol);
/* enqueue only: one integration */
int xengPeelRun(const void *vis_dev, void *out_dev, void *gains_dev, void *stats_dev, int warm);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengPeelCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengPeelMark(unsigned long long *ticket);
int xengPeelWait(unsigned long long ticket);
int xengPeelTicketDone(unsigned long long ticket, int *done);
int xengPeelSync(void);
int xengPeelDestroy(void);

/* ---------------------------------------------------------------- Hogbom CLEAN of the dirty images
 * UpchanClean (no reference counterpart: the reference leaves imaging and deconvolution to offline packages): Hogbom's CLEAN of the
 * images of xengImage*, per channel group, with the imager's EXACT point-spread function -- the imaging is a direct Fourier sum
 * over a free list of directions, so the response of pixel x to a unit source at pixel x0 is a closed form, the same for all four
 * words.  A context of its own, independent of all others, whose kernel runs on the beamformer's stream -- rings declared 'beam'
 * cover it, and xengBeamformSync waits for it too.  niter + 2 launches of one kernel per Run (csrc/clean_kernels.h); nothing is
 * read back, and no work-group waits for another.
 *   image    f32[ngroup][4][npix], the words [XX, YY, Re(XY), Im(XY)]: the output of xengImageRun, or the residual of an earlier
 *            xengCleanRun (cleaning deeper); 16-byte aligned; never written.  ngroup = nfine / nfavg.
 *   tables   those of xengImage*: freq f64[nfine] Hz; tau f64[npix][nstand] s; w f32[nstand], finite and >= 0 (after Initialize: all
 *            1); autos (after Initialize: 0).  They must be the ones the image was made with.
 *            norm = 1 / (nfavg * sum_{s,t} w_s w_t), over s != t with autos = 0, float64 on the host, rounded once.
 *   PSF      PSF_g(x, x0) = norm * sum_{c in group g, ascending} ( |S_c(x, x0)|^2 - D )
 *            S_c(x, x0)   = sum_s w_s * exp(+2 pi i * (fr_c(x,s) - fr_c(x0,s)))
 *            fr_c(x,s)    = freq[c]*tau[x][s] (the fp64 product, rounded) minus its nearest integer: xengImage*'s rule
 *            D            = sum_s w_s^2 with autos = 0 (float64 on the host, rounded once), else 0
 *            The difference of the two fractions is fp64; its conversion to fp32, sincospif of it and everything after are fp32:
 *              Re S = fma(w_s, cos, Re S), Im S = fma(w_s, sin, Im S), the stands in ascending order;
 *              p_c = fma(Re S, Re S, Im S * Im S) - D;  acc = acc + p_c, the channels of the group in ascending order;  PSF = norm * acc.
 *            It is real, PSF_g(x0, x0) = 1 up to rounding, and a stand with w_s = 0 contributes nothing: its tau is never turned
 *            into a phase.
 *   window   mask u8[npix]: components are searched among the pixels with mask != 0 only (after Initialize: every pixel); every
 *            pixel of the list, in or out of the window, is subtracted from.
 *   control  niter in [0, niter_max], gain in (0, 1], threshold >= 0, fraction >= 0 (after Initialize: niter_max, 0.1, 0, 0)
 *   loop     per channel group, R a copy of the image, k = 0, 1, ...:
 *              1. x_k = the window pixel that maximises |I(x)|, I = R[0][x] + R[1][x] (one fp32 add); strict >, ascending pixels: a
 *                 tie goes to the lowest index; a non-finite I never wins
 *              2. stop with reason 2 if no pixel won (an empty window, or no finite I in it); with reason 1 if
 *                 |I(x_k)| <= max(threshold, fraction * |I(x_0)|) (an fp32 product; x_0 the first peak of THIS Run); with reason 0 if
 *                 k = niter -- tested in this order
 *              3. component k: the pixel, I(x_k) and C_j = gain * R[j][x_k] (one fp32 multiply per word j); then at every pixel
 *                 R[j][x] = fma(-C_j, PSF_g(x, x_k), R[j][x])
 *   out      one span, 16-byte aligned; nothing past it is written:
 *              0             f32[ngroup][4][npix], the residual: the format of the input
 *              comp_offset   [ngroup][niter][8] 32-bit words {i32 pixel, f32 I(x_k), f32 C_XX, C_YY, C_Re, C_Im, +0, +0}; the records
 *                            past ncomp hold pixel -1 and +0
 *              stats_offset  [ngroup][4] 32-bit words {i32 ncomp, i32 reason, f32 peak, 0}: peak = |I| of the residual's peak in the
 *                            window (reasons 0 and 1), +0 (reason 2)
 *            comp_offset = 16 ngroup npix, stats_offset = comp_offset + 32 ngroup niter, span_bytes = stats_offset + 16 ngroup: they
 *            follow the niter of SetControl (GetInfo reports them for the current one).
 *   NaN      a pixel whose I is not finite is never a component; the subtraction leaves its NaN where it is.  A component whose
 *            own XY words are NaN (I is XX + YY: it can still win) turns those words of its group NaN at every pixel.  A group with no
 *            finite I in the window stops with reason 2 and its residual is the input bit for bit.  Nothing crosses from one channel
 *            group to another.
 * Every output word is a fixed function of the image, the tables and the controls: no atomics, one owner per word, one summation
 * order.  A pixel's residual words depend on its own row of tau and the component list only, not on which other pixels share its
 * work-group: a sub-list of the pixels that holds the whole window, in the same order, gives the same words bit for bit.  Nothing
 * depends on what else runs on the GPU.  Run(niter = a) followed by a Run on its residual with niter = b and fraction = 0 gives the
 * residual and the records of Run(niter = a + b).
 * The state (freq, tau transposed, w, mask, the launches' hand-over buffers) sits between two guard bands of 64 KiB.  SetGeometry,
 * SetWeights and SetWindow wait for the context's work in flight: a call between two Runs applies to the later one only;
 * SetControl sets the arguments of the Runs after it.
 * Rejected with INVALID_ARGUMENT at the call that sees it, before any device is touched: a non-positive size, nfavg not dividing
 * nfine, niter_max outside [1, XENG_CLEAN_MAX_NITER], nstand > XENG_CLEAN_MAX_NSTAND, more than 65535 channel groups, npix > 2^24, a
 * delay table above XENG_CLEAN_MAX_STATE_BYTES (Initialize); NULL, a non-finite word (SetGeometry); NULL, a negative or non-finite
 * weight, weights that leave no pair (SetWeights); niter outside [0, niter_max], gain outside (0, 1], a negative or non-finite
 * threshold or fraction (SetControl); NULL or misaligned pointers (Run).  Run before SetGeometry, or with a single stand and the
 * initial autos = 0, and every call without a context: XENG_STATUS_INVALID_STATE. */
#define XENG_CLEAN_MAX_NITER 4096
#define XENG_CLEAN_MAX_NSTAND 2048
#define XENG_CLEAN_MAX_STATE_BYTES (1LL << 31)
int xengCleanInitialize(int gpu, int nstand, int nfine, int nfavg, int npix, int niter_max);
/* the live context's number of channel groups, the pixels per work-group, the span's layout for the current niter, and norm (float64) */
int xengCleanGetInfo(int *ngroup, int *pixel_tile, long long *comp_offset, long long *stats_offset, long long *span_bytes, double *norm);
/* tau: f64[npix][nstand] seconds, freq: f64[nfine] Hz, on the host.  Waits for the context's work in flight, uploads both. */
int xengCleanSetGeometry(const double *tau, const double *freq);
/* w: f32[nstand] on the host.  Waits for the context's work in flight; holds from the next Run. */
int xengCleanSetWeights(const float *w, int autos);
/* mask: u8[npix] on the host, or NULL for every pixel.  Waits for the context's work in flight; holds from the next Run. */
int xengCleanSetWindow(const unsigned char *mask);
int xengCleanSetControl(int niter, float gain, float threshold, float fraction);
/* enqueue only: one image; image_dev is never written */
int xengCleanRun(const void *image_dev, void *out_dev);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengCleanCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengCleanMark(unsigned long long *ticket);
int xengCleanWait(unsigned long long ticket);
int xengCleanTicketDone(unsigned long long ticket, int *done);
int xengCleanSync(void);
int xengCleanDestroy(void);

/* ---------------------------------------------------------------- Outlier flags from the fine-channel visibilities
 * UpchanFlag (no reference counterpart: the reference leaves flagging to offline packages): robust per-(fine channel, polarisation,
 * stand) statistics from one pass over UpchanCorr's matrix, median / MAD outlier tests over the stands and over the channels, and a
 * mask from which blocks/flagging.py forms the per-stand weights of xengGaincal*, xengImage* and xengPeel* and the factors of
 * xengCalapply*.  A context of its own, independent of all others, whose kernels run on the beamformer's stream -- rings declared
 * 'beam' cover it, and xengBeamformSync waits for it too.  Three kernels per Run (csrc/flag_kernels.h).
 * Every integration stands alone: the context keeps nothing from one Run to the next, and there is no test along time.
 *   vis      cf32[nfine][nstand][2][nstand][2], the output of xengUpchanCorrDump or of xengCalapplyRun, V[c][s p][t q]; 16-byte aligned;
 *            never written.  With row i = 2 s + p and column j = 2 t + q only the words with i >= j and p = q contribute: the upper
 *            triangle and the cross hands may hold anything (neither is loaded).
 *   weights  w f32[nstand], finite and >= 0, used as on / off only; after Initialize all 1.  A stand with w_s = 0 is NOT READ (a select
 *            on the load: it may hold NaN or Inf).  At least 4 stands must stay.
 *   control  nsig_cross, nsig_auto, nsig_chan finite and >= 0 (0: that test is off), 0 <= wchan <= XENG_FLAG_MAX_WCHAN; after
 *            Initialize the XENG_FLAG_DEFAULT_* below.  The thresholds k = float32(nsig * 1.4826) are float64 products on the host,
 *            rounded once (1.4826 MAD = one sigma of a normal distribution).
 *   step 1   for every (c, p, s) with w_s > 0:
 *              A[c][p][s] = Re V[c][s p][s p]
 *              R[c][p][s] = sum over t != s with w_t > 0 of |V[c][s p][t p]|^2, the word read at [s p][t p] for t < s and at
 *                           [t p][s p] for t > s;  |z|^2 = fma(re, re, im * im)
 *            and +0 for both where w_s = 0.  The one summation order: the stands in tiles of 32 (tile K = the stands 32 K .. 32 K + 31,
 *            whatever nstand); a tile's partial is the sum of its terms from +0 in ascending t (a term that is left out adds +0); R
 *            is the sum of the partials from +0 in ascending K.  Plain fp32 adds, no atomics, one owner per word.  R and A do not
 *            depend on which other channels are in the call nor on what else runs on the GPU.  A non-finite word that is read makes
 *            the R (or, on the diagonal, the A) of its two stands in that (c, p) non-finite, and nothing else.
 *   step 2   per (c, p), exact in fp32.  L = the stands with w > 0 and finite R and A, n = |L|.  The median of n values sorted
 *            ascending, v[0 .. n-1], is v[n / 2] for odd n and 0.5f * (v[(n-1) / 2] + v[n / 2]) for even n.  For x in {R, A}:
 *              med = median_L(x);  d_s = |x_s - med| (one subtraction);  mad = median_L(d);
 *              stand s of L is an outlier where d_s > k_x * mad (one multiply, a strict compare), k_x > 0.
 *            With mad = 0 (more than half of L share one value) every stand with d_s > 0 is an outlier: the rule is kept as it
 *            stands, since a MAD of 0 between independent stands means test data or a broken digitiser, and both should show.
 *            If n < 4 no stand test is taken, the (c, p) is channel-flagged, has no y below, and med_R = mad_R = +0.
 *            y[c][p] = med_R.
 *   step 3   per p, over the channels that have a y.  b_c = the median of y over the channels of [c - wchan, c + wchan], clipped to
 *            [0, nfine), that have a y (c is one of them); with wchan = 0 the median over all of them.  r_c = y_c - b_c,
 *            m = the median of |r_c| over those channels; channel c is flagged where |r_c| > k_chan * m, k_chan > 0 (m = 0: as above).
 *            b = +0 for a channel without a y.
 *   mask     u8[nfine][2][nstand]: bit 0 cross-power outlier, bit 1 auto outlier, bit 2 channel flagged (on every stand of the
 *            (c, p), those of weight 0 included), bit 3 non-finite statistic (w > 0, R or A not finite: it is outside L), bit 4 weight 0
 *   stats    f32[nfine][2][nstand][2] = {R, A}; 4-byte aligned
 *   chan     f32[nfine][2][4] = {med_R, mad_R, b, n}; 4-byte aligned
 *            Nothing past any of the three is written.  Bits 0, 1, 3, 4, stats and chan[0, 1, 3] of a (c, p) depend on that (c, p)'s
 *            words only; bit 2 and b depend on the other channels of the call by definition.
 * The state (weights, the tiles' partial sums f32[nfine][2][nstand][ntile], the autos) sits between two guard bands of 64 KiB.
 * SetWeights and SetControl wait for the context's work in flight and hold from the next Run.
 * Rejected with INVALID_ARGUMENT at the call that sees it: a non-positive size, nstand < 4, nstand > XENG_FLAG_MAX_NSTAND, nfine >
 * XENG_FLAG_MAX_NFINE (the channel test's medians are taken in one work-group's LDS) (Initialize); NULL, a negative or non-finite
 * weight, fewer than 4 stands of weight > 0 (SetWeights); a negative or non-finite nsig, one whose threshold is not finite in
 * float32, wchan outside [0, XENG_FLAG_MAX_WCHAN] (SetControl); NULL results (GetInfo, GetControl, CheckGuards); NULL pointers, vis
 * not 16-byte or stats or chan not 4-byte aligned (Run).  Every call without a context: XENG_STATUS_INVALID_STATE. */
#define XENG_FLAG_MAX_NSTAND 512
#define XENG_FLAG_MAX_NFINE 8192
#define XENG_FLAG_MAX_WCHAN 64
#define XENG_FLAG_DEFAULT_NSIG_CROSS 6.0
#define XENG_FLAG_DEFAULT_NSIG_AUTO 6.0
#define XENG_FLAG_DEFAULT_NSIG_CHAN 6.0
#define XENG_FLAG_DEFAULT_WCHAN 0
int xengFlagInitialize(int gpu, int nstand, int nfine);
/* the bytes of mask, stats and chan, and the most LDS bytes a work-group of the three kernels takes */
int xengFlagGetInfo(long long *mask_bytes, long long *stats_bytes, long long *chan_bytes, int *lds_bytes);
/* w: f32[nstand] on the host.  Waits for the context's work in flight; holds from the next Run. */
int xengFlagSetWeights(const float *w);
/* Waits for the context's work in flight; holds from the next Run. */
int xengFlagSetControl(double nsig_cross, double nsig_auto, double nsig_chan, int wchan);
int xengFlagGetControl(double *nsig_cross, double *nsig_auto, double *nsig_chan, int *wchan);
/* enqueue only: one integration */
int xengFlagRun(const void *vis_dev, void *mask_dev, void *stats_dev, void *chan_dev);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengFlagCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengFlagMark(unsigned long long *ticket);
int xengFlagWait(unsigned long long ticket);
int xengFlagTicketDone(unsigned long long ticket, int *done);
int xengFlagSync(void);
int xengFlagDestroy(void);

/* ---------------------------------------------------------------- Component lists subtracted from the visibilities
 * UpchanPredict (no reference counterpart: the reference leaves deconvolution to offline packages): the visibility model of a list
 * of point components -- xengCleanRun's own records, or any catalogue -- taken out of UpchanCorr's matrix on all four polarisation
 * products, written as a matrix of the same format: the major cycle of a Cotton-Schwab CLEAN (xengImageRun of the output is
 * xengCleanRun's residual), and the subtraction of a sky catalogue of thousands of sources.  A context of its own, independent of all
 * others, whose kernels run on the beamformer's stream -- rings declared 'beam' cover it, and xengBeamformSync waits for it too.  One
 * kernel per Run (csrc/predict_kernels.h).
 *   vis         cf32[nfine][nstand][2][nstand][2], the output of xengUpchanCorrDump, xengCalapplyRun or xengPeelRun, V[c][s p][t q];
 *               16-byte aligned; never written.  With row i = 2 s + p and column j = 2 t + q only the words i >= j are read: the
 *               upper triangle may hold anything.
 *   geometry    tau f64[ndir][nstand] seconds -- the imager's pixel list or any catalogue (blocks/imaging.py steering_delays) --
 *               and freq f64[nfine] Hz, set once per context (SetGeometry).  ndir <= 2^24 and the table at most
 *               XENG_IMAGE_MAX_STATE_BYTES, as in xengImage*.
 *   components  records [ngroup][ncomp_max], ngroup = nfine / nfavg, 1 <= ncomp_max <= XENG_PREDICT_MAX_NCOMP (xengClean*'s niter
 *               cap), in xengCleanRun's own layout of 32 bytes (blocks/imaging.py CLEAN_COMPONENT): {pixel i32, I f32, C f32[4] =
 *               XX, YY, Re XY, Im XY, 8 bytes of padding} -- the component area of a Clean span can be handed over as it is.  pixel
 *               is an index into tau; pixel = -1 is an empty record: zero operands (z = 0, a = 0), its other words are not looked
 *               at.  I and the padding are ignored.  C must be finite and may be negative.  After Initialize every record is empty.
 *               SetComponents waits for the context's work in flight and holds from the next Run.
 *   model       for channel c of group g = c / nfavg, with a_ks = exp(-2 pi i * frac(freq[c] * tau[pixel_k][s])) -- freq*tau
 *               (__dmul_rn) and its reduction to a fraction of a turn in [-1/2, 1/2] fp64, sincospif of the fraction and everything
 *               after it fp32: the words of xengImage*, xengGaincal* and xengCalapply*, formed in registers by the lane that uses
 *               them and never stored (the state beyond the geometry is the records and one count per group) --
 *                 M_c[s p][t p] = sum_k C_k^pp * a_ks * conj(a_kt),   C^00 = C_XX, C^11 = C_YY
 *               and with cross = 1 at Initialize
 *                 M_c[s 0][t 1] = sum_k (C_Re + i C_Im)_k * a_ks * conj(a_kt),   M_c[s 1][t 0] = sum_k (C_Re - i C_Im)_k * a_ks * conj(a_kt)
 *               the convention under which xengImageRun reads a single component C at its pixel as [C_XX, C_YY, C_Re, C_Im].
 *               z_ks = C_k * a_ks is one fp32 multiply per part on the parallel hands; on the cross hands, with C = C_Re, D = C_Im:
 *                 XY:  Re z = fma(C, Re a, -(D Im a)),  Im z = fma(C, Im a, D Re a)
 *                 YX:  Re z = fma(C, Re a, D Im a),     Im z = fma(C, Im a, -(D Re a))
 *               Per word of M and per part one chain of fused multiply-adds on f32-input MFMAs, the records two per instruction in
 *               ascending order: of each pair first Re z Re a (k even, k odd), then Im z Im a (k even, k odd) for the real part; Im z
 *               Re a, then -Re z Im a for the imaginary part (xengCalapply*'s sequence).  The loop runs to the last filled record
 *               of the group, rounded up to a pair: the cost follows the list, not ncomp_max.  With cross = 0, C_Re and C_Im are
 *               ignored and the cross-hand words have no model.
 *   out         cf32 in vis's layout, not vis itself; 16-byte aligned; nothing past it is written.
 *                 mode XENG_PREDICT_SUBTRACT (after Initialize):  i > j: out = V - M, one fp32 subtraction per part; with cross = 0
 *                   the cross-hand words of the lower triangle are V's, bit for bit.
 *                 mode XENG_PREDICT_MODEL:  out = M; vis may be NULL and is not read; with cross = 0 the cross-hand words are +0.
 *                 i = j:  the real part of the same expression; the imaginary part is written as +0.
 *                 i < j:  the conjugate of out[c][j][i]: the same word with the sign of its imaginary part turned, not computed
 *                   again, so the output is Hermitian bit for bit.
 *               With no filled record the lower triangle is the input bit for bit (up to the sign of a zero).
 * There are no per-stand weights: every word of the lower triangle is read, and a NaN in an input word stays in that word and its
 * mirror.  One owner per Hermitian pair, no atomics, one summation order: a word does not depend on nstand, on the other channels or
 * groups of the call, on ncomp_max, on earlier settings nor on what else runs on the GPU.  Trailing empty records, and an empty
 * record in place of one with C = 0, leave every bit unchanged, up to the sign of a zero.
 * The state (records, freq, tau, counts) sits between two guard bands of 64 KiB.  SetGeometry and SetComponents wait for the context's
 * work in flight: a call between two Runs applies to the later one only; so does SetMode, which waits for nothing.
 * Rejected with INVALID_ARGUMENT at the call that sees it: a non-positive size, nfavg not dividing nfine, ncomp_max >
 * XENG_PREDICT_MAX_NCOMP, nstand > XENG_PREDICT_MAX_NSTAND, more than 65535 channels, ndir or the table above their limits, cross
 * not 0 or 1 (Initialize); NULL, a non-finite word (SetGeometry); NULL, a pixel outside [-1, ndir), a non-finite word of C in a
 * filled record -- with cross = 0 of C_XX, C_YY (SetComponents); an unknown mode (SetMode); NULL or misaligned pointers (Run).  Run
 * before SetGeometry, and every call without a context: XENG_STATUS_INVALID_STATE. */
#define XENG_PREDICT_MAX_NCOMP 4096
#define XENG_PREDICT_MAX_NSTAND 512
#define XENG_PREDICT_SUBTRACT 0
#define XENG_PREDICT_MODEL 1
int xengPredictInitialize(int gpu, int nstand, int nfine, int nfavg, int ndir, int ncomp_max, int cross);
/* the tiles of 32 stands per side, the work-groups of a Run, the LDS bytes of a work-group, the bytes of a span (input = output), the
 * bytes of state between the guard bands, the filled records of the list in force, the mode of the Runs to come */
int xengPredictGetInfo(int *ntile, int *ngroup, int *lds_bytes, long long *span_bytes, long long *state_bytes, long long *nfilled, int *mode);
/* tau: f64[ndir][nstand] seconds, freq: f64[nfine] Hz, on the host.  Waits for the context's work in flight. */
int xengPredictSetGeometry(const double *tau, const double *freq);
/* records: [nfine / nfavg][ncomp_max] of 32 bytes on the host, 4-byte aligned.  Waits for the context's work in flight; holds from
 * the next Run. */
int xengPredictSetComponents(const void *records);
/* XENG_PREDICT_SUBTRACT or XENG_PREDICT_MODEL, from the next Run */
int xengPredictSetMode(int mode);
/* enqueue only: one integration */
int xengPredictRun(const void *vis_dev, void *out_dev);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengPredictCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengPredictMark(unsigned long long *ticket);
int xengPredictWait(unsigned long long ticket);
int xengPredictTicketDone(unsigned long long ticket, int *done);
int xengPredictSync(void);
int xengPredictDestroy(void);

/* ---------------------------------------------------------------- Dedispersed transient search of the images
 * UpchanImageSearch (no reference counterpart: the reference has no detection stage): the image's channel groups are the
 * frequency axis and the integrations the time axis of a per-pixel dedispersed boxcar search (csrc/imsearch_kernels.h).
 * A context of its own, xengImsearch*.  It is independent of all others.  Its kernels run on the beamformer's stream, as
 * xengImage* and xengPulse* do.  One Run takes one integration.
 *   in
 *     - f32 [ngroup][4][npix], the span of xengImageRun.  The front of xengCleanRun's span has the same layout.
 *     - Only words 0 and 1 of a group are read.
 *     - The span is never written.
 *   series
 *     - I[n][g][x] = fl(XX + YY).
 *     - n counts integrations since the last reset: Initialize, Reset, SetDelays.
 *   baseline per (g, x): exactly xengPulse's.
 *     - Block k is the integrations [k*nstat, (k+1)*nstat).
 *     - The pivot is c_k, the block's first value.
 *     - For every integration: delta = fl(I - c_k), a = fl(a + delta), q = fmaf(delta, delta, q).
 *     - At the block's end: m_k = fl(a*r), v_k = fmaf(-m_k, m_k, fl(q*r)), with r = 1.0f/nstat from the host.
 *     - The block is valid iff 0 < v_k < inf.  Then g_k = 1.0f/sqrtf(v_k).
 *     - Every group is ingested, whatever its weight.
 *   normalised series
 *     - u[n][g][x] = fl(fl(fl(I - c_{k-1}) - m_{k-1}) * g_{k-1}) for n in a block k >= 1 that follows a valid block.
 *     - Otherwise there is "no u".
 *   delays
 *     - s[d][g], int32 [ndm][ngroup] on the host, 0 <= s <= max_delay, in integrations.
 *     - S = max s.  The back-delay is b[d][g] = S - s[d][g], xengDedisp's convention.
 *     - Output n is the event that reached the top of the band at integration n - S.
 *   weights
 *     - w[g], f32 [ngroup], finite and >= 0, at least one > 0.
 *     - A group of weight exactly 0 is left out of z, not multiplied.  A NaN in that group never reaches an output.
 *   dedispersed series
 *     - z[n][d][x] starts from +0.
 *     - The groups with w_g != 0 are taken in ascending g: z = fl(z + fl(w_g * u[n - b[d][g]][g][x])).
 *     - There is no fused multiply-add.  That keeps a numpy float32 restatement exact.
 *     - z[n] exists iff n >= n_w and every term has a u.  n_w is the integration count when the weights were last set.
 *     - A term needs n - b >= nstat as well as a valid block behind it.
 *     - kappa = (float)(1/sqrt(sum w^2)), float64 on the host, rounded once.
 *   boxcars
 *     - B_1 = z.
 *     - B_{2w}[n] = fl(B_w[n] + B_w[n - w]).
 *     - Widths are 1, 2, ... 2^(nwidth-1).
 *   score
 *     - fl(fl(B_w[n]*kappa)*rho_iw), with rho_iw = (float)2^(-iw/2).
 *     - It is scored iff every z under the boxcar exists and the score is not NaN.
 *   out
 *     - Per call [npix] x {f32 snr, i16 idm, i16 iw}, one 8-byte store per pixel, 16-byte aligned base.
 *     - The record holds the largest score over (d, iw), then the smallest d, then the smallest iw.
 *     - It is {+0, -1, -1} when nothing is scored.
 *     - Nothing past the plane is written.
 *   state, between two 64 KiB guard bands (xengImsearchCheckGuards)
 *     - f32 [7][ngroup][npix]: c, m, v, g of the last complete block and c, a, q of the running one.
 *     - A ring U[S + 1][ngroup][npitch], integration n at slot n mod (S+1).  "No u" is stored as a NaN.
 *     - A ring Z[T + 1][ndm][npitch], T = 2^(nwidth-1) - 1.
 *     - npitch is npix rounded up for aligned rows.
 *     - Whether a slot below the live range counts is taken from its index, never from what the buffer holds.
 *     - Reset moves only host counters.
 *     - SetDelays resets, because S moves the time axis.
 *     - SetWeights resets nothing but sets n_w.
 *   numerics
 *     - fp32, #pragma clang fp contract(off), no atomics.
 *     - Every word is one fixed-order chain.
 *     - A pixel's record depends on that pixel's words alone.  It does not depend on npix, on the pixel's place in the list,
 *       on the rings' wrap positions, or on what else runs on the GPU.
 *   entry points
 *     - xengImsearchInitialize(gpu, npix, ngroup, ndm, max_delay, nwidth, nstat)
 *     - SetDelays, SetWeights
 *     - Run(image_dev, out_dev)
 *     - Reset
 *     - GetInfo(&nintegrations, &S)
 *     - GetBaseline(c, m, v)
 *     - CheckGuards
 *     - Mark / Wait / TicketDone / Sync
 *     - Destroy
 *   rejected at Initialize, before a device is touched:
 *     - a non-positive size;
 *     - npix > 2^24, ndm > 1024, nwidth outside 1..6, nstat outside 2..2^20 or below the widest boxcar;
 *     - state above XENG_IMSEARCH_MAX_STATE_BYTES (1LL << 32).
 *   rejected by setters and Run, without a launch:
 *     - NULL or misaligned pointers, a delay outside 0..max_delay, a bad weight;
 *     - Run before SetDelays, and any call without a context: XENG_STATUS_INVALID_STATE.
 * The weights are all ones until SetWeights; max_delay may be 0 (one trial at DM 0), a negative one is rejected. */
#define XENG_IMSEARCH_MAX_STATE_BYTES (1LL << 32)
int xengImsearchInitialize(int gpu, int npix, int ngroup, int ndm, int max_delay, int nwidth, int nstat);
/* Both setters wait for the context's work in flight and upload from the host: int32 [ndm][ngroup], f32 [ngroup] */
int xengImsearchSetDelays(const int *delays);
int xengImsearchSetWeights(const float *weights);
/* enqueue only: one integration in, one record plane out */
int xengImsearchRun(const void *image_dev, void *out_dev);
/* host state only, nothing is launched and nothing cleared: the next input counts as integration 0 */
int xengImsearchReset(void);
/* integrations taken since the last reset, and S of the table in use (-1 before SetDelays) */
int xengImsearchGetInfo(long long *nintegrations, int *max_delay_in_use);
/* c, m and v of the last complete block into host f32[ngroup][npix] each; waits for the context's work in flight;
 * XENG_STATUS_INVALID_STATE before a block has completed */
int xengImsearchGetBaseline(float *c, float *m, float *var);
/* The state is allocated between two guard bands of 64 KiB: as xengDedispCheckGuards */
int xengImsearchCheckGuards(int *intact);
/* completion tickets for everything enqueued on the beamformer's stream so far, as xengUpchanMark / Wait / TicketDone */
int xengImsearchMark(unsigned long long *ticket);
int xengImsearchWait(unsigned long long ticket);
int xengImsearchTicketDone(unsigned long long ticket, int *done);
int xengImsearchSync(void);
int xengImsearchDestroy(void);

/* ---------------------------------------------------------------- bifrost-named adapters
 * Exact argument shapes of the reference's call sites; data pointers are taken from the
 * BFarray-like structs, sizes from the configured context. */
int bfXgpuInitialize(XENGarray *in, XENGarray *out, int gpu_dev);                      /* corr_block.py:253 */
int bfXgpuKernel(XENGarray *in, XENGarray *out, int doDump);                           /* corr_block.py:445 */
int bfXgpuCorrelate(XENGarray *in, XENGarray *out, int doDump);                        /* xgpu_test.py:86-89 */
int bfXgpuGetOrder(XENGarray *antpol_to_input, XENGarray *antpol_to_bl, XENGarray *is_conj); /* corr_block.py:331-333 */
int bfXgpuSubSelect(XENGarray *in, XENGarray *out, XENGarray *vismap, XENGarray *conj,
                    int nchan_sum, int unused);                                         /* corr_subsel_block.py:298 */
int bfXgpuReorder(XENGarray *in, XENGarray *out, XENGarray *baselines, XENGarray *is_conj); /* corr_output_full_block.py:669 */
int bfBeamformInitialize(int gpu, int ninput, int nchan, int ntime, int nbeam, int ntime_blocks); /* beamform_block.py:251 */
int bfBeamformRun(XENGarray *in, XENGarray *out, XENGarray *weights);                  /* beamform_block.py:449 */
int bfBeamformIntegrate(XENGarray *in, XENGarray *out, int ntime_sum);                 /* beamform_sum_beams_block.py:245 */
int bfBeamformIntegrateSingleBeam(XENGarray *in, XENGarray *out, int ntime_sum, int beam_id); /* beamform_sum_single_beam_block.py:114 */

#ifdef __cplusplus
}
#endif
#endif /* XENG_H_ */
