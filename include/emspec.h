/*
 * emspec.h — C ABI of libemspec, the MI355X reassigned-spectrogram engine.
 *
 * This is the drop-in boundary.  The reference
 * (effree/EM-Spec) ships binaries only: its source is private
 * (/root/reference/README.md:73), so NO reference FFI interface exists to
 * cite.  The only interface the reference side names is the renderer call
 *
 *     computeSpectrogramColumn(audioFrame, fftSize, hop, reassign)
 *
 * (BASELINE.json:north_star).  Every entry point below is therefore
 * [BUILD-DEFINED]; the comment on each one says which part of that call (or
 * which documented feature of the reference: README.md line) it serves.
 * INTEGRATION.md shows the N-API binding a maintainer adds on the
 * Electron/Node side.
 *
 * Conventions
 *   - plain C, no C++ types, no exceptions cross this boundary;
 *   - every function returns EMSPEC_OK (0) or a negative emspec_status;
 *     the message is available from emspec_last_error();
 *   - the caller owns every input and output buffer; buffers are borrowed
 *     for the duration of the call only;
 *   - one engine = one HIP device + one HIP stream; an engine is not
 *     thread-safe, calls on one engine are serialised by the caller;
 *   - there is NO CPU fallback: if no gfx950 device or no kernel image is
 *     available emspec_create fails with EMSPEC_ERR_NO_DEVICE.
 */
#ifndef EMSPEC_H
#define EMSPEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): emspec_config.mode is read (it was a reserved, ignored field in version 1, so a version-1 library would
 * silently run an EXACT-mode request in float32: emspec_create now rejects the mismatch); added emspec_mode,
 * emspec_build_info, emspec_device_status, emspec_comm_set_timeout; emspec_uses_fused answers for EXACT-mode engines too. */
/* (round 6 added the live multi-stream functions - emspec_columns ... emspec_live_streams - and changed no struct: still 2) */
#define EMSPEC_ABI_VERSION 2

typedef enum emspec_status {
    EMSPEC_OK = 0,
    EMSPEC_ERR_INVALID_ARG = -1,   /* bad size / null pointer / unsupported N,hop */
    EMSPEC_ERR_NO_DEVICE = -2,     /* no HIP device, or not gfx950 */
    EMSPEC_ERR_HIP = -3,           /* a HIP runtime call failed (message has the HIP error) */
    EMSPEC_ERR_OUT_OF_MEMORY = -4,
    EMSPEC_ERR_STATE = -5,         /* call sequence error (e.g. N/hop changed mid-stream without reset) */
    EMSPEC_ERR_COMM = -6           /* an RCCL call failed, or the ranks of a gather disagree (message has the detail) */
} emspec_status;

/* Output selection bits for emspec_out / emspec_out_device. */
#define EMSPEC_OUT_DB 1u     /* float32 dB per (column,row)               */
#define EMSPEC_OUT_RGBA 2u   /* uint8[4] colour per (column,row)          */
#define EMSPEC_OUT_INDEX 4u  /* uint8 palette index 0..255 per (column,row) */

/*
 * Engine configuration: the display-side settings the reference exposes as
 * sliders (README.md:43-51, assets/settings.png) plus the analysis grid.
 * All fields are plain scalars; zero-initialise then call
 * emspec_default_config().
 */
typedef struct emspec_config {
    int32_t abi_version;   /* must be EMSPEC_ABI_VERSION */
    int32_t device;        /* HIP device ordinal */
    int32_t rows;          /* R: log-frequency rows per column (64..4096), default 1024 */
    int32_t mode;          /* EMSPEC_MODE_FAST (0, default) or EMSPEC_MODE_EXACT; see below */
    float sample_rate;     /* Hz, default 48000 */
    float fmin_hz;         /* lowest row edge, default 20 */
    float fmax_hz;         /* highest row edge, default sample_rate/2 */
    float gain;            /* linear amplitude gain before dB ("Gain", README.md:47) */
    float db_top;          /* dB value mapped to palette index 255, default 0 */
    float db_range;        /* dB span mapped onto the palette ("dB Range", README.md:46) */
    float gate_db;         /* cells below this dB are drawn as index 0 ("Noise Gate", README.md:51) */
    float power_floor;     /* bins with |X_h|^2 below this are not reassigned/accumulated */
} emspec_config;

/*
 * Arithmetic modes [BUILD-DEFINED] (north_star: results must match the reference JS path "within 1e-4 relative on
 * magnitude and exactly on reassigned integer (time,freq) bin indices"; JavaScript arithmetic is IEEE binary64).
 *   EMSPEC_MODE_FAST   float32 throughout: indices are exact against the float32 bit model; against a
 *                      binary64 evaluation a few 1e-4 of the bins that sit on a cell edge land in the neighbouring
 *                      cell, and cells are summed in arrival order (dB reproducible to a few ulp).
 *   EMSPEC_MODE_EXACT  binary64 from the frame to the indices, energy summed in 64-bit fixed point (order-
 *                      independent), dB through a specified binary32 evaluation (no library call, no division; DESIGN.md 3.7;
 *                      within 2e-5 dB of the real value): (column,row) agree
 *                      with a float64 implementation of the three-window method on every bin, and dB / palette index /
 *                      RGBA are bit-reproducible run to run and equal to the CPU bit model's bytes (every table - twiddles,
 *                      log-spaced row edges, dB polynomial - is a specified sequence of IEEE operations, no libm call, so the
 *                      bytes do not depend on the host's C library; "(column,row) agree with a
 *                      float64 implementation on every bin" is a measured statement: 0 mismatches in > 10^8 values, where
 *                      two binary64 evaluations may still differ on a bin within ~1e-13 of an edge).  Inputs must stay
 *                      within |x| <= 4 (the fixed point covers 2^11 full-scale-sine powers per cell).  Cell sums are taken
 *                      modulo 2^64: one bin carries at most 2^61 units (2^9 full-scale sines; louder bins are dropped), and a
 *                      cell that receives more than 2^63 units is outside the guarantee (its sum wraps).  Same entry points;
 *                      emspec_parity_dump_exact replaces emspec_parity_dump.  Roughly 2.1x slower than the fast mode at N = 4096.
 */
#define EMSPEC_MODE_FAST 0
#define EMSPEC_MODE_EXACT 1

typedef struct emspec_engine emspec_engine;

/* Host-memory outputs of emspec_batch: any pointer may be NULL (not wanted).
 * Layout of each: [streams][columns][rows] (+[4] for rgba), C order. */
typedef struct emspec_out {
    float* db;
    uint8_t* rgba;
    uint8_t* index;
} emspec_out;

/* Fill *cfg with the defaults listed above. */
int emspec_default_config(emspec_config* cfg);

/* Create an engine on cfg->device.  Serves: engine construction behind the
 * renderer's first computeSpectrogramColumn call. */
int emspec_create(const emspec_config* cfg, emspec_engine** out_engine);
void emspec_destroy(emspec_engine* e);

/* The arithmetic mode this engine really runs in (EMSPEC_MODE_FAST / EMSPEC_MODE_EXACT), -1 for NULL: lets a binding
 * assert that a request for bit-exact results was honoured. */
int32_t emspec_mode(const emspec_engine* e);

/* What this library was built from: "emspec abi=2 sources=<16 hex digits> arch=gfx950", the digits being the sha1 of the
 * kernel / C-ABI sources (tools/sources_sha.py) taken when the library was compiled.  bench.py quotes profile-derived
 * numbers only while this, the source tree and the profile agree.  Never NULL; static storage. */
const char* emspec_build_info(void);

/* Synchronises the engine's device and reports what its kernels may have flagged since the last call: EMSPEC_OK, or
 * EMSPEC_ERR_HIP when a kernel's bounded wait timed out (the fused kernels order some phases with arrival counters in
 * LDS; every wait is bounded so that a protocol error cannot hang the device - the results of that launch are then
 * invalid) or the device reports an asynchronous error.  The synchronous batch entry points (emspec_batch,
 * emspec_batch_gather) check it themselves; callers of emspec_batch_device call this after their own stream
 * synchronisation when they want the check (the streaming calls run kernels without such waits). */
int emspec_device_status(emspec_engine* e);

/* Last error message of this engine (or of the failed emspec_create when
 * e == NULL).  Never NULL; valid until the next call on the same thread. */
const char* emspec_last_error(const emspec_engine* e);

/* Upload a 256-entry RGBA palette ("Color Map", README.md:15).  The default
 * is the 5-stop gradient measured from assets/settings.png. */
int emspec_set_colormap(emspec_engine* e, const uint8_t* rgba256x4);

/*
 * Frequency axis.  By default the R rows are log-spaced between fmin_hz and fmax_hz.
 * emspec_set_row_edges_hz installs any strictly increasing table of rows+1 edges in
 * (0, sample_rate/2] instead — the hook for the reference's "Frequency Scale" (zoom) and
 * "Low-End Boost" sliders (README.md:48-49), whose laws are undocumented and therefore
 * left to the host (em-spec_amd/js/index.js ships one).  NULL restores the log axis.
 * Row r collects the bins whose reassigned frequency lies in [edge[r], edge[r+1]).
 * emspec_get_row_edges_hz returns the table in use: the inverse map the shift+hover
 * frequency read-out needs (README.md:39).  Not allowed while streaming columns are pending.
 */
int emspec_set_row_edges_hz(emspec_engine* e, const float* edges_hz, int32_t count);

/*
 * Display-parameter laws [BUILD-DEFINED] (the reference's slider laws are undocumented,
 * README.md:44-51), host-independent so that every binding draws the same picture.  No engine needed.
 * emspec_warped_edges_hz: rows+1 edges for emspec_set_row_edges_hz from "Frequency Scale" (zoom:
 * the axis spans fmin .. fmin*(fmax/fmin)^(1/freq_scale)) and "Low-End Boost" (row r sits at
 * u = (r/rows)^low_end_boost along the log range; > 1 gives the low end more rows); (1, 1) is the
 * plain log axis.  emspec_make_colormap: the reference's 5-stop ramp scaled by
 * "Brightness" (0.5 = as measured), 256 RGBA entries for emspec_set_colormap.
 */
int emspec_warped_edges_hz(int32_t rows, float fmin_hz, float fmax_hz, float low_end_boost,
                           float freq_scale, float* out_edges_hz);
int emspec_make_colormap(float brightness, uint8_t* out_rgba256x4);
int emspec_get_row_edges_hz(emspec_engine* e, float* edges_hz, int32_t count);

/*
 * Display post-process over finished columns, per stream and in time order (README.md:14 "adaptive
 * brightness", README.md:50 "temporal smoothing"; laws [BUILD-DEFINED]):
 *   agc_strength in [0,1]: a column-peak follower (fast attack, slow release) shifts every column by
 *                          agc_strength * (db_top - level) dB, limited to +-40 dB;
 *   smoothing    in [0,0.95]: y[c] = smoothing*y[c-1] + (1-smoothing)*x[c] per row, on the dB values.
 * Both 0 (the default) = off.  Applies to emspec_batch / _device and to the streaming call (whose
 * state emspec_reset clears).  The dB output is the post-processed value; index and RGBA follow it.
 */
int emspec_set_display(emspec_engine* e, float smoothing, float agc_strength);

/* Number of columns a stream of L samples yields: (L-n)/hop+1, or 0. */
int64_t emspec_num_columns(int64_t L, int32_t n, int32_t hop);

/* Time reassignment moves energy up to ceil(n/(2*hop)) columns either way,
 * so the streaming call returns column j-D when fed frame j.  This is D. */
int32_t emspec_latency_columns(int32_t n, int32_t hop, int32_t reassign);

/*
 * Streaming, one frame per call — THE call the renderer makes:
 *   computeSpectrogramColumn(audioFrame, fftSize, hop, reassign)
 * frame: n float32 samples (frame j of the stream = samples [j*hop, j*hop+n)).
 * The engine keeps the pending-column ring on the device.  With D =
 * emspec_latency_columns(), call number j (0-based) writes finished column
 * j-D; for j < D the output is the empty column (all cells at the dB floor)
 * and *out_column (if non-NULL) is set to -1.  out_db (rows floats) and
 * out_rgba (rows*4 bytes) may each be NULL.
 * Changing n/hop/reassign between calls without emspec_reset() is
 * EMSPEC_ERR_STATE.
 */
int emspec_column(emspec_engine* e, const float* frame, int32_t n, int32_t hop,
                  int32_t reassign, float* out_db, uint8_t* out_rgba,
                  int32_t rows, int64_t* out_column);

/* Flush: emit the next of the D columns still pending after the last frame
 * (feeds no new samples).  Returns EMSPEC_ERR_STATE when nothing is pending.
 * A flushed stream is at its end - later frames would still have added to the
 * columns a flush emits - so feeding it again without emspec_reset() is
 * EMSPEC_ERR_STATE. */
int emspec_column_flush(emspec_engine* e, float* out_db, uint8_t* out_rgba,
                        int32_t rows, int64_t* out_column);

/*
 * Streaming by sample blocks: the audio callback hands over whatever block it
 * has (any count >= 0); the engine keeps the unconsumed tail of the stream on
 * the device (sample ring) next to the pending-column ring, and every `hop`
 * new samples complete one frame.  Finished columns (column c is complete once
 * frame c+D has been seen) are written oldest first to out_db [max_columns][rows]
 * and/or out_rgba [max_columns][rows][4]; *out_count receives how many,
 * *out_first_column the absolute index of the first (-1 if none).  Unlike
 * emspec_column no empty columns are produced while the ring primes.
 * emspec_push_columns() tells in advance how many columns a block of `count`
 * samples will complete (for sizing the outputs; -1 on invalid arguments); a
 * block that completes more than max_columns is rejected before any state changes.
 * (With both outputs NULL - a priming call - max_columns is not consulted: the columns are completed and dropped.)
 * The D columns pending after the last block are drained with emspec_column_flush;
 * samples short of a hop are dropped by emspec_reset.  One stream must be fed
 * through either emspec_column or emspec_push_samples, not both (EMSPEC_ERR_STATE).
 */
int64_t emspec_push_columns(const emspec_engine* e, int64_t count, int32_t n,
                            int32_t hop, int32_t reassign);
int emspec_push_samples(emspec_engine* e, const float* samples, int64_t count,
                        int32_t n, int32_t hop, int32_t reassign, float* out_db,
                        uint8_t* out_rgba, int32_t rows, int64_t max_columns,
                        int64_t* out_count, int64_t* out_first_column);

/* Drop all per-stream state (sample position, pending ring), of the single-stream calls above and of the live
 * multi-stream session below. */
int emspec_reset(emspec_engine* e);

/*
 * ---- Live multi-stream streaming: S streams advance together, ONE kernel launch and ONE synchronisation per call.
 * Serves: BASELINE.json configs[2] ("64 concurrent 48 kHz streams") in the form the renderer calls it - north_star's
 * per-frame computeSpectrogramColumn(audioFrame, fftSize, hop, reassign), README.md:36 ("automatically start visualizing
 * your system audio") - where one engine per stream would cost S launches + S synchronisations per hop on the host
 * thread.  [BUILD-DEFINED]; same arithmetic, same results as emspec_column / emspec_push_samples / emspec_batch on every
 * stream (FAST mode: the float32 sums are taken in arrival order, dB equal to a few ulp; EXACT mode: equal bytes).
 *
 * The first call fixes the session: streams, fft size, hop, reassign and the feeding form (per frame OR per sample block);
 * changing any of them later is EMSPEC_ERR_STATE until emspec_reset().  The session is independent of the single-stream
 * state of emspec_column / emspec_push_samples (which are the one-stream case of the same code, on a session of their own).  Every stream has its own position: emspec_reset_stream(e, s) restarts
 * stream s (its sample position, pending columns and display post-process state) while the others continue.
 * Buffers: any host memory works; when a buffer is page-locked (emspec_host_alloc) the kernel reads / writes it in place
 * (no staging copy on the host thread) - for 64 streams of n = 4096 that is 1 MB of frames per emspec_columns call.
 *
 * emspec_columns: per-frame form.  frames[streams][n]: frame j_s of each stream (stream s has been fed j_s frames so far).
 *   out_db[streams][rows] / out_rgba[streams][rows][4] (each may be NULL) receive column j_s - D of every stream
 *   (D = emspec_latency_columns), the empty column while a stream's ring primes; out_columns[streams] (optional) the
 *   column index, -1 for the empty column.
 * emspec_columns_flush: every stream that still has pending columns emits its next one (others: the empty column, -1).
 *   EMSPEC_ERR_STATE when no stream has any.  Works for both feeding forms.  A flushed stream is at its end: feeding the
 *   session again is EMSPEC_ERR_STATE until that stream is restarted (emspec_reset_stream) or the session reset.
 * emspec_push_samples_multi: per-sample-block form.  samples: `count` new samples of every stream, stream s at
 *   samples + s * stride (stride >= count: a window of a larger [streams][...] array works).  Finished columns of stream s
 *   go to out_db[s][0 .. out_counts[s]) of out_db[streams][max_columns][rows] (and / or out_rgba, same layout + [4]),
 *   oldest first; out_first_columns[s] = absolute index of the first, -1 if none.  No empty columns.  A block that
 *   completes more than max_columns columns on some stream is rejected before any state changes
 *   (emspec_push_columns_multi = the largest per-stream count a block of `count` samples will complete).  Blocks that
 *   complete no frame only join a staging block on the host: no launch.
 * emspec_live_streams: streams of the current session (0 = none).
 */
int emspec_columns(emspec_engine* e, const float* frames, int32_t streams, int32_t n, int32_t hop, int32_t reassign,
                   float* out_db, uint8_t* out_rgba, int32_t rows, int64_t* out_columns);
int emspec_columns_flush(emspec_engine* e, float* out_db, uint8_t* out_rgba, int32_t rows, int64_t* out_columns);
int64_t emspec_push_columns_multi(const emspec_engine* e, int64_t count, int32_t n, int32_t hop, int32_t reassign);
int emspec_push_samples_multi(emspec_engine* e, const float* samples, int32_t streams, int64_t count, int64_t stride,
                              int32_t n, int32_t hop, int32_t reassign, float* out_db, uint8_t* out_rgba, int32_t rows,
                              int64_t max_columns, int64_t* out_counts, int64_t* out_first_columns);
int emspec_reset_stream(emspec_engine* e, int32_t stream);
int32_t emspec_live_streams(const emspec_engine* e);

/*
 * Batched throughput entry point, host buffers: S streams of L samples
 * (pcm[S][L], row-major) -> every finished column of every stream.
 * Copies in, runs the fused column kernel, copies the selected outputs back.
 * When every buffer is page-locked (emspec_host_alloc) the call runs a three-stage pipeline over ~16 chunks of streams -
 * host->device copies, kernels, device->host copies on three HIP streams of the engine - in either arithmetic mode and with
 * the display post-process; what bounds it is PCIe (uint8 index out: ~45 GB/s each way at once on a Gen5 x16 link).
 * Ordinary (pageable) buffers run the same pipeline: the runtime's copies block the calling thread, so the library starts a
 * second host thread for the copies out (and three that touch the destination's pages ahead of it - a result array allocated
 * per call has none resident), all joined before the call returns: the page-locked rate when the pages are resident (4.3e7
 * columns/s on the bench shape), a third of it into a fresh array.  With fewer than sixteen streams (one long recording) the
 * pipeline's units are runs of >= 16,384 columns of a stream, each computed from the frames that reach it - the same columns
 * (EXACT mode: the same bytes) as in one piece; a batch too short for two units takes one copy in, the kernels, one copy out.
 * With the display post-process on, units are whole streams.  On an error return the outputs are unspecified (partly written
 * or page-touched).  Serves: the renderer-side batched computeColumns of the N-API addon (em-spec_amd/js/index.js).
 */
int emspec_batch(emspec_engine* e, const float* pcm, int32_t S, int64_t L,
                 int32_t n, int32_t hop, int32_t reassign, const emspec_out* out);

/*
 * Page-locked host memory for the buffers of emspec_batch / emspec_column / the live calls: copies from and to it
 * are asynchronous and need no extra host thread, and the streaming kernels read / write it in place (pageable
 * memory costs the streaming calls a staging copy each way).  Optional: any host memory works.  Needs no engine;
 * free with emspec_host_free.
 */
int emspec_host_alloc(size_t bytes, void** out);
void emspec_host_free(void* p);

/*
 * Same, device-resident: pcm and the outputs are device pointers on the
 * engine's device; the kernels are enqueued on hip_stream (a hipStream_t
 * passed as void*, NULL = the HIP default stream) and the call returns
 * without synchronising.  Output pointers may be NULL.  Calls on one engine
 * share its device workspaces: enqueue them on one stream, or order them
 * yourself (events) when using several.
 *
 * Streams and ordering (every entry with a hip_stream argument; tests/test_gpu_stream_order.py holds each to it under forced
 * delays).  All of an entry's work is enqueued on hip_stream, and the entry returns without synchronising, except where its own
 * text says otherwise (emspec_wire_pack when the size is asked for, emspec_wire_unpack's header check, emspec_gather_columns).
 *   The library orders by itself: the EXACT kernels' low-row scratch - a launch on another stream than the previous one waits
 *     for it, and a call that has to regrow the scratch blocks the host until the launch on the old buffer has finished; and
 *     the streaming calls behind the views and re-analyses of the live rings (emspec_history_view_device,
 *     emspec_history_view_stereo_device, emspec_audio_view_device, emspec_audio_batch_device): a push, emspec_reset_stream,
 *     emspec_set_live_history(0) and emspec_set_live_audio(0) that follow one of them take effect behind it.
 *   The caller orders: everything else that shares the engine's workspaces - two device entries on two streams need an event
 *     between them (record on the first stream behind call 1, make the second stream wait for it in front of call 2).  A call
 *     that has to build a shape's tables or grow a workspace may block the host while it does.
 *   The caller's duty: the setters that rewrite device tables - emspec_set_colormap, emspec_set_stereo_colormap,
 *     emspec_set_row_edges_hz - run on the engine's own stream; do not call them while a device entry is pending on another
 *     stream.
 */
int emspec_batch_device(emspec_engine* e, const float* pcm_dev, int32_t S,
                        int64_t L, int32_t n, int32_t hop, int32_t reassign,
                        float* db_dev, uint8_t* rgba_dev, uint8_t* index_dev,
                        void* hip_stream);

/*
 * Parity dump: per-bin results of frames [frame0, frame0+nframes) of each of
 * the S streams, before the histogram scatter.  K = n/2+1 bins per frame.
 *   power[s][f][k] = |X_h[k]|^2          (float32)
 *   col  [s][f][k] = absolute reassigned column index (int32)
 *   row  [s][f][k] = log-frequency row, or -1 if the bin is gated/out of range
 * Host pointers.  Used by the parity tests (exact col/row, 1e-4 on power).
 */
int emspec_parity_dump(emspec_engine* e, const float* pcm, int32_t S, int64_t L,
                       int32_t n, int32_t hop, int32_t reassign,
                       int64_t frame0, int64_t nframes,
                       float* power, int32_t* col, int32_t* row);

/*
 * Parity dump of an EXACT-mode engine (EMSPEC_ERR_STATE on a fast-mode engine, and vice versa for emspec_parity_dump):
 *   power[s][f][k] = |X_h[k]|^2 (binary64), col / row as above, q[s][f][k] (optional, may be NULL) = the bin's
 *   fixed-point energy as it is added to the histogram (0 when the bin is dropped): round(power * 2^52 / (n/4)^2).
 * Host pointers.
 */
int emspec_parity_dump_exact(emspec_engine* e, const float* pcm, int32_t S, int64_t L,
                             int32_t n, int32_t hop, int32_t reassign,
                             int64_t frame0, int64_t nframes,
                             double* power, int32_t* col, int32_t* row, int64_t* q);

/* Device-pointer form of emspec_parity_dump (all five buffers on the device). */
int emspec_parity_dump_device(emspec_engine* e, const float* pcm_dev, int32_t S,
                              int64_t L, int32_t n, int32_t hop, int32_t reassign,
                              int64_t frame0, int64_t nframes,
                              float* power_dev, int32_t* col_dev, int32_t* row_dev,
                              void* hip_stream);

/*
 * ---- Multi-GPU: shard the streams, gather the finished columns (BASELINE.json north_star: "many independent
 * audio streams shard embarrassingly across the 8 GPUs of one node with a single RCCL gather over xGMI to collect
 * finished columns").  The reference has no GPU path and no collectives: [BUILD-DEFINED].
 *
 * One process (or thread) per GPU, each with its own engine.  The host splits the streams into shards (equal, or a
 * smaller one for the root, which also expands what it receives), every rank runs emspec_batch_device on its shard
 * (no exchange during compute), then all ranks call emspec_gather_columns: the palette-index columns (uint8, 1 byte
 * per cell - the float32 dB columns stay on the producing GPU) of every rank arrive on `root`, the ranks' blocks
 * [columns_r][rows] one after the other in rank order.
 *
 * Rank 0 obtains an id with emspec_comm_unique_id and hands its 128 bytes to the other ranks by whatever channel
 * the host has (Node: IPC / a file; Python: torch.distributed's store); every rank then calls emspec_comm_init
 * (collective: returns when all `world` ranks have called it).  The communicator lives as long as the engine.
 */
#define EMSPEC_COMM_ID_BYTES 128
int emspec_comm_unique_id(uint8_t* id_out /* [EMSPEC_COMM_ID_BYTES] */);
int emspec_comm_init(emspec_engine* e, const uint8_t* id /* [EMSPEC_COMM_ID_BYTES] */, int32_t rank, int32_t world);
int emspec_comm_destroy(emspec_engine* e);
/* Bound (seconds, default 120; 0 = none) on the one host wait inside emspec_gather_columns - the size exchange every rank
 * must enter.  When it expires the communicator is aborted (ncclCommAbort) and the call returns EMSPEC_ERR_COMM: a rank
 * that died does not hang its peers for ever.  May be called before emspec_comm_init. */
int emspec_comm_set_timeout(emspec_engine* e, double seconds);
int32_t emspec_comm_rank(const emspec_engine* e);    /* -1 without a communicator */
int32_t emspec_comm_world(const emspec_engine* e);   /* 0 without a communicator */

/*
 * Collective over the engine's communicator.  index_dev: this rank's finished palette-index columns
 * [columns][rows] on its device (columns = streams * columns-per-stream of the shard; ranks may differ).
 * gathered_dev (root only; ignored elsewhere): the ranks' blocks in rank order on the root's device, sum(columns_r) *
 * rows bytes; gathered_capacity = the bytes available there (the call fails with EMSPEC_ERR_INVALID_ARG on the root
 * before writing anything if the announced shards do not fit).
 * xGMI is point-to-point - each rank reaches the root over one link - so the columns travel as a lossless packed
 * image (per-column offset + bit mask of the non-zero cells + their indices; emspec_wire_* below) and are expanded on the root.
 * The call enqueues everything on hip_stream and synchronises that stream ONCE (the packed sizes differ per rank
 * and must be known on the host before the transfers can be posted): enqueue the next chunk's
 * emspec_batch_device on another stream BEFORE calling it, and the gather overlaps that compute.
 * *wire_bytes_sent (optional) receives the size of this rank's packed image (0 on the root).
 * Failure semantics: whatever can fail on one rank alone (arguments, device memory, the pack launch) is detected before the
 * size exchange, and that rank still enters the exchange with an error mark in place of its size - so ALL ranks return
 * from the same call: the failing rank with its own error, the others with EMSPEC_ERR_COMM, nothing transferred, the
 * communicator still usable.  An RCCL error, or a peer that does not show up within the timeout, aborts the communicator
 * (later calls: EMSPEC_ERR_STATE).
 * flags: EMSPEC_GATHER_LOOPBACK makes the root's own columns take the wire as well (self send/recv; exercising
 * the whole path on a single GPU).
 * EMSPEC_GATHER_PACKED: the root does NOT expand: gathered_dev receives a directory (per rank: u64 offset, u64 image bytes,
 * u64 columns, u64 0; padded to 256 B) followed by every rank's wire image (the root's own included), 256-byte aligned,
 * in rank order; capacity needed: align256(32 * world) + sum over ranks of align256(emspec_wire_bound(columns_r, rows))
 * (align256(x) = x rounded up to a multiple of 256).  Nothing is
 * lost - emspec_wire_unpack(gathered_dev + offset, bytes, columns, ...) expands any rank's block on demand (the layout
 * is also available on the host: emspec_gather_packed_layout) - and the root, which otherwise expands world-1 images
 * per gather beside its own column kernel, only receives.
 */
#define EMSPEC_GATHER_LOOPBACK 1u
#define EMSPEC_GATHER_PACKED 2u
int emspec_gather_columns(emspec_engine* e, const uint8_t* index_dev, int64_t columns, int32_t root,
                          uint8_t* gathered_dev, int64_t gathered_capacity, uint32_t flags, void* hip_stream,
                          int64_t* wire_bytes_sent);

/* Root, after an EMSPEC_GATHER_PACKED gather: where rank `rank`'s image sits in gathered_dev (any pointer may be NULL). */
int emspec_gather_packed_layout(const emspec_engine* e, int32_t rank, int64_t* offset, int64_t* bytes, int64_t* columns);

/*
 * Host-buffer convenience for a rank process (the N-API addon's computeColumnsGather): this rank's S streams
 * (pcm[S][L], host memory) -> finished columns on the device -> emspec_gather_columns -> on `root` the palette-index
 * columns of all ranks in host memory, gathered_index[world][S][columns][rows] (ignored elsewhere).  db_local
 * (optional, any rank): this rank's own float32 dB columns [S][columns][rows].  Synchronous; collective.
 */
int emspec_batch_gather(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop,
                        int32_t reassign, int32_t root, uint8_t* gathered_index, float* db_local,
                        int64_t* wire_bytes_sent);

/*
 * The wire image by itself, for hosts that bring their own transport: header (32 B) + a u32 payload offset per
 * column + ceil(rows/32) mask words per column + the non-zero indices (column after column, rows ascending), zero-padded
 * to a multiple of 16 B: every byte of an image is specified, so equal columns give equal images (round 5; see
 * em-spec_amd/csrc/pack.hip.inc, restated in oracle/wire_ref.py).
 * emspec_wire_bound: capacity a destination needs for `columns` columns (-1 on invalid arguments).
 * emspec_wire_pack:  index_dev [columns][rows] -> wire_dev; *wire_bytes (optional) = the image size (reading it
 *                    synchronises hip_stream; pass NULL to stay asynchronous).
 * emspec_wire_unpack: validates the header against this engine (rows) and `columns`, then expands.
 * All pointers are device pointers on the engine's device; at most 2^32 cells per call.
 */
int64_t emspec_wire_bound(int64_t columns, int32_t rows);
int emspec_wire_pack(emspec_engine* e, const uint8_t* index_dev, int64_t columns, uint8_t* wire_dev,
                     int64_t* wire_bytes, void* hip_stream);
int emspec_wire_unpack(emspec_engine* e, const uint8_t* wire_dev, int64_t wire_bytes, int64_t columns,
                       uint8_t* index_dev, void* hip_stream);

/*
 * Host-buffer batch whose palette-index columns leave the device PACKED: the same columns as emspec_batch(out->index), but
 * what crosses PCIe is the lossless wire image above (~186 B instead of 1,024 B per column on typical audio), ONE IMAGE
 * PER STREAM, tightly packed into `wire` (host memory, pinned for full speed) in stream order: stream s occupies
 * wire[offsets[s] .. offsets[s+1]) (offsets: streams + 1 entries, offsets[0] = 0; every image STARTS on a 16-byte boundary,
 * so up to 12 bytes of slack may follow an image inside its slot, cleared to zero - wire[0 .. offsets[streams]) holds the
 * same bytes whatever the buffer held before; an image's own size is in its header, and emspec_wire_unpack_host /
 * emspec_wire_unpack accept the slot as it is).
 * wire_capacity = streams x emspec_wire_bound(columns, rows) always suffices; EMSPEC_ERR_INVALID_ARG when the images do not
 * fit.  Runs the three-stage pipeline of emspec_batch (H2D | kernels + pack | D2H on three HIP streams); rows % 4 == 0.
 * Serves: the renderer-side batched computeColumns when the host keeps or forwards the columns compressed
 * (north_star: "host code stays in JavaScript/Node calling HIP through a thin C-ABI N-API addon").
 * emspec_wire_unpack_host: expand one image on the host's own cores (plain C, no device, no engine):
 * wire -> index_out [columns][rows]; validates the header and every offset (a damaged image is rejected, never
 * read or written out of range).
 */
int emspec_batch_packed(emspec_engine* e, const float* pcm, int32_t streams, int64_t samples_per_stream, int32_t fft_size,
                        int32_t hop, int32_t reassign, uint8_t* wire, int64_t wire_capacity, int64_t* offsets);
int emspec_wire_unpack_host(const uint8_t* wire, int64_t wire_bytes, int64_t columns, int32_t rows, uint8_t* index_out);

/*
 * Time reduction [BUILD-DEFINED]: the zoomed-out view of a recording - the reference's "Scroll Speed"
 * (README.md:44) - computed on the device.  With factor f > 1 a batch call whose full-rate result would be C columns per stream
 * delivers Cr = emspec_reduced_columns(C, f) = ceil(C / f) columns: groups of f consecutive finished columns collapse into one
 * by maximum (peak hold: a click or a short tone stays visible at any zoom), the last group being the C - (Cr - 1) f columns
 * that remain.  With full_* what the same call returns at f = 1 - the display post-process (emspec_set_display: smoothing and
 * AGC run at full rate) and the multi-resolution composition included - for g in [0, Cr), r in [0, rows):
 *     db   [s][g][r] = m,  where m = full_db[s][g f][r]; then for c = g f + 1 .. min((g + 1) f, C) - 1 in order:
 *                          if (full_db[s][c][r] > m) m = full_db[s][c][r]
 *     index[s][g][r] = max over the group of full_index[s][c][r]      (unsigned bytes)
 *     rgba [s][g][r] = LUT[index[s][g][r]]
 * exact in either arithmetic mode: the reduced bytes follow from the full-rate bytes.  Layouts are those of the entry with Cr in
 * place of the column count; column g is centred in time on its group (the host maps pixels to time with f * hop).
 * Honoured by emspec_batch_device, emspec_batch, emspec_batch_packed, emspec_batch_pcm, emspec_batch_pcm_packed,
 * emspec_batch_multires, emspec_batch_multires_device, emspec_batch_multiband, emspec_batch_multiband_device and
 * emspec_batch_gather (whose gathered layout is [world][S][Cr][rows]).
 * The packed entries pack the REDUCED columns: the header's column count is Cr, wire_capacity = streams x emspec_wire_bound(Cr,
 * rows) always suffices, and the 2^32-cell limit applies to Cr x rows.  The device entries keep a chunk of streams' full-rate
 * columns in an engine workspace bounded like the records path's (1 byte per cell when only index / RGBA are asked for, 4 more
 * with dB); the host entries reduce inside each unit's staging set, and their copies out shrink by f.
 * Not affected: the parity dumps, emspec_pcm_decode_device, emspec_wire_*, emspec_gather_columns (its caller's column count
 * rules).  The STREAMING calls - emspec_column, emspec_push_samples, emspec_columns*, emspec_push_samples_*, the flushes - return
 * EMSPEC_ERR_STATE while f > 1 (a live host takes the maximum of a handful of 1 KB columns itself).
 * emspec_set_time_reduce: factor in 1 (off, the default) .. 65536, else EMSPEC_ERR_INVALID_ARG; EMSPEC_ERR_STATE while a
 *   streaming session has columns pending (as emspec_set_row_edges_hz).  A refusal changes nothing.
 * emspec_time_reduce: the factor in force, -1 for NULL.
 * emspec_reduced_columns: ceil(columns / factor); -1 for columns < 0 or a factor outside 1 .. 65536.  No engine needed.
 */
int emspec_set_time_reduce(emspec_engine* e, int32_t factor);
int32_t emspec_time_reduce(const emspec_engine* e);
int64_t emspec_reduced_columns(int64_t columns, int32_t factor);

/* Copy out the tables the kernels use for (n): row edges in bin units
 * (rows+1 floats) and the twiddle table (n/2 complex = n floats, re,im
 * interleaved).  Either pointer may be NULL.  For table-parity tests. */
int emspec_get_tables(emspec_engine* e, int32_t n, float* edges_bins, float* twiddle);

/* 1 if emspec_batch/_device would run a fused LDS-ring kernel for this shape
 * (n = 1024, 2048, 4096 at any hop whose column ring fits in LDS; n = 8192 at
 * hop 512 or 1024; n = 16384 at any hop whose ring has at most 33 slots of 1024
 * rows, e.g. hop 512; at most 1024 rows), 0 if the generic two-kernel path
 * (per-bin records + LDS tile / walking-ring scatter).  EXACT-mode engines:
 * 1 for n = 4096, 2048 and 1024 when the u64 column ring (2 D + 2 * 4096 / n slots) fits in LDS
 * beside the 64 KB of binary64 planes - whole, or with its low rows in a per-workgroup scratch in
 * global memory when at most 6 % of a frame's bins fall there (exact_fused_lr.hip.inc; on the default
 * log axis e.g. n = 4096 / hop 256, n = 2048 / hop 128 or 256, n = 1024 / hop 128 or 256; other
 * axes at n = 4096 run exact_fused.hip.inc's kernel, which parks the ring under the planes) - else 0:
 * n = 8192 and 16384 run the two-kernel records path.  Same results either way. */
int emspec_uses_fused(const emspec_engine* e, int32_t n, int32_t hop, int32_t reassign);

/* Name of the device the engine runs on, e.g. "gfx950". */
const char* emspec_device_arch(const emspec_engine* e);

/*
 * Multi-resolution batch: a long FFT (n_low) for the rows below split_row and a short one (n_high) for
 * the rows from split_row up, on ONE column grid - two bass notes a fraction of a short FFT's bin apart separate, and
 * transients in the upper rows stay sharp.  The image is defined as a stitch of two single-resolution batches on the same
 * engine and row table (emspec_batch at n_low and at n_high, same hop and reassign):
 *     image[s][c][r] = single(n_low)[s][c][r]           r <  split_row
 *     image[s][c][r] = single(n_high)[s][c + shift][r]  r >= split_row
 * for c in [0, columns): column c is centred at sample c * hop + n_low / 2 in both bands.  dB, palette index and RGBA are
 * those bytes (EXACT mode: bit for bit); with the display post-process on (emspec_set_display) it runs once over the
 * composed raw dB, by the law of a single-resolution batch.  Accepted shapes: n_low in {8192, 16384}, n_high in {1024, 2048,
 * 4096}, 1 <= hop <= n_high, shift = (n_low - n_high) / (2 hop) an integer (e.g. 16384 / 4096 at hop 128 ... 1024,
 * 8192 / 2048 at hop 128 or 256), split_row a multiple of 4 with 64 <= split_row <= rows - 64, L >= n_low; anything else is
 * EMSPEC_ERR_INVALID_ARG with a message naming the rule.
 * emspec_multires_shift: the shift, or -1 for a shape (n_low, n_high, hop) that is not accepted.
 * emspec_multires_columns: the column count (= emspec_num_columns(L, n_low, hop)), 0 when L < n_low, -1 for a shape
 *   that is not accepted.
 * emspec_batch_multires: host buffers, page-locked or not ([S][L] in, [S][columns][rows] (+[4]) out, any output NULL):
 *   runs the same pipeline as emspec_batch (units of whole streams), helper threads included; returns when the outputs are
 *   written.
 * emspec_batch_multires_device: device buffers, enqueued on hip_stream (NULL = the default stream); does not synchronise.
 * Both bands' raw dB live in an engine workspace bounded like the records path's (streams are processed in chunks).
 * Single-resolution results on the same engine are not affected by a multi-resolution call.
 */
int64_t emspec_multires_columns(int64_t L, int32_t n_low, int32_t n_high, int32_t hop);
int32_t emspec_multires_shift(int32_t n_low, int32_t n_high, int32_t hop);
int emspec_batch_multires(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n_low, int32_t n_high,
                          int32_t hop, int32_t split_row, int32_t reassign, const emspec_out* out);
int emspec_batch_multires_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n_low,
                                 int32_t n_high, int32_t hop, int32_t split_row, int32_t reassign,
                                 float* db_dev, uint8_t* rgba_dev, uint8_t* index_dev, void* hip_stream);

/*
 * Multi-band batch: the image above with up to four FFT sizes, the constant-Q-like ladder - e.g. 16384 below
 * 250 Hz, 4096 up to 2 kHz and 1024 above, so that the bass resolves to 3 Hz while a hi-hat keeps its column.  `bands` = K,
 * 2 <= K <= 4, FFT sizes n[0] > n[1] > ... > n[K-1], each in {1024, 2048, 4096, 8192, 16384}; ONE hop and ONE reassign for all
 * bands; K - 1 split rows split_rows[0] < ... < split_rows[K-2].  Band k owns the rows [lo_k, hi_k), lo_0 = 0, lo_k =
 * split_rows[k-1], hi_k = split_rows[k], hi_{K-1} = rows, and with shift[k] = (n[0] - n[k]) / (2 hop)
 *     image[s][c][r] = single(n[k])[s][c + shift[k]][r]      for lo_k <= r < hi_k,  c in [0, columns)
 * where columns = emspec_num_columns(L, n[0], hop) and single(n) is what emspec_batch delivers at that n on the same engine and
 * row table (same hop and reassign): column c is centred at sample c * hop + n[0] / 2 in every band.  dB, palette index and RGBA
 * are single(n[k])'s bytes (EXACT mode: bit for bit); with the display post-process on (emspec_set_display) it runs once over
 * the composed raw dB, by the law of a single-resolution batch.  For K = 2 the image is that of emspec_batch_multires.
 * Accepted: K in 2..4; sizes from the set above, strictly decreasing; 1 <= hop <= n[K-1]; every shift[k] an integer; every split
 * row a multiple of 4; every band at least 64 rows high (split_rows[0] >= 64, split_rows[k] - split_rows[k-1] >= 64, rows -
 * split_rows[K-2] >= 64); L >= n[0]; S in 1..65535.  Anything else is EMSPEC_ERR_INVALID_ARG with a message naming the rule; the
 * engine stays usable.
 * emspec_multiband_shifts: 0 and, when shifts_out is not NULL, the K shifts - or -1 for a shape (bands, n, hop) not accepted.
 * emspec_multiband_columns: the column count, 0 when L < n[0], -1 for a shape that is not accepted.
 * emspec_batch_multiband / _device: as emspec_batch_multires / _device in every other respect - any output NULL; the device entry
 *   is enqueued on hip_stream and does not synchronise; the host entry takes page-locked or pageable buffers and runs the host
 *   pipeline over units of whole streams.  Both honour emspec_set_time_reduce and emspec_set_display; the host entry honours
 *   emspec_set_wave_out with the envelope on the n[0] column grid.  The bands' raw dB share the two-band batch's engine workspace.
 * Single-resolution and two-band results on the same engine are not affected by a multi-band call.
 * Not offered: a multi-band form of emspec_batch_gather, of the packed entries and of the batch PCM entries; more than four
 * bands; per-band hops.  (The live form: emspec_columns_multiband and emspec_push_samples_multiband, below.)
 */
int emspec_multiband_shifts(int32_t bands, const int32_t* n, int32_t hop, int32_t* shifts_out /* [bands], may be NULL */);
int64_t emspec_multiband_columns(int64_t L, int32_t bands, const int32_t* n, int32_t hop);
int emspec_batch_multiband_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t bands, const int32_t* n,
                                  const int32_t* split_rows /* [bands-1] */, int32_t hop, int32_t reassign, float* db_dev,
                                  uint8_t* rgba_dev, uint8_t* index_dev, void* hip_stream);
int emspec_batch_multiband(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t bands, const int32_t* n,
                           const int32_t* split_rows, int32_t hop, int32_t reassign, const emspec_out* out);

/*
 * Multi-resolution LIVE session: the image above, column by column while the audio arrives.  These
 * calls open the engine's live multi-stream session (the one emspec_columns / emspec_push_samples_multi open) as a
 * multi-resolution session; streams = 1 is the one-stream renderer.  For a stream that was fed samples [0, L) and then
 * flushed, the emspec_multires_columns(L, ...) emitted columns are those of emspec_batch_multires on the same samples
 * (EXACT mode: bit for bit; FAST mode: sums in arrival order).  Latency: emspec_latency_columns(n_low, hop, reassign).
 * The short band needs no samples of its own: frame j of n_low ends where frame j + 2 shift of n_high ends, so a call
 * advances both bands by the same number of frames (a stream's first frame runs the short band's frames 0 .. 2 shift).
 * Per call: one frame launch per band (each band's last workgroup of a stream writes its own rows of the output column in
 * place), one host synchronisation.  With emspec_set_display on, the post-process runs once over the composed raw column.
 * emspec_columns_multires: as emspec_columns, frames [streams][n_low].
 * emspec_push_samples_multires: as emspec_push_samples_multi; max_columns must hold what the block completes
 *   (emspec_push_columns_multires) even when both outputs are NULL - EMSPEC_ERR_INVALID_ARG otherwise, nothing fed.
 * emspec_push_columns_multires: as emspec_push_columns_multi (-1 for a shape that is not accepted).
 * emspec_columns_flush, emspec_reset_stream, emspec_reset and emspec_live_streams act on the session as on a
 * single-resolution one.  Shapes, split rows and their messages: those of emspec_batch_multires.  EMSPEC_ERR_STATE until
 * emspec_reset(): a single-resolution live call on a multi-resolution session or the reverse; a change of streams, n_low,
 * n_high, hop, split_row, reassign or feeding form mid-session; feeding a flushed stream.
 */
int emspec_columns_multires(emspec_engine* e, const float* frames /* [streams][n_low] */, int32_t streams, int32_t n_low,
                            int32_t n_high, int32_t hop, int32_t split_row, int32_t reassign, float* out_db,
                            uint8_t* out_rgba, int32_t rows, int64_t* out_columns);
int64_t emspec_push_columns_multires(const emspec_engine* e, int64_t count, int32_t n_low, int32_t n_high, int32_t hop,
                                     int32_t reassign);
int emspec_push_samples_multires(emspec_engine* e, const float* samples, int32_t streams, int64_t count, int64_t stride,
                                 int32_t n_low, int32_t n_high, int32_t hop, int32_t split_row, int32_t reassign,
                                 float* out_db, uint8_t* out_rgba, int32_t rows, int64_t max_columns, int64_t* out_counts,
                                 int64_t* out_first_columns);

/*
 * Multi-band LIVE session: the multi-band image, column by column while the audio arrives - what the
 * multi-resolution live session is to emspec_batch_multires, for K = `bands` in 2..4.  These calls open the engine's live
 * multi-stream session as a multi-band session.  For a stream that was fed samples [0, L) and then flushed, the
 * emspec_multiband_columns(L, ...) emitted columns are those of emspec_batch_multiband on the same samples, engine and row table
 * (EXACT mode: bit for bit, dB and RGBA; FAST mode: sums in arrival order).  Latency: emspec_latency_columns(n[0], hop, reassign).
 * Only n[0]'s frame count drives a call: band k runs 2 shift[k] frames ahead on the same samples (a stream's first frame runs its
 * frames 0 .. 2 shift[k]) and keeps a column ring of its own, indexed by the emitted column.
 * Per call: one frame launch per band - the first moves the new samples into the device ring, the others are not launched when no
 * stream has a frame.  When no band's finalize is deferred, each band's last workgroup of a stream writes its own rows of the
 * output column in place; when any band's would be (a call that completes more than two columns per stream, or a band with
 * n < 2048), every frame launch only scatters and ONE further kernel finalises all bands' rows: at most K + 1 launches.  A flush
 * is one launch.  With emspec_set_display on, the post-process runs once over the composed raw column; the overlays
 * (emspec_set_live_peaks, emspec_set_live_wave) run once, the envelope on the n[0] grid.  One host synchronisation ends the call.
 * emspec_columns_multiband: as emspec_columns, frames [streams][n[0]].
 * emspec_push_samples_multiband: as emspec_push_samples_multi; max_columns must hold what the block completes
 *   (emspec_push_columns_multiband) even when both outputs are NULL - EMSPEC_ERR_INVALID_ARG otherwise, nothing fed.
 * emspec_push_columns_multiband: as emspec_push_columns_multi (-1 for a shape that is not accepted).
 * emspec_push_samples_pcm_multiband: the session fed raw interleaved frames, as emspec_push_samples_pcm_multires (PCM front end,
 *   below).
 * emspec_columns_flush, emspec_reset_stream, emspec_reset, emspec_live_streams, emspec_set_live_peaks, emspec_set_live_wave and
 * emspec_set_display act on the session as on a two-band one.  Shapes, split rows and their messages: those of
 * emspec_batch_multiband (EMSPEC_ERR_INVALID_ARG before anything is fed; the engine stays usable).  K = 2 is accepted with the
 * band rule's sizes; its columns are those of the two-band live session.  EMSPEC_ERR_STATE until emspec_reset(): a
 * single-resolution or two-band live call on a multi-band session or the reverse; a change of streams, bands, any size, any split
 * row, hop, reassign or feeding form mid-session; feeding a flushed stream; any of these calls while a time reduction is set.
 */
int emspec_columns_multiband(emspec_engine* e, const float* frames /* [streams][n[0]] */, int32_t streams, int32_t bands,
                             const int32_t* n, const int32_t* split_rows /* [bands-1] */, int32_t hop, int32_t reassign,
                             float* out_db, uint8_t* out_rgba, int32_t rows, int64_t* out_columns);
int64_t emspec_push_columns_multiband(const emspec_engine* e, int64_t count, int32_t bands, const int32_t* n, int32_t hop,
                                      int32_t reassign);
int emspec_push_samples_multiband(emspec_engine* e, const float* samples, int32_t streams, int64_t count, int64_t stride,
                                  int32_t bands, const int32_t* n, const int32_t* split_rows, int32_t hop, int32_t reassign,
                                  float* out_db, uint8_t* out_rgba, int32_t rows, int64_t max_columns, int64_t* out_counts,
                                  int64_t* out_first_columns);

/*
 * ---- PCM front end: the buffer an audio source really delivers - interleaved channels of int16,
 * packed 24-bit, int32 or float32 samples - crosses PCIe as it is, and ONE kernel on the device converts and mixes it into
 * the mono float32 streams every entry point above takes.  Serves: the reference's use ("optimized for music production and
 * mixing", README.md) - the left, right, mid and side views of one stereo capture buffer or WAV file - without a
 * de-interleave / convert / down-mix pass in JavaScript; [BUILD-DEFINED].  Little endian, signed; no resampling.
 *
 * A SOURCE is one interleaved recording ([frames][channels]); it yields `views` STREAMS, stream index = source * views + view,
 * and every output is laid out [sources * views][columns][rows] exactly as emspec_batch lays out [S][columns][rows].
 * Sample t of view v, with x_c the converted sample of channel c (EMSPEC_PCM_* below; the S16 and S24 conversions are exact):
 *     acc = mix[v][0] * x_0;   then for c = 1 .. channels-1:   acc = acc + mix[v][c] * x_c
 * every product and every sum rounded to binary32, channels in ascending order, no fused multiply-add: bit-reproducible
 * (mid / side with weights +-0.5 is exact).  DEFINITION of every PCM entry point: its result is the result of the
 * corresponding float entry point on the float32 array this decode yields.  The EXACT mode's input bound (|x| <= 4) applies
 * to the MIXED value.
 * Format errors are EMSPEC_ERR_INVALID_ARG with a message naming the field: sample_type not an EMSPEC_PCM_*, channels or views
 * outside 1..8, reserved != 0, a weight among the first views * channels that is not finite.
 */
#define EMSPEC_PCM_S16 1   /* int16 little endian                          value = s * 2^-15 */
#define EMSPEC_PCM_S24 2   /* 3 bytes little endian, packed (frame = 3*channels bytes)  s * 2^-23 */
#define EMSPEC_PCM_S32 3   /* int32: (float)s rounded to nearest even, then * 2^-31 */
#define EMSPEC_PCM_F32 4   /* float32, taken as is */
#define EMSPEC_PCM_MAX_CHANNELS 8
#define EMSPEC_PCM_MAX_VIEWS 8
typedef struct emspec_pcm_format {
    int32_t sample_type;   /* EMSPEC_PCM_* */
    int32_t channels;      /* interleaved channels per frame, 1..8 */
    int32_t views;         /* streams produced per source, 1..8 */
    int32_t reserved;      /* 0 */
    float mix[EMSPEC_PCM_MAX_VIEWS * EMSPEC_PCM_MAX_CHANNELS];   /* [views][channels], row-major, first views*channels used */
} emspec_pcm_format;

/* Bytes per interleaved frame (2 / 3 / 4 / 4 x channels); -1 for an invalid format or NULL.  No engine. */
int64_t emspec_pcm_frame_bytes(const emspec_pcm_format* fmt);

/*
 * The decode kernel by itself, for callers that keep their audio on the device (with emspec_batch_device,
 * emspec_batch_multires_device, emspec_parity_dump_device it gives the PCM form of every device entry).  src_dev: `frames`
 * frames of each of `sources` sources, source i at src_dev + i * src_stride_bytes (src_stride_bytes >= frames * frame bytes;
 * pointer and stride any multiple of the sample size - 1 for S24); device memory or page-locked host memory
 * (emspec_host_alloc), which the kernel reads in place.  pcm_dev [sources * views][frames] float32 on the engine's device.
 * Enqueued on hip_stream (NULL = the default stream); does not synchronise.  sources, frames >= 0.
 */
int emspec_pcm_decode_device(emspec_engine* e, const void* src_dev, const emspec_pcm_format* fmt, int32_t sources,
                             int64_t frames, int64_t src_stride_bytes, float* pcm_dev, void* hip_stream);

/*
 * emspec_batch / emspec_batch_packed from raw frames.  src: host memory (page-locked or not), [sources][frames][channels]
 * samples of fmt->sample_type, tightly packed.  Outputs / wire images as the float entries produce them for sources * views
 * streams of `frames` samples (offsets: sources * views + 1 entries).  The same pipeline: its copy-in stage moves the raw
 * bytes (frames * frame bytes per source instead of 4 bytes per stream sample - a sixteenth for four views of 16-bit stereo)
 * and the decode kernel runs in front of each unit's kernels; units are whole sources, or runs of columns of one source when
 * there are few.  Errors: those of the float entries, and the format's.
 */
int emspec_batch_pcm(emspec_engine* e, const void* src, const emspec_pcm_format* fmt, int32_t sources, int64_t frames,
                     int32_t n, int32_t hop, int32_t reassign, const emspec_out* out);
int emspec_batch_pcm_packed(emspec_engine* e, const void* src, const emspec_pcm_format* fmt, int32_t sources, int64_t frames,
                            int32_t fft_size, int32_t hop, int32_t reassign, uint8_t* wire, int64_t wire_capacity,
                            int64_t* offsets);

/*
 * Live session from raw frames: emspec_push_samples_multi / emspec_push_samples_multires for sources * views streams, fed
 * `count` frames of every source per call, source i at block + i * stride_bytes (stride_bytes >= count * frame bytes; host
 * memory, page-locked or not).  The session is the engine's live multi-stream session in its per-sample-block form; the
 * format (sample type, channels, views, weights) is fixed by the first call.  The raw frames join a page-locked staging block
 * (a block that completes no frame costs no launch); at launch time the decode kernel reads it in place and the frame kernels
 * read the decoded block on the device.  Outputs, counts and first columns per STREAM, as emspec_push_samples_multi lays them
 * out; max_columns must hold what the block completes (emspec_push_columns_multi / _multires) even when both outputs are NULL -
 * EMSPEC_ERR_INVALID_ARG otherwise, nothing fed.  emspec_columns_flush, emspec_reset_stream (per view stream; the other views
 * of its source continue), emspec_reset, emspec_live_streams (= sources * views) and emspec_push_columns_multi / _multires
 * act as on any session.  EMSPEC_ERR_STATE until emspec_reset(): a float live call on a PCM session or the reverse, a change
 * of format, sources or shape mid-session, feeding a flushed stream.  "The same format" means the same sample type, channels,
 * views and the same BITS of the views * channels weights (-0.0 is not 0.0: the sign of a zero result can differ).
 * sources * views, the session's streams, must be in 1..65535 as for every live session (EMSPEC_ERR_INVALID_ARG).
 * emspec_push_samples_pcm_multiband: the same for the multi-band live session (emspec_push_samples_multiband).
 */
int emspec_push_samples_pcm(emspec_engine* e, const void* block, const emspec_pcm_format* fmt, int32_t sources, int64_t count,
                            int64_t stride_bytes, int32_t n, int32_t hop, int32_t reassign, float* out_db, uint8_t* out_rgba,
                            int32_t rows, int64_t max_columns, int64_t* out_counts, int64_t* out_first_columns);
int emspec_push_samples_pcm_multires(emspec_engine* e, const void* block, const emspec_pcm_format* fmt, int32_t sources,
                                     int64_t count, int64_t stride_bytes, int32_t n_low, int32_t n_high, int32_t hop,
                                     int32_t split_row, int32_t reassign, float* out_db, uint8_t* out_rgba, int32_t rows,
                                     int64_t max_columns, int64_t* out_counts, int64_t* out_first_columns);
int emspec_push_samples_pcm_multiband(emspec_engine* e, const void* block, const emspec_pcm_format* fmt, int32_t sources,
                                      int64_t count, int64_t stride_bytes, int32_t bands, const int32_t* n,
                                      const int32_t* split_rows, int32_t hop, int32_t reassign, float* out_db, uint8_t* out_rgba,
                                      int32_t rows, int64_t max_columns, int64_t* out_counts, int64_t* out_first_columns);

/*
 * ---- Spectral peaks: the k loudest local maxima of every finished column, computed where the dB
 * columns already are.  Serves: the note and frequency read-out the reference shows on hover (README.md:39), a tuner line, a
 * note overlay, melody or partial tracks - a peak list of k = 8 is 64 bytes per column where the dB column is 4 KB;
 * [BUILD-DEFINED].
 *
 * DEFINITION.  The peaks of a column are a function of its dB values x[0 .. R) and of k (1 .. 32) and min_db (not NaN).  All
 * arithmetic is binary32, one rounding per operation, no fused multiply-add; the division is the IEEE one.
 *   1. Candidates.  L = x[r-1], or -inf at r = 0;  Rn = x[r+1], or -inf at r = R-1.  Row r is a peak iff
 *          x[r] >= min_db && x[r] > L && x[r] >= Rn
 *      by plain float comparisons: -0.0 equals +0.0; a NaN is never a peak and never beats a neighbour; a plateau reports its
 *      first row.
 *   2. Value.  db = x[r], the cell's own bits; the height is not interpolated.
 *   3. Position, in row units; row r spans [r, r+1) of the engine's edge table (emspec_get_row_edges_hz).  At r = 0 and
 *      r = R-1, pos = (float)r + 0.5f.  Elsewhere with a = L, b = x[r], c = Rn:
 *          t = a - c;   u = (a - b) + (c - b);   d = (0.5f * t) / u;
 *          if (d > 0.5f) d = 0.5f;   if (d < -0.5f) d = -0.5f;   if (d != d) d = 0.0f;
 *          pos = ((float)r + 0.5f) + d;
 *      - the vertex of the parabola through the three dB values, negative towards the louder left neighbour.
 *   4. Selection.  The k candidates that come first by db descending (float comparison), ties by ascending row, in that order
 *      into peaks[column][0 .. k); the slots that remain hold pos = -1.0f, db = -INFINITY.
 * What the position resolves: with reassignment on, a steady tone falls into ONE row and its neighbours sit at the -200 dB
 * floor, so d is about 0 and the resolution is the row width - 12 cents at the default 1,024 rows, 3 cents at 4,096.  The
 * parabola matters with reassign = 0 and for modulated partials.
 */
typedef struct emspec_peak { float pos; float db; } emspec_peak;   /* 8 bytes */

/*
 * The peaks of any [columns][rows] float32 dB array on the engine's device - the output of emspec_batch_device or of
 * emspec_batch_multires_device, streams x columns flattened (a column's peaks depend on that column alone) - into
 * peaks_dev[columns][k].  rows % 4 == 0 and 4 <= rows <= 4096 (not necessarily the engine's); columns >= 0, 0 is a no-op;
 * db_dev 16-byte and peaks_dev 8-byte aligned; no limit on columns * rows but memory.  One pass over the array.  Enqueued on
 * hip_stream (NULL = the default stream); does not synchronise.
 */
int emspec_peaks_device(emspec_engine* e, const float* db_dev, int64_t columns, int32_t rows, int32_t k, float min_db,
                        emspec_peak* peaks_dev, void* hip_stream);
/* The same definition in plain C++ on host arrays: no engine, no device (the twin emspec_wire_unpack_host is for the wire
 * image).  Serves the live calls' host columns and emspec_batch_multires.  The message of a refusal: emspec_last_error(NULL). */
int emspec_peaks_host(const float* db, int64_t columns, int32_t rows, int32_t k, float min_db, emspec_peak* peaks_out);
/*
 * peaks[S][C][k], C = emspec_num_columns(L, n, hop): the peaks of exactly the dB emspec_batch_device / emspec_batch would
 * deliver, display post-process included - without that dB leaving the device.  The device entry keeps the dB of a chunk of
 * streams in an engine workspace bounded like the records path's; the host entry runs the pipeline of emspec_batch (pinned or
 * pageable buffers, units of whole streams or runs of columns of a long stream) and copies out the peak lists only.
 * The engine's rows must satisfy the rule of emspec_peaks_device.  EMSPEC_ERR_STATE while a time reduction is set
 * (emspec_set_time_reduce; a host reduces 64-byte lists itself) - emspec_peaks_device / _host are not affected.
 */
int emspec_batch_peaks_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n, int32_t hop,
                              int32_t reassign, int32_t k, float min_db, emspec_peak* peaks_dev, void* hip_stream);
int emspec_batch_peaks(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t reassign,
                       int32_t k, float min_db, emspec_peak* peaks_out);
/*
 * A position in row units -> Hz on the engine's row axis: with i = floor(pos) clamped to [0, rows-1],
 *     hz = edge[i] * (edge[i+1] / edge[i]) ^ (pos - i)
 * in binary64 from the float table emspec_get_row_edges_hz returns.  pos outside [0, rows] (or NaN): EMSPEC_ERR_INVALID_ARG.
 */
int emspec_position_hz(emspec_engine* e, float pos, double* hz);
/* Every refusal above is EMSPEC_ERR_INVALID_ARG with a message naming the rule - k outside 1 .. 32, a NaN min_db, rows breaking
 * the rule, null or misaligned pointers - and leaves the engine usable. */

/*
 * ---- Waveform envelope: the smallest and the largest sample under each delivered column, computed
 * where the samples already are.  Serves: the waveform lane a viewer draws beside the spectrogram, also zoomed out
 * (emspec_set_time_reduce) and for the views of a PCM source, whose float streams exist in no host buffer; [BUILD-DEFINED].
 *
 * DEFINITION.  A stream of L samples, FFT size n, hop (1 <= hop <= n), factor f (1 .. 65536); C = emspec_num_columns(L, n, hop),
 * Cr = emspec_reduced_columns(C, f), off = n / 2 - hop / 2 (integer divisions).  The envelope is Cr pairs; pair g covers
 *     W(g) = [ g f hop + off,  min((g + 1) f, C) hop + off )
 * - at f = 1 the hop samples centred on column g's centre g hop + n / 2.  The windows tile [off, off + C hop) without gap or
 * overlap, and each lies inside the frames of its own columns (off + hop <= n).
 *   Order.  For a sample that is not NaN, u its 32 bits:  key = (u & 0x80000000) ? ~u : (u | 0x80000000), unsigned - the total
 *   order of the floats with -0.0 below +0.0.  lo is the sample of W(g) with the smallest key, hi the one with the largest, each
 *   with its own bits.  NaN samples are skipped; a window without a sample that is not NaN gives lo = +INFINITY, hi = -INFINITY.
 * The pair is a function of the window's bits alone: it does not depend on the order of evaluation, on how the work is split,
 * or on the engine's mode, and the pair at factor f is the key-min / key-max of the f = 1 pairs of its group (the peak-hold
 * rule of the reduced columns it sits under).  For the PCM entries the samples are the decoded, mixed float32 values of the
 * views; for emspec_batch_multires the column grid is the long band's, n = n_low
 * (emspec_batch_multiband: n = n[0]).
 * The live calls deliver it through emspec_set_live_wave (below).  Sums - RMS, correlation - are the level meters' (next section):
 * a float sum depends on its order, so they are summed as integers.
 */
typedef struct emspec_wave { float lo; float hi; } emspec_wave;   /* 8 bytes */

/*
 * The envelope of S device-resident streams, pcm_dev [S][L] laid out as for emspec_batch_device but 4-byte aligned only, into
 * wave_dev [S][Cr] (8-byte aligned).  S in 0 .. 65535; S = 0 or C = 0 (L < n) is a no-op; n follows the FFT-size rule of the
 * batch entries, hop in 1 .. n, factor in 1 .. 65536 - its own argument: the engine's time reduction and mode play no part.
 * One pass over the samples.  Enqueued on hip_stream (NULL = the default stream); does not synchronise.  It is what a caller of
 * the device batch entries uses; those entries do not change.
 */
int emspec_wave_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor,
                       emspec_wave* wave_dev, void* hip_stream);
/* The same definition in plain C++ on host arrays: no engine, no device.  The message of a refusal: emspec_last_error(NULL). */
int emspec_wave_host(const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor, emspec_wave* wave_out);
/*
 * While set, every entry that runs the host pipeline - emspec_batch, _packed, _pcm, _pcm_packed, _multires, _multiband and
 * emspec_batch_peaks - also writes the envelope of its streams to wave_out[streams][Cr], in the same pass, from each unit's
 * staged samples: f = the engine's time reduction, streams = S, or sources x views for the PCM entries.  capacity counts
 * pairs; a call with streams x Cr > capacity returns EMSPEC_ERR_INVALID_ARG before anything runs.  wave_out is 4-byte aligned
 * host memory, page-locked or pageable, and must stay valid while set; its contents are undefined after an error return.
 * NULL clears it.  emspec_batch_gather returns EMSPEC_ERR_STATE while it is set; device entries and streaming calls are not
 * affected.
 */
int emspec_set_wave_out(emspec_engine* e, emspec_wave* wave_out, int64_t capacity /* pairs */);
/* Every refusal above is EMSPEC_ERR_INVALID_ARG with a message naming the rule - a factor outside 1 .. 65536, a hop outside
 * 1 .. n, an unsupported n, S outside 0 .. 65535, null or misaligned pointers, a negative capacity - and leaves the engine usable. */

/*
 * ---- Level meters: exact RMS, peak and pair correlation of the samples under each delivered column.
 * Serves: the level meter a viewer draws beside the waveform lane and the correlation meter beside a stereo image, also zoomed
 * out and for the views of a PCM source, whose float streams exist in no host buffer; [BUILD-DEFINED].
 *
 * DEFINITION.  The windows are the envelope's: L, n, hop, factor f, C, Cr and off as above, record g covers W(g).
 *   Quantiser.  A sample x with bits u gives an integer k in units of 2^-24.  A NaN gives k = 0 and counts in `odd`.  Otherwise
 *   k = x 2^24 rounded to nearest, ties to even, saturated to +-(2^31 - 1); a saturated sample - |x| >= 128, or an infinity -
 *   also counts in `odd`.  The product x 2^24 is exact in binary32, and every |x| <= 2^-25 gives 0, so k does not depend on
 *   how denormals are handled and can be evaluated from the bits in integers.  s16 and s24 PCM are represented exactly; the
 *   floor is -144 dBFS, the ceiling +42 dBFS.
 *   Level record.  Over the samples of W(g), with q = k^2 (below 2^62):
 *       sq_lo = sum of (q & 0xffffffff),  sq_hi = sum of (q >> 32),  peak = max |k|,  odd = the count above
 *   so that the sum of k^2 is sq_hi 2^32 + sq_lo.  A window has at most 2^30 samples: no limb overflows.
 *   Cross record of a pair of streams (A, B).  With p = k_A k_B (int64):
 *       lo = sum of ((uint64)p & 0xffffffff),  hi = sum of (p >> 32, arithmetic shift)
 *   so that the sum of k_A k_B is hi 2^32 + lo.
 * LAWS.  The limbs are deliberately not normalised.  Every field is a sum or a maximum of integers: a record does not depend on
 * the order of evaluation, on how the work is split, or on the engine's mode - device, host, FAST and EXACT give the same bytes.
 * The record at factor f is the field-wise sum (peak: maximum) of the f = 1 records of its group.  For the PCM entries the
 * samples are the decoded, mixed float32 values of the views.
 */
typedef struct emspec_level { uint64_t sq_lo; uint64_t sq_hi; uint32_t peak; uint32_t odd; } emspec_level;   /* 24 bytes */
typedef struct emspec_cross { uint64_t lo; int64_t hi; } emspec_cross;                                         /* 16 bytes */

/*
 * The level records of S device-resident streams, pcm_dev [S][L] (4-byte aligned), into level_dev [S][Cr] (8-byte aligned).
 * Arguments and refusals as for emspec_wave_device; `factor` is the call's own.  One pass over the samples.  Enqueued on
 * hip_stream (NULL = the default stream); does not synchronise.
 */
int emspec_level_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor,
                        emspec_level* level_dev, void* hip_stream);
/* The same definition in plain C++ on host arrays: no engine, no device.  The message of a refusal: emspec_last_error(NULL). */
int emspec_level_host(const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor, emspec_level* level_out);
/*
 * The cross records of `pairs` pairs of device-resident streams: pair p is streams p views + a and p views + b of
 * pcm_dev [pairs views][L] - the addressing of emspec_stereo_device, but a == b is allowed (the cross limbs then are the level's
 * sums) - into cross_dev [pairs][Cr] (8-byte aligned).  views in 1 .. 64, a and b in 0 .. views - 1, pairs views <= 65535;
 * otherwise as emspec_level_device.
 */
int emspec_cross_device(emspec_engine* e, const float* pcm_dev, int32_t pairs, int32_t views, int32_t a, int32_t b, int64_t L, int32_t n,
                        int32_t hop, int32_t factor, emspec_cross* cross_dev, void* hip_stream);
int emspec_cross_host(const float* pcm, int32_t pairs, int32_t views, int32_t a, int32_t b, int64_t L, int32_t n, int32_t hop,
                      int32_t factor, emspec_cross* cross_out);
/*
 * While set, every entry that honours emspec_set_wave_out also writes the level records of its streams to
 * level_out[streams][Cr], in the same pass, from each unit's staged samples; f, streams, capacity (in records), validity and
 * the contents after an error return follow emspec_set_wave_out's rules.  level_out is 8-byte aligned host memory.  NULL clears
 * it.  emspec_batch_gather returns EMSPEC_ERR_STATE while it is set.
 */
int emspec_set_level_out(emspec_engine* e, emspec_level* level_out, int64_t capacity /* records */);
/*
 * While set, the PCM host entries - emspec_batch_pcm, _pcm_packed, _pcm_stereo - also write the cross records of views a and b
 * of each source to cross_out[sources][Cr] (8-byte aligned host memory; capacity in records).  a or b outside the call's views
 * gives EMSPEC_ERR_INVALID_ARG before anything runs, as does sources x Cr > capacity.  While it is set, the host entries on
 * float streams and emspec_batch_gather return EMSPEC_ERR_STATE.  NULL clears it.
 */
int emspec_set_cross_out(emspec_engine* e, int32_t a, int32_t b, emspec_cross* cross_out, int64_t capacity /* records */);
/*
 * Pure helpers, binary64, no engine.  emspec_level_window: the samples in W(g) (0 where there is no such window).
 * emspec_level_values: rms_db = 10 log10((ldexp((double)sq_hi, 32) + (double)sq_lo) / samples) - 20 log10(2^24), -INFINITY for a
 * zero sum; peak_db likewise from `peak`; either pointer may be null.  emspec_cross_correlation: rho = sum ab / sqrt(sum a^2
 * sum b^2), clamped to [-1, 1]; 0 for a zero denominator.  They return EMSPEC_ERR_INVALID_ARG for a null record or samples < 1.
 */
int64_t emspec_level_window(int64_t L, int32_t n, int32_t hop, int32_t factor, int64_t g);
int emspec_level_values(const emspec_level* level, int64_t samples, double* rms_db, double* peak_db);
int emspec_cross_correlation(const emspec_level* a, const emspec_level* b, const emspec_cross* ab, double* rho);
/* Every refusal above is EMSPEC_ERR_INVALID_ARG with a message naming the rule - those of the envelope's entries, an output that
 * is not 8-byte aligned, views outside 1 .. 64, a or b outside 0 .. views - 1, pairs views > 65535 - and leaves the engine usable. */

/*
 * ---- Overlays of the streaming calls: the spectral peaks of every column a live call delivers
 * and the waveform envelope of the samples under it, written by one more kernel behind the call's launch.  Serves: a live
 * viewer's note / frequency read-out and the waveform it draws beside the scrolling image - 64 bytes of peaks per column
 * instead of the 4 KB dB column over PCIe, and the envelope of a PCM session's views, whose float streams exist in no host
 * buffer; [BUILD-DEFINED].
 *
 * While a setting is on, every streaming call on either session of the engine - emspec_column, emspec_column_flush,
 * emspec_push_samples; emspec_columns, emspec_columns_flush, emspec_push_samples_multi; the _multires forms;
 * emspec_push_samples_pcm and _pcm_multires - also writes the overlay, for exactly the column slots it writes.  A call delivers
 * its dB as [S][cols][rows] (cols = 1 for the per-frame calls and the flushes, max_columns for the push calls); the same call
 * writes
 *     peaks_out[(s * cols + slot) * k + i],  i in 0 .. k-1        and        wave_out[s * cols + slot]
 * and leaves the other slots untouched; out_columns / out_counts / out_first_columns mean what they mean without overlays.
 * A push call with an overlay on must fit max_columns like one with an output.  A call with S * cols * k (peaks) or S * cols
 * (envelope) above the capacity returns EMSPEC_ERR_INVALID_ARG before anything is fed; the session stays as it was.
 * Both arrays are host memory, 4-byte aligned, valid while set: page-locked (emspec_host_alloc, 8-byte aligned) they are
 * written in place by the kernel, pageable they are staged and copied after the call's synchronisation, as out_db is.  NULL
 * clears a setting; with both cleared the calls launch, allocate and write exactly what they did before these entries.
 *
 * Peaks: those of emspec_peaks_host(k, min_db) applied to the dB column the call delivers - the post-processed column with
 * emspec_set_display on, the composed column of a multi-resolution session, the empty column "-1" of the per-frame form - so
 * byte-equal to emspec_peaks_host on the delivered bytes in both modes; written whether or not out_db is given (a renderer
 * that takes RGBA only still gets them).  Stateless: set, changed or cleared between any two calls.
 * EMSPEC_ERR_INVALID_ARG: k outside 1 .. 32, a NaN min_db, a negative capacity, engine rows that break the rule of
 * emspec_peaks_device (rows % 4 == 0, 4 <= rows <= 4096).
 *
 * Envelope: the pair of the definition above at factor 1 on the session's grid - n the session's FFT size (n_low for a
 * multi-resolution session), column c covers the samples [c hop + off, c hop + off + hop) of its stream, off = n / 2 - hop / 2;
 * the empty column of the per-frame form gives (+INFINITY, -INFINITY).  For a stream fed [0, L) and then flushed the emitted
 * pairs are byte-equal to emspec_wave_host(pcm, 1, L, n, hop, 1), in both modes; for a PCM session the samples are the decoded,
 * mixed float32 values of each view.  The pair of column c is taken when frame c arrives and kept on the device until c is
 * emitted, so the setting needs the session's whole history: with a non-NULL array it returns EMSPEC_ERR_STATE while either
 * session has frames fed (emspec_reset first) or a time reduction is set.  emspec_reset_stream restarts that stream's envelope
 * with its columns.  Clearing is always allowed.
 */
int emspec_set_live_peaks(emspec_engine* e, int32_t k, float min_db, emspec_peak* peaks_out, int64_t capacity /* pairs */);
int emspec_set_live_wave(emspec_engine* e, emspec_wave* wave_out, int64_t capacity /* pairs */);
/*
 * Live level meters: the level record of every stream and the cross record of every pair of streams,
 * per emitted column, from the same kernel and the same walk over the samples as the envelope.  Serves the RMS / peak meter
 * beside the waveform lane and the correlation meter beside a stereo image of a LIVE session - for a PCM session the decoded
 * views exist in no host buffer; [BUILD-DEFINED].
 *
 * While a setting is on, every streaming call named above (and the _multiband forms), on either session, also writes, for
 * exactly the column slots it writes,
 *     level_out[s * cols + slot],  s in 0 .. S-1        and        cross_out[p * cols + slot],  p in 0 .. S / views - 1
 * with cols as above, and leaves the other slots untouched.  Pair p is the streams p views + a and p views + b of the session,
 * as in emspec_cross_device (a == b is allowed).
 * The record of column c is the factor-1 record of the level meters' DEFINITION over the samples [c hop + off, c hop + off + hop)
 * of the stream (of the pair), off = n / 2 - hop / 2, n the session's FFT size (n_low, n[0] for a multi-resolution or multi-band
 * session); it is taken when frame c arrives and kept on the device until column c is emitted; the empty column "-1" of the
 * per-frame form gives the all-zero record; for a PCM session the samples are the decoded, mixed float32 values of each view.
 * For a stream fed [0, L) and then flushed, the emitted records are byte-equal to emspec_level_host(pcm, 1, L, n, hop, 1, ...),
 * those of a pair to emspec_cross_host(pcm, pairs, views, a, b, L, n, hop, 1, ...), in both modes, in both feeding forms,
 * however the samples were cut into calls.
 *
 * Both arrays are host memory, valid while set, 8-byte aligned (else EMSPEC_ERR_INVALID_ARG, as for emspec_set_level_out):
 * page-locked they are written in place by the kernel, pageable they are staged and copied after the call's synchronisation.
 * capacity counts records: a call that needs more - S cols, respectively (S / views) cols - returns EMSPEC_ERR_INVALID_ARG
 * before anything is fed, and a push call with either setting on must fit max_columns like one with an output.  NULL clears a
 * setting, always; with every overlay cleared the calls launch, allocate and write what they did before these entries.
 * State: the envelope's rules - a non-NULL array is EMSPEC_ERR_STATE while either session has frames fed or a time reduction
 * above 1 is set; emspec_reset_stream restarts that stream's level records with its columns.
 * The cross: views in 1 .. 64, a and b in 0 .. views - 1 at set time (EMSPEC_ERR_INVALID_ARG).  A streaming call on a session
 * whose stream count is not a multiple of `views` returns EMSPEC_ERR_INVALID_ARG before anything is fed; the session stays as
 * it was.  The two streams of a pair must stay in step: WHILE A LIVE CROSS IS SET, emspec_reset_stream RETURNS
 * EMSPEC_ERR_STATE and changes nothing (emspec_reset restarts all streams together) - the one place where a set overlay changes
 * what another entry answers.  (A session whose streams emspec_reset_stream moved apart BEFORE the cross was set - possible
 * only while no stream has a frame yet - refuses its streaming calls with EMSPEC_ERR_STATE until emspec_reset.)
 *
 * emspec_level_sum / emspec_cross_sum: pure, no engine - the field-wise sum (peak: maximum) of count >= 1 records, i.e. the law
 * "the record at factor f is the sum of its f = 1 records" as a helper, so that a meter integrates 300 or 400 ms of per-hop
 * records without restating the limb rules.  out may be one of the records.  A null pointer, count < 1, or a sum that a limb
 * cannot hold returns EMSPEC_ERR_INVALID_ARG (emspec_last_error(NULL)) and leaves *out as it was.
 */
int emspec_set_live_level(emspec_engine* e, emspec_level* level_out, int64_t capacity /* records */);
int emspec_set_live_cross(emspec_engine* e, int32_t views, int32_t a, int32_t b, emspec_cross* cross_out, int64_t capacity /* records */);
int emspec_level_sum(const emspec_level* records, int64_t count, emspec_level* out);
int emspec_cross_sum(const emspec_cross* records, int64_t count, emspec_cross* out);

/*
 * ---- Live history: a ring on the device of the dB columns the streaming calls deliver, W per stream,
 * and views that read it back reduced in time and coloured by a law of the caller's.  Serves the events that make a live
 * renderer redraw its whole visible image - a change of "Scroll Speed" (columns per pixel), a window resize, pause and scroll
 * back, a change of "dB Range", "Gain", "Noise Gate" or "Color Map" - without the host keeping every 4 KB column of every stream
 * and taking maxima and colours on its own cores; [BUILD-DEFINED].  Off unless set; with it cleared the streaming calls launch,
 * allocate and write exactly what they did before these entries.  The streaming calls keep refusing emspec_set_time_reduce
 * factors above 1 (above): a view's factor is given per view.
 *
 * Columns are numbered per stream: column c is the c-th finished column the stream's session has emitted since the stream was
 * (re)started - the batch's column index, the number out_columns / out_first_columns speak of.  The empty column "-1" the
 * per-frame form delivers before the latency has passed is not a column and is not stored.
 * Stored is the dB column the call delivers, byte for byte - the post-processed column with emspec_set_display on, the composed
 * column of a multi-resolution or multi-band session, the decoded views' columns of a PCM session - whether or not the caller
 * asked for out_db; flush columns too.  Column c lives in slot c mod W (W need not be a power of two); after any call the ring
 * of a stream holds the columns [max(0, end - W), end), end = the number emitted so far; a launch that emits more than W columns
 * of a stream stores its last W.
 * While a history is set the delivered dB passes through a device block, as with emspec_set_live_peaks: a push call must fit
 * max_columns like one with an output (EMSPEC_ERR_INVALID_ARG before anything is fed), and page-locked outputs of more than
 * one launch's columns are staged.
 *
 * emspec_set_live_history(e, W): W columns per stream for both sessions of the engine; 0 clears and frees the rings (always
 *   allowed).  EMSPEC_ERR_INVALID_ARG: W outside 0 .. 2^20, engine rows not a multiple of 4.  EMSPEC_ERR_STATE: W > 0 while
 *   either session has frames fed (emspec_reset first).  A ring (streams x W x rows x 4 bytes) is allocated by the first
 *   streaming call of a session, when its streams are known: EMSPEC_ERR_OUT_OF_MEMORY on that call, before anything is fed;
 *   the session stays as it was.  emspec_reset empties every ring; emspec_reset_stream empties that stream's ring and restarts
 *   its numbering, the other streams keep theirs.
 * emspec_live_history(e, session, stream, &first): the number of columns stream `stream` of the session has emitted (`end`),
 *   and in *first (may be NULL) the first column held; -1 for a NULL engine, an unknown session or stream (a session that has
 *   not started has no streams), or no history.  session: EMSPEC_SESSION_MULTI (emspec_columns*, emspec_push_samples_multi /
 *   _multires / _multiband / _pcm*) or EMSPEC_SESSION_ONE (emspec_column, emspec_push_samples, emspec_column_flush).
 *
 * A view of streams [stream0, stream0 + streams): for g in [0, groups), with a = first_column and f = factor, group g covers the
 * columns a + g f .. min(a + (g + 1) f, end) - 1 of each stream (the last group may be short) and
 *     db   [s][g][r] = the peak hold of emspec_set_time_reduce over the group's stored bytes, in column order, same comparison
 *     index[s][g][r] = the palette index of db[s][g][r] + map->shift_db under the law of map (db_top, db_range, gate_db as in
 *                      emspec_config; map == NULL: the engine's configuration, shift 0)
 *     rgba [s][g][r] = LUT[index[s][g][r]], the colour map the engine holds when the view runs (emspec_set_colormap)
 * Layouts [streams][groups][rows] (+[4]); any output may be NULL, not all.  The dB output is NOT shifted.  The index is the
 * law applied to the stored dB - that is what lets a view re-colour after the fact: in EXACT mode without the display
 * post-process it is the law on the dB bytes, not the cell-derived index of the live RGBA, and may differ from it by one step
 * on a borderline cell.  db_range must be > 0 and no field NaN.
 * Required: first_column >= the first held column and first_column + (groups - 1) factor < end, for every addressed stream -
 * else EMSPEC_ERR_INVALID_ARG with a message naming the stream and its held range, nothing written.  Also
 * EMSPEC_ERR_INVALID_ARG: factor outside 1 .. 65536, groups < 1, streams < 1, a stream range outside the session, all outputs
 * NULL, a misaligned output.  EMSPEC_ERR_STATE: no history set, or a session that does not exist.  Every refusal leaves the
 * engine usable.
 * emspec_history_view_device: outputs are device memory (db_dev and rgba_dev 16-byte, index_dev 4-byte aligned); enqueues on
 *   hip_stream (NULL: the default stream, as for emspec_batch_device) behind the session's launches - every streaming call
 *   has synchronised before it returned - and does not synchronise; later streaming calls are ordered behind the view.  emspec_history_view: outputs are host arrays, page-locked (written in place) or pageable (staged through
 *   page-locked blocks), as out_db of the live calls; synchronises.
 */
#define EMSPEC_SESSION_MULTI 0   /* emspec_columns*, emspec_push_samples_multi / _multires / _multiband / _pcm* */
#define EMSPEC_SESSION_ONE   1   /* emspec_column, emspec_push_samples, emspec_column_flush */

typedef struct emspec_view_map {   /* the colour law of a view; NULL = the engine's configuration, shift 0 */
    float db_top, db_range, gate_db;   /* as in emspec_config */
    float shift_db;                    /* added to the dB before the law ("Gain" after the fact); the dB output is NOT shifted */
} emspec_view_map;

int     emspec_set_live_history(emspec_engine* e, int64_t columns /* W per stream; 0 clears */);
int64_t emspec_live_history(const emspec_engine* e, int32_t session, int32_t stream, int64_t* first_column /* may be NULL */);
int     emspec_history_view_device(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_column,
                                   int32_t factor, int64_t groups, const emspec_view_map* map,
                                   float* db_dev, uint8_t* index_dev, uint8_t* rgba_dev, void* hip_stream);
int     emspec_history_view(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_column,
                            int32_t factor, int64_t groups, const emspec_view_map* map,
                            float* out_db, uint8_t* out_index, uint8_t* out_rgba);

/*
 * ---- Live audio history: a ring on the device of the samples the streaming calls were fed, W per
 * stream, views that read a range back bit for bit, and a re-analysis that runs the batch kernels over a held range.  Serves the
 * settings the live history above cannot follow because they change the analysis itself - "FFT Size", "Smoothing", the Enhanced
 * / Natural switch (reassign), and, through emspec_reset, "Frequency Scale" and "Low-End Boost"  - without the
 * host keeping every sample of every stream and pushing them over the bus again; [BUILD-DEFINED].  Off unless set; with it
 * cleared every streaming call launches, allocates and writes exactly what it did before these entries.
 *
 * Samples are numbered per stream: sample a is the a-th sample the stream's session has received since the stream was
 * (re)started.  Block forms (emspec_push_samples, _multi, _multires, _multiband, _pcm*): the stream's samples in the order
 * pushed; a PCM session stores the decoded views' float samples, one ring per view stream.  Per-frame forms (emspec_column,
 * emspec_columns, _multires, _multiband): frame j of a stream is taken to be samples [j hop, j hop + n), and each frame stores
 * the samples the ring does not yet have - frame 0 whole, then each frame's last `hop`; the library does not check that frames
 * overlap consistently, as it never has.
 * Stored is what a launch has moved to the device.  A block that completes no frame only joins the host staging block (see
 * emspec_push_samples_multi) and is stored by the launch that ingests it: `end` may trail the samples pushed by less than one
 * frame before the first frame, and by less than `hop` after.  Flush calls store nothing.  Sample a lives in slot a mod W (any
 * W in 1 .. 2^28; the per-stream stride of the allocation may be padded); after any call the ring of a stream holds
 * [max(0, end - W), end); a launch that ingests more than W samples of a stream stores its last W.
 *
 * emspec_set_live_audio(e, W): W samples per stream for both sessions of the engine; 0 clears and frees (always allowed).
 *   EMSPEC_ERR_INVALID_ARG: W outside 0 .. 2^28.  EMSPEC_ERR_STATE: W > 0 while either session has samples fed (emspec_reset
 *   first).  The rings (streams x W x 4 bytes) are allocated by the first streaming call of a session, when its streams are
 *   known: EMSPEC_ERR_OUT_OF_MEMORY on that call, before anything is fed; the session stays as it was.  emspec_reset empties
 *   every ring; emspec_reset_stream empties that stream's ring and restarts its numbering, the other streams keep theirs.
 * emspec_live_audio(e, session, stream, &first): the number of samples of the stream that were stored (`end`), and in *first
 *   (may be NULL) the first sample held; -1 for a NULL engine, an unknown session or stream (a session that has not started
 *   has no streams), or no audio history.  session: as for emspec_live_history.
 *
 * A view of streams [stream0, stream0 + streams): pcm[sv][i] = sample first_sample + i of stream stream0 + sv, bit for bit
 * (NaN payloads and -0 are kept), i < count; layout [streams][stride] float32, stride >= count.
 * Required: first_sample >= the first held sample and first_sample + count <= end, for every addressed stream - else
 * EMSPEC_ERR_INVALID_ARG with a message naming the stream and its held range, nothing written.  Also EMSPEC_ERR_INVALID_ARG:
 * count < 1, streams < 1, a stream range outside the session, a NULL output or one that is not 4-byte aligned, stride < count.
 * EMSPEC_ERR_STATE: no audio history set, or a session that does not exist.  Every refusal leaves the engine usable.
 * emspec_audio_view_device: pcm_dev is device memory at any 4-byte alignment, any stride; enqueues on hip_stream (NULL: the
 *   default stream) behind the session's launches - every streaming call has synchronised before it returned - and does not
 *   synchronise; later streaming calls are ordered behind the view.  emspec_audio_view: pcm is a host array, page-locked
 *   (written in place) or pageable (staged through a page-locked block), as emspec_history_view's outputs; synchronises.
 *
 * emspec_audio_batch_device: emspec_audio_view_device of the range into an engine workspace [streams][count], followed by
 *   emspec_batch_device(e, that, streams, count, n, hop, reassign, db_dev, rgba_dev, index_dev, hip_stream) on the same stream:
 *   everything emspec_batch_device honours applies - emspec_set_time_reduce, emspec_set_display, the engine's current row
 *   edges, colour law and colour map, its output layouts and its refusals; count < n is EMSPEC_ERR_INVALID_ARG.  n, hop and
 *   reassign need not be the session's.  The live sessions are not disturbed: the call shares none of their buffers and
 *   changes none of their counters.  The workspace is the engine's: a second re-analysis must be ordered behind the first.
 * emspec_audio_batch: the same with host outputs in an emspec_out ([streams][columns][rows] of emspec_num_columns(count, n,
 *   hop) columns, reduced by emspec_set_time_reduce): device blocks grown in the engine, plain copies out, synchronises.  No
 *   pipeline: the picture is one window's worth.
 */
int     emspec_set_live_audio(emspec_engine* e, int64_t samples /* W per stream; 0 clears */);
int64_t emspec_live_audio(const emspec_engine* e, int32_t session, int32_t stream, int64_t* first_sample /* may be NULL */);
int     emspec_audio_view_device(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_sample,
                                 int64_t count, float* pcm_dev, int64_t stride, void* hip_stream);
int     emspec_audio_view(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_sample,
                          int64_t count, float* pcm, int64_t stride);
int     emspec_audio_batch_device(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_sample,
                                  int64_t count, int32_t n, int32_t hop, int32_t reassign,
                                  float* db_dev, uint8_t* rgba_dev, uint8_t* index_dev, void* hip_stream);
int     emspec_audio_batch(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_sample,
                           int64_t count, int32_t n, int32_t hop, int32_t reassign, const emspec_out* out);

/*
 * ---- Stereo image: level and balance of a channel pair in ONE picture - brightness from the louder
 * channel's dB, hue from the difference of the two - composed on the device from dB that is already there (a batch's
 * workspace, the live history ring), so that a renderer need not pull both channels' dB over the bus and compare them on its
 * own cores; [BUILD-DEFINED].  Nothing existing changes: every entry below is new.
 *
 * Streams.  A pair is two streams of one [S][C][R] array, chosen by (views, a, b): pair p uses streams p views + a (channel A)
 * and p views + b (channel B); views >= 2, 0 <= a, b < views, a != b.  This is the PCM front end's stream numbering: views = 2,
 * a = 0, b = 1 for left / right; views = 4 (L R M S) with (0, 1) for left / right and (2, 3) for mid / side as a width display.
 *
 * The law, per cell, on the two dB values x_a, x_b; all arithmetic binary32, one rounding per operation, no fused multiply-add.
 * Scalars (computed on the host): lo = db_top - db_range (binary32), inv = (float)(1.0 / (double)db_range),
 * inv_pan = (float)(1.0 / (double)pan_range_db).
 *     level:   m = (x_b > x_a || x_a != x_a) ? x_b : x_a          the cell's own bits; a NaN only when both are
 *     shifted: s = m + shift_db;  gated = s < gate_db
 *     index:   0 if s is NaN, else the palette index of s under (lo, inv, gate_db) - the law of emspec_history_view
 *     balance: d = x_b - x_a;  u = d * inv_pan;  if (u > 1) u = 1;  if (u < -1) u = -1;
 *              pan = 16 + (int)rintf(u * 16.0f)  (round half to even);  pan = 16 if gated or d is NaN
 *     rgba:    PAL[pan][index]                                    the engine's stereo palette, [33][256][4]
 * Outputs: level (float32, NOT shifted), index, pan (bytes) and rgba; any may be NULL, not all.  The balance needs no power
 * sum: a difference of dB values is the log of the energy ratio.
 *
 * Palette.  emspec_make_stereo_colormap(brightness, out[33][256][4]) builds it in integers from base =
 * emspec_make_colormap(brightness): for row pan, t = pan - 16, w = |t|, K = t < 0 ? (255, 96, 32) : (32, 160, 255); for entry i,
 * v = max(r, g, b) of base[i], per colour channel tint = (K_c v + 127) / 255 and out = (base_c (16 - w) + tint w + 8) / 16
 * (truncating divisions); alpha is base's; row 16 is base itself.  emspec_set_stereo_colormap(e, rgba33x256x4) uploads any
 * palette; a new engine holds the built one at the brightness of its default colour map (0.5).
 *
 * emspec_stereo_default_map(e, &map): the engine's db_top, db_range and gate_db, shift 0, pan_range_db = 12.
 * emspec_stereo_device: the law on any device dB array [pairs views][cells]; outputs [pairs][cells] (rgba + [4]).
 *   cells % 4 == 0; db_dev, level_dev, rgba_dev 16-byte and index_dev, pan_dev 4-byte aligned; pairs in 0 .. 65535, 0 a no-op.
 *   Enqueues on hip_stream (NULL: the default stream); does not synchronise.
 * emspec_stereo_host: the same definition in plain C++ on host arrays: no engine, no device.  `palette` ([33][256][4]) is
 *   needed only with rgba.  The message of a refusal: emspec_last_error(NULL).
 * emspec_batch_stereo_device: the law on exactly the dB emspec_batch_device(e, pcm_dev, S, L, n, hop, reassign, ..) would deliver
 *   (the display post-process included), without that dB leaving the engine.  S % views == 0; outputs [S / views][C][R].
 *   Chunks of whole pairs run through the engine workspace emspec_batch_peaks_device uses.
 * emspec_batch_pcm_stereo: the host entry, from raw interleaved frames as emspec_batch_pcm takes them; views = fmt->views, a pair
 *   is the views of one source.  Outputs [sources][C][R] host arrays, page-locked or pageable.  Only the requested outputs
 *   cross the bus on the way out: 1 + 1 bytes (index, pan) or 4 (RGBA) per pair cell instead of 8 of dB.  emspec_set_wave_out is
 *   honoured as by emspec_batch_pcm (the envelope of all sources x views streams).
 * emspec_history_view_stereo_device / emspec_history_view_stereo: the live form.  Reads the live history ring: for each pair, the
 *   peak hold of each channel's group - exactly emspec_history_view's dB of that stream - then the law.  Streams
 *   stream0 .. stream0 + pairs views - 1 of the session; outputs [pairs][groups][rows].  Every rule of emspec_history_view
 *   applies to BOTH streams of every pair: held range, factor, groups, alignment (level as its dB, pan as its index), the
 *   ordering behind the session's launches.  A renderer calls it per redraw, like a mono view.
 *
 * Refusals.  The batch entries return EMSPEC_ERR_STATE while a time reduction is set (emspec_set_time_reduce(e, 1) turns it off).
 * Every other refusal is EMSPEC_ERR_INVALID_ARG with a message naming the rule: views / a / b, pan_range_db or db_range not > 0,
 * a NaN field, cells % 4, S % views, all outputs NULL, misalignment - and, for the views, those of emspec_history_view.  The
 * engine stays usable.
 */
#define EMSPEC_STEREO_PAN_CENTRE 16
#define EMSPEC_STEREO_PAN_LEVELS 33          /* balance byte 0 (all A / left) .. 32 (all B / right) */
typedef struct emspec_stereo_map {
    float db_top, db_range, gate_db, shift_db;   /* as emspec_view_map, applied to the level */
    float pan_range_db;                          /* |dB_b - dB_a| that reads as fully to one side; > 0 */
} emspec_stereo_map;                             /* 20 bytes */

int     emspec_stereo_default_map(const emspec_engine* e, emspec_stereo_map* map);
int     emspec_make_stereo_colormap(float brightness, uint8_t* rgba33x256x4);
int     emspec_set_stereo_colormap(emspec_engine* e, const uint8_t* rgba33x256x4);
int     emspec_stereo_device(emspec_engine* e, const float* db_dev, int32_t pairs, int32_t views, int32_t a, int32_t b,
                             int64_t cells, const emspec_stereo_map* map,
                             float* level_dev, uint8_t* index_dev, uint8_t* pan_dev, uint8_t* rgba_dev, void* hip_stream);
int     emspec_stereo_host(const float* db, int64_t pairs, int32_t views, int32_t a, int32_t b, int64_t cells,
                           const emspec_stereo_map* map, const uint8_t* palette,
                           float* level, uint8_t* index, uint8_t* pan, uint8_t* rgba);
int     emspec_batch_stereo_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n, int32_t hop,
                                   int32_t reassign, int32_t views, int32_t a, int32_t b, const emspec_stereo_map* map,
                                   float* level_dev, uint8_t* index_dev, uint8_t* pan_dev, uint8_t* rgba_dev, void* hip_stream);
int     emspec_batch_pcm_stereo(emspec_engine* e, const void* src, const emspec_pcm_format* fmt, int32_t sources, int64_t frames,
                                int32_t n, int32_t hop, int32_t reassign, int32_t a, int32_t b, const emspec_stereo_map* map,
                                float* out_level, uint8_t* out_index, uint8_t* out_pan, uint8_t* out_rgba);
int     emspec_history_view_stereo_device(emspec_engine* e, int32_t session, int32_t stream0, int32_t pairs, int32_t views,
                                          int32_t a, int32_t b, int64_t first_column, int32_t factor, int64_t groups,
                                          const emspec_stereo_map* map,
                                          float* level_dev, uint8_t* index_dev, uint8_t* pan_dev, uint8_t* rgba_dev, void* hip_stream);
int     emspec_history_view_stereo(emspec_engine* e, int32_t session, int32_t stream0, int32_t pairs, int32_t views,
                                   int32_t a, int32_t b, int64_t first_column, int32_t factor, int64_t groups,
                                   const emspec_stereo_map* map,
                                   float* out_level, uint8_t* out_index, uint8_t* out_pan, uint8_t* out_rgba);

#ifdef __cplusplus
}
#endif
#endif /* EMSPEC_H */
