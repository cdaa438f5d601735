/* include/maxigpu.h -- the C-ABI of libmaxigpu.so: the MI355X (gfx950) voice-bank DSP path
 * behind the Maximilian class API.
 *
 * The reference (micknoise/Maximilian, cited as C = src/maximilian.cpp, H = src/maximilian.h,
 * L/ = src/libs/) has no FFI: its "plugin API" is the C++ class surface a user's
 * `void play(double*)` calls once per sample (cpp/commandline/player.cpp:25-44 drives it).
 * Each entry point below is what a binding for that surface would bind: it renders N samples
 * of a BANK of V independent instances of one reference class in a single launch.  The host
 * facade (include/maximilian_bank.hpp) keeps the reference's class/method names on top.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types cross this boundary.
 *   - every `d_*` pointer is DEVICE memory (from mxg_malloc, hipMalloc, or a torch tensor's
 *     data_ptr()); `h_*` is host memory.  Pointers are borrowed for the call only.
 *   - bank signals are sample-major / voice-minor:  out[n*V + v],  n < N, v < V.
 *   - state is SoA: one array of length V per reference member, updated in place so
 *     consecutive calls continue the stream exactly like consecutive play() calls.
 *   - `stream` is a hipStream_t passed as void* (NULL = the library's own default stream; to
 *     target HIP's null stream pass hipStreamLegacy, i.e. (void*)1).
 *     Calls are asynchronous on that stream; mxg_sync()/mxg_stream_sync() wait.
 *   - returns 0 on success, a negative mxg_status otherwise; never throws, never exit()s
 *     (the reference exit(1)s on a bad FFT size, L/fft.cpp:129-132; here that is
 *     MXG_ERR_INVALID).  mxg_last_error() gives a thread-local message.
 *   - there is NO CPU fallback: without a HIP device every compute call fails with
 *     MXG_ERR_NO_DEVICE.
 */
#ifndef MAXIGPU_H
#define MAXIGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MXG_OK = 0,
    MXG_ERR_INVALID = -1,   /* bad argument (null pointer, unknown waveform, odd size ...) */
    MXG_ERR_NO_DEVICE = -2, /* no HIP device / runtime failure at init */
    MXG_ERR_HIP = -3,       /* a HIP call failed; see mxg_last_error() */
    MXG_ERR_NOMEM = -4
} mxg_status;

/* maxiOsc waveforms, numbered as in oracle/maxi_oracle.c.  Reference: C:228-373. */
typedef enum {
    MXG_OSC_SINEWAVE = 0,       /* C:228-235 */
    MXG_OSC_COSWAVE = 1,        /* C:276-283 */
    MXG_OSC_PHASOR = 2,         /* C:285-291 */
    MXG_OSC_SAW = 3,            /* C:333-340 */
    MXG_OSC_TRIANGLE = 4,       /* C:362-373 */
    MXG_OSC_SQUARE = 5,         /* C:293-300 */
    MXG_OSC_PULSE = 6,          /* C:302-311  p1 = duty */
    MXG_OSC_IMPULSE = 7,        /* C:312-319 */
    MXG_OSC_SINEBUF = 8,        /* C:266-274 */
    MXG_OSC_SINEBUF4 = 9,       /* C:237-264 */
    MXG_OSC_SAWN = 10,          /* C:342-359 */
    MXG_OSC_PHASORBETWEEN = 11  /* C:321-330  p1 = startphase, p2 = endphase */
} mxg_osc_waveform;

/* maxiFilter kinds.  Reference: C:442-500. */
typedef enum {
    MXG_FLT_LORES = 0,   /* C:455-468 */
    MXG_FLT_HIRES = 1,   /* C:471-484 */
    MXG_FLT_BANDPASS = 2,/* C:487-500 */
    MXG_FLT_LOPASS = 3,  /* C:442-446 */
    MXG_FLT_HIPASS = 4   /* C:449-453 */
} mxg_filter_kind;

/* ---- library / device ---------------------------------------------------------------- */
/* Select the HIP device (-1 = current), create the default stream.  Idempotent. */
int mxg_init(int device);
const char *mxg_last_error(void);
const char *mxg_version(void);
/* maxiSettings::setup (H:138-143): global sampleRate / channels / bufferSize (size_t). */
int mxg_settings(size_t sampleRate, size_t channels, size_t bufferSize);
size_t mxg_sample_rate(void);

/* ---- device memory / streams (thin pass-throughs, so a host needs no HIP headers) ----- */
void *mxg_malloc(size_t bytes);
int mxg_free(void *d_ptr);
int mxg_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream);
int mxg_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream);
int mxg_memset(void *d_dst, int value, size_t bytes, void *stream);
/* Asynchronous forms: the copy is only enqueued on `stream`; the host buffer must stay valid (and for a real overlap be
 * pinned: mxg_host_alloc) until the stream has passed it -- mxg_event_record + mxg_event_sync / mxg_event_query.  Together
 * with the render entry points (all of which only enqueue) this is the asynchronous double-buffering of SURVEY 8(b):
 * render block k+1 and its download on a stream while the audio thread still serves block k.  A bank's state is the
 * caller's own device SoA arrays, so a "state get/set" is a copy of those arrays (mxg_memcpy_d2h / _h2d). */
int mxg_memcpy_h2d_async(void *d_dst, const void *h_src, size_t bytes, void *stream);
int mxg_memcpy_d2h_async(void *h_dst, const void *d_src, size_t bytes, void *stream);
int mxg_memcpy_d2d_async(void *d_dst, const void *d_src, size_t bytes, void *stream);  /* device to device, in stream order */
void *mxg_host_alloc(size_t bytes); /* pinned host memory */
int mxg_host_free(void *h_ptr);
void *mxg_stream_create(void);
int mxg_stream_destroy(void *stream);
int mxg_stream_sync(void *stream);
int mxg_sync(void);
/* HIP events on `stream`, for timing a launch from the host side of the boundary. */
void *mxg_event_create(void);
int mxg_event_destroy(void *event);
int mxg_event_record(void *event, void *stream);
int mxg_event_elapsed_ms(void *start, void *stop, float *h_ms);
int mxg_event_sync(void *event);
int mxg_event_query(void *event); /* 1 = complete, 0 = not yet, < 0 error */
int mxg_stream_wait_event(void *stream, void *event);

/* The headless host: cpp/commandline/player.cpp:25-44 `routing()` restated without RtAudio -- calls the user's
 * `void play(double *output)` (src/maximilian.cpp:205-207) once per frame and copies `channels` doubles per frame into
 * the interleaved buffer.  h_lastValues [channels] persists between calls like the callback's userData. */
int mxg_host_render(void (*play)(double *), size_t channels, size_t nFrames, double *h_interleaved, double *h_lastValues);

/* ---- per-kernel timing (measurement only) --------------------------------------------------------- */
/* mxg_prof_enable(1): every entry point brackets its kernels with HIP events on the launch stream (one label per
 * kernel, e.g. "osc_kernel", "fft1024_kernel"); mxg_prof_read(i, ...) waits for label i's events and returns the
 * summed kernel time and the number of launches since the last mxg_prof_reset().  Off by default (no events, no
 * overhead).  This is how bench.py measures the average launch duration of the dominant kernel inside its timed
 * region; the rocprofv3 kernel-trace averages in profiles/ agree with it. */
int mxg_prof_enable(int on);  /* returns the previous setting */
int mxg_prof_reset(void);
int mxg_prof_count(void);
int mxg_prof_read(int index, const char **h_label, double *h_total_ms, size_t *h_launches);
/* Average interval of `pairs` EMPTY event pairs on `stream` (two records back to back, nothing between): the marker
 * overhead every figure of mxg_prof_read carries, for a caller that wants to subtract it. */
int mxg_prof_overhead_ms(void *stream, int pairs, double *h_ms);

/* ---- tuning knobs (performance only; results are identical for every setting) ---------- */
/* key: "osc_vpl" (voices per lane: 0 automatic, 1|2), "osc_block" (64..1024), "osc_nt" (non-temporal stores: 0 never, 1 always, 2 by the size of the output block),
 * "voice_block" (lanes per workgroup of the one-lane-per-voice bank kernels: a multiple of 64, capped at 256; the polyblep, drum, clock, line and
 * analysis banks run at 64 up to 16 384 voices whatever the knob says; bit-identical results at every value), "voice_nt" (as osc_nt), "mix_rows" (sample rows per workgroup of the mixdown, 1|2), "fft_generic",
 * "mfcc_tiled" (LDS-staged spectra 0|1), "grain_chunked" (time-sharded granular render 0|1), "grain_lanes_k",
 * "grain_unit" (coalesced unit-increment render 0|1), "grain_line" (tile render for arbitrary increments 0|1), "grain_fast_sched" (event-driven schedulers 0|1), "grain_streamed" (unit-path maxiTimeStretch call as ONE launch whose scheduler lanes
 * and tile renders run side by side, 1 default; 0 = time slices on the library's auxiliary streams), "grain_slices" (those time slices, 1..16), "osc_mix_win" (K1m: samples per workgroup combine window, 0 automatic, 128 or 256), "osc_mix_pcwin" (the same for the producer / consumer form: 0 automatic, 256 or 512), "osc_mix_pc" (K1m as producer / consumer wavefront pairs: 0 automatic, 1 off, 2 on),
 * "rw_store" (the read + write bank kernels' 16-byte pair-row streams: 0 automatic, 1 off, 2 / 3 / 4 on with plain / write-through /
 * non-temporal stores), "fft_exact" (1 default; 0 = TOLERANCE MODE of mxg_fft_mfcc_batch: the 512-point transform as true radix-8 butterflies with correctly
 * rounded twiddles and fused multiply-adds, hardware square root -- about a quarter fewer instructions; magnitudes within 6e-7 x the
 * frame's peak of the TRUE transform and -- because the reference's fp32 twiddle recurrences drift by ~1e-4 -- within 4e-4 of the reference's,
 * mfcc within 5e-4 of the reference's; bit-exactness is given up, accuracy is gained),
 * "time_parallel" (the other exception to "identical results": 1 lets banks of at most 4096 linear filters with block-constant
 * coefficients -- maxiBiquad, maxiSVF, maxiDCBlocker through mxg_filter2_render, lores / hires through mxg_filter_render -- and blocks
 * of 64, 128, 256, 512, 1024 or 2048 samples (64 x a power of two up to 32; every other block length keeps the bit-exact kernels) be
 * cut along time and joined by a wavefront scan: a 6-voice x 512-sample block in a few microseconds instead of 23-28, with reordered
 * arithmetic: |error| <= 1e-10 x the voice's peak of the sequential output over the carried blocks, for stable settings and finite
 * input, over the whole domain the classes accept (measured on the 64-lane host build of csrc/mxg_scan.h, whose bits the device
 * must give: <= 6.3e-11 for maxiBiquad -- at 10 Hz, N = 2048, where the float64 sequential recurrence is itself 3.8e-11 from a
 * long-double one; <= 1.4e-11 up to N = 512 -- and <= 8e-14 for the other kinds).  The biquad's scan is carried in (v2, v1, v1 - v2),
 * which is what
 * holds the bound at 10 ... 60 Hz.  A setting at which the reference itself diverges (lores at 10 kHz with resonance 1) is outside
 * the bound; such a voice, like one fed a NaN or an infinity, changes no other voice's bits.  default 0 = the bit-exact kernels),
 * "osc_plan" (K1, banks beyond ~350 MB per block: rendered as passes of 98 304 voices + a remainder launch; 0 automatic, 1 never, 2 / 3 always),
 * "osc_passes" / "osc_mix_passes" (K1 / K1m: voice groups a wavefront renders one after the other, the grid covering 1 / passes of the bank: 0 automatic, 1..64),
 * "osc_split" (time parts per voice group in K1: 0 automatic, 1..8), "osc_mix_split" (the same for the fused render + mixdown K1m,
 * 0 automatic, 1..4), "osc_mix_store" (K1m's per-voice block: 0 automatic, 1 plain 8-byte stores, 2 pair rows of 16-byte stores),
 * "smp_split" (time parts of a block-constant playAtSpeed / playOnceAtSpeed / playUntilAtSpeed launch: 0 automatic, 1..8),
 * "smp_pipe" (that launch issues the window loads of chunk k+1 before the stores of chunk k, 0|1),
 * "ifft_stream" (mxg_ifft_batch: inverse transform and hop buffer in one kernel: 0 never, 1 where hop >= fftSize / 2, 2 wherever it fits),
 * "mfcc_mfma_fullk" (the MFMA mel contraction runs over all numBins bins instead of the ones that carry weight, 0|1).
 * "fused_layout" (mxg_fft_mfcc_batch: 0 automatic, 1 = two frames in flight per wavefront and two 4-wave workgroups per CU, 2 = one
 * frame in flight and one 12-wave workgroup per CU; same bits either way),
 * "fused_waves16" (mxg_fft_mfcc_batch: the 16-waves-per-CU form of the fused kernel when the request allows it, 0|1),
 * "fused_mel" (mxg_fft_mfcc_batch, the stage after the magnitudes: 0 automatic = 3, or 2 when d_melraw / d_melbands are requested; 1 = sparse mel walk, logs and DCT on the vector ALU in
 * the reference's summation orders; 2 = the same walk -- band sums bit-exact -- with the DCT's 42-term sums on the matrix pipe
 * (v_mfma_f64_4x4x4_4b_f64: fused multiply-adds, within 1e-13 x the largest band log of form 1); 3 = the mel contraction on the matrix
 * pipe as well, banded per quad of filters: band sums within 4e-15 x the frame's largest band (measured 2.2e-16), mfcc within 1e-13 of form 1
 * (measured 1.4e-15) -- the north star's
 * "MFMA for the mel-filterbank x frame contraction" inside the one-kernel path).
 * "osc_store" (K1's store stream: 0 automatic by waveform and bank size; one voice per lane: 1 plain 8-byte stores, 2 non-temporal,
 * 3 / 4 / 5 two samples of a lane pair exchanged into one 16-byte store per lane, plain / write-through (sc1) / non-temporal; two
 * voices per lane: 1 plain, 2 non-temporal, 3 write-through 16-byte stores), "voice_store" / "voice_xcd" (the same for the fused voice kernel; one voice
 * per lane only), "voice_mix_store" (the store stream of mxg_voice_render_mix*: 0 automatic = "voice_store"'s rule, 1 ... 5 its flavours),
 * "voice_diet" (the fused voice, mode A without mixdown: 0 automatic = the short instruction stream of the fast paths, except around 65 536 voices when the launch cannot be paced; 1 = the round-5 stream; 2 = the short one; same bits),
 * "voice_pace" (the fused voice's paced store schedule, a chunk of 8 samples every P ticks of 10 ns: 0 automatic = a per-stream controller
 * at the store-bound bank sizes whose whole grid is resident at once (45 056 ... 262 144 voices; mode B to 131 072, the mixdown form to 65 536); 1 never; >= 2 a fixed P; timing only, same bits), "osc_pace" (the same for mxg_osc_render: 0 automatic = the table-free waveforms at 90 112 ... 327 680 voices; 1 never; >= 2 a fixed P),
 * "tab_sides" (mxg_osc_render_tables*: 0 automatic = 1 workgroups of 256 lanes, one round of 8 voices at a time, two per CU; 2 = workgroups of 512 lanes, two rounds side by side),
 * "smp_pace" (the paced schedule for mxg_sample_render: 0 automatic = play() at 45 056 ... 229 375 voices; 1 never; >= 2 a fixed P), "smp_ring" (the *AtSpeed players' window rows as rings: 0 automatic = samples beyond 1 GiB, 1 off, 2 on), "grain_spin_limit" (see mxg_granular_retries), "osc_xcd" (workgroups renumbered so that each of the eight XCDs renders
 * one contiguous eighth of the bank: 0 automatic, 1 off, 2 on), "grain_pool_tiles" (mxg_granular_pool_render: 0 automatic = the scheduler pass + tile
 * render for calls of at least 128 samples, 1 = the one-lane-per-stream walk only, 2 = the tile form wherever it can run), "grain_sync" (mxg_granular_render reads its error word back before it returns, 0|1;
 * default 0: deferred, see mxg_last_async_error), "part_spin_limit" (polls a time-split kernel's writer part makes before it gives up
 * and reports through mxg_last_async_error), "part_fault" (test-only fault injection: that writer waits for a signal that never comes).
 * "rw_chunk" (samples per chunk of the pair-row maxiFilter kernel / rows per chunk of the noise column walk: 0 automatic = 8, 4 / 8 / 16 / 32;
 * measured: 8 is the optimum, fewer loads in flight starve the read stream, longer chunks burst the stores).
 * The tests flip every one of them and demand identical bits.  Returns the previous value or MXG_ERR_INVALID. */
int mxg_tune(const char *key, int value);

/* Asynchronous device errors.  A kernel that detects, while it runs, a failure no argument check could see -- a time-split
 * launch whose writer part never got its sibling parts' signals (its state is then NOT stored), a granular render that ran out
 * of rand() draws or met a live grain its plan could not have made -- stores a code in a word of pinned host memory.  No call
 * synchronises for it: the NEXT call of any entry point (and every synchronising call -- mxg_stream_sync, mxg_sync,
 * mxg_memcpy_d2h -- after its wait) returns the failure as its status with the message in mxg_last_error(), once, and clears
 * it.  mxg_last_async_error() is that check by itself: MXG_OK, or the pending failure.  (Render entry points therefore never
 * block the host, and their launch sequences can be captured into a hipGraph; a captured launch reports the same way.)
 * After a time-part time-out the caller must synchronise that stream and treat the state of every bank rendered on it since the failed
 * launch as invalid (launches already enqueued behind it may have run from stale part counters): re-upload or re-create those banks.
 * "rw_store" (mxg_tune) is documented with the render entry points that honour it (maxiFilter, maxiEnv, maxiDelayline, maxiSample,
 * maxiEnvGen, filter2: 0 automatic, 1 8-byte streams, 2 / 3 / 4 16-byte pair rows with plain / write-through / non-temporal stores). */
int mxg_last_async_error(void);
/* Streamed granular launches (mxg_granular_render*, one-launch form) whose tile renders gave up waiting for the scheduler workgroups of
 * their own launch -- a pre-empted or partitioned device -- and were therefore rendered AGAIN by the kernel that follows every such
 * launch (the renderer-alone form over the completed lists: the same bits, no silence, no error).  A statistic: 0 on a healthy device.
 * Counted when the call's last kernel has run.  Knob "grain_spin_limit" (polls without progress before a render gives up; 0 = 2^22). */
int mxg_granular_retries(void);

/* ---- maxiOsc bank -------------------------------------------------------------------- */
/* Renders out[n][v] = bank[v].<waveform>(freq) for n < N, exactly as N consecutive per-sample
 * calls would (H:169-215).  d_freq is [V] (fps=0, block-constant) or [N][V] (fps=1, audio-rate
 * modulation); fps=2: d_freq AND d_p1 are [N][V] (a pulse width / start phase that changes per
 * sample as well).  d_p1/d_p2: per-voice extra arguments (see mxg_osc_waveform), may be NULL when
 * unused.  d_phase / d_outhold: the members `phase` and `output` (H:173,176), in/out.
 * maxiOsc::noise (C:214-220) draws from the process-wide rand(): see mxg_osc_noise. */
int mxg_osc_render(int waveform, size_t V, size_t N, const double *d_freq, int fps,
                   const double *d_p1, const double *d_p2, double *d_phase, double *d_outhold,
                   double *d_out, void *stream);
/* The same with a row pitch: sample n of voice v goes to d_out[n * out_pitch_bytes / 8 + v] (out_pitch_bytes a multiple of 8, >= V * 8;
 * a multiple of 16 keeps the 16-byte store streams).  mxg_osc_render is this call with out_pitch_bytes = V * 8.  Why a caller
 * would pad: when V * 8 is a multiple of 2 MB (262 144 voices and its multiples) the same column of every row lands on the same HBM
 * channel and the store stream runs at 0.68-0.71 of the peak instead of 0.75-0.80; a pitch of V * 8 + 256 ... 4096 bytes removes
 * that (profiles/r05_osc_pitch.md).  src/maximilian.cpp:266-274 per voice, nothing else changes. */
int mxg_osc_render_pitch(int waveform, size_t V, size_t N, const double *d_freq, int fps,
                         const double *d_p1, const double *d_p2, double *d_phase, double *d_outhold,
                         double *d_out, size_t out_pitch_bytes, void *stream);

/* maxiOsc::noise (C:214-220): `float r = rand()/(float)RAND_MAX; output = r*2-1`.  rand() is one
 * serial process-wide stream (not a per-object state), so which draw a voice sees is decided by
 * the order of the caller's per-sample loop.  The caller therefore supplies the draws, exactly as
 * the granular entry point does for its rand() uses: d_rand[n][v] is the value rand() returned for
 * voice v at sample n (for a voice-inner loop: draw number n*V+v); the kernel applies the
 * reference's float arithmetic (bit-exact).  count = N*V values; d_outhold ([V], may be NULL)
 * receives the member `output` (H:176) after the last sample. */
int mxg_osc_noise(size_t V, size_t N, const int32_t *d_rand, double *d_outhold, double *d_out,
                  void *stream);

/* Render + fused stereo mixdown: as mxg_osc_render (block-constant frequencies) and, in the same
 * pass, d_mix[n][0..1] = sum_v (out[n][v]*sqrt(1-pan_v), out[n][v]*sqrt(pan_v)) (maxiMix::stereo,
 * C:503-509, plus the user-side sum over voices, 15.polysynth/main.cpp:67).  The per-voice block is
 * never re-read: each workgroup sums its 256 voices through an LDS transpose and a small second
 * kernel adds the per-workgroup rows (fixed order: deterministic; tolerance on the mix as for
 * mxg_mix_stereo).  d_out may be NULL: then only the mix is produced (what a play() callback needs)
 * and nothing but [N][2] leaves the chip. */
int mxg_osc_render_mix(int waveform, size_t V, size_t N, const double *d_freq, const double *d_p1,
                       const double *d_p2, double *d_phase, double *d_outhold, double *d_out,
                       const double *d_pan, double *d_mix, void *stream);
/* The same render WITHOUT the second kernel: d_rows[g][n][0..1], g < mxg_osc_mix_groups(V) = ceil(V / 256), holds the
 * mix of voices [256 g, 256 g + 256); the mix is their sum in ascending g.  For a caller that adds the rows elsewhere:
 * a grouped mix queue (mxg_mixq_create_grouped) does it once per batch on its own stream, so that the render stream
 * carries ONE kernel per block; mxg_mix_rows_sum(groups, count = N * 2, d_rows, d_mix) is that sum as a call. */
size_t mxg_osc_mix_groups(size_t V);
int mxg_osc_render_mix_rows(int waveform, size_t V, size_t N, const double *d_freq, const double *d_p1,
                            const double *d_p2, double *d_phase, double *d_outhold, double *d_out,
                            const double *d_pan, double *d_rows, void *stream);
int mxg_mix_rows_sum(size_t groups, size_t count, const double *d_rows, double *d_mix, void *stream);

/* EXTENSION (no reference counterpart; SURVEY.md 8(d) row 2, north_star "HBM-read roofline on the wavetable path"):
 * maxiOsc::sinebuf (C:266-274) with a table PER VOICE.  d_tables[V][514] (16-byte aligned) plays the part of the reference's one
 * shared `double sineBuffer[514]` (C:63) for voice v: out = (1-rem)*T_v[1+(long)phase] + rem*T_v[2+(long)phase], same phase
 * recurrence, same expression order -- a bank whose tables all hold sineBuffer gives mxg_osc_render(MXG_OSC_SINEBUF)'s bits.
 * 4112 B of table are read per voice and block (8.03 B per sample at N = 512), each exactly once.  N <= 512.
 * Outputs, either or both: d_out [N][V] (the per-voice block) and the fused maxiMix::stereo mixdown as partial rows
 * d_rows[g][n][0..1], g < mxg_osc_tables_groups(V) (d_pan [V] given): the mix is the sum of the rows in ascending g
 * (mxg_mix_rows_sum, or a grouped mix queue).  d_phase / d_outhold as for mxg_osc_render. */
size_t mxg_osc_tables_groups(size_t V);
int mxg_osc_render_tables(size_t V, size_t N, const double *d_freq, const double *d_tables, double *d_phase,
                          double *d_outhold, double *d_out, const double *d_pan, double *d_rows, void *stream);
/* The same render with two additions (round 6), each optional and neither changing a bit of the block, the rows or the carried phase:
 *   d_mix [N][2] (needs d_pan + d_rows): the sum of the rows, formed INSIDE the render kernel by the workgroups that finish last --
 *     mxg_mix_rows_sum's additions in its order, no second launch;
 *   flags & MXG_TABLES_AHEAD: pipelined blocks.  The phase recurrence of a block (512 dependent steps per voice) has to run before
 *     the block's tables are rendered; with this flag the render of block k also walks block k + 1's, beside its table traffic, so
 *     from the second call on a call is ONE kernel.  The caller's promise: the next call on this stream has the same V and N, the same
 *     d_freq / d_pan (pointers AND contents) and d_phase untouched in between.  A call that breaks the pattern (other arguments, no
 *     flag) is still correct as long as d_phase was not written: d_phase always holds the phase after the last rendered block.
 *     Banks of more than 512 voices per workgroup (131 072 on a 256-CU device) ignore the flag. */
#define MXG_TABLES_AHEAD 1
int mxg_osc_render_tables_ex(size_t V, size_t N, const double *d_freq, const double *d_tables, double *d_phase, double *d_outhold,
                             double *d_out, const double *d_pan, double *d_rows, double *d_mix, int flags, void *stream);

/* ---- maxiFilter bank ------------------------------------------------------------------ */
/* d_st = [5][V]: x, y, outputs[0], outputs[1], outputs[2] (H:289-302), in/out.
 * lores/hires/bandpass with block-constant cutoff/resonance (cps=rps=0): the coefficients that
 * need cos/pow/sqrt (C:459-461: c, r; C:492-495: inputs[0..2]) must be supplied precomputed in
 * d_coef = [3][V] -- computed on the host with the host libm by mxg_filter_coeffs_host(),
 * which makes the recurrence bit-exact.  With cps or rps = 1 (per-sample modulation, e.g.
 * 14.monosynth/main.cpp:53) the coefficients are evaluated on the device (cos/sqrt) under the
 * tolerance stated in DESIGN.md; d_coef is ignored. d_res/d_coef may be NULL for
 * lopass/hipass. */
int mxg_filter_render(int kind, size_t V, size_t N, const double *d_in, const double *d_cutoff,
                      int cps, const double *d_res, int rps, const double *d_coef, double *d_st,
                      double *d_out, void *stream);
/* lores / hires / bandpass with PER-SAMPLE coefficients computed by the caller: d_coef_ps = [N][3][V], rows as mxg_filter_coeffs_host
 * writes them (c, r, unused | inputs[0..2]) for the cutoff / resonance of that sample.  The bit-exact form of a modulated cutoff
 * (the reference evaluates cos / pow / sqrt with the host libm on every call, src/maximilian.cpp:456-461): mxg_filter_render's own
 * per-sample mode evaluates them on the device, under a tolerance.  include/maximilian.h uses this when a cutoff follows another
 * object's output. */
int mxg_filter_render_coefs(int kind, size_t V, size_t N, const double *d_in, const double *d_coef_ps, double *d_st, double *d_out,
                            void *stream);
/* Host-side coefficient evaluation on this machine's libm: kind lores/hires -> h_coef[0]=c,
 * h_coef[1]=r (C:456-461); bandpass -> h_coef[0..2]=inputs[0..2] (C:489-495).  h_coef is [3][V]. */
int mxg_filter_coeffs_host(int kind, size_t V, const double *h_cutoff, const double *h_res,
                           double *h_coef);

/* ---- maxiEnvGen bank (H:2268-2547) ------------------------------------------------------------------ */
/* maxiEnvGen::setup(levels, times, curves, ...) (H:2366-2399) on the host: times in ms, or -46692
 * (maxiEnvGen::HOLD) for the one allowed hold stage; h_stages [nlevels-1][6] = startlevel, endlevel,
 * gradient, curve, length (samples), hold.  Returns the number of stages (<= 32) or MXG_ERR_INVALID
 * where setup() returns false.  setupAR/ASR/ADSR (H:2480-2504) are particular level/time/curve lists. */
int mxg_envgen_stages_host(size_t nlevels, const double *h_levels, const double *h_times,
                           const double *h_curves, double *h_stages);
/* d_out[n][v] = bank[v].play(trigger) (H:2277-2354) for one shared envelope shape d_stages [nstages][6]
 * (device copy of the table above), loop / retrigger flags, and a trigger signal d_trig that is [N][V]
 * (tpv = 1) or one shared [N] gate (tpv = 0).  State, in/out: d_dst = [5][V] envval,
 * stages[phase].currentlevel, previousValue of trigDetector / holdDetector / retriggerDetector;
 * d_ist = [7][V] int64: phase, state (0 WAITING, 1 TRIGGERED, 2 HOLDING), nxcHappened,
 * stages[phase].counter, firstTrigger of the three detectors.  A freshly set-up object is all zeros
 * except previousValue = 1.0 and firstTrigger = 1 (H:593-594).  State machine bit-exact; the value is exact
 * for curve == 1 and within the device pow's accuracy otherwise. */
int mxg_envgen_render(size_t V, size_t N, const double *d_trig, int tpv, const double *d_stages, int nstages,
                      int loop, int retrigger, double *d_dst, int64_t *d_ist, double *d_out, void *stream);

/* ---- maxiDCBlocker / maxiSVF / maxiBiquad banks (H:1255-1486) ------------------------------------ */
/* kind 0 maxiDCBlocker::play(input, R) H:1261-1266: d_coef = [1][V] R; d_st = [3][V] xm1, ym1, (unused).
 * kind 1 maxiSVF::play(w, lpmix, bpmix, hpmix, notchmix) H:1303-1317: d_coef = [9][V] g1, g2, g3, g4, k
 *        (rows 0-4 from mxg_svf_coeffs_host = setCutoff/setResonance -> setParams H:1320-1332) then the
 *        four mix arguments; d_st = [3][V] v0z, v1, v2.
 * kind 2 maxiBiquad::play(input) H:1360-1367: d_coef = [5][V] a0, a1, a2, b1, b2 (mxg_biquad_coeffs_host
 *        = set(type, cutoff, Q, peakGain) H:1376-1478); d_st = [3][V] v[0], v[1], v[2].
 * Coefficients come from the host libm (tan, pow, sqrt), so the recurrences are bit-exact. */
int mxg_filter2_render(int kind, size_t V, size_t N, const double *d_in, const double *d_coef,
                       double *d_st, double *d_out, void *stream);
int mxg_svf_coeffs_host(size_t V, const double *h_cutoff, const double *h_res, double *h_coef);
/* h_type[v]: 0 LOWPASS 1 HIGHPASS 2 BANDPASS 3 NOTCH 4 PEAK 5 LOWSHELF 6 HIGHSHELF (H:1349-1358) */
int mxg_biquad_coeffs_host(size_t V, const int32_t *h_type, const double *h_cutoff, const double *h_Q,
                           const double *h_peakGain, double *h_coef);

/* ---- maxiEnv bank --------------------------------------------------------------------- */
/* mode 0: adsr(input, trigger) (C:1415-1466)   mode 1: ar(input, attack, release, holdtime,
 * trigger) (C:1319-1358).  d_in NULL = constant 1.0 input.  d_trig: int32 [N] (tpv=0, one
 * trigger signal for the whole bank) or [N][V] (tpv=1).  d_par = [4][V] attack, decay,
 * sustain, release as stored by the setters; d_holdtime int64 [V]; d_dst = [2][V] amplitude,
 * output; d_ist = int64 [6][V] holdcount, attackphase, decayphase, sustainphase, holdphase,
 * releasephase.  All state in/out; zero-initialise to match static-storage maxiEnv objects. */
int mxg_env_render(int mode, size_t V, size_t N, const double *d_in, const int32_t *d_trig,
                   int tpv, const double *d_par, const int64_t *d_holdtime, double *d_dst,
                   int64_t *d_ist, double *d_out, void *stream);
/* maxiEnv setters on the host libm (C:1469-1494): which 0 setAttack 1 setDecay 2 setRelease
 * 3 setAttackMS. */
double mxg_env_coeff_host(int which, double ms);
/* maxiConvert::mtof (H:941, C:1498-1500): the reference's 129-entry table of six-decimal literals, bit for bit (host side;
 * midinote outside [0, 128], which the reference indexes out of bounds, returns 0). */
double mxg_mtof_host(int midinote);

/* ---- fused subtractive voice (saw -> lores -> adsr in registers, one store per sample) ---- */
/* mode 0: out = adsr(lores(saw(freq), cutoff, res), trig); coefficients hoisted: d_coef =
 *         [3][V] from mxg_filter_coeffs_host(MXG_FLT_LORES, ...) (bit-exact).
 * mode 1: e = adsr(1., trig); out = lores(saw(freq), e*cutoff, res) * e  (the call order of
 *         14.monosynth/main.cpp:50-55); cutoff is modulated per sample, coefficients on device,
 *         stated tolerance.  d_cutoff/d_res [V] are used, d_coef ignored.
 * d_ost = [2][V] osc phase/output; d_fst = [5][V] filter state; env arrays as mxg_env_render. */
int mxg_voice_render(int mode, size_t V, size_t N, const double *d_freq, const double *d_cutoff,
                     const double *d_res, const double *d_coef, const int32_t *d_trig, int tpv,
                     const double *d_par, const int64_t *d_holdtime, double *d_ost, double *d_fst,
                     double *d_dst, int64_t *d_ist, double *d_out, void *stream);
/* The same render with the maxiMix::stereo mixdown of the bank fused into it (C:503-509 applied voice after voice, the sum over
 * voices of the user's loop: 15.polysynth/main.cpp:54-70) -- the block is never read back.  d_out may be NULL (mix only).  The per-voice
 * block and every state array get mxg_voice_render's bits; the sum over voices is a fixed tree (tolerance on the mix, as
 * mxg_osc_render_mix).  _rows: d_rows[mxg_osc_mix_groups(V)][N][2], one row per 256 voices -- what a grouped mix queue's slot takes
 * (mxg_mixq_create_grouped) or mxg_mix_rows_sum adds; _mix: d_mix[N][2] (rows in library scratch + the row sum on `stream`).
 * Knob "voice_mix_store": the store stream of this form (0 automatic, 1 ... 5 as "voice_store"). */
int mxg_voice_render_mix_rows(int mode, size_t V, size_t N, const double *d_freq, const double *d_cutoff, const double *d_res,
                              const double *d_coef, const int32_t *d_trig, int tpv, const double *d_par, const int64_t *d_holdtime,
                              double *d_ost, double *d_fst, double *d_dst, int64_t *d_ist, double *d_out, const double *d_pan,
                              double *d_rows, void *stream);
int mxg_voice_render_mix(int mode, size_t V, size_t N, const double *d_freq, const double *d_cutoff, const double *d_res,
                         const double *d_coef, const int32_t *d_trig, int tpv, const double *d_par, const int64_t *d_holdtime,
                         double *d_ost, double *d_fst, double *d_dst, int64_t *d_ist, double *d_out, const double *d_pan, double *d_mix,
                         void *stream);

/* ---- maxiMix::stereo + mixdown over voices (C:503-509; user-side sum e.g. 15.polysynth:67) --- */
/* d_mix[n][0..1] = sum_v ( in[n][v]*sqrt(1-pan_v), in[n][v]*sqrt(pan_v) ).  The per-voice
 * products are exact; the sum over voices is a fixed-shape tree (deterministic, but not the
 * reference's sequential order => stated tolerance on the mix). d_mix is [N][2]. */
int mxg_mix_stereo(size_t V, size_t N, const double *d_in, const double *d_pan, double *d_mix,
                   void *stream);

/* maxiMix::stereo (channels 2, C:503-509), quad (4, C:512-522) or ambisonic (8, C:525-541) over a
 * bank: d_x/d_y/d_z are the per-voice [V] pan arguments (d_y for channels >= 4, d_z for 8).
 * d_bus, if not NULL, receives the per-voice bus signals bus[n][c][v] = what the reference leaves
 * in two/four/eight[c] for voice v at sample n (bit-exact, including ambisonic's quirks: z is
 * never clamped, `z>1` / `z<0` overwrite y, and eight[0..3] = input*(sqrt(..)*1.0 - z)).
 * d_mix [N][channels] = the sum over voices (fixed-shape tree, tolerance as mxg_mix_stereo). */
int mxg_mix_bus(int channels, size_t V, size_t N, const double *d_in, const double *d_x,
                const double *d_y, const double *d_z, double *d_bus, double *d_mix, void *stream);

/* ---- maxiDelayline bank ---------------------------------------------------------------- */
/* mode 0: dl(input, size, feedback) (C:420-429)   mode 1: dlFromPosition(input, size, feedback,
 * position) (C:431-439).  d_size int32 [V], d_feedback [V], d_position int32 [V] (mode 1).
 * d_mem = [cap][V] slot-major ring (the reference's per-object memory[88200*8], H:273, cut to
 * `cap` slots; every size must be <= cap), zero-initialise like the ctor (C:415-417);
 * d_phase int32 [V] in/out.  d_in/d_out are [N][V]. */
int mxg_delay_render(int mode, size_t V, size_t N, const double *d_in, const int32_t *d_size,
                     const double *d_feedback, const int32_t *d_position, double *d_mem, size_t cap,
                     int32_t *d_phase, double *d_out, void *stream);

/* ---- maxiFlanger / maxiChorus banks (H:1144-1212) ------------------------------------------- */
/* A delay line whose tap moves every sample.  ps_flags: a set bit makes that parameter [N][V] (one value per
 * call), a clear bit [V] (the same value for the whole block).  d_delay is uint32 (the reference's unsigned
 * delay).  Rings are VOICE-major: ring r of voice v is d_mem[(r*V + v)*cap .. +cap), zero-initialise like the
 * ctor (C:415-417).  d_phase (int32, the rings' maxiDelayline::phase) starts at 0 (value-initialised objects).
 * A tap size above `cap` is held to `cap` and, if d_overflow is not NULL, counted: d_overflow[v] (uint32) is
 * INCREASED by the number of clamped taps of the call -- the one defined departure from the reference, whose
 * ring is 705 600 slots and indexes past it there.  A size <= 0 (also NaN or beyond +-2^31, which x86 converts
 * to INT_MIN) resets the phase on every sample, as the reference does.  Bit-exact.  d_in / d_out are [N][V]. */
#define MXG_FX_PS_DELAY 1
#define MXG_FX_PS_FEEDBACK 2
#define MXG_FX_PS_SPEED 4
#define MXG_FX_PS_DEPTH 8
#define MXG_FX_PS_ALL 15
/* flange(in, delay, feedback, speed, depth) (H:1166-1172): one ring; d_phase [V]; d_lfo_phase [V] double =
 * maxiFlanger::lfo's maxiOsc::phase (the triangle, C:362-373, inc = 1./(sampleRate/speed)). */
int mxg_flanger_render(size_t V, size_t N, const double *d_in, const uint32_t *d_delay, const double *d_feedback,
                       const double *d_speed, const double *d_depth, int ps_flags, double *d_mem, size_t cap,
                       int32_t *d_phase, double *d_lfo_phase, uint32_t *d_overflow, double *d_out, void *stream);
/* chorus(in, delay, feedback, speed, depth) (H:1202-1212): two rings (dl, dl2), d_mem [2][V][cap], d_phase
 * [2][V].  d_rand int32 [N][V]: the rand() draw voice v's lfo.noise() takes at sample n (C:214-220).  The
 * speed enters only as lopass.lores's cutoff (resonance 1): d_coef = (c, r) from mxg_filter_coeffs_host
 * (MXG_FLT_LORES, speed, 1.0) rows 0-1, [2][V] (coef_ps 0) or [N][2][V] (coef_ps 1).  d_lp [2][V] = the lores
 * state x, y (maxiFilter::x, y).  ps_flags: MXG_FX_PS_DELAY / FEEDBACK / DEPTH. */
int mxg_chorus_render(size_t V, size_t N, const double *d_in, const uint32_t *d_delay, const double *d_feedback,
                      const double *d_depth, int ps_flags, const int32_t *d_rand, const double *d_coef, int coef_ps,
                      double *d_mem, size_t cap, int32_t *d_phase, double *d_lp, uint32_t *d_overflow, double *d_out,
                      void *stream);

/* ---- maxiDynamics / maxiRMS (H:2579-2897, K12) ----------------------------------------------
 * A bank of V compressor / expander / companders.  d_sig, d_control, d_out (and d_level_db, optional: the detector
 * level in dB each sample was compared with) are [N][V]; d_sig == d_control is compress() and is read once.  The six
 * parameters of maxiDynamics::play are [V], or [N][V] where their MXG_DYN_PS_* bit is set in ps_flags.  Per voice,
 * [V]: d_window (RMS window, samples), d_lookahead (samples; 0 = off), d_analyser (MXG_DYN_PEAK / MXG_DYN_RMS).
 * d_stages_high / d_stages_low: the [nstages][6] tables (mxg_envgen_stages_host, mxg_envgen_set_time_host) of
 * arEnvHigh / arEnvLow, one shape each per bank; the reference's are setupASR(10, 10), retrigger and loop off.
 * Carried state: d_rms_ring [cap_rms][V] and d_la_ring [cap_la][V] (slot-major; the reference's hold 500 ms and 1 s of
 * samples), d_rms_pos / d_la_pos int32 [V] (maxiRingBuf::idx; a stored position outside the ring restarts at slot 0),
 * d_running [V] (maxiRMS::runningRMS), and the envelopes' d_dst_* [5][V] / d_ist_* [7][V] exactly as
 * mxg_envgen_render keeps them (a fresh envelope: previousValue = 1 and firstTrigger = 1 for the three detectors,
 * everything else 0).  A window above cap_rms or a look-ahead above cap_la is held at the capacity and d_overflow [V]
 * (optional) is INCREASED by one per such parameter per call: the one defined departure from the reference.
 * Reproduces what the reference computes: outDB starts as log10(sig) * 20, so a sample with sig <= 0 that no section
 * overwrites gives exactly 0.0 and does NOT push the look-ahead ring; the scale is control / outAmp.
 * Bit-exact: the rings, positions, runningRMS, envelope states, overflow counts and the positions of NaN and exact
 * 0.0 in d_out -- as long as no detector level lies within the device log10's error (~1e-13 dB) of a boundary it is
 * compared with.  Tolerance: the non-zero values of d_out (device log10 and pow), d_level_db. */
#define MXG_DYN_PEAK 0
#define MXG_DYN_RMS 1
#define MXG_DYN_PS_THRESHOLD_HIGH 1
#define MXG_DYN_PS_RATIO_HIGH 2
#define MXG_DYN_PS_KNEE_HIGH 4
#define MXG_DYN_PS_THRESHOLD_LOW 8
#define MXG_DYN_PS_RATIO_LOW 16
#define MXG_DYN_PS_KNEE_LOW 32
#define MXG_DYN_PS_ALL 63
int mxg_dynamics_render(size_t V, size_t N, const double *d_sig, const double *d_control, const double *d_threshold_high,
                        const double *d_ratio_high, const double *d_knee_high, const double *d_threshold_low,
                        const double *d_ratio_low, const double *d_knee_low, int ps_flags, const uint32_t *d_window,
                        const uint32_t *d_lookahead, const int32_t *d_analyser, const double *d_stages_high,
                        const double *d_stages_low, int nstages, double *d_rms_ring, size_t cap_rms, double *d_la_ring,
                        size_t cap_la, int32_t *d_rms_pos, int32_t *d_la_pos, double *d_running, double *d_dst_high,
                        int64_t *d_ist_high, double *d_dst_low, int64_t *d_ist_low, uint32_t *d_overflow, double *d_out,
                        double *d_level_db, void *stream);
/* maxiRMS::play (H:2604-2610) alone, from the same code: d_ring [cap][V], d_pos [V], d_running [V], d_window [V]
 * (samples; above cap: held there and counted in d_overflow).  Bit-exact (the square root is correctly rounded). */
int mxg_rms_render(size_t V, size_t N, const double *d_in, const uint32_t *d_window, double *d_ring, size_t cap,
                   int32_t *d_pos, double *d_running, uint32_t *d_overflow, double *d_out, void *stream);
/* maxiEnvGen::setTime(index, ms) (H:2449-2462, setupSegmentTime H:2532-2546) on row `index` of a HOST [nstages][6]
 * table: length = floor(ms / 1000 * sampleRate), gradient = 1 / length, or a HOLD stage for ms == -46692.  Returns 0, or
 * 1 where setTime reports an error (a second HOLD stage; an index past the table, which the reference lets through
 * for index == nstages and then writes outside its vector).  Whether a HOLD stage exists is read off the table.
 * maxiDynamics::setAttackHigh / setReleaseHigh / setAttackLow / setReleaseLow are setupASR(10, 10) once, then
 * setTime(0, ms) / setTime(2, ms).  Host arithmetic only: bit-exact. */
int mxg_envgen_set_time_host(double *h_stages, size_t nstages, size_t index, double ms);
/* maxiEnvGen::setLevel(index, value) (H:2422-2437) and setCurve(index, value) (H:2440-2446) on a HOST [nstages][6] table.
 * setLevel writes startlevel of row `index` and endlevel of row `index - 1`; index == nstages writes the last row's endlevel
 * only; beyond that it returns 1 (the reference's `error`), else 0.  setCurve writes the curve of row `index` and returns 0
 * always; for index >= nstages it writes nothing (the reference writes outside its vector for index == nstages).  A null table
 * or nstages outside 1 .. 32: MXG_ERR_INVALID. */
int mxg_envgen_set_level_host(double *h_stages, size_t nstages, size_t index, double value);
int mxg_envgen_set_curve_host(double *h_stages, size_t nstages, size_t index, double value);

/* ---- maxiSatReverb / maxiFreeVerb / maxiFreeVerbStereo (libs/maxiReverb.h, K13) ------------------------------------
 * A bank of V reverbs.  Every delay length is a constant of the class (samples, independent of the sample rate):
 *   MXG_REVERB_SAT              4 plain combs 778 901 1011 1123, 3 allpasses 125 42 12
 *   MXG_REVERB_FREEVERB         8 low-pass combs 1557 1617 1491 1422 1277 1356 1188 1116, 31 allpasses 225 556 441 341 and
 *                               13 * (j + 1) for j = 4 .. 30
 *   MXG_REVERB_FREEVERB_STEREO  the same 8 combs, run plain, and the first 4 allpasses
 * mxg_reverb_layout_host answers these per kind (any output may be NULL): the number of combs and allpasses, the doubles
 * of ring state per voice (3 992 / 18 905 / 12 587) and, for filter f = 0 .. combs + allpasses - 1 (combs first), its
 * length and its first slot inside the voice's ring area (lengths / offsets: room for MXG_REVERB_MAX_FILTERS).
 * Carried state, caller-owned device memory, zero-initialised like the constructors: d_rings [V][ring_doubles]
 * (VOICE-major; filter f of voice v at d_rings[v * ring_doubles + offsets[f]]), d_idx int32 [V][combs + allpasses] (the ring
 * indices; one outside its ring restarts at slot 0), and for MXG_REVERB_FREEVERB d_lp [V][8] (the combs' low-pass states)
 * and d_wc [V][2] = (w, cut), which a fresh object holds at (0.84, 0.2) -- not zero.  The other kinds take NULL there.
 * d_in is [N][V]; d_out [N][V], for the stereo kind [2][N][V] (left, right).
 * mode (MXG_REVERB_FREEVERB only, otherwise MXG_REVERB_PLAY): MXG_REVERB_PLAY = play(x): d_wc as it stands, 4 allpasses,
 * the parameters are not read (NULL allowed).  MXG_REVERB_PLAY_PARAMS = play(x, roomsize, absorbtion): every sample first sets
 * w = clamp01(roomsize * 0.10 + 0.84) and cut = clamp01(absorbtion) (a NaN stays a NaN), runs all 31 allpasses, and the last
 * sample's (w, cut) stay in d_wc.  d_roomsize / d_absorbtion are [V], or [N][V] behind their MXG_REVERB_PS_* bit.
 * What the reference computes is kept, quirks included: both filters run at 0.85 whatever gains the constructors store;
 * the stereo class's right channel is the allpass chain fed 0.0 on the SAME four rings, a second step in the same sample,
 * and its roomsize / absorbtion are read by nothing, so this entry point does not take them.
 * Bit-exact (+ - * only, contraction off, subnormals kept): outputs and every piece of state. */
#define MXG_REVERB_SAT 0
#define MXG_REVERB_FREEVERB 1
#define MXG_REVERB_FREEVERB_STEREO 2
#define MXG_REVERB_PLAY 0
#define MXG_REVERB_PLAY_PARAMS 1
#define MXG_REVERB_PS_ROOMSIZE 1
#define MXG_REVERB_PS_ABSORBTION 2
#define MXG_REVERB_PS_ALL 3
#define MXG_REVERB_MAX_FILTERS 39
int mxg_reverb_layout_host(int kind, uint32_t *n_combs, uint32_t *n_allpasses, uint32_t *ring_doubles, uint32_t *lengths,
                           uint32_t *offsets);
int mxg_reverb_render(int kind, int mode, size_t V, size_t N, const double *d_in, const double *d_roomsize,
                      const double *d_absorbtion, int ps_flags, double *d_rings, int32_t *d_idx, double *d_lp, double *d_wc,
                      double *d_out, void *stream);

/* ---- maxiDattaroReverb (libs/maxiReverb.h, K14) ---------------------------------------------------------------------
 * A bank of V plate reverbs after Dattorro, stereo out.  Unlike the three classes above, every delay length follows the
 * sample rate in force when the object is constructed, in the reference's float arithmetic:
 *   floor(((float)orig / 29.8f) * ((float)sample_rate / 1000.0f)).
 * A voice owns ten rings, in this order inside its ring area (orig, the length at 29.8 kHz, in brackets):
 *   0 AP0 [142]   1 AP1 [107]      the input allpasses (fbap[0], fbap[1]), each stepped TWICE a sample
 *   2 AP4 [908]   3 AP5 [2656]   4 AP6 [672]   5 AP7 [1800]     the tank allpasses (fbap[4 .. 7])
 *   6 D0  [4217]  7 D1  [3163]   8 D2  [4453]  9 D3  [3720]     the tank delays
 * and reads fourteen taps (orig 266 2974 1913 1996 1990 187 1066 353 3627 1228 2673 2111 335 121) from rings
 * 6 6 3 7 8 5 9 8 8 5 9 6 3 7.  At 44 100 Hz: lengths 210 158 1343 3930 994 2663 6240 4680 6589 5505.
 * mxg_dattaro_layout_host needs no device and answers, for a sample rate (any output may be NULL): lengths [10],
 * offsets [10] (the ring's first slot inside the voice's ring area), the ring doubles per voice, tap_positions [14] and
 * tap_rings [14].  A rate is accepted exactly when every length lies in [2, 44100] (the reference's ring size) and a
 * tile of 64 samples is legal on rings 2 .. 9 (64 <= length) and on every tap (length - 1 - position is 0 or >= 64).
 * That holds from 3 345 to 295 129 Hz except for 3 349 .. 3 360 and 3 374 .. 3 377; any other rate fails with
 * MXG_ERR_INVALID and a message that names the range.
 * Carried state, caller-owned device memory, all zero for a fresh object: d_rings [V][ring_doubles] (VOICE-major; ring r
 * of voice v at d_rings[v * ring_doubles + offsets[r]]), d_idx int32 [V][10] (the ring indices; one outside its ring
 * restarts at slot 0), d_state [V][5] = the three one-pole low-pass states lp0 lp1 lp2, then sigl, sigr (the tank's
 * cross feedback).  d_in is [N][V]; d_out [2][N][V] (left, right).  The same sample_rate must accompany a bank for its
 * whole life: the layout is a function of it.
 * What the reference computes is kept, quirks included: the second input allpass pair runs on rings AP0 and AP1 again
 * (fbap[2], fbap[3] are never touched), and gettap uses the index after the step.  The 3 100-slot pre-delay ring is
 * written and read by every call, but its output is used by nothing and the ring is private: it cannot be observed, and
 * the bank does not carry it.
 * Bit-exact (+ - * only, contraction off, subnormals kept): outputs and every piece of state.  No CPU fallback. */
#define MXG_DATTARO_RINGS 10
#define MXG_DATTARO_TAPS 14
#define MXG_DATTARO_STATE 5
int mxg_dattaro_layout_host(uint32_t sample_rate, uint32_t *lengths, uint32_t *offsets, uint32_t *ring_doubles,
                            uint32_t *tap_positions, uint32_t *tap_rings);
int mxg_dattaro_render(uint32_t sample_rate, size_t V, size_t N, const double *d_in, double *d_rings, int32_t *d_idx,
                       double *d_state, double *d_out, void *stream);

/* ---- custom reverb networks out of maxiReverbFilters stages (libs/maxiReverb.h:42-73, K30) ---------------------------
 * A bank of V reverbs that share one topology the caller chooses: n_combs parallel feedback combs summed in order, then
 * n_allpasses serial allpasses, each count in [0, MXG_REVNET_MAX_STAGES], their sum at least 1.  Per sample and voice:
 *   acc = 0.0; acc += comb_c(x) for c = 0 .. n_combs - 1;  t = acc (t = x without combs);  t = allpass_a(t) in order;  out = t
 * where comb c is maxiReverbFilters::combfb(x, size, fb), or lpcombfb(x, size, fb, cutoff) where comb_lowpass[c] != 0
 * (comb_lowpass may be NULL: every comb plain), and allpass a is allpass(x, size, fb).  The sizes are host arrays of
 * integer lengths in samples, [1, 44100] (the reference's ring); they are per bank and must accompany it for its whole
 * life.  A low-pass comb must be at least 64 samples long; plain combs and allpasses may have any length from 1.
 * mxg_revnet_layout_host needs no device: it checks a topology (MXG_ERR_INVALID and a message otherwise) and answers
 * offsets [n_combs + n_allpasses] (stage f's first slot inside the voice's ring area, combs first) and the ring doubles
 * per voice, the sum of the lengths (either output may be NULL).
 * Parameters, device arrays, per voice and stage, constant within a call and free to change between calls; nothing
 * clamps them, as nothing does in the reference: d_comb_fb [V][n_combs], d_comb_cut [V][n_combs] (read for low-pass combs
 * only; NULL allowed without one), d_ap_fb [V][n_allpasses].
 * Carried state, caller-owned device memory, all zero for fresh objects: d_rings [V][ring_doubles] (VOICE-major; stage f of
 * voice v at d_rings[v * ring_doubles + offsets[f]]), d_idx int32 [V][n_combs + n_allpasses] (the ring indices; one
 * outside its ring restarts at slot 0), d_lp [V][n_combs] (the low-pass combs' filter states; NULL allowed without one).
 * d_in and d_out are [N][V], any N, any V, any split of a stream into calls.
 * Bit-exact (+ - * only, contraction off, subnormals kept): outputs and every piece of state.  No CPU fallback. */
#define MXG_REVNET_MAX_STAGES 32
int mxg_revnet_layout_host(uint32_t n_combs, uint32_t n_allpasses, const uint32_t *comb_sizes, const uint32_t *ap_sizes,
                           const uint32_t *comb_lowpass, uint32_t *offsets, uint32_t *ring_doubles);
int mxg_revnet_render(uint32_t n_combs, uint32_t n_allpasses, const uint32_t *comb_sizes, const uint32_t *ap_sizes,
                      const uint32_t *comb_lowpass, size_t V, size_t N, const double *d_in, const double *d_comb_fb,
                      const double *d_comb_cut, const double *d_ap_fb, double *d_rings, int32_t *d_idx, double *d_lp,
                      double *d_out, void *stream);

/* ---- sequencers: maxiRatioSeq / maxiStep / maxiCounter / maxiIndex / maxiZXToPulse / maxiTrigger::onZX (K15) ---------
 * (H:564-596, 1953-2013, 2093-2262.)  Compares, + - / floor and integer indexing only: every output and every state array is
 * BIT-EXACT.  The one departure: a table read index is held inside its table where the reference would index out of bounds
 * (maxiStep with step < -len, a NaN index, an uploaded state out of range).
 *
 * Tables are block-constant; a caller changes them between blocks.  A table is doubles [P][L] with int32 lengths [P] (row p
 * counts its first len[p] entries; a length is held in [1, L] on the device).  A voice picks its row with an int32 [V]
 * selector (NULL = row 0 for every voice; held in [0, P - 1]).  All tables of one call fit 48 KB.
 *
 * mxg_seq_ratio_host: maxiRatioSeq::playTrig's boundaries (H:2172-2186) for P patterns of at most L <= 64 ratios, on the host,
 * the reference's operations in the reference's order: h_norm[p][i] = (times[0] + ... + times[i]) / sum, a boundary equal to 1.0
 * becomes 0.0; entries past h_len[p] are NaN (never fire).  Refuses L > 64 and a length < 1 or > L.
 *
 * mxg_seq_render, the fused sequencer, per voice and sample:
 *     phase = maxiOsc::phasor(d_freq[v])                    internal clock: d_freq [V], d_clk [V] = maxiOsc::phase, in/out --
 *                                                           bit for bit mxg_osc_render(MXG_OSC_PHASOR); d_phase NULL
 *           | d_phase[n][v] (phase_pv = 1) | d_phase[n] (phase_pv = 0)      external clock: d_freq and d_clk NULL
 *     trig  = maxiRatioSeq::playTrig(phase, pattern d_pat[v] of d_norm / d_len [P][L])            -> d_trig [N][V]
 *     val   = playValues(phase, pattern, values)                      val_mode MXG_SEQ_VAL_VALUES
 *           | maxiStep::pull(trig, values, d_step[v])                 val_mode MXG_SEQ_VAL_STEP   -> d_val  [N][V]
 *             with values = list d_vpat[v] of d_values / d_vlen [PV][LV]; d_step NULL = 1
 *     gate  = maxiZXToPulse::play(trig, d_hold[v])  (samples; d_hold NULL = 0)                     -> d_gate [N][V]
 * Each output is optional (at least one): a stage whose output is NULL does not run and its state is untouched; playTrig always
 * runs.  d_trig / d_gate are what mxg_envgen_render reads with tpv = 1, d_val what mxg_osc_render reads with fps = 1.
 * State, in/out: d_dst [5][V] doubles = maxiRatioSeq::prevPhase | maxiStep: trig.previousValue, index |
 * maxiZXToPulse: trig.previousValue, holdCounter;  d_ist [6][V] int64 = maxiRatioSeq: first, counter, lengthOfValues |
 * maxiStep: trig.firstTrigger, first | maxiZXToPulse: trig.firstTrigger.  Fresh objects: all zero except previousValue = 1.0
 * (d_dst rows 1, 3) and the four first flags = 1 (d_ist rows 0, 3, 4, 5).  1 / sampleRate is read at the call (mxg_settings).
 *
 * mxg_seq_signal: one of the classes driven by the caller's signals, d_in / d_in2 / d_out [N][V] (d_out distinct from the inputs):
 *     MXG_SEQ_ONZX       maxiTrigger::onZX(d_in)                       d_dst: previousValue                 d_ist: firstTrigger
 *     MXG_SEQ_COUNTER    maxiCounter::count(d_in, d_in2)               value, inc.previousValue, rst.previousValue | inc.first, rst.first
 *     MXG_SEQ_STEP       maxiStep::pull(d_in, values, d_par[v])        trig.previousValue, index            | trig.firstTrigger, first
 *     MXG_SEQ_INDEX      maxiIndex::pull(d_in, d_in2, values)          trig.previousValue, value            | trig.firstTrigger
 *     MXG_SEQ_ZXTOPULSE  maxiZXToPulse::play(d_in, d_par[v])           trig.previousValue, holdCounter      | trig.firstTrigger
 * d_dst is [3][V] doubles and d_ist [2][V] int64 for every kind (rows a kind does not use are left alone); fresh objects:
 * every previousValue 1.0, every first flag 1, the rest 0.  d_par NULL = step 1 / hold 0. */
#define MXG_SEQ_MAX_RATIOS 64
#define MXG_SEQ_VAL_VALUES 0
#define MXG_SEQ_VAL_STEP 1
#define MXG_SEQ_ONZX 0
#define MXG_SEQ_COUNTER 1
#define MXG_SEQ_STEP 2
#define MXG_SEQ_INDEX 3
#define MXG_SEQ_ZXTOPULSE 4
int mxg_seq_ratio_host(size_t P, size_t L, const int32_t *h_len, const double *h_times, double *h_norm);
int mxg_seq_render(size_t V, size_t N, const double *d_freq, double *d_clk, const double *d_phase, int phase_pv,
                   const double *d_norm, const int32_t *d_len, size_t P, size_t L, const int32_t *d_pat, int val_mode,
                   const double *d_values, const int32_t *d_vlen, size_t PV, size_t LV, const int32_t *d_vpat,
                   const double *d_step, const double *d_hold, double *d_dst, int64_t *d_ist, double *d_trig, double *d_val,
                   double *d_gate, void *stream);
int mxg_seq_signal(int kind, size_t V, size_t N, const double *d_in, const double *d_in2, const double *d_values,
                   const int32_t *d_vlen, size_t PV, size_t LV, const int32_t *d_vpat, const double *d_par, double *d_dst,
                   int64_t *d_ist, double *d_out, void *stream);

/* ---- analysis: maxiZeroCrossingDetector / maxiZeroCrossingRate / maxiEnvelopeFollower / maxiSampleAndHold (K16) ------
 * (H:969-1040, 1214-1250.)  Compares, + - *, integer counts and indexing only: every output and every state array is
 * BIT-EXACT.  Two defined departures: a window above cap is held at cap and counted in d_overflow, where the reference indexes
 * out of bounds; the crossing count is a signed 64-bit integer, where the reference's size_t would pass through a negative
 * double when the window changes over a filled ring.  A negative or NaN hold time (undefined in the reference) is 0 samples.
 *
 * mxg_analysis_render, one fused pass over d_in [N][V]; `want` is a non-empty set of MXG_ANA_WANT_* bits, per voice and sample:
 *     zx   = maxiZeroCrossingDetector::zx(x): (prev <= 0 && x > 0), prev = x; 0.0 / 1.0              -> d_zx      [N][V]
 *     zcr  = maxiZeroCrossingRate::play(x): push zx, count += zx, count -= tail(d_window[v])         -> d_zcr     [N][V]
 *     env  = maxiEnvelopeFollower::play(x): a = fabs(x); env = (a > env ? attack : release) * (env - a) + a -> d_env_out [N][V]
 *     sah  = maxiSampleAndHold::sah(x, ms), hold = (double)(size_t)(ms / 1000 * sampleRate) per sample -> d_sah   [N][V]
 * A stage that is not wanted does not run: its state, parameter and output pointers are not read and may be NULL.  zx and zcr
 * share one detector (d_prev_x); zx alone needs only d_prev_x.  The outputs are distinct from d_in and from each other; they are
 * what mxg_envgen_render (tpv = 1), mxg_seq_signal and mxg_dynamics_render (d_control) read.
 * State, in/out (fresh objects: all zero):
 *     d_prev_x [V]                    the detector's previous_x
 *     d_zring  u64 [ceil(cap/64)][V]  the ring of crossings, one BIT per slot, word-major: slot s is bit s & 63 of word s >> 6 of
 *                                     the voice's column; the last word is partial when cap % 64 != 0 (its upper bits are unused)
 *     d_zpos   i32 [V]                maxiRingBuf::idx; a stored position outside [0, cap) restarts at slot 0
 *     d_zcount i64 [V]                runningCount
 *     d_overflow u32 [V] (optional)   INCREASED by one per call for a voice whose window is above cap
 *     d_env [V]; d_sah_phase, d_sah_value [V]
 * Parameters: d_window u32 [V] in samples (the reference reads maxiSettings::sampleRate at play time against a ring sized at
 * construction; 0 is the caller's error -- mxg_analysis_window_host refuses it, the kernel stays inside the ring);
 * d_attack, d_release [V] from mxg_envfollow_coeff_host; d_hold_ms [V], or [N][V] with hold_per_sample = 1.  The sample rate of
 * the hold time is read at the call (mxg_settings).
 * mxg_envfollow_coeff_host: pow(0.01, 1.0 / (ms * sample_rate * 0.001)) with the host libm, the reference's own expression
 * (setAttack / setRelease, H:1224-1231) -- the policy of the filter coefficients.
 * mxg_analysis_window_host: the host check of h_window [V] before upload: refuses cap == 0 and a window of 0. */
#define MXG_ANA_WANT_ZX 1
#define MXG_ANA_WANT_ZCR 2
#define MXG_ANA_WANT_ENV 4
#define MXG_ANA_WANT_SAH 8
#define MXG_ANA_WANT_ALL 15
double mxg_envfollow_coeff_host(double ms, double sample_rate);
int mxg_analysis_window_host(size_t V, const uint32_t *h_window, size_t cap);
int mxg_analysis_render(size_t V, size_t N, const double *d_in, int want, double *d_prev_x, const uint32_t *d_window,
                        uint64_t *d_zring, size_t cap, int32_t *d_zpos, int64_t *d_zcount, uint32_t *d_overflow,
                        const double *d_attack, const double *d_release, double *d_env, const double *d_hold_ms,
                        int hold_per_sample, double *d_sah_phase, double *d_sah_value, double *d_zx, double *d_zcr,
                        double *d_env_out, double *d_sah, void *stream);

/* ---- maxiKuramotoOscillatorSet / maxiAsyncKuramotoOscillator (K17) ------------------------------------------------------
 * (H:1628-1808.)  S sets of N phase-coupled oscillators (N = 1 .. 64; 0 and more than 64 are refused without a launch), B
 * samples per call.  Per set and sample, as maxiKuramotoOscillatorSet::play(freq, K):
 *     gathered[j] = phase[j] for all j;  then for every oscillator i, in order,
 *     adj = sum over j, in order, of sin(gathered[j] - phase[i]);
 *     phase[i] += dt * (freq + ((K / (double)N) * adj));  one wrap into [0, TWOPI);
 *     mix = (sum of the new phases in i order) / (double)N.
 * dt = TWOPI / sampleRate, read at the call (mxg_settings).  Everything but the sine keeps the reference's expression trees; the
 * sine is the library's own (within 1 ULP of glibc's per term), so phases and mix stay within the reference's own accumulated
 * rounding -- and are bit-identical to the host build of maximilian_amd/csrc/mxg_kuramoto.h.
 * mode bits:
 *     MXG_KURA_MEANFIELD  a TOLERANCE mode: adj = cos(phase[i]) * S - sin(phase[i]) * C with S = sum_j sin(gathered[j]),
 *                         C = sum_j cos(gathered[j]) in j order -- N sine / cosine pairs per sample instead of N * N sines
 *     MXG_KURA_ASYNC      maxiAsyncKuramotoOscillator: d_gathered is refreshed from the phases, and K applied, only on the first
 *                         sample of a call whose d_update[s] is non-zero; the kernel clears the flag.  Every other sample plays
 *                         K = 0 on the stale gathered phases.  (The sum is left out where that provably changes nothing: all
 *                         phases of the wavefront's sets within |32| and freq not -0.0; a non-finite phase propagates as in the
 *                         reference.)
 * d_freq, d_K: one value per set [S], or with freq_per_sample / K_per_sample a block [B][S] (what the other banks write).
 * State, in/out: d_phase [S][N] (set-major); async only: d_gathered [S][N], d_update i32 [S] (both may be NULL otherwise).
 * The reference's setPhase / setPhases between two calls is a write to d_phase (and, async, raising d_update[s]).
 * Outputs, any subset chosen by `want` (an unwanted block is not written and may be NULL; want = 0 only advances the state):
 *     MXG_KURA_WANT_MIX     d_mix        [B][S]      what play() returns
 *     MXG_KURA_WANT_PHASES  d_phases_out [B][S][N]   what getPhase(i) returns after each sample
 * Phases beyond |32| (the caller's setPhase; the wrap is applied once per sample) take the platform's sine above |x| = 64: still
 * within 1 ULP per term, no longer bit-identical to the host build. */
#define MXG_KURA_MEANFIELD 1
#define MXG_KURA_ASYNC 2
#define MXG_KURA_WANT_MIX 1
#define MXG_KURA_WANT_PHASES 2
int mxg_kuramoto_render(int mode, size_t S, size_t N, size_t B, const double *d_freq, int freq_per_sample, const double *d_K,
                        int K_per_sample, double *d_phase, double *d_gathered, int32_t *d_update, int want, double *d_mix,
                        double *d_phases_out, void *stream);

/* ---- the same classes for sets of up to 1024 oscillators (K26) ------------------------------------------------------------
 * mxg_kuramoto_wide_render: the arguments, layouts, mode and want bits of mxg_kuramoto_render, for N = 1 .. 1024 (0 and more than
 * 1024 are refused without a launch).  One workgroup per set and one lane per oscillator, two workgroup barriers per sample: it
 * pays from N = 65 on; for N <= 64 it is accepted and gives mxg_kuramoto_render's bits, but with one set per workgroup instead of
 * 64 / W per wavefront.  The results are bit-identical to the host build of maximilian_amd/csrc/mxg_kuramoto.h
 * (tests/host_kuramoto_wide.cpp) and stay within the reference's own accumulated rounding.  The choice
 * between the trusted and the general sine, and the async skip, look at all phases of the SET (not of the wavefront). */
#define MXG_KURA_WIDE_MAX_N 1024
int mxg_kuramoto_wide_render(int mode, size_t S, size_t N, size_t B, const double *d_freq, int freq_per_sample, const double *d_K,
                             int K_per_sample, double *d_phase, double *d_gathered, int32_t *d_update, int want, double *d_mix,
                             double *d_phases_out, void *stream);

/* ---- shapers, cross-fade, select and line: maxiNonlinearity / maxiDistortion, maxiXFade, maxiSelect(X), maxiLine (K18) ----
 * (H:1046-1139, 1491-1617, 2018-2088.)  All blocks are [N][V] doubles.  The first three are streams without a recurrence over
 * time: flat over the N * V elements, 16-byte accesses where every pointer is 16-byte aligned (else, and with the knob rw_store
 * = 1, 8-byte ones); a per-voice parameter [V] is read at element % V.
 *
 * mxg_shape_render: d_out[i] = maxiNonlinearity::<mode>(d_in[i], ...); d_out == d_in (in place) is allowed.
 *     MXG_SHAPE_HARDCLIP, _FASTATAN                 no parameter (d_a, d_b may be NULL)                        BIT-EXACT
 *     MXG_SHAPE_SOFTCLIP                            no parameter; the cube is (x * x) * x for the reference's pow(x, 3): at most
 *                                                   2^-52 absolute from it, bit-identical to the host build of mxg_shaper.h
 *     MXG_SHAPE_FASTATANDIST  d_a = shape                                                                      BIT-EXACT
 *     MXG_SHAPE_ATANDIST      d_a = shape, d_b = 1.0 / atan(shape) from mxg_atan_norm_host (per voice only; with per_sample the
 *                             factor is formed on the device and d_b is not read); the device's atan: tolerance, DESIGN.md
 *     MXG_SHAPE_ASYMCLIP      d_a = a (the exponent of the NEGATIVE half, as the reference uses it), d_b = b; the device's pow:
 *                             tolerance, DESIGN.md
 * The clipped branches (|x| >= 1 gives exactly +-1) and NaN positions are the reference's in every mode.  per_sample = 0: d_a, d_b
 * are [V]; 1: blocks [N][V] (K16's hold_per_sample convention).
 * mxg_atan_norm_host: 1.0 / atan(shape) with the host libm, the reference's own expression (H:1128).
 *
 * mxg_xfade_render: maxiXFade::xfade over C = 1 .. 8 channels: d_ch1, d_ch2, d_out are [C][N][V]; d_xfader is [V], or [N][V] with
 * xfader_per_sample.  n = linlin(clamp(x, -1, 1), -1, 1, 0, 1) in the reference's operation order, the gains sqrt(1.0 - n) and
 * sqrt(n) are formed once per element and applied to all C channels: out = (ch1 * g1) + (ch2 * g2).  BIT-EXACT.  d_out may be
 * d_ch1 or d_ch2.
 *
 * mxg_select_render: maxiSelect::play (interpolate = 0) / maxiSelectX::play (1) over K = 1 .. 64 values: d_index [N][V]; d_values
 * [K][V] constants, or with values_are_signals [K][N][V].  normalised: index *= (K - 1e-9).  Below 0 -> 0, >= K -> K - 1.
 * SelectX: a1 = floor(index), a2 = a1 + 1 wrapping to 0, mix = index - a1, (v[a1] * (1.0 - mix)) + (v[a2] * mix).  BIT-EXACT.
 * One defined departure: a NaN index (undefined in the reference: it falls through both clamps into a cast) is taken as index
 * 0.0 -- it reads element 0 -- and is counted per voice in d_nan_count u32 [V] when that is not NULL (INCREASED, never cleared).
 *
 * mxg_line_render: maxiLine::play per voice and sample; d_trig [N][V], or NULL: the constant trig_const on every sample
 * (line.play(1)).  d_par [5][V] = lineStart, lineEnd, inc, oneShot, trigEnable (the last two: non-zero = true); d_st [4][V], in/out
 * = lineValue, lastTrigVal, triggered, lineComplete (fresh objects: 0, -1, 0, 0; the flags are 0.0 / 1.0).  BIT-EXACT, the state
 * included.  d_out is distinct from d_trig.  inc of +-Inf or NaN (a duration of 0) is not refused: the compares decide, as in
 * the reference.
 * mxg_line_prepare_host: maxiLine::prepare on HOST copies of d_par / d_st for the voices whose h_mask is non-zero (NULL: all):
 * lineValue takes the PREVIOUS lineStart (the reference's order of assignments), inc = (end - start) / (ms / 1000.0 *
 * sample_rate), triggered and lineComplete are reset; lastTrigVal and trigEnable stay. */
#define MXG_SHAPE_HARDCLIP 0
#define MXG_SHAPE_SOFTCLIP 1
#define MXG_SHAPE_FASTATAN 2
#define MXG_SHAPE_FASTATANDIST 3
#define MXG_SHAPE_ATANDIST 4
#define MXG_SHAPE_ASYMCLIP 5
#define MXG_SHAPE_MODES 6
#define MXG_SELECT_MAX_K 64
#define MXG_XFADE_MAX_C 8
double mxg_atan_norm_host(double shape);
int mxg_shape_render(int mode, size_t V, size_t N, const double *d_in, const double *d_a, const double *d_b, int per_sample,
                     double *d_out, void *stream);
int mxg_xfade_render(size_t C, size_t V, size_t N, const double *d_ch1, const double *d_ch2, const double *d_xfader,
                     int xfader_per_sample, double *d_out, void *stream);
int mxg_select_render(int interpolate, size_t K, size_t V, size_t N, const double *d_index, const double *d_values,
                      int values_are_signals, int normalised, uint32_t *d_nan_count, double *d_out, void *stream);
int mxg_line_prepare_host(size_t V, const double *h_start, const double *h_end, const double *h_ms, const int32_t *h_oneshot,
                          const int32_t *h_mask, double sample_rate, double *h_par, double *h_st);
int mxg_line_render(size_t V, size_t N, const double *d_trig, double trig_const, const double *d_par, double *d_st, double *d_out,
                    void *stream);

/* ---- the classic core classes: maxiDyn, maxiEnvelope, maxiLagExp<double>, maxiMap, maxiConvert (K23) -------------------------
 * (src/maximilian.cpp:377-412, 1200-1314; src/maximilian.h:499-560, 801-854, 955-961.)  All blocks are [N][V] doubles.  The
 * sample rate in force is mxg_settings's.  Every mxg_*_render below has a twin mxg_*_host with the same arguments but the stream,
 * which runs the same arithmetic (maximilian_amd/csrc/mxg_classic.h) on HOST arrays and needs no device.
 *
 * mxg_dyn_gate_render: d_out[n][v] = bank[v].gate(d_in[n][v], threshold, holdtime, attack, release) (C:1200-1235).  BIT-EXACT, the
 * state included.  mxg_dyn_compress_render: maxiDyn::compressor(input, ratio, threshold, attack, release) (C:1238-1267); d_makeup
 * is 1 + log(ratio) from mxg_dyn_makeup_host (the host libm, the reference's expression), in the layout of d_ratio: the device
 * path has no transcendental and is BIT-EXACT.  maxiDyn::compress(input) (C:1269-1298) is the same step with the object's own
 * members as parameters; note that setAttack stores mxg_dyn_coeff_host(ms, sample_rate) = pow(0.01, 1.0 / (ms * sr * 0.001)),
 * which compress() then uses as 1 + attack (kept).
 *   d_threshold, d_attack, d_release, d_ratio (+ d_makeup): [V], or [N][V] where their MXG_CLASSIC_PS_* bit is set in ps_flags
 *   (ratio and makeup travel together); d_holdtime int64 [V].
 *   State, in/out, shared by gate and compressor as the members of one maxiDyn are: d_dst double [3][V] = amplitude,
 *   currentRatio, output; d_ist int64 [4][V] = holdcount, attackphase, holdphase, releasephase.  Fresh objects: all zero.
 *   d_out is distinct from d_in.
 *
 * mxg_envelope_line_render: d_out[n][v] = bank[v].line(d_count[v], segments of voice v) (C:377-402).  d_segments [S][V], S = 2 ..
 * 64 entries (value, time, value, time ...), d_count int32 [V] = numberofsegments.  d_trig: NULL, or a block [N][V]: a non-zero
 * value at sample n performs trigger(d_trig_index[v], d_trig_amp[v]) (C:407-412) before that sample's line().  State, in/out:
 * d_dst double [2][V] = amplitude, startval; d_ist int32 [2][V] = valindex, isPlaying.  Fresh objects: all zero (output 0 until
 * triggered).  BIT-EXACT, the state included; a zero segment time gives the reference's IEEE infinities and NaNs.  The
 * reference's reads past its table (segments[valindex + 2], and segments[n], segments[n + 1] for one call after the last
 * segment) reach no result and are not made.  One defined departure: every table index is held inside [0, count - 1] and a
 * trigger index inside [0, count - 2], where the reference would index out of its vector (d_count itself is held inside
 * [1, S]; a legal one is 2 .. S).  d_out is distinct from d_trig.
 * mxg_envelope_trigger_host: trigger(h_index[v], h_amp[v]) on HOST copies of d_dst / d_ist for the voices whose h_mask is
 * non-zero (NULL: all); an index outside [0, h_count[v] - 2] is refused and nothing is changed.
 *
 * mxg_lag_render: val = (alpha * x) + (alphaReciprocal * val) (H:523-526), d_out[n][v] = the new val.  d_alpha and
 * d_alpha_reciprocal are independent ([V], or both [N][V] with alpha_per_sample); d_val [V] in/out.  BIT-EXACT.  d_out is
 * distinct from d_in.
 *
 * mxg_map_render: stateless and flat over the N * V elements like mxg_shape_render; d_out == d_in is allowed.  d_range [4][V] =
 * inMin, inMax, outMin, outMax per voice.  The clip is max(min(val, inMax), inMin) as the reference's compares: a NaN passes.
 *     MXG_MAP_LINLIN                                                                                            BIT-EXACT
 *     MXG_MAP_LINEXP    the device's pow                                                             tolerance, DESIGN.md
 *     MXG_MAP_EXPLIN    d_aux [V] = log(inMax / inMin) from mxg_map_range_host; the device's log     tolerance, DESIGN.md
 *     MXG_MAP_CLAMP     d_range rows 0, 1 = low, high ([2][V] is enough)                                        BIT-EXACT
 *     MXG_MAP_AMPTODBS  log10(x) * 20.0, no range (d_range may be NULL); the device's log10          tolerance, DESIGN.md
 *     MXG_MAP_DBSTOAMP  pow(10.0, x * 0.05), no range; the device's pow                              tolerance, DESIGN.md
 * Positions of NaN and +-Inf are the reference's in every mode.
 * mxg_map_range_host: h_aux [V] for `mode` from a host copy of d_range (explin: log(inMax / inMin) with the host libm; else 0). */
#define MXG_MAP_LINLIN 0
#define MXG_MAP_LINEXP 1
#define MXG_MAP_EXPLIN 2
#define MXG_MAP_CLAMP 3
#define MXG_MAP_AMPTODBS 4
#define MXG_MAP_DBSTOAMP 5
#define MXG_MAP_MODES 6
#define MXG_ENVELOPE_MAX_S 64
#define MXG_CLASSIC_PS_THRESHOLD 1
#define MXG_CLASSIC_PS_ATTACK 2
#define MXG_CLASSIC_PS_RELEASE 4
#define MXG_CLASSIC_PS_RATIO 8
#define MXG_CLASSIC_PS_MASK 15
double mxg_dyn_coeff_host(double ms, double sample_rate);
double mxg_dyn_makeup_host(double ratio);
int mxg_dyn_gate_render(size_t V, size_t N, const double *d_in, const double *d_threshold, const double *d_attack, const double *d_release,
                        int ps_flags, const int64_t *d_holdtime, double *d_dst, int64_t *d_ist, double *d_out, void *stream);
int mxg_dyn_gate_host(size_t V, size_t N, const double *h_in, const double *h_threshold, const double *h_attack, const double *h_release,
                      int ps_flags, const int64_t *h_holdtime, double *h_dst, int64_t *h_ist, double *h_out);
int mxg_dyn_compress_render(size_t V, size_t N, const double *d_in, const double *d_ratio, const double *d_makeup, const double *d_threshold,
                            const double *d_attack, const double *d_release, int ps_flags, double *d_dst, int64_t *d_ist, double *d_out,
                            void *stream);
int mxg_dyn_compress_host(size_t V, size_t N, const double *h_in, const double *h_ratio, const double *h_makeup, const double *h_threshold,
                          const double *h_attack, const double *h_release, int ps_flags, double *h_dst, int64_t *h_ist, double *h_out);
int mxg_envelope_trigger_host(size_t V, const int32_t *h_index, const double *h_amp, const int32_t *h_mask, const int32_t *h_count,
                              double *h_dst, int32_t *h_ist);
int mxg_envelope_line_render(size_t V, size_t N, size_t S, const double *d_segments, const int32_t *d_count, const double *d_trig,
                             const int32_t *d_trig_index, const double *d_trig_amp, double *d_dst, int32_t *d_ist, double *d_out,
                             void *stream);
int mxg_envelope_line_host(size_t V, size_t N, size_t S, const double *h_segments, const int32_t *h_count, const double *h_trig,
                           const int32_t *h_trig_index, const double *h_trig_amp, double *h_dst, int32_t *h_ist, double *h_out);
int mxg_lag_render(size_t V, size_t N, const double *d_in, const double *d_alpha, const double *d_alpha_reciprocal, int alpha_per_sample,
                   double *d_val, double *d_out, void *stream);
int mxg_lag_host(size_t V, size_t N, const double *h_in, const double *h_alpha, const double *h_alpha_reciprocal, int alpha_per_sample,
                 double *h_val, double *h_out);
int mxg_map_range_host(int mode, size_t V, const double *h_range, double *h_aux);
int mxg_map_render(int mode, size_t V, size_t N, const double *d_in, const double *d_range, const double *d_aux, double *d_out, void *stream);
int mxg_map_host(int mode, size_t V, size_t N, const double *h_in, const double *h_range, const double *h_aux, double *h_out);

/* ---- maxiPolyBLEP: the anti-aliased oscillator (K20) --------------------------------------------------------------------
 * V x maxiPolyBLEP::play(freq) (src/libs/maxiPolyBLEP.h over src/libs/PolyBLEP/PolyBLEP.cpp): per sample dt = freq / sample_rate,
 * the waveform's sample on the phase t -- or a sine where (freq / sample_rate) * sample_rate >= sample_rate / 4 -- then
 * t += dt; t -= (int64)t.  One waveform per launch, MXG_PBLEP_* in the reference's enum order.
 * d_freq [V] (fps = 0) or [N][V] (fps = 1); d_pw [V] the pulse widths, NULL: 0.5; d_t [V] the phases, in/out; d_out [N][V],
 * distinct from d_freq.  DOMAIN: finite frequencies with |freq / sample_rate| < 2^62, finite pulse widths, phases in (-1, 1)
 * (what sync and play leave); a negative frequency is inside.
 * The phase is BIT-EXACT.  TRIANGLE, SQUARE, RECTANGLE, SAWTOOTH, RAMP, MODIFIED_TRIANGLE, MODIFIED_SQUARE, TRIANGULAR_PULSE,
 * TRAPEZOID_FIXED and TRAPEZOID_VARIABLE are BIT-EXACT wherever the sine fallback is not taken; SINE, COSINE and a fallback
 * sample are within 1 ULP, the two rectified sines within 2^-50 absolute.
 * Refused with MXG_ERR_INVALID: V == 0 or N == 0, a waveform outside 0 .. 13, sample_rate <= 0, a null d_freq / d_t / d_out.
 * mxg_polyblep_host: the same arguments on HOST arrays, the same arithmetic on the CPU (no device needed). */
enum {
    MXG_PBLEP_SINE = 0, MXG_PBLEP_COSINE = 1, MXG_PBLEP_TRIANGLE = 2, MXG_PBLEP_SQUARE = 3, MXG_PBLEP_RECTANGLE = 4,
    MXG_PBLEP_SAWTOOTH = 5, MXG_PBLEP_RAMP = 6, MXG_PBLEP_MODIFIED_TRIANGLE = 7, MXG_PBLEP_MODIFIED_SQUARE = 8,
    MXG_PBLEP_HALF_WAVE_RECTIFIED_SINE = 9, MXG_PBLEP_FULL_WAVE_RECTIFIED_SINE = 10, MXG_PBLEP_TRIANGULAR_PULSE = 11,
    MXG_PBLEP_TRAPEZOID_FIXED = 12, MXG_PBLEP_TRAPEZOID_VARIABLE = 13
};
#define MXG_PBLEP_WAVEFORMS 14
int mxg_polyblep_render(int waveform, size_t V, size_t N, const double *d_freq, int fps, const double *d_pw, double sample_rate,
                        double *d_t, double *d_out, void *stream);
int mxg_polyblep_host(int waveform, size_t V, size_t N, const double *h_freq, int fps, const double *h_pw, double sample_rate,
                      double *h_t, double *h_out);

/* ---- maxiKick / maxiSnare / maxiHats and maxiClock: the fused drum voices (K21) ------------------------------------------
 * V x play() of one drum class (src/libs/maxiSynths.cpp:11-259), N samples: envOut = envelope.adsr(1., trigger), optionally
 * fabs(1 - envOut); the voice -- kick sinewave(pitch*envOut)*envOut, snare (triangle(pitch*(0.1+(envOut*0.85))) + noise())*envOut,
 * hats (sinebuf(pitch) + noise())*envOut --; optionally fastAtanDist(output, distortion); optionally the filter (kick / snare
 * lores(output, cutoff, resonance), hats maxiSVF::play(output, 0., 0., 1., 0.)); output*gain, optionally limited to exactly +-1.
 * One kind per launch; flags = MXG_DRUM_INVERSE | DISTORTION | FILTER | LIMITER (the members inverse, useDistortion, useFilter,
 * useLimiter), constant per call.  The sample rate is mxg_settings'.
 *   d_trig   doubles [N][V] (tpv = 1) or [N] (tpv = 0), what mxg_seq_render's d_trig and mxg_clock_render's d_tick hold: a
 *            non-zero entry means trigger() was called before that play().  NULL: never.
 *   d_rand   int32 [N][V], as for mxg_osc_noise: the rand() draw voice v's noise() takes at sample n.  Required for snare and
 *            hats; REFUSED (not ignored) for the kick, which draws nothing.
 *   d_pitch [V]; d_env_par [4][V] attack, decay, sustain, release as the setters store them (mxg_env_coeff_host), d_holdtime int64
 *            [V] (the constructors: attack 1 -- setAttack(0) --, holdtime 1); d_shape [V] the member distortion (NULL unless
 *            DISTORTION); d_gain [V] (NULL: 1).
 *   d_coef   kick / snare: [3][V] as mxg_filter_coeffs_host(MXG_FLT_LORES, ...) writes it (rows c, r are read); hats: [5][V] as
 *            mxg_svf_coeffs_host writes it (the hats' filter.setCutoff / setResonance; the constructor: 8000, 1).  NULL only
 *            without FILTER.
 *   State, in / out, plain arrays; a fresh object is all zeros (mxg_memset):
 *     d_phase [V]      kick.phase / tone.phase
 *     d_dst   [2][V]   envelope.amplitude, envelope.output           } mxg_env_render's layout
 *     d_ist   [6][V]   int64: holdcount, attackphase, decayphase, sustainphase, holdphase, releasephase
 *     d_fst   [3][V]   kick / snare: filter.x, filter.y, (unused); hats: filter.v0z, v1, v2
 *   d_out [N][V], distinct from d_trig and d_rand.
 * DOMAIN: finite parameters; the hats' pitch in [0, sample rate) and its phase in [-1, 511), as maxiOsc::sinebuf's table read needs.
 * Snare, hats and every state row but the kick's filter state are BIT-EXACT (host coefficients); the kick's output carries its
 * sine's <= 1 ULP through the later stages.
 * Refused with MXG_ERR_INVALID: V == 0 or N == 0, an unknown kind or flag, a missing required pointer, d_rand given for the kick,
 * d_out overlapping d_trig or d_rand.
 * mxg_drum_host: the same arguments on HOST arrays, the same arithmetic on the CPU (no device needed). */
enum { MXG_DRUM_KICK = 0, MXG_DRUM_SNARE = 1, MXG_DRUM_HATS = 2 };
#define MXG_DRUM_KINDS 3
#define MXG_DRUM_INVERSE 1
#define MXG_DRUM_DISTORTION 2
#define MXG_DRUM_FILTER 4
#define MXG_DRUM_LIMITER 8
int mxg_drum_render(int kind, int flags, size_t V, size_t N, const double *d_trig, int tpv, const int32_t *d_rand,
                    const double *d_pitch, const double *d_env_par, const int64_t *d_holdtime, const double *d_shape,
                    const double *d_coef, const double *d_gain, double *d_phase, double *d_dst, int64_t *d_ist, double *d_fst,
                    double *d_out, void *stream);
int mxg_drum_host(int kind, int flags, size_t V, size_t N, const double *h_trig, int tpv, const int32_t *h_rand,
                  const double *h_pitch, const double *h_env_par, const int64_t *h_holdtime, const double *h_shape,
                  const double *h_coef, const double *h_gain, double *h_phase, double *h_dst, int64_t *h_ist, double *h_fst,
                  double *h_out);
/* V x maxiClock::ticker() (src/libs/maxiClock.cpp:16-28), N samples: currentCount = floor(timer.phasor(bps)); a sample ticks where
 * lastCount != currentCount, and playHead counts the ticks.  ticker() never writes lastCount, so with lastCount 0 a tick is the one
 * sample per wrap on which the phasor returns a phase >= 1.  d_bps [V] (setTempo: (bpm / 60.) * ticks); d_clk [V] timer.phase,
 * in / out; d_lastcount int32 [V], read only (NULL: 0); d_playhead int64 [V], in / out; d_count int32 [V], out: currentCount after
 * the block; d_tick [N][V] doubles 1.0 / 0.0, which feeds mxg_drum_render's d_trig directly.  Bit-exact.
 * Refused with MXG_ERR_INVALID: V == 0 or N == 0, a null d_bps / d_clk / d_playhead / d_count / d_tick, d_tick overlapping any of
 * the other arrays (all arrays are distinct). */
int mxg_clock_render(size_t V, size_t N, const double *d_bps, double *d_clk, const int32_t *d_lastcount, int64_t *d_playhead,
                     int32_t *d_count, double *d_tick, void *stream);
int mxg_clock_host(size_t V, size_t N, const double *h_bps, double *h_clk, const int32_t *h_lastcount, int64_t *h_playhead,
                   int32_t *h_count, double *h_tick);

/* ---- maxiAtoms: Gabor atom banks, the atom queue and the book player (K22) ------------------------------------------------
 * S independent streams, each one maxiAccelerator (src/libs/maxiAtoms.cpp:93-126) with, optionally, one maxiAtomBook and its
 * maxiAtomBookPlayer (:198-219).  A bank owns per stream sampleIdx, atomIdx and a live list of at most Q queued atoms in queue order;
 * a queued atom is GABOR (createGabor's parameters, :27-89, synthesised on the device from a float window table per distinct length)
 * or RAW (floats of the bank's raw pool: what addAtom(flArr&) queues).
 *   mxg_atoms_bank_create  h_book_start int64 [S + 1], rising from 0: stream s owns book atoms [start[s], start[s + 1]) (NULL: no
 *                          books); h_book float [5][A] rows position, length, amp, frequency, phase as maxiGaborAtom holds them
 *                          (A = start[S]); h_num_samples uint32 [S], the books' numSamples (>= 1); h_raw / raw_len the raw pool
 *                          (may be empty; mxg_atoms_raw_append adds to it later and returns the offset).  All HOST arrays, copied.
 *   mxg_atoms_add          n instances in order, HOST arrays: h_stream int32 [n]; h_kind [n] MXG_ATOM_GABOR / MXG_ATOM_RAW; h_length
 *                          uint32 [n] the atom's size; h_offset uint32 [n] addAtom's offset (NULL: 0): startTime = sampleIdx + offset;
 *                          h_par float [n][4] freq, sampleRate, startPhase, amp of createGabor (read for GABOR); h_raw_off uint32 [n]
 *                          where a RAW atom's floats start in the pool.  Synchronises the device.  More than Q queued in a stream:
 *                          MXG_ERR_INVALID and NOTHING is added.
 *   mxg_atoms_fill         fillNextBuffer(buffer, N) on every stream: d_out float32 [S][N], each stream's buffer contiguous.
 *                          accumulate != 0: the sum starts from what d_out holds (the reference's +=); 0: from zero.
 *   mxg_atoms_play         maxiAtomBookPlayer::play(book, stream, ., N) and then the fill, in one call.  The player's offset is
 *                          |looped - position| (the one deliberate departure).  A live list that would
 *                          pass Q is reported through the asynchronous error word (mxg_last_async_error: MXG_ERR_INVALID) by the
 *                          next call; that stream's block and state are left untouched, the other streams are rendered.
 *   onset                  MXG_ATOM_ONSET_BLOCK: the reference's -- a due atom starts at buffer[0] of the block in which it falls
 *                          due.  MXG_ATOM_ONSET_SAMPLE (an extension): it starts on its own sample, startTime - sampleIdx.
 *   mxg_atoms_state        synchronises and copies out (any pointer may be NULL): sampleIdx int64 [S], atomIdx uint32 [S], the live
 *                          counts int32 [S], and per live entry startTime int64 / pos uint32 / size uint32, each [S][Q].
 *   mxg_atoms_gabor_host   createGabor on the host: length floats.
 * RAW atoms are BIT-EXACT in either onset mode: a float sum in queue order.  GABOR atoms: every operation but the sine is the
 * reference's; the sine is the correctly reduced double sine rounded to float, within 1 float ULP of glibc's sinf (DESIGN.md
 * section 4), and the device result is bit-identical to the _host twin's.
 * DOMAIN: Gabor lengths in [1, 22 050) (the reference's window cache); finite parameters; |maxPhase| + |startPhase| <= 2^19 rad;
 * N <= 2^24; sample indices below 2^31 (the reference narrows startTime + pos to int).
 * The _host twins: the same calls on a bank made by mxg_atoms_bank_create_host, whose arrays -- and h_out -- are host memory; the
 * same functions (csrc/mxg_atoms.h) on the CPU, no device needed.  mxg_atoms_play_host returns the overflow itself.
 * mxg_atoms_bank_destroy, mxg_atoms_raw_append and mxg_atoms_state take both kinds of bank. */
#define MXG_ATOM_GABOR 0
#define MXG_ATOM_RAW 1
#define MXG_ATOM_KINDS 2
#define MXG_ATOM_ONSET_BLOCK 0
#define MXG_ATOM_ONSET_SAMPLE 1
#define MXG_ATOMS_PIECE 64 /* segments of a stream's block staged through LDS at a time (K22b) */
typedef struct mxg_atoms_bank mxg_atoms_bank;
mxg_atoms_bank *mxg_atoms_bank_create(size_t S, size_t Q, const int64_t *h_book_start, const float *h_book,
                                      const uint32_t *h_num_samples, const float *h_raw, size_t raw_len);
mxg_atoms_bank *mxg_atoms_bank_create_host(size_t S, size_t Q, const int64_t *h_book_start, const float *h_book,
                                           const uint32_t *h_num_samples, const float *h_raw, size_t raw_len);
int mxg_atoms_bank_destroy(mxg_atoms_bank *b);
int mxg_atoms_raw_append(mxg_atoms_bank *b, const float *h_raw, size_t n, uint32_t *offset);
int mxg_atoms_add(mxg_atoms_bank *b, size_t n, const int32_t *h_stream, const int32_t *h_kind, const uint32_t *h_length,
                  const uint32_t *h_offset, const float *h_par, const uint32_t *h_raw_off);
int mxg_atoms_add_host(mxg_atoms_bank *b, size_t n, const int32_t *h_stream, const int32_t *h_kind, const uint32_t *h_length,
                       const uint32_t *h_offset, const float *h_par, const uint32_t *h_raw_off);
int mxg_atoms_fill(mxg_atoms_bank *b, size_t N, float *d_out, int onset, int accumulate, void *stream);
int mxg_atoms_play(mxg_atoms_bank *b, size_t N, float *d_out, int onset, int accumulate, void *stream);
int mxg_atoms_fill_host(mxg_atoms_bank *b, size_t N, float *h_out, int onset, int accumulate);
int mxg_atoms_play_host(mxg_atoms_bank *b, size_t N, float *h_out, int onset, int accumulate);
int mxg_atoms_state(mxg_atoms_bank *b, int64_t *h_sample_idx, uint32_t *h_atom_idx, int32_t *h_nlive, int64_t *h_start,
                    uint32_t *h_pos, uint32_t *h_size);
int mxg_atoms_gabor_host(float freq, float sample_rate, uint32_t length, float start_phase, float amp, float *h_atom);

/* ---- maxiSample play family -------------------------------------------------------------- */
typedef enum {
    MXG_SMP_PLAY = 0,                    /* play()                       C:740-747   */
    MXG_SMP_PLAYONCE = 1,                /* playOnce()                   C:982-991   */
    MXG_SMP_PLAYLOOP = 2,                /* playLoop(start,end)          C:960-967   */
    MXG_SMP_PLAYUNTIL = 3,               /* playUntil(end)               C:969-978   */
    MXG_SMP_PLAYATSPEED = 4,             /* playAtSpeed(a)               C:1060-1075 */
    MXG_SMP_PLAYONCEATSPEED = 5,         /* playOnceAtSpeed(a)           C:994-1003  */
    MXG_SMP_PLAYUNTILATSPEED = 6,        /* playUntilAtSpeed(end,a)      C:1047-1058 */
    MXG_SMP_PLAY4 = 7,                   /* play4(a=frequency,start,end) C:884-956   */
    MXG_SMP_PLAYATSPEEDBETWEENPOINTS = 8,/* playAtSpeedBetweenPoints(a=frequency,start,end) C:823-880 */
    /* trigger-driven players, mxg_sample_render_trig only */
    MXG_SMP_PLAYONZX = 9,                /* playOnZX(trig)                                  C:1006-1011 */
    MXG_SMP_PLAYONZXATSPEED = 10,        /* playOnZXAtSpeed(trig, a)                        C:1013-1018 */
    MXG_SMP_PLAYONZXATSPEEDFROMOFFSET = 11, /* playOnZXAtSpeedFromOffset(trig, a, p0=offset) C:1020-1026 */
    MXG_SMP_PLAYONZXATSPEEDBETWEENPOINTS = 12, /* ...BetweenPoints(trig, a, p0=offset, p1=length) C:1028-1035 */
    MXG_SMP_LOOPSETPOSONZX = 13,         /* loopSetPosOnZX(trig, p0=pos)                    C:1037-1042 */
    MXG_SMP_PLAYWITHPHASOR = 14          /* playWithPhasor(trig=pha)                        C:753-816   */
} mxg_sample_mode;
/* Upload a mono sample (what maxiSample::setSample holds, H:670-678) into a device buffer that
 * is valid on [-4, len+5] with 0.0 guards: the reference reads amplitudes[len], [len+1]
 * (C:1063-1064) and [-1] (C:898) out of bounds; zero is the parity convention.  The
 * wider margin backs the players' index clamp: where the reference itself indexes outside its
 * vector (undefined: a play4 step longer than its loop, playLoop with end > 1, a head uploaded far
 * outside the sample) the device reads a guard zero, never memory outside this allocation.
 * Returns the device pointer to element 0 (NULL on failure); release with mxg_sample_free. */
double *mxg_sample_upload(const double *h_samples, size_t len);
int mxg_sample_free(double *d_samples);
/* V play heads over one shared sample.  d_a: speed or frequency, [V] (aps=0) or [N][V] (aps=1);
 * d_start/d_end [V] (fractions of the length for playLoop/playUntil*, sample indices for
 * play4/playAtSpeedBetweenPoints, exactly as in the reference); d_position [V] in/out is the
 * member `position` (setSample leaves it at len-1, H:677; trigger() sets 0, C:597-600).
 * mySampleRate is the int member (44100 after setSample): the step divides by the INTEGER
 * quotient sampleRate/mySampleRate (C:1070). */
int mxg_sample_render(int mode, size_t V, size_t N, const double *d_samples, size_t len,
                      int mySampleRate, const double *d_a, int aps, const double *d_start,
                      const double *d_end, double *d_position, double *d_out, void *stream);

/* ---- maxiLooperBank: writable sample slots, maxiSample::loopRecord / normalise on the device (K25) ---------- */
/* A pool of R slots of up to cap samples, zero-filled.  Slot r starts at p + r * (*stride) and is guarded with zeros on
 * [-4, cap + 5] exactly as mxg_sample_upload guards its buffer, so p + r * stride with the slot's length is an ordinary sample
 * pointer for mxg_sample_render*, mxg_sampler_render and the grain banks.  Returns NULL on failure; release with
 * mxg_sample_pool_free.  mxg_sample_pool_stride(cap) is the stride such a pool has (for host arrays in the same layout). */
double *mxg_sample_pool_alloc(size_t R, size_t cap, size_t *stride);
int mxg_sample_pool_free(double *d_pool);
size_t mxg_sample_pool_stride(size_t cap);
/* The slots' lengths (amplitudes.size() per slot; slots of different lengths share a pool): refuses len[r] == 0 and
 * len[r] > cap by name, then copies h_len [R] to d_len [R].  The render calls below take d_len; a length beyond cap that reaches
 * them another way is read as cap, never indexed. */
int mxg_sample_pool_lengths(size_t R, size_t cap, const uint64_t *h_len, uint64_t *d_len);
#define MXG_LOOPER_PLAY_NONE (-1)
/* N calls of loopRecord(in, enable, mix, start, end) (H:706-721) on every slot, each followed -- as a patch calls them -- by one
 * call of play() (play_mode MXG_SMP_PLAY) or playLoop(pstart, pend) (MXG_SMP_PLAYLOOP) on the same slot, or by nothing
 * (MXG_LOOPER_PLAY_NONE: d_out must be NULL).  d_in, d_out [N][R]; d_enable doubles, [R] (eps = 0) or [N][R] (eps = 1), non-zero =
 * true as C++ converts a double to bool; d_mix, d_start, d_end, d_pstart, d_pend [R]; d_recpos (recordPosition), d_lagval (the
 * enable lag's val, alpha 0.5) and d_position [R] in / out: trigger() zeroes recpos and position, setSample leaves position at
 * len - 1.  Bit-exact, and independent of how the samples are split into calls (the library itself cuts a call into launches of
 * mxg_looprec_piece() samples; a workgroup owns mxg_looprec_tile() slots).  The play head sees what this sample and earlier ones
 * recorded.  The one departure: where the record index falls outside [0, len[r]) -- start or end outside [0, 1], start == 1,
 * NaN, an uploaded recpos out of range; the reference indexes outside its vector -- the read gives 0, nothing is stored, and
 * d_dropped[r] (uint32 [R], may be NULL) counts the sample.  Inside 0 <= start < 1, 0 <= end <= 1 it stays as it was.
 * 1 <= N <= 2^24. */
int mxg_looprec_render(size_t R, size_t N, double *d_pool, size_t stride, size_t cap, const uint64_t *d_len, const double *d_in,
                       const double *d_enable, int eps, const double *d_mix, const double *d_start, const double *d_end, double *d_recpos,
                       double *d_lagval, int play_mode, const double *d_pstart, const double *d_pend, double *d_position, double *d_out,
                       uint32_t *d_dropped, void *stream);
int mxg_looprec_piece(void);
int mxg_looprec_tile(void);
/* maxiSample::normalise(maxLevel[r]) (C:1126-1137) on every slot: scale = (float)(maxLevel / max|a|), a = round(scale * a); an
 * all-zero slot becomes NaN, as in the reference.  R <= 65535. */
int mxg_sample_pool_normalise(size_t R, double *d_pool, size_t stride, size_t cap, const uint64_t *d_len, const double *d_maxLevel,
                              void *stream);
/* The same functions (csrc/mxg_looper.h) on host arrays in the pool's layout (h_pool = element 0 of slot 0, with its guards around
 * every slot); these two also refuse a bad h_len by name.  No device is touched. */
int mxg_looprec_host(size_t R, size_t N, double *h_pool, size_t stride, size_t cap, const uint64_t *h_len, const double *h_in,
                     const double *h_enable, int eps, const double *h_mix, const double *h_start, const double *h_end, double *h_recpos,
                     double *h_lagval, int play_mode, const double *h_pstart, const double *h_pend, double *h_position, double *h_out,
                     uint32_t *h_dropped);
int mxg_sample_pool_normalise_host(size_t R, double *h_pool, size_t stride, size_t cap, const uint64_t *h_len, const double *h_maxLevel);

/* maxiSample::playAtSpeedBetweenPointsFromPos(frequency, start, end, pos) (C:826-880) with the CALLER's position signal
 * d_pos [N][V]: the member `position` takes no part (it is the by-value parameter of C:823-825), so the call is a pure
 * function of its arguments.  d_freq [V] (fps = 0) or [N][V]; d_start / d_end [V] in samples.  Bit-exact. */
int mxg_sample_render_frompos(size_t V, size_t N, const double *d_samples, size_t len, const double *d_freq, int fps,
                              const double *d_start, const double *d_end, const double *d_pos, double *d_out, void *stream);

/* Trigger-driven players (modes 9-14).  d_trig is the per-sample [N][V] first argument of the
 * reference call: the trigger signal of playOnZX* / loopSetPosOnZX, or the phasor of
 * playWithPhasor.  d_a = speed ([V], or [N][V] when aps), d_p0/d_p1 = per-voice offset/length (or
 * pos), as listed in mxg_sample_mode.  State, in/out: d_position [V]; d_tprev [V] / d_tfirst [V] =
 * maxiSample::zxTrig's previousValue / firstTrigger (H:593-594: a fresh object holds 1.0 / 1), or
 * for mode 14 phasorPrev / phasorFirst (H:731-732: 0.0 / 1; d_position is not used and may be NULL).
 * All of it is compares, + - * / round and integer indexing => bit-exact. */
int mxg_sample_render_trig(int mode, size_t V, size_t N, const double *d_samples, size_t len,
                           int mySampleRate, const double *d_trig, const double *d_a, int aps,
                           const double *d_p0, const double *d_p1, double *d_position,
                           double *d_tprev, int32_t *d_tfirst, double *d_out, void *stream);

/* int32 <-> int64 copies of a device array (hosts that carry every integer member of a slot as int64 -- include/maximilian.h --
 * feed the int32 flag arrays above through these). */
int mxg_i64_from_i32(int64_t *d_dst, const int32_t *d_src, size_t n, void *stream);
int mxg_i32_from_i64(int32_t *d_dst, const int64_t *d_src, size_t n, void *stream);

/* maxiSample::load(fileName, channel) / read() (C:605-692): parse a 16-bit PCM RIFF/WAVE file the way the
 * reference walks it, upload the payload as int16 and de-interleave + normalise on the device
 * (amplitudes[i] = short/32767.0, C:679, bit-exact).  Returns the device sample buffer (guarded like
 * mxg_sample_upload, free with mxg_sample_free) or NULL (cannot open / malformed; the reference returns
 * false / reads garbage).  *h_len = amplitudes.size() = dataSize/2 -- for a multi-channel file that is the
 * FULL interleaved length: the reference keeps every (2*channels)-th short at the front and leaves the rest
 * (C:667-674, see wav.hip).  After read() the member `position` equals the size (C:681): start the bank's
 * play heads there.  h_hdr (int32[8], may be NULL) receives ChunkSize, SubChunk1Size, Format, Channels,
 * SampleRate, ByteRate, BlockAlign, BitsPerSample (set the bank's mySampleRate from [4]). */
double *mxg_sample_load_wav(const char *path, int channel, size_t *h_len, int32_t *h_hdr);
/* maxiSample::save(filename) (C:698-725): shorts = static_cast<short>(round(a*32767.0)) computed on the
 * device, written behind the 44-byte header built from h_hdr (same 8 fields).  Synchronous. */
int mxg_sample_save_wav(const char *path, const double *d_samples, size_t len, const int32_t *h_hdr,
                        void *stream);

/* ---- maxiSampler banks (L/maxiSynths.h:137-187, maxiSynths.cpp:262-300) ---------------------------------- */
/* V = NS * voices slots (any voices in 1 .. 32, as maxiSampler::setNumVoices accepts: maxiSynths.cpp:284-289), all over one sample
 * buffer (mxg_sample_upload / mxg_sample_load_wav).  Renders N calls of maxiSampler::play() for every
 * sampler: per slot envOut = adsr(gain, trigger); if (envOut > 0) { outputs = play4(freq, 0, len)*envOut;
 * output += outputs/voices; if (trigger == 1 && !sustain) trigger = 0; }.  d_mix [N][NS] = play();
 * d_outputs (optional) [N][V] = the member outputs[i] after each call.  d_freq [V] from
 * mxg_sampler_freq_host (pitchRatios[(int)pitch + 67] * ((1./len)*sampleRate), maxiSynths.cpp:297).
 * Slot state, in/out: d_position [V], d_trigger [V] (envelopes[i].trigger), d_outhold [V] (outputs[i]),
 * d_dst [2][V] / d_ist [6][V] as mxg_env_render; d_gain [V] = envOutGain, d_par [4][V] + d_holdtime [V] the
 * envelope parameters.  The control calls (trigger(), midiNoteOn/Off, setPitch: maxiSynths.cpp:351-391,
 * 484-491) edit that state between renders on the host.  Bit-exact, including the in-order sum. */
int mxg_sampler_freq_host(size_t V, const double *h_pitch, size_t len, double *h_freq);
int mxg_sampler_render(size_t V, size_t N, int voices, int sustain, const double *d_samples, size_t len,
                       const double *d_freq, const double *d_gain, const double *d_par,
                       const int64_t *d_holdtime, double *d_position, int32_t *d_trigger, double *d_outhold,
                       double *d_dst, int64_t *d_ist, double *d_mix, double *d_outputs, void *stream);

/* ---- maxiFFT batch ---------------------------------------------------------------------- */
/* A plan is what maxiFFT::setup(fftSize, hopSize, windowSize) prepares (L/maxiFFT.cpp:45-60): the
 * Hann window (fft::genWindow type 3, L/fft.cpp:409-413) and the fp32 twiddle sequences the
 * reference generates by recurrence (L/fft.cpp:161-182, :245-272), replayed on the host.
 * fftSize: power of two in [8, 8192] (the reference exit(1)s otherwise, L/fft.cpp:129-132 ->
 * here NULL + MXG_ERR_INVALID); windowSize < fftSize is raised to fftSize as in the reference;
 * windowSize > fftSize overruns the reference's buffers and is rejected. */
typedef struct mxg_fft_plan mxg_fft_plan;
mxg_fft_plan *mxg_fft_plan_create(int fftSize, int hopSize, int windowSize);
int mxg_fft_plan_destroy(mxg_fft_plan *plan);
int mxg_fft_plan_bins(const mxg_fft_plan *plan); /* getNumBins() = fftSize/2 */
/* Transform nframes frames; frame k = d_signal[k*frame_stride .. k*frame_stride + fftSize).
 * With frame_stride = hopSize over a signal prefixed by (windowSize-hopSize) zeros this is exactly
 * the sequence of frames maxiFFT::process() analyses (L/maxiFFT.cpp:65-91).  Outputs are
 * [nframes][bins] fp32, any of them may be NULL: real/imag = getReal()/getImag() (bin 0 packs
 * DC and Nyquist, L/fft.cpp:274-275), mags/phases = getMagnitudes()/getPhases() (cartToPol,
 * L/fft.cpp:507-515).  real, imag and mags are bit-exact; phases use the device atan2f. */
int mxg_fft_batch(const mxg_fft_plan *plan, const float *d_signal, size_t frame_stride,
                  size_t nframes, float *d_real, float *d_imag, float *d_mags, float *d_phases,
                  void *stream);

/* maxiFFT::magsToDB (fft::convToDB, L/fft.cpp:526-534), spectralFlatness and spectralCentroid
 * (L/maxiFFT.cpp:113-132) of nframes frames of magnitudes d_mags [nframes][bins] (e.g. the d_mags
 * output of mxg_fft_batch).  Outputs, any may be NULL: d_db [nframes][bins], d_flatness [nframes],
 * d_centroid [nframes] (uses maxiSettings::sampleRate).  The per-frame sums run over the bins in the
 * reference's order in float; centroid is bit-exact, dB and flatness go through the device
 * log10f/logf/expf (tolerances in DESIGN.md). */
int mxg_fft_features(const mxg_fft_plan *plan, const float *d_mags, size_t nframes, float *d_db,
                     float *d_flatness, float *d_centroid, void *stream);

/* ---- maxiIFFT batch (L/maxiFFT.cpp:140-192, SPECTRUM mode) ---------------------------------------- */
/* maxiIFFT::setup(fftSize, hopSize, windowSize): Hann window over (windowSize ? windowSize : fftSize),
 * zero beyond (note: not maxiFFT's max(windowSize, fftSize)).  fftSize: power of two in [8, 8192]. */
typedef struct mxg_ifft_plan mxg_ifft_plan;
mxg_ifft_plan *mxg_ifft_plan_create(int fftSize, int hopSize, int windowSize);
int mxg_ifft_plan_destroy(mxg_ifft_plan *plan);
/* nframes spectra d_mags/d_phases [nframes][bins] -> d_signal [nframes*hopSize]: the samples
 * maxiIFFT::process(mags, phases) returns when it is called hopSize times per spectrum (the spectrum is
 * consumed at pos == 0, L/maxiFFT.cpp:156).  Per frame: polToCart (L/fft.cpp:590-604), a full fftSize-point
 * complex inverse FFT with the reference's fp32 recurrence twiddles, /fftSize, x window (:606-611), then
 * the overlap-add hop buffer (:176-183) evaluated in the reference's order of additions.  d_buffer
 * ([fftSize], in/out, may be NULL = a fresh object) is the member `buffer`, so consecutive calls continue
 * one stream.  d_ifft_out (optional [nframes][fftSize]) receives each frame's windowed inverse transform
 * (`ifftOut`).  Bit-exact given the same cartesian inputs; the float cos/sin of polToCart are the
 * device's => tolerance.  COMPLEX mode of the reference copies its inputs into the wrong
 * arrays (L/fft.cpp:613-619: out_real/out_img, which calcIFFT then overwrites) and is not provided. */
int mxg_ifft_batch(const mxg_ifft_plan *plan, const float *d_mags, const float *d_phases, size_t nframes,
                   float *d_buffer, float *d_signal, float *d_ifft_out, void *stream);

/* maxiIFFT::process(real, imag, COMPLEX) (L/maxiFFT.cpp:155-192 with fftModes COMPLEX).  The reference's
 * fft::inverseFFTComplex (L/fft.cpp:613-619) copies its inputs into out_real/out_img -- the arrays calcIFFT then overwrites
 * with the inverse transform of in_real/in_img, which COMPLEX mode never writes.  On a fresh object those are the zeros
 * of fft::setup, so every frame's inverse transform is exactly 0 and the call returns the carried hop buffer running
 * out: as_reference = 1 reproduces that, bit for bit.  as_reference = 0 is what the function was written to do: real/imag
 * [nframes][bins] go to the transform's inputs (negative frequencies zero, like polToCart), everything after -- the
 * full-size inverse FFT with replayed twiddles, /fftSize, window, overlap-add -- exactly as mxg_ifft_batch; bit-exact
 * against the reference's own calcIFFT fed that way (tests/test_gpu_convolve.py). */
int mxg_ifft_batch_complex(const mxg_ifft_plan *plan, const float *d_real, const float *d_imag, size_t nframes,
                           int as_reference, float *d_buffer, float *d_signal, float *d_ifft_out, void *stream);

/* ---- maxiConvolve (L/maxiConvolve.cpp:13-107): partitioned convolution over a frequency delay line ------------------ */
/* maxiConvolve::setup(impulseFile, fftsize, hopsize) with the impulse already in memory: h_amplitudes [len] = the
 * loaded maxiSample's amplitudes, position0 = its play head (load()/read() leave it at len, C:681).  Replicated: the
 * impulse is played with play() (C:740-747; the first read is amplitudes[len], one past the end = 0 here) len times
 * into maxiFFT::setup(fftsize, fftsize, hopsize) -- hop = fftsize, full Hann window: non-overlapping frames (:35-40);
 * then getNumBins() - len % getNumBins() zeros (:41-45, which may or may not complete a last frame); the frames'
 * real / imaginary spectra are divided by the largest positive real / imaginary value (:47-52, float division).
 * The analysis runs on the device (mxg_fft_batch, bit-exact); NULL on failure. */
typedef struct mxg_convolve mxg_convolve;
mxg_convolve *mxg_convolve_create(const double *h_amplitudes, size_t len, double position0, int fftsize, int hopsize);
int mxg_convolve_destroy(mxg_convolve *c);
int mxg_convolve_frames(const mxg_convolve *c);  /* impulseReal.size() */
/* the normalised impulse spectra [frames][bins]; either pointer may be NULL */
int mxg_convolve_impulse(const mxg_convolve *c, float *h_real, float *h_imag);
/* play(w) (:76-107) for nblocks*fftsize consecutive samples d_in -> d_out (float, device).  The delay line, the current
 * sums and maxiIFFT's buffer are the object's state and carry from call to call.  Per fftsize samples: the input frame's
 * spectrum enters the delay line; sumReal/sumImag = sum over k of impulse[k] (x) FDL[k] accumulated in float in k order
 * (bin 0: real*real and imag*imag only, :86-87); block b of the output is the maxiIFFT (COMPLEX mode,
 * setup(fftsize, fftsize, hopsize)) of the sums formed at the end of block b-1.
 * mode 0 = as the reference computes (the COMPLEX-mode defect above: silence, while the state still advances);
 * mode 1 = as intended (the sums reach the inverse transform).  Both bit-exact against the reference (tests/test_gpu_convolve.py). */
int mxg_convolve_play(mxg_convolve *c, const float *d_in, size_t nblocks, float *d_out, int mode, void *stream);
int mxg_convolve_reset(mxg_convolve *c);
/* The two halves of one block of play(), for a host that is called once per sample (include/maxiConvolve.h): the output of the
 * NEXT fftsize samples depends only on the sums the previous input frame left, so it can be fetched before those samples'
 * inputs exist; mxg_convolve_input then takes the fftsize inputs (delay line, sums).  output + input == play(nblocks = 1). */
int mxg_convolve_output(mxg_convolve *c, float *d_out, int mode, void *stream);
int mxg_convolve_input(mxg_convolve *c, const float *d_in, void *stream);

/* ---- maxiConvolveBank: V independent maxiConvolve objects over I shared impulses (kernel K24) ------------ */
/* Stream v is, bit for bit, an mxg_convolve created from impulse h_imp_of[v] and fed stream v's input -- outputs and carried
 * state, for any split of the samples into calls and for both modes.  h_amps [I] = pointers to the impulses' amplitudes, h_lens [I]
 * their lengths, h_pos0 [I] their play heads (each as mxg_convolve_create takes one; 1 <= I <= V), h_imp_of [V] the impulse of each
 * stream; one fftsize / hopsize for the bank.  Every impulse is analysed exactly as mxg_convolve_create analyses it (the play-head
 * walk, the zero padding, the division by the largest positive real / imaginary value, a zero maximum included); the frame counts
 * K_i may differ and may be 0, and a stream's sum runs over k < K_i exactly (no zero frames stand in: 0 x Inf would differ).
 * Bad arguments are refused, with a message that names the argument, before any device call.
 * State per stream: its input spectra in a ring of max K_i - 1 + 16 rows -- the new rows enter it inside the multiply-accumulate
 * kernel, so keeping the history costs nblocks rows of writes per call and no copies -- and the pending sums, from which output
 * block 0 of the next call is transformed.  maxiIFFT's hop buffer is NOT state of the bank: maxiConvolve sets its maxiIFFT up with
 * hop = fftsize, so a frame never reaches into the next one and the buffer is never read back. */
typedef struct mxg_convolve_bank mxg_convolve_bank;
mxg_convolve_bank *mxg_convolve_bank_create(size_t V, size_t I, const double *const *h_amps, const size_t *h_lens, const double *h_pos0,
                                            const int *h_imp_of, int fftsize, int hopsize);
int mxg_convolve_bank_destroy(mxg_convolve_bank *b);
int mxg_convolve_bank_reset(mxg_convolve_bank *b);
int mxg_convolve_bank_frames(const mxg_convolve_bank *b, size_t i); /* K_i */
/* the normalised spectra of impulse i, [K_i][bins]; either pointer may be NULL */
int mxg_convolve_bank_impulse(const mxg_convolve_bank *b, size_t i, float *h_real, float *h_imag);
/* play(w) for nblocks * fftsize consecutive samples of every stream: d_in, d_out float [V][nblocks * fftsize] (device); mode as
 * mxg_convolve_play.  One forward batch over all V * nblocks frames, the multiply-accumulate kernel (one launch per 16 blocks, each
 * followed by a one-lane launch that advances the ring's head on the device), one inverse batch: the number of launches does not
 * depend on V. */
int mxg_convolve_bank_play(mxg_convolve_bank *b, const float *d_in, size_t nblocks, float *d_out, int mode, void *stream);
/* the same call on the layout the other banks speak: doubles [N][V], N = nblocks * fftsize.  The input is narrowed with a plain
 * (float) cast, as play(float w) narrows a double argument; the output is widened exactly. */
int mxg_convolve_bank_play_nv(mxg_convolve_bank *b, const double *d_in, size_t nblocks, double *d_out, int mode, void *stream);
/* The multiply-accumulate of a call on host arrays, no device needed: the text of the kernel's lanes (csrc/mxg_convolve.h) run in
 * the chunks, tiles and lanes of the launches.  h_K [V] = frames of each stream's impulse, h_imp_row [V] = its first row in
 * h_impR / h_impI [rows][bins]; h_ringR / h_ringI [V][R][bins] and *h_head (the slot the next frame takes; R >= max K, R >= 1) and
 * h_pendR / h_pendI [V][bins] are the state, in / out; h_XR / h_XI [V][nblocks][bins] = the spectra of the new frames;
 * h_SR / h_SI [V][nblocks][bins] receive the rows the inverse transform takes: row 0 = the pending sums on entry, row b = the sums
 * of frame b - 1.  A lane owns 2 bins of 4 consecutive frames; a launch covers at most R - max(max K, 1) + 1 frames. */
int mxg_convolve_bank_mac_host(size_t V, int bins, int R, const int *h_K, const int *h_imp_row, const float *h_impR, const float *h_impI,
                               float *h_ringR, float *h_ringI, int *h_head, float *h_pendR, float *h_pendI, const float *h_XR,
                               const float *h_XI, size_t nblocks, float *h_SR, float *h_SI);

/* ---- maxiFFTBank / maxiIFFTBank: V streaming analysers / resynthesisers over the banks' blocks (kernel K29) ---- */
/* maxiFFTBank(V) is V maxiFFT objects after setup(fftSize, hopSize, windowSize) (L/maxiFFT.cpp:45-60) fed in lock-step through
 * process(float value) (:65-91).  A call takes d_in, double [N][V] (device) for any N >= 0; sample (n, v) enters stream v as
 * (float)d_in[n][v], the conversion process(float) applies to a double argument.  State per stream: its last fftSize - hopSize
 * floats (zeros after setup, :51) and the samples taken since the last frame, on the device; `fill` = pos - (windowSize - hopSize),
 * 0 <= fill < hopSize, one counter for the bank, on the host (it depends only on the sequence of N values).
 * A call emits F = (fill + N) / hopSize frames per stream: frame f of stream v is the buffer the reference transforms at its
 * f-th `pos == windowSize` (:69) inside the call.  Outputs: real, imag, mags, phases, each fp32 [V * F][bins] (device), any of
 * them NULL but not all -- the bits of mxg_fft_batch on that stream alone.  layout 0 = frame-major, row = f * V + v (concatenates
 * across calls; what mxg_fft_features / mxg_mfcc_batch take); 1 = stream-major, row = v * F + f (what mxg_octave_batch takes).
 * Two launches per call whatever V and N (gather, frames); no host round trip.  NOT capturable into a hipGraph, nor is
 * mxg_ifft_bank_process: `fill` / `pos` and which of the two carry images is read advance on the host when a call is enqueued,
 * so a replayed graph would read the image and the counter of the call it was captured from.  Bad arguments are refused, with a message that
 * names the argument, before any device call: V = 0, an fftSize mxg_fft_plan_create refuses, windowSize above fftSize, hopSize
 * outside [1, fftSize], null pointers. */
typedef struct mxg_fft_bank mxg_fft_bank;
mxg_fft_bank *mxg_fft_bank_create(size_t V, int fftSize, int hopSize, int windowSize);
int mxg_fft_bank_destroy(mxg_fft_bank *b);
int mxg_fft_bank_reset(mxg_fft_bank *b);     /* the state after setup */
int mxg_fft_bank_pos(const mxg_fft_bank *b); /* fill */
int mxg_fft_bank_process(mxg_fft_bank *b, const double *d_in, size_t N, int layout, float *d_real, float *d_imag, float *d_mags,
                         float *d_phases, void *stream);

/* maxiIFFTBank(V) is V maxiIFFT objects after setup(fftSize, hopSize, windowSize) (L/maxiFFT.cpp:141-152) called once per sample
 * (:154-192).  A call produces d_out, double [N][V] (device), for any N: each float process() returns, widened exactly.  State
 * per stream: buffer[fftSize] on the device (mxg_ifft_bank_buffer: [V][fftSize] as the reference would leave them); `pos` in
 * [0, hopSize) for the bank, on the host.  A spectrum is consumed at every sample of the call where pos == 0 (:155): C points.
 * input 0 = SPECTRUM: d_a = magnitudes, d_b = phases, as mxg_ifft_batch; 1 = cartesian: d_a = real, d_b = imag, with the
 * as_reference = 0 meaning of mxg_ifft_batch_complex (the reference's COMPLEX mode, which transforms zeros, is not offered).
 * Rows are fp32 [V * nrows][bins], nrows per stream, in either layout of mxg_fft_bank_process.
 * row_mode 0 = direct: nrows = C, row j is consumed at point j.
 * row_mode 1 = after-FFT: the per-sample loop of cpp/commandline/tests/ffttest/ffttest.cpp in lock-step with an mxg_fft_bank of
 * the same hopSize created at the same time: nrows = the F rows that bank emitted for the same N.  Frame k completes at global
 * sample k * hopSize + hopSize - 1 and is consumed at (k + 1) * hopSize, so with p = pos on entry point j takes row j when
 * p > 0 and row j - 1 when p == 0; row -1 is the HELD spectrum, bank state [V][bins] x 2 that starts at zero (maxiFFT's
 * magnitudes / phases after setup, :52-54) and becomes the last row passed after every after-FFT call that passed one.
 * A wrong nrows is refused.  Launches per call: frames, overlap-add, and in after-FFT mode two device copies -- whatever V, N. */
typedef struct mxg_ifft_bank mxg_ifft_bank;
mxg_ifft_bank *mxg_ifft_bank_create(size_t V, int fftSize, int hopSize, int windowSize);
int mxg_ifft_bank_destroy(mxg_ifft_bank *b);
int mxg_ifft_bank_reset(mxg_ifft_bank *b);
int mxg_ifft_bank_pos(const mxg_ifft_bank *b);
const float *mxg_ifft_bank_buffer(const mxg_ifft_bank *b); /* device [V][fftSize]; valid until the next call on the bank */
int mxg_ifft_bank_process(mxg_ifft_bank *b, int input, int row_mode, int layout, const float *d_a, const float *d_b, size_t nrows,
                          size_t N, double *d_out, void *stream);

/* Where a call of N samples puts its frames and consumption points: stateless, integer host code, the function both _process
 * calls use (csrc/mxg_spectral_bank.h).  fft_fill / ifft_pos on entry (each in [0, hopSize)); *frames = F, *points = C,
 * *first_is_held = 1 when after-FFT rows start at the held spectrum (ifft_pos == 0 and C > 0), *new_fill / *new_pos on exit.
 * Any output pointer may be NULL. */
int mxg_spectral_bank_plan_host(int fftSize, int hopSize, int windowSize, int fft_fill, int ifft_pos, size_t N, size_t *frames,
                                size_t *points, int *first_is_held, int *new_fill, int *new_pos);

/* ---- maxiMFCC batch --------------------------------------------------------------------- */
/* maxiMFCC::setup(numBins, numFilters, numCoeffs, minFreq, maxFreq) (L/maxiMFCC.h:56-75): builds
 * the mel filterbank and DCT tables on the host libm.  Works without a device (tables only). */
typedef struct mxg_mfcc_plan mxg_mfcc_plan;
mxg_mfcc_plan *mxg_mfcc_plan_create(unsigned numBins, unsigned numFilters, unsigned numCoeffs,
                                    double minFreq, double maxFreq);
int mxg_mfcc_plan_destroy(mxg_mfcc_plan *plan);
/* Copy out the host tables in the reference's layouts: melFilters[filter + bin*numFilters],
 * dct[i + j*numCoeffs].  Either may be NULL.  Returns the number of leading bins that carry a
 * non-zero weight. */
int mxg_mfcc_plan_tables(const mxg_mfcc_plan *plan, double *h_melFilters, double *h_dct);
/* The same tables cut for the matrix pipe (knob "fused_mel" of mxg_fft_mfcc_batch): filters in quads, two quads per pair,
 * each quad contracting over a band of 16 * nb[pair] bins from base[pair][quad] on.  h_nb [6], h_base [6][2],
 * h_W [(batches + 1) * 128] = [batch][half][lane32 = 8 k + 4 quad + filter-of-quad][2] weights (melFilters of
 * L/maxiMFCC.h:118-182, zero outside a filter's support), h_D [4][6][32] = dct (L/maxiMFCC.h:183-203) as
 * [coefficient quad][pair][8 filter-of-quad + 4 quad + coefficient-of-quad].  Any pointer may be NULL.  Returns the number
 * of batches, 0 when the bank has no such tables (more than 48 filters or 16 coefficients, a filter reading bin 0 or beyond
 * bin 255).  Works without a device. */
int mxg_mfcc_plan_matrix_tables(const mxg_mfcc_plan *plan, int *h_nb, int *h_base, double *h_W, size_t capW, double *h_D);
/* mfcc() over nframes spectra d_mags[f*mag_stride + bin] (fp32, as getMagnitudes() yields) ->
 * d_mfcc [nframes][numCoeffs] (L/maxiMFCC.h:77-81).  Optional: d_melraw = the band sums before
 * the log (bit-exact with method 0), d_melbands = melBands after log-square, [nframes][numFilters].
 * method 0: exact sparse evaluation in the reference's summation order; method 1: dense fp64 MFMA
 * contraction (v_mfma_f64_16x16x4_f64), reordered/fused sums => tolerance. */
int mxg_mfcc_batch(const mxg_mfcc_plan *plan, const float *d_mags, size_t mag_stride, size_t nframes,
                   double *d_melraw, double *d_melbands, double *d_mfcc, int method, void *stream);

/* ---- maxiBark / maxiFFTOctaveAnalyzer batches (K19, bands.hip) ------------------------------------------------------- */
/* maxiBarkScaleAnalyser<double>::setup(sR, bS) (L/maxiBark.h:40-62): the 25 band limits, built on the host libm (works without a
 * device).  Limit 24 is specSize - 1 = bufferSize / 2 - 1, as the reference reads it back: the last bin is never summed, bands can
 * be empty.  NULL + MXG_ERR_INVALID: bufferSize outside [2, 4096] (the reference's barkScale[2048]), a bin * sampleRate that
 * overflows 32 bits. */
#define MXG_BARK_BANDS 24
typedef struct mxg_bark_plan mxg_bark_plan;
mxg_bark_plan *mxg_bark_plan_create(unsigned sampleRate, unsigned bufferSize);
int mxg_bark_plan_destroy(mxg_bark_plan *plan);
int mxg_bark_plan_limits(const mxg_bark_plan *plan, int *h_limits /* [25] */);
/* specificLoudness / relativeLoudness / totalLoudness (L/maxiBark.h:64-116) over nframes rows d_spectrum[f*stride + bin] (fp32,
 * stride >= bufferSize / 2) -> d_bandsum / d_specific / d_relative [nframes][24], d_total [nframes].  Any output may be NULL: a
 * stage not asked for neither runs nor touches its array.  The band sums are bit-exact (a double accumulated bin after bin);
 * specific = pow(sum, 0.23) is the device library's pow (tolerance: DESIGN.md, K19).  A silent frame gives 24 NaNs in d_relative. */
int mxg_bark_batch(const mxg_bark_plan *plan, const float *d_spectrum, size_t stride, size_t nframes, double *d_bandsum,
                   double *d_specific, double *d_relative, double *d_total, void *stream);
/* maxiFFTOctaveAnalyzer::setup (L/maxiFFT.cpp:207-259): the spe2avg map in float arithmetic, on the host (works without a device).
 * NULL + MXG_ERR_INVALID: nSpectrum outside [1, 4096], a non-finite or non-positive samplingRate, a negative nAveragesPerOctave
 * (the reference's setup() does not return), more than 16384 averages, and -- a defined departure -- a configuration with
 * nAverages == 0 (samplingRate / 2 at or below the first band's 55 Hz), which the reference sets up as an analyser of nothing. */
typedef struct mxg_octave_plan mxg_octave_plan;
mxg_octave_plan *mxg_octave_plan_create(float samplingRate, int nSpectrum, int nAveragesPerOctave);
int mxg_octave_plan_destroy(mxg_octave_plan *plan);
int mxg_octave_plan_averages(const mxg_octave_plan *plan);              /* nAverages */
int mxg_octave_plan_map(const mxg_octave_plan *plan, int *h_spe2avg);   /* [nSpectrum] */
/* calculate() (L/maxiFFT.cpp:261-300) for nstreams analysers over frames_per_stream frames each: frame g = s*frames_per_stream + k
 * is row d_mags[g*stride + bin] (stride >= nSpectrum).  d_averages and the optional d_peaks_out are
 * [nstreams*frames_per_stream][nAverages].  d_peak_state / d_hold_state [nstreams][nAverages] are peaks / peakHoldTimes, in and
 * out, carried from call to call (a fresh analyser: zeros); both NULL = no peak pass.  All float, bit-exact.  One stream's frames
 * are walked in order by one thread per average: the peak pass is serial in time. */
int mxg_octave_batch(const mxg_octave_plan *plan, const float *d_mags, size_t stride, size_t nstreams, size_t frames_per_stream,
                     float eq_intercept, float eq_slope, int peakHoldTime, float peakDecayRate, float *d_averages, float *d_peaks_out,
                     float *d_peak_state, int32_t *d_hold_state, void *stream);

/* ---- maxiFFT + maxiMFCC in one pass (the loop of cpp/commandline/tests/mfcctest/mfcctest.cpp:21-32 over a batch) ---- */
/* For every frame k = d_signal[k*frame_stride .. +1024): mags = maxiFFT(1024).process(...) magnitudes (L/fft.cpp:499-511),
 * then maxiMFCC::mfcc(mags) (L/maxiMFCC.h:77-81) -> d_mfcc [nframes][numCoeffs], in ONE kernel: the magnitudes stay in
 * LDS, so a frame costs its 4096 B of input and its numCoeffs*8 B of output in HBM traffic.  fft_plan must be a
 * 1024-point plan and mfcc_plan one for 512 bins with at most 64 filters (otherwise MXG_ERR_INVALID: use mxg_fft_batch +
 * mxg_mfcc_batch).  Optional outputs (NULL = not produced): d_mags [nframes][512] (bit-exact, as mxg_fft_batch),
 * d_melraw / d_melbands [nframes][numFilters] (as mxg_mfcc_batch method 0: band sums bit-exact, log-square / mfcc
 * within the device log's tolerance). */
int mxg_fft_mfcc_batch(const mxg_fft_plan *fft_plan, const mxg_mfcc_plan *mfcc_plan, const float *d_signal,
                       size_t frame_stride, size_t nframes, float *d_mags, double *d_melraw, double *d_melbands,
                       double *d_mfcc, void *stream);

/* ---- maxiGrains: maxiTimeStretch / maxiStretch banks --------------------------------------- */
/* Window kinds = the functors of L/maxiGrains.h:18-90: 0 hann 1 hamming 2 cosine 3 rect 4 triangle
 * 5 triangleNZ 6 blackmanHarris 7 blackmanNutall 8 gaussian(0.3).  A plan holds the window table
 * maxiGrainWindowCache::getWindow (:112-120) would build for grains of grainLength seconds of a
 * sample at mySampleRate (host libm); the length must be < sampleRate/2 like the cache (:98). */
typedef struct mxg_grain_plan mxg_grain_plan;
mxg_grain_plan *mxg_grain_plan_create(int window_kind, double grainLength, int mySampleRate);
int mxg_grain_plan_destroy(mxg_grain_plan *plan);
int mxg_grain_plan_window(const mxg_grain_plan *plan, double *h_window); /* returns sampleDur */
/* S independent streams over one shared sample (mxg_sample_upload), T samples each, d_out[n*S + s].
 * mode 0 = maxiTimeStretch<F>::play(speed = a[s], grainLength, overlaps, posMod[s]) (:341-355);
 * mode 1 = maxiStretch<F>::play(pitchstretch = a[s], timestretch = b[s], grainLength, overlaps,
 * posMod[s]) with the default loop (whole sample) (:512-530);
 * mode 2 = maxiTimeStretch<F>::playAtPosition(pos = a[n*S + s], grainLength, overlaps) (:359-367):
 * d_a is the per-sample [T][S] position signal, the member `position` is not touched;
 * mode 3 = maxiPitchShift<F>::play(speed = a[s], grainLength, overlaps, posMod[s]) (:412-430): the
 * `looper` slot of d_st holds the member `cycles` (a long), grains are born with
 * speed - (cycleMod/cycleLength)*0.1 and therefore arbitrary increments; no rand() is drawn.
 * d_posmod may be NULL (0).
 * d_rnd: int32 [S][R], the values `rand() % 10` returns at each spawn, consumed in order per
 * stream (NULL = 0): the reference draws them from the process-wide rand() stream, which a bank
 * cannot reproduce.  State, in/out: d_st = [4][S] position, looper, randomOffset, rand cursor
 * (setPosition(p) == position = clamp(p*len, 0, len-1), :335-338); d_gst = [4][8][S]: the live
 * grains in creation order: pos, inc, sampleIdx, sampleDur (0 = empty slot).  A live grain must be
 * one this plan made (same sampleDur: a bank has one window table per plan, so let grains finish -- or
 * clear d_gst -- before switching to a plan of another grain length).  The call only enqueues on `stream`; what the device finds while
 * it renders -- more than 8 live grains in a stream, an exhausted d_rnd, such a foreign / corrupt grain, a grain born with a step its
 * reads could not survive: MXG_ERR_INVALID -- is reported by the next synchronising call or by mxg_last_async_error (knob "grain_sync" 1:
 * by the call itself, which then waits).  A tile-rendered call is ONE launch whose first workgroups are the per-stream schedulers and whose
 * other workgroups render tiles as the schedulers' lists reach them (knob "grain_streamed"). */
int mxg_granular_render(const mxg_grain_plan *plan, int mode, size_t S, size_t T, const double *d_samples,
                        size_t len, int overlaps, const double *d_a, const double *d_b,
                        const double *d_posmod, const int32_t *d_rnd, size_t R, double *d_st, double *d_gst,
                        double *d_out, void *stream);

/* mxg_granular_render plus the maxiMix::stereo mixdown of the S streams (C:503-509 and the user-side sum,
 * e.g. ofApp.cpp:166-173 of the reference's granular example): d_pan [S], d_mix [T][2] -- BASELINE configs[4]'s "stereo
 * mixdown".  On the unit-increment path (maxiTimeStretch at 44.1 kHz) the render kernel mixes each 64-stream x 64-sample
 * tile while it still sits in LDS, so the [T][S] block is not read back; every other path runs mxg_mix_stereo after the
 * render.  Per-stream outputs bit-exact as mxg_granular_render; the sum over streams is tree-ordered (mix tolerance). */
int mxg_granular_render_mix(const mxg_grain_plan *plan, int mode, size_t S, size_t T, const double *d_samples,
                            size_t len, int overlaps, const double *d_a, const double *d_b,
                            const double *d_posmod, const int32_t *d_rnd, size_t R, double *d_st, double *d_gst,
                            double *d_out, const double *d_pan, double *d_mix, void *stream);

/* ---- granular streams over the slots of a sample pool (K27, csrc/grainpool.hip, csrc/mxg_grainpool.h) ------------------------
 * S streams that each read their OWN slot: the reference's maxiTimeStretch / maxiPitchShift / maxiStretch objects after
 * setSample(), maxiStretch with its loop points (L/maxiGrains.h:445, :493-509, :514-517) and maxiStretch::playAtPosition
 * (:531-539).  The pool is the one of mxg_sample_pool_alloc (slot r = d_pool + r * stride, d_len [R]; a length above cap is read as
 * cap); a pointer from mxg_sample_upload with R = 1, stride = 0 and a one-element d_len is a valid pool too.
 *   mode     0 ... 3 as mxg_granular_render; 4 = maxiStretch::playAtPosition(pitchstretch = a, pos = b, grainLength, overlaps).
 *   d_slot   uint32 [S]: the slot each stream reads; NULL: stream s reads slot s (needs S <= R).  An index >= R is refused before
 *            anything is launched: the S indices are read back, which is this entry point's one wait (NULL: none).
 *   d_loop   uint64 [2][S]: loopStart | loopEnd in samples (mxg_stretch_loop_host makes them); NULL: 0 and len.  Mode 1 only.
 *   d_a      modes 0 / 3 speed, 1 / 4 pitchstretch: [S], or [T][S] under MXG_GPOOL_PS_A; mode 2: the position signal [T][S].
 *   d_b      mode 1 timestretch, mode 4 the position: [S], or [T][S] under MXG_GPOOL_PS_B.
 *   d_posmod modes 0 / 1 / 3: NULL, [S], or [T][S] under MXG_GPOOL_PS_POSMOD.
 * A per-sample value is the argument a patch hands play() in that sample: speed / rate move `position` at every sample, a grain
 * takes the values of the sample it is born in.  d_rnd [S][Rn], d_st [4][S], d_gst [4][8][S] and d_out [T][S] mean what they mean in
 * mxg_granular_render (a carried grain is checked against the stream's own slot length), and what the device finds while it renders
 * is reported the same way, through mxg_last_async_error.  A stream whose slot is empty reads nothing, keeps its state and is
 * silent (reported as a step its reads could not survive).  BIT-EXACT, and independent of how T is split into calls; with one
 * slot, d_loop = NULL and ps_flags = 0, modes 0 ... 3 give the output and state of mxg_granular_render on the same sample.
 * mxg_granular_pool_host: the same text on host arrays in the pool's layout, no device touched; a failure of a stream is its
 * status.  mxg_stretch_loop_host: setLoopStart / setLoopEnd's conversions (unsigned long)(val * len); NaN, a negative value,
 * loopStart >= loopEnd (where the reference's unsigned loopLength wraps: INTEGRATION.md section 4) and loopEnd > len are refused. */
#define MXG_GPOOL_PS_A 1
#define MXG_GPOOL_PS_B 2
#define MXG_GPOOL_PS_POSMOD 4
int mxg_granular_pool_render(const mxg_grain_plan *plan, int mode, size_t S, size_t T, const double *d_pool, size_t stride, size_t cap,
                             size_t R, const uint64_t *d_len, const uint32_t *d_slot, const uint64_t *d_loop, int overlaps,
                             const double *d_a, const double *d_b, const double *d_posmod, int ps_flags, const int32_t *d_rnd, size_t Rn,
                             double *d_st, double *d_gst, double *d_out, void *stream);
int mxg_granular_pool_host(const mxg_grain_plan *plan, int mode, size_t S, size_t T, const double *h_pool, size_t stride, size_t cap,
                           size_t R, const uint64_t *h_len, const uint32_t *h_slot, const uint64_t *h_loop, int overlaps,
                           const double *h_a, const double *h_b, const double *h_posmod, int ps_flags, const int32_t *h_rnd, size_t Rn,
                           double *h_st, double *h_gst, double *h_out);
int mxg_stretch_loop_host(uint64_t len, double start01, double end01, uint64_t *loopStart, uint64_t *loopEnd);

/* ---- multi-GPU mixdown: RCCL over xGMI ------------------------------------------------ */
/* The reference is single-device; there is nothing to cite but the mix itself (maxiMix, C:503-541, and the user-side
 * sum over voices, 15.polysynth/main.cpp:67).  Banks shard over the GPUs of a node by contiguous voice / stream /
 * frame ranges, one process per GPU, private state, no data-path collective -- except that the per-rank
 * [samples][channels] fp64 mix blocks are summed onto one GPU with ncclReduce(ncclDouble, ncclSum, root).
 * Sum order across ranks is RCCL's, not the reference's sequential voice order: the mix carries the tolerance of
 * mxg_mix_stereo, per-voice signals stay bit-exact.
 * mxg_comm_unique_id: rank 0 obtains the 128-byte ncclUniqueId; the host distributes it (torch.distributed, MPI,
 * a file ...); every rank then calls mxg_comm_create(id, nranks, rank) on the device it selected with mxg_init.
 * librccl is resolved at this point (dlopen by SONAME), not when libmaxigpu.so loads. */
#define MXG_COMM_ID_BYTES 128
typedef struct mxg_comm mxg_comm;
int mxg_comm_unique_id(void *h_id);
mxg_comm *mxg_comm_create(const void *h_id, int nranks, int rank);
int mxg_comm_destroy(mxg_comm *comm);
int mxg_comm_rank(const mxg_comm *comm);
int mxg_comm_size(const mxg_comm *comm);
/* d_recv (on `root`; on every rank when all != 0) = sum over ranks of d_send[count], in `stream` order (in place
 * allowed).  comm NULL: a device copy (a one-rank communicator goes through RCCL like any other). */
int mxg_comm_reduce(mxg_comm *comm, const double *d_send, double *d_recv, size_t count, int root, int all,
                    void *stream);
/* maxiMix bus over this rank's V voices (as mxg_mix_bus without d_bus) into d_mix [N][channels], then the sum over
 * ranks into the root's d_mix -- the whole exchange step for a host that reduces block by block. */
int mxg_mix_reduce(mxg_comm *comm, int channels, size_t V, size_t N, const double *d_in, const double *d_x,
                   const double *d_y, const double *d_z, double *d_mix, int root, void *stream);
/* Batched, overlapped form: an 8 KiB [512][2] block is a latency-bound message, so the local mixes of `depth_blocks`
 * consecutive blocks are staged and reduced with ONE ncclReduce (depth 16 = 128 KiB) on the queue's own stream while
 * the caller's stream renders the next batch into the second staging buffer (device-side event ordering only; no call
 * here blocks the host).  Per block:  p = mxg_mixq_slot(q, stream);  <enqueue the local mix of the block into p, e.g.
 * mxg_osc_render_mix / mxg_mix_stereo with d_mix = p>;  mxg_mixq_push(q, stream).  mxg_mixq_flush reduces a partial
 * batch and makes `stream` wait for every outstanding reduce.  mxg_mixq_result: device pointer to the most recently
 * submitted batch's sum [blocks][block_doubles] (meaningful on the root once its reduce has completed, e.g. after
 * flush + stream sync; the reduce of the batch after next overwrites it ON THE QUEUE'S STREAM -- a consumer that reads it with
 * work enqueued on a stream calls mxg_mixq_release(q, that stream) after enqueueing its reads, and the overwriting reduce is
 * ordered behind them; a consumer that synchronises and copies before it pushes further blocks needs nothing).  mxg_mixq_set_sink: the root additionally copies every summed
 * block into a pinned host ring [ring_blocks][block_doubles] (the audio callback's side of the boundary). */
typedef struct mxg_mixq mxg_mixq;
mxg_mixq *mxg_mixq_create(mxg_comm *comm, size_t block_doubles, int depth_blocks, int root);
/* Grouped slots: mxg_mixq_slot hands out [groups][block_doubles] -- the rows of mxg_osc_render_mix_rows -- and the queue adds the
 * rows of a whole batch with one kernel on ITS stream in front of the reduce (groups = 1: the plain queue). */
mxg_mixq *mxg_mixq_create_grouped(mxg_comm *comm, size_t block_doubles, int depth_blocks, int root, size_t groups);
int mxg_mixq_destroy(mxg_mixq *q);
int mxg_mixq_set_sink(mxg_mixq *q, double *h_pinned, size_t ring_blocks);
double *mxg_mixq_slot(mxg_mixq *q, void *stream);
int mxg_mixq_push(mxg_mixq *q, void *stream);
int mxg_mixq_flush(mxg_mixq *q, void *stream);
const double *mxg_mixq_result(const mxg_mixq *q, size_t *h_blocks, size_t *h_batches);
int mxg_mixq_release(mxg_mixq *q, void *stream);

/* ---- long signals of few voices, parallel in time (K28) ------------------------------------------------------------------
 * mxg_scan_long_render: V voices (1 ... 4096) x N samples (1 ... 2^28) of a LINEAR filter with block-constant coefficients, the
 * signal [N][V] cut into chunks of 2048 samples that are joined by a scan: three launches on `stream` (chunk summaries, the scan
 * over the chunks, the render), no workgroup waiting on another.  V = 1 is a plain contiguous signal (a sample-pool slot, an
 * uploaded maxiSample).  d_out == d_in is allowed; any other overlap of the two is refused.  Out-of-range V, N or kind: MXG_ERR_INVALID.
 *   kind 0 maxiDCBlocker, 1 maxiSVF, 2 maxiBiquad   d_coef / d_st: mxg_filter2_render's [NC][V] / [3][V]
 *   kind 3 lores, 4 hires                           d_coef: rows c, r of mxg_filter_coeffs_host; d_st: mxg_filter_render's [5][V],
 *                                                   rows 0-1 read and written, rows 2-4 left as they are
 *   kind 5 maxiLagExp                               d_coef [2][V] = alpha, alphaReciprocal; d_st [1][V] = val (mxg_lag_render's d_val)
 * One state array can alternate between this entry point and the sequential one of its kind.  The knob time_parallel plays no part.
 * The arithmetic is REORDERED (a state reaches a chunk through matrix products): a TOLERANCE mode.  |error| <= SCAN_LONG_RTOL x the
 * voice's peak of the sequential output, for stable settings and finite input over the whole parameter domain and a stream of up to
 * 2.5e7 samples per voice carried from a state; per kind, measured on the host twin (worst over N = 2, 65 and 4097 chunks and a ragged N,
 * three carried calls, the whole sweep at 4097 chunks among them) -> the bound (worst x 2, one digit, rounded up):
 *     maxiDCBlocker 2.3e-12 -> 5e-12    maxiSVF 3.5e-10 -> 8e-10    maxiBiquad 1.6e-10 -> 4e-10 (the sequential recurrence is itself
 *     lores 7.6e-13 -> 2e-12            hires 7.4e-13 -> 2e-12      maxiLagExp 4.1e-12 -> 9e-12  1.3e-10 from a long-double one there)
 * The worst cases are the settings that barely decay.  An UNDAMPED maxiSVF (res 0, |pole| = 1) is the one whose error keeps growing
 * with the length of the stream -- 5.1e-11 after 8.4e6 samples, 3.3e-10 after 2.5e7 at 15 kHz -- and beyond that length its bound does
 * not hold (tests/test_scan_long_host.py has the table).
 * After a NaN / Inf input sample the outputs and states are non-finite where the sequential recurrence's are; NaN and Inf may
 * trade places.  mxg_scan_long_host: the same arithmetic on host arrays -- the device gives these bits. */
int mxg_scan_long_render(int kind, size_t V, size_t N, const double *d_in, const double *d_coef, double *d_st, double *d_out, void *stream);
int mxg_scan_long_host(int kind, size_t V, size_t N, const double *h_in, const double *h_coef, double *h_st, double *h_out);

/* ---- the same with PER-SAMPLE coefficients: a time-varying scan (K31) -------------------------------------------------------
 * mxg_scan_long_render_swept: mxg_scan_long_render for a filter whose coefficients move every sample -- kind 3 lores, 4 hires,
 * 5 maxiLagExp, the kinds that have a sequential per-sample entry point (mxg_filter_render_coefs; mxg_lag_render with
 * alpha_per_sample = 1) to hand a stream to and from.  Kinds 0-2 have no swept form: MXG_ERR_INVALID, and the message says so.
 *   d_coef_ps  [N][coef_rows][V], coef_rows 2 ... 8; rows 0 and 1 are read: (c, r) of mxg_filter_coeffs_host, or (alpha,
 *              alphaReciprocal).  The [N][3][V] array of mxg_filter_render_coefs is taken as it is with coef_rows = 3; a caller who
 *              minds the traffic packs 2 rows.
 *   d_st       as mxg_scan_long_render for the kind: [5][V], rows 0-1 read and written, rows 2-4 left as they are; [1][V] for the lag.
 * V 1 ... 4096, N 1 ... 2^28.  d_out == d_in is allowed; a partial overlap of the two, any overlap of d_out with d_coef_ps and null
 * pointers are refused (before the device is touched).  The signal is cut into chunks of 1024 samples; every chunk and every lane
 * carries an affine pair (M, e) of its own, composed by scans: three launches on `stream`, no workgroup waiting on another.  One
 * state array can alternate between this entry point, mxg_scan_long_render and the sequential entry points of the kind.
 * A TOLERANCE mode as mxg_scan_long_render: |error| <= SWEPT_RTOL x the voice's peak of the sequential output, for sweeps whose
 * sequential float64 output is finite with peak <= 1e6 (cutoffs inside 10 Hz ... 8 kHz) and finite input, measured on the host twin
 * over the sweep set of tests/scan_long_swept_host.py (LFOs, ramps, steps; resonance 1 ... 1000 and swept; alpha 1e-6 ... 1) at 2, 66
 * and 4097 chunks and a ragged N, and over the constant scan's full-domain settings HELD still at 66 and 4097 chunks, three carried
 * calls -> the bound (worst x 2, one digit, rounded up; tools/measure_longsweep_tolerance.py, profiles/longsweep_tolerance.json,
 * DESIGN.md K31):
 *     lores 2.8e-12 -> 6e-12    hires 2.8e-12 -> 6e-12    maxiLagExp 2.1e-12 -> 5e-12
 * The worst are barely-damped settings that stand still (10 Hz at resonance 1000; alpha 1e-6); their error stops growing once the
 * stream is longer than the setting's memory, so the bound does not depend on the length (measured to 1.26e7 samples per voice).
 * Over sweeps that move the figure is 4e-14, the float64 sequential recurrence's own distance from a long-double one.  A cutoff
 * stepping at random at resonance >= 100 diverges in the reference itself and is outside the set.
 * N < 64 is plain steps: the sequential recurrence's bits.  Non-finite input: as mxg_scan_long_render.
 * mxg_scan_long_swept_host: the same arithmetic on host arrays -- the device gives these bits. */
int mxg_scan_long_render_swept(int kind, size_t V, size_t N, const double *d_in, const double *d_coef_ps, size_t coef_rows,
                               double *d_st, double *d_out, void *stream);
int mxg_scan_long_swept_host(int kind, size_t V, size_t N, const double *h_in, const double *h_coef_ps, size_t coef_rows,
                             double *h_st, double *h_out);

/* (The bandwidth-probe kernels bench.py and tools/ measure ceilings with are NOT part of this ABI: include/maxicalib.h,
 * libmaxicalib.so -- measurement code, built beside the product library.) */

#ifdef __cplusplus
}
#endif
#endif /* MAXIGPU_H */
