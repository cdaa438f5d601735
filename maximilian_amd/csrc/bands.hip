// bands.hip -- K19: maxiBark and maxiFFTOctaveAnalyzer over batches of magnitude rows on gfx950.
//
// Path (reference, L/ = src/libs/): maxiBarkScaleAnalyser<double>::setup / specificLoudness / relativeLoudness / totalLoudness
// L/maxiBark.h:40-116; maxiFFTOctaveAnalyzer::setup / calculate L/maxiFFT.cpp:207-300.  The arithmetic is mxg_bands.h, shared
// with the host build of the tests; the tables are built on the host libm and work without a device.
//
// Both analysers are a segmented sum over a row of bins, per frame, in bin order.  `bark_kernel` and `octave_kernel` share one
// layout: a wavefront (= one workgroup of 64 threads) owns 64 consecutive frames, one LANE per frame.  Every lane walks the same
// band edges, so control flow is wave-uniform and no lane idles (a lane per band would keep 24 of 64 lanes busy, band 23 alone
// for 245 of 512 bins).  A row is 2 KB, so a lane must not read its own row from memory: the wave loads a [64 frames x 32 bins]
// tile with 16-byte loads ALONG the rows (8 lanes cover the 128 B of one row, one instruction = 8 rows), one tile ahead in
// registers, parks it in LDS with a row pitch of 36 floats and reads it back transposed, lane f taking 16 bytes at word
// 36 f + 4 j.  ds_read_b128 is served in four groups of 16 lanes whose lane numbers cover every residue mod 16; the 16-byte slot
// of lane f is (36 f / 4) mod 16 = 9 f mod 16, a bijection of f mod 16: each group touches 16 different slots = all 64 banks
// once, conflict-free (the tile of mfcc.hip's K7a-t).  Rows whose base or stride is not 16-byte aligned take 4-byte loads
// (ALIGNED = false); the last chunk and the frame tail are guarded per element / clamped to the last frame, so nothing outside a
// row's [0, bins) is read.
// Results leave as contiguous row segments: a closed band goes to an LDS result tile (Bark: [64][25] doubles, pitch 25 so that
// lanes f and f + 16 are the only pair on a bank; octave: [64][33] floats, bank (33 f + j) mod 32 = (f + j) mod 32, conflict-free)
// and the tile is copied out linearly -- the [64][24] block of a wave's frames is ONE contiguous 12 KB span of the output, the
// octave averages leave in chunks of 32 per frame (128-byte segments).
// `octave_peaks_kernel`: one thread per (stream, average) walks that stream's frames in order over the averages just written and
// carries peaks / peakHoldTimes.  One stream with very many frames is serial in time here; a time-parallel form is out of scope.
//
// Numerics: band sums, averages, peaks and hold counters are bit-exact (+, *, /, compares; no contraction).  pow(sum, 0.23) is
// the device library's: the only tolerance.
#include <math.h>
#include <string.h>

#include <vector>

#include "mxg_common.h"

#include "mxg_bands.h"

struct mxg_bark_plan {
    unsigned sampleRate, bufferSize, specSize;
    int lim[MXG_BARK_BANDS + 1];
    int *d_bandof;  // [specSize]: the band of every summed bin
};

struct mxg_octave_plan {
    float samplingRate, span, inc;
    int nSpectrum, perOctave, nAverages;
    std::vector<int> map;
    int *d_map;
};

namespace mxg {
namespace {

constexpr int kTileBins = 32, kTileStride = 36;  // floats; 144-byte rows: 16-byte aligned, conflict-free transposed b128 reads
constexpr int kBarkPitch = MXG_BARK_BANDS + 1;   // doubles
constexpr int kOctChunk = 32, kOctPitch = kOctChunk + 1;  // floats

// The tile's global side: lane -> (row = lane / 8 + 8 k, 4 bins at 4 * (lane % 8)), k = 0 .. 7.  Rows past the last frame are
// clamped to it (valid memory, results discarded); bins at or past nb are never read.
struct TileSrc {
    const float *row[8];
    int lcol;
};

__device__ inline TileSrc tile_src(const float *mags, size_t stride, size_t nframes, size_t frame0, int lane) {
    TileSrc s;
    s.lcol = (lane & 7) * 4;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        size_t fr = frame0 + (size_t)((lane >> 3) + 8 * k);
        if (fr >= nframes) fr = nframes - 1;
        s.row[k] = mags + fr * stride;
    }
    return s;
}

template <bool ALIGNED>
__device__ inline void tile_load(const TileSrc &s, unsigned t, int nb, float (&nxt)[8][4]) {
    const int b0 = (int)t * kTileBins + s.lcol;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (ALIGNED && b0 + 4 <= nb) {
            const float4 v4 = *reinterpret_cast<const float4 *>(s.row[k] + b0);
            nxt[k][0] = v4.x; nxt[k][1] = v4.y; nxt[k][2] = v4.z; nxt[k][3] = v4.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) nxt[k][j] = (b0 + j < nb) ? s.row[k][b0 + j] : 0.f;
        }
    }
}

__device__ inline void tile_park(float *tile, int lane, const float (&nxt)[8][4]) {
    const int lrow = lane >> 3, lcol = (lane & 7) * 4;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float4 v4 = {nxt[k][0], nxt[k][1], nxt[k][2], nxt[k][3]};
        *reinterpret_cast<float4 *>(tile + (lrow + 8 * k) * kTileStride + lcol) = v4;
    }
}

// ---- maxiBark ----------------------------------------------------------------------------------------------------------------
struct BarkArgs {
    const float *mags;
    size_t stride, nframes;
    int nb;             // bins that are summed: specSize - 1
    const int *bandof;  // [nb] the band of each of them (wave-uniform reads)
    double *bandsum, *specific, *relative, *total;
};

template <bool ALIGNED>
__global__ __launch_bounds__(64) void bark_kernel(const BarkArgs A) {
    __shared__ __attribute__((aligned(16))) float s_tile[64 * kTileStride];
    __shared__ double s_res[64 * kBarkPitch];
    const int lane = threadIdx.x;
    const size_t frame0 = (size_t)blockIdx.x * 64;
    const size_t left = A.nframes - frame0;
    const int rows = left < 64 ? (int)left : 64;
    const TileSrc src = tile_src(A.mags, A.stride, A.nframes, frame0, lane);
    const int nb = A.nb;
    const unsigned ntiles = (unsigned)((nb + kTileBins - 1) / kTileBins);
    float nxt[8][4];
    if (ntiles) tile_load<ALIGNED>(src, 0, nb, nxt);
    double *myres = s_res + lane * kBarkPitch;
    double sum = 0;
    int band = 0;
    for (unsigned t = 0; t < ntiles; t++) {
        tile_park(s_tile, lane, nxt);
        if (t + 1 < ntiles) tile_load<ALIGNED>(src, t + 1, nb, nxt);
        __syncthreads();
        const float *row = s_tile + lane * kTileStride;
        const int bbase = (int)t * kTileBins;
        for (int j4 = 0; j4 < kTileBins / 4; j4++) {
            const float4 xv = *reinterpret_cast<const float4 *>(row + 4 * j4);
            const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int b = bbase + 4 * j4 + j;
                if (b < nb) {  // wave-uniform, as the band of the bin
                    const int bd = A.bandof[b];
                    if (bd != band) {  // the bands that end before this bin: the open one, then the empty ones
                        for (int bb = band; bb < bd; bb++) {
                            myres[bb] = sum;
                            sum = 0;
                        }
                        band = bd;
                    }
                    sum = bnd_bark_add(sum, x4[j]);
                }
            }
        }
        __syncthreads();
    }
    for (int bb = band; bb < MXG_BARK_BANDS; bb++) {  // the band that ends at nb, and the empty ones after it
        myres[bb] = sum;
        sum = 0;
    }
    __syncthreads();
    const size_t obase = frame0 * MXG_BARK_BANDS;
    const int nout = rows * MXG_BARK_BANDS;
    if (A.bandsum) {
        for (int e = lane; e < nout; e += 64) A.bandsum[obase + e] = s_res[(e / MXG_BARK_BANDS) * kBarkPitch + e % MXG_BARK_BANDS];
    }
    if (A.specific || A.relative || A.total) {  // the loudness epilogue on the wave's tile: lane = frame, results out linearly
        __syncthreads();
        double mx, total;
        bnd_bark_loudness(myres, mx, total);
        if (A.total && lane < rows) A.total[frame0 + lane] = total;
        __syncthreads();
        if (A.specific) {
            for (int e = lane; e < nout; e += 64) A.specific[obase + e] = s_res[(e / MXG_BARK_BANDS) * kBarkPitch + e % MXG_BARK_BANDS];
        }
        if (A.relative) {
            __syncthreads();
            bnd_bark_relative(myres, mx);
            __syncthreads();
            for (int e = lane; e < nout; e += 64) A.relative[obase + e] = s_res[(e / MXG_BARK_BANDS) * kBarkPitch + e % MXG_BARK_BANDS];
        }
    }
}

// ---- maxiFFTOctaveAnalyzer -----------------------------------------------------------------------------------------------------
struct OctArgs {
    const float *mags;
    size_t stride, nframes;
    int nb, nAverages;
    const int *map;
    float intercept, slope;
    float *averages;
};

// averages [jbase, jbase + n) of the wave's `rows` frames: LDS result tile -> rows of the output, 4 n bytes per frame
__device__ inline void oct_flush(const float *s_res, float *averages, size_t frame0, int rows, int nAverages, int jbase, int n, int lane) {
    __syncthreads();
    const int nout = rows * n;
    if (n == kOctChunk) {
        for (int e = lane; e < nout; e += 64)
            averages[(frame0 + (size_t)(e >> 5)) * (size_t)nAverages + (size_t)(jbase + (e & 31))] = s_res[(e >> 5) * kOctPitch + (e & 31)];
    } else {
        for (int e = lane; e < nout; e += 64) {
            const int r = e / n, c = e - r * n;
            averages[(frame0 + (size_t)r) * (size_t)nAverages + (size_t)(jbase + c)] = s_res[r * kOctPitch + c];
        }
    }
    __syncthreads();
}

template <bool ALIGNED>
__global__ __launch_bounds__(64) void octave_kernel(const OctArgs A) {
    __shared__ __attribute__((aligned(16))) float s_tile[64 * kTileStride];
    __shared__ float s_res[64 * kOctPitch];
    const int lane = threadIdx.x;
    const size_t frame0 = (size_t)blockIdx.x * 64;
    const size_t left = A.nframes - frame0;
    const int rows = left < 64 ? (int)left : 64;
    const TileSrc src = tile_src(A.mags, A.stride, A.nframes, frame0, lane);
    const int nb = A.nb;
    const unsigned ntiles = (unsigned)((nb + kTileBins - 1) / kTileBins);
    float nxt[8][4];
    tile_load<ALIGNED>(src, 0, nb, nxt);
    float *myres = s_res + lane * kOctPitch;
    OctWalk w = {0.0f, 0, 0};
    int jbase = 0;  // the first average of the result tile
    for (unsigned t = 0; t < ntiles; t++) {
        tile_park(s_tile, lane, nxt);
        if (t + 1 < ntiles) tile_load<ALIGNED>(src, t + 1, nb, nxt);
        __syncthreads();
        const float *row = s_tile + lane * kTileStride;
        const int bbase = (int)t * kTileBins;
        for (int j4 = 0; j4 < kTileBins / 4; j4++) {
            const float4 xv = *reinterpret_cast<const float4 *>(row + 4 * j4);
            const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int b = bbase + 4 * j4 + j;
                if (b < nb) {  // wave-uniform, as the map value and with it every group boundary
                    float avg;
                    int from, to;
                    if (bnd_oct_bin(w, x4[j], b, A.map[b], A.intercept, A.slope, avg, from, to)) {
                        for (int jj = from; jj < to; jj++) {
                            myres[jj - jbase] = avg;
                            if (jj - jbase == kOctChunk - 1) {
                                oct_flush(s_res, A.averages, frame0, rows, A.nAverages, jbase, kOctChunk, lane);
                                jbase += kOctChunk;
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    // (the trailing group's index is nAverages: never written, L/maxiFFT.cpp:281)
    if (A.nAverages > jbase) oct_flush(s_res, A.averages, frame0, rows, A.nAverages, jbase, A.nAverages - jbase, lane);
}

__global__ __launch_bounds__(256) void octave_peaks_kernel(size_t nstreams, size_t frames_per_stream, int nAverages, int holdTime,
                                                           float decay, const float *__restrict__ averages,
                                                           float *__restrict__ peaks_out, float *__restrict__ peak_state,
                                                           int32_t *__restrict__ hold_state) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nstreams * (size_t)nAverages) return;
    const size_t s = i / (size_t)nAverages, a = i - s * (size_t)nAverages;
    float peak = peak_state[i];
    int32_t hold = hold_state[i];
    for (size_t k = 0; k < frames_per_stream; k++) {
        const size_t at = (s * frames_per_stream + k) * (size_t)nAverages + a;
        bnd_peak_step(averages[at], peak, hold, holdTime, decay);
        if (peaks_out) peaks_out[at] = peak;
    }
    peak_state[i] = peak;
    hold_state[i] = hold;
}

bool rows_aligned16(const float *p, size_t stride) { return (((uintptr_t)p) & 15) == 0 && (stride & 3) == 0; }

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

mxg_bark_plan *mxg_bark_plan_create(unsigned sampleRate, unsigned bufferSize) {
    if (bufferSize < 2 || bufferSize > MXG_BARK_MAX_BUFFER) {
        fail(MXG_ERR_INVALID, "mxg_bark_plan_create: bufferSize %u is outside [2, %d]", bufferSize, MXG_BARK_MAX_BUFFER);
        return nullptr;
    }
    const unsigned specSize = bufferSize / 2;
    if ((uint64_t)(specSize - 1) * (uint64_t)sampleRate > 0xffffffffull) {
        fail(MXG_ERR_INVALID, "mxg_bark_plan_create: sampleRate %u: bin * sampleRate overflows 32 bits at bufferSize %u", sampleRate,
             bufferSize);
        return nullptr;
    }
    mxg_bark_plan *p = new mxg_bark_plan();
    p->sampleRate = sampleRate;
    p->bufferSize = bufferSize;
    p->specSize = specSize;
    std::vector<double> barkScale(specSize);
    bnd_bark_limits(sampleRate, bufferSize, p->lim, barkScale.data());
    std::vector<int> bandof(specSize, MXG_BARK_BANDS - 1);
    for (int b = 0; b < MXG_BARK_BANDS; b++)
        for (int i = p->lim[b]; i < p->lim[b + 1]; i++) bandof[i] = b;
    // The limits stay valid without a device (mxg_bark_plan_limits); compute calls then fail.
    p->d_bandof = nullptr;
    if (ensure_init_only() || check_hip(hipMalloc(&p->d_bandof, sizeof(int) * specSize), "hipMalloc") ||
        check_hip(hipMemcpy(p->d_bandof, bandof.data(), sizeof(int) * specSize, hipMemcpyHostToDevice), "hipMemcpy")) {
        if (p->d_bandof) (void)hipFree(p->d_bandof);
        p->d_bandof = nullptr;
    }
    return p;
}

int mxg_bark_plan_destroy(mxg_bark_plan *plan) {
    if (!plan) return MXG_OK;
    if (plan->d_bandof) (void)hipFree(plan->d_bandof);
    delete plan;
    return MXG_OK;
}

int mxg_bark_plan_limits(const mxg_bark_plan *plan, int *h_limits) {
    MXG_REQUIRE(plan, "plan is null");
    MXG_REQUIRE(h_limits, "h_limits is null");
    memcpy(h_limits, plan->lim, sizeof(plan->lim));
    return MXG_OK;
}

int mxg_bark_batch(const mxg_bark_plan *plan, const float *d_spectrum, size_t stride, size_t nframes, double *d_bandsum,
                   double *d_specific, double *d_relative, double *d_total, void *stream) {
    MXG_REQUIRE(plan, "plan is null");
    MXG_REQUIRE(d_spectrum, "d_spectrum is null");
    MXG_REQUIRE(stride >= plan->specSize, "stride is below bufferSize / 2");
    MXG_REQUIRE((nframes + 63) / 64 <= 0x7fffffffull, "nframes is beyond 2^37");
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    MXG_REQUIRE(plan->d_bandof, "plan has no device table (created without a HIP device)");
    if (nframes == 0 || !(d_bandsum || d_specific || d_relative || d_total)) return MXG_OK;
    const BarkArgs A = {d_spectrum, stride, nframes, (int)plan->specSize - 1, plan->d_bandof, d_bandsum, d_specific, d_relative, d_total};
    const dim3 grid((unsigned)((nframes + 63) / 64)), block(64);
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("bark_kernel", st);
    if (rows_aligned16(d_spectrum, stride)) hipLaunchKernelGGL((bark_kernel<true>), grid, block, 0, st, A);
    else hipLaunchKernelGGL((bark_kernel<false>), grid, block, 0, st, A);
    return check_hip(hipGetLastError(), "bark_kernel launch");
}

mxg_octave_plan *mxg_octave_plan_create(float samplingRate, int nSpectrum, int nAveragesPerOctave) {
    if (nSpectrum < 1 || nSpectrum > MXG_OCTAVE_MAX_BINS) {
        fail(MXG_ERR_INVALID, "mxg_octave_plan_create: nSpectrum %d is outside [1, %d]", nSpectrum, MXG_OCTAVE_MAX_BINS);
        return nullptr;
    }
    if (!(samplingRate > 0.0f) || !(samplingRate <= 3.402823466e38f)) {
        fail(MXG_ERR_INVALID, "mxg_octave_plan_create: samplingRate %g is not a positive finite rate", (double)samplingRate);
        return nullptr;
    }
    if (nAveragesPerOctave < 0) {  // (the reference's setup() never returns: the band tops shrink)
        fail(MXG_ERR_INVALID, "mxg_octave_plan_create: nAveragesPerOctave %d is negative", nAveragesPerOctave);
        return nullptr;
    }
    mxg_octave_plan *p = new mxg_octave_plan();
    p->samplingRate = samplingRate;
    p->nSpectrum = nSpectrum;
    p->perOctave = nAveragesPerOctave;
    p->d_map = nullptr;
    p->map.assign((size_t)nSpectrum, 0);
    p->nAverages = bnd_octave_map(samplingRate, nSpectrum, nAveragesPerOctave, p->map.data(), &p->span, &p->inc);
    if (p->nAverages <= 0) {
        if (p->nAverages < 0)
            fail(MXG_ERR_INVALID, "mxg_octave_plan_create: nAveragesPerOctave %d at samplingRate %g gives more than %d averages",
                 nAveragesPerOctave, (double)samplingRate, MXG_OCTAVE_MAX_AVERAGES);
        else  // a defined departure: the reference sets up an analyser with no averages at all
            fail(MXG_ERR_INVALID, "mxg_octave_plan_create: nAverages is 0: samplingRate %g / 2 does not pass the first band's 55 Hz",
                 (double)samplingRate);
        delete p;
        return nullptr;
    }
    // The host tables stay valid without a device (mxg_octave_plan_map); compute calls then fail.
    if (ensure_init_only() || check_hip(hipMalloc(&p->d_map, sizeof(int) * (size_t)nSpectrum), "hipMalloc") ||
        check_hip(hipMemcpy(p->d_map, p->map.data(), sizeof(int) * (size_t)nSpectrum, hipMemcpyHostToDevice), "hipMemcpy")) {
        if (p->d_map) (void)hipFree(p->d_map);
        p->d_map = nullptr;
    }
    return p;
}

int mxg_octave_plan_destroy(mxg_octave_plan *plan) {
    if (!plan) return MXG_OK;
    if (plan->d_map) (void)hipFree(plan->d_map);
    delete plan;
    return MXG_OK;
}

int mxg_octave_plan_averages(const mxg_octave_plan *plan) {
    MXG_REQUIRE(plan, "plan is null");
    return plan->nAverages;
}

int mxg_octave_plan_map(const mxg_octave_plan *plan, int *h_spe2avg) {
    MXG_REQUIRE(plan, "plan is null");
    MXG_REQUIRE(h_spe2avg, "h_spe2avg is null");
    memcpy(h_spe2avg, plan->map.data(), sizeof(int) * plan->map.size());
    return MXG_OK;
}

int mxg_octave_batch(const mxg_octave_plan *plan, const float *d_mags, size_t stride, size_t nstreams, size_t frames_per_stream,
                     float eq_intercept, float eq_slope, int peakHoldTime, float peakDecayRate, float *d_averages, float *d_peaks_out,
                     float *d_peak_state, int32_t *d_hold_state, void *stream) {
    MXG_REQUIRE(plan, "plan is null");
    MXG_REQUIRE(d_mags, "d_mags is null");
    MXG_REQUIRE(d_averages, "d_averages is null");
    MXG_REQUIRE(stride >= (size_t)plan->nSpectrum, "stride is below nSpectrum");
    MXG_REQUIRE((d_peak_state == nullptr) == (d_hold_state == nullptr), "d_peak_state and d_hold_state go together (both null: no peak pass)");
    MXG_REQUIRE(!d_peaks_out || d_peak_state, "d_peaks_out needs d_peak_state and d_hold_state");
    MXG_REQUIRE(frames_per_stream == 0 || nstreams <= ((size_t)0x7fffffff * 64) / frames_per_stream, "nstreams * frames_per_stream is beyond 2^37");
    MXG_REQUIRE((nstreams * (size_t)plan->nAverages + 255) / 256 <= 0x7fffffffull, "nstreams is too large");
    if (int s = ensure_init()) return s;
    MXG_REQUIRE(plan->d_map, "plan has no device table (created without a HIP device)");
    const size_t nframes = nstreams * frames_per_stream;
    if (nframes == 0) return MXG_OK;
    const OctArgs A = {d_mags, stride, nframes, plan->nSpectrum, plan->nAverages, plan->d_map, eq_intercept, eq_slope, d_averages};
    const dim3 grid((unsigned)((nframes + 63) / 64)), block(64);
    hipStream_t st = resolve_stream(stream);
    {
        KernelTimer kt("octave_kernel", st);
        if (rows_aligned16(d_mags, stride)) hipLaunchKernelGGL((octave_kernel<true>), grid, block, 0, st, A);
        else hipLaunchKernelGGL((octave_kernel<false>), grid, block, 0, st, A);
        if (int s = check_hip(hipGetLastError(), "octave_kernel launch")) return s;
    }
    if (d_peak_state) {
        const size_t threads = nstreams * (size_t)plan->nAverages;
        KernelTimer kt("octave_peaks_kernel", st);
        hipLaunchKernelGGL(octave_peaks_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, nstreams, frames_per_stream,
                           plan->nAverages, peakHoldTime, peakDecayRate, d_averages, d_peaks_out, d_peak_state, d_hold_state);
        return check_hip(hipGetLastError(), "octave_peaks_kernel launch");
    }
    return MXG_OK;
}

}  // extern "C"
