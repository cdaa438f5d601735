// spectral_bank.hip -- maxiFFTBank / maxiIFFTBank (kernel K29): V streaming maxiFFT objects (L/maxiFFT.cpp:45-91) and V streaming
// maxiIFFT objects (:141-192) over the banks' own blocks, double [N][V], for any split of the samples into calls.
//
// A call is a constant number of launches, whatever V and N, and no host round trip:
//   maxiFFTBank   gather  -> spectral_gather_kernel: [N][V] doubles become per-stream float lines [V][hist + fill + N] (the carried
//                            samples, then (float)d_in[n][v]), 32 x 32 tiles through the LDS so that the read along v and the write
//                            along n are both coalesced; the same pass leaves each stream's new carry behind
//                 frames  -> the transform bodies of mxg_fft_batch (fft.hip), frame f of stream v at line v + f * hop
//   maxiIFFTBank  frames  -> the inverse body of mxg_ifft_batch's two-kernel form, one windowed transform per (stream, point)
//                 overlap -> spectral_ola_kernel: every output sample is ola_value() of its stream (the closed form of the hop
//                            buffer, oldest frame first), transposed through the LDS into [N][V] doubles; the same launch leaves
//                            the V hop buffers as the reference would
//                 held    -> after-FFT rows only: one device copy per block of the last row passed into the held spectrum
// State: maxiFFTBank keeps the last fftSize - hop + fill floats of every stream (two images, read one / write the other) and
// `fill` on the host; maxiIFFTBank keeps buffer[fftSize] per stream (two images), the held spectrum [V][bins] x 2, and `pos` on
// the host.  Both counters depend only on the sequence of N values (mxg_spectral_bank.h).  Streams are independent: no atomics,
// no workgroup waits on another.
#include "mxg_spectral.h"
#include "mxg_spectral_bank.h"

struct mxg_fft_bank {
    size_t V;
    int fftSize, hop, hist, fill;  // hist = windowSize - hopSize with windowSize = fftSize (L/maxiFFT.cpp:48, :55)
    mxg_fft_plan *plan;
    float *d_carry[2];             // [V][fftSize]: the first hist + fill floats of a row are the stream's pending samples
    int cur;
};

struct mxg_ifft_bank {
    size_t V;
    int fftSize, hop, bins, pos;
    mxg_ifft_plan *plan;
    float *d_buf[2];               // [V][fftSize]: member `buffer` of every object
    int cur;
    float *d_heldA, *d_heldB;      // [V][bins]: the spectrum a point takes when its frame came with the call before
};

namespace mxg {
namespace {

constexpr int kTile = 32;

// Line v = [carried samples: hc][(float)in[0..N)[v]], Ls floats apart.  Blocks [0, tilesIn) transpose the input tiles, the blocks
// after them copy the carried samples (one stream, 256 positions each).  Every position at or beyond keep0 = frames * hop is also
// the stream's new carry.  lines == nullptr (a call that completes no frame): only the carry is written.
__global__ __launch_bounds__(256) void spectral_gather_kernel(const double *__restrict__ in, size_t N, size_t V,
                                                              const float *__restrict__ carry_in, float *__restrict__ carry_out,
                                                              size_t cs, size_t hc, size_t keep0, float *__restrict__ lines,
                                                              size_t Ls, size_t tilesV, size_t tilesIn, size_t chunksH) {
    __shared__ float t[kTile][kTile + 1];
    const size_t b = blockIdx.x;
    if (b < tilesIn) {
        const size_t n0 = (b / tilesV) * kTile, v0 = (b % tilesV) * kTile;
        const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
        for (int j = y; j < kTile; j += 8)
            if (n0 + j < N && v0 + x < V) t[j][x] = (float)in[(n0 + j) * V + v0 + x];  // process(float value) narrows its argument
        __syncthreads();
        for (int j = y; j < kTile; j += 8) {
            const size_t v = v0 + j, n = n0 + x;
            if (v < V && n < N) {
                const float val = t[x][j];
                const size_t pos = hc + n;
                if (lines) lines[v * Ls + pos] = val;
                if (pos >= keep0) carry_out[v * cs + (pos - keep0)] = val;
            }
        }
    } else {
        const size_t c = b - tilesIn;
        const size_t v = c / chunksH, pos = (c % chunksH) * 256 + threadIdx.x;
        if (v < V && pos < hc) {
            const float val = carry_in[v * cs + pos];
            if (lines) lines[v * Ls + pos] = val;
            if (pos >= keep0) carry_out[v * cs + (pos - keep0)] = val;
        }
    }
}

// out[n][v] = (double) what maxiIFFT v returns at sample n of a call entered at `pos`: position (pos + n) % hop of its buffer after
// the consumption point before that sample (ola_value; point -1 = the carried buffer).  Blocks [0, tilesOut) cover 32 samples x
// 32 streams: the sums are read along n (consecutive floats of a stream's transforms) and written along v.  The blocks after them
// (C > 0 only) leave buffer v as it stands after the call's last point.
__global__ __launch_bounds__(256) void spectral_ola_kernel(const float *__restrict__ io, size_t C, int n, int hop, int pos,
                                                           const float *__restrict__ buf_in, float *__restrict__ buf_out,
                                                           double *__restrict__ out, size_t N, size_t V, size_t tilesV,
                                                           size_t tilesOut, size_t chunksB) {
    __shared__ float t[kTile][kTile + 1];
    const size_t b = blockIdx.x;
    if (b < tilesOut) {
        const size_t n0 = (b / tilesV) * kTile, v0 = (b % tilesV) * kTile;
        const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
        for (int j = y; j < kTile; j += 8) {
            const size_t v = v0 + j, s = n0 + x;
            if (v < V && s < N) {
                long long k;
                int i;
                spectral_bank_sample(hop, pos, s, &k, &i);
                t[j][x] = ola_value(io + v * C * (size_t)n, buf_in + v * (size_t)n, k, i, n, hop);
            }
        }
        __syncthreads();
        for (int j = y; j < kTile; j += 8)
            if (n0 + j < N && v0 + x < V) out[(n0 + j) * V + v0 + x] = (double)t[x][j];  // each float widened exactly
    } else {
        const size_t c = b - tilesOut;
        const size_t v = c / chunksB;
        const int i = (int)((c % chunksB) * 256 + threadIdx.x);
        if (v < V && i < n)
            buf_out[v * (size_t)n + i] = ola_value(io + v * C * (size_t)n, buf_in + v * (size_t)n, (long long)C - 1, i, n, hop);
    }
}

bool bad_fft_size(int fftSize) { return fftSize < 8 || fftSize > 8192 || (fftSize & (fftSize - 1)); }

}  // namespace
}  // namespace mxg

using namespace mxg;

#define MXG_SB_REFUSE(cond, ...)              \
    do {                                      \
        if (cond) {                           \
            fail(MXG_ERR_INVALID, __VA_ARGS__); \
            return nullptr;                   \
        }                                     \
    } while (0)

extern "C" {

int mxg_spectral_bank_plan_host(int fftSize, int hopSize, int windowSize, int fft_fill, int ifft_pos, size_t N, size_t *frames,
                                size_t *points, int *first_is_held, int *new_fill, int *new_pos) {
    MXG_REQUIRE(!bad_fft_size(fftSize), "fftSize must be a power of two in [8, 8192]");
    MXG_REQUIRE(windowSize >= 0 && windowSize <= fftSize, "windowSize must not exceed fftSize");
    MXG_REQUIRE(hopSize >= 1 && hopSize <= fftSize, "hopSize is outside [1, fftSize]");
    MXG_REQUIRE(fft_fill >= 0 && fft_fill < hopSize, "fft_fill is outside [0, hopSize)");
    MXG_REQUIRE(ifft_pos >= 0 && ifft_pos < hopSize, "ifft_pos is outside [0, hopSize)");
    const SpectralBankPlan p = spectral_bank_plan(hopSize, fft_fill, ifft_pos, N);
    if (frames) *frames = p.frames;
    if (points) *points = p.points;
    if (first_is_held) *first_is_held = p.first_is_held;
    if (new_fill) *new_fill = p.new_fill;
    if (new_pos) *new_pos = p.new_pos;
    return MXG_OK;
}

/* ---- maxiFFTBank -------------------------------------------------------------------------------------------------------- */

int mxg_fft_bank_destroy(mxg_fft_bank *b) {
    if (!b) return MXG_OK;
    if (b->plan) mxg_fft_plan_destroy(b->plan);
    for (float *p : b->d_carry)
        if (p) (void)hipFree(p);
    delete b;
    return MXG_OK;
}

int mxg_fft_bank_reset(mxg_fft_bank *b) {
    MXG_REQUIRE(b, "null object");
    MXG_HIP(hipMemset(b->d_carry[0], 0, sizeof(float) * b->V * (size_t)b->fftSize));  // buffer.resize(fftSize, 0), L/maxiFFT.cpp:51
    b->cur = 0;
    b->fill = 0;  // pos = windowSize - hopSize, :55
    return MXG_OK;
}

mxg_fft_bank *mxg_fft_bank_create(size_t V, int fftSize, int hopSize, int windowSize) {
    // the argument checks come first: a refused call never touches the device
    MXG_SB_REFUSE(V == 0 || V > 0x7fffffffu, "mxg_fft_bank_create: V = %zu streams (1 <= V < 2^31)", V);
    MXG_SB_REFUSE(bad_fft_size(fftSize), "mxg_fft_bank_create: fftSize %d is not a power of two in [8, 8192]", fftSize);
    MXG_SB_REFUSE(windowSize < 0 || windowSize > fftSize,
                  "mxg_fft_bank_create: windowSize %d above fftSize %d overruns the reference's buffers (maxiFFT.cpp:51-58)", windowSize,
                  fftSize);
    MXG_SB_REFUSE(hopSize < 1 || hopSize > fftSize, "mxg_fft_bank_create: hopSize %d is outside [1, fftSize = %d]", hopSize, fftSize);
    if (ensure_init_only()) return nullptr;
    mxg_fft_bank *b = new mxg_fft_bank();
    b->V = V; b->fftSize = fftSize; b->hop = hopSize; b->hist = fftSize - hopSize; b->fill = 0; b->cur = 0;
    b->d_carry[0] = b->d_carry[1] = nullptr;
    b->plan = mxg_fft_plan_create(fftSize, hopSize, windowSize);
    const size_t bytes = sizeof(float) * V * (size_t)fftSize;
    bool ok = b->plan && hipMalloc(&b->d_carry[0], bytes) == hipSuccess && hipMalloc(&b->d_carry[1], bytes) == hipSuccess;
    if (!ok || mxg_fft_bank_reset(b) != MXG_OK) {
        if (!ok && !*mxg_last_error()) fail(MXG_ERR_HIP, "mxg_fft_bank_create: device setup failed");
        mxg_fft_bank_destroy(b);
        return nullptr;
    }
    return b;
}

int mxg_fft_bank_pos(const mxg_fft_bank *b) { return b ? b->fill : MXG_ERR_INVALID; }

int mxg_fft_bank_process(mxg_fft_bank *b, const double *d_in, size_t N, int layout, float *d_real, float *d_imag, float *d_mags,
                         float *d_phases, void *stream) {
    MXG_REQUIRE(b, "null object");
    MXG_REQUIRE(d_in || N == 0, "d_in is null");
    MXG_REQUIRE(d_real || d_imag || d_mags || d_phases, "no output requested: d_real, d_imag, d_mags and d_phases are all null");
    MXG_REQUIRE(layout == 0 || layout == 1, "layout must be 0 (frame-major) or 1 (stream-major)");
    if (N == 0) return MXG_OK;
    if (int s = ensure_init()) return s;
    const SpectralBankPlan pl = spectral_bank_plan(b->hop, b->fill, 0, N);
    const size_t V = b->V, F = pl.frames, hop = (size_t)b->hop;
    MXG_REQUIRE(F == 0 || V * F < ((size_t)1 << 32), "V * frames must be < 2^32 in one call");
    hipStream_t st = resolve_stream(stream);
    const size_t hc = (size_t)(b->hist + b->fill), keep0 = F * hop;
    const size_t Ls = (hc + N + 1) & ~(size_t)1;  // even: a frame of an even hop starts 8-byte aligned
    float *lines = nullptr;
    if (F)
        if (int s = scratch_get(SCR_SPECTRAL_BANK, st, sizeof(float) * V * Ls, (void **)&lines)) return s;
    const size_t tilesV = (V + kTile - 1) / kTile, tilesIn = tilesV * ((N + kTile - 1) / kTile);
    const size_t chunksH = (hc + 255) / 256, blocks = tilesIn + V * chunksH;
    MXG_REQUIRE(blocks <= 0x7fffffffu, "V * N too large for one launch");
    float *cin = b->d_carry[b->cur], *cout = b->d_carry[b->cur ^ 1];
    {
        KernelTimer kt("spectral_gather_kernel", st);
        hipLaunchKernelGGL(spectral_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_in, N, V, cin, cout, (size_t)b->fftSize,
                           hc, keep0, lines, Ls, tilesV, tilesIn, chunksH ? chunksH : 1);
    }
    MXG_HIP(hipGetLastError());
    b->cur ^= 1;
    b->fill = pl.new_fill;
    if (!F) return MXG_OK;
    // row r = f * V + v (layout 0) or v * F + f (layout 1) is the frame at line v + f * hop
    return layout == 0 ? fft_bank_frames(b->plan, lines, V, hop, Ls, V * F, d_real, d_imag, d_mags, d_phases, st)
                       : fft_bank_frames(b->plan, lines, F, Ls, hop, V * F, d_real, d_imag, d_mags, d_phases, st);
}

/* ---- maxiIFFTBank ------------------------------------------------------------------------------------------------------- */

int mxg_ifft_bank_destroy(mxg_ifft_bank *b) {
    if (!b) return MXG_OK;
    if (b->plan) mxg_ifft_plan_destroy(b->plan);
    void *ptrs[] = {b->d_buf[0], b->d_buf[1], b->d_heldA, b->d_heldB};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete b;
    return MXG_OK;
}

int mxg_ifft_bank_reset(mxg_ifft_bank *b) {
    MXG_REQUIRE(b, "null object");
    MXG_HIP(hipMemset(b->d_buf[0], 0, sizeof(float) * b->V * (size_t)b->fftSize));  // buffer.resize(fftSize, 0), L/maxiFFT.cpp:147
    MXG_HIP(hipMemset(b->d_heldA, 0, sizeof(float) * b->V * (size_t)b->bins));      // maxiFFT's magnitudes / phases after setup, :52-54
    MXG_HIP(hipMemset(b->d_heldB, 0, sizeof(float) * b->V * (size_t)b->bins));
    b->cur = 0;
    b->pos = 0;  // :149
    return MXG_OK;
}

mxg_ifft_bank *mxg_ifft_bank_create(size_t V, int fftSize, int hopSize, int windowSize) {
    MXG_SB_REFUSE(V == 0 || V > 0x7fffffffu, "mxg_ifft_bank_create: V = %zu streams (1 <= V < 2^31)", V);
    MXG_SB_REFUSE(bad_fft_size(fftSize), "mxg_ifft_bank_create: fftSize %d is not a power of two in [8, 8192]", fftSize);
    MXG_SB_REFUSE(windowSize < 0 || windowSize == 1 || windowSize > fftSize,
                  "mxg_ifft_bank_create: windowSize %d is neither 0 nor in [2, fftSize = %d] (maxiFFT.cpp:151-152)", windowSize, fftSize);
    MXG_SB_REFUSE(hopSize < 1 || hopSize > fftSize, "mxg_ifft_bank_create: hopSize %d is outside [1, fftSize = %d]", hopSize, fftSize);
    if (ensure_init_only()) return nullptr;
    mxg_ifft_bank *b = new mxg_ifft_bank();
    b->V = V; b->fftSize = fftSize; b->hop = hopSize; b->bins = fftSize / 2; b->pos = 0; b->cur = 0;
    b->d_buf[0] = b->d_buf[1] = b->d_heldA = b->d_heldB = nullptr;
    b->plan = mxg_ifft_plan_create(fftSize, hopSize, windowSize);
    const size_t bytes = sizeof(float) * V * (size_t)fftSize, hbytes = sizeof(float) * V * (size_t)b->bins;
    bool ok = b->plan && hipMalloc(&b->d_buf[0], bytes) == hipSuccess && hipMalloc(&b->d_buf[1], bytes) == hipSuccess &&
              hipMalloc(&b->d_heldA, hbytes) == hipSuccess && hipMalloc(&b->d_heldB, hbytes) == hipSuccess;
    if (!ok || mxg_ifft_bank_reset(b) != MXG_OK) {
        if (!ok && !*mxg_last_error()) fail(MXG_ERR_HIP, "mxg_ifft_bank_create: device setup failed");
        mxg_ifft_bank_destroy(b);
        return nullptr;
    }
    return b;
}

int mxg_ifft_bank_pos(const mxg_ifft_bank *b) { return b ? b->pos : MXG_ERR_INVALID; }

const float *mxg_ifft_bank_buffer(const mxg_ifft_bank *b) { return b ? b->d_buf[b->cur] : nullptr; }

int mxg_ifft_bank_process(mxg_ifft_bank *b, int input, int row_mode, int layout, const float *d_a, const float *d_b, size_t nrows,
                          size_t N, double *d_out, void *stream) {
    MXG_REQUIRE(b, "null object");
    MXG_REQUIRE(input == 0 || input == 1, "input must be 0 (magnitudes, phases) or 1 (real, imag)");
    MXG_REQUIRE(row_mode == 0 || row_mode == 1, "row_mode must be 0 (direct) or 1 (after-FFT)");
    MXG_REQUIRE(layout == 0 || layout == 1, "layout must be 0 (frame-major) or 1 (stream-major)");
    MXG_REQUIRE(d_out || N == 0, "d_out is null");
    MXG_REQUIRE((d_a && d_b) || nrows == 0, "d_a or d_b is null");
    // after-FFT: the rows a maxiFFTBank in lock-step (fill == pos) emitted for the same N
    const SpectralBankPlan pl = spectral_bank_plan(b->hop, b->pos, b->pos, N);
    const size_t C = pl.points, R = row_mode ? pl.frames : pl.points;
    if (nrows != R)
        return fail(MXG_ERR_INVALID, "mxg_ifft_bank_process: nrows = %zu, but N = %zu at pos %d takes %zu rows per stream (%s)", nrows, N,
                    b->pos, R, row_mode ? "the frames a maxiFFTBank of this hop emits for N" : "one per consumption point");
    if (N == 0) return MXG_OK;
    if (int s = ensure_init()) return s;
    hipStream_t st = resolve_stream(stream);
    const size_t V = b->V, n = (size_t)b->fftSize, bins = (size_t)b->bins;
    float *io = nullptr;
    if (C) {
        MXG_REQUIRE(V * C < ((size_t)1 << 32), "V * points must be < 2^32 in one call");
        if (int s = scratch_get(SCR_SPECTRAL_BANK_IO, st, sizeof(float) * V * C * n, (void **)&io)) return s;
        if (int s = ifft_bank_frames(b->plan, input, d_a, d_b, b->d_heldA, b->d_heldB, layout, row_mode, pl.first_is_held, V, C, R, io, st))
            return s;
    }
    const size_t tilesV = (V + kTile - 1) / kTile, tilesOut = tilesV * ((N + kTile - 1) / kTile);
    const size_t chunksB = (n + 255) / 256, blocks = tilesOut + (C ? V * chunksB : 0);
    MXG_REQUIRE(blocks <= 0x7fffffffu, "V * N too large for one launch");
    float *bin = b->d_buf[b->cur], *bout = b->d_buf[b->cur ^ 1];
    {
        KernelTimer kt("spectral_ola_kernel", st);
        hipLaunchKernelGGL(spectral_ola_kernel, dim3((unsigned)blocks), dim3(256), 0, st, io, C, (int)n, b->hop, b->pos, bin, bout, d_out, N,
                           V, tilesV, tilesOut, chunksB);
    }
    MXG_HIP(hipGetLastError());
    if (C) b->cur ^= 1;
    b->pos = pl.new_pos;
    if (row_mode && R) {  // held = the last row passed: what the points of the next call see until its own first frame completes
        if (layout == 0) {
            MXG_HIP(hipMemcpyAsync(b->d_heldA, d_a + (R - 1) * V * bins, sizeof(float) * V * bins, hipMemcpyDeviceToDevice, st));
            MXG_HIP(hipMemcpyAsync(b->d_heldB, d_b + (R - 1) * V * bins, sizeof(float) * V * bins, hipMemcpyDeviceToDevice, st));
        } else {
            MXG_HIP(hipMemcpy2DAsync(b->d_heldA, sizeof(float) * bins, d_a + (R - 1) * bins, sizeof(float) * R * bins, sizeof(float) * bins, V,
                                     hipMemcpyDeviceToDevice, st));
            MXG_HIP(hipMemcpy2DAsync(b->d_heldB, sizeof(float) * bins, d_b + (R - 1) * bins, sizeof(float) * R * bins, sizeof(float) * bins, V,
                                     hipMemcpyDeviceToDevice, st));
        }
    }
    return MXG_OK;
}

}  // extern "C"
