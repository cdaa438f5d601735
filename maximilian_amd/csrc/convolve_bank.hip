// convolve_bank.hip -- maxiConvolveBank: V independent maxiConvolve objects (L/maxiConvolve.cpp:13-107) over I <= V shared impulses,
// nblocks * fftsize samples of every stream per call.  Stream v is, bit for bit, an mxg_convolve (convolve.hip) created from impulse
// imp_of[v] and fed stream v's input, for any split of the samples into calls.
//
// A call is a constant number of launches, whatever V:
//   frames  -> mxg_fft_batch over all V * nblocks input frames (hop = fftsize: [V][nblocks * fftsize] IS a batch of frames)
//   sums    -> conv_bank_mac_kernel (K24, mxg_convolve.h): one launch per chunk of up to conv_chunk() = kChunk frames; the new spectra
//              enter each stream's ring of R = max K - 1 + kChunk rows inside that kernel -- nothing is copied to keep the history,
//              the bytes written for state are those of the nblocks new rows.  The ring's head is a word in device memory that a
//              one-lane kernel advances behind each chunk, so that no launch argument depends on how many frames went before: all
//              state of the bank lives on the device, as the single object's does
//   inverse -> mxg_ifft_batch_complex over all V * nblocks rows of sums with d_buffer = NULL: maxiIFFT is set up with hop = fftsize,
//              so its hop buffer is never read back (no frame reaches the next one) and is not state of the bank
// State per stream: the ring, and the pending sums (what output block 0 of the next call is transformed from).
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "mxg_convolve.h"

struct mxg_convolve_bank {
    size_t V, I;
    int fftsize, hopsize, bins, Kmax, R;
    mxg_fft_plan *fplan;
    mxg_ifft_plan *iplan;
    std::vector<std::vector<float>> h_impR, h_impI;  // per impulse [K_i][bins]
    std::vector<int> K;                              // per impulse
    float *d_impR, *d_impI;                          // all impulses back to back
    int *d_K, *d_impRow, *d_order;                   // [V]: frames and first impulse row of a stream; the streams grouped by impulse
    float *d_ringR, *d_ringI;                        // [V][R][bins]
    float *d_pendR, *d_pendI;                        // [V][bins]
    int *d_head;                                     // the ring slot the next frame takes (the same for every stream)
};

namespace mxg {
namespace {

constexpr int kChunk = 16;  // frames per launch of the MAC kernel: the ring holds max K - 1 + kChunk rows per stream

// grid: (lane blocks of a row) x (tiles of the chunk) x (streams, in the order that keeps the streams of one impulse together: its
// rows are then read once from memory and by every later stream from the L2)
__global__ __launch_bounds__(256) void conv_bank_mac_kernel(conv_mac_args g, const int *__restrict__ head, const int *__restrict__ order,
                                                            int pairs, int tiles, int laneBlocks) {
    g.head = *head;
    const unsigned b = blockIdx.x;
    const int lb = (int)(b % (unsigned)laneBlocks);
    const unsigned vt = b / (unsigned)laneBlocks;
    const int tile = (int)(vt % (unsigned)tiles);
    const size_t v = (size_t)order[vt / (unsigned)tiles];
    const int pair = lb * (int)blockDim.x + (int)threadIdx.x;
    if (pair >= pairs) return;
    conv_mac_lane(g, v, tile, pair);
}

// behind a chunk of c frames (stream order: every lane of the chunk's launch has read the head by then)
__global__ void conv_bank_advance_kernel(int *head, int c, int R) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *head = (*head + c) % R;
}

// out[v][n] = (float)in[n][v] and out[n][v] = (double)in[v][n]: 32 x 32 tiles through the LDS, both sides coalesced
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void conv_bank_transpose_kernel(const TI *__restrict__ in, TO *__restrict__ out, size_t rows, size_t cols) {
    __shared__ TO t[32][33];
    const size_t tilesX = (cols + 31) / 32;
    const size_t r0 = (blockIdx.x / tilesX) * 32, c0 = (blockIdx.x % tilesX) * 32;
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    for (int j = y; j < 32; j += 8)
        if (r0 + j < rows && c0 + x < cols) t[j][x] = (TO)in[(r0 + j) * cols + c0 + x];
    __syncthreads();
    for (int j = y; j < 32; j += 8)
        if (c0 + j < cols && r0 + x < rows) out[(c0 + j) * rows + r0 + x] = t[x][j];
}

template <typename TI, typename TO>
int transpose_convert(const TI *in, TO *out, size_t rows, size_t cols, hipStream_t st) {
    const size_t blocks = ((rows + 31) / 32) * ((cols + 31) / 32);
    if (blocks > 0x7fffffffu) return fail(MXG_ERR_INVALID, "mxg_convolve_bank_play_nv: block too large");
    KernelTimer kt("conv_bank_transpose_kernel", st);
    hipLaunchKernelGGL((conv_bank_transpose_kernel<TI, TO>), dim3((unsigned)blocks), dim3(256), 0, st, in, out, rows, cols);
    return check_hip(hipGetLastError(), "conv_bank_transpose_kernel launch");
}

// the call on float [V][nblocks * fftsize]; scr: 4 * V * nblocks * bins floats (the new spectra and the rows of sums, real and imaginary)
int bank_play(mxg_convolve_bank *b, const float *d_in, size_t nblocks, float *d_out, int mode, hipStream_t st, float *scr) {
    const size_t V = b->V, bins = (size_t)b->bins, spec = V * nblocks * bins;
    float *XR = scr, *XI = scr + spec, *SR = scr + 2 * spec, *SI = scr + 3 * spec;
    if (int s = mxg_fft_batch(b->fplan, d_in, (size_t)b->fftsize, V * nblocks, XR, XI, nullptr, nullptr, st)) return s;
    const int pairs = b->bins / kConvBins, threads = pairs >= 256 ? 256 : (pairs > 64 ? pairs : 64);
    const int laneBlocks = (pairs + threads - 1) / threads;
    const size_t cmax = (size_t)conv_chunk(b->R, b->Kmax);
    for (size_t b0 = 0; b0 < nblocks; b0 += cmax) {
        conv_mac_args g;
        g.bins = b->bins; g.R = b->R; g.head = 0;  // (the kernel reads the head from d_head)
        g.c = (int)std::min(cmax, nblocks - b0);
        g.nblocks = nblocks; g.b0 = b0;
        g.K = b->d_K; g.impRow = b->d_impRow; g.impR = b->d_impR; g.impI = b->d_impI;
        g.ringR = b->d_ringR; g.ringI = b->d_ringI; g.pendR = b->d_pendR; g.pendI = b->d_pendI;
        g.XR = XR; g.XI = XI; g.SR = SR; g.SI = SI;
        const int tiles = conv_tiles(g.c);
        const size_t blocks = V * (size_t)tiles * (size_t)laneBlocks;
        MXG_REQUIRE(blocks <= 0x7fffffffu, "V * nblocks too large for one launch");
        {
            KernelTimer kt("conv_bank_mac_kernel", st);
            hipLaunchKernelGGL(conv_bank_mac_kernel, dim3((unsigned)blocks), dim3(threads), 0, st, g, b->d_head, b->d_order, pairs, tiles, laneBlocks);
        }
        MXG_HIP(hipGetLastError());
        hipLaunchKernelGGL(conv_bank_advance_kernel, dim3(1), dim3(64), 0, st, b->d_head, g.c, b->R);
        MXG_HIP(hipGetLastError());
    }
    return mxg_ifft_batch_complex(b->iplan, SR, SI, V * nblocks, mode == 0 ? 1 : 0, nullptr, d_out, nullptr, st);
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_convolve_bank_destroy(mxg_convolve_bank *b) {
    if (!b) return MXG_OK;
    if (b->fplan) mxg_fft_plan_destroy(b->fplan);
    if (b->iplan) mxg_ifft_plan_destroy(b->iplan);
    void *ptrs[] = {b->d_impR, b->d_impI, b->d_K, b->d_impRow, b->d_order, b->d_ringR, b->d_ringI, b->d_pendR, b->d_pendI, b->d_head};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete b;
    return MXG_OK;
}

mxg_convolve_bank *mxg_convolve_bank_create(size_t V, size_t I, const double *const *h_amps, const size_t *h_lens, const double *h_pos0,
                                            const int *h_imp_of, int fftsize, int hopsize) {
    // the argument checks come first: a refused call never touches the device
#define MXG_CB_REFUSE(cond, ...)                  \
    do {                                          \
        if (cond) {                               \
            fail(MXG_ERR_INVALID, __VA_ARGS__);   \
            return nullptr;                       \
        }                                         \
    } while (0)
    MXG_CB_REFUSE(I == 0 || I > V, "mxg_convolve_bank_create: I = %zu impulses for V = %zu streams (1 <= I <= V)", I, V);
    MXG_CB_REFUSE(V > 0x7fffffffu, "mxg_convolve_bank_create: V = %zu streams is too many", V);
    MXG_CB_REFUSE(!h_amps, "mxg_convolve_bank_create: h_amps is null");
    MXG_CB_REFUSE(!h_lens, "mxg_convolve_bank_create: h_lens is null");
    MXG_CB_REFUSE(!h_pos0, "mxg_convolve_bank_create: h_pos0 is null");
    MXG_CB_REFUSE(!h_imp_of, "mxg_convolve_bank_create: h_imp_of is null");
    MXG_CB_REFUSE(fftsize < 8 || fftsize > 8192 || (fftsize & (fftsize - 1)),
                  "mxg_convolve_bank_create: fftsize %d is not a power of two in [8, 8192]", fftsize);
    MXG_CB_REFUSE(hopsize <= 0 || hopsize > fftsize, "mxg_convolve_bank_create: hopsize %d is outside [1, fftsize = %d]", hopsize, fftsize);
    for (size_t i = 0; i < I; i++)
        MXG_CB_REFUSE(!h_amps[i] || h_lens[i] == 0, "mxg_convolve_bank_create: h_amps[%zu] is null or h_lens[%zu] is 0", i, i);
    for (size_t v = 0; v < V; v++)
        MXG_CB_REFUSE(h_imp_of[v] < 0 || (size_t)h_imp_of[v] >= I, "mxg_convolve_bank_create: h_imp_of[%zu] = %d names no impulse (I = %zu)", v,
                      h_imp_of[v], I);
#undef MXG_CB_REFUSE
    if (ensure_init_only()) return nullptr;
    mxg_convolve_bank *b = new mxg_convolve_bank();
    b->V = V; b->I = I; b->fftsize = fftsize; b->hopsize = hopsize; b->bins = fftsize / 2; b->Kmax = 0; b->R = 1;
    b->fplan = nullptr; b->iplan = nullptr;
    b->d_impR = b->d_impI = b->d_ringR = b->d_ringI = b->d_pendR = b->d_pendI = nullptr;
    b->d_K = b->d_impRow = b->d_order = b->d_head = nullptr;
    const int F = fftsize;
    const size_t bins = (size_t)b->bins;
    b->fplan = mxg_fft_plan_create(F, F, hopsize);   // maxiFFT::setup(fftsize, fftsize, hopsize): hop = window = fftsize
    b->iplan = mxg_ifft_plan_create(F, F, hopsize);  // maxiIFFT::setup(fftsize, fftsize, hopsize): Hann over `hopsize`
    bool ok = b->fplan && b->iplan;
    b->h_impR.resize(I); b->h_impI.resize(I); b->K.assign(I, 0);
    std::vector<int> row0(I, 0);
    size_t rows = 0;
    for (size_t i = 0; ok && i < I; i++) {
        ok = convolve_analyse(h_amps[i], h_lens[i], h_pos0[i], b->fplan, b->h_impR[i], b->h_impI[i]);  // as mxg_convolve_create
        b->K[i] = (int)(b->h_impR[i].size() / bins);
        row0[i] = (int)rows;
        rows += (size_t)b->K[i];
        b->Kmax = std::max(b->Kmax, b->K[i]);
    }
    b->R = std::max(b->Kmax, 1) - 1 + kChunk;
    std::vector<int> hK(V), hRow(V), hOrder(V);
    for (size_t v = 0; v < V; v++) {
        hK[v] = b->K[h_imp_of[v]];
        hRow[v] = row0[h_imp_of[v]];
    }
    std::iota(hOrder.begin(), hOrder.end(), 0);
    std::stable_sort(hOrder.begin(), hOrder.end(), [&](int x, int y) { return h_imp_of[x] < h_imp_of[y]; });
    const size_t impBytes = sizeof(float) * (rows ? rows : 1) * bins;
    ok = ok && hipMalloc(&b->d_impR, impBytes) == hipSuccess && hipMalloc(&b->d_impI, impBytes) == hipSuccess;
    ok = ok && hipMalloc(&b->d_K, sizeof(int) * V) == hipSuccess && hipMalloc(&b->d_impRow, sizeof(int) * V) == hipSuccess &&
         hipMalloc(&b->d_order, sizeof(int) * V) == hipSuccess && hipMalloc(&b->d_head, sizeof(int)) == hipSuccess;
    const size_t ringBytes = sizeof(float) * V * (size_t)b->R * bins;
    ok = ok && hipMalloc(&b->d_ringR, ringBytes) == hipSuccess && hipMalloc(&b->d_ringI, ringBytes) == hipSuccess;
    ok = ok && hipMalloc(&b->d_pendR, sizeof(float) * V * bins) == hipSuccess && hipMalloc(&b->d_pendI, sizeof(float) * V * bins) == hipSuccess;
    for (size_t i = 0; ok && i < I; i++)
        if (b->K[i])
            ok = hipMemcpy(b->d_impR + (size_t)row0[i] * bins, b->h_impR[i].data(), sizeof(float) * b->K[i] * bins, hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(b->d_impI + (size_t)row0[i] * bins, b->h_impI[i].data(), sizeof(float) * b->K[i] * bins, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(b->d_K, hK.data(), sizeof(int) * V, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(b->d_impRow, hRow.data(), sizeof(int) * V, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(b->d_order, hOrder.data(), sizeof(int) * V, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok || mxg_convolve_bank_reset(b) != MXG_OK) {
        if (ok == false && !*mxg_last_error()) fail(MXG_ERR_HIP, "mxg_convolve_bank_create: device setup failed");
        mxg_convolve_bank_destroy(b);
        return nullptr;
    }
    return b;
}

int mxg_convolve_bank_reset(mxg_convolve_bank *b) {
    MXG_REQUIRE(b, "null object");
    const size_t bins = (size_t)b->bins;
    MXG_HIP(hipMemset(b->d_ringR, 0, sizeof(float) * b->V * (size_t)b->R * bins));  // FDLs of blank frames, :63-68
    MXG_HIP(hipMemset(b->d_ringI, 0, sizeof(float) * b->V * (size_t)b->R * bins));
    MXG_HIP(hipMemset(b->d_pendR, 0, sizeof(float) * b->V * bins));  // :69-70
    MXG_HIP(hipMemset(b->d_pendI, 0, sizeof(float) * b->V * bins));
    MXG_HIP(hipMemset(b->d_head, 0, sizeof(int)));
    return MXG_OK;
}

int mxg_convolve_bank_frames(const mxg_convolve_bank *b, size_t i) { return (b && i < b->I) ? b->K[i] : 0; }

int mxg_convolve_bank_impulse(const mxg_convolve_bank *b, size_t i, float *h_real, float *h_imag) {
    MXG_REQUIRE(b, "null object");
    MXG_REQUIRE(i < b->I, "no such impulse");
    if (h_real && !b->h_impR[i].empty()) memcpy(h_real, b->h_impR[i].data(), sizeof(float) * b->h_impR[i].size());
    if (h_imag && !b->h_impI[i].empty()) memcpy(h_imag, b->h_impI[i].data(), sizeof(float) * b->h_impI[i].size());
    return MXG_OK;
}

int mxg_convolve_bank_play(mxg_convolve_bank *b, const float *d_in, size_t nblocks, float *d_out, int mode, void *stream) {
    if (int s = ensure_init()) return s;
    MXG_REQUIRE(b && d_in && d_out, "null object or pointer");
    MXG_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (as the reference computes) or 1 (as intended)");
    if (nblocks == 0) return MXG_OK;
    hipStream_t st = resolve_stream(stream);
    float *scr = nullptr;
    if (int s = scratch_get(SCR_CONVOLVE_BANK, st, sizeof(float) * 4 * b->V * nblocks * (size_t)b->bins, (void **)&scr)) return s;
    return bank_play(b, d_in, nblocks, d_out, mode, st, scr);
}

int mxg_convolve_bank_play_nv(mxg_convolve_bank *b, const double *d_in, size_t nblocks, double *d_out, int mode, void *stream) {
    if (int s = ensure_init()) return s;
    MXG_REQUIRE(b && d_in && d_out, "null object or pointer");
    MXG_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (as the reference computes) or 1 (as intended)");
    if (nblocks == 0) return MXG_OK;
    hipStream_t st = resolve_stream(stream);
    const size_t V = b->V, N = nblocks * (size_t)b->fftsize, spec = V * nblocks * (size_t)b->bins;
    float *scr = nullptr;  // the spectra and sums (4 * spec), then the float image of the block [V][N]: input, overwritten by the output
    if (int s = scratch_get(SCR_CONVOLVE_BANK, st, sizeof(float) * (4 * spec + 2 * V * N), (void **)&scr)) return s;
    float *fin = scr + 4 * spec, *fout = fin + V * N;
    if (int s = transpose_convert<double, float>(d_in, fin, N, V, st)) return s;  // (float)w, as play(float w) narrows its argument
    if (int s = bank_play(b, fin, nblocks, fout, mode, st, scr)) return s;
    return transpose_convert<float, double>(fout, d_out, V, N, st);
}

int mxg_convolve_bank_mac_host(size_t V, int bins, int R, const int *h_K, const int *h_imp_row, const float *h_impR, const float *h_impI,
                               float *h_ringR, float *h_ringI, int *h_head, float *h_pendR, float *h_pendI, const float *h_XR,
                               const float *h_XI, size_t nblocks, float *h_SR, float *h_SI) {
    MXG_REQUIRE(h_K && h_imp_row && h_impR && h_impI && h_ringR && h_ringI && h_head && h_pendR && h_pendI, "null state pointer");
    MXG_REQUIRE((h_XR && h_XI && h_SR && h_SI) || nblocks == 0, "null spectra or sums");
    MXG_REQUIRE(bins >= 4 && !(bins & (bins - 1)), "bins must be a power of two >= 4");
    int Kmax = 0;
    for (size_t v = 0; v < V; v++) {
        MXG_REQUIRE(h_K[v] >= 0 && h_imp_row[v] >= 0, "negative frame count or impulse row");
        Kmax = std::max(Kmax, h_K[v]);
    }
    MXG_REQUIRE(R >= 1 && R >= Kmax, "the ring must hold max K frames");
    MXG_REQUIRE(*h_head >= 0 && *h_head < R, "head outside the ring");
    const size_t cmax = (size_t)conv_chunk(R, Kmax);
    for (size_t b0 = 0; b0 < nblocks; b0 += cmax) {  // the chunks, tiles and lanes of bank_play()'s launches
        conv_mac_args g;
        g.bins = bins; g.R = R; g.head = *h_head;
        g.c = (int)std::min(cmax, nblocks - b0);
        g.nblocks = nblocks; g.b0 = b0;
        g.K = h_K; g.impRow = h_imp_row; g.impR = h_impR; g.impI = h_impI;
        g.ringR = h_ringR; g.ringI = h_ringI; g.pendR = h_pendR; g.pendI = h_pendI;
        g.XR = h_XR; g.XI = h_XI; g.SR = h_SR; g.SI = h_SI;
        for (size_t v = 0; v < V; v++)
            for (int tile = 0; tile < conv_tiles(g.c); tile++)
                for (int pair = 0; pair < bins / kConvBins; pair++) conv_mac_lane(g, v, tile, pair);
        *h_head = (*h_head + g.c) % R;
    }
    return MXG_OK;
}

}  // extern "C"
