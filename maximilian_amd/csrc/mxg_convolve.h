// mxg_convolve.h -- what convolve.hip (one maxiConvolve) and convolve_bank.hip (a bank of them, kernel K24) share:
//   * convolve_analyse(): maxiConvolve::setup's analysis of one impulse (L/maxiConvolve.cpp:13-52), used by both create functions
//   * conv_mac_lane():    the work of ONE lane of the bank's multiply-accumulate kernel -- the arithmetic of :86-97 and the ring
//                         indexing -- callable from the kernel and from the host (mxg_convolve_bank_mac_host runs the same text)
#pragma once
#include <vector>

#include "mxg_hd.h"
#include "mxg_spectral.h"

namespace mxg {
namespace {

// maxiConvolve::setup(impulse, fftsize, hopsize) for one impulse: the float stream setup() feeds its maxiFFT -- impulse.play() x len
// (C:740-747), then the zero padding (:41-45) -- transformed on the device (mxg_fft_batch, bit-exact) and divided by the largest
// positive real / imaginary value (:47-52; a zero maximum divides by zero there too).  impR / impI receive [frames][bins];
// frames may be 0 (an impulse shorter than one frame).  false = a device call failed.
inline bool convolve_analyse(const double *h_amp, size_t len, double position0, const mxg_fft_plan *fplan, std::vector<float> &impR,
                             std::vector<float> &impI) {
    const int F = fplan->fftSize, bins = F / 2;
    const size_t total = len + (size_t)(bins - (int)(len % (size_t)bins));
    std::vector<float> seq(total, 0.0f);
    double position = position0;
    for (size_t s = 0; s < len; s++) {
        const long idx = (long)position;
        seq[s] = (idx >= 0 && (size_t)idx < len) ? (float)h_amp[idx] : 0.0f;  // amplitudes[size] and beyond: the guard zero
        position++;
        if ((long)position >= (long)len) position = 0;
    }
    const size_t nfr = total / (size_t)F;
    impR.assign(nfr * bins, 0.0f);
    impI.assign(nfr * bins, 0.0f);
    if (!nfr) return true;
    const size_t specBytes = sizeof(float) * nfr * bins;
    float *d_seq = nullptr, *d_r = nullptr, *d_i = nullptr;
    bool ok = hipMalloc(&d_seq, sizeof(float) * total) == hipSuccess && hipMalloc(&d_r, specBytes) == hipSuccess &&
              hipMalloc(&d_i, specBytes) == hipSuccess;
    ok = ok && hipMemcpy(d_seq, seq.data(), sizeof(float) * total, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && mxg_fft_batch(fplan, d_seq, (size_t)F, nfr, d_r, d_i, nullptr, nullptr, nullptr) == MXG_OK;
    ok = ok && mxg_stream_sync(nullptr) == MXG_OK;
    ok = ok && hipMemcpy(impR.data(), d_r, specBytes, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(impI.data(), d_i, specBytes, hipMemcpyDeviceToHost) == hipSuccess;
    for (float *p : {d_seq, d_r, d_i})
        if (p) (void)hipFree(p);
    if (!ok) return false;
    float maxReal = 0, maxImag = 0;  // :17-18, :25-32
    for (float v : impR)
        if (v > maxReal) maxReal = v;
    for (float v : impI)
        if (v > maxImag) maxImag = v;
    for (float &v : impR) v /= maxReal;  // :47-52
    for (float &v : impI) v /= maxImag;
    return true;
}

// ---- K24: the multiply-accumulate over a bank of frequency delay lines -----------------------------------------------------------
// Stream v keeps its input spectra in a ring of R rows (ringR / ringI [V][R][bins]); the frame that entered n frames ago sits in slot
// (head - 1 - n) mod R, `head` being the slot the next frame takes.  One launch covers a chunk of c new frames (their spectra in
// XR / XI [V][nblocks][bins] from row b0 on) and forms, for each,
//     S[m][i] = sum_{k < K} imp[k][i] (x) frame[m - k][i]      float, k ascending, nothing contracted (L/maxiConvolve.cpp:86-97)
// A lane owns kConvBins neighbouring bins of kConvM consecutive output frames m0 .. m0 + kConvM - 1 of one stream.  It walks the frames
// from the NEWEST one its tile needs (m0 + kConvM - 1) to the oldest (m0 - K + 1): the frame read at step j is term k = a - (kConvM - 1) + j
// of accumulator a, so every accumulator receives its terms in ascending k while each row of the history is read once per tile --
// K + kConvM - 1 rows instead of K * kConvM -- and the impulse rows slide through a window of kConvM registers per bin.  A term with
// k outside [0, K) is not formed at all (a zero row would still turn an Inf into a NaN, and + 0 loses the sign of a -0 sum).
// Frames >= 0 come from X, older ones from the ring; the tile that owns a new frame also stores it into its ring slot, which no lane
// reads in the same launch as long as c <= R - max(K, 1) + 1: conv_chunk() is that bound, the entry points split a call by it.
// Output block b of a call is transformed from the sums of frame b - 1: the sums of frame m go to SR / SI [V][nblocks] row b0 + m + 1,
// those of the call's last frame to pendR / pendI [V][bins], and the lanes of the chunk's LAST tile first move the carried pend row
// to row 0 when the chunk opens the call -- the lane that reads pend is the one that overwrites it.
constexpr int kConvM = 4;     // output frames per lane
constexpr int kConvBins = 2;  // bins per lane: one 8-byte access per row and plane (bins is a power of two >= 4)

typedef float conv_v2 __attribute__((ext_vector_type(2)));

struct conv_mac_args {
    int bins, R, head;    // head: ring slot of the chunk's frame 0
    int c;                // frames in this chunk (1 <= c <= conv_chunk)
    size_t nblocks, b0;   // frames in the whole call, first frame of the chunk
    const int *K;         // [V] impulse frames of the stream
    const int *impRow;    // [V] first row of the stream's impulse in impR / impI
    const float *impR, *impI;
    float *ringR, *ringI;
    float *pendR, *pendI;
    const float *XR, *XI;
    float *SR, *SI;
};

MXG_HD int conv_chunk(int R, int Kmax) { return R - (Kmax > 1 ? Kmax : 1) + 1; }  // frames per launch
MXG_HD int conv_tiles(int c) { return (c + kConvM - 1) / kConvM; }
MXG_HD conv_v2 conv_ld(const float *p) { return *reinterpret_cast<const conv_v2 *>(p); }
MXG_HD void conv_st(float *p, const conv_v2 v) { *reinterpret_cast<conv_v2 *>(p) = v; }

// lane `pair` (bins kConvBins * pair ...) of tile `tile` of stream v
MXG_HD void conv_mac_lane(const conv_mac_args &g, size_t v, int tile, int pair) {
    constexpr int M = kConvM;
    const int bins = g.bins, i0 = pair * kConvBins;
    const int K = g.K[v], m0 = tile * M;
    const float *iR = g.impR + (size_t)g.impRow[v] * bins + i0, *iI = g.impI + (size_t)g.impRow[v] * bins + i0;
    float *rR = g.ringR + v * (size_t)g.R * bins + i0, *rI = g.ringI + v * (size_t)g.R * bins + i0;
    const float *xR = g.XR + (v * g.nblocks + g.b0) * bins + i0, *xI = g.XI + (v * g.nblocks + g.b0) * bins + i0;
    float *sR = g.SR + v * g.nblocks * bins + i0, *sI = g.SI + v * g.nblocks * bins + i0;
    float *pR = g.pendR + v * (size_t)bins + i0, *pI = g.pendI + v * (size_t)bins + i0;
    const bool lastTile = tile == conv_tiles(g.c) - 1;
    if (g.b0 == 0 && lastTile) {  // the carried sums: what output block 0 is transformed from
        conv_st(sR, conv_ld(pR));
        conv_st(sI, conv_ld(pI));
    }
    const bool bin0 = i0 == 0;  // element .x of this lane is bin 0: real * real, imag * imag (:93-94)
    conv_v2 accR[M], accI[M], wR[M], wI[M];
#pragma unroll
    for (int a = 0; a < M; a++) accR[a] = accI[a] = wR[a] = wI[a] = conv_v2{0.0f, 0.0f};  // std::fill(sumReal ...), :86-87
    const int steps = K ? K + M - 1 : 0;
    conv_v2 fR = {0.0f, 0.0f}, fI = {0.0f, 0.0f}, nR = fR, nI = fI, jR = fR, jI = fI, njR = fR, njI = fI;
    // the rows of step j: frame f = m0 + M - 1 - j (beyond the chunk in a ragged last tile: not read, it feeds no stored sum) and
    // impulse row j
#define MXG_CONV_FETCH(j, FR, FI, JR, JI)                                                  \
    do {                                                                                   \
        const int f_ = m0 + M - 1 - (j);                                                   \
        if (f_ >= 0) {                                                                     \
            if (f_ < g.c) {                                                                \
                FR = conv_ld(xR + (size_t)f_ * bins);                                      \
                FI = conv_ld(xI + (size_t)f_ * bins);                                      \
                if (f_ >= m0) { /* a frame of this tile: it enters the ring here */        \
                    int s_ = g.head + f_;                                                  \
                    if (s_ >= g.R) s_ -= g.R;                                              \
                    conv_st(rR + (size_t)s_ * bins, FR);                                   \
                    conv_st(rI + (size_t)s_ * bins, FI);                                   \
                }                                                                          \
            }                                                                              \
        } else {                                                                           \
            int s_ = g.head + f_;                                                          \
            if (s_ < 0) s_ += g.R;                                                         \
            FR = conv_ld(rR + (size_t)s_ * bins);                                          \
            FI = conv_ld(rI + (size_t)s_ * bins);                                          \
        }                                                                                  \
        if ((j) < K) {                                                                     \
            JR = conv_ld(iR + (size_t)(j) * bins);                                         \
            JI = conv_ld(iI + (size_t)(j) * bins);                                         \
        }                                                                                  \
    } while (0)
    if (steps) MXG_CONV_FETCH(0, nR, nI, njR, njI);
    for (int j = 0; j < steps; j++) {
        fR = nR; fI = nI; jR = njR; jI = njI;
        if (j + 1 < steps) MXG_CONV_FETCH(j + 1, nR, nI, njR, njI);  // the next step's rows are under way during this step's arithmetic
#pragma unroll
        for (int a = 0; a + 1 < M; a++) {
            wR[a] = wR[a + 1];
            wI[a] = wI[a + 1];
        }
        wR[M - 1] = jR;
        wI[M - 1] = jI;
#pragma unroll
        for (int a = 0; a < M; a++) {
            const int k = j - (M - 1) + a;  // the same in every lane of the tile
            if (k >= 0 && k < K) {
                const conv_v2 rr = wR[a] * fR, ii = wI[a] * fI, ri = wR[a] * fI, ir = wI[a] * fR;
                conv_v2 tr = rr - ii, ti = ri + ir;  // :96-97
                if (bin0) {                          // :93-94, a select of the result
                    tr.x = rr.x;
                    ti.x = ii.x;
                }
                accR[a] += tr;
                accI[a] += ti;
            }
        }
    }
#undef MXG_CONV_FETCH
#pragma unroll
    for (int a = 0; a < M; a++) {
        if (m0 + a < g.c) {
            const size_t row = g.b0 + (size_t)(m0 + a) + 1;
            if (row < g.nblocks) {
                conv_st(sR + row * bins, accR[a]);
                conv_st(sI + row * bins, accI[a]);
            } else {  // the call's last frame: carried to the next call
                conv_st(pR, accR[a]);
                conv_st(pI, accI[a]);
            }
        }
    }
}

}  // namespace
}  // namespace mxg
