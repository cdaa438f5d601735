// revnet.hip -- maxiReverbNetBank: banks of custom reverbs built from maxiReverbFilters stages on gfx950 (K30).
//
// Path: reference src/libs/maxiReverb.h / .cpp (maxiReverbFilters::combfb, lpcombfb, allpass); the arithmetic, the layout
// rule and the step-by-step walk are mxg_revfilt.h, the slot arithmetic of a time tile is mxg_reverb.h.  Everything is
// + - * with contraction off => bit-exact, subnormals included.
//
// A bank shares one topology: P parallel combs (plain or low-pass, a bit per comb) summed in order, then A serial allpasses,
// 0 <= P, A <= 32.  The delay lengths are run-time values: they travel with the launch as RnLayout (the way dattaro.hip
// takes DtLayout) and are copied to LDS once.  The shape is reverb.hip's: a workgroup of 4 wavefronts owns RN_VB = 8 voices
// and walks the block in tiles of RN_T = 64 samples:
//   1. the [N][V] input tile goes through LDS to be transposed;
//   2. a wavefront takes its two voices with one lane per SAMPLE.  On a ring of D >= 64 slots a tile touches 64 distinct
//      slots: one coalesced read and one coalesced write of <= two contiguous runs.  The comb sum is ordered per sample and
//      stays in the lane's register, as does the value that goes down the allpass chain.  The ring reads of RN_B = 8 stages
//      do not depend on the audio and are requested together;
//   3. the combs go in chunks of RN_C = 8.  A low-pass comb's only recurrence in time is y = y + (1 - cut) * (d - y): the
//      chunk's ring reads d are left in LDS, 16 lanes of the wavefront each walk one (voice, comb) pair's 64 steps there in
//      order, and the comb outputs and ring stores follow with one lane per sample again.  (All its reads precede the tile,
//      which is why the layout rule wants D >= 64 for such a comb.)  Every wavefront walks its own voices' pairs, so the
//      chunk needs wavefront barriers only;
//   4. a ring shorter than the tile (D < 64; plain combs and allpasses) is staged in LDS and the tile goes over it in
//      sub-tiles of rv_sub_len(D, 1, 64) = D samples, each a parallel pass over distinct slots.  D = 1 is 64 ordered passes;
//   5. the output tile leaves through LDS as [N][V] rows.
// A ring cell written in tile t and read in tile t+1 belongs to one wavefront and is ordered by the __syncthreads()
// between the tiles, as in reverb.hip.  Feedbacks and cutoffs are per voice and stage, constant inside a block: LDS.
// LDS per workgroup: 4 608 io + 6 144 parameters + 2 048 y + 2 048 indices + 2 048 staging + 512 lengths and offsets =
// 17 408 B, and 33 280 B of low-pass rows (dynamic) only where the network has a low-pass comb: 50 688 B.  No scratch.
// Algorithmic traffic per sample: 16 B per stage + 8 B in + 8 B out.
#include "mxg_common.h"
#include "mxg_revfilt.h"

namespace mxg {
namespace {

static_assert(RN_MAX == MXG_REVNET_MAX_STAGES, "stages");

constexpr int RN_VB = 8;                  // voices per workgroup
constexpr int RN_WAVES = 4;               // wavefronts per workgroup
constexpr int RN_VPW = RN_VB / RN_WAVES;  // voices per wavefront
constexpr int RN_ROWS = 256 / RN_VB;      // tile rows per pass of the whole workgroup
constexpr int RN_C = 8;                   // combs per chunk
constexpr int RN_B = 8;                   // stages whose ring reads are in flight together
static_assert(RN_VPW * RN_C <= 64 && RN_MAX % RN_C == 0 && RN_C % RN_B == 0, "a chunk's pairs fit a wavefront");

// a wavefront's LDS and ring writes visible to its other lanes
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A ring shorter than the tile, for the voice in hand: staged in `st`, the tile in sub-tiles of D samples.
// COMB: v = x, returns the comb's output; else v = the chain's value in, returns the allpass's output.
template <bool COMB>
__device__ __forceinline__ double short_ring(double *ring, double *st, int D, int i0, double g, double v, int lane, int nt, bool vin,
                                             bool act) {
    if (vin && lane < D) st[lane] = ring[lane];
    wave_sync();
    const int L = rv_sub_len(D, 1, RN_T);
    const int s = (i0 + lane) % D;
    double o = 0.0;
    for (int s0 = 0; s0 < nt; s0 += L) {
        if (act && lane >= s0 && lane < s0 + L) {
            if (COMB) {
                o = rf_combfb(v, g, st[s]);
                st[s] = o;
            } else {
                o = v;
                st[s] = rf_allpass(st[s], g, o);
            }
        }
        wave_sync();
    }
    if (vin && lane < D) ring[lane] = st[lane];
    wave_sync();  // the staging row is free again
    return o;
}

__global__ void __launch_bounds__(256) revnet_kernel(RnArgs A) {
    constexpr int T = RN_T;
    __shared__ double io[T][RN_VB + 1];            // input tile, then the output tile
    extern __shared__ double dlmem[];              // [RN_VB * RN_C][T + 1], only where the network has a low-pass comb
    double(*dl)[T + 1] = reinterpret_cast<double(*)[T + 1]>(dlmem);  // ring reads d of the chunk's low-pass combs, then their y
    __shared__ double sfb[RN_VB][RN_MAX];          // comb feedbacks
    __shared__ double scf[RN_VB][RN_MAX];          // 1 - cutoff of the low-pass combs
    __shared__ double sap[RN_VB][RN_MAX];          // allpass feedbacks
    __shared__ double sy[RN_VB][RN_MAX];           // low-pass states
    __shared__ int sidx[RN_VB][2 * RN_MAX];        // ring indices at the start of the tile
    __shared__ int slen[2 * RN_MAX], soff[2 * RN_MAX];
    __shared__ double srt[RN_WAVES][T];            // the short ring of the voice in hand

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t V = A.V, N = A.N;
    const int P = A.L.P, NA = A.L.A, F = P + NA;
    const size_t S = (size_t)A.L.S;
    const uint32_t lpmask = A.L.lpmask;
    const size_t v0 = (size_t)blockIdx.x * RN_VB;

    if (tid < 2 * RN_MAX) {
        slen[tid] = tid < F ? A.L.len[tid] : 1;
        soff[tid] = tid < F ? A.L.off[tid] : 0;
    }
    __syncthreads();
    for (int i = tid; i < RN_VB * 2 * RN_MAX; i += 256) {
        const int l = i / (2 * RN_MAX), f = i % (2 * RN_MAX);
        sidx[l][f] = f < F && v0 + l < V ? rv_idx_fix(A.idx[(v0 + l) * F + f], slen[f]) : 0;
    }
    {
        const int l = tid / RN_MAX, c = tid % RN_MAX;  // 256 = RN_VB * RN_MAX
        const bool in = v0 + l < V;
        const bool lp = in && c < P && ((lpmask >> c) & 1u);
        sfb[l][c] = in && c < P ? A.comb_fb[(v0 + l) * P + c] : 0.0;
        scf[l][c] = lp ? rf_lp_coef(A.comb_cut[(v0 + l) * P + c]) : 0.0;
        sy[l][c] = lp ? A.lp[(v0 + l) * P + c] : 0.0;
        sap[l][c] = in && c < NA ? A.ap_fb[(v0 + l) * NA + c] : 0.0;
    }
    static_assert(RN_VB * RN_MAX == 256, "one thread per (voice, stage)");

    const int col = tid % RN_VB, row0 = tid / RN_VB;
    const bool colv = v0 + col < V;
    const size_t cv = v0 + (colv ? col : 0);
    __syncthreads();

    for (size_t n0 = 0; n0 < N; n0 += T) {
        const int nt = (int)((N - n0) < (size_t)T ? (N - n0) : (size_t)T);
        // 1. the input tile
#pragma unroll
        for (int j = 0; j < T / RN_ROWS; j++) {
            const int row = row0 + j * RN_ROWS;
            io[row][col] = row < nt && colv ? A.in[(n0 + row) * V + cv] : 0.0;
        }
        __syncthreads();

        const bool lane_in = lane < nt;
        double x[RN_VPW], acc[RN_VPW];
        double *ring[RN_VPW];
        bool vin[RN_VPW], act[RN_VPW];
#pragma unroll
        for (int q = 0; q < RN_VPW; q++) {
            const int l = wave * RN_VPW + q;
            vin[q] = v0 + l < V;  // (wave-uniform)
            act[q] = lane_in && vin[q];
            ring[q] = A.rings + (v0 + (vin[q] ? l : 0)) * S;
            x[q] = io[lane][l];
            acc[q] = 0.0;
        }

        // 2. / 3. the combs, RN_C at a time
        for (int c0 = 0; c0 < P; c0 += RN_C) {
            const uint32_t lpc = (lpmask >> c0) & ((1u << RN_C) - 1u);  // (combs at and beyond P carry no bit)
            if (lpc) {
                double d[RN_VPW][RN_C];  // every read of the chunk is requested before the first one is used
#pragma unroll
                for (int q = 0; q < RN_VPW; q++) {
                    const int l = wave * RN_VPW + q;
#pragma unroll
                    for (int k = 0; k < RN_C; k++) {
                        const int c = c0 + k;  // (< 32; a comb that is plain, or beyond P, reads nothing)
                        const bool on = ((lpc >> k) & 1u) && act[q];
                        d[q][k] = on ? ring[q][soff[c] + rv_slot(sidx[l][c], lane, slen[c])] : 0.0;
                    }
                }
#pragma unroll
                for (int q = 0; q < RN_VPW; q++)
#pragma unroll
                    for (int k = 0; k < RN_C; k++) dl[(wave * RN_VPW + q) * RN_C + k][lane] = d[q][k];
                wave_sync();
                if (lane < RN_VPW * RN_C) {  // lane p: comb c0 + p % 8 of the wavefront's voice p / 8
                    const int l = wave * RN_VPW + lane / RN_C, k = lane % RN_C, c = c0 + k;
                    if (((lpc >> k) & 1u) && v0 + l < V) {
                        double y = sy[l][c];
                        const double coef = scf[l][c];
                        double *row = dl[l * RN_C + k];
                        for (int i = 0; i < nt; i++) {
                            y = rf_lopass(y, coef, row[i]);
                            row[i] = y;
                        }
                        sy[l][c] = y;
                    }
                }
                wave_sync();
            }
#pragma unroll
            for (int q = 0; q < RN_VPW; q++) {
                const int l = wave * RN_VPW + q;
                const int *ix = sidx[l];
#pragma unroll
                for (int b0 = 0; b0 < RN_C; b0 += RN_B) {
                    if (c0 + b0 >= P) break;
                    double d[RN_B];
                    int sl[RN_B];
#pragma unroll
                    for (int k = 0; k < RN_B; k++) {
                        const int c = c0 + b0 + k;
                        const bool direct = c < P && !((lpc >> (b0 + k)) & 1u) && slen[c] >= T;
                        sl[k] = soff[c] + rv_slot(ix[c], lane, slen[c]);  // (c < 64: the tables are padded)
                        d[k] = direct && act[q] ? ring[q][sl[k]] : 0.0;
                    }
#pragma unroll
                    for (int k = 0; k < RN_B; k++) {
                        const int c = c0 + b0 + k;
                        if (c >= P) break;
                        const double g = sfb[l][c];
                        double o;
                        if ((lpc >> (b0 + k)) & 1u) {
                            o = rf_combfb(x[q], g, dl[l * RN_C + b0 + k][lane]);
                            if (act[q]) ring[q][sl[k]] = o;
                        } else if (slen[c] >= T) {
                            o = rf_combfb(x[q], g, d[k]);
                            if (act[q]) ring[q][sl[k]] = o;
                        } else {
                            o = short_ring<true>(ring[q] + soff[c], srt[wave], slen[c], ix[c], g, x[q], lane, nt, vin[q], act[q]);
                        }
                        acc[q] += o;
                    }
                }
            }
            wave_sync();  // the chunk's rows of dl are free again
        }

        // the allpass chain
#pragma unroll
        for (int q = 0; q < RN_VPW; q++) {
            const int l = wave * RN_VPW + q;
            const int *ix = sidx[l];
            double t = P ? acc[q] : x[q];
            for (int j0 = 0; j0 < NA; j0 += RN_B) {
                double d[RN_B];
                int sl[RN_B];
#pragma unroll
                for (int k = 0; k < RN_B; k++) {
                    const int f = P + j0 + k;  // (< 64 + RN_B: read only where j0 + k < NA)
                    const bool in = j0 + k < NA;
                    const int D = in ? slen[f] : 1;
                    sl[k] = in ? soff[f] + rv_slot(ix[f], lane, D) : 0;
                    d[k] = in && D >= T && act[q] ? ring[q][sl[k]] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < RN_B; k++) {
                    if (j0 + k >= NA) break;
                    const int f = P + j0 + k;
                    const double g = sap[l][j0 + k];
                    if (slen[f] >= T) {
                        const double s = rf_allpass(d[k], g, t);
                        if (act[q]) ring[q][sl[k]] = s;
                    } else {
                        t = short_ring<false>(ring[q] + soff[f], srt[wave], slen[f], ix[f], g, t, lane, nt, vin[q], act[q]);
                    }
                }
            }
            io[lane][l] = t;
        }
        // the tile's index advance (every read of sidx above is done: the wavefront's own voices only)
        wave_sync();
        if (lane < F) {
            const int D = slen[lane];
#pragma unroll
            for (int q = 0; q < RN_VPW; q++) {
                int *p = &sidx[wave * RN_VPW + q][lane];
                *p = rv_idx_after(*p, nt, D);
            }
        }
        __syncthreads();

        // 5. the output tile
#pragma unroll
        for (int j = 0; j < T / RN_ROWS; j++) {
            const int row = row0 + j * RN_ROWS;
            if (row < nt && colv) A.out[(n0 + row) * V + cv] = io[row][col];
        }
        __syncthreads();
    }

    for (int i = tid; i < RN_VB * 2 * RN_MAX; i += 256) {
        const int l = i / (2 * RN_MAX), f = i % (2 * RN_MAX);
        if (f < F && v0 + l < V) A.idx[(v0 + l) * F + f] = sidx[l][f];
    }
    {
        const int l = tid / RN_MAX, c = tid % RN_MAX;
        if (v0 + l < V && c < P && ((lpmask >> c) & 1u)) A.lp[(v0 + l) * P + c] = sy[l][c];
    }
}

int revnet_layout(uint32_t P, uint32_t NA, const uint32_t *comb_sizes, const uint32_t *ap_sizes, const uint32_t *comb_lowpass, RnLayout &L) {
    switch (rn_layout(P, NA, comb_sizes, ap_sizes, comb_lowpass, L)) {
        case RN_OK: return MXG_OK;
        case RN_BAD_COUNT:
            return fail(MXG_ERR_INVALID, "reverb network: %u combs and %u allpasses: each count must lie in [0, %d], their sum must be at least 1 "
                        "and a non-empty kind needs its sizes", P, NA, RN_MAX);
        case RN_BAD_LENGTH: return fail(MXG_ERR_INVALID, "reverb network: every delay length must lie in [1, %d] samples", RF_RING);
        default:
            return fail(MXG_ERR_INVALID, "reverb network: a low-pass comb must be at least %d samples long (the tile its recurrence is walked over)",
                        RN_T);
    }
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_revnet_layout_host(uint32_t n_combs, uint32_t n_allpasses, const uint32_t *comb_sizes, const uint32_t *ap_sizes,
                           const uint32_t *comb_lowpass, uint32_t *offsets, uint32_t *ring_doubles) {
    RnLayout L;
    if (int s = revnet_layout(n_combs, n_allpasses, comb_sizes, ap_sizes, comb_lowpass, L)) return s;
    if (offsets)
        for (int f = 0; f < L.P + L.A; f++) offsets[f] = (uint32_t)L.off[f];
    if (ring_doubles) *ring_doubles = (uint32_t)L.S;
    return MXG_OK;
}

int mxg_revnet_render(uint32_t n_combs, uint32_t n_allpasses, const uint32_t *comb_sizes, const uint32_t *ap_sizes,
                      const uint32_t *comb_lowpass, size_t V, size_t N, const double *d_in, const double *d_comb_fb,
                      const double *d_comb_cut, const double *d_ap_fb, double *d_rings, int32_t *d_idx, double *d_lp, double *d_out,
                      void *stream) {
    RnLayout L;
    if (int s = revnet_layout(n_combs, n_allpasses, comb_sizes, ap_sizes, comb_lowpass, L)) return s;
    MXG_REQUIRE(d_in && d_rings && d_idx && d_out, "null device pointer");
    MXG_REQUIRE(!L.P || d_comb_fb, "a network with combs needs d_comb_fb");
    MXG_REQUIRE(!L.A || d_ap_fb, "a network with allpasses needs d_ap_fb");
    MXG_REQUIRE(!L.lpmask || (d_comb_cut && d_lp), "a network with low-pass combs needs d_comb_cut and d_lp");
    if (int s = ensure_init()) return s;
    if (V == 0 || N == 0) return MXG_OK;
    const RnArgs A = {V, N, d_in, d_comb_fb, d_comb_cut, d_ap_fb, d_rings, d_idx, d_lp, d_out, L};
    hipStream_t st = resolve_stream(stream);
    const dim3 grid((unsigned)((V + RN_VB - 1) / RN_VB));
    KernelTimer kt("revnet_kernel", st);
    const size_t lds = L.lpmask ? sizeof(double) * RN_VB * RN_C * (RN_T + 1) : 0;  // the low-pass rows
    hipLaunchKernelGGL(revnet_kernel, grid, dim3(256), lds, st, A);
    return check_hip(hipGetLastError(), "revnet_kernel launch");
}

}  // extern "C"
