// reverb.hip -- maxiSatReverb, maxiFreeVerb and maxiFreeVerbStereo voice banks on gfx950 (K13).
//
// Path: reference src/libs/maxiReverb.h / .cpp; the arithmetic, the topology tables and the slot rules are mxg_reverb.h.
// Everything is + - * with contraction off => bit-exact, subnormals included.
//
// Every delay length is a constant of the class, and over a tile of RV_T = 64 samples a ring of D slots that is stepped
// `steps` times per sample sees steps*64 distinct slots whenever steps*64 <= D.  That holds for every comb, for all 31
// allpasses of maxiFreeVerb (the shortest is 65) and for the stereo class's doubly stepped allpasses (128 <= 225); only
// maxiSatReverb's last two allpasses (42, 12) are shorter than a tile.  So a workgroup of 4 wavefronts owns RV_VB = 8
// voices and walks the block in tiles of 64 samples:
//   1. the [N][V] input tile (and the tile's w / cut) goes through LDS to be transposed;
//   2. a wavefront takes one of its two voices at a time with one lane per SAMPLE.  A plain comb is one coalesced read
//      and one coalesced write of <= two contiguous runs of the voice-major ring; the comb sum is ordered per sample and
//      stays in the lane's register; the value then goes through the 3 .. 31 allpass stages in that register, every
//      stage one coalesced read and write.  The ring reads of a batch of stages do not depend on the audio and are
//      requested before the chain starts;
//   3. maxiFreeVerb's low-pass combs: the only recurrence in time is y = y + (1 - cut) * (d - y).  The tile's ring reads
//      d of all 8 voices x 8 combs are left in LDS, the 64 lanes of wavefront 0 each walk one (voice, comb) pair's 64
//      steps there in order (three dependent flops a step), and the comb outputs and ring stores follow with one lane
//      per sample again;
//   4. a ring shorter than the tile (D < 64: 42 and 12) is staged in LDS and the tile goes over it in sub-tiles of D
//      samples, each a parallel pass over distinct slots (rv_sub_len);
//   5. the output tile leaves through LDS as [N][V] rows.
// A ring cell written in tile t and read in tile t+1 belongs to one wavefront and is ordered by the __syncthreads()
// between the tiles (workgroup-scope release / acquire), as in fx.hip.  Ring indices of the tile sit in LDS and are
// advanced once per tile.
// Algorithmic traffic per sample (16 B per ring step + input + output): Sat 128 B, FreeVerb play(x) 208 B,
// play(x, r, a) 640 B, Stereo 280 B.
#include <type_traits>

#include "mxg_common.h"
#include "mxg_reverb.h"

namespace mxg {
namespace {

static_assert(RV_SAT == MXG_REVERB_SAT && RV_FREEVERB == MXG_REVERB_FREEVERB && RV_STEREO == MXG_REVERB_FREEVERB_STEREO, "kinds");
static_assert(RV_PS_ROOM == MXG_REVERB_PS_ROOMSIZE && RV_PS_ABSORB == MXG_REVERB_PS_ABSORBTION, "ps bits");
static_assert(RV_MAX_FILTERS == MXG_REVERB_MAX_FILTERS, "filters");

constexpr int RV_T = 64;                     // samples per tile = lanes of a wavefront
constexpr int RV_VB = 8;                     // voices per workgroup
constexpr int RV_WAVES = 4;                  // wavefronts per workgroup
constexpr int RV_VPW = RV_VB / RV_WAVES;     // voices per wavefront
constexpr int RV_ROWS = 256 / RV_VB;         // tile rows per pass of the whole workgroup
constexpr int RV_APB = 9;                    // allpass stages whose ring reads are in flight together

template <int B, int E, class Fn>
__device__ __forceinline__ void static_for(Fn &&fn) {
    if constexpr (B < E) {
        fn(std::integral_constant<int, B>{});
        static_for<B + 1, E>(fn);
    }
}

// a wavefront's LDS and ring writes visible to its other lanes
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// stages [J0, J1) of the allpass chain for one sample per lane: PASSES values per lane (left, and the stereo class's
// right), all their ring reads requested first
template <int KIND, int J0, int J1>
__device__ __forceinline__ void allpass_stages(double *ring, const int *ix, int lane, bool act, double (&t)[rv_steps(KIND)]) {
    constexpr int P = rv_steps(KIND), NC = rv_ncomb(KIND);
    double d[J1 - J0][P];
    int sl[J1 - J0][P];
    static_for<J0, J1>([&](auto J) {
        constexpr int f = NC + J, D = rv_len(KIND, f), off = rv_off(KIND, f);
        static_assert(P * RV_T <= D, "a tile's slots must be distinct");
        const int i0 = ix[f];
#pragma unroll
        for (int p = 0; p < P; p++) {
            sl[J - J0][p] = off + rv_slot(i0, P * lane + p, D);
            d[J - J0][p] = act ? ring[sl[J - J0][p]] : 0.0;
        }
    });
    static_for<J0, J1>([&](auto J) {
#pragma unroll
        for (int p = 0; p < P; p++) {
            const double s = rv_allpass(d[J - J0][p], t[p]);
            if (act) ring[sl[J - J0][p]] = s;
        }
    });
}

template <int KIND>
__global__ void __launch_bounds__(256) reverb_kernel(RvArgs A) {
    constexpr int T = RV_T, NC = rv_ncomb(KIND), F = rv_nfilt(KIND), S = rv_ring_doubles(KIND), P = rv_steps(KIND);
    constexpr bool LP = KIND == RV_FREEVERB;
    __shared__ double io[P][T][RV_VB + 1];              // input tile, then the output tile(s)
    __shared__ double wt[LP ? T : 1][RV_VB + 1];        // the tile's w and cut per sample
    __shared__ double ct[LP ? T : 1][RV_VB + 1];
    __shared__ double dl[LP ? RV_VB * RV_LP : 1][T + 1];  // ring reads d of the low-pass combs, then their y
    __shared__ int sidx[RV_VB][F];                      // ring indices at the start of the tile
    __shared__ double srt[RV_WAVES][T];                 // Sat: the 42- and the 12-slot ring of the voice in hand

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t V = A.V, N = A.N;
    const size_t v0 = (size_t)blockIdx.x * RV_VB;

    for (int i = tid; i < RV_VB * F; i += 256) {
        const int l = i / F, f = i % F;
        sidx[l][f] = v0 + l < V ? rv_idx_fix(A.idx[(v0 + l) * F + f], rv_len(KIND, f)) : 0;
    }
    // wavefront 0, lane p: the low-pass state of pair (voice p / 8, comb p % 8)
    const bool pair = LP && wave == 0 && v0 + (lane >> 3) < V;
    double y = 0.0;
    if (pair) y = A.lp[(v0 + (lane >> 3)) * RV_LP + (lane & 7)];

    const int col = tid % RV_VB, row0 = tid / RV_VB;
    const bool colv = v0 + col < V;
    const size_t cv = v0 + (colv ? col : 0);
    double w0 = 0.0, c0 = 0.0;  // this column's w, cut where they do not change inside the block
    if (LP && colv) {
        if (!A.mode) {
            w0 = A.wc[cv * 2];
            c0 = A.wc[cv * 2 + 1];
        } else {
            if (!(A.ps & RV_PS_ROOM)) w0 = rv_room_w(A.room[cv]);
            if (!(A.ps & RV_PS_ABSORB)) c0 = rv_clamp01(A.absorb[cv]);
        }
    }
    __syncthreads();

    for (size_t n0 = 0; n0 < N; n0 += T) {
        const int nt = (int)((N - n0) < (size_t)T ? (N - n0) : (size_t)T);
        // 1. the input tile
#pragma unroll
        for (int j = 0; j < T / RV_ROWS; j++) {
            const int row = row0 + j * RV_ROWS;
            const bool in = row < nt && colv;
            const size_t e = (n0 + row) * V + cv;
            io[0][row][col] = in ? A.in[e] : 0.0;
            if constexpr (LP) {
                double w = w0, c = c0;
                if (in && A.mode) {
                    if (A.ps & RV_PS_ROOM) w = rv_room_w(A.room[e]);
                    if (A.ps & RV_PS_ABSORB) c = rv_clamp01(A.absorb[e]);
                }
                wt[row][col] = w;
                ct[row][col] = c;
            }
        }
        __syncthreads();

        const bool lane_in = lane < nt;
        // 3. the low-pass combs' ring reads, then the recurrence
        if constexpr (LP) {
            double d[RV_VPW][NC];
#pragma unroll
            for (int q = 0; q < RV_VPW; q++) {
                const int l = wave * RV_VPW + q;
                const bool act = lane_in && v0 + l < V;
                const double *ring = A.rings + (v0 + (v0 + l < V ? l : 0)) * (size_t)S;
                static_for<0, NC>([&](auto C) {
                    constexpr int D = rv_len(KIND, C), off = rv_off(KIND, C);
                    static_assert(RV_T <= D, "a tile's slots must be distinct");
                    d[q][C] = act ? ring[off + rv_slot(sidx[l][C], lane, D)] : 0.0;
                });
            }
#pragma unroll
            for (int q = 0; q < RV_VPW; q++)
#pragma unroll
                for (int c = 0; c < NC; c++) dl[(wave * RV_VPW + q) * RV_LP + c][lane] = d[q][c];
            __syncthreads();
            if (pair) {
                const int l = lane >> 3;
                for (int i = 0; i < nt; i++) {
                    y = rv_lowpass(y, ct[i][l], dl[lane][i]);
                    dl[lane][i] = y;
                }
            }
            __syncthreads();
        }

        // 2. one lane per sample: comb outputs, comb sum, allpass chain
#pragma unroll
        for (int q = 0; q < RV_VPW; q++) {
            const int l = wave * RV_VPW + q;
            const bool vin = v0 + l < V;  // (wave-uniform)
            const bool act = lane_in && vin;
            double *ring = A.rings + (v0 + (vin ? l : 0)) * (size_t)S;
            const int *ix = sidx[l];
            const double x = io[0][lane][l];
            double acc = 0.0;
            if constexpr (LP) {
                const double w = wt[lane][l];
                static_for<0, NC>([&](auto C) {
                    constexpr int D = rv_len(KIND, C), off = rv_off(KIND, C);
                    const double o = rv_comb_lp(x, w, dl[l * RV_LP + C][lane]);
                    if (act) ring[off + rv_slot(ix[C], lane, D)] = o;
                    acc += o;
                });
            } else {
                double d[NC];
                int sl[NC];
                static_for<0, NC>([&](auto C) {
                    constexpr int D = rv_len(KIND, C), off = rv_off(KIND, C);
                    static_assert(RV_T <= D, "a tile's slots must be distinct");
                    sl[C] = off + rv_slot(ix[C], lane, D);
                    d[C] = act ? ring[sl[C]] : 0.0;
                });
                static_for<0, NC>([&](auto C) {
                    const double o = rv_comb_plain(d[C], x);
                    if (act) ring[sl[C]] = o;
                    acc += o;
                });
            }
            double t[P];
            t[0] = acc;
            if constexpr (P == 2) t[1] = 0.0;
            if constexpr (KIND == RV_SAT) {
                allpass_stages<KIND, 0, 1>(ring, ix, lane, act, t);
                // 4. the two short rings: staged in LDS, sub-tiles of D samples
                constexpr int off1 = rv_off(KIND, NC + 1), D1 = rv_len(KIND, NC + 1), D2 = rv_len(KIND, NC + 2);
                static_assert(D1 + D2 <= RV_T && rv_off(KIND, NC + 2) == off1 + D1, "both short rings fit the staging row");
                double *st = srt[wave];
                if (vin && lane < D1 + D2) st[lane] = ring[off1 + lane];
                wave_sync();
                static_for<1, 3>([&](auto J) {
                    constexpr int D = rv_len(KIND, NC + J), base = J == 1 ? 0 : D1, L = rv_sub_len(D, 1, RV_T);
                    const int i0 = ix[NC + J];
                    const int s = base + (i0 + lane) % D;
                    for (int s0 = 0; s0 < nt; s0 += L) {
                        if (act && lane >= s0 && lane < s0 + L) st[s] = rv_allpass(st[s], t[0]);
                        wave_sync();
                    }
                });
                if (vin && lane < D1 + D2) ring[off1 + lane] = st[lane];
                wave_sync();  // the staging row is free again
            } else {
                allpass_stages<KIND, 0, 4>(ring, ix, lane, act, t);
                if constexpr (KIND == RV_FREEVERB) {
                    if (A.mode) {
                        allpass_stages<KIND, 4, 4 + RV_APB>(ring, ix, lane, act, t);
                        allpass_stages<KIND, 4 + RV_APB, 4 + 2 * RV_APB>(ring, ix, lane, act, t);
                        allpass_stages<KIND, 4 + 2 * RV_APB, 31>(ring, ix, lane, act, t);
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < P; p++) io[p][lane][l] = t[p];
        }
        // the tile's index advance (every read of sidx above is done: the wavefront's own voices only)
        wave_sync();
        {
            const int nrun = KIND == RV_FREEVERB ? (A.mode ? F : NC + 4) : F;
            if (lane < nrun) {
                const int D = rv_len(KIND, lane), k = (lane < NC ? 1 : P) * nt;
#pragma unroll
                for (int q = 0; q < RV_VPW; q++) {
                    int *p = &sidx[wave * RV_VPW + q][lane];
                    *p = rv_idx_after(*p, k, D);
                }
            }
        }
        __syncthreads();

        // 5. the output tile
#pragma unroll
        for (int j = 0; j < T / RV_ROWS; j++) {
            const int row = row0 + j * RV_ROWS;
            if (row < nt && colv) {
#pragma unroll
                for (int p = 0; p < P; p++) A.out[((size_t)p * N + n0 + row) * V + cv] = io[p][row][col];
            }
        }
        __syncthreads();
    }

    for (int i = tid; i < RV_VB * F; i += 256) {
        const int l = i / F, f = i % F;
        if (v0 + l < V) A.idx[(v0 + l) * F + f] = sidx[l][f];
    }
    if (pair) A.lp[(v0 + (lane >> 3)) * RV_LP + (lane & 7)] = y;
    if (LP && A.mode && tid < RV_VB && colv) {  // (tid < RV_VB: col == tid) play(x, r, a) leaves its last w, cut behind
        const size_t e = (N - 1) * V + cv;
        A.wc[cv * 2] = (A.ps & RV_PS_ROOM) ? rv_room_w(A.room[e]) : w0;
        A.wc[cv * 2 + 1] = (A.ps & RV_PS_ABSORB) ? rv_clamp01(A.absorb[e]) : c0;
    }
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_reverb_layout_host(int kind, uint32_t *n_combs, uint32_t *n_allpasses, uint32_t *ring_doubles, uint32_t *lengths,
                           uint32_t *offsets) {
    MXG_REQUIRE(kind == RV_SAT || kind == RV_FREEVERB || kind == RV_STEREO, "unknown kind");
    if (n_combs) *n_combs = (uint32_t)rv_ncomb(kind);
    if (n_allpasses) *n_allpasses = (uint32_t)rv_nap(kind);
    if (ring_doubles) *ring_doubles = (uint32_t)rv_ring_doubles(kind);
    for (int f = 0; f < rv_nfilt(kind); f++) {
        if (lengths) lengths[f] = (uint32_t)rv_len(kind, f);
        if (offsets) offsets[f] = (uint32_t)rv_off(kind, f);
    }
    return MXG_OK;
}

int mxg_reverb_render(int kind, int mode, size_t V, size_t N, const double *d_in, const double *d_roomsize,
                      const double *d_absorbtion, int ps_flags, double *d_rings, int32_t *d_idx, double *d_lp, double *d_wc,
                      double *d_out, void *stream) {
    if (int s = ensure_init()) return s;
    MXG_REQUIRE(kind == RV_SAT || kind == RV_FREEVERB || kind == RV_STEREO, "unknown kind");
    MXG_REQUIRE(mode == MXG_REVERB_PLAY || (mode == MXG_REVERB_PLAY_PARAMS && kind == RV_FREEVERB),
                "mode must be MXG_REVERB_PLAY, or MXG_REVERB_PLAY_PARAMS for MXG_REVERB_FREEVERB");
    MXG_REQUIRE(d_in && d_rings && d_idx && d_out, "null device pointer");
    MXG_REQUIRE(kind != RV_FREEVERB || (d_lp && d_wc), "maxiFreeVerb needs d_lp and d_wc");
    MXG_REQUIRE(mode != MXG_REVERB_PLAY_PARAMS || (d_roomsize && d_absorbtion), "play(x, roomsize, absorbtion) needs both parameters");
    MXG_REQUIRE((ps_flags & ~MXG_REVERB_PS_ALL) == 0, "unknown ps_flags bit");
    if (V == 0 || N == 0) return MXG_OK;
    const RvArgs A = {mode, V, N, d_in, d_roomsize, d_absorbtion, ps_flags, d_rings, d_idx, d_lp, d_wc, d_out};
    hipStream_t st = resolve_stream(stream);
    const dim3 grid((unsigned)((V + RV_VB - 1) / RV_VB));
    if (kind == RV_SAT) {
        KernelTimer kt("reverb_sat_kernel", st);
        hipLaunchKernelGGL(reverb_kernel<RV_SAT>, grid, dim3(256), 0, st, A);
    } else if (kind == RV_FREEVERB) {
        KernelTimer kt("reverb_freeverb_kernel", st);
        hipLaunchKernelGGL(reverb_kernel<RV_FREEVERB>, grid, dim3(256), 0, st, A);
    } else {
        KernelTimer kt("reverb_stereo_kernel", st);
        hipLaunchKernelGGL(reverb_kernel<RV_STEREO>, grid, dim3(256), 0, st, A);
    }
    return check_hip(hipGetLastError(), "reverb_kernel launch");
}

}  // extern "C"
