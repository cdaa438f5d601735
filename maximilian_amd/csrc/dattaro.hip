// dattaro.hip -- maxiDattaroReverb voice banks on gfx950 (K14).
//
// Path: reference src/libs/maxiReverb.h / .cpp (maxiDattaroReverb); the arithmetic, the lengths, the ring order and the tile
// rule are mxg_dattaro.h.  Everything is + - * with contraction off => bit-exact, subnormals included.
//
// The delay lengths follow the sample rate, so they are run-time values (kernel arguments, DtLayout); what is known is
// the rule that admitted the rate (dt_accepts): over a tile of DT_T = 64 samples every one of the eight tank rings sees 64
// distinct slots, and every tap reads either the sample's own write or something written before the tile.  As in
// reverb.hip a workgroup of 4 wavefronts owns DT_VB = 8 voices and walks the block in tiles of 64 samples:
//   1. the [N][V] input tile goes to LDS transposed; each wavefront adds, for its two voices, the tile's reads of the
//      delays D0 and D2 (what their onetap returns: the inputs of the low-passes lp1 and lp2);
//   2. the three low-passes are the only sample-to-sample recurrences: 24 lanes of wavefront 0, one per (voice, filter),
//      walk their 64 steps in LDS in order;
//   3. a wavefront takes one of its voices at a time with one lane per SAMPLE.
//      Input section: the allpasses AP0, AP1 are stepped twice a sample (0.75 then 0.625).  Where 2*64 <= D1 (above about
//      36 kHz) the 4 x 64 slots are distinct and the lane does its four read-modify-writes on the ring directly.
//      Otherwise (kernel variant SUB) both rings are staged whole in LDS (D0 + D1 <= DT_STAGE) and the tile goes over
//      them in sub-tiles of dt_in_sub_len = min(D0, D1) / 2 samples, each a parallel pass over distinct slots.
//      Tank: the old contents of the eight rings' slots and all fourteen taps are read first, then, after a wavefront
//      fence, the slots are written.  A tap's slot may be overwritten later in the same tile (positions below 64 at the
//      low rates), so every tap read precedes every write; a tap at distance 0 takes the lane's own value from its
//      register.  sigl / sigr of the previous sample are the previous lane's D1 / D3 reads (a lane shuffle); lane 0 takes
//      the carried state;
//   4. the two output tiles leave through LDS as [N][V] rows.
// A ring cell written in tile t and read in tile t+1 belongs to one wavefront and is ordered by the __syncthreads()
// between the tiles, as in reverb.hip.  No scratch.
// Algorithmic traffic per sample: 12 ring steps (2 x 2 input, 8 tank) x 16 B + 14 taps x 8 B + 8 B in + 16 B out = 328 B.
#include <type_traits>

#include "mxg_common.h"
#include "mxg_dattaro.h"

namespace mxg {
namespace {

static_assert(DT_RINGS == MXG_DATTARO_RINGS && DT_TAPS == MXG_DATTARO_TAPS && DT_STATE == MXG_DATTARO_STATE, "sizes");

constexpr int DT_T = 64;                  // samples per tile = lanes of a wavefront
constexpr int DT_VB = 8;                  // voices per workgroup
constexpr int DT_WAVES = 4;               // wavefronts per workgroup
constexpr int DT_VPW = DT_VB / DT_WAVES;  // voices per wavefront
constexpr int DT_ROWS = 256 / DT_VB;      // tile rows per pass of the whole workgroup
constexpr int DT_STAGE = 320;             // LDS slots for AP0 + AP1 where AP1 is shorter than 2 * DT_T (then D0 + D1 <= 296)

template <int B, int E, class Fn>
__device__ __forceinline__ void static_for(Fn &&fn) {
    if constexpr (B < E) {
        fn(std::integral_constant<int, B>{});
        static_for<B + 1, E>(fn);
    }
}

// a wavefront's LDS and ring accesses ordered against its other lanes'
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool SUB>
__global__ void __launch_bounds__(256) dattaro_kernel(DtArgs A) {
    constexpr int T = DT_T;
    __shared__ double io[2][T][DT_VB + 1];                     // the output tiles
    __shared__ double dl[DT_VB * 3][T + 1];                    // per (voice, low-pass): its inputs, then its outputs
    __shared__ int sidx[DT_VB][DT_RINGS];                      // ring indices at the start of the tile
    __shared__ double sig[DT_VB][2];                           // sigl, sigr at the start of the tile
    __shared__ int slen[DT_RINGS];
    __shared__ double stg[SUB ? DT_WAVES : 1][SUB ? DT_STAGE : 1];  // AP0 | AP1 of the voice in hand

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t V = A.V, N = A.N, S = (size_t)A.L.S;
    const size_t v0 = (size_t)blockIdx.x * DT_VB;
    const DtLayout &L = A.L;

    if (tid == 0) static_for<0, DT_RINGS>([&](auto R) { slen[R] = L.len[R]; });
    __syncthreads();
    if (tid < DT_VB * DT_RINGS) {
        const int l = tid / DT_RINGS, r = tid % DT_RINGS;
        sidx[l][r] = v0 + l < V ? dt_idx_fix(A.idx[(v0 + l) * DT_RINGS + r], slen[r]) : 0;
    }
    if (tid < DT_VB * 2) {
        const int l = tid >> 1;
        sig[l][tid & 1] = v0 + l < V ? A.state[(v0 + l) * DT_STATE + DT_SIGL + (tid & 1)] : 0.0;
    }
    // wavefront 0, lane p < 24: low-pass p % 3 of voice p / 3
    const bool pair = wave == 0 && lane < DT_VB * 3 && v0 + lane / 3 < V;
    const double lpc = lane % 3 == 0 ? 0.8 : 0.4;
    double y = 0.0;
    if (pair) y = A.state[(v0 + lane / 3) * DT_STATE + lane % 3];

    const int col = tid % DT_VB, row0 = tid / DT_VB;
    const bool colv = v0 + col < V;
    const size_t cv = v0 + (colv ? col : 0);
    __syncthreads();

    for (size_t n0 = 0; n0 < N; n0 += T) {
        const int nt = (int)((N - n0) < (size_t)T ? (N - n0) : (size_t)T);
        const bool lane_in = lane < nt;
        // 1. the input tile, and the reads of D0 and D2
#pragma unroll
        for (int j = 0; j < T / DT_ROWS; j++) {
            const int row = row0 + j * DT_ROWS;
            dl[col * 3][row] = row < nt && colv ? A.in[(n0 + row) * V + cv] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < DT_VPW; q++) {
            const int l = wave * DT_VPW + q;
            const bool act = lane_in && v0 + l < V;
            const double *ring = A.rings + (v0 + (v0 + l < V ? l : 0)) * S;
            dl[l * 3 + 1][lane] = act ? ring[L.off[DT_D0] + dt_slot(sidx[l][DT_D0], lane, L.len[DT_D0])] : 0.0;
            dl[l * 3 + 2][lane] = act ? ring[L.off[DT_D2] + dt_slot(sidx[l][DT_D2], lane, L.len[DT_D2])] : 0.0;
        }
        __syncthreads();
        // 2. the low-passes
        if (pair) {
            for (int i = 0; i < nt; i++) {
                y = dt_lopass(y, lpc, dl[lane][i]);
                dl[lane][i] = y;
            }
        }
        __syncthreads();

        // 3. one lane per sample
#pragma unroll
        for (int q = 0; q < DT_VPW; q++) {
            const int l = wave * DT_VPW + q;
            const bool vin = v0 + l < V;  // (wave-uniform)
            const bool act = lane_in && vin;
            double *ring = A.rings + (v0 + (vin ? l : 0)) * S;
            const int *ix = sidx[l];

            // the tank's ring reads and the taps: before any write of the tile
            int sl[DT_RINGS];
            double old[DT_RINGS];
            static_for<2, DT_RINGS>([&](auto R) {
                sl[R] = L.off[R] + dt_slot(ix[R], lane, L.len[R]);
                old[R] = (R == DT_D0 || R == DT_D2) ? 0.0 : act ? ring[sl[R]] : 0.0;  // (D0, D2: read in step 1)
            });
            double tp[DT_TAPS];
            static_for<0, DT_TAPS>([&](auto J) {
                constexpr int R = dt_tap_ring(J);
                tp[J] = act ? ring[L.off[R] + dt_tap_slot(ix[R], lane, L.tap[J], L.len[R])] : 0.0;
            });

            // the input section: b -> d
            double d = dl[l * 3][lane];
            const int D0 = L.len[DT_AP0], D1 = L.len[DT_AP1];
            if constexpr (!SUB) {
                const int a0 = L.off[DT_AP0] + dt_slot(ix[DT_AP0], 2 * lane, D0), a1 = L.off[DT_AP0] + dt_slot(ix[DT_AP0], 2 * lane + 1, D0);
                const int b0 = L.off[DT_AP1] + dt_slot(ix[DT_AP1], 2 * lane, D1), b1 = L.off[DT_AP1] + dt_slot(ix[DT_AP1], 2 * lane + 1, D1);
                const double ra0 = act ? ring[a0] : 0.0, ra1 = act ? ring[a1] : 0.0, rb0 = act ? ring[b0] : 0.0, rb1 = act ? ring[b1] : 0.0;
                const double wa0 = dt_allpass(ra0, d, 0.75);
                const double wb0 = dt_allpass(rb0, d, 0.75);
                const double wa1 = dt_allpass(ra1, d, 0.625);
                const double wb1 = dt_allpass(rb1, d, 0.625);
                wave_sync();  // every read of the tile is done
                if (act) {
                    ring[a0] = wa0;
                    ring[a1] = wa1;
                    ring[b0] = wb0;
                    ring[b1] = wb1;
                }
            } else {
                double *st = stg[wave];
                const int DD = D0 + D1;  // (AP1 follows AP0 in the ring area, which starts with AP0)
                if (vin)
                    for (int j = lane; j < DD; j += 64) st[j] = ring[j];
                wave_sync();
                const int Ls = dt_in_sub_len(D0, D1, T);
                const int a0 = (ix[DT_AP0] + 2 * lane) % D0, a1 = (ix[DT_AP0] + 2 * lane + 1) % D0;
                const int b0 = D0 + (ix[DT_AP1] + 2 * lane) % D1, b1 = D0 + (ix[DT_AP1] + 2 * lane + 1) % D1;
                for (int s0 = 0; s0 < nt; s0 += Ls) {
                    if (act && lane >= s0 && lane < s0 + Ls) {
                        st[a0] = dt_allpass(st[a0], d, 0.75);
                        st[b0] = dt_allpass(st[b0], d, 0.75);
                        st[a1] = dt_allpass(st[a1], d, 0.625);
                        st[b1] = dt_allpass(st[b1], d, 0.625);
                    }
                    wave_sync();
                }
                if (vin)
                    for (int j = lane; j < DD; j += 64) ring[j] = st[j];
                wave_sync();  // the staging row is free again; every read of the tile is done
            }

            // the tank
            double pl = __shfl_up(old[DT_D1], 1), pr = __shfl_up(old[DT_D3], 1);
            if (lane == 0) {
                pl = sig[l][0];
                pr = sig[l][1];
            }
            double wr[DT_RINGS];  // what each ring's slot gets
            double tl = dt_cross(d, pr), tr = dt_cross(d, pl);
            wr[DT_AP4] = dt_allpass(old[DT_AP4], tl, 0.7);
            wr[DT_D0] = tl;
            tl = dl[l * 3 + 1][lane];
            wr[DT_AP5] = dt_allpass(old[DT_AP5], tl, 0.5);
            wr[DT_D1] = tl;
            wr[DT_AP6] = dt_allpass(old[DT_AP6], tr, 0.7);
            wr[DT_D2] = tr;
            tr = dl[l * 3 + 2][lane];
            wr[DT_AP7] = dt_allpass(old[DT_AP7], tr, 0.5);
            wr[DT_D3] = tr;
            if (act) static_for<2, DT_RINGS>([&](auto R) { ring[sl[R]] = wr[R]; });
            static_for<0, DT_TAPS>([&](auto J) {
                constexpr int R = dt_tap_ring(J);
                if (dt_tap_dist(L.len[R], L.tap[J]) == 0) tp[J] = wr[R];
            });
            io[0][lane][l] = dt_mix(tp[0], tp[1], tp[2], tp[3], tp[4], tp[5], tp[6]);
            io[1][lane][l] = dt_mix(tp[7], tp[8], tp[9], tp[10], tp[11], tp[12], tp[13]);
            if (act && lane == nt - 1) {  // (lane 0 has read the old pair: the same wavefront, in order)
                sig[l][0] = old[DT_D1];
                sig[l][1] = old[DT_D3];
            }
        }
        // the tile's index advance (every read of sidx above is done: the wavefront's own voices only)
        wave_sync();
        if (lane < DT_RINGS) {
            const int D = slen[lane], k = (lane < 2 ? 2 : 1) * nt;
#pragma unroll
            for (int q = 0; q < DT_VPW; q++) {
                int *p = &sidx[wave * DT_VPW + q][lane];
                *p = dt_idx_after(*p, k, D);
            }
        }
        __syncthreads();

        // 4. the output tiles
#pragma unroll
        for (int j = 0; j < T / DT_ROWS; j++) {
            const int row = row0 + j * DT_ROWS;
            if (row < nt && colv) {
                A.out[(n0 + row) * V + cv] = io[0][row][col];
                A.out[(N + n0 + row) * V + cv] = io[1][row][col];
            }
        }
        __syncthreads();
    }

    if (tid < DT_VB * DT_RINGS) {
        const int l = tid / DT_RINGS, r = tid % DT_RINGS;
        if (v0 + l < V) A.idx[(v0 + l) * DT_RINGS + r] = sidx[l][r];
    }
    if (tid < DT_VB * 2 && v0 + (tid >> 1) < V) A.state[(v0 + (tid >> 1)) * DT_STATE + DT_SIGL + (tid & 1)] = sig[tid >> 1][tid & 1];
    if (pair) A.state[(v0 + lane / 3) * DT_STATE + lane % 3] = y;
}

// the ends of the accepted sample rates, found once by evaluating the rule
struct DtRange {
    uint32_t lo = 0, hi = 0;
    DtRange() {
        for (uint32_t sr = 1; sr <= (1u << 20); sr++) {
            if (!dt_accepts(dt_layout(sr), DT_T)) continue;
            if (!lo) lo = sr;
            hi = sr;
        }
    }
};

int dattaro_layout(uint32_t sample_rate, DtLayout &L) {
    L = dt_layout(sample_rate);
    if (!dt_accepts(L, DT_T)) {
        static const DtRange range;
        return fail(MXG_ERR_INVALID,
                    "maxiDattaroReverb: sample rate %u is not accepted: every delay length must lie in [2, 44100] samples and a tile of 64 "
                    "samples must be legal on the tank rings and taps, which holds from %u to %u Hz (sixteen rates just above the lower end excepted)",
                    sample_rate, range.lo, range.hi);
    }
    return MXG_OK;
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_dattaro_layout_host(uint32_t sample_rate, uint32_t *lengths, uint32_t *offsets, uint32_t *ring_doubles, uint32_t *tap_positions,
                            uint32_t *tap_rings) {
    DtLayout L;
    if (int s = dattaro_layout(sample_rate, L)) return s;
    for (int r = 0; r < DT_RINGS; r++) {
        if (lengths) lengths[r] = (uint32_t)L.len[r];
        if (offsets) offsets[r] = (uint32_t)L.off[r];
    }
    if (ring_doubles) *ring_doubles = (uint32_t)L.S;
    for (int j = 0; j < DT_TAPS; j++) {
        if (tap_positions) tap_positions[j] = (uint32_t)L.tap[j];
        if (tap_rings) tap_rings[j] = (uint32_t)dt_tap_ring(j);
    }
    return MXG_OK;
}

int mxg_dattaro_render(uint32_t sample_rate, size_t V, size_t N, const double *d_in, double *d_rings, int32_t *d_idx, double *d_state,
                       double *d_out, void *stream) {
    DtLayout L;
    if (int s = dattaro_layout(sample_rate, L)) return s;
    MXG_REQUIRE(d_in && d_rings && d_idx && d_state && d_out, "null device pointer");
    if (int s = ensure_init()) return s;
    if (V == 0 || N == 0) return MXG_OK;
    const bool sub = !dt_tile_ok_ring(L.len[DT_AP0], 2, DT_T) || !dt_tile_ok_ring(L.len[DT_AP1], 2, DT_T);
    MXG_REQUIRE(!sub || L.len[DT_AP0] + L.len[DT_AP1] <= DT_STAGE, "the input rings do not fit their staging area");
    const DtArgs A = {V, N, d_in, d_rings, d_idx, d_state, d_out, L};
    hipStream_t st = resolve_stream(stream);
    const dim3 grid((unsigned)((V + DT_VB - 1) / DT_VB));
    KernelTimer kt("dattaro_kernel", st);
    if (sub) hipLaunchKernelGGL(dattaro_kernel<true>, grid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL(dattaro_kernel<false>, grid, dim3(256), 0, st, A);
    return check_hip(hipGetLastError(), "dattaro_kernel launch");
}

}  // extern "C"
