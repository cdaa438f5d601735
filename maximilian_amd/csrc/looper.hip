// looper.hip -- K25: maxiSample::loopRecord (H:706-721) and normalise (C:1126-1137) over a pool of WRITABLE sample slots, with one
// play head (play() or playLoop) fused behind each slot's record head in the reference's call order.  The arithmetic is
// mxg_looper.h's; this file is the pool, the decomposition and the C-ABI.
//
// looprec_kernel: one workgroup owns kLpTile slots for a whole launch of at most kLpPiece samples; longer calls are cut into
// launches on the caller's stream (the launch boundary orders memory), so nothing here needs a fence.
//   1. the [n][r] rows of the input and enable blocks are staged into LDS in runs of kLpTile doubles;
//   2. one lane per slot walks the piece: the lag, the record head, the play head -- a short serial chain that depends on no
//      sample value.  It leaves per sample the lag, the index recorded on, the link to the NEXT visit of the same index inside
//      the piece, and for the play head either the latest visit (<= its own sample) of the index it reads or the index itself;
//   3. a lane per FIRST visit of an index loads the element (the slot's only global loads, with those of play-head reads of
//      indices the piece never records on) and walks that index's visits in order: the overdub of a loop shorter than the piece
//      runs from LDS, never from a global load after a store.  A loop of one index is one lane doing the piece's steps in a row;
//   4. barrier: every global load of the slot is complete;
//   5. the last content of every index visited with the enable on is stored once; the play head takes what it reads from LDS
//      (recorded in this piece: this sample's value included) or from the value loaded in 3, and is stored in runs of kLpTile.
// Steps 2 and 3 are lp_plan_slot and lp_walk_element of mxg_looper.h, which the host build runs over the same pieces.
#include "mxg_common.h"
#include "mxg_smp.h"
#include "mxg_looper.h"

namespace mxg {
namespace {

static_assert(kLpPlay == MXG_SMP_PLAY && kLpPlayLoop == MXG_SMP_PLAYLOOP, "mxg_looper.h restates the enum");

constexpr int kLpTile = 8;      // slots per workgroup: 64-byte runs of the [n][r] blocks
constexpr int kLpPiece = 128;   // samples per launch
constexpr int kLpThreads = 256;
constexpr int kLpEntries = kLpTile * kLpPiece;
constexpr int kLpPer = kLpEntries / kLpThreads;  // entries of a lane: one slot (lane & 7), samples (lane >> 3) + 32 k
static_assert(kLpThreads % kLpTile == 0 && kLpEntries % kLpThreads == 0, "a lane keeps one slot");
// LDS: 3 doubles + 3 ints per entry = 36 bytes * 1024 = 36 KiB of the CU's 160: four workgroups per CU
constexpr size_t kLpPoolAlign = 16;  // slot stride in doubles: every slot starts on the same offset inside a 128-byte line

struct LpArgs {
    size_t R, N, stride, cap;
    double *pool;
    const uint64_t *len;
    const double *in, *enable;
    int eps;
    const double *mix, *start, *end;
    double *recpos, *lagval;
    int play_mode;
    const double *pstart, *pend;
    double *position, *out;
    uint32_t *dropped;
};

__global__ void __launch_bounds__(kLpThreads) looprec_kernel(const LpArgs A) {
    __shared__ double sVal[kLpEntries];  // the input; after step 3 the content of the sample's index once the sample is done
    __shared__ double sEn[kLpEntries];   // the enable block (eps)
    __shared__ double sLag[kLpEntries];
    __shared__ int sIdx[kLpEntries];     // the index recorded on, inside [0, len), or -1
    __shared__ int sLink[kLpEntries];
    __shared__ int sPlay[kLpEntries];    // >= 0: the visit whose sVal the play head reads; < 0: -(index + 6), read from memory
    const int t = (int)threadIdx.x;
    const size_t r0 = (size_t)blockIdx.x * kLpTile;
    const int nT = (int)((A.R - r0) < (size_t)kLpTile ? (A.R - r0) : (size_t)kLpTile);
    const int N = (int)A.N;
    const int s = t & (kLpTile - 1);
    const bool live = s < nT;
    const size_t r = r0 + (size_t)s;

    // 1. stage
#pragma unroll
    for (int k = 0; k < kLpPer; k++) {
        const int n = (t >> 3) + k * (kLpThreads / kLpTile);
        if (live && n < N) {
            const int e = n * kLpTile + s;
            sVal[e] = A.in[(size_t)n * A.R + r];
            if (A.eps) sEn[e] = A.enable[(size_t)n * A.R + r];
        }
    }
    __syncthreads();

    // 2. one lane per slot: lanes 0, 32, 64 .. (two per wavefront)
    if ((t & 31) == 0 && (t >> 5) < nT) {
        const int ss = t >> 5;
        const size_t rr = r0 + (size_t)ss;
        const uint64_t l64 = A.len[rr];
        const size_t len = (size_t)(l64 > A.cap ? A.cap : l64);  // (mxg_sample_pool_lengths refuses such a length; never index past the slot)
        LpRec rec = {A.recpos[rr], A.lagval[rr]};
        const bool playing = A.play_mode != MXG_LOOPER_PLAY_NONE;
        double pos = playing ? A.position[rr] : 0.0;
        uint32_t drops = 0;
        lp_plan_slot(N, kLpTile, len, A.eps ? sEn + ss : nullptr, A.eps ? false : (A.enable[rr] != 0.0), A.start[rr], A.end[rr], A.play_mode,
                     (playing && A.pstart) ? A.pstart[rr] : 0.0, (playing && A.pend) ? A.pend[rr] : 0.0, rec, pos, drops, sLag + ss, sIdx + ss,
                     sLink + ss, sPlay + ss);
        A.recpos[rr] = rec.recpos;
        A.lagval[rr] = rec.lag;
        if (playing) A.position[rr] = pos;
        if (A.dropped && drops) A.dropped[rr] += drops;
    }
    __syncthreads();

    // 3. the slot's global loads, and every index's visits in order
    double *const slot = A.pool + r * A.stride;  // (dereferenced by live lanes only)
    const double mix = live ? A.mix[r] : 0.0;
    double *sp[kLpPer];
    double sv[kLpPer], pv[kLpPer];
#pragma unroll
    for (int k = 0; k < kLpPer; k++) {
        const int n = (t >> 3) + k * (kLpThreads / kLpTile);
        sp[k] = nullptr;
        sv[k] = 0.0;
        pv[k] = 0.0;
        if (live && n < N) {
            const int e = n * kLpTile + s;
            if (sLink[e] & kLpLinkHead) {
                double *p = slot + sIdx[e];
                double c = *p;
                if (lp_walk_element(n, kLpTile, mix, c, sVal + s, sLag + s, sLink + s)) {
                    sp[k] = p;
                    sv[k] = c;
                }
            }
            if (A.play_mode != MXG_LOOPER_PLAY_NONE) {
                const int enc = sPlay[e];
                if (enc < 0) pv[k] = slot[(long long)(-enc) - 6];  // inside [-2, len + 2]: the slot or its zero guards
            }
        }
    }
    // 4. every global load of the slot is complete before its first store
    __syncthreads();
    // 5.
#pragma unroll
    for (int k = 0; k < kLpPer; k++) {
        const int n = (t >> 3) + k * (kLpThreads / kLpTile);
        if (live && n < N) {
            if (sp[k]) *sp[k] = sv[k];
            if (A.play_mode != MXG_LOOPER_PLAY_NONE) {
                const int enc = sPlay[n * kLpTile + s];
                A.out[(size_t)n * A.R + r] = enc >= 0 ? sVal[enc * kLpTile + s] : pv[k];
            }
        }
    }
}

// ---- normalise: partial maxima per (slot, chunk), then every chunk folds its slot's partials and scales itself ------------
constexpr int kNormThreads = 256;
constexpr int kNormChunk = 2048;  // elements per workgroup

__device__ __forceinline__ double norm_block_max(double m, double *red) {  // max is exact in any order
    const int t = (int)threadIdx.x;
    red[t] = m;
    __syncthreads();
    for (int w = kNormThreads / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = red[t] > red[t + w] ? red[t] : red[t + w];
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}

__global__ void __launch_bounds__(kNormThreads) norm_max_kernel(const double *pool, size_t stride, size_t cap, const uint64_t *len,
                                                                double *partial) {
    __shared__ double red[kNormThreads];
    const size_t r = blockIdx.y;
    const uint64_t l64 = len[r];
    const size_t L = (size_t)(l64 > cap ? cap : l64);
    const double *a = pool + r * stride;
    const size_t i0 = (size_t)blockIdx.x * kNormChunk;
    double m = 0.0;
    for (size_t i = i0 + threadIdx.x; i < i0 + kNormChunk && i < L; i += kNormThreads) m = lp_norm_max(m, a[i]);
    m = norm_block_max(m, red);
    if (threadIdx.x == 0) partial[r * gridDim.x + blockIdx.x] = m;
}

__global__ void __launch_bounds__(kNormThreads) norm_scale_kernel(double *pool, size_t stride, size_t cap, const uint64_t *len,
                                                                  const double *maxLevel, const double *partial) {
    __shared__ double red[kNormThreads];
    const size_t r = blockIdx.y;
    const uint64_t l64 = len[r];
    const size_t L = (size_t)(l64 > cap ? cap : l64);
    const size_t i0 = (size_t)blockIdx.x * kNormChunk;
    if (i0 >= L) return;  // (uniform over the workgroup)
    double m = 0.0;
    for (unsigned c = threadIdx.x; c < gridDim.x; c += kNormThreads) {
        const double p = partial[r * gridDim.x + c];
        m = p > m ? p : m;
    }
    const double maxValue = norm_block_max(m, red);
    const float scale = lp_norm_scale(maxLevel[r], maxValue);
    double *a = pool + r * stride;
    for (size_t i = i0 + threadIdx.x; i < i0 + kNormChunk && i < L; i += kNormThreads) a[i] = lp_norm_apply(scale, a[i]);
}

int looprec_check(const char *fn, size_t N, const double *pool, size_t stride, const uint64_t *len, const double *in, const double *enable,
                  const double *mix, const double *start, const double *end, const double *recpos, const double *lagval, int play_mode,
                  const double *pstart, const double *pend, const double *position, const double *out) {
#define LP_REQ(cond, msg) \
    do { if (!(cond)) return fail(MXG_ERR_INVALID, "%s: %s", fn, msg); } while (0)
    LP_REQ(N != 0, "N is 0");
    LP_REQ(N <= MXG_LOOPER_MAX_N, "N is larger than 2^24");
    LP_REQ(pool, "the pool is null");
    LP_REQ(stride != 0, "stride is 0");
    LP_REQ(len, "len is null");
    LP_REQ(in, "the input block in is null");
    LP_REQ(enable, "enable is null");
    LP_REQ(mix, "mix is null");
    LP_REQ(start, "start is null");
    LP_REQ(end, "end is null");
    LP_REQ(recpos, "recpos is null");
    LP_REQ(lagval, "lagval is null");
    LP_REQ(play_mode == MXG_LOOPER_PLAY_NONE || play_mode == MXG_SMP_PLAY || play_mode == MXG_SMP_PLAYLOOP,
           "play_mode is not MXG_LOOPER_PLAY_NONE, MXG_SMP_PLAY or MXG_SMP_PLAYLOOP");
    if (play_mode == MXG_LOOPER_PLAY_NONE) {
        LP_REQ(!out, "out is given without a play mode");
    } else {
        LP_REQ(out, "the output block out is null (with a play mode)");
        LP_REQ(position, "position is null (with a play mode)");
        LP_REQ(out != in && out != enable, "the output block out must be distinct from in and enable");
        if (play_mode == MXG_SMP_PLAYLOOP) {
            LP_REQ(pstart, "pstart is null (MXG_SMP_PLAYLOOP)");
            LP_REQ(pend, "pend is null (MXG_SMP_PLAYLOOP)");
        }
    }
#undef LP_REQ
    return MXG_OK;
}

int lengths_check(const char *fn, size_t R, size_t cap, const uint64_t *h_len) {
    for (size_t r = 0; r < R; r++) {
        if (h_len[r] == 0) return fail(MXG_ERR_INVALID, "%s: len[%zu] is 0", fn, r);
        if (h_len[r] > cap) return fail(MXG_ERR_INVALID, "%s: len[%zu] = %llu is larger than cap = %zu", fn, r, (unsigned long long)h_len[r], cap);
    }
    return MXG_OK;
}

size_t pool_stride(size_t cap) {
    const size_t need = cap + (size_t)kSmpGuardLo + (size_t)kSmpGuardHi;
    return (need + kLpPoolAlign - 1) / kLpPoolAlign * kLpPoolAlign;
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

size_t mxg_sample_pool_stride(size_t cap) { return pool_stride(cap); }

int mxg_looprec_piece(void) { return kLpPiece; }

int mxg_looprec_tile(void) { return kLpTile; }

double *mxg_sample_pool_alloc(size_t R, size_t cap, size_t *stride) {
    if (!stride) {
        fail(MXG_ERR_INVALID, "mxg_sample_pool_alloc: stride is null");
        return nullptr;
    }
    if (R == 0 || cap == 0 || cap > MXG_LOOPER_MAX_CAP) {
        fail(MXG_ERR_INVALID, "mxg_sample_pool_alloc: %s", R == 0 ? "R is 0" : cap == 0 ? "cap is 0" : "cap is larger than 2^31 - 256");
        return nullptr;
    }
    if (ensure_init_only()) return nullptr;
    const size_t st = pool_stride(cap);
    double *base = nullptr;
    if (check_hip(hipMalloc(&base, R * st * sizeof(double)), "hipMalloc(sample pool)")) return nullptr;
    // (the fill is complete before the pointer is handed out: a copy or a launch on any other stream may follow at once)
    if (check_hip(hipMemset(base, 0, R * st * sizeof(double)), "hipMemset(sample pool)") ||
        check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize(sample pool)")) {
        (void)hipFree(base);
        return nullptr;
    }
    *stride = st;
    return base + kSmpGuardLo;  // slot r: p + r * stride, valid on [-4, cap + 5] like an uploaded sample (mxg_smp.h)
}

int mxg_sample_pool_free(double *d_pool) {
    if (!d_pool) return MXG_OK;
    MXG_HIP(hipFree(d_pool - kSmpGuardLo));
    return MXG_OK;
}

int mxg_sample_pool_lengths(size_t R, size_t cap, const uint64_t *h_len, uint64_t *d_len) {
    MXG_REQUIRE(h_len, "h_len is null");
    MXG_REQUIRE(d_len, "d_len is null");
    MXG_REQUIRE(cap != 0 && cap <= MXG_LOOPER_MAX_CAP, "cap is 0 or larger than 2^31 - 256");
    if (int s = lengths_check(__func__, R, cap, h_len)) return s;
    if (int s = ensure_init_only()) return s;
    if (R == 0) return MXG_OK;
    MXG_HIP(hipMemcpy(d_len, h_len, R * sizeof(uint64_t), hipMemcpyHostToDevice));
    return MXG_OK;
}

int mxg_looprec_render(size_t R, size_t N, double *d_pool, size_t stride, size_t cap, const uint64_t *d_len, const double *d_in,
                       const double *d_enable, int eps, const double *d_mix, const double *d_start, const double *d_end, double *d_recpos,
                       double *d_lagval, int play_mode, const double *d_pstart, const double *d_pend, double *d_position, double *d_out,
                       uint32_t *d_dropped, void *stream) {
    if (int s = looprec_check(__func__, N, d_pool, stride, d_len, d_in, d_enable, d_mix, d_start, d_end, d_recpos, d_lagval, play_mode, d_pstart,
                              d_pend, d_position, d_out))
        return s;
    MXG_REQUIRE(cap != 0 && cap <= MXG_LOOPER_MAX_CAP && pool_stride(cap) <= stride, "cap is 0, too large, or does not fit the stride with its guards");
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    if (R == 0) return MXG_OK;
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("looprec_kernel", st);
    const unsigned grid = (unsigned)((R + kLpTile - 1) / kLpTile);
    for (size_t n0 = 0; n0 < N; n0 += kLpPiece) {
        const size_t n = N - n0 < (size_t)kLpPiece ? N - n0 : (size_t)kLpPiece;
        const LpArgs A = {R, n, stride, cap, d_pool, d_len, d_in + n0 * R, eps ? d_enable + n0 * R : d_enable, eps != 0, d_mix, d_start, d_end,
                          d_recpos, d_lagval, play_mode, d_pstart, d_pend, d_position, d_out ? d_out + n0 * R : nullptr, d_dropped};
        hipLaunchKernelGGL(looprec_kernel, dim3(grid), dim3(kLpThreads), 0, st, A);
    }
    return check_hip(hipGetLastError(), "looprec_kernel launch");
}

int mxg_looprec_host(size_t R, size_t N, double *h_pool, size_t stride, size_t cap, const uint64_t *h_len, const double *h_in,
                     const double *h_enable, int eps, const double *h_mix, const double *h_start, const double *h_end, double *h_recpos,
                     double *h_lagval, int play_mode, const double *h_pstart, const double *h_pend, double *h_position, double *h_out,
                     uint32_t *h_dropped) {
    if (int s = looprec_check(__func__, N, h_pool, stride, h_len, h_in, h_enable, h_mix, h_start, h_end, h_recpos, h_lagval, play_mode, h_pstart,
                              h_pend, h_position, h_out))
        return s;
    MXG_REQUIRE(cap != 0 && cap <= MXG_LOOPER_MAX_CAP && pool_stride(cap) <= stride, "cap is 0, too large, or does not fit the stride with its guards");
    if (int s = lengths_check(__func__, R, cap, h_len)) return s;
    lp_host_render(R, N, h_pool, stride, h_len, h_in, h_enable, eps, h_mix, h_start, h_end, h_recpos, h_lagval, play_mode, h_pstart, h_pend,
                   h_position, h_out, h_dropped);
    return MXG_OK;
}

int mxg_sample_pool_normalise(size_t R, double *d_pool, size_t stride, size_t cap, const uint64_t *d_len, const double *d_maxLevel,
                              void *stream) {
    MXG_REQUIRE(d_pool, "the pool is null");
    MXG_REQUIRE(d_len, "len is null");
    MXG_REQUIRE(d_maxLevel, "maxLevel is null");
    MXG_REQUIRE(cap != 0 && cap <= MXG_LOOPER_MAX_CAP && pool_stride(cap) <= stride, "cap is 0, too large, or does not fit the stride with its guards");
    MXG_REQUIRE(R <= 65535, "R is larger than 65535 (normalise the pool in several calls)");
    if (int s = ensure_init()) return s;
    if (R == 0) return MXG_OK;
    hipStream_t st = resolve_stream(stream);
    const unsigned chunks = (unsigned)((cap + kNormChunk - 1) / kNormChunk);
    void *partial = nullptr;
    if (int s = scratch_get(SCR_LOOPER, st, R * chunks * sizeof(double), &partial)) return s;
    KernelTimer kt("norm_kernels", st);
    hipLaunchKernelGGL(norm_max_kernel, dim3(chunks, (unsigned)R), dim3(kNormThreads), 0, st, d_pool, stride, cap, d_len, (double *)partial);
    hipLaunchKernelGGL(norm_scale_kernel, dim3(chunks, (unsigned)R), dim3(kNormThreads), 0, st, d_pool, stride, cap, d_len, d_maxLevel,
                       (const double *)partial);
    return check_hip(hipGetLastError(), "norm kernels launch");
}

int mxg_sample_pool_normalise_host(size_t R, double *h_pool, size_t stride, size_t cap, const uint64_t *h_len, const double *h_maxLevel) {
    MXG_REQUIRE(h_pool, "the pool is null");
    MXG_REQUIRE(h_len, "len is null");
    MXG_REQUIRE(h_maxLevel, "maxLevel is null");
    MXG_REQUIRE(cap != 0 && cap <= MXG_LOOPER_MAX_CAP && pool_stride(cap) <= stride, "cap is 0, too large, or does not fit the stride with its guards");
    if (int s = lengths_check(__func__, R, cap, h_len)) return s;
    lp_host_normalise(R, h_pool, stride, h_len, h_maxLevel);
    return MXG_OK;
}

}  // extern "C"
