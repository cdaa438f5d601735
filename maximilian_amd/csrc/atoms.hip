// atoms.hip -- maxiAtomBank on gfx950 (K22): the reference's Gabor atoms, its atom queue and its book player
// (src/libs/maxiAtoms.cpp, the portable branch) for S independent streams.  The arithmetic and the queue's integer rules are
// mxg_atoms.h, which also compiles for the host (the mxg_atoms_*_host twins below, tests/host_atoms.cpp).
//
// A block is two kernels.
//   K22a atoms_due_kernel     one wavefront per stream.  With the player on it finds, by ballot over 64 book atoms at a time, the first
//                             atom from atomIdx on whose position fails the player's test, and takes the atoms before it as new queue
//                             entries.  It then walks the stream's live list (never the book), 64 entries at a time in queue order:
//                             the due test, the share of this block as a segment (kind, pool offset, src_pos, dst_off, count and the
//                             Gabor parameters), the position advance; segments and surviving entries are compacted IN ORDER by
//                             ballot + popcount, in place.  A live list that would pass its capacity Q stores a code in the device
//                             error word and marks the stream's block (nseg = -1); nothing of that stream changes.
//   K22b atoms_render_kernel  a workgroup of 128 lanes owns one stream and a tile of 256 output samples, lanes along time: lane l holds
//                             samples l and l + 128 of the tile in float registers, so a segment's parameters are wave-uniform and the
//                             float loads and stores are coalesced.  The stream's segment list is staged through LDS in pieces of
//                             MXG_ATOMS_PIECE entries and walked piece by piece; every lane adds the segments that reach its samples
//                             IN LIST ORDER, which is the reference's float sum in queue order.  No atomics.  GABOR synthesises the
//                             sample from the parameters and the length's float window table, RAW reads the caller's floats.
// HBM per block: 4 B per output sample (8 with accumulate), the window / raw floats of the live atoms (L2 hits after the first tile
// row), 36 B per segment and tile.  LDS 2.3 KB.  No scratch.
#include "mxg_common.h"  // (include/maxigpu.h first: the MXG_ATOM_* constants)

#include <math.h>
#include <string.h>

#include <map>
#include <vector>

#include "mxg_atoms.h"

#define MXG_ATOMS_TILE 256
#define MXG_ATOMS_LANES 128

struct mxg_atoms_bank {
    bool host;
    size_t S, Q, A;
    // the book: CSR over the streams
    int64_t *book_start;    // [S + 1]
    float *book_pos;        // [A]
    mxg::AtomInst *book_inst;  // [A]
    uint32_t *num_samples;  // [S]
    // state
    int64_t *sampleIdx;     // [S]
    uint32_t *atomIdx;      // [S]
    int32_t *nlive;         // [S]
    mxg::AtomInst *live;    // [S][Q]
    // this block
    int32_t *nseg;          // [S]
    mxg::AtomSeg *seg;      // [S][Q]
    // pools: one window table per distinct Gabor length, the caller's raw floats
    float *win, *raw;
    size_t win_len, win_cap, raw_len, raw_cap;
    std::map<uint32_t, uint32_t> win_off;
};

namespace mxg {
namespace {

struct AtomsDev {
    size_t S, Q;
    const int64_t *book_start;
    const float *book_pos;
    const AtomInst *book_inst;
    const uint32_t *num_samples;
    int64_t *sampleIdx;
    uint32_t *atomIdx;
    int32_t *nlive;
    AtomInst *live;
    int32_t *nseg;
    AtomSeg *seg;
};

template <bool PLAYER>
__global__ void __launch_bounds__(64) atoms_due_kernel(AtomsDev B, uint32_t N, int onset, int *err) {
    const size_t s = blockIdx.x;
    const unsigned lane = threadIdx.x;
    const int64_t idx = B.sampleIdx[s];
    const int n0 = B.nlive[s];
    uint32_t ai = B.atomIdx[s], end = ai;
    size_t b0 = 0;
    int32_t looped = 0;
    if constexpr (PLAYER) {
        b0 = (size_t)B.book_start[s];
        const uint32_t nb = (uint32_t)((size_t)B.book_start[s + 1] - b0);
        const uint32_t ns = B.num_samples[s];
        looped = player_looped(idx, ns);
        if ((int64_t)looped < (int64_t)N) ai = 0;
        const float limit = player_limit(idx, N, ns);
        end = ai;
        while (end < nb) {  // (wave-uniform)
            const uint32_t k = end + lane;
            const bool ok = k < nb && B.book_pos[b0 + k] < limit;
            const unsigned long long pass = __ballot(ok);
            if (pass == ~0ull) {
                end += 64;
                continue;
            }
            end += (uint32_t)(__ffsll((unsigned long long)~pass) - 1);
            break;
        }
        if ((size_t)n0 + (end - ai) > B.Q) {
            if (lane == 0) {
                if (err) __hip_atomic_store(err, (int)ASYNC_ATOMS_OVERFLOW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                B.nseg[s] = -1;
            }
            return;
        }
    }
    const int total = n0 + (int)(end - ai);  // <= Q
    AtomInst *live = B.live + s * B.Q;
    AtomSeg *seg = B.seg + s * B.Q;
    const unsigned long long lt = (1ull << lane) - 1;
    int nseg = 0, keep = 0;
    for (int k0 = 0; k0 < total; k0 += 64) {
        const int k = k0 + (int)lane;
        const bool have = k < total;
        AtomInst a = {0, 0, 0, 0, 0, 0.f, 0.f, 0.f, 0.f};
        if (have) {
            if (k < n0) {
                a = live[k];
            } else {
                const size_t bk = b0 + ai + (size_t)(k - n0);
                a = B.book_inst[bk];
                a.startTime = idx + (int64_t)player_offset(looped, B.book_pos[bk]);
                a.pos = 0;
            }
        }
        // every load of this chunk has returned before a lane stores over another lane's entry (the compaction is in place)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bool emit = false;
        AtomSeg g = {0, 0, 0, 0, 0, 0.f, 0.f, 0.f, 0.f};
        int32_t atomStart;
        if (have && atom_due(a.startTime, a.pos, idx, N, atomStart)) {
            uint32_t dst;
            const uint32_t cnt = atom_advance(a.pos, a.size, N, onset, atomStart, idx, dst);
            emit = cnt != 0;
            g = {a.kind, a.off, a.pos, dst, cnt, a.inc, a.maxPhase, a.startPhase, a.amp};
            a.pos += cnt;
        }
        const bool kp = have && a.pos != a.size;
        const unsigned long long em = __ballot(emit), km = __ballot(kp);
        if (emit) seg[nseg + __popcll(em & lt)] = g;  // nseg + ... <= k < Q
        if (kp) live[keep + __popcll(km & lt)] = a;   // keep + ... <= k < Q
        nseg += __popcll(em);
        keep += __popcll(km);
    }
    if (lane == 0) {
        B.sampleIdx[s] = idx + (int64_t)N;
        B.atomIdx[s] = end;
        B.nlive[s] = keep;
        B.nseg[s] = nseg;
    }
}

template <bool ACC>
__global__ void __launch_bounds__(MXG_ATOMS_LANES) atoms_render_kernel(size_t Q, uint32_t N, uint32_t tiles, const int32_t *__restrict__ nseg,
                                                                       const AtomSeg *__restrict__ seg, const float *__restrict__ win,
                                                                       const float *__restrict__ raw, float *out) {
    __shared__ uint32_t piece[MXG_ATOMS_PIECE * kAtomSegWords];
    const size_t s = blockIdx.x / tiles;
    const uint32_t t0 = (blockIdx.x % tiles) * MXG_ATOMS_TILE;
    const int cnt = nseg[s];
    if (cnt < 0) return;  // the stream overflowed in K22a: its block is left as it is
    constexpr int SPL = MXG_ATOMS_TILE / MXG_ATOMS_LANES;
    float *o = out + s * (size_t)N;
    uint32_t t[SPL];
    float acc[SPL];
#pragma unroll
    for (int j = 0; j < SPL; j++) {
        t[j] = t0 + threadIdx.x + j * MXG_ATOMS_LANES;
        acc[j] = (ACC && t[j] < N) ? o[t[j]] : 0.0f;
    }
    const uint32_t *list = reinterpret_cast<const uint32_t *>(seg + s * Q);
    for (int p0 = 0; p0 < cnt; p0 += MXG_ATOMS_PIECE) {
        const int np = cnt - p0 < MXG_ATOMS_PIECE ? cnt - p0 : MXG_ATOMS_PIECE;
        __syncthreads();  // the piece before this one has been read by every lane
        for (int w = threadIdx.x; w < np * kAtomSegWords; w += MXG_ATOMS_LANES) piece[w] = list[(size_t)p0 * kAtomSegWords + w];
        __syncthreads();
        for (int e = 0; e < np; e++) {
            const AtomSeg g = *reinterpret_cast<const AtomSeg *>(piece + e * kAtomSegWords);  // (a broadcast read: wave-uniform)
            if (g.dst_off + g.count <= t0 || g.dst_off >= t0 + MXG_ATOMS_TILE) continue;     // (not in this tile: workgroup-uniform)
#pragma unroll
            for (int j = 0; j < SPL; j++) {
                const uint32_t d = t[j] - g.dst_off;  // (wraps above count for t < dst_off)
                if (d < g.count) {                    // dst_off + count <= N: t[j] < N here
                    const uint32_t i = g.src_pos + d;
                    float v;
                    if (g.kind == MXG_ATOM_RAW) v = raw[(size_t)g.off + i];
                    else v = gabor_sample(win[(size_t)g.off + i], g.inc, g.maxPhase, g.startPhase, g.amp, i);
                    acc[j] = acc[j] + v;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < SPL; j++)
        if (t[j] < N) o[t[j]] = acc[j];
}

// ---- the bank's memory: host arrays (the _host twin) or device arrays ---------------------------------------------------------------
int bank_alloc(bool host, void **p, size_t bytes) {
    if (!bytes) bytes = 8;
    if (host) {
        *p = calloc(1, bytes);
        return *p ? MXG_OK : fail(MXG_ERR_NOMEM, "mxg_atoms: out of host memory (%zu bytes)", bytes);
    }
    MXG_HIP(hipMalloc(p, bytes));
    MXG_HIP(hipMemset(*p, 0, bytes));
    return MXG_OK;
}
void bank_free(bool host, void *p) {
    if (!p) return;
    if (host) free(p);
    else (void)hipFree(p);
}
int bank_put(bool host, void *dst, const void *src, size_t bytes) {
    if (!bytes) return MXG_OK;
    if (host) {
        memcpy(dst, src, bytes);
        return MXG_OK;
    }
    MXG_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return MXG_OK;
}
int bank_get(bool host, void *dst, const void *src, size_t bytes) {
    if (!bytes) return MXG_OK;
    if (host) {
        memcpy(dst, src, bytes);
        return MXG_OK;
    }
    MXG_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return MXG_OK;
}
// appends n floats to a grow-only pool; *off = where they start.  Growing moves the pool: the device is idle then (the caller synchronised).
int pool_append(bool host, float *&pool, size_t &len, size_t &cap, const float *h, size_t n, size_t *off) {
    if (len + n > cap) {
        size_t ncap = cap ? cap : 1024;
        while (ncap < len + n) ncap *= 2;
        float *np = nullptr;
        if (int st = bank_alloc(host, (void **)&np, ncap * sizeof(float))) return st;
        if (len) {
            if (host) memcpy(np, pool, len * sizeof(float));
            else MXG_HIP(hipMemcpy(np, pool, len * sizeof(float), hipMemcpyDeviceToDevice));
        }
        bank_free(host, pool);
        pool = np;
        cap = ncap;
    }
    if (int st = bank_put(host, pool + len, h, n * sizeof(float))) return st;
    *off = len;
    len += n;
    return MXG_OK;
}

constexpr uint32_t kWindowCache = 22050;  // maxiGrainWindowCache: lengths below sampleRate / 2 at the reference's static initialisation

// the offset of the window table of `length`, built on first use: (float)env[i], env from libm's exp as grains.hip builds its tables
int window_offset(mxg_atoms_bank *b, uint32_t length, uint32_t *off) {
    auto it = b->win_off.find(length);
    if (it != b->win_off.end()) {
        *off = it->second;
        return MXG_OK;
    }
    std::vector<float> w(length);
    for (uint32_t i = 0; i < length; i++) w[i] = (float)gabor_window(length, i);
    size_t at = 0;
    if (b->win_len + length > 0xffffffffull) return fail(MXG_ERR_INVALID, "mxg_atoms: the window tables pass 2^32 floats");
    if (int st = pool_append(b->host, b->win, b->win_len, b->win_cap, w.data(), length, &at)) return st;
    b->win_off[length] = (uint32_t)at;
    *off = (uint32_t)at;
    return MXG_OK;
}

// createGabor's arguments as a queue entry; refuses what the reference cannot take or the sine's reduction does not cover
int gabor_inst(mxg_atoms_bank *b, const char *who, float freq, float sampleRate, uint32_t length, float startPhase, float amp, AtomInst *a) {
    if (!(length >= 1 && length < kWindowCache))
        return fail(MXG_ERR_INVALID, "%s: a Gabor atom of %u samples is outside [1, %u): the reference's window cache holds lengths below 22 050",
                    who, length, kWindowCache);
    if (!isfinite(freq) || !isfinite(sampleRate) || !isfinite(startPhase) || !isfinite(amp))
        return fail(MXG_ERR_INVALID, "%s: a Gabor atom's frequency, sample rate, phase and amplitude must be finite", who);
    const GaborPar p = gabor_params(freq, sampleRate, length);
    if (!(fabsf(p.maxPhase) + fabsf(startPhase) <= kAtomsMaxArg))
        return fail(MXG_ERR_INVALID, "%s: the sine's argument would pass 2^19 rad (or is NaN: frequency and sample rate both 0)", who);
    uint32_t off = 0;
    if (b)  // (null: the checks alone)
        if (int st = window_offset(b, length, &off)) return st;
    *a = {0, 0, length, MXG_ATOM_GABOR, off, p.inc, p.maxPhase, startPhase, amp};
    return MXG_OK;
}

mxg_atoms_bank *bank_create(bool host, size_t S, size_t Q, const int64_t *book_start, const float *book, const uint32_t *num_samples,
                            const float *raw, size_t raw_len) {
    const char *who = host ? "mxg_atoms_bank_create_host" : "mxg_atoms_bank_create";
    if (!S || !Q || S > 0x7fffffffull / MXG_ATOMS_TILE || Q > 0x7fffffffull / S) {
        fail(MXG_ERR_INVALID, "%s: S and Q must be at least 1 (and S * Q below 2^31)", who);
        return nullptr;
    }
    size_t A = 0;
    if (book_start) {
        bool ok = book_start[0] == 0;
        for (size_t s = 0; s < S && ok; s++) ok = book_start[s + 1] >= book_start[s];
        if (!ok || book_start[S] > 0x7fffffff || (book_start[S] && (!book || !num_samples))) {
            fail(MXG_ERR_INVALID, "%s: book_start must rise from 0 (below 2^31), with the book and num_samples given", who);
            return nullptr;
        }
        A = (size_t)book_start[S];
    }
    if (raw_len > 0xffffffffull || (raw_len && !raw)) {
        fail(MXG_ERR_INVALID, "%s: the raw pool is null or passes 2^32 floats", who);
        return nullptr;
    }
    for (size_t s = 0; s < S && num_samples; s++)
        if (!num_samples[s]) {
            fail(MXG_ERR_INVALID, "%s: a book's numSamples is 0 (the player divides by it)", who);
            return nullptr;
        }
    std::vector<AtomInst> inst(A);
    mxg_atoms_bank *b = nullptr;
    int st = MXG_OK;
    for (int pass = 0; pass < 2 && !st; pass++) {  // the checks first: a refused book says why before the device is touched
        if (pass) {
            if (!host && ensure_init_only()) return nullptr;
            b = new mxg_atoms_bank();
            b->host = host;
            b->S = S, b->Q = Q, b->A = A;
        }
        for (size_t k = 0; k < A && !st; k++) {  // book rows: position, length, amp, frequency, phase
            const float pos = book[k], len = book[A + k], amp = book[2 * A + k], frq = book[3 * A + k], ph = book[4 * A + k];
            if (!(pos >= 0.0f && pos < 4294967296.0f)) st = fail(MXG_ERR_INVALID, "%s: atom %zu: position is negative, NaN or beyond 2^32", who, k);
            else if (!(len >= 0.0f && len < (float)kWindowCache)) st = fail(MXG_ERR_INVALID, "%s: atom %zu: length is negative, NaN or beyond the window cache (22 050)", who, k);
            else if (!isfinite(frq)) st = fail(MXG_ERR_INVALID, "%s: atom %zu: frequency is NaN or infinite", who, k);
            else st = gabor_inst(b, who, book_freq(frq), kBookSampleRate, (uint32_t)len, ph, book_amp(amp), &inst[k]);
        }
    }
    if (!b) return nullptr;
    std::vector<int64_t> starts(S + 1, 0);
    if (book_start) starts.assign(book_start, book_start + S + 1);
    std::vector<uint32_t> ns(S, 1);
    if (num_samples) ns.assign(num_samples, num_samples + S);
    if (!st) st = bank_alloc(host, (void **)&b->book_start, (S + 1) * 8);
    if (!st) st = bank_alloc(host, (void **)&b->book_pos, A * 4);
    if (!st) st = bank_alloc(host, (void **)&b->book_inst, A * sizeof(AtomInst));
    if (!st) st = bank_alloc(host, (void **)&b->num_samples, S * 4);
    if (!st) st = bank_alloc(host, (void **)&b->sampleIdx, S * 8);
    if (!st) st = bank_alloc(host, (void **)&b->atomIdx, S * 4);
    if (!st) st = bank_alloc(host, (void **)&b->nlive, S * 4);
    if (!st) st = bank_alloc(host, (void **)&b->nseg, S * 4);
    if (!st) st = bank_alloc(host, (void **)&b->live, S * Q * sizeof(AtomInst));
    if (!st) st = bank_alloc(host, (void **)&b->seg, S * Q * sizeof(AtomSeg));
    if (!st) st = bank_put(host, b->book_start, starts.data(), (S + 1) * 8);
    if (!st) st = bank_put(host, b->book_pos, book, A * 4);
    if (!st) st = bank_put(host, b->book_inst, inst.data(), A * sizeof(AtomInst));
    if (!st) st = bank_put(host, b->num_samples, ns.data(), S * 4);
    size_t at = 0;
    if (!st && raw_len) st = pool_append(host, b->raw, b->raw_len, b->raw_cap, raw, raw_len, &at);
    if (!st && !b->win) st = bank_alloc(host, (void **)&b->win, 8);  // (kernels take non-null pools)
    if (!st && !b->raw) st = bank_alloc(host, (void **)&b->raw, 8);
    if (st) {
        mxg_atoms_bank_destroy(b);
        return nullptr;
    }
    return b;
}

int bank_sync(const mxg_atoms_bank *b) {
    if (b->host) return MXG_OK;
    MXG_HIP(hipDeviceSynchronize());
    return MXG_OK;
}

int bank_add(mxg_atoms_bank *b, bool host, size_t n, const int32_t *stream, const int32_t *kind, const uint32_t *length,
             const uint32_t *offset, const float *par, const uint32_t *raw_off) {
    const char *who = host ? "mxg_atoms_add_host" : "mxg_atoms_add";
    MXG_REQUIRE(b, "null bank");
    MXG_REQUIRE(b->host == host, "a host bank takes the _host calls, a device bank the others");
    if (!n) return MXG_OK;
    MXG_REQUIRE(stream && kind && length, "stream, kind or length is null");
    if (int st = bank_sync(b)) return st;
    std::vector<int32_t> nlive(b->S);
    std::vector<int64_t> sidx(b->S);
    if (int st = bank_get(host, nlive.data(), b->nlive, b->S * 4)) return st;
    if (int st = bank_get(host, sidx.data(), b->sampleIdx, b->S * 8)) return st;
    std::vector<std::vector<AtomInst>> add(b->S);
    for (size_t k = 0; k < n; k++) {
        if (stream[k] < 0 || (size_t)stream[k] >= b->S) return fail(MXG_ERR_INVALID, "%s: instance %zu: stream %d is outside [0, S)", who, k, stream[k]);
        AtomInst a;
        if (kind[k] == MXG_ATOM_GABOR) {
            if (!par) return fail(MXG_ERR_INVALID, "%s: a Gabor instance needs the parameter rows", who);
            if ((int32_t)length[k] < 0) return fail(MXG_ERR_INVALID, "%s: instance %zu: negative length", who, k);
            if (int st = gabor_inst(b, who, par[4 * k], par[4 * k + 1], length[k], par[4 * k + 2], par[4 * k + 3], &a)) return st;
        } else if (kind[k] == MXG_ATOM_RAW) {
            if (!raw_off) return fail(MXG_ERR_INVALID, "%s: a raw instance needs raw_off", who);
            if ((int32_t)length[k] < 0) return fail(MXG_ERR_INVALID, "%s: instance %zu: negative length", who, k);
            if ((size_t)raw_off[k] + length[k] > b->raw_len)
                return fail(MXG_ERR_INVALID, "%s: instance %zu: raw floats [%u, %u + %u) are outside the pool (%zu)", who, k, raw_off[k], raw_off[k],
                            length[k], b->raw_len);
            a = {0, 0, length[k], MXG_ATOM_RAW, raw_off[k], 0.f, 0.f, 0.f, 0.f};
        } else {
            return fail(MXG_ERR_INVALID, "%s: instance %zu: kind is not MXG_ATOM_GABOR or MXG_ATOM_RAW", who, k);
        }
        const size_t s = (size_t)stream[k];
        a.startTime = sidx[s] + (int64_t)(offset ? offset[k] : 0u);  // A:100
        add[s].push_back(a);
        if ((size_t)nlive[s] + add[s].size() > b->Q)
            return fail(MXG_ERR_INVALID, "%s: stream %zu: more than Q = %zu atoms queued; nothing was added", who, s, b->Q);
    }
    for (size_t s = 0; s < b->S; s++) {
        if (add[s].empty()) continue;
        if (int st = bank_put(host, b->live + s * b->Q + nlive[s], add[s].data(), add[s].size() * sizeof(AtomInst))) return st;
        nlive[s] += (int32_t)add[s].size();
    }
    return bank_put(host, b->nlive, nlive.data(), b->S * 4);
}

int bank_step_host(mxg_atoms_bank *b, bool player, size_t N, float *out, int onset, int accumulate) {
    bool overflow = false;
    for (size_t s = 0; s < b->S; s++) {
        const size_t b0 = (size_t)b->book_start[s];
        const AtomBookView book = {b->book_pos + b0, b->book_inst + b0, (uint32_t)((size_t)b->book_start[s + 1] - b0), b->num_samples[s]};
        AtomSeg *seg = b->seg + s * b->Q;
        const int n = atoms_stream_step(player, book, onset, (uint32_t)N, b->Q, b->sampleIdx[s], b->atomIdx[s], b->nlive[s], b->live + s * b->Q, seg);
        b->nseg[s] = n;
        if (n < 0) {
            overflow = true;
            continue;
        }
        float *o = out + s * N;
        if (!accumulate) memset(o, 0, N * sizeof(float));
        for (int k = 0; k < n; k++) atoms_seg_render(seg[k], b->win, b->raw, o);
    }
    return overflow ? async_error_status(ASYNC_ATOMS_OVERFLOW) : MXG_OK;
}

int bank_step(mxg_atoms_bank *b, bool player, size_t N, float *out, int onset, int accumulate, void *stream) {
    if (int st = ensure_init()) return st;
    hipStream_t q = resolve_stream(stream);
    const AtomsDev B = {b->S, b->Q, b->book_start, b->book_pos, b->book_inst, b->num_samples, b->sampleIdx, b->atomIdx, b->nlive, b->live, b->nseg, b->seg};
    {
        KernelTimer kt("atoms_due_kernel", q);
        if (player) hipLaunchKernelGGL(atoms_due_kernel<true>, dim3((unsigned)b->S), dim3(64), 0, q, B, (uint32_t)N, onset, async_error_word());
        else hipLaunchKernelGGL(atoms_due_kernel<false>, dim3((unsigned)b->S), dim3(64), 0, q, B, (uint32_t)N, onset, async_error_word());
        if (int st = check_hip(hipGetLastError(), "atoms_due_kernel launch")) return st;
    }
    const uint32_t tiles = (uint32_t)((N + MXG_ATOMS_TILE - 1) / MXG_ATOMS_TILE);
    KernelTimer kt("atoms_render_kernel", q);
    const dim3 grid((unsigned)(b->S * tiles));
    if (accumulate) hipLaunchKernelGGL(atoms_render_kernel<true>, grid, dim3(MXG_ATOMS_LANES), 0, q, b->Q, (uint32_t)N, tiles, b->nseg, b->seg, b->win, b->raw, out);
    else hipLaunchKernelGGL(atoms_render_kernel<false>, grid, dim3(MXG_ATOMS_LANES), 0, q, b->Q, (uint32_t)N, tiles, b->nseg, b->seg, b->win, b->raw, out);
    return check_hip(hipGetLastError(), "atoms_render_kernel launch");
}

}  // namespace
}  // namespace mxg

using namespace mxg;

#define MXG_ATOMS_STEP_CHECKS(want_host)                                                                                      \
    MXG_REQUIRE(b, "null bank");                                                                                              \
    MXG_REQUIRE(b->host == (want_host), "a host bank takes the _host calls, a device bank the others");                       \
    MXG_REQUIRE(N >= 1 && N <= ((size_t)1 << 24), "N must be in [1, 2^24]");                                                  \
    MXG_REQUIRE(b->S * ((N + MXG_ATOMS_TILE - 1) / MXG_ATOMS_TILE) <= 0x7fffffffull, "S * tiles passes the grid limit");      \
    MXG_REQUIRE(out, "the output block is null");                                                                             \
    MXG_REQUIRE(onset == MXG_ATOM_ONSET_BLOCK || onset == MXG_ATOM_ONSET_SAMPLE, "onset is not MXG_ATOM_ONSET_BLOCK or _SAMPLE")

extern "C" {

mxg_atoms_bank *mxg_atoms_bank_create(size_t S, size_t Q, const int64_t *h_book_start, const float *h_book, const uint32_t *h_num_samples,
                                      const float *h_raw, size_t raw_len) {
    return bank_create(false, S, Q, h_book_start, h_book, h_num_samples, h_raw, raw_len);
}
mxg_atoms_bank *mxg_atoms_bank_create_host(size_t S, size_t Q, const int64_t *h_book_start, const float *h_book, const uint32_t *h_num_samples,
                                           const float *h_raw, size_t raw_len) {
    return bank_create(true, S, Q, h_book_start, h_book, h_num_samples, h_raw, raw_len);
}

int mxg_atoms_bank_destroy(mxg_atoms_bank *b) {
    if (!b) return MXG_OK;
    if (!b->host) (void)hipDeviceSynchronize();
    void *all[] = {b->book_start, b->book_pos, b->book_inst, b->num_samples, b->sampleIdx, b->atomIdx, b->nlive, b->live, b->nseg, b->seg, b->win, b->raw};
    for (void *p : all) bank_free(b->host, p);
    delete b;
    return MXG_OK;
}

int mxg_atoms_raw_append(mxg_atoms_bank *b, const float *h_raw, size_t n, uint32_t *offset) {
    MXG_REQUIRE(b, "null bank");
    MXG_REQUIRE(offset, "offset is null");
    MXG_REQUIRE(!n || h_raw, "the floats are null");
    MXG_REQUIRE(b->raw_len + n <= 0xffffffffull, "the raw pool would pass 2^32 floats");
    if (int st = bank_sync(b)) return st;
    size_t at = 0;
    if (int st = pool_append(b->host, b->raw, b->raw_len, b->raw_cap, h_raw, n, &at)) return st;
    *offset = (uint32_t)at;
    return MXG_OK;
}

int mxg_atoms_add(mxg_atoms_bank *b, size_t n, const int32_t *h_stream, const int32_t *h_kind, const uint32_t *h_length,
                  const uint32_t *h_offset, const float *h_par, const uint32_t *h_raw_off) {
    return bank_add(b, false, n, h_stream, h_kind, h_length, h_offset, h_par, h_raw_off);
}
int mxg_atoms_add_host(mxg_atoms_bank *b, size_t n, const int32_t *h_stream, const int32_t *h_kind, const uint32_t *h_length,
                       const uint32_t *h_offset, const float *h_par, const uint32_t *h_raw_off) {
    return bank_add(b, true, n, h_stream, h_kind, h_length, h_offset, h_par, h_raw_off);
}

int mxg_atoms_fill(mxg_atoms_bank *b, size_t N, float *d_out, int onset, int accumulate, void *stream) {
    float *out = d_out;
    MXG_ATOMS_STEP_CHECKS(false);
    return bank_step(b, false, N, out, onset, accumulate, stream);
}
int mxg_atoms_play(mxg_atoms_bank *b, size_t N, float *d_out, int onset, int accumulate, void *stream) {
    float *out = d_out;
    MXG_ATOMS_STEP_CHECKS(false);
    return bank_step(b, true, N, out, onset, accumulate, stream);
}
int mxg_atoms_fill_host(mxg_atoms_bank *b, size_t N, float *h_out, int onset, int accumulate) {
    float *out = h_out;
    MXG_ATOMS_STEP_CHECKS(true);
    return bank_step_host(b, false, N, out, onset, accumulate);
}
int mxg_atoms_play_host(mxg_atoms_bank *b, size_t N, float *h_out, int onset, int accumulate) {
    float *out = h_out;
    MXG_ATOMS_STEP_CHECKS(true);
    return bank_step_host(b, true, N, out, onset, accumulate);
}

int mxg_atoms_state(mxg_atoms_bank *b, int64_t *h_sample_idx, uint32_t *h_atom_idx, int32_t *h_nlive, int64_t *h_start, uint32_t *h_pos,
                    uint32_t *h_size) {
    MXG_REQUIRE(b, "null bank");
    if (int st = bank_sync(b)) return st;
    if (h_sample_idx)
        if (int st = bank_get(b->host, h_sample_idx, b->sampleIdx, b->S * 8)) return st;
    if (h_atom_idx)
        if (int st = bank_get(b->host, h_atom_idx, b->atomIdx, b->S * 4)) return st;
    if (h_nlive)
        if (int st = bank_get(b->host, h_nlive, b->nlive, b->S * 4)) return st;
    if (h_start || h_pos || h_size) {
        std::vector<AtomInst> live(b->S * b->Q);
        if (int st = bank_get(b->host, live.data(), b->live, live.size() * sizeof(AtomInst))) return st;
        for (size_t k = 0; k < live.size(); k++) {
            if (h_start) h_start[k] = live[k].startTime;
            if (h_pos) h_pos[k] = live[k].pos;
            if (h_size) h_size[k] = live[k].size;
        }
    }
    return MXG_OK;
}

int mxg_atoms_gabor_host(float freq, float sample_rate, uint32_t length, float start_phase, float amp, float *h_atom) {
    MXG_REQUIRE(h_atom, "the atom is null");
    MXG_REQUIRE(length >= 1 && length < kWindowCache, "length is outside [1, 22 050): the reference's window cache");
    MXG_REQUIRE(isfinite(freq) && isfinite(sample_rate) && isfinite(start_phase) && isfinite(amp), "a parameter is NaN or infinite");
    const GaborPar p = gabor_params(freq, sample_rate, length);
    MXG_REQUIRE(fabsf(p.maxPhase) + fabsf(start_phase) <= kAtomsMaxArg, "the sine's argument would pass 2^19 rad (or is NaN)");
    for (uint32_t i = 0; i < length; i++) h_atom[i] = gabor_sample((float)gabor_window(length, i), p.inc, p.maxPhase, start_phase, amp, i);
    return MXG_OK;
}

}  // extern "C"
