// mxg_stream.h -- the streaming skeleton of the per-voice bank kernels: one lane = one voice, chunks of U samples, the block
// out[n*V + v] written as a pure store stream.  The kernels keep their arithmetic; what is here is the part
// that has to be the same in all of them, with its reasons:
//
//  * Loads and stores retire in order on ONE counter (vmcnt).  A vector load inside the chunk loop whose value is used in the same
//    iteration makes the wait for it a wait for every store issued before it: the store stream drains once per chunk, the kernel
//    stays bit-exact and loses about a fifth of its rate.  So an [N][V] input is requested ONE CHUNK AHEAD (rows_first before the
//    loop, rows_next at the top of every chunk): the wait that rows_next's copy needs is a counted one that leaves the newer
//    stores in flight.
//  * The prefetch is CLAMPED (row min(n, N - 1)), not branched: a branch around the loads would give the loop two paths with
//    different numbers of loads in flight, and a wait that has to serve both is vmcnt(0).  Clamped, every chunk issues the same U
//    loads; the rows past the block are re-reads of its last row that nobody uses.  The same clamp in rows_first is all that
//    keeps a block shorter than one chunk from reading past its end.
//  * The state and parameters a kernel loads in its PROLOGUE are consumed by an empty `asm volatile("" : "+v"(x))` before the
//    loop.  A first use inside the loop is a wait at the loop header, which has to serve the entry path as well as the back edge
//    and therefore comes out as vmcnt(0..8) on every chunk.
//  * The surplus lanes of a bank's last wavefront stay alive (the shared-gate readlanes and the pair-row exchange need all 64
//    lanes) and shadow a voice: the same loads, arithmetic and stores as the lane that owns it.  With pair rows they shadow the
//    last PAIR, parity kept, because a lane's parity decides which half of a pair row it stores.
//  * A ragged last chunk is decided by cnt = min(U, N - n0), which depends on the block alone: it is WAVE-UNIFORM, so the branch
//    between the whole chunk (emit_chunk: 8-byte stores or 16-byte pair rows) and the ragged one (8-byte stores) never splits a
//    wavefront, and both lanes of a pair are on the same side of it.
//
// Host side: the workgroup size and grid of these kernels, and the runtime-bool -> template-argument dispatch of their launches.
#pragma once
#include <type_traits>

#include "mxg_common.h"
#include "mxg_gate.h"

namespace mxg {
namespace {

// true where the whole wavefront is past the bank: the kernel returns (after its last __syncthreads)
__device__ __forceinline__ bool bank_wave_idle(size_t gid, size_t V) { return (gid & ~(size_t)63) >= V; }

// the lane's voice; a surplus lane shadows voice V-1 (mxg_gate.h), with pair rows the voice of its parity in the last pair
template <bool PX>
__device__ __forceinline__ size_t bank_voice(size_t gid, size_t V) {
    return PX ? (gid < V ? gid : V - 2 + (gid & 1)) : live_voice(gid, V);
}

// rows 0 .. U-1 of the input stream p = in + v (doubles, or the int32 rand() draws), before the loop
template <typename T, int U>
__device__ __forceinline__ void rows_first(T (&xn)[U], const T *__restrict__ p, size_t V, size_t N) {
#pragma unroll
    for (int i = 0; i < U; i++) {
        const size_t m = (size_t)i < N ? (size_t)i : N - 1;
        xn[i] = p[m * V];
    }
}

// at the top of chunk n0: xc = this chunk's rows, xn = the request for the next chunk's, a chunk ahead of the stores
template <typename T, int U>
__device__ __forceinline__ void rows_next(T (&xc)[U], T (&xn)[U], const T *__restrict__ p, size_t V, size_t N, size_t n0) {
#pragma unroll
    for (int i = 0; i < U; i++) {
        xc[i] = xn[i];
        const size_t m = (n0 + U + i < N) ? n0 + U + i : N - 1;
        xn[i] = p[m * V];
    }
}

// a whole chunk (cnt == U) through emit_chunk; the first cnt rows of a ragged last one by 8-byte stores.  op advances by cnt rows.
template <bool PX, int U>
__device__ __forceinline__ void emit_rows(double *&op, size_t V, const double (&y)[U], int cnt, int px_store) {
    if (cnt == U) {
        emit_chunk<PX>(op, V, y, px_store);
    } else {
#pragma unroll
        for (int i = 0; i < U; i++) {
            if (i >= cnt) break;
            *op = y[i];
            op += V;
        }
    }
}

// The workgroup of a per-voice kernel: the knob voice_block (mxg_tune takes 64 .. 1024 in multiples of 64), at most 256 lanes (the
// kernels are compiled with __launch_bounds__(256)): 64, 128, 192 or 256.  small64: banks of up to 16 384 voices run in workgroups
// of one wavefront, so that they still spread over the compute units -- polyblep_kernel, drum_kernel and clock_kernel, line_kernel
// (shaper.hip) and analysis_kernel pass true.  tests/test_gpu_workgroups.py runs every caller at every size.
inline int voice_block(size_t V, bool small64 = false) {
    int block = tune_get("voice_block");
    if (block > 256) block = 256;
    if (small64 && V <= 16384) block = 64;
    return block;
}
inline dim3 voice_grid(size_t V, int block) { return dim3((unsigned)((V + block - 1) / block)); }

// with_bools(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...): a generic lambda reads each flag's
// ::value as a template argument, and every combination is instantiated -- what an if-ladder over the flags spells out by hand.
template <typename F>
void with_bools(F &&f) { f(); }
template <typename F, typename... Rest>
void with_bools(F &&f, bool b, Rest... rest) {
    if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

}  // namespace
}  // namespace mxg
