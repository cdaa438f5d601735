// tools/gen/atoms_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's maxiCollider,
// maxiAccelerator, maxiAtomBook and maxiAtomBookPlayer: tools/gen/gen_golden_atoms.py compiles it, together with the UNMODIFIED
// reference sources, into a shared library in a temporary directory and drives it to write tests/golden/atoms.npz.
//
// createGabor is `inline` inside the reference's maxiAtoms.cpp, so that file is included here, not linked.  Private members are read
// through -fno-access-control.
#include <cstdint>
#include <cstring>
#include <vector>

#include "maximilian.h"
#include "libs/maxiAtoms.cpp"

extern "C" {

void at_gabor(float freq, float sampleRate, unsigned length, float phase, float amp, float *out) {
    flArr atom;
    maxiCollider::createGabor(atom, freq, sampleRate, length, phase, 0.3, amp);
    memcpy(out, atom.data(), length * sizeof(float));
}

// One accelerator, optionally one book and its player, driven by a script.  ops [nops][3]:
//   0, a, b   addAtom(raw atom a, offset b)          raw atom a = raw[raw_start[a] .. raw_start[a + 1])
//   1, n, 0   fillNextBuffer(out + cursor, n); cursor += n
//   2, n, 0   player.play(book, accelerator, ., n) and then the fill, as 1
// book [5][A] rows position, length, amp, frequency, phase.  out holds the initial buffers and receives the sums.
// After every fill: rows [fill][3] sampleIdx, atomIdx, queue length; queue [fill][maxq][3] startTime, pos, size (-1 beyond the queue).
int at_run(size_t nops, const int64_t *ops, const float *raw, const int64_t *raw_start, size_t A, const float *book, unsigned numSamples,
           float *out, int64_t *rows, int64_t *queue, size_t maxq) {
    maxiAccelerator acc;
    maxiAtomBook bk;
    maxiAtomBookPlayer player;
    bk.numSamples = numSamples;
    bk.sampleRate = 44100;
    for (size_t k = 0; k < A; k++) {
        maxiGaborAtom *g = new maxiGaborAtom();
        g->atomType = GABOR;
        g->position = book[k];
        g->length = book[A + k];
        g->amp = book[2 * A + k];
        g->frequency = book[3 * A + k];
        g->phase = book[4 * A + k];
        bk.atoms.push_back(g);
    }
    size_t cursor = 0, fill = 0;
    for (size_t i = 0; i < nops; i++) {
        const int64_t op = ops[3 * i], a = ops[3 * i + 1], b = ops[3 * i + 2];
        if (op == 0) {
            flArr atom(raw + raw_start[a], raw + raw_start[a + 1]);
            acc.addAtom(atom, (unsigned)b);
            continue;
        }
        if (op == 2) player.play(bk, acc, out + cursor, (int)a);
        acc.fillNextBuffer(out + cursor, (unsigned)a);
        cursor += (size_t)a;
        rows[3 * fill] = acc.sampleIdx;
        rows[3 * fill + 1] = player.atomIdx;
        rows[3 * fill + 2] = (int64_t)acc.atomQueue.size();
        if (acc.atomQueue.size() > maxq) return -1;
        int64_t *q = queue + fill * maxq * 3;
        for (size_t j = 0; j < maxq * 3; j++) q[j] = -1;
        size_t j = 0;
        for (auto &e : acc.atomQueue) {
            q[3 * j] = e.startTime;
            q[3 * j + 1] = e.pos;
            q[3 * j + 2] = (int64_t)e.atom.size();
            j++;
        }
        fill++;
    }
    return 0;
}

}  // extern "C"
