// tests/patches/atoms_patch.cpp -- a program (its own main: the atoms classes work on whole float buffers, not in play(double*))
// around the reference's maxim.h: a maxiAtomBook of Gabor atoms on multiples of the buffer length, the maxiAtomBookPlayer that walks it
// over two and a half loops, and the maxiAccelerator it feeds -- to which raw atoms are also added by hand, one with an offset, and
// which is filled with buffers of 64 samples and, for a stretch, of 16, so that entries stall and resume.  Every buffer starts from a
// ramp, not from zero: fillNextBuffer adds.  Writes the float32 stream to argv[1].
// Compiled verbatim against include/ (host/dropin_at) and against the reference (tools/gen/gen_golden_atoms.py, tests/test_atoms_dropin_cpu.py).
#include <cstdio>
#include <vector>

#include "maximilian.h"
#include "libs/maxim.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    maxiAtomBook book;
    book.numSamples = 1024;
    book.sampleRate = 44100;
    const float rows[][5] = {{0, 63, 20, 0.02f, 0}, {0, 257, 12, 0.3f, 1}, {64, 2, 30, 0.9f, -1}, {192, 64, 25, 0.11f, 2}, {256, 65, 35, 0.05f, 0.3f},
                             {512, 1, 40, 0.5f, 0.5f}, {576, 300, 18, 0.15f, 0}, {960, 64, 40, 0.2f, 0}};
    for (auto &r : rows) {
        maxiGaborAtom *a = new maxiGaborAtom();
        a->atomType = GABOR;
        a->position = r[0], a->length = r[1], a->amp = r[2], a->frequency = r[3], a->phase = r[4];
        book.atoms.push_back(a);
    }
    maxiAtomBookPlayer player;
    maxiAccelerator acc;
    std::vector<float> stream;
    flArr click(40), ramp(100);
    for (size_t i = 0; i < click.size(); i++) click[i] = (i & 1) ? -0.5f : 0.5f;
    for (size_t i = 0; i < ramp.size(); i++) ramp[i] = 0.01f * i;
    float buffer[64];
    for (int blk = 0; blk < 40; blk++) {
        for (int i = 0; i < 64; i++) buffer[i] = 0.001f * i;
        if (blk == 3) acc.addAtom(click);
        if (blk == 5) acc.addAtom(ramp, 40);
        if (blk == 21) acc.addAtom(ramp, 63);
        player.play(book, acc, buffer, 64);
        if (blk >= 6 && blk < 8) {  // the same 64 samples as four buffers of 16: the ramp queued with offset 40 stalls and resumes
            for (int part = 0; part < 4; part++) acc.fillNextBuffer(buffer + 16 * part, 16);
        } else {
            acc.fillNextBuffer(buffer, 64);
        }
        stream.insert(stream.end(), buffer, buffer + 64);
    }
    FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    std::fwrite(stream.data(), sizeof(float), stream.size(), f);
    std::fclose(f);
    std::printf("atoms_patch: %zu samples, sampleIdx %ld\n", stream.size(), acc.getSampleIdx());
    return 0;
}
