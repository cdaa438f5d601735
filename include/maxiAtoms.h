// include/maxiAtoms.h -- DROP-IN for the reference's src/libs/maxiAtoms.h (the portable branch of maxiAtoms.cpp): maxiAtomTypes,
// maxiAtom, maxiGaborAtom, maxiCollider, maxiAccelerator, maxiAtomBook and maxiAtomBookPlayer with the reference's public members and
// signatures, over the atoms bank of the C-ABI (K22, mxg_atoms_*: include/maxigpu.h).
//   maxiCollider::createGabor   callable (in the reference it is `inline` inside the .cpp and out of a patch's reach) and evaluated on
//                               the host: mxg_atoms_gabor_host.  The reference's static envCache is not carried.
//   maxiAccelerator             one stream of a bank.  addAtom(atom, offset) copies the floats into the bank's raw pool and queues them;
//                               fillNextBuffer(buffer, n) renders ON THE DEVICE, on top of what buffer holds, in queue order -- the
//                               reference's float sum, bit for bit -- and the bank keeps (startTime, pos) per entry by the reference's
//                               rules, so an entry stalls exactly where the reference's does for any sequence of buffer lengths.
//                               Not copyable (it owns a device bank).  More than 4096 queued atoms: the call is refused, loudly.
//   maxiAtomBookPlayer::play    the reference's walk over the book; the Gabor atoms are queued BY PARAMETER and synthesised on the
//                               device.  The offset handed to the queue is |looped - position|: where the
//                               reference's `loopedSamplePos - atom->position` is non-negative it is that value, where it is negative
//                               -- undefined in the reference -- it is the atom's distance into this buffer.
#pragma once
#include <cstdio>
#include <vector>

#include "maximilian.h"
#include "maxiGrains.h"

typedef vector<float> flArr;

enum maxiAtomTypes { GABOR };

struct maxiAtom {
    maxiAtomTypes atomType;
    float length;
    float position;
    float amp;
    static bool atomSortPositionAsc(maxiAtom *a, maxiAtom *b) { return a->position < b->position; }
};

struct maxiGaborAtom : maxiAtom {
    float frequency;
    float phase;
};

class maxiCollider {
public:
    static inline void createGabor(flArr &atom, const float freq, const float sampleRate, const unsigned int length, float phase,
                                   const float kurtotis, const float amp) {
        (void)kurtotis;  // unused in the reference too
        atom.resize(length);
        if (length && mxg_atoms_gabor_host(freq, sampleRate, length, phase, amp, atom.data()) < 0)
            std::fprintf(stderr, "ERROR maxiCollider::createGabor: %s\n", mxg_last_error());
    }
};

class maxiAccelerator {
public:
    maxiAccelerator() { sampleIdx = 0; }
    ~maxiAccelerator() { release(); }
    maxiAccelerator(const maxiAccelerator &) = delete;
    maxiAccelerator &operator=(const maxiAccelerator &) = delete;

    void addAtom(flArr &atom, unsigned int offset = 0) {
        if (!ready()) return;
        uint32_t at = 0;
        if (mxg_atoms_raw_append(bank, atom.data(), atom.size(), &at) < 0) return complain("addAtom");
        rawFloats += atom.size();
        const int32_t stream = 0, kind = MXG_ATOM_RAW;
        const uint32_t length = (uint32_t)atom.size();
        if (mxg_atoms_add(bank, 1, &stream, &kind, &length, &offset, nullptr, &at) < 0) complain("addAtom");
    }
    void fillNextBuffer(float *buffer, unsigned int bufferLength) {
        if (!bufferLength || !ready()) return;
        if (bufferLength > devLen) {
            if (dev) mxg_free(dev);
            dev = (float *)mxg_malloc(sizeof(float) * bufferLength);
            devLen = dev ? bufferLength : 0;
            if (!dev) return complain("fillNextBuffer");
        }
        if (mxg_memcpy_h2d(dev, buffer, sizeof(float) * bufferLength, nullptr) < 0 ||
            mxg_atoms_fill(bank, bufferLength, dev, MXG_ATOM_ONSET_BLOCK, 1, nullptr) < 0 ||
            mxg_memcpy_d2h(buffer, dev, sizeof(float) * bufferLength, nullptr) < 0)
            return complain("fillNextBuffer");
        sampleIdx += bufferLength;
        // an empty queue is the moment to let go of the raw floats queued so far
        int32_t nlive = 0;
        if (rawFloats > kPoolFloats && mxg_atoms_state(bank, nullptr, nullptr, &nlive, nullptr, nullptr, nullptr) == 0 && nlive == 0) release();
    }
    inline long getSampleIdx() { return sampleIdx; }

    // (the drop-in player's way in: createGabor's arguments, synthesised on the device)
    void addGaborByParameter(float freq, float sampleRate, unsigned int length, float phase, float amp, unsigned int offset) {
        if (!ready()) return;
        const int32_t stream = 0, kind = MXG_ATOM_GABOR;
        const float par[4] = {freq, sampleRate, phase, amp};
        if (mxg_atoms_add(bank, 1, &stream, &kind, &length, &offset, par, nullptr) < 0) complain("play");
    }

private:
    static constexpr size_t kCapacity = 4096, kPoolFloats = (size_t)1 << 22;
    long sampleIdx;
    mxg_atoms_bank *bank = nullptr;
    float *dev = nullptr;
    size_t devLen = 0, rawFloats = 0;
    bool ready() {
        if (!bank) {
            bank = mxg_atoms_bank_create(1, kCapacity, nullptr, nullptr, nullptr, nullptr, 0);
            rawFloats = 0;
            if (!bank) complain("maxiAccelerator");
        }
        return bank != nullptr;
    }
    void release() {
        if (bank) mxg_atoms_bank_destroy(bank);
        bank = nullptr;
        if (dev) mxg_free(dev);
        dev = nullptr;
        devLen = 0;
    }
    void complain(const char *what) { std::fprintf(stderr, "ERROR maxiAccelerator::%s: %s\n", what, mxg_last_error()); }
};

class maxiAtomBook {
public:
    ~maxiAtomBook() {
        for (size_t i = 0; i < atoms.size(); i++) delete atoms[i];
    }
    typedef vector<maxiAtom *> maxiAtomBookData;
    unsigned int numSamples;
    unsigned int sampleRate;
    maxiAtomBookData atoms;
};

class maxiAtomBookPlayer {
public:
    maxiAtomBookPlayer() { atomIdx = 0; }
    void play(maxiAtomBook &book, maxiAccelerator &atomStream, float *output, int bufferSize) {  // maxiAtoms.cpp:198-219
        (void)output;
        long idx = atomStream.getSampleIdx();
        int loopedSamplePos = idx % book.numSamples;
        if (loopedSamplePos < bufferSize) atomIdx = 0;
        if (atomIdx < book.atoms.size()) {
            maxiGaborAtom *atom = (maxiGaborAtom *)book.atoms[atomIdx];
            while (atom->position < (idx + bufferSize) % book.numSamples) {
                float d = loopedSamplePos - atom->position;
                if (d < 0.0f) d = -d;
                atomStream.addGaborByParameter(maxiMap::linlin(atom->frequency, 0.0, 1.0, 20, 20000), 44100, atom->length, atom->phase,
                                               atom->amp / 40.0, (unsigned int)d);
                atomIdx++;
                if (book.atoms.size() == atomIdx) break;
                atom = (maxiGaborAtom *)book.atoms[atomIdx];
            }
        }
    }

private:
    unsigned int atomIdx;
};
