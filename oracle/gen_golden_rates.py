#!/usr/bin/env python3
"""oracle/gen_golden_rates.py -- TEST INFRASTRUCTURE.  Reference outputs at sample rates other than 44.1 kHz ->
tests/golden/rates.npz (+ MANIFEST entry): tests/rates_cases.golden_run() -- one small case per core family and rate, inputs
regenerated from seeds -- driven through pyoracle.reference(), the compiled UNMODIFIED reference (oracle/_ref/libmaxiref.so, built
only where /root/reference exists).  tests/test_rates_cpu.py runs the same function on the plain-C port and compares bit for bit,
which pins the port where oracle/_ref is absent.  The file holds data only: keys "sr<rate>/<case>", outputs as arrays."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import rates_cases as rc
    from oracle import pyoracle

    if not (os.path.isdir("/root/reference") and pyoracle.have_reference()):
        sys.exit("needs /root/reference and oracle/_ref (make -C oracle all)")
    R = pyoracle.reference()
    assert R.kind == "reference"
    data = {}
    for sr in rc.RATES + (192000,):
        for k, v in rc.golden_run(R, sr).items():
            data["sr%d/%s" % (sr, k)] = v
    path = os.path.join(GOLD, "rates.npz")
    np.savez_compressed(path, **data)
    sha = hashlib.sha256()
    for k in sorted(data):
        sha.update(k.encode())
        sha.update(np.ascontiguousarray(data[k]).tobytes())
    man_path = os.path.join(GOLD, "MANIFEST.json")
    man = json.load(open(man_path))
    man.setdefault("files", {})["rates.npz"] = (
        "tests/rates_cases.golden_run() through oracle/_ref/libmaxiref.so at maxiSettings::sampleRate 48000, 96000, 22050, 7919 and "
        "192000: oscillators, maxiFilter, maxiEnv, the fused voice, maxiSVF / maxiBiquad, maxiEnvGen, playAtSpeed, maxiSampler, the "
        "mel filter bank + mfcc, the spectral centroid and the granular players (last rows + final state); %d arrays, sha256 of keys "
        "+ data %s" % (len(data), sha.hexdigest()))
    json.dump(man, open(man_path, "w"), indent=1, sort_keys=True)
    print("wrote rates.npz: %d arrays, %d bytes" % (len(data), os.path.getsize(path)))


if __name__ == "__main__":
    main()
