"""CPU (-m "not gpu"): the K22 entry points are declared in include/maxigpu.h, exported by the library and bound by the Python
package; the kind and onset numbers agree in the header, the arithmetic header and the package; the bank classes are present in the
package and in the C++ facade; the calls refuse bad arguments with MXG_ERR_INVALID and a message that names the argument -- a negative
length, a NaN frequency, a raw offset outside the pool, an unknown kind, stream or onset, a host bank handed to a device call -- and
change nothing when they do; the player's overflow has its own asynchronous error code."""
import ctypes
import os
import re

import numpy as np

import atoms_host as ah
from conftest import ROOT

NEW = ["mxg_atoms_bank_create", "mxg_atoms_bank_create_host", "mxg_atoms_bank_destroy", "mxg_atoms_raw_append", "mxg_atoms_add",
       "mxg_atoms_add_host", "mxg_atoms_fill", "mxg_atoms_play", "mxg_atoms_fill_host", "mxg_atoms_play_host", "mxg_atoms_state",
       "mxg_atoms_gabor_host"]
MXG_ERR_INVALID = -1


def test_symbols_declared_exported_and_bound():
    import maximilian_amd as m
    hdr = open(os.path.join(ROOT, "include", "maxigpu.h")).read()
    arith = open(os.path.join(ROOT, "maximilian_amd", "csrc", "mxg_atoms.h")).read()
    L = ctypes.CDLL(m.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in m._lib.SIGNATURES, name
    for name, val in (("MXG_ATOM_GABOR", ah.GABOR), ("MXG_ATOM_RAW", ah.RAW), ("MXG_ATOM_ONSET_BLOCK", ah.ONSET_BLOCK),
                      ("MXG_ATOM_ONSET_SAMPLE", ah.ONSET_SAMPLE), ("MXG_ATOMS_PIECE", ah.PIECE)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr) and re.search(r"#define %s %d\b" % (name, val), arith), name
    assert m.ATOM_KINDS == {"gabor": ah.GABOR, "raw": ah.RAW} and m.ATOM_ONSETS == {"block": ah.ONSET_BLOCK, "sample": ah.ONSET_SAMPLE}
    assert hasattr(m, "maxiAtomBank")
    assert re.search(r"\bclass maxiAtomBank\b", open(os.path.join(ROOT, "include", "maximilian_bank.hpp")).read())
    src = open(os.path.join(ROOT, "maximilian_amd", "csrc", "atoms.hip")).read()
    assert "atomic" not in src.split("atoms_render_kernel(")[1].split("// ---- the bank's memory")[0], "the render adds in list order, without atomics"
    assert re.search(r"ASYNC_ATOMS_OVERFLOW\s*=\s*\d+", open(os.path.join(ROOT, "maximilian_amd", "csrc", "mxg_common.h")).read())


def _p(a):
    return None if a is None else a.ctypes.data


def test_creation_refuses_bad_books():
    import maximilian_amd as m
    L = m.lib()
    start = np.array([0, 1], np.int64)
    ns = np.array([512], np.uint32)
    good = np.array([[0], [64], [20], [0.5], [0]], np.float32)

    def make(book=good, start=start, ns=ns, S=1, Q=4, raw=None, raw_len=0, fn=L.mxg_atoms_bank_create_host):
        return fn(S, Q, _p(start), _p(np.ascontiguousarray(book, np.float32)), _p(ns), _p(raw), raw_len)

    b = make()
    assert b
    L.mxg_atoms_bank_destroy(b)
    bad = [(dict(S=0), b"S and Q"), (dict(Q=0), b"S and Q"), (dict(start=np.array([1, 1], np.int64)), b"book_start"),
           (dict(start=np.array([0, -1], np.int64)), b"book_start"), (dict(ns=np.array([0], np.uint32)), b"numSamples"),
           (dict(book=[[0], [-64], [20], [0.5], [0]]), b"length"), (dict(book=[[0], [22050], [20], [0.5], [0]]), b"length"),
           (dict(book=[[0], [0], [20], [0.5], [0]]), b"outside [1"), (dict(book=[[0], [np.nan], [20], [0.5], [0]]), b"length"),
           (dict(book=[[-1], [64], [20], [0.5], [0]]), b"position"), (dict(book=[[np.nan], [64], [20], [0.5], [0]]), b"position"),
           (dict(book=[[0], [64], [20], [np.nan], [0]]), b"frequency"), (dict(book=[[0], [64], [np.inf], [0.5], [0]]), b"finite"),
           (dict(book=[[0], [64], [20], [0.5], [np.nan]]), b"finite"), (dict(book=[[0], [64], [20], [0.5], [1e6]]), b"2^19"),
           (dict(raw=None, raw_len=4), b"raw pool")]
    for kw, word in bad:
        for fn in (L.mxg_atoms_bank_create_host, L.mxg_atoms_bank_create):      # (the checks run before the device is touched)
            assert not make(fn=fn, **kw), kw
            assert word in L.mxg_last_error(), (kw, L.mxg_last_error())


def test_calls_refuse_bad_arguments_and_change_nothing():
    import maximilian_amd as m
    L = m.lib()
    raw = np.arange(16, dtype=np.float32)
    b = L.mxg_atoms_bank_create_host(2, 3, None, None, None, _p(raw), len(raw))
    assert b

    def add(stream=0, kind=ah.RAW, length=4, offset=0, par=(440.0, 44100.0, 0.0, 1.0), raw_off=0, fn=L.mxg_atoms_add_host, drop=()):
        a = dict(stream=np.array([stream], np.int32), kind=np.array([kind], np.int32), length=np.array([length], np.int64).astype(np.uint32),
                 offset=np.array([offset], np.uint32), par=np.array([par], np.float32), raw_off=np.array([raw_off], np.uint32))
        for k in drop:
            a[k] = None
        return fn(b, 1, _p(a["stream"]), _p(a["kind"]), _p(a["length"]), _p(a["offset"]), _p(a["par"]), _p(a["raw_off"]))

    bad = [(dict(length=-3), b"negative length"), (dict(kind=ah.GABOR, length=-3), b"negative length"), (dict(raw_off=13), b"outside the pool"),
           (dict(raw_off=17, length=0), b"outside the pool"), (dict(kind=ah.GABOR, par=(np.nan, 44100.0, 0.0, 1.0)), b"finite"),
           (dict(kind=ah.GABOR, par=(440.0, 44100.0, np.inf, 1.0)), b"finite"), (dict(kind=ah.GABOR, length=0), b"outside [1"),
           (dict(kind=ah.GABOR, length=22050), b"outside [1"), (dict(kind=ah.GABOR, par=(0.0, 0.0, 0.0, 1.0)), b"2^19"),
           (dict(kind=ah.GABOR, par=(20000.0, 1.0, 0.0, 1.0), length=64), b"2^19"), (dict(kind=2), b"kind"), (dict(kind=-1), b"kind"),
           (dict(stream=2), b"stream"), (dict(stream=-1), b"stream"), (dict(kind=ah.GABOR, drop=("par",)), b"parameter rows"),
           (dict(drop=("raw_off",)), b"raw_off"), (dict(drop=("stream",)), b"null"), (dict(fn=L.mxg_atoms_add), b"host bank")]
    for kw, word in bad:
        assert add(**kw) == MXG_ERR_INVALID, kw
        assert word in L.mxg_last_error(), (kw, L.mxg_last_error())
    nl = np.zeros(2, np.int32)
    assert L.mxg_atoms_state(b, None, None, _p(nl), None, None, None) == 0 and nl.tolist() == [0, 0], "a refused call adds nothing"
    assert add(raw_off=12) == 0 and add(kind=ah.GABOR, length=64, offset=5) == 0 and add(raw_off=16, length=0) == 0 and add(stream=1, kind=ah.GABOR, length=2) == 0
    assert add() == MXG_ERR_INVALID and b"more than Q" in L.mxg_last_error()
    out = np.zeros((2, 8), np.float32)
    for fn in (L.mxg_atoms_fill_host, L.mxg_atoms_play_host):
        for args, word in (((b, 0, _p(out), 0, 1), b"N must"), ((b, (1 << 24) + 1, _p(out), 0, 1), b"N must"), ((b, 8, None, 0, 1), b"output"),
                           ((b, 8, _p(out), 2, 1), b"onset"), ((None, 8, _p(out), 0, 1), b"null bank")):
            assert fn(*args) == MXG_ERR_INVALID and word in L.mxg_last_error(), (fn, args)
    for fn in (L.mxg_atoms_fill, L.mxg_atoms_play):
        assert fn(None, 8, _p(out), 0, 1, None) == MXG_ERR_INVALID and b"null bank" in L.mxg_last_error()
        assert fn(b, 8, _p(out), 0, 1, None) == MXG_ERR_INVALID and b"host bank" in L.mxg_last_error()
    assert L.mxg_atoms_fill_host(b, 8, _p(out), 0, 0) == 0
    gab = np.zeros(64, np.float32)
    assert L.mxg_atoms_gabor_host(440.0, 44100.0, 64, 0.0, 1.0, _p(gab)) == 0
    exp = gab[:8].copy()
    exp[:4] = raw[12:16] + gab[:4]          # queue order: the raw atom, then the Gabor atom (offset 5: it starts at buffer[0] all the same)
    assert np.array_equal(out[0].view(np.uint32), exp.view(np.uint32)) and out[1, 1] != 0 and (out[1, 2:] == 0).all()
    off = ctypes.c_uint32(99)
    assert L.mxg_atoms_raw_append(b, _p(raw), 16, ctypes.byref(off)) == 0 and off.value == 16
    assert L.mxg_atoms_raw_append(b, None, 4, ctypes.byref(off)) == MXG_ERR_INVALID
    a = np.zeros(4, np.float32)
    for args, word in (((np.nan, 44100.0, 4, 0.0, 1.0), b"NaN"), ((440.0, 44100.0, 0, 0.0, 1.0), b"length"), ((440.0, 44100.0, 22050, 0.0, 1.0), b"length"),
                       ((440.0, 44100.0, 4, 1e7, 1.0), b"2^19")):
        assert L.mxg_atoms_gabor_host(*args, _p(a)) == MXG_ERR_INVALID and word in L.mxg_last_error(), args
    assert L.mxg_atoms_gabor_host(440.0, 44100.0, 4, 0.0, 1.0, None) == MXG_ERR_INVALID
    L.mxg_atoms_bank_destroy(b)
    assert L.mxg_atoms_bank_destroy(None) == 0
