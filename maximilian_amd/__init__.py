"""maximilian_amd -- MI355X (gfx950) voice-bank renderer behind the Maximilian class API.

The product is the C-ABI library `libmaxigpu.so` (include/maxigpu.h) built from
maximilian_amd/csrc/*.hip, and the C++ host facade include/maximilian_bank.hpp.  This Python
package is the thin host-side mirror used by the tests and bench.py: device buffers, and
`*Bank` classes whose methods carry the reference's names (maxiOsc::sinebuf -> maxiOscBank.sinebuf).
"""
from ._lib import LIB_PATH, MaxiGpuError, calib, lib  # noqa: F401
from .banks import (DeviceBuffer, maxiSettings, maxiOscBank, maxiFilterBank, maxiEnvBank,  # noqa: F401
                    maxiVoiceBank, maxiMixBank, maxiDelaylineBank, maxiSampleBank, maxiDCBlockerBank,
                    maxiSVFBank, maxiBiquadBank, maxiEnvGenBank, maxiSamplerBank, maxiFlangerBank, maxiChorusBank, maxiDynamicsBank,
                    maxiRMSBank, maxiSatReverbBank, maxiFreeVerbBank, maxiFreeVerbStereoBank, reverb_layout, maxiDattaroReverbBank,
                    dattaro_layout, maxiReverbNetBank, revnet_layout, maxiSeqBank, maxiTriggerBank, maxiCounterBank, maxiStepBank, maxiIndexBank,
                    maxiZXToPulseBank, seq_table, seq_ratio_tables, maxiAnalysisBank, maxiKuramotoBank, maxiKuramotoWideBank, envfollow_coeff, analysis_want, OSC_WAVEFORMS,
                    maxiShaperBank, maxiXFadeBank, maxiSelectBank, maxiLineBank, atan_norm, SHAPE_MODES,
                    maxiDynBank, maxiEnvelopeBank, maxiLagExpBank, maxiMapBank, dyn_coeff, dyn_makeup, MAP_MODES, CLASSIC_PS,
                    maxiPolyBLEPBank, polyblep_sync, POLYBLEP_WAVEFORMS,
                    maxiKickBank, maxiSnareBank, maxiHatsBank, maxiClockBank, DRUM_KINDS,
                    maxiAtomBank, ATOM_KINDS, ATOM_ONSETS, maxiLooperBank, LOOPER_PLAY, maxiLongScanBank, LONG_SCAN_KINDS,
                    sweep_lores, sweep_hires, sweep_lag, FILTER_KINDS, SAMPLE_MODES)
from .spectral import (maxiConvolve, maxiConvolveBank, maxiFFT, maxiIFFT, maxiFFTBank, maxiIFFTBank, spectral_bank_plan, maxiMFCC, maxiBarkBatch, maxiOctaveBatch, frames_in_stream,  # noqa: F401
                       padded_stream)
from .grains import maxiTimeStretchBank, maxiStretchBank, maxiPitchShiftBank, maxiGrainPoolBank, WINDOWS  # noqa: F401
