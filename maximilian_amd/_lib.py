"""ctypes binding of libmaxigpu.so (the C-ABI declared in include/maxigpu.h).

There is deliberately no fallback: if the HIP library has not been built, or no HIP
device is visible when a compute entry point is called, this raises.  Nothing in this
package imports or calls the CPU oracle under oracle/.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_size_t, c_uint32, c_void_p, POINTER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MXG_LIB") or os.path.join(_HERE, "libmaxigpu.so")  # (MXG_LIB: an A/B build of the same ABI, tools only)

_lib = None

# name -> (restype, argtypes); mirrors include/maxigpu.h one to one.
SIGNATURES = {
    "mxg_init": (c_int, [c_int]),
    "mxg_last_error": (c_char_p, []),
    "mxg_version": (c_char_p, []),
    "mxg_settings": (c_int, [c_size_t, c_size_t, c_size_t]),
    "mxg_sample_rate": (c_size_t, []),
    "mxg_malloc": (c_void_p, [c_size_t]),
    "mxg_free": (c_int, [c_void_p]),
    "mxg_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mxg_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mxg_memcpy_h2d_async": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mxg_memcpy_d2h_async": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mxg_memcpy_d2d_async": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mxg_host_alloc": (c_void_p, [c_size_t]),
    "mxg_host_free": (c_int, [c_void_p]),
    "mxg_event_sync": (c_int, [c_void_p]),
    "mxg_event_query": (c_int, [c_void_p]),
    "mxg_stream_wait_event": (c_int, [c_void_p, c_void_p]),
    "mxg_host_render": (c_int, [c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    "mxg_memset": (c_int, [c_void_p, c_int, c_size_t, c_void_p]),
    "mxg_stream_create": (c_void_p, []),
    "mxg_stream_destroy": (c_int, [c_void_p]),
    "mxg_stream_sync": (c_int, [c_void_p]),
    "mxg_sync": (c_int, []),
    "mxg_event_create": (c_void_p, []),
    "mxg_event_destroy": (c_int, [c_void_p]),
    "mxg_event_record": (c_int, [c_void_p, c_void_p]),
    "mxg_event_elapsed_ms": (c_int, [c_void_p, c_void_p, POINTER(c_float)]),
    "mxg_prof_enable": (c_int, [c_int]),
    "mxg_prof_reset": (c_int, []),
    "mxg_prof_count": (c_int, []),
    "mxg_prof_read": (c_int, [c_int, POINTER(c_char_p), POINTER(c_double), POINTER(c_size_t)]),
    "mxg_prof_overhead_ms": (c_int, [c_void_p, c_int, POINTER(c_double)]),
    "mxg_tune": (c_int, [c_char_p, c_int]),
    "mxg_last_async_error": (c_int, []),
    "mxg_osc_render": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_int, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_osc_render_pitch": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_int, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mxg_osc_render_mix": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_osc_mix_groups": (c_size_t, [c_size_t]),
    "mxg_osc_render_mix_rows": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_mix_rows_sum": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p]),
    "mxg_osc_tables_groups": (c_size_t, [c_size_t]),
    "mxg_osc_render_tables": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_osc_render_tables_ex": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_int, c_void_p]),
    "mxg_filter_render": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_int, c_void_p,
                                  c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_filter_render_coefs": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_filter_coeffs_host": (c_int, [c_int, c_size_t, c_void_p, c_void_p, c_void_p]),
    "mxg_env_render": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_int, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_env_coeff_host": (c_double, [c_int, c_double]),
    "mxg_mtof_host": (c_double, [c_int]),
    "mxg_voice_render": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "mxg_voice_render_mix_rows": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_voice_render_mix": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_envgen_stages_host": (c_int, [c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_envgen_render": (c_int, [c_size_t, c_size_t, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "mxg_filter2_render": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_svf_coeffs_host": (c_int, [c_size_t, c_void_p, c_void_p, c_void_p]),
    "mxg_biquad_coeffs_host": (c_int, [c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_mix_stereo": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_mix_bus": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p]),
    "mxg_osc_noise": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_sample_render_frompos": (c_int, [c_size_t, c_size_t, c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    "mxg_sample_render_trig": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_size_t, c_int, c_void_p, c_void_p,
                                       c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "mxg_delay_render": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "mxg_flanger_render": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                   c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_chorus_render": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                  c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "mxg_dynamics_render": (c_int, [c_size_t, c_size_t] + [c_void_p] * 8 + [c_int] + [c_void_p] * 5 + [c_int, c_void_p, c_size_t,
                                                                                                       c_void_p, c_size_t] + [c_void_p] * 11),
    "mxg_rms_render": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "mxg_envgen_set_time_host": (c_int, [c_void_p, c_size_t, c_size_t, c_double]),
    "mxg_envgen_set_level_host": (c_int, [c_void_p, c_size_t, c_size_t, c_double]),
    "mxg_envgen_set_curve_host": (c_int, [c_void_p, c_size_t, c_size_t, c_double]),
    "mxg_reverb_layout_host": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_reverb_render": (c_int, [c_int, c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_dattaro_layout_host": (c_int, [c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_dattaro_render": (c_int, [c_uint32, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_revnet_layout_host": (c_int, [c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_revnet_render": (c_int, [c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t] + [c_void_p] * 9),
    "mxg_seq_ratio_host": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p]),
    "mxg_seq_render": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p,
                               c_int, c_void_p, c_void_p, c_size_t, c_size_t] + [c_void_p] * 9),
    "mxg_seq_signal": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t] + [c_void_p] * 6),
    "mxg_envfollow_coeff_host": (c_double, [c_double, c_double]),
    "mxg_analysis_window_host": (c_int, [c_size_t, c_void_p, c_size_t]),
    "mxg_analysis_render": (c_int, [c_size_t, c_size_t, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t] + [c_void_p] * 7 +
                            [c_int] + [c_void_p] * 7),
    "mxg_kuramoto_render": (c_int, [c_int, c_size_t, c_size_t, c_size_t, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                            c_int, c_void_p, c_void_p, c_void_p]),
    "mxg_kuramoto_wide_render": (c_int, [c_int, c_size_t, c_size_t, c_size_t, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                 c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mxg_atan_norm_host": (c_double, [c_double]),
    "mxg_shape_render": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "mxg_xfade_render": (c_int, [c_size_t, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "mxg_select_render": (c_int, [c_int, c_size_t, c_size_t, c_size_t, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mxg_line_prepare_host": (c_int, [c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p]),
    "mxg_line_render": (c_int, [c_size_t, c_size_t, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_dyn_coeff_host": (c_double, [c_double, c_double]),
    "mxg_dyn_makeup_host": (c_double, [c_double]),
    "mxg_dyn_gate_render": (c_int, [c_size_t, c_size_t] + [c_void_p] * 4 + [c_int] + [c_void_p] * 5),
    "mxg_dyn_gate_host": (c_int, [c_size_t, c_size_t] + [c_void_p] * 4 + [c_int] + [c_void_p] * 4),
    "mxg_dyn_compress_render": (c_int, [c_size_t, c_size_t] + [c_void_p] * 6 + [c_int] + [c_void_p] * 4),
    "mxg_dyn_compress_host": (c_int, [c_size_t, c_size_t] + [c_void_p] * 6 + [c_int] + [c_void_p] * 3),
    "mxg_envelope_trigger_host": (c_int, [c_size_t] + [c_void_p] * 6),
    "mxg_envelope_line_render": (c_int, [c_size_t, c_size_t, c_size_t] + [c_void_p] * 9),
    "mxg_envelope_line_host": (c_int, [c_size_t, c_size_t, c_size_t] + [c_void_p] * 8),
    "mxg_lag_render": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mxg_lag_host": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "mxg_scan_long_render": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_scan_long_host": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_scan_long_render_swept": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "mxg_scan_long_swept_host": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mxg_map_range_host": (c_int, [c_int, c_size_t, c_void_p, c_void_p]),
    "mxg_map_render": (c_int, [c_int, c_size_t, c_size_t] + [c_void_p] * 5),
    "mxg_map_host": (c_int, [c_int, c_size_t, c_size_t] + [c_void_p] * 4),
    "mxg_polyblep_render": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_int, c_void_p, c_double, c_void_p, c_void_p, c_void_p]),
    "mxg_polyblep_host": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_int, c_void_p, c_double, c_void_p, c_void_p]),
    "mxg_drum_render": (c_int, [c_int, c_int, c_size_t, c_size_t, c_void_p, c_int] + [c_void_p] * 13),
    "mxg_drum_host": (c_int, [c_int, c_int, c_size_t, c_size_t, c_void_p, c_int] + [c_void_p] * 12),
    "mxg_clock_render": (c_int, [c_size_t, c_size_t] + [c_void_p] * 7),
    "mxg_clock_host": (c_int, [c_size_t, c_size_t] + [c_void_p] * 6),
    "mxg_atoms_bank_create": (c_void_p, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t]),
    "mxg_atoms_bank_create_host": (c_void_p, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t]),
    "mxg_atoms_bank_destroy": (c_int, [c_void_p]),
    "mxg_atoms_raw_append": (c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_uint32)]),
    "mxg_atoms_add": (c_int, [c_void_p, c_size_t] + [c_void_p] * 6),
    "mxg_atoms_add_host": (c_int, [c_void_p, c_size_t] + [c_void_p] * 6),
    "mxg_atoms_fill": (c_int, [c_void_p, c_size_t, c_void_p, c_int, c_int, c_void_p]),
    "mxg_atoms_play": (c_int, [c_void_p, c_size_t, c_void_p, c_int, c_int, c_void_p]),
    "mxg_atoms_fill_host": (c_int, [c_void_p, c_size_t, c_void_p, c_int, c_int]),
    "mxg_atoms_play_host": (c_int, [c_void_p, c_size_t, c_void_p, c_int, c_int]),
    "mxg_atoms_state": (c_int, [c_void_p] * 7),
    "mxg_atoms_gabor_host": (c_int, [c_float, c_float, c_uint32, c_float, c_float, c_void_p]),
    "mxg_sample_upload": (c_void_p, [c_void_p, c_size_t]),
    "mxg_sample_free": (c_int, [c_void_p]),
    "mxg_sample_render": (c_int, [c_int, c_size_t, c_size_t, c_void_p, c_size_t, c_int, c_void_p, c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_sample_pool_alloc": (c_void_p, [c_size_t, c_size_t, POINTER(c_size_t)]),
    "mxg_sample_pool_free": (c_int, [c_void_p]),
    "mxg_sample_pool_stride": (c_size_t, [c_size_t]),
    "mxg_sample_pool_lengths": (c_int, [c_size_t, c_size_t, c_void_p, c_void_p]),
    "mxg_looprec_render": (c_int, [c_size_t, c_size_t, c_void_p, c_size_t, c_size_t] + [c_void_p] * 3 + [c_int] + [c_void_p] * 5 + [c_int] +
                           [c_void_p] * 6),
    "mxg_looprec_host": (c_int, [c_size_t, c_size_t, c_void_p, c_size_t, c_size_t] + [c_void_p] * 3 + [c_int] + [c_void_p] * 5 + [c_int] +
                         [c_void_p] * 5),
    "mxg_looprec_piece": (c_int, []),
    "mxg_looprec_tile": (c_int, []),
    "mxg_sample_pool_normalise": (c_int, [c_size_t, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p]),
    "mxg_sample_pool_normalise_host": (c_int, [c_size_t, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    "mxg_fft_plan_create": (c_void_p, [c_int, c_int, c_int]),
    "mxg_fft_plan_destroy": (c_int, [c_void_p]),
    "mxg_fft_plan_bins": (c_int, [c_void_p]),
    "mxg_sample_load_wav": (c_void_p, [c_char_p, c_int, c_void_p, c_void_p]),
    "mxg_sample_save_wav": (c_int, [c_char_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mxg_ifft_plan_create": (c_void_p, [c_int, c_int, c_int]),
    "mxg_ifft_plan_destroy": (c_int, [c_void_p]),
    "mxg_ifft_batch": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_ifft_batch_complex": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_convolve_create": (c_void_p, [c_void_p, c_size_t, c_double, c_int, c_int]),
    "mxg_convolve_destroy": (c_int, [c_void_p]),
    "mxg_convolve_frames": (c_int, [c_void_p]),
    "mxg_convolve_impulse": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mxg_convolve_play": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    "mxg_convolve_reset": (c_int, [c_void_p]),
    "mxg_convolve_output": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "mxg_convolve_input": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mxg_convolve_bank_create": (c_void_p, [c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int]),
    "mxg_convolve_bank_destroy": (c_int, [c_void_p]),
    "mxg_convolve_bank_reset": (c_int, [c_void_p]),
    "mxg_convolve_bank_frames": (c_int, [c_void_p, c_size_t]),
    "mxg_convolve_bank_impulse": (c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    "mxg_convolve_bank_play": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    "mxg_convolve_bank_play_nv": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    "mxg_convolve_bank_mac_host": (c_int, [c_size_t, c_int, c_int] + [c_void_p] * 11 + [c_size_t, c_void_p, c_void_p]),
    "mxg_fft_bank_create": (c_void_p, [c_size_t, c_int, c_int, c_int]),
    "mxg_fft_bank_destroy": (c_int, [c_void_p]),
    "mxg_fft_bank_reset": (c_int, [c_void_p]),
    "mxg_fft_bank_pos": (c_int, [c_void_p]),
    "mxg_fft_bank_process": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_ifft_bank_create": (c_void_p, [c_size_t, c_int, c_int, c_int]),
    "mxg_ifft_bank_destroy": (c_int, [c_void_p]),
    "mxg_ifft_bank_reset": (c_int, [c_void_p]),
    "mxg_ifft_bank_pos": (c_int, [c_void_p]),
    "mxg_ifft_bank_buffer": (c_void_p, [c_void_p]),
    "mxg_ifft_bank_process": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    "mxg_spectral_bank_plan_host": (c_int, [c_int, c_int, c_int, c_int, c_int, c_size_t] + [c_void_p] * 5),
    "mxg_sampler_freq_host": (c_int, [c_size_t, c_void_p, c_size_t, c_void_p]),
    "mxg_sampler_render": (c_int, [c_size_t, c_size_t, c_int, c_int, c_void_p, c_size_t] + [c_void_p] * 12),
    "mxg_fft_features": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_fft_batch": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p]),
    "mxg_mfcc_plan_create": (c_void_p, [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, c_double, c_double]),
    "mxg_mfcc_plan_destroy": (c_int, [c_void_p]),
    "mxg_mfcc_plan_tables": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mxg_mfcc_plan_matrix_tables": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mxg_mfcc_batch": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p,
                               c_int, c_void_p]),
    "mxg_bark_plan_create": (c_void_p, [ctypes.c_uint, ctypes.c_uint]),
    "mxg_bark_plan_destroy": (c_int, [c_void_p]),
    "mxg_bark_plan_limits": (c_int, [c_void_p, c_void_p]),
    "mxg_bark_batch": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_octave_plan_create": (c_void_p, [ctypes.c_float, c_int, c_int]),
    "mxg_octave_plan_destroy": (c_int, [c_void_p]),
    "mxg_octave_plan_averages": (c_int, [c_void_p]),
    "mxg_octave_plan_map": (c_int, [c_void_p, c_void_p]),
    "mxg_octave_batch": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, ctypes.c_float, ctypes.c_float, c_int,
                                 ctypes.c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mxg_fft_mfcc_batch": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "mxg_grain_plan_create": (c_void_p, [c_int, c_double, c_int]),
    "mxg_grain_plan_destroy": (c_int, [c_void_p]),
    "mxg_grain_plan_window": (c_int, [c_void_p, c_void_p]),
    "mxg_granular_render": (c_int, [c_void_p, c_int, c_size_t, c_size_t, c_void_p, c_size_t, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "mxg_granular_render_mix": (c_int, [c_void_p, c_int, c_size_t, c_size_t, c_void_p, c_size_t, c_int, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    "mxg_granular_pool_render": (c_int, [c_void_p, c_int, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p, c_void_p,
                                         c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "mxg_granular_pool_host": (c_int, [c_void_p, c_int, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p, c_void_p,
                                       c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p,
                                       c_void_p]),
    "mxg_stretch_loop_host": (c_int, [ctypes.c_uint64, c_double, c_double, c_void_p, c_void_p]),
    "mxg_comm_unique_id": (c_int, [c_void_p]),
    "mxg_comm_create": (c_void_p, [c_void_p, c_int, c_int]),
    "mxg_comm_destroy": (c_int, [c_void_p]),
    "mxg_comm_rank": (c_int, [c_void_p]),
    "mxg_comm_size": (c_int, [c_void_p]),
    "mxg_comm_reduce": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "mxg_mix_reduce": (c_int, [c_void_p, c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_int, c_void_p]),
    "mxg_granular_retries": (c_int, []),
    "mxg_mixq_create": (c_void_p, [c_void_p, c_size_t, c_int, c_int]),
    "mxg_mixq_create_grouped": (c_void_p, [c_void_p, c_size_t, c_int, c_int, c_size_t]),
    "mxg_mixq_destroy": (c_int, [c_void_p]),
    "mxg_mixq_set_sink": (c_int, [c_void_p, c_void_p, c_size_t]),
    "mxg_mixq_slot": (c_void_p, [c_void_p, c_void_p]),
    "mxg_mixq_push": (c_int, [c_void_p, c_void_p]),
    "mxg_mixq_flush": (c_int, [c_void_p, c_void_p]),
    "mxg_mixq_result": (c_void_p, [c_void_p, POINTER(c_size_t), POINTER(c_size_t)]),
    "mxg_mixq_release": (c_int, [c_void_p, c_void_p]),
    "mxg_i64_from_i32": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mxg_i32_from_i64": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
}


# measurement only (include/maxicalib.h, libmaxicalib.so): the bandwidth probes of bench.py and tools/*_ceiling.py
CALIB_PATH = os.path.join(_HERE, "libmaxicalib.so")
CALIB_SIGNATURES = {
    "mxg_calib_fill": (c_int, [c_void_p, c_size_t, c_int, c_void_p]),
    "mxg_calib_fill_ex": (c_int, [c_void_p, c_size_t, c_size_t, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mxg_calib_read_ex": (c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
}
_calib = None


def calib():
    """Load libmaxicalib.so (after libmaxigpu.so, whose runtime it links against)."""
    global _calib
    if _calib is None:
        lib()
        C = ctypes.CDLL(CALIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in CALIB_SIGNATURES.items():
            fn = getattr(C, name)
            fn.restype = res
            fn.argtypes = args
        _calib = C
    return _calib


class MaxiGpuError(RuntimeError):
    pass


def lib():
    """Load libmaxigpu.so once (importing torch first, when present, so that both share one
    HIP runtime -- the library resolves libamdhip64.so.7 by SONAME)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MaxiGpuError(
            "libmaxigpu.so is not built (%s). Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C maximilian_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    try:
        import torch  # noqa: F401  (shared HIP runtime; optional)
    except Exception:  # pragma: no cover
        pass
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError here == header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(status, what=""):
    if status < 0:
        msg = lib().mxg_last_error().decode("utf-8", "replace")
        raise MaxiGpuError("%s failed (%d): %s" % (what or "libmaxigpu call", status, msg))
    return status
