"""ookiedokie_amd -- MI355X-native OOK receive / demodulation path.

Thin Python mirror of the reference's operator interface for the rx hot
path, bound over the C ABI of ``libookiedokie_amd.so`` with ctypes
(``include/ookiedokie_amd.h``).  Names follow the reference:

================================  ==========================================
here                              reference (OOKiedokie ``src/``)
================================  ==========================================
``Filter.load`` / ``fir_init``    ``fir_init`` (fir.h:43-55)
``Device.load`` / ``device_init`` ``device_init`` (device.h:47-55)
``Receiver.rx``                   loop body of ``ookiedokie_rx``
                                  (ookiedokie.c:243-288)
``StreamFir.filter_and_decimate`` ``fir_filter_and_decimate`` (fir.h:68-81)
``HipFileBackend``                ``sdr_<name>_{init,deinit,rx,tx,flush}``
                                  (sdr/supported_devices.h:32-48)
``Survey`` / ``suggest_threshold`` nothing: picks ``--rx-threshold``
                                  (ookiedokie_cfg.c:27) from the capture
``Spectrum`` / ``suggest_carriers`` nothing: finds the carriers' offsets
                                  (``Receiver(tune=...)``) in the capture
``Receiver.pulse_hist`` /         nothing: measures the pulse and gap lengths
``suggest_pulses``                a device file's states name (devices/README.md)
``Receiver.suggest_device`` /     nothing: writes that device file's state
``Device.from_suggestion``        machine for a sync + distance-coded remote
``Receiver.clean_edges`` /        nothing: drops glitch runs from the edge list
``clean_edges``                   before the two surveys read it
``Receiver(min_on=, min_off=)`` / nothing: the decoder itself on the cleaned
``Receiver.set_debounce``         list, so a glitch no longer costs a message
``Receiver.run_levels`` /         nothing: the peak power of every pulse and a
``Receiver.message_levels``       signal level per decoded message
``Receiver.run_moments`` /        nothing: the mean power and the carrier of every
``Receiver.message_carriers``     pulse, and which transmitter sent a message
``Receiver.bursts`` /             ``--rx-rec`` writes everything: the keyed
``Receiver.burst_samples``        stretches of a capture alone, cut on the GPU
``Receiver.burst_spectra`` /      nothing: a spectrum and the carrier of every
``suggest_burst_carriers``        burst -- which transmitter keyed when
``Receiver.burst_baseband``       nothing: the filtered, decimated signal of
                                  every burst, transmitter by transmitter
================================  ==========================================

There is no CPU fallback: the library is hand-written HIP for gfx950 and
every compute call fails loudly without a GPU (``OokdError``).  PyTorch is
only used by callers for device memory / streams / ``torch.distributed``.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libookiedokie_amd.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "ookiedokie_amd.h")

MAX_PAYLOAD_BYTES = 32
FILE_EOF = -(2 ** 31)                   # SDR_FILE_EOF, sdr.h:36
RX_EXACT_FIR = 1
RX_KEEP_FIR = 2
RX_FSM_ROUNDS = 4
RX_NO_QUIET_SKIP = 8
RX_COUNT_QUIET = 16
RX_SCAN_SIMS = 32
RX_NO_PIPELINE = 128
RX_FIR_VALU = 256
RX_SCAN_TABLES = 512
# sample format of a context's captures: neither = SC16Q11; 8-bit I,Q pairs, CS8 v = SC16Q11 16 v (HackRF .cs8),
# CU8 u = SC16Q11 16 (u - 128) (rtl_sdr .cu8)
RX_SAMPLES_CS8 = 1024
RX_SAMPLES_CU8 = 2048
RX_TUNED_FIR2 = 4096                    # tuned / carrier contexts: the fused kernel for 2 x decimate-by-2 filters
SAMPLE_FORMATS = {"sc16q11": (0, np.int16), "cs8": (RX_SAMPLES_CS8, np.int8), "cu8": (RX_SAMPLES_CU8, np.uint8)}
# front-end forms (stats["front_form"], Receiver.front_info()["form"]): OOKD_FRONT_*
FRONT_NO_FILTER = 1
FRONT_GENERIC = 2
FRONT_FIR1_VALU = 3
FRONT_FIR1_VALU_EXACT = 4
FRONT_FIR1_MFMA = 5
FRONT_FIR2_VALU = 6
FRONT_FIR2_VALU_EXACT = 7
FRONT_FIR2_MFMA = 8
FRONT_NO_FILTER_8 = 9                   # the fused forms of an 8-bit context
FRONT_FIR1_MFMA_8 = 10
FRONT_FIR2_MFMA_8 = 11
FRONT_TUNED_GENERIC = 12                # a tuned context (Receiver(tune=...)): any shape, the contract's order
FRONT_TUNED_FIR1 = 13                   # ... 1 stage, decimation 1, <= 256 taps: packed FMAs + guard band
FRONT_TUNED_MULTI = 14                  # a carrier context (Receiver(carriers=[...])): that shape, all carriers in one pass
FRONT_TUNED_FIR2 = 15                   # Receiver(..., tuned_fir2=True): 2 x decimate-by-2, packed FMAs + guard band
RX_MAX_CARRIERS = 16
SURVEY_GENERIC = 1                      # survey forms (Survey.form): OOKD_SURVEY_*; what an untuned Survey runs
SURVEY_TUNED_GENERIC = 2                # a tuned Survey (Survey(tune=...)): any shape, the contract's order
SURVEY_TUNED_FIR1 = 3                   # ... 1 stage, decimation 1, <= 256 taps: register-blocked, same histogram
SURVEY_TUNED_MULTI = 4                  # a carriers Survey (Survey(carriers=[...])): several carriers, one launch
SURVEY_TUNED_MULTI_FIR2 = 5             # ... with tuned_fir2=True on 2 x decimate-by-2 (<= 16, <= 32 taps): any stride
SURVEY_MAX_CARRIERS = 16                # OOKD_SURVEY_MAX_CARRIERS
SURVEY_MAX_STRIDE = 64                  # OOKD_SURVEY_MAX_STRIDE
LEVEL_BINS = 256                        # OOKD_LEVEL_BINS: envelope survey, four bins per octave of power
LEVEL_MIN_SEPARATION = 18               # OOKD_LEVEL_MIN_SEPARATION
LEVEL_MIN_SIDE = 512                    # OOKD_LEVEL_MIN_SIDE
SPECTRUM_BINS = 1024                    # OOKD_SPECTRUM_BINS: carrier survey, 1024-sample Hann frames
SPECTRUM_EPS = 12.0 * 10.0 / 16777216.0 # OOKD_SPECTRUM_EPS: the error bound's constant, 12 log2(1024) 2^-24
CARRIER_MIN_RATIO = 64.0                # OOKD_CARRIER_MIN_RATIO
CARRIER_MIN_SPACING = 32                # OOKD_CARRIER_MIN_SPACING
PULSE_BINS = 512                        # OOKD_PULSE_BINS: pulse survey, sixteen bins per octave of run length
PULSE_CLASS_GAP = 2                     # OOKD_PULSE_CLASS_GAP
PULSE_MAX_CLASSES = 16                  # OOKD_PULSE_MAX_CLASSES
SYMBOL_MAX_CLASSES = 16                 # OOKD_SYMBOL_MAX_CLASSES: symbol survey, ranges per level of a class table
SYMBOL_NONE = 16                        # OOKD_SYMBOL_NONE: the class of a run length inside no range
SYMBOL_KINDS = 17                       # OOKD_SYMBOL_KINDS: classes 0 .. 15 and "none", per level
FRAME_BINS = 512                        # OOKD_FRAME_BINS: distances between sync symbols, clamped to 511
ROLE_OTHER, ROLE_SYNC, ROLE_ZERO, ROLE_ONE = 0, 1, 2, 3         # OOKD_ROLE_*
CODING_OK, CODING_KINDS, CODING_NOT_DISTANCE, CODING_AMBIGUOUS, CODING_NO_SYNC, CODING_NO_FRAMES, CODING_TOO_LONG = range(7)
CODING_REASONS = ("ok", "fewer than three kinds of symbols", "the two data kinds differ in their pulse",
                  "the two gaps lie too close together", "no third kind that occurs at least twice",
                  "no frame length that half the frames have", "more bits than a message holds")
DEFAULT_THRESHOLD = 0.1                 # ookiedokie_cfg.c:27
DEFAULT_RATE = 3000000                  # ookiedokie_cfg.c:32
DEFAULT_SAMPLES_PER_BUF = 8192          # ookiedokie_cfg.c:34


class OokdError(RuntimeError):
    def __init__(self, code: int, text: str):
        super().__init__("ookiedokie_amd error %d: %s" % (code, text))
        self.code = code


# --------------------------------------------------------------------------
# C structures
# --------------------------------------------------------------------------

class FsmTables(C.Structure):
    _fields_ = [
        ("num_states", C.c_uint32), ("max_bits", C.c_uint32),
        ("sample_rate", C.c_uint32), ("num_triggers", C.c_uint32),
        ("state_duration_us", C.POINTER(C.c_uint64)),
        ("state_timeout_us", C.POINTER(C.c_uint64)),
        ("trig_begin", C.POINTER(C.c_uint32)),
        ("trig_cond", C.POINTER(C.c_uint8)),
        ("trig_action", C.POINTER(C.c_uint8)),
        ("trig_next", C.POINTER(C.c_uint32)),
        ("trig_duration_us", C.POINTER(C.c_uint64)),
        ("state_kmin", C.POINTER(C.c_uint64)), ("state_kmax", C.POINTER(C.c_uint64)),
        ("state_kto", C.POINTER(C.c_uint64)),
        ("trig_kmin", C.POINTER(C.c_uint64)), ("trig_kmax", C.POINTER(C.c_uint64)),
    ]


class RxConfig(C.Structure):
    _fields_ = [
        ("hip_device", C.c_int32), ("flags", C.c_uint32), ("threshold", C.c_float),
        ("samples_per_buffer", C.c_uint32), ("max_samples", C.c_uint64),
        ("max_captures", C.c_uint32), ("edge_capacity", C.c_uint64),
        ("segment_buffers", C.c_uint32), ("message_slots", C.c_uint32),
        ("message_capacity", C.c_uint64), ("stream", C.c_void_p),
        ("pipeline_chunk_samples", C.c_uint64), ("front_gate", C.c_void_p),
    ]


class Message(C.Structure):
    _fields_ = [("capture", C.c_uint32), ("reserved", C.c_uint32),
                ("sample", C.c_uint64), ("payload", C.c_uint8 * MAX_PAYLOAD_BYTES)]


class FsmState(C.Structure):
    _fields_ = [("state", C.c_uint32), ("num_bits", C.c_uint32), ("k", C.c_uint64),
                ("prev_bit", C.c_uint32), ("reserved", C.c_uint32),
                ("payload", C.c_uint8 * (MAX_PAYLOAD_BYTES + 8))]

    def key(self) -> bytes:
        return bytes(self)


class RxStats(C.Structure):
    _fields_ = [
        ("input_samples", C.c_uint64), ("decimated_samples", C.c_uint64),
        ("num_edges", C.c_uint64), ("num_messages", C.c_uint64),
        ("num_errors", C.c_uint64), ("guard_recomputes", C.c_uint64),
        ("fsm_iterations", C.c_uint32), ("num_segments", C.c_uint32),
        ("fsm_path", C.c_uint32), ("fsm_fallback_reason", C.c_uint32),
        ("fir_kernel_ms", C.c_float), ("total_device_ms", C.c_float),
        ("quiet_waves", C.c_uint64), ("total_waves", C.c_uint64),
        ("pipeline_chunks", C.c_uint32), ("front_launches", C.c_uint32),
        ("scan_entry_form", C.c_uint32), ("front_form", C.c_uint32),
    ]


class FrontInfo(C.Structure):
    _fields_ = [
        ("form", C.c_uint32), ("mfma_ksteps", C.c_uint32),
        ("p_star", C.c_float), ("p_lo", C.c_float), ("p_hi", C.c_float), ("mfma_c", C.c_float),
        ("err_nominal", C.c_double), ("err_wide", C.c_double), ("err_valu", C.c_double),
        ("mfma_delta", C.c_double),
    ]


class Tune(C.Structure):
    _fields_ = [("nu", C.c_double), ("reserved", C.c_uint64 * 3)]


class RxCarrier(C.Structure):
    _fields_ = [("nu", C.c_double), ("threshold", C.c_float), ("reserved", C.c_uint32 * 5)]


class SynthConfig(C.Structure):
    _fields_ = [
        ("seed", C.c_uint64), ("sample_rate", C.c_uint32), ("amplitude", C.c_uint32),
        ("noise", C.c_uint32), ("gap_min_us", C.c_uint32), ("gap_max_us", C.c_uint32),
        ("glitch_every", C.c_uint32), ("random_phase", C.c_uint32),
    ]


class LevelHist(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("bins", C.c_uint64 * LEVEL_BINS)]


class ThresholdSuggestion(C.Structure):
    _fields_ = [("found", C.c_int), ("threshold", C.c_float), ("off_level", C.c_float), ("on_level", C.c_float),
                ("split_bin", C.c_uint32), ("off_bin", C.c_uint32), ("on_bin", C.c_uint32),
                ("on_fraction", C.c_double)]


class SpectrumResult(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("power", C.c_double * SPECTRUM_BINS)]


class CarrierStruct(C.Structure):
    _fields_ = [("nu", C.c_double), ("bin", C.c_int32), ("at_dc", C.c_uint32), ("power", C.c_double),
                ("ratio", C.c_double)]


class RunLevels(C.Structure):
    _fields_ = [("num_runs", C.c_uint64), ("tiles_total", C.c_uint64), ("tiles_filtered", C.c_uint64),
                ("tile_outputs", C.c_uint32), ("reserved", C.c_uint32), ("hist", LevelHist)]


class RunMoments(C.Structure):
    _fields_ = [("num_runs", C.c_uint64), ("tiles_total", C.c_uint64), ("tiles_filtered", C.c_uint64),
                ("tile_outputs", C.c_uint32), ("decimation", C.c_uint32)]


class MessageCarrier(C.Structure):
    _fields_ = [("carrier", C.c_double), ("mean_power", C.c_double), ("coherence", C.c_double),
                ("outputs", C.c_uint64)]


class Burst(C.Structure):
    _fields_ = [("first_sample", C.c_uint64), ("num_samples", C.c_uint64), ("offset", C.c_uint64),
                ("first_run", C.c_uint64), ("num_runs", C.c_uint64)]


class BurstInfo(C.Structure):
    _fields_ = [("num_bursts", C.c_uint64), ("total_samples", C.c_uint64), ("num_runs", C.c_uint64),
                ("pre", C.c_uint64), ("post", C.c_uint64), ("max_gap", C.c_uint64), ("flags", C.c_uint32),
                ("sample_bytes", C.c_uint32), ("tile_edges", C.c_uint32), ("decimation", C.c_uint32)]


class BurstSpectrum(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("total_power", C.c_double), ("dc_power", C.c_double),
                ("peak_power", C.c_double), ("peak_bin", C.c_uint32), ("reserved", C.c_uint32)]


class BurstSpectraInfo(C.Structure):
    _fields_ = [("num_bursts", C.c_uint64), ("total_frames", C.c_uint64), ("spans", C.c_uint64),
                ("partial_rows", C.c_uint64), ("span_frames", C.c_uint32), ("flags", C.c_uint32),
                ("reduce_kernel_ms", C.c_float), ("reserved", C.c_uint32)]


class BurstCarrierStruct(C.Structure):
    _fields_ = [("nu", C.c_double), ("bin", C.c_int32), ("reserved", C.c_uint32), ("bursts", C.c_uint64),
                ("frames", C.c_uint64), ("power", C.c_double)]


class BasebandBurst(C.Structure):
    _fields_ = [("first_output", C.c_uint64), ("num_outputs", C.c_uint64), ("offset", C.c_uint64)]


class BasebandInfo(C.Structure):
    _fields_ = [("num_bursts", C.c_uint64), ("total_outputs", C.c_uint64), ("tiles_total", C.c_uint64),
                ("tiles_filtered", C.c_uint64), ("tile_outputs", C.c_uint32), ("decimation", C.c_uint32),
                ("nu", C.c_double), ("turn", C.c_double)]


BASEBAND_CF32 = 0                       # OOKD_BASEBAND_CF32
BASEBAND_SC16Q11 = 1                    # OOKD_BASEBAND_SC16Q11
BASEBAND_FORMATS = {"cf32": BASEBAND_CF32, "sc16q11": BASEBAND_SC16Q11}
BASEBAND_FIELDS = tuple(name for name, _ in BasebandBurst._fields_)
BURSTS_CLEAN = 1                        # OOKD_BURSTS_CLEAN
BURST_MIN_SHARE = 0.125                 # OOKD_BURST_MIN_SHARE
BURST_SPECTRA_MIN_SPAN = 32             # OOKD_BURST_SPECTRA_MIN_SPAN
BURST_SPECTRA_MAX_ROWS = 8192           # OOKD_BURST_SPECTRA_MAX_ROWS
BURST_SPECTRUM_DTYPE = np.dtype([("frames", "<u8"), ("total_power", "<f8"), ("dc_power", "<f8"), ("peak_power", "<f8"),
                                 ("peak_bin", "<u4"), ("reserved", "<u4")])
BURST_FIELDS = tuple(name for name, _ in Burst._fields_)


class PulseHist(C.Structure):
    _fields_ = [("num_edges", C.c_uint64), ("samples", C.c_uint64), ("runs", C.c_uint64 * 2),
                ("count", (C.c_uint64 * PULSE_BINS) * 2), ("sum", (C.c_uint64 * PULSE_BINS) * 2),
                ("open_head", C.c_uint64), ("open_tail", C.c_uint64), ("tail_level", C.c_uint32),
                ("reserved", C.c_uint32)]


class PulseClass(C.Structure):
    _fields_ = [("first_bin", C.c_uint32), ("last_bin", C.c_uint32), ("runs", C.c_uint64), ("mean", C.c_double),
                ("lower", C.c_uint64), ("upper", C.c_uint64), ("mean_us", C.c_double), ("lower_us", C.c_double),
                ("upper_us", C.c_double)]


class PulseSuggestion(C.Structure):
    _fields_ = [("found", C.c_int), ("reserved", C.c_uint32), ("num_classes", C.c_uint32 * 2),
                ("dropped_runs", C.c_uint64 * 2), ("classes", (PulseClass * PULSE_MAX_CLASSES) * 2)]


class CleanInfo(C.Structure):
    _fields_ = [("edges_in", C.c_uint64), ("edges_out", C.c_uint64), ("deleted", C.c_uint64 * 2),
                ("min_on", C.c_uint64), ("min_off", C.c_uint64)]


class SymbolTable(C.Structure):
    _fields_ = [("num_classes", C.c_uint32 * 2), ("lower", (C.c_uint64 * SYMBOL_MAX_CLASSES) * 2),
                ("upper", (C.c_uint64 * SYMBOL_MAX_CLASSES) * 2)]


class SymbolRoles(C.Structure):
    _fields_ = [("role", (C.c_uint8 * SYMBOL_KINDS) * SYMBOL_KINDS), ("reserved", C.c_uint8 * 7)]


class SymbolSurvey(C.Structure):
    _fields_ = [("num_symbols", C.c_uint64), ("kinds", (C.c_uint64 * SYMBOL_KINDS) * SYMBOL_KINDS),
                ("num_syncs", C.c_uint64), ("head_symbols", C.c_uint64), ("tail_symbols", C.c_uint64),
                ("frames", (C.c_uint64 * FRAME_BINS) * 2)]


class Coding(C.Structure):
    _fields_ = [("found", C.c_int), ("reason", C.c_uint32), ("data_on_class", C.c_uint32),
                ("zero_off_class", C.c_uint32), ("one_off_class", C.c_uint32), ("sync_on_class", C.c_uint32),
                ("sync_off_class", C.c_uint32), ("reserved", C.c_uint32), ("zero_count", C.c_uint64),
                ("one_count", C.c_uint64), ("sync_count", C.c_uint64), ("t0_us", C.c_double), ("t1_us", C.c_double)]


class DeviceSuggestion(C.Structure):
    _fields_ = [("found", C.c_int), ("reason", C.c_uint32), ("num_bits", C.c_uint32), ("frame_symbols", C.c_uint32),
                ("sync_on_us", C.c_uint64), ("sync_off_us", C.c_uint64), ("bit_on_us", C.c_uint64),
                ("zero_off_us", C.c_uint64), ("one_off_us", C.c_uint64), ("frames_seen", C.c_uint64),
                ("frames_counted", C.c_uint64), ("frames_clean", C.c_uint64), ("num_syncs", C.c_uint64)]


class HostCfg(C.Structure):
    """struct ookiedokie_cfg (ookiedokie_cfg.h:50-91), field for field."""
    _fields_ = [
        ("sdr_type", C.c_char_p), ("direction", C.c_int), ("sdr_args", C.c_char_p),
        ("frequency", C.c_uint), ("bandwidth", C.c_uint), ("samplerate", C.c_uint),
        ("gain", C.c_int), ("device", C.c_char_p), ("tx_count", C.c_uint),
        ("tx_delay_us", C.c_uint), ("device_params", C.c_void_p), ("rx_fmt", C.c_int),
        ("rx_threshold", C.c_float), ("rx_rec_filename", C.c_char_p),
        ("rx_rec_type", C.c_char_p), ("rx_filter", C.c_char_p),
        ("rx_rec_dig", C.c_char_p), ("rx_rec_input", C.c_ubyte),
        ("samples_per_buffer", C.c_uint), ("num_buffers", C.c_uint),
        ("num_transfers", C.c_uint), ("stream_timeout_ms", C.c_uint),
        ("sync_timeout_ms", C.c_uint), ("verbosity", C.c_int),
    ]


# --------------------------------------------------------------------------
# library
# --------------------------------------------------------------------------

_lib: Optional[C.CDLL] = None

_PROTOTYPES = {
    "ookd_last_error": (C.c_char_p, []),
    "ookd_api_version": (C.c_int, []),
    "ookd_filter_load": (C.c_void_p, [C.c_char_p]),
    "ookd_filter_create": (C.c_void_p, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ookd_filter_free": (None, [C.c_void_p]),
    "ookd_filter_total_decimation": (C.c_uint32, [C.c_void_p]),
    "ookd_filter_num_stages": (C.c_uint32, [C.c_void_p]),
    "ookd_filter_stage": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_float))]),
    "ookd_filter_tuned_taps": (C.c_int, [C.c_void_p, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p]),
    "ookd_device_load": (C.c_void_p, [C.c_char_p, C.c_uint32]),
    "ookd_device_create": (C.c_void_p, [C.POINTER(FsmTables)]),
    "ookd_device_free": (None, [C.c_void_p]),
    "ookd_device_num_bits": (C.c_uint32, [C.c_void_p]),
    "ookd_device_name": (C.c_char_p, [C.c_void_p]),
    "ookd_device_state_name": (C.c_char_p, [C.c_void_p, C.c_uint32]),
    "ookd_device_tables": (C.c_int, [C.c_void_p, C.POINTER(FsmTables)]),
    "ookd_rx_create": (C.c_void_p, [C.POINTER(RxConfig), C.c_void_p, C.c_void_p]),
    "ookd_rx_create_tuned": (C.c_void_p, [C.POINTER(RxConfig), C.c_void_p, C.c_void_p, C.POINTER(Tune)]),
    "ookd_rx_tune": (C.c_double, [C.c_void_p]),
    "ookd_rx_create_carriers": (C.c_void_p, [C.POINTER(RxConfig), C.c_void_p, C.c_void_p, C.POINTER(RxCarrier),
                                             C.c_uint32]),
    "ookd_rx_num_carriers": (C.c_uint32, [C.c_void_p]),
    "ookd_rx_get_carrier": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(RxCarrier)]),
    "ookd_rx_get_carrier_front_info": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(FrontInfo)]),
    "ookd_rx_destroy": (None, [C.c_void_p]),
    "ookd_rx_sample_bytes": (C.c_uint32, [C.c_void_p]),
    "ookd_rx_process_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]),
    "ookd_rx_submit_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]),
    "ookd_scan_domain_info": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ookd_rx_wait": (C.c_int, [C.c_void_p]),
    "ookd_rx_process_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "ookd_rx_shard_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                      C.c_int, C.POINTER(FsmState), C.POINTER(FsmState)]),
    "ookd_rx_shard_refine": (C.c_int, [C.c_void_p, C.POINTER(FsmState), C.POINTER(FsmState)]),
    "ookd_rx_halo_samples": (C.c_uint64, [C.c_void_p]),
    "ookd_rx_num_messages": (C.c_uint64, [C.c_void_p]),
    "ookd_rx_messages": (C.POINTER(Message), [C.c_void_p]),
    "ookd_rx_get_stats": (C.c_int, [C.c_void_p, C.POINTER(RxStats)]),
    "ookd_rx_get_front_info": (C.c_int, [C.c_void_p, C.POINTER(FrontInfo)]),
    "ookd_rx_bit_words": (C.c_uint64, [C.c_void_p]),
    "ookd_rx_get_bits": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "ookd_rx_get_edges": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                    C.POINTER(C.c_uint64)]),
    "ookd_rx_get_fir": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "ookd_rx_get_errors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ookd_fir_create": (C.c_void_p, [C.c_int32, C.c_void_p, C.c_size_t, C.c_uint32]),
    "ookd_fir_reset": (None, [C.c_void_p]),
    "ookd_fir_destroy": (None, [C.c_void_p]),
    "ookd_fir_filter_and_decimate": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ookd_synth_create": (C.c_void_p, [C.c_void_p, C.POINTER(SynthConfig), C.c_uint64]),
    "ookd_synth_free": (None, [C.c_void_p]),
    "ookd_synth_num_messages": (C.c_uint64, [C.c_void_p]),
    "ookd_synth_message": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]),
    "ookd_synth_fill_host": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "ookd_synth_fill_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64,
                                         C.c_void_p, C.c_void_p]),
    "ookd_rx_dig_text": (C.c_size_t, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]),
    "ookd_rx_record_dig": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p]),
    "ookd_rx_get_fir_sc16q11": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "ookd_rx_record_fir": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p]),
    "ookd_formatter_create": (C.c_void_p, [C.c_void_p]),
    "ookd_formatter_free": (None, [C.c_void_p]),
    "ookd_formatter_num_fields": (C.c_uint32, [C.c_void_p]),
    "ookd_formatter_field_name": (C.c_char_p, [C.c_void_p, C.c_uint32]),
    "ookd_formatter_ts_mode": (C.c_int, [C.c_void_p]),
    "ookd_formatter_field_to_str": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_char_p, C.c_size_t]),
    "ookd_formatter_default_data": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ookd_formatter_set_field": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "ookd_print_record": (C.c_size_t, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_size_t,
                                       C.c_char_p, C.c_size_t]),
    "ookd_print_messages": (C.c_size_t, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_uint64,
                                         C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]),
    "ookd_rx_gate_create": (C.c_void_p, []),
    "ookd_rx_gate_destroy": (None, [C.c_void_p]),
    "ookd_survey_create": (C.c_void_p, [C.c_int32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "ookd_survey_create_tuned": (C.c_void_p, [C.c_int32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                              C.POINTER(Tune)]),
    "ookd_survey_create_carriers": (C.c_void_p, [C.c_int32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                 C.POINTER(Tune), C.c_uint32, C.c_uint32]),
    "ookd_survey_num_carriers": (C.c_uint32, [C.c_void_p]),
    "ookd_survey_stride": (C.c_uint32, [C.c_void_p]),
    "ookd_survey_get_carrier_hist": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(LevelHist)]),
    "ookd_survey_tune": (C.c_double, [C.c_void_p]),
    "ookd_survey_form": (C.c_uint32, [C.c_void_p]),
    "ookd_survey_destroy": (None, [C.c_void_p]),
    "ookd_survey_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]),
    "ookd_survey_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "ookd_survey_get_hist": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(LevelHist)]),
    "ookd_survey_kernel_ms": (C.c_float, [C.c_void_p]),
    "ookd_level_bin": (C.c_uint32, [C.c_float]),
    "ookd_level_bin_lower": (C.c_float, [C.c_uint32]),
    "ookd_suggest_threshold": (C.c_int, [C.POINTER(LevelHist), C.POINTER(ThresholdSuggestion)]),
    "ookd_spectrum_create": (C.c_void_p, [C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "ookd_spectrum_destroy": (None, [C.c_void_p]),
    "ookd_spectrum_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]),
    "ookd_spectrum_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "ookd_spectrum_get": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(SpectrumResult)]),
    "ookd_spectrum_kernel_ms": (C.c_float, [C.c_void_p]),
    "ookd_spectrum_bin_nu": (C.c_double, [C.c_uint32]),
    "ookd_suggest_carriers": (C.c_int, [C.POINTER(SpectrumResult), C.c_double, C.c_uint32,
                                        C.POINTER(CarrierStruct), C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_double)]),
    "ookd_rx_pulse_hist": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(PulseHist)]),
    "ookd_rx_pulse_kernel_ms": (C.c_float, [C.c_void_p]),
    "ookd_pulse_bin": (C.c_uint32, [C.c_uint64]),
    "ookd_pulse_bin_lower": (C.c_uint64, [C.c_uint32]),
    "ookd_suggest_pulses": (C.c_int, [C.POINTER(PulseHist), C.c_double, C.POINTER(PulseSuggestion)]),
    "ookd_symbol_table_from_pulses": (C.c_int, [C.POINTER(PulseSuggestion), C.POINTER(SymbolTable)]),
    "ookd_rx_symbol_survey": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(SymbolTable), C.POINTER(SymbolRoles),
                                        C.POINTER(SymbolSurvey)]),
    "ookd_rx_symbol_kernel_ms": (C.c_float, [C.c_void_p]),
    "ookd_suggest_coding": (C.c_int, [C.POINTER(PulseSuggestion), C.POINTER(SymbolSurvey), C.POINTER(SymbolRoles),
                                      C.POINTER(Coding)]),
    "ookd_suggest_device": (C.c_int, [C.POINTER(PulseSuggestion), C.POINTER(SymbolSurvey), C.POINTER(Coding), C.c_double,
                                      C.POINTER(DeviceSuggestion)]),
    "ookd_clean_edges": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                   C.POINTER(C.c_uint64)]),
    "ookd_rx_clean_edges": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "ookd_rx_get_clean_info": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(CleanInfo)]),
    "ookd_rx_get_clean_edges": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ookd_rx_pulse_hist_clean": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(PulseHist)]),
    "ookd_rx_symbol_survey_clean": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(SymbolTable), C.POINTER(SymbolRoles),
                                              C.POINTER(SymbolSurvey)]),
    "ookd_rx_clean_kernel_ms": (C.c_float, [C.c_void_p]),
    "ookd_rx_set_debounce": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "ookd_rx_get_debounce": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ookd_rx_run_levels": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(RunLevels)]),
    "ookd_rx_run_levels_clean": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(RunLevels)]),
    "ookd_rx_get_run_peaks": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ookd_rx_get_run_peaks_clean": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ookd_rx_levels_kernel_ms": (C.c_float, [C.c_void_p]),
    "ookd_message_levels": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                      C.c_void_p]),
    "ookd_rx_run_moments": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(RunMoments)]),
    "ookd_rx_run_moments_clean": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(RunMoments)]),
    "ookd_rx_get_run_moments": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ookd_rx_get_run_moments_clean": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ookd_rx_moments_kernel_ms": (C.c_float, [C.c_void_p]),
    "ookd_run_moments_of": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "ookd_message_carriers": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                        C.c_uint32, C.c_uint32, C.c_double, C.c_void_p]),
    "ookd_find_bursts": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                   C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ookd_rx_bursts": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]),
    "ookd_rx_get_burst_info": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(BurstInfo)]),
    "ookd_rx_get_bursts": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ookd_rx_copy_bursts_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "ookd_rx_copy_bursts_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "ookd_rx_bursts_kernel_ms": (C.c_float, [C.c_void_p]),
    "ookd_rx_burst_copy_kernel_ms": (C.c_float, [C.c_void_p]),
    "ookd_baseband_bursts": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ookd_baseband_of": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64]),
    "ookd_rx_get_baseband_info": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(BasebandInfo)]),
    "ookd_rx_get_baseband_bursts": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ookd_rx_burst_baseband_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]),
    "ookd_rx_burst_baseband_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]),
    "ookd_rx_baseband_kernel_ms": (C.c_float, [C.c_void_p]),
    "ookd_rx_burst_spectra": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "ookd_rx_get_burst_spectra": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ookd_rx_get_keyed_spectrum": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(SpectrumResult)]),
    "ookd_rx_get_burst_spectra_info": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(BurstSpectraInfo)]),
    "ookd_rx_burst_spectrum": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(SpectrumResult)]),
    "ookd_rx_burst_spectra_kernel_ms": (C.c_float, [C.c_void_p]),
    "ookd_burst_spectra_span": (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ookd_suggest_burst_carriers": (C.c_int, [C.c_void_p, C.c_uint64, C.c_double, C.c_uint32, C.c_void_p, C.c_uint32,
                                              C.POINTER(C.c_uint32), C.c_void_p]),
    "ookd_device_from_suggestion": (C.c_void_p, [C.POINTER(DeviceSuggestion), C.c_uint32]),
    "ookd_device_suggestion_json": (C.c_size_t, [C.POINTER(DeviceSuggestion), C.c_char_p, C.c_char_p, C.c_size_t]),
    "sdr_hip_file_init": (C.c_void_p, [C.c_void_p]),
    "sdr_hip_file_deinit": (None, [C.c_void_p]),
    "sdr_hip_file_rx": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint]),
    "sdr_hip_file_tx": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint]),
    "sdr_hip_file_flush": (C.c_int, [C.c_void_p]),
    "sdr_hip_file_capture": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "sdr_hip_file_sample_flags": (C.c_int, [C.c_void_p]),
}


def lib() -> C.CDLL:
    """Loads libookiedokie_amd.so.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OokdError(-4, "%s is missing: run `python -m ookiedokie_amd.build` "
                                "(there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return (lib().ookd_last_error() or b"").decode("utf-8", "replace")


def _check(rc: int) -> None:
    if rc != 0:
        raise OokdError(rc, last_error())


# --------------------------------------------------------------------------
# filter / device
# --------------------------------------------------------------------------

class Filter:
    """Multi-stage decimating FIR description (struct fir_filter, fir.c:60-66)."""

    def __init__(self, handle: int):
        if not handle:
            raise OokdError(-3, last_error())
        self._h = handle

    @classmethod
    def load(cls, path: str) -> "Filter":
        return cls(lib().ookd_filter_load(os.fsencode(path)))

    @classmethod
    def from_stages(cls, stages: Sequence[Tuple[int, Sequence[float]]]) -> "Filter":
        dec = np.array([d for d, _ in stages], dtype=np.uint32)
        nt = np.array([len(t) for _, t in stages], dtype=np.uint32)
        taps = np.concatenate([np.asarray(t, dtype=np.float32) for _, t in stages]) \
            if stages else np.zeros(0, np.float32)
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        return cls(lib().ookd_filter_create(len(stages), dec.ctypes.data, nt.ctypes.data,
                                            taps.ctypes.data))

    @property
    def total_decimation(self) -> int:
        return int(lib().ookd_filter_total_decimation(self._h))

    @property
    def num_stages(self) -> int:
        return int(lib().ookd_filter_num_stages(self._h))

    def stage(self, s: int) -> Tuple[int, np.ndarray]:
        d, n = C.c_uint32(0), C.c_uint32(0)
        p = C.POINTER(C.c_float)()
        _check(lib().ookd_filter_stage(self._h, s, C.byref(d), C.byref(n), C.byref(p)))
        return int(d.value), np.ctypeslib.as_array(p, shape=(n.value,)).copy()

    def tuned_taps(self, nu: float, stage: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """The complex taps (re, im: float32) a context tuned to `nu` cycles per input sample runs stage `stage`
        with (ookd_filter_tuned_taps; pure host code)."""
        if not 0 <= stage < self.num_stages:
            raise OokdError(-1, "filter has no stage %d" % stage)
        n = self.stage(stage)[1].size
        re, im = np.zeros(n, np.float32), np.zeros(n, np.float32)
        _check(lib().ookd_filter_tuned_taps(self._h, float(nu), stage, re.ctypes.data, im.ctypes.data))
        return re, im

    def close(self) -> None:
        if self._h:
            lib().ookd_filter_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fir_init(path: str) -> Filter:
    return Filter.load(path)


class Device:
    """OOK device description: state machine tables + field layout (device.c:60-74)."""

    def __init__(self, handle: int):
        if not handle:
            raise OokdError(-3, last_error())
        self._h = handle

    @classmethod
    def load(cls, path: str, sample_rate: int) -> "Device":
        return cls(lib().ookd_device_load(os.fsencode(path), int(sample_rate)))

    @classmethod
    def from_tables(cls, *, max_bits: int, sample_rate: int, state_duration_us, state_timeout_us,
                    trig_begin, trig_cond, trig_action, trig_next, trig_duration_us) -> "Device":
        keep = [np.ascontiguousarray(state_duration_us, dtype=np.uint64),
                np.ascontiguousarray(state_timeout_us, dtype=np.uint64),
                np.ascontiguousarray(trig_begin, dtype=np.uint32),
                np.ascontiguousarray(trig_cond, dtype=np.uint8),
                np.ascontiguousarray(trig_action, dtype=np.uint8),
                np.ascontiguousarray(trig_next, dtype=np.uint32),
                np.ascontiguousarray(trig_duration_us, dtype=np.uint64)]
        t = FsmTables()
        t.num_states = len(keep[0])
        t.max_bits = max_bits
        t.sample_rate = sample_rate
        t.num_triggers = len(keep[3])
        t.state_duration_us = keep[0].ctypes.data_as(C.POINTER(C.c_uint64))
        t.state_timeout_us = keep[1].ctypes.data_as(C.POINTER(C.c_uint64))
        t.trig_begin = keep[2].ctypes.data_as(C.POINTER(C.c_uint32))
        t.trig_cond = keep[3].ctypes.data_as(C.POINTER(C.c_uint8))
        t.trig_action = keep[4].ctypes.data_as(C.POINTER(C.c_uint8))
        t.trig_next = keep[5].ctypes.data_as(C.POINTER(C.c_uint32))
        t.trig_duration_us = keep[6].ctypes.data_as(C.POINTER(C.c_uint64))
        return cls(lib().ookd_device_create(C.byref(t)))

    @classmethod
    def from_suggestion(cls, suggestion, sample_rate: int) -> "Device":
        """The device `suggest_device` (or `Receiver.suggest_device`) found, for the decoder: its six states through
        ookd_device_create.  sample_rate is that of the decimated samples, as for `load`."""
        return cls(lib().ookd_device_from_suggestion(C.byref(_device_suggestion_struct(suggestion)), int(sample_rate)))

    @property
    def num_bits(self) -> int:
        return int(lib().ookd_device_num_bits(self._h))

    @property
    def payload_bytes(self) -> int:
        return (self.num_bits + 7) // 8

    @property
    def name(self) -> str:
        return lib().ookd_device_name(self._h).decode()

    def tables(self) -> dict:
        t = FsmTables()
        _check(lib().ookd_device_tables(self._h, C.byref(t)))
        ns, nt = t.num_states, t.num_triggers

        def arr(p, n):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0)

        out = {"num_states": ns, "max_bits": t.max_bits, "sample_rate": t.sample_rate,
               "num_triggers": nt,
               "state_names": [lib().ookd_device_state_name(self._h, s).decode() for s in range(ns)]}
        for name in ("state_duration_us", "state_timeout_us", "state_kmin", "state_kmax", "state_kto"):
            out[name] = arr(getattr(t, name), ns)
        out["trig_begin"] = arr(t.trig_begin, ns + 1)
        for name in ("trig_cond", "trig_action", "trig_next", "trig_duration_us", "trig_kmin", "trig_kmax"):
            out[name] = arr(getattr(t, name), nt)
        return out

    def close(self) -> None:
        if self._h:
            lib().ookd_device_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_init(path: str, sample_rate: int) -> Device:
    return Device.load(path, sample_rate)


# --------------------------------------------------------------------------
# formatter / printer (host side of a decoded message)
# --------------------------------------------------------------------------

RX_FMT_PRETTY = 0       # enum ookiedokie_rx_fmt, ookiedokie_cfg.h:41-45
RX_FMT_CSV = 1


class Formatter:
    """struct formatter (src/formatter.h) built from a device's "fields":
    payload bits -> per-field text -> the text rx_print writes."""

    def __init__(self, device: Device):
        h = lib().ookd_formatter_create(device._h)
        if not h:
            raise OokdError(-1, last_error())
        self._h = h
        self._payload_bytes = max(device.payload_bytes, 1)
        self.first_print = True         # CSV heading still to be printed

    @property
    def field_names(self) -> List[str]:
        n = lib().ookd_formatter_num_fields(self._h)
        return [lib().ookd_formatter_field_name(self._h, i).decode() for i in range(n)]

    @property
    def ts_mode(self) -> int:
        return int(lib().ookd_formatter_ts_mode(self._h))

    def _payload(self, payload) -> np.ndarray:
        a = np.zeros(MAX_PAYLOAD_BYTES, dtype=np.uint8)
        p = np.frombuffer(bytes(payload), dtype=np.uint8) if not isinstance(payload, np.ndarray) else payload
        a[:min(p.size, a.size)] = p[:a.size]
        return a

    def data_to_keyval(self, payload) -> List[Tuple[str, str]]:
        """formatter_data_to_keyval (formatter.c:715-739), without the timestamp pair."""
        a = self._payload(payload)
        out = []
        buf = C.create_string_buffer(96)
        for i, name in enumerate(self.field_names):
            _check(lib().ookd_formatter_field_to_str(self._h, i, a.ctypes.data, buf, len(buf)))
            out.append((name, buf.value.decode("utf-8", "replace")))
        return out

    def default_data(self) -> np.ndarray:
        """formatter_default_data (formatter.c:835-846)."""
        a = np.zeros(MAX_PAYLOAD_BYTES, dtype=np.uint8)
        _check(lib().ookd_formatter_default_data(self._h, a.ctypes.data, a.size))
        return a[:self._payload_bytes].copy()

    def keyval_to_data(self, params: Sequence[Tuple[str, str]], data: Optional[np.ndarray] = None) -> np.ndarray:
        """formatter_keyval_to_data (formatter.c:793-832) on top of `data`
        (default: the defaults, as device_generate does, device.c:660-676)."""
        a = np.zeros(MAX_PAYLOAD_BYTES, dtype=np.uint8)
        base = self.default_data() if data is None else np.asarray(data, dtype=np.uint8)
        a[:base.size] = base
        for k, v in params:
            _check(lib().ookd_formatter_set_field(self._h, k.encode(), v.encode(), a.ctypes.data, a.size))
        return a[:self._payload_bytes].copy()

    def print_record(self, payloads: Sequence, fmt: int = RX_FMT_PRETTY) -> str:
        """rx_print for the messages of ONE buffer."""
        arrs = [self._payload(p) for p in payloads]
        ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        fp = C.c_int(1 if self.first_print else 0)
        need = lib().ookd_print_record(self._h, fmt, C.byref(fp), ptrs, len(arrs), None, 0)
        fp = C.c_int(1 if self.first_print else 0)
        buf = C.create_string_buffer(need + 1)
        lib().ookd_print_record(self._h, fmt, C.byref(fp), ptrs, len(arrs), buf, len(buf))
        self.first_print = bool(fp.value)
        return buf.value.decode("utf-8", "replace")

    def print_messages(self, result: "RxResult", samples_per_buffer: int, total_decimation: int = 1,
                       fmt: int = RX_FMT_PRETTY) -> str:
        """Everything the reference's rx loop prints for a run's messages."""
        n = len(result.msg_samples)
        msgs = (Message * max(n, 1))()
        for i in range(n):
            msgs[i].capture = int(result.captures[i])
            msgs[i].sample = int(result.msg_samples[i])
            p = self._payload(result.payloads[i])
            C.memmove(msgs[i].payload, p.ctypes.data, MAX_PAYLOAD_BYTES)
        fp = C.c_int(1 if self.first_print else 0)
        need = lib().ookd_print_messages(self._h, fmt, C.byref(fp), msgs, n, samples_per_buffer,
                                         total_decimation, None, 0)
        fp = C.c_int(1 if self.first_print else 0)
        buf = C.create_string_buffer(need + 1)
        lib().ookd_print_messages(self._h, fmt, C.byref(fp), msgs, n, samples_per_buffer, total_decimation,
                                  buf, len(buf))
        self.first_print = bool(fp.value)
        return buf.value.decode("utf-8", "replace")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().ookd_formatter_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------
# rx
# --------------------------------------------------------------------------

@dataclass
class RxResult:
    captures: np.ndarray        # uint32 [n]
    msg_samples: np.ndarray     # uint64 [n] decimated index of OUTPUT_READY
    payloads: np.ndarray        # uint8 [n, payload_bytes]
    stats: dict

    def payload_bits(self, i: int, nbits: int) -> str:
        b = np.unpackbits(self.payloads[i], bitorder="little")[:nbits]
        return "".join(str(int(x)) for x in b)

    def for_capture(self, c: int) -> "RxResult":
        m = self.captures == c
        return RxResult(self.captures[m], self.msg_samples[m], self.payloads[m], self.stats)


class FrontGate:
    """Contexts created with the same gate take turns for their (HBM-bound) front-end kernels
    (ookd_rx_gate_create); pass it to every Receiver that should."""

    def __init__(self):
        self._h = lib().ookd_rx_gate_create()
        if not self._h:
            raise OokdError(-3, "ookd_rx_gate_create failed")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().ookd_rx_gate_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Receiver:
    """Fused replacement of the reference rx loop body for whole captures in HBM."""

    def __init__(self, filt: Optional[Filter], device: Optional[Device], *,
                 max_samples: int, threshold: float = DEFAULT_THRESHOLD,
                 samples_per_buffer: int = DEFAULT_SAMPLES_PER_BUF, hip_device: int = 0,
                 max_captures: int = 1, exact_fir: bool = False, keep_fir: bool = False,
                 edge_capacity: int = 0, segment_buffers: int = 0, message_slots: int = 0,
                 message_capacity: int = 0, stream: int = 0, fsm_rounds: bool = False,
                 quiet_skip: bool = True, count_quiet: bool = False, scan_sims: bool = False,
                 pipeline: bool = True, pipeline_chunk_samples: int = 0,
                 front_gate: Optional["FrontGate"] = None, fir_valu: bool = False,
                 scan_tables: bool = False, sample_format: str = "sc16q11",
                 tune: Optional[float] = None, tune_hz: Optional[float] = None,
                 sample_rate: Optional[float] = None,
                 carriers: Optional[Sequence] = None, tuned_fir2: bool = False,
                 min_on: int = 0, min_off: int = 0):
        """tune: carrier offset in cycles per input sample (|tune| <= 0.5), or tune_hz with sample_rate -- one
        of the two forms.  The context then filters with the taps `Filter.tuned_taps` returns (ookd_rx_create_tuned);
        0 is an untuned context.

        carriers: several carriers of ONE capture decoded in one pass (ookd_rx_create_carriers): entries are `nu`
        (cycles per input sample, with this receiver's `threshold`) or `(nu, threshold)`.  Not together with tune /
        tune_hz.  Such a context runs one capture per run; wherever a method takes a capture index it takes the
        carrier index, and a result's `captures` field holds each message's carrier.

        tuned_fir2: a tuned or carrier context on a filter of two decimate-by-2 stages (<= 16 and <= 32 taps, the
        backend default fs128_fs16_dec4) runs the fused kernel FRONT_TUNED_FIR2 instead of FRONT_TUNED_GENERIC
        (OOKD_RX_TUNED_FIR2): same bits, floats within err_valu.  Changes nothing for any other context.

        min_on, min_off: debounce, in decimated samples (`set_debounce`); 0 and 1 leave the context as it always was."""
        if carriers is not None and (tune is not None or tune_hz is not None):
            raise ValueError("carriers and tune / tune_hz are mutually exclusive: a carrier list names every nu")
        if tune is not None and (tune_hz is not None or sample_rate is not None):
            raise ValueError("give either tune (cycles per sample) or tune_hz with sample_rate, not both")
        if (tune_hz is None) != (sample_rate is None):
            raise ValueError("tune_hz and sample_rate go together")
        if tune_hz is not None:
            if not sample_rate > 0:
                raise ValueError("sample_rate must be positive")
            tune = float(tune_hz) / float(sample_rate)
        if sample_format not in SAMPLE_FORMATS:
            raise ValueError("sample_format must be one of %s" % ", ".join(sorted(SAMPLE_FORMATS)))
        self.sample_format = sample_format
        fmt_flag, self._sample_dtype = SAMPLE_FORMATS[sample_format]
        cfg = RxConfig()
        cfg.hip_device = hip_device
        cfg.flags = ((RX_EXACT_FIR if exact_fir else 0) | (RX_KEEP_FIR if keep_fir else 0)
                     | (RX_FSM_ROUNDS if fsm_rounds else 0) | (0 if quiet_skip else RX_NO_QUIET_SKIP)
                     | (RX_COUNT_QUIET if count_quiet else 0) | (RX_SCAN_SIMS if scan_sims else 0)
                     | (0 if pipeline else RX_NO_PIPELINE)
                     | (RX_FIR_VALU if fir_valu else 0) | (RX_SCAN_TABLES if scan_tables else 0) | fmt_flag
                     | (RX_TUNED_FIR2 if tuned_fir2 else 0))
        cfg.threshold = threshold
        cfg.samples_per_buffer = samples_per_buffer
        cfg.max_samples = max_samples
        cfg.max_captures = max_captures
        cfg.edge_capacity = edge_capacity
        cfg.segment_buffers = segment_buffers
        cfg.message_slots = message_slots
        cfg.message_capacity = message_capacity
        cfg.stream = stream
        cfg.pipeline_chunk_samples = pipeline_chunk_samples
        cfg.front_gate = front_gate._h if front_gate is not None else None
        self._gate = front_gate         # keeps it alive as long as the context
        self._filter, self._device = filt, device
        self.payload_bytes = device.payload_bytes if device else 0
        self.total_decimation = filt.total_decimation if filt else 1
        if carriers is not None:
            entries = []
            for c in carriers:
                nu, thr = c if isinstance(c, (tuple, list)) else (c, threshold)
                entries.append((float(nu), float(thr)))
            arr = (RxCarrier * max(len(entries), 1))()
            for k, (nu, thr) in enumerate(entries):
                arr[k].nu, arr[k].threshold = nu, thr
            self._h = lib().ookd_rx_create_carriers(C.byref(cfg), filt._h if filt else None,
                                                    device._h if device else None, arr, len(entries))
        elif tune is None:
            self._h = lib().ookd_rx_create(C.byref(cfg), filt._h if filt else None,
                                           device._h if device else None)
        else:
            t = Tune()
            t.nu = float(tune)
            self._h = lib().ookd_rx_create_tuned(C.byref(cfg), filt._h if filt else None,
                                                 device._h if device else None, C.byref(t))
        if not self._h:
            raise OokdError(-4, last_error())
        if int(min_on) > 1 or int(min_off) > 1:
            try:
                self.set_debounce(min_on, min_off)
            except OokdError:
                self.close()
                raise

    def set_debounce(self, min_on: int = 0, min_off: int = 0) -> None:
        """From the next run on, every run cleans its edge list on the GPU in its chain (the `clean_edges` rule: "on" /
        "off" runs shorter than min_on / min_off decimated samples go, 0 and 1 keep every run of that level) and the
        state machine decodes the cleaned list (ookd_rx_set_debounce).  bits, edges(), the surveys and
        stats()["num_edges"] stay the raw stream's; edges(c, clean=True) and the other clean readers answer from the
        run's cleaned list without a `clean_edges` call.  Such a context never pipelines in chunks and refuses
        shards.  Both <= 1: off.  Refused while a run is in flight."""
        _check(lib().ookd_rx_set_debounce(self._h, int(min_on), int(min_off)))

    @property
    def debounce(self) -> Tuple[int, int]:
        """(min_on, min_off) as set; (0, 0) for a context never given any."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(lib().ookd_rx_get_debounce(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    @property
    def tune(self) -> float:
        """Carrier offset this context is tuned to, cycles per input sample (0: untuned)."""
        return float(lib().ookd_rx_tune(self._h))

    @property
    def num_carriers(self) -> int:
        """Carriers of a carrier context (Receiver(carriers=[...])), 0 for every other context."""
        return int(lib().ookd_rx_num_carriers(self._h))

    def carrier(self, k: int) -> Tuple[float, float]:
        """(nu, threshold) of carrier k."""
        c = RxCarrier()
        _check(lib().ookd_rx_get_carrier(self._h, k, C.byref(c)))
        return float(c.nu), float(c.threshold)

    def carrier_front_info(self, k: int) -> dict:
        """`front_info` with carrier k's p_star, guard band and err_valu."""
        f = FrontInfo()
        _check(lib().ookd_rx_get_carrier_front_info(self._h, k, C.byref(f)))
        return {name: getattr(f, name) for name, _ in FrontInfo._fields_}

    # -- runs ---------------------------------------------------------------
    def rx_device(self, d_iq_ptr: int, samples_per_capture: int, num_captures: int = 1,
                  stride: Optional[int] = None) -> RxResult:
        """Captures already resident in HBM (I,Q interleaved, in the context's sample format)."""
        _check(lib().ookd_rx_process_device(self._h, d_iq_ptr, num_captures, samples_per_capture,
                                            stride if stride is not None else samples_per_capture))
        return self._result()

    def process_device(self, d_iq_ptr: int, samples_per_capture: int, num_captures: int = 1,
                       stride: Optional[int] = None) -> None:
        """ookd_rx_process_device and nothing else: when it returns the messages
        are in host memory behind ookd_rx_messages(); `result()` / `raw_stats()`
        turn them into Python objects when (and if) the caller wants them."""
        _check(lib().ookd_rx_process_device(self._h, d_iq_ptr, num_captures, samples_per_capture,
                                            stride if stride is not None else samples_per_capture))

    def submit_device(self, d_iq_ptr: int, samples_per_capture: int, num_captures: int = 1,
                      stride: Optional[int] = None) -> None:
        """Queue a run on this context's stream and return (ookd_rx_submit_device)."""
        _check(lib().ookd_rx_submit_device(self._h, d_iq_ptr, num_captures, samples_per_capture,
                                           stride if stride is not None else samples_per_capture))

    def wait(self) -> None:
        """Block until the submitted run's results are in host memory (ookd_rx_wait)."""
        _check(lib().ookd_rx_wait(self._h))

    def result(self) -> RxResult:
        return self._result()

    def raw_stats(self) -> RxStats:
        s = RxStats()
        _check(lib().ookd_rx_get_stats(self._h, C.byref(s)))
        return s

    def rx(self, iq: np.ndarray) -> RxResult:
        """Host capture (staged over PCIe first): 2 n values I,Q of the context's sample format -- int16 for
        "sc16q11" (anything numpy converts, as before), an int8 array for "cs8", a uint8 array for "cu8"."""
        iq = self._samples(iq)
        _check(lib().ookd_rx_process_host(self._h, iq.ctypes.data, iq.size // 2))
        return self._result()

    def shard_begin(self, d_iq_ptr: int, num_samples: int, halo: Optional[np.ndarray],
                    last_shard: bool, state_in: Optional[FsmState]) -> Tuple[RxResult, FsmState]:
        out = FsmState()
        hp, hn = None, 0
        if halo is not None and hasattr(halo, "data_ptr"):
            # a device (or host) tensor an RCCL recv landed in: handed over as it is, never staged through numpy
            hp, hn = halo.data_ptr(), halo.numel() // 2
        elif halo is not None:
            halo = self._samples(halo)
            hp, hn = halo.ctypes.data, halo.size // 2
        _check(lib().ookd_rx_shard_begin(self._h, d_iq_ptr, num_samples, hp, hn, int(last_shard),
                                         C.byref(state_in) if state_in is not None else None,
                                         C.byref(out)))
        return self._result(), out

    def shard_refine(self, state_in: FsmState) -> Tuple[RxResult, FsmState]:
        out = FsmState()
        _check(lib().ookd_rx_shard_refine(self._h, C.byref(state_in), C.byref(out)))
        return self._result(), out

    def _samples(self, iq) -> np.ndarray:
        """A host array as contiguous samples of this context's format; an 8-bit context takes its own dtype only
        (converting would silently reinterpret the other format's bytes)."""
        if self.sample_format != "sc16q11" and np.asarray(iq).dtype != self._sample_dtype:
            raise TypeError("this Receiver takes %s samples as %s, not %s"
                            % (self.sample_format, np.dtype(self._sample_dtype).name, np.asarray(iq).dtype.name))
        return np.ascontiguousarray(iq, dtype=self._sample_dtype).reshape(-1)

    @property
    def sample_bytes(self) -> int:
        """Bytes per input sample: 4 (sc16q11) or 2 (cs8, cu8)."""
        return int(lib().ookd_rx_sample_bytes(self._h))

    @property
    def halo_samples(self) -> int:
        return int(lib().ookd_rx_halo_samples(self._h))

    @staticmethod
    def state_from_bytes(raw: bytes) -> FsmState:
        return FsmState.from_buffer_copy(raw)

    # -- results --------------------------------------------------------------
    def stats(self) -> dict:
        s = RxStats()
        _check(lib().ookd_rx_get_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in RxStats._fields_}

    def front_info(self) -> dict:
        """The front end this context runs (form: FRONT_*) and the per-component error bounds its guard
        bands were built from, in output units (2048 LSB = 1)."""
        f = FrontInfo()
        _check(lib().ookd_rx_get_front_info(self._h, C.byref(f)))
        return {name: getattr(f, name) for name, _ in FrontInfo._fields_}

    def _result(self) -> RxResult:
        n = int(lib().ookd_rx_num_messages(self._h))
        pb = self.payload_bytes
        caps = np.zeros(n, dtype=np.uint32)
        samples = np.zeros(n, dtype=np.uint64)
        pay = np.zeros((n, pb), dtype=np.uint8)
        if n:
            raw = np.ctypeslib.as_array(
                C.cast(lib().ookd_rx_messages(self._h), C.POINTER(C.c_uint8)),
                shape=(n, C.sizeof(Message))).copy()
            caps = raw[:, 0:4].copy().view(np.uint32).reshape(-1)
            samples = raw[:, 8:16].copy().view(np.uint64).reshape(-1)
            pay = raw[:, 16:16 + pb].copy()
        return RxResult(caps, samples, pay, self.stats())

    def bits(self, capture: int = 0) -> np.ndarray:
        """Thresholded stream as one uint8 per decimated sample."""
        nw = int(lib().ookd_rx_bit_words(self._h))
        words = np.zeros(max(nw, 1), dtype=np.uint64)
        _check(lib().ookd_rx_get_bits(self._h, capture, words.ctypes.data, nw))
        n = self.stats()["decimated_samples"]
        return np.unpackbits(words[:nw].view(np.uint8), bitorder="little")[:n]

    def edges(self, capture: int = 0, clean: bool = False) -> np.ndarray:
        """The capture's edge list; clean=True: its cleaned list (`clean_edges` first)."""
        get = lib().ookd_rx_get_clean_edges if clean else lib().ookd_rx_get_edges
        n = C.c_uint64(0)
        _check(get(self._h, capture, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint64)
        _check(get(self._h, capture, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def fir_output(self, capture: int = 0) -> np.ndarray:
        n = self.stats()["decimated_samples"]
        out = np.zeros((max(n, 1), 2), dtype=np.float32)
        _check(lib().ookd_rx_get_fir(self._h, capture, out.ctypes.data, n))
        return out[:n]

    # -- recorders (ookiedokie.c:146-169, :265-270) -------------------------------
    def dig_text(self, capture: int = 0) -> str:
        """The text --rx-rec-dig would hold for this capture."""
        need = lib().ookd_rx_dig_text(self._h, capture, None, 0)
        if need == 0 and last_error():
            raise OokdError(-1, last_error())
        buf = C.create_string_buffer(need + 1)
        lib().ookd_rx_dig_text(self._h, capture, buf, len(buf))
        return buf.value.decode("ascii")

    def record_dig(self, path: str, capture: int = 0) -> None:
        _check(lib().ookd_rx_record_dig(self._h, capture, os.fsencode(path)))

    def fir_sc16q11(self, capture: int = 0) -> np.ndarray:
        """Post-filter samples as SC16Q11 (needs keep_fir): what --rx-rec records."""
        n = self.stats()["decimated_samples"]
        out = np.zeros(2 * max(n, 1), dtype=np.int16)
        _check(lib().ookd_rx_get_fir_sc16q11(self._h, capture, out.ctypes.data, n))
        return out[:2 * n]

    def record_fir(self, path: str, capture: int = 0) -> None:
        _check(lib().ookd_rx_record_fir(self._h, capture, os.fsencode(path)))

    def errors(self, cap: int = 1 << 16) -> Tuple[np.ndarray, int]:
        n = C.c_uint64(0)
        out = np.zeros(cap, dtype=np.uint64)
        _check(lib().ookd_rx_get_errors(self._h, out.ctypes.data, cap, C.byref(n)))
        return out[:min(cap, n.value)], int(n.value)

    # -- edge cleaning ---------------------------------------------------------------
    def clean_edges(self, min_on: int = 0, min_off: int = 0) -> List[dict]:
        """Deletes the runs shorter than min_on ("on" runs) / min_off ("off" runs) decimated samples from every
        capture's (carrier's) edge list of the last run, on the GPU, into a second list (ookd_rx_clean_edges; the rule
        is `clean_edges` at module level).  0 and 1 keep every run of that level.  The run's own list and results stay
        what they were; `edges`, `pulse_hist` and `symbol_survey` read the cleaned list with clean=True.  Returns per
        capture edges_in, edges_out, deleted ([off runs, on runs]), min_on, min_off."""
        _check(lib().ookd_rx_clean_edges(self._h, int(min_on), int(min_off)))
        out = []
        info = CleanInfo()
        # (the call above answered the last run: the first refusal is the capture behind the run's last)
        while lib().ookd_rx_get_clean_info(self._h, len(out), C.byref(info)) == 0:
            out.append(dict(edges_in=int(info.edges_in), edges_out=int(info.edges_out),
                            deleted=[int(info.deleted[0]), int(info.deleted[1])], min_on=int(info.min_on),
                            min_off=int(info.min_off)))
        return out

    @property
    def clean_kernel_ms(self) -> float:
        """HIP-event time of the pass behind `clean_edges` for the last run; 0 while nobody has asked for it."""
        return float(lib().ookd_rx_clean_kernel_ms(self._h))

    # -- pulse survey ----------------------------------------------------------------
    def pulse_hist(self, capture: int = 0, clean: bool = False) -> dict:
        """Run-length histograms of one capture (or carrier) of the last run (ookd_rx_pulse_hist): `count` and `sum`
        as uint64 arrays [2, 512] indexed [level, bin] (level 1 = "on" runs), `runs` [2], and the scalars num_edges,
        samples, open_head, open_tail, tail_level.  Computed on the GPU for all captures at the first call after a
        run.  Feed it to `suggest_pulses`.  clean=True: of the cleaned list (`clean_edges` first)."""
        h = PulseHist()
        _check((lib().ookd_rx_pulse_hist_clean if clean else lib().ookd_rx_pulse_hist)(self._h, capture, C.byref(h)))
        return _pulse_hist_dict(h)

    @property
    def pulse_kernel_ms(self) -> float:
        """HIP-event time of the pass behind `pulse_hist` for the last run; 0 while nobody has asked about it."""
        return float(lib().ookd_rx_pulse_kernel_ms(self._h))

    # -- symbol survey ---------------------------------------------------------------
    def symbol_survey(self, table, roles=None, capture: int = 0, clean: bool = False) -> dict:
        """Pulse/gap symbols of one capture (or carrier) of the last run, counted on the GPU at every call
        (ookd_rx_symbol_survey).  `table` is a class table (`symbol_table_from_pulses`, or a dict with `lower` and
        `upper`: per level -- 0 = off, 1 = on -- a list of inclusive bounds); `roles` a uint8 array [17, 17] indexed
        [on class, off class] (`suggest_coding` makes one), or None for the kind counts alone.  Returns num_symbols,
        kinds (uint64 [17, 17]), num_syncs, head_symbols, tail_symbols and frames (uint64 [2, 512], [clean, distance]).
        clean=True: of the cleaned list (`clean_edges` first)."""
        t = _symbol_table_struct(table)
        r = None
        if roles is not None:
            a = np.ascontiguousarray(roles, dtype=np.uint8)
            if a.shape != (SYMBOL_KINDS, SYMBOL_KINDS):
                raise ValueError("roles have shape (%d, %d)" % (SYMBOL_KINDS, SYMBOL_KINDS))
            r = SymbolRoles()
            C.memmove(r.role, a.ctypes.data, a.nbytes)
        out = SymbolSurvey()
        survey = lib().ookd_rx_symbol_survey_clean if clean else lib().ookd_rx_symbol_survey
        _check(survey(self._h, capture, C.byref(t), C.byref(r) if r is not None else None, C.byref(out)))
        return _symbol_survey_dict(out)

    @property
    def symbol_kernel_ms(self) -> float:
        """HIP-event time of the last `symbol_survey` call's pass; 0 when it was refused or had nothing to launch."""
        return float(lib().ookd_rx_symbol_kernel_ms(self._h))

    def suggest_device(self, sample_rate: float, capture: int = 0, min_on: int = 0, min_off: int = 0) -> dict:
        """The whole chain for one capture of the last run: pulse_hist -> suggest_pulses -> class table -> kind
        counts -> suggest_coding -> frames -> `suggest_device`'s dict (found = 0 with a reason when the capture does
        not look like a sync + distance-coded device).  sample_rate is that of the decimated samples.  With min_on or
        min_off above 1 the list is cleaned first (`clean_edges`) and the chain runs on the cleaned list."""
        clean = min_on > 1 or min_off > 1
        if clean:
            self.clean_edges(min_on, min_off)
        pulses = suggest_pulses(self.pulse_hist(capture, clean), sample_rate)
        table = symbol_table_from_pulses(pulses)
        coding = suggest_coding(pulses, self.symbol_survey(table, None, capture, clean))
        survey = self.symbol_survey(table, coding["roles"], capture, clean) if coding["found"] else \
            dict(num_syncs=0, frames=np.zeros((2, FRAME_BINS), dtype=np.uint64))
        return suggest_device(pulses, survey, coding, sample_rate)

    # -- pulse levels ----------------------------------------------------------------
    def run_levels(self, capture: int = 0, clean: bool = False) -> dict:
        """The peak power of every on-run of one capture (or carrier) of the last run (ookd_rx_run_levels): `peaks`
        float32 [num_runs] -- run r begins at edge 2 r of `edges(capture, clean)` --, `hist` (uint64 [256], the peaks
        under `level_bin`), num_runs, tile_outputs, tiles_total and tiles_filtered (the tiles that held an on sample:
        the only ones the pass filtered).  Computed on the GPU for all captures at the first call after a run, from
        the capture itself: a capture handed over as a device pointer stays resident and unchanged until then.
        clean=True: over the cleaned list (`clean_edges` first, or a debounced context)."""
        out = RunLevels()
        _check((lib().ookd_rx_run_levels_clean if clean else lib().ookd_rx_run_levels)(self._h, capture, C.byref(out)))
        peaks = np.zeros(max(int(out.num_runs), 1), dtype=np.float32)
        n = C.c_uint64(0)
        get = lib().ookd_rx_get_run_peaks_clean if clean else lib().ookd_rx_get_run_peaks
        _check(get(self._h, capture, peaks.ctypes.data, int(out.num_runs), C.byref(n)))
        return dict(num_runs=int(out.num_runs), tiles_total=int(out.tiles_total), tiles_filtered=int(out.tiles_filtered),
                    tile_outputs=int(out.tile_outputs), hist=np.array(out.hist.bins, dtype=np.uint64),
                    peaks=peaks[:int(n.value)])

    def message_levels(self, result: RxResult, pulses: Optional[int] = None, clean: bool = False) -> np.ndarray:
        """A power per message of `result` (this context's last run), float32 aligned with it: the lower median of the
        peaks of the message's last `pulses` on-runs (`message_levels` at module level; pulses defaults to the
        device's num_bits + 2).  10 log10 of it is the level in dBFS.  In a carrier context each message uses its
        carrier's list."""
        if pulses is None:
            if self._device is None:
                raise ValueError("pulses is needed on a context without a device")
            pulses = self._device.num_bits + 2
        out = np.zeros(len(result.msg_samples), dtype=np.float32)
        for c in np.unique(result.captures):
            m = np.nonzero(result.captures == c)[0]
            lv = self.run_levels(int(c), clean)
            out[m] = message_levels(self.edges(int(c), clean), lv["peaks"], result.msg_samples[m], pulses)
        return out

    @property
    def levels_kernel_ms(self) -> float:
        """HIP-event time of the pass behind `run_levels` for the last run; 0 while nobody has asked about it."""
        return float(lib().ookd_rx_levels_kernel_ms(self._h))

    # -- pulse moments ---------------------------------------------------------------
    def run_moments(self, capture: int = 0, clean: bool = False) -> dict:
        """The summed power and the summed lag-1 product of every on-run of one capture (or carrier) of the last run
        (ookd_rx_run_moments): int64 arrays `power`, `lag_re`, `lag_im` [num_runs], fixed point with 30 fraction bits
        -- run r begins at edge 2 r of `edges(capture, clean)` --, num_runs, tile_outputs, tiles_total, tiles_filtered
        and decimation.  Exact integers, whatever the order the GPU summed them in.  Computed for all captures at the
        first call after a run, from the capture itself, as `run_levels` is; clean=True: over the cleaned list."""
        out = RunMoments()
        _check((lib().ookd_rx_run_moments_clean if clean else lib().ookd_rx_run_moments)(self._h, capture, C.byref(out)))
        sums = np.zeros((max(int(out.num_runs), 1), 3), dtype=np.int64)
        n = C.c_uint64(0)
        get = lib().ookd_rx_get_run_moments_clean if clean else lib().ookd_rx_get_run_moments
        _check(get(self._h, capture, sums.ctypes.data, int(out.num_runs), C.byref(n)))
        sums = sums[:int(n.value)]
        return dict(num_runs=int(out.num_runs), tiles_total=int(out.tiles_total), tiles_filtered=int(out.tiles_filtered),
                    tile_outputs=int(out.tile_outputs), decimation=int(out.decimation),
                    power=sums[:, 0].copy(), lag_re=sums[:, 1].copy(), lag_im=sums[:, 2].copy())

    def message_carriers(self, result: RxResult, pulses: Optional[int] = None, clean: bool = False) -> dict:
        """Per message of `result` (this context's last run), aligned with it: `carrier` (cycles per input sample; the
        branch nearest the context's nu), `mean_power` (10 log10 of it is the level in dBFS), `coherence` (float64) and
        `outputs` (uint64), from the moments of the message's last `pulses` on-runs (`message_carriers` at module
        level; pulses defaults to the device's num_bits + 2).  In a carrier context each message uses its carrier's
        list and nu."""
        if pulses is None:
            if self._device is None:
                raise ValueError("pulses is needed on a context without a device")
            pulses = self._device.num_bits + 2
        count = len(result.msg_samples)
        out = dict(carrier=np.zeros(count), mean_power=np.zeros(count), coherence=np.zeros(count),
                   outputs=np.zeros(count, dtype=np.uint64))
        n_out = self.stats()["decimated_samples"]
        for c in np.unique(result.captures):
            m = np.nonzero(result.captures == c)[0]
            mo = self.run_moments(int(c), clean)
            nu = self.carrier(int(c))[0] if self.num_carriers else self.tune
            got = message_carriers(self.edges(int(c), clean), mo, result.msg_samples[m], pulses, mo["decimation"], nu, n_out)
            for key in out:
                out[key][m] = got[key]
        return out

    @property
    def moments_kernel_ms(self) -> float:
        """HIP-event time of the pass behind `run_moments` for the last run; 0 while nobody has asked about it."""
        return float(lib().ookd_rx_moments_kernel_ms(self._h))

    # -- burst extraction ------------------------------------------------------------
    def _burst_info(self, capture: int) -> BurstInfo:
        info = BurstInfo()
        _check(lib().ookd_rx_get_burst_info(self._h, capture, C.byref(info)))
        return info

    def bursts(self, pre: int, post: int, max_gap: int, clean: bool = False) -> List[dict]:
        """The burst table of every capture (or carrier) of the last run, made on the GPU (ookd_rx_bursts; the rule is
        `find_bursts` at module level): on-runs whose gaps are at most max_gap decimated samples form one burst, which
        reaches `pre` outputs in front of its first rise and `post` behind its last fall; max_gap >= pre + post.
        Returns per capture num_bursts, total_samples, num_runs, pre, post, max_gap, sample_bytes, tile_edges,
        decimation and the table as uint64 arrays first_sample, num_samples, offset (input samples), first_run and
        burst_runs.  The same parameters on the same run launch nothing.  clean=True: over the cleaned list
        (`clean_edges` first, or a debounced context).  `burst_samples` then returns the cut."""
        _check(lib().ookd_rx_bursts(self._h, int(pre), int(post), int(max_gap), BURSTS_CLEAN if clean else 0))
        out = []
        info = BurstInfo()
        # (the call above answered the last run: the first refusal is the capture behind the run's last)
        while lib().ookd_rx_get_burst_info(self._h, len(out), C.byref(info)) == 0:
            nb = int(info.num_bursts)
            table = np.zeros((max(nb, 1), len(BURST_FIELDS)), dtype=np.uint64)
            n = C.c_uint64(0)
            _check(lib().ookd_rx_get_bursts(self._h, len(out), table.ctypes.data, nb, C.byref(n)))
            table = table[:int(n.value)]
            d = {name: int(getattr(info, name)) for name, _ in BurstInfo._fields_ if name != "num_runs"}
            d["num_runs"] = int(info.num_runs)
            for k, name in enumerate(BURST_FIELDS):
                d["burst_runs" if name == "num_runs" else name] = table[:, k].copy()
            out.append(d)
        return out

    def burst_samples(self, capture: int = 0) -> np.ndarray:
        """The cut of one capture (in a carrier context: of the one capture, by carrier `capture`'s list) after
        `bursts`: [total_samples, 2] in the format's dtype -- sample offset[b] + i is sample first_sample[b] + i of
        the capture, byte for byte (ookd_rx_copy_bursts_host).  Only the cut crosses PCIe.  A capture handed over as a
        device pointer stays resident and unchanged until this returns."""
        total = int(self._burst_info(capture).total_samples)
        out = np.zeros((max(total, 1), 2), dtype=self._sample_dtype)
        _check(lib().ookd_rx_copy_bursts_host(self._h, capture, out.ctypes.data, total))
        return out[:total]

    def burst_samples_device(self, capture: int, ptr: int, capacity: int) -> int:
        """The same cut into device memory at `ptr` with room for `capacity` samples (ookd_rx_copy_bursts_device); a
        16-byte aligned `ptr` is copied in vectors.  Returns total_samples; nothing at or beyond it is written."""
        _check(lib().ookd_rx_copy_bursts_device(self._h, capture, ptr, int(capacity)))
        return int(self._burst_info(capture).total_samples)

    def message_bursts(self, result: RxResult, capture: Optional[int] = None) -> np.ndarray:
        """For each message of `result` (this context's last run) the index of the burst of its capture's table whose
        outputs [lo, hi) hold its `sample`, or -1; int64 aligned with the messages.  capture: only that capture's
        messages get an index (the others -1).  Host only, after `bursts`."""
        out = np.full(len(result.msg_samples), -1, dtype=np.int64)
        for c in np.unique(result.captures):
            if capture is not None and int(c) != int(capture):
                continue
            info = self._burst_info(int(c))
            nb = int(info.num_bursts)
            if nb == 0:
                continue
            table = np.zeros((nb, len(BURST_FIELDS)), dtype=np.uint64)
            _check(lib().ookd_rx_get_bursts(self._h, int(c), table.ctypes.data, nb, None))
            e = self.edges(int(c), bool(info.flags & BURSTS_CLEAN))
            n_out = self.stats()["decimated_samples"]
            r0 = table[:, 3].astype(np.int64)
            r1 = r0 + table[:, 4].astype(np.int64) - 1
            a = e[2 * r0].astype(np.int64)
            f = np.array([int(e[2 * r + 1]) if 2 * r + 1 < e.size else n_out for r in r1], dtype=np.int64)
            lo = a - np.minimum(a, int(info.pre))
            hi = np.minimum(n_out, f + int(info.post))
            m = np.nonzero(result.captures == c)[0]
            s = result.msg_samples[m].astype(np.int64)
            b = np.searchsorted(lo, s, side="right") - 1
            ok = (b >= 0) & (s < hi[np.maximum(b, 0)])
            out[m] = np.where(ok, b, -1)
        return out

    @property
    def bursts_kernel_ms(self) -> float:
        """HIP-event time of the pass behind `bursts` for the last run; 0 while nobody has asked about it."""
        return float(lib().ookd_rx_bursts_kernel_ms(self._h))

    @property
    def burst_copy_kernel_ms(self) -> float:
        """HIP-event time of the last `burst_samples` / `burst_samples_device` kernel about the last run."""
        return float(lib().ookd_rx_burst_copy_kernel_ms(self._h))

    # -- burst spectra ---------------------------------------------------------------
    def burst_spectra(self, capture: int = 0, span_frames: int = 0) -> dict:
        """A Welch spectrum of every burst of the table `bursts` last made for this run, summed on the GPU
        (ookd_rx_burst_spectra): per burst the arrays frames, total_power, dc_power (bins -1, 0, +1), peak_power and
        peak_bin (the largest of bins 2 .. 1022), and num_bursts, total_frames, span_frames, spans, partial_rows,
        flags, reduce_kernel_ms.  The input of `suggest_burst_carriers`.  The same run, table, capture and span
        launch nothing.  span_frames: 0, or a power of two >= 32 (the header has the rule)."""
        _check(lib().ookd_rx_burst_spectra(self._h, capture, int(span_frames)))
        info = BurstSpectraInfo()
        _check(lib().ookd_rx_get_burst_spectra_info(self._h, capture, C.byref(info)))
        nb = int(info.num_bursts)
        table = np.zeros(max(nb, 1), dtype=BURST_SPECTRUM_DTYPE)
        n = C.c_uint64(0)
        _check(lib().ookd_rx_get_burst_spectra(self._h, capture, table.ctypes.data, nb, C.byref(n)))
        d = dict(num_bursts=nb, total_frames=int(info.total_frames), span_frames=int(info.span_frames),
                 spans=int(info.spans), partial_rows=int(info.partial_rows), flags=int(info.flags),
                 reduce_kernel_ms=float(info.reduce_kernel_ms))
        for name in ("frames", "total_power", "dc_power", "peak_power", "peak_bin"):
            d[name] = table[name][:nb].copy()
        return d

    def burst_spectrum(self, burst: int, capture: int = 0) -> np.ndarray:
        """power_b[1024] (float64, FFT order) of one burst: the sums its entry of `burst_spectra` was taken from,
        made again by the same kernels over that burst alone (ookd_rx_burst_spectrum).  After `burst_spectra`."""
        r = SpectrumResult()
        _check(lib().ookd_rx_burst_spectrum(self._h, capture, int(burst), C.byref(r)))
        return np.frombuffer(bytes(r.power), dtype=np.float64).copy()

    def keyed_spectrum(self, capture: int = 0) -> SpectrumResult:
        """The Welch spectrum of the keyed part of the capture alone -- frames and power summed over its bursts
        (ookd_rx_get_keyed_spectrum); `suggest_carriers` takes it.  After `burst_spectra`."""
        r = SpectrumResult()
        _check(lib().ookd_rx_get_keyed_spectrum(self._h, capture, C.byref(r)))
        return r

    @property
    def burst_spectra_kernel_ms(self) -> float:
        """HIP-event time of the last `burst_spectra` pass about the last run; 0 while nobody has asked about it."""
        return float(lib().ookd_rx_burst_spectra_kernel_ms(self._h))

    # -- burst basebands -------------------------------------------------------------
    def baseband_info(self, capture: int = 0) -> dict:
        """The baseband table of the burst table `bursts` last made for this run (ookd_rx_get_baseband_info,
        ookd_rx_get_baseband_bursts; host work, the rule is `baseband_bursts` at module level): num_bursts,
        total_outputs, tiles_total, tiles_filtered (of the last `burst_baseband` about this table, else 0),
        tile_outputs, decimation, nu, turn (where the carrier sits in the cut, cycles per output) and per burst the
        uint64 arrays first_output, num_outputs, offset."""
        info = BasebandInfo()
        _check(lib().ookd_rx_get_baseband_info(self._h, capture, C.byref(info)))
        nb = int(info.num_bursts)
        table = np.zeros((max(nb, 1), len(BASEBAND_FIELDS)), dtype=np.uint64)
        n = C.c_uint64(0)
        _check(lib().ookd_rx_get_baseband_bursts(self._h, capture, table.ctypes.data, nb, C.byref(n)))
        table = table[:nb]
        d = {name: (float if name in ("nu", "turn") else int)(getattr(info, name)) for name, _ in BasebandInfo._fields_}
        for k, name in enumerate(BASEBAND_FIELDS):
            d[name] = table[:, k].copy()
        return d

    def burst_baseband(self, capture: int = 0, format: str = "cf32") -> np.ndarray:
        """The filter's complex output over every burst of the table `bursts` last made for this run, burst after
        burst (ookd_rx_burst_baseband_host): complex64 [total_outputs], or int16 [total_outputs, 2] for "sc16q11" --
        element offset[b] + i is y at output first_output[b] + i, in a tuned or carrier context through the list's
        own taps.  The rate is fs / decimation; nothing is derotated (`baseband_info`'s turn)."""
        fmt = BASEBAND_FORMATS[format]
        info = BasebandInfo()
        _check(lib().ookd_rx_get_baseband_info(self._h, capture, C.byref(info)))
        total = int(info.total_outputs)
        out = np.zeros(max(total, 1), dtype=np.complex64) if fmt == BASEBAND_CF32 else np.zeros((max(total, 1), 2), dtype=np.int16)
        _check(lib().ookd_rx_burst_baseband_host(self._h, capture, fmt, out.ctypes.data, total))
        return out[:total]

    def burst_baseband_device(self, capture: int, ptr: int, capacity: int, format: str = "cf32") -> int:
        """The same cut into device memory at `ptr` (aligned to its element: 8 bytes for "cf32", 4 for "sc16q11") with
        room for `capacity` outputs (ookd_rx_burst_baseband_device).  Returns total_outputs; nothing at or beyond it
        is written."""
        _check(lib().ookd_rx_burst_baseband_device(self._h, capture, BASEBAND_FORMATS[format], ptr, int(capacity)))
        info = BasebandInfo()
        _check(lib().ookd_rx_get_baseband_info(self._h, capture, C.byref(info)))
        return int(info.total_outputs)

    @property
    def baseband_kernel_ms(self) -> float:
        """HIP-event time of the filtering kernel of the last `burst_baseband` about the last run; 0 while nobody has
        asked or there was nothing to launch."""
        return float(lib().ookd_rx_baseband_kernel_ms(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().ookd_rx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------
# edge cleaning

def clean_edges(edges, min_on: int, min_off: int) -> np.ndarray:
    """ookd_clean_edges: an edge list without its runs shorter than min_on ("on" runs: the first, third, ...) /
    min_off ("off" runs) -- d(i) = short(i) and not d(i - 1); a deleted run takes its two edges with it.  Pure host code."""
    e = np.ascontiguousarray(edges, dtype=np.uint64)
    out = np.zeros(max(e.size, 1), dtype=np.uint64)
    n = C.c_uint64(0)
    _check(lib().ookd_clean_edges(e.ctypes.data if e.size else None, e.size, int(min_on), int(min_off), out.ctypes.data,
                                  e.size, C.byref(n)))
    return out[:n.value]


# --------------------------------------------------------------------------
# burst extraction

def find_bursts(edges, n_out: int, decimation: int, n: int, pre: int, post: int, max_gap: int) -> dict:
    """ookd_find_bursts: the bursts of one edge list -- on-runs joined across gaps of at most max_gap outputs, `pre`
    in front and `post` behind, in input samples clipped at n.  Returns num_bursts, total_samples and the table as
    uint64 arrays first_sample, num_samples, offset, first_run, burst_runs.  Pure host code."""
    e = np.ascontiguousarray(edges, dtype=np.uint64)
    cap = (e.size + 1) // 2
    table = np.zeros((max(cap, 1), len(BURST_FIELDS)), dtype=np.uint64)
    nb, total = C.c_uint64(0), C.c_uint64(0)
    _check(lib().ookd_find_bursts(e.ctypes.data if e.size else None, e.size, int(n_out), int(decimation), int(n), int(pre),
                                  int(post), int(max_gap), table.ctypes.data, cap, C.byref(nb), C.byref(total)))
    table = table[:int(nb.value)]
    d = dict(num_bursts=int(nb.value), total_samples=int(total.value))
    for k, name in enumerate(BURST_FIELDS):
        d["burst_runs" if name == "num_runs" else name] = table[:, k].copy()
    return d


# --------------------------------------------------------------------------
# burst basebands

def _baseband_rows(table) -> np.ndarray:
    if isinstance(table, dict):
        table = np.stack([np.asarray(table[k], dtype=np.uint64) for k in BASEBAND_FIELDS], axis=1)
    return np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, len(BASEBAND_FIELDS))


def baseband_bursts(table, decimation: int) -> dict:
    """ookd_baseband_bursts: the baseband table of a burst table (`find_bursts`' or `Receiver.bursts`' dict, or a
    uint64 array [B, 5]) -- per burst first_output = ceil(first_sample / D), num_outputs and offset as uint64 arrays,
    and num_bursts, total_outputs.  Pure host code."""
    if isinstance(table, dict):
        table = np.stack([np.asarray(table["burst_runs" if k == "num_runs" else k], dtype=np.uint64) for k in BURST_FIELDS], axis=1)
    t = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, len(BURST_FIELDS))
    nb = t.shape[0]
    out = np.zeros((max(nb, 1), len(BASEBAND_FIELDS)), dtype=np.uint64)
    total = C.c_uint64(0)
    _check(lib().ookd_baseband_bursts(t.ctypes.data if nb else None, nb, int(decimation), out.ctypes.data, nb, C.byref(total)))
    d = dict(num_bursts=nb, total_outputs=int(total.value))
    for k, name in enumerate(BASEBAND_FIELDS):
        d[name] = out[:nb, k].copy()
    return d


def baseband_of(y, table, format: str = "cf32") -> np.ndarray:
    """ookd_baseband_of: the burst basebands' contract on the host, given the filter's complex output y (complex64
    [n_out] or float32 [n_out, 2]) and a baseband table (`baseband_bursts`' or `Receiver.baseband_info`'s dict, or a
    uint64 array [B, 3]): complex64 [total], or int16 [total, 2] for "sc16q11".  Pure host code."""
    fmt = BASEBAND_FORMATS[format]
    y = np.asarray(y)
    if np.iscomplexobj(y):
        y = np.ascontiguousarray(y, dtype=np.complex64).view(np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, 2)
    t = _baseband_rows(table)
    total = int(t[:, 1].sum())
    out = np.zeros(max(total, 1), dtype=np.complex64) if fmt == BASEBAND_CF32 else np.zeros((max(total, 1), 2), dtype=np.int16)
    _check(lib().ookd_baseband_of(y.ctypes.data if y.size else None, y.shape[0], t.ctypes.data if t.size else None,
                                  t.shape[0], fmt, out.ctypes.data, total))
    return out[:total]


# --------------------------------------------------------------------------
# burst spectra

@dataclass
class BurstCarrier:
    nu: float           # bin centre, cycles per input sample: Receiver(carriers=[...])
    bin: int            # -512 .. 511
    bursts: int         # members
    frames: int         # and their frames
    power: float        # the sum of their peak_power


def burst_spectra_span(total_samples: int, span_frames: int = 0) -> int:
    """The span `Receiver.burst_spectra` uses for a cut of total_samples (ookd_burst_spectra_span): span_frames itself,
    or for 0 the smallest power of two >= 32 whose partial rows fit the workspace.  Raises as the call would."""
    used = C.c_uint32(0)
    _check(lib().ookd_burst_spectra_span(int(total_samples), int(span_frames), C.byref(used)))
    return int(used.value)


def suggest_burst_carriers(spectra, min_share: float = 0.0, min_spacing_bins: int = 0,
                           capacity: int = 16) -> Tuple[List[BurstCarrier], np.ndarray]:
    """ookd_suggest_burst_carriers over what `Receiver.burst_spectra` returns (a dict with the arrays frames,
    total_power, dc_power, peak_power, peak_bin): (carriers in decreasing weight, carrier_of_burst as int32, -1 = none).
    The rule is stated in the header.  Pure host code."""
    nb = len(spectra["frames"])
    table = np.zeros(max(nb, 1), dtype=BURST_SPECTRUM_DTYPE)
    for name in ("frames", "total_power", "dc_power", "peak_power", "peak_bin"):
        table[name][:nb] = np.asarray(spectra[name])
    out = (BurstCarrierStruct * max(1, capacity))()
    count = C.c_uint32(0)
    of = np.full(max(nb, 1), -1, dtype=np.int32)
    _check(lib().ookd_suggest_burst_carriers(table.ctypes.data if nb else None, nb, float(min_share), int(min_spacing_bins),
                                             C.addressof(out) if capacity else None, int(capacity), C.byref(count),
                                             of.ctypes.data))
    return ([BurstCarrier(c.nu, c.bin, int(c.bursts), int(c.frames), c.power) for c in out[:count.value]], of[:nb].copy())


# --------------------------------------------------------------------------
# pulse levels

def message_levels(edges, peaks, msg_samples, pulses: int) -> np.ndarray:
    """ookd_message_levels: message m takes the on-runs whose rising edge is <= msg_samples[m] and beyond the message
    before, of these the last `pulses`, and its level is the lower median of their peaks (0 without any).  One
    capture's edges, peaks (`Receiver.run_levels`) and ascending message samples.  Pure host code."""
    e = np.ascontiguousarray(edges, dtype=np.uint64)
    p = np.ascontiguousarray(peaks, dtype=np.float32)
    m = np.ascontiguousarray(msg_samples, dtype=np.uint64)
    out = np.zeros(max(m.size, 1), dtype=np.float32)
    _check(lib().ookd_message_levels(e.ctypes.data if e.size else None, e.size, p.ctypes.data if p.size else None, p.size,
                                     m.ctypes.data if m.size else None, m.size, int(pulses), out.ctypes.data))
    return out[:m.size]


# --------------------------------------------------------------------------
# pulse moments

def _moment_rows(moments) -> np.ndarray:
    if isinstance(moments, dict):
        moments = np.stack([np.asarray(moments[k], dtype=np.int64) for k in ("power", "lag_re", "lag_im")], axis=1)
    return np.ascontiguousarray(moments, dtype=np.int64).reshape(-1, 3)


def run_moments_of(y, edges) -> dict:
    """ookd_run_moments_of: the pulse moments' contract on the host, given the filter's complex output y [n_out, 2]
    float32 and one capture's edges: int64 arrays `power`, `lag_re`, `lag_im`, one entry per on-run.  Pure host
    code."""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, 2)
    e = np.ascontiguousarray(edges, dtype=np.uint64)
    runs = (e.size + 1) // 2
    out = np.zeros((max(runs, 1), 3), dtype=np.int64)
    _check(lib().ookd_run_moments_of(y.ctypes.data if y.size else None, y.shape[0], e.ctypes.data if e.size else None,
                                     e.size, out.ctypes.data if runs else None, runs))
    out = out[:runs]
    return dict(power=out[:, 0].copy(), lag_re=out[:, 1].copy(), lag_im=out[:, 2].copy())


def message_carriers(edges, moments, msg_samples, pulses: int, decimation: int, nu: float, n_out: int) -> dict:
    """ookd_message_carriers: message m takes the on-runs `message_levels` takes and adds their sums: `carrier`
    (cycles per input sample, the branch nearest nu), `mean_power`, `coherence` (float64) and `outputs` (uint64).
    moments: `Receiver.run_moments`'s or `run_moments_of`'s dict, or an int64 array [R, 3].  n_out ends an open last
    run.  Pure host code."""
    e = np.ascontiguousarray(edges, dtype=np.uint64)
    mo = _moment_rows(moments)
    m = np.ascontiguousarray(msg_samples, dtype=np.uint64)
    out = (MessageCarrier * max(m.size, 1))()
    _check(lib().ookd_message_carriers(e.ctypes.data if e.size else None, e.size, int(n_out),
                                       mo.ctypes.data if mo.size else None, mo.shape[0], m.ctypes.data if m.size else None,
                                       m.size, int(pulses), int(decimation), float(nu), out))
    rows = [out[k] for k in range(m.size)]
    return dict(carrier=np.array([r.carrier for r in rows], dtype=np.float64),
                mean_power=np.array([r.mean_power for r in rows], dtype=np.float64),
                coherence=np.array([r.coherence for r in rows], dtype=np.float64),
                outputs=np.array([r.outputs for r in rows], dtype=np.uint64))


# --------------------------------------------------------------------------
# pulse survey
# --------------------------------------------------------------------------

def pulse_bin(length: int) -> int:
    """The histogram bin of a run length in decimated samples (ookd_pulse_bin): 1 .. 31 their own bin, sixteen
    bins per octave from 32 on."""
    return int(lib().ookd_pulse_bin(int(length)))


def pulse_bin_lower(bin: int) -> int:
    """The shortest run a bin holds (ookd_pulse_bin_lower)."""
    return int(lib().ookd_pulse_bin_lower(int(bin)))


def _pulse_hist_dict(h: PulseHist) -> dict:
    return dict(num_edges=int(h.num_edges), samples=int(h.samples),
                runs=np.frombuffer(bytes(h.runs), dtype=np.uint64).copy(),
                count=np.frombuffer(bytes(h.count), dtype=np.uint64).reshape(2, PULSE_BINS).copy(),
                sum=np.frombuffer(bytes(h.sum), dtype=np.uint64).reshape(2, PULSE_BINS).copy(),
                open_head=int(h.open_head), open_tail=int(h.open_tail), tail_level=int(h.tail_level))


def suggest_pulses(hist, sample_rate: float) -> dict:
    """ookd_suggest_pulses: the timing classes of a histogram (`Receiver.pulse_hist`'s dict, or anything with `count`
    and `sum` arrays [2, 512]).  sample_rate is that of the decimated samples; 0 leaves the *_us members 0.  Returns
    found, dropped_runs [off, on] and classes [off, on]: lists of dicts (first_bin, last_bin, runs, mean, lower, upper,
    mean_us, lower_us, upper_us) in ascending length.  The rule is stated in the header.  Pure host code."""
    count = np.ascontiguousarray(hist["count"], dtype=np.uint64)
    total = np.ascontiguousarray(hist["sum"], dtype=np.uint64)
    if count.shape != (2, PULSE_BINS) or total.shape != (2, PULSE_BINS):
        raise ValueError("a pulse histogram has count and sum of shape (2, %d)" % PULSE_BINS)
    h = PulseHist()
    C.memmove(h.count, count.ctypes.data, count.nbytes)
    C.memmove(h.sum, total.ctypes.data, total.nbytes)
    out = PulseSuggestion()
    _check(lib().ookd_suggest_pulses(C.byref(h), float(sample_rate), C.byref(out)))
    classes = [[{name: getattr(out.classes[lv][i], name) for name, _ in PulseClass._fields_}
                for i in range(out.num_classes[lv])] for lv in range(2)]
    return dict(found=int(out.found), dropped_runs=[int(out.dropped_runs[0]), int(out.dropped_runs[1])],
                classes=classes)


# --------------------------------------------------------------------------
# symbol survey
# --------------------------------------------------------------------------

def _pulse_suggestion_struct(pulses) -> PulseSuggestion:
    """`suggest_pulses`'s dict back into the C structure"""
    s = PulseSuggestion()
    s.found = int(pulses["found"])
    for lv in range(2):
        classes = pulses["classes"][lv]
        if len(classes) > PULSE_MAX_CLASSES:
            raise ValueError("at most %d classes per level" % PULSE_MAX_CLASSES)
        s.num_classes[lv] = len(classes)
        s.dropped_runs[lv] = int(pulses["dropped_runs"][lv])
        for i, k in enumerate(classes):
            for name, _ in PulseClass._fields_:
                setattr(s.classes[lv][i], name, k[name])
    return s


def _symbol_table_struct(table) -> SymbolTable:
    t = SymbolTable()
    for lv in range(2):
        lower, upper = list(table["lower"][lv]), list(table["upper"][lv])
        if len(lower) != len(upper):
            raise ValueError("a class table has as many lower as upper bounds")
        t.num_classes[lv] = len(lower)              # (more than 16: the library refuses it)
        for k in range(min(len(lower), SYMBOL_MAX_CLASSES)):
            t.lower[lv][k] = int(lower[k])
            t.upper[lv][k] = int(upper[k])
    return t


def _symbol_survey_dict(s: SymbolSurvey) -> dict:
    return dict(num_symbols=int(s.num_symbols),
                kinds=np.frombuffer(bytes(s.kinds), dtype=np.uint64).reshape(SYMBOL_KINDS, SYMBOL_KINDS).copy(),
                num_syncs=int(s.num_syncs), head_symbols=int(s.head_symbols), tail_symbols=int(s.tail_symbols),
                frames=np.frombuffer(bytes(s.frames), dtype=np.uint64).reshape(2, FRAME_BINS).copy())


def _symbol_survey_struct(survey) -> SymbolSurvey:
    s = SymbolSurvey()
    for name in ("num_symbols", "num_syncs", "head_symbols", "tail_symbols"):
        setattr(s, name, int(survey.get(name, 0)))
    for name, shape in (("kinds", (SYMBOL_KINDS, SYMBOL_KINDS)), ("frames", (2, FRAME_BINS))):
        if name in survey:
            a = np.ascontiguousarray(survey[name], dtype=np.uint64)
            if a.shape != shape:
                raise ValueError("%s has shape %s" % (name, shape))
            C.memmove(getattr(s, name), a.ctypes.data, a.nbytes)
    return s


def _coding_struct(coding) -> Coding:
    c = Coding()
    for name, _ in Coding._fields_:
        if name != "reserved":
            setattr(c, name, coding[name])
    return c


def _device_suggestion_struct(suggestion) -> DeviceSuggestion:
    s = DeviceSuggestion()
    for name, _ in DeviceSuggestion._fields_:
        setattr(s, name, int(suggestion[name]))
    return s


def symbol_table_from_pulses(pulses) -> dict:
    """ookd_symbol_table_from_pulses: the class table of `suggest_pulses`'s classes, {lower, upper}: per level (0 =
    off, 1 = on) the inclusive bounds of every class, ascending."""
    t = SymbolTable()
    _check(lib().ookd_symbol_table_from_pulses(C.byref(_pulse_suggestion_struct(pulses)), C.byref(t)))
    return dict(lower=[[int(t.lower[lv][k]) for k in range(t.num_classes[lv])] for lv in range(2)],
                upper=[[int(t.upper[lv][k]) for k in range(t.num_classes[lv])] for lv in range(2)])


def suggest_coding(pulses, survey) -> dict:
    """ookd_suggest_coding: which kinds of symbols are the zero, the one and the sync, from `suggest_pulses`'s dict
    and the kind counts of `Receiver.symbol_survey`.  Returns found, reason (CODING_*), the classes and counts of the
    three kinds, t0_us / t1_us, and `roles` (uint8 [17, 17]) for the second `symbol_survey`.  Pure host code."""
    roles, out = SymbolRoles(), Coding()
    _check(lib().ookd_suggest_coding(C.byref(_pulse_suggestion_struct(pulses)), C.byref(_symbol_survey_struct(survey)),
                                     C.byref(roles), C.byref(out)))
    d = {name: getattr(out, name) for name, _ in Coding._fields_ if name != "reserved"}
    d["roles"] = np.frombuffer(bytes(roles.role), dtype=np.uint8).reshape(SYMBOL_KINDS, SYMBOL_KINDS).copy()
    return d


def suggest_device(pulses, survey, coding, sample_rate: float) -> dict:
    """ookd_suggest_device: the device of a coding and of the frames a `symbol_survey` with its roles counted: found,
    reason (CODING_*), num_bits, frame_symbols, the five durations in microseconds (sync_on_us, sync_off_us, bit_on_us,
    zero_off_us, one_off_us), frames_seen, frames_counted, frames_clean, num_syncs.  `Device.from_suggestion` and
    `device_suggestion_json` take the dict.  Pure host code."""
    out = DeviceSuggestion()
    _check(lib().ookd_suggest_device(C.byref(_pulse_suggestion_struct(pulses)), C.byref(_symbol_survey_struct(survey)),
                                     C.byref(_coding_struct(coding)), float(sample_rate), C.byref(out)))
    return {name: int(getattr(out, name)) for name, _ in DeviceSuggestion._fields_}


def device_suggestion_json(suggestion, name: str) -> str:
    """ookd_device_suggestion_json: the suggestion as a device file `Device.load` accepts."""
    s = _device_suggestion_struct(suggestion)
    n = lib().ookd_device_suggestion_json(C.byref(s), name.encode(), None, 0)
    if n == 0:
        raise OokdError(-1, last_error())
    buf = C.create_string_buffer(n + 1)
    lib().ookd_device_suggestion_json(C.byref(s), name.encode(), buf, n + 1)
    return buf.value.decode()


# --------------------------------------------------------------------------
# envelope survey
# --------------------------------------------------------------------------

def level_bin(power: float) -> int:
    """The histogram bin of a post-filter power (ookd_level_bin): four bins per octave, bin 0 below 2^-40."""
    return int(lib().ookd_level_bin(C.c_float(power)))


def level_bin_lower(bin: int) -> float:
    """The power at which a bin starts (ookd_level_bin_lower)."""
    return float(lib().ookd_level_bin_lower(bin))


def suggest_threshold(hist) -> dict:
    """ookd_suggest_threshold over 256 counts: found, threshold, off_level, on_level, split_bin, off_bin, on_bin,
    on_fraction (the rule is stated in the header).  Pure host code."""
    h = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1)
    if h.size != LEVEL_BINS:
        raise ValueError("a level histogram has %d bins, not %d" % (LEVEL_BINS, h.size))
    lh = LevelHist()
    lh.samples = int(h.sum(dtype=np.uint64))
    C.memmove(lh.bins, h.ctypes.data, h.nbytes)
    out = ThresholdSuggestion()
    _check(lib().ookd_suggest_threshold(C.byref(lh), C.byref(out)))
    return {name: getattr(out, name) for name, _ in ThresholdSuggestion._fields_}


class Survey:
    """Histogram of the post-filter power of whole captures in HBM (ookd_survey_*): what `Receiver`'s slicer
    will compare against `threshold`, counted before a threshold is chosen.

    tune / tune_hz with sample_rate: as `Receiver` takes them -- the survey of a carrier beside the capture's
    centre, counted through the taps `Filter.tuned_taps` returns (ookd_survey_create_tuned).  exact=True runs the
    tuned survey's generic form for every shape (same histogram; for cross-checks).

    carriers=[nu, ...] with stride=S (a power of two, 1 .. 64; default 1): the tuned survey of every carrier in
    one pass over the capture, counting the outputs with index 0 (mod S) (ookd_survey_create_carriers).
    `hist(capture, carrier)` is one carrier's histogram, `survey(iq)` returns all of them as [K, 256].

    tuned_fir2=True (with carriers; OOKD_RX_TUNED_FIR2, as `Receiver` takes it): a filter of two decimate-by-2 stages
    (<= 16 and <= 32 taps, the backend default fs128_fs16_dec4) is surveyed in one pass for all carriers, at every
    stride (SURVEY_TUNED_MULTI_FIR2; the same histograms).  No effect on other shapes or with exact=True."""

    def __init__(self, filt: Optional[Filter], *, hip_device: int = 0, max_captures: int = 1, stream: int = 0,
                 sample_format: str = "sc16q11", tune: Optional[float] = None, tune_hz: Optional[float] = None,
                 sample_rate: Optional[float] = None, exact: bool = False, carriers=None,
                 stride: Optional[int] = None, tuned_fir2: bool = False):
        if carriers is not None and (tune is not None or tune_hz is not None or sample_rate is not None):
            raise ValueError("give either carriers or tune / tune_hz, not both")
        if stride is not None and carriers is None:
            raise ValueError("stride needs carriers: only a carriers survey counts every stride-th output")
        if tuned_fir2 and carriers is None:
            raise ValueError("tuned_fir2 needs carriers: only a carriers survey has the fused two-stage form")
        if tune is not None and (tune_hz is not None or sample_rate is not None):
            raise ValueError("give either tune (cycles per sample) or tune_hz with sample_rate, not both")
        if (tune_hz is None) != (sample_rate is None):
            raise ValueError("tune_hz and sample_rate go together")
        if tune_hz is not None:
            if not sample_rate > 0:
                raise ValueError("sample_rate must be positive")
            tune = float(tune_hz) / float(sample_rate)
        if sample_format not in SAMPLE_FORMATS:
            raise ValueError("sample_format must be one of %s" % ", ".join(sorted(SAMPLE_FORMATS)))
        self.sample_format = sample_format
        fmt_flag, self._sample_dtype = SAMPLE_FORMATS[sample_format]
        self._filter = filt
        self.total_decimation = filt.total_decimation if filt else 1
        if carriers is not None:
            nus = [float(nu) for nu in carriers]
            tunes = (Tune * max(len(nus), 1))()
            for t, nu in zip(tunes, nus):
                t.nu = nu
            if stride is None:
                stride = 1
            if int(stride) != stride or not 0 <= stride < 2 ** 32:
                raise ValueError("stride must be a power of two in 1 .. %d" % SURVEY_MAX_STRIDE)
            self._h = lib().ookd_survey_create_carriers(hip_device, filt._h if filt else None,
                                                        fmt_flag | (RX_EXACT_FIR if exact else 0)
                                                        | (RX_TUNED_FIR2 if tuned_fir2 else 0), max_captures,
                                                        stream, tunes, len(nus), int(stride))
        elif tune is None and not exact:
            self._h = lib().ookd_survey_create(hip_device, filt._h if filt else None, fmt_flag, max_captures, stream)
        else:
            t = None                                            # exact alone: tune = NULL, the untuned survey
            if tune is not None:
                t = Tune()
                t.nu = float(tune)
            self._h = lib().ookd_survey_create_tuned(hip_device, filt._h if filt else None,
                                                     fmt_flag | (RX_EXACT_FIR if exact else 0), max_captures, stream,
                                                     C.byref(t) if t is not None else None)
        if not self._h:
            raise OokdError(-4, last_error())

    @property
    def tune(self) -> float:
        """Carrier offset this survey is tuned to, cycles per input sample (0: untuned)."""
        return float(lib().ookd_survey_tune(self._h))

    @property
    def form(self) -> int:
        """The kernel form a run takes: SURVEY_GENERIC, SURVEY_TUNED_GENERIC, SURVEY_TUNED_FIR1,
        SURVEY_TUNED_MULTI or SURVEY_TUNED_MULTI_FIR2."""
        return int(lib().ookd_survey_form(self._h))

    @property
    def num_carriers(self) -> int:
        """Carriers of a carriers survey; 0 for the other kinds."""
        return int(lib().ookd_survey_num_carriers(self._h))

    @property
    def stride(self) -> int:
        """Every stride-th output is counted; 1 but for a carriers survey made with another stride."""
        return int(lib().ookd_survey_stride(self._h))

    def survey_device(self, d_iq_ptr: int, samples_per_capture: int, num_captures: int = 1,
                      stride: Optional[int] = None) -> None:
        """Captures already resident in HBM (I,Q interleaved, in the survey's sample format)."""
        _check(lib().ookd_survey_device(self._h, d_iq_ptr, num_captures, samples_per_capture,
                                        stride if stride is not None else samples_per_capture))

    def survey(self, iq: np.ndarray) -> np.ndarray:
        """One host capture (staged over PCIe first), same arrays as `Receiver.rx` takes; returns its histogram
        (a carriers survey: every carrier's, [K, 256])."""
        if self.sample_format != "sc16q11" and np.asarray(iq).dtype != self._sample_dtype:
            raise TypeError("this Survey takes %s samples as %s, not %s"
                            % (self.sample_format, np.dtype(self._sample_dtype).name, np.asarray(iq).dtype.name))
        iq = np.ascontiguousarray(iq, dtype=self._sample_dtype).reshape(-1)
        _check(lib().ookd_survey_host(self._h, iq.ctypes.data, iq.size // 2))
        K = self.num_carriers
        return np.stack([self.hist(0, k) for k in range(K)]) if K else self.hist(0)

    def hist(self, capture: int = 0, carrier: int = 0) -> np.ndarray:
        """The 256 counts of one capture (and, of a carriers survey, one carrier) of the last run (uint64); they
        sum to `samples`."""
        lh = LevelHist()
        if self.num_carriers:
            _check(lib().ookd_survey_get_carrier_hist(self._h, capture, carrier, C.byref(lh)))
        else:
            if carrier:
                raise ValueError("only a carriers survey has carriers")
            _check(lib().ookd_survey_get_hist(self._h, capture, C.byref(lh)))
        self.samples = int(lh.samples)
        return np.frombuffer(bytes(lh.bins), dtype=np.uint64).copy()

    @property
    def kernel_ms(self) -> float:
        return float(lib().ookd_survey_kernel_ms(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().ookd_survey_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------
# carrier survey
# --------------------------------------------------------------------------

def spectrum_bin_nu(bin: int) -> float:
    """The carrier offset of a spectrum bin in cycles per input sample (ookd_spectrum_bin_nu)."""
    return float(lib().ookd_spectrum_bin_nu(int(bin) % SPECTRUM_BINS))


@dataclass
class Carrier:
    nu: float           # bin centre, cycles per input sample: Receiver(tune=nu)
    bin: int            # -512 .. 511
    at_dc: bool         # |bin| <= 1
    power: float
    ratio: float        # power / floor


def suggest_carriers(power_or_result, min_ratio: float = 0.0, min_spacing_bins: int = 0,
                     max_carriers: int = 16, frames: Optional[int] = None) -> Tuple[List[Carrier], float]:
    """ookd_suggest_carriers over 1024 powers, or over the (frames, power) pair `Spectrum.result` returns:
    (carriers in decreasing power, floor).  The rule is stated in the header.  Pure host code.  A bare power
    array counts as one frame unless `frames` says otherwise."""
    if isinstance(power_or_result, SpectrumResult):         # (Receiver.keyed_spectrum)
        power_or_result = (int(power_or_result.frames), np.frombuffer(bytes(power_or_result.power), dtype=np.float64))
    if isinstance(power_or_result, tuple):
        if frames is None:
            frames = int(power_or_result[0])
        power_or_result = power_or_result[1]
    pw = np.ascontiguousarray(power_or_result, dtype=np.float64).reshape(-1)
    if pw.size != SPECTRUM_BINS:
        raise ValueError("a spectrum has %d bins, not %d" % (SPECTRUM_BINS, pw.size))
    sp = SpectrumResult()
    sp.frames = 1 if frames is None else int(frames)
    C.memmove(sp.power, pw.ctypes.data, pw.nbytes)
    out = (CarrierStruct * max(1, max_carriers))()
    count, floor = C.c_uint32(0), C.c_double(0.0)
    _check(lib().ookd_suggest_carriers(C.byref(sp), float(min_ratio), int(min_spacing_bins), out,
                                       int(max_carriers), C.byref(count), C.byref(floor)))
    return ([Carrier(c.nu, c.bin, bool(c.at_dc), c.power, c.ratio) for c in out[:count.value]], floor.value)


class Spectrum:
    """Welch power spectrum of whole captures in HBM (ookd_spectrum_*): 1024-sample periodic-Hann frames summed
    per bin, the input of `suggest_carriers`."""

    def __init__(self, *, sample_format: str = "sc16q11", max_captures: int = 1, hip_device: int = 0,
                 stream: int = 0):
        if sample_format not in SAMPLE_FORMATS:
            raise ValueError("sample_format must be one of %s" % ", ".join(sorted(SAMPLE_FORMATS)))
        self.sample_format = sample_format
        fmt_flag, self._sample_dtype = SAMPLE_FORMATS[sample_format]
        self._h = lib().ookd_spectrum_create(hip_device, fmt_flag, max_captures, stream)
        if not self._h:
            raise OokdError(-4, last_error())

    def spectrum_device(self, d_iq_ptr: int, samples_per_capture: int, num_captures: int = 1,
                        stride: Optional[int] = None) -> None:
        """Captures already resident in HBM (I,Q interleaved, in the context's sample format)."""
        _check(lib().ookd_spectrum_device(self._h, d_iq_ptr, num_captures, samples_per_capture,
                                          stride if stride is not None else samples_per_capture))

    def spectrum(self, iq: np.ndarray) -> Tuple[int, np.ndarray]:
        """One host capture (staged over PCIe first), same arrays as `Receiver.rx` takes; returns its result."""
        if self.sample_format != "sc16q11" and np.asarray(iq).dtype != self._sample_dtype:
            raise TypeError("this Spectrum takes %s samples as %s, not %s"
                            % (self.sample_format, np.dtype(self._sample_dtype).name, np.asarray(iq).dtype.name))
        iq = np.ascontiguousarray(iq, dtype=self._sample_dtype).reshape(-1)
        _check(lib().ookd_spectrum_host(self._h, iq.ctypes.data, iq.size // 2))
        return self.result(0)

    def result(self, capture: int = 0) -> Tuple[int, np.ndarray]:
        """(whole frames summed, power[1024] float64 in FFT order) of one capture of the last run."""
        r = SpectrumResult()
        _check(lib().ookd_spectrum_get(self._h, capture, C.byref(r)))
        return int(r.frames), np.frombuffer(bytes(r.power), dtype=np.float64).copy()

    @property
    def kernel_ms(self) -> float:
        return float(lib().ookd_spectrum_kernel_ms(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().ookd_spectrum_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StreamFir:
    """fir_filter_and_decimate with carried state (fir.h:68-81), GPU backed."""

    def __init__(self, filt: Filter, max_input: int, hip_device: int = 0):
        self._filter = filt
        self.max_input = max_input
        self._h = lib().ookd_fir_create(hip_device, filt._h, max_input, 0)
        if not self._h:
            raise OokdError(-4, last_error())

    def reset(self) -> None:
        lib().ookd_fir_reset(self._h)

    def filter_and_decimate(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2)
        out = np.zeros((x.shape[0] + 2, 2), dtype=np.float32)
        n = lib().ookd_fir_filter_and_decimate(self._h, x.ctypes.data, x.shape[0], out.ctypes.data)
        err = last_error()
        if n == 0 and err:
            raise OokdError(-4, err)
        return out[:n].copy()

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().ookd_fir_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Synth:
    """Deterministic synthetic capture (same samples on host and device)."""

    def __init__(self, device: Device, num_samples: int, *, seed: int = 0x00C0FFEE,
                 sample_rate: int = DEFAULT_RATE, amplitude: int = 1945, noise: int = 40,
                 gap_us: Tuple[int, int] = (4000, 20000), glitch_every: int = 64,
                 random_phase: bool = True):
        cfg = SynthConfig(seed, sample_rate, amplitude, noise, gap_us[0], gap_us[1],
                          glitch_every, int(random_phase))
        self._device = device
        self.num_samples = num_samples
        self._h = lib().ookd_synth_create(device._h, C.byref(cfg), num_samples)
        if not self._h:
            raise OokdError(-1, last_error())

    @property
    def num_messages(self) -> int:
        return int(lib().ookd_synth_num_messages(self._h))

    def message(self, i: int) -> Tuple[int, bytes]:
        start = C.c_uint64(0)
        buf = (C.c_uint8 * MAX_PAYLOAD_BYTES)()
        _check(lib().ookd_synth_message(self._h, i, C.byref(start), buf))
        return int(start.value), bytes(buf)[:self._device.payload_bytes]

    def fill_host(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        count = self.num_samples - first if count is None else count
        out = np.zeros(2 * count, dtype=np.int16)
        _check(lib().ookd_synth_fill_host(self._h, first, count, out.ctypes.data))
        return out

    def fill_device(self, d_ptr: int, first: int = 0, count: Optional[int] = None,
                    hip_device: int = 0, stream: int = 0) -> None:
        count = self.num_samples - first if count is None else count
        _check(lib().ookd_synth_fill_device(self._h, hip_device, first, count, d_ptr, stream))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().ookd_synth_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipFileBackend:
    """The five backend functions of SDR_INTERFACE(hip_file, ...) as an object."""

    def __init__(self, path: str, *, rx: bool = True,
                 samples_per_buffer: int = DEFAULT_SAMPLES_PER_BUF):
        cfg = HostCfg()
        cfg.sdr_type = b"hip_file"
        cfg.direction = 0 if rx else 1
        self._path = os.fsencode(path)
        cfg.sdr_args = self._path
        cfg.samples_per_buffer = samples_per_buffer
        cfg.rx_threshold = DEFAULT_THRESHOLD
        cfg.samplerate = DEFAULT_RATE
        self._cfg = cfg
        self._h = lib().sdr_hip_file_init(C.byref(cfg))
        if not self._h:
            raise OokdError(-2, last_error())

    def rx(self, count: int) -> Tuple[int, np.ndarray]:
        out = np.zeros((count, 2), dtype=np.float32)
        status = lib().sdr_hip_file_rx(self._h, out.ctypes.data, count)
        return status, out

    def tx(self, samples: np.ndarray) -> int:
        samples = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1, 2)
        return lib().sdr_hip_file_tx(self._h, samples.ctypes.data, samples.shape[0])

    def flush(self) -> int:
        return lib().sdr_hip_file_flush(self._h)

    @property
    def sample_flags(self) -> int:
        """0, RX_SAMPLES_CS8 or RX_SAMPLES_CU8 by the file's name (sdr_hip_file_sample_flags)."""
        return int(lib().sdr_hip_file_sample_flags(self._h))

    @property
    def sample_format(self) -> str:
        """The `sample_format` a Receiver for capture() is created with."""
        return {0: "sc16q11", RX_SAMPLES_CS8: "cs8", RX_SAMPLES_CU8: "cu8"}[self.sample_flags]

    def capture(self) -> Tuple[int, int]:
        p, n = C.c_void_p(0), C.c_uint64(0)
        _check(lib().sdr_hip_file_capture(self._h, C.byref(p), C.byref(n)))
        return int(p.value or 0), int(n.value)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().sdr_hip_file_deinit(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
