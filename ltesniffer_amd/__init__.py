"""ltesniffer_amd - MI355X-native (gfx950, HIP) replacement of LTESniffer's per-subframe worker.

The product is the C-ABI shared library ``ltesniffer_amd/lib/libltesniffer_amd.so`` (include/ltesniffer_amd.h); this
module is only the ctypes binding used by tests, ``bench.py`` and ``__graft_entry__`` plus thin Python mirrors of the
reference's ``Phy`` / ``SubframeWorker`` pair (/root/reference/src/include/Phy.h:22-66,
/root/reference/src/include/SubframeWorker.h:16-86).  There is no CPU fallback: importing works without a GPU (so
that the symbol table can be checked), but creating a ``Phy`` without a HIP device raises.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

# (GPU_MAX_HW_QUEUES: the engine's 12 decode chains + 4 stage-A chains want 16 hardware queues, the HIP runtime's default is 4 and the value is read at
#  runtime initialisation.  That is the HOST PROGRAM's business - bench.py and tests/conftest.py export it; importing this module changes nothing in the
#  process environment (round-4 advisor finding) and the engine adapts its chain count to what it finds)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LSN_LIB_PATH") or os.path.join(_HERE, "lib", "libltesniffer_amd.so")  # LSN_LIB_PATH: A/B builds of the same library (tools/)

LSN_SUCCESS, LSN_ERROR, LSN_ERROR_INVALID_INPUTS, LSN_ERROR_NO_DEVICE = 0, -1, -2, -3
TAP_GRID, TAP_CE, TAP_PDCCH_LLR, TAP_CHEST, TAP_CFI, TAP_CANDIDATES, TAP_CCE_POWER, TAP_ACCEPTED, TAP_RB_POWER = range(9)
TAP_PDSCH_JOBS, TAP_PDSCH_LLR16, TAP_RM_WORDS, TAP_CB_RESULT = 9, 10, 11, 12   # stage C: indexed by decode job (lsn_phy_set_stage_c_taps)
KERNELS = ["k_ofdm", "k_chest", "k_chest_fin", "k_pcfich", "k_pdcch_llr", "k_cce_power", "k_viterbi", "k_pdsch_prep",
           "k_pdsch_demod", "k_turbo<64>", "k_rb_power", "k_turbo<128>", "k_rm"]

# every symbol include/ltesniffer_amd.h declares
EXPORTS = ["lsn_phy_create", "lsn_phy_destroy", "lsn_phy_set_cell", "lsn_phy_get_avail", "lsn_phy_put_pending",
           "lsn_phy_join_pending", "lsn_phy_set_pdu_sink", "lsn_phy_get_stats", "lsn_phy_get_est_cfo",
           "lsn_phy_add_evergreen", "lsn_phy_add_forbidden", "lsn_phy_setup_default_rnti_intervals",
           "lsn_phy_nof_active_rnti", "lsn_phy_get_ue_config", "lsn_worker_buffers", "lsn_worker_buffer_len", "lsn_worker_prepare",
           "lsn_worker_sf_idx", "lsn_worker_sfn", "lsn_phy_process_device", "lsn_phy_process_host", "lsn_phy_process_host_int", "lsn_phy_tap",
           "lsn_phy_get_perf", "lsn_kernel_name", "lsn_version", "lsn_pcap_open", "lsn_pcap_open_mem",
           "lsn_pcap_set_wall_clock", "lsn_pcap_write", "lsn_pcap_sink", "lsn_pcap_mem", "lsn_pcap_nof_records",
           "lsn_pcap_reset", "lsn_pcap_close", "lsn_phy_set_pcap_writer", "lsn_phy_set_api_mode", "lsn_phy_tracked_ul_modulation", "lsn_phy_set_ul_config", "lsn_phy_get_ul_config", "lsn_sib2_decode", "lsn_phy_pusch_decode",
           "lsn_phy_tap_ul", "lsn_phy_set_ul_timing", "lsn_phy_get_pusch_timing", "lsn_pusch_toa_decide", "lsn_phy_get_ul_ue_stats", "lsn_phy_set_prach_config", "lsn_phy_prach_detect", "lsn_phy_set_prach_sink", "lsn_prach_tti_opportunity", "lsn_phy_process_file", "lsn_phy_mib_decode", "lsn_phy_mib_decode_llr", "lsn_phy_submit_device", "lsn_phy_wait", "lsn_cell_search",
           "lsn_phy_set_shortcut_discovery", "lsn_phy_get_shortcut_discovery", "lsn_phy_set_histogram_threshold", "lsn_phy_print_stats",
           "lsn_phy_set_mcs_update_interval", "lsn_phy_update_mcs_database", "lsn_phy_nof_tracked_rnti", "lsn_worker_buffers_offset", "lsn_pcap_digest", "lsn_pcap_set_store", "lsn_pcap_set_digest_blocks", "lsn_pcap_block_digests", "lsn_phy_create_multi", "lsn_phy_nof_devices",
           "lsn_phy_set_cfo_correction", "lsn_phy_get_cfo_correction", "lsn_phy_set_candidate_pruning", "lsn_phy_set_stage_c_taps", "lsn_phy_prepare_file", "lsn_phy_get_meta_formats", "lsn_phy_nof_workers", "lsn_phy_worker",
           "lsn_phy_set_sampling", "lsn_phy_get_sampling", "lsn_symbol_sz", "lsn_sampling_freq_hz", "lsn_cell_search_rates",
           "lsn_resample", "lsn_resample_span", "lsn_phy_process_file_rate", "lsn_resample_cells", "lsn_file_cells_span", "lsn_file_process_cells",
           "lsn_clock_plan", "lsn_clock_fit", "lsn_clock_replica", "lsn_clock_track", "lsn_clock_estimate", "lsn_file_clock_estimate",
           "lsn_carrier_scan_plan", "lsn_carrier_scan_decide", "lsn_carrier_scan", "lsn_file_carrier_scan", "lsn_carrier_channel", "lsn_carrier_channel_span",
           "lsn_phy_set_channel_filter", "lsn_channel_filter_design", "lsn_channel_filter", "lsn_channel_filter_span", "lsn_cells_stopbands",
           "lsn_resample_cells_ring", "lsn_stream_open", "lsn_stream_push", "lsn_stream_flush", "lsn_stream_status", "lsn_stream_close", "lsn_stream_span",
           "lsn_stream_track", "lsn_stream_track_status", "lsn_stream_track_step", "lsn_pss_timing", "lsn_pss_timing_error",
           "lsn_channel_filter_ring", "lsn_stream_span_filtered",
           "lsn_stream_reacquire", "lsn_stream_reacquire_status", "lsn_pss_acquire", "lsn_pss_acquire_decide",
           "lsn_phy_mib_decode_side", "lsn_stream_frame_sync", "lsn_stream_frame_sync_status", "lsn_frame_sync_decide",
           "lsn_cell_search_all", "lsn_pss_cancel", "lsn_sss_accumulate", "lsn_cell_search_all_plan", "lsn_cell_search_all_decide",
           "lsn_cell_search_ant",
           "lsn_phy_set_antenna_map", "lsn_resample_cells_map", "lsn_resample_cells_ring_map", "lsn_file_cells_span_map", "lsn_stream_span_map"]

RATES_3GPP, RATES_SRSRAN = 0, 1   # LSN_RATES_*: sampling mode of a Phy / of a cell search


def symbol_sz(nof_prb, rates=RATES_3GPP):
    """samples per OFDM symbol of a capture of this bandwidth in this sampling mode (lsn_symbol_sz); 0: no such bandwidth / mode"""
    return int(lib().lsn_symbol_sz(int(nof_prb), int(rates)))


def sampling_freq_hz(nof_prb, rates=RATES_3GPP):
    """15 kHz x symbol_sz (lsn_sampling_freq_hz); 0: no such bandwidth / mode"""
    return int(lib().lsn_sampling_freq_hz(int(nof_prb), int(rates)))


def turbo_nwin(K):
    """windows the turbo decoder cuts a block of K bits into (lsn_rm.h: lsn_turbo_nwin)"""
    p1 = p2 = 1
    for P in range(min(K // 32, 128), 0, -1):
        if K % P == 0:
            p2 = P
            break
    for P in range(min(K // 32, 64), 0, -1):
        if K % P == 0:
            p1 = P
            break
    return p2 if p2 >= 96 else p1


def unpack_rm_words(w, K):
    """the K + 12 uint32 words k_rm hands to k_turbo for one code block -> int16[3, K + 4], the de-rate-matched streams d0 | d1 | d2: word
    (x % W) * P + x // W carries the three 10-bit fields of trellis position x, words K + 4 s + j the termination value j of stream s"""
    w = np.asarray(w, dtype=np.uint32)
    P = turbo_nwin(K)
    W = K // P
    x = np.arange(K)
    ww = w[(x % W) * P + x // W]
    d3 = np.zeros((3, K + 4), dtype=np.int16)
    for s_ in range(3):
        f = ((ww >> (10 * s_)) & 0x3FF).astype(np.int32)
        d3[s_, :K] = np.where(f >= 512, f - 1024, f)
        d3[s_, K:] = w[K + 4 * s_:K + 4 * s_ + 4].view(np.int32)
    return d3


PRACH_NCS = [0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419]  # 36.211 Table 5.7.2-2


class Mib(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("found", "sfn", "sfn_offset", "nof_prb", "nof_ports", "phich_length", "phich_resources_x6", "mib_bits")]


TTI_FROM_MIB = 0xFFFFFFFF


class UeConfig(C.Structure):
    _fields_ = [("has_ue_config", C.c_uint32), ("p_a_db", C.c_float), ("i_offset_ack", C.c_uint32), ("i_offset_cqi", C.c_uint32),
                ("i_offset_ri", C.c_uint32), ("cqi_type", C.c_uint32)]


class CellSearchCfg(C.Structure):
    _fields_ = [("nof_periods", C.c_uint32), ("force_n_id_2", C.c_int32), ("threshold", C.c_float)]


class CellSearch(C.Structure):
    _fields_ = [("found", C.c_uint32), ("cell_id", C.c_uint32), ("n_id_2", C.c_uint32), ("n_id_1", C.c_uint32), ("sf_idx", C.c_uint32),
                ("pss_pos", C.c_uint32), ("sf_start", C.c_uint32), ("pss_peak", C.c_float), ("pss_p2avg", C.c_float),
                ("sss_metric", C.c_float), ("sss_second", C.c_float), ("cfo_hz", C.c_float), ("cfo_coarse_hz", C.c_float), ("cp", C.c_uint32)]


class CellSearchAnt(C.Structure):   # lsn_cell_search_ant_t
    _fields_ = [("pss_peak", C.c_float), ("sss_metric", C.c_float), ("sss_second", C.c_float), ("cfo_hz", C.c_float), ("n_id_1", C.c_uint32), ("occurrence", C.c_uint32)]


class CellSearchAllCfg(C.Structure):   # lsn_cell_search_all_cfg_t
    _fields_ = [("nof_periods", C.c_uint32), ("force_n_id_2", C.c_int32), ("threshold", C.c_float), ("threshold_next", C.c_float), ("sss_ratio_min", C.c_float),
                ("shared_pss_ratio", C.c_float), ("max_cells", C.c_uint32)]


class CellFound(C.Structure):   # lsn_cell_found_t
    _fields_ = [("cell", CellSearch), ("round", C.c_uint32), ("shared_pss", C.c_uint32), ("sss_ratio", C.c_float), ("rel_power_db", C.c_float)]


class CellSearchAllPlan(C.Structure):   # lsn_cell_search_all_plan_t
    _fields_ = [("n_lo", C.c_uint32), ("n_lag", C.c_uint32), ("nof_runs", C.c_uint32), ("run_lo", C.c_uint32 * 2), ("run_len", C.c_uint32 * 2)]


class CellSearchAllDecision(C.Structure):   # lsn_cell_search_all_decision_t
    _fields_ = [("accept", C.c_uint32), ("cp", C.c_uint32), ("best", C.c_uint32), ("second", C.c_uint32), ("shared", C.c_uint32), ("runner_up", C.c_uint32),
                ("p2avg", C.c_float), ("sss_ratio", C.c_float), ("best_power", C.c_float), ("second_power", C.c_float), ("runner_up_power", C.c_float)]


class FileCfg(C.Structure):
    _fields_ = [("nof_antennas", C.c_uint32), ("offset_time_samples", C.c_int64), ("offset_freq_hz", C.c_float), ("sample_format", C.c_uint32),
                ("sample_scale", C.c_float)]


FILE_CF32, FILE_SC16, FILE_SC8 = 0, 1, 2


class FileRate(C.Structure):   # lsn_file_rate_t
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("sample_rate_hz", C.c_double), ("offset_time_frac", C.c_double),
                ("center_offset_hz", C.c_double)]


FILE_MAX_CELLS = 8


class FileCell(C.Structure):   # lsn_file_cell_t
    _fields_ = [("struct_size", C.c_uint32), ("nof_prb", C.c_uint32), ("rates", C.c_int), ("phy", C.c_void_p), ("center_offset_hz", C.c_double),
                ("offset_time_samples", C.c_int64), ("offset_time_frac", C.c_double), ("offset_freq_hz", C.c_float), ("start_tti", C.c_uint32),
                ("update_meta_period", C.c_uint32), ("max_subframes", C.c_uint64), ("subframes_done", C.c_uint64), ("status", C.c_int)]


class FileCellsSpan(C.Structure):   # lsn_file_cells_span_t
    _fields_ = [("in_lo", C.c_int64), ("in_hi", C.c_int64), ("blk_used", C.c_uint32), ("nof_active", C.c_uint32), ("first_subframe", C.c_uint64 * FILE_MAX_CELLS),
                ("nof_subframes", C.c_uint32 * FILE_MAX_CELLS), ("taps", C.c_uint32 * FILE_MAX_CELLS)]


class StreamCfg(C.Structure):   # lsn_stream_cfg_t
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("sample_rate_hz", C.c_double), ("nof_antennas", C.c_uint32), ("sample_format", C.c_uint32),
                ("sample_scale", C.c_float), ("block_subframes", C.c_uint32), ("ring_samples", C.c_uint64)]


class StreamStatus(C.Structure):   # lsn_stream_status_t
    _fields_ = [("samples_pushed", C.c_uint64), ("ring_samples", C.c_uint64), ("oldest_needed", C.c_int64), ("block_subframes", C.c_uint32), ("nof_cells", C.c_uint32),
                ("failed", C.c_int), ("status", C.c_int * FILE_MAX_CELLS), ("subframes_submitted", C.c_uint64 * FILE_MAX_CELLS)]


class StreamTrackCfg(C.Structure):   # lsn_stream_track_cfg_t
    _fields_ = [("struct_size", C.c_uint32), ("lost_after", C.c_uint32), ("kp", C.c_double), ("ki", C.c_double), ("max_ppm", C.c_double),
                ("cfo_hz", C.c_float * FILE_MAX_CELLS), ("initial_ppm", C.c_double * FILE_MAX_CELLS), ("enable", C.c_uint32 * FILE_MAX_CELLS)]


class StreamTrackStatus(C.Structure):   # lsn_stream_track_status_t
    _fields_ = [("struct_size", C.c_uint32), ("nof_cells", C.c_uint32), ("segments", C.c_uint64 * FILE_MAX_CELLS), ("valid", C.c_uint64 * FILE_MAX_CELLS),
                ("invalid", C.c_uint64 * FILE_MAX_CELLS), ("lost", C.c_uint32 * FILE_MAX_CELLS), ("last_error", C.c_double * FILE_MAX_CELLS),
                ("correction_ppm", C.c_double * FILE_MAX_CELLS), ("integrator_ppm", C.c_double * FILE_MAX_CELLS), ("position_drift", C.c_double * FILE_MAX_CELLS)]


class StreamTrackState(C.Structure):   # lsn_stream_track_state_t
    _fields_ = [("integrator", C.c_double), ("correction", C.c_double), ("invalid_run", C.c_uint32), ("lost", C.c_uint32)]


class PssTimingCell(C.Structure):   # lsn_pss_timing_cell_t
    _fields_ = [("struct_size", C.c_uint32), ("N", C.c_uint32), ("d", C.c_uint32), ("sflen", C.c_uint32), ("nof_antennas", C.c_uint32), ("nof_subframes", C.c_uint32),
                ("n_occ", C.c_uint32), ("reserved", C.c_uint32), ("blocks", C.c_void_p), ("replica", C.c_void_p), ("occ", C.c_void_p), ("C", C.c_void_p)]


class StreamReacquireCfg(C.Structure):   # lsn_stream_reacquire_cfg_t
    _fields_ = [("struct_size", C.c_uint32), ("after", C.c_uint32), ("min_ratio", C.c_double), ("enable", C.c_uint32 * FILE_MAX_CELLS)]


class StreamReacquireStatus(C.Structure):   # lsn_stream_reacquire_status_t
    _fields_ = [("struct_size", C.c_uint32), ("nof_cells", C.c_uint32), ("launched", C.c_uint64 * FILE_MAX_CELLS), ("accepted", C.c_uint64 * FILE_MAX_CELLS),
                ("rejected", C.c_uint64 * FILE_MAX_CELLS), ("last_peak", C.c_double * FILE_MAX_CELLS), ("last_ratio", C.c_double * FILE_MAX_CELLS),
                ("last_offset", C.c_int64 * FILE_MAX_CELLS), ("jump_segment", C.c_uint64 * FILE_MAX_CELLS), ("jumps_total", C.c_double * FILE_MAX_CELLS)]


FRAME_SYNC_NO_HOLD = 2   # LSN_FRAME_SYNC_NO_HOLD


class StreamFrameSyncCfg(C.Structure):   # lsn_stream_frame_sync_cfg_t
    _fields_ = [("struct_size", C.c_uint32), ("tries", C.c_uint32), ("hold", C.c_uint32), ("enable", C.c_uint32 * FILE_MAX_CELLS)]


class StreamFrameSyncStatus(C.Structure):   # lsn_stream_frame_sync_status_t
    _fields_ = [("struct_size", C.c_uint32), ("nof_cells", C.c_uint32), ("checks", C.c_uint64 * FILE_MAX_CELLS), ("attempts", C.c_uint64 * FILE_MAX_CELLS),
                ("confirmed", C.c_uint64 * FILE_MAX_CELLS), ("relabelled", C.c_uint64 * FILE_MAX_CELLS), ("given_up", C.c_uint64 * FILE_MAX_CELLS),
                ("accept_segment", C.c_uint64 * FILE_MAX_CELLS), ("relabel_segment", C.c_uint64 * FILE_MAX_CELLS), ("held", C.c_uint64 * FILE_MAX_CELLS),
                ("last_sfn", C.c_uint32 * FILE_MAX_CELLS), ("last_delta", C.c_int32 * FILE_MAX_CELLS), ("shift", C.c_uint32 * FILE_MAX_CELLS)]


class PssAcquireCell(C.Structure):   # lsn_pss_acquire_cell_t
    _fields_ = [("struct_size", C.c_uint32), ("N", C.c_uint32), ("d", C.c_uint32), ("sflen", C.c_uint32), ("nof_antennas", C.c_uint32), ("reserved", C.c_uint32),
                ("blocks", C.c_void_p), ("replica", C.c_void_p), ("C", C.c_void_p)]


class StreamSpan(C.Structure):   # lsn_stream_span_t
    _fields_ = [("ring_samples", C.c_uint64), ("block_input", C.c_uint64), ("oldest_needed", C.c_int64), ("oldest_needed_flushed", C.c_int64), ("block_subframes", C.c_uint32),
                ("reserved", C.c_uint32), ("subframes_complete", C.c_uint64 * FILE_MAX_CELLS), ("subframes_submitted", C.c_uint64 * FILE_MAX_CELLS),
                ("taps", C.c_uint32 * FILE_MAX_CELLS)]


class ResampleCfg(C.Structure):   # lsn_resample_cfg_t
    _fields_ = [("struct_size", C.c_uint32), ("nof_antennas", C.c_uint32), ("sample_format", C.c_uint32), ("sample_scale", C.c_float),
                ("rate_in_hz", C.c_double), ("rate_out_hz", C.c_double), ("first_sample", C.c_uint64), ("first_frac", C.c_double),
                ("in_base", C.c_uint64), ("out_first", C.c_uint64), ("passband_hz", C.c_double), ("center_offset_hz", C.c_double)]


MAP_MAX_OUT = 2   # LSN_MAP_MAX_OUT


class AntennaMap(C.Structure):   # lsn_antenna_map_t
    _fields_ = [("struct_size", C.c_uint32), ("nof_out", C.c_uint32), ("src_antenna", C.c_uint32 * MAP_MAX_OUT), ("offset_hz", C.c_double * MAP_MAX_OUT)]


def antenna_map(src=None, offset_hz=None):
    """-> AntennaMap: output antenna a is cut from input antenna src[a] at the cell's carrier + offset_hz[a] (None: all 0.0).  src None: the identity (nof_out 0)"""
    m = AntennaMap()
    m.struct_size = C.sizeof(AntennaMap)
    if src is None:
        return m
    src = list(src)
    off = [0.0] * len(src) if offset_hz is None else list(offset_hz)
    if len(off) != len(src):
        raise ValueError("antenna map: one offset per source antenna")
    m.nof_out = len(src)
    for a in range(min(len(src), MAP_MAX_OUT)):   # (more than MAP_MAX_OUT: nof_out says so and the library refuses)
        m.src_antenna[a], m.offset_hz[a] = int(src[a]), float(off[a])
    return m


class ResampleSpan(C.Structure):   # lsn_resample_span_t
    _fields_ = [("in_lo", C.c_int64), ("in_hi", C.c_int64), ("max_out", C.c_uint64), ("taps", C.c_uint32), ("reserved", C.c_uint32)]


class ChannelFilterDesign(C.Structure):   # lsn_channel_filter_design_t
    _fields_ = [("struct_size", C.c_uint32), ("half_len", C.c_uint32), ("nof_taps", C.c_uint32), ("reserved", C.c_uint32), ("cutoff", C.c_double)]


class ChannelFilterCfg(C.Structure):   # lsn_channel_filter_cfg_t
    _fields_ = [("struct_size", C.c_uint32), ("nof_antennas", C.c_uint32), ("sample_format", C.c_uint32), ("sample_scale", C.c_float),
                ("rate_in_hz", C.c_double), ("passband_hz", C.c_double), ("stopband_hz", C.c_double), ("center_offset_hz", C.c_double),
                ("in_base", C.c_uint64), ("out_first", C.c_uint64)]


class ClockCfg(C.Structure):   # lsn_clock_cfg_t
    _fields_ = [("struct_size", C.c_uint32), ("nof_prb", C.c_uint32), ("rates", C.c_int), ("n_id_2", C.c_uint32), ("pss_pos", C.c_uint64), ("cfo_hz", C.c_float),
                ("max_ppm", C.c_double), ("max_periods", C.c_uint32), ("sf_start", C.c_uint32)]


class ClockObs(C.Structure):   # lsn_clock_obs_t
    _fields_ = [("period", C.c_uint32), ("valid", C.c_uint32), ("centre", C.c_int64), ("half_width", C.c_uint32), ("reserved", C.c_uint32), ("pos", C.c_double),
                ("peak", C.c_float)]


class Clock(C.Structure):   # lsn_clock_t
    _fields_ = [("found", C.c_uint32), ("nof_periods", C.c_uint32), ("nof_used", C.c_uint32), ("nof_rounds", C.c_uint32), ("eps", C.c_double),
                ("sample_rate_hz", C.c_double), ("pss_pos0", C.c_double), ("rms_residual", C.c_double), ("max_residual", C.c_double), ("sf_start", C.c_double)]


class CarrierScanCfg(C.Structure):   # lsn_carrier_scan_cfg_t
    _fields_ = [("struct_size", C.c_uint32), ("nof_antennas", C.c_uint32), ("antenna", C.c_uint32), ("sample_format", C.c_uint32), ("sample_scale", C.c_float),
                ("nof_periods", C.c_uint32), ("rate_in_hz", C.c_double), ("raster_hz", C.c_double), ("raster_offset_hz", C.c_double), ("f_lo_hz", C.c_double),
                ("f_hi_hz", C.c_double), ("min_spacing_hz", C.c_double), ("threshold", C.c_float), ("reserved", C.c_uint32)]


class CarrierScanPlan(C.Structure):   # lsn_carrier_scan_plan_t
    _fields_ = [("nof_hypotheses", C.c_uint32), ("taps", C.c_uint32), ("nof_periods", C.c_uint32), ("reserved", C.c_uint32), ("nof_channel_samples", C.c_uint64),
                ("nof_input_samples", C.c_uint64)]


class CarrierMetric(C.Structure):   # lsn_carrier_metric_t
    _fields_ = [("k", C.c_int32), ("root", C.c_uint32), ("f_hz", C.c_double), ("tuning_word", C.c_uint64), ("lag", C.c_uint32), ("peak", C.c_float),
                ("p2avg", C.c_float), ("reserved", C.c_uint32)]


class Carrier(C.Structure):   # lsn_carrier_t
    _fields_ = [("center_offset_hz", C.c_double), ("k", C.c_int32), ("scan_p2avg", C.c_float), ("scan_root", C.c_uint32), ("scan_lag", C.c_uint32),
                ("search", CellSearch)]


class CarrierChannelCfg(C.Structure):   # lsn_carrier_channel_cfg_t
    _fields_ = [("struct_size", C.c_uint32), ("nof_antennas", C.c_uint32), ("sample_format", C.c_uint32), ("sample_scale", C.c_float), ("rate_in_hz", C.c_double),
                ("center_offset_hz", C.c_double), ("first_sample", C.c_uint64), ("first_frac", C.c_double), ("in_base", C.c_uint64), ("out_first", C.c_uint64)]


class ApiEvent(C.Structure):
    _fields_ = [("tti", C.c_uint32), ("rnti", C.c_uint16), ("id_type", C.c_uint32), ("msg_type", C.c_uint32), ("value", C.c_char * 24)]


API_SINK = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(ApiEvent))


class Sib2(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_sb", "hopping_mode", "pusch_hop_offset", "enable_64qam", "group_hopping_enabled", "group_assignment_pusch",
                                          "sequence_hopping_enabled", "cyclic_shift", "root_seq_idx", "prach_config_idx", "high_speed_flag",
                                          "zero_corr_zone", "prach_freq_offset")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def sib2_decode(pdu):
    """BCCH-DL-SCH-Message -> (verdict 0 / 1 / 2, dict of the SIB2 fields or None)"""
    s = Sib2()
    r = lib().lsn_sib2_decode(bytes(pdu), len(pdu), C.byref(s))
    return r, (s.as_dict() if r == 2 else None)


class PrachCfg(C.Structure):
    _fields_ = [("config_idx", C.c_uint32), ("root_seq_idx", C.c_uint32), ("zero_corr_zone", C.c_uint32), ("freq_offset", C.c_uint32),
                ("hs_flag", C.c_uint32), ("detect_factor", C.c_float), ("zc_roots", C.POINTER(C.c_uint16))]


class PrachDet(C.Structure):
    _fields_ = [("sf", C.c_uint32), ("preamble", C.c_uint32), ("offset", C.c_uint32), ("offset_sec", C.c_float), ("p2avg", C.c_float)]


PRACH_SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.POINTER(PrachDet), C.c_uint32)


class Cell(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("nof_prb", "nof_ports", "id", "cp", "phich_length", "phich_resources", "frame_type")]


class DlSfCfg(C.Structure):
    _fields_ = [("tti", C.c_uint32), ("cfi", C.c_uint32), ("sf_type", C.c_uint32)]


class PhyCfg(C.Structure):
    _fields_ = [("nof_rx_antennas", C.c_uint32), ("nof_workers", C.c_uint32), ("max_batch", C.c_uint32),
                ("skip_secondary_meta_formats", C.c_int), ("meta_format_split_ratio", C.c_double),
                ("histogram_threshold", C.c_uint32), ("mcs_tracking_mode", C.c_int), ("harq_mode", C.c_int),
                ("device", C.c_int), ("max_turbo_iterations", C.c_int), ("sniffer_mode", C.c_int)]


class PduCtx(C.Structure):
    _fields_ = [("tti", C.c_uint32), ("rnti", C.c_uint16), ("direction", C.c_uint8), ("rnti_type", C.c_uint8),
                ("crc_ok", C.c_uint8), ("is_retx", C.c_uint8), ("tb", C.c_uint8), ("reserved", C.c_uint8)]


class BlindStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("nof_locations", "nof_decoded_locations", "nof_cce", "nof_missed_cce",
                                          "nof_subframes", "nof_subframe_collisions_dw", "nof_subframe_collisions_up")]


class Perf(C.Structure):
    _fields_ = [("ms_stage_a", C.c_double), ("ms_search", C.c_double), ("ms_stage_c", C.c_double), ("ms_commit", C.c_double),
                ("ms_total", C.c_double), ("kernel_ms", C.c_double * 16), ("kernel_launches", C.c_uint64 * 16),
                ("algo_bytes", C.c_uint64), ("turbo_algo_bytes", C.c_uint64), ("turbo128_algo_bytes", C.c_uint64),
                ("nof_tb_decodes", C.c_uint64),
                ("nof_cb_decodes", C.c_uint64), ("nof_turbo_iterations", C.c_uint64), ("nof_candidates_decoded", C.c_uint64),
                ("nof_ondemand_decodes", C.c_uint64), ("nof_pdus", C.c_uint64), ("ms_search_core", C.c_double), ("ms_rar", C.c_double), ("turbo_cyc_rm", C.c_uint64),
                ("turbo_cyc_map", C.c_uint64), ("turbo_cyc_out", C.c_uint64), ("ms_wait_front", C.c_double), ("ms_wait_slot", C.c_double), ("ms_drain", C.c_double),
                ("nof_turbo_iterations_run", C.c_uint64), ("nof_ondemand_commit", C.c_uint64 * 4), ("ms_ondemand_commit", C.c_double), ("nof_pusch_2prb_skipped", C.c_uint64), ("nof_pusch_on_unverified_dmrs", C.c_uint64), ("nof_tb_on_derived_tbs", C.c_uint64),
                ("nof_decode_jobs", C.c_uint64), ("nof_decode_jobs_used", C.c_uint64), ("nof_speculative_jobs", C.c_uint64),
                ("jobs_by_kind", C.c_uint64 * 5), ("jobs_unused_by_kind", C.c_uint64 * 5), ("iters_by_kind", C.c_uint64 * 5), ("iters_unused_by_kind", C.c_uint64 * 5),
                ("nof_table_hints_used", C.c_uint64), ("nof_table_hints_missed", C.c_uint64), ("nof_candidate_misses", C.c_uint64), ("ms_harq", C.c_double * 3), ("nof_harq_combines", C.c_uint64 * 4)]


class UlCfg(C.Structure):
    _fields_ = [("cyclic_shift", C.c_uint32), ("delta_ss", C.c_uint32), ("hopping_offset", C.c_uint32), ("group_hopping_enabled", C.c_uint32),
                ("sequence_hopping_enabled", C.c_uint32)]


class PuschGrant(C.Structure):
    _fields_ = [("sf", C.c_uint32), ("rnti", C.c_uint16), ("n_dmrs", C.c_uint16), ("n_prb", C.c_uint32), ("L_prb", C.c_uint32),
                ("mod", C.c_uint32), ("tbs", C.c_uint32), ("rv", C.c_int), ("nof_ack", C.c_uint32), ("cqi_bits", C.c_uint32), ("ri_bits", C.c_uint32),
                ("hop", C.c_uint32), ("n_prb_slot1", C.c_uint32),
                ("beta_offset_ack_idx_p1", C.c_uint32), ("beta_offset_cqi_idx_p1", C.c_uint32), ("beta_offset_ri_idx_p1", C.c_uint32)]


class PuschResult(C.Structure):
    _fields_ = [("crc_ok", C.c_uint32), ("iterations", C.c_uint32), ("snr_db", C.c_float), ("payload_off", C.c_uint32)]


class UlTimingCfg(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("min_shift", C.c_uint32), ("max_advance", C.c_uint32)]


class PuschTiming(C.Structure):
    _fields_ = [("measured", C.c_uint32), ("tau", C.c_float), ("shift", C.c_int32), ("flags", C.c_uint32), ("residual", C.c_float), ("toa_us", C.c_float),
                ("confidence", C.c_float)]


class UlUeStats(C.Structure):
    _fields_ = [("mod", C.c_uint32), ("active", C.c_uint32), ("success", C.c_uint32), ("mean_snr_db", C.c_float), ("measured", C.c_uint32),
                ("mean_toa_us", C.c_float), ("mean_toa_samples", C.c_float)]


TOA_FLAG_CLAMPED, TOA_FLAG_BELOW = 1, 2


def pusch_toa_decide(tau, N, min_shift=0, max_advance=0):
    """the window decision of k_pusch_toa without a GPU -> (shift, flags); ValueError for what lsn_pusch_toa_decide refuses"""
    cfg, shift, flags = UlTimingCfg(0, min_shift, max_advance), C.c_int32(0), C.c_uint32(0)
    if lib().lsn_pusch_toa_decide(C.c_float(tau), N, C.byref(cfg), C.byref(shift), C.byref(flags)) != LSN_SUCCESS:
        raise ValueError("lsn_pusch_toa_decide refused N = %r, min_shift = %r, max_advance = %r" % (N, min_shift, max_advance))
    return shift.value, flags.value


SINK_T = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(PduCtx), C.POINTER(C.c_uint8), C.c_uint32)

_lib = None


def build(verbose=False):
    """Compile the HIP kernels + host engine for gfx950 (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j8"], stdout=out)
    return LIB_PATH


def _preload_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1.  If this library pulled in
    /opt/rocm's copies first and torch were imported afterwards, the process would hold two HIP/HSA runtimes and device
    discovery fails.  When torch is installed, bind to its copy (one runtime per process, whichever is imported first)."""
    import importlib.util
    try:
        with open("/proc/self/maps") as f:
            if "libamdhip64" in f.read():
                return
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        d = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        for n in ("libhsa-runtime64.so", "libamdhip64.so"):
            p = os.path.join(d, n)
            if os.path.exists(p):
                C.CDLL(p, mode=C.RTLD_GLOBAL)
    except OSError:
        pass


def lib():
    """The C-ABI library. Fails loudly when it has not been built: there is no other implementation to fall back to."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("ltesniffer_amd: %s is missing - run ltesniffer_amd.build() / __graft_entry__.build() "
                               "(the HIP extension is the only implementation; there is no CPU fallback)" % LIB_PATH)
        _preload_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.lsn_phy_create.argtypes = [C.POINTER(PhyCfg), C.POINTER(C.c_void_p)]
        L.lsn_phy_destroy.argtypes = [C.c_void_p]
        L.lsn_phy_create_multi.argtypes = [C.POINTER(PhyCfg), C.POINTER(C.c_int), C.c_uint32, C.POINTER(C.c_void_p)]
        L.lsn_phy_nof_devices.argtypes = [C.c_void_p]
        L.lsn_phy_nof_devices.restype = C.c_uint32
        L.lsn_phy_destroy.restype = None
        L.lsn_phy_set_cell.argtypes = [C.c_void_p, C.POINTER(Cell)]
        L.lsn_phy_get_avail.argtypes = [C.c_void_p, C.c_int]
        L.lsn_phy_get_avail.restype = C.c_void_p
        L.lsn_phy_put_pending.argtypes = [C.c_void_p, C.c_void_p]
        L.lsn_phy_join_pending.argtypes = [C.c_void_p]
        L.lsn_phy_set_pdu_sink.argtypes = [C.c_void_p, SINK_T, C.c_void_p]
        L.lsn_phy_get_stats.argtypes = [C.c_void_p, C.POINTER(BlindStats)]
        L.lsn_phy_get_est_cfo.argtypes = [C.c_void_p]
        L.lsn_phy_get_est_cfo.restype = C.c_float
        L.lsn_phy_set_cfo_correction.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
        L.lsn_phy_set_candidate_pruning.argtypes = [C.c_void_p, C.c_int]
        L.lsn_phy_get_cfo_correction.argtypes = [C.c_void_p]
        L.lsn_phy_get_cfo_correction.restype = C.c_float
        L.lsn_phy_add_evergreen.argtypes = [C.c_void_p, C.c_uint16, C.c_uint16, C.c_uint32]
        L.lsn_phy_add_forbidden.argtypes = [C.c_void_p, C.c_uint16, C.c_uint16, C.c_uint32]
        L.lsn_phy_setup_default_rnti_intervals.argtypes = [C.c_void_p]
        L.lsn_phy_nof_active_rnti.argtypes = [C.c_void_p]
        L.lsn_phy_nof_active_rnti.restype = C.c_uint32
        L.lsn_phy_get_ue_config.argtypes = [C.c_void_p, C.c_uint16, C.POINTER(UeConfig)]
        L.lsn_worker_buffers.argtypes = [C.c_void_p]
        L.lsn_worker_buffers.restype = C.POINTER(C.POINTER(C.c_float))
        L.lsn_worker_buffer_len.argtypes = [C.c_void_p]
        L.lsn_worker_buffer_len.restype = C.c_uint32
        L.lsn_worker_prepare.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(DlSfCfg)]
        L.lsn_worker_sf_idx.argtypes = [C.c_void_p]
        L.lsn_worker_sf_idx.restype = C.c_uint32
        L.lsn_worker_sfn.argtypes = [C.c_void_p]
        L.lsn_worker_sfn.restype = C.c_uint32
        L.lsn_phy_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.lsn_phy_process_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        L.lsn_phy_process_host_int.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32]
        L.lsn_phy_tap.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t]
        L.lsn_phy_tap.restype = C.c_long
        L.lsn_phy_set_stage_c_taps.argtypes = [C.c_void_p, C.c_int]
        L.lsn_phy_get_perf.argtypes = [C.c_void_p, C.POINTER(Perf)]
        L.lsn_kernel_name.argtypes = [C.c_int]
        L.lsn_kernel_name.restype = C.c_char_p
        L.lsn_version.restype = C.c_char_p
        L.lsn_pcap_open.argtypes = [C.c_char_p]
        L.lsn_pcap_open.restype = C.c_void_p
        L.lsn_pcap_open_mem.restype = C.c_void_p
        L.lsn_pcap_set_wall_clock.argtypes = [C.c_void_p, C.c_int]
        L.lsn_pcap_set_wall_clock.restype = None
        L.lsn_pcap_write.argtypes = [C.c_void_p, C.POINTER(PduCtx), C.c_void_p, C.c_uint32]
        L.lsn_pcap_mem.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        L.lsn_pcap_mem.restype = C.c_void_p
        L.lsn_pcap_nof_records.argtypes = [C.c_void_p]
        L.lsn_pcap_nof_records.restype = C.c_uint32
        L.lsn_pcap_reset.argtypes = [C.c_void_p]
        L.lsn_pcap_reset.restype = None
        L.lsn_pcap_close.argtypes = [C.c_void_p]
        L.lsn_pcap_digest.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.lsn_pcap_set_store.argtypes = [C.c_void_p, C.c_int]
        L.lsn_pcap_set_store.restype = None
        L.lsn_pcap_set_digest_blocks.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.lsn_pcap_set_digest_blocks.restype = None
        L.lsn_pcap_block_digests.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.lsn_pcap_block_digests.restype = C.c_uint32
        L.lsn_pcap_close.restype = None
        L.lsn_phy_set_pcap_writer.argtypes = [C.c_void_p, C.c_void_p]
        L.lsn_phy_set_ul_config.argtypes = [C.c_void_p, C.POINTER(UlCfg)]
        L.lsn_phy_tracked_ul_modulation.argtypes = [C.c_void_p, C.c_uint16]
        L.lsn_phy_set_api_mode.argtypes = [C.c_void_p, C.c_int, API_SINK, C.c_void_p, C.c_void_p]
        L.lsn_phy_get_ul_config.argtypes = [C.c_void_p, C.POINTER(UlCfg), C.POINTER(Sib2), C.POINTER(C.c_uint32)]
        L.lsn_sib2_decode.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(Sib2)]
        L.lsn_phy_pusch_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                           C.c_void_p, C.c_size_t]
        L.lsn_phy_tap_ul.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t]
        L.lsn_phy_tap_ul.restype = C.c_long
        L.lsn_phy_set_ul_timing.argtypes = [C.c_void_p, C.POINTER(UlTimingCfg)]
        L.lsn_phy_get_pusch_timing.argtypes = [C.c_void_p, C.POINTER(PuschTiming), C.c_uint32]
        L.lsn_phy_get_pusch_timing.restype = C.c_long
        L.lsn_pusch_toa_decide.argtypes = [C.c_float, C.c_uint32, C.POINTER(UlTimingCfg), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
        L.lsn_phy_get_ul_ue_stats.argtypes = [C.c_void_p, C.c_uint16, C.POINTER(UlUeStats)]
        L.lsn_phy_submit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.lsn_phy_wait.argtypes = [C.c_void_p]
        L.lsn_phy_mib_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Mib)]
        L.lsn_phy_mib_decode_llr.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Mib), C.c_void_p]
        L.lsn_phy_process_file.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(FileCfg), C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
        L.lsn_phy_prepare_file.argtypes = [C.c_void_p, C.c_uint32]
        L.lsn_phy_process_file_rate.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(FileCfg), C.POINTER(FileRate), C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
        L.lsn_resample.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(ResampleCfg), C.c_void_p, C.c_int, C.c_uint64]
        L.lsn_resample_span.argtypes = [C.POINTER(ResampleCfg), C.c_uint64, C.c_uint64, C.POINTER(ResampleSpan)]
        L.lsn_resample_cells.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(ResampleCfg), C.c_uint32, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_uint64)]
        L.lsn_file_cells_span.argtypes = [C.POINTER(FileCfg), C.c_double, C.POINTER(FileCell), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(FileCellsSpan)]
        L.lsn_file_process_cells.argtypes = [C.c_char_p, C.POINTER(FileCfg), C.c_double, C.POINTER(FileCell), C.c_uint32]
        L.lsn_resample_cells_ring.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(ResampleCfg), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.lsn_phy_set_antenna_map.argtypes = [C.c_void_p, C.POINTER(AntennaMap)]
        L.lsn_resample_cells_map.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(ResampleCfg), C.POINTER(AntennaMap), C.c_uint32, C.POINTER(C.c_void_p), C.c_int,
                                             C.POINTER(C.c_uint64)]
        L.lsn_resample_cells_ring_map.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(ResampleCfg), C.POINTER(AntennaMap), C.c_uint32, C.POINTER(C.c_void_p),
                                                  C.POINTER(C.c_uint64)]
        L.lsn_file_cells_span_map.argtypes = [C.POINTER(FileCfg), C.c_double, C.POINTER(FileCell), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint64, C.c_uint32, C.c_uint32,
                                              C.POINTER(FileCellsSpan)]
        L.lsn_stream_span_map.argtypes = [C.POINTER(StreamCfg), C.POINTER(FileCell), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(StreamSpan)]
        L.lsn_stream_open.argtypes = [C.POINTER(StreamCfg), C.POINTER(FileCell), C.c_uint32, C.POINTER(C.c_void_p)]
        L.lsn_stream_push.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.lsn_stream_flush.argtypes = [C.c_void_p]
        L.lsn_stream_status.argtypes = [C.c_void_p, C.POINTER(StreamStatus)]
        L.lsn_stream_close.argtypes = [C.c_void_p]
        L.lsn_stream_span.argtypes = [C.POINTER(StreamCfg), C.POINTER(FileCell), C.c_uint32, C.c_uint64, C.POINTER(StreamSpan)]
        L.lsn_stream_track.argtypes = [C.c_void_p, C.POINTER(StreamTrackCfg)]
        L.lsn_stream_track_status.argtypes = [C.c_void_p, C.POINTER(StreamTrackStatus)]
        L.lsn_stream_track_step.argtypes = [C.POINTER(StreamTrackCfg), C.c_double, C.c_double, C.c_uint32, C.POINTER(StreamTrackState), C.c_double, C.c_int,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.lsn_pss_timing.argtypes = [C.c_int, C.c_int, C.POINTER(PssTimingCell), C.c_uint32]
        L.lsn_pss_timing_error.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.lsn_stream_reacquire.argtypes = [C.c_void_p, C.POINTER(StreamReacquireCfg)]
        L.lsn_stream_reacquire_status.argtypes = [C.c_void_p, C.POINTER(StreamReacquireStatus)]
        L.lsn_phy_mib_decode_side.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Mib), C.c_void_p]
        L.lsn_stream_frame_sync.argtypes = [C.c_void_p, C.POINTER(StreamFrameSyncCfg)]
        L.lsn_stream_frame_sync_status.argtypes = [C.c_void_p, C.POINTER(StreamFrameSyncStatus)]
        L.lsn_frame_sync_decide.argtypes = [C.POINTER(Mib), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]
        L.lsn_pss_acquire.argtypes = [C.c_int, C.c_int, C.POINTER(PssAcquireCell), C.c_uint32]
        L.lsn_pss_acquire_decide.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                             C.POINTER(C.c_double)]
        L.lsn_phy_set_prach_config.argtypes = [C.c_void_p, C.POINTER(PrachCfg)]
        L.lsn_phy_prach_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(PrachDet), C.c_uint32]
        L.lsn_phy_set_prach_sink.argtypes = [C.c_void_p, PRACH_SINK, C.c_void_p]
        L.lsn_phy_set_prach_sink.restype = None
        L.lsn_prach_tti_opportunity.argtypes = [C.c_uint32, C.c_uint32]
        L.lsn_phy_set_shortcut_discovery.argtypes = [C.c_void_p, C.c_int]
        L.lsn_phy_get_shortcut_discovery.argtypes = [C.c_void_p]
        L.lsn_phy_set_histogram_threshold.argtypes = [C.c_void_p, C.c_uint32]
        L.lsn_phy_print_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.lsn_phy_set_mcs_update_interval.argtypes = [C.c_void_p, C.c_uint32]
        L.lsn_phy_update_mcs_database.argtypes = [C.c_void_p]
        L.lsn_phy_nof_tracked_rnti.argtypes = [C.c_void_p]
        L.lsn_phy_nof_tracked_rnti.restype = C.c_uint32
        L.lsn_worker_buffers_offset.argtypes = [C.c_void_p]
        L.lsn_worker_buffers_offset.restype = C.POINTER(C.POINTER(C.c_float))
        L.lsn_cell_search.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.POINTER(CellSearchCfg), C.POINTER(CellSearch), C.c_void_p]
        L.lsn_cell_search_rates.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(CellSearchCfg), C.POINTER(CellSearch), C.c_void_p]
        L.lsn_cell_search_ant.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(CellSearchCfg), C.POINTER(CellSearch),
                                          C.POINTER(CellSearchAnt), C.c_void_p]
        L.lsn_phy_set_sampling.argtypes = [C.c_void_p, C.c_int]
        L.lsn_phy_get_sampling.argtypes = [C.c_void_p]
        L.lsn_symbol_sz.argtypes = [C.c_uint32, C.c_int]
        L.lsn_symbol_sz.restype = C.c_uint32
        L.lsn_sampling_freq_hz.argtypes = [C.c_uint32, C.c_int]
        L.lsn_sampling_freq_hz.restype = C.c_uint32
        L.lsn_clock_plan.argtypes = [C.POINTER(ClockCfg), C.c_uint64, C.c_uint32, C.POINTER(Clock), C.POINTER(ClockObs), C.c_uint32]
        L.lsn_clock_fit.argtypes = [C.POINTER(ClockObs), C.c_uint32, C.c_uint32, C.POINTER(Clock)]
        L.lsn_clock_replica.argtypes = [C.POINTER(ClockCfg), C.c_void_p]
        L.lsn_cell_search_all.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(CellSearchAllCfg), C.POINTER(CellFound),
                                          C.POINTER(C.c_uint32), C.c_void_p]
        L.lsn_pss_cancel.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
        L.lsn_sss_accumulate.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
        L.lsn_cell_search_all_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(CellSearchAllPlan)]
        L.lsn_cell_search_all_decide.argtypes = [C.POINTER(CellSearchAllCfg), C.c_uint32, C.c_float, C.c_double, C.c_uint32, C.c_void_p, C.POINTER(CellSearchAllDecision)]
        L.lsn_clock_track.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(ClockCfg), C.POINTER(ClockObs), C.c_uint32, C.c_void_p]
        L.lsn_clock_estimate.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(ClockCfg), C.POINTER(Clock), C.POINTER(ClockObs), C.c_uint32]
        L.lsn_file_clock_estimate.argtypes = [C.c_int, C.c_char_p, C.POINTER(FileCfg), C.POINTER(FileRate), C.c_uint32, C.POINTER(ClockCfg), C.POINTER(Clock)]
        L.lsn_carrier_scan_plan.argtypes = [C.POINTER(CarrierScanCfg), C.POINTER(CarrierScanPlan), C.POINTER(CarrierMetric), C.c_uint32, C.c_void_p]
        L.lsn_carrier_scan_decide.argtypes = [C.POINTER(CarrierScanCfg), C.POINTER(CarrierMetric), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]
        L.lsn_carrier_scan.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(CarrierScanCfg), C.POINTER(Carrier), C.c_uint32, C.POINTER(CarrierMetric)]
        L.lsn_file_carrier_scan.argtypes = [C.c_int, C.c_char_p, C.POINTER(FileCfg), C.POINTER(CarrierScanCfg), C.POINTER(Carrier), C.c_uint32, C.POINTER(CarrierMetric)]
        L.lsn_carrier_channel.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(CarrierChannelCfg), C.c_void_p, C.c_int, C.c_uint64]
        L.lsn_carrier_channel_span.argtypes = [C.POINTER(CarrierChannelCfg), C.c_uint64, C.c_uint64, C.POINTER(ResampleSpan)]
        L.lsn_phy_set_channel_filter.argtypes = [C.c_void_p, C.c_double]
        L.lsn_channel_filter_design.argtypes = [C.c_double, C.c_double, C.c_double, C.POINTER(ChannelFilterDesign), C.c_void_p, C.c_uint32]
        L.lsn_channel_filter.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(ChannelFilterCfg), C.c_void_p, C.c_int, C.c_uint64]
        L.lsn_channel_filter_ring.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(ChannelFilterCfg), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.lsn_stream_span_filtered.argtypes = [C.POINTER(StreamCfg), C.POINTER(FileCell), C.c_uint32, C.POINTER(C.c_double), C.c_uint64, C.POINTER(StreamSpan)]
        L.lsn_channel_filter_span.argtypes = [C.POINTER(ChannelFilterCfg), C.c_uint64, C.c_uint64, C.POINTER(ResampleSpan)]
        L.lsn_cells_stopbands.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_uint32, C.c_double, C.POINTER(C.c_double)]
        _lib = L
    return _lib


def _check(rc, what):
    if rc != LSN_SUCCESS:
        raise RuntimeError("%s failed: %d%s" % (what, rc, " (no HIP device: this library has no CPU path)"
                                                if rc == LSN_ERROR_NO_DEVICE else ""))


def _check_n(rc, what):
    if rc < 0:
        _check(rc, what)
    return rc


class PcapWriter:
    """Mirror of LTESniffer_pcap_writer (PcapWriter.h:39-51) on the native writer; path=None -> in-memory capture."""

    def __init__(self, path=None, wall_clock=None):
        L = lib()
        self._h = L.lsn_pcap_open(path.encode()) if path else L.lsn_pcap_open_mem()
        if not self._h:
            raise RuntimeError("cannot open pcap %r" % path)
        if wall_clock is not None:
            L.lsn_pcap_set_wall_clock(self._h, int(wall_clock))

    def write(self, ctx, pdu):
        c = PduCtx(ctx["tti"], ctx["rnti"], ctx["direction"], ctx["rnti_type"], ctx.get("crc_ok", 1), 0, ctx.get("tb", 0), 0)
        _check(lib().lsn_pcap_write(self._h, C.byref(c), pdu, len(pdu)), "pcap_write")

    def bytes(self):
        n = C.c_size_t()
        p = lib().lsn_pcap_mem(self._h, C.byref(n))
        return C.string_at(p, n.value)

    def nof_records(self):
        return lib().lsn_pcap_nof_records(self._h)

    def digest(self):
        """(64-bit digest, bytes) of the record stream since open / reset, timestamps excluded"""
        d, n = C.c_uint64(), C.c_uint64()
        _check(lib().lsn_pcap_digest(self._h, C.byref(d), C.byref(n)), "pcap_digest")
        return int(d.value), int(n.value)

    def set_store(self, on):
        lib().lsn_pcap_set_store(self._h, int(bool(on)))

    def set_digest_blocks(self, subframes_per_block, origin_tti=0):
        """cut the digest every n subframes counted from origin_tti (0 = off); clears the blocks collected so far"""
        lib().lsn_pcap_set_digest_blocks(self._h, int(subframes_per_block), int(origin_tti) % 10240)

    def block_digests(self):
        """-> [(digest, nof_records)] per block of the stream since reset / set_digest_blocks"""
        n = lib().lsn_pcap_block_digests(self._h, None, None, 0)
        d, c = (C.c_uint64 * max(1, n))(), (C.c_uint32 * max(1, n))()
        n = min(n, lib().lsn_pcap_block_digests(self._h, d, c, n))
        return [(int(d[i]), int(c[i])) for i in range(n)]

    def reset(self):
        lib().lsn_pcap_reset(self._h)

    def close(self):
        if self._h:
            lib().lsn_pcap_close(self._h)
            self._h = None


class SubframeWorker:
    """Mirror of SubframeWorker (SubframeWorker.h:16-86): buffers to fill + prepare(); work() runs inside Phy."""

    def __init__(self, phy, handle):
        self._phy, self._h = phy, handle

    def getBuffers(self):
        """-> list of numpy complex64 views (one per rx antenna, 3 * SF_LEN samples) of the pinned IQ buffers"""
        L = lib()
        n = L.lsn_worker_buffer_len(self._h)
        bufs = L.lsn_worker_buffers(self._h)
        out = []
        for rx in range(self._phy.nof_rx_antennas):
            a = np.ctypeslib.as_array(bufs[rx], shape=(2 * n,))
            out.append(a.view(np.complex64))
        return out

    def prepare(self, sf_idx, sfn, updateMetaFormats, dl_sf_cfg=None):
        cfg = dl_sf_cfg if dl_sf_cfg is not None else DlSfCfg(sfn * 10 + sf_idx, 0, 0)
        _check(lib().lsn_worker_prepare(self._h, sf_idx, sfn, int(bool(updateMetaFormats)), C.byref(cfg)), "prepare")

    def getSfidx(self):
        return lib().lsn_worker_sf_idx(self._h)

    def getSfn(self):
        return lib().lsn_worker_sfn(self._h)


class Phy:
    """Mirror of Phy (Phy.h:22-66). Constructor arguments keep the reference's names; the pcap writer argument is
    replaced by a PDU sink callable ``sink(ctx_dict, pdu_bytes)`` receiving what pack_and_write would serialise."""

    def __init__(self, nof_rx_antennas=2, nof_workers=20, skipSecondaryMetaFormats=False, metaFormatSplitRatio=0.99,
                 histogramThreshold=5, sink=None, mcs_tracking_mode=1, harq_mode=0, device=0, max_batch=64,
                 max_turbo_iterations=12, default_rnti_intervals=True, pcapwriter=None, sniffer_mode=0, devices=None):
        """devices: list of HIP devices that share ONE capture (lsn_phy_create_multi); None: the single `device`"""
        self.nof_rx_antennas = nof_rx_antennas
        self._cfg = PhyCfg(nof_rx_antennas, nof_workers, max_batch, int(skipSecondaryMetaFormats), metaFormatSplitRatio,
                           histogramThreshold, mcs_tracking_mode, harq_mode, devices[0] if devices else device, max_turbo_iterations, sniffer_mode)
        self._h = C.c_void_p()
        if devices:
            arr = (C.c_int * len(devices))(*devices)
            _check(lib().lsn_phy_create_multi(C.byref(self._cfg), arr, len(devices), C.byref(self._h)), "lsn_phy_create_multi")
        else:
            _check(lib().lsn_phy_create(C.byref(self._cfg), C.byref(self._h)), "lsn_phy_create")
        self.pdus = []
        self._user_sink = sink
        self._cb = SINK_T(self._on_pdu)
        self.pcapwriter = pcapwriter
        if pcapwriter is not None:  # native consumer, like the reference's LTESniffer_pcap_writer* ctor argument
            _check(lib().lsn_phy_set_pcap_writer(self._h, pcapwriter._h), "set_pcap_writer")
        else:
            _check(lib().lsn_phy_set_pdu_sink(self._h, self._cb, None), "set_pdu_sink")
        if default_rnti_intervals:
            _check(lib().lsn_phy_setup_default_rnti_intervals(self._h), "rnti intervals")
        self.cell = None

    def _on_pdu(self, user, ctx, pdu, n):
        c = ctx.contents
        d = dict(tti=c.tti, rnti=c.rnti, direction=c.direction, rnti_type=c.rnti_type, crc_ok=c.crc_ok, tb=c.tb)
        data = C.string_at(pdu, n)
        if self._user_sink is not None:
            self._user_sink(d, data)
        else:
            self.pdus.append((d, data))

    def set_sampling(self, rates):
        """sampling mode of the IQ this Phy is handed: RATES_3GPP (default) or RATES_SRSRAN (384 / 768 / 1024 / 1536 samples per symbol at 25 / 50 / 75 / 100 PRB,
        what the reference records); call it in front of setCell.  False: refused (unknown mode, or another mode than the one the cell was set with)"""
        return lib().lsn_phy_set_sampling(self._h, int(rates)) == LSN_SUCCESS

    def get_sampling(self):
        return int(lib().lsn_phy_get_sampling(self._h))

    def set_channel_filter(self, stopband_hz):
        """lsn_phy_set_channel_filter: this Phy's file replays (process_file, process_file_rate, process_file_cells) and the Streams opened on it from then on run a
        sharp channel filter at the recording's rate in front of the resampler - everything from stopband_hz on, relative to the cell's carrier, is 80 dB down (a
        neighbour carrier: the distance to its nearest occupied edge, cells_stopbands).  0: off (the default).  Sticky; checked against rate and bandwidth when a
        replay starts or a Stream opens; an open Stream stays as it was opened.  False: refused (negative or not finite)"""
        return lib().lsn_phy_set_channel_filter(self._h, float(stopband_hz)) == LSN_SUCCESS

    def set_antenna_map(self, src=None, offset_hz=None):
        """lsn_phy_set_antenna_map: in this Phy's process_file_rate / process_file_cells replays and in Streams opened on it from then on, antenna a of
        the Phy is cut from antenna src[a] of the recording at the cell's center_offset_hz + offset_hz[a]; the recording may then have any 1 .. 8 antennas
        (nof_antennas of the call).  UL_MODE from one wideband channel: set_antenna_map(src=(0, 0), offset_hz=(0.0, -duplex_spacing)).  set_antenna_map(None): off (the
        default).  Sticky, like set_channel_filter - and refused together with it when a replay starts.  False: refused (len(src) is not the Phy's antenna count, a
        source above 7, an offset that is not finite)"""
        if src is None:
            return lib().lsn_phy_set_antenna_map(self._h, None) == LSN_SUCCESS
        return lib().lsn_phy_set_antenna_map(self._h, C.byref(antenna_map(src, offset_hz))) == LSN_SUCCESS

    def setCell(self, nof_prb, nof_ports, cell_id, phich_resources=0, cp=0):
        """cp: srsran_cell_t.cp - 0 normal, 1 extended cyclic prefix (downlink path)"""
        self.cell = Cell(nof_prb, nof_ports, cell_id, cp, 0, phich_resources, 0)
        rc = lib().lsn_phy_set_cell(self._h, C.byref(self.cell))
        return rc == LSN_SUCCESS

    def getAvail(self):
        h = lib().lsn_phy_get_avail(self._h, 1)
        return SubframeWorker(self, h) if h else None

    def getAvailImmediate(self):
        h = lib().lsn_phy_get_avail(self._h, 0)
        return SubframeWorker(self, h) if h else None

    def putPending(self, worker):
        _check(lib().lsn_phy_put_pending(self._h, worker._h), "putPending")

    def joinPending(self):
        _check(lib().lsn_phy_join_pending(self._h), "joinPending")

    # ---- the calls LTESniffer_Core makes on PhyCommon / RNTIManager / MCSTracking (LTESniffer_Core.cc:87,473-499,561,616-620) ----
    def setShortcutDiscovery(self, enable):
        _check(lib().lsn_phy_set_shortcut_discovery(self._h, int(bool(enable))), "setShortcutDiscovery")

    def getShortcutDiscovery(self):
        return bool(lib().lsn_phy_get_shortcut_discovery(self._h))

    def setHistogramThreshold(self, threshold):
        _check(lib().lsn_phy_set_histogram_threshold(self._h, int(threshold)), "setHistogramThreshold")

    def printStats(self):
        """PhyCommon::printStats: the two CSV lines, returned as text (written through a FILE* by the library)"""
        import tempfile
        libc = C.CDLL(None)
        libc.fopen.restype = C.c_void_p
        libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        libc.fclose.argtypes = [C.c_void_p]
        with tempfile.NamedTemporaryFile() as t:
            f = libc.fopen(t.name.encode(), b"w")
            _check(lib().lsn_phy_print_stats(self._h, C.c_void_p(f)), "printStats")
            libc.fclose(f)
            return open(t.name).read()

    def setMcsUpdateInterval(self, seconds):
        _check(lib().lsn_phy_set_mcs_update_interval(self._h, int(seconds)), "setMcsUpdateInterval")

    def updateMcsDatabase(self):
        _check(lib().lsn_phy_update_mcs_database(self._h), "updateMcsDatabase")

    def nofTrackedRnti(self):
        return int(lib().lsn_phy_nof_tracked_rnti(self._h))

    # ---- offline / file-replay path ----
    def process_host(self, iq, start_tti, update_meta_period=0):
        """iq: complex64 [n_subframes, nof_rx, 15*N]"""
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        _check(lib().lsn_phy_process_host(self._h, iq.ctypes.data, iq.shape[0], start_tti, update_meta_period), "process_host")

    def process_host_int(self, q, start_tti, update_meta_period=0, sample_scale=0.0):
        """q: int16 or int8 [n_subframes, nof_rx, 15*N, 2] (I, Q); one LSB = sample_scale (0: full scale +-1) - lsn_phy_process_host_int"""
        assert q.dtype in (np.int16, np.int8) and q.ndim == 4 and q.shape[3] == 2
        q = np.ascontiguousarray(q)
        _check(lib().lsn_phy_process_host_int(self._h, q.ctypes.data, FILE_SC16 if q.dtype == np.int16 else FILE_SC8, float(sample_scale), q.shape[0], start_tti,
                                              update_meta_period), "process_host_int")

    def process_device(self, dev_ptr, n_subframes, start_tti, update_meta_period=0, stream=None):
        _check(lib().lsn_phy_process_device(self._h, C.c_void_p(dev_ptr), n_subframes, start_tti, update_meta_period,
                                            C.c_void_p(stream or 0)), "process_device")

    def submit_device(self, d_ptr, n_subframes, start_tti, update_meta_period=0, stream=None):
        """pipelined process_device: returns once the block is searched and queued; call wait() before reusing the buffer / reading results"""
        _check(lib().lsn_phy_submit_device(self._h, C.c_void_p(d_ptr), n_subframes, start_tti, update_meta_period, C.c_void_p(stream or 0)), "submit_device")

    def wait(self):
        _check(lib().lsn_phy_wait(self._h), "wait")

    def mib_decode(self, iq, with_llr=False):
        """srsran_ue_mib_decode on ONE subframe iq[nof_rx, 15*N] -> dict (found, sfn, sfn_offset, nof_prb, nof_ports, ...) [, raw PBCH soft bits]"""
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        m = Mib()
        llr = np.zeros(480, dtype=np.float32)
        r = lib().lsn_phy_mib_decode_llr(self._h, iq.ctypes.data, 0, C.byref(m), llr.ctypes.data)
        if r < 0:
            _check(r, "mib_decode")
        d = {n: int(getattr(m, n)) for n, _ in Mib._fields_}
        return (d, llr) if with_llr else d

    def mib_decode_side(self, iq, with_llr=False):
        """lsn_phy_mib_decode_side: mib_decode on the Phy's side scratch and a stream of its own - the same dict and soft bits -, allowed while submitted blocks
        are in flight"""
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        m = Mib()
        llr = np.zeros(480, dtype=np.float32)
        r = lib().lsn_phy_mib_decode_side(self._h, iq.ctypes.data, 0, C.byref(m), llr.ctypes.data if with_llr else None)
        if r < 0:
            _check(r, "mib_decode_side")
        d = {n: int(getattr(m, n)) for n, _ in Mib._fields_}
        return (d, llr) if with_llr else d

    def prepare_file(self):
        """reserve the file source's block buffers ahead of the first replay (lsn_phy_prepare_file)"""
        _check(lib().lsn_phy_prepare_file(self._h, self.nof_rx_antennas), "prepare_file")

    def process_file(self, path, start_tti=0, offset_time=0, offset_freq=0.0, max_subframes=0, update_meta_period=0, sample_format=FILE_CF32, sample_scale=0.0,
                     sample_rate=None, offset_time_frac=0.0, center_offset_hz=0.0, nof_antennas=None):
        """file mode of the reference (-i file -O offset_time -o offset_freq): replay a cf32 capture (antennas interleaved per sample);
        sample_format FILE_SC16 / FILE_SC8: integer I/Q pairs, one LSB = sample_scale (0: full scale +-1); returns the number of subframes processed.
        sample_rate (Hz): the file was recorded at this rate and goes through the GPU resampler (lsn_phy_process_file_rate); offset_time and
        offset_time_frac then count samples of the FILE's rate.  center_offset_hz: see process_file_rate.  nof_antennas: the recording's, when an antenna map
        (set_antenna_map) is set; None: the Phy's"""
        if center_offset_hz != 0.0 and sample_rate is None:
            raise ValueError("center_offset_hz needs sample_rate (the rate of the recording): the translation is part of the resampler")
        fc = FileCfg(self.nof_rx_antennas if nof_antennas is None else int(nof_antennas), int(offset_time), float(offset_freq), int(sample_format), float(sample_scale))
        done = C.c_uint64(0)
        if sample_rate is not None:
            fr = FileRate(C.sizeof(FileRate), 0, float(sample_rate), float(offset_time_frac), float(center_offset_hz))
            _check(lib().lsn_phy_process_file_rate(self._h, os.fsencode(path), C.byref(fc), C.byref(fr), start_tti if start_tti == TTI_FROM_MIB else start_tti % 10240,
                                                   max_subframes, update_meta_period, C.byref(done)), "process_file_rate")
            return int(done.value)
        _check(lib().lsn_phy_process_file(self._h, os.fsencode(path), C.byref(fc), start_tti if start_tti == TTI_FROM_MIB else start_tti % 10240, max_subframes, update_meta_period, C.byref(done)),
               "process_file")
        return int(done.value)

    def process_file_rate(self, path, sample_rate, center_offset_hz=0.0, **kw):
        """lsn_phy_process_file_rate: replay a recording made at sample_rate (Hz) whose wanted cell sits center_offset_hz off the recording's centre (an
        offset-tuned capture, or one carrier of a wideband capture; may be negative).  The input samples are translated by -center_offset_hz in front of the
        resampler's filter, with an integer phase that is a function of the sample's index in the recording.  Accepted when |center_offset_hz| + the cell's
        occupied half-band <= sample_rate / 2.  Two Phys replay two cells of one file.  Other arguments: process_file"""
        return self.process_file(path, sample_rate=sample_rate, center_offset_hz=center_offset_hz, **kw)

    # ---- uplink ----
    def setUlConfig(self, cyclic_shift, delta_ss, hopping_offset=0, group_hopping=0, sequence_hopping=0):
        u = UlCfg(cyclic_shift, delta_ss, hopping_offset, int(group_hopping), int(sequence_hopping))
        return lib().lsn_phy_set_ul_config(self._h, C.byref(u)) == LSN_SUCCESS

    def setApiMode(self, api_mode, api_pcapwriter=None):
        """-a of the reference: identities found in decoded downlink blocks are collected in self.api_events as
        (tti, rnti, id_type, msg_type, value); blocks that carried one also go to api_pcapwriter"""
        self.api_events = []
        self._api_pcap = api_pcapwriter

        def _cb(user, ev):
            e = ev.contents
            self.api_events.append((int(e.tti), int(e.rnti), int(e.id_type), int(e.msg_type), e.value.decode()))
        self._api_cb = API_SINK(_cb)
        return lib().lsn_phy_set_api_mode(self._h, int(api_mode), self._api_cb, None, api_pcapwriter._h if api_pcapwriter else None) == LSN_SUCCESS

    def trackedUlModulation(self, rnti):
        return int(lib().lsn_phy_tracked_ul_modulation(self._h, rnti))

    def getUlConfig(self):
        """None until an uplink configuration is in use, else dict(cyclic_shift, delta_ss, hopping_offset, from_sib2, sib2 = dict or None)"""
        u, s, f = UlCfg(), Sib2(), C.c_uint32(0)
        if lib().lsn_phy_get_ul_config(self._h, C.byref(u), C.byref(s), C.byref(f)) != 1:
            return None
        return dict(cyclic_shift=u.cyclic_shift, delta_ss=u.delta_ss, hopping_offset=u.hopping_offset, group_hopping=u.group_hopping_enabled,
                    sequence_hopping=u.sequence_hopping_enabled, from_sib2=bool(f.value),
                    sib2=s.as_dict() if f.value else None)

    def pusch_decode(self, ul_iq, start_tti, grants):
        """ul_iq: complex64 [n_subframes, 15*N]; grants: list of dict(sf, rnti, n_dmrs, n_prb, L_prb, mod, tbs, rv)
        -> list of dict(crc_ok, iterations, snr_db, payload)"""
        ul_iq = np.ascontiguousarray(ul_iq, dtype=np.complex64)
        n = len(grants)
        arr = (PuschGrant * max(1, n))(*[PuschGrant(g["sf"], g["rnti"], g.get("n_dmrs", 0), g["n_prb"], g["L_prb"], g["mod"], g["tbs"], g.get("rv", 0),
                                                    g.get("nof_ack", 0), g.get("cqi_bits", 0), g.get("ri_bits", 0), g.get("hop", 0), g.get("n_prb2", 0),
                                                    g.get("i_ack_p1", 0), g.get("i_cqi_p1", 0), g.get("i_ri_p1", 0))
                                         for g in grants])
        res = (PuschResult * max(1, n))()
        cap = sum(g["tbs"] // 8 for g in grants) + 64
        pay = np.zeros(cap, dtype=np.uint8)
        _check(lib().lsn_phy_pusch_decode(self._h, ul_iq.ctypes.data, 0, ul_iq.shape[0], start_tti, arr, n, res, pay.ctypes.data, cap), "pusch_decode")
        return [dict(crc_ok=int(res[i].crc_ok), iterations=int(res[i].iterations), snr_db=float(res[i].snr_db),
                     payload=bytes(pay[res[i].payload_off:res[i].payload_off + grants[i]["tbs"] // 8]) if res[i].crc_ok else b"")
                for i in range(n)]

    def setUlTiming(self, mode, min_shift=0, max_advance=0):
        """per-grant uplink arrival time: 0 off (default), 1 measure, 2 measure and re-window; the thresholds in samples (0: N / 128 and N / 4).
        -> the C return code (LSN_SUCCESS when accepted)"""
        t = UlTimingCfg(mode, min_shift, max_advance)
        return lib().lsn_phy_set_ul_timing(self._h, C.byref(t))

    def pusch_timing(self):
        """per grant of the last pusch_decode: list of dict(measured, tau, shift, flags, residual, toa_us, confidence)"""
        n = lib().lsn_phy_get_pusch_timing(self._h, None, 0)
        if n < 0:
            raise RuntimeError("get_pusch_timing failed: %d" % n)
        arr = (PuschTiming * max(1, n))()
        lib().lsn_phy_get_pusch_timing(self._h, arr, n)
        return [dict(measured=int(a.measured), tau=float(a.tau), shift=int(a.shift), flags=int(a.flags), residual=float(a.residual), toa_us=float(a.toa_us),
                     confidence=float(a.confidence)) for a in arr[:n]]

    def ul_ue_stats(self, rnti):
        """UL_MODE: the reference's uplink table row of one RNTI -> dict, or None without an entry; RuntimeError outside UL_MODE"""
        s = UlUeStats()
        r = lib().lsn_phy_get_ul_ue_stats(self._h, rnti, C.byref(s))
        if r < 0:
            raise RuntimeError("get_ul_ue_stats failed: %d" % r)
        return dict(mod=int(s.mod), active=int(s.active), success=int(s.success), mean_snr_db=float(s.mean_snr_db), measured=int(s.measured),
                    mean_toa_us=float(s.mean_toa_us), mean_toa_samples=float(s.mean_toa_samples)) if r == 1 else None

    def tap_ul_priv_grid(self, grant_index):
        """mode 2 of setUlTiming: the private grid rows of grant `grant_index` of the last pusch_decode -> complex64 [14 or 12, 12 nof_prb]"""
        nre = 12 * self.cell.nof_prb
        buf = np.zeros(14 * nre, dtype=np.complex64)
        nb = lib().lsn_phy_tap_ul(self._h, 5, grant_index, buf.ctypes.data, buf.nbytes)
        if nb < 0:
            raise RuntimeError("tap_ul failed: %d" % nb)
        return buf[: nb // 8].reshape(-1, nre)

    def tap_ul_grid(self, sf):
        nre = 12 * self.cell.nof_prb
        buf = np.zeros(14 * nre, dtype=np.complex64)
        nb = lib().lsn_phy_tap_ul(self._h, 0, sf, buf.ctypes.data, buf.nbytes)
        if nb < 0:
            raise RuntimeError("tap_ul failed: %d" % nb)
        return buf.reshape(14, nre)

    def tap_ul_llr(self, grant_index, count):
        buf = np.zeros(count, dtype=np.int16)
        nb = lib().lsn_phy_tap_ul(self._h, 1, grant_index, buf.ctypes.data, buf.nbytes)
        if nb < 0:
            raise RuntimeError("tap_ul failed: %d" % nb)
        return buf[: nb // 2]

    def tap_ul_cbs(self, grant_index):
        """code blocks of grant `grant_index` of the last pusch_decode call in transport-block order: list of dict(K, F, E, rv, ok, iters,
        d3=int16[3, K + 4] (what k_rm wrote for k_turbo, unpacked as in stage_c_jobs)); raises for a grant that was not decoded"""
        rec = np.zeros(6 * 32, dtype=np.uint32)   # a transport block has at most 32 code blocks
        nb = lib().lsn_phy_tap_ul(self._h, 3, grant_index, rec.ctypes.data, rec.nbytes)
        if nb < 0:
            raise RuntimeError("tap_ul failed: %d" % nb)
        rec = rec[: nb // 4].reshape(-1, 6)
        words = np.zeros(int(sum(int(c[0]) + 12 for c in rec)), dtype=np.uint32)
        nw = lib().lsn_phy_tap_ul(self._h, 4, grant_index, words.ctypes.data, words.nbytes)
        if nw != words.nbytes:
            raise RuntimeError("tap_ul failed: %d" % nw)
        out, o = [], 0
        for K, F, E, rv, ok, iters in rec.tolist():
            out.append(dict(K=K, F=F, E=E, rv=rv, ok=ok, iters=iters, d3=unpack_rm_words(words[o:o + K + 12], K)))
            o += K + 12
        return out

    # ---- PRACH ----
    def setPrachConfig(self, config_idx, root_seq_idx, zero_corr_zone, freq_offset, hs_flag=0, detect_factor=0.0, zc_roots=None):
        """PUSCH_Decoder::set_rach_config; zc_roots: 838 uint16 (36.211 Table 5.7.2-4) or None"""
        zc = np.ascontiguousarray(zc_roots, dtype=np.uint16) if zc_roots is not None else None
        p = PrachCfg(config_idx, root_seq_idx, zero_corr_zone, freq_offset, hs_flag, detect_factor,
                     zc.ctypes.data_as(C.POINTER(C.c_uint16)) if zc is not None else None)
        nwin = 839 // PRACH_NCS[zero_corr_zone] if 0 < zero_corr_zone < 16 else 1
        self._prach_nroots = (64 + nwin - 1) // nwin
        return lib().lsn_phy_set_prach_config(self._h, C.byref(p)) == LSN_SUCCESS

    def prach_detect(self, ul_iq, start_tti, cap=256):
        """PUSCH_Decoder::work_prach over ul_iq complex64 [n_subframes, 15*N] -> list of dict(sf, preamble, offset, offset_sec, p2avg)"""
        ul_iq = np.ascontiguousarray(ul_iq, dtype=np.complex64)
        det = (PrachDet * cap)()
        n = _check_n(lib().lsn_phy_prach_detect(self._h, ul_iq.ctypes.data, 0, ul_iq.shape[0], start_tti, det, cap), "prach_detect")
        return [dict(sf=int(d.sf), preamble=int(d.preamble), offset=int(d.offset), offset_sec=float(d.offset_sec), p2avg=float(d.p2avg)) for d in det[:n]]

    def set_prach_sink(self, fn):
        """fn(tti, [dict(...)]) for every PRACH occasion with detections while UL_MODE batches are processed"""
        def tramp(_user, tti, det, n):
            fn(int(tti), [dict(sf=int(det[i].sf), preamble=int(det[i].preamble), offset=int(det[i].offset), offset_sec=float(det[i].offset_sec),
                               p2avg=float(det[i].p2avg)) for i in range(n)])
        self._prach_cb = PRACH_SINK(tramp) if fn else PRACH_SINK()
        lib().lsn_phy_set_prach_sink(self._h, self._prach_cb, None)

    def tap_prach_corr(self, occasion):
        buf = np.zeros(self._prach_nroots * 839, dtype=np.float32)
        nb = lib().lsn_phy_tap_ul(self._h, 2, occasion, buf.ctypes.data, buf.nbytes)
        if nb < 0:
            raise RuntimeError("tap_ul failed: %d" % nb)
        return buf.reshape(self._prach_nroots, 839)

    # ---- taps / stats ----
    def tap(self, what, sf, dtype, count):
        buf = np.zeros(count, dtype=dtype)
        n = lib().lsn_phy_tap(self._h, what, sf, buf.ctypes.data, buf.nbytes)
        if n < 0:
            raise RuntimeError("tap %d failed: %d" % (what, n))
        return buf[: n // buf.itemsize]

    def set_stage_c_taps(self, on=True):
        """keep the soft bits / de-rate-matched words / per-code-block verdicts of every decode job of the batches processed from now on"""
        _check(lib().lsn_phy_set_stage_c_taps(self._h, 1 if on else 0), "set_stage_c_taps")

    def stage_c_jobs(self):
        """decode jobs of the LAST chunk: list of dict(sf, tti, rnti, nof_re, qm, tbs, crc, p_a_db, llr=[cw0, cw1] int16, cbs=[dict(tb, K, F, E, rv, ok, iters, skipped,
        d3=int16[3, K + 4] (the de-rate-matched streams unpacked from the kernel's transposed 10-bit words))])"""
        jt = np.dtype([("sf", "<u4"), ("tti", "<u4"), ("rnti", "<u4"), ("nof_re", "<u4"), ("qm", "<u4", 2), ("llr_len", "<u4", 2), ("tbs", "<u4", 2), ("crc", "<u4", 2),
                       ("ncb", "<u4"), ("have", "<u4"), ("done", "<u4"), ("p_a_db", "<f4")])
        ct = np.dtype([("tb", "<u4"), ("K", "<u4"), ("F", "<u4"), ("E", "<u4"), ("rv", "<u4"), ("ok", "<u4"), ("iters", "<u4"), ("skipped", "<u4")])
        hdr = self.tap(TAP_PDSCH_JOBS, 0, np.uint8, 1 << 22).view(jt)
        out = []
        for j, h in enumerate(hdr):
            d = dict(job=j, sf=int(h["sf"]), tti=int(h["tti"]), rnti=int(h["rnti"]), nof_re=int(h["nof_re"]), qm=[int(x) for x in h["qm"]], tbs=[int(x) for x in h["tbs"]],
                     crc=[int(x) for x in h["crc"]], p_a_db=float(h["p_a_db"]), have=bool(h["have"]), done=bool(h["done"]), llr=[None, None], cbs=[])
            if h["have"]:
                n0, n1 = int(h["llr_len"][0]), int(h["llr_len"][1])
                llr = self.tap(TAP_PDSCH_LLR16, j, np.int16, n0 + n1 + 8)
                d["llr"] = [llr[:n0].copy(), llr[n0:n0 + n1].copy()]
                cbs = self.tap(TAP_CB_RESULT, j, np.uint8, 64 * ct.itemsize).view(ct)
                words = self.tap(TAP_RM_WORDS, j, np.uint32, int(sum(int(c["K"]) + 12 for c in cbs)) + 8)
                o = 0
                for c in cbs:
                    K = int(c["K"])
                    d3 = unpack_rm_words(words[o:o + K + 12], K)
                    o += K + 12
                    d["cbs"].append(dict(tb=int(c["tb"]), K=K, F=int(c["F"]), E=int(c["E"]), rv=int(c["rv"]), ok=int(c["ok"]), iters=int(c["iters"]), skipped=int(c["skipped"]), d3=d3))
            out.append(d)
        return out

    def perf(self):
        p = Perf()
        _check(lib().lsn_phy_get_perf(self._h, C.byref(p)), "get_perf")
        return p

    def getStats(self):
        s = BlindStats()
        _check(lib().lsn_phy_get_stats(self._h, C.byref(s)), "get_stats")
        return s

    def est_cfo(self):
        return lib().lsn_phy_get_est_cfo(self._h)

    CFO_OFF, CFO_FIXED, CFO_TRACK = 0, 1, 2

    def setCfoCorrection(self, mode, cfo_hz=0.0, alpha=0.25):
        """CFO correction inside the OFDM kernel - what srsran_ue_sync's tracking does ahead of the reference's workers (LTESniffer_Core.cc:312-316,344).
        CFO_FIXED removes cfo_hz; CFO_TRACK starts there and follows the CRS estimate chunk by chunk (include/ltesniffer_amd.h)"""
        _check(lib().lsn_phy_set_cfo_correction(self._h, int(mode), float(cfo_hz), float(alpha)), "setCfoCorrection")

    PRUNE_OFF, PRUNE_ON, PRUNE_TEST = 0, 1, 2

    def setCandidatePruning(self, mode):
        """which slots of the candidate table the blind decoder computes ahead of the search (lsn_phy_set_candidate_pruning): PRUNE_OFF = all, PRUNE_ON (default) =
        not those under a location the search is predicted to accept (decoded on demand if it comes there after all), PRUNE_TEST = the prediction claims everything"""
        _check(lib().lsn_phy_set_candidate_pruning(self._h, int(mode)), "setCandidatePruning")

    def getCfoCorrection(self):
        return lib().lsn_phy_get_cfo_correction(self._h)

    def nof_active_rnti(self):
        return lib().lsn_phy_nof_active_rnti(self._h)

    def ue_config(self, rnti):
        """MCSTracking::get_ue_config_rnti: what RRCConnectionSetup messages taught about this RNTI (or the default)"""
        c = UeConfig()
        _check(lib().lsn_phy_get_ue_config(self._h, rnti, C.byref(c)), "get_ue_config")
        return c

    def close(self):
        if self._h:
            st = getattr(self, "_stream", None)     # a Stream this Phy is a cell of is closed first: its launches write this Phy's buffers
            st = st() if st is not None else None
            if st is not None:
                try:
                    st.close()
                except (RuntimeError, ValueError):
                    pass
            lib().lsn_phy_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cell_search(iq, nof_prb, nof_periods=2, force_n_id_2=-1, threshold=20.0, device=0, with_corr=False, rates=RATES_3GPP):
    """rf_search_and_decode_mib of the reference (LTESniffer_Core.cc:195-204) on a block of samples of one antenna:
    -> (rc, CellSearch[, corr[3, 75 N]]); rc 1 found / 0 not found; iq: numpy complex64 (host) or a torch cuda tensor;
    rates: sampling mode of iq (RATES_SRSRAN: pss_pos / sf_start count samples of that rate)"""
    import numpy as np
    N = symbol_sz(nof_prb, rates) or 128
    cfg = CellSearchCfg(nof_periods, force_n_id_2, threshold)
    out = CellSearch()
    corr = np.zeros((3, 75 * N), dtype=np.float32) if with_corr else None
    if hasattr(iq, "data_ptr"):
        ptr, n, on_dev = iq.data_ptr(), iq.numel(), 1
    else:
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        ptr, n, on_dev = iq.ctypes.data, iq.size, 0
    rc = _check_n(lib().lsn_cell_search_rates(device, ptr, on_dev, n, nof_prb, int(rates), C.byref(cfg), C.byref(out), corr.ctypes.data if with_corr else None), "lsn_cell_search")
    return (rc, out, corr) if with_corr else (rc, out)


SEARCH_MAX_ANTENNAS = 2


def cell_search_ant(iq, nof_prb, nof_periods=2, force_n_id_2=-1, threshold=20.0, device=0, with_corr=False, rates=RATES_3GPP):
    """lsn_cell_search_ant: cell_search over all receive antennas of a recording, combined without their phases.  iq: [antenna][sample] numpy
    complex64 or a torch cuda tensor; a view whose rows lie further apart than their length (a window into a wider buffer) is read in place
    -> (rc, CellSearch, [CellSearchAnt per antenna: pss_peak, sss_metric, sss_second, cfo_hz, n_id_1, occurrence][, corr[3, 75 N]])"""
    import numpy as np
    N = symbol_sz(nof_prb, rates) or 128
    cfg = CellSearchCfg(nof_periods, force_n_id_2, threshold)
    out = CellSearch()
    corr = np.zeros((3, 75 * N), dtype=np.float32) if with_corr else None
    if hasattr(iq, "data_ptr"):
        if iq.dim() != 2 or iq.stride(1) != 1:
            raise ValueError("cell_search_ant: a [antenna][sample] tensor with contiguous rows")
        ptr, nant, n, stride, on_dev = iq.data_ptr(), iq.shape[0], iq.shape[1], (iq.stride(0) if iq.shape[0] > 1 else iq.shape[1]), 1
    else:
        iq = np.asarray(iq)
        if iq.ndim != 2:
            raise ValueError("cell_search_ant: iq is [antenna][sample]")
        if iq.dtype != np.complex64 or iq.shape[1] == 0 or iq.strides[1] != 8 or iq.strides[0] % 8 or iq.strides[0] < 8 * iq.shape[1]:
            iq = np.ascontiguousarray(iq, dtype=np.complex64)
        ptr, nant, n, stride, on_dev = iq.ctypes.data, iq.shape[0], iq.shape[1], (iq.strides[0] // 8 if iq.shape[0] > 1 else iq.shape[1]), 0
    per = (CellSearchAnt * max(nant, 1))()
    rc = _check_n(lib().lsn_cell_search_ant(device, ptr, on_dev, n, stride, nant, nof_prb, int(rates), C.byref(cfg), C.byref(out), per,
                                            corr.ctypes.data if with_corr else None), "lsn_cell_search_ant")
    per = [CellSearchAnt.from_buffer_copy(p) for p in per[:nant]]
    return (rc, out, per, corr) if with_corr else (rc, out, per)


def cell_search_all(iq, nof_prb, nof_periods=8, force_n_id_2=-1, threshold=20.0, threshold_next=0.0, sss_ratio_min=0.0, shared_pss_ratio=0.0, max_cells=0,
                    device=0, with_corr=False, rates=RATES_3GPP):
    """lsn_cell_search_all: every cell of the carrier in iq (as cell_search: numpy complex64 or a torch cuda tensor, one antenna), strongest first -> list of
    CellFound (cell: what cell_search reports, round, shared_pss, sss_ratio, rel_power_db)[, corr[rounds run, 3, 75 N]: the correlation each round decided on].
    Arguments left 0 take the library's defaults (threshold_next 8, sss_ratio_min 1.5, shared_pss_ratio 0.6, max_cells 8); threshold_next is measured for 8
    periods and must be raised for fewer."""
    import numpy as np
    N = symbol_sz(nof_prb, rates) or 128
    cfg = CellSearchAllCfg(int(nof_periods), int(force_n_id_2), float(threshold), float(threshold_next), float(sss_ratio_min), float(shared_pss_ratio), int(max_cells))
    cap = int(max_cells) if 0 < int(max_cells) <= 8 else 8
    out = (CellFound * 8)()
    nf = C.c_uint32(0)
    corr = np.zeros((cap + 1, 3, 75 * N), dtype=np.float32) if with_corr else None
    if hasattr(iq, "data_ptr"):
        ptr, n, on_dev = iq.data_ptr(), iq.numel(), 1
    else:
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        ptr, n, on_dev = iq.ctypes.data, iq.size, 0
    _check_n(lib().lsn_cell_search_all(device, ptr, on_dev, n, nof_prb, int(rates), C.byref(cfg), out, C.byref(nf), corr.ctypes.data if with_corr else None),
             "lsn_cell_search_all")
    cells = [CellFound.from_buffer_copy(out[i]) for i in range(nf.value)]
    if not with_corr:
        return cells
    rounds = 1 if not cells else cells[-1].round + (2 if len(cells) < cap else 1)
    return cells, corr[:rounds]


def pss_cancel(iq, nof_prb, n_id_2, pss_pos, cfo_hz=0.0, nof_periods=8, device=0, rates=RATES_3GPP):
    """lsn_pss_cancel: the cancellation step of cell_search_all alone, on host samples -> (residual complex64 like iq, a complex64 [nof_periods + 1])"""
    import numpy as np
    iq = np.ascontiguousarray(iq, dtype=np.complex64)
    res = np.zeros_like(iq)
    a = np.zeros(int(nof_periods) + 1, dtype=np.complex64)
    _check(lib().lsn_pss_cancel(device, iq.ctypes.data, iq.size, int(nof_prb), int(rates), int(nof_periods), int(n_id_2), int(pss_pos), float(cfo_hz),
                                res.ctypes.data, a.ctypes.data), "lsn_pss_cancel")
    return res, a


def sss_accumulate(iq, nof_prb, n_id_2, pss_pos, nof_periods=8, device=0, rates=RATES_3GPP):
    """lsn_sss_accumulate: the accumulated SSS decision's numbers at lag pss_pos of root n_id_2 -> dict(sums complex64 [2 CP, occurrence, 336], valid [2, occurrence],
    halves float32 [occurrence, 2, 3], acc float32 [2, 336])"""
    import numpy as np
    iq = np.ascontiguousarray(iq, dtype=np.complex64)
    nocc = int(nof_periods) + 1
    sums = np.zeros((2, nocc, 336), dtype=np.complex64)
    valid = np.zeros((2, nocc), dtype=np.uint32)
    halves = np.zeros((nocc, 2, 3), dtype=np.float32)
    acc = np.zeros((2, 336), dtype=np.float32)
    _check(lib().lsn_sss_accumulate(device, iq.ctypes.data, iq.size, int(nof_prb), int(rates), int(nof_periods), int(n_id_2), int(pss_pos), sums.ctypes.data,
                                    valid.ctypes.data, halves.ctypes.data, acc.ctypes.data), "lsn_sss_accumulate")
    return dict(sums=sums, valid=valid, halves=halves, acc=acc)


def cell_search_all_plan(pss_pos, N, W5=None):
    """lsn_cell_search_all_plan (needs no GPU): the lags a cancellation at pss_pos changes -> dict(n_lo, n_lag, runs=[(lo, len), ...])"""
    pl = CellSearchAllPlan()
    rc = lib().lsn_cell_search_all_plan(int(pss_pos), int(N), int(75 * N if W5 is None else W5), C.byref(pl))
    if rc != LSN_SUCCESS:
        raise ValueError("lsn_cell_search_all_plan refused (pss_pos %d, N %d)" % (pss_pos, N))
    return dict(n_lo=int(pl.n_lo), n_lag=int(pl.n_lag), runs=[(int(pl.run_lo[i]), int(pl.run_len[i])) for i in range(pl.nof_runs)])


def cell_search_all_decide(round, peak, sum, W5, acc, nof_periods=8, threshold=20.0, threshold_next=0.0, sss_ratio_min=0.0, shared_pss_ratio=0.0, max_cells=0):
    """lsn_cell_search_all_decide (needs no GPU): the rule of one round on its statistics; acc: [2, 336] accumulated powers -> CellSearchAllDecision"""
    import numpy as np
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    if acc.shape != (2, 336):
        raise ValueError("acc: [2, 336]")
    cfg = CellSearchAllCfg(int(nof_periods), -1, float(threshold), float(threshold_next), float(sss_ratio_min), float(shared_pss_ratio), int(max_cells))
    out = CellSearchAllDecision()
    rc = lib().lsn_cell_search_all_decide(C.byref(cfg), int(round), float(peak), float(sum), int(W5), acc.ctypes.data, C.byref(out))
    if rc != LSN_SUCCESS:
        raise ValueError("lsn_cell_search_all_decide refused: %d" % rc)
    return out


def clock_cfg(nof_prb, search, max_ppm=200.0, rates=RATES_3GPP, max_periods=0):
    """lsn_clock_cfg_t from the answer of cell_search (or anything with n_id_2, pss_pos, sf_start, cfo_hz).  A pss_pos in the first four samples leaves no room
    for the first window: the occurrence one period later is taken as number 0"""
    W5 = 75 * (symbol_sz(nof_prb, rates) or 128)
    pss_pos = int(search.pss_pos) + (W5 if int(search.pss_pos) < 4 else 0)
    return ClockCfg(C.sizeof(ClockCfg), int(nof_prb), int(rates), int(search.n_id_2), pss_pos, float(search.cfo_hz), float(max_ppm), int(max_periods),
                    int(search.sf_start))


def clock_estimate(iq, nof_prb, search, max_ppm=200.0, rates=RATES_3GPP, with_obs=False, max_periods=0, device=0):
    """lsn_clock_estimate: the sample-clock error of the samples iq (one antenna at the nominal rate; numpy complex64 or a torch cuda tensor) from the positions of
    their PSS occurrences; search: the CellSearch of cell_search on their head.  -> Clock (found, eps, sample_rate_hz, sf_start, ...)[, the observations of
    the last round]"""
    import numpy as np
    cfg = clock_cfg(nof_prb, search, max_ppm, rates, max_periods)
    if hasattr(iq, "data_ptr"):
        ptr, n, on_dev = iq.data_ptr(), iq.numel(), 1
    else:
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        ptr, n, on_dev = iq.ctypes.data, iq.size, 0
    out = Clock()
    obs = (ClockObs * 4096)() if with_obs else None
    _check_n(lib().lsn_clock_estimate(device, ptr, on_dev, n, C.byref(cfg), C.byref(out), obs, 4096 if with_obs else 0), "lsn_clock_estimate")
    return (out, list(obs[:out.nof_periods])) if with_obs else out


def file_clock_estimate(path, nof_prb, search, nof_antennas=1, antenna=0, sample_format=FILE_CF32, sample_scale=0.0, offset_time=0, sample_rate=None,
                        center_offset_hz=0.0, offset_time_frac=0.0, max_ppm=200.0, rates=RATES_3GPP, max_periods=0, device=0):
    """lsn_file_clock_estimate: the same on a recording, of which only the slices around the PSS occurrences are read.  search: cell_search on the head of the
    file from offset_time on (resampled at the NOMINAL sample_rate when the file has a rate of its own).  -> Clock; sample_rate_hz and sf_start (samples of the
    file from its first one) are the sample_rate and offset_time + offset_time_frac of Phy.process_file"""
    cfg = clock_cfg(nof_prb, search, max_ppm, rates, max_periods)
    fc = FileCfg(int(nof_antennas), int(offset_time), 0.0, int(sample_format), float(sample_scale))
    fr = FileRate(C.sizeof(FileRate), 0, float(sample_rate), float(offset_time_frac), float(center_offset_hz)) if sample_rate is not None else None
    if fr is None and (center_offset_hz != 0.0 or offset_time_frac != 0.0):
        raise ValueError("center_offset_hz / offset_time_frac need sample_rate (the nominal rate of the recording): both are part of the resampler")
    out = Clock()
    _check_n(lib().lsn_file_clock_estimate(device, os.fsencode(path), C.byref(fc), C.byref(fr) if fr is not None else None, int(antenna), C.byref(cfg), C.byref(out)),
             "lsn_file_clock_estimate")
    return out


def _resample_cfg(nof_antennas, rate_in, rate_out, first_sample, first_frac, in_base, out_first, passband_hz, sample_format, sample_scale, center_offset_hz=0.0):
    return ResampleCfg(C.sizeof(ResampleCfg), int(nof_antennas), int(sample_format), float(sample_scale), float(rate_in), float(rate_out), int(first_sample),
                       float(first_frac), int(in_base), int(out_first), float(passband_hz), float(center_offset_hz))


def resample_span(n_out, in_end, rate_in, rate_out, first_sample=0, first_frac=0.0, out_first=0, passband_hz=0.0, center_offset_hz=0.0):
    """lsn_resample_span -> dict(in_lo, in_hi, max_out, taps): the input samples [in_lo, in_hi) that outputs out_first .. out_first + n_out - 1 read, and the
    number of outputs from out_first on that a recording of in_end samples carries"""
    cfg = _resample_cfg(1, rate_in, rate_out, first_sample, first_frac, 0, out_first, passband_hz, FILE_CF32, 0.0, center_offset_hz)
    sp = ResampleSpan()
    _check(lib().lsn_resample_span(C.byref(cfg), int(n_out), int(in_end), C.byref(sp)), "lsn_resample_span")
    return dict(in_lo=int(sp.in_lo), in_hi=int(sp.in_hi), max_out=int(sp.max_out), taps=int(sp.taps))


def resample(iq, rate_in, rate_out, n_out=None, first_sample=0, first_frac=0.0, in_base=0, out_first=0, passband_hz=0.0, sample_format=FILE_CF32,
             sample_scale=0.0, device=0, center_offset_hz=0.0):
    """lsn_resample (GPU polyphase resampler, needs no Phy).  iq: [sample][antenna] (or [sample]: one antenna) numpy complex64, or int16 / int8 with a last
    axis of 2 (I, Q) for FILE_SC16 / FILE_SC8; iq[0] is sample in_base of the recording.  Output sample m sits at input position first_sample + first_frac +
    m rate_in / rate_out; the call returns outputs out_first .. out_first + n_out - 1 as complex64 [antenna][n_out] (n_out None: as many as iq carries).
    passband_hz: 15 kHz * (6 nof_prb + 1) for an LTE cell.  center_offset_hz: the wanted carrier relative to the recording's centre; sample n of the
    recording is multiplied by exp(-2 pi j center_offset_hz n / rate_in) (integer phase, two-table NCO) in front of the filter."""
    import numpy as np
    iq = np.ascontiguousarray(iq)
    pairs = sample_format != FILE_CF32
    if iq.ndim == (2 if pairs else 1):
        iq = iq.reshape(iq.shape[0], 1, *iq.shape[1:])
    iq = np.ascontiguousarray(iq, dtype=(np.complex64, np.int16, np.int8)[sample_format])
    n_in, nant = iq.shape[0], iq.shape[1]
    cfg = _resample_cfg(nant, rate_in, rate_out, first_sample, first_frac, in_base, out_first, passband_hz, sample_format, sample_scale, center_offset_hz)
    if n_out is None:
        sp = ResampleSpan()
        _check(lib().lsn_resample_span(C.byref(cfg), 0, int(in_base) + n_in, C.byref(sp)), "lsn_resample_span")
        n_out = int(sp.max_out)
    out = np.zeros((nant, n_out), dtype=np.complex64)
    _check(lib().lsn_resample(device, iq.ctypes.data, 0, n_in, C.byref(cfg), out.ctypes.data, 0, n_out), "lsn_resample")
    return out


def resample_cells(iq, rate_in, cells, n_out=None, in_base=0, sample_format=FILE_CF32, sample_scale=0.0, device=0):
    """lsn_resample_cells: several resamplings of ONE input in one upload and one kernel launch (k_resample_cells).  iq and in_base as resample; cells: a list of
    dicts with resample's per-cell arguments (rate_out, and optionally n_out, first_sample, first_frac, out_first, passband_hz, center_offset_hz; n_out None:
    as many as iq carries, or the call's n_out).  -> a list of complex64 [antenna][n_out] arrays, each bit for bit resample's with that cell's arguments"""
    iq = _scan_input(iq, sample_format)
    n_in, nant = iq.shape[0], iq.shape[1]
    n = len(cells)
    cfgs = (ResampleCfg * max(n, 1))()
    counts = (C.c_uint64 * max(n, 1))()
    outs = []
    for i, c in enumerate(cells):
        cfgs[i] = _resample_cfg(nant, rate_in, c["rate_out"], c.get("first_sample", 0), c.get("first_frac", 0.0), in_base, c.get("out_first", 0), c.get("passband_hz", 0.0),
                                sample_format, sample_scale, c.get("center_offset_hz", 0.0))
        k = c.get("n_out", n_out)
        if k is None:
            sp = ResampleSpan()
            _check(lib().lsn_resample_span(C.byref(cfgs[i]), 0, int(in_base) + n_in, C.byref(sp)), "lsn_resample_span")
            k = int(sp.max_out)
        counts[i] = int(k)
        outs.append(np.zeros((nant, int(k)), dtype=np.complex64))
    ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    _check(lib().lsn_resample_cells(device, iq.ctypes.data, 0, n_in, cfgs, n, ptrs, 0, counts), "lsn_resample_cells")
    return outs


def _resample_cells_map(name, iq, rate_in, cells, ring_samples, n_out, in_base, sample_format, sample_scale, device):
    iq = _scan_input(iq, sample_format)
    n_in, nant = iq.shape[0], iq.shape[1]
    n = len(cells)
    cfgs = (ResampleCfg * max(n, 1))()
    maps = (AntennaMap * max(n, 1))()
    counts = (C.c_uint64 * max(n, 1))()
    outs = []
    for i, c in enumerate(cells):
        cfgs[i] = _resample_cfg(nant, rate_in, c["rate_out"], c.get("first_sample", 0), c.get("first_frac", 0.0), in_base, c.get("out_first", 0), c.get("passband_hz", 0.0),
                                sample_format, sample_scale, c.get("center_offset_hz", 0.0))
        maps[i] = antenna_map(c.get("src"), c.get("offset_hz"))
        k = c.get("n_out", n_out)
        if k is None:   # (the span does not depend on the offsets)
            sp = ResampleSpan()
            plain = _resample_cfg(nant, rate_in, c["rate_out"], c.get("first_sample", 0), c.get("first_frac", 0.0), in_base, c.get("out_first", 0), c.get("passband_hz", 0.0),
                                  sample_format, sample_scale, 0.0)
            _check(lib().lsn_resample_span(C.byref(plain), 0, int(in_base) + n_in, C.byref(sp)), "lsn_resample_span")
            k = int(sp.max_out)
        counts[i] = int(k)
        outs.append(np.zeros((int(maps[i].nof_out) if maps[i].nof_out else nant, int(k)), dtype=np.complex64))
    ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    if ring_samples is None:
        rc = lib().lsn_resample_cells_map(device, iq.ctypes.data, 0, n_in, cfgs, maps, n, ptrs, 0, counts)
    else:
        rc = lib().lsn_resample_cells_ring_map(device, iq.ctypes.data, n_in, int(ring_samples), cfgs, maps, n, ptrs, counts)
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("%s: refused" % name)
    _check(rc, name)
    return outs


def resample_cells_map(iq, rate_in, cells, n_out=None, in_base=0, sample_format=FILE_CF32, sample_scale=0.0, device=0):
    """lsn_resample_cells_map: resample_cells with an antenna map per cell (k_resample_map).  cells: resample_cells' dicts, and src=(...) [, offset_hz=(...)]:
    output row a is cut from antenna src[a] of iq at center_offset_hz + offset_hz[a] and equals row src[a] of resample with that offset, bit for bit; no src: the
    identity, the cell as resample_cells makes it.  -> a list of complex64 [len(src) or antennas][n_out] arrays.  Raises ValueError when the library refuses"""
    return _resample_cells_map("lsn_resample_cells_map", iq, rate_in, cells, None, n_out, in_base, sample_format, sample_scale, device)


def resample_cells_ring_map(iq, rate_in, cells, ring_samples, n_out=None, in_base=0, sample_format=FILE_CF32, sample_scale=0.0, device=0):
    """lsn_resample_cells_ring_map: resample_cells_map through the kernel a Stream runs (k_resample_map_ring), the window placed in a ring as resample_cells_ring does"""
    return _resample_cells_map("lsn_resample_cells_ring_map", iq, rate_in, cells, ring_samples, n_out, in_base, sample_format, sample_scale, device)


def resample_cells_ring(iq, rate_in, cells, ring_samples, n_out=None, in_base=0, sample_format=FILE_CF32, sample_scale=0.0, device=0):
    """lsn_resample_cells_ring: resample_cells through the kernel a Stream runs (k_resample_ring).  The window iq = samples in_base .. in_base + len(iq) of the
    recording is placed into a device ring of ring_samples samples (a power of two), sample n at slot n mod ring_samples, and the cells are resampled out of
    the ring.  Arguments and result as resample_cells - the arrays are equal bit for bit.  Raises ValueError when the library refuses the call"""
    iq = _scan_input(iq, sample_format)
    n_in, nant = iq.shape[0], iq.shape[1]
    n = len(cells)
    cfgs = (ResampleCfg * max(n, 1))()
    counts = (C.c_uint64 * max(n, 1))()
    outs = []
    for i, c in enumerate(cells):
        cfgs[i] = _resample_cfg(nant, rate_in, c["rate_out"], c.get("first_sample", 0), c.get("first_frac", 0.0), in_base, c.get("out_first", 0), c.get("passband_hz", 0.0),
                                sample_format, sample_scale, c.get("center_offset_hz", 0.0))
        k = c.get("n_out", n_out)
        if k is None:
            sp = ResampleSpan()
            _check(lib().lsn_resample_span(C.byref(cfgs[i]), 0, int(in_base) + n_in, C.byref(sp)), "lsn_resample_span")
            k = int(sp.max_out)
        counts[i] = int(k)
        outs.append(np.zeros((nant, int(k)), dtype=np.complex64))
    ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    rc = lib().lsn_resample_cells_ring(device, iq.ctypes.data, n_in, int(ring_samples), cfgs, n, ptrs, counts)
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("resample_cells_ring: refused")
    _check(rc, "lsn_resample_cells_ring")
    return outs


def channel_filter_design(rate_in, passband_hz, stopband_hz):
    """lsn_channel_filter_design (needs no GPU) -> dict(L, fc, taps: float32 [2 L + 1], g[-L] .. g[L]).  Raises ValueError when the library refuses the filter"""
    import numpy as np
    d = ChannelFilterDesign(C.sizeof(ChannelFilterDesign), 0, 0, 0, 0.0)
    taps = np.zeros(2 * 512 + 1, dtype=np.float32)
    rc = lib().lsn_channel_filter_design(float(rate_in), float(passband_hz), float(stopband_hz), C.byref(d), taps.ctypes.data, taps.size)
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("channel filter: refused")
    _check(rc, "lsn_channel_filter_design")
    return dict(L=int(d.half_len), fc=float(d.cutoff), taps=taps[:d.nof_taps].copy())


def _channel_filter_cfg(nof_antennas, rate_in, passband_hz, stopband_hz, center_offset_hz, in_base, out_first, sample_format, sample_scale):
    return ChannelFilterCfg(C.sizeof(ChannelFilterCfg), int(nof_antennas), int(sample_format), float(sample_scale), float(rate_in), float(passband_hz), float(stopband_hz),
                            float(center_offset_hz), int(in_base), int(out_first))


def channel_filter_span(n_out, in_end, rate_in, passband_hz, stopband_hz, out_first=0, center_offset_hz=0.0):
    """lsn_channel_filter_span (needs no GPU) -> dict(in_lo, in_hi, max_out, taps): the input samples [in_lo, in_hi) that y1[out_first .. out_first + n_out - 1]
    read, and the number of outputs from out_first on that a recording of in_end samples carries.  Raises ValueError when the library refuses the filter"""
    cfg = _channel_filter_cfg(1, rate_in, passband_hz, stopband_hz, center_offset_hz, 0, out_first, FILE_CF32, 0.0)
    sp = ResampleSpan()
    rc = lib().lsn_channel_filter_span(C.byref(cfg), int(n_out), int(in_end), C.byref(sp))
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("channel filter: refused")
    _check(rc, "lsn_channel_filter_span")
    return dict(in_lo=int(sp.in_lo), in_hi=int(sp.in_hi), max_out=int(sp.max_out), taps=int(sp.taps))


def channel_filter(iq, rate_in, passband_hz, stopband_hz, n_out=None, center_offset_hz=0.0, in_base=0, out_first=0, sample_format=FILE_CF32, sample_scale=0.0, device=0):
    """lsn_channel_filter (k_chan_fir, needs no Phy): stage 1 alone.  iq and in_base as resample.  -> y1[out_first .. out_first + n_out - 1] as complex64
    [n_out][antenna] (n_out None: as many as iq carries) - what resample takes as input with in_base=out_first and no center_offset_hz"""
    iq = _scan_input(iq, sample_format)
    n_in, nant = iq.shape[0], iq.shape[1]
    cfg = _channel_filter_cfg(nant, rate_in, passband_hz, stopband_hz, center_offset_hz, in_base, out_first, sample_format, sample_scale)
    if n_out is None:
        sp = ResampleSpan()
        _check(lib().lsn_channel_filter_span(C.byref(cfg), 0, int(in_base) + n_in, C.byref(sp)), "lsn_channel_filter_span")
        n_out = int(sp.max_out)
    out = np.zeros((int(n_out), nant), dtype=np.complex64)
    _check(lib().lsn_channel_filter(device, iq.ctypes.data, 0, n_in, C.byref(cfg), out.ctypes.data, 0, int(n_out)), "lsn_channel_filter")
    return out


def channel_filter_ring(iq, rate_in, cells, ring_samples, in_base=0, sample_format=FILE_CF32, sample_scale=0.0, device=0):
    """lsn_channel_filter_ring: stage 1 through the kernel a filtered Stream runs (k_chan_fir_ring).  The window iq = samples in_base .. in_base + len(iq) of the
    recording is placed into a device ring of ring_samples samples (a power of two), sample n at slot n mod ring_samples, every other slot holding a NaN pattern,
    and up to 8 filters run out of the ring in ONE launch.  cells: a list of dict(passband_hz, stopband_hz, n_out[, center_offset_hz, out_first]) -> a list of
    complex64 [n_out][antenna] arrays, each bit for bit channel_filter's with that cell's arguments.  Raises ValueError when the library refuses the call (the
    outputs, available as the exception's .outs, are untouched)"""
    iq = _scan_input(iq, sample_format)
    n_in, nant = iq.shape[0], iq.shape[1]
    n = len(cells)
    cfgs = (ChannelFilterCfg * max(n, 1))()
    counts = (C.c_uint64 * max(n, 1))()
    outs = []
    for i, c in enumerate(cells):
        cfgs[i] = _channel_filter_cfg(nant, rate_in, c["passband_hz"], c["stopband_hz"], c.get("center_offset_hz", 0.0), in_base, c.get("out_first", 0), sample_format, sample_scale)
        counts[i] = int(c["n_out"])
        outs.append(np.zeros((int(c["n_out"]), nant), dtype=np.complex64))
    ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    rc = lib().lsn_channel_filter_ring(device, iq.ctypes.data, n_in, int(ring_samples), cfgs, n, ptrs, counts)
    if rc == LSN_ERROR_INVALID_INPUTS:
        err = ValueError("channel_filter_ring: refused")
        err.outs = outs
        raise err
    _check(rc, "lsn_channel_filter_ring")
    return outs


def cells_stopbands(carriers_hz, nof_prb, rate_in):
    """lsn_cells_stopbands (needs no GPU): the stopband_hz of every cell of a recording from its neighbours - the distance from its carrier to the nearest occupied
    edge of another cell, capped at rate_in / 2; 0.0 (no filter) for a cell that has no neighbour.  Raises ValueError when a neighbour is too close for the filter"""
    n = len(carriers_hz)
    f = (C.c_double * max(n, 1))(*[float(c.center_offset_hz if isinstance(c, Carrier) else c) for c in carriers_hz])
    prb = (C.c_uint32 * max(n, 1))(*[int(p) for p in nof_prb])
    out = (C.c_double * max(n, 1))()
    rc = lib().lsn_cells_stopbands(f, prb, n, float(rate_in), out)
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("cells_stopbands: refused")
    _check(rc, "lsn_cells_stopbands")
    return [float(v) for v in out[:n]]


def _file_cell(phy, kw):
    """(phy or None, dict) -> FileCell.  center_offset_hz may be a Carrier of carrier_scan / file_carrier_scan: its center_offset_hz is taken as it is"""
    kw = dict(kw)
    if "stopband_hz" in kw:   # the channel filter is a setting of the Phy (set_channel_filter): sticky, like the call
        stop = kw.pop("stopband_hz")
        if phy is None or not phy.set_channel_filter(stop):
            raise ValueError("stopband_hz: %s" % ("needs a Phy" if phy is None else "refused"))
    f0 = kw.pop("center_offset_hz", 0.0)
    if isinstance(f0, Carrier):
        f0 = f0.center_offset_hz
    start_tti = kw.pop("start_tti", 0)
    cell = FileCell(C.sizeof(FileCell), int(kw.pop("nof_prb", 0)), int(kw.pop("rates", RATES_3GPP)), phy._h if phy is not None else None, float(f0),
                    int(kw.pop("offset_time", 0)), float(kw.pop("offset_time_frac", 0.0)), float(kw.pop("offset_freq", 0.0)),
                    start_tti if start_tti == TTI_FROM_MIB else start_tti % 10240, int(kw.pop("update_meta_period", 0)), int(kw.pop("max_subframes", 0)), 0, 0)
    if kw:
        raise TypeError("unknown cell argument(s): %s" % ", ".join(sorted(kw)))
    return cell


def file_cells_span(sample_rate, cells, in_end, block=0, blk_subframes=800, nof_antennas=1, sample_format=FILE_CF32, sample_scale=0.0, nof_out=None):
    """lsn_file_cells_span (needs no GPU): the plan of block `block` of process_file_cells.  cells: a list of dicts (nof_prb, rates, center_offset_hz, offset_time,
    offset_time_frac, max_subframes, ...) or of (phy, dict) pairs.  -> dict(in_lo, in_hi: the union of input samples the block reads; blk_used; nof_active;
    first_subframe, nof_subframes, taps: one entry per cell).  nof_out (lsn_file_cells_span_map, the antenna map): per cell the antennas of its Phy, 1 or 2, or 0 =
    nof_antennas, which is then the RECORDING's - blk_used follows it.  Raises ValueError when the library refuses the cells"""
    arr = (FileCell * max(len(cells), 1))()
    for i, c in enumerate(cells):
        arr[i] = _file_cell(*c) if isinstance(c, tuple) else _file_cell(None, c)
    fc = FileCfg(int(nof_antennas), 0, 0.0, int(sample_format), float(sample_scale))
    sp = FileCellsSpan()
    if nof_out is None:
        rc = lib().lsn_file_cells_span(C.byref(fc), float(sample_rate), arr, len(cells), int(in_end), int(block), int(blk_subframes), C.byref(sp))
    else:
        if len(nof_out) != len(cells):
            raise ValueError("file_cells_span: nof_out needs one value per cell")
        rows = (C.c_uint32 * max(len(cells), 1))(*[int(v) for v in nof_out])
        rc = lib().lsn_file_cells_span_map(C.byref(fc), float(sample_rate), arr, len(cells), rows, int(in_end), int(block), int(blk_subframes), C.byref(sp))
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("file cells: refused")
    _check(rc, "lsn_file_cells_span")
    n = len(cells)
    return dict(in_lo=int(sp.in_lo), in_hi=int(sp.in_hi), blk_used=int(sp.blk_used), nof_active=int(sp.nof_active), first_subframe=[int(v) for v in sp.first_subframe[:n]],
                nof_subframes=[int(v) for v in sp.nof_subframes[:n]], taps=[int(v) for v in sp.taps[:n]])


def process_file_cells(path, sample_rate, cells, nof_antennas=None, sample_format=FILE_CF32, sample_scale=0.0, with_status=False):
    """lsn_file_process_cells: replay several cells of one recording made at sample_rate (Hz) in ONE pass over the file - one read and one host-to-device copy
    per block, one kernel launch for all cells, each Phy fed with its own cell's subframes.  cells: a list of (phy, dict(center_offset_hz=, start_tti=, offset_time=,
    offset_time_frac=, offset_freq=, max_subframes=, update_meta_period=, stopband_hz=)); center_offset_hz may be a Carrier of file_carrier_scan; stopband_hz
    (cells_stopbands) is set on that Phy as set_channel_filter does - every cell or none.  start_tti may be
    TTI_FROM_MIB, per cell.  -> the list of subframes done, one per cell [, the list of per-cell status codes].  Raises ValueError when the library refuses
    the cells (nothing is decoded, every Phy stays usable)"""
    arr = (FileCell * max(len(cells), 1))()
    for i, (phy, kw) in enumerate(cells):
        arr[i] = _file_cell(phy, kw)
    if nof_antennas is None:
        nof_antennas = cells[0][0].nof_rx_antennas if cells else 1
    fc = FileCfg(int(nof_antennas), 0, 0.0, int(sample_format), float(sample_scale))
    rc = lib().lsn_file_process_cells(os.fsencode(path), C.byref(fc), float(sample_rate), arr, len(cells))
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("process_file_cells: refused")
    _check(rc, "lsn_file_process_cells")
    done = [int(c.subframes_done) for c in arr[:len(cells)]]
    return (done, [int(c.status) for c in arr[:len(cells)]]) if with_status else done


def _stream_cfg(sample_rate, nof_antennas, sample_format, sample_scale, block_subframes, ring_samples, device):
    return StreamCfg(C.sizeof(StreamCfg), int(device), float(sample_rate), int(nof_antennas), int(sample_format), float(sample_scale), int(block_subframes), int(ring_samples))


def stream_span(sample_rate, cells, pushed, nof_antennas=1, sample_format=FILE_CF32, sample_scale=0.0, block_subframes=0, ring_samples=0, stopbands=None, nof_out=None):
    """lsn_stream_span (needs no GPU): the plan of a Stream after `pushed` samples in all.  cells as file_cells_span.  stopbands (lsn_stream_span_filtered): None,
    or one stopband_hz per cell - the plan of the stream with the channel filter on, without a Phy: every span L samples wider on both sides, a cell's subframes
    counted in front of pushed - L; every cell or none (0.0: none), and all 0.0 is None.  With (phy, dict) cells the Phys' own setting counts, as in file_cells_span.  -> dict(ring_samples: the given one or the
    default; block_input: input samples of one block of every cell, which the ring must hold; block_subframes; per cell subframes_complete - what a flush at that
    point has submitted in all -, subframes_submitted - what a stream that was never flushed has - and taps; oldest_needed / oldest_needed_flushed: the oldest
    sample a cell still needs in the two cases).  nof_out (lsn_stream_span_map): as file_cells_span's; not together with stopbands.  Raises ValueError when the
    library refuses cells or ring"""
    arr = (FileCell * max(len(cells), 1))()
    for i, c in enumerate(cells):
        arr[i] = _file_cell(*c) if isinstance(c, tuple) else _file_cell(None, c)
    cfg = _stream_cfg(sample_rate, nof_antennas, sample_format, sample_scale, block_subframes, ring_samples, 0)
    sp = StreamSpan()
    if nof_out is not None:
        if stopbands is not None or len(nof_out) != len(cells):
            raise ValueError("stream_span: nof_out needs one value per cell and no stopbands")
        rows = (C.c_uint32 * max(len(cells), 1))(*[int(v) for v in nof_out])
        rc = lib().lsn_stream_span_map(C.byref(cfg), arr, len(cells), rows, int(pushed), C.byref(sp))
    elif stopbands is None:
        rc = lib().lsn_stream_span(C.byref(cfg), arr, len(cells), int(pushed), C.byref(sp))
    else:
        if len(stopbands) != len(cells):
            raise ValueError("stream_span: stopbands needs one value per cell")
        stop = (C.c_double * max(len(cells), 1))(*[float(v) for v in stopbands])
        rc = lib().lsn_stream_span_filtered(C.byref(cfg), arr, len(cells), stop, int(pushed), C.byref(sp))
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("stream: refused")
    _check(rc, "lsn_stream_span")
    n = len(cells)
    return dict(ring_samples=int(sp.ring_samples), block_input=int(sp.block_input), block_subframes=int(sp.block_subframes), oldest_needed=int(sp.oldest_needed),
                oldest_needed_flushed=int(sp.oldest_needed_flushed), subframes_complete=[int(v) for v in sp.subframes_complete[:n]],
                subframes_submitted=[int(v) for v in sp.subframes_submitted[:n]], taps=[int(v) for v in sp.taps[:n]])


def _track_cfg(n_cells, kp=0.0, ki=0.0, max_ppm=0.0, lost_after=0, cfo_hz=0.0, initial_ppm=0.0, enable=True):
    cfg = StreamTrackCfg()
    cfg.struct_size, cfg.lost_after, cfg.kp, cfg.ki, cfg.max_ppm = C.sizeof(StreamTrackCfg), int(lost_after), float(kp), float(ki), float(max_ppm)
    for name, val, conv in (("cfo_hz", cfo_hz, float), ("initial_ppm", initial_ppm, float), ("enable", enable, lambda v: 1 if v else 0)):
        vals = list(val) if isinstance(val, (list, tuple)) else [val] * n_cells
        if len(vals) != n_cells:
            raise ValueError("track: %s needs one value per cell" % name)
        for i, v in enumerate(vals):
            getattr(cfg, name)[i] = conv(v)
    return cfg


def stream_track_step(state, e, valid, rate_in, rate_out, seglen, kp=0.0, ki=0.0, max_ppm=0.0, lost_after=0):
    """lsn_stream_track_step (needs no GPU): one step of the timing loop.  state: dict(integrator, correction, invalid_run, lost) -> (the new state, step -
    step_nominal as a signed integer in units of 2^-64 input samples).  Raises ValueError when the library refuses the gains"""
    cfg = _track_cfg(0, kp, ki, max_ppm, lost_after)
    st = StreamTrackState(float(state["integrator"]), float(state["correction"]), int(state["invalid_run"]), int(state["lost"]))
    hi, lo = C.c_uint64(), C.c_uint64()
    rc = lib().lsn_stream_track_step(C.byref(cfg), float(rate_in), float(rate_out), int(seglen), C.byref(st), float(e), 1 if valid else 0, C.byref(hi), C.byref(lo))
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("stream_track_step: refused")
    _check(rc, "lsn_stream_track_step")
    delta = (hi.value << 64) | lo.value
    if delta >> 127:
        delta -= 1 << 128
    return dict(integrator=float(st.integrator), correction=float(st.correction), invalid_run=int(st.invalid_run), lost=int(st.lost)), delta


def pss_timing_error(Cv, d):
    """lsn_pss_timing_error (needs no GPU): the 13 values of one window -> (geometrically valid, e in output samples, peak)"""
    import numpy as np
    Cv = np.ascontiguousarray(Cv, dtype=np.float32)
    if Cv.shape != (13,):
        raise ValueError("pss_timing_error: 13 values")
    e, pk = C.c_double(), C.c_double()
    rc = lib().lsn_pss_timing_error(Cv.ctypes.data, int(d), C.byref(e), C.byref(pk))
    _check_n(rc, "lsn_pss_timing_error")
    return bool(rc), float(e.value), float(pk.value)


def pss_timing(cells, device=0):
    """lsn_pss_timing: k_pss_timing without a Phy.  cells: a list of dict(blocks: complex64 [subframe][antenna][sflen], occ: [(subframe, p), ...], replica: complex64
    [N], d) - all of them in one launch while no cell has more than four occurrences -> a list of float32 arrays [n_occ][13].  Raises ValueError when refused"""
    import numpy as np
    n = len(cells)
    arr = (PssTimingCell * max(n, 1))()
    keep, outs = [], []
    for i, c in enumerate(cells):
        x = np.ascontiguousarray(c["blocks"], dtype=np.complex64)
        r = np.ascontiguousarray(c["replica"], dtype=np.complex64)
        occ = np.ascontiguousarray(np.asarray(c["occ"], dtype=np.uint32).reshape(-1, 2))
        if x.ndim != 3 or r.ndim != 1:
            raise ValueError("pss_timing: blocks [subframe][antenna][sflen], replica [N]")
        out = np.zeros((len(occ), 13), dtype=np.float32)
        keep.append((x, r, occ))
        outs.append(out)
        arr[i] = PssTimingCell(C.sizeof(PssTimingCell), len(r), int(c["d"]), x.shape[2], x.shape[1], x.shape[0], len(occ), 0, x.ctypes.data, r.ctypes.data,
                               occ.ctypes.data if len(occ) else None, out.ctypes.data if len(occ) else None)
    rc = lib().lsn_pss_timing(int(device), 0, arr, n)
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("pss_timing: refused")
    _check(rc, "lsn_pss_timing")
    return outs


def _reacquire_cfg(n_cells, after=0, min_ratio=0.0, enable=True):
    cfg = StreamReacquireCfg()
    cfg.struct_size, cfg.after, cfg.min_ratio = C.sizeof(StreamReacquireCfg), int(after), float(min_ratio)
    vals = list(enable) if isinstance(enable, (list, tuple)) else [enable] * n_cells
    if len(vals) != n_cells:
        raise ValueError("reacquire: enable needs one value per cell")
    for i, v in enumerate(vals):
        cfg.enable[i] = 1 if v else 0
    return cfg


def pss_acquire_decide(Cv, d, N, min_ratio=0.0, history_mean=None):
    """lsn_pss_acquire_decide (needs no GPU): the 75 N / d values of one search -> (accepted, offset in output samples, peak, peak / far).  history_mean None: an
    empty history; min_ratio 0: the default.  Raises ValueError when refused"""
    import numpy as np
    Cv = np.ascontiguousarray(Cv, dtype=np.float32)
    if Cv.ndim != 1:
        raise ValueError("pss_acquire_decide: one row of values")
    o, pk, ra = C.c_int64(), C.c_double(), C.c_double()
    rc = lib().lsn_pss_acquire_decide(Cv.ctypes.data, len(Cv), int(d), int(N), float(min_ratio), -1.0 if history_mean is None else float(history_mean),
                                      C.byref(o), C.byref(pk), C.byref(ra))
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("pss_acquire_decide: refused")
    _check_n(rc, "lsn_pss_acquire_decide")
    return bool(rc), int(o.value), float(pk.value), float(ra.value)


def _frame_sync_cfg(n_cells, tries=0, hold=True, enable=True):
    cfg = StreamFrameSyncCfg()
    cfg.struct_size, cfg.tries, cfg.hold = C.sizeof(StreamFrameSyncCfg), int(tries), 1 if hold else FRAME_SYNC_NO_HOLD
    vals = list(enable) if isinstance(enable, (list, tuple)) else [enable] * n_cells
    if len(vals) != n_cells:
        raise ValueError("frame_sync: enable needs one value per cell")
    for i, v in enumerate(vals):
        cfg.enable[i] = 1 if v else 0
    return cfg


def frame_sync_decide(mib, nof_prb, nof_ports, counted_tti):
    """lsn_frame_sync_decide (needs no GPU): the decision over one attempt.  mib: None (not found) or a dict with found, sfn, nof_prb, nof_ports (Phy.mib_decode's)
    -> (accepted, delta in subframes, signed in (-5120, 5120]).  Raises ValueError when refused, RuntimeError for a counted_tti that is no multiple of 5"""
    m = Mib()
    for k, v in (mib or {}).items():
        setattr(m, k, int(v))
    if not 0 <= int(counted_tti) < 1 << 32:
        raise ValueError("frame_sync_decide: refused")
    delta = C.c_int32()
    rc = lib().lsn_frame_sync_decide(C.byref(m), int(nof_prb), int(nof_ports), int(counted_tti), C.byref(delta))
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("frame_sync_decide: refused")
    _check_n(rc, "lsn_frame_sync_decide")
    return bool(rc), int(delta.value)


def pss_acquire(cells, device=0):
    """lsn_pss_acquire: k_pss_acquire without a Phy.  cells: a list of dict(blocks: complex64 [6][antenna][15 N], replica: complex64 [N], d), all of them in one
    launch -> a list of float32 arrays [75 N / d].  Raises ValueError when refused"""
    import numpy as np
    n = len(cells)
    arr = (PssAcquireCell * max(n, 1))()
    keep, outs = [], []
    for i, c in enumerate(cells):
        x = np.ascontiguousarray(c["blocks"], dtype=np.complex64)
        r = np.ascontiguousarray(c["replica"], dtype=np.complex64)
        if x.ndim != 3 or x.shape[0] != 6 or r.ndim != 1:
            raise ValueError("pss_acquire: blocks [6][antenna][sflen], replica [N]")
        out = np.zeros(75 * len(r) // max(int(c["d"]), 1), dtype=np.float32)
        keep.append((x, r))
        outs.append(out)
        arr[i] = PssAcquireCell(C.sizeof(PssAcquireCell), len(r), int(c["d"]), x.shape[2], x.shape[1], 0, x.ctypes.data, r.ctypes.data, out.ctypes.data)
    rc = lib().lsn_pss_acquire(int(device), 0, arr, n)
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("pss_acquire: refused")
    _check(rc, "lsn_pss_acquire")
    return outs


class Stream:
    """lsn_stream_*: the cells of a live wideband stream that arrives in host buffers.  cells: a list of (phy, dict(...)) with the keys of process_file_cells
    (center_offset_hz, start_tti - not TTI_FROM_MIB -, offset_time / offset_time_frac: the start of the cell's subframe 0 counted from the first sample ever
    pushed, offset_freq, max_subframes, update_meta_period, stopband_hz).  stopband_hz (cells_stopbands) sets the channel filter on that Phy as
    set_channel_filter does - every cell or none: the stream then runs the file pass's two stages out of the ring (k_chan_fir_ring, then k_resample per cell) and
    the records are those of process_file_cells with the filter.  The raw samples live in a device ring (ring_samples, a power of two; 0: chosen by the library);
    a cell is submitted to its Phy whenever block_subframes complete subframes of it have arrived (0: the file source's block size).  The Phys' records are
    those of process_file_cells on a file of the same bytes, however the stream is cut into pushes.  Raises ValueError when the library refuses the stream
    (nothing is allocated, every Phy stays usable).  Close the stream before its Phys; a Phy that is closed first closes the stream."""

    def __init__(self, sample_rate, cells, nof_antennas=None, sample_format=FILE_CF32, sample_scale=0.0, block_subframes=0, ring_samples=0, device=0, track=None,
                 reacquire=None, frame_sync=None):
        """track: None, or the keyword arguments of track() - the timing loop is set up before the first push.  reacquire: None, or the keyword arguments of
        reacquire(), called behind track().  frame_sync: None, or the keyword arguments of frame_sync(), called behind reacquire().  A refused track, reacquire
        or frame_sync closes the stream and raises"""
        self._h = None
        self._phys = [phy for phy, _ in cells]     # kept alive as long as the stream
        arr = (FileCell * max(len(cells), 1))()
        for i, (phy, kw) in enumerate(cells):
            arr[i] = _file_cell(phy, kw)
        if nof_antennas is None:
            nof_antennas = cells[0][0].nof_rx_antennas if cells else 1
        self.nof_antennas, self.sample_format, self.nof_cells = int(nof_antennas), int(sample_format), len(cells)
        cfg = _stream_cfg(sample_rate, nof_antennas, sample_format, sample_scale, block_subframes, ring_samples, device)
        h = C.c_void_p()
        rc = lib().lsn_stream_open(C.byref(cfg), arr, len(cells), C.byref(h))
        if rc == LSN_ERROR_INVALID_INPUTS:
            raise ValueError("Stream: refused")
        _check(rc, "lsn_stream_open")
        self._h = h
        import weakref
        for phy in self._phys:
            phy._stream = weakref.ref(self)
        if track is not None:
            try:
                self.track(**track)
            except ValueError:
                self.close()
                raise
        if reacquire is not None:
            try:
                self.reacquire(**reacquire)
            except ValueError:
                self.close()
                raise
        if frame_sync is not None:
            try:
                self.frame_sync(**frame_sync)
            except ValueError:
                self.close()
                raise

    def track(self, kp=0.0, ki=0.0, max_ppm=0.0, lost_after=0, cfo_hz=0.0, initial_ppm=0.0, enable=True):
        """lsn_stream_track: a PSS timing loop per cell follows the sample clock.  Only before the first push.  cfo_hz, initial_ppm, enable: one
        value for every cell, or a list with one per cell; kp, ki, max_ppm, lost_after: 0 = the defaults (1/4, 1/32, 100, 40).  Raises ValueError when the
        library refuses (the stream is unchanged and usable)"""
        self._call(lib().lsn_stream_track(self._h, C.byref(_track_cfg(self.nof_cells, kp, ki, max_ppm, lost_after, cfo_hz, initial_ppm, enable))), "lsn_stream_track")

    def track_status(self):
        """lsn_stream_track_status -> dict of per-cell lists: segments, valid, invalid, lost, last_error (output samples), correction_ppm, integrator_ppm,
        position_drift (input samples).  Behind a flush it is a function of the samples pushed"""
        st = StreamTrackStatus()
        st.struct_size = C.sizeof(StreamTrackStatus)
        self._call(lib().lsn_stream_track_status(self._h, C.byref(st)), "lsn_stream_track_status")
        n = int(st.nof_cells)
        return dict(segments=[int(v) for v in st.segments[:n]], valid=[int(v) for v in st.valid[:n]], invalid=[int(v) for v in st.invalid[:n]],
                    lost=[int(v) for v in st.lost[:n]], last_error=[float(v) for v in st.last_error[:n]], correction_ppm=[float(v) for v in st.correction_ppm[:n]],
                    integrator_ppm=[float(v) for v in st.integrator_ppm[:n]], position_drift=[float(v) for v in st.position_drift[:n]])

    def reacquire(self, after=0, min_ratio=0.0, enable=True):
        """lsn_stream_reacquire: a cell whose loop saw `after` invalid segments in a row (0: the loop's lost_after) is searched over a whole half frame and its
        position moved once to the nearest PSS.  Only after track() and before the first push.  enable: one value for every cell, or a list.  Raises
        ValueError when the library refuses (the stream is unchanged and usable)"""
        self._call(lib().lsn_stream_reacquire(self._h, C.byref(_reacquire_cfg(self.nof_cells, after, min_ratio, enable))), "lsn_stream_reacquire")

    def reacquire_status(self):
        """lsn_stream_reacquire_status -> dict of per-cell lists: launched, accepted, rejected, last_peak, last_ratio, last_offset (output samples), jump_segment,
        jumps_total (input samples).  Behind a flush it is a function of the samples pushed"""
        st = StreamReacquireStatus()
        st.struct_size = C.sizeof(StreamReacquireStatus)
        self._call(lib().lsn_stream_reacquire_status(self._h, C.byref(st)), "lsn_stream_reacquire_status")
        n = int(st.nof_cells)
        return dict(launched=[int(v) for v in st.launched[:n]], accepted=[int(v) for v in st.accepted[:n]], rejected=[int(v) for v in st.rejected[:n]],
                    last_peak=[float(v) for v in st.last_peak[:n]], last_ratio=[float(v) for v in st.last_ratio[:n]], last_offset=[int(v) for v in st.last_offset[:n]],
                    jump_segment=[int(v) for v in st.jump_segment[:n]], jumps_total=[float(v) for v in st.jumps_total[:n]])

    def frame_sync(self, tries=0, hold=True, enable=True):
        """lsn_stream_frame_sync: after a jump of reacquire() the first subframe of the following segments goes through the PBCH decode until one - at most `tries`
        (0: 8) - says which TTI the cell is at; from two segments behind it on the records carry that TTI.  hold (the default): the subframes between
        the jump and that point are not submitted to the Phy; False: they are, as counted.  Only after reacquire() and before the first push.  enable: one value
        for every cell, or a list.  Raises ValueError when the library refuses (the stream is unchanged and usable)"""
        self._call(lib().lsn_stream_frame_sync(self._h, C.byref(_frame_sync_cfg(self.nof_cells, tries, hold, enable))), "lsn_stream_frame_sync")

    def frame_sync_status(self):
        """lsn_stream_frame_sync_status -> dict of per-cell lists: checks, attempts, confirmed, relabelled, given_up, accept_segment, relabel_segment, held
        (subframes), last_sfn, last_delta (subframes, signed), shift (subframes, mod 10240).  Behind a flush it is a function of the samples pushed"""
        st = StreamFrameSyncStatus()
        st.struct_size = C.sizeof(StreamFrameSyncStatus)
        self._call(lib().lsn_stream_frame_sync_status(self._h, C.byref(st)), "lsn_stream_frame_sync_status")
        n = int(st.nof_cells)
        return {name: [int(v) for v in getattr(st, name)[:n]] for name, _ in StreamFrameSyncStatus._fields_[2:]}

    def _call(self, rc, what):
        if rc == LSN_ERROR_INVALID_INPUTS:
            raise ValueError("%s: refused" % what)
        _check(rc, what)

    def push(self, iq):
        """samples as resample takes them: [sample][antenna] complex64 (or [sample] for one antenna), int16 / int8 with a last axis of 2 for FILE_SC16 / FILE_SC8.
        Returns when they are in the ring; a pinned (page-locked) array is copied without a detour"""
        import numpy as np
        dt = (np.complex64, np.int16, np.int8)[self.sample_format]
        iq = np.ascontiguousarray(iq, dtype=dt)
        per = self.nof_antennas * (1 if self.sample_format == FILE_CF32 else 2)
        if iq.size % per:
            raise ValueError("push: not a whole number of samples of %d antenna(s)" % self.nof_antennas)
        self._call(lib().lsn_stream_push(self._h, iq.ctypes.data, iq.size // per), "lsn_stream_push")

    def gap(self, n):
        """n samples the radio dropped: zeros arrive, positions stay"""
        self._call(lib().lsn_stream_push(self._h, None, int(n)), "lsn_stream_push")

    def flush(self):
        """submit every complete subframe, wait for every Phy -> subframes done per cell; the stream goes on afterwards"""
        self._call(lib().lsn_stream_flush(self._h), "lsn_stream_flush")
        return self.status()["subframes_submitted"]

    def status(self):
        st = StreamStatus()
        self._call(lib().lsn_stream_status(self._h, C.byref(st)), "lsn_stream_status")
        n = int(st.nof_cells)
        return dict(samples_pushed=int(st.samples_pushed), ring_samples=int(st.ring_samples), oldest_needed=int(st.oldest_needed), block_subframes=int(st.block_subframes),
                    failed=int(st.failed), status=[int(v) for v in st.status[:n]], subframes_submitted=[int(v) for v in st.subframes_submitted[:n]])

    def close(self):
        """flush, then free; the Phys stay usable -> subframes done per cell (None when the stream was closed already).  Every later call raises ValueError"""
        if self._h is None:
            return None
        h, self._h = self._h, None
        st = StreamStatus()
        rc = lib().lsn_stream_flush(h)              # (the close's own flush finds nothing left: the counts are read between the two)
        lib().lsn_stream_status(h, C.byref(st))
        rc2 = lib().lsn_stream_close(h)
        for phy in self._phys:
            phy._stream = None
        self._phys = []
        self._call(rc if rc != LSN_SUCCESS else rc2, "lsn_stream_close")
        return [int(v) for v in st.subframes_submitted[:int(st.nof_cells)]]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SCAN_MAX_HYPOTHESES = 8192
SCAN_RATE_HZ = 1.92e6   # rate of a carrier's channel: six resource blocks, 128 samples per symbol
SCAN_ALL_ANTENNAS = 0xFFFFFFFF   # carrier_scan_cfg(antenna="all"): every antenna of the input, combined without their phases


def carrier_scan_cfg(rate_in, nof_antennas=1, antenna=0, sample_format=FILE_CF32, sample_scale=0.0, nof_periods=2, raster_hz=100e3, raster_offset_hz=0.0,
                     f_lo_hz=0.0, f_hi_hz=0.0, min_spacing_hz=1.4e6, threshold=20.0):
    antenna = SCAN_ALL_ANTENNAS if isinstance(antenna, str) and antenna == "all" else antenna
    return CarrierScanCfg(C.sizeof(CarrierScanCfg), int(nof_antennas), int(antenna), int(sample_format), float(sample_scale), int(nof_periods), float(rate_in),
                          float(raster_hz), float(raster_offset_hz), float(f_lo_hz), float(f_hi_hz), float(min_spacing_hz), float(threshold), 0)


def carrier_scan_plan(rate_in, with_bank=False, **kw):
    """lsn_carrier_scan_plan (needs no GPU): the hypotheses of a scan of a recording at rate_in, the channel filter and what the scan reads ->
    dict(nof_hypotheses, taps, nof_periods, nof_channel_samples, nof_input_samples, k, f_hz, tuning_word[, bank[512, taps, 2]]); kw: carrier_scan_cfg.
    Raises ValueError when the library refuses the configuration"""
    cfg = carrier_scan_cfg(rate_in, **kw)
    pl = CarrierScanPlan()
    hyp = (CarrierMetric * SCAN_MAX_HYPOTHESES)()
    rc = lib().lsn_carrier_scan_plan(C.byref(cfg), C.byref(pl), hyp, SCAN_MAX_HYPOTHESES, None)
    if rc == LSN_ERROR_INVALID_INPUTS:
        raise ValueError("carrier scan: configuration refused")
    _check(rc, "lsn_carrier_scan_plan")
    n = int(pl.nof_hypotheses)
    d = {f: int(getattr(pl, f)) for f, _ in CarrierScanPlan._fields_ if f != "reserved"}
    d.update(k=[int(h.k) for h in hyp[:n]], f_hz=[float(h.f_hz) for h in hyp[:n]], tuning_word=[int(h.tuning_word) for h in hyp[:n]])
    if with_bank:
        bank = np.zeros((512, d["taps"], 2), dtype=np.float32)
        _check(lib().lsn_carrier_scan_plan(C.byref(cfg), C.byref(pl), None, 0, bank.ctypes.data), "lsn_carrier_scan_plan")
        d["bank"] = bank
    return d


def carrier_scan_decide(metric, rate_in, **kw):
    """lsn_carrier_scan_decide (needs no GPU): metric: CarrierMetric entries or (k, f_hz, p2avg, peak) tuples -> indices of the accepted ones, in the order of acceptance"""
    cfg = carrier_scan_cfg(rate_in, **kw)
    arr = (CarrierMetric * max(len(metric), 1))()
    for i, m in enumerate(metric):
        arr[i] = m if isinstance(m, CarrierMetric) else CarrierMetric(k=int(m[0]), f_hz=float(m[1]), p2avg=float(m[2]), peak=float(m[3]))
    idx = (C.c_uint32 * max(len(metric), 1))()
    n = _check_n(lib().lsn_carrier_scan_decide(C.byref(cfg), arr, len(metric), idx, len(metric)), "lsn_carrier_scan_decide")
    return [int(i) for i in idx[:n]]


def _scan_result(n, carriers, metric, nhyp, with_metric):
    found = [Carrier.from_buffer_copy(c) for c in carriers[:min(n, len(carriers))]]
    return (found, [CarrierMetric.from_buffer_copy(m) for m in metric[:nhyp]]) if with_metric else found


def _scan_input(iq, sample_format):
    iq = np.ascontiguousarray(iq)
    if iq.ndim == (2 if sample_format != FILE_CF32 else 1):
        iq = iq.reshape(iq.shape[0], 1, *iq.shape[1:])
    return np.ascontiguousarray(iq, dtype=(np.complex64, np.int16, np.int8)[sample_format])


def carrier_scan(iq, rate_in, with_metric=False, cap=64, device=0, sample_format=FILE_CF32, **kw):
    """lsn_carrier_scan: every LTE carrier in the head of a recording made at rate_in, given nothing else.  iq: [sample][antenna] (or [sample]) numpy complex64, or
    int16 / int8 with a last axis of 2 for FILE_SC16 / FILE_SC8; iq[0] is sample 0 of the recording; it must hold carrier_scan_plan(...)["nof_input_samples"].
    -> [Carrier (center_offset_hz, k, scan_p2avg, scan_root, scan_lag, search: CellSearch on the carrier's 1.92 MS/s channel)] in the order of acceptance
    [, the CarrierMetric of every hypothesis].  kw: carrier_scan_cfg (antenna: an index or "all", nof_periods, raster_hz, raster_offset_hz, f_lo_hz, f_hi_hz, min_spacing_hz, threshold)"""
    iq = _scan_input(iq, sample_format)
    cfg = carrier_scan_cfg(rate_in, nof_antennas=iq.shape[1], sample_format=sample_format, **kw)
    carriers = (Carrier * cap)()
    metric = (CarrierMetric * SCAN_MAX_HYPOTHESES)() if with_metric else None
    n = _check_n(lib().lsn_carrier_scan(device, iq.ctypes.data, 0, iq.shape[0], C.byref(cfg), carriers, cap, metric), "lsn_carrier_scan")
    nhyp = 0
    if with_metric:
        pl = CarrierScanPlan()
        _check(lib().lsn_carrier_scan_plan(C.byref(cfg), C.byref(pl), None, 0, None), "lsn_carrier_scan_plan")
        nhyp = int(pl.nof_hypotheses)
    return _scan_result(n, carriers, metric, nhyp, with_metric)


def file_carrier_scan(path, rate_in, nof_antennas=1, sample_format=FILE_CF32, sample_scale=0.0, offset_time=0, with_metric=False, cap=64, device=0, **kw):
    """lsn_file_carrier_scan: carrier_scan on a recording, of which only the head the scan needs is read, from sample offset_time on"""
    cfg = carrier_scan_cfg(rate_in, nof_antennas=nof_antennas, sample_format=sample_format, sample_scale=sample_scale, **kw)
    fc = FileCfg(int(nof_antennas), int(offset_time), 0.0, int(sample_format), float(sample_scale))
    carriers = (Carrier * cap)()
    metric = (CarrierMetric * SCAN_MAX_HYPOTHESES)() if with_metric else None
    n = _check_n(lib().lsn_file_carrier_scan(device, os.fsencode(path), C.byref(fc), C.byref(cfg), carriers, cap, metric), "lsn_file_carrier_scan")
    nhyp = 0
    if with_metric:
        pl = CarrierScanPlan()
        _check(lib().lsn_carrier_scan_plan(C.byref(cfg), C.byref(pl), None, 0, None), "lsn_carrier_scan_plan")
        nhyp = int(pl.nof_hypotheses)
    return _scan_result(n, carriers, metric, nhyp, with_metric)


def _channel_cfg(nof_antennas, rate_in, center_offset_hz, first_sample, first_frac, in_base, out_first, sample_format, sample_scale):
    return CarrierChannelCfg(C.sizeof(CarrierChannelCfg), int(nof_antennas), int(sample_format), float(sample_scale), float(rate_in), float(center_offset_hz),
                             int(first_sample), float(first_frac), int(in_base), int(out_first))


def carrier_channel_span(n_out, in_end, rate_in, first_sample=0, first_frac=0.0, out_first=0, center_offset_hz=0.0):
    """lsn_carrier_channel_span -> dict(in_lo, in_hi, max_out, taps), as resample_span for the 1.92 MS/s channel of a carrier"""
    cfg = _channel_cfg(1, rate_in, center_offset_hz, first_sample, first_frac, 0, out_first, FILE_CF32, 0.0)
    sp = ResampleSpan()
    _check(lib().lsn_carrier_channel_span(C.byref(cfg), int(n_out), int(in_end), C.byref(sp)), "lsn_carrier_channel_span")
    return dict(in_lo=int(sp.in_lo), in_hi=int(sp.in_hi), max_out=int(sp.max_out), taps=int(sp.taps))


def carrier_channel(iq, rate_in, center_offset_hz, n_out=None, first_sample=0, first_frac=0.0, in_base=0, out_first=0, sample_format=FILE_CF32, sample_scale=0.0,
                    device=0):
    """lsn_carrier_channel: the 1.92 MS/s channel (the centre six resource blocks) of the carrier center_offset_hz off the centre of a recording made at rate_in,
    all antennas -> complex64 [antenna][n_out]; with first_sample = 0 and first_frac = 0 the samples the scan correlated, bit for bit.  iq and the other
    arguments as resample"""
    iq = _scan_input(iq, sample_format)
    n_in, nant = iq.shape[0], iq.shape[1]
    cfg = _channel_cfg(nant, rate_in, center_offset_hz, first_sample, first_frac, in_base, out_first, sample_format, sample_scale)
    if n_out is None:
        sp = ResampleSpan()
        _check(lib().lsn_carrier_channel_span(C.byref(cfg), 0, int(in_base) + n_in, C.byref(sp)), "lsn_carrier_channel_span")
        n_out = int(sp.max_out)
    out = np.zeros((nant, n_out), dtype=np.complex64)
    _check(lib().lsn_carrier_channel(device, iq.ctypes.data, 0, n_in, C.byref(cfg), out.ctypes.data, 0, n_out), "lsn_carrier_channel")
    return out


def carrier_cells(head, sample_rate, carrier_hz, antenna=0, sample_format=FILE_CF32, sample_scale=0.0, device=0, **kw):
    """every cell of one carrier of a wideband recording's head: carrier_channel (the 1.92 MS/s channel of the carrier carrier_hz off the centre) followed by
    cell_search_all at 6 resource blocks on one antenna of it; kw: cell_search_all's.  pss_pos and sf_start count samples of the 1.92 MS/s channel, as
    CarrierResult.search's do.  carrier_scan itself reports one cell per carrier."""
    ch = carrier_channel(head, sample_rate, carrier_hz, sample_format=sample_format, sample_scale=sample_scale, device=device)
    return cell_search_all(ch[int(antenna)], 6, device=device, **kw)


def carrier_mib(channel, search, max_batch=1, device=0):
    """the MIB of a carrier the scan found, from public calls only: subframe 0 is cut out of the carrier's channel (carrier_channel: [antenna][n] at 1.92 MS/s)
    at the search's sf_start / sf_idx, a six-block Phy is set to the search's cell id and CP and decodes the PBCH - with 1, 2 and 4 ports in turn until the
    MIB's own nof_ports agrees.  A six-block Phy decodes the PBCH of a cell of any bandwidth: the CRS sequence is indexed from the largest bandwidth and the
    centre 72 sub-carriers start at a multiple of 6 in it.  -> the dict of Phy.mib_decode (found, nof_prb, nof_ports, sfn, ...) or None"""
    channel = np.ascontiguousarray(channel, dtype=np.complex64)
    if channel.ndim == 1:
        channel = channel.reshape(1, -1)
    sflen = 1920
    start = int(search.sf_start) + (0 if int(search.sf_idx) == 0 else 5 * sflen)
    starts = [s for s in range(start % (10 * sflen), channel.shape[1] - sflen + 1, 10 * sflen)]
    for ports in (1, 2, 4):
        phy = Phy(nof_rx_antennas=channel.shape[0], max_batch=max_batch, device=device, pcapwriter=PcapWriter(None))
        try:
            if not phy.setCell(6, ports, int(search.cell_id), cp=int(search.cp)):
                continue
            for s in starts:
                m = phy.mib_decode(channel[:, s:s + sflen])
                if m["found"] and m["nof_ports"] == ports:
                    return m
        finally:
            phy.close()
    return None


def mac_lte_record(ctx, pdu):
    """MAC-LTE (DLT 147) framing of one PDU exactly as LTESniffer_pcap_writer::pack_and_write emits it
    (/root/reference/src/src/PcapWriter.cc:93-118; byte layout SURVEY.md appendix B). -> context header + PDU bytes."""
    tti = ctx["tti"]
    fs = ((tti // 10) << 4) | (tti % 10)
    hdr = bytes([1, ctx["direction"], ctx["rnti_type"], 2, ctx["rnti"] >> 8, ctx["rnti"] & 255, 3, 0, 0, 4, (fs >> 8) & 255,
                 fs & 255, 7, ctx["crc_ok"], 10, 0, 15, 0, 1])
    return hdr + pdu


def write_pcap(path, records, ts=(0, 0)):
    """records: iterable of (ctx, pdu). Writes the same global header as the reference (network 147)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, 65535, 147))
        for ctx, pdu in records:
            body = mac_lte_record(ctx, pdu)
            f.write(struct.pack("<IIII", ts[0], ts[1], len(body), len(body)) + body)
