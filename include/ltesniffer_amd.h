/*
 * ltesniffer_amd.h - C ABI of the MI355X-native LTESniffer per-subframe worker (the drop-in boundary).
 *
 * Everything behind LTESniffer's Phy / SubframeWorker pair is replaced by this library:
 *   class Phy            /root/reference/src/include/Phy.h:22-66
 *   class SubframeWorker /root/reference/src/include/SubframeWorker.h:16-86
 * The caller (LTESniffer_Core::run, /root/reference/src/src/LTESniffer_Core.cc:292-299,365,434-451,547)
 * keeps filling antenna buffers and calling prepare/putPending; decoded MAC PDUs come back through a sink
 * callback that carries exactly the fields LTESniffer_pcap_writer::pack_and_write serialises
 * (/root/reference/src/src/PcapWriter.cc:93-118), in (tti, DCI acceptance order, TB) order.
 *
 * Plain C: pointers + sizes, int return codes (0 ok, <0 error: same convention as SRSRAN_SUCCESS / SRSRAN_ERROR /
 * SRSRAN_ERROR_INVALID_INPUTS), no exceptions cross the boundary.  The library REQUIRES a HIP device; there is no
 * CPU fallback: lsn_phy_create fails with LSN_ERROR_NO_DEVICE when none is visible.
 */
#ifndef LTESNIFFER_AMD_H
#define LTESNIFFER_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LSN_SUCCESS 0
#define LSN_ERROR (-1)
#define LSN_ERROR_INVALID_INPUTS (-2)
#define LSN_ERROR_NO_DEVICE (-3)

typedef struct lsn_phy lsn_phy_t;       /* replaces class Phy (Phy.h:22) */
typedef struct lsn_worker lsn_worker_t; /* replaces class SubframeWorker (SubframeWorker.h:16) */

/* srsran_cell_t subset that crosses the boundary (SubframeWorker::setCell, SubframeWorker.cc:100-107) */
typedef struct {
  uint32_t nof_prb;         /* 6, 15, 25, 50, 75, 100 */
  uint32_t nof_ports;       /* 1, 2 or 4 CRS ports (4: transmit diversity on every channel; spatial-multiplexing grants are found and not decoded, as with the reference's srsRAN) */
  uint32_t id;              /* physical cell id */
  uint32_t cp;              /* 0 = normal, 1 = extended cyclic prefix (6 symbols per slot; DL mode and UL_MODE; lsn_cell_search reports it) */
  uint32_t phich_length;    /* 0 = normal */
  uint32_t phich_resources; /* 0: 1/6, 1: 1/2, 2: 1, 3: 2 (LTESniffer_Core.cc:211-212 forces 1/6) */
  uint32_t frame_type;      /* 0 = FDD */
} lsn_cell_t;

/* srsran_dl_sf_cfg_t subset passed by SubframeWorker::prepare (SubframeWorker.cc:109-116, LTESniffer_Core.cc:429-434) */
typedef struct {
  uint32_t tti;
  uint32_t cfi;     /* ignored on input: decoded from PCFICH per subframe */
  uint32_t sf_type; /* 0 = SRSRAN_SF_NORM */
} lsn_dl_sf_cfg_t;

/* Constructor arguments of Phy::Phy (Phy.h:24-36) that influence the hot path */
typedef struct {
  uint32_t nof_rx_antennas;
  uint32_t nof_workers;             /* worker (buffer) pool size; Phy.h:19 uses 20 */
  uint32_t max_batch;               /* subframes processed per GPU batch (0 = default 64) */
  int skip_secondary_meta_formats;  /* Phy ctor skipSecondaryMetaFormats */
  double meta_format_split_ratio;   /* Settings.h:55, default 0.99 */
  uint32_t histogram_threshold;     /* Settings.h:57, default 5 */
  int mcs_tracking_mode;            /* ArgManager.cc:52, default 1 */
  int harq_mode;                    /* 0 (ArgManager.cc:50: the reference's only reachable value) or 1: DL HARQ soft combining (HARQ.cc:71-190,
                                       DL_Sniffer_PDSCH.cc:943-1020) for known-table C-RNTI grants; DL mode.  With lsn_phy_create_multi the soft-buffer pool lives on the
                                       first device and the other engines need peer access to it (the call fails otherwise) */
  int device;                       /* HIP device ordinal */
  int max_turbo_iterations;         /* SubframeWorker.cc:365, default 12 (0 = default) */
  int sniffer_mode;                 /* 0 = DL_MODE, 1 = UL_MODE (SubframeWorker.cc:166-199): antenna 0 = downlink, antenna 1 = uplink,
                                       nof_rx_antennas must be 2; the uplink configuration comes from lsn_phy_set_ul_config (+ lsn_phy_set_prach_config)
                                       or, when those are not called, from the first SIB2 decoded (PDSCH_Decoder::decode_SIB) */
} lsn_phy_cfg_t;

/* What LTESniffer_pcap_writer::pack_and_write receives (PcapWriter.cc:93-111) */
typedef struct {
  uint32_t tti;       /* sfn*10 + sf */
  uint16_t rnti;      /* SI/P constants already substituted (PcapWriter.cc:162-170) */
  uint8_t direction;  /* 0 UL, 1 DL */
  uint8_t rnti_type;  /* 0 NO, 1 P, 2 RA, 3 C, 4 SI */
  uint8_t crc_ok;
  uint8_t is_retx;
  uint8_t tb;         /* transport block index within the DCI */
  uint8_t reserved;
} lsn_pdu_ctx_t;
typedef void (*lsn_pdu_sink_t)(void* user, const lsn_pdu_ctx_t* ctx, const uint8_t* pdu, uint32_t len);

/* DCIBlindSearchStats (PhyCommon.h:12-26) */
typedef struct {
  uint32_t nof_locations, nof_decoded_locations, nof_cce, nof_missed_cce, nof_subframes, nof_subframe_collisions_dw,
      nof_subframe_collisions_up;
} lsn_blind_stats_t;

/* ---- Phy ---- */
int lsn_phy_create(const lsn_phy_cfg_t* cfg, lsn_phy_t** out);          /* Phy::Phy, Phy.cc:5 */
void lsn_phy_destroy(lsn_phy_t* phy);                                     /* Phy::~Phy */
/* ONE capture spread over several GPUs of the node: a Phy whose chunks of max_batch subframes go round-robin to one
 * engine per listed device.  Stage A, the exhaustive candidate decode and the PDSCH decodes of a chunk run on its device; the sequential
 * host state (FALCON search / RNTI manager, MCS tracking, record order) is shared and taken in turns, so the record stream is the one a
 * single device produces.  IQ blocks that live on another device travel by peer copies (xGMI).  devices[0] is the primary device (MIB,
 * uplink, taps); listing a device twice is allowed (two engines on one GPU).  Supported entry points in this mode: lsn_phy_process_device,
 * lsn_phy_submit_device, lsn_phy_wait and the getters; DL_MODE and UL_MODE (the ULSchedule / uplink tracking databases and the uplink
 * configuration are part of the shared state; a SIB2 learnt by one engine reaches the device tables of the others at their next commit turn).
 * Several CELLS are several Phys - one process per GPU, no exchange. */
int lsn_phy_create_multi(const lsn_phy_cfg_t* cfg, const int* devices, uint32_t n_devices, lsn_phy_t** out);
uint32_t lsn_phy_nof_devices(lsn_phy_t* phy);
int lsn_phy_set_cell(lsn_phy_t* phy, const lsn_cell_t* cell);             /* Phy::setCell, Phy.cc:111 */
/* Sampling mode: how many samples one OFDM symbol of the IQ handed to this Phy has (sampling rate = 15 kHz x that number).
 *   LSN_RATES_3GPP (default): the TS 36.211 sizes        6 / 15 / 25 / 50 / 75 / 100 PRB -> 128 / 256 / 512 / 1024 / 1536 / 2048
 *   LSN_RATES_SRSRAN: srsran_symbol_sz of an srsRAN built without FORCE_STANDARD_RATE - what LTESniffer runs, records and hands to its
 *                     workers (LTESniffer_Core.cc:222-226,358,365)                       -> 128 / 256 / 384 /  768 / 1024 / 1536
 * Everything counted in samples follows: a subframe is 15 x symbol size samples (every process call, file blocks, offset_time_samples,
 * lsn_worker_buffer_len = 3 subframes).  Call it in front of lsn_phy_set_cell (handles of lsn_phy_create_multi included: all engines follow).
 * Once a cell is set the mode is fixed: asking for the other one, or for an unknown mode, is LSN_ERROR_INVALID_INPUTS (a capture at another
 * rate is another Phy). */
#define LSN_RATES_3GPP 0
#define LSN_RATES_SRSRAN 1
int lsn_phy_set_sampling(lsn_phy_t* phy, int rates);
int lsn_phy_get_sampling(lsn_phy_t* phy);
uint32_t lsn_symbol_sz(uint32_t nof_prb, int rates);         /* srsran_symbol_sz; 0 for a bandwidth or mode that does not exist */
uint32_t lsn_sampling_freq_hz(uint32_t nof_prb, int rates);  /* srsran_sampling_freq_hz: 15000 x lsn_symbol_sz */
lsn_worker_t* lsn_phy_get_avail(lsn_phy_t* phy, int blocking);            /* Phy::getAvail / getAvailImmediate, Phy.cc:79-89 */
int lsn_phy_put_pending(lsn_phy_t* phy, lsn_worker_t* w);                 /* Phy::putPending, Phy.cc:95 */
int lsn_phy_join_pending(lsn_phy_t* phy);                                 /* Phy::joinPending, Phy.cc:100 */
int lsn_phy_set_pdu_sink(lsn_phy_t* phy, lsn_pdu_sink_t cb, void* user);  /* stands in for the pcapwriter ctor argument */
int lsn_phy_get_stats(lsn_phy_t* phy, lsn_blind_stats_t* out);            /* PhyCommon::getStats, PhyCommon.cc:60 */
float lsn_phy_get_est_cfo(lsn_phy_t* phy);                                /* SubframeWorker.cc:203 est_cfo */
/* CFO correction inside the OFDM kernel (an NCO on the samples as the FFT loads them).  Replaces, for this path, what srsran_ue_sync does to the samples before
 * they reach SubframeWorker::work: ue_sync.cfo_correct_enable_track = !args.disable_cfo (LTESniffer_Core.cc:344), started from the cell search's offset
 * (ue_sync.cfo_current_value = search_cell_cfo / 15000, :312-316) and kept on the carrier by srsran_ue_sync_set_cfo_ref with the CRS estimate.
 *   mode 0: off (the reference's file replay without -o)          mode 1: remove the fixed offset cfo_hz          mode 2: track - start from cfo_hz, then
 *   each chunk of max_batch subframes is corrected by c += alpha * (m - c), m = the absolute offset (correction + mean CRS residual) measured on the chunk
 *   LSN_NSTREAM_A (4) chunks earlier; 0 < alpha <= 1.  est_cfo keeps reporting the CRS estimate of the corrected samples (the residual), as in the reference.
 * Takes effect with the next chunk that enters the pipeline; call it between process calls.  mode 2 is refused on a handle of lsn_phy_create_multi. */
int lsn_phy_set_cfo_correction(lsn_phy_t* phy, int mode, float cfo_hz, float alpha);
float lsn_phy_get_cfo_correction(lsn_phy_t* phy);                         /* the offset removed from the chunk launched last (srsran_ue_sync_get_cfo) */
/* Blind DCI decoding (srsran_pdcch_decode_msg_limit_avg_llr_power per location and format, falcon_pdcch.c:110-170; DCISearch.cc:102-447): which (location, size)
 * slots of a subframe's candidate table the GPU decodes ahead of the sequential search.
 *   mode 0: all of them (rounds 1-5)
 *   mode 1 (default): the aggregation levels in four launches, 8 -> 1 CCEs; a slot under a location that holds a candidate the search is predicted to accept (its own
 *           stateless tests + the RNTI evergreen, or active in the newest published snapshot of the RNTI manager and not forbidden) is left out, and decoded
 *           on demand if the search comes there after all (lsn_perf_t.nof_candidate_misses) - the table the search sees is the exhaustive one
 *   mode 2: test - every RNTI counts as active, so that the on-demand path carries the search
 * Takes effect with the next chunk that enters the pipeline. */
int lsn_phy_set_candidate_pruning(lsn_phy_t* phy, int mode);
int lsn_phy_add_evergreen(lsn_phy_t* phy, uint16_t rnti_start, uint16_t rnti_end, uint32_t format_idx); /* RNTIManager::addEvergreen */
int lsn_phy_add_forbidden(lsn_phy_t* phy, uint16_t rnti_start, uint16_t rnti_end, uint32_t format_idx); /* RNTIManager::addForbidden */
int lsn_phy_setup_default_rnti_intervals(lsn_phy_t* phy);                 /* LTESniffer_Core.cc:398-417 in one call */
uint32_t lsn_phy_nof_active_rnti(lsn_phy_t* phy);
/* Phy::getMetaFormats (Phy.h:45, Phy.cc:152; DCIMetaFormats, MetaFormats.h): the primary / secondary split of the nine DCI formats the search is working with,
 * as indices into falcon_ue_all_formats (DCISearch.cc:84-95; = srsran_dci_format_t values 0..8).  Each list has room for 9.  Between process calls / after wait. */
int lsn_phy_get_meta_formats(lsn_phy_t* phy, uint32_t* primary, uint32_t* nof_primary, uint32_t* secondary, uint32_t* nof_secondary);
/* Phy::getWorkers (Phy.h:46, Phy.cc:112): the pool's workers by index, whoever holds them at the moment */
uint32_t lsn_phy_nof_workers(lsn_phy_t* phy);
lsn_worker_t* lsn_phy_worker(lsn_phy_t* phy, uint32_t index);
/* UE-specific configuration learned from RRCConnectionSetup messages on the downlink (MCSTracking::get_ue_config_rnti,
 * MCSTracking.cc:1482-1516; filled by PDSCH_Decoder::decode_rrc_connection_setup, DL_Sniffer_PDSCH.cc:129-181): the entry of the
 * RNTI, or the default (the first connection setup seen; before that p_a 0 dB, offsets 10 / 8 / 11, higher-layer sub-band CQI).
 * p_a_db is the PDSCH power offset every later decode of that RNTI runs with (DL_Sniffer_PDSCH.cc:926-927). */
typedef struct {
  uint32_t has_ue_config;                           /* 1: from this UE's own connection setup */
  float p_a_db;
  uint32_t i_offset_ack, i_offset_cqi, i_offset_ri; /* betaOffset-ACK / CQI / RI-Index */
  uint32_t cqi_type;                                /* 0 wideband, 1 UE-selected sub-band, 2 higher-layer sub-band (srsran_cqi_type_t) */
} lsn_ue_config_t;
int lsn_phy_get_ue_config(lsn_phy_t* phy, uint16_t rnti, lsn_ue_config_t* out);
/* PhyCommon::setShortcutDiscovery (PhyCommon.cc:69-71; LTESniffer_Core.cc:87,616): the parent/child shortcut of the recursive blind
 * search (DCISearch.cc:200-211).  Default on, like ArgManager.cc:47. */
int lsn_phy_set_shortcut_discovery(lsn_phy_t* phy, int enable);
int lsn_phy_get_shortcut_discovery(lsn_phy_t* phy);
/* RNTIManager::setHistogramThreshold (RNTIManager.cc:442-444; LTESniffer_Core.cc:620) */
int lsn_phy_set_histogram_threshold(lsn_phy_t* phy, uint32_t threshold);
/* PhyCommon::printStats -> DCIBlindSearchStats::print (PhyCommon.cc:65-67,102-114; LTESniffer_Core.cc:561): the two CSV lines of the
 * reference's stats file; `file` is a FILE* (NULL: stdout).  The blind-search time column is the search thread's time. */
int lsn_phy_print_stats(lsn_phy_t* phy, void* file);
/* MCSTracking database ageing (MCSTracking::update_database_dl, MCSTracking.cc:850-927, driven every get_interval() x 1000 subframes
 * by LTESniffer_Core.cc:473-499).  The library ages its database by itself on the SUBFRAME count of the stream it commits (one subframe
 * = 1 ms; the reference uses clock(), i.e. replay speed): interval in seconds, 0 = never, default 5 (MCSTracking.h:162).
 * lsn_phy_update_mcs_database runs one update now (between process calls), for callers that keep the reference's own timer. */
int lsn_phy_set_mcs_update_interval(lsn_phy_t* phy, uint32_t seconds);
int lsn_phy_update_mcs_database(lsn_phy_t* phy);
uint32_t lsn_phy_nof_tracked_rnti(lsn_phy_t* phy);   /* MCSTracking::nof_RNTI_member_dl; in UL_MODE nof_RNTI_member_ul (the uplink database is aged the
                                                         same way: update_database_ul, MCSTracking.cc:86-176, fed by update_statistic_ul :729-754) */
int lsn_phy_tracked_ul_modulation(lsn_phy_t* phy, uint16_t rnti); /* UL_MODE: 0 no entry, 1 unknown, 2 / 3 / 4 = 16 / 64 / 256QAM maximum (find_tracking_info_RNTI_ul without the time stamp) */

/* ---- SubframeWorker ---- */
float** lsn_worker_buffers(lsn_worker_t* w);         /* SubframeWorker::getBuffers: [antenna] -> interleaved cf32, pinned host */
float** lsn_worker_buffers_offset(lsn_worker_t* w);  /* SubframeWorker::getBuffers_offset (SubframeWorker.h:37): the two 3 * SF_LEN scratch buffers of SubframeBuffer.cc:28 */
uint32_t lsn_worker_buffer_len(lsn_worker_t* w);     /* complex samples per antenna buffer (3 * SF_LEN, SubframeBuffer.cc:25) */
int lsn_worker_prepare(lsn_worker_t* w, uint32_t sf_idx, uint32_t sfn, int update_meta_formats, const lsn_dl_sf_cfg_t* sf); /* SubframeWorker::prepare */
uint32_t lsn_worker_sf_idx(lsn_worker_t* w);
uint32_t lsn_worker_sfn(lsn_worker_t* w);

/* ---- MAC-LTE pcap writer: replaces LTESniffer_pcap_writer (PcapWriter.h:39-51, PcapWriter.cc:75-118) ----
 * Record layout = LTE_PCAP_MAC_WritePDU [srsRAN], pinned by the captures under /root/reference/pcap_file_example/ (DLT 147). */
typedef struct lsn_pcap lsn_pcap_t;
lsn_pcap_t* lsn_pcap_open(const char* path);                 /* LTESniffer_pcap_writer::open, PcapWriter.cc:75 */
lsn_pcap_t* lsn_pcap_open_mem(void);                         /* in-memory capture with zero timestamps (tests, bench) */
void lsn_pcap_set_wall_clock(lsn_pcap_t* p, int on);         /* record timestamps: gettimeofday (default for files) or 0 */
int lsn_pcap_write(lsn_pcap_t* p, const lsn_pdu_ctx_t* ctx, const uint8_t* pdu, uint32_t len); /* pack_and_write, PcapWriter.cc:93 */
void lsn_pcap_sink(void* user /* lsn_pcap_t* */, const lsn_pdu_ctx_t* ctx, const uint8_t* pdu, uint32_t len); /* an lsn_pdu_sink_t */
const uint8_t* lsn_pcap_mem(lsn_pcap_t* p, size_t* len);
uint32_t lsn_pcap_nof_records(lsn_pcap_t* p);
void lsn_pcap_reset(lsn_pcap_t* p);
/* order-sensitive 64-bit digest + byte count of all records since open / reset, timestamps excluded (two writers fed the same record
 * sequence agree); lsn_pcap_set_store(p, 0) keeps only the count and the digest (long streams that need not be kept) */
int lsn_pcap_digest(lsn_pcap_t* p, uint64_t* digest, uint64_t* nbytes);
void lsn_pcap_set_store(lsn_pcap_t* p, int on);
/* Piecewise digests: the record stream is cut every `subframes_per_block` subframes counted from `origin_tti` (the TTI of the records
 * is unwrapped modulo 10240 in arrival order); each block has its own digest chain and record count, so a long replay can be checked
 * block by block against a reference produced elsewhere.  0 switches the blocks off; lsn_pcap_reset clears them. */
void lsn_pcap_set_digest_blocks(lsn_pcap_t* p, uint32_t subframes_per_block, uint32_t origin_tti);
uint32_t lsn_pcap_block_digests(lsn_pcap_t* p, uint64_t* digests, uint32_t* nof_records, uint32_t cap); /* -> number of blocks */
void lsn_pcap_close(lsn_pcap_t* p);                          /* LTESniffer_pcap_writer::close */
int lsn_phy_set_pcap_writer(lsn_phy_t* phy, lsn_pcap_t* p);  /* Phy ctor argument `LTESniffer_pcap_writer*` (Phy.h:31) */

/* ---- resident (offline / file-replay) path: the IQ of n subframes is ALREADY in device memory ----
 * d_iq layout: [subframe][antenna][15*N] interleaved cf32 (N = FFT size). Subframe i has tti = start_tti + i.
 * update_meta_period: metaFormats.update_formats() runs when (sf_cnt % period) == 0 (LTESniffer_Core.cc:434), 0 = never.
 * stream: a hipStream_t (may be NULL for the default stream). Blocks until all PDUs of the batch have been delivered. */
int lsn_phy_process_device(lsn_phy_t* phy, const void* d_iq, uint32_t n_subframes, uint32_t start_tti,
                           uint32_t update_meta_period, void* stream);
/* same, from host memory (copies through pinned staging) */
int lsn_phy_process_host(lsn_phy_t* phy, const float* iq, uint32_t n_subframes, uint32_t start_tti, uint32_t update_meta_period);
/* same, for INTEGER samples as a radio driver delivers them when asked not to convert (UHD cpu format sc16 / sc8; the reference asks srsran_rf for cf_t,
 * LTESniffer_Core.cc:156,591-600: srsran_rf_recv_with_time_multi into cf_t buffers, so this has no counterpart there): iq [subframe][antenna][15*N] pairs of int16 (LSN_FILE_SC16) or int8 (LSN_FILE_SC8), I first;
 * sample = (float)integer * sample_scale (0 = full scale +-1), converted on the GPU behind the copy - half / a quarter of the bytes of lsn_phy_process_host
 * cross PCIe.  Formats and conversion are lsn_file_cfg_t's (below); LSN_FILE_CF32 is refused (that is lsn_phy_process_host). */
int lsn_phy_process_host_int(lsn_phy_t* phy, const void* iq, uint32_t sample_format, float sample_scale, uint32_t n_subframes, uint32_t start_tti,
                             uint32_t update_meta_period);
/* Pipelined form of lsn_phy_process_device: submit returns as soon as every subframe of the block has been searched and queued for
 * decoding, so the decode / commit tail of one block overlaps the front of the next; lsn_phy_wait returns when everything submitted
 * has been committed (PDUs delivered, in order).  The IQ buffer of a submit must stay valid until the next lsn_phy_wait.
 * lsn_phy_get_perf then describes the whole submit ... wait span.  process_device == submit + wait. */
int lsn_phy_submit_device(lsn_phy_t* phy, const void* d_iq, uint32_t n_subframes, uint32_t start_tti, uint32_t update_meta_period, void* hip_stream);
int lsn_phy_wait(lsn_phy_t* phy);

/* ---- PBCH / MIB ----
 * Replaces srsran_ue_mib_decode + srsran_pbch_mib_unpack of the reference's DECODE_MIB state (LTESniffer_Core.cc:382-395): decode
 * the MIB on a subframe 0 and return the SFN of that subframe (MIB SFN + position of the radio frame in the 40 ms BCH period,
 * "sfn = (sfn + sfn_offset) % 1024").  The cell (bandwidth, id, number of CRS ports for the channel estimate) must have been set;
 * nof_ports is what the CRC mask says (1 / 2 / 4).  Returns 1 = found, 0 = no MIB in this subframe, < 0 = error. */
typedef struct {
  uint32_t found;
  uint32_t sfn;                 /* SFN of the subframe that was handed in */
  uint32_t sfn_offset;          /* radio-frame position inside the BCH period, 0..3 */
  uint32_t nof_prb, nof_ports;  /* dl-Bandwidth, CRC mask */
  uint32_t phich_length;        /* 0 normal, 1 extended */
  uint32_t phich_resources_x6;  /* Ng * 6: 1, 3, 6, 12 */
  uint32_t mib_bits;            /* the 24 MIB bits, first bit = MSB */
} lsn_mib_t;
/* iq: ONE subframe, [nof_rx_antennas][15*N] cf32 (host memory unless iq_on_device) */
int lsn_phy_mib_decode(lsn_phy_t* phy, const void* iq, int iq_on_device, lsn_mib_t* out);
#define LSN_TTI_FROM_MIB 0xFFFFFFFFu /* start_tti of lsn_phy_process_file: take the SFN from the first MIB that decodes (subframes 0, 10, 20, ...
                                        of the file; the subframes in front of it are dropped, as in the reference's DECODE_MIB state) */

/* ---- PSS / SSS cell search ----
 * Replaces rf_search_and_decode_mib(&rf, nof_rx_ant, &cell_detect_config, force_N_id_2, &cell, &search_cell_cfo)
 * (LTESniffer_Core.cc:195-204, configuration :108-112) on a block of samples instead of a radio: physical cell id, the position
 * of the subframe-0/5 boundaries and the carrier offset - for a recording also the -O offset and -c cell id that the
 * reference's file mode asks the user for.  The MIB (bandwidth, ports, PHICH, SFN) then comes from lsn_phy_mib_decode.
 * Needs no Phy.  iq: one antenna, contiguous cf32 at the sampling rate of nof_prb (15 kHz * N), at least
 * (nof_periods + 1) * 75 * N + N samples.  FDD; the cyclic prefix is detected (out->cp).
 * Returns 1 when a cell was found (pss_p2avg >= threshold), 0 when not (out still holds the best guess), < 0 on error. */
typedef struct {
  uint32_t nof_periods;  /* 5 ms periods whose PSS correlation powers are added (1..16; 0 = 1) */
  int32_t force_n_id_2;  /* -1: search the three PSS roots (args.force_N_id_2 of the reference) */
  float threshold;       /* on peak / mean of the PSS correlation power; 20 is a safe floor (noise alone stays below 15; lower still over two antennas) */
} lsn_cell_search_cfg_t;
typedef struct {
  uint32_t found, cell_id, n_id_2, n_id_1;
  uint32_t sf_idx;    /* 0 or 5: index of the subframe that starts at sample sf_start */
  uint32_t pss_pos;   /* first sample of the useful part of the PSS symbol, 0 <= pss_pos < 75 N */
  uint32_t sf_start;  /* 0 <= sf_start < 75 N: lsn_file_cfg_t.offset_time_samples for a recording */
  float pss_peak, pss_p2avg;
  float sss_metric, sss_second;  /* best and second best of the 336 SSS hypotheses */
  float cfo_hz;                  /* from the phase turn between the SSS and PSS symbols (+-7 kHz) */
  float cfo_coarse_hz;           /* from the two halves of the PSS symbol (+-15 kHz; disturbed by the other carriers of a loaded cell) */
  uint32_t cp;                   /* 0 normal, 1 extended cyclic prefix (lsn_cell_t.cp): which of the two SSS positions in front of the PSS symbol carried the better SSS */
} lsn_cell_search_t;
int lsn_cell_search(int device, const void* iq, int iq_on_device, uint64_t nof_samples, uint32_t nof_prb, const lsn_cell_search_cfg_t* cfg,
                    lsn_cell_search_t* out, float* corr_out /* optional, host: [3][75 N] accumulated PSS correlation powers */);
/* the same on samples at the rate of sampling mode `rates` (LSN_RATES_*): N = lsn_symbol_sz(nof_prb, rates); pss_pos and sf_start count samples of that rate */
int lsn_cell_search_rates(int device, const void* iq, int iq_on_device, uint64_t nof_samples, uint32_t nof_prb, int rates, const lsn_cell_search_cfg_t* cfg,
                          lsn_cell_search_t* out, float* corr_out);

/* ---- the cell search over all receive antennas ----
 * lsn_cell_search_rates on nof_antennas antennas of one recording, antenna a at iq + a * ant_stride samples (cf32; [antenna][sample] with ant_stride >= nof_samples,
 * nof_samples per antenna).  The antennas are combined without their phases, per antenna and per 5 ms period - their channels are independent, and samples added
 * before the matched filter cancel a cell whose channels are opposite:
 *   timing   C[r][n] = sum over periods q and antennas a of |<p_r, x_a[q 75 N + n ...]>|^2 / E_a(q, n) (k_pss_corr_ant); peak, mean and pss_p2avg from C by
 *            lsn_cell_search's rule, the threshold is the caller's (noise alone reaches lower with two antennas than with one).
 *   SSS      per antenna and cyclic-prefix hypothesis at the common lag (k_sync_fin); M[h] = sum_a |hyp_a[h_a]|^2, h_a = h with the subframe 0 / 5 bit swapped when
 *            that antenna's occurrence is odd, so every antenna votes in the parity of the first occurrence; the CP with the larger best M (normal on a tie);
 *            sss_metric / sss_second from M; cfo_hz from the angle of sum_a hyp_a[best], cfo_coarse_hz from that of sum_a conj(y0_a) y1_a; sf_start and sf_idx by
 *            lsn_cell_search's formulas.
 * per_ant (optional, [nof_antennas]): what each antenna alone holds at the common lag, under the winning CP hypothesis - which antenna carried the decision.
 * With nof_antennas = 1 every field of out and corr_out are lsn_cell_search_rates' (==).  nof_antennas 0 or > LSN_SEARCH_MAX_ANTENNAS, ant_stride < nof_samples,
 * too few samples, an unknown bandwidth or mode, nof_periods > 16: LSN_ERROR_INVALID_INPUTS, before the device is looked at.  Return value as lsn_cell_search. */
#define LSN_SEARCH_MAX_ANTENNAS 2 /* the Phy's antenna limit */
typedef struct {
  float pss_peak;                /* this antenna's own sum over the periods at (n_id_2, pss_pos): the antennas' values add up to lsn_cell_search_t.pss_peak */
  float sss_metric, sss_second;  /* best and second best of its own 336 hypothesis powers */
  float cfo_hz;                  /* from its own best hypothesis */
  uint32_t n_id_1;               /* of its own best hypothesis */
  uint32_t occurrence;           /* the PSS occurrence its SSS was taken from (sample pss_pos + occurrence * 75 N) */
} lsn_cell_search_ant_t;
int lsn_cell_search_ant(int device, const void* iq, int iq_on_device, uint64_t nof_samples /* per antenna */, uint64_t ant_stride /* samples */, uint32_t nof_antennas,
                        uint32_t nof_prb, int rates, const lsn_cell_search_cfg_t* cfg, lsn_cell_search_t* out, lsn_cell_search_ant_t* per_ant /* optional */,
                        float* corr_out /* optional, host: [3][75 N] */);

/* ---- every cell of a carrier: successive cell search ----
 * lsn_cell_search reports the strongest cell.  A network reuses one frequency in all its cells, so a receiver hears several on each carrier: the sectors of
 * a site share their timing and differ in N_id_2, other sites arrive at other timings.  lsn_cell_search_all finds them one after the other on a device copy
 * of the samples (the caller's buffer is never written):
 *   round 0      lsn_cell_search's decision on the untouched samples - every field of cell 0 is what lsn_cell_search returns for the same input and
 *                configuration; no cell at all when its found is 0.
 *   every round  the SSS decision is repeated robustly at the round's peak: the 336 hypothesis powers are added over ALL occurrences whose SSS symbol lies
 *                in the buffer (subframe 0 / 5 swapped on odd occurrences), with the channel from the PSS averaged over +-2 carriers inside each half of
 *                the band.  sss_ratio = best / second accumulated power of the winning cyclic-prefix hypothesis.
 *   rounds >= 1  accept the peak when peak / mean(root) >= threshold_next AND sss_ratio >= sss_ratio_min AND the cell is not one already reported; cell id, CP,
 *                sf_start, sf_idx and the carrier offsets come from the accumulated decision by lsn_cell_search's formulas.  The search stops at the first
 *                round that accepts nothing, or at max_cells.
 *   shared PSS   two cells with the same root at the same timing are one PSS peak: the runner-up hypothesis of a round (another N_id_1 than the best) is
 *                reported as a cell of its own, shared_pss = 1 and the round's timing, when its accumulated power is >= shared_pss_ratio x the best.
 *   cancellation after an accepted round the cell's PSS is taken out of the working copy, one complex gain per occurrence (lsn_pss_cancel), and the
 *                correlation is recomputed only where samples changed: the lags |n - pss_pos| < N (mod 75 N), lsn_cell_search_all_plan.
 * threshold_next = 8 was measured for 8 periods (the floor after a cancellation stays below 4.7); with fewer periods noise alone reaches
 * higher (10.2 at 2 periods) and the threshold must be raised.  Cells more than about 6 dB below the strongest are not reported reliably.  FDD, one antenna.
 * Same input as lsn_cell_search_rates.  Returns the number of cells found (0..max_cells), < 0 on error. */
typedef struct {
  uint32_t nof_periods;    /* 1..16, 0 = 8 */
  int32_t  force_n_id_2;   /* -1: the three roots */
  float threshold;         /* round 0, as lsn_cell_search_cfg_t.threshold */
  float threshold_next;    /* rounds >= 1 on peak / mean; 0 = 8 */
  float sss_ratio_min;     /* rounds >= 1 on best / second accumulated SSS power; 0 = 1.5 */
  float shared_pss_ratio;  /* 0 = 0.6; < 0: no second cell from one PSS peak */
  uint32_t max_cells;      /* 1..8, 0 = 8 */
} lsn_cell_search_all_cfg_t;
#define LSN_SEARCH_MAX_CELLS 8
typedef struct {
  lsn_cell_search_t cell;
  uint32_t round;          /* the round that found it */
  uint32_t shared_pss;     /* 1: the runner-up of its round (same root, same timing as the cell before it) */
  float sss_ratio;         /* best / second accumulated SSS power of its round */
  float rel_power_db;      /* mean |a_j|^2 of its cancellation against cell 0's (a shared-PSS cell: its round's, scaled by runner-up / best power) */
} lsn_cell_found_t;
int lsn_cell_search_all(int device, const void* iq, int iq_on_device, uint64_t nof_samples, uint32_t nof_prb, int rates, const lsn_cell_search_all_cfg_t* cfg,
                        lsn_cell_found_t* out /* [max_cells] */, uint32_t* nof_found, float* corr_out /* optional, host: [rounds run][3][75 N] */);
/* corr_out: room for max_cells + 1 rounds.  Rounds run: 1 when nothing was found; else the last found cell's round + 2 when the search ended on a round that
 * accepted nothing, + 1 when max_cells ended it (the correlation after the last cancellation is then not formed). */
/* the cancellation alone: iq (host, (nof_periods + 1) 75 N + N samples at least) -> residual (host, as many samples as iq) and a [nof_periods + 1][2]:
 * a_j = sum_k conj(p[k]) iq[pss_pos + j 75 N + k], residual = iq - a_j p at each occurrence; p: lsn_clock_replica's (unit energy, rotated by cfo_hz) */
int lsn_pss_cancel(int device, const void* iq, uint64_t nof_samples, uint32_t nof_prb, int rates, uint32_t nof_periods, uint32_t n_id_2, uint32_t pss_pos,
                   float cfo_hz, void* residual, float* a_out);
/* the accumulated SSS decision's raw numbers at a lag (no search): sums [2 CP][nof_periods + 1][336][2] coherent sums (0 where the SSS symbol is outside
 * the buffer), valid [2][nof_periods + 1], halves [nof_periods + 1][2][3] (re, im, energy of the PSS matched-filter halves), acc [2][336] powers */
int lsn_sss_accumulate(int device, const void* iq, uint64_t nof_samples, uint32_t nof_prb, int rates, uint32_t nof_periods, uint32_t n_id_2, uint32_t pss_pos,
                       float* sums, uint32_t* valid, float* halves, float* acc);
/* No GPU.  The lags a cancellation at pss_pos changes: n_lag = 2 N - 1 lags from n_lo on, modulo W5 = 75 N; as runs of consecutive lags: one, or two when
 * the window wraps at W5 (the run that starts at 0 comes second). */
typedef struct {
  uint32_t n_lo, n_lag;
  uint32_t nof_runs;
  uint32_t run_lo[2], run_len[2];
} lsn_cell_search_all_plan_t;
int lsn_cell_search_all_plan(uint32_t pss_pos, uint32_t N, uint32_t W5, lsn_cell_search_all_plan_t* out);
/* No GPU.  The rule of one round on its statistics: peak and sum of the winning root's correlation over W5 lags, acc [2 CP][336] accumulated powers. */
typedef struct {
  uint32_t accept;         /* round 0: p2avg >= threshold; rounds >= 1: both tests above */
  uint32_t cp;             /* winning cyclic-prefix hypothesis: the larger best power, normal on a tie */
  uint32_t best, second;   /* hypotheses h = 2 N_id_1 + (subframe 5 at occurrence 0): first maximum and second largest power */
  uint32_t shared;         /* 1: runner_up is a cell of its own when the round is accepted */
  uint32_t runner_up;      /* largest power among the hypotheses of another N_id_1 than best's */
  float p2avg, sss_ratio;
  float best_power, second_power, runner_up_power;
} lsn_cell_search_all_decision_t;
int lsn_cell_search_all_decide(const lsn_cell_search_all_cfg_t* cfg, uint32_t round, float peak, double sum, uint32_t W5, const float* acc,
                               lsn_cell_search_all_decision_t* out);

/* ---- IQ capture file replay ----
 * Replaces the file source of the reference's file mode: srsran_ue_sync_init_file_multi(&ue_sync, nof_prb, file, offset_time,
 * offset_freq, nof_rx_antennas) + one srsran_ue_sync_zerocopy per subframe (LTESniffer_Core.cc:252-258,365; options -O / -o,
 * ArgManager.cc:144-149).  File format: complex float32 (or integer pairs, sample_format below), antennas interleaved sample by sample, subframe aligned after the
 * offset (file mode has no PSS tracking); every 15*N samples per antenna are one subframe, counted from start_tti.
 * offset_freq_hz != 0: every subframe is multiplied by exp(-j 2 pi offset_freq n / fs) with n restarting per subframe.
 * The SFN the reference takes from the MIB (LTESniffer_Core.cc:382-420) is an input here (start_tti).
 * Blocks of LSN_FILE_BLOCK (default 800) subframes go to the GPU and are re-laid-out there while the previous blocks are processed
 * (LSN_FILE_SLOTS, default 8, blocks in flight): LSN_FILE_READERS (default 12) threads pread() a block into a pinned buffer;
 * LSN_FILE_MMAP=1 page-locks the blocks in a mapping of the file instead (no CPU copy; slower on the boxes measured).  The block
 * buffers stay allocated between calls, so the first call pays ~0.15 s of allocation. */
/* sample_format: LSN_FILE_CF32 is the reference's (srsran_filesource_init(.., SRSRAN_COMPLEX_FLOAT_BIN) behind srsran_ue_sync_init_file_multi).
 * LSN_FILE_SC16 / LSN_FILE_SC8 are an extension: integer I/Q pairs (int16 / int8, little endian, I first) as the radio delivers them over its
 * link and as srsRAN's SRSRAN_COMPLEX_SHORT_BIN files hold them; the GPU converts, sample = (float)integer * sample_scale (exact for a power of
 * two, one float rounding otherwise), everything behind that is the cf32 path.  A subframe is 245 760 B instead of 491 520 B at 20 MHz / 2 antennas,
 * so a host link that feeds 108 k subframes/s of cf32 feeds twice that of sc16. */
#define LSN_FILE_CF32 0u
#define LSN_FILE_SC16 1u
#define LSN_FILE_SC8 2u
typedef struct {
  uint32_t nof_antennas;        /* interleaved antennas in the file = nof_rx_antennas of the Phy */
  int64_t offset_time_samples;  /* -O: samples (per antenna) skipped at the start */
  float offset_freq_hz;         /* -o: frequency offset correction */
  uint32_t sample_format;       /* LSN_FILE_CF32 (0, the reference's), LSN_FILE_SC16, LSN_FILE_SC8; anything else is refused */
  float sample_scale;           /* integer formats: value of one LSB; 0 = full scale +-1 (1/32768, 1/128); ignored for cf32 */
} lsn_file_cfg_t;
int lsn_phy_process_file(lsn_phy_t* phy, const char* path, const lsn_file_cfg_t* cfg, uint32_t start_tti, uint64_t max_subframes /* 0 = to the end */,
                         uint32_t update_meta_period, uint64_t* subframes_done);
/* Reserves the file source's block buffers (page-locked read blocks + device blocks, 4.7 GB at 20 MHz / 2 antennas) ahead of the first replay:
 * the reference knows at start-up that it replays a file (args.input_file_name, LTESniffer_Core.cc:240-262) - call this behind lsn_phy_set_cell and the
 * first lsn_phy_process_file does not pay for page-locking 1.5 GB inside the replay.  Optional (lsn_phy_process_file reserves what is missing).
 * nof_antennas = lsn_file_cfg_t.nof_antennas of the replay. */
int lsn_phy_prepare_file(lsn_phy_t* phy, uint32_t nof_antennas);

/* ---- recordings made at any sample rate: polyphase resampler on the GPU ----
 * Output sample m sits at input position P0 + m * D, D = round(rate_in / rate_out * 2^64), a 64.64 fixed-point number formed in 128-bit
 * integers: a sample is a function of (input, configuration, m) and of nothing else - not of block sizes or call boundaries.  The rates are
 * doubles, so a recording whose clock is off by a KNOWN amount replays correctly when the true rate is given (open loop: nothing tracks;
 * lsn_clock_estimate / lsn_file_clock_estimate below MEASURE that amount ahead of the replay).
 * Filter: Kaiser-windowed sinc, cut-off min(rate_in, rate_out) / 2, 80 dB design attenuation, pass band |f| <= passband_hz, stop band from
 * min(rate_in, rate_out) - passband_hz; the number of taps follows from the width between the two.  Accepted: rate_in <= 4 rate_out with at most 192
 * taps (a pass band the lower rate cannot carry with them - min(rate_in, rate_out) below about 2.06 passband_hz when up-sampling - is refused), and 4 rate_out <
 * rate_in <= 32 rate_out with rate_in <= 122.88e6, rate_out >= 3.84e6 and at most 768 taps: every cell of 15 resource blocks or more out of a recording of up
 * to 122.88 MS/s (a 1.92 MS/s output - the 6-PRB cell - stays refused above ratio 4).  Refused (LSN_ERROR_INVALID_INPUTS): everything
 * else, a struct_size the library does not know, rates that are zero, negative or not finite.
 *
 * A cell that is not at the centre of the recording (offset-tuned capture, one carrier of a wideband capture): center_offset_hz is its carrier relative
 * to the recording's centre.  Input sample n (its index in the RECORDING) is multiplied by exp(-2 pi j Phi(n) / 2^64) before the filter sees it, Phi(n) =
 * n W mod 2^64, W = round(center_offset_hz / rate_in * 2^64) mod 2^64: integer phase, so pieces, block sizes and call boundaries still change no bit.  The
 * exponential is a two-table NCO (12 + 10 phase bits, float32).  Same filter, same tap counts.  Accepted when finite and |center_offset_hz| + passband_hz <=
 * rate_in / 2 (the cell lies inside the recording), otherwise LSN_ERROR_INVALID_INPUTS.  Open loop: nothing tracks a carrier (lsn_carrier_scan FINDS the carriers of a
 * recording and the sample clock is measured, lsn_clock_estimate, both ahead of the replay); one cell per
 * call - lsn_file_process_cells replays several cells of one file in one pass over it.  0 runs the kernel without the mixer.  Unlike lsn_file_cfg_t.offset_freq_hz (a rotation of the OUTPUT samples
 * that restarts every subframe, behind the filter) this is a translation in front of it.
 *
 * lsn_resample: needs no Phy.  in: [sample][antenna] in sample_format, in[0] = sample in_base of the recording; out: [antenna][n_out] cf32,
 * out[0] = output sample out_first.  Output sample 0 sits at first_sample + first_frac.  Samples in front of sample 0 of the recording read as
 * zeros; every other sample the outputs read must lie inside in (lsn_resample_span tells which), otherwise LSN_ERROR_INVALID_INPUTS.  A caller
 * that resamples a long recording in pieces keeps first_sample / first_frac, moves in_base and out_first, and gets the samples of one call bit for bit. */
typedef struct {
  uint32_t struct_size;      /* sizeof(lsn_resample_cfg_t), or the size up to and including passband_hz; the library refuses every other size */
  uint32_t nof_antennas;     /* interleaved in the input */
  uint32_t sample_format;    /* LSN_FILE_* */
  float    sample_scale;     /* as lsn_file_cfg_t */
  double   rate_in_hz, rate_out_hz;
  uint64_t first_sample;     /* input position of output sample 0: integer part ... */
  double   first_frac;       /* ... and fraction, 0 <= f < 1 */
  uint64_t in_base;          /* index, in the recording, of in[0] */
  uint64_t out_first;        /* index m of out[0] */
  double   passband_hz;      /* |f| that must come through unharmed: 15 kHz * (6 nof_prb + 1) for an LTE cell; 0 = 0.44 min(rate_in, rate_out) */
  double   center_offset_hz; /* carrier of the wanted cell relative to the recording's centre (may be negative); absent in the old struct_size: 0 */
} lsn_resample_cfg_t;
typedef struct {
  int64_t in_lo, in_hi;      /* outputs out_first .. out_first + n_out - 1 read the input samples in_lo <= n < in_hi (in_lo < 0: zeros) */
  uint64_t max_out;          /* number of outputs from out_first on whose samples all lie in front of in_end */
  uint32_t taps, reserved;   /* T: products per output */
} lsn_resample_span_t;
int lsn_resample(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_resample_cfg_t* cfg, float* out /* [antenna][n_out] cf32 */,
                 int out_on_device, uint64_t n_out);
int lsn_resample_span(const lsn_resample_cfg_t* cfg, uint64_t n_out, uint64_t in_end /* samples in the recording */, lsn_resample_span_t* out);

/* lsn_phy_process_file on a recording made at sample_rate_hz: the reader fetches, for every block of output subframes, the input samples the block
 * reads, and the resampler takes the place of the format conversion (same formats, same -o rotation on the output samples).  Output rate:
 * lsn_sampling_freq_hz(nof_prb, sampling mode of the Phy); pass band 15 kHz * (6 nof_prb + 1).  The start of subframe 0 is input position
 * cfg->offset_time_samples + offset_time_frac; lsn_cell_search on a resampled head gives sf_start in OUTPUT samples: multiply by sample_rate_hz /
 * output rate.  Only subframes whose whole input lies inside the file are produced.  The block buffers are those of lsn_phy_prepare_file: when
 * sample_rate_hz is above the output rate a block carries fewer subframes so that its input fits (LSN_FILE_BLOCK too small for one subframe's
 * input: LSN_ERROR_INVALID_INPUTS).  sample_rate_hz equal to the output rate with a zero fraction and a zero center_offset_hz is
 * lsn_phy_process_file; with a non-zero center_offset_hz it goes through the resampler (equal rates, the mixer in front).  LSN_TTI_FROM_MIB resamples through the
 * same plan, offset included.  A rate or an offset outside the accepted range (above), a wrong struct_size: LSN_ERROR_INVALID_INPUTS, nothing is decoded. */
typedef struct {
  uint32_t struct_size;        /* sizeof(lsn_file_rate_t), or the size up to and including offset_time_frac; every other size is refused */
  uint32_t reserved;
  double   sample_rate_hz;     /* rate of the file; the output rate is lsn_sampling_freq_hz(nof_prb, the Phy's sampling mode) */
  double   offset_time_frac;   /* added to cfg->offset_time_samples (both in INPUT samples); >= 0 */
  double   center_offset_hz;   /* carrier of the wanted cell relative to the recording's centre, as lsn_resample_cfg_t; absent in the old struct_size: 0 */
} lsn_file_rate_t;
int lsn_phy_process_file_rate(lsn_phy_t* phy, const char* path, const lsn_file_cfg_t* cfg, const lsn_file_rate_t* rate, uint32_t start_tti, uint64_t max_subframes,
                              uint32_t update_meta_period, uint64_t* subframes_done);

/* ---- every cell of a wideband recording in ONE pass over the file ----
 * lsn_carrier_scan returns the carriers of a recording; replaying them one lsn_phy_process_file_rate call each reads and copies the whole file once per cell.
 * Here every cell has its own Phy and its own resampler plan (formed exactly as lsn_phy_process_file_rate forms it: rate pair, pass band 15 kHz (6 nof_prb + 1),
 * start position, tuning word), and block k of the replay - output subframes [first + k blk, first + (k + 1) blk) of EVERY cell - is fed from the union of the
 * cells' input spans: one read, one host-to-device copy, one kernel launch (k_resample_cells) that writes each cell's subframes into its own Phy's block buffer,
 * then one submit per Phy in the order of the list.  An output sample is a function of (input, configuration, m) only, so each Phy gets, bit for bit, the samples
 * of its single-cell replay and produces its records.  The cells may differ in bandwidth, start position, start TTI (LSN_TTI_FROM_MIB is resolved per cell) and
 * length; a cell that has run out takes no part in later blocks.  The block size starts from LSN_FILE_BLOCK and shrinks until the union fits the largest raw
 * block buffer the Phys hold - no allocation grows.  All Phys live on one GPU; at most LSN_FILE_MAX_CELLS of them.
 * Refused with LSN_ERROR_INVALID_INPUTS before a byte is read: n_cells 0 or above LSN_FILE_MAX_CELLS; a struct_size the library does not know; a null or
 * repeated phy, one without a cell, one from lsn_phy_create_multi, Phys on different devices, a Phy whose antenna count is not cfg->nof_antennas; non-zero offset
 * fields in cfg (the cells carry their own); a cell lsn_phy_process_file_rate would refuse; cells whose starts lie so far apart that one subframe of each does
 * not fit one block (pass start positions closer together, or replay the cells separately).  A refusal decodes nothing and leaves every Phy usable.
 * When one Phy fails during the replay, nothing more is submitted to any of them, all are waited for, and its code is returned; subframes_done and status are
 * filled per cell either way. */
#define LSN_FILE_MAX_CELLS 8u
typedef struct {
  uint32_t struct_size;          /* sizeof(lsn_file_cell_t); every other size is refused */
  uint32_t nof_prb; int rates;   /* bandwidth and sampling mode of the cell: read only when phy is NULL (lsn_file_cells_span on a machine with no GPU) */
  lsn_phy_t* phy;                /* its cell is set; one engine, not a lsn_phy_create_multi handle */
  double center_offset_hz;       /* as lsn_file_rate_t; the field lsn_carrier_t.center_offset_hz goes into */
  int64_t offset_time_samples; double offset_time_frac;   /* start of the cell's subframe 0 in the file, in samples of the file */
  float offset_freq_hz;          /* -o rotation of this cell's output samples, as lsn_file_cfg_t */
  uint32_t start_tti;            /* may be LSN_TTI_FROM_MIB */
  uint32_t update_meta_period;
  uint64_t max_subframes;        /* 0 = to the end */
  uint64_t subframes_done;       /* out */
  int status;                    /* out: this cell's engine's return code */
} lsn_file_cell_t;
int lsn_file_process_cells(const char* path, const lsn_file_cfg_t* cfg /* nof_antennas, sample_format, sample_scale; the offset fields must be 0 */, double sample_rate_hz,
                           lsn_file_cell_t* cells, uint32_t n_cells);
/* The plan of block `block` of that replay, without a device: the union [in_lo, in_hi) of input samples it reads (clamped at sample 0) and, per cell, the
 * first output subframe (counted from the cell's start position; LSN_TTI_FROM_MIB counts as no subframes dropped), the number of subframes and the taps.
 * blk_subframes stands for LSN_FILE_BLOCK: the raw block buffer holds blk_subframes subframes of cf32 of the widest cell; blk_used is what the block size shrank
 * to.  A block behind the end of every cell has nof_active 0.  Same refusals as lsn_file_process_cells, phy aside: with phy NULL the cell's bandwidth comes from
 * nof_prb / rates. */
typedef struct {
  int64_t in_lo, in_hi;
  uint32_t blk_used, nof_active;
  uint64_t first_subframe[LSN_FILE_MAX_CELLS];
  uint32_t nof_subframes[LSN_FILE_MAX_CELLS];
  uint32_t taps[LSN_FILE_MAX_CELLS];
} lsn_file_cells_span_t;
int lsn_file_cells_span(const lsn_file_cfg_t* cfg, double sample_rate_hz, const lsn_file_cell_t* cells, uint32_t n_cells, uint64_t in_end /* samples in the recording */,
                        uint32_t block, uint32_t blk_subframes, lsn_file_cells_span_t* out);
/* k_resample_cells without a Phy: several resamplings of ONE input in one upload and one launch - the sibling of lsn_carrier_channel for full-bandwidth carriers.
 * cfgs[c] is validated exactly as lsn_resample validates it and outs[c] ([antenna][n_out[c]] cf32) equals lsn_resample with cfgs[c], bit for bit.  nof_antennas,
 * sample_format, sample_scale, rate_in_hz and in_base must agree across cfgs and every cfg must have the full struct_size; n_cells 0 or above
 * LSN_FILE_MAX_CELLS, n_out NULL: LSN_ERROR_INVALID_INPUTS, the outputs untouched.  in must hold what every cell reads (lsn_resample_span per cell). */
int lsn_resample_cells(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_resample_cfg_t* cfgs, uint32_t n_cells, float* const* outs,
                       int out_on_device, const uint64_t* n_out);

/* k_resample_ring without a Phy, the sibling of lsn_resample_cells for the kernel a stream runs (below): the host input window in[0 .. n_in) = samples in_base ..
 * in_base + n_in of the recording (in_base of the cfgs) is placed into a device ring of ring_samples samples per antenna, sample n at slot n mod ring_samples -
 * two copies when the window crosses the end of the ring - and the cells are resampled out of the ring in one launch; outs[c] ([antenna][n_out[c]] cf32, host)
 * equals lsn_resample_cells' with the same arguments, bit for bit.  Refused like lsn_resample_cells, and: ring_samples not a power of two or above 2^32,
 * n_in > ring_samples.  A refusal leaves the outputs untouched. */
int lsn_resample_cells_ring(int device, const void* in, uint64_t n_in, uint64_t ring_samples, const lsn_resample_cfg_t* cfgs, uint32_t n_cells, float* const* outs,
                            const uint64_t* n_out);

/* ---- the antenna map ----
 * Everything above moves ALL antennas of a recording by one center_offset_hz and wants a Phy with as many antennas as the recording has.  With a map, output
 * antenna a of a Phy is cut from input antenna src_antenna[a] of the recording at carrier center_offset_hz + offset_hz[a]; positions, filter, pass band and sample
 * clock are the cell's own and shared by its outputs.  Two uses: UL_MODE (antenna 0 = downlink, antenna 1 = uplink) from ONE wideband channel that holds both
 * directions - src_antenna = {0, 0}, offset_hz = {0, -duplex spacing} -, and the replay of any one or two antennas of a recording of up to eight.
 * While a map is set, in that Phy's lsn_phy_process_file_rate and lsn_file_process_cells replays and in streams opened on it, nof_antennas of the file or stream
 * is the RECORDING's, 1 .. 8, and need not equal the Phy's; every src_antenna must be below it.  Each output must satisfy
 * |center_offset_hz + offset_hz[a]| + passband <= rate_in / 2, finite (the rule of lsn_file_rate_t, per output); otherwise the replay returns
 * LSN_ERROR_INVALID_INPUTS, nothing is decoded and the Phy stays usable.  A mapped replay always goes through the resampler, equal rates included, and
 * LSN_TTI_FROM_MIB reads the mapped samples.  A pass or a stream may mix mapped and unmapped Phys; an unmapped Phy still needs the recording's antenna count.
 * The setter refuses (LSN_ERROR_INVALID_INPUTS, the map as it was): a struct_size other than sizeof, nof_out other than the Phy's nof_rx_antennas (so 0 and 3),
 * src_antenna above 7, an offset that is not finite, a lsn_phy_create_multi handle.  Limits of a mapped Phy, refused when the replay or stream starts: the channel
 * filter (lsn_phy_set_channel_filter) together with a map, lsn_phy_process_file (it has no rate) - and on a stream that has a mapped cell lsn_stream_track,
 * lsn_stream_reacquire and lsn_stream_frame_sync.  The worker pool and lsn_phy_process_host* take no map.  The duplex spacing is an input. */
#define LSN_MAP_MAX_OUT 2u
typedef struct {
  uint32_t struct_size;                  /* sizeof(lsn_antenna_map_t); every other size is refused */
  uint32_t nof_out;                      /* = the Phy's nof_rx_antennas */
  uint32_t src_antenna[LSN_MAP_MAX_OUT]; /* input antenna each output antenna is cut from; may repeat */
  double   offset_hz[LSN_MAP_MAX_OUT];   /* added to the cell's center_offset_hz for this output */
} lsn_antenna_map_t;
int lsn_phy_set_antenna_map(lsn_phy_t* phy, const lsn_antenna_map_t* map /* NULL = off, the default */);
/* lsn_resample_cells / lsn_resample_cells_ring with a map per cell (k_resample_map, k_resample_map_ring and their wide-ratio twins).  maps[c].nof_out = 0: the
 * identity - the cell as lsn_resample_cells resamples it; else outs[c] is [nof_out][n_out[c]] cf32 and row a equals row src_antenna[a] of lsn_resample with
 * center_offset_hz + offset_hz[a], bit for bit.  cfgs are validated as there (cfgs[c].center_offset_hz itself only through the outputs of a mapped cell), maps as
 * lsn_phy_set_antenna_map validates them with nof_out 1 or 2, src_antenna below cfgs' nof_antennas, and the rule above per output.  maps NULL: refused. */
int lsn_resample_cells_map(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_resample_cfg_t* cfgs, const lsn_antenna_map_t* maps, uint32_t n_cells,
                           float* const* outs, int out_on_device, const uint64_t* n_out);
int lsn_resample_cells_ring_map(int device, const void* in, uint64_t n_in, uint64_t ring_samples, const lsn_resample_cfg_t* cfgs, const lsn_antenna_map_t* maps,
                                uint32_t n_cells, float* const* outs, const uint64_t* n_out);
/* lsn_file_cells_span with the antennas of every cell's Phy given: nof_out[c] = 1 or 2, or 0 = cfg->nof_antennas (an unmapped cell); NULL = all 0.  cfg->nof_antennas
 * is the recording's.  The raw block buffer is the one of the Phy with the largest blocks - blk_subframes subframes of nof_out antennas of cf32 - and holds samples
 * of ALL the recording's antennas, so blk_used follows the recording's antenna count; in_lo and in_hi of a block of a given size do not.  A cell with a Phy
 * takes its Phy's map and antenna count, and a non-zero nof_out[c] must agree with it. */
int lsn_file_cells_span_map(const lsn_file_cfg_t* cfg, double sample_rate_hz, const lsn_file_cell_t* cells, uint32_t n_cells, const uint32_t* nof_out, uint64_t in_end,
                            uint32_t block, uint32_t blk_subframes, lsn_file_cells_span_t* out);

/* ---- a live wideband stream pushed in host buffers ----
 * The file replays above take a path.  A stream takes the same samples as they arrive, in host buffers of any length, and feeds the same cells: per cell exactly
 * the subframes a file of the samples pushed so far replays, and - an output sample being a function of (input, configuration, m) only - bit for bit the samples
 * of lsn_file_process_cells on those bytes, however the stream was cut into pushes.
 *   cells     lsn_file_cell_t as lsn_file_process_cells takes them: Phy, center_offset_hz, start of the cell's subframe 0 in samples of the stream counted from the
 *             first sample ever pushed, start_tti, update_meta_period, max_subframes, offset_freq_hz; subframes_done and status are not written (status call).
 *             Each cell's plan is the one lsn_phy_process_file_rate forms.  A stream starts at the cell's subframe 0.
 *   storage   ONE device buffer of ring_samples samples per antenna, a power of two; sample n of the stream sits at slot n mod ring_samples.  A push copies its
 *             samples host-to-device straight to their slots (two copies when it crosses the end of the ring, a long push in pieces): no host staging buffer, no
 *             memcpy on the caller's thread.  A gap - the radio reported dropped samples - is a memset of the same slots: zeros arrive, positions stay.
 *   when      after `pushed` samples cell c has floor(outputs whose whole input span lies in front of pushed / subframe length) complete subframes, capped by
 *             max_subframes - the rule a file's subframes are counted by (with a channel filter: in front of pushed - L, lsn_file_cells_span's rule).  A cell is submitted when block_subframes of them are not submitted yet (fewer: the last
 *             ones in front of max_subframes, or a flush): one k_resample_ring launch for all cells that are due, into block buffers of their Phys (those of
 *             lsn_phy_prepare_file), then one submit per Phy in the order of the list.
 *   ring      nothing at or behind the oldest sample a cell still needs - the first input sample of its next subframe, minimised over the cells that have not run
 *             out - is overwritten; a piece that is written over slots an unfinished launch may still read waits for that launch, and for nothing else.
 *             ring_samples = 0: the smallest power of two that holds four blocks of the union input (block_subframes of every cell from the oldest start to the
 *             newest end, the filters' spans included).
 * lsn_stream_push returns when its samples are in the ring - the caller's buffer is free again - and decoding goes on behind it; it blocks only while the Phys
 * are more than their block buffers behind.  lsn_stream_flush submits every complete subframe and waits for every Phy; the stream goes on afterwards.
 * lsn_stream_close flushes and frees; the Phys stay usable.  Close a stream before its Phys are destroyed (lsn_phy_destroy on a Phy of an open stream closes the stream first, with a line on
 * stderr, and the stream's handle is dead from then on).  One call at a time per stream.
 * When a Phy fails nothing more is submitted to any of them; the next push or flush returns its code and lsn_stream_status shows which cell it was.  Push, gap
 * and flush on a failed stream return that code and do nothing; on a NULL (closed) stream LSN_ERROR_INVALID_INPUTS.
 * Refused at open with LSN_ERROR_INVALID_INPUTS - nothing is allocated, every Phy stays usable: everything lsn_file_process_cells refuses; start_tti =
 * LSN_TTI_FROM_MIB (the head of a live stream goes through lsn_carrier_scan and lsn_phy_mib_decode first, and that chain yields the TTI); a channel filter
 * (below) on some of the Phys but not on all, or a stop band the filter's design refuses; a Phy that belongs to an open stream; cfg->device other than the Phys'; block_subframes
 * above LSN_FILE_BLOCK; ring_samples not a power of two, above 2^32, or shorter than one block of every cell - which is also how cells whose starts lie further
 * apart than the ring less one block are refused.
 * The channel filter (lsn_phy_set_channel_filter): a stream opened on Phys that have it set runs the file pass's two stages - ONE
 * k_chan_fir_ring launch reads the ring for all cells that are due and writes every cell's y1 into an intermediate of its Phy, then one k_resample per cell reads
 * that - and submits, per cell, exactly the subframes and records of lsn_file_process_cells with the filter on the same bytes.  A cell's input span is L samples
 * wider on both sides: oldest_needed, block_input, the default ring and the ring checks (lsn_stream_track's too) count with the widened spans.  The setting is read
 * at open; changing it on a Phy of an open stream leaves that stream as it was opened and counts for the next open or file replay.
 * Not on a stream: LSN_TTI_FROM_MIB, the worker pool, cells on several GPUs, a mix of filtered and unfiltered cells.  Rate and offsets are inputs, as for files; a stream that asks
 * for it (lsn_stream_track, below) follows the sample clock from there with a timing loop per cell.  File replays and the worker pool do not track. */
typedef struct lsn_stream lsn_stream_t;
typedef struct {
  uint32_t struct_size;      /* sizeof(lsn_stream_cfg_t); every other size is refused */
  int      device;           /* the Phys' */
  double   sample_rate_hz;
  uint32_t nof_antennas;     /* interleaved sample by sample in what is pushed */
  uint32_t sample_format;    /* LSN_FILE_* */
  float    sample_scale;     /* as lsn_file_cfg_t */
  uint32_t block_subframes;  /* a cell is submitted once it has that many complete subframes; 0 = the file source's block size (LSN_FILE_BLOCK) */
  uint64_t ring_samples;     /* 0 = chosen by the library */
} lsn_stream_cfg_t;
typedef struct {
  uint64_t samples_pushed;
  uint64_t ring_samples;
  int64_t  oldest_needed;    /* the oldest sample of the stream a cell still needs; samples_pushed when none does */
  uint32_t block_subframes, nof_cells;
  int      failed;           /* LSN_SUCCESS, or the code every later push and flush returns */
  int      status[LSN_FILE_MAX_CELLS];                 /* per cell: its Phy's return code */
  uint64_t subframes_submitted[LSN_FILE_MAX_CELLS];
} lsn_stream_status_t;
/* The plan after pushed_samples samples in all, without a device (cells with phy NULL take nof_prb / rates, as lsn_file_cells_span).  subframes_complete: per
 * cell, what a flush at that point has submitted in all; subframes_submitted: what a stream that was never flushed has submitted - whole blocks, and the last
 * ones in front of max_subframes; oldest_needed belongs to the latter, oldest_needed_flushed to the former.  ring_samples: cfg's, or the default; block_input: the
 * input samples of one block of every cell from the oldest start to the newest end, which the ring must hold.  Same refusals as the open, Phys and device aside. */
typedef struct {
  uint64_t ring_samples, block_input;
  int64_t  oldest_needed, oldest_needed_flushed;
  uint32_t block_subframes, reserved;
  uint64_t subframes_complete[LSN_FILE_MAX_CELLS];
  uint64_t subframes_submitted[LSN_FILE_MAX_CELLS];
  uint32_t taps[LSN_FILE_MAX_CELLS];
} lsn_stream_span_t;
int lsn_stream_open(const lsn_stream_cfg_t* cfg, lsn_file_cell_t* cells, uint32_t n_cells, lsn_stream_t** out);
int lsn_stream_push(lsn_stream_t* s, const void* iq /* [sample][antenna] in sample_format; NULL = a gap of n_samples zeros */, uint64_t n_samples);
int lsn_stream_flush(lsn_stream_t* s);
int lsn_stream_status(lsn_stream_t* s, lsn_stream_status_t* out);
int lsn_stream_close(lsn_stream_t* s);
int lsn_stream_span(const lsn_stream_cfg_t* cfg, const lsn_file_cell_t* cells, uint32_t n_cells, uint64_t pushed_samples, lsn_stream_span_t* out);
/* lsn_stream_span reads the channel filter's setting from a non-NULL phy, as lsn_file_cells_span does.  The plan of a filtered stream without a Phy: the same call
 * with stopband_hz[n_cells], a non-zero entry being that cell's stop band (lsn_phy_set_channel_filter's value); NULL or all zero: lsn_stream_span.  Every cell
 * or none; a stop band the design refuses is refused. */
int lsn_stream_span_filtered(const lsn_stream_cfg_t* cfg, const lsn_file_cell_t* cells, uint32_t n_cells, const double* stopband_hz, uint64_t pushed_samples,
                             lsn_stream_span_t* out);
/* lsn_stream_span with the antennas of every cell's Phy given, as lsn_file_cells_span_map takes them (the antenna map, above): cfg->nof_antennas is the stream's.  A
 * stream's ring and block input count samples per antenna and do not depend on either number; the call refuses what a mapped open refuses. */
int lsn_stream_span_map(const lsn_stream_cfg_t* cfg, const lsn_file_cell_t* cells, uint32_t n_cells, const uint32_t* nof_out, uint64_t pushed_samples, lsn_stream_span_t* out);
/* lsn_stream_span describes the NOMINAL plan: a tracked stream (below) counts a cell's subframes by the positions its loop has decided, which leave the plan's by
 * lsn_stream_track_status_t.position_drift. */

/* ---- a stream that follows the sample clock: a PSS timing loop per cell ----
 * Opt-in, per cell of an open stream, accepted only before the first sample is pushed.  A stream that does not ask for it runs exactly the launches described above.
 * The resampler's position becomes piecewise linear in the output index.  The unit is a SEGMENT, one half frame (5 output subframes), anchored so that a segment
 * starts at every output subframe whose TTI is a multiple of 5 (segment 0 may be shorter); segment h > 0 holds one PSS, in its first subframe.
 *   position(m) = base_h + (m - m_h) step_h for the outputs of segment h;  base_(h+1) = base_h + n_h step_h in exact 128-bit integers: only the step changes, the
 *   position never jumps, the FFT window never moves.
 * The measurement taken in segment h decides the step of segment h + 2, whatever the pushes look like: no part of segment h + 2 is resampled before the measurement
 * of segment h has come back (the host waits for that launch's event then, and nowhere else).  Segments 0 and 1 run at the opened rate times 1 + initial_ppm 1e-6.
 * Every decision is a function of (input samples, configuration) only: the samples a Phy receives, its records and the loop's state do not depend on how the
 * stream was cut into pushes, on the ring size or on block_subframes.  Resampling launches are per segment (or the part of one that fits the block buffer) and
 * write into the Phy's block buffer at the segment's subframe offset; a block is still submitted once block_subframes subframes are in it.
 *   detector  k_pss_timing: N the symbol size, d = max(1, N / 128), lags l_j = (j - 6) d, j = 0 .. 12, p = 13 N / 2 the index of the first useful sample of the PSS
 *             symbol in the segment's first subframe, r the replica of lsn_clock_replica (unit energy, rotated by the cell's cfo_hz):
 *               C_j = sum_a | sum_(k<N) x_a[p + l_j + k] conj r[k] |^2 / sum_a sum_(k<N) |x_a[p + l_j + k]|^2     (0 when the denominator is 0)
 *             j* = first maximum; geometrically valid when 0 < j* < 12; frac = 0.5 (C[j*-1] - C[j*+1]) / (C[j*-1] - 2 C[j*] + C[j*+1]);
 *             e = (j* - 6 + frac) d output samples, positive: the PSS arrived late.  Valid when geometrically valid and peak >= 0.25 mean(the last up to 8 valid
 *             peaks); the first geometrically valid one is valid.  Invalid too: a segment without a PSS (a short segment 0), one whose first subframe reads
 *             samples of a gap, a cell that is not enabled.
 *   loop      valid: I += Ki e, c = Kp e + I;  invalid: c = I;  I and c clamped to +- lim = max_ppm 1e-6 seglen (seglen = 5 subframe lengths); anti-windup: a valid
 *             step leaves I as it was when Kp e + clamp(I + Ki e) lies beyond +- lim on the side e pushes to (the correction is at its limit already);
 *             step_(h+2) = step_nominal + (int128) nearbyint(ldexp(rate_in / rate_out, 64) * c / seglen), in doubles, one rounding per operation.
 *             lost is set after lost_after consecutive invalid segments: the loop holds its rate and keeps measuring; the next valid measurement clears it.
 * lsn_stream_track refuses with LSN_ERROR_INVALID_INPUTS, the stream unchanged and usable: after a push; gains not finite or not positive; max_ppm outside
 * (0, 120]; |initial_ppm| > max_ppm or not finite; cfo_hz not finite; a ring shorter than block_input recomputed with every step widened by 1 + max_ppm 1e-6
 * (and, on a filtered stream, every cell's span by its 2 L). */
typedef struct {
  uint32_t struct_size;      /* sizeof(lsn_stream_track_cfg_t); every other size is refused */
  uint32_t lost_after;       /* 0 = 40 */
  double   kp, ki;           /* 0 = 1/4, 1/32 */
  double   max_ppm;          /* 0 = 100 */
  float    cfo_hz[LSN_FILE_MAX_CELLS];        /* per cell: the replica is rotated by it (lsn_cell_search_t.cfo_hz) */
  double   initial_ppm[LSN_FILE_MAX_CELLS];   /* per cell: the correction segments 0 and 1 run at, and the integrator's start */
  uint32_t enable[LSN_FILE_MAX_CELLS];        /* per cell: 0 = this cell keeps the opened rate */
} lsn_stream_track_cfg_t;
typedef struct {
  uint32_t struct_size;      /* in: sizeof(lsn_stream_track_status_t); every other size is refused */
  uint32_t nof_cells;
  uint64_t segments[LSN_FILE_MAX_CELLS];      /* segments decided */
  uint64_t valid[LSN_FILE_MAX_CELLS], invalid[LSN_FILE_MAX_CELLS];   /* measurements that have come back */
  uint32_t lost[LSN_FILE_MAX_CELLS];
  double   last_error[LSN_FILE_MAX_CELLS];       /* e of the last valid measurement, output samples */
  double   correction_ppm[LSN_FILE_MAX_CELLS];   /* c / seglen 1e6 of the segment decided last */
  double   integrator_ppm[LSN_FILE_MAX_CELLS];
  double   position_drift[LSN_FILE_MAX_CELLS];   /* position of the next output to resample minus the nominal plan's, input samples */
} lsn_stream_track_status_t;
int lsn_stream_track(lsn_stream_t* s, const lsn_stream_track_cfg_t* cfg);
/* the measurements in flight are waited for first, so after a flush the answer is a function of the samples pushed */
int lsn_stream_track_status(lsn_stream_t* s, lsn_stream_track_status_t* out);
/* The loop without a GPU: one step on *state with the gains of cfg (its per-cell fields are not read) -> the new state and step - step_nominal as the two halves
 * of a 128-bit two's complement integer.  seglen: output samples of a segment. */
typedef struct {
  double   integrator, correction;   /* I and c, output samples per segment */
  uint32_t invalid_run, lost;
} lsn_stream_track_state_t;
int lsn_stream_track_step(const lsn_stream_track_cfg_t* cfg, double rate_in_hz, double rate_out_hz, uint32_t seglen, lsn_stream_track_state_t* state, double e, int valid,
                          uint64_t* delta_hi, uint64_t* delta_lo);
/* the observation of one window without a GPU: C[13] -> 1 and e, peak when geometrically valid, 0 (peak filled) when not */
int lsn_pss_timing_error(const float* C, uint32_t d, double* e, double* peak);
/* k_pss_timing without a Phy, the sibling of lsn_clock_track: per cell, blocks in the block-buffer layout [subframe][antenna][sflen] cf32 (host or device memory),
 * a list of n_occ (subframe, p) pairs, the replica [N] cf32 (host) and d -> C [n_occ][13] (host).  All cells go into one launch when no cell has more than four
 * occurrences (more: four per launch).  Refused: n_cells 0 or above LSN_FILE_MAX_CELLS, a struct_size the library does not know, N outside 128 .. 2048,
 * d != max(1, N / 128), a subframe outside the blocks, a window [p - 6 d, p + 6 d + N) outside its subframe. */
typedef struct {
  uint32_t struct_size;      /* sizeof(lsn_pss_timing_cell_t) */
  uint32_t N, d, sflen, nof_antennas, nof_subframes, n_occ, reserved;
  const void* blocks;
  const float* replica;
  const uint32_t* occ;       /* [n_occ][2]: subframe, p */
  float* C;                  /* out */
} lsn_pss_timing_cell_t;
int lsn_pss_timing(int device, int blocks_on_device, const lsn_pss_timing_cell_t* cells, uint32_t n_cells);

/* ---- a tracked stream that finds a cell's timing again after samples were lost ----
 * k_pss_timing sees 13 lags, +- 6 d around the place where the PSS must be.  A radio that overflows drops (or repeats) a few thousand samples without saying how
 * many; the PSS then lies outside that window for good and every segment is invalid.  Opt-in per stream, accepted only after lsn_stream_track and before the first
 * push; a stream that does not ask runs exactly the launches it ran before.  Notation as above, W5 = 75 N (a half frame), sflen = 15 N.
 *   metric    k_pss_acquire over the SPAN of segment h: the 6 sflen outputs m = 0 .. 6 sflen - 1 at the positions base_h + m step_h - segment h and one subframe
 *             more, all at segment h's step -, resampled out of the ring into a scratch of the cell's; lags L_i = i d, i = 0 .. W5 / d - 1 (9600 at every N):
 *               C_i = sum_a | sum_(k<N) x_a[L_i + k] conj r[k] |^2 / sum_a sum_(k<N) |x_a[L_i + k]|^2      (0 when the denominator is 0)
 *             k_pss_timing's quantity, with its arithmetic: C[p / d + j - 6] of a span is bit for bit k_pss_timing's C_j on the span's first subframe.
 *   decision  host, doubles: i* the first maximum, peak = C[i*]; far = the largest C_i whose circular distance from i* is above 8 lags.  Accepted when peak > 0,
 *             peak >= min_ratio far, and peak >= 0.25 mean(the cell's valid-peak history as it stands behind the measurement of segment h + 1; empty: accepts).
 *             o = ((i* d - p + W5 / 2) mod W5) - W5 / 2 output samples, signed: the nearest PSS, so a slip of up to +- 2.5 ms is repaired with the TTI intact.
 *   when      on entering segment h, after the loop's step that consumed the measurement of segment h - 2 (and after a search's result was taken in): a search of
 *             segment h is due when invalid_run >= after, no search of the cell is in flight and the cell is enabled.  It is launched once its span is complete in
 *             the ring and its result is taken in on entering segment h + 3.  Accepted: base_(h+3) = end of segment h + 2 + o step_h, exact in the 64.64 integers,
 *             invalid_run = 0, integrator and correction untouched; the measurements still queued from the old timing go through the loop as they are (the peak test
 *             rejects them).  Rejected: nothing changes, the next search is due as soon as the rule allows.  A search whose span reads a declared gap is not
 *             launched and counts as rejected.  Output subframes stay contiguous and the TTI keeps counting: only a position jumps, and only here.
 *   ring      a cell with re-acquisition keeps 8 output subframes of input more (at the step widened by 1 + max_ppm 1e-6), behind what it keeps anyway: 6 for the
 *             span of the segment behind, 2.5 for a backward jump, rounded up.  oldest_needed and the ring guards count with it; lsn_stream_span keeps describing
 *             the nominal plan.
 * Limits: a slip beyond +- 2.5 ms is repaired to the nearest PSS and leaves the TTI off by a multiple of 5 subframes (lsn_stream_frame_sync,
 * below and DESIGN section 3.1m, sets it right from one PBCH decode; no SSS is needed);
 * one search per cell in flight; streams only - file replays do not track -, and not on a stream with the channel filter.
 * lsn_stream_reacquire refuses with LSN_ERROR_INVALID_INPUTS, the stream unchanged and usable: a struct_size it does not know, an untracked stream, a second call,
 * after a push, min_ratio not finite or below 1 (0 = the default), a stream with the channel filter, a ring shorter than lsn_stream_track's bound plus the 8
 * subframes. */
typedef struct {
  uint32_t struct_size;      /* sizeof(lsn_stream_reacquire_cfg_t); every other size is refused */
  uint32_t after;            /* consecutive invalid segments that make a search due; 0 = the loop's lost_after */
  double   min_ratio;        /* 0 = 3: the geometric mean of the ratio peak / far measured on noise (1.86) and with the cell present (5.1) */
  uint32_t enable[LSN_FILE_MAX_CELLS];        /* per cell: 0 = this cell is never searched */
} lsn_stream_reacquire_cfg_t;
typedef struct {
  uint32_t struct_size;      /* in: sizeof(lsn_stream_reacquire_status_t); every other size is refused */
  uint32_t nof_cells;
  uint64_t launched[LSN_FILE_MAX_CELLS], accepted[LSN_FILE_MAX_CELLS], rejected[LSN_FILE_MAX_CELLS];   /* rejected counts the searches a gap kept from being launched */
  double   last_peak[LSN_FILE_MAX_CELLS], last_ratio[LSN_FILE_MAX_CELLS];   /* of the last search that came back */
  int64_t  last_offset[LSN_FILE_MAX_CELLS];    /* o, output samples */
  uint64_t jump_segment[LSN_FILE_MAX_CELLS];   /* the segment at which the last jump took force (0: none yet) */
  double   jumps_total[LSN_FILE_MAX_CELLS];    /* the sum of all jumps, input samples */
} lsn_stream_reacquire_status_t;
int lsn_stream_reacquire(lsn_stream_t* s, const lsn_stream_reacquire_cfg_t* cfg);
/* the measurements and the searches in flight are waited for first, so after a flush the answer is a function of the samples pushed */
int lsn_stream_reacquire_status(lsn_stream_t* s, lsn_stream_reacquire_status_t* out);
/* the decision without a GPU: C[n], n d = 75 N -> 1 accepted, 0 rejected (offset, peak and ratio = peak / far filled either way), or LSN_ERROR_INVALID_INPUTS.
 * min_ratio 0 = the default; history_mean < 0: an empty history */
int lsn_pss_acquire_decide(const float* C, uint32_t n, uint32_t d, uint32_t N, double min_ratio, double history_mean, int64_t* offset, double* peak, double* ratio);
/* k_pss_acquire without a Phy, the sibling of lsn_pss_timing: per cell a span of 6 subframes in the block-buffer layout [6][antenna][sflen] cf32 (host or device
 * memory), the replica [N] cf32 (host) and d -> C [75 N / d] (host).  All cells go into one launch.  Refused: n_cells 0 or above LSN_FILE_MAX_CELLS, a struct_size
 * the library does not know, N outside 128 .. 2048, d != max(1, N / 128), sflen != 15 N. */
typedef struct {
  uint32_t struct_size;      /* sizeof(lsn_pss_acquire_cell_t) */
  uint32_t N, d, sflen, nof_antennas, reserved;
  const void* blocks;
  const float* replica;
  float* C;                  /* out */
} lsn_pss_acquire_cell_t;
int lsn_pss_acquire(int device, int blocks_on_device, const lsn_pss_acquire_cell_t* cells, uint32_t n_cells);

/* ---- a re-acquiring stream that sets the TTI right again after a slip of any length ----
 * lsn_stream_reacquire moves the position to the NEAREST PSS: a slip beyond +- 2.5 ms leaves the TTI off by a multiple of 5 subframes, and a slip by whole radio
 * frames even decodes perfectly - every record then carries the wrong frame number.  The PBCH exists only in subframe 0 and is scrambled with the cell id, so ONE
 * PBCH decode of a segment's first subframe settles the half frame, the frame number and the cell; no SSS is needed.  Opt-in per stream, accepted only after
 * lsn_stream_reacquire and before the first push; a stream that does not ask runs exactly the launches it ran before, and one that asks and loses nothing runs no
 * PBCH launch at all.  Notation of the section above: the search of segment h was accepted and its jump is in force at segment g = h + 3.
 *   check     a jump of an enabled cell starts a check at segment g.  Attempts run on the segments a = g, g + 1, ..., at most `tries` of them.  A new accepted jump
 *             restarts the check at its own g; attempts on segments in front of that g are ignored when they come back.
 *   attempt   the PBCH decode (lsn_phy_mib_decode_side's: the Phy's side scratch) of the first subframe of segment a, read from the block buffer, queued directly
 *             behind that piece's k_pss_timing window.  Not launched - and counted as "not found" - when that subframe's input span reads a declared gap: the test
 *             that decides whether the window is launched.  Its result rides with the measurement of segment a and is taken in on entering segment a + 2, behind
 *             that measurement; status calls and flushes may fetch it early and change nothing, the rule looks at it on entering segment a + 2 only.
 *   decision  lsn_frame_sync_decide: accepted when the MIB is found and its nof_prb and nof_ports equal the Phy's.  T = 10 sfn; C = the TTI the segment's first
 *             subframe was counted as; delta = (T - C) mod 10240, reported signed in (-5120, 5120].  C mod 5 != 0 (and with it delta mod 5 != 0) is an internal
 *             error, not a case.  Chance of accepting garbage: 3 CRC masks x 4 phases / 2^16, times 1/3 for the port mask, times 1/8 for the bandwidth field
 *             (6 of its 8 values are bandwidths, one of them the Phy's): about 8e-6 per attempt.
 *   relabel   from the first subframe of segment a + 2 on the cell's TTI is start_tti + sf + shift, shift += delta mod 10240.  delta = 0 counts as confirmed,
 *             anything else as relabelled.  A partly filled block buffer is submitted, as a flush would submit it, before the first relabelled subframe goes in: no
 *             block spans two countings, and the records do not depend on block_subframes.  Segment boundaries stay on TTI multiples of 5.  After `tries` attempts
 *             without an accept given_up is incremented when the last of them is taken in, and nothing else changes.  The attempt of segment a + 1 is always in
 *             flight when the one of segment a decides; it is launched, counted and ignored.
 *   hold      (the default) the subframes from segment g up to the relabel (or the giving up) are resampled and measured but NOT submitted to the Phy: a slip by
 *             whole frames would otherwise be written out with the wrong frame number.  hold = LSN_FRAME_SYNC_NO_HOLD submits them as counted.
 * Everything is a function of (input samples, configuration): records and statuses do not depend on how the stream was pushed, on the ring or on block_subframes.
 * Limits: a slip by an exact multiple of 5 ms moves no PSS - nothing is searched and nothing is checked, the TTI stays off silently; LSN_TTI_FROM_MIB at open stays
 * refused; no channel filter (lsn_stream_reacquire's limit); file replays are not covered.
 * lsn_stream_frame_sync refuses with LSN_ERROR_INVALID_INPUTS, the stream unchanged and usable: a struct_size it does not know, a stream without
 * lsn_stream_reacquire, a second call, after a push, tries above 64, a hold it does not know. */
#define LSN_FRAME_SYNC_NO_HOLD 2u
typedef struct {
  uint32_t struct_size;      /* sizeof(lsn_stream_frame_sync_cfg_t); every other size is refused */
  uint32_t tries;            /* attempts per check; 0 = 8: four radio frames, one PBCH period.  At most 64 */
  uint32_t hold;             /* 0 = the default = 1: hold; LSN_FRAME_SYNC_NO_HOLD: submit the subframes of a running check as counted */
  uint32_t enable[LSN_FILE_MAX_CELLS];        /* per cell: 0 = never checked (a cell that is not searched is never checked either) */
} lsn_stream_frame_sync_cfg_t;
typedef struct {
  uint32_t struct_size;      /* in: sizeof(lsn_stream_frame_sync_status_t); every other size is refused */
  uint32_t nof_cells;
  uint64_t checks[LSN_FILE_MAX_CELLS], attempts[LSN_FILE_MAX_CELLS];   /* checks started; attempts launched (one a gap kept from being launched is not counted) */
  uint64_t confirmed[LSN_FILE_MAX_CELLS], relabelled[LSN_FILE_MAX_CELLS], given_up[LSN_FILE_MAX_CELLS];
  uint64_t accept_segment[LSN_FILE_MAX_CELLS];  /* the segment a of the last accepted attempt (0: none yet) */
  uint64_t relabel_segment[LSN_FILE_MAX_CELLS]; /* the segment from whose first subframe on the last relabel (delta != 0) is in force (0: none yet) */
  uint64_t held[LSN_FILE_MAX_CELLS];            /* subframes resampled and not submitted */
  uint32_t last_sfn[LSN_FILE_MAX_CELLS];        /* of the last accepted attempt */
  int32_t  last_delta[LSN_FILE_MAX_CELLS];      /* of the last accepted attempt, subframes, signed */
  uint32_t shift[LSN_FILE_MAX_CELLS];           /* the sum of all deltas mod 10240 */
} lsn_stream_frame_sync_status_t;
int lsn_stream_frame_sync(lsn_stream_t* s, const lsn_stream_frame_sync_cfg_t* cfg);
/* the measurements, searches and attempts in flight are waited for first, so after a flush the answer is a function of the samples pushed */
int lsn_stream_frame_sync_status(lsn_stream_t* s, lsn_stream_frame_sync_status_t* out);
/* the decision without a GPU: -> 1 accepted (*delta filled, signed, a multiple of 5), 0 not accepted (*delta = 0), LSN_ERROR_INVALID_INPUTS (a null pointer,
 * counted_tti >= 10240, a found MIB with sfn >= 1024), LSN_ERROR when the MIB is accepted and counted_tti is no multiple of 5 */
int lsn_frame_sync_decide(const lsn_mib_t* mib, uint32_t nof_prb, uint32_t nof_ports, uint32_t counted_tti, int32_t* delta);

/* ---- sharp channel filter in front of the resampler: a cell next to a much stronger carrier ----
 * The resampler's filter has the transition band [B, min(rate) - B]: a neighbour carrier inside it reaches the FFT's guard bins undamped and leaks into the
 * occupied bins at about -40 dB.  The channel filter is an opt-in stage 1 at the RECORDING's rate, the resampler becomes stage 2:
 *   y1[n] = sum over k = n - L .. n + L, in that order, of g[n - k] xm[k]      (one fma per product into one float32 accumulator per component)
 *   xm[n] = x[n] exp(-2 pi j (n W mod 2^64) / 2^64)  - the mixer of lsn_resample (same W, same NCO), n the index in the recording; xm[n] = 0 for n < 0
 *   g[j]  = 2 fc sinc(2 fc j) I0(beta sqrt(1 - (j / (L + 1))^2)) / I0(beta), j = -L .. L, float32;   fc = (B + S) / (2 R),   beta = 0.1102 (80 - 8.7),
 *   L     = ceil((80 - 7.95) / (14.36 (S - B) / R) / 2)
 * with R the recording's rate, B = passband_hz and S = stopband_hz: from |f| >= S on, relative to the wanted carrier, everything is 80 dB down by design.  Stage 2
 * is the resampler's plan of the same rate pair, pass band and start with center_offset_hz = 0, reading y1.  y1[n] is a function of (input, configuration, n) only:
 * block sizes, pieces and call boundaries change no bit.  Accepted: S finite, B < S <= R / 2, L <= 512 (S - B >= 0.0049 R: 301 kHz at 61.44 MS/s), and the
 * resampler's rule |center_offset_hz| + B <= R / 2; everything else is LSN_ERROR_INVALID_INPUTS.
 *
 * lsn_phy_set_channel_filter: stopband_hz of this Phy's file replays (lsn_phy_process_file, lsn_phy_process_file_rate, lsn_file_process_cells; LSN_TTI_FROM_MIB
 * resamples through the same two stages) and of the streams opened on it from then on (lsn_stream_open); 0 = off, the default.  Sticky, like lsn_phy_set_sampling.  Negative, NaN or infinite: LSN_ERROR_INVALID_INPUTS; the
 * value is checked against rate and bandwidth when a replay starts (a refused replay decodes nothing and leaves the Phy usable).  With the filter set a file at
 * the Phy's own rate goes through both stages too.  In lsn_file_process_cells either every cell's Phy has a filter or none has: a mix is refused.
 * lsn_file_cells_span reads the setting from a non-NULL phy (the block's input is L samples wider on both sides); with phy NULL it plans the unfiltered pass. */
int lsn_phy_set_channel_filter(lsn_phy_t* phy, double stopband_hz);
typedef struct {
  uint32_t struct_size;      /* in: sizeof(lsn_channel_filter_design_t); every other size is refused */
  uint32_t half_len;         /* L */
  uint32_t nof_taps;         /* 2 L + 1 */
  uint32_t reserved;
  double   cutoff;           /* fc, cycles per input sample */
} lsn_channel_filter_design_t;
/* The design alone, no GPU: L, fc and (taps != NULL: cap >= 2 L + 1 floats) g[-L] .. g[L]. */
int lsn_channel_filter_design(double rate_in_hz, double passband_hz, double stopband_hz, lsn_channel_filter_design_t* out, float* taps, uint32_t cap);
typedef struct {
  uint32_t struct_size;      /* sizeof(lsn_channel_filter_cfg_t); every other size is refused */
  uint32_t nof_antennas;     /* interleaved in the input */
  uint32_t sample_format;    /* LSN_FILE_* */
  float    sample_scale;     /* as lsn_file_cfg_t */
  double   rate_in_hz, passband_hz, stopband_hz, center_offset_hz;
  uint64_t in_base;          /* index, in the recording, of in[0] */
  uint64_t out_first;        /* index n of out[0] */
} lsn_channel_filter_cfg_t;
/* Stage 1 alone, no Phy.  in: [sample][antenna] in sample_format; out: [sample][antenna] cf32, out[0] = y1[out_first] - what lsn_resample takes as cf32 input with
 * in_base = out_first and center_offset_hz = 0.  Samples in front of sample 0 of the recording read as zeros; every other sample in [out_first - L, out_first +
 * n_out + L) must lie inside in, otherwise LSN_ERROR_INVALID_INPUTS. */
int lsn_channel_filter(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_channel_filter_cfg_t* cfg, float* out, int out_on_device, uint64_t n_out);
/* k_chan_fir_ring without a Phy, the sibling of lsn_resample_cells_ring for stage 1 of a filtered stream: the host input window in[0 .. n_in) = samples in_base ..
 * in_base + n_in of the recording is placed at its slots of a device ring of ring_samples samples per antenna (sample n at slot n mod ring_samples; every other
 * slot holds a NaN pattern, so that a read outside the window shows in the outputs), and up to LSN_FILE_MAX_CELLS filters run out of the ring in ONE launch.
 * cfgs[c]: the cell's filter and out_first; antennas, format, scale, rate and in_base are the recording's and must agree.  outs[c]: [n_out[c]][antenna] cf32
 * (host), outs[c][0] = y1[out_first] - lsn_channel_filter's with the same arguments, bit for bit; n_out[c] = 0: the cell takes no part.  Refused
 * (LSN_ERROR_INVALID_INPUTS, the outputs untouched): whatever lsn_channel_filter refuses, n_cells 0 or above LSN_FILE_MAX_CELLS, ring_samples not a power of two
 * or above 2^32, n_in > ring_samples. */
int lsn_channel_filter_ring(int device, const void* in, uint64_t n_in, uint64_t ring_samples, const lsn_channel_filter_cfg_t* cfgs, uint32_t n_cells, float* const* outs,
                            const uint64_t* n_out);
/* in_lo / in_hi: the input samples n_out outputs from out_first read; max_out: outputs from out_first on whose input lies in front of in_end; taps = 2 L + 1.  No GPU. */
int lsn_channel_filter_span(const lsn_channel_filter_cfg_t* cfg, uint64_t n_out, uint64_t in_end, lsn_resample_span_t* out);
/* The stop band of every cell of a recording from its neighbours: S_i = min over j != i of (|f_j - f_i| - B_j), B_j = 15 kHz (6 nof_prb_j + 1), capped at
 * rate_in / 2; 0 (no filter) for a cell without a neighbour or when that is not above B_i.  LSN_ERROR_INVALID_INPUTS when a cell's L would exceed 512. */
int lsn_cells_stopbands(const double* carrier_hz, const uint32_t* nof_prb, uint32_t n, double rate_in_hz, double* stopband_hz);

/* ---- the sample clock of a recording, measured from its PSS train ----
 * A recording made by a radio whose clock is off by eps runs at fs (1 + eps), fs = 15 kHz * N the nominal rate: PSS occurrence q (one every 5 ms, W5 = 75 N
 * nominal samples) starts at p_q = p_0 + q W5 (1 + eps).  lsn_clock_estimate correlates the PSS replica of the cell (rotated by cfo_hz) over a short window
 * of lags around every occurrence (k_pss_track: the expressions of the cell search's matched filter, C(l) = |sum x[l + k] conj r[k]|^2 / sum |x[l + k]|^2),
 * refines every peak by a parabola through its three lags and fits a line through the positions - coarse to fine: round 0 looks at the first 8 periods
 * with windows wide enough for +-max_ppm, every later round at four times as many with windows placed by the previous fit, the last at all of them.
 * The answer goes, as sample_rate_hz and sf_start, into lsn_phy_process_file_rate: lsn_cell_search -> lsn_clock_estimate -> lsn_phy_mib_decode / replay
 * needs no number from the user.  ONE constant eps per recording: nothing is tracked inside the replay; max_residual shows when the drift of a recording
 * is not a line.
 *   windows   round 0: period q < min(Q, 8), centre pss_pos + q W5, half width 4 + ceil(q W5 max_ppm 1e-6); round r >= 1: q < Q_r = min(Q, 4 Q_(r-1)), centre
 *             floor(p0 + q W5 (1 + eps) + 1/2) of the previous fit, half width 4 + ceil(q / (Q_(r-1) - 1)).  Q = the periods whose round-0-style window lies inside
 *             the samples, at most max_periods (0 = 4096); Q < 4: LSN_ERROR_INVALID_INPUTS (pss_pos < 4 leaves no room for the first window: pass pss_pos + W5)
 *   observation  l* = first maximum of C over the window; valid when l* is neither its first nor its last lag; pos = l* + 0.5 (C[l*-1] - C[l*+1]) / (C[l*-1] -
 *             2 C[l*] + C[l*+1]) (double), peak = C[l*]
 *   fit       valid observations with peak >= 0.25 median(peak) (the mean of the two middle ones for an even number); least squares of pos on q; those more than 1.0
 *             sample off the line are dropped and the rest fitted once more; found when the number used is >= 4 and >= half of the observations handed in, and
 *             the rms residual is <= 0.5 sample; eps = slope / W5 - 1, pss_pos0 = intercept.  Fewer than two left to fit: found = 0, nothing else is filled in
 * lsn_clock_plan, lsn_clock_fit and lsn_clock_replica need no GPU. */
typedef struct {
  uint32_t struct_size;   /* sizeof(lsn_clock_cfg_t); every other size is refused */
  uint32_t nof_prb;
  int rates;              /* LSN_RATES_*: N = lsn_symbol_sz(nof_prb, rates) */
  uint32_t n_id_2;        /* lsn_cell_search_t.n_id_2 */
  uint64_t pss_pos;       /* an integer near p_0: lsn_cell_search_t.pss_pos (+ a multiple of 75 N) */
  float cfo_hz;           /* lsn_cell_search_t.cfo_hz: the replica is rotated by it */
  double max_ppm;         /* largest |eps| looked for, 1e-6; 0 < max_ppm <= 1000 (the Python binding's default is 200) */
  uint32_t max_periods;   /* 0 = 4096, the most looked at (20 s) */
  uint32_t sf_start;      /* lsn_cell_search_t.sf_start: only its distance to pss_pos is used (lsn_clock_t.sf_start) */
} lsn_clock_cfg_t;
typedef struct {
  uint32_t period, valid;
  int64_t centre;         /* lags centre - half_width .. centre + half_width */
  uint32_t half_width, reserved;
  double pos;
  float peak;
} lsn_clock_obs_t;
typedef struct {
  uint32_t found, nof_periods /* observations of the last round */, nof_used /* of those in the fit */, nof_rounds;
  double eps;             /* the recording runs at nominal * (1 + eps) */
  double sample_rate_hz;  /* nominal * (1 + eps): lsn_file_rate_t.sample_rate_hz of the replay */
  double pss_pos0;        /* fitted position of occurrence 0 */
  double rms_residual, max_residual;  /* of the observations used, samples */
  double sf_start;        /* pss_pos0 - ((pss_pos - cfg.sf_start) mod 75 N) (1 + eps), + 75 N (1 + eps) while negative: start of a subframe 0 / 5, for
                             lsn_file_cfg_t.offset_time_samples (whole part) and lsn_file_rate_t.offset_time_frac.  It lies a whole number k of half frames
                             (k = round of the difference / 75 N, normally 0) behind the cell search's sf_start: its subframe index is the search's sf_idx + 5 k */
} lsn_clock_t;
/* the windows of round `round` (previous: the fit of round - 1, ignored for round 0) -> number written (period, centre, half_width filled, the rest zero);
 * 0: the previous round was the last; windows == NULL: the number alone; cap too small or a previous fit that was not found: LSN_ERROR_INVALID_INPUTS */
int lsn_clock_plan(const lsn_clock_cfg_t* cfg, uint64_t nof_samples, uint32_t round, const lsn_clock_t* previous, lsn_clock_obs_t* windows, uint32_t cap);
/* fills found, nof_periods = n, nof_used, eps, pss_pos0 and the residuals; returns found */
int lsn_clock_fit(const lsn_clock_obs_t* obs, uint32_t n, uint32_t W5, lsn_clock_t* out);
/* the replica the correlator uses: the unit-energy time-domain PSS of n_id_2 times exp(2 pi j cfo_hz k / fs), formed in double, rounded to float once; out: [N] cf32 */
int lsn_clock_replica(const lsn_clock_cfg_t* cfg, float* out);
/* one round on the GPU: fills pos / peak / valid of the given windows, each of which must lie inside the samples (lags >= 0, lag + N <= nof_samples);
 * corr_out optional (host): the C values window by window.  iq: one antenna, cf32 at the nominal rate, host or device memory */
int lsn_clock_track(int device, const void* iq, int iq_on_device, uint64_t nof_samples, const lsn_clock_cfg_t* cfg, lsn_clock_obs_t* windows, uint32_t n,
                    float* corr_out);
/* all rounds; 1 found, 0 not found (a round's fit failed, or placed a window outside the samples), < 0 error.  obs_out optional: the observations of the last
 * round that ran (cap >= their number, at most the Q of the plan) */
int lsn_clock_estimate(int device, const void* iq, int iq_on_device, uint64_t nof_samples, const lsn_clock_cfg_t* cfg, lsn_clock_t* out, lsn_clock_obs_t* obs_out,
                       uint32_t cap);
/* the same on a recording.  Only the slices the windows read are fetched (pread) - a few MB of a recording of any length.  cf32 / sc16 / sc8 as lsn_file_cfg_t
 * (antenna `antenna` of the interleaved file, counted from cfg->offset_time_samples; offset_freq_hz is not applied); integer samples are converted on the host by
 * the file source's rule, sample = (float)integer * scale.  rate == NULL: the file is nominally at the rate of cfg (nof_prb, rates).  Otherwise every slice comes
 * out of the resampler's plan at the NOMINAL sample_rate_hz / center_offset_hz / offset_time_frac (k_resample, output samples from the first lag of the slice
 * on; lags and pss_pos count output samples, output sample 0 = file position offset_time_samples + offset_time_frac), and the answer's sample_rate_hz =
 * rate->sample_rate_hz * (1 + eps).  sf_start of the answer counts samples of the FILE from its first one (the offset included): directly the offset of the replay. */
int lsn_file_clock_estimate(int device, const char* path, const lsn_file_cfg_t* fcfg, const lsn_file_rate_t* rate, uint32_t antenna, const lsn_clock_cfg_t* cfg,
                            lsn_clock_t* out);

/* ---- the LTE carriers of a wideband recording: carrier scan ----
 * Given the head of a recording and its sample rate, lsn_carrier_scan reports every LTE carrier in it: the offset from the recording's centre in the form
 * lsn_resample_cfg_t.center_offset_hz / lsn_file_rate_t.center_offset_hz take, and the cell search's answer (cell id, CP, subframe timing, CFO) on that carrier.
 *   hypotheses  f_k = (double)k * raster_hz + raster_offset_hz for every integer k with |f_k| + 555 kHz <= rate_in_hz / 2 (555 kHz = 15 kHz * 37, the centre six
 *               resource blocks, which carry PSS, SSS and PBCH of a cell of any bandwidth; the acceptance rule of center_offset_hz), narrowed to f_lo_hz <= f_k
 *               <= f_hi_hz unless both are 0.  None, or more than 8192: LSN_ERROR_INVALID_INPUTS.  The tuning word of f_k is lsn_resample's W of that double.
 *   channel     the resampler of section 3.1b from rate_in_hz to 1.92 MS/s with pass band 555 kHz, output sample 0 at input sample 0, with two limits lifted for
 *               this caller: 1.92e6 <= rate_in_hz <= 122.88e6 (ratio up to 64) and up to 768 taps (382 at 61.44 MS/s, 764 at 122.88 MS/s).  k_chan_bank, one
 *               launch for a batch of hypotheses; a channel sample is a function of (input, configuration, hypothesis, m) only.
 *   metric      per hypothesis the cell search's PSS correlation on its channel (N = 128, 9600 lags, three roots, nof_periods periods added) and its
 *               pss_p2avg: the first maximum in (root, lag) order over the mean of the winning root.
 *   decision    hypotheses with p2avg >= threshold and peak >= threshold * nof_periods / 128 (the mean of the correlation on a white channel: a channel that
 *               holds a strong neighbour only in its transition band has a far lower mean and a large p2avg on nothing), by metric descending (ties: lower |f_k|, then lower k), accepted greedily; one strictly closer than
 *               min_spacing_hz to an accepted one is dropped (a hypothesis a whole number of sub-carriers off a real carrier sees a time-shifted PSS).
 *   verification  lsn_cell_search's algorithm on the channel of every accepted carrier (6 resource blocks, same nof_periods, root free); found is the search's.
 * The head must hold lsn_carrier_scan_plan_t.nof_input_samples samples.  Device scratch for channels and correlations is bounded by 256 MB whatever the number
 * of hypotheses (they are processed in batches).  One antenna is scanned, or all of them: with antenna = LSN_SCAN_ALL_ANTENNAS the bank forms a channel per
 * (hypothesis, antenna), the metric is k_pss_corr_ant's correlation added over the antennas, the decision is unchanged, and the verification is
 * lsn_cell_search_ant on the carrier's nof_antennas channels (a batch holds nof_antennas times the channel memory per hypothesis).  With nof_antennas = 1 that is
 * the scan of antenna 0, bit for bit.  lsn_carrier_scan_plan and lsn_carrier_scan_decide need no GPU. */
#define LSN_SCAN_MAX_HYPOTHESES 8192u
#define LSN_SCAN_ALL_ANTENNAS 0xFFFFFFFFu /* lsn_carrier_scan_cfg_t.antenna: every antenna of the input, combined without their phases */
typedef struct {
  uint32_t struct_size;      /* sizeof(lsn_carrier_scan_cfg_t); every other size is refused */
  uint32_t nof_antennas;     /* interleaved in the input (lsn_file_carrier_scan: taken from lsn_file_cfg_t) */
  uint32_t antenna;          /* the one that is scanned, 0 .. nof_antennas - 1, or LSN_SCAN_ALL_ANTENNAS */
  uint32_t sample_format;    /* LSN_FILE_* (lsn_file_carrier_scan: from lsn_file_cfg_t, as sample_scale) */
  float    sample_scale;
  uint32_t nof_periods;      /* 5 ms periods added, 1..16; 0 = 2.  With the threshold of 20 one period leaves a false alarm in a few percent of the scans of a
                                61.44 MS/s recording, two periods about 1e-9 */
  double   rate_in_hz;       /* rate of the recording, 1.92e6 .. 122.88e6 */
  double   raster_hz;        /* 0 = 100e3, the LTE channel raster */
  double   raster_offset_hz; /* position of a raster point relative to the recording's centre */
  double   f_lo_hz, f_hi_hz; /* both 0: every hypothesis inside the recording; else only f_lo_hz <= f_k <= f_hi_hz */
  double   min_spacing_hz;   /* 0 = 1.4e6, the narrowest LTE channel */
  float    threshold;        /* on p2avg; 0 = 20 */
  uint32_t reserved;
} lsn_carrier_scan_cfg_t;
typedef struct {
  uint32_t nof_hypotheses, taps /* T of the channel filter */, nof_periods, reserved;
  uint64_t nof_channel_samples;  /* (nof_periods + 1) * 9600 + 128 at 1.92 MS/s */
  uint64_t nof_input_samples;    /* the scan reads samples 0 .. nof_input_samples - 1 of the input */
} lsn_carrier_scan_plan_t;
typedef struct {
  int32_t  k;
  uint32_t root;             /* of the peak */
  double   f_hz;             /* f_k */
  uint64_t tuning_word;      /* W of f_k */
  uint32_t lag;              /* of the peak, 0 .. 9599 */
  float    peak, p2avg;
  uint32_t reserved;
} lsn_carrier_metric_t;
typedef struct {
  double   center_offset_hz; /* f_k of the carrier: center_offset_hz of lsn_resample / lsn_phy_process_file_rate / lsn_carrier_channel */
  int32_t  k;
  float    scan_p2avg;       /* the scan's own metric ... */
  uint32_t scan_root, scan_lag;  /* ... and where its peak was */
  lsn_cell_search_t search;  /* the cell search on the carrier's channel; pss_pos and sf_start count samples of the 1.92 MS/s channel */
} lsn_carrier_t;
/* the hypotheses (k, f_hz, tuning_word filled, the rest zero; hyp optional, cap >= their number), the bank of the channel filter (optional: [512][taps][2] floats,
 * H[p][j] and H[p + 1][j] - H[p][j]) and what the scan reads */
int lsn_carrier_scan_plan(const lsn_carrier_scan_cfg_t* cfg, lsn_carrier_scan_plan_t* out, lsn_carrier_metric_t* hyp, uint32_t cap, float* bank_out);
/* the decision on n metrics -> number accepted; accepted_out: their indices into metric in the order of acceptance (the first cap of them) */
int lsn_carrier_scan_decide(const lsn_carrier_scan_cfg_t* cfg, const lsn_carrier_metric_t* metric, uint32_t n, uint32_t* accepted_out, uint32_t cap);
/* in: [sample][antenna] in sample_format, in[0] = sample 0 of the recording, host or device memory.  Returns the number of carriers (the first cap of them in
 * carriers_out, in the order of acceptance), < 0 on error.  metric_out optional: one entry per hypothesis (lsn_carrier_scan_plan_t.nof_hypotheses) */
int lsn_carrier_scan(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_carrier_scan_cfg_t* cfg, lsn_carrier_t* carriers_out, uint32_t cap,
                     lsn_carrier_metric_t* metric_out);
/* the same on a recording: only the head the scan needs is read (pread), from fcfg->offset_time_samples on - that sample is sample 0 of the scan.  nof_antennas,
 * sample_format and sample_scale are fcfg's (cf32 / sc16 / sc8 by the file source's rule); offset_freq_hz is not applied.  A file shorter than the head:
 * LSN_ERROR_INVALID_INPUTS */
int lsn_file_carrier_scan(int device, const char* path, const lsn_file_cfg_t* fcfg, const lsn_carrier_scan_cfg_t* cfg, lsn_carrier_t* carriers_out, uint32_t cap,
                          lsn_carrier_metric_t* metric_out);
/* The 1.92 MS/s channel of one offset, all antennas: out [antenna][n_out] cf32, out[0] = output sample out_first; output sample 0 sits at first_sample + first_frac,
 * in[0] = sample in_base of the recording (fields as lsn_resample_cfg_t).  With first_sample = 0 and first_frac = 0 these are, bit for bit, the samples the scan
 * correlated for that offset - what lsn_phy_mib_decode on a six-block Phy needs.  Pieces, batches and call boundaries change no bit. */
typedef struct {
  uint32_t struct_size;      /* sizeof(lsn_carrier_channel_cfg_t); every other size is refused */
  uint32_t nof_antennas;
  uint32_t sample_format;
  float    sample_scale;
  double   rate_in_hz, center_offset_hz;
  uint64_t first_sample;
  double   first_frac;
  uint64_t in_base, out_first;
} lsn_carrier_channel_cfg_t;
int lsn_carrier_channel(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_carrier_channel_cfg_t* cfg, float* out, int out_on_device,
                        uint64_t n_out);
int lsn_carrier_channel_span(const lsn_carrier_channel_cfg_t* cfg, uint64_t n_out, uint64_t in_end, lsn_resample_span_t* out);

/* ---- security-API sink (the step behind the path: PDSCH_Decoder::run_api_dl_mode, DL_Sniffer_PDSCH.cc:804-879) ----
 * api_mode as ArgManager's -a (ArgManager.cc:63,218): -1 off (default), 0 identity mapping, 2 IMSI catching, 3 all.  For every CRC-ok
 * downlink block the writer thread reports, in record order: paging records (modes 2, 3; decode_imsi_tmsi_paging :84-127: IMSI as 15
 * digits, S-TMSI as 8 hex digits of the m-TMSI, rnti 65534) and the contention resolution identity next to an RRCConnectionSetup
 * (modes 0, 3; :813-877: characters 3..10 of the identity printed in hex).  In UL_MODE a decoded Msg3 (PUSCH of a RAR grant) reports the
 * initial UE identity of its RRCConnectionRequest (modes 0, 3; UL_Sniffer_PUSCH.cc:47-93,306-327: m-TMSI in hex, or the last eight hex
 * digits of the random value - the same characters the connection setup reports); every other decoded uplink block is read as SRB
 * traffic (modes 1-3; :95-247,328-372: MAC / RLC AM / PDCP walk, UL-DCCH head, NAS): UECapabilityInformation (modes 1, 3: id_type
 * 0xFFFFFFFF, value "-"), attach request and identity response identities (modes 2, 3: IMSI / IMEI / IMEISV digits, m-TMSI of a GUTI).
 * Blocks that produced an identity are also written to api_pcap (write_dl_paging_api / write_dl_crnti_api / write_ul_crnti_api,
 * PcapWriter.cc:120-145,177-190) when it is not NULL.
 * Not covered: RRCConnectionReconfiguration / NAS identities of the downlink (LCID 1, :837-850); the body of a UECapabilityInformation is
 * not unpacked. */
typedef struct {
  uint32_t tti; uint16_t rnti;
  uint32_t id_type;   /* Sniffer_dependency.h:42-47: 0 ID_RAN_VAL, 1 ID_TMSI, 2 ID_CON_RES, 3 ID_IMSI, 4 ID_IMEI, 5 ID_IMEISV, 0xFFFFFFFF none */
  uint32_t msg_type;  /* Sniffer_dependency.h:49-55: 0 MSG_CON_REQ, 1 MSG_CON_SET, 2 MSG_ATT_REQ, 3 MSG_ID_RES, 4 MSG_UE_CAP, 5 MSG_PAGING, 6 MSG_CON_RECONFIG (M-TMSI of the GUTI an attach accept inside an RRCConnectionReconfiguration assigns) */
  char value[24];     /* the string print_api_dl receives */
} lsn_api_event_t;
typedef void (*lsn_api_sink_t)(void* user, const lsn_api_event_t* ev);
int lsn_phy_set_api_mode(lsn_phy_t* phy, int api_mode, lsn_api_sink_t cb, void* user, lsn_pcap_t* api_pcap);

/* ---- uplink (PUSCH) ----
 * lsn_phy_set_ul_config replaces srsran_enb_ul_set_cell(&enb_ul, cell, &ul_cfg.dmrs, ...) (SubframeWorker.cc:258-262); the two
 * values come from SIB2 (ULSchedule::set_config, ULSchedule.cc:140-158: cyclicShift, groupAssignmentPUSCH).
 * lsn_phy_pusch_decode runs srsran_enb_ul_fft + srsran_chest_ul_estimate_pusch + srsran_pusch_decode
 * (UL_Sniffer_PUSCH.cc:392,256,262) for a whole list of grants on n_subframes of the uplink antenna.
 * Round-1 scope: one antenna, no group/sequence hopping, type-1 frequency hopping only (type 2 grants come back with crc_ok = 0), no SRS, L_prb >= 3 of the 2^a3^b5^c set; control information on the
 * PUSCH is located and skipped / erased, not decoded
 * (UL_Sniffer_PUSCH.cc:3-10); any other grant comes back with crc_ok = 0. */
typedef struct {
  uint32_t cyclic_shift;    /* SIB2 cyclicShift */
  uint32_t delta_ss;        /* SIB2 groupAssignmentPUSCH */
  uint32_t hopping_offset;  /* SIB2 pusch-HoppingOffset (ul_cfg.hopping.n_rb_ho, SubframeWorker.cc:271-273): second-slot position of type-1 hopping grants */
  uint32_t group_hopping_enabled;     /* SIB2 ul-ReferenceSignalsPUSCH.groupHoppingEnabled (ULSchedule.cc:143-146): sequence group per slot, 36.211 5.5.1.3 */
  uint32_t sequence_hopping_enabled;  /* ... sequenceHoppingEnabled: base sequence number per slot for >= 6 PRB, 36.211 5.5.1.4 */
} lsn_ul_cfg_t;
typedef struct {
  uint32_t sf;       /* subframe index inside ul_iq (tti = start_tti + sf) */
  uint16_t rnti;
  uint16_t n_dmrs;   /* cyclic shift field of DCI 0 (0 for a RAR grant) */
  uint32_t n_prb, L_prb;
  uint32_t mod;      /* bits per symbol: 2, 4, 6, 8 */
  uint32_t tbs;      /* bits */
  int rv;
  /* control information multiplexed into the PUSCH (TS 36.212 5.2.2.6-8), located so that the UL-SCH bits are de-multiplexed
   * correctly; the reference's settings are UL_Sniffer_PUSCH.cc:429-450 with the offsets I_ack = 10, I_cqi = 8, I_ri = 11 of
   * MCSTracking.cc:1534-1538 */
  uint32_t nof_ack;  /* HARQ-ACK bits 0..2 (uci_cfg.ack[0].nof_acks) */
  uint32_t cqi_bits; /* size of the CQI report, 0 = none (aperiodic request: wideband 4, UE-selected sub-band 5, higher-layer sub-band 4 + 2 N) */
  uint32_t ri_bits;  /* rank indication bits (1 with a CQI request) */
  uint32_t hop;      /* 0: both slots on n_prb; 1: type-1 frequency hopping, slot 1 starts at n_prb_slot1 (36.213 8.4.1) */
  uint32_t n_prb_slot1;
  /* 1 + betaOffset-ACK-Index / betaOffset-CQI-Index / betaOffset-RI-Index of the UE (ul_cfg.pusch.uci_offset = ue_config.uci_config,
   * UL_Sniffer_PUSCH.cc:433-435; 36.213 Tables 8.6.3-1/-2/-3); 0 = the reference's defaults 10 / 8 / 11.  A reserved index makes the
   * grant undecodable (crc_ok = 0). */
  uint32_t beta_offset_ack_idx_p1, beta_offset_cqi_idx_p1, beta_offset_ri_idx_p1;
} lsn_pusch_grant_t;
typedef struct { uint32_t crc_ok; uint32_t iterations; float snr_db; uint32_t payload_off; } lsn_pusch_result_t;
int lsn_phy_set_ul_config(lsn_phy_t* phy, const lsn_ul_cfg_t* cfg);
/* The SIB2 fields the sniffer reads (ULSchedule::set_config, ULSchedule.cc:140-158; SubframeWorker.cc:271-273). */
typedef struct {
  uint32_t n_sb, hopping_mode, pusch_hop_offset, enable_64qam;                                                  /* pusch-ConfigBasic */
  uint32_t group_hopping_enabled, group_assignment_pusch, sequence_hopping_enabled, cyclic_shift;                /* ul-ReferenceSignalsPUSCH */
  uint32_t root_seq_idx, prach_config_idx, high_speed_flag, zero_corr_zone, prach_freq_offset;                   /* prach-Config */
} lsn_sib2_t;
/* ULSchedule::get_config / getSIB2 (ULSchedule.h:90-93, DL_Sniffer_PDSCH.h:137): in UL_MODE without lsn_phy_set_ul_config the commit stage
 * runs PDSCH_Decoder::decode_SIB (DL_Sniffer_PDSCH.cc:459-560) on every subframe until a SystemInformation with SIB2 decodes, writes
 * that one SI-RNTI record, configures DMRS / hopping offset / PRACH detector from it and decodes PUSCH from the next subframe on.
 * Returns 1 when an uplink configuration is in use (ul filled; *from_sib2 = 1 and sib2 filled when it was learned from SIB2), else 0.
 * Any output pointer may be NULL.  Call between lsn_phy_wait and the next submit. */
int lsn_phy_get_ul_config(lsn_phy_t* phy, lsn_ul_cfg_t* ul, lsn_sib2_t* sib2, uint32_t* from_sib2);
/* BCCH-DL-SCH-Message -> SIB2 (the parser behind decode_SIB): 0 = does not unpack, 1 = unpacks without SIB2 in front, 2 = SIB2 (out filled) */
int lsn_sib2_decode(const uint8_t* pdu, uint32_t len, lsn_sib2_t* out);
/* ul_iq: [n_subframes][15*N] interleaved cf32 of the uplink antenna, host memory (iq_on_device = 0) or device memory (1).
 * payloads (may be NULL): decoded transport blocks, tbs/8 bytes each at results[i].payload_off. */
int lsn_phy_pusch_decode(lsn_phy_t* phy, const void* ul_iq, int iq_on_device, uint32_t n_subframes, uint32_t start_tti,
                         const lsn_pusch_grant_t* grants, uint32_t n_grants, lsn_pusch_result_t* results, uint8_t* payloads, size_t payload_cap);
/* Read-only taps of the last lsn_phy_pusch_decode / lsn_phy_prach_detect call; returns the bytes written.  what = 0: uplink grid of subframe `index`,
 * 1: rate-matched LLRs of grant `index`, 2: PRACH correlation power of occasion `index`, 3: the code blocks of grant `index` in transport-block order, six
 * uint32 each (K, F, E, rv, ok, iters), 4: for the same blocks in the same order the K + 12 words the rate de-matcher handed to the turbo decoder,
 * 5: the private grid rows of grant `index` ([14 or 12 symbols][12 nof_prb] cf32) when the last lsn_phy_pusch_decode ran with lsn_phy_set_ul_timing mode 2:
 * the grant's symbols cut again `shift` samples earlier, or a copy of the common rows when its shift is 0; LSN_ERROR_INVALID_INPUTS in the other modes. */
long lsn_phy_tap_ul(lsn_phy_t* phy, int what, uint32_t index, void* out, size_t cap);

/* ---- uplink arrival time ----
 * A UE transmits its timing advance ahead of its own downlink, so at a sniffer that does not stand at the eNB its subframe arrives EARLY by
 * (d_eNB-UE + d_eNB-sniffer - d_UE-sniffer) / c: between 0 and the UE's full timing advance, never late.  The cyclic prefix protects against late arrival
 * only; an arrival a samples ahead of the common SC-FDMA window puts a samples of the next symbol into it (ISI floor about N / 2a) and a phase ramp of
 * 2 pi a / N per carrier under the three-tap smoother of the channel estimate.  This is the reference's chest_res.ta_us ("DL-UL_delay" of its uplink table).
 * mode 0 (the default): off - lsn_phy_pusch_decode and UL_MODE issue exactly the launches they issue without this call.
 * mode 1: measure.  One more launch per decode call; per grant tau = arg(sum_n ls[n+1] conj(ls[n])) N / 2 pi over the least-squares estimates of both
 *         reference-signal symbols, in samples at the cell's rate, positive = early.  Every other result is bit for bit that of mode 0.
 * mode 2: measure and re-window.  shift = round(tau), clamped to [-late_max, +max_advance], 0 when |shift| < min_shift; a grant with a shift is demodulated
 *         again with every symbol cut `shift` samples earlier, into grid rows of its own, and estimated, equalised and decoded from those; a grant with
 *         shift 0 comes out bit for bit as in mode 0.  snr_db of lsn_pusch_result_t is that of the re-cut symbols.  Decided per grant on the device,
 *         nothing is remembered between subframes.  In UL_MODE the uplink antenna of the chunk is the source.
 * min_shift: 0 = N / 128 (at least 1).  max_advance: 0 = N / 4; at most N / 2.  late_max is the normal cyclic prefix, 144 N / 2048.
 * The zero rule: a sample in front of the grant's own subframe, or behind its end, reads as zero in the second window, in every subframe - a result never
 * depends on where a call or a chunk begins.  A shift above the first cyclic prefix (160 N / 2048) therefore costs the start of symbol 0.
 * Limits: one arrival per grant, measured on that grant alone; a UE whose neighbours in frequency arrive at other times sees their leakage (the
 * orthogonality is lost), which is not cancelled; PRACH and the downlink are untouched.
 * Returns LSN_ERROR_INVALID_INPUTS for a null pointer, mode > 2, max_advance > N / 2 or min_shift > N / 2; LSN_ERROR before a cell is set and while
 * submitted blocks are in flight (call lsn_phy_wait first).  Nothing changes on a refusal. */
typedef struct { uint32_t mode, min_shift, max_advance; } lsn_ul_timing_cfg_t;
#define LSN_TOA_FLAG_CLAMPED 1u   /* round(tau) lay outside [-late_max, +max_advance] */
#define LSN_TOA_FLAG_BELOW 2u     /* |shift| < min_shift: shift = 0 */
typedef struct {
  uint32_t measured;  /* 1: the fields below are filled (a grant that was decoded in mode 1 / 2), 0: all zero */
  float tau;          /* samples, positive = early */
  int32_t shift;      /* the decision (also reported in mode 1, where nothing is moved) */
  uint32_t flags;     /* LSN_TOA_FLAG_* */
  float residual;     /* mode 2 with a sample source: tau measured again on the re-cut symbols; else 0 */
  float toa_us;       /* the arrival in microseconds: (shift + residual) after a re-cut, else tau, times 1 / (15000 N) */
  float confidence;   /* |z| / sum |ls|^2 */
} lsn_pusch_timing_t;
int lsn_phy_set_ul_timing(lsn_phy_t* phy, const lsn_ul_timing_cfg_t* cfg);
/* per grant of the last lsn_phy_pusch_decode, in the caller's grant order: min(cap, n_grants) records are written, n_grants is returned */
long lsn_phy_get_pusch_timing(lsn_phy_t* phy, lsn_pusch_timing_t* out, uint32_t cap);
/* The decision without a GPU (what k_pusch_toa computes from tau): N = symbol length of the cell (128 .. 2048), cfg as for lsn_phy_set_ul_timing (mode
 * is not read).  Ties of round() go to the even integer.  Returns LSN_SUCCESS, or LSN_ERROR_INVALID_INPUTS (null pointer, N out of range, max_advance or
 * min_shift above N / 2). */
int lsn_pusch_toa_decide(float tau, uint32_t N, const lsn_ul_timing_cfg_t* cfg, int32_t* shift, uint32_t* flags);
/* UL_MODE only (else LSN_ERROR_INVALID_INPUTS): the row of the reference's uplink table for one RNTI (MCSTracking.cc:441-472) - modulation class, counted
 * (active) and successful decodes, mean SNR and mean arrival ("DL-UL_delay") over the counted decodes.  Updated where update_statistic_ul is, behind the
 * same SNR gate, with the values of the last attempt that ran; dropped with the RNTI's database entry.  In mode 0 the arrival fields are 0 and
 * measured = 0.  Returns 1 when the RNTI has an entry (out filled), 0 when not.  Call between lsn_phy_wait and the next submit. */
typedef struct { uint32_t mod, active, success; float mean_snr_db; uint32_t measured; float mean_toa_us, mean_toa_samples; } lsn_ul_ue_stats_t;
int lsn_phy_get_ul_ue_stats(lsn_phy_t* phy, uint16_t rnti, lsn_ul_ue_stats_t* out);

/* ---- uplink (PRACH) ----
 * lsn_phy_set_prach_config replaces PUSCH_Decoder::set_rach_config (UL_Sniffer_PUSCH.cc:640-653: srsran_prach_init,
 * srsran_prach_set_cfg, srsran_prach_set_detect_factor(60)); the fields are SIB2's prach-ConfigInfo as the reference copies
 * them in ULSchedule::set_config (ULSchedule.cc:149-154).  lsn_phy_prach_detect replaces PUSCH_Decoder::work_prach
 * (UL_Sniffer_PUSCH.cc:656-713: srsran_prach_tti_opportunity + srsran_prach_detect_offset on one uplink subframe) for a
 * block of uplink subframes.  Scope: preamble format 0 (config_idx 0..15, the format that fits the one subframe the
 * reference hands over), unrestricted cyclic shifts (hs_flag = 0); anything else is LSN_ERROR_INVALID_INPUTS.
 * The logical->physical root map (TS 36.211 Table 5.7.2-4, srsRAN's prach_zc_roots[838]) is passed in by the caller;
 * with zc_roots = NULL the numbers root_seq_idx + i (+1) are used as physical roots.
 * In UL_MODE (sniffer_mode = 1) a configured detector also runs on the uplink antenna of every processed PRACH occasion
 * and reports through the sink (the reference prints the strongest preamble there). */
typedef struct {
  uint32_t config_idx;       /* prach-ConfigIndex */
  uint32_t root_seq_idx;     /* rootSequenceIndex 0..837 */
  uint32_t zero_corr_zone;   /* zeroCorrelationZoneConfig 0..15 */
  uint32_t freq_offset;      /* prach-FreqOffset: first of the 6 PRBs */
  uint32_t hs_flag;          /* highSpeedFlag, must be 0 */
  float detect_factor;       /* peak / mean threshold, 0 = 60 (UL_Sniffer_PUSCH.cc:651) */
  const uint16_t* zc_roots;  /* 838 entries or NULL (only read during the call) */
} lsn_prach_cfg_t;
typedef struct {
  uint32_t sf;        /* subframe index inside the block (tti = start_tti + sf) */
  uint32_t preamble;  /* 0..63 */
  uint32_t offset;    /* peak lag inside the cyclic-shift window, units of T_SEQ / 839 */
  float offset_sec;   /* the same in seconds (srsran_prach_detect_offset's t_offsets) */
  float p2avg;        /* peak / mean correlation power */
} lsn_prach_det_t;
typedef void (*lsn_prach_sink_t)(void* user, uint32_t tti, const lsn_prach_det_t* det, uint32_t n_det);
int lsn_phy_set_prach_config(lsn_phy_t* phy, const lsn_prach_cfg_t* cfg);
/* returns the number of detections written to out (<= cap), in (subframe, root, cyclic shift) order, or < 0 */
int lsn_phy_prach_detect(lsn_phy_t* phy, const void* ul_iq, int iq_on_device, uint32_t n_subframes, uint32_t start_tti, lsn_prach_det_t* out,
                         uint32_t cap);
void lsn_phy_set_prach_sink(lsn_phy_t* phy, lsn_prach_sink_t cb, void* user);
int lsn_prach_tti_opportunity(uint32_t config_idx, uint32_t tti); /* srsran_prach_tti_opportunity(p, tti, -1), format 0 */

/* ---- measurement + parity taps (not part of the reference surface) ---- */
enum { LSN_TAP_GRID = 0, LSN_TAP_CE = 1, LSN_TAP_PDCCH_LLR = 2, LSN_TAP_CHEST = 3, LSN_TAP_CFI = 4, LSN_TAP_CANDIDATES = 5,
       LSN_TAP_CCE_POWER = 6, LSN_TAP_ACCEPTED = 7, LSN_TAP_RB_POWER = 8,
       /* (LSN_TAP_CANDIDATES: [160 locations][8 sizes] of {u64 payload bits, u32 CRC remainder, u32 flags}; with candidate pruning on, a slot the blind decoder left
        * out and the search never asked for has flags = 0x80 - lsn_phy_set_candidate_pruning(phy, 0) gives the exhaustive table) */
       /* stage C (a14, srsran_ue_dl_decode_pdsch as called at DL_Sniffer_PDSCH.cc:997,1110,1207): retained only for batches processed after
        * lsn_phy_set_stage_c_taps(phy, 1) - the arenas of a decode launch are recycled otherwise.  For these the index argument of lsn_phy_tap
        * is the DECODE JOB of the chunk (one job = one decode call of one accepted DCI with one MCS table), not a subframe. */
       LSN_TAP_PDSCH_JOBS = 9,    /* lsn_tap_job_t of every job of the chunk (index ignored) */
       LSN_TAP_PDSCH_LLR16 = 10,  /* descrambled int16 soft bits of the job: codeword 0 (nof_re x Qm), then codeword 1 */
       LSN_TAP_RM_WORDS = 11,     /* per code block (TB 0 blocks, then TB 1), K + 12 u32: the de-rate-matched block as k_rm hands it to k_turbo - word
                                     (x % W) P + x / W = d0[x] | d1[x] << 10 | d2[x] << 20 (10-bit two's complement), P = windows, W = K / P; words K + 4 s + j =
                                     stream s at position K + j (int32) */
       LSN_TAP_CB_RESULT = 12 };  /* lsn_tap_cb_t per code block, same order */
typedef struct { uint32_t sf, tti, rnti, nof_re, qm[2], llr_len[2], tbs[2], crc[2], ncb, have, done; float p_a_db; } lsn_tap_job_t;
typedef struct { uint32_t tb, K, F, E, rv, ok, iters, skipped; } lsn_tap_cb_t;  /* skipped: not decoded because the first block of its TB had failed */
/* copies tap `what` of subframe `sf_in_batch` of the LAST processed batch into out (host); returns bytes written or <0 */
long lsn_phy_tap(lsn_phy_t* phy, int what, uint32_t sf_in_batch, void* out, size_t cap);
int lsn_phy_set_stage_c_taps(lsn_phy_t* phy, int enable);
/* lsn_phy_mib_decode + the 480 raw (not descrambled) PBCH soft bits of the subframe */
int lsn_phy_mib_decode_llr(lsn_phy_t* phy, const void* iq, int iq_on_device, lsn_mib_t* out, float* llr_raw480);
/* the same decode - the same launches, the same result and soft bits (llr_raw480 may be null) - on a one-subframe scratch of its own (allocated on first use) and
 * a stream of its own: allowed while submitted blocks are in flight, where lsn_phy_mib_decode, which borrows a slot of the pipeline, refuses */
int lsn_phy_mib_decode_side(lsn_phy_t* phy, const void* iq, int iq_on_device, lsn_mib_t* out, float* llr_raw480);
typedef struct {
  double ms_stage_a, ms_search, ms_stage_c, ms_commit, ms_total; /* wall clock of the last process call */
  double kernel_ms[16];                                          /* HIP-event time per kernel class, last call */
  uint64_t kernel_launches[16];
  uint64_t algo_bytes;        /* algorithmic HBM bytes of the last call (SURVEY.md 8d formula) */
  uint64_t turbo_algo_bytes;  /* part of algo_bytes moved by the turbo kernels */
  uint64_t turbo128_algo_bytes; /* ... of which by k_turbo<128> */
  uint64_t nof_tb_decodes, nof_cb_decodes, nof_turbo_iterations, nof_candidates_decoded, nof_ondemand_decodes, nof_pdus;
  double ms_search_core;      /* part of ms_search inside the FALCON decision tree proper */
  double ms_rar;              /* part of ms_search spent waiting for on-demand RAR decodes */
  uint64_t turbo_cyc_rm, turbo_cyc_map, turbo_cyc_out;  /* shader cycles summed over code blocks: rate-dematch / MAP iterations / output */
  double ms_wait_front, ms_wait_slot, ms_drain;          /* search thread waiting for stage A / front thread waiting for a free chunk slot / final wait for the commits */
  uint64_t nof_turbo_iterations_run;                     /* iterations executed (equals nof_turbo_iterations) */
  uint64_t nof_ondemand_commit[4];                       /* decodes created at commit: [0] p-a changed, [1] table known at commit but unknown when planned or vice versa, [2] no job planned at all, [3] other */
  double ms_ondemand_commit;                             /* commit-thread time inside those decodes */
  uint64_t nof_pusch_2prb_skipped;                       /* (always 0 since round 3: 2-PRB grants are decoded) */
  uint64_t nof_pusch_on_unverified_dmrs;                 /* UL_MODE: PUSCH attempts on 1- / 2-PRB allocations, whose reference signals come from the restated (structure-checked, not text-verified) 36.211 Tables 5.5.1.2-1 / -2 */
  uint64_t nof_tb_on_derived_tbs;                        /* transport-block decodes whose size came from the DERIVED TBS rows I_TBS 27..33 (spec/gen_tables.py): a real capture that fails exactly there points at the table */
  uint64_t nof_decode_jobs, nof_decode_jobs_used, nof_speculative_jobs;  /* PDSCH decode calls run / of those the commit stage consumed (what the reference would have run) / run ahead only because the
                                                            RNTI's table might be known by commit time (second-table attempt although the first one passed a CRC) */
  /* decode jobs by why they were run: [0] first attempt of the plan, [1] second-table attempt after the first failed on every TB, [2] second-table attempt run
   * ahead although the first passed a CRC (speculative), [3] RA-RNTI candidates decoded ahead of the search, [4] decoded on demand (search / commit turn);
   * jobs / turbo iterations run, and the part of both the commit stage never looked at */
  uint64_t jobs_by_kind[5], jobs_unused_by_kind[5], iters_by_kind[5], iters_unused_by_kind[5];
  uint64_t nof_table_hints_used, nof_table_hints_missed;  /* DCIs planned for the 256QAM table alone on the decode threads' own evidence / of those the commit wanted the 64QAM-table attempt of after all (engine totals) */
  uint64_t nof_candidate_misses;  /* slots of the candidate table the blind decoder had left out (lsn_phy_set_candidate_pruning) and the search had decoded on demand */
  double ms_harq[3];              /* harq_mode = 1, commit-thread time: [0] predicting the retransmissions of the chunks (harqScout), [1] inside the batches (descriptors, launches, wait), [2] bringing the touched buffers home at the end of the turns */
  uint64_t nof_harq_combines[4];  /* harq_mode = 1: [0] batches of retransmissions combined and decoded ahead of the commit walk, [1] combined decodes the walk took from a batch, [2] ... it had to run alone inside its turn, [3] batch results nobody asked for */
} lsn_perf_t;
int lsn_phy_get_perf(lsn_phy_t* phy, lsn_perf_t* out);
enum { LSN_K_OFDM = 0, LSN_K_CHEST, LSN_K_CHEST_FIN, LSN_K_PCFICH, LSN_K_PDCCH_LLR, LSN_K_CCE_POWER, LSN_K_VITERBI,
       LSN_K_PDSCH_PREP, LSN_K_PDSCH_DEMOD, LSN_K_TURBO, LSN_K_RB_POWER, LSN_K_TURBO128, LSN_K_RM, LSN_K_COUNT };
/* LSN_K_TURBO = k_turbo<64> (one wavefront per code block), LSN_K_TURBO128 = k_turbo<128> (two), LSN_K_RM = k_rm (rate de-matching in front of both) */
const char* lsn_kernel_name(int k);
const char* lsn_version(void);

#ifdef __cplusplus
}
#endif
#endif
